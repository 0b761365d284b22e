"""Model construction exactly as the reference drivers do it
(train_video_segment_point.py:323-363, test_video_segment_point.py:69-100):

    lang_model = BertHugface(pretrain_stage=False)
    vision_model = Resnet50TSM(segments_size=clip_frame_num, shift_div=8, pretrain_stage=False)
    model = TwoStream(lang_model.base_model, vision_model.base_model, lang_model.embed_size,
                      vision_model.feature_dim, clip_frame_num, hidden_size=128)
    model.build_chapter_head(output_size=2, head_type=head_type)
"""
import contextlib
import io

from . import synth


def build_mlm_model(seed=None, device=None, precision="bf16", dropout=None):
    """The pre-training driver's model (pretrain_lang_model_hugface.py:237): BertHugface() with its vocabulary head."""
    from model.lang.bert_hugface import BertHugface
    from vcg_hip.nn import BertConfig
    cfg = BertConfig(output_attentions=True)
    if dropout is not None:
        cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = dropout
    with contextlib.redirect_stdout(io.StringIO()):
        model = BertHugface(pretrain_stage=True, config=cfg)
    if device is not None:
        model = model.to(device)
    if seed is not None:
        synth.init_params(model, seed)
    model.precision = precision
    return model


def build_gpt_model(seed=None, device=None, precision="bf16", dropout=None, config=None, checkpoint=None):
    """The generative pre-training driver's model (pretrain_lang_model_hugface.py:234, model_type "gpt"): GPTHugface()
    with its vocabulary head. With a seed every parameter is seeded by name; checkpoint (or $VCG_GPT_CHECKPOINT): a
    local HF openai-gpt state dict for the decoder, loaded AFTER the seeding."""
    import os
    from model.lang.gpt_hugface import GPTHugface
    from vcg_hip.nn import OpenAIGPTConfig
    cfg = config if config is not None else OpenAIGPTConfig()
    if dropout is not None:
        cfg.resid_pdrop = cfg.embd_pdrop = cfg.attn_pdrop = dropout
    with contextlib.redirect_stdout(io.StringIO()):
        model = GPTHugface(config=cfg, checkpoint=checkpoint)
    if device is not None:
        model = model.to(device)
    if seed is not None:
        synth.init_params(model, seed)
        ckpt = checkpoint or os.environ.get("VCG_GPT_CHECKPOINT")
        if ckpt:  # (the seeding covered every parameter: the constructor's load is applied again)
            model.load_checkpoint(ckpt)
    model.precision = precision
    return model


def load_lang_pretrain(bert, path):
    """The hand-off of train_video_segment_point.py:326-330: the language model starts from the masked-LM stage's
    checkpoint (pretrain_lang_model_hugface.py's checkpoint["model_state_dict"], a BertHugface state dict with its
    vocabulary head). `bert` is the scorer's BertModel; its weights become the checkpoint's base_model.*, strictly."""
    import torch
    sd = torch.load(path, map_location="cpu", weights_only=True)["model_state_dict"]
    V, H = bert.config.vocab_size, bert.config.hidden_size
    if "head.weight" not in sd or tuple(sd["head.weight"].shape) != (V, H):
        raise ValueError(f"{path}: not a masked-LM pre-training checkpoint (no [{V}, {H}] head.weight)")
    pre = "base_model."
    bert.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)


def build_contrast_model(seed=None, device=None, precision="bf16", dropout=None, K=65536, copy_key=True, m=0.999,
                         T=0.07, config=None):
    """The contrastive pre-training driver's model (train_lang/pretrain_constrast_lang_model.py:207):
    BertHugfaceConstrast(K, m, T). With a seed every parameter and the queue are seeded by name; copy_key (the
    reference's state: both encoders start from the same weights) copies encoder_q into encoder_k afterwards, False
    leaves the two seeded differently (tests: a mix-up of the encoders then shows)."""
    import torch
    from model.lang.bert_hugface_constrast import BertHugfaceConstrast
    from vcg_hip.nn import BertConfig
    cfg = config if config is not None else BertConfig()
    if dropout is not None:
        cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = dropout
    with contextlib.redirect_stdout(io.StringIO()):
        model = BertHugfaceConstrast(K=K, m=m, T=T, config=cfg)
    if device is not None:
        model = model.to(device)
    if seed is not None:
        synth.init_params(model, seed)
        with torch.no_grad():
            synth.fill(model.queue, synth.KIND_NORMAL, synth.key_of(seed, "queue"), 0.0, 1.0)
            model.queue.copy_(torch.nn.functional.normalize(model.queue, dim=0))
            if copy_key:
                model.encoder_k.load_state_dict(model.encoder_q.state_dict())
    model.precision = precision
    return model


def load_contrast_pretrain(bert, path):
    """The contrastive stage's hand-off: `path` is pretrain_constrast_lang_model.py's checkpoint, a bare
    BertHugfaceConstrast state dict (encoder_q.*, encoder_k.*, queue, queue_ptr). `bert` is the scorer's BertModel; its
    weights become the checkpoint's encoder_q.*, strictly. Anything else (the masked-LM stage's checkpoint, say) is a
    ValueError."""
    import torch
    sd = torch.load(path, map_location="cpu", weights_only=True)
    pre = "encoder_q."
    if not isinstance(sd, dict) or "queue" not in sd or not any(k.startswith(pre) for k in sd):
        raise ValueError(f"{path}: not a contrastive pre-training checkpoint (no queue / encoder_q.* entries)")
    bert.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)


def build_listnet_model(seed=None, device=None, precision="bf16", dropout=None, config=None):
    """The listwise driver's model (train_lang/train_listwise.py:274-279): bert_hugface_listnet.BertHugface(
    pretrain_stage=False) with build_chapter_head(). With a seed every parameter (surrogate_head included) is seeded by
    name."""
    from model.lang.bert_hugface_listnet import BertHugface
    from vcg_hip.nn import BertConfig
    cfg = config if config is not None else BertConfig(output_attentions=True)
    if dropout is not None:
        cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = dropout
    with contextlib.redirect_stdout(io.StringIO()):
        model = BertHugface(pretrain_stage=False, config=cfg)
    model.build_chapter_head()
    if device is not None:
        model = model.to(device)
    if seed is not None:
        synth.init_params(model, seed)
    model.precision = precision
    return model


def load_listnet_pretrain(bert, path):
    """The listwise stage's hand-off: `path` is train_lang/train_listwise.py's checkpoint, a bare
    bert_hugface_listnet.BertHugface state dict (base_model.*, head.* [2, H], surrogate_head.*). `bert` is the scorer's
    BertModel; its weights become the checkpoint's base_model.*, strictly. Anything else (the masked-LM or the
    contrastive stage's checkpoint, say) is a ValueError."""
    import torch
    sd = torch.load(path, map_location="cpu", weights_only=True)
    H = bert.config.hidden_size
    hw = sd.get("head.weight") if isinstance(sd, dict) else None
    if hw is None or "surrogate_head.weight" not in sd or not hasattr(hw, "shape") or tuple(hw.shape) != (2, H):
        raise ValueError(f"{path}: not a listwise fine-tuning checkpoint (no surrogate_head.weight / [2, {H}] "
                         f"head.weight)")
    pre = "base_model."
    bert.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)


def _load_lang(bert, lang_pretrain_ckpt, lang_contrast_ckpt, lang_listnet_ckpt=None):
    if sum(bool(c) for c in (lang_pretrain_ckpt, lang_contrast_ckpt, lang_listnet_ckpt)) > 1:
        raise ValueError("lang_pretrain_ckpt, lang_contrast_ckpt and lang_listnet_ckpt: one language-model checkpoint "
                         "at most")
    if lang_pretrain_ckpt:
        load_lang_pretrain(bert, lang_pretrain_ckpt)
    if lang_contrast_ckpt:
        load_contrast_pretrain(bert, lang_contrast_ckpt)
    if lang_listnet_ckpt:
        load_listnet_pretrain(bert, lang_listnet_ckpt)


def build_two_stream(clip_frame_num=16, hidden_size=128, head_type="mlp", dropout=None, seed=None, device=None,
                     precision="fp32", bn_stats=None, lang_pretrain_ckpt=None, lang_contrast_ckpt=None,
                     lang_listnet_ckpt=None):
    from model.fusion.two_stream import TwoStream
    from model.lang.bert_hugface import BertHugface
    from model.vision.resnet50_tsm import Resnet50TSM
    from vcg_hip.nn import BertConfig

    cfg = BertConfig(output_attentions=True)
    if dropout is not None:
        cfg.hidden_dropout_prob = dropout
        cfg.attention_probs_dropout_prob = dropout
    with contextlib.redirect_stdout(io.StringIO()):
        lang_model = BertHugface(pretrain_stage=False, config=cfg)
    vision_model = Resnet50TSM(segments_size=clip_frame_num, shift_div=8, pretrain_stage=False)
    model = TwoStream(lang_model.base_model, vision_model.base_model, lang_model.embed_size, vision_model.feature_dim,
                      clip_frame_num, hidden_size)
    model.build_chapter_head(output_size=2, head_type=head_type)
    if dropout is not None and head_type == "attn":
        model.fusion_head.head.attn_drop.p = dropout
    if device is not None:
        model = model.to(device)
    if seed is not None:
        synth.init_params(model, seed)  # on the GPU this runs the HIP generator (bit-identical to numpy)
    # (after the seeded init, which covers every parameter)
    _load_lang(model.lang_model, lang_pretrain_ckpt, lang_contrast_ckpt, lang_listnet_ckpt)
    if bn_stats is not None:
        synth.load_bn_stats(model, bn_stats)
    model.precision = precision
    return model


def build_model(data_mode="all", clip_frame_num=16, hidden_size=128, head_type="mlp", model_type="r50tsm", seed=None,
                device=None, precision="bf16", dropout=None, lang_pretrain_ckpt=None, lang_contrast_ckpt=None,
                lang_listnet_ckpt=None):
    """The driver's model by `--data_mode` (`train_video_segment_point.py:330-363`): "text" ->
    BertHugface + head, "image" -> Resnet50TSM (or Resnet50) + head, "all" -> TwoStream. lang_pretrain_ckpt: the
    masked-LM stage's checkpoint for the language model (`:326-330`; "all" and "text"); lang_contrast_ckpt: the
    contrastive stage's instead; lang_listnet_ckpt: the listwise stage's instead."""
    if data_mode == "all":
        return build_two_stream(clip_frame_num, hidden_size, head_type, dropout, seed, device, precision,
                                lang_pretrain_ckpt=lang_pretrain_ckpt, lang_contrast_ckpt=lang_contrast_ckpt,
                                lang_listnet_ckpt=lang_listnet_ckpt)
    if data_mode == "text":
        from model.lang.bert_hugface import BertHugface
        from vcg_hip.nn import BertConfig
        cfg = BertConfig(output_attentions=True)
        if dropout is not None:
            cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = dropout
        with contextlib.redirect_stdout(io.StringIO()):
            model = BertHugface(pretrain_stage=False, config=cfg)
    elif data_mode == "image":
        if model_type == "r50tsm":
            from model.vision.resnet50_tsm import Resnet50TSM
            model = Resnet50TSM(segments_size=clip_frame_num, shift_div=8, pretrain_stage=False)
        elif model_type == "r50":
            from model.vision.resnet50 import Resnet50
            model = Resnet50(segments_size=clip_frame_num, pretrain_stage=False)
        else:
            raise RuntimeError(f"Unknown model_type {model_type}")
    else:
        raise RuntimeError(f"Unknown data mode {data_mode}")
    model.build_chapter_head()
    if device is not None:
        model = model.to(device)
    if seed is not None:
        synth.init_params(model, seed)
    if lang_pretrain_ckpt or lang_contrast_ckpt or lang_listnet_ckpt:
        if data_mode != "text":
            raise ValueError("lang_pretrain_ckpt / lang_contrast_ckpt / lang_listnet_ckpt: the image-only model has no "
                             "language model")
        _load_lang(model.base_model, lang_pretrain_ckpt, lang_contrast_ckpt, lang_listnet_ckpt)
    model.precision = precision
    return model


def build_window_two_stream(clip_frame_num=16, window_size=1, hidden_size=128, head_type="cross_attn", seed=None,
                            device=None, precision="fp32", bn_stats=None):
    """The window model as the reference DDP driver builds it (train_video_segment_ddp.py:463-486):
    two_stream_window.TwoStream(lang.base_model, vision.base_model, 768, 2048, T, 128, window_size) +
    build_chapter_head(2, head_type)."""
    from model.fusion.two_stream_window import TwoStream
    from model.lang.bert_hugface import BertHugface
    from model.vision.resnet50_tsm import Resnet50TSM
    from vcg_hip.nn import BertConfig

    with contextlib.redirect_stdout(io.StringIO()):
        lang_model = BertHugface(pretrain_stage=False, config=BertConfig(output_attentions=True))
    vision_model = Resnet50TSM(segments_size=clip_frame_num, shift_div=8, pretrain_stage=False)
    model = TwoStream(lang_model.base_model, vision_model.base_model, lang_model.embed_size, vision_model.feature_dim,
                      clip_frame_num, hidden_size, window_size)
    with contextlib.redirect_stdout(io.StringIO()):
        model.build_chapter_head(output_size=2, head_type=head_type)
    if device is not None:
        model = model.to(device)
    if seed is not None:
        synth.init_params(model, seed)
    if bn_stats is not None:
        synth.load_bn_stats(model, bn_stats)
    model.precision = precision
    return model
