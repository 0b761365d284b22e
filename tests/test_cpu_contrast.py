"""CPU tests of the shot-contrastive (MoCo) pre-training stage: the dataset against tests/golden/contrast_dataset.json
(the REFERENCE class YoutubeClipConstrastSubtitleDataset run by tools/oracle/make_golden_contrast.py on
tests/corpus_util.py's corpus writer with the HashTokenizer), the model's parameter groups and state-dict keys, and
the checkpoint hand-off into the scorer's language model."""
import json
import os
import random

import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "contrast_dataset.json")
K = 64


@pytest.fixture(scope="module")
def golden():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory, golden):
    import corpus_util as cu
    root = str(tmp_path_factory.mktemp("contrast_corpus"))
    nf = tuple(golden["n_frames"])
    _, data_file, vid_file, subs, _, _ = cu.write_corpus(root, n_videos=len(nf), n_frames=nf, hw=8)
    return data_file, vid_file, subs


def _small_config():
    from vcg_hip.nn import BertConfig
    return BertConfig(vocab_size=1200, num_hidden_layers=2, max_position_embeddings=64)


@pytest.fixture(scope="module")
def model():
    from vcg_hip.build import build_contrast_model
    return build_contrast_model(seed=3, K=K, copy_key=False, config=_small_config())


def test_dataset_reproduces_reference(corpus, golden):
    """ids, masks and the candidate order (left neighbours, then right), bit for bit, the re-draw branch included."""
    from data.synthetic_dataset import HashTokenizer
    from data.youtube_subtitle_dataset import YoutubeClipConstrastSubtitleDataset
    data_file, vid_file, _ = corpus
    settings = [(c["clip_frame_num"], c["max_text_len"], c["neighbor_size"]) for c in golden["configs"]]
    assert settings == [(10, 50, 3), (4, 12, 1), (8, 24, 2)]
    n = n_redraw = 0
    for cfg in golden["configs"]:
        T, L, nb = cfg["clip_frame_num"], cfg["max_text_len"], cfg["neighbor_size"]
        ds = YoutubeClipConstrastSubtitleDataset(data_file, vid_file, HashTokenizer(), clip_frame_num=T, max_text_len=L,
                                                 neighbor_size=nb)
        assert len(ds) == 3
        assert sorted({it["seed"] for it in cfg["items"]}) == [1, 2, 3, 4]
        for it in cfg["items"]:
            random.seed(it["seed"])
            q, qm, c, cm = ds[it["i"]]
            assert q.dtype == qm.dtype == c.dtype == cm.dtype == torch.int64
            assert q.shape == qm.shape == (L,) and c.shape == cm.shape == (2 * nb, L)
            assert (q.tolist(), qm.tolist(), c.tolist(), cm.tolist()) == \
                (it["query_ids"], it["query_mask"], it["cand_ids"], it["cand_mask"]), (T, L, nb, it["seed"], it["i"])
            n += 1
            n_redraw += it["redraw"]
    assert n == 36 and n_redraw >= 4  # (the golden exercises the too-short-video re-draw)


def test_candidate_order_and_pure_function(corpus):
    """contrast_item with its own generator: the candidates are the left neighbours in time order, then the right."""
    from data.synthetic_dataset import HashTokenizer
    from data.youtube_subtitle_dataset import contrast_clip_texts, contrast_clips, contrast_item, encode_plain
    _, _, subs = corpus
    tok, T, L, nb = HashTokenizer(), 4, 12, 1
    s = subs["vid01XyZ"]
    rng = random.Random(5)
    q, qm, c, cm = contrast_item(s, 56, tok, T, L, nb, rng)
    t = random.Random(5).sample(list(range(nb * T, 56 - (nb + 1) * T)), k=1)[0]
    clips = contrast_clips(t, T, nb)
    assert clips == [[t - T, t], [t, t + T], [t + T, t + 2 * T]]
    texts = contrast_clip_texts(s, clips)
    assert torch.equal(c[0], encode_plain(tok, texts[0], L)[0]) and torch.equal(c[1], encode_plain(tok, texts[2], L)[0])
    assert torch.equal(q, encode_plain(tok, texts[1], L)[0]) and q[0].item() == 101
    assert contrast_item(s, 3 * T, tok, T, L, nb, rng) is None  # too short: nothing drawn, the caller re-draws


def test_synthetic_variant():
    from data.synthetic_dataset import HashTokenizer, SyntheticVideoCorpus
    from data.youtube_subtitle_dataset import SyntheticClipConstrastSubtitleDataset
    corpus = SyntheticVideoCorpus(3, H=8, W=8, seed=5)
    ds = SyntheticClipConstrastSubtitleDataset(corpus, HashTokenizer(), 4, 16, 2)
    random.seed(3)
    a = [ds[i] for i in range(3)]
    random.seed(3)
    b = [ds[i] for i in range(3)]
    for x, y in zip(a, b):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
        assert x[0].shape == (16,) and x[2].shape == (4, 16) and x[0][0].item() == 101 and (x[2][:, 0] == 101).all()
    with pytest.raises(ValueError, match="no video longer"):
        SyntheticClipConstrastSubtitleDataset(corpus, HashTokenizer(), 40, 16, 3)


def test_param_groups(model):
    """This class's own rule: biases and names containing "ln" / "emb" take no decay, so every LayerNorm.weight outside
    `embeddings.` IS decayed (embeddings.LayerNorm.weight contains "emb"); encoder_k is listed, as in the reference."""
    from types import SimpleNamespace
    groups = model.param_groups(0.01)
    names = {id(p): n for n, p in model.named_parameters()}
    decay = [names[id(p)] for p in groups[0]["params"]]
    no_decay = [names[id(p)] for p in groups[1]["params"]]
    assert groups[0]["weight_decay"] == 0.01 and groups[1]["weight_decay"] == 0.0
    assert decay == sorted(decay) and no_decay == sorted(no_decay)
    assert sorted(decay + no_decay) == sorted(names.values()) and not set(decay) & set(no_decay)
    ln = [n for n in names.values() if n.endswith("LayerNorm.weight") and ".embeddings." not in n]
    assert len(ln) == 2 * 2 * 2 and all(n in decay for n in ln)  # 2 encoders x 2 layers x 2 LayerNorms
    for n in names.values():
        if n.endswith("bias") or ".embeddings." in n:
            assert n in no_decay, n
    assert any(n.startswith("encoder_k.") for n in decay) and any(n.startswith("encoder_k.") for n in no_decay)
    # the reference's loop, restated (bert_hugface_constrast.py:66-79)
    ref_no_decay = set()
    for mn, m in model.named_modules():
        for pn, _ in m.named_parameters():
            fpn = "%s.%s" % (mn, pn) if mn else pn
            if pn.endswith("bias") or "ln" in fpn or "emb" in fpn:
                ref_no_decay.add(fpn)
    assert set(no_decay) == ref_no_decay
    opt = model.configure_optimizers(SimpleNamespace(weight_decay=0.01, learning_rate=1e-4, betas=(0.9, 0.95)))
    assert [len(g["params"]) for g in opt.param_groups] == [len(decay), len(no_decay)]
    assert opt._skip == {id(p) for p in model.encoder_k.parameters()}


def test_state_dict_keys(model):
    from vcg_hip.nn import BertModel
    bert_keys = set(BertModel(_small_config()).state_dict())
    want = {pre + k for pre in ("encoder_q.", "encoder_k.") for k in bert_keys} | {"queue", "queue_ptr"}
    sd = model.state_dict()
    assert set(sd) == want
    assert tuple(sd["queue"].shape) == (768, K) and sd["queue"].dtype == torch.float32
    assert tuple(sd["queue_ptr"].shape) == (1,) and sd["queue_ptr"].dtype == torch.int64 and int(sd["queue_ptr"]) == 0
    assert (sd["queue"].norm(dim=0) - 1).abs().max().item() < 1e-5  # unit columns
    assert model.vocab_size == 1200 and model.embed_size == 768 and (model.K, model.m, model.T) == (K, 0.999, 0.07)


def test_default_constructor_copies_the_query_encoder():
    from model.lang.bert_hugface_constrast import BertHugfaceConstrast
    m = BertHugfaceConstrast(K=16, config=_small_config())
    for (nq, pq), (nk, pk) in zip(m.encoder_q.named_parameters(), m.encoder_k.named_parameters()):
        assert nq == nk and torch.equal(pq, pk) and pq.data_ptr() != pk.data_ptr()


def test_checkpoint_hand_off(model, tmp_path):
    from vcg_hip.build import load_contrast_pretrain
    from vcg_hip.nn import BertModel
    path = str(tmp_path / "pretrain.pth")
    torch.save(model.state_dict(), path)  # (the driver's checkpoint: a bare state dict)
    bert = BertModel(_small_config())
    load_contrast_pretrain(bert, path)
    differs = 0
    for (n, p), (_, pq), (_, pk) in zip(bert.named_parameters(), model.encoder_q.named_parameters(),
                                        model.encoder_k.named_parameters()):
        assert torch.equal(p, pq), n
        differs += not torch.equal(p, pk)
    assert differs > 0  # (copy_key=False: taking encoder_k by mistake would show)
    mlm = str(tmp_path / "mlm.pth")
    sd = {"base_model." + k: v for k, v in bert.state_dict().items()}
    sd["head.weight"] = torch.zeros(1200, 768)
    torch.save({"epoch": 0, "model_state_dict": sd}, mlm)
    with pytest.raises(ValueError, match="contrastive"):
        load_contrast_pretrain(BertModel(_small_config()), mlm)
    # a key missing from the checkpoint is an error (strict)
    sd2 = {k: v for k, v in model.state_dict().items() if k != "encoder_q.pooler.dense.bias"}
    torch.save(sd2, path)
    with pytest.raises(RuntimeError):
        load_contrast_pretrain(BertModel(_small_config()), path)


def test_point_driver_flag(monkeypatch, tmp_path):
    """--lang_contrast_ckpt goes through the scorer driver's own parser into vcg_hip.build.build_model; absent, it is
    None, and --lang_pretrain_ckpt is untouched."""
    import inspect

    import train_video_segment_point as drv
    from vcg_hip import build
    assert inspect.signature(build.build_model).parameters["lang_contrast_ckpt"].default is None
    assert inspect.signature(build.build_two_stream).parameters["lang_contrast_ckpt"].default is None

    class _Stop(Exception):
        pass

    seen = []

    def fake_build(*a, **kw):
        seen.append(kw)
        raise _Stop

    monkeypatch.setattr(build, "build_model", fake_build)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    tiny = ["--clip_frame_num", "4", "--resolution", "8", "--max_text_len", "16", "--videos", "2", "--epoch", "0"]
    for extra, want in (([], (None, None)), (["--lang_contrast_ckpt", "c.pth"], (None, "c.pth")),
                        (["--lang_pretrain_ckpt", "m.pth"], ("m.pth", None))):
        with pytest.raises(_Stop):
            drv.main(tiny + extra)
        assert (seen[-1]["lang_pretrain_ckpt"], seen[-1]["lang_contrast_ckpt"]) == want
    monkeypatch.undo()
    path = str(tmp_path / "x.pth")
    torch.save({"queue": torch.zeros(1)}, path)
    with pytest.raises(ValueError, match="one language-model checkpoint"):  # the two flags exclude each other
        build._load_lang(None, path, path)
