"""CPU tests of the listwise (ListNet) stage: the two datasets against tests/golden/listnet_dataset.json (the REFERENCE
classes YoutubeListwiseClipDataset and InferYoutubeVideoDataset run by tools/oracle/make_golden_listnet.py on
tests/corpus_util.py's corpus writer with the HashTokenizer), the driver's balanced selection and schedule against the
reference's expressions, the model's parameter groups, and the checkpoint hand-off's refusals."""
import json
import math
import os
import random

import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "listnet_dataset.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def corpora(tmp_path_factory, golden):
    """One corpus on disk per golden configuration."""
    import corpus_util as cu
    out = []
    for k, cfg in enumerate(golden["configs"]):
        root = str(tmp_path_factory.mktemp(f"listnet_corpus{k}"))
        nf = tuple(cfg["n_frames"])
        img_dir, data_file, vid_file, _, _, _ = cu.write_corpus(root, n_videos=len(nf), n_frames=nf, hw=8)
        out.append((img_dir, data_file, vid_file))
    return out


def _image_ok(img, rec):
    import corpus_util as cu
    img = torch.as_tensor(img)
    return (list(img.shape), str(img.dtype), cu.tensor_digest(img)) == (rec["img_shape"], rec["img_dtype"],
                                                                        rec["img_digest"])


def test_golden_configurations(golden):
    got = [(c["n_frames"], c["clip_frame_num"], c["max_text_len"], c["negative_clip_num"]) for c in golden["configs"]]
    assert got == [([40, 57], 8, 24, 4), ([95, 120], 8, 50, 10)]


def test_listwise_dataset_reproduces_reference(corpora, golden):
    """ids, masks, labels and images (by digest) of every slate, in modes "text" and "all", item by item."""
    from data.synthetic_dataset import HashTokenizer
    from data.youtube_dataset import YoutubeListwiseClipDataset
    n = 0
    for (img_dir, data_file, vid_file), cfg in zip(corpora, golden["configs"]):
        T, L, neg = cfg["clip_frame_num"], cfg["max_text_len"], cfg["negative_clip_num"]
        assert {r["mode"] for r in cfg["listwise"]} == {"text", "all"}
        ds = {mode: YoutubeListwiseClipDataset(img_dir, data_file, vid_file, HashTokenizer(), T, L,
                                               negative_clip_num=neg, mode=mode) for mode in ("text", "all")}
        for rec in cfg["listwise"]:
            random.seed(rec["seed"])
            img, ids, mask, labels = ds[rec["mode"]][rec["i"]]
            assert ids.dtype == mask.dtype == labels.dtype == torch.int64
            assert ids.shape == mask.shape == (2 + neg, L)
            assert labels.tolist() == [1, 1] + [0] * neg == rec["labels"]
            assert (ids.tolist(), mask.tolist()) == (rec["ids"], rec["mask"]), (rec["mode"], rec["seed"], rec["i"])
            assert _image_ok(img, rec), (rec["mode"], rec["seed"], rec["i"])
            if rec["mode"] == "text":
                assert tuple(img.shape) == (2 + neg,) and not img.any()  # the dummy image of every clip
            else:
                assert tuple(img.shape) == (2 + neg, T, 8, 8, 3) and img.dtype == torch.float32  # raw frames
            n += 1
    assert n == 24


def test_infer_video_dataset_reproduces_reference(corpora, golden):
    from data.infer_youtube_video_dataset import InferYoutubeVideoDataset
    from data.synthetic_dataset import HashTokenizer
    from train_video_segment_point import vision_transform
    n = n_pos = 0
    for (img_dir, data_file, vid_file), cfg in zip(corpora, golden["configs"]):
        T, L = cfg["clip_frame_num"], cfg["max_text_len"]
        for video in cfg["infer"]:
            ds = InferYoutubeVideoDataset(img_dir, data_file, vid_file, HashTokenizer(), T, L, mode=video["mode"],
                                          transform=vision_transform(False))
            ds.manual_choose_vid(video["vid"])
            assert len(ds) == len(video["items"]) and ds.get_duration() == video["duration"]
            for i, rec in enumerate(video["items"]):
                img, ids, mask, label = ds[i]
                assert (ids.tolist(), mask.tolist(), int(label)) == (rec["ids"], rec["mask"], rec["label"])
                assert _image_ok(img, rec), (video["mode"], video["vid"], i)
                n += 1
                n_pos += rec["label"]
    assert n == 142 and n_pos >= 12


def test_infer_video_dataset_needs_a_video(corpora, golden):
    from data.infer_youtube_video_dataset import InferYoutubeVideoDataset
    from data.synthetic_dataset import HashTokenizer
    img_dir, data_file, vid_file = corpora[0]
    ds = InferYoutubeVideoDataset(img_dir, data_file, vid_file, HashTokenizer(), 8, 24, mode="text")
    with pytest.raises(RuntimeError, match="You should run choose_vid before iterate this dataset"):
        len(ds)
    with pytest.raises(RuntimeError, match="You should run choose_vid before iterate this dataset"):
        ds[0]
    with pytest.raises(RuntimeError, match="is not existed in dataset"):
        ds.manual_choose_vid("nope")
    random.seed(3)
    ds.random_choose_vid()
    random.seed(3)
    assert ds.infer_vid == random.sample(ds.vids, 1)[0] and len(ds) > 0


def test_synthetic_datasets():
    from data.synthetic_dataset import (HashTokenizer, InferYoutubeVideoDataset, SyntheticVideoCorpus,
                                        YoutubeListwiseClipDataset)
    corpus = SyntheticVideoCorpus(3, min_len=160, max_len=240, H=8, W=8, seed=5)
    ds = YoutubeListwiseClipDataset(corpus, HashTokenizer(), 8, 16, negative_clip_num=3)
    random.seed(1)
    img, ids, mask, labels = ds[0]
    assert ids.shape == mask.shape == (5, 16) and labels.tolist() == [1, 1, 0, 0, 0] and tuple(img.shape) == (5,)
    assert (ids[:, 0] == 101).all()
    random.seed(1)
    assert torch.equal(ds[0][1], ids)
    frames = YoutubeListwiseClipDataset(corpus, HashTokenizer(), 8, 16, negative_clip_num=3, mode="all")
    random.seed(1)
    assert tuple(frames[0][0].shape) == (5, 8, 8, 8, 3)
    with pytest.raises(ValueError, match="negative clips"):
        YoutubeListwiseClipDataset(corpus, HashTokenizer(), 8, 16, negative_clip_num=500)
    dv = InferYoutubeVideoDataset(corpus, HashTokenizer(), 8, 16)
    with pytest.raises(RuntimeError, match="choose_vid"):
        len(dv)
    dv.manual_choose_vid(corpus.vids[1])
    assert len(dv) == len(range(0, corpus.image_num[corpus.vids[1]] - 8, 4))
    assert sum(dv[i][3] for i in range(len(dv))) >= 2


@pytest.mark.parametrize("batch_size", [2, 5, 64])
def test_balance_selection_is_the_references(batch_size):
    from train_lang.train_listwise import balance_selection
    slate_length = 12
    random.seed(batch_size)
    sel, cls = balance_selection(batch_size, slate_length)
    # the reference's draws (train_listwise.py:145-151), in its order: slate ix of the first half of the batch gives one
    # of its two positive clips, slate ix of the second half one of its negatives
    random.seed(batch_size)
    half = batch_size // 2
    want = []
    for ix in range(batch_size):
        lo, hi = (0, 1) if ix < half else (2, slate_length - 1)
        want.append(slate_length * ix + random.randint(lo, hi))
    assert sel == want and cls == [1] * half + [0] * (batch_size - half)
    assert all(0 <= s < batch_size * slate_length for s in sel)


def _small_config():
    from vcg_hip.nn import BertConfig
    return BertConfig(vocab_size=1200, num_hidden_layers=2, max_position_embeddings=64)


def test_parameter_groups_and_state_dict():
    from vcg_hip.build import build_listnet_model
    m = build_listnet_model(seed=3, config=_small_config())
    decay, no_decay = m.param_groups(0.01)
    assert decay["weight_decay"] == 0.01 and no_decay["weight_decay"] == 0.0
    names = {id(p): n for n, p in m.named_parameters()}
    dn, nn_ = {names[id(p)] for p in decay["params"]}, {names[id(p)] for p in no_decay["params"]}
    assert dn | nn_ == set(names.values()) and not dn & nn_
    for n in names.values():
        if n.endswith("bias") or "embeddings." in n:
            assert n in nn_, n
        else:
            assert n in dn, n
    # HF's LayerNorm.weight holds no "ln": outside embeddings. it IS decayed by this class's rule
    assert "base_model.encoder.layer.0.output.LayerNorm.weight" in dn
    assert "base_model.embeddings.LayerNorm.weight" in nn_
    assert {"head.weight", "surrogate_head.weight"} <= dn and {"head.bias", "surrogate_head.bias"} <= nn_
    assert [k for k in m.state_dict() if not k.startswith("base_model.")] == [
        "head.weight", "head.bias", "surrogate_head.weight", "surrogate_head.bias"]
    from model.lang import bert_hugface_constrast, bert_hugface_listnet
    assert bert_hugface_listnet._no_decay is bert_hugface_constrast._no_decay  # shared, not copied


@pytest.mark.parametrize("kind", ["cosine", "exp"])
def test_schedule_matches_reference(kind):
    from train_lang.train_listwise import TrainerConfig, lr_multiplier
    cfg = TrainerConfig(lr_decay=True, lr_decay_type=kind, warmup_epochs=30, final_epochs=270)

    def reference(epoch):  # train_listwise.py:186-212
        if epoch < cfg.warmup_epochs:
            return max(epoch / cfg.warmup_epochs, 1e-2)
        progress = epoch / cfg.final_epochs if epoch < cfg.final_epochs else 1.0
        if kind == "cosine":
            return max(0.001, 0.5 * (1.0 + math.cos(math.pi * progress)))
        th = 1 / 5
        if progress < th:
            return 1
        elif th < progress < th * 2:
            return 0.1
        elif th * 2 < progress < th * 3:
            return 0.01
        return 0.001

    for epoch in (0, 15, 30, 40, 60, 100, 135, 200, 269, 270, 400):
        assert lr_multiplier(cfg, epoch) == reference(epoch), epoch
    assert lr_multiplier(cfg, 0) == 1e-2 and lr_multiplier(cfg, 400) == 0.001


def test_hand_off_and_refusals(tmp_path):
    from vcg_hip.build import (_load_lang, build_contrast_model, build_listnet_model, load_listnet_pretrain)
    from vcg_hip.nn import BertModel
    m = build_listnet_model(seed=3, config=_small_config())
    ck = str(tmp_path / "listnet.pth")
    torch.save(m.state_dict(), ck)
    bert = BertModel(_small_config())
    load_listnet_pretrain(bert, ck)
    for n, p in bert.named_parameters():
        assert torch.equal(p.detach(), m.state_dict()["base_model." + n]), n
    contrast = build_contrast_model(seed=3, K=64, config=_small_config())
    cpath, mpath = str(tmp_path / "contrast.pth"), str(tmp_path / "mlm.pth")
    torch.save(contrast.state_dict(), cpath)
    mlm_sd = {k: v for k, v in m.state_dict().items() if k.startswith("base_model.")}
    mlm_sd["head.weight"] = torch.zeros(1200, 768)
    torch.save({"model_state_dict": mlm_sd}, mpath)
    torch.save(mlm_sd, str(tmp_path / "bare_mlm.pth"))
    for bad in (cpath, mpath, str(tmp_path / "bare_mlm.pth")):
        with pytest.raises(ValueError, match="not a listwise fine-tuning checkpoint"):
            load_listnet_pretrain(bert, bad)
    for two in ((ck, cpath, None), (ck, None, ck), (None, cpath, ck), (ck, cpath, ck)):
        with pytest.raises(ValueError, match="one language-model checkpoint at most"):
            _load_lang(bert, *two)
    import inspect
    from vcg_hip import build
    assert inspect.signature(build.build_model).parameters["lang_listnet_ckpt"].default is None  # off by default
    assert inspect.signature(build.build_two_stream).parameters["lang_listnet_ckpt"].default is None
