"""CPU tests of the masked-LM pre-training data path and driver plumbing: the masking rule and dataset against
tests/golden/mlm_masking.json (the REFERENCE class YoutubeClipSubtitleDatasetForHugFace run by
tools/oracle/make_golden_mlm.py on tests/corpus_util.py's corpus with the HashTokenizer), short sequences, truncation,
the token-counted learning-rate schedule at hand-computed points, and the driver's argument errors."""
import json
import math
import os
import random

import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden", "mlm_masking.json")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    import corpus_util as cu
    root = str(tmp_path_factory.mktemp("mlm_corpus"))
    _, data_file, vid_file, subs, _, _ = cu.write_corpus(root, hw=8)
    return data_file, vid_file, subs


@pytest.fixture(scope="module")
def golden():
    with open(GOLD) as f:
        return json.load(f)


def test_dataset_reproduces_reference(corpus, golden):
    from data.synthetic_dataset import HashTokenizer
    from data.youtube_subtitle_dataset import YoutubeClipSubtitleDatasetForHugFace
    data_file, vid_file, _ = corpus
    n = n_masked = n_replaced = 0
    for cfg in golden["configs"]:
        ds = YoutubeClipSubtitleDatasetForHugFace(data_file, vid_file, "bert", HashTokenizer(),
                                                  clip_frame_num=cfg["clip_frame_num"],
                                                  max_text_len=cfg["max_text_len"])
        assert len(ds) == 2
        for it in cfg["items"]:
            random.seed(it["seed"])
            x, y, m = ds[it["i"]]
            assert x.dtype == y.dtype == m.dtype == torch.int64
            assert (x.tolist(), y.tolist(), m.tolist()) == (it["ids"], it["targets"], it["mask"]), (cfg, it["seed"])
            n += 1
            n_masked += sum(t != -1 for t in it["targets"])
        if cfg["max_text_len"] == 64:  # long enough for the 10 % replacement draw (>= 6 masked positions)
            mask_id = HashTokenizer().convert_tokens_to_ids(["[MASK]"])[0]
            n_replaced += sum(1 for it in cfg["items"] for t, i in zip(it["targets"], it["ids"])
                              if t != -1 and i != mask_id)
    assert n == 48 and n_masked > 100
    assert n_replaced > 0  # the golden exercises the replacement quirk


def test_pure_function_with_its_own_generator(corpus, golden):
    """The same items from random.Random instances: the clip draw, then encode_mlm's masking draws."""
    from data.synthetic_dataset import HashTokenizer
    from data.youtube_subtitle_dataset import clip_text, encode_mlm
    _, _, subs = corpus
    vids, image_num = ("vid00XyZ", "vid01XyZ"), (round(40.5 - 1), round(57.5 - 1))
    tok = HashTokenizer()
    for cfg in golden["configs"]:
        h = cfg["clip_frame_num"] // 2
        for it in cfg["items"]:
            rng = random.Random(it["seed"])
            t = rng.sample(list(range(h, image_num[it["i"]] - h)), k=1)[0]
            x, y, m = encode_mlm(tok, clip_text(subs[vids[it["i"]]], t, h), cfg["max_text_len"], rng)
            assert (x.tolist(), y.tolist(), m.tolist()) == (it["ids"], it["targets"], it["mask"])


@pytest.mark.parametrize("n_tokens,n_masks", [(1, 0), (2, 0), (3, 0), (4, 0), (5, 1), (11, 2)])
def test_short_sequences(n_tokens, n_masks):
    """round(n * 0.15) over the n = len - 1 maskable positions: none for n <= 3 (1 to 4 tokens), one at n = 4."""
    from data.youtube_subtitle_dataset import mask_tokens
    toks = ["[CLS]"] + [f"t{i}" for i in range(n_tokens - 1)]
    for seed in range(5):
        out, orig = mask_tokens(toks, random.Random(seed))
        assert len(out) == n_tokens and out[0] == "[CLS]" and len(orig) == n_masks
        assert toks == ["[CLS]"] + [f"t{i}" for i in range(n_tokens - 1)]  # the input list is not modified
        for pos, tok in orig.items():
            assert pos >= 1 and tok == toks[pos] and out[pos] == "[MASK]"  # (< 6 masks: nothing is replaced)
        assert [o for i, o in enumerate(out) if i not in orig] == [t for i, t in enumerate(toks) if i not in orig]


def test_replacement_samples_the_masked_list():
    """>= 6 masks: round(0.1 * masks) positions are overwritten with a draw from the already-masked token list, and
    the "stay unmasked" draw changes nothing but the generator's state."""
    from data.youtube_subtitle_dataset import mask_tokens
    toks = ["[CLS]"] + [f"t{i}" for i in range(60)]
    for seed in range(20):
        out, orig = mask_tokens(toks, random.Random(seed))
        assert len(orig) == round(60 * 0.15) == 9
        not_mask = [p for p in orig if out[p] != "[MASK]"]
        assert len(not_mask) <= round(9 * 0.1) == 1  # (a replacement may itself draw "[MASK]")
        for p in not_mask:
            assert out[p] in toks
        # replayed by hand
        rng = random.Random(seed)
        masked = rng.sample(list(range(1, 61)), 9)
        rng.sample(masked, 1)
        rep = rng.sample(masked, 1)
        exp = list(toks)
        for p in masked:
            exp[p] = "[MASK]"
        exp[rep[0]] = rng.sample(exp, 1)[0]
        assert out == exp and sorted(orig) == sorted(masked)


def test_truncation_and_padding():
    from data.synthetic_dataset import HashTokenizer
    from data.youtube_subtitle_dataset import encode_mlm
    tok = HashTokenizer()
    text = " ".join(f"w{i}" for i in range(40))
    x, y, m = encode_mlm(tok, text, 16, random.Random(0))
    assert x.shape == y.shape == m.shape == (16,) and m.tolist() == [1] * 16 and x[0].item() == 101
    assert int((y != -1).sum()) == round(15 * 0.15) and y[0].item() == -1
    plain = tok.convert_tokens_to_ids(tok.tokenize("[CLS] " + text)[:16])
    for p in range(16):  # a target is the original id at its position; other positions keep their id
        assert (y[p].item() == plain[p]) if y[p].item() != -1 else (x[p].item() == plain[p])
    x, y, m = encode_mlm(tok, "a b c", 16, random.Random(0))
    assert m.tolist() == [1] * 4 + [0] * 12 and x.tolist()[4:] == [0] * 12 and (y == -1).all()


def test_gpt_branch_raises(corpus):
    from data.synthetic_dataset import HashTokenizer
    from data.youtube_subtitle_dataset import YoutubeClipSubtitleDatasetForHugFace
    data_file, vid_file, _ = corpus
    with pytest.raises(RuntimeError, match="bert"):
        YoutubeClipSubtitleDatasetForHugFace(data_file, vid_file, "gpt", HashTokenizer(), 16, 50)


def test_synthetic_variant():
    from data.synthetic_dataset import HashTokenizer, SyntheticVideoCorpus
    from data.youtube_subtitle_dataset import SyntheticSubtitleDatasetForHugFace
    ds = SyntheticSubtitleDatasetForHugFace(SyntheticVideoCorpus(3, H=8, W=8, seed=5), "bert", HashTokenizer(), 16, 50)
    assert len(ds) == 3
    random.seed(3)
    a = [ds[i] for i in range(3)]
    random.seed(3)
    b = [ds[i] for i in range(3)]
    for (x, y, m), (x2, y2, m2) in zip(a, b):
        assert torch.equal(x, x2) and torch.equal(y, y2) and torch.equal(m, m2)
        assert x.shape == (50,) and x[0].item() == 101 and ((y == -1) | (m == 1)).all()
        assert int((y != -1).sum()) == round((int(m.sum()) - 1) * 0.15)


def test_lr_schedule():
    import pretrain_lang_model_hugface as drv
    c = drv.TrainerConfig(warmup_tokens=1000, final_tokens=11000, lr_decay_type="cosine")
    assert drv.lr_multiplier(c, 0) == 0.0
    assert drv.lr_multiplier(c, 250) == 0.25
    assert drv.lr_multiplier(c, 1000) == 1.0                      # progress 0
    assert drv.lr_multiplier(c, 6000) == pytest.approx(0.5)       # progress 0.5
    assert drv.lr_multiplier(c, 3500) == pytest.approx(0.5 * (1 + math.cos(math.pi * 0.25)))
    assert drv.lr_multiplier(c, 11000) == 0.001                   # progress 1: the floor
    # past final_tokens the reference does not clamp the progress: 4.9 -> 0.5 (1 + cos(0.9 pi))
    assert drv.lr_multiplier(c, 50000) == pytest.approx(0.5 * (1 + math.cos(0.9 * math.pi)), rel=1e-9)
    assert drv.lr_multiplier(c, 21000) == pytest.approx(1.0)      # progress 2: the cosine is back at its top
    e = drv.TrainerConfig(warmup_tokens=1000, final_tokens=11000, lr_decay_type="exp")
    assert drv.lr_multiplier(e, 2000) == 1                        # progress 0.1
    assert drv.lr_multiplier(e, 4000) == 0.1                      # 0.3
    assert drv.lr_multiplier(e, 6000) == 0.01                     # 0.5
    assert drv.lr_multiplier(e, 8000) == 0.001                    # 0.7
    assert drv.lr_multiplier(e, 3000) == 0.001                    # exactly 0.2: no branch takes the edge
    z = drv.TrainerConfig(warmup_tokens=0, final_tokens=0, lr_decay_type="cosine")
    assert drv.lr_multiplier(z, 11) == 0.001                      # max(1, 0) denominators: progress 11, cos = -1
    with pytest.raises(RuntimeError):
        drv.lr_multiplier(drv.TrainerConfig(warmup_tokens=0, final_tokens=10, lr_decay_type="linear"), 5)


def test_driver_argument_errors(capsys):
    import pretrain_lang_model_hugface as drv
    with pytest.raises(SystemExit):
        drv.main(["--model_type", "gpt"])
    assert "bert" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        drv.main(["--lr_decay_type", "linear"])
    with pytest.raises(SystemExit):
        drv.main(["--data_file", "x.csv"])
    with pytest.raises(SystemExit, match="max_text_len"):  # checked before the GPU is touched
        drv.main(["--max_text_len", "513"])
    args = drv.parse_args([])
    assert (args.model_type, args.epoch, args.batch_size, args.lr_decay_type, args.max_text_len) == \
        ("bert", 3001, 64, "cosine", 50)


def test_point_driver_flag_default():
    """--lang_pretrain_ckpt is absent by default: build_model receives None and nothing changes."""
    import inspect

    from vcg_hip import build
    assert inspect.signature(build.build_model).parameters["lang_pretrain_ckpt"].default is None
    assert inspect.signature(build.build_two_stream).parameters["lang_pretrain_ckpt"].default is None
