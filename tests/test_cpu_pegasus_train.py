"""CPU checks of tests/pegasus_train_ref.py, the training statement the GPU tests of the Pegasus training kernels are
held against, on the tiny config and the padded batch of tests/test_cpu_pegasus.py:

  * with every mask equal to one, its loss and every parameter gradient in fp64 equal the installed transformers'
    PegasusForConditionalGeneration in train() mode with the three dropout rates at 0, within 1e-10, with the tied and
    with an untied head; row pad_token_id of the embedding gradient is exactly zero with an untied head (the source
    ids hold pad tokens, and the decoder's start token is the pad token);
  * the dropout sites: torch.nn.functional.dropout is patched to record (p, shape, training) during one transformers
    training forward with three distinct rates; the multiset of (rate, shape) equals what the statement applies;
  * cross_attention_train without a keep mask is pegasus_ref.cross_attention_ref, and a keep mask scales the kept
    probabilities by 1 / (1 - p);
  * data.youtube_chapter_title_dataset.YoutubeChapterTitleDataset gives the reference class's items
    (tests/golden/title_dataset.json, tools/oracle/make_golden_title.py) for every recorded seed and config, among them
    a chapter without subtitles and a title of at least chapter_title_text_len tokens; the stub tokenizer's id ranges;
    clean_str / remove_timestamp;
  * the host logic of train_chapter_title_gen.py with the device step stubbed: the learning-rate schedule's values,
    the test epoch every 20 epochs, the checkpoint names, contents and the checkpoint_best.pth link.
"""
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

import pegasus_ref as ref
import pegasus_train_ref as tref
from test_cpu_pegasus import CFG, NH, _batch

PAD = 0


def _hf_train(seed=0, untie=False, rates=(0.0, 0.0, 0.0)):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(seed)
    cfg = transformers.PegasusConfig(attn_implementation="eager", dropout=rates[0], attention_dropout=rates[1],
                                     activation_dropout=rates[2], **CFG)
    hf = transformers.PegasusForConditionalGeneration(cfg)
    with torch.no_grad():  # (LayerNorms away from the identity, biases away from zero)
        for n, p in hf.named_parameters():
            if n.endswith("bias") or "layer_norm" in n:
                p.add_(torch.randn_like(p) * 0.1)
    if untie:  # (the reference's reinit_head=True: a fresh Linear in place of the tied head)
        hf.lm_head = torch.nn.Linear(CFG["d_model"], CFG["vocab_size"], bias=False)
        hf.lm_head.weight.data.normal_(mean=0.0, std=0.02)
    assert hf.config.pad_token_id == PAD
    return hf.double().train()


def _statement_params(hf):
    """the statement's parameter dict: a fresh leaf per trained parameter of hf (a tied head is the same leaf)"""
    P = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    names = [n for n, p in hf.named_parameters() if p.requires_grad]
    for n in names:
        P[n].requires_grad_()
    if "lm_head.weight" not in names:
        P["lm_head.weight"] = P["model.shared.weight"]
    return P, names


@pytest.mark.parametrize("untie", [False, True])
def test_gradients_match_transformers_fp64(untie):
    hf = _hf_train(untie=untie)
    ids, _, dec, _ = _batch()  # (the padded ids; every mask is one below)
    mask, dmask = torch.ones_like(ids), torch.ones_like(dec)
    targets = torch.randint(2, CFG["vocab_size"], dec.shape, generator=torch.Generator().manual_seed(4))
    assert (ids == PAD).any() and (dec == PAD).any()
    logits = hf(input_ids=ids, attention_mask=mask, decoder_input_ids=dec, decoder_attention_mask=dmask).logits
    want = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), targets.reshape(-1))
    want.backward()
    P, names = _statement_params(hf)
    loss, _ = tref.title_loss(P, ids, mask, dec, dmask, targets, NH, pad=PAD)
    loss.backward()
    assert loss.dtype == torch.float64 and abs(loss.item() - want.item()) <= 1e-10
    worst = 0.0
    for n, p in hf.named_parameters():
        if not p.requires_grad:
            continue
        err = (P[n].grad - p.grad).abs().max().item()
        worst = max(worst, err)
        assert err <= 1e-10, n
    print(f"untie={untie}: loss {loss.item():.6f}, worst gradient error {worst:.3e} over {len(names)} parameters")
    g = P["model.shared.weight"].grad
    if untie:
        assert bool((g[PAD] == 0).all()) and g.abs().sum() > 0
    else:  # (the tied head's gradient lands on every row)
        assert g[PAD].abs().sum() > 0


def test_dropout_sites_match_transformers(monkeypatch):
    rates = (0.1, 0.2, 0.3)
    hf = _hf_train(rates=rates)
    ids, mask, dec, dmask = _batch()
    seen = []
    real = F.dropout

    def record(x, p=0.5, training=True, inplace=False):
        seen.append((float(p), tuple(x.shape), bool(training)))
        return real(x, p, training, inplace)

    monkeypatch.setattr(torch.nn.functional, "dropout", record)
    hf(input_ids=ids, attention_mask=mask, decoder_input_ids=dec, decoder_attention_mask=dmask)
    monkeypatch.undo()
    assert seen and all(t for _, _, t in seen)
    sites = tref.Sites(rates)
    P = {k: v.detach() for k, v in hf.state_dict().items()}
    tref.title_loss(P, ids, mask, dec, dmask, dec, NH, drop=sites, pad=PAD)
    got, want = Counter(sites.seen), Counter((p, s) for p, s, _ in seen)
    assert got == want, (got - want, want - got)
    assert {p for p, _ in got} == set(rates)  # every rate is used somewhere


def test_cross_attention_statement():
    B, nh, Lq, Lk = 2, 2, 3, 5
    g = torch.Generator().manual_seed(3)
    q, kv = torch.randn(B * Lq, nh * 64, generator=g).double(), torch.randn(B * Lk, 2 * nh * 64, generator=g).double()
    mask = torch.tensor([[1, 1, 0, 1, 0], [0, 0, 0, 0, 0]])
    want = ref.cross_attention_ref(q, kv, mask, B, nh, Lq, Lk)[0]
    assert torch.allclose(tref.cross_attention_train(q, kv, mask, B, nh, Lq, Lk), want, rtol=0, atol=1e-14)
    keep = torch.zeros(B * nh, Lq, Lk, dtype=torch.bool)
    keep[:, :, 0] = True  # only key 0 survives: ctx = P[:, 0] v[0] / (1 - p)
    out = tref.cross_attention_train(q, kv, mask, B, nh, Lq, Lk, keep, 0.5).view(B, Lq, nh, 64)
    v0 = kv.view(B, Lk, 2, nh, 64)[:, 0, 1]  # [B, nh, 64]
    assert torch.allclose(out[1], (v0[1] / Lk / 0.5)[None].expand(Lq, nh, 64), rtol=0, atol=1e-14)  # no valid key: 1 / Lk


# ------------------------------------------------------------------------------------------------ data and driver
def test_title_dataset_matches_the_reference(tmp_path):
    import json
    import os
    import random

    import title_corpus_util as tc
    from data.synthetic_dataset import HashPegasusTokenizer
    from data.youtube_chapter_title_dataset import YoutubeChapterTitleDataset
    with open(os.path.join(os.path.dirname(__file__), "golden", "title_dataset.json")) as f:
        gold = json.load(f)
    data_file, vid_file = tc.write_title_corpus(str(tmp_path))
    tok = HashPegasusTokenizer(tc.VOCAB)
    names = ("text_ids", "attention_mask", "input_decode_ids", "decode_attention_mask", "target_decode_ids")
    assert [(c["max_text_len"], c["chapter_title_text_len"]) for c in gold["configs"]] == tc.CONFIGS
    empty = long_title = 0
    for cfg in gold["configs"]:
        L, T = cfg["max_text_len"], cfg["chapter_title_text_len"]
        ds = YoutubeChapterTitleDataset(data_file, vid_file, tok, max_text_len=L, chapter_title_text_len=T)
        assert len(ds) == 2 and len(cfg["items"]) == 2 * len(tc.SEEDS)
        for it in cfg["items"]:
            random.seed(it["seed"])
            got = ds[it["i"]]
            for n, t in zip(names, got):
                assert t.dtype == torch.int64 and t.tolist() == it[n], (L, T, it["seed"], it["i"], n)
            empty += sum(it["attention_mask"]) == 0
            long_title += T <= 2 and it["target_decode_ids"][-1] == 1 and sum(it["decode_attention_mask"]) == T
    assert empty > 0 and long_title > 0  # the fixture holds both edge cases


def test_stub_tokenizer_and_text_helpers():
    from data.common_utils import clean_str, remove_timestamp
    from data.synthetic_dataset import HashPegasusTokenizer
    tok = HashPegasusTokenizer(50)
    assert tok.tokenize("Hello  World\tagain") == ["hello", "world", "again"] and tok.tokenize("") == []
    ids = tok.convert_tokens_to_ids([tok.pad_token, tok.eos_token] + [f"w{i}" for i in range(500)])
    assert ids[:2] == [0, 1] and min(ids[2:]) >= 2 and max(ids[2:]) < 50 and len(set(ids[2:])) > 20
    assert tok.convert_tokens_to_ids("w1") == ids[3]
    assert clean_str("- (Intro) part 1!! ") == "Intro) part 1" and clean_str("--") == "--"
    assert remove_timestamp("at 1:02:03  the  end") == "at the end" and remove_timestamp("no  stamp") == "no  stamp"
    assert remove_timestamp("0:09 part 1") == "part 1"


def test_driver_schedule():
    import math

    import train_chapter_title_gen as drv
    c = drv.TrainerConfig(warmup_epochs=30, final_epochs=2700, lr_decay_type="cosine")
    assert drv.lr_multiplier(c, 0) == 1e-2 and drv.lr_multiplier(c, 15) == 0.5 and drv.lr_multiplier(c, 29) == 29 / 30
    assert drv.lr_multiplier(c, 30) == 0.5 * (1 + math.cos(math.pi * 30 / 2700))
    assert drv.lr_multiplier(c, 1350) == pytest.approx(0.5) and drv.lr_multiplier(c, 2700) == 0.001
    assert drv.lr_multiplier(c, 5000) == 0.001
    e = drv.TrainerConfig(warmup_epochs=10, final_epochs=100, lr_decay_type="exp")
    assert [drv.lr_multiplier(e, k) for k in (10, 19, 21, 39, 41, 59, 61, 100, 200)] == \
        [1, 1, 0.1, 0.1, 0.01, 0.01, 0.001, 0.001, 0.001]
    assert drv.lr_multiplier(e, 20) == 0.001  # (the reference's strict inequalities: exactly on a threshold)
    with pytest.raises(RuntimeError, match="decay type"):
        drv.lr_multiplier(drv.TrainerConfig(warmup_epochs=0, final_epochs=10, lr_decay_type="linear"), 3)
    z = drv.TrainerConfig(warmup_epochs=0, final_epochs=0)  # (--epoch below 100)
    assert drv.lr_multiplier(z, 1) == 0.001
    a = drv.parse_args([])
    assert (a.epoch, a.batch_size, a.lr_decay_type, a.model_type, a.gpu) == (3000, 4, "cosine", "pegasus", 0)
    assert (a.max_text_len, a.chapter_title_text_len, a.pegasus_ckpt, a.tokenizer) == (512, 30, None, None)
    d = drv.TrainerConfig()
    assert (d.max_epochs, d.batch_size, d.learning_rate, d.betas, d.grad_norm_clip, d.weight_decay, d.lr_decay) == \
        (10, 64, 3e-4, (0.9, 0.95), 1.0, 0.01, False)


class _StubOpt:
    def __init__(self):
        self.param_groups = [{"lr": None}, {"lr": None}]

    def state_dict(self):
        return {"state": {}, "param_groups": self.param_groups}


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(3))

    def configure_optimizers(self, config):
        return _StubOpt()


def _stub_trainer(tmp_path, test_accs, **conf):
    import train_chapter_title_gen as drv
    data = [tuple(torch.zeros(2, dtype=torch.int64) for _ in range(5)) for _ in range(4)]
    c = drv.TrainerConfig(batch_size=2, ckpt_dir=str(tmp_path / "ck"), learning_rate=1e-3, lr_decay=True,
                          warmup_epochs=2, final_epochs=40, **conf)
    tr = drv.Trainer(_StubModel(), None, data, data if test_accs is not None else None, c)
    accs = iter(test_accs or [])
    state = {"test_acc": None, "calls": []}

    def step(batch, is_train):  # the device step, stubbed: (loss, correct, count)
        state["calls"].append(is_train)
        if is_train:
            return 2.0, 1, 4
        return 1.0, state["test_acc"], 10

    real_run = tr.run_epoch

    def run_epoch(split, epoch):
        if split == "test":
            state["test_acc"] = next(accs)
        return real_run(split, epoch)

    tr.step, tr.run_epoch = step, run_epoch
    return tr, state


def test_driver_checkpoints_without_a_test_split(tmp_path):
    import os
    tr, state = _stub_trainer(tmp_path, None, max_epochs=3)
    tr.train()
    ck = tmp_path / "ck"
    names = sorted(p.name for p in ck.iterdir())
    assert names == ["checkpoint_1_-inf.pth", "checkpoint_2_-inf.pth", "checkpoint_3_-inf.pth", "checkpoint_best.pth"]
    link = ck / "checkpoint_best.pth"
    assert os.path.islink(link) and os.path.realpath(link) == os.path.realpath(ck / "checkpoint_3_-inf.pth")
    sd = torch.load(str(link), map_location="cpu", weights_only=True)
    assert set(sd) == {"epoch", "best_result", "model_state_dict", "optimizer_state_dict"} and sd["epoch"] == 3
    assert list(sd["model_state_dict"]) == ["w"]
    assert state["calls"] == [True] * 6  # two batches per epoch, no test epoch
    assert [h["epoch"] for h in tr.history] == [1, 2, 3] and all(h["loss"] == 2.0 and h["acc"] == 0.25 for h in tr.history)
    # the learning rate follows the epoch: warm-up 1 / 2, then the cosine over 40 epochs
    import math
    assert [h["lr"] for h in tr.history] == [1e-3 * 0.5, 1e-3 * 0.5 * (1 + math.cos(math.pi * 2 / 40)),
                                             1e-3 * 0.5 * (1 + math.cos(math.pi * 3 / 40))]
    assert all(g["lr"] == tr.history[-1]["lr"] for g in tr.optimizer.param_groups)


def test_driver_checkpoints_follow_the_test_accuracy(tmp_path):
    import os
    tr, state = _stub_trainer(tmp_path, [5, 3, 7], max_epochs=60)  # test accuracy 0.5, 0.3, 0.7 at epochs 20, 40, 60
    tr.train()
    ck = tmp_path / "ck"
    names = sorted(p.name for p in ck.iterdir())
    # epochs 20 .. 39 keep the first result (nothing better), 40 is worse, 60 is better
    assert names == ["checkpoint_20_0.5000.pth", "checkpoint_60_0.7000.pth", "checkpoint_best.pth"]
    assert os.path.realpath(ck / "checkpoint_best.pth") == os.path.realpath(ck / "checkpoint_60_0.7000.pth")
    tests = [h for h in tr.history if h["split"] == "test"]
    assert [h["epoch"] for h in tests] == [20, 40, 60] and [h["acc"] for h in tests] == [0.5, 0.3, 0.7]
    assert state["calls"].count(False) == 6 and state["calls"].count(True) == 120
