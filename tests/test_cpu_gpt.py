"""CPU checks of the generative (GPT) stage (reference model/lang/gpt_hugface.py, the `gpt` branches of
data/youtube_subtitle_dataset.py:329-347 and pretrain_lang_model_hugface.py):

  * tests/gpt_ref.py -- the oracle of the GPU tests -- equals transformers.OpenAIGPTModel within 1e-5 (fp32, eval mode)
    on right-padded, holed and all-zero masks;
  * the native model's state dict has transformers' keys and shapes, and weights load in both directions;
  * the dataset class reproduces tests/golden/gpt_dataset.json (the reference class's recorded output) item for item;
  * the optimizer's decay groups follow gpt_hugface.py:51-64;
  * the driver's argument errors.
"""
import json
import os
import random

import pytest
import torch

from gpt_ref import gpt_hidden

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpt_dataset.json")
CFG = dict(n_layer=2, n_embd=128, n_head=2, vocab_size=211, n_positions=64)


def _masks(B, L):
    m = torch.ones(B, L, dtype=torch.int64)
    m[0, L - 5:] = 0          # right padding
    m[1, 3:7] = 0             # a hole behind a valid position 0
    m[2, :] = 0               # all zero
    return m


def test_reference_matches_transformers():
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(0)
    hf = transformers.OpenAIGPTModel(transformers.OpenAIGPTConfig(**CFG)).eval()
    with torch.no_grad():  # (LayerNorms away from the identity, biases away from zero)
        for n, p in hf.named_parameters():
            if n.endswith("bias") or ".ln_" in n:
                p.add_(torch.randn_like(p) * 0.1)
    B, L = 3, 19
    ids = torch.randint(0, CFG["vocab_size"], (B, L))
    mask = _masks(B, L)
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=mask).last_hidden_state
        got = gpt_hidden(dict(hf.state_dict()), ids, mask, CFG["n_head"])
    err = (got - want).abs().max().item()
    print(f"gpt_ref vs transformers: max abs err {err:.3e}")
    assert err <= 1e-5
    # fp64: the same function, exact arithmetic
    got64 = gpt_hidden({k: v.double() for k, v in hf.state_dict().items()}, ids, mask, CFG["n_head"])
    assert (got64 - want.double()).abs().max().item() <= 1e-5


def test_state_dict_parity():
    transformers = pytest.importorskip("transformers")
    from vcg_hip.nn import OpenAIGPTConfig, OpenAIGPTModel
    ours = OpenAIGPTModel(OpenAIGPTConfig(**CFG))
    hf = transformers.OpenAIGPTModel(transformers.OpenAIGPTConfig(**CFG))
    a = {k: tuple(v.shape) for k, v in ours.state_dict().items()}
    b = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    assert a == b
    assert a["h.0.attn.c_attn.weight"] == (128, 384) and a["h.1.mlp.c_proj.weight"] == (512, 128)  # Conv1D: [in, out]
    hf.load_state_dict(ours.state_dict(), strict=True)
    ours2 = OpenAIGPTModel(OpenAIGPTConfig(**CFG))
    ours2.load_state_dict(hf.state_dict(), strict=True)
    assert all(torch.equal(v, ours2.state_dict()[k]) for k, v in ours.state_dict().items())
    # the full-size default is openai-gpt's
    c = OpenAIGPTConfig()
    assert (c.vocab_size, c.n_positions, c.n_embd, c.n_layer, c.n_head, c.layer_norm_epsilon) == \
        (40478, 512, 768, 12, 12, 1e-5)


def test_checkpoint_loads(tmp_path):
    transformers = pytest.importorskip("transformers")
    from model.lang.gpt_hugface import GPTHugface
    from vcg_hip.nn import OpenAIGPTConfig
    hf = transformers.OpenAIGPTModel(transformers.OpenAIGPTConfig(**CFG))
    path = str(tmp_path / "openai-gpt.bin")
    torch.save(hf.state_dict(), path)
    m = GPTHugface(checkpoint=path, config=OpenAIGPTConfig(**CFG))
    assert all(torch.equal(v, m.base_model.state_dict()[k]) for k, v in hf.state_dict().items())
    assert (m.vocab_size, m.embed_size) == (211, 128)
    assert m.head.bias is None and tuple(m.head.weight.shape) == (211, 128)
    m.build_chapter_head(2)
    assert tuple(m.head.weight.shape) == (2, 128) and not m.head.bias.any()
    # biases away from zero arrive too, and a seeded build keeps the checkpoint (also given by the environment)
    with torch.no_grad():
        for p in hf.parameters():
            p.add_(0.01)
    torch.save(hf.state_dict(), path)
    from vcg_hip.build import build_gpt_model
    m2 = build_gpt_model(seed=3, precision="fp32", config=OpenAIGPTConfig(**CFG), checkpoint=path)
    assert all(torch.equal(v, m2.base_model.state_dict()[k]) for k, v in hf.state_dict().items())
    os.environ["VCG_GPT_CHECKPOINT"] = path
    try:
        m3 = build_gpt_model(seed=3, precision="fp32", config=OpenAIGPTConfig(**CFG))
    finally:
        del os.environ["VCG_GPT_CHECKPOINT"]
    assert all(torch.equal(v, m3.base_model.state_dict()[k]) for k, v in hf.state_dict().items())
    assert torch.equal(m3.head.weight, m2.head.weight)  # (the head stays the seeded one)
    # this class's own checkpoint, and a file of another model
    torch.save({"model_state_dict": m2.state_dict()}, path)
    m4 = GPTHugface(checkpoint=path, config=OpenAIGPTConfig(**CFG))
    assert all(torch.equal(v, m4.base_model.state_dict()[k]) for k, v in hf.state_dict().items())
    torch.save({"encoder.layer.0.weight": torch.zeros(2)}, path)
    with pytest.raises(ValueError, match="not an OpenAIGPTModel"):
        GPTHugface(checkpoint=path, config=OpenAIGPTConfig(**CFG))


def test_dataset_matches_reference_golden(tmp_path):
    import corpus_util as cu
    from data.synthetic_dataset import HashGPTTokenizer
    from data.youtube_subtitle_dataset import YoutubeClipSubtitleDatasetForGPT
    with open(GOLDEN) as f:
        gold = json.load(f)
    _, data_file, vid_file, _, _, _ = cu.write_corpus(str(tmp_path), hw=8)
    n = 0
    for cfg in gold["configs"]:
        ds = YoutubeClipSubtitleDatasetForGPT(data_file, vid_file, HashGPTTokenizer(), cfg["clip_frame_num"],
                                              cfg["max_text_len"])
        assert len(ds) == 2 and ds.model_type == "gpt"
        for it in cfg["items"]:
            random.seed(it["seed"])
            x, y, m = ds[it["i"]]
            assert x.dtype == y.dtype == m.dtype == torch.int64
            assert x.tolist() == it["x"] and y.tolist() == it["y"] and m.tolist() == it["mask"], (cfg, it["seed"])
            n += 1
    assert n == 30


def test_encode_gpt_edges():
    from data.synthetic_dataset import HashGPTTokenizer, SyntheticVideoCorpus
    from data.youtube_subtitle_dataset import SyntheticSubtitleDatasetForGPT, encode_gpt
    tok = HashGPTTokenizer(97)
    for text, n in (("", 0), ("one", 0), ("one two", 1), ("a b c d e f g h", 5)):
        x, y, m = encode_gpt(tok, text, 5)
        assert x.shape == y.shape == m.shape == (5,)
        assert int(m.sum()) == n and (y[n:] == -1).all() and (x[n:] == 0).all()
        assert (y[:n] >= 0).all() and (y[:n] < 97).all()
        assert x[1:n].tolist() == y[:max(n - 1, 0)].tolist()  # next-token pairs
    encode_gpt(tok, "a b c", 5, vocab_size=97)
    with pytest.raises(ValueError, match="token id outside"):  # checked on the host, where the ids are made
        encode_gpt(HashGPTTokenizer(40478), "a b c d e f g h i j k l", 5, vocab_size=10)
    ds = SyntheticSubtitleDatasetForGPT(SyntheticVideoCorpus(3, H=8, W=8, seed=5), HashGPTTokenizer(), 16, 50)
    random.seed(3)
    a = [ds[i] for i in range(len(ds))]
    random.seed(3)
    b = [ds[i] for i in range(len(ds))]
    assert len(a) == 3 and all(torch.equal(s, t) for u, v in zip(a, b) for s, t in zip(u, v))
    assert all(int(x.max()) < 40478 and int(x.min()) >= 0 for x, _, _ in a)


def test_optimizer_groups():
    from model.lang.gpt_hugface import GPTHugface, no_decay
    from vcg_hip.nn import OpenAIGPTConfig
    from vcg_hip.optim import param_groups
    m = GPTHugface(config=OpenAIGPTConfig(**CFG))
    groups = param_groups(m, 0.01, no_decay)
    names = {id(p): n for n, p in m.named_parameters()}
    decay = sorted(names[id(p)] for p in groups[0]["params"])
    nodecay = sorted(names[id(p)] for p in groups[1]["params"])
    assert groups[0]["weight_decay"] == 0.01 and groups[1]["weight_decay"] == 0.0
    assert len(decay) + len(nodecay) == len(names)
    # gpt_hugface.py:51-64: biases, "ln" and "emb" names take no decay
    want_nd = sorted(n for n in names.values() if n.endswith("bias") or "ln" in n or "emb" in n)
    assert nodecay == want_nd
    assert decay == sorted(["head.weight"] + [f"base_model.h.{i}.{w}.weight" for i in range(2)
                                              for w in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")])
    assert "base_model.tokens_embed.weight" in nodecay and "base_model.h.0.ln_1.weight" in nodecay


def test_driver_argument_errors():
    from train_lang import pretrain_gpt_lang_model as drv
    for bad in (["--lr_decay_type", "linear"], ["--data_file", "x.csv"], ["--vocab_file", "vocab.json"],
                ["--n_layer", "0"], ["--dropout", "1.0"], ["--model_type", "gpt"]):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)
    with pytest.raises(SystemExit, match="max_text_len"):  # checked before the GPU is touched
        drv.main(["--max_text_len", "513", "--n_layer", "1"])
    args = drv.parse_args([])
    assert (args.epoch, args.batch_size, args.lr_decay_type, args.max_text_len, args.n_layer) == \
        (3001, 64, "cosine", 50, 12)
    assert drv.TrainerConfig().model_type == "gpt"
