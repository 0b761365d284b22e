"""CPU checks of the chapter-title (Pegasus) stage, inference half (reference model/lang/pegasus_hugface.py):

  * tests/pegasus_ref.py -- the oracle of the GPU tests -- equals transformers.PegasusForConditionalGeneration in fp64
    (eval mode, eager attention) within 1e-10 on right-padded sources and decoder inputs;
  * the native module tree has transformers' state-dict keys and shapes and its sinusoidal table; the flat layout puts
    q | k | v and the cross-attention's k | v back to back;
  * checkpoint loading: HF keys bare, under "base_model." and under "module.base_model.", inside "model_state_dict",
    into a tied and an untied head; a file that does not match is a ValueError, a nonzero final_logits_bias is refused;
  * configure_optimizers' two groups follow pegasus_hugface.py:58-72;
  * the host logic of generate (stub tokenizer, stubbed device steps): the EOS stop, the 1 + 2 + ... + n rows of
    sentence_logits, the max_text_len crop; cut_at_eos.
"""
import types

import pytest
import torch

import pegasus_ref as ref

CFG = dict(vocab_size=515, d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2,
           decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=256, max_position_embeddings=64,
           activation_function="relu", scale_embedding=True)  # (pegasus-large's values; transformers' defaults differ)
NH = 2


def _hf(seed=0, dtype=torch.float64):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(seed)
    cfg = transformers.PegasusConfig(attn_implementation="eager", **CFG)
    hf = transformers.PegasusForConditionalGeneration(cfg).eval()
    with torch.no_grad():  # (LayerNorms away from the identity, biases away from zero)
        for n, p in hf.named_parameters():
            if n.endswith("bias") or "layer_norm" in n:
                p.add_(torch.randn_like(p) * 0.1)
    return hf.to(dtype)


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    B, Ls, Ld = 3, 40, 7
    ids = torch.randint(2, CFG["vocab_size"], (B, Ls), generator=g)
    dec = torch.randint(2, CFG["vocab_size"], (B, Ld), generator=g)
    dec[:, 0] = 0
    mask = (torch.arange(Ls)[None] < torch.tensor([40, 33, 9])[:, None]).long()
    dmask = (torch.arange(Ld)[None] < torch.tensor([7, 5, 1])[:, None]).long()
    return ids * mask, mask, dec * dmask, dmask


def test_reference_matches_transformers_fp64():
    hf = _hf()
    ids, mask, dec, dmask = _batch()
    with torch.no_grad():
        want = hf(input_ids=ids, attention_mask=mask, decoder_input_ids=dec, decoder_attention_mask=dmask).logits
        got = ref.pegasus_logits(dict(hf.state_dict()), ids, mask, dec, dmask, NH)
    err = (got - want).abs().max().item()
    print(f"pegasus_ref vs transformers (fp64): max abs err {err:.3e}, max|logit| {want.abs().max().item():.3f}")
    assert got.dtype == torch.float64 and err <= 1e-10


def test_state_dict_keys_and_position_table():
    hf = _hf(dtype=torch.float32)
    from vcg_hip.nn import PegasusConfig, PegasusForConditionalGeneration
    ours = PegasusForConditionalGeneration(PegasusConfig(**CFG))
    a = {k: tuple(v.shape) for k, v in ours.state_dict().items()}
    b = {k: tuple(v.shape) for k, v in hf.state_dict().items()}
    assert a == b
    for st in ("encoder", "decoder"):
        k = f"model.{st}.embed_positions.weight"
        assert torch.equal(ours.state_dict()[k], hf.state_dict()[k])
        assert not getattr(ours.model, st).embed_positions.weight.requires_grad
        assert getattr(ours.model, st).embed_tokens.weight is ours.model.shared.weight
    assert ours.lm_head.weight is ours.model.shared.weight
    assert {n for n, _ in ours.named_parameters()} == {n for n, _ in hf.named_parameters()}
    hf.load_state_dict(ours.state_dict(), strict=True)
    c = PegasusConfig()  # google/pegasus-large
    assert (c.vocab_size, c.d_model, c.encoder_layers, c.decoder_layers, c.encoder_attention_heads, c.encoder_ffn_dim,
            c.max_position_embeddings, c.activation_function, c.scale_embedding, c.pad_token_id, c.eos_token_id,
            c.decoder_start_token_id, c.dropout, c.layer_norm_eps) == \
        (96103, 1024, 16, 16, 16, 4096, 1024, "relu", True, 0, 1, 0, 0.1, 1e-5)


def test_unsupported_configurations():
    from vcg_hip.nn import PegasusConfig, PegasusForConditionalGeneration
    with pytest.raises(NotImplementedError, match="relu"):
        PegasusForConditionalGeneration(PegasusConfig(**dict(CFG, activation_function="gelu")))
    with pytest.raises(NotImplementedError, match="head dim"):
        PegasusForConditionalGeneration(PegasusConfig(**dict(CFG, decoder_attention_heads=4)))
    m = PegasusForConditionalGeneration(PegasusConfig(**CFG))
    m.check_supported()
    m.final_logits_bias[0, 3] = 0.5
    with pytest.raises(NotImplementedError, match="final_logits_bias"):
        m.check_supported()


def test_flat_order_groups_projections():
    from model.lang.pegasus_hugface import PegasusHugface
    from vcg_hip.nn import PegasusConfig, _flat_order
    m = PegasusHugface(config=PegasusConfig(**CFG))
    order = _flat_order([n for n, _ in m.named_parameters()])
    assert sorted(order) == sorted(n for n, _ in m.named_parameters())
    pre = "base_model.model.decoder.layers.1."
    i = order.index(pre + "self_attn.q_proj.weight")
    assert order[i:i + 6] == [pre + "self_attn." + n for n in ("q_proj.weight", "k_proj.weight", "v_proj.weight",
                                                               "q_proj.bias", "k_proj.bias", "v_proj.bias")]
    i = order.index(pre + "encoder_attn.k_proj.weight")
    assert order[i:i + 4] == [pre + "encoder_attn." + n for n in ("k_proj.weight", "v_proj.weight", "k_proj.bias",
                                                                  "v_proj.bias")]


@pytest.mark.parametrize("prefix,wrap", [("", False), ("base_model.", False), ("module.base_model.", True)])
def test_checkpoint_prefixes(tmp_path, prefix, wrap):
    from model.lang.pegasus_hugface import PegasusHugface
    from vcg_hip.nn import PegasusConfig
    hf = _hf(seed=3, dtype=torch.float32)
    sd = {prefix + k: v for k, v in hf.state_dict().items()}
    path = str(tmp_path / "pegasus.bin")
    torch.save({"model_state_dict": sd, "epoch": 3} if wrap else sd, path)
    m = PegasusHugface(checkpoint=path, config=PegasusConfig(**CFG))
    got = m.base_model.state_dict()
    assert all(torch.equal(v, got[k]) for k, v in hf.state_dict().items())
    assert m.base_model.lm_head.weight is m.base_model.model.shared.weight  # still tied
    ids, mask, dec, dmask = _batch()
    with torch.no_grad():  # the loaded weights compute transformers' logits (through the statement, fp32)
        want = hf(input_ids=ids, attention_mask=mask, decoder_input_ids=dec, decoder_attention_mask=dmask).logits
        z = ref.pegasus_logits(dict(m.base_model.state_dict()), ids, mask, dec, dmask, NH)
    assert (z - want).abs().max().item() <= 1e-4


def test_checkpoint_env_untied_and_mismatch(tmp_path, monkeypatch):
    transformers = pytest.importorskip("transformers")
    from model.lang.pegasus_hugface import PegasusHugface
    from vcg_hip.nn import PegasusConfig
    hf = _hf(seed=4, dtype=torch.float32)
    sd = dict(hf.state_dict())
    # a fine-tuned head that was re-initialised (reinit_head=True): lm_head differs from shared
    sd["lm_head.weight"] = torch.randn_like(sd["lm_head.weight"])
    path = str(tmp_path / "finetuned.bin")
    torch.save(sd, path)
    monkeypatch.setenv("VCG_PEGASUS_CHECKPOINT", path)
    m = PegasusHugface(reinit_head=True, config=PegasusConfig(**CFG))
    assert m.base_model.lm_head.weight is not m.base_model.model.shared.weight
    assert torch.equal(m.base_model.lm_head.weight, sd["lm_head.weight"])
    assert torch.equal(m.base_model.model.shared.weight, sd["model.shared.weight"])
    with pytest.raises(ValueError, match="ties them"):  # the tied model cannot hold two different tensors
        PegasusHugface(config=PegasusConfig(**CFG))
    monkeypatch.delenv("VCG_PEGASUS_CHECKPOINT")
    # another model's file / another config's shapes / a nonzero final_logits_bias
    other = str(tmp_path / "gpt.bin")
    torch.save(transformers.OpenAIGPTModel(transformers.OpenAIGPTConfig(n_layer=1, n_embd=64, n_head=1, vocab_size=50,
                                                                        n_positions=16)).state_dict(), other)
    with pytest.raises(ValueError, match="not a PegasusForConditionalGeneration state dict"):
        PegasusHugface(checkpoint=other, config=PegasusConfig(**CFG))
    with pytest.raises(ValueError, match="shape mismatch"):
        PegasusHugface(checkpoint=path, config=PegasusConfig(**dict(CFG, vocab_size=500)), reinit_head=True)
    sd2 = dict(hf.state_dict())
    sd2["final_logits_bias"] = torch.full_like(sd2["final_logits_bias"], 0.25)
    biased = str(tmp_path / "biased.bin")
    torch.save(sd2, biased)
    with pytest.raises(NotImplementedError, match="final_logits_bias"):
        PegasusHugface(checkpoint=biased, config=PegasusConfig(**CFG))


def test_configure_optimizers_groups():
    from model.lang.pegasus_hugface import PegasusHugface
    from vcg_hip.nn import PegasusConfig
    m = PegasusHugface(reinit_head=True, config=PegasusConfig(**CFG))
    tc = types.SimpleNamespace(weight_decay=0.01, learning_rate=3e-4, betas=(0.9, 0.95))
    opt = m.configure_optimizers(tc)
    named = dict(m.named_parameters())
    decay, no_decay = set(), set()
    for pn in named:  # pegasus_hugface.py:58-72
        if pn.endswith("bias") or "layer_norm" in pn or "bn" in pn or "emb" in pn:
            no_decay.add(pn)
        else:
            decay.add(pn)
    ids = [{id(p) for p in g["params"]} for g in opt.param_groups]
    assert len(opt.param_groups) == 2
    assert ids[0] == {id(named[n]) for n in decay} and opt.param_groups[0]["weight_decay"] == 0.01
    assert ids[1] == {id(named[n]) for n in no_decay} and opt.param_groups[1]["weight_decay"] == 0.0
    assert "base_model.lm_head.weight" in decay and "base_model.model.shared.weight" in decay
    assert "base_model.model.encoder.embed_positions.weight" in no_decay
    m.fix_backbone()
    assert [n for n, p in m.named_parameters() if p.requires_grad] == ["base_model.lm_head.weight"]


class _Tok:
    """a word-level stub of PegasusTokenizer's three methods generate uses"""

    def tokenize(self, text):
        return text.split()

    def convert_tokens_to_ids(self, tokens):
        return [2 + (sum(map(ord, t)) % 500) for t in tokens]

    def decode(self, ids):
        return " ".join(f"<{i}>" for i in ids)


def _stubbed(script, seen):
    """a PegasusHugface whose device steps are stubs: step t's last-row argmax is script[t]"""
    from model.lang.pegasus_hugface import PegasusHugface
    from vcg_hip.nn import PegasusConfig
    m = PegasusHugface(config=PegasusConfig(**CFG)).eval()
    V = CFG["vocab_size"]

    def encode_once(input_ids):
        seen["input_ids"] = input_ids.clone()
        seen["encodes"] = seen.get("encodes", 0) + 1
        return None

    def step_logits(memory, dec_ids):
        t = dec_ids.shape[1] - 1
        seen.setdefault("dec", []).append(dec_ids.clone())
        z = torch.zeros(1, t + 1, V)
        z[0, :, 7] = 0.5
        z[0, -1, script[t]] = 1.0 + t
        return z

    m._encode_once = encode_once
    m._step_logits = step_logits
    m._draw = lambda z, temperature, top_k, sample: z.argmax(-1)
    return m


def test_generate_host_logic_eos_stop_and_rows():
    seen = {}
    m = _stubbed([11, 12, 1, 13, 14], seen)  # EOS (id 1) is the third token
    text, logits = m.generate("a b c d e f", _Tok(), "cpu", max_text_len=512, max_len=5)
    assert text == "<11> <12> <1>"
    assert tuple(logits.shape) == (1, 1 + 2 + 3, CFG["vocab_size"])
    assert seen["encodes"] == 1 and tuple(seen["input_ids"].shape) == (1, 6)  # no EOS appended to the source
    assert [d.tolist() for d in seen["dec"]] == [[[0]], [[0, 11]], [[0, 11, 12]]]
    # the rows are the steps' logits in order: step t's last row peaks at script[t]
    assert logits[0, [0, 2, 5]].argmax(-1).tolist() == [11, 12, 1]


def test_generate_host_logic_max_len_and_truncation():
    seen = {}
    m = _stubbed([11, 12, 13, 14, 15], seen)  # no EOS: max_len stops the loop
    text, logits = m.generate(" ".join(f"w{i}" for i in range(20)), _Tok(), "cpu", max_text_len=8, max_len=4)
    assert text == "<11> <12> <13> <14>"
    assert logits.shape[1] == 1 + 2 + 3 + 4
    tok = _Tok()
    assert seen["input_ids"].tolist() == [tok.convert_tokens_to_ids([f"w{i}" for i in range(8)])]
    with pytest.raises(ValueError, match="max_len"):
        m.generate("a", _Tok(), "cpu", max_len=64)
    with pytest.raises(ValueError, match="top_k"):
        m.generate("a", _Tok(), "cpu", top_k=0)


def test_cut_at_eos():
    from model.lang.pegasus_hugface import cut_at_eos
    t = torch.tensor([[5, 1, 7, 1, 9], [5, 6, 7, 8, 1], [1, 2, 3, 4, 5], [5, 6, 7, 8, 9]])
    out, n = cut_at_eos(t[:3], eos=1, pad=0)
    assert n.tolist() == [2, 5, 1] and out.tolist() == [[5, 1, 0, 0, 0], [5, 6, 7, 8, 1], [1, 0, 0, 0, 0]]
    out, n = cut_at_eos(t[[0, 2]], eos=1, pad=0)  # cropped to the longest row
    assert n.tolist() == [2, 1] and out.tolist() == [[5, 1], [1, 0]]
    out, n = cut_at_eos(t[3:], eos=1, pad=0)  # no EOS: the full length
    assert n.tolist() == [5] and out.tolist() == [[5, 6, 7, 8, 9]]


def test_forward_refuses_training():
    from model.lang.pegasus_hugface import PegasusHugface
    from vcg_hip.nn import PegasusConfig
    m = PegasusHugface(config=PegasusConfig(**CFG))
    ids, mask, dec, dmask = _batch()
    with pytest.raises(NotImplementedError, match="training"):
        m.train()(ids, mask, dec, dmask)
    with pytest.raises(NotImplementedError, match="training"):  # eval mode, but a gradient would be expected
        m.eval()(ids, mask, dec, dmask)
