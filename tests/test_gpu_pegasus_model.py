"""The native Pegasus (vcg_hip/pegasus.py, model/lang/pegasus_hugface.py) against tests/pegasus_ref.py on a tiny config
(d_model 128, 2 heads, 2 + 2 layers, FFN 256, vocab 515, 64 positions): B = 3, source lengths (40, 33, 9) and decoder
lengths (7, 5, 1), right-padded.

  * fp32 parity mode: logits and title_loss against the fp64 statement within 4 x the error of the same statement in
    fp32 on the CPU + 1e-6 x max|ref| (the margin: other summation orders in the GEMMs);
  * bf16: relative Frobenius error of the logits <= 1.5 x that of the statement under torch.autocast(bfloat16) on the
    CPU, both against fp64 (README.md's measure for the BERT gradients); the loss within 1.5 x autocast's error + 1e-3;
  * the padded source columns of x do not reach the logits (bit-identical);
  * generate_ids, greedy, fp32 mode: the statement's greedy loop at every step whose fp64 top-2 logit margin exceeds
    1e-3 (at least 90 % of the steps have one: a condition on the statement, asserted); the EOS cut and `lengths` with
    the EOS planted through an untied head row; generate on batch row 0 gives generate_ids' tokens and
    1 + 2 + ... + n rows of logits;
  * the d_model = 256 tree, whose q | k | v and k | v lie back to back in the flat buffer: one GEMM per projection
    group gives the logits of a GEMM per member;
  * forward refuses training mode.
"""
import pytest
import torch

import pegasus_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(vocab_size=515, d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2,
           decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=256, max_position_embeddings=64)
NH = 2
SRC_LENS, DEC_LENS = (40, 33, 9), (7, 5, 1)
MAX_LEN = 8


@pytest.fixture(scope="module", autouse=True)
def _init():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)


def _model(seed=11, reinit_head=False, **over):
    """the tiny model on the CPU, LayerNorms away from the identity and biases away from zero"""
    from model.lang.pegasus_hugface import PegasusHugface
    from vcg_hip.nn import PegasusConfig
    torch.manual_seed(seed)
    m = PegasusHugface(reinit_head=reinit_head, config=PegasusConfig(**dict(CFG, **over)))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias") or "layer_norm" in n:
                p.add_(torch.randn_like(p) * 0.1)
    return m.eval()


def _params(m, dtype):
    return {k: v.detach().cpu().to(dtype).clone() for k, v in m.base_model.state_dict().items()}


def _batch(seed=1, V=CFG["vocab_size"]):
    g = torch.Generator().manual_seed(seed)
    B, Ls, Ld = 3, max(SRC_LENS), max(DEC_LENS)
    ids = torch.randint(2, V, (B, Ls), generator=g)
    dec = torch.randint(2, V, (B, Ld), generator=g)
    dec[:, 0] = 0
    tgt = torch.randint(2, V, (B, Ld), generator=g)
    mask = (torch.arange(Ls)[None] < torch.tensor(SRC_LENS)[:, None]).long()
    dmask = (torch.arange(Ld)[None] < torch.tensor(DEC_LENS)[:, None]).long()
    return ids * mask, mask, dec * dmask, dmask, tgt


@pytest.fixture(scope="module")
def oracle():
    """the model (CPU), the batch and the statement's logits in fp64, fp32 and fp32 under autocast(bf16); computed
    once and only read"""
    m = _model()
    ids, mask, dec, dmask, tgt = _batch()
    out = dict(model=m, batch=(ids, mask, dec, dmask, tgt))
    with torch.no_grad():
        out["f64"] = ref.pegasus_logits(_params(m, torch.float64), ids, mask, dec, dmask, NH)
        out["f32"] = ref.pegasus_logits(_params(m, torch.float32), ids, mask, dec, dmask, NH)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out["ac"] = ref.pegasus_logits(_params(m, torch.float32), ids, mask, dec, dmask, NH).float()
    for k in ("f64", "f32", "ac"):
        out["loss_" + k] = ref.title_loss_ref(out[k], dmask, tgt)
    return out


def _gpu(m, precision):
    import copy
    g = copy.deepcopy(m).to(DEV)
    g.precision = precision
    return g.eval()


def _rel(a, b):
    return ((a.double().cpu() - b.double()).norm() / b.double().norm()).item()


def test_fp32_parity(oracle):
    m = _gpu(oracle["model"], "fp32")
    ids, mask, dec, dmask, tgt = (t.to(DEV) for t in oracle["batch"])
    want = oracle["f64"]
    with torch.no_grad():
        logits = m(ids, mask, dec, dmask)
        loss, n_correct, n_valid = m.title_loss(ids, mask, dec, dmask, tgt)
    torch.cuda.synchronize()
    assert logits.dtype == torch.float32 and tuple(logits.shape) == tuple(want.shape)
    e = (logits.double().cpu() - want).abs().max().item()
    e32 = (oracle["f32"].double() - want).abs().max().item()
    print(f"fp32 logits: max err {e:.3e}, the statement in fp32 on the CPU {e32:.3e}, max|ref| {want.abs().max():.3f}")
    assert e <= 4 * e32 + 1e-6 * want.abs().max().item()
    l64, c64, v64 = oracle["loss_f64"]
    el, el32 = abs(loss.item() - l64.item()), abs(oracle["loss_f32"][0].item() - l64.item())
    print(f"fp32 title_loss {loss.item():.7f} exact {l64.item():.7f}: err {el:.3e}, the statement in fp32 {el32:.3e}")
    assert el <= 4 * el32 + 1e-6 * abs(l64.item())
    assert n_valid == v64 == sum(DEC_LENS) and int(n_correct) == c64


def test_bf16(oracle):
    m = _gpu(oracle["model"], "bf16")
    ids, mask, dec, dmask, tgt = (t.to(DEV) for t in oracle["batch"])
    want = oracle["f64"]
    with torch.no_grad():
        logits = m(ids, mask, dec, dmask)
        loss, n_correct, n_valid = m.title_loss(ids, mask, dec, dmask, tgt)
    torch.cuda.synchronize()
    e, e_ac = _rel(logits, want), _rel(oracle["ac"], want)
    print(f"bf16 logits: rel err {e:.3e}, autocast on the CPU {e_ac:.3e}, ratio {e / e_ac:.2f}")
    assert logits.dtype == torch.float32 and e <= 1.5 * e_ac
    l64 = oracle["loss_f64"][0].item()
    el, el_ac = abs(loss.item() - l64), abs(oracle["loss_ac"][0].item() - l64)
    print(f"bf16 title_loss {loss.item():.6f} exact {l64:.6f}: err {el:.3e}, autocast {el_ac:.3e}")
    assert el <= 1.5 * el_ac + 1e-3 and n_valid == sum(DEC_LENS)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_padded_source_columns_do_not_matter(oracle, precision):
    m = _gpu(oracle["model"], precision)
    ids, mask, dec, dmask, _ = (t.to(DEV) for t in oracle["batch"])
    other = torch.where(mask != 0, ids, torch.randint_like(ids, 2, CFG["vocab_size"]))
    assert not torch.equal(other, ids)
    with torch.no_grad():
        a, b = m(ids, mask, dec, dmask), m(other, mask, dec, dmask)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _plant_eos(m, P64, ids, mask):
    """an untied head whose EOS row points along what sets sequence 1's hidden state at step 3 of the unplanted greedy
    run apart from the other two sequences': the EOS then comes at a step that depends on the source"""
    _, _, hid = ref.greedy_ref(P64, ids, mask, NH, MAX_LEN)
    v = hid[1, 3] - 0.5 * (hid[0, 3] + hid[2, 3])
    with torch.no_grad():
        m.base_model.lm_head.weight[1] = (5.0 * v / v.norm() ** 2).float()


def _assert_greedy(tokens, lengths, want, margins, eos=1):
    """tokens / lengths of generate_ids against the statement's uncut tokens `want` [B, MAX_LEN]"""
    ok = margins > 1e-3
    assert ok.float().mean().item() >= 0.9, f"only {ok.float().mean().item():.2f} of the steps have a margin > 1e-3"
    for b in range(want.shape[0]):
        n = MAX_LEN
        for t in range(MAX_LEN):
            if int(want[b, t]) == eos:
                n = t + 1
                break
        clear = bool(ok[b, :n].all())
        for t in range(n):
            if t >= tokens.shape[1]:
                assert clear is False, (b, t)
                break
            if ok[b, t]:
                assert int(tokens[b, t]) == int(want[b, t]), (b, t, tokens[b], want[b])
            elif int(tokens[b, t]) != int(want[b, t]):
                break  # (a tie within 1e-3 went the other way: the sequences differ from here on)
        if clear:
            assert int(lengths[b]) == n and not tokens[b, n:].any()
    return ok


def test_generate_ids_greedy_fp32():
    cpu = _model(seed=11, reinit_head=True)
    ids, mask, _, _, _ = _batch()
    _plant_eos(cpu, _params(cpu, torch.float64), ids, mask)
    P64 = _params(cpu, torch.float64)
    want, margins, _ = ref.greedy_ref(P64, ids, mask, NH, MAX_LEN)
    first_eos = [(row.tolist() + [1]).index(1) + 1 for row in want]
    print(f"the statement's greedy tokens {want.tolist()}, lengths {[min(n, MAX_LEN) for n in first_eos]}, "
          f"smallest margin {margins.min().item():.3e}")
    assert min(first_eos) < MAX_LEN and len(set(first_eos)) > 1  # EOS cuts come, at different steps
    m = _gpu(cpu, "fp32")
    tokens, lengths = m.generate_ids(ids.to(DEV), mask.to(DEV), max_len=MAX_LEN)
    assert tokens.dtype == torch.int64 and tokens.shape[0] == 3 and tokens.shape[1] == int(lengths.max())
    ok = _assert_greedy(tokens, lengths, want, margins)

    # generate on batch row 0 (its source is unpadded): a stub tokenizer whose tokens are the ids themselves
    class Tok:
        def tokenize(self, text):
            return text.split()

        def convert_tokens_to_ids(self, toks):
            return [int(t) for t in toks]

        def decode(self, ids_):
            return " ".join(str(i) for i in ids_)

    assert bool(ok[0].all())  # (a condition on the statement: row 0 has no near-tie)
    text, logits = m.generate(" ".join(str(int(i)) for i in ids[0]) + " 9 9 9", Tok(), DEV, max_text_len=SRC_LENS[0],
                              max_len=MAX_LEN)
    got = [int(t) for t in text.split()]
    n = int(lengths[0])
    assert got == tokens[0, :n].tolist()
    assert tuple(logits.shape) == (1, n * (n + 1) // 2, CFG["vocab_size"]) and logits.dtype == torch.float32
    # the last step's logits are the statement's on the same prefix
    dec = torch.tensor([[0] + got[:-1]])
    z = ref.pegasus_logits(P64, ids[:1], mask[:1], dec, torch.ones_like(dec), NH)
    assert (logits[0, -n:].double().cpu() - z[0]).abs().max().item() <= 1e-4


def test_generate_ids_sampling_is_reproducible():
    m = _gpu(_model(seed=12), "bf16")
    ids, mask, _, _, _ = _batch()
    g = torch.Generator().manual_seed(5)
    a, la = m.generate_ids(ids.to(DEV), mask.to(DEV), max_len=6, sample=True, top_k=10, temperature=0.8, generator=g)
    g = torch.Generator().manual_seed(5)
    b, lb = m.generate_ids(ids.to(DEV), mask.to(DEV), max_len=6, sample=True, top_k=10, temperature=0.8, generator=g)
    assert torch.equal(a, b) and torch.equal(la, lb) and int(a.max()) < CFG["vocab_size"]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fused_projection_groups(precision):
    """d_model 256 (4 heads): every parameter fills whole 256-element units of the flat buffer, so q | k | v and
    k | v are contiguous and run as one GEMM each"""
    from vcg_hip import ops
    from vcg_hip.pegasus import PegasusEngine
    cfg = dict(d_model=256, encoder_attention_heads=4, decoder_attention_heads=4, encoder_layers=1, decoder_layers=1)
    cpu = _model(seed=13, **cfg)
    ids, mask, dec, dmask, _ = _batch()
    with torch.no_grad():
        want = ref.pegasus_logits(_params(cpu, torch.float64), ids, mask, dec, dmask, 4)
    m = _gpu(cpu, precision)
    args = [t.to(DEV) for t in (ids, mask, dec, dmask)]
    out = {}
    for on in (True, False):
        PegasusEngine.fuse_proj = on
        try:
            ops.gemm_census_enable(True)
            with torch.no_grad():
                out[on] = m(*args)
            torch.cuda.synchronize()
            keys = ops.gemm_census()
            ops.gemm_census_enable(False)
        finally:
            PegasusEngine.fuse_proj = True
        wide = sum(v for k, v in keys.items() if " N=768 " in k or " N=512 " in k)
        assert (wide >= 3) if on else (wide == 0), keys  # [3H, H] x 2 and [2H, H] x 1; (the head has N = 520)
    tol = 2e-5 if precision == "fp32" else 3e-2
    assert _rel(out[True], want) <= tol and _rel(out[False], want) <= tol


def test_forward_refuses_training(oracle):
    m = _gpu(oracle["model"], "fp32")
    ids, mask, dec, dmask, _ = (t.to(DEV) for t in oracle["batch"])
    with pytest.raises(NotImplementedError, match="training"):
        m.train()(ids, mask, dec, dmask)
    m.eval()
    with pytest.raises(NotImplementedError, match="training"):  # grad enabled on parameters that require it
        m(ids, mask, dec, dmask)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        with torch.no_grad():
            m(ids.repeat(1, 2), mask.repeat(1, 2), dec, dmask)
