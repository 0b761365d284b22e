"""BERT attention forward + backward alone, fused (bert_attn.hip / bert_attn_long.hip) vs unfused (QK^T GEMM -> softmax ->
PV GEMM), B = 64, 12 heads, p = 0.1, L = 128 .. 512 (device events over 20 calls; profiles/long_text_attn_ab.txt). With
VCG_LIB_PATH it times another build of the library: the fused lines of the parent's and this tree's are compared in
profiles/bert_attn_shared_ab.txt and profiles/attn_dkv_shared_ab.txt (--fused-only: only those lines)."""
import sys, os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "video-chapter-generation_amd"))
import torch
from vcg_hip import _lib
from vcg_hip.bert import attention_fwd, attention_bwd
_lib.call("vcg_init", 0)
B, nh, H = 64, 12, 768
for L in (128, 256, 384, 512):
    Lp = L
    qkv = (torch.randn(B * L + 8, 3 * H) * 1.5).to(torch.bfloat16).cuda()
    dctx = torch.randn(B * L, H).to(torch.bfloat16).cuda()
    n = torch.randint(L // 2, L + 1, (B,))
    mask = (torch.arange(L)[None, :] < n[:, None]).to(torch.int64).cuda()
    for fused in ((True,) if "--fused-only" in sys.argv[1:] else (True, False)):
        ts = []
        for which in ("fwd", "bwd"):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ctx, att = attention_fwd(qkv, mask, B, nh, L, Lp, 64, 0.125, 0.1, 5, fused)
            for it in range(23):
                if it == 3:
                    ev[0].record()
                if which == "fwd":
                    ctx, att = attention_fwd(qkv, mask, B, nh, L, Lp, 64, 0.125, 0.1, 5, fused)
                else:
                    d = attention_bwd(qkv, dctx, ctx, mask, att, B, nh, L, Lp, 64, 0.125, 0.1, 5)
            ev[1].record()
            torch.cuda.synchronize()
            ts.append(ev[0].elapsed_time(ev[1]) / 20)
        fl = 4.0 * L * L * 64 * B * nh
        print(f"L={L} {'fused  ' if fused else 'unfused'} fwd {ts[0]*1e3:8.1f} us ({fl/ts[0]/1e9:6.1f} TF/s useful)  "
              f"bwd {ts[1]*1e3:8.1f} us ({2.5*fl/ts[1]/1e9:6.1f} TF/s useful)", flush=True)
