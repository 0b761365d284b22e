"""The MoCo-specific part of BertHugfaceConstrast (reference model/lang/bert_hugface_constrast.py:97-165) on
csrc/contrast.hip.

`L2NormFn`: F.normalize(x, dim=1) of the pooled output, fp32 statistics. The backward computes dx in fp32; autograd
hands it on in the input's dtype, so in bf16 mode BertFn receives it rounded to bf16 (as it does every pooled gradient).

`InfoNceLossFn`: the fused loss. The reference enqueues the new keys right after forming the logits (:163), so a
backward that recomputed the tiles from the live queue would see N overwritten rows: d loss / dq for a unit upstream
gradient is computed INSIDE the forward call, before the caller's enqueue, and kept as fp32 [N, H]; the backward only
scales it by the incoming scalar. No gradient flows to k or to the queue (the reference's keys are detached).

`InfoNceLogitsFn`: the drop-in forward's logits [N, 1 + K]. Its backward needs the queue as it was and keeps a copy of
the operand queue, as the reference's `queue.clone()` does: the compatibility path, not the fast one.
"""
import torch

from . import ops


class L2NormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        y, denom = ops.l2norm_fwd(x)
        ctx.save_for_backward(x, denom)
        return y

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return None
        x, denom = ctx.saved_tensors
        return ops.l2norm_bwd(dy.to(torch.float32).contiguous(), x, denom)


class InfoNceLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, queue_km, K, inv_T):
        ctx.set_materialize_grads(False)
        want_dq = ctx.needs_input_grad[0]
        _, _, loss, n_correct, dq, _ = ops.infonce(q.contiguous(), k.contiguous(), queue_km, K, inv_T, want_dq=want_dq)
        ctx.dq = dq
        ctx.mark_non_differentiable(n_correct)
        return loss, n_correct

    @staticmethod
    def backward(ctx, dloss, _dn):
        if dloss is None or ctx.dq is None:
            return None, None, None, None, None
        return ctx.dq * dloss.to(torch.float32), None, None, None, None


class InfoNceLogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, queue_km, K, inv_T):
        ctx.set_materialize_grads(False)
        q, k = q.contiguous(), k.contiguous()
        _, _, _, _, _, logits = ops.infonce(q, k, queue_km, K, inv_T, want_logits=True)
        ctx.K, ctx.inv_T = K, inv_T
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(k, queue_km.clone())
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        if dlogits is None:
            return None, None, None, None, None
        k, km = ctx.saved_tensors
        K, (Kp, H), N = ctx.K, km.shape, k.shape[0]
        dl = dlogits.to(torch.float32)
        dz = torch.zeros((N, Kp), dtype=torch.float32, device=dl.device)
        dz[:, :K].copy_(dl[:, 1:])
        if km.dtype == torch.bfloat16:
            dq = torch.empty((N, H), dtype=torch.float32, device=dl.device)
            ops.gemm_splitk(ops.cast_from_f32(dz, torch.bfloat16), km, dq, N, H, K, Kp, H, transA=False, transB=True,
                            accumulate=False)
        else:
            dq = ops.gemm(dz, km, N, H, Kp, Kp, H, transB=True)
        dq = (dq + dl[:, 0:1] * k.to(torch.float32)) * ctx.inv_T
        return dq, None, None, None, None
