"""Masked-LM vocabulary head of BertHugface(pretrain_stage=True) (reference model/lang/bert_hugface.py:98-132, trained
by pretrain_lang_model_hugface.py:127-150) on csrc/mlm_head.hip.

`MlmLossFn`: the fused loss over the masked rows only. bf16: vcg_mlm_loss_fwd projects hidden[rows] onto the vocabulary
and reduces it on the fly (nothing R x V is stored); the backward recomputes the tiles into ONE bf16 [R, Vp] dZ, from
which dX = dZ W (split over the long K = V, fp32 out) and head.weight.grad += dZ^T X. fp32 parity mode: the masked
rows' logits by the fp32 vcg_gemm, reduced by the same finalize kernel.

`MlmLogitsFn`: the drop-in forward's logits of every position, fp32 [B L, Vp] (returned as a [..., :V] view).

As in functions.py the head weight is not a Function input: its gradient is accumulated by the kernels into the flat
.grad buffer, and `hooks` (DDP) is told when it is final.
"""
import numpy as np
import torch

from . import ops


def _head_weights(root, head, dtype):
    """(W in the compute dtype [V, H], W padded with zero rows to [Vp, H] for the fp32 GEMMs or None)."""
    # (the caller's native_flat() -- BertHugface._last_hidden -- has validated the buffers and refreshed the bf16 shadow
    # for this forward; walking every parameter again costs more host time than the fused loss' kernels run)
    flat = getattr(root, "_vcg_flat", None)
    if flat is None or id(head.weight) not in flat.index:
        flat = root.native_flat()
    W = flat.compute_view(head.weight, dtype)
    if dtype != torch.float32:
        return W, None
    V, H = W.shape
    Wp = torch.zeros((ops.mlm_vp(V), H), dtype=torch.float32, device=W.device)
    Wp[:V].copy_(W)
    return W, Wp


def _dx_dw(dz, x, W, Wp, head, hooks):
    """dz [M, Vp] (pad columns zero), x [M, H] -> dX fp32 [M, H]; head.weight.grad += dz^T x."""
    M, Vp = dz.shape
    V, H = W.shape
    if Wp is not None:  # fp32: the padded weight makes K = Vp a whole number of 16-byte vectors
        dx = ops.gemm(dz, Wp, M, H, Vp, Vp, H, transB=True)
    else:  # bf16: a skinny output over K = V -- split over K, fp32 out
        dx = torch.empty((M, H), dtype=torch.float32, device=dz.device)
        ops.gemm_splitk(dz, W, dx, M, H, V, Vp, H, transA=False, transB=True, accumulate=False)
    if head.weight.requires_grad:
        ops.gemm_splitk(dz, x, head.weight.grad, V, H, M, Vp, H, transA=True, transB=True, accumulate=True)
        if hooks is not None:
            hooks([head.weight])
    return dx


class MlmLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, anchor, root, head, rows, targets, hooks):
        ctx.set_materialize_grads(False)
        dt = hidden.dtype
        W, Wp = _head_weights(root, head, dt)
        V, H = W.shape
        R = targets.numel()
        hidden = hidden.contiguous()
        ctx.root_head, ctx.hooks, ctx.n_rows = (head, W, Wp), hooks, hidden.shape[0]
        if dt == torch.bfloat16:
            lse, _, loss, n_correct = ops.mlm_loss_fwd(hidden, rows, W, targets)
            ctx.save_for_backward(hidden, rows, targets, lse)
        else:
            x = hidden.index_select(0, rows)
            logits = ops.gemm(x, Wp, R, Wp.shape[0], H, H, H)
            lse, _, loss, n_correct = ops.mlm_reduce_f32(logits, V, targets)
            ctx.save_for_backward(x, rows, targets, lse, logits)
        ctx.mark_non_differentiable(n_correct)
        return loss, n_correct

    @staticmethod
    def backward(ctx, dloss, _dn):
        if dloss is None:
            return (None,) * 7
        head, W, Wp = ctx.root_head
        dloss = dloss.to(torch.float32).contiguous()
        if Wp is None:
            hidden, rows, targets, lse = ctx.saved_tensors
            dz = ops.mlm_loss_bwd(hidden, rows, W, targets, lse, dloss)
            x = hidden.index_select(0, rows)
        else:
            if getattr(ctx, "logits_used", False):
                raise RuntimeError("MlmLossFn (fp32): a second backward would need the logits the first one overwrote")
            x, rows, targets, lse, logits = ctx.saved_tensors
            dz = ops.mlm_dz_f32(logits, W.shape[0], lse, targets, dloss)  # (in place: the logits are done with)
            ctx.logits_used = True
        dx = _dx_dw(dz, x, W, Wp, head, ctx.hooks)
        dh = torch.zeros((ctx.n_rows, x.shape[1]), dtype=dx.dtype, device=dx.device)
        dh.index_copy_(0, rows, dx)  # (the rows are distinct positions)
        return dh, None, None, None, None, None, None


class MlmLogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, anchor, root, head, hooks):
        ctx.set_materialize_grads(False)
        dt = hidden.dtype
        W, Wp = _head_weights(root, head, dt)
        hidden = hidden.contiguous()
        ctx.root_head, ctx.hooks = (head, W, Wp), hooks
        ctx.save_for_backward(hidden)
        if dt == torch.bfloat16:
            return ops.mlm_logits(hidden, W)
        M, H = hidden.shape
        return ops.gemm(hidden, Wp, M, Wp.shape[0], H, H, H)

    @staticmethod
    def backward(ctx, dlogits):
        if dlogits is None:
            return (None,) * 5
        head, W, Wp = ctx.root_head
        (hidden,) = ctx.saved_tensors
        dz = dlogits.to(torch.float32).contiguous()  # [M, Vp]; the [..., :V] view's gradient has zero pad columns
        if Wp is None:
            dz = ops.cast_from_f32(dz, torch.bfloat16)
        return _dx_dw(dz, hidden, W, Wp, head, ctx.hooks), None, None, None, None


def select_targets(targets, vocab_size):
    """Host side of the loss: targets [B, L] (-1 = ignored, the reference's Y_PAD) -> (rows int64 [R] = flat b L + t of
    the masked positions in order, their targets int64 [R]) as CPU tensors. A target outside [0, V) other than -1 is a
    ValueError."""
    t = targets.detach().to("cpu", torch.int64).reshape(-1).numpy()
    if ((t < -1) | (t >= vocab_size)).any():
        bad = t[(t < -1) | (t >= vocab_size)]
        raise ValueError(f"mlm_loss: target {int(bad[0])} outside [0, {vocab_size}) (-1 marks an ignored position)")
    rows = np.flatnonzero(t != -1).astype(np.int64)
    return torch.from_numpy(rows), torch.from_numpy(t[rows].copy())
