"""The listwise part of model/lang/bert_hugface_listnet.py's BertHugface (reference :148-176) on csrc/listnet.hip.

`ListNetLossFn`: the slate loss (softmax over <boundary clip, contrast clip> of the pooled output, cross-entropy against
the soft targets with the reference's 1e-10 inside the log) and the 2-way boundary head with its cross-entropy, one
forward launch (plus a one-workgroup mean) and one backward launch. The forward keeps p [B, S - 1] and the head's
probabilities; the backward writes dP in fp32 -- autograd hands it on in the pooled output's dtype, so in bf16 mode
BertFn receives it rounded to bf16, as it does every pooled gradient.

As in functions.py / mlm.py the head's parameters are not Function inputs: the kernel reads the fp32 masters and adds
their gradients into the flat .grad buffer, and `hooks` (DDP) is told when they are final. `binary_logits` and
`binary_prob` are outputs for reading (the driver's scores): no gradient flows back through them.
"""
import torch

from . import ops


class ListNetLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pooled, anchor, head, targets, idx, hooks):
        """-> (loss, binary_logits [M, 2], binary_prob [M, 2], parts [2] = surrogate, binary)"""
        ctx.set_materialize_grads(False)
        pooled = pooled.contiguous()
        W, bias = head.weight.data, head.bias.data
        loss3, logits, prob, p, idx = ops.listnet_fwd(pooled, targets, idx, None, W, bias)
        ctx.head, ctx.idx, ctx.hooks = head, idx, hooks
        ctx.save_for_backward(pooled, targets, p, prob)
        parts = loss3[1:]
        ctx.mark_non_differentiable(logits, prob, parts)
        return loss3[0], logits, prob, parts

    @staticmethod
    def backward(ctx, dloss, _dlogits, _dprob, _dparts):
        if dloss is None:
            return (None,) * 6
        pooled, targets, p, prob = ctx.saved_tensors
        head = ctx.head
        train_head = head.weight.requires_grad
        if train_head != head.bias.requires_grad:
            raise RuntimeError("ListNetLossFn: the boundary head's weight and bias must be trained or frozen together")
        if train_head and (head.weight.grad is None or head.bias.grad is None):
            raise RuntimeError("ListNetLossFn: the head has no gradient buffers (call native_flat() on the root)")
        dP = ops.listnet_bwd(pooled, targets, ctx.idx, head.weight.data, p, prob,
                             dloss.to(torch.float32).reshape(1).contiguous(),
                             dW=head.weight.grad if train_head else None, db=head.bias.grad if train_head else None)
        if train_head and ctx.hooks is not None:
            ctx.hooks([head.weight, head.bias])
        return dP, None, None, None, None, None
