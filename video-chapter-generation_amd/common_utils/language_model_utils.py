"""Drop-in for reference common_utils/language_model_utils.py:6-42: `top_k_logits` and `token_idx_sample`, the GPT
stage's text sampler (train_lang/test_gpt_hugface.py).

A model with `generate` (model/lang/gpt_hugface.py:GPTHugface) samples on its KV cache with the fused top-k sampler
(vcg_hip/gpt_decode.py); its random draws come from torch.rand, not torch.multinomial, so for one seed the tokens differ
from the reference's while their distribution is the same. Any other model runs the plain loop below, whose draws are
torch.multinomial's. (`token_embedding_sample`, the sampler of the reference's own minGPT over word embeddings, has no
counterpart: that model is not part of this project.)
"""
import torch
from torch.nn import functional as F


def top_k_logits(logits, k):
    """logits [B, V] with everything below each row's k-th largest value set to -inf; entries equal to the k-th value
    all stay."""
    kth = torch.topk(logits, k).values[:, -1:]
    return logits.masked_fill(logits < kth, float("-inf"))


@torch.no_grad()
def token_idx_sample(model, x, steps, temperature=1.0, sample=False, top_k=None, generator=None):
    """Extend the token ids x [B, T] by `steps` tokens, each predicted from the sequence so far, the context cropped
    to its last `steps` tokens (the reference uses the step count as the block size). Returns (x with the new columns
    [B, T + steps], the new ids: a list of ints for B = 1, of per-step lists otherwise). The model is left in eval
    mode."""
    if hasattr(model, "generate"):
        block = steps
        n_pos = getattr(getattr(getattr(model, "base_model", None), "config", None), "n_positions", None)
        if n_pos is not None:
            block = min(block, n_pos)
        seq, new = model.generate(x, None, steps=steps, temperature=temperature, sample=sample, top_k=top_k,
                                  block_size=block, generator=generator)
        ids = new.cpu()
        return seq, (ids[0].tolist() if ids.shape[0] == 1 else ids.t().tolist())
    model.eval()
    new_ids = []
    for _ in range(steps):
        context = x[:, -steps:] if x.size(1) > steps else x
        z = model(context)[0][:, -1, :] / temperature
        if top_k is not None:
            z = top_k_logits(z, top_k)
        p = F.softmax(z, dim=-1)
        nxt = torch.multinomial(p, 1, generator=generator) if sample else p.argmax(dim=-1, keepdim=True)
        x = torch.cat((x, nxt), dim=1)
        col = nxt[:, 0].tolist()
        new_ids.append(col[0] if len(col) == 1 else col)
    return x, new_ids
