"""Module trees with the reference's parameter names, executed by the native engines.

* `ResNet50`  — torchvision.models.resnet50 topology (v1.5) so `Resnet50TSM.base_model` state-dict
  keys match (`conv1.weight`, `layer1.0.conv1.net.weight` once TSM-wrapped, `bn*.running_mean`, ...).
* `BertModel` — HF transformers BertModel names (`embeddings.word_embeddings.weight`,
  `encoder.layer.N.attention.self.query.weight`, `pooler.dense.weight`, ...), built from a config
  (the reference's `from_pretrained('bert-base-uncased')` needs the network; a local checkpoint
  can be loaded with load_state_dict).
* `NativeRoot` — mixin owning the flat parameter buffers and the compute precision.
"""
import math

import torch
from torch import nn

from . import flat as flatmod
from . import ops


# ============================================================================ native root
class NativeRoot:
    """Mixin for modules whose forward runs on libvcg_hip.

    precision: "fp32" (parity mode; f32-input MFMA) or "bf16" (bf16 activations and MFMA operands,
    fp32 accumulation / statistics / master weights)."""

    _vcg_precision = "fp32"

    @property
    def precision(self):
        return self._vcg_precision

    @precision.setter
    def precision(self, value):
        if value not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        for m in self.modules():
            if isinstance(m, NativeRoot):
                object.__setattr__(m, "_vcg_precision", value)

    def compute_dtype(self):
        return ops.torch_dtype(self.precision)

    def native_flat(self):
        params = list(self.parameters())
        if not params:
            raise RuntimeError("module has no parameters")
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError(
                f"{type(self).__name__}: the native MI355X path needs the module on the GPU (model.to('cuda')); "
                "there is no CPU fallback")
        dt = self.compute_dtype()
        want_shadow = None if dt == torch.float32 else dt
        f = getattr(self, "_vcg_flat", None)
        ok = (f is not None and f.device == dev and f.shadow_dtype == want_shadow and len(f.params) >= len(params)
              and all(id(p) in f.index for p in (params[0], params[-1])) and f.intact())
        if not ok:
            named = list(self.named_parameters())
            f = flatmod.FlatParams(named, dev, shadow_dtype=want_shadow, order=_flat_order([n for n, _ in named]))
            for m in self.modules():
                object.__setattr__(m, "_vcg_flat", f)
            self._bind_bn_counters(dev)
        f.refresh_shadow()
        return f

    # one int64 buffer for every BatchNorm's num_batches_tracked -> one increment per step
    def _bind_bn_counters(self, dev):
        bns = [m for m in self.modules() if isinstance(m, nn.BatchNorm2d) and m.num_batches_tracked is not None]
        if not bns:
            object.__setattr__(self, "_vcg_bn_counter", None)
            return
        buf = torch.stack([b.num_batches_tracked.detach().to(dev) for b in bns]).reshape(-1)
        for i, b in enumerate(bns):
            b._buffers["num_batches_tracked"] = buf[i]
        object.__setattr__(self, "_vcg_bn_counter", (buf, bns))

    def _bump_bn_counters(self):
        c = getattr(self, "_vcg_bn_counter", None)
        if c is None:
            return
        buf, bns = c
        if all(b._buffers.get("num_batches_tracked") is not None and
               b.num_batches_tracked.data_ptr() == buf[i].data_ptr() for i, b in enumerate(bns)):
            flags = [b.training and b.track_running_stats for b in bns]
            if all(flags):
                buf.add_(1)
                return
        for b in bns:
            if b.training and b.track_running_stats and b.num_batches_tracked is not None:
                b.num_batches_tracked.add_(1)

    def zero_grad(self, set_to_none=True):  # noqa: D401 - keeps grads as flat views
        f = getattr(self, "_vcg_flat", None)
        if f is not None and f.intact():
            f.zero_grad()
        else:
            super().zero_grad(set_to_none=set_to_none)

    def _anchor(self, dev):
        a = getattr(self, "_vcg_anchor", None)
        if a is None or a.device != dev:
            a = torch.zeros(0, device=dev, requires_grad=True)
            object.__setattr__(self, "_vcg_anchor", a)
        return a


def _flat_order(names):
    """Layout order: keep module order but put each BERT layer's query/key/value weights (and
    biases) back to back so the fused QKV GEMM reads one [3H, H] view."""
    out, seen = [], set()
    for n in names:
        if n in seen:
            continue
        if n.endswith("attention.self.query.weight"):
            pre = n[: -len("query.weight")]
            grp = [pre + "query.weight", pre + "key.weight", pre + "value.weight",
                   pre + "query.bias", pre + "key.bias", pre + "value.bias"]
            for g in grp:
                if g in names and g not in seen:
                    out.append(g)
                    seen.add(g)
            continue
        # Pegasus (module order k, v, q): the self-attention's q | k | v and the cross-attention's k | v back to back
        for suffix, members in (("self_attn.k_proj.weight", ("q_proj", "k_proj", "v_proj")),
                                ("encoder_attn.k_proj.weight", ("k_proj", "v_proj"))):
            if n.endswith(suffix):
                pre = n[: -len("k_proj.weight")]
                for g in [pre + m + ".weight" for m in members] + [pre + m + ".bias" for m in members]:
                    if g in names and g not in seen:
                        out.append(g)
                        seen.add(g)
                break
        else:
            out.append(n)
            seen.add(n)
    return out


def new_seed():
    return int(torch.randint(0, 2 ** 62, (1,)).item())


# ============================================================================ ResNet-50
class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


class Identity(nn.Module):
    def forward(self, x):
        return x


class ResNet50(NativeRoot, nn.Module):
    """torchvision resnet50 topology; forward(x [N,3,H,W] fp32) -> [N, 2048] (fc = Identity)."""

    def __init__(self, num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(64, 3)
        self.layer2 = self._make_layer(128, 4, stride=2)
        self.layer3 = self._make_layer(256, 6, stride=2)
        self.layer4 = self._make_layer(512, 3, stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(2048, num_classes)
        for m in self.modules():  # torchvision init
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * 4:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * 4, 1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * 4))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * 4
        for _ in range(1, blocks):
            layers.append(Bottleneck(self.inplanes, planes))
        return nn.Sequential(*layers)

    def forward(self, x):
        if not isinstance(self.fc, Identity):
            raise RuntimeError("native ResNet50 implements the fc=Identity trunk (Resnet50TSM / TwoStream usage)")
        from .functions import TrunkFn
        from .trunk import ResNetTrunk
        self.native_flat()
        need_grad = torch.is_grad_enabled()
        if self.training:
            self._bump_bn_counters()
        eng = ResNetTrunk(self, self.compute_dtype())
        return TrunkFn.apply(x.float().contiguous(), self._anchor(x.device), eng, need_grad, None)


# ============================================================================ BERT
class BertConfig:
    """The subset of transformers.BertConfig the encoder uses (bert-base-uncased defaults)."""

    def __init__(self, vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                 intermediate_size=3072, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
                 max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12, pad_token_id=0,
                 initializer_range=0.02, output_attentions=False, **kwargs):
        self.vocab_size = vocab_size
        self.hidden_size = hidden_size
        self.num_hidden_layers = num_hidden_layers
        self.num_attention_heads = num_attention_heads
        self.intermediate_size = intermediate_size
        self.hidden_dropout_prob = hidden_dropout_prob
        self.attention_probs_dropout_prob = attention_probs_dropout_prob
        self.max_position_embeddings = max_position_embeddings
        self.type_vocab_size = type_vocab_size
        self.layer_norm_eps = layer_norm_eps
        self.pad_token_id = pad_token_id
        self.initializer_range = initializer_range
        self.output_attentions = output_attentions
        for k, v in kwargs.items():
            setattr(self, k, v)


class _Embeddings(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.word_embeddings = nn.Embedding(c.vocab_size, c.hidden_size, padding_idx=c.pad_token_id)
        self.position_embeddings = nn.Embedding(c.max_position_embeddings, c.hidden_size)
        self.token_type_embeddings = nn.Embedding(c.type_vocab_size, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)


class _SelfAttn(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.query = nn.Linear(c.hidden_size, c.hidden_size)
        self.key = nn.Linear(c.hidden_size, c.hidden_size)
        self.value = nn.Linear(c.hidden_size, c.hidden_size)
        self.dropout = nn.Dropout(c.attention_probs_dropout_prob)


class _SelfOut(nn.Module):
    def __init__(self, c, din):
        super().__init__()
        self.dense = nn.Linear(din, c.hidden_size)
        self.LayerNorm = nn.LayerNorm(c.hidden_size, eps=c.layer_norm_eps)
        self.dropout = nn.Dropout(c.hidden_dropout_prob)


class _Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.self = _SelfAttn(c)
        self.output = _SelfOut(c, c.hidden_size)


class _Intermediate(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.intermediate_size)


class _Layer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attention = _Attention(c)
        self.intermediate = _Intermediate(c)
        self.output = _SelfOut(c, c.intermediate_size)


class _Encoder(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.layer = nn.ModuleList([_Layer(c) for _ in range(c.num_hidden_layers)])


class _Pooler(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.dense = nn.Linear(c.hidden_size, c.hidden_size)


class BertOutput:
    """Subset of transformers' BaseModelOutputWithPoolingAndCrossAttentions."""

    def __init__(self, last_hidden_state, pooler_output):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = pooler_output
        self.attentions = None

    def __getitem__(self, i):
        return (self.last_hidden_state, self.pooler_output)[i]


class BertModel(NativeRoot, nn.Module):
    def __init__(self, config=None, add_pooling_layer=True):
        super().__init__()
        self.config = config if config is not None else BertConfig()
        c = self.config
        self.embeddings = _Embeddings(c)
        self.encoder = _Encoder(c)
        self.pooler = _Pooler(c) if add_pooling_layer else None
        self._init_weights()

    def _init_weights(self):
        std = self.config.initializer_range
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0.0, std)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, 0.0, std)
                if m.padding_idx is not None:
                    with torch.no_grad():
                        m.weight[m.padding_idx].zero_()
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def check_text_len(self, L):
        """A text longer than the position table would read past it (vcg_embed_ln_fwd indexes it by position)."""
        P = self.config.max_position_embeddings
        if L > P:
            raise ValueError(f"BertModel: text length {L} exceeds max_position_embeddings {P}")

    def native_forward(self, input_ids, attention_mask, hooks=None):
        """Returns (pooled, last_hidden) in the compute dtype (autograd-connected)."""
        self.check_text_len(input_ids.shape[-1])
        from .bert import BertEncoderEngine
        from .functions import BertFn
        f = self.native_flat()
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        eng = BertEncoderEngine(self, f, self.compute_dtype())
        return BertFn.apply(input_ids, attention_mask, self._anchor(input_ids.device), eng, torch.is_grad_enabled(),
                            new_seed(), hooks)

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, **kwargs):
        if token_type_ids is not None and bool((token_type_ids != 0).any()):
            raise NotImplementedError("native BertModel supports token_type_ids == 0 (the reference passes none)")
        B, L = input_ids.shape
        self.check_text_len(L)
        pooled, last = self.native_forward(input_ids, attention_mask)
        return BertOutput(last.view(B, L, -1), pooled)


# ============================================================================ OpenAI GPT
class OpenAIGPTConfig:
    """The subset of transformers.OpenAIGPTConfig the decoder uses (openai-gpt defaults). afn "gelu" is transformers'
    NewGELUActivation (the tanh form), as ACT_FNS resolves it there."""

    def __init__(self, vocab_size=40478, n_positions=512, n_embd=768, n_layer=12, n_head=12, afn="gelu",
                 resid_pdrop=0.1, embd_pdrop=0.1, attn_pdrop=0.1, layer_norm_epsilon=1e-5, initializer_range=0.02,
                 **kwargs):
        self.vocab_size = vocab_size
        self.n_positions = n_positions
        self.n_embd = n_embd
        self.n_layer = n_layer
        self.n_head = n_head
        self.afn = afn
        self.resid_pdrop = resid_pdrop
        self.embd_pdrop = embd_pdrop
        self.attn_pdrop = attn_pdrop
        self.layer_norm_epsilon = layer_norm_epsilon
        self.initializer_range = initializer_range
        for k, v in kwargs.items():
            setattr(self, k, v)

    hidden_size = property(lambda self: self.n_embd)
    max_position_embeddings = property(lambda self: self.n_positions)


class Conv1D(nn.Module):
    """transformers.pytorch_utils.Conv1D: a Linear whose weight is stored [in, out] (y = x W + b)."""

    def __init__(self, nf, nx):
        super().__init__()
        self.nf, self.nx = nf, nx
        self.weight = nn.Parameter(torch.empty(nx, nf))
        self.bias = nn.Parameter(torch.zeros(nf))


class _GptAttention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.c_attn = Conv1D(3 * c.n_embd, c.n_embd)
        self.c_proj = Conv1D(c.n_embd, c.n_embd)
        self.attn_dropout = nn.Dropout(c.attn_pdrop)
        self.resid_dropout = nn.Dropout(c.resid_pdrop)


class _GptMLP(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.c_fc = Conv1D(4 * c.n_embd, c.n_embd)
        self.c_proj = Conv1D(c.n_embd, 4 * c.n_embd)
        self.dropout = nn.Dropout(c.resid_pdrop)


class _GptBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.attn = _GptAttention(c)
        self.ln_1 = nn.LayerNorm(c.n_embd, eps=c.layer_norm_epsilon)
        self.mlp = _GptMLP(c)
        self.ln_2 = nn.LayerNorm(c.n_embd, eps=c.layer_norm_epsilon)


class GPTOutput:
    """Subset of transformers' BaseModelOutput."""

    def __init__(self, last_hidden_state):
        self.last_hidden_state = last_hidden_state
        self.hidden_states = self.attentions = None

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class OpenAIGPTModel(NativeRoot, nn.Module):
    """transformers.OpenAIGPTModel (the reference's model/lang/gpt_hugface.py:18) with its parameter names and shapes
    -- `tokens_embed`, `positions_embed`, `h.{i}.attn.c_attn|c_proj`, `ln_1`, `mlp.c_fc|c_proj`, `ln_2`, Conv1D weights
    [in, out] -- so state dicts are interchangeable; executed by vcg_hip/gpt.py's GptEncoderEngine (causal fused
    attention, tanh-GELU epilogues).

    Attention: key j is visible to query i iff j <= i and attention_mask[j] != 0. A query without any visible key is
    uniform over all L keys, which is what transformers computes for a fully masked sequence (its -1e4 causal fill and
    finfo.min padding fill are both absorbed). For a LEFT-padded mask (position 0 masked, a later one not) transformers
    attends to the future valid keys instead, since its causal fill is finite; this model does not. The datasets here
    only pad on the right."""

    def __init__(self, config=None):
        super().__init__()
        self.config = config if config is not None else OpenAIGPTConfig()
        c = self.config
        if c.afn not in ("gelu", "gelu_new"):
            raise NotImplementedError(f"native OpenAIGPTModel implements afn='gelu' (the tanh form), not {c.afn!r}")
        self.tokens_embed = nn.Embedding(c.vocab_size, c.n_embd)
        self.positions_embed = nn.Embedding(c.n_positions, c.n_embd)
        self.drop = nn.Dropout(c.embd_pdrop)
        self.h = nn.ModuleList([_GptBlock(c) for _ in range(c.n_layer)])
        std = c.initializer_range
        for m in self.modules():
            if isinstance(m, (Conv1D, nn.Embedding)):
                nn.init.normal_(m.weight, 0.0, std)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def check_text_len(self, L):
        P = self.config.n_positions
        if L > P:
            raise ValueError(f"OpenAIGPTModel: text length {L} exceeds n_positions {P}")

    def native_forward(self, input_ids, attention_mask, hooks=None):
        """Returns the last hidden state [B L, H] in the compute dtype (autograd-connected)."""
        self.check_text_len(input_ids.shape[-1])
        from .functions import BertFn
        from .gpt import GptEncoderEngine
        f = self.native_flat()
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        eng = GptEncoderEngine(self, f, self.compute_dtype())
        _, last = BertFn.apply(input_ids, attention_mask, self._anchor(input_ids.device), eng,
                               torch.is_grad_enabled(), new_seed(), hooks)
        return last

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, **kwargs):
        if token_type_ids is not None or position_ids is not None:
            raise NotImplementedError("native OpenAIGPTModel takes input_ids and attention_mask (the reference passes "
                                      "nothing else)")
        B, L = input_ids.shape
        return GPTOutput(self.native_forward(input_ids, attention_mask).view(B, L, -1))


# ============================================================================ Pegasus
class PegasusConfig:
    """The subset of transformers.PegasusConfig the model uses (google/pegasus-large defaults)."""

    def __init__(self, vocab_size=96103, d_model=1024, encoder_layers=16, decoder_layers=16,
                 encoder_attention_heads=16, decoder_attention_heads=16, encoder_ffn_dim=4096, decoder_ffn_dim=4096,
                 max_position_embeddings=1024, activation_function="relu", scale_embedding=True, pad_token_id=0,
                 eos_token_id=1, decoder_start_token_id=0, dropout=0.1, attention_dropout=0.1, activation_dropout=0.1,
                 layer_norm_eps=1e-5, init_std=0.02, **kwargs):
        self.vocab_size = vocab_size
        self.d_model = d_model
        self.encoder_layers = encoder_layers
        self.decoder_layers = decoder_layers
        self.encoder_attention_heads = encoder_attention_heads
        self.decoder_attention_heads = decoder_attention_heads
        self.encoder_ffn_dim = encoder_ffn_dim
        self.decoder_ffn_dim = decoder_ffn_dim
        self.max_position_embeddings = max_position_embeddings
        self.activation_function = activation_function
        self.scale_embedding = scale_embedding
        self.pad_token_id = pad_token_id
        self.eos_token_id = eos_token_id
        self.decoder_start_token_id = decoder_start_token_id
        self.dropout = dropout
        self.attention_dropout = attention_dropout
        self.activation_dropout = activation_dropout
        self.layer_norm_eps = layer_norm_eps
        self.init_std = init_std
        for k, v in kwargs.items():
            setattr(self, k, v)

    hidden_size = property(lambda self: self.d_model)


def pegasus_sinusoidal_table(n_pos, dim):
    """transformers' PegasusSinusoidalPositionalEmbedding.create_weight: sin in columns [0, dim/2), cos behind them (not
    interleaved), computed in float64 and rounded to fp32."""
    import numpy as np
    j = np.arange(dim)
    enc = np.arange(n_pos)[:, None] / np.power(10000, 2 * (j // 2) / dim)[None, :]
    out = torch.empty(n_pos, dim, dtype=torch.float32)
    sentinel = dim // 2 if dim % 2 == 0 else dim // 2 + 1
    out[:, :sentinel] = torch.from_numpy(np.sin(enc[:, 0::2])).float()
    out[:, sentinel:] = torch.from_numpy(np.cos(enc[:, 1::2])).float()
    return out


class _PegasusAttention(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.k_proj = nn.Linear(d, d)
        self.v_proj = nn.Linear(d, d)
        self.q_proj = nn.Linear(d, d)
        self.out_proj = nn.Linear(d, d)


class _PegasusLayer(nn.Module):
    def __init__(self, d, ffn, eps, cross):
        super().__init__()
        self.self_attn = _PegasusAttention(d)
        self.self_attn_layer_norm = nn.LayerNorm(d, eps=eps)
        if cross:
            self.encoder_attn = _PegasusAttention(d)
            self.encoder_attn_layer_norm = nn.LayerNorm(d, eps=eps)
        self.fc1 = nn.Linear(d, ffn)
        self.fc2 = nn.Linear(ffn, d)
        self.final_layer_norm = nn.LayerNorm(d, eps=eps)


class _PegasusStack(nn.Module):
    def __init__(self, c, shared, n_layers, ffn, cross):
        super().__init__()
        self.embed_tokens = shared
        self.embed_positions = nn.Embedding(c.max_position_embeddings, c.d_model)
        self.embed_positions.weight.requires_grad = False
        self.layers = nn.ModuleList([_PegasusLayer(c.d_model, ffn, c.layer_norm_eps, cross) for _ in range(n_layers)])
        self.layer_norm = nn.LayerNorm(c.d_model, eps=c.layer_norm_eps)


class _PegasusModel(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.shared = nn.Embedding(c.vocab_size, c.d_model, padding_idx=c.pad_token_id)
        self.encoder = _PegasusStack(c, self.shared, c.encoder_layers, c.encoder_ffn_dim, cross=False)
        self.decoder = _PegasusStack(c, self.shared, c.decoder_layers, c.decoder_ffn_dim, cross=True)


class PegasusForConditionalGeneration(NativeRoot, nn.Module):
    """transformers.PegasusForConditionalGeneration (the reference's model/lang/pegasus_hugface.py:23) with its
    state-dict keys -- `final_logits_bias`, `model.shared`, `model.{encoder,decoder}.embed_tokens` (tied to `shared`),
    `embed_positions` (the sinusoidal table: not trained, a checkpoint may overwrite it), `layers.{i}.self_attn.
    {k,v,q,out}_proj`, `self_attn_layer_norm`, `encoder_attn*` (decoder), `fc1`, `fc2`, `final_layer_norm`,
    `layer_norm`, `lm_head` (tied to `shared`) -- executed by vcg_hip/pegasus.py's PegasusEngine: pre-LayerNorm
    blocks, ReLU, fused self- and cross-attention; inference through encode / cross_kv / decode, training through
    train_forward / train_backward (model.lang.pegasus_hugface.PegasusHugface.title_loss; dropout in train() mode only).

    Not implemented (NotImplementedError): an activation other than relu, a head dim other than 64, a nonzero
    final_logits_bias (pegasus-large's is all zero)."""

    def __init__(self, config=None):
        super().__init__()
        self.config = config if config is not None else PegasusConfig()
        c = self.config
        if c.activation_function != "relu":
            raise NotImplementedError(f"native Pegasus implements activation_function='relu', not "
                                      f"{c.activation_function!r}")
        for what, nh in (("encoder", c.encoder_attention_heads), ("decoder", c.decoder_attention_heads)):
            if c.d_model != 64 * nh:
                raise NotImplementedError(f"native Pegasus needs head dim 64: d_model {c.d_model} with {nh} {what} "
                                          "heads")
        self.model = _PegasusModel(c)
        self.lm_head = nn.Linear(c.d_model, c.vocab_size, bias=False)
        self.lm_head.weight = self.model.shared.weight
        self.register_buffer("final_logits_bias", torch.zeros(1, c.vocab_size))
        for m in self.modules():
            if isinstance(m, nn.Linear):
                if m.weight is not self.model.shared.weight:
                    nn.init.normal_(m.weight, 0.0, c.init_std)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)
        with torch.no_grad():
            nn.init.normal_(self.model.shared.weight, 0.0, c.init_std)
            self.model.shared.weight[c.pad_token_id].zero_()
            for st in (self.model.encoder, self.model.decoder):
                st.embed_positions.weight.copy_(pegasus_sinusoidal_table(c.max_position_embeddings, c.d_model))

    def check_supported(self):
        """After loading a checkpoint: the head's additive bias must be zero (it is not applied)."""
        if bool((self.final_logits_bias != 0).any()):
            raise NotImplementedError("native Pegasus: final_logits_bias is not all zero")

    def check_text_len(self, L, what="text"):
        P = self.config.max_position_embeddings
        if L > P:
            raise ValueError(f"Pegasus: {what} length {L} exceeds max_position_embeddings {P}")

    def engine(self, root=None):
        """The PegasusEngine of this model on the flat buffers of `root` (the module that owns the parameters: this
        one, or a wrapper such as model.lang.pegasus_hugface.PegasusHugface)."""
        from .pegasus import PegasusEngine
        flat = (root if root is not None else self).native_flat()
        return PegasusEngine(self, flat, self.compute_dtype())


def check_max_text_len(model, max_text_len):
    """Drivers: --max_text_len against the position table of every BertModel inside `model`, before any data is built."""
    for m in model.modules():
        if isinstance(m, BertModel) and max_text_len > m.config.max_position_embeddings:
            raise SystemExit(f"error: --max_text_len {max_text_len} exceeds the language model's "
                             f"{m.config.max_position_embeddings} positions (BertConfig.max_position_embeddings)")
        if isinstance(m, OpenAIGPTModel) and max_text_len > m.config.n_positions:
            raise SystemExit(f"error: --max_text_len {max_text_len} exceeds the language model's "
                             f"{m.config.n_positions} positions (OpenAIGPTConfig.n_positions)")
