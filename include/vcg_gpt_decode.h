/*
 * vcg_gpt_decode_desc: everything one KV-cached decode step of the GPT stage reads (vcg_gpt_decode_step,
 * csrc/gpt_decode.hip). Included by vcg_hip.h and by the library; Python mirrors it field for field
 * (vcg_hip/gpt_decode.py) and checks its size against vcg_gpt_decode_desc_bytes().
 *
 * All pointers are device pointers; the struct itself lives on the host and is read while the step is enqueued.
 */
#ifndef VCG_GPT_DECODE_H
#define VCG_GPT_DECODE_H

#define VCG_GPT_MAX_LAYERS 48

typedef struct vcg_gpt_decode_layer {
  const void* w[4];     /* QKV, attention output, FFN1, FFN2 in the storage dtype: [out][in] (K-contiguous), or the
                           stored HF Conv1D weight [in][out] with w_stored_in_out */
  const float* b[4];    /* their fp32 biases */
  const float* ln_g[2]; /* ln_1, ln_2 */
  const float* ln_b[2];
  void* kcache;         /* [B][nh][Tcap][64] in the storage dtype */
  void* vcache;
} vcg_gpt_decode_layer;

typedef struct vcg_gpt_decode_desc {
  int dtype;            /* VCG_F32 / VCG_BF16: activations, caches, weights */
  int B, H, nh, n_layer, n_inner, V, Tcap;
  int n_pos;            /* rows of the position table */
  int max_len0;         /* max over b of len0[b] (host copy: the refusals are made before any launch) */
  int steps;            /* rows of u, columns of forced / chosen */
  int w_stored_in_out;  /* 1: w[] are the Conv1D weights as stored (the fp32 parity mode, read as vcg_gemm's transB) */
  int top_k, greedy;
  int use_skinny;       /* 1: the Linear layers and the head run on vcg_gemm_skinny (bf16, B <= 16, K-contiguous w) */
  float temperature, ln_eps;
  long long ldz;        /* V rounded up to 8 */
  const float* tok;     /* [V][H] fp32 */
  const float* pos;     /* [n_pos][H] fp32 */
  const void* head_w;   /* bf16: [V][H]; fp32: [ldz][H], pad rows zero */
  long long* seq;       /* [B][Tcap] int64 tokens: the prompt, then what each step writes */
  const int* len0;      /* [B] prompt lengths */
  /* generated token g = 0..steps-1 goes to column len0 + g; g = 0 is drawn from the prompt's own forward, step t
     draws g = t + 1 */
  const float* u;       /* [steps][B] uniforms in [0, 1), row g (NULL with greedy) */
  const long long* forced; /* optional [B][steps]: written to seq instead of the sampler's choice */
  long long* chosen;    /* optional [B][steps]: the sampler's choice */
  float* prob;          /* optional [steps][B]: its probability */
  /* workspaces, allocated once by the caller */
  void* h;              /* [B][H] the residual stream (step input) */
  void* qkv;            /* [B][3H] */
  void* ctx;            /* [B][H] */
  void* ao;             /* [B][H] */
  void* h1;             /* [B][H] */
  void* ff;             /* [B][n_inner] */
  void* fo;             /* [B][H] */
  void* h2;             /* [B][H] */
  float* logits;        /* [B][ldz] fp32 */
  float* ln_stat;       /* [2][B] */
  vcg_gpt_decode_layer layers[VCG_GPT_MAX_LAYERS];
} vcg_gpt_decode_desc;

#endif
