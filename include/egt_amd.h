/*
 * egt_amd.h — C-ABI of the MI355X-native EGT edge-augmented attention path.
 *
 * The reference (shamim-hussain/egt) has NO FFI for this path: its seam is a
 * pure-Python plugin registry (lib/base/track_layers/base.py:43-60) through
 * which lib/models/graph_xformer_model_base.py:117-131 instantiates
 * lib/models/egt_layers.py:4 `EGT`.  This header is the boundary a native
 * replacement of that layer binds (see INTEGRATION.md for the ctypes stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer valid on `stream` (a hipStream_t passed
 *     as void*; NULL = the null stream); the caller allocates everything; the
 *     library never allocates, frees or keeps user memory and never syncs.
 *   - tensors are dense row-major fp32 in the reference's layouts:
 *       qkv   [B,N,3*d*H]   channel c = s*d*H + k*H + h   (egt_layers.py:73-76)
 *       E,G,M,h_hat,a_tild [B,N,N,H]  (h innermost)       (egt_layers.py:63-65)
 *       v_att [B,N,d*H]     channel k*H + h               (egt_layers.py:139-141)
 *       key_mask [B,N] uint8, 1 = real node               (egt_layers.py:91-94)
 *       h [B,N,Dh], e [B,N,N,De]        (graph_xformer_model_base.py:192-223)
 *     Dense kernels are Keras-layout [in,out].
 *   - return value: EGT_OK or a negative EGT_E_* code; egt_last_error_string()
 *     describes the last failure on the calling thread.  No C++ exception
 *     crosses this boundary.
 *   - kernels are stateless and re-entrant; safe from several host threads on
 *     different streams.
 *
 * Buffer contract (held by tests/test_memcontract_gpu.py, entry point by entry point)
 *   - a buffer has EXACTLY the byte count its tensor shape or its *_bytes() query states: no call reads or writes a byte
 *     before its first or past its last, whatever the launch geometry (one exception, reads only: next item).
 *   - alignment.  Tensors, masks, targets, seeds, saved buffers and workspaces: as torch allocates tensors (512 bytes;
 *     anything less is outside this contract).  Parameter tensors (every member of a *_params struct, and the parameter
 *     pointers of egt_edge_* and egt_edge_embed*) and gradient sinks (the d_* / grads counterparts of those): the alignment of
 *     their element, 4 bytes -- they may be views of one flat buffer at any float offset, and the results are bit-identical
 *     to the call on 512-byte-aligned copies.  For an unaligned parameter a call may READ, and never write, the bytes
 *     between the enclosing 16-byte boundary and the parameter's first byte (the node kernels load from the pointer rounded
 *     down and commit from the true one); a gradient sink is written from its first byte to its last and nowhere else.
 *   - every output, and every gradient sink behind a non-NULL pointer, is written in full by the call -- padded rows, masked
 *     rows and unused parameter rows included -- unless the entry point's comment names the exception (the "reserved" slot of
 *     rowstats after a forward; the "gradient outputs are scratch" pointers of EGT_BF_NO_EDGE_LN).
 *   - a workspace is scratch: its contents on entry do not matter and the results do not depend on them.  What travels
 *     from a forward to its backward: `saved` of block / stack, rowstats, `hops`, and a workspace handed over under
 *     EGT_ATTN_WS_SHARED (MFMA inner op, pair operator) or EGT_FFN_WS_PREPARED.  `const` inputs are never written.
 *   - the aliasings allowed, all of them: d_e may alias d_e_out (egt_block_bwd, egt_stack_bwd, egt_pair_bwd; in place under
 *     EGT_BF_STATIC_EDGE), dx may alias dy (egt_ffn_bwd), d_e_base may alias d_e (egt_edge_proj_bwd_acc).  The result is
 *     bit-identical to the call on separate buffers.  Nothing else may overlap (d_h must NOT alias d_h_out).
 */
#ifndef EGT_AMD_H_
#define EGT_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGT_ABI_VERSION 4

/* error codes */
#define EGT_OK 0
#define EGT_E_NULL (-1)      /* required pointer is NULL                        */
#define EGT_E_SHAPE (-2)     /* bad / unsupported shape (the reference's assert,
                                egt_layers.py:70, maps here)                    */
#define EGT_E_DTYPE (-3)     /* unsupported dtype                               */
#define EGT_E_FLAGS (-4)     /* inconsistent flags (egt_layers.py:20-24)        */
#define EGT_E_HIP (-5)       /* a HIP runtime call failed                       */
#define EGT_E_WORKSPACE (-6) /* workspace too small                             */
#define EGT_E_RCCL (-7)      /* RCCL missing or a collective call failed        */

/* dtype */
#define EGT_F32 0
#define EGT_BF16 1 /* the EDGE tensors are bfloat16 in HBM; node tensors, parameters, gradients of
                      parameters, workspaces and all arithmetic stay fp32.  Taken by the fused
                      block/stack (e, e', d e', d e and the stack's saved e_l), the channel FFN
                      (x, y, dy, dx) and the edge embedding (e_out, d_e; the hop planes stay
                      fp32); every other op is fp32 only */

/* egt_attn_desc.flags — the operator attributes of EGT.__init__
 * (egt_layers.py:5-16) */
#define EGT_F_EDGE_INPUT 0x001u    /* edge_input: E is added to the logits      */
#define EGT_F_GATE_INPUT 0x002u    /* gate_input: call_gated, else call_ungated */
#define EGT_F_ATTN_MASK 0x004u     /* attn_mask: M present                      */
#define EGT_F_SCALE_DEGREE 0x008u  /* scale_degree                              */
#define EGT_F_SCALER_LINEAR 0x010u /* scaler_type == 'linear' (else 'log')      */
#define EGT_F_TRAINING 0x020u      /* training: random mask / dropout active    */
#define EGT_F_CLIP 0x040u          /* clip_logits_value is not None             */

typedef struct egt_attn_desc {
  int32_t B, N, H, d;        /* graphs, padded nodes, heads, per-head dot dim   */
  int32_t dtype;             /* EGT_F32                                         */
  uint32_t flags;            /* EGT_F_*                                         */
  float clip_lo, clip_hi;    /* clip_logits_value                               */
  float random_mask_prob;    /* egt_layers.py:103                               */
  float attn_dropout;        /* egt_layers.py:116                               */
  int32_t num_virtual_nodes; /* egt_layers.py:131                               */
  int32_t reserved;          /* 0, or EGT_ATTN_WS_* bits (MFMA path only)       */
  uint64_t seed;             /* counter-hash seed for the in-kernel mask RNG    */
} egt_attn_desc;
/* egt_attn_desc.reserved, MFMA path: the caller gives egt_attn_mfma_fwd a workspace of
 * egt_attn_mfma_workspace_bytes() and hands THE SAME, untouched workspace to egt_attn_mfma_bwd:
 * the forward then packs the q/k/v operand copies of both directions once and the backward packs
 * only dV_att.  Without the bit each call packs what it needs into its own workspace. */
#define EGT_ATTN_WS_SHARED 0x1
/* egt_attn_desc.reserved, MFMA path, opt-in arithmetic mode: QK^T, A.V and their backward products take
 * bfloat16 operands on v_mfma_f32_16x16x{32,16}_bf16 and accumulate in fp32.  Every tensor at the interface
 * keeps its fp32 type and layout; egt_attn_mfma_fwd / _bwd cover exactly the descriptors
 * egt_attn_mfma_supported answers 1 for.  Exactly these values are rounded to bfloat16 (round to nearest
 * even), each once: s.Q (s = d^-1/2, rounded after the fp32 scaling), K, V, dV_att, the gated probabilities P
 * that enter A.V and P^T.dV_att, and the logit gradient dS (after the clip mask, d_h_ext already added;
 * the one rounded value feeds dK = dS^T.(sQ) and, through the workspace, dQ = dS.K.s).  Everything else is
 * fp32 on unrounded values: the accumulators, scale / clip / +E / masks, exp, the softmax max and sum
 * (rowstats slots 0 / 1), sigmoid, delta = sum dO.O, dA = dO.V^T, H_hat, dE, dG.  So H_hat and dG are as
 * accurate as in the default mode relative to a reference fed the rounded operands; V_att, dQKV and (through
 * delta) dE carry the bf16 noise (normalised L2 error ~1.7e-3).  Forward and backward of one step must agree
 * on the bit.  The rowstats layout is unchanged, so egt_attn_bwd pairs with this forward as well.  The
 * workspace queries answer for the bit: the dA tiles are bf16 there, so the size for both directions is smaller than
 * without it (84 MB against 118 MB at B = 8, N = 512, d = 64); with EGT_ATTN_WS_SHARED the forward's size is the total.  Any other bit of `reserved` is EGT_E_FLAGS. */
#define EGT_ATTN_MM_BF16 0x2

const char* egt_last_error_string(void);
int egt_abi_version(void);

/* ---- inner op: EGT.call_gated / call_ungated ---------------------------------
 * Replaces lib/models/egt_layers.py:57-143 (gated) and :145-213 (ungated):
 *   (V_att, H_hat, A_tild) = EGT([QKV, E?, G?, M?], mask)
 * key_mask may be NULL (mask=None).  rand_mask / drop_keep ([B,N,N,H] uint8;
 * rand_mask 1 = key masked, drop_keep 1 = kept) are optional INJECTED samples of
 * the two stochastic ops (egt_layers.py:103-108,116-117) used by parity tests;
 * when NULL and (flags & TRAINING) the kernel draws them from the counter hash
 * on (seed,b,l,m,h) (egt_mask_sample exposes the same stream).
 * a_tild may be NULL (only lib/models/analysis.py reads it).
 * rowstats [B,N,H,4] fp32 (softmax max, softmax sum, gate degree, reserved) is
 * written for egt_attn_bwd. */
int egt_attn_fwd(const egt_attn_desc* desc, const void* qkv, const void* E,
                 const void* G, const uint8_t* key_mask, const void* attn_mask,
                 const uint8_t* rand_mask, const uint8_t* drop_keep, void* v_att,
                 void* h_hat, void* a_tild, void* rowstats, void* stream);

/* Backward of the above — what TF autodiff derives for egt_layers.py:57-143
 * (triggered by model.fit, lib/training/training_base.py:294).
 * d_h_ext (grad w.r.t. output 2, H_hat) may be NULL.  d_E / d_G may be NULL
 * when the corresponding input is absent.  v_att and rowstats are the forward's
 * outputs.  workspace: egt_attn_bwd_workspace_bytes() bytes. */
size_t egt_attn_bwd_workspace_bytes(const egt_attn_desc* desc);
int egt_attn_bwd(const egt_attn_desc* desc, const void* qkv, const void* E,
                 const void* G, const uint8_t* key_mask, const void* attn_mask,
                 const uint8_t* rand_mask, const uint8_t* drop_keep,
                 const void* v_att, const void* rowstats, const void* d_v_att,
                 const void* d_h_ext, void* d_qkv, void* d_E, void* d_G,
                 void* workspace, void* stream);

/* MFMA-tiled (flash-style) variant of the inner op for the large-head geometry
 * (H = 8, d in {16,32,64}; BASELINE config 5): QK^T and A.V on
 * v_mfma_f32_16x16x4_f32, probabilities never leave registers.  Same outputs and the
 * same rowstats as egt_attn_fwd (so egt_attn_bwd pairs with either); not covered:
 * attention dropout, degree scalers, the A_tild output.  egt_attn_mfma_supported
 * returns 1 when `desc` (and the A_tild request) is covered. */
int egt_attn_mfma_supported(const egt_attn_desc* desc, int need_a_tild);
/* Workspace of the MFMA path: head-major operand copies of Q/K/V/dV_att (+ per-row constants and
 * the dA tiles in the backward).  *_fwd_* is what egt_attn_mfma_fwd needs on its own; the other
 * covers both directions (and is what EGT_ATTN_WS_SHARED asks for). */
size_t egt_attn_mfma_fwd_workspace_bytes(const egt_attn_desc* desc);
size_t egt_attn_mfma_workspace_bytes(const egt_attn_desc* desc);
int egt_attn_mfma_fwd(const egt_attn_desc* desc, const void* qkv, const void* E,
                      const void* G, const uint8_t* key_mask, const void* attn_mask,
                      const uint8_t* rand_mask, void* v_att, void* h_hat, void* rowstats,
                      void* workspace, void* stream);
/* Backward on MFMA tiles (launches: pack, dK/dV/dE/dG per 32-key block, dQ per query
 * block).  rowstats is read and its 4th slot written; workspace: egt_attn_mfma_workspace_bytes. */
int egt_attn_mfma_bwd(const egt_attn_desc* desc, const void* qkv, const void* E,
                      const void* G, const uint8_t* key_mask, const void* attn_mask,
                      const uint8_t* rand_mask, const void* v_att, void* rowstats,
                      const void* d_v_att, const void* d_h_ext, void* d_qkv, void* d_E,
                      void* d_G, void* workspace, void* stream);

/* The in-kernel sample streams, materialised ([B,N,N,H] uint8), for bit-exact
 * checks against oracle/rng_ref.py.  which: 0 = random mask (1 = masked),
 * 1 = dropout keep (1 = kept). */
int egt_mask_sample(int which, uint64_t seed, float prob, int32_t B, int32_t N,
                    int32_t H, uint8_t* out, void* stream);

/* EGT_BF_SEED_DEVICE companion (see egt_block_desc): words[i] += increment (mod 2^64) for i < count, as ONE launch
 * on `stream` — capturable, so a hipGraph that contains it in front of the forward draws a fresh random mask on
 * every replay.  The torch host advances its words by 0xD1B54A32D192ED03 per call (EGT.next_seed's step). */
int egt_seed_advance(uint64_t* words, int32_t count, uint64_t increment, void* stream);

/* ---- edge-channel projections around the inner op ----------------------------
 * rows = B*N*N edge rows of width De; H must be 8. */
#define EGT_EP_LAYERNORM 0x1u /* norm_edge before the projections (residual /
                                 constrained); absent for 'bias'               */
#define EGT_EP_GATES 0x2u     /* attention_gates present (gate_attention)       */
#define EGT_ACT_NONE 0
#define EGT_ACT_LRELU 1 /* 'lreluN': alpha = N/10 (graph_xformer_model_base.py:150-156) */
#define EGT_ACT_RELU 2
#define EGT_ACT_ELU 3

typedef struct egt_edge_desc {
  int64_t rows;     /* B*N*N                                                   */
  int32_t De, H;    /* edge_width, num_heads (8)                               */
  int32_t dtype;    /* EGT_F32                                                 */
  uint32_t flags;   /* EGT_EP_*                                                */
  int32_t act;      /* EGT_ACT_* for dense_edge_b                              */
  float act_alpha;  /* leaky-relu slope                                        */
  float ln_eps;     /* Keras LayerNormalization default 1e-3                   */
  int32_t reserved;
} egt_edge_desc;

/* G = LN(e)·Wg + bg ; E = act(LN(e)·We + be)
 * Replaces graph_xformer_model_base.py:195 (norm_edge), :201-204
 * (attention_gates), :149-162 (edge_channel_contrib / dense_edge_b).
 * Wg/We [De,H], bg/be [H]; G_out may be NULL without EGT_EP_GATES. */
int egt_edge_proj_fwd(const egt_edge_desc* desc, const void* e,
                      const void* ln_gamma, const void* ln_beta, const void* Wg,
                      const void* bg, const void* We, const void* be,
                      void* G_out, void* E_out, void* stream);

/* Backward: d_e is WRITTEN (not accumulated).  E_out = forward output (only
 * read when act != NONE).  Parameter grads are written.  workspace:
 * egt_edge_proj_bwd_workspace_bytes(). */
size_t egt_edge_proj_bwd_workspace_bytes(const egt_edge_desc* desc);
int egt_edge_proj_bwd(const egt_edge_desc* desc, const void* e,
                      const void* ln_gamma, const void* ln_beta, const void* Wg,
                      const void* We, const void* E_out, const void* d_G,
                      const void* d_E, void* d_e, void* d_ln_gamma,
                      void* d_ln_beta, void* d_Wg, void* d_bg, void* d_We,
                      void* d_be, void* workspace, void* stream);
/* Same, with d_e = d_e_base + (projection backward): d_e_base [rows,De] is the gradient e already
 * carries from the residual branch e' = e + ... (graph_xformer_model_base.py:218), so the sum the
 * autodiff of the reference forms with a separate add costs no extra pass.  d_e_base may be NULL
 * (then identical to egt_edge_proj_bwd) and may alias d_e. */
int egt_edge_proj_bwd_acc(const egt_edge_desc* desc, const void* e,
                          const void* ln_gamma, const void* ln_beta, const void* Wg,
                          const void* We, const void* E_out, const void* d_G,
                          const void* d_E, const void* d_e_base, void* d_e,
                          void* d_ln_gamma, void* d_ln_beta, void* d_Wg, void* d_bg,
                          void* d_We, void* d_be, void* workspace, void* stream);

/* e' = e + H_hat·Wr + br   (dense_edge_r + res_edge,
 * graph_xformer_model_base.py:214-218).  Wr [H,De], br [De]. */
int egt_edge_update_fwd(const egt_edge_desc* desc, const void* e,
                        const void* h_hat, const void* Wr, const void* br,
                        void* e_out, void* stream);

/* Backward: d_h_hat = d_e_out·Wrᵀ (written); d_Wr, d_br written.  The residual
 * branch (d_e += d_e_out) is the caller's add. */
size_t egt_edge_update_bwd_workspace_bytes(const egt_edge_desc* desc);
int egt_edge_update_bwd(const egt_edge_desc* desc, const void* d_e_out,
                        const void* h_hat, const void* Wr, void* d_h_hat,
                        void* d_Wr, void* d_br, void* workspace, void* stream);

/* ---- outer op: the fused attention block (the data-parallel hot path) ---------
 *   (h', e') = edge_update_residual(h, e) with mha_block inside, pre-norm
 * Replaces graph_xformer_model_base.py:192-223 + :106-145 for
 * edge_channel_type 'residual' / 'constrained' (add_n_norm=False, no dropout;
 * scale_degree with EGT_BF_SCALE_DEGREE, fp32 edge tensors): norm_edge -> attention_gates / dense_edge_b -> norm_mha ->
 * dense_qkv -> EGT -> dense_mha + res_mha ; dense_edge_r + res_edge.
 * One launch streams e once: LN, the two De->H projections, QK^T, clip, +E,
 * masks, softmax x sigmoid gate, A.V and e' = e + H_hat.Wr + br never leave the
 * CU (E, G, H_hat, A_tild are not materialised).  Everything else (other
 * variants, node / edge dropout, attention dropout without EGT_BF_ATTN_DROPOUT,
 * degree scalers with virtual nodes or bf16 edges, d > 8) composes the kernels above.
 * Parameter pointers carry the reference's Keras layer names. */
#define EGT_BF_GATE 0x1u      /* gate_attention                                  */
#define EGT_BF_ATTN_MASK 0x2u /* 'constrained': attn_mask [B,N,N,H] fp32 present */
#define EGT_BF_TRAINING 0x4u  /* random attention mask active                    */
#define EGT_BF_CLIP 0x8u      /* clip_logits_value is not None                   */
#define EGT_BF_NO_EDGE_LN 0x10u /* 'bias' edge channels (EGT-simple, :173-190): gates / edge bias from
                                  the RAW e.  The caller passes norm_edge gamma = 1, beta = 0 and
                                  dense_edge_r kernel = bias = 0 (then e' = e); their gradient
                                  outputs are scratch */
#define EGT_BF_SEED_DEVICE 0x20u /* hipGraph-safe random mask: the kernels draw from the stream seeded with
                                  desc->seed ^ *desc->seed_device (a uint64 in DEVICE memory, read by the
                                  kernel when it runs, not by the host at launch).  A captured step replays
                                  with a fresh sample by advancing that word on the device; forward and
                                  backward of one step must see the same value */
#define EGT_BF_STATIC_EDGE 0x40u /* 'bias' edge channels as what they are: e is an INPUT only (every layer of an
                                  EGT-simple model reads the same e, :173-190).  Only valid with EGT_BF_NO_EDGE_LN.
                                  Forward: e_out is never written and may be NULL; the norm_edge_* and dense_edge_r_*
                                  parameter pointers are never read and may be NULL.  Backward: d_e_out may be NULL
                                  (= zeros; it is then not read); d_e may alias d_e_out (d_e[i] = d_e_out[i] +
                                  contribution, in place: a lane reads and writes only its own (row, key,
                                  channel pair) element, exactly once per launch, and the requests that run ahead
                                  touch elements no lane has written yet); the norm_edge_* / dense_edge_r_*
                                  gradient pointers are never written and may be NULL.  The in-kernel random mask
                                  only (rand_mask must be NULL).  egt_block_supported() answers 1 with this flag
                                  exactly where the De = 8 pair kernels run: De = 8, d <= 8, H = 8, fp32 or bf16
                                  edges, no EGT_BF_ATTN_MASK; egt_stack_* refuses it (EGT_E_FLAGS) */
#define EGT_BF_SCALE_DEGREE (1u << 7) /* 0x80: scale_degree (egt_layers.py:122-136, no virtual nodes): V_att of (row, head) is
                                  multiplied by s(deg), deg = the row's sum of gates over the keys (0 for a masked or
                                  padded key), s = log1p (default) or the identity (EGT_BF_SCALER_LINEAR).  Needs
                                  EGT_BF_GATE; not with EGT_BF_STATIC_EDGE (both EGT_E_FLAGS).  fp32 edge tensors only
                                  (EGT_BF16: not covered).  Runs on the MFMA-tile pair kernels for every De (De = 8
                                  included); `saved` does not grow: slot 3 of the per-(row, head) statistics carries deg
                                  forward and d deg into the backward pair kernel.  egt_stack_* and the pair operator
                                  refuse it (EGT_E_FLAGS / egt_pair_supported = 0) */
#define EGT_BF_SCALER_LINEAR (1u << 8) /* 0x100: scaler_type 'linear' (s = deg); only valid with EGT_BF_SCALE_DEGREE */
#define EGT_BF_ATTN_DROPOUT (EGT_BF_SCALER_LINEAR << 1) /* 0x200, the next bit: attn_dropout (egt_layers.py:116-117): A_tild of (b, l, m, h) is dropped before A.V,
                                  keep <=> (egt_hash32(i, s0, s1 ^ 0x5BD1E995) >> 8) >= floor(rate * 2^24) with
                                  i = ((b N + l) N + m) H + h as a uint32 and (s0, s1) the low / high word of the
                                  effective seed (desc->seed, ^ *seed_device under EGT_BF_SEED_DEVICE); a kept element is
                                  scaled by 1 / (1 - rate) in fp32 -- the stream of egt_attn_fwd and
                                  egt_mask_sample(which = 1).  The random mask of the call draws from the same seed on
                                  its own stream.  The rate travels in desc->reserved as its fp32 bit pattern and must
                                  lie in (0, 1) (else EGT_E_FLAGS).  Needs EGT_BF_TRAINING (EGT_E_FLAGS without: clear
                                  the flag for evaluation); not with EGT_BF_SCALE_DEGREE or EGT_BF_STATIC_EDGE (both
                                  EGT_E_FLAGS).  fp32 and bf16 edge tensors, gated or not, every De (De = 8 runs on the
                                  MFMA-tile pair kernels); sizes do not change and nothing is saved for the mask: both
                                  directions recompute it.  H_hat, e' and the softmax statistics do not see the mask.
                                  egt_stack_* and the pair operator refuse it (EGT_E_FLAGS / egt_pair_supported = 0) */

typedef struct egt_block_desc {
  int32_t B, N, H, d, De;   /* model_width Dh = d*H                             */
  int32_t dtype;            /* EGT_F32                                          */
  uint32_t flags;           /* EGT_BF_*                                         */
  float clip_lo, clip_hi;
  float random_mask_prob;
  float ln_eps;             /* 1e-3                                             */
  int32_t reserved;         /* EGT_BF_ATTN_DROPOUT: the fp32 bit pattern of the rate; else ignored              */
  uint64_t seed;
  const void* seed_device;  /* EGT_BF_SEED_DEVICE: const uint64_t* on the device, else ignored (NULL) */
} egt_block_desc;

typedef struct egt_block_params {
  const void* norm_edge_gamma;        /* [De]      norm_edge_XX/gamma            */
  const void* norm_edge_beta;         /* [De]                                    */
  const void* attention_gates_kernel; /* [De,H]    attention_gates_XX            */
  const void* attention_gates_bias;   /* [H]                                     */
  const void* dense_edge_b_kernel;    /* [De,H]    dense_edge_b_XX               */
  const void* dense_edge_b_bias;      /* [H]                                     */
  const void* norm_mha_gamma;         /* [Dh]      norm_mha_XX                   */
  const void* norm_mha_beta;          /* [Dh]                                    */
  const void* dense_qkv_kernel;       /* [Dh,3Dh]  dense_qkv_XX                  */
  const void* dense_qkv_bias;         /* [3Dh]                                   */
  const void* dense_mha_kernel;       /* [Dh,Dh]   dense_mha_XX                  */
  const void* dense_mha_bias;         /* [Dh]                                    */
  const void* dense_edge_r_kernel;    /* [H,De]    dense_edge_r_XX               */
  const void* dense_edge_r_bias;      /* [De]                                    */
} egt_block_params;

/* 1 when the fused kernels cover `desc`, else 0 (caller composes instead). */
int egt_block_supported(const egt_block_desc* desc);
/* Name of the backward pair-kernel family the dispatch takes for `desc` when no mask tensor is passed (
 * "k_block_bwd_v5", "k_block_bwd_v4", "k_block_bwd_v4r", "k_narrow_bwd": DESIGN.md section 4); NULL when `desc` is not covered.
 * Static string; for tests and bench lines (the launch profiler reports every family as "k_block_bwd"). */
const char* egt_block_bwd_kernel(const egt_block_desc* desc);
/* The launch forms the dispatch takes for `desc` when no mask tensor is passed, as text:
 * "fwd=<family>/<waves>w[/half] bwd=<family>/<waves>w/tl<rows per workgroup>", e.g. "fwd=k_narrow_fwd/8w/half bwd=k_narrow_bwd/8w/tl8".
 * Thread-local string, valid until the thread's next call; NULL when `desc` is not covered.  For tests and bench lines. */
const char* egt_block_launch_form(const egt_block_desc* desc);
/* 1 when the dispatch gives `desc` (no mask tensor passed) the compile-time forward instance of the headline shape, k_block_fwd_s64
 * (N = 64, De = 64, d = 8, fp32, gate + clip, training with the in-kernel random mask, 16-row groups) -- which a call then runs
 * if it passes a key mask and its geometry takes the node epilogue; else 0 (any other descriptor, EGT_NO_STATIC=1, NULL, not
 * covered).  Results are bit-identical either way.  Read-only; for tests and bench lines that must know which form ran. */
int egt_block_plan_static(const egt_block_desc* desc);
/* bytes of the forward->backward buffer (V_att, softmax row statistics, packed
 * Q/K/V, the LN-folded edge weights and the MFMA-fragment-major copies of Wqkv / Wo the forward prepares: the backward
 * must be given the `saved` buffer of ITS forward call, made with the same parameter values) and of the scratch
 * workspace (max of forward and backward needs). */
size_t egt_block_saved_bytes(const egt_block_desc* desc);
size_t egt_block_workspace_bytes(const egt_block_desc* desc);

/* rand_mask: optional injected sample ([B,N,N,H] uint8, 1 = masked) as in
 * egt_attn_fwd; NULL => in-kernel counter hash when TRAINING and prob > 0. */
int egt_block_fwd(const egt_block_desc* desc, const egt_block_params* params,
                  const void* h, const void* e, const uint8_t* key_mask,
                  const void* attn_mask, const uint8_t* rand_mask, void* h_out,
                  void* e_out, void* saved, void* workspace, void* stream);

/* Backward.  h, e are the block's INPUTS (nothing else of size [B,N,N,*] is
 * kept: LN, projections, logits and softmax are recomputed from e).  d_e may
 * alias d_e_out; d_h must NOT alias d_h_out (the deferred dense_mha weight
 * gradient reads d_h_out after d_h has been written).  Every pointer of `grads`
 * (same layout as the params, but writable) is written. */
int egt_block_bwd(const egt_block_desc* desc, const egt_block_params* params,
                  const void* h, const void* e, const uint8_t* key_mask,
                  const void* attn_mask, const uint8_t* rand_mask,
                  const void* saved, const void* d_h_out, const void* d_e_out,
                  void* d_h, void* d_e, const egt_block_params* grads,
                  void* workspace, void* stream);

/* ---- the model_height loop over attention blocks -------------------------------
 * Replaces the `for ii in range(model_height): h, e = edge_update(tag, h, e)` half
 * of graph_xformer_model_base.py:336-339 when the blocks are applied back to back
 * (the measurement configuration; the reference interleaves ffn_block, for which
 * egt_block_fwd/bwd is the per-layer drop-in).  params / grads are arrays of
 * `layers` structs.  saved keeps the layer activations h_l, e_l (l = 1..layers-1)
 * and each layer's egt_block_saved buffer.  Forward: one launch per layer where the
 * node-side epilogue covers the geometry (Dh = 64), else three.  Backward: d_e carries
 * the edge gradient down the stack in place, every layer's dh and dQKV rows are kept
 * in the workspace, and the GEMM-shaped weight gradients plus all partial sums of ALL
 * layers are finished by three launches at the end (d_h must not alias d_h_out; at
 * most 64 layers per call).  Layer l draws its random attention mask from
 * the counter hash seeded with desc->seed ^ 0x9E3779B97F4A7C15*(l+1). */
size_t egt_stack_saved_bytes(const egt_block_desc* desc, int32_t layers);
size_t egt_stack_workspace_bytes(const egt_block_desc* desc, int32_t layers);
/* The launch plane of egt_stack_bwd's three closing launches for `desc` and `layers` (no mask tensor), as text:
 * "wgrad=<rows per workgroup>r/<row chunks>c partials=<edge-parameter partials> reduce=<reduction launches>
 *  epg=<edge-parameter-gradient launches> prep=<stack16|stack40|edge_prep>", e.g.
 * "wgrad=160r/27c partials=384 reduce=2 epg=1 prep=stack16" (prep: how the forward prepares the edge weights).
 * A read-only query computed by the functions the launches call; it needs no device.  Thread-local string, valid until
 * the thread's next call; NULL when the call is not covered (1 <= layers <= 64).  For tests and bench lines. */
const char* egt_stack_tail_form(const egt_block_desc* desc, int32_t layers);
int egt_stack_fwd(const egt_block_desc* desc, int32_t layers,
                  const egt_block_params* params, const void* h, const void* e,
                  const uint8_t* key_mask, const void* attn_mask, void* h_out,
                  void* e_out, void* saved, void* workspace, void* stream);
int egt_stack_bwd(const egt_block_desc* desc, int32_t layers,
                  const egt_block_params* params, const void* h, const void* e,
                  const uint8_t* key_mask, const void* attn_mask, const void* saved,
                  const void* d_h_out, const void* d_e_out, void* d_h, void* d_e,
                  const egt_block_params* grads, void* workspace, void* stream);

/* ---- the fused pair operator at large heads (BASELINE config 5: N = 512, d = 64, De = 32) ------------------
 *   (V_att, e') = norm_edge -> attention_gates / dense_edge_b -> EGT([QKV,E,G],mask) -> dense_edge_r + res_edge
 * Replaces graph_xformer_model_base.py:195-218 (edge_update_residual around mha_block's EGT call, :117-131) with
 * lib/models/egt_layers.py:57-143 inside, for gated 'residual' edge channels: ONE pair kernel per direction streams
 * e (and de' in the backward) once; E, G, H_hat, dE, dG, dH_ext exist only in LDS.  At this head width the
 * node-side Dense layers of mha_block (norm_mha, dense_qkv :109-113, dense_mha :136) are [B N, 512] GEMMs and stay
 * with the caller (library GEMMs): the operator takes QKV [B,N,3 d H] (channel s*dH + k*H + h, egt_layers.py:73-76)
 * and returns V_att [B,N,d H].  egt_block_desc / egt_block_params are reused (node-side pointers are ignored);
 * desc->reserved & EGT_ATTN_WS_SHARED: the caller hands the forward's untouched workspace to the backward, called
 * with the same parameter values (the q / k / v operand copies and the LN-folded weight table are then made once).  In-kernel random mask as in egt_block_fwd. */
int egt_pair_supported(const egt_block_desc* desc);
size_t egt_pair_workspace_bytes(const egt_block_desc* desc);
int egt_pair_fwd(const egt_block_desc* desc, const egt_block_params* params, const void* qkv,
                 const void* e, const uint8_t* key_mask, void* v_att, void* e_out, void* rowstats,
                 void* workspace, void* stream);
/* rowstats [B,N,H,4] is the forward's output (read; slot 3 written).  d_e may alias d_e_out.  Every edge-side
 * pointer of `grads` is written (norm_edge_*, attention_gates_*, dense_edge_b_*, dense_edge_r_*). */
int egt_pair_bwd(const egt_block_desc* desc, const egt_block_params* params, const void* qkv,
                 const void* e, const uint8_t* key_mask, const void* v_att, void* rowstats,
                 const void* d_v_att, const void* d_e_out, void* d_qkv, void* d_e,
                 const egt_block_params* grads, void* workspace, void* stream);

/* ---- the whole block at large heads: the node side of mha_block on the library's own fp32 MFMA GEMMs around the pair operator ----
 *   (h', e') = edge_update_residual(h, e) with mha_block inside (graph_xformer_model_base.py:192-223 + :106-145), covered
 * exactly where egt_pair_supported() answers 1 (d = 64, H = 8, De = 32, gated 'residual' edge channels, fp32; every flag the pair
 * operator refuses is refused here the same way, EGT_BF_SEED_DEVICE included).  egt_block_fwd / egt_block_bwd's signature without
 * attn_mask / rand_mask; all fourteen egt_block_params pointers are read and all fourteen `grads` pointers are written.
 * Forward: per-row LayerNorm statistics, QKV = LN(h).Wqkv + bqkv (rows normalised while the operand is staged: no [B N, 512] LN(h)
 * tensor exists in memory, in either direction), egt_pair_fwd, h' = V_att.Wo + bo + h.  Backward: dV_att = dh'.Wo^T, egt_pair_bwd,
 * d(LN out) = dQKV.Wqkv^T, dh = dh' + LN_bwd, and the node-side parameter gradients as per-row-chunk partials summed in chunk
 * order (bit-reproducible: no floating-point atomics).  Products are exact fp32 (v_mfma_f32_32x32x2_f32).
 * `saved` (egt_pair_block_saved_bytes) carries QKV, V_att, the attention row statistics, the LayerNorm row statistics [B N, 2] and
 * the pair operator's shared workspace from the forward to the backward, which completes parts of it (it is not const there);
 * `workspace` (egt_pair_block_workspace_bytes) is scratch.  desc->reserved must be 0.  d_e may alias d_e_out; d_h must NOT alias
 * d_h_out.  Same parameter values in both directions; no allocation, no synchronisation, everything on `stream` (capturable).
 * egt_pair_block_launch_form: the launch plan, a pure host function of B N, as text:
 * "tile=<rows per row tile>r/<row tiles>t[/ragged] wgrad=<rows per chunk>r/<row chunks>c[/ragged] ln=<rows>r/<partials>p
 *  reduce=<reduction launches>", e.g. "tile=128r/9t/ragged wgrad=256r/5c/ragged ln=64r/17p reduce=1".  Thread-local string, valid
 * until the thread's next call; needs no device; NULL when `desc` is not covered. */
int egt_pair_block_supported(const egt_block_desc* desc);
const char* egt_pair_block_launch_form(const egt_block_desc* desc);
size_t egt_pair_block_saved_bytes(const egt_block_desc* desc);
size_t egt_pair_block_workspace_bytes(const egt_block_desc* desc);
int egt_pair_block_fwd(const egt_block_desc* desc, const egt_block_params* params, const void* h,
                       const void* e, const uint8_t* key_mask, void* h_out, void* e_out, void* saved,
                       void* workspace, void* stream);
int egt_pair_block_bwd(const egt_block_desc* desc, const egt_block_params* params, const void* h,
                       const void* e, const uint8_t* key_mask, const void* saved, const void* d_h_out,
                       const void* d_e_out, void* d_h, void* d_e, const egt_block_params* grads,
                       void* workspace, void* stream);

/* ---- channel FFN (the step after the attention block in every layer) ----
 * Replaces ffnlr1 / ffnact / ffnlr2 of lib/models/graph_xformer_model_base.py:230-258 as
 * ffn_block applies them (:309-324; pre-norm, no cross-talk, ffn_multiplier = 2):
 *   y = x + Dense_2( act( Dense_1( LayerNorm(x) ) ) )
 * on `rows` rows of `width` channels: the edge channels [B*N*N, De] or the node channels
 * [B*N, Dh].  Keras layouts: kernels are [in,out]; LayerNormalization epsilon = ln_eps.
 * Fused MFMA kernels for width in {16,32,48,64}, fp32, activation EGT_ACT_ELU (config default) or
 * EGT_ACT_RELU; egt_ffn_supported says whether a desc is covered. */
/* how the matrix products are evaluated (tensors stay fp32 in HBM, accumulation is always fp32):
 *   EGT_MM_F32     exact fp32 products (v_mfma_f32_16x16x4_f32)
 *   EGT_MM_BF16X3  every operand split into two bfloat16 terms, a.b = a_hi.b_hi + a_lo.b_hi + a_hi.b_lo on the
 *                  bf16 matrix pipe: per-product error <= 2^-16 (fp32: 2^-24); stays inside the fp32 parity
 *                  tolerances of the test-suite at 3/16 of the fp32 MFMA cost
 *   EGT_MM_BF16    plain bfloat16 products (hi terms only): tolerance rtol 2e-2 (SURVEY 8(c) bf16 figure) */
#define EGT_MM_F32 0
#define EGT_MM_BF16X3 1
#define EGT_MM_BF16 2

typedef struct egt_ffn_desc {
  int64_t rows;
  int32_t width;
  int32_t dtype;      /* EGT_F32, or EGT_BF16: x, y, dy, dx in bfloat16 (parameters and their gradients fp32) */
  int32_t activation; /* EGT_ACT_* (config.activation) */
  float ln_eps;       /* 1e-3 */
  int32_t matmul;     /* EGT_MM_* */
  int32_t flags;      /* EGT_FFN_* (0 for plain calls) */
} egt_ffn_desc;
/* egt_ffn_bwd only: `workspace` is the buffer an egt_ffn_fwd call with the same rows / width / activation / matmul and
 * the same parameter VALUES has used on this stream or an earlier-ordered one; the prepared operands in it
 * (LayerNorm-folded weight slabs) are reused and the backward skips its preparation launch. */
#define EGT_FFN_WS_PREPARED 1

typedef struct egt_ffn_params {
  const void* norm_gamma;  /* [W]     norm_fnn_{node,edge}_XX */
  const void* norm_beta;   /* [W]                              */
  const void* lr1_kernel;  /* [W,2W]  fnn_lr1_XX               */
  const void* lr1_bias;    /* [2W]                             */
  const void* lr2_kernel;  /* [2W,W]  fnn_lr2_XX               */
  const void* lr2_bias;    /* [W]                              */
} egt_ffn_params;

int egt_ffn_supported(const egt_ffn_desc* desc);
size_t egt_ffn_workspace_bytes(const egt_ffn_desc* desc);
int egt_ffn_fwd(const egt_ffn_desc* desc, const egt_ffn_params* params, const void* x, void* y,
                void* workspace, void* stream);
/* x is the layer INPUT (the hidden activations are recomputed); dx may alias dy; every pointer
 * of `grads` (same layout as the params, writable) is written. */
int egt_ffn_bwd(const egt_ffn_desc* desc, const egt_ffn_params* params, const void* x,
                const void* dy, void* dx, const egt_ffn_params* grads, void* workspace,
                void* stream);

/* ---- edge FFN with node<->edge cross-talk (node2edge_xtalk / edge2node_xtalk) ----
 * The edge side of ffn_block with cross-talk (lib/models/graph_xformer_model_base.py:227-324), ffn_multiplier = 2:
 *   pre = Dense_1(LayerNorm(e))                      [B,N,N,H], H = 2 De, split along channels into
 *         [ er (s_e) | ec (s_e) | tail (H - 2 s_e) ]
 *   hn[b,n,c] = divide_no_nan( sum_i m[b,i] er[b,i,n,c] + sum_j m[b,j] ec[b,n,j,c], sum_k m[b,k] )   [B,N,s_e]
 *   e_out = e + Dense_2( act( [ tail | hr[b,i,:] + hc[b,j,:] ] ) )
 * hr / hc [B,N,s_n] are the two leading channel groups of the node side's Dense_1 output, hn joins the node side's
 * Dense_2 input; the node side (three [B,N,.] operations) stays with the caller.  lr2_kernel is [H - 2 s_e + s_n, De];
 * the other parameters have the shapes of egt_ffn_params.  mask: [B,N] fp32, 1 = node, 0 = padding; padded pairs are
 * not masked in e_out, only the summed index is.  Sums are taken in a fixed order, without atomics.
 * Covered: fp32, De in {16,32,64}, Dh in {48,64}, any N, s_e and s_n multiples of 4 with 2 s_e <= 2 De, 2 s_n <= 2 Dh,
 * not both 0 (that is egt_ffn_fwd), EGT_ACT_ELU / EGT_ACT_RELU, exact fp32 products.  egt_xtalk_supported answers; the
 * entry points refuse anything else with a code and a message before any launch.
 * With s_n = 0, hr / hc / d_hr / d_hc are not touched and may be NULL; with s_e = 0, hn / d_hn likewise.
 * One workspace size serves both directions; nothing in it is carried from the forward to the backward.
 * No aliasing: in particular d_e must not alias d_e_out (at De = 64 with s_n > 32 the backward reads d_e_out a second time). */
typedef struct egt_xtalk_desc {
  int32_t B, N;
  int32_t De;         /* edge width */
  int32_t Dh;         /* node width (bounds s_n) */
  int32_t s_e;        /* edge -> node channels: round(edge2node_xtalk * De) */
  int32_t s_n;        /* node -> edge channels: round(node2edge_xtalk * Dh) */
  int32_t dtype;      /* EGT_F32 */
  int32_t activation; /* EGT_ACT_ELU or EGT_ACT_RELU */
  float ln_eps;       /* 1e-3 */
  int32_t flags;      /* 0 */
  int32_t reserved;   /* 0 */
} egt_xtalk_desc;

int egt_xtalk_supported(const egt_xtalk_desc* desc);
size_t egt_xtalk_workspace_bytes(const egt_xtalk_desc* desc);
/* The launch plan, a pure host function of the descriptor, as text:
 *   "fwd=k_xtalk_fwd<W,SNT>/rb8/g<grid> bwd=k_xtalk_bwd<W,SNT>/rb<rows per wave>/g<grid>[/walk2]"
 * W = De, SNT = ceil(s_n / 16); /walk2 marks the W = 64, SNT >= 3 instances whose backward walks its pairs a second time.
 * Thread-local string, needs no device; NULL for a descriptor egt_xtalk_supported declines. */
const char* egt_xtalk_launch_form(const egt_xtalk_desc* desc);
int egt_xtalk_fwd(const egt_xtalk_desc* desc, const egt_ffn_params* params, const void* e, const void* mask,
                  const void* hr, const void* hc, void* e_out, void* hn, void* workspace, void* stream);
/* e is the layer INPUT (the hidden activations are recomputed); every pointer of `grads` is written, and so is every
 * element of d_e, d_hr and d_hc. */
int egt_xtalk_bwd(const egt_xtalk_desc* desc, const egt_ffn_params* params, const void* e, const void* mask,
                  const void* hr, const void* hc, const void* d_e_out, const void* d_hn, void* d_e, void* d_hr,
                  void* d_hc, const egt_ffn_params* grads, void* workspace, void* stream);

/* ---- mask producers (integer / boolean work: bit-exact) ---------
 * The masks the path consumes are produced by the model around it; these entry points replace
 *   Neg1MaskedEmbedding.compute_mask   lib/base/xformer_layers/masking.py:35-43   (x + 1) != 0
 *   keras.layers.Masking(mask_value)   lib/models/cifar10/dc.py:69               any(x != v, -1)
 *   VirtualNodeEmbedding.compute_mask  lib/base/graph_layers/virtual_nodes.py:47-50
 *   AdjMatModel.get_edge_mask          lib/models/graph_model_base.py:131-142     tile(adj, H)
 *   VNModel.get_edge_mask              lib/models/graph_model_base.py:248-268     ones for VN rows/cols
 * features [B,N] int32 (padding value -1)  ->  mask [B, num_virtual_nodes + N] uint8 (1 = real node) */
int egt_node_mask_from_features(const int32_t* features, int32_t B, int32_t N, int32_t num_virtual_nodes,
                                uint8_t* mask, void* stream);
/* features [B,N,width] fp32 -> mask [B, num_virtual_nodes + N] uint8: some feature != mask_value */
int egt_node_mask_from_float_features(const float* features, int32_t B, int32_t N, int32_t width,
                                      float mask_value, int32_t num_virtual_nodes, uint8_t* mask,
                                      void* stream);
/* adj [B,N,N] fp32 -> M [B, nv+N, nv+N, H] fp32 (nv = num_virtual_nodes): the attention mask of
 * edge_channel_type 'constrained' as the inner op / fused block take it */
int egt_constrained_edge_mask(const float* adj, int32_t B, int32_t N, int32_t H, int32_t num_virtual_nodes,
                              float* M, void* stream);

/* ---- edge-channel input embedding (the model code that PRODUCES e) -----------
 *   e0 = Neg1MaskedEmbedding(num_edge_features + 1, De)(feature_matrix)        lib/models/zinc/dc.py:70-73
 *      + Dense(upto_hop -> De)(stack_hops(graph_matrix))                        lib/models/graph_model_base.py:97-127
 * feature_matrix [B,N,N] int32 (-1 = no edge / padding), graph_matrix [B,N,N] fp32, fm_table [V,De]
 * (V = num_edge_features + 1), adj_kernel [upto_hop, De] (Keras layout), adj_bias [De].  `hops`
 * ([upto_hop + num_float_features,B,N,N] fp32 -- plane-major --, egt_edge_embed_hops_bytes) receives the hop matrices; the backward
 * reads them again.  Gradients: d_fm_table, d_adj_kernel, d_adj_bias (no gradient flows to the inputs). */
typedef struct egt_embed_desc {
  int32_t B, N, De;
  int32_t upto_hop;           /* 1..16 */
  int32_t clip_hops;          /* clip every hop product to [0,1] (graph_model_base.py:114-115) */
  int32_t num_edge_features;  /* embedding rows - 1 (0: no integer feature matrix; pass a zero one-row table) */
  int32_t dtype;              /* EGT_F32, or EGT_BF16: e_out and d_e in bfloat16 (hop planes fp32) */
  int32_t num_float_features; /* 0..4 real-valued edge features per pair: keras Masking(mask_value) + Dense
                                 (lib/models/cifar10/dc.py:70-73); the rows of that Dense kernel are appended to
                                 adj_kernel ([upto_hop + num_float_features, De]) and its bias added to adj_bias */
  float mask_value;           /* Masking: a pair whose features all equal mask_value contributes 0 */
  int32_t reserved;
} egt_embed_desc;
int egt_edge_embed_supported(const egt_embed_desc* desc);
size_t egt_edge_embed_hops_bytes(const egt_embed_desc* desc);
size_t egt_edge_embed_workspace_bytes(const egt_embed_desc* desc);
int egt_edge_embed_fwd(const egt_embed_desc* desc, const int32_t* feature_matrix, const void* graph_matrix,
                       const void* float_features /* [B,N,N,num_float_features] or NULL */, const void* fm_table,
                       const void* adj_kernel, const void* adj_bias, void* hops, void* e_out, void* stream);
int egt_edge_embed_bwd(const egt_embed_desc* desc, const int32_t* feature_matrix, const void* hops,
                       const void* d_e, void* d_fm_table, void* d_adj_kernel, void* d_adj_bias,
                       void* workspace, void* stream);
/* The same embedding bordered with nv virtual nodes (VNModel, lib/models/graph_model_base.py:212-246;
 * VirtualEdgeEmbedding, lib/base/graph_layers/virtual_nodes.py:86-99), N' = nv + N, written once:
 *   e_out[b, nv+l, nv+m] = e0[b,l,m]              e_out[b, i, nv+m] = vn[i]   (every m < N, padded columns too)
 *   e_out[b, nv+l, j]    = vn[j]                  e_out[b, i, j]    = 0.5 (vn[i] + vn[j])
 * desc->N stays the number of real (padded) nodes; `hops` is unchanged ([K+F,B,N,N]).  vn_table / d_vn_table [nv,De] fp32;
 * e_out / d_e [B,N',N',De] in desc->dtype.  Covered: 1 <= nv <= 16 on a desc egt_edge_embed_supported accepts, with
 * N' N' De / 4 < 2^31.  The backward reads the interior of d_e for the three gradients above and its border for d_vn_table;
 * no atomics: two calls on the same inputs give the same bits. */
int egt_edge_embed_vn_supported(const egt_embed_desc* desc, int32_t nv);
size_t egt_edge_embed_vn_workspace_bytes(const egt_embed_desc* desc, int32_t nv);
int egt_edge_embed_vn_fwd(const egt_embed_desc* desc, int32_t nv, const int32_t* feature_matrix, const void* graph_matrix,
                          const void* float_features, const void* fm_table, const void* adj_kernel, const void* adj_bias,
                          const void* vn_table, void* hops, void* e_out, void* stream);
int egt_edge_embed_vn_bwd(const egt_embed_desc* desc, int32_t nv, const int32_t* feature_matrix, const void* hops,
                          const void* d_e, void* d_fm_table, void* d_adj_kernel, void* d_adj_bias, void* d_vn_table,
                          void* workspace, void* stream);

/* ---- distance objective (the reference's *_spe_do configs: distance_loss / distance_target) ----
 *   target    = round(sum_{k=1..T} hop_k), hop_1 = A, hop_k = clip(A . hop_{k-1}, 0, 1)     lib/models/graph_model_base.py:66-76
 *   logits    = Dense_t(act(Dense_1(act(Dense_0(edge_norm_final(e))))))   De -> M0 -> M1 -> C = T + 1   :83-94
 *   per_graph = sum over the pairs of a graph of CE(logits, target) * (target > 0)           lib/base/genutil/loss_layers.py:38-67
 * e [B,N,N,De] is the FINAL edge tensor (fp32, or bf16 with EGT_BF16; parameters, their gradients and the arithmetic are
 * fp32).  egt_distance_target: adj [B,N,N] fp32 -> target [B,N,N] uint8, N <= 192 (the graph's adjacency stays in LDS).
 * Covered: De in {8,16,32,48,64}, (M0, M1) in {(24,12), (32,16)}, 2 <= C <= 16, EGT_ACT_ELU / EGT_ACT_RELU, B*N*N < 2^31.
 * The backward recomputes the forward from e; d_per_graph [B] fp32 is the upstream gradient of per_graph_loss.  Kernels in
 * Keras layout [in, out].  No atomics: two calls on the same inputs give the same bits.  `workspace`
 * (egt_edge_head_workspace_bytes) is scratch: nothing is carried from the forward to the backward. */
#define EGT_EH_LAYERNORM 0x1 /* edge_norm_final (eps = ln_eps) before the head; off: gamma / beta may be NULL */
typedef struct egt_head_desc {
  int32_t B, N, De, M0, M1, C;
  int32_t dtype;      /* EGT_F32 or EGT_BF16: storage of e and d_e */
  int32_t activation; /* EGT_ACT_ELU or EGT_ACT_RELU (config.activation) */
  int32_t flags;      /* EGT_EH_LAYERNORM */
  float ln_eps;
  int32_t reserved;   /* 0 */
} egt_head_desc;

typedef struct egt_head_params {
  void* edge_norm_final_gamma;      /* [De] */
  void* edge_norm_final_beta;       /* [De] */
  void* mlp_out_dist_targ_0_kernel; /* [De, M0] */
  void* mlp_out_dist_targ_0_bias;   /* [M0] */
  void* mlp_out_dist_targ_1_kernel; /* [M0, M1] */
  void* mlp_out_dist_targ_1_bias;   /* [M1] */
  void* distance_target_kernel;     /* [M1, C] */
  void* distance_target_bias;       /* [C] */
} egt_head_params;

int egt_distance_target(const float* adj, int32_t B, int32_t N, int32_t T, uint8_t* target, void* stream);
int egt_edge_head_supported(const egt_head_desc* desc);
size_t egt_edge_head_workspace_bytes(const egt_head_desc* desc);
int egt_edge_head_fwd(const egt_head_desc* desc, const egt_head_params* params, const void* e, const uint8_t* target,
                      float* per_graph_loss /* [B] */, void* workspace, void* stream);
int egt_edge_head_bwd(const egt_head_desc* desc, const egt_head_params* params, const void* e, const uint8_t* target,
                      const float* d_per_graph /* [B] */, void* d_e, const egt_head_params* grads, void* workspace,
                      void* stream);

/* ---- node-classification head (the PATTERN / CLUSTER readout and its class-weighted loss) ----
 *   z     = Dense_t(act(Dense_1(act(Dense_0(node_norm_final(h))))))   W -> M0 -> M1 -> C     lib/models/sbm_pattern/dc.py:51-58
 *   stats = { sum_rows mask w[y] CE(z, y),  sum_rows mask [argmax_c z == y],  sum_rows mask }  lib/base/genutil/losses.py:41-118
 * over the R = B*N rows of h [B,N,W] fp32; target [B,N] int32, mask [B,N] uint8 (the node mask), class_weights [C] fp32.
 * The target of a masked row is never read as a class (any value there has no effect); on an arg-max tie the lowest class
 * wins.  No logits tensor is written.  The backward recomputes the forward from h; d_loss is a DEVICE pointer to the upstream
 * gradient of stats[0] (no host read: the step stays capturable); d_h gets exact zeros on masked rows.
 * Covered: W in {16,32,48,64}, (M0, M1) in {(24,12), (32,16)}, 2 <= C <= 16, EGT_ACT_ELU / EGT_ACT_RELU, B*N < 2^31.
 * Kernels in Keras layout [in, out].  No atomics: two calls on the same inputs give the same bits.  `workspace`
 * (egt_node_head_workspace_bytes) is scratch: nothing is carried from the forward to the backward. */
#define EGT_NH_LAYERNORM 0x1 /* node_norm_final (eps = ln_eps) before the head; off: gamma / beta may be NULL */
typedef struct egt_node_head_desc {
  int32_t B, N, W, M0, M1, C;
  int32_t activation; /* EGT_ACT_ELU or EGT_ACT_RELU (config.activation) */
  int32_t flags;      /* EGT_NH_LAYERNORM */
  float ln_eps;
  int32_t reserved;   /* 0 */
} egt_node_head_desc;

typedef struct egt_node_head_params {
  void* node_norm_final_gamma; /* [W] */
  void* node_norm_final_beta;  /* [W] */
  void* mlp_out_0_kernel;      /* [W, M0] */
  void* mlp_out_0_bias;        /* [M0] */
  void* mlp_out_1_kernel;      /* [M0, M1] */
  void* mlp_out_1_bias;        /* [M1] */
  void* target_kernel;         /* [M1, C] */
  void* target_bias;           /* [C] */
} egt_node_head_params;

int egt_node_head_supported(const egt_node_head_desc* desc);
size_t egt_node_head_workspace_bytes(const egt_node_head_desc* desc);
int egt_node_head_fwd(const egt_node_head_desc* desc, const egt_node_head_params* params, const float* h,
                      const int32_t* target, const uint8_t* mask, const float* class_weights, float* stats /* [3] */,
                      void* workspace, void* stream);
int egt_node_head_bwd(const egt_node_head_desc* desc, const egt_node_head_params* params, const float* h,
                      const int32_t* target, const uint8_t* mask, const float* class_weights,
                      const float* d_loss /* device, [1] */, float* d_h, const egt_node_head_params* grads, void* workspace,
                      void* stream);

/* ---- graph-level readout head (the ZINC / ZINC-full / CIFAR10 / MNIST readout and its loss) ----
 *   x      = node_norm_final(h)                                          h [B,N',W] fp32, N' = nv + N
 *   pooled = nv == 0 ? sum_n mask[b,n] x[b,n,:] / sum_n mask[b,n]        MaskedGlobalAvgPooling, lib/models/zinc/dc.py:109
 *                    : concat_{i<nv} x[b,i,:]                            GetVirtualNodes -> Flatten, zinc/dc.py:105-108   [B, max(nv,1) W]
 *   y      = Dense_t(act(Dense_1(act(Dense_0(pooled)))))                 max(nv,1) W -> M0 -> M1 -> C
 *   MAE :  stats = { sum_b sum_c |y - t|,         0,                     B*C }   target [B,C] fp32    schemes/zinc/svd.py:37-42
 *   XENT:  stats = { sum_b CE(y_b, t_b),  sum_b [argmax_c y_b == t_b],   B   }   target [B] int32     schemes/cifar10/svd.py:37-48
 * mask [B,N'] uint8 (the node mask, virtual rows included).  The parameter and gradient structs are egt_node_head_params with
 * mlp_out_0_kernel [max(nv,1) W, M0].  pred [B,C] (the predictions / logits) is written by the forward; on an arg-max tie the
 * lowest class wins.  With nv == 0 a masked row never enters the pooled sum (a predicate, not a product: its content is never
 * used); with nv > 0 only the first nv rows of a graph are read and the mask is not consulted (virtual rows are real by
 * construction).  Where |y - t| is exactly 0 the MAE gradient is 0.  The backward recomputes the forward from h; d_loss is a
 * DEVICE pointer to the upstream gradient of stats[0] (no host read, allocation or synchronisation: the step stays
 * capturable); d_h gets exact zeros on masked rows (nv == 0) / on every row >= nv (nv > 0).  A graph without a real node is
 * 0/0 as in the reference (outside the contract; the kernels stay inside their buffers).
 * Covered: W in {48,64}, (M0, M1) in {(24,12), (32,16)}, 1 <= C <= 16, 0 <= nv <= 4, EGT_ACT_ELU / EGT_ACT_RELU, any N >= 1,
 * B*N' < 2^31.  Kernels in Keras layout [in, out].  No atomics: the sums over rows and over graphs run in a fixed order, two
 * calls on the same inputs give the same bits.  `workspace` (egt_graph_head_workspace_bytes) is scratch: nothing is carried
 * from the forward to the backward. */
#define EGT_GH_LAYERNORM 0x1 /* node_norm_final (eps = ln_eps) before the pooling; off: gamma / beta may be NULL */
#define EGT_GH_MAE 0
#define EGT_GH_XENT 1
typedef struct egt_graph_head_desc {
  int32_t B, N, W, M0, M1, C;
  int32_t nv;         /* virtual nodes in front of every graph's N nodes (0: masked mean pooling) */
  int32_t loss;       /* EGT_GH_MAE or EGT_GH_XENT */
  int32_t activation; /* EGT_ACT_ELU or EGT_ACT_RELU (config.activation) */
  int32_t flags;      /* EGT_GH_LAYERNORM */
  float ln_eps;
  int32_t reserved;   /* 0 */
} egt_graph_head_desc;

int egt_graph_head_supported(const egt_graph_head_desc* desc);
size_t egt_graph_head_workspace_bytes(const egt_graph_head_desc* desc);
int egt_graph_head_fwd(const egt_graph_head_desc* desc, const egt_node_head_params* params, const float* h,
                       const void* target, const uint8_t* mask, float* stats /* [3] */, float* pred /* [B,C] */,
                       void* workspace, void* stream);
int egt_graph_head_bwd(const egt_graph_head_desc* desc, const egt_node_head_params* params, const float* h,
                       const void* target, const uint8_t* mask, const float* d_loss /* device, [1] */, float* d_h,
                       const egt_node_head_params* grads, void* workspace, void* stream);

/* ---- node-input embedding: from a batch's node features to the stack's h and mask ----
 * One launch writes h_out [B,nv+N,Dh] fp32 and mask_out [B,nv+N] uint8 (1 = real node):
 *   rows 0..nv-1 : virtual_node_emb [nv,Dh], mask 1                          lib/base/graph_layers/virtual_nodes.py:31-50
 *   row nv+n     : base + encoding
 *     EGT_NE_INT    base = node_emb[features[b,n] + 1]    features [B,N] int32, padding -1 -> row 0 (an ordinary trainable
 *                   row), mask = features != -1; node_emb [R,Dh]             lib/base/xformer_layers/masking.py:31-43
 *     EGT_NE_FLOAT  base = (x m) node_emb + node_emb_bias, m = any_f(x[f] != mask_value): keras Masking + Dense, mask = m;
 *                   features [B,N,F] fp32, node_emb [F,Dh]                   lib/models/cifar10/dc.py:66-69
 *     EGT_NE_PE_SVD pe [B,N,T,2]: x = (s_0 u_0 .. s_{sel-1} u_{sel-1}, s_0 v_0 .. s_{sel-1} v_{sel-1}) from the first sel of the T
 *                   stored pairs (u = pe[..,k,0], v = pe[..,k,1]); under EGT_NE_TRANSFORM the encoding is x pe_kernel + pe_bias
 *                   (pe_kernel [2 sel, Dh]), otherwise u is added to channels 0..sel-1 and v to Dh/2..Dh/2+sel-1
 *     EGT_NE_PE_EIG pe [B,N,T]: x = (s_0 w_0 .. s_{sel-1} w_{sel-1}); x pe_kernel + pe_bias (pe_kernel [sel, Dh]) under
 *                   EGT_NE_TRANSFORM, otherwise added to channels 0..sel-1   lib/models/graph_model_base.py:284-414
 *   signs (EGT_NE_SIGNS): s_k = signs[b * sign_stride + k], the caller's sample of the training-time sign flip (+-1 floats,
 *   lib/base/genutil/misc.py:53-94); without the flag every s_k is 1 and `signs` may be NULL.  The library draws nothing.
 * The backward takes d_h [B,nv+N,Dh] and writes, through `grads` (the same struct), the gradients of node_emb, node_emb_bias
 * (float kind), pe_kernel / pe_bias (EGT_NE_TRANSFORM) and virtual_node_emb (nv > 0); pointers the geometry does not use are
 * never touched and may be NULL.  The sums run over ALL B N rows, padded rows included (a Dense bias gradient counts them; a
 * padded integer row adds to table row 0), as autograd of the composed ops gives.  There are no input gradients.  It needs no
 * parameter values.  Per-workgroup partials in `workspace` (egt_node_embed_workspace_bytes; scratch) and a fixed-order
 * finish launch: no atomics, two calls on the same inputs give the same bits.  Parameters and gradient sinks need 4-byte
 * alignment only (16-byte accesses are used where a pointer allows them); h_out, d_h likewise.  features, pe, signs and d_h are
 * const; every element of h_out, mask_out and of each used sink is written exactly once per call.
 * Covered: Dh in {16,32,48,64}, 1 <= R <= 32, 1 <= F <= 8, 1 <= sel <= 32 with T >= sel, 2 sel <= Dh (SVD) / sel <= Dh (EIG)
 * without EGT_NE_TRANSFORM, 0 <= nv <= 16, any N >= 1, B >= 1 with B (nv+N) 64 < 2^31. */
#define EGT_NE_INT 0
#define EGT_NE_FLOAT 1
#define EGT_NE_PE_NONE 0
#define EGT_NE_PE_SVD 1
#define EGT_NE_PE_EIG 2
#define EGT_NE_TRANSFORM 0x1 /* the encoding goes through its Dense (pe_kernel, pe_bias) */
#define EGT_NE_SIGNS 0x2     /* `signs` holds the sign sample */
typedef struct egt_node_embed_desc {
  int32_t B, N, Dh;
  int32_t nv;          /* virtual nodes in front of every graph's N nodes */
  int32_t kind;        /* EGT_NE_INT or EGT_NE_FLOAT */
  int32_t R;           /* EGT_NE_INT: rows of node_emb (num_node_features + 1); 0 otherwise */
  int32_t F;           /* EGT_NE_FLOAT: feature columns; 0 otherwise */
  int32_t pe_kind;     /* EGT_NE_PE_* */
  int32_t T;           /* stored pairs / eigenvector entries per node (the stride of pe); 0 without an encoding */
  int32_t sel;         /* how many of them are used */
  int32_t flags;       /* EGT_NE_TRANSFORM | EGT_NE_SIGNS */
  float mask_value;    /* EGT_NE_FLOAT: keras Masking's value */
  int32_t sign_stride; /* floats between two graphs' signs; 0 = sel */
  int32_t reserved;    /* 0 */
} egt_node_embed_desc;

typedef struct egt_node_embed_params {
  void* node_emb;         /* [R, Dh] table / [F, Dh] Dense kernel */
  void* node_emb_bias;    /* [Dh], EGT_NE_FLOAT */
  void* pe_kernel;        /* [2 sel, Dh] (SVD) / [sel, Dh] (EIG), EGT_NE_TRANSFORM */
  void* pe_bias;          /* [Dh], EGT_NE_TRANSFORM */
  void* virtual_node_emb; /* [nv, Dh], nv > 0 */
} egt_node_embed_params;

int egt_node_embed_supported(const egt_node_embed_desc* desc);
size_t egt_node_embed_workspace_bytes(const egt_node_embed_desc* desc);
int egt_node_embed_fwd(const egt_node_embed_desc* desc, const egt_node_embed_params* params, const void* features,
                       const float* pe, const float* signs, float* h_out, uint8_t* mask_out, void* stream);
int egt_node_embed_bwd(const egt_node_embed_desc* desc, const void* features, const float* pe, const float* signs,
                       const float* d_h, const egt_node_embed_params* grads, void* workspace, void* stream);

/* ---- batch data parallelism: the gradient all-reduce on RCCL -------------------
 * Replaces what tf.distribute.MirroredStrategy does for the reference
 * (lib/training/training_base.py:230-247): one synchronous all-reduce of every
 * parameter gradient per step.  One process per GPU and ONE communicator per process
 * (the library's only global state).  Bootstrap: rank 0 calls egt_dp_unique_id and
 * hands the 128 bytes to every rank out of band (the launcher's TCP store); every
 * rank then calls egt_dp_init with its HIP device current.  egt_dp_allreduce reduces
 * `count` fp32 values in place on `stream` (the stream the backward ran on; no host
 * synchronisation) -- SUM, or the mean over ranks when average != 0.  RCCL is resolved
 * at run time (the copy already mapped into the process, else librccl.so.1); its
 * absence is EGT_E_RCCL, not a load failure of this library. */
#define EGT_DP_ID_BYTES 128
int egt_dp_unique_id(void* id_out /* host, EGT_DP_ID_BYTES */);
int egt_dp_init(const void* id /* host, EGT_DP_ID_BYTES */, int32_t world, int32_t rank);
int egt_dp_allreduce(void* buf, size_t count, int32_t average, void* stream);
int egt_dp_world(void); /* 0 before init */
int egt_dp_rank(void);  /* -1 before init */
int egt_dp_finalize(void);

/* ---- per-kernel timing (measurement only) ------------------------------------
 * egt_prof_enable(1) makes every launch site bracket its kernel with hipEvents
 * on the launch stream (2 = reset counters and enable, 0 = off).  After the
 * caller has synchronised, egt_prof_read(name, ...) returns the launch count
 * and summed milliseconds of kernel `name`; egt_prof_names lists the names. */
int egt_prof_enable(int on);
int egt_prof_filter(const char* kernel_name); /* time only this kernel (NULL/"" = all) */
int egt_prof_stride(int every);               /* time every `every`-th launch of each timed kernel (default 1 = all): an event pair
                                                * costs the stream a few microseconds, a sample keeps a throughput measurement honest */
int egt_prof_read(const char* name, int64_t* count, double* total_ms);
/* Launches captured into a hipGraph while the profile is enabled carry their hipEvents as event-record nodes of
 * that graph; every replay re-records them.  After a replay has completed, egt_prof_collect_graph() adds its elapsed times to
 * the kernels' counts / sums (reset_counts != 0: zero them first) and returns the number of event pairs read. */
int egt_prof_collect_graph(int reset_counts);
int egt_prof_forget_graphs(void);             /* drop the event pairs of captured graphs from the profile (the graphs may go on replaying) */
int egt_prof_names(char* buf, size_t cap);

/* ---- fused flat optimizer: the parameter update of a step as two launches -----
 * Adam / RMSprop / SGD with torch.optim's arithmetic (what the training driver runs: lib/training/training_base.py:59-72)
 * over flat buffers in the layout of FlatGradAllReduce: element k of `grad`, `m`, `v` belongs to the parameter whose running
 * sum of element counts covers k; no padding.  The parameters stay separate tensors, reached through `table`: device-resident
 * work items {param, offset, count} -- `count` floats at `param` pair with the flat elements [offset, offset + count).  The host
 * cuts the table so that no item straddles a parameter (egt_amd.optim.plan_items: at most 2048 elements per item; the kernel
 * takes any count >= 1) and one workgroup runs one item.  `param` needs 4-byte alignment and `offset` is any float offset;
 * grad / m / v are 16-byte-aligned buffers of exactly `total` floats; nothing outside an item's floats is read or written.
 * An element's result does not depend on the item it falls into.
 *   EGT_OPT_ADAM     m = lerp(m, g, 1-beta1); v = beta2 v + (1-beta2) g^2; p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
 *   EGT_OPT_RMSPROP  v = beta2 v + (1-beta2) g^2 (beta2 is RMSprop's alpha);  p -= lr g / (sqrt(v) + eps);  m ignored (NULL accepted)
 *   EGT_OPT_SGD      p -= lr g;  m and v ignored (NULL accepted)
 * with g = grad * grad_scale, clamped to +-clip_value under EGT_OPT_CLIP (Keras clipvalue).  Under EGT_OPT_ZERO_GRAD every
 * gradient element is set to 0 after it was read: `grad` is written, which is why it is not const.
 * State block: EGT_OPTIM_STATE_BYTES on the device, 8-byte aligned.  Kernel arguments are frozen when a hipGraph is captured,
 * so what changes from step to step lives here.  The host owns the first 24 bytes:
 *   int64 t (steps taken so far; 0 for a fresh run), double lr, float grad_scale, 4 bytes padding
 * and updates lr / grad_scale with a plain copy (bytes 8..23); the rest belongs to the library.  egt_optim_prepare (ONE thread)
 * increments t and forms step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) in fp64; egt_optim_step reads them and
 * writes no state.  A step is egt_optim_prepare, then egt_optim_step, on one stream; both are capturable. */
#define EGT_OPT_ADAM 0
#define EGT_OPT_RMSPROP 1
#define EGT_OPT_SGD 2
#define EGT_OPT_CLIP 0x1u      /* clamp g to [-clip_value, clip_value] before use */
#define EGT_OPT_ZERO_GRAD 0x2u /* store 0 to each gradient element after reading it */
#define EGT_OPTIM_STATE_BYTES 64
typedef struct {
  int32_t algo;         /* EGT_OPT_ADAM / _RMSPROP / _SGD */
  uint32_t flags;       /* EGT_OPT_* */
  int32_t num_segments; /* entries of `table` = workgroups */
  int32_t reserved;     /* 0 */
  int64_t total;        /* floats in grad / m / v = sum of the counts */
  double beta1;         /* Adam */
  double beta2;         /* Adam's beta2, RMSprop's alpha */
  float eps;
  float clip_value;     /* EGT_OPT_CLIP */
} egt_optim_desc;
typedef struct {
  float* param;   /* first float of the item in its parameter */
  int64_t offset; /* of the item in the flat buffers, in floats */
  int64_t count;  /* >= 1 */
} egt_optim_segment; /* 24 bytes */
int egt_optim_supported(const egt_optim_desc* desc);
int egt_optim_prepare(const egt_optim_desc* desc, void* state, void* stream);
int egt_optim_step(const egt_optim_desc* desc, const egt_optim_segment* table /* device */, float* grad, float* m, float* v,
                   void* state, void* stream);

/* ---- device-resident datasets: the padded tensors of a batch from a split's packed records ----
 * What egt_amd.data.GraphDataset (collate + the per-record maps; lib/data/graph.py:4-42, dataset_base.py:100-130) builds on
 * the host, bit for bit, from records that live in device memory: only the B record indices `idx` change per batch.
 * Store (all const, device; egt_amd.device_data.pack_split writes it).  Record r has n = num_nodes[r] nodes whose rows start
 * at node_off[r], and edge_off[r+1] - edge_off[r] edges starting at edge_off[r], STABLY sorted by source row, so the
 * duplicates of one (i,j) keep the order of the edge list:
 *   num_nodes [R] int32;  node_off [R+1] int64;  edge_off [R+1] int64
 *   row_off   [node_off[R] + R] int32: entries node_off[r] + r + i, i = 0..n: first edge of row i, relative to edge_off[r]
 *   edge_dst  [E] int32 (0 <= dst < n);  edge_feat [E] int32 / fp32 (edge_kind)
 *   node_rows [node_off[R], node_width] int32 / fp32 (node_kind);  pe_rows [node_off[R], F, 2] (SVD) / [node_off[R], F] (EIGEN) fp32
 *   targets   [R] fp32 (TGT_GRAPH_F32: the output is [B,1]) / [R] int32 (TGT_GRAPH_I32) / [node_off[R]] int32 (TGT_NODE_I32)
 * Outputs (device, 16-byte aligned, exactly these element counts; NULL = not asked for and not written):
 *   graph_matrix   [B,N,N] fp32: inside n x n the count of (i,j) in the edge list + 1 on the diagonal; matrix_pad outside
 *   feature_matrix [B,N,N] int32 / fp32: inside n x n (sum over the (i,j) duplicates, in edge-list order, of (feat + m)) - m
 *                  starting from 0, m = 1 under EGT_BATCH_MARK_INVALID else 0; mask_i / mask_f outside
 *   node_features  [B,N,node_width]: the record's rows, then mask_i / mask_f;   pe [B,N,F,2] / [B,N,F]: rows, then 0
 *   target         [B] words, or [B,N] int32: rows, then 0;   num_nodes [B] int32
 * Every element of every requested output is written exactly once per call and nothing is read back: the result does not
 * depend on what the outputs held.  No output may overlap the store, idx or another output.  Only records idx[b] of the store
 * are read; an idx[b] outside [0, R) gives an empty graph (all padding, num_nodes 0, target 0).  N must be >= every n of the
 * batch (rows beyond N would be dropped).  No workspace, no host synchronisation, no atomics; capturable.
 * Covered: 1 <= N <= 512, B N N < 2^31, node / PE rows of at most 64 words, one value per edge. */
#define EGT_BATCH_NONE 0
#define EGT_BATCH_I32 1
#define EGT_BATCH_F32 2
#define EGT_BATCH_PE_NONE 0
#define EGT_BATCH_PE_SVD 1   /* rows of [F,2] floats */
#define EGT_BATCH_PE_EIGEN 2 /* rows of [F] floats */
#define EGT_BATCH_TGT_GRAPH_F32 0
#define EGT_BATCH_TGT_GRAPH_I32 1
#define EGT_BATCH_TGT_NODE_I32 2
#define EGT_BATCH_MARK_INVALID 0x1u /* feature_matrix: feat + 1 summed, - 1 at the end (non-edges become -1) */
typedef struct egt_batch_desc {
  int32_t B, N;
  int32_t records;                /* R */
  int32_t node_kind, node_width;  /* EGT_BATCH_I32 (width 1) or EGT_BATCH_F32 */
  int32_t edge_kind, edge_width;  /* EGT_BATCH_NONE (width 0), _I32 or _F32 (width 1) */
  int32_t pe_kind, pe_features;   /* EGT_BATCH_PE_*; F (0 without) */
  int32_t target_kind;            /* EGT_BATCH_TGT_* */
  uint32_t flags;                 /* EGT_BATCH_MARK_INVALID */
  float matrix_pad;               /* graph_matrix outside n x n */
  float mask_f;                   /* fp32 node rows / feature_matrix outside the graph */
  int32_t mask_i;                 /* int32 node rows / feature_matrix outside the graph */
  int32_t reserved[2];            /* 0 */
} egt_batch_desc;
typedef struct egt_batch_store {
  const int32_t* num_nodes;
  const int64_t* node_off;
  const int64_t* edge_off;
  const int32_t* row_off;
  const int32_t* edge_dst;
  const void* edge_feat;
  const void* node_rows;
  const float* pe_rows;
  const void* targets;
} egt_batch_store;
typedef struct egt_batch_out {
  float* graph_matrix;
  void* feature_matrix;
  void* node_features;
  float* pe;
  void* target;
  int32_t* num_nodes;
} egt_batch_out;
int egt_batch_supported(const egt_batch_desc* desc);
int egt_batch_assemble(const egt_batch_desc* desc, const egt_batch_store* store, const int32_t* idx /* device, [B] */,
                       const egt_batch_out* out, void* stream);
/* egt_batch_assemble with idx = idx_table + *cursor: the B indices of the batch are idx_table[*cursor .. *cursor + B).  `cursor`
 * (device, 8-byte aligned) is read by the kernel when it RUNS, as egt_block_desc.seed_device is, so a captured launch walks the
 * table from replay to replay while egt_seed_advance(cursor, 1, B, stream) moves the cursor behind it.  The caller keeps
 * *cursor + B inside the table.  Checks, outputs and coverage are egt_batch_assemble's; the table and the cursor are only read. */
int egt_batch_assemble_at(const egt_batch_desc* desc, const egt_batch_store* store, const int32_t* idx_table /* device, int32[capacity] */,
                          const uint64_t* cursor /* device */, const egt_batch_out* out, void* stream);

/* ---- resident training step: epoch sums of (metric sum, count) pairs on the device ----
 * One launch of one wave: for k < K   acc[2k] += (double)*items[k].sum;   acc[2k+1] += items[k].count ? (double)*items[k].count
 * : (double)items[k].count_value.  `items` (device, 8-byte aligned) and what it points to are only read, when the kernel runs;
 * nothing outside acc[0 .. 2K) is written.  The additions of a pair happen in launch order, in fp64: the accumulator holds
 * what the same sequence of `a += (double)x` gives on the host.  Plain stores, no atomics, no workspace; capturable.
 * EGT_E_NULL (acc / items) and EGT_E_SHAPE (K outside 1..32, an unaligned pointer) are returned before any launch. */
typedef struct egt_acc_item {
  const float* sum;   /* device: this step's sum */
  const float* count; /* device: this step's count, or NULL */
  float count_value;  /* the count where `count` is NULL */
} egt_acc_item;       /* 24 bytes */
int egt_accumulate(double* acc /* device, [2K] */, const egt_acc_item* items /* device, [K] */, int32_t K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGT_AMD_H_ */
