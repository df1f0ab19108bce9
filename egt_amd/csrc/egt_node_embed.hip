// Node-input embedding of every model (include/egt_amd.h, "node-input embedding"): from a batch's node features to the
// h [B,nv+N,Dh] and mask [B,nv+N] that enter the layer stack.
//   rows 0..nv-1 : virtual_node_emb, mask 1                                   lib/base/graph_layers/virtual_nodes.py:31-50
//   row  nv+n    : table[features + 1]                (integer kind)          lib/base/xformer_layers/masking.py:31-43
//                  (x m) W + b, m = any(x != mask_value)   (float kind)       lib/models/cifar10/dc.py:66-69
//                + the SVD / eigenvector encoding, through its Dense or added to its channels
//                                                                            lib/models/graph_model_base.py:284-414
// Forward: one launch.  A 16-lane row of a wave owns one output row (float4 per lane, the lanes past Dh idle); the parameters
// (at most 8 KiB of table and 16 KiB of encoding kernel) are read through the cache, not staged: a workgroup's 64 rows would
// not pay for the copy.
// Backward: the parameter gradients are sums over all B N real rows of x_j d_h[c].  k_node_embed_bwd gives a workgroup a
// contiguous run of rows; per 32-row tile it stages d_h and the rows' inputs x (encoding values, masked features, a constant 1
// for the bias) in LDS, and every thread owns gradient elements (j, c) in registers: no atomics, the rows of a workgroup are
// summed in index order.  Each workgroup leaves one partial in the workspace; k_node_embed_finish sums the partials in index
// order, one thread per gradient element, and sums d_h's virtual rows over the graphs.  Two runs give the same bits.
#include "egt_common.h"
#include <cstring>

#define NE_NT 256
#define NE_FWD_ROWS 64           // output rows per forward workgroup
#define NE_TILE 32               // rows per backward tile
#define NE_ROWS_PER_WG 128       // backward: rows a workgroup sums before it writes its partial
#define NE_MAX_WG 256
#define NE_MAX_SEL 32
#define NE_MAX_R 32
#define NE_MAX_F 8
#define NE_MAX_NV 16
#define NE_XMAX (2 * NE_MAX_SEL + NE_MAX_F + 1)   // widest input row of the backward: encoding | features | 1
#define NE_XPT ((NE_XMAX + 3) / 4)                // input columns a backward thread owns
#define NE_TPT (NE_MAX_R / 4)                     // table rows a backward thread owns

struct NeGeo {
  int B, N, NP, Dh, nv, kind, R, F, pe, T, sel, transform, has_signs, sstride;
  float mask_value;
};

struct NeParams { float* p[5]; };   // node_emb, node_emb_bias, pe_kernel, pe_bias, virtual_node_emb
static_assert(sizeof(egt_node_embed_params) == sizeof(NeParams), "the parameter struct is five pointers");

// four consecutive floats of a parameter: one 16-byte load where the caller found the tensor 16-byte aligned (rows are
// multiples of 64 bytes: the base decides for every row), four scalar loads otherwise
__device__ __forceinline__ float4 ne_ld4(const float* p, bool al) {
  if (al) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
__device__ __forceinline__ void ne_fma4(float4& a, float x, float4 w) {
  a.x = fmaf(x, w.x, a.x); a.y = fmaf(x, w.y, a.y); a.z = fmaf(x, w.z, a.z); a.w = fmaf(x, w.w, a.w);
}
__device__ __forceinline__ bool ne_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// input j of the encoding's Dense for node row gn of graph b: (u_0..u_{sel-1}, v_0..v_{sel-1}) of the SVD pairs, the first
// sel eigenvector entries otherwise, times the graph's sign of that pair
__device__ __forceinline__ float ne_pe_x(const float* __restrict__ pe, const float* __restrict__ signs, const NeGeo& g, size_t gn,
                                         int b, int j) {
  int k = j, o = j;
  if (g.pe == EGT_NE_PE_SVD) { k = j < g.sel ? j : j - g.sel; o = 2 * k + (j < g.sel ? 0 : 1); }
  float x = pe[gn * (size_t)(g.pe == EGT_NE_PE_SVD ? 2 * g.T : g.T) + o];
  if (g.has_signs) x *= signs[(size_t)b * g.sstride + k];
  return x;
}

__global__ void __launch_bounds__(NE_NT) k_node_embed_fwd(const void* __restrict__ feat, const float* __restrict__ pe,
                                                          const float* __restrict__ signs, const NeParams P,
                                                          float* __restrict__ h_out, uint8_t* __restrict__ mask_out, const NeGeo g) {
  const int tid = threadIdx.x, q = tid & 15;
  const int Dh = g.Dh;
  const bool col = 4 * q < Dh;
  const bool al_e = ne_al16(P.p[0]), al_b = ne_al16(P.p[1]), al_k = ne_al16(P.p[2]), al_kb = ne_al16(P.p[3]), al_v = ne_al16(P.p[4]);
  const bool al_h = ne_al16(h_out);
  const long total = (long)g.B * g.NP;
#pragma unroll 1
  for (int pass = 0; pass < NE_FWD_ROWS / 16; ++pass) {
    const long row = (long)blockIdx.x * NE_FWD_ROWS + pass * 16 + (tid >> 4);
    if (row >= total) continue;
    const int b = (int)(row / g.NP), r = (int)(row - (long)b * g.NP);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    uint8_t m = 1;
    if (r < g.nv) {
      if (col) acc = ne_ld4(P.p[4] + r * Dh + 4 * q, al_v);
    } else {
      const size_t gn = (size_t)b * g.N + (r - g.nv);
      if (g.kind == EGT_NE_INT) {
        const int f = reinterpret_cast<const int32_t*>(feat)[gn];
        m = f != -1;
        int idx = f + 1;
        idx = idx < 0 ? 0 : (idx >= g.R ? g.R - 1 : idx);        // (outside the contract: stay inside the table)
        if (col) acc = ne_ld4(P.p[0] + idx * Dh + 4 * q, al_e);
      } else {
        const float* x = reinterpret_cast<const float*>(feat) + gn * g.F;
        bool any = false;
        for (int f = 0; f < g.F; ++f) any = any || (x[f] != g.mask_value);
        m = any;
        if (col) {
          acc = ne_ld4(P.p[1] + 4 * q, al_b);
          const float mf = any ? 1.f : 0.f;
          for (int f = 0; f < g.F; ++f) ne_fma4(acc, x[f] * mf, ne_ld4(P.p[0] + f * Dh + 4 * q, al_e));
        }
      }
      if (g.pe != EGT_NE_PE_NONE && col) {
        if (g.transform) {
          const int J = g.pe == EGT_NE_PE_SVD ? 2 * g.sel : g.sel;
          float4 t = ne_ld4(P.p[3] + 4 * q, al_kb);
          for (int j = 0; j < J; ++j) ne_fma4(t, ne_pe_x(pe, signs, g, gn, b, j), ne_ld4(P.p[2] + j * Dh + 4 * q, al_k));
          acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
        } else {
          // no Dense: u in channels 0..sel-1 and v in Dh/2..Dh/2+sel-1 (SVD), the eigenvector entries in 0..sel-1
          float a[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int c = 4 * q + i, half = Dh >> 1;
            int j = -1;
            if (c < g.sel) j = c;
            else if (g.pe == EGT_NE_PE_SVD && c >= half && c - half < g.sel) j = g.sel + (c - half);
            if (j >= 0) a[i] += ne_pe_x(pe, signs, g, gn, b, j);
          }
          acc = make_float4(a[0], a[1], a[2], a[3]);
        }
      }
    }
    if (col) {
      float* o = h_out + (size_t)row * Dh + 4 * q;
      if (al_h) *reinterpret_cast<float4*>(o) = acc;
      else { o[0] = acc.x; o[1] = acc.y; o[2] = acc.z; o[3] = acc.w; }
    }
    if (q == 0) mask_out[row] = m;
  }
}

// rows of a workgroup's partial (each Dh floats): encoding kernel [JP] | float kernel [F] | bias [1] | table [R]
struct NeBwdGeo { int JP, JX, PR, rows_per_wg; };   // JX = JP + F + 1 input columns, PR = JX + R partial rows

__global__ void __launch_bounds__(NE_NT) k_node_embed_bwd(const void* __restrict__ feat, const float* __restrict__ pe,
                                                          const float* __restrict__ signs, const float* __restrict__ d_h,
                                                          float* __restrict__ part, const NeGeo g, const NeBwdGeo bg) {
  __shared__ __attribute__((aligned(16))) float s_dh[NE_TILE][64];
  __shared__ float s_x[NE_TILE][NE_XMAX + 1];
  __shared__ int s_idx[NE_TILE];
  __shared__ float s_m[NE_TILE];

  const int tid = threadIdx.x, c = tid & 63, jg = tid >> 6, Dh = g.Dh;
  const long total = (long)g.B * g.N;
  const long first = (long)blockIdx.x * bg.rows_per_wg;
  const long last = first + bg.rows_per_wg < total ? first + bg.rows_per_wg : total;
  const int JP = bg.JP, JX = bg.JX;
  const bool al_d = ne_al16(d_h);

  float ax[NE_XPT], at[NE_TPT];
#pragma unroll
  for (int i = 0; i < NE_XPT; ++i) ax[i] = 0.f;
#pragma unroll
  for (int i = 0; i < NE_TPT; ++i) at[i] = 0.f;

#pragma unroll 1
  for (long t0 = first; t0 < last; t0 += NE_TILE) {
    __syncthreads();                      // the previous tile is consumed
    // d_h of the tile's rows (zeros past the run), the row's table index / Masking flag
    for (int i = tid; i < NE_TILE * 16; i += NE_NT) {
      const int lr = i >> 4, q = i & 15;
      const long gn = t0 + lr;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gn < last && 4 * q < Dh) {
        const int b = (int)(gn / g.N), n = (int)(gn - (long)b * g.N);
        const float* s = d_h + ((size_t)b * g.NP + g.nv + n) * Dh + 4 * q;
        v = al_d ? *reinterpret_cast<const float4*>(s) : make_float4(s[0], s[1], s[2], s[3]);
      }
      *reinterpret_cast<float4*>(&s_dh[lr][4 * q]) = v;
    }
    if (tid < NE_TILE) {
      const long gn = t0 + tid;
      int idx = -1;
      float m = 0.f;
      if (gn < last) {
        if (g.kind == EGT_NE_INT) {
          idx = reinterpret_cast<const int32_t*>(feat)[gn] + 1;
          idx = idx < 0 ? 0 : (idx >= g.R ? g.R - 1 : idx);
        } else {
          const float* x = reinterpret_cast<const float*>(feat) + (size_t)gn * g.F;
          bool any = false;
          for (int f = 0; f < g.F; ++f) any = any || (x[f] != g.mask_value);
          m = any ? 1.f : 0.f;
        }
      }
      s_idx[tid] = idx;
      s_m[tid] = m;
    }
    __syncthreads();
    // the rows' inputs: encoding values | masked features | 1 (zeros past the run: such a row adds nothing)
    for (int i = tid; i < NE_TILE * JX; i += NE_NT) {
      const int lr = i / JX, j = i - lr * JX;
      const long gn = t0 + lr;
      float x = 0.f;
      if (gn < last) {
        if (j < JP) x = ne_pe_x(pe, signs, g, (size_t)gn, (int)(gn / g.N), j);
        else if (j < JX - 1) x = reinterpret_cast<const float*>(feat)[(size_t)gn * g.F + (j - JP)] * s_m[lr];
        else x = 1.f;
      }
      s_x[lr][j] = x;
    }
    __syncthreads();
    if (c < Dh) {
#pragma unroll 4
      for (int lr = 0; lr < NE_TILE; ++lr) {
        const float d = s_dh[lr][c];
#pragma unroll
        for (int i = 0; i < NE_XPT; ++i) {
          const int j = jg + 4 * i;
          if (j < JX) ax[i] = fmaf(s_x[lr][j], d, ax[i]);
        }
        if (g.kind == EGT_NE_INT) {
          const int idx = s_idx[lr];
#pragma unroll
          for (int i = 0; i < NE_TPT; ++i) at[i] += (idx == jg + 4 * i) ? d : 0.f;
        }
      }
    }
  }
  if (c < Dh) {
    float* o = part + (size_t)blockIdx.x * bg.PR * Dh;
#pragma unroll
    for (int i = 0; i < NE_XPT; ++i) {
      const int j = jg + 4 * i;
      if (j < JX) o[j * Dh + c] = ax[i];
    }
    if (g.kind == EGT_NE_INT) {
#pragma unroll
      for (int i = 0; i < NE_TPT; ++i) {
        const int r = jg + 4 * i;
        if (r < g.R) o[(JX + r) * Dh + c] = at[i];
      }
    }
  }
}

// sum over the workgroups' partials in index order (four interleaved chains, combined in a fixed order)
__device__ __forceinline__ float ne_sum(const float* __restrict__ a, int n, size_t stride) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    s0 += a[(size_t)i * stride]; s1 += a[(size_t)(i + 1) * stride]; s2 += a[(size_t)(i + 2) * stride]; s3 += a[(size_t)(i + 3) * stride];
  }
  for (; i < n; ++i) s0 += a[(size_t)i * stride];
  return (s0 + s1) + (s2 + s3);
}

// One thread per gradient element: node_emb (table rows / float kernel rows) | node_emb_bias | pe_kernel | pe_bias from the
// partials, virtual_node_emb from d_h's virtual rows.  Both Dense biases are the same sum (every real row adds d_h to each).
__global__ void __launch_bounds__(256) k_node_embed_finish(const float* __restrict__ part, const float* __restrict__ d_h,
                                                           const NeParams G, const NeGeo g, const NeBwdGeo bg, int nwg) {
  const int Dh = g.Dh, JP = bg.JP;
  const size_t stride = (size_t)bg.PR * Dh;
  const int n_emb = (g.kind == EGT_NE_INT ? g.R : g.F) * Dh, n_eb = g.kind == EGT_NE_INT ? 0 : Dh;
  const int n_k = JP * Dh, n_kb = JP > 0 ? Dh : 0;
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_emb) {
    const int prow = g.kind == EGT_NE_INT ? bg.JX + i / Dh : JP + i / Dh;
    G.p[0][i] = ne_sum(part + (size_t)prow * Dh + i % Dh, nwg, stride);
    return;
  }
  i -= n_emb;
  if (i < n_eb) { G.p[1][i] = ne_sum(part + (size_t)(bg.JX - 1) * Dh + i, nwg, stride); return; }
  i -= n_eb;
  if (i < n_k) { G.p[2][i] = ne_sum(part + i, nwg, stride); return; }
  i -= n_k;
  if (i < n_kb) { G.p[3][i] = ne_sum(part + (size_t)(bg.JX - 1) * Dh + i, nwg, stride); return; }
  i -= n_kb;
  if (i < g.nv * Dh) G.p[4][i] = ne_sum(d_h + i, g.B, (size_t)g.NP * Dh);
}

// =================================== host ===================================
static int node_embed_check(const egt_node_embed_desc* d) {
  if (!d) EGT_FAIL(EGT_E_NULL, "desc is NULL");
  if ((d->flags & ~(int32_t)(EGT_NE_TRANSFORM | EGT_NE_SIGNS)) != 0 || d->reserved != 0)
    EGT_FAIL(EGT_E_FLAGS, "node embed: unknown flag bits 0x%x / reserved %d", (unsigned)d->flags, d->reserved);
  if (d->kind != EGT_NE_INT && d->kind != EGT_NE_FLOAT)
    EGT_FAIL(EGT_E_FLAGS, "node embed: kind is EGT_NE_INT or EGT_NE_FLOAT (got %d)", d->kind);
  if (d->pe_kind != EGT_NE_PE_NONE && d->pe_kind != EGT_NE_PE_SVD && d->pe_kind != EGT_NE_PE_EIG)
    EGT_FAIL(EGT_E_FLAGS, "node embed: pe_kind is EGT_NE_PE_NONE, _SVD or _EIG (got %d)", d->pe_kind);
  if (!(d->Dh == 16 || d->Dh == 32 || d->Dh == 48 || d->Dh == 64))
    EGT_FAIL(EGT_E_SHAPE, "node embed covers Dh in {16,32,48,64} (got %d)", d->Dh);
  if (d->nv < 0 || d->nv > NE_MAX_NV) EGT_FAIL(EGT_E_SHAPE, "node embed covers 0 <= nv <= %d virtual nodes (got %d)", NE_MAX_NV, d->nv);
  if (d->B < 1 || d->N < 1 || (long)d->B * ((long)d->nv + d->N) > 2147483647L / 64)
    EGT_FAIL(EGT_E_SHAPE, "node embed: B, N >= 1 and B*(nv+N)*64 inside 32-bit indexing (B=%d N=%d nv=%d)", d->B, d->N, d->nv);
  if (d->kind == EGT_NE_INT) {
    if (d->R < 1 || d->R > NE_MAX_R || d->F != 0)
      EGT_FAIL(EGT_E_SHAPE, "node embed, integer kind: 1 <= R <= %d table rows and F = 0 (got R=%d F=%d)", NE_MAX_R, d->R, d->F);
  } else if (d->F < 1 || d->F > NE_MAX_F || d->R != 0) {
    EGT_FAIL(EGT_E_SHAPE, "node embed, float kind: 1 <= F <= %d feature columns and R = 0 (got F=%d R=%d)", NE_MAX_F, d->F, d->R);
  }
  if (d->pe_kind == EGT_NE_PE_NONE) {
    if (d->T != 0 || d->sel != 0 || d->flags != 0 || d->sign_stride != 0)
      EGT_FAIL(EGT_E_SHAPE, "node embed without an encoding: T, sel, sign_stride and flags are 0 (got %d, %d, %d, 0x%x)", d->T, d->sel,
               d->sign_stride, (unsigned)d->flags);
  } else {
    if (d->sel < 1 || d->sel > NE_MAX_SEL || d->T < d->sel)
      EGT_FAIL(EGT_E_SHAPE, "node embed covers 1 <= sel <= %d of T >= sel stored features (got sel=%d T=%d)", NE_MAX_SEL, d->sel, d->T);
    if (!(d->flags & EGT_NE_TRANSFORM) && (d->pe_kind == EGT_NE_PE_SVD ? 2 * d->sel : d->sel) > d->Dh)
      EGT_FAIL(EGT_E_SHAPE, "node embed without EGT_NE_TRANSFORM: %s (got sel=%d Dh=%d)",
               d->pe_kind == EGT_NE_PE_SVD ? "2 sel <= Dh" : "sel <= Dh", d->sel, d->Dh);
    if ((d->flags & EGT_NE_SIGNS) ? (d->sign_stride != 0 && d->sign_stride < d->sel) : d->sign_stride != 0)
      EGT_FAIL(EGT_E_SHAPE, "node embed: sign_stride is 0 (= sel) or >= sel under EGT_NE_SIGNS, 0 without (got %d)", d->sign_stride);
  }
  return EGT_OK;
}
static NeGeo node_embed_geo(const egt_node_embed_desc* d) {
  const int sg = (d->flags & EGT_NE_SIGNS) ? 1 : 0;
  return {d->B, d->N, d->nv + d->N, d->Dh, d->nv, d->kind, d->R, d->F, d->pe_kind, d->T, d->sel, (d->flags & EGT_NE_TRANSFORM) ? 1 : 0, sg,
          sg ? (d->sign_stride ? d->sign_stride : d->sel) : 0, d->mask_value};
}
static NeBwdGeo node_embed_bwd_geo(const NeGeo& g) {
  NeBwdGeo b;
  b.JP = (g.pe != EGT_NE_PE_NONE && g.transform) ? (g.pe == EGT_NE_PE_SVD ? 2 * g.sel : g.sel) : 0;
  b.JX = b.JP + g.F + 1;
  b.PR = b.JX + g.R;
  const long total = (long)g.B * g.N;
  long per = NE_ROWS_PER_WG;
  if ((total + per - 1) / per > NE_MAX_WG) per = (total + NE_MAX_WG - 1) / NE_MAX_WG;
  b.rows_per_wg = (int)((per + NE_TILE - 1) / NE_TILE * NE_TILE);
  return b;
}
static int node_embed_nwg(const NeGeo& g, const NeBwdGeo& b) { return (int)(((long)g.B * g.N + b.rows_per_wg - 1) / b.rows_per_wg); }

// which pointers of a parameter / gradient struct the geometry uses
static int node_embed_params(const NeGeo& g, const egt_node_embed_params* p, const char* what, NeParams* out) {
  if (!p) EGT_FAIL(EGT_E_NULL, "node embed: %s is NULL", what);
  memcpy(out, p, sizeof(NeParams));
  const bool need[5] = {true, g.kind == EGT_NE_FLOAT, g.pe != EGT_NE_PE_NONE && g.transform != 0, g.pe != EGT_NE_PE_NONE && g.transform != 0,
                        g.nv > 0};
  static const char* names[5] = {"node_emb", "node_emb_bias", "pe_kernel", "pe_bias", "virtual_node_emb"};
  for (int k = 0; k < 5; ++k)
    if (need[k] && !out->p[k]) EGT_FAIL(EGT_E_NULL, "node embed: %s of %s is NULL", names[k], what);
  return EGT_OK;
}

extern "C" int egt_node_embed_supported(const egt_node_embed_desc* d) { return node_embed_check(d) == EGT_OK ? 1 : 0; }

// workspace (floats): the backward's partials [workgroups][PR][Dh]
extern "C" size_t egt_node_embed_workspace_bytes(const egt_node_embed_desc* d) {
  if (node_embed_check(d) != EGT_OK) return 0;
  const NeGeo g = node_embed_geo(d);
  const NeBwdGeo b = node_embed_bwd_geo(g);
  return sizeof(float) * (size_t)node_embed_nwg(g, b) * b.PR * g.Dh;
}

extern "C" int egt_node_embed_fwd(const egt_node_embed_desc* d, const egt_node_embed_params* params, const void* features,
                                  const float* pe, const float* signs, float* h_out, uint8_t* mask_out, void* stream) {
  int rc = node_embed_check(d);
  if (rc) return rc;
  const NeGeo g = node_embed_geo(d);
  NeParams P;
  if ((rc = node_embed_params(g, params, "params", &P))) return rc;
  if (!features || !h_out || !mask_out) EGT_FAIL(EGT_E_NULL, "node embed: features/h_out/mask_out is NULL");
  if (g.pe != EGT_NE_PE_NONE && !pe) EGT_FAIL(EGT_E_NULL, "node embed: pe is NULL with an encoding in the descriptor");
  if (g.has_signs && !signs) EGT_FAIL(EGT_E_NULL, "node embed: signs is NULL under EGT_NE_SIGNS");
  const long total = (long)g.B * g.NP;
  EGT_LAUNCH("k_node_embed_fwd", k_node_embed_fwd, dim3((unsigned)((total + NE_FWD_ROWS - 1) / NE_FWD_ROWS)), dim3(NE_NT), 0,
             (hipStream_t)stream, features, pe, signs, P, h_out, mask_out, g);
  EGT_HIP_LAUNCH_CHECK("egt_node_embed_fwd");
  return EGT_OK;
}

extern "C" int egt_node_embed_bwd(const egt_node_embed_desc* d, const void* features, const float* pe, const float* signs,
                                  const float* d_h, const egt_node_embed_params* grads, void* workspace, void* stream) {
  int rc = node_embed_check(d);
  if (rc) return rc;
  const NeGeo g = node_embed_geo(d);
  NeParams G;
  if ((rc = node_embed_params(g, grads, "grads", &G))) return rc;
  if (!features || !d_h || !workspace) EGT_FAIL(EGT_E_NULL, "node embed: features/d_h/workspace is NULL");
  if (g.pe != EGT_NE_PE_NONE && g.transform && !pe) EGT_FAIL(EGT_E_NULL, "node embed: pe is NULL with an encoding Dense in the descriptor");
  if (g.has_signs && g.transform && !signs) EGT_FAIL(EGT_E_NULL, "node embed: signs is NULL under EGT_NE_SIGNS");
  const NeBwdGeo b = node_embed_bwd_geo(g);
  const int nwg = node_embed_nwg(g, b);
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)workspace;
  EGT_LAUNCH("k_node_embed_bwd", k_node_embed_bwd, dim3((unsigned)nwg), dim3(NE_NT), 0, st, features, pe, signs, d_h, part, g, b);
  const int n = ((g.kind == EGT_NE_INT ? g.R : g.F + 1) + (b.JP ? b.JP + 1 : 0) + g.nv) * g.Dh;
  EGT_LAUNCH("k_node_embed_finish", k_node_embed_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)part, d_h, G,
             g, b, nwg);
  EGT_HIP_LAUNCH_CHECK("egt_node_embed_bwd");
  return EGT_OK;
}
