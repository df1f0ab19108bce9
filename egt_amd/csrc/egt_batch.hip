// egt_batch_* — padded training batches assembled on the device from a split's packed records.
//
// The host pipeline (egt_amd/data.py: GraphDataset._load_record + collate) builds the dense [B,N,N] matrices of a batch with
// one numpy scatter per record and ships ~23 MB per CIFAR10 batch over the bus.  Here the split's PACKED records live in HBM
// (edge lists, node rows, positional-encoding rows: under a tenth of the dense bytes) and one launch writes every tensor of the
// batch from the B record indices alone.
//
// Store layout (egt_amd.device_data.pack_split).  Record r has n = num_nodes[r] nodes and edge_off[r+1] - edge_off[r] edges.
// Its edges are STABLY sorted by source row: edge_dst / edge_feat hold the destination and the feature of each edge in that
// order, and row_off[node_off[r] + r + i] (i = 0..n) is the offset of row i's first edge inside the record, so duplicates
// of one (i,j) keep the order of the edge list.  node_rows / pe_rows / node targets are ragged rows at node_off[r].
//
// k_batch_assemble.  Workgroups [0, B * tiles) own `rows` consecutive rows of one batch graph, the B workgroups after them
// own the node-level and per-graph outputs of one graph each.  A matrix workgroup
//   1. fills its [rows, N] tile(s) in LDS: 0 (+1 on the diagonal for graph_matrix) inside n x n, the pad value outside;
//   2. one lane per row walks that row's edges IN ORDER and adds 1 (graph_matrix) / feat + inc (feature_matrix) in LDS --
//      the sequence of fp32 additions np.add.at performs for that cell;
//   3. subtracts `inc` from the inside cells of the feature tile (the "mark invalid" trick: non-edges end at -1);
//   4. stores the tile as ONE flat span of rows * N words: the rows of one graph are contiguous in the output.  The tile sits
//      in LDS at the span's own offset modulo 4 words, so dwords up to the first 16-byte boundary of the output, dwordx4
//      from there (aligned on both sides), dwords for the rest.
// A tile at or below row n is all padding: it is stored straight from registers and never touches the store.  Every output
// word is written exactly once; nothing is read back from HBM and there are no atomics, so the result does not depend on
// what the buffers held.  Node rows, PE rows and node targets are 4-byte words whatever their type: one flat
// copy-then-pad (span_copy_pad) moves them all.
// k_batch_assemble_at is the same text with the indices taken from a table at a device-resident cursor (egt_batch_assemble_at).
#include "egt_common.h"

namespace {
constexpr int BA_THREADS = 256;
constexpr int BA_MAX_N = 512;
constexpr int BA_MAX_ROWS = 32;        // rows of a tile (one walking lane each)
constexpr int BA_TILE_WORDS = 7680;    // rows * N <= this: two tiles and their alignment slack stay under 64 KB of LDS
constexpr int BA_MAX_WIDTH = 64;       // words of a node row / a PE row
constexpr int BA_WALK = 8;             // edges a walking lane loads before it applies them

struct BatchPlan { int rows, tiles, stride; size_t lds; };   // stride: LDS words from one tile to the next

struct BatchArgs {
  egt_batch_desc d;
  egt_batch_store s;
  egt_batch_out o;
  const int32_t* idx;
  int rows, tiles, stride;
};

__device__ __forceinline__ void store4(uint32_t* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  *reinterpret_cast<uint4*>(p) = make_uint4(a, b, c, d);
}

// dst[s0 .. s0 + len) = src[0 .. valid) followed by `pad`; dst is 16-byte aligned at word 0, s0 is any word offset
__device__ __forceinline__ void span_copy_pad(uint32_t* __restrict__ dst, int64_t s0, int len, const uint32_t* __restrict__ src,
                                              int valid, uint32_t pad, int tid) {
  int head = (int)((4 - (s0 & 3)) & 3);
  if (head > len) head = len;
  const int nv = (len - head) >> 2, tail0 = head + 4 * nv;
  uint32_t* const out = dst + s0;
  if (tid < head) out[tid] = tid < valid ? src[tid] : pad;
  for (int q = tid; q < nv; q += BA_THREADS) {
    const int t = head + 4 * q;
    uint32_t v[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = (t + c) < valid ? src[t + c] : pad;
    store4(out + t, v[0], v[1], v[2], v[3]);
  }
  if (tid < len - tail0) out[tail0 + tid] = (tail0 + tid) < valid ? src[tail0 + tid] : pad;
}

// the tile (at LDS word `sh`, the span's offset modulo 4) -> dst[s0 .. s0 + len)
__device__ __forceinline__ void span_store_lds(uint32_t* __restrict__ dst, int64_t s0, int len, const uint32_t* tile, int tid) {
  int head = (int)((4 - (s0 & 3)) & 3);
  if (head > len) head = len;
  const int nv = (len - head) >> 2, tail0 = head + 4 * nv;
  uint32_t* const out = dst + s0;
  if (tid < head) out[tid] = tile[tid];
  for (int q = tid; q < nv; q += BA_THREADS) {
    const int t = head + 4 * q;                                          // (sh + t) is a multiple of 4: tile + t is 16-byte aligned
    *reinterpret_cast<uint4*>(out + t) = *reinterpret_cast<const uint4*>(tile + t);
  }
  if (tid < len - tail0) out[tail0 + tid] = tile[tail0 + tid];
}

template <bool FEAT_F32>
__device__ __forceinline__ void matrix_tile(const BatchArgs& a, int b, int tile_i, int n, int64_t e0, int64_t rbase, uint32_t* lds) {
  const int N = a.d.N, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = tile_i * a.rows;
  const int nr = min(a.rows, N - r0);                 // rows of this tile
  if (nr <= 0) return;                                // (plan_batch leaves no empty tile for N <= BA_MAX_N)
  const int len = nr * N;
  const int64_t s0 = ((int64_t)b * N + r0) * N;
  const uint32_t gpad = __float_as_uint(a.d.matrix_pad);
  const uint32_t fpad = FEAT_F32 ? __float_as_uint(a.d.mask_f) : (uint32_t)a.d.mask_i;
  uint32_t* const gm = reinterpret_cast<uint32_t*>(a.o.graph_matrix);
  uint32_t* const fm = reinterpret_cast<uint32_t*>(a.o.feature_matrix);
  if (r0 >= n) {                                      // all padding: no LDS, no store access
    if (gm) span_copy_pad(gm, s0, len, nullptr, 0, gpad, tid);
    if (fm) span_copy_pad(fm, s0, len, nullptr, 0, fpad, tid);
    return;
  }
  const int sh = (int)(s0 & 3);
  float* const tg = reinterpret_cast<float*>(lds) + sh;
  uint32_t* const tfu = lds + (gm ? a.stride : 0) + sh;  // (the stride is a multiple of 4 words: both tiles share the 16-byte phase)
  const float inc = (a.d.flags & EGT_BATCH_MARK_INVALID) ? 1.f : 0.f;
  const int inci = (a.d.flags & EGT_BATCH_MARK_INVALID) ? 1 : 0;
  // 1. initialise: a wave per row, lanes over the columns
  for (int r = wave; r < nr; r += BA_THREADS / 64) {
    const int gi = r0 + r;
    for (int c = lane; c < N; c += 64) {
      const bool inside = gi < n && c < n;
      if (gm) tg[r * N + c] = inside ? (c == gi ? 1.f : 0.f) : a.d.matrix_pad;
      if (fm) tfu[r * N + c] = inside ? 0u : fpad;
    }
  }
  __syncthreads();
  // 2. one lane per row (rows dealt round-robin to the four waves) walks the row's edges in edge-list order
  {
    const int r = lane * (BA_THREADS / 64) + wave;
    const int gi = r0 + r;
    if (r < nr && gi < n) {
      const int k0 = a.s.row_off[rbase + gi], k1 = a.s.row_off[rbase + gi + 1];
      const uint32_t* const ef = reinterpret_cast<const uint32_t*>(a.s.edge_feat);
      for (int k = k0; k < k1; k += BA_WALK) {        // BA_WALK edges' loads in flight, then their updates in list order
        int j[BA_WALK];
        uint32_t f[BA_WALK];
#pragma unroll
        for (int c = 0; c < BA_WALK; ++c) {
          const bool in = k + c < k1;
          j[c] = in ? a.s.edge_dst[e0 + k + c] : -1;
          f[c] = in && fm ? ef[e0 + k + c] : 0u;
        }
#pragma unroll
        for (int c = 0; c < BA_WALK; ++c) {
          if ((unsigned)j[c] >= (unsigned)n) continue; // (past the row's end; pack_split refuses a store with a node outside the graph)
          const int t = r * N + j[c];
          if (gm) tg[t] += 1.f;
          if (fm) {
            if (FEAT_F32) {
              float* const tf = reinterpret_cast<float*>(tfu);
              tf[t] = tf[t] + (__uint_as_float(f[c]) + inc);
            } else {
              tfu[t] += f[c] + (uint32_t)inci;
            }
          }
        }
      }
    }
  }
  __syncthreads();
  // 3. the decrement of the inside cells
  if (fm && inci) {
    for (int r = wave; r < nr && r0 + r < n; r += BA_THREADS / 64)
      for (int c = lane; c < n; c += 64) {
        if (FEAT_F32) {
          float* const tf = reinterpret_cast<float*>(tfu);
          tf[r * N + c] = tf[r * N + c] - 1.f;
        } else {
          tfu[r * N + c] -= 1u;
        }
      }
    __syncthreads();
  }
  // 4. the tile as one flat span
  if (gm) span_store_lds(gm, s0, len, reinterpret_cast<const uint32_t*>(tg), tid);
  if (fm) span_store_lds(fm, s0, len, tfu, tid);
}

// The kernel's text, instantiated twice below.  k_batch_assemble takes the B indices of the batch; k_batch_assemble_at takes the
// index table and reads the batch's first entry `*cursor` when it RUNS: a replayed hipGraph walks the table as egt_seed_advance
// moves the cursor behind it.  Neither the cursor nor the table is written.  (A macro and not an inlined function: the plain
// kernel's machine code stays what it was, instruction for instruction -- profiles/resident_step_asm.txt.)
#define BA_KERNEL(NAME, PARAMS, IDX) \
__global__ __launch_bounds__(BA_THREADS) void NAME PARAMS {                                                               \
  extern __shared__ __align__(16) uint32_t ba_lds[];                                                                      \
  const int B = a.d.B, N = a.d.N, tid = threadIdx.x;                                                                      \
  const int mat_wgs = B * a.tiles;                                                                                        \
  const bool is_mat = (int)blockIdx.x < mat_wgs;                                                                          \
  const int b = is_mat ? (int)blockIdx.x / a.tiles : (int)blockIdx.x - mat_wgs;                                           \
  const int r = (IDX)[b];                                                                                                 \
  const bool ok = (unsigned)r < (unsigned)a.d.records;             /* an index outside the split writes an empty graph */ \
  const int n = ok ? min(max(a.s.num_nodes[r], 0), N) : 0;                                                                \
  const int64_t nd0 = ok ? a.s.node_off[r] : 0;                                                                           \
  if (is_mat) {                                                                                                           \
    const int64_t e0 = ok && a.s.edge_off ? a.s.edge_off[r] : 0;                                                          \
    if (a.d.edge_kind == EGT_BATCH_F32) matrix_tile<true>(a, b, (int)blockIdx.x % a.tiles, n, e0, nd0 + r, ba_lds);       \
    else matrix_tile<false>(a, b, (int)blockIdx.x % a.tiles, n, e0, nd0 + r, ba_lds);                                     \
    return;                                                                                                               \
  }                                                                                                                       \
  /* node-level and per-graph outputs of graph b */                                                                       \
  if (a.o.node_features) {                                                                                                \
    const int W = a.d.node_width;                                                                                         \
    const uint32_t pad = a.d.node_kind == EGT_BATCH_F32 ? __float_as_uint(a.d.mask_f) : (uint32_t)a.d.mask_i;             \
    span_copy_pad(reinterpret_cast<uint32_t*>(a.o.node_features), (int64_t)b * N * W, N * W,                              \
                  reinterpret_cast<const uint32_t*>(a.s.node_rows) + nd0 * W, n * W, pad, tid);                           \
  }                                                                                                                       \
  if (a.o.pe) {                                                                                                           \
    const int W = a.d.pe_kind == EGT_BATCH_PE_SVD ? 2 * a.d.pe_features : a.d.pe_features;                                \
    span_copy_pad(reinterpret_cast<uint32_t*>(a.o.pe), (int64_t)b * N * W, N * W,                                         \
                  reinterpret_cast<const uint32_t*>(a.s.pe_rows) + nd0 * W, n * W, 0u, tid);                              \
  }                                                                                                                       \
  if (a.o.target) {                                                                                                       \
    const uint32_t* const tg = reinterpret_cast<const uint32_t*>(a.s.targets);                                            \
    if (a.d.target_kind == EGT_BATCH_TGT_NODE_I32)                                                                        \
      span_copy_pad(reinterpret_cast<uint32_t*>(a.o.target), (int64_t)b * N, N, tg + nd0, n, 0u, tid);                    \
    else if (tid == 0)                                                                                                    \
      reinterpret_cast<uint32_t*>(a.o.target)[b] = ok ? tg[r] : 0u;                                                       \
  }                                                                                                                       \
  if (a.o.num_nodes && tid == 0) a.o.num_nodes[b] = ok ? a.s.num_nodes[r] : 0;                                            \
}

BA_KERNEL(k_batch_assemble, (BatchArgs a), a.idx)
BA_KERNEL(k_batch_assemble_at, (BatchArgs a, const uint64_t* cursor), a.idx + *cursor)
#undef BA_KERNEL

// one text behind egt_batch_supported and egt_batch_assemble
int batch_desc_check(const egt_batch_desc* d, bool report) {
  if (!d) EGT_BAD(EGT_E_NULL, "desc is NULL");
  if (d->B < 1) EGT_BAD(EGT_E_SHAPE, "egt_batch_desc.B must be >= 1 (got %d)", d->B);
  if (d->N < 1 || d->N > BA_MAX_N) EGT_BAD(EGT_E_SHAPE, "egt_batch_desc.N %d outside 1..%d", d->N, BA_MAX_N);
  if (d->records < 1) EGT_BAD(EGT_E_SHAPE, "egt_batch_desc.records must be >= 1 (got %d)", d->records);
  if ((int64_t)d->B * d->N * d->N >= (int64_t)1 << 31) EGT_BAD(EGT_E_SHAPE, "B N N must stay below 2^31");
  if (d->node_kind != EGT_BATCH_I32 && d->node_kind != EGT_BATCH_F32) EGT_BAD(EGT_E_DTYPE, "node_kind %d: EGT_BATCH_I32 or EGT_BATCH_F32", d->node_kind);
  if (d->node_width < 1 || d->node_width > BA_MAX_WIDTH || (d->node_kind == EGT_BATCH_I32 && d->node_width != 1))
    EGT_BAD(EGT_E_SHAPE, "node_width %d: 1 for EGT_BATCH_I32, 1..%d for EGT_BATCH_F32", d->node_width, BA_MAX_WIDTH);
  if (d->edge_kind != EGT_BATCH_NONE && d->edge_kind != EGT_BATCH_I32 && d->edge_kind != EGT_BATCH_F32)
    EGT_BAD(EGT_E_DTYPE, "edge_kind %d: EGT_BATCH_NONE, EGT_BATCH_I32 or EGT_BATCH_F32", d->edge_kind);
  if (d->edge_width != (d->edge_kind == EGT_BATCH_NONE ? 0 : 1)) EGT_BAD(EGT_E_SHAPE, "edge_width %d: one value per edge (0 without edge features)", d->edge_width);
  if (d->pe_kind != EGT_BATCH_PE_NONE && d->pe_kind != EGT_BATCH_PE_SVD && d->pe_kind != EGT_BATCH_PE_EIGEN)
    EGT_BAD(EGT_E_FLAGS, "pe_kind %d: EGT_BATCH_PE_NONE, _SVD or _EIGEN", d->pe_kind);
  if (d->pe_kind == EGT_BATCH_PE_NONE ? d->pe_features != 0
                                       : (d->pe_features < 1 || d->pe_features * (d->pe_kind == EGT_BATCH_PE_SVD ? 2 : 1) > BA_MAX_WIDTH))
    EGT_BAD(EGT_E_SHAPE, "pe_features %d: 0 without a positional encoding, else a row of at most %d floats", d->pe_features, BA_MAX_WIDTH);
  if (d->target_kind != EGT_BATCH_TGT_GRAPH_F32 && d->target_kind != EGT_BATCH_TGT_GRAPH_I32 && d->target_kind != EGT_BATCH_TGT_NODE_I32)
    EGT_BAD(EGT_E_FLAGS, "target_kind %d: EGT_BATCH_TGT_GRAPH_F32, _GRAPH_I32 or _NODE_I32", d->target_kind);
  if (d->flags & ~EGT_BATCH_MARK_INVALID) EGT_BAD(EGT_E_FLAGS, "egt_batch_desc.flags 0x%x has unknown bits", d->flags);
  if (d->reserved[0] != 0 || d->reserved[1] != 0) EGT_BAD(EGT_E_FLAGS, "egt_batch_desc.reserved must be 0");
  return EGT_OK;
}

// rows per tile: as many as LDS and the lane-per-row walk allow, then balanced over the tiles of a graph
BatchPlan plan_batch(const egt_batch_desc* d, int fields) {
  BatchPlan p;
  const int cap = min(BA_MAX_ROWS, BA_TILE_WORDS / d->N);
  p.tiles = (d->N + cap - 1) / cap;
  p.rows = (d->N + p.tiles - 1) / p.tiles;
  p.stride = (p.rows * d->N + 3) / 4 * 4 + 4;        // the tile, shifted by up to 3 words
  p.lds = (size_t)fields * p.stride * sizeof(uint32_t);
  return p;
}
}  // namespace

extern "C" int egt_batch_supported(const egt_batch_desc* desc) { return batch_desc_check(desc, false) == EGT_OK ? 1 : 0; }

namespace {
// egt_batch_assemble (cursor == nullptr, idx = the B indices) and egt_batch_assemble_at (idx = the table)
int batch_assemble_launch(const egt_batch_desc* desc, const egt_batch_store* store, const int32_t* idx, const uint64_t* cursor, bool at,
                          const egt_batch_out* out, void* stream) {
  const int rc = batch_desc_check(desc, true);
  if (rc != EGT_OK) return rc;
  if (!store) EGT_FAIL(EGT_E_NULL, "store is NULL");
  if (!idx) EGT_FAIL(EGT_E_NULL, at ? "idx_table is NULL" : "idx is NULL");
  if (at && !cursor) EGT_FAIL(EGT_E_NULL, "cursor is NULL");
  if (at && (reinterpret_cast<uintptr_t>(cursor) & 7)) EGT_FAIL(EGT_E_SHAPE, "cursor must be 8-byte aligned");
  if (!out) EGT_FAIL(EGT_E_NULL, "out is NULL");
  if (!store->num_nodes || !store->node_off) EGT_FAIL(EGT_E_NULL, "store.num_nodes / store.node_off is NULL");
  const bool mats = out->graph_matrix || out->feature_matrix;
  if (out->feature_matrix && desc->edge_kind == EGT_BATCH_NONE) EGT_FAIL(EGT_E_FLAGS, "feature_matrix asked of a store without edge features");
  if (mats && (!store->edge_off || !store->edge_dst || !store->row_off)) EGT_FAIL(EGT_E_NULL, "store.edge_off / edge_dst / row_off is NULL");
  if (out->feature_matrix && !store->edge_feat) EGT_FAIL(EGT_E_NULL, "store.edge_feat is NULL");
  if (out->node_features && !store->node_rows) EGT_FAIL(EGT_E_NULL, "store.node_rows is NULL");
  if (out->pe && desc->pe_kind == EGT_BATCH_PE_NONE) EGT_FAIL(EGT_E_FLAGS, "pe asked of a store without a positional encoding");
  if (out->pe && !store->pe_rows) EGT_FAIL(EGT_E_NULL, "store.pe_rows is NULL");
  if (out->target && !store->targets) EGT_FAIL(EGT_E_NULL, "store.targets is NULL");
  if ((reinterpret_cast<uintptr_t>(out->graph_matrix) | reinterpret_cast<uintptr_t>(out->feature_matrix) |
       reinterpret_cast<uintptr_t>(out->node_features) | reinterpret_cast<uintptr_t>(out->pe) | reinterpret_cast<uintptr_t>(out->target)) & 15)
    EGT_FAIL(EGT_E_SHAPE, "the output tensors must be 16-byte aligned");
  const int fields = (out->graph_matrix ? 1 : 0) + (out->feature_matrix ? 1 : 0);
  const BatchPlan p = plan_batch(desc, fields);
  BatchArgs a;
  a.d = *desc; a.s = *store; a.o = *out; a.idx = idx;
  a.rows = p.rows; a.tiles = mats ? p.tiles : 0; a.stride = p.stride;
  const dim3 grid((unsigned)(desc->B * a.tiles + desc->B)), block(BA_THREADS);
  if (at) {
    EGT_LAUNCH("k_batch_assemble_at", k_batch_assemble_at, grid, block, mats ? p.lds : 0, (hipStream_t)stream, a, cursor);
    EGT_HIP_LAUNCH_CHECK("egt_batch_assemble_at");
  } else {
    EGT_LAUNCH("k_batch_assemble", k_batch_assemble, grid, block, mats ? p.lds : 0, (hipStream_t)stream, a);
    EGT_HIP_LAUNCH_CHECK("egt_batch_assemble");
  }
  return EGT_OK;
}
}  // namespace

extern "C" int egt_batch_assemble(const egt_batch_desc* desc, const egt_batch_store* store, const int32_t* idx,
                                  const egt_batch_out* out, void* stream) {
  return batch_assemble_launch(desc, store, idx, nullptr, false, out, stream);
}

extern "C" int egt_batch_assemble_at(const egt_batch_desc* desc, const egt_batch_store* store, const int32_t* idx_table,
                                     const uint64_t* cursor, const egt_batch_out* out, void* stream) {
  return batch_assemble_launch(desc, store, idx_table, cursor, true, out, stream);
}
