// Segment / elementwise / reduction kernels (gfx950):
//   K9+K10  pattern-weighted global-add-pool (fwd: wave-per-graph segment sum
//           over the batch-ptr — deterministic, no atomics; bwd: gather)
//   K1+K11  embedding gathers fused with concat (+ scatter-add backward)
//   K7+K8   BatchNorm1d (+fused ReLU) forward/backward
//   K12/K13 quantile loss + eval-metric reductions
//   K14     Adam step (flat master buffers — one kernel for the whole model)
#include "common.h"
#include "launchers.h"
#include <cstdlib>
#include <type_traits>

// ---------------------------------------------------------------------------
// pattern pool: out[b] = sum_{i in graph b} x[i] * p[i] / n[i]
// ---------------------------------------------------------------------------

#define WAVES_PER_BLOCK 4

// two-level: P sub-waves per graph each sum a strided node interleave into
// partial[g*P+sub], then one wave per graph folds the P partials in order
// (deterministic, no atomics; single waves per graph would leave the chip
// ~64/256 CUs busy at trace-scale batches).
template <int VPT, typename TX = float>
__global__ void seg_pool_p1_kernel(const TX* __restrict__ x,
                                   const float* __restrict__ probs,
                                   const float* __restrict__ nn,
                                   const int* __restrict__ batch_ptr,
                                   float* __restrict__ partial, int b, int P,
                                   int h) {
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int w = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (w >= b * P) return;
  const int g = w / P;
  const int sub = w % P;
  float acc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) acc[j] = 0.f;
  for (int i = batch_ptr[g] + sub; i < batch_ptr[g + 1]; i += P) {
    const float wt = probs[i] / nn[i];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = lane + j * PERTGNN_WAVE;
      if (c < h) acc[j] += (float)x[(long)i * h + c] * wt;
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = lane + j * PERTGNN_WAVE;
    if (c < h) partial[(long)w * h + c] = acc[j];
  }
}

template <int VPT>
__global__ void seg_pool_p2_kernel(const float* __restrict__ partial,
                                   float* __restrict__ out, int b, int P,
                                   int h) {
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int g = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (g >= b) return;
  float acc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) acc[j] = 0.f;
  for (int sub = 0; sub < P; ++sub) {
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = lane + j * PERTGNN_WAVE;
      if (c < h) acc[j] += partial[((long)g * P + sub) * h + c];
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = lane + j * PERTGNN_WAVE;
    if (c < h) out[(long)g * h + c] = acc[j];
  }
}

template <typename TD = float>
__global__ void seg_pool_bwd_kernel(const float* __restrict__ gout,
                                    const float* __restrict__ probs,
                                    const float* __restrict__ nn,
                                    const long* __restrict__ batch,
                                    TD* __restrict__ dx, long n, int h) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const long numel = n * h;
  for (long t = i; t < numel; t += stride) {
    const long row = t / h;
    const int c = (int)(t - row * h);
    dx[t] = (TD)pool_bwd_dx(gout[batch[row] * h + c], probs[row], nn[row]);
  }
}

void launch_seg_pool_fwd(const float* x, const float* probs, const float* nn,
                         const int* batch_ptr, float* partial, float* out,
                         int b, int P, int h, hipStream_t stream) {
  if (b == 0) return;
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const int vpt = (h + PERTGNN_WAVE - 1) / PERTGNN_WAVE;
  switch (vpt) {
#define CASE(V)                                                                \
  case V:                                                                      \
    seg_pool_p1_kernel<V>                                                      \
        <<<dim3(ceil_div((long)b * P, WAVES_PER_BLOCK)), block, 0, stream>>>(  \
            x, probs, nn, batch_ptr, partial, b, P, h);                        \
    seg_pool_p2_kernel<V>                                                      \
        <<<dim3(ceil_div(b, WAVES_PER_BLOCK)), block, 0, stream>>>(            \
            partial, out, b, P, h);                                            \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: pertgnn_shape_fail("segops launcher", "vpt", vpt);
  }
}

void launch_seg_pool_bwd(const float* gout, const float* probs,
                         const float* nn, const long* batch, float* dx, long n,
                         int h, hipStream_t stream) {
  if (n == 0) return;
  const long numel = n * h;
  const int tpb = 256;
  const int blocks = (int)min((numel + tpb - 1) / tpb, (long)4096);
  seg_pool_bwd_kernel<<<dim3(blocks), dim3(tpb), 0, stream>>>(gout, probs, nn,
                                                              batch, dx, n, h);
}

// act16 variants: x16 in (bf16 last-layer activations), bf16 dx out
void launch_seg_pool_fwd16(const void* x, const float* probs, const float* nn,
                           const int* batch_ptr, float* partial, float* out,
                           int b, int P, int h, hipStream_t stream) {
  if (b == 0) return;
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const int vpt = (h + PERTGNN_WAVE - 1) / PERTGNN_WAVE;
  switch (vpt) {
#define CASE(V)                                                                \
  case V:                                                                      \
    seg_pool_p1_kernel<V, __bf16>                                              \
        <<<dim3(ceil_div((long)b * P, WAVES_PER_BLOCK)), block, 0, stream>>>(  \
            (const __bf16*)x, probs, nn, batch_ptr, partial, b, P, h);         \
    seg_pool_p2_kernel<V>                                                      \
        <<<dim3(ceil_div(b, WAVES_PER_BLOCK)), block, 0, stream>>>(            \
            partial, out, b, P, h);                                            \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: pertgnn_shape_fail("segops launcher", "vpt", vpt);
  }
}

void launch_seg_pool_bwd16(const float* gout, const float* probs,
                           const float* nn, const long* batch, void* dx,
                           long n, int h, hipStream_t stream) {
  if (n == 0) return;
  const long numel = n * h;
  const int tpb = 256;
  const int blocks = (int)min((numel + tpb - 1) / tpb, (long)4096);
  seg_pool_bwd_kernel<<<dim3(blocks), dim3(tpb), 0, stream>>>(
      gout, probs, nn, batch, (__bf16*)dx, n, h);
}

// ---------------------------------------------------------------------------
// embedding gathers fused with concat
// ---------------------------------------------------------------------------

template <typename TY = float>
__global__ void embed_node_fwd_kernel(const float* __restrict__ x_raw,
                                      const long* __restrict__ idx,
                                      const float* __restrict__ table,
                                      TY* __restrict__ out, long n, int f,
                                      int h) {
  const int w = f + h;
  const long numel = n * w;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = i0; t < numel; t += stride) {
    const long row = t / w;
    const int c = (int)(t - row * w);
    out[t] = (TY)((c < f) ? x_raw[row * f + c]
                          : table[idx[row] * h + (c - f)]);
  }
}

// embed_node_fwd with the row padded to pad_to >= f + h columns (+0 past
// f + h): the layer-1 GEMM operand at its staging width, written once.
// LPR lanes share a row, so the row index and idx[row] are uniform over the
// sub-wave and nothing is divided per element.  EPC > 1: each lane builds
// EPC consecutive columns (16 B) in registers and stores them whole; the
// launcher guarantees pad_to % EPC == 0, so every row starts 16-B aligned.
// Table rows are only 4-B aligned relative to a chunk (f is arbitrary), so
// they are read by dword.  EPC == 1 is the scalar path for any other pad_to.
template <typename TY, int EPC, int LPR>
__global__ void embed_node_pad_kernel(const float* __restrict__ x_raw,
                                      const long* __restrict__ idx,
                                      const float* __restrict__ table,
                                      TY* __restrict__ out, long n, int f,
                                      int h, int pad_to) {
  typedef __attribute__((ext_vector_type(EPC))) TY chunk_t;
  constexpr int RPW = PERTGNN_WAVE / LPR;
  const int lane0 = threadIdx.x % PERTGNN_WAVE;
  const int lane = lane0 % LPR;
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) / PERTGNN_WAVE;
  const long waves = (long)gridDim.x * blockDim.x / PERTGNN_WAVE;
  const int w = f + h;
  for (long row = wave * RPW + lane0 / LPR; row < n; row += waves * RPW) {
    const float* xr = x_raw + row * f;
    const float* tr = table + idx[row] * h;
    TY* orow = out + row * pad_to;
    for (int c0 = lane * EPC; c0 < pad_to; c0 += LPR * EPC) {
      float v[EPC];
      if (c0 >= f && c0 + EPC <= w) {
#pragma unroll
        for (int u = 0; u < EPC; ++u) v[u] = tr[c0 - f + u];
      } else {
        // the raw/table seam or the table/pad seam falls inside this chunk
#pragma unroll
        for (int u = 0; u < EPC; ++u) {
          const int c = c0 + u;
          v[u] = (c < f) ? xr[c] : (c < w) ? tr[c - f] : 0.f;
        }
      }
      if constexpr (EPC == 1) {
        orow[c0] = (TY)v[0];
      } else {
        chunk_t o;
#pragma unroll
        for (int u = 0; u < EPC; ++u) o[u] = (TY)v[u];
        *reinterpret_cast<chunk_t*>(orow + c0) = o;
      }
    }
  }
}

__global__ void embed_edge_fwd_kernel(const long* __restrict__ attr,
                                      const float* __restrict__ ifc,
                                      const float* __restrict__ rpc,
                                      float* __restrict__ out, long e, int h,
                                      int astride) {
  const int w = 2 * h;
  const long numel = e * w;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = i0; t < numel; t += stride) {
    const long row = t / w;
    const int c = (int)(t - row * w);
    out[t] = (c < h) ? ifc[attr[row * astride] * h + c]
                     : rpc[attr[row * astride + 1] * h + (c - h)];
  }
}

// Deterministic grouped embedding backward: rows of g pre-grouped by table
// index (order/ptr built once per backward from a sort).  Low-cardinality
// tables (rpctype has ~5 rows over 5e4 edges) would serialize a whole segment
// on one wave, so the reduction is TWO-PHASE: P sub-waves per table row each
// sum a strided interleave of the segment (phase 1, deterministic), then one
// wave per row folds the P partials in fixed order (phase 2).  No atomics.
template <int VPT>
__global__ void embed_grouped_p1_kernel(
    const float* __restrict__ g, const int* __restrict__ order,
    const int* __restrict__ ptr, float* __restrict__ partial, int rows, int P,
    int h, int gstride, int col_off) {
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int w = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (w >= rows * P) return;
  const int row = w / P;
  const int sub = w % P;
  float acc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) acc[j] = 0.f;
  for (int p = ptr[row] + sub; p < ptr[row + 1]; p += P) {
    const long r = order[p];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = lane + j * PERTGNN_WAVE;
      if (c < h) acc[j] += g[r * gstride + col_off + c];
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = lane + j * PERTGNN_WAVE;
    if (c < h) partial[(long)w * h + c] = acc[j];
  }
}

template <int VPT>
__global__ void embed_grouped_p2_kernel(const float* __restrict__ partial,
                                        float* __restrict__ dtable, int rows,
                                        int P, int h) {
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int row = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (row >= rows) return;
  float acc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) acc[j] = 0.f;
  for (int sub = 0; sub < P; ++sub) {
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = lane + j * PERTGNN_WAVE;
      if (c < h) acc[j] += partial[((long)row * P + sub) * h + c];
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = lane + j * PERTGNN_WAVE;
    if (c < h) dtable[(long)row * h + c] = acc[j];
  }
}

// order==nullptr reads g rows directly (r = p): that is how the SECOND
// reduction level folds the level-1 partials — same balanced assignment,
// with ptr = level-1 wave_start (each row's partials are contiguous).
// VEC: contiguous lane*VPT column mapping with packed 8-B (bf16) / 16-B
// (fp32) row loads — the strided lane+j*64 mapping issues VPT scalar loads
// per gathered row, which dominates this latency-bound kernel.  Requires
// h == VPT*64, VPT%4==0, and 4-element-aligned rows (gstride%4, col_off%4).
// The column mapping is internal: p1, the level-2 fold and p2 all use the
// same c_of(j), so dtable comes out identical either way.
typedef __attribute__((ext_vector_type(4))) float segf4;
typedef __attribute__((ext_vector_type(4))) __bf16 segb4;

template <int VPT, typename TG = float, bool VEC = false>
__global__ void embed_grouped_bal_p1_kernel(
    const TG* __restrict__ g, const int* __restrict__ order,
    const int* __restrict__ ptr, const int* __restrict__ row_map,
    const int* __restrict__ wave_start, float* __restrict__ partial,
    int n_waves, int h, int gstride, int col_off) {
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int w = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (w >= n_waves) return;
  const int row = row_map[w];
  const int w0 = wave_start[row];
  const int P = wave_start[row + 1] - w0;
  const int sub = w - w0;
  float acc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) acc[j] = 0.f;
  for (int p = ptr[row] + sub; p < ptr[row + 1]; p += P) {
    const long r = order ? order[p] : p;
    const TG* src = &g[(long)r * gstride + col_off];
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < VPT; q += 4) {
        if constexpr (sizeof(TG) == 2) {
          const segb4 v = *reinterpret_cast<const segb4*>(
              (const __bf16*)src + lane * VPT + q);
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[q + u] += (float)v[u];
        } else {
          const segf4 v = *reinterpret_cast<const segf4*>(
              (const float*)src + lane * VPT + q);
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[q + u] += v[u];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const int c = lane + j * PERTGNN_WAVE;
        if (c < h) acc[j] += (float)src[c];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = VEC ? lane * VPT + j : lane + j * PERTGNN_WAVE;
    if (c < h) partial[(long)w * h + c] = acc[j];
  }
}

template <int VPT, bool VEC = false>
__global__ void embed_grouped_bal_p2_kernel(
    const float* __restrict__ partial, const int* __restrict__ wave_start,
    float* __restrict__ dtable, int rows, int h) {
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int row = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (row >= rows) return;
  float acc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) acc[j] = 0.f;
  for (int s = wave_start[row]; s < wave_start[row + 1]; ++s) {
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < VPT; q += 4) {
        const segf4 v = *reinterpret_cast<const segf4*>(
            &partial[(long)s * h + lane * VPT + q]);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[q + u] += v[u];
      }
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const int c = lane + j * PERTGNN_WAVE;
        if (c < h) acc[j] += partial[(long)s * h + c];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = VEC ? lane * VPT + j : lane + j * PERTGNN_WAVE;
    if (c < h) dtable[(long)row * h + c] = acc[j];
  }
}

// Two-level balanced reduction: level 1 over the grouped g rows, optional
// level 2 over the level-1 partials (needed when one group's partial count
// itself is large — the interface-0 mega-group), final fold per row.
void launch_embed_grouped_scatter_bal(
    const void* g, int g16, const int* order, const int* ptr,
    const int* row_map, const int* wave_start, const int* row_map2,
    const int* wave_start2, float* partial, float* partial2, float* dtable,
    int n_waves, int n_waves2, int rows, int h, int gstride, int col_off,
    hipStream_t s) {
  if (rows == 0) return;
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const int vpt = (h + PERTGNN_WAVE - 1) / PERTGNN_WAVE;
  // packed-load column mapping when the whole row divides evenly and the
  // g rows are 4-element aligned (the hot de/entry cases; the embed-node
  // grad with col_off=9 keeps the strided scalar path)
  const bool vec = (h == vpt * PERTGNN_WAVE) && (vpt % 4 == 0) &&
                   (gstride % 4 == 0) && (col_off % 4 == 0);
  switch (vpt) {
#define CASE(V) case V: { const int grid1 = ceil_div(n_waves, WAVES_PER_BLOCK); if (vec) { if (g16) { embed_grouped_bal_p1_kernel<V, __bf16, true><<<dim3(grid1), block, 0, s>>>((const __bf16*)g, order, ptr, row_map, wave_start, partial, n_waves, h, gstride, col_off); } else { embed_grouped_bal_p1_kernel<V, float, true><<<dim3(grid1), block, 0, s>>>((const float*)g, order, ptr, row_map, wave_start, partial, n_waves, h, gstride, col_off); } if (n_waves2 > 0) { embed_grouped_bal_p1_kernel<V, float, true><<<dim3(ceil_div(n_waves2, WAVES_PER_BLOCK)), block, 0, s>>>(partial, nullptr, wave_start, row_map2, wave_start2, partial2, n_waves2, h, h, 0); embed_grouped_bal_p2_kernel<V, true><<<dim3(ceil_div(rows, WAVES_PER_BLOCK)), block, 0, s>>>(partial2, wave_start2, dtable, rows, h); } else { embed_grouped_bal_p2_kernel<V, true><<<dim3(ceil_div(rows, WAVES_PER_BLOCK)), block, 0, s>>>(partial, wave_start, dtable, rows, h); } } else { if (g16) { embed_grouped_bal_p1_kernel<V, __bf16><<<dim3(grid1), block, 0, s>>>((const __bf16*)g, order, ptr, row_map, wave_start, partial, n_waves, h, gstride, col_off); } else { embed_grouped_bal_p1_kernel<V, float><<<dim3(grid1), block, 0, s>>>((const float*)g, order, ptr, row_map, wave_start, partial, n_waves, h, gstride, col_off); } if (n_waves2 > 0) { embed_grouped_bal_p1_kernel<V, float><<<dim3(ceil_div(n_waves2, WAVES_PER_BLOCK)), block, 0, s>>>(partial, nullptr, wave_start, row_map2, wave_start2, partial2, n_waves2, h, h, 0); embed_grouped_bal_p2_kernel<V><<<dim3(ceil_div(rows, WAVES_PER_BLOCK)), block, 0, s>>>(partial2, wave_start2, dtable, rows, h); } else { embed_grouped_bal_p2_kernel<V><<<dim3(ceil_div(rows, WAVES_PER_BLOCK)), block, 0, s>>>(partial, wave_start, dtable, rows, h); } } } break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: pertgnn_shape_fail("segops launcher", "vpt", vpt);
  }
}

void launch_embed_grouped_scatter(const float* g, const int* order,
                                  const int* ptr, float* partial,
                                  float* dtable, long num_src, int rows, int P,
                                  int h, int gstride, int col_off,
                                  hipStream_t s) {
  if (rows == 0) return;
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const int vpt = (h + PERTGNN_WAVE - 1) / PERTGNN_WAVE;
  switch (vpt) {
#define CASE(V)                                                                \
  case V:                                                                      \
    embed_grouped_p1_kernel<V>                                                 \
        <<<dim3(ceil_div((long)rows * P, WAVES_PER_BLOCK)), block, 0, s>>>(    \
            g, order, ptr, partial, rows, P, h, gstride, col_off);             \
    embed_grouped_p2_kernel<V>                                                 \
        <<<dim3(ceil_div(rows, WAVES_PER_BLOCK)), block, 0, s>>>(              \
            partial, dtable, rows, P, h);                                      \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: pertgnn_shape_fail("segops launcher", "vpt", vpt);
  }
}

// ---------------------------------------------------------------------------
// list sums: out[w, :] = sum over p in [lptr[w], lptr[w+1]) of src[idx[p], :]
// ---------------------------------------------------------------------------
// One wave per list, fp32 accumulation in list order (bitwise reproducible:
// no atomics, no memset — an empty list stores a zero row).  Contiguous
// lane*VPT column mapping with packed loads (h == VPT*64).  U rows are in
// flight per wave: the wave index is made wave-uniform, so lptr and the U
// idx entries are scalar loads issued ahead of the U row loads, and the
// index-then-row dependency is paid once per U rows.  A list's last (< U)
// rows take one more round that re-reads the last row for the unused slots
// and adds nothing for them, so short lists keep their loads in flight too.
// The edge-table gradient runs this three times (edge_table_grad in
// bindings.cpp): level-1 chunks over de, level-2 groups over the partials,
// one list per table row.
template <int VPT, typename T>
__device__ __forceinline__ void rows_sum_load(const T* __restrict__ row,
                                              int lane, float (&v)[VPT]) {
  if constexpr (sizeof(T) == 2) {
#pragma unroll
    for (int q = 0; q < VPT; q += 4) {
      const segb4 x = *reinterpret_cast<const segb4*>(
          (const __bf16*)row + lane * VPT + q);
#pragma unroll
      for (int u = 0; u < 4; ++u) v[q + u] = (float)x[u];
    }
  } else {
#pragma unroll
    for (int q = 0; q < VPT; q += 4) {
      const segf4 x = *reinterpret_cast<const segf4*>(
          (const float*)row + lane * VPT + q);
#pragma unroll
      for (int u = 0; u < 4; ++u) v[q + u] = x[u];
    }
  }
}

// The body serves two kernels.  rows_sum_lists_kernel sums whole rows of
// width H = VPT*64 (both strides H, column 0).  rows_sum_lists_wide_kernel
// sums rows wider than one wave's H columns: blockIdx.y names a column
// segment of H columns, rows are src_stride / out_stride elements apart, so
// a list still gets one wave per H columns (the layer-1 dqkvs [N, 4h] is
// summed by category this way: embed_dgrad_fold in bindings.cpp).
template <int VPT, typename TIn, typename TOut, int U>
__device__ __forceinline__ void rows_sum_lists_body(
    const TIn* __restrict__ src, const int* __restrict__ idx,
    const int* __restrict__ lptr, TOut* __restrict__ out, int n_lists,
    long src_stride, long out_stride) {
  static_assert(VPT % 4 == 0, "packed loads need 4 columns per lane");
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int w = __builtin_amdgcn_readfirstlane(
      blockIdx.x * WAVES_PER_BLOCK + threadIdx.x / PERTGNN_WAVE);
  if (w >= n_lists) return;
  const int p0 = lptr[w];
  const int p1 = lptr[w + 1];
  float acc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) acc[j] = 0.f;
  int p = p0;
  for (; p + U <= p1; p += U) {
    int r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = idx[p + u];
    float v[U][VPT];
#pragma unroll
    for (int u = 0; u < U; ++u)
      rows_sum_load<VPT>(src + (long)r[u] * src_stride, lane, v[u]);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < VPT; ++j) acc[j] += v[u][j];
  }
  if (p < p1) {
    int r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) r[u] = idx[min(p + u, p1 - 1)];
    float v[U][VPT];
#pragma unroll
    for (int u = 0; u < U; ++u)
      rows_sum_load<VPT>(src + (long)r[u] * src_stride, lane, v[u]);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (p + u < p1) {
#pragma unroll
        for (int j = 0; j < VPT; ++j) acc[j] += v[u][j];
      }
  }
  TOut* dst = out + (long)w * out_stride + lane * VPT;
  if constexpr (sizeof(TOut) == 2) {
#pragma unroll
    for (int q = 0; q < VPT; q += 4) {
      segb4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = (__bf16)acc[q + u];
      *reinterpret_cast<segb4*>((__bf16*)dst + q) = o;
    }
  } else {
#pragma unroll
    for (int q = 0; q < VPT; q += 4) {
      segf4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) o[u] = acc[q + u];
      *reinterpret_cast<segf4*>((float*)dst + q) = o;
    }
  }
}

template <int VPT, typename TIn, typename TOut, int U>
__global__ void rows_sum_lists_kernel(const TIn* __restrict__ src,
                                      const int* __restrict__ idx,
                                      const int* __restrict__ lptr,
                                      TOut* __restrict__ out, int n_lists) {
  constexpr int H = VPT * PERTGNN_WAVE;
  rows_sum_lists_body<VPT, TIn, TOut, U>(src, idx, lptr, out, n_lists, H, H);
}

template <int VPT, typename TIn, int U>
__global__ void rows_sum_lists_wide_kernel(const TIn* __restrict__ src,
                                           const int* __restrict__ idx,
                                           const int* __restrict__ lptr,
                                           float* __restrict__ out,
                                           int n_lists, int src_stride,
                                           int out_stride) {
  const int col0 = blockIdx.y * (VPT * PERTGNN_WAVE);
  rows_sum_lists_body<VPT, TIn, float, U>(src + col0, idx, lptr, out + col0,
                                          n_lists, src_stride, out_stride);
}

// in16/out16: bf16 rows in / out (else fp32); h in {256, 512}; unroll in
// {4, 8}.  Only the three type pairs the edge-table gradient uses exist:
// bf16->fp32 and fp32->fp32 (levels 1 and 2), fp32->bf16 (final rows).
void launch_rows_sum_lists(const void* src, int in16, const int* idx,
                           const int* lptr, void* out, int out16, int n_lists,
                           int h, int unroll, hipStream_t s) {
  if (n_lists == 0) return;
  if (h != 256 && h != 512) pertgnn_shape_fail("rows_sum_lists", "h", h);
  if (unroll != 4 && unroll != 8)
    pertgnn_shape_fail("rows_sum_lists", "unroll", unroll);
  if (in16 && out16) pertgnn_shape_fail("rows_sum_lists", "in16+out16", 1);
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const dim3 grid(ceil_div(n_lists, WAVES_PER_BLOCK));
#define RSL(V, TI, TO, UU)                                                     \
  rows_sum_lists_kernel<V, TI, TO, UU><<<grid, block, 0, s>>>(                 \
      (const TI*)src, idx, lptr, (TO*)out, n_lists)
#define RSL_T(V, UU)                                                           \
  do {                                                                         \
    if (in16) RSL(V, __bf16, float, UU);                                       \
    else if (out16) RSL(V, float, __bf16, UU);                                 \
    else RSL(V, float, float, UU);                                             \
  } while (0)
  if (h == 256) {
    if (unroll == 8) RSL_T(4, 8); else RSL_T(4, 4);
  } else {
    if (unroll == 8) RSL_T(8, 8); else RSL_T(8, 4);
  }
#undef RSL_T
#undef RSL
}

// Wide form: rows of `width` columns (a multiple of seg_cols, 256 or 512),
// one wave per list and column segment; src rows are src_stride elements
// apart (bf16 if in16, else fp32), out rows out_stride fp32 elements.  Both
// strides and both base pointers keep every segment 16-byte aligned for fp32
// and 8-byte aligned for bf16 (strides % 4 == 0; checked by the binding).
void launch_rows_sum_lists_wide(const void* src, int in16, int src_stride,
                                const int* idx, const int* lptr, float* out,
                                int out_stride, int n_lists, int width,
                                int seg_cols, int unroll, hipStream_t s) {
  if (n_lists == 0) return;
  if (seg_cols != 256 && seg_cols != 512)
    pertgnn_shape_fail("rows_sum_lists_wide", "seg_cols", seg_cols);
  if (width <= 0 || width % seg_cols != 0)
    pertgnn_shape_fail("rows_sum_lists_wide", "width", width);
  if (src_stride < width || out_stride < width || src_stride % 4 != 0 ||
      out_stride % 4 != 0)
    pertgnn_shape_fail("rows_sum_lists_wide", "stride",
                       src_stride < out_stride ? src_stride : out_stride);
  if (unroll != 4 && unroll != 8)
    pertgnn_shape_fail("rows_sum_lists_wide", "unroll", unroll);
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const dim3 grid(ceil_div(n_lists, WAVES_PER_BLOCK), width / seg_cols);
#define RSW(V, TI, UU)                                                         \
  rows_sum_lists_wide_kernel<V, TI, UU><<<grid, block, 0, s>>>(                \
      (const TI*)src, idx, lptr, out, n_lists, src_stride, out_stride)
#define RSW_T(V, UU)                                                           \
  do {                                                                         \
    if (in16) RSW(V, __bf16, UU);                                              \
    else RSW(V, float, UU);                                                    \
  } while (0)
  if (seg_cols == 256) {
    if (unroll == 8) RSW_T(4, 8); else RSW_T(4, 4);
  } else {
    if (unroll == 8) RSW_T(8, 8); else RSW_T(8, 4);
  }
#undef RSW_T
#undef RSW
}

// Single-pass vocab accumulator for small vocabularies: blocks stream
// CONTIGUOUS gradient rows (coalesced, no sort/gather), accumulate into an
// LDS-resident [V,h] table (LDS atomics — contention only within the CU),
// then one global atomicAdd per (v,c) per block.  Weight-gradient class:
// fp32 reduction order varies run to run (same class as split-K wgrad).
__global__ void vocab_scatter_kernel(const float* __restrict__ g,
                                     const long* __restrict__ idx,
                                     long idx_stride, float* __restrict__ dtable,
                                     long n, int rows, int h, int gstride,
                                     int col_off) {
  extern __shared__ float acc[];  // [rows*h]
  const long vh = (long)rows * h;
  for (long t = threadIdx.x; t < vh; t += blockDim.x) acc[t] = 0.f;
  __syncthreads();
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(n, r0 + rows_per_block);
  for (long r = r0 + wid; r < r1; r += WAVES_PER_BLOCK) {
    const long v = idx[r * idx_stride];
    for (int c = lane; c < h; c += PERTGNN_WAVE)
      atomicAdd(&acc[v * h + c], g[r * gstride + col_off + c]);
  }
  __syncthreads();
  for (long t = threadIdx.x; t < vh; t += blockDim.x)
    if (acc[t] != 0.f) atomicAdd(&dtable[t], acc[t]);
}

// vectorized variant (h % 256 == 0, aligned): lane owns 4 contiguous columns
// — one f32x4 load per row instead of 4 strided scalars (measured: loads, not
// the LDS atomics, dominate this kernel).
__global__ void vocab_scatter_vec_kernel(const float* __restrict__ g,
                                         const long* __restrict__ idx,
                                         long idx_stride,
                                         float* __restrict__ dtable, long n,
                                         int rows, int h, int gstride,
                                         int col_off) {
  typedef __attribute__((ext_vector_type(4))) float f4;
  extern __shared__ float acc[];  // [rows*h]
  const long vh = (long)rows * h;
  for (long t = threadIdx.x; t < vh; t += blockDim.x) acc[t] = 0.f;
  __syncthreads();
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(n, r0 + rows_per_block);
  const int nq = h / (4 * PERTGNN_WAVE);  // f32x4 chunks per lane (1 at h=256)
  long r = r0 + wid;
  for (; r + WAVES_PER_BLOCK <= r1; r += 2 * WAVES_PER_BLOCK) {
    const long ra = r, rb = r + WAVES_PER_BLOCK;
    const long va = idx[ra * idx_stride];
    const long vb = idx[rb * idx_stride];
    for (int q = 0; q < nq; ++q) {
      const int c = (q * PERTGNN_WAVE + lane) * 4;
      const f4 xa = *reinterpret_cast<const f4*>(&g[ra * gstride + col_off + c]);
      const f4 xb = *reinterpret_cast<const f4*>(&g[rb * gstride + col_off + c]);
#pragma unroll
      for (int u = 0; u < 4; ++u) atomicAdd(&acc[va * h + c + u], xa[u]);
#pragma unroll
      for (int u = 0; u < 4; ++u) atomicAdd(&acc[vb * h + c + u], xb[u]);
    }
  }
  for (; r < r1; r += WAVES_PER_BLOCK) {
    const long v = idx[r * idx_stride];
    for (int q = 0; q < nq; ++q) {
      const int c = (q * PERTGNN_WAVE + lane) * 4;
      const f4 xv = *reinterpret_cast<const f4*>(&g[r * gstride + col_off + c]);
#pragma unroll
      for (int u = 0; u < 4; ++u) atomicAdd(&acc[v * h + c + u], xv[u]);
    }
  }
  __syncthreads();
  for (long t = threadIdx.x; t < vh; t += blockDim.x)
    if (acc[t] != 0.f) atomicAdd(&dtable[t], acc[t]);
}

// dual-table variant: accumulates BOTH vocab tables (interface + rpctype)
// in one pass over g — the two dP reductions of the attention backward share
// the same 56MB de stream.
typedef __attribute__((ext_vector_type(4))) float vs_f4;
typedef __attribute__((ext_vector_type(4))) __bf16 vs_b4;
__device__ __forceinline__ void vs_ld4(const float* p, float (&v)[4]) {
  *reinterpret_cast<vs_f4*>(v) = *reinterpret_cast<const vs_f4*>(p);
}
__device__ __forceinline__ void vs_ld4(const __bf16* p, float (&v)[4]) {
  const vs_b4 b = *reinterpret_cast<const vs_b4*>(p);
#pragma unroll
  for (int u = 0; u < 4; ++u) v[u] = (float)b[u];
}

// U rows are prefetched per loop iteration (independent index + gradient
// loads issue together before the LDS-atomic block) — the plain one-row loop
// exposes two dependent memory latencies per row and, at 1 block/CU, ran at
// ~200 GB/s; prefetch + 3 blocks/CU recovers the latency-bound gap.
template <typename GT, int U>
__global__ void vocab_scatter_dual_kernel(const GT* __restrict__ g,
                                          const long* __restrict__ ea,
                                          int astride,
                                          float* __restrict__ dt0,
                                          float* __restrict__ dt1, long n,
                                          int rows0, int rows1, int h) {
  extern __shared__ float acc[];  // [(rows0+rows1)*h]
  float* acc1 = acc + (long)rows0 * h;
  const long vh = (long)(rows0 + rows1) * h;
  for (long t = threadIdx.x; t < vh; t += blockDim.x) acc[t] = 0.f;
  __syncthreads();
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(n, r0 + rows_per_block);
  const int nq = h / (4 * PERTGNN_WAVE);
  const long step = WAVES_PER_BLOCK;
  long r = r0 + wid;
  for (; r + (U - 1) * step < r1; r += U * step) {
    long v0[U], v1[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v0[u] = ea[(r + u * step) * astride];
      v1[u] = ea[(r + u * step) * astride + 1];
    }
    for (int q = 0; q < nq; ++q) {
      const int c = (q * PERTGNN_WAVE + lane) * 4;
      float xv[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u) vs_ld4(&g[(r + u * step) * h + c], xv[u]);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          atomicAdd(&acc[v0[u] * h + c + k], xv[u][k]);
          atomicAdd(&acc1[v1[u] * h + c + k], xv[u][k]);
        }
    }
  }
  for (; r < r1; r += step) {
    const long v0 = ea[r * astride];
    const long v1 = ea[r * astride + 1];
    for (int q = 0; q < nq; ++q) {
      const int c = (q * PERTGNN_WAVE + lane) * 4;
      float xv[4];
      vs_ld4(&g[r * h + c], xv);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        atomicAdd(&acc[v0 * h + c + u], xv[u]);
        atomicAdd(&acc1[v1 * h + c + u], xv[u]);
      }
    }
  }
  __syncthreads();
  for (long t = threadIdx.x; t < (long)rows0 * h; t += blockDim.x)
    if (acc[t] != 0.f) atomicAdd(&dt0[t], acc[t]);
  for (long t = threadIdx.x; t < (long)rows1 * h; t += blockDim.x)
    if (acc1[t] != 0.f) atomicAdd(&dt1[t], acc1[t]);
}

// Wave-private variant — the production path.  Measured decomposition
// (benchmarks/vocab_micro.hip, E=216k/h=256/V=47): the LDS-atomic kernel is
// 100% ds_add_f32-bound at ~80 cycles/instruction (538 us; loads alone are
// 23 us; bank layout, unrolling, occupancy and index skew all change
// nothing).  Plain read+add+write into per-WAVE private tables removes the
// atomics entirely: 75 us for the same reduction (7.2x).  Each wave owns a
// private [rows0+rows1, HH] LDS table for one HH-wide column slice
// (grid.y = h/HH selects the slice); tables merge in LDS, one global-atomic
// flush per block.
template <typename GT, int U, int HH>
__global__ void vocab_scatter_dual_priv_kernel(const GT* __restrict__ g,
                                               const long* __restrict__ ea,
                                               int astride,
                                               float* __restrict__ dt0,
                                               float* __restrict__ dt1, long n,
                                               int rows0, int rows1, int h) {
  constexpr int CPL = HH / PERTGNN_WAVE;  // columns per lane
  extern __shared__ float acc[];  // [WAVES_PER_BLOCK][(rows0+rows1)*HH]
  const long vwh = (long)(rows0 + rows1) * HH;
  for (long t = threadIdx.x; t < WAVES_PER_BLOCK * vwh; t += blockDim.x)
    acc[t] = 0.f;
  __syncthreads();
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  float* my0 = acc + (long)wid * vwh;
  float* my1 = my0 + (long)rows0 * HH;
  const int c0 = blockIdx.y * HH;
  const long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(n, r0 + rows_per_block);
  const long step = WAVES_PER_BLOCK;
  long r = r0 + wid;
  for (; r + (U - 1) * step < r1; r += U * step) {
    long v0[U], v1[U];
    float xv[U][CPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v0[u] = ea[(r + u * step) * astride];
      v1[u] = ea[(r + u * step) * astride + 1];
#pragma unroll
      for (int k = 0; k < CPL; ++k)
        xv[u][k] = (float)g[(r + u * step) * h + c0 + lane * CPL + k];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) my0[v0[u] * HH + lane * CPL + k] += xv[u][k];
#pragma unroll
      for (int k = 0; k < CPL; ++k) my1[v1[u] * HH + lane * CPL + k] += xv[u][k];
    }
  }
  for (; r < r1; r += step) {
    const long v0 = ea[r * astride];
    const long v1 = ea[r * astride + 1];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const float x = (float)g[r * h + c0 + lane * CPL + k];
      my0[v0 * HH + lane * CPL + k] += x;
      my1[v1 * HH + lane * CPL + k] += x;
    }
  }
  __syncthreads();
  for (long t = threadIdx.x; t < vwh; t += blockDim.x)
    acc[t] += acc[vwh + t] + acc[2 * vwh + t] + acc[3 * vwh + t];
  __syncthreads();
  for (long t = threadIdx.x; t < (long)rows0 * HH; t += blockDim.x) {
    const float v = acc[t];
    if (v != 0.f) atomicAdd(&dt0[(t / HH) * h + c0 + t % HH], v);
  }
  for (long t = threadIdx.x; t < (long)rows1 * HH; t += blockDim.x) {
    const float v = acc[(long)rows0 * HH + t];
    if (v != 0.f) atomicAdd(&dt1[(t / HH) * h + c0 + t % HH], v);
  }
}

template <typename GT>
static void vocab_dual_impl(const GT* g, const long* ea, int astride,
                            float* dt0, float* dt1, long n, int rows0,
                            int rows1, int h, hipStream_t s) {
  HIP_CHECK(hipMemsetAsync(dt0, 0, (long)rows0 * h * sizeof(float), s));
  HIP_CHECK(hipMemsetAsync(dt1, 0, (long)rows1 * h * sizeof(float), s));
  if (n == 0) return;
  // wave-private path (7.2x the LDS-atomic kernel, see kernel comment)
  const long vrows = rows0 + rows1;
  // block count scaled inversely with table size: each extra block
  // costs a table-sized atomic merge, but small tables (rpctype ~5
  // rows) need far more than 128 blocks to occupy 256 CUs (measured
  // 1 wave/SIMD at the old cap)
  const long merge_cap = (long)1000000 / (long)max((int)vrows * 128, 1);
  const int blocks =
      (int)min((n + 255) / 256, max((long)128, min((long)768, merge_cap)));
  const size_t lds128 = (size_t)WAVES_PER_BLOCK * vrows * 128 * sizeof(float);
  const size_t lds64 = (size_t)WAVES_PER_BLOCK * vrows * 64 * sizeof(float);
  if (h % 128 == 0 && lds128 <= 160 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)vocab_scatter_dual_priv_kernel<GT, 4, 128>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds128));
    vocab_scatter_dual_priv_kernel<GT, 4, 128>
        <<<dim3(max(blocks, 1), h / 128),
           dim3(WAVES_PER_BLOCK * PERTGNN_WAVE), lds128, s>>>(
            g, ea, astride, dt0, dt1, n, rows0, rows1, h);
    return;
  }
  if (h % 64 == 0 && lds64 <= 160 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)vocab_scatter_dual_priv_kernel<GT, 4, 64>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds64));
    vocab_scatter_dual_priv_kernel<GT, 4, 64>
        <<<dim3(max(blocks, 1), h / 64),
           dim3(WAVES_PER_BLOCK * PERTGNN_WAVE), lds64, s>>>(
            g, ea, astride, dt0, dt1, n, rows0, rows1, h);
    return;
  }
  const size_t lds = (size_t)vrows * h * sizeof(float);
  if (lds > 64 * 1024) {
    HIP_CHECK(hipFuncSetAttribute(
        (const void*)vocab_scatter_dual_kernel<GT, 4>,
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  const int ablocks = (int)min((long)768, (n + 63) / 64);
  vocab_scatter_dual_kernel<GT, 4><<<dim3(max(ablocks, 1)),
                                     dim3(WAVES_PER_BLOCK * PERTGNN_WAVE), lds,
                                     s>>>(g, ea, astride, dt0, dt1, n, rows0,
                                          rows1, h);
}

void launch_vocab_scatter_dual(const float* g, const long* ea, int astride,
                               float* dt0, float* dt1, long n, int rows0,
                               int rows1, int h, hipStream_t s) {
  vocab_dual_impl<float>(g, ea, astride, dt0, dt1, n, rows0, rows1, h, s);
}

void launch_vocab_scatter_dual16(const void* g, const long* ea, int astride,
                                 float* dt0, float* dt1, long n, int rows0,
                                 int rows1, int h, hipStream_t s) {
  vocab_dual_impl<__bf16>((const __bf16*)g, ea, astride, dt0, dt1, n, rows0,
                          rows1, h, s);
}

// single-table wave-private variant (same rationale/measurements as the dual
// kernel above: plain LDS read+add+write beats ds_add_f32 ~7x)
template <int U, int HH, typename GT = float>
__global__ void vocab_scatter_priv_kernel(const GT* __restrict__ g,
                                          const long* __restrict__ idx,
                                          long idx_stride,
                                          float* __restrict__ dtable, long n,
                                          int rows, int h, int gstride,
                                          int col_off) {
  constexpr int CPL = HH / PERTGNN_WAVE;
  extern __shared__ float acc[];  // [WAVES_PER_BLOCK][rows*HH]
  const long vwh = (long)rows * HH;
  for (long t = threadIdx.x; t < WAVES_PER_BLOCK * vwh; t += blockDim.x)
    acc[t] = 0.f;
  __syncthreads();
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  float* my = acc + (long)wid * vwh;
  const int c0 = blockIdx.y * HH;
  const long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(n, r0 + rows_per_block);
  const long step = WAVES_PER_BLOCK;
  long r = r0 + wid;
  for (; r + (U - 1) * step < r1; r += U * step) {
    long v[U];
    float xv[U][CPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      v[u] = idx[(r + u * step) * idx_stride];
#pragma unroll
      for (int k = 0; k < CPL; ++k)
        xv[u][k] = (float)g[(r + u * step) * gstride + col_off + c0 + lane * CPL + k];
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < CPL; ++k) my[v[u] * HH + lane * CPL + k] += xv[u][k];
  }
  for (; r < r1; r += step) {
    const long v = idx[r * idx_stride];
#pragma unroll
    for (int k = 0; k < CPL; ++k)
      my[v * HH + lane * CPL + k] +=
          (float)g[r * gstride + col_off + c0 + lane * CPL + k];
  }
  __syncthreads();
  for (long t = threadIdx.x; t < vwh; t += blockDim.x)
    acc[t] += acc[vwh + t] + acc[2 * vwh + t] + acc[3 * vwh + t];
  __syncthreads();
  for (long t = threadIdx.x; t < vwh; t += blockDim.x) {
    const float val = acc[t];
    if (val != 0.f) atomicAdd(&dtable[(t / HH) * h + c0 + t % HH], val);
  }
}

template <int HH, typename GT>
static void vocab_priv_launch(const GT* g, const long* idx, long idx_stride,
                              float* dtable, long n, int rows, int h,
                              int gstride, int col_off, int blocks, size_t lds,
                              hipStream_t s) {
  HIP_CHECK(hipFuncSetAttribute(
      (const void*)vocab_scatter_priv_kernel<4, HH, GT>,
      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  vocab_scatter_priv_kernel<4, HH, GT>
      <<<dim3(max(blocks, 1), h / HH), dim3(WAVES_PER_BLOCK * PERTGNN_WAVE),
         lds, s>>>(g, idx, idx_stride, dtable, n, rows, h, gstride, col_off);
}

// GT = float (launch_vocab_scatter) or __bf16 (launch_vocab_scatter16).  The
// wave-private kernel takes either; the whole-table kernels behind it are
// fp32 only, so a bf16 gradient whose private tables do not fit is an error
// (the caller upcasts it to f32)
template <typename GT>
static void vocab_scatter_launch(const GT* g, const long* idx,
                                 long idx_stride, float* dtable, long n,
                                 int rows, int h, int gstride, int col_off,
                                 hipStream_t s) {
  HIP_CHECK(hipMemsetAsync(dtable, 0, (long)rows * h * sizeof(float), s));
  if (n == 0) return;
  // block count scaled inversely with table size: each extra block
  // costs a table-sized atomic merge, but small tables (rpctype ~5
  // rows) need far more than 128 blocks to occupy 256 CUs (measured
  // 1 wave/SIMD at the old cap)
  const long merge_cap = (long)1000000 / (long)max(rows * 128, 1);
  const int pblocks =
      (int)min((n + 255) / 256, max((long)128, min((long)768, merge_cap)));
  const size_t lds128 = (size_t)WAVES_PER_BLOCK * rows * 128 * sizeof(float);
  const size_t lds64 = (size_t)WAVES_PER_BLOCK * rows * 64 * sizeof(float);
  if (h % 128 == 0 && lds128 <= 160 * 1024) {
    vocab_priv_launch<128>(g, idx, idx_stride, dtable, n, rows, h, gstride,
                           col_off, pblocks, lds128, s);
    return;
  }
  if (h % 64 == 0 && lds64 <= 160 * 1024) {
    vocab_priv_launch<64>(g, idx, idx_stride, dtable, n, rows, h, gstride,
                          col_off, pblocks, lds64, s);
    return;
  }
  if constexpr (!std::is_same_v<GT, float>) {
    pertgnn_shape_fail("vocab_scatter", "table_bytes_over_lds_h", h);
  } else {
    const size_t lds = (size_t)rows * h * sizeof(float);
    const bool vec = (h % (4 * PERTGNN_WAVE) == 0) && ((gstride & 3) == 0) &&
                     ((col_off & 3) == 0);
    const void* fn = vec ? (const void*)vocab_scatter_vec_kernel
                         : (const void*)vocab_scatter_kernel;
    if (lds > 64 * 1024) {
      HIP_CHECK(hipFuncSetAttribute(
          fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    const int blocks = (int)min((long)256, (n + 63) / 64);
    if (vec)
      vocab_scatter_vec_kernel<<<dim3(blocks),
                                 dim3(WAVES_PER_BLOCK * PERTGNN_WAVE), lds,
                                 s>>>(g, idx, idx_stride, dtable, n, rows, h,
                                      gstride, col_off);
    else
      vocab_scatter_kernel<<<dim3(blocks),
                             dim3(WAVES_PER_BLOCK * PERTGNN_WAVE), lds, s>>>(
          g, idx, idx_stride, dtable, n, rows, h, gstride, col_off);
  }
}

void launch_vocab_scatter(const float* g, const long* idx, long idx_stride,
                          float* dtable, long n, int rows, int h, int gstride,
                          int col_off, hipStream_t s) {
  vocab_scatter_launch(g, idx, idx_stride, dtable, n, rows, h, gstride,
                       col_off, s);
}

void launch_vocab_scatter16(const void* g, const long* idx, long idx_stride,
                            float* dtable, long n, int rows, int h,
                            int gstride, int col_off, hipStream_t s) {
  vocab_scatter_launch((const __bf16*)g, idx, idx_stride, dtable, n, rows, h,
                       gstride, col_off, s);
}

// entry embedding gather: out[b] = table[idx[b]] — plain gather (fwd) +
// scatter-add (bwd); reuses the edge kernels' grid-stride shape.
__global__ void gather_rows_kernel(const long* __restrict__ idx,
                                   const float* __restrict__ table,
                                   float* __restrict__ out, long n, int h) {
  const long numel = n * h;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = i0; t < numel; t += stride) {
    const long row = t / h;
    const int c = (int)(t - row * h);
    out[t] = table[idx[row] * h + c];
  }
}

__global__ void scatter_add_rows_kernel(const float* __restrict__ g,
                                        const long* __restrict__ idx,
                                        float* __restrict__ dtable, long n,
                                        int h) {
  const long numel = n * h;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = i0; t < numel; t += stride) {
    const long row = t / h;
    const int c = (int)(t - row * h);
    atomicAdd(&dtable[idx[row] * h + c], g[t]);
  }
}

static int grid_for(long numel, int tpb = 256, long cap = 4096) {
  return (int)min((numel + tpb - 1) / tpb, cap);
}

void launch_embed_node_fwd(const float* x_raw, const long* idx,
                           const float* table, float* out, long n, int f,
                           int h, hipStream_t s) {
  if (n == 0) return;
  embed_node_fwd_kernel<<<grid_for(n * (f + h)), 256, 0, s>>>(x_raw, idx, table,
                                                              out, n, f, h);
}

void launch_embed_node_fwd16(const float* x_raw, const long* idx,
                             const float* table, void* out, long n, int f,
                             int h, hipStream_t stream) {
  if (n == 0) return;
  const long numel = n * (long)(f + h);
  const int tpb = 256;
  const int blocks = (int)min((numel + tpb - 1) / tpb, (long)4096);
  embed_node_fwd_kernel<<<dim3(blocks), dim3(tpb), 0, stream>>>(
      x_raw, idx, table, (__bf16*)out, n, f, h);
}

// padded output [n, pad_to], pad_to >= f + h (checked by the binding)
template <typename TY, int EPC>
static void embed_node_pad_launch(const float* x_raw, const long* idx,
                                  const float* table, TY* out, long n, int f,
                                  int h, int pad_to, hipStream_t s) {
  // lanes per row: the sub-wave width that wastes the fewest lane slots on
  // the row's pad_to / EPC chunks, the widest on a tie
  const int chunks = pad_to / EPC;
  int lpr = PERTGNN_WAVE;
  for (int l = PERTGNN_WAVE; l >= 8; l /= 2)
    if (ceil_div(chunks, l) * l < ceil_div(chunks, lpr) * lpr) lpr = l;
  const int tpb = 256;
  const long rows_per_block = (long)(tpb / PERTGNN_WAVE) * (PERTGNN_WAVE / lpr);
  const dim3 grid((unsigned)min((n + rows_per_block - 1) / rows_per_block,
                                (long)8192));
#define LAUNCH(L)                                                              \
  embed_node_pad_kernel<TY, EPC, L>                                            \
      <<<grid, dim3(tpb), 0, s>>>(x_raw, idx, table, out, n, f, h, pad_to)
  if (lpr == 64) LAUNCH(64);
  else if (lpr == 32) LAUNCH(32);
  else if (lpr == 16) LAUNCH(16);
  else LAUNCH(8);
#undef LAUNCH
}

void launch_embed_node_pad(const float* x_raw, const long* idx,
                           const float* table, void* out, int out16, long n,
                           int f, int h, int pad_to, hipStream_t s) {
  if (n == 0) return;
  if (out16) {
    if (pad_to % 8 == 0)
      embed_node_pad_launch<__bf16, 8>(x_raw, idx, table, (__bf16*)out, n, f,
                                       h, pad_to, s);
    else
      embed_node_pad_launch<__bf16, 1>(x_raw, idx, table, (__bf16*)out, n, f,
                                       h, pad_to, s);
  } else {
    if (pad_to % 4 == 0)
      embed_node_pad_launch<float, 4>(x_raw, idx, table, (float*)out, n, f, h,
                                      pad_to, s);
    else
      embed_node_pad_launch<float, 1>(x_raw, idx, table, (float*)out, n, f, h,
                                      pad_to, s);
  }
}

void launch_embed_edge_fwd(const long* attr, const float* ifc,
                           const float* rpc, float* out, long e, int h,
                           int astride, hipStream_t s) {
  if (e == 0) return;
  embed_edge_fwd_kernel<<<grid_for(e * 2 * h), 256, 0, s>>>(attr, ifc, rpc, out,
                                                            e, h, astride);
}
void launch_gather_rows(const long* idx, const float* table, float* out,
                        long n, int h, hipStream_t s) {
  if (n == 0) return;
  gather_rows_kernel<<<grid_for(n * h), 256, 0, s>>>(idx, table, out, n, h);
}

// ---------------------------------------------------------------------------
// BatchNorm1d (+ReLU) — two-stage column reduction, coalesced row tiles
// ---------------------------------------------------------------------------

// stage A: per-block partial sum/sumsq over a row range; thread t owns
// channels t and t+256 in REGISTERS (H <= 512), one atomicAdd per channel
// per block at the end — coalesced loads, no LDS traffic.
// adjacent-channel pair load: one 4-B (bf16) / 8-B (fp32) transaction for
// the thread's two channels (c, c+1) — halves the load count of the
// latency-bound per-channel reduction kernels
__device__ __forceinline__ void bn_ld2(const float* p, float& a, float& b) {
  typedef __attribute__((ext_vector_type(2))) float f2_t;
  const f2_t v = *reinterpret_cast<const f2_t*>(p);
  a = v[0]; b = v[1];
}
__device__ __forceinline__ void bn_ld2(const __bf16* p, float& a, float& b) {
  typedef __attribute__((ext_vector_type(2))) __bf16 b2_t;
  const b2_t v = *reinterpret_cast<const b2_t*>(p);
  a = (float)v[0]; b = (float)v[1];
}

template <typename TX = float, bool SLAB = false>
__global__ void bn_stats_partial_kernel(const TX* __restrict__ x, long n,
                                        int h, float* __restrict__ partials) {
  // ADJACENT channel pair per thread (c0 = 2*tid, c1 = c0+1): one paired
  // load serves both, halving the load count of this latency-bound kernel
  const int c0 = 2 * threadIdx.x;
  const int c1 = c0 + 1;
  float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
  const long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(n, r0 + rows_per_block);
  long r = r0;
  if ((h & 1) == 0 && c1 < h) {
    // 8-row unroll: the kernel is latency-bound (one bf16x2 load per
    // channel pair per row) — 8 independent loads in flight halve the
    // stall count vs 4 (measured 58.7 -> ~35 us at 180k x 256)
    for (; r + 16 <= r1; r += 16) {
      float a[16], b[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) bn_ld2(&x[(r + u) * h + c0], a[u], b[u]);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        s0 += a[u]; q0 += a[u] * a[u];
        s1 += b[u]; q1 += b[u] * b[u];
      }
    }
    for (; r < r1; ++r) {
      float a, b;
      bn_ld2(&x[r * h + c0], a, b);
      s0 += a; q0 += a * a;
      s1 += b; q1 += b * b;
    }
  } else {
    for (; r < r1; ++r) {
      if (c0 < h) {
        const float v = x[r * h + c0];
        s0 += v; q0 += v * v;
      }
      if (c1 < h) {
        const float v = x[r * h + c1];
        s1 += v; q1 += v * v;
      }
    }
  }
  if (SLAB) {
    // deterministic mode: per-block slab row, reduced in fixed block order
    float* row = partials + (long)blockIdx.x * 2 * h;
    if (c0 < h) { row[c0] = s0; row[h + c0] = q0; }
    if (c1 < h) { row[c1] = s1; row[h + c1] = q1; }
    return;
  }
  if (c0 < h && r0 < r1) {
    atomicAdd(&partials[c0], s0);
    atomicAdd(&partials[h + c0], q0);
  }
  if (c1 < h && r0 < r1) {
    atomicAdd(&partials[c1], s1);
    atomicAdd(&partials[h + c1], q1);
  }
}

// fixed-order fold of the deterministic-mode slab rows
__global__ void bn_slab_reduce_kernel(const float* __restrict__ slab, int nb,
                                      int w, float* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= w) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += slab[(long)b * w + c];
  out[c] = s;
}

// lazily-allocated device slab for the deterministic BN reductions of the
// pair-per-thread kernels (512 blocks x 2 x 1024 channels); deterministic
// mode is documented as incompatible with hipGraph capture, so the lazy
// hipMalloc is safe.  The wide-load path below does not use it: its slab is
// a per-call tensor from the binding layer.
static float* bn_det_slab() {
  static float* p = [] {
    float* q = nullptr;
    HIP_CHECK(hipMalloc(&q, (size_t)512 * 2 * 1024 * sizeof(float)));
    return q;
  }();
  return p;
}

static inline bool pertgnn_deterministic_seg() {
  const char* e = getenv("PERTGNN_DETERMINISTIC");
  return e && e[0] == '1';
}

// grid size for the BN channel reductions (atomic-combine path): 512 blocks
// is 2 blocks/CU — enough to stream ~3.5 TB/s but measurably latency-bound
// on the single-stream stats kernel; PERTGNN_BN_BLOCKS overrides for tuning
static inline int bn_partial_blocks(long n) {
  static const int env = [] {
    const char* e = getenv("PERTGNN_BN_BLOCKS");
    return e ? atoi(e) : 0;
  }();
  const long cap = (n + 63) / 64;
  const long want = env > 0 ? env : 512;
  return (int)min(want, cap);
}

template <typename TX>
static void bn_stats_dispatch(const TX* x, long n, int h, float* partials,
                              hipStream_t s) {
  const int nblocks = pertgnn_deterministic_seg()
                          ? (int)min((long)512, (n + 63) / 64)
                          : bn_partial_blocks(n);
  if (pertgnn_deterministic_seg() && h <= 1024) {
    float* slab = bn_det_slab();
    bn_stats_partial_kernel<TX, true><<<nblocks, 256, 0, s>>>(x, n, h, slab);
    bn_slab_reduce_kernel<<<ceil_div(2 * h, 256), 256, 0, s>>>(
        slab, nblocks, 2 * h, partials);
  } else {
    HIP_CHECK(hipMemsetAsync(partials, 0, 2 * h * sizeof(float), s));
    bn_stats_partial_kernel<TX, false><<<nblocks, 256, 0, s>>>(x, n, h,
                                                               partials);
  }
}


// stage B: finalize mean/invstd (+ running-stat update, training only)
// count_ptr (may be null): device-side GLOBAL row count — sync-BN appends
// the local count to the stats partials so ONE all-reduce carries sums AND
// count, with no host round-trip per BN layer (the count slot lives at
// partials[2h], untouched by the 2h-wide reducers).
__global__ void bn_finalize_kernel(const float* __restrict__ partials, long n,
                                   int h, float eps, float momentum,
                                   float* __restrict__ mean,
                                   float* __restrict__ invstd,
                                   float* __restrict__ running_mean,
                                   float* __restrict__ running_var,
                                   int update_running,
                                   const float* __restrict__ count_ptr = nullptr) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= h) return;
  const float nf = count_ptr ? *count_ptr : (float)n;
  const float m = partials[c] / nf;
  const float var = fmaxf(partials[h + c] / nf - m * m, 0.f);
  mean[c] = m;
  invstd[c] = rsqrtf(var + eps);
  if (update_running) {
    const float unbiased = (nf > 1.f) ? var * nf / (nf - 1.f) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
  }
}

// counter-based per-element uniform for fused dropout (splitmix64 mix of
// the device-resident step counter and the element index; quality is ample
// for dropout masks and the sequence is deterministic given the counter)
__device__ __forceinline__ float bn_rand01(unsigned long long seed, long t) {
  unsigned long long z = seed * 0x9E3779B97F4A7C15ull + (unsigned long long)t;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.f / 16777216.f);  // top 24 bits
}

// stage C: normalize + affine (+ReLU) (+fused dropout: reference K8 — the
// model applies dropout right after BN+ReLU, model.py:101-103; keep_inv =
// 1/(1-p), seed_ptr = device step counter so captured hipGraphs draw FRESH
// masks every replay).  Post-dropout y==0 <=> dropped-or-relu-negative, so
// the backward needs NO RNG: the existing y<=0 mask plus the keep_inv
// scale reproduces d(dropout.relu)/dy exactly.
// TY = output/activation dtype: fp32 in exact mode, bf16 in the act16 mode
// (standard mixed-precision BN: statistics and normalization math stay fp32,
// only the activation stream is 16-bit).
// DROP is a TEMPLATE parameter: the hash-RNG code measurably bloats the
// 4-wide loop even when dropout_p==0 at runtime (bn_apply 39 -> 168 us at
// 181k x 256), so the p==0 instantiation must not contain it.
template <typename TY, typename TX = float, bool DROP = false>
__global__ void bn_apply_kernel(const TX* __restrict__ x,
                                const float* __restrict__ mean,
                                const float* __restrict__ invstd,
                                const float* __restrict__ gamma,
                                const float* __restrict__ beta,
                                TY* __restrict__ y, long n, int h,
                                int relu, float dropout_p = 0.f,
                                const unsigned long long* __restrict__
                                    seed_ptr = nullptr) {
  typedef __attribute__((ext_vector_type(4))) float bnf4;
  const float keep_inv = DROP ? 1.f / (1.f - dropout_p) : 1.f;
  unsigned long long seed = 0ull;
  if constexpr (DROP) seed = seed_ptr ? *seed_ptr : 0ull;
  if ((h & 3) == 0) {  // 4-wide: one f32x4 load + packed store per thread
    const long numq = n * (h / 4);
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long q = i0; q < numq; q += stride) {
      const long t = q * 4;
      const int c = (int)(t % h);
      float xv[4];
      vs_ld4(&x[t], xv);
      struct alignas(4 * sizeof(TY)) TY4 { TY v[4]; };
      TY4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float v = (xv[u] - mean[c + u]) * invstd[c + u] * gamma[c + u] +
                  beta[c + u];
        if (relu) v = fmaxf(v, 0.f);
        if constexpr (DROP)
          v = (bn_rand01(seed, t + u) >= dropout_p) ? v * keep_inv : 0.f;
        o.v[u] = (TY)v;
      }
      *reinterpret_cast<TY4*>(&y[t]) = o;  // one packed 8B/16B store
    }
    return;
  }
  const long numel = n * h;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = i0; t < numel; t += stride) {
    const int c = (int)(t % h);
    float v = ((float)x[t] - mean[c]) * invstd[c] * gamma[c] + beta[c];
    if (relu) v = fmaxf(v, 0.f);
    if constexpr (DROP)
      v = (bn_rand01(seed, t) >= dropout_p) ? v * keep_inv : 0.f;
    y[t] = (TY)v;
  }
}

__global__ void counter_bump_kernel(unsigned long long* __restrict__ c) {
  ++*c;
}

// backward stage A: per-channel sums of gm and gm*xhat (gm = relu-masked g)
template <typename TG, typename TY, typename TX = float, bool SLAB = false>
__global__ void bn_bwd_partial_kernel(const TG* __restrict__ g,
                                      const TX* __restrict__ x,
                                      const TY* __restrict__ y,
                                      const float* __restrict__ mean,
                                      const float* __restrict__ invstd, long n,
                                      int h, int relu,
                                      float* __restrict__ partials,
                                      float keep_inv = 1.f) {
  // adjacent channel pair per thread (see bn_stats): paired g/y/x loads
  const int c0 = 2 * threadIdx.x;
  const int c1 = c0 + 1;
  float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
  const long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(n, r0 + rows_per_block);
  const float m0 = (c0 < h) ? mean[c0] : 0.f;
  const float i0 = (c0 < h) ? invstd[c0] : 0.f;
  const float m1 = (c1 < h) ? mean[c1] : 0.f;
  const float i1 = (c1 < h) ? invstd[c1] : 0.f;
  long r = r0;
  if ((h & 1) == 0 && c1 < h) {
    for (; r + 8 <= r1; r += 8) {
      float ga[8], gb[8], ya[8], yb[8], xa[8], xb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        bn_ld2(&g[(r + u) * h + c0], ga[u], gb[u]);
        bn_ld2(&y[(r + u) * h + c0], ya[u], yb[u]);
        bn_ld2(&x[(r + u) * h + c0], xa[u], xb[u]);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        float gm0 = (relu && ya[u] <= 0.f) ? 0.f : ga[u] * keep_inv;
        float gm1 = (relu && yb[u] <= 0.f) ? 0.f : gb[u] * keep_inv;
        s0 += gm0; q0 += gm0 * (xa[u] - m0) * i0;
        s1 += gm1; q1 += gm1 * (xb[u] - m1) * i1;
      }
    }
    for (; r < r1; ++r) {
      float ga, gb, ya, yb, xa, xb;
      bn_ld2(&g[r * h + c0], ga, gb);
      bn_ld2(&y[r * h + c0], ya, yb);
      bn_ld2(&x[r * h + c0], xa, xb);
      float gm0 = (relu && ya <= 0.f) ? 0.f : ga * keep_inv;
      float gm1 = (relu && yb <= 0.f) ? 0.f : gb * keep_inv;
      s0 += gm0; q0 += gm0 * (xa - m0) * i0;
      s1 += gm1; q1 += gm1 * (xb - m1) * i1;
    }
  } else {
    for (; r < r1; ++r) {
      if (c0 < h) {
        float gm = (float)g[r * h + c0] * keep_inv;
        if (relu && (float)y[r * h + c0] <= 0.f) gm = 0.f;
        s0 += gm;
        q0 += gm * ((float)x[r * h + c0] - m0) * i0;
      }
      if (c1 < h) {
        float gm = (float)g[r * h + c1] * keep_inv;
        if (relu && (float)y[r * h + c1] <= 0.f) gm = 0.f;
        s1 += gm;
        q1 += gm * ((float)x[r * h + c1] - m1) * i1;
      }
    }
  }
  if (SLAB) {
    float* row = partials + (long)blockIdx.x * 2 * h;
    if (c0 < h) { row[c0] = s0; row[h + c0] = q0; }
    if (c1 < h) { row[c1] = s1; row[h + c1] = q1; }
    return;
  }
  if (c0 < h && r0 < r1) {
    atomicAdd(&partials[c0], s0);
    atomicAdd(&partials[h + c0], q0);
  }
  if (c1 < h && r0 < r1) {
    atomicAdd(&partials[c1], s1);
    atomicAdd(&partials[h + c1], q1);
  }
}


template <typename TG, typename TY, typename TX>
static void bn_bwd_partials_dispatch(const TG* g, const TX* x, const TY* y,
                                     const float* mean, const float* invstd,
                                     long n, int h, bool relu, float* partials,
                                     float keep_inv, hipStream_t s) {
  const int nblocks = pertgnn_deterministic_seg()
                          ? (int)min((long)512, (n + 63) / 64)
                          : bn_partial_blocks(n);
  if (pertgnn_deterministic_seg() && h <= 1024) {
    float* slab = bn_det_slab();
    bn_bwd_partial_kernel<TG, TY, TX, true><<<nblocks, 256, 0, s>>>(
        g, x, y, mean, invstd, n, h, relu ? 1 : 0, slab, keep_inv);
    bn_slab_reduce_kernel<<<ceil_div(2 * h, 256), 256, 0, s>>>(
        slab, nblocks, 2 * h, partials);
  } else {
    HIP_CHECK(hipMemsetAsync(partials, 0, 2 * h * sizeof(float), s));
    bn_bwd_partial_kernel<TG, TY, TX, false><<<nblocks, 256, 0, s>>>(
        g, x, y, mean, invstd, n, h, relu ? 1 : 0, partials, keep_inv);
  }
}

// backward stage B: dx = gamma*invstd*(gm - sum_gm/n - xhat*sum_gmx/n)
// 4-wide vectorized (16-bit scalar loads left the kernel latency-bound:
// 163 us vs 133 us fp32 at 165k x 256 — 4x-unrolled loads recover it)
template <typename TG, typename TY, typename TX = float>
__global__ void bn_bwd_apply_kernel(
    const TG* __restrict__ g, const TX* __restrict__ x,
    const TY* __restrict__ y, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ partials, TX* __restrict__ dx, long n,
    long count, int h, int relu,
    const float* __restrict__ count_ptr = nullptr, float keep_inv = 1.f) {
  typedef __attribute__((ext_vector_type(4))) float bnf4;
  const float invn = 1.f / (count_ptr ? *count_ptr : (float)count);
  if ((h & 3) == 0) {
    const long numq = n * (h / 4);
    const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    struct alignas(4 * sizeof(TG)) TG4 { TG v[4]; };
    struct alignas(4 * sizeof(TY)) TY4 { TY v[4]; };
    for (long q = i0; q < numq; q += stride) {
      const long t = q * 4;
      const int c = (int)(t % h);
      float gv[4], yv[4], xv[4];
      // vectorized g/y quad loads (4 scalar 16-bit loads left this kernel
      // issue-bound alongside the already-vector x load)
      const TG4 gq = *reinterpret_cast<const TG4*>(&g[t]);
#pragma unroll
      for (int u = 0; u < 4; ++u) gv[u] = (float)gq.v[u];
      if (relu) {
        const TY4 yq = *reinterpret_cast<const TY4*>(&y[t]);
#pragma unroll
        for (int u = 0; u < 4; ++u) yv[u] = (float)yq.v[u];
      }
      vs_ld4(&x[t], xv);
      struct alignas(4 * sizeof(TX)) TX4 { TX v[4]; };
      TX4 o;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float gm = gv[u] * keep_inv;
        if (relu && yv[u] <= 0.f) gm = 0.f;
        const float xhat = (xv[u] - mean[c + u]) * invstd[c + u];
        o.v[u] = (TX)(gamma[c + u] * invstd[c + u] *
                      (gm - partials[c + u] * invn -
                       xhat * partials[h + c + u] * invn));
      }
      *reinterpret_cast<TX4*>(&dx[t]) = o;
    }
    return;
  }
  const long numel = n * h;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = i0; t < numel; t += stride) {
    const int c = (int)(t % h);
    float gm = (float)g[t] * keep_inv;
    if (relu && (float)y[t] <= 0.f) gm = 0.f;
    const float xhat = ((float)x[t] - mean[c]) * invstd[c];
    dx[t] = (TX)(gamma[c] * invstd[c] *
                 (gm - partials[c] * invn - xhat * partials[h + c] * invn));
  }
}

// dgamma[c] = sum gm*xhat = partials[h+c]; dbeta[c] = sum gm = partials[c];
// acc: dgamma/dbeta are gradient sinks, added to instead of stored
__global__ void bn_grad_affine_kernel(const float* __restrict__ partials,
                                      float* __restrict__ dgamma,
                                      float* __restrict__ dbeta, int h,
                                      int acc) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= h) return;
  if (acc) {
    dgamma[c] += partials[h + c];
    dbeta[c] += partials[c];
  } else {
    dgamma[c] = partials[h + c];
    dbeta[c] = partials[c];
  }
}

// ---------------------------------------------------------------------------
// Wide-load BN reductions: every lane owns 8 ADJACENT channels and loads them
// with one 16-B instruction (two for an fp32 stream); h/8 lanes cover a row
// and a 256-thread block covers 256/(h/8) rows ("row slots") per iteration.
// Taken when h % 8 == 0 and 256 % (h/8) == 0 (h = 8..2048 in powers of
// two); every other shape stays on the pair-per-thread kernels above.
//
// The bf16 training forward with ReLU also emits a bit-packed keep mask
// mask[N, h/8] (bit u of byte (r, c/8) = !(y[r, c+u] <= 0) on the STORED
// bf16 value, after dropout), and the backward reads that 1 bit/element in
// place of the whole y stream.
// ---------------------------------------------------------------------------

bool bn_wide_ok(int h) {
  return h >= 8 && (h & 7) == 0 && 256 % (h >> 3) == 0;
}

// cross-block combine of the wide reductions: per-block slab row + fixed-
// order fold kernel (default, also the deterministic mode), or float atomics
// into the one partials row (PERTGNN_BN_COMBINE=atomic)
static inline bool bn_wide_atomic() {
  if (pertgnn_deterministic_seg()) return false;
  const char* e = getenv("PERTGNN_BN_COMBINE");
  return e && e[0] == 'a';
}

// grid of the wide reductions.  PERTGNN_BN_BLOCKS is taken as given (blocks
// with an empty row range contribute exact zeros), clamped to 4096.
static inline int bn_wide_blocks(long n) {
  const char* e = getenv("PERTGNN_BN_BLOCKS");
  const int env = e ? atoi(e) : 0;
  if (env > 0) return env < 4096 ? env : 4096;
  const long cap = (n + 63) / 64;
  return (int)(cap < 512 ? (cap > 0 ? cap : 1) : 512);
}

// slab rows ([rows, 2h] fp32) the caller has to provide for a wide reduction
// over [n, h]; 0 = no slab (other shape, n == 0, or the atomic combine)
int bn_wide_slab_rows(long n, int h) {
  if (n <= 0 || !bn_wide_ok(h) || bn_wide_atomic()) return 0;
  return bn_wide_blocks(n);
}

typedef __attribute__((ext_vector_type(4))) unsigned int bn_u4;

// 8 adjacent bf16 -> fp32 from one 16-B load (bf16 -> fp32 is a 16-bit shift)
__device__ __forceinline__ void bn_ld8(const __bf16* p, float (&v)[8]) {
  const bn_u4 w = *reinterpret_cast<const bn_u4*>(p);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] = __uint_as_float(w[k] << 16);
    v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
  }
}

// fp32 stream: the lane's 8 channels are two 16-B loads
__device__ __forceinline__ void bn_ld8(const float* p, float (&v)[8]) {
  typedef __attribute__((ext_vector_type(4))) float bn_f4;
  const bn_f4 a = *reinterpret_cast<const bn_f4*>(p);
  const bn_f4 b = *reinterpret_cast<const bn_f4*>(p + 4);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = a[k];
    v[4 + k] = b[k];
  }
}

__device__ __forceinline__ void bn_st8(__bf16* p, const __bf16 (&o)[8]) {
  bn_u4 w;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    w[k] = (unsigned)__builtin_bit_cast(unsigned short, o[2 * k]) |
           ((unsigned)__builtin_bit_cast(unsigned short, o[2 * k + 1]) << 16);
  *reinterpret_cast<bn_u4*>(p) = w;
}

// end of a wide reduction block: fold the row slots through LDS in slot
// order, then one value per (block, column): slab row store or atomic.
// red holds slots x 2h = 4096 floats for every fast-path h.
__device__ __forceinline__ void bn_wide_combine(
    float* __restrict__ red, const float (&s)[8], const float (&q)[8],
    int slot, int slots, int c0, int h, float* __restrict__ out, int slab,
    bool nonempty) {
  const int w = 2 * h;
  float* row = red + slot * w;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    row[c0 + j] = s[j];
    row[h + c0 + j] = q[j];
  }
  __syncthreads();
  for (int col = threadIdx.x; col < w; col += 256) {
    float a = 0.f;
    for (int sl = 0; sl < slots; ++sl) a += red[sl * w + col];
    if (slab)
      out[(long)blockIdx.x * w + col] = a;
    else if (nonempty)
      atomicAdd(&out[col], a);
  }
}

// forward statistics.  U row groups are unrolled so that a lane has 128 B of
// loads in flight (U = 8 for bf16, 4 for fp32): 8 KiB per wave, 32 KiB per
// block.  kernel-resource-usage: 122 VGPRs (bf16; 68 fp32), 16 KiB LDS, no
// scratch -> occupancy 4 (7) waves/SIMD, so both blocks/CU of the default
// 512-block grid are resident and keep ~64 KiB of loads in flight per CU.
template <typename TS, int U>
__global__ __launch_bounds__(256) void bn_stats_wide_kernel(
    const TS* __restrict__ x, long n, int h, float* __restrict__ out,
    int slab) {
  __shared__ float red[4096];
  const int lpr = h >> 3;  // lanes per row
  const int slots = 256 / lpr;
  const int slot = threadIdx.x / lpr;
  const int c0 = (threadIdx.x - slot * lpr) * 8;
  const long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(n, r0 + rows_per_block);
  float s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;
  long r = r0 + slot;
  for (; r + (long)(U - 1) * slots < r1; r += (long)U * slots) {
    float v[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) bn_ld8(&x[(r + (long)u * slots) * h + c0], v[u]);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s[j] += v[u][j];
        q[j] += v[u][j] * v[u][j];
      }
  }
  for (; r < r1; r += slots) {
    float v[8];
    bn_ld8(&x[r * h + c0], v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      s[j] += v[j];
      q[j] += v[j] * v[j];
    }
  }
  bn_wide_combine(red, s, q, slot, slots, c0, h, out, slab, r0 < r1);
}

// backward partials.  MODE 0: no ReLU (neither y nor the mask is touched),
// 1: ReLU from y, 2: ReLU from the bit-packed mask.  U = 4 row groups for
// bf16 (2 for fp32): (g + x [+ y]) x 64 B per lane = 8-12 KiB per wave,
// 32-48 KiB per block.  kernel-resource-usage: 124 VGPRs without ReLU, 166
// with y or mask (bf16; 82-96 fp32), 16 KiB LDS, no scratch -> occupancy
// 4 / 3 (5) waves/SIMD, so both blocks/CU of the 512-block grid are resident
// and keep 64+ KiB of loads in flight per CU.
template <typename TS, int MODE, int U>
__global__ __launch_bounds__(256) void bn_bwd_partial_wide_kernel(
    const TS* __restrict__ g, const TS* __restrict__ x,
    const void* __restrict__ ym, const float* __restrict__ mean,
    const float* __restrict__ invstd, long n, int h, float* __restrict__ out,
    int slab, float keep_inv) {
  __shared__ float red[4096];
  const TS* y = (const TS*)ym;
  const unsigned char* mask = (const unsigned char*)ym;
  const int lpr = h >> 3;
  const int slots = 256 / lpr;
  const int slot = threadIdx.x / lpr;
  const int lane = threadIdx.x - slot * lpr;
  const int c0 = lane * 8;
  const long rows_per_block = (n + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = min(n, r0 + rows_per_block);
  float s[8], q[8], m[8], is[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    s[j] = q[j] = 0.f;
    m[j] = mean[c0 + j];
    is[j] = invstd[c0 + j];
  }
  auto acc = [&](const float (&gv)[8], const float (&xv)[8],
                 const float (&yv)[8], unsigned bits) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      bool dead = false;
      if (MODE == 1) dead = yv[j] <= 0.f;
      if (MODE == 2) dead = !((bits >> j) & 1u);
      const float gm = dead ? 0.f : gv[j] * keep_inv;
      s[j] += gm;
      q[j] += gm * (xv[j] - m[j]) * is[j];
    }
  };
  long r = r0 + slot;
  for (; r + (long)(U - 1) * slots < r1; r += (long)U * slots) {
    float gv[U][8], xv[U][8], yv[U][8];
    unsigned bits[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long rr = r + (long)u * slots;
      bn_ld8(&g[rr * h + c0], gv[u]);
      bn_ld8(&x[rr * h + c0], xv[u]);
      if (MODE == 1) bn_ld8(&y[rr * h + c0], yv[u]);
      bits[u] = (MODE == 2) ? mask[rr * lpr + lane] : 0u;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc(gv[u], xv[u], yv[u], bits[u]);
  }
  for (; r < r1; r += slots) {
    float gv[8], xv[8], yv[8];
    bn_ld8(&g[r * h + c0], gv);
    bn_ld8(&x[r * h + c0], xv);
    if (MODE == 1) bn_ld8(&y[r * h + c0], yv);
    const unsigned bits = (MODE == 2) ? mask[r * lpr + lane] : 0u;
    acc(gv, xv, yv, bits);
  }
  bn_wide_combine(red, s, q, slot, slots, c0, h, out, slab, r0 < r1);
}

__device__ __forceinline__ void bn_finalize_one(
    int c, float sum, float sumsq, float nf, float eps, float momentum,
    float* __restrict__ mean, float* __restrict__ invstd,
    float* __restrict__ running_mean, float* __restrict__ running_var) {
  // same math as bn_finalize_kernel (training: running stats always updated)
  const float m = sum / nf;
  const float var = fmaxf(sumsq / nf - m * m, 0.f);
  mean[c] = m;
  invstd[c] = rsqrtf(var + eps);
  const float unbiased = (nf > 1.f) ? var * nf / (nf - 1.f) : var;
  running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * m;
  running_var[c] = (1.f - momentum) * running_var[c] + momentum * unbiased;
}

// fixed-order fold of the slab rows of a wide reduction into partials[2h],
// with the per-channel epilogue of its direction fused in (no extra launch,
// no memset): EPI 1 = bn_finalize math, EPI 2 = dgamma/dbeta copy, EPI 3 =
// dgamma/dbeta added into gradient sinks.
// Block = 8 channels x {sum, sumsq} x 16 row slices; slices are folded in
// slice order, rows inside a slice in row order.
template <int EPI>
__global__ __launch_bounds__(256) void bn_slab_fold_kernel(
    const float* __restrict__ slab, int nb, int h,
    float* __restrict__ partials, long n, float eps, float momentum,
    float* __restrict__ o0, float* __restrict__ o1,
    float* __restrict__ running_mean, float* __restrict__ running_var) {
  __shared__ float red[16][16];
  __shared__ float tot[16];
  const int j = threadIdx.x & 15;
  const int sl = threadIdx.x >> 4;
  const int ch = blockIdx.x * 8 + (j & 7);
  const int col = (j >> 3) * h + ch;
  const int per = (nb + 15) / 16;
  const int b0 = sl * per;
  const int b1 = min(nb, b0 + per);
  float a = 0.f;
  if (ch < h) {
#pragma unroll 8
    for (int b = b0; b < b1; ++b) a += slab[(long)b * 2 * h + col];
  }
  red[sl][j] = a;
  __syncthreads();
  if (threadIdx.x < 16) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][threadIdx.x];
    tot[threadIdx.x] = t;
    if (ch < h) partials[col] = t;
  }
  if (EPI == 0) return;
  __syncthreads();
  if (threadIdx.x < 8 && ch < h) {
    if (EPI == 1) {
      bn_finalize_one(ch, tot[threadIdx.x], tot[8 + threadIdx.x], (float)n,
                      eps, momentum, o0, o1, running_mean, running_var);
    } else if (EPI == 2) {
      o0[ch] = tot[8 + threadIdx.x];  // dgamma = sum gm*xhat
      o1[ch] = tot[threadIdx.x];      // dbeta = sum gm
    } else {
      o0[ch] += tot[8 + threadIdx.x];
      o1[ch] += tot[threadIdx.x];
    }
  }
}

// wide forward statistics into partials[2h]; finalize != 0 also writes
// mean/invstd and updates the running stats (fused path, local count n).
// slab == nullptr selects the atomic combine.
template <typename TS>
static void bn_stats_wide_launch(const TS* x, long n, int h,
                                 float* partials, float* slab, bool finalize,
                                 float eps, float momentum, float* mean,
                                 float* invstd, float* running_mean,
                                 float* running_var, hipStream_t s) {
  const int nb = bn_wide_blocks(n);
  constexpr int U = 16 / sizeof(TS);
  if (slab) {
    bn_stats_wide_kernel<TS, U><<<nb, 256, 0, s>>>(x, n, h, slab, 1);
    if (finalize)
      bn_slab_fold_kernel<1><<<h / 8, 256, 0, s>>>(
          slab, nb, h, partials, n, eps, momentum, mean, invstd, running_mean,
          running_var);
    else
      bn_slab_fold_kernel<0><<<h / 8, 256, 0, s>>>(
          slab, nb, h, partials, n, 0.f, 0.f, nullptr, nullptr, nullptr,
          nullptr);
    return;
  }
  HIP_CHECK(hipMemsetAsync(partials, 0, 2 * h * sizeof(float), s));
  bn_stats_wide_kernel<TS, U><<<nb, 256, 0, s>>>(x, n, h, partials, 0);
  if (finalize)
    bn_finalize_kernel<<<ceil_div(h, 256), 256, 0, s>>>(
        partials, n, h, eps, momentum, mean, invstd, running_mean,
        running_var, 1);
}

// wide backward partials into partials[2h]; dgamma != nullptr also writes
// dgamma/dbeta (acc: adds them into gradient sinks).  mask (uint8 [n, h/8])
// takes precedence over y.
template <typename TS>
static void bn_bwd_partials_wide_launch(
    const TS* g, const TS* x, const TS* y,
    const unsigned char* mask, const float* mean, const float* invstd, long n,
    int h, bool relu, float* partials, float* slab, float* dgamma,
    float* dbeta, float keep_inv, hipStream_t s, bool acc = false) {
  const int nb = bn_wide_blocks(n);
  float* out = slab ? slab : partials;
  const int sl = slab ? 1 : 0;
  constexpr int U = 8 / sizeof(TS);
  if (!slab) HIP_CHECK(hipMemsetAsync(partials, 0, 2 * h * sizeof(float), s));
  if (!relu)
    bn_bwd_partial_wide_kernel<TS, 0, U><<<nb, 256, 0, s>>>(
        g, x, nullptr, mean, invstd, n, h, out, sl, keep_inv);
  else if (mask)
    bn_bwd_partial_wide_kernel<TS, 2, U><<<nb, 256, 0, s>>>(
        g, x, mask, mean, invstd, n, h, out, sl, keep_inv);
  else
    bn_bwd_partial_wide_kernel<TS, 1, U><<<nb, 256, 0, s>>>(
        g, x, y, mean, invstd, n, h, out, sl, keep_inv);
  if (slab) {
    if (dgamma && acc)
      bn_slab_fold_kernel<3><<<h / 8, 256, 0, s>>>(
          slab, nb, h, partials, n, 0.f, 0.f, dgamma, dbeta, nullptr,
          nullptr);
    else if (dgamma)
      bn_slab_fold_kernel<2><<<h / 8, 256, 0, s>>>(
          slab, nb, h, partials, n, 0.f, 0.f, dgamma, dbeta, nullptr,
          nullptr);
    else
      bn_slab_fold_kernel<0><<<h / 8, 256, 0, s>>>(
          slab, nb, h, partials, n, 0.f, 0.f, nullptr, nullptr, nullptr,
          nullptr);
  } else if (dgamma) {
    bn_grad_affine_kernel<<<ceil_div(h, 256), 256, 0, s>>>(
        partials, dgamma, dbeta, h, acc ? 1 : 0);
  }
}

// 8-wide training apply with ReLU for the fast-path shapes: one 16-B bf16
// load, one 16-B store and one mask byte per thread and step.  h divides
// 2048 = 8 x blockDim, so a thread keeps the same 8 channels over the whole
// grid-stride loop and the per-channel parameters stay in registers.
// DROP stays a template parameter (see bn_apply_kernel).
template <bool DROP>
__global__ __launch_bounds__(256) void bn_apply_mask_kernel(
    const __bf16* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, __bf16* __restrict__ y,
    unsigned char* __restrict__ mask, long n, int h, float dropout_p,
    const unsigned long long* __restrict__ seed_ptr) {
  const float keep_inv = DROP ? 1.f / (1.f - dropout_p) : 1.f;
  unsigned long long seed = 0ull;
  if constexpr (DROP) seed = seed_ptr ? *seed_ptr : 0ull;
  const long numo = n * (h >> 3);
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const int c = (int)((i0 * 8) % h);
  float mu[8], is[8], ga[8], be[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    mu[u] = mean[c + u];
    is[u] = invstd[c + u];
    ga[u] = gamma[c + u];
    be[u] = beta[c + u];
  }
  for (long o = i0; o < numo; o += stride) {
    const long t = o * 8;
    float xv[8];
    bn_ld8(&x[t], xv);
    __bf16 ov[8];
    unsigned bits = 0u;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float v = (xv[u] - mu[u]) * is[u] * ga[u] + be[u];
      v = fmaxf(v, 0.f);
      if constexpr (DROP)
        v = (bn_rand01(seed, t + u) >= dropout_p) ? v * keep_inv : 0.f;
      ov[u] = (__bf16)v;
      // the backward's `y <= 0` test on the stored value, NaNs included
      if (!((float)ov[u] <= 0.f)) bits |= 1u << u;
    }
    bn_st8(&y[t], ov);
    mask[o] = (unsigned char)bits;
  }
}

// 8-wide backward apply with ReLU for the fast-path shapes (same thread ->
// channel invariance as bn_apply_mask_kernel).  MODE 2 reads the keep mask
// (1 B per 8 elements) instead of y; MODE 1 reads bf16 y, so the two give
// bitwise-equal dx.
template <int MODE>
__global__ __launch_bounds__(256) void bn_bwd_apply_wide_kernel(
    const __bf16* __restrict__ g, const __bf16* __restrict__ x,
    const void* __restrict__ ym, const float* __restrict__ mean,
    const float* __restrict__ invstd, const float* __restrict__ gamma,
    const float* __restrict__ partials, __bf16* __restrict__ dx, long n,
    long count, int h, const float* __restrict__ count_ptr, float keep_inv) {
  const float invn = 1.f / (count_ptr ? *count_ptr : (float)count);
  const long numo = n * (h >> 3);
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const int c = (int)((i0 * 8) % h);
  float mu[8], is[8], ga[8], p0[8], p1[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    mu[u] = mean[c + u];
    is[u] = invstd[c + u];
    ga[u] = gamma[c + u];
    p0[u] = partials[c + u];
    p1[u] = partials[h + c + u];
  }
  for (long o = i0; o < numo; o += stride) {
    const long t = o * 8;
    float gv[8], xv[8];
    bn_ld8(&g[t], gv);
    bn_ld8(&x[t], xv);
    unsigned bits = 0u;
    if (MODE == 2) {
      bits = ((const unsigned char*)ym)[o];
    } else {
      float yv[8];
      bn_ld8((const __bf16*)ym + t, yv);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (!(yv[u] <= 0.f)) bits |= 1u << u;
    }
    __bf16 ov[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      ov[u] = bn_bwd_dx16(gv[u], xv[u], (bits >> u) & 1u, mu[u], is[u], ga[u],
                          p0[u], p1[u], invn, keep_inv);
    bn_st8(&dx[t], ov);
  }
}

static void bn_apply_mask_launch(const __bf16* x, const float* mean,
                                 const float* invstd, const float* gamma,
                                 const float* beta, __bf16* y,
                                 unsigned char* mask, long n, int h,
                                 float dropout_p,
                                 const unsigned long long* seed_ptr,
                                 hipStream_t s) {
  const int grid = grid_for(n * (h / 8));
  if (dropout_p > 0.f)
    bn_apply_mask_kernel<true><<<grid, 256, 0, s>>>(
        x, mean, invstd, gamma, beta, y, mask, n, h, dropout_p, seed_ptr);
  else
    bn_apply_mask_kernel<false><<<grid, 256, 0, s>>>(
        x, mean, invstd, gamma, beta, y, mask, n, h, 0.f, nullptr);
}

__global__ void bn_eval_stats_kernel(const float* __restrict__ rm,
                                     const float* __restrict__ rv,
                                     float* __restrict__ mean,
                                     float* __restrict__ invstd, int h,
                                     float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= h) return;
  mean[c] = rm[c];
  invstd[c] = rsqrtf(rv[c] + eps);
}

void launch_bn_eval_stats(const float* running_mean, const float* running_var,
                          float* mean, float* invstd, int h, float eps,
                          hipStream_t s) {
  bn_eval_stats_kernel<<<ceil_div(h, 256), 256, 0, s>>>(running_mean,
                                                        running_var, mean,
                                                        invstd, h, eps);
}

// --- BN launchers.  Each operation is one template over the activation
// dtype T: float (launch_bn_*) or __bf16 (launch_bn_*16, the act16 mode: x,
// y, the incoming grad g and dx are bf16; statistics, affine params and
// their grads stay fp32 — standard mixed-precision BN).  The keep mask and
// the 8-wide apply kernels exist for bf16 only.  The granular ones serve
// sync-BN: partials are all-reduced across ranks between the stats and apply
// phases, and `count_ptr` holds the GLOBAL row count. ---

// slab: [bn_wide_slab_rows(n, h), 2h] per-call scratch (nullptr when that
// returns 0) — same convention for every reduction launcher below
template <typename T>
static void bn_stats_only(const T* x, long n, int h, float* partials,
                          float* slab, hipStream_t s) {
  if (n == 0) {
    HIP_CHECK(hipMemsetAsync(partials, 0, 2 * h * sizeof(float), s));
    return;
  }
  if (bn_wide_ok(h)) {
    bn_stats_wide_launch(x, n, h, partials, slab, false, 0.f, 0.f, nullptr,
                         nullptr, nullptr, nullptr, s);
    return;
  }
  bn_stats_dispatch(x, n, h, partials, s);
}

// the element-wise forward over [n, h], n > 0; a mask selects the 8-wide
// kernel that also writes it
template <typename T>
static void bn_apply_launch(const T* x, const float* mean, const float* invstd,
                            const float* gamma, const float* beta, T* y,
                            unsigned char* mask, long n, int h, bool training,
                            bool relu, float dropout_p,
                            const unsigned long long* seed_ptr,
                            hipStream_t s) {
  if constexpr (std::is_same_v<T, __bf16>) {
    if (mask) {
      bn_apply_mask_launch(x, mean, invstd, gamma, beta, y, mask, n, h,
                           dropout_p, seed_ptr, s);
      return;
    }
  }
  if (training && dropout_p > 0.f)
    bn_apply_kernel<T, T, true><<<grid_for(n * h), 256, 0, s>>>(
        x, mean, invstd, gamma, beta, y, n, h, relu ? 1 : 0, dropout_p,
        seed_ptr);
  else
    bn_apply_kernel<T, T, false><<<grid_for(n * h), 256, 0, s>>>(
        x, mean, invstd, gamma, beta, y, n, h, relu ? 1 : 0);
}

template <typename T>
static void bn_fwd(const T* x, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float* mean,
                   float* invstd, float* partials, T* y, long n, int h,
                   float momentum, float eps, bool training, bool relu,
                   float dropout_p, const unsigned long long* seed_ptr,
                   float* slab, unsigned char* mask, hipStream_t s) {
  if (n == 0) return;
  if (training && bn_wide_ok(h)) {
    bn_stats_wide_launch(x, n, h, partials, slab, true, eps, momentum, mean,
                         invstd, running_mean, running_var, s);
  } else if (training) {
    bn_stats_dispatch(x, n, h, partials, s);
    bn_finalize_kernel<<<ceil_div(h, 256), 256, 0, s>>>(
        partials, n, h, eps, momentum, mean, invstd, running_mean, running_var,
        1);
  } else {
    launch_bn_eval_stats(running_mean, running_var, mean, invstd, h, eps, s);
  }
  bn_apply_launch(x, mean, invstd, gamma, beta, y, mask, n, h, training, relu,
                  dropout_p, seed_ptr, s);
}

template <typename T>
static void bn_finalize_apply(const T* x, const float* partials,
                              const float* count_ptr, const float* gamma,
                              const float* beta, float* running_mean,
                              float* running_var, float* mean, float* invstd,
                              T* y, long n, int h, float momentum, float eps,
                              bool training, bool relu, float dropout_p,
                              const unsigned long long* seed_ptr,
                              unsigned char* mask, hipStream_t s) {
  if (training) {
    bn_finalize_kernel<<<ceil_div(h, 256), 256, 0, s>>>(
        partials, n, h, eps, momentum, mean, invstd, running_mean,
        running_var, 1, count_ptr);
  } else {
    bn_eval_stats_kernel<<<ceil_div(h, 256), 256, 0, s>>>(
        running_mean, running_var, mean, invstd, h, eps);
  }
  if (n > 0)
    bn_apply_launch(x, mean, invstd, gamma, beta, y, mask, n, h, training,
                    relu, dropout_p, seed_ptr, s);
}

template <typename T>
static void bn_bwd_partials_only(const T* g, const T* x, const T* y,
                                 const float* mean, const float* invstd,
                                 long n, int h, bool relu, float* partials,
                                 float keep_inv, float* slab,
                                 const unsigned char* mask, hipStream_t s) {
  if (n == 0) {
    HIP_CHECK(hipMemsetAsync(partials, 0, 2 * h * sizeof(float), s));
    return;
  }
  if (bn_wide_ok(h)) {
    bn_bwd_partials_wide_launch(g, x, y, mask, mean, invstd, n, h, relu,
                                partials, slab, nullptr, nullptr, keep_inv, s);
    return;
  }
  bn_bwd_partials_dispatch(g, x, y, mean, invstd, n, h, relu, partials,
                           keep_inv, s);
}

// the element-wise backward over [n, h], n > 0 (count_ptr null: count is n)
template <typename T>
static void bn_bwd_apply_launch(const T* g, const T* x, const T* y,
                                const float* mean, const float* invstd,
                                const float* gamma, const float* partials,
                                const float* count_ptr, T* dx, long n, int h,
                                bool relu, float keep_inv,
                                const unsigned char* mask, hipStream_t s) {
  if constexpr (std::is_same_v<T, __bf16>) {
    if (relu && bn_wide_ok(h)) {
      if (mask)
        bn_bwd_apply_wide_kernel<2><<<grid_for(n * (h / 8)), 256, 0, s>>>(
            g, x, mask, mean, invstd, gamma, partials, dx, n, n, h, count_ptr,
            keep_inv);
      else
        bn_bwd_apply_wide_kernel<1><<<grid_for(n * (h / 8)), 256, 0, s>>>(
            g, x, y, mean, invstd, gamma, partials, dx, n, n, h, count_ptr,
            keep_inv);
      return;
    }
  }
  bn_bwd_apply_kernel<<<grid_for(n * h), 256, 0, s>>>(
      g, x, y, mean, invstd, gamma, partials, dx, n, n, h, relu ? 1 : 0,
      count_ptr, keep_inv);
}

template <typename T>
static void bn_bwd(const T* g, const T* x, const T* y, const float* mean,
                   const float* invstd, const float* gamma, float* partials,
                   T* dx, float* dgamma, float* dbeta, long n, int h,
                   bool relu, float keep_inv, float* slab,
                   const unsigned char* mask, hipStream_t s, bool acc) {
  if (n == 0) return;
  const bool wide = bn_wide_ok(h);
  if (wide)
    bn_bwd_partials_wide_launch(g, x, y, mask, mean, invstd, n, h, relu,
                                partials, slab, dgamma, dbeta, keep_inv, s,
                                acc);
  else
    bn_bwd_partials_dispatch(g, x, y, mean, invstd, n, h, relu, partials,
                             keep_inv, s);
  bn_bwd_apply_launch(g, x, y, mean, invstd, gamma, partials, nullptr, dx, n,
                      h, relu, keep_inv, mask, s);
  if (wide) return;  // dgamma/dbeta written with the partials
  bn_grad_affine_kernel<<<ceil_div(h, 256), 256, 0, s>>>(
      partials, dgamma, dbeta, h, acc ? 1 : 0);
}

// --- the extern names (launchers.h): fp32 has no keep mask ---

void launch_bn_stats_only(const float* x, long n, int h, float* partials,
                          float* slab, hipStream_t s) {
  bn_stats_only(x, n, h, partials, slab, s);
}
void launch_bn_stats_only16(const void* x, long n, int h, float* partials,
                            float* slab, hipStream_t s) {
  bn_stats_only((const __bf16*)x, n, h, partials, slab, s);
}

void launch_bn_fwd(const float* x, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float* mean,
                   float* invstd, float* partials, float* y, long n, int h,
                   float momentum, float eps, bool training, bool relu,
                   float dropout_p, const unsigned long long* seed_ptr,
                   float* slab, hipStream_t s) {
  bn_fwd(x, gamma, beta, running_mean, running_var, mean, invstd, partials, y,
         n, h, momentum, eps, training, relu, dropout_p, seed_ptr, slab,
         nullptr, s);
}
void launch_bn_fwd16(const void* x, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, float* mean,
                     float* invstd, float* partials, void* y, long n, int h,
                     float momentum, float eps, bool training, bool relu,
                     float dropout_p, const unsigned long long* seed_ptr,
                     float* slab, unsigned char* mask, hipStream_t s) {
  bn_fwd((const __bf16*)x, gamma, beta, running_mean, running_var, mean,
         invstd, partials, (__bf16*)y, n, h, momentum, eps, training, relu,
         dropout_p, seed_ptr, slab, mask, s);
}

void launch_bn_finalize_apply(const float* x, const float* partials,
                              const float* count_ptr, const float* gamma,
                              const float* beta, float* running_mean,
                              float* running_var, float* mean, float* invstd,
                              float* y, long n, int h, float momentum,
                              float eps, bool training, bool relu,
                              float dropout_p,
                              const unsigned long long* seed_ptr,
                              hipStream_t s) {
  bn_finalize_apply(x, partials, count_ptr, gamma, beta, running_mean,
                    running_var, mean, invstd, y, n, h, momentum, eps,
                    training, relu, dropout_p, seed_ptr, nullptr, s);
}
void launch_bn_finalize_apply16(const void* x, const float* partials,
                                const float* count_ptr, const float* gamma,
                                const float* beta, float* running_mean,
                                float* running_var, float* mean, float* invstd,
                                void* y, long n, int h, float momentum,
                                float eps, bool training, bool relu,
                                float dropout_p,
                                const unsigned long long* seed_ptr,
                                unsigned char* mask, hipStream_t s) {
  bn_finalize_apply((const __bf16*)x, partials, count_ptr, gamma, beta,
                    running_mean, running_var, mean, invstd, (__bf16*)y, n, h,
                    momentum, eps, training, relu, dropout_p, seed_ptr, mask,
                    s);
}

void launch_bn_bwd_partials_only(const float* g, const float* x,
                                 const float* y, const float* mean,
                                 const float* invstd, long n, int h, bool relu,
                                 float* partials, float keep_inv,
                                 float* slab, hipStream_t s) {
  bn_bwd_partials_only(g, x, y, mean, invstd, n, h, relu, partials, keep_inv,
                       slab, nullptr, s);
}
void launch_bn_bwd_partials_only16(const void* g, const void* x,
                                   const void* y, const float* mean,
                                   const float* invstd, long n, int h,
                                   bool relu, float* partials, float keep_inv,
                                   float* slab, const unsigned char* mask,
                                   hipStream_t s) {
  bn_bwd_partials_only((const __bf16*)g, (const __bf16*)x, (const __bf16*)y,
                       mean, invstd, n, h, relu, partials, keep_inv, slab,
                       mask, s);
}

// first half of launch_bn_bwd16 on the keep-mask path (training forward with
// ReLU on a fast-path shape): partials[2h] plus dgamma/dbeta, no dx — the
// attention backward applies the element-wise part itself
void launch_bn_bwd_partials_affine16(const void* g, const void* x,
                                     const unsigned char* mask,
                                     const float* mean, const float* invstd,
                                     long n, int h, float* partials,
                                     float keep_inv, float* slab,
                                     float* dgamma, float* dbeta,
                                     hipStream_t s, bool acc) {
  if (n <= 0 || !mask || !bn_wide_ok(h))
    pertgnn_shape_fail("bn_bwd_partials_affine16", "h", h);
  bn_bwd_partials_wide_launch((const __bf16*)g, (const __bf16*)x,
                              (const __bf16*)nullptr, mask, mean, invstd, n,
                              h, true, partials, slab, dgamma, dbeta,
                              keep_inv, s, acc);
}

void launch_bn_bwd_apply_only(const float* g, const float* x, const float* y,
                              const float* mean, const float* invstd,
                              const float* gamma, const float* partials,
                              const float* count_ptr, float* dx, long n, int h,
                              bool relu, float keep_inv, hipStream_t s) {
  if (n == 0) return;
  bn_bwd_apply_launch(g, x, y, mean, invstd, gamma, partials, count_ptr, dx, n,
                      h, relu, keep_inv, nullptr, s);
}
void launch_bn_bwd_apply_only16(const void* g, const void* x, const void* y,
                                const float* mean, const float* invstd,
                                const float* gamma, const float* partials,
                                const float* count_ptr, void* dx, long n,
                                int h, bool relu, float keep_inv,
                                const unsigned char* mask, hipStream_t s) {
  if (n == 0) return;
  bn_bwd_apply_launch((const __bf16*)g, (const __bf16*)x, (const __bf16*)y,
                      mean, invstd, gamma, partials, count_ptr, (__bf16*)dx, n,
                      h, relu, keep_inv, mask, s);
}

void launch_bn_grad_affine(const float* partials, float* dgamma, float* dbeta,
                           int h, hipStream_t s, bool acc) {
  bn_grad_affine_kernel<<<ceil_div(h, 256), 256, 0, s>>>(
      partials, dgamma, dbeta, h, acc ? 1 : 0);
}

void launch_counter_bump(unsigned long long* c, hipStream_t s) {
  counter_bump_kernel<<<1, 1, 0, s>>>(c);
}

void launch_bn_bwd(const float* g, const float* x, const float* y,
                   const float* mean, const float* invstd, const float* gamma,
                   float* partials, float* dx, float* dgamma, float* dbeta,
                   long n, int h, bool relu, float keep_inv, float* slab,
                   hipStream_t s, bool acc) {
  bn_bwd(g, x, y, mean, invstd, gamma, partials, dx, dgamma, dbeta, n, h, relu,
         keep_inv, slab, nullptr, s, acc);
}
void launch_bn_bwd16(const void* g, const void* x, const void* y,
                     const float* mean, const float* invstd,
                     const float* gamma, float* partials, void* dx,
                     float* dgamma, float* dbeta, long n, int h, bool relu,
                     float keep_inv, float* slab, const unsigned char* mask,
                     hipStream_t s, bool acc) {
  bn_bwd((const __bf16*)g, (const __bf16*)x, (const __bf16*)y, mean, invstd,
         gamma, partials, (__bf16*)dx, dgamma, dbeta, n, h, relu, keep_inv,
         slab, mask, s, acc);
}

// ---------------------------------------------------------------------------
// quantile loss + eval metrics
// ---------------------------------------------------------------------------

__global__ void quantile_loss_fwd_kernel(const float* __restrict__ y,
                                         const float* __restrict__ y_hat,
                                         float* __restrict__ out, long b,
                                         float tau) {
  __shared__ float smem[256];
  float acc = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < b;
       i += (long)gridDim.x * blockDim.x) {
    const float e = y[i] - y_hat[i];
    acc += fmaxf(tau * e, (tau - 1.f) * e);
  }
  smem[threadIdx.x] = acc;
  __syncthreads();
  for (int off = blockDim.x / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off) smem[threadIdx.x] += smem[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out, smem[0] / b);
}

__global__ void quantile_loss_bwd_kernel(const float* __restrict__ g,
                                         const float* __restrict__ y,
                                         const float* __restrict__ y_hat,
                                         float* __restrict__ dy_hat, long b,
                                         float tau) {
  const float gs = g[0] / b;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < b;
       i += (long)gridDim.x * blockDim.x) {
    const float e = y[i] - y_hat[i];
    float d;
    if (e > 0.f) d = -tau;
    else if (e < 0.f) d = 1.f - tau;
    else d = 0.5f * (-tau) + 0.5f * (1.f - tau);  // torch.maximum tie split
    dy_hat[i] = gs * d;
  }
}

__global__ void eval_metrics_kernel(const float* __restrict__ y,
                                    const float* __restrict__ y_hat,
                                    float* __restrict__ out3, long b,
                                    float tau) {
  __shared__ float smem[3][256];
  float mae = 0.f, mape = 0.f, q = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < b;
       i += (long)gridDim.x * blockDim.x) {
    const float err = y_hat[i] - y[i];
    const float a = fabsf(err);
    mae += a;
    mape += a / y[i];
    const float e = -err;
    q += fmaxf(tau * e, (tau - 1.f) * e);
  }
  smem[0][threadIdx.x] = mae;
  smem[1][threadIdx.x] = mape;
  smem[2][threadIdx.x] = q;
  __syncthreads();
  for (int off = blockDim.x / 2; off > 0; off >>= 1) {
    if (threadIdx.x < off)
      for (int k = 0; k < 3; ++k)
        smem[k][threadIdx.x] += smem[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; ++k) atomicAdd(&out3[k], smem[k][0]);
}

void launch_quantile_loss_fwd(const float* y, const float* y_hat, float* out,
                              long b, float tau, hipStream_t s) {
  if (b == 0) {
    // mean over no elements: NaN (all-ones is a quiet NaN), nothing launched
    HIP_CHECK(hipMemsetAsync(out, 0xFF, sizeof(float), s));
    return;
  }
  HIP_CHECK(hipMemsetAsync(out, 0, sizeof(float), s));
  quantile_loss_fwd_kernel<<<grid_for(b, 256, 256), 256, 0, s>>>(y, y_hat, out,
                                                                 b, tau);
}
void launch_quantile_loss_bwd(const float* g, const float* y,
                              const float* y_hat, float* dy_hat, long b,
                              float tau, hipStream_t s) {
  if (b == 0) return;
  quantile_loss_bwd_kernel<<<grid_for(b), 256, 0, s>>>(g, y, y_hat, dy_hat, b,
                                                       tau);
}
void launch_eval_metrics(const float* y, const float* y_hat, float* out3,
                         long b, float tau, hipStream_t s) {
  HIP_CHECK(hipMemsetAsync(out3, 0, 3 * sizeof(float), s));
  if (b == 0) return;  // empty sums: three zeros
  eval_metrics_kernel<<<grid_for(b, 256, 256), 256, 0, s>>>(y, y_hat, out3, b,
                                                            tau);
}

// ---------------------------------------------------------------------------
// Adam on flat master buffers (torch.optim.Adam math, K14)
// ---------------------------------------------------------------------------

// step/bias state lives ON DEVICE (state[0]=step, state[1]=1-b1^t,
// state[2]=1-b2^t) so the whole Adam update is hipGraph-replayable: each
// replay increments the step and recomputes the bias corrections.
// sstate (dynamic loss scaling, all device-resident so the whole step is
// hipGraph-replayable with the scale evolving across replays):
//   sstate[0] = current scale, sstate[1] = clean-step counter,
//   sstate[2] = found_inf flag for THIS step.
// A skipped step (non-finite grads) advances neither the Adam moments nor
// the bias-correction counter — torch.cuda.amp.GradScaler semantics.
__global__ void adam_tick_kernel(float* __restrict__ state, float b1,
                                 float b2,
                                 const float* __restrict__ sstate = nullptr) {
  if (sstate && sstate[2] != 0.f) return;  // skipped step
  const float t = state[0] + 1.f;
  state[0] = t;
  state[1] = 1.f - powf(b1, t);
  state[2] = 1.f - powf(b2, t);
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                            float* __restrict__ m, float* __restrict__ v,
                            const float* __restrict__ state, long numel,
                            float lr, float b1, float b2, float eps,
                            float gscale,
                            const float* __restrict__ sstate = nullptr) {
  if (sstate && sstate[2] != 0.f) return;  // skipped step
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const float step_size = lr / state[1];
  const float sqrt_bias2 = sqrtf(state[2]);
  const float gs = sstate ? 1.f / sstate[0] : gscale;
  for (long t = i0; t < numel; t += stride) {
    const float gt = g[t] * gs;  // loss-scaling unscale
    const float mt = b1 * m[t] + (1.f - b1) * gt;
    const float vt = b2 * v[t] + (1.f - b2) * gt * gt;
    m[t] = mt;
    v[t] = vt;
    const float denom = sqrtf(vt) / sqrt_bias2 + eps;
    p[t] -= step_size * mt / denom;
  }
}

__global__ void scaler_begin_kernel(float* __restrict__ sstate) {
  sstate[2] = 0.f;
}

__global__ void grad_scan_kernel(const float* __restrict__ g, long numel,
                                 float* __restrict__ sstate) {
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  float bad = 0.f;
  for (long t = i0; t < numel; t += stride) {
    const float x = g[t];
    if (!isfinite(x)) { bad = 1.f; break; }
  }
  if (bad != 0.f) sstate[2] = 1.f;  // benign race: every writer stores 1
}

__global__ void scaler_update_kernel(float* __restrict__ sstate, float backoff,
                                     float growth, float interval) {
  if (sstate[2] != 0.f) {
    sstate[0] = fmaxf(sstate[0] * backoff, 1.f);
    sstate[1] = 0.f;
  } else {
    sstate[1] += 1.f;
    if (sstate[1] >= interval) {
      sstate[0] = fminf(sstate[0] * growth, 4294967296.f);
      sstate[1] = 0.f;
    }
  }
}

void launch_adam(float* p, const float* g, float* m, float* v, float* state,
                 long numel, float lr, float b1, float b2, float eps, float gscale,
                 hipStream_t s) {
  if (numel == 0) return;
  adam_tick_kernel<<<1, 1, 0, s>>>(state, b1, b2, nullptr);
  adam_kernel<<<grid_for(numel), 256, 0, s>>>(p, g, m, v, state, numel, lr,
                                              b1, b2, eps, gscale, nullptr);
}

void launch_adam_dynamic(float* p, const float* g, float* m, float* v,
                         float* state, float* sstate, long numel, float lr,
                         float b1, float b2, float eps, float backoff,
                         float growth, float interval, hipStream_t s) {
  if (numel == 0) return;
  scaler_begin_kernel<<<1, 1, 0, s>>>(sstate);
  grad_scan_kernel<<<grid_for(numel), 256, 0, s>>>(g, numel, sstate);
  adam_tick_kernel<<<1, 1, 0, s>>>(state, b1, b2, sstate);
  adam_kernel<<<grid_for(numel), 256, 0, s>>>(p, g, m, v, state, numel, lr,
                                              b1, b2, eps, 1.f, sstate);
  scaler_update_kernel<<<1, 1, 0, s>>>(sstate, backoff, growth, interval);
}

// ---------------------------------------------------------------------------
// Extended Adam: global-norm clipping, decoupled weight decay and a learning-
// rate table, all driven from device state so a captured step replays with
// the rate and the clip coefficient evolving.  The plain path above is left
// alone; this one is taken only when one of the three is on.
//   hstate[0] = learning rate of this step
//   hstate[1] = clip coefficient of this step (1 when clipping is off)
//   hstate[2] = gradient norm of this step
//   hstate[3] = sum of the norms over applied steps since the last reset
//   hstate[4] = maximum norm since the last reset
//   hstate[5] = number of clipped steps (coefficient < 1)
//   hstate[6] = number of applied steps
//   hstate[7] = spare
// The norm is a two-level fixed-order reduction (per lane, wave, LDS, then
// one block over the per-block slab in fp64): no atomics, no memset, and the
// same bits on every run.
// ---------------------------------------------------------------------------

// slab[blockIdx.x] = sum of (g[i] * gs)^2 over this block's grid-stride share.
// g is split by the launcher into `head` scalars up to the first 16-byte
// boundary, `nvec` float4 and `tail` scalars, so any 4-byte-aligned pointer
// and any numel work; head and tail (at most 3 each) go to the first lanes
// of block 0.
__global__ void grad_sumsq_partial_kernel(const float* __restrict__ g,
                                          int head, long nvec, int tail,
                                          float gscale,
                                          const float* __restrict__ sstate,
                                          float* __restrict__ slab) {
  __shared__ float wsum[4];
  const float gs = sstate ? 1.f / sstate[0] : gscale;
  const float4* __restrict__ g4 = (const float4*)(g + head);
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (long t = i0; t < nvec; t += stride) {
    const float4 x = g4[t];
    const float a = x.x * gs, b = x.y * gs, c = x.z * gs, d = x.w * gs;
    acc += a * a;
    acc += b * b;
    acc += c * c;
    acc += d * d;
  }
  if (i0 < head) {
    const float a = g[i0] * gs;
    acc += a * a;
  }
  if (i0 < tail) {
    const float a = g[head + 4 * nvec + i0] * gs;
    acc += a * a;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    slab[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// One block: folds the slab in fp64 in a fixed order, then writes the norm,
// torch.nn.utils.clip_grad_norm_'s coefficient and the running statistics.
// A skipped step of the dynamic scaler leaves hstate untouched.
__global__ void grad_norm_fold_kernel(const float* __restrict__ slab, int n,
                                      float max_norm,
                                      const float* __restrict__ sstate,
                                      float* __restrict__ hstate) {
  __shared__ double part[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += (double)slab[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (sstate && sstate[2] != 0.f) return;  // skipped step
  const float norm = (float)sqrt(part[0]);
  float coef = 1.f;
  if (!isinf(max_norm)) {
    const float c = max_norm / (norm + 1e-6f);
    coef = c > 1.f ? 1.f : c;  // a NaN norm stays NaN, as torch's clamp does
  }
  hstate[1] = coef;
  hstate[2] = norm;
  hstate[3] += norm;
  hstate[4] = fmaxf(hstate[4], norm);
  if (coef < 1.f) hstate[5] += 1.f;
  hstate[6] += 1.f;
}

// adam_tick_kernel, and the learning rate of the new step t into hstate[0]:
// lr_table[min(t, T) - 1] with a table, the by-value lr without one.
__global__ void adam_tick_ex_kernel(float* __restrict__ state, float b1,
                                    float b2, const float* __restrict__ sstate,
                                    float* __restrict__ hstate,
                                    const float* __restrict__ lr_table,
                                    long table_len, float lr) {
  if (sstate && sstate[2] != 0.f) return;  // skipped step
  const float t = state[0] + 1.f;
  state[0] = t;
  state[1] = 1.f - powf(b1, t);
  state[2] = 1.f - powf(b2, t);
  if (lr_table) {
    const long k = (long)t < table_len ? (long)t : table_len;
    lr = lr_table[k - 1];
  }
  hstate[0] = lr;
}

// adam_kernel's expressions with lr and the clip coefficient read from
// hstate and torch.optim.AdamW's decoupled decay, p *= 1 - lr * wd, before
// the moment update wherever decay_mask is set (null when wd == 0).
__global__ void adam_ex_kernel(float* __restrict__ p,
                               const float* __restrict__ g,
                               float* __restrict__ m, float* __restrict__ v,
                               const float* __restrict__ state,
                               const float* __restrict__ hstate,
                               const unsigned char* __restrict__ decay_mask,
                               long numel, float b1, float b2, float eps,
                               float gscale, float wd,
                               const float* __restrict__ sstate) {
  if (sstate && sstate[2] != 0.f) return;  // skipped step
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  const float lr = hstate[0];
  const float coef = hstate[1];
  const float step_size = lr / state[1];
  const float sqrt_bias2 = sqrtf(state[2]);
  const float gs = sstate ? 1.f / sstate[0] : gscale;
  const float keep = 1.f - lr * wd;
  for (long t = i0; t < numel; t += stride) {
    const float gt = (g[t] * gs) * coef;  // unscale, then clip
    float pt = p[t];
    // rounded on its own, so the update below is adam_kernel's to the bit
    if (decay_mask && decay_mask[t]) pt = __fmul_rn(pt, keep);
    const float mt = b1 * m[t] + (1.f - b1) * gt;
    const float vt = b2 * v[t] + (1.f - b2) * gt * gt;
    m[t] = mt;
    v[t] = vt;
    const float denom = sqrtf(vt) / sqrt_bias2 + eps;
    p[t] = pt - step_size * mt / denom;
  }
}

// sstate null: static scaling by gscale; otherwise the dynamic scaler's
// begin / scan / update kernels wrap the step exactly as in
// launch_adam_dynamic.  slab holds slab_len >= 1 floats; the partial grid
// never exceeds it.  Everything is a launch on s: no host read, no copy.
void launch_adam_ex(float* p, const float* g, float* m, float* v,
                    float* state, float* sstate, float* hstate, float* slab,
                    int slab_len, const unsigned char* decay_mask,
                    const float* lr_table, long table_len, long numel,
                    float lr, float b1, float b2, float eps, float gscale,
                    float wd, float max_norm, float backoff, float growth,
                    float interval, hipStream_t s) {
  if (numel == 0) return;
  if (sstate) {
    scaler_begin_kernel<<<1, 1, 0, s>>>(sstate);
    grad_scan_kernel<<<grid_for(numel), 256, 0, s>>>(g, numel, sstate);
  }
  const long mis = (long)(((uintptr_t)g & 15) / 4);
  const int head = (int)min((4 - mis) & 3, numel);
  const long nvec = (numel - head) / 4;
  const int tail = (int)(numel - head - 4 * nvec);
  const int grid = min(max(grid_for(nvec), 1), slab_len);
  grad_sumsq_partial_kernel<<<grid, 256, 0, s>>>(g, head, nvec, tail, gscale,
                                                 sstate, slab);
  grad_norm_fold_kernel<<<1, 256, 0, s>>>(slab, grid, max_norm, sstate,
                                          hstate);
  adam_tick_ex_kernel<<<1, 1, 0, s>>>(state, b1, b2, sstate, hstate, lr_table,
                                      table_len, lr);
  adam_ex_kernel<<<grid_for(numel), 256, 0, s>>>(p, g, m, v, state, hstate,
                                                 decay_mask, numel, b1, b2,
                                                 eps, sstate ? 1.f : gscale,
                                                 wd, sstate);
  if (sstate)
    scaler_update_kernel<<<1, 1, 0, s>>>(sstate, backoff, growth, interval);
}
