// Fused CSR edge-attention kernels (gfx950) — the graph-transformer hot path.
//
// Implements PyG-TransformerConv heads=1 semantics (reference model.py:25-52,
// SURVEY.md kernels K3-K6 + their backward K15) as a single fused forward
// kernel and a 3-stage backward, with NO atomics anywhere: the forward
// reduces per destination row (one wave per row over its CSR edge segment,
// online softmax in registers), the backward scatters per-edge gradients and
// segment-sums them per SOURCE row over the CSC permutation — deterministic
// by construction.
//
// Layouts: q,k,v,skip,out: [N,H] f32 row-major; e: [E,H] f32 in CSR (dst-
// sorted) edge order; row_ptr [N+1] / csr_src [E] / col_ptr [N+1] / csc_dst
// [E] / csc_eid [E] int32.  One wave (64 lanes) owns one row; lane l covers
// columns l, l+64, ..., so all global accesses are coalesced.  H <= 512
// (VPT = ceil(H/64) <= 8 register slots per lane).

#include "common.h"
#include "launchers.h"
#include <cmath>

#define WAVES_PER_BLOCK 4

template <int VPT>
__global__ void edge_attn_fwd_kernel(
    const float* __restrict__ q, const float* __restrict__ k,
    const float* __restrict__ v, const float* __restrict__ e,
    const int* __restrict__ row_ptr, const int* __restrict__ csr_src,
    const float* __restrict__ skip, float* __restrict__ out,
    float* __restrict__ alpha, int n, int h, float scale) {
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int row = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (row >= n) return;

  float qr[VPT], acc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = lane + j * PERTGNN_WAVE;
    qr[j] = (c < h) ? q[(long)row * h + c] : 0.f;
    acc[j] = 0.f;
  }

  const int beg = row_ptr[row], end = row_ptr[row + 1];
  float m = -INFINITY, s = 0.f;
  for (int p = beg; p < end; ++p) {
    const long src = csr_src[p];
    float part = 0.f;
    float ke[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = lane + j * PERTGNN_WAVE;
      if (c < h) {
        ke[j] = k[src * h + c] + e[(long)p * h + c];
        part += qr[j] * ke[j];
      }
    }
    const float logit = wave_reduce_sum(part) * scale;
    // stash the raw logit from the SAME lane that re-reads it in the
    // finalize sweep below (same-thread store->load, well-defined)
    if (lane == (p - beg) % PERTGNN_WAVE) alpha[p] = logit;
    const float m_new = fmaxf(m, logit);
    const float corr = __expf(m - m_new);  // 0 on first edge (m = -inf)
    const float pexp = __expf(logit - m_new);
    s = s * corr + pexp;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = lane + j * PERTGNN_WAVE;
      if (c < h) {
        const float ve = v[src * h + c] + e[(long)p * h + c];
        acc[j] = acc[j] * corr + pexp * ve;
      }
    }
    m = m_new;
  }

  const float inv_s = (s > 0.f) ? 1.f / s : 0.f;
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = lane + j * PERTGNN_WAVE;
    if (c < h) {
      const float sk = skip ? skip[(long)row * h + c] : 0.f;
      out[(long)row * h + c] = acc[j] * inv_s + sk;
    }
  }
  // finalize alpha[p] = exp(logit - m) / s, lanes parallel over the segment
  for (int p = beg + lane; p < end; p += PERTGNN_WAVE)
    alpha[p] = __expf(alpha[p] - m) * inv_s;
}

// backward stage 1 (per dst row): dlogit, dq, per-edge de_k / de_v
template <int VPT>
__global__ void edge_attn_bwd_row_kernel(
    const float* __restrict__ g, const float* __restrict__ q,
    const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ e, const float* __restrict__ alpha,
    const int* __restrict__ row_ptr, const int* __restrict__ csr_src,
    float* __restrict__ dq, float* __restrict__ dek, float* __restrict__ dev,
    int n, int h, float scale) {
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int row = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (row >= n) return;

  float gr[VPT], qr[VPT], dqacc[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = lane + j * PERTGNN_WAVE;
    gr[j] = (c < h) ? g[(long)row * h + c] : 0.f;
    qr[j] = (c < h) ? q[(long)row * h + c] : 0.f;
    dqacc[j] = 0.f;
  }

  const int beg = row_ptr[row], end = row_ptr[row + 1];
  // pass 1: dalpha_p = <g_row, v_src+e_p>; sdot = sum alpha_p * dalpha_p.
  // dalpha is stashed in dek[p*h] scratch column 0 then overwritten in pass 2?
  // No: a second sweep recomputes it — instead we keep it in dev row 0 is also
  // needed; use a per-wave local sweep with recompute-free design: store
  // dalpha into dek[p*h + 0..] later; simplest correct form: recompute.
  float sdot = 0.f;
  for (int p = beg; p < end; ++p) {
    const long src = csr_src[p];
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = lane + j * PERTGNN_WAVE;
      if (c < h) part += gr[j] * (v[src * h + c] + e[(long)p * h + c]);
    }
    const float dalpha = wave_reduce_sum(part);
    sdot += alpha[p] * dalpha;
    // stash dalpha in dev[p][0] slot via lane 0 (dev fully overwritten pass 2)
    if (lane == 0) dev[(long)p * h] = dalpha;
  }
  // pass 2
  for (int p = beg; p < end; ++p) {
    const long src = csr_src[p];
    // lane 0 stashed dalpha in pass 1; only lane 0 re-reads its own store
    // (same-thread dependency, well-defined) and broadcasts it.
    const float dalpha_l0 = (lane == 0) ? dev[(long)p * h] : 0.f;
    const float dalpha = __shfl(dalpha_l0, 0, PERTGNN_WAVE);
    const float a = alpha[p];
    const float dl = a * (dalpha - sdot) * scale;  // includes 1/sqrt(h)
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = lane + j * PERTGNN_WAVE;
      if (c < h) {
        const float kec = k[src * h + c] + e[(long)p * h + c];
        dqacc[j] += dl * kec;
        dek[(long)p * h + c] = dl * qr[j];
        dev[(long)p * h + c] = a * gr[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = lane + j * PERTGNN_WAVE;
    if (c < h) dq[(long)row * h + c] = dqacc[j];
  }
}

// backward stage 2 (per src row over CSC): dk[s] = sum dek, dv[s] = sum dev
template <int VPT>
__global__ void edge_attn_bwd_col_kernel(
    const float* __restrict__ dek, const float* __restrict__ dev,
    const int* __restrict__ col_ptr, const int* __restrict__ csc_eid,
    float* __restrict__ dk, float* __restrict__ dv, int n, int h) {
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int row = blockIdx.x * WAVES_PER_BLOCK + wid;
  if (row >= n) return;
  float ka[VPT], va[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) { ka[j] = 0.f; va[j] = 0.f; }
  for (int p = col_ptr[row]; p < col_ptr[row + 1]; ++p) {
    const long eid = csc_eid[p];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const int c = lane + j * PERTGNN_WAVE;
      if (c < h) {
        ka[j] += dek[eid * h + c];
        va[j] += dev[eid * h + c];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const int c = lane + j * PERTGNN_WAVE;
    if (c < h) {
      dk[(long)row * h + c] = ka[j];
      dv[(long)row * h + c] = va[j];
    }
  }
}

// backward stage 3: de = dek + dev (elementwise over E*H)
__global__ void add_kernel(const float* __restrict__ a,
                           const float* __restrict__ b,
                           float* __restrict__ out, long numel) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = i; t < numel; t += stride) out[t] = a[t] + b[t];
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

void launch_edge_attn_fwd(const float* q, const float* k, const float* v,
                          const float* e, const int* row_ptr,
                          const int* csr_src, const float* skip, float* out,
                          float* alpha, int n, int h, hipStream_t stream) {
  if (n == 0) return;
  const float scale = 1.f / std::sqrt((float)h);
  const dim3 grid(ceil_div(n, WAVES_PER_BLOCK));
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const int vpt = (h + PERTGNN_WAVE - 1) / PERTGNN_WAVE;
  switch (vpt) {
#define CASE(V)                                                                \
  case V:                                                                      \
    edge_attn_fwd_kernel<V><<<grid, block, 0, stream>>>(                       \
        q, k, v, e, row_ptr, csr_src, skip, out, alpha, n, h, scale);          \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: pertgnn_shape_fail("edge_attn launcher", "vpt", vpt);
  }
}

void launch_edge_attn_bwd(const float* g, const float* q, const float* k,
                          const float* v, const float* e, const float* alpha,
                          const int* row_ptr, const int* csr_src,
                          const int* col_ptr, const int* csc_eid, float* dq,
                          float* dk, float* dv, float* de, float* dek,
                          float* dev, int n, int h, long num_edges,
                          hipStream_t stream) {
  if (n == 0) return;
  const float scale = 1.f / std::sqrt((float)h);
  const dim3 grid(ceil_div(n, WAVES_PER_BLOCK));
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const int vpt = (h + PERTGNN_WAVE - 1) / PERTGNN_WAVE;
  switch (vpt) {
#define CASE(V)                                                                \
  case V:                                                                      \
    edge_attn_bwd_row_kernel<V><<<grid, block, 0, stream>>>(                   \
        g, q, k, v, e, alpha, row_ptr, csr_src, dq, dek, dev, n, h, scale);    \
    edge_attn_bwd_col_kernel<V><<<grid, block, 0, stream>>>(                   \
        dek, dev, col_ptr, csc_eid, dk, dv, n, h);                             \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: pertgnn_shape_fail("edge_attn launcher", "vpt", vpt);
  }
  const long numel = num_edges * h;
  if (numel > 0) {
    const int tpb = 256;
    const int blocks = (int)min((numel + tpb - 1) / tpb, (long)2048);
    add_kernel<<<dim3(blocks), dim3(tpb), 0, stream>>>(dek, dev, de, numel);
  }
}
