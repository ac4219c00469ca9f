// Fused-layout CSR edge attention (gfx950) — production path.
//
// Differences from edge_attn.hip (which remains as the reference-layout
// kernel used by the op-level parity tests):
//   * q/k/v/skip live in ONE [N,4H] tensor (output of the fused QKVS GEMM)
//     — one GEMM launch and one gradient buffer instead of four;
//   * the per-edge embedding e_ij = W_e [ifc(a0) ‖ rpc(a1)] is NOT
//     materialized: by linearity it equals P_ifc[a0] + P_rpc[a1] where
//     P_ifc = ifc_table @ W_e[:, :H]^T (a tiny [V,H] table computed once per
//     layer) — the kernel gathers from these L2-resident tables instead of
//     streaming an [E,H] operand from HBM (halves forward edge traffic).
//
// Row mapping: LPR lanes per CSR destination row (default 32 — PERT rows
// average degree ~1.3, so packing 2 rows per wave doubles row throughput of
// the latency-bound per-edge loop); reductions are sub-wave shfl_xor trees.
//
// Column mapping: in VEC mode each sub-wave lane owns VPT CONTIGUOUS columns
// (lane*VPT..) so every per-edge row access is vectorized 16B loads (guide
// G13); otherwise the strided lane+j*64 mapping with per-column guards
// (LPR=64 only).  The mapping is an internal detail — every tensor is
// read/written with the same mapping.
//
// Backward: row kernel writes dq + dskip segments of dqkvs and per-edge
// dek/dev scratch; col kernel (CSC) segment-sums dk/dv into dqkvs; de =
// dek + dev feeds the per-vocab scatter (python side) to produce
// dP_ifc/dP_rpc.  Deterministic — no atomics anywhere.

#include "common.h"
#include "launchers.h"
#include "attn_bn.h"
#include <cmath>
#include <cstdlib>
#include <type_traits>

#define WAVES_PER_BLOCK 4

typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;

// row-slice accessors for the two column mappings; fp32 and bf16 overloads
// (bf16 rows are the qkvs/dqkvs tensors in bf16-resident-activation mode).
template <int VPT, bool VEC>
struct Slice {
  static __device__ __forceinline__ void load(const float* base, int lane,
                                              int h, float (&dst)[VPT]) {
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < VPT; q += 4)
        *reinterpret_cast<f32x4_t*>(&dst[q]) =
            *reinterpret_cast<const f32x4_t*>(&base[lane * VPT + q]);
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const int c = lane + j * PERTGNN_WAVE;
        dst[j] = (c < h) ? base[c] : 0.f;
      }
    }
  }
  static __device__ __forceinline__ void load(const __bf16* base, int lane,
                                              int h, float (&dst)[VPT]) {
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < VPT; q += 4) {
        const bf16x4_t v =
            *reinterpret_cast<const bf16x4_t*>(&base[lane * VPT + q]);
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[q + u] = (float)v[u];
      }
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const int c = lane + j * PERTGNN_WAVE;
        dst[j] = (c < h) ? (float)base[c] : 0.f;
      }
    }
  }
  static __device__ __forceinline__ void load_add(const float* a,
                                                  const float* b, int lane,
                                                  int h, float (&dst)[VPT]) {
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < VPT; q += 4) {
        const f32x4_t va = *reinterpret_cast<const f32x4_t*>(&a[lane * VPT + q]);
        const f32x4_t vb = *reinterpret_cast<const f32x4_t*>(&b[lane * VPT + q]);
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[q + u] = va[u] + vb[u];
      }
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const int c = lane + j * PERTGNN_WAVE;
        dst[j] = (c < h) ? a[c] + b[c] : 0.f;
      }
    }
  }
  static __device__ __forceinline__ void load_add(const __bf16* a,
                                                  const __bf16* b, int lane,
                                                  int h, float (&dst)[VPT]) {
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < VPT; q += 4) {
        const bf16x4_t va =
            *reinterpret_cast<const bf16x4_t*>(&a[lane * VPT + q]);
        const bf16x4_t vb =
            *reinterpret_cast<const bf16x4_t*>(&b[lane * VPT + q]);
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[q + u] = (float)va[u] + (float)vb[u];
      }
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const int c = lane + j * PERTGNN_WAVE;
        dst[j] = (c < h) ? (float)a[c] + (float)b[c] : 0.f;
      }
    }
  }
  static __device__ __forceinline__ void store(float* base, int lane, int h,
                                               const float (&src)[VPT]) {
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < VPT; q += 4)
        *reinterpret_cast<f32x4_t*>(&base[lane * VPT + q]) =
            *reinterpret_cast<const f32x4_t*>(&src[q]);
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const int c = lane + j * PERTGNN_WAVE;
        if (c < h) base[c] = src[j];
      }
    }
  }
  static __device__ __forceinline__ void store(__bf16* base, int lane, int h,
                                               const float (&src)[VPT]) {
    if constexpr (VEC) {
#pragma unroll
      for (int q = 0; q < VPT; q += 4) {
        bf16x4_t v;
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (__bf16)src[q + u];
        *reinterpret_cast<bf16x4_t*>(&base[lane * VPT + q]) = v;
      }
    } else {
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const int c = lane + j * PERTGNN_WAVE;
        if (c < h) base[c] = (__bf16)src[j];
      }
    }
  }
};

// Multi-head attention (heads * C == h, concat): head t owns channels
// [tC, (t+1)C), its logit is the dot product over those channels scaled by
// 1/sqrt(C), and the softmax runs per head.  Every [.,h] tensor keeps its
// shape; the per-edge scalars alpha/dal become [E, heads] row-major.
//
//   * VEC mapping: LPH = C/VPT lanes hold one head (a lane's VPT contiguous
//     columns never straddle a head), heads = LPR/LPH.  The logit reduce is
//     a LPH-lane tree and each lane carries the softmax state of ITS head,
//     so the per-lane work is the single-head code with a shorter tree.
//     LPH == LPR is the single-head kernel, instruction for instruction.
//   * non-VEC mapping (PCH, "per-column heads"): C divides 64, so register
//     column j of a lane (channel lane + j*64) belongs to head
//     lane/C + j*(64/C); each j gets its own C-lane reduce and its own
//     softmax state.  LPH carries C here.
//
// Slot (edge p, head t) of alpha/dal has ONE writer lane, inside the lane
// group of head t: sub-lane (p - beg) % LPH.  The finalize loops stride the
// row's edges by LPH from the same sub-lane, so a thread re-reads exactly
// the slots it stored itself (same-thread read-after-write, no fence), and
// the heads of one edge are written by different lanes.
template <int LPR, int LPH>
struct HeadMap {
  static constexpr int HEADS = LPR / LPH;
  static __device__ __forceinline__ int head(int lane) {
    if constexpr (HEADS == 1) return 0;
    else return lane / LPH;
  }
  static __device__ __forceinline__ int sub(int lane) {
    if constexpr (HEADS == 1) return lane;
    else return lane % LPH;
  }
  static __device__ __forceinline__ long slot(int p, int hd) {
    if constexpr (HEADS == 1) return p;
    else return (long)p * HEADS + hd;
  }
};

// LPR = lanes per row: CSR rows average degree ~1.3 on PERT graphs, so a
// full 64-lane wave per row is latency-bound with most lanes idle between
// the few row loads.  LPR<64 packs 64/LPR rows into a wave (each sub-group
// owns h/LPR contiguous columns); reductions become sub-wave shfl_xor trees.
// LPR=32 measured best at H=256 (see attn_lpr below).
template <int VPT, bool VEC, typename QT = float, int LPR = PERTGNN_WAVE,
          typename TO = float, typename PT = float, int LPH = LPR,
          bool PCH = false>
__global__ void edge_attn_fused_fwd_kernel(
    const QT* __restrict__ qkvs,  // [N, 4h]
    const PT* __restrict__ pifc,  // [Vi, h] (bf16 in act16 mode — halves
    const PT* __restrict__ prpc,  // [Vr, h]  the per-edge ec gathers)
    const long* __restrict__ ea, int astride,
    const int* __restrict__ row_ptr, const int* __restrict__ csr_src,
    TO* __restrict__ out, float* __restrict__ alpha, int n, int h,
    float scale) {
  using S = Slice<VPT, VEC>;
  static_assert(VEC || LPR == PERTGNN_WAVE, "sub-wave rows need VEC layout");
  static_assert(PCH ? !VEC : (VEC || LPH == LPR),
                "heads split the sub-row (VEC) or the columns (PCH)");
  static_assert(LPH >= 1 && LPH <= LPR && (LPH & (LPH - 1)) == 0,
                "lanes per head: a power of two within the row");
  constexpr int RPW = PERTGNN_WAVE / LPR;
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane0 = threadIdx.x % PERTGNN_WAVE;
  const int sub = lane0 / LPR;
  const int lane = lane0 % LPR;
  const int row = (blockIdx.x * WAVES_PER_BLOCK + wid) * RPW + sub;
  if (row >= n) return;
  const long ld = 4L * h;

  float qr[VPT], acc[VPT];
  S::load(&qkvs[row * ld], lane, h, qr);
#pragma unroll
  for (int j = 0; j < VPT; ++j) acc[j] = 0.f;

  const int beg = row_ptr[row], end = row_ptr[row + 1];
  if constexpr (PCH) {
    // per-column heads: one softmax state per register column
    constexpr int HPJ = PERTGNN_WAVE / LPH;  // heads per register column
    const int heads = h / LPH;
    const int hg = lane / LPH, hl = lane % LPH;
    float m[VPT], s[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) { m[j] = -INFINITY; s[j] = 0.f; }
    for (int p = beg; p < end; ++p) {
      const long src = csr_src[p];
      const long a0 = ea[(long)p * astride];
      const long a1 = ea[(long)p * astride + 1];
      float ec[VPT], ke[VPT], ve[VPT], logit[VPT];
      S::load_add(&pifc[a0 * h], &prpc[a1 * h], lane, h, ec);
      S::load(&qkvs[src * ld + h], lane, h, ke);
      S::load(&qkvs[src * ld + 2 * h], lane, h, ve);
#pragma unroll
      for (int j = 0; j < VPT; ++j)
        logit[j] = subwave_reduce_sum<LPH>(qr[j] * (ke[j] + ec[j])) * scale;
      const bool writer = hl == (p - beg) % LPH;
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        // lanes past h hold no head (their slot would lie outside the row)
        if (writer && lane + j * PERTGNN_WAVE < h)
          alpha[(long)p * heads + hg + j * HPJ] = logit[j];
        const float m_new = fmaxf(m[j], logit[j]);
        const float corr = __expf(m[j] - m_new);
        const float pexp = __expf(logit[j] - m_new);
        s[j] = s[j] * corr + pexp;
        acc[j] = acc[j] * corr + pexp * (ve[j] + ec[j]);
        m[j] = m_new;
      }
    }
    float sk[VPT], res[VPT], inv_s[VPT];
    S::load(&qkvs[row * ld + 3 * h], lane, h, sk);
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      inv_s[j] = (s[j] > 0.f) ? 1.f / s[j] : 0.f;
      res[j] = acc[j] * inv_s[j] + sk[j];
    }
    S::store(&out[(long)row * h], lane, h, res);
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      if (lane + j * PERTGNN_WAVE < h) {
        for (int p = beg + hl; p < end; p += LPH) {
          const long sl = (long)p * heads + hg + j * HPJ;
          alpha[sl] = __expf(alpha[sl] - m[j]) * inv_s[j];
        }
      }
    }
    return;
  }
  using HM = HeadMap<LPR, LPH>;
  const int hd = HM::head(lane), hl = HM::sub(lane);
  float m = -INFINITY, s = 0.f;
  for (int p = beg; p < end; ++p) {
    const long src = csr_src[p];
    const long a0 = ea[(long)p * astride];
    const long a1 = ea[(long)p * astride + 1];
    float ec[VPT], ke[VPT], ve[VPT];
    // all three gathers issue together: the ve load must not sit behind the
    // sub-wave reduce + expf chain (one exposed memory latency per edge)
    S::load_add(&pifc[a0 * h], &prpc[a1 * h], lane, h, ec);
    S::load(&qkvs[src * ld + h], lane, h, ke);
    S::load(&qkvs[src * ld + 2 * h], lane, h, ve);
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) part += qr[j] * (ke[j] + ec[j]);
    const float logit = subwave_reduce_sum<LPH>(part) * scale;
    if (hl == (p - beg) % LPH) alpha[HM::slot(p, hd)] = logit;
    const float m_new = fmaxf(m, logit);
    const float corr = __expf(m - m_new);
    const float pexp = __expf(logit - m_new);
    s = s * corr + pexp;
#pragma unroll
    for (int j = 0; j < VPT; ++j)
      acc[j] = acc[j] * corr + pexp * (ve[j] + ec[j]);
    m = m_new;
  }

  const float inv_s = (s > 0.f) ? 1.f / s : 0.f;
  float sk[VPT], res[VPT];
  S::load(&qkvs[row * ld + 3 * h], lane, h, sk);
#pragma unroll
  for (int j = 0; j < VPT; ++j) res[j] = acc[j] * inv_s + sk[j];
  S::store(&out[(long)row * h], lane, h, res);
  for (int p = beg + hl; p < end; p += LPH)
    alpha[HM::slot(p, hd)] = __expf(alpha[HM::slot(p, hd)] - m) * inv_s;
}

// Forward-only variant for inference: same row/column mapping and online
// softmax as the training forward, but nothing is kept for a backward — no
// alpha tensor, no per-edge logit store, no second pass over the row's
// edges — and the eval-mode BatchNorm (a fixed per-channel affine, folded
// on the host into bn_scale/bn_shift) plus the ReLU ride in the epilogue
// while the row is still in fp32 registers: one store, rounded once.
// bn_scale == nullptr skips the affine.  Rows without in-edges (s == 0)
// produce epilogue(skip).
template <int VPT, bool VEC, typename QT = float, int LPR = PERTGNN_WAVE,
          typename TO = float, typename PT = float, int LPH = LPR,
          bool PCH = false>
__global__ void edge_attn_fused_infer_kernel(
    const QT* __restrict__ qkvs,  // [N, 4h]
    const PT* __restrict__ pifc,  // [Vi, h]
    const PT* __restrict__ prpc,  // [Vr, h]
    const long* __restrict__ ea, int astride,
    const int* __restrict__ row_ptr, const int* __restrict__ csr_src,
    const float* __restrict__ bn_scale,  // [h] or null
    const float* __restrict__ bn_shift,  // [h] or null
    int relu, TO* __restrict__ out, int n, int h, float scale) {
  using S = Slice<VPT, VEC>;
  static_assert(VEC || LPR == PERTGNN_WAVE, "sub-wave rows need VEC layout");
  static_assert(PCH ? !VEC : (VEC || LPH == LPR),
                "heads split the sub-row (VEC) or the columns (PCH)");
  static_assert(LPH >= 1 && LPH <= LPR && (LPH & (LPH - 1)) == 0,
                "lanes per head: a power of two within the row");
  constexpr int RPW = PERTGNN_WAVE / LPR;
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane0 = threadIdx.x % PERTGNN_WAVE;
  const int sub = lane0 / LPR;
  const int lane = lane0 % LPR;
  const int row = (blockIdx.x * WAVES_PER_BLOCK + wid) * RPW + sub;
  if (row >= n) return;
  const long ld = 4L * h;

  float qr[VPT], acc[VPT];
  S::load(&qkvs[row * ld], lane, h, qr);
#pragma unroll
  for (int j = 0; j < VPT; ++j) acc[j] = 0.f;

  const int beg = row_ptr[row], end = row_ptr[row + 1];
  float sk[VPT], res[VPT];
  if constexpr (PCH) {
    // per-column heads: one softmax state per register column
    float m[VPT], s[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) { m[j] = -INFINITY; s[j] = 0.f; }
    for (int p = beg; p < end; ++p) {
      const long src = csr_src[p];
      const long a0 = ea[(long)p * astride];
      const long a1 = ea[(long)p * astride + 1];
      float ec[VPT], ke[VPT], ve[VPT];
      S::load_add(&pifc[a0 * h], &prpc[a1 * h], lane, h, ec);
      S::load(&qkvs[src * ld + h], lane, h, ke);
      S::load(&qkvs[src * ld + 2 * h], lane, h, ve);
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const float logit =
            subwave_reduce_sum<LPH>(qr[j] * (ke[j] + ec[j])) * scale;
        const float m_new = fmaxf(m[j], logit);
        const float corr = __expf(m[j] - m_new);
        const float pexp = __expf(logit - m_new);
        s[j] = s[j] * corr + pexp;
        acc[j] = acc[j] * corr + pexp * (ve[j] + ec[j]);
        m[j] = m_new;
      }
    }
    S::load(&qkvs[row * ld + 3 * h], lane, h, sk);
#pragma unroll
    for (int j = 0; j < VPT; ++j)
      res[j] = acc[j] * ((s[j] > 0.f) ? 1.f / s[j] : 0.f) + sk[j];
  } else {
    float m = -INFINITY, s = 0.f;
    for (int p = beg; p < end; ++p) {
      const long src = csr_src[p];
      const long a0 = ea[(long)p * astride];
      const long a1 = ea[(long)p * astride + 1];
      float ec[VPT], ke[VPT], ve[VPT];
      // all three gathers issue together, as in the training forward
      S::load_add(&pifc[a0 * h], &prpc[a1 * h], lane, h, ec);
      S::load(&qkvs[src * ld + h], lane, h, ke);
      S::load(&qkvs[src * ld + 2 * h], lane, h, ve);
      float part = 0.f;
#pragma unroll
      for (int j = 0; j < VPT; ++j) part += qr[j] * (ke[j] + ec[j]);
      // the lane's own head: LPH-lane tree, per-lane softmax state
      const float logit = subwave_reduce_sum<LPH>(part) * scale;
      const float m_new = fmaxf(m, logit);
      const float corr = __expf(m - m_new);
      const float pexp = __expf(logit - m_new);
      s = s * corr + pexp;
#pragma unroll
      for (int j = 0; j < VPT; ++j)
        acc[j] = acc[j] * corr + pexp * (ve[j] + ec[j]);
      m = m_new;
    }

    const float inv_s = (s > 0.f) ? 1.f / s : 0.f;
    S::load(&qkvs[row * ld + 3 * h], lane, h, sk);
#pragma unroll
    for (int j = 0; j < VPT; ++j) res[j] = acc[j] * inv_s + sk[j];
  }
  if (bn_scale != nullptr) {
    // same Slice mapping as the row: the non-VEC c < h guard covers these
    float bs[VPT], bb[VPT];
    S::load(bn_scale, lane, h, bs);
    S::load(bn_shift, lane, h, bb);
#pragma unroll
    for (int j = 0; j < VPT; ++j) res[j] = res[j] * bs[j] + bb[j];
  }
  if (relu) {
#pragma unroll
    for (int j = 0; j < VPT; ++j) res[j] = fmaxf(res[j], 0.f);
  }
  S::store(&out[(long)row * h], lane, h, res);
}

// BN(+ReLU+dropout) backward of one row slice in the VEC mapping: gr holds
// the BN output gradient of the lane's VPT contiguous channels on entry and
// the BN input gradient, rounded to bf16, on return — the bits the stand-
// alone bn_bwd_apply_wide_kernel stores as dx.  Keep-mask layout (segops.hip,
// above bn_wide_ok): bit u of byte (r, c/8) belongs to channel c+u, so the
// lane's bits start at bit (lane*VPT)%8 of byte (lane*VPT)/8 of the row's
// h/8 bytes (VPT = 4 shares a byte between two lanes, VPT >= 8 owns VPT/8
// bytes).  The per-channel constants are live in here only.
template <int VPT>
__device__ __forceinline__ void attn_bn_bwd_row(const AttnBnBwd& bn, int row,
                                                int lane, int h,
                                                float (&gr)[VPT]) {
  using S = Slice<VPT, true>;
  static_assert(VPT == 4 || VPT % 8 == 0, "a lane's channels fill mask bytes");
  constexpr int NB = (VPT + 7) / 8;
  const float invn =
      1.f / (bn.count_ptr ? *bn.count_ptr : (float)bn.count);
  const int c0 = lane * VPT;
  const unsigned char* mrow = bn.mask + (long)row * (h >> 3) + (c0 >> 3);
  unsigned bits[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) bits[b] = mrow[b];
  float xr[VPT], mu[VPT], is[VPT], ga[VPT], p0[VPT], p1[VPT];
  S::load(&((const __bf16*)bn.x)[(long)row * h], lane, h, xr);
  S::load(bn.mean, lane, h, mu);
  S::load(bn.invstd, lane, h, is);
  S::load(bn.gamma, lane, h, ga);
  S::load(bn.partials, lane, h, p0);
  S::load(bn.partials + h, lane, h, p1);
#pragma unroll
  for (int j = 0; j < VPT; ++j) {
    const bool keep = (bits[j >> 3] >> ((c0 & 7) + (j & 7))) & 1u;
    gr[j] = (float)bn_bwd_dx16(gr[j], xr[j], keep, mu[j], is[j], ga[j], p0[j],
                               p1[j], invn, bn.keep_inv);
  }
}

// Pattern-pool backward of one node's row slice: the fp32 values that
// seg_pool_bwd_kernel would have stored at [node, lane's channels].
template <int VPT>
__device__ __forceinline__ void attn_pool_bwd_row(const AttnPoolBwd& pool,
                                                  long node, int lane, int h,
                                                  float (&gr)[VPT]) {
  const float p = pool.probs[node];
  const float nn = pool.nn[node];
  Slice<VPT, true>::load(&pool.gout[pool.batch[node] * h], lane, h, gr);
#pragma unroll
  for (int j = 0; j < VPT; ++j) gr[j] = pool_bwd_dx(gr[j], p, nn);
}

// POOL (both backward kernels): there is no g; a node's gradient is the
// pattern pool's backward, formed from `pool`.  Only the instantiations the
// last conv takes in act16 mode carry it (fp32 gradient, bf16 qkvs, VEC
// mapping).  A template parameter and not a branch on pool.gout: with both
// paths in one kernel the col kernel's edge loop held the registers of both
// gathers (62 -> 91 VGPRs at H = 256, three waves per SIMD lost).
template <bool POOL, bool VEC, typename QT, typename TG>
constexpr bool attn_pool_ok =
    !POOL ||
    (VEC && std::is_same<TG, float>::value && std::is_same<QT, __bf16>::value);

template <int VPT, bool VEC, typename QT = float,
          int LPR = PERTGNN_WAVE, typename TG = float, typename PT = float,
          int LPH = LPR, bool PCH = false, bool POOL = false>
__global__ void edge_attn_fused_bwd_row_kernel(
    const TG* __restrict__ g, const QT* __restrict__ qkvs,
    const PT* __restrict__ pifc, const PT* __restrict__ prpc,
    const long* __restrict__ ea, int astride, const float* __restrict__ alpha,
    const int* __restrict__ row_ptr, const int* __restrict__ csr_src,
    QT* __restrict__ dqkvs, float* __restrict__ dal, int n, int h,
    float scale, AttnBnBwd bn = AttnBnBwd{},
    AttnPoolBwd pool = AttnPoolBwd{}) {
  // SINGLE pass over the row's edges (the old two-pass form re-gathered
  // ec+ke per edge after sdot was known).  Softmax backward re-expressed:
  //   dq = scale * (Sum a*da*(k+e)  -  sdot * Sum a*(k+e))
  // accumulates both sums alongside sdot = Sum a*da; the per-edge logit
  // grad dl = scale*a*(da - sdot) is a SCALAR — dek = dl*q_row and
  // dev = a*g_row are rank-1, so the [E,h] dek/dev scratch tensors are
  // gone: the col kernel regenerates them from (dal, alpha) and row
  // gathers of q/g.
  using S = Slice<VPT, VEC>;
  static_assert(VEC || LPR == PERTGNN_WAVE, "sub-wave rows need VEC layout");
  static_assert(PCH ? !VEC : (VEC || LPH == LPR),
                "heads split the sub-row (VEC) or the columns (PCH)");
  static_assert(LPH >= 1 && LPH <= LPR && (LPH & (LPH - 1)) == 0,
                "lanes per head: a power of two within the row");
  constexpr int RPW = PERTGNN_WAVE / LPR;
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane0 = threadIdx.x % PERTGNN_WAVE;
  const int lane = lane0 % LPR;
  const int row = (blockIdx.x * WAVES_PER_BLOCK + wid) * RPW + lane0 / LPR;
  if (row >= n) return;
  const long ld = 4L * h;

  float gr[VPT], a1[VPT], a2[VPT];
  static_assert(attn_pool_ok<POOL, VEC, QT, TG>, "pool mode: act16, fp32 g");
  // POOL: the row's gradient is the pattern pool's backward, formed here
  // and stored as dskip below like any other
  if constexpr (POOL) attn_pool_bwd_row<VPT>(pool, row, lane, h, gr);
  else S::load(&g[(long)row * h], lane, h, gr);
  // g is the BN OUTPUT gradient when bn.x is set (wave-uniform): the row's
  // gradient is then formed here, and stored as dskip below like any other
  // (h = 256 / 512 only: VPT <= 16 in every lane mapping of those widths)
  if constexpr (VEC && std::is_same<TG, __bf16>::value && VPT <= 16) {
    if (bn.x) attn_bn_bwd_row<VPT>(bn, row, lane, h, gr);
  }
#pragma unroll
  for (int j = 0; j < VPT; ++j) { a1[j] = 0.f; a2[j] = 0.f; }

  const int beg = row_ptr[row], end = row_ptr[row + 1];
  if constexpr (PCH) {
    // per-column heads: sdot and the (alpha, dal) slot are per register column
    constexpr int HPJ = PERTGNN_WAVE / LPH;
    const int heads = h / LPH;
    const int hg = lane / LPH, hl = lane % LPH;
    float sdot[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) sdot[j] = 0.f;
    for (int p = beg; p < end; ++p) {
      const long src = csr_src[p];
      const long e0 = ea[(long)p * astride];
      const long e1 = ea[(long)p * astride + 1];
      float ec[VPT], ke[VPT], ve[VPT];
      S::load_add(&pifc[e0 * h], &prpc[e1 * h], lane, h, ec);
      S::load(&qkvs[src * ld + h], lane, h, ke);
      S::load(&qkvs[src * ld + 2 * h], lane, h, ve);
      const bool writer = hl == (p - beg) % LPH;
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const float dalpha =
            subwave_reduce_sum<LPH>(gr[j] * (ve[j] + ec[j]));
        // lanes past h hold no head: no slot to read or write
        const bool live = lane + j * PERTGNN_WAVE < h;
        const long sl = (long)p * heads + hg + j * HPJ;
        const float a = live ? alpha[sl] : 0.f;
        sdot[j] += a * dalpha;
        if (writer && live) dal[sl] = dalpha;
        const float kec = ke[j] + ec[j];
        a1[j] += a * dalpha * kec;
        a2[j] += a * kec;
      }
    }
    float dq[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) dq[j] = scale * (a1[j] - sdot[j] * a2[j]);
    S::store(&dqkvs[row * ld], lane, h, dq);             // dq
    S::store(&dqkvs[row * ld + 3 * h], lane, h, gr);     // dskip = g
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      if (lane + j * PERTGNN_WAVE < h) {
        for (int p = beg + hl; p < end; p += LPH) {
          const long sl = (long)p * heads + hg + j * HPJ;
          dal[sl] = scale * alpha[sl] * (dal[sl] - sdot[j]);
        }
      }
    }
    return;
  }
  using HM = HeadMap<LPR, LPH>;
  const int hd = HM::head(lane), hl = HM::sub(lane);
  float sdot = 0.f;
  for (int p = beg; p < end; ++p) {
    const long src = csr_src[p];
    const long e0 = ea[(long)p * astride];
    const long e1 = ea[(long)p * astride + 1];
    float ec[VPT], ke[VPT], ve[VPT];
    S::load_add(&pifc[e0 * h], &prpc[e1 * h], lane, h, ec);
    S::load(&qkvs[src * ld + h], lane, h, ke);
    S::load(&qkvs[src * ld + 2 * h], lane, h, ve);
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < VPT; ++j) part += gr[j] * (ve[j] + ec[j]);
    const float dalpha = subwave_reduce_sum<LPH>(part);
    const float a = alpha[HM::slot(p, hd)];
    sdot += a * dalpha;
    if (hl == (p - beg) % LPH) dal[HM::slot(p, hd)] = dalpha;
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const float kec = ke[j] + ec[j];
      a1[j] += a * dalpha * kec;
      a2[j] += a * kec;
    }
  }
  float dq[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) dq[j] = scale * (a1[j] - sdot * a2[j]);
  S::store(&dqkvs[row * ld], lane, h, dq);             // dq
  S::store(&dqkvs[row * ld + 3 * h], lane, h, gr);     // dskip = g
  // finalize per-edge logit grads: each lane rewrites exactly the slots it
  // stored above (same-thread read-after-write)
  for (int p = beg + hl; p < end; p += LPH)
    dal[HM::slot(p, hd)] =
        scale * alpha[HM::slot(p, hd)] * (dal[HM::slot(p, hd)] - sdot);
}

template <int VPT, bool VEC, typename QT = float, typename ET = float,
          int LPR = PERTGNN_WAVE, typename TG = float, int LPH = LPR,
          bool PCH = false, bool POOL = false>
__global__ void edge_attn_fused_bwd_col_kernel(
    const TG* g, const QT* __restrict__ qkvs,
    const float* __restrict__ alpha, const float* __restrict__ dal,
    const int* __restrict__ col_ptr, const int* __restrict__ csc_dst,
    const int* __restrict__ csc_eid, QT* dqkvs,
    ET* __restrict__ de, int n, int h, long gld,
    AttnPoolBwd pool = AttnPoolBwd{}) {
  // g rows lie gld elements apart: h for a compact [n, h] gradient, 4h when
  // g is the dskip segment of dqkvs that the row kernel wrote before this
  // kernel started (same stream).  g and dqkvs then share an allocation —
  // the columns read (3h..4h) and written (h..3h) are disjoint — so neither
  // pointer is __restrict__.
  using S = Slice<VPT, VEC>;
  static_assert(VEC || LPR == PERTGNN_WAVE, "sub-wave rows need VEC layout");
  static_assert(PCH ? !VEC : (VEC || LPH == LPR),
                "heads split the sub-row (VEC) or the columns (PCH)");
  static_assert(LPH >= 1 && LPH <= LPR && (LPH & (LPH - 1)) == 0,
                "lanes per head: a power of two within the row");
  static_assert(attn_pool_ok<POOL, VEC, QT, TG>, "pool mode: act16, fp32 g");
  constexpr int RPW = PERTGNN_WAVE / LPR;
  const int wid = threadIdx.x / PERTGNN_WAVE;
  const int lane0 = threadIdx.x % PERTGNN_WAVE;
  const int lane = lane0 % LPR;
  const int row = (blockIdx.x * WAVES_PER_BLOCK + wid) * RPW + lane0 / LPR;
  if (row >= n) return;
  const long ld = 4L * h;
  float ka[VPT], va[VPT];
#pragma unroll
  for (int j = 0; j < VPT; ++j) { ka[j] = 0.f; va[j] = 0.f; }
  if constexpr (PCH) {
    // per-column heads: each register column reads its head's (dal, alpha)
    constexpr int HPJ = PERTGNN_WAVE / LPH;
    const int heads = h / LPH;
    const int hg = lane / LPH;
    for (int p = col_ptr[row]; p < col_ptr[row + 1]; ++p) {
      const long eid = csc_eid[p];
      const long dst = csc_dst[p];
      float qd[VPT], gd[VPT], des[VPT];
      S::load(&qkvs[dst * ld], lane, h, qd);
      S::load(&g[dst * gld], lane, h, gd);
#pragma unroll
      for (int j = 0; j < VPT; ++j) {
        const bool live = lane + j * PERTGNN_WAVE < h;
        const long sl = eid * heads + hg + j * HPJ;
        const float dk1 = (live ? dal[sl] : 0.f) * qd[j];
        const float dv1 = (live ? alpha[sl] : 0.f) * gd[j];
        ka[j] += dk1;
        va[j] += dv1;
        des[j] = dk1 + dv1;
      }
      S::store(&de[eid * h], lane, h, des);
    }
    S::store(&dqkvs[(long)row * ld + h], lane, h, ka);
    S::store(&dqkvs[(long)row * ld + 2 * h], lane, h, va);
    return;
  }
  using HM = HeadMap<LPR, LPH>;
  const int hd = HM::head(lane);
  for (int p = col_ptr[row]; p < col_ptr[row + 1]; ++p) {
    const long eid = csc_eid[p];
    const long dst = csc_dst[p];
    const float dl = dal[eid * HM::HEADS + hd];
    const float a = alpha[eid * HM::HEADS + hd];
    float qd[VPT], gd[VPT], des[VPT];
    S::load(&qkvs[dst * ld], lane, h, qd);
    // pool mode: the destination's gradient from its graph's gout row and
    // its two scalars, the same bits the row kernel formed for that node
    if constexpr (POOL) attn_pool_bwd_row<VPT>(pool, dst, lane, h, gd);
    else S::load(&g[dst * gld], lane, h, gd);
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
      const float dk1 = dl * qd[j];
      const float dv1 = a * gd[j];
      ka[j] += dk1;
      va[j] += dv1;
      des[j] = dk1 + dv1;
    }
    // every edge appears exactly once in the CSC sweep: de rides along
    S::store(&de[eid * h], lane, h, des);
  }
  S::store(&dqkvs[(long)row * ld + h], lane, h, ka);
  S::store(&dqkvs[(long)row * ld + 2 * h], lane, h, va);
}


// ---------------------------------------------------------------------------

// --- head-count dispatch shared by all launchers ---------------------------

[[noreturn]] static void attn_heads_fail(const char* launcher, int h,
                                         int heads, int lpr) {
  throw std::runtime_error(
      std::string("pertgnn ") + launcher + ": unsupported shape (h=" +
      std::to_string(h) + ", heads=" + std::to_string(heads) + ", lpr=" +
      std::to_string(lpr) + "): the lanes of a row cannot be split into " +
      "these heads");
}

static bool attn_heads_ok(int h, int heads) {
  return heads >= 1 && h % heads == 0;
}

// VEC mapping: lanes per head for C = h/heads channels at vpt contiguous
// columns per lane, or 0 when a lane would straddle heads / the head is no
// power-of-two lane group inside the lpr lanes of the row
static int vec_lph(int h, int heads, int vpt, int lpr) {
  if (!attn_heads_ok(h, heads)) return 0;
  const int c = h / heads;
  if (c % vpt != 0) return 0;
  const int lph = c / vpt;
  if (lph < 1 || lph > lpr || (lph & (lph - 1)) != 0) return 0;
  return lph;
}

// non-VEC mapping (per-column heads): C must divide the 64 lanes
static int pch_lanes(int h, int heads) {
  if (!attn_heads_ok(h, heads)) return 0;
  const int c = h / heads;
  return (c <= PERTGNN_WAVE && PERTGNN_WAVE % c == 0) ? c : 0;
}

// M(A, LPR, LPH) for the runtime lanes-per-head L (a power of two <= LPR;
// anything else, 0 included, is the shape error).  Every branch names a
// valid instantiation — the ones LPR rules out collapse onto LPH == LPR and
// are never taken.
#define HEAD_CHAIN(M, A, LPR, L, NAME)                                         \
  do {                                                                         \
    if ((L) == 64 && 64 <= LPR) M(A, LPR, (64 <= LPR ? 64 : LPR));             \
    else if ((L) == 32 && 32 <= LPR) M(A, LPR, (32 <= LPR ? 32 : LPR));        \
    else if ((L) == 16 && 16 <= LPR) M(A, LPR, (16 <= LPR ? 16 : LPR));        \
    else if ((L) == 8 && 8 <= LPR) M(A, LPR, (8 <= LPR ? 8 : LPR));            \
    else if ((L) == 4 && 4 <= LPR) M(A, LPR, (4 <= LPR ? 4 : LPR));            \
    else if ((L) == 2 && 2 <= LPR) M(A, LPR, (2 <= LPR ? 2 : LPR));            \
    else if ((L) == 1) M(A, LPR, 1);                                           \
    else attn_heads_fail(NAME, h, heads, LPR);                                 \
  } while (0)

void launch_edge_attn_fused_fwd(const float* qkvs, const float* pifc,
                                const float* prpc, const long* ea, int astride,
                                const int* row_ptr, const int* csr_src,
                                float* out, float* alpha, int n, int h,
                                int heads, hipStream_t stream) {
  const int vpt = (h + PERTGNN_WAVE - 1) / PERTGNN_WAVE;
  const bool vec = (h % 256 == 0);
  if (heads != 1) {
    // shape errors come before the n == 0 shortcut: an unsupported
    // (h, heads) pair is an error whatever the graph
    const dim3 grid(ceil_div(n, WAVES_PER_BLOCK));
    const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
    const float scale =
        attn_heads_ok(h, heads) ? 1.f / std::sqrt((float)(h / heads)) : 0.f;
#define FWD_VEC(V, LPR, LPH)                                                   \
  do {                                                                         \
    if (n > 0)                                                                 \
      edge_attn_fused_fwd_kernel<V, true, float, LPR, float, float, LPH>       \
          <<<grid, block, 0, stream>>>(qkvs, pifc, prpc, ea, astride, row_ptr, \
                                       csr_src, out, alpha, n, h, scale);      \
  } while (0)
#define FWD_PCH(V, LPR, C)                                                     \
  do {                                                                         \
    if (n > 0)                                                                 \
      edge_attn_fused_fwd_kernel<V, false, float, LPR, float, float, C, true>  \
          <<<grid, block, 0, stream>>>(qkvs, pifc, prpc, ea, astride, row_ptr, \
                                       csr_src, out, alpha, n, h, scale);      \
  } while (0)
    const char* name = "edge_attn_fused launcher";
    if (vec && vpt == 4) {
      HEAD_CHAIN(FWD_VEC, 4, 64, vec_lph(h, heads, 4, 64), name);
    } else if (vec && vpt == 8) {
      HEAD_CHAIN(FWD_VEC, 8, 64, vec_lph(h, heads, 8, 64), name);
    } else if (!vec && vpt >= 1 && vpt <= 8) {
      const int c = pch_lanes(h, heads);
      switch (vpt) {
#define CASE(V) case V: HEAD_CHAIN(FWD_PCH, V, 64, c, name); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
      }
    } else {
      attn_heads_fail(name, h, heads, PERTGNN_WAVE);
    }
#undef FWD_VEC
#undef FWD_PCH
    return;
  }
  if (n == 0) return;
  const float scale = 1.f / std::sqrt((float)h);
  const dim3 grid(ceil_div(n, WAVES_PER_BLOCK));
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  switch (vpt) {
#define CASE(V)                                                                \
  case V:                                                                      \
    if (vec && (V % 4 == 0))                                                   \
      edge_attn_fused_fwd_kernel<V, true><<<grid, block, 0, stream>>>(         \
          qkvs, pifc, prpc, ea, astride, row_ptr, csr_src, out, alpha, n, h,   \
          scale);                                                              \
    else                                                                       \
      edge_attn_fused_fwd_kernel<V, false><<<grid, block, 0, stream>>>(        \
          qkvs, pifc, prpc, ea, astride, row_ptr, csr_src, out, alpha, n, h,   \
          scale);                                                              \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: pertgnn_shape_fail("edge_attn_fused launcher", "vpt", vpt);
  }
}

void launch_edge_attn_fused_bwd(const float* g, const float* qkvs,
                                const float* pifc, const float* prpc,
                                const long* ea, int astride,
                                const float* alpha, const int* row_ptr,
                                const int* csr_src, const int* col_ptr,
                                const int* csc_dst, const int* csc_eid,
                                float* dqkvs, float* de, float* dal, int n,
                                int h, long num_edges, int heads,
                                hipStream_t stream) {
  const int vpt = (h + PERTGNN_WAVE - 1) / PERTGNN_WAVE;
  const bool vec = (h % 256 == 0);
  if (heads != 1) {
    const dim3 grid(ceil_div(n, WAVES_PER_BLOCK));
    const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
    const float scale =
        attn_heads_ok(h, heads) ? 1.f / std::sqrt((float)(h / heads)) : 0.f;
#define BWD_VEC(V, LPR, LPH)                                                   \
  do {                                                                         \
    if (n > 0) {                                                               \
      edge_attn_fused_bwd_row_kernel<V, true, float, LPR, float, float, LPH>   \
          <<<grid, block, 0, stream>>>(g, qkvs, pifc, prpc, ea, astride,       \
                                       alpha, row_ptr, csr_src, dqkvs, dal,    \
                                       n, h, scale);                           \
      edge_attn_fused_bwd_col_kernel<V, true, float, float, LPR, float, LPH>   \
          <<<grid, block, 0, stream>>>(g, qkvs, alpha, dal, col_ptr, csc_dst,  \
                                       csc_eid, dqkvs, de, n, h, h);           \
    }                                                                          \
  } while (0)
#define BWD_PCH(V, LPR, C)                                                     \
  do {                                                                         \
    if (n > 0) {                                                               \
      edge_attn_fused_bwd_row_kernel<V, false, float, LPR, float, float, C,    \
                                     true>                                     \
          <<<grid, block, 0, stream>>>(g, qkvs, pifc, prpc, ea, astride,       \
                                       alpha, row_ptr, csr_src, dqkvs, dal,    \
                                       n, h, scale);                           \
      edge_attn_fused_bwd_col_kernel<V, false, float, float, LPR, float, C,    \
                                     true>                                     \
          <<<grid, block, 0, stream>>>(g, qkvs, alpha, dal, col_ptr, csc_dst,  \
                                       csc_eid, dqkvs, de, n, h, h);           \
    }                                                                          \
  } while (0)
    const char* name = "edge_attn_fused launcher";
    if (vec && vpt == 4) {
      HEAD_CHAIN(BWD_VEC, 4, 64, vec_lph(h, heads, 4, 64), name);
    } else if (vec && vpt == 8) {
      HEAD_CHAIN(BWD_VEC, 8, 64, vec_lph(h, heads, 8, 64), name);
    } else if (!vec && vpt >= 1 && vpt <= 8) {
      const int c = pch_lanes(h, heads);
      switch (vpt) {
#define CASE(V) case V: HEAD_CHAIN(BWD_PCH, V, 64, c, name); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
      }
    } else {
      attn_heads_fail(name, h, heads, PERTGNN_WAVE);
    }
#undef BWD_VEC
#undef BWD_PCH
    return;
  }
  if (n == 0) return;
  const float scale = 1.f / std::sqrt((float)h);
  const dim3 grid(ceil_div(n, WAVES_PER_BLOCK));
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  switch (vpt) {
#define CASE(V)                                                                \
  case V:                                                                      \
    if (vec && (V % 4 == 0)) {                                                 \
      edge_attn_fused_bwd_row_kernel<V, true><<<grid, block, 0, stream>>>(     \
          g, qkvs, pifc, prpc, ea, astride, alpha, row_ptr, csr_src, dqkvs,    \
          dal, n, h, scale);                                                   \
      edge_attn_fused_bwd_col_kernel<V, true><<<grid, block, 0, stream>>>(     \
          g, qkvs, alpha, dal, col_ptr, csc_dst, csc_eid, dqkvs, de, n, h, h); \
    } else {                                                                   \
      edge_attn_fused_bwd_row_kernel<V, false><<<grid, block, 0, stream>>>(    \
          g, qkvs, pifc, prpc, ea, astride, alpha, row_ptr, csr_src, dqkvs,    \
          dal, n, h, scale);                                                   \
      edge_attn_fused_bwd_col_kernel<V, false><<<grid, block, 0, stream>>>(    \
          g, qkvs, alpha, dal, col_ptr, csc_dst, csc_eid, dqkvs, de, n, h, h); \
    }                                                                          \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: pertgnn_shape_fail("edge_attn_fused launcher", "vpt", vpt);
  }
}


// ---------------------------------------------------------------------------
// bf16-qkvs launchers (activation-resident bf16 mode; requires h % 256 == 0)
// ---------------------------------------------------------------------------

// sub-wave row packing: PERT CSR rows average degree ~1.3, so a full wave
// per row is latency-bound with idle lanes.  LPR=32 (two rows per wave,
// 8 cols/lane at H=256) measured best: 14.87 vs 15.33 ms/step at LPR=64;
// LPR=16 loses it back to register pressure.  PERTGNN_ATTN_LPR overrides.
static int attn_lpr() {
  static int v = [] {
    const char* e = getenv("PERTGNN_ATTN_LPR");
    const int x = e ? atoi(e) : 32;
    return (x == 16 || x == 32 || x == 64) ? x : 32;
  }();
  return v;
}

void launch_edge_attn_fused_fwd16(const void* qkvs_v, const void* pifc_v,
                                  const void* prpc_v, int p16, const long* ea,
                                  int astride, const int* row_ptr,
                                  const int* csr_src, void* out_v, int out16,
                                  float* alpha, int n, int h, int heads,
                                  hipStream_t stream) {
  const __bf16* qkvs = (const __bf16*)qkvs_v;
  if (n == 0 && heads == 1) return;
  // with heads the shape check runs for an empty graph too (an unsupported
  // split is an error whatever the graph); FWD16 launches nothing then
  const float scale =
      attn_heads_ok(h, heads) ? 1.f / std::sqrt((float)(h / heads)) : 0.f;
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const int lpr = attn_lpr();
  const int rpb = WAVES_PER_BLOCK * (PERTGNN_WAVE / lpr);
  const dim3 grid(ceil_div(n, rpb));
  const char* name = "edge_attn_fused act16 launcher";
#define FWD16(VPT, LPR, LPH)                                                   \
  do {                                                                         \
    if (n == 0) break;                                                         \
    if (p16 && out16) {                                                        \
      edge_attn_fused_fwd_kernel<VPT, true, __bf16, LPR, __bf16, __bf16, LPH>  \
          <<<grid, block, 0, stream>>>(qkvs, (const __bf16*)pifc_v,            \
                                       (const __bf16*)prpc_v, ea, astride,     \
                                       row_ptr, csr_src, (__bf16*)out_v,       \
                                       alpha, n, h, scale);                    \
    } else if (p16) {                                                          \
      edge_attn_fused_fwd_kernel<VPT, true, __bf16, LPR, float, __bf16, LPH>   \
          <<<grid, block, 0, stream>>>(qkvs, (const __bf16*)pifc_v,            \
                                       (const __bf16*)prpc_v, ea, astride,     \
                                       row_ptr, csr_src, (float*)out_v,        \
                                       alpha, n, h, scale);                    \
    } else if (out16) {                                                        \
      edge_attn_fused_fwd_kernel<VPT, true, __bf16, LPR, __bf16, float, LPH>   \
          <<<grid, block, 0, stream>>>(qkvs, (const float*)pifc_v,             \
                                       (const float*)prpc_v, ea, astride,      \
                                       row_ptr, csr_src, (__bf16*)out_v,       \
                                       alpha, n, h, scale);                    \
    } else {                                                                   \
      edge_attn_fused_fwd_kernel<VPT, true, __bf16, LPR, float, float, LPH>    \
          <<<grid, block, 0, stream>>>(qkvs, (const float*)pifc_v,             \
                                       (const float*)prpc_v, ea, astride,      \
                                       row_ptr, csr_src, (float*)out_v,        \
                                       alpha, n, h, scale);                    \
    }                                                                          \
  } while (0)
#define FWD16_H(VPT, LPR)                                                      \
  HEAD_CHAIN(FWD16, VPT, LPR, vec_lph(h, heads, VPT, LPR), name)
  if (h == 256) {
    if (lpr == 16) FWD16_H(16, 16);
    else if (lpr == 32) FWD16_H(8, 32);
    else FWD16_H(4, 64);
  } else if (h == 512) {
    if (lpr == 16 || lpr == 32) FWD16_H(16, 32);
    else FWD16_H(8, 64);
  } else if (h % 256 == 0 && h / PERTGNN_WAVE <= 32) {
    // wider rows: single-head only (one full wave per row)
    if (heads != 1) attn_heads_fail(name, h, heads, PERTGNN_WAVE);
    const int vpt = h / PERTGNN_WAVE;
    if (vpt == 4) FWD16(4, 64, 64);
    else if (vpt == 8) FWD16(8, 64, 64);
    else if (vpt == 16) FWD16(16, 64, 64);
    else FWD16(32, 64, 64);
  } else {
    pertgnn_shape_fail("edge_attn_fused act16 launcher", "h", h);
  }
#undef FWD16_H
#undef FWD16
}

void launch_edge_attn_fused_bwd16(const void* g_v, int g16,
                                  const void* qkvs_v,
                                  const void* pifc_v, const void* prpc_v,
                                  int p16, const long* ea, int astride,
                                  const float* alpha, const int* row_ptr,
                                  const int* csr_src, const int* col_ptr,
                                  const int* csc_dst, const int* csc_eid,
                                  void* dqkvs_v, void* de_v, float* dal,
                                  int n, int h, long num_edges, int heads,
                                  hipStream_t stream, const AttnBnBwd* bn,
                                  const AttnPoolBwd* pool) {
  const __bf16* qkvs = (const __bf16*)qkvs_v;
  __bf16* dqkvs = (__bf16*)dqkvs_v;
  __bf16* de = (__bf16*)de_v;
  // pool (may be null): there is no g_v; both kernels form the fp32 gradient
  // of a node from the pattern pool's backward (the fp32-g branches only)
  if (pool && (g16 || bn))
    pertgnn_shape_fail("edge_attn_fused act16 launcher",
                       bn ? "pool with bn, h" : "pool with bf16 g, h", h);
  const AttnPoolBwd poolk = pool ? *pool : AttnPoolBwd{};
  // bn (may be null): g_v is the gradient of the BN OUTPUT; the row kernel
  // applies the BN backward to each row it loads and the col kernel gathers
  // the result from the dskip columns the row kernel wrote (bf16 g only)
  if (bn && (!g16 || (h != 256 && h != 512)))
    pertgnn_shape_fail("edge_attn_fused act16 launcher",
                       g16 ? "bn, h" : "bn with fp32 g, h", h);
  const AttnBnBwd bnk = bn ? *bn : AttnBnBwd{};
  const __bf16* gcol = bn ? dqkvs + 3L * h : (const __bf16*)g_v;
  const long gld = bn ? 4L * h : h;
  if (n == 0 && heads == 1) return;
  const float scale =
      attn_heads_ok(h, heads) ? 1.f / std::sqrt((float)(h / heads)) : 0.f;
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const int lpr = attn_lpr();
  const int rpb = WAVES_PER_BLOCK * (PERTGNN_WAVE / lpr);
  const dim3 grid(ceil_div(n, rpb));
  const char* name = "edge_attn_fused act16 launcher";
// fp32 (or, POOL, no) upstream gradient: the last conv's backward
#define BWD16_G32(VPT, LPR, LPH, PT, POOL)                                     \
  do {                                                                         \
    edge_attn_fused_bwd_row_kernel<VPT, true, __bf16, LPR, float, PT, LPH,     \
                                   false, POOL>                                \
        <<<grid, block, 0, stream>>>((const float*)g_v, qkvs,                  \
                                     (const PT*)pifc_v, (const PT*)prpc_v, ea, \
                                     astride, alpha, row_ptr, csr_src, dqkvs,  \
                                     dal, n, h, scale, AttnBnBwd{}, poolk);    \
    edge_attn_fused_bwd_col_kernel<VPT, true, __bf16, __bf16, LPR, float,      \
                                   LPH, false, POOL>                           \
        <<<grid, block, 0, stream>>>((const float*)g_v, qkvs, alpha, dal,      \
                                     col_ptr, csc_dst, csc_eid, dqkvs, de, n,  \
                                     h, h, poolk);                             \
  } while (0)
#define BWD16(VPT, LPR, LPH)                                                   \
  do {                                                                         \
    if (n == 0) break;                                                         \
    if (g16 && p16) {                                                          \
      edge_attn_fused_bwd_row_kernel<VPT, true, __bf16, LPR, __bf16, __bf16,   \
                                     LPH>                                      \
          <<<grid, block, 0, stream>>>((const __bf16*)g_v, qkvs,               \
                                       (const __bf16*)pifc_v,                  \
                                       (const __bf16*)prpc_v,                  \
                                       ea, astride, alpha, row_ptr, csr_src,   \
                                       dqkvs, dal, n, h, scale, bnk);          \
      edge_attn_fused_bwd_col_kernel<VPT, true, __bf16, __bf16, LPR, __bf16,   \
                                     LPH>                                      \
          <<<grid, block, 0, stream>>>(gcol, qkvs, alpha, dal, col_ptr,        \
                                       csc_dst, csc_eid, dqkvs, de, n, h,      \
                                       gld);                                   \
    } else if (g16) {                                                          \
      edge_attn_fused_bwd_row_kernel<VPT, true, __bf16, LPR, __bf16, float,    \
                                     LPH>                                      \
          <<<grid, block, 0, stream>>>((const __bf16*)g_v, qkvs,               \
                                       (const float*)pifc_v,                   \
                                       (const float*)prpc_v,                   \
                                       ea, astride, alpha, row_ptr, csr_src,   \
                                       dqkvs, dal, n, h, scale, bnk);          \
      edge_attn_fused_bwd_col_kernel<VPT, true, __bf16, __bf16, LPR, __bf16,   \
                                     LPH>                                      \
          <<<grid, block, 0, stream>>>(gcol, qkvs, alpha, dal, col_ptr,        \
                                       csc_dst, csc_eid, dqkvs, de, n, h,      \
                                       gld);                                   \
    } else if (p16) {                                                          \
      /* fp32 upstream grad (the last conv's out16=false) + bf16 P tables — \
         reading the tables at the wrong width over-reads 2x (OOB) */        \
      if (pool) BWD16_G32(VPT, LPR, LPH, __bf16, true);                        \
      else BWD16_G32(VPT, LPR, LPH, __bf16, false);                            \
    } else {                                                                   \
      if (pool) BWD16_G32(VPT, LPR, LPH, float, true);                         \
      else BWD16_G32(VPT, LPR, LPH, float, false);                             \
    }                                                                          \
  } while (0)
#define BWD16_H(VPT, LPR)                                                      \
  HEAD_CHAIN(BWD16, VPT, LPR, vec_lph(h, heads, VPT, LPR), name)
  if (h == 256) {
    if (lpr == 16) BWD16_H(16, 16);
    else if (lpr == 32) BWD16_H(8, 32);
    else BWD16_H(4, 64);
  } else if (h == 512) {
    if (lpr == 16 || lpr == 32) BWD16_H(16, 32);
    else BWD16_H(8, 64);
  } else if (h % 256 == 0 && h / PERTGNN_WAVE <= 32) {
    if (heads != 1) attn_heads_fail(name, h, heads, PERTGNN_WAVE);
    const int vpt = h / PERTGNN_WAVE;
    if (vpt == 4) BWD16(4, 64, 64);
    else if (vpt == 8) BWD16(8, 64, 64);
    else if (vpt == 16) BWD16(16, 64, 64);
    else BWD16(32, 64, 64);
  } else {
    pertgnn_shape_fail("edge_attn_fused act16 launcher", "h", h);
  }
#undef BWD16_H
#undef BWD16
#undef BWD16_G32
}


// ---------------------------------------------------------------------------
// inference launchers (forward-only kernel, folded BN+ReLU epilogue); same
// shape coverage and kernel selection as the two training forward launchers
// ---------------------------------------------------------------------------

void launch_edge_attn_fused_infer(const float* qkvs, const float* pifc,
                                  const float* prpc, const long* ea,
                                  int astride, const int* row_ptr,
                                  const int* csr_src, const float* bn_scale,
                                  const float* bn_shift, int relu, float* out,
                                  int n, int h, int heads,
                                  hipStream_t stream) {
  const int vpt = (h + PERTGNN_WAVE - 1) / PERTGNN_WAVE;
  const bool vec = (h % 256 == 0);
  if (heads != 1) {
    const dim3 grid(ceil_div(n, WAVES_PER_BLOCK));
    const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
    const float scale =
        attn_heads_ok(h, heads) ? 1.f / std::sqrt((float)(h / heads)) : 0.f;
#define INF_VEC(V, LPR, LPH)                                                   \
  do {                                                                         \
    if (n > 0)                                                                 \
      edge_attn_fused_infer_kernel<V, true, float, LPR, float, float, LPH>     \
          <<<grid, block, 0, stream>>>(qkvs, pifc, prpc, ea, astride, row_ptr, \
                                       csr_src, bn_scale, bn_shift, relu, out, \
                                       n, h, scale);                           \
  } while (0)
#define INF_PCH(V, LPR, C)                                                     \
  do {                                                                         \
    if (n > 0)                                                                 \
      edge_attn_fused_infer_kernel<V, false, float, LPR, float, float, C,      \
                                   true>                                       \
          <<<grid, block, 0, stream>>>(qkvs, pifc, prpc, ea, astride, row_ptr, \
                                       csr_src, bn_scale, bn_shift, relu, out, \
                                       n, h, scale);                           \
  } while (0)
    const char* name = "edge_attn_fused infer launcher";
    if (vec && vpt == 4) {
      HEAD_CHAIN(INF_VEC, 4, 64, vec_lph(h, heads, 4, 64), name);
    } else if (vec && vpt == 8) {
      HEAD_CHAIN(INF_VEC, 8, 64, vec_lph(h, heads, 8, 64), name);
    } else if (!vec && vpt >= 1 && vpt <= 8) {
      const int c = pch_lanes(h, heads);
      switch (vpt) {
#define CASE(V) case V: HEAD_CHAIN(INF_PCH, V, 64, c, name); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
      }
    } else {
      attn_heads_fail(name, h, heads, PERTGNN_WAVE);
    }
#undef INF_VEC
#undef INF_PCH
    return;
  }
  if (n == 0) return;
  const float scale = 1.f / std::sqrt((float)h);
  const dim3 grid(ceil_div(n, WAVES_PER_BLOCK));
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  switch (vpt) {
#define CASE(V)                                                                \
  case V:                                                                      \
    if (vec && (V % 4 == 0))                                                   \
      edge_attn_fused_infer_kernel<V, true><<<grid, block, 0, stream>>>(       \
          qkvs, pifc, prpc, ea, astride, row_ptr, csr_src, bn_scale,           \
          bn_shift, relu, out, n, h, scale);                                   \
    else                                                                       \
      edge_attn_fused_infer_kernel<V, false><<<grid, block, 0, stream>>>(      \
          qkvs, pifc, prpc, ea, astride, row_ptr, csr_src, bn_scale,           \
          bn_shift, relu, out, n, h, scale);                                   \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default: pertgnn_shape_fail("edge_attn_fused infer launcher", "vpt", vpt);
  }
}

void launch_edge_attn_fused_infer16(const void* qkvs_v, const void* pifc_v,
                                    const void* prpc_v, int p16,
                                    const long* ea, int astride,
                                    const int* row_ptr, const int* csr_src,
                                    const float* bn_scale,
                                    const float* bn_shift, int relu,
                                    void* out_v, int out16, int n, int h,
                                    int heads, hipStream_t stream) {
  const __bf16* qkvs = (const __bf16*)qkvs_v;
  if (n == 0 && heads == 1) return;
  const float scale =
      attn_heads_ok(h, heads) ? 1.f / std::sqrt((float)(h / heads)) : 0.f;
  const dim3 block(WAVES_PER_BLOCK * PERTGNN_WAVE);
  const int lpr = attn_lpr();
  const int rpb = WAVES_PER_BLOCK * (PERTGNN_WAVE / lpr);
  const dim3 grid(ceil_div(n, rpb));
  const char* name = "edge_attn_fused infer act16 launcher";
#define INF16(VPT, LPR, LPH)                                                   \
  do {                                                                         \
    if (n == 0) break;                                                         \
    if (p16 && out16) {                                                        \
      edge_attn_fused_infer_kernel<VPT, true, __bf16, LPR, __bf16, __bf16,     \
                                   LPH>                                        \
          <<<grid, block, 0, stream>>>(qkvs, (const __bf16*)pifc_v,            \
                                       (const __bf16*)prpc_v, ea, astride,     \
                                       row_ptr, csr_src, bn_scale, bn_shift,   \
                                       relu, (__bf16*)out_v, n, h, scale);     \
    } else if (p16) {                                                          \
      edge_attn_fused_infer_kernel<VPT, true, __bf16, LPR, float, __bf16,      \
                                   LPH>                                        \
          <<<grid, block, 0, stream>>>(qkvs, (const __bf16*)pifc_v,            \
                                       (const __bf16*)prpc_v, ea, astride,     \
                                       row_ptr, csr_src, bn_scale, bn_shift,   \
                                       relu, (float*)out_v, n, h, scale);      \
    } else if (out16) {                                                        \
      edge_attn_fused_infer_kernel<VPT, true, __bf16, LPR, __bf16, float,      \
                                   LPH>                                        \
          <<<grid, block, 0, stream>>>(qkvs, (const float*)pifc_v,             \
                                       (const float*)prpc_v, ea, astride,      \
                                       row_ptr, csr_src, bn_scale, bn_shift,   \
                                       relu, (__bf16*)out_v, n, h, scale);     \
    } else {                                                                   \
      edge_attn_fused_infer_kernel<VPT, true, __bf16, LPR, float, float,       \
                                   LPH>                                        \
          <<<grid, block, 0, stream>>>(qkvs, (const float*)pifc_v,             \
                                       (const float*)prpc_v, ea, astride,      \
                                       row_ptr, csr_src, bn_scale, bn_shift,   \
                                       relu, (float*)out_v, n, h, scale);      \
    }                                                                          \
  } while (0)
#define INF16_H(VPT, LPR)                                                      \
  HEAD_CHAIN(INF16, VPT, LPR, vec_lph(h, heads, VPT, LPR), name)
  if (h == 256) {
    if (lpr == 16) INF16_H(16, 16);
    else if (lpr == 32) INF16_H(8, 32);
    else INF16_H(4, 64);
  } else if (h == 512) {
    if (lpr == 16 || lpr == 32) INF16_H(16, 32);
    else INF16_H(8, 64);
  } else if (h % 256 == 0 && h / PERTGNN_WAVE <= 32) {
    if (heads != 1) attn_heads_fail(name, h, heads, PERTGNN_WAVE);
    const int vpt = h / PERTGNN_WAVE;
    if (vpt == 4) INF16(4, 64, 64);
    else if (vpt == 8) INF16(8, 64, 64);
    else if (vpt == 16) INF16(16, 64, 64);
    else INF16(32, 64, 64);
  } else {
    pertgnn_shape_fail("edge_attn_fused infer act16 launcher", "h", h);
  }
#undef INF16_H
#undef INF16
}
