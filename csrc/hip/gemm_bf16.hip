// bf16-compute GEMM path (gfx950): fp32 operands in HBM, rounded to bf16
// during LDS staging, v_mfma_f32_16x16x32_bf16 matrix cores (≈2 PF ceiling,
// 16x the f32-MFMA rate), fp32 accumulate, fp32 output.  This is the
// mixed-precision mode of BASELINE configs 2/5: memory traffic identical to
// the f32 path (activations stay fp32 end-to-end), only the matmul operands
// are bf16-rounded.
//
// LDS layout: [free][BK+PAD] bf16 rows (k-contiguous), so each lane's MFMA
// fragment (8 consecutive k) is ONE ds_read_b128; the +8-element row pad
// makes the 16-lane fragment reads conflict-free (guide §6 G4).

#include "common.h"
#include "launchers.h"
#include "gemm_dispatch.h"

// PERTGNN_DETERMINISTIC=1: collapse split-K wgrad to one slice so the dw/db
// reduction order is fixed (read per call — tests flip it at runtime)
static inline bool pertgnn_deterministic() {
  const char* e = getenv("PERTGNN_DETERMINISTIC");
  return e && e[0] == '1';
}
#include <cstdlib>

#define BGEMM_PAD 8
#define BGEMM_THREADS 256

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

// element-type traits: bf16 and fp16 share the whole kernel structure; only
// the packed vector types and the MFMA intrinsic differ.
template <typename T16> struct Vec16;
template <> struct Vec16<__bf16> {
  using v4 = bf16x4;
  using v8 = bf16x8;
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Vec16<_Float16> {
  using v4 = f16x4;
  using v8 = f16x8;
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

template <typename T16>
__device__ __forceinline__ typename Vec16<T16>::v4 pack4(float a, float b,
                                                         float c, float d) {
  typename Vec16<T16>::v4 r;
  r[0] = (T16)a; r[1] = (T16)b; r[2] = (T16)c; r[3] = (T16)d;
  return r;
}

// 4 consecutive source elements -> float[4] (vector load for both dtypes)
__device__ __forceinline__ void ld4(const float* p, float (&v)[4]) {
  *reinterpret_cast<f32x4*>(v) = *reinterpret_cast<const f32x4*>(p);
}
__device__ __forceinline__ void ld4(const __bf16* p, float (&v)[4]) {
  const bf16x4 b = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
  for (int u = 0; u < 4; ++u) v[u] = (float)b[u];
}
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const __bf16* p) { return (float)*p; }

// global [free][contract] (contract-minor) -> LDS [free][BK+PAD]
// 4 bf16 packed into one 8-byte LDS write (scalar u16 LDS writes are ~2x
// slower — guide G13 applies to LDS too).
//
// Split into load() / commit() so the mainloop can ISSUE the next tile's
// global loads, run the MFMA work on the current LDS buffer while they are
// in flight, and only then wait + write LDS: the fused form stalled every
// wave on s_waitcnt(vmcnt) BEFORE any MFMA issued (PMC: 72% SQ_WAIT_ANY on
// the NT kernel).
template <int BF, int BK, typename T16, typename TA,
          int THREADS = BGEMM_THREADS>
struct StageCmin {
  static constexpr int LDW = BK + BGEMM_PAD;
  static constexpr int QUADS = BK / 4;
  static constexpr int FSTEP = THREADS / QUADS;
  static constexpr int HALVES = BF / FSTEP;
  float v[HALVES][4];

  __device__ __forceinline__ void load(const TA* __restrict__ g, long ld,
                                       int free0, int contract0, int free_max,
                                       int contract_max) {
    const int t = threadIdx.x;
    const int f = t / QUADS;
    const int cq = (t % QUADS) * 4;
    const bool interior = (free0 + BF <= free_max) &&
                          (contract0 + BK <= contract_max);
    const bool aligned = (ld & 3) == 0;
    // path choice HOISTED outside the loops: a branch inside the staging
    // loop makes hipcc emit per-element load+vmcnt(0) chains
    // (guide §5 ".s-level traps" (c))
    if (interior && aligned) {
#pragma unroll
      for (int half = 0; half < HALVES; ++half)
        ld4(&g[(long)(free0 + f + half * FSTEP) * ld + contract0 + cq],
            v[half]);
    } else if (interior) {  // odd leading dim: unchecked scalars
#pragma unroll
      for (int half = 0; half < HALVES; ++half) {
        const TA* row =
            &g[(long)(free0 + f + half * FSTEP) * ld + contract0 + cq];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[half][u] = ld1(row + u);
      }
    } else {
#pragma unroll
      for (int half = 0; half < HALVES; ++half) {
        const int gf = free0 + f + half * FSTEP;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int gc = contract0 + cq + u;
          v[half][u] = (gf < free_max && gc < contract_max)
                           ? ld1(&g[(long)gf * ld + gc])
                           : 0.f;
        }
      }
    }
  }

  __device__ __forceinline__ void commit(T16* lds) const {
    const int t = threadIdx.x;
    const int f = t / QUADS;
    const int cq = (t % QUADS) * 4;
#pragma unroll
    for (int half = 0; half < HALVES; ++half)
      *reinterpret_cast<typename Vec16<T16>::v4*>(
          &lds[(f + half * FSTEP) * LDW + cq]) =
          pack4<T16>(v[half][0], v[half][1], v[half][2], v[half][3]);
  }
};

template <int BF, int BK, typename T16, int THREADS = BGEMM_THREADS,
          typename TA>
__device__ __forceinline__ void bstage_cmin(const TA* __restrict__ g,
                                            long ld, int free0, int contract0,
                                            int free_max, int contract_max,
                                            T16* lds) {
  StageCmin<BF, BK, T16, TA, THREADS> s;
  s.load(g, ld, free0, contract0, free_max, contract_max);
  s.commit(lds);
}

// global [contract][free] (contract-major) -> LDS [free][BK+PAD]: each thread
// transposes a 4x4 block in registers (4 coalesced f32x4 loads from 4
// contract rows), then writes 4 packed 8-byte LDS rows.  Split load/commit
// for the same software-pipelining reason as StageCmin.
template <int BF, int BK, typename T16, typename TA,
          int THREADS = BGEMM_THREADS>
struct StageCmaj {
  static constexpr int LDW = BK + BGEMM_PAD;
  static constexpr int FQUADS = BF / 4;
  static constexpr int CSTEP = (THREADS / FQUADS) * 4;
  static constexpr int HALVES = (BK > CSTEP ? BK / CSTEP : 1);
  // with more threads than BK/4 * FQUADS lanes of work, the surplus threads
  // idle through staging (ACTIVE guarded below) but still hit the barrier
  static constexpr bool SURPLUS = CSTEP > BK;
  float v[HALVES][4][4];

  __device__ __forceinline__ void load(const TA* __restrict__ g, long ld,
                                       int contract0, int free0,
                                       int contract_max, int free_max) {
    const int t = threadIdx.x;
    const int cb = (t / FQUADS) * 4;
    const int fq = (t % FQUADS) * 4;
    if (SURPLUS && cb >= BK) return;
    const bool interior = (contract0 + BK <= contract_max) &&
                          (free0 + BF <= free_max);
    const bool aligned = ((ld & 3) == 0) && ((free0 & 3) == 0);
    // path choice hoisted outside the loops (guide §5 ".s-level traps" (c))
    if (interior && aligned) {
#pragma unroll
      for (int half = 0; half < HALVES; ++half)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          ld4(&g[(long)(contract0 + cb + half * CSTEP + u) * ld + free0 + fq],
              v[half][u]);
    } else if (interior) {
#pragma unroll
      for (int half = 0; half < HALVES; ++half)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const TA* row =
              &g[(long)(contract0 + cb + half * CSTEP + u) * ld + free0 + fq];
#pragma unroll
          for (int w = 0; w < 4; ++w) v[half][u][w] = ld1(row + w);
        }
    } else {
#pragma unroll
      for (int half = 0; half < HALVES; ++half) {
        const int cc = cb + half * CSTEP;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int gc = contract0 + cc + u;
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            const int gf = free0 + fq + w;
            v[half][u][w] = (gc < contract_max && gf < free_max)
                                ? ld1(&g[(long)gc * ld + gf])
                                : 0.f;
          }
        }
      }
    }
  }

  __device__ __forceinline__ void commit(T16* lds) const {
    const int t = threadIdx.x;
    const int cb = (t / FQUADS) * 4;
    const int fq = (t % FQUADS) * 4;
    if (SURPLUS && cb >= BK) return;
#pragma unroll
    for (int half = 0; half < HALVES; ++half)
#pragma unroll
      for (int w = 0; w < 4; ++w)
        *reinterpret_cast<typename Vec16<T16>::v4*>(
            &lds[(fq + w) * LDW + cb + half * CSTEP]) =
            pack4<T16>(v[half][0][w], v[half][1][w], v[half][2][w],
                       v[half][3][w]);
  }

  // what commit() rounded away: x - (float)(T16)x, itself rounded to T16.
  // An MFMA over this image added to the one over commit()'s carries the
  // operand to ~16 mantissa bits (grouped P-table dgrad, tiny tables).
  __device__ __forceinline__ void commit_lo(T16* lds) const {
    const int t = threadIdx.x;
    const int cb = (t / FQUADS) * 4;
    const int fq = (t % FQUADS) * 4;
    if (SURPLUS && cb >= BK) return;
    const auto lo = [](float x) { return x - (float)(T16)x; };
#pragma unroll
    for (int half = 0; half < HALVES; ++half)
#pragma unroll
      for (int w = 0; w < 4; ++w)
        *reinterpret_cast<typename Vec16<T16>::v4*>(
            &lds[(fq + w) * LDW + cb + half * CSTEP]) =
            pack4<T16>(lo(v[half][0][w]), lo(v[half][1][w]),
                       lo(v[half][2][w]), lo(v[half][3][w]));
  }
};

template <int BF, int BK, typename T16, int THREADS = BGEMM_THREADS,
          typename TA>
__device__ __forceinline__ void bstage_cmaj(const TA* __restrict__ g,
                                            long ld, int contract0, int free0,
                                            int contract_max, int free_max,
                                            T16* lds) {
  StageCmaj<BF, BK, T16, TA, THREADS> s;
  s.load(g, ld, contract0, free0, contract_max, free_max);
  s.commit(lds);
}

// ---------------------------------------------------------------------------
// wave tile: FM x FN fragments of 16x16; K-step 32 per MFMA, BK=64 = 2 steps
// fragment layout (mfma_f32_16x16x32_bf16): lane l holds 8 k-consecutive
// elements at k = (l>>4)*8 of row/col (l&15); C/D: col=l&15, row=(l>>4)*4+r.
// ---------------------------------------------------------------------------

template <int FM, int FN, int BK, typename T16>
struct BWaveTile {
  f32x4 acc[FM][FN];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
  }
  __device__ __forceinline__ void mma(const T16* lds_a, const T16* lds_b,
                                      int wm, int wn, int lane) {
    constexpr int LDW = BK + BGEMM_PAD;
    const int fi = lane & 15;
    const int fk = (lane >> 4) * 8;
#pragma unroll
    for (int s = 0; s < BK / 32; ++s) {
      const int k = s * 32 + fk;
      using v8 = typename Vec16<T16>::v8;
      v8 a[FM], b[FN];
#pragma unroll
      for (int mi = 0; mi < FM; ++mi)
        a[mi] = *reinterpret_cast<const v8*>(
            &lds_a[(wm + mi * 16 + fi) * LDW + k]);
#pragma unroll
      for (int ni = 0; ni < FN; ++ni)
        b[ni] = *reinterpret_cast<const v8*>(
            &lds_b[(wn + ni * 16 + fi) * LDW + k]);
#pragma unroll
      for (int mi = 0; mi < FM; ++mi)
#pragma unroll
        for (int ni = 0; ni < FN; ++ni)
          acc[mi][ni] = Vec16<T16>::mfma(a[mi], b[ni], acc[mi][ni]);
    }
  }
  template <typename TO>
  __device__ __forceinline__ void store(TO* __restrict__ c, long ldc,
                                        int row0, int col0, int m_max,
                                        int n_max, const float* bias, int relu,
                                        int lane) {
    const int fcol = lane & 15;
    const int frow = (lane >> 4) * 4;
#pragma unroll
    for (int mi = 0; mi < FM; ++mi)
#pragma unroll
      for (int ni = 0; ni < FN; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + mi * 16 + frow + r;
          const int col = col0 + ni * 16 + fcol;
          if (row < m_max && col < n_max) {
            float v = acc[mi][ni][r];
            if (bias) v += bias[col];
            if (relu) v = fmaxf(v, 0.f);
            c[(long)row * ldc + col] = (TO)v;
          }
        }
  }
};

// ---------------------------------------------------------------------------
// kernels — same three layouts as the f32 suite
// ---------------------------------------------------------------------------

template <int BM, int BN, int BK = 64, typename T16 = __bf16,
          typename TA = float, typename TO = float,
          int THREADS = BGEMM_THREADS>
__launch_bounds__(THREADS)
__global__ void gemm_bf16_nt_kernel(const TA* __restrict__ a,
                                    const float* __restrict__ b,
                                    const float* __restrict__ bias,
                                    TO* __restrict__ c, int m, int n, int k,
                                    int relu) {
  constexpr int LDW = BK + BGEMM_PAD;
  constexpr int WCOL = THREADS / PERTGNN_WAVE / 2;  // wave columns
  constexpr int FM = (BM / 2) / 16, FN = (BN / WCOL) / 16;
  __shared__ T16 lds_a[2][BM * LDW];
  __shared__ T16 lds_b[2][BN * LDW];
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tiles_n = (n + BN - 1) / BN;
  const int m0 = (bid / tiles_n) * BM;
  const int n0 = (bid % tiles_n) * BN;
  const int wave = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int wm = (wave / WCOL) * (BM / 2);
  const int wn = (wave % WCOL) * (BN / WCOL);

  BWaveTile<FM, FN, BK, T16> wt;
  wt.zero();
  int buf = 0;
  bstage_cmin<BM, BK, T16, THREADS>(a, k, m0, 0, m, k, lds_a[0]);
  bstage_cmin<BN, BK, T16, THREADS>(b, k, n0, 0, n, k, lds_b[0]);
  __syncthreads();
  StageCmin<BM, BK, T16, TA, THREADS> sa;
  StageCmin<BN, BK, T16, float, THREADS> sb;
  for (int k0 = BK; k0 < k; k0 += BK) {
    sa.load(a, k, m0, k0, m, k);        // issue loads…
    sb.load(b, k, n0, k0, n, k);
    wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);  // …MFMA while in flight
    sa.commit(lds_a[buf ^ 1]);
    sb.commit(lds_b[buf ^ 1]);
    __syncthreads();
    buf ^= 1;
  }
  wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
  wt.store(c, n, m0 + wm, n0 + wn, m, n, bias, relu, lane);
}

template <int BM, int BN, int BK = 64, typename T16 = __bf16,
          typename TA = float, typename TO = float,
          int THREADS = BGEMM_THREADS>
__launch_bounds__(THREADS, 3)
__global__ void gemm_bf16_nn_kernel(const TA* __restrict__ a,
                                    const float* __restrict__ b,
                                    const float* __restrict__ bias,
                                    TO* __restrict__ c, int m, int n,
                                    int k2, int relu) {
  constexpr int LDW = BK + BGEMM_PAD;
  constexpr int WCOL = THREADS / PERTGNN_WAVE / 2;
  constexpr int FM = (BM / 2) / 16, FN = (BN / WCOL) / 16;
  __shared__ T16 lds_a[2][BM * LDW];
  __shared__ T16 lds_b[2][BN * LDW];
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tiles_n = (k2 + BN - 1) / BN;
  const int m0 = (bid / tiles_n) * BM;
  const int n0 = (bid % tiles_n) * BN;
  const int wave = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int wm = (wave / WCOL) * (BM / 2);
  const int wn = (wave % WCOL) * (BN / WCOL);

  BWaveTile<FM, FN, BK, T16> wt;
  wt.zero();
  int buf = 0;
  bstage_cmin<BM, BK, T16, THREADS>(a, n, m0, 0, m, n, lds_a[0]);
  bstage_cmaj<BN, BK, T16, THREADS>(b, k2, 0, n0, n, k2, lds_b[0]);
  __syncthreads();
  StageCmin<BM, BK, T16, TA, THREADS> sa;
  StageCmaj<BN, BK, T16, float, THREADS> sb;
  for (int c0 = BK; c0 < n; c0 += BK) {
    sa.load(a, n, m0, c0, m, n);
    sb.load(b, k2, c0, n0, n, k2);
    wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
    sa.commit(lds_a[buf ^ 1]);
    sb.commit(lds_b[buf ^ 1]);
    __syncthreads();
    buf ^= 1;
  }
  wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
  wt.store(c, k2, m0 + wm, n0 + wn, m, k2, bias, relu, lane);
}

template <int BM, int BN, int BK = 64, typename T16 = __bf16,
          typename TA = float, typename TB = float,
          int THREADS = BGEMM_THREADS, bool ACC = false>
__launch_bounds__(THREADS)
__global__ void gemm_bf16_tn_kernel(const TA* __restrict__ a,
                                    const TB* __restrict__ b,
                                    float* __restrict__ c,
                                    float* __restrict__ dbias, int m, int n,
                                    int k2, int slices) {
  constexpr int LDW = BK + BGEMM_PAD;
  constexpr int WCOL = THREADS / PERTGNN_WAVE / 2;
  constexpr int FM = (BM / 2) / 16, FN = (BN / WCOL) / 16;
  __shared__ T16 lds_a[2][BM * LDW];
  __shared__ T16 lds_b[2][BN * LDW];
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tiles_k = (k2 + BN - 1) / BN;
  const int tile_id = bid / slices;
  const int slice = bid % slices;
  const int n0 = (tile_id / tiles_k) * BM;
  const int k0 = (tile_id % tiles_k) * BN;
  if (n0 >= n) return;
  const int wave = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int wm = (wave / WCOL) * (BM / 2);
  const int wn = (wave % WCOL) * (BN / WCOL);

  const int per_slice =
      ((m + slices - 1) / slices + BK - 1) / BK * BK;
  const int c_beg = slice * per_slice;
  const int c_end = min(m, c_beg + per_slice);
  if (c_beg >= c_end) return;

  BWaveTile<FM, FN, BK, T16> wt;
  wt.zero();
  // fused bias grad: sum the STAGED bf16 A (=g) tile columns.  NOTE: this
  // sums bf16-rounded g — for exact-f32 db the caller uses the f32 path.
  const bool do_bias = (dbias != nullptr) && (k0 == 0);
  float dbsum = 0.f;
  const int bcol = threadIdx.x;
  int buf = 0;
  bstage_cmaj<BM, BK, T16, THREADS>(a, n, c_beg, n0, c_end, n, lds_a[0]);
  bstage_cmaj<BN, BK, T16, THREADS>(b, k2, c_beg, k0, c_end, k2, lds_b[0]);
  __syncthreads();
  StageCmaj<BM, BK, T16, TA, THREADS> sa;
  StageCmaj<BN, BK, T16, TB, THREADS> sb;
  for (int cc = c_beg + BK; cc < c_end; cc += BK) {
    sa.load(a, n, cc, n0, c_end, n);
    sb.load(b, k2, cc, k0, c_end, k2);
    wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
    if (do_bias && bcol < BM)
#pragma unroll
      for (int r = 0; r < BK; ++r)
        dbsum += (float)lds_a[buf][bcol * LDW + r];
    sa.commit(lds_a[buf ^ 1]);
    sb.commit(lds_b[buf ^ 1]);
    __syncthreads();
    buf ^= 1;
  }
  wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
  if (do_bias && bcol < BM) {
#pragma unroll
    for (int r = 0; r < BK; ++r)
      dbsum += (float)lds_a[buf][bcol * LDW + r];
    if (n0 + bcol < n) atomicAdd(&dbias[n0 + bcol], dbsum);
  }

  const int fcol = lane & 15;
  const int frow = (lane >> 4) * 4;
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + wm + mi * 16 + frow + r;
        const int col = k0 + wn + ni * 16 + fcol;
        if (row < n && col < k2) {
          if (slices != 1)
            atomicAdd(&c[(long)row * k2 + col], wt.acc[mi][ni][r]);
          else if (ACC)  // gradient sink: this thread owns the element
            c[(long)row * k2 + col] += wt.acc[mi][ni][r];
          else
            c[(long)row * k2 + col] = wt.acc[mi][ni][r];
        }
      }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

static int gemm_bk() {
  static int bk = [] {
    const char* e = getenv("PERTGNN_GEMM_BK");
    return (e && atoi(e) == 64) ? 64 : 32;  // default 32 (4 blocks/CU)
  }();
  return bk;
}

static bool gemm_t512() {  // 8-wave (512-thread) blocks for the a16 GEMMs
  static bool v = [] {
    const char* e = getenv("PERTGNN_GEMM_T512");
    return e && atoi(e) == 1;
  }();
  return v;
}

static bool gemm_n64() {  // narrow-BN experiment: 128x64 tiles, 4 waves/SIMD
  static bool v = [] {
    const char* e = getenv("PERTGNN_GEMM_N64");
    return e && atoi(e) == 1;
  }();
  return v;
}

void launch_gemm_bf16_nt(const float* a, const float* b, const float* bias,
                         float* c, int m, int n, int k, bool relu,
                         hipStream_t s) {
  if (gemm_dispatch::tile128(m, n)) {
    if (gemm_n64()) {
      const int grid = ((m + 127) / 128) * ((n + 63) / 64);
      gemm_bf16_nt_kernel<128, 64, 32><<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(
          a, b, bias, c, m, n, k, relu ? 1 : 0);
      return;
    }
    const int grid = ((m + 127) / 128) * ((n + 127) / 128);
    if (gemm_bk() == 32)
      gemm_bf16_nt_kernel<128, 128, 32><<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(
          a, b, bias, c, m, n, k, relu ? 1 : 0);
    else
      gemm_bf16_nt_kernel<128, 128, 64><<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(
          a, b, bias, c, m, n, k, relu ? 1 : 0);
  } else {
    const int grid = ((m + 63) / 64) * ((n + 63) / 64);
    gemm_bf16_nt_kernel<64, 64><<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(
        a, b, bias, c, m, n, k, relu ? 1 : 0);
  }
}

void launch_gemm_bf16_nn(const float* a, const float* b, const float* bias,
                         float* c, int m, int n, int k2, bool relu,
                         hipStream_t s) {
  if (gemm_dispatch::tile128(m, k2)) {
    if (gemm_n64()) {
      const int grid = ((m + 127) / 128) * ((k2 + 63) / 64);
      gemm_bf16_nn_kernel<128, 64, 32><<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(
          a, b, bias, c, m, n, k2, relu ? 1 : 0);
      return;
    }
    const int grid = ((m + 127) / 128) * ((k2 + 127) / 128);
    if (gemm_bk() == 32)
      gemm_bf16_nn_kernel<128, 128, 32><<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(
          a, b, bias, c, m, n, k2, relu ? 1 : 0);
    else
      gemm_bf16_nn_kernel<128, 128, 64><<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(
          a, b, bias, c, m, n, k2, relu ? 1 : 0);
  } else {
    const int grid = ((m + 63) / 64) * ((k2 + 63) / 64);
    gemm_bf16_nn_kernel<64, 64><<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(
        a, b, bias, c, m, n, k2, relu ? 1 : 0);
  }
}

void launch_gemm_bf16_tn(const float* a, const float* b, float* c,
                         float* dbias, int m, int n, int k2, hipStream_t s) {
  const bool big = gemm_dispatch::tn_tile128(n, k2);
  const int tiles = gemm_dispatch::tn_tiles(n, k2);
  const int slices =
      gemm_dispatch::tn_slices(m, tiles, 64, pertgnn_deterministic());
  if (slices > 1)
    HIP_CHECK(hipMemsetAsync(c, 0, (long)n * k2 * sizeof(float), s));
  if (dbias) HIP_CHECK(hipMemsetAsync(dbias, 0, n * sizeof(float), s));
  if (big) {
    if (gemm_bk() == 32)
      gemm_bf16_tn_kernel<128, 128, 32>
          <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                                m, n, k2,
                                                                slices);
    else
      gemm_bf16_tn_kernel<128, 128, 64>
          <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                                m, n, k2,
                                                                slices);
  } else
    gemm_bf16_tn_kernel<64, 64>
        <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                              m, n, k2,
                                                              slices);
}


// ---------------------------------------------------------------------------
// fp16 launchers (BASELINE config 5 — mfma_f32_16x16x32_f16, fp32 accumulate)
// ---------------------------------------------------------------------------

void launch_gemm_fp16_nt(const float* a, const float* b, const float* bias,
                         float* c, int m, int n, int k, bool relu,
                         hipStream_t s) {
  if (gemm_dispatch::tile128(m, n)) {
    const int grid = ((m + 127) / 128) * ((n + 127) / 128);
    gemm_bf16_nt_kernel<128, 128, 32, _Float16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k,
                                                    relu ? 1 : 0);
  } else {
    const int grid = ((m + 63) / 64) * ((n + 63) / 64);
    gemm_bf16_nt_kernel<64, 64, 64, _Float16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k,
                                                    relu ? 1 : 0);
  }
}

void launch_gemm_fp16_nn(const float* a, const float* b, const float* bias,
                         float* c, int m, int n, int k2, bool relu,
                         hipStream_t s) {
  if (gemm_dispatch::tile128(m, k2)) {
    const int grid = ((m + 127) / 128) * ((k2 + 127) / 128);
    gemm_bf16_nn_kernel<128, 128, 32, _Float16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k2,
                                                    relu ? 1 : 0);
  } else {
    const int grid = ((m + 63) / 64) * ((k2 + 63) / 64);
    gemm_bf16_nn_kernel<64, 64, 64, _Float16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k2,
                                                    relu ? 1 : 0);
  }
}

void launch_gemm_fp16_tn(const float* a, const float* b, float* c,
                         float* dbias, int m, int n, int k2, hipStream_t s) {
  const bool big = gemm_dispatch::tn_tile128(n, k2);
  const int tiles = gemm_dispatch::tn_tiles(n, k2);
  const int slices =
      gemm_dispatch::tn_slices(m, tiles, 64, pertgnn_deterministic());
  if (slices > 1)
    HIP_CHECK(hipMemsetAsync(c, 0, (long)n * k2 * sizeof(float), s));
  if (dbias) HIP_CHECK(hipMemsetAsync(dbias, 0, n * sizeof(float), s));
  if (big)
    gemm_bf16_tn_kernel<128, 128, 32, _Float16>
        <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                              m, n, k2,
                                                              slices);
  else
    gemm_bf16_tn_kernel<64, 64, 64, _Float16>
        <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                              m, n, k2,
                                                              slices);
}


// ---------------------------------------------------------------------------
// mixed-dtype launchers for the bf16-resident-activation mode: the QKVS
// forward writes its C as bf16; the backward GEMMs read the bf16 gradient
// directly (no conversion pass — bf16 LDS copy).
// ---------------------------------------------------------------------------

void launch_gemm_bf16_nt_o16(const float* a, const float* b, const float* bias,
                             void* c_v, int m, int n, int k, hipStream_t s) {
  __bf16* c = (__bf16*)c_v;
  if (gemm_dispatch::tile128(m, n)) {
    const int grid = ((m + 127) / 128) * ((n + 127) / 128);
    gemm_bf16_nt_kernel<128, 128, 32, __bf16, float, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k, 0);
  } else {
    const int grid = ((m + 63) / 64) * ((n + 63) / 64);
    gemm_bf16_nt_kernel<64, 64, 64, __bf16, float, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k, 0);
  }
}

void launch_gemm_bf16_nn_a16(const void* a_v, const float* b, float* c, int m,
                             int n, int k2, hipStream_t s) {
  const __bf16* a = (const __bf16*)a_v;
  if (gemm_dispatch::tile128(m, k2)) {
    const int grid = ((m + 127) / 128) * ((k2 + 127) / 128);
    gemm_bf16_nn_kernel<128, 128, 32, __bf16, __bf16, float>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, nullptr, c, m, n, k2,
                                                    0);
  } else {
    const int grid = ((m + 63) / 64) * ((k2 + 63) / 64);
    gemm_bf16_nn_kernel<64, 64, 64, __bf16, __bf16, float>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, nullptr, c, m, n, k2,
                                                    0);
  }
}

// `acc` (here and in the two a16b16 launchers below): c and dbias are
// gradient sinks that already hold a sum — no memset, the epilogue adds.
void launch_gemm_bf16_tn_a16(const void* a_v, const float* b, float* c,
                             float* dbias, int m, int n, int k2,
                             hipStream_t s, bool acc) {
  const __bf16* a = (const __bf16*)a_v;
  const bool big = gemm_dispatch::tn_tile128(n, k2);
  const int tiles = gemm_dispatch::tn_tiles(n, k2);
  const int slices =
      gemm_dispatch::tn_slices(m, tiles, 64, pertgnn_deterministic());
  if (acc) {
    if (big)
      gemm_bf16_tn_kernel<128, 128, 32, __bf16, __bf16, float, BGEMM_THREADS,
                          true>
          <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                                m, n, k2,
                                                                slices);
    else
      gemm_bf16_tn_kernel<64, 64, 64, __bf16, __bf16, float, BGEMM_THREADS,
                          true>
          <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                                m, n, k2,
                                                                slices);
    return;
  }
  if (slices > 1)
    HIP_CHECK(hipMemsetAsync(c, 0, (long)n * k2 * sizeof(float), s));
  if (dbias) HIP_CHECK(hipMemsetAsync(dbias, 0, n * sizeof(float), s));
  if (big)
    gemm_bf16_tn_kernel<128, 128, 32, __bf16, __bf16>
        <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                              m, n, k2,
                                                              slices);
  else
    gemm_bf16_tn_kernel<64, 64, 64, __bf16, __bf16>
        <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                              m, n, k2,
                                                              slices);
}

// ---------------------------------------------------------------------------
// act16-v2 launchers: fully bf16 activation IO (x16 in / qkvs16 out on the
// forward, bf16 gradients through dgrad, bf16 x through wgrad).  Weights and
// accumulation stay fp32; only stream dtypes change — at the flagship shapes
// the three model GEMMs are stream-bound, so halving A/C bytes is the lever
// (isolated: hipBLASLt bf16 reaches 1.9-3.5 TB/s effective on these shapes).
// ---------------------------------------------------------------------------

void launch_gemm_bf16_nt_a16o16(const void* a_v, const float* b,
                                const float* bias, void* c_v, int m, int n,
                                int k, hipStream_t s) {
  const __bf16* a = (const __bf16*)a_v;
  __bf16* c = (__bf16*)c_v;
  if (gemm_dispatch::tile128(m, n)) {
    const int grid = ((m + 127) / 128) * ((n + 127) / 128);
    if (gemm_t512()) {
      gemm_bf16_nt_kernel<128, 128, 32, __bf16, __bf16, __bf16, 512>
          <<<dim3(grid), dim3(512), 0, s>>>(a, b, bias, c, m, n, k, 0);
      return;
    }
    gemm_bf16_nt_kernel<128, 128, 32, __bf16, __bf16, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k, 0);
  } else {
    const int grid = ((m + 63) / 64) * ((n + 63) / 64);
    gemm_bf16_nt_kernel<64, 64, 64, __bf16, __bf16, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k, 0);
  }
}

void launch_gemm_bf16_nn_a16o16(const void* a_v, const float* b, void* c_v,
                                int m, int n, int k2, hipStream_t s) {
  const __bf16* a = (const __bf16*)a_v;
  __bf16* c = (__bf16*)c_v;
  if (gemm_dispatch::tile128(m, k2)) {
    const int grid = ((m + 127) / 128) * ((k2 + 127) / 128);
    if (gemm_t512()) {
      gemm_bf16_nn_kernel<128, 128, 32, __bf16, __bf16, __bf16, 512>
          <<<dim3(grid), dim3(512), 0, s>>>(a, b, nullptr, c, m, n, k2, 0);
      return;
    }
    gemm_bf16_nn_kernel<128, 128, 32, __bf16, __bf16, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, nullptr, c, m, n, k2,
                                                    0);
  } else {
    const int grid = ((m + 63) / 64) * ((k2 + 63) / 64);
    gemm_bf16_nn_kernel<64, 64, 64, __bf16, __bf16, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, nullptr, c, m, n, k2,
                                                    0);
  }
}

void launch_gemm_bf16_tn_a16b16(const void* a_v, const void* b_v, float* c,
                                float* dbias, int m, int n, int k2,
                                hipStream_t s, bool acc) {
  const __bf16* a = (const __bf16*)a_v;
  const __bf16* b = (const __bf16*)b_v;
  const bool big = gemm_dispatch::tn_tile128(n, k2);
  const int tiles = gemm_dispatch::tn_tiles(n, k2);
  const int slices =
      gemm_dispatch::tn_slices(m, tiles, 64, pertgnn_deterministic());
  if (acc) {
    if (big && gemm_t512())
      gemm_bf16_tn_kernel<128, 128, 32, __bf16, __bf16, __bf16, 512, true>
          <<<dim3(tiles * slices), dim3(512), 0, s>>>(a, b, c, dbias, m, n,
                                                      k2, slices);
    else if (big)
      gemm_bf16_tn_kernel<128, 128, 32, __bf16, __bf16, __bf16, BGEMM_THREADS,
                          true>
          <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                                m, n, k2,
                                                                slices);
    else
      gemm_bf16_tn_kernel<64, 64, 64, __bf16, __bf16, __bf16, BGEMM_THREADS,
                          true>
          <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                                m, n, k2,
                                                                slices);
    return;
  }
  if (slices > 1)
    HIP_CHECK(hipMemsetAsync(c, 0, (long)n * k2 * sizeof(float), s));
  if (dbias) HIP_CHECK(hipMemsetAsync(dbias, 0, n * sizeof(float), s));
  if (big) {
    if (gemm_t512()) {
      gemm_bf16_tn_kernel<128, 128, 32, __bf16, __bf16, __bf16, 512>
          <<<dim3(tiles * slices), dim3(512), 0, s>>>(a, b, c, dbias, m, n,
                                                      k2, slices);
      return;
    }
    gemm_bf16_tn_kernel<128, 128, 32, __bf16, __bf16, __bf16>
        <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                              m, n, k2,
                                                              slices);
  } else
    gemm_bf16_tn_kernel<64, 64, 64, __bf16, __bf16, __bf16>
        <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                              m, n, k2,
                                                              slices);
}

// fp16-COMPUTE variants of the act16 launchers: activation streams stay bf16
// (storage dtype is independent of the MFMA operand dtype — staging converts
// while packing), matrix cores run v_mfma_f32_16x16x32_f16.
void launch_gemm_fp16_nt_a16o16(const void* a_v, const float* b,
                                const float* bias, void* c_v, int m, int n,
                                int k, hipStream_t s) {
  const __bf16* a = (const __bf16*)a_v;
  __bf16* c = (__bf16*)c_v;
  if (gemm_dispatch::tile128(m, n)) {
    const int grid = ((m + 127) / 128) * ((n + 127) / 128);
    gemm_bf16_nt_kernel<128, 128, 32, _Float16, __bf16, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k, 0);
  } else {
    const int grid = ((m + 63) / 64) * ((n + 63) / 64);
    gemm_bf16_nt_kernel<64, 64, 64, _Float16, __bf16, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, bias, c, m, n, k, 0);
  }
}

void launch_gemm_fp16_nn_a16o16(const void* a_v, const float* b, void* c_v,
                                int m, int n, int k2, hipStream_t s) {
  const __bf16* a = (const __bf16*)a_v;
  __bf16* c = (__bf16*)c_v;
  if (gemm_dispatch::tile128(m, k2)) {
    const int grid = ((m + 127) / 128) * ((k2 + 127) / 128);
    gemm_bf16_nn_kernel<128, 128, 32, _Float16, __bf16, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, nullptr, c, m, n, k2,
                                                    0);
  } else {
    const int grid = ((m + 63) / 64) * ((k2 + 63) / 64);
    gemm_bf16_nn_kernel<64, 64, 64, _Float16, __bf16, __bf16>
        <<<dim3(grid), dim3(BGEMM_THREADS), 0, s>>>(a, b, nullptr, c, m, n, k2,
                                                    0);
  }
}

void launch_gemm_fp16_tn_a16b16(const void* a_v, const void* b_v, float* c,
                                float* dbias, int m, int n, int k2,
                                hipStream_t s, bool acc) {
  const __bf16* a = (const __bf16*)a_v;
  const __bf16* b = (const __bf16*)b_v;
  const bool big = gemm_dispatch::tn_tile128(n, k2);
  const int tiles = gemm_dispatch::tn_tiles(n, k2);
  const int slices =
      gemm_dispatch::tn_slices(m, tiles, 64, pertgnn_deterministic());
  if (acc) {
    if (big)
      gemm_bf16_tn_kernel<128, 128, 32, _Float16, __bf16, __bf16,
                          BGEMM_THREADS, true>
          <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                                m, n, k2,
                                                                slices);
    else
      gemm_bf16_tn_kernel<64, 64, 64, _Float16, __bf16, __bf16, BGEMM_THREADS,
                          true>
          <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                                m, n, k2,
                                                                slices);
    return;
  }
  if (slices > 1)
    HIP_CHECK(hipMemsetAsync(c, 0, (long)n * k2 * sizeof(float), s));
  if (dbias) HIP_CHECK(hipMemsetAsync(dbias, 0, n * sizeof(float), s));
  if (big)
    gemm_bf16_tn_kernel<128, 128, 32, _Float16, __bf16, __bf16>
        <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                              m, n, k2,
                                                              slices);
  else
    gemm_bf16_tn_kernel<64, 64, 64, _Float16, __bf16, __bf16>
        <<<dim3(tiles * slices), dim3(BGEMM_THREADS), 0, s>>>(a, b, c, dbias,
                                                              m, n, k2,
                                                              slices);
}

// ---------------------------------------------------------------------------
// glds NT kernel: both operands bf16 in HBM, staged by global_load_lds
// width-16 (direct-to-LDS DMA — no staging VGPRs, no ds_write pass; guide
// "optimization ladder" step 3: +67% over register staging on its own).
// LDS image is lane-linear row-major [128 rows][64 k] bf16 with the
// st_16x32 XOR swizzle (byte ^= ((byte>>9)&1)<<5 within each 1024-B
// subtile) applied on BOTH the per-lane glds SOURCE address and the
// ds_read address: linear 128-B rows put every fragment lane-group on the
// same bank row (8-way conflict); the swizzle spreads rows 4..7 of each
// 8-row group one 32-B slot over (guide: bank-conflict 141x down).
// One barrier per K-step: issue next tile's glds -> MFMA current ->
// s_waitcnt vmcnt(0) -> barrier (the accepted step-3 stall).
// The grid covers ceil(m / BM) row tiles: the partial last tile stages
// clamped (duplicate) A rows and skips the stores of rows >= m, so its valid
// rows get exactly the arithmetic of interior rows.  Requires n % BN == 0,
// k % BK == 0 and 16-B-aligned rows (lda % 8 == 0).
// ---------------------------------------------------------------------------

__device__ __forceinline__ unsigned glds_swz(unsigned byte_off) {
  return byte_off ^ (((byte_off >> 9) & 1u) << 5);
}

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

template <int BM, int BN, int BK, typename TO, int THREADS, bool NTC>
__launch_bounds__(THREADS)
__global__ void gemm_a16_glds_nt_kernel(const __bf16* __restrict__ a,
                                        const __bf16* __restrict__ b,
                                        const float* __restrict__ bias,
                                        TO* __restrict__ c, int m, int n,
                                        int k, int relu) {
  constexpr int NWAVE = THREADS / PERTGNN_WAVE;
  constexpr int WCOL = NWAVE / 2;
  constexpr int FM = (BM / 2) / 16, FN = (BN / WCOL) / 16;
  constexpr int TILE_BYTES = BM * BK * 2;          // A-operand K-tile
  constexpr int GRPS_A = TILE_BYTES / 1024;        // 1 KiB per wave-glds
  constexpr int GRPS_B = (BN * BK * 2) / 1024;
  // one arena: [A0 A1 B0 B1] operand buffers; the C-store scratch reuses it
  __shared__ char smem[2 * (BM + BN) * BK * 2];
  const auto lds_ab = [&](int i) { return (__bf16*)(smem + i * TILE_BYTES); };
  const auto lds_bb = [&](int i) {
    return (__bf16*)(smem + 2 * TILE_BYTES + i * (BN * BK * 2));
  };
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tiles_n = n / BN;
  const int m0 = (bid / tiles_n) * BM;
  const int n0 = (bid % tiles_n) * BN;
  const int wave = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int wm = (wave / WCOL) * (BM / 2);
  const int wn = (wave % WCOL) * (BN / WCOL);

  // per-lane glds source mapping: lds slot (grp, lane*16) holds the element
  // at LOGICAL tile offset swz(grp*1024 + lane*16) = (row, kbyte); row
  // width is BK*2 bytes, so one 1-KiB group covers 1024/(BK*2) rows
  constexpr int ROW_BYTES = BK * 2;
  constexpr int ROWS_PER_GRP = 1024 / ROW_BYTES;
  const unsigned l_off = glds_swz((unsigned)lane * 16);
  const int src_row = (int)(l_off / ROW_BYTES);    // within the group
  const int src_kb = (int)(l_off % ROW_BYTES);     // byte within row

  const long lda = k;  // elements
  // per-lane source bases (byte offsets at k0 = 0), fixed before the K loop.
  // The A rows of the edge tile (m0 + BM > m) are clamped to m - 1: the
  // block stages duplicates of a valid row, never reads past the tensor,
  // and the epilogue drops the rows >= m.  B always has full tiles.
  // Per-operand group counts: A covers BM rows, B covers BN (they differ
  // for the single-column-tile dgrad variant).
  long a_base[GRPS_A / NWAVE], b_base[GRPS_B / NWAVE];
#pragma unroll
  for (int i = 0; i < GRPS_A / NWAVE; ++i) {
    const int row = m0 + (wave + i * NWAVE) * ROWS_PER_GRP + src_row;
    a_base[i] = (long)min(row, m - 1) * lda * 2 + src_kb;
  }
#pragma unroll
  for (int i = 0; i < GRPS_B / NWAVE; ++i) {
    const int row = n0 + (wave + i * NWAVE) * ROWS_PER_GRP + src_row;
    b_base[i] = (long)row * lda * 2 + src_kb;
  }
  auto stage = [&]<int GRPS>(const __bf16* g, const long* base, int k0,
                             __bf16* lds) {
#pragma unroll
    for (int i = 0; i < GRPS / NWAVE; ++i) {
      const int grp = wave + i * NWAVE;
      const __bf16* src =
          (const __bf16*)((const char*)g + base[i] + (long)k0 * 2);
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(lds + grp * 512),
          16, 0, 0);
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  stage.template operator()<GRPS_A>(a, a_base, 0, lds_ab(0));
  stage.template operator()<GRPS_B>(b, b_base, 0, lds_bb(0));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int fi = lane & 15;
  const int fk = (lane >> 4) * 8;
  auto mma = [&](const __bf16* la, const __bf16* lb) {
#pragma unroll
    for (int s = 0; s < BK / 32; ++s) {
      const int kb = (s * 32 + fk) * 2;
      bf16x8 av[FM], bv[FN];
#pragma unroll
      for (int mi = 0; mi < FM; ++mi) {
        const int row = wm + mi * 16 + fi;
        av[mi] = *reinterpret_cast<const bf16x8*>(
            (const char*)la + glds_swz((unsigned)(row * (BK * 2) + kb)));
      }
#pragma unroll
      for (int ni = 0; ni < FN; ++ni) {
        const int row = wn + ni * 16 + fi;
        bv[ni] = *reinterpret_cast<const bf16x8*>(
            (const char*)lb + glds_swz((unsigned)(row * (BK * 2) + kb)));
      }
#pragma unroll
      for (int mi = 0; mi < FM; ++mi)
#pragma unroll
        for (int ni = 0; ni < FN; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    }
  };

  int buf = 0;
  for (int k0 = BK; k0 < k; k0 += BK) {
    stage.template operator()<GRPS_A>(a, a_base, k0, lds_ab(buf ^ 1));
    stage.template operator()<GRPS_B>(b, b_base, k0, lds_bb(buf ^ 1));
    mma(lds_ab(buf), lds_bb(buf));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    buf ^= 1;
  }
  mma(lds_ab(buf), lds_bb(buf));

  // LDS-staged coalesced epilogue: the MFMA C fragment layout (lane owns
  // col=l&15, rows (l>>4)*4+r) would store 2-B/4-B scalars at row stride —
  // the measured bottleneck at [M,1024] outputs.  Each wave transposes one
  // 16-row band at a time through its private LDS scratch, then writes
  // 16-B lane chunks (8 lanes cover a full 128-B row of bf16).  NTC stores
  // the C stream nontemporally — 370 MB of writes with zero reuse would
  // otherwise wash the operand tiles out of L2.
  __syncthreads();  // operand LDS is being re-purposed as scratch
  constexpr int BNW = BN / WCOL;              // wave's output columns
  constexpr int SW = BNW + 8;                 // padded scratch stride
  TO* scratch = reinterpret_cast<TO*>(smem + wave * 16 * SW * sizeof(TO));
  const int fcol = lane & 15;
  const int frow = (lane >> 4) * 4;
  constexpr int EPL = 16 / sizeof(TO);        // elements per 16-B chunk
  constexpr int CPR = BNW / EPL;              // chunks per scratch row
#pragma unroll
  for (int mi = 0; mi < FM; ++mi) {
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = ni * 16 + fcol;
        float v = acc[mi][ni][r];
        if (bias) v += bias[n0 + wn + col];
        if (relu) v = fmaxf(v, 0.f);
        scratch[(frow + r) * SW + col] = (TO)v;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < 16 * CPR / PERTGNN_WAVE; ++it) {
      const int chunk = it * PERTGNN_WAVE + lane;
      const int r = chunk / CPR;
      const int off = (chunk % CPR) * EPL;
      const u32x4_t val = *reinterpret_cast<const u32x4_t*>(&scratch[r * SW + off]);
      const int grow = m0 + wm + mi * 16 + r;
      if (grow >= m) continue;  // edge tile: rows past the tensor
      u32x4_t* dst =
          reinterpret_cast<u32x4_t*>(&c[(long)grow * n + n0 + wn + off]);
      if constexpr (NTC)
        __builtin_nontemporal_store(val, dst);
      else
        *dst = val;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

// ---------------------------------------------------------------------------
// A-resident glds NT kernel (forward with a short K and a wide output): one
// block owns a BM-row tile of A for the whole call and sweeps all n / 128
// column tiles.  The kernel above stages every A row tile once per column
// tile and pays a barrier per 32 of K; here the BM x KT tile is staged once,
// as KT/32 slabs in that kernel's lane-linear [BM][32] image (same glds_swz
// on both sides, rows past m clamped to m - 1), and is never restaged, so A
// has no WAR hazard.  The weight image (L2-resident) streams through a ring
// of two [128 cols][BKB k] stages, each BKB/32 slabs of the [128][32] image:
//   issue stage t+1 -> MFMA stage t -> s_waitcnt vmcnt(0) -> barrier
// which is the streaming kernel's sync structure at BKB/32 times the MFMAs
// per barrier.  RAW: a stage is read only after the vmcnt(0) + barrier that
// follow its issue.  WAR: stage t+1 overwrites the buffer read in iteration
// t-1, whose ds_reads all fed MFMAs issued before that iteration's barrier.
// Per output element the MFMA chain is the streaming kernel's (16x16x32, k
// ascending in steps of 32, one accumulator), as are the bias add and the
// single rounding, so C is bit-equal to it on any input.
// Waves are (BM/32) x 2 with a 32 x 64 wave tile: the epilogue transposes a
// 16-row band through a per-wave scratch of its own (the A tile stays live)
// and every 16-B-per-lane store instruction covers 8 whole 128-B lines.
// The epilogue of a column tile runs after the barrier that ends its last
// stage, so its stores drain behind the next tile's MFMAs and the ordinary
// bias loads never meet a glds in flight.
// Requires k == KT, n % 128 == 0, 16-B-aligned rows; any m >= 1.
// Reads stay in bounds: A rows are clamped, the last A slab ends at byte
// KT * 2 of its row, B rows end at n0 + 128 <= n and B slabs at k.
// ---------------------------------------------------------------------------
template <int BM, int KT, int BKB, bool NTC>
__launch_bounds__(BM * 4)
__global__ void gemm_a16_resident_nt_kernel(const __bf16* __restrict__ a,
                                            const __bf16* __restrict__ b,
                                            const float* __restrict__ bias,
                                            __bf16* __restrict__ c, int m,
                                            int n) {
  constexpr int BN = 128;
  constexpr int THREADS = BM * 4;
  constexpr int NWAVE = THREADS / PERTGNN_WAVE;      // BM / 16
  constexpr int FM = 2, FN = 4;                      // 32 x 64 wave tile
  constexpr int SLAB_A = BM * 64;                    // [BM][32] bf16
  constexpr int SLAB_B = BN * 64;                    // [128][32] bf16
  constexpr int NSLAB = BKB / 32;                    // slabs per B stage
  constexpr int KS = KT / BKB;                       // B stages per tile
  constexpr int A_BYTES = (KT / 32) * SLAB_A;
  constexpr int B_BYTES = NSLAB * SLAB_B;
  constexpr int GRPS_B = B_BYTES / 1024;             // 1 KiB per wave-glds
  constexpr int BNW = 64;                            // wave's output columns
  constexpr int SW = BNW + 8;                        // padded scratch stride
  static_assert(SLAB_A / 1024 == NWAVE, "one glds per wave per A slab");
  static_assert(KS % 2 == 0 && GRPS_B % NWAVE == 0, "ring of two stages");
  // one arena: [A tile][B0 B1][per-wave C scratch]
  __shared__ char smem[A_BYTES + 2 * B_BYTES + NWAVE * 16 * SW * 2];
  char* const lds_a = smem;
  const auto lds_bb = [&](int i) { return smem + A_BYTES + i * B_BYTES; };
  const int m0 = blockIdx.x * BM;
  const int wave = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int wm = (wave / 2) * 32;
  const int wn = (wave % 2) * BNW;

  // per-lane glds source mapping of the [rows][32] image (see above): one
  // 1-KiB group covers 16 rows of 64 B
  const unsigned l_off = glds_swz((unsigned)lane * 16);
  const int src_row = (int)(l_off / 64);
  const int src_kb = (int)(l_off % 64);
  const long ldb = (long)KT * 2;                     // row bytes, A and B

  const auto glds16 = [](const char* src, char* dst) {
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) void*)src,
        (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
  };
  // B stage t = (column tile, ks): group g is rows (g % 8) * 16 .. of slab
  // g / 8
  const auto stage_b = [&](int n0, int ks, char* lds) {
#pragma unroll
    for (int i = 0; i < GRPS_B / NWAVE; ++i) {
      const int grp = wave + i * NWAVE;
      const int row = n0 + (grp % 8) * 16 + src_row;
      const int kb = (ks * BKB + (grp / 8) * 32) * 2 + src_kb;
      glds16((const char*)b + (long)row * ldb + kb, lds + grp * 1024);
    }
  };

  {
    const int row = min(m0 + wave * 16 + src_row, m - 1);
    const char* src = (const char*)a + (long)row * ldb + src_kb;
#pragma unroll
    for (int s = 0; s < KT / 32; ++s)
      glds16(src + s * 64, lds_a + s * SLAB_A + wave * 1024);
  }
  stage_b(0, 0, lds_bb(0));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int fi = lane & 15;
  const int kb = (lane >> 4) * 16;                   // fragment k byte
  const int fcol = lane & 15;
  const int frow = (lane >> 4) * 4;
  __bf16* scratch = reinterpret_cast<__bf16*>(smem + A_BYTES + 2 * B_BYTES +
                                              wave * 16 * SW * 2);
  const int tiles_n = n / BN;
  for (int ct = 0; ct < tiles_n; ++ct) {
    const int n0 = ct * BN;
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      // next stage into the other buffer (KS is even: buffer = ks & 1)
      if (ks + 1 < KS)
        stage_b(n0, ks + 1, lds_bb((ks + 1) & 1));
      else if (ct + 1 < tiles_n)
        stage_b(n0 + BN, 0, lds_bb(0));
      const char* lb = lds_bb(ks & 1);
#pragma unroll
      for (int s = 0; s < NSLAB; ++s) {
        const char* la = lds_a + (ks * NSLAB + s) * SLAB_A;
        bf16x8 av[FM], bv[FN];
#pragma unroll
        for (int mi = 0; mi < FM; ++mi) {
          const int row = wm + mi * 16 + fi;
          av[mi] = *reinterpret_cast<const bf16x8*>(
              la + glds_swz((unsigned)(row * 64 + kb)));
        }
#pragma unroll
        for (int ni = 0; ni < FN; ++ni) {
          const int row = wn + ni * 16 + fi;
          bv[ni] = *reinterpret_cast<const bf16x8*>(
              lb + s * SLAB_B + glds_swz((unsigned)(row * 64 + kb)));
        }
#pragma unroll
        for (int mi = 0; mi < FM; ++mi)
#pragma unroll
          for (int ni = 0; ni < FN; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }

    // epilogue of this column tile: bias, one rounding, per-wave transpose,
    // 16-B nontemporal stores (8 lanes per 128-B line of bf16)
    float bv4[FN] = {0.f, 0.f, 0.f, 0.f};
    if (bias) {  // one branch around all four loads, one wait for them
#pragma unroll
      for (int ni = 0; ni < FN; ++ni)
        bv4[ni] = bias[n0 + wn + ni * 16 + fcol];
    }
    constexpr int CPR = BNW / 8;                     // 16-B chunks per row
#pragma unroll
    for (int mi = 0; mi < FM; ++mi) {
#pragma unroll
      for (int ni = 0; ni < FN; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[mi][ni][r];
          if (bias) v += bv4[ni];
          scratch[(frow + r) * SW + ni * 16 + fcol] = (__bf16)v;
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int it = 0; it < 16 * CPR / PERTGNN_WAVE; ++it) {
        const int chunk = it * PERTGNN_WAVE + lane;
        const int r = chunk / CPR;
        const int off = (chunk % CPR) * 8;
        const u32x4_t val =
            *reinterpret_cast<const u32x4_t*>(&scratch[r * SW + off]);
        const int grow = m0 + wm + mi * 16 + r;
        if (grow >= m) continue;  // edge tile: rows past the tensor
        u32x4_t* dst =
            reinterpret_cast<u32x4_t*>(&c[(long)grow * n + n0 + wn + off]);
        if constexpr (NTC)
          __builtin_nontemporal_store(val, dst);
        else
          *dst = val;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
}

// fp32 [n][k] row-major -> bf16 [n][k] (weight operand for the glds path)
__global__ void convert_w16_kernel(const float* __restrict__ w,
                                   __bf16* __restrict__ o, long numel) {
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = i0; t < numel; t += stride) o[t] = (__bf16)w[t];
}

// fp32 [rows][cols] -> bf16 [cols][rows] (transposed weight for dgrad-as-NT)
__global__ void transpose_convert_w16_kernel(const float* __restrict__ w,
                                             __bf16* __restrict__ o, int rows,
                                             int cols) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32;
  const int r0 = blockIdx.y * 32;
  const int tx = threadIdx.x % 32;
  const int ty = threadIdx.x / 32;
  for (int dy = ty; dy < 32; dy += blockDim.x / 32) {
    const int r = r0 + dy, ccol = c0 + tx;
    tile[dy][tx] = (r < rows && ccol < cols) ? w[(long)r * cols + ccol] : 0.f;
  }
  __syncthreads();
  for (int dy = ty; dy < 32; dy += blockDim.x / 32) {
    const int ccol = c0 + dy, r = r0 + tx;
    if (ccol < cols && r < rows) o[(long)ccol * rows + r] = (__bf16)tile[tx][dy];
  }
}

// Both bf16 weight images of one fp32 [rows][cols] weight from one launch:
// o [rows][cols] for the forward, ot [cols][rows] for the dgrad-as-NT.  Each
// 32x32 tile is read once; the same (__bf16) rounding as the two kernels
// above, so the images are bit-identical to theirs.
__global__ void convert_w16_both_kernel(const float* __restrict__ w,
                                        __bf16* __restrict__ o,
                                        __bf16* __restrict__ ot, int rows,
                                        int cols) {
  __shared__ float tile[32][33];
  const int c0 = blockIdx.x * 32;
  const int r0 = blockIdx.y * 32;
  const int tx = threadIdx.x % 32;
  const int ty = threadIdx.x / 32;
  for (int dy = ty; dy < 32; dy += blockDim.x / 32) {
    const int r = r0 + dy, ccol = c0 + tx;
    float v = 0.f;
    if (r < rows && ccol < cols) {
      v = w[(long)r * cols + ccol];
      o[(long)r * cols + ccol] = (__bf16)v;
    }
    tile[dy][tx] = v;
  }
  __syncthreads();
  for (int dy = ty; dy < 32; dy += blockDim.x / 32) {
    const int ccol = c0 + dy, r = r0 + tx;
    if (ccol < cols && r < rows)
      ot[(long)ccol * rows + r] = (__bf16)tile[tx][dy];
  }
}

void launch_convert_w16_both(const float* w, void* o, void* ot, int rows,
                             int cols, hipStream_t s) {
  convert_w16_both_kernel<<<dim3((cols + 31) / 32, (rows + 31) / 32),
                            dim3(256), 0, s>>>(w, (__bf16*)o, (__bf16*)ot,
                                               rows, cols);
}

void launch_convert_w16(const float* w, void* o, long numel, hipStream_t s) {
  const int blocks = (int)min((numel + 255) / 256, (long)4096);
  convert_w16_kernel<<<blocks, 256, 0, s>>>(w, (__bf16*)o, numel);
}

void launch_transpose_convert_w16(const float* w, void* o, int rows, int cols,
                                  hipStream_t s) {
  transpose_convert_w16_kernel<<<dim3((cols + 31) / 32, (rows + 31) / 32),
                                 dim3(256), 0, s>>>(w, (__bf16*)o, rows, cols);
}

// A + B16 bf16, NT: every row tile, the partial last one included, runs in
// the one glds launch.
static int glds_bk() {  // default 32 (measured: +13-20% over 64 at model shapes)
  static int v = [] {
    const char* e = getenv("PERTGNN_GLDS_BK");
    return (e && atoi(e) == 64) ? 64 : 32;
  }();
  return v;
}
static bool glds_t512() {  // default ON (8 waves; measured faster everywhere)
  static bool v = [] {
    const char* e = getenv("PERTGNN_GLDS_T512");
    return !(e && atoi(e) == 0);
  }();
  return v;
}
static bool glds_ntc() {  // nontemporal C stores (default ON)
  static bool v = [] {
    const char* e = getenv("PERTGNN_GLDS_NTC");
    return !(e && atoi(e) == 0);
  }();
  return v;
}


static bool glds_n256() {  // 256-wide output tile for big dgrads (default ON)
  static bool v = [] {
    const char* e = getenv("PERTGNN_GLDS_N256");
    return !(e && atoi(e) == 0);
  }();
  return v;
}

void launch_gemm_a16_glds_nt(const void* a_v, const void* b16_v,
                             const float* bias, void* c_v, int c16, int m,
                             int n, int k, bool relu, hipStream_t s) {
  const __bf16* a = (const __bf16*)a_v;
  const __bf16* b = (const __bf16*)b16_v;
  constexpr int BM = 128, BN = 128;
  if (m <= 0) return;
  const int mt = (m + BM - 1) / BM;  // row tiles, the partial last one included
  if (gemm_dispatch::glds_nt_wide(m, n, k) && glds_n256()) {
    // single-column-tile variant for the dgrad shape: A is streamed exactly
    // once and the per-block K-loop halves its barrier count (measured
    // +12% at [180k,1024]x[1024,256]); needs >= ~1024 full row tiles to fill
    // the chip (it LOSES at 45k rows where the 128-wide grid is 2x larger)
    if (c16)
      gemm_a16_glds_nt_kernel<128, 256, 32, __bf16, 512, true>
          <<<dim3(mt), dim3(512), 0, s>>>(a, b, bias, (__bf16*)c_v, m, n, k,
                                          relu ? 1 : 0);
    else
      gemm_a16_glds_nt_kernel<128, 256, 32, float, 512, true>
          <<<dim3(mt), dim3(512), 0, s>>>(a, b, bias, (float*)c_v, m, n, k,
                                          relu ? 1 : 0);
  } else {
    const int grid = mt * (n / BN);
    const int bk = glds_bk();
    const bool t512 = glds_t512();
    const bool ntc = glds_ntc();
#define GLDS_DISPATCH(BKV, TH, NTCV)                                           \
  do {                                                                         \
    if (c16)                                                                   \
      gemm_a16_glds_nt_kernel<BM, BN, BKV, __bf16, TH, NTCV>                   \
          <<<dim3(grid), dim3(TH), 0, s>>>(a, b, bias, (__bf16*)c_v, m, n, k,  \
                                           relu ? 1 : 0);                      \
    else                                                                       \
      gemm_a16_glds_nt_kernel<BM, BN, BKV, float, TH, NTCV>                    \
          <<<dim3(grid), dim3(TH), 0, s>>>(a, b, bias, (float*)c_v, m, n, k,   \
                                           relu ? 1 : 0);                      \
  } while (0)
    if ((bk == 32 || k % 64 != 0) && k % 32 == 0) {
      if (t512) { if (ntc) GLDS_DISPATCH(32, 512, true); else GLDS_DISPATCH(32, 512, false); }
      else      { if (ntc) GLDS_DISPATCH(32, 256, true); else GLDS_DISPATCH(32, 256, false); }
    } else {
      if (t512) { if (ntc) GLDS_DISPATCH(64, 512, true); else GLDS_DISPATCH(64, 512, false); }
      else      { if (ntc) GLDS_DISPATCH(64, 256, true); else GLDS_DISPATCH(64, 256, false); }
    }
#undef GLDS_DISPATCH
  }
}

// Forward variant (streaming / A-resident glds NT kernel) as it runs in this
// process: gemm_dispatch::fwd_variant() under the set_fwd_variant() test hook
// and PERTGNN_NO_FWD_RESIDENT (read per call, so one process can run both).
static int g_fwd_variant = gemm_dispatch::FWD_AUTO;  // test hook
void set_fwd_variant_hook(int v) { g_fwd_variant = v; }

int fwd_variant_for(int m, int n, int k) {
  const char* e = getenv("PERTGNN_NO_FWD_RESIDENT");
  return gemm_dispatch::fwd_variant(m, n, k, g_fwd_variant,
                                    e && e[0] == '1');
}

// Geometry of the A-resident kernel: 1 = 128-row tiles, 512 threads, B stages
// of 128 k, one block per CU; 2 = 64-row tiles, 256 threads, B stages of 64 k,
// two blocks per CU.  PERTGNN_FWD_RES_GEOM (read per call) picks one for the
// micro-benchmarks; the default is the one that measured faster at the
// flagship shape (profiles/25_fwd_resident.md).
static int fwd_resident_geom() {
  const char* e = getenv("PERTGNN_FWD_RES_GEOM");
  const int g = e ? atoi(e) : 0;
  return (g == 1 || g == 2) ? g : gemm_dispatch::FWD_RESIDENT_GEOM;
}

void launch_gemm_a16_resident_nt(const void* a_v, const void* b16_v,
                                 const float* bias, void* c_v, int m, int n,
                                 int k, hipStream_t s) {
  if (m <= 0) return;
  const __bf16* a = (const __bf16*)a_v;
  const __bf16* b = (const __bf16*)b16_v;
  __bf16* c = (__bf16*)c_v;
  if (!gemm_dispatch::fwd_resident_can(m, n, k))
    pertgnn_shape_fail("launch_gemm_a16_resident_nt", k != 256 ? "k" : "n",
                       k != 256 ? k : n);
  if (fwd_resident_geom() == 1)
    gemm_a16_resident_nt_kernel<128, 256, 128, true>
        <<<dim3((m + 127) / 128), dim3(512), 0, s>>>(a, b, bias, c, m, n);
  else
    gemm_a16_resident_nt_kernel<64, 256, 64, true>
        <<<dim3((m + 63) / 64), dim3(256), 0, s>>>(a, b, bias, c, m, n);
}

// ---------------------------------------------------------------------------
// glds TN kernel (wgrad): dw[n,k2] = sum_m g[m,n]^T x[m,k2].  Both operands
// are contract(m)-major in HBM, so the NT kernel's row-linear glds image
// cannot feed k-minor MFMA fragments.  Instead each operand tile is staged
// as an image of 256-B blocks, [8 m][16 cols] row-major, ordered
// [64-column group][m octet][4 panels of 16 columns] (the per-lane glds
// source addresses assemble them directly; one wave-instruction fetches 8
// rows x 128 B, whole lines) — and the MFMA fragments are read with
// gfx950's ds_read_b64_tr_b16 hardware transpose-read (lane gets 4
// contract-consecutive elements at 32-B stride; two reads, the halves of
// one block, make the 8-element k fragment).  Split-K over m with
// atomicAdd combine, same contract as the register-staging TN kernel.
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_g;

template <int BM /*n cols*/, int BN /*k2 cols*/, int BKM /*m per step*/,
          int THREADS = 512, bool ACC = false>
__launch_bounds__(THREADS)
__global__ void gemm_a16_glds_tn_kernel(const __bf16* __restrict__ a,
                                        const __bf16* __restrict__ b,
                                        float* __restrict__ c,
                                        float* __restrict__ dbias, int m,
                                        int n, int k2, int slices) {
  constexpr int NWAVE = THREADS / PERTGNN_WAVE;
  constexpr int WCOL = NWAVE / 2;
  constexpr int FM = (BM / 2) / 16, FN = (BN / WCOL) / 16;
  constexpr int OCTS = BKM / 8;                    // m octets per step
  constexpr int GROUP_BYTES = OCTS * 1024;         // [OCTS][4][8][16] bf16
  constexpr int TILE_BYTES = BM * BKM * 2;
  // 1 KiB per wave-glds; the two operands' images differ when BM != BN
  constexpr int GRPS_A = TILE_BYTES / 1024 / NWAVE;
  constexpr int GRPS_B = BN * BKM * 2 / 1024 / NWAVE;
  static_assert(GRPS_A * NWAVE * 1024 == TILE_BYTES &&
                    GRPS_B * NWAVE * 1024 == BN * BKM * 2,
                "every wave stages whole 1-KiB groups of both images");
  __shared__ char smem[2 * (BM + BN) * BKM * 2];
  const auto lds_ab = [&](int i) { return smem + i * TILE_BYTES; };
  const auto lds_bb = [&](int i) {
    return smem + 2 * TILE_BYTES + i * (BN * BKM * 2);
  };
  const int bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tiles_k = k2 / BN;
  const int tile_id = bid / slices;
  const int slice = bid % slices;
  const int n0 = (tile_id / tiles_k) * BM;
  const int k0 = (tile_id % tiles_k) * BN;
  const int wave = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int wm = (wave / WCOL) * (BM / 2);
  const int wn = (wave % WCOL) * (BN / WCOL);

  // m range of this slice (multiples of BKM; the m % BKM rows behind
  // m_full are a partial last step of the last slice, below)
  const int m_full = m - m % BKM;
  const int per_slice = ((m_full / BKM + slices - 1) / slices) * BKM;
  const int c_beg = slice * per_slice;
  const int c_end = min(m_full, c_beg + per_slice);
  if (c_beg >= c_end) return;

  // glds staging: group g covers one m octet of a 64-column group (8 m x
  // 128 B, four [8][16] blocks); lane's 16-B chunk = 8 columns of one m-row
  // of block lane / 16, so eight lanes fetch one whole 128-B line
  // (TAIL: the partial last step clamps the m-row to m - 1, so it stages
  // duplicates of a valid row and never reads past the tensor)
  auto stage = [&]<int GRPS_PER_WAVE, bool TAIL = false>(
                   const __bf16* src_base, long ld, int col0, int mrow0,
                   char* lds) {
#pragma unroll
    for (int i = 0; i < GRPS_PER_WAVE; ++i) {
      const int grp = wave + i * NWAVE;
      int mrow = mrow0 + (grp % OCTS) * 8 + ((lane >> 1) & 7);
      if constexpr (TAIL) mrow = min(mrow, m - 1);
      const int col = (grp / OCTS) * 64 + (lane >> 4) * 16 + (lane & 1) * 8;
      const __bf16* src = src_base + (long)mrow * ld + col0 + col;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(lds + grp * 1024),
          16, 0, 0);
    }
  };

  f32x4 acc[FM][FN];
  float dbacc[FM];  // fused bias grad rides the A fragments (see below)
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    dbacc[i] = 0.f;
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
  }

  stage.template operator()<GRPS_A>(a, n, n0, c_beg, lds_ab(0));
  stage.template operator()<GRPS_B>(b, k2, k0, c_beg, lds_bb(0));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // wave-uniform: of the WCOL waves that read the same A fragments, one sums
  const bool do_bias = (dbias != nullptr) && (k0 == 0) && wave % WCOL == 0;

  // fragment read via ds_read_b64_tr_b16: each 16-lane group passes
  // CONSECUTIVE 8-B addresses covering one 128-B [4 m][16 col] sub-tile;
  // the hardware redistributes so lane receives COLUMN (l&15) — i.e. 4
  // contract-consecutive elements.  Two reads (sub-tiles m+0..3, m+4..7)
  // assemble the 8-element MFMA k fragment.
  auto frag = [&](const char* img, int block16, int s) {
    const char* p = img + (block16 >> 2) * GROUP_BYTES +
                    (s * 4 + (lane >> 4)) * 1024 + (block16 & 3) * 256 +
                    (lane & 15) * 8;
    bf16x4_g lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (__attribute__((address_space(3))) bf16x4_g*)p);
    bf16x4_g hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (__attribute__((address_space(3))) bf16x4_g*)(p + 128));
    union { bf16x8 v8; bf16x4_g v4[2]; } u;
    u.v4[0] = lo;
    u.v4[1] = hi;
    return u.v8;
  };

  // bias grad (db = colsum of g): the A fragments already pass EVERY g
  // element through registers, so accumulate there instead of a separate
  // 32-B-strided LDS sweep (PMC: that sweep was 8.5x the NT kernel's LDS
  // bank conflicts).  Each column's sum lands spread over the wave's four
  // 16-lane groups (different k slices) — folded by shfl at the end; the
  // WCOL waves sharing a wm row-block read identical fragments, so only
  // wave % WCOL == 0 contributes.
  auto mma = [&](const char* la, const char* lb) {
#pragma unroll
    for (int s = 0; s < BKM / 32; ++s) {
      bf16x8 av[FM], bv[FN];
#pragma unroll
      for (int mi = 0; mi < FM; ++mi) av[mi] = frag(la, (wm >> 4) + mi, s);
#pragma unroll
      for (int ni = 0; ni < FN; ++ni) bv[ni] = frag(lb, (wn >> 4) + ni, s);
      if (do_bias)
#pragma unroll
        for (int mi = 0; mi < FM; ++mi)
#pragma unroll
          for (int j = 0; j < 8; ++j) dbacc[mi] += (float)av[mi][j];
#pragma unroll
      for (int mi = 0; mi < FM; ++mi)
#pragma unroll
        for (int ni = 0; ni < FN; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    }
  };

  int buf = 0;
  for (int cc = c_beg + BKM; cc < c_end; cc += BKM) {
    stage.template operator()<GRPS_A>(a, n, n0, cc, lds_ab(buf ^ 1));
    stage.template operator()<GRPS_B>(b, k2, k0, cc, lds_bb(buf ^ 1));
    mma(lds_ab(buf), lds_bb(buf));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    buf ^= 1;
  }
  // m tail: the slice that ends at m_full owns the m % BKM rows behind it
  // as one more, partial, step.  Every wave left the other buffer at the
  // loop's last barrier, so it is staged under the final full step's MFMAs;
  // block-uniform and run once, hence not part of the double-buffered loop.
  const int rem = m - m_full;
  const bool tail = rem > 0 && c_end == m_full;
  if (tail) {
    stage.template operator()<GRPS_A, true>(a, n, n0, m_full,
                                            lds_ab(buf ^ 1));
    stage.template operator()<GRPS_B, true>(b, k2, k0, m_full,
                                            lds_bb(buf ^ 1));
  }
  mma(lds_ab(buf), lds_bb(buf));
  if (tail) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // zero the rows >= rem of every [8][16] block in BOTH images (32 B per
    // row and block; 64 chunks of 16 B per octet): a zero on one side only
    // would turn an Inf in the duplicated row of the other into a NaN
    const u32x4_t z = {0u, 0u, 0u, 0u};
    for (int t = threadIdx.x; t < (BM + BN) / 16 * BKM * 2; t += THREADS) {
      const bool in_b = t >= BM / 16 * BKM * 2;
      const int u = in_b ? t - BM / 16 * BKM * 2 : t;  // 16-B chunk in image
      if ((u >> 6) % OCTS * 8 + ((u & 15) >> 1) >= rem)
        *reinterpret_cast<u32x4_t*>(
            (in_b ? lds_bb(buf ^ 1) : lds_ab(buf ^ 1)) + u * 16) = z;
    }
    __syncthreads();
    mma(lds_ab(buf ^ 1), lds_bb(buf ^ 1));
  }
  if (do_bias) {
#pragma unroll
    for (int mi = 0; mi < FM; ++mi) {
      float v = dbacc[mi];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if ((lane >> 4) == 0)
        atomicAdd(&dbias[n0 + wm + mi * 16 + (lane & 15)], v);
    }
  }

  const int fcol = lane & 15;
  const int frow = (lane >> 4) * 4;
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + wm + mi * 16 + frow + r;
        const int col = k0 + wn + ni * 16 + fcol;
        if (slices != 1)
          atomicAdd(&c[(long)row * k2 + col], acc[mi][ni][r]);
        else if (ACC)  // gradient sink: this thread owns the element
          c[(long)row * k2 + col] += acc[mi][ni][r];
        else
          c[(long)row * k2 + col] = acc[mi][ni][r];
      }
}

// Both operands bf16 contract-major (g [m][n], x [m][k2]); the m tail rows
// beyond the last BKM multiple are a partial last step inside the kernel.
// When dbias sits right behind c (one [n*k2 + n] buffer, as the binding
// allocates them) a single memset clears both.  `acc`: c and dbias are
// gradient sinks that already hold a sum — nothing is cleared and every
// element is added to.
//
// Output tile: gemm_dispatch::glds_tn_tile() picks it (128x128 today); `tile`
// forces 128x128, 256x128 or 256x256 (TN_AUTO: the dispatch's choice), and
// set_glds_tn_tile() moves the automatic choice for A/B runs and tests.
static int g_glds_tn_tile = gemm_dispatch::TN_AUTO;  // test hook
void set_glds_tn_tile(int tile) { g_glds_tn_tile = tile; }

int glds_tn_tile_for(int m, int n, int k2, int tile) {
  namespace gd = gemm_dispatch;
  // a tile asked for by the caller must fit the shape (-1 otherwise) ...
  if (tile != gd::TN_AUTO)
    return gd::glds_tn_tile_ok(tile, m, n, k2) ? tile : -1;
  // ... a process-wide override applies where it fits
  if (g_glds_tn_tile != gd::TN_AUTO &&
      gd::glds_tn_tile_ok(g_glds_tn_tile, m, n, k2))
    return g_glds_tn_tile;
  return gd::glds_tn_tile(m, n, k2);
}

template <int BM, int BN>
static void launch_glds_tn_tile(const __bf16* a, const __bf16* b, float* c,
                                float* dbias, int m, int n, int k2,
                                hipStream_t s, bool acc) {
  constexpr int BKM = 64;
  const int tiles = (n / BM) * (k2 / BN);
  // split-K over the full BKM steps; the tail step rides the last slice and
  // does not change the split (m and m - m % BKM slice alike)
  const int slices = gemm_dispatch::glds_tn_slices(m, tiles);
  if (acc)
    gemm_a16_glds_tn_kernel<BM, BN, BKM, 512, true>
        <<<dim3(tiles * slices), dim3(512), 0, s>>>(a, b, c, dbias, m, n, k2,
                                                    slices);
  else
    gemm_a16_glds_tn_kernel<BM, BN, BKM>
        <<<dim3(tiles * slices), dim3(512), 0, s>>>(a, b, c, dbias, m, n, k2,
                                                    slices);
}

void launch_gemm_a16_glds_tn(const void* a_v, const void* b_v, float* c,
                             float* dbias, int m, int n, int k2,
                             hipStream_t s, bool acc, int tile) {
  namespace gd = gemm_dispatch;
  const __bf16* a = (const __bf16*)a_v;
  const __bf16* b = (const __bf16*)b_v;
  const long nc = (long)n * k2;
  if (!acc) {
    if (dbias == c + nc) {
      HIP_CHECK(hipMemsetAsync(c, 0, (nc + n) * sizeof(float), s));
    } else {
      HIP_CHECK(hipMemsetAsync(c, 0, nc * sizeof(float), s));
      if (dbias) HIP_CHECK(hipMemsetAsync(dbias, 0, n * sizeof(float), s));
    }
  }
  switch (glds_tn_tile_for(m, n, k2, tile)) {
    case gd::TN_256x256:
      return launch_glds_tn_tile<256, 256>(a, b, c, dbias, m, n, k2, s, acc);
    case gd::TN_256x128:
      return launch_glds_tn_tile<256, 128>(a, b, c, dbias, m, n, k2, s, acc);
    default:
      return launch_glds_tn_tile<128, 128>(a, b, c, dbias, m, n, k2, s, acc);
  }
}

// ---------------------------------------------------------------------------
// Skinny NN dgrad: dx[m,k2] = g[m,n] . w[n,k2] for TINY m (the P-table
// backward: rpctype has ~5 rows).  The tiled kernel's boundary path runs
// per-element guarded scalar staging on 8 underoccupied workgroups
// (measured 85 us for 2.6 MFLOP at [5,512]x[512,512]); here one wave owns
// one (row, 64-column block) output strip — w reads are lane-coalesced,
// g[i,n] is a broadcast scalar, fully deterministic.
// ---------------------------------------------------------------------------
template <typename OT = float>
__global__ void gemm_skinny_nn_kernel(const __bf16* __restrict__ g,
                                      const float* __restrict__ w,
                                      OT* __restrict__ dx, int m, int n,
                                      int k2) {
  const int i = blockIdx.x;           // output row
  const int j0 = blockIdx.y * PERTGNN_WAVE;
  const int j = j0 + threadIdx.x;     // output column
  if (i >= m || j >= k2) return;
  // 8-deep unroll with split accumulators: the w loads of a batch issue
  // together (a bare loop serializes one memory latency per iteration —
  // the whole kernel is a ~20-wave latency chain)
  float a0 = 0.f, a1 = 0.f;
  int t = 0;
  for (; t + 8 <= n; t += 8) {
    float gv[8], wv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) gv[u] = (float)g[(long)i * n + t + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) wv[u] = w[(long)(t + u) * k2 + j];
#pragma unroll
    for (int u = 0; u < 8; u += 2) {
      a0 += gv[u] * wv[u];
      a1 += gv[u + 1] * wv[u + 1];
    }
  }
  for (; t < n; ++t) a0 += (float)g[(long)i * n + t] * w[(long)t * k2 + j];
  dx[(long)i * k2 + j] = (OT)(a0 + a1);
}

void launch_gemm_skinny_nn(const void* g_v, const float* w, float* dx, int m,
                           int n, int k2, hipStream_t s) {
  gemm_skinny_nn_kernel<<<dim3(m, (k2 + PERTGNN_WAVE - 1) / PERTGNN_WAVE),
                          dim3(PERTGNN_WAVE), 0, s>>>(
      (const __bf16*)g_v, w, dx, m, n, k2);
}

// ---------------------------------------------------------------------------
// Grouped P-table GEMMs.  Every layer projects the same two embedding tables
// (interface [V,H], rpctype [R,H]) through its own [H,H] edge weights; run
// per layer these are 4-32-block launches that leave most of the chip idle.
// The three kernels below take ALL layers' operands in one launch: the group
// is found from blockIdx, and the per-group pointers and row counts arrive
// in a descriptor struct passed BY VALUE (kernarg: no device pointer array,
// no host-to-device copy, and a captured graph bakes the addresses in).  A
// struct holds at most PT_MAX_GROUPS groups; the launchers split above that.
//
// All three use the 64x64x64 register-staging tile of the small-shape
// kernels above (36 KB LDS, 4 blocks/CU; 45 KB and 3 in the dgrad).  A
// block's result depends only on its operands and the ascending order of
// its 32-wide MFMA K steps, never on the grid, so the forward is
// bit-identical to the per-layer gemm_bf16_nt_kernel launches whatever tile
// those picked.
// ---------------------------------------------------------------------------

#define PT_MAX_GROUPS 32
#define PT_TILE 64

struct PTFwdArgs {
  const float* a[PT_MAX_GROUPS];   // table [m_g, k]
  const float* w[PT_MAX_GROUPS];   // weight [n, k]
  __bf16* c[PT_MAX_GROUPS];        // out [m_g, n]
  int m[PT_MAX_GROUPS];
  int blk_beg[PT_MAX_GROUPS + 1];  // first block of each group
  int groups, n, k;
};

// C_g (bf16) = A_g (fp32) @ W_g^T (fp32), heterogeneous m_g
__launch_bounds__(BGEMM_THREADS)
__global__ void ptables_fwd_kernel(const PTFwdArgs p) {
  constexpr int BM = PT_TILE, BN = PT_TILE, BK = 64;
  constexpr int LDW = BK + BGEMM_PAD;
  constexpr int WCOL = BGEMM_THREADS / PERTGNN_WAVE / 2;
  constexpr int FM = (BM / 2) / 16, FN = (BN / WCOL) / 16;
  __shared__ __bf16 lds_a[2][BM * LDW];
  __shared__ __bf16 lds_b[2][BN * LDW];
  const int bid = blockIdx.x;
  int g = 0;
  while (g + 1 < p.groups && bid >= p.blk_beg[g + 1]) ++g;
  const float* __restrict__ a = p.a[g];
  const float* __restrict__ b = p.w[g];
  const int m = p.m[g], n = p.n, k = p.k;
  const int tile = bid - p.blk_beg[g];
  const int tiles_n = (n + BN - 1) / BN;
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;
  const int wave = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int wm = (wave / WCOL) * (BM / 2);
  const int wn = (wave % WCOL) * (BN / WCOL);

  BWaveTile<FM, FN, BK, __bf16> wt;
  wt.zero();
  int buf = 0;
  bstage_cmin<BM, BK, __bf16>(a, k, m0, 0, m, k, lds_a[0]);
  bstage_cmin<BN, BK, __bf16>(b, k, n0, 0, n, k, lds_b[0]);
  __syncthreads();
  StageCmin<BM, BK, __bf16, float> sa;
  StageCmin<BN, BK, __bf16, float> sb;
  for (int k0 = BK; k0 < k; k0 += BK) {
    sa.load(a, k, m0, k0, m, k);
    sb.load(b, k, n0, k0, n, k);
    wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
    sa.commit(lds_a[buf ^ 1]);
    sb.commit(lds_b[buf ^ 1]);
    __syncthreads();
    buf ^= 1;
  }
  wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
  wt.store(p.c[g], n, m0 + wm, n0 + wn, m, n, nullptr, 0, lane);
}

struct PTDgradArgs {
  const __bf16* dp[PT_MAX_GROUPS];  // (dP_l, W_l) pairs, table 0's first
  const float* w[PT_MAX_GROUPS];
  int pair_beg[3];                  // table t owns pairs [beg[t], beg[t+1])
  float* out[2];                    // dT_t [m_t, h]
  int m[2];
  int blk_beg[3];
  int h;
  int splits;   // >1: each block takes 1/splits of its table's pairs
  // per table: 0 stores, 1 adds atomically (out is zeroed, a gradient sink
  // shared by several blocks, or holds an earlier launch's sum), 2 adds with
  // a plain read-modify-write (a gradient sink, one block per element)
  int mode[2];
};

// dT_t (fp32) = sum_l dP_l (bf16) @ W_l (fp32) for both tables: the K loop
// walks the table's (dP_l, W_l) pairs — one GEMM with K = L*h — so the
// per-layer dgrads and the L-1 adds of their results become one register
// accumulation in a fixed order (or, with `splits`, a few atomic partials).
__launch_bounds__(BGEMM_THREADS)
__global__ void ptables_dgrad_kernel(const PTDgradArgs p) {
  constexpr int BM = PT_TILE, BN = PT_TILE, BK = 64;
  constexpr int LDW = BK + BGEMM_PAD;
  constexpr int WCOL = BGEMM_THREADS / PERTGNN_WAVE / 2;
  constexpr int FM = (BM / 2) / 16, FN = (BN / WCOL) / 16;
  __shared__ __bf16 lds_a[2][BM * LDW];
  __shared__ __bf16 lds_b[2][BN * LDW];
  __shared__ __bf16 lds_b_lo[BN * LDW];  // single buffer: 45 KB, 3 blocks/CU
  const int bid = blockIdx.x;
  const int t = bid >= p.blk_beg[1] ? 1 : 0;
  const int m = p.m[t], h = p.h;
  // Tables of at most 16 rows (rpctype) keep the low half of the fp32
  // weights in a second B image and run a second MFMA over it: their
  // per-layer dgrad is the skinny fp32-FMA kernel, which never rounded W,
  // and a bf16-rounded W here would move that gradient by 2^-9 relative
  // (1e-5 at the flagship) where two runs of one tree differ by 1e-8.
  const bool exact_w = m <= 16;
  const int tiles_n = (h + BN - 1) / BN;
  const int tiles = ((m + BM - 1) / BM) * tiles_n;
  const int rel = bid - p.blk_beg[t];
  const int split = rel / tiles;
  const int tile = rel % tiles;
  const int m0 = (tile / tiles_n) * BM;
  const int n0 = (tile % tiles_n) * BN;
  const int wave = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int wm = (wave / WCOL) * (BM / 2);
  const int wn = (wave % WCOL) * (BN / WCOL);

  const int npairs = p.pair_beg[t + 1] - p.pair_beg[t];
  const int per = (npairs + p.splits - 1) / p.splits;
  const int l_beg = p.pair_beg[t] + min(npairs, split * per);
  const int l_end = p.pair_beg[t] + min(npairs, (split + 1) * per);
  // an adding block with no pairs adds nothing; a storing one writes zeros
  const int mode = p.mode[t];
  if (mode != 0 && l_beg >= l_end) return;

  // Two-level sum: each pair's K = h chain runs in the MFMA accumulator from
  // zero, exactly as its per-layer dgrad would, and is then added to `tot`
  // with one fp32 add.  One chain over all L*h was measured 3x less accurate
  // than the per-layer path at L = 3, h = 256 (3.1e-6 vs 1.1e-6 on outputs
  // of 7): every MFMA step rounds at the magnitude of the running sum.
  BWaveTile<FM, FN, BK, __bf16> wt;
  f32x4 tot[FM][FN];
  wt.zero();
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) tot[i][j] = {0.f, 0.f, 0.f, 0.f};
  if (l_beg < l_end) {
    int buf = 0;
    int l = l_beg, c0 = 0;  // the K step staged in lds[buf]
    StageCmin<BM, BK, __bf16, __bf16> sa;
    StageCmaj<BN, BK, __bf16, float> sb;
    bstage_cmin<BM, BK, __bf16>(p.dp[l], h, m0, 0, m, h, lds_a[0]);
    sb.load(p.w[l], h, 0, n0, h, h);
    sb.commit(lds_b[0]);
    if (exact_w) sb.commit_lo(lds_b_lo);
    __syncthreads();
    while (true) {
      int nl = l, nc = c0 + BK;
      if (nc >= h) { nc = 0; ++nl; }
      const bool more = nl < l_end;
      if (more) {
        sa.load(p.dp[nl], h, m0, nc, m, h);
        sb.load(p.w[nl], h, nc, n0, h, h);
      }
      wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
      if (exact_w) wt.mma(lds_a[buf], lds_b_lo, wm, wn, lane);
      if (nc == 0) {  // that was pair l's last step
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            tot[i][j] += wt.acc[i][j];
            wt.acc[i][j] = {0.f, 0.f, 0.f, 0.f};
          }
      }
      if (!more) break;
      sa.commit(lds_a[buf ^ 1]);
      sb.commit(lds_b[buf ^ 1]);
      if (exact_w) {  // every wave is done reading the one lo image
        __syncthreads();
        sb.commit_lo(lds_b_lo);
      }
      __syncthreads();
      buf ^= 1;
      l = nl;
      c0 = nc;
    }
  }

  float* __restrict__ c = p.out[t];
  const int fcol = lane & 15;
  const int frow = (lane >> 4) * 4;
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + mi * 16 + frow + r;
        const int col = n0 + wn + ni * 16 + fcol;
        if (row < m && col < h) {
          if (mode == 1)
            atomicAdd(&c[(long)row * h + col], tot[mi][ni][r]);
          else if (mode == 2)
            c[(long)row * h + col] += tot[mi][ni][r];
          else
            c[(long)row * h + col] = tot[mi][ni][r];
        }
      }
}

struct PTWgradArgs {
  const __bf16* dp[PT_MAX_GROUPS];  // dP_g [m_g, h]
  const float* a[PT_MAX_GROUPS];    // table [m_g, h]
  float* dw[PT_MAX_GROUPS];         // dW_g [h, h]
  int m[PT_MAX_GROUPS];
  int slices[PT_MAX_GROUPS];        // split-K over m_g; >1 adds atomically
  int blk_beg[PT_MAX_GROUPS + 1];
  int groups, h;
  unsigned acc;  // bit g: dw[g] is a gradient sink, add instead of store
};

// dW_g (fp32) = dP_g^T (bf16) @ A_g (fp32), reducing over m_g
__launch_bounds__(BGEMM_THREADS)
__global__ void ptables_wgrad_kernel(const PTWgradArgs p) {
  constexpr int BM = PT_TILE, BN = PT_TILE, BK = 64;
  constexpr int LDW = BK + BGEMM_PAD;
  constexpr int WCOL = BGEMM_THREADS / PERTGNN_WAVE / 2;
  constexpr int FM = (BM / 2) / 16, FN = (BN / WCOL) / 16;
  __shared__ __bf16 lds_a[2][BM * LDW];
  __shared__ __bf16 lds_b[2][BN * LDW];
  const int bid = blockIdx.x;
  int g = 0;
  while (g + 1 < p.groups && bid >= p.blk_beg[g + 1]) ++g;
  const __bf16* __restrict__ a = p.dp[g];
  const float* __restrict__ b = p.a[g];
  const int m = p.m[g], h = p.h, slices = p.slices[g];
  const int rel = bid - p.blk_beg[g];
  const int tiles_k = (h + BN - 1) / BN;
  const int tile_id = rel / slices;
  const int slice = rel % slices;
  const int n0 = (tile_id / tiles_k) * BM;
  const int k0 = (tile_id % tiles_k) * BN;
  const int wave = threadIdx.x / PERTGNN_WAVE;
  const int lane = threadIdx.x % PERTGNN_WAVE;
  const int wm = (wave / WCOL) * (BM / 2);
  const int wn = (wave % WCOL) * (BN / WCOL);

  const int per_slice = ((m + slices - 1) / slices + BK - 1) / BK * BK;
  const int c_beg = slice * per_slice;
  const int c_end = min(m, c_beg + per_slice);
  const bool acc = (p.acc >> g) & 1u;
  if ((slices > 1 || acc) && c_beg >= c_end) return;

  BWaveTile<FM, FN, BK, __bf16> wt;
  wt.zero();
  if (c_beg < c_end) {
    int buf = 0;
    bstage_cmaj<BM, BK, __bf16>(a, h, c_beg, n0, c_end, h, lds_a[0]);
    bstage_cmaj<BN, BK, __bf16>(b, h, c_beg, k0, c_end, h, lds_b[0]);
    __syncthreads();
    StageCmaj<BM, BK, __bf16, __bf16> sa;
    StageCmaj<BN, BK, __bf16, float> sb;
    for (int cc = c_beg + BK; cc < c_end; cc += BK) {
      sa.load(a, h, cc, n0, c_end, h);
      sb.load(b, h, cc, k0, c_end, h);
      wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
      sa.commit(lds_a[buf ^ 1]);
      sb.commit(lds_b[buf ^ 1]);
      __syncthreads();
      buf ^= 1;
    }
    wt.mma(lds_a[buf], lds_b[buf], wm, wn, lane);
  }

  float* __restrict__ c = p.dw[g];
  const int fcol = lane & 15;
  const int frow = (lane >> 4) * 4;
#pragma unroll
  for (int mi = 0; mi < FM; ++mi)
#pragma unroll
    for (int ni = 0; ni < FN; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + wm + mi * 16 + frow + r;
        const int col = k0 + wn + ni * 16 + fcol;
        if (row < h && col < h) {
          if (slices != 1)
            atomicAdd(&c[(long)row * h + col], wt.acc[mi][ni][r]);
          else if (acc)
            c[(long)row * h + col] += wt.acc[mi][ni][r];
          else
            c[(long)row * h + col] = wt.acc[mi][ni][r];
        }
      }
}

int ptables_max_groups() { return PT_MAX_GROUPS; }

static inline int pt_tiles(int rows, int cols) {
  return ((rows + PT_TILE - 1) / PT_TILE) * ((cols + PT_TILE - 1) / PT_TILE);
}

// forward: groups = every (table, layer) product; m[g] rows, all [.,k]x[n,k]^T
void launch_ptables_fwd(int groups, const float* const* a,
                        const float* const* w, void* const* c, const int* m,
                        int n, int k, hipStream_t s) {
  for (int g0 = 0; g0 < groups; g0 += PT_MAX_GROUPS) {
    PTFwdArgs p;
    p.groups = min(PT_MAX_GROUPS, groups - g0);
    p.n = n;
    p.k = k;
    int blocks = 0;
    for (int i = 0; i < p.groups; ++i) {
      p.a[i] = a[g0 + i];
      p.w[i] = w[g0 + i];
      p.c[i] = (__bf16*)c[g0 + i];
      p.m[i] = m[g0 + i];
      p.blk_beg[i] = blocks;
      blocks += pt_tiles(m[g0 + i], n);
    }
    p.blk_beg[p.groups] = blocks;
    if (blocks > 0)
      ptables_fwd_kernel<<<dim3(blocks), dim3(BGEMM_THREADS), 0, s>>>(p);
  }
}

// table dgrad: npairs[t] (dP, W) pairs per table, table 0's first in dp/w.
// Writes out[t] [m[t], h] unless addto[t]: the caller cleared that output or
// it is a gradient sink, and every launch adds to it.  `splits` may exceed 1
// only when both outputs are added to (the adds are then atomic).  With
// splits == 1 the sum order is fixed: one block per element, the first
// launch stores (or, into a sink, adds with a plain read-modify-write) and
// launches past the first (more pairs than one struct holds) add onto that
// in stream order.
void launch_ptables_dgrad(const void* const* dp, const float* const* w,
                          const int* npairs, float* const* out, const int* m,
                          int h, int splits, const bool* addto,
                          hipStream_t s) {
  if (!(addto[0] && addto[1])) splits = 1;
  const int half = PT_MAX_GROUPS / 2;  // pairs per table per launch
  const int most = max(npairs[0], npairs[1]);
  bool first = true;
  for (int l0 = 0; l0 < most || first; l0 += half) {
    PTDgradArgs p;
    int np = 0, blocks = 0;
    for (int t = 0; t < 2; ++t) {
      const int base = t == 0 ? 0 : npairs[0];
      const int cnt = max(0, min(half, npairs[t] - l0));
      p.pair_beg[t] = np;
      for (int i = 0; i < cnt; ++i) {
        p.dp[np] = (const __bf16*)dp[base + l0 + i];
        p.w[np] = w[base + l0 + i];
        ++np;
      }
      p.out[t] = out[t];
      p.m[t] = m[t];
      p.blk_beg[t] = blocks;
      // a table with nothing (more) to add needs blocks only to store zeros
      if (cnt > 0 || (first && !addto[t]))
        blocks += pt_tiles(m[t], h) * splits;
      p.mode[t] = (splits > 1 || !first) ? 1 : addto[t] ? 2 : 0;
    }
    p.pair_beg[2] = np;
    p.blk_beg[2] = blocks;
    p.h = h;
    p.splits = splits;
    if (blocks > 0)
      ptables_dgrad_kernel<<<dim3(blocks), dim3(BGEMM_THREADS), 0, s>>>(p);
    first = false;
  }
}

// weight wgrad: dw[g] [h,h] = dp[g]^T @ a[g] over m[g] rows.  Outside
// PERTGNN_DETERMINISTIC=1 large-m groups are split-K'd with atomics, and the
// caller must then have zeroed every dw that is not a gradient sink (returns
// true if it relies on that); `probe` only answers that question without
// launching.  sink[g] (may be null: none): dw[g] already holds a sum and is
// added to, never stored or cleared.
bool launch_ptables_wgrad(int groups, const void* const* dp,
                          const float* const* a, float* const* dw,
                          const int* m, int h, bool probe, hipStream_t s,
                          const bool* sink) {
  const bool det = pertgnn_deterministic();
  int total_tiles = 0;
  for (int g = 0; g < groups; ++g) total_tiles += pt_tiles(h, h);
  bool any_split = false;
  for (int g0 = 0; g0 < groups; g0 += PT_MAX_GROUPS) {
    PTWgradArgs p;
    p.groups = min(PT_MAX_GROUPS, groups - g0);
    p.h = h;
    p.acc = 0u;
    int blocks = 0;
    for (int i = 0; i < p.groups; ++i) {
      const int mg = m[g0 + i];
      if (sink && sink[g0 + i]) p.acc |= 1u << i;
      int slices = 1;
      while (!det && (long)total_tiles * slices < 2048 && slices < 64 &&
             (long)slices * 64 * 4 < mg)
        slices *= 2;
      any_split |= slices > 1 && !(sink && sink[g0 + i]);
      p.dp[i] = (const __bf16*)dp[g0 + i];
      p.a[i] = a[g0 + i];
      p.dw[i] = dw[g0 + i];
      p.m[i] = mg;
      p.slices[i] = slices;
      p.blk_beg[i] = blocks;
      blocks += pt_tiles(h, h) * slices;
    }
    p.blk_beg[p.groups] = blocks;
    if (!probe && blocks > 0)
      ptables_wgrad_kernel<<<dim3(blocks), dim3(BGEMM_THREADS), 0, s>>>(p);
  }
  return any_split;
}
