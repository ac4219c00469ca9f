// Host-only dispatch predicates of the linear / GEMM paths.  The launchers in
// gemm.hip and gemm_bf16.hip, the linear_* bindings and the linear_path()
// binding all decide through these, so what linear_path() reports is what
// runs.  Plain C++: no device code, no HIP call, no environment read (the
// callers pass PERTGNN_DETERMINISTIC in; the experiment knobs stay with the
// launchers and are assumed at their defaults by linear_path()).
//
// Shapes follow the torch Linear layout: x [m, k], w [n, k], y / g [m, n].
#pragma once

namespace gemm_dispatch {

// NT / NN kernels with register (or fp32) staging: the 128x128 tile for big
// shapes, 64x64 otherwise.  `cols` is the output width (n forward, k dgrad).
inline bool tile128(int m, int cols) { return m >= 512 && cols >= 128; }

// TN (wgrad) kernels with register (or fp32) staging: tile by the output
inline bool tn_tile128(int n, int k2) { return n >= 128 && k2 >= 128; }

inline int tn_tiles(int n, int k2) {
  const int b = tn_tile128(n, k2) ? 128 : 64;
  return ((n + b - 1) / b) * ((k2 + b - 1) / b);
}

// split-K slice count of those TN kernels: double while the grid is under
// 512 blocks and every slice keeps at least four K steps of `step` rows
// (32 for the fp32 kernel, 64 for the 16-bit ones); one slice when
// deterministic.
inline int tn_slices(int m, int tiles, int step, bool deterministic) {
  int slices = 1;
  while (!deterministic && tiles * slices < 512 && slices < 64 &&
         (long)slices * step * 4 < m)
    slices *= 2;
  return slices;
}

// forward on the glds NT kernel: full 128-wide column tiles, full K steps of
// 32 (which also makes the rows 16-B aligned)
inline bool fwd_glds_ok(int m, int n, int k) {
  return m >= 512 && n % 128 == 0 && k % 32 == 0;
}

// dgrad as glds NT over the transposed weight image (contraction n, width k);
// shared with the forward so that it can hand the image over
inline bool dgrad_glds_ok(int m, int n, int k) {
  return m >= 512 && k % 128 == 0 && n % 64 == 0;
}

// wgrad on the glds TN kernel; its split-K adds atomically, so not in the
// deterministic mode
inline bool wgrad_glds_ok(int m, int n, int k, bool deterministic) {
  return !deterministic && m >= 512 && n % 128 == 0 && k % 128 == 0;
}

// 128x256 single-column-tile variant of the glds NT kernel (`cols` is the
// output width, `contract` the contraction length)
inline bool glds_nt_wide(int m, int cols, int contract) {
  return m / 128 >= 1024 && cols == 256 && contract % 32 == 0;
}

// Forward on the glds NT family: the streaming kernel (every block stages its
// own A and W K-tiles) or the A-resident kernel (one block keeps a row tile
// of A in LDS and sweeps the column tiles).  Both give the same bits, so
// linear_path() reports the family ("glds_nt_128x128") for either.
enum FwdVariant { FWD_AUTO = 0, FWD_STREAM = 1, FWD_RESIDENT = 2 };

// shapes the two kernels can run at all (a forced variant takes any of them)
inline bool fwd_stream_can(int m, int n, int k) {
  return m >= 1 && n % 128 == 0 && k % 32 == 0;
}
inline bool fwd_resident_can(int m, int n, int k) {
  return m >= 1 && n % 128 == 0 && k == 256;
}

// Geometry the A-resident kernel runs by default (1: 128-row tiles, one
// block per CU; 2: 64-row tiles, two blocks per CU) and the row count from
// which it takes over from the streaming kernel.  Measured at n = 1024,
// k = 256, us per call, streaming / geometry 1 / geometry 2
// (profiles/25_fwd_resident.md): 16 384 rows 22.7 / 25.9 / 29.3, 45 056
// 47.8 / 51.1 / 50.0, 57 344 62.3 / 53.6 / 58.1, 65 536 72.6 / 56.6 / 61.5,
// 73 728 74.5 / 73.6 / 73.3, 90 112 92.3 / 77.5 / 84.4, 180 762 181.5 /
// 150.2 / 158.1.  Geometry 1 wins from 57 344 rows (448 row tiles) on and
// loses at 45 056 and below, where its grid is under two blocks per CU.
constexpr int FWD_RESIDENT_GEOM = 1;
constexpr int FWD_RESIDENT_MIN_M = 57344;

// the A-resident kernel by default: the k == 256 forward from
// FWD_RESIDENT_MIN_M rows on, except where the 128x256 tile already streams
// A once (n == 256 at >= 1024 row tiles)
inline bool fwd_resident_ok(int m, int n, int k) {
  return fwd_glds_ok(m, n, k) && fwd_resident_can(m, n, k) &&
         m >= FWD_RESIDENT_MIN_M && !glds_nt_wide(m, n, k);
}

// -> FWD_STREAM, FWD_RESIDENT, or 0 where the shape is not on the glds
// forward.  `forced` (the set_fwd_variant() hook) names the kernel to take
// on every shape the A-resident kernel can run, rows below the glds gate
// included, so that the two can be compared there; on any other shape the
// automatic choice holds.  `no_resident` is PERTGNN_NO_FWD_RESIDENT=1.
inline int fwd_variant(int m, int n, int k, int forced, bool no_resident) {
  if (forced != FWD_AUTO && fwd_resident_can(m, n, k)) return forced;
  if (!fwd_glds_ok(m, n, k)) return 0;
  return fwd_resident_ok(m, n, k) && !no_resident ? FWD_RESIDENT : FWD_STREAM;
}

// split-K slice count of the glds TN kernel (K steps of 64 rows; the m % 64
// tail rides the last non-empty slice and does not change the split)
inline int glds_tn_slices(int m, int tiles) {
  constexpr int BKM = 64;
  int slices = 1;
  while (tiles * slices < 512 && slices < 64 &&
         (long)slices * BKM * 4 < m - m % BKM)
    slices *= 2;
  return slices;
}

// Output tile of the glds TN kernel, rows (of n) x columns (of k).
enum TnTile { TN_AUTO = 0, TN_128x128 = 1, TN_256x128 = 2, TN_256x256 = 3 };

inline int tn_tile_rows(int tile) { return tile == TN_128x128 ? 128 : 256; }
inline int tn_tile_cols(int tile) { return tile == TN_256x256 ? 256 : 128; }
inline const char* tn_tile_name(int tile) {
  return tile == TN_256x256 ? "256x256"
         : tile == TN_256x128 ? "256x128" : "128x128";
}

// whether the glds TN kernel can run this shape with this tile
inline bool glds_tn_tile_ok(int tile, int m, int n, int k) {
  return tile >= TN_128x128 && tile <= TN_256x256 && m >= 512 &&
         n % tn_tile_rows(tile) == 0 && k % tn_tile_cols(tile) == 0;
}

// The tile the glds TN kernel takes by default: 128x128 at every shape.  The
// wide tiles stage each operand row block half as often, but at one block
// per CU they lose more in latency hiding than they save in staged bytes
// (measured at [180k, 1024]^T x [180k, 256] and at 45k rows:
// profiles/21_wgrad_tiles.md), so they run only where a caller forces them.
inline int glds_tn_tile(int /*m*/, int /*n*/, int /*k*/) { return TN_128x128; }

inline int glds_tn_tiles(int tile, int n, int k) {
  return (n / tn_tile_rows(tile)) * (k / tn_tile_cols(tile));
}

// one-wave-per-strip NN kernel for the tiny-row dgrad (fp32 x, bf16 g)
inline bool dgrad_skinny(int m) { return m <= 16; }

}  // namespace gemm_dispatch
