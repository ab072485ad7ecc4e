// Dynamic time warping of a batch of feature-sequence pairs in ONE launch (DESIGN.md 3.6 holds the definition).  Pair u is
// a[ao[u] .. ao[u + 1]) against b[bo[u] .. bo[u + 1]), rows of K floats; with Ta and Tb rows:
//   c(i, j) = sqrt(sum_k (a[i, k] - b[j, k])^2)      fp32, k ascending in one chain, the difference, the product and the sum each
//                                                    rounded (no fused multiply-add), the square root correctly rounded
//   D(0, 0) = c(0, 0);  D(i, j) = best + c(i, j)     best: the smallest of the predecessors that exist, taken in the order diagonal
//                                                    (i-1, j-1), up (i-1, j), left (i, j-1); a later one replaces an earlier one
//                                                    only when it is strictly smaller
//   L(0, 0) = 1;        L(i, j) = L(chosen) + 1
// cost[u] = D(Ta-1, Tb-1), steps[u] = L(Ta-1, Tb-1); with dirs / path the chosen predecessor of every cell goes to a byte of the
// caller's workspace and one lane walks back from the corner.  These are the operations of utils/mel_distance.py dtw_numpy in its
// order, so the two agree bit for bit, ties included.
//
// One workgroup of DTW_NT threads per pair, an anti-diagonal wavefront: diagonal d holds the cells i + j == d, one barrier per
// diagonal, Ta + Tb - 1 of them.  Row i belongs to thread i % DTW_NT for the whole launch (dtw_k<R>: R rows a lane, the smallest of
// 1 / 2 / 4 that covers the caller's max_ta).  The local costs do not depend on the recurrence, so a lane computes them DTW_Q
// diagonals ahead: every DTW_Q diagonals it forms c(i, j .. j + DTW_Q - 1) of each of its rows in registers - a[i, k] loaded once
// for the DTW_Q columns, all loads in flight together - and the DTW_Q diagonals that follow touch only LDS: one memory latency per
// DTW_Q barriers instead of one per barrier.  D and L of the last three diagonals sit in LDS indexed by ROW: cell (i, j) reads
// diag = [d-2][i-1], up = [d-1][i-1], left = [d-1][i] and writes [d][i]; the slot written on diagonal d was last read on diagonal
// d - 1, behind that diagonal's barrier.  3 x 2048 x (4 + 4) bytes = 48 KiB is what bounds the frames.  A predecessor is read only
// where it exists, and it exists only where its diagonal wrote it: no LDS word is read that this launch has not written.
// DTW_NT = 512 and DTW_Q = 4 are the measured choice among 256 / 512 / 1024 threads and 4 / 8 / 16 diagonals
// (profiles/dtw_bench_and_kernel_times.txt).
//
// The direction bytes are laid out by diagonal, not by row: cell (i, j) sits at ((i + j) % Tb) * Ta + i (for a fixed i the Tb
// columns take the Tb residues once each: Ta * Tb bytes, every cell its own), so the lanes of a diagonal store consecutive bytes.
// The walk back is one lane's chain of dependent byte loads; it writes path[steps - 1] .. path[0], clamps at row 0 and column 0
// whatever the byte says and takes at most Ta + Tb - 1 entries.
//
// Memory safety does not depend on the CONTENTS of the features or of the offset tables: a pair is taken only when its rows lie in
// [0, total_a) / [0, total_b), 1 <= Ta <= min(DTW_MAX_T, R * DTW_NT), 1 <= Tb <= DTW_MAX_T and (with a path) its workspace and path ranges lie inside their totals and
// hold Ta * Tb bytes and Ta + Tb - 1 entries; anything else is left untouched.  A NaN feature makes every comparison false (the
// first existing predecessor stays chosen): no loop bound depends on a feature.  No atomics, nothing crosses workgroups.
#include "common.h"
#include "dtw_walk.h"
#include <math.h>

namespace {

constexpr int DTW_NT = 512;              // threads per workgroup (utils/mel_distance.py DTW_NT)
constexpr int DTW_Q = 4;                 // diagonals whose local costs a lane computes at a time
constexpr int DTW_MAX_T = 2048;          // frames per sequence (satt_dtw_max_frames)
constexpr int DTW_MAX_K = 128;
static_assert(4 * DTW_NT == DTW_MAX_T, "dtw_k<4> covers the longest sequence");

struct DtwArgs {
  int n_pairs, K;
  long long total_a, total_b, total_dirs, total_path;
  const float* a; const float* b;
  const int64_t* a_offsets; const int64_t* b_offsets;
  float* cost; int32_t* steps;
  uint8_t* dirs; const int64_t* dir_offsets;
  int32_t* path; const int64_t* path_offsets;
};

template <int R>                        // rows a lane owns: tid, tid + DTW_NT, .. (the host picks the smallest that covers max_ta)
__global__ __launch_bounds__(DTW_NT) void dtw_k(DtwArgs p) {
  __shared__ float Ds[3][DTW_MAX_T];
  __shared__ int Ls[3][DTW_MAX_T];
  const int tid = threadIdx.x, u = blockIdx.x;
  const int K = p.K;

  // every value that steers the control flow below is the same in all lanes (block index, kernel arguments, the offset tables)
  const long long a0 = p.a_offsets[u], a1 = p.a_offsets[u + 1], b0 = p.b_offsets[u], b1 = p.b_offsets[u + 1];
  bool ok = a0 >= 0 && a1 > a0 && a1 <= p.total_a && a1 - a0 <= R * DTW_NT && a1 - a0 <= DTW_MAX_T &&
            b0 >= 0 && b1 > b0 && b1 <= p.total_b && b1 - b0 <= DTW_MAX_T;
  const int Ta = ok ? (int)(a1 - a0) : 1, Tb = ok ? (int)(b1 - b0) : 1;
  const bool want_path = p.dirs != nullptr;
  long long d0 = 0, q0 = 0;
  if (ok && want_path) {
    d0 = p.dir_offsets[u];
    q0 = p.path_offsets[u];
    const long long d1 = p.dir_offsets[u + 1], q1 = p.path_offsets[u + 1];
    ok = d0 >= 0 && d1 >= d0 && d1 <= p.total_dirs && d1 - d0 >= (long long)Ta * Tb &&
         q0 >= 0 && q1 >= q0 && q1 <= p.total_path && q1 - q0 >= (long long)Ta + Tb - 1;
  }
  if (!ok) return;

  const float* A = p.a + (size_t)a0 * K;
  const float* B = p.b + (size_t)b0 * K;
  uint8_t* dirs = want_path ? p.dirs + d0 : nullptr;
  const int nd = Ta + Tb - 1;
  int cur = 0, dm = 0;                                            // d % 3, d % Tb
  float cq[R][DTW_Q];                                             // c(i, db - i + q) of this lane's rows, q = 0 .. DTW_Q - 1
  for (int db = 0; db < nd; db += DTW_Q) {
    // the local costs of the next DTW_Q diagonals, all loads in flight together: one memory latency per DTW_Q barriers.  Row i meets
    // column db - i + q on diagonal db + q; a column outside [0, Tb) is clamped into it - a valid load whose cost no cell uses.
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = tid + r * DTW_NT, jb = db - i;
      if (i < Ta && jb + DTW_Q > 0 && jb < Tb) {
        const float* ar = A + (size_t)i * K;
        const float* br[DTW_Q];
        float acc[DTW_Q];
#pragma unroll
        for (int q = 0; q < DTW_Q; ++q) {
          const int j = jb + q < 0 ? 0 : (jb + q < Tb ? jb + q : Tb - 1);
          br[q] = B + (size_t)j * K;
          acc[q] = 0.f;
        }
#pragma unroll 4
        for (int k = 0; k < K; ++k) {
#pragma clang fp contract(off)                                                 // difference, product and sum each rounded
          const float av = ar[k];
#pragma unroll
          for (int q = 0; q < DTW_Q; ++q) {
            const float df = av - br[q][k];
            acc[q] = acc[q] + df * df;
          }
        }
#pragma unroll
        for (int q = 0; q < DTW_Q; ++q) cq[r][q] = sqrtf(acc[q]);   // correctly rounded: no fast-math flags
      }
    }
#pragma unroll
    for (int q = 0; q < DTW_Q; ++q) {
      const int d = db + q;
      if (d < nd) {
        const int lo = d - (Tb - 1) > 0 ? d - (Tb - 1) : 0, hi = d < Ta - 1 ? d : Ta - 1;
        const int p1 = cur == 0 ? 2 : cur - 1, p2 = cur == 2 ? 0 : cur + 1;     // (d - 1) % 3, (d - 2) % 3
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int i = tid + r * DTW_NT;
          if (i >= lo && i <= hi) {
            const int j = d - i;
            float best = 0.f;                   // (0, 0): 0 + c == c exactly
            int len = 0, dir = 0;
            if (i > 0 && j > 0) {
              best = Ds[p2][i - 1]; len = Ls[p2][i - 1];
              const float up = Ds[p1][i - 1];
              if (up < best) { best = up; len = Ls[p1][i - 1]; dir = 1; }
              const float left = Ds[p1][i];
              if (left < best) { best = left; len = Ls[p1][i]; dir = 2; }
            } else if (i > 0) {
              best = Ds[p1][i - 1]; len = Ls[p1][i - 1]; dir = 1;
            } else if (j > 0) {
              best = Ds[p1][i]; len = Ls[p1][i]; dir = 2;
            }
            Ds[cur][i] = best + cq[r][q];
            Ls[cur][i] = len + 1;
            if (want_path) dirs[(size_t)dm * Ta + i] = (uint8_t)dir;
          }
        }
        __syncthreads();                        // diagonal d is whole; its stores to dirs are visible to the workgroup
        if (d + 1 < nd) {
          cur = cur == 2 ? 0 : cur + 1;
          dm = dm + 1 == Tb ? 0 : dm + 1;
        }
      }
    }
  }

  if (tid != 0) return;
  const int n = Ls[cur][Ta - 1];
  p.cost[u] = Ds[cur][Ta - 1];
  p.steps[u] = n;
  if (!want_path) return;
  dtw_walk_back(dirs, Ta, Tb, n, p.path + 2 * q0);
}

inline bool dtw_supported(int Ta, int Tb, int K) {
  return Ta >= 1 && Ta <= DTW_MAX_T && Tb >= 1 && Tb <= DTW_MAX_T && K >= 1 && K <= DTW_MAX_K;
}

}  // namespace

extern "C" int satt_dtw_supported(int Ta, int Tb, int K) { return dtw_supported(Ta, Tb, K) ? 1 : 0; }

extern "C" int satt_dtw_max_frames(void) { return DTW_MAX_T; }

extern "C" int satt_dtw(const satt_dtw_params* p, void* stream) {
  if (!p || !p->a || !p->b || !p->a_offsets || !p->b_offsets || !p->cost || !p->steps) return SATT_E_BADARG;
  if (p->n_pairs < 1 || p->total_a < 1 || p->total_b < 1) return SATT_E_BADARG;
  const bool want_path = p->dirs || p->path || p->dir_offsets || p->path_offsets;
  if (want_path) {                                                // the path needs all four pointers and room in both buffers
    if (!p->dirs || !p->path || !p->dir_offsets || !p->path_offsets) return SATT_E_BADARG;
    if (p->total_dirs < 1 || p->total_path < 1) return SATT_E_BADARG;
  }
  if (!dtw_supported(p->max_ta, p->max_tb, p->K)) return SATT_E_UNSUPPORTED;
  if (p->max_ta > p->total_a || p->max_tb > p->total_b) return SATT_E_BADARG;
  DtwArgs a{p->n_pairs, p->K, (long long)p->total_a, (long long)p->total_b, want_path ? (long long)p->total_dirs : 0,
            want_path ? (long long)p->total_path : 0, p->a, p->b, p->a_offsets, p->b_offsets, p->cost, p->steps,
            p->dirs, p->dir_offsets, p->path, p->path_offsets};
  const dim3 grid((unsigned)p->n_pairs), block(DTW_NT);
  const int rows = (p->max_ta + DTW_NT - 1) / DTW_NT;               // rows per lane; a pair longer than max_ta says is left untouched
  if (rows <= 1) hipLaunchKernelGGL(dtw_k<1>, grid, block, 0, (hipStream_t)stream, a);
  else if (rows <= 2) hipLaunchKernelGGL(dtw_k<2>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(dtw_k<4>, grid, block, 0, (hipStream_t)stream, a);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}
