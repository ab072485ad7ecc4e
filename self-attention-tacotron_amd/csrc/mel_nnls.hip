// Non-negative inversion of the mel basis for a batch of frames in ONE launch (DESIGN.md 3.6 holds the definition): K iterations of
// accelerated projected gradient on  min_{x >= 0} |W x - a|^2 / 2  from the floored pseudo-inverse x_0.  W is the banded float32
// mel basis of utils/audio.py MelspecTables (band m covers bins band_start[m] .. + n_m - 1 with weights band_weight[band_offset[m]
// ..]), the operator csrc/melspec.hip applies; W^T comes from the transposed table of utils/audio.py MelNnlsTables (bin f lies under
// bands bin_first[f] .. + c_f - 1 with weights bin_weight[bin_offset[f] ..], c_f = bin_offset[f + 1] - bin_offset[f]; a band of
// that range that does not cover the bin has weight 0).  One frame, a float32 [M], x_0 float32 [F]:
//   y_1 = x_0
//   for k = 1 .. K:
//     p[m]  = sum over the band's bins of w * y_k                 the order below
//     r[m]  = p[m] - a[m]
//     g[f]  = sum over the bin's bands of w^T * r                 one chain from +0, bands ascending; no band: g = 0
//     v     = y_k - step * g
//     x_k   = v > 0 ? v : 0                                       (a NaN becomes 0)
//     y_k+1 = x_k + beta_k * (x_k - x_k-1)
//   result: x_K
// Every product, difference and sum is rounded to float32 on its own (no fused multiply-add).  step and the table beta[K] come
// from the host (step = float32(1 / L) not above 1 / L, L the largest eigenvalue of W W^T; beta_k = (t_k - 1) / t_k+1 of FISTA;
// neither depends on the data).
// THE ORDER OF p[m]: lane j = 0 .. 15 of a team of 16 sums the band's terms i = j, j + 16, j + 32, .. ascending in one chain from
// +0 (s_j = s_j + w_i * y_i), and the sixteen partial sums are joined by the adjacent pairwise tree
//   ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7))  +  ((s8 + s9) + (s10 + s11)) + ((s12 + s13) + (s14 + s15)).
// These are the operations of utils/audio.py mel_nnls_numpy in its order, so the two agree bit for bit.
//
// One workgroup of 256 threads takes one frame.  Thread t owns the bins t, t + 256, .. (NB = ceil(F / 256) of them, compile time):
// x_k, y_k and the bin's entry of the transposed table stay in its registers.  y, r, a, the bands' (start, offset, length)
// and - where they fit - both weight tables are staged in LDS; every word read there was written by this kernel first.  A team is a
// DPP row of 16 lanes, the tree four DPP adds; team q takes the bands q, q + 16, ..  An iteration has two barriers: behind r and
// behind y.  Tables too large for 64 KiB of LDS (a dense basis) are read from global memory by the same code (LDSW = false).
//
// Memory safety does not depend on the CONTENTS of the tables or of the data: a band whose (start, offset, length) does not lie
// inside num_bins / n_weights is taken as empty, and so is a bin whose (first, offset, count) does not lie inside num_mels /
// n_tweights.  No loop bound and no address depends on a sample: a NaN makes the comparison false, nothing more.  No atomics,
// nothing crosses workgroups: two launches are bit-identical and a frame's result does not depend on its batch.
#include "common.h"
#include <math.h>

namespace {

constexpr int NNLS_NT = 256;              // threads per workgroup: 4 waves of 64, 16 teams of 16
constexpr int NNLS_TEAM = 16;
constexpr int NNLS_TEAMS = NNLS_NT / NNLS_TEAM;
constexpr int NNLS_MAX_BINS = 2049;       // n_fft = 4096
constexpr int NNLS_MAX_MELS = 128;
constexpr int NNLS_MAX_ITERS = 1024;
constexpr size_t NNLS_LDS_BYTES = 64 * 1024;

struct NnlsArgs {
  int F, M, K, n_w, n_tw;
  float step;
  const float* amp; const float* x0; const float* beta;
  const int* band_start; const int* band_offset; const float* band_weight;
  const int* bin_first; const int* bin_offset; const float* bin_weight;
  float* out;
};

__host__ __device__ inline int nnls_pad4(int n) { return (n + 3) & ~3; }

// the fixed part of LDS in floats: y [F], r [M], a [M], the bands' start / offset / length [M] each (all padded to 16 bytes)
inline size_t nnls_fixed_floats(int F, int M) { return (size_t)nnls_pad4(F) + 5 * (size_t)nnls_pad4(M); }

// NB: bins a thread owns.  LDSW: both weight tables are staged in LDS (else they are read from global memory)
template <int NB, bool LDSW>
__global__ __launch_bounds__(NNLS_NT) void mel_nnls_k(NnlsArgs a) {
#pragma clang fp contract(off)            // every product, difference and sum below is rounded on its own: NumPy's float32 bits
  extern __shared__ __attribute__((aligned(16))) float nnls_smem[];
  const int F = a.F, M = a.M, Mp = nnls_pad4(a.M);
  float* ys = nnls_smem;
  float* rs = ys + nnls_pad4(F);
  float* as = rs + Mp;
  int* bst = reinterpret_cast<int*>(as + Mp);
  int* bof = bst + Mp;
  int* bln = bof + Mp;
  float* wl = reinterpret_cast<float*>(bln + Mp);          // [n_w], then [n_tw]: only with LDSW
  float* twl = wl + nnls_pad4(a.n_w);
  const int tid = threadIdx.x, team = tid >> 4, j = tid & (NNLS_TEAM - 1);
  const size_t frame = blockIdx.x;
  const float* amp = a.amp + frame * (size_t)M;
  const float* x0 = a.x0 + frame * (size_t)F;
  float* out = a.out + frame * (size_t)F;

  // ---- staging: the frame's amplitudes, the validated bands, the weights; the thread's bins and their table entries
  for (int m = tid; m < M; m += NNLS_NT) {
    as[m] = amp[m];
    rs[m] = 0.f;
    const int s = a.band_start[m], o = a.band_offset[m], e = a.band_offset[m + 1];
    const bool ok = s >= 0 && o >= 0 && e >= o && e <= a.n_w && e - o <= F && s <= F - (e - o);
    bst[m] = ok ? s : 0;
    bof[m] = ok ? o : 0;
    bln[m] = ok ? e - o : 0;
  }
  if constexpr (LDSW) {
    for (int i = tid; i < a.n_w; i += NNLS_NT) wl[i] = a.band_weight[i];
    for (int i = tid; i < a.n_tw; i += NNLS_NT) twl[i] = a.bin_weight[i];
  }
  const float* w = LDSW ? wl : a.band_weight;
  const float* tw = LDSW ? twl : a.bin_weight;
  float x[NB], y[NB];
  int tfirst[NB], toff[NB], tcnt[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int f = tid + NNLS_NT * i;
    x[i] = y[i] = 0.f;
    tfirst[i] = toff[i] = tcnt[i] = 0;
    if (f < F) {
      x[i] = y[i] = x0[f];
      ys[f] = y[i];
      const int b = a.bin_first[f], o = a.bin_offset[f], e = a.bin_offset[f + 1];
      if (b >= 0 && o >= 0 && e >= o && e <= a.n_tw && e - o <= M && b <= M - (e - o)) {
        tfirst[i] = b; toff[i] = o; tcnt[i] = e - o;
      }
    }
  }
  __syncthreads();

  for (int k = 0; k < a.K; ++k) {
    const float beta = a.beta[k];
    // ---- r = W y - a: team q takes the bands q, q + 16, ..; every team walks the same number of rounds (the DPP adds below are
    // executed by whole waves)
    for (int mb = 0; mb < M; mb += NNLS_TEAMS) {
      const int m = mb + team;
      const bool live = m < M;
      const int n = live ? bln[m] : 0, s = live ? bst[m] : 0, o = live ? bof[m] : 0;
      float acc = 0.f;
      for (int i = j; i < n; i += NNLS_TEAM) acc = acc + w[o + i] * ys[s + i];          // o + i < n_w, s + i < F: validated above
      SATT_DPP_ADD(acc, 0xB1);      // s0 + s1 (quad_perm [1,0,3,2])
      SATT_DPP_ADD(acc, 0x4E);      // (s0 + s1) + (s2 + s3) (quad_perm [2,3,0,1])
      SATT_DPP_ADD(acc, 0x141);     // + the neighbouring quad (row_half_mirror)
      SATT_DPP_ADD(acc, 0x140);     // + the other half of the row (row_mirror)
      if (live && j == 0) rs[m] = acc - as[m];
    }
    __syncthreads();
    // ---- g = W^T r, the step, the projection and the momentum, each thread on its own bins
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int f = tid + NNLS_NT * i;
      if (f < F) {
        float g = 0.f;
        for (int c = 0; c < tcnt[i]; ++c) g = g + tw[toff[i] + c] * rs[tfirst[i] + c];   // < n_tw, < M: validated above
        const float v = y[i] - a.step * g;
        const float xn = v > 0.f ? v : 0.f;
        y[i] = xn + beta * (xn - x[i]);                                                 // x[i] is still x_k-1 here
        x[i] = xn;
        ys[f] = y[i];
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int f = tid + NNLS_NT * i;
    if (f < F) out[f] = x[i];
  }
}

inline bool nnls_supported(int num_bins, int num_mels, int iters) {
  return num_bins >= 1 && num_bins <= NNLS_MAX_BINS && num_mels >= 1 && num_mels <= NNLS_MAX_MELS && iters >= 1 && iters <= NNLS_MAX_ITERS;
}

template <int NB>
void nnls_launch(const NnlsArgs& a, unsigned blocks, bool ldsw, size_t lds, hipStream_t st) {
  const dim3 grid(blocks), block(NNLS_NT);
  if (ldsw) hipLaunchKernelGGL((mel_nnls_k<NB, true>), grid, block, lds, st, a);
  else hipLaunchKernelGGL((mel_nnls_k<NB, false>), grid, block, lds, st, a);
}

}  // namespace

extern "C" int satt_mel_nnls_supported(int num_bins, int num_mels, int iters) { return nnls_supported(num_bins, num_mels, iters) ? 1 : 0; }

extern "C" int satt_mel_nnls(const satt_mel_nnls_params* p, void* stream) {
  if (!p || !p->amp || !p->start || !p->beta || !p->band_start || !p->band_offset || !p->band_weight || !p->bin_first ||
      !p->bin_offset || !p->bin_weight || !p->out)
    return SATT_E_BADARG;
  if (!nnls_supported(p->num_bins, p->num_mels, p->iters)) return SATT_E_UNSUPPORTED;
  if (p->n_frames < 1 || p->n_frames > 0x7fffffffLL) return SATT_E_UNSUPPORTED;
  if (p->n_weights < 1 || p->n_tweights < 1) return SATT_E_BADARG;
  if (!(p->step > 0.f) || !(p->step <= 3.0e38f)) return SATT_E_BADARG;
  NnlsArgs a{p->num_bins, p->num_mels, p->iters, p->n_weights, p->n_tweights, p->step, p->amp, p->start, p->beta,
             p->band_start, p->band_offset, p->band_weight, p->bin_first, p->bin_offset, p->bin_weight, p->out};
  const size_t fixed = nnls_fixed_floats(a.F, a.M) * sizeof(float);                   // <= (2052 + 5 * 128) 4 = 10 768 bytes
  const size_t full = fixed + ((size_t)nnls_pad4(a.n_w) + (size_t)nnls_pad4(a.n_tw)) * sizeof(float);
  const bool ldsw = full <= NNLS_LDS_BYTES;
  const size_t lds = ldsw ? full : fixed;
  const unsigned blocks = (unsigned)p->n_frames;
  hipStream_t st = (hipStream_t)stream;
  switch ((a.F + NNLS_NT - 1) / NNLS_NT) {                                           // 1 .. 9: num_bins <= 2049
    case 1: nnls_launch<1>(a, blocks, ldsw, lds, st); break;
    case 2: nnls_launch<2>(a, blocks, ldsw, lds, st); break;
    case 3: nnls_launch<3>(a, blocks, ldsw, lds, st); break;
    case 4: nnls_launch<4>(a, blocks, ldsw, lds, st); break;
    case 5: nnls_launch<5>(a, blocks, ldsw, lds, st); break;
    case 6: nnls_launch<6>(a, blocks, ldsw, lds, st); break;
    case 7: nnls_launch<7>(a, blocks, ldsw, lds, st); break;
    case 8: nnls_launch<8>(a, blocks, ldsw, lds, st); break;
    default: nnls_launch<9>(a, blocks, ldsw, lds, st); break;
  }
  SATT_LAUNCH_CHECK(); return SATT_OK;
}
