// Per-utterance stop of a free-running batch: behind a decode launch that evaluated no stop rule, find for every sample the first
// step of the launch's window at which ITS stop probability exceeds the threshold.  satt_dec_stop_scan
// (decode_mega2.hip) is the reference's batch rule - all samples above the threshold at the same step; this one lets every
// utterance end on its own, and the batch is done when the last one has.
//
// One workgroup of 256 threads = 4 waves.  Wave w takes samples w, w + 4, ... (any B >= 1); its lanes take steps t0 + lane,
// t0 + lane + 64, ... of the window, a lane keeps the first step of its own that qualifies, and a wave-wide integer minimum (the
// DPP butterfly of common.h's wave_max + four v_readlane) gives the sample's first.  Every branch around the butterfly is
// wave-uniform (b, ends[b] and the loop bounds are the same in all 64 lanes), so it always runs with all lanes active.  ends[b] is
// written by lane 0 of the one wave that owns sample b with a plain store; the waves' maxima and "still open" bits meet in LDS and
// thread 0 writes the flag.  No atomics anywhere: the integers do not depend on timing.
//
// The comparison is literally dec_stop_scan_k's and the step loop's, 1.f / (1.f + __expf(-logit)) > stop_threshold.
//
// Loads: row t + 1 of sample b, t + 1 <= t0 + nsteps < rows (checked by the entry point), b < B.  Stores: ends[b], b < B, and *flag.
#include "common.h"

namespace {

constexpr int DE_NONE = 0x7fffffff;

#define SATT_DPP_IMIN(v, ctrl) (v) = min((v), __builtin_amdgcn_update_dpp((v), (v), (ctrl), 0xF, 0xF, false))
__device__ __forceinline__ int wave_imin(int v) {          // all 64 lanes active
  SATT_DPP_IMIN(v, 0xB1); SATT_DPP_IMIN(v, 0x4E); SATT_DPP_IMIN(v, 0x141); SATT_DPP_IMIN(v, 0x140);
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

__global__ __launch_bounds__(256) void dec_ends_scan_k(const float* __restrict__ yout, int B, int rows, int NO, int t0, int nsteps, int min_steps,
                                                       float stop_threshold, int* __restrict__ ends, int* flag) {
  __shared__ int w_last[4], w_open[4];
  if (*flag != 0) return;                            // (the batch ended behind an earlier launch: every thread reads the same word)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int last = 0, open = 0;                            // of this wave's samples: the latest end, and whether one has none yet
  for (int b = wave; b < B; b += 4) {
    int e = __builtin_amdgcn_readfirstlane(ends[b]);
    if (e == 0) {
      const float* col = yout + ((int64_t)b * rows + t0 + 1) * NO + NO - 1;
      int first = DE_NONE;
      for (int s = lane; s < nsteps && first == DE_NONE; s += 64) {
        const int t = t0 + s;
        if (t > min_steps && 1.f / (1.f + __expf(-col[(int64_t)s * NO])) > stop_threshold) first = t;
      }
      first = wave_imin(first);
      if (first != DE_NONE) {
        e = first + 1;
        if (lane == 0) ends[b] = e;
      }
    }
    last = max(last, e);
    open |= e == 0;
  }
  if (lane == 0) { w_last[wave] = last; w_open[wave] = open; }
  __syncthreads();
  if (threadIdx.x == 0 && !(w_open[0] | w_open[1] | w_open[2] | w_open[3]))
    *flag = max(max(w_last[0], w_last[1]), max(w_last[2], w_last[3]));
}

}  // namespace

extern "C" int satt_dec_ends_scan(const float* yout, int B, int rows, int NO, int t0, int nsteps, int min_steps, float stop_threshold,
                                  int* ends, int* flag, void* stream) {
  if (!yout || !flag || !ends) return SATT_E_BADARG;
  if (B < 1 || NO < 1 || t0 < 0 || nsteps < 1 || (int64_t)t0 + nsteps >= rows) return SATT_E_BADARG;
  hipLaunchKernelGGL(dec_ends_scan_k, dim3(1), dim3(256), 0, (hipStream_t)stream, yout, B, rows, NO, t0, nsteps, min_steps, stop_threshold, ends, flag);
  SATT_LAUNCH_CHECK();
  return SATT_OK;
}
