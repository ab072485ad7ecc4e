// Sample-rate conversion of a batch of utterances in ONE launch: a Kaiser-windowed sinc evaluated on the rational grid up / down
// (DESIGN.md 3.6 holds the definition).  For an utterance of n samples, n_out = ceil(n up / down) and output m sits at input time
// m down / up:
//   k0 = (m down) / up,  phase = (m down) % up                                   (64-bit products)
//   y[m] = sum_{jj = 0 .. taps - 1} table[phase][jj] * x[k0 - half + 1 + jj]       half = taps / 2,  x = 0 outside [0, n)
// The table [up][taps] is the caller's (float64 on the host, rounded once); the sum runs in fp32, taps ascending, one chain per
// output, acc = acc + w * x with the product and the sum each rounded to fp32 (no fused multiply-add: these are the operations
// the NumPy backend of utils/audio.py performs, so the two backends agree bit for bit).  No atomics, nothing crosses lanes or
// workgroups, so two launches are bit-identical and an utterance's result does not depend on its batch or on where the workgroup
// seams fall.
//
// A workgroup takes RS_RUN consecutive outputs of the batch (outputs are numbered through the utterances; the utterance of an
// output is found by bisection of out_offsets, as stft_lds.h does for frames) and walks the utterances its run touches.  Per
// utterance it goes in chunks of `sub` outputs whose input span - (sub - 1) down / up + 1 + taps samples at most - fits RS_SPAN
// floats of LDS: the span is staged once (zeros outside the utterance), then one lane per output walks its own table row.  At
// the common ratios a whole run is one chunk (22050 -> 16000: 512 outputs read 893 samples; 48000 -> 8000: 3879).
//
// LDS banks (ds_read_b32, 32 lanes a group): lanes of a group read xs[k0(m) + jj] with k0 advancing by down / up per lane.
// Below 1 (upsampling) neighbouring lanes share words (broadcast); an odd integer step (48000 -> 16000: 3) is conflict-free; an
// even step s pays gcd(s, 32)-way conflicts (48000 -> 24000: 2-way).  The table rows are read from global memory through the
// caches, two taps a load: with up == 1 every lane reads the same row, otherwise a lane walks a row of its own.
//
// Memory safety does not depend on the CONTENTS of the offset tables: an utterance is taken only when its sample range lies in
// [0, total_in), its output range in [0, total_out) and the two lengths agree; anything else is left untouched.  Stores go to
// indices inside the workgroup's own run, loads to indices inside the utterance's checked sample range.
#include "common.h"

namespace {

constexpr int RS_NT = 256;              // threads per workgroup
constexpr int RS_RUN = 512;             // outputs per workgroup (satt_resample_run_length)
constexpr int RS_SPAN = 8192;           // floats of staged input (32 KiB)
constexpr int RS_MAX_UP = 1024, RS_MAX_DOWN = 4096, RS_MAX_TAPS = 4096;
constexpr long long RS_MAX_N = 1LL << 52;   // n * up stays inside 64 bits

struct RsArgs {
  int up, down, taps, n_utts, sub;
  long long total_in, total_out;
  const float* x; const int64_t* in_offsets; const int64_t* out_offsets;
  const float* table;
  float* y;
};

// the last utterance whose first output is <= g
__device__ __forceinline__ int rs_utt(const int64_t* out_offsets, int n_utts, long long g) {
  int lo = 0, hi = n_utts;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (out_offsets[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(RS_NT) void resample_k(RsArgs a) {
  __shared__ float xs[RS_SPAN];
  const int tid = threadIdx.x;
  const int half = a.taps >> 1;
  const long long up = a.up, down = a.down;
  long long g = (long long)blockIdx.x * RS_RUN;
  long long g1 = g + RS_RUN;
  if (g1 > a.total_out) g1 = a.total_out;

  // every value that steers this loop is the same in all lanes (block index, kernel arguments, the offset tables)
  while (g < g1) {
    const int u = rs_utt(a.out_offsets, a.n_utts, g);
    const long long o0 = a.out_offsets[u], o1 = a.out_offsets[u + 1], i0 = a.in_offsets[u], i1 = a.in_offsets[u + 1];
    const long long n = i1 - i0;
    bool ok = o0 >= 0 && o0 <= g && o1 > g && o1 <= a.total_out && i0 >= 0 && i1 > i0 && i1 <= a.total_in && n <= RS_MAX_N;
    if (ok) ok = (n * up + down - 1) / down == o1 - o0;
    const long long end = (o1 > g && o1 < g1) ? o1 : g1;      // the next utterance's first output, or the end of the run
    if (ok) {
      const float* x = a.x + i0;
      float* y = a.y + o0;
      const long long mb = end - o0;
      for (long long c0 = g - o0; c0 < mb; c0 += a.sub) {
        const long long c1 = c0 + a.sub < mb ? c0 + a.sub : mb;
        const long long klo = (c0 * down) / up - half + 1;                    // first and last sample the chunk reads
        const long long khi = ((c1 - 1) * down) / up + half;
        const int cnt = khi - klo + 1 < RS_SPAN ? (int)(khi - klo + 1) : RS_SPAN;   // (<= RS_SPAN by the choice of sub)
        __syncthreads();                                                      // the chunk before has been read
        for (int e = tid; e < cnt; e += RS_NT) {
          const long long k = klo + e;
          xs[e] = (k >= 0 && k < n) ? x[k] : 0.f;
        }
        __syncthreads();
        for (long long m = c0 + tid; m < c1; m += RS_NT) {
          const long long t = m * down, k0 = t / up;
          const int phase = (int)(t - k0 * up);
          const float* row = a.table + (size_t)phase * a.taps;
          const float* xw = xs + (int)(k0 - half + 1 - klo);                  // taps words, inside [0, cnt)
          float acc = 0.f;
#pragma unroll 8                                                               // eight row loads in flight; the chain stays ascending
          for (int jj = 0; jj < a.taps; jj += 2) {
#pragma clang fp contract(off)                                                 // product and sum each rounded: NumPy's float32 bits
            const float2 w = *reinterpret_cast<const float2*>(row + jj);
            acc = acc + w.x * xw[jj];
            acc = acc + w.y * xw[jj + 1];
          }
          y[m] = acc;
        }
      }
    }
    g = end;
  }
}

inline long long rs_gcd(long long a, long long b) {
  while (b) { const long long t = a % b; a = b; b = t; }
  return a;
}

inline bool rs_supported(int up, int down, int taps) {
  if (up < 1 || up > RS_MAX_UP || down < 1 || down > RS_MAX_DOWN) return false;
  if (up == 1 && down == 1) return false;
  if (rs_gcd(up, down) != 1) return false;
  return taps >= 2 && taps <= RS_MAX_TAPS && (taps & 1) == 0;
}

}  // namespace

extern "C" int satt_resample_supported(int up, int down, int taps) { return rs_supported(up, down, taps) ? 1 : 0; }

extern "C" int satt_resample_run_length(void) { return RS_RUN; }

extern "C" int satt_resample(const satt_resample_params* p, void* stream) {
  if (!p || !p->signal_in || !p->in_offsets || !p->out_offsets || !p->table || !p->signal_out) return SATT_E_BADARG;
  if (p->n_utts < 1 || p->total_in < 1 || p->total_out < 1) return SATT_E_BADARG;
  if (reinterpret_cast<uintptr_t>(p->table) & 7) return SATT_E_BADARG;            // rows are read two taps a load
  if (!rs_supported(p->up, p->down, p->taps)) return SATT_E_UNSUPPORTED;
  const long long blocks = ((long long)p->total_out + RS_RUN - 1) / RS_RUN;
  if (blocks > 0x7fffffffLL) return SATT_E_UNSUPPORTED;
  // the longest chunk whose span (sub - 1) down / up + 1 + taps fits RS_SPAN: >= 1 because taps <= 4096 and down <= 4096
  long long sub = 1 + (long long)(RS_SPAN - 1 - p->taps) * p->up / p->down;
  if (sub > RS_RUN) sub = RS_RUN;
  RsArgs a{p->up, p->down, p->taps, p->n_utts, (int)sub, (long long)p->total_in, (long long)p->total_out,
           p->signal_in, p->in_offsets, p->out_offsets, p->table, p->signal_out};
  hipLaunchKernelGGL(resample_k, dim3((unsigned)blocks), dim3(RS_NT), 0, (hipStream_t)stream, a);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}
