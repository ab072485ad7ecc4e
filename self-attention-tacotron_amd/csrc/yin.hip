// YIN pitch tracking (de Cheveigne & Kawahara 2002) of a batch of utterances on the mel frame grid in ONE launch (DESIGN.md 3.6
// holds the definition).  An utterance of n samples has T = 1 + n / hop frames; for frame t, s = t hop - (W + tau_max) / 2 and
// x = 0 outside [0, n):
//   d(tau)  = sum_{j = 0 .. W - 1} (x[s + j] - x[s + j + tau])^2     tau = 0 .. tau_max; fp32, j ascending in one chain, the
//                                                                   difference, the product and the sum each rounded (no FMA)
//   power   = (sum_j x[s + j]^2) / W                                 the same way, the division correctly rounded
//   c(tau)  = c(tau - 1) + d(tau), c(0) = 0                          one ascending chain
//   d'(0)   = 1;  d'(tau) = (d(tau) * tau) / c(tau) if c(tau) > 0, else 1      product rounded, division correctly rounded
//   tau0    = the smallest tau in [tau_min, tau_max - 1] with d'(tau) < threshold.  None: f0 = 0 and aperiodicity = the minimum of
//             d' over [tau_min, tau_max] (fminf: a NaN entry is passed over; +inf when every entry is NaN).  Otherwise tau* walks up
//             from tau0 while tau* + 1 <= tau_max - 1 and d'(tau* + 1) < d'(tau*); aperiodicity = d'(tau*) and, with
//             a = d'(tau* - 1), b = d'(tau*), c = d'(tau* + 1):
//               num = a - c;  den = (a - b) + (c - b);  off = den > 0 ? (0.5 num) / den : 0, then 1 if off > 1, -1 if off < -1
//               f0 = sample_rate / ((float)tau* + off)
// These are the operations of utils/pitch.py yin_numpy in its order, so the two agree bit for bit.
//
// satt_yin_candidates is the same kernel with another pick (yin_k<NCH, true>), for the Viterbi tracker of csrc/f0_viterbi.hip: lag k
// in [tau_min, tau_max - 1] is a dip when d'(k) < d'(k - 1) and d'(k) <= d'(k + 1); the YIN_K = 8 dips with the smallest d' (ties to
// the smaller lag) are stored in ascending lag order as period = (float)k + off (the parabola above) and value = d'(k), unused slots
// as period 0 and value +inf: the operations of utils/pitch.py yin_candidates_numpy.
//
// A workgroup of 4 waves takes YIN_RUN = 16 consecutive frames of the batch (frames are numbered through the utterances; the
// utterance of a frame is found by bisection of frame_offsets), a wave one frame at a time.  The wave stages the frame's span
// xs[e] = x[s + e] in its own LDS region (zeros outside the utterance, and on to the end of the region: every word read below was
// written here), 16-byte aligned at the frame's first sample whatever hop is.  A lane owns the four consecutive lags
// 256 c + 4 lane .. + 3 of each of NCH chunks and keeps their sums in registers.  Four steps of j take one 16-byte read of
// x[s + j ..] - the same address in all lanes, a broadcast - shared by all chunks, and per chunk one 16-byte read of the four
// samples behind the lane's sliding window of eight, lanes side by side and conflict-free: 1 + NCH reads for 48 NCH + 8 VALU
// operations.  d goes to LDS, lane 0 runs the chain c over it in place, every lane turns its own lags into d' (d still in its
// registers), and the pick is wave-uniform: ballots find tau0, the walk reads broadcasts.  Only the chain c is serial.
//
// Memory safety does not depend on the CONTENTS of the signal or of the offset tables: a frame is computed only when its
// utterance's sample range lies in [0, total_in), its frame range in [0, total_frames) and holds 1 + n / hop frames; anything else
// is left untouched.  Stores go to the frame's own index, below total_frames.  No loop bound depends on a sample: a NaN makes
// comparisons false, nothing more.  No atomics, nothing crosses waves, so two launches are bit-identical and a frame's result does
// not depend on its batch or on where the workgroup seams fall.
#include "common.h"
#include <math.h>

namespace {

constexpr int YIN_NT = 256;               // threads per workgroup: 4 waves of 64
constexpr int YIN_WAVES = YIN_NT / 64;
constexpr int YIN_FPW = 4;                // frames a wave takes, one after the other
constexpr int YIN_RUN = YIN_WAVES * YIN_FPW;   // frames per workgroup (satt_yin_run_length)
constexpr int YIN_CHUNK = 256;            // lags per chunk: 64 lanes of 4
constexpr int YIN_MAX_W = 1536;           // satt_yin_max_window
constexpr int YIN_MAX_TAU = 1023;         // satt_yin_max_lag: tau = 0 .. 1023 is 4 chunks
constexpr int YIN_MAX_HOP = 1 << 20;

struct YinArgs {
  int W, tau_min, tau_max, hop, n_utts, span, lags;
  float sr, thr;
  long long total_in, total_frames;
  const float* x; const int64_t* in_offsets; const int64_t* frame_offsets;
  float* f0; float* ap; float* pw;
  float* cper; float* cval;               // the candidates kernel's outputs, [total_frames, YIN_K] each
};

constexpr int YIN_K = SATT_F0_CANDIDATES;

// the parabola through d' at t - 1, t, t + 1 and its clamp: the offset of the minimum from t
__device__ __forceinline__ float yin_offset(float ya, float yb, float yc) {
#pragma clang fp contract(off)
  const float num = ya - yc, den = (ya - yb) + (yc - yb);
  float off = 0.f;
  if (den > 0.f) {
    off = (0.5f * num) / den;
    if (off > 1.f) off = 1.f;
    if (off < -1.f) off = -1.f;
  }
  return off;
}

// the last utterance whose first frame is <= g
__device__ __forceinline__ int yin_utt(const int64_t* frame_offsets, int n_utts, long long g) {
  int lo = 0, hi = n_utts;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (frame_offsets[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// NCH: chunks of 256 lags, the smallest that covers 0 .. tau_max.  CAND: the pick of satt_yin_candidates in place of satt_yin's
template <int NCH, bool CAND>
__global__ __launch_bounds__(YIN_NT) void yin_k(YinArgs a) {
#pragma clang fp contract(off)            // every difference, product and sum below is rounded on its own: NumPy's float32 bits
  extern __shared__ __attribute__((aligned(16))) float yin_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* xs = yin_smem + (size_t)wave * (a.span + a.lags);   // the frame's span, then d / c / d' of its lags
  float* db = xs + a.span;
  const float4* xv = reinterpret_cast<const float4*>(xs);
  const int W = a.W, W4 = a.W & ~3, tmax = a.tau_max;

  // a wave's control flow depends on the block index, the kernel arguments and the offset tables alone; the barriers are reached
  // by all four waves YIN_FPW times whatever their frames are
  for (int it = 0; it < YIN_FPW; ++it) {
    const long long g = (long long)blockIdx.x * YIN_RUN + it * YIN_WAVES + wave;
    bool ok = g < a.total_frames;
    long long i0 = 0, n = 0, s = 0;
    if (ok) {
      const int u = yin_utt(a.frame_offsets, a.n_utts, g);
      const long long o0 = a.frame_offsets[u], o1 = a.frame_offsets[u + 1], i1 = a.in_offsets[u + 1];
      i0 = a.in_offsets[u];
      n = i1 - i0;
      ok = o0 >= 0 && o0 <= g && o1 > g && o1 <= a.total_frames && i0 >= 0 && i1 > i0 && i1 <= a.total_in;
      if (ok) ok = 1 + n / a.hop == o1 - o0;
      s = (g - o0) * a.hop - ((W + tmax) >> 1);
    }
    __syncthreads();                                           // the frame before has been read
    if (ok) {
      const float* x = a.x + i0;
      for (int e = lane; e < a.span; e += 64) {
        const long long k = s + e;
        xs[e] = (k >= 0 && k < n) ? x[k] : 0.f;
      }
    }
    __syncthreads();
    float acc[NCH][4];
    float pw = 0.f;
    if (ok) {
      float4 cur[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        cur[c] = xv[64 * c + lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[c][r] = 0.f;
      }
      for (int j = 0; j < W4; j += 4) {
        const float4 av = xv[j >> 2];
        const float aq[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) pw = pw + aq[q] * aq[q];
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const float4 nx = xv[(j >> 2) + 64 * c + lane + 1];   // words j + 256 c + 4 lane + 4 .. + 7 < W4 + 256 NCH + 4 <= span
          const float v[8] = {cur[c].x, cur[c].y, cur[c].z, cur[c].w, nx.x, nx.y, nx.z, nx.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {                        // j + q ascending in every lag's chain
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float df = aq[q] - v[q + r];
              acc[c][r] = acc[c][r] + df * df;
            }
          }
          cur[c] = nx;
        }
      }
      for (int j = W4; j < W; ++j) {                           // the last W % 4 terms
        const float aj = xs[j];
        pw = pw + aj * aj;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float df = aj - xs[j + YIN_CHUNK * c + 4 * lane + r];      // < W + 256 NCH <= span
            acc[c][r] = acc[c][r] + df * df;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int tau = YIN_CHUNK * c + 4 * lane + r;
          if (tau <= tmax) db[tau] = acc[c][r];
        }
      }
    }
    __syncthreads();
    if (ok && lane == 0) {                                     // c(tau), one ascending chain, in place of d
      float c = 0.f;
      for (int tau = 1; tau <= tmax; ++tau) {
        c = c + db[tau];
        db[tau] = c;
      }
    }
    __syncthreads();
    if (ok) {                                                  // d' in place of c: a lane reads and writes its own lags only
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int tau = YIN_CHUNK * c + 4 * lane + r;
          if (tau <= tmax) {
            const float cc = db[tau];
            float dp = 1.f;
            if (tau > 0 && cc > 0.f) dp = (acc[c][r] * (float)tau) / cc;
            db[tau] = dp;
          }
        }
      }
    }
    __syncthreads();
    if constexpr (CAND) {
      if (ok) {
        // a lane marks the dips among its lags tau_min + lane + 64 i (at most 16 of them: tau_max <= 1023) in a register, then
        // YIN_K rounds take the wave-wide minimum of (d', lag) over the marks that are left and its owner drops the mark.  A dip's
        // d' is below its neighbour's, so it is neither NaN nor +inf: +inf with lag INT_MAX stands for "none"
        unsigned marks = 0;
        for (int i = 0, t = a.tau_min + lane; t < tmax; ++i, t += 64) {          // tau_min >= 2: t - 1 >= 1; t + 1 <= tau_max
          const float v = db[t];
          if (v < db[t - 1] && v <= db[t + 1]) marks |= 1u << i;
        }
        float selv[YIN_K]; int selk[YIN_K];
#pragma unroll
        for (int r = 0; r < YIN_K; ++r) {
          float bv = INFINITY; int bk = 0x7fffffff;
          for (unsigned m = marks; m; m &= m - 1) {                              // ascending lags: a strict < keeps the smaller one
            const int t = a.tau_min + lane + 64 * (__ffs((int)m) - 1);
            const float v = db[t];
            if (v < bv) { bv = v; bk = t; }
          }
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o); const int ol = __shfl_xor(bk, o);
            if (ov < bv || (ov == bv && ol < bk)) { bv = ov; bk = ol; }
          }
          selv[r] = bv; selk[r] = bk;
          if (bk != 0x7fffffff && ((bk - a.tau_min) & 63) == lane) marks &= ~(1u << ((bk - a.tau_min) >> 6));
        }
        // lane c < YIN_K stores the slot c: the kept dip with c kept dips at smaller lags (the lags are distinct)
        if (lane < YIN_K) {
          float v = INFINITY, per = 0.f;
#pragma unroll
          for (int i = 0; i < YIN_K; ++i) {
            int rank = 0;
#pragma unroll
            for (int j = 0; j < YIN_K; ++j) rank += selk[j] < selk[i] ? 1 : 0;
            if (selk[i] != 0x7fffffff && rank == lane) {
              const int t = selk[i];                                             // tau_min <= t <= tau_max - 1 by construction
              v = selv[i];
              per = (float)t + yin_offset(db[t - 1], db[t], db[t + 1]);
            }
          }
          a.cper[g * YIN_K + lane] = per;
          a.cval[g * YIN_K + lane] = v;
        }
        if (lane == 0) a.pw[g] = pw / (float)W;
      }
    } else if (ok) {                                           // the pick: every lane takes the same way through it
      int t0 = -1;
      for (int b = a.tau_min; b < tmax && t0 < 0; b += 64) {
        const int t = b + lane;
        const bool hit = t < tmax && db[t] < a.thr;
        const unsigned long long m = __ballot(hit);
        if (m) t0 = b + __ffsll((long long)m) - 1;
      }
      float f0 = 0.f, ap;
      if (t0 < 0) {
        float m = INFINITY;
        for (int t = a.tau_min + lane; t <= tmax; t += 64) m = fminf(m, db[t]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = fminf(m, __shfl_xor(m, o));
        ap = m;
      } else {
        int t = t0;
        while (t + 1 < tmax && db[t + 1] < db[t]) ++t;         // at most tau_max steps
        const float ya = db[t - 1], yb = db[t], yc = db[t + 1];  // 1 <= t - 1 and t + 1 <= tau_max: tau_min >= 2
        ap = yb;
        f0 = a.sr / ((float)t + yin_offset(ya, yb, yc));
      }
      if (lane == 0) {
        a.f0[g] = f0;
        a.ap[g] = ap;
        a.pw[g] = pw / (float)W;
      }
    }
  }
}

inline bool yin_supported(int W, int tau_max, int hop) {
  return W >= 1 && W <= YIN_MAX_W && tau_max >= 3 && tau_max <= YIN_MAX_TAU && hop >= 1 && hop <= YIN_MAX_HOP;
}

}  // namespace

extern "C" int satt_yin_supported(int window, int tau_max, int hop) { return yin_supported(window, tau_max, hop) ? 1 : 0; }

extern "C" int satt_yin_max_window(void) { return YIN_MAX_W; }

extern "C" int satt_yin_max_lag(void) { return YIN_MAX_TAU; }

extern "C" int satt_yin_run_length(void) { return YIN_RUN; }

// the checks that both entry points share, then the launch: the sizes of the grid and of LDS are the same for both picks
template <bool CAND>
int yin_launch(YinArgs a, void* stream) {
  if (a.n_utts < 1 || a.total_in < 1 || a.total_frames < 1) return SATT_E_BADARG;
  if (!yin_supported(a.W, a.tau_max, a.hop)) return SATT_E_UNSUPPORTED;
  if (a.tau_min < 2 || a.tau_min >= a.tau_max) return SATT_E_BADARG;                // [tau_min, tau_max - 1] holds a lag, tau* - 1 >= 1
  if (!(a.sr > 0.f) || !(a.thr == a.thr)) return SATT_E_BADARG;
  const long long blocks = (a.total_frames + YIN_RUN - 1) / YIN_RUN;
  if (blocks > 0x7fffffffLL) return SATT_E_UNSUPPORTED;
  const int nch = (a.tau_max + YIN_CHUNK) / YIN_CHUNK;                              // covers tau = 0 .. tau_max
  a.lags = nch * YIN_CHUNK;
  a.span = ((a.W + 3) & ~3) + a.lags + 4;                                           // the last 16-byte read ends at W4 + lags + 3
  const size_t lds = (size_t)YIN_WAVES * (a.span + a.lags) * sizeof(float);         // <= 4 (1536 + 1028 + 1024) 4 = 57 408 bytes
  const dim3 grid((unsigned)blocks), block(YIN_NT);
  hipStream_t st = (hipStream_t)stream;
  if (nch == 1) hipLaunchKernelGGL((yin_k<1, CAND>), grid, block, lds, st, a);
  else if (nch == 2) hipLaunchKernelGGL((yin_k<2, CAND>), grid, block, lds, st, a);
  else if (nch == 3) hipLaunchKernelGGL((yin_k<3, CAND>), grid, block, lds, st, a);
  else hipLaunchKernelGGL((yin_k<4, CAND>), grid, block, lds, st, a);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}

extern "C" int satt_yin(const satt_yin_params* p, void* stream) {
  if (!p || !p->signal || !p->in_offsets || !p->frame_offsets || !p->f0 || !p->aperiodicity || !p->power) return SATT_E_BADARG;
  YinArgs a{p->window, p->tau_min, p->tau_max, p->hop, p->n_utts, 0, 0, p->sample_rate, p->threshold,
            (long long)p->total_in, (long long)p->total_frames, p->signal, p->in_offsets, p->frame_offsets,
            p->f0, p->aperiodicity, p->power, nullptr, nullptr};
  return yin_launch<false>(a, stream);
}

extern "C" int satt_yin_candidates(const satt_yin_candidates_params* p, void* stream) {
  if (!p || !p->signal || !p->in_offsets || !p->frame_offsets || !p->cand_period || !p->cand_value || !p->power) return SATT_E_BADARG;
  YinArgs a{p->window, p->tau_min, p->tau_max, p->hop, p->n_utts, 0, 0, 1.f, 0.f,   // (neither a sample rate nor a threshold here)
            (long long)p->total_in, (long long)p->total_frames, p->signal, p->in_offsets, p->frame_offsets,
            nullptr, nullptr, p->power, p->cand_period, p->cand_value};
  return yin_launch<true>(a, stream);
}
