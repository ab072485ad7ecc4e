// The second stage of the pitch tracker: the cheapest path through the period candidates of csrc/yin.hip (satt_yin_candidates), one
// utterance per workgroup, a batch of utterances in ONE launch (DESIGN.md 3.6 holds the definition).  States 0 .. 7 of frame t are
// its candidate slots (used when period > 0), state 8 is "unvoiced"; all fp32, every operation rounded on its own:
//   obs(t, j)   = value_j + lag_bias * (period_j / (float)tau_max) for a used slot of a gated-in frame, else +inf;  obs(t, 8) = unvoiced_cost
//   trans(q, j) = 0 when both are 8, switch_cost when exactly one is 8, else jump_cost * (hi / lo - 1), hi = pq > pj ? pq : pj and
//                 lo the other one
//   delta_0     = obs(0, .);  delta_t(j) = (min_q (delta_{t-1}(q) + trans(q, j))) + obs(t, j), best = +inf and predecessor 8 to
//                 begin with, q ascending, taken when strictly < best
//   end         = the minimum of delta_{T-1} found the same way; the path walks the stored predecessors back
// These are the operations of utils/pitch.py f0_viterbi_numpy in its order, so the two agree bit for bit.
//
// The 81 transition costs and the 9 observation costs of a step do not depend on delta.  The workgroup has 4 waves: wave 0 walks the
// serial chain over a chunk of F0V_CH frames whose costs lie in LDS while waves 1 .. 3 fill the other buffer with the costs of the
// next chunk (all four fill the first one); one barrier per chunk hands the buffers over.  On the chain lane j <= 8 owns state j:
// nine broadcasts of delta_{t-1}(q), nine additions and comparisons, one addition, one predecessor byte to LDS.  The walk back
// runs on one lane over the predecessor bytes (9 per frame, 18 KiB for 2048 frames) and leaves the path in LDS; all threads then
// write f0 and state.  This is a latency-bound kernel: a chain of T steps per utterance, utterances side by side on the CUs.
//
// Memory safety does not depend on the CONTENTS of the tables: an utterance is computed only when its frame range lies in
// [0, total_frames] and holds 1 .. F0V_MAX_T frames, anything else is left untouched; a predecessor read back is cut to 0 .. 8.
// The barriers depend on T alone, which the whole workgroup shares.  Every LDS word read was written in this launch: the costs of
// a chunk by the fill in front of the barrier, the predecessors of frame t >= 1 by step t, the path by the walk.  No atomics,
// nothing crosses workgroups.
#include "common.h"
#include <math.h>

namespace {

constexpr int F0V_NT = 256;               // threads per workgroup: 4 waves of 64
constexpr int F0V_K = SATT_F0_CANDIDATES; // candidate slots of a frame
constexpr int F0V_S = F0V_K + 1;          // states: the slots and "unvoiced"
constexpr int F0V_MAX_T = 2048;           // satt_f0_viterbi_max_frames
constexpr int F0V_CH = 32;                // frames per chunk of staged costs
constexpr int F0V_ITEMS = F0V_S * F0V_S + F0V_S;   // 81 transition costs and 9 observation costs a frame

struct F0vArgs {
  int n_utts, tau_max;
  float sr, jump, sw, unv, bias;
  long long total_frames;
  const float* cper; const float* cval; const uint8_t* gate; const int64_t* frame_offsets;
  float* f0; uint8_t* state; float* cost;
};

// the costs of chunk c of the utterance at frame o0 with T frames, by the threads first, first + 1, .. of `count`
__device__ __forceinline__ void f0v_fill(const F0vArgs& a, long long o0, int T, int c, float* tr, float* ob, int first, int count) {
#pragma clang fp contract(off)
  for (int i = (int)threadIdx.x - first; i < F0V_CH * F0V_ITEMS; i += count) {
    const int lt = i / F0V_ITEMS, r = i - lt * F0V_ITEMS, t = c * F0V_CH + lt;
    if (t >= T) break;                                         // (i ascends: the frames behind are past T as well)
    const long long g = o0 + t;                                // 0 <= g < total_frames
    if (r < F0V_S * F0V_S) {
      if (t == 0) continue;                                    // no step leads into frame 0
      const int q = r / F0V_S, j = r - q * F0V_S;
      float v;
      if (q == F0V_K || j == F0V_K) v = (q == j) ? 0.f : a.sw;
      else {
        const float pq = a.cper[(g - 1) * F0V_K + q], pj = a.cper[g * F0V_K + j];
        const bool up = pq > pj;
        const float hi = up ? pq : pj, lo = up ? pj : pq;
        v = a.jump * (hi / lo - 1.f);
      }
      tr[lt * F0V_S * F0V_S + r] = v;
    } else {
      const int j = r - F0V_S * F0V_S;
      float v = a.unv;
      if (j < F0V_K) {
        const float per = a.cper[g * F0V_K + j];
        v = INFINITY;
        if (a.gate[g] != 0 && per > 0.f) v = a.cval[g * F0V_K + j] + a.bias * (per / (float)a.tau_max);
      }
      ob[lt * F0V_S + j] = v;
    }
  }
}

__global__ __launch_bounds__(F0V_NT) void f0_viterbi_k(F0vArgs a) {
#pragma clang fp contract(off)
  __shared__ float trs[2][F0V_CH * F0V_S * F0V_S];             // 20 736 bytes
  __shared__ float obs[2][F0V_CH * F0V_S];                     //  2 304
  __shared__ uint8_t pred[F0V_MAX_T * F0V_S];                  // 18 432
  __shared__ uint8_t path[F0V_MAX_T];                          //  2 048
  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (u >= a.n_utts) return;
  const long long o0 = a.frame_offsets[u], o1 = a.frame_offsets[u + 1];
  if (o0 < 0 || o1 <= o0 || o1 > a.total_frames || o1 - o0 > F0V_MAX_T) return;   // the whole workgroup takes the same way
  const int T = (int)(o1 - o0), chunks = (T + F0V_CH - 1) / F0V_CH;
  const int jj = lane < F0V_S ? lane : F0V_K;                  // the lanes past 8 of wave 0 go along as state 8 and store nothing

  f0v_fill(a, o0, T, 0, trs[0], obs[0], 0, F0V_NT);
  __syncthreads();
  float delta = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const int b = c & 1;
    if (wave == 0) {
      const int t1 = min(T - c * F0V_CH, F0V_CH);
      for (int lt = 0; lt < t1; ++lt) {
        const float o = obs[b][lt * F0V_S + jj];
        if (c == 0 && lt == 0) { delta = o; continue; }
        const float* tr = trs[b] + lt * F0V_S * F0V_S + jj;
        float best = INFINITY;
        int arg = F0V_K;
#pragma unroll
        for (int q = 0; q < F0V_S; ++q) {
          const float v = __shfl(delta, q) + tr[q * F0V_S];
          if (v < best) { best = v; arg = q; }
        }
        delta = best + o;
        if (lane < F0V_S) pred[(c * F0V_CH + lt) * F0V_S + lane] = (uint8_t)arg;
      }
    } else if (c + 1 < chunks) {
      f0v_fill(a, o0, T, c + 1, trs[b ^ 1], obs[b ^ 1], 64, F0V_NT - 64);
    }
    __syncthreads();
  }
  if (wave == 0) {
    float best = INFINITY;
    int end = F0V_K;
#pragma unroll
    for (int q = 0; q < F0V_S; ++q) {
      const float v = __shfl(delta, q);
      if (v < best) { best = v; end = q; }
    }
    if (lane == 0) {
      a.cost[u] = best;
      int s = end;
      for (int t = T - 1; t >= 0; --t) {                       // t < T <= 2048
        path[t] = (uint8_t)s;
        if (t > 0) s = min((int)pred[t * F0V_S + s], F0V_K);   // 0 <= s <= 8 whatever the byte holds
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < T; t += F0V_NT) {
    const int s = path[t];                                     // written above, 0 .. 8
    a.state[o0 + t] = (uint8_t)s;
    a.f0[o0 + t] = s < F0V_K ? a.sr / a.cper[(o0 + t) * F0V_K + s] : 0.f;
  }
}

inline bool f0v_cost_ok(float c) { return c >= 0.f && c < INFINITY; }

}  // namespace

extern "C" int satt_f0_viterbi_supported(int max_frames) { return (max_frames >= 1 && max_frames <= F0V_MAX_T) ? 1 : 0; }

extern "C" int satt_f0_viterbi_max_frames(void) { return F0V_MAX_T; }

extern "C" int satt_f0_viterbi(const satt_f0_viterbi_params* p, void* stream) {
  if (!p || !p->cand_period || !p->cand_value || !p->gate || !p->frame_offsets || !p->f0 || !p->state || !p->cost) return SATT_E_BADARG;
  if (p->n_utts < 1 || p->total_frames < 1 || p->max_frames < 1 || p->tau_max < 1) return SATT_E_BADARG;
  if (!satt_f0_viterbi_supported(p->max_frames)) return SATT_E_UNSUPPORTED;
  if (!(p->sample_rate > 0.f) || !f0v_cost_ok(p->jump_cost) || !f0v_cost_ok(p->switch_cost) || !f0v_cost_ok(p->unvoiced_cost) ||
      !f0v_cost_ok(p->lag_bias)) return SATT_E_BADARG;
  F0vArgs a{p->n_utts, p->tau_max, p->sample_rate, p->jump_cost, p->switch_cost, p->unvoiced_cost, p->lag_bias,
            (long long)p->total_frames, p->cand_period, p->cand_value, p->gate, p->frame_offsets, p->f0, p->state, p->cost};
  hipLaunchKernelGGL(f0_viterbi_k, dim3((unsigned)p->n_utts), dim3(F0V_NT), 0, (hipStream_t)stream, a);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}
