// Speaker term of the multi-speaker decoder pre-net with the resize layer (reference models/models.py:307-312 composes
// Dense(R, relu) behind the speaker embedding; modules/multi_speaker_modules.py:27-32 projects the result):
//   semb = table[id - offset]            [B, E]      (or a ready embedding, or ONE id for every row: speaker_for_synthesis)
//   rs   = relu(semb Wr + br)            [B, R]
//   sproj = softsign(rs Ws + bs)         [B, P0]
// The term is constant over time: B rows, three tiny products, at the head of the decoder's critical path.  Composed from the
// generic ops the forward is 3 launch-bound launches; here it is ONE launch of one workgroup of 1024 threads (16 waves).
// Activations live in LDS, weights are read from global memory with the output column on the lanes (coalesced; a weight element is
// reused for four batch rows from registers).  fp32 FMA throughout.
//
// FORWARD ONLY.  The backward of the term runs as the chain of generic ops (engine.py _speaker_term_bwd): a one-workgroup backward
// kernel of this design was built and measured at 75 us per call against 49 us for the chain (its serial weight-row reads are
// latency-bound in a single workgroup) and was not kept - profiles/speaker_cond_bench_and_kernel_times.txt.
//
// LDS discipline: every word that is read was written by the same launch - tests run this under SATT_DEBUG_POISON_LDS.
#include "common.h"

namespace {

constexpr int SC_NT = 1024;
constexpr int SC_MAX_E = 256, SC_MAX_R = 256, SC_MAX_P0 = 512, SC_MAX_B = 256;
constexpr int SC_LDS_MAX = 64 * 1024;
constexpr int SC_RT = 4;            // batch rows per thread and weight element

enum { SC_MODE_IDS = 0, SC_MODE_EMBED = 1, SC_MODE_SCALAR = 2 };

struct ScArgs {
  const int64_t* ids; const float* emb_in; int64_t scalar_id; int mode;
  int B, nspk, offset, E, R, P0;
  const float* table; const float* Wr; const float* br; const float* Ws; const float* bs;
};

// table row of batch row b; ids outside the table are clamped (memory safety only: the input pipeline and validate_params reject them)
__device__ __forceinline__ int sc_row_of(const ScArgs& a, int b) {
  const int64_t v = (a.mode == SC_MODE_SCALAR ? a.scalar_id : a.ids[b]) - a.offset;
  return (int)(v < 0 ? 0 : (v >= a.nspk ? a.nspk - 1 : v));
}

__global__ __launch_bounds__(SC_NT) void speaker_cond_fwd_k(ScArgs a, float* __restrict__ semb, float* __restrict__ rs,
                                                            float* __restrict__ sproj) {
  extern __shared__ float lds[];
  float* x = lds;                   // [B][E]
  float* y = x + a.B * a.E;         // [B][R]
  const int tid = threadIdx.x, B = a.B, E = a.E, R = a.R, P0 = a.P0;
  for (int e = tid; e < B * E; e += SC_NT) {
    const int b = e / E, k = e - b * E;
    const float v = a.mode == SC_MODE_EMBED ? a.emb_in[e] : a.table[(int64_t)sc_row_of(a, b) * E + k];
    x[e] = v; semb[e] = v;
  }
  __syncthreads();
  for (int e = tid; e < B * R; e += SC_NT) {
    const int b = e / R, c = e - b * R;
    float acc = a.br[c];
    for (int k = 0; k < E; ++k) acc = fmaf(x[b * E + k], a.Wr[k * R + c], acc);
    acc = fmaxf(acc, 0.f);
    y[e] = acc; rs[e] = acc;
  }
  __syncthreads();
  const int nbt = (B + SC_RT - 1) / SC_RT;
  for (int e = tid; e < nbt * P0; e += SC_NT) {
    const int bt = e / P0, c = e - bt * P0, b0 = bt * SC_RT;
    int rb[SC_RT]; float acc[SC_RT];
#pragma unroll
    for (int i = 0; i < SC_RT; ++i) { rb[i] = min(b0 + i, B - 1) * R; acc[i] = a.bs[c]; }
    for (int k = 0; k < R; ++k) {
      const float w = a.Ws[(int64_t)k * P0 + c];
#pragma unroll
      for (int i = 0; i < SC_RT; ++i) acc[i] = fmaf(y[rb[i] + k], w, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < SC_RT; ++i)
      if (b0 + i < B) sproj[(int64_t)(b0 + i) * P0 + c] = acc[i] / (1.f + fabsf(acc[i]));
  }
}

inline size_t sc_fwd_lds(int B, int E, int R) { return sizeof(float) * (size_t)B * (E + R); }

inline bool sc_supported(int B, int E, int R, int P0) {
  if (B < 1 || E < 1 || R < 1 || P0 < 1) return false;
  if (B > SC_MAX_B || E > SC_MAX_E || R > SC_MAX_R || P0 > SC_MAX_P0) return false;
  return sc_fwd_lds(B, E, R) <= (size_t)SC_LDS_MAX;
}

inline bool sc_args_ok(const ScArgs& a) {
  if (a.mode == SC_MODE_IDS) return a.ids && a.table && a.nspk >= 1;
  if (a.mode == SC_MODE_EMBED) return a.emb_in != nullptr;
  if (a.mode == SC_MODE_SCALAR) return a.table && a.nspk >= 1;
  return false;
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int satt_speaker_cond_supported(int B, int E, int R, int P0) { return sc_supported(B, E, R, P0) ? 1 : 0; }

extern "C" int satt_speaker_cond_fwd(int mode, const int64_t* ids, int64_t scalar_id, const float* emb_in, int B, const float* table,
                                     int nspk, int offset, int E, const float* Wr, const float* br, int R, const float* Ws,
                                     const float* bs, int P0, float* semb, float* rs, float* sproj, void* stream) {
  if (B <= 0 || E <= 0 || R <= 0 || P0 <= 0 || !Wr || !br || !Ws || !bs || !semb || !rs || !sproj) return SATT_E_BADARG;
  ScArgs a{ids, emb_in, scalar_id, mode, B, nspk, offset, E, R, P0, table, Wr, br, Ws, bs};
  if (!sc_args_ok(a)) return SATT_E_BADARG;
  if (!sc_supported(B, E, R, P0)) return SATT_E_UNSUPPORTED;
  hipLaunchKernelGGL(speaker_cond_fwd_k, dim3(1), dim3(SC_NT), sc_fwd_lds(B, E, R), S_, a, semb, rs, sproj);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}

// ---- speaker vector fed to the decoder memories (speaker_embedd_to_decoder, reference models/models.py:366-372) ----------------
// The speaker columns of a memory are the same in every memory row and attention weights sum to one, so the wide memories are
// never formed (engine.py): every consumer of the wide context receives a per-sample row instead.  Two memory-bound kernels:
//   rows_bcast_add:  y[b, t, :] += v[b, :]            for t0 <= t < t1       (gate pre-activations, key rows)
//   rows_time_sum:   dv[b, :]   = sum_t dy[b, t, :]   for t0 <= t < min(T, len_b)   (their gradients)
// rows_bcast_add: one float4 (or, without 16-byte rows, one float) per thread, the feature index on the lanes.
// rows_time_sum: a workgroup owns 64 columns of one sample (lanes = columns: coalesced 256-byte row pieces); its RS_NW waves take
// the time steps t0 + w, t0 + w + RS_NW, ... in ascending order and the partial sums are combined through LDS in wave order -
// a FIXED summation order, no float atomics: two runs on the same input are bit-equal.  Every LDS word read was written by the
// same launch (all RS_NW x 64 partials are stored, columns beyond N as zeros).
namespace {

constexpr int RB_NT = 256;
constexpr int RS_NW = 8, RS_COLS = 64;

template <bool VEC>
__global__ __launch_bounds__(RB_NT) void rows_bcast_add_k(float* __restrict__ y, int64_t ld, const float* __restrict__ v, int64_t ldv,
                                                          int T, int N, int t0, int nt, int64_t total) {
  const int W = VEC ? N / 4 : N;            // work items per row
  const int64_t idx = (int64_t)blockIdx.x * RB_NT + threadIdx.x;
  if (idx >= total) return;
  const int64_t row = idx / W;
  const int c = (int)(idx - row * W);
  const int b = (int)(row / nt), t = t0 + (int)(row - (int64_t)b * nt);
  float* yp = y + ((int64_t)b * T + t) * ld;
  const float* vp = v + (int64_t)b * ldv;
  if (VEC) {
    float4 a = *reinterpret_cast<float4*>(yp + 4 * c);
    const float4 s = *reinterpret_cast<const float4*>(vp + 4 * c);
    a.x += s.x; a.y += s.y; a.z += s.z; a.w += s.w;
    *reinterpret_cast<float4*>(yp + 4 * c) = a;
  } else {
    yp[c] += vp[c];
  }
}

__global__ __launch_bounds__(RS_NW * RS_COLS) void rows_time_sum_k(const float* __restrict__ dy, int64_t ld,
                                                                   const int64_t* __restrict__ lengths, float* __restrict__ dv,
                                                                   int64_t lddv, int T, int N, int t0) {
  __shared__ float part[RS_NW][RS_COLS];
  const int lane = threadIdx.x % RS_COLS, w = threadIdx.x / RS_COLS;
  const int b = blockIdx.y, n = blockIdx.x * RS_COLS + lane;
  int te = T;
  if (lengths) { const int64_t l = lengths[b]; te = (int)(l < 0 ? 0 : (l < T ? l : T)); }
  float acc = 0.f;
  if (n < N) {
    const float* p = dy + (int64_t)b * T * ld + n;
    for (int t = t0 + w; t < te; t += RS_NW) acc += p[(int64_t)t * ld];
  }
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && n < N) {
    float s = part[0][lane];
#pragma unroll
    for (int i = 1; i < RS_NW; ++i) s += part[i][lane];
    dv[(int64_t)b * lddv + n] = s;
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int satt_rows_bcast_add(float* y, int64_t ld, const float* v, int64_t ldv, int B, int T, int N, int t0, int t1,
                                   void* stream) {
  if (!y || !v || B <= 0 || T <= 0 || N <= 0 || ld < N || ldv < N || t0 < 0 || t1 > T) return SATT_E_BADARG;
  if (t0 >= t1) return SATT_OK;            // empty range: y stays as it is
  const int nt = t1 - t0;
  const bool vec = N % 4 == 0 && ld % 4 == 0 && ldv % 4 == 0 && al16(y) && al16(v);
  const int64_t total = (int64_t)B * nt * (vec ? N / 4 : N);
  const int64_t blocks = (total + RB_NT - 1) / RB_NT;
  if (blocks > 0x7fffffffLL) return SATT_E_UNSUPPORTED;
  if (vec) hipLaunchKernelGGL(rows_bcast_add_k<true>, dim3((unsigned)blocks), dim3(RB_NT), 0, S_, y, ld, v, ldv, T, N, t0, nt, total);
  else hipLaunchKernelGGL(rows_bcast_add_k<false>, dim3((unsigned)blocks), dim3(RB_NT), 0, S_, y, ld, v, ldv, T, N, t0, nt, total);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}

extern "C" int satt_rows_time_sum(const float* dy, int64_t ld, const int64_t* lengths, float* dv, int64_t lddv, int B, int T, int N,
                                  int t0, void* stream) {
  if (!dy || !dv || B <= 0 || T <= 0 || N <= 0 || ld < N || lddv < N || t0 < 0 || B > 65535) return SATT_E_BADARG;
  hipLaunchKernelGGL(rows_time_sum_k, dim3((N + RS_COLS - 1) / RS_COLS, B), dim3(RS_NW * RS_COLS), 0, S_, dy, ld, lengths, dv, lddv,
                     T, N, t0);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}
