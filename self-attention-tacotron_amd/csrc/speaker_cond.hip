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
