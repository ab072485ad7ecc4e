// Griffin-Lim phase reconstruction of a batch of utterances: the inverse of melspec.hip's framing (librosa / torch.istft with
// center = True: an utterance of T frames gives n = (T - 1) hop samples, and 1 + n / hop == T frames again).
//   y    = istft(mag * ang)      per frame irfft, x window, overlap-add over n_fft + hop (T - 1) padded positions, / sum_t window^2,
//                                trimmed by n_fft / 2 at either end
//   c    = stft(y)               melspec_k's framing: reflect-centred, windowed, rfft
//   u    = c + alpha (c - c_prev);   ang' = u / max(|u|, 1e-30);   c_prev' = c
// Three kernels, nothing crosses workgroups inside a launch (no grid barrier, no persistent kernel, no atomics):
//   gl_synth_k     4 frames a workgroup: X = mag * ang (imaginary parts of bins 0 and n_fft / 2 dropped, as every c2r transform
//                  does), Z[k] = E[k] + i O[k] with E = (X[k] + conj X[M - k]) / 2, O = conj(w^k) (X[k] - conj X[M - k]) / 2,
//                  z = ifft_M(Z) = conj(fft_M(conj Z)) / M through the SAME Stockham stage loop as the forward transform,
//                  frame[2 j] = Re z[j], frame[2 j + 1] = Im z[j]; the windowed frame goes to workspace [frames][n_fft];
//   gl_analysis_k  4 frames a workgroup: every sample of the frame is GATHERED from the workspace - the sum over the frames that
//                  cover it in ascending frame order, times the reciprocal envelope - windowed, transformed, recombined to the
//                  n_fft / 2 + 1 bins and turned into ang' / c_prev' (/ spec_out);
//   gl_signal_k    one workgroup a frame: the same gather for the hop samples behind the frame's centre, written to `signal`.
// An entry call enqueues (synth, analysis) x iters, synth, signal: two launches an iteration.  The gather replaces an overlap-ADD:
// a sample's value has one fixed summation order whatever shares its launch, so two launches are bit-identical and an utterance's
// result does not depend on its batch (the property melspec_k has).
//
// The Stockham stage loop, the LDS layout and the forward recombination live in stft_lds.h, shared with melspec.hip.  The
// recombination of gl_synth_k reads global memory and writes LDS with unit stride (one float2 a lane: conflict-free);
// gl_analysis_k's reads Z[k] ascending and Z[M - k] descending, both unit stride.
//
// Envelope: sum_{0 <= t < T} w^2[p - t hop] = F[p mod hop] - (p < n_fft ? H[p] : 0) - (p >= T hop ? G[p - T hop] : 0) from the
// float64 tables F [hop], H [n_fft], G [n_fft] of the host (utils/audio.py overlap_envelope_tables); the difference is taken in
// float64 and rounded once, so it is the float32 nearest to the direct float64 sum for every frame count.
//
// Memory safety does not depend on the CONTENTS of the device tables: an utterance is taken only when its frame rows lie inside
// [0, total_frames), its samples inside [0, total_samples), its sample count is (T - 1) hop and n_fft / 2 + 1 <= (T - 1) hop <
// 2^30; anything else is left untouched.  Frames gathered are rows of the utterance itself, in-frame indices lie inside the
// window's support.  Every LDS word read was written by the same launch.
#include "stft_lds.h"

namespace {

struct GlArgs {
  int hop, win, lead, lead_mod, n_utts;
  float alpha;
  long long total_samples, total_frames;
  const int64_t* sample_offsets; const int64_t* frame_offsets;
  const float* window; const float2* twiddle; const double* envelope;
  const float* mag; float2* ang; float2* c_prev; float2* spec_out;
  float* signal; float* ws;
};

// frame slot of a workgroup: the utterance's first frame row (-1: the slot is empty), its frame count, the frame's index in it, the
// utterance's first sample
struct GlSlot { long long f0; int T, t; long long s0; };

template <int N>
__device__ __forceinline__ GlSlot gl_find(const GlArgs& a, long long gf) {
  GlSlot r{-1, 0, 0, 0};
  if (gf >= a.total_frames) return r;
  const int lo = stft_utt(a.frame_offsets, a.n_utts, gf);
  const long long f0 = a.frame_offsets[lo], f1 = a.frame_offsets[lo + 1];
  const long long s0 = a.sample_offsets[lo], s1 = a.sample_offsets[lo + 1];
  if (f0 < 0 || f1 <= f0 || f1 > a.total_frames || gf < f0 || gf >= f1) return r;
  if (s0 < 0 || s1 < s0 || s1 > a.total_samples) return r;
  const long long n = (f1 - f0 - 1) * (long long)a.hop;
  if (n != s1 - s0 || n < N / 2 + 1 || n >= (1LL << 30)) return r;
  r.f0 = f0; r.T = (int)(f1 - f0); r.t = (int)(gf - f0); r.s0 = s0;
  return r;
}

// sample at padded position p (n_fft / 2 <= p < n_fft / 2 + (T - 1) hop) of an utterance whose windowed frames are the rows wsu:
// the frames t with lead <= p - t hop < lead + win (the window's support), 0 <= t < T, ascending, times 1 / envelope
template <int N>
__device__ __forceinline__ float gl_sample(const GlArgs& a, const float* wsu, int T, int p) {
  const int d = p - a.lead;                               // >= 0: lead <= n_fft / 2 <= p
  const int tu = d / a.hop, r = d - tu * a.hop;           // the last covering frame without the T bound; its in-support index
  const int cnt = (a.win - 1 - r) / a.hop;                // covering frames in front of it
  const int thi = tu < T - 1 ? tu : T - 1;
  const int tlo = tu - cnt > 0 ? tu - cnt : 0;
  float acc = 0.f;
  for (int t = tlo; t <= thi; ++t) acc += wsu[(long long)t * N + (p - t * a.hop)];
  int pm = r + a.lead_mod;                                // p mod hop
  pm = pm >= a.hop ? pm - a.hop : pm;
  double env = a.envelope[pm];
  if (p < N) env -= a.envelope[a.hop + p];
  const int g = p - T * a.hop;                            // < n_fft / 2 - hop
  if (g >= 0) env -= a.envelope[a.hop + N + g];
  return acc * (1.0f / (float)env);
}

template <int N>
__global__ __launch_bounds__(stft_nt(N)) void gl_synth_k(GlArgs a) {
  constexpr int M = N / 2, NT = stft_nt(N), NF = M + 1;
  extern __shared__ __attribute__((aligned(16))) char gl_smem[];
  const int tid = threadIdx.x;
  const StftLds l = stft_carve<N>(gl_smem, a.twiddle, tid);
  float2 *x = l.x, *y = l.y;
  long long* s_f0 = l.slot;                                 // [STFT_FR]
  const long long gf0 = (long long)blockIdx.x * STFT_FR;

  if (tid < STFT_FR) s_f0[tid] = gl_find<N>(a, gf0 + tid).f0;
  __syncthreads();

  // conj(Z[k]), k < M, of every frame (zeros for an empty slot)
  for (int e = tid; e < STFT_FR * M; e += NT) {
    const int f = e / M, k = e - f * M;
    float2 z = make_float2(0.f, 0.f);
    if (s_f0[f] >= 0) {
      const long long row = (gf0 + f) * NF;
      const float mk = a.mag[row + k], mm = a.mag[row + M - k];
      const float2 ak = a.ang[row + k], am = a.ang[row + M - k];
      float2 xk = make_float2(mk * ak.x, mk * ak.y), xm = make_float2(mm * am.x, -(mm * am.y));   // X[k], conj X[M - k]
      if (k == 0) { xk.y = 0.f; xm.y = 0.f; }
      const float2 E = make_float2(0.5f * (xk.x + xm.x), 0.5f * (xk.y + xm.y));
      const float2 D = make_float2(0.5f * (xk.x - xm.x), 0.5f * (xk.y - xm.y));
      float2 w = a.twiddle[k];
      w.y = -w.y;                                          // conj(w^k) = exp(+2 pi i k / n_fft)
      const float2 O = stft_cmul(w, D);
      z = make_float2(E.x - O.y, -(E.y + O.x));            // conj(E + i O)
    }
    x[e] = z;
  }
  __syncthreads();

  stft_fft<N>(x, y, l.tw, tid);

  // z[j] = conj(x[j]) / M: samples 2 j and 2 j + 1 of the frame, windowed
  constexpr float inv_m = 1.0f / (float)M;
  for (int e = tid; e < STFT_FR * M; e += NT) {
    const int f = e / M, j = e - f * M;
    if (s_f0[f] < 0) continue;
    const float2 w = *reinterpret_cast<const float2*>(a.window + 2 * j);
    const float2 v = x[e];
    *reinterpret_cast<float2*>(a.ws + (gf0 + f) * N + 2 * j) = make_float2(v.x * inv_m * w.x, -(v.y * inv_m) * w.y);
  }
}

template <int N>
__global__ __launch_bounds__(stft_nt(N)) void gl_analysis_k(GlArgs a) {
  constexpr int M = N / 2, NT = stft_nt(N), NF = M + 1;
  extern __shared__ __attribute__((aligned(16))) char gl_smem[];
  const int tid = threadIdx.x;
  const StftLds l = stft_carve<N>(gl_smem, a.twiddle, tid);
  float2 *x = l.x, *y = l.y;
  long long* s_f0 = l.slot;                                 // [STFT_FR]
  int* s_T = reinterpret_cast<int*>(s_f0 + STFT_FR);        // [STFT_FR]
  int* s_t = s_T + STFT_FR;                                 // [STFT_FR]
  const long long gf0 = (long long)blockIdx.x * STFT_FR;

  if (tid < STFT_FR) {
    const GlSlot s = gl_find<N>(a, gf0 + tid);
    s_f0[tid] = s.f0; s_T[tid] = s.T; s_t[tid] = s.t;
  }
  __syncthreads();

  // windowed frames of the re-synthesised signal, two real samples a complex point
  for (int e = tid; e < STFT_FR * M; e += NT) {
    const int f = e / M, j = e - f * M;
    float2 z = make_float2(0.f, 0.f);
    if (s_f0[f] >= 0) {
      const int T = s_T[f], n = (T - 1) * a.hop;
      const float2 w = *reinterpret_cast<const float2*>(a.window + 2 * j);
      const int i = s_t[f] * a.hop + 2 * j - M, i0 = stft_reflect(i, n), i1 = stft_reflect(i + 1, n);
      const float* wsu = a.ws + s_f0[f] * N;
      // (where the padded window is zero - (n_fft - win) / 2 points at either end - nothing is gathered)
      z = make_float2(w.x != 0.f ? gl_sample<N>(a, wsu, T, i0 + M) * w.x : 0.f, w.y != 0.f ? gl_sample<N>(a, wsu, T, i1 + M) * w.y : 0.f);
    }
    x[e] = z;
  }
  __syncthreads();

  stft_fft<N>(x, y, l.tw, tid);

  for (int e = tid; e < STFT_FR * NF; e += NT) {
    const int f = e / NF, k = e - f * NF;
    if (s_f0[f] < 0) continue;
    const float2 c = stft_bin<N>(x + f * M, a.twiddle, k);
    const long long o = (gf0 + f) * NF + k;
    float2 u = c;
    if (a.alpha != 0.f) {
      const float2 cp = a.c_prev[o];
      u = make_float2(c.x + a.alpha * (c.x - cp.x), c.y + a.alpha * (c.y - cp.y));
    }
    const float inv = 1.0f / fmaxf(sqrtf(u.x * u.x + u.y * u.y), 1e-30f);
    a.ang[o] = make_float2(u.x * inv, u.y * inv);
    if (a.c_prev) a.c_prev[o] = c;
    if (a.spec_out) a.spec_out[o] = c;
  }
}

// one workgroup a frame row: the hop samples [t hop, (t + 1) hop) of its utterance (the last frame of an utterance has none)
template <int N>
__global__ __launch_bounds__(256) void gl_signal_k(GlArgs a) {
  __shared__ GlSlot slot;
  if (threadIdx.x == 0) slot = gl_find<N>(a, (long long)blockIdx.x);
  __syncthreads();
  const GlSlot s = slot;
  if (s.f0 < 0 || s.t >= s.T - 1) return;
  const float* wsu = a.ws + s.f0 * N;
  float* out = a.signal + s.s0 + (long long)s.t * a.hop;
  for (int i = threadIdx.x; i < a.hop; i += 256) out[i] = gl_sample<N>(a, wsu, s.T, s.t * a.hop + i + N / 2);
}

inline bool gl_supported(int n_fft, int win, int hop) {
  return stft_supported(n_fft, win) && hop >= 1 && hop <= win / 2;
}

template <int N>
int gl_run(GlArgs a, int iters, float2* spec_out, hipStream_t st) {
  const size_t lds = stft_lds(N);
  const bool limit_s = stft_lds_limit<gl_synth_k<N>, N>(), limit_a = stft_lds_limit<gl_analysis_k<N>, N>();
  if (!limit_s || !limit_a) return SATT_E_LAUNCH;
  const dim3 grid((unsigned)((a.total_frames + STFT_FR - 1) / STFT_FR)), block(stft_nt(N));
  for (int it = 0; it < iters; ++it) {
    a.spec_out = it == iters - 1 ? spec_out : nullptr;
    hipLaunchKernelGGL(gl_synth_k<N>, grid, block, lds, st, a);
    SATT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gl_analysis_k<N>, grid, block, lds, st, a);
    SATT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gl_synth_k<N>, grid, block, lds, st, a);
  SATT_LAUNCH_CHECK();
  hipLaunchKernelGGL(gl_signal_k<N>, dim3((unsigned)a.total_frames), dim3(256), 0, st, a);
  SATT_LAUNCH_CHECK();
  return SATT_OK;
}

}  // namespace

extern "C" int satt_griffin_lim_supported(int n_fft, int win, int hop) { return gl_supported(n_fft, win, hop) ? 1 : 0; }

extern "C" int64_t satt_griffin_lim_workspace_bytes(int n_fft, int64_t total_frames) {
  if (n_fft < 1 || total_frames < 1) return 0;
  return total_frames * (int64_t)n_fft * (int64_t)sizeof(float);
}

extern "C" int satt_griffin_lim(const satt_griffin_lim_params* p, void* stream) {
  if (!p || !p->sample_offsets || !p->frame_offsets || !p->window || !p->twiddle || !p->envelope || !p->mag || !p->ang || !p->signal ||
      !p->workspace)
    return SATT_E_BADARG;
  if (p->n_utts < 1 || p->total_samples < 1 || p->total_frames < 1 || p->iters < 0) return SATT_E_BADARG;
  if (!(p->alpha == p->alpha) || (p->alpha != 0.f && !p->c_prev)) return SATT_E_BADARG;
  if (!gl_supported(p->n_fft, p->win, p->hop)) return SATT_E_UNSUPPORTED;
  if (p->total_frames > 0x7fffffffLL) return SATT_E_UNSUPPORTED;
  const int lead = (p->n_fft - p->win) / 2;
  GlArgs a{p->hop, p->win, lead, lead % p->hop, p->n_utts, p->alpha, (long long)p->total_samples, (long long)p->total_frames,
           p->sample_offsets, p->frame_offsets, p->window, reinterpret_cast<const float2*>(p->twiddle), p->envelope,
           p->mag, reinterpret_cast<float2*>(p->ang), reinterpret_cast<float2*>(p->c_prev), nullptr, p->signal, p->workspace};
  float2* spec = reinterpret_cast<float2*>(p->spec_out);
  hipStream_t st = (hipStream_t)stream;
  return stft_dispatch(p->n_fft, [&](auto n) { return gl_run<decltype(n)::value>(a, p->iters, spec, st); });
}
