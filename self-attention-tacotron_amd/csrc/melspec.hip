// Log-mel spectrogram of a batch of utterances in ONE launch (the reference's Audio.melspectrogram, utils/audio.py:51-73, i.e.
// librosa.stft defaults: centred frames, reflect padding, periodic Hann window zero-padded to n_fft):
//   frame t of an utterance of n samples covers padded positions [t hop, t hop + n_fft), T = 1 + n / hop frames;
//   mag[t, k] = |rfft(window * frame)[k]|, k < n_fft / 2 + 1;   mel[t, m] = 20 log10(max(1e-5, sum_k basis[m, k] mag[t, k])) - ref.
//
// The transform is an FFT held in LDS, not a DFT GEMM (~4.5 MFLOP per LJSpeech frame dense against ~0.1 here).  It lives
// in stft_lds.h - Stockham stages, LDS layout and its bank analysis, recombination to the real transform - shared with griffin_lim.hip.
//   * the magnitudes stay in LDS ([frames][M + 1], in the buffer the last stage left free) and go to global memory only when the
//     caller asks for `mag`;
//   * the mel stage reads the magnitudes from LDS: one thread per (frame, band) walks the band's non-zero weights in ascending
//     bin order - a fixed summation order, no atomics: two launches on the same input are bit-identical, and a frame's result does
//     not depend on which frames share its workgroup or its launch.
// A workgroup takes STFT_FR = 4 consecutive frames of the batch (frames are numbered through the utterances; a slot finds its
// utterance by bisection of frame_offsets).  Nothing crosses workgroups.
//
// Memory safety does not depend on the CONTENTS of the device tables: sample ranges are clamped to [0, total_samples), rows written
// are < total_frames, band walks are clamped to the weight buffer and to the M + 1 bins.  Every LDS word read was written by the
// same launch (slots beyond the batch are transformed as zeros).
#include "stft_lds.h"

namespace {

constexpr int MS_MAX_MELS = 128;

struct MsArgs {
  int hop, num_mels, n_utts, n_band_weights;
  long long total_samples, total_frames;
  const float* signal; const int64_t* sample_offsets; const int64_t* frame_offsets;
  const float* window; const float2* twiddle;
  const int* band_start; const int* band_offset; const float* band_weight;
  float ref_level_db;
  float* mel; float* mag;
};

template <int N>
__global__ __launch_bounds__(stft_nt(N)) void melspec_k(MsArgs a) {
  constexpr int M = N / 2, NT = stft_nt(N), NF = M + 1;
  extern __shared__ __attribute__((aligned(16))) char ms_smem[];
  const int tid = threadIdx.x;
  const StftLds l = stft_carve<N>(ms_smem, a.twiddle, tid);
  float2 *x = l.x, *y = l.y;
  long long* s_base = l.slot;                               // [STFT_FR] first sample of the slot's utterance
  long long* s_n = s_base + STFT_FR;                        // [STFT_FR] its length (0: the slot is empty)
  long long* s_pos = s_n + STFT_FR;                         // [STFT_FR] t * hop
  const long long gf0 = (long long)blockIdx.x * STFT_FR;

  if (tid < STFT_FR) {
    const long long gf = gf0 + tid;
    long long base = 0, n = 0, pos = 0;
    if (gf < a.total_frames) {
      const int lo = stft_utt(a.frame_offsets, a.n_utts, gf);
      const long long t = gf - a.frame_offsets[lo];
      long long s0 = a.sample_offsets[lo], s1 = a.sample_offsets[lo + 1];
      s0 = s0 < 0 ? 0 : (s0 > a.total_samples ? a.total_samples : s0);
      s1 = s1 < s0 ? s0 : (s1 > a.total_samples ? a.total_samples : s1);
      const long long len = s1 - s0;
      if (t >= 0 && len >= NF && t <= len / a.hop) { base = s0; n = len; pos = t * a.hop; }
    }
    s_base[tid] = base; s_n[tid] = n; s_pos[tid] = pos;
  }
  __syncthreads();

  // windowed frames, two real samples a complex point
  for (int e = tid; e < STFT_FR * M; e += NT) {
    const int f = e / M, j = e - f * M;
    const long long n = s_n[f];
    float2 z = make_float2(0.f, 0.f);
    if (n > 0) {
      const float2 w = *reinterpret_cast<const float2*>(a.window + 2 * j);
      const long long i0 = s_pos[f] + 2 * j - M;
      const float* sig = a.signal + s_base[f];
      z = make_float2(sig[stft_reflect(i0, n)] * w.x, sig[stft_reflect(i0 + 1, n)] * w.y);
    }
    x[e] = z;
  }
  __syncthreads();

  stft_fft<N>(x, y, l.tw, tid);

  // x: Z[k] of the half-length transform.  Magnitudes of the n_fft-point real transform into the free buffer, [STFT_FR][2 M] floats
  float* magf = reinterpret_cast<float*>(y);
  for (int e = tid; e < STFT_FR * NF; e += NT) {
    const int f = e / NF, k = e - f * NF;
    const float2 X = stft_bin<N>(x + f * M, a.twiddle, k);
    const float m = sqrtf(X.x * X.x + X.y * X.y);
    magf[f * 2 * M + k] = m;
    if (a.mag && s_n[f] > 0) a.mag[(gf0 + f) * NF + k] = m;
  }
  __syncthreads();

  for (int e = tid; e < STFT_FR * a.num_mels; e += NT) {
    const int f = e / a.num_mels, m = e - f * a.num_mels;
    if (s_n[f] == 0) continue;
    const int k0 = a.band_start[m];
    int o0 = a.band_offset[m], o1 = a.band_offset[m + 1];
    o0 = o0 < 0 ? 0 : (o0 > a.n_band_weights ? a.n_band_weights : o0);
    o1 = o1 < o0 ? o0 : (o1 > a.n_band_weights ? a.n_band_weights : o1);
    const float* mf = magf + f * 2 * M;
    float acc = 0.f;
    for (int j = 0; j < o1 - o0; ++j) {
      const int k = k0 + j;
      if ((unsigned)k < (unsigned)NF) acc = fmaf(a.band_weight[o0 + j], mf[k], acc);
    }
    a.mel[(gf0 + f) * a.num_mels + m] = 20.f * log10f(fmaxf(1e-5f, acc)) - a.ref_level_db;
  }
}

inline bool ms_supported(int n_fft, int win, int hop, int num_mels) {
  if (!stft_supported(n_fft, win)) return false;
  if (hop < 1 || hop > n_fft) return false;
  return num_mels >= 1 && num_mels <= MS_MAX_MELS;
}

template <int N>
int ms_launch(const MsArgs& a, hipStream_t st) {
  if (!stft_lds_limit<melspec_k<N>, N>()) return SATT_E_LAUNCH;
  const long long blocks = (a.total_frames + STFT_FR - 1) / STFT_FR;
  hipLaunchKernelGGL(melspec_k<N>, dim3((unsigned)blocks), dim3(stft_nt(N)), stft_lds(N), st, a);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}

}  // namespace

extern "C" int satt_melspec_supported(int n_fft, int win, int hop, int num_mels) { return ms_supported(n_fft, win, hop, num_mels) ? 1 : 0; }

extern "C" int satt_melspec(const satt_melspec_params* p, void* stream) {
  if (!p || !p->signal || !p->sample_offsets || !p->frame_offsets || !p->window || !p->twiddle || !p->band_start || !p->band_offset ||
      !p->band_weight || !p->mel)
    return SATT_E_BADARG;
  if (p->n_utts < 1 || p->total_samples < 1 || p->total_frames < 1 || p->n_band_weights < 1) return SATT_E_BADARG;
  if (!ms_supported(p->n_fft, p->win, p->hop, p->num_mels)) return SATT_E_UNSUPPORTED;
  if ((p->total_frames + STFT_FR - 1) / STFT_FR > 0x7fffffffLL) return SATT_E_UNSUPPORTED;
  MsArgs a{p->hop, p->num_mels, p->n_utts, p->n_band_weights, (long long)p->total_samples, (long long)p->total_frames,
           p->signal, p->sample_offsets, p->frame_offsets, p->window, reinterpret_cast<const float2*>(p->twiddle),
           p->band_start, p->band_offset, p->band_weight, p->ref_level_db, p->mel, p->mag};
  hipStream_t st = (hipStream_t)stream;
  return stft_dispatch(p->n_fft, [&](auto n) { return ms_launch<decltype(n)::value>(a, st); });
}
