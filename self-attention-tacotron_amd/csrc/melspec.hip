// Log-mel spectrogram of a batch of utterances in ONE launch (the reference's Audio.melspectrogram, utils/audio.py:51-73, i.e.
// librosa.stft defaults: centred frames, reflect padding, periodic Hann window zero-padded to n_fft):
//   frame t of an utterance of n samples covers padded positions [t hop, t hop + n_fft), T = 1 + n / hop frames;
//   mag[t, k] = |rfft(window * frame)[k]|, k < n_fft / 2 + 1;   mel[t, m] = 20 log10(max(1e-5, sum_k basis[m, k] mag[t, k])) - ref.
//
// The transform is an FFT held in LDS, not a DFT GEMM (~4.5 MFLOP per LJSpeech frame dense against ~0.1 here).
//   * real input through a half-length complex transform: z[j] = x[2j] + i x[2j+1], M = n_fft / 2 points;
//   * Stockham autosort, radix 4 (decimation in frequency) with one radix-2 stage behind it when log2 M is odd: every stage reads
//     one LDS buffer and writes the other, no bit reversal.  Stage (n, s), n s = M: butterfly t = p s + q reads
//     x[q + s (p + c n/4)] and writes y[q + s (4 p + c)], c = 0..3, twiddles w^(c p s) from the M-th roots kept in LDS;
//   * X[k] = E[k] + exp(-2 pi i k / n_fft) O[k] from Z[k] and conj(Z[M - k]); the magnitudes stay in LDS ([frames][M + 1], in the
//     buffer the last stage left free) and go to global memory only when the caller asks for `mag`;
//   * the mel stage reads the magnitudes from LDS: one thread per (frame, band) walks the band's non-zero weights in ascending
//     bin order - a fixed summation order, no atomics: two launches on the same input are bit-identical, and a frame's result does
//     not depend on which frames share its workgroup or its launch.
// A workgroup takes MS_FR = 4 consecutive frames of the batch (frames are numbered through the utterances; a slot finds its utterance
// by bisection of frame_offsets), so LDS = (2 MS_FR + 1) M float2 = 144 KiB at n_fft = 4096.  Nothing crosses workgroups.
//
// LDS banks (8-byte accesses: 32 lanes a group on reads, 16 contiguous lanes on writes): with s >= 16 lanes of a group differ in q
// alone, so reads and writes are unit-stride and conflict-free.  The stages with s = 1 and s = 4 read unit-stride (in p resp. in
// (p, q)) but write with a stride of 4 s float2: with s = 1 the four outputs of a butterfly are adjacent (32 bytes per lane, wide
// stores), with s = 4 a group of 16 lanes writes 4 runs of 4 float2 - the one stage that pays store conflicts.
//
// Memory safety does not depend on the CONTENTS of the device tables: sample ranges are clamped to [0, total_samples), rows written
// are < total_frames, band walks are clamped to the weight buffer and to the M + 1 bins.  Every LDS word read was written by the
// same launch (slots beyond the batch are transformed as zeros).
#include "common.h"

namespace {

constexpr int MS_FR = 4;                // frames per workgroup
constexpr int MS_MAX_MELS = 128;

constexpr int ms_nt(int N) { return N >= 4096 ? 1024 : (N >= 2048 ? 512 : 256); }
inline size_t ms_lds(int N) { return (size_t)(2 * MS_FR + 1) * (N / 2) * sizeof(float2) + 4 * MS_FR * sizeof(long long); }

struct MsArgs {
  int hop, num_mels, n_utts, n_band_weights;
  long long total_samples, total_frames;
  const float* signal; const int64_t* sample_offsets; const int64_t* frame_offsets;
  const float* window; const float2* twiddle;
  const int* band_start; const int* band_offset; const float* band_weight;
  float ref_level_db;
  float* mel; float* mag;
};

__device__ __forceinline__ float2 ms_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 ms_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 ms_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

template <int N>
__global__ __launch_bounds__(ms_nt(N)) void melspec_k(MsArgs a) {
  constexpr int M = N / 2, NT = ms_nt(N), NF = M + 1, NB = M / 4;
  extern __shared__ __attribute__((aligned(16))) char ms_smem[];
  float2* x = reinterpret_cast<float2*>(ms_smem);          // [MS_FR][M]
  float2* y = x + MS_FR * M;                                // [MS_FR][M]
  float2* tw = y + MS_FR * M;                               // [M]: exp(-2 pi i j / M)
  long long* s_base = reinterpret_cast<long long*>(tw + M); // [MS_FR] first sample of the slot's utterance
  long long* s_n = s_base + MS_FR;                          // [MS_FR] its length (0: the slot is empty)
  long long* s_pos = s_n + MS_FR;                           // [MS_FR] t * hop
  const int tid = threadIdx.x;
  const long long gf0 = (long long)blockIdx.x * MS_FR;

  if (tid < MS_FR) {
    const long long gf = gf0 + tid;
    long long base = 0, n = 0, pos = 0;
    if (gf < a.total_frames) {
      int lo = 0, hi = a.n_utts;                            // the last utterance whose first frame is <= gf
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.frame_offsets[mid] <= gf) lo = mid; else hi = mid;
      }
      const long long t = gf - a.frame_offsets[lo];
      long long s0 = a.sample_offsets[lo], s1 = a.sample_offsets[lo + 1];
      s0 = s0 < 0 ? 0 : (s0 > a.total_samples ? a.total_samples : s0);
      s1 = s1 < s0 ? s0 : (s1 > a.total_samples ? a.total_samples : s1);
      const long long len = s1 - s0;
      if (t >= 0 && len >= NF && t <= len / a.hop) { base = s0; n = len; pos = t * a.hop; }
    }
    s_base[tid] = base; s_n[tid] = n; s_pos[tid] = pos;
  }
  for (int j = tid; j < M; j += NT) tw[j] = a.twiddle[2 * j];
  __syncthreads();

  // windowed frames, two real samples a complex point; signal index i of padded position q is q - M, reflected once at either end
  // (n >= M + 1 and t hop <= n keep the reflected index inside [0, n))
  for (int e = tid; e < MS_FR * M; e += NT) {
    const int f = e / M, j = e - f * M;
    const long long n = s_n[f];
    float2 z = make_float2(0.f, 0.f);
    if (n > 0) {
      const float2 w = *reinterpret_cast<const float2*>(a.window + 2 * j);
      long long i0 = s_pos[f] + 2 * j - M, i1 = i0 + 1;
      i0 = i0 < 0 ? -i0 : (i0 >= n ? 2 * (n - 1) - i0 : i0);
      i1 = i1 < 0 ? -i1 : (i1 >= n ? 2 * (n - 1) - i1 : i1);
      const float* sig = a.signal + s_base[f];
      z = make_float2(sig[i0] * w.x, sig[i1] * w.y);
    }
    x[e] = z;
  }
  __syncthreads();

#pragma unroll
  for (int n = M, s = 1; n >= 4; n >>= 2, s <<= 2) {
    const int n1 = n >> 2;
    for (int e = tid; e < MS_FR * NB; e += NT) {
      const int f = e / NB, t = e - f * NB, p = t / s, q = t - p * s;
      const float2* xf = x + f * M;
      float2* yf = y + f * M;
      const float2 A = xf[q + s * p], B = xf[q + s * (p + n1)], C = xf[q + s * (p + 2 * n1)], D = xf[q + s * (p + 3 * n1)];
      const float2 apc = ms_add(A, C), amc = ms_sub(A, C), bpd = ms_add(B, D), bmd = ms_sub(B, D);
      const float2 jbmd = make_float2(-bmd.y, bmd.x);
      const float2 w1 = tw[p * s], w2 = tw[2 * p * s], w3 = tw[3 * p * s];
      yf[q + s * (4 * p)] = ms_add(apc, bpd);
      yf[q + s * (4 * p + 1)] = ms_cmul(w1, ms_sub(amc, jbmd));
      yf[q + s * (4 * p + 2)] = ms_cmul(w2, ms_sub(apc, bpd));
      yf[q + s * (4 * p + 3)] = ms_cmul(w3, ms_add(amc, jbmd));
    }
    __syncthreads();
    float2* tmp = x; x = y; y = tmp;
  }
  constexpr bool ODD = M == 512 || M == 2048;               // log2 M odd (n_fft 1024 and 4096): a radix-2 stage is left, s = M / 2
  if (ODD) {
    constexpr int s = M / 2;
    for (int e = tid; e < MS_FR * s; e += NT) {
      const int f = e / s, q = e - f * s;
      const float2 A = x[f * M + q], B = x[f * M + q + s];
      y[f * M + q] = ms_add(A, B);
      y[f * M + q + s] = ms_sub(A, B);
    }
    __syncthreads();
    float2* tmp = x; x = y; y = tmp;
  }

  // x: Z[k] of the half-length transform.  Magnitudes of the n_fft-point real transform into the free buffer, [MS_FR][2 M] floats
  float* magf = reinterpret_cast<float*>(y);
  for (int e = tid; e < MS_FR * NF; e += NT) {
    const int f = e / NF, k = e - f * NF;
    const float2 zk = x[f * M + (k & (M - 1))];
    float2 zm = x[f * M + ((M - k) & (M - 1))];
    zm.y = -zm.y;
    const float2 E = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
    const float2 O = make_float2(0.5f * (zk.y - zm.y), -0.5f * (zk.x - zm.x));
    const float2 X = ms_add(E, ms_cmul(a.twiddle[k], O));
    const float m = sqrtf(X.x * X.x + X.y * X.y);
    magf[f * 2 * M + k] = m;
    if (a.mag && s_n[f] > 0) a.mag[(gf0 + f) * NF + k] = m;
  }
  __syncthreads();

  for (int e = tid; e < MS_FR * a.num_mels; e += NT) {
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
  if (n_fft != 512 && n_fft != 1024 && n_fft != 2048 && n_fft != 4096) return false;
  if (win < 16 || win > n_fft) return false;
  if (hop < 1 || hop > n_fft) return false;
  return num_mels >= 1 && num_mels <= MS_MAX_MELS;
}

template <int N>
int ms_launch(const MsArgs& a, hipStream_t st) {
  const size_t lds = ms_lds(N);
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(melspec_k<N>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)ms_lds(N));
  if (attr != hipSuccess) return SATT_E_LAUNCH;
  const long long blocks = (a.total_frames + MS_FR - 1) / MS_FR;
  hipLaunchKernelGGL(melspec_k<N>, dim3((unsigned)blocks), dim3(ms_nt(N)), lds, st, a);
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
  if ((p->total_frames + MS_FR - 1) / MS_FR > 0x7fffffffLL) return SATT_E_UNSUPPORTED;
  MsArgs a{p->hop, p->num_mels, p->n_utts, p->n_band_weights, (long long)p->total_samples, (long long)p->total_frames,
           p->signal, p->sample_offsets, p->frame_offsets, p->window, reinterpret_cast<const float2*>(p->twiddle),
           p->band_start, p->band_offset, p->band_weight, p->ref_level_db, p->mel, p->mag};
  hipStream_t st = (hipStream_t)stream;
  switch (p->n_fft) {
    case 512: return ms_launch<512>(a, st);
    case 1024: return ms_launch<1024>(a, st);
    case 2048: return ms_launch<2048>(a, st);
    default: return ms_launch<4096>(a, st);
  }
}
