// The short-time Fourier transform core of melspec.hip and griffin_lim.hip: 4 frames a workgroup, an FFT held in LDS.
//   * real input through a half-length complex transform: z[j] = x[2j] + i x[2j+1], M = n_fft / 2 points;
//   * Stockham autosort, radix 4 (decimation in frequency) with one radix-2 stage behind it when log2 M is odd: every stage reads
//     one LDS buffer and writes the other, no bit reversal.  Stage (n, s), n s = M: butterfly t = p s + q reads
//     x[q + s (p + c n/4)] and writes y[q + s (4 p + c)], c = 0..3, twiddles w^(c p s) from the M-th roots kept in LDS;
//   * X[k] = E[k] + exp(-2 pi i k / n_fft) O[k] from Z[k] and conj(Z[M - k]), the n_fft-th roots read from global memory.
// LDS: [4][M] x | [4][M] y | [M] twiddles | 16 slot words = (2 x 4 + 1) M float2 = 144 KiB at n_fft = 4096, 72 KiB at 2048.
//
// LDS banks (8-byte accesses: 32 lanes a group on reads, 16 contiguous lanes on writes): with s >= 16 lanes of a group differ in q
// alone, so reads and writes are unit-stride and conflict-free.  The stages with s = 1 and s = 4 read unit-stride (in p resp. in
// (p, q)) but write with a stride of 4 s float2: with s = 1 the four outputs of a butterfly are adjacent (32 bytes per lane, wide
// stores), with s = 4 a group of 16 lanes writes 4 runs of 4 float2 - the one stage that pays store conflicts.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int STFT_FR = 4;              // frames per workgroup

constexpr int stft_nt(int N) { return N >= 4096 ? 1024 : (N >= 2048 ? 512 : 256); }
inline size_t stft_lds(int N) { return (size_t)(2 * STFT_FR + 1) * (N / 2) * sizeof(float2) + 4 * STFT_FR * sizeof(long long); }

__device__ __forceinline__ float2 stft_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 stft_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 stft_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

struct StftLds {
  float2 *x, *y;                        // [STFT_FR][M] each
  float2* tw;                           // [M]: exp(-2 pi i j / M)
  long long* slot;                      // 4 STFT_FR words of the caller's
};

// the carve of the dynamic LDS (16-byte aligned, stft_lds(N) bytes) and the twiddle preload; the caller's barrier publishes it
template <int N>
__device__ __forceinline__ StftLds stft_carve(char* smem, const float2* twiddle, int tid) {
  constexpr int M = N / 2;
  StftLds l;
  l.x = reinterpret_cast<float2*>(smem);
  l.y = l.x + STFT_FR * M;
  l.tw = l.y + STFT_FR * M;
  l.slot = reinterpret_cast<long long*>(l.tw + M);
  for (int j = tid; j < M; j += stft_nt(N)) l.tw[j] = twiddle[2 * j];
  return l;
}

// the last utterance whose first frame is <= gf
__device__ __forceinline__ int stft_utt(const int64_t* frame_offsets, int n_utts, long long gf) {
  int lo = 0, hi = n_utts;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (frame_offsets[mid] <= gf) lo = mid; else hi = mid;
  }
  return lo;
}

// signal index of position i of a reflect-centred frame (padded position i + n_fft / 2), reflected once at either end:
// n >= n_fft / 2 + 1 and t hop <= n keep it inside [0, n)
template <class I>
__device__ __forceinline__ I stft_reflect(I i, I n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// M-point complex transform of the STFT_FR frames held in x, behind a barrier.  On return x holds the result and y is free.
template <int N>
__device__ __forceinline__ void stft_fft(float2*& x, float2*& y, const float2* tw, int tid) {
  constexpr int M = N / 2, NT = stft_nt(N), NB = M / 4;
#pragma unroll
  for (int n = M, s = 1; n >= 4; n >>= 2, s <<= 2) {
    const int n1 = n >> 2;
    for (int e = tid; e < STFT_FR * NB; e += NT) {
      const int f = e / NB, t = e - f * NB, p = t / s, q = t - p * s;
      const float2* xf = x + f * M;
      float2* yf = y + f * M;
      const float2 A = xf[q + s * p], B = xf[q + s * (p + n1)], C = xf[q + s * (p + 2 * n1)], D = xf[q + s * (p + 3 * n1)];
      const float2 apc = stft_add(A, C), amc = stft_sub(A, C), bpd = stft_add(B, D), bmd = stft_sub(B, D);
      const float2 jbmd = make_float2(-bmd.y, bmd.x);
      const float2 w1 = tw[p * s], w2 = tw[2 * p * s], w3 = tw[3 * p * s];
      yf[q + s * (4 * p)] = stft_add(apc, bpd);
      yf[q + s * (4 * p + 1)] = stft_cmul(w1, stft_sub(amc, jbmd));
      yf[q + s * (4 * p + 2)] = stft_cmul(w2, stft_sub(apc, bpd));
      yf[q + s * (4 * p + 3)] = stft_cmul(w3, stft_add(amc, jbmd));
    }
    __syncthreads();
    float2* tmp = x; x = y; y = tmp;
  }
  constexpr bool ODD = M == 512 || M == 2048;               // log2 M odd (n_fft 1024 and 4096): a radix-2 stage is left, s = M / 2
  if (ODD) {
    constexpr int s = M / 2;
    for (int e = tid; e < STFT_FR * s; e += NT) {
      const int f = e / s, q = e - f * s;
      const float2 A = x[f * M + q], B = x[f * M + q + s];
      y[f * M + q] = stft_add(A, B);
      y[f * M + q + s] = stft_sub(A, B);
    }
    __syncthreads();
    float2* tmp = x; x = y; y = tmp;
  }
}

// bin k <= M of the n_fft-point real transform of one frame from its half-length transform Z [M]; twiddle: the n_fft-th roots
template <int N>
__device__ __forceinline__ float2 stft_bin(const float2* Z, const float2* twiddle, int k) {
  constexpr int M = N / 2;
  const float2 zk = Z[k & (M - 1)];
  float2 zm = Z[(M - k) & (M - 1)];
  zm.y = -zm.y;
  const float2 E = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y + zm.y));
  const float2 O = make_float2(0.5f * (zk.y - zm.y), -0.5f * (zk.x - zm.x));
  return stft_add(E, stft_cmul(twiddle[k], O));
}

inline bool stft_supported(int n_fft, int win) {
  if (n_fft != 512 && n_fft != 1024 && n_fft != 2048 && n_fft != 4096) return false;
  return win >= 16 && win <= n_fft;
}

// f(std::integral_constant<int, n_fft>) of a supported n_fft
template <class F>
int stft_dispatch(int n_fft, F f) {
  switch (n_fft) {
    case 512: return f(std::integral_constant<int, 512>());
    case 1024: return f(std::integral_constant<int, 1024>());
    case 2048: return f(std::integral_constant<int, 2048>());
    default: return f(std::integral_constant<int, 4096>());
  }
}

// raises the dynamic LDS limit of kernel K to stft_lds(N), once a process
template <auto K, int N>
bool stft_lds_limit() {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)stft_lds(N));
  return attr == hipSuccess;
}

}  // namespace
