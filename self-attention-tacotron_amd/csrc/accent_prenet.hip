// Accent-type branch of SelfAttentionCBHGEncoderWithAccentType (reference modules/module.py:444-527, models/models.py:285-288,
// :361-364): accent_embedding[id - offset] -> PreNet stack (Dense, ReLU, dropout; 1 or 2 layers) -> columns [col0, col0 + Wa) of the
// pre-net output buffer the phoneme branch shares (no concatenation copy).  The branch is tiny per row (id -> 32 -> 32 -> 16 floats,
// 1 584 weights at the shipped sizes) and sits in the launch-bound part of the step, so forward and backward are ONE launch each:
// every weight and bias lives in LDS, a workgroup carries a tile of rows through all layers.  fp32 FMA throughout (MFMA buys nothing
// at K <= 64, and the f32 parity mode compares against float64 at 2e-4).
//
// LDS discipline: every word that is read was written by the same launch (weights, biases, whole activation tiles including the rows
// past the end of the batch, the whole table-gradient accumulator) - tests run this under SATT_DEBUG_POISON_LDS.
#include "common.h"

namespace {

constexpr int AP_NT = 256;          // threads per workgroup
constexpr int AP_MAXW = 64;         // cap of the embedding width and of every layer width
constexpr int AP_FWD_ROWS = 16;     // rows per workgroup, forward (5120 rows -> 320 workgroups)
constexpr int AP_BWD_ROWS = 64;     // rows per workgroup, backward (fewer workgroups = fewer atomics per weight element)
constexpr int AP_LDS_MAX = 64 * 1024;

struct ApArgs {
  const int64_t* ids; const float* table; int ntypes, offset, dim;
  const float* W0; const float* b0; int n0;
  const float* W1; const float* b1; int n1;     // n1 == 0: one layer
  int rows;
  uint32_t thresh; float scale; uint32_t stream0, stream1; const uint32_t* seed;
};

// LDS weight rows are padded to an odd stride: W[k][c] is read along c by the forward products and along k by the input
// gradients - both conflict-free
__device__ __forceinline__ int ap_ws(int n) { return n | 1; }

__host__ __device__ inline int ap_weight_floats(int dim, int n0, int n1) {
  return dim * (n0 | 1) + n0 + (n1 > 0 ? n0 * (n1 | 1) + n1 : 0);
}

// weights and biases of all layers -> LDS (w0 | b0 | w1 | b1)
__device__ __forceinline__ void ap_load_weights(const ApArgs& a, float* w0, float* b0, float* w1, float* b1) {
  const int tid = threadIdx.x;
  for (int e = tid; e < a.dim * a.n0; e += AP_NT) { const int k = e / a.n0, c = e - k * a.n0; w0[k * ap_ws(a.n0) + c] = a.W0[e]; }
  for (int e = tid; e < a.n0; e += AP_NT) b0[e] = a.b0[e];
  if (a.n1 > 0) {
    for (int e = tid; e < a.n0 * a.n1; e += AP_NT) { const int k = e / a.n1, c = e - k * a.n1; w1[k * ap_ws(a.n1) + c] = a.W1[e]; }
    for (int e = tid; e < a.n1; e += AP_NT) b1[e] = a.b1[e];
  }
}

// table row of a token; ids outside the table are clamped (memory safety only: the input pipeline rejects or remaps them)
__device__ __forceinline__ int ap_row_of(const ApArgs& a, int r) {
  const int64_t v = a.ids[r] - a.offset;
  return (int)(v < 0 ? 0 : (v >= a.ntypes ? a.ntypes - 1 : v));
}

// one Dense + ReLU + dropout layer over a tile: y[r][c] = drop(relu(x[r][:] . W[:][c] + b[c])); rows >= nvalid are written as 0.
// Dropout element index = C-order index inside the layer's own [rows, N] output (oracle/rng.py keep_mask of a [B, Ti, N] tensor).
template <int TILE>
__device__ __forceinline__ void ap_layer(const float* x, int K, const float* W, const float* b, int N, float* y, int row0, int nvalid,
                                         uint32_t thresh, float scale, uint32_t stream, uint32_t seed) {
  const int ws = ap_ws(N);
  for (int e = threadIdx.x; e < TILE * N; e += AP_NT) {
    const int r = e / N, c = e - r * N;
    float acc = b[c];
    for (int k = 0; k < K; ++k) acc = fmaf(x[r * K + k], W[k * ws + c], acc);
    acc = fmaxf(acc, 0.f);
    if (thresh != 0) acc = satt_keep(seed, stream, (uint32_t)(row0 + r) * (uint32_t)N + (uint32_t)c, thresh) ? acc * scale : 0.f;
    y[e] = r < nvalid ? acc : 0.f;
  }
}

// gather of the embedding rows of a tile (rows >= nvalid: zeros)
template <int TILE>
__device__ __forceinline__ void ap_gather(const ApArgs& a, float* x, int row0, int nvalid) {
  for (int e = threadIdx.x; e < TILE * a.dim; e += AP_NT) {
    const int r = e / a.dim, k = e - r * a.dim;
    x[e] = r < nvalid ? a.table[(int64_t)ap_row_of(a, row0 + r) * a.dim + k] : 0.f;
  }
}

__global__ __launch_bounds__(AP_NT) void accent_prenet_fwd_k(ApArgs a, float* __restrict__ out, int64_t ldo) {
  extern __shared__ float lds[];
  float* w0 = lds; float* b0 = w0 + a.dim * ap_ws(a.n0);
  float* w1 = b0 + a.n0; float* b1 = w1 + (a.n1 > 0 ? a.n0 * ap_ws(a.n1) : 0);
  float* x0 = b1 + a.n1;                         // [TILE][dim]
  float* y0 = x0 + AP_FWD_ROWS * a.dim;          // [TILE][n0]
  float* y1 = y0 + AP_FWD_ROWS * a.n0;           // [TILE][n1]
  const int row0 = blockIdx.x * AP_FWD_ROWS, nvalid = min(AP_FWD_ROWS, a.rows - row0);
  const uint32_t seed = (a.thresh != 0 && a.seed) ? *a.seed : 0u;
  ap_load_weights(a, w0, b0, w1, b1);
  ap_gather<AP_FWD_ROWS>(a, x0, row0, nvalid);
  __syncthreads();
  ap_layer<AP_FWD_ROWS>(x0, a.dim, w0, b0, a.n0, y0, row0, nvalid, a.thresh, a.scale, a.stream0, seed);
  __syncthreads();
  const float* y = y0; int N = a.n0;
  if (a.n1 > 0) {
    ap_layer<AP_FWD_ROWS>(y0, a.n0, w1, b1, a.n1, y1, row0, nvalid, a.thresh, a.scale, a.stream1, seed);
    __syncthreads();
    y = y1; N = a.n1;
  }
  for (int e = threadIdx.x; e < nvalid * N; e += AP_NT) {
    const int r = e / N, c = e - r * N;
    out[(int64_t)(row0 + r) * ldo + c] = y[e];
  }
}

// dW[k][c] += sum_r x[r][k] * dz[r][c], db[c] += sum_r dz[r][c]: a thread owns an element, sums the tile's rows in order and adds the
// workgroup's partial sum to the flat gradient with ONE float atomic (the project's convention: steps reproducible to rounding)
template <int TILE>
__device__ __forceinline__ void ap_dw(const float* x, int K, const float* dz, int N, float* dW, float* db) {
  for (int e = threadIdx.x; e < (K + 1) * N; e += AP_NT) {
    const int k = e / N, c = e - k * N;
    float acc = 0.f;
    if (k < K) { for (int r = 0; r < TILE; ++r) acc = fmaf(x[r * K + k], dz[r * N + c], acc); }
    else       { for (int r = 0; r < TILE; ++r) acc += dz[r * N + c]; }
    // an exact zero adds nothing: skip the atomic (whole columns are zero where ReLU / dropout cut every row of the tile)
    if (acc != 0.f) atomicAdd(k < K ? &dW[k * N + c] : &db[c], acc);
  }
}

// dx[r][k] = sum_c dz[r][c] * W[k][c]
template <int TILE>
__device__ __forceinline__ void ap_dx(const float* dz, int N, const float* W, int K, float* dx) {
  const int ws = ap_ws(N);
  for (int e = threadIdx.x; e < TILE * K; e += AP_NT) {
    const int r = e / K, k = e - r * K;
    float acc = 0.f;
    for (int c = 0; c < N; ++c) acc = fmaf(dz[r * N + c], W[k * ws + c], acc);
    dx[e] = acc;
  }
}

// Backward of the whole branch in one launch.  The forward activations are recomputed from the ids (cheaper than saving them).  Many
// tokens share few accent ids: the table-row gradients of a tile are summed in an LDS copy of the table gradient (LDS float atomics)
// and only the rows the tile touched go to global memory - one atomic per element and workgroup instead of one per token.
__global__ __launch_bounds__(AP_NT) void accent_prenet_bwd_k(ApArgs a, const float* __restrict__ dout, int64_t ldd,
                                                             float* __restrict__ dtable, float* __restrict__ dW0,
                                                             float* __restrict__ db0, float* __restrict__ dW1,
                                                             float* __restrict__ db1) {
  extern __shared__ float lds[];
  constexpr int T = AP_BWD_ROWS;
  float* w0 = lds; float* b0 = w0 + a.dim * ap_ws(a.n0);
  float* w1 = b0 + a.n0; float* b1 = w1 + (a.n1 > 0 ? a.n0 * ap_ws(a.n1) : 0);
  float* x0 = b1 + a.n1;                         // [T][dim]   embedding rows
  float* y0 = x0 + T * a.dim;                    // [T][n0]    layer-0 output
  float* y1 = y0 + T * a.n0;                     // [T][n1]    layer-1 output (n1 > 0)
  float* g = y1 + T * a.n1;                      // [T][max(dim, n0)]  gradient scratch
  float* dT = g + T * max(a.dim, a.n0);          // [ntypes][dim]  table-gradient accumulator
  int* touched = reinterpret_cast<int*>(dT + a.ntypes * a.dim);      // [ntypes]
  const int row0 = blockIdx.x * T, nvalid = min(T, a.rows - row0);
  const uint32_t seed = (a.thresh != 0 && a.seed) ? *a.seed : 0u;
  ap_load_weights(a, w0, b0, w1, b1);
  ap_gather<T>(a, x0, row0, nvalid);
  for (int e = threadIdx.x; e < a.ntypes * a.dim; e += AP_NT) dT[e] = 0.f;
  for (int e = threadIdx.x; e < a.ntypes; e += AP_NT) touched[e] = 0;
  __syncthreads();
  ap_layer<T>(x0, a.dim, w0, b0, a.n0, y0, row0, nvalid, a.thresh, a.scale, a.stream0, seed);
  __syncthreads();
  if (a.n1 > 0) {
    ap_layer<T>(y0, a.n0, w1, b1, a.n1, y1, row0, nvalid, a.thresh, a.scale, a.stream1, seed);
    __syncthreads();
    // dz1 = dout * relu'(y1) * scale (in place of y1: a dropped or clipped unit has y1 == 0)
    for (int e = threadIdx.x; e < T * a.n1; e += AP_NT) {
      const int r = e / a.n1, c = e - r * a.n1;
      y1[e] = (r < nvalid && y1[e] > 0.f) ? dout[(int64_t)(row0 + r) * ldd + c] * a.scale : 0.f;
    }
    __syncthreads();
    ap_dw<T>(y0, a.n0, y1, a.n1, dW1, db1);
    ap_dx<T>(y1, a.n1, w1, a.n0, g);             // d y0
    __syncthreads();
    for (int e = threadIdx.x; e < T * a.n0; e += AP_NT) y0[e] = y0[e] > 0.f ? g[e] * a.scale : 0.f;      // dz0 in place of y0
  } else {
    for (int e = threadIdx.x; e < T * a.n0; e += AP_NT) {
      const int r = e / a.n0, c = e - r * a.n0;
      y0[e] = (r < nvalid && y0[e] > 0.f) ? dout[(int64_t)(row0 + r) * ldd + c] * a.scale : 0.f;
    }
  }
  __syncthreads();
  ap_dw<T>(x0, a.dim, y0, a.n0, dW0, db0);
  ap_dx<T>(y0, a.n0, w0, a.dim, g);              // gradient of the embedding rows
  __syncthreads();
  for (int e = threadIdx.x; e < nvalid * a.dim; e += AP_NT) {
    const int r = e / a.dim, k = e - r * a.dim, row = ap_row_of(a, row0 + r);
    atomicAdd(&dT[row * a.dim + k], g[e]);
    if (k == 0) touched[row] = 1;        // several rows of the tile may share `row`: they all store the same 1 (benign race)
  }
  __syncthreads();
  for (int e = threadIdx.x; e < a.ntypes * a.dim; e += AP_NT)
    if (touched[e / a.dim]) atomicAdd(&dtable[e], dT[e]);
}

inline bool ap_shape_ok(int ntypes, int dim, int nlayers, int n0, int n1) {
  if (nlayers < 1 || nlayers > 2) return false;
  if (dim > AP_MAXW || n0 > AP_MAXW || (nlayers == 2 && n1 > AP_MAXW)) return false;
  return ntypes >= 1;
}
inline size_t ap_fwd_lds(int dim, int n0, int n1) {
  return sizeof(float) * (size_t)(ap_weight_floats(dim, n0, n1) + AP_FWD_ROWS * (dim + n0 + n1));
}
inline size_t ap_bwd_lds(int ntypes, int dim, int n0, int n1) {
  return sizeof(float) * (size_t)(ap_weight_floats(dim, n0, n1) + AP_BWD_ROWS * (dim + n0 + n1 + (dim > n0 ? dim : n0)) +
                                  (size_t)ntypes * dim + ntypes);
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int satt_accent_prenet_fwd(const int64_t* ids, const float* table, int ntypes, int offset, int dim, int nlayers,
                                      const float* W0, const float* b0, int n0, const float* W1, const float* b1, int n1,
                                      float* out, int64_t ldo, int rows, uint32_t drop_thresh, float drop_scale, uint32_t stream0,
                                      uint32_t stream1, const uint32_t* seed, void* stream) {
  if (rows <= 0) return SATT_OK;
  if (!ids || !table || !W0 || !b0 || !out || dim <= 0 || n0 <= 0 || (nlayers == 2 && (!W1 || !b1 || n1 <= 0))) return SATT_E_BADARG;
  if (nlayers != 2) n1 = 0;
  if (ldo < (n1 > 0 ? n1 : n0)) return SATT_E_BADARG;
  if (!ap_shape_ok(ntypes, dim, nlayers, n0, n1) || ap_fwd_lds(dim, n0, n1) > (size_t)AP_LDS_MAX) return SATT_E_UNSUPPORTED;
  ApArgs a{ids, table, ntypes, offset, dim, W0, b0, n0, W1, b1, n1, rows, drop_thresh, drop_scale, stream0, stream1, seed};
  hipLaunchKernelGGL(accent_prenet_fwd_k, dim3((rows + AP_FWD_ROWS - 1) / AP_FWD_ROWS), dim3(AP_NT), ap_fwd_lds(dim, n0, n1), S_, a,
                     out, ldo);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}

extern "C" int satt_accent_prenet_bwd(const int64_t* ids, const float* table, int ntypes, int offset, int dim, int nlayers,
                                      const float* W0, const float* b0, int n0, const float* W1, const float* b1, int n1,
                                      const float* dout, int64_t ldd, int rows, uint32_t drop_thresh, float drop_scale,
                                      uint32_t stream0, uint32_t stream1, const uint32_t* seed, float* dtable, float* dW0, float* db0,
                                      float* dW1, float* db1, void* stream) {
  if (rows <= 0) return SATT_OK;
  if (!ids || !table || !W0 || !b0 || !dout || !dtable || !dW0 || !db0 || dim <= 0 || n0 <= 0 ||
      (nlayers == 2 && (!W1 || !b1 || !dW1 || !db1 || n1 <= 0))) return SATT_E_BADARG;
  if (nlayers != 2) n1 = 0;
  if (ldd < (n1 > 0 ? n1 : n0)) return SATT_E_BADARG;
  if (!ap_shape_ok(ntypes, dim, nlayers, n0, n1) || ap_bwd_lds(ntypes, dim, n0, n1) > (size_t)AP_LDS_MAX) return SATT_E_UNSUPPORTED;
  ApArgs a{ids, table, ntypes, offset, dim, W0, b0, n0, W1, b1, n1, rows, drop_thresh, drop_scale, stream0, stream1, seed};
  hipLaunchKernelGGL(accent_prenet_bwd_k, dim3((rows + AP_BWD_ROWS - 1) / AP_BWD_ROWS), dim3(AP_NT),
                     ap_bwd_lds(ntypes, dim, n0, n1), S_, a, dout, ldd, dtable, dW0, db0, dW1, db1);
  SATT_LAUNCH_CHECK(); return SATT_OK;
}
