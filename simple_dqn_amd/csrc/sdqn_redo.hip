// sdqn_redo.hip — dormant-neuron recycling (--redo_interval): the kernels.  The rules — score, draw, index maps — are redo.h's.
//   redo_partial_kernel   first stage of the column reduction: one workgroup per redo_chunk(l) rows of one layer's activation matrix.  A thread
//                         owns one 16-byte piece of a row (4 floats / 8 halves) and walks the chunk's rows 256 / pieces-per-row apart, adding
//                         |a| in fp64; the workgroup's row lanes are then folded in LDS by halving (lane r += lane r + s, s = lanes/2 .. 1).
//                         Leaves [blocks][units] partial sums per layer.
//   redo_finish_kernel    second stage, one workgroup per layer: a thread per unit adds the layer's partials in block order, divides by the row
//                         count, the layer sum is folded by halving in LDS; leaves the 672 scores.
//   redo_apply_kernel     walks the flat weight buffer by 16-byte pieces: every entry decides from the scores whether it is redrawn, zeroed or
//                         kept (redo_action); a piece with no such entry is not written.  Workgroup 0 also leaves the event's record.
// No atomics; which thread adds what is a function of the batch size alone, so two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "problems.h"
#include "redo.h"
#include "launch.h"

namespace sdqn {

static_assert(redo_pix(0) == PIX1 && redo_pix(1) == PIX2 && redo_pix(2) == PIX3, "rows per sample");

namespace {

typedef float redo_f4 __attribute__((ext_vector_type(4)));

// T: float | half_t.  C: units (columns).  a: [rows][C], 16-byte aligned rows.  out: [C] the chunk's sums.  sh: [8][256] doubles
template <typename T, int C>
__device__ __forceinline__ void partial_cols(const T* a, int64_t rows, int chunk, int chunk_rows, double* out, double* sh) {
  constexpr int V = 16 / (int)sizeof(T), G = C / V, RP = 256 / G;      // values per piece, pieces per row, row lanes
  static_assert(G * RP == 256 && RP >= 2 && V <= 8, "a workgroup covers whole rows");
  const int tid = threadIdx.x, g = tid % G, rr = tid / G;
  const int64_t r0 = (int64_t)chunk * chunk_rows, r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
  double acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.0;
  for (int64_t r = r0 + rr; r < r1; r += RP) {                       // r < rows: inside the matrix
    const T* p = a + r * C + g * V;
    if constexpr (sizeof(T) == 4) {
      const redo_f4 x = *reinterpret_cast<const redo_f4*>(p);
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[v] = acc[v] + fabs((double)x[v]);
    } else {
      const half8 x = *reinterpret_cast<const half8*>(p);
#pragma unroll
      for (int v = 0; v < 8; ++v) acc[v] = acc[v] + fabs((double)(float)x[v]);
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) sh[v * 256 + tid] = acc[v];
  __syncthreads();
  for (int s = RP / 2; s >= 1; s >>= 1) {
    if (rr < s) {
#pragma unroll
      for (int v = 0; v < V; ++v) sh[v * 256 + tid] = sh[v * 256 + tid] + sh[v * 256 + tid + s * G];      // (lane rr + s of the same piece)
    }
    __syncthreads();
  }
  if (rr == 0) {
#pragma unroll
    for (int v = 0; v < V; ++v) out[g * V + v] = sh[v * 256 + tid];
  }
}

__global__ void __launch_bounds__(256) redo_partial_kernel(const RedoScoreArgs a) {
  __shared__ double sh[8 * 256];
  int b = blockIdx.x, l = 0;
  double* out = a.partial;
  while (l < REDO_LAYERS - 1 && b >= redo_blocks(l, a.B)) { b -= redo_blocks(l, a.B); out += (int64_t)redo_blocks(l, a.B) * relu_units(l); ++l; }
  out += (int64_t)b * relu_units(l);
  const int64_t rows = (int64_t)a.B * redo_pix(l);
  if (l == 3) { partial_cols<float, NFC>(static_cast<const float*>(a.a[3]), rows, b, redo_chunk(3), out, sh); return; }
  if (a.half123) {
    if (l == 0) partial_cols<half_t, K1>(static_cast<const half_t*>(a.a[0]), rows, b, redo_chunk(0), out, sh);
    else partial_cols<half_t, K2>(static_cast<const half_t*>(a.a[l]), rows, b, redo_chunk(l), out, sh);
  } else {
    if (l == 0) partial_cols<float, K1>(static_cast<const float*>(a.a[0]), rows, b, redo_chunk(0), out, sh);
    else partial_cols<float, K2>(static_cast<const float*>(a.a[l]), rows, b, redo_chunk(l), out, sh);
  }
}
static_assert(K2 == K3, "conv2 and conv3 share an instantiation");

__global__ void __launch_bounds__(512) redo_finish_kernel(const RedoScoreArgs a) {
  __shared__ double sh[512];
  const int l = blockIdx.x, n = relu_units(l), j = threadIdx.x, nb = redo_blocks(l, a.B);
  const double* part = a.partial;
  for (int k = 0; k < l; ++k) part += (int64_t)redo_blocks(k, a.B) * relu_units(k);
  double m = 0.0;
  if (j < n) {
    for (int b = 0; b < nb; ++b) m = m + part[(int64_t)b * n + j];
    m = m / (double)((int64_t)a.B * redo_pix(l));
  }
  sh[j] = m;
  __syncthreads();
  for (int s = n / 2; s >= 1; s >>= 1) {
    if (j < s) sh[j] = sh[j] + sh[j + s];
    __syncthreads();
  }
  const double mean = sh[0] / (double)n;
  if (j < n) a.scores[relu_off(l) + j] = mean > 0.0 ? (float)(m / mean) : 0.0f;
}

__global__ void __launch_bounds__(256) redo_apply_kernel(const RedoApplyArgs a) {
  __shared__ float sc[RELU_UNITS];
  for (int k = threadIdx.x; k < RELU_UNITS; k += 256) sc[k] = a.scores[k];
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < REDO_LAYERS) {
    const int l = threadIdx.x;
    int64_t c = 0;
    for (int k = relu_off(l); k < relu_off(l + 1); ++k) c += redo_dormant(sc[k], a.tau) ? 1 : 0;
    a.info[2 + l] = c;
    if (l == 0) { a.info[0] = (int64_t)a.event; a.info[1] = a.step; }
  }
  const uint64_t key = redo_key(a.seed, a.event);
  const int64_t n4 = a.n >> 2;                                         // (the launcher has checked n % 4 == 0)
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n4; p += (int64_t)gridDim.x * 256) {
    const int64_t i0 = p * 4;                                          // i0 + 3 < n
    int act[4]; int any = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) { act[v] = redo_action(sc, a.tau, redo_entry(i0 + v)); any |= act[v]; }
    if (!any) continue;
    redo_f4 w = *reinterpret_cast<const redo_f4*>(a.theta + i0);
    redo_f4 s1 = *reinterpret_cast<const redo_f4*>(a.state + i0);
    redo_f4 s2 = a.state2 ? *reinterpret_cast<const redo_f4*>(a.state2 + i0) : redo_f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int v = 0; v < 4; ++v) if (act[v]) {
      w[v] = act[v] == 1 ? redo_draw(key, (uint64_t)(i0 + v), redo_entry(i0 + v).L) : 0.0f;
      s1[v] = 0.0f; s2[v] = 0.0f;
    }
    *reinterpret_cast<redo_f4*>(a.theta + i0) = w;
    *reinterpret_cast<redo_f4*>(a.state + i0) = s1;
    if (a.state2) *reinterpret_cast<redo_f4*>(a.state2 + i0) = s2;
  }
}

}  // namespace

// stage 0: the partial sums, stage 1: the scores from them (two launches, in this order on one stream)
hipError_t launch_redo_scores(const RedoScoreArgs& a, int stage, hipStream_t s) {
  if (a.B <= 0 || !a.partial || !a.scores) return hipErrorInvalidValue;
  for (int l = 0; l < REDO_LAYERS; ++l) if (!a.a[l]) return hipErrorInvalidValue;
  if (stage == 0) {
    int blocks = 0;
    for (int l = 0; l < REDO_LAYERS; ++l) blocks += redo_blocks(l, a.B);
    SDQN_LAUNCH(redo_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  } else SDQN_LAUNCH(redo_finish_kernel, dim3(REDO_LAYERS), dim3(512), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_redo_apply(const RedoApplyArgs& a, hipStream_t s) {
  if (a.n < OFF5 || (a.n & 3) || !a.scores || !a.theta || !a.state || !a.info) return hipErrorInvalidValue;
  int64_t blocks = ((a.n >> 2) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  SDQN_LAUNCH(redo_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sdqn
