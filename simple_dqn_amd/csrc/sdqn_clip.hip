// sdqn_clip.hip — global gradient-norm clipping, --clip_grad_norm (interface and semantics: sdqn_clip.h).
// Both kernels walk g the same way: CLIP_GRID workgroups of 256 threads, 16-byte loads, thread (bid, t) takes the vectors
// bid * 256 + t + k * (CLIP_GRID * 256), four of them issued together per round trip (clamped index + select, as update_body.h's slab
// loop: no data-dependent trip count in front of the loads); the n % (16 / sizeof(T)) values behind the last whole vector belong to the
// first threads of workgroup 0.  No atomics, no scratch; the reduction's shape depends on n alone.
#include "sdqn_clip.h"
#include "launch.h"

namespace sdqn {
namespace {

constexpr int CLIP_THREADS = 256, CLIP_INFLIGHT = 4;
template <typename T> struct alignas(16) Vec16 { T v[16 / sizeof(T)]; };

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }          // one rounding, never part of an FMA
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
// sum over the wave's 64 lanes, every lane receives it (a + b == b + a: both lanes of a pair compute the same bits)
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

template <typename T>
__global__ void __launch_bounds__(CLIP_THREADS) grad_sqnorm_kernel(const T* __restrict__ g, const int64_t n, double* __restrict__ part) {
  constexpr int V = 16 / sizeof(T);
  __shared__ double wsum[CLIP_THREADS / 64];
  const int t = threadIdx.x;
  const int64_t nv = n / V, stride = (int64_t)gridDim.x * CLIP_THREADS;
  const Vec16<T>* gv = reinterpret_cast<const Vec16<T>*>(g);
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * CLIP_THREADS + t; i < nv; i += CLIP_INFLIGHT * stride) {
    Vec16<T> x[CLIP_INFLIGHT];
#pragma unroll
    for (int j = 0; j < CLIP_INFLIGHT; ++j) { const int64_t ij = i + j * stride; x[j] = gv[ij < nv ? ij : nv - 1]; }   // < nv: inside g
#pragma unroll
    for (int j = 0; j < CLIP_INFLIGHT; ++j)
      if (i + j * stride < nv) {
#pragma unroll
        for (int k = 0; k < V; ++k) { const double d = (double)x[j].v[k]; acc += d * d; }
      }
  }
  if (blockIdx.x == 0 && t < (int)(n - nv * V)) { const double d = (double)g[nv * V + t]; acc += d * d; }              // < n
  acc = wave_sum(acc);
  if ((t & 63) == 0) wsum[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    double s = wsum[0];
#pragma unroll
    for (int w = 1; w < CLIP_THREADS / 64; ++w) s += wsum[w];                                      // fixed order
    part[blockIdx.x] = s;
  }
}

template <typename T>
__global__ void __launch_bounds__(CLIP_THREADS) grad_scale_kernel(T* __restrict__ g, const int64_t n, const double* __restrict__ part,
                                                                  const double bsz, const double max_norm, double* __restrict__ rec) {
  constexpr int V = 16 / sizeof(T);
  static_assert(CLIP_GRID == 4 * 64, "a wave folds the partials four per lane");
  const int t = threadIdx.x, lane = t & 63;
  // every wave of every workgroup folds all CLIP_GRID partials the same way: four per lane in index order, then the butterfly
  const double p0 = part[lane], p1 = part[64 + lane], p2 = part[128 + lane], p3 = part[192 + lane];
  const double sq = wave_sum(((p0 + p1) + p2) + p3);
  const double norm = sqrt(sq) / bsz;
  double sc64 = 1.0;
  if (isfinite(norm)) { const double r = max_norm / (norm + CLIP_EPS); sc64 = r < 1.0 ? r : 1.0; }
  const T sc = (T)sc64;                                                                            // rounded once to the net's precision
  if (blockIdx.x == 0 && t == 0) { rec[0] = norm; rec[1] = (double)sc; }
  if (!(sc < (T)1)) return;                                                                        // nothing to clip: g keeps its bits
  const int64_t nv = n / V, stride = (int64_t)gridDim.x * CLIP_THREADS;
  Vec16<T>* gv = reinterpret_cast<Vec16<T>*>(g);
  for (int64_t i = (int64_t)blockIdx.x * CLIP_THREADS + t; i < nv; i += CLIP_INFLIGHT * stride) {
    Vec16<T> x[CLIP_INFLIGHT];
#pragma unroll
    for (int j = 0; j < CLIP_INFLIGHT; ++j) { const int64_t ij = i + j * stride; x[j] = gv[ij < nv ? ij : nv - 1]; }
#pragma unroll
    for (int j = 0; j < CLIP_INFLIGHT; ++j)
      if (i + j * stride < nv) {                                                                   // each vector has ONE owner: no clamped store
#pragma unroll
        for (int k = 0; k < V; ++k) x[j].v[k] = mul_rn(x[j].v[k], sc);
        gv[i + j * stride] = x[j];
      }
  }
  if (blockIdx.x == 0 && t < (int)(n - nv * V)) g[nv * V + t] = mul_rn(g[nv * V + t], sc);
}

bool clip_args_ok(const void* g, int64_t n, const void* part) { return g && part && n > 0 && (reinterpret_cast<uintptr_t>(g) & 15) == 0; }

}  // namespace

template <typename T> hipError_t launch_grad_sqnorm(const T* g, int64_t n, double* part, hipStream_t s) {
  if (!clip_args_ok(g, n, part)) return hipErrorInvalidValue;
  SDQN_LAUNCH(grad_sqnorm_kernel<T>, dim3(CLIP_GRID), dim3(CLIP_THREADS), 0, s, g, n, part);
  return hipGetLastError();
}
template <typename T> hipError_t launch_grad_scale(T* g, int64_t n, const double* part, double bsz, double max_norm, double* rec, hipStream_t s) {
  if (!clip_args_ok(g, n, part) || !rec || !(bsz > 0.0) || !(max_norm > 0.0)) return hipErrorInvalidValue;
  SDQN_LAUNCH(grad_scale_kernel<T>, dim3(CLIP_GRID), dim3(CLIP_THREADS), 0, s, g, n, part, bsz, max_norm, rec);
  return hipGetLastError();
}
template hipError_t launch_grad_sqnorm<float>(const float*, int64_t, double*, hipStream_t);
template hipError_t launch_grad_sqnorm<double>(const double*, int64_t, double*, hipStream_t);
template hipError_t launch_grad_scale<float>(float*, int64_t, const double*, double, double, double*, hipStream_t);
template hipError_t launch_grad_scale<double>(double*, int64_t, const double*, double, double, double*, hipStream_t);

}  // namespace sdqn
