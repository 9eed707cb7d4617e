// sdqn_noisy.hip — --noisy_nets (the noise: noisy.h): factorised Gaussian noise on fc4 and fc5.
//   noisy_compose : the effective flat buffers the step's kernels read as StepArgs::theta.  conv slices: copied; fc4 / fc5:
//                   W = mu + sigma * (e_out * e_in), each operation rounded once.  Every workgroup regenerates its net's four factor
//                   vectors from the counter into LDS (4192 values, no hand-off between workgroups); workgroup 0 of a net also leaves
//                   them in the device buffer the tail and sdqn_net_debug_read "noisy_eps" read.
//   noisy_tail    : between update modes 1 and 2: g_sigma = g * (e_out * e_in) on the fc4 / fc5 range of the flat gradient sums, and
//                   the net's optimizer rule (kernels.h: opt_apply) on sigma with optimizer state of its own.
// Both walk their range grid-stride with 16-byte loads and stores; fc4 lies pixel-major in the flat buffers (noisy_fc4_input).
#include "kernels.h"
#include "noisy.h"

namespace sdqn {
namespace {

static_assert(K3 == 64 && PIX3 == 49, "noisy_fc4_input");
static_assert(MAX_ACTIONS <= NOISY_OUT5_PAD && OFF4 % 4 == 0 && OFF5 % 4 == 0 && NOISY_EPS_OUT4 % 4 == 0 && NOISY_EPS_IN5 % 4 == 0, "16-byte pieces");
constexpr int NOISY_THREADS = 256, NOISY_GRID = 512;

__device__ __forceinline__ float4 mul4(const float4& a, float b) { return make_float4(__fmul_rn(a.x, b), __fmul_rn(a.y, b), __fmul_rn(a.z, b), __fmul_rn(a.w, b)); }
__device__ __forceinline__ float4 mul4(const float4& a, const float4& b) { return make_float4(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y), __fmul_rn(a.z, b.z), __fmul_rn(a.w, b.w)); }
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w)); }
// e_out * e_in of the four consecutive values at offset r (a multiple of 4) of the fc range [fc4 | fc5]; sh: one net's factor vectors
__device__ __forceinline__ float4 factor4(const float* sh, int64_t r) {
  if (r < NW4) {                                     // row k of the internal layout, units u .. u + 3
    const int k = (int)(r >> 9), u = (int)(r & 511);
    return mul4(*reinterpret_cast<const float4*>(sh + NOISY_EPS_OUT4 + u), sh[NOISY_EPS_IN4 + noisy_fc4_input(k)]);
  }
  const int r5 = (int)(r - NW4), act = r5 >> 9, j = r5 & 511;          // output `act`, hidden units j .. j + 3
  return mul4(*reinterpret_cast<const float4*>(sh + NOISY_EPS_IN5 + j), sh[NOISY_EPS_OUT5 + act]);
}

__global__ void __launch_bounds__(NOISY_THREADS) noisy_compose_kernel(const NoisyArgs a) {
  __shared__ alignas(16) float sh[NOISY_EPS_NET];
  __shared__ uint64_t keys[4];                       // the net's four streams (layer, side): three mixes each, once per workgroup
  const int z = blockIdx.y, t = threadIdx.x;
  if (t < 4) keys[t] = noisy_key(a.seed, a.step, z, t >> 1, t & 1);
  __syncthreads();
  for (int i = t; i < NOISY_EPS_NET; i += NOISY_THREADS) {
    const int layer = i < NOISY_EPS_IN5 ? 0 : 1, side = (i < NOISY_EPS_OUT4 || (i >= NOISY_EPS_IN5 && i < NOISY_EPS_OUT5)) ? 0 : 1;
    const int idx = i - (layer == 0 ? (side == 0 ? NOISY_EPS_IN4 : NOISY_EPS_OUT4) : (side == 0 ? NOISY_EPS_IN5 : NOISY_EPS_OUT5));
    const float e = (layer == 1 && side == 1 && idx >= a.A) ? 0.0f : noisy_factor(keys[2 * layer + side], (uint64_t)idx);
    sh[i] = e;
    if (blockIdx.x == 0) a.eps[z * NOISY_EPS_NET + i] = e;                                       // < 2 * NOISY_EPS_NET
  }
  __syncthreads();
  const float4* __restrict__ mu = reinterpret_cast<const float4*>(a.mu[z]);
  const float4* __restrict__ sg = reinterpret_cast<const float4*>(a.sigma[z]);
  float4* __restrict__ out = reinterpret_cast<float4*>(a.eff[z]);
  const int64_t n4 = a.NP / 4, stride = (int64_t)gridDim.x * NOISY_THREADS;
  for (int64_t i4 = (int64_t)blockIdx.x * NOISY_THREADS + t; i4 < n4; i4 += stride) {       // < NP / 4: inside all three buffers
    const float4 m = mu[i4];
    if (i4 < OFF4 / 4) { out[i4] = m; continue; }
    const float4 s = sg[i4 - OFF4 / 4];
    out[i4] = add4(m, mul4(s, factor4(sh, i4 * 4 - OFF4)));
  }
}

__global__ void __launch_bounds__(NOISY_THREADS) noisy_tail_kernel(const NoisyTailArgs a) {
  __shared__ alignas(16) float sh[NOISY_EPS_NET];
  const int t = threadIdx.x;
  for (int i = t; i < NOISY_EPS_NET; i += NOISY_THREADS) sh[i] = a.eps[i];
  __syncthreads();
  const float4* __restrict__ g = reinterpret_cast<const float4*>(a.g + OFF4);
  float4* __restrict__ sg = reinterpret_cast<float4*>(a.sigma);
  float4* __restrict__ s1 = reinterpret_cast<float4*>(a.state);
  float4* __restrict__ s2 = reinterpret_cast<float4*>(a.state2);
  float4* __restrict__ gk = reinterpret_cast<float4*>(a.gsig);
  const int64_t n4 = a.n / 4, stride = (int64_t)gridDim.x * NOISY_THREADS;
  for (int64_t i4 = (int64_t)blockIdx.x * NOISY_THREADS + t; i4 < n4; i4 += stride) {                // < n / 4: inside every buffer
    const float4 gs = mul4(g[i4], factor4(sh, i4 * 4));
    float4 w = sg[i4], p = s1[i4], q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.u.opt != 0) q = s2[i4];
    if (gk) gk[i4] = gs;
    w.x = opt_apply(w.x, p.x, q.x, gs.x, a.u); w.y = opt_apply(w.y, p.y, q.y, gs.y, a.u);
    w.z = opt_apply(w.z, p.z, q.z, gs.z, a.u); w.w = opt_apply(w.w, p.w, q.w, gs.w, a.u);
    sg[i4] = w; s1[i4] = p;
    if (a.u.opt != 0) s2[i4] = q;
  }
}

bool aligned16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_noisy_compose(const NoisyArgs& a, hipStream_t s) {
  if (a.nets < 1 || a.nets > 2 || a.A < 1 || a.A > MAX_ACTIONS || a.NP != OFF5 + (int64_t)a.A * NFC || !a.eps) return hipErrorInvalidValue;
  for (int z = 0; z < a.nets; ++z) if (!aligned16(a.mu[z]) || !aligned16(a.sigma[z]) || !aligned16(a.eff[z])) return hipErrorInvalidValue;
  SDQN_LAUNCH(noisy_compose_kernel, dim3(NOISY_GRID, a.nets), dim3(NOISY_THREADS), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_noisy_tail(const NoisyTailArgs& a, hipStream_t s) {
  if (a.u.A < 1 || a.u.A > MAX_ACTIONS || a.n != NW4 + (int64_t)a.u.A * NFC || !a.eps || !(a.u.bsz > 0.0f)) return hipErrorInvalidValue;
  if (!aligned16(a.g) || !aligned16(a.sigma) || !aligned16(a.state) || (a.u.opt != 0 && !aligned16(a.state2)) || (a.gsig && !aligned16(a.gsig))) return hipErrorInvalidValue;
  SDQN_LAUNCH(noisy_tail_kernel, dim3(NOISY_GRID), dim3(NOISY_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace sdqn
