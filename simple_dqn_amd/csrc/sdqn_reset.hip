// sdqn_reset.hip — periodic resets with shrink-and-perturb (--reset_interval): the kernel.  The rules — layer map, factors, draw,
// per-entry formula — are reset.h's.
//   reset_apply_kernel    walks the tail [reset_first, n) of the flat buffers by 16-byte pieces, a piece per thread and grid stride (at most
//                         2048 workgroups of 256: the whole tail of the default net is 1 piece per thread).  The layer boundaries are
//                         multiples of 4 entries, so a piece lies in one layer and has one action; a piece of a kept layer is skipped without
//                         a read.  A redrawn piece reads nothing; a shrunk one reads theta and theta_t.  theta, theta_t, state and state2 are
//                         written in the same pass with the same four draws.  Workgroup 0 also leaves the event's record.
// No atomics, no LDS, no scratch; a piece's result is a function of its index alone.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "problems.h"
#include "reset.h"
#include "launch.h"

namespace sdqn {

static_assert((OFF2 & 3) == 0 && (OFF3 & 3) == 0 && (OFF4 & 3) == 0 && (OFF5 & 3) == 0 && (NFC & 3) == 0, "a 16-byte piece lies in one layer");

namespace {

typedef float reset_f4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256) reset_apply_kernel(const ResetApplyArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { a.info[0] = (int64_t)a.event; a.info[1] = a.step; }
  const ResetRule r = reset_rule(a.layers, a.alpha);
  const uint64_t key = reset_key(a.seed, a.event);
  const int64_t first = reset_first(a.layers, a.alpha);
  const int64_t n4 = (a.n - first) >> 2;                               // (the launcher has checked first <= n and n % 4 == 0)
  const bool two = a.theta_t && a.theta_t != a.theta;
  const reset_f4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n4; p += (int64_t)gridDim.x * 256) {
    const int64_t i0 = first + p * 4;                                  // i0 + 3 < n
    const int L = layer_of(i0), act = reset_action(r, L);
    if (!act) continue;
    reset_f4 w = zero, wt = zero;
    if (act == 2) {
      w = *reinterpret_cast<const reset_f4*>(a.theta + i0);
      if (two) wt = *reinterpret_cast<const reset_f4*>(a.theta_t + i0);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float phi = reset_draw(key, (uint64_t)(i0 + v), L);
      w[v] = reset_value(r, act, w[v], phi);
      wt[v] = reset_value(r, act, wt[v], phi);
    }
    *reinterpret_cast<reset_f4*>(a.theta + i0) = w;
    if (two) *reinterpret_cast<reset_f4*>(a.theta_t + i0) = wt;
    *reinterpret_cast<reset_f4*>(a.state + i0) = zero;
    if (a.state2) *reinterpret_cast<reset_f4*>(a.state2 + i0) = zero;
  }
}

}  // namespace

hipError_t launch_reset_apply(const ResetApplyArgs& a, hipStream_t s) {
  if (a.n < OFF5 + NFC || (a.n & 3) || !a.theta || !a.state || !a.info) return hipErrorInvalidValue;
  if (a.layers < 0 || a.layers > RESET_LAYERS || !(a.alpha >= 0.0 && a.alpha <= 1.0) || reset_noop(a.layers, a.alpha)) return hipErrorInvalidValue;
  const int64_t first = reset_first(a.layers, a.alpha);                // <= OFF5 < n: at least fc5 is in the tail
  if (first < 0 || first >= a.n || (first & 3)) return hipErrorInvalidValue;
  int64_t blocks = (((a.n - first) >> 2) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  SDQN_LAUNCH(reset_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sdqn
