// sdqn_advantage.hip — the head of an advantage-learning train step, --advantage_learning / --persistent_advantage (Bellemare, Ostrovski,
// Guez, Thomas, Munos 2016, "Increasing the Action Gap").  With qbar(s) = Q(theta-, s), alpha = HeadArgs::al_alpha:
//     gap(q, a) = max_k q[k] - q[a]                                                     (>= 0, exactly 0 when a is a maximiser)
//     y_std[n]  = r_c[n] + (terminal ? 0 : gamma max_a qbar(s'_n)[a])                    (--n_step: R, done, gamma^n in their places)
//     y_AL[n]   = y_std[n] - alpha gap(qbar(s_n), a_n)                                   (on terminal transitions too)
//     y_PAL[n]  = terminal ? y_AL[n] : max(y_AL[n], y_std[n] - alpha gap(qbar(s'_n), a_n))          (HeadArgs::al_persistent)
// all in double from the stored fp32 Q-values, as head_kernel computes its y; everything behind y (delta, clip, the PER weighting and
// priority, cost term, dq, fc5 dgrad) is head_kernel's code.  maxq[n] receives max_a qbar(s'_n)[a], as the standard head's.
// One 512-thread workgroup per sample, as head_kernel (sdqn_kernels.hip) and munchausen_head_kernel (sdqn_munchausen.hip): the fc4 slab
// reduce + ReLU and the fc5 of slots 0 (online net, prestates) and 1 (target net, poststates) are the same loads, the same prod[][]
// transpose and the same single butterfly per row, so Q(pre), Q(post), a4 and d4 are what the standard head leaves.  qbar(s_n) is NOT
// computed here: a forward of the target weights on the prestates runs in front of the step and leaves it in q slot 2 (sdqn_api_step.hip:
// run_extra_forward); thread 0 reads row n of it.  The PAL choice is a run-time branch in thread 0: one kernel per (bucket, PER, NSTEP).
// A kernel of its own name in a translation unit of its own: head_kernel's template parameter list and the instantiation set of
// sdqn_kernels.hip (part of that file's tuning) stay what they are.  No scratch, no atomics; LDS = munchausen_head_kernel's per bucket.
#include "kernels.h"

namespace sdqn {
namespace {

// max_k q[k] - q[act] of one Q row, double: every term is a stored value, so the gap of a maximiser is exactly +0
__device__ __forceinline__ double action_gap(const float* q, int A, int act) {
  double v = (double)q[0];
  for (int k = 1; k < A; ++k) { const double x = (double)q[k]; v = x > v ? x : v; }
  return v - (double)q[act];
}

template <int AMAX, bool PER, bool NSTEP>
__global__ void __launch_bounds__(512) advantage_head_kernel(const StepArgs a, const HeadArgs h) {
  const int n = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6;
  __shared__ float prod[2 * AMAX][NFC];
  __shared__ float sh_q[2][AMAX];
  __shared__ float sh_dc;
  __shared__ int sh_act;
  const int A = a.A;                                   // (a train step: nz = 2)
  const float* __restrict__ th0 = a.theta[0];
  const float* __restrict__ th1 = a.theta[1];
  const float* __restrict__ slab = a.slab4;
  float a4v[2] = {0.0f, 0.0f};
  const int64_t sstride = (int64_t)2 * a.B * NFC;
  float t[2][7];
  if (a.S4 == 7) {                                     // the built-in split: 14 independent loads in flight
#pragma unroll
    for (int z = 0; z < 2; ++z)
#pragma unroll
      for (int s = 0; s < 7; ++s) t[z][s] = slab[s * sstride + ((int64_t)z * a.B + n) * NFC + j];
  }
  float w5[2][AMAX];
#pragma unroll
  for (int act = 0; act < AMAX; ++act) {
    const int ac = act < A ? act : A - 1;
    w5[0][act] = th0[OFF5 + ac * NFC + j];
    w5[1][act] = th1[OFF5 + ac * NFC + j];
  }
  int m_act = 0, m_term = 0; int64_t m_rew = 0;
  if (j == 0) { m_act = h.st_actions[n]; m_rew = h.st_rewards[n]; m_term = h.st_terminals[n]; }
  float m_w = 1.0f;
  if constexpr (PER) { if (j == 0) m_w = h.per_w[n]; }
  m_act = m_act < A ? m_act : A - 1;                   // memory safety only: the host rejects out-of-range actions before launching
  if (a.S4 == 7) {
#pragma unroll
    for (int z = 0; z < 2; ++z) { float v = 0.0f;
#pragma unroll
      for (int s = 0; s < 7; ++s) v += t[z][s];                                                   // fixed order
      a4v[z] = v; }
  } else {
#pragma unroll
    for (int z = 0; z < 2; ++z) { float v = 0.0f;
      for (int s = 0; s < a.S4; ++s) v += slab[s * sstride + ((int64_t)z * a.B + n) * NFC + j];
      a4v[z] = v; }
  }
#pragma unroll
  for (int z = 0; z < 2; ++z) {
    const float v = fmaxf(a4v[z], 0.0f);
    a4v[z] = v;
    a.a4[((int64_t)z * a.B + n) * NFC + j] = v;
#pragma unroll
    for (int act = 0; act < AMAX; ++act)
      if (act < A) prod[z * A + act][j] = w5[z][act] * v;
  }
  __syncthreads();
  for (int row = wave; row < 2 * A; row += 8) {
    float p = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) p += prod[row][lane + 64 * k];                                    // fixed order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p += __shfl_xor(p, off, 64);
    if (lane == 0) {
      const int z = row / A, act = row - z * A;
      sh_q[z][act] = p;
      h.q[((int64_t)z * a.B + n) * A + act] = p;
    }
  }
  __syncthreads();
  if (j == 0) {
    const int act = m_act, term = m_term; const int64_t rew = m_rew;
    const float* qpre = h.q + ((int64_t)2 * a.B + n) * A;                                         // qbar(s_n): q slot 2, left by the extra forward
    float m = sh_q[1][0];
    for (int k = 1; k < A; ++k) m = fmaxf(m, sh_q[1][k]);                                         // max_a qbar(s'_n)[a]
    double rr, gam;
    if constexpr (NSTEP) { rr = __builtin_bit_cast(double, rew); gam = h.gamma_n; }
    else {
      rr = (double)rew;
      rr = rr < h.min_reward ? h.min_reward : (rr > h.max_reward ? h.max_reward : rr);
      gam = h.discount;
    }
    const double ystd = term ? rr : rr + gam * (double)m;
    double y = ystd - h.al_alpha * action_gap(qpre, A, act);                                      // the gap correction applies on terminal transitions too
    if (h.al_persistent && !term) {                                                               // PAL: the better of leaving a_n now and repeating it in s'_n
      const double yp = ystd - h.al_alpha * ((double)m - (double)sh_q[1][act]);
      y = yp > y ? yp : y;
    }
    const float d = sh_q[0][act] - (float)y;
    float dc = d;
    if (h.clip_error != 0.0f) dc = fminf(fmaxf(d, -h.clip_error), h.clip_error);
    if constexpr (PER) {                               // importance weight on the taken action's row: clip first, then weight
      h.cost_terms[n] = m_w * (0.5f * (d * d));
      dc = m_w * dc;
      h.per_p[n] = (float)pow(fabs((double)d) + h.per_eps, h.per_alpha);                          // unclipped |delta|
    } else
    h.cost_terms[n] = 0.5f * (d * d);
    h.maxq[n] = m;
    sh_dc = dc; sh_act = act;
  }
  __syncthreads();
  const float dc = sh_dc; const int act = sh_act;
  // fc5 dgrad: delta4 = W5^T delta * 1[a4 > 0]; delta is non-zero on the taken action only (W5 row already in registers)
  float wa = 0.0f;
#pragma unroll
  for (int k = 0; k < AMAX; ++k) wa = (k == act) ? w5[0][k] : wa;
  const float d4v = a4v[0] > 0.0f ? wa * dc : 0.0f;
  if (a.h16) a.h_d4[(int64_t)n * NFC + j] = (half_t)(d4v * a.loss_scale);     // fp16 mode: loss-scaled half delta
  else a.d4[(int64_t)n * NFC + j] = d4v;
  if (j < A) h.dq[(int64_t)n * A + j] = (j == act) ? dc : 0.0f;
}

typedef void (*AdvantageHead)(const StepArgs, const HeadArgs);
template <bool PER, bool NSTEP>
AdvantageHead head_for(int bucket) {
  return bucket == 0 ? advantage_head_kernel<4, PER, NSTEP> : bucket == 1 ? advantage_head_kernel<8, PER, NSTEP> : advantage_head_kernel<MAX_ACTIONS, PER, NSTEP>;
}

}  // namespace

// launch_head's branch for HeadArgs::train == 5 (a.nz = 2: the step's own forward; q has a third slot holding qbar of the prestates)
hipError_t launch_head_advantage(const StepArgs& a, const HeadArgs& h, hipStream_t s) {
  if (h.train != 5 || a.nz != 2 || a.bn || a.A < 1 || a.A > MAX_ACTIONS || !(h.al_alpha > 0.0 && h.al_alpha < 1.0)) return hipErrorInvalidValue;
  if (h.al_persistent && h.nstep > 1) return hipErrorInvalidValue;             // (PAL repeats a_n in the NEXT state: refused with n-step returns)
  const int bucket = a.A <= 4 ? 0 : (a.A <= 8 ? 1 : 2);
  const bool per = h.per_w != nullptr, nstep = h.nstep > 1;
  const AdvantageHead k = per ? (nstep ? head_for<true, true>(bucket) : head_for<true, false>(bucket))
                              : (nstep ? head_for<false, true>(bucket) : head_for<false, false>(bucket));
  SDQN_LAUNCH(k, dim3(a.B), dim3(512), 0, s, a, h);
  return hipGetLastError();
}

}  // namespace sdqn
