// head_body.h — what the option heads' kernels share, as device functions (HIP only): munchausen_head_kernel (sdqn_munchausen.hip),
// bootstrap_head_kernel (sdqn_bootstrap.hip), advantage_head_kernel (sdqn_advantage.hip), quantile_head_kernel (sdqn_quantile.hip),
// dueling_head_kernel (sdqn_dueling.hip) and cql_head_kernel (sdqn_cql.hip) are these pieces around the few lines of their own rule.  The statements and the floating-point operation order are
// head_kernel's (sdqn_kernels.hip) for a train step without batch_norm, nz = 2: one 512-thread workgroup per sample; the fc4 slab reduce +
// ReLU and the fc5 of slots 0 (online net, prestates) and 1 (target net, poststates) are the same loads, the same prod[][] transpose and the
// same single butterfly per row, so Q(pre), Q(post), a4 and d4 are what the standard head of a net with a.A outputs leaves.  head_kernel
// itself keeps its own text: it carries the leading-argument block, BN, QSYS, the third Double DQN slot and the timing stamps, and its
// instantiation set is part of sdqn_kernels.hip's tuning.
// A kernel calls head_front_issue, THEN loads its minibatch metadata, then head_front_q: nothing the front end loads waits behind the metadata.
// The __shared__ arrays are declared in each kernel (its LDS layout stays visible there) and passed by reference.  No scratch, no atomics.
#pragma once
#include "kernels.h"

namespace sdqn {

template <int AMAX>
struct HeadFront {
  float t[2][7];          // the fc4 slabs of this thread's column, both slots (S4 == 7 only)
  float w5[2][AMAX];      // fc5 rows of this thread's column: [0] online, [1] target; rows >= A repeat row A - 1 (never used)
  float a4v[2];           // a4[z][n][j]: the slab sum, after head_front_q its ReLU
};

// everything this thread will ever load but the metadata, issued up front (one memory round trip)
template <int AMAX>
__device__ __forceinline__ void head_front_issue(const StepArgs& a, int n, int j, HeadFront<AMAX>& f) {
  const int A = a.A;                                   // (a train step: nz = 2)
  const float* __restrict__ th0 = a.theta[0];
  const float* __restrict__ th1 = a.theta[1];
  const float* __restrict__ slab = a.slab4;
  f.a4v[0] = 0.0f; f.a4v[1] = 0.0f;
  const int64_t sstride = (int64_t)2 * a.B * NFC;
  if (a.S4 == 7) {                                     // the built-in split: 14 independent loads in flight
#pragma unroll
    for (int z = 0; z < 2; ++z)
#pragma unroll
      for (int s = 0; s < 7; ++s) f.t[z][s] = slab[s * sstride + ((int64_t)z * a.B + n) * NFC + j];
  }
#pragma unroll
  for (int act = 0; act < AMAX; ++act) {
    const int ac = act < A ? act : A - 1;
    f.w5[0][act] = th0[OFF5 + ac * NFC + j];
    f.w5[1][act] = th1[OFF5 + ac * NFC + j];
  }
}

// slab sum + ReLU -> a4 (stored), fc5 of both slots -> sh_q and h.q: every thread contributes w5[z][act][j] * a4[z][j], the 2 A block-wide
// sums go through LDS — products transposed into prod[row][512], then wave w reduces rows w, w + 8, ... (8 values per lane + one butterfly
// per row).  Ends behind a barrier: sh_q is complete, prod[][] is dead
template <int AMAX>
__device__ __forceinline__ void head_front_q(const StepArgs& a, const HeadArgs& h, int n, int j, HeadFront<AMAX>& f,
                                             float (&prod)[2 * AMAX][NFC], float (&sh_q)[2][AMAX]) {
  const int A = a.A, lane = j & 63, wave = j >> 6;
  if (a.S4 == 7) {
#pragma unroll
    for (int z = 0; z < 2; ++z) { float v = 0.0f;
#pragma unroll
      for (int s = 0; s < 7; ++s) v += f.t[z][s];                                                 // fixed order
      f.a4v[z] = v; }
  } else {
    const float* __restrict__ slab = a.slab4;
    const int64_t sstride = (int64_t)2 * a.B * NFC;
#pragma unroll
    for (int z = 0; z < 2; ++z) { float v = 0.0f;
      for (int s = 0; s < a.S4; ++s) v += slab[s * sstride + ((int64_t)z * a.B + n) * NFC + j];
      f.a4v[z] = v; }
  }
#pragma unroll
  for (int z = 0; z < 2; ++z) {                        // static indices only: w5 / a4v stay in registers
    const float v = fmaxf(f.a4v[z], 0.0f);
    f.a4v[z] = v;
    a.a4[((int64_t)z * a.B + n) * NFC + j] = v;
#pragma unroll
    for (int act = 0; act < AMAX; ++act)
      if (act < A) prod[z * A + act][j] = f.w5[z][act] * v;
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
}

// the reward and the discount of a target: the clipped reward and gamma, or (--n_step) the return R, which st_rewards holds as a double, and gamma^n
template <bool NSTEP>
__device__ __forceinline__ void head_reward(const HeadArgs& h, int64_t rew, double& rr, double& gam) {
  if constexpr (NSTEP) { rr = __builtin_bit_cast(double, rew); gam = h.gamma_n; }
  else {
    rr = (double)rew;
    rr = rr < h.min_reward ? h.min_reward : (rr > h.max_reward ? h.max_reward : rr);
    gam = h.discount;
  }
}

__device__ __forceinline__ float head_clip(const HeadArgs& h, float d) {
  float dc = d;
  if (h.clip_error != 0.0f) dc = fminf(fmaxf(d, -h.clip_error), h.clip_error);
  return dc;
}

// everything behind the target y of the taken action (one thread): delta, clip, the PER weighting and priority, the cost term.  Returns dq's entry
template <bool PER>
__device__ __forceinline__ float head_delta(const HeadArgs& h, int n, float q_taken, double y, float m_w) {
  const float d = q_taken - (float)y;
  float dc = head_clip(h, d);
  if constexpr (PER) {                                 // importance weight on the taken action's row: clip first, then weight
    h.cost_terms[n] = m_w * (0.5f * (d * d));
    dc = m_w * dc;
    h.per_p[n] = (float)pow(fabs((double)d) + h.per_eps, h.per_alpha);                            // unclipped |delta|
  } else
  h.cost_terms[n] = 0.5f * (d * d);
  return dc;
}

__device__ __forceinline__ void head_store_d4(const StepArgs& a, int n, int j, float d4v) {
  if (a.h16) a.h_d4[(int64_t)n * NFC + j] = (half_t)(d4v * a.loss_scale);     // fp16 mode: loss-scaled half delta
  else a.d4[(int64_t)n * NFC + j] = d4v;
}

// fc5 dgrad: delta4 = W5^T delta * 1[a4 > 0]; delta is dc on the taken action only (W5 row already in registers).  Writes d4 and the dq row
template <int AMAX>
__device__ __forceinline__ void head_back_one(const StepArgs& a, const HeadArgs& h, int n, int j, const HeadFront<AMAX>& f, int act, float dc) {
  float wa = 0.0f;
#pragma unroll
  for (int k = 0; k < AMAX; ++k) wa = (k == act) ? f.w5[0][k] : wa;
  head_store_d4(a, n, j, f.a4v[0] > 0.0f ? wa * dc : 0.0f);
  if (j < a.A) h.dq[(int64_t)n * a.A + j] = (j == act) ? dc : 0.0f;
}

// fc5 dgrad over the rows whose bit is set in `rows`, in row order; dq: the sample's dq row (LDS).  Writes d4
template <int AMAX>
__device__ __forceinline__ void head_back_rows(const StepArgs& a, int n, int j, const HeadFront<AMAX>& f, int rows, const float (&dq)[AMAX]) {
  float acc = 0.0f;
#pragma unroll
  for (int r = 0; r < AMAX; ++r) if ((rows >> r) & 1) acc += f.w5[0][r] * dq[r];
  head_store_d4(a, n, j, f.a4v[0] > 0.0f ? acc : 0.0f);
}

// the AMAX a launcher picks: 0 / 1 / 2 = kernel<4> / <8> / <MAX_ACTIONS>
inline int head_bucket(int A) { return A <= 4 ? 0 : (A <= 8 ? 1 : 2); }

}  // namespace sdqn
