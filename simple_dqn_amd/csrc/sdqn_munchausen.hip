// sdqn_munchausen.hip — the head of a Munchausen DQN train step, --munchausen.  The rule is munchausen.h's, with tau / alpha /
// l0 = HeadArgs::mu_tau / mu_alpha / mu_clip; thread 0 applies it to the stored fp32 rows, as head_kernel computes its y.
// Everything in front of y and behind it is head_body.h.  qbar(s_n) is NOT computed here: a forward of the target weights on the
// prestates runs in front of the step and leaves it in q slot 2 (sdqn_api_step.hip: run_extra_forward); thread 0 reads row n of it
// the way the batch_norm Double DQN head reads its slot 2.
#include "head_body.h"
#include "munchausen.h"

namespace sdqn {
namespace {

template <int AMAX, bool PER, bool NSTEP>
__global__ void __launch_bounds__(512) munchausen_head_kernel(const StepArgs a, const HeadArgs h) {
  const int n = blockIdx.x, j = threadIdx.x;
  __shared__ float prod[2 * AMAX][NFC];
  __shared__ float sh_q[2][AMAX];
  __shared__ float sh_dc;
  __shared__ int sh_act;
  const int A = a.A;
  HeadFront<AMAX> f;
  head_front_issue<AMAX>(a, n, j, f);
  int m_act = 0, m_term = 0; int64_t m_rew = 0;
  if (j == 0) { m_act = h.st_actions[n]; m_rew = h.st_rewards[n]; m_term = h.st_terminals[n]; }
  float m_w = 1.0f;
  if constexpr (PER) { if (j == 0) m_w = h.per_w[n]; }
  m_act = m_act < A ? m_act : A - 1;                   // memory safety only: the host rejects out-of-range actions before launching
  head_front_q<AMAX>(a, h, n, j, f, prod, sh_q);
  if (j == 0) {
    const float* qpre = h.q + ((int64_t)2 * a.B + n) * A;                                         // qbar(s_n): q slot 2, left by the extra forward
    double rr, gam; head_reward<NSTEP>(h, m_rew, rr, gam);
    double V; const double y = munchausen_target<float>(qpre, sh_q[1], A, m_act, rr, m_term, gam, h.mu_alpha, h.mu_tau, h.mu_clip, &V);
    const float dc = head_delta<PER>(h, n, sh_q[0][m_act], y, m_w);
    h.maxq[n] = (float)V;
    sh_dc = dc; sh_act = m_act;
  }
  __syncthreads();
  head_back_one<AMAX>(a, h, n, j, f, sh_act, sh_dc);
}

typedef void (*MunchausenHead)(const StepArgs, const HeadArgs);
template <bool PER, bool NSTEP>
MunchausenHead head_for(int bucket) {
  return bucket == 0 ? munchausen_head_kernel<4, PER, NSTEP> : bucket == 1 ? munchausen_head_kernel<8, PER, NSTEP> : munchausen_head_kernel<MAX_ACTIONS, PER, NSTEP>;
}

}  // namespace

// launch_head's branch for HEAD_MUNCHAUSEN (a.nz = 2: the step's own forward; q has a third slot holding qbar of the prestates)
hipError_t launch_head_munchausen(const StepArgs& a, const HeadArgs& h, hipStream_t s) {
  if (h.train != HEAD_MUNCHAUSEN || a.nz != 2 || a.bn || a.A < 1 || a.A > MAX_ACTIONS || !(h.mu_tau > 0.0)) return hipErrorInvalidValue;
  const int bucket = head_bucket(a.A);
  const bool per = h.per_w != nullptr, nstep = h.nstep > 1;
  const MunchausenHead k = per ? (nstep ? head_for<true, true>(bucket) : head_for<true, false>(bucket))
                               : (nstep ? head_for<false, true>(bucket) : head_for<false, false>(bucket));
  SDQN_LAUNCH(k, dim3(a.B), dim3(512), 0, s, a, h);
  return hipGetLastError();
}

}  // namespace sdqn
