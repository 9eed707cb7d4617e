// sdqn_cql.hip — the head of a conservative Q-learning train step, --cql_alpha (Kumar, Zhou, Tucker, Levine 2020, CQL(H), discrete form;
// DESIGN.md §35).  With q = Q(theta, s_n) (q slot 0, the step's own forward), a = a_n, alpha = HeadArgs::cql_alpha, y the standard target
// exactly as head_kernel forms it and w = 1 or the importance weight of a prioritized memory (cql.h holds the formulas, shared with the
// generic path and the host restatement sdqn_cql_loss):
//     lse    = m + log(sum_k exp(q[k] - m)), m = max_k q[k]        double from the stored fp32 row, the sum in action order
//     pi[k]  = exp(q[k] - lse)
//     delta  = q[a] - (float)y,  dc = clip(delta)                   (head_clip; clip first, then weight)
//     dq[k]  = w (float)(alpha (pi[k] - 1[k == a]))  +  1[k == a] w dc
//     cost   = w 0.5 delta^2  +  w (float)(alpha (lse - q[a]))      (head_delta's term plus the regulariser's)
//     d4     = 1[a4 > 0] sum_k W5[k] dq[k], in row order            (every fc5 row carries gradient)
// maxq[n] and the new priority (PER) are the standard head's: max_k Q(theta-, s'_n)[k] and (|delta| + eps)^alpha_per of the unclipped delta.
// The front end and the fc5 dgrad are head_body.h.  Between them the first A lanes of wave 0 work, lane k on action k: one exp for its term
// of the sum, the sum by A shuffles in action order, one log, one exp for pi[k]; y and delta are restated per lane from the two rows in LDS
// (no hand-off, no barrier); lane 0 alone writes maxq, the cost term and the priority.  No extra forward, no added launch, no scratch, no
// atomics: the step launches what the standard step launches.  alpha rides in mu_alpha's bytes (refused together): no field moves.
#include "head_body.h"
#include "cql.h"

namespace sdqn {
namespace {

template <int AMAX, bool PER, bool NSTEP>
__global__ void __launch_bounds__(512) cql_head_kernel(const StepArgs a, const HeadArgs h) {
  const int n = blockIdx.x, j = threadIdx.x;
  __shared__ float prod[2 * AMAX][NFC];
  __shared__ float sh_q[2][AMAX];
  __shared__ float sh_dq[AMAX];
  const int A = a.A;
  HeadFront<AMAX> f;
  head_front_issue<AMAX>(a, n, j, f);
  // minibatch metadata: the action lanes only (one address each: a broadcast load)
  int m_act = 0, m_term = 0; int64_t m_rew = 0;
  if (j < A) { m_act = h.st_actions[n]; m_rew = h.st_rewards[n]; m_term = h.st_terminals[n]; }
  float m_w = 1.0f;
  if constexpr (PER) { if (j < A) m_w = h.per_w[n]; }
  m_act = m_act < A ? m_act : A - 1;                   // memory safety only: the host rejects out-of-range actions before launching
  head_front_q<AMAX>(a, h, n, j, f, prod, sh_q);
  if (j < A) {                                         // A <= 18 lanes of wave 0; lane j owns action j
    float m = sh_q[1][0], qm = sh_q[0][0];
    for (int k = 1; k < A; ++k) { m = fmaxf(m, sh_q[1][k]); const float x = sh_q[0][k]; qm = x > qm ? x : qm; }   // max_a Q(theta-, s')[a]; cql_lse's maximum
    double rr, gam; head_reward<NSTEP>(h, m_rew, rr, gam);
    const double y = m_term ? rr : rr + gam * (double)m;
    const double e = exp((double)sh_q[0][j] - (double)qm);
    double s = 0.0;
    for (int k = 0; k < A; ++k) s += __shfl(e, k, 64);                                            // action order, as cql_lse (lanes k < A are all here)
    const double lse = (double)qm + log(s);
    const float qa = sh_q[0][m_act];
    const float d = qa - (float)y;
    const float dc = head_clip(h, d);
    const float t = m_w * cql_grad<float>(sh_q[0], j, m_act, lse, h.cql_alpha);
    const float v = j == m_act ? t + m_w * dc : t;                                                // (without PER m_w is 1: both products are exact)
    sh_dq[j] = v;
    h.dq[(int64_t)n * A + j] = v;
    if (j == 0) {
      if constexpr (PER) h.per_p[n] = (float)pow(fabs((double)d) + h.per_eps, h.per_alpha);       // unclipped |delta|, as head_delta
      h.cost_terms[n] = m_w * (0.5f * (d * d)) + m_w * cql_cost<float>(sh_q[0], m_act, lse, h.cql_alpha);
      h.maxq[n] = m;
    }
  }
  __syncthreads();
  head_back_rows<AMAX>(a, n, j, f, (1 << A) - 1, sh_dq);
}

typedef void (*CqlHead)(const StepArgs, const HeadArgs);
template <bool PER, bool NSTEP>
CqlHead head_for(int bucket) {
  return bucket == 0 ? cql_head_kernel<4, PER, NSTEP> : bucket == 1 ? cql_head_kernel<8, PER, NSTEP> : cql_head_kernel<MAX_ACTIONS, PER, NSTEP>;
}

}  // namespace

// launch_head's branch for HEAD_CQL (a.nz = 2: the step's own forward and nothing in front of it)
hipError_t launch_head_cql(const StepArgs& a, const HeadArgs& h, hipStream_t s) {
  if (h.train != HEAD_CQL || a.nz != 2 || a.bn || a.A < 1 || a.A > MAX_ACTIONS || !(h.cql_alpha > 0.0 && h.cql_alpha < INFINITY)) return hipErrorInvalidValue;
  const int bucket = head_bucket(a.A);
  const bool per = h.per_w != nullptr, nstep = h.nstep > 1;
  const CqlHead k = per ? (nstep ? head_for<true, true>(bucket) : head_for<true, false>(bucket))
                        : (nstep ? head_for<false, true>(bucket) : head_for<false, false>(bucket));
  SDQN_LAUNCH(k, dim3(a.B), dim3(512), 0, s, a, h);
  return hipGetLastError();
}

}  // namespace sdqn
