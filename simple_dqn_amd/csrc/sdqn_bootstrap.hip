// sdqn_bootstrap.hip — Bootstrapped DQN, --bootstrap_heads K: the head of a train step and the acting rule's select launch.
// The net has A' = K A outputs; the rule (targets, masks m_k, dq row, cost term, maxq) is bootstrap.h's bootstrap_sample, and
//     d4     = 1[a4 > 0] sum_k W5[k A + a_n] dq_k  over the rows with m_k = 1, in head order
// The front end over the A' rows and the fc5 dgrad are head_body.h.  Thread 0 runs the rule with fmaxf / fminf (td_rule.h: FminmaxOps); the
// dq row replaces the (dead) target-net row in LDS and reaches the other threads with a bit mask of its live rows.  K, A, the mask threshold and
// seed and the index pointer are a third kernel argument (BootArgs), StepArgs and HeadArgs keep their layout.
#include "head_body.h"

namespace sdqn {
namespace {

template <int AMAX, bool NSTEP>
__global__ void __launch_bounds__(512) bootstrap_head_kernel(const StepArgs a, const HeadArgs h, const BootArgs b) {
  const int n = blockIdx.x, j = threadIdx.x;
  __shared__ float prod[2 * AMAX][NFC];
  __shared__ float sh_q[2][AMAX];
  __shared__ int sh_rows;
  const int A = a.A;                                   // K A rows
  HeadFront<AMAX> f;
  head_front_issue<AMAX>(a, n, j, f);
  int m_act = 0, m_term = 0; int64_t m_rew = 0, m_idx = 0;
  if (j == 0) {
    m_act = h.st_actions[n]; m_rew = h.st_rewards[n]; m_term = h.st_terminals[n];
    if (b.idx) m_idx = b.idx[n];
  }
  m_act = m_act < b.A ? m_act : b.A - 1;               // memory safety only: the host rejects out-of-range actions before launching
  head_front_q<AMAX>(a, h, n, j, f, prod, sh_q);
  if (j == 0) {
    double rr, gam; head_reward<NSTEP>(h, m_rew, rr, gam);
    int rows;                                          // dq = sh_q[1]: each Q-head's slice of the target row is dead once its maximum is taken
    h.cost_terms[n] = bootstrap_sample<float, FminmaxOps>(sh_q[0], sh_q[1], b.K, b.A, m_act, rr, m_term, gam, h.clip_error, b.mask_seed, b.thresh,
                                                          m_idx, sh_q[1], &rows, &h.maxq[n]);
    sh_rows = rows;
  }
  __syncthreads();
  head_back_rows<AMAX>(a, n, j, f, sh_rows, sh_q[1]);  // over the live rows, in head order
  if (j < A) h.dq[(int64_t)n * A + j] = sh_q[1][j];
}

typedef void (*BootstrapHead)(const StepArgs, const HeadArgs, const BootArgs);
template <bool NSTEP>
BootstrapHead head_for(int bucket) {
  return bucket == 0 ? bootstrap_head_kernel<4, NSTEP> : bucket == 1 ? bootstrap_head_kernel<8, NSTEP> : bootstrap_head_kernel<MAX_ACTIONS, NSTEP>;
}

// The acting rule's reduction of the forward's [N][K A] rows to [N][A] acting rows, one thread per copy.
//   vote = 0 (collecting): the slice of Q-head k(e, episodes_e); episodes_e is read from the copies' records at recs + e stride + offset
//   vote = 1 (testing): the vote counts of the K per-head greedy actions, as numbers of T (their first maximum is the lowest action with the most votes)
template <typename T>
__global__ void __launch_bounds__(64) bootstrap_select_kernel(const T* __restrict__ q, T* __restrict__ out, int N, int K, int A, int vote,
                                                              uint64_t head_seed, const unsigned char* __restrict__ recs, size_t stride, size_t offset) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N) return;
  const T* row = q + (size_t)e * K * A;
  T* o = out + (size_t)e * A;
  if (vote) {
    for (int c = 0; c < A; ++c) o[c] = (T)0;
    for (int k = 0; k < K; ++k) {
      const T* r = row + k * A; int best = 0;
      for (int c = 1; c < A; ++c) if (r[c] > r[best] || (r[c] != r[c] && r[best] == r[best])) best = c;
      o[best] += (T)1;
    }
  } else {
    const int64_t ep = *reinterpret_cast<const int64_t*>(recs + (size_t)e * stride + offset);
    const int k = bootstrap_head_of(head_seed, K, (uint64_t)e, (uint64_t)ep);
    for (int c = 0; c < A; ++c) o[c] = row[k * A + c];
  }
}

}  // namespace

// launch_head's branch for HEAD_BOOTSTRAP (a.nz = 2; a.A = K b.A)
hipError_t launch_head_bootstrap(const StepArgs& a, const HeadArgs& h, const BootArgs& b, hipStream_t s) {
  if (h.train != HEAD_BOOTSTRAP || a.nz != 2 || a.bn || h.per_w || b.K < 1 || b.A < 1 || a.A != b.K * b.A || a.A > MAX_ACTIONS) return hipErrorInvalidValue;
  if (!b.idx && b.thresh < (1ull << 53)) return hipErrorInvalidValue;           // masks need the ring index
  const BootstrapHead k = h.nstep > 1 ? head_for<true>(head_bucket(a.A)) : head_for<false>(head_bucket(a.A));
  SDQN_LAUNCH(k, dim3(a.B), dim3(512), 0, s, a, h, b);
  return hipGetLastError();
}

hipError_t launch_bootstrap_select(const void* q, void* out, bool f64, int N, int K, int A, int vote, uint64_t head_seed,
                                   const void* recs, size_t stride, size_t offset, hipStream_t s) {
  if (N < 1 || K < 1 || A < 1 || (!vote && !recs)) return hipErrorInvalidValue;
  const dim3 grid((N + 63) / 64), block(64);
  const unsigned char* rp = static_cast<const unsigned char*>(recs);
  if (f64) SDQN_LAUNCH(bootstrap_select_kernel<double>, grid, block, 0, s, static_cast<const double*>(q), static_cast<double*>(out), N, K, A, vote, head_seed, rp, stride, offset);
  else SDQN_LAUNCH(bootstrap_select_kernel<float>, grid, block, 0, s, static_cast<const float*>(q), static_cast<float*>(out), N, K, A, vote, head_seed, rp, stride, offset);
  return hipGetLastError();
}

}  // namespace sdqn
