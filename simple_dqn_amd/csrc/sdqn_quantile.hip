// sdqn_quantile.hip — quantile-regression DQN, --quantiles N (Dabney, Rowland, Bellemare, Munos 2018): the head of a train
// step and the acting paths' mean launch.  The net has A' = N A outputs, row j A + a = quantile j of action a, tau_j = (2 j + 1) / (2 N).
// For sample n (quantile.h holds the formulas, shared with the generic path and the host restatement sdqn_quantile_loss):
//     m(a)   = (sum_j theta_j(theta-, s')[a]) / N in double, a* = its first maximum, maxq[n] = (float)m(a*)
//     T_j'   = r_c + (terminal ? 0 : gamma theta_j'(theta-, s')[a*])              (double from the stored fp32 Q, as head_kernel's y;
//                                                                                  --n_step: R, done, gamma^n in their places)
//     d_jj'  = theta_j(theta, s)[a_n] - (float)T_j',  w_jj' = |tau_j - 1[d_jj' > 0]|,  kappa = HeadArgs::clip_error
//     dq[n][j A + a_n] = (sum_j' w_jj' clip(d_jj', -kappa, kappa) / kappa) / N^2, the sum in j' order; zero elsewhere
//     cost term = (sum_jj' w_jj' L_kappa(d_jj') / kappa) / N^2, the sum in double in j-major order
//     d4     = 1[a4 > 0] sum_j W5[j A + a_n] dq_j, in quantile order
// The front end over the A' rows and the fc5 dgrad are head_body.h.  Between them the work is spread, not left to thread 0: thread t < N^2 owns
// the pair (j, j') = (t / N, t % N) — it restates m(a) and a* from the row in LDS (N A reads; no hand-off, no barrier), then its target and
// its pair's two terms, which go to the dead prod[][] rows 0 / 1; thread r < A' sums dq row r's N terms in j' order; behind its own share
// of the fc5 dgrad thread 0 adds the N^2 cost terms up in double, in the j-major order the rule states — a serial tail of every workgroup
// (36 LDS reads and adds at N = 6, 81 at N = 9, 324 at (A = 1, N = 18)), not overlapped work.  N, A and the targets' read-back buffer are a third kernel argument
// (QuantArgs); StepArgs and HeadArgs keep their layout.
#include "head_body.h"

namespace sdqn {
namespace {

template <int AMAX, bool NSTEP>
__global__ void __launch_bounds__(512) quantile_head_kernel(const StepArgs a, const HeadArgs h, const QuantArgs b) {
  const int n = blockIdx.x, j = threadIdx.x;
  __shared__ float prod[2 * AMAX][NFC];
  __shared__ float sh_q[2][AMAX];
  __shared__ int sh_rows;
  const int A = a.A;                                   // N A rows
  const int N = b.N, GA = b.A, NN = N * N;
  HeadFront<AMAX> f;
  head_front_issue<AMAX>(a, n, j, f);
  // minibatch metadata: the pair threads and the row threads only
  int m_act = 0, m_term = 0; int64_t m_rew = 0;
  if (j < NN || j < A) { m_act = h.st_actions[n]; m_rew = h.st_rewards[n]; m_term = h.st_terminals[n]; }
  m_act = m_act < GA ? m_act : GA - 1;                 // memory safety only: the host rejects out-of-range actions before launching
  head_front_q<AMAX>(a, h, n, j, f, prod, sh_q);       // prod[][] is dead from here on: rows 0 / 1 take the pairs' gradient / cost terms
  if (j < NN) {                                        // pair (qj, qp): quantile qj of the online net against target qp
    const int qj = j / N, qp = j - qj * N;
    double mb; const int as = quantile_greedy(sh_q[1], N, GA, &mb);
    double rr, gam; head_reward<NSTEP>(h, m_rew, rr, gam);
    const double y = m_term ? rr : rr + gam * (double)sh_q[1][qp * GA + as];
    float g, rho; quantile_pair<float>(sh_q[0][qj * GA + m_act] - (float)y, quantile_tau<float>(qj, N), h.clip_error, &g, &rho);
    prod[0][j] = g; prod[1][j] = rho;
    if (qj == 0 && b.targets) b.targets[(int64_t)n * N + qp] = (float)y;
    if (j == 0) {
      h.maxq[n] = (float)mb;
      int rows = 0;
      for (int k = 0; k < N; ++k) rows |= 1 << (k * GA + m_act);
      sh_rows = rows;
    }
  }
  __syncthreads();                                     // the target net's row is dead from here on: it becomes the dq row
  if (j < A) {
    const int qj = j / GA;
    float v = 0.0f;
    if (j - qj * GA == m_act) {
      float s = 0.0f;
      for (int qp = 0; qp < N; ++qp) s += prod[0][qj * N + qp];                                   // fixed order
      v = s / (float)NN;
    }
    sh_q[1][j] = v;
    h.dq[(int64_t)n * A + j] = v;
  }
  __syncthreads();
  head_back_rows<AMAX>(a, n, j, f, sh_rows, sh_q[1]);  // over the taken action's N rows, in quantile order
  if (j == 0) {
    double cost = 0.0;
    for (int p = 0; p < NN; ++p) cost += (double)prod[1][p];                                      // j-major
    h.cost_terms[n] = (float)(cost / (double)NN);
  }
}

typedef void (*QuantileHead)(const StepArgs, const HeadArgs, const QuantArgs);
template <bool NSTEP>
QuantileHead head_for(int bucket) {
  return bucket == 0 ? quantile_head_kernel<4, NSTEP> : bucket == 1 ? quantile_head_kernel<8, NSTEP> : quantile_head_kernel<MAX_ACTIONS, NSTEP>;
}

// The acting paths' reduction of the forward's [M][N A] rows to the [M][A] action values the game kernels read, one thread per (copy, action):
// a sum of T in quantile order, divided by N (quantile.h: quantile_action_value)
template <typename T>
__global__ void __launch_bounds__(64) quantile_mean_kernel(const T* __restrict__ q, T* __restrict__ out, int M, int N, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * A) return;
  const int e = i / A, c = i - e * A;
  out[i] = quantile_action_value(q + (size_t)e * N * A, N, A, c);
}

}  // namespace

// launch_head's branch for HEAD_QUANTILE (a.nz = 2; a.A = b.N b.A)
hipError_t launch_head_quantile(const StepArgs& a, const HeadArgs& h, const QuantArgs& b, hipStream_t s) {
  if (h.train != HEAD_QUANTILE || a.nz != 2 || a.bn || h.per_w || b.N < 2 || b.A < 1 || a.A != b.N * b.A || a.A > MAX_ACTIONS || !(h.clip_error > 0.0f))
    return hipErrorInvalidValue;                       // (N <= 18: at most 324 pair threads; N A <= 18 rows)
  const QuantileHead k = h.nstep > 1 ? head_for<true>(head_bucket(a.A)) : head_for<false>(head_bucket(a.A));
  SDQN_LAUNCH(k, dim3(a.B), dim3(512), 0, s, a, h, b);
  return hipGetLastError();
}

hipError_t launch_quantile_mean(const void* q, void* out, bool f64, int M, int N, int A, hipStream_t s) {
  if (M < 1 || N < 1 || A < 1) return hipErrorInvalidValue;
  const dim3 grid((M * A + 63) / 64), block(64);
  if (f64) SDQN_LAUNCH(quantile_mean_kernel<double>, grid, block, 0, s, static_cast<const double*>(q), static_cast<double*>(out), M, N, A);
  else SDQN_LAUNCH(quantile_mean_kernel<float>, grid, block, 0, s, static_cast<const float*>(q), static_cast<float*>(out), M, N, A);
  return hipGetLastError();
}

}  // namespace sdqn
