// sdqn_dueling.hip — the dueling architecture, --dueling (Wang et al. 2016): the head of a train step, the block mask of
// fc5 and the acting paths' Q launch.  The net has A' = A + 1 outputs, row 0 = V, row 1 + a = Adv_a; fc5 is block-sparse (dueling.h:
// dueling_mask), so V is a function of fc4's units j < 256 and every Adv_a of its units j >= 256.  For sample n (dueling.h holds the
// formulas, shared with the generic path and the host restatement sdqn_dueling_loss):
//     Q(s, a)  = (float)((V + Adv_a) - (sum_b Adv_b) / A)               double from the stored fp32 rows, the sum in action order
//     y        = r_c + (terminal ? 0 : gamma max_a Q(theta-, s', a))    (double, as head_kernel's y; --n_step: R, done, gamma^n in their places)
//     c        = head_delta<PER>(Q(theta, s, a_n), y)                   (delta, the clip, the cost term, PER's weight and priority: head_body.h)
//     dq[n][0] = c,  dq[n][1 + b] = c (1[b = a_n] - 1 / A)
//     d4       = 1[a4 > 0] sum_rows W5[row] dq[row], in row order       (the masked weights are +0: a stream receives its own rows only)
// The front end over the A' rows and the fc5 dgrad are head_body.h.  Between them thread 0 applies the rule to the two rows in LDS and
// leaves the dq row where the target net's row lay.  A, the armed flag and the read-back buffer are a third kernel argument (DuelArgs);
// StepArgs and HeadArgs keep their layout.  LDS: prod[][] and sh_q[][] only.
#include "head_body.h"

namespace sdqn {
namespace {

template <int AMAX, bool NSTEP, bool PER>
__global__ void __launch_bounds__(512) dueling_head_kernel(const StepArgs a, const HeadArgs h, const DuelArgs b) {
  const int n = blockIdx.x, j = threadIdx.x;
  __shared__ float prod[2 * AMAX][NFC];
  __shared__ float sh_q[2][AMAX];
  const int R = a.A;                                   // A + 1 rows
  const int A = b.A;
  HeadFront<AMAX> f;
  head_front_issue<AMAX>(a, n, j, f);
  int m_act = 0, m_term = 0; int64_t m_rew = 0;
  if (j == 0) { m_act = h.st_actions[n]; m_rew = h.st_rewards[n]; m_term = h.st_terminals[n]; }
  float m_w = 1.0f;
  if constexpr (PER) { if (j == 0) m_w = h.per_w[n]; }
  m_act = m_act < A ? m_act : A - 1;                   // memory safety only: the host rejects out-of-range actions before launching
  head_front_q<AMAX>(a, h, n, j, f, prod, sh_q);
  if (j == 0) {
    float m; dueling_greedy(sh_q[1], A, &m);                                                      // max_a Q(theta-, s', a)
    double rr, gam; head_reward<NSTEP>(h, m_rew, rr, gam);
    const double y = m_term ? rr : rr + gam * (double)m;
    const float qt = dueling_q(sh_q[0], A, m_act);
    const float c = head_delta<PER>(h, n, qt, y, m_w);
    h.maxq[n] = m;
    if (b.step) { b.step[n] = (float)y; b.step[(int64_t)a.B + n] = qt - (float)y; }
    dueling_dq<float>(c, A, m_act, sh_q[1]);                                                      // the target net's row is dead: it becomes the dq row
  }
  __syncthreads();
  if (j < R) h.dq[(int64_t)n * R + j] = sh_q[1][j];
  head_back_rows<AMAX>(a, n, j, f, (1 << R) - 1, sh_q[1]);
}

typedef void (*DuelingHead)(const StepArgs, const HeadArgs, const DuelArgs);
template <bool NSTEP, bool PER>
DuelingHead head_for(int bucket) {
  return bucket == 0 ? dueling_head_kernel<4, NSTEP, PER> : bucket == 1 ? dueling_head_kernel<8, NSTEP, PER> : dueling_head_kernel<MAX_ACTIONS, NSTEP, PER>;
}

// fc5's block mask on one flat vector's [rows][H] fc5 range (weights or gradient sums): the entries outside the two streams become +0.0
template <typename T>
__global__ void __launch_bounds__(256) dueling_mask_kernel(T* __restrict__ w5, int rows, int H) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * H) return;
  const int row = i / H;
  if (!dueling_mask(row, i - row * H, H)) w5[i] = (T)0;
}

// The acting paths' reduction of the forward's [M][A + 1] rows to the [M][A] action values the game kernels read, one thread per (copy, action)
template <typename T>
__global__ void __launch_bounds__(64) dueling_q_kernel(const T* __restrict__ q, T* __restrict__ out, int M, int A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M * A) return;
  const int e = i / A;
  out[i] = dueling_q(q + (size_t)e * (A + 1), A, i - e * A);
}

}  // namespace

// launch_head's branch for HEAD_DUELING (a.nz = 2; a.A = b.A + 1)
hipError_t launch_head_dueling(const StepArgs& a, const HeadArgs& h, const DuelArgs& b, hipStream_t s) {
  if (h.train != HEAD_DUELING || a.nz != 2 || a.bn || !b.on || b.A < 1 || a.A != b.A + 1 || a.A > MAX_ACTIONS) return hipErrorInvalidValue;
  const int bucket = head_bucket(a.A);
  const bool per = h.per_w != nullptr, nstep = h.nstep > 1;
  const DuelingHead k = per ? (nstep ? head_for<true, true>(bucket) : head_for<false, true>(bucket))
                            : (nstep ? head_for<true, false>(bucket) : head_for<false, false>(bucket));
  SDQN_LAUNCH(k, dim3(a.B), dim3(512), 0, s, a, h, b);
  return hipGetLastError();
}

hipError_t launch_dueling_mask(void* w5, bool f64, int rows, int H, hipStream_t s) {
  if (!w5 || rows < 2 || rows > MAX_ACTIONS || H < 2) return hipErrorInvalidValue;
  const dim3 grid((rows * H + 255) / 256), block(256);
  if (f64) SDQN_LAUNCH(dueling_mask_kernel<double>, grid, block, 0, s, static_cast<double*>(w5), rows, H);
  else SDQN_LAUNCH(dueling_mask_kernel<float>, grid, block, 0, s, static_cast<float*>(w5), rows, H);
  return hipGetLastError();
}

hipError_t launch_dueling_q(const void* q, void* out, bool f64, int M, int A, hipStream_t s) {
  if (M < 1 || A < 1) return hipErrorInvalidValue;
  const dim3 grid((M * A + 63) / 64), block(64);
  if (f64) SDQN_LAUNCH(dueling_q_kernel<double>, grid, block, 0, s, static_cast<const double*>(q), static_cast<double*>(out), M, A);
  else SDQN_LAUNCH(dueling_q_kernel<float>, grid, block, 0, s, static_cast<const float*>(q), static_cast<float*>(out), M, A);
  return hipGetLastError();
}

}  // namespace sdqn
