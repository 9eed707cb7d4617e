// sdqn_bootstrap.hip — Bootstrapped DQN, --bootstrap_heads K (Osband, Blundell, Pritzel, Van Roy 2016): the head of a train
// step and the acting rule's select launch.  The net has A' = K A outputs, row k A + a = Q-head k, action a.  For sample n, ring slot i_n:
//     y_k    = r_c + (terminal ? 0 : gamma max_a Q_k(theta-, s')[a])          (double from the stored fp32 Q, as head_kernel's y;
//                                                                               --n_step: R, done, gamma^n in their places)
//     d_k    = Q_k(theta, s)[a_n] - (float)y_k,  dc_k = clip(d_k)
//     dq[n][k A + a_n] = m_k(i_n) dc_k / K, zero elsewhere;  cost term = (sum_k m_k 0.5 d_k^2) / K, sum in head order
//     d4     = 1[a4 > 0] sum_k W5[k A + a_n] dq_k  over the rows with m_k = 1, in head order
//     maxq[n] = (float)((sum_k max_a Q_k(theta-, s')[a]) / K)
// m_k: bootstrap.h.  One 512-thread workgroup per sample, as head_kernel and munchausen_head_kernel (sdqn_munchausen.hip): the fc4 slab
// reduce + ReLU and the fc5 of slots 0 / 1 are the same loads, the same prod[][] transpose and the same single butterfly per row, over
// A' rows, so Q(pre), Q(post), a4 are what the standard head of an A'-action net leaves.  Thread 0 computes the K targets; the dq row
// replaces the (dead) target-net row in LDS and reaches the other threads with a bit mask of its live rows.  A kernel of its own name in
// a translation unit of its own: head_kernel's template list and instantiation set stay what they are; K, A, the mask threshold and
// seed and the index pointer are a third kernel argument (BootArgs), StepArgs and HeadArgs keep their layout.
// No scratch, no atomics; LDS = head_kernel's for the same bucket (minus one float).
#include "kernels.h"

namespace sdqn {
namespace {

template <int AMAX, bool NSTEP>
__global__ void __launch_bounds__(512) bootstrap_head_kernel(const StepArgs a, const HeadArgs h, const BootArgs b) {
  const int n = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6;
  __shared__ float prod[2 * AMAX][NFC];
  __shared__ float sh_q[2][AMAX];
  __shared__ int sh_rows;
  const int A = a.A;                                   // K A rows (a train step: nz = 2)
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
  int m_act = 0, m_term = 0; int64_t m_rew = 0, m_idx = 0;
  if (j == 0) {
    m_act = h.st_actions[n]; m_rew = h.st_rewards[n]; m_term = h.st_terminals[n];
    if (b.idx) m_idx = b.idx[n];
  }
  m_act = m_act < b.A ? m_act : b.A - 1;               // memory safety only: the host rejects out-of-range actions before launching
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
    const int act = m_act, term = m_term, K = b.K, GA = b.A; const int64_t rew = m_rew;
    double rr, gam;
    if constexpr (NSTEP) { rr = __builtin_bit_cast(double, rew); gam = h.gamma_n; }
    else {
      rr = (double)rew;
      rr = rr < h.min_reward ? h.min_reward : (rr > h.max_reward ? h.max_reward : rr);
      gam = h.discount;
    }
    const float fK = (float)K;
    double msum = 0.0; float cost = 0.0f; int rows = 0;
    for (int k = 0; k < K; ++k) {
      float* qp = sh_q[1] + k * GA;                    // Q-head k's slice of the target net's poststate row
      float m = qp[0];
      for (int c = 1; c < GA; ++c) m = fmaxf(m, qp[c]);
      msum += (double)m;
      const double y = term ? rr : rr + gam * (double)m;
      const float d = sh_q[0][k * GA + act] - (float)y;
      float dc = d;
      if (h.clip_error != 0.0f) dc = fminf(fmaxf(d, -h.clip_error), h.clip_error);
      const int live = bootstrap_mask_bit(b.mask_seed, b.thresh, m_idx, k);
      if (live) { cost += 0.5f * (d * d); rows |= 1 << (k * GA + act); }
      for (int c = 0; c < GA; ++c) qp[c] = (live && c == act) ? dc / fK : 0.0f;   // the slice is dead: it becomes the dq row's
    }
    h.cost_terms[n] = cost / fK;
    h.maxq[n] = (float)(msum / (double)K);
    sh_rows = rows;
  }
  __syncthreads();
  const int rows = sh_rows;
  // fc5 dgrad: delta4 = W5^T delta * 1[a4 > 0] over the live rows, in head order (W5 rows already in registers)
  float acc = 0.0f;
#pragma unroll
  for (int r = 0; r < AMAX; ++r) if ((rows >> r) & 1) acc += w5[0][r] * sh_q[1][r];
  const float d4v = a4v[0] > 0.0f ? acc : 0.0f;
  if (a.h16) a.h_d4[(int64_t)n * NFC + j] = (half_t)(d4v * a.loss_scale);     // fp16 mode: loss-scaled half delta
  else a.d4[(int64_t)n * NFC + j] = d4v;
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

// launch_head's branch for HeadArgs::train == 4 (a.nz = 2; a.A = K b.A)
hipError_t launch_head_bootstrap(const StepArgs& a, const HeadArgs& h, const BootArgs& b, hipStream_t s) {
  if (h.train != 4 || a.nz != 2 || a.bn || h.per_w || b.K < 1 || b.A < 1 || a.A != b.K * b.A || a.A > MAX_ACTIONS) return hipErrorInvalidValue;
  if (!b.idx && b.thresh < (1ull << 53)) return hipErrorInvalidValue;           // masks need the ring index
  const int bucket = a.A <= 4 ? 0 : (a.A <= 8 ? 1 : 2);
  const BootstrapHead k = h.nstep > 1 ? head_for<true>(bucket) : head_for<false>(bucket);
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
