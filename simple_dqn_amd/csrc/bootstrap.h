// bootstrap.h — Bootstrapped DQN, --bootstrap_heads K (Osband, Blundell, Pritzel and Van Roy 2016): the pure functions
// every layer shares, compiled for host and device.  Output row k A + a of a K-head net is Q-head k, action a.  For sample n, ring slot i_n:
//     y_k    = r_c + (terminal ? 0 : gamma max_a Q_k(theta-, s')[a])          (double from the stored Q; --n_step: R, done, gamma^n in their places)
//     d_k    = Q_k(theta, s)[a_n] - (T)y_k,  dc_k = clip(d_k)
//     dq[n][k A + a_n] = m_k(i_n) dc_k / K, zero elsewhere;  cost term = (sum_k m_k 0.5 d_k^2) / K, sum in head order
//     maxq[n] = (T)((sum_k max_a Q_k(theta-, s')[a]) / K)                                                              (bootstrap_sample)
//   mask   m_k(i) = 1 iff the 53-bit draw hash(mask_seed, ring index i, k) >> 11 lies below ceil(ldexp(P, 53)); P = 1: all ones, no hash
//   acting k(e, ep) = hash(head_seed, copy e, episode number ep) mod K
// with hash(s, a, b) three steps of the project's generator (stream.h: stream_next), the operands folded in between the steps, and
// mask_seed / head_seed streams 0 / 1 of the seed given to sdqn_net_set_bootstrap (stream_seed).  Nothing is stored: a transition
// keeps its mask for as long as it sits in its ring slot, a copy keeps its Q-head for as long as its episode counter stands.
#pragma once
#include <stdint.h>
#include "stream.h"
#include "td_rule.h"

namespace sdqn {

SDQN_HD uint64_t bootstrap_hash(uint64_t seed, uint64_t a, uint64_t b) {
  uint64_t s = seed;
  s = stream_next(s) ^ a;
  s = stream_next(s) ^ b;
  return stream_next(s);
}
SDQN_HD uint64_t bootstrap_mask_seed(uint64_t seed) { return stream_seed(seed, 0, 0); }
SDQN_HD uint64_t bootstrap_head_seed(uint64_t seed) { return stream_seed(seed, 0, 1); }
// thresh = ceil(ldexp(P, 53)); P = 1 gives 2^53, above every 53-bit draw
SDQN_HD int bootstrap_mask_bit(uint64_t mask_seed, uint64_t thresh, int64_t index, int k) {
  if (thresh >= (1ull << 53)) return 1;
  return (bootstrap_hash(mask_seed, (uint64_t)index, (uint64_t)k) >> 11) < thresh ? 1 : 0;
}
SDQN_HD int bootstrap_head_of(uint64_t head_seed, int K, uint64_t copy, uint64_t episode) {
  return K <= 1 ? 0 : (int)(bootstrap_hash(head_seed, copy, episode) % (uint64_t)K);
}
// majority vote of the K per-head greedy actions (first maximum, a NaN counts as one: sdqn_net_act_greedy's rule); votes[A] receives the
// counts, the winner is the lowest action with the most votes.  q: one raw row [K A]
template <typename T>
SDQN_HD int bootstrap_vote(const T* q, int K, int A, int* votes) {
  for (int a = 0; a < A; ++a) votes[a] = 0;
  for (int k = 0; k < K; ++k) {
    const T* r = q + k * A; int best = 0;
    for (int a = 1; a < A; ++a) if (r[a] > r[best] || (r[a] != r[a] && r[best] == r[best])) best = a;
    votes[best] += 1;
  }
  int win = 0;
  for (int a = 1; a < A; ++a) if (votes[a] > votes[win]) win = a;
  return win;
}

// The whole train rule on one sample, sequentially, Q-head by Q-head (the generic path's head branch and thread 0 of the tuned head).  Ops:
// how a maximum is taken and an error clipped (td_rule.h: CompareOps<T> on the generic path, FminmaxOps in the tuned head).  r: the clipped
// reward or the n-step return; gam: the discount or discount^n; clip: clip_error (0: none); index: the sample's ring slot.  dq[K A] receives
// the row and MAY BE q_post itself: a Q-head's slice of q_post is dead once its maximum is taken, which is how the tuned head reuses its
// LDS row.  *rows (may be nullptr) receives the bit mask of the dq rows that can be non-zero (K A <= 32 there), *maxq the mean of the K
// maxima; returns the cost term.
template <typename T, typename Ops>
SDQN_HD T bootstrap_sample(const T* q_pre, const T* q_post, int K, int A, int act, double r, int terminal, double gam, T clip,
                            uint64_t mask_seed, uint64_t thresh, int64_t index, T* dq, int* rows, T* maxq) {
  const T fK = (T)K;
  double msum = 0.0; T cost = (T)0;
  if (rows) *rows = 0;
  for (int k = 0; k < K; ++k) {
    const T* qp = q_post + k * A;
    T m = qp[0];
    for (int a = 1; a < A; ++a) m = Ops::max(m, qp[a]);
    msum += (double)m;
    const double y = terminal ? r : r + gam * (double)m;
    const T d = q_pre[k * A + act] - (T)y;
    const T dc = clip != (T)0 ? Ops::clip(d, clip) : d;
    const int live = bootstrap_mask_bit(mask_seed, thresh, index, k);
    if (live) { cost += (T)0.5 * (d * d); if (rows) *rows |= 1 << (k * A + act); }
    for (int a = 0; a < A; ++a) dq[k * A + a] = (live && a == act) ? dc / fK : (T)0;
  }
  *maxq = (T)(msum / (double)K);
  return cost / fK;
}

// what the bootstrap head and the select kernel get on top of the step's arguments (a kernel argument of their own: StepArgs and
// HeadArgs keep their byte layout)
struct BootArgs {
  int K, A;                      // Q-heads, the game's actions (the net has K A outputs)
  uint64_t thresh, mask_seed;    // ceil(ldexp(P, 53)), the mask stream's seed
  const int64_t* idx;            // [B] ring indexes of the step's samples; nullptr: tuple path (only with P = 1)
};

}  // namespace sdqn
