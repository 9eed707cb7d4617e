// bootstrap.h — Bootstrapped DQN, --bootstrap_heads K (Osband, Blundell, Pritzel and Van Roy 2016): the two pure functions
// every layer shares, compiled for host and device.  Output row k A + a of a K-head net is Q-head k, action a.
//   mask   m_k(i) = 1 iff the 53-bit draw hash(mask_seed, ring index i, k) >> 11 lies below ceil(ldexp(P, 53)); P = 1: all ones, no hash
//   acting k(e, ep) = hash(head_seed, copy e, episode number ep) mod K
// with hash(s, a, b) three steps of the project's splitmix64 (env_catch.h: catch_next), the operands folded in between the steps, and
// mask_seed / head_seed streams 0 / 1 of the seed given to sdqn_net_set_bootstrap (catch_stream_seed).  Nothing is stored: a transition
// keeps its mask for as long as it sits in its ring slot, a copy keeps its Q-head for as long as its episode counter stands.
#pragma once
#include <stdint.h>
#include "env_catch.h"

namespace sdqn {

CATCH_HD uint64_t bootstrap_hash(uint64_t seed, uint64_t a, uint64_t b) {
  uint64_t s = seed;
  s = catch_next(s) ^ a;
  s = catch_next(s) ^ b;
  return catch_next(s);
}
CATCH_HD uint64_t bootstrap_mask_seed(uint64_t seed) { return catch_stream_seed(seed, 0, 0); }
CATCH_HD uint64_t bootstrap_head_seed(uint64_t seed) { return catch_stream_seed(seed, 0, 1); }
// thresh = ceil(ldexp(P, 53)); P = 1 gives 2^53, above every 53-bit draw
CATCH_HD int bootstrap_mask_bit(uint64_t mask_seed, uint64_t thresh, int64_t index, int k) {
  if (thresh >= (1ull << 53)) return 1;
  return (bootstrap_hash(mask_seed, (uint64_t)index, (uint64_t)k) >> 11) < thresh ? 1 : 0;
}
CATCH_HD int bootstrap_head_of(uint64_t head_seed, int K, uint64_t copy, uint64_t episode) {
  return K <= 1 ? 0 : (int)(bootstrap_hash(head_seed, copy, episode) % (uint64_t)K);
}
// majority vote of the K per-head greedy actions (first maximum, a NaN counts as one: sdqn_net_act_greedy's rule); votes[A] receives the
// counts, the winner is the lowest action with the most votes.  q: one raw row [K A]
template <typename T>
CATCH_HD int bootstrap_vote(const T* q, int K, int A, int* votes) {
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

// what the bootstrap head and the select kernel get on top of the step's arguments (a kernel argument of their own: StepArgs and
// HeadArgs keep their byte layout)
struct BootArgs {
  int K, A;                      // Q-heads, the game's actions (the net has K A outputs)
  uint64_t thresh, mask_seed;    // ceil(ldexp(P, 53)), the mask stream's seed
  const int64_t* idx;            // [B] ring indexes of the step's samples; nullptr: tuple path (only with P = 1)
};

}  // namespace sdqn
