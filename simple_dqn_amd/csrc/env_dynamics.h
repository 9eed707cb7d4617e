// env_dynamics.h — frame skip and sticky actions for the library's games: ONE definition in plain integer C++, written
// against the game trait (CatchGame, BreakoutGame), compiled for the host (sdqn_env_step, the host mirror of the fused act step) and
// for the device (thread 0 of the eval / collect kernels of sdqn_env.hip), like env_catch.h.  No floating point, no library state.
//
//   frame_skip k   1 <= k <= 8: one agent step is up to k game ticks with the same chosen action; the rewards add up (|R| <= k);
//                  a tick that sets terminal ends the agent step
//   thresh_p       ceil(p 2^53) for repeat_action_probability p in [0, 1): before every tick ONE draw u of the copy's sticky generator
//                  (splitmix64, stream 2 of stream_seed); (u >> 11) < thresh_p: the tick executes `prev`, the action the last tick
//                  executed, instead of the chosen one.  thresh_p == 0 draws nothing: the generator never moves
//   prev           0 ("stay") after init and after every restart
// Only the state after the last tick is rendered; callers record the CHOSEN action.
#pragma once
#include "env_catch.h"

namespace sdqn {

constexpr int DYNAMICS_MAX_SKIP = 8;
constexpr uint64_t DYNAMICS_STICKY_STREAM = 2;       // stream_seed(seed, e, 2): the sticky generator of copy e

// one agent step; returns the summed reward R; caught / lost: ticks with a positive reward / that lost a ball (the tallies' per-tick rule)
template <class G>
SDQN_HD int dynamics_step(typename G::State& s, int32_t& prev, uint64_t& sticky_rng, int action, int bpe, int frame_skip, uint64_t thresh_p,
                           int& caught, int& lost) {
  int R = 0;
  caught = 0; lost = 0;
#pragma unroll 1
  for (int k = 0; k < frame_skip; ++k) {
    int exec = action;
    if (thresh_p > 0) {
      const uint64_t u = catch_next(sticky_rng);
      if ((u >> 11) < thresh_p) exec = prev;
    }
    int l;
    const int r = G::step(s, exec, bpe, l);
    prev = exec;
    R += r; caught += r > 0; lost += l;
    if (s.terminal) break;
  }
  return R;
}
// a new episode: the game's own restart, and the emulator's reset to no-op
template <class G>
SDQN_HD void dynamics_restart(typename G::State& s, int32_t& prev) { G::restart(s); prev = 0; }

}  // namespace sdqn
