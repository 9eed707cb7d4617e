// shift.h — random-shift augmentation (--random_shift P): the draw and the clamp, ONE definition in plain integer C++,
// compiled for the host (sdqn_random_shift_draw, the setter's checks) and for the device (shift_gather_kernel of sdqn_shift.hip), like
// env_dynamics.h.  No floating point, no library state.
//
//   shift   sample n of train step t, state s (0 prestate, 1 poststate) draws (dy, dx) in [-P, P]^2; output pixel (y, x) of every frame of
//           that state is input pixel (clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1)): replicate-padding by P, crop at (P + dy, P + dx)
//   stream  the project's generator (stream.h) started at
//             k  = stream_keyed(seed, t)          = mix(seed + G (t + 1))
//             s0 = stream_seed(k, n, s)           = mix(k + STREAM_MUL (2 n + s + 1))
//           the first output z0 gives dy = (int)(z0 % (2P + 1)) - P, the second z1 gives dx likewise
#pragma once
#include "stream.h"

namespace sdqn {

constexpr int SHIFT_MAX_PAD = 8;

SDQN_HD uint64_t shift_stream(uint64_t seed, uint64_t step, uint64_t n, uint64_t s) {
  return stream_seed(stream_keyed(seed, step), n, s);
}
SDQN_HD void shift_draw(uint64_t seed, uint64_t step, uint64_t n, uint64_t s, int P, int& dy, int& dx) {
  uint64_t g = shift_stream(seed, step, n, s);
  const uint64_t m = (uint64_t)(2 * P + 1);
  dy = (int)(stream_next(g) % m) - P;
  dx = (int)(stream_next(g) % m) - P;
}
SDQN_HD int shift_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// sdqn_shift.hip: one launch writes the B shifted prestates and the B shifted poststates of the step into pre | post
struct ShiftArgs {
  const uint8_t* ring;          // [size][H][W] the replay ring's HBM mirror
  const int64_t* idx;           // [B] the step's sampled indexes (device memory, or the device alias of a pinned slot)
  uint8_t* pre; uint8_t* post;  // [B][hist][H][W] each
  int8_t* shifts;               // [B][2][2] the (dy, dx) drawn per sample and state, for sdqn_net_last_shifts
  int64_t size;                 // ring slots: a frame number outside [0, size) is clamped into it (the host has checked the indexes)
  uint64_t seed, step;
  int B, hist, H, W, P, post_off;   // post_off: the poststate starts this many frames after the prestate (--n_step n, else 1)
};
hipError_t launch_shift_gather(const ShiftArgs& a, hipStream_t s);

}  // namespace sdqn
