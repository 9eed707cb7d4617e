// sdqn_shift.hip — random-shift augmentation (--random_shift P): shift_gather_kernel reads the replay ring's HBM mirror at the
// step's sampled indexes and writes the B shifted prestates and the B shifted poststates into the replay handle's device minibatch
// (pre | post, what sdqn_replay_gather fills); the step then reads that minibatch in place.  The draw and the clamp: shift.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "shift.h"
#include "launch.h"

namespace sdqn {

// One workgroup per (sample n, state s, frame j): grid (2 hist, B).  (dy, dx) is uniform over the workgroup — all frames of one state share
// it, the two states of a sample draw their own.  A frame of a multiple of 16 bytes on 16-byte aligned buffers goes by 16-byte pieces of the
// OUTPUT: a piece that lies in one output row and whose source columns need no clamp is one 16-byte load (at the source's own alignment)
// and one aligned 16-byte store; every other piece, and every frame of another size, goes byte by byte through the clamps.  No atomics, no
// LDS; every output byte is written by exactly one thread.
__global__ void __launch_bounds__(256) shift_gather_kernel(const ShiftArgs a) {
  const int n = blockIdx.y, s = (int)blockIdx.x / a.hist, j = (int)blockIdx.x % a.hist;
  int dy, dx;
  shift_draw(a.seed, a.step, (uint64_t)n, (uint64_t)s, a.P, dy, dx);
  if (j == 0 && threadIdx.x == 0) { a.shifts[(n * 2 + s) * 2] = (int8_t)dy; a.shifts[(n * 2 + s) * 2 + 1] = (int8_t)dx; }
  int64_t f = a.idx[n] - a.hist + j + (s ? a.post_off : 0);        // pre: frames idx - hist .. idx - 1, post: post_off further (problems.h soff)
  f = f < 0 ? 0 : (f >= a.size ? a.size - 1 : f);
  const int64_t frame = (int64_t)a.H * a.W;
  const uint8_t* src = a.ring + f * frame;
  uint8_t* dst = (s ? a.post : a.pre) + ((int64_t)n * a.hist + j) * frame;
  const int W = a.W, Hm = a.H - 1, Wm = a.W - 1;
  const bool vec = (frame & 15) == 0 && ((reinterpret_cast<uintptr_t>(a.pre) | reinterpret_cast<uintptr_t>(a.post)) & 15) == 0;
  if (vec) {
    for (int c = threadIdx.x; c < (int)(frame >> 4); c += 256) {
      const int o = c << 4, y = o / W, x = o - y * W;
      const int sy = shift_clamp(y + dy, Hm), sx = x + dx;
      if (x + 15 < W && sx >= 0 && sx + 15 <= Wm) {
        uint4 v;
        __builtin_memcpy(&v, src + (int64_t)sy * W + sx, 16);
        *reinterpret_cast<uint4*>(dst + o) = v;
      } else {
        int yi = y, xi = x;                                     // (walked, not divided: a piece crosses at most 16 row ends)
        const uint8_t* row = src + (int64_t)sy * W;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
          dst[o + i] = row[shift_clamp(xi + dx, Wm)];
          if (++xi == W) { xi = 0; ++yi; row = src + (int64_t)shift_clamp(yi + dy, Hm) * W; }
        }
      }
    }
  } else {
    for (int o = threadIdx.x; o < (int)frame; o += 256) {
      const int y = o / W, x = o - y * W;
      dst[o] = src[(int64_t)shift_clamp(y + dy, Hm) * W + shift_clamp(x + dx, Wm)];
    }
  }
}

hipError_t launch_shift_gather(const ShiftArgs& a, hipStream_t s) {
  SDQN_LAUNCH(shift_gather_kernel, dim3(2 * a.hist, a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sdqn
