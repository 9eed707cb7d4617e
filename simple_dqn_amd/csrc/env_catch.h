// env_catch.h — the game "catch" (DESIGN.md §18): ONE definition in plain integer C++, compiled for the host (sdqn_env_* entry points,
// the host mirrors of the fused act step) and for the device (render and evaluation kernels of sdqn_env.hip), so both run the same
// text and agree bit for bit by construction.  No floating point, no library state: the environment owns its generator.
//
//   court   12 x 12 cells of ch = H / 12 by cw = W / 12 pixels (integer division); pixels outside 12 ch x 12 cw stay 0
//   state   ball (row, col, dx), paddle left edge p (3 cells wide on row 11, 0 <= p <= 9), balls landed in this episode, terminal flag,
//           64-bit generator state
//   act(a)  0 stay, 1 left, 2 right (clamped); then row += 1, col += dx with reflection at the side walls (dx flips).  Ball on row 11:
//           reward +1 if p <= col <= p + 2 else -1, balls += 1, terminal when balls == balls_per_episode, a new ball spawns at row 0
//           from ONE draw d: col = d % 12, dx = (d / 12) % 3 - 1.  Every other step: reward 0.
//   render  u8[H][W]: background 0, ball cell 255, paddle cells 128
#pragma once
#include <stdint.h>
#include "stream.h"

namespace sdqn {

constexpr int CATCH_CELLS = 12, CATCH_PADDLE = 3, CATCH_ACTIONS = 3;
constexpr int CATCH_BALL_PIXEL = 255, CATCH_PADDLE_PIXEL = 128;

struct CatchState {            // == sdqn_env_state (include/sdqn.h), 32 bytes
  int32_t row, col, dx, paddle, balls, terminal;
  uint64_t rng;
};

// the generator is stream.h's; catch_next is the games' name for one draw of it.  Generator `stream` (0 the game's, 1 the acting policy's,
// 2 the sticky one) of copy `e` of a vectorised call seeded with `seed` starts at stream_seed(seed, e, stream)
SDQN_HD uint64_t catch_next(uint64_t& s) { return stream_next(s); }
SDQN_HD void catch_spawn(CatchState& s) {
  const uint64_t d = catch_next(s.rng);
  s.row = 0; s.col = (int32_t)(d % CATCH_CELLS); s.dx = (int32_t)((d / CATCH_CELLS) % 3) - 1;
}
SDQN_HD void catch_restart(CatchState& s) {      // new episode; the generator goes on (no reseed)
  s.balls = 0; s.terminal = 0; s.paddle = 4;
  catch_spawn(s);
}
SDQN_HD void catch_init(CatchState& s, uint64_t seed) { s.rng = seed; catch_restart(s); }

SDQN_HD int catch_step(CatchState& s, int action, int balls_per_episode) {
  if (action == 1 && s.paddle > 0) s.paddle -= 1;
  if (action == 2 && s.paddle < CATCH_CELLS - CATCH_PADDLE) s.paddle += 1;
  s.row += 1; s.col += s.dx;
  if (s.col < 0) { s.col = -s.col; s.dx = -s.dx; }
  if (s.col > CATCH_CELLS - 1) { s.col = 2 * (CATCH_CELLS - 1) - s.col; s.dx = -s.dx; }
  if (s.row < CATCH_CELLS - 1) return 0;
  const int reward = (s.col >= s.paddle && s.col < s.paddle + CATCH_PADDLE) ? 1 : -1;
  s.balls += 1;
  if (s.balls >= balls_per_episode) s.terminal = 1;
  catch_spawn(s);
  return reward;
}

// what the renderer needs of a state, small enough to ride in kernel arguments
struct CatchView { int32_t row, col, paddle; };
SDQN_HD CatchView catch_view(const CatchState& s) { CatchView v; v.row = s.row; v.col = s.col; v.paddle = s.paddle; return v; }
// one pixel, as range tests on the cell rectangles (no division: the device calls this per byte); the ball is drawn over the paddle
SDQN_HD uint8_t catch_pixel(const CatchView& v, int y, int x, int ch, int cw) {
  if ((unsigned)(y - v.row * ch) < (unsigned)ch && (unsigned)(x - v.col * cw) < (unsigned)cw) return (uint8_t)CATCH_BALL_PIXEL;
  if ((unsigned)(y - (CATCH_CELLS - 1) * ch) < (unsigned)ch && (unsigned)(x - v.paddle * cw) < (unsigned)(CATCH_PADDLE * cw))
    return (uint8_t)CATCH_PADDLE_PIXEL;
  return 0;
}
// the whole frame on the host: the same rectangles, filled
SDQN_HD void catch_fill(uint8_t* out, int W, int y0, int x0, int h, int w, uint8_t value) {
  for (int y = y0; y < y0 + h; ++y)
    for (int x = x0; x < x0 + w; ++x) out[y * W + x] = value;
}
SDQN_HD void catch_render(const CatchView& v, uint8_t* out, int H, int W) {
  const int ch = H / CATCH_CELLS, cw = W / CATCH_CELLS;
  for (int i = 0; i < H * W; ++i) out[i] = 0;
  catch_fill(out, W, (CATCH_CELLS - 1) * ch, v.paddle * cw, ch, CATCH_PADDLE * cw, (uint8_t)CATCH_PADDLE_PIXEL);
  catch_fill(out, W, v.row * ch, v.col * cw, ch, cw, (uint8_t)CATCH_BALL_PIXEL);
}

// epsilon-greedy with the acting generator: one draw u; explore when (u >> 11) < thresh, thresh = ceil(epsilon * 2^53) (the 53-bit
// uniform (u >> 11) * 2^-53 < epsilon, in integers); only then a second draw picks the action, draw % A
SDQN_HD int catch_epsilon_greedy(uint64_t& act_rng, uint64_t thresh, int greedy, int A) {
  const uint64_t u = catch_next(act_rng);
  if ((u >> 11) < thresh) return (int)(catch_next(act_rng) % (uint64_t)A);
  return greedy;
}

// the game as the generic device code of sdqn_env.hip sees it: state, view, rules, renderer and tallies of one game
struct CatchCursor { int32_t y, x; };              // where a renderer stands; made once per 16-byte chunk, then walked byte by byte
struct CatchGame {
  typedef CatchState State;
  typedef CatchView View;
  typedef CatchCursor Cursor;
  static constexpr int ACTIONS = CATCH_ACTIONS, CELLS = CATCH_CELLS, VIEW_WORDS = 3;
  static constexpr const char* NAME = "catch";
  SDQN_HD static void init(State& s, uint64_t seed) { catch_init(s, seed); }
  SDQN_HD static void restart(State& s) { catch_restart(s); }
  SDQN_HD static int step(State& s, int action, int bpe, int& lost) {          // caught = reward > 0, missed = reward < 0
    const int reward = catch_step(s, action, bpe); lost = reward < 0; return reward;
  }
  SDQN_HD static View view(const State& s) { return catch_view(s); }
  SDQN_HD static bool valid(const State& s) {
    return s.row >= 0 && s.row < CATCH_CELLS && s.col >= 0 && s.col < CATCH_CELLS && s.dx >= -1 && s.dx <= 1 && s.paddle >= 0 &&
           s.paddle <= CATCH_CELLS - CATCH_PADDLE && s.balls >= 0 && (s.terminal == 0 || s.terminal == 1);
  }
  SDQN_HD static void render(const View& v, uint8_t* out, int H, int W) { catch_render(v, out, H, W); }
  SDQN_HD static void pack(const View& v, int* w) { w[0] = v.row; w[1] = v.col; w[2] = v.paddle; }
  SDQN_HD static View unpack(const int* w) { View v; v.row = w[0]; v.col = w[1]; v.paddle = w[2]; return v; }
  SDQN_HD static Cursor cursor(int y, int x, int, int) { Cursor c; c.y = y; c.x = x; return c; }
  SDQN_HD static void advance(Cursor& c, int W, int, int) { if (++c.x == W) { c.x = 0; ++c.y; } }
  SDQN_HD static uint8_t pixel(const View& v, const Cursor& c, int ch, int cw) { return catch_pixel(v, c.y, c.x, ch, cw); }
};

}  // namespace sdqn
