// env_breakout.h — the game "breakout" (DESIGN.md §20): ONE definition in plain integer C++, compiled for the host (sdqn_env_* entry
// points, the host mirrors of the fused act step) and for the device (the breakout_* kernels of sdqn_env.hip), like env_catch.h, whose
// generator (stream.h, drawn from with catch_next) and epsilon-greedy rule it shares.  No floating point, no library state.
//
//   court   12 x 12 cells of ch = H / 12 by cw = W / 12 pixels (integer division); pixels outside 12 ch x 12 cw stay 0
//   state   ball (row, col, dx, dy), dx, dy in {-1, +1}; paddle left edge p (3 cells wide on row 11, 0 <= p <= 9); balls lost in this
//           episode; terminal flag; brick mask (bit 12 (r - 1) + c: a brick at row r in {1, 2, 3}, column c); 64-bit generator state
//   spawn   ONE draw d: row = 4, col = d % 12, dx = ((d / 12) & 1) ? +1 : -1, dy = +1
//   act(a)  0 stay, 1 left, 2 right (clamped); nc = col + dx with reflection at the side walls (dx flips); nr = row + dy, above the top
//           wall dy = +1 and nr = row + 1.  A brick at (nr, nc): it is cleared, reward +1, dy flips, the ball takes (row, nc) — unless
//           (row, nc) holds a brick too (inside the wall's rows): then it keeps (row, col) and dx flips as well.  The last brick: all
//           36 are set again, and a ball that would then stand inside the wall takes (4, nc) with dy = +1.  Else nr == 11:
//           on the paddle dy = -1, the ball takes (10, nc), dx = -1 / unchanged / +1 on the left / middle / right cell; beside it
//           balls += 1, terminal when balls >= balls_per_episode, a new ball spawns, the bricks stay.  Else the ball takes (nr, nc).
//           Only a brick gives a reward.
//   render  u8[H][W]: background 0, bricks 64, paddle cells 128, ball cell 255 (drawn last)
#pragma once
#include "env_catch.h"

namespace sdqn {

constexpr int BREAKOUT_CELLS = 12, BREAKOUT_PADDLE = 3, BREAKOUT_ACTIONS = 3;
constexpr int BREAKOUT_BRICK_ROWS = 3, BREAKOUT_SPAWN_ROW = 4;                    // bricks on rows 1 .. 3, a new ball below them
constexpr uint64_t BREAKOUT_WALL = (1ull << (BREAKOUT_BRICK_ROWS * BREAKOUT_CELLS)) - 1;
constexpr int BREAKOUT_BALL_PIXEL = 255, BREAKOUT_PADDLE_PIXEL = 128, BREAKOUT_BRICK_PIXEL = 64;

struct BreakoutState {         // == sdqn_env_state_breakout (include/sdqn.h), 48 bytes
  int32_t row, col, dx, dy, paddle, balls, terminal, pad;
  uint64_t bricks, rng;
};

SDQN_HD bool breakout_brick_row(int r) { return r >= 1 && r <= BREAKOUT_BRICK_ROWS; }
SDQN_HD uint64_t breakout_brick_bit(int r, int c) { return 1ull << (BREAKOUT_CELLS * (r - 1) + c); }

SDQN_HD void breakout_spawn(BreakoutState& s) {
  const uint64_t d = catch_next(s.rng);
  s.row = BREAKOUT_SPAWN_ROW; s.col = (int32_t)(d % BREAKOUT_CELLS); s.dx = ((d / BREAKOUT_CELLS) & 1) ? 1 : -1; s.dy = 1;
}
SDQN_HD void breakout_restart(BreakoutState& s) {      // new episode; the generator goes on (no reseed)
  s.balls = 0; s.terminal = 0; s.paddle = 4; s.pad = 0; s.bricks = BREAKOUT_WALL;
  breakout_spawn(s);
}
SDQN_HD void breakout_init(BreakoutState& s, uint64_t seed) { s.rng = seed; breakout_restart(s); }

// returns the reward (1: a brick broke); lost = 1 when the ball passed the paddle
SDQN_HD int breakout_step(BreakoutState& s, int action, int balls_per_episode, int& lost) {
  lost = 0;
  if (action == 1 && s.paddle > 0) s.paddle -= 1;
  if (action == 2 && s.paddle < BREAKOUT_CELLS - BREAKOUT_PADDLE) s.paddle += 1;
  int nc = s.col + s.dx;
  if (nc < 0) { nc = -nc; s.dx = -s.dx; }
  if (nc > BREAKOUT_CELLS - 1) { nc = 2 * (BREAKOUT_CELLS - 1) - nc; s.dx = -s.dx; }
  int nr = s.row + s.dy;
  if (nr < 0) { s.dy = 1; nr = s.row + 1; }
  if (breakout_brick_row(nr) && (s.bricks & breakout_brick_bit(nr, nc))) {
    s.bricks &= ~breakout_brick_bit(nr, nc);
    s.dy = -s.dy;
    if (breakout_brick_row(s.row) && (s.bricks & breakout_brick_bit(s.row, nc))) s.dx = -s.dx;      // (row, nc) is a brick too: back the way it came
    else s.col = nc;
    if (s.bricks == 0) {
      s.bricks = BREAKOUT_WALL;
      if (breakout_brick_row(s.row)) { s.row = BREAKOUT_SPAWN_ROW; s.dy = 1; }
    }
    return 1;
  }
  if (nr == BREAKOUT_CELLS - 1) {
    const int k = nc - s.paddle;
    if (k >= 0 && k < BREAKOUT_PADDLE) {
      s.dy = -1; s.row = BREAKOUT_CELLS - 2; s.col = nc;
      if (k == 0) s.dx = -1;
      if (k == BREAKOUT_PADDLE - 1) s.dx = 1;
      return 0;
    }
    lost = 1;
    s.balls += 1;
    if (s.balls >= balls_per_episode) s.terminal = 1;
    breakout_spawn(s);
    return 0;
  }
  s.row = nr; s.col = nc;
  return 0;
}

// what the renderer needs of a state, small enough to ride in kernel arguments
struct BreakoutView { int32_t row, col, paddle; uint64_t bricks; };
SDQN_HD BreakoutView breakout_view(const BreakoutState& s) {
  BreakoutView v; v.row = s.row; v.col = s.col; v.paddle = s.paddle; v.bricks = s.bricks; return v;
}

// Where a renderer stands: pixel (y, x), the cell column cx of x and x's offset rx inside that cell (cx >= 12: right of the court).  The
// device makes one per 16-byte chunk (ONE division, first / W, by the caller; cx by four comparisons) and walks it byte by byte.
struct BreakoutCursor { int32_t y, x, cx, rx; };
SDQN_HD BreakoutCursor breakout_cursor(int y, int x, int cw) {
  int cx = 0;                                            // floor(x / cw), capped at 12, by bisection over the 13 cell boundaries
  if (x >= 8 * cw) cx = 8;
  if (x >= (cx + 4) * cw) cx += 4;
  if (x >= (cx + 2) * cw) cx += 2;
  if (x >= (cx + 1) * cw) cx += 1;
  if (cx > BREAKOUT_CELLS) cx = BREAKOUT_CELLS;
  BreakoutCursor c; c.y = y; c.x = x; c.cx = cx; c.rx = x - cx * cw; return c;
}
SDQN_HD void breakout_advance(BreakoutCursor& c, int W, int cw) {
  if (++c.x == W) { c.x = 0; c.cx = 0; c.rx = 0; ++c.y; return; }
  if (++c.rx == cw && c.cx < BREAKOUT_CELLS) { c.rx = 0; ++c.cx; }
}
// one pixel, by comparisons only (the device calls this per byte): rows as range tests on y, columns through the cursor's cell column
SDQN_HD uint8_t breakout_pixel(const BreakoutView& v, const BreakoutCursor& c, int ch) {
  if ((unsigned)c.cx >= (unsigned)BREAKOUT_CELLS) return 0;
  if (c.cx == v.col && (unsigned)(c.y - v.row * ch) < (unsigned)ch) return (uint8_t)BREAKOUT_BALL_PIXEL;
  if (c.y >= ch && c.y < (BREAKOUT_BRICK_ROWS + 1) * ch) {
    const int r = (c.y >= 2 * ch) + (c.y >= 3 * ch);     // brick row - 1
    return ((v.bricks >> (BREAKOUT_CELLS * r + c.cx)) & 1) ? (uint8_t)BREAKOUT_BRICK_PIXEL : (uint8_t)0;
  }
  if ((unsigned)(c.y - (BREAKOUT_CELLS - 1) * ch) < (unsigned)ch && (unsigned)(c.cx - v.paddle) < (unsigned)BREAKOUT_PADDLE)
    return (uint8_t)BREAKOUT_PADDLE_PIXEL;
  return 0;
}
// the whole frame on the host: the same rectangles, filled
SDQN_HD void breakout_render(const BreakoutView& v, uint8_t* out, int H, int W) {
  const int ch = H / BREAKOUT_CELLS, cw = W / BREAKOUT_CELLS;
  for (int i = 0; i < H * W; ++i) out[i] = 0;
  for (int r = 1; r <= BREAKOUT_BRICK_ROWS; ++r)
    for (int c = 0; c < BREAKOUT_CELLS; ++c)
      if (v.bricks & breakout_brick_bit(r, c)) catch_fill(out, W, r * ch, c * cw, ch, cw, (uint8_t)BREAKOUT_BRICK_PIXEL);
  catch_fill(out, W, (BREAKOUT_CELLS - 1) * ch, v.paddle * cw, ch, BREAKOUT_PADDLE * cw, (uint8_t)BREAKOUT_PADDLE_PIXEL);
  catch_fill(out, W, v.row * ch, v.col * cw, ch, cw, (uint8_t)BREAKOUT_BALL_PIXEL);
}

// every field in range, no brick bit above bit 35, the ball on rows 0 .. 10 and in no brick cell
SDQN_HD bool breakout_state_valid(const BreakoutState& s) {
  if (s.row < 0 || s.row > BREAKOUT_CELLS - 2 || s.col < 0 || s.col >= BREAKOUT_CELLS) return false;
  if ((s.dx != 1 && s.dx != -1) || (s.dy != 1 && s.dy != -1)) return false;
  if (s.paddle < 0 || s.paddle > BREAKOUT_CELLS - BREAKOUT_PADDLE || s.balls < 0 || (s.terminal != 0 && s.terminal != 1) || s.pad != 0) return false;
  if (s.bricks & ~BREAKOUT_WALL) return false;
  if (breakout_brick_row(s.row) && (s.bricks & breakout_brick_bit(s.row, s.col))) return false;
  return true;
}

// the game as the generic device code of sdqn_env.hip sees it
struct BreakoutGame {
  typedef BreakoutState State;
  typedef BreakoutView View;
  typedef BreakoutCursor Cursor;
  static constexpr int ACTIONS = BREAKOUT_ACTIONS, CELLS = BREAKOUT_CELLS, VIEW_WORDS = 5;
  static constexpr const char* NAME = "breakout";
  SDQN_HD static void init(State& s, uint64_t seed) { breakout_init(s, seed); }
  SDQN_HD static void restart(State& s) { breakout_restart(s); }
  SDQN_HD static int step(State& s, int action, int bpe, int& lost) { return breakout_step(s, action, bpe, lost); }   // caught = bricks broken, missed = balls lost
  SDQN_HD static View view(const State& s) { return breakout_view(s); }
  SDQN_HD static bool valid(const State& s) { return breakout_state_valid(s); }
  SDQN_HD static void render(const View& v, uint8_t* out, int H, int W) { breakout_render(v, out, H, W); }
  SDQN_HD static void pack(const View& v, int* w) { w[0] = v.row; w[1] = v.col; w[2] = v.paddle; w[3] = (int)(uint32_t)v.bricks; w[4] = (int)(uint32_t)(v.bricks >> 32); }
  SDQN_HD static View unpack(const int* w) {
    View v; v.row = w[0]; v.col = w[1]; v.paddle = w[2]; v.bricks = (uint64_t)(uint32_t)w[3] | ((uint64_t)(uint32_t)w[4] << 32); return v;
  }
  SDQN_HD static Cursor cursor(int y, int x, int ch, int cw) { (void)ch; return breakout_cursor(y, x, cw); }
  SDQN_HD static void advance(Cursor& c, int W, int ch, int cw) { (void)ch; breakout_advance(c, W, cw); }
  SDQN_HD static uint8_t pixel(const View& v, const Cursor& c, int ch, int cw) { (void)cw; return breakout_pixel(v, c, ch); }
};

}  // namespace sdqn
