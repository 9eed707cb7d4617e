// env_freeway.h — the game "freeway" (DESIGN.md §25): ONE definition in plain integer C++, compiled for the host (sdqn_env_* entry
// points, the host mirrors of the fused act step) and for the device (the freeway_* kernels of sdqn_env.hip), like env_catch.h, whose
// generator (stream.h, drawn from with catch_next) and epsilon-greedy rule it shares.  No floating point, no library state.
//
//   court   12 x 12 cells of ch = H / 12 by cw = W / 12 pixels (integer division); pixels outside 12 ch x 12 cw stay 0
//   state   the chicken's row (0 .. 11; its column is always 6); game ticks played in this episode; crossings made in it; terminal flag;
//           two padding words kept at 0; for each traffic row r = 1 .. 10 the nibble r - 1 of three 64-bit words: the car's column
//           (cars, 0 .. 11), the ticks until it moves (timers, 1 .. period) and its period (periods, 1 .. 5); 64-bit generator state.
//           Odd rows drive right (+1), even rows left (-1); columns wrap modulo 12
//   shuffle ONE draw d; for r = 1 .. 10 in order: period = 1 + d % 5, d /= 5; col = d % 12, d /= 12; timer = period (60^10 < 2^64).
//           A car of row 10 drawn onto column 6 takes column 7
//   step(a) 0 stay, 1 up, 2 down (clamped to rows 0 .. 11).  (1) the chicken moves; (2) on row 0: reward +1, crossings += 1, the
//           chicken is back on row 11, shuffle, and the cars do not move in this tick; (3) else on a traffic row whose car stands on
//           column 6, it walked into a car: back to row 11, lost = 1; (5) unless (2): every timer -= 1, at 0 the car moves one cell in its
//           row's direction and timer = period; then, when nothing was lost in (3) and the chicken stands on a traffic row whose car is
//           now on column 6, a car drove into it: back to row 11, lost = 1; (6) ticks += 1, terminal when ticks >= episode_ticks.
//           Only a crossing gives a reward: a hit costs position
//   render  u8[H][W]: background 0, cars 128, the chicken's cell 255 (drawn last)
#pragma once
#include "env_catch.h"

namespace sdqn {

constexpr int FREEWAY_CELLS = 12, FREEWAY_ACTIONS = 3, FREEWAY_COLUMN = 6;      // the chicken's column
constexpr int FREEWAY_FIRST_LANE = 1, FREEWAY_LAST_LANE = 10, FREEWAY_START_ROW = 11, FREEWAY_MAX_PERIOD = 5;
constexpr uint64_t FREEWAY_LANE_BITS = (1ull << (4 * (FREEWAY_LAST_LANE - FREEWAY_FIRST_LANE + 1))) - 1;      // the 40 bits the ten nibbles take
constexpr int FREEWAY_CHICKEN_PIXEL = 255, FREEWAY_CAR_PIXEL = 128;

struct FreewayState {          // == sdqn_env_state_freeway (include/sdqn.h), 56 bytes
  int32_t row, ticks, crossings, terminal, pad0, pad1;
  uint64_t cars, timers, periods, rng;
};

SDQN_HD bool freeway_lane(int r) { return r >= FREEWAY_FIRST_LANE && r <= FREEWAY_LAST_LANE; }
SDQN_HD int freeway_nibble(uint64_t w, int r) { return (int)((w >> (4 * (r - FREEWAY_FIRST_LANE))) & 15); }
SDQN_HD uint64_t freeway_with_nibble(uint64_t w, int r, int v) {
  const int sh = 4 * (r - FREEWAY_FIRST_LANE);
  return (w & ~(15ull << sh)) | ((uint64_t)v << sh);
}
// whether the car of traffic row `row` stands on the chicken's column (false on rows 0 and 11, which have no car)
SDQN_HD bool freeway_car_at_chicken(uint64_t cars, int row) { return freeway_lane(row) && freeway_nibble(cars, row) == FREEWAY_COLUMN; }

SDQN_HD void freeway_shuffle(FreewayState& s) {
  uint64_t d = catch_next(s.rng);
  uint64_t cars = 0, periods = 0;
  for (int r = FREEWAY_FIRST_LANE; r <= FREEWAY_LAST_LANE; ++r) {
    const int period = 1 + (int)(d % FREEWAY_MAX_PERIOD); d /= FREEWAY_MAX_PERIOD;
    int col = (int)(d % FREEWAY_CELLS); d /= FREEWAY_CELLS;
    if (r == FREEWAY_LAST_LANE && col == FREEWAY_COLUMN) col = FREEWAY_COLUMN + 1;
    cars = freeway_with_nibble(cars, r, col); periods = freeway_with_nibble(periods, r, period);
  }
  s.cars = cars; s.periods = periods; s.timers = periods;
}
SDQN_HD void freeway_restart(FreewayState& s) {       // new episode; the generator goes on (no reseed)
  s.row = FREEWAY_START_ROW; s.ticks = 0; s.crossings = 0; s.terminal = 0; s.pad0 = 0; s.pad1 = 0;
  freeway_shuffle(s);
}
SDQN_HD void freeway_init(FreewayState& s, uint64_t seed) { s.rng = seed; freeway_restart(s); }

// returns the reward (1: a crossing); lost = 1 when the chicken was hit
SDQN_HD int freeway_step(FreewayState& s, int action, int episode_ticks, int& lost) {
  lost = 0;
  int reward = 0;
  if (action == 1 && s.row > 0) s.row -= 1;
  if (action == 2 && s.row < FREEWAY_CELLS - 1) s.row += 1;
  if (s.row == 0) {
    reward = 1; s.crossings += 1; s.row = FREEWAY_START_ROW;
    freeway_shuffle(s);
  } else {
    if (freeway_car_at_chicken(s.cars, s.row)) { s.row = FREEWAY_START_ROW; lost = 1; }
    uint64_t cars = s.cars, timers = s.timers;
    for (int r = FREEWAY_FIRST_LANE; r <= FREEWAY_LAST_LANE; ++r) {
      int t = freeway_nibble(timers, r) - 1;
      if (t <= 0) {
        int c = freeway_nibble(cars, r) + ((r & 1) ? 1 : -1);
        if (c < 0) c = FREEWAY_CELLS - 1;
        if (c > FREEWAY_CELLS - 1) c = 0;
        cars = freeway_with_nibble(cars, r, c);
        t = freeway_nibble(s.periods, r);
      }
      timers = freeway_with_nibble(timers, r, t);
    }
    s.cars = cars; s.timers = timers;
    if (!lost && freeway_car_at_chicken(s.cars, s.row)) { s.row = FREEWAY_START_ROW; lost = 1; }
  }
  s.ticks += 1;
  if (s.ticks >= episode_ticks) s.terminal = 1;
  return reward;
}

// what the renderer needs of a state, small enough to ride in kernel arguments
struct FreewayView { int32_t row; uint64_t cars; };
SDQN_HD FreewayView freeway_view(const FreewayState& s) { FreewayView v; v.row = s.row; v.cars = s.cars & FREEWAY_LANE_BITS; return v; }

// floor(x / c), capped at 12, by bisection over the 13 cell boundaries (four comparisons, no division)
SDQN_HD int freeway_cell(int x, int c) {
  int k = 0;
  if (x >= 8 * c) k = 8;
  if (x >= (k + 4) * c) k += 4;
  if (x >= (k + 2) * c) k += 2;
  if (x >= (k + 1) * c) k += 1;
  return k > FREEWAY_CELLS ? FREEWAY_CELLS : k;
}
// Where a renderer stands: pixel (y, x), the cell column cx of x with x's offset rx inside it and the cell row cy of y with y's offset ry
// (cx, cy >= 12: right of / below the court).  The device makes one per 16-byte chunk (ONE division, first / W, by the caller; cx and cy by
// four comparisons each: the range tests on y that find a pixel's traffic row) and walks it byte by byte.
struct FreewayCursor { int32_t y, x, cx, rx, cy, ry; };
SDQN_HD FreewayCursor freeway_cursor(int y, int x, int ch, int cw) {
  FreewayCursor c; c.y = y; c.x = x;
  c.cx = freeway_cell(x, cw); c.rx = x - c.cx * cw;
  c.cy = freeway_cell(y, ch); c.ry = y - c.cy * ch;
  return c;
}
SDQN_HD void freeway_advance(FreewayCursor& c, int W, int ch, int cw) {
  if (++c.x == W) {
    c.x = 0; c.cx = 0; c.rx = 0; ++c.y;
    if (++c.ry == ch && c.cy < FREEWAY_CELLS) { c.ry = 0; ++c.cy; }
    return;
  }
  if (++c.rx == cw && c.cx < FREEWAY_CELLS) { c.rx = 0; ++c.cx; }
}
// one pixel, by comparisons and shifts only (the device calls this per byte)
SDQN_HD uint8_t freeway_pixel(const FreewayView& v, const FreewayCursor& c) {
  if ((unsigned)c.cx >= (unsigned)FREEWAY_CELLS || (unsigned)c.cy >= (unsigned)FREEWAY_CELLS) return 0;
  if (c.cy == v.row && c.cx == FREEWAY_COLUMN) return (uint8_t)FREEWAY_CHICKEN_PIXEL;
  if ((unsigned)(c.cy - FREEWAY_FIRST_LANE) <= (unsigned)(FREEWAY_LAST_LANE - FREEWAY_FIRST_LANE) &&
      (int)((v.cars >> (4 * (c.cy - FREEWAY_FIRST_LANE))) & 15) == c.cx)
    return (uint8_t)FREEWAY_CAR_PIXEL;
  return 0;
}
// the whole frame on the host: the same rectangles, filled
SDQN_HD void freeway_render(const FreewayView& v, uint8_t* out, int H, int W) {
  const int ch = H / FREEWAY_CELLS, cw = W / FREEWAY_CELLS;
  for (int i = 0; i < H * W; ++i) out[i] = 0;
  for (int r = FREEWAY_FIRST_LANE; r <= FREEWAY_LAST_LANE; ++r)
    catch_fill(out, W, r * ch, freeway_nibble(v.cars, r) * cw, ch, cw, (uint8_t)FREEWAY_CAR_PIXEL);
  catch_fill(out, W, v.row * ch, FREEWAY_COLUMN * cw, ch, cw, (uint8_t)FREEWAY_CHICKEN_PIXEL);
}

// every field in range, every nibble in range (column <= 11, 1 <= timer <= period <= 5), no bit above the ten nibbles, the padding
// zero, the chicken in no car's cell.  `ticks` has no upper bound: the episode length is the handle's, not the state's
SDQN_HD bool freeway_state_valid(const FreewayState& s) {
  if (s.row < 0 || s.row >= FREEWAY_CELLS || s.ticks < 0 || s.crossings < 0 || (s.terminal != 0 && s.terminal != 1)) return false;
  if (s.pad0 != 0 || s.pad1 != 0) return false;
  if ((s.cars | s.timers | s.periods) & ~FREEWAY_LANE_BITS) return false;
  for (int r = FREEWAY_FIRST_LANE; r <= FREEWAY_LAST_LANE; ++r) {
    const int col = freeway_nibble(s.cars, r), t = freeway_nibble(s.timers, r), p = freeway_nibble(s.periods, r);
    if (col >= FREEWAY_CELLS || t < 1 || t > p || p > FREEWAY_MAX_PERIOD) return false;
  }
  return !freeway_car_at_chicken(s.cars, s.row);
}

// the game as the generic device code of sdqn_env.hip sees it; the trait's third step argument carries episode_ticks
struct FreewayGame {
  typedef FreewayState State;
  typedef FreewayView View;
  typedef FreewayCursor Cursor;
  static constexpr int ACTIONS = FREEWAY_ACTIONS, CELLS = FREEWAY_CELLS, VIEW_WORDS = 3;
  static constexpr const char* NAME = "freeway";
  SDQN_HD static void init(State& s, uint64_t seed) { freeway_init(s, seed); }
  SDQN_HD static void restart(State& s) { freeway_restart(s); }
  SDQN_HD static int step(State& s, int action, int episode_ticks, int& lost) { return freeway_step(s, action, episode_ticks, lost); }   // caught = crossings, missed = hits
  SDQN_HD static View view(const State& s) { return freeway_view(s); }
  SDQN_HD static bool valid(const State& s) { return freeway_state_valid(s); }
  SDQN_HD static void render(const View& v, uint8_t* out, int H, int W) { freeway_render(v, out, H, W); }
  SDQN_HD static void pack(const View& v, int* w) { w[0] = v.row; w[1] = (int)(uint32_t)v.cars; w[2] = (int)(uint32_t)(v.cars >> 32); }
  SDQN_HD static View unpack(const int* w) { View v; v.row = w[0]; v.cars = (uint64_t)(uint32_t)w[1] | ((uint64_t)(uint32_t)w[2] << 32); return v; }
  SDQN_HD static Cursor cursor(int y, int x, int ch, int cw) { return freeway_cursor(y, x, ch, cw); }
  SDQN_HD static void advance(Cursor& c, int W, int ch, int cw) { freeway_advance(c, W, ch, cw); }
  SDQN_HD static uint8_t pixel(const View& v, const Cursor& c, int ch, int cw) { (void)ch; (void)cw; return freeway_pixel(v, c); }
};

}  // namespace sdqn
