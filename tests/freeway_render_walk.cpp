// The device renderer's text on the host: every game's cursor / advance / pixel walked in 16-byte chunks exactly as render_chunk and
// render_bytes of csrc/sdqn_env.hip walk them (ONE division per chunk, first / W, then the cursor), against the game's host renderer
// (filled rectangles), byte for byte, at ten geometries x `states` states reached by a pseudo-random game.  The headers are plain
// C++ when no device compiler reads them, so this is the text the kernels run.  tests/test_freeway.py builds and runs it.
//   freeway_render_walk [states]      prints one line per game, exits 1 at the first differing byte
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "env_breakout.h"
#include "env_catch.h"
#include "env_freeway.h"

using namespace sdqn;

template <class G>
static void walk(const typename G::View& v, uint8_t* out, int H, int W) {
  const int frame = H * W, ch = H / G::CELLS, cw = W / G::CELLS;
  for (int first = 0; first < frame; first += 16) {
    const int y = first / W;
    typename G::Cursor c = G::cursor(y, first - y * W, ch, cw);
    for (int i = first; i < first + 16 && i < frame; ++i) {
      out[i] = G::pixel(v, c, ch, cw);
      G::advance(c, W, ch, cw);
    }
  }
}

static const int GEOMETRIES[10][2] = {{84, 84}, {12, 12}, {36, 38}, {96, 96}, {60, 52}, {13, 23}, {47, 12}, {12, 95}, {100, 31}, {210, 160}};

template <class G>
static int check(int states, int per_episode) {
  long bytes = 0;
  for (int g = 0; g < 10; ++g) {
    const int H = GEOMETRIES[g][0], W = GEOMETRIES[g][1];
    std::vector<uint8_t> a((size_t)H * W), b((size_t)H * W);
    typename G::State s;
    G::init(s, 1000 + g);
    uint64_t pol = 77 + g;
    for (int t = 0; t < states; ++t) {
      const typename G::View v = G::view(s);
      G::render(v, a.data(), H, W);
      walk<G>(v, b.data(), H, W);
      for (int i = 0; i < H * W; ++i)
        if (a[i] != b[i]) {
          printf("%s %d x %d state %d: byte %d (y %d, x %d) host %d walk %d\n", G::NAME, H, W, t, i, i / W, i % W, a[i], b[i]);
          return 1;
        }
      bytes += H * W;
      // mostly "up" / "left" every third state, so that freeway's chicken visits every row and breakout's wall opens
      int lost;
      const int action = (t % 3 == 0) ? 1 : (int)(catch_next(pol) % G::ACTIONS);
      G::step(s, action, per_episode, lost);
      if (s.terminal) G::restart(s);
    }
  }
  printf("%s: %d states at each of 10 geometries, %ld bytes equal\n", G::NAME, states, bytes);
  return 0;
}

int main(int argc, char** argv) {
  const int states = argc > 1 ? atoi(argv[1]) : 3000;
  if (check<FreewayGame>(states, 500)) return 1;
  if (check<BreakoutGame>(states, 30)) return 1;
  if (check<CatchGame>(states, 10)) return 1;
  return 0;
}
