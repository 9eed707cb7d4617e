// The counter-based generator and the net layout on their own: a host program that includes hd.h, stream.h and net_layout.h
// and nothing else of the project, and writes every seeded feature's derivation out of their functions alone — the keying schemes are
// restated here from the features' headers, so that a scheme that stopped being expressible in stream.h would show.
// tests/test_streams.py builds it, feeds it one request per line and holds the answers to tests/golden/stream_kat.json.
//   noisy seed step slot layer side i -> word        redo | reset seed event i L -> word, draw (float bits)
//   shift seed t n s P -> dy dx                      mask seed thresh index k -> bit          head seed K copy episode -> Q-head
//   game seed -> catch's first ball (col, dx), its generator after the draw, the sticky generator's start
//   layer L -> first index, bound (float bits)       layer_of i -> L                          units l -> units, first score
#include <stdio.h>
#include <string.h>

#include "../../simple_dqn_amd/csrc/hd.h"
#include "../../simple_dqn_amd/csrc/net_layout.h"
#include "../../simple_dqn_amd/csrc/stream.h"

using namespace sdqn;
typedef unsigned long long ull;

static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static uint64_t hash3(uint64_t s, uint64_t a, uint64_t b) {      // bootstrap.h: three steps, the operands folded in between
  s = stream_next(s) ^ a;
  s = stream_next(s) ^ b;
  return stream_next(s);
}

int main() {
  char what[32];
  ull a[6];
  while (scanf("%31s", what) == 1) {
    const int want = !strcmp(what, "noisy") ? 6 : !strcmp(what, "shift") ? 5 : !strcmp(what, "game") || !strcmp(what, "layer") || !strcmp(what, "layer_of") || !strcmp(what, "units") ? 1 : 4;
    for (int k = 0; k < want; ++k) if (scanf("%llu", &a[k]) != 1) return 2;
    if (!strcmp(what, "noisy")) {
      const uint64_t key = stream_keyed(stream_keyed(stream_keyed(a[0], 0), a[1]), 4 * a[2] + 2 * a[3] + a[4]);
      printf("%llu\n", (ull)stream_keyed(key, a[5]));
    } else if (!strcmp(what, "redo") || !strcmp(what, "reset")) {
      const uint64_t domain = what[2] == 's' ? 0x52455345545F5350ull : 0;      // reset.h: RESET_DOMAIN, "RESET_SP"
      const uint64_t w = stream_keyed(stream_keyed(stream_keyed(a[0], 0) ^ domain, a[1]), a[2]);
      printf("%llu %u\n", (ull)w, bits(init_draw(w, (int)a[3])));
    } else if (!strcmp(what, "shift")) {
      uint64_t g = stream_seed(stream_keyed(a[0], a[1]), a[2], a[3]);
      const uint64_t m = 2 * a[4] + 1;
      const int dy = (int)(stream_next(g) % m) - (int)a[4], dx = (int)(stream_next(g) % m) - (int)a[4];
      printf("%d %d\n", dy, dx);
    } else if (!strcmp(what, "mask")) {
      printf("%d\n", a[1] >= (1ull << 53) || (hash3(stream_seed(a[0], 0, 0), a[2], a[3]) >> 11) < a[1] ? 1 : 0);
    } else if (!strcmp(what, "head")) {
      printf("%d\n", (int)(hash3(stream_seed(a[0], 0, 1), a[2], a[3]) % a[1]));
    } else if (!strcmp(what, "game")) {
      uint64_t g = a[0];
      const uint64_t d = stream_next(g);
      printf("%d %d %llu %llu\n", (int)(d % 12), (int)((d / 12) % 3) - 1, (ull)g, (ull)stream_seed(a[0], 0, 2));
    } else if (!strcmp(what, "layer")) {
      printf("%lld %u\n", (long long)layer_first((int)a[0]), bits(init_bound((int)a[0])));
    } else if (!strcmp(what, "layer_of")) {
      printf("%d\n", layer_of((int64_t)a[0]));
    } else if (!strcmp(what, "units")) {
      printf("%d %d\n", a[0] < 4 ? relu_units((int)a[0]) : 0, relu_off((int)a[0]));
    } else return 2;
  }
  return 0;
}
