// route.cpp — resolve_route (simple_dqn_amd/csrc/launch_route.h) behind a C interface for tests/test_launch_route.py: built with g++, no HIP.
#include "../../simple_dqn_amd/csrc/launch_route.h"

using namespace sdqn;

extern "C" {

int route_kernel_count() { return K_COUNT; }
const char* route_unit(int u) { return route_unit_name((RouteUnit)u); }
const char* route_form(int f) { return route_form_name((RouteForm)f); }

// One id under one set of options over a list of batch sizes x (f4w_count 0 / > 0) x (from_ring 0 / 1) x (host indexes without / with), in
// that order: out[((b * 2 + f4w) * 2 + ring) * 2 + hidx][3] = {unit, form, rides_in}.
// key = {nz, h16, bn, tps1, has_src, has_w1p}; bt[K_COUNT], nw[12].
void route_rows(int id, const int* key, const int* bt, const int* nw, int wt, int variant, int nB, const int* Bs, int* out) {
  LaunchTune t = {};
  for (int i = 0; i < K_COUNT; ++i) t.bt[i] = bt[i];
  for (int i = 0; i < 12; ++i) t.nw_override[i] = nw[i];
  t.wt = wt; t.variant = variant;
  static const int64_t some_idx[32] = {0};
  for (int b = 0; b < nB; ++b) for (int f4w = 0; f4w < 2; ++f4w) for (int ring = 0; ring < 2; ++ring) for (int hidx = 0; hidx < 2; ++hidx) {
    t.host_idx = hidx ? some_idx : nullptr;
    const RouteKey k = {Bs[b], key[0], key[1], key[2], f4w ? 1568 : 0, ring, key[3], key[4] != 0, key[5] != 0, hidx != 0};
    const Route r = resolve_route(id, k, t);
    *out++ = r.unit; *out++ = r.form; *out++ = r.rides_in;
  }
}

}
