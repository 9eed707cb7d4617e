// reset.h — periodic resets with shrink-and-perturb (--reset_interval; Nikishin et al. 2022, Ash & Adams 2020, D'Oro et al.
// 2023): the entry-to-layer map, the per-layer factor, the draw and the per-entry formula, ONE definition in plain C++, compiled for the host
// (sdqn_reset_apply_host, sdqn_reset_draw: the oracle's source of truth) and for the device (sdqn_reset.hip), like redo.h.
//
//   layers   l = 1..5: conv1, conv2, conv3, fc4, fc5; entry i of the flat weight buffer (problems.h: internal layouts) lies in the layer
//            layer_of(i) (net_layout.h; fc5 ends at n = OFF5 + 512 A)
//   factor   alpha_l = 0 for the last `layers` layers (l > 5 - layers), ALPHA for the others; a = (float)ALPHA, b = (float)(1.0 - ALPHA): the
//            subtraction in double, rounded once
//   entry    alpha_l == 1: never written, in any buffer | alpha_l == 0: theta = phi (the old value is not read: a NaN is healed) | else
//            theta = fmaf(a, theta, b * phi), b * phi rounded once.  theta_t takes the same formula with the SAME phi; state / state2 -> +0.0
//            wherever alpha_l < 1; the gradient buffer is nobody's business here
//   draw     phi = init_draw(w, l) = (u 2^-23 - 1) k (net_layout.h), k = float(sqrt(3 / fan_in)), fan_in 256, 512, 576, 3136, 512 (fc5:
//            deepqnetwork.py draws every layer from U(-k, k) with fan_in = the second dimension of the affine layers' (out, in) shapes, 512 for
//            fc5 whatever its rows); u = the top 24 bits of w = stream_keyed(reset_key(seed, event), i)
//   key      reset_key = mix((mix(seed + G) ^ RESET_DOMAIN) + G (event + 1)), redo_key = mix(mix(seed + G) + G (event + 1)): mix is a bijection
//            of the 64-bit words and RESET_DOMAIN != 0, so under one seed the two keys of an event number differ, and with them the words of
//            every index i (mix(key + G (i + 1)) of two different keys)
//   range    the entries with alpha_l < 1 are one tail of the buffer: [reset_first(layers, ALPHA), n) — everything when ALPHA < 1, else the
//            last `layers` layers
#pragma once
#include <math.h>
#include "net_layout.h"
#include "stream.h"

namespace sdqn {

constexpr int RESET_LAYERS = NET_LAYERS;
constexpr uint64_t RESET_DOMAIN = 0x52455345545F5350ull;      // "RESET_SP"

SDQN_HD uint64_t reset_key(uint64_t seed, uint64_t event) { return stream_keyed(stream_keyed(seed, 0) ^ RESET_DOMAIN, event); }
SDQN_HD float reset_draw(uint64_t key, uint64_t i, int L) { return init_draw(stream_keyed(key, i), L); }
// the two factors of a shrunk layer and what decides a layer's treatment
struct ResetRule {
  int layers;        // the last `layers` of the five are re-initialised in full
  double alpha;      // the others' factor, in [0, 1]
  float a, b;        // (float)alpha, (float)(1.0 - alpha)
};
SDQN_HD ResetRule reset_rule(int layers, double alpha) { ResetRule r; r.layers = layers; r.alpha = alpha; r.a = (float)alpha; r.b = (float)(1.0 - alpha); return r; }
// 0: kept (alpha_l == 1) | 1: redrawn (alpha_l == 0) | 2: shrunk and perturbed
SDQN_HD int reset_action(const ResetRule& r, int L) {
  if (L > RESET_LAYERS - r.layers || r.alpha == 0.0) return 1;
  return r.alpha == 1.0 ? 0 : 2;
}
SDQN_HD int64_t reset_first(int layers, double alpha) { return alpha < 1.0 ? 0 : layer_first(RESET_LAYERS - layers + 1); }
SDQN_HD bool reset_noop(int layers, double alpha) { return layers == 0 && alpha == 1.0; }
// the new value of an entry whose action is 1 or 2 (old: read only by action 2)
SDQN_HD float reset_value(const ResetRule& r, int act, float old, float phi) {
  if (act == 1) return phi;
  const float bp = r.b * phi;                                      // rounded once
  return fmaf(r.a, old, bp);                                       // one fused multiply-add
}
// one event on host arrays: theta / theta_t (may alias theta or be NULL: one write) / state / state2 (may be NULL) [n] in place
inline void reset_apply_host(int layers, double alpha, uint64_t seed, uint64_t event, int64_t n, float* theta, float* theta_t, float* state, float* state2) {
  const ResetRule r = reset_rule(layers, alpha);
  const uint64_t key = reset_key(seed, event);
  if (theta_t == theta) theta_t = nullptr;
  for (int64_t i = reset_first(layers, alpha); i < n; ++i) {
    const int L = layer_of(i), act = reset_action(r, L);
    if (!act) continue;
    const float phi = reset_draw(key, (uint64_t)i, L);
    theta[i] = reset_value(r, act, theta[i], phi);
    if (theta_t) theta_t[i] = reset_value(r, act, theta_t[i], phi);
    if (state) state[i] = 0.0f;
    if (state2) state2[i] = 0.0f;
  }
}

// sdqn_reset.hip
struct ResetApplyArgs {
  float* theta; float* theta_t;             // [n]; theta_t == theta or NULL: one net
  float* state; float* state2;              // [n]; state2 may be NULL
  int64_t n;
  int layers; double alpha;
  uint64_t seed, event; int64_t step;
  int64_t* info;                            // [2] event, step (written by workgroup 0)
};

#if defined(__HIPCC__)
hipError_t launch_reset_apply(const ResetApplyArgs& a, hipStream_t s);
#endif

}  // namespace sdqn
