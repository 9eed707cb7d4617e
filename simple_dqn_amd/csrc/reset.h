// reset.h — periodic resets with shrink-and-perturb (--reset_interval; Nikishin et al. 2022, Ash & Adams 2020, D'Oro et al.
// 2023): the entry-to-layer map, the per-layer factor, the draw and the per-entry formula, ONE definition in plain C++, compiled for the host
// (sdqn_reset_apply_host, sdqn_reset_draw: the oracle's source of truth) and for the device (sdqn_reset.hip), like redo.h.
//
//   layers   l = 1..5: conv1, conv2, conv3, fc4, fc5; entry i of the flat weight buffer (problems.h: internal layouts) lies in the layer
//            whose [REDO_OFFl, REDO_OFFl+1) holds it (redo.h restates the boundaries; fc5 ends at n = REDO_OFF5 + 512 A)
//   factor   alpha_l = 0 for the last `layers` layers (l > 5 - layers), ALPHA for the others; a = (float)ALPHA, b = (float)(1.0 - ALPHA): the
//            subtraction in double, rounded once
//   entry    alpha_l == 1: never written, in any buffer | alpha_l == 0: theta = phi (the old value is not read: a NaN is healed) | else
//            theta = fmaf(a, theta, b * phi), b * phi rounded once.  theta_t takes the same formula with the SAME phi; state / state2 -> +0.0
//            wherever alpha_l < 1; the gradient buffer is nobody's business here
//   draw     phi = (u 2^-23 - 1) k as redo.h's draw, k = float(sqrt(3 / fan_in)), fan_in 256, 512, 576, 3136, 512 (fc5: deepqnetwork.py draws
//            every layer from U(-k, k) with fan_in = the second dimension of the affine layers' (out, in) shapes, 512 for fc5 whatever its rows);
//            u = the top 24 bits of redo_word(reset_key(seed, event), i)
//   key      reset_key = mix((mix(seed + G) ^ RESET_DOMAIN) + G (event + 1)), redo_key = mix(mix(seed + G) + G (event + 1)): mix is a bijection
//            of the 64-bit words and RESET_DOMAIN != 0, so under one seed the two keys of an event number differ, and with them the words of
//            every index i (mix(key + G (i + 1)) of two different keys)
//   range    the entries with alpha_l < 1 are one tail of the buffer: [reset_first(layers, ALPHA), n) — everything when ALPHA < 1, else the
//            last `layers` layers
#pragma once
#include <math.h>
#include "redo.h"

namespace sdqn {

constexpr int RESET_LAYERS = 5;
constexpr uint64_t RESET_DOMAIN = 0x52455345545F5350ull;      // "RESET_SP"

REDO_HD uint64_t reset_key(uint64_t seed, uint64_t event) { return redo_mix((redo_mix(seed + REDO_G) ^ RESET_DOMAIN) + REDO_G * (event + 1)); }
// first flat index of layer L = 1..5 (6: one past fc5 is the caller's n)
REDO_HD constexpr int64_t reset_off(int L) { return L <= 1 ? 0 : L == 2 ? REDO_OFF2 : L == 3 ? REDO_OFF3 : L == 4 ? REDO_OFF4 : REDO_OFF5; }
REDO_HD int reset_layer(int64_t i) { return i < REDO_OFF2 ? 1 : i < REDO_OFF3 ? 2 : i < REDO_OFF4 ? 3 : i < REDO_OFF5 ? 4 : 5; }
// k of layer L = 1..5: redo.h's for the four ReLU layers, fc5's fan_in is fc4's width (512, conv2's value)
REDO_HD float reset_bound(int L) { return L == 5 ? redo_bound(2) : redo_bound(L); }
REDO_HD float reset_draw(uint64_t key, uint64_t i, int L) {
  const float u = (float)(uint32_t)(redo_word(key, i) >> 40);      // < 2^24: exact
  const float t = u * 1.1920928955078125e-07f - 1.0f;              // u 2^-23 - 1 in [-1, 1): both operations exact
  return t * reset_bound(L);
}
// the two factors of a shrunk layer and what decides a layer's treatment
struct ResetRule {
  int layers;        // the last `layers` of the five are re-initialised in full
  double alpha;      // the others' factor, in [0, 1]
  float a, b;        // (float)alpha, (float)(1.0 - alpha)
};
REDO_HD ResetRule reset_rule(int layers, double alpha) { ResetRule r; r.layers = layers; r.alpha = alpha; r.a = (float)alpha; r.b = (float)(1.0 - alpha); return r; }
// 0: kept (alpha_l == 1) | 1: redrawn (alpha_l == 0) | 2: shrunk and perturbed
REDO_HD int reset_action(const ResetRule& r, int L) {
  if (L > RESET_LAYERS - r.layers || r.alpha == 0.0) return 1;
  return r.alpha == 1.0 ? 0 : 2;
}
REDO_HD int64_t reset_first(int layers, double alpha) { return alpha < 1.0 ? 0 : reset_off(RESET_LAYERS - layers + 1); }
REDO_HD bool reset_noop(int layers, double alpha) { return layers == 0 && alpha == 1.0; }
// the new value of an entry whose action is 1 or 2 (old: read only by action 2)
REDO_HD float reset_value(const ResetRule& r, int act, float old, float phi) {
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
    const int L = reset_layer(i), act = reset_action(r, L);
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
