// regularize.h — decoupled weight decay and L2-init regularisation (--weight_decay WD, --l2_init LAMBDA; Loshchilov & Hutter 2019,
// Kumar, Marklund & Van Roy 2023): the two coefficients and the per-weight rule, ONE definition in plain C++, compiled for the host
// (sdqn_regularize_apply_host: the oracle's source of truth) and for the device (sdqn_regularize.hip), like reset.h.
//
//   weights  the n = OFF5 + 512 A values of the online net's flat buffer, all five layers
//   factors  kf = (float)(1.0 - lr WD), cf = (float)(lr LAMBDA): double arithmetic, rounded once; lr = the net's learning_rate
//   rule     v = theta[e];  WD > 0: v = v * kf;  LAMBDA > 0: v = v + cf * (anchor[e] - v);  theta[e] = v — every operation rounded on its own,
//            never contracted (numpy float32 reproduces the bits).  A coefficient of 0 skips its line: no multiplication by 1.0f, no anchor read
//   ranges   WD >= 0, LAMBDA >= 0, lr WD < 1, lr LAMBDA <= 1 (reg_range_error names the first one violated; a NaN violates)
#pragma once
#include "net_layout.h"

namespace sdqn {

struct RegRule {
  float kf, cf;      // (float)(1.0 - lr * wd), (float)(lr * lambda)
  int wd_on, l2_on;  // wd > 0, lambda > 0
};
SDQN_HD RegRule reg_rule(double wd, double lambda, double lr) {
  RegRule r; r.kf = (float)(1.0 - lr * wd); r.cf = (float)(lr * lambda); r.wd_on = wd > 0.0; r.l2_on = lambda > 0.0; return r;
}
// 0: fine | 1: WD < 0 | 2: LAMBDA < 0 | 3: lr WD >= 1 | 4: lr LAMBDA > 1 (each comparison is written so that a NaN fails it)
SDQN_HD int reg_range_error(double wd, double lambda, double lr) {
  if (!(wd >= 0.0)) return 1;
  if (!(lambda >= 0.0)) return 2;
  if (!(lr * wd < 1.0)) return 3;
  if (!(lr * lambda <= 1.0)) return 4;
  return 0;
}
// one rounding per operation on both sides: the device names the instructions, the host is compiled with -ffp-contract=off
#if defined(__HIP_DEVICE_COMPILE__)
SDQN_HD float reg_mul(float a, float b) { return __fmul_rn(a, b); }
SDQN_HD float reg_add(float a, float b) { return __fadd_rn(a, b); }
SDQN_HD float reg_sub(float a, float b) { return __fsub_rn(a, b); }
#else
SDQN_HD float reg_mul(float a, float b) { volatile float p = a * b; return p; }
SDQN_HD float reg_add(float a, float b) { volatile float s = a + b; return s; }
SDQN_HD float reg_sub(float a, float b) { volatile float d = a - b; return d; }
#endif
SDQN_HD float reg_decay(const RegRule& r, float v) { return reg_mul(v, r.kf); }
SDQN_HD float reg_pull(const RegRule& r, float v, float anchor) { return reg_add(v, reg_mul(r.cf, reg_sub(anchor, v))); }
// the rule on host arrays: theta [n] in place, anchor [n] read when lambda > 0 only (may be NULL otherwise)
inline void reg_apply_host(double wd, double lambda, double lr, int64_t n, float* theta, const float* anchor) {
  const RegRule r = reg_rule(wd, lambda, lr);
  for (int64_t e = 0; e < n; ++e) {
    float v = theta[e];
    if (r.wd_on) v = reg_decay(r, v);
    if (r.l2_on) v = reg_pull(r, v, anchor[e]);
    theta[e] = v;
  }
}

constexpr int REG_LAYERS = NET_LAYERS;
constexpr int REG_NORM_BLOCKS = 64;        // partial sums per layer and quantity (sdqn_regularize.hip: weight_norms)
constexpr int REG_NORM_DOUBLES = 2 * REG_LAYERS * REG_NORM_BLOCKS + 2 * REG_LAYERS;   // partials | the ten results

// sdqn_regularize.hip
struct RegularizeArgs {
  float* theta;                 // [n] the online weights, regularised in place
  const float* anchor;          // [n], read when rule.l2_on only
  int64_t n;                    // OFF5 + 512 A
  RegRule rule;
  void* wh; void* wht;          // float16 nets: the ONLINE net's half copies (master layout / transposed), else nullptr
  unsigned short* w1p;          // float32 nets: the ONLINE net's three bf16 planes of W1, else nullptr
  // the fused form with --target_tau: theta_t != nullptr blends theta- toward the new theta and writes the target's derived copies too
  float* theta_t; float tau;
  void* wh_t; void* wht_t; unsigned short* w1p_t;
  int tiles; int64_t flat_first;   // (filled in by launch_regularize, as launch_target_blend does)
};
struct WeightNormArgs {
  const float* theta; const float* anchor;   // [n]; anchor may be NULL: the five distances are not computed
  int64_t n;
  double* buf;                  // [REG_NORM_DOUBLES]
};

#if defined(__HIPCC__)
hipError_t launch_regularize(RegularizeArgs a, hipStream_t s);
hipError_t launch_weight_norms(const WeightNormArgs& a, hipStream_t s);      // two launches: per-block partials, then the fold
#endif

}  // namespace sdqn
