// munchausen.h — Munchausen DQN targets, --munchausen (Vieillard, Pietquin and Geist 2020): the pure functions every layer
// shares, compiled for host and device.  With qbar(s) = Q(theta-, s), pi = softmax(qbar / tau) and (alpha, tau, l0) = munchausen_alpha /
// munchausen_tau / munchausen_clip:
//     lse(q) = v + tau log(sum_a exp((q[a] - v) / tau)),  v = max_a q[a]                 (sum in action order)              (soft_value)
//     V[n]   = lse(qbar(s'_n))                                                           (the soft value of the poststate)
//     m[n]   = alpha clip(qbar(s_n)[a_n] - lse(qbar(s_n)), l0, 0)                         (= alpha clip(tau ln pi(a_n | s_n))) (munchausen_bonus)
//     y[n]   = (r_c[n] + m[n]) + (terminal ? 0 : gamma V[n])                             (--n_step: R, done, gamma^n in their places) (munchausen_target)
// all in double from the stored Q-values; T is their number type (float on the tuned path, float or double on the generic one).  maxq[n]
// receives (T)V[n].  The bonus is added on terminal transitions too.
#pragma once
#include <stdint.h>
#include <math.h>
#include "hd.h"

namespace sdqn {

// lse of one Q row.  Every term of the sum lies in (0, 1] and the maximum's is 1: never inf, s >= 1.  A = 1: exp(0) = 1, log(1) = +0, so
// lse == q[0] exactly.  The maximum is taken in double with a comparison on both paths
template <typename T>
SDQN_HD double soft_value(const T* q, int A, double tau) {
  double v = (double)q[0];
  for (int k = 1; k < A; ++k) { const double x = (double)q[k]; v = x > v ? x : v; }
  double s = 0.0;
  for (int k = 0; k < A; ++k) s += exp(((double)q[k] - v) / tau);
  return v + tau * log(s);
}
// alpha clip(tau ln pi(act | s), l0, 0) from qbar(s): the log-policy term is <= 0 up to rounding and exactly 0 for a unique maximiser far
// above the rest
template <typename T>
SDQN_HD double munchausen_bonus(const T* q_pre, int A, int act, double alpha, double tau, double l0) {
  const double lp = (double)q_pre[act] - soft_value(q_pre, A, tau);
  return alpha * (lp < l0 ? l0 : (lp > 0.0 ? 0.0 : lp));
}
// the target y of one sample from the rows qbar(s) and qbar(s'); r: the clipped reward or the n-step return; gam: the discount or
// discount^n.  *V receives the soft value of the poststate
template <typename T>
SDQN_HD double munchausen_target(const T* q_pre, const T* q_post, int A, int act, double r, int terminal, double gam, double alpha, double tau,
                                  double l0, double* V) {
  *V = soft_value(q_post, A, tau);
  const double rm = r + munchausen_bonus(q_pre, A, act, alpha, tau, l0);      // the bonus is added on terminal transitions too
  return terminal ? rm : rm + gam * *V;
}

}  // namespace sdqn
