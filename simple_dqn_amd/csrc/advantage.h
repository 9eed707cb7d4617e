// advantage.h — advantage-learning targets, --advantage_learning / --persistent_advantage (Bellemare, Ostrovski, Guez, Thomas and Munos 2016,
// "Increasing the Action Gap"): the pure functions every layer shares, compiled for host and device.  With
// qbar(s) = Q(theta-, s) and alpha = advantage_learning:
//     gap(q, a) = max_k q[k] - q[a]                                                     (>= 0, exactly 0 when a is a maximiser)  (action_gap)
//     y_std[n]  = r_c[n] + (terminal ? 0 : gamma max_a qbar(s'_n)[a])                    (--n_step: R, done, gamma^n in their places)
//     y_AL[n]   = y_std[n] - alpha gap(qbar(s_n), a_n)                                   (on terminal transitions too)
//     y_PAL[n]  = terminal ? y_AL[n] : max(y_AL[n], y_std[n] - alpha gap(qbar(s'_n), a_n))          (persistent)     (advantage_target)
// all in double from the stored Q-values; T is their number type (float on the tuned path, float or double on the generic one).  maxq[n]
// receives max_a qbar(s'_n)[a], as the standard head's.
#pragma once
#include <stdint.h>
#include "hd.h"

namespace sdqn {

// max_k q[k] - q[act] of one Q row: every term is a stored value, so the gap of a maximiser is exactly +0.  The maximum is taken in double
// with a comparison on both paths
template <typename T>
SDQN_HD double action_gap(const T* q, int A, int act) {
  double v = (double)q[0];
  for (int k = 1; k < A; ++k) { const double x = (double)q[k]; v = x > v ? x : v; }
  return v - (double)q[act];
}
// The AL / PAL target from the standard one.  m_post is max_a qbar(s')[a] AS THE CALLER TOOK IT for y_std and maxq (the tuned head with
// fmaxf on floats, the generic head with comparisons in T: td_rule.h), q_post is the row qbar(s'): the gap of the poststate is
// m_post - q_post[act], so PAL reads the same maximum its y_std did
template <typename T>
SDQN_HD double advantage_target(double y_std, const T* q_pre, const T* q_post, int A, int act, double m_post, double alpha, int persistent,
                                 int terminal) {
  double y = y_std - alpha * action_gap(q_pre, A, act);
  if (persistent && !terminal) {                       // PAL: the better of leaving act now and repeating it in s'
    const double yp = y_std - alpha * (m_post - (double)q_post[act]);
    y = yp > y ? yp : y;
  }
  return y;
}

}  // namespace sdqn
