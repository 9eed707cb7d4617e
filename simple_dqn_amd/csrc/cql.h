// cql.h — conservative Q-learning, --cql_alpha (Kumar, Zhou, Tucker and Levine 2020, CQL(H) in its discrete form): the pure
// functions every layer shares, compiled for host and device.  The regulariser reads one row only, q = Q(theta, s_n), the online net on the
// prestate, which a train step already holds.  T is the network's number type (float on the tuned path, float or double on the generic one).
//   lse    = m + log(sum_k exp(q[k] - m)), m = max_k q[k]        double from the stored row, the sum in action order                (cql_lse)
//   pi[k]  = exp(q[k] - lse)
//   reg[k] = (T)(alpha (pi[k] - 1[k == a]))                       the regulariser's gradient into row k, rounded once               (cql_grad)
//   cost   = (T)(alpha (lse - q[a]))                              >= 0 up to rounding                                               (cql_cost)
// Every term of the sum lies in (0, 1] and the maximum's is 1: never inf, s >= 1, pi underflows to +0 far below the maximum.  With A = 1:
// exp(0) = 1, log(1) = +0, lse == q[0] and pi == 1 exactly, so reg and cost are +0.
#pragma once
#include <stdint.h>
#include <math.h>
#include "hd.h"

namespace sdqn {

template <typename T>
SDQN_HD double cql_lse(const T* q, int A) {
  double m = (double)q[0];
  for (int k = 1; k < A; ++k) { const double x = (double)q[k]; m = x > m ? x : m; }
  double s = 0.0;
  for (int k = 0; k < A; ++k) s += exp((double)q[k] - m);
  return m + log(s);
}
template <typename T>
SDQN_HD T cql_grad(const T* q, int k, int act, double lse, double alpha) {
  return (T)(alpha * (exp((double)q[k] - lse) - (k == act ? 1.0 : 0.0)));
}
template <typename T>
SDQN_HD T cql_cost(const T* q, int act, double lse, double alpha) { return (T)(alpha * (lse - (double)q[act])); }

// The whole rule on one sample, sequentially (the generic path's head branch and the host restatement sdqn_cql_loss; the tuned head computes
// the same operations, one action per lane).  y: the standard target, in double; clip: clip_error (0: none); w: the importance weight of a
// prioritized memory, else 1 (a product with 1 is exact: one text serves both).  The error is clipped first, then weighted.  dq[A] receives
// the row, *delta_out (may be nullptr) the unclipped error; returns the cost term.
template <typename T>
SDQN_HD T cql_sample(const T* q, int A, int act, double y, double alpha, T clip, T w, T* dq, T* delta_out) {
  const double lse = cql_lse(q, A);
  const T d = q[act] - (T)y;
  T dc = d;
  if (clip != (T)0) { const T lo = d > -clip ? d : -clip; dc = lo < clip ? lo : clip; }          // fmin(fmax(d, -clip), clip): a NaN d gives -clip, as head_clip
  for (int k = 0; k < A; ++k) {
    const T t = w * cql_grad<T>(q, k, act, lse, alpha);
    dq[k] = k == act ? t + w * dc : t;
  }
  if (delta_out) *delta_out = d;
  return w * ((T)0.5 * (d * d)) + w * cql_cost<T>(q, act, lse, alpha);
}

}  // namespace sdqn
