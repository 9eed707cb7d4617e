// quantile.h — quantile-regression DQN, --quantiles N (Dabney, Rowland, Bellemare and Munos 2018): the pure functions every
// layer shares, compiled for host and device.  Output row j A + a of an N-quantile net is quantile j of action a, at the midpoint
// tau_j = (2 j + 1) / (2 N).  T is the network's number type (float on the tuned path, float or double on the generic one).
//   m(a)        = (sum_j theta_j[a]) / N, in double, in quantile order                      (quantile_mean)
//   a*          = the first a with the largest m(a); `>` against the running best, as head_kernel's Double DQN argmax: a NaN m(a) is
//                 never chosen over a number, a NaN m(0) stays                              (quantile_greedy)
//   pair (j,j') : w = |tau_j - 1[delta > 0]| (strict), g = w clip(delta, -kappa, kappa) / kappa, rho = w L_kappa(delta) / kappa   (quantile_pair)
//   acting      : Q(s, a) = (sum_j theta_j[a]) / N as a sum of T in quantile order           (quantile_action_value)
#pragma once
#include <stdint.h>
#include "hd.h"

namespace sdqn {

template <typename T>
SDQN_HD T quantile_tau(int j, int N) { return (T)((double)(2 * j + 1) / (double)(2 * N)); }

template <typename T>
SDQN_HD double quantile_mean(const T* q, int N, int A, int a) {
  double s = 0.0;
  for (int j = 0; j < N; ++j) s += (double)q[j * A + a];
  return s / (double)N;
}
template <typename T>
SDQN_HD int quantile_greedy(const T* q, int N, int A, double* m_best) {
  int best = 0; double bv = quantile_mean(q, N, A, 0);
  for (int a = 1; a < A; ++a) { const double v = quantile_mean(q, N, A, a); if (v > bv) { bv = v; best = a; } }
  *m_best = bv;
  return best;
}
template <typename T>
SDQN_HD void quantile_pair(T delta, T tau, T kappa, T* g, T* rho) {
  const T w = delta > (T)0 ? (T)1 - tau : tau;
  const T ad = delta < (T)0 ? -delta : delta;
  const T dc = delta < -kappa ? -kappa : (delta > kappa ? kappa : delta);
  const T L = ad <= kappa ? (T)0.5 * (delta * delta) : kappa * (ad - (T)0.5 * kappa);
  *g = (w * dc) / kappa;
  *rho = (w * L) / kappa;
}
template <typename T>
SDQN_HD T quantile_action_value(const T* q, int N, int A, int a) {
  T s = (T)0;
  for (int j = 0; j < N; ++j) s += q[j * A + a];
  return s / (T)N;
}
// the acting rule on one raw row q[N A]: the first maximum of the action values, a NaN counts as one (sdqn_net_act_greedy's rule)
template <typename T>
SDQN_HD int quantile_act(const T* q, int N, int A) {
  int best = 0; T bv = quantile_action_value(q, N, A, 0);
  for (int a = 1; a < A; ++a) { const T v = quantile_action_value(q, N, A, a); if (v > bv || (v != v && bv == bv)) { bv = v; best = a; } }
  return best;
}

// The whole rule on one sample, sequentially (the generic path's head branch and the host restatement sdqn_quantile_loss; the tuned head
// spreads the same operations over threads, in the same order per result).  r: the clipped reward or the n-step return; gam: the discount
// or discount^n.  dq[N A] receives the row, targets[N] (may be null) the targets in T; returns the cost term, *maxq = (T) m(a*).
template <typename T>
SDQN_HD T quantile_sample(const T* q_pre, const T* q_post, int N, int A, int act, double r, int terminal, double gam, T kappa,
                           T* dq, T* targets, T* maxq) {
  double mb; const int as = quantile_greedy(q_post, N, A, &mb);
  *maxq = (T)mb;
  for (int i = 0; i < N * A; ++i) dq[i] = (T)0;
  const T nn = (T)(N * N);
  double cost = 0.0;
  for (int j = 0; j < N; ++j) {
    const T tau = quantile_tau<T>(j, N), th = q_pre[j * A + act];
    T s = (T)0;
    for (int jp = 0; jp < N; ++jp) {
      const double y = terminal ? r : r + gam * (double)q_post[jp * A + as];
      if (targets && j == 0) targets[jp] = (T)y;
      T g, rho; quantile_pair<T>(th - (T)y, tau, kappa, &g, &rho);
      s += g; cost += (double)rho;
    }
    dq[j * A + act] = s / nn;
  }
  return (T)(cost / (double)(N * N));
}

// what the quantile head and the generic head's branch get on top of the step's arguments (a kernel argument of their own: StepArgs and
// HeadArgs keep their byte layout)
struct QuantArgs {
  int N, A;                      // quantiles, the game's actions (the net has N A outputs)
  float* targets;                // [B][N] the step's targets as stored floats (sdqn_net_debug_read "quantile_targets"); nullptr: not kept
};

}  // namespace sdqn
