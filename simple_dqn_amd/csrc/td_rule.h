// td_rule.h — the standard TD rule of a train step (deepqnetwork.py:133-159) with its Double DQN and prioritized-replay forms, as the generic
// path computes it (generic_net.hip: head_kernel), and the two small things the option rules' headers share: the (reward, discount) of a
// sample and the two ways the paths take a maximum and clip an error.  Pure functions compiled for host and device; T is the
// network's number type.  head_kernel of sdqn_kernels.hip and head_body.h keep their own text.
//   m      = max_a qbar(s')[a], or (Double DQN) qbar(s')[first argmax_a Q(theta, s')[a]]                                 (td_post_value)
//   y      = r_c + (terminal ? 0 : gamma m), in double                       (--n_step: R, done, gamma^n in their places) (td_target)
//   d      = Q(theta, s)[a_n] - (T)y;  dq = clip(d) on the taken action, 0 elsewhere;  cost term = 0.5 d^2 before the clip
//   PER    : dq and the cost term times the importance weight w (clip first, then weight), priority (|d| + eps)^alpha     (td_sample)
#pragma once
#include <stdint.h>
#include <math.h>
#include "hd.h"

namespace sdqn {

// The two paths differ in how they take a maximum and clip an error, and a NaN can see it: the generic path compares (a NaN entry is
// skipped by the maximum unless it is the first, a NaN error passes the clip), the tuned heads use fmaxf / fminf (a NaN entry is always
// skipped, a NaN error becomes -clip).  A rule that needs either takes the variant as a template parameter; neither is the other's fallback.
template <typename T>
struct CompareOps {
  static SDQN_HD T max(T m, T v) { return v > m ? v : m; }
  static SDQN_HD T clip(T e, T c) { return e < -c ? -c : (e > c ? c : e); }
};
struct FminmaxOps {
  static SDQN_HD float max(float m, float v) { return fmaxf(m, v); }
  static SDQN_HD float clip(float e, float c) { return fminf(fmaxf(e, -c), c); }
};

// the reward and the discount of a target: the clipped reward and gamma, or (--n_step) the return R, which `rew` holds as a double's bits
// (clipped per step), and gamma^n.  The generic path's counterpart of head_body.h's head_reward
SDQN_HD void td_reward(int64_t rew, int nstep, double discount, double gamma_n, double minr, double maxr, double* r, double* gam) {
  if (nstep > 1) { *r = __builtin_bit_cast(double, rew); *gam = gamma_n; return; }
  const double x = (double)rew;
  *r = x < minr ? minr : (x > maxr ? maxr : x);                                // np.clip(rewards, min_reward, max_reward) :136
  *gam = discount;
}

// be.max(postq, axis=0) :124, or with q_sel = Q(theta, s') the target net's Q at the online net's first maximum
template <typename T>
SDQN_HD T td_post_value(const T* q_post, const T* q_sel, int A) {
  if (q_sel) {
    int best = 0; T bv = q_sel[0];
    for (int a = 1; a < A; ++a) { const T v = q_sel[a]; if (v > bv) { bv = v; best = a; } }
    return q_post[best];
  }
  T m = q_post[0];
  for (int a = 1; a < A; ++a) m = CompareOps<T>::max(m, q_post[a]);
  return m;
}
SDQN_HD double td_target(double r, int terminal, double gam, double m) { return terminal ? r : r + gam * m; }     // :139-143, python float arithmetic

// everything behind the target y: dq[A] receives the row, *prio (with per != 0) the new priority; returns the cost term.  w: the importance
// weight of a prioritized memory (per != 0), else unused
template <typename T>
SDQN_HD T td_sample(const T* q_pre, int A, int act, double y, T clip, int per, T w, double per_alpha, double per_eps, T* dq, float* prio) {
  const T target = (T)y;                                                       // stored into the backend dtype
  T d = (T)0;
  for (int a = 0; a < A; ++a) {
    T e = (a == act) ? q_pre[a] - target : (T)0;                               // deltas = preq - targets: 0 off the taken action
    if (a == act) d = e;
    if (clip != (T)0) e = CompareOps<T>::clip(e, clip);                        // :158-159
    if (per && a == act) e = w * e;                                            // clip, then weight
    dq[a] = e;
  }
  if (!per) return (T)0.5 * (d * d);                                           // SumSquared before the clip (A7) :154
  *prio = (float)pow(fabs((double)d) + per_eps, per_alpha);                    // unclipped |delta|
  return w * ((T)0.5 * (d * d));
}

}  // namespace sdqn
