// dueling.h — the dueling architecture, --dueling (Wang, Schaul, Hessel, van Hasselt, Lanctot and de Freitas 2016): the pure
// functions every layer shares, compiled for host and device.  A dueling net over A actions is a library net with A + 1 outputs: row 0 is
// V, row 1 + a is Adv_a.  The two streams are the two halves of fc4's H hidden units: V reads units j < H / 2 only, every Adv_a reads units
// j >= H / 2 only — fc5 is block-sparse, its other entries are exactly +0.0 and stay there (dueling_mask).  T is the network's number type
// (float on the tuned path, float or double on the generic one).
//   Q(s, a)  = (T)((V + Adv_a) - (sum_b Adv_b) / A), in double from the stored rows, the sum in action order          (dueling_q)
//   greedy   = the first a with the largest Q(s, a); `>` against the running best, as head_kernel's argmax: a NaN Q(a) is never chosen
//              over a number, a NaN Q(0) stays                                                                         (dueling_greedy)
//   dq       = c on row 0, c (1[b = a_n] - 1 / A) on row 1 + b: one multiply of c by a constant rounded once to T       (dueling_dq)
// A NaN anywhere in a row makes every Q(s, a) NaN (V enters all of them, every Adv_b enters the mean), so the rule above and np.argmax's
// (a NaN counts as a maximum: what the game kernels apply to the [A] rows dueling_q_kernel hands them) agree on every row without an
// infinity in it: both say action 0.
#pragma once
#include <stdint.h>
#include <math.h>
#include "hd.h"

namespace sdqn {

template <typename T>
SDQN_HD T dueling_q(const T* row, int A, int a) {
  double s = 0.0;
  for (int b = 0; b < A; ++b) s += (double)row[1 + b];
  return (T)(((double)row[0] + (double)row[1 + a]) - s / (double)A);
}
template <typename T>
SDQN_HD int dueling_greedy(const T* row, int A, T* q_best) {
  double s = 0.0;                                      // dueling_q's operations, the mean taken once
  for (int b = 0; b < A; ++b) s += (double)row[1 + b];
  const double mean = s / (double)A;
  int best = 0; T bv = (T)(((double)row[0] + (double)row[1]) - mean);
  for (int a = 1; a < A; ++a) { const T v = (T)(((double)row[0] + (double)row[1 + a]) - mean); if (v > bv) { bv = v; best = a; } }
  *q_best = bv;
  return best;
}
// the acting rule on one raw row [A + 1]: the greedy action above
template <typename T>
SDQN_HD int dueling_act(const T* row, int A) { T v; return dueling_greedy(row, A, &v); }
// fc5's block mask: 1 where entry (row, j) of the [A + 1][H] matrix belongs to the net, 0 where it is held at +0.0
SDQN_HD int dueling_mask(int row, int j, int H) { return row == 0 ? (j < H / 2) : (j >= H / 2); }
// the gradient into the A + 1 rows from c = dLoss / dQ(s, a_n)
template <typename T>
SDQN_HD void dueling_dq(T c, int A, int act, T* dq) {
  const T on = (T)(1.0 - 1.0 / (double)A), off = (T)(-1.0 / (double)A);
  dq[0] = c;
  for (int b = 0; b < A; ++b) dq[1 + b] = c * (b == act ? on : off);
}

// The whole rule on one sample, sequentially (the generic path's head branch and the host restatement sdqn_dueling_loss; the tuned head
// computes the same operations in the same order).  r: the clipped reward or the n-step return; gam: the discount or discount^n; clip:
// clip_error (0: none); per != 0: the importance weight w multiplies the cost term and the clipped error, *prio receives
// (|delta| + per_eps)^per_alpha of the unclipped error.  dq[A + 1] receives the row; returns the cost term; *y_out = (T)y,
// *delta_out = delta, *maxq = max_a Q(theta-, s', a).
template <typename T>
SDQN_HD T dueling_sample(const T* q_pre, const T* q_post, int A, int act, double r, int terminal, double gam, T clip, int per, T w,
                          double per_alpha, double per_eps, T* dq, T* y_out, T* delta_out, T* maxq, float* prio) {
  T m; dueling_greedy(q_post, A, &m);
  *maxq = m;
  const double y = terminal ? r : r + gam * (double)m;
  const T d = dueling_q(q_pre, A, act) - (T)y;
  T dc = d;
  if (clip != (T)0) { const T lo = d > -clip ? d : -clip; dc = lo < clip ? lo : clip; }      // fmin(fmax(d, -clip), clip): a NaN d gives -clip, as head_clip
  T cost = (T)0.5 * (d * d);
  if (per) {
    cost = w * cost; dc = w * dc;
    if (prio) *prio = (float)pow(fabs((double)d) + per_eps, per_alpha);
  }
  dueling_dq<T>(dc, A, act, dq);
  if (y_out) *y_out = (T)y;
  if (delta_out) *delta_out = d;
  return cost;
}

// what the dueling head and the generic head's branch get on top of the step's arguments (a kernel argument of their own: StepArgs and
// HeadArgs keep their byte layout)
struct DuelArgs {
  int on, A;                     // armed; the game's actions (the net has A + 1 outputs)
  float* step;                   // [2][B] the step's (float)y and delta (sdqn_net_debug_read "dueling_step"); nullptr: not kept
};

}  // namespace sdqn
