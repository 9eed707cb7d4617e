// head_rules.cpp — the TD head's rule headers on the host, for tests/test_head_rules.py: plain C entry points that run
// each rule over a batch of float or double rows, composed the way generic_net.hip's head_kernel composes them.
#include "../../simple_dqn_amd/csrc/td_rule.h"
#include "../../simple_dqn_amd/csrc/munchausen.h"
#include "../../simple_dqn_amd/csrc/advantage.h"
#include "../../simple_dqn_amd/csrc/bootstrap.h"

using namespace sdqn;

namespace {

template <typename T>
void munchausen(const T* q_pre, const T* q_post, int B, int A, const int* act, const int64_t* rew, const int* term, int nstep, double discount,
                double gamma_n, double minr, double maxr, double alpha, double tau, double l0, double* y, double* V, double* bonus) {
  for (int n = 0; n < B; ++n) {
    double r, gam; td_reward(rew[n], nstep, discount, gamma_n, minr, maxr, &r, &gam);
    y[n] = munchausen_target<T>(q_pre + n * A, q_post + n * A, A, act[n], r, term[n], gam, alpha, tau, l0, V + n);
    bonus[n] = munchausen_bonus<T>(q_pre + n * A, A, act[n], alpha, tau, l0);
  }
}
template <typename T>
void advantage(const T* q_pre, const T* q_post, int B, int A, const int* act, const int64_t* rew, const int* term, int nstep, double discount,
               double gamma_n, double minr, double maxr, double alpha, int persistent, double* y, T* maxq) {
  for (int n = 0; n < B; ++n) {
    double r, gam; td_reward(rew[n], nstep, discount, gamma_n, minr, maxr, &r, &gam);
    const T m = td_post_value<T>(q_post + n * A, nullptr, A);
    maxq[n] = m;
    y[n] = advantage_target<T>(td_target(r, term[n], gam, (double)m), q_pre + n * A, q_post + n * A, A, act[n], (double)m, alpha, persistent, term[n]);
  }
}
template <typename T, typename Ops>
void bootstrap(const T* q_pre, const T* q_post, int B, int K, int A, const int* act, const int64_t* rew, const int* term, int nstep, double discount,
               double gamma_n, double minr, double maxr, T clip, uint64_t seed, uint64_t thresh, const int64_t* idx, T* dq, T* cost, T* maxq, int* rows) {
  for (int n = 0; n < B; ++n) {
    double r, gam; td_reward(rew[n], nstep, discount, gamma_n, minr, maxr, &r, &gam);
    cost[n] = bootstrap_sample<T, Ops>(q_pre + n * K * A, q_post + n * K * A, K, A, act[n], r, term[n], gam, clip, bootstrap_mask_seed(seed), thresh,
                                       idx ? idx[n] : 0, dq + n * K * A, rows + n, maxq + n);
  }
}
template <typename T>
void td(const T* q_pre, const T* q_post, const T* q_sel, int B, int A, const int* act, const int64_t* rew, const int* term, int nstep, double discount,
        double gamma_n, double minr, double maxr, T clip, const float* per_w, double per_alpha, double per_eps, T* dq, T* cost, T* maxq, float* prio,
        double* y) {
  for (int n = 0; n < B; ++n) {
    double r, gam; td_reward(rew[n], nstep, discount, gamma_n, minr, maxr, &r, &gam);
    maxq[n] = td_post_value<T>(q_post + n * A, q_sel ? q_sel + n * A : nullptr, A);
    y[n] = td_target(r, term[n], gam, (double)maxq[n]);
    cost[n] = td_sample<T>(q_pre + n * A, A, act[n], y[n], clip, per_w != nullptr, per_w ? (T)per_w[n] : (T)1, per_alpha, per_eps, dq + n * A,
                           per_w ? prio + n : nullptr);
  }
}

}  // namespace

#define RULES(S, T)                                                                                                                                    \
  extern "C" void hr_munchausen_##S(const T* q_pre, const T* q_post, int B, int A, const int* act, const int64_t* rew, const int* term, int nstep,        \
                                    double discount, double gamma_n, double minr, double maxr, double alpha, double tau, double l0, double* y, double* V, \
                                    double* bonus) {                                                                                                    \
    munchausen<T>(q_pre, q_post, B, A, act, rew, term, nstep, discount, gamma_n, minr, maxr, alpha, tau, l0, y, V, bonus);                               \
  }                                                                                                                                                     \
  extern "C" void hr_advantage_##S(const T* q_pre, const T* q_post, int B, int A, const int* act, const int64_t* rew, const int* term, int nstep,         \
                                   double discount, double gamma_n, double minr, double maxr, double alpha, int persistent, double* y, T* maxq) {         \
    advantage<T>(q_pre, q_post, B, A, act, rew, term, nstep, discount, gamma_n, minr, maxr, alpha, persistent, y, maxq);                                 \
  }                                                                                                                                                     \
  extern "C" void hr_bootstrap_##S(const T* q_pre, const T* q_post, int B, int K, int A, const int* act, const int64_t* rew, const int* term, int nstep,  \
                                   double discount, double gamma_n, double minr, double maxr, double clip, uint64_t seed, uint64_t thresh,               \
                                   const int64_t* idx, T* dq, T* cost, T* maxq, int* rows) {                                                             \
    bootstrap<T, CompareOps<T>>(q_pre, q_post, B, K, A, act, rew, term, nstep, discount, gamma_n, minr, maxr, (T)clip, seed, thresh, idx, dq, cost,       \
                                maxq, rows);                                                                                                             \
  }                                                                                                                                                     \
  extern "C" void hr_td_##S(const T* q_pre, const T* q_post, const T* q_sel, int B, int A, const int* act, const int64_t* rew, const int* term,           \
                            int nstep, double discount, double gamma_n, double minr, double maxr, double clip, const float* per_w, double per_alpha,      \
                            double per_eps, T* dq, T* cost, T* maxq, float* prio, double* y) {                                                           \
    td<T>(q_pre, q_post, q_sel, B, A, act, rew, term, nstep, discount, gamma_n, minr, maxr, (T)clip, per_w, per_alpha, per_eps, dq, cost, maxq, prio, y); \
  }
RULES(f, float)
RULES(d, double)

// the tuned heads' variant of the bootstrap rule (fmaxf / fminf), float rows only
extern "C" void hr_bootstrap_fminmax_f(const float* q_pre, const float* q_post, int B, int K, int A, const int* act, const int64_t* rew, const int* term,
                                       int nstep, double discount, double gamma_n, double minr, double maxr, double clip, uint64_t seed, uint64_t thresh,
                                       const int64_t* idx, float* dq, float* cost, float* maxq, int* rows) {
  bootstrap<float, FminmaxOps>(q_pre, q_post, B, K, A, act, rew, term, nstep, discount, gamma_n, minr, maxr, (float)clip, seed, thresh, idx, dq, cost,
                               maxq, rows);
}
