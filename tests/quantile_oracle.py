"""Quantile-regression DQN (--quantiles N) restated in numpy scalars and Python floats (test helper, not product code).

The net has N A outputs; output row j A + a is quantile j of action a, at the midpoint tau_j = (2 j + 1) / (2 N).  t is the network's
number type; "double" is a Python float.  For sample n:

    m(a)       = (sum_j theta_j(theta-, s')[a]) / N          double, summed in quantile order from the stored Q
    a*         = the first a with the largest m(a): `>` against the running best (a NaN m(a) is never chosen over a number, a NaN m(0) stays)
    maxq[n]    = t(m(a*))
    T_j'       = r_c + (terminal ? 0 : gamma theta_j'(theta-, s')[a*])          double from the stored Q; stored as t
    delta_jj'  = theta_j(theta, s)[a_n] - t(T_j')
    w_jj'      = 1 - tau_j if delta_jj' > 0 else tau_j       (= |tau_j - 1[delta > 0]|, the indicator strict)
    g_jj'      = (w_jj' clip(delta_jj', -kappa, kappa)) / kappa
    rho_jj'    = (w_jj' L_kappa(delta_jj')) / kappa,  L_kappa(d) = 0.5 d^2 if |d| <= kappa else kappa (|d| - 0.5 kappa)
    dq[n][j A + a_n] = (sum_j' g_jj') / t(N^2), the sum in t in j' order; zero elsewhere
    cost term  = t((sum_jj' rho_jj') / N^2), the sum in double in j-major order;  cost = the mean of the terms
    (n_step > 1: R, done, gamma^n in the places of r_c, terminal, gamma)

    acting: Q(s, a) = (sum_j theta_j(s)[a]) / t(N), a sum of t in quantile order; then np.argmax (the first maximum, a NaN counts as one)

The mean over the N^2 pairs divides the paper's loss (sum over j, mean over j') by N once more.
"""
import numpy as np

from nstep_oracle import gamma_n
from oracle.dqn_numpy import CONV, OracleDQN, _col2im

GAP = 1e-4                      # every oracle comparison asks that a sample's best and second-best m(a) differ by more than this


def tau(j, N, t=np.float32):
    return t((2 * j + 1) / (2.0 * N))


def means(q_post_row, N, A):
    """[m(a)] as Python floats"""
    q = np.asarray(q_post_row).reshape(N, A)
    out = []
    for a in range(A):
        s = 0.0
        for j in range(N):
            s += float(q[j, a])
        out.append(s / float(N))
    return out


def greedy(m):
    best, bv = 0, m[0]
    for a in range(1, len(m)):
        if m[a] > bv:
            best, bv = a, m[a]
    return best


def gap(m):
    """best minus second-best m(a) (inf with one action)"""
    s = sorted(m, reverse=True)
    return float("inf") if len(s) < 2 else s[0] - s[1]


def pair(delta, tau_j, kappa, t):
    zero, half, one = t(0), t(0.5), t(1)
    w = one - tau_j if delta > zero else tau_j
    ad = -delta if delta < zero else delta
    dc = -kappa if delta < -kappa else (kappa if delta > kappa else delta)
    L = half * (delta * delta) if ad <= kappa else kappa * (ad - half * kappa)
    return (w * dc) / kappa, (w * L) / kappa


def sample(q_pre_row, q_post_row, N, A, action, r, terminal, gam, kappa, t=np.float32):
    """one sample -> dict(dq [N A], cost, targets [N], maxq, astar, gap)"""
    q_pre, q_post = np.asarray(q_pre_row, t).reshape(N, A), np.asarray(q_post_row, t).reshape(N, A)
    kappa, r, gam = t(kappa), float(r), float(gam)
    m = means(q_post, N, A)
    astar = greedy(m)
    targets = np.array([t(r if terminal else r + gam * float(q_post[jp, astar])) for jp in range(N)], t)
    dq = np.zeros((N, A), t)
    cost = 0.0
    with np.errstate(all="ignore"):
        for j in range(N):
            s = t(0)
            for jp in range(N):
                g, rho = pair(t(q_pre[j, action] - targets[jp]), tau(j, N, t), kappa, t)
                s = t(s + g)
                cost += float(rho)
            dq[j, action] = s / t(N * N)
    return dict(dq=dq.reshape(-1), cost=t(cost / float(N * N)), targets=targets, maxq=t(m[astar]), astar=astar, gap=gap(m))


def action_values(q_row, N, A, t=np.float32):
    q = np.asarray(q_row, t).reshape(N, A)
    s = np.zeros(A, t)
    with np.errstate(all="ignore"):
        for j in range(N):
            s = (s + q[j]).astype(t)
        return (s / t(N)).astype(t)


def act(q_row, N, A, t=np.float32):
    return int(np.argmax(action_values(q_row, N, A, t)))               # np.argmax: the first maximum, a NaN counts as one


class QuantileOracle(OracleDQN):
    """OracleDQN over N A outputs with the targets and gradients above; clip_error is kappa"""

    def __init__(self, game_actions, quantiles, *a, n_step=1, **kw):
        OracleDQN.__init__(self, quantiles * game_actions, *a, **kw)
        self.quantiles, self.game_actions, self.n_step = int(quantiles), int(game_actions), int(n_step)
        assert self.clip_error and self.clip_error > 0
        self.last_maxq = self.last_targets = self.last_cost_terms = self.last_d4 = self.last_gaps = self.last_postq = None

    def predict_quantiles(self, states_u8):
        return self.predict(states_u8).reshape(-1, self.quantiles, self.game_actions)

    def predict_mean(self, states_u8):
        q = self.predict(states_u8)
        return np.stack([action_values(row, self.quantiles, self.game_actions, self.dtype) for row in q])

    def gradients(self, minibatch):
        prestates, actions, rewards, poststates, terminals = minibatch
        B, N, A, t = prestates.shape[0], self.quantiles, self.game_actions, self.dtype
        postq = self.fprop(self.Wt, self._normalize(poststates))
        preq, (acts, cols_all, a3f, a4) = self.fprop(self.W, self._normalize(prestates), keep=True)
        if self.n_step > 1:
            r, gam = [float(x) for x in rewards], gamma_n(self.n_step, self.discount_rate)
        else:
            r, gam = [float(x) for x in np.clip(rewards, self.min_reward, self.max_reward)], self.discount_rate
        out = [sample(preq[n], postq[n], N, A, int(actions[n]), r[n], bool(terminals[n]), gam, self.clip_error, t) for n in range(B)]
        deltas = np.stack([o["dq"] for o in out]).astype(t)
        terms = np.array([o["cost"] for o in out], t)
        cost = t(terms.mean())
        self.last_maxq = np.array([o["maxq"] for o in out], t)
        self.last_targets = np.stack([o["targets"] for o in out])
        self.last_gaps = np.array([o["gap"] for o in out])
        self.last_cost_terms, self.last_postq = terms, postq
        # ---- bprop: OracleDQN.gradients from here on
        g = [None] * 5
        g[4] = deltas.T @ a4
        d4 = self._hd((deltas @ self.W[4]) * (a4 > 0))
        self.last_d4 = d4
        g[3] = d4.T @ a3f
        d = self._hd((d4 @ self._h(self.W[3])) * (a3f > 0))
        for li in (2, 1, 0):
            R, S, Kc, st = CONV[li]
            a_out = acts[li + 1]
            d = d.reshape(a_out.shape)
            dmat = np.ascontiguousarray(d.reshape(B, Kc, -1).transpose(0, 2, 1))
            g[li] = np.einsum('nmc,nmk->ck', cols_all[li], dmat, optimize=True).astype(t)
            if li > 0:
                a_in = acts[li]
                dcols = dmat @ self._h(self.W[li]).T
                d = self._hd(_col2im(dcols, a_in.shape[1], a_in.shape[2], a_in.shape[3], R, S, st) * (a_in > 0))
        return g, cost, deltas, preq
