"""The dueling architecture (--dueling) restated in numpy scalars and Python floats (test helper, not product code).

The net has A + 1 outputs: row 0 is V, row 1 + a is Adv_a.  With H = 512 hidden units in fc4, units j < H / 2 are the value stream and
units j >= H / 2 the advantage stream: W5[0][j] is held at +0.0 for j >= H / 2, W5[1 + a][j] for j < H / 2, in the online and the target
net, and the same entries of the gradient are set to +0.0 before it is clipped or applied.  t is the network's number type; "double" is a
Python float.  For sample n:

    Q(s, a)   = t((V + Adv_a) - (sum_b Adv_b) / A)           double from the stored rows, the sum in action order
    greedy    = the first a with the largest Q(s, a): `>` against the running best (a NaN Q(a) is never chosen over a number, a NaN Q(0) stays)
    y         = r_c + (terminal ? 0 : gamma max_a Q(theta-, s', a))           double; stored as t
    delta     = Q(theta, s, a_n) - t(y)
    c         = clip(delta, -clip_error, clip_error) (clip_error 0: delta);  cost term 0.5 delta^2
                (prioritized replay, weight w: c = w clip(delta), cost term w (0.5 delta^2), new priority (|delta| + eps)^alpha)
    dq[n][0]  = c,   dq[n][1 + b] = c * t(1 - 1 / A) if b == a_n else c * t(-1 / A)
    d4[j]     = 1[a4[j] > 0] sum_rows W5[row][j] dq[row]
    (n_step > 1: R, done, gamma^n in the places of r_c, terminal, gamma)

    acting: the greedy rule on the A + 1 row
"""
import numpy as np

from nstep_oracle import gamma_n
from oracle.dqn_numpy import CONV, FC_HIDDEN, OracleDQN, _col2im

GAP = 1e-4                      # every oracle comparison asks that a sample's best and second-best Q(theta-, s', .) differ by more than this,
                                # and that |delta| stays further than this from clip_error: no maximum and no clip edge is decided by rounding


def mask(A, H=FC_HIDDEN, dtype=bool):
    """M [A + 1][H]: M[0][j] = 1[j < H / 2], M[1 + a][j] = 1[j >= H / 2]"""
    m = np.zeros((A + 1, H), dtype)
    m[0, :H // 2] = 1
    m[1:, H // 2:] = 1
    return m


def masked(w5):
    """W5 with +0.0 outside the two blocks"""
    w = np.array(w5)
    w[~mask(w.shape[0] - 1, w.shape[1])] = 0
    return w


def q_values(row, A, t=np.float32):
    """[Q(s, a)] as t, from one raw row [A + 1]"""
    row = np.asarray(row)
    s = 0.0
    for b in range(A):
        s += float(row[1 + b])
    mean = s / float(A)
    with np.errstate(all="ignore"):
        return np.array([t((float(row[0]) + float(row[1 + a])) - mean) for a in range(A)], t)


def greedy(q):
    best, bv = 0, q[0]
    for a in range(1, len(q)):
        if q[a] > bv:
            best, bv = a, q[a]
    return best


def act(row, A, t=np.float32):
    return greedy(q_values(row, A, t))


def gap(q):
    """best minus second-best (inf with one action)"""
    s = sorted((float(x) for x in q), reverse=True)
    return float("inf") if len(s) < 2 else s[0] - s[1]


def dq_row(c, A, action, t=np.float32):
    on, off = t(1.0 - 1.0 / A), t(-1.0 / A)
    out = np.empty(A + 1, t)
    out[0] = c
    for b in range(A):
        out[1 + b] = t(c * (on if b == action else off))
    return out


def sample(q_pre_row, q_post_row, A, action, r, terminal, gam, clip_error, t=np.float32, weight=None, per_alpha=0.0, per_eps=0.0):
    """one sample -> dict(dq [A + 1], cost, y, delta, maxq, q_taken, gap, edge[, priority])"""
    qp, qn = q_values(q_pre_row, A, t), q_values(q_post_row, A, t)
    m = qn[greedy(qn)]
    y = float(r) if terminal else float(r) + float(gam) * float(m)
    with np.errstate(all="ignore"):
        d = t(qp[action] - t(y))
        c = d
        if clip_error:
            k = t(clip_error)
            lo = d if d > -k else -k                              # fmin(fmax(d, -k), k): a NaN d gives -k
            c = lo if lo < k else k
        cost = t(t(0.5) * t(d * d))
        out = dict(y=t(y), delta=d, maxq=m, q_taken=qp[action], gap=gap(qn),
                   edge=abs(abs(float(d)) - float(clip_error)) if clip_error else float("inf"))
        if weight is not None:
            w = t(weight)
            cost, c = t(w * cost), t(w * c)
            out["priority"] = np.float32((abs(float(d)) + per_eps) ** per_alpha)
        out.update(dq=dq_row(t(c), A, action, t), cost=cost)
    return out


class DuelingOracle(OracleDQN):
    """OracleDQN over A + 1 outputs with fc5 masked, the targets and gradients above"""

    def __init__(self, game_actions, *a, n_step=1, **kw):
        OracleDQN.__init__(self, game_actions + 1, *a, **kw)
        self.game_actions, self.n_step = int(game_actions), int(n_step)
        self.W[4] = masked(self.W[4])
        if self.Wt is not self.W:
            self.Wt[4] = masked(self.Wt[4])
        self.per_weights = None                                    # [B] importance weights of the next gradients() call, or None
        self.per_alpha = self.per_eps = 0.0
        self.last = None

    def set_target(self, wt):
        self.Wt = [np.array(w, dtype=self.dtype) for w in wt]
        self.Wt[4] = masked(self.Wt[4])

    def streams(self, states_u8):
        raw = self.predict(states_u8)
        return raw[:, 0], raw[:, 1:]

    def predict_q(self, states_u8):
        return np.stack([q_values(row, self.game_actions, self.dtype) for row in self.predict(states_u8)])

    def gradients(self, minibatch):
        prestates, actions, rewards, poststates, terminals = minibatch
        B, A, t = prestates.shape[0], self.game_actions, self.dtype
        postq = self.fprop(self.Wt, self._normalize(poststates))
        preq, (acts, cols_all, a3f, a4) = self.fprop(self.W, self._normalize(prestates), keep=True)
        if self.n_step > 1:
            r, gam = [float(x) for x in rewards], gamma_n(self.n_step, self.discount_rate)
        else:
            r, gam = [float(x) for x in np.clip(rewards, self.min_reward, self.max_reward)], self.discount_rate
        w = self.per_weights
        out = [sample(preq[n], postq[n], A, int(actions[n]), r[n], bool(terminals[n]), gam, self.clip_error, t,
                      None if w is None else w[n], self.per_alpha, self.per_eps) for n in range(B)]
        deltas = np.stack([o["dq"] for o in out]).astype(t)
        terms = np.array([o["cost"] for o in out], t)
        cost = t(terms.mean())
        self.last = dict(y=np.array([o["y"] for o in out], t), delta=np.array([o["delta"] for o in out], t),
                         maxq=np.array([o["maxq"] for o in out], t), gaps=np.array([o["gap"] for o in out]),
                         edges=np.array([o["edge"] for o in out]), cost_terms=terms, postq=postq, a4=a4, dq=deltas,
                         q_taken=np.array([o["q_taken"] for o in out], t),
                         priority=np.array([o["priority"] for o in out], np.float32) if w is not None else None)
        # ---- bprop: OracleDQN.gradients from here on, the fc5 gradient masked
        g = [None] * 5
        g[4] = (deltas.T @ a4).astype(t)
        g[4][~mask(A)] = 0
        d4 = self._hd((deltas @ self.W[4]) * (a4 > 0))
        self.last["d4"] = d4
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
