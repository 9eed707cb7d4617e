"""--noisy_nets restatement on the numpy oracle (test helper, not product code).

fc4 and fc5 are W = mu + sigma * (e_out e_in^T) with the factor vectors e = f(z) GIVEN (the device's own, or the host restatement's): the
oracle composes them in float32 — e = e_out * e_in, then W = mu + sigma * e, each operation rounded once — runs oracle/dqn_numpy.py's
forward / backward unchanged on the effective weights, derives d sigma = dW * e, and applies the optimizer rule to mu and to sigma
(sigma with state of its own).  The noise itself is restated in integers (words) and float32 (normal, factor) below.
The composition is float32 whatever the oracle's dtype; with dtype=np.float64 everything behind it (forward, backward, mu's optimizer) runs
in float64 on those float32 effective weights — the reference for free-running steps, which has no Rectlin gate flips of its own.
"""
import numpy as np

from double_dqn_oracle import _DoubleDQN
from nstep_oracle import _NStep
from oracle.dqn_numpy import OracleDQN
from per_oracle import _PER

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
IN4, OUT4, IN5 = 3136, 512, 512


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def key(seed, step, slot, layer, side):
    k = mix((seed + G) & M64)
    k = mix((k + G * (step + 1)) & M64)
    return mix((k + G * (4 * slot + 2 * layer + side + 1)) & M64)


def words(seed, step, slot, layer, side, n):
    k = key(seed, step, slot, layer, side)
    return np.array([mix((k + G * (i + 1)) & M64) for i in range(n)], dtype=np.uint64)


def normal(w):
    """float32 Box-Muller of the words (numpy's log / cos: a few ulps from any other libm)"""
    w = np.asarray(w, dtype=np.uint64)
    f = np.float32
    u1 = ((w >> np.uint64(32)) + np.uint64(1)).astype(f) * f(2.0 ** -32)
    u2 = (w & np.uint64(0xFFFFFFFF)).astype(f) * f(2.0 ** -32)
    return (np.sqrt(f(-2.0) * np.log(u1)) * np.cos(f(6.28318530717958647692) * u2)).astype(f)


def factor(z):
    z = np.asarray(z, dtype=np.float32)
    return np.copysign(np.sqrt(np.abs(z)), z).astype(np.float32)


def sizes(A):
    """(layer, side) -> length of the stream"""
    return {(0, 0): IN4, (0, 1): OUT4, (1, 0): IN5, (1, 1): A}


def compose(mu4, mu5, s4, s5, eps):
    """effective (W4, W5) in float32 from one net's factor vectors eps = dict(in4, out4, in5, out5)"""
    f = np.float32
    e4 = (eps["out4"].astype(f)[:, None] * eps["in4"].astype(f)[None, :]).astype(f)
    e5 = (eps["out5"].astype(f)[:, None] * eps["in5"].astype(f)[None, :]).astype(f)
    w4 = (mu4.astype(f) + (s4.astype(f) * e4).astype(f)).astype(f)
    w5 = (mu5.astype(f) + (s5.astype(f) * e5).astype(f)).astype(f)
    return w4, w5, e4, e5


class _Noisy:
    """mix-in over OracleDQN: self.W / self.Wt hold mu; sigma / sigma_t the two nets' sigmas [fc4, fc5]"""

    def init_noisy(self, sigma0=0.5):
        f = np.float32
        A = self.num_actions
        mk = lambda: [np.full((OUT4, IN4), f(sigma0 / np.sqrt(float(IN4))), f), np.full((A, IN5), f(sigma0 / np.sqrt(float(IN5))), f)]
        self.sigma, self.sigma_t = mk(), (mk() if self.target_enabled else None)
        if self.sigma_t is None:
            self.sigma_t = self.sigma
        # sigma's optimizer: the parent's rule on a five-layer list whose first three layers are placeholders
        ph = [np.zeros((1, 1), f)] * 3
        self._sopt = OracleDQN(A, batch_size=self.batch_size, weights=ph + [s.copy() for s in self.sigma], optimizer=self.optimizer,
                               learning_rate=self.lr, decay_rate=self.rho, epsilon=self.eps, beta_1=self.beta_1, beta_2=self.beta_2)
        self.last_gsigma = None
        return self

    last_acts = None            # [x, a1, a2, a3] (N, K, P, Q) of the last forward that kept its tensors: the online net on the prestates

    # A Rectlin gate whose input lies within the float32 forward's round-off of zero is not decided by the arithmetic: the device and an exact
    # forward may fall on different sides (measured: device 5.2e-8 against 0, one gate of a2 in 166 000), and the backward then differs by
    # that sample's whole delta.  follow = {layer 1..3: the device's activations (N, K, P, Q)}: where the two gates differ and BOTH values
    # are below follow_tol, the oracle's kept activation takes the device's value, so its backward takes the device's side (as
    # tests/test_gpu_head_edges.py's _follow does for an argmax within round-off).  follow_tol = 1e-6: ten times the round-off of a
    # 512-term float32 dot product of O(0.1) operands; a gate that differs at a larger value is left alone and shows as a miss.
    follow, follow_tol, followed = None, 1e-6, ()

    def fprop(self, W, x, keep=False):
        out = super().fprop(W, x, keep)
        if keep:
            acts = out[1][0]
            self.followed = []
            for li, dev in (self.follow or {}).items():
                ref = acts[li]
                dev = np.asarray(dev).reshape(ref.shape)
                m = ((dev > 0) != (ref > 0)) & (np.maximum(np.abs(dev), np.abs(ref)) < self.follow_tol)
                for idx in np.argwhere(m):
                    self.followed.append((li, tuple(int(i) for i in idx), float(dev[tuple(idx)]), float(ref[tuple(idx)])))
                ref[m] = dev[m]
            self.last_acts = acts
        return out

    def effective(self, eps, target=False):
        W, S = (self.Wt, self.sigma_t) if target else (self.W, self.sigma)
        w4, w5, _, _ = compose(W[3], W[4], S[0], S[1], eps)
        return [W[0], W[1], W[2], w4, w5]

    def predict_noisy(self, states, eps, target=False):
        return self.fprop(self.effective(eps, target), self._normalize(states))

    def noisy_gradients(self, minibatch, eps, eps_t):
        """(g mu [5], g sigma [2], cost, preq) of one step under the given factor vectors"""
        mu, mu_t = self.W, self.Wt
        _, _, e4, e5 = compose(mu[3], mu[4], self.sigma[0], self.sigma[1], eps)
        self.W, self.Wt = self.effective(eps), self.effective(eps_t, target=True)
        try:
            g, cost, _, preq = self.gradients(minibatch)
        finally:
            self.W, self.Wt = mu, mu_t
        gs = [(g[3].astype(np.float32) * e4).astype(np.float32), (g[4].astype(np.float32) * e5).astype(np.float32)]
        self.last_gsigma = gs
        return g, gs, cost, preq

    def noisy_train(self, minibatch, eps, eps_t, epoch=0):
        g, gs, cost, preq = self.noisy_gradients(minibatch, eps, eps_t)
        B = minibatch[0].shape[0]
        self.optimize(g, B, epoch)
        self._sopt.W[3], self._sopt.W[4] = self.sigma[0], self.sigma[1]
        self._sopt.optimize([np.zeros((1, 1), np.float32)] * 3 + gs, B, epoch)
        self.sigma[0], self.sigma[1] = self._sopt.W[3], self._sopt.W[4]
        self.train_iterations += 1
        return g, gs, cost, preq

    def update_target_network(self):
        super().update_target_network()
        if self.target_enabled:
            self.sigma_t = [s.copy() for s in self.sigma]


class NoisyOracle(_Noisy, OracleDQN):
    pass


class NoisyOracleDDQN(_Noisy, _DoubleDQN, OracleDQN):
    pass


class NoisyOracleNStep(_Noisy, _NStep, OracleDQN):
    pass


class NoisyOraclePER(_Noisy, _PER, OracleDQN):
    pass
