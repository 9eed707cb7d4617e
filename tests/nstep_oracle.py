"""n-step returns restated in numpy (test helper, not product code).

  accepts / valid_mask   the indexes the n-step rejection sampler accepts: hist <= i <= count - n, the window [i - hist, i + n - 1] does
                         not straddle `current`, no terminal in terminals[i - hist : i]
  sample_indexes         that rejection loop on oracle.replay_numpy.MT19937: index = randint(hist, count - n); (indexes, draws)
  returns                R = sum_k g_k clip(r_{i+k}) up to and including the first terminal, g_k = gamma^k by repeated multiplication,
                         done = a terminal was met; float64, one rounding per operation
  gather                 (prestates, actions, returns, poststates, dones) with poststate = state(i + n - 1)
  NStepOracle*           OracleDQN / OracleDQNBN whose td_targets take (R, done) and bootstrap with gamma^n; composed with the Double DQN
                         (tests/double_dqn_oracle.py) and PER (tests/per_oracle.py) restatements the way those two compose
"""
import numpy as np

from double_dqn_oracle import _DoubleDQN
from oracle.dqn_bn_numpy import OracleDQNBN
from oracle.dqn_numpy import OracleDQN
from per_oracle import _PER


def accepts(i, terminals, count, current, hist, n):
    if i < hist or i > count - n:
        return False
    if i + n - 1 >= current and i - hist < current:
        return False
    return not np.asarray(terminals[i - hist:i]).any()


def valid_mask(terminals, count, current, hist, size, n):
    t = np.zeros(size + 1, dtype=np.int64)
    t[1:] = np.cumsum(np.asarray(terminals[:size], dtype=bool))
    i = np.arange(size)
    lo = np.clip(i - hist, 0, size)
    ok = (i >= hist) & (i <= count - n) & ~((i + n - 1 >= current) & (i - hist < current))
    ok &= (t[i] - t[lo]) == 0
    return ok


def sample_indexes(rng, terminals, count, current, hist, n, batch):
    """the rejection loop (replay_memory.py:54-68 with the n-step rule) on an MT19937; returns (indexes, draws)"""
    assert count >= hist + n
    out, draws = [], 0
    while len(out) < batch:
        while True:
            index = rng.randint(hist, count - n)
            draws += 1
            if index + n - 1 >= current and index - hist < current:
                continue
            if np.asarray(terminals[index - hist:index]).any():
                continue
            break
        out.append(index)
    return np.array(out, dtype=np.int64), draws


def gamma_n(n, gamma):
    g = 1.0
    for _ in range(n):
        g = g * gamma
    return g


def returns(rewards, terminals, indexes, n, gamma, min_reward, max_reward):
    """the contract's loop, sample by sample, in Python floats"""
    R_out, d_out = [], []
    for i in indexes:
        R, g, done = 0.0, 1.0, False
        for k in range(n):
            r = min(max(float(rewards[i + k]), min_reward), max_reward)
            R = R + g * r
            if terminals[i + k]:
                done = True
                break
            g = g * gamma
        R_out.append(R)
        d_out.append(done)
    return np.array(R_out, dtype=np.float64), np.array(d_out, dtype=np.bool_)


def gather(mem, indexes, n, gamma, min_reward, max_reward):
    """ReplayOracle's gather with the poststate of sample i taken from state(i + n - 1)"""
    pre = np.stack([mem.getState(i - 1) for i in indexes])
    post = np.stack([mem.getState(i + n - 1) for i in indexes])
    R, done = returns(mem.rewards, mem.terminals, indexes, n, gamma, min_reward, max_reward)
    return pre, mem.actions[np.asarray(indexes)], R, post, done


class _NStep:
    n_step = 1

    def td_targets(self, preq, maxpostq, actions, rewards, terminals):
        if self.n_step <= 1:
            return super().td_targets(preq, maxpostq, actions, rewards, terminals)
        gn = gamma_n(self.n_step, self.discount_rate)
        targets = preq.copy()
        for i, action in enumerate(actions):
            R = float(rewards[i])                      # (clipped per step already)
            targets[i, action] = R if terminals[i] else R + gn * float(maxpostq[i])
        return targets


class NStepOracle(_NStep, OracleDQN):
    pass


class NStepOracleBN(_NStep, OracleDQNBN):
    pass


class NStepOracleDDQN(_DoubleDQN, _NStep, OracleDQN):
    pass


class NStepOraclePER(_PER, _NStep, OracleDQN):
    pass


class NStepOraclePERDDQN(_PER, _DoubleDQN, _NStep, OracleDQN):
    pass
