"""Agent — the caller of the hot path, with the observable behaviour of /root/reference/src/agent.py:7-135 (same
public methods, same order of `random` draws and environment calls, same callback events) and its own structure:

    _Epsilon            linear exploration schedule (agent.py:41-46)
    _greedy_action()    picks the cheapest Q-value path the network offers
    _advance()          one environment transition + bookkeeping (agent.py:48-85)
    _learn()            the {getMinibatch ; net.train} pair (agent.py:108-114) — fused into ONE library call,
                        net.train_from_memory(mem), when the replay memory is device-backed: same indexes from the
                        same global random stream, no host minibatch.  fused=False forces the reference's two calls.
"""
import logging
import random

import numpy as np

from .state_buffer import DeviceStateBuffer, StateBuffer

logger = logging.getLogger(__name__)


class _Epsilon:
    """exploration rate annealed linearly over `decay_steps` training steps, then constant"""

    def __init__(self, start, end, decay_steps):
        self.start, self.end, self.decay_steps = start, end, decay_steps

    def at(self, train_step):
        if train_step >= self.decay_steps:
            return self.end
        return self.start - train_step * (self.start - self.end) / self.decay_steps


def priority_beta(beta0, beta_steps, train_step):
    """importance-sampling exponent of prioritized replay, annealed linearly from beta0 to 1 over beta_steps training steps"""
    if beta_steps <= 0:
        return 1.0
    return min(1.0, beta0 + (1.0 - beta0) * train_step / beta_steps)


class Agent:
    def __init__(self, environment, replay_memory, deep_q_network, args, fused=True, offline_chunk=64):
        self.env, self.mem, self.net = environment, replay_memory, deep_q_network
        # --offline_replay: train_offline hands the library at most this many learns per call
        self.offline_chunk = max(1, int(offline_chunk))
        # acting state resident on the device when the network can read it there
        on_device = hasattr(deep_q_network, "predict_state")
        self.buf = DeviceStateBuffer(args) if on_device else StateBuffer(args)
        self.num_actions = self.env.numActions()
        self.history_length, self.random_starts = args.history_length, args.random_starts
        self._epsilon = _Epsilon(args.exploration_rate_start, args.exploration_rate_end, args.exploration_decay_steps)
        self.exploration_rate_test = args.exploration_rate_test
        self.total_train_steps = args.start_epoch * args.train_steps
        self.train_frequency, self.train_repeat, self.target_steps = args.train_frequency, args.train_repeat, args.target_steps
        # --target_tau > 0: the library blends the target net after every train step; the loops below only make the
        # reference's very first copy (agent.py:105 at total_train_steps == 0), so that training starts from theta- = theta
        self.target_tau = float(getattr(args, "target_tau", 0.0) or 0.0)
        self.callback = None
        # --bootstrap_heads: the net follows one Q-head per episode while collecting and votes while testing
        self._boot = getattr(deep_q_network, "bootstrap_heads", 1) > 1
        # --quantiles: the net acts on the mean over its quantiles, training and testing alike; like the Q-heads' rule it
        # turns a raw row of the net into an action (net.acting_action), but it has no mode and no episode bookkeeping
        # --dueling: likewise, the first maximum of V + Adv - mean(Adv) over the net's A + 1 outputs
        self._reduced_acting = self._boot or getattr(deep_q_network, "quantiles", 1) > 1 or bool(getattr(deep_q_network, "dueling", False))
        self._per = getattr(replay_memory, "prioritized", False)
        if self._per:
            self._beta0, self._beta_steps = float(args.priority_beta), int(args.priority_beta_steps)
        self.fused = fused and hasattr(self.net, "train_from_memory") and hasattr(self.mem, "_h")
        # one library call per environment transition (state-buffer add [+ ring add] [+ the next acting forward enqueued ahead of its use])
        self._one_call = hasattr(self.net, "act_step") and hasattr(self.buf, "_h")
        # ... and the environment's step inside it when the game lives in the library (CatchEnvironment, BreakoutEnvironment): the frame is rendered on the
        # device, nothing is uploaded.  fused=False keeps the host-driven path (env.act + act_step with the screen)
        self._env_call = fused and self._one_call and hasattr(self.net, "act_step_env") and hasattr(self.env, "_h")
        # --train_envs N: the random and train phases run N copies of the game in lockstep on the device
        # (play_random_vectorised / train_vectorised); the replay memory becomes N lanes, one episode stream each
        self.train_envs = int(getattr(args, "train_envs", 0) or 0)
        if self.train_envs:
            if not (hasattr(self.net, "collect") and hasattr(self.env, "_h") and hasattr(self.mem, "set_lanes")):
                raise ValueError("--train_envs needs --environment catch, breakout or freeway and the device-backed replay memory")
            if self.mem.lanes[0] != self.train_envs:
                self.mem.set_lanes(self.train_envs)
            self._vec_seed = int(getattr(args, "random_seed", 0) or 0)      # None until the copies have been seeded with it
            self._vec_due = 0
            self._vec_tally = self._vec_base = None

    # ---- acting ------------------------------------------------------------------------------------------
    def _greedy_action(self):
        if self._one_call and hasattr(self.net, "act_greedy"):
            a = self.net.act_greedy(self.buf)                         # predict_state + argmax inside the library
            assert 0 <= a < self.num_actions
            return a
        if hasattr(self.buf, "_h") and hasattr(self.net, "predict_state"):
            q = self.net.predict_state(self.buf)                      # state already in HBM: one 7 KB upload per env step
        elif hasattr(self.net, "predict_one"):
            q = self.net.predict_one(self.buf.getState())             # same numbers as predict(padded batch)[0]
        else:
            q = self.net.predict(self.buf.getStateMinibatch())[0]     # the reference's padded minibatch, agent.py:55-58
        if self._reduced_acting:
            return self.net.acting_action(q)
        assert len(q) == self.num_actions
        return int(np.argmax(q))

    def _fresh_episode(self):
        """restart and idle through a random number of no-op frames so episodes do not all start alike (agent.py:29-39)"""
        self.env.restart()
        if self._boot:
            self.net.next_episode()
        for _ in range(random.randint(self.history_length, self.random_starts) + 1):
            self.env.act(0)
            if self.env.isTerminal():
                self.env.restart()
            self.buf.add(self.env.getScreen())

    def _advance(self, exploration_rate, store=False):
        explore = random.random() < exploration_rate                  # draw order matters: shared global stream
        action = random.randrange(self.num_actions) if explore else self._greedy_action()
        ring = store and hasattr(self.mem, "_h")
        if self._env_call:
            # the game steps inside the library too: one call, the frame rendered on the device (the library skips the speculative
            # forward after a terminal step, as below)
            reward, terminal = self.net.act_step_env(self.buf, self.mem if ring else None, self.env, action,
                                                     speculate=(exploration_rate < 0.5))
            screen = self.env.getScreen()
        else:
            reward = self.env.act(action)
            screen, terminal = self.env.getScreen(), self.env.isTerminal()
            if self._one_call:
                # the acting forward of the new state is started now when the next step will most likely want it (greedy with probability
                # 1 - exploration_rate) and the episode goes on; same Q-values as a forward started at the next step
                self.net.act_step(self.buf, self.mem if ring else None, screen, action, reward, terminal,
                                  speculate=(exploration_rate < 0.5 and not terminal))
            else:
                self.buf.add(screen)
        if terminal:
            self._fresh_episode()
        if self.callback:
            self.callback.on_step(action, reward, terminal, screen, exploration_rate)
        if store and not (self._one_call and ring):
            self.mem.add(action, reward, screen, terminal)
        return action, reward, screen, terminal

    def _advance_and_store(self, exploration_rate):
        return self._advance(exploration_rate, store=True)

    # ---- learning ----------------------------------------------------------------------------------------
    def _learn(self, epoch):
        if self._per:
            self.mem.set_priority_beta(priority_beta(self._beta0, self._beta_steps, self.total_train_steps))
        if self.fused:
            if hasattr(self.net, "set_epoch"):
                self.net.set_epoch(epoch)                             # what net.train(minibatch, epoch) would receive
            self.net.train_from_memory(self.mem, self.train_repeat)
            return
        for _ in range(self.train_repeat):
            self.net.train(self.mem.getMinibatch(), epoch)

    # ---- the reference's public surface -------------------------------------------------------------------
    def step(self, exploration_rate):
        return self._advance(exploration_rate)

    def _restartRandom(self):
        self._fresh_episode()

    def _explorationRate(self):
        return self._epsilon.at(self.total_train_steps)

    def _acting_mode(self, test):
        if self._boot or getattr(self.net, "noisy_nets", False):      # --noisy_nets: the noise while collecting, mu while testing
            self.net.set_acting(test)

    def play_random(self, random_steps):                              # fill the replay memory with uniform-random play
        self._acting_mode(False)
        self.env.restart()
        if self._boot:
            self.net.next_episode()
        for _ in range(random_steps):
            self._advance_and_store(1)

    def train(self, train_steps, epoch=0):
        self._acting_mode(False)
        for i in range(train_steps):
            self._advance_and_store(self._epsilon.at(self.total_train_steps))
            if self.target_tau > 0:
                if self.target_steps and self.total_train_steps == 0:
                    self.net.update_target_network()
            elif self.target_steps and i % self.target_steps == 0:    # also fires at i == 0 of every call (agent.py:105)
                self.net.update_target_network()
            if self.mem.count > self.mem.batch_size and i % self.train_frequency == 0:
                self._learn(epoch)
            self.total_train_steps += 1

    # ---- --train_envs: vectorised collection ---------------------------------------------------------------
    def _collect(self, locksteps, exploration_rate):
        seed, self._vec_seed = self._vec_seed, None
        self._vec_tally = self.net.collect(self.env, self.mem, self.train_envs, locksteps, exploration_rate, seed=seed)
        if self._vec_base is None:
            self._vec_base = dict((k, np.zeros_like(v)) for k, v in self._vec_tally.items())
        self._vec_rate = exploration_rate

    def vectorised_tallies(self):
        """(tallies of the copies since the last call of this method, last exploration rate): what Statistics.record_evaluation takes"""
        now = self._vec_tally
        delta = dict((k, now[k] - self._vec_base[k]) for k in now)
        self._vec_base = now
        return delta, self._vec_rate

    def play_random_vectorised(self, random_steps):
        """ceil(random_steps / train_envs) locksteps of uniform-random play in ONE library call (no forward runs).  --random_starts has
        no meaning here: the library's games spawn their balls at random and a restart is the game's own."""
        self._collect(-(-int(random_steps) // self.train_envs), 1.0)

    def train_vectorised(self, train_steps, epoch=0):
        """ceil(train_steps / train_envs) locksteps: all copies act with the exploration rate of total_train_steps, the lockstep's
        transitions are collected, one train call (train_repeat steps) is due per train_frequency environment steps, the target net
        is refreshed whenever total_train_steps crosses a multiple of target_steps (and at step 0), total_train_steps += train_envs."""
        N = self.train_envs
        for _ in range(-(-int(train_steps) // N)):
            self._collect(1, self._epsilon.at(self.total_train_steps))
            if self.target_tau > 0:
                if self.target_steps and self.total_train_steps == 0:
                    self.net.update_target_network()
            elif self.target_steps and self.total_train_steps % self.target_steps < N:
                self.net.update_target_network()
            self._vec_due += N
            while self._vec_due >= self.train_frequency:
                if self.mem.can_sample():
                    self._learn(epoch)
                self._vec_due -= self.train_frequency
            self.total_train_steps += N

    # ---- --offline_replay: training from a fixed memory -------------------------------------------------------
    def _offline_refresh_due(self, t):
        """the target net is refreshed before learn t (= total_train_steps): with --target_tau only the reference's very first copy"""
        if not self.target_steps:
            return False
        return t == 0 if self.target_tau > 0 else t % self.target_steps == 0

    def train_offline(self, train_steps, epoch=0):
        """train_steps learns (each train_repeat gradient steps) from the memory as it stands: no environment step, no exploration.  Before
        learn t = total_train_steps the target net is refreshed where _offline_refresh_due says so; total_train_steps += 1 after every learn.
        Consecutive learns with no refresh between them go to the library as ONE call of k <= offline_chunk learns; a prioritized memory's
        beta is set once per call, from total_train_steps at its start."""
        if not self.mem.can_sample():
            raise ValueError("offline training needs more than batch_size = %d transitions in the replay memory, it holds %d"
                             % (self.mem.batch_size, self.mem.count))
        left = int(train_steps)
        while left > 0:
            t = self.total_train_steps
            if self._offline_refresh_due(t):
                self.net.update_target_network()
            k = 1
            while k < min(left, self.offline_chunk) and not self._offline_refresh_due(t + k):
                k += 1
            if self._per:
                self.mem.set_priority_beta(priority_beta(self._beta0, self._beta_steps, t))
            if self.fused:
                if hasattr(self.net, "set_epoch"):
                    self.net.set_epoch(epoch)
                self.net.train_from_memory(self.mem, k * self.train_repeat)
            else:
                for _ in range(k * self.train_repeat):
                    self.net.train(self.mem.getMinibatch(), epoch)
            self.total_train_steps += k
            left -= k

    def test(self, test_steps, epoch=0):
        self._acting_mode(True)
        self._fresh_episode()
        for _ in range(test_steps):
            self._advance(self.exploration_rate_test)

    def play(self, num_games):
        self._acting_mode(True)
        self._fresh_episode()
        for _ in range(num_games):
            terminal = False
            while not terminal:
                terminal = self._advance_and_store(self.exploration_rate_test)[3]
