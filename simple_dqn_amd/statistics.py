"""Run statistics with the reference's observable behaviour (callbacks, log lines, 16-column CSV —
/root/reference/src/statistics.py:8-124), organised as: a per-phase tally (`_PhaseTally`), a CSV sink (`_CsvSink`)
and the `Statistics` facade that Agent / DeepQNetwork call back into.

Observability only; it is the second caller of mem.getMinibatch() (statistics.py:85) and net.predict() (:90).
Clock: CPU time (`time.process_time()`), which is what the reference's `time.clock()` returned on Linux.
Kept quirks: `validation_states` is whatever array getMinibatch() returned first (the reference aliases
mem.prestates, :85-86 — with the fused Agent path nothing overwrites it later; README.md), and the training-cost
average divides by the net's GLOBAL train_iterations although it restarts every phase (:55,71).
"""
import csv
import logging
import sys
import time

import numpy as np

logger = logging.getLogger(__name__)

COLUMNS = ("epoch", "phase", "steps", "nr_games", "average_reward", "min_game_reward", "max_game_reward",
           "last_exploration_rate", "total_train_steps", "replay_memory_count", "meanq", "meancost",
           "weight_updates", "total_time", "epoch_time", "steps_per_second")
DORMANT_COLUMNS = ("dormant_1", "dormant_2", "dormant_3", "dormant_4")      # only with --redo_interval / --log_dormant
# only with --log_weight_norms: the L2 norm of each layer's weights and their L2 distance from the L2-init anchor
WEIGHT_NORM_COLUMNS = tuple("wnorm_%d" % l for l in range(1, 6)) + tuple("winit_%d" % l for l in range(1, 6))


class _PhaseTally:
    """Everything that restarts with reset(): step / game counters, reward extremes, running means."""

    def __init__(self):
        self.began = time.process_time()
        self.num_steps = self.num_games = 0
        self.game_rewards = self.average_reward = self.average_cost = 0
        self.min_game_reward, self.max_game_reward = sys.maxsize, -sys.maxsize - 1
        self.last_exploration_rate = 1

    def step(self, reward, terminal, exploration_rate):
        self.num_steps += 1
        self.game_rewards += reward
        self.last_exploration_rate = exploration_rate
        if not terminal:
            return
        self.num_games += 1                                              # a game ended: fold its return in
        self.average_reward += float(self.game_rewards - self.average_reward) / self.num_games
        self.min_game_reward = min(self.min_game_reward, self.game_rewards)
        self.max_game_reward = max(self.max_game_reward, self.game_rewards)
        self.game_rewards = 0

    def close_open_game(self):
        if self.num_games == 0:                                          # no finished game in this phase: report the open one
            self.num_games, self.average_reward = 1, self.game_rewards


class _CsvSink:
    def __init__(self, path, columns=COLUMNS):
        self.path = path
        self.fh = self.writer = None
        if path:
            logger.info("Results are written to %s" % path)
            self.fh = open(path, "w", newline="")
            self.writer = csv.writer(self.fh)
            self.row(columns)

    def row(self, values):
        if self.writer:
            self.writer.writerow(values)
            self.fh.flush()

    def close(self):
        if self.fh:
            self.fh.close()


_TALLY_FIELDS = ("num_steps", "num_games", "game_rewards", "average_reward", "min_game_reward", "max_game_reward",
                 "last_exploration_rate", "average_cost")


class Statistics:
    def __init__(self, agent, net, mem, env, args):
        self.agent, self.net, self.mem, self.env = agent, net, mem, env
        agent.callback = net.callback = self                            # both producers report here
        self.csv_name = args.csv_file
        # the dormancy columns exist only when asked for, so that every other run's CSV keeps its 16-column header
        self._dormant = bool(getattr(args, "redo_interval", 0) or getattr(args, "log_dormant", False))
        self._weight_norms = bool(getattr(args, "log_weight_norms", False))
        self._csv = _CsvSink(self.csv_name, COLUMNS + (DORMANT_COLUMNS if self._dormant else ()) + (WEIGHT_NORM_COLUMNS if self._weight_norms else ()))
        self.start_time = time.process_time()
        self.validation_states = None
        self.reset()

    # the tally's fields are part of the reference's public surface (st.num_games, st.average_cost, ...)
    def __getattr__(self, name):
        if name in _TALLY_FIELDS:
            if name == "average_cost" and self.__dict__.get("_pending"):
                self._resolve_pending()
            return getattr(self.__dict__["_tally"], name)
        raise AttributeError(name)

    def reset(self):
        self._resolve_pending()                                         # (costs of the phase that ends belong to its tally)
        self._tally = _PhaseTally()
        self.epoch_start_time = self._tally.began

    def on_step(self, action, reward, terminal, screen, exploration_rate):
        self._tally.step(reward, terminal, exploration_rate)

    def record_evaluation(self, tallies, exploration_rate):
        """The phase's tally from DeepQNetwork.evaluate (--eval_envs): steps, nr_games and last_exploration_rate are exact.  The device
        keeps sums, not per-game returns: average_reward is the summed reward of ALL steps divided by the games finished (it includes
        the open games' rewards; exact when none is open), min_game_reward / max_game_reward are not available and are written as 0."""
        t = self._tally
        t.num_steps = int(tallies["steps"].sum())
        t.num_games = int(tallies["episodes"].sum())
        t.game_rewards = int(tallies["reward"].sum())
        t.last_exploration_rate = exploration_rate
        t.min_game_reward = t.max_game_reward = 0
        if t.num_games:
            t.average_reward = float(t.game_rewards) / t.num_games

    def on_train(self, cost):
        self._resolve_pending()
        t = self._tally
        t.average_cost += (cost - t.average_cost) / self.net.train_iterations

    # Deferred form of on_train (simple_dqn_amd.DeepQNetwork.train_from_memory offers it to callbacks that have this method): the train
    # step has been ENQUEUED, its cost is collected later — when the next one is announced, or when average_cost is read / the phase
    # ends.  The running mean is updated with exactly the (cost, train_iterations) pairs and in exactly the order the immediate form
    # would have used (statistics.py:70-71 of the reference), so the tally is bit-identical; the host just no longer waits 65 us for
    # the GPU after every fourth environment step.
    def on_train_deferred(self, collect, train_iterations):
        self._resolve_pending()
        self._pending.append((collect, train_iterations))

    def _resolve_pending(self):
        pend = self.__dict__.get("_pending")
        if pend is None:
            self._pending = []
            return
        while pend:
            collect, iters = pend.pop(0)
            t = self._tally
            t.average_cost += (collect() - t.average_cost) / iters

    def _mean_max_q(self):
        if self.validation_states is None:
            return 0
        q = self.net.predict(self.validation_states)
        best = np.max(q, axis=1)
        assert best.shape[0] == q.shape[0]
        return np.mean(best)

    def write(self, epoch, phase):
        self._resolve_pending()                                         # a deferred cost still outstanding belongs in this row's meancost
        t = self._tally
        now = time.process_time()
        total_time, epoch_time = now - self.start_time, max(now - t.began, 1e-9)
        rate = t.num_steps / epoch_time
        if t.num_steps or t.num_games or t.game_rewards:
            t.close_open_game()
        else:                                                           # a phase without an environment step (--offline_replay's train phase):
            t.min_game_reward = t.max_game_reward = 0                   # zero games, and no extremes of games that were never played
        if self.validation_states is None and self.mem.count > self.mem.batch_size:
            self.validation_states = self.mem.getMinibatch()[0]         # fixed held-out states for the meanq column
        if self.csv_name:
            self._csv.row((epoch, phase, t.num_steps, t.num_games, t.average_reward, t.min_game_reward, t.max_game_reward,
                           t.last_exploration_rate, self.agent.total_train_steps, self.mem.count, self._mean_max_q(),
                           t.average_cost, self.net.train_iterations, total_time, epoch_time, rate)
                          + (tuple(self.net.logged_dormant()) if self._dormant else ())
                          + (tuple(self.net.logged_weight_norms()) if self._weight_norms else ()))
        logger.info("  num_games: %d, average_reward: %f, min_game_reward: %d, max_game_reward: %d" %
                    (t.num_games, t.average_reward, t.min_game_reward, t.max_game_reward))
        logger.info("  last_exploration_rate: %f, epoch_time: %ds, steps_per_second: %d" %
                    (t.last_exploration_rate, epoch_time, rate))

    def close(self):
        self._csv.close()
