"""python -m simple_dqn_amd.main — the reference's top-level loop (/root/reference/src/main.py:16-165) on the
MI355X hot path.  Same flags and defaults; `--environment synthetic` (default here) replaces the ALE / gym
wrappers, which are emulator I/O outside the hot path.  Plumbing for BASELINE.json configs[0]."""
import argparse
import logging
import random
import sys

# the checks of the options that DeepQNetwork refuses on its own as well: the same functions, refused here before anything touches the device
from .deepqnetwork import (check_advantage_learning, check_bootstrap, check_cql, check_dueling, check_noisy, check_quantiles,  # noqa: F401
                           check_random_shift, check_redo, check_regularizer, check_reset, refuse_conflicts)


def _flag(text):
    return text.lower() in ("yes", "true", "t", "1")


# The command line of the reference (same flag names, defaults and grouping: src/main.py:16-84), as data.
# (flag, type, default[, extra argparse keywords])
_OPTIONS = {
    "Environment": [
        ("--environment", str, "synthetic", dict(choices=["synthetic", "ale", "gym", "catch", "breakout", "freeway"])),
        ("--num_actions", int, 4, dict(help="Action-set size of the synthetic environment.")),
        ("--synthetic_frame_pool", int, 256, dict(help="Synthetic environment: serve frames from a pool of this many pre-generated frames (0: generate 7 KB of random bytes every step).")),
        ("--catch_balls", int, 10, dict(help="Catch environment: balls per episode.")),
        ("--breakout_balls", int, 3, dict(help="Breakout environment: lost balls per episode.")),
        ("--freeway_ticks", int, 500, dict(help="Freeway environment: game ticks per episode (>= 1).")),
        ("--eval_envs", int, 0, dict(help="Catch / breakout / freeway environment: play the test phase on this many copies of the game at once, on the device (0: Agent.test, one environment).")),
        ("--train_envs", int, 0, dict(help="Catch / breakout / freeway environment: collect experience from this many copies of the game at once, on the device; the replay memory becomes that many lanes (0: Agent.train, one environment).")),
        ("--frame_skip", int, 1, dict(help="Catch / breakout / freeway environment: game ticks per agent step (1..8); the rewards of the ticks add up.")),
        ("--repeat_action_probability", float, 0.0, dict(help="Catch / breakout / freeway environment: sticky actions; before every game tick the action executed last is repeated with this probability, in [0, 1).")),
        ("--screen_width", int, 84), ("--screen_height", int, 84),
    ],
    "Replay memory": [
        ("--replay_size", int, 1000000), ("--history_length", int, 4),
        ("--prioritized_replay", _flag, False, dict(help="Prioritized experience replay (proportional): sample by (|TD error| + epsilon)^alpha, importance-weighted loss.")),
        ("--priority_alpha", float, 0.6), ("--priority_beta", float, 0.4),
        ("--priority_beta_steps", int, 1000000, dict(help="Training steps over which the importance-sampling exponent anneals from --priority_beta to 1.")),
        ("--priority_epsilon", float, 1e-6),
        ("--n_step", int, 1, dict(help="n-step returns (1..16): bootstrap from the state n steps later, rewards summed with the discount (1: one-step targets).")),
        ("--save_replay", str, None, dict(help="Write the replay memory to this file when the run ends: a dataset for --offline_replay.")),
        ("--offline_replay", str, None, dict(help="Offline training: load the replay memory from this file (written by --save_replay with the same --replay_size, screen size and --history_length), collect nothing, and count --train_steps in learns; the test phase plays the game as ever.")),
    ],
    "Deep Q-learning network": [
        ("--learning_rate", float, 0.00025), ("--discount_rate", float, 0.99), ("--batch_size", int, 32),
        ("--optimizer", str, "rmsprop", dict(choices=["rmsprop", "adam", "adadelta"])),
        ("--decay_rate", float, 0.95), ("--clip_error", float, 1), ("--min_reward", float, -1), ("--max_reward", float, 1),
        ("--batch_norm", _flag, False),
        ("--double_dqn", _flag, False, dict(help="Double DQN targets: the online net picks the poststate's action, the target net values it.")),
        ("--target_tau", float, 0.0, dict(help="Soft target updates: after every train step the target net moves by this fraction toward the online net (0: hard copy every --target_steps steps).")),
        ("--clip_grad_norm", float, 0.0, dict(help="Global gradient-norm clipping: scale the whole (mean) gradient to at most this L2 norm before the optimizer (0: off; Dueling / Rainbow use 10).")),
        ("--munchausen", _flag, False, dict(help="Munchausen DQN targets: the target net's soft value of the poststate plus a scaled, clipped log-policy bonus for the action taken (alpha 0: Soft-DQN).")),
        ("--munchausen_alpha", float, 0.9, dict(help="Munchausen DQN: scale of the log-policy bonus, in [0, 1].")),
        ("--munchausen_tau", float, 0.03, dict(help="Munchausen DQN: temperature of the target net's softmax policy, > 0.")),
        ("--munchausen_clip", float, -1.0, dict(help="Munchausen DQN: lower clip of tau * ln pi(a|s), <= 0.")),
        ("--advantage_learning", float, 0.0, dict(help="Advantage learning (Bellemare et al. 2016): subtract this fraction, in [0, 1), of the target net's action gap max_a Q(s, a) - Q(s, a_taken) from the target (0: off; the paper uses 0.9).")),
        ("--persistent_advantage", _flag, False, dict(help="Persistent advantage learning: on non-terminal transitions take the larger of the advantage-learning target and the one with the poststate's gap of the same action (needs --advantage_learning > 0).")),
        ("--cql_alpha", float, 0.0, dict(help="Conservative Q-learning (Kumar et al. 2020, CQL(H)): add this multiple of logsumexp_a Q(s, a) - Q(s, a_taken) to the loss, which holds down the values of actions the data never took (0: off; offline training commonly uses 1).")),
        ("--dueling", _flag, False, dict(help="Dueling architecture (Wang et al. 2016): a value stream over one half of fc4's units and an advantage stream over the other, Q = V + Adv - mean(Adv); the network gets actions + 1 <= 18 outputs.")),
        ("--noisy_nets", _flag, False, dict(help="Noisy networks (Fortunato et al. 2018): factorised Gaussian noise on the two fully connected layers, W = mu + sigma * noise with learned sigma; one noise sample per net per train step, collecting acts under the last step's noise, testing on mu alone. Use with --exploration_rate_start 0 --exploration_rate_end 0.")),
        ("--noisy_sigma", float, 0.5, dict(help="Noisy networks: sigma starts at this value / sqrt(fan_in).")),
        ("--random_shift", int, 0, dict(help="Random-shift augmentation (DrQ, Kostrikov et al. 2020): every sampled state is replicate-padded by this many pixels (0..8) and cropped back at a random offset, prestate and poststate independently (0: off).")),
        ("--redo_interval", int, 0, dict(help="Dormant-neuron recycling (ReDo, Sokar et al. 2023): after every this many train steps, the ReLU units whose normalised mean activation on the step's minibatch is at most --redo_threshold get fresh incoming weights and zeroed outgoing ones, and their optimizer state is reset (0: off).")),
        ("--redo_threshold", float, 0.1, dict(help="Dormant-neuron recycling: a unit is dormant when its mean |activation| divided by its layer's mean is at most this, in [0, 1) (0: exactly silent units only).")),
        ("--log_dormant", _flag, False, dict(help="Measure the dormant fraction of the four ReLU layers after every train call and write it to the CSV columns dormant_1..4 (with --redo_interval alone the columns hold the last recycle event's fractions).")),
        ("--reset_interval", int, 0, dict(help="Periodic resets against the primacy bias (Nikishin et al. 2022): after every this many train steps the last --reset_layers layers of both nets are re-initialised, the others are shrunk by --shrink_perturb and perturbed, and the optimizer state is cleared there; the replay memory is kept (0: off).")),
        ("--reset_layers", int, 2, dict(help="Periodic resets: how many of the last layers (of conv1, conv2, conv3, fc4, fc5) are re-initialised in full, 0..5 (default 2: fc4 and fc5).")),
        ("--shrink_perturb", float, 1.0, dict(help="Periodic resets: the layers that are not re-initialised become ALPHA x weights + (1 - ALPHA) x a fresh draw of the initialiser (Ash & Adams 2020), ALPHA in [0, 1]; 1 (default) keeps them bit for bit, BBF uses 0.5.")),
        ("--weight_decay", float, 0.0, dict(help="Decoupled weight decay (AdamW, Loshchilov & Hutter 2019; BBF and SR-SPR use 0.1): after every train step each weight of the online net is multiplied by 1 - learning_rate x WD, for all three optimizers (0: off).")),
        ("--l2_init", float, 0.0, dict(help="L2-init regularisation (Kumar, Marklund & Van Roy 2023): after every train step each weight of the online net moves by learning_rate x LAMBDA of the way back toward its value at initialisation (or at --load_weights) (0: off).")),
        ("--log_weight_norms", _flag, False, dict(help="Measure the L2 norm of each layer's weights and their L2 distance from the --l2_init anchor when a CSV row is written: columns wnorm_1..5 and winit_1..5 (winit is nan without --l2_init).")),
        ("--quantiles", int, 1, dict(help="Quantile-regression DQN: this many quantile estimates per action (quantiles x actions <= 18), trained with the quantile Huber loss at threshold --clip_error; acting takes the mean over the quantiles (1: off).")),
        ("--bootstrap_heads", int, 1, dict(help="Bootstrapped DQN: this many Q-heads over one shared torso (heads x actions <= 18); acting follows one head per episode while training, the heads' majority vote while testing (1: off).")),
        ("--bootstrap_mask_probability", float, 1.0, dict(help="Bootstrapped DQN: probability that a Q-head trains on a transition, in (0, 1]; the mask is a fixed function of the replay slot.")),
    ],
    "Backend": [
        ("--backend", str, "hip", dict(choices=["hip", "gpu", "cpu"])), ("--device_id", int, 0),
        ("--datatype", str, "float32", dict(choices=["float16", "float32", "float64"])),
        ("--stochastic_round", int, False, dict(const=True, nargs="?")),
    ],
    "Agent": [
        ("--exploration_rate_start", float, 1), ("--exploration_rate_end", float, 0.1),
        ("--exploration_decay_steps", float, 1000000), ("--exploration_rate_test", float, 0.05),
        ("--train_frequency", int, 4), ("--train_repeat", int, 1), ("--target_steps", int, 10000), ("--random_starts", int, 30),
    ],
    "Visualization": [
        ("--visualization_filters", int, 4), ("--visualization_file", str, None),
    ],
    "Main loop": [
        ("--random_steps", int, 50000), ("--train_steps", int, 250000), ("--test_steps", int, 125000), ("--epochs", int, 200),
        ("--start_epoch", int, 0), ("--play_games", int, 0),
        ("--load_weights", str, None), ("--save_weights_prefix", str, None), ("--csv_file", str, None),
    ],
    "Common": [
        ("--random_seed", int, None),
        ("--log_level", str, "INFO", dict(choices=["DEBUG", "INFO", "WARNING", "ERROR", "CRITICAL"])),
    ],
}


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    for title, options in _OPTIONS.items():
        group = parser.add_argument_group(title)
        if title == "Environment":
            group.add_argument("game", nargs="?", default="synthetic", help="gym environment id (ignored by the synthetic environment)")
        for flag, typ, default, *extra in options:
            group.add_argument(flag, type=typ, default=default, **(extra[0] if extra else {}))
    return parser


def check_train_envs(args):
    """--train_envs N: what it cannot be combined with, refused before anything touches the device"""
    n = int(getattr(args, "train_envs", 0) or 0)
    if n < 0:
        raise ValueError("--train_envs %d: must be >= 0" % n)
    if n == 0:
        return 0
    from .environment import LIBRARY_GAMES
    if args.environment not in LIBRARY_GAMES:
        raise ValueError("--train_envs needs --environment catch, breakout or freeway (got %s): only the library's own games run on the device" % args.environment)
    if n > args.batch_size:
        raise ValueError("--train_envs %d exceeds --batch_size %d: the copies' states are one batch of the acting forward" % (n, args.batch_size))
    if getattr(args, "prioritized_replay", False):
        raise ValueError("--train_envs cannot be combined with --prioritized_replay: the sum-tree refresh takes 4 slot ranges per "
                         "launch, a lockstep writes one per lane")
    if args.replay_size % n:
        raise ValueError("--train_envs %d does not divide --replay_size %d: the ring is cut into equal lanes" % (n, args.replay_size))
    need = args.history_length + int(getattr(args, "n_step", 1)) + 2
    if args.replay_size // n < need:
        raise ValueError("--train_envs %d: lanes of --replay_size / train_envs = %d slots, at least history_length + n_step + 2 = %d needed"
                         % (n, args.replay_size // n, need))
    return n


def check_dynamics(args):
    """--frame_skip / --repeat_action_probability: their ranges and the environments that honour them, refused before anything touches
    the device"""
    k = getattr(args, "frame_skip", 1)
    k = 1 if k is None else int(k)
    p = getattr(args, "repeat_action_probability", 0.0)
    p = 0.0 if p is None else float(p)
    if not 1 <= k <= 8:
        raise ValueError("--frame_skip %d: must be in [1, 8]" % k)
    if not 0.0 <= p < 1.0:                                           # (a NaN fails both comparisons)
        raise ValueError("--repeat_action_probability %g: must be in [0, 1)" % p)
    from .environment import LIBRARY_GAMES
    if args.environment not in LIBRARY_GAMES:
        if k != 1:
            raise ValueError("--frame_skip %d needs --environment catch, breakout or freeway (got %s): only the library's own games honour it" % (k, args.environment))
        if p != 0.0:
            raise ValueError("--repeat_action_probability %g needs --environment catch, breakout or freeway (got %s): only the library's own games honour it"
                             % (p, args.environment))
    return k, p


def check_freeway_ticks(args):
    """--freeway_ticks: its range, refused before anything touches the device"""
    t = getattr(args, "freeway_ticks", 500)
    t = 500 if t is None else int(t)
    if t < 1:
        raise ValueError("--freeway_ticks %d: must be >= 1" % t)
    return t


def check_target_tau(args):
    """--target_tau: its range and what it needs, refused before anything touches the device"""
    tau = float(getattr(args, "target_tau", 0.0) or 0.0)
    if not 0.0 <= tau <= 1.0:                                        # (a NaN fails both comparisons)
        raise ValueError("--target_tau %g: must be in [0, 1]" % tau)
    if tau > 0 and not args.target_steps:
        raise ValueError("--target_tau %g needs a target network, and --target_steps 0 switches it off" % tau)
    return tau


def check_clip_grad_norm(args):
    """--clip_grad_norm: its range, refused before anything touches the device (it combines with every other option)"""
    g = getattr(args, "clip_grad_norm", 0.0)
    g = 0.0 if g is None else float(g)
    if not 0.0 <= g < float("inf"):                                  # (a NaN fails both comparisons)
        raise ValueError("--clip_grad_norm %g: must be a finite value >= 0 (0: off)" % g)
    return g


def check_munchausen(args):
    """--munchausen: the ranges of its three parameters and what it cannot be combined with, refused before anything touches the device"""
    on = bool(getattr(args, "munchausen", False))
    tau = float(getattr(args, "munchausen_tau", 0.03))
    alpha = float(getattr(args, "munchausen_alpha", 0.9))
    clip = float(getattr(args, "munchausen_clip", -1.0))
    if not (tau > 0.0 and tau < float("inf")):                       # (a NaN fails the comparison)
        raise ValueError("--munchausen_tau %g: must be > 0" % tau)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("--munchausen_alpha %g: must be in [0, 1]" % alpha)
    if not (clip <= 0.0 and clip > -float("inf")):
        raise ValueError("--munchausen_clip %g: must be <= 0" % clip)
    refuse_conflicts(args, "munchausen")
    return on


def check_offline(args):
    """--save_replay / --offline_replay: what they cannot be combined with, refused before anything touches the device.  Returns
    (save_replay, offline_replay)."""
    save, offline = getattr(args, "save_replay", None) or None, getattr(args, "offline_replay", None) or None
    train_envs = int(getattr(args, "train_envs", 0) or 0)
    if save and train_envs > 0:
        raise ValueError("--save_replay cannot be combined with --train_envs %d: laned memories have no checkpoint" % train_envs)
    if offline:
        if train_envs > 0:
            raise ValueError("--offline_replay cannot be combined with --train_envs %d: offline training collects nothing, and laned "
                             "memories have no checkpoint" % train_envs)
        if int(getattr(args, "play_games", 0) or 0):
            raise ValueError("--offline_replay cannot be combined with --play_games %d: playing trains nothing" % int(args.play_games))
        if save:
            raise ValueError("--offline_replay cannot be combined with --save_replay: the memory would be written back as it was read")
    return save, offline


def check_offline_file(args, path):
    """--offline_replay FILE against --replay_size, --screen_height / --screen_width and --history_length: a ValueError naming both values
    where they differ.  Reads the file's header only.  Returns ReplayMemory.peek's dictionary."""
    from .replay_memory import ReplayMemory
    head = ReplayMemory.peek(path)
    for key, flag, want in (("size", "--replay_size", args.replay_size), ("H", "--screen_height", args.screen_height),
                            ("W", "--screen_width", args.screen_width), ("hist", "--history_length", args.history_length)):
        if int(head[key]) != int(want):
            raise ValueError("--offline_replay %s was written with %s %d, this run has %s %d" % (path, flag, head[key], flag, want))
    return head


def run(args):
    train_envs = check_train_envs(args)
    check_random_shift(args)
    check_redo(args)
    check_reset(args)
    check_regularizer(args)
    check_noisy(args)
    check_dueling(args)
    check_bootstrap(args)
    check_quantiles(args)
    check_target_tau(args)
    check_munchausen(args)
    check_advantage_learning(args)
    check_cql(args)
    save_replay, offline_replay = check_offline(args)
    if offline_replay:
        check_offline_file(args, offline_replay)                     # (the header only: a mismatch is refused before the memory is allocated)
    check_clip_grad_norm(args)
    check_dynamics(args)
    check_freeway_ticks(args)
    from . import Agent, DeepQNetwork, ReplayMemory, SyntheticEnvironment, _lib, load
    from .environment import LIBRARY_GAMES
    from .statistics import Statistics
    logger = logging.getLogger()
    logger.setLevel(args.log_level)
    if args.random_seed:                                             # main.py:89-90
        random.seed(args.random_seed)
    if args.device_id:
        _lib.check(load().sdqn_set_device(args.device_id))
    if args.environment == "ale":
        raise NotImplementedError("the ALE wrapper (src/environment.py:35-110) is emulator I/O outside the hot path; "
                                  "use --environment gym with gymnasium[atari] installed, or the synthetic environment")
    if args.environment == "gym":
        from .environment import GymEnvironment                    # needs gymnasium (or gym); not part of this image
        env = GymEnvironment(args.game, args)
    elif args.environment in LIBRARY_GAMES:                          # the library's own games (--num_actions is ignored: they have 3)
        env = LIBRARY_GAMES[args.environment](args, seed=args.random_seed or 0)
    else:
        env = SyntheticEnvironment(args, num_actions=args.num_actions, seed=args.random_seed or 0, frame_pool=args.synthetic_frame_pool)
    mem = ReplayMemory(args.replay_size, args)                       # main.py:103-106
    net = DeepQNetwork(env.numActions(), args)
    agent = Agent(env, mem, net, args)
    stats = Statistics(agent, net, mem, env, args)
    if args.load_weights:
        net.load_weights(args.load_weights)
    if args.play_games:                                              # :112-128
        env.setMode('test')
        stats.reset()
        agent.play(args.play_games)
        stats.write(0, "play")
        if args.visualization_file:                                  # the states of the game just played, straight from the device ring
            from .visualization import visualize
            indexes = range(agent.history_length, mem.current - agent.random_starts)
            if len(indexes) == 0:
                raise ValueError("no game states to visualise: range(%d, current %d - random_starts %d) is empty (the replay memory must "
                                 "hold the whole game)" % (agent.history_length, mem.current, agent.random_starts))
            logger.info("visualising ring indexes %d..%d: %d states of the game played" % (indexes[0], indexes[-1], len(indexes)))
            visualize(net, mem, args.visualization_filters, args.visualization_file, indexes=indexes)
        if save_replay:                                              # --save_replay: the games just played
            mem.save(save_replay)
        return stats
    if offline_replay:                                               # --offline_replay: the dataset is the memory; no random phase
        mem.load(offline_replay)
        logger.info("offline training on %s: %d transitions" % (offline_replay, mem.count))
    if args.random_steps and not offline_replay:                     # :130-137
        env.setMode('train')
        stats.reset()
        if train_envs:
            agent.play_random_vectorised(args.random_steps)
            stats.record_evaluation(*agent.vectorised_tallies())
        else:
            agent.play_random(args.random_steps)
        stats.write(0, "random")
    for epoch in range(args.start_epoch, args.epochs):               # :140-162
        if args.train_steps:
            env.setMode('train')
            stats.reset()
            if offline_replay:
                agent.train_offline(args.train_steps, epoch)
            elif train_envs:
                agent.train_vectorised(args.train_steps, epoch)
                stats.record_evaluation(*agent.vectorised_tallies())
            else:
                agent.train(args.train_steps, epoch)
            stats.write(epoch + 1, "train")
            if args.save_weights_prefix:
                net.save_weights(args.save_weights_prefix + "_%d.npz" % (epoch + 1))
        if args.test_steps:
            env.setMode('test')
            stats.reset()
            if getattr(args, "eval_envs", 0) > 0:                    # vectorised on the device (the library's games only)
                if not hasattr(env, "_h"):
                    raise ValueError("--eval_envs needs --environment catch, breakout or freeway")
                stats.record_evaluation(net.evaluate(env, args.eval_envs, -(-args.test_steps // args.eval_envs), args.exploration_rate_test,
                                                     seed=(args.random_seed or 0) + epoch + 1), args.exploration_rate_test)
            else:
                agent.test(args.test_steps, epoch)
            stats.write(epoch + 1, "test")
    if save_replay:                                                  # --save_replay: the memory as the run leaves it
        mem.save(save_replay)
        logger.info("replay memory written to %s: %d transitions" % (save_replay, mem.count))
    stats.close()
    return stats


if __name__ == "__main__":
    logging.basicConfig(format='%(asctime)s %(message)s')
    run(build_parser().parse_args())
    sys.exit(0)
