"""DeepQNetwork — drop-in for /root/reference/src/deepqnetwork.py:15-192, no Neon.

Same constructor (num_actions, args), methods (train / predict / update_target_network /
load_weights / save_weights) and attributes (train_iterations, callback, batch_size, num_actions).
The whole step — target forward, online forward, TD target, clipped error, backward, RMSProp —
runs in libsdqn_hip.so on the device with zero host round trips (the reference does six, :119-171).
"""
import array
import ctypes as C
import logging

import numpy as np

from . import _lib
from ._lazy import LazyMinibatchArray

logger = logging.getLogger(__name__)

# (rows, cols) in Neon layout per layer (deepqnetwork.py:83-91): conv (C*R*S, K), affine (nout, nin);
# 84x84x4 inputs give (256, 32), (512, 64), (576, 64), (512, 3136), (A, 512)
def layer_shapes(num_actions, history_length=4, screen_height=84, screen_width=84):
    shapes, c, h, w = [], history_length, screen_height, screen_width
    for (r, s_, k, st) in ((8, 8, 32, 4), (4, 4, 64, 2), (3, 3, 64, 1)):
        assert h >= r and w >= s_, "screen too small for the layer stack of deepqnetwork.py:83-87"
        shapes.append((c * r * s_, k))
        h, w, c = (h - r) // st + 1, (w - s_) // st + 1, k
    return shapes + [(512, c * h * w), (num_actions, 512)]


MAX_ACTIONS = 18                                          # outputs of the library's head kernels (csrc/problems.h)
# the tuned net's geometry as csrc/net_layout.h states it: the ReLU units of conv1, conv2, conv3, fc4 (RELU_UNITS there is their sum) and
# the flat buffer's length in front of fc5 (OFF5)
REDO_UNITS = tuple(s[1] for s in layer_shapes(1)[:3]) + (layer_shapes(1)[3][0],)
FLAT_OFF5 = sum(r * c for r, c in layer_shapes(1)[:4])


def _flat_size(num_outputs):
    rows, cols = layer_shapes(int(num_outputs))[4]
    return FLAT_OFF5 + rows * cols


def _keyed_draw(fn, seed, event, index, layer):
    w, v = C.c_uint64(), C.c_float()
    _lib.check(fn(int(seed) & 0xFFFFFFFFFFFFFFFF, int(event), int(index), int(layer), C.byref(w), C.byref(v)))
    return w.value, np.float32(v.value)


# ---- which flags combine ---------------------------------------------------------------------------------------------
# One row per refusal: (the flag the message names first, the flag it names second, the message; a % conversion in it takes the second
# flag's value).  A pair is refused whichever of its flags is checked first; where both have words of their own (--bootstrap_heads /
# --advantage_learning) there are two rows and each flag's check speaks its own.  The rows between the library's options are its table
# (csrc/option_table.h; tests/test_option_table.py holds the two to each other) restated here, because these refusals come before the
# library is loaded; --prioritized_replay, --random_shift, --persistent_advantage / --n_step and --noisy_nets' datatype and geometry
# are this layer's alone.
def _row(first, second, tail="", value=""):
    return first, second, "--%s cannot be combined with --%s%s%s" % (first, second, value and " " + value, tail)


def _follow(section):
    return " (DESIGN.md §%d lists it as a follow-up)" % section


_NO_BN_THIRD_FORWARD = ": inference-mode statistics for its third forward are not defined"
CONFLICTS = (
    [_row("bootstrap_heads", f, _follow(27)) for f in ("double_dqn", "prioritized_replay", "munchausen", "batch_norm", "advantage_learning")]
    + [_row("quantiles", f, _follow(29)) for f in ("double_dqn", "prioritized_replay", "munchausen", "batch_norm", "advantage_learning")]
    + [_row("quantiles", "bootstrap_heads", _follow(29), "%d")]
    + [_row("dueling", f, _follow(32)) for f in ("double_dqn", "munchausen", "batch_norm", "advantage_learning")]
    + [_row("dueling", f, _follow(32), "%d") for f in ("bootstrap_heads", "quantiles")]
    + [_row("noisy_nets", "datatype", _follow(33), "%s"),
       ("noisy_nets", "geometry", "--noisy_nets needs 84 x 84 screens with --history_length 4, not --screen_height %d --screen_width %d "
                                  "--history_length %d" + _follow(33))]
    + [_row("noisy_nets", f, _follow(33)) for f in ("batch_norm", "munchausen", "dueling")]
    + [_row("noisy_nets", f, _follow(33), "%g") for f in ("clip_grad_norm", "target_tau", "advantage_learning")]
    + [_row("noisy_nets", f, _follow(33), "%d") for f in ("bootstrap_heads", "quantiles")]
    + [_row("random_shift", "batch_norm", ": the shift would change the batch statistics, and that case has no oracle"),
       _row("persistent_advantage", "n_step", " (--advantage_learning alone can): it repeats the action in the NEXT state", "%d"),
       _row("advantage_learning", "double_dqn", ": q slot 2 is taken by its third forward" + _follow(28)),
       _row("advantage_learning", "munchausen", ": both targets want q slot 2 for a head of their own"),
       _row("advantage_learning", "bootstrap_heads", _follow(28), "%d"),
       _row("advantage_learning", "batch_norm", _NO_BN_THIRD_FORWARD)]
    + [_row("cql_alpha", f, _follow(35)) for f in ("double_dqn", "munchausen", "dueling", "noisy_nets", "batch_norm")]
    + [_row("cql_alpha", "advantage_learning", _follow(35), "%g")]
    + [_row("cql_alpha", f, _follow(35), "%d") for f in ("bootstrap_heads", "quantiles")]
    + [_row("munchausen", "double_dqn", ": the Munchausen target has no argmax for the online net to choose"),
       _row("munchausen", "batch_norm", _NO_BN_THIRD_FORWARD)])
_OFF_AT = {"bootstrap_heads": 1, "quantiles": 1, "n_step": 1, "random_shift": 0, "datatype": "float32",     # a number: on above this value
           "advantage_learning": 0.0, "cql_alpha": 0.0, "clip_grad_norm": 0.0, "target_tau": 0.0}            # every other flag: a switch


def flag_setting(args, flag):
    """(whether `flag` is on in args, its value as the messages print it); a missing or None attribute is the flag's off value"""
    if flag == "geometry":
        geom = tuple(int(getattr(args, k, d)) for k, d in (("screen_height", 84), ("screen_width", 84), ("history_length", 4)))
        return geom != (84, 84, 4), geom
    off = _OFF_AT.get(flag, False)
    v = type(off)(getattr(args, flag, off) or off)
    return (v != off if isinstance(off, (bool, str)) else v > off), v


def refuse_conflicts(args, flag):
    """The "cannot be combined" part of every check_* function: ValueError in the words of the first row of CONFLICTS that pairs `flag`
    with another flag when both are on, rows that name `flag` first taken first.  Touches no device."""
    for first, second, message in sorted((r for r in CONFLICTS if flag in r[:2]), key=lambda r: r[0] != flag):
        (on1, _), (on2, value) = flag_setting(args, first), flag_setting(args, second)
        if on1 and on2:
            raise ValueError(message % value if "%" in message else message)


def check_bootstrap(args, num_actions=None):
    """--bootstrap_heads K / --bootstrap_mask_probability P: K >= 1, K x num_actions <= 18 (when num_actions is known),
    P in (0, 1], and K > 1 with none of --double_dqn, --prioritized_replay, --munchausen, --batch_norm.  Raises ValueError; touches no
    device.  Returns (K, P).  --advantage_learning is refused here too, in check_advantage_learning's words."""
    K = getattr(args, "bootstrap_heads", 1)
    K = 1 if K is None else int(K)
    P = float(getattr(args, "bootstrap_mask_probability", 1.0))
    if K < 1:
        raise ValueError("--bootstrap_heads %d: must be >= 1" % K)
    if not 0.0 < P <= 1.0:                                    # (a NaN fails the comparison)
        raise ValueError("--bootstrap_mask_probability %g: must be in (0, 1]" % P)
    if K > 1 and num_actions is not None and K * int(num_actions) > MAX_ACTIONS:      # (K = 1: the library's own range check, as ever)
        raise ValueError("--bootstrap_heads %d x %d actions = %d outputs: the network has at most %d"
                         % (K, int(num_actions), K * int(num_actions), MAX_ACTIONS))
    refuse_conflicts(args, "bootstrap_heads")
    return K, P


def check_quantiles(args, num_actions=None):
    """--quantiles N: N >= 1, N x num_actions <= 18 (when num_actions is known), and N > 1 with clip_error > 0 (the Huber
    threshold) and none of --double_dqn, --prioritized_replay, --munchausen, --advantage_learning, --bootstrap_heads > 1, --batch_norm.
    Raises ValueError; touches no device.  Returns N."""
    N = getattr(args, "quantiles", 1)
    N = 1 if N is None else int(N)
    if N < 1:
        raise ValueError("--quantiles %d: must be >= 1" % N)
    if N == 1:
        return N
    if num_actions is not None and N * int(num_actions) > MAX_ACTIONS:
        raise ValueError("--quantiles %d x %d actions = %d outputs: the network has at most %d"
                         % (N, int(num_actions), N * int(num_actions), MAX_ACTIONS))
    kappa = getattr(args, "clip_error", 1.0)
    if not float(kappa or 0.0) > 0.0:
        raise ValueError("--quantiles %d needs --clip_error > 0 (got %s): it is the Huber threshold of the quantile loss; the pure "
                         "pinball loss is not offered" % (N, kappa))
    refuse_conflicts(args, "quantiles")
    return N


def check_dueling(args, num_actions=None):
    """--dueling: num_actions + 1 <= 18 outputs (when num_actions is known) and none of --double_dqn, --munchausen,
    --advantage_learning, --bootstrap_heads > 1, --quantiles > 1, --batch_norm.  Raises ValueError; touches no device.  Returns the flag."""
    if not bool(getattr(args, "dueling", False)):
        return False
    if num_actions is not None and int(num_actions) + 1 > MAX_ACTIONS:
        raise ValueError("--dueling with %d actions needs %d outputs (V and one advantage per action): the network has at most %d"
                         % (int(num_actions), int(num_actions) + 1, MAX_ACTIONS))
    if num_actions is not None and int(num_actions) < 1:
        raise ValueError("--dueling needs at least one action, got %d" % int(num_actions))
    refuse_conflicts(args, "dueling")
    return True


def check_noisy(args):
    """--noisy_nets / --noisy_sigma: float32 on 84 x 84 x 4 and none of --batch_norm, --clip_grad_norm, --target_tau,
    --munchausen, --advantage_learning, --bootstrap_heads > 1, --quantiles > 1, --dueling.  Raises ValueError naming the flag; touches no
    device.  Returns (on, sigma0)."""
    sigma0 = float(getattr(args, "noisy_sigma", 0.5) if getattr(args, "noisy_sigma", 0.5) is not None else 0.5)
    if not bool(getattr(args, "noisy_nets", False)):
        return False, sigma0
    if not (sigma0 >= 0.0 and sigma0 < float("inf")):
        raise ValueError("--noisy_sigma %r: must be a finite value >= 0" % (sigma0,))
    refuse_conflicts(args, "noisy_nets")
    return True, sigma0


def noisy_words(seed, step, slot, layer, side, n):
    """--noisy_nets: the n 64-bit words of noise stream (seed, step, slot, layer, side), restated on the host (csrc/noisy.h; no device)"""
    out = np.empty(int(n), np.uint64)
    lib = _lib.load()
    _lib.check(lib.sdqn_noisy_words(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(slot), int(layer), int(side), out.size, _lib.ptr(out, C.c_uint64)))
    return out


def noisy_noise(seed, step, slot, layer, side, n):
    """--noisy_nets: the n unit normals z of that stream (float32); the factor is f(z) = sgn(z) sqrt|z|"""
    out = np.empty(int(n), np.float32)
    lib = _lib.load()
    _lib.check(lib.sdqn_noisy_noise(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(slot), int(layer), int(side), out.size, _lib.ptr(out, C.c_float)))
    return out


def check_random_shift(args):
    """--random_shift P: P in 0..8 (0: off), P < min(screen_height, screen_width), and P > 0 not with --batch_norm.  Raises
    ValueError naming the flag; touches no device.  Returns P."""
    P = getattr(args, "random_shift", 0)
    P = 0 if P is None else int(P)
    if not 0 <= P <= 8:
        raise ValueError("--random_shift %d: must be in [0, 8] (0: off)" % P)
    if P == 0:
        return 0
    refuse_conflicts(args, "random_shift")
    hw = (int(getattr(args, "screen_height", 84)), int(getattr(args, "screen_width", 84)))
    if P >= min(hw):
        raise ValueError("--random_shift %d needs screens larger than the shift (--screen_height %d --screen_width %d)" % ((P,) + hw))
    return P


def random_shift_draw(seed, step, n, s, P):
    """--random_shift: (dy, dx) of sample n, state s (0 prestate, 1 poststate) of shifted train step `step`, restated on the host (csrc/shift.h; no device)"""
    dy, dx = C.c_int(), C.c_int()
    _lib.check(_lib.load().sdqn_random_shift_draw(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), int(n), int(s), int(P), C.byref(dy), C.byref(dx)))
    return dy.value, dx.value


def refuse_net_properties(args, flag, batch_norm, noisy_nets, float64):
    """What --redo_interval, --reset_interval and --weight_decay / --l2_init (and their read-outs) share: `flag`, as its message prints it,
    with none of --batch_norm, --noisy_nets, --datatype float64 or screens other than 84 x 84 x 4; the three reasons are the feature's
    (csrc/option_table.h: FEATURES words the first two for the library).  Raises ValueError; touches no device."""
    if bool(getattr(args, "batch_norm", False)):
        raise ValueError("%s cannot be combined with --batch_norm: %s" % (flag, batch_norm))
    if bool(getattr(args, "noisy_nets", False)):
        raise ValueError("%s cannot be combined with --noisy_nets: %s" % (flag, noisy_nets))
    if str(getattr(args, "datatype", "float32")) == "float64":
        raise ValueError("%s cannot be combined with --datatype float64: %s" % (flag, float64))
    generic, geom = flag_setting(args, "geometry")
    if generic:
        raise ValueError("%s needs 84 x 84 screens with --history_length 4, not --screen_height %d --screen_width %d --history_length %d"
                         % ((flag,) + geom))


def check_redo(args):
    """--redo_interval N / --redo_threshold T / --log_dormant: N >= 0 (0: off), T in [0, 1), and recycling or the dormancy
    read-out with none of --batch_norm, --noisy_nets, --datatype float64 or screens other than 84 x 84 x 4 (the generic path).  Raises
    ValueError naming the flag; touches no device.  Returns (N, T, log_dormant)."""
    n = getattr(args, "redo_interval", 0)
    n = 0 if n is None else int(n)
    tau = getattr(args, "redo_threshold", 0.1)
    tau = 0.1 if tau is None else float(tau)
    log = bool(getattr(args, "log_dormant", False))
    if n < 0:
        raise ValueError("--redo_interval %d: must be >= 0 (0: off)" % n)
    if not 0.0 <= tau < 1.0:                                  # (a NaN fails both comparisons)
        raise ValueError("--redo_threshold %g: must be in [0, 1)" % tau)
    for on, flag in ((n > 0, "--redo_interval %d" % n), (log, "--log_dormant")):
        if on:
            refuse_net_properties(args, flag, "the stored planes are not what the next layer reads", "sigma would have to be recycled too",
                                  "the generic path keeps no activations to score")
    return n, tau, log


def redo_draw(seed, event, index, layer):
    """--redo_interval: (the splitmix64 word, the float32 draw) of flat internal index `index` in layer 1..4 at recycle event `event`,
    restated on the host (csrc/redo.h; no device)"""
    return _keyed_draw(_lib.load().sdqn_redo_draw, seed, event, index, layer)


def redo_apply_host(scores, tau, seed, event, num_outputs, theta, state=None, state2=None):
    """--redo_interval: one recycle event on host arrays in the library's internal layouts (flat float32 buffers of 1 683 456 + 512 x
    num_outputs values, changed in place; csrc/redo.h, no device).  Returns the four dormant counts."""
    sc = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    assert sc.size == sum(REDO_UNITS)
    n = _flat_size(num_outputs)
    for b in (theta, state, state2):
        assert b is None or (b.dtype == np.float32 and b.flags.c_contiguous and b.flags.writeable and b.size == n)
    counts = np.zeros(4, np.int64)
    _lib.check(_lib.load().sdqn_redo_apply_host(_lib.ptr(sc, C.c_float), float(tau), int(seed) & 0xFFFFFFFFFFFFFFFF, int(event), int(num_outputs),
                                                _lib.ptr(theta, C.c_float), None if state is None else _lib.ptr(state, C.c_float),
                                                None if state2 is None else _lib.ptr(state2, C.c_float), _lib.ptr(counts, C.c_int64)))
    return counts


RESET_LAYER_NAMES = ("conv1", "conv2", "conv3", "fc4", "fc5")


def check_reset(args):
    """--reset_interval N / --reset_layers L / --shrink_perturb ALPHA: N >= 0 (0: off), L in 0..5, ALPHA in [0, 1]; N > 0
    with something to do (not L = 0 with ALPHA = 1) and with none of --batch_norm, --noisy_nets, --datatype float64 or screens other than
    84 x 84 x 4 (the generic path).  Raises ValueError naming both flags; touches no device.  Returns (N, L, ALPHA)."""
    n = getattr(args, "reset_interval", 0)
    n = 0 if n is None else int(n)
    layers = getattr(args, "reset_layers", 2)
    layers = 2 if layers is None else int(layers)
    alpha = getattr(args, "shrink_perturb", 1.0)
    alpha = 1.0 if alpha is None else float(alpha)
    if n < 0:
        raise ValueError("--reset_interval %d: must be >= 0 (0: off)" % n)
    if not 0 <= layers <= 5:
        raise ValueError("--reset_layers %d: must be in 0..5" % layers)
    if not 0.0 <= alpha <= 1.0:                                # (a NaN fails both comparisons)
        raise ValueError("--shrink_perturb %g: must be in [0, 1]" % alpha)
    if n > 0:
        flag = "--reset_interval %d" % n
        if layers == 0 and alpha == 1.0:
            raise ValueError("%s with --reset_layers 0 --shrink_perturb 1 would reset nothing" % flag)
        refuse_net_properties(args, flag, "the running statistics would have to be reset too", "sigma would have to be reset too",
                              "the generic path has no reset pass")
    return n, layers, alpha


def reset_draw(seed, event, index, layer):
    """--reset_interval: (the splitmix64 word, the float32 draw) of flat internal index `index` in layer 1..5 at reset event `event`,
    restated on the host (csrc/reset.h; no device)"""
    return _keyed_draw(_lib.load().sdqn_reset_draw, seed, event, index, layer)


def reset_apply_host(layers, alpha, seed, event, num_outputs, optimizer, theta, theta_t=None, state=None, state2=None):
    """--reset_interval: one reset event on host arrays in the library's internal layouts (flat float32 buffers of 1 683 456 + 512 x
    num_outputs values, changed in place; csrc/reset.h, no device).  theta_t None or theta itself: a net without a target net."""
    n = _flat_size(num_outputs)
    for b in (theta, theta_t, state, state2):
        assert b is None or (b.dtype == np.float32 and b.flags.c_contiguous and b.flags.writeable and b.size == n)
    p = lambda b: None if b is None else _lib.ptr(b, C.c_float)
    _lib.check(_lib.load().sdqn_reset_apply_host(int(layers), float(alpha), int(seed) & 0xFFFFFFFFFFFFFFFF, int(event), int(num_outputs),
                                                 ("rmsprop", "adam", "adadelta").index(optimizer), p(theta), p(theta_t), p(state), p(state2)))


def check_regularizer(args):
    """--weight_decay WD / --l2_init LAMBDA / --log_weight_norms: WD >= 0 and LAMBDA >= 0 (0: off), learning_rate x WD < 1,
    learning_rate x LAMBDA <= 1, and any of the three with none of --batch_norm, --noisy_nets, --datatype float64 or screens other than
    84 x 84 x 4 (the generic path).  Raises ValueError naming the flag; touches no device.  Returns (WD, LAMBDA, log_weight_norms)."""
    wd = getattr(args, "weight_decay", 0.0)
    wd = 0.0 if wd is None else float(wd)
    lam = getattr(args, "l2_init", 0.0)
    lam = 0.0 if lam is None else float(lam)
    log = bool(getattr(args, "log_weight_norms", False))
    lr = float(getattr(args, "learning_rate", 0.00025))
    if not wd >= 0.0:                                         # (a NaN fails every comparison)
        raise ValueError("--weight_decay %g: must be >= 0 (0: off)" % wd)
    if not lam >= 0.0:
        raise ValueError("--l2_init %g: must be >= 0 (0: off)" % lam)
    if not lr * wd < 1.0:
        raise ValueError("--weight_decay %g: --learning_rate x --weight_decay = %g must be below 1" % (wd, lr * wd))
    if not lr * lam <= 1.0:
        raise ValueError("--l2_init %g: --learning_rate x --l2_init = %g must be at most 1" % (lam, lr * lam))
    for on, flag in ((wd > 0.0, "--weight_decay %g" % wd), (lam > 0.0, "--l2_init %g" % lam), (log, "--log_weight_norms")):
        if on:
            refuse_net_properties(args, flag, "its block of the flat buffer is not weights", "sigma would have to be regularised too",
                                  "the generic path has no regulariser pass")
    return wd, lam, log


def regularize_apply_host(weight_decay, l2_init, learning_rate, theta, anchor=None):
    """--weight_decay / --l2_init: the rule on a host array of float32 weights, changed in place (csrc/regularize.h, no device); anchor: the
    same number of float32 values, read when l2_init > 0 only."""
    assert theta.dtype == np.float32 and theta.flags.c_contiguous and theta.flags.writeable
    assert anchor is None or (anchor.dtype == np.float32 and anchor.flags.c_contiguous and anchor.size == theta.size)
    _lib.check(_lib.load().sdqn_regularize_apply_host(float(weight_decay), float(l2_init), float(learning_rate), int(theta.size),
                                                      _lib.ptr(theta, C.c_float), None if anchor is None else _lib.ptr(anchor, C.c_float)))


def check_advantage_learning(args):
    """--advantage_learning alpha / --persistent_advantage: alpha in [0, 1) (0: off), the persistent form only with
    alpha > 0 and one-step targets, and alpha > 0 with none of --double_dqn, --munchausen, --bootstrap_heads K > 1, --batch_norm.  Raises
    ValueError; touches no device.  Returns (alpha, persistent)."""
    alpha = getattr(args, "advantage_learning", 0.0)
    alpha = 0.0 if alpha is None else float(alpha)
    pal = bool(getattr(args, "persistent_advantage", False))
    if not 0.0 <= alpha < 1.0:                                # (a NaN fails both comparisons)
        raise ValueError("--advantage_learning %g: must be in [0, 1) (0: off)" % alpha)
    if pal and alpha == 0.0:
        raise ValueError("--persistent_advantage needs --advantage_learning > 0: it is a form of the same gap correction")
    if alpha == 0.0:
        return alpha, pal
    refuse_conflicts(args, "persistent_advantage")
    refuse_conflicts(args, "advantage_learning")
    return alpha, pal


def check_cql(args):
    """--cql_alpha ALPHA: a finite value >= 0 (0: off), and ALPHA > 0 with none of --double_dqn, --munchausen,
    --advantage_learning > 0, --bootstrap_heads > 1, --quantiles > 1, --dueling, --noisy_nets, --batch_norm.  Raises ValueError naming the
    flag; touches no device.  Returns alpha."""
    alpha = getattr(args, "cql_alpha", 0.0)
    alpha = 0.0 if alpha is None else float(alpha)
    if not 0.0 <= alpha < float("inf"):                       # (a NaN fails both comparisons)
        raise ValueError("--cql_alpha %g: must be a finite value >= 0 (0: off)" % alpha)
    if alpha == 0.0:
        return alpha
    refuse_conflicts(args, "cql_alpha")
    return alpha


def cql_loss(q_row, action, y, alpha, clip_error=1.0, weight=1.0):
    """--cql_alpha: (dq row, cost term) of one sample from its stored float32 row q = Q(theta, s) and its target y, restated on the host
    (csrc/cql.h; no device)"""
    q = np.ascontiguousarray(q_row, dtype=np.float32).reshape(-1)
    dq, cost = np.empty(q.size, np.float32), C.c_float()
    _lib.check(_lib.load().sdqn_cql_loss(q.size, float(alpha), float(clip_error), _lib.ptr(q, C.c_float), int(action), float(y), float(weight),
                                         _lib.ptr(dq, C.c_float), C.byref(cost)))
    return dq, np.float32(cost.value)


class DeepQNetwork:
    def __init__(self, num_actions, args):
        # Bootstrapped DQN: K Q-heads over one torso are a library net with K x num_actions outputs, row k A + a = head k, action a
        al_alpha, al_persistent = check_advantage_learning(args)
        cql_alpha = check_cql(args)
        self.noisy_nets, self.noisy_sigma = check_noisy(args)
        random_shift = check_random_shift(args)
        redo_interval, redo_threshold, self.log_dormant = check_redo(args)
        reset_interval, reset_layers, shrink_perturb = check_reset(args)
        weight_decay, l2_init, self.log_weight_norms = check_regularizer(args)
        self.bootstrap_heads, self.bootstrap_mask_probability = check_bootstrap(args, num_actions)
        # quantile-regression DQN: N quantiles per action are a library net with N x num_actions outputs, row j A + a = quantile j, action a
        self.quantiles = check_quantiles(args, num_actions)
        self._net_actions = self.bootstrap_heads * self.quantiles * num_actions
        # the dueling architecture: V and one advantage per action are a library net with num_actions + 1 outputs, row 0 = V,
        # row 1 + a = Adv_a, over the two halves of fc4's units (fc5 block-sparse: the library holds the other entries at +0.0)
        self.dueling = check_dueling(args, num_actions)
        if self.dueling:
            self._net_actions = num_actions + 1
        self._lib = _lib.load()
        self.num_actions = num_actions
        self.batch_size = args.batch_size
        self.discount_rate = args.discount_rate
        self.history_length = args.history_length
        self.screen_dim = (args.screen_height, args.screen_width)
        self._state_shape = (self.batch_size, self.history_length) + self.screen_dim      # what train() / predict() take
        self.clip_error = args.clip_error
        self.min_reward = args.min_reward
        self.max_reward = args.max_reward
        self.batch_norm = bool(getattr(args, "batch_norm", False))                      # :26
        if getattr(args, "backend", "hip") == "cpu":
            raise NotImplementedError("there is no CPU backend: libsdqn_hip is MI355X-only")
        dt = str(getattr(args, "datatype", "float32"))
        if dt not in ("float32", "float16", "float64"):                                 # main.py:53
            raise NotImplementedError("datatype %s: float16, float32 and float64 are implemented" % dt)
        self.datatype = dt
        # float64 and screens other than 84x84x4 run on the library's generic im2col + GEMM path (csrc/generic_net.hip), everything
        # else on the tuned kernels; the choice is the library's, from the configuration alone
        self._f64 = dt == "float64"
        self._np = np.float64 if self._f64 else np.float32
        self._shapes = layer_shapes(self._net_actions, self.history_length, *self.screen_dim)
        tuned_geom = (self.history_length,) + tuple(self.screen_dim) == (4, 84, 84)
        if not tuned_geom and (dt == "float16" or self.batch_norm):
            raise NotImplementedError("float16 and batch_norm are implemented for 84x84 screens with history_length 4")
        if getattr(args, "stochastic_round", False):                                    # main.py:54 -> gen_backend(stochastic_round=...)
            raise NotImplementedError("stochastic rounding (a Neon fp16 GPU-backend feature) is not implemented")
        if self.batch_norm and dt != "float32":
            raise NotImplementedError("batch_norm is implemented for float32 only")
        optimizer = getattr(args, "optimizer", "rmsprop")
        assert optimizer in ("rmsprop", "adam", "adadelta"), "Unknown optimizer"      # deepqnetwork.py:61
        self.optimizer = optimizer
        _lib.bind_device(args)                                                        # :29-34 gen_backend(device_id=args.device_id)
        cfg = _lib.NetCfg()
        cfg.batch_size, cfg.history_length = self.batch_size, self.history_length
        cfg.screen_height, cfg.screen_width = self.screen_dim
        cfg.num_actions = self._net_actions
        cfg.target_enabled = 1 if getattr(args, "target_steps", 10000) else 0          # :64
        cfg.discount_rate, cfg.clip_error = float(self.discount_rate), float(self.clip_error or 0)
        cfg.min_reward, cfg.max_reward = float(self.min_reward), float(self.max_reward)
        cfg.learning_rate = float(getattr(args, "learning_rate", 0.00025))
        cfg.decay_rate = float(getattr(args, "decay_rate", 0.95))
        cfg.optimizer = ("rmsprop", "adam", "adadelta").index(optimizer)              # :50-59
        cfg.datatype = {"float32": 0, "float16": 1, "float64": 2}[dt]                # :33
        cfg.loss_scale = float(getattr(args, "loss_scale", 1024.0))
        cfg.batch_norm = 1.0 if self.batch_norm else 0.0                              # :83-89 Conv/Affine(batch_norm=...)
        # Neon's defaults (the reference passes none): RMSProp/Adadelta epsilon 1e-6, Adam epsilon 1e-8, betas 0.9/0.999
        cfg.epsilon = float(getattr(args, "optimizer_epsilon", 1e-8 if optimizer == "adam" else 1e-6))
        cfg.beta_1, cfg.beta_2 = float(getattr(args, "beta_1", 0.9)), float(getattr(args, "beta_2", 0.999))
        h = C.c_void_p()
        _lib.check(self._lib.sdqn_net_create(C.byref(h), C.byref(cfg)))
        self._h = h
        import os
        for env, opt in (("SDQN_FUSED_LAUNCHES", b"fused_launches"), ("SDQN_XCD_MAP", b"xcd_map"), ("SDQN_H16_WGRAD_MFMA", b"h16_wgrad_mfma")):
            if os.environ.get(env) is not None:                       # A/B switches for benchmarking
                _lib.check(self._lib.sdqn_net_set_option(h, opt, int(os.environ[env])))
        if os.environ.get("SDQN_F4_SHARE"):                           # tuning: "s3,s2" percent of fc4-wgrad tiles in bwd3 / bwd2
            s3, s2 = [int(x) for x in os.environ["SDQN_F4_SHARE"].split(",")]
            _lib.check(self._lib.sdqn_net_set_option(h, b"f4_share3", s3))
            _lib.check(self._lib.sdqn_net_set_option(h, b"f4_share2", s2))
        # Double DQN targets (van Hasselt, Guez and Silver 2016): the online net picks the poststate's action, the target net values it
        self.double_dqn = bool(getattr(args, "double_dqn", False))
        if self.double_dqn:
            _lib.check(self._lib.sdqn_net_set_option(h, b"double_dqn", 1))
        # n-step returns: train() takes (prestates, actions, returns, poststates, dones) and bootstraps with discount^n
        self.n_step = int(getattr(args, "n_step", 1))
        if self.n_step != 1:
            _lib.check(self._lib.sdqn_net_set_option(h, b"n_step", self.n_step))
        # soft (Polyak) target updates: > 0 makes the library blend the target toward the online net after every train step
        self.target_tau = float(getattr(args, "target_tau", 0.0) or 0.0)
        if self.target_tau:
            self.set_target_tau(self.target_tau)
        # global gradient-norm clipping: > 0 scales the whole mean gradient to at most this L2 norm before the optimizer
        self.clip_grad_norm = 0.0
        if float(getattr(args, "clip_grad_norm", 0.0) or 0.0):
            self.set_clip_grad_norm(float(args.clip_grad_norm))
        # Munchausen DQN targets: soft value of the poststate plus a scaled, clipped log-policy bonus, both from the target net
        self.munchausen = False
        self.munchausen_alpha = float(getattr(args, "munchausen_alpha", 0.9))
        self.munchausen_tau = float(getattr(args, "munchausen_tau", 0.03))
        self.munchausen_clip = float(getattr(args, "munchausen_clip", -1.0))
        if bool(getattr(args, "munchausen", False)):
            self.set_munchausen(True)
        # advantage-learning targets: the standard target minus alpha x the target net's action gap of the taken action
        self.advantage_learning, self.persistent_advantage = 0.0, False
        if al_alpha > 0.0:                                     # (alpha = 0: the library is not told anything)
            self.set_advantage_learning(al_alpha, al_persistent)
        # conservative Q-learning: alpha x (logsumexp_k Q(s, k) - Q(s, a_taken)) added to the loss, from the step's own Q-values
        self.cql_alpha = 0.0
        if cql_alpha > 0.0:                                    # (alpha = 0: the library is not told anything)
            self.set_cql(cql_alpha)
        seed = int(getattr(args, "random_seed", 0) or 0) & 0xFFFFFFFFFFFFFFFF        # what every seeded option starts from
        self.bootstrap_seed = self.noisy_seed = self.random_shift_seed = self.redo_seed = self.reset_seed = seed
        self._boot_vote, self._boot_episode = False, 0
        if self.bootstrap_heads > 1:                           # (K = 1: the library is not told anything)
            _lib.check(self._lib.sdqn_net_set_bootstrap(h, self.bootstrap_heads, self.bootstrap_mask_probability, self.bootstrap_seed))
        if self.quantiles > 1:                                 # (N = 1: the library is not told anything)
            _lib.check(self._lib.sdqn_net_set_quantiles(h, self.quantiles))
        if self.dueling:                                       # (off: the library is not told anything)
            _lib.check(self._lib.sdqn_net_set_dueling(h, 1))
        # noisy networks: fc4 and fc5 are mu + sigma * noise; the weights (get_weights, the .npz keys) are mu
        if self.noisy_nets:                                    # (off: the library is not told anything)
            _lib.check(self._lib.sdqn_net_set_noisy(h, 1, self.noisy_sigma, self.noisy_seed))
        # random-shift augmentation: the train steps that sample from a replay memory read shifted states
        self.random_shift = 0
        if random_shift:                                       # (off: the library is not told anything)
            self.set_random_shift(random_shift)
        # dormant-neuron recycling: every redo_interval-th train step ends with one recycle event inside the library
        self.redo_interval, self.redo_threshold = 0, redo_threshold
        self._dormant_logged = None
        if redo_interval:                                      # (off: the library is not told anything)
            self.set_redo(redo_interval, redo_threshold)
        # periodic resets with shrink-and-perturb: every reset_interval-th train step ends with one reset event inside the library
        self.reset_interval, self.reset_layers, self.shrink_perturb = 0, reset_layers, shrink_perturb
        if reset_interval:                                     # (off: the library is not told anything)
            self.set_reset(reset_interval, reset_layers, shrink_perturb)
        self._mt_buf = (C.c_uint32 * _lib.MT_WORDS)()
        self._act_out = C.c_int(); self._act_greedy = self._lib.sdqn_net_act_greedy
        self._env_r, self._env_t = C.c_int(), C.c_int(); self._act_step_env = self._lib.sdqn_net_act_step_env
        self.train_iterations = 0
        self.callback = None
        self.save_weights_prefix = getattr(args, "save_weights_prefix", None)
        # Xavier init (A4): online layers first, then the target model's own draw (:65-70)
        # (gen_backend(rng_seed=args.random_seed), :31: seed 0 is a seed here, unlike main.py:89's `if args.random_seed`)
        rng = np.random.RandomState(getattr(args, "random_seed", None))
        for which in ((0, 1) if cfg.target_enabled else (0,)):
            for i, shp in enumerate(self._shapes):
                fan_in = shp[0] if i < 3 else shp[1]
                k = np.sqrt(3.0 / fan_in)
                self.set_layer(i, rng.uniform(-k, k, size=shp).astype(self._np), which)
        # decoupled weight decay and L2-init: every train step ends with one regulariser launch inside the library.  Set behind
        # the initialiser: the anchor of --l2_init is the weights as they are when the coefficient leaves 0
        self.weight_decay, self.l2_init = 0.0, 0.0
        self._weight_norms_logged = None
        if weight_decay or l2_init:                            # (off: the library is not told anything)
            self.set_regularizer(weight_decay, l2_init)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and self._lib is not None:
            self._lib.sdqn_net_destroy(h)

    # ---- weights at the boundary are ALWAYS in Neon layout --------------------------------------
    def set_layer(self, layer, w, which=0):
        w = np.ascontiguousarray(w, dtype=self._np)
        assert w.shape == self._shapes[layer], (w.shape, layer)
        if self._f64:
            _lib.check(self._lib.sdqn_net_set_weights_f64(self._h, which, layer, _lib.ptr(w, C.c_double), w.size))
        else:
            _lib.check(self._lib.sdqn_net_set_weights(self._h, which, layer, _lib.ptr(w, C.c_float), w.size))

    def get_layer(self, layer, which=0):
        w = np.empty(self._shapes[layer], dtype=self._np)
        if self._f64:
            _lib.check(self._lib.sdqn_net_get_weights_f64(self._h, which, layer, _lib.ptr(w, C.c_double), w.size))
        else:
            _lib.check(self._lib.sdqn_net_get_weights(self._h, which, layer, _lib.ptr(w, C.c_float), w.size))
        return w

    # --batch_norm: BatchNorm layer l = 0..3 (after conv1, conv2, conv3, fc4).  which as above for (beta, gamma);
    # running=True addresses (gmean, gvar) of the online (which=0) or target (which=1) net
    def get_bn(self, l, which=0, running=False):
        assert self.batch_norm and 0 <= l < 4
        c = (32, 64, 64, 512)[l]
        w = np.empty((2, c), dtype=np.float32)
        _lib.check(self._lib.sdqn_net_get_weights(self._h, (5 + which) if running else which, 5 + l, _lib.ptr(w, C.c_float), w.size))
        return w[0].copy(), w[1].copy()

    def set_bn(self, l, first, second, which=0, running=False):
        assert self.batch_norm and 0 <= l < 4
        w = np.ascontiguousarray(np.stack([first, second]), dtype=np.float32)
        assert w.shape == (2, (32, 64, 64, 512)[l])
        _lib.check(self._lib.sdqn_net_set_weights(self._h, (5 + which) if running else which, 5 + l, _lib.ptr(w, C.c_float), w.size))

    def set_weights(self, weights, which=0):
        """--dueling: the entries of W5 (layer 4, which 0 / 1) outside the two streams' blocks — row 0 over units >= 256, rows 1.. over
        units < 256 — are accepted with any value and zeroed by the library; load_weights goes through here."""
        for i, w in enumerate(weights):
            self.set_layer(i, w, which)

    def get_weights(self, which=0):
        return [self.get_layer(i, which) for i in range(5)]

    # ---- reference API ----------------------------------------------------------------------------
    def update_target_network(self):                               # :102-105
        _lib.check(self._lib.sdqn_net_update_target(self._h))

    def soft_update_target_network(self, tau):
        """One soft target update now: theta- <- theta- + tau (theta - theta-), tau in (0, 1] (1: update_target_network)."""
        _lib.check(self._lib.sdqn_net_soft_update(self._h, float(tau)))

    def set_munchausen(self, on, alpha=None, tau=None, clip=None):
        """--munchausen: switch Munchausen DQN targets on or off between steps; alpha / tau / clip left None keep their values
        (--munchausen_alpha in [0, 1], --munchausen_tau > 0, --munchausen_clip <= 0).  Refused with double_dqn and batch_norm."""
        alpha = self.munchausen_alpha if alpha is None else float(alpha)
        tau = self.munchausen_tau if tau is None else float(tau)
        clip = self.munchausen_clip if clip is None else float(clip)
        _lib.check(self._lib.sdqn_net_set_munchausen(self._h, 1 if on else 0, alpha, tau, clip))
        self.munchausen, self.munchausen_alpha, self.munchausen_tau, self.munchausen_clip = bool(on), alpha, tau, clip

    def set_advantage_learning(self, alpha, persistent=None):
        """--advantage_learning / --persistent_advantage: set the gap scale alpha in [0, 1) between steps (0 switches the option off, and the
        persistent form with it); persistent left None keeps its value.  Refused with double_dqn, munchausen, bootstrap_heads > 1 and
        batch_norm, and the persistent form with n_step > 1."""
        alpha = float(alpha)
        persistent = (self.persistent_advantage if persistent is None else bool(persistent)) and alpha != 0.0
        _lib.check(self._lib.sdqn_net_set_advantage_learning(self._h, alpha, 1 if persistent else 0))
        self.advantage_learning, self.persistent_advantage = alpha, persistent

    def set_cql(self, alpha):
        """--cql_alpha: set the regulariser's scale between steps (a finite value >= 0; 0 switches the option off).  Refused with double_dqn,
        munchausen, advantage_learning, bootstrap_heads > 1, quantiles > 1, dueling, noisy_nets and batch_norm."""
        alpha = float(alpha)
        _lib.check(self._lib.sdqn_net_set_cql(self._h, alpha))
        self.cql_alpha = alpha

    # ---- --bootstrap_heads: the acting rule of the single-environment paths (the game loops carry theirs: evaluate votes, collect follows heads)
    def set_acting(self, test):
        """test=True: act by the majority vote of the Q-heads; False: follow the Q-head of the current episode.  Nothing with one head."""
        self._boot_vote = bool(test)
        if self.bootstrap_heads > 1:
            _lib.check(self._lib.sdqn_net_bootstrap_acting(self._h, int(self._boot_vote), 0))
        if self.noisy_nets:                                     # --noisy_nets: mu alone while testing, the last step's noise while collecting
            _lib.check(self._lib.sdqn_net_noisy_acting(self._h, 0 if test else 1))

    def next_episode(self, reset=False):
        """a fresh episode starts: the episode number, which picks the Q-head to follow, advances (reset=True: returns to 0)"""
        self._boot_episode = 0 if reset else self._boot_episode + 1
        if self.bootstrap_heads > 1:
            _lib.check(self._lib.sdqn_net_bootstrap_acting(self._h, int(self._boot_vote), -1 if reset else 1))

    def acting_action(self, q_row):
        """the action of the acting rule on one raw Q row [K A] (what act_greedy returns for the buffered state)"""
        q = np.ascontiguousarray(q_row, dtype=np.float32).reshape(-1)
        assert q.size == self._net_actions
        a = C.c_int()
        if self.dueling:                                        # --dueling: the first maximum of V + Adv - mean(Adv)
            _lib.check(self._lib.sdqn_dueling_act(_lib.ptr(q, C.c_float), self.num_actions, C.byref(a), None))
            return a.value
        if self.quantiles > 1:                                  # --quantiles: the first maximum of the quantile means
            _lib.check(self._lib.sdqn_quantile_act(_lib.ptr(q, C.c_float), self.quantiles, self.num_actions, C.byref(a)))
            return a.value
        _lib.check(self._lib.sdqn_bootstrap_act(_lib.ptr(q, C.c_float), self.bootstrap_heads, self.num_actions, int(self._boot_vote),
                                                self.bootstrap_seed, 0, self._boot_episode, C.byref(a)))
        return a.value

    def set_random_shift(self, P, seed=None):
        """--random_shift: P in 1..8 shifts every state the ring-fed train steps sample (train_from_memory and its kin), 0 switches it off;
        seed left None keeps its value (--random_seed).  The step counter of the draws returns to 0.  Refused with batch_norm."""
        seed = self.random_shift_seed if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        _lib.check(self._lib.sdqn_net_set_random_shift(self._h, int(P), seed))
        self.random_shift, self.random_shift_seed = int(P), seed

    def random_shift_steps(self):
        """--random_shift: shifted train steps enqueued since set_random_shift = the step counter of the next step's draws"""
        t = C.c_int64()
        _lib.check(self._lib.sdqn_net_get_random_shift(self._h, None, C.byref(t)))
        return t.value

    def last_shifts(self):
        """--random_shift: int8 [B][2][2], the (dy, dx) of every sample's prestate [:, 0] and poststate [:, 1] as the last shifted step's
        launch drew them.  Waits for the device; raises SdqnError before the first such step."""
        out = np.empty((self.batch_size, 2, 2), np.int8)
        _lib.check(self._lib.sdqn_net_last_shifts(self._h, _lib.ptr(out, C.c_int8)))
        return out

    def set_redo(self, interval, threshold=None, seed=None):
        """--redo_interval / --redo_threshold: interval N > 0 makes every N-th train step of this net end with one recycle event inside the
        library (units whose score <= threshold get fresh incoming weights and zeroed outgoing ones), 0 switches it off; threshold and seed
        left None keep their values (--redo_threshold, --random_seed).  Refused on batch_norm, noisy, float64 / other-geometry and
        multi-rank data-parallel nets."""
        tau = self.redo_threshold if threshold is None else float(threshold)
        seed = self.redo_seed if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        _lib.check(self._lib.sdqn_net_set_redo(self._h, int(interval), tau, seed))
        self.redo_interval, self.redo_threshold, self.redo_seed = int(interval), tau, seed

    def redo_now(self):
        """One recycle event now, from the last train step's activations.  Raises SdqnError before any train step, or once a forward of
        its own (predict, acting) has overwritten them."""
        _lib.check(self._lib.sdqn_net_redo_now(self._h))

    def dormant_scores(self):
        """{"conv1": [32], "conv2": [64], "conv3": [64], "fc4": [512]} float32: every ReLU unit's mean |activation| over the online net's
        prestate half of the last train step, divided by its layer's mean (0 where the layer is silent).  Recycles nothing; usable with
        redo_interval 0.  Waits for the device; raises SdqnError where redo_now does."""
        out = np.empty(sum(REDO_UNITS), np.float32)
        _lib.check(self._lib.sdqn_net_redo_scores(self._h, _lib.ptr(out, C.c_float)))
        edges = np.cumsum((0,) + REDO_UNITS)
        return {name: out[edges[l]:edges[l + 1]].copy() for l, name in enumerate(("conv1", "conv2", "conv3", "fc4"))}

    def dormant_fraction(self, tau=None):
        """The fraction of each of the four layers' units whose score is <= tau (None: the net's redo_threshold), from dormant_scores()"""
        tau = self.redo_threshold if tau is None else float(tau)
        return tuple(float(np.mean(v.astype(np.float64) <= tau)) for v in self.dormant_scores().values())

    def last_redo(self):
        """{"event": the last recycle event's number (0: none yet), "step": the train step it followed, "dormant": its four counts}, as the
        device left them.  Waits for the device."""
        out = np.zeros(6, np.int64)
        _lib.check(self._lib.sdqn_net_redo_last(self._h, _lib.ptr(out, C.c_int64)))
        return {"event": int(out[0]), "step": int(out[1]), "dormant": tuple(int(c) for c in out[2:])}

    def set_reset(self, interval, layers=None, alpha=None, seed=None):
        """--reset_interval / --reset_layers / --shrink_perturb: interval N > 0 makes every N-th train step of this net end with one reset
        event inside the library (the last `layers` of conv1, conv2, conv3, fc4, fc5 redrawn from the initialiser, the others theta <-
        alpha theta + (1 - alpha) phi, both nets with the same phi, the optimizer state cleared there), 0 switches it off; layers, alpha and
        seed left None keep their values (--reset_layers, --shrink_perturb, --random_seed).  With interval 0 the values are what reset_now()
        uses.  Refused on batch_norm, noisy, float64 / other-geometry and multi-rank data-parallel nets."""
        layers = self.reset_layers if layers is None else int(layers)
        alpha = self.shrink_perturb if alpha is None else float(alpha)
        seed = self.reset_seed if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        _lib.check(self._lib.sdqn_net_set_reset(self._h, int(interval), layers, alpha, seed))
        self.reset_interval, self.reset_layers, self.shrink_perturb, self.reset_seed = int(interval), layers, alpha, seed

    def get_reset(self):
        """(interval, layers, alpha, seed) as the library holds them"""
        n, l, a, s = C.c_int(), C.c_int(), C.c_double(), C.c_uint64()
        _lib.check(self._lib.sdqn_net_get_reset(self._h, C.byref(n), C.byref(l), C.byref(a), C.byref(s)))
        return n.value, l.value, a.value, s.value

    def reset_now(self):
        """One reset event now, outside the schedule and numbered like the scheduled ones.  Enqueued; does not wait."""
        _lib.check(self._lib.sdqn_net_reset_now(self._h))

    def last_reset(self):
        """(the last reset event's number, 0: none yet; the train step it followed), as the device left them.  Waits for the device."""
        out = np.zeros(2, np.int64)
        _lib.check(self._lib.sdqn_net_reset_last(self._h, _lib.ptr(out, C.c_int64)))
        return int(out[0]), int(out[1])

    def set_regularizer(self, weight_decay=None, l2_init=None):
        """--weight_decay / --l2_init: either > 0 makes every applied train step of this net end with one launch of the rule
        v <- v (1 - lr WD); v <- v + lr LAMBDA (anchor - v) on the online weights, in front of the soft target update (with --target_tau the
        same launch blends the target net).  The anchor is taken when l2_init leaves 0 (anchor_now() takes it again).  None keeps a value."""
        wd = self.weight_decay if weight_decay is None else float(weight_decay)
        lam = self.l2_init if l2_init is None else float(l2_init)
        _lib.check(self._lib.sdqn_net_set_regularizer(self._h, wd, lam))
        self.weight_decay, self.l2_init = wd, lam

    def last_regularizer(self):
        """(weight_decay, l2_init) as the library holds them"""
        wd, lam = C.c_double(), C.c_double()
        _lib.check(self._lib.sdqn_net_get_regularizer(self._h, C.byref(wd), C.byref(lam)))
        return wd.value, lam.value

    def regularize_now(self, weight_decay=None, l2_init=None):
        """One launch of the rule now, outside a train step, with the net's coefficients or the ones given (l2_init > 0 needs an anchor).
        The target net is not touched.  Enqueued; does not wait."""
        if weight_decay is None and l2_init is None:
            _lib.check(self._lib.sdqn_net_regularize_now(self._h))
        else:
            _lib.check(self._lib.sdqn_net_regularize_with(self._h, float(weight_decay or 0.0), float(l2_init or 0.0)))

    def anchor_now(self):
        """The anchor of --l2_init becomes the online weights as they are now (allocated if the net has none yet).  Enqueued."""
        _lib.check(self._lib.sdqn_net_anchor_now(self._h))

    def get_anchor(self):
        """The anchor's five layers in the shapes get_weights uses.  Waits for the device."""
        out = []
        for layer, shp in enumerate(self._shapes):
            w = np.empty(shp, np.float32)
            _lib.check(self._lib.sdqn_net_get_anchor(self._h, layer, _lib.ptr(w, C.c_float), w.size))
            out.append(w)
        return out

    def weight_norms(self, squared=False):
        """(norms, distances): per layer conv1..fc5 the L2 norm of the online weights and their L2 distance from the anchor (nan without one),
        two float64 arrays of 5; squared=True returns the device's fp64 sums of squares themselves.  Three launches and a wait."""
        out = np.zeros(10, np.float64)
        _lib.check(self._lib.sdqn_net_weight_norms(self._h, _lib.ptr(out, C.c_double)))
        if not squared:
            out = np.sqrt(out)
        return out[:5].copy(), out[5:].copy()

    def logged_weight_norms(self):
        """The ten values of the CSV columns wnorm_1..5 and winit_1..5 (--log_weight_norms), measured now"""
        norms, dists = self.weight_norms()
        return tuple(float(x) for x in norms) + tuple(float(x) for x in dists)

    def _note_trained(self):
        """What every train entry point ends with.  --log_dormant: the four dormant fractions of the step just enqueued are measured now
        (two launches and a wait), while its activations are still in place; Statistics writes the last ones of a phase."""
        if self.log_dormant:
            self._dormant_logged = self.dormant_fraction()

    def logged_dormant(self):
        """The four values of the CSV columns dormant_1..4: with --log_dormant the fractions measured after the last train call, else
        (--redo_interval alone) the last recycle event's dormant counts over the layers' units; zeros before either exists."""
        if self.log_dormant:
            return self._dormant_logged or (0.0,) * 4
        return tuple(c / float(n) for c, n in zip(self.last_redo()["dormant"], REDO_UNITS))

    def set_target_tau(self, tau):
        """--target_tau: tau in (0, 1] makes every train step of this net end with one soft target update inside the library; 0: off."""
        _lib.check(self._lib.sdqn_net_set_target_tau(self._h, float(tau)))
        self.target_tau = float(tau)

    def set_clip_grad_norm(self, max_norm):
        """--clip_grad_norm: G > 0 clips the gradient of every applied train step to global L2 norm G (of the mean gradient); 0: off.
        A negative or non-finite value raises and keeps the previous one."""
        _lib.check(self._lib.sdqn_net_set_clip_grad_norm(self._h, float(max_norm)))
        self.clip_grad_norm = float(max_norm)

    def last_grad_norm(self):
        """(norm, scale) of the last clipped step: the pre-clip L2 norm of the mean gradient and the factor that was applied (1.0: nothing
        was clipped).  Waits for the device; raises SdqnError before any clipped step."""
        n, sc = C.c_double(), C.c_double()
        _lib.check(self._lib.sdqn_net_last_grad_norm(self._h, C.byref(n), C.byref(sc)))
        return n.value, sc.value

    def get_target_tau(self):
        t = C.c_double()
        _lib.check(self._lib.sdqn_net_get_target_tau(self._h, C.byref(t)))
        return t.value

    def train(self, minibatch, epoch=0):                           # :107-172
        prestates, actions, rewards, poststates, terminals = minibatch
        ps, qs, as_, rs, ts = prestates.shape, poststates.shape, actions.shape, rewards.shape, terminals.shape     # (the reference's asserts, :108-115)
        assert len(ps) == 4
        assert len(qs) == 4
        assert len(as_) == 1
        assert len(rs) == 1
        assert len(ts) == 1
        assert ps == qs
        assert ps[0] == as_[0] == rs[0] == qs[0] == ts[0]
        assert ps == self._state_shape
        act = np.ascontiguousarray(actions, dtype=np.uint8)
        if self.n_step > 1:                                        # --n_step: float64 returns R (already clipped per step), bool dones
            if np.asarray(rewards).dtype.kind in "iub":
                raise ValueError("n_step %d: train() takes float64 returns (ReplayMemory.getMinibatch), not integer rewards" % self.n_step)
            rew = np.ascontiguousarray(rewards, dtype=np.float64)
        else:
            rew = np.ascontiguousarray(rewards, dtype=np.int64)
        term = np.ascontiguousarray(terminals).astype(np.uint8)
        cost = C.c_float()
        want = self.callback is not None
        if self.optimizer == "adam":
            _lib.check(self._lib.sdqn_net_set_epoch(self._h, int(epoch)))        # optimizer.optimize(.., epoch), :165
        # The reference's loop body net.train(mem.getMinibatch()): the gathered states are still on the device.
        #  * untouched lazy views of one ReplayMemory (nobody has looked at or written the host buffers since the last gather): the step
        #    reads the device copy, the 1.8 MB never cross PCIe in either direction;
        #  * the memory's own buffers, fetched but not written since: same, declared the round-3 way;
        #  * anything else (written buffers, foreign arrays): uploaded.
        mem = None
        if (isinstance(prestates, LazyMinibatchArray) and isinstance(poststates, LazyMinibatchArray) and prestates._mem is poststates._mem
                and prestates._which == "pre" and poststates._which == "post"):
            mem = prestates._mem
            if mem._mb_pending:
                # (generation 2^64 - 1 = "the minibatch of the last gather() call, not fetched yet": the library refuses — RuntimeError —
                #  if anything has overwritten the device minibatch since; everything in this package that re-gathers into it
                #  materialises a pending minibatch first, so this is the backstop for foreign callers of the C ABI)
                _lib.check(self._lib.sdqn_replay_declare_minibatch_on_device(mem._h, 0xFFFFFFFFFFFFFFFF))
                pre_p, post_p = mem._mb_ptrs                                   # (addresses only: they name the handle's buffers)
            else:
                prestates, poststates = mem._states("pre"), mem._states("post")   # fetch; then the ordinary path below
                mem = None
        if mem is None:
            pre = np.ascontiguousarray(prestates, dtype=np.uint8)
            post = np.ascontiguousarray(poststates, dtype=np.uint8)
            pre_p, post_p = _lib.ptr(pre, C.c_uint8), _lib.ptr(post, C.c_uint8)
            owner = getattr(prestates, "_owner", None)
            m2 = owner() if owner is not None else None
            if (m2 is not None and prestates is getattr(m2, "_prestates", None) and poststates is getattr(m2, "_poststates", None)
                    and not getattr(m2, "_mb_pending", True) and not getattr(m2, "_mb_dirty", True)):
                _lib.check(self._lib.sdqn_replay_declare_minibatch_clean(m2._h))
        if self.n_step > 1:
            _lib.check(self._lib.sdqn_net_train_host_returns(self._h, pre_p, _lib.ptr(act, C.c_uint8), _lib.ptr(rew, C.c_double), post_p,
                                                             _lib.ptr(term, C.c_uint8), C.byref(cost) if want else None))
        else:
            _lib.check(self._lib.sdqn_net_train_host(self._h, pre_p, _lib.ptr(act, C.c_uint8), _lib.ptr(rew, C.c_int64), post_p,
                                                     _lib.ptr(term, C.c_uint8), C.byref(cost) if want else None))
        self.train_iterations += 1                                 # :168
        self._note_trained()
        if self.callback:
            self.callback.on_train(cost.value)                     # :171-172

    def predict(self, states):                                     # :174-186
        assert states.shape == ((self.batch_size, self.history_length,) + self.screen_dim)
        st = np.ascontiguousarray(states, dtype=np.uint8)
        q = self._predict_raw(st)
        if self.dueling:                                        # Q [B][A] = t((V + Adv_a) - (sum_b Adv_b) / A), in double, the sum in action order
            return self._dueling_q(q)
        if self.quantiles > 1:                                  # the action values [B][A]: the sum over the quantiles, in order, over N
            qs = q.reshape(self.batch_size, self.quantiles, self.num_actions)
            s = np.zeros((self.batch_size, self.num_actions), self._np)
            for j in range(self.quantiles):
                s += qs[:, j]
            return s / self._np(self.quantiles)
        if self.bootstrap_heads == 1:
            return q
        return q.reshape(self.batch_size, self.bootstrap_heads, self.num_actions).mean(axis=1, dtype=self._np)     # the head-mean [B][A]

    def predict_noisy(self, states):
        """--noisy_nets: the collecting-mode Q-values [B][A] — the online net's current mu and sigma under the last train step's noise
        (the noise of step 0 before the first); predict() reads mu alone."""
        assert self.noisy_nets, "predict_noisy needs --noisy_nets"
        assert states.shape == ((self.batch_size, self.history_length,) + self.screen_dim)
        st = np.ascontiguousarray(states, dtype=np.uint8)
        q = np.empty((self.batch_size, self._net_actions), dtype=np.float32)
        _lib.check(self._lib.sdqn_net_predict_noisy(self._h, _lib.ptr(st, C.c_uint8), _lib.ptr(q, C.c_float)))
        return q

    def get_noisy_sigma(self, which=0):
        """--noisy_nets: [sigma of fc4 (512, 3136), sigma of fc5 (A, 512)] of the online (0) or target (1) net, laid out as the weights"""
        out = []
        for layer in (3, 4):
            w = np.empty(self._shapes[layer], dtype=np.float32)
            _lib.check(self._lib.sdqn_net_get_noisy_sigma(self._h, int(which), layer, _lib.ptr(w, C.c_float), w.size))
            out.append(w)
        return out

    def set_noisy_sigma(self, sigmas, which=0):
        """--noisy_nets: set both sigmas of one net between steps (the next forward that reads them sees them)"""
        for layer, w in zip((3, 4), sigmas):
            w = np.ascontiguousarray(w, dtype=np.float32)
            assert w.shape == self._shapes[layer], (w.shape, layer)
            _lib.check(self._lib.sdqn_net_set_noisy_sigma(self._h, int(which), layer, _lib.ptr(w, C.c_float), w.size))

    def noisy_step(self):
        """--noisy_nets: t of the noise xi_t the acting paths read now = train steps this net has run"""
        t = C.c_int64()
        _lib.check(self._lib.sdqn_net_get_noisy(self._h, None, None, None, C.byref(t)))
        return t.value

    def noisy_eps(self):
        """--noisy_nets: the factor vectors f(z) last composed on the device, per net slot: [{"in4", "out4", "in5", "out5"}, ...]"""
        (o4, i4), (o5, i5) = self._shapes[3], self._shapes[4]      # fc4 (512, 3136), fc5 (A, 512); a net's block: in4 | out4 | in5 | out5 padded to 32
        n_net = i4 + o4 + i5 + 32
        raw = self.debug_read("noisy_eps", 2 * n_net)
        out = []
        for z in range(2):
            v = raw[z * n_net:(z + 1) * n_net]
            out.append(dict(in4=v[:i4].copy(), out4=v[i4:i4 + o4].copy(), in5=v[i4 + o4:i4 + o4 + i5].copy(), out5=v[i4 + o4 + i5:i4 + o4 + i5 + o5].copy()))
        return out

    def noisy_fc(self, name):
        """--noisy_nets: the fc4 / fc5 slices of a debug buffer in the weights' layout [(512, 3136), (A, 512)]: "noisy_theta",
        "noisy_theta_t" (the effective weights) or "noisy_sigma_grad" (option keep_gradients)"""
        size = lambda shp: int(np.prod(shp))
        nconv, n4, n5 = sum(size(s) for s in self._shapes[:3]), size(self._shapes[3]), size(self._shapes[4])
        units, maps = self._shapes[3][0], self._shapes[2][1]        # 512 hidden units; conv3's 64 feature maps of 49 pixels
        skip = 0 if name == "noisy_sigma_grad" else nconv
        raw = self.debug_read(name, skip + n4 + n5)[skip:]
        w4 = raw[:n4].reshape(-1, maps, units).transpose(2, 1, 0).reshape(self._shapes[3])        # internal [pix][f][unit] -> [unit][f 49 + pix]
        return [np.ascontiguousarray(w4), raw[n4:].reshape(self._shapes[4]).copy()]

    def predict_heads(self, states):
        """--bootstrap_heads: the Q-values of every Q-head, [B][K][A] (K = 1: predict() with an axis of one)"""
        assert states.shape == ((self.batch_size, self.history_length,) + self.screen_dim)
        return self._predict_raw(np.ascontiguousarray(states, dtype=np.uint8)).reshape(self.batch_size, self.bootstrap_heads, self.num_actions)

    def predict_quantiles(self, states):
        """--quantiles: the quantile estimates of every action, [B][N][A] (N = 1: predict() with an axis of one)"""
        assert states.shape == ((self.batch_size, self.history_length,) + self.screen_dim)
        return self._predict_raw(np.ascontiguousarray(states, dtype=np.uint8)).reshape(self.batch_size, self.quantiles, self.num_actions)

    def _dueling_q(self, raw):
        raw = np.asarray(raw)
        v, adv = raw[..., 0].astype(np.float64), raw[..., 1:].astype(np.float64)
        s = np.zeros(v.shape, np.float64)
        for b in range(self.num_actions):
            s = s + adv[..., b]
        return ((v[..., None] + adv) - (s / float(self.num_actions))[..., None]).astype(self._np)

    def predict_streams(self, states):
        """--dueling: the two streams' outputs (V [B], Adv [B][A]); predict() returns Q = V + Adv - mean(Adv)"""
        assert self.dueling, "predict_streams needs --dueling"
        assert states.shape == ((self.batch_size, self.history_length,) + self.screen_dim)
        raw = self._predict_raw(np.ascontiguousarray(states, dtype=np.uint8))
        return raw[:, 0].copy(), raw[:, 1:].copy()

    def _predict_raw(self, st):
        q = np.empty((self.batch_size, self._net_actions), dtype=self._np)
        if self._f64:
            _lib.check(self._lib.sdqn_net_predict_f64(self._h, _lib.ptr(st, C.c_uint8), _lib.ptr(q, C.c_double)))
        else:
            _lib.check(self._lib.sdqn_net_predict(self._h, _lib.ptr(st, C.c_uint8), _lib.ptr(q, C.c_float)))
        return q

    def predict_one(self, state):
        """Acting-path fast path: Q-values of one state u8[hist,H,W] -> float32[A]; identical to
        predict(padded_batch)[0] (agent.py:55-61) without computing the zero rows.  --bootstrap_heads K > 1: the raw row [K A]
        (acting_action turns it into an action)."""
        assert state.shape == (self.history_length,) + self.screen_dim
        st = np.ascontiguousarray(state, dtype=np.uint8)
        q = np.empty((self._net_actions,), dtype=np.float32)
        _lib.check(self._lib.sdqn_net_predict_one(self._h, _lib.ptr(st, C.c_uint8), _lib.ptr(q, C.c_float)))
        return q

    def predict_state(self, state_buffer):
        """Acting path with a DeviceStateBuffer: Q-values float32[A] of the buffered state, read in place from HBM
        (no state upload; same numbers as predict(state_buffer.getStateMinibatch())[0]; --bootstrap_heads K > 1: the raw row [K A])."""
        q = np.empty((self._net_actions,), dtype=np.float32)
        _lib.check(self._lib.sdqn_net_predict_state(self._h, state_buffer._h, _lib.ptr(q, C.c_float)))
        return q

    def act_greedy(self, state_buffer):
        """agent.py:55-59 in one call: int(np.argmax(predict_state(state_buffer)))."""
        a = self._act_out
        _lib.check(self._act_greedy(self._h, state_buffer._h, C.byref(a), None))
        return a.value

    def act_step(self, state_buffer, mem, screen, action=0, reward=0, terminal=False, speculate=False):
        """One environment transition in ONE library call: `state_buffer.add(screen)` and — with a device-backed replay memory —
        `mem.add(action, reward, screen, terminal)` (agent.py:62 / replay_memory.py:26-34); `speculate` also enqueues the acting forward of
        the new state, so that the next predict_state(state_buffer) only collects Q-values that are already on their way."""
        assert screen.shape == state_buffer.dims
        assert mem is None or screen.shape == mem.dims              # (replay_memory.py:28: mem.add's own assert)
        scr = np.ascontiguousarray(screen, dtype=np.uint8)
        rh = mem._h if mem is not None else None
        _lib.check(self._lib.sdqn_net_act_step(self._h, state_buffer._h, rh, _lib.ptr(scr, C.c_uint8), int(action), int(reward),
                                               int(bool(terminal)), int(bool(speculate))))

    def act_step_env(self, state_buffer, mem, env, action, speculate=False):
        """act_step for an environment that lives in the library (CatchEnvironment): steps the game with `action`, adds the new frame to
        the state buffer and — with a device-backed replay memory — the transition to the ring.  The frame is rendered by a kernel
        straight into the device state buffer and the ring's HBM mirror (nothing is uploaded) and by the host into their host copies.
        Returns (reward, terminal)."""
        assert env.dims == state_buffer.dims
        assert mem is None or env.dims == mem.dims
        r, t = self._env_r, self._env_t
        _lib.check(self._act_step_env(self._h, state_buffer._h, mem._h if mem is not None else None, env._h, int(action),
                                      int(bool(speculate)), C.byref(r), C.byref(t)))
        env._stepped(t.value)
        return r.value, bool(t.value)

    def _play(self, fn, head, n, steps, trace):
        """evaluate() / collect(): library call fn(*head, <five tally arrays [n]>, <four trace arrays or NULLs>) -> the dict both return."""
        tallies = ("steps", "reward", "caught", "missed", "episodes")
        out = dict((k, np.zeros(n, dtype=np.int64)) for k in tallies)
        tr = [None] * 4
        if trace:
            acts, rews = np.zeros((steps, n), np.uint8), np.zeros((steps, n), np.int8)
            terms, q = np.zeros((steps, n), np.uint8), np.zeros((steps, n, self.num_actions), np.float64)
            tr = [_lib.ptr(acts, C.c_uint8), _lib.ptr(rews, C.c_int8), _lib.ptr(terms, C.c_uint8), _lib.ptr(q, C.c_double)]
        _lib.check(fn(*(list(head) + [_lib.ptr(out[k], C.c_int64) for k in tallies] + tr)))
        if trace:
            out.update(actions=acts, rewards=rews, terminals=terms.astype(bool), q=q.astype(self._np))     # (float32 -> double -> float32: exact)
        return out

    def evaluate(self, env, num_envs, steps, epsilon=0.05, seed=0, trace=False):
        """Vectorised evaluation on the device: `num_envs` (<= batch_size) independent copies of `env`'s game (its geometry and
        balls_per_episode; env itself is not stepped), `steps` steps each, epsilon-greedy on the online net — per step one batched
        forward and one kernel, no host round trip until the end.  Returns a dict of int64 arrays [num_envs]: steps, reward (summed),
        caught, missed, episodes; with trace=True also actions / rewards / terminals [steps, num_envs] and q [steps, num_envs, A]
        (the network's precision; float64 for a float64 network)."""
        n, steps = int(num_envs), int(steps)
        head = (self._h, env._h, n, steps, float(epsilon), int(seed) & 0xFFFFFFFFFFFFFFFF)
        return self._play(self._lib.sdqn_env_eval, head, n, steps, trace)

    def collect(self, env, mem, num_envs, locksteps, epsilon=1.0, epsilon_step=0.0, seed=None, trace=False):
        """--train_envs: `locksteps` locksteps of `num_envs` copies of `env`'s game, every lockstep's num_envs transitions
        written into the laned memory `mem` (mem.set_lanes(num_envs)) by one kernel behind the batched forward (no forward while
        epsilon >= 1); no frame goes host to device, one wait at the end.  The copies live on this network between calls: an integer
        `seed` seeds them as evaluate() does, seed=None goes on where the last call stopped.  Lockstep t of the call plays with
        epsilon + t epsilon_step, clamped to [0, 1].  Returns the copies' running tallies since they were seeded, as evaluate()
        (with trace=True also actions / rewards / terminals [locksteps, num_envs] and q [locksteps, num_envs, A])."""
        n, steps = int(num_envs), int(locksteps)
        mem._check_mirror()                                        # (slots edited through the numpy views reach the mirror first)
        head = (self._h, env._h, mem._h, n, steps, float(epsilon), float(epsilon_step), -1 if seed is None else int(seed) & 0x7FFFFFFFFFFFFFFF)
        return self._play(self._lib.sdqn_env_collect, head, n, steps, trace)

    def load_weights(self, load_path):                             # :188-189
        """Own .npz snapshots, or a Neon pickle (the reference's `model.load_params`, best effort: neon_compat.py).  The anchor of --l2_init is
        not part of a snapshot: a net that loads weights anchors at what it loaded."""
        self._load_weights(load_path)
        if getattr(self, "l2_init", 0.0) > 0.0:
            self.anchor_now()

    def _load_weights(self, load_path):
        if not str(load_path).endswith(".npz"):
            from .neon_compat import read_neon_pickle
            ws, states, A = read_neon_pickle(load_path)
            assert A == self._net_actions, "snapshot has %d actions, the network %d" % (A, self._net_actions)
            for i in range(5):
                self.set_layer(i, ws[i], 0)
                if states is not None and self.optimizer == "rmsprop":
                    self.set_layer(i, states[i], 2)
            return                                                 # (online model only, like model.load_params: the target
                                                                   #  net follows at the next update_target_network, agent.py:105)
        with np.load(load_path) as f:
            has_sigma = any(k in f for k in ("NS3", "NS4", "NSt3", "NSt4"))
            if has_sigma and not self.noisy_nets:
                raise ValueError("%s holds noisy-net sigmas (keys NS3 / NS4): load it into a network created with --noisy_nets" % (load_path,))
            for which, key in ((0, "W"), (1, "Wt"), (2, "S"), (4, "S2")):
                for i in range(5):
                    name = "%s%d" % (key, i)
                    if name in f:
                        self.set_layer(i, f[name], which)
                if self.batch_norm:
                    for l in range(4):
                        if "%s_bn%d" % (key, l) in f:
                            self.set_bn(l, *f["%s_bn%d" % (key, l)], which=which)
            if self.batch_norm:
                for which, key in ((0, "run"), (1, "run_t")):
                    for l in range(4):
                        if "%s_bn%d" % (key, l) in f:
                            self.set_bn(l, *f["%s_bn%d" % (key, l)], which=which, running=True)
            # --noisy_nets: sigma of both nets ("NS3" / "NS4", "NSt3" / "NSt4"; its optimizer state does not travel).  A file without the
            # keys leaves the init sigma; a file with them is a noisy net's: a plain net has refused it by name above
            if has_sigma:
                for which, key in ((0, "NS"), (1, "NSt")):
                    if key + "3" in f and key + "4" in f:
                        self.set_noisy_sigma([f[key + "3"], f[key + "4"]], which)
            if "train_iterations" in f:
                self.train_iterations = int(f["train_iterations"])

    def save_weights(self, save_path):                             # :191-192
        """.npz (everything needed to resume: online + target weights, optimizer state, step counter) or, for a
        path ending in .prm / .pkl, a Neon-style pickle of the online model (neon_compat.py)."""
        if str(save_path).endswith((".prm", ".pkl")):
            from .neon_compat import write_neon_pickle
            write_neon_pickle(save_path, [self.get_layer(i, 0) for i in range(5)],
                              [self.get_layer(i, 2) for i in range(5)] if self.optimizer == "rmsprop" else None)
            return
        d = {}
        for which, key in ((0, "W"), (1, "Wt"), (2, "S")) + ((() if self.optimizer == "rmsprop" else ((4, "S2"),))):
            for i in range(5):
                d["%s%d" % (key, i)] = self.get_layer(i, which)
            if self.batch_norm:
                for l in range(4):
                    d["%s_bn%d" % (key, l)] = np.stack(self.get_bn(l, which))
        if self.batch_norm:
            for which, key in ((0, "run"), (1, "run_t")):
                for l in range(4):
                    d["%s_bn%d" % (key, l)] = np.stack(self.get_bn(l, which, running=True))
        if self.noisy_nets:
            for which, key in ((0, "NS"), (1, "NSt")):
                s4, s5 = self.get_noisy_sigma(which)
                d[key + "3"], d[key + "4"] = s4, s5
        d["train_iterations"] = np.int64(self.train_iterations)
        with open(save_path, "wb") as f:
            np.savez(f, **d)

    # ---- additive fast paths (SURVEY.md §8b "new, additive") ------------------------------------------
    def set_epoch(self, epoch):
        _lib.check(self._lib.sdqn_net_set_epoch(self._h, int(epoch)))

    def train_from_memory(self, mem, n_steps=1, use_global_random=True, mt_state=None, want_cost=None):
        """n_steps x { sample ; fused gather+train } entirely inside the library (agent.py:108-114's
        loop body).  Consumes Python's global random stream unless an explicit 625-word mt_state
        (ctypes uint32 array) is given."""
        import random
        mem._check_mirror()
        self._keep_pending_minibatch(mem)
        if mt_state is None:
            # Python's generator state goes in as a copy (array('I') of the 625 words: 6 us; a ctypes slice assignment took 25); afterwards
            # Python's own generator is advanced by exactly the 32-bit words the library drew — one getrandbits call instead of
            # rebuilding a 625-tuple and random.setstate (another 40 us per call)
            st = random.getstate()
            arr = array.array("I", st[1])
            mt = (C.c_uint32 * _lib.MT_WORDS).from_buffer(arr)
            w0 = C.c_uint64(); self._lib.sdqn_mt_words(C.byref(w0))
        else:
            mt = mt_state

        def resync():
            if mt_state is None:
                w1 = C.c_uint64(); self._lib.sdqn_mt_words(C.byref(w1))
                n = w1.value - w0.value
                if n:
                    random.getrandbits(32 * n)                     # ceil(k / 32) genrand_uint32 calls: the same n words (Modules/_randommodule.c)

        want = (self.callback is not None) if want_cost is None else want_cost
        cost = C.c_float()
        if self.callback is not None and n_steps > 1:
            # the reference reports every step to the callback (deepqnetwork.py:168-172: train_iterations, then
            # on_train(cost)): step by step, so Statistics' running mean sees the same sequence; no callback -> one call
            total = 0.0
            try:
                for _ in range(int(n_steps)):
                    _lib.check(self._lib.sdqn_net_train_many(self._h, mem._h, mt, 1, C.byref(cost)))
                    self.train_iterations += 1
                    self._note_trained()
                    self.callback.on_train(cost.value)
                    total += cost.value
            finally:
                resync()
            return total / n_steps if want else None
        if self.callback is not None and n_steps == 1 and want_cost is None and hasattr(self.callback, "on_train_deferred"):
            # the callback can take the cost later: enqueue the step, hand it a collector (deepqnetwork.py:168-172, order kept)
            ticket = C.c_int64()
            try:
                _lib.check(self._lib.sdqn_net_train_many_deferred(self._h, mem._h, mt, 1, C.byref(ticket)))
            finally:
                resync()
            self.train_iterations += 1
            self._note_trained()
            tk = ticket.value

            def collect(tk=tk):
                c = C.c_float()
                _lib.check(self._lib.sdqn_net_cost_collect(self._h, tk, C.byref(c)))
                return c.value
            self.callback.on_train_deferred(collect, self.train_iterations)
            return None
        try:
            _lib.check(self._lib.sdqn_net_train_many(self._h, mem._h, mt, int(n_steps), C.byref(cost) if want else None))
        finally:
            resync()
        self.train_iterations += n_steps
        if n_steps:
            self._note_trained()
        if self.callback and n_steps:
            self.callback.on_train(cost.value)
        return cost.value if want else None

    def _keep_pending_minibatch(self, mem):
        """A getMinibatch() whose states nobody has looked at yet lives ONLY in the device minibatch.  The generic path (float64, other
        screen geometries) gathers a fused step's states into that very buffer: fetch the pending one to the host first, so that a
        later net.train(mb) / np.asarray(mb[0]) still sees its own states.  The tuned 84x84x4 path gathers inside conv1 and never
        touches the buffer — except with --random_shift > 0, whose launch writes every step's shifted states there."""
        if getattr(mem, "_mb_pending", False) and (self.random_shift > 0 or self.step_structure()[0] == "generic"):
            mem._materialize()

    def train_indexes(self, mem, indexes, want_cost=False):
        idx = np.ascontiguousarray(indexes, dtype=np.int64)
        mem._check_mirror()
        self._keep_pending_minibatch(mem)
        cost = C.c_float()
        _lib.check(self._lib.sdqn_net_train_replay(self._h, mem._h, _lib.ptr(idx, C.c_int64), C.byref(cost) if want_cost else None))
        self.train_iterations += 1
        self._note_trained()
        return cost.value if want_cost else None

    def visualize(self, states=None, mem=None, indexes=None, max_fm=4, timing=None):
        """Guided-backpropagation filter visualisation (the reference's --visualization_file; visualization.py, Neon's DeconvCallback).
        The states are host arrays u8[N,4,84,84] or ring indexes of a ReplayMemory (mem + indexes: getState(i) of each, read on the
        device).  Returns one dict per conv layer with, for each of its first min(K, max_fm) maps, the winning state ("state": its
        position in `states` / `indexes`), output position ("pos", row-major), pre-activation value ("value") and the projection
        ("vis": float32 [F,4,84,84]).  timing: a dict that receives the device ms of the two launches ("search_ms", "project_ms")."""
        if self._f64 or self.screen_dim != (84, 84) or self.history_length != 4:
            raise NotImplementedError("filter visualisation is implemented for 84x84x4 float32 / float16 networks")
        if self.batch_norm:
            raise NotImplementedError("filter visualisation is not implemented for batch_norm networks")
        if (states is None) == (mem is None) or (mem is None) != (indexes is None):
            raise ValueError("give either states or (mem, indexes)")
        if mem is not None:
            idx = np.ascontiguousarray(indexes, dtype=np.int64).reshape(-1)
            n = idx.size
            mem._check_mirror()                                    # slots edited through the numpy views reach the HBM ring first
            src = (mem._h, _lib.ptr(idx, C.c_int64), None)
        else:
            st = np.ascontiguousarray(states, dtype=np.uint8)
            assert st.ndim == 4 and st.shape[1:] == (4, 84, 84), st.shape
            n = st.shape[0]
            src = (None, None, _lib.ptr(st, C.c_uint8))
        F = [min(k, int(max_fm)) for k in (32, 64, 64)] if max_fm >= 1 else [0, 0, 0]
        R = sum(F)
        rs, rp = np.zeros(max(R, 1), np.int64), np.zeros(max(R, 1), np.int32)
        rv, vis = np.zeros(max(R, 1), np.float32), np.zeros((max(R, 1), 4, 84, 84), np.float32)
        ms = np.zeros(2, np.float32)
        _lib.check(self._lib.sdqn_net_visualize(self._h, src[0], src[1], src[2], int(n), int(max_fm), _lib.ptr(rs, C.c_int64),
                                                _lib.ptr(rp, C.c_int32), _lib.ptr(rv, C.c_float), _lib.ptr(vis, C.c_float),
                                                _lib.ptr(ms, C.c_float) if timing is not None else None))
        if timing is not None:
            timing["search_ms"], timing["project_ms"] = float(ms[0]), float(ms[1])
        out, o = [], 0
        for f in F:
            out.append({"state": rs[o:o + f].copy(), "pos": rp[o:o + f].copy(), "value": rv[o:o + f].copy(), "vis": vis[o:o + f].copy()})
            o += f
        return out

    def set_option(self, name, value):
        """Tuning / test hooks of the library (sdqn_net_set_option), e.g. 'keep_gradients' (materialise the fc4 gradient; disables the
        fused fc4 RMSProp), 'fused_launches', 'bt:<kernel id>' (throughput-regime menu), 'nw:<id>', 'tps:<layer>', 's4'.  Retired
        experiments ('two_streams', ...) are refused by name.  'double_dqn' (0 / 1) switches Double DQN targets between steps, 'n_step'
        (1..16) n-step returns."""
        _lib.check(self._lib.sdqn_net_set_option(self._h, name.encode(), int(value)))
        if name == "dp_overlap":
            self._dp_overlap_opt = int(value)
        elif name == "double_dqn":
            self.double_dqn = bool(value)
        elif name == "n_step":
            self.n_step = int(value)

    def sync(self):
        _lib.check(self._lib.sdqn_net_sync(self._h))

    def last_q(self):
        preq = np.empty((self.batch_size, self._net_actions), dtype=np.float32)
        mq = np.empty((self.batch_size,), dtype=np.float32)
        _lib.check(self._lib.sdqn_net_last_q(self._h, _lib.ptr(preq, C.c_float), _lib.ptr(mq, C.c_float)))
        return preq, mq

    def last_quantile_step(self):
        """--quantiles N > 1: (targets float64[B, N], dq float64[B, N * A]) of the last train step's head, on every path"""
        t = np.empty((self.batch_size, self.quantiles), np.float64)
        dq = np.empty((self.batch_size, self._net_actions), np.float64)
        _lib.check(self._lib.sdqn_net_last_quantile_step(self._h, _lib.ptr(t, C.c_double), _lib.ptr(dq, C.c_double)))
        return t, dq

    def last_dueling_step(self):
        """--dueling: (y float64[B], delta float64[B], dq float64[B, A + 1]) of the last train step's head, on every path"""
        y, d = np.empty(self.batch_size, np.float64), np.empty(self.batch_size, np.float64)
        dq = np.empty((self.batch_size, self._net_actions), np.float64)
        _lib.check(self._lib.sdqn_net_last_dueling_step(self._h, _lib.ptr(y, C.c_double), _lib.ptr(d, C.c_double), _lib.ptr(dq, C.c_double)))
        return y, d, dq

    def debug_read(self, name, n):
        out = np.empty(int(n), dtype=np.float32)
        _lib.check(self._lib.sdqn_net_debug_read(self._h, name.encode(), _lib.ptr(out, C.c_float), out.size))
        return out

    # ---- per-kernel device timing (bench.py roofline leg) -------------------------------------------
    def profile(self, enable, kernel=-1):
        _lib.check(self._lib.sdqn_net_profile(self._h, int(bool(enable)), int(kernel)))

    def profile_reset(self):
        _lib.check(self._lib.sdqn_net_profile_reset(self._h))

    def profile_read(self):
        n = C.c_int()
        _lib.check(self._lib.sdqn_net_profile_count(C.byref(n)))
        out = []
        for k in range(n.value):
            name, ms, cnt = C.c_char_p(), C.c_double(), C.c_int64()
            _lib.check(self._lib.sdqn_net_profile_read(self._h, k, C.byref(name), C.byref(ms), C.byref(cnt)))
            out.append(dict(id=k, name=name.value.decode(), total_ms=ms.value, launches=cnt.value))
        return out

    # ---- data parallel -----------------------------------------------------------------------------
    def dp_init(self, unique_id, rank, nranks, rccl=None, vote=None, probe_timeout_ms=5000, inject_probe_timeout=False):
        """One learner per GPU: RCCL communicator over `nranks` ranks.  With option "dp_overlap" at its default (-1, auto) and
        nranks >= 2 the OVERLAPPED form (fc4's 95 % of the gradient all-reduced + applied on a second communicator under the rest of
        the step) is tried by rule: every rank probes it with bounded waits (sdqn_dp_probe), the ranks agree through `vote` — a
        callable taking this rank's bool and returning the AND over all ranks, e.g. a gloo all-reduce(MIN) of the control plane — and
        all of them activate it, or all of them tear the second communicator down and run the serial form (one all-reduce on the
        library stream).  Without a `vote` the ranks cannot agree, so the serial form runs.  dp_form() says which one it is."""
        path = (rccl or _lib.rccl_path()).encode()
        # Every rank must issue the SAME control-plane collectives whatever happens locally: the ranks whose start-up went fine will sit
        # in the vote, so a rank whose init / probe raised casts vote(False) before it re-raises — and whether a vote happens
        # at all is decided from facts every rank shares (nranks, the dp_overlap option), not from this rank's communicator state.
        req = self._dp_overlap_req()                                  # (-2: auto also for a 1-rank communicator, tests)
        will_vote = vote is not None and ((nranks >= 2 and req == -1) or req == -2)
        try:
            _lib.check(self._lib.sdqn_dp_init(self._h, path, unique_id, rank, nranks))
            form = self.dp_form()
            probing = form["form"] == "serial" and form["second_communicator"] and not form["overlap_forced"]
            ok = C.c_int(0)
            if probing:
                _lib.check(self._lib.sdqn_dp_probe(self._h, int(probe_timeout_ms), int(bool(inject_probe_timeout)), C.byref(ok)))
        except Exception:
            if will_vote:
                vote(False)
            raise
        if probing or will_vote:
            agreed = bool(vote(bool(ok.value) and probing)) if will_vote else False
            if probing:
                _lib.check(self._lib.sdqn_dp_set_overlap(self._h, int(agreed)))
            self._dp_vote = dict(local_probe_ok=bool(ok.value), agreed=agreed, voted=will_vote)
        return self.dp_form()

    def _dp_overlap_req(self):
        return getattr(self, "_dp_overlap_opt", -1)

    STEP_STRUCTURES = ("fused", "h16_block_tile", "dp_overlap", "unfused", "generic")
    UPDATE_FORMS = ("single", "dp_serial", "dp_overlap", "grad_only", "clip")

    def step_structure(self):
        """(launch structure of a train step, form of its optimizer pass) — DESIGN.md 12's table, as the library itself sees this handle."""
        a, b = C.c_int(), C.c_int()
        _lib.check(self._lib.sdqn_net_step_structure(self._h, C.byref(a), C.byref(b)))
        return self.STEP_STRUCTURES[a.value], self.UPDATE_FORMS[b.value]

    def tuple_counters(self):
        """How train(minibatch) calls have been served: (calls, states read from the device minibatch in place, nothing uploaded at all)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self._lib.sdqn_net_tuple_counters(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def dp_form(self):
        """Which data-parallel form runs: 'none' / 'serial' / 'overlapped', the start-up probe's local result and the vote."""
        f, p, c2 = C.c_int(0), C.c_int(-1), C.c_int(0)
        _lib.check(self._lib.sdqn_dp_form(self._h, C.byref(f), C.byref(p), C.byref(c2)))
        d = dict(form=("none", "serial", "overlapped")[f.value], probe={-1: None, 0: False, 1: True}[p.value],
                 second_communicator=bool(c2.value), overlap_forced=(f.value == 2 and p.value == -1))
        d.update(getattr(self, "_dp_vote", {}))
        return d

    def overflow_steps(self):
        """float16 mode under data parallel: steps skipped because the all-reduced half gradient overflowed."""
        n = C.c_int64()
        _lib.check(self._lib.sdqn_net_overflow_steps(self._h, C.byref(n)))
        return n.value

    def dp_info(self):
        """What RCCL reports about the communicator + the bound device (all -1 without a communicator)."""
        v = [C.c_int(-1) for _ in range(4)]
        _lib.check(self._lib.sdqn_dp_info(self._h, *[C.byref(x) for x in v]))
        return dict(comm_ranks=v[0].value, comm_rank=v[1].value, comm_device=v[2].value, bound_device=v[3].value)

    def apply_update(self, bsz):
        """Optimizer step on the gradient sums currently in the flat buffer (which=3) with divisor bsz: the second half of
        a data-parallel step (see option 'grad_only')."""
        _lib.check(self._lib.sdqn_net_apply_update(self._h, float(bsz)))

    def flat_size(self):
        """values in the flat weight / gradient buffer (float16 networks have no BatchNorm block)"""
        n, tot = C.c_int64(), 0
        for layer in range(5):
            _lib.check(self._lib.sdqn_net_layer_size(self._h, layer, C.byref(n)))
            tot += n.value
        return tot

    def grad_to_half(self):
        """float16 data parallel, first half of the exchange: the flat gradient sums scaled by the payload scale as IEEE half
        (np.float16 array, internal layout) — what a rank hands to the all-reduce."""
        out = np.empty(self.flat_size(), dtype=np.float16)
        _lib.check(self._lib.sdqn_net_grad_to_half(self._h, out.ctypes.data_as(C.POINTER(C.c_uint16)), out.size))
        return out

    def grad_from_half(self, payload):
        """... second half: the SUMMED half payload back into the fp32 gradient buffer; apply_update() then honours its overflow flag."""
        p = np.ascontiguousarray(payload, dtype=np.float16)
        _lib.check(self._lib.sdqn_net_grad_from_half(self._h, p.ctypes.data_as(C.POINTER(C.c_uint16)), p.size))

    def half_payload_state(self):
        v = [C.c_int() for _ in range(3)]
        _lib.check(self._lib.sdqn_net_half_payload_state(self._h, *[C.byref(x) for x in v]))
        return dict(overflow=v[0].value, scale_log2=v[1].value, clean_steps=v[2].value)

    def dp_shutdown(self):
        _lib.check(self._lib.sdqn_dp_shutdown(self._h))


def dp_unique_id(rccl=None):
    buf = C.create_string_buffer(128)
    path = (rccl or _lib.rccl_path()).encode()
    _lib.check(_lib.load().sdqn_dp_unique_id(path, buf))
    return buf.raw
