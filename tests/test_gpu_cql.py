"""--cql_alpha on the GPU against the CQL restatement of the numpy oracles (tests/cql_oracle.py).  Configurations, bounds and
gradient rules are those of tests/test_gpu_advantage_learning.py for the same cell (the cells share their code path: head_body.h around
a few lines of their own); the CQL term adds one double-to-float cast.  The oracle of a float32 net runs in float64 on the same float32
draws, for the reason that file's docstring gives; float16 nets keep the half oracle.

Every parity test first checks, on the oracle alone, that the regulariser moves the gradient: every fc5 row of every sample carries some,
and off the taken action it is far above the bound.  A library that ignores alpha, or writes the taken action's row only, fails the
comparison that follows."""
import random

import numpy as np
import pytest

import cql_oracle as CO
import nstep_oracle as N
from oracle.dqn_numpy import xavier_weights
from test_gpu_advantage_learning import _force
from test_gpu_double_dqn import _minibatch
from test_gpu_munchausen import CONFIGS as MU_CONFIGS, _cfg, _check_grads, _check_priorities, _dt, _layers
from test_gpu_nstep import GAMMA, MAXR, MINR, _mems, _per_kw
from test_gpu_quantile import _counts
from util import make_args

pytestmark = pytest.mark.gpu

ALPHA = 1.0
ERR_ARG = -1                                                 # include/sdqn.h: SDQN_ERR_ARG
CONFIGS = dict((k, MU_CONFIGS[k]) for k in ("fp32_b32", "fp32_b128", "fp16_b32", "f64_b8", "f32_generic", "a5_b3"))
CONFIGS["a18_b3"] = (18, 3, (4, 84, 84), {}, 1e-4, 1e-4)     # AMAX 18, as a5_b3 is AMAX 8


def _c(name):
    return CONFIGS[name] if isinstance(name, str) else _cfg(name)


@pytest.fixture(scope="module")
def sd():
    import simple_dqn_amd
    return simple_dqn_amd


class _Cost:
    cost = None

    def on_train(self, cost):
        self.cost = cost


def _oracle(name, ws, wt, cls=CO.CQLOracle, alpha=ALPHA, **attrs):
    A, B, (hist, H, W), kw, _, _ = _c(name)
    half = kw.get("datatype") == "float16"
    o = cls(A, batch_size=B, history_length=hist, screen_height=H, screen_width=W, dtype=np.float32 if half else np.float64, weights=ws,
            half_activations=half)
    o.Wt = [np.array(w, dtype=o.dtype) for w in wt]
    o.cql_alpha = alpha
    for k, v in attrs.items():
        setattr(o, k, v)
    return o


def _net(sd, name, ws, wt, alpha=ALPHA, **extra):
    A, B, geom, kw, _, _ = _c(name)
    opt = {} if alpha is None else dict(cql_alpha=alpha)
    net = sd.DeepQNetwork(A, make_args(batch_size=B, history_length=geom[0], screen_height=geom[1], screen_width=geom[2], **kw, **opt, **extra))
    net.set_weights(wt, 1)
    net.set_weights(ws, 0)
    return net


def _weights(name, seed):
    A, _, geom, kw, _, _ = _c(name)
    return xavier_weights(A, seed, _dt(kw), *geom), xavier_weights(A, seed + 100, _dt(kw), *geom)


def _discriminates(o, actions, tol):
    """on the oracle alone: every row of every sample carries gradient, and off the taken action it exceeds 100 x the bound everywhere"""
    dq = np.abs(np.asarray(o.last_dq, np.float64))
    off = np.ones(dq.shape, bool)
    off[np.arange(len(actions)), np.asarray(actions, np.int64)] = False
    return bool((dq > 0).all() and (dq.shape[1] == 1 or dq[off].min() > 100 * max(tol, 1e-6) / dq.shape[1]))


def _check_q(net, preq, maxq, tol):
    tol = max(tol, 1e-6)                                     # (last_q returns float32)
    q, mq = net.last_q()
    eq, ev = np.abs(q - preq).max(), np.abs(mq - maxq).max()
    print("Q(pre) max abs err %.3e, maxq max abs err %.3e" % (eq, ev))
    assert eq < tol * max(1.0, float(np.abs(preq).max()))
    assert ev < 3 * tol * max(1.0, float(np.abs(maxq).max()))


def _check_cost(cost, ref, kw):
    rt = 1e-2 if kw.get("datatype") == "float16" else 1e-5   # a mean of B float terms; the half net's Q carry 3e-3
    print("cost %.8g, oracle %.8g" % (cost, ref))
    assert abs(cost - float(ref)) <= rt * max(1.0, abs(float(ref)))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_step_parity(sd, name):
    A, B, geom, kw, tol, _ = CONFIGS[name]
    mb = _minibatch(B, A, geom, 5)
    ws, wt = _weights(name, 11)
    net, o = _net(sd, name, ws, wt), _oracle(name, ws, wt)
    net.set_option("keep_gradients", 1)
    net.callback = _Cost()
    g, cost, _, preq = o.gradients(mb)
    assert _discriminates(o, mb[1], tol)
    net.train(mb)
    _check_q(net, preq, o.fprop(o.Wt, o._normalize(mb[3])).max(1), tol)
    _check_cost(net.callback.cost, cost, kw)
    _check_grads(net, CONFIGS[name], g)
    assert net.cql_alpha == ALPHA


def _ring_seed(name, mem, om, ws, wt, cls, n):
    """tests/test_gpu_advantage_learning.py::_ring_seed for this oracle: the first sampling seed whose three uniform minibatches keep every
    fc4 pre-activation further than 1e-6 from zero"""
    B = _c(name)[1]
    for seed in range(17, 37):
        o = _oracle(name, ws, wt, cls, n_step=n)
        random.seed(seed)
        ok = True
        for s in range(3):
            idx = np.array(mem.sample_indexes(), dtype=np.int64)
            mb = N.gather(om, idx, n, GAMMA, MINR, MAXR) if n > 1 else om.gather(idx)
            _, (_, _, a3f, _) = o.fprop(o.W, o._normalize(mb[0]), keep=True)
            ok = ok and float(np.abs(a3f @ o._h(o.W[3]).T).min()) > 1e-6
            g = o.gradients(mb)[0]
            o.optimize(g, B)
            o.W = [np.asarray(w, np.float32).astype(o.dtype) for w in o.W]
        if ok:
            return seed
    pytest.fail("no sampling seed with a well-conditioned reference")


def _composed(sd, n, per):
    """three teacher-forced steps through train_from_memory on a 600-slot ring with terminals against the combined oracle fed the same
    indexes, at A = 5: Q(pre), maxq, every gradient; PER: the priorities written back"""
    name = (5, 32, (4, 84, 84), {}, 1e-4, 1e-4)
    A, B, geom, kw, tol, _ = name
    per_kw = _per_kw() if per else {}
    mem, om = _mems(sd, name, n, size=600, **dict(dict(cql_alpha=ALPHA), **per_kw))
    ws, wt = _weights(name, 71)
    net = _net(sd, name, ws, wt, n_step=n, **per_kw)
    net.set_option("keep_gradients", 1)
    cls = CO.CQLOracleNStep if n > 1 else CO.CQLOracle
    o = _oracle(name, ws, wt, cls, n_step=n)
    random.seed(17 if per else _ring_seed(name, mem, om, ws, wt, cls, n))      # (PER samples by the net's priorities: no oracle-only walk)
    seen_done = False
    for s in range(3):
        _force(net, o)
        st = random.getstate()
        net.train_from_memory(mem, 1)
        if per:
            idx, w = mem.last_sample()
            o.weights = w
        else:
            after = random.getstate()
            random.setstate(st)
            idx = np.array(mem.sample_indexes(), dtype=np.int64)
            random.setstate(after)
        mb = N.gather(om, idx, n, GAMMA, MINR, MAXR) if n > 1 else om.gather(idx)
        seen_done = seen_done or bool(np.asarray(mb[4]).any())
        g, _, _, preq = o.gradients(mb)
        assert _discriminates(o, mb[1], tol)
        _check_q(net, preq, o.fprop(o.Wt, o._normalize(mb[3])).max(1), tol)
        _check_grads(net, name, g)
        if per:
            _check_priorities(mem, idx, o, kw)
        o.optimize(g, B)
    assert seen_done


def test_composed_with_n_step(sd):
    _composed(sd, 3, False)


def test_composed_with_prioritized_replay(sd):
    _composed(sd, 1, True)


def test_composed_with_both(sd):
    _composed(sd, 3, True)


@pytest.mark.parametrize("name", ["fp32_b32", "f64_b8"])
def test_one_action_and_alpha_zero_are_bit_identical_to_standard(sd, name):
    """A = 1: pi = 1 exactly, the regulariser is +0; alpha = 0: nothing new runs.  Three steps leave the weights of a standard net"""
    A, B, geom, kw, _, _ = CONFIGS[name]
    for acts, alphas in ((1, (ALPHA, None)), (A, (0.0, None))):
        mbs = [_minibatch(B, acts, geom, 40 + s) for s in range(3)]
        ws, wt = xavier_weights(acts, 41, _dt(kw), *geom), xavier_weights(acts, 141, _dt(kw), *geom)
        cfg = (acts, B, geom, kw, 0, 0)
        nets = [_net(sd, cfg, ws, wt, alpha=alpha) for alpha in alphas]
        assert nets[0].cql_alpha == alphas[0] and nets[1].cql_alpha == 0.0
        counts = [_counts(net, lambda: [net.train(mb) for mb in mbs], n=1) for net in nets]
        if alphas[0] == 0.0:
            assert counts[0] == counts[1]                    # the same launches
        for a, b in zip(_layers(nets[0]), _layers(nets[1])):
            assert np.array_equal(a, b)
        assert np.array_equal(nets[0].last_q()[1], nets[1].last_q()[1])


@pytest.mark.parametrize("name", ["fp32_b32", "fp16_b32", "f64_b8", "f32_generic"])
def test_ten_free_running_steps_with_target_sync(sd, name):
    A, B, geom, kw, tol, tol10 = CONFIGS[name]
    mbs = [_minibatch(B, A, geom, 100 + s, p_term=0.05) for s in range(10)]
    ws, wt = _weights(name, 21)
    net, o = _net(sd, name, ws, wt), _oracle(name, ws, wt)
    for s in range(10):
        if s == 5:
            net.update_target_network(); o.update_target_network()
        net.train(mbs[s])
        o.train(mbs[s])
    hold = _minibatch(B, A, geom, 99)[0]
    ref = o.predict(hold)
    err = np.abs(net.predict(hold) - ref).max()
    print("%s: Q max abs err after 10 steps %.3e" % (name, err))
    assert err < tol10 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.parametrize("name", ["fp32_b32", "fp32_b128", "fp16_b32"])
def test_launches_per_step(sd, name):
    """a CQL step launches exactly what the default step launches, and a prioritized CQL step what the prioritized default launches"""
    A, B, geom, kw, _, _ = CONFIGS[name]
    mb = _minibatch(B, A, geom, 50)
    ws, wt = _weights(name, 52)
    cql, std = _net(sd, name, ws, wt), _net(sd, name, ws, wt, alpha=None)
    assert cql.step_structure() == std.step_structure()
    c_cql, c_std = _counts(cql, lambda: cql.train(mb)), _counts(std, lambda: std.train(mb))
    print(name, c_cql, c_std)
    assert c_cql == c_std
    m1, _ = _mems(sd, CONFIGS[name], 1, **_per_kw())          # a fresh memory each, as tests/test_gpu_nstep.py: the first calls on one differ
    m2, _ = _mems(sd, CONFIGS[name], 1, **_per_kw())
    p_cql, p_std = _net(sd, name, ws, wt, **_per_kw()), _net(sd, name, ws, wt, alpha=None, **_per_kw())
    random.seed(1); d_std = _counts(p_std, lambda: p_std.train_from_memory(m1, 2))
    random.seed(1); d_cql = _counts(p_cql, lambda: p_cql.train_from_memory(m2, 2))
    assert d_cql == d_std
    cql.set_cql(0.0)                                         # switched off between steps: the standard step again
    assert _counts(cql, lambda: cql.train(mb)) == c_std and cql.cql_alpha == 0.0


@pytest.mark.parametrize("kw,word", [(dict(double_dqn=True), "double_dqn"), (dict(munchausen=True), "munchausen"),
                                     (dict(advantage_learning=0.9), "advantage_learning"), (dict(bootstrap_heads=2), "bootstrap_heads"),
                                     (dict(quantiles=2), "quantiles"), (dict(dueling=True), "dueling"), (dict(noisy_nets=True), "noisy_nets"),
                                     (dict(batch_norm=True), "batch_norm"),
                                     (dict(double_dqn=True, datatype="float64", batch_size=8), "double_dqn"),
                                     (dict(munchausen=True, datatype="float64", batch_size=8), "munchausen")])
def test_library_refusals(sd, kw, word):
    from simple_dqn_amd import _lib
    net = sd.DeepQNetwork(2, make_args(**dict(dict(batch_size=32), **kw)))
    lib = sd.load()
    rc = lib.sdqn_net_set_cql(net._h, 1.0)
    msg = lib.sdqn_last_error().decode()
    assert rc == ERR_ARG and word in msg and "cql_alpha" in msg, msg
    for bad in (-0.1, float("nan"), float("inf")):
        assert lib.sdqn_net_set_cql(net._h, bad) == ERR_ARG, bad
    assert lib.sdqn_net_set_cql(net._h, 0.0) == 0            # off is nobody's business
    if word == "batch_norm":
        return                                               # (batch_norm is fixed at creation: one order only)
    # the other order: the option on a CQL net
    cql = sd.DeepQNetwork(4, make_args(batch_size=kw.get("batch_size", 32), datatype=kw.get("datatype", "float32"), cql_alpha=1.0))
    with pytest.raises(Exception) as ei:
        if word == "double_dqn":
            cql.set_option("double_dqn", 1)
        elif word == "munchausen":
            cql.set_munchausen(True)
        elif word == "advantage_learning":
            cql.set_advantage_learning(0.9)
        elif word == "bootstrap_heads":
            _lib.check(lib.sdqn_net_set_bootstrap(cql._h, 2, 1.0, 0))
        elif word == "quantiles":
            _lib.check(lib.sdqn_net_set_quantiles(cql._h, 2))
        elif word == "dueling":
            _lib.check(lib.sdqn_net_set_dueling(cql._h, 1))
        else:
            _lib.check(lib.sdqn_net_set_noisy(cql._h, 1, 0.5, 0))
    assert "cql_alpha" in str(ei.value), str(ei.value)
    import ctypes as C
    a = C.c_double()
    assert lib.sdqn_net_get_cql(cql._h, C.byref(a)) == 0 and a.value == 1.0
