"""Which kernel runs for a stage of the train step is resolve_route's answer (simple_dqn_amd/csrc/launch_route.h).  The whole table over the
default-options grid and every `bt` deviation is pinned in tests/golden/launch_routes.txt — it was generated once, after the launches of the
tree with the resolver had been compared record for record with those of the five-function chain it replaced (tools/route_trace.sh), so a
change that reroutes any configuration shows up here as a diff of readable lines.  The riding rules the old chain only implied are asserted
on top of it."""
import os
import re

import pytest

import route_emul as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "launch_routes.txt")
CHAINS = {"SS_CHAIN_NS1", "SS_CHAIN_NS2"} | {"SSH_CHAIN%s_NS%d%s" % (c, n, w) for c in ("", "_C1") for n in (1, 2) for w in ("", "_WB")}
C1_CHAINS = {f for f in CHAINS if "_C1_" in f}
DGRAD_CHAINS = {"SSH_DGRAD_CHAIN", "SSH_DGRAD_CHAIN_WB"}


def test_routes_match_the_pinned_table():
    got = list(R.table_lines())
    want = open(GOLDEN).read().splitlines()
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not diff, "%d of %d lines differ; first:\n- %s\n+ %s" % (len(diff), len(want), diff[0][1] if diff else "", diff[0][0] if diff else "")


def _walk():
    """(bt, variant, datatype, nz) of the default grid, the bt deviations and the riding conv1_wgrad variants"""
    opts = [(bt, 0) for _, bt, _ in R.deviations()] + [({}, 16), ({}, 48), ({R.K_BWD1: 1}, 16), ({"*": -1}, 16)]
    for bt, variant in opts:
        for _, h16, bn in R.DTYPES:
            for nz in (1, 2, 3):
                yield bt, variant, h16, bn, nz


def test_riding_rules():
    """A `none` route names a sibling that launches for the same key; conv3_fwd rides iff conv2_fwd is a chain; conv1_fwd rides only in
    float16 chains that compute conv1; conv2_dgrad rides iff conv3_dgrad is the dgrad chain; bwd1 rides only in the weight-gradient launch."""
    n_none = 0
    for bt, variant, h16, bn, nz in _walk():
        table = {kid: R.rows(kid, nz, h16, bn, bt=bt, variant=variant) for kid in R.IDS}
        for b in range(len(R.BS)):
            for i in range(8):
                at = {kid: table[kid][b][i] for kid in R.IDS}
                ctx = (bt, variant, h16, bn, nz, R.BS[b], i)
                for kid, (unit, form, rides_in) in at.items():
                    assert (unit == "none") == (form == "FORM_NONE") == (rides_in >= 0), ctx
                    if unit == "none":
                        n_none += 1
                        assert at[rides_in][0] != "none" and at[rides_in][1] != "FORM_INVALID", (ctx, kid)
                        assert (kid, rides_in) in ((R.K_CONV1_FWD, R.K_CONV2_FWD), (R.K_CONV3_FWD, R.K_CONV2_FWD), (R.K_CONV2_DGRAD, R.K_CONV3_DGRAD), (R.K_BWD1, R.K_WGRADS)), (ctx, kid)
                assert (at[R.K_CONV3_FWD][0] == "none") == (at[R.K_CONV2_FWD][1] in CHAINS), ctx
                assert (at[R.K_CONV1_FWD][0] == "none") == (at[R.K_CONV2_FWD][1] in C1_CHAINS), ctx
                assert at[R.K_CONV1_FWD][0] != "none" or h16, ctx
                assert (at[R.K_CONV2_DGRAD][0] == "none") == (at[R.K_CONV3_DGRAD][1] in DGRAD_CHAINS), ctx
                if at[R.K_BWD1][0] == "none":
                    assert h16 and R.BS[b] >= 128 and variant & 16, ctx
                    if h16 == 2:
                        assert at[R.K_WGRADS][1] in ("BT_WGRADS_C1W_LAST", "BT_WGRADS_C1W_FIRST"), ctx
    assert n_none > 1000


def test_five_step_configurations():
    """the rides the GPU test (test_gpu_launch_route.py) watches, at the smallest batch size where each switches"""
    silent = lambda B, h16: sorted(k for k in R.IDS if R.route(k, B, 2, h16, 0, ring=1, variant=16 if k in (18, 24) else 0)[0] == "none")
    assert silent(32, 0) == [] and silent(128, 0) == [2] and silent(160, 0) == []
    assert silent(32, 2) == [0, 2] and silent(128, 2) == [0, 2, 9, 18]


def test_resolver_reads_the_route_key_only():
    """launch_route.h is plain C++ that knows nothing of the kernel-argument struct: a route cannot depend on xcd_map or on any StepArgs
    field that route_key (kernels.h) does not copy, so the patched argument copies of the step orchestration all route alike."""
    code = re.sub(r"//[^\n]*", "", open(R.HEADER).read())
    assert "StepArgs" not in code and "xcd_map" not in code and "#include <hip" not in code and '#include "' not in code
    assert re.search(r"Route resolve_route\(int id, const RouteKey& k, const LaunchTune& t\)", code)
    fields = re.search(r"struct RouteKey \{(.*?)\};", code, re.S).group(1)
    assert sorted(re.findall(r"\b(\w+)[,;]", fields)) == sorted(["B", "nz", "h16", "bn", "f4w_count", "from_ring", "tps1", "has_src", "has_w1p", "has_host_idx"])
    kernels_h = open(os.path.join(os.path.dirname(R.HEADER), "kernels.h")).read()
    key = re.search(r"inline RouteKey route_key\(const StepArgs& a, const LaunchTune& t\) \{(.*?)\n\}", kernels_h, re.S).group(1)
    assert sorted(set(re.findall(r"\ba\.(\w+)", key))) == sorted(["B", "nz", "h16", "bn", "f4w_count", "from_ring", "tps1", "src", "w1p"])


def test_design_menu_table_is_the_resolvers():
    """DESIGN.md 12.6 prints what every `bt:<id>` entry means per id, regime and datatype: generated from the resolver, held to it here"""
    text = open(os.path.join(HERE, "..", "DESIGN.md")).read()
    block = text.split("<!-- launch-route-menu:begin -->\n")[1].split("\n<!-- launch-route-menu:end -->")[0]
    assert block.splitlines() == list(R.menu_table_lines())
