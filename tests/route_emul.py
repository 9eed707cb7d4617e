"""resolve_route (simple_dqn_amd/csrc/launch_route.h) from Python: tests/emul/route.cpp built with g++ on demand, like test_emul.py's library.
Shared by tests/test_launch_route.py (the pinned table and the riding rules) and tests/test_gpu_launch_route.py (a profiled step against it)."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "simple_dqn_amd", "csrc", "launch_route.h")
IDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 17, 18, 24)
BS = (1, 32, 33, 47, 48, 64, 127, 128, 160, 204, 205, 208, 256, 257, 512)      # 204 / 205 straddle the 80 % fill rule at nz = 2
DTYPES = (("f32", 0, 0), ("f32+bn", 0, 1), ("h16=1", 1, 0), ("h16=2", 2, 0))    # name, h16, bn
FLAGS = ("f4w", "ring", "hidx")             # the order route_rows walks them in: out[b][f4w][ring][hidx]
BT_VALUES = (-1, 1, 2, 3, 6, 7, 8)
K_CONV1_FWD, K_CONV2_FWD, K_CONV3_FWD, K_CONV3_DGRAD, K_CONV2_DGRAD, K_BWD1, K_WGRADS = 0, 1, 2, 7, 9, 18, 24
GROUPS = ((0, 1, 2), (7, 9), (18, 24))      # ids whose routes read one another's bt / nw entries (the chains)

_lib = None


def lib():
    global _lib
    if _lib is None:
        so, src = os.path.join(HERE, "emul", "libsdqn_route.so"), os.path.join(HERE, "emul", "route.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(HEADER)):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so, src])
        _lib = C.CDLL(so)
        _lib.route_unit.restype = _lib.route_form.restype = C.c_char_p
    return _lib


def rows(kid, nz, h16, bn, bt=None, nw=None, wt=0, variant=0, tps1=5, has_src=1, has_w1p=1, Bs=BS):
    """[(unit, form, rides_in)] names per B x f4w x ring x hidx: a list over Bs of 8-tuples in FLAGS order."""
    L = lib()
    kc = L.route_kernel_count()
    btv, nwv = [0] * kc, [0] * 12
    for k, v in (bt or {}).items():
        for i in (range(kc) if k == "*" else (k,)):
            btv[i] = v
    for k, v in (nw or {}).items():
        nwv[k] = v
    out = (C.c_int * (len(Bs) * 8 * 3))()
    L.route_rows(kid, (C.c_int * 6)(nz, h16, bn, tps1, has_src, has_w1p), (C.c_int * kc)(*btv), (C.c_int * 12)(*nwv), wt, variant, len(Bs), (C.c_int * len(Bs))(*Bs), out)
    names = {}

    def name(u, f, r):
        if (u, f, r) not in names:
            names[(u, f, r)] = (L.route_unit(u).decode(), L.route_form(f).decode(), r)
        return names[(u, f, r)]
    flat = [name(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(len(Bs) * 8)]
    return [tuple(flat[8 * b:8 * b + 8]) for b in range(len(Bs))]


def route(kid, B, nz, h16, bn, f4w=0, ring=0, hidx=0, **kw):
    return rows(kid, nz, h16, bn, Bs=(B,), **kw)[0][(f4w * 2 + ring) * 2 + hidx]


def reaches(j, kid):
    return kid == j or any(j in g and kid in g for g in GROUPS)


def deviations():
    """(label, bt dict, ids to walk): default options, then every bt entry off its default alone, then all entries alike."""
    yield "default", {}, IDS
    for v in BT_VALUES:
        for j in IDS:
            yield "bt[%d]=%d" % (j, v), {j: v}, tuple(i for i in IDS if reaches(j, i))
        yield "bt[*]=%d" % v, {"*": v}, IDS


def _cell(r8):
    """the 8 routes of one B: one name when no flag matters, else the flags that do and the routes in their order"""
    txt = ["%s/%s" % (u, f) if u != "none" else "none>%d" % r for u, f, r in r8]
    for keep in ((), (0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
        pick = {}
        ok = True
        for i in range(8):
            bits = ((i >> 2) & 1, (i >> 1) & 1, i & 1)
            if pick.setdefault(tuple(bits[k] for k in keep), txt[i]) != txt[i]:
                ok = False
                break
        if ok:
            return txt[0] if not keep else "%s(%s)" % (",".join(FLAGS[k] for k in keep), "|".join(pick[k] for k in sorted(pick)))
    raise AssertionError


def _content(kid, nz, h16, bn, bt):
    cells = [_cell(r8) for r8 in rows(kid, nz, h16, bn, bt=bt)]
    runs, b = [], 0
    while b < len(BS):
        e = b
        while e + 1 < len(BS) and cells[e + 1] == cells[b]:
            e += 1
        runs.append(("B%d" % BS[b] if e == b else "B%d-%d" % (BS[b], BS[e])) + " " + cells[b])
        b = e + 1
    return "; ".join(runs)


def table_lines():
    """the text of tests/golden/launch_routes.txt.  Every (options, id, datatype, nz, B, f4w, ring, hidx) of the grid is in it, folded: runs
    of batch sizes with one answer, flags only where they matter (_cell), (datatype, nz) combinations with one answer on one line, and under
    a `bt` deviation only what differs from the default-options answer of the same id — `as default` when nothing does."""
    combos = [(d, nz) for d in DTYPES for nz in (1, 2, 3)]
    default = {}
    for label, bt, ids in deviations():
        out = []
        for kid in ids:
            groups = {}
            for (dname, h16, bn), nz in combos:
                c = _content(kid, nz, h16, bn, bt)
                if label == "default":
                    default[kid, dname, nz] = c
                elif c == default[kid, dname, nz]:
                    continue
                groups.setdefault(c, {}).setdefault(dname, []).append(str(nz))
            for c, who in groups.items():
                names = [d if len(z) == 3 else "%s/nz%s" % (d, "+".join(z)) for d, z in who.items()]
                out.append("%s id=%d %s : %s" % (label, kid, ",".join(names), c))
        for line in out or ["%s : as default" % label]:
            yield line


MENU_IDS = ((0, "conv1_fwd"), (1, "conv2_fwd"), (2, "conv3_fwd"), (3, "fc4_fwd"), (5, "fc4_dgrad"), (6, "fc4_wgrad"), (7, "conv3_dgrad"), (8, "conv3_wgrad"),
            (9, "conv2_dgrad"), (10, "conv2_wgrad"), (11, "conv1_wgrad"), (16, "bwd3"), (17, "bwd2"), (18, "bwd1"), (24, "wgrads"))
MENU_BS = (32, 64, 160, 256)                # below / above float16's conv1 rule (B >= 48); throughput regime without / with the 80 % fill
MENU_ENTRIES = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8)


def menu_table_lines():
    """DESIGN.md 12.6's table: what `bt:<id>` = entry means per id, batch regime and datatype (both nets, ring step, every other option at its
    default; bwd3 with fc4_wgrad riding).  `=` repeats entry 0's answer; `none>n` rides in the launch of id n; a (id, datatype, B) without a row routes alike under every entry."""
    yield "| id | datatype | B | " + " | ".join("bt = %d" % e for e in MENU_ENTRIES) + " |"
    yield "|---|---|---|" + "---|" * len(MENU_ENTRIES)
    for kid, kname in MENU_IDS:
        for dname, h16 in (("float32", 0), ("float16", 2)):
            per_b = []
            for B in MENU_BS:
                cells = []
                for e in MENU_ENTRIES:
                    u, f, r = route(kid, B, 2, h16, 0, f4w=int(kid == 16), ring=1, bt={kid: e})
                    cells.append(f if u != "none" else "none>%d" % r)
                per_b.append(tuple(c if i == 1 or c != cells[1] else "=" for i, c in enumerate(cells)))
            b = 0
            while b < len(MENU_BS):
                e = b
                while e + 1 < len(MENU_BS) and per_b[e + 1] == per_b[b]:
                    e += 1
                if any(c != "=" for i, c in enumerate(per_b[b]) if i != 1):      # (rows where no entry changes the route are left out)
                    yield "| %d %s | %s | %s | %s |" % (kid, kname, dname, ", ".join(str(x) for x in MENU_BS[b:e + 1]), " | ".join(per_b[b]))
                b = e + 1
