"""Host side of the extend-add cases (tests/extend_add_shapes.py), on the CPU.

  * Structure: the symbolic phase (the host list driver of tests/test_pulled_leaf_lists_host.py, built with AddressSanitizer
    and UBSan) gives every case its designed parent, links and children on the chosen rows, the dense children, sliced
    fronts and pulled leaves the table says; the "[pieces]" lines of the host-only symbolic call (HIPKKT_DUMP_LEVELS) equal
    the counts the construction predicts from the chosen positions alone.
  * Edges: the wave slices (wcut) and the tiles' wave shares (tcut) hold exactly the intended 15 .. 129 items; the row slices'
    own lists hold the pieces of each kind the sliced case is for.
  * References: exact right-hand sides, an a-priori condition bound that holds, tolerances scipy's fp64 solve meets -- and
    that a factorisation with ONE extend-add fault at the entry only the case's edge reaches does not (a term dropped, an
    entry off by 1e-7, a stale update buffer)."""
import json
import os
import subprocess
import sys
from collections import Counter, defaultdict

import numpy as np
import pytest

from tests import extend_add_shapes as ea
from tests import front_shapes as fs
from tests import pulled_leaf_shapes as pls
from tests.test_host_sanitizers import CSRC, ROOT
from tests.test_pulled_leaf_lists_host import _check, _dump

CASES = ea.cases()
NAMES = ea.names()


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """name -> the list driver's dump under the case's own environment (one process per environment)."""
    d = tmp_path_factory.mktemp("extend_add")
    exe = str(d / "pulled_lists_driver")
    src = [os.path.join(ROOT, "tests", "sanitize", "pulled_lists_driver.cpp")] + [os.path.join(CSRC, f) for f in ("symbolic.cpp", "ordering.cpp", "schedule.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include")] + src + ["-o", exe])
    by_env = defaultdict(list)
    for name in NAMES:
        path = str(d / (name + ".bin"))
        pls.write_pattern(ea.case(name).K, path)
        by_env[tuple(sorted((CASES[name]["env"] if name in CASES else {}).items()))].append((name, path))
    out = {}
    for env, items in by_env.items():
        for (name, _), D in zip(items, _dump(exe, 2, [p for _, p in items], env=dict(env))):
            out[name] = D
        for (name, _), D in zip(items, _dump(exe, 2, [p for _, p in items], env=dict(env, HIPKKT_PULL_FACTOR_LEAVES="0"))):
            out[name, "stored"] = D
    return out


def _parent(D, d):
    """The designed parent (its first link) in a dump: the supernode of the expected shape that has the children."""
    nc = d["links"][0] if d["links"] else d["shape"]["rp"] + d["shape"]["k"]
    nb = d["shape"]["rp"] + d["shape"]["k"] + d["shape"]["sp_"] - nc
    hits = [s for s, S in D["S"].items() if (S["nc"], S["nb"]) == (nc, nb) and len(D["CH"][s]) == len(d["leaves"]) + len(d["children"])]
    assert len(hits) == 1, (nc, nb, {s: (S["nc"], S["nb"], len(D["CH"][s])) for s, S in D["S"].items() if S["nc"] > 8})
    return hits[0]


def _chain(D, s):
    """(widths, members) of the chain of dense children from supernode s upwards."""
    m = [s]
    while True:
        p = D["S"][s]["parent"]
        if p < 0 or D["S"][s]["nb"] != D["S"][p]["nc"] + D["S"][p]["nb"]:
            return tuple(D["S"][x]["nc"] for x in m), m
        m.append(p)
        s = p


# ------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize("name", list(CASES))
def test_symbolic_gives_the_designed_parent_links_and_children(dumps, name):
    d = CASES[name]
    for D in (dumps[name], dumps[name, "stored"]):
        p = _parent(D, d)
        k = d["shape"]["k"]
        # the children: on the chosen rows of P' (positions of P moved up by the poison columns), whatever their order
        want = Counter([(1, tuple(q + k for q in pos)) for pos in d["leaves"]] + [(nc, tuple(q + k for q in pos)) for nc, pos in d["children"]])
        got = Counter((D["S"][c]["nc"], tuple(D["REL"][c])) for c in D["CH"][p])
        assert got == want
        assert all(D["S"][c]["nc"] >= 2 for c in D["CH"][p]) or d["leaves"]
        # every child's first row is a column of the designed supernode; in a chain, of the link the case says
        links, members = _chain(D, p)
        top = members[-1]
        assert links == (d["links"] or (d["shape"]["rp"] + k,)), links
        if d["links"] and d["children"]:
            cum = np.cumsum((0,) + links)
            firsts = sorted(int(np.searchsorted(cum, D["REL"][c][0], side="right")) - 1 for c in D["CH"][p])
            assert firsts == [1, 1, len(links) - 1, len(links) - 1], firsts       # the second and the last link: two fronts each
        assert all(len(D["CH"][s]) == 1 for s in members[1:])                     # UNREACHABLE: a link above the first has ONE child
        if d["shape"]["sp_"]:
            g = D["S"][top]["parent"]
            assert g >= 0 and _chain(D, g)[0] == (d["glinks"] or tuple([d["shape"]["ng"] // ea._g_links(d["shape"]["ng"])] * ea._g_links(d["shape"]["ng"])))
        else:
            assert D["S"][top]["parent"] < 0
        assert bool(D["S"][p]["tile_base"] >= 0) == d["block"]
        n_sliced = sum(1 for s in members if D["S"][s]["sliced"])
        assert n_sliced == d["sliced"] and (n_sliced == 0 or D["S"][p]["sliced"]), n_sliced
    # the lists, checked independently of their builder (the pulled leaves' rule and terms, every other piece in the item
    # lists, dense children in neither), and the counts the table carries
    st = _check(dumps[name])
    assert (st["leaves"], st["terms"]) == d["pulled"], st
    assert st["dense"] == d["dense"], st
    st0 = _check(dumps[name, "stored"], 0, 0, knob=False)
    assert st0["dense"] == d["dense"]
    # the item lists of the parent, against the construction's counts (every child stored)
    D = dumps[name, "stored"]
    p = _parent(D, d)
    if d["block"]:
        tiles = [t for t, T in D["T"].items() if T["s"] == p]
        assert len([1 for v in D["I"] if v[0] == p]) == d["level1"][0] and sum(v[3] for v in D["I"] if v[0] == p) == d["level1"][1]
        assert len([1 for v in D["U"] if v[0] in tiles]) == d["level1"][2] and sum(v[3] for v in D["U"] if v[0] in tiles) == d["level1"][3]
    else:
        assert not [t for t, T in D["T"].items() if T["s"] == p]          # a one-wave parent has no tiles (k_front_wave walks the children)


def test_a_tiny_parent_keeps_its_wide_children(dumps):
    """REACHABLE_AFTER_ALL: the root (8, 0) keeps (25, 1), (26, 1) and (25, 1) -- and the neighbouring shapes merge, as the
    arithmetic says."""
    D = dumps["tiny_parent"]
    S = D["S"]
    assert sorted((v["nc"], v["nb"]) for v in S.values()) == [(8, 0), (25, 1), (25, 1), (26, 1)]
    root = [s for s, v in S.items() if v["nc"] == 8][0]
    assert len(D["CH"][root]) == 3 and sorted(D["REL"][c][0] for c in D["CH"][root]) == [0, 0, 5]
    assert fs.klass(8, 8) == "tiny"
    trap = lambda nc: nc * (nc + 1) / 2
    for n, stays in ((24, False), (25, True), (26, True), (27, False)):
        frac, allow = 7 * n / trap(n + 8), (1.0 if n + 8 <= 32 else 0.3)
        assert (frac > allow) == stays, (n, frac)


_SYM = r"""
import sys
sys.path.insert(0, {root!r})
from cuclarabel_amd import _lib
from tests import extend_add_shapes as ea
for name in {names!r}:
    print("@@case", name, file=sys.stderr, flush=True)
    _lib.symbolic_analyse(ea.case(name).K, ordering=_lib.ORDER_NATURAL)
"""


def _pieces_lines(names, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("HIPKKT_")}
    e.update(env, HIPKKT_DUMP_LEVELS="1")
    r = subprocess.run([sys.executable, "-c", _SYM.format(root=ROOT, names=list(names))], env=e, cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    chunks = r.stderr.split("@@case ")[1:]
    assert len(chunks) == len(names)
    return {c.split("\n", 1)[0].strip(): ea.parse_pieces(c) for c in chunks}


def test_pieces_lines_equal_the_constructions_counts():
    """HIPKKT_DUMP_LEVELS through the host-only symbolic call.  With every child stored the parents' level (level 1: the
    children are leaves) shows exactly the predicted pieces, entries and length classes; with the default knobs the pulled
    leaves take their share out of the lists and the total stays."""
    plain = [n for n in CASES if not CASES[n]["env"]]
    for env_names, env in ((plain, {}), ([n for n in CASES if CASES[n]["env"]], {"HIPKKT_PANEL_CAP": "3000"})):
        stored = _pieces_lines(env_names, dict(env, HIPKKT_PULL_FACTOR_LEAVES="0"))
        default = _pieces_lines(env_names, env)
        for name in env_names:
            d = CASES[name]
            lv, pulled = stored[name]
            assert pulled == (0, 0)
            if d["block"] and any(d["level1"][:4]):
                assert lv[1]["listed"] == d["level1"], (name, lv[1], d["level1"])
                assert lv[1]["out"] == (0, 0, 0)
            else:
                assert 1 not in lv, (name, lv)
            lv, pulled = default[name]
            assert pulled == d["pulled"], (name, pulled)
            if d["block"] and any(d["level1"][:4]):
                got = lv[1]
                assert got["listed"][0] + got["out"][1] == d["level1"][0] and got["listed"][2] + got["out"][0] == d["level1"][2], (name, got)
                assert got["listed"][1] + got["listed"][3] + got["out"][2] == d["level1"][1] + d["level1"][3], (name, got)
                assert got["out"][2] == d["pulled"][1]


# ------------------------------------------------------------------------------------------------ the edges in the lists
def _ranges(cuts, per):
    """Sizes of the ranges a wave walks when it owns `per` consecutive slices."""
    return [cuts[min(len(cuts) - 1, w + per)] - cuts[w] for w in range(0, len(cuts) - 1, per)]


@pytest.mark.parametrize("n", ea.COUNTS)
def test_a_wave_slice_of_the_panel_holds_the_intended_items(dumps, n):
    """n children on two panel columns: two of the 16 wave slices hold n one-piece items each, for a kernel of 16, 8 and 4
    waves alike (a wave of a narrower kernel walks 16 / NW consecutive slices): the 16-in-flight edge at 15 | 16 | 17, the
    64-descriptor round at 63 | 64 | 65 (the caller's first round serves the first 64 only), a third round at 129."""
    d = CASES[f"panel_n{n}"]
    for key in (f"panel_n{n}", (f"panel_n{n}", "stored")):
        D = dumps[key]
        p = _parent(D, d)
        (wc,) = [v for v in D["WC"] if v[0] == p]
        base, cuts = wc[1], wc[2:]
        items = [v for v in D["I"] if v[0] == p]
        assert cuts[0] == base and cuts[16] - base == len(items) == 2 * n
        for per in (1, 2, 4):
            assert sorted(x for x in _ranges(cuts, per) if x) == [n, n], (per, cuts)
        for w in range(16):                                  # a slice holds whole columns: one target column each here
            cols = {items[i - base][1] for i in range(cuts[w], cuts[w + 1])}
            assert len(cols) <= 1 and cols <= {3 + 8, 9 + 8}
        assert all(v[3] == (2 if v[1] == 11 else 1) for v in items)


@pytest.mark.parametrize("name", ea.names("tile_rounds"))
def test_a_waves_share_of_a_tile_holds_the_intended_sub_items(dumps, name):
    """n children on U rows 0, 63 and 64 .. 127: in the diagonal tile (0, 0) and the off-diagonal tile (1, 0) two of the four
    wave shares hold n sub-items each, in qcol 0 and qcol 63, of cnt 2 (1 in the _b cases) and 1, and of cnt 64; the diagonal
    tile (1, 1) holds n pieces of cnt 64 - q in every column q, 16 n to a share."""
    d = CASES[name]
    n, b = len(d["children"]), name.endswith("_b")
    for key in (name, (name, "stored")):
        D = dumps[key]
        p = _parent(D, d)
        tiles = {(T["ti"], T["tj"]): t for t, T in D["T"].items() if T["s"] == p}
        assert sorted(tiles) == [(0, 0), (1, 0), (1, 1)]
        for (ti, tj), t in tiles.items():
            (tc,) = [v for v in D["TC"] if v[0] == t]
            base, cuts = tc[1], tc[2:]
            subs = [v for v in D["U"] if v[0] == t]                    # (t, qcol, relstart, cnt)
            assert cuts[0] == base and cuts[4] - base == len(subs)
            shares = [[subs[i - base] for i in range(cuts[w], cuts[w + 1])] for w in range(4)]
            sig = sorted((len(s), s[0][1], s[0][3]) for s in shares if s)
            if (ti, tj) == (0, 0):
                assert sig == ([(n, 0, 1)] if b else [(n, 0, 2), (n, 63, 1)]), sig
            elif (ti, tj) == (1, 0):
                assert sig == ([(n, 0, 64)] if b else [(n, 0, 64), (n, 63, 64)]), sig
            else:
                assert [len(s) for s in shares] == [16 * n] * 4
                assert [v[3] for v in shares[0][:n]] == [64] * n and (shares[3][-1][1], shares[3][-1][3]) == (63, 1)
            for s in shares:
                assert [v[1] for v in s] == sorted(v[1] for v in s)        # grouped by tile column, children in order within


def test_piece_lengths_and_starts_reach_their_edges(dumps):
    for nbc in (63, 64, 65, 128, 129):
        d = CASES[f"len_{nbc}"]
        D = dumps[f"len_{nbc}"]
        p = _parent(D, d)
        pnc = D["S"][p]["nc"]
        (c,) = D["CH"][p]
        rel = D["REL"][c]
        assert len(rel) == nbc and rel[0] == 13 and rel != list(range(rel[0], rel[0] + nbc))             # tcol > 0, gaps
        assert {pnc - 2, pnc - 1, pnc, pnc + 1} <= set(rel)                                              # panel | update rows
        u = [r - pnc for r in rel if r >= pnc]
        assert {62, 63, 66} <= set(u) and not {64, 65} & set(u)                                          # U rows 63 | 64, a gap
        items = [v for v in D["I"] if v[0] == p]
        assert all(v[1] > 0 for v in items)
        assert sorted((v[3] for v in items if v[1] == 13), reverse=True) == [64] * (nbc // 64) + ([nbc % 64] if nbc % 64 else [])
        # a sub-item of tile row 1 starts at row 2 of its tile, so the lane -> row map is not the identity there
        flat = {D["relbase"][c] + i: r for i, r in enumerate(rel)}
        t10 = [t for t, T in D["T"].items() if T["s"] == p and (T["ti"], T["tj"]) == (1, 0)][0]
        assert {(flat[v[2]] - pnc) & 63 for v in D["U"] if v[0] == t10} == {2}
    d, D = CASES["len_tail"], dumps["len_tail"]
    p = _parent(D, d)
    tiles = {(T["ti"], T["tj"]): t for t, T in D["T"].items() if T["s"] == p}
    n = Counter(v[0] for v in D["U"])
    assert n[tiles[(0, 0)]] == 0 and n[tiles[(1, 0)]] == 0 and n[tiles[(1, 1)]] == d["level1"][2] > 0


def test_the_row_slices_lists_hold_pieces_of_every_kind(dumps):
    """sliced_kinds under HIPKKT_PANEL_CAP=3000: three slices of 43, 43 and 42 update rows; every slice's own list holds the
    pieces that reach its rows or the top block, and each kind of piece the case is for exists."""
    d, D = CASES["sliced_kinds"], dumps["sliced_kinds"]
    p = _parent(D, d)
    pnc, nb = D["S"][p]["nc"], D["S"][p]["nb"]
    sl = [v for v in D["SL"] if v[1] == p]
    assert [v[2:4] for v in sl] == [[0, 3], [1, 3], [2, 3]]
    rsmax = -(-nb // 3)
    assert rsmax == 43
    flat = {}
    for c in D["CH"][p]:
        for i, r in enumerate(D["REL"][c]):
            flat[D["relbase"][c] + i] = r
    items = [(v[1], v[2], v[3], flat[v[2]], flat[v[2] + v[3] - 1]) for v in D["I"] if v[0] == p]      # tcol, relstart, cnt, rfirst, rlast
    kinds = Counter()
    for v in sl:
        q, s_i = v[0], v[2]
        lo, hi = pnc + s_i * rsmax, min(pnc + (s_i + 1) * rsmax, pnc + nb)
        want = [it for it in items if it[3] < pnc or not (it[4] < lo or it[3] >= hi)]
        got = [tuple(j[1:]) for j in D["J"] if j[0] == q]
        assert got == want, (s_i, len(got), len(want))
        assert v[4 + 16] - v[4] == len(got)
        for it in want:
            if it[4] < pnc:
                kinds["top block only"] += 1
            elif it[3] < pnc:
                kinds["across the top-block boundary"] += 1
            elif lo <= it[3] and it[4] < hi:
                kinds["inside one slice"] += 1
            else:
                kinds["across a slice boundary"] += 1
        kinds["outside this slice"] += len(items) - len(want)
    assert all(kinds[k] > 0 for k in ("top block only", "across the top-block boundary", "inside one slice", "across a slice boundary",
                                      "outside this slice")), kinds
    # the faulted entry is the first row of slice 2, reached by a piece that crosses 85 | 86
    assert d["fault"][1] - d["shape"]["rp"] == 2 * rsmax


def test_one_wave_parents_have_the_children_at_the_kernels_edges(dumps):
    """k_front_wave: a child of 10 rows takes the one-round path (55 entries <= 64 lanes), one of 11 the column loop; the
    children's headers are read 64 at a time: 64 and 65 children."""
    for nbc in (10, 11):
        d, D = CASES[f"wave_nbc{nbc}"], dumps[f"wave_nbc{nbc}"]
        p = _parent(D, d)
        (c,) = D["CH"][p]
        assert D["S"][c]["nb"] == nbc and nbc * (nbc + 1) // 2 == (55 if nbc == 10 else 66) and D["S"][p]["tile_base"] < 0
        assert fs.klass(D["S"][p]["nc"] + D["S"][p]["nb"], D["S"][p]["nc"]) == "wave"
    for n in (64, 65):
        d, D = CASES[f"wave_kids{n}"], dumps[f"wave_kids{n}"]
        assert len(D["CH"][_parent(D, d)]) == n


# ------------------------------------------------------------------------------------------------ references and faults
@pytest.mark.parametrize("name", NAMES)
def test_references_are_exact_calibrated_and_discriminating(name):
    c = ea.case(name)
    # b = K~ x_true was rounded once from long double
    r = fs.symmetric_matvec_ld(c.Kt, c.x_true)
    assert np.abs(r - np.asarray(c.b, np.longdouble)).max() <= fs.U * np.abs(r).max()
    # the a-priori condition bound holds
    assert np.linalg.cond(fs.full(c.Kt).toarray()) <= c.cond_bound * (1 + 1e-12)
    # scipy's fp64 solve meets the tolerances the GPU must meet
    x = fs.reference_solve(c)
    fwd, bwd = fs.errors(c, x)
    assert fwd <= 100 * c.cond_bound * fs.U and bwd <= fs.BWD_BOUND, (fwd, bwd, c.cond_bound)
    tol = fs.forward_bound(c, fwd)
    # discrimination: ONE extend-add fault at the entry only this case's edge reaches is over both bounds of the GPU test
    xe = fs.reference_solve(c, K=ea.faulted(name, c))
    fe, be = fs.errors(c, xe)
    print(f"\n[extend-add fault] {name:14s} fault {(CASES[name]['fault'] if name in CASES else ('drop',))[0]:6s} forward {fe:.2e} "
          f"(bound {tol:.2e}, x{fe / tol:.0f}) backward {be:.2e} (x{be / fs.BWD_BOUND:.0f})")
    assert fe > tol, (fe, tol)
    assert be > fs.BWD_BOUND, be


def test_the_table_covers_every_group_and_edge():
    groups = Counter(d["group"] for d in CASES.values())
    assert set(groups) == set(ea.GROUPS)
    assert {len(d["children"]) for d in CASES.values() if d["group"] == "panel_rounds"} == set(ea.COUNTS)
    assert {len(d["children"]) for n, d in CASES.items() if d["group"] == "tile_rounds" and not n.endswith("_b")} == set(ea.COUNTS)
    assert sorted(len(d["links"]) for d in CASES.values() if d["links"]) == [3, 3, 3, 5, 5, 5]
    assert {bool(d["shape"]["sp_"]) for d in CASES.values() if d["links"]} == {True, False}
    assert len(CASES["many_33"]["children"]) == 33 and {nc for nc, _ in CASES["many_33"]["children"]} == {2, 3, 5}
    assert all(nc >= 2 for d in CASES.values() for nc, _ in d["children"])
