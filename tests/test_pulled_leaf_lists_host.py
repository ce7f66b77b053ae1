"""The pulled leaves' term lists of the factorisation (csrc/schedule.cpp: build_factor_lists), checked on the CPU.

tests/sanitize/pulled_lists_driver.cpp (host code only, built here with AddressSanitizer and UBSan) dumps the lists of a
pattern: the reduced cfg2 in its nested-dissection order and the trees of tests/pulled_leaf_shapes.py in their natural
order.  Checked, independently of the builder:
  * which fronts are pulled: one column, no children, a parent, in a one-wave launch, the parent a block-class front that
    is not cut into row slices -- and nothing else;
  * every entry (leaf, a >= b) of a pulled leaf is exactly one term, with the target rel[] gives it, in the chunk range of
    the wave that owns its target column;
  * in a chunk the terms of one target are neighbours (so the lanes that add -- the last of each run -- have distinct
    targets), lane 0 holds a term and the doubling steps that cover the longest run; a target's terms follow the
    parent's child order through the whole list;
  * nothing of a pulled leaf is left in the item / sub-item lists, and everything of the other children still is;
  * HIPKKT_PULL_FACTOR_LEAVES=0: no leaf, no term; a sliced parent (HIPKKT_PANEL_CAP) pulls nothing."""
import os
import subprocess
from collections import defaultdict

import numpy as np
import pytest

from tests import pulled_leaf_shapes as pls
from tests.test_host_sanitizers import CSRC, ROOT

SHAPES = pls.cases()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("pulled")
    exe = str(d / "pulled_lists_driver")
    src = [os.path.join(ROOT, "tests", "sanitize", "pulled_lists_driver.cpp")] + [os.path.join(CSRC, f) for f in ("symbolic.cpp", "ordering.cpp", "schedule.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, "-I", os.path.join(ROOT, "include")] + src + ["-o", exe])
    files = {}
    for name in SHAPES:
        files[name] = str(d / (name + ".bin"))
        pls.write_pattern(pls.case(name).K, files[name])
    return exe, files, d


def _dump(exe, ordering, paths, env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("HIPKKT_")}
    e.update(env or {})
    r = subprocess.run([exe, str(ordering)] + list(paths), env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    out = []
    for chunk in r.stdout.split("@@case ")[1:]:
        head, body = chunk.split("\n", 1)
        D = dict(S={}, REL={}, relbase={}, CH={}, W={}, T={}, I=[], U=[], P=[], WC=[], TC=[], SL=[], J=[], nchunks=int(head.split()[-1]))
        for line in body.splitlines():
            k, *v = line.split()
            v = list(map(int, v))
            if k == "S":
                D["S"][v[0]] = dict(zip(("c0", "nc", "nb", "parent", "pulled", "tile_base", "small", "sliced", "front_off"), v[1:]))
            elif k == "REL":
                D["relbase"][v[0]], D["REL"][v[0]] = v[1], v[2:]
            elif k == "CH":
                D["CH"][v[0]] = v[1:]
            elif k == "W":
                D["W"][v[0]] = dict(spw=v[1], wcol=v[2:19], pwcut=v[19:36])
            elif k == "T":
                D["T"][v[0]] = dict(s=v[1], ti=v[2], tj=v[3], tcol=v[4:9], ptcut=v[9:14])
            else:
                D[k].append(v)
        out.append(D)
    return out


def _check(D, expect_leaves=None, expect_terms=None, knob=True):
    S, REL = D["S"], D["REL"]
    # ---- the rule
    want = {s for s, d in S.items() if knob and d["nc"] == 1 and not D["CH"][s] and d["parent"] >= 0 and d["small"] and 1 <= d["nb"] <= 63
            and S[d["parent"]]["tile_base"] >= 0 and not S[d["parent"]]["sliced"]}
    got = {s for s, d in S.items() if d["pulled"]}
    assert got == want
    for s in got:                                          # never under a one-wave or a sliced parent
        assert S[S[s]["parent"]]["tile_base"] >= 0 and not S[S[s]["parent"]]["sliced"]
    if expect_leaves is not None:
        assert len(got) == expect_leaves, (len(got), expect_leaves)
    # ---- the expected terms: (leaf_off, a, b) -> (chunk range of the owning wave, target)
    tiles_of = {(t["s"], t["ti"], t["tj"]): (k, t) for k, t in D["T"].items()}
    leaf_at = {S[s]["front_off"]: s for s in got}
    exp = {}
    for c in got:
        p = S[c]["parent"]
        pnc, fp, rel = S[p]["nc"], S[p]["nc"] + S[p]["nb"], REL[c]
        assert rel == sorted(rel)
        for b in range(len(rel)):
            for a in range(b, len(rel)):
                ra, rb = rel[a], rel[b]
                if rb < pnc:
                    W = D["W"][p]
                    w = max(x for x in range(16) if W["wcol"][x] <= rb)
                    assert W["wcol"][w] <= rb < W["wcol"][w + 1]
                    g = w - w % W["spw"]
                    rng, target = (W["pwcut"][g], W["pwcut"][g + W["spw"]]), ra + (rb * (2 * fp - 1 - rb)) // 2
                else:
                    i, j = ra - pnc, rb - pnc
                    k, t = tiles_of[(p, i >> 6, j >> 6)]
                    w = max(x for x in range(4) if t["tcol"][x] <= (j & 63))
                    assert t["tcol"][w] <= (j & 63) < t["tcol"][w + 1]
                    rng, target = (t["ptcut"][w], t["ptcut"][w + 1]), (j & 63) * 65 + (i & 63)
                exp[(S[c]["front_off"], a, b)] = (rng, target)
    if expect_terms is not None:
        assert len(exp) == expect_terms
    seen = set()
    chunks = defaultdict(list)
    for chunk, lane, off, target, a, b, steps in D["P"]:
        key = (off, a, b)
        assert key in exp and key not in seen, key        # a term of a pulled leaf, once
        seen.add(key)
        (c0, c1), tg = exp[key]
        assert c0 <= chunk < c1 and target == tg, (key, chunk, (c0, c1), target, tg)
        assert steps == 0 or lane == 0
        chunks[chunk].append((lane, target, off, steps))
    assert seen == set(exp)
    assert all(0 <= c < D["nchunks"] for c in chunks)
    # ---- runs inside a chunk; child order per target through the list
    order = {}
    for p, ch in D["CH"].items():
        for i, c in enumerate(ch):
            order[c] = i
    last_child = {}
    for chunk in sorted(chunks):
        terms = sorted(chunks[chunk])
        assert [l for l, *_ in terms] == list(range(len(terms)))          # packed from lane 0, no holes
        runs, longest, run = [], 1, 1
        for q, (lane, target, off, _) in enumerate(terms):
            if q and terms[q - 1][1] == target:
                run += 1
            else:
                runs.append(target)
                run = 1
            longest = max(longest, run)
            key = (chunk_owner(D, chunk)[:2], target)      # (a target belongs to one front or tile)
            ci = order[leaf_at[off]]
            assert ci > last_child.get(key, -1), "a target's terms out of child order"
            last_child[key] = ci
        assert len(runs) == len(set(runs)), "two runs of one target in a chunk: two lanes would add to one address"
        assert (1 << terms[0][3]) >= longest, (terms[0][3], longest)
    # ---- the item / sub-item lists: the other children's pieces, all of them and only them
    child_of_row = {}
    for s in S:
        for q in range(D["relbase"][s], D["relbase"][s] + S[s]["nb"]):
            child_of_row[q] = s
    items = defaultdict(int)
    for s, tcol, relstart, cnt in D["I"]:
        c = child_of_row[relstart]
        assert c not in got and S[c]["parent"] == s
        items[c] += cnt
    subs = defaultdict(int)
    for t, qcol, relstart, cnt in D["U"]:
        c = child_of_row[relstart]
        assert c not in got and S[c]["parent"] == D["T"][t]["s"]
        subs[c] += cnt
    dense = 0
    for c, d in S.items():
        p = d["parent"]
        if p < 0 or S[p]["tile_base"] < 0 or c in got:
            continue
        pnc, rel = S[p]["nc"], REL[c]
        if len(rel) == S[p]["nc"] + S[p]["nb"] and rel == list(range(len(rel))):
            dense += 1                                     # (a dense child is in neither list)
            continue
        n_panel = sum(len(rel) - b for b in range(len(rel)) if rel[b] < pnc)
        n_upd = sum(len(rel) - b for b in range(len(rel)) if rel[b] >= pnc)
        assert items[c] == n_panel and subs[c] == n_upd, (c, items[c], n_panel, subs[c], n_upd)
    return dict(leaves=len(got), terms=len(exp), chunks=len(chunks), dense=dense, fullest=max([len(v) for v in chunks.values()] + [0]))


_OWNERS = {}


def chunk_owner(D, chunk):
    """The (front, slice) or (tile, wave) whose range holds the chunk."""
    key = id(D)
    if key not in _OWNERS:
        o = {}
        for s, W in D["W"].items():
            for w in range(16):
                for c in range(W["pwcut"][w], W["pwcut"][w + 1]):
                    assert c not in o
                    o[c] = ("front", s, w)
        for t, T in D["T"].items():
            for w in range(4):
                for c in range(T["ptcut"][w], T["ptcut"][w + 1]):
                    assert c not in o
                    o[c] = ("tile", t, w)
        _OWNERS.clear()
        _OWNERS[key] = o
    return _OWNERS[key][chunk]


def test_lists_of_the_designed_trees(driver):
    exe, files, _ = driver
    for (name, (_, _, leaves, terms, block)), D in zip(SHAPES.items(), _dump(exe, 2, files.values())):
        st = _check(D, leaves, terms)
        print(name, st)
        if name == "mixed":
            assert st["dense"] >= 1
        if name.startswith("stack_"):                      # a wave with more than 64 terms, in full chunks
            assert st["fullest"] == 64 and st["chunks"] <= -(-terms // 64) + 2      # (two panel columns: two waves)


def test_lists_of_the_reduced_cfg2(driver):
    from cuclarabel_amd import problems
    from tests.oracle_bindings import make_oracle
    exe, _, d = driver
    pb = problems.config2(n=3000)
    o = make_oracle(pb, perm=np.arange(pb.n + pb.m + 2 * sum(1 for c in pb.cones if c.kind == 2 and c.dim > 4)))
    path = str(d / "cfg2_n3000.bin")
    pls.write_pattern(o.K(), path)
    st = _check(_dump(exe, 1, [path])[0])
    print("cfg2 n=3000", st)
    assert st["leaves"] > 100 and st["terms"] > st["leaves"]


def test_knob_off_and_sliced_parents_pull_nothing(driver):
    exe, files, _ = driver
    for D in _dump(exe, 2, [files["heights"], files["stack_70"]], env={"HIPKKT_PULL_FACTOR_LEAVES": "0"}):
        assert _check(D, 0, 0, knob=False)["chunks"] == 0 and not any(d["pulled"] for d in D["S"].values())
    # HIPKKT_PANEL_CAP 3000: P' = (48, 60) has a trapezoid of 4056 doubles and is cut into row slices
    D = _dump(exe, 2, [files["heights"]], env={"HIPKKT_PANEL_CAP": "3000"})[0]
    par = {d["parent"] for d in D["S"].values() if d["nc"] == 1 and d["parent"] >= 0 and d["small"]}
    assert any(D["S"][p]["sliced"] for p in par), "no sliced parent: the case does not test what it says"
    st = _check(D)
    assert all(not d["pulled"] for s, d in D["S"].items() if d["parent"] >= 0 and D["S"][d["parent"]]["sliced"])
