"""The sweep plans of every knob environment, decided and asserted on the CPU.

csrc/schedule.cpp holds what the engine decides -- the launch schedule and how one sweep is split -- as host-only code.
tests/sanitize/host_driver.cpp --plans builds that schedule for a pattern with a fixed device (256 CUs, 240 resident
workgroups) and prints the "[hipkkt] sweep plan" / "[hipkkt] sweep launch" lines of HIPKKT_VERBOSE=2 exactly as the
engine prints them: for a claimed sweep (persistent and chained kernels allowed) with W pending and in the steady state,
then for the unclaimed sweeps of 1, 2 and 4 columns.  Here it runs over the forests of front_shapes.sweep_cases() under
every environment of test_gpu_sweep_paths.ENVS -- one child process per environment, the knobs read from the environment
by knobs.hpp as in the product -- and the lines are parsed with the GPU suite's own regexes.  What that suite asserts
about the PATH from a GPU child's stderr is asserted here without a GPU; the numbers stay with the GPU suite."""
import os
import subprocess

import numpy as np
import pytest

from tests import front_shapes as fs
from tests.test_gpu_sweep_paths import ENVS, TALL, _empty, _sweep_plans
from tests.test_host_sanitizers import CSRC, ROOT, SOURCES

CASES = fs.sweep_cases()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The plain g++ build of the driver (no sanitizers) and one pattern file per forest."""
    d = tmp_path_factory.mktemp("schedule")
    exe = str(d / "host_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "include")] + SOURCES + ["-o", exe])
    files = {}
    for name, (spec, *_rest) in CASES.items():
        K = fs.make_case(spec, 1).K.tocsc()
        path = str(d / (name + ".bin"))
        with open(path, "wb") as f:
            np.array([K.shape[0], K.nnz], dtype=np.int64).tofile(f)
            K.indptr.astype(np.int64).tofile(f)
            K.indices.astype(np.int64).tofile(f)
        files[name] = path
    return exe, files


_RUNS = {}


def plans(driver, env_id):
    """-> {case: dict(nl, claimed: plans, unclaimed: plans)} under ENVS[env_id]."""
    if env_id not in _RUNS:
        exe, files = driver
        env = {k: v for k, v in os.environ.items() if not k.startswith("HIPKKT_")}
        env.update(ENVS[env_id])
        r = subprocess.run([exe, "--plans"] + list(files.values()), env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        res = {}
        for name, chunk in zip(files, r.stdout.split("@@case ")[1:]):
            head, body = chunk.split("\n", 1)
            assert head.split()[0] == files[name], head
            claimed, unclaimed = body.split("@@claimed\n", 1)[1].split("@@unclaimed\n", 1)
            res[name] = dict(nl=int(head.split()[-1]), claimed=_sweep_plans(claimed), unclaimed=_sweep_plans(unclaimed))
        assert set(res) == set(CASES)
        _RUNS[env_id] = res
    return _RUNS[env_id]


@pytest.mark.parametrize("env_id", list(ENVS))
def test_plans_of_every_environment(driver, env_id):
    env = ENVS[env_id]
    bs128_f = 128                                          # knobs.hpp: HIPKKT_BS128_F
    for name, run in plans(driver, env_id).items():
        nl, tag = run["nl"], (env_id, name, run)
        assert [p["w_pending"] for p in run["claimed"]] == [True, False], tag
        assert run["unclaimed"] and run["unclaimed"][0]["nr"] == 1, tag
        for p in run["claimed"] + run["unclaimed"]:
            assert p["persistent"][1] == nl and p["per_level"][1] == p["chained"][0] and p["chained"][1] == p["persistent"][0], tag
            assert p["packed"] == (env.get("HIPKKT_PACKED") != "0"), tag
            assert len(p["launches"]) + sum(l["merged"] for l in p["launches"]) == p["per_level"][1], tag
        for p in run["unclaimed"]:                         # no token: no kernel that waits
            assert _empty(p["chained"]) and _empty(p["persistent"]) and p["kernel"] == "none", tag
        every = [l for p in run["claimed"] + run["unclaimed"] for l in p["launches"]]
        steady = run["claimed"][1]                         # _check_paths' steady[0]: a claimed sweep, W there
        level0 = [l for l in steady["launches"] if l["level"] == 0]
        if "HIPKKT_NO_TOP" in env:                         # with HIPKKT_CHAIN=0: per level to the root
            for p in run["claimed"]:
                assert _empty(p["chained"]) and _empty(p["persistent"]) and p["per_level"] == (0, nl) and p["kernel"] == "none", tag
                assert p["launches"], tag
            fam = [l for p in run["claimed"] for l in p["launches"]]
            if env_id == "unmerged":
                assert all(l["family"] != "level" and not l["merged"] for l in fam), tag
                if name in ("mixed_129", "merge_129"):     # more small fronts than ride along: two launches in level 0
                    assert {l["family"] for l in fam if l["level"] == 0} == {"block", "small"}, tag
            if env_id == "merge0" and name in ("mixed_few", "mixed_129", "merge_128", "tall_mixed"):
                l0 = level0                                # nothing rides along: one merged launch
                assert len(l0) == 1 and l0[0]["family"] == "level" and l0[0]["block"] > 0 and l0[0]["wave"] + l0[0]["tiny"] > 0, tag
            if env_id == "per_level" and name == "mixed_129":
                l0 = level0
                assert len(l0) == 1 and (l0[0]["family"], l0[0]["block"], l0[0]["wave"], l0[0]["tiny"]) == ("level", 2, 96, 33), tag
            if env_id == "per_level" and name.startswith("tiny_n"):
                l0 = level0
                assert len(l0) == 1 and (l0[0]["family"], l0[0]["tiny"]) == ("small", int(name[6:])), tag
        if "HIPKKT_CHAIN_TOP" in env:                      # chained to the root instead of the persistent kernel
            for p in run["claimed"]:
                assert _empty(p["persistent"]) and p["kernel"] == "none", tag
                if nl >= 2:
                    assert p["chained"][1] == nl and p["chained"][1] - p["chained"][0] >= 2, tag
        if env_id in ("default", "top_cap3", "top_512") and name in TALL:
            for p in run["claimed"]:                       # two chained launches under a persistent set of six fronts
                assert p["chained"] == (0, 2) and p["persistent"] == (2, 5) and p["kernel"] == "top", tag
                assert p["grid"] == (3 if env_id == "top_cap3" else 6), tag     # HIPKKT_TOP_CAP=3 shrinks the set's grid
                assert p["threads"] == (512 if env_id == "top_512" else 1024), tag
        if "HIPKKT_NO_LEVEL_MERGE" in env:
            assert all(l["family"] != "level" and not l["merged"] for l in every), tag
        for l in every:
            if l["family"] in ("block", "level"):
                assert l["solve_bs"] == (128 if "HIPKKT_BS128_COUNT" in env and l["fmax"] <= bs128_f else 256), (l, tag)

def test_environments_differ_where_they_should(driver):
    """The knobs reach the schedule: unmerged launches outnumber merged ones somewhere, and HIPKKT_MERGE_SMALL=0 leaves
    a level with both classes to one merged launch (which one: test_plans_of_every_environment)."""
    base, unmerged, merge0 = plans(driver, "per_level"), plans(driver, "unmerged"), plans(driver, "merge0")
    assert any(len(unmerged[n]["claimed"][1]["launches"]) > len(base[n]["claimed"][1]["launches"]) for n in CASES)
    assert any(l["family"] == "level" for n in CASES for l in base[n]["claimed"][1]["launches"])
    assert any(len([l for l in merge0[n]["claimed"][1]["launches"] if l["level"] == 0]) <
               len([l for l in unmerged[n]["claimed"][1]["launches"] if l["level"] == 0]) for n in CASES)
