"""Per-iteration wall time of the interior-point loop on the mixed-size generalized power cone workload
(problems.generalized_power_mix), through the two loops the package has for it, same process, same device, runs
alternating:

    host    ipm.solve over HipSystemBackend: level C for the KKT side, the cone operations between the solves on the host
            (numpy classes), so s, z and the steps cross the bus several times per iteration, and after every update
            the device's (grad, d, p, q, r) of each generalized power cone are read back (ipm.adopt_device_genpow)
    device  ipm_device.solve_device_genpow: the iterate resident in HBM, the cone operations through
            hipkkt_kkt_system_affine_ds_gp / _combined_ds_gp / _step_length_gp / _barrier_gp

An iteration is timed from one kkt_update! to the next (a host clock; every iteration ends in calls that synchronise:
the solves' status, alpha), so handle construction and the symbolic analysis are outside the window.  The first solve of
each kind is a warm-up and is discarded.  Prints one JSON line:

    host_ms / device_ms            median over the repeats of the median iteration of a solve
    host_spread / device_spread    (max - min) / median over the repeats
    host_iters / device_iters      iterations to SOLVED
    host_bytes_per_iter            what the host loop's level-C calls move per iteration, counted from the arrays they are
                                   given and return: kkt_update! sends s, z; each kkt_solve! sends the right-hand side and
                                   the variables and returns the step; genpow() returns five arrays
    device_bytes_per_iter          the scalars the device loop reads back (12 residual scalars, (dtau, dkappa) twice,
                                   alpha twice; + 2 per barrier evaluation under the dual strategy), 8 bytes each

Usage: python scripts/bench_genpow_loop.py [--copies 4] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuclarabel_amd import ipm, problems                              # noqa: E402
from cuclarabel_amd.ipm_device import solve_device_genpow             # noqa: E402


def run_host(pb):
    be = ipm.HipSystemBackend(pb.P, pb.A, pb.cones)
    stamps, moved = [], [0]
    upd, sol, gpw = be.system.update, be.system.solve, be.ks.genpow

    def update(s, z):
        stamps.append(time.perf_counter())
        moved[0] += 8 * (np.size(s) + np.size(z))
        return upd(s, z)

    def solve(rhs_x, rhs_s, rhs_z, rhs_tau, rhs_kappa, x, s, z, *a, **kw):
        moved[0] += 8 * sum(np.size(v) for v in (rhs_x, rhs_s, rhs_z, x, s, z)) + 8 * (np.size(x) + 2 * np.size(z))
        return sol(rhs_x, rhs_s, rhs_z, rhs_tau, rhs_kappa, x, s, z, *a, **kw)

    def genpow():
        out = gpw()
        moved[0] += 8 * sum(np.size(v) for cone in out for v in cone)
        return out

    be.system.update, be.system.solve, be.ks.genpow = update, solve, genpow
    r = ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, be)
    return r, np.diff(stamps), moved[0] / max(1, len(stamps))


def run_device(pb):
    import torch
    stamps = []

    def inspect(vecs, backend):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    r = solve_device_genpow(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=inspect)
    return r, np.diff(stamps), 8.0 * (12 + 2 * 2 + 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_genpow_loop: no GPU (a timing needs one)")
    pb = problems.generalized_power_mix(copies=args.copies)
    run_host(pb)
    run_device(pb)                                                     # warm-up: code objects, torch, the allocator
    th, td, res = [], [], {}
    for _ in range(args.repeats):
        for name, fn, acc in (("host", run_host, th), ("device", run_device, td)):
            r, dt, nbytes = fn(pb)
            if r.status != ipm.SOLVED:
                raise SystemExit(f"bench_genpow_loop: the {name} loop ended with {r.status}")
            acc.append(float(np.median(dt)) * 1e3)
            res[name + "_iters"], res[name + "_bytes_per_iter"], res[name + "_obj"] = r.iterations, nbytes, r.obj_val
    if not abs(res["host_obj"] - res["device_obj"]) <= 1e-6 * max(1.0, abs(res["host_obj"])):
        raise SystemExit(f"bench_genpow_loop: the two loops disagree: {res['host_obj']} / {res['device_obj']}")
    med = lambda v: float(np.median(v))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    res.update(workload=f"generalized_power_mix(copies={args.copies})", n=pb.n, m=pb.m, ncones=len(pb.cones), host_ms=med(th),
               device_ms=med(td), host_spread=spread(th), device_spread=spread(td), repeats=args.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
