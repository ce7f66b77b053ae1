"""PSD cones of side 49 ... 96 on the device (hipkkt_kkt_enable_large_psd): two measurements, one JSON line.

  scaling   For cone lists of `--counts` cones of each side in `--sides` (P = I_2, A = ones): one
            hipkkt_kkt_update_from_sz_dev, the profile's update_ms of it (NT scaling of every cone, the Hs launch, the
            value scatter) and its factor_ms; and hs_ms, what the update costs from a GIVEN scaling, measured as
            hipkkt_kkt_system_update_scaling from the device's own (w, eta, lambda, R, Rinv) -- A = R R' and the
            many-workgroup Hs launch and the value scatter, no SVD -- by the same profile slot.  The Hs launch by itself
            is read from a kernel trace, for which --trace-list COUNTxSIDE runs six updates of one list and nothing
            else:  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_large_psd.py --trace-list 8x96
            (k_psd_hs_big and k_cone_psd_big in DIR's kernel_stats.csv).  A list whose Hs blocks exceed --max-hs
            entries is skipped and named in "skipped" (64 cones of side 96 are 5.5 GB of Hs and as much again in K).
  loop      sdp_large_cones(sides = --loop-sides, n = --n): per-iteration wall time of ipm_device.solve_device against the
            only route such a problem has without the opt-in: ipm.solve with the host's numpy cone objects over level B
            (hipkkt_kkt_update_cones), which forms the Hs blocks on the host and ships them every iteration.  Runs
            alternate; the host route is cut after --host-iters iterations (its per-iteration time does not depend on
            how far the iterate has come).  hs_bytes_per_iter: what that route sends per update.

Medians over --repeats with (max - min) / median as the spread.
Usage: python scripts/bench_large_psd.py [--counts 1,8,64] [--sides 64,96] [--n 2000] [--repeats 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuclarabel_amd import ipm, problems                              # noqa: E402
from cuclarabel_amd.cones import PSDTriangleConeT                     # noqa: E402
from cuclarabel_amd.ipm_device import solve_device                    # noqa: E402
from cuclarabel_amd.kktsolver import HipKKTSolver, HipKKTSystem       # noqa: E402

med = lambda v: float(np.median(v))
spread = lambda v: float((max(v) - min(v)) / np.median(v)) if np.median(v) > 0 else 0.0


def _delta(ks, before, key):
    return float(ks.profile()[key]) - before[key]


def bench_scaling(count, side, repeats, feed_back=True):
    import torch
    cones = [PSDTriangleConeT(side) for _ in range(count)]
    m = sum(c.numel for c in cones)
    pt = problems.interior_point(cones, np.random.default_rng(side * 1000 + count))
    ks = HipKKTSolver(sp.identity(2, format="csc"), sp.csc_matrix(np.ones((m, 2))), cones, large_psd=True)
    system = HipKKTSystem(ks)
    system.init(np.zeros(2), np.zeros(m))
    ks.profile_enable(True)
    d = torch.from_numpy(pt).to("cuda")
    torch.cuda.synchronize()
    upd, fac, hs = [], [], []
    for rep in range(repeats + 1):
        p0 = ks.profile()
        assert ks.kktsolver_update_from_sz_dev(d.data_ptr(), d.data_ptr())
        u, f = _delta(ks, p0, "update_ms"), _delta(ks, p0, "factor_ms")
        if not feed_back:
            continue
        lam, psd = ks.scaling()
        w, eta = ks.scaling_w()
        R = np.concatenate([t[0].ravel(order="F") for t in psd])
        Ri = np.concatenate([t[1].ravel(order="F") for t in psd])
        p0 = ks.profile()
        assert system.update_scaling(w, eta, lam, R, Ri)
        h = _delta(ks, p0, "update_ms")
        if rep:                                                        # (the first round is a warm-up)
            upd.append(u), fac.append(f), hs.append(h)
    if not feed_back:
        return None
    return dict(count=count, side=side, hs_entries=ks.info["nHs"], update_ms=med(upd), update_spread=spread(upd),
                hs_ms=med(hs), hs_spread=spread(hs), factor_ms=med(fac))


class LevelBHostCones(ipm.HipBackend):
    """level B with the caller's scaling: numpy cone objects form Hs, hipkkt_kkt_update_cones receives it"""

    def __init__(self, P, A, specs):
        super().__init__(P, A, specs)
        self.host = ipm._make_cones(specs)
        self.stamps, self.bytes = [], 0

    def update(self, s, z, mu=None, strategy=None):
        self.stamps.append(time.perf_counter())
        for c in self.host:
            if c.n and not c.update_scaling(s[c.rng].copy(), z[c.rng].copy()):
                return False
        Hs, u, v, e2 = ipm.host_cone_data(self.host)[:4]
        self.bytes = 8 * (Hs.size + u.size + v.size + e2.size)
        return self.ks.kktsolver_update(Hs, u, v, e2)


def run_host(pb, iters):
    be = LevelBHostCones(pb.P, pb.A, pb.cones)
    st = ipm.IPMSettings()
    st.max_iter = iters
    ipm.solve(pb.P, pb.q, pb.A, pb.b, pb.cones, be, settings=st)
    return np.diff(be.stamps), be.bytes


def run_device(pb):
    import torch
    stamps = []

    def inspect(vecs, backend):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    r = solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, inspect=inspect)
    if r.status != ipm.SOLVED:
        raise SystemExit(f"bench_large_psd: the device loop ended with {r.status}")
    return np.diff(stamps), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,8,64")
    ap.add_argument("--sides", default="64,96")
    ap.add_argument("--max-hs", type=float, default=2e8)
    ap.add_argument("--loop-sides", default="64,64,64,64")
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--host-iters", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--trace-list", default=None, help="COUNTxSIDE: six updates of that list only, for a kernel trace")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_large_psd: no GPU (a timing needs one)")
    if args.trace_list:
        count, side = (int(t) for t in args.trace_list.split("x"))
        bench_scaling(count, side, 5, feed_back=False)
        return
    res = dict(scaling=[], skipped=[], repeats=args.repeats)
    for side in (int(t) for t in args.sides.split(",")):
        for count in (int(t) for t in args.counts.split(",")):
            t = side * (side + 1) // 2
            if count * t * (t + 1) // 2 > args.max_hs:
                res["skipped"].append(f"{count}x{side}")
                continue
            res["scaling"].append(bench_scaling(count, side, args.repeats))
    if not args.skip_loop:
        sides = tuple(int(t) for t in args.loop_sides.split(","))
        pb = problems.sdp_large_cones(n=args.n, sides=sides)
        run_device(pb)                                                 # warm-up: code objects, torch, the allocator
        th, td = [], []
        for _ in range(args.repeats):
            dt, nbytes = run_host(pb, args.host_iters)
            th.append(float(np.median(dt)) * 1e3)
            dt, r = run_device(pb)
            td.append(float(np.median(dt)) * 1e3)
        res["loop"] = dict(workload=pb.name, n=pb.n, m=pb.m, host_ms=med(th), host_spread=spread(th), device_ms=med(td),
                           device_spread=spread(td), device_iters=r.iterations, host_iters_timed=args.host_iters - 1,
                           hs_bytes_per_iter=nbytes)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
