#!/usr/bin/env python
"""Per-iteration time of the interior-point loop on a batch of independent cfg4 members (problems.config4), two ways:

  --mode batch    ipm_device.solve_device_batch on the members: every member its own scalars and status
  --mode stacked  ipm_device.solve_device(plumbing="device") on problems.block_diagonal of the same members: ONE conic
                  problem -- the only loop a library without the _batch entry points can run on such a stack

Both loops do the same vector work per iteration (one update, two solves, the same elementwise and cone kernels), so
their per-iteration times are comparable; the iteration COUNTS are not the same thing (the stacked loop ends with one
status).  --member-refinement (mode batch): ipm_device.solve_device_batch_refined, the refinement's accept / stop rule per
member; `refinement_rounds` is the handle's total of refinement rounds (sweep pairs behind the first solve) either way,
`refinement_rounds_per_member` each member's own total under the member rule.  --isolate (mode batch):
ipm_device.solve_device_batch_isolated, every member under its own static regulariser and failure status (with
--member-refinement: its member rule as well).  --profile (mode batch): the handle's event profile is switched on at the
loop's first iteration; `update_ms_per_update` and `factor_ms_per_update` are the device times of a kkt_update!'s value
update (cone scaling, scatter, regulariser) and factorisation (with --isolate: the pivot pass behind it included) -- the
timed loop is slower with the events in it, so take problems/s from a run without.  One JSON line per run.  --root: the tree whose cuclarabel_amd is imported (another build of the library for an
A/B comparison in one session: run this script with the other tree's root and --mode stacked).

--resident (mode batch): a parameter sweep on one structure, two ways in alternation, one JSON line per round with both
times: `seconds_resident` -- a solver_device.DeviceBatchSolver set up ONCE before the rounds, per round
`.update_data_stack(q=..., b=...)` (device tensors, by pointer) plus `.solve()`; `seconds_fresh` -- the batch built anew
from the round's data (a new DeviceBatchSolver with the same equilibrations, then `.solve()`), which is what a user
without the resident solver pays every round.  --member-refinement / --isolate choose the member modes of both.

    python scripts/bench_batch_loop.py --mode batch --members 64 --n 10000 --runs 3
    python scripts/bench_batch_loop.py --mode batch --members 64 --n 10000 --runs 3 --resident --member-refinement --isolate
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["batch", "stacked", "alone"], default="batch")
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--member-refinement", action="store_true")
    ap.add_argument("--isolate", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    if args.member_refinement and args.mode != "batch":
        ap.error("--member-refinement goes with --mode batch")
    if (args.isolate or args.profile or args.resident) and args.mode != "batch":
        ap.error("--isolate, --profile and --resident go with --mode batch")
    if args.resident and args.profile:
        ap.error("--resident times whole rounds; --profile goes with the plain batch loop")
    sys.path.insert(0, args.root)
    import torch
    from cuclarabel_amd import ipm_device, problems

    pbs = [problems.config4(j, n=args.n) for j in range(args.members)]
    if args.resident:
        return resident_rounds(args, pbs, torch)
    # the loops call `inspect` once per iteration, right behind the residual call's read-back: the time between the first
    # and the last call is the loop's own, without the handle's set-up (symbolic analysis) and the final copy
    stamps, seen = [], {}

    def stamp(tensors, backend):
        stamps.append(time.perf_counter())
        if args.profile and len(stamps) == 1:
            backend.ks.profile_enable(True)
        seen["ks"] = backend.ks
    if args.mode == "batch":
        data = [(pb.P, pb.q, pb.A, pb.b, pb.cones) for pb in pbs]
        loop = ipm_device.solve_device_batch_refined if args.member_refinement else ipm_device.solve_device_batch
        if args.isolate:
            loop = lambda d, inspect: ipm_device.solve_device_batch_isolated(d, inspect=inspect, member_refinement=args.member_refinement)
        run = lambda: loop(data, inspect=stamp)
        iters = lambda res: max(r.iterations for r in res)
        def device_times():
            pr = seen["ks"].profile()
            return dict(update_ms_per_update=round(pr["update_ms"] / max(pr["n_factor"], 1), 5),
                        factor_ms_per_update=round(pr["factor_ms"] / max(pr["n_factor"], 1), 5)) if args.profile else {}
        extra = lambda res: dict(iterations_per_member=[r.iterations for r in res],
                                 statuses=sorted(set(r.status for r in res)), member_refinement=bool(args.member_refinement),
                                 isolate=bool(args.isolate), **device_times(),
                                 refinement_rounds=int(seen["ks"].profile()["ir_iterations"]),
                                 **(dict(refinement_rounds_per_member=[r.kkt_ir_rounds for r in res]) if args.member_refinement else {}))
    elif args.mode == "stacked":
        st = problems.block_diagonal(pbs)
        run = lambda: ipm_device.solve_device(st.P, st.q, st.A, st.b, st.cones, inspect=stamp, plumbing="device")
        iters = lambda res: res.iterations
        extra = lambda res: dict(statuses=[res.status])
    else:                                                # every member by itself: the counts the batch's are compared with
        run = lambda: [ipm_device.solve_device(pb.P, pb.q, pb.A, pb.b, pb.cones, plumbing="device") for pb in pbs]
        iters = lambda res: sum(r.iterations for r in res)
        extra = lambda res: dict(iterations_per_member=[r.iterations for r in res], iterations_max=max(r.iterations for r in res),
                                 statuses=sorted(set(r.status for r in res)))
    run()                                                # warm-up: kernels loaded, allocator primed
    for k in range(args.runs):
        torch.cuda.synchronize()
        del stamps[:]
        t0 = time.perf_counter()
        res = run()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = dict(mode=args.mode, members=args.members, n=args.n, run=k, seconds=round(dt, 6), loop_iterations=iters(res),
                   root=os.path.basename(os.path.abspath(args.root)))
        if args.mode == "batch":
            out["problems_per_s"] = round(args.members / dt, 2)
        if len(stamps) > 1:
            out["ms_per_iteration"] = round(1e3 * (stamps[-1] - stamps[0]) / (len(stamps) - 1), 4)
        out.update(extra(res))
        print(json.dumps(out), flush=True)


def resident_rounds(args, pbs, torch):
    """set-up once, then per round new q and b for every member: resident update + solve against a batch built anew"""
    import numpy as np
    from cuclarabel_amd.solver_device import DeviceBatchSolver
    modes = dict(member_refinement=bool(args.member_refinement), isolate=bool(args.isolate))
    data = [(pb.P, np.asarray(pb.q, float), pb.A, np.asarray(pb.b, float), pb.cones) for pb in pbs]
    t0 = time.perf_counter()
    S = DeviceBatchSolver(data, **modes)
    S.solve()                                            # warm-up: kernels loaded, allocator primed
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    dev = S._c.dev
    for k in range(args.runs):
        fq, fb = 1.0 + 0.05 * (k + 1), 1.0 + 0.01 * (k + 1)
        new = [(P, fq * q, A, fb * b, cones) for (P, q, A, b, cones) in data]
        qd = torch.from_numpy(np.concatenate([mb[1] for mb in new])).to(dev)
        bd = torch.from_numpy(np.concatenate([mb[3] for mb in new])).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.update_data_stack(q=qd, b=bd)
        res = S.solve()
        torch.cuda.synchronize()
        t_res = time.perf_counter() - t0
        t0 = time.perf_counter()
        ref = DeviceBatchSolver(new, equilibrations=S.equilibrations, **modes).solve()
        torch.cuda.synchronize()
        t_fresh = time.perf_counter() - t0
        same = all(a.x.tobytes() == b.x.tobytes() and a.status == b.status for a, b in zip(res, ref))
        print(json.dumps(dict(mode="batch-resident", members=args.members, n=args.n, run=k, setup_seconds=round(setup, 6),
                              seconds_resident=round(t_res, 6), seconds_fresh=round(t_fresh, 6),
                              problems_per_s_resident=round(args.members / t_res, 2),
                              problems_per_s_fresh=round(args.members / t_fresh, 2),
                              loop_iterations=max(r.iterations for r in res), statuses=sorted(set(r.status for r in res)),
                              resident_equals_fresh=bool(same), root=os.path.basename(os.path.abspath(args.root)), **modes)),
              flush=True)


if __name__ == "__main__":
    main()
