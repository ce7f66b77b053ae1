#!/usr/bin/env python
"""What a re-solve costs against a fresh solve: on cfg3 and on a block-diagonal stack of 64 x cfg4,

  (a) a fresh DeviceSolver(...) plus .solve()                  -- ordering, symbolic analysis, schedule, allocations, loop
  (b) .update_q(new) plus .solve() on the resident solver      -- the loop alone
  (c) one full-vector update of P on the handle, alone         -- hipkkt_kkt_system_update_data_P, values already on the device
  (d) a two-entry update of P, alone                           -- the same call with two positions
  (e) the route to (c) without the data-updating calls         -- equilibrate.rescale_P, then HipKKTSolver.kktsolver_update_P

Every time is a host clock around work that ends in a device synchronise, after a warm-up of the same call; (c)-(e) are
means over --reps calls.  Where P has no entries the matrix updated in (c)-(e) is A.  One JSON line per problem.

    python scripts/bench_resolve.py [--small] [--reps 50] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuclarabel_amd import equilibrate, problems          # noqa: E402
from cuclarabel_amd.solver_device import DeviceSolver    # noqa: E402


def clock(fn, sync, reps=1):
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    sync()
    return (time.perf_counter() - t0) / reps, out


def measure(pb, reps):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resolve.py measures on the GPU: no device found")
    sync = torch.cuda.synchronize
    rec = dict(problem=pb.name, n=pb.n, m=pb.m, nnzP=int(pb.P.nnz), nnzA=int(pb.A.nnz))

    def fresh():
        s = DeviceSolver(pb.P, pb.q, pb.A, pb.b, pb.cones)
        return s, s.solve()

    clock(fresh, sync)                                           # warm-up: code objects, torch's allocator
    rec["a_fresh_solver_and_solve_s"], (s, r0) = clock(fresh, sync)
    rec.update(status=r0.status, iterations=r0.iterations, nnzK=int(s.system.ks.info["nnzK"]), nnzL=int(s.system.ks.info["nnzL"]))
    t_solve, _ = clock(s.solve, sync)
    rec["solve_alone_s"] = t_solve

    rng = np.random.default_rng(1)
    qs = [pb.q * (1.0 + 0.05 * rng.standard_normal(pb.n)) for _ in range(3)]

    def resolve(q):
        s.update_q(q)
        return s.solve()

    resolve(qs[0])
    tb = [clock(lambda q=q: resolve(q), sync) for q in qs[1:]]
    rec["b_update_q_and_solve_s"] = float(np.mean([t for t, _ in tb]))
    rec["b_status"] = [r.status for _, r in tb]

    which = "P" if pb.P.nnz else "A"
    M = s.P if which == "P" else s.A
    rec["updated_matrix"] = which
    vals = torch.from_numpy(M.data * 1.01).to(s._c.dev)
    two = torch.from_numpy(M.data[[0, M.nnz - 1]] * 1.01).to(s._c.dev)
    idx2 = np.array([0, M.nnz - 1], dtype=np.int64)
    upd = getattr(s.system, f"update_data_{which}_dev")
    full = lambda: upd(vals.data_ptr(), None, M.nnz)
    pair = lambda: upd(two.data_ptr(), idx2, 2)
    for fn in (full, pair):
        fn()
    rec["c_full_vector_update_s"], _ = clock(full, sync, reps)
    s.system.ks.residual(np.zeros(s.system.ks.N), np.zeros(s.system.ks.N))       # a reader: the image is current again
    rec["d_two_entry_update_s"], _ = clock(pair, sync, reps)

    eq, ks = s.equilibration, s.system.ks
    rescale = equilibrate.rescale_P if which == "P" else equilibrate.rescale_A
    push = ks.kktsolver_update_P if which == "P" else ks.kktsolver_update_A
    M2 = M.copy()
    M2.data = M.data * 1.01
    old = lambda: push(rescale(M2, eq))
    old()
    rec["e_rescale_then_update_s"], _ = clock(old, sync, max(1, reps // 10))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--small", action="store_true", help="toy sizes (a rehearsal of the script, not a measurement)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    if args.small:
        pbs = [problems.config3(nblocks=4, blk=50), problems.block_diagonal([problems.config4(j, n=300) for j in range(4)])]
    else:
        pbs = [problems.config3(), problems.block_diagonal([problems.config4(j) for j in range(64)])]
    for pb in pbs:
        line = json.dumps(measure(pb, args.reps))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
