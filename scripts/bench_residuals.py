"""One hipkkt_kkt_system_residuals call against the torch block of `ipm_device.solve_device` that it replaces (the three
CSR mat-vecs, five vector expressions and twelve reductions at the top of the loop, read-back included), on config2 at the
benchmark's size, same process, same device, runs interleaved.  Prints one JSON line:

    torch_us / device_us     median over the rounds of the per-call time (host clock around calls that end in a synchronise)
    torch_spread / device_spread   (max - min) / median over the rounds: the run-to-run spread of each
    bytes, hbm_share         what the new call must move (the image's walked prefixes: value + column per entry, two row
                             pointers per row; five vectors in -- nine with equilibration, not timed here --, five out)
                             and that over device_us as a share of 8 TB/s

Usage: python scripts/bench_residuals.py [--n 100000] [--rounds 8] [--calls 1000] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuclarabel_amd import ipm_device, problems          # noqa: E402
from cuclarabel_amd.ipm import HipSystemBackend          # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import scipy.sparse as sp
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_residuals: no GPU (a timing needs one)")
    pb = problems.config2(n=args.n)
    n, m = pb.n, pb.m
    backend = HipSystemBackend(pb.P, pb.A, pb.cones)
    ks, system = backend.ks, backend.system
    dev = system._devstr
    ks.set_stream(torch.cuda.current_stream(torch.device(dev)).cuda_stream)
    system.init(pb.q, pb.b)
    Pt = sp.triu(sp.csc_matrix(pb.P), format="csc")
    Pfull_h = (Pt + sp.triu(Pt, 1).T).tocsr()
    A_h = sp.csr_matrix(pb.A)
    Pfull, Ad, At = (ipm_device._Csr(M, dev) for M in (Pfull_h, A_h, A_h.T))
    rng = np.random.default_rng(5)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    x, s, z, qd, bd = up(rng.standard_normal(n)), up(rng.standard_normal(m)), up(rng.standard_normal(m)), up(pb.q), up(pb.b)
    tau = 0.9
    out = [torch.zeros(k, dtype=torch.float64, device=dev) for k in (n, m, n, m, n)]
    nrm = torch.linalg.vector_norm

    def torch_block():
        Px = Pfull.mv(x)
        rx_inf = -At.mv(z)
        rz_inf = Ad.mv(x) + s
        rx = rx_inf - Px - qd * tau
        rz = rz_inf - bd * tau
        return torch.stack([qd @ x, bd @ z, s @ z, x @ Px, nrm(x), nrm(z), nrm(s), nrm(rx_inf), nrm(Px), nrm(rz_inf), nrm(rz),
                            nrm(rx)]).tolist()

    p = lambda t: t.data_ptr()

    def device_call():
        return system.residuals_dev(p(x), p(s), p(z), tau, p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(out[4]))

    a, b = np.array(torch_block()), device_call()
    agree = float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(a))))
    if not agree <= 1e-9:
        raise SystemExit(f"bench_residuals: the two paths disagree ({agree:.3g} relative): {a} / {b}")
    for _ in range(args.warmup):
        torch_block()
        device_call()
    torch.cuda.synchronize()
    t_torch, t_dev = [], []
    for _ in range(args.rounds):
        for fn, acc in ((torch_block, t_torch), (device_call, t_dev)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            acc.append((time.perf_counter() - t0) / args.calls * 1e6)
    med = lambda v: float(np.median(v))
    spread = lambda v: float((max(v) - min(v)) / np.median(v))
    walked = Pfull_h.nnz + int((Pfull_h.diagonal() == 0).sum()) + 2 * A_h.nnz      # x rows: P and A'; z rows: A
    nbytes = walked * 12 + (n + m) * 16 + 8 * 5 * (n + m)       # vectors in: x q (n), s z b (m) -- no equilibration; out: 3 n + 2 m
    res = dict(config="config2", n=n, m=m, mode=Pfull.mode, torch_us=med(t_torch), device_us=med(t_dev),
               torch_spread=spread(t_torch), device_spread=spread(t_dev), scalars_max_rel_diff=agree, bytes=nbytes,
               hbm_share=nbytes / (med(t_dev) * 1e-6) / HBM_PEAK, rounds=args.rounds, calls=args.calls)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
