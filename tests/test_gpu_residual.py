"""The residual, norm and partial-reduction kernels of the refinement layer against an exact residual, at the edges of
their dispatch (csrc/kernels.hip: k_residual<G, NC>, k_residual_long_chunks / _finish, k_residual_rm<V>, k_finish_norm,
k_finish_norm_rm, k_absmax, and block_max3_of inside k_ir_round), through hipkkt_kkt_get_residual -- which launches them
the way a solve of that column count does (route 0: column-major with a finishing kernel; 1: partial maxima reduced by
k_ir_round; 2: row-major).

For every case, with tests/residual_reference.py:
  - the device's e lies within residual_bound of residual_exact, row by row (a bound that holds for ANY summation order,
    so there is no measured margin in it);
  - norm_e[c] is max |e[:, c]| of the device's own e and norm_b[c] is max |b[:, c]|, bit for bit: a maximum is exact.
The problems come from builders with prescribed row lengths; each asserts from the handle's own pattern that the edge
its case is named after is reached.  Worst error / bound ratios are printed under -s.  Short rows sit close to the
bound by nature (a 2-entry row's bound is 3 u S and two roundings already give up to 2 u S)."""
import numpy as np
import pytest

from tests import residual_reference as rr
from tests.cone_reference import Worst

pytestmark = pytest.mark.gpu

WORST = Worst("residual kernels")
_H = {}


def handle(name):
    """(ks, K image, facts) of a builder: created, given values (kktsolver_update) and checked once per session."""
    if name not in _H:
        from cuclarabel_amd.kktsolver import HipKKTSolver
        spec = getattr(rr, "spec_" + name)()
        P, A, cones = rr.make_problem(spec)
        ks = HipKKTSolver(P, A, cones)
        assert ks.kktsolver_update(rr.hs_values(cones, spec["seed"] + 1))
        K = rr.sym_of(ks)
        facts = rr.check_shape(K, spec["want"])
        assert ks.N == K.shape[0] and ks.p == 0
        _H[name] = (ks, K, facts)
    return _H[name]


def check(name, route, k, tag, x=None, b=None, clean=None):
    """One probe call and the three assertions; clean: the columns to compare (default all).  -> (e, norm_e, norm_b)"""
    ks, K, facts = handle(name)
    if x is None:
        x, b = rr.probe_vectors(facts["N"], k, 977 + 31 * k + route)
    e, ne, nb = ks.residual(x, b, route=route)
    cols = list(range(k)) if clean is None else clean
    exact = rr.residual_exact(K, x[:, cols], b[:, cols])
    bound = rr.residual_bound(K, x[:, cols], b[:, cols])
    ratio = rr.error_vs_exact(e[:, cols], exact) / bound
    i, j = np.unravel_index(np.argmax(ratio), ratio.shape)
    where = f"{tag} row {i} (length {facts['lengths'][i]}) column {cols[j]}"
    print(f"\n[residual] {tag}: N {facts['N']} lanes {facts['lanes']} nlong {facts['nlong']} grid {facts['grid']} "
          f"worst error/bound {ratio.max():.3f} at row {i} (length {facts['lengths'][i]})")
    WORST.add({f"{name}/route{route}": float(ratio.max())}, where)
    assert ratio.max() <= 1.0, (where, float(ratio.max()))
    for c in cols:
        assert ne[c] == np.abs(e[:, c]).max(), (tag, c, ne[c], np.abs(e[:, c]).max())
        assert nb[c] == np.abs(b[:, c]).max(), (tag, c, nb[c], np.abs(b[:, c]).max())
    return e, ne, nb


# ------------------------------------------------------------------------------------------------ row-length edges
@pytest.mark.parametrize("k", [1, 2, 3, 9, 10])
def test_lanes8_row_length_edges_route0(k):
    """Rows of 1, 2, 7, 8, 9, 63, 64, 65, 4095, 4096, 4097, 6144 (a whole number of chunks) and 6145 entries, four long
    rows that are no neighbours, N = 6270 (no multiple of 32); NC = 2 for even k, 1 for odd."""
    check("edges8", 0, k, f"lanes8-lengths-1..6145-route0-nrhs{k}")


@pytest.mark.parametrize("route,k", [(0, 1), (0, 2), (0, 5), (1, 1), (1, 2), (1, 4), (2, 9), (2, 17), (2, 33), (2, 64)],
                         ids=lambda v: str(v))
def test_lanes64_row_length_edges(route, k):
    """Rows of 63, 64, 65, 127, 128, 129 entries at lane width 64, N = 179 (no multiple of 4), no long rows.  Route 2:
    KP = 16 (V = 1), 32 (V = 2), 48 (V = 1, three column groups), 64 (V = 4 where the multi_vec knob allows it; the
    schedule summary does not say which instance ran, so that is not asserted)."""
    ks, K, facts = handle("edges64")
    KP = (k + 15) & ~15
    if route == 2:
        assert KP == {9: 16, 17: 32, 33: 48, 64: 64}[k]
    e, ne, nb = check("edges64", route, k, f"lanes64-lengths-63..129-route{route}-nrhs{k}-KP{KP}")
    assert e.shape == (facts["N"], k)


def test_row_major_padding_columns_do_not_leak():
    """9 columns in a KP = 16 layout, after a 16-column call that left seven more columns of x, b and e in the buffers:
    the 9 returned columns are those of a 9-column call on clean buffers, bit for bit, and the norms are theirs."""
    ks, K, facts = handle("edges64")
    x, b = rr.probe_vectors(facts["N"], 16, 4242)
    x[:, 9:] *= 1e6
    b[:, 9:] *= 1e6
    e16, ne16, nb16 = ks.residual(x, b, route=2)
    e9, ne9, nb9 = check("edges64", 2, 9, "lanes64-route2-padding-after-16", x=x[:, :9].copy(), b=b[:, :9].copy())
    assert np.array_equal(e9, e16[:, :9]) and np.array_equal(ne9, ne16[:9]) and np.array_equal(nb9, nb16[:9])
    assert ne9.max() < 1e3 < ne16[9:].min()                 # nothing of the x 1e6 columns in the nine


@pytest.mark.parametrize("k", [1, 2])
def test_lanes64_more_than_256_long_rows(k):
    """257 rows of 4201 entries (a dense 257 x 4200 block on a zero cone) at lane width 64: the second trip of
    k_residual_long_finish's loop over the long rows."""
    ks, K, facts = handle("long257")
    assert facts["nlong"] == 257 > 256 and facts["lanes"] == 64
    check("long257", 0, k, f"lanes64-257-long-rows-route0-nrhs{k}")


# ------------------------------------------------------------------------------------------------ grid-stride wraps
@pytest.mark.parametrize("route,k", [(0, 1), (0, 2), (2, 9), (1, 4)], ids=lambda v: str(v))
def test_grid_stride_wraps(route, k):
    """N = 70 001 at lane width 8: k_residual's grid is capped at 2048 workgroups of 32 rows (routes 0 and 1: every
    workgroup takes a second trip, and route 1 reduces 2048 + 1 partials per column in k_ir_round); k_residual_rm's at
    512 workgroups of 16 rows (route 2: nine trips)."""
    ks, K, facts = handle("wrap70k")
    assert facts["grid_uncapped"] > rr.NORM_PARTS == facts["grid"] and facts["N"] > rr.RM_BLOCKS * 16 and facts["lanes"] == 8
    check("wrap70k", route, k, f"wrap-N70001-route{route}-nrhs{k}")


# ------------------------------------------------------------------------------------------------ non-finite input
def _bad_vectors(N, k, rows_b, row_x, seed):
    x, b = rr.probe_vectors(N, k, seed)
    b[rows_b, 0] = np.inf
    x[row_x, 1] = np.nan
    return x, b


@pytest.mark.parametrize("route,k", [(0, 3), (0, 4), (1, 4), (2, 9)], ids=lambda v: str(v))
def test_non_finite_input_is_reported_per_column(route, k):
    """inf in b of column 0, nan in x of column 1, the rest clean: ordinary arithmetic on valid memory.  The call
    succeeds; norm_e is non-finite in columns 0 and 1 only, norm_b is inf in column 0, the clean columns meet the bound
    (with k = 4 on route 0 a clean column shares its matrix walk with no bad one, with k = 3 there is no sharing, on
    routes 1 and 2 clean and bad columns share a workgroup)."""
    ks, K, facts = handle("edges64")
    x, b = _bad_vectors(facts["N"], k, 5, 140, 600 + route)
    clean = list(range(2, k))
    e, ne, nb = check("edges64", route, k, f"nonfinite-lanes64-route{route}-nrhs{k}", x=x, b=b, clean=clean)
    assert not np.isfinite(ne[0]) and not np.isfinite(ne[1]) and np.isfinite(ne[2:]).all(), ne
    assert nb[0] == np.inf and nb[1] == np.abs(b[:, 1]).max(), nb


@pytest.mark.parametrize("where", ["long_row", "short_row"])
def test_non_finite_input_with_long_rows(where):
    """The same on the problem with long rows, the bad entries in a long row (k_residual_long_*) or in a 2-entry row."""
    ks, K, facts = handle("edges8")
    L = facts["lengths"]
    i = int(np.flatnonzero(L == (6145 if where == "long_row" else 2))[0])
    x, b = _bad_vectors(facts["N"], 4, i, i, 700)
    e, ne, nb = check("edges8", 0, 4, f"nonfinite-lanes8-{where}-route0-nrhs4", x=x, b=b, clean=[2, 3])
    assert not np.isfinite(ne[0]) and not np.isfinite(ne[1]) and np.isfinite(ne[2:]).all(), ne
    assert nb[0] == np.inf and nb[1] == np.abs(b[:, 1]).max(), nb
    assert not np.isfinite(e[i, 0]) and not np.isfinite(e[i, 1])


# ------------------------------------------------------------------------------------------------ route validity
def test_route_validity_and_the_handle_survives_the_probe():
    """Routes 1 and 2 need a K without long rows, route 1 also 1, 2 or 4 columns: HIPKKT_ERR_ARG otherwise.  The probe
    leaves the right-hand side of kktsolver_setrhs and the solver's state alone: the solve after the probe calls returns
    what the solve before them did."""
    from cuclarabel_amd import _lib
    ks, K, facts = handle("edges8")
    n, m = ks.n, ks.m
    rng = np.random.default_rng(5)
    rx, rz = rng.standard_normal(n), rng.standard_normal(m)
    ks.kktsolver_setrhs(rx, rz)
    xs = [np.zeros(n) for _ in range(3)]
    zs = [np.zeros(m) for _ in range(3)]
    assert ks.kktsolver_solve(xs[0], zs[0]) and ks.kktsolver_solve(xs[1], zs[1])
    x, b = rr.probe_vectors(facts["N"], 4, 1)
    L = _lib.lib()
    ne = np.zeros(4)
    for route, k in ((1, 1), (1, 2), (1, 4), (2, 4), (2, 3)):
        rc = L.hipkkt_kkt_get_residual(ks._h, route, k, _lib.ptr(x), _lib.ptr(b), None, _lib.ptr(ne), None)
        assert rc == -1, (route, k, rc)                      # HIPKKT_ERR_ARG
        with pytest.raises(_lib.HipKKTError):
            ks.residual(x[:, :k], b[:, :k], route=route)
    ks64 = handle("edges64")[0]
    x64, b64 = rr.probe_vectors(ks64.N, 3, 2)
    assert L.hipkkt_kkt_get_residual(ks64._h, 1, 3, _lib.ptr(np.asfortranarray(x64)), _lib.ptr(np.asfortranarray(b64)), None,
                                     _lib.ptr(ne), None) == -1
    assert L.hipkkt_kkt_get_residual(ks._h, 3, 1, _lib.ptr(x), _lib.ptr(b), None, _lib.ptr(ne), None) == -1
    for k in (1, 2, 9):                                      # valid probes between the solves as well
        ks.residual(x[:, :1].repeat(k, axis=1), b[:, :1].repeat(k, axis=1), route=0)
    assert ks.kktsolver_solve(xs[2], zs[2])
    assert np.array_equal(xs[2], xs[1]) and np.array_equal(zs[2], zs[1])


def test_report_worst_ratios():
    WORST.report()
