"""The extended-precision cone reference (tests/cone_reference.py) on the host: it agrees with the independent numpy
construction (tests/ref_kkt_numpy.py) on well-conditioned points, the oracle stays inside its bounds at every shape the
GPU tests use (PSD sides up to 48, SOC dims up to 4097, every spectrum class, points near the SOC boundary), and the
bounds are tight enough to reject wrong answers by at least 10x."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd.cones import SecondOrderConeT, PSDTriangleConeT
from tests import cone_reference as cr
from tests.oracle_bindings import OracleKKT
from tests.ref_kkt_numpy import soc_nt, soc_W2, psd_W2

PSD_SIDES = (1, 2, 3, 7, 8, 15, 16, 17, 24, 25, 31, 32, 33, 40, 47, 48)
SOC_DIMS = (2, 3, 4, 5, 6, 63, 64, 65, 66, 127, 128, 129, 1000, 4097)
WORST = cr.Worst("oracle against the extended-precision reference")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    WORST.report()


def _oracle(cones):
    m = sum(c.numel for c in cones)
    return OracleKKT(sp.identity(2, format="csc"), sp.csc_matrix(np.ones((m, 2))), cones)


def _assert_within(ratios, where):
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"{where}: error / bound > 1 for {bad}"


# ---- the reference against ref_kkt_numpy --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 5, 12, 65])
def test_soc_reference_matches_numpy_construction(n):
    rng = np.random.default_rng(100 + n)
    s, z = cr.soc_pair(rng, n)
    ref = cr.soc_ref(s, z)
    eta, w = soc_nt(s, z)
    assert abs(ref["eta"] - eta) <= 1e-14 * eta
    np.testing.assert_allclose(ref["w"], w, rtol=0, atol=1e-14 * np.abs(w).max())
    assert abs(ref["wJw_minus_1"]) < 1e-40
    H = soc_W2(s, z)
    if n <= 4:
        np.testing.assert_allclose(ref["H"], H, rtol=0, atol=1e-13 * np.abs(H).max())
    else:
        D = np.r_[ref["d"], np.ones(n - 1)]
        H2 = ref["eta2"] * (np.diag(D) + np.outer(ref["u"], ref["u"]) - np.outer(ref["v"], ref["v"]))
        np.testing.assert_allclose(H2, H, rtol=0, atol=1e-13 * np.abs(H).max())
    # lambda = W z = W^{-T} s: lambda' lambda = s'z and lambda'J lambda = res(s) res(z)
    J = np.r_[1.0, -np.ones(n - 1)]
    lam = ref["lam"]
    assert lam @ lam == pytest.approx(s @ z, rel=1e-13)
    assert lam @ (J * lam) == pytest.approx(np.sqrt((s @ (J * s)) * (z @ (J * z))), rel=1e-12)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_psd_reference_matches_numpy_construction(k):
    rng = np.random.default_rng(200 + k)
    s, z = cr.psd_pair(rng, k, "interior")
    ref = cr.psd_ref(s, z, k)
    H = psd_W2(s, z, k)
    Href = cr.skron(ref["A"], ref["A"])
    np.testing.assert_allclose(Href, H, rtol=0, atol=1e-12 * np.abs(H).max())
    Hs, _ = cr.psd_hs(ref)
    np.testing.assert_array_equal(Hs, cr.packed_triu(Href))
    # lambda = the eigenvalues of (Z^{1/2} S Z^{1/2})^{1/2}
    S, Z = cr.smat(s, k), cr.smat(z, k)
    w, V = np.linalg.eigh(Z)
    Zh = (V * np.sqrt(w)) @ V.T
    ev = np.sqrt(np.linalg.eigvalsh(Zh @ S @ Zh))[::-1]
    np.testing.assert_allclose(ref["lam"], ev, rtol=1e-12)
    np.testing.assert_allclose(ref["A"] @ ref["Ainv"], np.eye(k), atol=1e-13)
    x = rng.standard_normal(len(s))
    y, _ = cr.psd_mul_Hs(ref, x)
    np.testing.assert_allclose(y, H @ x, rtol=0, atol=1e-12 * np.abs(H @ x).max())


def test_nn_reference_and_numpys_formula():
    """s/z is correctly rounded; sqrt(fl(s/z)) rounds twice and stays within the bound of the exact sqrt(s/z)"""
    rng = np.random.default_rng(7)
    s, z = cr.nn_point(rng, 300), cr.nn_point(rng, 300)
    ref = cr.nn_ref(s, z)
    np.testing.assert_array_equal(ref["Hs"], s / z)
    b = cr.nn_bounds(ref)
    assert cr.ratio(np.sqrt(s / z) - ref["w"], b["w"]) <= 1.0
    assert cr.ratio(np.sqrt(s * z) - ref["lam"], b["lam"]) <= 1.0


# ---- the oracle inside the bounds at every new shape -----------------------------------------------------------------
@pytest.mark.parametrize("k", PSD_SIDES)
def test_oracle_psd_within_bounds_every_side(k):
    rng = np.random.default_rng(1000 + k)
    s, z = cr.psd_pair(rng, k, "interior")
    ref = cr.psd_ref(s, z, k)
    o = _oracle([PSDTriangleConeT(k)])
    assert o.update_scaling(s, z)
    (R, Ri, lam), = o.psd_scaling()
    r = cr.psd_ratios(ref, lam, R, Ri, o.get_Hs())
    x = rng.standard_normal(len(s))
    y, b = cr.psd_mul_Hs(ref, x)
    r["mulHs"] = cr.ratio(o.mul_Hs(x) - y, b)
    r["mulHs_z"] = cr.ratio(o.mul_Hs(z) - s, cr.psd_mul_Hs(ref, z)[1])
    _assert_within(WORST.add(r, f"PSD({k}) interior"), f"PSD({k})")


@pytest.mark.parametrize("cls", [c for c in cr.PSD_CLASSES if c != "interior"])
@pytest.mark.parametrize("k", [7, 48])
def test_oracle_psd_within_bounds_every_spectrum(k, cls):
    rng = np.random.default_rng(2000 + k)
    s, z = cr.psd_pair(rng, k, cls)
    ref = cr.psd_ref(s, z, k)
    o = _oracle([PSDTriangleConeT(k)])
    assert o.update_scaling(s, z)
    (R, Ri, lam), = o.psd_scaling()
    _assert_within(WORST.add(cr.psd_ratios(ref, lam, R, Ri, o.get_Hs()), f"PSD({k}) {cls}"), f"PSD({k}) {cls}")


@pytest.mark.parametrize("delta", [None, 1e-2, 1e-6, 1e-10])
def test_oracle_soc_within_bounds(delta):
    rng = np.random.default_rng(3000)
    for n in SOC_DIMS:
        for which in ("s", "z", "both"):
            s, z = cr.soc_pair(rng, n, delta, which)
            ref = cr.soc_ref(s, z)
            o = _oracle([SecondOrderConeT(n)])
            assert o.update_scaling(s, z)
            w, eta = o.scaling_w()
            kw = dict(lam=o.cone_lambda(), Hs=o.get_Hs(), w=w, eta=eta[0])
            if n > 4:
                u, v, e2, _ = o.soc_sparse()
                kw.update(u=u, v=v, eta2=e2[0])
            _assert_within(WORST.add(cr.soc_ratios(ref, **kw), f"SOC({n}) delta={delta} {which}"), f"SOC({n}) {delta}")
            if delta is None:
                break


# ---- the bounds have teeth -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 17, 48])
def test_lambda_from_eig_of_MtM_is_rejected(k):
    """lambda from eig(M'M), M = L2'L1 (the squared-condition route k_cone_psd's comment rejects), on the ill-conditioned
    set: at least 10x outside the bound that the SVD of M meets."""
    rng = np.random.default_rng(5)
    s, z = cr.psd_pair(rng, k, "cond")
    ref = cr.psd_ref(s, z, k)
    L1, L2 = np.linalg.cholesky(cr.smat(s, k)), np.linalg.cholesky(cr.smat(z, k))
    M = L2.T @ L1
    b = cr.psd_bounds(ref)["lam"]
    assert cr.ratio(np.linalg.svd(M, compute_uv=False) - ref["lam"], b) <= 1.0
    bad = np.sqrt(np.abs(np.linalg.eigvalsh(M.T @ M)))[::-1]
    assert cr.ratio(bad - ref["lam"], b) >= 10.0


def _bump(x, i, rel=1e-10):
    y = np.array(x, dtype=float, copy=True)
    y.flat[i] *= 1.0 + rel
    return y


@pytest.mark.parametrize("k", [3, 8])
def test_psd_bounds_reject_a_1e10_change(k):
    rng = np.random.default_rng(300 + k)
    s, z = cr.psd_pair(rng, k, "interior")
    ref = cr.psd_ref(s, z, k)
    b = cr.psd_bounds(ref)
    for i in range(k):
        assert cr.ratio(_bump(ref["lam"], i) - ref["lam"], b["lam"]) >= 10.0
    # a relative change of 1e-10 of every entry of A of at least a tenth of the largest, and a change of 1e-10 max|A| of
    # every entry: a small entry of A is only determined to ~ k u |R| |R|' (its own size carries no relative accuracy)
    Amax = np.abs(ref["A"]).max()
    for i in range(k * k):
        if abs(ref["A"].flat[i]) >= 0.1 * Amax:
            assert cr.ratio(_bump(ref["A"], i) - ref["A"], b["A"]) >= 10.0
        dA = np.zeros((k, k))
        dA.flat[i] = 1e-10 * Amax
        assert cr.ratio(dA, b["A"]) >= 10.0
    H, _ = cr.psd_hs(ref)
    j = int(np.argmax(np.abs(H)))
    assert cr.ratio(_bump(H, j) - H, b["Hs"]) >= 10.0


@pytest.mark.parametrize("n", [3, 5, 65, 129])
def test_soc_bounds_reject_a_1e10_change(n):
    rng = np.random.default_rng(400 + n)
    s, z = cr.soc_pair(rng, n)
    ref = cr.soc_ref(s, z)
    b = cr.soc_bounds(ref)
    assert cr.ratio(ref["eta"] * 1e-10, b["eta"]) >= 10.0
    for i in (0, 1, n // 2, n - 1):
        assert cr.ratio(_bump(ref["w"], i) - ref["w"], b["w"]) >= 10.0
        assert cr.ratio(_bump(ref["lam"], i) - ref["lam"], b["lam"]) >= 10.0
        if n > 4 and i > 0:
            assert cr.ratio(_bump(ref["u"], i) - ref["u"], b["u"]) >= 10.0
            assert cr.ratio(_bump(ref["v"], i) - ref["v"], b["v"]) >= 10.0


def test_nn_bounds_reject_a_1e10_change():
    rng = np.random.default_rng(9)
    s, z = cr.nn_point(rng, 50), cr.nn_point(rng, 50)
    ref, b = cr.nn_ref(s, z), cr.nn_bounds(cr.nn_ref(s, z))
    assert cr.ratio(_bump(ref["w"], 3) - ref["w"], b["w"]) >= 10.0


def test_ratio_does_not_let_nan_or_inf_through():
    assert cr.ratio([np.nan, 1e-20, 0.0], [1.0, 1.0, 1.0]) > 1.0
    assert cr.ratio([1.0, 1e-20], [np.nan, 1.0]) > 1.0
    assert cr.ratio([np.inf, 0.0], [1.0, 1.0]) > 1.0
    assert cr.ratio([0.0, 1e-20], [0.0, 1.0]) == 1e-20


@pytest.mark.parametrize("e", [300, -300])
@pytest.mark.parametrize("k", [7, 48])
def test_oracle_psd_at_scale_extremes(k, e):
    """s, z scaled by 2^+-300: the oracle's Jacobi SVD must still succeed and match the reference scaled exactly (the
    product of squared column norms in its skip test overflowed at 2^300: every rotation skipped, no failure reported)"""
    rng = np.random.default_rng(1000 + k)
    s, z = cr.psd_pair(rng, k, "interior")
    ref = cr.psd_ref(s, z, k)
    o = _oracle([PSDTriangleConeT(k)])
    assert o.update_scaling(s * 2.0 ** e, z * 2.0 ** e)
    (R, Ri, lam), = o.psd_scaling()
    r = cr.psd_ratios(ref, lam / 2.0 ** e, R, Ri, o.get_Hs())
    _assert_within(WORST.add(r, f"PSD({k}) at 2^{e}"), f"PSD({k}) at 2^{e}")
