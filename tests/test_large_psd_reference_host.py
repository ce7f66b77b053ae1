"""The references of the large-PSD GPU tests, on the host.  The bounds of tests/cone_reference.py carry k u factors and
were fixed at sides <= 48 so that the fp64 host code uses at most a quarter of each, which leaves the device 4x.  Here
the oracle is held to that quarter at the new sides: 49 (smallest, odd), 64 (32 column pairs), 65 and 66 (the first
sides past them), and at 65 for every spectrum class.  Worst ratio per quantity is printed under -s."""
import numpy as np
import pytest
import scipy.sparse as sp

from cuclarabel_amd.cones import PSDTriangleConeT
from tests import cone_reference as cr
from tests.oracle_bindings import OracleKKT

HOST_SHARE = 0.25
WORST = cr.Worst("oracle against the extended-precision reference, sides 49 .. 66")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    WORST.report()


def _oracle_ratios(k, cls, seed):
    rng = np.random.default_rng(seed)
    s, z = cr.psd_pair(rng, k, cls)
    ref = cr.psd_ref(s, z, k)
    o = OracleKKT(sp.identity(2, format="csc"), sp.csc_matrix(np.ones((len(s), 2))), [PSDTriangleConeT(k)])
    assert o.update_scaling(s, z)
    (R, Ri, lam), = o.psd_scaling()
    r = cr.psd_ratios(ref, lam, R, Ri, o.get_Hs())
    x = rng.standard_normal(len(s))
    y, b = cr.psd_mul_Hs(ref, x)
    r["mulHs"] = cr.ratio(o.mul_Hs(x) - y, b)
    r["mulHs_z"] = cr.ratio(o.mul_Hs(z) - s, cr.psd_mul_Hs(ref, z)[1])
    return r


def _assert_within_share(ratios, where):
    bad = {k: v for k, v in ratios.items() if not v <= HOST_SHARE}
    assert not bad, f"{where}: the oracle uses more than {HOST_SHARE} of the bound for {bad}"


@pytest.mark.parametrize("k", [49, 64, 65, 66])
def test_oracle_within_a_quarter_of_the_bounds_at_the_new_sides(k):
    _assert_within_share(WORST.add(_oracle_ratios(k, "interior", 1000 + k), f"PSD({k}) interior"), f"PSD({k})")


@pytest.mark.parametrize("cls", [c for c in cr.PSD_CLASSES if c != "interior"])
def test_oracle_within_a_quarter_of_the_bounds_every_spectrum_at_65(cls):
    _assert_within_share(WORST.add(_oracle_ratios(65, cls, 2065), f"PSD(65) {cls}"), f"PSD(65) {cls}")


@pytest.mark.parametrize("leave", [True, False], ids=["binding", "nothing-binds"])
@pytest.mark.parametrize("k", [49, 65])
def test_numpy_cone_classes_within_a_quarter_of_the_step_bounds(k, leave):
    """ds (affine and combined), the step length, margins and the shift of the fp64 classes of ipm.py against
    tests/step_reference.py, by the method (and under the HOST_SHARE) of tests/test_step_reference_host.py"""
    from tests import step_reference as sr
    from tests.test_step_reference_host import _compare, HOST_SHARE as share
    assert share == HOST_SHARE
    _compare(sr.Case([("psd", k, "interior", leave)], seed=k), f"psd {k} {'leaving' if leave else 'staying'}")
