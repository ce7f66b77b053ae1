"""The ABI surface of batches of independent problems: hipkkt_kkt_system_set_problems and the seven _batch entry points
are exported, declared in include/hipkkt.h each behind a documenting comment (reference lines, what synchronises, the
aliasing rule where the twin has one), and bound in cuclarabel_amd._lib.SYMBOLS with the header's signature; the header
states what stays joint; the Python layer has the methods and the loop."""
import ctypes as C
import inspect
import os
import re

import pytest

from cuclarabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWINS = {
    "hipkkt_kkt_system_residuals_batch": "hipkkt_kkt_system_residuals",
    "hipkkt_kkt_system_solve_batch": "hipkkt_kkt_system_solve",
    "hipkkt_kkt_system_combined_ds_batch": "hipkkt_kkt_system_combined_ds",
    "hipkkt_kkt_system_step_length_batch": "hipkkt_kkt_system_step_length",
    "hipkkt_kkt_system_shift_to_interior_batch": "hipkkt_kkt_system_shift_to_interior",
    "hipkkt_kkt_system_combined_rhs_batch": "hipkkt_kkt_system_combined_rhs",
    "hipkkt_kkt_system_add_step_batch": "hipkkt_kkt_system_add_step",
}
NAMES = ["hipkkt_kkt_system_set_problems"] + list(TWINS)
CTYPE = {"hipkkt_kkt_t": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _declaration(name):
    """(comment in front of the declaration, [parameter strings])"""
    h = _read("include", "hipkkt.h")
    mt = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", h, re.S)
    assert mt, f"{name} is not declared behind a comment in include/hipkkt.h"
    return mt.group(1), [" ".join(p.split()) for p in mt.group(2).split(",")]


def _argtypes(params):
    out = []
    for p in params:
        if "*" in p:
            out.append(C.c_void_p)
        else:
            out.append(CTYPE[p.replace("const ", "").split()[0]])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_declared_behind_a_comment_and_bound_with_the_header_signature(name):
    doc, params = _declaration(name)
    assert len(doc.split()) >= 40, "the header documents the entry point"
    assert re.search(r"\w+\.jl:\d+", doc), "the reference lines it restates"
    assert re.search(r"synchroni", doc, re.I), "what synchronises"
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int and list(argtypes) == _argtypes(params)


@pytest.mark.parametrize("name", list(TWINS))
def test_a_batch_call_is_its_twin_with_every_scalar_an_array(name):
    """same parameters in the same order; a `double` of the twin is a `const double *` here, a host result array stays one"""
    _, params = _declaration(name)
    _, twin = _declaration(TWINS[name])
    def split(p):                        # -> (type words, is a pointer or an array, name)
        words, name = p.rsplit(" ", 1)
        return words, "*" in name or "[" in name, name.lstrip("*").split("[")[0]

    assert len(params) == len(twin)
    for p, t in zip(params, twin):
        (pw, pptr, pn), (tw, tptr, tn) = split(p), split(t)
        assert pn == tn, (p, t)
        if tw == "double" and not tptr:
            assert pw == "const double" and pptr, (p, t)
        else:
            assert pw == tw and pptr == tptr, (p, t)


def test_the_aliasing_rules_are_stated_where_the_twin_has_one():
    for name in ("hipkkt_kkt_system_residuals_batch", "hipkkt_kkt_system_solve_batch", "hipkkt_kkt_system_combined_ds_batch",
                 "hipkkt_kkt_system_combined_rhs_batch", "hipkkt_kkt_system_add_step_batch"):
        assert "alias" in _declaration(name)[0], name


def test_the_header_states_the_partition_rules_and_what_stays_joint():
    h = _read("include", "hipkkt.h")
    doc, params = _declaration("hipkkt_kkt_system_set_problems")
    assert params == ["hipkkt_kkt_t h", "int64_t nb", "const int64_t *x_off", "const int64_t *z_off"]
    for word in ("at least one x row", "inside one member", "same member", "HIPKKT_ERR_ARG", "exponential", "side > 48",
                 "hipkkt_kkt_enable_large_psd", "deferred-status", "nb = 0"):
        assert word in doc, word
    block = h[h.index("Level C on a stack of INDEPENDENT problems"):h.index("int hipkkt_kkt_system_set_problems")]
    for word in ("JOINT", "regulariser", "refinement", "status", "no floating-point atomic", "does not depend on nb"):
        assert word in block, word
    assert "alpha[b] == 0 leaves member b's rows bit for bit" in " ".join(_declaration("hipkkt_kkt_system_add_step_batch")[0].split())


def test_the_library_exports_them():
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_the_python_layer_has_the_methods_and_the_loop():
    from cuclarabel_amd import ipm_device
    from cuclarabel_amd.kktsolver import HipKKTSystem
    for meth in ("set_problems", "residuals_batch_dev", "solve_batch_dev", "combined_ds_batch_dev", "step_length_batch_dev",
                 "shift_to_interior_batch_dev", "combined_rhs_batch_dev", "add_step_batch_dev"):
        assert callable(getattr(HipKKTSystem, meth)), meth
    sig = inspect.signature(ipm_device.solve_device_batch)
    assert list(sig.parameters) == ["problems", "settings", "inspect"]
    assert sig.parameters["settings"].default is None and sig.parameters["inspect"].default is None


def test_cone_lists_outside_the_batched_set_are_refused_before_a_handle_is_built():
    import numpy as np
    import scipy.sparse as sp
    from cuclarabel_amd import ipm_device
    from cuclarabel_amd.cones import ExponentialConeT, NonnegativeConeT, PSDTriangleConeT
    P, q = sp.identity(3, format="csc"), np.ones(3)
    ok = (P, q, sp.identity(3, format="csc"), np.ones(3), [NonnegativeConeT(3)])
    with pytest.raises(ValueError, match="ExponentialConeT"):
        ipm_device.solve_device_batch([ok, (P, q, sp.identity(3, format="csc"), np.ones(3), [ExponentialConeT()])])
    A = sp.csc_matrix((49 * 50 // 2, 3))
    with pytest.raises(ValueError, match="side 48"):
        ipm_device.solve_device_batch([ok, (P, q, A, np.zeros(A.shape[0]), [PSDTriangleConeT(49)])])
    with pytest.raises(ValueError, match="at least one"):
        ipm_device.solve_device_batch([])
