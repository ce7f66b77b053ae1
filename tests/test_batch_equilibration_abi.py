"""The ABI surface of the member cost scalings: hipkkt_kkt_system_set_equilibration_batch and
hipkkt_kkt_system_data_norms_batch are declared in include/hipkkt.h each behind a documenting comment, exported by the
library and bound in cuclarabel_amd._lib.SYMBOLS with the header's signature; the header states the rule of the P and q
updates under member costs; the Python layer has the methods, the loop's argument and the resident class."""
import ctypes as C
import inspect
import os
import re

import pytest

from cuclarabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hipkkt_kkt_system_set_equilibration_batch", "hipkkt_kkt_system_data_norms_batch"]
CTYPE = {"hipkkt_kkt_t": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}


def _header():
    return open(os.path.join(ROOT, "include", "hipkkt.h")).read()


def _declaration(name):
    """(comment in front of the declaration, [parameter strings])"""
    mt = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", _header(), re.S)
    assert mt, f"{name} is not declared behind a comment in include/hipkkt.h"
    return " ".join(mt.group(1).replace("*", " ").split()), [" ".join(p.split()) for p in mt.group(2).split(",")]


def _argtypes(params):
    return [C.c_void_p if "*" in p else CTYPE[p.replace("const ", "").split()[0]] for p in params]


@pytest.mark.parametrize("name", NAMES)
def test_declared_behind_a_comment_and_bound_with_the_header_signature(name):
    doc, params = _declaration(name)
    assert len(doc.split()) >= 40, "the header documents the entry point"
    assert re.search(r"problemdata\.jl:\d+", doc), "the reference lines it replaces"
    assert re.search(r"synchroni", doc, re.I), "what synchronises"
    assert "deferred-status" in doc and "partition" in doc
    assert name in _lib.SYMBOLS, f"{name} is not bound in _lib.SYMBOLS"
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int and list(argtypes) == _argtypes(params)


def test_the_argument_lists():
    assert _declaration(NAMES[0])[1] == ["hipkkt_kkt_t h", "const double *d", "const double *e", "const double *c"]
    assert _declaration(NAMES[1])[1] == ["hipkkt_kkt_t h", "double *out"]


def test_the_header_states_the_rules():
    doc, _ = _declaration(NAMES[0])
    for word in ("HIPKKT_ERR_ARG", "finite and > 0", "nothing derived", "left alone", "one joint c",
                 "hipkkt_kkt_system_set_problems is refused"):
        assert word in doc, word
    doc, _ = _declaration(NAMES[1])
    for word in ("out[2 b]", "out[2 b + 1]", "atomicMax", "no floating-point atomic", "NaN", "One launch", "without z rows"):
        assert word in doc, word
    upd, _ = _declaration("hipkkt_kkt_system_update_data_P")
    assert "carry no per-member scalar" not in upd
    for word in ("hipkkt_kkt_system_set_equilibration_batch", "owns the entry's row", "_A and _b carry no c"):
        assert word in upd, word
    assert "holds member cost scalings" in _declaration("hipkkt_kkt_system_set_problems")[0]


def test_the_library_exports_them():
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_the_python_layer_has_the_methods_the_loop_and_the_resident_class():
    from cuclarabel_amd import ipm_device, solver_device
    from cuclarabel_amd.kktsolver import HipKKTSystem
    for meth in ("set_equilibration_batch", "data_norms_batch"):
        assert callable(getattr(HipKKTSystem, meth)), meth
    sig = inspect.signature(ipm_device._solve_batch)
    assert list(sig.parameters)[:6] == ["who", "problems", "settings", "inspect", "member_refinement", "isolate"]
    assert sig.parameters["equilibrations"].default is None
    assert callable(ipm_device._setup_batch) and callable(ipm_device._loop_batch)
    sig = inspect.signature(solver_device.DeviceBatchSolver.__init__)
    assert list(sig.parameters) == ["self", "problems", "settings", "equilibrate", "equilibrations", "member_refinement", "isolate"]
    p = sig.parameters
    assert (p["settings"].default, p["equilibrate"].default, p["equilibrations"].default, p["member_refinement"].default,
            p["isolate"].default) == (None, True, None, True, True)
    for meth in ("solve", "update_data", "update_data_stack"):
        assert callable(getattr(solver_device.DeviceBatchSolver, meth)), meth


def test_cone_lists_outside_the_batched_set_are_refused_before_a_handle_is_built():
    import numpy as np
    import scipy.sparse as sp
    from cuclarabel_amd.solver_device import DeviceBatchSolver
    from cuclarabel_amd.cones import ExponentialConeT, NonnegativeConeT, PSDTriangleConeT
    P, q = sp.identity(3, format="csc"), np.ones(3)
    ok = (P, q, sp.identity(3, format="csc"), np.ones(3), [NonnegativeConeT(3)])
    with pytest.raises(ValueError, match="ExponentialConeT"):
        DeviceBatchSolver([ok, (P, q, sp.identity(3, format="csc"), np.ones(3), [ExponentialConeT()])])
    A = sp.csc_matrix((49 * 50 // 2, 3))
    with pytest.raises(ValueError, match="side 48"):
        DeviceBatchSolver([ok, (P, q, A, np.zeros(A.shape[0]), [PSDTriangleConeT(49)])])
    with pytest.raises(ValueError, match="at least one"):
        DeviceBatchSolver([])
