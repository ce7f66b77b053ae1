"""The ABI surface of the per-member regulariser and failure status: hipkkt_kkt_system_set_member_status and
hipkkt_kkt_system_member_status are exported, declared in include/hipkkt.h each behind a documenting comment (the
reference's lines, what synchronises, how many launches) and bound in cuclarabel_amd._lib.SYMBOLS with the header's
signature; the header says what is per member now and what stays joint; the Python layer has the methods and the loop,
and the signatures of the two existing batch loops are unchanged."""
import ctypes as C
import inspect
import os
import re

import pytest

from cuclarabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hipkkt_kkt_system_set_member_status", "hipkkt_kkt_system_member_status"]
CTYPE = {"hipkkt_kkt_t": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64, "double": C.c_double}


def _header():
    return open(os.path.join(ROOT, "include", "hipkkt.h")).read()


def _declaration(name):
    """(comment in front of the declaration, [parameter strings])"""
    mt = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", _header(), re.S)
    assert mt, f"{name} is not declared behind a comment in include/hipkkt.h"
    return " ".join(mt.group(1).replace("\n *", " ").split()), [" ".join(p.split()) for p in mt.group(2).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_declared_behind_a_comment_and_bound_with_the_header_signature(name):
    doc, params = _declaration(name)
    assert len(doc.split()) >= 40, "the header documents the entry point"
    assert "kktsolver_directldl.jl:259-310" in doc and "directldl_qdldl.jl:72-81" in doc, "the reference lines it restates"
    assert re.search(r"synchroni", doc, re.I), "what synchronises"
    restype, argtypes = _lib.SYMBOLS[name]
    want = [C.c_void_p if "*" in p else CTYPE[p.replace("const ", "").split()[0]] for p in params]
    assert restype is C.c_int and list(argtypes) == want


def test_the_signatures():
    assert _declaration(NAMES[0])[1] == ["hipkkt_kkt_t h", "int enable"]
    assert _declaration(NAMES[1])[1] == ["hipkkt_kkt_t h", "double *out"]


def test_the_header_says_what_is_per_member_and_what_stays_joint():
    doc, _ = _declaration(NAMES[0])
    for word in ("kktsystem.jl:62-78", "expansion rows", "eps_b", "static_regularization_enable = 0", "hipkkt_kkt_last_regularizer",
                 "largest eps_b", "HIPKKT_NUMERIC_FAILURE", "launches", "whatever nb", "no floating-point atomic", "bit for bit",
                 "HIPKKT_ERR_ARG", "without a partition", "not in an update", "un-regularised"):
        assert word in doc, word
    assert re.search(r"replacing or clearing the partition", doc)
    info, _ = _declaration(NAMES[1])
    for word in ("3 nb", "out[3 b ..]", "HIPKKT_ERR_ARG", "one read-back", "no kernel"):
        assert word in info, word
    h = _header()
    block = " ".join(h[h.index("Level C on a stack of INDEPENDENT problems"):h.index("int hipkkt_kkt_system_set_problems")].split())
    for word in ("JOINT", "hipkkt_kkt_system_set_member_status", "hipkkt_kkt_system_set_member_refinement", "RETURN VALUE",
                 "LP / QP branch", "dynamic regularisations"):
        assert word in block, word


def test_the_library_exports_them():
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_the_python_layer_has_the_methods_and_the_loop():
    from cuclarabel_amd import ipm_device
    from cuclarabel_amd.kktsolver import HipKKTSystem
    for meth in ("set_member_status", "member_status"):
        assert callable(getattr(HipKKTSystem, meth)), meth
    sig = inspect.signature(ipm_device.solve_device_batch_isolated)
    assert list(sig.parameters) == ["problems", "settings", "inspect", "member_refinement"]
    assert sig.parameters["settings"].default is None and sig.parameters["inspect"].default is None
    assert sig.parameters["member_refinement"].default is True
    assert "JOINT" in ipm_device.solve_device_batch_isolated.__doc__, "what a failed solve does without the member rule"
    for loop in (ipm_device.solve_device_batch, ipm_device.solve_device_batch_refined):
        sig = inspect.signature(loop)
        assert list(sig.parameters) == ["problems", "settings", "inspect"]
        assert sig.parameters["settings"].default is None and sig.parameters["inspect"].default is None


def test_the_isolated_loop_refuses_before_a_handle_is_built():
    import numpy as np
    import scipy.sparse as sp
    from cuclarabel_amd import ipm_device
    from cuclarabel_amd.cones import ExponentialConeT, NonnegativeConeT
    eye = lambda: sp.identity(3, format="csc")
    ok = (eye(), np.ones(3), eye(), np.ones(3), [NonnegativeConeT(3)])
    with pytest.raises(ValueError, match="solve_device_batch_isolated"):
        ipm_device.solve_device_batch_isolated([ok, (eye(), np.ones(3), eye(), np.ones(3), [ExponentialConeT()])])
    with pytest.raises(ValueError, match="at least one"):
        ipm_device.solve_device_batch_isolated([])
    q = np.ones(3)
    q[1] = np.nan
    with pytest.raises(ValueError, match=r"member 1 .*non-finite.* q"):
        ipm_device.solve_device_batch_isolated([ok, (eye(), q, eye(), np.ones(3), [NonnegativeConeT(3)])])
    A = eye()
    A.data[0] = np.inf
    with pytest.raises(ValueError, match=r"member 0 .*non-finite.* A"):
        ipm_device.solve_device_batch_isolated([(eye(), np.ones(3), A, np.ones(3), [NonnegativeConeT(3)]), ok])
