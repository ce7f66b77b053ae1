"""The ABI surface of the per-member refinement rule: hipkkt_kkt_system_set_member_refinement and
hipkkt_kkt_system_member_refinement_info are exported, declared in include/hipkkt.h each behind a documenting comment
(the reference's lines, what synchronises) and bound in cuclarabel_amd._lib.SYMBOLS with the header's signature; the
header says what the rule covers and what stays joint; the Python layer has the methods and the loop."""
import ctypes as C
import inspect
import os
import re

import pytest

from cuclarabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hipkkt_kkt_system_set_member_refinement", "hipkkt_kkt_system_member_refinement_info"]
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
    assert "kktsolver_directldl.jl:389-449" in doc, "the reference lines it restates"
    assert re.search(r"synchroni", doc, re.I), "what synchronises"
    restype, argtypes = _lib.SYMBOLS[name]
    want = [C.c_void_p if "*" in p else CTYPE[p.replace("const ", "").split()[0]] for p in params]
    assert restype is C.c_int and list(argtypes) == want


def test_the_signatures():
    assert _declaration(NAMES[0])[1] == ["hipkkt_kkt_t h", "int enable"]
    assert _declaration(NAMES[1])[1] == ["hipkkt_kkt_t h", "double *out"]


def test_the_header_says_what_the_rule_covers_and_what_stays_joint():
    doc, _ = _declaration(NAMES[0])
    for word in ("hipkkt_kkt_solve", "hipkkt_kkt_solve_dev", "_solve_constant_rhs", "_solve_initial_point", "_solve_batch",
                 "hipkkt_kkt_system_solve", "2-column pairing", "hipkkt_kkt_solve_multi", "deferred-status", "HIPKKT_ERR_ARG",
                 "without a partition", "expansion rows", "status stays joint", "HIPKKT_NUMERIC_FAILURE",
                 "no floating-point atomic", "bit for bit"):
        assert word in doc, word
    assert re.search(r"[Rr]eplacing or clearing the partition", doc)
    info, _ = _declaration(NAMES[1])
    for word in ("4 nb", "out[4 b ..]", "HIPKKT_ERR_ARG", "one read-back"):
        assert word in info, word
    h = _header()
    block = h[h.index("Level C on a stack of INDEPENDENT problems"):h.index("int hipkkt_kkt_system_set_problems")]
    assert "hipkkt_kkt_system_set_member_refinement" in " ".join(block.split()), "the JOINT paragraph names the way out"


def test_the_library_exports_them():
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), name


def test_the_python_layer_has_the_methods_and_the_loop():
    from cuclarabel_amd import ipm_device
    from cuclarabel_amd.kktsolver import HipKKTSystem
    for meth in ("set_member_refinement", "member_refinement_info"):
        assert callable(getattr(HipKKTSystem, meth)), meth
    sig = inspect.signature(ipm_device.solve_device_batch_refined)
    assert list(sig.parameters) == ["problems", "settings", "inspect"]
    assert sig.parameters["settings"].default is None and sig.parameters["inspect"].default is None
    assert list(inspect.signature(ipm_device.solve_device_batch).parameters) == ["problems", "settings", "inspect"]


def test_the_refined_loop_refuses_what_the_batch_loop_refuses_before_a_handle_is_built():
    import numpy as np
    import scipy.sparse as sp
    from cuclarabel_amd import ipm_device
    from cuclarabel_amd.cones import ExponentialConeT, NonnegativeConeT
    P, q = sp.identity(3, format="csc"), np.ones(3)
    ok = (P, q, sp.identity(3, format="csc"), np.ones(3), [NonnegativeConeT(3)])
    with pytest.raises(ValueError, match="solve_device_batch_refined"):
        ipm_device.solve_device_batch_refined([ok, (P, q, sp.identity(3, format="csc"), np.ones(3), [ExponentialConeT()])])
    with pytest.raises(ValueError, match="at least one"):
        ipm_device.solve_device_batch_refined([])
