"""The ABI surface of the iterate entry points: hipkkt_kkt_system_residuals, _combined_rhs and _add_step are declared and
documented in include/hipkkt.h, and cuclarabel_amd._lib.SYMBOLS binds them with the header's signatures."""
import ctypes as C
import os
import re

import pytest

from cuclarabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hipkkt_kkt_system_residuals", "hipkkt_kkt_system_combined_rhs", "hipkkt_kkt_system_add_step")


def _header():
    return open(os.path.join(ROOT, "include", "hipkkt.h")).read()


def _ctype(param):
    param = param.strip()
    if "*" in param or "[" in param or param.startswith("hipkkt_kkt_t"):
        return C.c_void_p
    return {"double": C.c_double, "int": C.c_int, "int64_t": C.c_int64}[param.split()[-2] if len(param.split()) > 1 else param]


@pytest.mark.parametrize("name", NAMES)
def test_bound_with_the_header_signature_and_documented(name):
    h = _header()
    mt = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + name + r"\s*\(([^;]*)\)\s*;", h, re.S)
    assert mt, f"{name} is not declared behind a comment in include/hipkkt.h"
    doc, params = mt.group(1), [p for p in mt.group(2).replace("\n", " ").split(",")]
    assert len(doc.split()) >= 40, "the header documents the entry point"
    assert re.search(r"\w+\.jl:\d+", doc), "the reference lines it replaces"
    assert re.search(r"synchroni", doc, re.I) and re.search(r"alias", doc, re.I)
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int
    assert list(argtypes) == [_ctype(p) for p in params], (argtypes, params)


def test_the_library_exports_them():
    lib = _lib.lib()
    for name in NAMES:
        assert hasattr(lib, name)


def test_the_python_layer_has_the_three_calls_and_the_plumbing_switch():
    import inspect
    from cuclarabel_amd.ipm_device import solve_device
    from cuclarabel_amd.kktsolver import HipKKTSystem
    for name in ("residuals_dev", "combined_rhs_dev", "add_step_dev"):
        assert callable(getattr(HipKKTSystem, name))
    assert inspect.signature(solve_device).parameters["plumbing"].default == "torch"
