"""The ABI surface of the generalized power cones' operations between the solves: the five _gp entry points are declared
and documented in include/hipkkt.h (each behind a comment that cites the lines of coneops_genpowcone.jl it replaces),
cuclarabel_amd._lib.SYMBOLS binds them with the header's signatures, the library exports them, and the Python layer has
the five methods and the loop."""
import ctypes as C
import os
import re

import pytest

from cuclarabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hipkkt_kkt_system_unit_initialization_gp", "hipkkt_kkt_system_affine_ds_gp", "hipkkt_kkt_system_combined_ds_gp",
         "hipkkt_kkt_system_step_length_gp", "hipkkt_kkt_system_barrier_gp")


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
    assert re.search(r"coneops_genpowcone\.jl:\d+-\d+", doc), "the reference lines it replaces"
    assert re.search(r"synchroni", doc, re.I) and re.search(r"alias", doc, re.I)
    restype, argtypes = _lib.SYMBOLS[name]
    assert restype is C.c_int
    assert list(argtypes) == [_ctype(p) for p in params], (argtypes, params)
    # the same signature as the counterpart without generalized power cones
    twin = name[:-3] if name.endswith(("unit_initialization_gp", "barrier_gp")) else name[:-3] + "_ns"
    assert list(_lib.SYMBOLS[twin][1]) == list(argtypes)


def test_the_library_exports_them():
    lib = _lib.lib()
    for name in NAMES:
        assert hasattr(lib, name)


def test_the_python_layer_has_the_five_calls_and_the_loop():
    import inspect
    from cuclarabel_amd import ipm_device
    from cuclarabel_amd.kktsolver import HipKKTSystem
    for name in ("unit_initialization_gp_dev", "affine_ds_gp_dev", "combined_ds_gp_dev", "step_length_gp_dev", "barrier_gp_dev"):
        assert callable(getattr(HipKKTSystem, name))
        twin = name.replace("_gp_dev", "_dev") if name.startswith(("unit", "barrier")) else name.replace("_gp_dev", "_ns_dev")
        assert list(inspect.signature(getattr(HipKKTSystem, name)).parameters) == \
            list(inspect.signature(getattr(HipKKTSystem, twin)).parameters)
    sig = inspect.signature(ipm_device.solve_device_genpow)
    assert list(sig.parameters) == ["P", "q", "A", "b", "cone_specs", "settings", "inspect", "plumbing"]
    assert sig.parameters["plumbing"].default == "device"
