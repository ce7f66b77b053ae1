"""The data-updating block of level C in include/hipkkt.h (no GPU): its seven symbols are exported by the library,
declared behind comments that cite the reference lines they replace, and bound in cuclarabel_amd/_lib.SYMBOLS with the
header's signatures."""
import ctypes as C
import os
import re

import pytest

from cuclarabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "hipkkt.h")).read()

_P = C.c_void_p
# name -> (the header's parameter list, its ctypes form)
SYMBOLS = {
    "hipkkt_kkt_system_set_equilibration": ("hipkkt_kkt_t h, const double *d, const double *e, double c", [_P, _P, _P, C.c_double]),
    "hipkkt_kkt_system_equilibration_dev": ("hipkkt_kkt_t h, const double **d_d, const double **d_dinv, const double **d_e, "
                                            "const double **d_einv", [_P, _P, _P, _P, _P]),
    "hipkkt_kkt_system_update_data_P": ("hipkkt_kkt_t h, const double *d_values, const int64_t *index, int64_t k",
                                        [_P, _P, _P, C.c_int64]),
    "hipkkt_kkt_system_update_data_A": ("hipkkt_kkt_t h, const double *d_values, const int64_t *index, int64_t k",
                                        [_P, _P, _P, C.c_int64]),
    "hipkkt_kkt_system_update_data_q": ("hipkkt_kkt_t h, const double *d_values, const int64_t *index, int64_t k",
                                        [_P, _P, _P, C.c_int64]),
    "hipkkt_kkt_system_update_data_b": ("hipkkt_kkt_t h, const double *d_values, const int64_t *index, int64_t k",
                                        [_P, _P, _P, C.c_int64]),
    "hipkkt_kkt_system_data_norms": ("hipkkt_kkt_t h, double out[2]", [_P, _P]),
}


def declaration(name):
    """(the comment in front of the declaration -- for a run of declarations, the comment in front of the run --, the
    parameter list with white space collapsed)"""
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", HEADER)
    assert m, f"{name} is not declared in include/hipkkt.h"
    head = HEADER[:m.start()]
    end = head.rfind("*/")
    assert end >= 0
    between = head[end + 2:]
    # only declarations may stand between the comment and this one
    assert re.fullmatch(r"(\s*int\s+hipkkt_\w+\s*\([^;]*\)\s*;)*\s*", between), (name, between[-200:])
    comment = head[head.rfind("/*", 0, end):end]
    return comment, re.sub(r"\s+", " ", m.group(1)).strip()


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_is_exported_declared_and_bound(name):
    params, argtypes = SYMBOLS[name]
    L = C.CDLL(_lib.SO_PATH)
    assert hasattr(L, name), f"libhipkkt.so lacks {name}"
    comment, declared = declaration(name)
    assert declared == params
    assert re.search(r"(data_updating|problemdata)\.jl:\d+", comment), f"the comment in front of {name} cites no reference lines"
    assert name in _lib.SYMBOLS, f"{name} is not bound"
    res, args = _lib.SYMBOLS[name]
    assert res is C.c_int and args == argtypes
    bound = getattr(_lib.lib(), name)
    assert bound.restype is C.c_int and bound.argtypes == argtypes


def test_block_says_what_synchronises_and_how_the_tuple_form_differs():
    start = HEADER.index("Level C: data updating")
    block = HEADER[start:HEADER.index("Level C on a stack of INDEPENDENT problems")]
    for name in SYMBOLS:
        assert name in block, f"{name} is declared outside the data-updating block"
    assert len(re.findall(r"[Ss]ynchronis", block)) >= 3
    assert "data_updating.jl:26-247" in block and "problemdata.jl:91-109" in block
    assert ":208-210" in block and "last bit" in block                # the reference's tuple form multiplies in another order
    assert "HIPKKT_ERR_ARG" in block and "REPEATED" in block


def test_null_handle_is_an_argument_error_everywhere():
    """before any device call: runs without a GPU"""
    L = _lib.lib()
    out = (C.c_double * 2)()
    ptrs = [C.c_void_p() for _ in range(4)]
    assert L.hipkkt_kkt_system_set_equilibration(None, None, None, 1.0) == -1
    assert L.hipkkt_kkt_system_equilibration_dev(None, *[C.byref(p) for p in ptrs]) == -1
    for w in "PAqb":
        assert getattr(L, "hipkkt_kkt_system_update_data_" + w)(None, None, None, 1) == -1
        assert b"null handle" in L.hipkkt_last_error()
    assert L.hipkkt_kkt_system_data_norms(None, out) == -1
