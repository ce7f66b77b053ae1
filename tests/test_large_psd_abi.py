"""The ABI surface of the large-PSD opt-in: hipkkt_kkt_enable_large_psd is exported, declared in include/hipkkt.h behind a
comment that cites the reference's lines and states the limit, and bound in cuclarabel_amd._lib.SYMBOLS with the
header's signature; the header's HIPKKT_PSD_MAX_SIDE_LARGE is 96 and the kernels' constant agrees with it."""
import ctypes as C
import inspect
import os
import re

import pytest

from cuclarabel_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "hipkkt_kkt_enable_large_psd"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_declared_behind_a_comment_and_bound_with_the_header_signature():
    h = _read("include", "hipkkt.h")
    mt = re.search(r"/\*((?:(?!\*/).)*)\*/\s*#define\s+HIPKKT_PSD_MAX_SIDE_LARGE\s+(\d+)\s*int\s+" + NAME +
                   r"\s*\(([^;]*)\)\s*;", h, re.S)
    assert mt, f"{NAME} is not declared behind a comment and the limit's #define in include/hipkkt.h"
    doc, limit, params = mt.group(1), int(mt.group(2)), [p.strip() for p in mt.group(3).split(",")]
    assert limit == 96
    assert len(doc.split()) >= 40, "the header documents the entry point"
    assert re.search(r"coneops_psdtrianglecone\.jl:\d+", doc), "the reference lines it replaces"
    assert "147 456" in doc and "160 KiB" in doc, "the limit's derivation"
    assert re.search(r"synchroni", doc, re.I)
    assert params == ["hipkkt_kkt_t h", "int enable"]
    restype, argtypes = _lib.SYMBOLS[NAME]
    assert restype is C.c_int and list(argtypes) == [C.c_void_p, C.c_int]


def test_the_library_exports_it():
    assert hasattr(_lib.lib(), NAME)


def test_the_kernels_limit_is_the_headers():
    hpp = _read("cuclarabel_amd", "csrc", "kernels.hpp")
    assert re.search(r"constexpr\s+int\s+kPsdBigMaxDim\s*=\s*96\s*;", hpp)
    # (the small class's limit lives where host-only code sees it too; kernels.hpp includes that header)
    shapes = _read("cuclarabel_amd", "csrc", "launch_shapes.hpp")
    assert re.search(r'#include\s+"launch_shapes.hpp"', hpp)
    assert re.search(r"constexpr\s+int\s+kPsdMaxDim\s*=\s*48\s*;", shapes), "the all-in-LDS class keeps its limit"
    assert len(re.findall(r"constexpr\s+int\s+kPsdMaxDim\b", hpp + shapes)) == 1


def test_the_python_layer_has_the_switch_and_defaults_to_off():
    from cuclarabel_amd.kktsolver import HipKKTSolver
    assert callable(HipKKTSolver.enable_large_psd)
    assert inspect.signature(HipKKTSolver.__init__).parameters["large_psd"].default is False
    assert inspect.signature(HipKKTSolver.enable_large_psd).parameters["enable"].default is True


def test_ipm_device_limits_agree_with_the_header():
    from cuclarabel_amd import ipm_device
    from cuclarabel_amd.cones import PSDTriangleConeT
    limit = int(re.search(r"#define\s+HIPKKT_PSD_MAX_SIDE_LARGE\s+(\d+)", _read("include", "hipkkt.h")).group(1))
    assert ipm_device.PSD_MAX_SIDE_LARGE == limit == 96 and ipm_device.PSD_MAX_SIDE == 48
    allowed = (PSDTriangleConeT,)
    assert ipm_device._check_cones("solve_device", [PSDTriangleConeT(96)], allowed, "{}")[0].dim == 96
    with pytest.raises(ValueError, match="up to side 96"):
        ipm_device._check_cones("solve_device", [PSDTriangleConeT(97)], allowed, "{}")
    assert inspect.signature(__import__("cuclarabel_amd.ipm", fromlist=["x"]).HipSystemBackend.__init__).parameters[
        "large_psd"].default is False


def test_the_hs_launch_spreads_a_big_cone_over_many_workgroups():
    """by construction: k_psd_hs_big is launched over a (chunks, big cones) grid with more than one chunk, from the scaling
    and from a caller's scaling alike"""
    src = _read("cuclarabel_amd", "csrc", "kernels.hip")
    chunks = int(re.search(r"constexpr\s+int\s+kPsdBigHsChunks\s*=\s*(\d+)\s*;", src).group(1))
    assert chunks > 1
    launches = re.findall(r"hipLaunchKernelGGL\(k_psd_hs_big,\s*dim3\(([^)]*)\)", src)
    assert len(launches) == 2 and all(re.fullmatch(r"kPsdBigHsChunks,\s*C\.npsdb", a.strip()) for a in launches), launches
    assert re.search(r"col = blockIdx\.x; col < t; col \+= gridDim\.x", src), "the columns are dealt over the chunks"
