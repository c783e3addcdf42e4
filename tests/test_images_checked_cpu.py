"""CPU tests of the checked image runs' interface (srukf_run_images_checked_async / srukf_run_images_checked / srukf_get_image_checks): the library
exports the three entry points and refuses NULL handles and bad counts before it touches a device, the header declares them, the kernel's launcher is declared
once, and the Python methods reject wrong argument types and frame ranges before they call the library (parameter VALUES — ratio, exclusion, threshold — are the
library's to refuse, with SRUKF_ERR_BAD_ARG: tests/test_gpu_images_checked.py).  The numerics are tests/test_gpu_images_checked.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_images_cpu import _shell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srukf_run_images_checked_async", "srukf_run_images_checked", "srukf_get_image_checks"]


def test_library_exports_and_header_declares(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), f"libsrukf_hip.so does not export {n}"
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), f"include/srukf.h does not declare {n}"
        assert n in pkg.srukf.EXPORTS
    assert re.search(r"srukf_run_images_checked\s*\([^)]*const\s+srukf_match_params\s*\*\s*params[^)]*double\s*\*\s*traj_host\s*\)", txt)
    assert lib.srukf_abi_version() == 6                          # additions only


def test_launcher_is_declared_once_and_the_decision_text_is_shared():
    csrc = os.path.join(ROOT, "cv-monoslam_amd", "csrc")
    decl = [fn for fn in sorted(os.listdir(csrc)) if fn.endswith((".h", ".hip"))
            for _ in re.finditer(r"^void\s+srukf_launch_associate_checked_staged\s*\([^;{]*\)\s*;", open(os.path.join(csrc, fn)).read(), flags=re.M)]
    assert decl == ["srukf_launch.h"], decl
    txt = open(os.path.join(csrc, "srukf_unique.hip")).read()
    assert len(re.findall(r"=\s*match_decide\s*\(", txt)) == 2   # k_associate_checked and k_associate_checked_staged: one text of the decisions
    assert len(re.findall(r"corr2\s*>=\s*ma\.ratio\s*\*", txt)) == 1


def test_null_handles_and_bad_counts_are_bad_arguments(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    mp = pkg.srukf.MatchParams(0.8, 0.9, 4, 1)
    for fn in (lib.srukf_run_images_checked_async, lib.srukf_run_images_checked):
        assert fn(None, 0, 1, 1, C.byref(mp), None) == -1
        assert fn(None, 0, 1, 1, None, None) == -1
        assert fn(None, 0, 0, 1, C.byref(mp), None) == -1
        assert fn(None, -1, 1, 2, C.byref(mp), None) == -1
    assert lib.srukf_get_image_checks(None, 0, 1, None, None, None) == -1
    assert lib.srukf_get_image_checks(None, 0, 0, None, None, None) == -1


@pytest.mark.parametrize("method", ["run_images_checked", "run_images_checked_async", "get_image_checks"])
def test_frame_ranges_are_checked_before_the_library(pkg, method):
    f = _shell(pkg)
    call = getattr(f, method)
    with pytest.raises(ValueError): call(-1, 2)
    with pytest.raises(ValueError): call(0, 0)
    with pytest.raises(TypeError): call(0.0, 2)
    with pytest.raises(TypeError): call(0, 2.5)
    with pytest.raises(TypeError): call(0, True)
    if method != "get_image_checks":
        with pytest.raises(TypeError): call(0, 2, mode="joint")


@pytest.mark.parametrize("method", ["run_images_checked", "run_images_checked_async"])
def test_parameter_types_are_checked_before_the_library(pkg, method):
    f = _shell(pkg)
    call = getattr(f, method)
    with pytest.raises(TypeError): call(0, 2, ratio="0.9")
    with pytest.raises(TypeError): call(0, 2, ratio=None)
    with pytest.raises(TypeError): call(0, 2, ratio=True)
    with pytest.raises(TypeError): call(0, 2, corr_threshold=[0.8])
    with pytest.raises(TypeError): call(0, 2, exclusion=4.0)
    with pytest.raises(TypeError): call(0, 2, exclusion=True)
    with pytest.raises(TypeError): call(0, 2, subpixel="yes")
    with pytest.raises(TypeError): call(0, 2, subpixel=2)
    with pytest.raises(ValueError): call(0, 2, exclusion=2 ** 40)


def test_parameter_values_reach_the_library_as_given(pkg):
    """ratio / exclusion / threshold values are not judged in Python: the struct the library gets holds them (the library refuses them, SRUKF_ERR_BAD_ARG)"""
    mp = pkg.srukf.Filter._match_params(np.float32(0.5), float("nan"), np.int64(21), np.bool_(True))
    assert mp.corr_threshold == 0.5 and mp.ratio != mp.ratio and mp.exclusion == 21 and mp.subpixel == 1
    mp = pkg.srukf.Filter._match_params(1, 0, 0, 0)
    assert (mp.corr_threshold, mp.ratio, mp.exclusion, mp.subpixel) == (1.0, 0.0, 0, 0)
