"""CPU tests of the searching image runs' interface (srukf_images_search_archive / srukf_get_image_archive): the library exports the two entry
points and refuses NULL handles and bad counts before it touches a device, the header declares them, the staged search kernel's launcher is declared once, the
search's score exists once (k_archive_search and k_archive_search_staged share one text of the body), and the Python methods reject wrong argument types and frame
ranges before they call the library (parameter VALUES — half_cap, chi2, threshold — are the library's to refuse, with SRUKF_ERR_BAD_ARG:
tests/test_gpu_images_archive.py).  The numerics are tests/test_gpu_images_archive.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_images_cpu import _shell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cv-monoslam_amd", "csrc")
NAMES = ["srukf_images_search_archive", "srukf_get_image_archive"]


def test_library_exports_and_header_declares(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), f"libsrukf_hip.so does not export {n}"
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), f"include/srukf.h does not declare {n}"
        assert n in pkg.srukf.EXPORTS
    assert re.search(r"srukf_images_search_archive\s*\(\s*srukf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*,\s*const\s+srukf_archive_params\s*\*\s*params\s*\)", txt)
    assert re.search(r"srukf_get_image_archive\s*\([^)]*int\s*\*\s*L\s*,[^)]*int\s*\*\s*hits\s*\)", txt)
    assert lib.srukf_abi_version() == 6                          # additions only
    assert re.search(r"#define\s+SRUKF_ABI_VERSION\s+6\b", txt)


def test_launcher_is_declared_once_and_the_search_text_is_shared():
    decl = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip"))
            for _ in re.finditer(r"^void\s+launch_archive_search_staged\s*\([^;{]*\)\s*;", open(os.path.join(CSRC, fn)).read(), flags=re.M)]
    assert decl == ["srukf_launch.h"], decl
    txt = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "srukf_archive.hip")).read())
    assert len(re.findall(r"\(double\)\s*A\s*/\s*sqrt\s*\(", txt)) == 1                    # the score
    assert len(re.findall(r"patch_gate_dist\s*\(", txt)) == 1                              # the gate of the window rule
    assert len(re.findall(r"block_first_max\s*\(", txt)) == 1                              # the first-maximum reduction
    assert len(re.findall(r"\barchive_search_body\s*\(", txt)) == 3                        # its definition and the two kernels that call it
    for k in ("k_archive_search", "k_archive_search_staged"):
        assert len(re.findall(r"__global__[^\n]*\bvoid\s+" + k + r"\s*\(", txt)) == 1, k


def test_null_handles_and_bad_counts_are_bad_arguments(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    ap = pkg.srukf.ArchiveParams(40, 0.8, 5.99146454710798)
    assert lib.srukf_images_search_archive(None, 1, C.byref(ap)) == -1
    assert lib.srukf_images_search_archive(None, 1, None) == -1
    assert lib.srukf_images_search_archive(None, 0, None) == -1
    nul = (None,) * 8
    assert lib.srukf_get_image_archive(None, 0, 1, *nul) == -1
    assert lib.srukf_get_image_archive(None, 0, 0, *nul) == -1
    assert lib.srukf_get_image_archive(None, -1, 1, *nul) == -1


def test_frame_ranges_are_checked_before_the_library(pkg):
    f = _shell(pkg)
    with pytest.raises(ValueError): f.get_image_archive(-1, 2)
    with pytest.raises(ValueError): f.get_image_archive(0, 0)
    with pytest.raises(TypeError): f.get_image_archive(0.0, 2)
    with pytest.raises(TypeError): f.get_image_archive(0, 2.5)
    with pytest.raises(TypeError): f.get_image_archive(0, True)


def test_parameter_types_are_checked_before_the_library(pkg):
    f = _shell(pkg)
    call = f.images_search_archive
    with pytest.raises(TypeError): call("on")
    with pytest.raises(TypeError): call(2)
    with pytest.raises(TypeError): call(1.0)
    with pytest.raises(TypeError): call(None)
    with pytest.raises(TypeError): call(True, half_cap=40.0)
    with pytest.raises(TypeError): call(True, half_cap=True)
    with pytest.raises(TypeError): call(True, half_cap="40")
    with pytest.raises(TypeError): call(True, corr_threshold="0.8")
    with pytest.raises(TypeError): call(True, corr_threshold=None)
    with pytest.raises(TypeError): call(True, corr_threshold=True)
    with pytest.raises(TypeError): call(True, chi2=[5.99])
    with pytest.raises(TypeError): call(False, chi2=False)
    with pytest.raises(ValueError): call(True, half_cap=2 ** 40)


def test_parameter_values_reach_the_library_as_given(pkg):
    """half_cap / threshold / chi2 values are not judged in Python: the struct the library gets holds them (the library refuses them, SRUKF_ERR_BAD_ARG)"""
    ap = pkg.srukf.Filter._archive_params(np.int64(41), np.float32(0.5), float("nan"))
    assert ap.half_cap == 41 and ap.corr_threshold == 0.5 and ap.chi2 != ap.chi2
    ap = pkg.srukf.Filter._archive_params(9, 2, -1)
    assert (ap.half_cap, ap.corr_threshold, ap.chi2) == (9, 2.0, -1.0)
