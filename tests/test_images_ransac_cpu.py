"""CPU tests of the interface of the 1-point RANSAC consensus inside image runs (srukf_images_ransac / srukf_get_image_ransac): the library exports
the two entry points and refuses NULL handles, bad ranges and bad thresholds before it touches a device, the header declares them, the launchers are declared once,
the votes and the pick rule exist as one text that both launch fronts call, and the Python methods reject wrong argument types before they call the library.  The
kernels against the step-wise twin: tests/test_gpu_images_ransac.py."""
import ctypes as C
import os
import re

import pytest

from test_images_cpu import _shell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cv-monoslam_amd", "csrc")
NAMES = ["srukf_images_ransac", "srukf_get_image_ransac"]


def test_library_exports_and_header_declares(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), f"libsrukf_hip.so does not export {n}"
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), f"include/srukf.h does not declare {n}"
        assert n in pkg.srukf.EXPORTS
    assert re.search(r"srukf_images_ransac\s*\(\s*srukf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*,\s*double\s+threshold\s*\)", txt)
    assert re.search(r"srukf_get_image_ransac\s*\([^)]*int\s*\*\s*flags[^)]*int\s*\*\s*votes[^)]*double\s*\*\s*dist[^)]*int\s*\*\s*best[^)]*int\s*\*\s*n_active"
                     r"[^)]*int\s*\*\s*n_low[^)]*int\s*\*\s*first_outlier\s*\)", txt)
    assert re.search(r"#define\s+SRUKF_RANSAC_ACTIVE\s+1\b", txt) and re.search(r"#define\s+SRUKF_RANSAC_INLIER\s+2\b", txt)
    assert lib.srukf_abi_version() == 6                          # additions only
    assert re.search(r"#define\s+SRUKF_ABI_VERSION\s+6\b", txt)


def test_null_handles_bad_ranges_and_bad_thresholds_are_bad_arguments(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    for thr in (8.0, 0.0, -1.0, float("nan"), float("inf")):
        assert lib.srukf_images_ransac(None, 1, thr) == -1
        assert lib.srukf_images_ransac(None, 0, thr) == -1
    nul = (None,) * 7
    assert lib.srukf_get_image_ransac(None, 0, 1, *nul) == -1
    assert lib.srukf_get_image_ransac(None, 0, 0, *nul) == -1
    assert lib.srukf_get_image_ransac(None, -1, 1, *nul) == -1
    fo = C.c_int(5)
    assert lib.srukf_get_image_ransac(None, 0, 1, None, None, None, None, None, None, C.byref(fo)) == -1 and fo.value == 5


def test_python_wrappers_check_their_arguments_before_the_library(pkg):
    f = _shell(pkg)
    assert callable(f.images_ransac) and callable(f.get_image_ransac)
    with pytest.raises(ValueError): f.get_image_ransac(-1, 2)
    with pytest.raises(ValueError): f.get_image_ransac(0, 0)
    with pytest.raises(TypeError): f.get_image_ransac(0.0, 2)
    with pytest.raises(TypeError): f.get_image_ransac(0, True)
    call = f.images_ransac
    with pytest.raises(TypeError): call("on")
    with pytest.raises(TypeError): call(2)
    with pytest.raises(TypeError): call(None)
    with pytest.raises(TypeError): call(True, threshold="8")
    with pytest.raises(TypeError): call(True, threshold=True)
    with pytest.raises(TypeError): call(True, threshold=None)


def test_launchers_are_declared_once_and_both_fronts_share_one_text():
    for name in ("launch_ransac_staged", "launch_set_ransac_args"):
        decl = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip"))
                for _ in re.finditer(r"^void\s+" + name + r"\s*\([^;{]*\)\s*;", open(os.path.join(CSRC, fn)).read(), flags=re.M)]
        assert decl == ["srukf_launch.h"], (name, decl)
    txt = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "srukf_ransac.hip")).read())
    assert len(re.findall(r"\bransac_votes_body\s*\(", txt)) == 3                          # its definition and the two kernels that call it
    assert len(re.findall(r"\bransac_pick_best\s*\(", txt)) == 3
    assert len(re.findall(r"\bsrukf_project\s*\(", txt)) == 1                              # the projection of a pair exists once
    for k in ("k_ransac_votes", "k_ransac_votes_staged", "k_ransac_pick", "k_ransac_pick_staged"):
        assert len(re.findall(r"__global__[^\n]*\bvoid\s+" + k + r"\s*\(", txt)) == 1, k
    assert not re.search(r"\batomic\w*\s*\(", txt)                                         # every dependency is a launch boundary: ballots, shuffles and LDS only
