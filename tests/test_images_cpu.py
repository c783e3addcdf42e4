"""CPU tests of the image runs of the staged replay (srukf_stage_images / srukf_run_images_async / srukf_run_images / srukf_get_image_matches): the
library exports the four entry points and refuses NULL handles and bad counts before it touches a device, and the Python methods reject wrong shapes and dtypes
before they call the library.  The numerics are tests/test_gpu_images.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["srukf_stage_images", "srukf_run_images_async", "srukf_run_images", "srukf_get_image_matches"]


def test_library_exports_and_header_declares(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), f"libsrukf_hip.so does not export {n}"
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), f"include/srukf.h does not declare {n}"
        assert n in pkg.srukf.EXPORTS
    assert lib.srukf_abi_version() == 6                          # additions only


def test_null_handles_and_bad_counts_are_bad_arguments(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    img = (C.c_ubyte * 16)()
    assert lib.srukf_stage_images(None, 1, img) == -1
    assert lib.srukf_stage_images(None, 0, None) == -1
    for fn in (lib.srukf_run_images_async, lib.srukf_run_images):
        assert fn(None, 0, 1, 1, None) == -1
        assert fn(None, 0, 0, 1, None) == -1
        assert fn(None, -1, 1, 2, None) == -1
    assert lib.srukf_get_image_matches(None, 0, 1, None, None, None, None, None) == -1
    assert lib.srukf_get_image_matches(None, 0, 0, None, None, None, None, None) == -1


class _NoLibrary:
    """stands where Filter keeps the library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) with arguments the method must reject")


def _shell(pkg, N=8):
    """a Filter that never met a device: what the argument checks read, and a library that must not be reached"""
    f = pkg.srukf.Filter.__new__(pkg.srukf.Filter)
    f.params = pkg.srukf.Params.from_dict(pkg.synth.scene_params())
    f.N, f.n = N, 6 * N + 4
    f._lib, f._h = _NoLibrary(), None
    return f


def test_stage_images_rejects_wrong_shapes_and_dtypes(pkg):
    f = _shell(pkg)
    with pytest.raises(TypeError): f.stage_images(np.zeros((2, 480, 640), dtype=np.float64))
    with pytest.raises(TypeError): f.stage_images([[0]])
    with pytest.raises(ValueError): f.stage_images(np.zeros((480, 640), dtype=np.uint8))
    with pytest.raises(ValueError): f.stage_images(np.zeros((2, 640, 480), dtype=np.uint8))
    with pytest.raises(ValueError): f.stage_images(np.zeros((0, 480, 640), dtype=np.uint8))


@pytest.mark.parametrize("method", ["run_images", "run_images_async", "get_image_matches"])
def test_frame_ranges_are_checked_before_the_library(pkg, method):
    f = _shell(pkg)
    call = getattr(f, method)
    with pytest.raises(ValueError): call(-1, 2)
    with pytest.raises(ValueError): call(0, 0)
    with pytest.raises(TypeError): call(0.0, 2)
    with pytest.raises(TypeError): call(0, 2.5)
    with pytest.raises(TypeError): call(0, True)
    if method != "get_image_matches":
        with pytest.raises(TypeError): call(0, 2, mode="joint")
