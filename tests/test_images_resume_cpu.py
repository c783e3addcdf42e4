"""CPU tests of the interface of the state at a block's stop (srukf_images_snapshots / srukf_get_image_snapshots / srukf_images_resume): the library
exports the three entry points and refuses NULL handles and bad ranges before it touches a device, the header declares them, the launchers are declared once, the
snapshot kernel's dependencies are launch boundaries only, and the Python methods reject wrong argument types before they call the library.  The kernel and the
resume against the rewind-and-rerun route: tests/test_gpu_images_resume.py."""
import ctypes as C
import os
import re

import pytest

from test_images_cpu import _shell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cv-monoslam_amd", "csrc")
NAMES = ["srukf_images_snapshots", "srukf_get_image_snapshots", "srukf_images_resume"]


def test_library_exports_and_header_declares(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), f"libsrukf_hip.so does not export {n}"
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), f"include/srukf.h does not declare {n}"
        assert n in pkg.srukf.EXPORTS
    assert re.search(r"srukf_images_snapshots\s*\(\s*srukf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)", txt)
    assert re.search(r"srukf_get_image_snapshots\s*\(\s*srukf_ctx\s*\*\s*ctx\s*,\s*int\s+frames\s*\[\s*2\s*\]\s*\)", txt)
    assert re.search(r"srukf_images_resume\s*\(\s*srukf_ctx\s*\*\s*ctx\s*,\s*int\s+keep\s*\)", txt)
    assert lib.srukf_abi_version() == 6                          # additions only
    assert re.search(r"#define\s+SRUKF_ABI_VERSION\s+6\b", txt)


def test_null_handles_and_bad_ranges_are_bad_arguments(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    lib.srukf_get_image_snapshots.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    for on in (0, 1):
        assert lib.srukf_images_snapshots(None, on) == -1
    tags = (C.c_int * 2)(5, 7)
    assert lib.srukf_get_image_snapshots(None, tags) == -1 and list(tags) == [5, 7]
    assert lib.srukf_get_image_snapshots(None, None) == -1
    for keep in (0, 1, 8, -1):
        assert lib.srukf_images_resume(None, keep) == -1


def test_python_wrappers_check_their_arguments_before_the_library(pkg):
    f = _shell(pkg)
    assert callable(f.images_snapshots) and callable(f.get_image_snapshots) and callable(f.images_resume)
    for bad in ("on", 2, None, 1.0):
        with pytest.raises(TypeError): f.images_snapshots(bad)
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError): f.images_resume(bad)
    with pytest.raises(ValueError): f.images_resume(-1)


def test_launchers_are_declared_once_and_the_kernel_waits_for_nothing():
    for name in ("launch_image_snapshot", "launch_set_snapshot_args"):
        decl = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip"))
                for _ in re.finditer(r"^void\s+" + name + r"\s*\([^;{]*\)\s*;", open(os.path.join(CSRC, fn)).read(), flags=re.M)]
        assert decl == ["srukf_launch.h"], (name, decl)
    txt = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "srukf_snapshot.hip")).read())
    assert len(re.findall(r"__global__[^\n]*\bvoid\s+k_image_snapshot\s*\(", txt)) == 1
    assert re.search(r"__launch_bounds__\(256\)\s*void\s+k_image_snapshot", txt)
    # every dependency is a launch boundary on the stream: no atomics, no polling loop, no fence for another workgroup to read behind
    assert not re.search(r"\batomic\w*\s*\(", txt) and not re.search(r"\bwhile\s*\(", txt) and "__threadfence" not in txt and "volatile" not in txt
    assert re.search(r"\buint4\b", txt)                          # the copy's body moves 16 bytes per lane
    # the host issues it in front of the frame's first launch, and only with the form's bit
    img = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "srukf_images.hip")).read())
    body = img[img.index("static void replay_one_image_frame"):]
    assert 0 < body.index("if (form.snap)") < body.index("launch_image_snapshot") < body.index("seq_predict_motion(c, nullptr)")
    ctx = open(os.path.join(CSRC, "srukf_ctx.h")).read()
    assert re.search(r"constexpr int IMAGE_FORMS = 16;", ctx)
