"""CPU tests of the interface of colour frames in the staged stack and of the overlays of a run of frames (srukf_stage_images_bgr / srukf_get_staged_image /
srukf_render_image_overlays): the header declares the three entry points with their signatures, a NULL handle is a bad argument that touches no
output buffer, the Python methods reject wrong arguments before they call the library, the gray rule stands once in csrc/, cslam_vision no longer refuses colour
with block=, and the new device buffers are named in image_group and freed by nobody by hand.  The bytes: tests/test_gpu_images_colour.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_images_cpu import _shell
from test_images_display_cpu import CSRC, ROOT, _body, _code

NAMES = ["srukf_stage_images_bgr", "srukf_get_staged_image", "srukf_render_image_overlays"]


def test_library_exports_and_header_declares(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    ws = lambda s: re.sub(r"\s+", "", s)
    flat = ws(txt)
    for n in NAMES:
        assert hasattr(lib, n), f"libsrukf_hip.so does not export {n}"
        assert n in pkg.srukf.EXPORTS
    assert ws("int srukf_stage_images_bgr(srukf_ctx* ctx, int n_frames, const unsigned char* bgr, int keep_colour);") in flat
    assert ws("int srukf_get_staged_image(srukf_ctx* ctx, int frame, unsigned char* gray_out, unsigned char* bgr_out);") in flat
    assert ws("int srukf_render_image_overlays(srukf_ctx* ctx, int first, int count, unsigned char* out_bgr);") in flat
    assert lib.srukf_abi_version() == 6 and re.search(r"#define\s+SRUKF_ABI_VERSION\s+6\b", txt)      # additions only


def test_null_handle_is_a_bad_argument_and_touches_nothing(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    bp = C.POINTER(C.c_ubyte)
    lib.srukf_stage_images_bgr.argtypes = [C.c_void_p, C.c_int, bp, C.c_int]
    lib.srukf_get_staged_image.argtypes = [C.c_void_p, C.c_int, bp, bp]
    lib.srukf_render_image_overlays.argtypes = [C.c_void_p, C.c_int, C.c_int, bp]
    a, b = (C.c_ubyte * 12)(*range(12)), (C.c_ubyte * 12)(*range(100, 112))
    for F, keep in ((1, 0), (1, 1), (0, 1), (2, 7)):
        assert lib.srukf_stage_images_bgr(None, F, a, keep) == -1
    for frame in (0, -1, 5):
        assert lib.srukf_get_staged_image(None, frame, a, b) == -1
        assert lib.srukf_get_staged_image(None, frame, a, None) == -1
        assert lib.srukf_get_staged_image(None, frame, None, b) == -1
    for first, count in ((0, 1), (-1, 1), (0, 0), (2, 3)):
        assert lib.srukf_render_image_overlays(None, first, count, a) == -1
    assert list(a) == list(range(12)) and list(b) == list(range(100, 112))


def test_python_wrappers_check_their_arguments_before_the_library(pkg):
    f = _shell(pkg)
    H, W = int(f.params.image_h), int(f.params.image_w)
    good = np.zeros((2, H, W, 3), dtype=np.uint8)
    for bad in (good.astype(np.float64), good.astype(np.int8), good.tolist(), None):
        with pytest.raises(TypeError): f.stage_images_bgr(bad)
    for bad in (good[0], good[:, :, :, :2], good[:, :-1], np.zeros((2, H, W), dtype=np.uint8), good[:0]):
        with pytest.raises(ValueError): f.stage_images_bgr(bad)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(TypeError): f.stage_images_bgr(good, keep_colour=bad)
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError): f.get_staged_image(bad)
    with pytest.raises(TypeError): f.get_staged_image(0, want_bgr=1)
    with pytest.raises(ValueError): f.get_staged_image(-1)
    for bad in ((1.0, 1), (0, "2"), (None, 1), (0, True)):
        with pytest.raises(TypeError): f.render_image_overlays(*bad)
    for bad in ((-1, 1), (0, 0)):
        with pytest.raises(ValueError): f.render_image_overlays(*bad)


def test_the_gray_rule_stands_once():
    ov = _code("srukf_overlay.hip")
    assert len(re.findall(r"\bgray_of\s*\([^;{]*\)\s*\{", ov)) == 1
    everything = "".join(_code(fn) for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip", ".cpp")))
    for w in ("4899", "9617", "1868"):
        assert len(re.findall(r"\b" + w + r"u?\b", everything)) == 1, w
    # the stack goes through k_bgr2gray itself: one conversion kernel, and the staging body launches it on chunks that are multiples of four pixels
    assert len(re.findall(r"__global__[^\n]*\bvoid\s+k_bgr2gray\w*\s*\(", ov)) == 1
    stage = _body(_code("srukf_images.hip"), "static int stage_images_any")
    assert "launch_bgr2gray(" in stage
    m = re.search(r"constexpr size_t STAGE_CHUNK = \(size_t\)1 << (\d+);", _code("srukf_images.hip"))
    assert m and int(m.group(1)) >= 2
    # the block launcher is declared once, beside the single-frame ones
    decl = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip"))
            for _ in re.finditer(r"^void\s+launch_overlay_block\s*\([^;{]*\)\s*;", open(os.path.join(CSRC, fn)).read(), flags=re.M)]
    assert decl == ["srukf_ctx.h"], decl
    # both pairs of kernels call one body each
    for kernel, body in (("void k_overlay_prep(", "ov_prep_one("), ("void k_overlay_prep_block(", "ov_prep_one("), ("void k_overlay(", "ov_raster_tile("), ("void k_overlay_block(", "ov_raster_tile(")):
        assert body in _body(ov, kernel), kernel
    assert ov.count("ov_prep_one(") == 3 and ov.count("ov_raster_tile(") == 3
    for head in ("void k_overlay_prep_block(", "void k_overlay_block(", "void ov_raster_tile(", "OvRec ov_prep_one("):
        b = _body(ov, head)
        assert not re.search(r"\batomic\w*\s*\(", b) and not re.search(r"\bwhile\s*\(", b) and "__threadfence" not in b and "volatile" not in b, head
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"srukf_overlay\.o:[^\n]*\n\t[^\n]*-ffp-contract=off", mk)


def test_cslam_vision_takes_colour_with_block():
    txt = open(os.path.join(ROOT, "cv-monoslam_amd", "host", "cslam_vision.cpp")).read()
    refusals = [m.group(0) for m in re.finditer(r'"[^"\n]*block=<F> runs without[^"\n]*"', txt)]
    assert len(refusals) == 1, refusals
    assert "colour" not in refusals[0] and "loops" in refusals[0] and "archive=" in refusals[0]
    assert "SLAMBlockColour" in txt and "colour=2" in txt and "overlays=" in txt
    assert re.search(r'if \(!overlays\.empty\(\) && \(block < 1 \|\| display\.empty\(\)\)\) \{[^}]*return 2;', txt)      # overlays= without block= and display= is refused


def test_the_new_buffers_are_in_image_group_and_nobody_frees_them_by_hand():
    img = _code("srukf_images.hip")
    group = _body(img, "static std::vector<ImageBuf> image_group")
    for name in ("im.bgr", "im.ovs_out", "im.ovs_rec"):
        assert len(re.findall(r"buf\(&" + re.escape(name) + r"\b", group)) == 1, name
    assert len(re.findall(r"case IMG_COLOUR:", img)) == 1 and len(re.findall(r"case IMG_OVERLAYS:", img)) == 1
    drop = _body(img, "void images_drop")
    assert "g < IMG_GROUPS" in drop and "image_buffers_free(image_group(" in drop
    everything = "".join(_code(fn) for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip")))
    for member in ("bgr", "ovs_out", "ovs_rec"):
        assert not re.search(r"(srukf_dfree\w*|hipFree\w*)\s*\([^;]*\b(im|img)\s*\.\s*" + member + r"\b", everything), member
        assert not re.search(r"(srukf_dmalloc\w*|hipMalloc\w*)\s*\([^;]*\b(im|img)\s*\.\s*" + member + r"\b", everything), member
