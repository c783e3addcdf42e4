"""CPU tests of the interface of the display view behind image frames (srukf_images_display / srukf_get_image_display / srukf_render_image_overlay; DESIGN.md
§26): the library exports the three entry points and refuses NULL handles and bad ranges before it touches a device, the header declares them, the launcher is
declared once, k_image_view's dependencies are launch boundaries only and its two bodies are one text each with two callers, the frame forms are untouched, and the
Python methods reject wrong argument types before they call the library.  The record and the overlay against the step-wise getters: tests/test_gpu_images_display.py."""
import ctypes as C
import os
import re

import pytest

from test_images_cpu import _shell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cv-monoslam_amd", "csrc")
NAMES = ["srukf_images_display", "srukf_get_image_display", "srukf_render_image_overlay"]


def _code(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def _body(txt, head):
    """the text of the function whose signature begins with `head`, from its first brace to the matching one"""
    i = txt.index("{", txt.index(head))
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(txt[j], 0)
        if depth == 0: return txt[i:j + 1]
        j += 1


def test_library_exports_and_header_declares(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), f"libsrukf_hip.so does not export {n}"
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), f"include/srukf.h does not declare {n}"
        assert n in pkg.srukf.EXPORTS
    ws = lambda s: re.sub(r"\s+", "", s)
    flat = ws(txt)
    assert ws("srukf_images_display(srukf_ctx* ctx, int on)") in flat
    assert ws("srukf_get_image_display(srukf_ctx* ctx, int first, int count, double* xyz, double* cov, double* axis, double* sigma, int* rot, double* pose4, "
              "double* P4, double* Si)") in flat
    assert ws("srukf_render_image_overlay(srukf_ctx* ctx, int frame, unsigned char* out_bgr)") in flat
    assert lib.srukf_abi_version() == 6                          # additions only
    assert re.search(r"#define\s+SRUKF_ABI_VERSION\s+6\b", txt)
    # each citation names the reference member it stands for
    full = open(os.path.join(ROOT, "include", "srukf.h")).read()
    assert "updateFeaturesInformation" in full and "2566-2575" in full and "display2DFeatureModel" in full and "3009-3051" in full


def test_null_handles_and_bad_ranges_are_bad_arguments(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    lib.srukf_get_image_display.argtypes = [C.c_void_p, C.c_int, C.c_int, dp, dp, dp, dp, ip, dp, dp, dp]
    lib.srukf_render_image_overlay.argtypes = [C.c_void_p, C.c_int, bp]
    for on in (0, 1):
        assert lib.srukf_images_display(None, on) == -1
    buf, rot, img = (C.c_double * 16)(*range(16)), (C.c_int * 4)(5, 6, 7, 8), (C.c_ubyte * 12)(*range(12))
    for first, count in ((0, 1), (-1, 1), (0, 0), (3, -2)):
        assert lib.srukf_get_image_display(None, first, count, buf, None, None, None, rot, None, None, None) == -1
    assert lib.srukf_get_image_display(None, 0, 1, None, None, None, None, None, None, None, None) == -1
    for frame in (0, -1, 7):
        assert lib.srukf_render_image_overlay(None, frame, img) == -1
    assert lib.srukf_render_image_overlay(None, 0, None) == -1
    assert list(buf) == list(range(16)) and list(rot) == [5, 6, 7, 8] and list(img) == list(range(12))


def test_python_wrappers_check_their_arguments_before_the_library(pkg):
    f = _shell(pkg)
    assert callable(f.images_display) and callable(f.get_image_display) and callable(f.render_image_overlay)
    for bad in ("on", 2, None, 1.0):
        with pytest.raises(TypeError): f.images_display(bad)
    for bad in ((1.0, 1), (0, "2"), (None, 1), (0, True)):
        with pytest.raises(TypeError): f.get_image_display(*bad)
    for bad in ((-1, 1), (0, 0)):
        with pytest.raises(ValueError): f.get_image_display(*bad)
    for bad in (1.0, "3", None, True):
        with pytest.raises(TypeError): f.render_image_overlay(bad)
    with pytest.raises(ValueError): f.render_image_overlay(-1)


def test_launcher_is_declared_once_and_the_kernel_waits_for_nothing():
    decl = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip"))
            for _ in re.finditer(r"^void\s+launch_image_view\s*\([^;{]*\)\s*;", open(os.path.join(CSRC, fn)).read(), flags=re.M)]
    assert decl == ["srukf_launch.h"], decl
    txt = _code("srukf_predict.hip")
    assert len(re.findall(r"__global__[^\n]*\bvoid\s+k_image_view\s*\(", txt)) == 1
    assert re.search(r"__launch_bounds__\(256\)\s*void\s+k_image_view", txt)
    # every dependency is a launch boundary on the stream: no atomics, no polling loop, no fence for another workgroup to read behind, in the kernel and in the two
    # bodies it calls
    for head in ("void k_image_view", "void landmark_cartesian_body", "void block_cov_body"):
        body = _body(txt, head)
        assert not re.search(r"\batomic\w*\s*\(", body) and not re.search(r"\bwhile\s*\(", body) and "__threadfence" not in body and "volatile" not in body, head
    # one text, two callers.  The product cph * cth / rho stands twice in the Cartesian body itself (the z row of xyz, and d x / d theta in J), so the count that
    # shows one text is 2; the first row of the Jacobian occurs once
    assert txt.count("cph * cth / rho") == 2
    assert len(re.findall(r"\{\s*1,\s*0,\s*0,\s*cph \* cth / rho", txt)) == 1
    assert txt.count("landmark_cartesian_body(") == 3 and txt.count("block_cov_body(") == 3      # the definition and two callers each
    kv = _body(txt, "void k_image_view")
    assert "landmark_cartesian_body(" in kv and "block_cov_body(" in kv
    assert "landmark_cartesian_body(" in _body(txt, "void k_landmarks_cartesian") and "block_cov_body(" in _body(txt, "void k_block_cov")


def test_the_frame_forms_are_untouched_and_the_display_is_a_property_of_the_run():
    ctx = open(os.path.join(CSRC, "srukf_ctx.h")).read()
    assert re.search(r"constexpr int IMAGE_FORMS = 16;", ctx)
    img = _code("srukf_images.hip")
    frame = _body(img, "static void replay_one_image_frame")
    assert "issue_image_display" not in frame and "launch_image_view" not in frame
    run = _body(img, "static int run_images_issue")
    assert run.count("issue_image_display(c, first") == 3        # the eager first frame, the graph loop, the eager loop
    # display first, then the policy, in all three places
    for m in re.finditer(r"issue_image_display\(c, first[^;]*;", run):
        rest = run[m.end():]
        assert re.match(r"\s*if \(policy\) issue_image_policy\(", rest), rest[:80]
    # the group is named once and freed with the others; the launches sit inside profiling scopes
    assert len(re.findall(r"case IMG_DISPLAY:", img)) == 1
    issue = _body(img, "static void issue_image_display")
    assert issue.count("ProfScope") == 2 and issue.index("launch_image_view") < issue.index("launch_lm_ellipsoid")
    # the two translation units keep their own rounding: no contraction switch on srukf_predict.o, -ffp-contract=off on srukf_display.o
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"srukf_display\.o:[^\n]*\n\t[^\n]*-ffp-contract=off", mk) and not re.search(r"srukf_predict\.o:", mk)
