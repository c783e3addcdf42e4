"""CPU tests of the rescue gate (srukf_images_rescue_gate / srukf_get_image_rescue / srukf_rescue_gate): the rule's numpy restatement
(tests/np_rescue.py) against a hand-written table; the library exports the three entry points and refuses NULL handles, bad ranges and bad thresholds before it
touches a device; the header declares them; the launchers are declared once; the gate's body exists as one text that both launch fronts call; a frame of an image run
issues it only with the consensus; the Python methods reject wrong argument types before they call the library.  The kernels: tests/test_gpu_images_rescue.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_rescue
from test_images_cpu import _shell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cv-monoslam_amd", "csrc")
NAMES = ["srukf_images_rescue_gate", "srukf_get_image_rescue", "srukf_rescue_gate"]


def test_rule_against_a_hand_written_table():
    """Seven landmarks, Si' = diag(2, 2) unless noted, so y = (z - h') / 2 and the distance is |z - h'|^2 / 4."""
    chi2 = np_rescue.CHI2
    r = 2.0 * np.sqrt(chi2)                                      # |z - h'| at the threshold, to rounding: the exact case is made below, from the distance the rule forms
    h2 = np.array([[100.0, 100.0]] * 7)
    Si = np.array([[2.0, 0.0, 0.0, 2.0]] * 7)
    z = h2.copy()
    active = np.array([0, 1, 1, 1, 1, 1, 1])
    low = np.array([0, 1, 0, 0, 0, 0, 0])
    vis = np.array([1, 1, 0, 1, 1, 1, 1])
    z[0] += (1.0, 0.0)                                           # 0: not in A
    z[1] += (1.0, 0.0)                                           # 1: a low inlier
    z[2] += (1.0, 0.0)                                           # 2: not visible from the posterior
    Si[3, 0] = 0.0; z[3] += (1.0, 0.0)                           # 3: Si'[0] == 0
    z[4] += (3.0, 0.0)                                           # 4: 9 / 4 = 2.25 < chi2: rescued
    z[5] += (0.0, 6.0)                                           # 5: 36 / 4 = 9 > chi2: not rescued
    z[6] += (r, 0.0)                                             # 6: at the threshold
    flags, dist = np_rescue.gate(z.ravel(), active, low, h2.ravel(), Si, vis)
    assert list(flags[:6]) == [0, 0, 1, 1, 3, 1] and flags[6] & 1 and abs(dist[6] - chi2) < 1e-12
    assert dist[4] == 2.25 and dist[5] == 9.0 and dist[0] == dist[1] == dist[2] == dist[3] == 0.0
    # exactly at the threshold: not rescued, the test is strict (a threshold equal to the distance the rule forms)
    flags_eq, dist_eq = np_rescue.gate(z.ravel(), active, low, h2.ravel(), Si, vis, chi2=float(dist[6]))
    assert dist_eq[6] == dist[6] and flags_eq[6] == 1
    flags_above, _ = np_rescue.gate(z.ravel(), active, low, h2.ravel(), Si, vis, chi2=float(np.nextafter(dist[6], np.inf)))
    assert flags_above[6] == 3
    # the off-diagonal entry takes part by forward substitution: y0 = 1, y1 = (2 - 0.5 * 1) / 3 = 0.5
    f2, d2 = np_rescue.gate([1.0, 2.0, 0.0, 0.0], [1, 1], [0, 1], [0.0, 0.0, 0.0, 0.0], [[1.0, 0.5, 0.0, 3.0], [1.0, 0.0, 0.0, 1.0]], [1, 1])
    assert list(f2) == [3, 0] and d2[0] == 1.25
    # Si'[3] == 0
    f3, _ = np_rescue.gate([1.0, 2.0, 0.0, 0.0], [1, 1], [0, 1], [0.0] * 4, [[1.0, 0.5, 0.0, 0.0], [1.0, 0.0, 0.0, 1.0]], [1, 1])
    assert list(f3) == [1, 0]
    # frames without candidates: n_low == 0, n_low == n_active, fewer than two active matches
    for a, l in (([1, 1, 1], [0, 0, 0]), ([1, 1, 0], [1, 1, 0]), ([1, 0, 0], [0, 0, 0]), ([0, 0, 0], [0, 0, 0])):
        assert not np_rescue.frame_has_candidates(a, l)
        f4, d4 = np_rescue.gate(np.ones(6), a, l, np.zeros(6), [[1.0, 0.0, 0.0, 1.0]] * 3, [1, 1, 1])
        assert not f4.any() and not d4.any()
    assert np_rescue.frame_has_candidates([1, 1, 0], [1, 0, 0])
    assert np_rescue.frame_has_candidates([1, 0, 1], [1, 1, 0])  # (low outside A does not count: n_low = 1 of n_active = 2)


def test_library_exports_and_header_declares(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), f"libsrukf_hip.so does not export {n}"
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), f"include/srukf.h does not declare {n}"
        assert n in pkg.srukf.EXPORTS
    assert re.search(r"srukf_images_rescue_gate\s*\(\s*srukf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*,\s*double\s+chi2\s*\)", txt)
    assert re.search(r"srukf_get_image_rescue\s*\([^)]*int\s*\*\s*flags[^)]*double\s*\*\s*h2[^)]*double\s*\*\s*Si2[^)]*double\s*\*\s*chi2[^)]*int\s*\*\s*n_cand"
                     r"[^)]*int\s*\*\s*n_high[^)]*int\s*\*\s*first_rescue\s*\)", txt)
    assert re.search(r"srukf_rescue_gate\s*\([^)]*const\s+double\s*\*\s*z[^)]*const\s+int\s*\*\s*matched[^)]*const\s+int\s*\*\s*inlier[^)]*double\s+chi2[^)]*int\s*\*\s*flags"
                     r"[^)]*double\s*\*\s*h2[^)]*double\s*\*\s*Si2[^)]*double\s*\*\s*chi2_out[^)]*int\s*\*\s*n_high\s*\)", txt)
    assert re.search(r"#define\s+SRUKF_RESCUE_CANDIDATE\s+1\b", txt) and re.search(r"#define\s+SRUKF_RESCUE_RESCUED\s+2\b", txt)
    assert lib.srukf_abi_version() == 6                          # additions only
    for name in ("images_rescue_gate", "get_image_rescue", "rescue_gate"):
        assert callable(getattr(pkg.srukf.Filter, name))


def test_null_handles_bad_ranges_and_bad_thresholds_are_bad_arguments(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    for chi2 in (5.99, 0.0, -1.0, float("nan"), float("inf")):
        assert lib.srukf_images_rescue_gate(None, 1, chi2) == -1
        assert lib.srukf_images_rescue_gate(None, 0, chi2) == -1
    nul = (None,) * 7
    assert lib.srukf_get_image_rescue(None, 0, 1, *nul) == -1
    assert lib.srukf_get_image_rescue(None, 0, 0, *nul) == -1
    assert lib.srukf_get_image_rescue(None, -1, 1, *nul) == -1
    fr = C.c_int(5)
    assert lib.srukf_get_image_rescue(None, 0, 1, None, None, None, None, None, None, C.byref(fr)) == -1 and fr.value == 5
    z, m = np.zeros(4), np.zeros(2, dtype=np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    nh = C.c_int(7)
    for chi2 in (5.99, float("nan"), -1.0):
        assert lib.srukf_rescue_gate(None, z.ctypes.data_as(dp), m.ctypes.data_as(ip), m.ctypes.data_as(ip), chi2, None, None, None, None, C.byref(nh)) == -1
    assert nh.value == 7


def test_python_wrappers_check_their_arguments_before_the_library(pkg):
    f = _shell(pkg)
    with pytest.raises(ValueError): f.get_image_rescue(-1, 2)
    with pytest.raises(ValueError): f.get_image_rescue(0, 0)
    with pytest.raises(TypeError): f.get_image_rescue(0.0, 2)
    with pytest.raises(TypeError): f.get_image_rescue(0, True)
    call = f.images_rescue_gate
    with pytest.raises(TypeError): call("on")
    with pytest.raises(TypeError): call(2)
    with pytest.raises(TypeError): call(None)
    with pytest.raises(TypeError): call(True, chi2="6")
    with pytest.raises(TypeError): call(True, chi2=True)
    with pytest.raises(TypeError): call(True, chi2=None)
    N = f.N
    with pytest.raises(TypeError): f.rescue_gate(np.zeros(2 * N), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32), chi2="6")
    with pytest.raises(AssertionError): f.rescue_gate(np.zeros(2 * N), np.zeros(N, dtype=np.int32), np.zeros(N + 1, dtype=np.int32))


def _code(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, name)).read())


def test_launchers_are_declared_once_and_both_fronts_share_one_text():
    for name in ("launch_rescue_gate_staged", "launch_rescue_gate", "launch_set_rescue_args"):
        decl = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip"))
                for _ in re.finditer(r"^void\s+" + name + r"\s*\([^;{]*\)\s*;", open(os.path.join(CSRC, fn)).read(), flags=re.M)]
        assert decl == ["srukf_launch.h"], (name, decl)
    txt = _code("srukf_rescue.hip")
    assert len(re.findall(r"\brescue_gate_body\s*\(", txt)) == 3                           # its definition and the two kernels that call it
    for k in ("k_rescue_gate", "k_rescue_gate_staged", "k_rescue_sum_staged"):
        assert len(re.findall(r"__global__[^\n]*\bvoid\s+" + k + r"\s*\(", txt)) == 1, k
    # the body occurs once in the sources: nobody else restates it, and it restates none of the texts it is built from
    others = "".join(_code(fn) for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip")) and fn != "srukf_rescue.hip")
    assert "rescue_gate_body" not in others
    assert len(re.findall(r"\bmeas_final_tail\s*\(", txt)) == 1 and len(re.findall(r"\bsrukf_sigma_feat\s*\(", txt)) == 1
    assert len(re.findall(r"\bsrukf_motion_point\s*\(", txt)) == 1 and len(re.findall(r"\bsrukf_project\s*\(", txt)) == 2      # the centre point and the +/- pair
    assert "sincos" not in txt and "sqrt(" not in txt             # no trigonometry and no Householder step of its own
    # every dependency is a launch boundary: no atomics, no polling loop, no fence for another workgroup to read behind
    dev = txt[:txt.index("#define RQ_ALLOC")]                    # (the device code: the host part behind it has an allocation macro's do-while)
    assert "__global__" in dev and "__global__" not in txt[len(dev):]
    assert not re.search(r"\batomic\w*\s*\(", dev) and not re.search(r"\bwhile\s*\(", dev) and "__threadfence" not in dev and "volatile" not in dev
    assert re.search(r"y0 \* y0 \+ y1 \* y1", txt) and re.search(r"dist < chi2", txt)      # strictly below
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"srukf_rescue\.o:[^\n]*\n\t[^\n]*-ffp-contract=off", mk) and "srukf_rescue.hip" in mk


def test_a_frame_issues_the_gate_only_with_the_consensus_and_in_front_of_the_archive_search():
    img = _code("srukf_images.hip")
    body = img[img.index("static void replay_one_image_frame"):]
    body = body[:body.index("\n}\n")]
    assert body.count("launch_rescue_gate_staged") == 1
    i_tail, i_if, i_gate, i_search = (body.index(s) for s in ("seq_refactor(c, refactor_frame_tail(c), FORM_PLAIN)", "if (form.ransac && form.rescue)",
                                                                "launch_rescue_gate_staged", "if (form.search) seq_archive_search(c)"))
    assert i_tail < i_if < i_gate < i_search
    assert img.count("launch_rescue_gate_staged") == 1           # and nobody else does
    run = img[img.index("static int run_images_issue"):]
    assert re.search(r"c->img_ransac\s*&&\s*c->img_rescue", run)  # the form's bit needs both switches
    assert len(re.findall(r"case IMG_RESCUE:", img)) == 1
    # the snapshot guard reads the gate's summary in the consensus term's place, and only when it is given one
    snap = _code("srukf_snapshot.hip")
    assert re.search(r"rq \? rq\[f - 1\]\.n_high > 0 : rs\[f - 1\]\.outlier != 0", snap)
    ctx = open(os.path.join(CSRC, "srukf_ctx.h")).read()
    assert re.search(r"constexpr int IMAGE_FORM_ROWS = 2 \* IMAGE_FORMS;", ctx)
