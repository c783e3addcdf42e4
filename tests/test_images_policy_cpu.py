"""CPU tests of the map policy's interface (srukf_map_policy / srukf_images_policy / srukf_images_set_policy_state / srukf_get_image_policy / srukf_images_rewind;
DESIGN.md §23): the library exports the five entry points and refuses NULL handles and bad ranges before it touches a device, the header declares them, the
launchers are declared once and the two kernels share one text of the body, the Python methods reject wrong argument types before they call the library — and the
numpy restatement (tests/np_policy.py) is held to a hand-written table: one case per verdict bit, the three STORE branches, the stale predictLocation of an
invisible landmark, need_add at min_matches and at min_matches - 1.  The table tests exercise tests/np_policy.py alone; the checks that need the library and
the binding of this change are the exports, the struct layouts, the launcher declarations, the refusals and the argument checks.  The kernel against the
restatement: tests/test_gpu_policy.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_policy as P
from test_images_cpu import _shell

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cv-monoslam_amd", "csrc")
NAMES = ["srukf_map_policy", "srukf_images_policy", "srukf_images_set_policy_state", "srukf_get_image_policy", "srukf_images_rewind"]
W, H = 640.0, 480.0


def test_library_exports_and_header_declares(pkg):
    lib = pkg.srukf.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srukf.h")).read(), flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), f"libsrukf_hip.so does not export {n}"
        assert re.search(r"\bint\s+" + n + r"\s*\(", txt), f"include/srukf.h does not declare {n}"
        assert n in pkg.srukf.EXPORTS
    assert re.search(r"srukf_images_policy\s*\(\s*srukf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*,\s*const\s+srukf_policy_params\s*\*\s*params\s*\)", txt)
    assert re.search(r"srukf_get_image_policy\s*\([^)]*int\s*\*\s*first_change\s*\)", txt)
    assert re.search(r"#define\s+SRUKF_POLICY_DEFAULTS\s*\{\s*20\.0\s*,\s*0\.01\s*,\s*10\s*,\s*5\s*\}", txt)
    assert lib.srukf_abi_version() == 6                          # additions only
    assert re.search(r"#define\s+SRUKF_ABI_VERSION\s+6\b", txt)


def test_structs_match_the_header(pkg):
    s = pkg.srukf
    assert C.sizeof(s.PolicyParams) == 24 and C.sizeof(s.PolicySummary) == 32
    assert s.POLICY_STATE_DTYPE.itemsize == 24 and s.POLICY_SUMMARY_DTYPE.itemsize == 32
    assert s.POLICY_STATE_DTYPE == P.STATE_DTYPE and tuple(s.POLICY_SUMMARY_FIELDS) == P.SUMMARY_FIELDS
    assert (s.POLICY_UNMATCHED, s.POLICY_RHO, s.POLICY_BEHIND, s.POLICY_PRED_BORDER, s.POLICY_MATCH_BORDER, s.POLICY_STORE) == (1, 2, 4, 8, 16, 32)
    txt = open(os.path.join(ROOT, "include", "srukf.h")).read()
    for name, bit in (("UNMATCHED", 1), ("RHO", 2), ("BEHIND", 4), ("PRED_BORDER", 8), ("MATCH_BORDER", 16), ("STORE", 32)):
        assert re.search(r"#define\s+SRUKF_POLICY_" + name + r"\s+" + str(bit) + r"\b", txt), name


def test_launchers_are_declared_once_and_the_policy_text_is_shared():
    for name in ("launch_map_policy", "launch_map_policy_staged", "launch_set_policy_params"):
        decl = [fn for fn in sorted(os.listdir(CSRC)) if fn.endswith((".h", ".hip"))
                for _ in re.finditer(r"^void\s+" + name + r"\s*\([^;{]*\)\s*;", open(os.path.join(CSRC, fn)).read(), flags=re.M)]
        assert decl == ["srukf_launch.h"], (name, decl)
    txt = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "srukf_policy.hip")).read())
    assert len(re.findall(r"\bmap_policy_body\s*\(", txt)) == 3                            # its definition and the two kernels that call it
    assert len(re.findall(r"cos\s*\(\s*phi\s*\)\s*\*\s*cos\s*\(\s*theta\s*\)", txt)) == 1  # the BEHIND test exists once
    for k in ("k_map_policy", "k_map_policy_staged"):
        assert len(re.findall(r"__global__[^\n]*\bvoid\s+" + k + r"\s*\(", txt)) == 1, k
    assert not re.search(r"\batomic\w*\s*\(", txt)                                         # reductions by shuffles and LDS only


def test_null_handles_and_bad_ranges_are_bad_arguments(pkg):
    """no device is touched: this runs on a machine without one"""
    lib = pkg.srukf.load_library()
    pp = pkg.srukf.PolicyParams(20.0, 0.01, 10, 5)
    assert lib.srukf_images_policy(None, 1, C.byref(pp)) == -1
    assert lib.srukf_images_policy(None, 1, None) == -1
    assert lib.srukf_images_policy(None, 0, None) == -1
    assert lib.srukf_images_set_policy_state(None, None) == -1
    st = P.zero_state(4)
    assert lib.srukf_images_set_policy_state(None, st.ctypes.data_as(C.c_void_p)) == -1
    assert lib.srukf_images_rewind(None) == -1
    nul = (None,) * 4
    assert lib.srukf_get_image_policy(None, 0, 1, *nul) == -1
    assert lib.srukf_get_image_policy(None, 0, 0, *nul) == -1
    assert lib.srukf_get_image_policy(None, -1, 1, *nul) == -1
    assert lib.srukf_map_policy(None, None, None, None, None, None, None, None, None) == -1
    assert lib.srukf_map_policy(None, C.byref(pp), st.ctypes.data_as(C.c_void_p), None, None, None, None, None, None) == -1


def test_argument_types_and_ranges_are_checked_before_the_library(pkg):
    f = _shell(pkg)
    with pytest.raises(ValueError): f.get_image_policy(-1, 2)
    with pytest.raises(ValueError): f.get_image_policy(0, 0)
    with pytest.raises(TypeError): f.get_image_policy(0.0, 2)
    with pytest.raises(TypeError): f.get_image_policy(0, True)
    call = f.images_policy
    with pytest.raises(TypeError): call("on")
    with pytest.raises(TypeError): call(2)
    with pytest.raises(TypeError): call(None)
    with pytest.raises(TypeError): call(True, border="20")
    with pytest.raises(TypeError): call(True, border=True)
    with pytest.raises(TypeError): call(True, rho_min=None)
    with pytest.raises(TypeError): call(True, min_predictions=10.0)
    with pytest.raises(TypeError): call(True, min_matches=True)
    with pytest.raises(ValueError): call(True, min_matches=2 ** 40)
    with pytest.raises(ValueError): f.set_policy_state(P.zero_state(7))                    # N = 8
    with pytest.raises(ValueError): f.map_policy(P.zero_state(8), np.zeros(15), np.zeros(8), np.zeros(16), np.zeros(8))
    pp = pkg.srukf.Filter._policy_params(np.float32(70), float("nan"), np.int64(3), 0)     # values are the library's to judge
    assert pp.border == 70.0 and pp.rho_min != pp.rho_min and (pp.min_predictions, pp.min_matches) == (3, 0)


# ---- the restatement against a hand-written table ----
def _scene(N=6):
    """N landmarks in front of the camera (theta = phi = 0, rho = 0.5, zi = 0; robot z = 0: Hlr_z = 1), predicted and matched mid-image"""
    X = np.zeros(6 * N + 4)
    X[5::6][:N] = 0.5
    st = P.zero_state(N)
    st["predictLocation"] = (320.0, 240.0)
    h = np.tile([320.0, 240.0], N)
    z = np.tile([321.0, 239.0], N)
    return X, st, h, np.ones(N, dtype=np.int32), z, np.ones(N, dtype=np.int32)


def _run(X, st, h, vis, z, m, **kw):
    return P.policy(st, X, h, vis, z, m, W, H, **kw)


def test_table_clean_frame():
    v, s, st = _run(*_scene())
    assert v.tolist() == [0] * 6
    assert s == dict(n_predicts=6, n_matches=6, n_deletes=0, n_stores=0, n_predicts_after=6, n_matches_after=6, need_add=0, change=0)
    assert st["nPredictTimes"].tolist() == [1] * 6 and st["nMatchTimes"].tolist() == [1] * 6
    assert st["predictLocation"].tolist() == [[320.0, 240.0]] * 6


def test_table_one_case_per_bit():
    # UNMATCHED: 9 predictions and 4 matches before; visible and not matched now: 10 > 8 and 10 >= 10
    X, st, h, vis, z, m = _scene()
    st["nPredictTimes"][1], st["nMatchTimes"][1] = 9, 4
    m[1] = 0
    v, s, st2 = _run(X, st, h, vis, z, m)
    assert v.tolist() == [0, P.UNMATCHED, 0, 0, 0, 0] and (st2["nPredictTimes"][1], st2["nMatchTimes"][1]) == (10, 4)
    assert (s["n_predicts"], s["n_matches"], s["n_deletes"], s["n_stores"], s["n_predicts_after"], s["n_matches_after"], s["need_add"], s["change"]) == (6, 5, 1, 0, 5, 5, 0, 1)
    # ... one prediction short of min_predictions: 9 > 8 but 9 < 10
    st["nPredictTimes"][1] = 8
    assert _run(X, st, h, vis, z, m)[0].tolist() == [0] * 6
    # ... and matched now: 10 > 10 is false
    st["nPredictTimes"][1] = 9
    m[1] = 1
    assert _run(X, st, h, vis, z, m)[0].tolist() == [0] * 6
    # RHO
    X, st, h, vis, z, m = _scene()
    X[6 * 2 + 5] = 0.009
    assert _run(X, st, h, vis, z, m)[0].tolist() == [0, 0, P.RHO, 0, 0, 0]
    X[6 * 2 + 5] = 0.011
    assert _run(X, st, h, vis, z, m)[0].tolist() == [0] * 6
    # BEHIND: theta + pi turns the ray round, cos(phi) cos(theta) = -1; rho (zi - zr) = 0.5 * (0 - 0)
    X, st, h, vis, z, m = _scene()
    X[6 * 3 + 3] = np.pi
    assert _run(X, st, h, vis, z, m)[0].tolist() == [0, 0, 0, P.BEHIND, 0, 0]
    # ... the robot's z enters: rho (zi - zr) = 0.5 * (0 - 3) = -1.5 < -1
    X, st, h, vis, z, m = _scene()
    X[-2] = 3.0
    assert _run(X, st, h, vis, z, m)[0].tolist() == [P.BEHIND] * 6
    # PRED_BORDER (not matched: no store), each edge
    for px, py in ((19.0, 240.0), (320.0, 19.5), (640.0 - 19.0, 240.0), (320.0, 480.0 - 19.9)):
        X, st, h, vis, z, m = _scene()
        h[8:10] = (px, py)
        m[4] = 0
        v, s, _ = _run(X, st, h, vis, z, m)
        assert v.tolist() == [0, 0, 0, 0, P.PRED_BORDER, 0] and (s["n_deletes"], s["n_stores"], s["n_predicts_after"], s["n_matches_after"]) == (1, 0, 5, 5)
    # exactly `border` from an edge is not within it (px < border)
    X, st, h, vis, z, m = _scene()
    h[8:10] = (20.0, 460.0)
    assert _run(X, st, h, vis, z, m)[0].tolist() == [0] * 6
    # MATCH_BORDER needs a match: the same pixel unmatched raises nothing
    X, st, h, vis, z, m = _scene()
    z[10:12] = (630.0, 240.0)
    assert _run(X, st, h, vis, z, m)[0].tolist() == [0, 0, 0, 0, 0, P.MATCH_BORDER | P.STORE]
    m[5] = 0
    assert _run(X, st, h, vis, z, m)[0].tolist() == [0] * 6


def test_table_the_three_store_branches():
    # (a) a hard reason: never stored, whatever the borders say (cslam.cpp:460)
    X, st, h, vis, z, m = _scene()
    X[5] = 0.001
    h[0:2] = (5.0, 240.0)
    z[0:2] = (5.0, 240.0)
    v, s, _ = _run(X, st, h, vis, z, m)
    assert v[0] == P.RHO | P.PRED_BORDER | P.MATCH_BORDER and (s["n_deletes"], s["n_stores"], s["n_predicts_after"], s["n_matches_after"]) == (1, 0, 5, 6)
    # (b) PRED_BORDER: stored only with a match (cslam.cpp:461)
    X, st, h, vis, z, m = _scene()
    h[0:2] = (5.0, 240.0)
    v, s, _ = _run(X, st, h, vis, z, m)
    assert v[0] == P.PRED_BORDER | P.STORE and (s["n_deletes"], s["n_stores"], s["n_predicts_after"], s["n_matches_after"]) == (1, 1, 5, 5)
    m[0] = 0
    v, s, _ = _run(X, st, h, vis, z, m)
    assert v[0] == P.PRED_BORDER and (s["n_deletes"], s["n_stores"], s["n_matches"], s["n_matches_after"]) == (1, 0, 5, 5)
    # (c) MATCH_BORDER alone: stored (cslam.cpp:462)
    X, st, h, vis, z, m = _scene()
    z[0:2] = (321.0, 470.0)
    v, s, _ = _run(X, st, h, vis, z, m)
    assert v[0] == P.MATCH_BORDER | P.STORE and (s["n_deletes"], s["n_stores"], s["n_predicts_after"], s["n_matches_after"]) == (1, 1, 5, 5)


def test_table_stale_predict_location_of_an_invisible_landmark():
    X, st, h, vis, z, m = _scene()
    st["predictLocation"][2] = (10.0, 240.0)                    # where it was last predicted: at the border
    st["nPredictTimes"][2], st["nMatchTimes"][2] = 3, 3
    vis[2] = 0
    m[2] = 0
    h[4:6] = (320.0, 240.0)                                     # this frame's h is not taken
    v, s, st2 = _run(X, st, h, vis, z, m)
    assert v.tolist() == [0, 0, P.PRED_BORDER, 0, 0, 0]
    assert st2["predictLocation"][2].tolist() == [10.0, 240.0] and (st2["nPredictTimes"][2], st2["nMatchTimes"][2]) == (3, 3)
    assert (s["n_predicts"], s["n_matches"], s["n_deletes"], s["n_predicts_after"]) == (5, 5, 1, 4)      # the decrement does not ask whether it was counted
    vis[2] = 1                                                  # visible again: h replaces it
    v, _, st2 = _run(X, st, h, vis, z, m)
    assert v.tolist() == [0] * 6 and st2["predictLocation"][2].tolist() == [320.0, 240.0] and st2["nPredictTimes"][2] == 4


def test_table_need_add_at_min_matches_and_one_below():
    X, st, h, vis, z, m = _scene()
    m[5] = 0                                                    # 5 matches = min_matches: no add
    st["nMatchTimes"][5], st["nPredictTimes"][5] = 5, 5
    v, s, _ = _run(X, st, h, vis, z, m)
    assert v.tolist() == [0] * 6 and (s["n_matches_after"], s["need_add"], s["change"]) == (5, 0, 0)
    m[4] = 0                                                    # 4 = min_matches - 1
    st["nMatchTimes"][4], st["nPredictTimes"][4] = 5, 5
    v, s, _ = _run(X, st, h, vis, z, m)
    assert v.tolist() == [0] * 6 and (s["n_matches_after"], s["n_deletes"], s["need_add"], s["change"]) == (4, 0, 1, 1)
    # a store takes a match away: 5 matches, one of them stored -> 4
    X, st, h, vis, z, m = _scene()
    m[5] = 0
    st["nMatchTimes"][5], st["nPredictTimes"][5] = 5, 5
    z[0:2] = (321.0, 470.0)
    _, s, _ = _run(X, st, h, vis, z, m)
    assert (s["n_matches"], s["n_stores"], s["n_matches_after"], s["need_add"], s["change"]) == (5, 1, 4, 1, 1)
    # min_matches is a parameter
    _, s, _ = _run(X, st, h, vis, z, m, min_matches=4)
    assert (s["need_add"], s["change"]) == (0, 1)


def test_margins_report_every_real_valued_test():
    X, st, h, vis, z, m = _scene(2)
    m[1] = 0
    mg = []
    P.policy(st, X, h, vis, z, m, W, H, margins=mg)
    assert len(mg) == 2 * (2 + 4) + 4                           # rho, Hlr_z, four edges of the prediction per landmark; four edges of the one match
    assert min(mg) == pytest.approx(0.49)                       # rho - rho_min
