"""CPU tests of the archive search's restatement (tests/np_archive.py) and of the library's interface for it (include/srukf.h: srukf_archive_*)."""
import ctypes
import os
import re

import numpy as np
import pytest

import np_archive as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["srukf_archive_set", "srukf_archive_count", "srukf_archive_get_template", "srukf_archive_search"]


def params(synth, **kw):
    p = dict(synth.scene_params())
    p["image_w"], p["image_h"] = 640.0, 480.0
    p.update(kw)
    return p


def smooth(rng, shape, k=4):
    R = rng.integers(0, 256, size=(shape[0] + k, shape[1] + k)).astype(np.float64)
    c = np.cumsum(np.cumsum(R, 0), 1)
    return ((c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)).astype(np.uint8)


def test_library_exports_and_header_declares(pkg):
    lib_path = os.path.join(ROOT, "cv-monoslam_amd", "libsrukf_hip.so")
    if not os.path.exists(lib_path):
        pytest.fail("libsrukf_hip.so is not built")
    lib = ctypes.CDLL(lib_path)
    header = open(os.path.join(ROOT, "include", "srukf.h")).read()
    for name in CALLS:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in pkg.srukf.EXPORTS
    assert "typedef struct srukf_archive_params { int half_cap; double corr_threshold; double chi2; } srukf_archive_params;" in header
    assert lib.srukf_abi_version() == 6                          # additions do not bump it
    for m in ("archive_set", "archive_count", "archive_search", "archive_template"):
        assert hasattr(pkg.srukf.Filter, m)


def test_integer_correlation_equals_mean_subtracted_form():
    rng = np.random.default_rng(0)
    worst = 0.0
    for trial in range(200):
        v = rng.integers(0, 256, size=(17, 17), dtype=np.uint8)
        t = rng.integers(0, 256, size=(17, 17), dtype=np.uint8) if trial % 2 else np.clip(v.astype(int) + rng.integers(-20, 21, size=(17, 17)), 0, 255).astype(np.uint8)
        worst = max(worst, abs(A.corr_int(v, t) - A.corr_reference(v, t)))
    assert worst < 1e-12, worst
    v = smooth(rng, (17, 17))
    assert abs(A.corr_int(v, v) - 1.0) < 1e-15 and abs(A.corr_int(v, 255 - v) + 1.0) < 1e-15


def test_flat_patches_score_zero():
    rng = np.random.default_rng(1)
    v = rng.integers(0, 256, size=(17, 17), dtype=np.uint8)
    flat = np.full((17, 17), 93, dtype=np.uint8)
    assert A.corr_int(flat, v) == 0.0                            # B = 0
    assert A.corr_int(v, flat) == 0.0                            # C = 0
    assert A.corr_int(flat, flat) == 0.0
    # ... and inside the search: a flat frame gives corr 0, no match
    p = {"image_w": 640.0, "image_h": 480.0}
    z, m, cr = A.search(p, np.full((480, 640), 7, dtype=np.uint8), np.array([[300.2, 200.7]]), np.array([[[5.0, 0.0], [0.0, 5.0]]]), [1], v[None], 40)
    assert m[0] == 0 and cr[0] == 0.0 and np.array_equal(z[0], [0.0, 0.0])


def test_first_maximum_in_row_major_order():
    rng = np.random.default_rng(2)
    blob = smooth(rng, (17, 17))
    img = np.full((480, 640), 128, dtype=np.uint8)
    h = np.array([[320.4, 240.6]])
    Si = np.array([[[12.0, 0.0], [0.0, 12.0]]])                  # gate radius sqrt(5.99) * 12 = 29.4 px: half = 30
    spots = [(335, 250), (305, 250), (320, 228)]                 # (x, y) centres; the first maximum in row-major order is the smallest y, then the smallest x
    for x, y in spots:
        img[y - 8:y + 9, x - 8:x + 9] = blob
    z, m, cr = A.search({}, img, h, Si, [1], blob[None], 40)
    assert m[0] == 1 and cr[0] == 1.0 and np.array_equal(z[0], [320.0, 228.0])
    img[228 - 8:228 + 9, 320 - 8:320 + 9] = 128
    z, m, cr = A.search({}, img, h, Si, [1], blob[None], 40)
    assert m[0] == 1 and cr[0] == 1.0 and np.array_equal(z[0], [305.0, 250.0])      # equal y: the smaller x
    cc, x0, y0 = A.scores(img, h[0], Si[0], blob, 40)
    assert cc.shape == (61, 61) and (x0, y0) == (290, 210)
    assert cc[250 - y0, 335 - x0] == 1.0 and cc[250 - y0, 305 - x0] == 1.0
    # cap 10: both blobs (15 and 17.8 px away) lie outside the 21 x 21 window
    z, m, cr = A.search({}, img, h, Si, [1], blob[None], 10)
    assert m[0] == 0 and cr[0] < 0.8
    # a blob in the box and outside the gate ellipse is skipped: (345, 262) is 33 px away, inside the 61 x 61 box
    img2 = np.full((480, 640), 128, dtype=np.uint8)
    img2[262 - 8:262 + 9, 345 - 8:345 + 9] = blob
    cc, x0, y0 = A.scores(img2, h[0], Si[0], blob, 40)
    assert cc[262 - y0, 345 - x0] == 0.0
    assert A.search({}, img2, h, Si, [1], blob[None], 40)[1][0] == 0


def test_window_is_cut_by_the_image(synth):
    rng = np.random.default_rng(3)
    img = smooth(rng, (480, 640))
    for hx, hy, cx, cy in ((14.3, 12.8, 9, 8), (629.6, 470.2, 631, 471)):
        t = img[cy - 8:cy + 9, cx - 8:cx + 9]
        z, m, cr = A.search({}, img, np.array([[hx, hy]]), np.array([[[6.0, 0.0], [0.0, 6.0]]]), [1], t[None], 40)
        assert m[0] == 1 and cr[0] == 1.0 and np.array_equal(z[0], [cx, cy])
        cc, x0, y0 = A.scores(img, (hx, hy), np.array([[6.0, 0.0], [0.0, 6.0]]), t, 40)
        I = x0 + np.arange(cc.shape[1])
        assert (cc[:, (I < 8) | (I > 631)] == 0.0).all()          # candidates whose patch leaves the image


def test_certain_record_predicts_the_projection_of_its_mean(synth, oracle):
    """S66 = 0, P4 = 0, no pixel noise and an epsilon far below the state's ulp: all 25 sigma points are the mean, and h = wm0 Z0 + wi (24 Z0 summed in order).
    Bound from the weights (wm0 = -3, wi = 1/6, sum = 1), u = 2^-53: the running sum k Z0, k = 2 .. 24, rounds 23 times by at most u |k Z0| <= 299 u |Z0| in all,
    times wi; wi itself and the product round (2 u * 4 |Z0|), wm0 Z0 rounds (3 u |Z0|), the final sum rounds (4 u |Z0|): (299 / 6 + 8 + 3 + 4) u |Z0| < 65 u |Z0|."""
    p = params(synth, sigma_measure=0.0, epsilon=1e-300)
    X4 = np.array([0.3, -0.2, 0.0, 0.4])
    uv = np.array([[100.0, 90.0], [333.0, 251.0], [560.0, 400.0]])
    rec = A.make_records(oracle, params(synth), X4, np.diag([0.02, 0.02, 0.005, 0.02]), uv, np.zeros((480, 640), dtype=np.uint8))
    h, Si, vis, xyz, Z = A.predict(oracle, p, rec["X6"], np.zeros((3, 6, 6)), X4, np.zeros((4, 4)))
    Z0 = oracle.project(p, rec["X6"], np.tile(X4[:3], (3, 1)), np.full(3, X4[3]), np.zeros((3, 2)))
    assert np.array_equal(Z[:, 0], Z0) and (Z == Z[:, :1]).all()
    assert vis.tolist() == [1, 1, 1]
    err = np.abs(h - Z0).max()
    assert err <= 65 * 2.0 ** -53 * np.abs(Z0).max(), err
    np.testing.assert_allclose(Z0, uv, atol=0.5)                  # (the unscented mean of a joint initialisation projects next to its pixel)
    assert np.abs(Si).max() < 1e-140


def test_sigma_points_straddling_the_validity_border_hide_the_record(synth, oracle):
    """The mean projects 13 px inside the image — valid, the reference's test (1727) would call the landmark visible — while the pixel-noise sigma points
    (gamma sigma_measure = 5.2 px) cross the 10-px border and come back zeroed (a fraction of a pixel from the origin, behind the distortion): not visible here."""
    p = params(synth)
    X4 = np.array([0.0, 0.0, 0.0, 0.0])
    S4 = np.diag([0.02, 0.02, 0.005, 0.02])
    uv = np.array([[13.0, 240.0], [320.0, 13.0], [627.0, 240.0], [320.0, 240.0]])
    rec = A.make_records(oracle, p, X4, S4, uv, np.zeros((480, 640), dtype=np.uint8))
    h, Si, vis, xyz, Z = A.predict(oracle, p, rec["X6"], rec["S66"], X4, S4 @ S4)
    assert np.all(Z[:, 0] >= 10.0)                               # every mean pixel is valid
    assert vis.tolist() == [0, 0, 0, 1]
    assert all((Z[k] < 1.0).all(axis=1).any() for k in range(3))   # the zeroed pixels, behind the distortion
    z, m, cr = A.search(p, np.zeros((480, 640), dtype=np.uint8), h, Si, vis, np.zeros((4, 17, 17), dtype=np.uint8), 40)
    assert m.tolist() == [0, 0, 0, 0] and (cr == 0.0).all()


def test_chol_generalises_chol6():
    import np_loop
    rng = np.random.default_rng(4)
    M = rng.standard_normal((6, 6))
    P = M.T @ M
    assert np.array_equal(A.chol(P), np_loop.chol6(P))
    assert np.array_equal(A.chol(np.zeros((4, 4)), 1e-13), np.sqrt(1e-13) * np.eye(4))
    S = A.chol(P[:4, :4])
    np.testing.assert_allclose(S.T @ S, P[:4, :4], rtol=1e-12, atol=1e-12)
