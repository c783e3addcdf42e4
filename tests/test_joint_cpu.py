"""CPU tests of the joint measurement update's numpy restatement (tests/np_joint.py): its anchor to the reference's update (one
active landmark), a direct formula, positive semi-definiteness, the evidence the mode was built on (shipped constants, displaced pose) and its own
rounding floor, which the GPU tests' tolerance for the shipped constants is derived from."""
import numpy as np
import pytest

import np_joint as J
from np_filter import NpFilter


def _predicted(synth, sc, params=None, frames=0, X0=None, S0=None):
    """a joint filter `frames` joint frames into the scene, then predicted for the next one; returns (filter, frame index)"""
    f = J.NpJointFilter(sc["N"], params or sc["params"], synth)
    f.set_state(sc["X0"] if X0 is None else X0, sc["S0"] if S0 is None else S0)
    for fr in range(frames):
        f.predict_motion(sc["odo"][fr], sc["odo"][fr + 1]); f.predict_measurement()
        f.update_joint(sc["z"][fr], sc["matched"][fr])
    f.predict_motion(sc["odo"][frames], sc["odo"][frames + 1]); f.predict_measurement()
    return f, frames


@pytest.fixture(scope="module")
def scene8(synth):
    return synth.make_scene(8, 60, seed=3)


@pytest.fixture(scope="module")
def shipped(synth):
    """the shipped constants (a1..a4 = 8), N = 8 and N = 20, seed 3, 60 joint frames: (scene, filter after the run, per-frame pose errors, cond(Pzz))"""
    out = {}
    p = synth.default_params()
    for N in (8, 20):
        sc = synth.make_scene(N, 60, seed=3, p=p)
        f = J.make_filter(synth, sc, p)
        err, cond, lam = [], [], []
        for fr in range(60):
            f.predict_motion(sc["odo"][fr], sc["odo"][fr + 1]); f.predict_measurement()
            o = f.update_joint(sc["z"][fr], sc["matched"][fr])
            cond.append(np.linalg.cond(o["Pzz"]))
            ev = np.linalg.eigvalsh(o["G"])
            lam.append(ev[0] / ev[-1])
            err.append(np.linalg.norm(f.X[f.n - 4:f.n - 2] - sc["odo"][fr + 1, :2]))
        out[N] = (sc, f, np.array(err), np.array(cond), np.array(lam))
    return out


@pytest.mark.parametrize("k", [0, 5])
def test_one_active_landmark_is_the_reference_update(synth, scene8, k):
    """With one active landmark the joint update IS the reference's update for that landmark (Ki = Pxy Pi^-1, U = Ki Si^T): X and S^T S to 1e-12 relative."""
    sc = scene8
    for frames in (0, 2):
        f, fr = _predicted(synth, sc, frames=frames)
        g = NpFilter(8, sc["params"], synth)
        g.set_state(f.X, f.S); g.sig, g.Z, g.h, g.Si, g.w, g.wc0, g.wi = f.sig, f.Z, f.h, f.Si, f.w, f.wc0, f.wi
        m = np.zeros(8, dtype=np.int32); m[k] = 1
        f.update_joint(sc["z"][fr], m)
        g.update(sc["z"][fr], m, mode=1)
        P, Pg = f.S.T @ f.S, g.S.T @ g.S
        assert np.abs(f.X - g.X).max() <= 1e-12 * np.abs(g.X).max()
        assert np.abs(P - Pg).max() <= 1e-12 * np.abs(Pg).max()


def test_direct_formula_and_masking_equals_compaction(synth, scene8):
    """S^T S - U U^T = P - Pxy Pzz^-1 Pxy^T and X = X + Pxy Pzz^-1 (z - h) by numpy.linalg.solve on the COMPACTED system (inactive rows removed):
    masking by identity changes nothing."""
    sc = scene8
    f, fr = _predicted(synth, sc, frames=1)
    m = np.array([1, 0, 1, 1, 0, 0, 1, 1], dtype=np.int32)
    f.h[2 * 3:2 * 3 + 2] = 0.0                               # landmark 3 out of view: matched but inactive
    f.Z[2 * 6:2 * 6 + 2] = f.Z[2 * 6:2 * 6 + 2, :1]; f.Si[6] = 0.0  # landmark 6: every sigma point at the same pixel, Si = 0 (all of them outside the image): inactive
    o = f.joint(sc["z"][fr], m)
    assert list(o["active"]) == [True, False, True, False, False, False, False, True]
    on = np.repeat(o["active"], 2)
    Pzz_full = J.joint_pzz(f.Z, f.wi, f.n, f.Na, np.ones(8, dtype=bool))
    Pzz = Pzz_full[np.ix_(on, on)]
    Pxy = f.cross_covariance()[:, on]
    P = f.S.T @ f.S
    G = P - Pxy @ np.linalg.solve(Pzz, Pxy.T)
    X = f.X + Pxy @ np.linalg.solve(Pzz, (sc["z"][fr] - f.h)[on])
    assert np.abs(o["G"] - G).max() <= 1e-12 * np.abs(P).max()
    assert np.abs(o["X"] - X).max() <= 1e-12 * np.abs(X).max()
    assert np.array_equal(o["Ut"][~on], np.zeros((int((~on).sum()), f.n)))       # rows of inactive landmarks are zero
    # the 2 x 2 diagonal blocks are the reference's Si^T Si
    for k in (0, 1, 2, 4, 5, 7):
        np.testing.assert_allclose(Pzz_full[2 * k:2 * k + 2, 2 * k:2 * k + 2], f.Si[k].T @ f.Si[k], rtol=1e-12, atol=0)


def test_landmark_out_of_view_is_inactive(synth, scene8):
    """A landmark turned out of the image: every sigma point projects to the same pixel, so h != 0 ("visible") and Si = 0.  The reference's gain for it is zero
    (closed-form inverse of a singular Si); the joint form masks it, and equals the update without it."""
    sc = scene8
    X0 = sc["X0"].copy(); X0[6 * 5 + 3] += 1.2
    f, fr = _predicted(synth, sc, X0=X0)
    assert f.h[10] != 0 and f.h[11] != 0 and np.all(f.Si[5] == 0)
    m = np.ones(8, dtype=np.int32)
    a = f.joint(sc["z"][fr], m)
    assert not a["active"][5] and a["active"].sum() == 7
    m[5] = 0
    b = f.joint(sc["z"][fr], m)
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["G"], b["G"])


def test_no_active_landmark_is_a_no_op(synth, scene8):
    f, fr = _predicted(synth, scene8)
    X, S = f.X.copy(), f.S.copy()
    assert f.update_joint(scene8["z"][fr], np.zeros(8, dtype=np.int32)) is None
    assert np.array_equal(f.X, X) and np.array_equal(f.S, S)


def test_downdated_covariance_is_positive_semidefinite(synth, scene8, shipped):
    """lambda_min(S^T S - U U^T) >= -1e-12 lambda_max on every frame of the shipped-constant runs and on the scene-constant and displaced-pose frames"""
    for N in (8, 20):
        assert shipped[N][4].min() >= -1e-12, (N, shipped[N][4].min())
    f, fr = _predicted(synth, scene8, frames=3)
    ev = np.linalg.eigvalsh(f.joint(scene8["z"][fr], scene8["matched"][fr])["G"])
    assert ev[0] >= -1e-12 * ev[-1]
    sc, X0, S0 = J.displaced_scene(synth)
    f, fr = _predicted(synth, sc, X0=X0, S0=S0)
    ev = np.linalg.eigvalsh(f.joint(sc["z"][fr], sc["matched"][fr])["G"])
    assert ev[0] >= -1e-12 * ev[-1]


@pytest.mark.parametrize("N", [8, 20])
def test_shipped_constants_joint_tracks_where_the_reference_form_breaks(synth, shipped, N):
    """Shipped a1..a4 = 8, seed 3, 60 frames: the joint form finishes with no theta clamp and a finite pose (max pose error 1.1e-2 m at N = 8, 4.0e-3 m at
    N = 20); the reference's form clamps or fails within the first 5 frames."""
    sc, f, err, cond, _ = shipped[N]
    print("N = %d joint: theta clamps %d, max pose error %.3e m, cond(Pzz) <= %.3e (frame %d)" % (N, f.stats["theta"], err.max(), cond.max(), int(cond.argmax())))
    assert f.stats["theta"] == 0 and np.isfinite(f.X).all() and np.isfinite(f.S).all()
    assert err.max() < 2e-2
    g = NpFilter(N, sc["params"], synth); g.set_state(sc["X0"], sc["S0"])
    broke = False
    for fr in range(5):
        try:
            g.predict_motion(sc["odo"][fr], sc["odo"][fr + 1]); g.predict_measurement()
            g.update(sc["z"][fr], sc["matched"][fr], mode=1)
        except np.linalg.LinAlgError:
            broke = True
            break
        if g.stats["theta"] > 0 or not np.isfinite(g.X).all():
            broke = True
            break
    print("N = %d reference: theta clamps %d, min pivot %.3e by frame %d" % (N, g.stats["theta"], g.stats["min_pivot"], fr))
    assert broke


def test_scene_constants_joint_agrees_with_the_reference_form(synth):
    """Where the filter is healthy (scene constants, cond(Pzz) ~ 1) the two forms give the same trajectory: 60 frames at N = 8 within 1e-8 m."""
    sc = synth.make_scene(8, 60, seed=3)
    tj = J.make_filter(synth, sc).run_joint(sc)
    g = NpFilter(8, sc["params"], synth); g.set_state(sc["X0"], sc["S0"])
    tr = g.run(sc, mode=1)
    assert np.abs(tj[:, :4] - tr[:, :4]).max() < 1e-8
    assert abs(np.linalg.norm(tj[-1, :2] - sc["odo"][60, :2]) - 5.364e-7) < 1e-9


def test_displaced_pose_joint_recovers_reference_overshoots(synth):
    """Pose displaced 0.1 m, 0.15 m added to the robot's x / y sigma in quadrature, noiseless measurements (innovations ~ 25 px): one joint update brings the
    error down, one reference update (every landmark's gain from the same prior, added) drives it up."""
    sc, X0, S0 = J.displaced_scene(synth)
    res = {}
    for name in ("joint", "reference"):
        f, fr = _predicted(synth, sc, X0=X0, S0=S0)
        before = np.linalg.norm(f.X[f.n - 4:f.n - 2] - sc["odo"][1, :2])
        if name == "joint":
            f.update_joint(sc["z"][0], sc["matched"][0])
        else:
            f.update(sc["z"][0], sc["matched"][0], mode=1)
        res[name] = (before, np.linalg.norm(f.X[f.n - 4:f.n - 2] - sc["odo"][1, :2]))
        print("%s: pose error %.4f -> %.4f m" % (name, *res[name]))
    assert np.abs(sc["z"][0] - f.h).max() > 20
    assert res["joint"][1] < 0.05 * res["joint"][0]
    assert res["reference"][1] > res["reference"][0]


def test_rounding_floor_float64_against_longdouble(synth):
    """The restatement's own rounding (float64 against numpy.longdouble on the same frame), printed: the GPU tests' tolerance for the shipped constants is the
    larger of the project's per-frame bounds (1e-9, 1e-11) and 10 x this floor.  Measured: N = 20 scene constants d_X 5.0e-17, d_P 6.7e-18 (cond 1.5);
    shipped constants at the frame where cond(Pzz) peaks: N = 8 d_X 1.3e-15, d_P 1.8e-16 (cond 1.5e4, frame 33), N = 20 d_X 2.1e-15, d_P 2.3e-17 (cond 2.8e4)."""
    rows = [("scene N=20", 20, synth.scene_params(), 60), ("shipped N=8", 8, synth.default_params(), 60), ("shipped N=20", 20, synth.default_params(), 60)]
    for name, N, p, F in rows:
        dX, dP, cond, fr = J.rounding_floor(synth, N, p, F)
        print("%s: d_X %.3e d_P %.3e cond(Pzz) %.3e at frame %d" % (name, dX, dP, cond, fr))
        assert dX < 1e-12 and dP < 1e-13                     # far below the per-frame bounds: 10 x the floor never widens them
    tx, tp = J.shipped_tolerance(synth, 8, 20)
    assert (tx, tp) == (1e-9, 1e-11)
