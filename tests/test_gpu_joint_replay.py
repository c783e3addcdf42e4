"""GPU tests of the joint measurement update as a mode of the staged replay (run_frames / run_frames_async / prepare_frames with mode = UPDATE_JOINT;
csrc/srukf_replay.hip, srukf_joint.hip) against its numpy restatement (tests/np_joint.py) and against the step-wise update_joint, which
tests/test_gpu_joint.py holds to the same restatement.  Shapes as there: N = 8, 33, 70 are one, two and three 64-row panels of the innovation covariance; they
also give the frame tail's refactor forms below T = 16 (full rank at n = 52, rank-aware above n = 128).  Bounds: the project's per-frame |dX| <= 1e-9,
|dP| <= 1e-11; for the shipped constants np_joint.shipped_tolerance (the same numbers)."""
import functools

import numpy as np
import pytest

import np_joint as J
from test_gpu_joint import TOL_X, TOL_P, mask, params_of

pytestmark = pytest.mark.gpu

F6 = 6


@functools.lru_cache(maxsize=None)
def _scene(synth, N, which, F=F6, seed=3):
    return synth.make_scene(N, F, seed=seed, p=params_of(synth, which))


@functools.lru_cache(maxsize=None)
def _shipped_tol(synth):
    return J.shipped_tolerance(synth, 8, 20)


def tol(synth, which):
    return (TOL_X, TOL_P) if which == "scene" else _shipped_tol(synth)


def matches(sc, kind):
    """the scene's matches under a mask of test_gpu_joint.mask's kinds, every frame"""
    return (sc["matched"] * mask(kind, sc["N"])[None, :]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(synth, N, which, kind):
    """NpJointFilter.run_joint over the six frames -> (trajectory, X, S^T S); computed once per case"""
    sc = dict(_scene(synth, N, which))
    sc["matched"] = matches(sc, kind)
    g = J.make_filter(synth, sc)
    traj = g.run_joint(sc)
    return traj, g.X.copy(), g.S.T @ g.S


def staged(srukf, sc, m=None, graph=None, z=None):
    f = srukf.Filter(sc["N"], sc["params"])
    if graph is not None: f.debug_set("use_graph", graph)
    f.set_state(sc["X0"], sc["S0"])
    f.stage_sequence(sc["odo"], sc["z"] if z is None else z, sc["matched"] if m is None else m)
    return f


def state_bytes(f):
    X, S = f.get_state()
    return X.tobytes(), S.tobytes()


def traj_diff(a, b):
    return np.abs(a[:, :4] - b[:, :4]).max(), np.abs(a[:, 4:] - b[:, 4:]).max()


@pytest.mark.parametrize("N,kind,which", [(8, "all", "scene"), (33, "all", "scene"), (70, "all", "scene"), (8, "all", "shipped"), (33, "all", "shipped"),
                                          (33, "alt", "scene"), (33, "first32", "scene")])
def test_replay_against_the_restatement(srukf, synth, N, kind, which):
    """run_frames(0, 6, mode = UPDATE_JOINT): the trajectory rows and the final X and S^T S against NpJointFilter.run_joint; no frame flagged.
    (On the parent commit run_frames refuses the mode.)"""
    sc = _scene(synth, N, which)
    ref_traj, ref_X, ref_P = _reference(synth, N, which, kind)
    f = staged(srukf, sc, matches(sc, kind))
    traj = f.run_frames(0, F6, mode=srukf.UPDATE_JOINT)
    X, S = f.get_state()
    info = f.clamp_info()
    f.close()
    tx, tp = tol(synth, which)
    dtx, dtp = traj_diff(traj, ref_traj)
    dX, dP = np.abs(X - ref_X).max(), np.abs(S.T @ S - ref_P).max()
    print("N=%d %s %s: trajectory |dX| %.2e |dP| %.2e, final |dX| %.2e |dP| %.2e (bounds %.1e %.1e)" % (N, kind, which, dtx, dtp, dX, dP, tx, tp))
    assert info == (-1, -1)
    assert dtx <= tx and dtp <= tp and dX <= tx and dP <= tp


def test_owners_fold_tail_reads_the_permuted_Ut(srukf, synth):
    """The smallest N whose frame tail is RF_OWNERS_FOLD in the plain form (read from srukf_debug_get "plan_fold" and asserted: the owners read U^T with permuted
    columns from c->Utp and nowhere else, which the joint launches now write).  Three joint replay frames against the same filter driven step by step with
    predict_motion / predict_measurement / update_joint (tests/test_gpu_joint.py holds that to np_joint)."""
    N = 160                                                     # n = 964 -> np = 1024: T = 16, the first size at which the owners fold (N = 159: T = 15)
    sc = synth.make_scene(N, 3, seed=3, p=synth.scene_params())
    f = staged(srukf, sc)
    print("N=%d: plan_fold %d plan_T %d plan_kept %d" % (N, f.debug_get("plan_fold"), f.debug_get("plan_T"), f.debug_get("plan_kept")))
    assert f.debug_get("plan_fold") == 1 and f.debug_get("plan_T") == 16
    traj = f.run_frames(0, 3, mode=srukf.UPDATE_JOINT)
    assert f.debug_get("plan_fold") == 1 and f.clamp_info() == (-1, -1)
    X, S = f.get_state(); f.close()
    g = srukf.Filter(N, sc["params"]); g.set_state(sc["X0"], sc["S0"])
    worst = [0.0, 0.0]
    for t in range(3):
        g.predict_motion(sc["odo"][t], sc["odo"][t + 1]); g.predict_measurement(); g.update_joint(sc["z"][t], sc["matched"][t])
        pose, P4 = g.get_robot()
        worst = [max(worst[0], np.abs(traj[t, :4] - pose).max()), max(worst[1], np.abs(traj[t, 4:] - P4[:2, :2].ravel()).max())]
    assert g.clamp_info() == (-1, -1)
    Xs, Ss = g.get_state(); g.close()
    dX, dP = np.abs(X - Xs).max(), np.abs(S.T @ S - Ss.T @ Ss).max()
    print("N=%d owners' fold, 3 frames: trajectory |dX| %.2e |dP| %.2e, final |dX| %.2e |dP| %.2e" % (N, *worst, dX, dP))
    assert worst[0] <= TOL_X and worst[1] <= TOL_P and dX <= TOL_X and dP <= TOL_P


def test_graph_forms_are_one_computation(srukf, synth):
    """N = 33, 19 + 8 frames of the joint replay: the default graphs (8-frame graphs + single frames), a prepared 19-frame joint graph and eager launches give
    bit-identical trajectory, X and S."""
    sc = _scene(synth, 33, "scene", 27)
    out = []
    for name in ("default", "prepared", "eager"):
        f = staged(srukf, sc, graph=0 if name == "eager" else None)
        if name == "prepared": f.prepare_frames(19, mode=srukf.UPDATE_JOINT)
        t = np.vstack([f.run_frames(0, 19, mode=srukf.UPDATE_JOINT), f.run_frames(19, 8, mode=srukf.UPDATE_JOINT)])
        assert f.clamp_info() == (-1, -1)
        out.append((t.tobytes(),) + state_bytes(f)); f.close()
    assert out[0] == out[1] and out[0] == out[2]


def test_modes_alternate_without_replaying_each_others_graph(srukf, synth):
    """N = 33: 4 BATCHED + 4 JOINT + 4 BATCHED frames in three calls equal, within the per-frame bounds, the same twelve frames driven step by step with the
    matching update per frame, and are bit-identical to the same three calls with eager launches."""
    sc = _scene(synth, 33, "scene", 12)
    modes = [srukf.UPDATE_BATCHED] * 4 + [srukf.UPDATE_JOINT] * 4 + [srukf.UPDATE_BATCHED] * 4
    out = []
    for graph in (None, 0):
        f = staged(srukf, sc, graph=graph)
        t = np.vstack([f.run_frames(4 * q, 4, mode=modes[4 * q]) for q in range(3)])
        out.append((t,) + state_bytes(f))
        X, S = f.get_state(); f.close()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1:] == out[1][1:]
    g = srukf.Filter(33, sc["params"]); g.set_state(sc["X0"], sc["S0"])
    worst = [0.0, 0.0]
    for t in range(12):
        g.predict_motion(sc["odo"][t], sc["odo"][t + 1]); g.predict_measurement()
        if modes[t] == srukf.UPDATE_JOINT: g.update_joint(sc["z"][t], sc["matched"][t])
        else: g.update(sc["z"][t], sc["matched"][t], mode=srukf.UPDATE_BATCHED)
        pose, P4 = g.get_robot()
        worst = [max(worst[0], np.abs(out[0][0][t, :4] - pose).max()), max(worst[1], np.abs(out[0][0][t, 4:] - P4[:2, :2].ravel()).max())]
    Xs, Ss = g.get_state(); g.close()
    dX, dP = np.abs(X - Xs).max(), np.abs(S.T @ S - Ss.T @ Ss).max()
    print("4 B + 4 J + 4 B against step-wise: trajectory |dX| %.2e |dP| %.2e, final |dX| %.2e |dP| %.2e" % (*worst, dX, dP))
    assert worst[0] <= TOL_X and worst[1] <= TOL_P and dX <= TOL_X and dP <= TOL_P


@pytest.mark.parametrize("N", [8, 70])
def test_one_active_landmark_equals_batched_replay(srukf, synth, N):
    """With one active landmark the joint update is the reference's update for that landmark (section 19's anchor property), now on the replay: two joint frames
    against two BATCHED frames"""
    sc = _scene(synth, N, "scene")
    m = matches(sc, "one")
    assert m[:2].sum() == 2
    out = []
    for mode in (srukf.UPDATE_JOINT, srukf.UPDATE_BATCHED):
        f = staged(srukf, sc, m)
        t = f.run_frames(0, 2, mode=mode)
        X, S = f.get_state(); f.close()
        out.append((t, X, S.T @ S))
    dtx, dtp = traj_diff(out[0][0], out[1][0])
    dX, dP = np.abs(out[0][1] - out[1][1]).max(), np.abs(out[0][2] - out[1][2]).max()
    print("N=%d one landmark: trajectory |dX| %.2e |dP| %.2e, final |dX| %.2e |dP| %.2e" % (N, dtx, dtp, dX, dP))
    assert dtx <= TOL_X and dtp <= TOL_P and dX <= TOL_X and dP <= TOL_P


def test_non_finite_measurement_is_reported_not_propagated(srukf, synth):
    """N = 8, six frames, z[3, 0] = nan.  run_frames_async + synchronize: SRUKF_ERR_UNSUPPORTED, the text names frame 3; the first three trajectory rows are the
    state of a twin that ran frames 0 - 2 only; nothing in the state is NaN.  The synchronous run_frames: the same code, X and S bit-identical to before the call."""
    import torch
    sc = _scene(synth, 8, "scene")
    z = sc["z"].copy(); z[3, 0] = np.nan
    twin = staged(srukf, sc)
    t3 = twin.run_frames(0, 3, mode=srukf.UPDATE_JOINT)
    f = staged(srukf, sc, z=z)
    d_traj = torch.zeros((F6, 8), dtype=torch.float64, device="cuda")
    f.run_frames_async(0, F6, mode=srukf.UPDATE_JOINT, d_traj_ptr=d_traj.data_ptr())
    with pytest.raises(srukf.SrukfError) as e: f.synchronize()
    assert e.value.rc == -6 and "frame 3, row 0" in str(e.value), str(e.value)
    traj = d_traj.cpu().numpy()
    X, S = f.get_state(); f.close()
    assert np.isfinite(X).all() and np.isfinite(S).all() and np.isfinite(traj).all()
    assert traj[:3].tobytes() == t3.tobytes()
    pose, P4 = twin.get_robot(); twin.close()
    assert np.array_equal(traj[2, :4], pose) and np.abs(traj[2, 4:] - P4[:2, :2].ravel()).max() <= TOL_P      # (the block of P: another kernel's summation order)
    f = staged(srukf, sc, z=z)
    before = state_bytes(f)
    with pytest.raises(srukf.SrukfError) as e: f.run_frames(0, F6, mode=srukf.UPDATE_JOINT)
    assert e.value.rc == -6 and "frame 3" in str(e.value)
    X, S = f.get_state()
    assert np.isfinite(X).all() and np.isfinite(S).all() and state_bytes(f) == before
    # ... and the filter is usable: the finite frames in front of the bad one
    assert f.run_frames(0, 3, mode=srukf.UPDATE_JOINT).tobytes() == t3.tobytes()
    f.close()


def test_refusals(srukf, synth):
    """run_frames_batch in the new mode, the float-stored modes and SEQUENTIAL: SRUKF_ERR_UNSUPPORTED with a text, nothing runs"""
    sc = _scene(synth, 8, "scene")
    f = staged(srukf, sc)
    before = state_bytes(f)
    with pytest.raises(srukf.SrukfError) as e: srukf.run_frames_batch([f], 0, 2, mode=srukf.UPDATE_JOINT)
    assert e.value.rc == -6 and "run_frames_batch" in str(e.value)
    with pytest.raises(srukf.SrukfError) as e: f.run_frames(0, 2, mode=srukf.UPDATE_SEQUENTIAL)
    assert e.value.rc == -6
    with pytest.raises(srukf.SrukfError) as e: f.update(sc["z"][0], sc["matched"][0], mode=srukf.UPDATE_JOINT)      # (the step-wise entry is update_joint)
    assert e.value.rc == -5                                                                                            # ... before predict_measurement, as for every mode
    assert state_bytes(f) == before
    f.close()
    X0, S0 = sc["X0"].astype(np.float32).astype(np.float64), np.triu(sc["S0"]).astype(np.float32).astype(np.float64)
    for storage in (srukf.STORAGE_F32_MIXED, srukf.STORAGE_F32):
        f = srukf.Filter(8, sc["params"])
        if storage == srukf.STORAGE_F32_MIXED: f.debug_allow_mixed(1)
        f.set_storage(storage); f.set_state(X0, S0)
        f.stage_sequence(sc["odo"], sc["z"], sc["matched"])
        for call in (lambda: f.run_frames(0, 2, mode=srukf.UPDATE_JOINT), lambda: f.run_frames_async(0, 2, mode=srukf.UPDATE_JOINT),
                     lambda: f.prepare_frames(2, mode=srukf.UPDATE_JOINT)):
            with pytest.raises(srukf.SrukfError) as e: call()
            assert e.value.rc == -6 and "SRUKF_UPDATE_JOINT" in str(e.value)
        f.run_frames(0, 2, mode=srukf.UPDATE_BATCHED)                # the default mode runs as before
        f.close()
