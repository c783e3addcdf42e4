"""GPU tests of the image runs of the staged replay (srukf_stage_images / srukf_run_images* / srukf_get_image_matches, k_associate_staged; csrc/srukf_images.hip,
srukf_assoc.hip): staged camera frames replayed with the association on the device, against the step-wise calls (predict_motion, predict_measurement,
associate, update / update_joint), against the staged replay fed with the record the image run left, across its graph forms, and at its edges.

Scenes: the smooth texture and the Scene recipe of tests/test_gpu_unique.py (seed 13, one update into the sequence), patches captured at the pose of the first
frame, frames as test_facade_searches_the_archive makes them: the texture rolled one pixel per frame over a robot that moves 1 cm per frame.  Landmark 5 has no
appearance record, landmark 2's record was cut somewhere else.  Texture seed 17 was chosen on the CPU with the oracle's association (oracle.warp_patch /
associate_one around the oracle's filter): over 11 frames at N = 8 every matched correlation is >= 0.999 and every unmatched one <= 0.54; at N = 33, >= 0.95 and <= 0.52.
Sizes: N = 8 (mp = 64, one panel) and N = 33 (two panels), 640 x 480 images, at most 11 frames.  Bounds: the project's |dX| <= 1e-9, |dP| <= 1e-11."""
import functools

import numpy as np
import pytest

from test_gpu_unique import _rot, _texture

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-9, 1e-11
TEXTURE_SEED = 17
NO_RECORD, WRONG_RECORD = 5, 2
F_MAX = 11


@functools.lru_cache(maxsize=None)
def _frames():
    T = _texture(np.random.default_rng(TEXTURE_SEED))
    return np.ascontiguousarray(np.stack([np.roll(T, (0, f), axis=(0, 1)) for f in range(F_MAX)]))


@functools.lru_cache(maxsize=None)
def _case(srukf, synth, N, which="scene"):
    """start state (one update into the synthetic scene), odometry of F_MAX frames, the frames, and every landmark's appearance record; computed once per shape"""
    p = synth.scene_params() if which == "scene" else synth.default_params()
    sc = synth.make_scene(N, 3, seed=13, p=p)
    f = srukf.Filter(N, p)
    f.set_state(sc["X0"], sc["S0"])
    f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement(); f.update(sc["z"][0], sc["matched"][0])
    X1, S1 = f.get_state()
    base = sc["odo"][1]
    odo = np.array([[base[0] + 0.01 * i, base[1], base[2]] for i in range(F_MAX + 1)])
    f.predict_motion(odo[0], odo[1])
    h0, _, vis0 = f.predict_measurement()
    pose = f.get_state()[0][-4:].copy()                         # the pose the patches are 'captured' at: the first frame's
    f.close()
    frames = _frames()
    h0 = h0.reshape(N, 2)
    recs = []
    for k in range(N):
        cu, cv = int(round(h0[k, 0])), int(round(h0[k, 1]))
        if not vis0[k] or not (20 <= cu < 620 and 20 <= cv <= 459):
            cu, cv = 320, 240
        if k == WRONG_RECORD:
            su, sv = (cu - 70, cv + 50) if cu > 100 and cv < 400 else (110, 110)
            patch = frames[0][sv - 10:sv + 11, su - 10:su + 11].copy()
        else:
            patch = frames[0][cv - 10:cv + 11, cu - 10:cu + 11].copy()
        recs.append((patch, np.array([float(cu), float(cv)])))
    return dict(N=N, p=p, X1=X1, S1=S1, odo=odo, frames=frames, pose=pose, recs=recs)


def _filter(srukf, cs, F=None, graph=None, appearance=True):
    """a filter at the start state with the appearance records set (matchPatch zeroed); F: the first F frames staged, odometry and images (z / matched rows zero)"""
    N = cs["N"]
    f = srukf.Filter(N, cs["p"])
    if graph is not None: f.debug_set("use_graph", graph)
    f.set_state(cs["X1"], cs["S1"])
    if appearance:
        R = _rot(cs["pose"][3])
        for k, (patch, px) in enumerate(cs["recs"]):
            if k != NO_RECORD: f.set_landmark_appearance(k, patch, R, cs["pose"][:3], px)
    if F is not None:
        f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 2 * N)), np.zeros((F, N), dtype=np.int32))
        f.stage_images(cs["frames"][:F])
    return f


def _state_bytes(f):
    X, S = f.get_state()
    return X.tobytes(), S.tobytes()


def _patch_bytes(f):
    return b"".join(f.get_match_patch(k).tobytes() for k in range(f.N))


def _record_bytes(rec):
    return tuple(rec[k].tobytes() for k in ("z", "matched", "corr", "visible", "h"))


@functools.lru_cache(maxsize=None)
def _stepwise(srukf, synth, N, mode, F=6):
    """the reference run: the same frames through predict_motion -> predict_measurement -> associate -> update / update_joint on a twin; computed once per case"""
    cs = _case(srukf, synth, N)
    g = _filter(srukf, cs)
    out = dict(z=[], matched=[], corr=[], visible=[], h=[], pose=[], P22=[])
    for t in range(F):
        g.predict_motion(cs["odo"][t], cs["odo"][t + 1])
        h, _, vis = g.predict_measurement()
        z, m, cr = g.associate(cs["frames"][t])
        if mode == srukf.UPDATE_JOINT: g.update_joint(z, m)
        else: g.update(z, m, mode=srukf.UPDATE_BATCHED)
        pose, P4 = g.get_robot()
        for k, v in zip(("z", "matched", "corr", "visible", "h", "pose", "P22"), (z, m, cr, vis, h, pose, P4[:2, :2].ravel())): out[k].append(np.array(v, copy=True))
    out = {k: np.array(v) for k, v in out.items()}
    out["info"] = g.clamp_info()
    out["X"], S = g.get_state(); out["P"] = S.T @ S
    g.close()
    return out


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_against_the_stepwise_calls(srukf, synth, mode_name):
    """N = 8, 6 frames.  run_images against the twin driven step by step: matched and visible equal, z and h to 1e-9 with equal integer offsets, corr to 1e-12,
    trajectory, X and S^T S within the bounds.  The twin's run alone shows that the comparison is not vacuous."""
    N, F, mode = 8, 6, getattr(srukf, "UPDATE_" + mode_name)
    cs = _case(srukf, synth, N)
    ref = _stepwise(srukf, synth, N, mode)
    has = np.array([k != NO_RECORD for k in range(N)])
    # conditions on the reference run
    assert (ref["matched"].sum(axis=1) >= 3).all(), ref["matched"].sum(axis=1)
    assert ((ref["matched"] == 0) & has[None, :] & (ref["visible"] != 0)).any()              # a landmark with a record, in view, unmatched in some frame
    assert (ref["matched"][:, NO_RECORD] == 0).all() and (ref["corr"][:, NO_RECORD] == 0).all()
    mc, uc = ref["corr"][ref["matched"] != 0], ref["corr"][(ref["matched"] == 0)]
    print("twin %s: matches per frame %s, matched corr >= %.4f, unmatched corr <= %.4f" % (mode_name, ref["matched"].sum(axis=1).tolist(), mc.min(), uc.max()))
    assert mc.min() >= 0.9 and uc.max() <= 0.7                  # no decision sits on the 0.8 threshold
    f = _filter(srukf, cs, F)
    traj = f.run_images(0, F, mode=mode)
    rec = f.get_image_matches(0, F)
    assert f.clamp_info() == (-1, -1) and ref["info"] in ((-1, -1), (0, -1))
    X, S = f.get_state(); f.close()
    assert np.array_equal(rec["matched"], ref["matched"]) and np.array_equal(rec["visible"], ref["visible"])
    dz, dh, dc = np.abs(rec["z"] - ref["z"]).max(), np.abs(rec["h"] - ref["h"]).max(), np.abs(rec["corr"] - ref["corr"]).max()
    m2 = np.repeat(ref["matched"] != 0, 2, axis=1)
    assert np.array_equal(np.rint(rec["z"] - rec["h"])[m2], np.rint(ref["z"] - ref["h"])[m2])  # the integer offsets of 1991-1992
    assert not rec["z"][~m2].any()
    dtx, dtp = np.abs(traj[:, :4] - ref["pose"]).max(), np.abs(traj[:, 4:] - ref["P22"]).max()
    dX, dP = np.abs(X - ref["X"]).max(), np.abs(S.T @ S - ref["P"]).max()
    print("N=%d %s: |dz| %.2e |dh| %.2e |dcorr| %.2e, trajectory |dX| %.2e |dP| %.2e, final |dX| %.2e |dP| %.2e" % (N, mode_name, dz, dh, dc, dtx, dtp, dX, dP))
    assert dz <= 1e-9 and dh <= 1e-9 and dc <= 1e-12
    assert dtx <= TOL_X and dtp <= TOL_P and dX <= TOL_X and dP <= TOL_P


@pytest.mark.parametrize("N,mode_name", [(8, "BATCHED"), (8, "JOINT"), (33, "JOINT")])
def test_exact_twin_of_the_staged_replay(srukf, synth, N, mode_name):
    """run_images(0, F), then the record it left staged on a twin from the same start state and run_frames(0, F) in the same frame form ("fused_motion" 0 for BATCHED;
    a JOINT frame is the plain form anyway): trajectory, X and S bit-identical — the association launches touch nothing the filter's arithmetic reads but their rows."""
    F, mode = 6, getattr(srukf, "UPDATE_" + mode_name)
    cs = _case(srukf, synth, N)
    f = _filter(srukf, cs, F)
    traj = f.run_images(0, F, mode=mode)
    rec = f.get_image_matches(0, F)
    assert f.clamp_info() == (-1, -1)
    got = _state_bytes(f); f.close()
    assert (rec["matched"].sum(axis=1) >= 3).all()
    g = _filter(srukf, cs, appearance=False)
    if mode == srukf.UPDATE_BATCHED: g.debug_set("fused_motion", 0)
    g.stage_sequence(cs["odo"][:F + 1], rec["z"], rec["matched"])
    traj2 = g.run_frames(0, F, mode=mode)
    assert g.clamp_info() == (-1, -1) and g.debug_get("exact_frames") == 0
    want = _state_bytes(g); g.close()
    assert traj.tobytes() == traj2.tobytes() and got == want


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_graph_forms_are_one_computation(srukf, synth, mode_name):
    """N = 8, 11 frames: the default graphs (one 8-frame graph + three single frames), eager launches and two calls of 5 + 6 frames leave bit-identical trajectory,
    X, S, record and matchPatches.  Then run_frames and run_images calls alternate on one filter: with graphs and with eager launches the same bits, so neither
    replayed the other's captured frame."""
    F, mode = F_MAX, getattr(srukf, "UPDATE_" + mode_name)
    cs = _case(srukf, synth, 8)
    out = []
    for name in ("default", "eager", "split"):
        f = _filter(srukf, cs, F, graph=0 if name == "eager" else None)
        t = np.vstack([f.run_images(0, 5, mode=mode), f.run_images(5, 6, mode=mode)]) if name == "split" else f.run_images(0, F, mode=mode)
        assert f.clamp_info() == (-1, -1)
        rec = f.get_image_matches(0, F)
        out.append((t.tobytes(),) + _state_bytes(f) + _record_bytes(rec) + (_patch_bytes(f),))
        f.close()
    assert out[0] == out[1] and out[0] == out[2]
    assert (rec["matched"].sum(axis=1) >= 3).all()
    alt = []
    for graph in (None, 0):
        f = _filter(srukf, cs, F, graph=graph)
        f.stage_sequence(cs["odo"][:F + 1], rec["z"], rec["matched"]); f.stage_images(cs["frames"][:F])      # rows of frames only run_frames visits hold real matches
        t = np.vstack([f.run_images(0, 3, mode=mode), f.run_frames(3, 3, mode=mode), f.run_images(6, 3, mode=mode), f.run_frames(9, 2, mode=mode)])
        alt.append((t.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + (_patch_bytes(f),))
        f.close()
    assert alt[0] == alt[1]


def test_held_frame_is_not_touched(srukf, synth):
    """The frame the handle holds before an image run is the one associate_held searches after it: the same bits as a twin that brings that frame itself"""
    cs = _case(srukf, synth, 8)
    held = np.ascontiguousarray(cs["frames"][3])
    res = []
    for who in ("held", "brought"):
        f = _filter(srukf, cs, 3)
        if who == "held": f.detect_features(held)              # (any call that brings a gray frame holds it)
        f.run_images(0, 3)
        f.predict_motion(cs["odo"][3], cs["odo"][4]); f.predict_measurement()
        z, m, cr = f.associate_held() if who == "held" else f.associate(held)
        res.append((z.tobytes(), m.tobytes(), cr.tobytes(), _patch_bytes(f)))
        assert m.sum() >= 3
        f.close()
    assert res[0] == res[1]


def test_lifetime_and_refusals(srukf, synth):
    """Restaging the sequence, a map change and reset drop the images (SRUKF_ERR_SEQUENCE); frames beyond the staged ones: SRUKF_ERR_DIM_MISMATCH; modes the
    replay does not have and the float-stored modes: SRUKF_ERR_UNSUPPORTED.  Nothing runs in any of them."""
    cs = _case(srukf, synth, 8)
    N, F = 8, 3
    f = _filter(srukf, cs, F)
    before = _state_bytes(f)
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F + 1)
    assert e.value.rc == -2
    with pytest.raises(srukf.SrukfError) as e: f.run_images(2, 2)
    assert e.value.rc == -2
    with pytest.raises(srukf.SrukfError) as e: f.get_image_matches(0, F + 1)
    assert e.value.rc == -2
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F, mode=srukf.UPDATE_SEQUENTIAL)
    assert e.value.rc == -6 and "BATCHED and JOINT only" in str(e.value)
    with pytest.raises(srukf.SrukfError) as e: f.stage_images(cs["frames"][:F + 1])          # not the staged sequence's frame count
    assert e.value.rc == -2
    assert _state_bytes(f) == before
    f.run_images(0, F)                                           # (the images staged before the refused call are still there)
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 2 * N)), np.zeros((F, N), dtype=np.int32))
    for call in (lambda: f.run_images(0, F), lambda: f.run_images_async(0, F), lambda: f.get_image_matches(0, F)):
        with pytest.raises(srukf.SrukfError) as e: call()
        assert e.value.rc == -5 and "stage_images" in str(e.value)
    f.stage_images(cs["frames"][:F]); f.run_images(0, 1)
    f.reset()
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F)
    assert e.value.rc == -5
    f.close()
    f = _filter(srukf, cs, F)
    f.delete_landmark(0)                                         # a map change
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F)
    assert e.value.rc == -5
    with pytest.raises(srukf.SrukfError) as e: f.stage_images(cs["frames"][:F])              # ... which dropped the staged sequence too
    assert e.value.rc == -5
    f.close()
    f = srukf.Filter(N, cs["p"]); f.set_state(cs["X1"], cs["S1"])
    with pytest.raises(srukf.SrukfError) as e: f.stage_images(cs["frames"][:F])              # no staged sequence
    assert e.value.rc == -5
    f.close()
    X0, S0 = cs["X1"].astype(np.float32).astype(np.float64), np.triu(cs["S1"]).astype(np.float32).astype(np.float64)
    for storage in (srukf.STORAGE_F32_MIXED, srukf.STORAGE_F32):
        f = srukf.Filter(N, cs["p"])
        if storage == srukf.STORAGE_F32_MIXED: f.debug_allow_mixed(1)
        f.set_storage(storage); f.set_state(X0, S0)
        f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 2 * N)), np.zeros((F, N), dtype=np.int32))
        f.stage_images(cs["frames"][:F])
        before = _state_bytes(f)
        for mode in (srukf.UPDATE_BATCHED, srukf.UPDATE_JOINT):
            for call in (lambda: f.run_images(0, F, mode=mode), lambda: f.run_images_async(0, F, mode=mode)):
                with pytest.raises(srukf.SrukfError) as e: call()
                assert e.value.rc == -6
        assert _state_bytes(f) == before
        f.close()


def test_flagged_block_restores_its_checkpoint(srukf, synth):
    """N = 8, BATCHED, the shipped a1..a4 = 8 (the reference update clamps by frame 2 there).  run_images returns SRUKF_ERR_CLAMP_PENDING, X, S and
    every matchPatch are bit-identical to their values before the call, clamp_info names a frame inside the block — and the filter runs a clean block afterwards."""
    F = 6
    cs = _case(srukf, synth, 8, "shipped")
    f = _filter(srukf, cs, F)
    before = _state_bytes(f) + (_patch_bytes(f),)
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F)
    assert e.value.rc == -7, str(e.value)
    frame, row = f.clamp_info()
    print("flagged frame %d, row %d: %s" % (frame, row, e.value))
    assert 0 <= frame < F
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    if frame > 0:
        f.run_images(0, frame)                                   # the frames in front of the flagged one are clean
        assert f.clamp_info() == (frame, row) and _patch_bytes(f) != before[2]
    f.close()
