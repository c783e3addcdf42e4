"""GPU tests of the checked image runs (srukf_run_images_checked* / srukf_get_image_checks, k_associate_checked_staged; csrc/srukf_images.hip, srukf_unique.hip;
DESIGN.md §21): image runs whose frames take srukf_associate_checked's decisions (ambiguity veto, sub-pixel peak) — against the plain image run under neutral
parameters, against the step-wise calls (predict_motion, predict_measurement, associate_checked, update / update_joint), against the staged replay fed with the
record the run left, across graph forms and parameter changes, for the score maps, and at the edges.

Scene of the decision tests: tests/test_gpu_images.py's (texture seed 17 rolled one pixel per frame, the robot moving 1 cm per frame, landmark 5 without a record,
landmark 2 with a wrong one) with test_gpu_unique._tiled's 6-px periodic regions stamped into the texture before rolling, around the first-frame pixels of
landmarks 1 and 6, whose patches are cut from inside them.  Found on the CPU (the oracle's filter, oracle.warp_patch, np_unique.score_map / peaks; ratio 0.9,
exclusion 4, sub-pixel on; 6 frames, N = 8): the eight first-frame pixels lie within ~100 px of each other, so a region centred ON a landmark reaches the search
windows of its neighbours and makes them ambiguous too (with regions on (0, 7) or (1, 6) one or two matches per frame are left).  The regions are therefore shifted:
(0, +15) px for landmark 1, (+17, -17) px for landmark 6 — the landmark's 33 x 33 px of template and window plus the first alias stay inside, the far side of the region
points away from the neighbours.  Every pair of landmarks with a record (7 left out: the CPU run never matches it in §20's scene, the device does) and every shift in
{-15, 0, 15}^2 was tried with seed 17; only pair (1, 6) with landmark 6's region at (+15, -15) met every condition, landmark 3's corr2 / corr at 0.796; at (+17, -17)
landmark 3 is back at its value without regions.  With that scene the CPU run has, in every frame: landmarks 1 and 6 with flags 3 and corr2 == corr >= 0.9995,
landmarks 0, 3, 4 matched with flag bit 2 (corr >= 0.9998, corr2 / corr <= 0.731), landmarks 2 and 7 not raw (corr <= 0.52).  The same regions at N = 33: 18 matches per frame,
landmarks 1 and 6 vetoed.  The tests assert the conditions on the step-wise twin's own run before any comparison.
Sizes: N = 8 (n = 52, one panel), N = 33 once (two panels, JOINT), 640 x 480 images, at most 11 frames.  Bounds: the project's |dX| <= 1e-9, |dP| <= 1e-11."""
import functools

import numpy as np
import pytest

import np_unique as U
from test_gpu_images import F_MAX, NO_RECORD, TEXTURE_SEED, TOL_P, TOL_X, WRONG_RECORD, _case, _filter, _patch_bytes, _record_bytes, _state_bytes
from test_gpu_unique import _texture, _tiled

pytestmark = pytest.mark.gpu

TILED = (1, 6)                                                   # the landmarks inside periodic regions
TILE_SHIFT = {1: (0, 15), 6: (17, -17)}                          # centre of each region minus the landmark's first-frame pixel
PAR = dict(corr_threshold=0.8, ratio=0.9, exclusion=4, subpixel=True)
NEUTRAL = dict(corr_threshold=0.8, ratio=2.0, exclusion=4, subpixel=False)


@functools.lru_cache(maxsize=None)
def _tiled_case(srukf, synth, N):
    """test_gpu_images._case with the periodic regions in the texture: the frames, and every record but the wrong one cut again from the first of them"""
    cs = dict(_case(srukf, synth, N))
    px = [rec[1] for rec in cs["recs"]]
    centres = [(int(px[k][0]) + TILE_SHIFT[k][0], int(px[k][1]) + TILE_SHIFT[k][1]) for k in TILED]
    T = _tiled(_texture(np.random.default_rng(TEXTURE_SEED)), centres)
    frames = np.ascontiguousarray(np.stack([np.roll(T, (0, f), axis=(0, 1)) for f in range(F_MAX)]))
    recs = []
    for k, (patch, p2) in enumerate(cs["recs"]):
        cu, cv = int(p2[0]), int(p2[1])
        recs.append((patch if k == WRONG_RECORD else frames[0][cv - 10:cv + 11, cu - 10:cu + 11].copy(), p2))
    cs["frames"], cs["recs"] = frames, recs
    return cs


def _check_bytes(chk):
    return tuple(chk[k].tobytes() for k in ("corr2", "z2", "flags"))


def _all(f, F, traj=None):
    """everything a run leaves, as bytes: (trajectory,) state, both records, matchPatches"""
    return ((traj.tobytes(),) if traj is not None else ()) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + _check_bytes(f.get_image_checks(0, F)) + (_patch_bytes(f),)


def _maps(f):
    return [f.match_scores(k) for k in range(f.N)]


@functools.lru_cache(maxsize=None)
def _stepwise_checked(srukf, synth, N, mode, F=6):
    """the reference run on the tiled scene: predict_motion -> predict_measurement -> associate_checked(frame, PAR) -> update / update_joint fed exactly that call's z and
    matched, on a twin; the plain association's z (np_unique.peaks on the device's own map, sub-pixel off) beside it; the last frame's score maps; computed once per case"""
    cs = _tiled_case(srukf, synth, N)
    g = _filter(srukf, cs)
    keys = ("z", "matched", "corr", "corr2", "z2", "flags", "visible", "h", "pose", "P22", "z_plain")
    out = {k: [] for k in keys}
    for t in range(F):
        g.predict_motion(cs["odo"][t], cs["odo"][t + 1])
        h, _, vis = g.predict_measurement()
        r = g.associate_checked(cs["frames"][t], **PAR)
        maps = _maps(g)
        zp = np.zeros(2 * N)
        for k, (m, _, _) in enumerate(maps):
            if m.size:
                zp[2 * k:2 * k + 2] = U.peaks(m, h[2 * k], h[2 * k + 1], (m.shape[1] - 1) // 2, (m.shape[0] - 1) // 2, dict(PAR, subpixel=False))["z"]
        if mode == srukf.UPDATE_JOINT: g.update_joint(r["z"], r["matched"])
        else: g.update(r["z"], r["matched"], mode=srukf.UPDATE_BATCHED)
        pose, P4 = g.get_robot()
        vals = [r[k] for k in keys[:6]] + [vis, h, pose, P4[:2, :2].ravel(), zp]
        for k, v in zip(keys, vals): out[k].append(np.array(v, copy=True))
    out = {k: np.array(v) for k, v in out.items()}
    out["maps"] = maps
    out["info"] = g.clamp_info()
    out["X"], S = g.get_state(); out["P"] = S.T @ S
    g.close()
    return out


def _assert_scene(ref, N, name):
    """the conditions of the decision tests on the step-wise twin's run alone: a comparison with it cannot pass vacuously"""
    matched, flags, corr, corr2 = ref["matched"], ref["flags"], ref["corr"], ref["corr2"]
    raw = (flags & 1) != 0
    others = raw.copy(); others[:, list(TILED)] = False
    ratio = np.where(others, corr2 / np.where(corr > 0, corr, 1.0), 0.0)
    moved = (matched != 0) & ((flags & 4) != 0) & (np.abs(ref["z"] - ref["z_plain"]).reshape(-1, N, 2).max(axis=2) > 1e-3)
    print("twin %s: matches per frame %s, tiled flags %s, other raw corr2 / corr <= %.4f, matched corr >= %.4f, non-raw corr <= %.4f, refined and moved per frame %s"
          % (name, matched.sum(axis=1).tolist(), flags[:, list(TILED)].tolist(), ratio.max(), corr[matched != 0].min(), corr[~raw].max(), moved.sum(axis=1).tolist()))
    assert (matched.sum(axis=1) >= 3).all()
    assert (flags[:, list(TILED)] == 3).all()
    assert ratio.max() <= 0.8
    assert corr[matched != 0].min() >= 0.9 and corr[~raw].max() <= 0.7
    assert (moved.sum(axis=1) >= 1).all()


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_neutral_parameters_change_nothing(srukf, synth, mode_name):
    """ratio 2, sub-pixel off, threshold 0.8: run_images_checked(0, 6) and run_images(0, 6) on a twin leave bit-identical trajectory, X, S, record and matchPatches,
    on §20's scene and on the tiled one (where corr2 == corr for two landmarks and still nothing is vetoed); flags in {0, 1}, corr2 <= corr."""
    N, F, mode = 8, 6, getattr(srukf, "UPDATE_" + mode_name)
    for cs in (_case(srukf, synth, N), _tiled_case(srukf, synth, N)):
        f = _filter(srukf, cs, F)
        t0 = f.run_images(0, F, mode=mode)
        assert f.clamp_info() == (-1, -1)
        plain = (t0.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + (_patch_bytes(f),)
        zero = f.get_image_checks(0, F)                          # no checked run has written a row
        assert not zero["corr2"].any() and not zero["z2"].any() and not zero["flags"].any()
        f.close()
        g = _filter(srukf, cs, F)
        t1 = g.run_images_checked(0, F, mode=mode, **NEUTRAL)
        assert g.clamp_info() == (-1, -1)
        rec, chk = g.get_image_matches(0, F), g.get_image_checks(0, F)
        got = (t1.tobytes(),) + _state_bytes(g) + _record_bytes(rec) + (_patch_bytes(g),)
        g.close()
        assert got == plain
        assert (rec["matched"].sum(axis=1) >= 3).all()
        assert np.isin(chk["flags"], (0, 1)).all() and np.array_equal(chk["flags"], rec["matched"])
        assert (chk["corr2"] <= rec["corr"]).all() and (chk["corr2"] > 0).any()


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_against_the_stepwise_calls(srukf, synth, mode_name):
    """The tiled scene, ratio 0.9, exclusion 4, sub-pixel on, N = 8, 6 frames: run_images_checked against the twin driven step by step.  matched, flags, visible equal;
    z, z2, h to 1e-9; corr, corr2 to 1e-12; trajectory and final state within the bounds.  The veto acts: a plain run_images over the same frames matches the tiled
    landmarks, and where it ends clean its final X is another one.
    Measured (MI355X), BATCHED and JOINT: every one of these differences is 0; the twin has 4 matches per frame, other raw corr2 / corr <= 0.7310, matched corr >= 0.9997,
    non-raw corr <= 0.5193; the plain run ends clean, 0.368 away in X."""
    N, F, mode = 8, 6, getattr(srukf, "UPDATE_" + mode_name)
    cs = _tiled_case(srukf, synth, N)
    ref = _stepwise_checked(srukf, synth, N, mode)
    _assert_scene(ref, N, mode_name)
    f = _filter(srukf, cs, F)
    traj = f.run_images_checked(0, F, mode=mode, **PAR)
    rec, chk = f.get_image_matches(0, F), f.get_image_checks(0, F)
    assert f.clamp_info() == (-1, -1) and ref["info"] in ((-1, -1), (0, -1))
    X, S = f.get_state(); f.close()
    assert np.array_equal(rec["matched"], ref["matched"]) and np.array_equal(chk["flags"], ref["flags"]) and np.array_equal(rec["visible"], ref["visible"])
    d = {k: np.abs(a[k] - ref[k]).max() for a, ks in ((rec, ("z", "h", "corr")), (chk, ("z2", "corr2"))) for k in ks}
    dtx, dtp = np.abs(traj[:, :4] - ref["pose"]).max(), np.abs(traj[:, 4:] - ref["P22"]).max()
    dX, dP = np.abs(X - ref["X"]).max(), np.abs(S.T @ S - ref["P"]).max()
    print("N=%d %s: |dz| %.2e |dz2| %.2e |dh| %.2e |dcorr| %.2e |dcorr2| %.2e, trajectory |dX| %.2e |dP| %.2e, final |dX| %.2e |dP| %.2e"
          % (N, mode_name, d["z"], d["z2"], d["h"], d["corr"], d["corr2"], dtx, dtp, dX, dP))
    assert d["z"] <= 1e-9 and d["z2"] <= 1e-9 and d["h"] <= 1e-9 and d["corr"] <= 1e-12 and d["corr2"] <= 1e-12
    assert dtx <= TOL_X and dtp <= TOL_P and dX <= TOL_X and dP <= TOL_P
    assert rec["z"].reshape(F, N, 2)[:, list(TILED)].all()       # z is kept for a vetoed landmark
    # the veto acts
    g = _filter(srukf, cs, F)
    try:
        g.run_images(0, F, mode=mode)
        clean = True
    except srukf.SrukfError as e:
        assert e.rc == -7, str(e)
        clean = False
    if clean:
        assert (g.get_image_matches(0, F)["matched"][:, list(TILED)] == 1).all()
        Xp, _ = g.get_state()
        print("plain run_images on the tiled scene: clean, |X - X_checked| %.2e" % np.abs(Xp - X).max())
        assert not np.array_equal(Xp, X)
    else:
        fr, _ = g.clamp_info()
        print("plain run_images on the tiled scene: flagged in frame %d" % fr)
        if fr > 0:
            g.run_images(0, fr, mode=mode)
            assert (g.get_image_matches(0, fr)["matched"][:, list(TILED)] == 1).all()
    g.close()


@pytest.mark.parametrize("N,mode_name", [(8, "BATCHED"), (8, "JOINT"), (33, "JOINT")])
def test_exact_twin_of_the_staged_replay(srukf, synth, N, mode_name):
    """run_images_checked(0, F) on the tiled scene, then the record it left (z, matched) staged on a twin and run_frames(0, F) in the same frame form: trajectory, X and
    S bit-identical — the filter reads of the checked association its matched and z rows and nothing else (the vetoed landmarks' non-zero z included: unmatched rows
    are not read)."""
    F, mode = 6, getattr(srukf, "UPDATE_" + mode_name)
    cs = _tiled_case(srukf, synth, N)
    f = _filter(srukf, cs, F)
    traj = f.run_images_checked(0, F, mode=mode, **PAR)
    rec, chk = f.get_image_matches(0, F), f.get_image_checks(0, F)
    assert f.clamp_info() == (-1, -1)
    got = _state_bytes(f); f.close()
    assert (rec["matched"].sum(axis=1) >= 3).all()
    assert (chk["flags"][:, list(TILED)] == 3).all() and (rec["matched"][:, list(TILED)] == 0).all()
    g = _filter(srukf, cs, appearance=False)
    if mode == srukf.UPDATE_BATCHED: g.debug_set("fused_motion", 0)
    g.stage_sequence(cs["odo"][:F + 1], rec["z"], rec["matched"])
    traj2 = g.run_frames(0, F, mode=mode)
    assert g.clamp_info() == (-1, -1) and g.debug_get("exact_frames") == 0
    want = _state_bytes(g); g.close()
    assert traj.tobytes() == traj2.tobytes() and got == want


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_graph_forms_and_parameters(srukf, synth, mode_name):
    """N = 8, 11 frames of the tiled scene.  (a) default graphs (8 + 1 + 1 + 1), eager launches and two calls of 5 + 6 frames: bit-identical state, records and
    matchPatches.  (b) graphs on, frames 0-2 with ratio 0.9 and frames 3-5 with ratio 2: the bits of the same two runs made eagerly, and frames 3-5 match the tiled
    landmarks — no graph replayed stale parameters.  (c) run_images and run_images_checked alternate inside one block (3 + 3 + 3 + 2 asynchronous runs, one
    synchronize): with graphs and eagerly the same bits, so neither kind replayed the other's captured frame."""
    F, mode = F_MAX, getattr(srukf, "UPDATE_" + mode_name)
    cs = _tiled_case(srukf, synth, 8)
    out = []
    for name in ("default", "eager", "split"):
        f = _filter(srukf, cs, F, graph=0 if name == "eager" else None)
        if name == "split": t = np.vstack([f.run_images_checked(0, 5, mode=mode, **PAR), f.run_images_checked(5, 6, mode=mode, **PAR)])
        else: t = f.run_images_checked(0, F, mode=mode, **PAR)
        assert f.clamp_info() == (-1, -1)
        out.append(_all(f, F, t))
        rec, chk = f.get_image_matches(0, F), f.get_image_checks(0, F)
        f.close()
    assert out[0] == out[1] and out[0] == out[2]
    # (the conditions of the decision tests hold for frames 0-5; further on the periodic texture decorrelates under the warp: on the device landmark 1 is not raw in frames 9, 10)
    assert (rec["matched"].sum(axis=1) >= 3).all() and (chk["flags"][:6, list(TILED)] == 3).all() and (rec["matched"][:, list(TILED)] == 0).all()
    two = []
    for graph in (None, 0):
        f = _filter(srukf, cs, 6, graph=graph)
        t = np.vstack([f.run_images_checked(0, 3, mode=mode, **PAR), f.run_images_checked(3, 3, mode=mode, **dict(PAR, ratio=2.0))])
        assert f.clamp_info() == (-1, -1)
        two.append(_all(f, 6, t))
        m = f.get_image_matches(0, 6)["matched"][:, list(TILED)]
        f.close()
        assert (m[:3] == 0).all() and (m[3:] == 1).all(), m
    assert two[0] == two[1]
    alt = []
    for graph in (None, 0):
        f = _filter(srukf, cs, F, graph=graph)
        f.run_images_async(0, 3, mode=mode); f.run_images_checked_async(3, 3, mode=mode, **PAR)
        f.run_images_async(6, 3, mode=mode); f.run_images_checked_async(9, 2, mode=mode, **PAR)
        f.synchronize()
        assert f.clamp_info() == (-1, -1)
        alt.append(_all(f, F))
        m, fl = f.get_image_matches(0, F)["matched"][:, list(TILED)], f.get_image_checks(0, F)["flags"][:, list(TILED)]
        f.close()
        assert (m[[0, 1, 2]] == 1).all() and (m[[3, 4, 5, 9, 10]] == 0).all(), m                  # plain frames match the tiled landmarks, checked frames never
        assert (fl[[0, 1, 2, 6, 7, 8]] == 0).all() and (fl[[3, 4, 5]] == 3).all(), fl             # rows only plain runs wrote stay zero
    assert alt[0] == alt[1]


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_score_maps_are_the_last_frames(srukf, synth, mode_name):
    """After a clean run_images_checked(0, 6), match_scores(k) is what the step-wise twin's associate_checked left for frame 5: the map and its window, bit for bit;
    np_unique.peaks on that map reproduces the last record row's matched and flags."""
    N, F, mode = 8, 6, getattr(srukf, "UPDATE_" + mode_name)
    cs = _tiled_case(srukf, synth, N)
    ref = _stepwise_checked(srukf, synth, N, mode)
    f = _filter(srukf, cs, F)
    with pytest.raises(srukf.SrukfError) as e: f.match_scores(0)
    assert e.value.rc == -5                                      # no checked association yet
    f.run_images_checked(0, F, mode=mode, **PAR)
    maps = _maps(f)
    rec, chk = f.get_image_matches(F - 1, 1), f.get_image_checks(F - 1, 1)
    f.close()
    searched = 0
    for k, ((m, x0, y0), (rm, rx0, ry0)) in enumerate(zip(maps, ref["maps"])):
        assert m.shape == rm.shape and (x0, y0) == (rx0, ry0), k
        assert m.tobytes() == rm.tobytes(), (k, np.abs(m - rm).max())
        if not m.size:
            assert rec["matched"][0, k] == 0 and chk["flags"][0, k] == 0
            continue
        searched += 1
        pk = U.peaks(m, rec["h"][0, 2 * k], rec["h"][0, 2 * k + 1], (m.shape[1] - 1) // 2, (m.shape[0] - 1) // 2, PAR)
        assert pk["matched"] == rec["matched"][0, k] and pk["flags"] == chk["flags"][0, k], k
    assert searched >= 5 and maps[NO_RECORD][0].size == 0


def _rc(srukf, call):
    with pytest.raises(srukf.SrukfError) as e: call()
    return e.value.rc


def test_refusals_leave_everything_untouched(srukf, synth):
    """Bad parameters: SRUKF_ERR_BAD_ARG.  Nothing staged, a restage, delete_landmark, reset: SRUKF_ERR_SEQUENCE.  Frames beyond the stack: SRUKF_ERR_DIM_MISMATCH.
    SEQUENTIAL and the float-stored modes: SRUKF_ERR_UNSUPPORTED.  State and matchPatches as before in every one."""
    cs = _tiled_case(srukf, synth, 8)
    N, F = 8, 3
    f = _filter(srukf, cs, F)
    before = _state_bytes(f) + (_patch_bytes(f),)
    for kw in (dict(ratio=0.0), dict(ratio=-1.0), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(exclusion=0), dict(exclusion=21),
               dict(corr_threshold=float("nan")), dict(corr_threshold=float("inf"))):
        assert _rc(srukf, lambda: f.run_images_checked(0, F, **kw)) == -1, kw
        assert _rc(srukf, lambda: f.run_images_checked_async(0, F, **kw)) == -1, kw
    assert _rc(srukf, lambda: f.run_images_checked(0, F + 1, **PAR)) == -2
    assert _rc(srukf, lambda: f.run_images_checked(2, 2, **PAR)) == -2
    assert _rc(srukf, lambda: f.get_image_checks(0, F + 1)) == -2
    with pytest.raises(srukf.SrukfError) as e: f.run_images_checked(0, F, mode=srukf.UPDATE_SEQUENTIAL, **PAR)
    assert e.value.rc == -6 and "BATCHED and JOINT only" in str(e.value)
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    f.run_images_checked(0, F, exclusion=20, **{k: v for k, v in PAR.items() if k != "exclusion"})      # (the limits themselves are accepted)
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 2 * N)), np.zeros((F, N), dtype=np.int32))          # a restage drops the images
    before = _state_bytes(f) + (_patch_bytes(f),)
    for call in (lambda: f.run_images_checked(0, F, **PAR), lambda: f.run_images_checked_async(0, F, **PAR), lambda: f.get_image_checks(0, F)):
        with pytest.raises(srukf.SrukfError) as e: call()
        assert e.value.rc == -5 and "stage_images" in str(e.value)
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    f.stage_images(cs["frames"][:F]); f.run_images_checked(0, 1, **PAR)
    f.reset()
    assert _rc(srukf, lambda: f.run_images_checked(0, F, **PAR)) == -5
    assert _rc(srukf, lambda: f.match_scores(0)) == -5
    f.close()
    f = _filter(srukf, cs, F)
    f.run_images_checked(0, 1, **PAR)
    f.delete_landmark(0)                                         # a map change
    assert _rc(srukf, lambda: f.run_images_checked(0, F, **PAR)) == -5
    assert _rc(srukf, lambda: f.get_image_checks(0, 1)) == -5
    f.close()
    f = srukf.Filter(N, cs["p"]); f.set_state(cs["X1"], cs["S1"])
    assert _rc(srukf, lambda: f.run_images_checked(0, F, **PAR)) == -5      # nothing staged
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
            assert _rc(srukf, lambda: f.run_images_checked(0, F, mode=mode, **PAR)) == -6
            assert _rc(srukf, lambda: f.run_images_checked_async(0, F, mode=mode, **PAR)) == -6
        assert _state_bytes(f) == before
        f.close()


def test_flagged_checked_block_restores_its_checkpoint(srukf, synth):
    """N = 8, BATCHED, the shipped a1..a4 = 8 (§20's last row), run checked: SRUKF_ERR_CLAMP_PENDING, X, S and every matchPatch as before the call, and match_scores
    refuses as it does when no valid map exists."""
    F = 6
    cs = _case(srukf, synth, 8, "shipped")
    f = _filter(srukf, cs, F)
    before = _state_bytes(f) + (_patch_bytes(f),)
    with pytest.raises(srukf.SrukfError) as e: f.run_images_checked(0, F, **PAR)
    assert e.value.rc == -7, str(e.value)
    frame, row = f.clamp_info()
    print("flagged frame %d, row %d: %s" % (frame, row, e.value))
    assert 0 <= frame < F
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    assert _rc(srukf, lambda: f.match_scores(0)) == -5
    f.close()
