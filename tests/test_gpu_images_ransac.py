"""GPU tests of the 1-point RANSAC consensus inside image runs (srukf_images_ransac / srukf_get_image_ransac, k_ransac_votes_staged / k_ransac_pick_staged;
csrc/srukf_ransac.hip, srukf_images.hip): against a twin driven step by step (predict_motion -> predict_measurement -> associate -> ransac_consensus
-> update / update_joint with matched & inlier), against the run with the switch off on a clean scene, across the graph forms, with fewer than two matches, with
the map policy and the archive search behind the frames, through a threshold change, the switch's lifetime and a flagged block; every form of an image frame
(checked, search, ransac: ImageForm, csrc/srukf_ctx.h) on one handle against fresh handles; and the step-wise consensus at N = 260, where the shared votes body
strides twice.

Scenes: tests/test_gpu_images.py's (N = 8, seed 13, texture seed 17, 640 x 480, at most 11 frames; landmark 5 has no record, landmark 2's was cut elsewhere).
The outlier scene is that scene with landmark OUT_LM's patch cut (DX, DY) pixels aside of its record's pixel: the association finds it that far from where the
state puts it.  In this scene the texture rolls one pixel per frame over a robot that moves 1 cm, so the clean matches themselves sit 2.8 (frame 0) to 4.5 px
(frame 5) from every hypothesis' projection — a one-point update barely moves the other landmarks, d_ij is |z_j - h_j| to a few hundredths for i != j — and a
hypothesis takes back about half of its own innovation.  (DX, DY) = (7, -8) and THR = 4.8 px were chosen on the CPU with the oracle's association
(oracle.warp_patch / associate_one around the oracle's filter, tests/np_ransac.py's consensus): over frames 0..5 the displaced match stays inside the 8-px search
window, lies 5.1 - 6.3 px from the best hypothesis' projection and the clean ones at most 4.48 px; no pair closer than 0.3 px to the threshold.  A displaced
match that were an inlier would be absorbed by the update and the displacement would be gone in the next frame; held outside, it persists.  Beyond frame 5 the
clean distances pass 4.8 px: the 11-frame runs of the graph-form test compare the forms with one another, not with a twin.
Integers are compared as integers; the twin's preconditions are asserted on the twin alone, before any comparison."""
import functools

import numpy as np
import pytest

import np_ransac
from test_gpu_images import F_MAX, NO_RECORD, _case, _filter, _patch_bytes, _record_bytes, _state_bytes
from test_gpu_policy import NEUTRAL, PAR, _seed, _summary_dict, _same_state
from test_gpu_ransac import DIST_TOL, KINDS, make_z

pytestmark = pytest.mark.gpu

TOL_X, TOL_P = 1e-9, 1e-11
OUT_LM, DX, DY, THR = 0, 7, -8, 4.8
THR_DEFAULT = 8.0
MARGIN = 1e-6                                                    # 100 x the 1e-8 px DESIGN.md §13 holds dist to: the integers compare exactly
REC_KEYS = ("flags", "votes", "dist", "best", "n_active", "n_low")


@functools.lru_cache(maxsize=None)
def _outlier_case(srukf, synth, which="scene"):
    cs = dict(_case(srukf, synth, 8, which))
    recs = list(cs["recs"])
    _, px = recs[OUT_LM]
    cu, cv = int(px[0]) + DX, int(px[1]) + DY
    recs[OUT_LM] = (cs["frames"][0][cv - 10:cv + 11, cu - 10:cu + 11].copy(), px)
    cs["recs"] = recs
    return cs


def _scene(srukf, synth, scene, which="scene"):
    return _outlier_case(srukf, synth, which) if scene == "outlier" else _case(srukf, synth, 8, which)


def _run(f, first, count, mode, checked=False):
    return f.run_images_checked(first, count, mode=mode, **NEUTRAL) if checked else f.run_images(first, count, mode=mode)


def _ransac_bytes(rec):
    return tuple(rec[k].tobytes() for k in REC_KEYS) + (rec["first_outlier"],)


@functools.lru_cache(maxsize=None)
def _twin(srukf, synth, scene, mode, checked, thr, F=6):
    """the step-wise route with the consensus in it, the map policy behind every frame (fed with the masked matches), and the preconditions of the outlier scene"""
    cs = _scene(srukf, synth, scene)
    N = 8
    g = _filter(srukf, cs)
    st = _seed()
    out = {k: [] for k in REC_KEYS + ("matched", "z", "pose", "P22", "verdict", "summary", "raw")}
    for t in range(F):
        g.predict_motion(cs["odo"][t], cs["odo"][t + 1])
        h, _, vis = g.predict_measurement()
        if checked:
            r = g.associate_checked(cs["frames"][t], **NEUTRAL); z, m = r["z"], r["matched"]
        else:
            z, m, _ = g.associate(cs["frames"][t])
        z, m = np.array(z, copy=True), np.array(m, dtype=np.int32, copy=True)
        act = (m != 0) & (np.asarray(vis) != 0)
        if act.sum() >= 2:
            inl, votes, dist, best = g.ransac_consensus(z, m, thr)
            inl = np.array(inl, dtype=np.int32)
        else:
            inl, votes, dist, best = act.astype(np.int32), np.zeros(N, dtype=np.int32), np.zeros(N), -1
        used = (m * (inl != 0)).astype(np.int32) if act.sum() >= 2 else m
        if scene == "outlier" and thr == THR:
            # what the scene was chosen for, on the twin alone: the displaced landmark matched, outside the threshold under the best hypothesis, the clean ones
            # inside; no pair within MARGIN of the threshold.  The pairs: the consensus with the threshold a MARGIN lower and higher votes the same
            assert m[OUT_LM] == 1 and act.sum() >= 3, (t, m)
            assert inl[OUT_LM] == 0 and inl[act].sum() == act.sum() - 1, (t, inl, dist)
            for th2 in (thr - MARGIN, thr + MARGIN):
                i2, v2, _, b2 = g.ransac_consensus(z, m, th2)
                assert np.array_equal(i2, inl) and np.array_equal(v2, votes) and b2 == best, (t, th2)
            assert np.abs(np.asarray(dist)[act] - thr).min() >= MARGIN
        if mode == srukf.UPDATE_JOINT: g.update_joint(z, used)
        else: g.update(z, used, mode=srukf.UPDATE_BATCHED)
        v, s, st = g.map_policy(st, h, vis, z, used, **PAR)
        pose, P4 = g.get_robot()
        flags = act.astype(np.int32) | (2 * (inl != 0)).astype(np.int32)
        for k, val in zip(REC_KEYS + ("matched", "z", "pose", "P22", "verdict", "summary", "raw"),
                          (flags, votes, dist, best, int(act.sum()), int((inl != 0).sum()), used, z, pose, P4[:2, :2].ravel(), v, s, m)):
            out[k].append(val if k == "summary" else np.array(val, copy=True))
    out = {k: (v if k == "summary" else np.array(v)) for k, v in out.items()}
    out["state"] = st
    out["X"], S = g.get_state(); out["P"] = S.T @ S
    out["info"] = g.clamp_info()
    g.close()
    print("twin %s thr %.2f: active %s, low inliers %s, best %s, dist of frame 0 %s" % (scene, thr, out["n_active"].tolist(), out["n_low"].tolist(),
                                                                                        out["best"].tolist(), np.round(out["dist"][0], 3).tolist()))
    return out


def _ransac_filter(srukf, synth, scene, F, thr, graph=None, which="scene"):
    f = _filter(srukf, _scene(srukf, synth, scene, which), F, graph=graph)
    f.images_ransac(True, thr)
    return f


def _equal_records(rec, tw, F):
    for k in ("flags", "votes", "best", "n_active", "n_low"):
        assert np.array_equal(rec[k], tw[k][:F]), (k, rec[k], tw[k][:F])
    dd = np.abs(rec["dist"] - tw["dist"][:F]).max()
    return dd


# ---- 1. against the step-wise twin ----
@pytest.mark.parametrize("mode_name,checked", [("BATCHED", False), ("JOINT", False), ("BATCHED", True), ("JOINT", True)])
def test_against_the_stepwise_twin(srukf, synth, mode_name, checked):
    """the outlier scene, 6 frames: flags, votes, best, n_active, n_low and the masked matched equal; dist bit-identical (both routes run one text of the kernels
    on operands the same launches formed); trajectory and final state within the project's bounds; first_outlier == 0"""
    F, mode = 6, getattr(srukf, "UPDATE_" + mode_name)
    tw = _twin(srukf, synth, "outlier", mode, checked, THR)
    f = _ransac_filter(srukf, synth, "outlier", F, THR)
    traj = _run(f, 0, F, mode, checked)
    rec, mt = f.get_image_ransac(0, F), f.get_image_matches(0, F)
    assert f.clamp_info() == (-1, -1) and tw["info"] in ((-1, -1), (0, -1))
    X, S = f.get_state(); f.close()
    dd = _equal_records(rec, tw, F)
    assert np.array_equal(mt["matched"], tw["matched"])
    assert (tw["raw"][:, OUT_LM] == 1).all() and (mt["matched"][:, OUT_LM] == 0).all()       # the association found it, the filter did not use it
    m2 = np.repeat(tw["raw"] != 0, 2, axis=1)
    assert np.abs(mt["z"] - tw["z"])[m2].max() <= 1e-9 and mt["z"][:, 2 * OUT_LM:2 * OUT_LM + 2].all()      # z stays as the association left it
    dtx, dtp = np.abs(traj[:, :4] - tw["pose"]).max(), np.abs(traj[:, 4:] - tw["P22"]).max()
    dX, dP = np.abs(X - tw["X"]).max(), np.abs(S.T @ S - tw["P"]).max()
    print("%s%s: |ddist| max %.3e (bit-identical: %s), trajectory |dX| %.2e |dP| %.2e, final |dX| %.2e |dP| %.2e" %
          (mode_name, " checked" if checked else "", dd, rec["dist"].tobytes() == tw["dist"].tobytes(), dtx, dtp, dX, dP))
    assert rec["dist"].tobytes() == tw["dist"].tobytes()
    assert dtx <= TOL_X and dtp <= TOL_P and dX <= TOL_X and dP <= TOL_P
    assert rec["first_outlier"] == 0 and (rec["n_low"] == rec["n_active"] - 1).all()


# ---- 2. a clean scene ----
@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_clean_scene_is_the_run_without_the_switch(srukf, synth, mode_name):
    """DESIGN.md §13's default threshold 8, 6 frames: trajectory, X, S, the match record and every matchPatch bit-identical to the run with the switch off; every
    match is an inlier, best is the lowest active index, no frame is an outlier frame"""
    F, mode = 6, getattr(srukf, "UPDATE_" + mode_name)
    cs = _case(srukf, synth, 8)
    g = _filter(srukf, cs, F)
    t = g.run_images(0, F, mode=mode)
    mt = g.get_image_matches(0, F)
    off = (t.tobytes(),) + _state_bytes(g) + _record_bytes(mt) + (_patch_bytes(g),)
    assert g.clamp_info() == (-1, -1)
    g.close()
    f = _ransac_filter(srukf, synth, "clean", F, THR_DEFAULT)
    t = f.run_images(0, F, mode=mode)
    on = (t.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + (_patch_bytes(f),)
    rec = f.get_image_ransac(0, F)
    assert f.clamp_info() == (-1, -1)
    f.close()
    print("clean %s: n_active %s n_low %s best %s, largest dist %.3f" % (mode_name, rec["n_active"].tolist(), rec["n_low"].tolist(), rec["best"].tolist(), rec["dist"].max()))
    assert on == off
    assert rec["n_active"].tolist() == [6] * F and rec["n_low"].tolist() == [6] * F
    assert np.array_equal(rec["n_active"], mt["matched"].sum(axis=1))
    assert rec["best"].tolist() == [int(np.flatnonzero(mt["matched"][q])[0]) for q in range(F)]
    assert np.array_equal(rec["flags"], 3 * (mt["matched"] != 0)) and rec["first_outlier"] == -1
    assert (rec["votes"][mt["matched"] != 0] == 6).all() and rec["dist"].max() < THR_DEFAULT - MARGIN


# ---- 3. graph forms ----
@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_graph_forms_are_one_computation(srukf, synth, mode_name):
    """the outlier scene over 11 frames: the default graphs (8 + 1 + 1 + 1), eager launches and two calls of 5 + 6 frames leave bit-identical trajectory, state,
    match record, consensus record and matchPatches"""
    F, mode = F_MAX, getattr(srukf, "UPDATE_" + mode_name)
    out = []
    for name in ("default", "eager", "split"):
        f = _ransac_filter(srukf, synth, "outlier", F, THR, graph=0 if name == "eager" else None)
        t = np.vstack([f.run_images(0, 5, mode=mode), f.run_images(5, 6, mode=mode)]) if name == "split" else f.run_images(0, F, mode=mode)
        assert f.clamp_info() == (-1, -1)
        rec = f.get_image_ransac(0, F)
        out.append((t.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + _ransac_bytes(rec) + (_patch_bytes(f),))
        f.close()
    print("graph forms %s: n_active %s n_low %s first_outlier %d" % (mode_name, rec["n_active"].tolist(), rec["n_low"].tolist(), rec["first_outlier"]))
    assert out[0] == out[1] and out[0] == out[2]
    assert rec["first_outlier"] == 0 and (rec["n_active"][:6] >= 3).all()


# ---- 4. fewer than two active matches ----
@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_one_match_cannot_out_vote_itself(srukf, synth, mode_name):
    """a filter with one appearance record: the matched rows are untouched, the record says inlier = active, votes 0, best -1, dist 0, and the state is the run's
    with the switch off, bit for bit"""
    from test_gpu_unique import _rot
    F, mode, ONE = 4, getattr(srukf, "UPDATE_" + mode_name), 3
    cs = _case(srukf, synth, 8)
    res = []
    for on in (False, True):
        f = _filter(srukf, cs, F, appearance=False)
        patch, px = cs["recs"][ONE]
        f.set_landmark_appearance(ONE, patch, _rot(cs["pose"][3]), cs["pose"][:3], px)
        if on: f.images_ransac(True, 0.5)                        # (a threshold the match would fail against any hypothesis but its own)
        t = f.run_images(0, F, mode=mode)
        mt = f.get_image_matches(0, F)
        res.append((t.tobytes(),) + _state_bytes(f) + _record_bytes(mt) + (_patch_bytes(f),))
        if on: rec = f.get_image_ransac(0, F)
        assert f.clamp_info() == (-1, -1)
        f.close()
    assert res[0] == res[1]
    want = np.zeros((F, 8), dtype=np.int32); want[:, ONE] = 1
    assert np.array_equal(mt["matched"], want)                   # the one landmark with a record matches in every frame
    assert np.array_equal(rec["flags"], 3 * want) and not rec["votes"].any() and not rec["dist"].any()
    assert rec["best"].tolist() == [-1] * F and rec["n_active"].tolist() == [1] * F and rec["n_low"].tolist() == [1] * F and rec["first_outlier"] == -1


# ---- 5. with the map policy and the archive search behind the frames ----
@pytest.mark.parametrize("mode_name,checked", [("BATCHED", False), ("JOINT", True)])
def test_policy_sees_the_masked_matches(srukf, synth, mode_name, checked):
    """the policy record equals the twin's map_policy fed with matched & inlier: nMatchTimes of the displaced landmark does not move"""
    F, mode = 6, getattr(srukf, "UPDATE_" + mode_name)
    tw = _twin(srukf, synth, "outlier", mode, checked, THR)
    f = _ransac_filter(srukf, synth, "outlier", F, THR)
    f.images_policy(True, **PAR); f.set_policy_state(_seed())
    _run(f, 0, F, mode, checked)
    pol, rec = f.get_image_policy(0, F), f.get_image_ransac(0, F)
    assert f.clamp_info() == (-1, -1)
    f.close()
    assert _equal_records(rec, tw, F) == 0.0
    assert pol["verdict"].tolist() == tw["verdict"].tolist()
    for t in range(F):
        assert _summary_dict(pol, t) == tw["summary"][t], t
    assert _same_state(pol["state"], tw["state"])
    assert pol["state"]["nMatchTimes"][OUT_LM] == 0 and pol["state"]["nPredictTimes"][OUT_LM] == F
    assert [s["n_matches"] for s in tw["summary"]] == rec["n_low"].tolist()


def test_with_the_archive_search_and_the_policy(srukf, synth):
    """the searching frames with the consensus in them and the policy launch behind: the consensus and policy records are the step-wise twin's, the search record
    that of a twin that runs the frames one by one (the consensus on, the search off) with archive_search behind each"""
    import test_gpu_archive as ga
    import test_gpu_images_archive as gia
    F, mode = 6, srukf.UPDATE_BATCHED
    tw = _twin(srukf, synth, "outlier", mode, False, THR)
    arc_rec = gia._archive(srukf, synth)
    g = _ransac_filter(srukf, synth, "outlier", F, THR)
    ga.set_archive(g, arc_rec, list(gia.ALL))
    want = {k: [] for k in gia.KEYS}
    tg = []
    for t in range(F):
        tg.append(g.run_images(t, 1, mode=mode))
        for k, v in zip(gia.KEYS, g.archive_search(_outlier_case(srukf, synth)["frames"][t])): want[k].append(np.array(v, copy=True))
    want_state = _state_bytes(g)
    g.close()
    f = _ransac_filter(srukf, synth, "outlier", F, THR)
    ga.set_archive(f, arc_rec, list(gia.ALL))
    f.images_search_archive(True)
    f.images_policy(True, **PAR); f.set_policy_state(_seed())
    traj = f.run_images(0, F, mode=mode)
    rec, pol, arc = f.get_image_ransac(0, F), f.get_image_policy(0, F), f.get_image_archive(0, F)
    assert f.clamp_info() == (-1, -1)
    state = _state_bytes(f)
    f.close()
    assert _equal_records(rec, tw, F) == 0.0 and rec["first_outlier"] == 0
    assert pol["verdict"].tolist() == tw["verdict"].tolist() and _same_state(pol["state"], tw["state"])
    for k in gia.KEYS:
        assert arc[k].reshape(-1).tobytes() == np.array(want[k]).reshape(-1).tobytes(), k
    assert arc["hits"].tolist() == [3] * F
    assert traj.tobytes() == np.vstack(tg).tobytes() and state == want_state


# ---- 6. the threshold, the switch, their lifetime ----
def test_threshold_switch_and_lifetime(srukf, synth):
    """a threshold change between two runs over the same frames reaches the captured frames (the value lives on the device): first_outlier moves from -1 to 0; the
    switch is refused with a run in flight; off, the record stays and the frames are the plain ones (a twin with eager launches runs the same bits: no captured
    frame of the other kind was replayed); reset and a map change drop the record, the switch survives both"""
    cs = _outlier_case(srukf, synth)
    F = 6
    res = []
    for graph in (None, 0):
        f = _ransac_filter(srukf, synth, "outlier", F, 20.0, graph=graph)
        if graph is None:
            with pytest.raises(srukf.SrukfError) as e: f.get_image_ransac(0, F)                  # no such run yet
            assert e.value.rc == -5
            for bad in (0.0, -1.0, float("nan"), float("inf")):
                with pytest.raises(srukf.SrukfError) as e: f.images_ransac(True, bad)
                assert e.value.rc == -1, bad
            f.images_ransac(False, -1.0)                         # (switching off judges no threshold)
            f.images_ransac(True, 20.0)
        f.run_images(0, 3)
        r = f.get_image_ransac(0, 3)
        assert r["first_outlier"] == -1 and np.array_equal(r["n_low"], r["n_active"]) and (r["n_active"] >= 3).all()      # 20 px: the displaced match is an inlier
        assert f.get_image_matches(0, 3)["matched"][:, OUT_LM].all()
        with pytest.raises(srukf.SrukfError) as e: f.get_image_ransac(0, F + 1)
        assert e.value.rc == -2
        f.images_rewind()
        z0 = f.get_image_ransac(0, F)
        assert z0["first_outlier"] == -1 and not any(z0[k].any() for k in REC_KEYS)              # the rewound frames' rows do not stand
        f.images_ransac(True, THR)
        f.run_images(0, 3)
        r = f.get_image_ransac(0, 3)
        assert r["first_outlier"] == 0 and (r["n_low"] == r["n_active"] - 1).all()
        f.run_images_async(3, 1)
        for on in (False, True):
            with pytest.raises(srukf.SrukfError) as e: f.images_ransac(on, THR)                   # not while a run is in flight
            assert e.value.rc == -5
        f.synchronize()
        f.images_ransac(False)
        before = _ransac_bytes(f.get_image_ransac(0, F))
        t_off = f.run_images(4, 2)
        assert _ransac_bytes(f.get_image_ransac(0, F)) == before                                 # the record stays as it is
        mt = f.get_image_matches(4, 2)
        assert mt["matched"][:, OUT_LM].all()                    # the plain frames: the association's row goes to the update as it is
        res.append((t_off.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + (_patch_bytes(f),))
        if graph is None:
            # reset drops the images and the record; the switch survives
            f.images_ransac(True, THR)
            f.reset()
            with pytest.raises(srukf.SrukfError) as e: f.get_image_ransac(0, 1)
            assert e.value.rc == -5
        f.close()
    assert res[0] == res[1]
    # a map change drops the record; the switch survives it
    f = _ransac_filter(srukf, synth, "outlier", F, THR)
    f.run_images(0, 2)
    f.delete_landmark(7)
    with pytest.raises(srukf.SrukfError) as e: f.get_image_ransac(0, 1)
    assert e.value.rc == -5
    N = 7
    f.stage_sequence(cs["odo"][:3], np.zeros((2, 2 * N)), np.zeros((2, N), dtype=np.int32))
    f.stage_images(cs["frames"][:2])
    with pytest.raises(srukf.SrukfError) as e: f.get_image_ransac(0, 1)                          # staged again, no run yet
    assert e.value.rc == -5
    f.run_images(0, 2)
    r = f.get_image_ransac(0, 2)                                 # the switch is still on, with its threshold
    mt = f.get_image_matches(0, 2)
    print("after the map change: n_active %s n_low %s matched %s" % (r["n_active"].tolist(), r["n_low"].tolist(), mt["matched"].sum(axis=1).tolist()))
    assert r["flags"].shape == (2, N) and np.array_equal((r["flags"] & 1).sum(axis=1), r["n_active"]) and (r["n_active"] >= 2).all()
    assert np.array_equal(mt["matched"], (r["flags"] >> 1) & 1)  # the rows the update took are the consensus sets
    f.close()


def test_switch_survives_reset(srukf, synth):
    from test_gpu_unique import _rot
    cs = _outlier_case(srukf, synth)
    f = _ransac_filter(srukf, synth, "outlier", 2, THR)
    f.run_images(0, 2)
    want = _ransac_bytes(f.get_image_ransac(0, 2))
    f.reset()
    f.set_state(cs["X1"], cs["S1"])
    for k, (patch, px) in enumerate(cs["recs"]):
        if k != NO_RECORD: f.set_landmark_appearance(k, patch, _rot(cs["pose"][3]), cs["pose"][:3], px)
    f.stage_sequence(cs["odo"][:3], np.zeros((2, 16)), np.zeros((2, 8), dtype=np.int32))
    f.stage_images(cs["frames"][:2])
    f.run_images(0, 2)
    assert _ransac_bytes(f.get_image_ransac(0, 2)) == want and want[-1] == 0
    f.close()


# ---- 7. a flagged block ----
def test_flagged_block_leaves_a_zero_record(srukf, synth):
    """the shipped a1..a4 = 8 (tests/test_gpu_images.py) with the switch on: SRUKF_ERR_CLAMP_PENDING, X, S and the matchPatches as before the call, every record
    row zero, first_outlier -1.  The threshold is 1000 px: every match is an inlier and the frames' updates are the ones that flag without the switch (at 8 px
    this scene's consensus drops matches and the block does not flag)"""
    F = 6
    f = _ransac_filter(srukf, synth, "clean", F, 1000.0, which="shipped")
    before = _state_bytes(f) + (_patch_bytes(f),)
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F)
    assert e.value.rc == -7, str(e.value)
    frame, _ = f.clamp_info()
    assert 0 <= frame < F
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    r = f.get_image_ransac(0, F)
    assert r["first_outlier"] == -1 and not any(r[k].any() for k in REC_KEYS)
    f.close()


# ---- 8. every form of an image frame on one handle ----
CHECKED_PAR = dict(corr_threshold=0.8, ratio=0.8, exclusion=4, subpixel=True)      # not neutral: a plain frame replayed in a checked frame's place shows
FORM_ORDER = (0, 7, 1, 6, 2, 5, 3, 4)                            # checked | 2 search | 4 ransac: every bit alternates at least four times
F_FORMS = 9                                                      # one eight-frame graph and one single-frame graph


def _form_run(srukf, synth, f, form, mode):
    """switches of `form` set, frames 0..8 run: everything the run leaves and every record the form writes, as bytes; the block rewound behind it"""
    import test_gpu_images_archive as gia
    from test_gpu_images_checked import _check_bytes
    checked, search, ransac = bool(form & 1), bool(form & 2), bool(form & 4)
    f.images_search_archive(search)
    f.images_ransac(ransac, THR)
    t = f.run_images_checked(0, F_FORMS, mode=mode, **CHECKED_PAR) if checked else f.run_images(0, F_FORMS, mode=mode)
    assert f.clamp_info() == (-1, -1), form
    out = (t.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F_FORMS)) + (_patch_bytes(f),)
    if checked: out += _check_bytes(f.get_image_checks(0, F_FORMS))
    if search:
        arc = f.get_image_archive(0, F_FORMS)
        out += gia._rows(arc) + (arc["hits"].tobytes(),)
    if ransac: out += _ransac_bytes(f.get_image_ransac(0, F_FORMS))
    f.images_rewind()
    return out


def _form_filter(srukf, synth):
    import test_gpu_archive as ga
    import test_gpu_images_archive as gia
    f = _filter(srukf, _outlier_case(srukf, synth), F_FORMS)
    ga.set_archive(f, gia._archive(srukf, synth), list(gia.ALL))
    return f


@functools.lru_cache(maxsize=None)
def _fresh_form(srukf, synth, form, mode):
    """a handle that runs nothing but this form; computed once per form and mode"""
    f = _form_filter(srukf, synth)
    out = _form_run(srukf, synth, f, form, mode)
    f.close()
    return out


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_every_form_on_one_handle_is_the_fresh_handles(srukf, synth, mode_name):
    """the outlier scene, 9 frames (an eight-frame graph and a single frame), the archive set: the eight combinations of checked, search and ransac run one
    behind the other on ONE handle, each rewound, leave what a fresh handle that runs only that form leaves, byte for byte — trajectory, state, match record,
    matchPatches and every record the form writes — and again in a second round, every graph captured by then: no form replays a frame captured for another"""
    mode = getattr(srukf, "UPDATE_" + mode_name)
    f = _form_filter(srukf, synth)
    for rnd in (0, 1):
        for form in FORM_ORDER:
            got, want = _form_run(srukf, synth, f, form, mode), _fresh_form(srukf, synth, form, mode)
            assert len(got) == len(want) and got == want, (rnd, form, [i for i, (a, b) in enumerate(zip(got, want)) if a != b])
    f.close()
    # the forms differ where they should: a table index that fell back to another form's graph on both sides would still have passed above
    base = _fresh_form(srukf, synth, 0, mode)
    for form in (1, 4):
        assert _fresh_form(srukf, synth, form, mode)[:8] != base[:8], form


# ---- 9. the step-wise consensus beyond one stride of the votes body ----
@pytest.mark.parametrize("fast", [0, 1])
def test_stepwise_consensus_at_260_landmarks(srukf, synth, oracle, fast):
    """N = 260 against tests/np_ransac.py: the votes body strides j by 256 and nothing else in the suite has N > 256.  Seed 9's first frame from the scene's own
    start state: chosen with the restatement on the CPU so that no pair lies within DIST_TOL of the threshold (the nearest: 0.06 px)"""
    N, seed = 260, 9
    p = synth.scene_params()
    sc = synth.make_scene(N, 3, seed=seed, p=p)
    o = oracle.Oracle(N, p); o.set_state(sc["X0"], sc["S0"])
    o.predict_motion(sc["odo"][0], sc["odo"][1])
    ho, _, viso = o.predict_measurement()
    f = srukf.Filter(N, p); f.set_state(sc["X0"], sc["S0"]); f.debug_set("step_fast", fast)
    f.predict_motion(sc["odo"][0], sc["odo"][1])
    if fast: f.predict_motion_next(sc["odo"][1], sc["odo"][2])
    _, _, vis = f.predict_measurement()
    assert np.array_equal(vis, viso)
    for kind in KINDS:
        z, m, moved = make_z(sc, 0, ho, viso, kind, seed)
        res = np_ransac.consensus(oracle, o, p, z, m)
        A = np.flatnonzero(res["active"])
        assert A.max() >= 256 and A.size > 200                   # hypotheses and pairs of the second stride take part
        inl, votes, dist, best = f.ransac_consensus(z, m, 8.0)
        err, share = np_ransac.compare(res, inl, votes, dist, best, 8.0, DIST_TOL)
        print("ransac N=260 path=%s %s: M=%d moved=%d best=%d votes=%d max|ddist|=%.3e" % ("fast" if fast else "slow", kind, A.size, len(moved), best, votes[best], err))
        assert share == 0.0 and err <= DIST_TOL
        assert np.array_equal(votes, res["votes"]) and np.array_equal(inl, res["inlier"]) and best == res["best"]
        assert kind == "near" or set(np.flatnonzero(inl)).isdisjoint(moved)
    f.close()
