"""GPU tests of the rescue gate (srukf_rescue_gate / srukf_images_rescue_gate / srukf_get_image_rescue, k_rescue_gate / k_rescue_gate_staged;
csrc/srukf_rescue.hip, srukf_images.hip, srukf_snapshot.hip): the step-wise front against the CPU oracle and tests/np_rescue.py, the staged front
against a twin driven step by step (... -> ransac_consensus -> update -> rescue_gate), the stops of a block on "a match would be rescued", the graph forms and the
switch's lifetime.

Step-wise cases: tests/test_gpu_ransac.py's scenes and make_z, seed 3, kinds "fifth" and "near", the matches split as test_repredict_and_second_update_equal_oracle
splits them (even landmarks are the low-innovation inliers and keep the scene's own pixel, odd ones are the candidates).  Chosen on the CPU with the oracle's filter:
N = 20: 6 / 9 of 10 candidates rescued, N = 50: 19 / 21 of 25, no candidate's distance within 0.55 of the threshold.

Staged scenes: tests/test_gpu_images_ransac.py's outlier scene (N = 8, landmark 0's patch cut (7, -8) px aside).  Chosen on the CPU with the oracle's association
(oracle.warp_patch / associate_one around the oracle's filter, tests/np_ransac.py's consensus, the update with the consensus set, a fresh oracle's prediction from
the posterior, tests/np_rescue.py), BATCHED updates:
  scene A, consensus threshold 4.8 px (§24's): frames 0 .. 5 each drop landmark 0, whose distance from the posterior is 5.304, 4.925, 4.469, 4.771, 5.698, 6.906.
    chi2 4.0: never rescued (first_outlier 0, first_rescue -1); chi2 4.6: first rescue in frame 2; chi2 5.1: in frame 1; the default 5.99: in frame 0.
  scene B, consensus threshold 5.25 px, 9 frames: landmark 0 is an inlier in frames 0 .. 3 and 5 .. 7 (nearest pair distance to the threshold: 0.018 px), dropped in
    frame 4 at distance 5.168, and frame 8 drops landmarks 3, 4, 6 at 3.365.  chi2 4.3: first_outlier 4, first_rescue 8.  (The device's association finds one clean
    match more than the CPU chain's, six active matches for its five, so a frame between may drop a match too, far outside chi2: on the MI355X frame 5, at 6.755.)
Every margin is above 0.1, seven orders above what 1e-8 px can move a distance.  Integers and records are compared as integers and bytes; the twin's preconditions
are asserted on the twin alone, before any comparison."""
import functools

import numpy as np
import pytest

import np_rescue
from test_gpu_images import F_MAX, _filter, _patch_bytes, _record_bytes, _state_bytes
from test_gpu_images_ransac import NEUTRAL, OUT_LM, THR, _outlier_case, _ransac_bytes, _scene
from test_gpu_policy import PAR, _seed
from test_gpu_ransac import F0, _predict, _warm_state, make_z

pytestmark = pytest.mark.gpu

TOL_H, TOL_SI = 1e-8, 1e-9                                       # test_repredict_and_second_update_equal_oracle's bounds
CHI2 = np_rescue.CHI2
CHI2_MARGIN = 1e-6
SEED, KINDS_R = 3, ("fifth", "near")
THR_B, F_B = 5.25, 9
CHI2_NEVER, CHI2_K2, CHI2_K1, CHI2_B = 4.0, 4.6, 5.1, 4.3
A_DIST = (5.304331, 4.925112, 4.469088, 4.770608, 5.698311, 6.90633)      # scene A, landmark 0, from the CPU chain
RQ_KEYS = ("flags", "h2", "Si2", "chi2", "n_cand", "n_high")


def _rescue_bytes(rec):
    return tuple(rec[k].tobytes() for k in RQ_KEYS) + (rec["first_rescue"],)


# ---- 1. the step-wise front against the oracle ----
def _split(sc, t, h, vis, kind):
    """make_z's displaced measurements; A = matched and visible; even landmarks are the low-innovation inliers (with the scene's own pixel), odd ones the candidates"""
    z, m, moved = make_z(sc, t, h, vis, kind, SEED)
    act = ((m != 0) & (np.asarray(vis) != 0)).astype(np.int32)
    low = act.copy(); low[1::2] = 0
    for k in np.flatnonzero(low): z[2 * k:2 * k + 2] = sc["z"][t][2 * k:2 * k + 2]
    return z, act, low


@pytest.mark.parametrize("N", [20, 50])
@pytest.mark.parametrize("fast", [0, 1])
def test_stepwise_gate_equals_oracle(srukf, synth, oracle, fast, N):
    """N = 20: Na + 1 = 130 items, one trip, the full-rank form; N = 50: 310 items, a partial second trip, the rank-aware form and the fast step path"""
    p = synth.scene_params()
    sc = synth.make_scene(N, F0 + 4, seed=SEED, p=p)
    X3, S3 = _warm_state(srukf, sc, N, p)
    for kind in KINDS_R:
        hs = []
        for who in ("gate", "repredict"):
            f = srukf.Filter(N, p); f.set_state(X3, S3); f.debug_set("step_fast", fast)
            h, Si, vis = _predict(f, sc, F0, fast)
            z, act, low = _split(sc, F0, h, vis, kind)
            f.update(z, low)
            assert f.debug_get("step_fast") == (fast if N >= 50 else 0)
            if who == "gate":
                r = f.rescue_gate(z, act, low)
                Xp, Sp = f.get_state()
            else:
                hr, Sir, visr = f.repredict_measurement()
                assert np.array_equal(f.get_state()[0], Xp)               # the same posterior on both handles
            hs.append((h, vis))
            f.close()
        assert np.array_equal(hs[0][0], hs[1][0])
        o = oracle.Oracle(N, p); o.set_state(Xp, Sp)
        o.predict_motion(np.zeros(3), np.zeros(3))
        ho, Sio, viso = o.predict_measurement()
        fo, do = np_rescue.gate(z, act, low, ho, Sio, viso)
        cand = (fo & 1) != 0
        formed = cand & (do > 0)
        # the case's preconditions, on the oracle's values: no distance near the threshold, both outcomes present
        assert formed.any() and np.abs(do[formed] - CHI2).min() >= CHI2_MARGIN
        assert ((fo & 2) != 0).sum() >= 1 and (cand & ((fo & 2) == 0)).sum() >= 1 and cand.sum() == act.sum() - low.sum()
        c2 = np.repeat(cand, 2)
        eh = np.abs(r["h2"] - ho)[c2].max()
        es = np.abs(np.abs(r["Si2"]) - np.abs(Sio))[cand].max()
        vis_gate = (r["h2"].reshape(N, 2) != 0).all(axis=1)
        fr, _ = np_rescue.gate(z, act, low, hr, Sir, visr)
        dh, ds = np.abs(r["h2"] - hr)[c2].max(), np.abs(np.abs(r["Si2"]) - np.abs(Sir))[cand].max()
        print(f"rescue gate N={N} path={'fast' if fast else 'slow'} {kind}: candidates {int(cand.sum())} rescued {r['n_high']} | vs oracle |dh|={eh:.3e} |d|Si||={es:.3e} "
              f"| vs repredict_measurement |dh|={dh:.3e} |d|Si||={ds:.3e} | nearest distance to chi2 {np.abs(do[formed] - CHI2).min():.3f}")
        assert eh < TOL_H and es < TOL_SI
        assert np.array_equal(r["flags"], fo) and r["n_high"] == int(((fo & 2) != 0).sum())
        assert np.array_equal(r["flags"], fr) and np.array_equal(vis_gate[cand], visr[cand] != 0)
        # rows of non-candidates read zero
        assert not r["h2"][~c2].any() and not r["Si2"][~cand].any() and not r["chi2"][~cand].any() and not r["flags"][~cand].any()
        assert np.abs(r["chi2"] - do)[formed].max() < 1e-6


@pytest.mark.parametrize("fast", [0, 1])
def test_stepwise_gate_is_read_only(srukf, synth, fast):
    """three frames with the gate behind every update against three frames without it: every frame's prediction, the state bytes and the step path's counters are
    equal (the gate does not un-chain the next frame); a second call returns the same bytes; repredict_measurement and a second update behind the gate give the
    bits they give without it"""
    N = 50
    p = synth.scene_params()
    sc = synth.make_scene(N, F0 + 6, seed=SEED, p=p)
    X3, S3 = _warm_state(srukf, sc, N, p)
    out = []
    for with_gate in (0, 1):
        f = srukf.Filter(N, p); f.set_state(X3, S3); f.debug_set("step_fast", fast)
        seen = []
        for t in range(F0, F0 + 3):
            h, Si, vis = _predict(f, sc, t, fast)
            z, act, low = _split(sc, t, h, vis, "fifth")
            seen.append(h.tobytes() + Si.tobytes() + vis.tobytes())
            f.update(z, low)
            if with_gate:
                r = f.rescue_gate(z, act, low)
                r2 = f.rescue_gate(z, act, low)                  # phase and state as they were: legal again, the same answer
                assert all(r[k].tobytes() == r2[k].tobytes() for k in ("flags", "h2", "Si2", "chi2")) and r["n_high"] == r2["n_high"] and (r["flags"] & 1).any()
                with pytest.raises(srukf.SrukfError) as e: f.ransac_consensus(z, act)      # the frame is over, as without the gate
                assert e.value.rc == -5
        counts = (f.debug_get("step_fast"), f.debug_get("step_slow"))
        mid = _state_bytes(f)
        t = F0 + 3
        h, Si, vis = _predict(f, sc, t, fast)
        z, act, low = _split(sc, t, h, vis, "fifth")
        f.update(z, low)
        if with_gate: r = f.rescue_gate(z, act, low)
        h2, Si2, vis2 = f.repredict_measurement()
        f.update(z, ((act != 0) & (low == 0)).astype(np.int32))
        out.append((seen, counts, mid, h.tobytes(), h2.tobytes() + Si2.tobytes() + vis2.tobytes(), _state_bytes(f)))
        f.close()
    assert out[0] == out[1]
    assert out[0][1][0] == 3 * fast


def test_stepwise_gate_refusals(srukf, synth):
    N = 8
    p = synth.scene_params()
    sc = synth.make_scene(N, 3, seed=0, p=p)
    f = srukf.Filter(N, p); f.set_state(sc["X0"], sc["S0"])
    z, m = sc["z"][0], sc["matched"][0].astype(np.int32)
    low = m.copy(); low[1::2] = 0
    with pytest.raises(srukf.SrukfError) as e: f.rescue_gate(z, m, low)      # no update of this frame
    assert e.value.rc == -5
    f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement()
    with pytest.raises(srukf.SrukfError) as e: f.rescue_gate(z, m, low)
    assert e.value.rc == -5
    f.update(z, low)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(srukf.SrukfError) as e: f.rescue_gate(z, m, low, chi2=bad)
        assert e.value.rc == -1, bad
    r = f.rescue_gate(z, m, low)
    assert (r["flags"] & 1).sum() == m.sum() - low.sum()
    # frames without candidates: every match a low inlier, none, fewer than two matches
    one = np.zeros(N, dtype=np.int32); one[0] = 1
    for mm, ll in ((m, m), (m, np.zeros(N, dtype=np.int32)), (one, np.zeros(N, dtype=np.int32))):
        r = f.rescue_gate(z, mm, ll)
        assert not r["flags"].any() and not r["h2"].any() and not r["Si2"].any() and not r["chi2"].any() and r["n_high"] == 0
    f.predict_motion(sc["odo"][1], sc["odo"][2])
    with pytest.raises(srukf.SrukfError) as e: f.rescue_gate(z, m, low)      # the update belongs to the frame before
    assert e.value.rc == -5
    f.close()


# ---- 2. the staged front against the step-wise one ----
def _run(f, first, count, mode, checked=False):
    return f.run_images_checked(first, count, mode=mode, **NEUTRAL) if checked else f.run_images(first, count, mode=mode)


def _gate_filter(srukf, synth, F, thr, chi2, graph=None, which="scene", scene="outlier"):
    f = _filter(srukf, _scene(srukf, synth, scene, which), F, graph=graph)
    f.images_ransac(True, thr)
    if chi2 is not None: f.images_rescue_gate(True, chi2)
    return f


@functools.lru_cache(maxsize=None)
def _twin(srukf, synth, mode, checked, thr, chi2, F):
    """the step-wise route: ... -> ransac_consensus -> update with the consensus set -> rescue_gate, no second update"""
    cs = _outlier_case(srukf, synth)
    N = 8
    g = _filter(srukf, cs)
    out = {k: [] for k in RQ_KEYS + ("n_active", "n_low")}
    for t in range(F):
        g.predict_motion(cs["odo"][t], cs["odo"][t + 1])
        h, _, vis = g.predict_measurement()
        if checked:
            r = g.associate_checked(cs["frames"][t], **NEUTRAL); z, m = r["z"], r["matched"]
        else:
            z, m, _ = g.associate(cs["frames"][t])
        z, m = np.array(z, copy=True), np.array(m, dtype=np.int32, copy=True)
        act = ((m != 0) & (np.asarray(vis) != 0)).astype(np.int32)
        if act.sum() >= 2:
            inl, _, _, _ = g.ransac_consensus(z, m, thr)
            inl = (np.array(inl, dtype=np.int32) != 0).astype(np.int32)
        else:
            inl = act.copy()
        used = (m * inl).astype(np.int32) if act.sum() >= 2 else m
        if mode == srukf.UPDATE_JOINT: g.update_joint(z, used)
        else: g.update(z, used, mode=srukf.UPDATE_BATCHED)
        r = g.rescue_gate(z, act, inl, chi2)
        formed = r["chi2"] > 0
        assert not formed.any() or np.abs(r["chi2"][formed] - chi2).min() >= CHI2_MARGIN, (t, r["chi2"])
        for k in ("flags", "h2", "Si2", "chi2"): out[k].append(np.array(r[k], copy=True))
        out["n_cand"].append(int((r["flags"] & 1).sum())); out["n_high"].append(r["n_high"])
        out["n_active"].append(int(act.sum())); out["n_low"].append(int((act & inl).sum()))
    g.close()
    out = {k: np.array(v) for k, v in out.items()}
    out["n_cand"], out["n_high"] = out["n_cand"].astype(np.int32), out["n_high"].astype(np.int32)
    high = np.flatnonzero(out["n_high"] > 0)
    out["first_rescue"] = int(high[0]) if high.size else -1
    print("twin thr %.2f chi2 %.2f: active %s low %s candidates %s rescued %s distances %s" % (thr, chi2, out["n_active"].tolist(), out["n_low"].tolist(),
          out["n_cand"].tolist(), out["n_high"].tolist(), [np.round(c[c > 0], 4).tolist() for c in out["chi2"]]))
    return out


@pytest.mark.parametrize("thr,chi2,F", [(THR, CHI2_NEVER, 6), (THR, CHI2_K2, 6), (THR_B, CHI2_B, F_B)])
@pytest.mark.parametrize("mode_name,checked", [("BATCHED", False), ("JOINT", False), ("BATCHED", True), ("JOINT", True)])
def test_staged_against_the_stepwise_front(srukf, synth, mode_name, checked, thr, chi2, F):
    """every row of the gate's record byte-equal to the twin's; trajectory, state, match record, consensus record and matchPatches byte-equal to the same run with
    the gate off.  BATCHED: the runs are the ones the CPU chain chose — a run whose frames drop a match and rescue none, a run with the first rescue in a known frame"""
    mode = getattr(srukf, "UPDATE_" + mode_name)
    tw = _twin(srukf, synth, mode, checked, thr, chi2, F)
    res = []
    for on in (True, False):
        f = _gate_filter(srukf, synth, F, thr, chi2 if on else None)
        t = _run(f, 0, F, mode, checked)
        assert f.clamp_info() == (-1, -1)
        rs = f.get_image_ransac(0, F)
        res.append((t.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + _ransac_bytes(rs) + (_patch_bytes(f),))
        if on: rec = f.get_image_rescue(0, F)
        else:
            with pytest.raises(srukf.SrukfError) as e: f.get_image_rescue(0, F)      # no run with the gate in it
            assert e.value.rc == -5
        f.close()
    assert res[0] == res[1]
    print("%s%s thr %.2f chi2 %.2f: candidates %s rescued %s first_outlier %d first_rescue %d" % (mode_name, " checked" if checked else "", thr, chi2,
          rec["n_cand"].tolist(), rec["n_high"].tolist(), rs["first_outlier"], rec["first_rescue"]))
    assert np.array_equal(rs["n_active"], tw["n_active"]) and np.array_equal(rs["n_low"], tw["n_low"])
    for k in RQ_KEYS:
        assert rec[k].tobytes() == tw[k].tobytes(), (k, rec[k], tw[k])
    assert rec["first_rescue"] == tw["first_rescue"]
    has = (rs["n_active"] >= 2) & (rs["n_low"] > 0) & (rs["n_low"] < rs["n_active"])
    assert np.array_equal(rec["n_cand"], np.where(has, rs["n_active"] - rs["n_low"], 0))
    assert np.array_equal(rec["flags"] & 1, np.where(has[:, None], (rs["flags"] & 3) == 1, 0))
    if mode_name == "BATCHED":                                   # what the CPU chain chose the runs for
        if thr == THR:
            assert rs["first_outlier"] == 0 and (rec["n_cand"] == 1).all() and (rec["flags"][:, OUT_LM] & 1).all()
            # (the CPU chain is the oracle's from the scene's start on and associates five clean matches where the device finds six: its distances are the device's
            #  to ~4e-4; 1e-2 is a tenth of the smallest margin the chi2 values were chosen with)
            assert np.abs(rec["chi2"][:, OUT_LM] - np.array(A_DIST)).max() < 1e-2
            assert rec["first_rescue"] == (-1 if chi2 == CHI2_NEVER else 2)
            if chi2 == CHI2_NEVER: assert not rec["n_high"].any()
        else:
            # (frames 0 .. 3 drop nothing, frame 4 drops landmark 0 and does not rescue it, frame 8 is the first to rescue; the device associates one clean match
            #  more than the CPU chain, so the counts of the frames between are its own: nothing of them is asserted but that they rescue nothing)
            assert rs["first_outlier"] == 4 and rec["first_rescue"] == 8 and rec["n_cand"][4] == 1 and rec["flags"][4, OUT_LM] == 1
            assert not rec["n_cand"][:4].any() and not rec["n_high"][:8].any() and rec["n_high"][8] >= 1
            assert abs(rec["chi2"][4, OUT_LM] - 5.16783) < 1e-2 and np.abs(rec["chi2"][8][rec["flags"][8] == 3] - 3.365).max() < 1e-2


# ---- 3. stops ----
def _held(f, keep):
    out = _state_bytes(f) + (_patch_bytes(f),) + _record_bytes(f.get_image_matches(0, keep))
    return out + _ransac_bytes(f.get_image_ransac(0, keep)) + _rescue_bytes(f.get_image_rescue(0, keep))


def _rows_zero(f, first, count):
    if count < 1: return True
    a, b = f.get_image_ransac(first, count), f.get_image_rescue(first, count)
    return (not any(a[k].any() for k in ("flags", "votes", "dist", "best", "n_active", "n_low")) and a["first_outlier"] == -1 and
            not any(b[k].any() for k in RQ_KEYS) and b["first_rescue"] == -1)


def test_never_rescued_all_frames_stand(srukf, synth):
    """scene A at chi2 4.0 with snapshots on: first_outlier 0, first_rescue -1, the latch never closes: the slots hold the starts of the last two frames.
    (The stops are tested with BATCHED updates, which the CPU chain chose chi2 for; JOINT frames with the gate: section 2 and the forms below)"""
    F, mode = 6, srukf.UPDATE_BATCHED
    tw = _twin(srukf, synth, mode, False, THR, CHI2_NEVER, F)
    assert tw["first_rescue"] == -1 and (tw["n_cand"] == 1).all()
    f = _gate_filter(srukf, synth, F, THR, CHI2_NEVER)
    f.images_snapshots(True)
    f.run_images(0, F, mode=mode)
    assert f.get_image_ransac(0, F)["first_outlier"] == 0 and f.get_image_rescue(0, F)["first_rescue"] == -1
    assert f.get_image_snapshots() == (4, 5)
    after = _held(f, F)
    f.images_resume(F)                                           # all frames stand
    assert _held(f, F) == after
    f.close()


@pytest.mark.parametrize("thr,chi2,F,k", [(THR, CHI2_K2, 6, 2), (THR, CHI2_K1, 6, 1), (THR_B, CHI2_B, F_B, 8)])
def test_resume_at_the_first_rescue(srukf, synth, thr, chi2, F, k):
    """first_rescue == k (asserted): slot k & 1 holds the state frame k started from and images_resume(k) leaves what a fresh handle's run of k frames leaves, byte
    for byte.  Scene B: first_outlier == 4 != k, and images_resume(4) is SRUKF_ERR_SEQUENCE and leaves everything as it was (the frames 4 .. 7 stand: no slot holds
    the start of frame 4).  In scene A first_outlier is the block's first frame, where a resume is the rewind"""
    mode = srukf.UPDATE_BATCHED
    tw = _twin(srukf, synth, mode, False, thr, chi2, F)
    assert tw["first_rescue"] == k
    f = _gate_filter(srukf, synth, F, thr, chi2)
    f.images_snapshots(True)
    t = f.run_images(0, F, mode=mode)
    fo, fr = f.get_image_ransac(0, F)["first_outlier"], f.get_image_rescue(0, F)["first_rescue"]
    tags = f.get_image_snapshots()
    print("thr %.2f chi2 %.2f: first_outlier %d first_rescue %d tags %s" % (thr, chi2, fo, fr, tags))
    assert fr == k and 0 <= fo <= k
    assert tags[k & 1] == k and tags[(k - 1) & 1] == k - 1       # frame k + 1's launch saw the stop: the other slot was not overwritten
    if thr == THR_B:
        assert fo == 4
        before = _held(f, F)
        with pytest.raises(srukf.SrukfError) as e: f.images_resume(fo)
        assert e.value.rc == -5
        assert _held(f, F) == before
    else:
        assert fo == 0
    f.images_resume(k)
    got = (t[:k].tobytes(),) + _held(f, k)
    assert _rows_zero(f, k, F - k)
    f.close()
    g = _gate_filter(srukf, synth, F, thr, chi2)
    t = g.run_images(0, k, mode=mode)
    want = (t.tobytes(),) + _held(g, k)
    g.close()
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


def test_gate_off_the_latch_is_section_25s(srukf, synth):
    """tests/test_gpu_images_resume.py's outlier stop in front of a frame, on a handle that had the gate on and off again: first_outlier == k stops the block"""
    import test_gpu_images_resume as gr
    F, mode = 6, srukf.UPDATE_BATCHED
    k, thr = gr._outlier_threshold(srukf, synth, mode)
    f = _gate_filter(srukf, synth, F, thr, CHI2, scene="clean")
    f.images_snapshots(True)
    f.run_images(0, F, mode=mode)
    f.images_rewind()
    f.images_rescue_gate(False)
    t = f.run_images(0, F, mode=mode)
    assert f.get_image_ransac(0, F)["first_outlier"] == k
    tags = f.get_image_snapshots()
    assert tags[k & 1] == k and tags[(k - 1) & 1] == k - 1
    f.images_resume(k)
    got = (t[:k].tobytes(),) + gr._held(f, k, ransac=True)
    assert gr._rows_zero(f, k, F - k, ransac=True)
    f.close()
    g = gr._ransac_filter(srukf, synth, "clean", F, thr)
    t = g.run_images(0, k, mode=mode)
    want = (t.tobytes(),) + gr._held(g, k, ransac=True)
    g.close()
    assert got == want


@pytest.mark.parametrize("chi2,kw", [(CHI2_K1, {}), (CHI2_K2, dict(min_predictions=9)), (CHI2_NEVER, {})])
def test_policy_and_rescue_stops_in_one_block(srukf, synth, chi2, kw):
    """the smaller of first_change + 1 and first_rescue wins"""
    F, mode = 6, srukf.UPDATE_BATCHED

    def make():
        h = _gate_filter(srukf, synth, F, THR, chi2)
        h.images_policy(True, **dict(PAR, **kw)); h.set_policy_state(_seed())
        return h

    f = make()
    f.images_snapshots(True)
    t = f.run_images(0, F, mode=mode)
    fc, fr = f.get_image_policy(0, F)["first_change"], f.get_image_rescue(0, F)["first_rescue"]
    assert fc >= 0 and fr == {CHI2_K1: 1, CHI2_K2: 2, CHI2_NEVER: -1}[chi2], (fc, fr)
    stop = fc + 1 if fr < 0 else min(fc + 1, fr)
    tags = f.get_image_snapshots()
    print("chi2 %.2f: first_change %d first_rescue %d stop %d tags %s" % (chi2, fc, fr, stop, tags))
    assert 0 < stop < F and tags[stop & 1] == stop

    def held(h):
        r = h.get_image_policy(0, stop)
        return _held(h, stop) + (r["verdict"].tobytes(), r["summary"].tobytes(), r["state"].tobytes(), r["first_change"])

    f.images_resume(stop)
    got = (t[:stop].tobytes(),) + held(f)
    assert _rows_zero(f, stop, F - stop)
    f.close()
    g = make()
    t = g.run_images(0, stop, mode=mode)
    want = (t.tobytes(),) + held(g)
    g.close()
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


# ---- 4. forms and lifetime ----
@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_graph_forms_are_one_computation(srukf, synth, mode_name):
    """scene A over 11 frames: the default graphs (8 + 1 + 1 + 1), eager launches and two calls of 5 + 6 frames leave bit-identical trajectory, state, records"""
    F, mode = F_MAX, getattr(srukf, "UPDATE_" + mode_name)
    out = []
    for name in ("default", "eager", "split"):
        f = _gate_filter(srukf, synth, F, THR, CHI2_K2, graph=0 if name == "eager" else None)
        t = np.vstack([f.run_images(0, 5, mode=mode), f.run_images(5, 6, mode=mode)]) if name == "split" else f.run_images(0, F, mode=mode)
        assert f.clamp_info() == (-1, -1)
        rec = f.get_image_rescue(0, F)
        out.append((t.tobytes(),) + _held(f, F))
        f.close()
    print("graph forms %s: candidates %s rescued %s" % (mode_name, rec["n_cand"].tolist(), rec["n_high"].tolist()))
    assert out[0] == out[1] and out[0] == out[2]
    assert rec["n_cand"][:6].tolist() == [1] * 6


CHECKED_PAR = dict(corr_threshold=0.8, ratio=0.8, exclusion=4, subpixel=True)
FORM_ORDER = (0, 7, 1, 6, 2, 5, 3, 4)                            # checked | 2 search | 4 snap, every one with ransac and rescue
F_FORMS = 9


def _form_filter(srukf, synth):
    import test_gpu_archive as ga
    import test_gpu_images_archive as gia
    f = _filter(srukf, _outlier_case(srukf, synth), F_FORMS)
    ga.set_archive(f, gia._archive(srukf, synth), list(gia.ALL))
    f.images_ransac(True, THR); f.images_rescue_gate(True, CHI2_K2)
    return f


def _form_run(srukf, synth, f, form, mode):
    import test_gpu_images_archive as gia
    from test_gpu_images_checked import _check_bytes
    checked, search, snap = bool(form & 1), bool(form & 2), bool(form & 4)
    f.images_search_archive(search)
    f.images_snapshots(snap)
    t = f.run_images_checked(0, F_FORMS, mode=mode, **CHECKED_PAR) if checked else f.run_images(0, F_FORMS, mode=mode)
    assert f.clamp_info() == (-1, -1), form
    out = (t.tobytes(),) + _held(f, F_FORMS)
    if checked: out += _check_bytes(f.get_image_checks(0, F_FORMS))
    if search:
        arc = f.get_image_archive(0, F_FORMS)
        out += gia._rows(arc) + (arc["hits"].tobytes(),)
    if snap: out += (f.get_image_snapshots(),)
    f.images_rewind()
    return out


@functools.lru_cache(maxsize=None)
def _fresh_form(srukf, synth, form, mode):
    f = _form_filter(srukf, synth)
    out = _form_run(srukf, synth, f, form, mode)
    f.close()
    return out


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_every_form_with_the_gate_on_one_handle_is_the_fresh_handles(srukf, synth, mode_name):
    """the eight forms with the gate (x checked, search, snap), 9 frames each, one behind the other on ONE handle, each rewound: each leaves what a fresh handle that
    runs only that form leaves, byte for byte, and again in a second round, every graph captured by then"""
    mode = getattr(srukf, "UPDATE_" + mode_name)
    f = _form_filter(srukf, synth)
    for rnd in (0, 1):
        for form in FORM_ORDER:
            got, want = _form_run(srukf, synth, f, form, mode), _fresh_form(srukf, synth, form, mode)
            assert len(got) == len(want) and got == want, (rnd, form, [i for i, (a, b) in enumerate(zip(got, want)) if a != b])
    f.close()
    if mode_name == "BATCHED":
        assert _fresh_form(srukf, synth, 4, mode)[-1] == (2, 1)   # snapshots with the gate: the latch closed behind the rescue in frame 2


def test_chi2_switch_and_lifetime(srukf, synth):
    """chi2 changed between two runs over the same frames reaches the captured frames: first_rescue moves; the switch is refused in flight and survives reset and a
    map change, which drop the record; with images_ransac off a run issues the plain frames"""
    cs = _outlier_case(srukf, synth)
    F = 6
    f = _gate_filter(srukf, synth, F, THR, CHI2_K2)
    with pytest.raises(srukf.SrukfError) as e: f.get_image_rescue(0, F)      # no such run yet
    assert e.value.rc == -5
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(srukf.SrukfError) as e: f.images_rescue_gate(True, bad)
        assert e.value.rc == -1, bad
    f.images_rescue_gate(False, -1.0)                            # (switching off judges no threshold)
    f.images_rescue_gate(True, CHI2_K2)
    f.run_images(0, F)
    assert f.get_image_rescue(0, F)["first_rescue"] == 2
    with pytest.raises(srukf.SrukfError) as e: f.get_image_rescue(0, F + 1)
    assert e.value.rc == -2
    f.images_rewind()
    z0 = f.get_image_rescue(0, F)
    assert z0["first_rescue"] == -1 and not any(z0[k].any() for k in RQ_KEYS)      # the rewound frames' rows do not stand
    for chi2, want in ((CHI2_K1, 1), (CHI2, 0), (CHI2_NEVER, -1)):
        f.images_rescue_gate(True, chi2)
        f.run_images(0, F)                                       # the frames captured above, replayed
        assert f.get_image_rescue(0, F)["first_rescue"] == want, chi2
        f.images_rewind()
    f.run_images_async(0, 1)
    for on in (False, True):
        with pytest.raises(srukf.SrukfError) as e: f.images_rescue_gate(on, CHI2)      # not while a run is in flight
        assert e.value.rc == -5
    f.synchronize()
    # with images_ransac off the gate adds nothing: the bits of a handle that never had the switch
    f.images_ransac(False)
    before = _rescue_bytes(f.get_image_rescue(0, F))
    t = f.run_images(1, F - 1)
    assert _rescue_bytes(f.get_image_rescue(0, F)) == before
    got = (t.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + (_patch_bytes(f),)
    g = _gate_filter(srukf, synth, F, THR, None)
    g.run_images(0, 1)
    g.images_ransac(False)
    t = g.run_images(1, F - 1)
    want = (t.tobytes(),) + _state_bytes(g) + _record_bytes(g.get_image_matches(0, F)) + (_patch_bytes(g),)
    g.close()
    assert got == want
    # reset drops the images and the record; the switch survives
    f.images_ransac(True, THR)
    f.reset()
    with pytest.raises(srukf.SrukfError) as e: f.get_image_rescue(0, 1)
    assert e.value.rc == -5
    from test_gpu_unique import _rot
    from test_gpu_images import NO_RECORD
    f.set_state(cs["X1"], cs["S1"])
    for k, (patch, px) in enumerate(cs["recs"]):
        if k != NO_RECORD: f.set_landmark_appearance(k, patch, _rot(cs["pose"][3]), cs["pose"][:3], px)
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 16)), np.zeros((F, 8), dtype=np.int32))
    f.stage_images(cs["frames"][:F])
    f.run_images(0, F)
    assert f.get_image_rescue(0, F)["first_rescue"] == -1 and f.get_image_rescue(0, F)["n_cand"].tolist() == [1] * F      # still on, with chi2 4.0
    # a map change drops the record; the switch survives it
    f.delete_landmark(7)
    with pytest.raises(srukf.SrukfError) as e: f.get_image_rescue(0, 1)
    assert e.value.rc == -5
    N = 7
    f.stage_sequence(cs["odo"][:3], np.zeros((2, 2 * N)), np.zeros((2, N), dtype=np.int32))
    f.stage_images(cs["frames"][:2])
    f.run_images(0, 2)
    r, rs = f.get_image_rescue(0, 2), f.get_image_ransac(0, 2)
    assert r["flags"].shape == (2, N)
    has = (rs["n_active"] >= 2) & (rs["n_low"] > 0) & (rs["n_low"] < rs["n_active"])
    assert np.array_equal(r["n_cand"], np.where(has, rs["n_active"] - rs["n_low"], 0))
    f.close()


def test_flagged_block_leaves_a_zero_record(srukf, synth):
    """the shipped a1..a4 = 8 with both switches on (threshold 1000 px: the frames' updates are the ones that flag): SRUKF_ERR_CLAMP_PENDING, every row zero"""
    F = 6
    f = _gate_filter(srukf, synth, F, 1000.0, CHI2, which="shipped", scene="clean")
    before = _state_bytes(f) + (_patch_bytes(f),)
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F)
    assert e.value.rc == -7, str(e.value)
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    r = f.get_image_rescue(0, F)
    assert r["first_rescue"] == -1 and not any(r[k].any() for k in RQ_KEYS)
    f.close()


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_fewer_than_two_matches_give_no_candidates(srukf, synth, mode_name):
    from test_gpu_images import _case
    from test_gpu_unique import _rot
    F, mode, ONE = 4, getattr(srukf, "UPDATE_" + mode_name), 3
    cs = _case(srukf, synth, 8)
    f = _filter(srukf, cs, F, appearance=False)
    patch, px = cs["recs"][ONE]
    f.set_landmark_appearance(ONE, patch, _rot(cs["pose"][3]), cs["pose"][:3], px)
    f.images_ransac(True, 0.5); f.images_rescue_gate(True, CHI2)
    f.run_images(0, F, mode=mode)
    assert f.get_image_ransac(0, F)["n_active"].tolist() == [1] * F
    r = f.get_image_rescue(0, F)
    assert r["first_rescue"] == -1 and not any(r[k].any() for k in RQ_KEYS)
    f.close()
