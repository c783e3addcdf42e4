"""GPU tests of the map policy's verdict (srukf_map_policy, srukf_images_policy / srukf_images_set_policy_state / srukf_get_image_policy / srukf_images_rewind;
csrc/srukf_policy.hip, srukf_images.hip): the step-wise kernel against the numpy restatement (tests/np_policy.py), the staged form against a twin
driven step by step, that the policy is read-only for the filter, the rewind of a clean block, a flagged block, and the switch's lifetime.

Scene: tests/test_gpu_images.py's (N = 8, seed 13, texture seed 17, 640 x 480, at most 11 frames; landmark 5 has no appearance record and never matches, landmark
2's record was cut somewhere else).  Landmark 5 is seeded with nPredictTimes = 7, nMatchTimes = 3: it is visible in every frame, so UNMATCHED (n > 2 m and n >= 10)
first fires behind frame index 2.  Every other landmark is seeded at zero with predictLocation mid-image.  The step-wise twin has 6 matches in each of its frames
(min_matches 5) and no landmark within 70 px of an image edge, so with the default parameters nothing else asks for a change in frames 0 and 1: asserted on the twin.
Integers (verdicts, summaries, counters, first_change) are compared as integers.  Preconditions are asserted on the reference's side alone: every real-valued test
of the restatement is at least 1e-6 from its threshold."""
import functools

import numpy as np
import pytest

import np_policy as P
from test_gpu_images import F_MAX, _case, _filter, _patch_bytes, _record_bytes, _state_bytes

pytestmark = pytest.mark.gpu

W, H = 640.0, 480.0
LM, SEED_COUNTS = 5, (7, 3)
PAR = dict()                                                     # the defaults: border 20, rho_min 0.01, min_predictions 10, min_matches 5
NEUTRAL = dict(corr_threshold=0.8, ratio=2.0, exclusion=4, subpixel=False)      # a checked run that decides as the plain one


def _seed(N=8):
    st = P.zero_state(N)
    st["predictLocation"] = (320.0, 240.0)
    st["nPredictTimes"][LM], st["nMatchTimes"][LM] = SEED_COUNTS
    return st


def _summary_dict(rec, t):
    return {k: int(rec["summary"][k][t]) for k in P.SUMMARY_FIELDS}


def _restate(st, X, h, vis, z, m, **kw):
    """the restatement, with its precondition: no real-valued test within 1e-6 of its threshold"""
    mg = []
    out = P.policy(st, X, h, vis, z, m, W, H, margins=mg, **kw)
    assert min(mg) >= 1e-6, min(mg)
    return out


def _same_state(a, b):
    return a["nPredictTimes"].tolist() == b["nPredictTimes"].tolist() and a["nMatchTimes"].tolist() == b["nMatchTimes"].tolist() and \
        a["predictLocation"].tobytes() == b["predictLocation"].tobytes()


# ---- 1. the step-wise kernel against the restatement ----
@functools.lru_cache(maxsize=None)
def _clean_frame(srukf, synth, N):
    """posterior and association of one clean frame.  N = 8: the image scene's first frame; other N: the synthetic scene's first frame with its own measurements"""
    if N == 8:
        cs = _case(srukf, synth, 8)
        f = _filter(srukf, cs)
        f.predict_motion(cs["odo"][0], cs["odo"][1])
        h, _, vis = f.predict_measurement()
        z, m, _ = f.associate(cs["frames"][0])
        f.update(z, m)
        p = cs["p"]
    else:
        p = synth.scene_params()
        sc = synth.make_scene(N, 3, seed=13, p=p)
        f = srukf.Filter(N, p)
        f.set_state(sc["X0"], sc["S0"])
        f.predict_motion(sc["odo"][0], sc["odo"][1])
        h, _, vis = f.predict_measurement()
        z, m = np.array(sc["z"][0], dtype=np.float64), np.array(sc["matched"][0], dtype=np.int32)
        f.update(z, m)
    X, S = f.get_state()
    f.close()
    assert np.isfinite(X).all() and vis.sum() >= 3 and m.sum() >= 3
    return dict(p=p, X=X, S=S, h=np.array(h), vis=np.array(vis), z=np.array(z), m=np.array(m))


def _check_stepwise(srukf, fr, X, st, h, vis, z, m, **kw):
    """map_policy on a filter holding (X, S) against the restatement: verdicts, summary and state equal"""
    N = len(st)
    want_v, want_s, want_st = _restate(st, X, h, vis, z, m, **kw)
    f = srukf.Filter(N, fr["p"])
    f.set_state(X, fr["S"])
    v, s, st2 = f.map_policy(st, h, vis, z, m, **kw)
    Xa, Sa = f.get_state()
    f.close()
    assert Xa.tobytes() == np.asarray(X).tobytes() and Sa.tobytes() == fr["S"].tobytes()          # read-only
    assert v.tolist() == want_v.tolist(), (v, want_v)
    assert s == want_s, (s, want_s)
    assert _same_state(st2, want_st)
    return want_v, want_s, want_st


@pytest.mark.parametrize("N", [8, 300])
def test_stepwise_kernel_against_the_restatement(srukf, synth, N):
    """the posterior of a clean frame; N = 300 needs more than one stride of the 256 threads.  Random counters and last pixels, the defaults and a second set of
    parameters"""
    fr = _clean_frame(srukf, synth, N)
    rng = np.random.default_rng(5)
    st = P.zero_state(N)
    st["nPredictTimes"] = rng.integers(0, 13, N)
    st["nMatchTimes"] = rng.integers(0, 7, N)
    st["predictLocation"] = np.column_stack([rng.uniform(0.0, W, N), rng.uniform(0.0, H, N)])
    # the association is the caller's: every third landmark out of view (its random last pixel then stands), every fifth match somewhere else in the image
    vis, m, z = fr["vis"].copy(), fr["m"].copy(), fr["z"].copy()
    vis[::3] = 0; m[::3] = 0
    moved = np.flatnonzero(m != 0)[::5]
    z.reshape(N, 2)[moved] = np.column_stack([rng.uniform(0.0, W, len(moved)), rng.uniform(0.0, H, len(moved))])
    tot = 0
    for kw in (dict(), dict(border=70.0, rho_min=0.05, min_predictions=6, min_matches=N)):
        v, s, _ = _check_stepwise(srukf, fr, fr["X"], st, fr["h"], vis, z, m, **kw)
        print("N=%d %s: summary %s, bits seen %#x" % (N, kw, s, int(np.bitwise_or.reduce(v))))
        assert s["n_predicts"] == int((vis != 0).sum()) and s["n_matches"] == int((m != 0).sum())
        tot |= int(np.bitwise_or.reduce(v))
    if N == 300:                                                 # landmarks of the second stride decide too, and the inputs reach the counting bits
        assert np.flatnonzero(v)[-1] >= 256 and tot & P.UNMATCHED and tot & P.PRED_BORDER and tot & P.MATCH_BORDER and tot & P.STORE


def test_stepwise_kernel_each_bit_alone(srukf, synth):
    """N = 8, crafted states and inputs that raise each bit alone on one landmark (the restatement says so; the kernel must agree)"""
    fr = _clean_frame(srukf, synth, 8)
    X, h, vis, z, m = fr["X"], fr["h"], fr["vis"], fr["z"], fr["m"]
    st = P.zero_state(8)
    st["predictLocation"] = (320.0, 240.0)
    base = _check_stepwise(srukf, fr, X, st, h, vis, z, m)[0]
    k = int(np.flatnonzero((m != 0) & (base == 0))[0])           # a matched landmark the policy leaves alone
    u = LM                                                       # visible, never matched
    assert vis[u] and not m[u] and base[u] == 0
    # BEHIND: theta + pi
    Xb = X.copy(); Xb[6 * k + 3] += np.pi
    v = _check_stepwise(srukf, fr, Xb, st, h, vis, z, m)[0]
    assert v[k] == P.BEHIND and (np.delete(v, k) == np.delete(base, k)).all()
    # RHO: rho_min above this landmark's rho (the other landmarks are held to the restatement, whatever it says of them), then this landmark's rho below the default
    rho = X[5:6 * 8:6]
    v = _check_stepwise(srukf, fr, X, st, h, vis, z, m, rho_min=float(rho[k]) + 1e-3)[0]
    assert v[k] & P.RHO and not v[k] & (P.UNMATCHED | P.BEHIND)
    Xr = X.copy(); Xr[6 * k + 5] = 0.005
    v = _check_stepwise(srukf, fr, Xr, st, h, vis, z, m)[0]
    assert v[k] == P.RHO
    # UNMATCHED: 9 predictions, 4 matches, visible and unmatched now
    st2 = st.copy(); st2["nPredictTimes"][u], st2["nMatchTimes"][u] = 9, 4
    v, _, stn = _check_stepwise(srukf, fr, X, st2, h, vis, z, m)
    assert v[u] == P.UNMATCHED and stn["nPredictTimes"][u] == 10
    # the pixel bits at border = 70: as the scene has them ...
    v = _check_stepwise(srukf, fr, X, st, h, vis, z, m, border=70.0)[0]
    print("border = 70: verdicts", v.tolist())
    # ... and alone: a predicted pixel 30 px from the left edge on the unmatched landmark, a matched pixel 30 px from the bottom on the matched one
    h2 = h.copy(); h2[2 * u:2 * u + 2] = (30.0, 240.0)
    v = _check_stepwise(srukf, fr, X, st, h2, vis, z, m, border=70.0)[0]
    assert v[u] == P.PRED_BORDER
    hm, zm = h.copy(), z.copy()
    hm[2 * k:2 * k + 2] = (320.0, 240.0); zm[2 * k:2 * k + 2] = (321.0, 450.0)
    v = _check_stepwise(srukf, fr, X, st, hm, vis, zm, m, border=70.0)[0]
    assert v[k] == P.MATCH_BORDER | P.STORE
    # STORE's other branch: predicted at the border, with a match
    hm[2 * k:2 * k + 2] = (30.0, 240.0); zm[2 * k:2 * k + 2] = (320.0, 240.0)
    v = _check_stepwise(srukf, fr, X, st, hm, vis, zm, m, border=70.0)[0]
    assert v[k] == P.PRED_BORDER | P.STORE
    # an invisible landmark keeps its last pixel
    vi = vis.copy(); vi[u] = 0
    st3 = st.copy(); st3["predictLocation"][u] = (5.0, 5.0)
    v, _, stn = _check_stepwise(srukf, fr, X, st3, h, vi, z, m)
    assert v[u] == P.PRED_BORDER and stn["predictLocation"][u].tolist() == [5.0, 5.0] and stn["nPredictTimes"][u] == 0


def test_stepwise_refusals(srukf, synth):
    fr = _clean_frame(srukf, synth, 8)
    f = srukf.Filter(8, fr["p"]); f.set_state(fr["X"], fr["S"])
    for kw in (dict(border=-1.0), dict(border=float("nan")), dict(rho_min=float("inf")), dict(min_predictions=-1), dict(min_matches=-2)):
        with pytest.raises(srukf.SrukfError) as e: f.map_policy(_seed(), fr["h"], fr["vis"], fr["z"], fr["m"], **kw)
        assert e.value.rc == -1, kw
        with pytest.raises(srukf.SrukfError) as e: f.images_policy(True, **kw)
        assert e.value.rc == -1, kw
    f.images_policy(False, border=-1.0)                          # (switching off judges no parameters)
    f.close()


# ---- 2. the staged form against the step-wise twin ----
@functools.lru_cache(maxsize=None)
def _twin(srukf, synth, mode, checked=False, F=6):
    """predict_motion -> predict_measurement -> associate -> update -> map_policy per frame on a twin; the restatement runs beside it on the twin's own numbers"""
    cs = _case(srukf, synth, 8)
    g = _filter(srukf, cs)
    st, st_np = _seed(), _seed()
    out = dict(verdict=[], summary=[], pose=[])
    for t in range(F):
        g.predict_motion(cs["odo"][t], cs["odo"][t + 1])
        h, _, vis = g.predict_measurement()
        if checked:
            r = g.associate_checked(cs["frames"][t], **NEUTRAL); z, m = r["z"], r["matched"]
        else:
            z, m, _ = g.associate(cs["frames"][t])
        if mode == srukf.UPDATE_JOINT: g.update_joint(z, m)
        else: g.update(z, m, mode=srukf.UPDATE_BATCHED)
        v, s, st = g.map_policy(st, h, vis, z, m, **PAR)
        X = g.get_state()[0]
        v_np, s_np, st_np = _restate(st_np, X, h, vis, z, m, **PAR)
        assert v.tolist() == v_np.tolist() and s == s_np and _same_state(st, st_np)
        out["verdict"].append(v); out["summary"].append(s)
    g.close()
    out["verdict"], out["state"] = np.array(out["verdict"]), st
    ch = [s["change"] for s in out["summary"]]
    print("twin: change per frame %s, matches %s, verdicts of frame 2 %s" % (ch, [s["n_matches"] for s in out["summary"]], out["verdict"][2].tolist()))
    # what the seed was chosen for
    assert ch[:3] == [0, 0, 1] and out["verdict"][2][LM] == P.UNMATCHED and not out["verdict"][:2].any()
    return out


def _policy_filter(srukf, synth, F, graph=None, which="scene", seed=True, **kw):
    cs = _case(srukf, synth, 8, which)
    f = _filter(srukf, cs, F, graph=graph)
    f.images_policy(True, **dict(PAR, **kw))
    if seed: f.set_policy_state(_seed())
    return f


def _run(f, first, count, mode, checked=False):
    return f.run_images_checked(first, count, mode=mode, **NEUTRAL) if checked else f.run_images(first, count, mode=mode)


@pytest.mark.parametrize("mode_name,checked", [("BATCHED", False), ("JOINT", False), ("BATCHED", True)])
def test_staged_against_the_stepwise_twin(srukf, synth, mode_name, checked):
    """run_images(0, 6) with the switch on against the twin: every verdict, every summary, first_change == 2 and the final state"""
    F, mode = 6, getattr(srukf, "UPDATE_" + mode_name)
    tw = _twin(srukf, synth, mode, checked)
    f = _policy_filter(srukf, synth, F)
    _run(f, 0, F, mode, checked)
    rec = f.get_image_policy(0, F)
    assert f.clamp_info() == (-1, -1)
    f.close()
    assert rec["verdict"].tolist() == tw["verdict"].tolist()
    for t in range(F):
        assert _summary_dict(rec, t) == tw["summary"][t], t
    assert rec["first_change"] == 2
    d = np.abs(rec["state"]["predictLocation"] - tw["state"]["predictLocation"]).max()
    print("%s%s: |predictLocation - twin's| max %.3e" % (mode_name, " checked" if checked else "", d))
    assert _same_state(rec["state"], tw["state"])


def test_staged_behind_a_searching_run(srukf, synth):
    """the archive search (tests/test_gpu_images_archive.py's archive of L = 5) and the policy behind the same frames: the searching frames' own captured graphs
    with the policy launch behind them.  The policy record is the twin's, the search record the searching twin's, bit for bit"""
    import test_gpu_images_archive as gia
    F, mode = 6, srukf.UPDATE_BATCHED
    tw, ar = _twin(srukf, synth, mode), gia._twin(srukf, synth, mode, gia.ALL, F)
    f = gia._searching(srukf, synth, F)
    f.images_policy(True, **PAR)
    f.set_policy_state(_seed())
    traj = f.run_images(0, F, mode=mode)
    rec, arc = f.get_image_policy(0, F), f.get_image_archive(0, F)
    assert f.clamp_info() == (-1, -1)
    state = _state_bytes(f)
    f.close()
    assert rec["verdict"].tolist() == tw["verdict"].tolist() and rec["first_change"] == 2 and _same_state(rec["state"], tw["state"])
    for t in range(F):
        assert _summary_dict(rec, t) == tw["summary"][t], t
    for k in gia.KEYS:
        assert arc[k].reshape(-1).tobytes() == ar[k].reshape(-1).tobytes(), k
    assert arc["hits"].tolist() == [3] * F
    assert traj.tobytes() == ar["traj"].tobytes() and state == ar["state"]


# ---- 3. read-only ----
@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_policy_is_read_only_and_one_computation(srukf, synth, mode_name):
    """11 frames: trajectory, X, S, the match record and the matchPatches with the switch on are those of the run with it off; eager launches, graphs and a 5 + 6
    split leave the same bits, and the same policy record"""
    F, mode = F_MAX, getattr(srukf, "UPDATE_" + mode_name)
    cs = _case(srukf, synth, 8)
    g = _filter(srukf, cs, F)
    t = g.run_images(0, F, mode=mode)
    off = (t.tobytes(),) + _state_bytes(g) + _record_bytes(g.get_image_matches(0, F)) + (_patch_bytes(g),)
    assert g.clamp_info() == (-1, -1)
    g.close()
    recs = []
    for name in ("default", "eager", "split"):
        f = _policy_filter(srukf, synth, F, graph=0 if name == "eager" else None)
        t = np.vstack([f.run_images(0, 5, mode=mode), f.run_images(5, 6, mode=mode)]) if name == "split" else f.run_images(0, F, mode=mode)
        assert f.clamp_info() == (-1, -1)
        on = (t.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + (_patch_bytes(f),)
        assert on == off, name
        r = f.get_image_policy(0, F)
        recs.append((r["verdict"].tobytes(), r["summary"].tobytes(), r["state"].tobytes(), r["first_change"]))
        f.close()
    assert recs[0] == recs[1] and recs[0] == recs[2]
    assert recs[0][3] == 2 and np.frombuffer(recs[0][0], dtype=np.int32).any()


# ---- 4. rewind ----
def test_rewind_equals_a_fresh_run(srukf, synth):
    """run_images(0, 6), synchronize, images_rewind, run_images(0, 3): X, S, matchPatches and policy state of a fresh filter's run_images(0, 3)"""
    f = _policy_filter(srukf, synth, 6)
    f.run_images(0, 6)
    assert f.get_image_policy(0, 6)["first_change"] == 2
    after6 = _state_bytes(f)
    f.images_rewind()
    r0 = f.get_image_policy(0, 6)                                # the rewound frames' rows are no verdicts any more; the state is the seed again
    assert r0["first_change"] == -1 and not r0["verdict"].any() and not r0["summary"]["n_predicts"].any() and _same_state(r0["state"], _seed())
    t = f.run_images(0, 3)
    got = (t.tobytes(),) + _state_bytes(f) + (_patch_bytes(f),)
    r = f.get_image_policy(0, 3)
    f.close()
    g = _policy_filter(srukf, synth, 6)
    t = g.run_images(0, 3)
    want = (t.tobytes(),) + _state_bytes(g) + (_patch_bytes(g),)
    r2 = g.get_image_policy(0, 3)
    g.close()
    assert got == want and got[1:3] != after6
    assert _same_state(r["state"], r2["state"]) and r["verdict"].tobytes() == r2["verdict"].tobytes() and r["summary"].tobytes() == r2["summary"].tobytes()
    assert r["first_change"] == 2 and r["state"]["nPredictTimes"][LM] == SEED_COUNTS[0] + 3


def test_rewind_refusals(srukf, synth):
    """SRUKF_ERR_SEQUENCE: nothing synchronised, a run pending, and after predict_motion, set_state and run_frames; the state is left alone"""
    cs = _case(srukf, synth, 8)
    f = _policy_filter(srukf, synth, 6)

    def refused():
        before = _state_bytes(f)
        with pytest.raises(srukf.SrukfError) as e: f.images_rewind()
        assert e.value.rc == -5, str(e.value)
        assert _state_bytes(f) == before

    refused()                                                    # no image block has been synchronised
    f.run_images_async(0, 3)
    with pytest.raises(srukf.SrukfError) as e: f.images_rewind()  # a run is pending
    assert e.value.rc == -5
    f.synchronize()
    f.predict_motion(cs["odo"][3], cs["odo"][4])
    refused()
    f.predict_measurement(); z, m, _ = f.associate(cs["frames"][3]); f.update(z, m)
    refused()
    f.run_images(0, 3)
    X, S = f.get_state()                                         # (a getter alone does not spoil the block ...)
    f.set_state(X, S)                                            # (... a state from outside does)
    refused()
    f.run_images(0, 2)
    f.run_frames(2, 1)
    refused()
    f.run_images(0, 2)
    f.set_policy_state(_seed())                                  # a seed is not in the block's checkpoint
    refused()
    assert _same_state(f.get_image_policy(0, 1)["state"], _seed())
    f.run_images(0, 2)
    f.images_rewind()
    refused()                                                    # one rewind per block
    f.close()


# ---- 5. a flagged block ----
def test_flagged_block_restores_the_policy_state(srukf, synth):
    """the shipped a1..a4 = 8 (tests/test_gpu_images.py): run_images returns SRUKF_ERR_CLAMP_PENDING and the policy state is the seed again, as X and S are their
    values before the call"""
    F = 6
    f = _policy_filter(srukf, synth, F, which="shipped")
    before = _state_bytes(f) + (_patch_bytes(f),)
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F)
    assert e.value.rc == -7, str(e.value)
    frame, _ = f.clamp_info()
    assert 0 <= frame < F
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    r = f.get_image_policy(0, F)
    assert _same_state(r["state"], _seed())
    assert r["first_change"] == -1 and not r["verdict"].any() and not r["summary"]["change"].any()      # what the restored frames wrote does not stand
    with pytest.raises(srukf.SrukfError) as e: f.images_rewind()  # the restore has run already: not a clean block
    assert e.value.rc == -5
    f.close()


# ---- 6. lifetime ----
def test_parameters_switch_and_lifetime(srukf, synth):
    """a parameter change between runs reaches the launches (no captured frame holds a value): first_change moves; the switch off restores the old path; reset and a
    map change drop state and record"""
    cs = _case(srukf, synth, 8)
    F = 6
    f = _policy_filter(srukf, synth, F)
    with pytest.raises(srukf.SrukfError) as e: f.get_image_policy(0, F)                      # no policy run yet
    assert e.value.rc == -5
    f.run_images(0, 3)
    assert f.get_image_policy(0, 3)["first_change"] == 2
    with pytest.raises(srukf.SrukfError) as e: f.get_image_policy(0, F + 1)
    assert e.value.rc == -2
    f.images_rewind()
    f.images_policy(True, **dict(PAR, min_predictions=9))        # 9 > 6 and 9 >= 9: one frame earlier
    f.run_images(0, 3)
    r = f.get_image_policy(0, 3)
    assert r["first_change"] == 1 and r["verdict"][1][LM] == P.UNMATCHED
    f.run_images_async(3, 1)
    with pytest.raises(srukf.SrukfError) as e: f.images_policy(False)                        # not while an image run is in flight
    assert e.value.rc == -5
    with pytest.raises(srukf.SrukfError) as e: f.set_policy_state(_seed())
    assert e.value.rc == -5
    f.synchronize()
    # the switch off: the record and the state stay as they are, the run is the plain one
    f.images_policy(False)
    before = f.get_image_policy(0, F)
    t_off = f.run_images(4, 2)
    after = f.get_image_policy(0, F)
    assert before["verdict"].tobytes() == after["verdict"].tobytes() and before["state"].tobytes() == after["state"].tobytes()
    g = _filter(srukf, cs, F)
    t_ref = np.vstack([g.run_images(0, 3), g.run_images(3, 1), g.run_images(4, 2)])
    assert t_off.tobytes() == t_ref[4:].tobytes() and _state_bytes(f) == _state_bytes(g)
    g.close()
    # reset clears the switch and drops the images
    f.images_policy(True, **PAR)
    f.reset()
    with pytest.raises(srukf.SrukfError) as e: f.get_image_policy(0, 1)
    assert e.value.rc == -5
    f.close()
    # a map change drops state and record; the switch survives it
    f = _policy_filter(srukf, synth, F)
    f.run_images(0, 2)
    f.delete_landmark(0)
    for call in (lambda: f.get_image_policy(0, 1), lambda: f.set_policy_state(_seed(7)), lambda: f.images_rewind()):
        with pytest.raises(srukf.SrukfError) as e: call()
        assert e.value.rc == -5
    N = 7
    f.stage_sequence(cs["odo"][:3], np.zeros((2, 2 * N)), np.zeros((2, N), dtype=np.int32))
    f.stage_images(cs["frames"][:2])
    f.run_images(0, 2)
    r = f.get_image_policy(0, 2)                                 # the switch is still on; the state started at zero
    assert r["verdict"].shape == (2, N) and r["state"]["nPredictTimes"].max() == 2
    f.close()
