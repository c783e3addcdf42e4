"""The device motion step against the longdouble restatement (np_motion.py), off the figure-8, in every form it exists in (-m gpu).

Inputs: motion_cases.py (odometry pairs, robot blocks of S, whole-frame sequences, the translated scene).  Bounds: the restatement's own rounding bounds,
nothing measured on the device; tests/test_motion_cpu.py shows that the oracle keeps them and that five wrong restatements miss them by 100 x and more.

Step-wise, motion only    predict_motion then get_state (which commits the fast path's results: launch_commit_motion): the robot rows of X, P12 and P22 of
                          P = S^T S and the table of sigma points (sigR: pose, cos / sin of the new heading) within the bound; landmark rows of X and
                          S[:, :n-4] bit-unchanged.  Forms: k_motion ("step_fast" 0), the fast path without announced odometry (k_sigr_rows + k_project_table
                          + the reduction on k_pxy2), the fast path with predict_motion_next (the rows from the tail of k_rank_expand).
Staged replay, motion only  frames staged with `matched` all zero.  What the motion step leaves for k_gain (Xr1, Cmat: R12 and R22) is held to the bound exactly as
                          above; the state after the frame is that through the refactorisation: X within the bound (nothing is added to it), the robot columns of P
                          within the bound + the refactorisation's per-frame allowance (1e-11: it rounds, and clamps pivots below epsilon = 1e-13 to epsilon, the
                          z pivot among them; the oracle does not refactor a frame without matches).  Forms: "fused_motion" 0 / 1 / 2, "tail_fuse" 0 / 1,
                          set_rank_aware(0), graphs and eager, STORAGE_F32, run_frames_batch.
Whole frames              one ordinary frame, then three of standstill / stop-and-go / turn on the spot / 6 cm steps, against the live oracle at the project's
                          per-frame bounds; on the translated scene against the oracle with exact means, at 8 x the running-sum oracle's own distance to it.

Shapes: N = 2 (Na = 21), 21 (135: the first N with the fused tail), 43 (267: second trip of the 256-thread reduction), 86 (525: second pass of the 512-thread
replay body), 256 (1545: past the step-wise body's three prefetched slots; step-wise and the batched replay only).  Every test prints measured / bound per case
(lines "MOTION ..."; docs/LAB_NOTEBOOK.md keeps the first run's)."""
import numpy as np
import pytest

import motion_cases as MC
import np_motion as NM

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
REFACTOR_P = 1e-11                     # the project's per-frame bound on P (README "Parity"): what one refactorisation may move


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


_STATES = {}


def states(srukf, synth, N, storage="f64"):
    """(scene, X0, S0, X1, S1): the joint-initialised start state and the state the DEVICE leaves after one ordinary frame (null rows canonical: a state the fast
    path and "table" mode accept from outside).  Once per (N, storage)."""
    key = (N, storage)
    if key not in _STATES:
        sc = MC.scene(synth, N)
        X0, S0 = sc["X0"].copy(), np.triu(sc["S0"])
        f = srukf.Filter(N, sc["params"])
        if storage == "f32":
            f.set_storage(srukf.STORAGE_F32)
            X0, S0 = _f32(X0), _f32(S0)
        f.set_state(X0, S0)
        f.predict_motion(sc["odo"][0], sc["odo"][1])
        h, Si, vis = f.predict_measurement()
        f.update(sc["z"][0], (sc["matched"][0] * vis).astype(np.int32))
        X1, S1 = f.get_state()
        assert f.debug_get("clamp_rows") == 0 and f.debug_get("exact_frames") == 0 and f.debug_get("gmw_aborts") == 0
        f.close()
        _STATES[key] = (sc, X0, S0, X1, np.triu(S1))
    return _STATES[key]


def case_state(srukf, synth, N, odo_name, blk, storage="f64"):
    sc, X0, S0, X1, S1 = states(srukf, synth, N, storage)
    prev, cur = MC.odometry(synth, odo_name)
    X, S = (X0, S0) if blk == "fresh_S0" else (X1, S1)
    X, S = MC.place(X, prev), MC.block(blk, S)
    if storage == "f32":
        X, S = _f32(X), _f32(S)
    return sc["params"], X, S, prev, cur


def launches(f):
    return {k: v["launches"] for k, v in f.profile().items() if v["launches"]}


def clean(f):
    return f.debug_get("gmw_aborts") == 0 and f.debug_get("clamp_rows") == 0 and f.debug_get("exact_frames") == 0


def table_ratios(ref, sigR):
    """the device's table of sigma points (row c: pose, cos and sin of the new heading) against the restatement's: measured / bound"""
    L = ref["sigma"].shape[0]
    t = sigR.reshape(-1, 8)[:L]
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs((t[:, :4].astype(NM.LD) - ref["sigma"]).astype(np.float64))
        rs = np.where(d == 0, 0.0, d / ref["sigma_bound"]).max()
        dt = np.abs(t[:, 4:6] - ref["trig"])
        rt = np.where(dt == 0, 0.0, dt / ref["trig_bound"][:, None]).max()
    return float(rs), float(rt)


# ---- step-wise, motion only -------------------------------------------------------------------------------------------------------------------------------

def stepwise(srukf, N, p, X, S, prev, cur, form, z_front=None):
    """one motion step through the step-wise API in the named form -> (ratios, landmark part untouched, the reference).  form "tail": a standstill frame with the
    measurements z_front runs first, with (prev, cur) announced, so that its tail prepares the step under test"""
    n = X.shape[0]
    zero_z, zero_m = np.zeros(2 * N), np.zeros(N, dtype=np.int32)
    f = srukf.Filter(N, p)
    f.debug_set("step_fast", 0 if form == "k_motion" else 1)
    f.set_profiling(True)
    f.set_state(X, S)
    Xb, Sb = X, S
    frames = 1
    if form != "k_motion":
        assert f.debug_get("plan_fuse") == 1                     # the canonical null rows were recognised: the fast path is open
    if form == "tail":
        # the state the frame in front leaves is read from a twin that announces nothing (same state bit for bit: test_gpu_parity_r5.py)
        g = srukf.Filter(N, p); g.set_state(X, S)
        for q in (g, f):
            if q is f:
                q.predict_motion_next(prev, cur)
            q.predict_motion(prev, prev)
            h, Si, vis = q.predict_measurement()
            assert vis.all()
            q.update(z_front, vis.astype(np.int32))
        Xb, Sb = g.get_state()
        Sb = np.triu(Sb)
        assert g.debug_get("step_fast") == 1 and clean(g)
        g.close()
        frames = 2
    before = launches(f)
    f.predict_motion(prev, cur)
    Xd, Sd = f.get_state()
    sigR = f.debug_copy("sigR", (2 * (n + 5) + 2) * 8)
    got = launches(f)
    # which form ran
    if form == "k_motion":
        assert got.get("k_motion") == 1 and "k_project_table" not in got and "k_pxy2" not in got, got
    elif form == "table":
        assert got.get("k_project_table") == 1 and got.get("k_pxy2") == 1 and "k_motion" not in got and "k_project_motion" not in got, got
    else:
        assert got.get("k_project_table") == before.get("k_project_table") == 1 and got.get("k_pxy2") == 2 and got.get("k_rank_expand") == 1, (before, got)
        assert "k_motion" not in got and "k_project_motion" not in got, got
    # the frame ends without matches: the counters tell which path took it
    f.predict_measurement()
    f.update(zero_z, zero_m)
    counts = (f.debug_get("step_fast"), f.debug_get("step_slow"))
    assert counts == ((0, 1) if form == "k_motion" else (frames, 0)), counts
    assert clean(f)
    f.close()
    ref = NM.motion_step(Xb, Sb, prev, cur, p)
    P12, P22 = NM.robot_columns_of_P(Sd)
    r = NM.ratios(ref, Xd[n - 4:], P12, P22)
    r["sigma"], r["trig"] = table_ratios(ref, sigR)
    untouched = np.array_equal(Xd[:n - 4], Xb[:n - 4]) and np.array_equal(Sd[:, :n - 4], Sb[:, :n - 4])
    return r, untouched, ref


def hold(tag, results):
    """print every case's ratios, then assert them all"""
    bad = []
    for name, r, ok in results:
        print(f"MOTION {tag} {name}: measured / bound  " + "  ".join(f"{k} {v:.3f}" for k, v in r.items()) + ("" if ok else "   LANDMARK PART CHANGED"))
        if not ok or not all(np.isfinite(v) and v <= 1.0 for v in r.values()):
            bad.append((name, r, ok))
    assert not bad, bad


STEP_GROUPS = ([(2, b, "k_motion") for b in MC.BLOCKS] +
               [(21, b, form) for b in MC.BLOCKS for form in ("k_motion", "table") if not (b == "fresh_S0" and form == "table")] +
               [(N, "after_frame", form) for N in (21, 43, 86, 256) for form in ("tail",)] +
               [(N, "after_frame", form) for N in (43, 86, 256) for form in ("k_motion", "table")])
SUBSET = ("still_0", "wrap", "translated")                      # the larger shapes: the exact-zero control, the 2 pi rot2, the ill-conditioned mean


@pytest.mark.parametrize("N,blk,form", STEP_GROUPS)
def test_stepwise_motion_step_within_the_reference_bound(srukf, synth, N, blk, form):
    names = MC.ODOMETRY if N <= 21 else SUBSET + (("heading_40",) if N == 256 else ())
    results = []
    for name in names:
        p, X, S, prev, cur = case_state(srukf, synth, N, name, blk)
        z_front = None
        if form == "tail":
            if name == "heading_40":
                continue                                          # (a standstill at heading 40 has Mt of 0.6 rad and 1.9 m: no frame to put in front of anything)
            sc, _, _, X1, S = states(srukf, synth, N)
            X, prev, cur, z_front = MC.standstill_in_front(synth, sc, X1, *MC.odometry(synth, name))
        r, untouched, ref = stepwise(srukf, N, p, X, S, prev, cur, form, z_front)
        results.append((name, r, untouched))
    hold(f"step N={N} {blk} {form}", results)


# ---- staged replay, motion only ---------------------------------------------------------------------------------------------------------------------------

STAGED_FORMS = {
    # name: (debug switches, rank-aware, plan_motion from a canonical state, does a frame's tail run the next frame's reduction)
    "default":        ({}, 1, 2, True),
    "fused_motion_0": ({"fused_motion": 0}, 1, 0, False),
    "fused_motion_1": ({"fused_motion": 1}, 1, 1, False),
    "tail_fuse_0":    ({"tail_fuse": 0}, 1, 2, False),
    "rank_aware_0":   ({}, 0, 1, False),
    "eager":          ({"use_graph": 0}, 1, 2, True),
}


def staged_filter(srukf, N, p, X, S, odo, form, storage="f64", profiling=True):
    dbg, rank_aware, _, _ = STAGED_FORMS[form]
    f = srukf.Filter(N, p)
    if not rank_aware:
        f.set_rank_aware(0)
    if storage == "f32":
        f.set_storage(srukf.STORAGE_F32)
    for k, v in dbg.items():
        f.debug_set(k, v)
    if profiling:
        f.set_profiling(True)
    f.set_state(X, S)
    F = len(odo) - 1
    f.stage_sequence(np.asarray(odo), np.zeros((F, 2 * N)), np.zeros((F, N), dtype=np.int32))
    return f


def pending_ratios(f, ref, S11, n):
    """what the motion step of the replay leaves for k_gain: the new robot mean (Xr1) and the new last four columns of S (Cmat: R12 over R22)"""
    Xr1 = f.debug_copy("Xr1", 4)
    Cm = f.debug_copy("Cmat", n * 4).reshape(n, 4)
    R12, R22 = Cm[:n - 4].astype(NM.LD), np.triu(Cm[n - 4:]).astype(NM.LD)
    P12 = (S11.T.astype(NM.LD) @ R12).astype(np.float64)
    P22 = (R12.T @ R12 + R22.T @ R22).astype(np.float64)
    return NM.ratios(ref, Xr1, P12, P22), Xr1


def staged(srukf, N, p, X, S, prev, cur, form, canonical, storage="f64"):
    """one staged frame without matches (and, where the frame tail prepares the next frame's motion step, a second one) -> (ratios, landmark part untouched)"""
    n = X.shape[0]
    dbg, rank_aware, plan_motion, tail = STAGED_FORMS[form]
    rank_form = rank_aware and n >= 128
    ref = NM.motion_step(X, S, prev, cur, p)
    f = staged_filter(srukf, N, p, X, S, [prev, cur], form, storage)
    want = plan_motion if (canonical and rank_form) or plan_motion < 2 else 1
    assert f.debug_get("plan_motion") == want, (f.debug_get("plan_motion"), want)
    assert f.debug_get("plan_fuse") == (1 if want == 2 and dbg.get("tail_fuse", 1) else 0)
    f.run_frames(0, 1)
    Xd, Sd = f.get_state()
    got = launches(f)
    if plan_motion == 0:
        assert got.get("k_motion") == 1 and "k_project_table" not in got and "k_project_motion" not in got, got
    elif want == 1:
        assert got.get("k_project_motion") == 1 and "k_project_table" not in got and "k_motion" not in got, got
    else:
        assert got.get("k_project_table") == 1 and "k_project_motion" not in got and "k_motion" not in got, got
    assert clean(f) and f.clamp_info() == (-1, -1)
    r = {}
    if plan_motion != 0:                                          # (k_motion writes X and S itself)
        r, Xr1 = pending_ratios(f, ref, S[:n - 4, :n - 4], n)
        assert np.array_equal(Xd[n - 4:], _f32(Xr1) if storage == "f32" else Xr1)      # nothing was matched: nothing was added to the mean
    f.close()
    # the state behind the frame: X as it was formed, P through one refactorisation
    P12, P22 = NM.robot_columns_of_P(Sd)
    wide = dict(ref)
    A = np.abs(Sd)
    f32 = 4 * EPS32 * (A.T @ A[:, n - 4:]) if storage == "f32" else np.zeros((n, 4))
    wide["mean_bound"] = ref["mean_bound"] + (EPS32 * np.abs(ref["mean"]) if storage == "f32" else 0.0)
    wide["P12_bound"] = ref["P12_bound"] + REFACTOR_P + f32[:n - 4]
    wide["P22_bound"] = ref["P22_bound"] + REFACTOR_P + f32[n - 4:]
    for k, v in NM.ratios(wide, Xd[n - 4:], P12, P22).items():
        r["after " + k] = v
    untouched = np.array_equal(Xd[:n - 4], X[:n - 4])
    if tail and canonical and rank_form and storage == "f64":
        # two frames in one run: the tail of the first (k_rank_expand) writes the second one's table rows and runs its reduction.  The state between them is the
        # one the single staged frame above left (the same launches on the same values: test_gpu_parity_r3.py holds runs cut in two to whole ones bit for bit)
        nxt = cur + (cur - prev)
        Xa, Sa = Xd, np.triu(Sd)
        f = staged_filter(srukf, N, p, X, S, [prev, cur, nxt], form)
        f.run_frames(0, 2)
        got = launches(f)
        assert got.get("k_project_table") == 1 and got.get("k_pxy2") == 2 and got.get("k_rank_expand") == 2 and "k_project_motion" not in got, got
        assert clean(f) and f.clamp_info() == (-1, -1)
        ref2 = NM.motion_step(Xa, Sa, cur, nxt, p)
        r2, Xr1 = pending_ratios(f, ref2, Sa[:n - 4, :n - 4], n)
        sigR = f.debug_copy("sigR", (2 * (n + 5) + 2) * 8)
        r2["sigma"], r2["trig"] = table_ratios(ref2, sigR)
        Xd2, _ = f.get_state()
        assert np.array_equal(Xd2[n - 4:], Xr1)
        untouched = untouched and np.array_equal(Xd2[:n - 4], Xa[:n - 4])
        f.close()
        for k, v in r2.items():
            r["tail " + k] = v
    return r, untouched


STAGED_GROUPS = ([(2, b, "default") for b in ("after_frame", "z_zero", "xy_dependent")] +
                 [(21, b, "default") for b in MC.BLOCKS] +
                 [(21, b, form) for b in MC.DEGENERATE for form in ("fused_motion_0", "fused_motion_1", "rank_aware_0")] +
                 [(N, "after_frame", form) for N in (21, 43, 86) for form in STAGED_FORMS if not (N == 21 and form == "default")])


@pytest.mark.parametrize("N,blk,form", STAGED_GROUPS)
def test_staged_motion_only_frame_within_the_reference_bound(srukf, synth, N, blk, form):
    names = MC.ODOMETRY if N <= 21 and blk == "after_frame" else SUBSET + (("reverse",) if N <= 21 else ())
    results = []
    for name in names:
        p, X, S, prev, cur = case_state(srukf, synth, N, name, blk)
        r, untouched = staged(srukf, N, p, X, S, prev, cur, form, canonical=blk != "fresh_S0")
        results.append((name, r, untouched))
    hold(f"staged N={N} {blk} {form}", results)


def test_staged_motion_only_frame_with_f32_storage(srukf, synth):
    """the state kept in float: the motion step reads what the float state holds and its results are double (the sharp bound applies to them as they wait for k_gain);
    the state behind the frame is rounded to float when it is stored (bound widened by float ulps of the stored entries, as test_gpu_parity_r5._f32_metrics)"""
    N, results = 43, []
    for name in SUBSET:
        p, X, S, prev, cur = case_state(srukf, synth, N, name, "after_frame", storage="f32")
        r, untouched = staged(srukf, N, p, X, S, prev, cur, "default", canonical=True, storage="f32")
        results.append((name, r, untouched))
    hold(f"staged N={N} after_frame f32", results)


@pytest.mark.parametrize("N", [86, 256])
def test_batched_replay_equals_the_solo_run_on_standstill_and_translated(srukf, synth, N):
    """run_frames_batch with B = 2 (N = 256: the batched launches; N = 86: below their smallest shape, the filters run side by side on streams of their own): two
    motion-only frames of the standstill in one filter and of the translated pose in the other, bit-identical to each filter's solo run"""
    pairs = []
    for name in ("still_0", "translated"):
        p, X, S, prev, cur = case_state(srukf, synth, N, name, "after_frame")
        pairs.append((X, S, [prev, cur, cur + (cur - prev)]))
    fs = [staged_filter(srukf, N, p, X, S, odo, "default", profiling=False) for X, S, odo in pairs]
    tb = srukf.run_frames_batch(fs, 0, 2)
    for b, (X, S, odo) in enumerate(pairs):
        assert clean(fs[b]) and fs[b].debug_get("gate_timeouts") == 0
        assert fs[b].debug_get("gmw_shared") == (0 if 6 * N + 4 > 960 else 1)      # the batched launches need 16 panels (np >= 1024); below, one tenant per filter
        g = staged_filter(srukf, N, p, X, S, odo, "default", profiling=False)
        ts = g.run_frames(0, 2)
        Xs, Ss = g.get_state(); Xb, Sb = fs[b].get_state()
        assert clean(g)
        assert np.array_equal(tb[b], ts) and np.array_equal(Xs, Xb) and np.array_equal(Ss, Sb)
        # ... and the solo run's mean is the restatement's: frame 1 from the state that was set
        ref = NM.motion_step(X, S, odo[0], odo[1], p)
        d = np.abs(ts[0, :4] - ref["mean"])
        print(f"MOTION batch N={N} case {b}: |traj - mean| / bound {np.where(d == 0, 0.0, d / ref['mean_bound']).max():.3f}   gmw_shared {fs[b].debug_get('gmw_shared')}")
        assert (d <= ref["mean_bound"]).all()
        g.close()
    for f in fs:
        f.close()


# ---- whole frames ------------------------------------------------------------------------------------------------------------------------------------------

_ORACLE = {}
WHOLE_F = 4


def oracle_frames(oracle, synth, N, name, translated, exact):
    key = (N, name, translated, exact)
    if key not in _ORACLE:
        sc = MC.scene(synth, N)
        shift = MC.TRANSLATION if translated else (0.0, 0.0)
        odo, z, m = MC.sequence(synth, sc, name, shift)
        o = oracle.Oracle(N, sc["params"])
        o.set_exact_means(exact)
        o.set_state(MC.translate_state(sc["X0"], shift), np.triu(sc["S0"]))
        for t in range(WHOLE_F):
            o.predict_motion(odo[t], odo[t + 1])
            h, Si, vis = o.predict_measurement()
            assert vis.all()
            o.update(z[t], m[t], oracle.Oracle.NEEDNOT_REORDER, 0, oracle.Oracle.BATCHED)
        X, S = o.get_state()
        _ORACLE[key] = (X, S.T @ S, o.clamp_stats()["theta"])
        o.close()
    return _ORACLE[key]


def device_frames(srukf, synth, N, name, translated, how):
    sc = MC.scene(synth, N)
    shift = MC.TRANSLATION if translated else (0.0, 0.0)
    odo, z, m = MC.sequence(synth, sc, name, shift)
    f = srukf.Filter(N, sc["params"])
    f.set_state(MC.translate_state(sc["X0"], shift), np.triu(sc["S0"]))
    if how == "staged":
        f.stage_sequence(odo, z, m)
        f.run_frames(0, WHOLE_F)
        assert f.debug_get("plan_fuse") == 1 and f.debug_get("plan_motion") == 2
    else:
        for t in range(WHOLE_F):
            f.predict_motion(odo[t], odo[t + 1])
            h, Si, vis = f.predict_measurement()
            assert vis.all()
            f.update(z[t], m[t])
        assert (f.debug_get("step_fast"), f.debug_get("step_slow")) == (WHOLE_F - 1, 1)      # (the joint-initialised start state is not a fast-path state)
    assert clean(f)
    X, S = f.get_state()
    f.close()
    return X, S.T @ S


@pytest.mark.parametrize("how", ["step", "staged"])
@pytest.mark.parametrize("N", [21, 43])
def test_whole_frames_off_the_figure8_against_the_oracle(srukf, oracle, synth, N, how):
    worst = []
    for name in MC.SEQUENCES:
        Xo, Po, theta = oracle_frames(oracle, synth, N, name, False, 0)
        assert theta == 0                                         # the reference's theta clamp stays out of these inputs
        X, P = device_frames(srukf, synth, N, name, False, how)
        dx, dp = np.abs(X - Xo).max(), np.abs(P - Po).max()
        print(f"MOTION whole N={N} {how} {name}: |dX| {dx:.2e} ({dx / 1e-9:.3f} of the bound)  |dP| {dp:.2e} ({dp / (1e-11 * WHOLE_F):.3f})")
        worst.append((name, dx <= 1e-9 and dp <= 1e-11 * WHOLE_F, dx, dp))
    assert all(w[1] for w in worst), worst


@pytest.mark.parametrize("how", ["step", "staged"])
@pytest.mark.parametrize("N", [21, 43])
def test_whole_frames_on_the_translated_scene_against_the_exact_mean_oracle(srukf, oracle, synth, N, how):
    """50 m from the origin the weighted means cancel L terms of size |wm0| |x|: the reference's running sums and any other summation order differ by far more than
    1e-9.  Reference: the oracle with its means summed in binary128.  The device may be 8 x as far from it as the reference itself is (two roundings of one sum
    differ by a random factor; not a measured device number), and never needs to be closer than the project's per-frame bounds."""
    worst = []
    for name in MC.SEQUENCES:
        Xe, Pe, theta_e = oracle_frames(oracle, synth, N, name, True, 1)
        Xr, Pr, theta_r = oracle_frames(oracle, synth, N, name, True, 0)
        assert theta_e == 0 and theta_r == 0
        bx, bp = max(8 * np.abs(Xr - Xe).max(), 1e-9), max(8 * np.abs(Pr - Pe).max(), 1e-11 * WHOLE_F)
        X, P = device_frames(srukf, synth, N, name, True, how)
        dx, dp = np.abs(X - Xe).max(), np.abs(P - Pe).max()
        print(f"MOTION translated N={N} {how} {name}: |dX| {dx:.2e} ({dx / bx:.3f} of the bound {bx:.2e}; the reference's own {np.abs(Xr - Xe).max():.2e})  "
              f"|dP| {dp:.2e} ({dp / bp:.3f} of {bp:.2e}; {np.abs(Pr - Pe).max():.2e})")
        worst.append((name, dx <= bx and dp <= bp, dx, dp))
    assert all(w[1] for w in worst), worst
