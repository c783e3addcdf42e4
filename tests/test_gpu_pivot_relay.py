"""Pivot relay of the persistent factorisation (srukf_gmw_persist.hip, gmw_pivot_relay): two pivot workgroups take the panels alternately.

The relay applies the same products in the same order as the single pivot workgroup, so a staged replay with "pivot_relay" 1 must give, bit for bit, the trajectory,
X and S of the same replay with "pivot_relay" 0.  The sizes are the smallest at which the exclusive replay selects the register-tile persistent launch with
  Tp = 2  one hand-off, the second pivot factors the last panel        Tp = 3  the first pivot returns and its LDS is reused        Tp = 4  an even number of panels,
each with a last panel that stops after its first 32 pivots (half_only) and with one that does not; the full-rank form (Tp = T); fp32 storage once.
The kept rank r comes from null_directions(), the expected panel count and the half_only condition from r (gmw_pivot_persist: klim = r rounded up to 16).

Both persistent pivots and the per-panel pivot (srukf_factor.hip, gmw_step64_block00) are built from the panel phases of srukf_gmw_pivot.h, so every case replays a third
time with "gmw_persist" 0 (one launch per 64-row panel) and must again give the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 3


def _relay_default(srukf):
    return int(srukf.load_library().srukf_gmw_get_pivot_relay())


def _replay(srukf, synth, N, relay, rank_aware, storage, persist=1):
    was = _relay_default(srukf)
    srukf.debug_set_global("pivot_relay", relay)                # read when a plan is built: before the filter exists
    srukf.debug_set_global("gmw_persist", persist)
    try:
        p = synth.scene_params()
        sc = synth.make_scene(N, F, seed=5, p=p)
        rng = np.random.default_rng(77 + N)
        matched = np.ones((F, N), dtype=np.int32)
        for t in range(F):
            matched[t, rng.permutation(N)[:N // 4]] = 0
        X0, S0 = sc["X0"], np.triu(sc["S0"])
        f = srukf.Filter(N, p)
        if not rank_aware:
            f.set_rank_aware(0)
        if storage == "f32":
            f.set_storage(srukf.STORAGE_F32)
            X0, S0 = X0.astype(np.float32).astype(np.float64), S0.astype(np.float32).astype(np.float64)
        f.set_state(X0, S0); f.stage_sequence(sc["odo"], sc["z"], matched)
        traj = f.run_frames(0, F)
        X, S = f.get_state()
        info = dict(aborts=f.debug_get("gmw_aborts"), clamp=f.debug_get("clamp_rows"), relay=f.debug_get("plan_relay"), reg=f.debug_get("plan_register_form"),
                    persist=f.debug_get("plan_persist"), T=f.debug_get("plan_T"), Tp=f.debug_get("plan_Tp"), null=f.null_directions(), n=6 * N + 4)
        f.close()
    finally:
        srukf.debug_set_global("gmw_persist", 1)
        srukf.debug_set_global("pivot_relay", was)
    return traj, X, S, info


# (N, rank-aware, storage, Tp, last panel half_only)
CASES = [
    (25, 1, "f64", 2, True), (35, 1, "f64", 2, False),
    (45, 1, "f64", 3, True), (55, 1, "f64", 3, False),
    (70, 1, "f64", 4, True), (75, 1, "f64", 4, False),
    (30, 0, "f64", 3, False),                                  # every pivot factored: Tp = T
    (45, 1, "f32", 3, True),
]


@pytest.mark.parametrize("N,rank_aware,storage,Tp,half_only", CASES)
def test_relay_replay_is_bit_identical_to_the_single_pivot(srukf, synth, N, rank_aware, storage, Tp, half_only):
    t1, X1, S1, i1 = _replay(srukf, synth, N, 1, rank_aware, storage)
    t0, X0, S0, i0 = _replay(srukf, synth, N, 0, rank_aware, storage)
    tp, Xp, Sp, ip = _replay(srukf, synth, N, 1, rank_aware, storage, persist=0)     # one launch per panel: gmw_step64_block00
    print(N, i1, i0, ip)
    for i in (i1, i0):
        assert i["aborts"] == 0 and i["clamp"] == 0 and i["reg"] == 1 and i["persist"] == 1, i
    assert ip["persist"] == 0 and ip["aborts"] == 0 and ip["clamp"] == 0, ip
    assert i1["relay"] == 1 and i0["relay"] == 0
    # the case is the one its name says: panels pivoted, and whether the kept pivots end in the first half of the last one
    r = i1["n"] - i1["null"]
    assert i1["Tp"] == Tp == (r + 63) // 64 if rank_aware else i1["Tp"] == Tp == i1["T"]
    assert (i1["null"] > 0) == bool(rank_aware)
    if rank_aware:
        assert i1["Tp"] < i1["T"] and (((r + 15) & ~15) <= 64 * (Tp - 1) + 32) == half_only
    assert np.array_equal(t1, t0)
    assert np.array_equal(X1, X0)
    assert np.array_equal(S1, S0)
    assert np.array_equal(tp, t1)
    assert np.array_equal(Xp, X1)
    assert np.array_equal(Sp, S1)


def test_relay_step_api_is_bit_identical_to_the_single_pivot(srukf, synth):
    """The step-wise API (predict_motion / predict_measurement / update) at N = 55 (Tp = 3): same state bit for bit with and without the relay."""
    N = 55
    out = []
    was = _relay_default(srukf)
    for relay in (1, 0):
        srukf.debug_set_global("pivot_relay", relay)
        try:
            p = synth.scene_params()
            sc = synth.make_scene(N, F, seed=5, p=p)
            f = srukf.Filter(N, p)
            f.set_state(sc["X0"], np.triu(sc["S0"]))
            for t in range(F):
                f.predict_motion(sc["odo"][t], sc["odo"][t + 1])
                f.predict_measurement()
                f.update(sc["z"][t], sc["matched"][t], mode=srukf.UPDATE_BATCHED)
            X, S = f.get_state()
            assert f.debug_get("gmw_aborts") == 0 and f.debug_get("clamp_rows") == 0
            assert f.debug_get("plan_relay") == relay
            f.close()
            out.append((X, S))
        finally:
            srukf.debug_set_global("pivot_relay", was)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
