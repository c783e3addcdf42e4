"""The longdouble restatement of the motion step (np_motion.py) against the CPU oracle, off the figure-8 (no GPU).

Every odometry case x robot block of motion_cases.py at N = 2 and 8, and the translated and wrap cases at N = 86: the oracle's robot mean and the robot
columns of its P = S^T S lie within the restatement's rounding bound, its landmark rows of X do not change and its leading block of P changes by the rounding
of (X + gamma S) - X only.  Then the bound's teeth: five wrong restatements each miss it by a factor of 100 and more on at least one case."""
import numpy as np
import pytest

import motion_cases as MC
import np_motion as NM


def _frame(o, O, sc, odo, z, matched, t):
    o.predict_motion(odo[t], odo[t + 1])
    h, Si, vis = o.predict_measurement()
    o.update(z[t], (matched[t] * vis).astype(np.int32), O.Oracle.NEEDNOT_REORDER, 0, O.Oracle.BATCHED)


_STATES = {}


def states(synth, oracle, N):
    """the scene, its joint-initialised start state and the oracle's state after one ordinary frame (computed once per N)"""
    if N not in _STATES:
        sc = MC.scene(synth, N)
        o = oracle.Oracle(N, sc["params"])
        o.set_state(sc["X0"], np.triu(sc["S0"]))
        _frame(o, oracle, sc, sc["odo"], sc["z"], sc["matched"], 0)
        X1, S1 = o.get_state()
        o.close()
        _STATES[N] = (sc, sc["X0"].copy(), np.triu(sc["S0"]), X1, np.triu(S1))
    return _STATES[N]


def case_state(synth, oracle, N, odo_name, blk):
    sc, X0, S0, X1, S1 = states(synth, oracle, N)
    prev, cur = MC.odometry(synth, odo_name)
    X, S = (X0, S0) if blk == "fresh_S0" else (X1, S1)
    return sc["params"], MC.place(X, prev), MC.block(blk, S), prev, cur


def oracle_step(oracle, N, p, X, S, prev, cur):
    """-> X, S and the robot part of the sigma points ((L, 4), in the restatement's order) behind the oracle's motion step"""
    o = oracle.Oracle(N, p)
    o.set_state(X, S)
    o.predict_motion(prev, cur)
    Xo, So = o.get_state()
    n = Xo.shape[0]
    sig = o.sigma()[n - 4:n].T.copy()
    o.close()
    return Xo, So, sig


def hold_oracle(oracle, N, p, X, S, prev, cur, ref):
    n = X.shape[0]
    Xo, So, sig = oracle_step(oracle, N, p, X, S, prev, cur)
    assert np.isfinite(Xo).all() and np.isfinite(So).all()
    assert np.array_equal(Xo[:n - 4], X[:n - 4])
    P12, P22 = NM.robot_columns_of_P(So)
    r = NM.ratios(ref, Xo[n - 4:], P12, P22, sig)
    S11 = S[:n - 4, :n - 4]
    d11 = np.abs(So[:, :n - 4].T @ So[:, :n - 4] - S11.T @ S11)
    with np.errstate(divide="ignore", invalid="ignore"):
        r["P11"] = float(np.where(d11 == 0, 0.0, d11 / (ref["P11_bound"] + NM.U * n * (np.abs(S11).T @ np.abs(S11)))).max())
    return r


CASES = [(N, o, b) for N in (2, 8) for o in MC.ODOMETRY for b in MC.BLOCKS] + [(86, "translated", "after_frame"), (86, "wrap", "after_frame")]


@pytest.mark.parametrize("N,odo_name,blk", CASES)
def test_restatement_and_oracle_agree_within_the_bound(synth, oracle, N, odo_name, blk):
    p, X, S, prev, cur = case_state(synth, oracle, N, odo_name, blk)
    ref = NM.motion_step(X, S, prev, cur, p)
    r = hold_oracle(oracle, N, p, X, S, prev, cur, ref)
    print(f"MOTION-CPU N={N} {odo_name} {blk}: oracle / bound  sigma {r['sigma']:.3f}  X {r['X']:.3f}  P12 {r['P12']:.3f}  P22 {r['P22']:.3f}  P11 {r['P11']:.3f}   "
          f"max bound X {ref['mean_bound'].max():.2e} P12 {ref['P12_bound'].max():.2e} P22 {ref['P22_bound'].max():.2e}")
    assert max(r.values()) <= 1.0, r


def test_the_quirks_of_the_control_are_the_cases_the_table_promises(synth):
    p = synth.scene_params()
    Ut, Mt = NM.control(*MC.odometry(synth, "still_0"), p)
    assert not Ut.any() and not Mt.any()
    Ut, Mt = NM.control(*MC.odometry(synth, "still_1p2"), p)
    assert Ut[0] == -1.2 and Ut[1] == 0.0 and Ut[2] == 1.2 and Mt.all()
    Ut, Mt = NM.control(*MC.odometry(synth, "reverse"), p)
    assert abs(abs(Ut[0]) - np.pi) < 1e-12 and abs(Mt[0] - (p["a1"] * np.pi ** 2 + p["a2"] * 1e-4)) < 1e-12
    Ut, Mt = NM.control(*MC.odometry(synth, "wrap"), p)
    assert abs(Ut[2] + 2 * np.pi) < 0.02 and Mt[2] > p["a1"] * 39
    Ut, Mt = NM.control(*MC.odometry(synth, "heading_40"), p)
    assert abs(Ut[0]) > 37 and abs(Ut[2]) > 37


def test_the_weights_are_the_oracles(oracle):
    for wt in (0, 1, 2):
        for Na in (21, 135, 525):
            w = oracle.sample_parameter(Na, wt, 1e-3, 2.0)
            got = NM.weights(Na, dict(weight_type=wt, ut_alpha=1e-3, ut_beta=2.0))
            assert got == (w["wm0"], w["wc0"], w["wi"], w["wi_sr"], w["gamma"]), (wt, Na)


# ---- the bound has teeth ---------------------------------------------------------------------------------------------------------------------------------

def _teeth_cases(synth, oracle):
    """every case x block at N = 2, and the figure-8 frame under weight type 1 (scaled weights: the only type with wc0 != wm0)"""
    for o in MC.ODOMETRY:
        for b in MC.BLOCKS:
            yield (o, b, 0) + case_state(synth, oracle, 2, o, b)
    p, X, S, prev, cur = case_state(synth, oracle, 2, "figure8", "after_frame")
    yield ("figure8", "after_frame", 1, dict(p, weight_type=1), X, S, prev, cur)


@pytest.mark.parametrize("mutant", NM.MUTANTS)
def test_a_wrong_restatement_misses_the_bound_by_100(synth, oracle, mutant):
    worst, where = 0.0, None
    for o, b, wt, p, X, S, prev, cur in _teeth_cases(synth, oracle):
        ref = NM.motion_step(X, S, prev, cur, p)
        bad = NM.motion_step(X, S, prev, cur, p, mutant=mutant)
        r = max(NM.ratios(ref, bad["mean"], bad["P12"], bad["P22"], bad["sigma"]).values())
        if r > worst:
            worst, where = r, (o, b, wt)
    print(f"MUTANT {mutant}: misses the bound by {worst:.3g} x at {where}")
    assert worst >= 100.0, (mutant, worst, where)


def test_the_oracle_holds_the_bound_under_weight_type_1(synth, oracle):
    """(the case the wc0 mutant is caught on is one the oracle passes)"""
    p, X, S, prev, cur = case_state(synth, oracle, 2, "figure8", "after_frame")
    p = dict(p, weight_type=1)
    ref = NM.motion_step(X, S, prev, cur, p)
    r = hold_oracle(oracle, 2, p, X, S, prev, cur, ref)
    print("MOTION-CPU weight type 1:", r)
    assert max(r.values()) <= 1.0, r


# ---- whole frames: what the GPU tests rely on ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MC.SEQUENCES)
def test_the_oracle_stays_clean_on_the_whole_frame_sequences(synth, oracle, name):
    """no theta clamp on one ordinary frame + three of the named kind at N = 21 (test_gpu_motion.py asserts the same at N = 21 and 43 next to its comparison)"""
    N = 21
    sc = MC.scene(synth, N)
    odo, z, matched = MC.sequence(synth, sc, name)
    o = oracle.Oracle(N, sc["params"])
    o.set_state(sc["X0"], np.triu(sc["S0"]))
    for t in range(4):
        _frame(o, oracle, sc, odo, z, matched, t)
    X, S = o.get_state()
    assert np.isfinite(X).all() and np.isfinite(S).all()
    assert o.clamp_stats()["theta"] == 0
    assert np.abs(X[-4:-2] - odo[4][:2]).max() < 0.05 and abs(X[-1] - odo[4][2]) < 0.05      # the filter follows the odometry
    o.close()
