"""The numpy restatement of the 1-point RANSAC consensus (tests/np_ransac.py) against itself on constructed cases.  Runs without a GPU."""
import numpy as np
import pytest

import np_ransac


def _predicted(O, synth, N, seed, warm=2):
    """An oracle filter that has predicted frame `warm` of a synthetic scene (after `warm` whole frames), and that frame's h, visible."""
    p = synth.scene_params()
    sc = synth.make_scene(N, warm + 2, seed=seed, p=p)
    o = O.Oracle(N, p)
    o.set_state(sc["X0"], sc["S0"])
    for t in range(warm):
        o.predict_motion(sc["odo"][t], sc["odo"][t + 1]); o.predict_measurement()
        o.update(sc["z"][t], sc["matched"][t], 1, 0, O.Oracle.BATCHED)
    o.predict_motion(sc["odo"][warm], sc["odo"][warm + 1])
    h, Si, vis = o.predict_measurement()
    return p, o, h, vis


@pytest.mark.parametrize("N,seed", [(10, 3), (16, 5)])
def test_all_consistent_everyone_votes_M(oracle, synth, N, seed):
    p, o, h, vis = _predicted(oracle, synth, N, seed)
    rng = np.random.default_rng(seed)
    matched = np.ones(N, dtype=np.int32); matched[N // 2] = 0
    z = h + rng.normal(0, 0.3, 2 * N)
    r = np_ransac.consensus(oracle, o, p, z, matched)
    A = np.flatnonzero((matched != 0) & (vis != 0))
    assert A.size >= N - 3
    assert np.array_equal(r["votes"][A], np.full(A.size, A.size)) and r["votes"][N // 2] == 0
    assert r["best"] == A[0]
    assert np.array_equal(np.flatnonzero(r["inlier"]), A)
    assert r["dist"][N // 2] == 0.0 and np.all(r["dist"][A] < 8.0)


@pytest.mark.parametrize("N,seed,outliers", [(12, 3, (0,)), (16, 7, (0, 5, 11))])
def test_gross_outliers_are_the_complement(oracle, synth, N, seed, outliers):
    p, o, h, vis = _predicted(oracle, synth, N, seed)
    rng = np.random.default_rng(seed)
    matched = np.ones(N, dtype=np.int32)
    z = h + rng.normal(0, 0.3, 2 * N)
    for q, k in enumerate(outliers):                             # pixels moved by tens of pixels
        z[2 * k:2 * k + 2] += (45.0 + 7 * q) * np.array([np.cos(1.0 + q), np.sin(1.0 + q)])
    r = np_ransac.consensus(oracle, o, p, z, matched)
    A = np.flatnonzero(vis != 0)
    good = np.array([k for k in A if k not in outliers])
    assert all(k in A for k in outliers) and good.size >= 2
    assert np.array_equal(np.flatnonzero(r["inlier"]), good)     # the mask is exactly the complement
    assert np.all(r["votes"][good] == good.size)                 # every clean hypothesis sees the clean set: a tie ...
    # ... that the lowest index wins.  (A displaced landmark that is weakly tied to the pose moves mostly itself: its hypothesis then still sees the whole
    # clean set, without itself, and takes part in the tie.)
    assert np.all(r["votes"][list(outliers)] <= good.size)
    assert r["best"] == np.flatnonzero(r["votes"] == good.size)[0]
    assert np.all(r["dist"][list(outliers)] > 8.0)


def test_empty_set_gives_minus_one(oracle, synth):
    p, o, h, vis = _predicted(oracle, synth, 8, 2)
    r = np_ransac.consensus(oracle, o, p, h.copy(), np.zeros(8, dtype=np.int32))
    assert r["best"] == -1 and not r["votes"].any() and not r["inlier"].any() and not r["dist"].any()
    np_ransac.compare(r, r["inlier"], r["votes"], r["dist"], -1, 8.0, 1e-6)


def test_compare_accepts_itself_and_catches_a_wrong_vote(oracle, synth):
    p, o, h, vis = _predicted(oracle, synth, 10, 4)
    z = h + np.random.default_rng(1).normal(0, 0.3, 20); z[0:2] += 60.0
    r = np_ransac.consensus(oracle, o, p, z, np.ones(10, dtype=np.int32))
    err, share = np_ransac.compare(r, r["inlier"], r["votes"], r["dist"], r["best"], 8.0, 1e-6)
    assert err == 0.0 and share == 0.0
    bad = r["votes"].copy(); bad[r["best"]] -= 1
    with pytest.raises(AssertionError):
        np_ransac.compare(r, r["inlier"], bad, r["dist"], r["best"], 8.0, 1e-6)
