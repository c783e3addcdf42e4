"""GPU tests of loop points (srukf_get_landmark_record / srukf_insert_landmarks, include/srukf.h): the record's factor equals the numpy
restatement (tests/np_loop.py) bit for bit on the device's own P66, the insertion is the numpy placement bit for bit, K_new and the frames behind an
insertion keep to the oracle, records survive a round trip, a revived context gives a new slot no stale appearance, and the CSLAM facade puts the loop
points of a redirection restart back into the filter (host/cslam_vision.cpp `loops`)."""
import os

import numpy as np
import pytest

import np_loop as LP
from test_gpu_detect import VISION, _host_cut, _parse, _run_vision, params, texture

pytestmark = pytest.mark.gpu
BAD_ARG = -1


def _sigma4(p):
    return np.diag([p["sigma_x"], p["sigma_y"], p["sigma_z"], p["sigma_theta"]])


def _after_one_frame(srukf, synth, N, seed):
    """a filter of N landmarks one batched frame into a synthetic scene (cross-covariances everywhere)"""
    p = synth.scene_params()
    sc = synth.make_scene(N, 8, seed=seed, p=p)
    f = srukf.Filter(N, p)
    f.set_state(sc["X0"], sc["S0"])
    if N > 0:
        f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement(); f.update(sc["z"][0], sc["matched"][0])
    return f, sc, p


def _blocks(rng, L):
    X6 = rng.normal(size=(L, 6))
    S66 = np.triu(rng.normal(scale=0.1, size=(L, 6, 6)))
    for j in range(L):
        S66[j][np.diag_indices(6)] = np.abs(S66[j][np.diag_indices(6)]) + 0.05
    return X6, S66


def _captured(srukf, synth, seed=21, n=8):
    """a filter whose landmarks were initialised at GFTT points of a texture and had their appearance captured on the device"""
    p = params(synth)
    img = texture(seed)
    f = srukf.Filter(0, p)
    f.set_state(np.array([0.1, 0.05, 0.0, 0.3]), _sigma4(p))
    uv, _ = f.detect_features(img, max_corners=n, unfiltered=True)
    f.add_landmarks(uv)
    f.capture_appearance(0, uv, img)
    return f, p, img, uv


def test_record_factor_is_bit_identical_to_the_restatement(srukf, synth):
    f, p, img, uv = _captured(srukf, synth)
    X, _ = f.get_state()
    for k in range(f.N):
        r = f.get_landmark_record(k)
        _, P66 = f.get_landmark_block(k)
        assert np.array_equal(r["S66"], LP.chol6(P66, p["epsilon"])), k
        assert np.array_equal(r["X6"], X[6 * k:6 * k + 6])
        assert r["has_app"] and np.array_equal(r["patch"], _host_cut(img, *uv[k]))
        assert np.array_equal(r["px"], uv[k])
    g, sc, p2 = _after_one_frame(srukf, synth, 12, 41)             # dense cross-covariances, no appearance records
    X, _ = g.get_state()
    for k in (0, 5, 11):
        r = g.get_landmark_record(k)
        _, P66 = g.get_landmark_block(k)
        assert np.array_equal(r["S66"], LP.chol6(P66, p2["epsilon"]))
        np.testing.assert_allclose(r["S66"].T @ r["S66"], P66, rtol=0, atol=1e-14 * np.abs(P66).max())
        assert np.array_equal(r["X6"], X[6 * k:6 * k + 6])
        assert not r["has_app"] and not r["patch"].any() and not r["R"].any()


@pytest.mark.parametrize("N", [0, 8, 200])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_insert_is_the_numpy_placement(srukf, synth, N, L, storage):
    f, sc, p = _after_one_frame(srukf, synth, N, 50 + N)
    if storage == "f32":
        f.set_storage(srukf.STORAGE_F32)
    X, S = f.get_state()
    X6, S66 = _blocks(np.random.default_rng(N + L), L)
    if storage == "f32":                                             # the stored state is the float rounding of what goes in
        X6e, S66e = X6.astype(np.float32).astype(np.float64), S66.astype(np.float32).astype(np.float64)
    else:
        X6e, S66e = X6, S66
    Xe, Se = LP.place(X, S, 0, X6e, S66e)
    f.insert_landmarks(X6, S66)
    assert (f.N, f.n) == (N + L, 6 * (N + L) + 4)
    X2, S2 = f.get_state()
    assert np.array_equal(X2, Xe)
    assert np.all(np.tril(S2, -1) == 0.0)
    if f.null_directions() == 0:
        assert np.array_equal(S2, Se)
    else:                                                            # null rows are rewritten as sqrt(EPSILON) e_k (rank-aware form)
        Pe = Se.T @ Se
        np.testing.assert_allclose(S2.T @ S2, Pe, rtol=0, atol=1e-12 * np.abs(Pe).max())
    if storage == "f32":
        X32, S32 = f.get_state_f32()
        assert np.array_equal(X32.astype(np.float64), X2) and np.array_equal(np.triu(S32).astype(np.float64), S2)


def _restart(srukf, synth, N, seed, ks):
    """the redirection restart the loop points are for: a fresh 4-state filter at the pose of a filter one frame into a scene, and the records of its
    landmarks ks put into it (archived mean, marginal factor, no cross-covariance)"""
    f, sc, p = _after_one_frame(srukf, synth, N, seed)
    X, _ = f.get_state()
    recs = [f.get_landmark_record(k) for k in ks]
    g = srukf.Filter(0, p)
    g.set_state(np.r_[X[-4:-2], 0.0, X[-1]], _sigma4(p))
    g.insert_landmarks(np.array([r["X6"] for r in recs]), np.array([r["S66"] for r in recs]))
    f.close()
    return g, sc, p


def _frame_vs_oracle(oracle, f, p, odo0, odo1, rng, reorder=1, k_new=0, mode=1):
    """one frame of f against the oracle started from f's own state: the per-frame bounds |dX| <= 1e-9, |dP| <= 1e-11 (relative to |P| beyond 1)"""
    X, S = f.get_state()
    o = oracle.Oracle(f.N, p); o.set_state(X, S)
    f.predict_motion(odo0, odo1); h, _, vis = f.predict_measurement()
    o.predict_motion(odo0, odo1); _, _, viso = o.predict_measurement()
    assert np.array_equal(vis, viso)
    z = h + rng.normal(0, 0.1, h.shape); m = np.asarray(vis, dtype=np.int32)
    f.update(z, m, reorder=reorder, mode=mode)
    o.update(z, m, reorder=reorder, k_new=k_new, mode=mode)
    X2, S2 = f.get_state(); Xo, So = o.get_state()
    o.close()
    P, Po = S2.T @ S2, So.T @ So
    assert np.abs(X2 - Xo).max() <= 1e-9 * max(1.0, np.abs(Xo).max()), np.abs(X2 - Xo).max()
    assert np.abs(P - Po).max() <= 1e-11 * max(1.0, np.abs(Po).max()), (np.abs(P - Po).max(), np.abs(Po).max())
    return z, m


def test_insert_keeps_k_new_for_the_reorder_update(srukf, oracle, synth):
    """insert_landmarks(L) into the restart filter, add_landmarks(K): the K armed landmarks stay last and K_new = K keeps its meaning — the NEED_REORDER
    frame equals the oracle's with k_new = K in X, and the device's own frame from the same state through set_state + set_new_landmarks(K) bit for bit.
    (P is not compared with the oracle here: behind the frame it is no longer well conditioned — DESIGN.md §12.)"""
    g, sc, p = _restart(srukf, synth, 10, 61, range(10))
    rng = np.random.default_rng(7)
    K = 4
    g.add_landmarks(np.column_stack([rng.uniform(80, 560, K), rng.uniform(80, 400, K)]))
    X6, S66 = np.array([g.get_landmark_record(k)["X6"] for k in (1, 4)]), np.array([g.get_landmark_record(k)["S66"] for k in (1, 4)])
    g.insert_landmarks(X6 + 1e-3, S66)                               # K_new = 4 armed: these two go in front of the four
    assert g.N == 16
    X, S = g.get_state()
    assert np.array_equal(X[60:72], (X6 + 1e-3).ravel())            # landmarks 10, 11: behind the ten, in front of the four armed ones
    twin = srukf.Filter(g.N, p); twin.set_state(X, S); twin.set_new_landmarks(K)
    o = oracle.Oracle(g.N, p); o.set_state(X, S)
    res = []
    for f in (g, twin):
        f.predict_motion(sc["odo"][1], sc["odo"][2]); h, _, vis = f.predict_measurement()
        z = h + np.random.default_rng(3).normal(0, 0.1, h.shape); m = np.asarray(vis, dtype=np.int32)
        f.update(z, m, reorder=srukf.NEED_REORDER, mode=srukf.UPDATE_SEQUENTIAL)
        res.append(f.get_state())
    o.predict_motion(sc["odo"][1], sc["odo"][2]); o.predict_measurement()
    o.update(z, m, reorder=oracle.Oracle.NEED_REORDER, k_new=K, mode=oracle.Oracle.SEQUENTIAL)
    Xo, _ = o.get_state(); o.close()
    assert m[10:12].all() and m[12:].sum() >= 1                        # inserted and armed landmarks took part
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert np.abs(res[0][0] - Xo).max() <= 1e-9, np.abs(res[0][0] - Xo).max()


def test_frames_after_an_insert_against_the_oracle_and_the_staged_replay(srukf, oracle, synth):
    g, sc, p = _restart(srukf, synth, 30, 71, range(30))
    X1, S1 = g.get_state()
    b = srukf.Filter(g.N, p); b.set_state(X1, S1)
    rng = np.random.default_rng(5)
    F = 5
    odo = sc["odo"][1:F + 2]
    zs, ms, traj = [], [], []
    for t in range(F):
        z, m = _frame_vs_oracle(oracle, g, p, odo[t], odo[t + 1], rng)
        zs.append(z); ms.append(m)
        pose, _ = g.get_robot(); traj.append(pose)
    assert np.array(ms).sum() >= 5 * 20
    b.stage_sequence(odo, np.array(zs), np.array(ms))
    tb = b.run_frames(0, F)
    Xg, Sg = g.get_state(); Xb, Sb = b.get_state()
    assert np.array_equal(Xg, Xb) and np.array_equal(Sg, Sb)
    assert np.array_equal(np.array(traj), tb[:, :4])


def test_record_delete_insert_round_trip(srukf, synth):
    f, sc, p = _after_one_frame(srukf, synth, 8, 81)
    for k in (7, 3):
        X, S = f.get_state()
        N = f.N
        r = f.get_landmark_record(k)
        _, P66 = f.get_landmark_block(k)
        f.delete_landmark(k)
        Xd, Sd = f.get_state()
        f.insert_landmarks(r["X6"], r["S66"])                        # (K_new = 0: the landmark comes back behind the map)
        X2, S2 = f.get_state()
        order = np.r_[0:6 * k, 6 * k + 6:6 * N, 6 * k:6 * k + 6, 6 * N:6 * N + 4]
        assert np.array_equal(X2, X[order])
        P2 = S2.T @ S2
        b = slice(6 * (N - 1), 6 * N)
        np.testing.assert_allclose(P2[b, b], P66, rtol=0, atol=1e-14 * np.abs(P66).max())
        assert not P2[b, :6 * (N - 1)].any() and not P2[b, 6 * N:].any()             # no cross-covariance
        keep = np.r_[0:6 * (N - 1), 6 * N:6 * N + 4]
        np.testing.assert_allclose(P2[np.ix_(keep, keep)], (Sd.T @ Sd), rtol=0, atol=1e-14)


def test_revived_context_gives_a_new_slot_no_stale_record(srukf, synth):
    res = {}
    for mode in ("none", "patch", "host"):
        f, p, img, uv = _captured(srukf, synth, seed=23)
        img2 = np.roll(img, (1, 2), axis=(0, 1))
        K = f.N
        f.set_new_landmarks(0)
        r = f.get_landmark_record(K - 1)
        f.delete_landmark(K - 1)                                     # the context of K landmarks (records in every slot) is retired ...
        if mode == "patch":
            f.insert_landmarks(r["X6"], r["S66"], patches=r["patch"][None], R=r["R"][None], t=r["t"][None], px=r["px"][None])
        else:                                                        # ... and revived here: the new slot must not inherit its old record
            f.insert_landmarks(r["X6"], r["S66"])
            assert not f.get_landmark_record(K - 1)["has_app"]
            if mode == "host":
                f.set_landmark_appearance(K - 1, _host_cut(img, *uv[K - 1]), r["R"], r["t"], uv[K - 1])
        assert f.N == K
        f.predict_motion(np.zeros(3), np.array([0.01, 0.004, 0.002]))
        f.predict_measurement()
        res[mode] = f.associate(img2)
        f.close()
    z, m, corr = res["none"]
    assert m[-1] == 0
    # the revived slot held this very patch in its past life: a stale record would correlate exactly as the record put back with its patch does
    assert corr[-1] != res["patch"][2][-1]
    assert np.array_equal(corr[:-1], res["patch"][2][:-1]) and np.array_equal(m[:-1], res["patch"][1][:-1])
    for a, b in zip(res["patch"], res["host"]):                     # the record put back with its patch associates as the host-cut one does
        assert np.array_equal(a, b)


def test_bad_arguments(srukf, synth):
    f, sc, p = _after_one_frame(srukf, synth, 4, 91)
    X6, S66 = _blocks(np.random.default_rng(1), 2)
    lib = f._lib
    assert lib.srukf_insert_landmarks(f._h, 0, None, None, None, None, None, None) == BAD_ARG

    def rc(fn):
        with pytest.raises(srukf.SrukfError) as e:
            fn()
        return e.value.rc
    bad = X6.copy(); bad[1, 3] = np.nan
    assert rc(lambda: f.insert_landmarks(bad, S66)) == BAD_ARG
    bad = S66.copy(); bad[0, 0, 0] = np.inf
    assert rc(lambda: f.insert_landmarks(X6, bad)) == BAD_ARG
    bad = S66.copy(); bad[1, 4, 2] = 1e-3
    assert rc(lambda: f.insert_landmarks(X6, bad)) == BAD_ARG
    patches = np.zeros((2, 21, 21), dtype=np.uint8)
    assert rc(lambda: f.insert_landmarks(X6, S66, patches=patches)) == BAD_ARG
    assert rc(lambda: f.insert_landmarks(X6, S66, patches=patches, R=np.zeros((2, 9)), t=np.zeros((2, 3)), px=np.full((2, 2), np.nan))) == BAD_ARG
    assert rc(lambda: f.get_landmark_record(4)) == BAD_ARG and rc(lambda: f.get_landmark_record(-1)) == BAD_ARG
    assert f.N == 4                                                  # nothing changed
    f.insert_landmarks(X6, S66)
    assert f.N == 6


def _vision_records(out):
    """per frame: the parsed frame record of test_gpu_detect plus `ids` [(ID, isLoop)]; and the `reinsert` lines"""
    frames = _parse(out)
    ids, reins, fr = [], [], -1
    for line in out.splitlines():
        t = line.split()
        if not t:
            continue
        if t[0] == "frame":
            fr = int(t[1])
        elif t[0] == "ids":
            ids.append(np.array([int(v) for v in t[1:]], dtype=np.int64).reshape(-1, 2))
        elif t[0] == "reinsert":
            a, i, x, s = t.index("archive"), t.index("ids"), t.index("x6"), t.index("sr")
            reins.append({"frame": fr + 1, "call": int(t[2]), "archive": [int(v) for v in t[a + 2:i]], "ids": [int(v) for v in t[i + 2:t.index("n_after")]],
                          "n_after": int(t[t.index("n_after") + 1]), "archived_after": int(t[t.index("archived_after") + 1]),
                          "x6": np.array([float(v) for v in t[x + 1:s]]).reshape(-1, 6), "sr": np.array([float(v) for v in t[s + 1:]]).reshape(-1, 6, 6)})
    assert len(ids) == len(frames)
    for f, i in zip(frames, ids):
        f["ids"] = i
    return frames, reins


def _strip(out):
    return [line for line in out.splitlines() if line.split()[:1] not in (["ids"], ["reinsert"])]


def test_facade_reinserts_the_loop_points_of_a_restart(tmp_path):
    assert os.path.exists(VISION), "run __graft_entry__.build() first"
    base = texture(31)
    frames = [np.roll(base, (0, s), axis=(0, 1)) for s in range(4)]
    odo = [(0.01 * i, 0.0, 0.0) for i in range(7)]
    plain = _run_vision(str(tmp_path), frames, odo, "redirect=3")
    out = _run_vision(str(tmp_path), frames, odo, "redirect=3", "loops")
    assert not any(line.split()[:1] in (["ids"], ["reinsert"]) for line in plain.splitlines())
    recs, reins = _vision_records(out)
    assert len(recs) == 5 and len(reins) == 1                         # one restart
    rn = reins[0]
    fr = rn["frame"]
    assert fr >= 1
    # up to the restart the switch changes nothing the host sees
    n_before = sum(1 for line in plain.splitlines() if line.startswith("frame ") and int(line.split()[1]) < fr)
    cut = [i for i, line in enumerate(plain.splitlines()) if line.startswith("frame ")][n_before - 1] + 1
    assert _strip(out)[:cut + 2] == plain.splitlines()[:cut + 2]       # (frame line, init, pose of the last frame before the restart)
    rec, prev = recs[fr], recs[fr - 1]
    last = [ps for ps in rec["passes"] if int(ps["call"]) == rn["call"]][-1]
    assert bool(last["proj"])                                         # the restart's isAdding pass
    first_reported = []
    for a in last["loops"][:, 1].tolist():                            # the last pass's loops, one per archived entry, in the order first reported
        if a not in first_reported:
            first_reported.append(a)
    L, K = len(rn["ids"]), len(last["uv"]) // 2
    assert L >= 1 and L == len(first_reported)
    archive = rn["archive"] + prev["ids"][:, 0].tolist()              # the archive the restart searched: what was there + the whole map it left
    assert rn["ids"] == [archive[a] for a in first_reported]
    arch = last["arch"].reshape(-1, 6)
    assert len(arch) == len(archive)
    assert np.array_equal(rn["x6"], arch[first_reported])             # the archived state goes back in
    for s in rn["sr"]:
        assert np.all(np.tril(s, -1) == 0.0) and np.all(np.diag(s) > 0)
    assert rn["n_after"] == L + K                                     # m_nMapFeatures behind the restart's addFeatures
    assert rn["archived_after"] == len(archive) - L                   # the archive shrinks by L
    ids = rec["ids"]
    loops = ids[ids[:, 1] == 1, 0].tolist()
    assert loops and ids[:len(loops), 1].all()                        # the loop nodes come first ...
    assert loops == [i for i in rn["ids"] if i in loops]              # ... in the order they went in (the deletion policy may have removed some since)
    before = set()
    for r in recs[:fr]:
        before |= set(r["ids"][:, 0].tolist())
    assert set(loops) <= before                                       # a loop node keeps the ID it had
    for r in recs:
        assert len(set(r["ids"][:, 0].tolist())) == len(r["ids"])    # no ID twice in a map
    for r in recs[fr:]:
        fresh = r["ids"][r["ids"][:, 1] == 0, 0]
        assert not (set(fresh.tolist()) & before)                     # ID is not advanced for loop points, and never reused
