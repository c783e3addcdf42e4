"""srukf_delete_landmarks on the device: K landmarks leave in one call — against the marginal P[keep, keep] and the oracle's K sequential
deleteOneFeature calls, against srukf_delete_landmark on a twin, with the records of the landmarks that leave, the appearance records of the ones that stay, K_new,
fp32 storage, and the identity gather of srukf_add_landmarks.

The scenes are the ones the K sequential deletions of the reference were measured on (CPU, oracle.delete_feature, ascending and descending): within 1e-15 of
P[keep, keep] and of each other, 9.4e-16 at N = 86."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [(6, [0, 5]), (6, [1, 2, 3]), (6, [0, 1, 2, 3, 4, 5]), (30, [3, 11, 12, 29]), (43, [0, 20, 21, 42]), (86, [5, 40, 41, 42, 85])]


def _posterior(srukf, synth, N, storage=None):
    """the posterior after one frame of make_scene(N, 2, seed=31 + N), as test_delete_landmark_matches_oracle builds it"""
    p = synth.scene_params()
    sc = synth.make_scene(N, 2, seed=31 + N, p=p)
    f = srukf.Filter(N, p)
    if storage is not None:
        f.set_storage(storage)
    f.set_state(sc["X0"], sc["S0"])
    f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement(); f.update(sc["z"][0], sc["matched"][0])
    return f, sc, p


def _keep(N, ids):
    lm = [k for k in range(N) if k not in set(ids)]
    rows = np.array([6 * k + e for k in lm for e in range(6)] + [6 * N + e for e in range(4)], dtype=int)
    return lm, rows


def _next_frame(f, sc, lm):
    N = sc["z"].shape[1] // 2
    z, m = sc["z"][1].reshape(N, 2)[lm].ravel(), sc["matched"][1][lm]
    f.predict_motion(sc["odo"][1], sc["odo"][2]); f.predict_measurement(); f.update(z, m)
    return z, m


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("N,ids", CASES)
def test_delete_landmarks_matches_marginal_and_oracle(srukf, oracle, synth, N, ids):
    f, sc, p = _posterior(srukf, synth, N)
    X, S = f.get_state()
    P = S.T @ S
    lm, keep = _keep(N, ids)
    Xo, So = X, S
    for k in sorted(ids, reverse=True):                          # the reference: K calls of deleteOneFeature, descending
        Xo, So = oracle.delete_feature(p, Xo, So, k)
    assert f.delete_landmarks(ids) is None
    K = len(ids)
    assert (f.N, f.n) == (N - K, 6 * (N - K) + 4)
    Xd, Sd = f.get_state()
    assert _same_bytes(Xd, X[keep])
    assert np.all(np.tril(Sd, -1) == 0.0)
    e_marg, e_orc = np.abs(Sd.T @ Sd - P[np.ix_(keep, keep)]).max(), np.abs(Sd.T @ Sd - So.T @ So).max()
    print(f"N={N} ids={ids}: |SdtSd - P[keep,keep]| = {e_marg:.3e}, |SdtSd - SotSo| = {e_orc:.3e}")
    assert e_marg <= 1e-13                                       # the existing single-deletion bound
    assert e_orc <= 1e-11                                        # the project's per-frame bound
    assert np.array_equal(Xd, Xo)
    if K < N:                                                    # the filter keeps running on the smaller map
        o = oracle.Oracle(N - K, p); o.set_state(Xd, Sd)
        z, m = _next_frame(f, sc, lm)
        o.predict_motion(sc["odo"][1], sc["odo"][2]); o.predict_measurement(); o.update(z, m, mode=oracle.Oracle.BATCHED)
        X2, S2 = f.get_state(); Xo2, So2 = o.get_state(); o.close()
        np.testing.assert_allclose(X2, Xo2, atol=1e-9)
        np.testing.assert_allclose(S2.T @ S2, So2.T @ So2, atol=1e-10)
    f.close()


@pytest.mark.parametrize("N,idx", [(6, 3), (30, 11), (43, 0)])
def test_one_landmark_is_delete_landmark(srukf, synth, N, idx):
    f, sc, p = _posterior(srukf, synth, N)
    g, _, _ = _posterior(srukf, synth, N)
    assert all(_same_bytes(a, b) for a, b in zip(f.get_state(), g.get_state()))
    f.delete_landmarks([idx]); g.delete_landmark(idx)
    assert (f.N, f.n, f.Na, f.L) == (g.N, g.n, g.Na, g.L) == (N - 1, 6 * N - 2, g.Na, g.L)
    assert all(_same_bytes(a, b) for a, b in zip(f.get_state(), g.get_state()))
    assert f.null_directions() == g.null_directions()
    lm, _ = _keep(N, [idx])
    _next_frame(f, sc, lm); _next_frame(g, sc, lm)
    assert all(_same_bytes(a, b) for a, b in zip(f.get_state(), g.get_state()))
    f.close(); g.close()


def test_order_of_the_ids_does_not_matter(srukf, synth):
    f, sc, p = _posterior(srukf, synth, 6)
    g, _, _ = _posterior(srukf, synth, 6)
    f.delete_landmarks([5, 0]); g.delete_landmarks([0, 5])
    assert all(_same_bytes(a, b) for a, b in zip(f.get_state(), g.get_state()))
    f.close(); g.close()


def test_refusals_leave_the_handle_as_it_was(srukf, synth):
    N = 6
    f, sc, p = _posterior(srukf, synth, N)
    f.stage_sequence(sc["odo"][1:], sc["z"][1:], sc["matched"][1:])
    X, S = f.get_state()
    for ids in ([2, 4, 2], [1, N], [-1], [0, 1, 2, 3, 4, 5, 5]):
        with pytest.raises(srukf.SrukfError) as e:
            f.delete_landmarks(ids)
        assert e.value.rc == -1 and "delete_landmarks" in str(e.value), (ids, str(e.value))
        with pytest.raises(srukf.SrukfError) as e:
            f.delete_landmarks(ids, records=True)
        assert e.value.rc == -1
    with pytest.raises(srukf.SrukfError) as e:
        f.delete_landmarks([])
    assert e.value.rc == -1
    assert f.N == N and f.n == 6 * N + 4
    X1, S1 = f.get_state()
    assert _same_bytes(X, X1) and _same_bytes(S, S1)
    f.run_frames(0, 1)                                            # the staged sequence is still there
    g = srukf.Filter(N, p); g.set_state(X, S); g.stage_sequence(sc["odo"][1:], sc["z"][1:], sc["matched"][1:]); g.run_frames(0, 1)
    assert all(_same_bytes(a, b) for a, b in zip(f.get_state(), g.get_state()))
    f.delete_landmarks([0])                                       # ... and a deletion drops it, as today
    with pytest.raises(srukf.SrukfError):
        f.run_frames(0, 1)
    f.close(); g.close()


# ---- appearance records ----
def _with_appearance(srukf, synth, N, who, seed=5):
    """the posterior filter with appearance records on the landmarks `who` (distinct random patches), one association behind them (the matchPatches are written)
    and the frame closed"""
    f, sc, p = _posterior(srukf, synth, N)
    rng = np.random.default_rng(seed + N)
    pose = f.get_state()[0][-4:]
    R0 = np.array([[np.cos(pose[3]), -np.sin(pose[3]), 0], [np.sin(pose[3]), np.cos(pose[3]), 0], [0, 0, 1.0]])
    f.predict_motion(sc["odo"][1], sc["odo"][2]); h, _, vis = f.predict_measurement()
    for k in who:
        px = np.clip(h.reshape(N, 2)[k], 30, 400) + rng.uniform(-1, 1, 2)
        f.set_landmark_appearance(k, rng.integers(1, 256, (21, 21), dtype=np.uint8), R0, pose[:3] + rng.normal(0, 1e-3, 3), px)
    frame = rng.integers(0, 256, (int(p["image_h"]), int(p["image_w"])), dtype=np.uint8)
    f.associate(frame)
    f.update(sc["z"][1], sc["matched"][1])
    return f, sc, p, rng


def _appearance(f):
    out = []
    for k in range(f.N):
        r = f.get_landmark_record(k)
        out.append({"patch": r["patch"], "R": r["R"], "t": r["t"], "px": r["px"], "has_app": r["has_app"], "tmpl": f.get_match_patch(k)})
    return out


def _assert_same_appearance(new, old, src):
    assert len(new) == len(src)
    for a, k in enumerate(src):
        assert new[a]["has_app"] == old[k]["has_app"], (a, k)
        for key in ("patch", "R", "t", "px", "tmpl"):
            assert _same_bytes(new[a][key], old[k][key]), (a, k, key)
        if not new[a]["has_app"]:
            assert not new[a]["patch"].any() and not new[a]["R"].any() and not new[a]["tmpl"].any(), (a, k)


def test_kept_landmarks_keep_their_appearance_records(srukf, synth):
    N, who = 6, [0, 2, 3, 5]
    f, sc, p, rng = _with_appearance(srukf, synth, N, who)
    before = _appearance(f)
    assert [b["has_app"] for b in before] == [k in who for k in range(N)]
    assert any(before[k]["tmpl"].any() for k in who)              # the association has written matchPatches
    assert len({before[k]["patch"].tobytes() for k in who}) == len(who)
    f.delete_landmarks([1, 3])
    lm, _ = _keep(N, [1, 3])                                      # 0, 2, 4, 5 -> records on 0, 1, 3
    after = _appearance(f)
    _assert_same_appearance(after, before, lm)
    assert [a["has_app"] for a in after] == [True, True, False, True]
    # back to 6 (the context of the first life comes back), records on the two new ones, then down to 4 again: the context that held 0, 2, 4, 5 is revived
    f.add_landmarks(np.array([[200.0, 150.0], [420.0, 300.0]]))
    R0 = before[0]["R"]
    for k in (4, 5):
        f.set_landmark_appearance(k, rng.integers(1, 256, (21, 21), dtype=np.uint8), R0, before[0]["t"], np.array([100.0 + k, 90.0]))
    mid = _appearance(f)
    _assert_same_appearance(mid[:4], after, range(4))             # the identity gather of srukf_add_landmarks
    f.delete_landmarks([4, 0])
    lm2, _ = _keep(6, [0, 4])                                     # 1, 2, 3, 5: slot 1 held a record in the context's past life and holds none now
    last = _appearance(f)
    _assert_same_appearance(last, mid, lm2)
    assert [a["has_app"] for a in last] == [True, False, True, True]
    f.close()


@pytest.mark.parametrize("N,ids,app", [(6, [4, 0, 3], False), (6, [4, 0, 3], True), (43, [42, 0, 21, 20], False), (43, [42, 0, 21, 20], True)])
def test_records_are_get_landmark_record_before_the_call(srukf, synth, N, ids, app):
    who = [k for k in range(N) if k % 3 != 1] if app else []
    if app:
        f, sc, p, _ = _with_appearance(srukf, synth, N, who)
        g, _, _, _ = _with_appearance(srukf, synth, N, who)
    else:
        f, sc, p = _posterior(srukf, synth, N)
        g, _, _ = _posterior(srukf, synth, N)
    assert all(_same_bytes(a, b) for a, b in zip(f.get_state(), g.get_state()))
    want = [g.get_landmark_record(k) for k in ids]
    X, S = f.get_state()
    rec = f.delete_landmarks(ids, records=True)
    assert sorted(rec) == sorted(["X6", "S66", "patch", "R", "t", "px", "has_app"])
    assert rec["X6"].shape == (len(ids), 6) and rec["S66"].shape == (len(ids), 6, 6) and rec["patch"].shape == (len(ids), 21, 21)
    for q, k in enumerate(ids):
        for key in ("X6", "S66", "patch", "R", "t", "px"):
            assert _same_bytes(np.ascontiguousarray(rec[key][q]), want[q][key]), (q, k, key)
        assert bool(rec["has_app"][q]) == want[q]["has_app"] == (k in who)
        assert _same_bytes(np.ascontiguousarray(rec["X6"][q]), X[6 * k:6 * k + 6])
    # asking for the records changes nothing of the deletion
    g.delete_landmarks(ids)
    assert all(_same_bytes(a, b) for a, b in zip(f.get_state(), g.get_state()))
    f.close(); g.close()


def test_k_new_counts_the_armed_landmarks_that_leave(srukf, synth):
    """add_landmarks arms K_new = 3; one old and one new landmark leave: the NEED_REORDER update behind it runs with K_new = 2, as on a twin that deleted
    the two one by one (the new one first: positions stay valid)"""
    p = synth.scene_params()
    N0, K = 10, 3
    sc = synth.make_scene(N0, 3, seed=22, p=p)
    uv = np.column_stack([np.random.default_rng(3).uniform(60, 580, K), np.random.default_rng(4).uniform(60, 420, K)])
    res = []
    for batched in (True, False):
        f = srukf.Filter(N0, p); f.set_state(sc["X0"], sc["S0"])
        f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement(); f.update(sc["z"][0], sc["matched"][0])
        f.add_landmarks(uv)
        if batched:
            f.delete_landmarks([2, N0 + 1])
        else:
            f.delete_landmark(N0 + 1); f.delete_landmark(2)
        assert f.N == N0 + K - 2
        f.predict_motion(sc["odo"][1], sc["odo"][2]); h, _, vis = f.predict_measurement()
        if batched:
            z, m = h + np.random.default_rng(9).normal(0, 0.5, h.shape), np.asarray(vis, dtype=np.int32)
        f.update(z, m, reorder=srukf.NEED_REORDER, mode=srukf.UPDATE_SEQUENTIAL)
        res.append(f.get_state())
        f.close()
    assert m[-2:].any()                                           # an armed landmark took part
    (Xa, Sa), (Xb, Sb) = res
    ex, ep = np.abs(Xa - Xb).max(), np.abs(Sa.T @ Sa - Sb.T @ Sb).max()
    print(f"NEED_REORDER after delete_landmarks vs one by one: |dX| = {ex:.3e}, |dP| = {ep:.3e}")
    assert ex <= 1e-9 and ep <= 1e-11


def test_fp32_storage_survives_the_call(srukf, synth):
    """P against the one-by-one twin at 2e-8: the bound of tests/test_gpu_step_random.py (_Pair.tp, one update behind a map change under fp32 storage:
    the two states are float roundings of nearly equal values)"""
    N, ids = 6, [1, 4]
    f, sc, p = _posterior(srukf, synth, N, storage=srukf.STORAGE_F32)
    g, _, _ = _posterior(srukf, synth, N, storage=srukf.STORAGE_F32)
    X, S = f.get_state()
    lm, keep = _keep(N, ids)
    f.delete_landmarks(ids)
    g.delete_landmark(4); g.delete_landmark(1)
    Xd, Sd = f.get_state(); X32, S32 = f.get_state_f32()
    assert np.array_equal(Xd, X32.astype(np.float64)) and np.array_equal(np.triu(Sd), np.triu(S32).astype(np.float64))     # still the float-rounded state
    assert _same_bytes(Xd, X[keep]) and np.all(np.tril(Sd, -1) == 0.0)
    Xg, Sg = g.get_state()
    assert _same_bytes(Xd, Xg)
    assert np.abs(Sd.T @ Sd - Sg.T @ Sg).max() <= 2e-8
    _next_frame(f, sc, lm)
    X2, S2 = f.get_state(); X32, S32 = f.get_state_f32()
    assert np.isfinite(X2).all() and np.isfinite(S2).all() and not _same_bytes(X2, Xd)
    assert np.array_equal(X2, X32.astype(np.float64))
    f.close(); g.close()


def test_add_landmarks_keeps_the_old_appearance_records(srukf, synth):
    """the identity table: srukf_add_landmarks moves the old landmarks' records with the launch a deletion issues"""
    N, who = 6, [0, 2, 3, 5]
    f, sc, p, rng = _with_appearance(srukf, synth, N, who)
    before = _appearance(f)
    X, _ = f.get_state()
    f.add_landmarks(np.array([[180.0, 140.0], [300.0, 260.0], [450.0, 330.0]]))
    assert f.N == N + 3
    _assert_same_appearance(_appearance(f)[:N], before, range(N))
    assert _same_bytes(f.get_state()[0][:6 * N], X[:6 * N])
    f.close()
