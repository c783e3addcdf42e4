"""numpy restatement of the map policy's verdict (cv-monoslam_amd/csrc/srukf_policy.hip): the counters of predictMeasurement / KalmanUpdate
(cslam.cpp:713-723, 751), the deletion tests of updateFeaturesInformation (cslam.cpp:446-462) and the addFeatures trigger (SLAM.cpp:556).  A pure function of
(state, X, h, vis, z, matched, params); nothing here reads the library."""
import numpy as np

UNMATCHED, RHO, BEHIND, PRED_BORDER, MATCH_BORDER, STORE = 1, 2, 4, 8, 16, 32
DELETE_BITS = UNMATCHED | RHO | BEHIND | PRED_BORDER | MATCH_BORDER
DEFAULTS = dict(border=20.0, rho_min=0.01, min_predictions=10, min_matches=5)
STATE_DTYPE = np.dtype([("nPredictTimes", np.int32), ("nMatchTimes", np.int32), ("predictLocation", np.float64, (2,))])
SUMMARY_FIELDS = ("n_predicts", "n_matches", "n_deletes", "n_stores", "n_predicts_after", "n_matches_after", "need_add", "change")


def zero_state(N):
    return np.zeros(N, dtype=STATE_DTYPE)


def policy(state, X, h, vis, z, matched, image_w, image_h, border=20.0, rho_min=0.01, min_predictions=10, min_matches=5, margins=None):
    """-> (verdict[N] int32, summary dict, new state).  X: the posterior (landmark k at 6k .. 6k + 5, the robot block last: X[n - 2] is what the BEHIND test reads).
    margins (a list): receives |value - threshold| of every real-valued test that was evaluated, for the caller's 1e-6 precondition."""
    X = np.asarray(X, dtype=np.float64).reshape(-1)
    N = len(state)
    n = 6 * N + 4
    assert X.size >= n
    h = np.asarray(h, dtype=np.float64).reshape(N, 2)
    z = np.asarray(z, dtype=np.float64).reshape(N, 2)
    vis = np.asarray(vis).reshape(N) != 0
    mt = np.asarray(matched).reshape(N) != 0
    st = np.array(state, dtype=STATE_DTYPE, copy=True)
    verdict = np.zeros(N, dtype=np.int32)
    W, H = float(image_w), float(image_h)

    def near_edge(x, y):
        vals = (x, y, W - x, H - y)
        if margins is not None:
            margins.extend(abs(v - border) for v in vals)
        return any(v < border for v in vals)

    n_del = n_store = 0
    for k in range(N):
        if vis[k]:                                                   # cslam.cpp:716-720 (not visible: the last predictLocation stays)
            st["nPredictTimes"][k] += 1
            st["predictLocation"][k] = h[k]
        if mt[k]:                                                    # cslam.cpp:751
            st["nMatchTimes"][k] += 1
        zi, theta, phi, rho = X[6 * k + 2], X[6 * k + 3], X[6 * k + 4], X[6 * k + 5]
        hlr_z = rho * (zi - X[n - 2]) + np.cos(phi) * np.cos(theta)  # cslam.cpp:447
        npt, nmt = int(st["nPredictTimes"][k]), int(st["nMatchTimes"][k])
        unmatched = npt > 2 * nmt and npt >= min_predictions        # cslam.cpp:449
        rho_low, behind = rho < rho_min, hlr_z < 0.0
        if margins is not None:
            margins.extend([abs(rho - rho_min), abs(hlr_z)])
        pred_b = near_edge(*st["predictLocation"][k])                # cslam.cpp:450
        match_b = bool(mt[k]) and near_edge(*z[k])                   # cslam.cpp:453-456
        hard = unmatched or rho_low or behind
        store = (not hard) and ((pred_b and mt[k]) or (not pred_b and match_b))      # cslam.cpp:460-462
        verdict[k] = (UNMATCHED * unmatched) | (RHO * rho_low) | (BEHIND * behind) | (PRED_BORDER * pred_b) | (MATCH_BORDER * match_b) | (STORE * bool(store))
        n_del += bool(verdict[k] & DELETE_BITS)
        n_store += bool(store)
    n_pred, n_match = int(vis.sum()), int(mt.sum())
    s = dict(n_predicts=n_pred, n_matches=n_match, n_deletes=n_del, n_stores=n_store, n_predicts_after=n_pred - n_del, n_matches_after=n_match - n_store)
    s["need_add"] = int(s["n_matches_after"] < min_matches)          # SLAM.cpp:556
    s["change"] = int(n_del > 0 or s["need_add"])
    return verdict, s, st
