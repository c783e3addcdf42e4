"""numpy restatement of the 1-point RANSAC consensus (srukf_ransac_consensus, include/srukf.h) on top of the CPU oracle.

An oracle filter that has run predict_motion + predict_measurement holds the sigma points (Oracle.sigma()) and their pixels (Oracle.Z()):
Pxy_i is formed from them as calculateOneFeatureCrossCovariance does (SLAM.cpp:2020-2038), the gain and the hypothesis' mean as KalmanUpdate
does (2077-2079), and the projection is oracle.project (1615-1690, zero pixel noise).  Every matched and visible landmark is a hypothesis.
"""
from __future__ import annotations

import numpy as np


def inv2(si):
    """OpenCV's closed-form 2 x 2 inverse (zero matrix when the determinant is zero)."""
    det = si[0, 0] * si[1, 1] - si[0, 1] * si[1, 0]
    if det == 0.0:
        return np.zeros((2, 2))
    d = 1.0 / det
    return np.array([[si[1, 1] * d, -si[0, 1] * d], [-si[1, 0] * d, si[0, 0] * d]])


def consensus(O, orc, params, z, matched, threshold=8.0):
    """orc: an oracle.Oracle after predict_motion (+ predict_measurement, which is run again here: it is idempotent).
    Returns a dict: active[N], D[N, N] (d_ij; nan outside A x A), ok[N, N] (projection valid), votes[N], best, inlier[N], dist[N]."""
    N, n = orc.N, orc.n
    z = np.asarray(z, dtype=np.float64)
    h, Si, vis = orc.predict_measurement()
    X, _ = orc.get_state()
    active = (np.asarray(matched) != 0) & (vis != 0)
    A = np.flatnonzero(active)
    out = {"active": active, "D": np.full((N, N), np.nan), "ok": np.zeros((N, N), dtype=bool), "votes": np.zeros(N, dtype=np.int64),
           "best": -1, "inlier": np.zeros(N, dtype=np.int64), "dist": np.zeros(N)}
    if A.size == 0:
        return out
    Na = n + 5
    w = O.sample_parameter(Na, int(params.get("weight_type", 0)), params["ut_alpha"], params["ut_beta"])
    wc = np.full(2 * Na + 1, w["wi"])
    wc[0] = w["wc0"]
    sig, Z = orc.sigma()[:n], orc.Z()
    dev = (sig - X[:, None]) * wc                                # sub1 * weight, SLAM.cpp:2030-2036
    Pxy_all = dev @ (Z - h[:, None]).T                           # n x 2N: columns 2i, 2i + 1 are Pxy_i
    feats, poss, psis = [], [], []
    for i in A:
        sii = inv2(Si[i])
        K = Pxy_all[:, 2 * i:2 * i + 2] @ sii @ sii.T            # 2078
        x = X + K @ (z[2 * i:2 * i + 2] - h[2 * i:2 * i + 2])    # 2079
        feats.append(x[:6 * N].reshape(N, 6)[A])
        poss.append(np.broadcast_to(x[n - 4:n - 1], (A.size, 3)))
        psis.append(np.full(A.size, x[n - 1]))
    uv = O.project(params, np.concatenate(feats), np.concatenate(poss), np.concatenate(psis), np.zeros((A.size * A.size, 2)))
    uv = uv.reshape(A.size, A.size, 2)
    zz = z.reshape(N, 2)[A]
    d = np.sqrt(((zz[None] - uv) ** 2).sum(axis=2))
    ok = (uv[..., 0] != 0.0) & (uv[..., 1] != 0.0)               # predictMeasurement's visibility test, 1727
    out["D"][np.ix_(A, A)] = d
    out["ok"][np.ix_(A, A)] = ok
    inl = ok & (d < threshold)
    out["votes"][A] = inl.sum(axis=1)
    b = int(np.argmax(out["votes"][A]))                          # (argmax returns the first maximum: the lowest landmark index)
    out["best"] = int(A[b])
    out["inlier"][A] = inl[b]
    out["dist"][A] = d[b]
    return out


def compare(res, inlier, votes, dist, best, threshold, tol):
    """Device results against the restatement `res`: dist within tol; votes / inlier / best exactly, except that a pair whose restated d_ij lies within
    tol of the threshold is left out (a hypothesis whose count then is ambiguous is compared as an interval).  Returns (max |ddist|, share of pairs left out)."""
    A = np.flatnonzero(res["active"])
    assert np.array_equal(np.asarray(votes)[~res["active"]], np.zeros((~res["active"]).sum(), dtype=np.int64))
    if A.size == 0:
        assert best == -1
        return 0.0, 0.0
    D, ok = res["D"][np.ix_(A, A)], res["ok"][np.ix_(A, A)]
    amb = ok & (np.abs(D - threshold) <= tol)
    sure = ok & (D < threshold) & ~amb
    lo, hi = sure.sum(axis=1), sure.sum(axis=1) + amb.sum(axis=1)
    v = np.asarray(votes)[A]
    assert np.all((lo <= v) & (v <= hi)), (v, lo, hi)
    share = float(amb.sum()) / float(amb.size)
    cand = A[hi >= lo.max()]                                     # hypotheses that can hold the maximum
    assert best in cand, (best, cand)
    if not amb.any():
        assert best == res["best"] and np.array_equal(np.asarray(votes), res["votes"]) and np.array_equal(np.asarray(inlier), res["inlier"])
    err = 0.0
    if best == res["best"]:
        err = float(np.abs(np.asarray(dist) - res["dist"]).max())
        b = int(np.flatnonzero(A == best)[0])
        keep = ~amb[b]
        assert np.array_equal(np.asarray(inlier)[A][keep], sure[b][keep].astype(np.int64))
    return err, share
