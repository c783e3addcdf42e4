"""Numpy restatement of the joint measurement update: one Kalman update over all of a frame's matches with the full
innovation covariance, in place of the reference's per-landmark gains that are all taken from the same prior and added (SLAM.cpp:2070-2080).

    Pzz  = wi sum_{i not noise} dZ_i dZ_i^T  +  blockdiag_k( wi sum_{i in noise} dZ_i[2k:2k+2] dZ_i[2k:2k+2]^T ),   dZ_i = Z_i - Z_0  (i >= 1)
    Pzz  = R^T R,   U^T = R^-T Pxy^T,   w = R^-T (z - h),   X += U w,   S <- gmw(S^T S - U U^T)

`noise` are the four sigma points of the two pixel-noise directions (augmented indices n+3, n+4): the reference adds the same two err components to
every landmark, which a joint covariance would read as perfectly correlated pixel noise, so here every landmark keeps its own (the 2 x 2 diagonal
blocks are exactly the reference's Si^T Si).  A row pair of a landmark that is unmatched, invisible or has a singular Si is replaced by identity rows / columns in Pzz, zero
columns in Pxy and a zero innovation: the result is exact and needs no compaction.

joint_arrays takes Z, h, X, S, Pxy as arrays (any float dtype), so it can be fed a device's own buffers or run in numpy.longdouble;
NpJointFilter.update_joint is the same on NpFilter's frame."""
from __future__ import annotations

import numpy as np
from scipy.linalg import solve_triangular

from np_filter import NpFilter, gmw


def noise_columns(n, Na):
    """columns of dZ (sigma points 1 .. 2 Na, so sigma index - 1) that belong to the two pixel-noise directions"""
    return np.array([n + 3, n + 4, Na + n + 3, Na + n + 4])


def si_det(Si):
    """det of the N 2 x 2 factors Si (N x 2 x 2)"""
    Si = np.asarray(Si).reshape(-1, 2, 2)
    return Si[:, 0, 0] * Si[:, 1, 1] - Si[:, 0, 1] * Si[:, 1, 0]


def chol_upper(A):
    """R upper with A = R^T R.  float64: LAPACK; any other dtype (numpy.longdouble): the same right-looking loop the device runs, in that dtype."""
    if A.dtype == np.float64:
        return np.linalg.cholesky(A).T
    A = A.copy()
    m = A.shape[0]
    for j in range(m):
        if not A[j, j] > 0:
            raise np.linalg.LinAlgError("non-positive pivot %d" % j)
        A[j, j:] = A[j, j:] / np.sqrt(A[j, j])
        A[j + 1:, j + 1:] -= np.outer(A[j, j + 1:], A[j, j + 1:])
    return np.triu(A)


def solve_rt(R, B):
    """R^-T B (forward substitution with the lower triangle R^T)"""
    if R.dtype == np.float64:
        return solve_triangular(R, B, trans="T", lower=False)
    Y = np.array(B, dtype=R.dtype, copy=True)
    for i in range(R.shape[0]):
        Y[i] = (Y[i] - R[:i, i] @ Y[:i]) / R[i, i]
    return Y


def joint_pzz(Z, wi, n, Na, active):
    """Pzz (2N x 2N) from Z (2N x L) with the per-landmark noise blocks and identity rows / columns for inactive row pairs"""
    M = Z.shape[0]
    dZ = Z[:, 1:] - Z[:, :1]
    nz = noise_columns(n, Na)
    keep = np.ones(dZ.shape[1], dtype=bool)
    keep[nz] = False
    C = dZ[:, keep]
    Pzz = wi * (C @ C.T)
    for k in range(M // 2):
        B = dZ[2 * k:2 * k + 2][:, nz]
        Pzz[2 * k:2 * k + 2, 2 * k:2 * k + 2] += wi * (B @ B.T)
    on = np.repeat(np.asarray(active, dtype=bool), 2)
    Pzz[~on, :] = 0
    Pzz[:, ~on] = 0
    Pzz[~on, ~on] = 1
    return Pzz


def joint_arrays(Z, h, X, S, Pxy, z, active, wi, n, Na):
    """The joint update on arrays: Z (2N x L), h (2N), X (n), S (n x n upper), Pxy (n x 2N), z (2N), active (N bools).
    Returns dict(X, G = S^T S - U U^T, R, Ut (2N x n), w, Pzz).  The dtype is Z's."""
    dt = Z.dtype
    on = np.repeat(np.asarray(active, dtype=bool), 2)
    Pzz = joint_pzz(Z, dt.type(wi), n, Na, active)
    Pxy = np.where(on[None, :], np.asarray(Pxy, dtype=dt), dt.type(0))
    innov = np.where(on, np.asarray(z, dtype=dt) - np.asarray(h, dtype=dt), dt.type(0))
    R = chol_upper(Pzz)
    Ut = solve_rt(R, Pxy.T)
    w = solve_rt(R, innov)
    S = np.asarray(S, dtype=dt)
    return {"X": np.asarray(X, dtype=dt) + Ut.T @ w, "G": S.T @ S - Ut.T @ Ut, "R": R, "Ut": Ut, "w": w, "Pzz": Pzz}


class NpJointFilter(NpFilter):
    """NpFilter with the joint update.  update_joint(z, matched) replaces update(z, matched, mode) for a frame."""

    def active(self, matched):
        """matched, visible, Si not singular (a landmark whose sigma points all leave the image has h != 0 and Si = 0: the reference's closed-form inverse of a
        singular Si is zero, so it contributes nothing there and is inactive here)"""
        vis = (self.h[0::2] != 0) & (self.h[1::2] != 0)
        return (np.asarray(matched) != 0) & vis & (si_det(self.Si) != 0)

    def cross_covariance(self, dtype=np.float64):
        """Pxy (n x 2N) from the single prior, as the reference's BATCHED form takes it for every landmark"""
        wc = self.w.astype(dtype)
        wc[0] = self.wc0
        sig, Z = self.sig[:self.n].astype(dtype), self.Z.astype(dtype)
        return ((sig - self.X.astype(dtype)[:, None]) * wc) @ (Z - self.h.astype(dtype)[:, None]).T

    def joint(self, z, matched, dtype=np.float64):
        """the update's pieces without touching the filter (joint_arrays' dict, plus `active`)"""
        act = self.active(matched)
        out = joint_arrays(self.Z.astype(dtype), self.h.astype(dtype), self.X.astype(dtype), self.S.astype(dtype), self.cross_covariance(dtype),
                           np.asarray(z, dtype=dtype), act, self.wi, self.n, self.Na)
        out["active"] = act
        return out

    def update_joint(self, z, matched):
        act = self.active(matched)
        if not act.any():                                   # SLAM.cpp:2050-2051 (and a frame whose matches are all out of view changes nothing)
            return None
        out = self.joint(z, matched)
        self.X = out["X"]
        self._refactor(out["G"])
        self.last_joint = out
        return out

    def run_joint(self, sc, frames=None):
        F = sc["z"].shape[0] if frames is None else frames
        traj = np.zeros((F, 8))
        n = self.n
        for f in range(F):
            self.predict_motion(sc["odo"][f], sc["odo"][f + 1])
            self.predict_measurement()
            self.update_joint(sc["z"][f], sc["matched"][f])
            traj[f, :4] = self.X[n - 4:]
            traj[f, 4:] = (self.S[:, n - 4:n - 2].T @ self.S[:, n - 4:n - 2]).ravel()
        return traj


def make_filter(synth, sc, params=None):
    f = NpJointFilter(sc["N"], params or sc["params"], synth)
    f.set_state(sc["X0"], sc["S0"])
    return f


def displaced_scene(synth, N=8, seed=3, shift=0.1, extra_sigma=0.15):
    """The evidence table's last row: the pose is displaced by `shift` m in x, `extra_sigma` is added to the robot's x / y sigma in quadrature
    (so the filter knows it may be off), the measurements carry no noise.  Returns (scene, X0, S0) with the displaced prior."""
    sc = synth.make_scene(N, 4, seed=seed, meas_sigma=0.0)
    n = 6 * N + 4
    X0, S0 = sc["X0"].copy(), sc["S0"].copy()
    P = S0.T @ S0
    P[n - 4, n - 4] += extra_sigma ** 2
    P[n - 3, n - 3] += extra_sigma ** 2
    S0 = gmw(P, sc["params"]["epsilon"])[0]
    X0[n - 4] += shift
    return sc, X0, S0


def rounding_floor(synth, N, params, frames, seed=3):
    """The restatement's own rounding: the joint update in float64 against numpy.longdouble on the same frame — the frame among the first `frames` of
    make_scene(N, frames, seed) where cond(Pzz) peaks.  Returns (d_X, d_P, cond, frame): max |X64 - Xld|, max |G64 - Gld| over S^T S - U U^T."""
    sc = synth.make_scene(N, frames, seed=seed, p=params)
    f = make_filter(synth, sc, params)
    best = (0.0, 0.0, 0.0, -1)
    for fr in range(frames):
        f.predict_motion(sc["odo"][fr], sc["odo"][fr + 1])
        f.predict_measurement()
        a = f.joint(sc["z"][fr], sc["matched"][fr])
        cond = float(np.linalg.cond(a["Pzz"]))
        if cond > best[2]:
            b = f.joint(sc["z"][fr], sc["matched"][fr], dtype=np.longdouble)
            best = (float(np.abs(a["X"] - b["X"]).max()), float(np.abs(a["G"] - b["G"]).max()), cond, fr)
        f.update_joint(sc["z"][fr], sc["matched"][fr])
    return best


def shipped_tolerance(synth, N, frames):
    """Per-frame bounds for the shipped constants (a1..a4 = 8): the larger of the project's 1e-9 / 1e-11 and 10 x the float64-vs-longdouble floor
    (the factor covers the different summation order of the device's matrix tiles)."""
    dX, dP, _, _ = rounding_floor(synth, N, synth.default_params(), frames)
    return max(1e-9, 10 * dX), max(1e-11, 10 * dP)


def reorder_refactor(G, K, eps, synth):
    """GSLCholeskyUpdate with FLAG_NEED_REORDER (SLAM.cpp:2122-2138, 2158-2179) on G = S^T S - U U^T, K = the landmarks just added: to the disordered layout
    (the rank-deficient new-anchor block last), factor, keep the first r = n - 3 K rows, back to the normal layout, factor again.  Returns P = S^T S."""
    n = G.shape[0]
    perm = synth.permutation(n, K)
    inv = np.argsort(perm)
    Sd = gmw(G[np.ix_(inv, inv)], eps)[0]
    Sd[n - 3 * K:] = 0.0
    Pd = Sd.T @ Sd
    S = gmw(Pd[np.ix_(perm, perm)], eps)[0]
    return S.T @ S
