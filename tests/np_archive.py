"""numpy restatement of the archive search (include/srukf.h: srukf_archive_search; csrc/srukf_archive.hip), stage by stage.

predict: stage (a), the unscented transform over [record 6 | robot 4 | pixel noise 2]; the projection is the CPU oracle's (as in np_ransac.py), everything
         else follows the device's order of operations (scalar fp64, sums in ascending sigma index).
warp:    stage (b), the oracle's wrapPatch into a zeroed template (the device's k_warp_patch equals it byte for byte: tests/test_gpu_parity.py).
search:  stage (c), the gate and the integer correlation; exact integers and one fp64 expression per candidate, so the device must EQUAL it.
chol:    np_loop.chol6's rule for any size."""
import math

import numpy as np

NA = 12
NSIG = 2 * NA + 1
HP = 8
TW = 2 * HP + 1
NP_ = TW * TW
CHI2 = 5.99146454710798


def chol(P, eps=1e-13):
    """Upper S with S^T S = P: d_j = max(eps, P_jj - sum_{m<j} S_mj^2), S_jj = sqrt(d_j), S_ji = (P_ji - sum_{m<j} S_mj S_mi) / S_jj (i > j), sums in ascending m."""
    P = [[float(v) for v in row] for row in np.asarray(P, dtype=np.float64)]
    D = len(P)
    S = [[0.0] * D for _ in range(D)]
    for j in range(D):
        s = 0.0
        for m in range(j):
            s += S[m][j] * S[m][j]
        d = P[j][j] - s
        d = d if d > eps else eps
        sjj = math.sqrt(d)
        S[j][j] = sjj
        for i in range(j + 1, D):
            q = 0.0
            for m in range(j):
                q += S[m][j] * S[m][i]
            S[j][i] = (P[j][i] - q) / sjj
    return np.array(S, dtype=np.float64)


def sigma_points(O, params, x6, s66, pose, P4):
    """The 25 sigma points (rows) of one record: mu, mu + gamma row_i, mu - gamma row_i of S_aug = blockdiag(S66, S_rr, sigma_measure I2)."""
    w = O.sample_parameter(NA, int(params.get("weight_type", 0)), params["ut_alpha"], params["ut_beta"])
    Saug = np.zeros((NA, NA))
    Saug[:6, :6] = np.asarray(s66, dtype=np.float64).reshape(6, 6)
    Saug[6:10, 6:10] = chol(np.asarray(P4, dtype=np.float64).reshape(4, 4), params["epsilon"])
    Saug[10, 10] = Saug[11, 11] = params["sigma_measure"]
    mu = np.concatenate([np.asarray(x6, dtype=np.float64), np.asarray(pose, dtype=np.float64), np.zeros(2)])
    sig = np.empty((NSIG, NA))
    sig[0] = mu + 0.0 * Saug[0]
    for i in range(NA):
        sig[1 + i] = mu + w["gamma"] * Saug[i]
        sig[1 + NA + i] = mu + (-w["gamma"]) * Saug[i]
    return sig, w


def predict(O, params, X6, S66, pose, P4):
    """Stage (a) for L records.  Returns h[L,2], Si[L,2,2], visible[L], xyz[L,3] and Z[L,25,2] (the projected sigma points)."""
    X6 = np.asarray(X6, dtype=np.float64).reshape(-1, 6)
    L = X6.shape[0]
    S66 = np.asarray(S66, dtype=np.float64).reshape(L, 6, 6)
    h, Si, vis, xyz, Zs = np.zeros((L, 2)), np.zeros((L, 2, 2)), np.zeros(L, dtype=np.int32), np.zeros((L, 3)), np.zeros((L, NSIG, 2))
    for k in range(L):
        sig, w = sigma_points(O, params, X6[k], S66[k], pose, P4)
        Z = O.project(params, sig[:, :6], sig[:, 6:9], sig[:, 9], sig[:, 10:12])
        Zs[k] = Z
        sx = sy = p00 = p01 = p11 = 0.0
        for q in range(1, NSIG):
            sx += Z[q, 0]; sy += Z[q, 1]
            dx, dy = Z[q, 0] - Z[0, 0], Z[q, 1] - Z[0, 1]
            p00 += dx * dx; p01 += dx * dy; p11 += dy * dy
        h[k] = [w["wm0"] * Z[0, 0] + w["wi"] * sx, w["wm0"] * Z[0, 1] + w["wi"] * sy]
        Si[k] = chol([[w["wi"] * p00, w["wi"] * p01], [w["wi"] * p01, w["wi"] * p11]], params["epsilon"])
        vis[k] = int(np.all(Z >= 1.0))                            # a zeroed sigma pixel comes out of the distortion a fraction of a pixel from the origin
        xi, yi, zi, th, ph, rho = (float(v) for v in X6[k])
        xyz[k] = [xi + math.cos(ph) * math.sin(th) / rho, yi - math.sin(ph) / rho, zi + math.cos(ph) * math.cos(th) / rho]
    return h, Si, vis, xyz, Zs


def border_margin(params, Z):
    """Smallest distance of any valid (not zeroed) sigma pixel of Z[..., 2] to a validity border of the projection (10 px inside the image, on the undistorted pixel — taken
    here on the distorted one, which lies within a pixel of it for k1 = 1e-4: callers ask for margins of a pixel or more, or of 1e-3 around exact zeros)."""
    Z = np.asarray(Z).reshape(-1, 2)
    ok = np.all(Z >= 1.0, axis=1)
    if not ok.any():
        return np.inf
    W, H = params["image_w"], params["image_h"]
    z = Z[ok]
    return float(np.min([z[:, 0] - 10.0, W - 10.0 - z[:, 0], z[:, 1] - 10.0, H - 10.0 - z[:, 1]]))


def warp(O, params, pose, patches, R, t, px, xyz, h, vis):
    """Stage (b): the 17 x 17 template of every visible record (zeros otherwise), warped into a zeroed buffer."""
    L = len(vis)
    out = np.zeros((L, TW, TW), dtype=np.uint8)
    for k in range(L):
        if vis[k]:
            out[k] = O.warp_patch(params, pose, np.asarray(R[k]).reshape(3, 3), t[k], px[k], xyz[k], h[k], np.asarray(patches[k]).reshape(21, 21),
                                  np.zeros((TW, TW), dtype=np.uint8))
    return out


def corr_int(v, t):
    """The integer form of the normalised cross correlation of two equally sized uint8 arrays."""
    v = np.asarray(v).astype(np.int64).ravel(); t = np.asarray(t).astype(np.int64).ravel()
    n = int(v.size)
    A = n * int((v * t).sum()) - int(v.sum()) * int(t.sum())
    B = n * int((v * v).sum()) - int(v.sum()) ** 2
    C = n * int((t * t).sum()) - int(t.sum()) ** 2
    if B == 0 or C == 0:
        return 0.0
    return float(A) / math.sqrt(float(B) * float(C))


def corr_reference(v, t):
    """calculateCrossCorrelation (SLAM.cpp:3141-3166): means subtracted, dot over the two norms."""
    v = np.asarray(v, dtype=np.float64).ravel(); t = np.asarray(t, dtype=np.float64).ravel()
    a, b = v - v.mean(), t - t.mean()
    s1, s2 = math.sqrt(float(a @ a)), math.sqrt(float(b @ b))
    if s1 == 0.0 or s2 == 0.0:
        return 0.0
    return float(a @ b) / s1 / s2


def window(h, Si, half_cap=40, chi2=CHI2):
    """(half_x, half_y, x0, y0, Pi^-1 entries) of one record, in the device's arithmetic."""
    s00, s01, s10, s11 = (float(v) for v in np.asarray(Si).reshape(4))
    p00 = s00 * s00 + s10 * s10; p01 = s00 * s01 + s10 * s11; p10 = s01 * s00 + s11 * s10; p11 = s01 * s01 + s11 * s11
    det = p00 * p11 - p01 * p10
    i00 = i01 = i10 = i11 = 0.0
    if det != 0.0:
        det = 1.0 / det
        i00, i01, i10, i11 = p11 * det, -p01 * det, -p10 * det, p00 * det
    cap = float(min(max(int(half_cap), HP), 40))
    hx = int(min(max(math.ceil(math.sqrt(chi2 * p00)), float(HP)), cap))
    hy = int(min(max(math.ceil(math.sqrt(chi2 * p11)), float(HP)), cap))
    return hx, hy, int(h[0]) - hx, int(h[1]) - hy, (i00, i01, i10, i11)


def scores(img, h, Si, tmpl, half_cap=40, chi2=CHI2):
    """The wy x wx score map of one visible record (0 where a candidate is skipped) and its window (x0, y0)."""
    img = np.asarray(img)
    H, W = img.shape
    px, py = float(h[0]), float(h[1])
    hx, hy, x0, y0, (i00, i01, i10, i11) = window(h, Si, half_cap, chi2)
    wx, wy = 2 * hx + 1, 2 * hy + 1
    I = (x0 + np.arange(wx))[None, :] + np.zeros((wy, 1), dtype=np.int64)
    J = (y0 + np.arange(wy))[:, None] + np.zeros((1, wx), dtype=np.int64)
    inside = (I >= HP) & (I <= W - HP - 1) & (J >= HP) & (J <= H - HP - 1)
    ex, ey = I - px, J - py
    pii = (ex * i00 + ey * i10) * ex + (ex * i01 + ey * i11) * ey
    live = inside & (pii < chi2)
    reg = np.zeros((wy + 2 * HP, wx + 2 * HP), dtype=np.int64)                    # pixels outside the image as 0 (never under a live candidate)
    ys, xs = np.arange(y0 - HP, y0 + wy + HP), np.arange(x0 - HP, x0 + wx + HP)
    yv, xv = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    reg[np.ix_(yv, xv)] = img[np.ix_(ys[yv], xs[xv])]
    win = np.lib.stride_tricks.sliding_window_view(reg, (TW, TW))                # [wy, wx, 17, 17]
    t = np.asarray(tmpl).astype(np.int64).reshape(TW, TW)
    sv = win.sum(axis=(2, 3)); svv = (win * win).sum(axis=(2, 3)); svt = (win * t).sum(axis=(2, 3))
    St, Stt = int(t.sum()), int((t * t).sum())
    A = NP_ * svt - sv * St
    B = NP_ * svv - sv * sv
    C = NP_ * Stt - St * St
    cc = np.zeros((wy, wx))
    good = live & (B != 0) & (C != 0)
    cc[good] = A[good].astype(np.float64) / np.sqrt(B[good].astype(np.float64) * float(C))
    return cc, x0, y0


def search(params, img, h, Si, vis, tmpl, half_cap=40, corr_threshold=0.8, chi2=CHI2):
    """Stage (c) for L records: z[L,2], matched[L], corr[L]."""
    L = len(vis)
    z, m, cr = np.zeros((L, 2)), np.zeros(L, dtype=np.int32), np.zeros(L)
    for k in range(L):
        if not vis[k]:
            continue
        cc, x0, y0 = scores(img, h[k], Si[k], tmpl[k], half_cap, chi2)
        c = int(np.argmax(cc))                                                   # the first maximum in row-major order
        cr[k] = cc.flat[c]
        if cr[k] > corr_threshold:
            m[k] = 1
            z[k] = [x0 + c % cc.shape[1], y0 + c // cc.shape[1]]
    return z, m, cr


def make_records(O, params, X4, S4, uv, img):
    """Records of landmarks first seen at the pixels uv[K,2] of `img` from the robot state (X4, S4), without a device: the oracle's joint initialisation
    (integrateFeaturesInformation), chol of each marginal 6 x 6 block, the 21 x 21 init patch at round(uv), Rwc of the heading, the robot position."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    K = uv.shape[0]
    Xn, Sn = O.joint_init(params, np.asarray(X4, dtype=np.float64), np.asarray(S4, dtype=np.float64), uv)
    P = Sn.T @ Sn
    c, s = math.cos(X4[3]), math.sin(X4[3])
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    rec = {"X6": np.zeros((K, 6)), "S66": np.zeros((K, 6, 6)), "patch": np.zeros((K, 21, 21), dtype=np.uint8), "R": np.tile(R, (K, 1, 1)),
           "t": np.tile(np.asarray(X4[:3], dtype=np.float64), (K, 1)), "px": uv.copy()}
    for k in range(K):
        rec["X6"][k] = Xn[6 * k:6 * k + 6]
        rec["S66"][k] = chol(P[6 * k:6 * k + 6, 6 * k:6 * k + 6], params["epsilon"])
        u, v = int(np.rint(uv[k, 0])), int(np.rint(uv[k, 1]))
        rec["patch"][k] = np.asarray(img)[v - 10:v + 11, u - 10:u + 11]
    return rec
