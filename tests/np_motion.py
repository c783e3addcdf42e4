"""The motion step in numpy longdouble: a reference for predictMotion's numeric tail that shares neither the reference's formulation (a Householder QR of
the 2Na x n deviation matrix) nor the device's (R11 untouched, R12 from the +/- differences, R22 from a 4x4 Gram Cholesky).

motion_step(X, S, odo_prev, odo_cur, params) restates SLAM.cpp:1444-1458 (the control), 1148-1162 (the sigma points, robot and control-noise rows only),
1476-1532 (the odometry model and the weighted mean) and the covariance that the QR at 1539-1555 stands for:

    P = wi sum_c (sigma_c - sigma_0)(sigma_c - sigma_0)^T        about sigma_0, weight wi, no centre term

of which only the last four columns change.  With sigma_c[:n-4] - sigma_0[:n-4] = +-gamma S[i, :n-4] they are
    P12 = wi gamma S11^T (r+ - r-)         ((n-4) x 4)
    P22 = wi sum_c (r_c - r_0)(r_c - r_0)^T   (4 x 4)
from the robot part r_c of the L = 2 Na + 1 sigma points alone: O(n Na) work, the n x L matrix is never formed.

The control (Ut, Mt) is formed in DOUBLE, operation for operation as srukf_motion_control_a and the oracle write it, so its quirks are shared and not
repaired: atan2(0, 0) - theta at a standstill, no angle wrap (a heading that crosses +-pi yields a 2 pi rot2 and its noise), Mt used as the square-root
row of the augmented factor although it is a variance.  Everything behind the control is longdouble (64-bit significand), weights included as the doubles
calculateSampleParameter produces.

Every returned quantity comes with a ROUNDING BOUND for a double-precision evaluation, built from this module's own numbers only (u = 2^-53):
    each sum                 u L sum |terms|     (any summation order of L terms; the Gram / QR form of the covariance included, n < L)
    each deviation r - s0    the cancellation term: the operands carry their own errors at magnitude |r|, the difference does not shrink them
    each sigma point         the rounding of the pose arithmetic at the magnitude of its operands, a few ulp of the control, and 2 ulp of the sin / cos
                             argument (at the magnitude of the argument's operands) times the translation
The bounds are worst-case, so a correct evaluation sits well inside them; tests/test_motion_cpu.py shows that they still tell five wrong restatements from
rounding by a factor of 100 and more."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

MUTANTS = ("sin_for_cos", "rot2_noise_sign", "minus_point_dropped", "wc0_in_mean", "mt_squared")


def weights(Na, p):
    """calculateSampleParameter (SLAM.cpp:1050-1103) in double: wm0, wc0, wi, wi_sr, gamma"""
    wt = int(p.get("weight_type", 0))
    if wt == 0:
        wm0 = 1.0 - Na / 3.0
        wc0 = 1.0 - Na / 3.0
        wi = (1.0 - wc0) / (2 * Na)
        gamma = float(np.sqrt(Na / (1.0 - wm0)))
    elif wt == 1:
        a2 = p["ut_alpha"] * p["ut_alpha"]
        lam = a2 * (Na + 0.0) - Na
        gamma = float(np.sqrt(Na + lam))
        wm0 = lam / (Na + lam)
        wc0 = wm0 + (1 - a2 + p["ut_beta"])
        wi = 1.0 / (2 * (Na + lam))
    else:
        gamma = float(np.sqrt(3.0 * Na / 2.0))
        wm0 = wc0 = 1.0 / 3.0
        wi = 1.0 / (3.0 * Na)
    return wm0, wc0, wi, float(np.sqrt(abs(wi))), gamma


def control(odo_prev, odo_cur, p):
    """(Ut, Mt) in double, SLAM.cpp:1446-1458 as srukf_motion_control_a writes it (Python floats: one rounding per operation, left to right)."""
    o0, o1 = [float(v) for v in odo_prev], [float(v) for v in odo_cur]
    dx = o1[0] - o0[0]
    dy = o1[1] - o0[1]
    rot1 = float(np.arctan2(dy, dx)) - o0[2]
    trans = float(np.sqrt(dy * dy + dx * dx))
    rot2 = o1[2] - o0[2] - rot1
    a1, a2, a3, a4 = p["a1"], p["a2"], p["a3"], p["a4"]
    Mt = (a1 * rot1 * rot1 + a2 * trans * trans,
          a3 * trans * trans + a4 * rot1 * rot1 + a4 * rot2 * rot2,
          a1 * rot2 * rot2 + a2 * trans * trans)
    return np.array([rot1, trans, rot2]), np.array(Mt)


def motion_step(X, S, odo_prev, odo_cur, p, mutant=None):
    """-> dict: Ut, Mt (double); sigma ((L, 4) longdouble: centre, the Na plus points, the Na minus points) with sigma_bound, and trig ((L, 2): cos and sin of
    every point's new heading, which the device keeps beside the pose) with trig_bound; mean (4), P12 ((n-4, 4)), P22 ((4, 4)) rounded to
    double; mean_bound, P12_bound, P22_bound, P11_bound (for a double evaluation that forms sigma_c[:n-4] - sigma_0[:n-4] by subtraction, as the reference does)."""
    assert mutant is None or mutant in MUTANTS, mutant
    X = np.asarray(X, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    n = X.shape[0]
    Na, L = n + 5, 2 * (n + 5) + 1
    wm0, wc0, wi, wi_sr, gamma = weights(Na, p)
    Ut, Mt = control(odo_prev, odo_cur, p)
    rot1, trans, rot2 = [LD(v) for v in Ut]
    mrow = Mt * Mt if mutant == "mt_squared" else Mt

    # robot and control-noise part of the Na rows of blockdiag(S, Mt, Qt)
    srow = np.zeros((Na, 4), dtype=LD)
    srow[:n] = S[:, n - 4:]
    q = np.zeros((Na, 3), dtype=LD)
    q[n + np.arange(3), np.arange(3)] = mrow
    xr = X[n - 4:].astype(LD)
    g = LD(gamma)
    sg = np.concatenate([np.zeros(1, dtype=LD), np.full(Na, g), np.full(Na, -g)])[:, None]      # (L, 1)
    rows = np.concatenate([np.zeros((1, 4), dtype=LD), srow, srow])
    qs = np.concatenate([np.zeros((1, 3), dtype=LD), q, q]) * sg
    pt = xr[None, :] + rows * sg                                                                 # generateSigmaPoints, robot rows
    r1 = rot1 - qs[:, 0]
    tr = trans - qs[:, 1]
    r2 = rot2 + qs[:, 2] if mutant == "rot2_noise_sign" else rot2 - qs[:, 2]
    th = pt[:, 3]
    arg = th + r1
    cx, cy = (np.sin, np.cos) if mutant == "sin_for_cos" else (np.cos, np.sin)
    sig = np.stack([pt[:, 0] + tr * cx(arg), pt[:, 1] + tr * cy(arg), pt[:, 2], th + (r1 + r2)], axis=1)      # 1518-1523
    wts = np.full(L, LD(wi))
    wts[0] = LD(wc0) if mutant == "wc0_in_mean" else LD(wm0)       # (weight types 0 and 2 have wc0 == wm0: this mutant shows under weight type 1 only)
    live = np.ones(L, dtype=bool)
    if mutant == "minus_point_dropped":
        live[1 + Na + (n - 1)] = False                          # the minus point of the heading's own direction
    mean = (wts[live, None] * sig[live]).sum(axis=0)

    dev = sig - sig[:1]
    dev[~live] = 0
    P22 = LD(wi) * (dev.T @ dev)
    D = dev[1:1 + n - 4] - dev[1 + Na:1 + Na + n - 4]                                            # r+ - r-, the landmark directions
    S11 = S[:n - 4, :n - 4]
    P12 = LD(wi) * g * (S11.T.astype(LD) @ D)

    # ---- rounding bounds (double arithmetic is enough for a bound) -------------------------------------------------------------------------------------------
    f = lambda a: np.abs(np.asarray(a, dtype=np.float64))
    a_sig, a_rows, a_qs = f(sig), f(rows * sg), f(qs)
    m_r1 = abs(float(Ut[0])) + a_qs[:, 0] + abs(float(odo_prev[2]))      # rot1 = atan2 - theta_prev is rounded at the magnitude of theta_prev
    m_tr = abs(float(Ut[1])) + a_qs[:, 1]
    m_r2 = abs(float(Ut[2])) + a_qs[:, 2] + m_r1 + abs(float(odo_cur[2]))
    m_th = abs(float(xr[3])) + a_rows[:, 3]
    e_arg = 2 * 2.0 ** -52 * (m_th + m_r1) + 4 * U * m_r1               # 2 ulp of the argument's operands + the control's own ulps
    e_tr = 4 * U * m_tr
    delta = np.empty((L, 4))                                             # error bound of one sigma point evaluated in double
    for e in (0, 1):
        delta[:, e] = 3 * U * (abs(float(xr[e])) + a_rows[:, e] + a_sig[:, e]) + m_tr * (e_arg + 4 * U) + e_tr
    delta[:, 2] = 2 * U * (abs(float(xr[2])) + a_rows[:, 2])
    delta[:, 3] = 4 * U * (m_th + m_r1 + m_r2)
    aw = f(wts)
    mean_bound = U * L * (aw[:, None] * a_sig).sum(axis=0) + (aw[:, None] * delta).sum(axis=0)
    a_dev = f(dev)
    eps = delta + delta[:1] + U * (a_sig + a_sig[:1])                    # error bound of one deviation r_c - s0
    eps[0] = 0
    P22_bound = wi * (U * L * (a_dev.T @ a_dev) + a_dev.T @ eps + eps.T @ a_dev + eps.T @ eps)
    A11 = np.abs(S11)
    a_D = f(D)
    e_D = eps[1:1 + n - 4] + eps[1 + Na:1 + Na + n - 4]
    a_dd = a_dev[1:1 + n - 4] + a_dev[1 + Na:1 + Na + n - 4]
    K = U * ((A11 > 0) * np.abs(X[None, :n - 4]) + gamma * A11)          # the reference forms sigma_c[j] - sigma_0[j] = (X_j + gamma S_ij) - X_j by subtraction
    P12_bound = wi * gamma * (U * L * (A11.T @ a_D) + A11.T @ e_D) + wi * (K.T @ a_dd)
    P11_bound = U * 2 * L * (A11.T @ A11) + 2 * wi * gamma * (K.T @ A11 + A11.T @ K)
    return dict(Ut=Ut, Mt=Mt, weights=(wm0, wc0, wi, wi_sr, gamma), sigma=sig,
                mean=mean.astype(np.float64), P12=P12.astype(np.float64), P22=P22.astype(np.float64),
                mean_ld=mean, P12_ld=P12, P22_ld=P22,
                sigma_bound=delta, trig=np.stack([np.cos(sig[:, 3]), np.sin(sig[:, 3])], axis=1).astype(np.float64), trig_bound=delta[:, 3] + 6 * U,
                mean_bound=mean_bound, P12_bound=P12_bound, P22_bound=P22_bound, P11_bound=P11_bound)


def robot_columns_of_P(S):
    """(P12, P22) of P = S^T S from a double factor, accumulated in longdouble: the comparison then measures the factor, not this product."""
    S = np.asarray(S, dtype=np.float64)
    n = S.shape[0]
    cols = S.T.astype(LD) @ S[:, n - 4:].astype(LD)
    return cols[:n - 4].astype(np.float64), cols[n - 4:].astype(np.float64)


def ratios(ref, mean, P12, P22, sigma=None):
    """measured / bound, the largest per quantity (0 / 0 counts as 0, x / 0 as inf): {"X": .., "P12": .., "P22": ..} and, given the (L, 4) robot part of the sigma
    points, "sigma" (two evaluations that swap or move a point differ there even where the mean and the covariance cannot tell)"""
    def worst(d, b):
        d, b = np.abs(np.asarray(d, dtype=np.float64)), np.asarray(b, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d == 0, 0.0, d / b)
        return float(r.max()) if r.size else 0.0
    more = {} if sigma is None else {"sigma": worst(np.asarray(sigma, dtype=LD) - ref["sigma"], ref["sigma_bound"])}
    return {**more, "X": worst(mean - ref["mean"], ref["mean_bound"]), "P12": worst(P12 - ref["P12"], ref["P12_bound"]), "P22": worst(P22 - ref["P22"], ref["P22_bound"])}
