"""The three kernels of csrc/srukf_overlay.hip restated in numpy, bit for bit: k_bgr2gray's integer gray formula, k_overlay_prep's per-landmark record on Python
floats (IEEE fp64, one rounding per operation, math.sqrt correctly rounded) in the kernel's operation order, and k_overlay's raster rule vectorised over the
pixels with the same paint order (landmarks in index order, later over earlier; predicted cross, matched cross, ellipse).  include/srukf.h states the rules."""
import math

import numpy as np

CHI2 = 5.99146454710798                                          # CHI2INV_TABLE(0, 2)
CROSS = 10
BLUE = (255, 0, 0)                                               # B, G, R of CV_RGB(0, 0, 255): the predicted cross
RED = (0, 0, 255)                                                # CV_RGB(255, 0, 0): the matched cross and the ellipse
LIMIT = 2.0 ** 30


def gray(bgr):
    """(..., 3) uint8 in memory order c0, c1, c2 -> uint8: (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14"""
    c = np.asarray(bgr).astype(np.int64)
    return ((4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def eigen2(p00, p01, p11):
    """Closed-form eigen-pair of the symmetric [[p00, p01], [p01, p11]]: (l0, l1, c, s), l0 >= l1 (l1 clamped at 0), (c, s) the unit eigenvector of l0."""
    t = 0.5 * (p00 + p11)
    d = 0.5 * (p00 - p11)
    r = math.sqrt(d * d + p01 * p01)
    l0 = t + r
    l1 = t - r
    l1 = l1 if l1 > 0.0 else 0.0                                 # max(t - r, 0); only read when l0 is finite
    if not (l0 < 1e12):
        return l0, l1, 1.0, 0.0
    if r == 0.0:
        return l0, l1, 1.0, 0.0
    if d >= 0.0:
        vx, vy = d + r, p01
    else:
        vx, vy = p01, r - d
    m = max(abs(vx), abs(vy))                                    # scaled first: the squares neither overflow nor underflow
    ux, uy = vx / m, vy / m
    n = math.sqrt(ux * ux + uy * uy)
    return l0, l1, ux / n, uy / n


def prep(h, Si, z, matched):
    """One record per landmark: dict(drawn, ellipse, px, py, mx, my, a, b, c, s)."""
    h, Si, z = np.asarray(h, dtype=np.float64).reshape(-1, 2), np.asarray(Si, dtype=np.float64).reshape(-1, 4), np.asarray(z, dtype=np.float64).reshape(-1, 2)
    matched = np.asarray(matched).reshape(-1)
    recs = []
    for k in range(len(matched)):
        r = dict(drawn=False, ellipse=False, px=0, py=0, mx=0, my=0, a=1, b=1, c=1.0, s=0.0)
        v = [float(h[k, 0]), float(h[k, 1]), float(z[k, 0]), float(z[k, 1])]
        if matched[k] != 0 and all(abs(q) < LIMIT for q in v):   # (a NaN or an infinity fails the comparison)
            r["drawn"] = True
            r["px"], r["py"], r["mx"], r["my"] = (int(np.rint(q)) for q in v)      # to nearest, ties to even
            s00, s01, s10, s11 = (float(q) for q in Si[k])
            p00 = s00 * s00 + s10 * s10
            p01 = s00 * s01 + s10 * s11
            p11 = s01 * s01 + s11 * s11
            l0, l1, c, s = eigen2(p00, p01, p11)
            if l0 < 1e12:
                chi = math.sqrt(CHI2)
                r["ellipse"] = True
                r["a"] = max(1, int(math.sqrt(l0) * chi))
                r["b"] = max(1, int(math.sqrt(l1) * chi))
                r["c"], r["s"] = c, s
        recs.append(r)
    return recs


def cross_mask(X, Y, cx, cy):
    dx, dy = np.abs(X - cx), np.abs(Y - cy)
    return ((dx <= CROSS) & (dy <= 1)) | ((dy <= CROSS) & (dx <= 1))


def ellipse_mask(X, Y, r):
    dx, dy = (X - r["mx"]).astype(np.float64), (Y - r["my"]).astype(np.float64)
    c, s, a, b = r["c"], r["s"], r["a"], r["b"]
    p = c * dx + s * dy
    q = c * dy - s * dx

    def inside(A, B):
        u, v = p / float(A), q / float(B)
        return u * u + v * v <= 1.0

    with np.errstate(invalid="ignore"):
        m = inside(a + 1, b + 1)
        if a >= 2 and b >= 2:
            m &= ~inside(a - 1, b - 1)
    return m


def render(src, h, Si, z, matched):
    """src: (H, W, 3) uint8 colour frame or (H, W) uint8 gray frame -> (H, W, 3) uint8"""
    src = np.asarray(src, dtype=np.uint8)
    out = np.repeat(src[:, :, None], 3, axis=2).copy() if src.ndim == 2 else src.copy()
    H, W = out.shape[:2]
    Y, X = np.mgrid[0:H, 0:W].astype(np.int64)
    for r in prep(h, Si, z, matched):
        if not r["drawn"]:
            continue
        out[cross_mask(X, Y, r["px"], r["py"])] = BLUE
        out[cross_mask(X, Y, r["mx"], r["my"])] = RED
        if r["ellipse"]:
            out[ellipse_mask(X, Y, r)] = RED
    return out
