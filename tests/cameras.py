"""Cameras for the camera-model tests, and two restatements of the projection that those tests compare against.

CAMERAS      named parameter sets: synth.scene_params() with overrides that make every term of the model count (k2 != 0, f1 != f2, dx != dy, image_w != the
             default, odd and small Newton iteration counts).
tail()       srukf_project (srukf_device.h) from the distortOnePointRW comment to the end, operation for operation with the device's placement of every fused
             multiply-add, in plain Python floats: what the device must give BIT FOR BIT once (ux, uy) are known.
exact_*()    inputs for which the front of srukf_project is exact, so that (ux, uy) ARE known: feat = (0,0,0,0,0,1), pos = (0,0,-1), psi = 0 give
             sincos(0) = (0, 1), rx = ry = 0, rz = 2, hence uy = fl(cam_cx + e0), ux = fl(cam_cy + e1); the border test is a plain IEEE comparison.
mp_project() the whole projection in mpmath at 40 digits with the distortion equation solved to convergence: the high-precision reference.
"""
import functools

import numpy as np

OVERRIDES = {
    "default": {},
    "k2_strong": dict(cam_k1=0.12, cam_k2=0.035),
    "barrel_neg": dict(cam_k1=-0.06, cam_k2=0.01),
    "nonsquare": dict(cam_dx=0.0031, cam_dy=0.0024, cam_cx=287.4, cam_cy=251.9, cam_k1=0.05, cam_k2=0.02),
    "odd_iters": dict(cam_k1=0.12, cam_k2=0.035, newton_iters=99),
    "few_iters": dict(cam_k1=0.12, cam_k2=0.035, newton_iters=3),
    "small_img": dict(image_w=480, image_h=400, cam_cx=231.7, cam_cy=188.2, cam_k1=0.08, cam_k2=0.02),
}
NAMES = list(OVERRIDES)
CONVERGED = [c for c in NAMES if c != "few_iters"]        # the cameras whose Newton iteration runs to convergence
NEWTON_KS = (0, 1, 2, 3, 7, 99, 100, 101)
SCENES = ((8, 80.0), (40, 150.0))                          # (N, disc_radius) of the frame tests; make_scene(N, 6, seed=11, disc_radius=...)
SCENE_SEED, SCENE_FRAMES = 11, 6


def camera(synth, name, **more):
    p = synth.scene_params()
    p.update(OVERRIDES[name])
    p.update(more)
    return p


def scene(synth, name, N, disc_radius):
    return synth.make_scene(N, SCENE_FRAMES, seed=SCENE_SEED, p=camera(synth, name), disc_radius=disc_radius)


# ---- the bit-exact restatement ---------------------------------------------------------------------------------------------------------------------------

def fma(a, b, c):
    """a * b + c rounded once.  Python 3.10 has no math.fma; a double is an integer over a power of two, and int / int is correctly rounded, so this is
    float(Fraction(a) * Fraction(b) + Fraction(c)) without the gcd work (test_camera_cpu.py holds the two to each other)."""
    na, da = a.as_integer_ratio(); nb, db = b.as_integer_ratio(); nc, dc = c.as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def _front(p, ux, uy):
    """distortOnePointRW up to the start value of the iteration: (xu, yu, ru, rd0)"""
    k1, k2 = p["cam_k1"], p["cam_k2"]
    xu = (ux - p["cam_cx"]) * p["cam_dx"]
    yu = (uy - p["cam_cy"]) * p["cam_dy"]
    ru = float(np.sqrt(fma(xu, xu, yu * yu)))              # (IEEE sqrt: correctly rounded on both sides)
    ru2 = ru * ru
    rd = ru / fma(k2 * ru2, ru2, fma(k1, ru2, 1.0))
    return xu, yu, ru, rd


def _newton(p, rd, ru):
    k1, k2 = p["cam_k1"], p["cam_k2"]
    k1_3, k2_5 = 3.0 * k1, 5.0 * k2
    rd2 = rd * rd
    f = fma(k2 * rd2 * rd2, rd, fma(k1 * rd2, rd, rd)) - ru
    ff = fma(k2_5 * rd2, rd2, fma(k1_3, rd2, 1.0))
    return rd - f / ff


def _back(p, xu, yu, rd):
    k1, k2 = p["cam_k1"], p["cam_k2"]
    d = fma(k2 * rd * rd * rd, rd, fma(k1 * rd, rd, 1.0))
    if d == 0.0: d = p["epsilon"]
    vx = p["cam_cx"] + (xu / d) / p["cam_dx"]
    vy = p["cam_cy"] + (yu / d) / p["cam_dy"]
    vis = (vx >= 0.0) and (vx <= p["image_w"]) and (vy >= 0.0) and (vy <= p["image_h"])
    return (vx, vy) if vis else (0.0, 0.0)


def tail(p, ux, uy, K, shortcut, want_iters=False):
    """srukf_project from `// distortOnePointRW` to the end with newton_iters = K.  shortcut: with the device's two early exits (fixed point; 2-cycle between
    two doubles, resolved by the parity of the iterations left); without: all K iterations, as the reference runs them."""
    ux, uy = float(ux), float(uy)
    xu, yu, ru, rd = _front(p, ux, uy)
    rprev = float("nan")
    done = 0
    for it in range(K):
        rn = _newton(p, rd, ru)
        done = it + 1
        if shortcut:
            if rn == rd: break
            if rn == rprev:
                if (K - it) & 1: rd = rn
                break
        rprev = rd
        rd = rn
    out = _back(p, xu, yu, rd)
    return out + (done,) if want_iters else out


def tail_full(p, ux, uy, Ks=NEWTON_KS):
    """{K: tail(p, ux, uy, K, shortcut=False)} for several K from ONE run of the full loop (its iterates after K steps are a prefix of the longer runs)."""
    ux, uy = float(ux), float(uy)
    xu, yu, ru, rd = _front(p, ux, uy)
    out = {}
    for it in range(max(Ks) + 1):
        if it in Ks: out[it] = _back(p, xu, yu, rd)
        rd = _newton(p, rd, ru)
    return out


def _cam_key(p):
    return tuple(p[k] for k in ("cam_dx", "cam_dy", "cam_cx", "cam_cy", "cam_k1", "cam_k2", "image_w", "image_h", "epsilon"))


@functools.lru_cache(maxsize=None)
def _tail_full_table(key, pix):
    p = dict(zip(("cam_dx", "cam_dy", "cam_cx", "cam_cy", "cam_k1", "cam_k2", "image_w", "image_h", "epsilon"), key))
    rows = [tail_full(p, ux, uy) for ux, uy in pix]
    return {K: np.array([r[K] for r in rows]) for K in NEWTON_KS}


def tail_full_table(p, ux, uy):
    """{K: out[n, 2]} of tail(shortcut=False) over pixel arrays; shared between the cameras that differ in newton_iters only and between the tests."""
    return _tail_full_table(_cam_key(p), tuple(zip(map(float, ux), map(float, uy))))


# ---- inputs that make the front of srukf_project exact ---------------------------------------------------------------------------------------------------

def exact_inputs(err):
    """(feat6, pos3, psi) for err[n, 2]: hx = hy = 0, hz = 2, det = 1 -> rx = ry = 0, rz = 2, and f * 0 / 2 = 0 is added to cam_cx / cam_cy exactly"""
    n = len(err)
    return np.tile([0.0, 0.0, 0.0, 0.0, 0.0, 1.0], (n, 1)), np.tile([0.0, 0.0, -1.0], (n, 1)), np.zeros(n)


def exact_seen(p, err):
    """The (ux, uy) the device must hold after coordinatesCamera2Image for exact_inputs(err): uy = fl(cam_cx + e0), ux = fl(cam_cy + e1) (the reference's x/y
    swap), both zeroed outside [10, image_w - 10] x [10, image_h - 10].  Returns (ux, uy, zeroed)."""
    err = np.asarray(err, dtype=np.float64)
    uy = p["cam_cx"] + err[:, 0]
    ux = p["cam_cy"] + err[:, 1]
    bad = (ux < 10.0) | (ux > p["image_w"] - 10.0) | (uy < 10.0) | (uy > p["image_h"] - 10.0)
    return np.where(bad, 0.0, ux), np.where(bad, 0.0, uy), bad


def _err_for(c, target):
    """e with fl(c + e) == target, then the nearest e on either side at which fl(c + e) moves: [(e, fl(c + e))] for at, below, above.  c + e moves in steps of
    the coarser of the two ulps, so next to a small target (10) the values on either side are the nearest the sum can take, not always the adjacent doubles."""
    e = target - c
    for _ in range(8):
        if c + e == target: break
        e = np.nextafter(e, np.inf if c + e < target else -np.inf)
    assert c + e == target, (c, target)
    out = [(e, c + e)]
    for way in (-np.inf, np.inf):
        x = e
        for _ in range(64):
            x = np.nextafter(x, way)
            if c + x != target: break
        assert c + x != target
        out.append((float(x), c + float(x)))
    return out


def border_errs(p):
    """err rows whose computed ux or uy is exactly 10, image_w - 10 / image_h - 10, or the nearest value on either side; the other coordinate mid-image."""
    rows = []
    mid0, mid1 = p["image_h"] / 2 - p["cam_cx"], p["image_w"] / 2 - p["cam_cy"]
    for t in (10.0, p["image_w"] - 10.0):                   # ux = fl(cam_cy + e1) against image_w
        rows += [(mid0, e) for e, _ in _err_for(p["cam_cy"], t)]
    for t in (10.0, p["image_h"] - 10.0):                   # uy = fl(cam_cx + e0) against image_h
        rows += [(e, mid1) for e, _ in _err_for(p["cam_cx"], t)]
    return np.array(rows)


def exact_errs(p, n, seed, border=True):
    """n err rows: the border rows, then seeded pixels spread over the whole admissible rectangle (a few outside it)."""
    rng = np.random.default_rng(seed)
    b = border_errs(p) if border else np.zeros((0, 2))
    m = n - len(b)
    uy = rng.uniform(4.0, p["image_h"] - 4.0, m)            # 6 px of margin outside the admissible rectangle: zeroed
    ux = rng.uniform(4.0, p["image_w"] - 4.0, m)
    return np.vstack([b, np.column_stack([uy - p["cam_cx"], ux - p["cam_cy"]])])


def admissible_pixels(p, n, seed):
    """n seeded (ux, uy) inside [10, image_w - 10] x [10, image_h - 10]"""
    rng = np.random.default_rng(seed)
    return rng.uniform(10.0, p["image_w"] - 10.0, n), rng.uniform(10.0, p["image_h"] - 10.0, n)


# ---- general points and the high-precision reference -----------------------------------------------------------------------------------------------------

def general_points(synth, p, n, seed, radius=200.0):
    """(feat, pos, psi, err) drawn as test_projection_matches_oracle_and_golden draws them (true landmarks of a scene on a 3 m ceiling + N(0, 1e-3), robot
    N(0, 0.05), heading N(0, 0.5), pixel error N(0, 3)) with the landmarks spread to `radius` px from the principal point.  (make_scene's own draw of the
    truth, without its joint initialisation: that is a QR of order 6 n.)"""
    rng = np.random.default_rng(seed)
    r = radius * np.sqrt(rng.uniform(0, 1, n))
    a = rng.uniform(0, 2 * np.pi, n)
    uv = np.column_stack([p["cam_cy"] + r * np.cos(a), p["cam_cx"] + r * np.sin(a)])
    th, ph = synth.pixel_to_angles(uv, 0.0, p)
    truth = np.column_stack([np.zeros((n, 3)), th, ph, np.cos(ph) * np.cos(th) / 3.0])
    feat = truth + rng.normal(0, 1e-3, truth.shape)
    return feat, rng.normal(0, 0.05, (n, 3)), rng.normal(0, 0.5, n), rng.normal(0, 3, (n, 2))


def raw_pixels(p, feat, pos, psi, err):
    """Un-thresholded (ux, uy, vx, vy) in numpy doubles: ux, uy before the border test, vx, vy (from the thresholded ux, uy, as the model goes on) before the
    view test.  For telling which points sit next to a threshold; 1e-6 px is far above its rounding."""
    xi, yi, zi, th, ph, rho = [feat[:, i] for i in range(6)]
    hx = xi + 1 / rho * np.cos(ph) * np.sin(th) - pos[:, 0]
    hy = yi - 1 / rho * np.sin(ph) - pos[:, 1]
    hz = zi + 1 / rho * np.cos(ph) * np.cos(th) - pos[:, 2]
    c, s = np.cos(psi), np.sin(psi)
    rx, ry = c * hx + s * hy, -s * hx + c * hy
    f1, f2 = p["cam_f"] / p["cam_dx"], p["cam_f"] / p["cam_dy"]
    uy = p["cam_cx"] + f1 * rx / hz + err[:, 0]
    ux = p["cam_cy"] + f2 * ry / hz + err[:, 1]
    bad = (ux < 10) | (ux > p["image_w"] - 10) | (uy < 10) | (uy > p["image_h"] - 10)
    k1, k2 = p["cam_k1"], p["cam_k2"]
    xu = (np.where(bad, 0.0, ux) - p["cam_cx"]) * p["cam_dx"]
    yu = (np.where(bad, 0.0, uy) - p["cam_cy"]) * p["cam_dy"]
    ru = np.sqrt(xu * xu + yu * yu)
    rd = ru / (1 + k1 * ru * ru + k2 * ru ** 4)
    for _ in range(p["newton_iters"]):
        rd = rd - (rd + k1 * rd ** 3 + k2 * rd ** 5 - ru) / (1.0 + 3.0 * k1 * rd * rd + 5.0 * k2 * rd ** 4)
    d = 1 + k1 * rd * rd + k2 * rd ** 4
    return ux, uy, p["cam_cx"] + (xu / d) / p["cam_dx"], p["cam_cy"] + (yu / d) / p["cam_dy"]


def near_threshold(p, feat, pos, psi, err, margin=1e-6):
    """bool[n]: the point's un-thresholded ux, uy, vx or vy lies within `margin` px of 10, image_w - 10, image_h - 10, 0, image_w or image_h"""
    vals = np.stack(raw_pixels(p, feat, pos, psi, err))
    lines = np.array([10.0, p["image_w"] - 10.0, p["image_h"] - 10.0, 0.0, p["image_w"], p["image_h"]])
    return (np.abs(vals[:, :, None] - lines[None, None, :]) <= margin).any(axis=(0, 2))


def branches(p, feat, pos, psi, err):
    """(border[n], out_of_view[n]): which zeroing branch of the model each point takes (numpy doubles)"""
    ux, uy, vx, vy = raw_pixels(p, feat, pos, psi, err)
    border = (ux < 10) | (ux > p["image_w"] - 10) | (uy < 10) | (uy > p["image_h"] - 10)
    oov = ~((vx >= 0) & (vx <= p["image_w"]) & (vy >= 0) & (vy <= p["image_h"]))
    return border, oov


def mp_project(p, feat, pos, psi, err, steps=None):
    """The projection in mpmath at 40 digits -> out[n, 2] (rounded to double at the very end).  steps None: rd + k1 rd^3 + k2 rd^5 = ru solved by Newton from
    the model's start value until the step is below 1e-36; steps = K: exactly K Newton steps (the few-iterations cameras)."""
    import mpmath
    mp = mpmath.mp.clone(); mp.dps = 40
    m = lambda v: mp.mpf(float(v))
    P = {k: m(p[k]) for k in ("cam_k1", "cam_k2", "cam_cx", "cam_cy", "cam_dx", "cam_dy", "cam_f", "image_w", "image_h", "epsilon")}
    k1, k2, cx, cy, dx, dy, W, H = (P[k] for k in ("cam_k1", "cam_k2", "cam_cx", "cam_cy", "cam_dx", "cam_dy", "image_w", "image_h"))
    f1, f2 = P["cam_f"] / dx, P["cam_f"] / dy
    out = np.zeros((len(feat), 2))
    for i in range(len(feat)):
        xi, yi, zi, th, ph, rho = (m(v) for v in feat[i])
        hx = xi + mp.cos(ph) * mp.sin(th) / rho - m(pos[i][0])
        hy = yi - mp.sin(ph) / rho - m(pos[i][1])
        hz = zi + mp.cos(ph) * mp.cos(th) / rho - m(pos[i][2])
        c, s = mp.cos(m(psi[i])), mp.sin(m(psi[i]))
        rx, ry, rz = c * hx + s * hy, -s * hx + c * hy, hz
        if rz == 0: ux = uy = mp.mpf(0)
        else:
            uy = cx + f1 * rx / rz + m(err[i][0])
            ux = cy + f2 * ry / rz + m(err[i][1])
            if ux < 10 or ux > W - 10 or uy < 10 or uy > H - 10: ux = uy = mp.mpf(0)
        xu, yu = (ux - cx) * dx, (uy - cy) * dy
        ru = mp.sqrt(xu * xu + yu * yu)
        rd = ru / (1 + k1 * ru ** 2 + k2 * ru ** 4)
        it = 0
        while True:
            if steps is not None and it == steps: break
            step = (rd + k1 * rd ** 3 + k2 * rd ** 5 - ru) / (1 + 3 * k1 * rd ** 2 + 5 * k2 * rd ** 4)
            rd -= step; it += 1
            if steps is None and abs(step) < mp.mpf(10) ** -36: break
            assert it < 200, "the distortion equation did not converge"
        d = 1 + k1 * rd ** 2 + k2 * rd ** 4
        if d == 0: d = P["epsilon"]
        vx, vy = cx + (xu / d) / dx, cy + (yu / d) / dy
        if vx >= 0 and vx <= W and vy >= 0 and vy <= H:
            out[i] = float(vx), float(vy)
    return out


EXACT_N, EXACT_SEED = 1024, 33                 # exact_errs() of the bit-for-bit GPU test; k2_strong: the parity rule decides 10 of its pixels
GENERAL_N, GENERAL_SEED = 4096, 2024      # near_threshold() leaves out at most 1 % of these points under any camera (test_camera_cpu.py)


def general(synth, name):
    """(p, feat, pos, psi, err): the GENERAL_N general points of a camera"""
    p = camera(synth, name)
    return (p,) + general_points(synth, p, GENERAL_N, GENERAL_SEED)


@functools.lru_cache(maxsize=None)
def _mp_reference(name, n):
    import __graft_entry__ as ge
    synth = ge.load_package().synth
    p, feat, pos, psi, err = general(synth, name)
    return mp_project(p, feat[:n], pos[:n], psi[:n], err[:n], steps=None if name in CONVERGED else p["newton_iters"])


def mp_reference(name, n=256):
    """mp_project of the first n of the general points of a camera, computed once per process (few_iters: its own three steps)"""
    return _mp_reference(name, n)
