"""CPU tests of the colour-frame intake and the 2-D overlay (srukf_set_frame_bgr / srukf_associate_held / srukf_render_overlay): the library exports them, the
header declares them, Filter binds them, and the numpy restatement (tests/np_overlay.py) that the GPU tests hold the kernels to bit for bit is right.  No GPU.

BOUND of the 2 x 2 eigen-pair, with u = 2^-53 and l0 the larger eigenvalue (>= every |p_ij|): l0 = t + r passes through eight roundings (p00 + p11, p00 - p11,
d d, p01 p01, their sum, the square root, t + r; the halvings are exact), each at most u relative on a quantity no larger than l0, and numpy.linalg.eigh's own
backward error is a small multiple of u |P|: 16 u l0 for both eigenvalues, absolute (l1 = t - r cancels: its error is relative to l0, not to l1).  The eigenvector
takes seven more (d + r, the two scalings, two squares, their sum, the root, two divisions) and the residual |P v - l0 v| is itself formed in fp64: 32 u l0."""
import math
import os
import re

import numpy as np
import pytest

import np_overlay as OV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srukf_set_frame_bgr", "srukf_associate_held", "srukf_render_overlay")
U = 2.0 ** -53


def test_library_exports_and_header_declares_the_calls(pkg):
    lib = pkg.srukf.load_library()
    txt = open(os.path.join(ROOT, "include", "srukf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in pkg.srukf.EXPORTS
    assert lib.srukf_abi_version() == 6
    for m in ("set_frame_bgr", "associate_held", "render_overlay"):
        assert callable(getattr(pkg.srukf.Filter, m, None)), m


def test_gray_against_the_float_weights():
    rng = np.random.default_rng(0)
    bgr = rng.integers(0, 256, size=(50, 70, 3), dtype=np.uint8)
    g = OV.gray(bgr).astype(np.float64)
    f = 0.299 * bgr[..., 0] + 0.587 * bgr[..., 1] + 0.114 * bgr[..., 2]
    worst = np.abs(g - f).max()
    print(f"gray against 0.299 c0 + 0.587 c1 + 0.114 c2: worst difference {worst:.3f} gray levels")
    assert worst <= 1.0


def test_gray_keeps_a_gray_frame_and_swaps_red_and_blue():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(OV.gray(np.stack([v, v, v], axis=-1)), v)          # the weights sum to 2^14
    assert 4899 + 9617 + 1868 == 1 << 14
    assert OV.gray(np.array([255, 0, 0], dtype=np.uint8)) == 76               # the BLUE byte gets red's weight
    assert OV.gray(np.array([0, 0, 255], dtype=np.uint8)) == 29
    assert OV.gray(np.array([0, 255, 0], dtype=np.uint8)) == 150


def _spd2(seed):
    rng = np.random.default_rng(seed)
    th = rng.uniform(0.0, math.pi)
    lam = 10.0 ** rng.uniform(-6.0, 4.0, 2)
    Q = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    P = (Q * lam) @ Q.T
    return 0.5 * (P + P.T)


def test_eigen_pair_against_eigh():
    worst_val = worst_vec = worst_unit = 0.0
    branches = set()
    for seed in range(500):
        P = _spd2(seed)
        l0, l1, c, s = OV.eigen2(float(P[0, 0]), float(P[0, 1]), float(P[1, 1]))
        w = np.linalg.eigvalsh(P)
        ev = max(abs(l0 - w[1]), abs(l1 - w[0])) / l0
        res = np.abs(P @ np.array([c, s]) - l0 * np.array([c, s])).max() / l0
        unit = abs(c * c + s * s - 1.0)
        worst_val, worst_vec, worst_unit = max(worst_val, ev), max(worst_vec, res), max(worst_unit, unit)
        branches.add(P[0, 0] >= P[1, 1])
        assert ev <= 16 * U and res <= 32 * U and unit <= 8 * U, (seed, ev, res, unit)
    print(f"500 SPD inputs: worst eigenvalue error {worst_val / U:.2f} u l0, worst residual {worst_vec / U:.2f} u l0, worst |c^2 + s^2 - 1| {worst_unit / U:.2f} u")
    assert branches == {True, False}                             # both eigenvector forms (d >= 0, d < 0)


def test_eigen_pair_special_inputs():
    assert OV.eigen2(0.0, 0.0, 0.0) == (0.0, 0.0, 1.0, 0.0)      # r == 0
    assert OV.eigen2(4.0, 0.0, 4.0) == (4.0, 4.0, 1.0, 0.0)
    assert OV.eigen2(1.0, 0.0, 9.0) == (9.0, 1.0, 0.0, 1.0)      # p01 = 0, d < 0: upright
    l0, l1, c, s = OV.eigen2(2.0, 1.0, 2.0)                      # d = 0, p01 != 0: 45 degrees
    assert (l0, l1) == (3.0, 1.0) and c == s and abs(c - math.sqrt(0.5)) < 2 * U
    l0, l1, c, s = OV.eigen2(1e-300, 1e-300, 1e-300)             # squares that would underflow unscaled
    assert abs(c * c + s * s - 1.0) <= 8 * U
    l0, _, _, _ = OV.eigen2(float("nan"), 0.0, 1.0)
    assert l0 != l0


def _mask(a, b, c, s, half=40):
    Y, X = np.mgrid[-half:half + 1, -half:half + 1].astype(np.int64)
    return OV.ellipse_mask(X, Y, dict(mx=0, my=0, a=a, b=b, c=c, s=s)), X, Y


@pytest.mark.parametrize("a,b,angle", [(1, 1, 0.0), (2, 1, 0.3), (2, 2, 1.0), (7, 3, 0.0), (12, 5, 0.7), (20, 20, 0.2), (30, 2, 2.5), (9, 1, math.pi / 4)])
def test_painted_ellipse_set(a, b, angle):
    c, s = math.cos(angle), math.sin(angle)
    m, X, Y = _mask(a, b, c, s)
    assert m.any()
    assert np.array_equal(m, m[::-1, ::-1])                     # point-symmetric about the centre
    p, q = c * X + s * Y, c * Y - s * X
    outer = (p / (a + 1)) ** 2 + (q / (b + 1)) ** 2
    assert (outer[m] <= 1.0 + 1e-12).all()                       # inside the real ellipse (a + 1, b + 1) ...
    if a >= 2 and b >= 2:
        inner = (p / (a - 1)) ** 2 + (q / (b - 1)) ** 2
        assert (inner[m] > 1.0 - 1e-12).all()                    # ... and not inside (a - 1, b - 1)
        assert not m[X.shape[0] // 2, X.shape[1] // 2]
    assert (np.hypot(X, Y)[m] <= a + 1 + 1e-9).all()             # the box the kernel culls by: b <= a
    if a == 1 and b == 1:
        assert m.sum() == 13                                     # the disc of radius 2


def test_render_paint_order_and_rounding():
    src = np.full((40, 60), 90, dtype=np.uint8)
    h = [[20.5, 20.0], [21.5, 20.0]]                             # ties to even: 20 and 22
    z = [[40.0, 20.0], [40.0, 20.0]]
    Si = [[0.0, 0.0, 0.0, 0.0]] * 2
    recs = OV.prep(h, Si, z, [1, 1])
    assert [r["px"] for r in recs] == [20, 22] and all(r["a"] == r["b"] == 1 and r["ellipse"] for r in recs)
    out = OV.render(src, h, Si, z, [1, 1])
    assert tuple(out[20, 20]) == OV.BLUE and tuple(out[20, 40]) == OV.RED and tuple(out[0, 0]) == (90, 90, 90)
    # a later landmark's blue cross over an earlier one's red
    out = OV.render(src, [[0.0, 0.0], [40.0, 20.0]], Si, [[40.0, 20.0], [5.0, 5.0]], [1, 1])
    assert tuple(out[20, 40]) == OV.BLUE
    out = OV.render(src, [[40.0, 20.0], [0.0, 0.0]], Si, [[5.0, 5.0], [40.0, 20.0]], [1, 1])
    assert tuple(out[20, 40]) == OV.RED
    # unmatched, non-finite and huge centres are skipped; NaN in Si keeps the crosses
    nan = float("nan")
    out = OV.render(src, [[20.0, 20.0]] * 4, [[1.0, 0.0, 0.0, 1.0]] * 4, [[40.0, 20.0], [nan, 20.0], [40.0, float("inf")], [2.0 ** 30, 20.0]], [0, 1, 1, 1])
    assert np.array_equal(out, np.repeat(src[:, :, None], 3, axis=2))
    r = OV.prep([[20.0, 20.0]], [[nan, 0.0, 0.0, 1.0]], [[40.0, 20.0]], [1])[0]
    assert r["drawn"] and not r["ellipse"]
    r = OV.prep([[20.0, 20.0]], [[1e6, 0.0, 0.0, 1.0]], [[40.0, 20.0]], [1])[0]
    assert r["drawn"] and not r["ellipse"]                       # l0 = 1e12
