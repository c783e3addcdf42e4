"""GPU tests of the checked association (srukf_associate_checked / srukf_get_match_scores, cv-monoslam_amd/csrc/srukf_unique.hip): it must EQUAL
srukf_associate when nothing vetoes, its score map must be the restatement's (tests/np_unique.py: score_map) to 1e-9, and every decision taken on that map — best,
rival, flags, sub-pixel offset — must EQUAL np_unique.peaks run on the device's own map.  The scenes follow test_gpu_parity.py::test_data_association_matches_oracle
(N = 24, seed 13, appearance set by the host), and N = 1; the equality with srukf_associate is also held at 21-wide windows and at a window the image border cuts."""
import math
import os

import numpy as np
import pytest

import np_unique as U
import test_gpu_detect as TD

pytestmark = pytest.mark.gpu
SHIFT = (2, -1)                                                  # (dx, dy) of the scene content between creation and now


def _texture(rng, h=480, w=640):
    """the smooth random texture of test_gpu_parity.py's association test"""
    t = rng.uniform(0, 255, (h, w))
    k = 5
    c = np.cumsum(np.cumsum(np.pad(t, ((k, k), (k, k)), mode="wrap"), axis=0), axis=1)
    t = (c[2 * k:, 2 * k:] - c[:-2 * k, 2 * k:] - c[2 * k:, :-2 * k] + c[:-2 * k, :-2 * k]) / (2 * k) ** 2
    t = (t - t.min()) / (t.max() - t.min()) * 255
    return t.astype(np.uint8)


def _rot(th):
    return np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1.0]])


class Scene:
    """A filter one predict_measurement into its second frame, as the parity test builds it; H: image height (a low image puts landmarks at its border)."""

    def __init__(self, srukf, synth, N, sigma=None, H=480):
        p = dict(synth.scene_params())
        if sigma is not None:
            p["sigma_measure"] = float(sigma)
        self.sc = sc = synth.make_scene(N, 3, seed=13, p=p)
        p["image_h"] = float(H)
        self.p, self.N, self.W, self.H = p, N, 640, H
        self.f = f = srukf.Filter(N, p)
        f.set_state(sc["X0"], sc["S0"])
        self.pose0 = sc["X0"][-4:].copy()
        f.predict_motion(sc["odo"][0], sc["odo"][1]); f.predict_measurement(); f.update(sc["z"][0], sc["matched"][0])
        f.predict_motion(sc["odo"][1], sc["odo"][2])
        h, Si, vis = f.predict_measurement()
        self.h, self.Si, self.vis = h.reshape(N, 2).copy(), Si.reshape(N, 4).copy(), vis.copy()
        self.X, _ = f.get_state()
        self.xyz, _ = f.get_landmarks_cartesian()
        self.pose = self.X[-4:].copy()

    def inside(self, cu, cv):
        return 20 <= cu < self.W - 20 and 20 <= cv <= min(459, self.H - 11)      # (the 21 x 21 patch lies inside the image)

    def set_turned(self, T, skip=()):
        """landmarks 'created' at the first pose from texture T, a few pixels off the prediction: the warp is a real homography.  Returns (init_px, patches)."""
        rng = np.random.default_rng(2)
        R0 = _rot(self.pose0[3])
        init_px, patches = [], []
        for k in range(self.N):
            ipx = self.h[k] - np.array(SHIFT) + rng.uniform(-1.5, 1.5, 2)
            cu, cv = int(round(ipx[0])), int(round(ipx[1]))
            if not self.inside(cu, cv):
                ipx = np.array([self.W / 2.0, 240.0]); cu, cv = self.W // 2, 240
            patch = T[cv - 10:cv + 11, cu - 10:cu + 11].copy()
            init_px.append(ipx); patches.append(patch)
            if k not in skip:
                self.f.set_landmark_appearance(k, patch, R0, self.pose0[:3], ipx)
        return init_px, patches

    def set_current(self, img, skip=()):
        """landmarks created at the CURRENT pose at the rounded predicted pixel, patches cut from img: the identity view"""
        Rc = _rot(self.pose[3])
        for k in range(self.N):
            cu, cv = int(round(self.h[k, 0])), int(round(self.h[k, 1]))
            if not self.vis[k] or not self.inside(cu, cv):
                cu, cv = self.W // 2, 240
            if k not in skip:
                self.f.set_landmark_appearance(k, img[cv - 10:cv + 11, cu - 10:cu + 11].copy(), Rc, self.pose[:3], np.array([float(cu), float(cv)]))

    def flip_si(self):
        """Si with a positive diagonal.  The device's factor has the reference's QR signs (negative diagonal), under which ceil(2 Si00) never exceeds HP_MATCH and every
        window is 17 wide; negating a row of Si leaves the gate Si^T Si as it is and lets the window follow sigma_measure (1953-1956).  Uploaded as the frame's Si."""
        self.Si[:, 0:2] *= np.where(self.Si[:, 0] < 0, -1.0, 1.0)[:, None]
        self.Si[:, 2:4] *= np.where(self.Si[:, 3] < 0, -1.0, 1.0)[:, None]
        self.f.debug_upload("Si", self.Si)

    def patches_now(self):
        return [self.f.get_match_patch(k) for k in range(self.N)]


def _frame(T, H=480):
    return np.ascontiguousarray(np.roll(T, (SHIFT[1], SHIFT[0]), axis=(0, 1))[:H])


def _same(a, r):
    return np.array_equal(a[0], r["z"]) and np.array_equal(a[1], r["matched"]) and np.array_equal(a[2], r["corr"])


def _check_peaks(s, r, params, ks=None):
    """every output of the device call r EQUALS np_unique.peaks on the device's own maps; returns the per-landmark peak records"""
    recs = {}
    for k in (range(s.N) if ks is None else ks):
        m, x0, y0 = s.f.match_scores(k)
        if m.size == 0:
            assert not r["matched"][k] and r["flags"][k] == 0 and r["corr"][k] == 0 and r["corr2"][k] == 0
            assert not r["z"][2 * k:2 * k + 2].any() and not r["z2"][2 * k:2 * k + 2].any()
            continue
        wy, wx = m.shape
        pk = U.peaks(m, s.h[k, 0], s.h[k, 1], (wx - 1) // 2, (wy - 1) // 2, params)
        assert (x0, y0) == (int(s.h[k, 0]) - (wx - 1) // 2, int(s.h[k, 1]) - (wy - 1) // 2)
        assert r["corr"][k] == pk["corr"], k
        assert tuple(r["z"][2 * k:2 * k + 2]) == pk["z"], (k, r["z"][2 * k:2 * k + 2], pk["z"])
        assert r["corr2"][k] == pk["corr2"], (k, r["corr2"][k], pk["corr2"])
        assert tuple(r["z2"][2 * k:2 * k + 2]) == pk["z2"], k
        assert r["flags"][k] == pk["flags"] and r["matched"][k] == pk["matched"], (k, r["flags"][k], pk["flags"])
        recs[k] = pk
    return recs


def _scene(srukf, synth, N, sigma, H, flip):
    s = Scene(srukf, synth, N, sigma=sigma, H=H)
    if flip:
        s.flip_si()
    return s


# the scenes of test_score_map_against_restatement: 17-wide windows, 21-wide windows (sigma_measure 5, Si's diagonal made positive), a window cut by the border
@pytest.mark.parametrize("N, sigma, H, flip", [(24, None, 480, False), (1, None, 480, False), (24, 5, 480, True), (24, 3, 380, False)],
                         ids=["24", "1", "24-sigma5-flipped", "24-sigma3-H380"])
def test_equals_associate_when_nothing_vetoes(srukf, synth, N, sigma, H, flip):
    T = _texture(np.random.default_rng(2))
    frame = _frame(T, H)
    s = _scene(srukf, synth, N, sigma, H, flip)
    f = s.f
    skip = (5,) if N > 5 else ()
    for half in ("turned", "identity"):
        if half == "turned":
            s.set_turned(T, skip)
        else:
            s.set_current(frame, skip)
        a = f.associate(frame); pa = s.patches_now()
        r = f.associate_checked(frame, ratio=2.0, subpixel=False); pr = s.patches_now()
        assert _same(a, r) and not (r["flags"] & 6).any() and np.array_equal(r["flags"] & 1, r["matched"])
        assert all(np.array_equal(x, y) for x, y in zip(pa, pr))
        a = f.associate_held(); pa = s.patches_now()
        r = f.associate_checked(None, ratio=2.0); pr = s.patches_now()
        assert _same(a, r) and all(np.array_equal(x, y) for x, y in zip(pa, pr))
        if half == "identity":
            assert r["matched"].sum() >= max(1, int(s.vis.sum()) // 2)      # (something did match: the comparison is not between zeros)
        maps = [f.match_scores(k) for k in range(N)]            # (the scene is what its name says)
        if flip:
            assert any(21 in m.shape for m, _, _ in maps)
        if H < 480:
            assert any(m.size and y0 + m.shape[0] - 1 > H - 9 for m, _, y0 in maps)
    # two consecutive frames: one call on the first, the other on the second, against associate on both
    sc = s.sc
    runs = []
    for order in (("a", "a"), ("c", "a"), ("a", "c")):
        g = _scene(srukf, synth, N, sigma, H, flip)             # (the flipped Si is the first frame's: the second frame's is the device's own)
        g.set_current(frame, skip)
        out = []
        for t, which in enumerate(order):
            if which == "a":
                z, m, cr = g.f.associate(frame)
            else:
                r = g.f.associate_checked(frame, ratio=2.0)
                z, m, cr = r["z"], r["matched"], r["corr"]
            out.append((z.copy(), m.copy(), cr.copy(), g.patches_now()))
            if t == 0:
                g.f.update(z, m)
                g.f.predict_motion(sc["odo"][2], sc["odo"][3]); g.f.predict_measurement()
        runs.append(out)
    for other in runs[1:]:
        for t in range(2):
            for q in range(3):
                assert np.array_equal(runs[0][t][q], other[t][q]), (t, q)
            assert all(np.array_equal(x, y) for x, y in zip(runs[0][t][3], other[t][3]))
    assert runs[0][0][1].sum() >= 1 and runs[0][1][2].max() > 0.0   # (not a comparison between zeros)


def test_score_map_against_restatement(srukf, oracle, synth):
    """match_scores(k) against np_unique.score_map fed the ORACLE's template; 1e-9 per entry, the bound the project holds corr to (test_gpu_parity.py:405).
    sigma_measure 3 and 5: 17- and 21-wide windows (the latter with Si's diagonal made positive, Scene.flip_si).  A 380-row image cuts the window of a landmark
    at its lower border (the height was found with the CPU oracle: predictions near a border move with the image size, their sigma points being zeroed outside it).
    Measured (MI355X): worst |device - restatement| 5.6e-16."""
    T = _texture(np.random.default_rng(2))
    all_sizes, all_cut = set(), {}
    for sigma, H, flip in ((3, 480, False), (5, 480, True), (3, 380, False)):
        frame = _frame(T, H)
        s = Scene(srukf, synth, 24, sigma=sigma, H=H)
        if flip:
            s.flip_si()
        init_px, patches = s.set_turned(T, skip=(5,))
        r = s.f.associate_checked(frame)
        R0 = _rot(s.pose0[3])
        sizes, cut, worst = set(), 0, 0.0
        for k in range(s.N):
            m, x0, y0 = s.f.match_scores(k)
            if k == 5 or not s.vis[k]:                          # no appearance record / not visible: all outputs zero, no window
                assert m.shape == (0, 0) and (x0, y0) == (0, 0)
                assert r["matched"][k] == 0 and r["flags"][k] == 0 and r["corr"][k] == 0.0 and r["corr2"][k] == 0.0
                assert not r["z"][2 * k:2 * k + 2].any() and not r["z2"][2 * k:2 * k + 2].any()
                continue
            mp_o = oracle.warp_patch(s.p, s.X[-4:], R0, s.pose0[:3], init_px[k], s.xyz[k], s.h[k], patches[k], np.zeros((17, 17), dtype=np.uint8))
            ref, rx0, ry0 = U.score_map(s.p, frame, s.h[k], s.Si[k], mp_o)
            assert m.shape == ref.shape and (x0, y0) == (rx0, ry0), (k, m.shape, ref.shape)
            sizes.update(m.shape)
            worst = max(worst, np.abs(m - ref).max())
            np.testing.assert_allclose(m, ref, rtol=0, atol=1e-9)
            assert np.array_equal(m == 0.0, ref == 0.0)         # the same candidates skipped
            ys = y0 + np.arange(m.shape[0])
            out = (ys < 8) | (ys > H - 9)                        # 1969
            if out.any():
                assert not m[out].any() and not ref[out].any()
                cut += bool(m[~out].any())                       # (a template that the warp left empty scores 0 everywhere)
        print(f"sigma {sigma} H {H}: window sizes {sorted(sizes)}, cut windows {cut}, worst |device - restatement| {worst:.3e}")
        all_sizes |= sizes
        all_cut[H] = all_cut.get(H, 0) + cut
    assert all_cut[380] >= 1 and all_cut[480] == 0               # a window the image border cuts
    assert {17, 21} <= all_sizes, all_sizes                      # both window sizes occurred


def _tiled(base, centres, seed=9):
    """a 6-px periodic random tile region (+-33 px) around every centre"""
    rng = np.random.default_rng(seed)
    img = base.copy()
    for (cx, cy) in centres:
        tile = rng.integers(0, 256, (6, 6)).astype(np.uint8)
        img[cy - 33:cy + 34, cx - 33:cx + 34] = np.tile(tile, (12, 12))[:67, :67]
    return img


def test_peaks_exact_on_the_device_map(srukf, synth):
    base = TD.texture(4)
    s = Scene(srukf, synth, 24)
    centres, ks = [], []
    for k in range(s.N):
        c = (int(round(s.h[k, 0])), int(round(s.h[k, 1])))
        if s.vis[k] and 45 <= c[0] < 640 - 45 and 45 <= c[1] < 480 - 45 and all(math.hypot(c[0] - o[0], c[1] - o[1]) >= 70 for o in centres):
            centres.append(c); ks.append(k)
    assert len(centres) >= 3
    centres, ks = centres[:3], ks[:3]
    frame = _tiled(base, centres)
    s.set_current(frame)
    for excl in (4, 6, 12):
        par = dict(corr_threshold=0.8, ratio=0.9, exclusion=excl, subpixel=False)
        r = s.f.associate_checked(frame, **par)
        recs = _check_peaks(s, r, par)
        assert all(recs[k]["raw"] for k in ks)
    par = dict(corr_threshold=0.8, ratio=1.0, exclusion=4, subpixel=False)
    r = s.f.associate_checked(frame, **par)
    _check_peaks(s, r, par)
    for k in ks:                                                 # identical pixels in identical order: bit-equal scores at the aliases
        assert r["flags"][k] == 3 and r["matched"][k] == 0 and r["corr2"][k] == r["corr"][k] and r["corr"][k] > 0.8, (k, r["corr"][k], r["corr2"][k])
        m, _, _ = s.f.match_scores(k)
        assert (m == m.max()).sum() >= 5
        d = r["z2"][2 * k:2 * k + 2] - r["z"][2 * k:2 * k + 2]
        di = np.rint(d)
        assert np.abs(d - di).max() < 1e-9 and di[0] % 6 == 0 and di[1] % 6 == 0 and np.abs(di).max() >= 6      # the rival is an alias of the best
    # plain texture: nothing is ambiguous at 0.9, and the second peak stays well below (tests/test_unique_cpu.py::test_second_peak_on_smooth_texture: 0.667 over 42 centres)
    s.set_current(base)
    par = dict(corr_threshold=0.8, ratio=0.9, exclusion=4, subpixel=False)
    r = s.f.associate_checked(base, **par)
    _check_peaks(s, r, par)
    raw = (r["flags"] & 1) != 0
    assert raw.sum() >= int(s.vis.sum()) // 2 and not (r["flags"] & 2).any()
    ratio = (r["corr2"][raw] / r["corr"][raw]).max()
    print(f"plain texture(4): largest corr2 / corr = {ratio:.3f} over {raw.sum()} landmarks")
    assert ratio < 0.9


def test_subpixel(srukf, synth):
    """texture(4) with its content shifted by (0.3, 0.6) px (bilinear); patches cut from the unshifted texture at the current pose.
    |z - truth| is the Euclidean length of the 2-vector; the integer centre is off by |(0.3, 0.4)| = 0.5 px.  Measured (MI355X): 24 of 24 visible landmarks
    refined, worst |z - truth| 0.245 px (largest single component 0.234 px) against 0.500 px for the integer centre.  The bound 0.25 px holds on these landmarks with little room: the
    same study on the CPU over 42 other centres (tests/test_unique_cpu.py::test_subpixel_study_on_smooth_texture) has a worst case of 0.290 px."""
    T = TD.texture(4)
    t = T.astype(np.float64)
    fx, fy = 0.3, 0.6
    sh = t.copy()
    sh[1:, 1:] = (1 - fx) * (1 - fy) * t[1:, 1:] + fx * (1 - fy) * t[1:, :-1] + (1 - fx) * fy * t[:-1, 1:] + fx * fy * t[:-1, :-1]     # frame(x, y) = T(x - 0.3, y - 0.6)
    shifted = np.rint(sh).astype(np.uint8)
    s = Scene(srukf, synth, 24)
    s.set_current(T)
    par = dict(corr_threshold=0.8, ratio=2.0, exclusion=4, subpixel=True)
    r = s.f.associate_checked(shifted, **par)
    recs = _check_peaks(s, r, par)
    refined, worst, worst_int = 0, 0.0, 0.0
    for k, pk in recs.items():
        if not pk["flags"] & 4:
            continue
        ref, x0, y0 = U.score_map(s.p, T, s.h[k], s.Si[k], s.f.get_match_patch(k))      # the restatement's integer best on the unshifted texture
        b = int(np.argmax(ref))                                  # (first maximum)
        truth = np.array([x0 + b % ref.shape[1] + fx, y0 + b // ref.shape[1] + fy])
        z = r["z"][2 * k:2 * k + 2]
        err = math.hypot(z[0] - truth[0], z[1] - truth[1])
        worst, worst_int = max(worst, err), max(worst_int, float(np.linalg.norm(np.floor(z + 0.5) - truth)))
        print(f"landmark {k}: z {z} truth {truth} |z - truth| {err:.3f}")
        refined += 1
    print(f"sub-pixel: {refined} refined of {int(s.vis.sum())} visible, worst |z - truth| {worst:.3f} px (integer centre: {worst_int:.3f})")
    assert refined >= (int(s.vis.sum()) + 1) // 2
    assert worst <= 0.25


def test_arguments(srukf, synth):
    sc_p = synth.scene_params()
    sc = synth.make_scene(4, 3, seed=13, p=sc_p)
    f = srukf.Filter(4, sc_p); f.set_state(sc["X0"], sc["S0"])
    frame = TD.texture(4)

    def rc_of(call):
        with pytest.raises(srukf.SrukfError) as e:
            call()
        return e.value.rc

    assert rc_of(lambda: f.match_scores(0)) == -5                # no checked call yet
    assert rc_of(lambda: f.associate_checked(frame)) == -5       # before predict_measurement
    f.predict_motion(sc["odo"][0], sc["odo"][1])
    assert rc_of(lambda: f.associate_checked(frame)) == -5
    f.predict_measurement()
    assert rc_of(lambda: f.associate_checked(None)) == -5        # no frame held
    for kw in (dict(ratio=0.0), dict(ratio=-1.0), dict(ratio=float("nan")), dict(ratio=float("inf")), dict(exclusion=0), dict(exclusion=21),
               dict(corr_threshold=float("nan")), dict(corr_threshold=float("inf"))):
        assert rc_of(lambda: f.associate_checked(frame, **kw)) == -1, kw
    r = f.associate_checked(frame, exclusion=20)
    assert not r["matched"].any()                                # no appearance records
    m, x0, y0 = f.match_scores(0)
    assert m.shape == (0, 0)
    assert rc_of(lambda: f.match_scores(4)) == -1
    f.update(r["z"], r["matched"])
    f.add_landmarks([[300.0, 200.0]])
    assert rc_of(lambda: f.match_scores(0)) == -5                # the maps went with the map change
    f.reset()
    assert rc_of(lambda: f.match_scores(0)) == -5


def _periodic_frame(base, cx, cy, R=45, seed=5):
    """a 6-px periodic region around (cx, cy) whose contrast falls gently from the centre (so that detection takes its corners centre first, well inside the region)"""
    rng = np.random.default_rng(seed)
    tile = rng.integers(0, 256, (6, 6)).astype(np.float64)
    reg = np.tile(tile, (2 * R // 6 + 2, 2 * R // 6 + 2))[:2 * R + 1, :2 * R + 1]
    yy, xx = np.mgrid[-R:R + 1, -R:R + 1]
    env = 1.0 - 0.3 * np.maximum(np.abs(yy), np.abs(xx)) / R
    img = base.copy()
    img[cy - R:cy + R + 1, cx - R:cx + R + 1] = np.rint(128 + (reg - 128) * env).astype(np.uint8)
    return img


def _lines(out, key):
    return [ln for ln in out.splitlines() if ln.split() and ln.split()[0] == key]


def test_facade_vetoes_ambiguous_landmarks(tmp_path, synth, pkg):
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    base = TD.texture(31)
    odo = [(0.01 * i, 0.0, 0.0) for i in range(5)]
    # (a) unique=2 never vetoes: the default run's lines, plus "ambiguous 0" per frame
    frames = [np.roll(base, (0, q), axis=(0, 1)) for q in range(4)]
    d0, d1 = tmp_path / "a", tmp_path / "b"
    d0.mkdir(); d1.mkdir()
    plain = TD._run_vision(str(d0), frames, odo)
    uniq = TD._run_vision(str(d1), frames, odo, "unique=2")
    keep = lambda out: [ln for ln in out.splitlines() if not ln.startswith(("ambiguous", "add_features_frame1_ms"))]
    assert keep(plain) == keep(uniq)
    assert not _lines(plain, "ambiguous")
    amb = _lines(uniq, "ambiguous")
    assert len(amb) == len(_lines(uniq, "frame")) == 4 and all(ln.split() == ["ambiguous", "0"] for ln in amb)
    assert any(rec["matches"] > 0 for rec in TD._parse(uniq))
    # (b) frames that carry a periodic region: the landmarks created inside it are reported, and m_nMatches is lower by their number
    cx, cy = 400, 240
    frames = [_periodic_frame(base, cx, cy)] * 3
    d2, d3 = tmp_path / "c", tmp_path / "d"
    d2.mkdir(); d3.mkdir()
    free = TD._run_vision(str(d2), frames, odo[:4], "unique=2")
    veto = TD._run_vision(str(d3), frames, odo[:4], "unique=0.9,4")
    rf, rv = TD._parse(free), TD._parse(veto)
    init = rv[0]["init"]                                         # the map the second frame associates: IDs 1 .. in this order
    assert np.array_equal(init, rf[0]["init"])
    inside = [k + 1 for k in range(len(init)) if max(abs(init[k, 0] - cx), abs(init[k, 1] - cy)) <= 45 - 20]
    assert inside
    ids = [int(v) for v in _lines(veto, "ambiguous")[1].split()[2:]]
    n = int(_lines(veto, "ambiguous")[1].split()[1])
    assert n == len(ids) and set(inside) <= set(ids), (inside, ids)
    assert all(max(abs(init[i - 1, 0] - cx), abs(init[i - 1, 1] - cy)) <= 45 for i in ids)
    assert rf[1]["matches"] - rv[1]["matches"] == n and n >= 1
    assert _lines(free, "ambiguous")[1].split() == ["ambiguous", "0"]


def _overlay_rows(path):
    rows = {}
    for ln in open(path + ".in"):
        t = ln.split()
        v = [float.fromhex(x) for x in t[:8]]
        rows[(v[0], v[1])] = (np.array(v[6:8]), int(t[8]))        # predicted pixel -> (matchLocation, isMatching)
    return rows


def test_facade_subpixel_matches(tmp_path, synth, pkg):
    """cslam_vision subpix=1 (CSLAM::subpixelMatches alone: ratio 2.0, nothing vetoed): the second frame matches the same landmarks as the default run, and their
    matchLocation is the default run's integer centre (its matchLocation minus the fraction of the prediction) plus an offset within +-0.5 px."""
    assert os.path.exists(TD.VISION), "run __graft_entry__.build() first"
    base = TD.texture(31)
    frames = [base, np.roll(base, (0, 1), axis=(0, 1))]
    odo = [(0.01 * i, 0.0, 0.0) for i in range(3)]
    d0, d1 = tmp_path / "a", tmp_path / "b"
    d0.mkdir(); d1.mkdir()
    plain = TD._run_vision(str(d0), frames, odo, f"overlay={d0}/ovl.bin")
    sub = TD._run_vision(str(d1), frames, odo, "subpix=1", f"overlay={d1}/ovl.bin")
    rp, rs = TD._parse(plain), TD._parse(sub)
    assert len(rp) == len(rs) == 2 and rp[1]["matches"] == rs[1]["matches"] and rs[1]["matches"] >= 1
    assert not _lines(sub, "ambiguous")
    a, b = _overlay_rows(f"{d0}/ovl.bin"), _overlay_rows(f"{d1}/ovl.bin")
    seen = moved = 0
    for h, (zd, md) in a.items():
        if not md or h not in b:
            continue
        zs, ms = b[h]
        assert ms
        centre = zd - (np.array(h) - np.trunc(np.array(h)))     # 1991-1992 without the fraction of the prediction
        assert np.abs(centre - np.rint(centre)).max() < 1e-9
        assert np.abs(zs - np.rint(centre)).max() <= 0.5
        seen += 1
        moved += bool(np.abs(zs - np.rint(centre)).max() > 0)
    assert seen >= 1 and moved >= 1
