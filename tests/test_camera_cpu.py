"""The camera model's references, held to each other without a GPU (tests/cameras.py): the bit-exact restatement of srukf_project's tail with and without the
device's early exits, that restatement against the oracle, the oracle against a 40-digit mpmath projection, and the preconditions of the GPU comparisons in
test_gpu_camera.py (no point next to a threshold beyond the allowance, every sigma point of the frame scenes in view, no theta clamp)."""
from fractions import Fraction

import numpy as np
import pytest

import cameras as C

# |oracle.project - mp_project| over the first 256 general points of every camera whose iteration converges (few_iters: against its own three mpmath steps).
# Measured worst case 1.279e-13 px (default, k2_strong, odd_iters, few_iters; barrel_neg, nonsquare, small_img 1.137e-13): one ulp of a pixel value above 256
# plus a fraction.  The bound is ten times that; test_gpu_camera.py adds the project's 1e-10 for the device.
MP_MEASURED = 1.28e-13
MP_BOUND = 10 * MP_MEASURED
# 400 pixels over the admissible rectangle.  Under k2_strong 35 to 61 of 400 random pixels end in a 2-cycle and 3 to 8 on different bits after 99 and 100
# iterations, seed by seed (six seeds measured); this seed gives 48 and 8, so that the parity rule decides 2 % of the outputs below.
PIXEL_SEED = 32


def test_fma_is_the_single_rounding_of_the_exact_value():
    rng = np.random.default_rng(0)
    for a, b, c in rng.normal(size=(2000, 3)) * 10.0 ** rng.integers(-8, 8, (2000, 3)):
        a, b, c = float(a), float(b), float(c)
        assert C.fma(a, b, c) == float(Fraction(a) * Fraction(b) + Fraction(c))
    assert C.fma(3.0, 1.0 / 3.0, -1.0) == -2.0 ** -54 and 3.0 * (1.0 / 3.0) - 1.0 == 0.0        # (and it is not the two-rounding form)


@pytest.mark.parametrize("name", C.NAMES)
def test_shortcut_equals_full_loop(synth, name):
    """tail(shortcut=True) == tail(shortcut=False) bit for bit: the fixed-point exit and the 2-cycle exit with its parity rule give what all K iterations
    give, for every K of NEWTON_KS, 400 pixels over the whole admissible rectangle.  (Measured: 0 mismatches, at most 6 iterations before an exit.)"""
    p = C.camera(synth, name)
    ux, uy = C.admissible_pixels(p, 400, seed=PIXEL_SEED)
    full = C.tail_full_table(p, ux, uy)
    worst = 0
    for K in C.NEWTON_KS:
        short = [C.tail(p, x, y, K, True, want_iters=True) for x, y in zip(ux, uy)]
        worst = max(worst, max(s[2] for s in short))
        np.testing.assert_array_equal(np.array([s[:2] for s in short]), full[K], err_msg=f"{name} K={K}")
    print(f"{name}: at most {worst} iterations before an exit")
    assert worst <= 12                                       # (quadratic convergence from a start value within 2 %: the exits are reached, not the loop's end)


def test_parity_branch_is_exercised(synth):
    """Under k2_strong at least 1 % of the pixels end on different bits after 99 and after 100 iterations (measured: 2 %): there the parity of the iterations
    left decides the output, so the bit-for-bit GPU test is not vacuous."""
    p = C.camera(synth, "k2_strong")
    ux, uy = C.admissible_pixels(p, 400, seed=PIXEL_SEED)
    full = C.tail_full_table(p, ux, uy)
    differ = np.any(full[99] != full[100], axis=1).sum()
    print(f"k2_strong: {differ} of 400 pixels differ between K = 99 and K = 100")
    assert differ >= 4
    assert np.array_equal(full[99], full[101])               # a 2-cycle, not drift
    # the pixels test_gpu_camera.py feeds the device, border rows and zeroed pixels included: one such pixel fails a wrong parity; measured: 10 of 1024
    ux, uy, _ = C.exact_seen(p, C.exact_errs(p, C.EXACT_N, seed=C.EXACT_SEED))
    full = C.tail_full_table(p, ux, uy)
    assert np.any(full[99] != full[100], axis=1).sum() >= 4 and np.any(full[2] != full[3], axis=1).sum() >= 500


@pytest.mark.parametrize("name", C.NAMES)
def test_restatement_matches_oracle(synth, oracle, name):
    """tail(shortcut=False) at K = 100 and at the camera's own iteration count (99; 3), fed through the exact-input trick, against oracle.project(early_exit=0): they
    differ by the placement of the fused multiply-adds only (measured: 2.27e-13 px under nonsquare, 1.14e-13 px or nothing under the others).  The border rows are among the pixels: the oracle zeroes
    exactly where the restatement's IEEE comparisons do."""
    for K in sorted({100, C.camera(synth, name)["newton_iters"]}):
        p = C.camera(synth, name, newton_iters=K)
        err = C.exact_errs(p, 400, seed=32)
        ux, uy, zeroed = C.exact_seen(p, err)
        assert zeroed.sum() >= 6 and (~zeroed).sum() >= 300
        ref = C.tail_full_table(p, ux, uy)[K]
        feat, pos, psi = C.exact_inputs(err)
        o0 = oracle.project(p, feat, pos, psi, err, early_exit=0)
        d = np.abs(o0 - ref).max()
        print(f"{name} K={K}: |oracle - restatement| max = {d:.3e} px")
        assert d <= 1e-12
        assert np.array_equal(o0, oracle.project(p, feat, pos, psi, err, early_exit=1))


def test_border_rows_sit_on_the_thresholds(synth):
    """the exact-input border rows: computed ux / uy exactly 10, image_w - 10, image_h - 10 (kept) and the nearest values on either side (one zeroed, one kept)"""
    for name in C.NAMES:
        p = C.camera(synth, name)
        err = C.border_errs(p)
        assert err.shape == (12, 2)
        uy, ux = p["cam_cx"] + err[:, 0], p["cam_cy"] + err[:, 1]
        _, _, zeroed = C.exact_seen(p, err)
        W, H = p["image_w"], p["image_h"]
        assert list(ux[0:6:3]) == [10.0, W - 10.0] and list(uy[6:12:3]) == [10.0, H - 10.0]
        assert ux[1] < 10.0 < ux[2] and ux[4] < W - 10.0 < ux[5] and uy[7] < 10.0 < uy[8] and uy[10] < H - 10.0 < uy[11]
        assert max(ux[2] - ux[1], ux[5] - ux[4], uy[8] - uy[7], uy[11] - uy[10]) < 3e-13
        assert list(zeroed) == [False, True, False, False, False, True] * 2


@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_matches_mpmath(synth, oracle, name):
    """The oracle's projection (the reference's 100 fixed Newton steps in doubles) against the model evaluated in mpmath at 40 digits with the distortion
    equation solved to convergence, on the first 256 general points (landmarks to 200 px from the principal point).  few_iters has not converged after its
    three steps and is held to three mpmath steps.  Measured worst case over the cameras: 1.279e-13 px; asserted: ten times that, 1.28e-12 px."""
    p, feat, pos, psi, err = C.general(synth, name)
    keep = ~C.near_threshold(p, feat, pos, psi, err)[:256]
    o = oracle.project(p, feat[:256], pos[:256], psi[:256], err[:256], early_exit=0)
    d = np.abs(o - C.mp_reference(name))[keep].max()
    print(f"{name}: |oracle - mpmath| max = {d:.3e} px over {keep.sum()} points")
    assert keep.sum() >= 254
    assert d <= MP_BOUND < 1e-9


@pytest.mark.parametrize("name", C.NAMES)
def test_general_points_meet_the_gpu_test_conditions(synth, oracle, name):
    """What test_gpu_camera.py's comparison of 4096 general points presumes, shown with the oracle alone: at most 1 % of the points lie within 1e-6 px of a
    threshold, the oracle agrees with synth.project on the others, its early exit changes no bit, and both zeroing branches occur where they can."""
    p, feat, pos, psi, err = C.general(synth, name)
    near = C.near_threshold(p, feat, pos, psi, err)
    assert near.sum() <= 0.01 * len(near)
    o = oracle.project(p, feat, pos, psi, err, early_exit=0)
    assert np.array_equal(o, oracle.project(p, feat, pos, psi, err, early_exit=1))
    d = np.abs(o - synth.project(feat, pos, psi, err, p))[~near].max()
    print(f"{name}: {near.sum()} of {len(near)} points next to a threshold; |oracle - synth.project| max = {d:.3e} px")
    assert d <= 1e-12                                        # (measured: 1.7e-13 at the worst; numpy's pow against the oracle's products)
    border, oov = C.branches(p, feat, pos, psi, err)
    assert (border & ~near).sum() >= 40                      # coordinatesCamera2Image's zeroing, every camera
    if p["cam_k1"] < 0:
        # The view test of distortOnePointRW can only fail where d < 1 (negative k1): an admitted ux in [10, image_w - 10] is drawn TOWARDS cam_cx by d > 1, and
        # a zeroed one lands on cam_cx (1 - 1/d) in [0, cam_cx).  Among the cameras that is barrel_neg alone; under small_img the branch is unreachable.
        assert (oov & ~near).sum() >= 40 and np.all(o[oov & ~near] == 0.0)
    else:
        assert not oov.any()


@pytest.mark.parametrize("N,radius", C.SCENES)
@pytest.mark.parametrize("name", C.NAMES)
def test_scene_conditions(synth, oracle, name, N, radius):
    """The frame scenes of test_gpu_camera.py keep border discontinuities out of its comparisons: over all six frames every projected sigma point is in view
    (no zero in Oracle.Z()), no theta clamp fires and the state stays finite, in both update modes."""
    sc = C.scene(synth, name, N, radius)
    for mode in (oracle.Oracle.SEQUENTIAL, oracle.Oracle.BATCHED):
        o = oracle.Oracle(N, sc["params"]); o.set_state(sc["X0"], sc["S0"])
        for t in range(C.SCENE_FRAMES):
            o.predict_motion(sc["odo"][t], sc["odo"][t + 1])
            h, Si, vis = o.predict_measurement()
            assert vis.all() and np.all(o.Z() != 0.0), (name, N, t)
            o.update(sc["z"][t], sc["matched"][t], 1, 0, mode)
        X, S = o.get_state()
        assert o.clamp_stats()["theta"] == 0 and np.all(np.isfinite(X)) and np.all(np.isfinite(S))
        o.close()
