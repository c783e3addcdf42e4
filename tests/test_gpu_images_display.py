"""GPU tests of the display view behind image frames and of the overlay of a staged frame (srukf_images_display / srukf_get_image_display /
srukf_render_image_overlay, k_image_view; csrc/srukf_predict.hip, srukf_images.hip).  The yardstick is the library's own step-wise display: row t
of a run with the switch on must hold, byte for byte, what get_frame_view_display() (xyz, cov, axis, sigma, pose, P4) and get_landmarks_display() (rot) return on
a fresh handle that ran frames 0 .. t with the switch off; the overlay of frame t must be render_overlay's bytes on a second handle that holds the frame as a
colour frame and is fed with the record's rows from the host.

Scenes and helpers: tests/test_gpu_images.py's (N = 8 and 33, 640 x 480, at most 11 staged frames), tests/test_gpu_policy.py's seeded policy (first_change == 2),
tests/test_gpu_images_ransac.py's outlier scene (4.8 px) and tests/test_gpu_images_archive.py's archive.  Everything is compared as bytes, NaN positions included
and a NaN's sign not (DESIGN.md §14's rule), except the Si row against predict_measurement() of the step-wise route, which is held to 1e-9: the bound
tests/test_gpu_images.py::test_against_the_stepwise_calls holds h to between the same two routes."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_images_archive as gia
from test_gpu_images import F_MAX, NO_RECORD, _case, _filter, _patch_bytes, _record_bytes, _state_bytes
from test_gpu_policy import NEUTRAL, _policy_filter
from test_gpu_images_ransac import OUT_LM, THR, _ransac_bytes, _ransac_filter

pytestmark = pytest.mark.gpu

MODES = ["BATCHED", "JOINT"]
VIEW = ("xyz", "cov", "axis", "sigma", "rot", "pose", "P4")      # what the step-wise getters have
KEYS = VIEW + ("Si",)


def _mode(srukf, name):
    return getattr(srukf, "UPDATE_" + name)


def _run(f, first, count, mode, checked=False):
    return f.run_images_checked(first, count, mode=mode, **NEUTRAL) if checked else f.run_images(first, count, mode=mode)


def _canon(a):
    """the bytes of a, every NaN as one NaN"""
    a = np.array(a, copy=True)
    if a.dtype.kind == "f": a[np.isnan(a)] = np.nan
    return a.tobytes()


def _rows(rec, a=0, b=None, keys=KEYS):
    return tuple(_canon(rec[k][a:b]) for k in keys)


def _view(g):
    """the step-wise display of handle g now, as one row of the record (without Si)"""
    _, xyz, cov, axis, sigma, pose, P4 = g.get_frame_view_display()
    rot = g.get_landmarks_display()[4]
    d = dict(xyz=xyz, cov=cov, axis=axis, sigma=sigma, rot=rot, pose=pose, P4=P4)
    return tuple(_canon(d[k][None]) for k in VIEW)


def _all_zero(rec):
    return not any(np.asarray(rec[k]).view(np.uint8).any() for k in KEYS)


def _against_fresh(make, frames, mode, checked=False, staged=6):
    """row t of a run of `staged` frames on make(display=True) against the view of make(display=False) behind frames 0 .. t, for every t of `frames`"""
    f = make(True)
    _run(f, 0, staged, mode, checked)
    assert f.clamp_info() == (-1, -1)
    rec = f.get_image_display(0, staged)
    f.close()
    for t in frames:
        g = make(False)
        _run(g, 0, t + 1, mode, checked)
        assert g.clamp_info() == (-1, -1)
        want = _view(g)
        g.close()
        got = _rows(rec, t, t + 1, VIEW)
        assert got == want, (t, [VIEW[i] for i, (a, b) in enumerate(zip(got, want)) if a != b])
    return rec


# ---- 1. rows against a fresh handle ----
@pytest.mark.parametrize("checked", [False, True])
@pytest.mark.parametrize("mode_name", MODES)
def test_rows_against_a_fresh_handle(srukf, synth, mode_name, checked):
    cs = _case(srukf, synth, 8)

    def make(display):
        f = _filter(srukf, cs, 6)
        f.images_display(display)
        return f

    f = make(True)
    _run(f, 0, 6, _mode(srukf, mode_name), checked)
    rec = f.get_image_display(0, 6)
    f.close()
    assert all(a != b for a, b in zip(_rows(rec, 0, 1), _rows(rec, 5, 6))), "rows 0 and 5 do not differ: the comparison would be vacuous"
    assert (rec["rot"] >= 0).all() and np.isfinite(rec["sigma"]).all()
    _against_fresh(make, (0, 2, 5), _mode(srukf, mode_name), checked)


# ---- 2. the Si row ----
@functools.lru_cache(maxsize=None)
def _stepwise_si(srukf, synth, mode, F=6):
    """predict_measurement()'s Si and visible of every frame on the step-wise twin of tests/test_gpu_images.py::_stepwise"""
    cs = _case(srukf, synth, 8)
    g = _filter(srukf, cs)
    Sis, viss = [], []
    for t in range(F):
        g.predict_motion(cs["odo"][t], cs["odo"][t + 1])
        _, Si, vis = g.predict_measurement()
        z, m, _ = g.associate(cs["frames"][t])
        if mode == srukf.UPDATE_JOINT: g.update_joint(z, m)
        else: g.update(z, m, mode=srukf.UPDATE_BATCHED)
        Sis.append(np.array(Si, copy=True).reshape(-1)); viss.append(np.array(vis, copy=True))
    g.close()
    return np.array(Sis), np.array(viss)


@pytest.mark.parametrize("mode_name", MODES)
def test_si_row_is_what_the_association_read(srukf, synth, mode_name):
    F, mode = 6, _mode(srukf, mode_name)
    cs = _case(srukf, synth, 8)
    f = _filter(srukf, cs, F)
    f.images_display(True)
    f.run_images(0, F, mode=mode)
    Si = f.get_image_display(0, F)["Si"]
    vis = f.get_image_matches(0, F)["visible"]
    f.close()
    ref, rvis = _stepwise_si(srukf, synth, mode)
    assert np.array_equal(vis, rvis) and vis.any()
    d = np.abs(Si.reshape(F, -1) - ref).max()
    print("Si row against predict_measurement() of the step-wise twin, %s: max |d| %.3e" % (mode_name, d))
    assert d <= 1e-9
    nz = np.abs(Si.reshape(F, 8, 4)).max(axis=2) > 0
    assert nz[vis != 0].all(), "a visible landmark with a zero Si row"


# ---- 3. read-only ----
@pytest.mark.parametrize("policy,ransac", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("mode_name", MODES)
def test_display_is_read_only(srukf, synth, mode_name, policy, ransac):
    """11 frames, the switch on against off: trajectory, X, S, the match record, every matchPatch and the records of the options are bit-identical"""
    F, mode = F_MAX, _mode(srukf, mode_name)
    out = []
    for display in (True, False):
        f = _policy_filter(srukf, synth, F) if policy else _filter(srukf, _case(srukf, synth, 8), F)
        if ransac: f.images_ransac(True, 1000.0)
        f.images_display(display)
        t = f.run_images(0, F, mode=mode)
        assert f.clamp_info() == (-1, -1)
        res = (t.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + (_patch_bytes(f),)
        if policy:
            r = f.get_image_policy(0, F)
            res += (r["verdict"].tobytes(), r["summary"].tobytes(), r["state"].tobytes(), r["first_change"])
        if ransac: res += _ransac_bytes(f.get_image_ransac(0, F))
        assert _all_zero(f.get_image_display(0, F)) == (not display)
        out.append(res)
        f.close()
    assert out[0] == out[1], [i for i, (a, b) in enumerate(zip(*out)) if a != b]


# ---- 4. graph forms ----
@pytest.mark.parametrize("mode_name", MODES)
def test_graph_forms_leave_one_record(srukf, synth, mode_name):
    F, mode = F_MAX, _mode(srukf, mode_name)
    cs = _case(srukf, synth, 8)
    out = []
    for name in ("default", "eager", "async"):
        f = _filter(srukf, cs, F, graph=0 if name == "eager" else None)
        f.images_display(True)
        if name == "async":
            f.run_images_async(0, 5, mode=mode); f.run_images_async(5, 6, mode=mode); f.synchronize()
        else:
            f.run_images(0, F, mode=mode)
        assert f.clamp_info() == (-1, -1)
        out.append(_rows(f.get_image_display(0, F)) + _state_bytes(f))
        f.close()
    assert out[0] == out[1] and out[0] == out[2]
    assert out[0][KEYS.index("Si")] != bytes(len(out[0][KEYS.index("Si")]))


# ---- 5. other options ----
def test_with_the_archive_search_and_with_snapshots(srukf, synth):
    """neither option changes the state: the record is the plain run's"""
    F = 6
    cs = _case(srukf, synth, 8)
    f = _filter(srukf, cs, F); f.images_display(True); f.run_images(0, F)
    plain = _rows(f.get_image_display(0, F)); f.close()
    f = gia._searching(srukf, synth, F); f.images_display(True); f.run_images(0, F)
    assert f.get_image_archive(0, F)["L"] == 5
    searched = _rows(f.get_image_display(0, F)); f.close()
    f = _filter(srukf, cs, F); f.images_snapshots(True); f.images_display(True); f.run_images(0, F)
    assert f.get_image_snapshots() == (4, 5)
    snapped = _rows(f.get_image_display(0, F)); f.close()
    assert searched == plain and snapped == plain


@pytest.mark.parametrize("mode_name", MODES)
def test_with_the_consensus_on_the_outlier_scene(srukf, synth, mode_name):
    def make(display):
        f = _ransac_filter(srukf, synth, "outlier", 6, THR)
        f.images_display(display)
        return f

    rec = _against_fresh(make, (0, 2, 5), _mode(srukf, mode_name))
    cs = _case(srukf, synth, 8)
    f = _filter(srukf, cs, 6); f.images_display(True); f.run_images(0, 6, mode=_mode(srukf, mode_name))
    clean = f.get_image_display(0, 6); f.close()
    assert _rows(rec, 5, 6, VIEW) != _rows(clean, 5, 6, VIEW)      # the consensus changed what the filter used, and the view shows it


# ---- 6. resume and rewind ----
def test_resume_keeps_the_rows_in_front_of_the_stop_and_rewind_none(srukf, synth):
    F, keep = 6, 3
    f = _policy_filter(srukf, synth, F)
    f.images_snapshots(True); f.images_display(True)
    f.run_images(0, F)
    assert f.get_image_policy(0, F)["first_change"] == 2
    assert not _all_zero(f.get_image_display(keep, F - keep))
    f.images_resume(keep)
    rec = f.get_image_display(0, F)
    for t in range(keep, F):
        with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(t)
        assert e.value.rc == -5
    assert f.render_image_overlay(keep - 1).shape == (480, 640, 3)
    f.close()
    assert _all_zero({k: rec[k][keep:] for k in KEYS})
    for t in range(keep):
        g = _policy_filter(srukf, synth, F)
        g.run_images(0, t + 1)
        want = _view(g); g.close()
        assert _rows(rec, t, t + 1, VIEW) == want, t
    f = _policy_filter(srukf, synth, F)
    f.images_display(True)
    f.run_images(0, F)
    assert not _all_zero(f.get_image_display(0, F))
    f.images_rewind()
    assert _all_zero(f.get_image_display(0, F))
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(0)
    assert e.value.rc == -5
    f.close()


# ---- 7. a flagged block ----
def test_flagged_block_leaves_a_zero_record(srukf, synth):
    F = 6
    cs = _case(srukf, synth, 8, "shipped")
    f = _filter(srukf, cs, F)
    f.images_display(True)
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F)
    assert e.value.rc == -7, str(e.value)
    assert _all_zero(f.get_image_display(0, F))
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(0)
    assert e.value.rc == -5
    frame, _ = f.clamp_info()
    if frame > 0:                                                # the frames in front of the flagged one are clean, and their rows come back
        f.run_images(0, frame)
        assert _rows(f.get_image_display(frame - 1, 1), keys=VIEW) == _view(f)
    f.close()


# ---- 8. lifetime and refusals ----
def test_lifetime_and_refusals(srukf, synth):
    cs = _case(srukf, synth, 8)
    N, F = 8, 3
    zeros = (np.zeros((F, 2 * N)), np.zeros((F, N), dtype=np.int32))
    f = _filter(srukf, cs, F)
    assert _all_zero(f.get_image_display(0, F))                  # no run has allocated the record
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(0)
    assert e.value.rc == -5
    f.images_display(True)
    f.run_images(0, F)
    twin = _rows(f.get_image_display(0, F))
    assert _rows(f.get_image_display(F - 1, 1), keys=VIEW) == _view(f)
    # the getter's and the overlay's codes
    with pytest.raises(srukf.SrukfError) as e: f.get_image_display(0, F + 1)
    assert e.value.rc == -2
    with pytest.raises(srukf.SrukfError) as e: f.get_image_display(F, 1)
    assert e.value.rc == -2
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(F)
    assert e.value.rc == -1
    assert f._lib.srukf_get_image_display(f._h, 0, 1, None, None, None, None, None, None, None, None) == -1
    assert f._lib.srukf_render_image_overlay(f._h, 0, None) == -1
    one = np.zeros((1, 4))
    assert f._lib.srukf_get_image_display(f._h, 0, 1, None, None, None, None, None, one.ctypes.data_as(C.POINTER(C.c_double)), None, None) == 0      # any one pointer will do
    assert one.any()
    # a frame run again without the switch keeps its row (the rule of get_image_checks) but is not drawable any more: its Si would be the earlier run's
    f.images_display(False); f.set_state(cs["X1"], cs["S1"]); f.run_images(0, 1)
    assert _rows(f.get_image_display(0, F)) == twin
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(0)
    assert e.value.rc == -5
    assert f.render_image_overlay(1).shape == (480, 640, 3)
    f.images_display(True)
    # the switch is refused in flight and with a block pending
    f.set_state(cs["X1"], cs["S1"])
    f.run_images_async(0, 2)
    for on in (False, True):
        with pytest.raises(srukf.SrukfError) as e: f.images_display(on)
        assert e.value.rc == -5
    f.synchronize()
    f.images_display(True)
    # restaging drops the record, the switch survives
    f.set_state(cs["X1"], cs["S1"])
    f.stage_sequence(cs["odo"][:F + 1], *zeros)
    with pytest.raises(srukf.SrukfError) as e: f.get_image_display(0, F)
    assert e.value.rc == -5
    f.stage_images(cs["frames"][:F])
    assert _all_zero(f.get_image_display(0, F))
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(0)
    assert e.value.rc == -5
    f.run_images(0, F)
    assert not _all_zero(f.get_image_display(0, F))
    assert _rows(f.get_image_display(F - 1, 1), keys=VIEW) == _view(f)
    f.close()
    # ... and behind fresh match patches the run after a restage is its twin's
    g = _filter(srukf, cs, F); g.images_display(True)
    g.stage_sequence(cs["odo"][:F + 1], *zeros); g.stage_images(cs["frames"][:F])
    g.run_images(0, F)
    assert _rows(g.get_image_display(0, F)) == twin
    # reset drops the record with the images; the switch survives
    g.reset()
    with pytest.raises(srukf.SrukfError) as e: g.get_image_display(0, F)
    assert e.value.rc == -5
    g.set_state(cs["X1"], cs["S1"])
    g.stage_sequence(cs["odo"][:F + 1], *zeros); g.stage_images(cs["frames"][:F])
    assert _all_zero(g.get_image_display(0, F))
    g.run_images(0, F)
    assert not _all_zero(g.get_image_display(0, F)) and _rows(g.get_image_display(F - 1, 1), keys=VIEW) == _view(g)
    # a map change drops it too; the switch survives on the smaller map
    g.delete_landmark(0)
    with pytest.raises(srukf.SrukfError) as e: g.get_image_display(0, F)
    assert e.value.rc == -5
    M = N - 1
    g.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 2 * M)), np.zeros((F, M), dtype=np.int32)); g.stage_images(cs["frames"][:F])
    rec = g.get_image_display(0, F)
    assert rec["xyz"].shape == (F, M, 3) and _all_zero(rec)
    g.run_images(0, 2)
    rec = g.get_image_display(0, F)
    assert not _all_zero({k: rec[k][:2] for k in KEYS}) and _all_zero({k: rec[k][2:] for k in KEYS})
    assert _rows(rec, 1, 2, VIEW) == _view(g)
    g.close()
    h = srukf.Filter(N, cs["p"]); h.set_state(cs["X1"], cs["S1"])
    with pytest.raises(srukf.SrukfError) as e: h.get_image_display(0, 1)      # no staged images
    assert e.value.rc == -5
    with pytest.raises(srukf.SrukfError) as e: h.render_image_overlay(0)
    assert e.value.rc == -5
    h.close()


# ---- 9. sizes where the shared bodies can go wrong ----
def test_two_panels_at_33_landmarks(srukf, synth):
    cs = _case(srukf, synth, 33)

    def make(display):
        f = _filter(srukf, cs, 3)
        f.images_display(display)
        return f

    for mode_name in MODES:
        rec = _against_fresh(make, (0, 2), _mode(srukf, mode_name), staged=3)
        assert (np.abs(rec["Si"]).max(axis=(2, 3)) > 0).any()


def test_second_trip_of_the_cartesian_body_at_172_landmarks(srukf, synth):
    """N = 172, no appearance records (the frames update nothing: the view is the predicted state's), 2 frames.  Landmarks 170 and 171 take the second 1 024-row
    trip of the Cartesian body (rows 1 020 .. 1 031), the ellipsoid launch has a partial third workgroup, the robot block sits at row 1 032.  Seed 13 (the
    scene's own) is asserted clean on the reference handle."""
    N, F = 172, 2
    cs = _case(srukf, synth, N)

    def make(display):
        f = _filter(srukf, cs, F, appearance=False)
        f.images_display(display)
        return f

    g = make(False)
    g.run_images(0, F)
    assert g.clamp_info() == (-1, -1)                            # a condition on the reference handle alone
    g.close()
    rec = _against_fresh(make, (0, 1), srukf.UPDATE_BATCHED, staged=F)
    assert np.isfinite(rec["cov"][:, 170:]).all() and (rec["cov"][:, 170:, 0, 0] > 0).all()
    assert rec["rot"].shape == (F, N) and (rec["rot"][:, 128:] >= 0).all()


# ---- 10. the overlay ----
def _reference_overlay(srukf, cs, gray, h, Si, z, matched):
    """render_overlay on a second handle that holds the frame as a colour frame (the fixed-point conversion maps (g, g, g) to g), fed from the host"""
    r = srukf.Filter(cs["N"], cs["p"])
    bgr = np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))
    back = r.set_frame_bgr(bgr)
    assert np.array_equal(back, gray)
    out = r.render_overlay(h, Si, z, matched)
    r.close()
    return out, bgr


@pytest.mark.parametrize("mode_name", MODES)
def test_overlay_of_a_staged_frame(srukf, synth, mode_name):
    F = 6
    cs = _case(srukf, synth, 8)
    f = _filter(srukf, cs, F)
    f.images_display(True)
    f.run_images(0, F, mode=_mode(srukf, mode_name))
    before = _state_bytes(f) + (_patch_bytes(f),)
    for t in (0, 5):
        got = f.render_image_overlay(t)
        m, d = f.get_image_matches(t, 1), f.get_image_display(t, 1)
        assert m["matched"][0].sum() >= 3
        want, bare = _reference_overlay(srukf, cs, cs["frames"][t], m["h"][0], d["Si"][0], m["z"][0], m["matched"][0])
        assert got.tobytes() == want.tobytes(), t
        assert got.tobytes() != bare.tobytes(), "nothing was drawn"
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    f.close()


def test_overlay_draws_the_masked_set_after_a_consensus_run(srukf, synth):
    F, t = 6, 0
    f = _ransac_filter(srukf, synth, "outlier", F, THR)
    f.images_display(True)
    f.run_images(0, F)
    got = f.render_image_overlay(t)
    m, d, r = f.get_image_matches(t, 1), f.get_image_display(t, 1), f.get_image_ransac(t, 1)
    f.close()
    masked = m["matched"][0]
    assert (r["flags"][0][OUT_LM] & 1) and masked[OUT_LM] == 0 and masked.sum() >= 2      # the displaced landmark matched and the consensus dropped it
    cs = _case(srukf, synth, 8)
    want, bare = _reference_overlay(srukf, cs, cs["frames"][t], m["h"][0], d["Si"][0], m["z"][0], masked)
    assert got.tobytes() == want.tobytes() and got.tobytes() != bare.tobytes()
    raw = masked.copy(); raw[OUT_LM] = 1
    other, _ = _reference_overlay(srukf, cs, cs["frames"][t], m["h"][0], d["Si"][0], m["z"][0], raw)
    assert other.tobytes() != got.tobytes()                      # with the association's own row the dropped landmark would have been drawn
