"""GPU tests of colour frames in the staged stack and of the overlays of a run of frames (srukf_stage_images_bgr / srukf_get_staged_image /
srukf_render_image_overlays, k_overlay_prep_block / k_overlay_block; csrc/srukf_images.hip, srukf_overlay.hip).  Every comparison is byte
equality.  The yardsticks: tests/np_overlay.gray, the restatement §15 holds the device's conversion to, and the library's own gray-staged route — a handle staged
with stage_images(np_overlay.gray(bgr)) must be indistinguishable from one staged with stage_images_bgr(bgr).

Scenes: tests/test_gpu_images.py's case (N = 8, 640 x 480, 6 staged frames) with colour frames whose B, G and R are its texture rolled by three different
offsets (the appearance records are cut again from the converted first frame, as tests/test_gpu_images_checked.py cuts its own); tests/test_gpu_policy.py's seeded
policy scene for a block cut by images_resume; tests/test_gpu_images_display.py's N = 172 case for three compaction chunks of the raster; the contexts of
tests/test_gpu_overlay.py at 9 x 9, 71 x 51 and 70 x 50 for the conversion where frames of the tight stack start at every offset mod 4, and two stacks of
more than 2^22 pixels (640 x 480 x 15, 641 x 481 x 14) for the second chunk of the staging."""
import ctypes as C
import functools

import numpy as np
import pytest

import np_overlay as OV
from test_gpu_detect import params
from test_gpu_images import NO_RECORD, WRONG_RECORD, _case, _filter, _patch_bytes, _record_bytes, _state_bytes
from test_gpu_images_display import KEYS, _rows
from test_gpu_policy import NEUTRAL, _policy_filter

pytestmark = pytest.mark.gpu

MODES = ["BATCHED", "JOINT"]
F6 = 6
ROLLS = ((0, 0), (3, 5), (-4, 2))                               # (rows, columns) the texture is rolled by in B, G, R


def _colour_of(frames):
    """[F, H, W] gray -> [F, H, W, 3]: channel c is the frame rolled by ROLLS[c]"""
    return np.ascontiguousarray(np.stack([np.roll(frames, r, axis=(1, 2)) for r in ROLLS], axis=-1))


def _gray_of(bgr):
    return np.ascontiguousarray(np.stack([OV.gray(b) for b in bgr]))


@functools.lru_cache(maxsize=None)
def _colour_case(srukf, synth, N=8, which="scene"):
    """test_gpu_images._case with colour frames: cs["bgr"], cs["frames"] = their conversion, the records cut from the converted first frame"""
    cs = dict(_case(srukf, synth, N, which))
    bgr = _colour_of(cs["frames"])
    gray = _gray_of(bgr)
    assert (gray != cs["frames"]).mean() > 0.5 and (bgr[..., 0] != bgr[..., 2]).mean() > 0.5      # the channels differ, and the blend is no channel's bytes
    recs = []
    for k, (patch, px) in enumerate(cs["recs"]):
        cu, cv = int(px[0]), int(px[1])
        recs.append((patch if k == WRONG_RECORD else gray[0][cv - 10:cv + 11, cu - 10:cu + 11].copy(), px))
    cs["bgr"], cs["frames"], cs["recs"] = bgr, gray, recs
    return cs


def _staged(srukf, cs, F, how, display=False, appearance=True):
    """a filter at the case's start state with F frames staged: how = "gray" (stage_images of the converted frames), 0 or 1 (stage_images_bgr, keep_colour)"""
    f = _filter(srukf, cs, appearance=appearance)
    N = cs["N"]
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 2 * N)), np.zeros((F, N), dtype=np.int32))
    if how == "gray": f.stage_images(cs["frames"][:F])
    else: f.stage_images_bgr(cs["bgr"][:F], keep_colour=bool(how))
    if display: f.images_display(True)
    return f


def _mode(srukf, name):
    return getattr(srukf, "UPDATE_" + name)


def _run(f, first, count, mode, checked=False):
    return f.run_images_checked(first, count, mode=mode, **NEUTRAL) if checked else f.run_images(first, count, mode=mode)


# ---- 1. the conversion at the sizes where it can go wrong ----
def _random_colour(seed, F, H, W):
    bgr = np.random.default_rng(seed).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)
    bgr[0, 0, 0] = (255, 0, 0); bgr[-1, -1, -1] = (0, 0, 255)
    return bgr


def test_restatement_tells_the_channels_apart():
    """on the CPU: the comparison below is not vacuous — the weight of channel 0 is not that of channel 2"""
    bgr = _random_colour(7, 2, 9, 9)
    g, s = _gray_of(bgr), _gray_of(np.ascontiguousarray(bgr[..., ::-1]))
    assert (g != s).mean() > 0.5
    assert g[0, 0, 0] == 76 and g[-1, -1, -1] == 29
    assert OV.gray(np.array([[[255, 0, 0]]], dtype=np.uint8))[0, 0] == 76 and OV.gray(np.array([[[0, 0, 255]]], dtype=np.uint8))[0, 0] == 29


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("W,H,F", [(9, 9, 5), (71, 51, 5), (70, 50, 3), (640, 480, 2), (640, 480, 15), (641, 481, 14)])
def test_conversion_of_a_stack(srukf, synth, W, H, F, keep):
    """9 x 9 and 71 x 51: W H = 1 (mod 4), frames start at byte offsets 0, 1, 2, 3, 0 (mod 4) of the gray stack; 71 x 51 is more than one workgroup.  Every
    frame read back in ascending and in descending order: a byte clobbered across a frame boundary shows in either.  640 x 480 x 15 (4 608 000 pixels) and
    641 x 481 x 14 (4 316 494) exceed the staging's chunk of 2^22 pixels: the second chunk's offsets into both stacks, the transit buffer's second use (keep
    False) and, at 641 x 481 (308 321 = 1 mod 4), frames at every offset mod 4 with the chunk boundary inside frame 13 and a partial last group behind it"""
    assert (W * H * F > 1 << 22) == (F > 5)
    bgr = _random_colour(1000 + W, F, H, W)
    want = _gray_of(bgr)
    assert (want != _gray_of(np.ascontiguousarray(bgr[..., ::-1]))).mean() > 0.5 and want[0, 0, 0] == 76 and want[-1, -1, -1] == 29
    f = srukf.Filter(1, params(synth, W, H))
    f.stage_sequence(np.zeros((F + 1, 3)), np.zeros((F, 2)), np.zeros((F, 1), dtype=np.int32))
    f.stage_images_bgr(bgr, keep_colour=keep)
    for order in (range(F), reversed(range(F))):
        for t in order:
            if keep:
                g, c = f.get_staged_image(t, want_bgr=True)
                assert np.array_equal(c, bgr[t]), (t, np.argwhere((c != bgr[t]).any(axis=2))[:5])
            else:
                g = f.get_staged_image(t)
            assert np.array_equal(g, want[t]), (t, np.argwhere(g != want[t])[:5])
    if not keep:
        with pytest.raises(srukf.SrukfError) as e: f.get_staged_image(0, want_bgr=True)
        assert e.value.rc == -5
    with pytest.raises(srukf.SrukfError) as e: f.get_staged_image(F)
    assert e.value.rc == -1
    f.close()


# ---- 2. an image run on colour frames ----
@functools.lru_cache(maxsize=None)
def _run_bytes(srukf, synth, how, mode_name, checked):
    """everything a 6-frame run with the display switch on leaves, as bytes"""
    cs = _colour_case(srukf, synth)
    f = _staged(srukf, cs, F6, how, display=True)
    traj = _run(f, 0, F6, _mode(srukf, mode_name), checked)
    assert f.clamp_info() == (-1, -1)
    rec = f.get_image_matches(0, F6)
    out = (traj.tobytes(),) + _state_bytes(f) + _record_bytes(rec) + _rows(f.get_image_display(0, F6)) + (_patch_bytes(f),)
    if checked: out += tuple(f.get_image_checks(0, F6)[k].tobytes() for k in ("corr2", "z2", "flags"))
    out += tuple(f.get_staged_image(t).tobytes() for t in range(F6))
    f.close()
    return out, rec["matched"].sum(axis=1)


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("checked", [False, True])
@pytest.mark.parametrize("mode_name", MODES)
def test_run_on_colour_frames_is_the_gray_staged_run(srukf, synth, mode_name, checked, keep):
    want, matches = _run_bytes(srukf, synth, "gray", mode_name, checked)
    assert (matches >= 3).all(), matches                          # a condition on the gray-staged run alone
    got, _ = _run_bytes(srukf, synth, keep, mode_name, checked)
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


def test_held_frame_is_neither_read_nor_written(srukf, synth):
    cs = _colour_case(srukf, synth)
    N = cs["N"]
    held = np.ascontiguousarray(cs["bgr"][3][:, ::-1])           # a frame that is none of the staged ones
    nothing = (np.zeros(2 * N), np.zeros(4 * N), np.zeros(2 * N), np.zeros(N, dtype=np.int32))

    def associate(f):
        f.set_state(cs["X1"], cs["S1"])
        f.predict_motion(cs["odo"][0], cs["odo"][1]); f.predict_measurement()
        return f.associate_held()

    f = _filter(srukf, cs)
    f.set_frame_bgr(held)
    before = associate(f)
    for keep in (True, False):
        f.stage_sequence(cs["odo"][:F6 + 1], np.zeros((F6, 2 * N)), np.zeros((F6, N), dtype=np.int32))
        f.stage_images_bgr(cs["bgr"][:F6], keep_colour=keep)
        assert np.array_equal(f.get_staged_image(2), cs["frames"][2])
        assert np.array_equal(f.render_overlay(*nothing), held)
        after = associate(f)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    f.close()


# ---- 3. the overlay's source ----
def _reference_overlay(srukf, cs, bgr, h, Si, z, matched):
    """render_overlay on a second handle that holds the colour frame through set_frame_bgr, fed the record's rows from the host (DESIGN.md §26's construction)"""
    r = srukf.Filter(cs["N"], cs["p"])
    r.set_frame_bgr(np.ascontiguousarray(bgr), want_gray=False)
    out = r.render_overlay(h, Si, z, matched)
    r.close()
    return out


@functools.lru_cache(maxsize=None)
def _gray_staged_overlays(srukf, synth, mode_name):
    f = _staged(srukf, _colour_case(srukf, synth), F6, "gray", display=True)
    f.run_images(0, F6, mode=_mode(srukf, mode_name))
    out = [f.render_image_overlay(t) for t in range(F6)]
    f.close()
    return out


@pytest.mark.parametrize("mode_name", MODES)
def test_overlay_source(srukf, synth, mode_name):
    cs = _colour_case(srukf, synth)
    gray_ov = _gray_staged_overlays(srukf, synth, mode_name)
    f = _staged(srukf, cs, F6, 1, display=True)
    f.run_images(0, F6, mode=_mode(srukf, mode_name))
    before = _state_bytes(f) + (_patch_bytes(f),)
    for t in (0, 5):
        got = f.render_image_overlay(t)
        m, d = f.get_image_matches(t, 1), f.get_image_display(t, 1)
        assert m["matched"][0].sum() >= 3
        want = _reference_overlay(srukf, cs, cs["bgr"][t], m["h"][0], d["Si"][0], m["z"][0], m["matched"][0])
        assert got.tobytes() == want.tobytes(), t
        assert got.tobytes() != cs["bgr"][t].tobytes(), "nothing was drawn"
        assert got.tobytes() != gray_ov[t].tobytes()
        unpainted = (got == cs["bgr"][t]).all(axis=2)
        assert 0 < (~unpainted).sum() < 0.05 * unpainted.size
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    f.close()
    f = _staged(srukf, cs, F6, 0, display=True)
    f.run_images(0, F6, mode=_mode(srukf, mode_name))
    for t in (0, 5):
        assert f.render_image_overlay(t).tobytes() == gray_ov[t].tobytes(), t
    f.close()


# ---- 4. the overlays of a run of frames ----
@pytest.mark.parametrize("how", ["gray", 1])
def test_block_overlay_is_the_single_calls_stacked(srukf, synth, how):
    cs = _colour_case(srukf, synth)
    f = _staged(srukf, cs, F6, how, display=True)
    f.run_images(0, F6)
    single = np.stack([f.render_image_overlay(t) for t in range(F6)])
    assert len({s.tobytes() for s in single}) == F6              # the six frames differ
    before = _state_bytes(f) + _record_bytes(f.get_image_matches(0, F6)) + _rows(f.get_image_display(0, F6)) + (_patch_bytes(f),)
    part = f.render_image_overlays(2, 3)                         # the smaller count first: the scratch grows behind it
    assert part.shape == (3, 480, 640, 3) and part.tobytes() == single[2:5].tobytes()
    whole = f.render_image_overlays(0, F6)
    assert whole.tobytes() == single.tobytes()
    assert f.render_image_overlays(5, 1).tobytes() == single[5:].tobytes()
    assert _state_bytes(f) + _record_bytes(f.get_image_matches(0, F6)) + _rows(f.get_image_display(0, F6)) + (_patch_bytes(f),) == before
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlays(4, 3)
    assert e.value.rc == -1
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlays(F6, 1)
    assert e.value.rc == -1
    f.close()


def test_block_overlay_at_172_landmarks(srukf, synth):
    """tests/test_gpu_images_display.py's N = 172 case: three prep workgroups per frame and three compaction chunks per tile"""
    N, F = 172, 2
    cs = _case(srukf, synth, N)
    f = _filter(srukf, cs, F, appearance=False)
    f.images_display(True)
    f.run_images(0, F)
    assert f.clamp_info() == (-1, -1)
    single = np.stack([f.render_image_overlay(t) for t in range(F)])
    assert f.render_image_overlays(0, F).tobytes() == single.tobytes()
    f.close()


def test_block_overlay_refuses_a_range_with_an_undrawable_row(srukf, synth):
    F, keep = 6, 3
    f = _policy_filter(srukf, synth, F)
    f.images_snapshots(True); f.images_display(True)
    f.run_images(0, F)
    f.images_resume(keep)
    assert f.render_image_overlays(0, keep).tobytes() == np.stack([f.render_image_overlay(t) for t in range(keep)]).tobytes()
    H, W = 480, 640
    out = np.full((F, H, W, 3), 0xA5, dtype=np.uint8)
    for first, count in ((0, F), (keep - 1, 2), (keep, 1)):
        assert f._lib.srukf_render_image_overlays(f._h, first, count, out.ctypes.data_as(C.POINTER(C.c_ubyte))) == -5
        assert (out == 0xA5).all()
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlays(0, F)
    assert e.value.rc == -5 and "frame %d" % keep in str(e.value)
    f.close()


# ---- 5. lifetime ----
def test_lifetime_of_the_colour_stack(srukf, synth):
    cs = _colour_case(srukf, synth)
    N = cs["N"]
    gray_ov = _gray_staged_overlays(srukf, synth, "BATCHED")
    f = _staged(srukf, cs, F6, 1, display=True)
    f.run_images(0, F6)
    assert f.render_image_overlay(1).tobytes() != gray_ov[1].tobytes()
    assert np.array_equal(f.get_staged_image(4, want_bgr=True)[1], cs["bgr"][4])
    # a later stage_images drops the colour stack: the getter refuses, the overlay is gray again
    f.set_state(cs["X1"], cs["S1"])
    f.stage_images(cs["frames"][:F6])
    assert np.array_equal(f.get_staged_image(4), cs["frames"][4])
    with pytest.raises(srukf.SrukfError) as e: f.get_staged_image(4, want_bgr=True)
    assert e.value.rc == -5
    f.close()
    f = _staged(srukf, cs, F6, 1, display=True)
    f.stage_images(cs["frames"][:F6])
    f.run_images(0, F6)
    assert f.render_image_overlay(1).tobytes() == gray_ov[1].tobytes()
    assert f.render_image_overlays(0, 2).tobytes() == np.stack(gray_ov[:2]).tobytes()
    # a map change drops both stacks
    f.stage_images_bgr(cs["bgr"][:F6], keep_colour=True)
    assert np.array_equal(f.get_staged_image(0, want_bgr=True)[1], cs["bgr"][0])
    f.delete_landmark(0)
    for want_bgr in (False, True):
        with pytest.raises(srukf.SrukfError) as e: f.get_staged_image(0, want_bgr=want_bgr)
        assert e.value.rc == -5
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlays(0, 1)
    assert e.value.rc == -5
    f.close()
    # nothing staged at all
    h = srukf.Filter(N, cs["p"]); h.set_state(cs["X1"], cs["S1"])
    with pytest.raises(srukf.SrukfError) as e: h.get_staged_image(0)
    assert e.value.rc == -5
    with pytest.raises(srukf.SrukfError) as e: h.stage_images_bgr(cs["bgr"][:F6])      # no staged sequence: stage_images' refusal
    assert e.value.rc == -5
    h.stage_sequence(cs["odo"][:F6 + 1], np.zeros((F6, 2 * N)), np.zeros((F6, N), dtype=np.int32))
    with pytest.raises(srukf.SrukfError) as e: h.stage_images_bgr(cs["bgr"][:F6 - 1])  # not the staged sequence's frame count
    assert e.value.rc == -2
    assert h._lib.srukf_stage_images_bgr(h._h, F6, cs["bgr"].ctypes.data_as(C.POINTER(C.c_ubyte)), 2) == -1
    h.close()


def test_flagged_block_leaves_the_stacks_readable(srukf, synth):
    """tests/test_gpu_images_display.py's flagged block (the shipped a1 ... a4 = 8), its gray frames staged as B = G = R colour frames: the conversion keeps such
    a frame byte for byte, so the block is the one that test sees flagged"""
    cs = dict(_case(srukf, synth, 8, "shipped"))
    cs["bgr"] = np.ascontiguousarray(np.repeat(cs["frames"][:, :, :, None], 3, axis=3))
    f = _staged(srukf, cs, F6, 1, display=True)
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F6)
    assert e.value.rc == -7, str(e.value)
    for t in (0, F6 - 1):
        g, c = f.get_staged_image(t, want_bgr=True)
        assert np.array_equal(g, cs["frames"][t]) and np.array_equal(c, cs["bgr"][t])
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(0)
    assert e.value.rc == -5
    with pytest.raises(srukf.SrukfError) as e: f.render_image_overlays(0, F6)
    assert e.value.rc == -5
    f.close()
