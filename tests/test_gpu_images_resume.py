"""GPU tests of the state kept at a block's stop (srukf_images_snapshots / srukf_get_image_snapshots / srukf_images_resume, k_image_snapshot;
csrc/srukf_snapshot.hip, srukf_images.hip).  The yardstick is the library's own rewind-and-rerun route: after images_resume(keep) the handle
must hold, byte for byte, what a fresh filter's run of the first `keep` frames leaves (which tests/test_gpu_policy.py holds images_rewind + run to).

Scenes and helpers: tests/test_gpu_images.py's (N = 8, 640 x 480, at most 11 staged frames), tests/test_gpu_policy.py's seeded policy (first_change == 2 with the
defaults, 1 with min_predictions 9) and tests/test_gpu_images_ransac.py's outlier scene (first_outlier == 0 at 4.8 px).  The outlier stop inside a block uses the
clean scene: its own matches drift from hypothesis to hypothesis by 2.8 px (frame 0) to 4.5 px (frame 5), so a threshold halfway between the largest distance of
frames 0 .. k - 1 and the largest of frame k makes frame k the first with an outlier.  Everything is compared as bytes."""
import functools

import numpy as np
import pytest

import test_gpu_images_ransac as gir
from test_gpu_images import F_MAX, NO_RECORD, _case, _filter, _patch_bytes, _record_bytes, _state_bytes
from test_gpu_policy import NEUTRAL, PAR, _policy_filter, _seed
from test_gpu_images_ransac import THR, _ransac_bytes, _ransac_filter

pytestmark = pytest.mark.gpu

MODES = ["BATCHED", "JOINT"]
POL_ROWS = ("verdict", "summary")
RS_ROWS = ("flags", "votes", "dist", "best", "n_active", "n_low")


def _run(f, first, count, mode, checked=False):
    return f.run_images_checked(first, count, mode=mode, **NEUTRAL) if checked else f.run_images(first, count, mode=mode)


def _held(f, keep, policy=False, ransac=False):
    """what the handle holds for the first `keep` frames: X, S, matchPatches, rows < keep of the match record and of the records switched on, the policy state"""
    out = _state_bytes(f) + (_patch_bytes(f),) + _record_bytes(f.get_image_matches(0, keep))
    if policy:
        r = f.get_image_policy(0, keep)
        out += (r["verdict"].tobytes(), r["summary"].tobytes(), r["state"].tobytes(), r["first_change"])
    if ransac:
        out += _ransac_bytes(f.get_image_ransac(0, keep))
    return out


def _rows_zero(f, first, count, policy=False, ransac=False):
    if count < 1: return True
    ok = True
    if policy:
        r = f.get_image_policy(first, count)
        ok = ok and not r["verdict"].any() and not any(r["summary"][k].any() for k in r["summary"].dtype.names) and r["first_change"] == -1
    if ransac:
        r = f.get_image_ransac(first, count)
        ok = ok and not any(r[k].any() for k in RS_ROWS) and r["first_outlier"] == -1
    return ok


def _mode(srukf, name):
    return getattr(srukf, "UPDATE_" + name)


# ---- 1. / 2. a policy stop: the odd slot, the even slot ----
@pytest.mark.parametrize("checked", [False, True])
@pytest.mark.parametrize("mode_name", MODES)
def test_policy_stop_odd_slot(srukf, synth, mode_name, checked):
    """first_change == 2: three frames are kept, slot 1 holds the state frame 3 started from"""
    F, keep, mode = 6, 3, _mode(srukf, mode_name)
    f = _policy_filter(srukf, synth, F)
    f.images_snapshots(True)
    t = _run(f, 0, F, mode, checked)
    assert f.get_image_policy(0, F)["first_change"] == 2
    tags = f.get_image_snapshots()
    print("tags", tags)
    assert 3 in tags and tags[1] == 3
    after6 = _state_bytes(f)
    f.images_resume(keep)
    got = (t[:keep].tobytes(),) + _held(f, keep, policy=True)
    assert _rows_zero(f, keep, F - keep, policy=True)
    f.close()
    g = _policy_filter(srukf, synth, F)
    t = _run(g, 0, keep, mode, checked)
    want = (t.tobytes(),) + _held(g, keep, policy=True)
    g.close()
    assert len(got) == len(want) and got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert got[1:3] != after6 and got[1] != after6[0] and got[2] != after6[1]


@pytest.mark.parametrize("mode_name", MODES)
def test_policy_stop_even_slot(srukf, synth, mode_name):
    """min_predictions 9: first_change == 1, two frames are kept, slot 0 holds the state frame 2 started from"""
    F, keep, mode = 6, 2, _mode(srukf, mode_name)
    f = _policy_filter(srukf, synth, F, min_predictions=9)
    f.images_snapshots(True)
    t = f.run_images(0, F, mode=mode)
    assert f.get_image_policy(0, F)["first_change"] == 1
    assert f.get_image_snapshots()[0] == 2
    f.images_resume(keep)
    got = (t[:keep].tobytes(),) + _held(f, keep, policy=True)
    assert _rows_zero(f, keep, F - keep, policy=True)
    f.close()
    g = _policy_filter(srukf, synth, F, min_predictions=9)
    t = g.run_images(0, keep, mode=mode)
    want = (t.tobytes(),) + _held(g, keep, policy=True)
    g.close()
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


# ---- 3. an outlier stop in front of a frame ----
@functools.lru_cache(maxsize=None)
def _outlier_threshold(srukf, synth, mode):
    """(k, threshold): the clean scene's largest distance per frame under a threshold nothing fails; k >= 2 the first frame that exceeds every frame before it by
    more than 1e-3 px, the threshold halfway"""
    F = 6
    f = _ransac_filter(srukf, synth, "clean", F, 1000.0)
    f.run_images(0, F, mode=mode)
    r = f.get_image_ransac(0, F)
    f.close()
    assert r["first_outlier"] == -1 and (r["n_active"] >= 2).all()
    mx = r["dist"].max(axis=1)
    print("largest distance per frame:", np.round(mx, 4).tolist())
    ks = [k for k in range(2, F) if mx[k] > mx[:k].max()]
    assert ks, mx
    k = ks[0]
    assert mx[k] - mx[:k].max() > 1e-3, mx                       # precondition of the scene: asserted, not skipped
    return k, 0.5 * (mx[k] + mx[:k].max())


@pytest.mark.parametrize("mode_name", MODES)
def test_outlier_stop_in_front_of_a_frame(srukf, synth, mode_name):
    F, mode = 6, _mode(srukf, mode_name)
    k, thr = _outlier_threshold(srukf, synth, mode)
    f = _ransac_filter(srukf, synth, "clean", F, thr)
    f.images_snapshots(True)
    t = f.run_images(0, F, mode=mode)
    fo = f.get_image_ransac(0, F)["first_outlier"]
    tags = f.get_image_snapshots()
    print("k %d threshold %.4f first_outlier %d tags %s" % (k, thr, fo, tags))
    assert fo == k                                               # precondition: asserted, not skipped
    assert tags[k & 1] == k and tags[(k - 1) & 1] == k - 1       # the other slot was not overwritten two frames later
    f.images_resume(k)
    got = (t[:k].tobytes(),) + _held(f, k, ransac=True)
    assert _rows_zero(f, k, F - k, ransac=True)
    f.close()
    g = _ransac_filter(srukf, synth, "clean", F, thr)
    t = g.run_images(0, k, mode=mode)
    want = (t.tobytes(),) + _held(g, k, ransac=True)
    g.close()
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


def test_outlier_in_the_first_frame_resume_is_rewind(srukf, synth):
    """the outlier scene at 4.8 px: first_outlier == 0; images_resume(0) leaves what images_rewind leaves"""
    F = 6
    res = []
    for name in ("resume", "rewind"):
        f = _ransac_filter(srukf, synth, "outlier", F, THR)
        f.images_snapshots(True)
        start = _state_bytes(f) + (_patch_bytes(f),)
        f.run_images(0, F)
        assert f.get_image_ransac(0, F)["first_outlier"] == 0
        assert f.get_image_snapshots() == (0, -1)
        if name == "resume": f.images_resume(0)
        else: f.images_rewind()
        now = _state_bytes(f) + (_patch_bytes(f),)
        assert now == start
        assert _rows_zero(f, 0, F, ransac=True)
        res.append(now + _record_bytes(f.get_image_matches(0, F)))
        with pytest.raises(srukf.SrukfError) as e: f.images_rewind()      # one resume or one rewind per block
        assert e.value.rc == -5
        f.close()
    assert res[0] == res[1]


# ---- 4. both stops in one block ----
@pytest.mark.parametrize("mode_name,kw", [("BATCHED", {}), ("JOINT", {}), ("BATCHED", dict(min_predictions=9))])
def test_both_stops_in_one_block(srukf, synth, mode_name, kw):
    F, mode = 6, _mode(srukf, mode_name)
    k, thr = _outlier_threshold(srukf, synth, mode)

    def make():
        h = _policy_filter(srukf, synth, F, **kw)
        h.images_ransac(True, thr)
        return h

    f = make()
    f.images_snapshots(True)
    t = f.run_images(0, F, mode=mode)
    fc, fo = f.get_image_policy(0, F)["first_change"], f.get_image_ransac(0, F)["first_outlier"]
    assert fc >= 0 and fo >= 0, (fc, fo)
    stop = min(fc + 1, fo)
    tags = f.get_image_snapshots()
    print("first_change %d first_outlier %d stop %d tags %s" % (fc, fo, stop, tags))
    assert 0 < stop < F and tags[stop & 1] == stop
    f.images_resume(stop)
    got = (t[:stop].tobytes(),) + _held(f, stop, policy=True, ransac=True)
    assert _rows_zero(f, stop, F - stop, policy=True, ransac=True)
    f.close()
    g = make()
    t = g.run_images(0, stop, mode=mode)
    want = (t.tobytes(),) + _held(g, stop, policy=True, ransac=True)
    g.close()
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


# ---- 5. graph forms and split blocks ----
@pytest.mark.parametrize("mode_name", MODES)
def test_graph_forms_and_a_split_block_leave_the_same_bytes(srukf, synth, mode_name):
    F, keep, mode = 6, 3, _mode(srukf, mode_name)
    res = []
    for name in ("default", "eager", "split"):
        f = _policy_filter(srukf, synth, F, graph=0 if name == "eager" else None)
        f.images_snapshots(True)
        if name == "split":
            f.run_images_async(0, 2, mode=mode); f.run_images_async(2, 4, mode=mode); f.synchronize()      # one block, the stop in its second run
        else:
            f.run_images(0, F, mode=mode)
        assert f.get_image_policy(0, F)["first_change"] == 2 and f.get_image_snapshots()[1] == 3, name
        f.images_resume(keep)
        res.append(_held(f, keep, policy=True))
        assert _rows_zero(f, keep, F - keep, policy=True), name
        f.close()
    g = _policy_filter(srukf, synth, F)
    g.run_images(0, keep, mode=mode)
    want = _held(g, keep, policy=True)
    g.close()
    for name, got in zip(("default", "eager", "split"), res):
        assert got == want, (name, [i for i, (a, b) in enumerate(zip(got, want)) if a != b])


@pytest.mark.parametrize("ransac", [False, True])
def test_eleven_frames_stop_behind_frame_nine(srukf, synth, ransac):
    """an eight-frame graph, then single frames: the slots hold the starts of frames 9 and 10; ten frames are kept.  ransac: the consensus' frames (a threshold
    nothing fails), whose captured frames are others"""
    F, keep = F_MAX, 10
    cs = _case(srukf, synth, 8)

    def make():
        h = _filter(srukf, cs, F)
        if ransac: h.images_ransac(True, 1000.0)
        return h

    f = make()
    f.images_snapshots(True)
    t = f.run_images(0, F)
    assert f.clamp_info() == (-1, -1)
    assert f.get_image_snapshots() == (10, 9)
    after = _state_bytes(f)
    f.images_resume(keep)
    got = (t[:keep].tobytes(),) + _held(f, keep, ransac=ransac)
    assert _rows_zero(f, keep, 1, ransac=ransac)
    f.close()
    g = make()
    t = g.run_images(0, keep)
    want = (t.tobytes(),) + _held(g, keep, ransac=ransac)
    g.close()
    assert got == want and got[1:3] != after


# ---- 6. read-only ----
@pytest.mark.parametrize("policy,ransac", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("mode_name", MODES)
def test_snapshots_are_read_only(srukf, synth, mode_name, policy, ransac):
    """11 frames with the switch on against the switch off: trajectory, X, S, every record, every matchPatch"""
    F, mode = F_MAX, _mode(srukf, mode_name)
    res = []
    for on in (False, True):
        f = _filter(srukf, _case(srukf, synth, 8), F)
        if policy: f.images_policy(True, **PAR); f.set_policy_state(_seed())
        if ransac: f.images_ransac(True, THR)
        f.images_snapshots(on)
        t = f.run_images(0, F, mode=mode)
        assert f.clamp_info() == (-1, -1)
        res.append((t.tobytes(),) + _held(f, F, policy=policy, ransac=ransac))
        assert f.get_image_snapshots() == (-1, -1) or on
        f.close()
    assert res[0] == res[1], [i for i, (a, b) in enumerate(zip(*res)) if a != b]


# ---- 7. no stop ----
@pytest.mark.parametrize("mode_name", MODES)
def test_block_without_a_stop(srukf, synth, mode_name):
    F, mode = 6, _mode(srukf, mode_name)
    cs = _case(srukf, synth, 8)
    f = _filter(srukf, cs, F)
    f.images_snapshots(True)
    t = f.run_images(0, F, mode=mode)
    assert sorted(f.get_image_snapshots()) == [4, 5]
    before = _held(f, F)
    f.images_resume(6)                                           # nothing moves ...
    assert _held(f, F) == before
    with pytest.raises(srukf.SrukfError) as e: f.images_resume(3)      # ... no slot holds frame 3 ...
    assert e.value.rc == -5 and _held(f, F) == before
    f.images_resume(5)                                           # ... and the block can still be cut
    got = (t[:5].tobytes(),) + _held(f, 5)
    f.close()
    g = _filter(srukf, cs, F)
    t5 = g.run_images(0, 5, mode=mode)
    want = (t5.tobytes(),) + _held(g, 5)
    g.close()
    assert got == want and got[1:3] != before[0:2]
    # a refused resume leaves the rewind
    f = _filter(srukf, cs, F)
    f.images_snapshots(True)
    start = _state_bytes(f) + (_patch_bytes(f),)
    f.run_images(0, F, mode=mode)
    with pytest.raises(srukf.SrukfError) as e: f.images_resume(3)
    assert e.value.rc == -5
    f.images_rewind()
    assert _state_bytes(f) + (_patch_bytes(f),) == start
    f.close()


# ---- 8. refusals ----
def test_resume_refusals(srukf, synth):
    """every situation that refuses a rewind refuses a resume (tests/test_gpu_policy.py's test_rewind_refusals), and the resume's own"""
    cs = _case(srukf, synth, 8)
    f = _policy_filter(srukf, synth, 6)
    f.images_snapshots(True)

    def refused(keep=1, rc=-5):
        before = _state_bytes(f)
        with pytest.raises(srukf.SrukfError) as e: f.images_resume(keep)
        assert e.value.rc == rc, str(e.value)
        assert _state_bytes(f) == before

    refused()                                                    # no image block has been synchronised
    f.run_images_async(0, 3)
    with pytest.raises(srukf.SrukfError) as e: f.images_resume(1)      # a run is pending
    assert e.value.rc == -5
    for on in (False, True):
        with pytest.raises(srukf.SrukfError) as e: f.images_snapshots(on)      # no switch change with a run in flight
        assert e.value.rc == -5
    f.synchronize()
    f.predict_motion(cs["odo"][3], cs["odo"][4])
    refused()
    f.predict_measurement(); z, m, _ = f.associate(cs["frames"][3]); f.update(z, m)
    refused()                                                    # a step-wise frame
    f.run_images(0, 3)
    X, S = f.get_state()
    f.set_state(X, S)
    refused()
    f.run_images(0, 2)
    f.run_frames(2, 1)
    refused()
    f.run_images(0, 2)
    f.set_policy_state(_seed())                                  # a seed is not in the slots
    refused()
    f.run_images(0, 2)                                           # (two frames: whatever the policy says by now, slot 1 holds frame 1)
    refused(3, -1)                                               # keep beyond the frames the block ran
    assert f._lib.srukf_images_resume(f._h, -1) == -1
    f.images_resume(1)
    refused()                                                    # a second time
    with pytest.raises(srukf.SrukfError) as e: f.images_rewind()  # rewind after resume
    assert e.value.rc == -5
    f.run_images(0, 3)
    f.images_rewind()
    refused()                                                    # resume after rewind
    # the switch off during the block
    f.images_snapshots(False)
    f.run_images(0, 3)
    refused()
    refused(2)
    f.images_rewind()                                            # (the refusal left the block as it was)
    # ... during one of its runs
    f.images_snapshots(True)
    f.run_images(0, 2)
    f.images_resume(1)
    f.close()


# ---- 9. lifetime ----
def test_lifetime(srukf, synth):
    from test_gpu_unique import _rot
    cs = _case(srukf, synth, 8)
    F = 4

    def block(f, N=8):
        t = f.run_images(0, 3)
        assert f.get_image_snapshots() == (2, 1)
        f.images_resume(2)
        return (t[:2].tobytes(),) + _held(f, 2)

    f = _filter(srukf, cs, F)
    f.images_snapshots(True)
    first = block(f)
    # a restage drops the slots
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 16)), np.zeros((F, 8), dtype=np.int32))
    f.stage_images(cs["frames"][:F])
    assert f.get_image_snapshots() == (-1, -1)
    # reset drops them, the switch survives, the next block works and is the first one again
    f.reset()
    assert f.get_image_snapshots() == (-1, -1)
    f.set_state(cs["X1"], cs["S1"])
    for k, (patch, px) in enumerate(cs["recs"]):
        if k != NO_RECORD: f.set_landmark_appearance(k, patch, _rot(cs["pose"][3]), cs["pose"][:3], px)
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 16)), np.zeros((F, 8), dtype=np.int32))
    f.stage_images(cs["frames"][:F])
    assert block(f) == first
    # a map change drops them, the switch survives, the next block works
    f.delete_landmark(0)
    assert f.get_image_snapshots() == (-1, -1)
    with pytest.raises(srukf.SrukfError) as e: f.images_resume(1)
    assert e.value.rc == -5
    N = 7
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 2 * N)), np.zeros((F, N), dtype=np.int32))
    f.stage_images(cs["frames"][:F])
    got = block(f)
    f.close()
    g = _filter(srukf, cs, F)                                    # (the same history without the switch: two frames, the map change, two frames)
    g.run_images(0, 2)
    g.delete_landmark(0)
    g.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 2 * N)), np.zeros((F, N), dtype=np.int32))
    g.stage_images(cs["frames"][:F])
    t = g.run_images(0, 2)
    assert got == (t.tobytes(),) + _held(g, 2)
    g.close()


def test_flagged_block_is_restored_and_refuses_a_resume(srukf, synth):
    """the shipped a1 .. a4 = 8 (tests/test_gpu_images.py) with the switch on: SRUKF_ERR_CLAMP_PENDING, the seed state is back, a resume is refused"""
    F = 6
    f = _filter(srukf, _case(srukf, synth, 8, "shipped"), F)
    f.images_snapshots(True)
    before = _state_bytes(f) + (_patch_bytes(f),)
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, F)
    assert e.value.rc == -7, str(e.value)
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    for keep in (0, 1, F):
        with pytest.raises(srukf.SrukfError) as e: f.images_resume(keep)
        assert e.value.rc == -5
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    f.close()


# ---- 10. forms on one handle ----
@pytest.mark.parametrize("mode_name", MODES)
def test_every_form_with_and_without_the_bit_on_one_handle(srukf, synth, mode_name):
    """tests/test_gpu_images_ransac.py's test_every_form_on_one_handle_is_the_fresh_handles with the fourth bit: the eight combinations of checked, search and
    ransac, each run with the snapshot bit on and then off on ONE handle, leave what a fresh handle that runs only that form leaves — no frame captured with the
    snapshot launch is replayed for a form without it, nor the other way round — and the slots hold the last two frames of the runs with the bit"""
    mode = _mode(srukf, mode_name)
    f = gir._form_filter(srukf, synth)
    for form in gir.FORM_ORDER:
        want = gir._fresh_form(srukf, synth, form, mode)
        for snap in (True, False, True):
            f.images_snapshots(snap)
            got = gir._form_run(srukf, synth, f, form, mode)
            assert len(got) == len(want) and got == want, (form, snap, [i for i, (a, b) in enumerate(zip(got, want)) if a != b])
            if snap:
                tags = f.get_image_snapshots()
                # (an outlier frame in front closes the slots: the forms with the consensus stop at frame 0 of this scene)
                assert tags == ((0, -1) if form & 4 else (8, 7)), (form, tags)
    f.close()
