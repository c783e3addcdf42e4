"""GPU tests of the searching image runs (srukf_images_search_archive / srukf_get_image_archive, k_archive_search_staged; csrc/srukf_archive.hip, srukf_images.hip;
DESIGN.md §22): the archive search behind every frame of an image run, against the step-wise call srukf_archive_search made between the frames of a twin, bit for
bit; that it is read-only; across its graph forms, parameter values, a replaced archive, alternation with plain runs; its refusals; a flagged block.

Scene: tests/test_gpu_images.py's (N = 8, seed 13, the smooth texture of seed 17 rolled one pixel per frame over a robot that moves 1 cm per frame, 640 x 480, at
most 11 frames) with an archive of L = 5 records captured by tests/test_gpu_archive.py's capture_records from frame 0 at the pose of the first frame (its module
constant X4 holds that pose for the call: the scene's heading is 0.25 rad, and a record initialised from another pose projects 50 - 80 px from its patch):
  0, 1, 2  at (550, 200), (375, 375), (130, 200): >= 86 px from every landmark pixel; matched in every frame
  3        at (305, 200), its patch cut from the texture at rows / columns 100 .. 120: visible, never matched
  4        at (410, 130), its anchor moved 50 m aside: never visible
The search behind it, on the CPU (the oracle's filter through the 11 frames with oracle.warp_patch / associate_one as the association, tests/np_archive.py's predict /
warp / search on the posterior of every frame): of 154 candidate pixels on a 35-px grid, >= 40 px from every landmark pixel, 7 are matched in all 11 frames — the
reference's wrapPatch keeps a patch only in part of the view once the pose moves (tests/test_gpu_archive.py, LEFT_UV); the three with the largest margins were
taken: minimum corr over the 11 frames 0.8749, 0.8649, 0.8419 (threshold 0.8).  The cut record's corr stays in [0.495, 0.595]; the far record's 25 sigma pixels are
all zeroed.  Every comparison below is preceded by these conditions, asserted on the step-wise twin alone: a comparison of two all-zero records would show nothing.

Runs inside one block (between two srukf_synchronize) cannot differ in the switch — it is refused while an image run is in flight — so the alternation case
alternates synchronous runs over one staged stack."""
import functools

import numpy as np
import pytest

import test_gpu_archive as ga
from test_gpu_images import F_MAX, _case, _filter, _patch_bytes, _record_bytes, _state_bytes

pytestmark = pytest.mark.gpu

UV = np.array([[550.0, 200.0], [375.0, 375.0], [130.0, 200.0], [305.0, 200.0], [410.0, 130.0]])
GOOD, CUT, FAR = (0, 1, 2), 3, 4
ALL = (0, 1, 2, 3, 4)
KEYS = ("h", "Si", "visible", "z", "matched", "corr")


@functools.lru_cache(maxsize=None)
def _archive(srukf, synth, which="scene"):
    """the five records, captured once per scene"""
    cs = _case(srukf, synth, 8, which)
    keep = ga.X4
    ga.X4 = cs["pose"].copy()                                    # (capture_records creates its landmarks from the robot state X4)
    try:
        rec, f = ga.capture_records(srukf, cs["p"], cs["frames"][0], UV)
    finally:
        ga.X4 = keep
    f.close()
    lm = np.array([px for _, px in cs["recs"]])                  # the landmarks' pixels in frame 0
    if which == "scene":
        assert np.linalg.norm(UV[:, None, :] - lm[None, :, :], axis=2).min() >= 40.0
    rec["patch"][CUT] = cs["frames"][0][100:121, 100:121]
    rec["X6"][FAR, 0] += 50.0
    return rec


def _run(f, srukf, first, count, mode, checked):
    return f.run_images_checked(first, count, mode=mode) if checked else f.run_images(first, count, mode=mode)


@functools.lru_cache(maxsize=None)
def _twin(srukf, synth, mode, idx=ALL, F=6, checked=False):
    """the reference: run_images(f, 1) then archive_search(frames[f]) for every frame, the switch off; computed once per case"""
    cs, rec = _case(srukf, synth, 8), _archive(srukf, synth)
    g = _filter(srukf, cs, F)
    ga.set_archive(g, rec, list(idx))
    out = {k: [] for k in KEYS}
    traj = []
    for t in range(F):
        traj.append(_run(g, srukf, t, 1, mode, checked))
        res = g.archive_search(cs["frames"][t])
        for k, v in zip(KEYS, res): out[k].append(np.array(v, copy=True))
    out = {k: np.array(v) for k, v in out.items()}
    out["tmpl"] = [g.archive_template(j) for j in range(len(idx))]
    out["traj"] = np.vstack(traj)
    out["state"] = _state_bytes(g)
    out["matches"] = _record_bytes(g.get_image_matches(0, F))
    out["patches"] = _patch_bytes(g)
    assert g.clamp_info() == (-1, -1)
    g.close()
    _conditions(out, idx)
    return out


def _conditions(tw, idx):
    """what the scene was chosen for, on the twin alone"""
    m, v, c = tw["matched"], tw["visible"], tw["corr"]
    good = [j for j, r in enumerate(idx) if r in GOOD]
    if good:
        assert (m[:, good] == 1).all() and (v[:, good] == 1).all(), (m, v)
        print("twin: L = %d, good records' corr >= %.4f over %d frames" % (len(idx), c[:, good].min(), len(m)))
        assert c[:, good].min() > 0.8
        assert tw["z"].reshape(len(m), len(idx), 2)[:, good].all()
    if CUT in idx:
        j = idx.index(CUT)
        assert (v[:, j] == 1).all() and (m[:, j] == 0).all() and (c[:, j] < 0.7).all() and (c[:, j] > 0.0).all(), (v[:, j], m[:, j], c[:, j])
    if FAR in idx:
        j = idx.index(FAR)
        assert (v[:, j] == 0).all() and (m[:, j] == 0).all() and (c[:, j] == 0).all()


def _rows(rec, a=0, b=None):
    return tuple(np.ascontiguousarray(rec[k][a:b]).tobytes() for k in KEYS)


def _searching(srukf, synth, F, idx=ALL, graph=None, which="scene", **params):
    cs, rec = _case(srukf, synth, 8, which), _archive(srukf, synth, which)
    f = _filter(srukf, cs, F, graph=graph)
    ga.set_archive(f, rec, list(idx))
    f.images_search_archive(True, **params)
    return f


@pytest.mark.parametrize("mode_name,checked,idx", [("BATCHED", False, ALL), ("JOINT", False, ALL), ("BATCHED", True, ALL), ("BATCHED", False, (0,))])
def test_against_the_stepwise_call_bit_for_bit(srukf, synth, mode_name, checked, idx):
    """run_images(0, 6) with the switch on against the twin's six run_images(f, 1) + archive_search(frame f): every row of h, Si, visible, z, matched and corr
    bit-identical, hits = the row sums of matched, the templates those of the twin's last search; L = 5 in both modes and through run_images_checked, and L = 1."""
    F, mode = 6, getattr(srukf, "UPDATE_" + mode_name)
    tw = _twin(srukf, synth, mode, idx, F, checked)
    f = _searching(srukf, synth, F, idx)
    traj = _run(f, srukf, 0, F, mode, checked)
    rec = f.get_image_archive(0, F)
    assert f.clamp_info() == (-1, -1)
    assert rec["L"] == len(idx)
    for k in KEYS:
        assert rec[k].reshape(-1).tobytes() == tw[k].reshape(-1).tobytes(), k
    assert np.array_equal(rec["hits"], tw["matched"].sum(axis=1)), (rec["hits"], tw["matched"].sum(axis=1))
    assert rec["hits"].tolist() == [len([r for r in idx if r in GOOD])] * F
    for j in range(len(idx)):
        assert np.array_equal(f.archive_template(j), tw["tmpl"][j]), j
    assert any(t.any() for t in tw["tmpl"])
    assert traj.tobytes() == tw["traj"].tobytes() and _state_bytes(f) == tw["state"]
    f.close()


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_search_is_read_only_inside_a_run(srukf, synth, mode_name):
    """the switch on against a filter with it off: trajectory, X, S, get_image_matches' record and every matchPatch bit-identical"""
    F, mode = 6, getattr(srukf, "UPDATE_" + mode_name)
    _twin(srukf, synth, mode, ALL, F)
    cs = _case(srukf, synth, 8)
    f = _searching(srukf, synth, F)
    g = _filter(srukf, cs, F)
    ga.set_archive(g, _archive(srukf, synth))
    out = []
    for q in (f, g):
        t = q.run_images(0, F, mode=mode)
        assert q.clamp_info() == (-1, -1)
        out.append((t.tobytes(),) + _state_bytes(q) + _record_bytes(q.get_image_matches(0, F)) + (_patch_bytes(q),))
    assert f.get_image_archive(0, F)["hits"].tolist() == [3] * F
    with pytest.raises(srukf.SrukfError) as e: g.get_image_archive(0, F)      # the switch is off: no record
    assert e.value.rc == -5
    f.close(); g.close()
    assert out[0] == out[1]


@pytest.mark.parametrize("mode_name", ["BATCHED", "JOINT"])
def test_graph_forms_are_one_computation(srukf, synth, mode_name):
    """11 frames as the default graphs (one 8-frame graph + three single frames), as eager launches and as two calls of 5 + 6 frames: state, the association's
    record and the search record bit-identical — and the search record that of the twin's 11 step-wise searches"""
    F, mode = F_MAX, getattr(srukf, "UPDATE_" + mode_name)
    tw = _twin(srukf, synth, mode, ALL, F)
    out = []
    for name in ("default", "eager", "split"):
        f = _searching(srukf, synth, F, graph=0 if name == "eager" else None)
        t = np.vstack([f.run_images(0, 5, mode=mode), f.run_images(5, 6, mode=mode)]) if name == "split" else f.run_images(0, F, mode=mode)
        assert f.clamp_info() == (-1, -1)
        rec = f.get_image_archive(0, F)
        out.append((t.tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + _rows(rec) + (rec["hits"].tobytes(), _patch_bytes(f)))
        f.close()
    assert out[0] == out[1] and out[0] == out[2]
    assert _rows(rec) == _rows(tw) and rec["hits"].tolist() == [3] * F


def test_parameters_live_in_the_device_struct(srukf, synth):
    """graphs on: frames 0 - 2 with half_cap 40, frames 3 - 5 with corr_threshold 2.0 — the same captured frames, other values; against the same two runs eager.
    Frames 3 - 5 then hold no match, the same visible rows, and corr as before"""
    F, mode = 6, srukf.UPDATE_BATCHED
    tw = _twin(srukf, synth, mode, ALL, F)
    out = []
    for graph in (None, 0):
        f = _searching(srukf, synth, F, graph=graph, half_cap=40)
        f.run_images(0, 3, mode=mode)
        f.images_search_archive(True, corr_threshold=2.0)
        f.run_images(3, 3, mode=mode)
        rec = f.get_image_archive(0, F)
        out.append(_rows(rec) + (rec["hits"].tobytes(),) + _state_bytes(f))
        f.close()
    assert out[0] == out[1]
    assert _rows(rec, 0, 3) == _rows(tw, 0, 3) and rec["hits"].tolist() == [3, 3, 3, 0, 0, 0]
    assert np.array_equal(rec["visible"][3:], tw["visible"][3:]) and rec["visible"][3:, :4].all()
    assert not rec["matched"][3:].any() and not rec["z"][3:].any()
    assert rec["corr"][3:].tobytes() == tw["corr"][3:].tobytes()


def test_archive_replaced_inside_a_sequence(srukf, synth):
    """L = 5 for frames 0 - 2, then archive_set with records 1 and 3 and frames 3 - 5: rows 3 - 5 are the twin's step-wise searches at L = 2, L reads 2 and the
    earlier rows are zero (the record was rebuilt for the new L); then an empty archive: a clean run, L = 0, no hits"""
    F, mode, idx = 8, srukf.UPDATE_BATCHED, (1, 3)
    tw = _twin(srukf, synth, mode, idx, 6)
    f = _searching(srukf, synth, F)
    f.run_images(0, 3, mode=mode)
    assert f.get_image_archive(0, 3)["hits"].tolist() == [3, 3, 3]
    ga.set_archive(f, _archive(srukf, synth), list(idx))
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 3)      # the record went with the old archive
    assert e.value.rc == -5
    f.run_images(3, 3, mode=mode)
    rec = f.get_image_archive(0, 6)
    assert rec["L"] == 2 and _rows(rec, 3, 6) == _rows(tw, 3, 6) and rec["hits"].tolist() == [0, 0, 0, 1, 1, 1]
    assert not any(rec[k][:3].any() for k in KEYS)
    for j in range(2):
        assert np.array_equal(f.archive_template(j), tw["tmpl"][j])
    z = np.zeros
    f.archive_set(z((0, 6)), z((0, 6, 6)), z((0, 21, 21), dtype=np.uint8), z((0, 3, 3)), z((0, 3)), z((0, 2)))
    f.run_images(6, 2, mode=mode)
    assert f.clamp_info() == (-1, -1)
    rec = f.get_image_archive(0, F)
    assert rec["L"] == 0 and rec["hits"].tolist() == [0] * F and rec["h"].shape == (F, 0)
    f.close()


def test_switch_off_again_and_alternation(srukf, synth):
    """searching and plain runs alternate over one staged stack (3 + 3 + 3 + 2 frames: on, off, on, off), graphs against eager: the same bits, so neither kind
    replayed the other's captured frame; the rows only plain runs wrote are zero, the others the twin's"""
    F, mode = F_MAX, srukf.UPDATE_BATCHED
    tw = _twin(srukf, synth, mode, ALL, F)
    out = []
    for graph in (None, 0):
        f = _searching(srukf, synth, F, graph=graph)
        t = [f.run_images(0, 3, mode=mode)]
        f.images_search_archive(False); t.append(f.run_images(3, 3, mode=mode))
        f.images_search_archive(True); t.append(f.run_images(6, 3, mode=mode))
        f.images_search_archive(False); t.append(f.run_images(9, 2, mode=mode))
        rec = f.get_image_archive(0, F)
        out.append((np.vstack(t).tobytes(),) + _state_bytes(f) + _record_bytes(f.get_image_matches(0, F)) + _rows(rec) + (rec["hits"].tobytes(), _patch_bytes(f)))
        f.close()
    assert out[0] == out[1]
    assert rec["hits"].tolist() == [3, 3, 3, 0, 0, 0, 3, 3, 3, 0, 0]
    for a, b, searched in ((0, 3, True), (3, 6, False), (6, 9, True), (9, 11, False)):
        if searched: assert _rows(rec, a, b) == _rows(tw, a, b)
        else: assert not any(rec[k][a:b].any() for k in KEYS)
    assert out[0][0] == tw["traj"].tobytes() and out[0][1:3] == tw["state"]


def test_refusals(srukf, synth):
    """bad parameters: SRUKF_ERR_BAD_ARG, the switch as it was; the switch with a run in flight, and get_image_archive without a record (nothing staged, restaged,
    a map change, reset): SRUKF_ERR_SEQUENCE; rows beyond the stack: SRUKF_ERR_DIM_MISMATCH.  X, S and the matchPatches untouched throughout"""
    F, mode = 6, srukf.UPDATE_BATCHED
    tw = _twin(srukf, synth, mode, ALL, F)
    cs, arc = _case(srukf, synth, 8), _archive(srukf, synth)
    bad = (dict(half_cap=9), dict(half_cap=41), dict(chi2=0.0), dict(chi2=float("nan")), dict(chi2=float("inf")), dict(corr_threshold=float("nan")))
    f = _filter(srukf, cs, F)
    ga.set_archive(f, arc)
    before = _state_bytes(f) + (_patch_bytes(f),)
    for kw in bad:                                               # off stays off
        with pytest.raises(srukf.SrukfError) as e: f.images_search_archive(True, **kw)
        assert e.value.rc == -1 and "archive_search" in str(e.value), kw
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 1)
    assert e.value.rc == -5
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    f.run_images(0, 2, mode=mode)
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 1)      # a plain run: still no record
    assert e.value.rc == -5
    f.close()
    f = _searching(srukf, synth, F)
    for kw in bad:                                               # on stays on, with the parameters it had
        with pytest.raises(srukf.SrukfError) as e: f.images_search_archive(True, **kw)
        assert e.value.rc == -1, kw
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    f.run_images_async(0, 3, mode=mode)
    for on in (False, True):
        with pytest.raises(srukf.SrukfError) as e: f.images_search_archive(on)
        assert e.value.rc == -5 and "in flight" in str(e.value)
    f.synchronize()
    f.run_images(3, 3, mode=mode)
    rec = f.get_image_archive(0, F)
    assert _rows(rec) == _rows(tw) and rec["hits"].tolist() == [3] * F
    for first, count in ((0, F + 1), (F, 1), (4, 3)):
        with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(first, count)
        assert e.value.rc == -2
    state = _state_bytes(f)
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 16)), np.zeros((F, 8), dtype=np.int32))      # restaged: the images and the record are gone
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 1)
    assert e.value.rc == -5 and "stage_images" in str(e.value)
    f.stage_images(cs["frames"][:F])
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 1)      # staged again, nothing run
    assert e.value.rc == -5
    assert _state_bytes(f) == state
    f.delete_landmark(0)                                         # a map change
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 1)
    assert e.value.rc == -5
    f.close()
    f = _searching(srukf, synth, F)
    f.run_images(0, 2, mode=mode)
    assert f.get_image_archive(0, 2)["hits"].tolist() == [3, 3]
    f.reset()
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 1)
    assert e.value.rc == -5
    f.close()
    f = srukf.Filter(8, cs["p"]); f.set_state(cs["X1"], cs["S1"])
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 1)      # nothing staged
    assert e.value.rc == -5
    f.close()


def test_reset_clears_the_switch(srukf, synth):
    """after reset the switch is off: a run on the state set again leaves no record"""
    F, cs = 3, _case(srukf, synth, 8)
    f = _searching(srukf, synth, F)
    f.reset()
    f.set_state(cs["X1"], cs["S1"])
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 16)), np.zeros((F, 8), dtype=np.int32)); f.stage_images(cs["frames"][:F])
    ga.set_archive(f, _archive(srukf, synth))
    f.run_images(0, F)
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 1)
    assert e.value.rc == -5
    f.close()


def test_flagged_block_leaves_no_record(srukf, synth):
    """the shipped a1..a4 = 8 (tests/test_gpu_images.py, test_flagged_block_restores_its_checkpoint: the block flags by itself) with the switch on:
    SRUKF_ERR_CLAMP_PENDING, X, S and every matchPatch as before, get_image_archive SRUKF_ERR_SEQUENCE; a clean searching run afterwards answers again.
    The block flags in its first frame (row 48: the update of the frame's matches; on the CPU the oracle's update clamps there too, and not in a frame without a
    match), so the clean run is over frames 3 - 5 of the same stack, staged black: nothing matches, nothing clamps, the records are still predicted"""
    F = 6
    cs, arc = _case(srukf, synth, 8, "shipped"), _archive(srukf, synth, "shipped")
    f = _filter(srukf, cs)
    stack = np.ascontiguousarray(cs["frames"][:F]).copy(); stack[3:] = 0
    f.stage_sequence(cs["odo"][:F + 1], np.zeros((F, 16)), np.zeros((F, 8), dtype=np.int32)); f.stage_images(stack)
    ga.set_archive(f, arc)
    f.images_search_archive(True)
    before = _state_bytes(f) + (_patch_bytes(f),)
    with pytest.raises(srukf.SrukfError) as e: f.run_images(0, 3)
    assert e.value.rc == -7, str(e.value)
    frame, row = f.clamp_info()
    print("flagged frame %d, row %d" % (frame, row))
    assert 0 <= frame < 3
    assert _state_bytes(f) + (_patch_bytes(f),) == before
    with pytest.raises(srukf.SrukfError) as e: f.get_image_archive(0, 1)
    assert e.value.rc == -5 and "flagged" in str(e.value)
    f.run_images(3, 3)
    assert f.clamp_info() == (-1, -1) or f.clamp_info() == (frame, row)      # (clamp_info keeps the last flag's answer)
    rec = f.get_image_archive(3, 3)
    assert rec["L"] == 5 and rec["hits"].tolist() == [0, 0, 0] and not rec["matched"].any() and not rec["corr"].any()
    assert rec["h"].any(axis=1).all() and rec["Si"].any(axis=(1, 2, 3)).all()      # the rows were written (under a1..a4 = 8 the robot block is too wide for any record to be visible)    f.close()
