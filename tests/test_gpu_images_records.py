"""GPU tests of the per-frame records of the image runs taken together (csrc/srukf_images.hip: image_group, images_restore, the srukf_get_image_* getters; DESIGN.md
§20 - §27): ONE handle with every option on — checked association, archive search, map policy, 1-point RANSAC consensus, rescue gate, display view, snapshots —
through srukf_images_resume and through a flagged block, and EVERY output field of EVERY getter walked from one list (GETTERS below).  A record column whose rows a
restore forgets to zero, zeroes though they stand, or whose row a getter copies with another width shows here as one named (getter, field).

The yardstick is the library's own other route, as in tests/test_gpu_images_resume.py: a fresh handle that runs only the first `keep` frames.  Everything is
compared as bytes; there is no tolerance.

Scenes and helpers are the sibling files': tests/test_gpu_images.py's N = 8 scene with F = 6 staged frames (the shape every sibling uses), the outlier scene and
THR = 4.8 px of tests/test_gpu_images_ransac.py (the consensus drops landmark 0's match in every frame, so the rescue gate has a candidate row to write), the seeded
policy of tests/test_gpu_policy.py (first_change == 2 on the clean scene) and the archive of L = 5 of tests/test_gpu_images_archive.py.  Which frames a block's
slots hold follows from its records (csrc/srukf_snapshot.hip): the test reads the tags and resumes where a slot holds the frame; where none does it holds the
library to its refusal, with every field unmoved."""
import numpy as np
import pytest

import test_gpu_archive as ga
import test_gpu_images_archive as gia
import test_gpu_images_ransac as gir
from test_gpu_images import _filter, _patch_bytes, _state_bytes
from test_gpu_images_ransac import THR
from test_gpu_policy import NEUTRAL, PAR, _seed

pytestmark = pytest.mark.gpu

F = 6
# (name, getter, the per-frame fields, what else the getter returns, block-scoped: rows a restored block wrote do not stand).  The archive record is not
# block-scoped: a resume keeps it whole, a flagged block invalidates it whole
GETTERS = (
    ("matches", "get_image_matches", ("z", "matched", "corr", "visible", "h"), (), False),
    ("checks", "get_image_checks", ("corr2", "z2", "flags"), (), False),
    ("archive", "get_image_archive", ("h", "Si", "visible", "z", "matched", "corr", "hits"), ("L",), False),
    ("policy", "get_image_policy", ("verdict", "summary"), ("state", "first_change"), True),
    ("ransac", "get_image_ransac", ("flags", "votes", "dist", "best", "n_active", "n_low"), ("first_outlier",), True),
    ("rescue", "get_image_rescue", ("flags", "h2", "Si2", "chi2", "n_cand", "n_high"), ("first_rescue",), True),
    ("display", "get_image_display", ("xyz", "cov", "axis", "sigma", "rot", "pose", "P4", "Si"), (), True),
)
FIRSTS = ("first_change", "first_outlier", "first_rescue")
# columns that may be zero in every row of these scenes: index 0 is a legal best hypothesis, no frame need rescue a match, 0 Jacobi rotations is a legal count
MAY_BE_ZERO = (("ransac", "best"), ("rescue", "n_high"), ("display", "rot"))


def _all_on(srukf, synth, scene, thr=THR, which="scene", chi2=None):
    f = _filter(srukf, gir._scene(srukf, synth, scene, which), F)
    ga.set_archive(f, gia._archive(srukf, synth, which))
    f.images_search_archive(True)
    f.images_policy(True, **PAR); f.set_policy_state(_seed())
    f.images_ransac(True, thr)
    if chi2 is None: f.images_rescue_gate(True)
    else: f.images_rescue_gate(True, chi2)
    f.images_display(True)
    f.images_snapshots(True)
    return f


def _run(f, count, mode, checked):
    return f.run_images_checked(0, count, mode=mode, **NEUTRAL) if checked else f.run_images(0, count, mode=mode)


def _read(f, first, count, only=None):
    """{(getter, field): bytes of rows [first, first + count)} and {(getter, extra): value} of every getter; the list above must name all a getter returns"""
    rows, extra = {}, {}
    for name, getter, fields, extras, _ in GETTERS:
        if only is not None and name not in only: continue
        rec = getattr(f, getter)(first, count)
        assert set(rec) == set(fields) | set(extras), (name, sorted(rec))
        for k in fields:
            assert len(rec[k]) == count, (name, k)
            rows[name, k] = np.ascontiguousarray(rec[k]).tobytes()
        for k in extras:
            extra[name, k] = rec[k].tobytes() if isinstance(rec[k], np.ndarray) else rec[k]
    return rows, extra


def _held(f):
    return _state_bytes(f) + (_patch_bytes(f),)


def _differ(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def _block_scoped(key):
    return next(g[4] for g in GETTERS if g[0] == key[0])


# chi2 = NO_RESCUE: the gate tests `dist < chi2` on a match the consensus dropped for lying more than THR pixels from its prediction — nothing passes, so the
# gate writes its candidates' rows and stops no block: the outlier scene then stops where the policy stops it, behind frame 2, and keep = 3 has a slot.  With the
# default chi2 the displaced match is rescued in frame 0: the block stops there, resume(0) is the rewind and resume(3) is refused
NO_RESCUE = 1e-9


@pytest.mark.parametrize("scene,mode_name,checked,chi2", [("clean", "BATCHED", False, None), ("clean", "JOINT", True, None), ("outlier", "BATCHED", True, NO_RESCUE),
                                                          ("outlier", "JOINT", False, NO_RESCUE), ("outlier", "BATCHED", False, None)])
def test_resume_with_every_option_on(srukf, synth, scene, mode_name, checked, chi2):
    """a block of 6 frames, then images_resume(keep) at keep = 3 and at the first stop the records report: state, patches and rows < keep of every field are the
    fresh handle's; rows >= keep are zero where block-scoped and the block's own elsewhere; the overlay draws a kept row and refuses a zeroed one"""
    mode = getattr(srukf, "UPDATE_" + mode_name)
    f = _all_on(srukf, synth, scene, chi2=chi2)
    traj = _run(f, F, mode, checked)
    assert f.clamp_info() == (-1, -1)
    wrote, wx = _read(f, 0, F)
    tags = f.get_image_snapshots()
    fc, fo, fr = wx["policy", "first_change"], wx["ransac", "first_outlier"], wx["rescue", "first_rescue"]
    stops = [s for s in (fc + 1 if fc >= 0 else None, fr if fr >= 0 else None) if s is not None]      # (the rescue gate is on: an outlier alone stops nothing)
    print("%s %s checked %d: first_change %d first_outlier %d first_rescue %d tags %s" % (scene, mode_name, checked, fc, fo, fr, tags))
    # every option wrote rows: a comparison of all-zero columns would show nothing
    zero = {k for k, v in wrote.items() if not any(v)}
    print("all-zero columns:", sorted(zero))
    allowed = set(MAY_BE_ZERO)
    if not checked: allowed |= {k for k in wrote if k[0] == "checks"}
    assert zero <= allowed, sorted(zero - allowed)
    keeps = sorted({3} | ({min(stops)} if stops and min(stops) < F else set()))
    resumed = 0
    for i, keep in enumerate(keeps):
        if i > 0:                                                # (one resume per block: the block again, on a handle of its own)
            f = _all_on(srukf, synth, scene, chi2=chi2)
            assert _run(f, F, mode, checked).tobytes() == traj.tobytes()
            again, ax = _read(f, 0, F)
            assert not _differ(again, wrote) and not _differ(ax, wx)
        if tags[keep & 1] != keep:                               # no slot holds that frame: refused, nothing moved
            before = _held(f)
            with pytest.raises(srukf.SrukfError) as e: f.images_resume(keep)
            assert e.value.rc == -5
            now, nx = _read(f, 0, F)
            assert _held(f) == before and not _differ(now, wrote) and not _differ(nx, wx)
            f.close()
            continue
        resumed += 1
        f.images_resume(keep)
        state = _held(f)
        lo, lx = _read(f, 0, keep) if keep else ({}, {})
        hi, hx = _read(f, keep, F - keep)
        ovl = f.render_image_overlay(keep - 1).tobytes() if keep else b""
        with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(keep)
        assert e.value.rc == -5
        f.close()
        g = _all_on(srukf, synth, scene, chi2=chi2)
        if keep:                                                 # (keep 0 is the rewind: the fresh handle as it stands)
            tg = _run(g, keep, mode, checked)
            assert g.clamp_info() == (-1, -1)
            want, wantx = _read(g, 0, keep)
            assert traj[:keep].tobytes() == tg.tobytes()
            assert not _differ(lo, want), (keep, _differ(lo, want))
            assert not _differ(lx, wantx), (keep, _differ(lx, wantx))
            assert ovl == g.render_image_overlay(keep - 1).tobytes()
        assert state == _held(g), keep
        g.close()
        row = {k: len(v) // F for k, v in wrote.items()}
        for k, v in hi.items():
            if _block_scoped(k): assert not any(v), (keep, k)
            else: assert v == wrote[k][keep * row[k]:], (keep, k)
        assert all(hx[g[0], k] == -1 for g in GETTERS for k in g[3] if k in FIRSTS), hx
    assert resumed >= 1, (keeps, tags)                           # precondition of the scene: asserted, not skipped


def test_flagged_block_with_every_option_on(srukf, synth):
    """the shipped a1 .. a4 = 8 (tests/test_gpu_images.py; threshold 1000 px as in the siblings' test_flagged_block_*: the frames' updates are the ones that flag):
    SRUKF_ERR_CLAMP_PENDING, state and patches as before the block, every block-scoped field zero over the block's rows; in front of the block and behind it every
    getter follows its own rule for a record never allocated, or allocated and zero"""
    f = _all_on(srukf, synth, "clean", thr=1000.0, which="shipped")

    def refused(names, word=None):
        for name in names:
            with pytest.raises(srukf.SrukfError) as e: _read(f, 0, F, only=(name,))
            assert e.value.rc == -5 and (word is None or word in str(e.value)), (name, str(e.value))

    # no run yet: the checked and the display record read as zeros, the others refuse (the policy group exists since the seed, its record has no run)
    rows, _ = _read(f, 0, F, only=("checks", "display"))
    assert rows and not any(any(v) for v in rows.values())
    refused(("archive", "policy", "ransac", "rescue"))
    before = _held(f)
    with pytest.raises(srukf.SrukfError) as e: _run(f, F, srukf.UPDATE_BATCHED, True)
    assert e.value.rc == -7, str(e.value)
    frame, _ = f.clamp_info()
    assert 0 <= frame < F
    assert _held(f) == before
    rows, extra = _read(f, 0, F, only=("matches", "checks", "policy", "ransac", "rescue", "display"))
    for k, v in rows.items():
        if _block_scoped(k): assert not any(v), k
    assert all(extra[g[0], k] == -1 for g in GETTERS for k in g[3] if k in FIRSTS and (g[0], k) in extra), extra
    assert extra["policy", "state"] == _seed().tobytes()
    assert any(rows["matches", "h"])                             # the association's record keeps what the block's frames wrote
    refused(("archive",), "flagged")
    for t in range(F):
        with pytest.raises(srukf.SrukfError) as e: f.render_image_overlay(t)
        assert e.value.rc == -5
    f.close()
