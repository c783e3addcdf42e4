"""The launch sequence of every frame form, pinned (-m gpu).

Which launches a frame consists of is decided on the host (srukf_replay.hip: frame_form / refactor_form).  Each case below runs a few frames
with profile() on and holds the per-class scope counts ("launches": one per ProfScope the sequence opens) to literals.  The literals were recorded on the commit
BEFORE the forms were named (docs/LAB_NOTEBOOK.md, "Frame forms"), so a change of the host's control flow that alters a sequence shows here as a changed count.
Scope counts alone cannot tell the refactorisation forms apart (a k_syrk launch is a k_syrk launch), so each case also holds the plan the filter reports
(plan_fold / plan_head_fold / plan_red_perm / split_form) and how many sequences ran with the split fold and the gain fold, recorded on the same commit (PLANS).
The values the sequences compute are held elsewhere (test_gpu_parity_r4.py's switch test, test_gpu_parity_r5.py's plan table)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 3   # frames per case: the first one behind a state from outside (null rows not canonical yet: the sequence that reads them as they are), then the default twice

# name -> (N, how the filter is set up and driven, expected non-zero counts)
#   staged: stage_sequence + run_frames(0, F);  step: F step-wise frames (predict_motion, predict_measurement, update)
CASES = {
    # the default staged replay on the plans of test_gpu_parity_r5.py's table
    "staged_head_fold_n200":      (200, dict(), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 1, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 3}),
    "staged_owners_fold_n224":    (224, dict(), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 1, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 3, 'k_syrk': 3}),
    "staged_no_head_fold_n159":   (159, dict(), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 1, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 3, 'k_syrk': 3}),
    "staged_permuted_syrk_n21":   (21, dict(), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 1, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 3, 'k_syrk': 3}),
    "staged_split_n395":          (395, dict(), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 1, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 3, 'k_syrk': 3}),
    # the srukf_debug_set switches at N = 200
    "staged_fused_motion_0":      (200, dict(debug={"fused_motion": 0}), {'k_gain': 3, 'k_gmw_persist': 3, 'k_motion': 3, 'k_project': 3, 'k_pxy': 3, 'k_rank_expand': 3}),
    "staged_fused_motion_1":      (200, dict(debug={"fused_motion": 1}), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 3, 'k_pxy': 3, 'k_rank_expand': 3}),
    "staged_pxy2_0":              (200, dict(debug={"pxy2": 0}), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 2, 'k_pxy': 3, 'k_rank_expand': 3}),
    "staged_tail_fuse_0":         (200, dict(debug={"tail_fuse": 0}), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 2, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 3}),
    "staged_head_fold_0":         (200, dict(debug={"head_fold": 0}), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 1, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 3, 'k_syrk': 3}),
    # other forms
    "staged_rank_aware_off":      (200, dict(rank_aware=0), {'k_gain': 3, 'k_gmw_check': 3, 'k_gmw_persist': 3, 'k_project_motion': 3, 'k_pxy': 3, 'k_syrk': 3}),
    "staged_full_rank_n8":        (8, dict(), {'k_gain': 3, 'k_gmw_check': 3, 'k_gmw_persist': 3, 'k_project_motion': 3, 'k_pxy': 3, 'k_syrk': 3}),
    "staged_f32_storage":         (200, dict(storage="F32"), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 1, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 3}),
    "staged_f32_mixed":           (200, dict(storage="F32_MIXED"), {'k_gain': 3, 'k_gmw_persist': 3, 'k_project_motion': 1, 'k_project_table': 1, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 3, 'k_syrk': 3}),
    "step_fast":                  (200, dict(step="fast"), {'k_gain': 3, 'k_gmw_check': 1, 'k_gmw_persist': 3, 'k_meas_stats': 1, 'k_motion': 1, 'k_project': 1, 'k_project_table': 2, 'k_pxy': 1, 'k_pxy2': 2, 'k_rank_expand': 2, 'k_syrk': 1, 'misc': 1}),
    "step_fast_next_announced":   (200, dict(step="fast", hint=True), {'k_gain': 3, 'k_gmw_check': 1, 'k_gmw_persist': 3, 'k_meas_stats': 1, 'k_motion': 1, 'k_project': 1, 'k_project_table': 1, 'k_pxy': 1, 'k_pxy2': 3, 'k_rank_expand': 2, 'k_syrk': 1, 'misc': 1}),
    "step_slow_batched":          (200, dict(step="slow"), {'k_gain': 3, 'k_gmw_check': 3, 'k_gmw_persist': 3, 'k_meas_stats': 3, 'k_motion': 3, 'k_project': 3, 'k_pxy': 3, 'k_syrk': 3, 'misc': 3}),
    "step_slow_sequential":       (200, dict(step="sequential"), {'k_gain': 3, 'k_gmw_check': 18, 'k_gmw_persist': 18, 'k_meas_stats': 3, 'k_motion': 3, 'k_project': 3, 'k_pxy': 3, 'k_syrk': 18, 'misc': 36}),
}


# name -> (plan_fold, plan_head_fold, plan_red_perm, split_form, split_fold_seqs and fold_seqs of the F frames)
PLANS = {
    "staged_head_fold_n200":    (1, 1, 0, 0, 0, 0),
    "staged_owners_fold_n224":  (1, 0, 0, 0, 0, 0),
    "staged_no_head_fold_n159": (0, 0, 1, 0, 0, 0),
    "staged_permuted_syrk_n21": (0, 0, 1, 0, 0, 0),
    "staged_split_n395":        (0, 0, 1, 1, 3, 0),
    "staged_fused_motion_0":    (1, 1, 0, 0, 0, 0),
    "staged_fused_motion_1":    (1, 1, 0, 0, 0, 0),
    "staged_pxy2_0":            (1, 1, 0, 0, 0, 0),
    "staged_tail_fuse_0":       (1, 1, 0, 0, 0, 0),
    "staged_head_fold_0":       (1, 0, 0, 0, 0, 0),
    "staged_rank_aware_off":    (0, 0, 0, 0, 0, 0),
    "staged_full_rank_n8":      (0, 0, 0, 0, 0, 0),
    "staged_f32_storage":       (1, 1, 0, 0, 0, 0),
    "staged_f32_mixed":         (0, 0, 1, 0, 0, 0),
    "step_fast":                (1, 1, 0, 0, 0, 0),
    "step_fast_next_announced": (1, 1, 0, 0, 0, 0),
    "step_slow_batched":        (1, 1, 0, 0, 0, 0),
    "step_slow_sequential":     (1, 1, 0, 0, 0, 0),
}


def launch_counts(srukf, synth, N, how):
    """(non-zero per-class scope counts of F frames, (step_fast, step_slow, exact_frames, clamp_rows), the plan tuple of PLANS)"""
    p = synth.scene_params()
    sc = synth.make_scene(N, F + 1, seed=3, p=p)
    f = srukf.Filter(N, p)
    if "rank_aware" in how:
        f.set_rank_aware(how["rank_aware"])
    if "storage" in how:
        f.set_storage(getattr(srukf, "STORAGE_" + how["storage"]))
    f.set_state(sc["X0"], sc["S0"])
    for k, v in how.get("debug", {}).items():
        f.debug_set(k, v)
    step = how.get("step")
    if step in ("slow", "sequential"):
        f.debug_set("step_fast", 0)
    f.set_profiling(True)
    seqs0 = (f.debug_get("split_fold_seqs"), f.debug_get("fold_seqs"))
    if not step:
        f.stage_sequence(sc["odo"], sc["z"], sc["matched"])
        f.run_frames(0, F)
    else:
        for t in range(F):
            if how.get("hint"):
                f.predict_motion_next(sc["odo"][t + 1], sc["odo"][t + 2])
            f.predict_motion(sc["odo"][t], sc["odo"][t + 1])
            h, Si, vis = f.predict_measurement()
            m = (sc["matched"][t] * vis).astype(np.int32)
            if step == "sequential":                             # three matched landmarks: six single-column refactorisations per frame
                keep = np.nonzero(m)[0][:3]
                assert keep.size == 3
                m = np.zeros_like(m); m[keep] = 1
            f.update(sc["z"][t], m, mode=srukf.UPDATE_SEQUENTIAL if step == "sequential" else srukf.UPDATE_BATCHED)
    got = {k: v["launches"] for k, v in f.profile().items() if v["launches"]}
    side = (f.debug_get("step_fast"), f.debug_get("step_slow"), f.debug_get("exact_frames"), f.debug_get("clamp_rows"))
    plan = (f.debug_get("plan_fold"), f.debug_get("plan_head_fold"), f.debug_get("plan_red_perm"), f.debug_get("split_form"),
            f.debug_get("split_fold_seqs") - seqs0[0], f.debug_get("fold_seqs") - seqs0[1])
    f.close()
    return got, side, plan


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_is_pinned(srukf, synth, name):
    N, how, want = CASES[name]
    got, side, plan = launch_counts(srukf, synth, N, how)
    print(f"LAUNCHES {name!r}: {got!r}  (step_fast, step_slow, exact_frames, clamp_rows) = {side}  PLAN {plan!r}")
    assert side[2] == 0 and side[3] == 0, side                   # no frame was flagged: the counts are the form's own
    if how.get("step") == "fast":
        assert side[:2] == (F - 1, 1), side                      # (the first frame of a state from outside is not a fast-path frame)
    elif how.get("step"):
        assert side[:2] == (0, F), side
    assert got == want
    assert plan == PLANS[name]
