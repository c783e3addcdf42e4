// srukf_switches.h — where every measurement / test switch of srukf_debug_set is stored: the process-wide ones (one struct, one instance) and the per-filter ones
// (DbgSwitches, a member of every context).  None of them is needed to use the library; all default to the product path.  The table in srukf_debug.hip names each
// key once, with its range, its default and what a change invalidates; readers name the member.  Included by srukf_ctx.h and by the two kernel files whose host
// code reads a switch (srukf_factor.hip, srukf_gmw_persist.hip).
#pragma once
#include <atomic>

#ifndef SRUKF_PIVOT_RELAY_DEFAULT
#define SRUKF_PIVOT_RELAY_DEFAULT 1      // measured (docs/LAB_NOTEBOOK.md, pivot relay): N = 100 +5 %, N = 200 +1.2 %, N = 300 +4.8 % frames/s
#endif

namespace srukf_impl {
// Process-wide switches, one member per key of the same name (atomics: another thread's context may be launching while a switch is set; a switch applies to whatever
// is built or captured afterwards).  The library reads no environment variable
struct ProcessSwitches {
    std::atomic<int> gmw_persist{1}, gmw_fused{1}, rank_fused{1}, rank_fold{1}, rank_aware{1}, graphs{1}, mem_split{1}, head_fold_free{0};
    std::atomic<int> batch_wide{1}, batch_groups{0}, batch_split{1}, batch_k128{1}, batch_xcd{1};
    std::atomic<int> shared_tenants{2}, timing{0}, fold_head{0}, fold_force{0}, ctx_keep{24}, pivot_relay{SRUKF_PIVOT_RELAY_DEFAULT}, exact_rl{1};
};
inline ProcessSwitches g_sw;
}  // namespace srukf_impl

// Per-filter switches (srukf_switches::dbg in srukf_ctx.h; plain ints, read on the filter's own host path)
struct DbgSwitches {
    int fused_motion = 2;              // "fused_motion": the replay's motion step — 0: its own launch (k_motion + k_project), 1: inside the projection launch
                                       // (k_project_motion), 2: "table" mode where the rank-aware tail allows it (replay_motion_mode)
    int f32_fuse = 1;                  // "f32_fuse": fp32 storage also runs in "fused tail" mode (rounding inside k_rank_expand<2> and the state update)
    int table_perm = 1;                // "table_perm": "table" / "fused tail" mode also where the owners do not fold (k_syrk over the kept rows: N >= 300); 0: k_project_motion + k_pxy there
    int tail_fuse = 1;                 // "tail_fuse": k_rank_expand also projects the next frame ("fused tail" mode); 0: k_project_table in front of every frame
    int head_fold = 1;                 // "head_fold": exclusive rank-aware replay without the k_syrk launch (helper workgroups of the persistent launch)
    int nullskip = 1;                  // "nullskip": with pxy2, structurally null directions are projected for their own landmark only (NullSkip)
    int pxy2 = 1;                      // "pxy2": "table" mode forms the cross covariances on the permuted operands (k_pxy2); 0: k_pxy
    int step_fuse_export = 1;          // "step_fuse_export": the step-wise fast path's results reach the host from the launches that form them (the statistics' final passes inside
                                       // k_pxy2, the status + robot view from k_block_cov) instead of two k_export launches behind them (0: round 5's first form, for A/B)
    int view_auto = 1;                 // "view_auto": a host that fetched srukf_get_frame_view after its last update gets the view exported with the next update's status (0: never)
    int step_early = 2;                // "step_early": the update submits the next frame's checkpoint copy and (announced odometry) its k_set_step behind its own last launch (0: the predict
                                       // does), 2: and that frame's first launch, k_pxy2, too — srukf_predict_motion for the announced pair then has nothing left to submit
                                       // (the statistics as a launch of their own in front of it were tried: alone they still take 16 us — eight dependent memory round trips —, and
                                       //  16 + 25 us of launches lose to 25 us + the 12-us round trip they were meant to hide)
    int step_spin = 1;                 // "step_spin": the step-wise fast path waits for its two exports by spinning on a pinned flag word (0: hipStreamSynchronize)
    int step_fast = 1;                 // "step_fast": 0: the step-wise API keeps to its own launch sequences (k_motion, k_project, k_meas_*, k_pxy, ...: round 4's path)
    int split_record = 0;              // "split_record": every split-form factorisation first copies its input matrix to Gbak (scripts/split_replay.py)
    int null_canon = 1;                // "null_canon": a factor of the library's own making that was not produced by a rank-aware tail (NEED_REORDER, map changes) gets its null rows rewritten as sqrt(EPSILON) e_k at once
    int split_fold = 1;                // "split_fold": the split form's tile launch forms the tiles of S^T S - U U^T itself (k_gmw_tiles_fold), k_syrk in front keeps block row 0; 0: k_syrk forms everything first
    int gain_fold = 0;                 // "gain_fold": the staged replay's "fused tail" frames form U^T and the state update in the tile epilogue of k_pxy2 (three launches per frame); 0: k_gain
    int mixed_rank = 1;                // "mixed_rank": SRUKF_STORAGE_F32_MIXED runs the rank-aware refactorisation (fp32-formed S^T S - U U^T over the kept rows, FP64 factorisation
                                       // of the kept pivots only); 0: round 2's full-rank form, in which the null pivots divide fp32 noise (the negative study of rounds 2 / 5)
    int mixed_null_ppm = 1;            // "mixed_null_ppm": ... and its null-direction check allows this many 1e-6 of G_aa on top of 1e-12 (an fp32-formed G cannot resolve 1e-12)
    int mixed_bf16 = 0;                // "mixed_bf16": 1: the fp32 products from three bf16 pieces per operand on the bf16 matrix pipe (k_syrk_bf3) instead of the fp32 pipe
                                       // (k_syrk32).  Built and measured in round 6 (N = 500): 168 us + 2 x 19 us of splitting against 187 us + 2 x 9 us of conversion —
                                       // no gain: at one workgroup per CU (the FP64 accumulators beside the fp32 ones: 256 + 65 registers) every 32-row slab waits for its
                                       // operands (~1 us of load latency against 0.64 us of matrix work), so neither form is bound by its matrix pipe; and its error is
                                       // 1.6 x the fp32 pipe's (12.5 against 7.7 eps32 units over fixture g9).  Kept behind the switch, held to the same fixture
    int mixed_f64_robot = 1;           // "mixed_f64_robot": ... with the tiles of the robot block and of the shared anchor in FP64 (mxr_f64_tiles); 0: every kept tile from the fp32 pipe (study)
};
