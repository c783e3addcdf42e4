// srukf_ctx.h — what the host-side translation units of libsrukf_hip.so share: the context (struct srukf_ctx), the helpers behind the C-ABI.  Internal:
// include/srukf.h is the boundary.  What the kernel files offer (launchers, size / table helpers, their argument structs) comes from srukf_launch.h, declared there only.
//   srukf_api.hip     context lifetime, state accessors, the step-wise calls (predictMotion / predictMeasurement / KalmanUpdate), storage, profiling read-out
//   srukf_replay.hip  the launch sequences of a frame (seq_*), the rank-aware null set, graph cache, staged replay (srukf_run_frames*)
//   srukf_images.hip  image runs of the staged replay: the association (checked or not), the consensus and the archive search inside captured frames (srukf_stage_images,
//                     srukf_run_images*, srukf_get_image_*, srukf_images_*)
//   srukf_split.hip   split form of the persistent factorisation: side stream, probe, buffers
//   srukf_batch.hip   batched replay (srukf_run_frames_batch)
//   srukf_map.hip     map changes (srukf_add_landmarks / srukf_delete_landmark / srukf_insert_landmarks) and data association
//   srukf_ransac.hip  1-point RANSAC: the consensus over all single-match hypotheses, the measurement prediction from the posterior
//   srukf_rescue.hip  the rescue gate: would a match the consensus dropped be rescued? (srukf_rescue_gate; srukf_images_rescue_gate: k_rescue_gate_staged behind the
//                     tail of the frames that hold the consensus, issued by srukf_images.hip)
//   srukf_overlay.hip colour-frame intake (srukf_set_frame_bgr) and the 2-D feature overlay (srukf_render_overlay)
//   srukf_loop.hip    loop points: the record an archived landmark takes along, the placement of re-inserted landmarks
//   srukf_archive.hip the archive on the handle and its search by appearance (srukf_archive_set / srukf_archive_search), step-wise and behind the frames of an image run
//                     (srukf_images_search_archive: seq_archive_search, k_archive_search_staged; srukf_get_image_archive: srukf_images.hip)
//   srukf_policy.hip  the map policy's verdict (srukf_map_policy; srukf_images_policy: k_map_policy_staged behind the frames of an image run, issued by srukf_images.hip)
//   srukf_snapshot.hip the state a block of image frames is resumed from (srukf_images_snapshots / srukf_images_resume: k_image_snapshot in front of every frame, issued by srukf_images.hip)
//   srukf_joint.hip   the joint measurement update's kernels (srukf_update_joint, SRUKF_UPDATE_JOINT frames of the staged replay; host code: srukf_step.hip, srukf_replay.hip, srukf_images.hip)
//   srukf_unique.hip  the association that keeps the score map: ambiguity veto, sub-pixel peak (srukf_associate_checked; its host code is in srukf_map.hip; srukf_run_images_checked*: srukf_images.hip)
//   srukf_patch.h     (through srukf_launch.h) the appearance record's sizes, the checked association's buffer layouts, the search kernels' shared front
//   srukf_debug.hip   srukf_debug_*, stand-alone primitives for the parity tests
//   srukf_switches.h  where the switches of srukf_debug_set are stored: the process-wide struct g_sw, the per-filter DbgSwitches
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <cstddef>
#include <vector>
#include <algorithm>
#include <utility>
#include <atomic>
#include <functional>
#include <mutex>
#include <map>
#include "srukf_launch.h"
#include "srukf_switches.h"

#define SRUKF_GRAPH_FRAMES 8
#define SRUKF_MAX_TENANTS 4                                    // 4 x (1 pivot + 63 workers with two register tiles each) fill 256 CUs at N = 200
#define SRUKF_NULL_ENERGY 1e-12
#ifndef SRUKF_BATCH_GROUPS_MAX
#define SRUKF_BATCH_GROUPS_MAX 4
#endif
//                                                          // groups of filters srukf_run_frames_batch runs side by side, each on a stream of its own

enum KClass { KC_MOTION = 0, KC_PROJECT, KC_STATS, KC_PXY, KC_GAIN, KC_SYRK, KC_GMW_TRAIL, KC_GMW_PERSIST, KC_GMW_CHECK,
              KC_GMW_COL, KC_RANK_EXPAND, KC_PROJECT_MOTION, KC_PROJECT_TABLE, KC_PXY2, KC_MISC,
              KC_DET_RESPONSE, KC_DET_CAND, KC_DET_RANK, KC_DET_SELECT, KC_CAPTURE, KC_LM_ELLIPSOID, KC_BGR2GRAY, KC_OVERLAY,
              KC_ARCHIVE_PREDICT, KC_ARCHIVE_WARP, KC_ARCHIVE_SEARCH, KC_ASSOC_CHECKED, KC_COUNT };
struct ProfEvent { hipEvent_t a, b; int kc; };

// the captured frames of one update mode of the staged replay: one frame / SRUKF_GRAPH_FRAMES frames / srukf_prepare_frames*: a whole block of frames in ONE graph
struct ReplayGraphs {
    hipGraph_t one = nullptr, eight = nullptr, block = nullptr;
    hipGraphExec_t one_exec = nullptr, eight_exec = nullptr, block_exec = nullptr;
    int block_frames = 0;
};

// ---- persistent GMW launch (k_gmw_persist): per-matrix-size resources --------------------------------
// nreal: the tiles that hold values (ntiles minus the T - Tp pass-on tiles of the rank-aware form, which ride as a register-free third slot of the first workers)
struct GmwPlan { GmwPanel64* pans = nullptr; GmwSync* sync = nullptr; GmwTile* tiles = nullptr; int ntiles = 0, nreal = 0, T = 0, Tp = 0, workers = -1, tenants = 1, cus = 0, relay = 0; };      // relay: two pivot workgroups (gmw_pivot_relay), 2 + workers resident

// feature detection (srukf_detect.hip): scratch of one pass over an image_w x image_h frame, allocated on the first srukf_detect_features;
// in / out grow with the caller's map, archive and output capacities
struct DetScratch {
    double *resp = nullptr, *cand_r = nullptr; int *cand_pix = nullptr, *sorted = nullptr, *rank = nullptr, *gxy = nullptr, *blk = nullptr; void* hdr = nullptr;
    void *in = nullptr, *out = nullptr; size_t in_bytes = 0, out_bytes = 0;
};

// 1-point RANSAC (srukf_ransac.hip), allocated on the first call and sized by the context's N (map-size scope; a revive frees it).
// Ut: k_pxy's product for the consensus; D / F: d_ij and the inlier flag of every pair (N x N); zin: z | matched; res: dist | inlier | votes | best.
// X, S, odo, Cm, fs: a copy of the state, an odometry pair and where k_motion leaves its by-products (the fast path's consensus; srukf_repredict_measurement);
// the rest: the slow path's predict half on that copy
struct RansacScratch {
    double *Ut = nullptr, *D = nullptr, *zin = nullptr, *res = nullptr, *X = nullptr, *S = nullptr, *odo = nullptr;
    double *sigR = nullptr, *Cm = nullptr, *Z = nullptr, *DZ = nullptr, *h = nullptr, *PxyR = nullptr, *mpart = nullptr;
    unsigned char* F = nullptr; int* votes = nullptr; FrameScalars* fs = nullptr;
    // srukf_rescue_gate: rq_in = z (mp) | matched, inlier (N ints each); rq_out = h2 (2N) | Si2 (4N) | chi2 (N) | flags (N ints); rq_scr = PxyR (5 mp) | vis (N ints)
    double *rq_in = nullptr, *rq_out = nullptr, *rq_scr = nullptr;
};

// the archive searched by appearance (srukf_archive.hip): L records in the layouts of srukf_insert_landmarks (patch / tmpl with the strides of the map's appearance
// records), rob = pose | P4 of the search in hand, out = h | Si | z | corr | xyz | visible | matched, hst = the same pinned, then pose | P4.  Handle scope;
// srukf_reset and srukf_destroy drop it
struct ArchiveState {
    int L = 0;
    double *X6 = nullptr, *S66 = nullptr, *R = nullptr, *t = nullptr, *px = nullptr, *rob = nullptr, *out = nullptr, *hst = nullptr;
    unsigned char *patch = nullptr, *tmpl = nullptr;
};

// { X, S, the matchPatch array, the policy state } of an image run, kept on the device: the block's checkpoint and the two snapshot slots are one of these each
// (image_state_copy, srukf_images.hip, is the one place that knows the four sizes).  pol is only ever copied while the policy group exists
struct ImageState { double *X = nullptr, *S = nullptr; unsigned char* tmpl = nullptr; srukf_policy_state* pol = nullptr; };

// image runs of the staged replay (srukf_stage_images / srukf_run_images*; DESIGN.md sections 20 - 27).  Map-size scope, the staged sequence's lifetime: images_drop.
// Every device buffer below is named once, in image_group (srukf_images.hip), with its size, whether it is zeroed, and for a per-frame record column its row width
// and whether a restored block's rows stand: allocation (image_group_ensure, in front of the first run that needs the group, outside any capture), images_drop,
// images_archive_drop, images_restore and the getters all read that table.  Here only what the table cannot say.
// graphs: the captured frames (one and eight) of every form of an image frame and update mode, ONE table: graphs[ImageForm::index()][0 BATCHED / 1 JOINT].  A form
// never replays a frame captured for another one (nor a frame of srukf_run_frames*, nor the other way round): the index is the guarantee.  drop_graphs walks the table.
struct ImageReplay {
    // the staged gray frames [frames][image_h][image_w]; the record the association leaves beside the staged z_seq / m_seq rows it overwrites (corr_seq, vis_seq,
    // h_seq); the Cartesian points the warp reads (xyz: not c->G — nothing has shown G to be free inside a replayed block)
    unsigned char* images = nullptr;
    double *corr_seq = nullptr, *h_seq = nullptr, *xyz = nullptr;
    int* vis_seq = nullptr;
    int frames = 0;
    ReplayGraphs graphs[32][2];
    // The block: every image run since the last srukf_synchronize.  ck: the state it started from (ck.pol lives in the policy group), ck_canon: whether the null rows
    // were canonical then.  pending / checked / searching: the frames srukf_synchronize waits for are image frames / with a checked / a searching run among them
    // (images_block_end takes the three).  ck_clean: ck is that of a block srukf_synchronize ended clean and nothing has written X, S, a matchPatch or the policy
    // state since (srukf_images_rewind / _resume; cleared by step_invalidate, which every state-writing entry passes, and by the few that do not pass it, each in place)
    ImageState ck;
    bool pending = false, ck_canon = false, checked = false, searching = false, ck_clean = false;
    // Checked image runs: the checked record, and the parameters the checked frames read (written in stream order in front of every checked
    // run).  The captured checked frames hold the pointer of the filter's score buffer they were captured with, chk_scores
    double *corr2_seq = nullptr, *z2_seq = nullptr; int* flags_seq = nullptr;
    MatchArgs* match_args = nullptr; const double* chk_scores = nullptr;
    // Searching image runs: ar_rec, ONE allocation laid out column-major over frames (ImageArchiveRecord for frames x ar_L), and the
    // parameters.  The captured searching frames hold the archive's pointers and L workgroups: images_archive_drop.  ar_valid: a searching run has written the
    // record and no flagged block has been restored since
    double* ar_rec = nullptr; ArchiveArgs* ar_args = nullptr; int ar_L = 0;
    bool ar_valid = false;
    // The map policy behind image frames: the per-landmark state, the record and the parameters.  No captured frames of their own:
    // run_images_issue.  pol_valid (and rs_valid, rq_valid below): a run with the switch on has written the record
    srukf_policy_state* pol_state = nullptr; int* pol_verdict = nullptr; srukf_policy_summary* pol_sum = nullptr; srukf_policy_params* pol_args = nullptr;
    bool pol_valid = false;
    // The 1-point RANSAC consensus inside image frames: the scratch of the two launches (rs_D, rs_F, rs_votes), the record, the threshold
    double *rs_D = nullptr, *rs_dist = nullptr; unsigned char* rs_F = nullptr; int *rs_votes = nullptr, *rs_flags = nullptr, *rs_rvotes = nullptr;
    RansacSummary* rs_sum = nullptr; RansacArgs* rs_args = nullptr;
    bool rs_valid = false;
    // The rescue gate behind the tail of such frames: the record, what meas_final_tail stores besides (rq_vis, rq_PxyR), the threshold
    int *rq_flags = nullptr, *rq_vis = nullptr; double *rq_h2 = nullptr, *rq_Si2 = nullptr, *rq_chi2 = nullptr, *rq_PxyR = nullptr;
    RescueSummary* rq_sum = nullptr; RescueArgs* rq_args = nullptr;
    bool rq_valid = false;
    // The state a block is resumed from: two slots (sn[f & 1]: the state frame f started from), the tags and the latch (sn_ctl), the guard's
    // parameters.  The block, as srukf_images_resume needs it: blk_first its first frame, blk_end the frame behind its last, blk_snap: every run of it had the switch
    // on and began where the one before ended
    ImageState sn[2];
    SnapshotCtl* sn_ctl = nullptr; SnapshotArgs* sn_args = nullptr;
    int blk_first = 0, blk_end = 0; bool blk_snap = false;
    // The display view behind image frames: one row of ImageDisplayRow per staged frame (dp_rec) and one of rotation counts (dp_rot).
    // dp_rows [frames]: the host's mark per row — a run with the switch on has issued the row's launches and no restore has zeroed it since (what
    // srukf_render_image_overlay asks: rot cannot tell, 0 rotations is a legal value)
    double* dp_rec = nullptr; int* dp_rot = nullptr;
    std::vector<unsigned char> dp_rows;
    // Colour frames in the staged stack (srukf_stage_images_bgr): bgr holds bgr_pix pixels of 3 bytes, padded to whole groups of four —
    // the whole stack, tight like `images`, when bgr_kept, else the transit buffer of the staging call, freed before it returns.  The overlays of a run of frames
    // (srukf_render_image_overlays): ovs_count output frames (ovs_out) and record slabs (ovs_rec), the largest count asked for so far
    unsigned char* bgr = nullptr; size_t bgr_pix = 0; bool bgr_kept = false;
    unsigned char* ovs_out = nullptr; void* ovs_rec = nullptr; int ovs_count = 0;
};

// one frame's row of the display record, offsets in doubles: xyz [3N] | cov [9N] | axis [4N] | sigma [3N] | robot [20] = P4 | pose | Si [4N]
struct ImageDisplayRow { size_t xyz, cov, axis, sigma, robot, Si, doubles; };
constexpr ImageDisplayRow image_display_row(size_t N) { return { 0, 3 * N, 12 * N, 16 * N, 19 * N, 19 * N + 20, 23 * N + 20 }; }

// ---- the context: who owns what across a map change ("who owns what across a map change") ----------------------
// srukf_ctx = srukf_handle_scope + srukf_map_scope (which holds one srukf_life).  WHERE a member is declared says what a map change, a revive and srukf_destroy do
// with it; adopt_context, ctx_revive and srukf_destroy hold no list of members, only the few exceptions, each with its reason.

// The per-filter switches, a part of the handle scope with a name of its own for one reason: ctx_retire gives the retiring context a copy in one assignment (see there)
struct srukf_switches {
    int rank_aware = 1;                    // srukf_set_rank_aware
    int debug_starve = 0;                  // srukf_debug_starve_workers: persistent launches start without their workers (tests of the fallback)
    bool split_off = false;                // a split-form pair of this filter was abandoned (its two launches did not run side by side — e.g. the branches of a captured
                                           // graph sharing a hardware queue): it keeps to the memory-tile instance of k_gmw_persist (read_fs; srukf_debug_get "split_off")
    bool use_graph = true;
    DbgSwitches dbg;                       // the measurement / test switches of srukf_debug_set (srukf_switches.h)
};

// Handle scope: what stays at the caller's address through every map change.  A context built for another map size (ctx_obtain) carries a handle scope too: its own
// defaults, on the handle's device / stream / parameters, never the owner of the stream; what it allocates there itself (ensure_image) it frees itself.
struct srukf_handle_scope : srukf_switches {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    srukf_params p;
    // Map changes rebuild the map-size scope behind the handle.  A rebuilt context used to be destroyed and the next one created from nothing — ~0.3 ms of
    // allocations, plans and tile tables, 0.5 - 2.4 ms of frees (pinned host memory among them) per map change at N = 200, where the reference's map changes every
    // few frames (SLAM.cpp:552-562, 2443-2460) and N only moves by +- 1.  The handle keeps the last few contexts it outgrew and revives one instead: ctx_obtain / ctx_retire
    std::vector<srukf_ctx*> retired;
    double* spare_stage = nullptr; size_t spare_stage_bytes = 0;   // pinned staging of the context retired last (retired contexts keep none: pinning 11.8 MB costs ~2.5 ms)
    // profiling
    bool profiling = false;
    std::vector<ProfEvent> pev;
    double prof_ms[KC_COUNT] = {}; long long prof_n[KC_COUNT] = {}; double prof_flops[KC_COUNT] = {}; double prof_bytes[KC_COUNT] = {};
    // the frame the filter holds (same image size whatever the map's): d_image, gray (srukf_associate / srukf_detect_features / srukf_capture_appearance with a frame);
    // d_bgr, its colour (srukf_set_frame_bgr: W x H x 3, B G R), and d_ovl, the overlay's output (srukf_render_overlay), both padded to whole groups of four pixels.
    // All allocated on first use.  frame_valid: d_image holds the caller's last frame; bgr_valid: d_bgr is its colour (a later call that brings a gray frame clears
    // it).  srukf_reset drops both flags
    unsigned char *d_image = nullptr, *d_bgr = nullptr, *d_ovl = nullptr; bool frame_valid = false, bgr_valid = false;
    DetScratch det;                        // srukf_detect_features
    ArchiveState archive;                  // srukf_archive_set / srukf_archive_search
    bool img_search = false;               // srukf_images_search_archive: every frame of every later image run is followed by a search of the archive, with ...
    ArchiveArgs img_search_args = { 40, 0.8, 5.99146454710798 };   // ... these parameters.  Survives map changes; srukf_reset clears it
    bool img_policy = false;               // srukf_images_policy: every frame of every later image run is followed by the map policy's verdict, with ...
    srukf_policy_params img_policy_args = SRUKF_POLICY_DEFAULTS;   // ... these parameters.  Survives map changes; srukf_reset clears it
    bool img_ransac = false;               // srukf_images_ransac: every frame of every later image run holds the 1-point RANSAC consensus between association and update, with ...
    double img_ransac_thr = 8.0;           // ... this threshold.  Survives map changes and srukf_reset
    bool img_rescue = false;               // srukf_images_rescue_gate: every frame of every later image run that holds the consensus is followed by the rescue gate, with ...
    double img_rescue_chi2 = 5.99146454710798;      // ... this threshold (CHI2INV_TABLE(0, 2)).  Survives map changes and srukf_reset
    bool img_snap = false;                 // srukf_images_snapshots: every frame of every later image run begins with k_image_snapshot.  Survives map changes and srukf_reset
    bool img_display = false;              // srukf_images_display: every frame of every later image run is followed by k_image_view + k_lm_ellipsoid into its row of the display record.  Survives map changes and srukf_reset
    std::string err;
    // the pool allocations among the members above (det and archive: det_scratch_free / archive_free).  A new buffer of this scope is added HERE
    template <class F> void each_device_buffer(F f) const { void* b[] = { d_image, d_bgr, d_ovl }; for (void* q : b) f(q); }
};

// One life of a context — from srukf_create or ctx_revive to the map change that retires it: the flags and counters a revive sets back, by assigning a fresh one.
// A member belongs here only if a revived context must find it at its initialiser; what survives a revive (spin_ok, step_seq, the mxr_* shape, ...) stays below
struct srukf_life {
    int storage = SRUKF_STORAGE_F64;       // SRUKF_STORAGE_F32 / _F32_MIXED: X32 / S32 hold the inter-frame state (a map change sets the handle's mode again; the buffers stay)
    bool dx_pending = false;               // k_gain left slice partials of dX that the next k_syrk must add to X
    bool dx_lm = false;                    // ... as per-landmark shares in dxk (the gain fold of k_pxy2) instead of k_gain's slice partials in dxp
    bool xr1_pending = false;              // replay path: the robot mean after the motion step waits in fs->Xr1 for the same launch
    // NEED_REORDER (frames that follow a landmark addition): K_new = m_nFilters, permutation between the normal and the
    // disordered layout (getPermutationMatrix, SLAM.cpp:1303-1334), disordered factor
    int K_new = 0;
    bool null_canonical = false;           // every structurally null row of S is exactly sqrt(EPSILON) e_k (update_null_set checks; true behind every rank-aware frame tail)
    bool tail_ok = false;                  // "fused tail" mode is possible: directions 0 and 1 are kept rows (the Si factor names their Z rows: they are projected for every landmark, which
                                           // the frame tail only does for kept rows — a state where they are structurally null stays with k_project_table)
    int clamp_frame_host = -1, clamp_row_host = -1;   // what the last SRUKF_ERR_CLAMP_PENDING was about (srukf_clamp_info)
    int seqF = 0;                          // frames of the staged sequence (odo_seq / z_seq / m_seq below)
    // state machine
    int phase = 0;   // 0 idle, 1 after predict_motion, 2 after predict_measurement
    bool frame_updated = false;            // the last call that touched the state was a srukf_update of the frame in hand (srukf_repredict_measurement may follow)
    bool next_odo_valid = false;           // srukf_predict_motion_next: next_odo is the pair the next srukf_predict_motion will bring
    bool async_pending = false;
    bool joint_bad_host = false;           // the SRUKF_ERR_UNSUPPORTED in hand is a joint frame's non-finite input (joint_bad_report): srukf_run_frames restores its checkpoint
    // the step-wise fast path (step_* below)
    bool step_fast = false;                // the frame in flight runs on the fast path
    bool step_uncommitted = false;         // ... and its motion step still waits beside the state (fs->Xr1, Cmat): state getters commit it first (k_commit_motion)
    bool step_chain = false;               // X, S, the permuted copy and the frame scalars are exactly what the last fast-path tail left: its constant rows stand
    bool proj_valid = false;               // ... and that tail projected the frame with the odometry pair proj_odo (Z, DZ, the table, fs->ctl)
    bool fs_seq_step = false;              // fs->odo_seq points at odo_step (srukf_run_frames_async points it back at the staged sequence)
    bool last_update_sequential = false;   // a host that updates in SRUKF_UPDATE_SEQUENTIAL mode never takes the fast path (decided at predict time)
    bool ck_valid = false;                 // the next srukf_predict_motion finds its checkpoint made (ckS2 / ckX2)
    bool ck3_inflight = false;             // ... and until then the copy is in flight on ck_stream with nothing but ck_e3 to wait on (step_ck_join)
    bool ck_pending = false;               // the copy of the state before the frame runs beside the frame's first launch (step_ck_join)
    bool pre_issued = false;               // the NEXT frame's first launch (k_pxy2) went out behind this frame's tail, for the odometry pair pre_odo
    bool next_pose_pending = false;        // the next k_gain launch carries next_odo[3..5] as the sequence's third pose (no launch of its own)
    bool setstep_done = false;             // k_set_step for the announced next frame went out behind this frame's tail (poses: setstep_odo)
    unsigned long long meas_seq = 0;       // != 0: k_pxy2's statistics jobs mirror h | Si | visible into hstage and raise the flag word with this number (srukf_predict_measurement waits for it)
    bool step_export_attached = false;     // the last rank_expand carried step_export
    StepExport step_export = {};           // dst != null: the next rank_expand is the step-wise fast path's and exports the frame's status + robot view itself
    bool mirror_next = false;              // the next seq_pxy is the step-wise fast path's: its MeasArgs carry the host mirror
    bool view_auto = false; int view_unused = 0;   // the host called srukf_get_frame_view after its last update -> the following updates export the view with their status; three views nobody read end it
    int view_hits = 0;
    bool view_cached = false;              // *hview is the view of the CURRENT state (same lifetime as robot_cached)
    bool robot_cached = false;             // the 20 doubles behind *hfs hold P4 and the pose of the CURRENT state (fast path: fetched with the frame's status)
    bool f32_stale = false;                // fp32 storage: X32 / S32 (srukf_get_state_f32) are behind the rounded fp64 working copies (refreshed on demand)
    int step_fast_frames = 0, step_slow_frames = 0;   // srukf_debug_get "step_fast" / "step_slow"
    int exact_frames = 0;                  // staged frames srukf_run_frames repeated on the exact column path (flagged: theta clamp, a skipped direction that is not null, an abandoned launch): "exact_frames"
};

// Map-size scope: everything sized by N or tied to one factor.  adopt_context swaps it between the handle and the context built for the new size, whole; a retired
// context keeps it for the next time the map has that size (what depends only on N, the device and the parameters — buffers, plans, tile tables, pinned areas,
// side streams — is what it is kept for), srukf_destroy frees it (map_scope_free, over the list at the end)
struct srukf_map_scope : srukf_life {
    KDims d;
    KWeights w;
    // HBM buffers
    double *X = nullptr, *S = nullptr, *G = nullptr, *Gbak = nullptr, *Wf = nullptr;
    double *sigR = nullptr, *Cmat = nullptr, *Z = nullptr, *DZ = nullptr, *Ut = nullptr;
    double *h = nullptr, *Si = nullptr, *PxyR = nullptr, *D = nullptr;
    double *zcur = nullptr, *odocur = nullptr, *small = nullptr, *mpart = nullptr, *dxp = nullptr;
    int *vis = nullptr, *mcur = nullptr;
    unsigned long long* theta = nullptr;
    // gain fold (round 6: k_gain's work inside k_pxy2 in the staged replay's "fused tail" mode): its sync words (zero between frames), the per-landmark shares of the
    // state update (N x np), how many tile workgroups read the robot columns of the permuted copy
    unsigned int* fold_sync = nullptr; double* dxk = nullptr; int fold_robot_tiles = 0;
    // data association (srukf_assoc.hip): per-landmark appearance records, allocated on first use
    unsigned char *app_patch = nullptr, *app_tmpl = nullptr;
    double *appR = nullptr, *appT = nullptr, *appPx = nullptr, *corr = nullptr;
    int* has_app = nullptr;
    // what the overlay is drawn from: h | Si | z (8N doubles) | matched (N ints), the per-landmark records
    double* ov_in = nullptr; void* ov_rec = nullptr;
    // srukf_associate_checked (srukf_unique.hip), allocated on its first call: match_res = z | corr | corr2 | z2 | matched, flags (7N doubles, exported in one piece),
    // match_scores = every landmark's score map (PT_SCORE_STRIDE doubles each: map | wx wy x0 y0).  match_valid: the maps are the last checked call's (srukf_get_match_scores);
    // a map change and srukf_reset drop both buffers (match_drop)
    double *match_res = nullptr, *match_scores = nullptr; bool match_valid = false;
    RansacScratch ransac;                  // srukf_ransac_consensus / srukf_repredict_measurement
    // the joint update (srukf_update_joint, SRUKF_UPDATE_JOINT frames of the staged replay; srukf_joint.hip), allocated by joint_ensure on first use: jointZd = the sigma points' deviations dZ (joint_dev_rows x mp), jointW = [ Pzz | Pxy^T | z - h ]
    // (mp x joint_work_ld), jointRd = the factored diagonal blocks (mp x 64) with the status word behind them
    double *jointZd = nullptr, *jointW = nullptr, *jointRd = nullptr;
    // srukf_get_landmarks_display / srukf_get_frame_view_display: xyz (3N) | cov (9N) | axis (4N) | sigma (3N) | P4, pose (20) | rot (N ints).  A buffer of its own,
    // allocated by the first call (not G: the next frame's pre-issued first launch may be in flight behind the update)
    double* disp = nullptr;
    float *S32 = nullptr, *X32 = nullptr;  // storage != SRUKF_STORAGE_F64
    // SRUKF_STORAGE_F32_MIXED: S^T S - U U^T on the fp32 matrix pipe (srukf_mixed.hip)
    float *U32 = nullptr; double* mx_part = nullptr; void *mx_tasks = nullptr, *mx_tiles = nullptr; int mx_ntasks = 0, mx_ntiles = 0;
    // ... in the rank-aware form (round 6): the kept rows of S in permuted column order as float (the permuted copy's values are the stored floats), K <= r, only the
    // macro tiles of the pivoted panels; task list / partials of that shape (mixed_red_ensure)
    float* A32 = nullptr; double* mxr_part = nullptr; void *mxr_tasks = nullptr, *mxr_tiles = nullptr; int mxr_ntasks = 0, mxr_ntiles = 0, mxr_krows = 0, mxr_for_r = 0;
    // ... and which 32 x 32 tiles of it are formed in FP64 after all (k_syrk over this list, behind the fp32 launch): the tile rows / columns that hold the robot block
    // and the map's shared anchor (permuted positions r-4 .. r-1 and 0 .. 2).  The robot's pivots are its variance GIVEN the map — 2e-6 .. 9e-6 of its marginal variance
    // in the benchmark scene, the z coordinate exactly null (scripts/pivot_ratio_probe.py) — and the regression that produces them has weight ~1 on the anchor the
    // robot position was copied into: an fp32-formed entry there (relative error ~1e-7 .. 1e-6) is as large as the pivot itself.  Every other kept pivot is >= 0.1 of
    // its marginal variance
    int* mxr_f64_tiles = nullptr; int mxr_n_f64_tiles = 0;
    // ... and the operands of the bf16-piece form of the product (k_split_bf3 / k_syrk_bf3): X^T = [kept rows of S | U^T]^T as three planes of bf16, [np columns][mxr_ktot]
    unsigned short* mxr_xt = nullptr; size_t mxr_xt_stride = 0; int mxr_ktot = 0;
    int *perm = nullptr, *iperm = nullptr;
    double* Sdis = nullptr;
    GmwPanel64* pan[2] = { nullptr, nullptr };   // GMW panel hand-off buffers (double-buffered), one launch per panel
    GmwPlan gplan;                         // persistent GMW launch: panel buffers, sync block, task list
    // rank-aware refactorisation (srukf_rank.hip): red_r > 0 = the n - red_r structurally null directions are not pivoted
    int red_r = 0, red_Tp = 0;
    int *red_perm = nullptr, *red_iperm = nullptr;     // permuted position <-> state index, kept indices first
    double* gdiag = nullptr;                           // diagonal of G in permuted order (the factorisation overwrites it)
    double *shadowA = nullptr, *Utp = nullptr;         // replay form: kept rows of S / U^T in permuted column order (srukf_rank.hip)
    double *slabW = nullptr, *slabL = nullptr;         // batched replay: two panels' slabs W and L = W / D (2 x 64 x np each: the K = 128 trailing update reads a pair)
    // split form of the persistent factorisation (memory-tile sizes, a filter that has the GPU to itself): the slabs of every pivoted panel (gs_panels x 64 x np
    // each), the side stream the tile launch runs on and the events that fork it off / join it to the filter's stream
    double *gsW = nullptr, *gsL = nullptr; int gs_panels = 0;
    hipStream_t side = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    double* P1 = nullptr; int* pxy2_tiles = nullptr; int n_pxy2_tiles = 0, pxy2_split_b0 = 0;   // "table" mode: k_pxy2's second K half, its tile list
    int* nskip = nullptr; int ns_full = 0, ns_null = 0, ns_rows = 0;   // NullSkip lists (srukf_device.h): [dirs | nulls | rows] in one buffer
    int* red_head0_tiles = nullptr; int n_red_head0_tiles = 0; // split fold: the k_syrk tiles that stay with the launch in front (block row 0, tile (1, 1)) ...
    GmwTile* split_fold_list = nullptr; int n_split_fold = 0;     // ... and the grid of k_gmw_tiles_fold (forming jobs + tile workgroups, row by row: srukf_gmw_build_fold_list)
    double red_head0_flop = 0.0;                               // flop of the tiles in red_head0_tiles (the rest of k_syrk's count moves to the persistent launch's line of the profile)
    int* red_syrk_tiles = nullptr; int n_red_syrk_tiles = 0;   // k_syrk tiles of the kept rows (rows < 64 red_Tp) in permuted order: replay form without the owners' fold
    double red_fac_flop = 0, red_own_flop = 0;         // algorithmic flop of the rank-aware persistent launch: factorisation / owners' tiles of S^T S - U U^T
    GmwPlan gplan_red;                                 // tile list / sync block of the persistent launch with red_Tp pivoted panels
    // Sharing the GPU is the handle's choice, but the plans above are built for it: adopt_context applies the outgoing side's pair again through set_shared
    int shared_tenants = 2;                // SRUKF_GPU_SHARED: how many persistent launches share the GPU (each keeps to cus / tenants CUs; the gate admits that many)
    int gmw_shared = 0;                    // 0: the filter has the GPU to itself; 1: shared with other filters — persistent launches of at most half the CUs behind
                                           // the admission gate (k_gmw_gate); 2: one launch per panel (forced, or after an abandoned persistent launch)
    double *ckS = nullptr, *ckX = nullptr; // srukf_run_frames: state before the block of frames in flight (recovery from a theta-clamp frame)
    int *syrk_tiles = nullptr, *pxy_tiles = nullptr;   // (by, bx) per workgroup, XCD-aware order
    int *syrk_head_tiles = nullptr;                    // k_syrk tiles of the first srukf_gmw_head_rows() rows only (fused refactor)
    int n_syrk_tiles = 0, n_pxy_tiles = 0, n_syrk_head_tiles = 0, n_syrk_head_crit = 0;
    int* syrk_head_tiles_b = nullptr; int n_syrk_head_tiles_b = 0;      // the same tiles in the batched launch's order (k_syrk_b): one pair of tile columns per XCD, empty slots (-1) where a share is shorter
    FrameScalars* fs = nullptr;
    // staged sequence (seqF frames)
    double *odo_seq = nullptr, *z_seq = nullptr;
    int* m_seq = nullptr;
    // pinned staging
    double* hstage = nullptr; size_t hstage_bytes = 0;
    FrameScalars* hfs = nullptr;
    double* hmeas = nullptr;               // inside the hfs allocation, behind the robot view and the flag word
    double next_odo[6] = { 0, 0, 0, 0, 0, 0 };   // srukf_predict_motion_next (next_odo_valid)
    // Fast path of the step-wise API: a frame of the staged replay's own launch sequence ("fused tail" mode) cut in two at the host's association step
    double* odo_step = nullptr;            // device: (prev, cur, next) poses of the frame in flight — a three-pose "staged sequence" fs->odo_seq points at
    double step_odo[6] = { 0, 0, 0, 0, 0, 0 };   // the pair srukf_predict_motion was called with (the fallback to the other path needs it again)
    int step_seqF = 1;                     // 2: odo_step holds the next pose too (hint), the tail prepares and projects the next frame
    double proj_odo[6] = { 0, 0, 0, 0, 0, 0 };   // proj_valid
    // The copy for the NEXT frame is submitted by the update that ends this one, right behind its last launch (into the second pair of buffers; pair and event swap
    // when the frame turns out clean): the next srukf_predict_motion then finds its checkpoint made (ck_valid) and submits its first launch at once
    double *ckS2 = nullptr, *ckX2 = nullptr; hipEvent_t ck_e3 = nullptr;
    unsigned spin_ok = 0;                  // successful spin waits (step_wait_export queries the stream every 256th)
    double pre_odo[6] = { 0, 0, 0, 0, 0, 0 };       // pre_issued
    double setstep_odo[6] = { 0, 0, 0, 0, 0, 0 };   // setstep_done (poses: prev, cur)
    hipStream_t ck_stream = nullptr; hipEvent_t ck_e1 = nullptr, ck_e2 = nullptr;   // the copy of the state before the frame runs BESIDE the frame's first launch on a
                                           // stream of its own (it only has to be complete before k_gain touches S): ck_pending
    int* export_cnt = nullptr;             // 64 x 64 ints (zero): first-level counters of the exporting launch (StepExport::cnt)
    unsigned long long step_seq = 0;       // sequence number of the step-wise fast path's exports: the host spins on a pinned word (behind the robot view) that receives it
    double* hview = nullptr; size_t hview_doubles = 0;      // pinned: xyz (3N) | cov (9N) | X (n) of the state an update of the fast path left, when the host is known to ask for it
    int split_fold_seqs = 0;               // split-form pairs enqueued (or captured) with the split fold: "split_fold_seqs"
    int fold_seqs = 0;                     // frame sequences enqueued (or captured) with the gain fold: "fold_seqs" (tests: the switch took effect)
    // captured frames (staged inputs), replayed by srukf_run_frames_async: one set per update mode of the replay ([0] BATCHED, [1] JOINT: replay_graphs), so that a call in
    // one mode never replays the other's launch sequence; drop_graphs drops both
    ReplayGraphs graphs[2];
    ImageReplay img;                       // srukf_stage_images / srukf_run_images* (captured frames with the association in them: never the ones above, nor the other way round)
    // the pool allocations among the members above (Si and vis are inside h, mcur inside zcur; ransac, gplan, gplan_red, img: ransac_scratch_free / gmw_plan_destroy /
    // images_drop).
    // A new buffer of this scope is added HERE
    template <class F> void each_device_buffer(F f) const {
        void* b[] = { X, S, G, Gbak, Wf, sigR, Cmat, Z, DZ, Ut, h, PxyR, D, zcur, odocur, small, mpart, dxp, theta, fold_sync, dxk,
                      app_patch, app_tmpl, appR, appT, appPx, corr, has_app, ov_in, ov_rec, match_res, match_scores, disp,
                      S32, X32, U32, mx_part, mx_tasks, mx_tiles, A32, mxr_part, mxr_tasks, mxr_tiles, mxr_f64_tiles, mxr_xt,
                      perm, iperm, Sdis, pan[0], pan[1], red_perm, red_iperm, gdiag, shadowA, Utp, slabW, slabL, gsW, gsL, P1, pxy2_tiles, nskip,
                      red_head0_tiles, split_fold_list, red_syrk_tiles, ckS, ckX, syrk_tiles, pxy_tiles, syrk_head_tiles, syrk_head_tiles_b, fs,
                      odo_seq, z_seq, m_seq, odo_step, ckS2, ckX2, export_cnt, jointZd, jointW, jointRd };
        for (void* q : b) f(q);
    }
};

struct srukf_ctx : srukf_handle_scope, srukf_map_scope {};

#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    char b_[256]; snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    (ctx)->err = b_; return SRUKF_ERR_HIP; } } while (0)

namespace srukf_impl {

// fp32 storage of the state with everything that goes with it in "fused tail" mode (the tail and the state update round what they write).  The mixed-precision downdate in
// its rank-aware form (round 6) IS that mode with one difference: where the staged frame forms S^T S - U U^T over the kept rows (RF_PERMUTED_SYRK)
inline bool storage_f32_like(const srukf_ctx* c) { return c->storage == SRUKF_STORAGE_F32 || (c->storage == SRUKF_STORAGE_F32_MIXED && c->dbg.mixed_rank && c->A32); }

extern const char* const kclass_name[KC_COUNT];
extern thread_local std::string g_create_error;

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- device memory: the stream-ordered pool of the device (srukf_api.hip) ----
void srukf_pool_init();
hipError_t srukf_dmalloc_raw(void** p, size_t bytes);
template <class T> inline hipError_t srukf_dmalloc(T** p, size_t bytes) { return srukf_dmalloc_raw((void**)p, bytes); }
hipError_t srukf_dfree(void* p);
// the same, ordered on a context's own stream (no synchronisation: everything that touches the block is on that stream)
template <class T> inline hipError_t srukf_dmalloc_on(T** p, size_t bytes, hipStream_t st) { srukf_pool_init(); return hipMallocAsync((void**)p, bytes ? bytes : 8, st); }
hipError_t srukf_dfree_on(void* p, hipStream_t st);

// ---- small kernels of the host layer behind launchers (srukf_replay.hip) ----
void launch_refactor_reset(hipStream_t st, int np, unsigned long long* theta_bits, FrameScalars* fs, int reset_stats);
void launch_set_seq(hipStream_t st, FrameScalars* fs, const double* odo_seq, int seqF, const srukf_params& p);
void launch_set_run(hipStream_t st, FrameScalars* fs, int frame, int clear_clamp, double* traj_base);      // traj_base null: a frame outside a staged run
void launch_set_step(hipStream_t st, FrameScalars* fs, double* odo, int seqF, double a1, double a2, double a3, double a4, int fresh, const double poses[9]);
// device -> pinned host memory, two segments of 8-byte words; flag (pinned too, may be null) receives seq behind the data
void launch_export(hipStream_t st, const void* a, size_t bytes_a, const void* b, size_t bytes_b, void* host_pinned, unsigned long long* flag = nullptr, unsigned long long seq = 0);
void launch_set_frame_control(hipStream_t st, FrameScalars* fs);
void launch_commit_motion(hipStream_t st, int n, int ld, double* X, double* S, const double* Cm, const FrameScalars* fs, double* A, const int* iperm, int rk);
void launch_sym_permute(hipStream_t st, int n, int ld, const double* src, int lds, double* dst, const int* map);
void launch_gather(hipStream_t st, int n, int ld, const double* src, double* dst, const int* map);

// ---- plans, tables (srukf_api.hip) ----
void gmw_plan_destroy(GmwPlan& g, hipStream_t st = nullptr);
int gmw_plan_create(GmwPlan& g, int np, hipStream_t st, int Tp = 0, int tenants = 1);
void host_weights(int Na, const srukf_params& p, KWeights& w);
std::vector<int> build_tile_table(int n_own, int n_other, bool upper, bool own_is_row, int k_index /* 0: K grows with tile.x, 1: with tile.y */);
void prof_collect(srukf_ctx* c);
void adopt_context(srukf_ctx* c, srukf_ctx* c2);
int ctx_obtain(srukf_ctx* handle, srukf_ctx** out, int N);     // a context for N landmarks with the handle's device / stream / parameters: a retired one revived, or srukf_create
void ctx_retire(srukf_ctx* handle, srukf_ctx* old);

// ---- feature detection and appearance capture (srukf_detect.hip) ----
void det_scratch_free(DetScratch& s, hipStream_t st);
int ensure_image(srukf_ctx* c);
int take_frame(srukf_ctx* c, const unsigned char* gray);       // gray -> d_image (the held frame); NULL: the held one or SRUKF_ERR_SEQUENCE
void launch_capture_patch(hipStream_t st, const unsigned char* img, int W, int first, int K, const double* uv, const double* X, int n,
                          unsigned char* app_patch, unsigned char* app_tmpl, double* appR, double* appT, double* appPx, int* has_app);

// ---- 1-point RANSAC (srukf_ransac.hip) ----
void ransac_scratch_free(RansacScratch& s, hipStream_t st);

// ---- srukf_associate_checked's buffers, the appearance records (srukf_map.hip) ----
void match_drop(srukf_ctx* c);
int match_ensure(srukf_ctx* c, const char* who);      // match_res and match_scores, allocated on first use (never inside a capture)
int ensure_appearance(srukf_ctx* c);      // the per-landmark appearance records (and the handle's frame buffer), allocated and zeroed on first use

// ---- archive search (srukf_archive.hip) ----
void archive_free(ArchiveState& a, hipStream_t st);
void seq_archive_search(srukf_ctx* c);                 // the search behind a frame of a searching image run (behind seq_refactor)

// ---- the map policy's verdict (srukf_policy.hip) ----
int policy_params(srukf_ctx* c, const srukf_policy_params* pp, srukf_policy_params* out, const char* who);      // srukf_policy_params' rules (pp null: the defaults)

// ---- display ellipsoids (srukf_display.hip) ----
void launch_lm_ellipsoid(hipStream_t st, int N, double eps, const double* cov, double* axis, double* sigma, int* rot);

// ---- colour-frame intake, 2-D overlay (srukf_overlay.hip) ----
size_t overlay_rec_bytes(int N);
size_t overlay_bgr_bytes(int npix);
void launch_bgr2gray(hipStream_t st, int npix, const unsigned char* bgr, unsigned char* gray);
void launch_overlay(hipStream_t st, int W, int H, int N, const double* h, const double* Si, const double* z, const int* matched, void* rec,
                    const unsigned char* bgr /* NULL: gray three times */, const unsigned char* gray, unsigned char* out);
constexpr int OVERLAY_BLOCK_MAX = 65535;                     // frames in one launch_overlay_block: the frame is gridDim.y
// the same for `count` staged frames in two launches (W H a multiple of four, N >= 1, count <= OVERLAY_BLOCK_MAX): every pointer is the first frame's, the rows' strides are in elements, the
// stacks tight, rec count slabs of overlay_rec_bytes(N)
void launch_overlay_block(hipStream_t st, int W, int H, int N, int count, const double* h, size_t h_stride, const double* Si, size_t Si_stride, const double* z, size_t z_stride,
                          const int* matched, size_t m_stride, void* rec, const unsigned char* bgr /* NULL: gray three times */, const unsigned char* gray, unsigned char* out);

// ---- loop points (srukf_loop.hip) ----
// k_lm_record's staging block: X6 | S66 | R | t | px | has_app, then the patch at its stride (zero-filled behind its bytes)
constexpr int LM_REC_DOUBLES = 6 + 36 + 9 + 3 + 2 + 1, LM_REC_PATCH_DOUBLES = PT_PATCH_STRIDE / 8, SRUKF_LM_RECORD_DOUBLES = LM_REC_DOUBLES + LM_REC_PATCH_DOUBLES;
void launch_lm_record(hipStream_t st, const double* P66, const double* X, int k, double eps, const unsigned char* app_patch, const double* appR,
                      const double* appT, const double* appPx, const int* has_app, double* out);
void launch_lm_insert(hipStream_t st, const double* S, int ld, const double* X, int p6, int L, const double* blk, double* S2, double* X2, int n2, int ld2);

struct ProfScope {
    srukf_ctx* c; int kc; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(srukf_ctx* c_, int kc_, double flops, double bytes) : c(c_), kc(kc_) {
        if (c->profiling) {
            hipEventCreate(&a); hipEventCreate(&b); hipEventRecord(a, c->stream);
            c->prof_flops[kc] += flops; c->prof_bytes[kc] += bytes;
        }
    }
    ~ProfScope() {
        if (c->profiling) { hipEventRecord(b, c->stream); c->pev.push_back({ a, b, kc }); }
    }
};

// ---- the step-wise fast path's bookkeeping (srukf_api.hip) ----
void step_commit_motion(srukf_ctx* c);
unsigned long long* step_flag(srukf_ctx* c);          // the pinned word exports raise behind their data
int step_wait_export(srukf_ctx* c, unsigned long long seq);   // spin on it ("step_spin"), or synchronise the stream
void step_invalidate(srukf_ctx* c);
void step_state_replaced(srukf_ctx* c);
void step_ck_join(srukf_ctx* c);

// ---- launch sequences (srukf_replay.hip) ----
// The measurement half of a frame, a ladder: k_meas_stats as a launch of its own (step-wise slow path) / the statistics ride on k_pxy / ... and the motion step ran
// inside the projection launch / ... and the product is k_pxy2's, on the permuted operands / ... and the previous frame's tail projected this frame.
enum MeasForm { MEAS_SEPARATE_STATS, MEAS_PLAIN, MEAS_FUSED_MOTION, MEAS_TABLE, MEAS_FUSED_TAIL };
struct FrameForm {
    MeasForm meas; bool robot_table;       // robot_table: projection and tail work on the table of robot poses — from MEAS_TABLE on, and with "pxy2" off below it
    bool fused_stats() const { return meas >= MEAS_PLAIN; }
    bool fused_motion() const { return meas >= MEAS_FUSED_MOTION; }
    bool pxy2() const { return meas >= MEAS_TABLE; }
    bool fused_tail() const { return meas >= MEAS_FUSED_TAIL; }
};
constexpr FrameForm FORM_SEPARATE_STATS{ MEAS_SEPARATE_STATS, false }, FORM_PLAIN{ MEAS_PLAIN, false }, FORM_FUSED_TAIL{ MEAS_FUSED_TAIL, true };
// What a frame of an image run holds beyond the plain frame form (replay_one_image_frame): checked — k_associate_checked_staged in k_associate_staged's place;
// search — the archive search behind its tail; ransac — the consensus between association and update; snap — k_image_snapshot in front of it (DESIGN.md
// section 25); rescue — the rescue gate behind its tail, in front of the archive search (only ever set with ransac).  index(): the form's row
// of ImageReplay::graphs.  IMAGE_FORMS counts the forms without the gate, as it did; a gated form's row is its ungated form's + IMAGE_FORMS (IMAGE_FORM_ROWS rows in all,
// of which only those with ransac are ever issued or captured)
// The map policy is no part of the form: it has no captured frames of its own, it is an eager launch behind each frame and a property of the run (run_images_issue)
constexpr int IMAGE_FORMS = 16;
constexpr int IMAGE_FORM_ROWS = 2 * IMAGE_FORMS;
struct ImageForm {
    bool checked, search, ransac, snap, rescue;
    int index() const { return ((checked ? 1 : 0) | (search ? 2 : 0) | (ransac ? 4 : 0) | (snap ? 8 : 0)) + (rescue ? IMAGE_FORMS : 0); }
    static ImageForm at(int index) { return ImageForm{ (index & 1) != 0, (index & 2) != 0, (index & 4) != 0, (index & 8) != 0, index >= IMAGE_FORMS }; }
};
static_assert(sizeof(ImageReplay::graphs) / sizeof(ImageReplay::graphs[0]) == IMAGE_FORM_ROWS, "ImageReplay::graphs has one row per form of an image frame");
// What is asked of a refactorisation  S <- gmw(S^T S - U[ub:ue] U[ub:ue]^T):  the tail of a staged or fast-path frame (no backup, the last launch ends the frame) /
// checked (G kept in Gbak, the host reads clamp_rows afterwards) / one column of SEQUENTIAL mode (as checked, behind a reset of the gamma / xi accumulators)
struct RefactorRequest { enum Kind { FRAME_TAIL, CHECKED, SEQ_COLUMN } kind; int ub, ue; };
inline RefactorRequest refactor_frame_tail(const srukf_ctx* c) { return RefactorRequest{ RefactorRequest::FRAME_TAIL, 0, c->d.mp }; }
inline RefactorRequest refactor_checked(const srukf_ctx* c) { return RefactorRequest{ RefactorRequest::CHECKED, 0, c->d.mp }; }
inline RefactorRequest refactor_column(int m) { return RefactorRequest{ RefactorRequest::SEQ_COLUMN, m, m + 1 }; }
// ... and the launches it consists of (refactor_form): the owners of the persistent launch form their tiles / k_syrk over the kept rows in permuted order / k_syrk in
// state order + permutation pass / every pivot factored.  sub: head fold (owners' fold), own order or split fold (permuted k_syrk), fused (full rank)
enum RefactorForm { RF_OWNERS_FOLD, RF_PERMUTED_SYRK, RF_RANK_VIA_PERMUTATION, RF_FULL_RANK };
struct RefactorPlan { RefactorForm form; bool persist, head_fold, own_order, split_fold, fused; };      // persist: persistent launch(es), not one launch per panel
enum GmwPanels { GMW_ALL_PANELS, GMW_KEPT_PANELS, GMW_KEPT_PANELS_SPLIT_FOLD };      // launch_gmw_fast: the full plan / the rank-aware plan / ... whose tile launch forms tiles too
inline int kept_rows16(const srukf_ctx* c) { return (c->red_r + 15) & ~15; }      // K range of the products over the kept rows
void quantize_state(srukf_ctx* c);
RankArgs rank_args(const srukf_ctx* c);
RankArgs tail_rank_args(const srukf_ctx* c, FrameForm ff);
NullSkip null_skip(const srukf_ctx* c);
FrameForm frame_form(const srukf_ctx* c);
RefactorPlan refactor_form(const srukf_ctx* c, const RefactorRequest& rq);
void seq_predict_fused(srukf_ctx* c, FrameForm ff);
void seq_predict_motion(srukf_ctx* c, const double* odo_pair_dev);
void seq_predict_measurement(srukf_ctx* c, FrameForm ff);
void shadow_rebuild(srukf_ctx* c);
bool plan_persists(const srukf_ctx* c, const GmwPlan& gp);
int gate_limit(const srukf_ctx* c);
bool replay_red_perm(const srukf_ctx* c);
int replay_motion_mode(const srukf_ctx* c);
void seq_refactor(srukf_ctx* c, const RefactorRequest& rq, FrameForm ff);
int exact_repeat_begin(srukf_ctx* c, int frame, double* traj_base);
void launch_gmw_fast(srukf_ctx* c, double* Gbuf, double* Sout, GmwPanels which);
// the arguments of a factorisation Gbuf -> Sout on plan gp of this context (Tp / krows <= 0: every panel pivoted / every row kept)
GmwLaunch gmw_launch(const srukf_ctx* c, const GmwPlan& gp, double* Gbuf, double* Sout, int Tp, int krows);
// ... as one launch per 64-row panel (g.pans / sync / tiles are not used), the two hand-off buffers alternating: j0 = -64 factors the first 64 x 64 region; rank-aware
// form: the step after the last pivoted panel still runs (it writes that panel's S rows).  per_step(j0): what the caller holds around each launch (a ProfScope)
template <class PerStep> inline void gmw_per_panel(hipStream_t st, const GmwLaunch& gl, GmwPanel64* const* pan, PerStep per_step)
{
    const GmwLaunch g = gmw_normalised(gl);
    int pb = 0;
    for (int j0 = -64; j0 + 64 < g.ld && j0 + 64 <= 64 * g.Tp; j0 += 64, pb ^= 1) {
        auto around = per_step(j0);
        srukf_launch_gmw_step64(st, g.n, g.ld, j0, g.eps, g.G, pan[pb ^ 1], pan[pb], g.D, g.Sout, g.fs);
    }
}
static inline void gmw_per_panel(hipStream_t st, const GmwLaunch& g, GmwPanel64* const* pan) { gmw_per_panel(st, g, pan, [](int) { return 0; }); }
void run_gmw(srukf_ctx* c, double* Gbuf, double* Sout, bool slow);
int refactor_reorder(srukf_ctx* c, int ub, int ue);
void seq_pxy(srukf_ctx* c, FrameForm ff);
void seq_gain_only(srukf_ctx* c, const double* z_dev, const int* m_dev, FrameForm ff);
void seq_gain(srukf_ctx* c, const double* z_dev, const int* m_dev, FrameForm ff);
// the joint update in seq_gain_only's place behind seq_pxy (srukf_step.hip): its work buffers, allocated outside any capture; its launches (no host in between)
int joint_ensure(srukf_ctx* c, const char* what);
void seq_joint_launches(srukf_ctx* c, const double* z_dev, const int* m_dev);
int update_null_set(srukf_ctx* c);
int mixed_red_ensure(srukf_ctx* c);
void drop_graphs(srukf_map_scope* c);
void graphs_destroy(ReplayGraphs& g);                  // one set of captured frames goes (one, eight, block)
void exact_path(srukf_ctx* c, const double* Gbuf, double* Sout);      // the exact column path for Gbuf -> Sout (D, theta, clamp count as side effects)
void set_null_canonical(srukf_ctx* c);
void canonicalize_null_rows(srukf_ctx* c);      // after update_null_set on a factor of the library's own making (NEED_REORDER, map changes): the next frame may take the fast path
int read_fs(srukf_ctx* c);
int read_fs_host(srukf_ctx* c);
int set_shared(srukf_ctx* c, int shared, int tenants);

// ---- what the staged replay (srukf_replay.hip) and the image runs (srukf_images.hip) share ----
int replay_mode_check(srukf_ctx* c, int mode, const char* who);      // which update modes the staged replay has, and on which storage
// nframes frames captured into *g / *ge: issue_frame enqueues one frame on c->stream (replay_one_frame, replay_one_image_frame); never leaves the stream capturing
int capture_frames(srukf_ctx* c, int nframes, hipGraph_t* g, hipGraphExec_t* ge, const std::function<void()>& issue_frame);
void replay_prologue(srukf_ctx* c);                    // in front of a run: a pending motion step committed, the frame scalars point at the staged sequence
int replay_launch_graphs(srukf_ctx* c, const ReplayGraphs& g, int count);      // count frames: eight-frame graphs, then single frames
int replay_epilogue(srukf_ctx* c);                     // behind what a run issued: frames are in flight (srukf_synchronize), the step-wise state machine is idle
// run(dt) with dt = count trajectory rows on the device; copied to traj_host (may be null) when run returns SRUKF_OK
int with_device_traj(srukf_ctx* c, int count, double* traj_host, const std::function<int(double*)>& run);
void images_archive_drop(srukf_map_scope* c, hipStream_t st);      // the searching image runs' record, parameters and captured frames go (the archive changes; the caller has synchronised the stream)
void images_drop(srukf_map_scope* c, hipStream_t st);      // the staged images, their record, checkpoint and captured frames go (the caller has synchronised the stream)
// srukf_synchronize, behind the frames it waited for: the flags of the block in flight go; read: the frame scalars came back; flagged: they hold a flag — a block of
// image frames then comes back to its checkpoint and leaves no score map and no search record; a block that ended clean can be rewound or resumed
void images_block_end(srukf_ctx* c, bool read, bool flagged);

// ---- split form of the persistent factorisation (srukf_split.hip) ----
bool split_form(const srukf_ctx* c, const GmwPlan& gp, bool ignore_starve = false);
void split_ensure(srukf_ctx* c, const GmwPlan& gp);
void side_stream_lend(srukf_ctx* c);

// ---- batched replay (srukf_batch.hip) ----
void batch_plan_forget(const srukf_ctx* c);
void batch_drop_all_graphs();

}  // namespace srukf_impl
