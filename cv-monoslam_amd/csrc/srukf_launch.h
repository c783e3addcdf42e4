// srukf_launch.h — what the kernel files offer the host layer, declared ONCE: every srukf_launch_* launcher, the size / table / list helpers (the process-wide
// switches their host code reads are members of g_sw, srukf_switches.h).  Included by srukf_ctx.h (the callers) and, behind their own headers, by the eight files that define these functions (srukf_predict,
// srukf_factor, srukf_gmw_persist, srukf_rank, srukf_mixed, srukf_augment, srukf_assoc, srukf_unique): linkage is C, so only the compiler can compare a declaration
// with its definition, and it does so in the file that defines it.  A function of this kind is declared here and nowhere else (tests/test_host.py holds the tree to it).
// srukf_joint.hip's launchers (launch_joint_*, C++ linkage) are declared at the end.
#pragma once
#include "srukf_device.h"
#include "srukf_rank.h"
#include "srukf_patch.h"       // the appearance record's sizes, MatchArgs

struct GmwPanel64;      // srukf_gmw_panel.h: the hand-off buffer of one 64-row panel
struct GmwTile;         // srukf_gmw_persist.hip: one entry of a persistent launch's tile list (4 shorts)

// ---- argument structs of the launchers whose lists nobody can read: plain aggregates, filled by name at the call site, unpacked into the kernel call ----

// One blocked factorisation G (upper triangle, destroyed) -> factor rows in Sout, as every form of it is launched (persistent, split pair, one launch per panel).
// pans / sync / tiles / ntiles / workers / relay: the plan's (GmwPlan); Tp: pivoted panels (<= 0: all ld / 64), krows: where the kept pivots end (<= 0: ld) — see
// gmw_normalised; gate_limit > 0: behind the admission gate (k_gmw_gate) for that many tenants
struct GmwLaunch {
    int n, ld; double eps;
    double* G; GmwPanel64* pans; double* D; double* Sout; GmwSync* sync;
    const GmwTile* tiles; int ntiles, workers;
    FrameScalars* fs;
    int Tp, krows, gate_limit, relay;
};
inline GmwLaunch gmw_normalised(GmwLaunch g)
{
    const int T = g.ld / 64;
    if (g.Tp <= 0 || g.Tp > T) g.Tp = T;
    if (g.krows <= 0 || g.krows > g.ld) g.krows = g.ld;
    return g;
}
// fused form of the persistent launch: the owners form their tiles of S0^T S0 - Ut0[u0:u1]^T Ut0[u0:u1] themselves (k_gmw_persist)
struct GmwFused { const double* S0; const double* Ut0; int u0, u1; };

// The riders of a k_syrk launch: the pending state update X += dX (dxp: slice partials or per-landmark shares; xr1: the robot mean after the motion step) and the
// rank-aware replay's operands (ra.A != null: S / Ut are the permuted operands, the dropped diagonal is formed too).  Empty: the plain product
struct SyrkRider { const double* dxp; double* X; RankArgs ra; const double* xr1; };

// k_gain: U^T, the gains and the slice partials of the state update.  z_cur / m_cur: this frame's measurements and matches (null: the staged sequence's z_seq / m_seq);
// Cm != null: the motion step's columns are committed here; P1 != null: the cross covariances are k_pxy2's (second K half, cut at split_b0); fmode: "fused tail" mode
// (the robot rows are re-centred); next_pose (3 doubles, host) with odo_dev: the launch also stores the sequence's third pose
struct GainLaunch {
    KDims d; KWeights w;
    double* Ut; const double* PxyR; const double* Si; const int* vis; const double* h;
    const double* z_seq; const double* z_cur; const int* m_seq; const int* m_cur;
    FrameScalars* fs; double* dxp; const double* Z; RankArgs ra;
    const double* Cm; double* S; const double* P1; int split_b0; const double* DZp; double sqeps; const double* sigR;
    bool fmode; const double* next_pose; double* odo_dev;
};

// k_rank_expand, the tail of a rank-aware refactorisation: factor rows Sp (permuted order) -> S and the permuted copy A, theta / null-direction checks.
// do_traj: it ends a frame (trajectory row, frame counter); sigR != null: it prepares the next frame's table of robot poses; fuse: "fused tail" mode, it projects
// the next frame into Z / DZ (k_rank_expand<2>) and then may round what it writes (f32round), export the step-wise frame's status (step_export) and clear the gain
// fold's sync words (fold_sync); null_rel: what the null-direction check allows relative to G_aa
struct RankExpandLaunch {
    KDims d; KWeights w; srukf_params p;
    int r;
    const double* Sp; const double* D; const int* perm; const int* iperm; const double* gdiag; FrameScalars* fs; const double* X;
    double* S; double* A; double* sigR; double* Z; double* DZ;
    bool do_traj, fuse, f32round;
    const StepExport* step_export; double null_rel; unsigned int* fold_sync; int fold_words;
};

// k_associate_staged: the staged image stack and where frame fs->frame's rows go (frames: how many the stack and every per-frame array hold)
struct StagedAssoc {
    const unsigned char* images; int frames;
    double* z_seq; int* m_seq; double* corr_seq; int* vis_seq; double* h_seq;
    const FrameScalars* fs;
};
// k_associate_checked_staged: k_associate_staged's addressing (rec), the checked record beside it (corr2_seq, flags_seq stride N, z2_seq stride 2N), the filter's score
// buffer (PT_SCORE_STRIDE doubles per landmark: the last frame's maps) and the parameters on the device (ma: written in stream order, srukf_launch_set_match_args)
struct StagedChecked {
    StagedAssoc rec;
    double* corr2_seq; double* z2_seq; int* flags_seq; double* scores;
    const MatchArgs* ma;
};

// The archive search behind every frame of an image run (srukf_images_search_archive).  ArchiveArgs: srukf_archive_search's parameters on the
// device, written in stream order in front of a run (MatchArgs' pattern).  ImageArchiveRecord: the per-frame record, one allocation — h [F][2L] | Si [F][4L] |
// z [F][2L] | corr [F][L] (offsets in doubles), then from `ints` (in doubles) on, as ints: visible [F][L] | matched [F][L] | hits [F]; `doubles`: its size.
// StagedArchive: what k_archive_search_staged takes of it — the staged image stack, the record's arrays, the frame counter (the frame searched is fs->frame - 1: the
// frame tail has advanced it), the parameters
struct ArchiveArgs { int half_cap; double corr_threshold, chi2; };
struct ImageArchiveRecord { size_t h, Si, z, corr, ints, vis_i, m_i, hits_i, doubles; };
constexpr ImageArchiveRecord image_archive_record(size_t F, size_t L)
{
    return { .h = 0, .Si = 2 * F * L, .z = 6 * F * L, .corr = 8 * F * L, .ints = 9 * F * L, .vis_i = 0, .m_i = F * L, .hits_i = 2 * F * L, .doubles = 9 * F * L + (2 * F * L + F + 1) / 2 };
}
struct StagedArchive {
    const unsigned char* images; int frames;
    double* h_seq; double* Si_seq; double* z_seq; double* corr_seq; int* vis_seq; int* m_seq; int* hits;
    const FrameScalars* fs; const ArchiveArgs* args;
};

extern "C" {
// ---- srukf_predict.hip ----
void srukf_launch_landmarks_cartesian(hipStream_t st, KDims d, const double* X, const double* S, double* xyz, double* cov);
void srukf_launch_motion(hipStream_t st, KDims d, KWeights w, srukf_params p, double* X, double* S, double* sigR, double* Cmat, FrameScalars* fs, const double* odo_seq,
                         const double* odo_pair, RankArgs ra);
void srukf_launch_project_motion(hipStream_t st, KDims d, KWeights w, srukf_params p, double* X, double* S, double* sigR, double* Cm, double* Z, double* DZ, FrameScalars* fs,
                                 RankArgs ra);
void srukf_launch_project_table(hipStream_t st, KDims d, KWeights w, srukf_params p, double* X, double* S, double* sigR, double* Cm, double* Z, double* DZ, FrameScalars* fs,
                                RankArgs ra, NullSkip ns);
void srukf_launch_sigr_rows(hipStream_t st, KDims d, KWeights w, const double* X, const double* S, double* sigR, const FrameScalars* fs, const int* iperm, int rkeep);
void srukf_launch_project(hipStream_t st, KDims d, KWeights w, srukf_params p, const double* X, const double* S, const double* sigR, double* Z, double* DZ, const FrameScalars* fs);
void srukf_launch_meas_stats(hipStream_t st, KDims d, KWeights w, const double* X, const double* sigR, const double* Z, double* part, double* h, double* Si, int* vis, double* PxyR);
int srukf_meas_part_doubles(int mp);
void srukf_launch_gain(hipStream_t st, const GainLaunch& a);
void srukf_launch_gain_b(hipStream_t st, KDims d, KWeights w, const GainArgs* tab, int B, int split_b0, double sqeps);
int srukf_gain_part_doubles(int np);
void srukf_launch_traj(hipStream_t st, KDims d, const double* X, const double* S, FrameScalars* fs, double* traj, int advance);
void srukf_launch_block_cov(hipStream_t st, KDims d, const double* S, int off, int bs, double* out, const double* X);
// ... for K landmarks in one launch: the 6 x 6 block of landmark ids[q] (device table, each in [0, N)) into out + 36 q
void srukf_launch_block_cov_many(hipStream_t st, KDims d, const double* S, const int* ids, int K, double* out);
void srukf_launch_project_points(hipStream_t st, srukf_params p, int count, const double* feat6, const double* pos3, const double* psi, const double* err2, double* out);

// ---- srukf_factor.hip ----
void srukf_launch_pxy(hipStream_t st, KDims d, const double* DZ, const double* S, double* Ut, const int* tiles, int ntiles, KWeights w, MeasArgs ms);
void srukf_launch_pxy2(hipStream_t st, KDims d, const double* DZp, const double* A, double* P0, double* P1, const int* tiles, int ntiles, int kr, KWeights w, MeasArgs ms, GainFold gf);
int srukf_pxy2_build_tiles(int mp, int np, int kr, int* out);
int srukf_pxy2_split_groups(void);
void srukf_launch_syrk(hipStream_t st, KDims d, const double* S, const double* Ut, int ub, int ue, double* G, FrameScalars* fs, const int* tiles, int ntiles, const SyrkRider& rider);
void srukf_launch_gmw_step64(hipStream_t st, int n, int ld, int j0, double eps, double* G, const GmwPanel64* cur, GmwPanel64* nxt, double* D, double* Sout, const FrameScalars* fs);
int srukf_gmw_panel_bytes(void);
void srukf_launch_gmw_pivslab_b(hipStream_t st, int n, int ld, int j0, double eps, const Step64Args* tab, int B, int flip, int sel);
void srukf_launch_gmw_trail_b(hipStream_t st, int ld, int j0, const Step64Args* tab, int B, int rows, int sel, int form);
int srukf_pxy2_b_per(int ntiles, int gx);
void srukf_launch_pxy2_b(hipStream_t st, KDims d, const Pxy2Args* tab, int B, const int* tiles, int ntiles, int kr, KWeights w, int gx);
void srukf_launch_syrk_b(hipStream_t st, KDims d, const SyrkArgs* tab, int B, const int* tiles, int ntiles, int krows, int ndx, int ngd);
void srukf_launch_gmw_step64_b(hipStream_t st, int n, int ld, int j0, double eps, const Step64Args* tab, int B, int rows, int flip);
void srukf_launch_gmw_check(hipStream_t st, int n, int ld, const double* D, const double* S, FrameScalars* fs, const double* X, int do_traj, double* Scopy);
void srukf_warm_exact_path(hipStream_t st, FrameScalars* fs);
void srukf_launch_gmw_col(hipStream_t st, int n, int ld, int j, double eps, const double* G, double* Wf, double* D, unsigned long long* theta_bits, FrameScalars* fs, double* Sout);
void srukf_launch_gmw_stats(hipStream_t st, int n, int ld, const double* G, FrameScalars* fs);

// ---- srukf_gmw_persist.hip ----
int srukf_gmw_sync_bytes(int T);
int srukf_gmw_build_tiles(int T, int Tp, short* out);
int srukf_gmw_get_pivot_relay(void);
int srukf_gmw_persist_workers(int T, int Tp, int max_workers);
int srukf_gmw_register_form(int T, int Tp, int ntiles, int workers);
// fused / head: null = every tile is read from G / no helper workgroups (head fold)
void srukf_launch_gmw_persist(hipStream_t st, const GmwLaunch& g, const GmwFused* fused, const HeadArgs* head);
void srukf_launch_syrk_own(hipStream_t st, int n, int ld, const double* S0, const double* Ut0, int u0, int u1, int krows, double* G, FrameScalars* fs, const GmwTile* tiles, int ntiles, int Tp);
void srukf_launch_syrk_own_b(hipStream_t st, int n, int ld, const SyrkOwnArgs* tab, int B, int u0, int u1, int krows, const GmwTile* tiles, int ntiles, int Tp);
// the split pair: stA = the filter's stream (pivot / slab launch), stB = its side stream (gate + tile launch); Wslab / Lslab: the slabs of every pivoted panel
void srukf_launch_gmw_split(hipStream_t stA, hipStream_t stB, const GmwLaunch& g, double* Wslab, double* Lslab, int starve);
void srukf_launch_gmw_split_alone(hipStream_t st, int which, const GmwLaunch& g, double* Wslab, double* Lslab);
// ... whose tile launch forms tiles too: list / nlist = its grid (srukf_gmw_build_fold_list) in place of g.tiles, A / Ut (mp rows) = the operands k_syrk would have read
void srukf_launch_gmw_split_fold(hipStream_t stA, hipStream_t stB, const GmwLaunch& g, double* Wslab, double* Lslab, const GmwTile* list, int nlist, const double* A, const double* Ut, int mp);
int srukf_gmw_fold_head_rows(int Tp);
int srukf_gmw_fold_head_tile(int tr, int tc, int head_rows);
int srukf_gmw_build_fold_list(int T, int Tp, short* out);
int srukf_gmw_head_rows(void);
int srukf_gmw_head_extra_diag(void);

// ---- srukf_rank.hip ----
void srukf_launch_rank_round(hipStream_t st, int ld, int r, double* A);
void srukf_launch_row_energy(hipStream_t st, int n, int ld, const double* S, double* e);
void srukf_launch_rank_diag(hipStream_t st, int n, int ld, const double* G, const int* perm, double* gdiag);
void srukf_launch_rank_expand(hipStream_t st, const RankExpandLaunch& a);
void srukf_launch_rank_expand_b(hipStream_t st, int n, int ld, int r, double eps, const ExpandArgs* tab, int B, double gamma, KDims d, KWeights w, srukf_params p);
void srukf_launch_rank_canon(hipStream_t st, int n, int ld, int r, double sq, const int* perm, double* S);
void srukf_launch_rank_shadow(hipStream_t st, int n, int ld, int r, const double* S, const int* perm, double* A);

// ---- srukf_mixed.hip (tasks / tiles / planes: the lists and operand planes of srukf_mixed_build_tasks* and k_split_bf3, opaque to the host) ----
int srukf_mixed_build_tasks_red(int np, int ue, int krows, int rows_lim, short* out_tasks, int* out_tiles, int* ntiles);
int srukf_mixed_build_tasks(int np, int ue, short* out_tasks, int* out_tiles, int* ntiles);
int srukf_mixed_krows(int r);
size_t srukf_mixed_part_bytes(int ntasks);
void srukf_launch_cvt_f32(hipStream_t st, size_t count, const double* src, float* dst);
void srukf_launch_gain_dx(hipStream_t st, int n, int np, const double* dxp, double* X, const double* xr1);
void srukf_launch_cvt_robot_cols(hipStream_t st, int n, int np, const double* S, float* S32);
void srukf_launch_syrk32(hipStream_t st, int n, int np, int ue, const float* S32, const float* U32, const void* tasks, int ntasks, const void* tiles, int ntiles, double* part,
                         double* G, FrameScalars* fs, int krows);
void srukf_launch_split_bf3(hipStream_t st, int rows, int ld, int ktot, int koff, const double* src, void* planes, size_t plane_stride);
void srukf_launch_syrk_bf3(hipStream_t st, int n, int np, int ue, int krows, int ktot, const void* planes, size_t plane_stride, const void* tasks, int ntasks, const void* tiles,
                           int ntiles, double* part, double* G, FrameScalars* fs);

// ---- srukf_augment.hip ----
void srukf_launch_aug_map(hipStream_t st, srukf_params p, int dim, int ld, int K, int Na, double gamma, const double* X, const double* S, const double* uv, double* ang);
void srukf_launch_aug_x(hipStream_t st, int dim, int K, int Na, double wm0, double wi, const double* X, const double* ang, const int* perm, double* mu_ang, double* Xn, int dimn, int ldn);
void srukf_launch_aug_build(hipStream_t st, int dim, int ld, int K, int Na, double gamma, double wi_sr, const double* X, const double* S, const double* ang, double* A, int rows_p,
                            int dimn, int ldn);
void srukf_launch_gram(hipStream_t st, int rows_p, int ld, const double* A, double* G);

// ---- srukf_assoc.hip, srukf_unique.hip ----
void srukf_launch_warp_patch(hipStream_t st, KDims d, srukf_params p, const double* X, const double* xyz, const double* h, const double* appR, const double* appT,
                             const double* appPx, const unsigned char* initPatch, const int* has_app, unsigned char* matchPatch);
void srukf_launch_associate(hipStream_t st, KDims d, srukf_params p, const unsigned char* image, const double* h, const double* Si, const int* vis, const int* has_app,
                            const unsigned char* matchPatch, double* z, int* matched, double* corr);
// k_associate_staged (image runs of the staged replay): frame fs->frame of the staged images [frames][image_h][image_w] is searched; z / matched go into that frame's
// rows of the staged sequence (z_seq stride 2N, m_seq stride N), corr / visible / the predicted pixels into the record's (corr_seq, vis_seq stride N, h_seq stride 2N)
void srukf_launch_associate_staged(hipStream_t st, KDims d, srukf_params p, StagedAssoc a, const double* h, const double* Si, const int* vis, const int* has_app,
                                   const unsigned char* matchPatch);
// res / scores: the packed result block and the score buffer (match_res, PT_SCORE_*: srukf_patch.h)
void srukf_launch_associate_checked(hipStream_t st, KDims d, srukf_params p, MatchArgs ma, const unsigned char* image, const double* h, const double* Si, const int* vis,
                                    const int* has_app, const unsigned char* matchPatch, double* z, int* matched, double* corr, double* res, double* scores);
// k_associate_checked_staged (checked image runs): k_associate_checked with k_associate_staged's addressing; srukf_launch_set_match_args: *dst = v on the stream
void srukf_launch_associate_checked_staged(hipStream_t st, KDims d, srukf_params p, StagedChecked a, const double* h, const double* Si, const int* vis, const int* has_app,
                                           const unsigned char* matchPatch);
void srukf_launch_set_match_args(hipStream_t st, MatchArgs* dst, MatchArgs v);
}  // extern "C"

// ---- srukf_joint.hip (the joint measurement update; C++ linkage: its launchers are named launch_joint_*) ----
// Zd: joint_dev_rows(Na) x mp, W: mp x joint_work_ld(mp, np) = [ Pzz | Pxy^T | z - h ], Rd: mp x 64 (the factored diagonal blocks), status: one int (0, or 1 + the row
// of the first non-positive pivot / non-finite innovation; cleared by the form launch).  form: W from Z and k_pxy's products (Ut raw, PxyR); factor: the blocked Cholesky,
// two launches per 64-row panel, leaves R, U^T and w in W; dx: X += U w, U^T -> Ut in state order and -> ra.Utp with permuted columns (ra.Utp != null: what k_gain leaves
// for the frame-tail forms on the permuted operands), the gamma / xi accumulators cleared for the k_syrk launch that follows; a set status word: zero U^T, X untouched,
// fs->joint_bad_frame / joint_bad_row (first hit only).
// JointFrame: whose measurements — z_cur / m_cur (the step-wise call's, on the device), or null: the rows of frame fs->frame in the staged z_seq / m_seq, as k_gain reads them
struct JointFrame { const double* z_cur; const int* m_cur; const double* z_seq; const int* m_seq; const FrameScalars* fs; };
int joint_dev_rows(int Na);
int joint_work_ld(int mp, int np);
void launch_joint_form(hipStream_t st, KDims d, KWeights w, const JointFrame& f, const double* Z, const int* vis, const double* Si, const double* Ut, const double* PxyR, const double* h,
                       double* Zd, double* W, int* status);
void launch_joint_factor(hipStream_t st, KDims d, double* W, double* Rd, int* status);
void launch_joint_dx(hipStream_t st, KDims d, double* W, const double* Rd, const int* status, double* Ut, double* X, FrameScalars* fs, const RankArgs& ra);

// ---- srukf_archive.hip (the search behind the frames of an image run; C++ linkage) ----
// k_archive_search_staged: k_archive_search (one text of its body) on frame fs->frame - 1 of the staged images, L workgroups; h / Si / vis / tmpl: the archive's own
// arrays as k_archive_predict and k_warp_patch left them.  launch_set_archive_args: *dst = v on the stream
void launch_archive_search_staged(hipStream_t st, int L, srukf_params p, StagedArchive a, const double* h, const double* Si, const int* vis, const unsigned char* tmpl);
void launch_set_archive_args(hipStream_t st, ArchiveArgs* dst, ArchiveArgs v);

// ---- srukf_policy.hip (the map policy's verdict; C++ linkage) ----
// k_map_policy: one workgroup of 256 threads; X: the state (landmark k at 6k, the robot block last), h / vis / z / m: one frame's association, state / verdict [N] and
// *sum: what it writes; prm: the parameters on the device.  k_map_policy_staged: the same body on row `frame` of the association's record (StagedPolicy: the record's
// arrays, the policy state, the verdict rows [frames][N] and the summary rows [frames]); launch_set_policy_params: *dst = v on the stream
struct StagedPolicy {
    const double* X; int frames;
    const double* h_seq; const int* vis_seq; const double* z_seq; const int* m_seq;
    srukf_policy_state* st; int* verdict; srukf_policy_summary* sum;
};
void launch_map_policy(hipStream_t st, KDims d, srukf_params p, const srukf_policy_params* prm, const double* X, const double* h, const int* vis, const double* z, const int* m,
                       srukf_policy_state* state, int* verdict, srukf_policy_summary* sum);
void launch_map_policy_staged(hipStream_t st, KDims d, srukf_params p, const srukf_policy_params* prm, StagedPolicy a, int frame);

// ---- srukf_ransac.hip (the consensus inside the frames of an image run; C++ linkage) ----
// k_ransac_votes_staged (N workgroups) + k_ransac_pick_staged (one): k_ransac_votes / k_ransac_pick (one text of each body) on row fs->frame of the staged z_seq /
// m_seq, with the context's live Ut (S^T DZ behind seq_pxy(FORM_PLAIN)), PxyR, h, Si, vis, X.  StagedRansac: the rows, the frame counter, the threshold on the device
// (args: written in stream order, launch_set_ransac_args), the scratch (D [N][N], F [N][N] bytes, votes [N]) and the record (rec_flags / rec_votes / rec_dist
// [frames][N], rec_sum [frames]).  The pick launch rewrites the frame's m_seq row to the inlier mask
struct RansacArgs { double threshold; };
struct RansacSummary { int best, n_active, n_low, outlier; };
struct StagedRansac {
    int frames; const double* z_seq; int* m_seq; const FrameScalars* fs; const RansacArgs* args;
    double* D; unsigned char* F; int* votes;
    int* rec_flags; int* rec_votes; double* rec_dist; RansacSummary* rec_sum;
};
void launch_ransac_staged(hipStream_t st, KDims d, KWeights w, srukf_params p, StagedRansac a, const double* X, const double* Ut, const double* PxyR, const double* h,
                          const double* Si, const int* vis);
void launch_set_ransac_args(hipStream_t st, RansacArgs* dst, RansacArgs v);
// ---- srukf_rescue.hip (the rescue gate; C++ linkage) ----
// k_rescue_gate (step-wise) / k_rescue_gate_staged (behind the tail of a frame of an image run): one body, N workgroups of 256.  Landmark k is a candidate when its
// frame has any (n_active >= 2, 0 < n_low < n_active) and it is in A and no low-innovation inlier; its workgroup forms h', Si', visible' of
// srukf_repredict_measurement for the posterior (X, S) and the chi-square test of dataAssociation (1977); every other workgroup zeroes its entry.  RescueRow: one
// frame's row of the record (flags: bit 0 candidate, bit 1 rescued; h2 [2N]; Si2 [4N]; chi2 [N]: y0^2 + y1^2, 0 where it was not formed).  RescueScratch: what
// meas_final_tail stores besides (vis [N], PxyR [5 mp]).  StagedRescue: the staged rows, the consensus record the candidates come from, the frame counter (the tail
// has advanced it: the frame is fs->frame - 1), the threshold on the device (args: written in stream order, launch_set_rescue_args) and the record, rec_sum
// [frames] written by k_rescue_sum_staged (one workgroup behind the gate: integer counts of the row)
struct RescueArgs { double chi2; };
struct RescueSummary { int n_cand, n_high; };
struct RescueRow { int* flags; double* h2; double* Si2; double* chi2; };
struct RescueScratch { int* vis; double* PxyR; };
struct StagedRescue {
    int frames; const double* z_seq; const FrameScalars* fs; const RescueArgs* args;
    const int* rs_flags; const RansacSummary* rs_sum;
    RescueRow rec; RescueSummary* rec_sum; RescueScratch scr;
};
void launch_rescue_gate_staged(hipStream_t st, KDims d, KWeights w, srukf_params p, StagedRescue a, const double* X, const double* S);
// frame_has: the caller's matched / inlier hold a frame with candidates (the rule above); cand[k] = frame_has && matched[k] && !inlier[k]
void launch_rescue_gate(hipStream_t st, KDims d, KWeights w, srukf_params p, const double* X, const double* S, const double* z, const int* matched, const int* inlier,
                        int frame_has, double chi2, RescueRow row, RescueScratch scr);
void launch_set_rescue_args(hipStream_t st, RescueArgs* dst, RescueArgs v);
void launch_set_policy_params(hipStream_t st, srukf_policy_params* dst, srukf_policy_params v);

// ---- srukf_snapshot.hip (the state a block of image frames is resumed from; C++ linkage) ----
// k_image_snapshot, the first launch of a frame with the snapshot bit: while no stop of the block is on record in front of frame fs->frame (the latch, see the file),
// X, S, the matchPatch array and the policy state go into slot (frame & 1), and tag[slot] = frame.  SnapshotArgs: what the guard reads, on the device, written in
// stream order in front of every run (launch_set_snapshot_args; begin: the run begins a block — tags -1, latch open): the block's first frame, the summaries of the
// policy and the consensus (null: this run has none) and the policy state (null: not allocated).  SnapshotCtl: the two tags and the latch.  ImageSnapshot: the live
// arrays, their sizes in bytes and the two slots; the grid is sized by S (image_snapshot_blocks: SNAPSHOT_TRIPS 16-byte trips per lane, at most SNAPSHOT_MAX_BLOCKS)
struct SnapshotArgs { int b0; const srukf_policy_summary* pol_sum; const RansacSummary* rs_sum; const srukf_policy_state* pol_state;
                      const RescueSummary* rq_sum; };      // rq_sum (the rescue gate is on): the consensus term is "frame f - 1 rescued a match"
struct SnapshotCtl { int tag[2]; int latch[2]; };
struct ImageSnapshot {
    const double* X_src; const double* S_src; const unsigned char* tmpl_src;
    size_t X_bytes, S_bytes, tmpl_bytes, pol_bytes;
    double* X[2]; double* S[2]; unsigned char* tmpl[2]; srukf_policy_state* pol[2];
};
#ifndef SRUKF_SNAPSHOT_TRIPS                                     // (measurement builds name other grids: DESIGN.md section 25)
#define SRUKF_SNAPSHOT_TRIPS 4
#define SRUKF_SNAPSHOT_MAX_BLOCKS 1024
#endif
constexpr int SNAPSHOT_TRIPS = SRUKF_SNAPSHOT_TRIPS, SNAPSHOT_MAX_BLOCKS = SRUKF_SNAPSHOT_MAX_BLOCKS;
int image_snapshot_blocks(size_t S_bytes);
void launch_image_snapshot(hipStream_t st, const FrameScalars* fs, const SnapshotArgs* args, SnapshotCtl* ctl, const ImageSnapshot& sn);
void launch_set_snapshot_args(hipStream_t st, SnapshotArgs* dst, SnapshotArgs v, SnapshotCtl* ctl, int begin);

// ---- srukf_predict.hip (the display view behind the frames of an image run; C++ linkage) ----
// k_image_view, N + 1 workgroups: k_landmarks_cartesian's body per landmark into xyz [3N] / cov [9N], k_block_cov's body for the robot block into robot [20]
// (P4 | pose), and the innovation factors Si [4N] as the frame's association read them into Si_row [4N].  The output pointers are one frame's rows of the
// display record (ImageDisplayRow, srukf_ctx.h): the host computes them, the kernel knows no frame index
void launch_image_view(hipStream_t st, KDims d, const double* X, const double* S, const double* Si, double* xyz, double* cov, double* robot, double* Si_row);

// ---- srukf_loop.hip, srukf_map.hip (deleting several landmarks in one call; C++ linkage) ----
// the records of K landmarks, two launches of K workgroups: k_block_cov (srukf_launch_block_cov_many) leaves the 6 x 6 blocks of P = S^T S at 6 ids[q] in P66 [K][36],
// k_lm_records packs landmark ids[q]'s record (k_lm_record's body: X6 | S66 | R | t | px | has_app | patch, SRUKF_LM_RECORD_DOUBLES doubles) at
// out + q * SRUKF_LM_RECORD_DOUBLES.  ids on the device, each in [0, N)
void launch_lm_records(hipStream_t st, int K, KDims d, const double* S, const double* X, const int* ids, double eps, const unsigned char* app_patch, const double* appR,
                       const double* appT, const double* appPx, const int* has_app, double* P66, double* out);
// k_appearance_gather, M workgroups of 64: the appearance record of landmark src_of[a] of one map-size scope (AppearanceArrays: initPatch at PT_PATCH_STRIDE,
// matchPatch at PT_TMPL_STRIDE, R [9], t [3], px [2], has_app) becomes the one of landmark a of another, a < M; the two byte arrays move in 16-byte accesses.
// src_of on the device, each entry inside the source's arrays
struct AppearanceArrays { unsigned char* patch; unsigned char* tmpl; double* R; double* T; double* px; int* has; };
void launch_appearance_gather(hipStream_t st, int M, const int* src_of, AppearanceArrays src, AppearanceArrays dst);
