// srukf_replay.hip — the launch sequences of a frame (seq_*: which kernels run, in which order, for which launch plan), the rank-aware null set, the graph cache
// and the staged replay (srukf_stage_sequence / srukf_run_frames*: the OnBnClickedAuto loop of MonoSLAMView.cpp:526-572 with inputs resident in HBM).
// Also the small host-layer kernels (frame scalars, permutations, rounding) behind their launchers.  The image runs of the staged replay (srukf_run_images*)
// are srukf_images.hip's; what it takes from here is declared in srukf_ctx.h under a heading of its own.

#include "srukf_ctx.h"
using namespace srukf_impl;

// resets the per-refactor accumulators (theta row maxima, gamma/xi)
__global__ void k_refactor_reset(int np, unsigned long long* theta_bits, FrameScalars* fs, int reset_stats)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < np) theta_bits[i] = 0ull;
    if (i == 0 && reset_stats) { fs->gmax_bits = 0ull; fs->ximax_bits = 0ull; }
}

// staged sequence: what srukf_prepare_control needs to prepare the control of a frame on the device
__global__ void k_set_seq(FrameScalars* fs, const double* odo_seq, int seqF, double a1, double a2, double a3, double a4)
{
    fs->odo_seq = odo_seq; fs->seqF = seqF;
    fs->a[0] = a1; fs->a[1] = a2; fs->a[2] = a3; fs->a[3] = a4;
}

// start of a staged replay, or of a single frame outside one (traj_base null): frame counter, flags and trajectory base in one launch
__global__ void k_set_run(FrameScalars* fs, int frame, int clear_clamp, double* traj_base)
{
    fs->frame = frame;
    srukf_prepare_control(fs);                                 // the first frame's control (k_project_motion); later ones by the frame tails
    fs->stat_count = 0;
    fs->const_rows_ok = 0; fs->const_rows_pending = 0;         // whatever happened to S since the last staged frame: its first tail writes every row again
    for (int q = 0; q < SRUKF_STAT_GROUPS; q++) fs->stat_cnt[q] = 0;
    fs->traj_base = traj_base;
    if (clear_clamp) { fs->clamp_rows = 0; fs->clamp_first = 0x7fffffff; fs->clamp_frame = 0x7fffffff; fs->frozen = 0; fs->gmw_aborts = 0; fs->joint_bad_frame = 0; fs->joint_bad_row = 0; }
}

// Step-wise API, fast path: start of a frame.  odo = (prev, cur[, next]) poses on the device: a staged sequence of one (two) frames the frame scalars point at.
// fresh: nothing prepared this frame (the control, the flags of the constant rows); otherwise the previous frame's tail prepared fs->ctl and projected the frame.
// (the poses arrive as kernel arguments and are written to the device buffer here: a 72-byte host-to-device copy in front of the frame's first launch cost 12 us of stream
//  time — 4.5 for the blit kernel, 7.5 of gap behind it; scripts/profile_step.sh)
struct StepPoses { double v[9]; };
__global__ void k_set_step(FrameScalars* fs, double* odo, int seqF, double a1, double a2, double a3, double a4, int fresh, StepPoses po)
{
    for (int e = 0; e < 9; e++) odo[e] = po.v[e];
    const double a[4] = { a1, a2, a3, a4 };
    srukf_step_scalars(fs, odo, seqF, a);
    if (fresh) { srukf_prepare_control(fs); fs->const_rows_ok = 0; fs->const_rows_pending = 0; }
}

__global__ void k_set_frame_control(FrameScalars* fs) { srukf_prepare_control(fs); }
// Small results for the host (h | Si | visible after the predict half; frame scalars + robot view after the update half) written straight into its pinned buffer by a kernel:
// a hipMemcpyAsync of a few KB is a blit kernel plus ~7.5 us of gap behind it on the stream (scripts/profile_step.sh); this is one short launch.  Two segments, 8-byte words.
// flag (may be null): a word of the same pinned buffer that receives `seq` AFTER the data — every wave's stores made visible at system scope first — so that the host can
// spin on it instead of going through hipStreamSynchronize (one workgroup then: the flag needs a barrier over all stores).
__global__ __launch_bounds__(256) void k_export(const unsigned long long* __restrict__ a, int na, const unsigned long long* __restrict__ b, int nb, unsigned long long* __restrict__ dst,
                                                unsigned long long* flag, unsigned long long seq)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < na + nb; i += gridDim.x * 256) dst[i] = i < na ? a[i] : b[i - na];
    if (flag) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ... and the commit of its motion step on demand (a state getter or srukf_associate between predict and update; a frame without a match): what k_gain does with Cmat /
// the state update with fs->Xr1 — the new last four columns of S (and of the permuted copy), the new robot mean.  Idempotent: k_gain / the update write the same values again.
__global__ __launch_bounds__(256) void k_commit_motion(int n, int ld, double* __restrict__ X, double* __restrict__ S, const double* __restrict__ Cm, const FrameScalars* __restrict__ fs,
                                                       double* __restrict__ A, const int* __restrict__ iperm, int rk)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const double4 v = *reinterpret_cast<const double4*>(Cm + (size_t)r * 4);
    *reinterpret_cast<double2*>(S + (size_t)r * ld + (n - 4)) = make_double2(v.x, v.y);
    *reinterpret_cast<double2*>(S + (size_t)r * ld + (n - 2)) = make_double2(v.z, v.w);
    if (A) {
        const int arow = (r < n - 4) ? iperm[r] : rk - 4 + (r - (n - 4));
        if (arow < rk) { double* o = A + (size_t)arow * ld + (rk - 4); o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
    }
    if (r >= n - 4) X[r] = fs->Xr1[r - (n - 4)];
}

// dst = P^T src P on the upper triangle of a symmetric matrix stored upper: dst[a][b] = src[ip[a]][ip[b]] (a <= b),
// ip[a] = the row r of the source with perm[r] = a.  forward = 0 swaps the roles (dst[r][c] = src[perm[r]][perm[c]]).
// Entries outside the upper n x n part are zeroed.
// The same kernel compacts a covariance when landmarks leave the state (map skips their indices, lds > ld).
__global__ __launch_bounds__(256) void k_sym_permute(int n, int ld, const double* __restrict__ src, int lds, double* __restrict__ dst,
                                                     const int* __restrict__ map)
{
    const int a = blockIdx.x;
    for (int b = threadIdx.x; b < ld; b += 256) {
        double v = 0.0;
        if (a < n && b < n && b >= a) {
            const int r = map[a], c = map[b];
            v = (r <= c) ? src[(size_t)r * lds + c] : src[(size_t)c * lds + r];
        }
        dst[(size_t)a * ld + b] = v;
    }
}

__global__ __launch_bounds__(256) void k_gather(int n, int ld, const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ map)
{
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a < ld) dst[a] = (a < n) ? src[map[a]] : 0.0;
}

// "bottom rows zero" of CholeskyDecompositionWithPivoting (SLAM.cpp:2161, 2176): rows >= rank of the disordered factor
__global__ __launch_bounds__(256) void k_zero_rows(int ld, int r0, double* __restrict__ A)
{
    const int r = r0 + blockIdx.x;
    for (int b = threadIdx.x; b < ld; b += 256) A[(size_t)r * ld + b] = 0.0;
}

// SRUKF_STORAGE_F32 (BASELINE configs[4]: fp32 filter state, fp64 arithmetic): the state that lives from frame to frame
// is X32 / S32; the fp64 working copies are rounded to the stored values at the end of every refactorisation, so the
// next frame computes from exactly what fp32 storage holds.  One workgroup per row of S (+ one for X).
__global__ __launch_bounds__(256) void k_quantize(int n, int ld, double* __restrict__ S, double* __restrict__ X,
                                                  float* __restrict__ S32, float* __restrict__ X32)
{
    const int r = blockIdx.x;
    if (r == n) {
        for (int c = threadIdx.x; c < n; c += 256) { const float f = (float)X[c]; X32[c] = f; X[c] = (double)f; }
        return;
    }
    for (int c = r + threadIdx.x; c < n; c += 256) {
        const float f = (float)S[(size_t)r * ld + c];
        S32[(size_t)r * ld + c] = f;
        S[(size_t)r * ld + c] = (double)f;
    }
}

namespace srukf_impl {
void launch_refactor_reset(hipStream_t st, int np, unsigned long long* theta_bits, FrameScalars* fs, int reset_stats) { hipLaunchKernelGGL(k_refactor_reset, dim3((np + 255) / 256), dim3(256), 0, st, np, theta_bits, fs, reset_stats); }
void launch_set_seq(hipStream_t st, FrameScalars* fs, const double* odo_seq, int seqF, const srukf_params& p) { hipLaunchKernelGGL(k_set_seq, dim3(1), dim3(1), 0, st, fs, odo_seq, seqF, p.a1, p.a2, p.a3, p.a4); }
void launch_set_run(hipStream_t st, FrameScalars* fs, int frame, int clear_clamp, double* traj_base) { hipLaunchKernelGGL(k_set_run, dim3(1), dim3(1), 0, st, fs, frame, clear_clamp, traj_base); }
void launch_set_step(hipStream_t st, FrameScalars* fs, double* odo, int seqF, double a1, double a2, double a3, double a4, int fresh, const double poses[9])
{
    StepPoses po; for (int e = 0; e < 9; e++) po.v[e] = poses[e];
    hipLaunchKernelGGL(k_set_step, dim3(1), dim3(1), 0, st, fs, odo, seqF, a1, a2, a3, a4, fresh, po);
}
void launch_export(hipStream_t st, const void* a, size_t bytes_a, const void* b, size_t bytes_b, void* host_pinned, unsigned long long* flag, unsigned long long seq)
{
    const int na = (int)((bytes_a + 7) / 8), nb = (int)((bytes_b + 7) / 8);
    const int blocks = flag ? 1 : ((na + nb + 255) / 256 > 8 ? 8 : (na + nb + 255) / 256);
    hipLaunchKernelGGL(k_export, dim3(blocks), dim3(256), 0, st, (const unsigned long long*)a, na, (const unsigned long long*)b, nb, (unsigned long long*)host_pinned, flag, seq);
}
void launch_set_frame_control(hipStream_t st, FrameScalars* fs) { hipLaunchKernelGGL(k_set_frame_control, dim3(1), dim3(1), 0, st, fs); }
void launch_commit_motion(hipStream_t st, int n, int ld, double* X, double* S, const double* Cm, const FrameScalars* fs, double* A, const int* iperm, int rk) { hipLaunchKernelGGL(k_commit_motion, dim3((n + 255) / 256), dim3(256), 0, st, n, ld, X, S, Cm, fs, A, iperm, rk); }
void launch_sym_permute(hipStream_t st, int n, int ld, const double* src, int lds, double* dst, const int* map) { hipLaunchKernelGGL(k_sym_permute, dim3(ld), dim3(256), 0, st, n, ld, src, lds, dst, map); }
void launch_gather(hipStream_t st, int n, int ld, const double* src, double* dst, const int* map) { hipLaunchKernelGGL(k_gather, dim3((ld + 255) / 256), dim3(256), 0, st, n, ld, src, dst, map); }

void quantize_state(srukf_ctx* c)
{
    if (c->storage != SRUKF_STORAGE_F64) hipLaunchKernelGGL(k_quantize, dim3(c->d.n + 1), dim3(256), 0, c->stream, c->d.n, c->d.np, c->S, c->X, c->S32, c->X32);
}

// rank-aware replay form: what k_motion / k_gain / k_syrk carry along (all null when the shadow copy does not exist)
// the pending state update as the launch that applies it takes it: k_gain's slice partials, or the per-landmark shares the gain fold of k_pxy2 left (RankArgs::dxN)
static const double* dx_src(const srukf_ctx* c) { return c->dx_pending ? (c->dx_lm ? c->dxk : c->dxp) : nullptr; }

RankArgs rank_args(const srukf_ctx* c)
{
    RankArgs ra = {};
    ra.dxN = (c->dx_pending && c->dx_lm) ? c->d.N : 0;
    if (c->red_r > 0 && c->shadowA) { ra.A = c->shadowA; ra.Utp = c->Utp; ra.gdiag = c->gdiag; ra.iperm = c->red_iperm; ra.perm = c->red_perm; ra.r = c->red_r; }
    return ra;
}

// ... as the launch that applies the state update in front of a frame tail takes them (the tail prepares the next table; "fused tail" on fp32 storage rounds)
RankArgs tail_rank_args(const srukf_ctx* c, FrameForm ff) { RankArgs ra = rank_args(c); ra.prep_next = ff.robot_table ? 1 : 0; ra.f32round = (ff.fused_tail() && storage_f32_like(c)) ? 1 : 0; return ra; }

// NullSkip of the "table" mode (all null: every direction is projected and read in full)
NullSkip null_skip(const srukf_ctx* c)
{
    NullSkip ns = {};
    if (c->dbg.nullskip && c->dbg.pxy2 && c->nskip && c->red_r > 0) {
        ns.dirs = c->nskip; ns.nulls = c->nskip + c->ns_full; ns.rows = c->nskip + c->ns_full + c->ns_null;
        ns.nfull = c->ns_full; ns.nnull = c->ns_null; ns.nrows = c->ns_rows; ns.iperm = c->red_iperm; ns.r = c->red_r;
    }
    return ns;
}

// fs->Xr1 for the launch that applies the pending state update (and only once)
static const double* take_xr1(srukf_ctx* c)
{
    if (!c->xr1_pending) return nullptr;
    c->xr1_pending = false;
    return (const double*)((const char*)c->fs + offsetof(FrameScalars, Xr1));
}

// Replay path: motion step + projection of all sigma points in ONE launch (k_project_motion): workgroup 0 is the motion step,
// whose results wait beside the state (fs->Xr1, Cmat) until k_gain / the dX job commit them.
void seq_predict_fused(srukf_ctx* c, FrameForm ff)
{
    const KDims& d = c->d;
    ProfScope ps(c, ff.robot_table ? KC_PROJECT_TABLE : KC_PROJECT_MOTION, 2.0 * 60.0 * d.Na * d.N + 60.0 * d.L, 8.0 * ((double)d.n * d.n / 2 + 2.0 * d.L * 2 * d.N + (double)d.n * 2 * d.N + 8.0 * d.L + 8.0 * d.n));
    RankArgs ra = rank_args(c);
    ra.dzperm = (ff.robot_table && ff.pxy2()) ? 1 : 0;          // (k_pxy2 reads DZ in permuted order)
    if (ff.robot_table) srukf_launch_project_table(c->stream, d, c->w, c->p, c->X, c->S, c->sigR, c->Cmat, c->Z, c->DZ, c->fs, ra, null_skip(c));
    else srukf_launch_project_motion(c->stream, d, c->w, c->p, c->X, c->S, c->sigR, c->Cmat, c->Z, c->DZ, c->fs, ra);
    c->xr1_pending = true;
}

void seq_predict_motion(srukf_ctx* c, const double* odo_pair_dev)
{
    const KDims& d = c->d;
    ProfScope ps(c, KC_MOTION, 60.0 * d.L, 8.0 * (4.0 * d.n + 8.0 * d.L + 4.0 * d.n));
    srukf_launch_motion(c->stream, d, c->w, c->p, c->X, c->S, c->sigR, c->Cmat, c->fs, c->odo_seq, odo_pair_dev, rank_args(c));
}

// (from MEAS_PLAIN on the statistics ride on the k_pxy launch of seq_gain: replay path, no host in between)
void seq_predict_measurement(srukf_ctx* c, FrameForm ff)
{
    const KDims& d = c->d;
    {
        ProfScope ps(c, KC_PROJECT, 2.0 * 60.0 * d.Na * d.N, 8.0 * ((double)d.n * d.n / 2 + 2.0 * d.L * 2 * d.N + (double)d.n * 2 * d.N));
        srukf_launch_project(c->stream, d, c->w, c->p, c->X, c->S, c->sigR, c->Z, c->DZ, c->fs);
    }
    if (!ff.fused_stats()) {
        ProfScope ps(c, KC_STATS, 30.0 * d.L * d.N, 8.0 * 3.0 * d.L * 2 * d.N);
        srukf_launch_meas_stats(c->stream, d, c->w, c->X, c->sigR, c->Z, c->mpart, c->h, c->Si, c->vis, c->PxyR);
    }
}

void shadow_rebuild(srukf_ctx* c)
{
    if (c->red_r > 0 && c->shadowA) srukf_launch_rank_shadow(c->stream, c->d.n, c->d.np, c->red_r, c->S, c->red_perm, c->shadowA);
}

// does a factorisation on plan gp run as persistent launch(es), or as one launch per 64-row panel?  (the filter at all: gmw_use_persist)
static bool gmw_plan_persists(const srukf_ctx* c, const GmwPlan& gp) { return gp.workers >= 0 || split_form(c, gp, true); }
static bool gmw_use_persist(const srukf_ctx* c) { return g_sw.gmw_persist && c->gmw_shared != 2 && gmw_plan_persists(c, c->gplan); }
bool plan_persists(const srukf_ctx* c, const GmwPlan& gp) { return gmw_use_persist(c) && gmw_plan_persists(c, gp); }

// SRUKF_GPU_SHARED: how many persistent launches share the GPU (each keeps to 1 / tenants of the CUs; the gate admits that many)
// (per context: srukf_run_frames_batch picks it from the number of filters it runs — one tenant per filter up to SRUKF_MAX_TENANTS; srukf_set_exclusive alone uses the
//  process-wide default of srukf_debug_set "shared_tenants")
static int plan_tenants(const srukf_ctx* c) { return c->gmw_shared == 1 ? c->shared_tenants : 1; }
int gate_limit(const srukf_ctx* c) { return c->gmw_shared == 1 ? c->shared_tenants : 0; }

// Tail of every rank-aware refactorisation: factor rows (c->G, permuted order) -> S and the permuted copy, checks, frame tail.
// fp32 storage: S, X and the permuted copy are rounded to the stored values first, and the trajectory row is taken from those
// (as the full-rank form does: quantize_state before the tail).
// ff.robot_table: the tail also prepares the next frame's table of robot poses (k_rank_expand)
// ff.fused_tail(): this launch also projects the next frame's sigma points (k_rank_expand<2>)
static void rank_expand(srukf_ctx* c, const RefactorRequest& rq, FrameForm ff)
{
    const int np = c->d.np;
    const bool frame_tail = rq.kind == RefactorRequest::FRAME_TAIL, table = ff.robot_table, fuse = ff.fused_tail();
    const bool f32s = c->storage != SRUKF_STORAGE_F64;            // (the mixed mode stores floats as well: the launches behind the tail round, as for fp32 storage without "fused tail" mode)
    const bool f32fuse = storage_f32_like(c) && fuse && table && frame_tail;      // fp32 storage in "fused tail" mode: the launch rounds what it writes (no k_quantize / k_rank_round / k_traj behind it)
    const bool f32 = f32s && !f32fuse;
    const bool tt = table && frame_tail && !f32;
    const bool exports = c->step_export.dst && tt && fuse;         // step-wise fast path: this launch is the frame's last and hands status + robot view to the host itself
    srukf_launch_rank_expand(c->stream, RankExpandLaunch{
        .d = c->d, .w = c->w, .p = c->p, .r = c->red_r,
        .Sp = c->G, .D = c->D, .perm = c->red_perm, .iperm = c->red_iperm, .gdiag = c->gdiag, .fs = c->fs, .X = c->X,
        .S = c->S, .A = c->shadowA, .sigR = tt ? c->sigR : nullptr, .Z = c->Z, .DZ = c->DZ,
        .do_traj = frame_tail && !f32, .fuse = tt && fuse, .f32round = f32fuse,
        .step_export = exports ? &c->step_export : nullptr,
        .null_rel = c->storage == SRUKF_STORAGE_F32_MIXED ? 1e-6 * c->dbg.mixed_null_ppm : 0.0,
        .fold_sync = (tt && fuse) ? c->fold_sync : nullptr, .fold_words = c->fold_sync ? 4 * (c->d.mp / 64) * (c->d.np / 64) : 0 });
    c->step_export_attached = exports;
    if (f32) {
        quantize_state(c);
        srukf_launch_rank_round(c->stream, np, c->red_r, c->shadowA);
        if (frame_tail) srukf_launch_traj(c->stream, c->d, c->X, c->S, c->fs, nullptr, 1);
    }
}

// How many tiles per worker (in percent) the owners' fold accepts.  A filter that has the GPU to itself: 106 = about one tile per worker (measured in round 2: with two
// tiles per worker, both to be formed before the first step, the exclusive replay loses — N = 300: 1 544 against 1 663 frames/s; srukf_debug_set "fold_tiles_pct").
// A filter that shares the GPU (three or four tenants of 256 / tenants CUs: two register tiles per worker): 200 — measured in round 4 at N = 200, four filters and four
// tenants, aggregate frames/s: owners fold both tiles 12 260; the same tiles from a launch of their own in the owners' summation order (k_syrk_own) 8 500 - 11 900;
// split-K k_syrk over the kept rows 13 100 but then the results differ in rounding from the same filter running alone.
static int fold_tiles_pct(const srukf_ctx* c) { return c->gmw_shared == 1 ? 200 : 106; }

static bool replay_red_fused(const srukf_ctx* c)
{
    return c->red_r > 0 && c->storage != SRUKF_STORAGE_F32_MIXED && c->shadowA && c->w.wc0 == c->w.wm0 && gmw_use_persist(c) &&
           c->gplan_red.workers >= 0 && c->gplan_red.nreal <= c->gplan_red.workers * fold_tiles_pct(c) / 100 && c->gplan_red.T >= 16 &&
           !c->debug_starve && g_sw.gmw_fused && g_sw.rank_fused && g_sw.rank_fold;
}

// RF_PERMUTED_SYRK as far as "table" mode may build on it ("table_perm" 0: the form runs, "table" mode does not); srukf_debug_get "plan_red_perm" reports THIS
bool replay_red_perm(const srukf_ctx* c) { return c->dbg.table_perm && refactor_form(c, refactor_frame_tail(c)).form == RF_PERMUTED_SYRK; }

// 0: k_motion + k_project; 1: k_project_motion (motion workgroup + projection with the robot part inline); 2: "table" (k_project_table: the
// previous frame's tail prepared the robot part of every sigma point) — only where the tail is k_rank_expand on the permuted operands
int replay_motion_mode(const srukf_ctx* c)
{
    // fp32 storage: only as "fused tail" mode (k_rank_expand<2> and the state update round what they write; "table" mode alone has no such form)
    const bool st_ok = c->storage == SRUKF_STORAGE_F64 ||
                       (storage_f32_like(c) && c->dbg.f32_fuse && c->dbg.tail_fuse && c->dbg.pxy2 && c->dbg.nullskip && c->nskip && c->tail_ok &&
                        (size_t)c->d.np * sizeof(double) <= 48 * 1024);
    // (null_canonical: "table" mode and everything on top of it read the structurally null rows of S as sqrt(EPSILON) e_k without looking)
    if (c->dbg.fused_motion == 2 && !((replay_red_fused(c) || replay_red_perm(c)) && st_ok && c->null_canonical)) return 1;
    return c->dbg.fused_motion;
}

// The form of the next staged frame's measurement half, chosen here and nowhere else ("pxy2" off: "table" mode keeps k_pxy, robot_table).
// "fused tail" mode: k_rank_expand<2> also projects the next frame, the motion reduction rides on k_pxy2 (MeasArgs::fmode), k_gain re-centres the robot rows
FrameForm frame_form(const srukf_ctx* c)
{
    const int mode = replay_motion_mode(c);
    const bool fuse = mode == 2 && c->dbg.pxy2 && c->dbg.nullskip && c->nskip && c->tail_ok && c->dbg.tail_fuse &&
                      (size_t)c->d.np * sizeof(double) <= 48 * 1024;      // (k_rank_expand<2> keeps a row of the factor in dynamic LDS)
    return FrameForm{ fuse ? MEAS_FUSED_TAIL : (mode == 2 && c->dbg.pxy2) ? MEAS_TABLE : mode ? MEAS_FUSED_MOTION : MEAS_PLAIN, mode == 2 };
}

// Round 5 measured where the head fold pays and where it cannot run at all (scripts/head_fold_sweep.py, scripts/abort_probe.py with the diagnostic build's time stamps):
//   * every worker's first step waits for ALL head tiles, and the helpers only get the CUs that pivot + workers leave free: with 261 helper jobs on 34 free CUs (N = 266) the
//     last one ends 125 us into the launch, the workers idle from 57 us on and the pivot behind them — frames/s with / without the fold: N = 200 5 269 / 5 098, 215 4 847 / 4 713,
//     230 4 488 / 4 487, 240 4 256 / 4 299, 250 3 681 / 4 179, 266 3 224 / 3 790.  The fold is kept while the helpers are at most 2.25 rounds on the free CUs (N <= 223);
//   * with 22 free CUs (N = 267 .. 275, pivot + 233 workers) the launch never completes by itself: some helpers run, then no further one starts until the workers give up
//     (all 270 finish right after the 10.7 ms bound: stamps).  29 or 30 main workgroups on an XCD's 32 CUs leave one of its shader engines without a free CU, and the
//     dispatcher, which deals workgroups round-robin to the engines, apparently does not skip a full one: with at most 28 per XCD (7 per engine: <= 224 main workgroups, >= 32
//     CUs free) it never happened.  Until this sweep the threshold was 16 free CUs and nothing between 9 and 34 had ever run: N = 267 .. 275 fell back to one launch per
//     panel without saying so.
#define SRUKF_HEAD_FOLD_MIN_FREE_CUS 32

// the helper workgroups of a head fold: one per head tile, per 256 rows of the pending X += dX, per SRUKF_RANK_COLS dropped diagonal entries
struct HeadJobs { int tiles, dx, gd; int total() const { return tiles + dx + gd; } };
static HeadJobs head_fold_jobs(const srukf_ctx* c) { return HeadJobs{ c->n_syrk_head_tiles, (c->d.n + 255) / 256, (c->d.n - c->red_r + SRUKF_RANK_COLS - 1) / SRUKF_RANK_COLS }; }

static bool head_fold_ok(const srukf_ctx* c)
{
    const int need = g_sw.head_fold_free.load() > 0 ? g_sw.head_fold_free.load() : SRUKF_HEAD_FOLD_MIN_FREE_CUS;
    const int free_cus = c->gplan_red.cus - (c->gplan_red.relay ? 2 : 1) - c->gplan_red.workers;      // what pivot(s) + workers really leave free
    const int nhelp = head_fold_jobs(c).total();
    // (the rounds rule was measured with one pivot workgroup and keeps counting that way: the relay's CU does not move the sizes at which the fold is taken)
    const bool pays = g_sw.head_fold_free.load() > 0 || 4 * nhelp <= 9 * (c->gplan_red.cus - 1 - c->gplan_red.workers);      // (the A/B switch "head_fold_free" overrides the rounds rule: measurements)
    return c->dbg.head_fold && c->gmw_shared == 0 && free_cus >= need && pays;
}

// split fold (srukf_gmw_persist.hip, k_gmw_tiles_fold): the rank-aware replay's k_syrk over the kept rows becomes jobs of the split form's tile launch
static bool split_fold_ok(const srukf_ctx* c)
{
    // Only while every tile workgroup of the plan can be resident beside the pivot / slab launch (four per CU): they hold their places from dispatch to their row's
    // last update, and beyond that the forming jobs queue behind waiting workgroups — frames/s with / without the fold: N = 400 2 150 / 1 960, 500 1 385 / 1 350,
    // 600 (1 190 tile workgroups for 796 places) 855 / 893, 800 393 / 459.
    const GmwPlan& gp = c->gplan_red;
    const bool fits = gp.nreal <= 4 * (gp.cus - gp.T) || g_sw.fold_force.load() != 0;      // ("fold_force": measurements)
    return c->dbg.split_fold && (fits || c->dbg.split_fold == 2) && c->red_r > 0 && c->storage != SRUKF_STORAGE_F32_MIXED && c->split_fold_list && c->n_split_fold > 0 && c->red_head0_tiles &&
           !c->debug_starve && !c->dbg.split_record && plan_persists(c, gp) && split_form(c, gp, true);
}

// Which launches a refactorisation consists of, chosen here and nowhere else: seq_refactor runs it, srukf_debug_get "plan_*" reports it.
RefactorPlan refactor_form(const srukf_ctx* c, const RefactorRequest& rq)
{
    RefactorPlan p = {};
    const GmwPlan& gr = c->gplan_red;
    const bool tail = rq.kind == RefactorRequest::FRAME_TAIL;    // the forms on the permuted operands keep no backup and take all of U: frame tails only
    // rank-aware (srukf_rank.hip): the null directions permuted to the end, only the leading red_Tp panels pivoted (the mixed-precision downdate too, round 6)
    const bool reduced = c->red_r > 0 && (c->storage != SRUKF_STORAGE_F32_MIXED || (c->dbg.mixed_rank && c->A32));
    if (tail && replay_red_fused(c)) {                           // (pays with about one tile per worker and T >= 16: docs/LAB_NOTEBOOK.md, round 2)
        p.form = RF_OWNERS_FOLD; p.persist = true; p.head_fold = head_fold_ok(c);
    } else if (reduced && tail && c->shadowA && c->w.wc0 == c->w.wm0 && g_sw.rank_fused) {
        p.form = RF_PERMUTED_SYRK; p.persist = plan_persists(c, gr);
        // own order (a filter that shares the GPU, two register tiles per worker): head rows by k_syrk, every other tile by k_syrk_own in the owners' summation order —
        // bit for bit what the same filter computes alone.  (Memory tiles and launches per panel keep the split-K k_syrk over the kept rows: nothing to be identical to.)
        p.own_order = c->gmw_shared == 1 && gmw_use_persist(c) && gr.workers > 0 && gr.T >= 16 && !c->debug_starve && g_sw.gmw_fused && g_sw.rank_fold &&
                      srukf_gmw_register_form(gr.T, gr.Tp, gr.ntiles, gr.workers);
        p.split_fold = !p.own_order && split_fold_ok(c);
    } else if (reduced) {
        p.form = RF_RANK_VIA_PERMUTATION; p.persist = plan_persists(c, gr);
    } else {
        // fused only with one tile per worker and T >= 16 (frames/s fused / not: N = 200 2 965 / 2 910, N = 100 5 247 / 5 262, N = 50 9 256 / 9 465, N = 300 1 544 / 1 663)
        p.form = RF_FULL_RANK; p.persist = gmw_use_persist(c);
        p.fused = tail && p.persist && c->storage == SRUKF_STORAGE_F64 && c->gplan.ntiles <= c->gplan.workers && c->gplan.T >= 16 && !c->debug_starve && g_sw.gmw_fused;
    }
    return p;
}

// k_syrk on the permuted operands (shadow copy, U^T with permuted columns) for one tile list, into Gp; spare workgroups: the pending state update, the dropped diagonal
static void syrk_permuted(srukf_ctx* c, FrameForm ff, const int* tiles, int ntiles)
{
    srukf_launch_syrk(c->stream, c->d, c->shadowA, c->Utp, 0, c->d.mp, c->Wf, c->fs, tiles, ntiles, SyrkRider{ dx_src(c), c->X, tail_rank_args(c, ff), take_xr1(c) });
    c->dx_pending = false;
}

// RF_OWNERS_FOLD: the owners form their tiles of S^T S - U U^T themselves, in permuted order from the shadow copy (no full k_syrk, no permutation pass)
static void refactor_owners_fold(srukf_ctx* c, const RefactorRequest& rq, const RefactorPlan& plan, FrameForm ff)
{
    const KDims& d = c->d; const int n = d.n;
    const double rr = c->red_r, hr = srukf_gmw_head_rows();
    const double head_flop = 2.0 * hr * n * (hr / 2.0 + d.mp) + 2.0 * (n - rr) * (rr + d.mp), head_byte = 8.0 * ((hr + d.mp) * n + (n - rr) * (rr + d.mp));
    // head fold (head_fold_ok): the head tiles, the pending X += dX and the dropped diagonal are helper workgroups of the persistent launch, not a k_syrk launch in front
    if (!plan.head_fold) {                                      // head rows of Gp: K = hr rows of the shadow copy + the 2N measurement rows; + the dropped diagonal
        ProfScope ps(c, KC_SYRK, head_flop, head_byte);
        syrk_permuted(c, ff, c->syrk_head_tiles, c->n_syrk_head_tiles);
    }
    {
        // factorisation of the leading red_Tp panels (all n columns carried along) + the owners' tiles of S^T S - U U^T
        // (kept rows below the head x all columns, K <= r and 2N): red_*_flop, update_null_set
        ProfScope ps(c, KC_GMW_PERSIST, c->red_fac_flop + c->red_own_flop + (plan.head_fold ? head_flop : 0.0), 8.0 * (2.0 * rr * n + (double)d.mp * n));
        HeadArgs ha = {};
        if (plan.head_fold) {
            HeadJobs hj = head_fold_jobs(c);
            if (!c->dx_pending) hj.dx = 0;
            ha.tiles = (const int2*)c->syrk_head_tiles; ha.ntiles = hj.tiles; ha.ncrit = c->n_syrk_head_crit;
            ha.dxp = dx_src(c); ha.X = c->X; ha.xr1 = take_xr1(c); ha.ndx = hj.dx;
            ha.ra = tail_rank_args(c, ff); ha.ngd = hj.gd;
            ha.nhelp = hj.total();                              // one helper workgroup per job, behind the pivot and the workers in dispatch order
            c->dx_pending = false;
        }
        const GmwFused fused = { c->shadowA, c->Utp, 0, d.mp };
        srukf_launch_gmw_persist(c->stream, gmw_launch(c, c->gplan_red, c->Wf, c->G, c->red_Tp, kept_rows16(c)), &fused, plan.head_fold ? &ha : nullptr);
    }
    ProfScope ps(c, KC_RANK_EXPAND, 0, 8.0 * 2.5 * (double)n * n);
    rank_expand(c, rq, ff);
}

// RF_PERMUTED_SYRK: where the owners cannot fold (memory tiles, one launch per panel), still in permuted order: k_syrk over the kept rows only, K <= r, into Gp
static void refactor_permuted_syrk(srukf_ctx* c, const RefactorRequest& rq, const RefactorPlan& plan, FrameForm ff)
{
    const KDims& d = c->d; const int np = d.np, n = d.n;
    const double rr = c->red_r, rp = 64.0 * c->red_Tp;
    const bool sfold = plan.split_fold;
    const double syrk_flop_all = rr * rr * rr / 3.0 + rr * rr * (n - rr) + 2.0 * d.mp * (rr * n - rr * rr / 2.0) + 2.0 * (n - rr) * (rr + d.mp);
    {
        ProfScope ps(c, KC_SYRK, sfold ? c->red_head0_flop + 2.0 * (n - rr) * (rr + d.mp) : syrk_flop_all, 8.0 * (rr * n + (double)d.mp * n + rp * n));
        if (c->storage == SRUKF_STORAGE_F32_MIXED) {
            // the mixed-precision downdate in the rank-aware form: the kept rows of S in permuted column order (what the stored floats hold: the permuted copy is
            // rounded with S) and U^T with permuted columns as fp32 operands, K <= r, products on the fp32 matrix pipe, chunk sums in FP64 — only the macro tiles of the
            // pivoted panels; the state update and the dropped diagonal (FP64, from the same operands) by k_syrk's spare workgroups with an empty tile list
            if (c->dbg.mixed_bf16 && c->mxr_xt) {
                // operands as three bf16 pieces each, transposed (K contiguous per column): the products on the bf16 matrix pipe, six per fp32 product
                srukf_launch_split_bf3(c->stream, c->mxr_krows, np, c->mxr_ktot, 0, c->shadowA, c->mxr_xt, c->mxr_xt_stride);
                srukf_launch_split_bf3(c->stream, d.mp, np, c->mxr_ktot, c->mxr_krows, c->Utp, c->mxr_xt, c->mxr_xt_stride);
                srukf_launch_syrk_bf3(c->stream, n, np, d.mp, c->mxr_krows, c->mxr_ktot, c->mxr_xt, c->mxr_xt_stride, c->mxr_tasks, c->mxr_ntasks, c->mxr_tiles, c->mxr_ntiles,
                                      c->mxr_part, c->Wf, c->fs);
            } else {
                srukf_launch_cvt_f32(c->stream, (size_t)c->mxr_krows * np, c->shadowA, c->A32);
                srukf_launch_cvt_f32(c->stream, (size_t)d.mp * np, c->Utp, c->U32);
                srukf_launch_syrk32(c->stream, n, np, d.mp, c->A32, c->U32, c->mxr_tasks, c->mxr_ntasks, c->mxr_tiles, c->mxr_ntiles, c->mxr_part, c->Wf, c->fs, c->mxr_krows);
            }
            // ... and BEHIND it, in FP64 from the FP64 operands, the few tiles whose pivots an fp32-formed product cannot resolve (the robot block, the shared anchor:
            // mxr_f64_tiles) — they overwrite what the fp32 launch left there
            syrk_permuted(c, ff, c->mxr_f64_tiles, c->dbg.mixed_f64_robot ? c->mxr_n_f64_tiles : 0);
        } else if (plan.own_order) {
            syrk_permuted(c, ff, c->syrk_head_tiles, c->n_syrk_head_tiles);
            srukf_launch_syrk_own(c->stream, n, np, c->shadowA, c->Utp, 0, d.mp, kept_rows16(c), c->Wf, c->fs, c->gplan_red.tiles, c->gplan_red.ntiles, c->red_Tp);
        } else if (sfold && c->dbg.split_fold != 2)
            // split fold: block row 0 and tile (1, 1) here (+ the state update and the dropped diagonal, as always); the tile launch of the pair forms the rest
            syrk_permuted(c, ff, c->red_head0_tiles, c->n_red_head0_tiles);
        else
            syrk_permuted(c, ff, c->red_syrk_tiles, c->n_red_syrk_tiles);
    }
    {
        ProfScope ps(c, plan.persist ? KC_GMW_PERSIST : KC_GMW_TRAIL, c->red_fac_flop + (sfold ? syrk_flop_all - c->red_head0_flop : 0.0), 8.0 * 2.0 * rp * n);
        launch_gmw_fast(c, c->Wf, c->G, sfold ? GMW_KEPT_PANELS_SPLIT_FOLD : GMW_KEPT_PANELS);
    }
    ProfScope ps(c, KC_RANK_EXPAND, 0, 8.0 * 2.5 * (double)n * n);
    rank_expand(c, rq, ff);
}

// G = S^T S - U[ub:ue] U[ub:ue]^T in state order; plan.fused: only the head rows (returns the share k_syrk computed).  Checked requests keep a copy in Gbak.
static double product_state_order(srukf_ctx* c, const RefactorRequest& rq, const RefactorPlan& plan)
{
    const KDims& d = c->d; const int np = d.np, n = d.n, ub = rq.ub, ue = rq.ue;
    const bool fused = plan.fused;
    const double nn = n;
    const double syrk_flop = nn * nn * nn / 3.0 + nn * nn * (ue - ub), syrk_byte = 8.0 * (nn * nn + (double)(ue - ub) * nn);
    const double head_frac = fused ? fmin(1.0, 2.0 * srukf_gmw_head_rows() / nn) : 1.0;      // rows / n, upper triangle
    if (c->storage == SRUKF_STORAGE_F32_MIXED && ub == 0 && ue == d.mp && !(c->dbg.mixed_rank && c->A32)) {
        // mixed precision, round 2's full-rank form (study: "mixed_rank" 0): the fp32 state S32 and U^T rounded once, products on the fp32 matrix pipe, chunk sums in FP64.
        // (In the rank-aware form of the mode only RF_PERMUTED_SYRK forms the product in fp32; whatever comes through here — the step-wise calls, a
        //  flagged frame's repeat on the exact path — forms it in FP64 from the FP64 working copies of the stored floats: the exact path must not divide fp32 noise.)
        ProfScope ps(c, KC_SYRK, syrk_flop, 4.0 * (nn * nn + (double)(ue - ub) * nn) + 8.0 * nn * nn / 2);
        if (c->dx_pending) srukf_launch_gain_dx(c->stream, n, np, c->dxp, c->X, take_xr1(c));
        c->dx_pending = false;
        srukf_launch_cvt_f32(c->stream, (size_t)d.mp * np, c->Ut, c->U32);
        srukf_launch_cvt_robot_cols(c->stream, n, np, c->S, c->S32);          // the motion step's columns, computed after the state was rounded
        srukf_launch_syrk32(c->stream, n, np, d.mp, c->S32, c->U32, c->mx_tasks, c->mx_ntasks, c->mx_tiles, c->mx_ntiles, c->mx_part, c->G, c->fs, np);
    } else {
        ProfScope ps(c, KC_SYRK, syrk_flop * head_frac, syrk_byte * head_frac);
        srukf_launch_syrk(c->stream, d, c->S, c->Ut, ub, ue, c->G, c->fs, fused ? c->syrk_head_tiles : c->syrk_tiles,
                          fused ? c->n_syrk_head_tiles : c->n_syrk_tiles, SyrkRider{ dx_src(c), c->X, RankArgs{}, take_xr1(c) });
        c->dx_pending = false;
    }
    if (rq.kind != RefactorRequest::FRAME_TAIL) hipMemcpyAsync(c->Gbak, c->G, sizeof(double) * (size_t)np * np, hipMemcpyDeviceToDevice, c->stream);
    return head_frac;
}

// RF_RANK_VIA_PERMUTATION: Gp = Pi^T G Pi into Wf (+ its diagonal), factor the leading red_Tp panels of Gp with the factor rows going to G (scratch
// now), then back to state order with the theta check, the null-direction check and the frame tail in one kernel
static void refactor_via_permutation(srukf_ctx* c, const RefactorRequest& rq, const RefactorPlan& plan)
{
    const int np = c->d.np, n = c->d.n;
    const double nn = n;
    product_state_order(c, rq, plan);
    {
        ProfScope ps(c, KC_MISC, 0, 16.0 * nn * nn);
        launch_sym_permute(c->stream, n, np, c->G, np, c->Wf, c->red_perm);
        srukf_launch_rank_diag(c->stream, n, np, c->G, c->red_perm, c->gdiag);
    }
    {
        const double rr = 64.0 * c->red_Tp;
        ProfScope ps(c, plan.persist ? KC_GMW_PERSIST : KC_GMW_TRAIL, rr * rr * rr / 3.0 + rr * rr * (nn - rr) + rr * (nn - rr) * (nn - rr) / 2.0, 8.0 * (rr * nn));
        launch_gmw_fast(c, c->Wf, c->G, GMW_KEPT_PANELS);
    }
    ProfScope ps(c, KC_GMW_CHECK, 0, 8.0 * nn * nn);
    rank_expand(c, rq, FORM_PLAIN);      // (a frame tail on this form never runs "table" mode: replay_motion_mode)
}

// RF_FULL_RANK: every pivot factored.  fused (replay path): k_syrk only for the first block rows, the persistent launch computes the other tiles of S^T S - U U^T
// itself while it is already factoring; it reads the filter's S for that, so the factor goes to the scratch buffer Wf and k_gmw_check copies it into S.
static void refactor_full_rank(srukf_ctx* c, const RefactorRequest& rq, const RefactorPlan& plan)
{
    const int np = c->d.np, n = c->d.n;
    const double nn = n;
    const bool fused = plan.fused;
    const double head_frac = product_state_order(c, rq, plan);
    const double syrk_flop = nn * nn * nn / 3.0 + nn * nn * (rq.ue - rq.ub), syrk_byte = 8.0 * (nn * nn + (double)(rq.ue - rq.ub) * nn);
    // 64-row panels: j0 = -64 factors the first 64x64 region, then one launch per panel
    // per panel: trailing update 64*r2^2 (upper half, 2 flop) + three-stage slab recompute + next 64x64 diagonal region
    auto panel_flop = [&](int j0) { const double r2 = np - j0 - 64; return j0 < 0 ? 64.0 * 64.0 * 64.0 / 3.0 : 64.0 * r2 * r2 + 3.0 * 2.0 * 32.0 * 32.0 * r2 + 64.0 * 64.0 * 64.0 / 3.0; };
    auto panel_byte = [&](int j0) { const double r2 = np - j0 - 64; return 8.0 * (r2 * r2 + 2.0 * 64.0 * r2); };
    if (plan.persist) {
        double fl = 0.0, by = 0.0;
        for (int j0 = -64; j0 + 64 < np; j0 += 64) { fl += panel_flop(j0); by += panel_byte(j0); }
        ProfScope ps(c, KC_GMW_PERSIST, fl + syrk_flop * (1.0 - head_frac), by + syrk_byte * (1.0 - head_frac));
        const GmwFused operands = { c->S, c->Ut, rq.ub, rq.ue };
        if (fused) srukf_launch_gmw_persist(c->stream, gmw_launch(c, c->gplan, c->G, c->Wf, 0, 0), &operands, nullptr);
        else launch_gmw_fast(c, c->G, c->S, GMW_ALL_PANELS);
    } else
        gmw_per_panel(c->stream, gmw_launch(c, c->gplan, c->G, c->S, 0, 0), c->pan, [&](int j0) { return ProfScope(c, KC_GMW_TRAIL, panel_flop(j0), panel_byte(j0)); });
    quantize_state(c);
    {
        ProfScope ps(c, KC_GMW_CHECK, 0, 8.0 * (double)n * n / 2);      // (frame tail: the check kernel also records the trajectory row and advances the frame counter)
        srukf_launch_gmw_check(c->stream, n, np, c->D, fused ? c->Wf : c->S, c->fs, c->X, rq.kind == RefactorRequest::FRAME_TAIL ? 1 : 0, fused ? c->S : nullptr);
    }
    shadow_rebuild(c);                                 // S was rewritten by a path that does not keep the permuted copy in step
}

void seq_refactor(srukf_ctx* c, const RefactorRequest& rq, FrameForm ff)
{
    if (rq.kind == RefactorRequest::SEQ_COLUMN) {               // the gamma/xi accumulators were not just cleared by k_gain
        ProfScope ps(c, KC_MISC, 0, 8.0 * c->d.np);
        launch_refactor_reset(c->stream, c->d.np, c->theta, c->fs, 1);
    }
    const RefactorPlan plan = refactor_form(c, rq);
    switch (plan.form) {
    case RF_OWNERS_FOLD: refactor_owners_fold(c, rq, plan, ff); break;
    case RF_PERMUTED_SYRK: refactor_permuted_syrk(c, rq, plan, ff); break;
    case RF_RANK_VIA_PERMUTATION: refactor_via_permutation(c, rq, plan); break;
    case RF_FULL_RANK: refactor_full_rank(c, rq, plan); break;
    }
}

// A flagged refactorisation again from the backup its checked request kept: what goes in front of the caller's exact_path + quantize_state (traj_base: staged form)
int exact_repeat_begin(srukf_ctx* c, int frame, double* traj_base)
{
    const size_t np = c->d.np;
    launch_set_run(c->stream, c->fs, frame, 1, traj_base);
    launch_refactor_reset(c->stream, (int)np, c->theta, c->fs, 0);
    HIPCHK(c, hipMemcpyAsync(c->G, c->Gbak, sizeof(double) * np * np, hipMemcpyDeviceToDevice, c->stream));
    return SRUKF_OK;
}

// The blocked factorisation on an arbitrary matrix buffer: Gbuf (upper triangle, destroyed) -> upper-triangular factor rows in Sout (whose lower triangle must already
// be zero).  which: every panel (the full plan), or the leading red_Tp panels of a permuted matrix (the rank-aware plan; split fold: its tile launch forms tiles too)
GmwLaunch gmw_launch(const srukf_ctx* c, const GmwPlan& gp, double* Gbuf, double* Sout, int Tp, int krows)
{
    return GmwLaunch{ .n = c->d.n, .ld = c->d.np, .eps = c->p.epsilon, .G = Gbuf, .pans = gp.pans, .D = c->D, .Sout = Sout, .sync = gp.sync, .tiles = gp.tiles, .ntiles = gp.ntiles,
                      .workers = gp.workers, .fs = c->fs, .Tp = Tp, .krows = krows, .gate_limit = gate_limit(c), .relay = gp.relay };
}

void launch_gmw_fast(srukf_ctx* c, double* Gbuf, double* Sout, GmwPanels which)
{
    const int np = c->d.np;
    const bool reduced = which != GMW_ALL_PANELS, fold = which == GMW_KEPT_PANELS_SPLIT_FOLD;
    const GmwPlan& gp = reduced ? c->gplan_red : c->gplan;
    const int Tp = reduced ? c->red_Tp : np / 64;
    const int krows = reduced ? kept_rows16(c) : 0;              // where the kept pivots end — the last pivoted panel is not factored beyond them
    GmwLaunch g = gmw_launch(c, gp, Gbuf, Sout, Tp, krows);
    if (plan_persists(c, gp)) {
        if (split_form(c, gp, true)) {                         // (srukf_debug_starve_workers: the pair without its tile launch)
            // the tile launch depends on what produced Gbuf, not on the pivot / slab launch: fork before, join after (in a capture: two parallel branches)
            if (c->dbg.split_record) hipMemcpyAsync(c->Gbak, Gbuf, sizeof(double) * (size_t)np * np, hipMemcpyDeviceToDevice, c->stream);
            hipEventRecord(c->ev_fork, c->stream);
            hipStreamWaitEvent(c->side, c->ev_fork, 0);
            if (fold) {
                c->split_fold_seqs++;
                srukf_launch_gmw_split_fold(c->stream, c->side, g, c->gsW, c->gsL, c->split_fold_list, c->n_split_fold, c->shadowA, c->Utp, c->d.mp);
            } else
                srukf_launch_gmw_split(c->stream, c->side, g, c->gsW, c->gsL, c->debug_starve ? 1 : 0);
            hipEventRecord(c->ev_join, c->side);
            hipStreamWaitEvent(c->stream, c->ev_join, 0);
            return;
        }
        // srukf_debug_starve_workers (tests only): launch without workers, as if the GPU were taken — the pivot's bounded wait
        // expires, the frame is flagged and repeated on the exact path, and the context falls back to one launch per panel
        if (c->debug_starve == 1) g.workers = 0;               // (2: only a split-form pair is starved — the tier below it then runs undisturbed)
        srukf_launch_gmw_persist(c->stream, g, nullptr, nullptr);
        return;
    }
    gmw_per_panel(c->stream, g, c->pan);
}

// The exact path: n + 1 launches behind one call (srukf_launch_gmw_col submits the right-looking sequence on its first call).  Launch-bound: 13.6 ms per flagged frame at
// N = 200 for ~5 ms of kernels.  As ONE captured graph per context it measured worse where it counts (38.8 ms per flagged frame over bench.py's 20-frame leg with three flagged
// frames: instantiating 1 205 nodes costs more than the two replays save), so the launches stay eager.
void exact_path(srukf_ctx* c, const double* Gbuf, double* Sout)
{
    const int np = c->d.np, n = c->d.n;
    for (int j = 0; j < n; j++) srukf_launch_gmw_col(c->stream, n, np, j, c->p.epsilon, Gbuf, c->Wf, c->D, c->theta, c->fs, Sout);
}

void run_gmw(srukf_ctx* c, double* Gbuf, double* Sout, bool slow)
{
    const int np = c->d.np, n = c->d.n;
    if (!slow) {
        launch_gmw_fast(c, Gbuf, Sout, GMW_ALL_PANELS);
        srukf_launch_gmw_check(c->stream, n, np, c->D, Sout, c->fs, c->X, 0, nullptr);
    } else {
        launch_refactor_reset(c->stream, np, c->theta, c->fs, 0);
        exact_path(c, Gbuf, Sout);
    }
}

// GSLCholeskyUpdate with FLAG_NEED_REORDER (SLAM.cpp:2122-2138) for the columns [ub, ue) of U:
//   dst = S^T S - U U^T;  dst_dis = Pi^T dst Pi  (disordered layout: the rank-deficient new-anchor block last);
//   S_dis = [R11 R12; 0 0],  R11 = gmw(dst_dis[0:r, 0:r]),  R12 = R11^{-T} dst_dis[0:r, r:n]   (2158-2179, r = n - 3 K_new);
//   S = R factor of QR(Pi S_dis Pi^T).
// [R11 R12] is what the right-looking GMW leaves in its first r rows whatever stands in the lower right block, so the
// full factorisation runs and rows >= r are zeroed.  R^T R = Pi (S_dis^T S_dis) Pi^T, so the QR is a second
// SYRK + permutation + GMW (P = S^T S is what the filter consumes; row signs of R are a convention).
int refactor_reorder(srukf_ctx* c, int ub, int ue)
{
    const KDims& d = c->d;
    const int np = d.np, n = d.n, r = n - 3 * c->K_new;
    const size_t bytes = sizeof(double) * (size_t)np * np;
    if (!c->Sdis) { if (srukf_dmalloc((void**)&c->Sdis, bytes) != hipSuccess) { c->err = "out of device memory (NEED_REORDER buffer)"; return SRUKF_ERR_NOMEM; } }
    launch_refactor_reset(c->stream, np, c->theta, c->fs, 1);
    srukf_launch_syrk(c->stream, d, c->S, c->Ut, ub, ue, c->G, c->fs, c->syrk_tiles, c->n_syrk_tiles, SyrkRider{ dx_src(c), c->X, RankArgs{}, take_xr1(c) });
    c->dx_pending = false;
    for (int stage = 0; stage < 2; stage++) {
        double* out = stage == 0 ? c->Sdis : c->S;
        if (stage == 1) {
            launch_refactor_reset(c->stream, np, c->theta, c->fs, 1);
            srukf_launch_syrk(c->stream, d, c->Sdis, c->Ut, 0, 0, c->G, c->fs, c->syrk_tiles, c->n_syrk_tiles, SyrkRider{});
        }
        for (int slow = 0; slow < 2; slow++) {
            launch_set_run(c->stream, c->fs, 0, 1, nullptr);
            launch_sym_permute(c->stream, n, np, c->G, np, c->Gbak, stage == 0 ? c->iperm : c->perm);
            if (stage == 0) HIPCHK(c, hipMemsetAsync(c->Sdis, 0, bytes, c->stream));
            run_gmw(c, c->Gbak, out, slow != 0);
            if (stage == 0 && r < np) hipLaunchKernelGGL(k_zero_rows, dim3(np - r), dim3(256), 0, c->stream, np, r, c->Sdis);
            if (slow) break;
            int rc = read_fs(c); if (rc) return rc;
            if (c->hfs->clamp_rows == 0) break;        // the theta clamp never won: the blocked result is the reference's
        }
    }
    quantize_state(c);
    return SRUKF_OK;
}

// first half: the cross covariances (riding on the launch: the statistics h / Si / visible, in "fused tail" mode the motion reduction); gf: the gain fold's, or null
static void launch_pxy(srukf_ctx* c, FrameForm ff, const GainFold& gf)
{
    const KDims& d = c->d;
    const double nn = d.n;
    const bool fused_stats = ff.fused_stats(), fused_motion = ff.fused_motion(), table = ff.pxy2(), fmode = ff.fused_tail();
    ProfScope ps(c, table ? KC_PXY2 : KC_PXY, nn * nn * 2.0 * d.N, 8.0 * (nn * nn / 2 + 2.0 * nn * 2 * d.N));
    MeasArgs ms = {};
    // ("fused tail" mode: the statistics are centred on the centre point's robot part, row 0 of the table: the mean does not exist yet)
    const double* xrob = fmode ? c->sigR : fused_motion ? (const double*)((const char*)c->fs + offsetof(FrameScalars, Xr1)) : c->X + (d.n - 4);
    if (fused_stats) ms = MeasArgs{ c->X, xrob, c->sigR, c->Z, c->mpart, c->h, c->Si, c->vis, c->PxyR, c->fs, (d.N + 31) / 32, table ? null_skip(c) : NullSkip{}, fmode ? 1 : 0,
                                    fmode ? 1 : 0, c->Cmat };
    if (fused_stats && c->mirror_next) {                       // step-wise API: the host's pinned copy of h | Si | visible is filled by the statistics jobs themselves
        ms.hmirror = (char*)c->hmeas;
        ms.hflag = (unsigned long long*)((char*)c->hfs + sizeof(FrameScalars) + sizeof(double) * 32);
        ms.hseq = c->meas_seq;
        ms.hstamp = (unsigned long long*)(c->hmeas + c->d.mp + 5 * (size_t)c->d.N);       // (the spare words behind h | Si | visible)
    }
    if (table) srukf_launch_pxy2(c->stream, d, c->DZ, c->shadowA, c->Utp, c->P1, c->pxy2_tiles, c->n_pxy2_tiles, kept_rows16(c), c->w, ms, gf);
    else srukf_launch_pxy(c->stream, d, c->DZ, c->S, c->Ut, c->pxy_tiles, c->n_pxy_tiles, c->w, ms);
}

void seq_pxy(srukf_ctx* c, FrameForm ff) { launch_pxy(c, ff, GainFold{}); }

// second half: gains, U^T, slice partials of the state update; z_dev / m_dev: this frame's measurements and matches on the device (null: the staged sequence's)
void seq_gain_only(srukf_ctx* c, const double* z_dev, const int* m_dev, FrameForm ff)
{
    const KDims& d = c->d;
    const bool fused_motion = ff.fused_motion(), table = ff.pxy2(), fmode = ff.fused_tail();
    ProfScope ps(c, KC_GAIN, 8.0 * d.n * 2 * d.N, 8.0 * 2.0 * d.n * 2 * d.N);
    srukf_launch_gain(c->stream, GainLaunch{
        .d = d, .w = c->w, .Ut = c->Ut, .PxyR = c->PxyR, .Si = c->Si, .vis = c->vis, .h = c->h,
        .z_seq = c->z_seq, .z_cur = z_dev, .m_seq = c->m_seq, .m_cur = m_dev,
        .fs = c->fs, .dxp = c->dxp, .Z = c->Z, .ra = rank_args(c),
        .Cm = fused_motion ? c->Cmat : nullptr, .S = c->S, .P1 = table ? c->P1 : nullptr, .split_b0 = c->pxy2_split_b0, .DZp = c->DZ,
        .sqeps = (fmode && storage_f32_like(c)) ? (double)(float)sqrt(c->p.epsilon) : sqrt(c->p.epsilon),   // (the null rows of S as they are stored)
        .sigR = c->sigR, .fmode = fmode, .next_pose = c->next_pose_pending ? c->next_odo + 3 : nullptr, .odo_dev = c->odo_step });
    c->next_pose_pending = false;
    c->dx_pending = true; c->dx_lm = false;           // applied by the next k_syrk launch (seq_refactor)
}

void seq_gain(srukf_ctx* c, const double* z_dev, const int* m_dev, FrameForm ff)
{
    // gain fold: the staged replay's "fused tail" frames (staged measurements, nothing for the host in between) form U^T and the state update inside k_pxy2
    const bool fold = c->dbg.gain_fold && ff.fused_tail() && !z_dev && !m_dev && !c->mirror_next && !c->next_pose_pending &&
                      c->fold_sync && c->dxk && c->w.wc0 == c->w.wm0 && c->z_seq && c->m_seq;
    GainFold gf = {};
    if (fold) {
        const KDims& d = c->d;
        gf.sync = c->fold_sync; gf.Utp = c->Utp; gf.dxk = c->dxk; gf.z_seq = c->z_seq; gf.m_seq = c->m_seq;
        gf.DZp = c->DZ; gf.perm = c->red_perm; gf.iperm = c->red_iperm; gf.r = c->red_r; gf.split_b0 = c->pxy2_split_b0;
        gf.sqeps = storage_f32_like(c) ? (double)(float)sqrt(c->p.epsilon) : sqrt(c->p.epsilon);      // (the null rows of S as they are stored: what seq_gain_only hands k_gain)
        gf.sc = c->w.wi * c->w.gamma;
        gf.S = c->S; gf.A = c->shadowA;
        gf.nmt = d.mp / 64; gf.nbt = d.np / 64; gf.bt_r0 = (c->red_r - 4) / 64; gf.bt_r1 = (c->red_r - 1) / 64; gf.robot_tiles = c->fold_robot_tiles;
    }
    launch_pxy(c, ff, gf);
    if (fold) { c->dx_pending = true; c->dx_lm = true; c->fold_seqs++; }
    else seq_gain_only(c, z_dev, m_dev, ff);
}

// Which directions of the state are structurally null (srukf_rank.hip)?  Called whenever a state arrives from outside
// (srukf_set_state*, map changes): row energies of S on the device, the lists on the host.  srukf_debug_set(0, "rank_aware", 0) switches it off.

int update_null_set(srukf_ctx* c)
{
    const int enabled = g_sw.rank_aware;
    const int n = c->d.n, np = c->d.np, T = np / 64;
    const int was = c->red_r;
    step_invalidate(c);
    c->red_r = 0;
    if (enabled && c->rank_aware && n >= 128) {
        srukf_launch_row_energy(c->stream, n, np, c->S, c->D);
        HIPCHK(c, hipMemcpyAsync(c->hstage, c->D, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpy2DAsync(c->hstage + np, sizeof(double), c->S, sizeof(double) * (np + 1), sizeof(double), n, hipMemcpyDeviceToHost, c->stream));   // diag S
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<int> perm, drop;
        for (int k = 0; k < n; k++) ((k < n - 4 && c->hstage[k] < SRUKF_NULL_ENERGY) ? drop : perm).push_back(k);
        // NullSkip and the sqrt(EPSILON) DZ term of k_gain assume that every structurally null row IS sqrt(EPSILON) e_k (what the reference's clamp leaves there and
        // every frame tail rewrites).  A state from outside only promises energy < 1e-12 (zero rows after joint initialisation, another small diagonal): then the
        // first staged frame runs the launch sequence that reads the rows as they are, and its tail makes them canonical (null_canonical, run_frames_async).
        {
            const double sq = c->storage != SRUKF_STORAGE_F64 ? (double)(float)sqrt(c->p.epsilon) : sqrt(c->p.epsilon);
            bool canon = true;
            for (int k : drop) canon = canon && c->hstage[np + k] == sq && c->hstage[k] == sq * sq;
            c->null_canonical = canon;
        }
        const int r = (int)perm.size(), Tp = (r + 63) / 64;
        if (!drop.empty() && Tp < T) {                            // worth it only if at least one whole panel leaves the pivot chain
            perm.insert(perm.end(), drop.begin(), drop.end());
            for (int k = n; k < np; k++) perm.push_back(k);
            std::vector<int> iperm(np);
            for (int a = 0; a < np; a++) iperm[perm[a]] = a;
            if (!c->red_perm) {
                HIPCHK(c, srukf_dmalloc(&c->red_perm, sizeof(int) * np)); HIPCHK(c, srukf_dmalloc(&c->red_iperm, sizeof(int) * np));
                HIPCHK(c, srukf_dmalloc(&c->gdiag, sizeof(double) * np));
            }
            HIPCHK(c, hipMemcpy(c->red_perm, perm.data(), sizeof(int) * np, hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(c->red_iperm, iperm.data(), sizeof(int) * np, hipMemcpyHostToDevice));
            if (c->gplan_red.Tp != Tp || !c->gplan_red.pans || c->gplan_red.tenants != plan_tenants(c)) {
                gmw_plan_destroy(c->gplan_red, c->stream);
                const int rc = gmw_plan_create(c->gplan_red, np, c->stream, Tp, plan_tenants(c));
                if (rc) { c->err = "rank-aware refactorisation: allocation failed"; return rc; }
            }
            split_ensure(c, c->gplan_red);
            c->red_r = r; c->red_Tp = Tp;
            {
                // algorithmic flop of the rank-aware refactorisation (DESIGN.md "flop model"): pivots j < rp update rows (j, rp) x
                // columns [row, n) of the upper triangle; the owners form the tiles of rows [head, rp) from K = min(row + 32, r) + 2N terms
                const double rp = 64.0 * Tp, nn = n, kr = (r + 15) & ~15;
                c->red_fac_flop = (nn - rp) * rp * rp + rp * rp * rp / 3.0;
                c->red_own_flop = 0.0;
                for (int I = srukf_gmw_head_rows() / 64; I < Tp; I++)
                    for (int J = I; J < T; J++)
                        for (int h = 0; h < 2; h++) c->red_own_flop += 2.0 * 32.0 * 64.0 * (fmin(64.0 * I + 32.0 * h + 32.0, kr) + c->d.mp) * (I == J ? 0.75 : 1.0);
            }
            {
                // k_syrk tiles of block rows < Tp in the XCD-aware order of the full table (build_tile_table)
                std::vector<int> ts = build_tile_table(np / 32, np / 32, true, true, 0), tr;
                for (size_t q = 0; q + 1 < ts.size(); q += 2) if (ts[q] >= 0 && ts[q] * 32 < 64 * Tp) { tr.push_back(ts[q]); tr.push_back(ts[q + 1]); }
                if (c->red_syrk_tiles) srukf_dfree_on(c->red_syrk_tiles, c->stream);
                c->red_syrk_tiles = nullptr; c->n_red_syrk_tiles = (int)tr.size() / 2;
                HIPCHK(c, srukf_dmalloc(&c->red_syrk_tiles, sizeof(int) * tr.size()));
                HIPCHK(c, hipMemcpy(c->red_syrk_tiles, tr.data(), sizeof(int) * tr.size(), hipMemcpyHostToDevice));
                // split fold: what of that list stays with k_syrk, and the grid of the tile launch that forms the rest (srukf_gmw_persist.hip)
                std::vector<int> th;
                c->red_head0_flop = 0.0;
                const int kr16 = (r + 15) & ~15;
                const int fold_head = srukf_gmw_fold_head_rows(Tp);
                for (size_t q = 0; q + 1 < tr.size(); q += 2) if (srukf_gmw_fold_head_tile(tr[q], tr[q + 1], fold_head)) {
                    th.push_back(tr[q]); th.push_back(tr[q + 1]);
                    c->red_head0_flop += 2.0 * 32.0 * 32.0 * (std::min(32 * tr[q] + 32, kr16) + c->d.mp);
                }
                if (c->red_head0_tiles) srukf_dfree_on(c->red_head0_tiles, c->stream);
                if (c->split_fold_list) srukf_dfree_on(c->split_fold_list, c->stream);
                c->red_head0_tiles = nullptr; c->split_fold_list = nullptr;
                c->n_red_head0_tiles = (int)th.size() / 2;
                HIPCHK(c, srukf_dmalloc(&c->red_head0_tiles, sizeof(int) * std::max<size_t>(th.size(), 2)));
                HIPCHK(c, hipMemcpy(c->red_head0_tiles, th.data(), sizeof(int) * th.size(), hipMemcpyHostToDevice));
                c->n_split_fold = srukf_gmw_build_fold_list(T, Tp, nullptr);
                std::vector<short> fl((size_t)4 * std::max(c->n_split_fold, 1));
                srukf_gmw_build_fold_list(T, Tp, fl.data());
                HIPCHK(c, srukf_dmalloc(&c->split_fold_list, sizeof(short) * fl.size()));
                HIPCHK(c, hipMemcpy(c->split_fold_list, fl.data(), sizeof(short) * fl.size(), hipMemcpyHostToDevice));
            }
            if (!c->shadowA) {
                HIPCHK(c, srukf_dmalloc(&c->shadowA, sizeof(double) * (size_t)np * np)); HIPCHK(c, srukf_dmalloc(&c->Utp, sizeof(double) * (size_t)c->d.mp * np));
                HIPCHK(c, hipMemsetAsync(c->Utp, 0, sizeof(double) * (size_t)c->d.mp * np, c->stream));
                HIPCHK(c, srukf_dmalloc(&c->P1, sizeof(double) * (size_t)c->d.mp * np));
                HIPCHK(c, hipMemsetAsync(c->P1, 0, sizeof(double) * (size_t)c->d.mp * np, c->stream));
                // gain fold of k_pxy2: sync words (zero between frames) and the per-landmark shares of the state update
                const size_t fw = sizeof(unsigned int) * (size_t)(srukf_fold_words(c->d.mp / 64, np / 64) + 2) + sizeof(unsigned long long) * FOLD_DBG_STAMPS;
                HIPCHK(c, srukf_dmalloc(&c->fold_sync, fw)); HIPCHK(c, hipMemsetAsync(c->fold_sync, 0, fw, c->stream));
                HIPCHK(c, srukf_dmalloc(&c->dxk, sizeof(double) * (size_t)(c->d.N > 0 ? c->d.N : 1) * np));
                HIPCHK(c, hipMemsetAsync(c->dxk, 0, sizeof(double) * (size_t)(c->d.N > 0 ? c->d.N : 1) * np, c->stream));
            }
            {
                // k_pxy2 ("table" mode): 64 x 64 tiles of the permuted product, K ends at the kept rows, long K ranges in two halves
                const int kr = (r + 15) & ~15;
                const int nt = srukf_pxy2_build_tiles(c->d.mp, np, kr, nullptr);
                std::vector<int> tl((size_t)4 * nt);
                srukf_pxy2_build_tiles(c->d.mp, np, kr, tl.data());
                if (c->pxy2_tiles) srukf_dfree_on(c->pxy2_tiles, c->stream);
                c->pxy2_tiles = nullptr; c->n_pxy2_tiles = nt;
                c->fold_robot_tiles = 0;                          // tile workgroups that read the robot columns (permuted positions r-4 .. r-1) of the permuted copy: gain fold
                for (int q = 0; q < nt; q++) if (tl[4 * q] >= 0 && (tl[4 * q + 1] == (r - 4) / 64 || tl[4 * q + 1] == (r - 1) / 64)) c->fold_robot_tiles++;
                HIPCHK(c, srukf_dmalloc(&c->pxy2_tiles, sizeof(int) * tl.size()));
                HIPCHK(c, hipMemcpy(c->pxy2_tiles, tl.data(), sizeof(int) * tl.size(), hipMemcpyHostToDevice));
                {
                    // NullSkip: which directions are projected for all landmarks, which only for their own, which rows of Z the statistics walk
                    std::vector<int> dirs, nulls, rows;
                    const int Na = n + 5;
                    for (int i = 0; i < Na; i++) ((i >= n || i < 2 || iperm[i] < r) ? dirs : nulls).push_back(i);
                    rows.push_back(0);
                    for (int i : dirs) rows.push_back(1 + i);
                    for (int i : dirs) rows.push_back(1 + Na + i);
                    std::vector<int> all(dirs); all.insert(all.end(), nulls.begin(), nulls.end()); all.insert(all.end(), rows.begin(), rows.end());
                    if (c->nskip) srukf_dfree_on(c->nskip, c->stream);
                    c->nskip = nullptr;
                    HIPCHK(c, srukf_dmalloc(&c->nskip, sizeof(int) * all.size()));
                    HIPCHK(c, hipMemcpy(c->nskip, all.data(), sizeof(int) * all.size(), hipMemcpyHostToDevice));
                    c->ns_full = (int)dirs.size(); c->ns_null = (int)nulls.size(); c->ns_rows = (int)rows.size();
                    // (directions 0 and 1 are projected for every landmark even when they are structurally null — the Si factor names their Z rows —
                    //  and the frame tail (k_rank_expand<2>) only does that for kept rows: such a state stays with k_project_table)
                    c->tail_ok = iperm[0] < r && iperm[1] < r;
                }
                c->pxy2_split_b0 = np;                            // first permuted column whose K range is cut in two
                for (int bt = 0; bt < np / 64; bt++) if (std::min(4 * (bt + 1), ((kr + 63) / 64) * 4) >= srukf_pxy2_split_groups()) { c->pxy2_split_b0 = 64 * bt; break; }
            }
            shadow_rebuild(c);
        }
    }
    if (was || c->red_r) drop_graphs(c);                          // the captured frames contain one or the other launch sequence
    return mixed_red_ensure(c);
}

// SRUKF_STORAGE_F32_MIXED in the rank-aware form: the fp32 copy of the kept rows, the task list of k_syrk32 over the pivoted panels (shape: r, Tp).  Called whenever the
// null set or the storage mode changes — never inside a capture.
int mixed_red_ensure(srukf_ctx* c)
{
    if (c->storage != SRUKF_STORAGE_F32_MIXED || c->red_r <= 0 || !c->shadowA) return SRUKF_OK;
    const int np = c->d.np, mp = c->d.mp;
    if (!c->A32) HIPCHK(c, srukf_dmalloc(&c->A32, sizeof(float) * (size_t)np * np));
    if (c->mxr_for_r == c->red_r && c->mxr_tasks) return SRUKF_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (void* b : { (void*)c->mxr_part, c->mxr_tasks, c->mxr_tiles, (void*)c->mxr_f64_tiles, (void*)c->mxr_xt }) if (b) srukf_dfree_on(b, c->stream);
    c->mxr_part = nullptr; c->mxr_tasks = nullptr; c->mxr_tiles = nullptr; c->mxr_f64_tiles = nullptr; c->mxr_xt = nullptr;
    c->mxr_krows = std::min(np, srukf_mixed_krows(c->red_r));
    int ntiles = 0;
    const int ntasks = srukf_mixed_build_tasks_red(np, mp, c->mxr_krows, 64 * c->red_Tp, nullptr, nullptr, &ntiles);
    std::vector<short> tk((size_t)4 * ntasks); std::vector<int> tl((size_t)2 * ntiles);
    srukf_mixed_build_tasks_red(np, mp, c->mxr_krows, 64 * c->red_Tp, tk.data(), tl.data(), &ntiles);
    HIPCHK(c, srukf_dmalloc(&c->mxr_part, srukf_mixed_part_bytes(ntasks)));
    HIPCHK(c, srukf_dmalloc(&c->mxr_tasks, sizeof(short) * tk.size()));
    HIPCHK(c, srukf_dmalloc(&c->mxr_tiles, sizeof(int) * tl.size()));
    HIPCHK(c, hipMemcpy(c->mxr_tasks, tk.data(), sizeof(short) * tk.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->mxr_tiles, tl.data(), sizeof(int) * tl.size(), hipMemcpyHostToDevice));
    c->mxr_ntasks = ntasks; c->mxr_ntiles = ntiles; c->mxr_for_r = c->red_r;
    c->mxr_ktot = c->mxr_krows + mp; c->mxr_xt_stride = (size_t)np * c->mxr_ktot;
    HIPCHK(c, srukf_dmalloc(&c->mxr_xt, sizeof(unsigned short) * 3 * c->mxr_xt_stride));
    HIPCHK(c, hipMemsetAsync(c->mxr_xt, 0, sizeof(unsigned short) * 3 * c->mxr_xt_stride, c->stream));
    {
        // the FP64 tiles (32 x 32, permuted order, upper triangle, rows of the pivoted panels): tile row / column 0 (the shared anchor: permuted positions 0 .. 2) and the
        // one or two tile rows / columns of the robot block (r-4 .. r-1)
        const int T32 = np / 32, rows32 = 2 * c->red_Tp, q0 = 0, q1 = (c->red_r - 4) / 32, q2 = (c->red_r - 1) / 32;
        std::vector<int> tl;
        for (int I = 0; I < rows32 && I < T32; I++)
            for (int J = I; J < T32; J++)
                if (I == q0 || I == q1 || I == q2 || J == q1 || J == q2) { tl.push_back(I); tl.push_back(J); }
        HIPCHK(c, srukf_dmalloc(&c->mxr_f64_tiles, sizeof(int) * (tl.size() + 2)));
        HIPCHK(c, hipMemcpy(c->mxr_f64_tiles, tl.data(), sizeof(int) * tl.size(), hipMemcpyHostToDevice));
        c->mxr_n_f64_tiles = (int)tl.size() / 2;
    }
    drop_graphs(c);
    return SRUKF_OK;
}

int read_fs(srukf_ctx* c)
{
    HIPCHK(c, hipMemcpyAsync(c->hfs, c->fs, sizeof(FrameScalars), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return read_fs_host(c);
}
// the frame scalars are in *c->hfs already (the step-wise fast path has a kernel write them there with the robot view)
int read_fs_host(srukf_ctx* c)
{
    if (c->hfs->clamp_rows > 0 && c->hfs->clamp_frame == 0x7fffffff) c->hfs->clamp_frame = c->hfs->frame - 1;   // the run's last frame
    if (c->hfs->gmw_aborts > 0 && c->gmw_shared != 2) {
        // a persistent launch did not get all its workgroups onto the GPU in time (somebody else is using it, or the two launches of a split-form pair were not
        // run side by side): the flagged frame is repeated on the exact path like a clamp frame, and the filter steps down ONE tier — from the split form to the
        // memory-tile instance of k_gmw_persist (one launch, no second hardware queue needed), from any single persistent launch to one launch per panel
        const GmwPlan& gp = c->red_r > 0 ? c->gplan_red : c->gplan;
        if (split_form(c, gp, true)) { c->split_off = true; c->err = "a split-form factorisation pair was abandoned: this filter continues with the memory-tile persistent launch (srukf_debug_get \"split_off\")"; }
        else { c->gmw_shared = 2; c->err = "a persistent factorisation launch was abandoned: this filter continues with one launch per panel (srukf_debug_get \"gmw_shared\" = 2)"; }
        drop_graphs(c);
    }
    return SRUKF_OK;
}

void graphs_destroy(ReplayGraphs& g)
{
    for (hipGraphExec_t* e : { &g.one_exec, &g.eight_exec, &g.block_exec }) if (*e) { hipGraphExecDestroy(*e); *e = nullptr; }
    for (hipGraph_t* q : { &g.one, &g.eight, &g.block }) if (*q) { hipGraphDestroy(*q); *q = nullptr; }
    g.block_frames = 0;
}

// the captured frames of both update modes: the replay's, and every form of an image frame
void drop_graphs(srukf_map_scope* c)
{
    for (int m = 0; m < 2; m++) {
        graphs_destroy(c->graphs[m]);
        for (int i = 0; i < IMAGE_FORM_ROWS; i++) graphs_destroy(c->img.graphs[i][m]);
    }
}

// shared: 0 exclusive, 1 shared (tenants persistent launches at a time), 2 one launch per panel
int set_shared(srukf_ctx* c, int shared, int tenants)
{
    if (tenants < 2) tenants = 2;
    if (shared == c->gmw_shared && (shared != 1 || tenants == c->shared_tenants)) return SRUKF_OK;
    const int was = plan_tenants(c);
    step_invalidate(c);
    c->gmw_shared = shared;
    if (shared == 1) c->shared_tenants = tenants;
    drop_graphs(c);
    if (plan_tenants(c) != was) {                              // the persistent launches keep to half the CUs / may use all of them again
        gmw_plan_destroy(c->gplan, c->stream);
        const int rc = gmw_plan_create(c->gplan, c->d.np, c->stream, 0, plan_tenants(c));
        if (rc) { c->err = "set_exclusive: persistent GMW resources: allocation failed"; return rc; }
        split_ensure(c, c->gplan);
        return update_null_set(c);                             // the rank-aware plan with the same limit
    }
    return SRUKF_OK;
}

// the captured frames of an update mode the replay has (BATCHED, JOINT)
static ReplayGraphs& replay_graphs(srukf_ctx* c, int mode) { return c->graphs[mode == SRUKF_UPDATE_JOINT ? 1 : 0]; }

// A joint frame of the staged replay (SRUKF_UPDATE_JOINT): always the plain frame form, whatever "fused_motion" and its neighbours say — all of
// c->Z is written, c->Ut holds S^T DZ in state order, nothing of the motion step is pending: what the joint kernels read — with the joint launches in k_gain's place.
// They leave what k_gain leaves in this form (gain_body with Cm, P1 null): U^T in c->Ut and, with permuted columns, in c->Utp; the gamma / xi accumulators cleared;
// and X updated already, where k_gain leaves slice partials for the k_syrk launch (dx_pending false: the tail's launches carry no state update).
// joint_ensure has run (run_frames_async, prepare_frames_mode: never inside a capture)
static void replay_one_frame_joint(srukf_ctx* c)
{
    seq_predict_motion(c, nullptr);
    seq_predict_measurement(c, FORM_PLAIN);
    seq_pxy(c, FORM_PLAIN);
    seq_joint_launches(c, nullptr, nullptr);
    seq_refactor(c, refactor_frame_tail(c), FORM_PLAIN);
}

// srukf_debug_set(ctx, "fused_motion", 0): the replay keeps k_motion and k_project as two launches (A/B runs)
static void replay_one_frame(srukf_ctx* c, int mode)
{
    if (mode == SRUKF_UPDATE_JOINT) { replay_one_frame_joint(c); return; }
    const FrameForm ff = frame_form(c);
    // "fused tail" mode: the previous frame's tail (or, for a run's first frame, run_frames_async) projected this frame; its motion reduction rides on k_pxy2
    if (ff.fused_tail()) c->xr1_pending = true;
    else if (ff.fused_motion()) seq_predict_fused(c, ff);
    else {
        seq_predict_motion(c, nullptr);
        seq_predict_measurement(c, ff);
    }
    seq_gain(c, nullptr, nullptr, ff);
    seq_refactor(c, refactor_frame_tail(c), ff);
}

int capture_frames(srukf_ctx* c, int nframes, hipGraph_t* g, hipGraphExec_t* ge, const std::function<void()>& issue_frame)
{
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    for (int q = 0; q < nframes; q++) issue_frame();
    const hipError_t launch_err = hipGetLastError();            // a failed launch inside the capture must not leave the stream capturing
    HIPCHK(c, hipStreamEndCapture(c->stream, g));
    HIPCHK(c, launch_err);
    HIPCHK(c, hipGraphInstantiate(ge, *g, nullptr, nullptr, 0));
    return SRUKF_OK;
}

// the null rows are canonical from here on (a rank-aware frame tail has been issued): captured frames of the other launch sequence are stale
// fp64 storage only (the float-stored modes keep their rounded copies in step elsewhere); "null_canon" 0: the first frame behind such a factor runs the launch sequence that
// reads the rows as they are and its tail rewrites them (rounds 2 - 5)
void canonicalize_null_rows(srukf_ctx* c)
{
    if (!c->dbg.null_canon || c->red_r <= 0 || c->null_canonical || c->storage != SRUKF_STORAGE_F64 || !c->red_perm) return;
    srukf_launch_rank_canon(c->stream, c->d.n, c->d.np, c->red_r, sqrt(c->p.epsilon), c->red_perm, c->S);
    c->null_canonical = true;
    drop_graphs(c);
}

void set_null_canonical(srukf_ctx* c)
{
    if (c->red_r > 0 && !c->null_canonical) { c->null_canonical = true; drop_graphs(c); }
}

}  // namespace srukf_impl

// which update modes the staged replay has, and on which storage: BATCHED everywhere; JOINT on fp64 storage (the step-wise srukf_update_joint refuses
// SRUKF_STORAGE_F32_MIXED too; SRUKF_STORAGE_F32: the replay's frame tails round in launches the step-wise call's checked refactorisation does not share —
// not shown to round at the same points, so refused, include/srukf.h)
int srukf_impl::replay_mode_check(srukf_ctx* c, int mode, const char* who)
{
    if (mode == SRUKF_UPDATE_BATCHED) return SRUKF_OK;
    if (mode != SRUKF_UPDATE_JOINT) { c->err = std::string(who) + " supports BATCHED and JOINT only (SEQUENTIAL needs a host check per column)"; return SRUKF_ERR_UNSUPPORTED; }
    if (c->storage != SRUKF_STORAGE_F64) {
        c->err = std::string(who) + (c->storage == SRUKF_STORAGE_F32_MIXED ? ": SRUKF_UPDATE_JOINT is not available in SRUKF_STORAGE_F32_MIXED" : ": SRUKF_UPDATE_JOINT frames are not available in SRUKF_STORAGE_F32 (use srukf_update_joint)");
        return SRUKF_ERR_UNSUPPORTED;
    }
    return SRUKF_OK;
}

// What srukf_run_frames_async and the image runs (run_images_issue) share to the letter.  In front of a run:
void srukf_impl::replay_prologue(srukf_ctx* c)
{
    step_commit_motion(c); step_state_replaced(c);
    if (c->fs_seq_step) {                                      // the step-wise fast path pointed the frame scalars at its own three poses
        launch_set_seq(c->stream, c->fs, c->odo_seq, c->seqF, c->p);
        c->fs_seq_step = false;
    }
}

// count frames from the captured frames of one form: a graph of SRUKF_GRAPH_FRAMES consecutive frames while that many are left (one host launch per 8 frames keeps the
// host ahead of the device when several filters share one host thread), then single frames
int srukf_impl::replay_launch_graphs(srukf_ctx* c, const ReplayGraphs& g, int count)
{
    int f = 0;
    for (; f + SRUKF_GRAPH_FRAMES <= count; f += SRUKF_GRAPH_FRAMES) HIPCHK(c, hipGraphLaunch(g.eight_exec, c->stream));
    for (; f < count; f++) HIPCHK(c, hipGraphLaunch(g.one_exec, c->stream));
    return SRUKF_OK;
}

// behind the frames a run issued
int srukf_impl::replay_epilogue(srukf_ctx* c)
{
    c->async_pending = true;
    c->phase = 0; c->frame_updated = false;
    HIPCHK(c, hipGetLastError());
    return SRUKF_OK;
}

// the synchronous entries' frame: the trajectory rows on the device around run(dt), copied to the host when it ends well
int srukf_impl::with_device_traj(srukf_ctx* c, int count, double* traj_host, const std::function<int(double*)>& run)
{
    double* dt = nullptr;
    HIPCHK(c, srukf_dmalloc((void**)&dt, sizeof(double) * 8 * (size_t)count));
    const int rc = run(dt);
    if (traj_host && rc == SRUKF_OK) hipMemcpy(traj_host, dt, sizeof(double) * 8 * (size_t)count, hipMemcpyDeviceToHost);
    srukf_dfree(dt);
    return rc;
}

// *c->hfs holds a set sticky pair of the joint update: the error the caller returns.  Frames before that one are valid; it and the later ones are not
static int joint_bad_report(srukf_ctx* c)
{
    char b[240]; snprintf(b, sizeof b, "joint update: non-positive pivot in the innovation covariance or non-finite innovation in staged frame %d, row %d: the frame's inputs are not finite "
                                       "(frames before it are valid; it and the later ones are not)", c->hfs->joint_bad_frame - 1, c->hfs->joint_bad_row);
    c->err = b; c->joint_bad_host = true;
    return SRUKF_ERR_UNSUPPORTED;
}

// One staged frame (index `frame`) through the path that checks the theta clamp on the host and repeats the
// refactorisation column by column when the reference's third pivot candidate would have won — what srukf_update does,
// with the staged inputs.  traj_row: device pointer of this frame's trajectory row, or null.
// mode JOINT: seq_pxy + the joint launches in seq_gain's place, as step_update_slow runs them (built by passing the mode through; no test reaches it: DESIGN.md section 19)
static int run_staged_frame_exact(srukf_ctx* c, int frame, double* traj_row, int mode)
{
    const KDims& d = c->d;
    c->exact_frames++;
    const bool timing = g_sw.timing.load() != 0;              // (srukf_debug_set(0, "timing", 1): where a flagged frame's milliseconds go, on stderr)
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto t0 = now();
    auto lap = [&](const char* what) { if (timing) { hipStreamSynchronize(c->stream); auto t1 = now(); fprintf(stderr, "[exact frame] %s %.0f us\n", what, std::chrono::duration<double, std::micro>(t1 - t0).count()); t0 = t1; } };
    double* tb = traj_row ? traj_row - (size_t)8 * frame : nullptr;
    launch_set_run(c->stream, c->fs, frame, 1, tb);
    seq_predict_motion(c, nullptr);
    seq_predict_measurement(c, FORM_PLAIN);
    lap("predict");
    if (mode == SRUKF_UPDATE_JOINT) {
        const int rcj = joint_ensure(c, "run_frames"); if (rcj) return rcj;
        seq_pxy(c, FORM_PLAIN);
        seq_joint_launches(c, nullptr, nullptr);
    } else
        seq_gain(c, nullptr, nullptr, FORM_PLAIN);
    lap("gain");
    seq_refactor(c, refactor_checked(c), FORM_PLAIN);
    int rc = read_fs(c); if (rc) return rc;
    lap("blocked refactor");
    if (mode == SRUKF_UPDATE_JOINT && c->hfs->joint_bad_frame > 0) return joint_bad_report(c);
    if (c->hfs->clamp_rows > 0) {
        rc = exact_repeat_begin(c, frame, tb); if (rc) return rc;
        ProfScope ps(c, KC_GMW_COL, 0, 0);
        exact_path(c, c->G, c->S);
        quantize_state(c);
        lap("exact path");
        rc = update_null_set(c); if (rc) return rc;      // the null set is re-derived from the exact factor (see srukf_update)
        lap("null set");
    } else if (c->storage != SRUKF_STORAGE_F32_MIXED || storage_f32_like(c)) set_null_canonical(c);
    srukf_launch_traj(c->stream, d, c->X, c->S, c->fs, nullptr, 1);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return SRUKF_OK;
}

extern "C" {

int srukf_set_exclusive(srukf_ctx* c, int exclusive)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));                         // the plans below size themselves on the CURRENT device's CU count
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int shared = exclusive == SRUKF_GPU_SHARED ? 1 : exclusive == SRUKF_GPU_SHARED_PER_PANEL ? 2 : 0;
    return set_shared(c, shared, g_sw.shared_tenants.load());
}

int srukf_stage_sequence(srukf_ctx* c, int F, const double* odo, const double* z, const int* matched)
{
    if (!c || F < 1 || !odo || !z || !matched) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int N = c->d.N;
    HIPCHK(c, hipStreamSynchronize(c->stream));             // frames in flight may still read the staged inputs
    if (c->odo_seq) { srukf_dfree(c->odo_seq); srukf_dfree(c->z_seq); srukf_dfree(c->m_seq); c->odo_seq = nullptr; c->z_seq = nullptr; c->m_seq = nullptr; }
    drop_graphs(c);
    images_drop(c, c->stream);                              // (staged images belong to the sequence they were staged for: srukf_stage_images)
    HIPCHK(c, srukf_dmalloc((void**)&c->odo_seq, sizeof(double) * 3 * (F + 1)));
    HIPCHK(c, srukf_dmalloc((void**)&c->z_seq, sizeof(double) * (size_t)F * 2 * N));
    HIPCHK(c, srukf_dmalloc((void**)&c->m_seq, sizeof(int) * (size_t)F * N));
    HIPCHK(c, hipMemcpy(c->odo_seq, odo, sizeof(double) * 3 * (F + 1), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->z_seq, z, sizeof(double) * (size_t)F * 2 * N, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->m_seq, matched, sizeof(int) * (size_t)F * N, hipMemcpyHostToDevice));
    c->seqF = F;
    launch_set_seq(c->stream, c->fs, c->odo_seq, F, c->p);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SRUKF_OK;
}

// A block of `count` staged frames as ONE captured graph for the next srukf_run_frames_async(ctx, *, count, ...) calls (the default
// is graphs of 8 frames + single frames; between two graph launches the device idles for ~10 us, which shows in short blocks).
// Nothing runs; the graph is dropped with the others whenever the launch sequence changes.  count <= 512.
int srukf_prepare_frames_mode(srukf_ctx* c, int count, int mode)
{
    if (!c || count < 1 || count > 512) return SRUKF_ERR_BAD_ARG;
    int rc = replay_mode_check(c, mode, "prepare_frames"); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    ReplayGraphs& g = replay_graphs(c, mode);
    if (!c->use_graph || (g.block_exec && g.block_frames == count)) return SRUKF_OK;
    if (g.block_exec) { HIPCHK(c, hipStreamSynchronize(c->stream)); hipGraphExecDestroy(g.block_exec); g.block_exec = nullptr; }   // a launch of the old one may still be in flight
    if (g.block) { hipGraphDestroy(g.block); g.block = nullptr; }
    g.block_frames = 0;
    if (mode == SRUKF_UPDATE_JOINT) { rc = joint_ensure(c, "prepare_frames"); if (rc) return rc; }      // (before the capture begins)
    rc = capture_frames(c, count, &g.block, &g.block_exec, [=] { replay_one_frame(c, mode); });
    if (rc) return rc;
    g.block_frames = count;
    return SRUKF_OK;
}

int srukf_prepare_frames(srukf_ctx* c, int count) { return srukf_prepare_frames_mode(c, count, SRUKF_UPDATE_BATCHED); }

int srukf_run_frames_async(srukf_ctx* c, int first, int count, int mode, double* d_traj)
{
    if (!c || first < 0 || count < 1) return SRUKF_ERR_BAD_ARG;
    if (!c->odo_seq || first + count > c->seqF) { c->err = "frames outside the staged sequence"; return SRUKF_ERR_DIM_MISMATCH; }
    c->joint_bad_host = false;
    { const int rcm = replay_mode_check(c, mode, "run_frames_async"); if (rcm) return rcm; }
    HIPCHK(c, hipSetDevice(c->device));
    const KDims& d = c->d;
    const bool joint = mode == SRUKF_UPDATE_JOINT;
    if (joint) { const int rcj = joint_ensure(c, "run_frames_async"); if (rcj) return rcj; }      // (before any capture begins)
    replay_prologue(c);
    // traj rows are indexed by the absolute frame counter; offset so that frame `first` lands in row 0
    double* traj = d_traj ? d_traj - (size_t)8 * first : nullptr;
    int clear = c->async_pending ? 0 : 1;
    if (c->red_r > 0 && !c->null_canonical) {
        // A state that arrived from outside with structurally null rows that are not (yet) sqrt(EPSILON) e_k — zero rows after the joint initialisation, say: the
        // run's first frame takes the launch sequence that reads those rows as they are (k_project_motion, k_pxy; replay_motion_mode), eagerly; its tail writes the
        // canonical rows, and the frames behind it run the default sequence.
        launch_set_run(c->stream, c->fs, first, clear, traj);
        replay_one_frame(c, mode);
        set_null_canonical(c);
        c->async_pending = true; c->phase = 0; c->frame_updated = false; clear = 0;
        first += 1; count -= 1;
        HIPCHK(c, hipGetLastError());
        if (count == 0) return SRUKF_OK;
    }
    launch_set_run(c->stream, c->fs, first, clear, traj);
    // "table" mode: the first frame's table of robot poses (the frames after it get theirs from their predecessor's tail)
    // (a joint frame is always the plain form: nothing is prepared in front of it)
    const FrameForm ff = joint ? FORM_PLAIN : frame_form(c);
    if (ff.robot_table) srukf_launch_sigr_rows(c->stream, d, c->w, c->X, c->S, c->sigR, c->fs, c->red_iperm, c->red_r);
    // "fused tail" mode: ... and the first frame's projection (k_project_table); every later frame is projected by its predecessor's tail
    if (ff.fused_tail()) seq_predict_fused(c, ff);
    if (c->use_graph && !c->profiling) {
        // every per-frame argument lives in HBM (frame counter, staged inputs, trajectory base), so ONE
        // captured frame replays for all frames: the 45 launches cost one hipGraphLaunch on the host
        ReplayGraphs& g = replay_graphs(c, mode);               // (per mode: a BATCHED call never replays a captured JOINT frame, nor the other way round)
        if (!g.one_exec) {
            const auto frame = [=] { replay_one_frame(c, mode); };
            int rc = capture_frames(c, 1, &g.one, &g.one_exec, frame); if (rc) return rc;
            rc = capture_frames(c, SRUKF_GRAPH_FRAMES, &g.eight, &g.eight_exec, frame); if (rc) return rc;      // (replay_launch_graphs)
        }
        if (g.block_exec && g.block_frames == count) HIPCHK(c, hipGraphLaunch(g.block_exec, c->stream));   // srukf_prepare_frames / srukf_prepare_frames_mode
        else { const int rc = replay_launch_graphs(c, g, count); if (rc) return rc; }
    } else {
        for (int f = 0; f < count; f++) replay_one_frame(c, mode);
    }
    // fp32 storage in "fused tail" mode: S and X are rounded as they are written; the float copies (srukf_get_state_f32) once per run
    if (storage_f32_like(c) && ff.fused_tail()) quantize_state(c);
    return replay_epilogue(c);
}

// Synchronous form (BATCHED or JOINT frames).  Unlike the asynchronous replay it never returns SRUKF_ERR_CLAMP_PENDING: the state before the
// block is kept, and when a frame is flagged (theta clamp of the modified Cholesky, SLAM.cpp:2279-2285, or an abandoned
// persistent launch) the block is rewound to that state, the frames before the flagged one are replayed, the flagged
// frame runs on the exact path, and the replay continues behind it.  This is that loop (dt: the block's trajectory rows on the device); the entry is below
static int run_frames_recovering(srukf_ctx* c, int first, int count, int mode, double* dt)
{
    const size_t np = c->d.np;
    bool ck_canon = c->null_canonical;
    auto checkpoint = [&](bool save) {
        hipMemcpyAsync(save ? c->ckS : c->S, save ? c->S : c->ckS, sizeof(double) * np * np, hipMemcpyDeviceToDevice, c->stream);
        hipMemcpyAsync(save ? c->ckX : c->X, save ? c->X : c->ckX, sizeof(double) * np, hipMemcpyDeviceToDevice, c->stream);
        if (save) ck_canon = c->null_canonical;
        else { if (c->null_canonical != ck_canon) { c->null_canonical = ck_canon; drop_graphs(c); } quantize_state(c); shadow_rebuild(c); }
    };
    int rc = SRUKF_OK, done = 0;
    const bool timing = g_sw.timing.load() != 0;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) { if (timing) { hipStreamSynchronize(c->stream); auto t1 = std::chrono::steady_clock::now(); fprintf(stderr, "[run_frames] %s %.0f us\n", what, std::chrono::duration<double, std::micro>(t1 - t0).count()); t0 = t1; } };
    while (done < count) {
        checkpoint(true);
        rc = srukf_run_frames_async(c, first + done, count - done, mode, dt + (size_t)8 * done);
        if (rc == SRUKF_OK) rc = srukf_synchronize(c);
        if (rc != SRUKF_ERR_CLAMP_PENDING) break;
        lap("flagged attempt");
        const int fc = c->clamp_frame_host;                               // absolute index of the first flagged frame
        if (fc < first + done || fc >= first + count) { c->err = "run_frames: flagged frame outside the block"; rc = SRUKF_ERR_HIP; break; }
        checkpoint(false);
        lap("rewind");
        const int good = fc - (first + done);
        if (good > 0) {
            rc = srukf_run_frames_async(c, first + done, good, mode, dt + (size_t)8 * done);
            if (rc == SRUKF_OK) rc = srukf_synchronize(c);
            if (rc != SRUKF_OK) break;                                    // (the same frames passed a moment ago)
        }
        rc = run_staged_frame_exact(c, fc, dt + (size_t)8 * (fc - first), mode);
        if (rc != SRUKF_OK) break;
        done = fc - first + 1;
    }
    if (rc == SRUKF_ERR_UNSUPPORTED && c->joint_bad_host) {
        // a joint frame's inputs were not finite (srukf_synchronize, or the flagged frame's repeat, names frame and row): the block leaves nothing behind — the checkpoint
        // comes back (the state before the call; behind a flagged frame of the same block, the state behind that frame)
        const std::string why = c->err;
        checkpoint(false);
        hipStreamSynchronize(c->stream);
        c->err = why;
    }
    return rc;
}

int srukf_run_frames(srukf_ctx* c, int first, int count, int mode, double* traj_host)
{
    if (!c || count < 1) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = c->d.np;
    if (!c->ckS) {
        if (srukf_dmalloc((void**)&c->ckS, sizeof(double) * np * np) != hipSuccess || srukf_dmalloc((void**)&c->ckX, sizeof(double) * np) != hipSuccess) {
            c->err = "run_frames: out of device memory (checkpoint)"; return SRUKF_ERR_NOMEM;
        }
    }
    return with_device_traj(c, count, traj_host, [=](double* dt) { return run_frames_recovering(c, first, count, mode, dt); });
}

// What the last SRUKF_ERR_CLAMP_PENDING of srukf_synchronize was about: the first flagged staged frame (frames before it
// are valid) and the first flagged pivot row.  -1 / -1 if there was none.
int srukf_clamp_info(srukf_ctx* c, int* frame, int* row)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (frame) *frame = c->clamp_frame_host;
    if (row) *row = c->clamp_row_host;
    return SRUKF_OK;
}

// Rank-aware refactorisation on / off (default on); re-derives the null set from the current state.
int srukf_set_rank_aware(srukf_ctx* c, int on)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rank_aware = on ? 1 : 0;
    return update_null_set(c);
}

// How many of the n pivots the refactorisation skips (0: the rank-aware form is off or found nothing to skip).
int srukf_null_directions(srukf_ctx* c) { return c ? (c->red_r > 0 ? c->d.n - c->red_r : 0) : SRUKF_ERR_BAD_ARG; }

// what the frames srukf_synchronize has waited for left in *c->hfs (read_fs): the first flag as an error, or SRUKF_OK
static int flagged_frames_report(srukf_ctx* c)
{
    // joint frames: the sticky pair k_joint_dx left (first hit).  A clamp flag of an EARLIER frame goes first: from that frame on nothing is valid anyway
    if (c->hfs->joint_bad_frame > 0 && !(c->hfs->clamp_rows > 0 && c->hfs->clamp_frame < c->hfs->joint_bad_frame - 1)) return joint_bad_report(c);
    if (c->hfs->clamp_rows <= 0) return SRUKF_OK;
    c->clamp_frame_host = c->hfs->clamp_frame; c->clamp_row_host = c->hfs->clamp_first;
    char b[220]; snprintf(b, sizeof b, "GMW theta clamp active on %d pivot rows (first row %d), first in staged frame %d, during async frames%s", c->hfs->clamp_rows, c->hfs->clamp_first, c->hfs->clamp_frame,
                         c->hfs->gmw_aborts > 0 ? " (a persistent factorisation launch was abandoned: the GPU is shared; see srukf_set_exclusive)" : "");
    c->err = b;
    return SRUKF_ERR_CLAMP_PENDING;
}

int srukf_synchronize(srukf_ctx* c)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->joint_bad_host = false;
    if (!c->async_pending) return SRUKF_OK;
    c->async_pending = false;
    int rc = read_fs(c);
    const bool read = rc == SRUKF_OK;
    if (read) rc = flagged_frames_report(c);
    images_block_end(c, read, rc != SRUKF_OK);                  // the frames were image frames: a flagged block comes back to its checkpoint here (X, S, matchPatch)
    return rc;
}

}  // extern "C"
