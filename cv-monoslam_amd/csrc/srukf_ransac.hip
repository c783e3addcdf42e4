// srukf_ransac.hip — 1-point RANSAC on the device: the consensus of KalmanUpdate's isUseRANSAC branch (SLAM.cpp:2097-2103, the four calls the reference names and
// never wrote) and the second look at the measurement prediction its rescue step needs.  gfx950 only.
//   srukf_ransac_consensus       every matched landmark is a hypothesis (Civera's random draw becomes exhaustive: M^2 <= 40 000 projections at N = 200):
//     k_pxy (srukf_factor.hip)   S^T DZ once more, into a buffer of this file's own — the update that follows forms it again in its own buffers
//     k_ransac_votes             one workgroup per hypothesis i: x(i) = X + K_i (z_i - h_i) restricted to the ten rows a pair needs, the projection of every
//                                matched landmark j under it, d_ij, the votes of i (wave ballots, integer adds)
//     k_ransac_pick              one workgroup: the hypothesis with the most votes (lowest index among equals), its mask and distances
//   srukf_images_ransac          the same consensus inside every frame of an image run (the switch and the record: srukf_images.hip):
//     k_ransac_votes_staged      k_ransac_votes' body on the frame's own operands — c->Ut is S^T DZ behind seq_pxy(FORM_PLAIN), z / matched are row fs->frame of
//                                z_seq / m_seq behind k_associate_staged — with the threshold in a device struct
//     k_ransac_pick_staged       k_ransac_pick's rule, the frame's row of the record, and the frame's m_seq row rewritten to the consensus set for the update
//   srukf_repredict_measurement  the slow path's measurement prediction from the posterior: k_motion with a zero control on a COPY of the state fills the table of
//                                robot poses (the sigma points' robot parts as they stand), k_project / k_meas_* as in srukf_predict_measurement.  No new kernels.
// The consensus reads the filter and writes nothing of it.  A frame predicted on the slow path has its predicted state and statistics in the context's buffers.  A frame
// on the step-wise fast path holds its motion step beside the state and its cross covariances in permuted tiles: there the state before the frame is copied and the slow
// path's predict half (k_motion, k_project, k_meas_*) runs on a copy of the fast path's checkpoint in buffers of this file's own (RansacScratch) — ~27 MB and five launches at N = 200 instead of
// reading the fast path's operands in flight; h and Si of the consensus are then the slow path's (equal to the fast path's to rounding).
// This file is built with -ffp-contract=off: tests/np_ransac.py restates its arithmetic.
#include "srukf_ctx.h"
using namespace srukf_impl;

// The votes of hypothesis i = blockIdx.x: the one text of both launch fronts.  act[k] = matched[k] && visible[k].  Ut[c][r] = (S^T DZ)^T (k_pxy), PxyR[e][c] the robot
// rows of the cross covariances.  D[i][j] = d_ij, F[i][j] = 1 for an inlier pair (rows of length N; only rows / columns of A are written), votes[i] for i in A.
__device__ __forceinline__ void ransac_votes_body(KDims d, KWeights w, srukf_params p, const double* __restrict__ X, const double* __restrict__ Ut,
                                                  const double* __restrict__ PxyR, const double* __restrict__ h, const double* __restrict__ Si,
                                                  const int* __restrict__ vis, const double* __restrict__ z, const int* __restrict__ matched, double thr,
                                                  double* __restrict__ D, unsigned char* __restrict__ F, int* __restrict__ votes)
{
    __shared__ double sh[12];                                  // Si_i^-1 (4), y_i = Si_i^-T (z_i - h_i) (2), robot rows of x(i) (4), cos / sin of its heading
    __shared__ int wv[4];
    const int i = blockIdx.x, N = d.N, n = d.n, ld = d.np, mp = d.mp;
    if (matched[i] == 0 || vis[i] == 0) return;
    if (threadIdx.x == 0) {
        const GainLm g = srukf_gain_lm(Si[4 * i], Si[4 * i + 1], Si[4 * i + 2], Si[4 * i + 3], z[2 * i], z[2 * i + 1], h[2 * i], h[2 * i + 1], 1);
        sh[0] = g.i00; sh[1] = g.i01; sh[2] = g.i10; sh[3] = g.i11; sh[4] = g.y0; sh[5] = g.y1;
        for (int e = 0; e < 4; e++) {
            double u0, u1, c;
            srukf_gain_apply(g, PxyR[(size_t)e * mp + 2 * i], PxyR[(size_t)e * mp + 2 * i + 1], u0, u1, c);
            sh[6 + e] = X[n - 4 + e] + c;
        }
        sh[10] = cos(sh[9]); sh[11] = sin(sh[9]);
    }
    if (threadIdx.x < 4) wv[threadIdx.x] = 0;
    __syncthreads();
    const GainLm g = { sh[0], sh[1], sh[2], sh[3], sh[4], sh[5], 1 };
    const double sc = w.wi * w.gamma;
    const double* u0r = Ut + (size_t)(2 * i) * ld;
    const double* u1r = Ut + (size_t)(2 * i + 1) * ld;
    int mine = 0;
    for (int j0 = 0; j0 < N; j0 += 256) {
        const int j = j0 + threadIdx.x;
        bool inl = false;
        if (j < N && matched[j] != 0 && vis[j] != 0) {
            double feat[6];
#pragma unroll
            for (int e = 0; e < 6; e++) {
                const int r = 6 * j + e;
                double a0, a1, c;
                srukf_gain_apply(g, sc * u0r[r], sc * u1r[r], a0, a1, c);
                feat[e] = X[r] + c;
            }
            double ox, oy;
            srukf_project(p, p.cam_f / p.cam_dx, p.cam_f / p.cam_dy, feat, sh[6], sh[7], sh[8], sh[10], sh[11], 0.0, 0.0, ox, oy);
            const double dx = z[2 * j] - ox, dy = z[2 * j + 1] - oy;
            const double dist = sqrt(dx * dx + dy * dy);
            inl = (ox != 0.0) && (oy != 0.0) && dist < thr;   // (an invisible prediction is (0, 0): predictMeasurement's test, SLAM.cpp:1727)
            D[(size_t)i * N + j] = dist;
            F[(size_t)i * N + j] = inl ? 1 : 0;
        }
        mine += __popcll(__ballot(inl));                       // (wave-uniform: every lane of the wave holds the wave's count)
    }
    if ((threadIdx.x & 63) == 0) wv[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) votes[i] = (wv[0] + wv[1]) + (wv[2] + wv[3]);
}

// step-wise: the caller's z / matched, the threshold as an argument
__global__ __launch_bounds__(256) void k_ransac_votes(KDims d, KWeights w, srukf_params p, const double* __restrict__ X, const double* __restrict__ Ut,
                                                      const double* __restrict__ PxyR, const double* __restrict__ h, const double* __restrict__ Si,
                                                      const int* __restrict__ vis, const double* __restrict__ z, const int* __restrict__ matched, double thr,
                                                      double* __restrict__ D, unsigned char* __restrict__ F, int* __restrict__ votes)
{
    ransac_votes_body(d, w, p, X, Ut, PxyR, h, Si, vis, z, matched, thr, D, F, votes);
}

// inside a frame of an image run (srukf_images_ransac), behind k_associate_staged and in front of k_gain / the joint kernels: z / matched are
// row fs->frame of the staged z_seq / m_seq, the threshold is the device struct's, the rest the context's live buffers as seq_pxy(FORM_PLAIN) left them (Ut is still
// S^T DZ: k_gain turns it into U^T afterwards).  A frame counter outside the staged stack writes nothing
__global__ __launch_bounds__(256) void k_ransac_votes_staged(KDims d, KWeights w, srukf_params p, StagedRansac a, const double* __restrict__ X,
                                                             const double* __restrict__ Ut, const double* __restrict__ PxyR, const double* __restrict__ h,
                                                             const double* __restrict__ Si, const int* __restrict__ vis)
{
    const int f = a.fs->frame;
    if (f < 0 || f >= a.frames) return;
    ransac_votes_body(d, w, p, X, Ut, PxyR, h, Si, vis, a.z_seq + (size_t)f * 2 * d.N, a.m_seq + (size_t)f * d.N, a.args->threshold, a.D, a.F, a.votes);
}

// The pick rule, the one text of both launch fronts: the active hypothesis with the most votes, the lowest index among equals; -1 without an active one.  All 256
// threads call it; active(i) / votes[i] are read once per index, seen(i, act, votes) is called once per index by the thread that owns it (i = tid + 256 q).
// Ends behind a barrier: every thread's reads of the active set are complete when it returns
template <class Active, class Seen>
__device__ __forceinline__ int ransac_pick_best(int N, const int* __restrict__ votes, Active active, Seen seen)
{
    __shared__ int bv[256], bi[256];
    int v = -1, b = -1;                                        // this thread's best: most votes, then lowest index (its indices ascend)
    for (int i = threadIdx.x; i < N; i += 256) {
        const bool act = active(i);
        const int vi = act ? votes[i] : 0;
        seen(i, act, vi);
        if (act && vi > v) { v = vi; b = i; }
    }
    bv[threadIdx.x] = v; bi[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const int v2 = bv[threadIdx.x + s], b2 = bi[threadIdx.x + s];
            if (b2 >= 0 && (v2 > bv[threadIdx.x] || (v2 == bv[threadIdx.x] && (bi[threadIdx.x] < 0 || b2 < bi[threadIdx.x])))) { bv[threadIdx.x] = v2; bi[threadIdx.x] = b2; }
        }
        __syncthreads();
    }
    return bi[0];
}

// res = dist[N] (doubles) | inlier[N] | votes[N] | best (ints).  One workgroup.
__global__ __launch_bounds__(256) void k_ransac_pick(int N, const int* __restrict__ vis, const int* __restrict__ matched, const double* __restrict__ D,
                                                     const unsigned char* __restrict__ F, const int* __restrict__ votes, double* __restrict__ dist,
                                                     int* __restrict__ inlier, int* __restrict__ votes_out, int* __restrict__ best_out)
{
    const int best = ransac_pick_best(N, votes, [&](int i) { return matched[i] != 0 && vis[i] != 0; }, [&](int i, bool, int vi) { votes_out[i] = vi; });
    if (threadIdx.x == 0) *best_out = best;
    for (int j = threadIdx.x; j < N; j += 256) {
        const bool act = best >= 0 && matched[j] != 0 && vis[j] != 0;
        inlier[j] = act ? (int)F[(size_t)best * N + j] : 0;
        dist[j] = act ? D[(size_t)best * N + j] : 0.0;
    }
}

// One workgroup behind k_ransac_votes_staged: k_ransac_pick's rule, the frame's row of the record (flags: bit 0 in A, bit 1 low-innovation inlier; votes; dist; the
// summary), and the frame's m_seq row rewritten to the inlier mask, which the update that follows then takes for its matches (z_seq stays).  Fewer than two active
// matches (the facade's m_nMatches < 2 branch): m_seq is left alone, the record says inlier = active, votes 0, best -1, dist 0.  The active set goes to LDS in the
// first pass (act_s, N bytes of dynamic LDS) and ransac_pick_best's barriers stand between that pass and the rewrite.  A frame counter outside the staged stack
// writes nothing
__global__ __launch_bounds__(256) void k_ransac_pick_staged(int N, StagedRansac a, const int* __restrict__ vis)
{
    extern __shared__ unsigned char act_s[];
    __shared__ int cnt[2][4];
    const int f = a.fs->frame, tid = threadIdx.x;
    if (f < 0 || f >= a.frames) return;
    int* mrow = a.m_seq + (size_t)f * N;
    int* rflags = a.rec_flags + (size_t)f * N;
    int* rvotes = a.rec_votes + (size_t)f * N;
    double* rdist = a.rec_dist + (size_t)f * N;
    int n_act = 0;
    const int best = ransac_pick_best(N, a.votes, [&](int i) { return mrow[i] != 0 && vis[i] != 0; }, [&](int i, bool act, int) { act_s[i] = act ? 1 : 0; n_act += act ? 1 : 0; });
    for (int off = 32; off > 0; off >>= 1) n_act += __shfl_down(n_act, off, 64);
    if ((tid & 63) == 0) cnt[0][tid >> 6] = n_act;
    __syncthreads();
    const int n_active = (cnt[0][0] + cnt[0][1]) + (cnt[0][2] + cnt[0][3]);
    const bool vote = n_active >= 2;
    int n_low = 0;
    for (int j = tid; j < N; j += 256) {
        const bool act = act_s[j] != 0;
        const bool inl = act && (!vote || a.F[(size_t)best * N + j] != 0);
        rflags[j] = (act ? 1 : 0) | (inl ? 2 : 0);
        rvotes[j] = (vote && act) ? a.votes[j] : 0;
        rdist[j] = (vote && act) ? a.D[(size_t)best * N + j] : 0.0;
        if (vote) mrow[j] = inl ? 1 : 0;
        n_low += inl ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) n_low += __shfl_down(n_low, off, 64);
    if ((tid & 63) == 0) cnt[1][tid >> 6] = n_low;
    __syncthreads();
    if (tid == 0) {
        const int nl = (cnt[1][0] + cnt[1][1]) + (cnt[1][2] + cnt[1][3]);
        RansacSummary o;
        o.best = vote ? best : -1; o.n_active = n_active; o.n_low = nl; o.outlier = (vote && nl < n_active) ? 1 : 0;
        a.rec_sum[f] = o;
    }
}

__global__ void k_set_ransac_args(RansacArgs* dst, RansacArgs v) { *dst = v; }

void launch_ransac_staged(hipStream_t st, KDims d, KWeights w, srukf_params p, StagedRansac a, const double* X, const double* Ut, const double* PxyR, const double* h,
                          const double* Si, const int* vis)
{
    hipLaunchKernelGGL(k_ransac_votes_staged, dim3(d.N), dim3(256), 0, st, d, w, p, a, X, Ut, PxyR, h, Si, vis);
    hipLaunchKernelGGL(k_ransac_pick_staged, dim3(1), dim3(256), (size_t)((d.N + 7) / 8 * 8), st, d.N, a, vis);
}
void launch_set_ransac_args(hipStream_t st, RansacArgs* dst, RansacArgs v) { hipLaunchKernelGGL(k_set_ransac_args, dim3(1), dim3(1), 0, st, dst, v); }

namespace srukf_impl {

void ransac_scratch_free(RansacScratch& s, hipStream_t st)
{
    void* bufs[] = { s.Ut, s.D, s.F, s.votes, s.zin, s.res, s.X, s.S, s.odo, s.sigR, s.Cm, s.Z, s.DZ, s.h, s.PxyR, s.mpart, s.fs, s.rq_in, s.rq_out, s.rq_scr };
    for (void* b : bufs) if (b) srukf_dfree_on(b, st);
    s = RansacScratch{};
}

}  // namespace srukf_impl

#define RS_ALLOC(ptr, count) do { if (!(ptr)) { if (srukf_dmalloc(&(ptr), sizeof(*(ptr)) * (size_t)(count)) != hipSuccess) { (void)hipGetLastError(); c->err = "ransac: out of device memory"; return SRUKF_ERR_NOMEM; } \
    HIPCHK(c, hipMemsetAsync((ptr), 0, sizeof(*(ptr)) * (size_t)(count), c->stream)); } } while (0)

// the copy of the state (both calls) and the six doubles of an odometry pair
static int ransac_ensure_copy(srukf_ctx* c)
{
    RansacScratch& s = c->ransac;
    const size_t np = c->d.np;
    RS_ALLOC(s.X, np); RS_ALLOC(s.S, np * np); RS_ALLOC(s.odo, 8); RS_ALLOC(s.Cm, (np + 64) * 4); RS_ALLOC(s.fs, 1);
    return SRUKF_OK;
}

static int ransac_ensure(srukf_ctx* c, bool fast)
{
    RansacScratch& s = c->ransac;
    const KDims& d = c->d;
    const size_t np = d.np, mp = d.mp, N = d.N;
    RS_ALLOC(s.Ut, mp * np); RS_ALLOC(s.D, N * N); RS_ALLOC(s.F, (N * N + 7) / 8 * 8); RS_ALLOC(s.votes, N);
    RS_ALLOC(s.zin, mp + (N + 1) / 2); RS_ALLOC(s.res, N + N + 1);
    if (!fast) return SRUKF_OK;
    const int rc = ransac_ensure_copy(c); if (rc) return rc;
    RS_ALLOC(s.sigR, (size_t)d.L * 8 + 8); RS_ALLOC(s.Z, (size_t)d.L * mp); RS_ALLOC(s.DZ, np * mp);
    RS_ALLOC(s.h, mp + 4 * N + (N + 1) / 2); RS_ALLOC(s.PxyR, 5 * mp); RS_ALLOC(s.mpart, srukf_meas_part_doubles(d.mp));
    return SRUKF_OK;
}

extern "C" {

int srukf_ransac_consensus(srukf_ctx* c, const double* z, const int* matched, double threshold, int* inlier, int* votes, double* dist, int* best)
{
    if (!c || !z || !matched) return SRUKF_ERR_BAD_ARG;
    if (c->phase != 2) { c->err = "ransac_consensus outside predict_measurement .. update"; return SRUKF_ERR_SEQUENCE; }
    HIPCHK(c, hipSetDevice(c->device));
    const KDims& d = c->d;
    const int N = d.N;
    if (N == 0) { if (best) *best = -1; return SRUKF_OK; }
    const bool fast = c->step_fast;
    int rc = ransac_ensure(c, fast); if (rc) return rc;
    RansacScratch& s = c->ransac;
    const size_t np = d.np, mp = d.mp;
    const double *X = c->X, *S = c->S, *DZ = c->DZ, *h = c->h, *Si = c->Si, *PxyR = c->PxyR;
    const int* vis = c->vis;
    if (fast) {
        // the state before the frame is the fast path's checkpoint (ckS / ckX: what a flagged frame is repeated from): the slow path's predict half on a copy of it
        step_ck_join(c);
        double* hs = c->hstage;
        memcpy(hs, c->step_odo, sizeof(double) * 6);
        HIPCHK(c, hipMemcpyAsync(s.odo, hs, sizeof(double) * 6, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(s.X, c->ckX, sizeof(double) * np, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(s.S, c->ckS, sizeof(double) * np * np, hipMemcpyDeviceToDevice, c->stream));
        double* sSi = s.h + mp; int* svis = (int*)(s.h + mp + 4 * (size_t)N);
        srukf_launch_motion(c->stream, d, c->w, c->p, s.X, s.S, s.sigR, s.Cm, s.fs, nullptr, s.odo, RankArgs{});
        srukf_launch_project(c->stream, d, c->w, c->p, s.X, s.S, s.sigR, s.Z, s.DZ, s.fs);
        srukf_launch_meas_stats(c->stream, d, c->w, s.X, s.sigR, s.Z, s.mpart, s.h, sSi, svis, s.PxyR);
        HIPCHK(c, hipStreamSynchronize(c->stream));           // (hstage is free again)
        X = s.X; S = s.S; DZ = s.DZ; h = s.h; Si = sSi; vis = svis; PxyR = s.PxyR;
    }
    double* hs = c->hstage;
    memcpy(hs, z, sizeof(double) * 2 * N);
    memcpy(hs + mp, matched, sizeof(int) * N);
    HIPCHK(c, hipMemcpyAsync(s.zin, hs, sizeof(double) * mp + sizeof(int) * N, hipMemcpyHostToDevice, c->stream));
    const int* mdev = (const int*)(s.zin + mp);
    srukf_launch_pxy(c->stream, d, DZ, S, s.Ut, c->pxy_tiles, c->n_pxy_tiles, c->w, MeasArgs{});
    hipLaunchKernelGGL(k_ransac_votes, dim3(N), dim3(256), 0, c->stream, d, c->w, c->p, X, s.Ut, PxyR, h, Si, vis, s.zin, mdev, threshold, s.D, s.F, s.votes);
    int* rint = (int*)(s.res + N);
    hipLaunchKernelGGL(k_ransac_pick, dim3(1), dim3(256), 0, c->stream, N, vis, mdev, s.D, s.F, s.votes, s.res, rint, rint + N, rint + 2 * N);
    const size_t out_bytes = sizeof(double) * N + sizeof(int) * (2 * (size_t)N + 1);
    HIPCHK(c, hipMemcpyAsync(hs, s.res, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    const int* hi = (const int*)(hs + N);
    if (dist) memcpy(dist, hs, sizeof(double) * N);
    if (inlier) memcpy(inlier, hi, sizeof(int) * N);
    if (votes) memcpy(votes, hi + N, sizeof(int) * N);
    if (best) *best = hi[2 * N];
    return SRUKF_OK;
}

int srukf_repredict_measurement(srukf_ctx* c, double* h, double* Si, int* visible)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (!c->frame_updated || c->phase != 0) { c->err = "repredict_measurement without an update of this frame before it"; return SRUKF_ERR_SEQUENCE; }
    HIPCHK(c, hipSetDevice(c->device));
    const KDims& d = c->d;
    const int N = d.N;
    if (N == 0) { c->phase = 2; return SRUKF_OK; }
    int rc = ransac_ensure_copy(c); if (rc) return rc;
    RansacScratch& s = c->ransac;
    const size_t np = d.np, mp = d.mp;
    // what the first update's tail prepared for the next frame (projected sigma points, a launch submitted ahead, cached views) describes a state the second update
    // replaces, and this call overwrites Z / DZ / the table under it
    step_invalidate(c);
    c->step_fast = false;
    // The table of robot poses (sigR) as k_motion leaves it for a control of zero: the robot parts of the sigma points of (X, S) themselves and, in its last row,
    // sum_c w_c (r_c - xr), which k_meas_final reads.  k_motion's own results (robot mean, last four columns of S, frame scalars, Cm) go to the copy and to scratch:
    // nothing of the filter but sigR is written.  (k_sigr_rows fills the same table from the state as it stands, but it reads the control from the live frame
    // scalars, needs the rank-aware form's index table — absent below n = 128 or with the form switched off — and leaves that last row unwritten.)
    HIPCHK(c, hipMemsetAsync(s.odo, 0, sizeof(double) * 8, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.X, c->X, sizeof(double) * np, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.S, c->S, sizeof(double) * np * np, hipMemcpyDeviceToDevice, c->stream));
    srukf_launch_motion(c->stream, d, c->w, c->p, s.X, s.S, c->sigR, s.Cm, s.fs, nullptr, s.odo, RankArgs{});
    seq_predict_measurement(c, FORM_SEPARATE_STATS);
    double* hs = c->hstage;
    const size_t out_bytes = sizeof(double) * (mp + 4 * (size_t)N) + sizeof(int) * N;
    HIPCHK(c, hipMemcpyAsync(hs, c->h, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (h) memcpy(h, hs, sizeof(double) * 2 * N);
    if (Si) memcpy(Si, hs + mp, sizeof(double) * 4 * N);
    if (visible) memcpy(visible, hs + mp + 4 * (size_t)N, sizeof(int) * N);
    c->phase = 2;
    return SRUKF_OK;
}

}  // extern "C"
