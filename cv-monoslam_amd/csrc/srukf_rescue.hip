// srukf_rescue.hip — the rescue gate of 1-point RANSAC on the device: would a match the consensus dropped be rescued?  gfx950 only.
//   k_rescue_gate          step-wise (srukf_rescue_gate): the caller's z / matched / inlier, the posterior (X, S) read in place behind a srukf_update
//   k_rescue_gate_staged   the same body behind the tail of a frame of an image run (srukf_images_rescue_gate; the switch and the record: srukf_images.hip), the
//                          candidates from the frame's row of the consensus record, chi2 in a device struct
//   k_rescue_sum_staged    one workgroup behind it: the frame's counts (what the snapshot guard and srukf_get_image_rescue read)
// The gate reads the filter and writes nothing of it.  No polling, no flags between workgroups, no atomics: every dependency is a launch boundary.
// This file is built with -ffp-contract=off: tests/np_rescue.py restates the rule.
#include "srukf_ctx.h"
#include "srukf_motion.h"
#include "srukf_meas.h"
using namespace srukf_impl;

// ---- the rescue gate: would a match the consensus dropped be rescued? ----
// The one text of both launch fronts.  Landmark k = blockIdx.x; cand: it is a candidate (in A, no low-innovation inlier, in a frame that has candidates).  A candidate's
// workgroup forms h', Si', visible' of srukf_repredict_measurement for the posterior (X, S): the sigma points of project_item<INLINE_ROBOT> under a control of zero
// (MotionCtl{ 0, 0, 0, 1, 0 }, zero motion-noise rows) — item 0 the centre, item ii >= 1 the +/- pair of row ii - 1 of the augmented sqrt matrix — in trips of 256
// items, the five sums meas_final_tail needs (sum (Z_c - Z_0), the second moments with wi_sr) reduced in a fixed order: lanes by __shfl_down, then the four waves
// through LDS as (w0 + w1) + (w2 + w3).  Thread 0 finishes: meas_final_tail in its "defer" form (it then reads neither the table of robot poses nor Z: rows 0 - 2 of
// Z come through MeasPre, the robot rows of Pxy it stores — raw, here zero — go to the gate's own scratch), then dataAssociation's gate (1977) on y = Si'^-T (z - h')
// by forward substitution, strictly below chi2.  Every other workgroup zeroes its entry of the row and returns.  S is upper triangular: only col >= i is read
__device__ __forceinline__ void rescue_gate_body(const KDims& d, const KWeights& w, const srukf_params& p, const double* __restrict__ X, const double* __restrict__ S,
                                                 const double* __restrict__ z, bool cand, double chi2, const RescueRow& row, const RescueScratch& scr)
{
    __shared__ double red[4][5];
    __shared__ double2 zpre[3];
    const int k = blockIdx.x, tid = threadIdx.x, n = d.n, Na = d.Na, ld = d.np;
    if (!cand) {
        if (tid == 0) {
            row.flags[k] = 0; row.chi2[k] = 0.0; row.h2[2 * k] = 0.0; row.h2[2 * k + 1] = 0.0;
            for (int e = 0; e < 4; e++) row.Si2[4 * k + e] = 0.0;
        }
        return;
    }
    const double f1 = p.cam_f / p.cam_dx, f2 = p.cam_f / p.cam_dy;
    const MotionCtl mc = { 0, 0, 0, 1, 0 };
    const double mnoise[3] = { 0, 0, 0 };
    double base[6], xr[4];
#pragma unroll
    for (int e = 0; e < 6; e++) base[e] = X[6 * k + e];
#pragma unroll
    for (int e = 0; e < 4; e++) xr[e] = X[n - 4 + e];
    // the centre point: every thread forms it (the sums are taken around it)
    double s0[4], c0s, s0s, z0x, z0y;
    srukf_motion_centre(mc, xr, s0, c0s, s0s);
    srukf_project(p, f1, f2, base, s0[0], s0[1], s0[2], c0s, s0s, 0.0, 0.0, z0x, z0y);
    double s[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    for (int t0 = 0; t0 <= Na; t0 += 256) {
        const int ii = t0 + tid;
        if (ii < 1 || ii > Na) continue;                           // (item 0 is the centre: its own term is zero)
        const int i = ii - 1;
        double dev[6] = { 0, 0, 0, 0, 0, 0 }, srow[4] = { 0, 0, 0, 0 };
        if (i < n) {
#pragma unroll
            for (int e = 0; e < 6; e++) { const int col = 6 * k + e; dev[e] = (col >= i) ? S[(size_t)i * ld + col] : 0.0; }
#pragma unroll
            for (int e = 0; e < 4; e++) { const int col = n - 4 + e; srow[e] = (col >= i) ? S[(size_t)i * ld + col] : 0.0; }
        }
        double e0 = 0.0, e1 = 0.0;                                 // pixel-noise sigma rows n + 3, n + 4
        if (i == n + 3) e0 = p.sigma_measure; else if (i == n + 4) e1 = p.sigma_measure;
#pragma unroll
        for (int sgn = 0; sgn < 2; sgn++) {
            const double gq = sgn ? -w.gamma : w.gamma;
            double feat[6], q0, q1, r[4], c2, s2, ox, oy;
            srukf_sigma_feat(base, dev, e0, e1, gq, feat, q0, q1);
            srukf_motion_point(mc, xr, srow, mnoise, gq, r, c2, s2);
            srukf_project(p, f1, f2, feat, r[0], r[1], r[2], c2, s2, q0, q1, ox, oy);
            if (sgn == 0 && ii <= 2) zpre[ii] = make_double2(ox, oy);      // rows 1 and 2 of Z: what the Si factor's first Householder step names
            const double dx = ox - z0x, dy = oy - z0y;
            s[0] += dx; s[1] += dy;
            const double a = w.wi_sr * dx, b = w.wi_sr * dy;
            s[2] += a * a; s[3] += a * b; s[4] += b * b;
        }
    }
#pragma unroll
    for (int q = 0; q < 5; q++) {
        double v = s[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    double t[MEAS_NS];
#pragma unroll
    for (int q = 0; q < MEAS_NS; q++) t[q] = q < 5 ? (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]) : 0.0;
    MeasPre pre; pre.z[0] = make_double2(z0x, z0y); pre.z[1] = zpre[1]; pre.z[2] = zpre[2];
    MeasOut o;
    meas_final_tail(d, w, /* sigR, Z: not read in this form */ X, X, t, row.h2, row.Si2, scr.vis, scr.PxyR, k, 1, &pre, &o, 0);
    int fl = 1; double dist = 0.0;
    if (o.vis && o.si[0] != 0.0 && o.si[3] != 0.0) {
        const double v0 = z[2 * k] - o.h[0], v1 = z[2 * k + 1] - o.h[1];
        const double y0 = v0 / o.si[0], y1 = (v1 - o.si[1] * y0) / o.si[3];
        dist = y0 * y0 + y1 * y1;
        if (dist < chi2) fl |= 2;
    }
    row.flags[k] = fl; row.chi2[k] = dist;
}

// step-wise: the caller's z / matched / inlier, the threshold as an argument
__global__ __launch_bounds__(256) void k_rescue_gate(KDims d, KWeights w, srukf_params p, const double* __restrict__ X, const double* __restrict__ S,
                                                     const double* __restrict__ z, const int* __restrict__ matched, const int* __restrict__ inlier, int frame_has,
                                                     double chi2, RescueRow row, RescueScratch scr)
{
    const int k = blockIdx.x;
    rescue_gate_body(d, w, p, X, S, z, frame_has != 0 && matched[k] != 0 && inlier[k] == 0, chi2, row, scr);
}

// behind the tail of a frame of an image run (srukf_images_rescue_gate), in front of the archive search: X and S are the frame's posterior — the tail's k_syrk launch
// has added the pending dX, its last launch has written S in state order: what srukf_get_state returns —, the frame is fs->frame - 1 (the tail has advanced the
// counter, as k_archive_search_staged finds it), the candidates come from the frame's row of the consensus record, z from its row of z_seq, chi2 from the device
// struct.  A frame counter outside the staged stack writes nothing
__global__ __launch_bounds__(256) void k_rescue_gate_staged(KDims d, KWeights w, srukf_params p, StagedRescue a, const double* __restrict__ X, const double* __restrict__ S)
{
    const int f = a.fs->frame - 1, N = d.N, k = blockIdx.x;
    if (f < 0 || f >= a.frames) return;
    const RansacSummary sm = a.rs_sum[f];
    const bool frame_has = sm.n_active >= 2 && sm.n_low > 0 && sm.n_low < sm.n_active;
    const RescueRow row = { a.rec.flags + (size_t)f * N, a.rec.h2 + (size_t)f * 2 * N, a.rec.Si2 + (size_t)f * 4 * N, a.rec.chi2 + (size_t)f * N };
    rescue_gate_body(d, w, p, X, S, a.z_seq + (size_t)f * 2 * N, frame_has && (a.rs_flags[(size_t)f * N + k] & 3) == 1, a.args->chi2, row, a.scr);
}

// one workgroup behind k_rescue_gate_staged: the frame's summary, integer counts of its row of flags
__global__ __launch_bounds__(256) void k_rescue_sum_staged(int N, StagedRescue a)
{
    __shared__ int cnt[2][4];
    const int f = a.fs->frame - 1, tid = threadIdx.x;
    if (f < 0 || f >= a.frames) return;
    const int* fl = a.rec.flags + (size_t)f * N;
    int nc = 0, nh = 0;
    for (int j = tid; j < N; j += 256) { const int v = fl[j]; nc += v & 1; nh += (v >> 1) & 1; }
    for (int off = 32; off > 0; off >>= 1) { nc += __shfl_down(nc, off, 64); nh += __shfl_down(nh, off, 64); }
    if ((tid & 63) == 0) { cnt[0][tid >> 6] = nc; cnt[1][tid >> 6] = nh; }
    __syncthreads();
    if (tid == 0) { RescueSummary o; o.n_cand = (cnt[0][0] + cnt[0][1]) + (cnt[0][2] + cnt[0][3]); o.n_high = (cnt[1][0] + cnt[1][1]) + (cnt[1][2] + cnt[1][3]); a.rec_sum[f] = o; }
}

__global__ void k_set_rescue_args(RescueArgs* dst, RescueArgs v) { *dst = v; }

void launch_rescue_gate_staged(hipStream_t st, KDims d, KWeights w, srukf_params p, StagedRescue a, const double* X, const double* S)
{
    hipLaunchKernelGGL(k_rescue_gate_staged, dim3(d.N), dim3(256), 0, st, d, w, p, a, X, S);
    hipLaunchKernelGGL(k_rescue_sum_staged, dim3(1), dim3(256), 0, st, d.N, a);
}
void launch_rescue_gate(hipStream_t st, KDims d, KWeights w, srukf_params p, const double* X, const double* S, const double* z, const int* matched, const int* inlier,
                        int frame_has, double chi2, RescueRow row, RescueScratch scr)
{
    hipLaunchKernelGGL(k_rescue_gate, dim3(d.N), dim3(256), 0, st, d, w, p, X, S, z, matched, inlier, frame_has, chi2, row, scr);
}
void launch_set_rescue_args(hipStream_t st, RescueArgs* dst, RescueArgs v) { hipLaunchKernelGGL(k_set_rescue_args, dim3(1), dim3(1), 0, st, dst, v); }


#define RQ_ALLOC(ptr, count) do { if (!(ptr)) { if (srukf_dmalloc(&(ptr), sizeof(*(ptr)) * (size_t)(count)) != hipSuccess) { (void)hipGetLastError(); c->err = "rescue_gate: out of device memory"; return SRUKF_ERR_NOMEM; } \
    HIPCHK(c, hipMemsetAsync((ptr), 0, sizeof(*(ptr)) * (size_t)(count), c->stream)); } } while (0)

extern "C" {

// The rescue gate, step-wise: for the matches the consensus dropped, srukf_repredict_measurement's h, Si, visible from the posterior and the
// chi-square test, in one launch that reads X and S in place.  It joins what srukf_repredict_measurement joins first (the checkpoint copies that still read the
// state) and nothing else: no step_invalidate, phase and state as they were — what the first update's tail prepared for the next frame stands
int srukf_rescue_gate(srukf_ctx* c, const double* z, const int* matched, const int* inlier, double chi2, int* flags, double* h2, double* Si2, double* chi2_out, int* n_high)
{
    if (!c || !z || !matched || !inlier) return SRUKF_ERR_BAD_ARG;
    if (!std::isfinite(chi2) || chi2 <= 0.0) { c->err = "rescue_gate: chi2 must be finite and positive"; return SRUKF_ERR_BAD_ARG; }
    if (!c->frame_updated || c->phase != 0) { c->err = "rescue_gate without an update of this frame before it"; return SRUKF_ERR_SEQUENCE; }
    const KDims& d = c->d;
    const int N = d.N;
    if (n_high) *n_high = 0;
    if (N == 0) return SRUKF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    RansacScratch& s = c->ransac;
    const size_t mp = d.mp, n = (size_t)N, ints = (n + 1) / 2;
    RQ_ALLOC(s.rq_in, mp + 2 * ints); RQ_ALLOC(s.rq_out, 7 * n + ints); RQ_ALLOC(s.rq_scr, 5 * mp + ints);
    int n_active = 0, n_low = 0;
    for (int k = 0; k < N; k++) { n_active += matched[k] ? 1 : 0; n_low += (matched[k] && inlier[k]) ? 1 : 0; }
    const int frame_has = (n_active >= 2 && n_low > 0 && n_low < n_active) ? 1 : 0;      // rescueHighInnovationInliers' condition
    step_ck_join(c);
    double* hs = c->hstage;
    memcpy(hs, z, sizeof(double) * 2 * n);
    int* hm = (int*)(hs + mp);
    memcpy(hm, matched, sizeof(int) * n); memcpy(hm + 2 * ints, inlier, sizeof(int) * n);
    HIPCHK(c, hipMemcpyAsync(s.rq_in, hs, sizeof(double) * (mp + 2 * ints), hipMemcpyHostToDevice, c->stream));
    const int* dm = (const int*)(s.rq_in + mp);
    const RescueRow row = { (int*)(s.rq_out + 7 * n), s.rq_out, s.rq_out + 2 * n, s.rq_out + 6 * n };
    launch_rescue_gate(c->stream, d, c->w, c->p, c->X, c->S, s.rq_in, dm, dm + 2 * ints, frame_has, chi2, row, RescueScratch{ (int*)(s.rq_scr + 5 * mp), s.rq_scr });
    HIPCHK(c, hipMemcpyAsync(hs, s.rq_out, sizeof(double) * (7 * n + ints), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    const int* hf = (const int*)(hs + 7 * n);
    if (h2) memcpy(h2, hs, sizeof(double) * 2 * n);
    if (Si2) memcpy(Si2, hs + 2 * n, sizeof(double) * 4 * n);
    if (chi2_out) memcpy(chi2_out, hs + 6 * n, sizeof(double) * n);
    if (flags) memcpy(flags, hf, sizeof(int) * n);
    if (n_high) for (int k = 0; k < N; k++) *n_high += (hf[k] >> 1) & 1;
    return SRUKF_OK;
}

}  // extern "C"
