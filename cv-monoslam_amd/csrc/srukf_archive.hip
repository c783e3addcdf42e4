// srukf_archive.hip — archived landmarks found in the frame by appearance (ours, not the reference's: its loop points are a 15-px test of the
// projected mean against the corners of a detection pass, SLAM.cpp:699-727).  gfx950 only.
//   srukf_archive_set     the archive on the handle: per record its state, 6 x 6 square-root block and appearance record (the layouts of srukf_insert_landmarks)
//   srukf_archive_search  every record, every call, nothing of the filter written:
//     k_archive_predict   one workgroup per record: the unscented transform over [record 6 | robot 4 | pixel noise 2] through srukf_project -> h, Si, visible,
//                         the record's Cartesian mean
//     k_warp_patch        (srukf_assoc.hip, unchanged) on the archive's arrays: the 17 x 17 template of every visible record under the current pose
//     k_archive_search    one workgroup per visible record: the frame bytes of the gate's bounding box in LDS, the normalised cross correlation of every gated
//                         candidate from exact integer sums, the first maximum in row-major order.  The gate (Si^T Si, its inverse, the distance) and the
//                         first-maximum reduction are the association's (srukf_patch.h); the window rule, the score and the byte staging are this file's
//   srukf_images_search_archive  the same search behind every frame of an image run: seq_archive_search = k_block_cov (P4, the launch srukf_get_robot
//                         makes) + k_archive_frame_begin (pose, templates and hit counter zeroed) + k_archive_predict + k_warp_patch + k_archive_search_staged, which
//                         is k_archive_search's body (one text: archive_search_body) on the frame's staged image, writing the frame's row of the search record
// The robot pose and its 4 x 4 covariance are what srukf_get_robot returns at that moment (that call is made); every buffer written is the archive's own, and the
// staging area is the archive's own pinned block (the context's may hold a statistics mirror the next srukf_predict_measurement reads).
// This file is built with -ffp-contract=off: tests/np_archive.py restates its arithmetic.
#include "srukf_ctx.h"
#include "srukf_crtrig.h"
#include "srukf_patch.h"
#include <cmath>
using namespace srukf_impl;

#define AR_NA 12                       // record 6 | robot 4 | pixel noise 2
#define AR_L (2 * AR_NA + 1)
#define AR_CAP_MAX 40
#define AR_RG_W (2 * AR_CAP_MAX + 1 + 2 * PT_MATCH_HALF)      // 97: bytes per side every candidate of the widest window can touch
#define AR_RG_STRIDE 100                              // LDS row stride of the staged region (whole dwords per row)

// upper Cholesky factor by the rule of k_lm_record: d_j = max(eps, P_jj - sum_{m<j} S_mj^2), S_jj = sqrt(d_j), S_ji = (P_ji - sum_{m<j} S_mj S_mi) / S_jj, sums in ascending m
template <int D> __device__ __forceinline__ void ar_chol(const double* P, double eps, double* S)
{
    for (int e = 0; e < D * D; e++) S[e] = 0.0;
    for (int j = 0; j < D; j++) {
        double s = 0.0;
        for (int m = 0; m < j; m++) s += S[D * m + j] * S[D * m + j];
        double d = P[D * j + j] - s;
        d = d > eps ? d : eps;
        const double sjj = sqrt(d);
        S[D * j + j] = sjj;
        for (int i = j + 1; i < D; i++) {
            double q = 0.0;
            for (int m = 0; m < j; m++) q += S[D * m + j] * S[D * m + i];
            S[D * j + i] = (P[D * j + i] - q) / sjj;
        }
    }
}

// rob = pose (4) | P4 (16).  Sigma point 0 is the mean, 1 + i / 1 + 12 + i are mean +- gamma * row i of S_aug = blockdiag(S66, S_rr, sigma_measure I2); thread c < 25
// projects sigma point c; thread 0 forms the statistics, every sum in ascending sigma index.
__global__ __launch_bounds__(64) void k_archive_predict(srukf_params p, KWeights w, const double* __restrict__ X6, const double* __restrict__ S66,
                                                        const double* __restrict__ rob, double* __restrict__ h, double* __restrict__ Si, int* __restrict__ vis,
                                                        double* __restrict__ xyz)
{
    __shared__ double srr[16];
    __shared__ double Z[2 * AR_L];
    const int k = blockIdx.x, c = threadIdx.x;
    if (c == 0) ar_chol<4>(rob + 4, p.epsilon, srr);
    __syncthreads();
    if (c < AR_L) {
        double mu[AR_NA], row[AR_NA];
        for (int e = 0; e < 6; e++) mu[e] = X6[6 * k + e];
        for (int e = 0; e < 4; e++) mu[6 + e] = rob[e];
        mu[10] = 0.0; mu[11] = 0.0;
        for (int e = 0; e < AR_NA; e++) row[e] = 0.0;
        double g = 0.0;
        if (c > 0) {
            const int i = (c - 1) % AR_NA;
            g = c <= AR_NA ? w.gamma : -w.gamma;
            if (i < 6) for (int e = 0; e < 6; e++) row[e] = S66[36 * (size_t)k + 6 * i + e];
            else if (i < 10) for (int e = 0; e < 4; e++) row[6 + e] = srr[4 * (i - 6) + e];
            else row[i] = p.sigma_measure;
        }
        double s[AR_NA];
        for (int e = 0; e < AR_NA; e++) s[e] = mu[e] + g * row[e];
        const double cs = cos(s[9]), sn = sin(s[9]);
        double ox, oy;
        srukf_project(p, p.cam_f / p.cam_dx, p.cam_f / p.cam_dy, s, s[6], s[7], s[8], cs, sn, s[10], s[11], ox, oy);
        Z[2 * c] = ox; Z[2 * c + 1] = oy;
    }
    __syncthreads();
    if (c != 0) return;
    double sx = 0.0, sy = 0.0, p00 = 0.0, p01 = 0.0, p11 = 0.0;
    // A sigma point outside the projection's validity border has its undistorted pixel zeroed (coordinatesCamera2Image, 3341-3345); the distortion that follows maps
    // that (0, 0) to c (1 - 1 / d), a fraction of a pixel from the origin (0.037, 0.028 with the default intrinsics) — not to zero, so the reference's `!= 0` never
    // sees it.  A valid pixel lies 10 px inside the image before the distortion, which moves it by less than a pixel: below 1 in either coordinate = zeroed.
    bool ok = Z[0] >= 1.0 && Z[1] >= 1.0;
    for (int q = 1; q < AR_L; q++) {
        sx += Z[2 * q]; sy += Z[2 * q + 1];
        const double dx = Z[2 * q] - Z[0], dy = Z[2 * q + 1] - Z[1];
        p00 += dx * dx; p01 += dx * dy; p11 += dy * dy;
        ok = ok && Z[2 * q] >= 1.0 && Z[2 * q + 1] >= 1.0;
    }
    h[2 * k] = w.wm0 * Z[0] + w.wi * sx;
    h[2 * k + 1] = w.wm0 * Z[1] + w.wi * sy;
    const double Pi[4] = { w.wi * p00, w.wi * p01, w.wi * p01, w.wi * p11 };
    double sf[4];
    ar_chol<2>(Pi, p.epsilon, sf);
    for (int e = 0; e < 4; e++) Si[4 * k + e] = sf[e];
    vis[k] = ok ? 1 : 0;
    double sth, cth, sph, cph;
    crt_sincos(X6[6 * k + 3], &sth, &cth);                     // (correctly rounded: the warp's bytes depend on the last bit of this point)
    crt_sincos(X6[6 * k + 4], &sph, &cph);
    const double rho = X6[6 * k + 5];
    xyz[3 * k] = X6[6 * k] + cph * sth / rho;
    xyz[3 * k + 1] = X6[6 * k + 1] - sph / rho;
    xyz[3 * k + 2] = X6[6 * k + 2] + cph * cth / rho;
}

// One workgroup per record.  Window: half_x = clamp(ceil(sqrt(chi2 Pi00)), 8, cap), half_y from Pi11 (Pi = Si^T Si): the bounding box of the gate ellipse; candidate c
// (row-major) has the centre (i, j) = ((int)h_x - half_x + c % wx, (int)h_y - half_y + c / wx) and is skipped (cc = 0) when its 17 x 17 patch leaves the image or
// e^T Pi^-1 e >= chi2, e = (i - h_x, j - h_y).  With v the frame bytes under the template and t the template bytes, all sums exact integers:
//   (NP = PT_TMPL_BYTES)  A = NP sum(vt) - sum(v) sum(t),  B = NP sum(v^2) - sum(v)^2,  C = NP sum(t^2) - sum(t)^2,  cc = (B == 0 || C == 0) ? 0 : (double)A / sqrt((double)B (double)C)
// The staged bytes stay bytes (<= 97 x 97 in rows of 100): neighbouring lanes take neighbouring centres, so a wave's byte reads of one template position fall into
// <= 17 consecutive dwords of a row (and the rows of a wave that spans two window rows lie 25 banks apart); the template is read as one broadcast dword per position.
// the body of k_archive_search and k_archive_search_staged for record k: z (2), matched, corr are the record's own slots.  256 threads
__device__ __forceinline__ void archive_search_body(int k, const srukf_params& p, int cap, double thr, double chi2, const unsigned char* __restrict__ image,
                                                    const double* __restrict__ h, const double* __restrict__ Si, const unsigned char* __restrict__ tmpl, int tmpl_stride,
                                                    double* __restrict__ z, int* __restrict__ matched, double* __restrict__ corr)
{
    __shared__ unsigned char rg[AR_RG_W * AR_RG_STRIDE];
    __shared__ int tm[PT_TMPL_BYTES];
    __shared__ int tsum[2];
    __shared__ double bestv[256];
    __shared__ int besti[256];
    const int tid = threadIdx.x;
    const int W = (int)p.image_w, H = (int)p.image_h;
    const double px = h[2 * k], py = h[2 * k + 1];
    const PatchGate g = patch_gate(Si + 4 * k);
    const double capd = (double)min(max(cap, PT_MATCH_HALF), AR_CAP_MAX);
    const int half_x = (int)fmin(fmax(ceil(sqrt(chi2 * g.p00)), (double)PT_MATCH_HALF), capd);   // (a NaN ends as 8: fmax / fmin return the other operand)
    const int half_y = (int)fmin(fmax(ceil(sqrt(chi2 * g.p11)), (double)PT_MATCH_HALF), capd);
    const int wx = 2 * half_x + 1, wy = 2 * half_y + 1;
    const int x0 = (int)px - half_x, y0 = (int)py - half_y;
    const int rw = wx + 2 * PT_MATCH_HALF, rh = wy + 2 * PT_MATCH_HALF, rx0 = x0 - PT_MATCH_HALF, ry0 = y0 - PT_MATCH_HALF;   // rw, rh <= 97
    for (int e = tid; e < rw * rh; e += 256) {
        const int ry = e / rw, rx = e % rw, yy = ry0 + ry, xx = rx0 + rx;
        rg[ry * AR_RG_STRIDE + rx] = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? image[(size_t)yy * W + xx] : (unsigned char)0;
    }
    const unsigned char* mp = tmpl + (size_t)k * tmpl_stride;
    for (int e = tid; e < PT_TMPL_BYTES; e += 256) tm[e] = mp[e];
    __syncthreads();
    if (tid < 64) {                                            // sum(t), sum(t^2): one wave, integer adds (any order gives the same sums)
        int a = 0, b = 0;
        for (int e = tid; e < PT_TMPL_BYTES; e += 64) { const int t = tm[e]; a += t; b += t * t; }
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
        if (tid == 0) { tsum[0] = a; tsum[1] = b; }
    }
    __syncthreads();
    const long long St = tsum[0], Stt = tsum[1];
    const long long C = PT_TMPL_BYTES * Stt - St * St;
    double bv = -2.0; int bi = PT_NO_CAND;
    for (int c = tid; c < wx * wy; c += 256) {
        const int cy = c / wx, cx = c % wx, j = y0 + cy, i = x0 + cx;
        double cc = 0.0;
        if (i >= PT_MATCH_HALF && i <= W - PT_MATCH_HALF - 1 && j >= PT_MATCH_HALF && j <= H - PT_MATCH_HALF - 1) {
            const double ex = i - px, ey = j - py;
            if (patch_gate_dist(g, ex, ey) < chi2) {
                const unsigned char* roi = rg + cy * AR_RG_STRIDE + cx;        // image(j - 8 .., i - 8 ..)
                int sv = 0, svv = 0, svt = 0;                                  // <= PT_TMPL_BYTES * 255^2 < 2^31
                for (int r = 0; r < PT_TMPL_W; r++) {
#pragma unroll
                    for (int cl = 0; cl < PT_TMPL_W; cl++) {
                        const int v = roi[r * AR_RG_STRIDE + cl];
                        sv += v; svv += v * v; svt += v * tm[r * PT_TMPL_W + cl];
                    }
                }
                const long long A = (long long)PT_TMPL_BYTES * svt - (long long)sv * St;
                const long long B = (long long)PT_TMPL_BYTES * svv - (long long)sv * sv;
                cc = (B == 0 || C == 0) ? 0.0 : (double)A / sqrt((double)B * (double)C);
            }
        }
        if (cc > bv) { bv = cc; bi = c; }                      // a thread's candidates come in increasing index: its first maximum
    }
    block_first_max(bv, bi, bestv, besti);
    if (tid == 0) {
        const double mx = bestv[0];
        const int c = besti[0];
        *corr = mx;
        if (mx > thr) { z[0] = (double)(x0 + c % wx); z[1] = (double)(y0 + c / wx); *matched = 1; }
        else { z[0] = 0.0; z[1] = 0.0; *matched = 0; }
    }
}

__global__ __launch_bounds__(256) void k_archive_search(srukf_params p, int cap, double thr, double chi2, const unsigned char* __restrict__ image,
                                                        const double* __restrict__ h, const double* __restrict__ Si, const int* __restrict__ vis,
                                                        const unsigned char* __restrict__ tmpl, int tmpl_stride, double* __restrict__ z, int* __restrict__ matched,
                                                        double* __restrict__ corr)
{
    const int k = blockIdx.x;
    if (!vis[k]) { if (threadIdx.x == 0) { matched[k] = 0; corr[k] = 0.0; z[2 * k] = 0.0; z[2 * k + 1] = 0.0; } return; }
    archive_search_body(k, p, cap, thr, chi2, image, h, Si, tmpl, tmpl_stride, z + 2 * k, matched + k, corr + k);
}

// ---- the search behind every frame of an image run (srukf_images_search_archive) ----
// The frame tail has advanced fs->frame by the time these run: the frame that was just updated is fs->frame - 1.  A frame outside the staged stack writes nothing
// outside the archive's own scratch.

// in front of a frame's search: the posterior pose into rob (k_block_cov has left P4 behind it), the templates zeroed (a template depends on this search's inputs
// only), the frame's hit counter zeroed
__global__ __launch_bounds__(256) void k_archive_frame_begin(int n, const double* __restrict__ X, double* __restrict__ rob, unsigned long long* __restrict__ tmpl8, int words,
                                                             StagedArchive a)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < words) tmpl8[g] = 0ull;
    if (g < 4) rob[g] = X[n - 4 + g];
    const int f = a.fs->frame - 1;
    if (g == 0 && f >= 0 && f < a.frames) a.hits[f] = 0;
}

// k_archive_search on frame fs->frame - 1 of the staged stack, with half cap, threshold and chi2 read from a.args (written in stream order in front of the run: a captured
// frame holds the pointer, not the values); the frame's h, Si, visible and the result go into its row of the record, its matches are counted in hits
__global__ __launch_bounds__(256) void k_archive_search_staged(srukf_params p, StagedArchive a, const double* __restrict__ h, const double* __restrict__ Si,
                                                               const int* __restrict__ vis, const unsigned char* __restrict__ tmpl, int tmpl_stride)
{
    const int k = blockIdx.x, L = gridDim.x, tid = threadIdx.x;
    const int f = a.fs->frame - 1;
    if (f < 0 || f >= a.frames) return;
    const ArchiveArgs ar = *a.args;
    const size_t r1 = (size_t)f * L + k;
    const int v = vis[k];
    if (tid == 0) {
        a.vis_seq[r1] = v; a.h_seq[2 * r1] = h[2 * k]; a.h_seq[2 * r1 + 1] = h[2 * k + 1];
        for (int e = 0; e < 4; e++) a.Si_seq[4 * r1 + e] = Si[4 * k + e];
    }
    if (!v) { if (tid == 0) { a.m_seq[r1] = 0; a.corr_seq[r1] = 0.0; a.z_seq[2 * r1] = 0.0; a.z_seq[2 * r1 + 1] = 0.0; } return; }
    const unsigned char* image = a.images + (size_t)f * (size_t)((int)p.image_w * (int)p.image_h);
    archive_search_body(k, p, ar.half_cap, ar.corr_threshold, ar.chi2, image, h, Si, tmpl, tmpl_stride, a.z_seq + 2 * r1, a.m_seq + r1, a.corr_seq + r1);
    if (tid == 0 && a.m_seq[r1]) atomicAdd(a.hits + f, 1);
}

__global__ void k_set_archive_args(ArchiveArgs* dst, ArchiveArgs v) { *dst = v; }

void launch_archive_search_staged(hipStream_t st, int L, srukf_params p, StagedArchive a, const double* h, const double* Si, const int* vis, const unsigned char* tmpl)
{
    hipLaunchKernelGGL(k_archive_search_staged, dim3(L), dim3(256), 0, st, p, a, h, Si, vis, tmpl, PT_TMPL_STRIDE);
}
void launch_set_archive_args(hipStream_t st, ArchiveArgs* dst, ArchiveArgs v) { hipLaunchKernelGGL(k_set_archive_args, dim3(1), dim3(1), 0, st, dst, v); }

namespace srukf_impl {

void archive_free(ArchiveState& a, hipStream_t st)
{
    void* bufs[] = { a.X6, a.S66, a.R, a.t, a.px, a.patch, a.tmpl, a.rob, a.out };
    for (void* b : bufs) if (b) srukf_dfree_on(b, st);
    if (a.hst) hipHostFree(a.hst);
    a = ArchiveState{};
}

}  // namespace srukf_impl

// out (device) and hst (pinned) share one layout, in doubles: h 2L | Si 4L | z 2L | corr L | xyz 3L | visible L ints | matched L ints
static size_t ar_out_doubles(int L) { return 12 * (size_t)L + ((size_t)L + 1) / 2 * 2; }
struct ArOut { double *h, *Si, *z, *corr, *xyz; int *vis, *m; };
static ArOut ar_out(const ArchiveState& a)
{
    const size_t L = (size_t)a.L;
    ArOut o;
    o.h = a.out; o.Si = o.h + 2 * L; o.z = o.Si + 4 * L; o.corr = o.z + 2 * L; o.xyz = o.corr + L;
    o.vis = (int*)(o.xyz + 3 * L); o.m = o.vis + L;
    return o;
}
static double ar_search_bytes(int half_cap, int L)
{
    const double side = 2.0 * half_cap + 1.0 + 2.0 * PT_MATCH_HALF;
    return (side * side + PT_TMPL_BYTES) * L;
}

// stages (a) and (b) of a search over the archive's arrays, for the pose | P4 that stand in a.rob (the templates are zeroed): what srukf_archive_search and the
// searching frames of an image run both launch
static void archive_predict_warp(srukf_ctx* c)
{
    ArchiveState& a = c->archive;
    const int L = a.L;
    const ArOut o = ar_out(a);
    KWeights w; host_weights(AR_NA, c->p, w);
    {
        ProfScope ps(c, KC_ARCHIVE_PREDICT, 0, 8.0 * 62 * L);
        hipLaunchKernelGGL(k_archive_predict, dim3(L), dim3(64), 0, c->stream, c->p, w, a.X6, a.S66, a.rob, o.h, o.Si, o.vis, o.xyz);
    }
    KDims ad = {}; ad.N = L; ad.n = 4;                                                                  // k_warp_patch reads d.N and X[n - 4 .. n - 1]: the archive's pose
    {
        ProfScope ps(c, KC_ARCHIVE_WARP, 0, (double)(PT_PATCH_BYTES + PT_TMPL_BYTES) * L);
        srukf_launch_warp_patch(c->stream, ad, c->p, a.rob, o.xyz, o.h, a.R, a.t, a.px, a.patch, o.vis, a.tmpl);
    }
}

// srukf_archive_search's parameter rules (ap null: its defaults), for the step-wise call and the switch of the image runs
static int archive_params(srukf_ctx* c, const srukf_archive_params* ap, srukf_archive_params* out)
{
    srukf_archive_params prm = { AR_CAP_MAX, 0.8, 5.99146454710798 };                                   // THRESHOLD_MATCH_PATCH, the gate of dataAssociation (1977)
    if (ap) prm = *ap;
    if (prm.half_cap < 10 || prm.half_cap > AR_CAP_MAX) { c->err = "archive_search: half_cap outside [10, 40]"; return SRUKF_ERR_BAD_ARG; }
    if (!(prm.chi2 > 0.0) || !std::isfinite(prm.chi2) || !std::isfinite(prm.corr_threshold)) { c->err = "archive_search: chi2 / corr_threshold"; return SRUKF_ERR_BAD_ARG; }
    *out = prm;
    return SRUKF_OK;
}

namespace srukf_impl {

// The search behind a frame of a searching image run (replay_one_image_frame, behind seq_refactor: the posterior).  P4 by the launch srukf_get_robot makes, straight
// into rob's P4 slots; the pose, the zeroed templates and the zeroed hit counter by k_archive_frame_begin; then the step-wise call's two launches and the staged search.
// Every launch on the filter's stream; images_archive_ensure has run (never inside a capture)
void seq_archive_search(srukf_ctx* c)
{
    ArchiveState& a = c->archive;
    const ImageReplay& im = c->img;
    const int L = a.L;
    const ArOut o = ar_out(a);
    const ImageArchiveRecord r = image_archive_record(im.frames, L);
    double* rec = im.ar_rec; int* reci = (int*)(rec + r.ints);
    const StagedArchive sa = { im.images, im.frames, rec + r.h, rec + r.Si, rec + r.z, rec + r.corr, reci + r.vis_i, reci + r.m_i, reci + r.hits_i, c->fs, im.ar_args };
    {
        ProfScope ps(c, KC_ARCHIVE_PREDICT, 0, 8.0 * (20 + (double)L * PT_TMPL_STRIDE / 8));
        srukf_launch_block_cov(c->stream, c->d, c->S, c->d.n - 4, 4, a.rob + 4, nullptr);
        const int words = L * (PT_TMPL_STRIDE / 8);
        hipLaunchKernelGGL(k_archive_frame_begin, dim3((words + 255) / 256), dim3(256), 0, c->stream, c->d.n, c->X, a.rob, (unsigned long long*)a.tmpl, words, sa);
    }
    archive_predict_warp(c);
    {
        ProfScope ps(c, KC_ARCHIVE_SEARCH, 0, ar_search_bytes(c->img_search_args.half_cap, L));
        launch_archive_search_staged(c->stream, L, c->p, sa, o.h, o.Si, o.vis, a.tmpl);
    }
}

}  // namespace srukf_impl

extern "C" {

int srukf_archive_set(srukf_ctx* c, int L, const double* X6, const double* S66, const unsigned char* patches, const double* R, const double* t, const double* px)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (L < 0) { c->err = "archive_set: L < 0"; return SRUKF_ERR_BAD_ARG; }
    if (L > 0) {
        if (!X6 || !S66 || !patches || !R || !t || !px) { c->err = "archive_set: a NULL array"; return SRUKF_ERR_BAD_ARG; }
        auto finite = [](const double* a, size_t m) { for (size_t i = 0; i < m; i++) if (!std::isfinite(a[i])) return false; return true; };
        if (!finite(X6, 6 * (size_t)L) || !finite(S66, 36 * (size_t)L) || !finite(R, 9 * (size_t)L) || !finite(t, 3 * (size_t)L) || !finite(px, 2 * (size_t)L)) {
            c->err = "archive_set: an input is not finite"; return SRUKF_ERR_BAD_ARG;
        }
        for (int j = 0; j < L; j++)
            for (int a = 1; a < 6; a++)
                for (int b = 0; b < a; b++)
                    if (S66[36 * (size_t)j + 6 * a + b] != 0.0) { c->err = "archive_set: S66 is not upper triangular"; return SRUKF_ERR_BAD_ARG; }
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    images_archive_drop(c, c->stream);                           // (the record of the searching image runs and their captured frames are sized by L and hold these pointers)
    archive_free(c->archive, c->stream);
    if (L == 0) return SRUKF_OK;
    ArchiveState& a = c->archive;
    const size_t ps = PT_PATCH_STRIDE, ts = PT_TMPL_STRIDE, n = (size_t)L, od = ar_out_doubles(L);
    hipError_t e = srukf_dmalloc_on(&a.X6, sizeof(double) * 6 * n, c->stream);
    if (e == hipSuccess) e = srukf_dmalloc_on(&a.S66, sizeof(double) * 36 * n, c->stream);
    if (e == hipSuccess) e = srukf_dmalloc_on(&a.R, sizeof(double) * 9 * n, c->stream);
    if (e == hipSuccess) e = srukf_dmalloc_on(&a.t, sizeof(double) * 3 * n, c->stream);
    if (e == hipSuccess) e = srukf_dmalloc_on(&a.px, sizeof(double) * 2 * n, c->stream);
    if (e == hipSuccess) e = srukf_dmalloc_on(&a.patch, ps * n, c->stream);
    if (e == hipSuccess) e = srukf_dmalloc_on(&a.tmpl, ts * n, c->stream);
    if (e == hipSuccess) e = srukf_dmalloc_on(&a.rob, sizeof(double) * 20, c->stream);
    if (e == hipSuccess) e = srukf_dmalloc_on(&a.out, sizeof(double) * od, c->stream);
    if (e == hipSuccess) e = hipHostMalloc((void**)&a.hst, sizeof(double) * (od + 20));
    if (e != hipSuccess) { (void)hipGetLastError(); archive_free(a, c->stream); c->err = "archive_set: out of memory"; return SRUKF_ERR_NOMEM; }
    e = hipMemcpyAsync(a.X6, X6, sizeof(double) * 6 * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.S66, S66, sizeof(double) * 36 * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.R, R, sizeof(double) * 9 * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.t, t, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(a.px, px, sizeof(double) * 2 * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.patch, 0, ps * n, c->stream);
    if (e == hipSuccess) e = hipMemcpy2DAsync(a.patch, ps, patches, PT_PATCH_BYTES, PT_PATCH_BYTES, n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.tmpl, 0, ts * n, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);         // (pageable host memory)
    if (e != hipSuccess) { archive_free(a, c->stream); c->err = std::string("archive_set: ") + hipGetErrorString(e); return SRUKF_ERR_HIP; }
    a.L = L;
    return SRUKF_OK;
}

int srukf_archive_count(srukf_ctx* c) { return c ? c->archive.L : SRUKF_ERR_BAD_ARG; }

int srukf_archive_get_template(srukf_ctx* c, int j, unsigned char out[PT_TMPL_BYTES])
{
    if (!c || !out || j < 0 || j >= c->archive.L) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->archive.tmpl + (size_t)j * PT_TMPL_STRIDE, PT_TMPL_BYTES, hipMemcpyDeviceToHost));
    return SRUKF_OK;
}

int srukf_archive_search(srukf_ctx* c, const unsigned char* gray, const srukf_archive_params* ap, double* h, double* Si, int* visible, double* z, int* matched,
                         double* corr)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    srukf_archive_params prm;
    int rc = archive_params(c, ap, &prm); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = take_frame(c, gray); if (rc) return rc;
    ArchiveState& a = c->archive;
    const int L = a.L;
    if (L == 0) { if (gray) HIPCHK(c, hipStreamSynchronize(c->stream)); return SRUKF_OK; }
    const size_t od = ar_out_doubles(L);
    double* hrob = a.hst + od;
    rc = srukf_get_robot(c, hrob, hrob + 4); if (rc) return rc;                                         // pose | P4, exactly as the caller would get them now
    HIPCHK(c, hipMemcpyAsync(a.rob, hrob, sizeof(double) * 20, hipMemcpyHostToDevice, c->stream));
    const ArOut o = ar_out(a);
    HIPCHK(c, hipMemsetAsync(a.tmpl, 0, (size_t)L * PT_TMPL_STRIDE, c->stream));  // a template depends on this call's inputs only
    archive_predict_warp(c);
    {
        ProfScope ps(c, KC_ARCHIVE_SEARCH, 0, ar_search_bytes(prm.half_cap, L));
        hipLaunchKernelGGL(k_archive_search, dim3(L), dim3(256), 0, c->stream, c->p, prm.half_cap, prm.corr_threshold, prm.chi2, c->d_image, o.h, o.Si, o.vis, a.tmpl,
                           PT_TMPL_STRIDE, o.z, o.m, o.corr);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(a.hst, a.out, sizeof(double) * od, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double* hs = a.hst;
    const int* hi = (const int*)(hs + 12 * (size_t)L);
    if (h) memcpy(h, hs, sizeof(double) * 2 * L);
    if (Si) memcpy(Si, hs + 2 * (size_t)L, sizeof(double) * 4 * L);
    if (z) memcpy(z, hs + 6 * (size_t)L, sizeof(double) * 2 * L);
    if (corr) memcpy(corr, hs + 8 * (size_t)L, sizeof(double) * L);
    if (visible) memcpy(visible, hi, sizeof(int) * L);
    if (matched) memcpy(matched, hi + L, sizeof(int) * L);
    return SRUKF_OK;
}

// The switch of the image runs: on the handle, like the archive; the parameters are srukf_archive_search's, checked by its rules.  Touches no
// device: the values reach it in stream order in front of the next searching run (run_images_issue)
int srukf_images_search_archive(srukf_ctx* c, int on, const srukf_archive_params* ap)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    srukf_archive_params prm = { AR_CAP_MAX, 0.8, 5.99146454710798 };
    if (on) { const int rc = archive_params(c, ap, &prm); if (rc) return rc; }
    if (c->async_pending && c->img.pending) { c->err = "images_search_archive: an image run is in flight (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    c->img_search = on != 0;
    c->img_search_args = ArchiveArgs{ prm.half_cap, prm.corr_threshold, prm.chi2 };
    return SRUKF_OK;
}

}  // extern "C"
