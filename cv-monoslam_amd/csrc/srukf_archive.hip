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
__global__ __launch_bounds__(256) void k_archive_search(srukf_params p, int cap, double thr, double chi2, const unsigned char* __restrict__ image,
                                                        const double* __restrict__ h, const double* __restrict__ Si, const int* __restrict__ vis,
                                                        const unsigned char* __restrict__ tmpl, int tmpl_stride, double* __restrict__ z, int* __restrict__ matched,
                                                        double* __restrict__ corr)
{
    __shared__ unsigned char rg[AR_RG_W * AR_RG_STRIDE];
    __shared__ int tm[PT_TMPL_BYTES];
    __shared__ int tsum[2];
    __shared__ double bestv[256];
    __shared__ int besti[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int W = (int)p.image_w, H = (int)p.image_h;
    if (!vis[k]) { if (tid == 0) { matched[k] = 0; corr[k] = 0.0; z[2 * k] = 0.0; z[2 * k + 1] = 0.0; } return; }
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
        corr[k] = mx;
        if (mx > thr) { z[2 * k] = (double)(x0 + c % wx); z[2 * k + 1] = (double)(y0 + c / wx); matched[k] = 1; }
        else { z[2 * k] = 0.0; z[2 * k + 1] = 0.0; matched[k] = 0; }
    }
}

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
    srukf_archive_params prm = { AR_CAP_MAX, 0.8, 5.99146454710798 };                                   // THRESHOLD_MATCH_PATCH, the gate of dataAssociation (1977)
    if (ap) prm = *ap;
    if (prm.half_cap < 10 || prm.half_cap > AR_CAP_MAX) { c->err = "archive_search: half_cap outside [10, 40]"; return SRUKF_ERR_BAD_ARG; }
    if (!(prm.chi2 > 0.0) || !std::isfinite(prm.chi2) || !std::isfinite(prm.corr_threshold)) { c->err = "archive_search: chi2 / corr_threshold"; return SRUKF_ERR_BAD_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = take_frame(c, gray); if (rc) return rc;
    ArchiveState& a = c->archive;
    const int L = a.L;
    if (L == 0) { if (gray) HIPCHK(c, hipStreamSynchronize(c->stream)); return SRUKF_OK; }
    const size_t od = ar_out_doubles(L);
    double* hrob = a.hst + od;
    rc = srukf_get_robot(c, hrob, hrob + 4); if (rc) return rc;                                         // pose | P4, exactly as the caller would get them now
    HIPCHK(c, hipMemcpyAsync(a.rob, hrob, sizeof(double) * 20, hipMemcpyHostToDevice, c->stream));
    double* dh = a.out; double* dSi = dh + 2 * (size_t)L; double* dz = dSi + 4 * (size_t)L; double* dcorr = dz + 2 * (size_t)L; double* dxyz = dcorr + L;
    int* dvis = (int*)(dxyz + 3 * (size_t)L); int* dm = dvis + L;
    HIPCHK(c, hipMemsetAsync(a.tmpl, 0, (size_t)L * PT_TMPL_STRIDE, c->stream));  // a template depends on this call's inputs only
    KWeights w; host_weights(AR_NA, c->p, w);
    {
        ProfScope ps(c, KC_ARCHIVE_PREDICT, 0, 8.0 * 62 * L);
        hipLaunchKernelGGL(k_archive_predict, dim3(L), dim3(64), 0, c->stream, c->p, w, a.X6, a.S66, a.rob, dh, dSi, dvis, dxyz);
    }
    KDims ad = {}; ad.N = L; ad.n = 4;                                                                  // k_warp_patch reads d.N and X[n - 4 .. n - 1]: the archive's pose
    {
        ProfScope ps(c, KC_ARCHIVE_WARP, 0, (double)(PT_PATCH_BYTES + PT_TMPL_BYTES) * L);
        srukf_launch_warp_patch(c->stream, ad, c->p, a.rob, dxyz, dh, a.R, a.t, a.px, a.patch, dvis, a.tmpl);
    }
    {
        const double side = 2.0 * prm.half_cap + 1.0;
        ProfScope ps(c, KC_ARCHIVE_SEARCH, 0, ((side + 2.0 * PT_MATCH_HALF) * (side + 2.0 * PT_MATCH_HALF) + PT_TMPL_BYTES) * L);
        hipLaunchKernelGGL(k_archive_search, dim3(L), dim3(256), 0, c->stream, c->p, prm.half_cap, prm.corr_threshold, prm.chi2, c->d_image, dh, dSi, dvis, a.tmpl,
                           PT_TMPL_STRIDE, dz, dm, dcorr);
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

}  // extern "C"
