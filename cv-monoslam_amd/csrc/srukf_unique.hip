// srukf_unique.hip — data association that keeps the score map: dataAssociation (SLAM.cpp:1915-2009) as k_associate runs it, plus a
// uniqueness test on the second peak and a sub-pixel refinement of the first.  gfx950 only.
//
// k_associate (srukf_assoc.hip) keeps the first maximum of the normalised cross correlation inside the chi-square gate and nothing else.  Two things a patch
// tracker is expected to do need the whole surface: (1) on repetitive texture (ceiling tiles, lamps, grilles: periods of a few pixels, inside the +-8..10 px
// window) a second peak as good as the first is not an outlier, and the first in raster order is an arbitrary choice — such a match is reported as ambiguous
// and not used; (2) the reference's matchLocation is the integer candidate centre plus the FRACTION OF THE PREDICTION (1991-1992), a pull of up to one pixel
// towards where the filter already believes the landmark is — the parabola through the peak's 4-neighbours locates it to a fraction of a pixel instead.
//
// k_associate_checked restates k_associate's template statistics, window, border test, gate and candidate score operation for operation (this file is compiled
// with -ffp-contract=off like srukf_assoc.hip; the GPU tests hold the two kernels together bit for bit), keeps every candidate's score in LDS and in a device
// buffer (448 doubles per landmark: the map row-major, then wx, wy, x0, y0), and then decides:
//   best   the first maximum in row-major order (start value -1, ties to the lower index); corr = s[best]; raw = corr > corr_threshold
//   rival  (only when raw) the largest s[c], first in row-major order among equals, over the candidates with Chebyshev distance > exclusion from best, s[c] > 0
//          and s[c] >= s[c'] for every c' of the window at Chebyshev distance 1 (neighbours outside the window do not exist, gated ones count with their 0);
//          corr2 = its score, z2 = its location by the reference's formula; both 0 without a rival
//   ambiguous = raw && corr2 >= ratio * corr;  matched = raw && !ambiguous;  flags = raw | ambiguous << 1 | refined << 2
//   z      the best's location whenever raw (also when vetoed), (0, 0) otherwise.  subpixel == 0: the reference's form (c % wx) - half_x + px.  subpixel != 0:
//          ((int)px - half_x + bx + dx, (int)py - half_y + by + dy) — the integer centre plus the parabola's offset, WITHOUT the reference's + frac(h): a
//          refinement on top of an arbitrary fractional offset means nothing.  dx = dy = 0 unless best is off the window's edge and its four 4-neighbours all
//          score > 0 (then bit 2 is set): den = (sL - 2 s0) + sR, dx = den < 0 ? (0.5 (sL - sR)) / den : 0, clamped to [-0.5, 0.5]; dy likewise from the
//          upper (y - 1) and lower neighbours
// One workgroup of 256 threads per landmark, static LDS only (~20 KB), no atomics, nothing between workgroups.
#include "srukf_device.h"
#include "srukf_launch.h"

#define HP_INIT 10             // SLAM.cpp:41-42
#define HP_MATCH 8             // SLAM.cpp:43-44
#define TMPL_W (2 * HP_MATCH + 1)
#define APP_TMPL_STRIDE 320    // bytes per landmark in the matchPatch array (srukf_assoc.hip; the host checks it against srukf_app_tmpl_stride)
#define SCORE_W (2 * HP_INIT + 1)
#define SCORE_STRIDE 448       // doubles per landmark in the score buffer: 441 scores | wx | wy | x0 | y0 | 3 unused
#define NO_CAND 0x7fffffff

struct MatchArgs { double corr_threshold, ratio; int exclusion, subpixel; };

// the block's maximum of (bv, bi), ties to the lower index: k_associate's reduction.  Result in bestv[0] / besti[0], valid for every thread after the call
__device__ __forceinline__ void block_first_max(double bv, int bi, double* bestv, int* besti)
{
    const int tid = threadIdx.x;
    bestv[tid] = bv; besti[tid] = bi;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) {
            const double ov = bestv[tid + st]; const int oi = besti[tid + st];
            if (ov > bestv[tid] || (ov == bestv[tid] && oi < besti[tid])) { bestv[tid] = ov; besti[tid] = oi; }
        }
        __syncthreads();
    }
}

// res (7 N doubles, what the host exports in one piece): z[2N] | corr[N] | corr2[N] | z2[2N] | matched[N ints] flags[N ints]
// z / matched / corr: the filter's own buffers, left as k_associate leaves them
__global__ __launch_bounds__(256) void k_associate_checked(KDims d, srukf_params p, MatchArgs ma, const unsigned char* __restrict__ image,
                                                           const double* __restrict__ h, const double* __restrict__ Si, const int* __restrict__ vis,
                                                           const int* __restrict__ has_app, const unsigned char* __restrict__ matchPatch,
                                                           double* __restrict__ z, int* __restrict__ matched, double* __restrict__ corr,
                                                           double* __restrict__ res, double* __restrict__ scores)
{
    __shared__ double tm[TMPL_W * TMPL_W];
    __shared__ double red[8];
    __shared__ double bestv[256];
    __shared__ int besti[256];
    __shared__ double smap[SCORE_W * SCORE_W];
    const int k = blockIdx.x, tid = threadIdx.x, N = d.N;
    const int W = p.image_w, H = p.image_h, NP = TMPL_W * TMPL_W;
    double* rz = res; double* rcorr = res + 2 * (size_t)N; double* rcorr2 = res + 3 * (size_t)N; double* rz2 = res + 4 * (size_t)N;
    int* rmatched = (int*)(res + 6 * (size_t)N); int* rflags = rmatched + N;
    double* sc = scores + (size_t)k * SCORE_STRIDE;
    if (!vis[k] || !has_app[k]) {                                                                       // 1946
        if (tid == 0) {
            matched[k] = 0; corr[k] = 0.0; z[2 * k] = 0.0; z[2 * k + 1] = 0.0;
            rz[2 * k] = 0.0; rz[2 * k + 1] = 0.0; rcorr[k] = 0.0; rcorr2[k] = 0.0; rz2[2 * k] = 0.0; rz2[2 * k + 1] = 0.0; rmatched[k] = 0; rflags[k] = 0;
            sc[441] = 0.0; sc[442] = 0.0; sc[443] = 0.0; sc[444] = 0.0;
        }
        return;
    }
    // ---- k_associate, restated (srukf_assoc.hip:201-249) ----
    // template statistics (calculateCrossCorrelation, 3151-3161): cv::mean, subtract, cv::norm
    const unsigned char* mp = matchPatch + (size_t)k * APP_TMPL_STRIDE;
    double s[1] = { 0.0 };
    for (int e = tid; e < NP; e += 256) s[0] += mp[e];
    block_sum<1>(s, red);
    const double a2 = s[0] / NP;
    double q[1] = { 0.0 };
    for (int e = tid; e < NP; e += 256) { const double v = mp[e] - a2; tm[e] = v; q[0] += v * v; }
    block_sum<1>(q, red);
    const double std2 = sqrt(q[0]);
    __syncthreads();
    const double px = h[2 * k], py = h[2 * k + 1];
    const double s00 = Si[4 * k], s01 = Si[4 * k + 1], s10 = Si[4 * k + 2], s11 = Si[4 * k + 3];
    const double p00 = s00 * s00 + s10 * s10, p01 = s00 * s01 + s10 * s11, p10 = s01 * s00 + s11 * s10, p11 = s01 * s01 + s11 * s11;   // Si^T Si, 1951
    double det = p00 * p11 - p01 * p10, i00 = 0, i01 = 0, i10 = 0, i11 = 0;                             // cv 2x2 closed-form inverse
    if (det != 0.0) { det = 1.0 / det; i00 = p11 * det; i01 = -p01 * det; i10 = -p10 * det; i11 = p00 * det; }
    int half_x = (int)ceil(2 * s00), half_y = (int)ceil(2 * s11);                                       // 1953-1954
    half_x = min(HP_INIT, max(HP_MATCH, half_x)); half_y = min(HP_INIT, max(HP_MATCH, half_y));         // 1955-1956
    const int wx = 2 * half_x + 1, wy = 2 * half_y + 1;
    const int x0 = (int)px - half_x, y0 = (int)py - half_y;
    // the pixels every candidate can touch, staged once as doubles; outside the image: 0 (such a candidate is skipped by the border test)
    constexpr int RG_W = 2 * HP_INIT + 1 + 2 * HP_MATCH;       // 37
    __shared__ double rg[RG_W * RG_W];
    const int rw = wx + 2 * HP_MATCH, rh = wy + 2 * HP_MATCH, rx0 = x0 - HP_MATCH, ry0 = y0 - HP_MATCH;
    for (int e = tid; e < rw * rh; e += 256) {
        const int yy = ry0 + e / rw, xx = rx0 + e % rw;
        rg[(e / rw) * RG_W + e % rw] = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? (double)image[(size_t)yy * W + xx] : 0.0;
    }
    __syncthreads();
    double bv = -1.0; int bi = NO_CAND;
    for (int c = tid; c < wx * wy; c += 256) {
        const int j = y0 + c / wx, i = x0 + c % wx;                                                     // row-major index of `correlation`
        double cc = 0.0;
        if (!(i < HP_MATCH || i > W - HP_MATCH - 1) && !(j < HP_MATCH || j > H - HP_MATCH - 1)) {       // 1962, 1969
            const double ex = i - px, ey = j - py;
            const double pii = (ex * i00 + ey * i10) * ex + (ex * i01 + ey * i11) * ey;                 // 1975
            if (pii < 5.99146454710798) {                                                               // 1977
                const double* roi = rg + (j - y0) * RG_W + (i - x0);                                    // 1979
                double s1 = 0.0;
                for (int r = 0; r < TMPL_W; r++) for (int cl = 0; cl < TMPL_W; cl++) s1 += roi[r * RG_W + cl];
                const double a1 = s1 / NP;
                double q1 = 0.0, dot = 0.0;
                for (int r = 0; r < TMPL_W; r++) for (int cl = 0; cl < TMPL_W; cl++) { const double v1 = roi[r * RG_W + cl] - a1; q1 += v1 * v1; dot += v1 * tm[r * TMPL_W + cl]; }
                const double std1 = sqrt(q1);
                cc = (std1 == 0.0 || std2 == 0.0) ? 0.0 : dot / std1 / std2;                            // 3163-3166
            }
        }
        smap[c] = cc; sc[c] = cc;                               // c < 441: inside both
        if (cc > bv) { bv = cc; bi = c; }                       // candidates of one thread come in increasing index: first maximum kept
    }
    block_first_max(bv, bi, bestv, besti);                      // (its barriers also complete smap)
    // ---- what the map is kept for ----
    const double maxVal = bestv[0];
    const int b = besti[0];
    const bool raw = maxVal > ma.corr_threshold;                // the same for every thread
    const int bx = b % wx, by = b / wx;
    __syncthreads();                                            // bestv / besti are used again
    double corr2 = 0.0; int rv = NO_CAND;
    if (raw) {
        double v2 = 0.0; int r2 = NO_CAND;
        for (int c = tid; c < wx * wy; c += 256) {
            const int cx = c % wx, cy = c / wx;
            const double v = smap[c];
            if (!(v > 0.0) || max(abs(cx - bx), abs(cy - by)) <= ma.exclusion) continue;
            bool top = true;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int nx = cx + dx, ny = cy + dy;
                    if ((dx == 0 && dy == 0) || nx < 0 || nx >= wx || ny < 0 || ny >= wy) continue;
                    if (smap[ny * wx + nx] > v) top = false;
                }
            if (top && v > v2) { v2 = v; r2 = c; }
        }
        block_first_max(v2, r2, bestv, besti);
        rv = besti[0];
        corr2 = rv == NO_CAND ? 0.0 : bestv[0];
    }
    if (tid != 0) return;
    int flags = 0, ok = 0;
    double zx = 0.0, zy = 0.0, z2x = 0.0, z2y = 0.0;
    if (raw) {                                                                                          // 1989
        flags = 1;
        if (rv != NO_CAND) { z2x = (rv % wx) - half_x + px; z2y = (rv / wx) - half_y + py; }            // 1991-1992
        const bool ambiguous = corr2 >= ma.ratio * maxVal;
        if (ambiguous) flags |= 2;
        ok = ambiguous ? 0 : 1;
        if (!ma.subpixel) {
            zx = (b % wx) - half_x + px;                                                                // 1991-1992
            zy = (b / wx) - half_y + py;
        } else {
            double dx = 0.0, dy = 0.0;
            if (0 < bx && bx < wx - 1 && 0 < by && by < wy - 1) {
                const double s0 = smap[b], sL = smap[b - 1], sR = smap[b + 1], sU = smap[b - wx], sD = smap[b + wx];
                if (sL > 0.0 && sR > 0.0 && sU > 0.0 && sD > 0.0) {
                    flags |= 4;
                    const double denx = (sL - 2.0 * s0) + sR, deny = (sU - 2.0 * s0) + sD;
                    dx = denx < 0.0 ? (0.5 * (sL - sR)) / denx : 0.0;
                    dy = deny < 0.0 ? (0.5 * (sU - sD)) / deny : 0.0;
                    dx = dx < -0.5 ? -0.5 : (dx > 0.5 ? 0.5 : dx);
                    dy = dy < -0.5 ? -0.5 : (dy > 0.5 ? 0.5 : dy);
                }
            }
            zx = (double)(x0 + bx) + dx;
            zy = (double)(y0 + by) + dy;
        }
    }
    corr[k] = maxVal; z[2 * k] = zx; z[2 * k + 1] = zy; matched[k] = ok;
    rz[2 * k] = zx; rz[2 * k + 1] = zy; rcorr[k] = maxVal; rcorr2[k] = corr2; rz2[2 * k] = z2x; rz2[2 * k + 1] = z2y; rmatched[k] = ok; rflags[k] = flags;
    sc[441] = (double)wx; sc[442] = (double)wy; sc[443] = (double)x0; sc[444] = (double)y0;
}

extern "C" {
void srukf_launch_associate_checked(hipStream_t st, KDims d, srukf_params p, double corr_threshold, double ratio, int exclusion, int subpixel,
                                    const unsigned char* image, const double* h, const double* Si, const int* vis, const int* has_app,
                                    const unsigned char* matchPatch, double* z, int* matched, double* corr, double* res, double* scores)
{
    MatchArgs ma; ma.corr_threshold = corr_threshold; ma.ratio = ratio; ma.exclusion = exclusion; ma.subpixel = subpixel;
    hipLaunchKernelGGL(k_associate_checked, dim3(d.N), dim3(256), 0, st, d, p, ma, image, h, Si, vis, has_app, matchPatch, z, matched, corr, res, scores);
}
int srukf_match_score_stride(void) { return SCORE_STRIDE; }
int srukf_match_tmpl_stride(void) { return APP_TMPL_STRIDE; }
}  // extern "C"
