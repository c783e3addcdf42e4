// srukf_unique.hip — data association that keeps the score map: dataAssociation (SLAM.cpp:1915-2009) as k_associate runs it, plus a
// uniqueness test on the second peak and a sub-pixel refinement of the first.  gfx950 only.
//
// k_associate (srukf_assoc.hip) keeps the first maximum of the normalised cross correlation inside the chi-square gate and nothing else.  Two things a patch
// tracker is expected to do need the whole surface: (1) on repetitive texture (ceiling tiles, lamps, grilles: periods of a few pixels, inside the +-8..10 px
// window) a second peak as good as the first is not an outlier, and the first in raster order is an arbitrary choice — such a match is reported as ambiguous
// and not used; (2) the reference's matchLocation is the integer candidate centre plus the FRACTION OF THE PREDICTION (1991-1992), a pull of up to one pixel
// towards where the filter already believes the landmark is — the parabola through the peak's 4-neighbours locates it to a fraction of a pixel instead.
//
// k_associate_checked runs the matching front k_associate runs (srukf_patch.h, match_front: template statistics, window, border test, gate and candidate score —
// one text, so the two kernels' scores are the same bits; the GPU tests hold them together all the same), keeps every candidate's score in LDS and in a device
// buffer (PT_SCORE_STRIDE doubles per landmark: the map row-major, then wx, wy, x0, y0), and then decides:
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
// k_associate_checked_staged is the same kernel for a frame of an image run (srukf_run_images_checked*): the staged addressing of k_associate_staged,
// the parameters read from the device.  The decisions exist once: match_decide.
#include "srukf_device.h"
#include "srukf_launch.h"
#include "srukf_patch.h"

// ---- what the map is kept for: the rules above on a complete score map (smap: LDS, row-major over the window; bestv[0] / besti[0]: match_front's first maximum).
// One text for k_associate_checked and k_associate_checked_staged, which differ only in where the results are stored.  Every thread of the 256 calls it (it reduces
// over the block); the decision it returns is thread 0's to store: maxVal and corr2 are valid for every thread, the rest for thread 0 only
struct MatchDecision { double maxVal, zx, zy, z2x, z2y, corr2; int flags, ok; };
__device__ __forceinline__ MatchDecision match_decide(const MatchWindow& w, const MatchArgs& ma, const double* smap, double* bestv, int* besti)
{
    const int tid = threadIdx.x;
    const int wx = w.wx, wy = w.wy, x0 = w.x0, y0 = w.y0, half_x = w.half_x, half_y = w.half_y;
    const double px = w.px, py = w.py;
    const double maxVal = bestv[0];
    const int b = besti[0];
    const bool raw = maxVal > ma.corr_threshold;                // the same for every thread
    const int bx = b % wx, by = b / wx;
    __syncthreads();                                            // bestv / besti are used again
    double corr2 = 0.0; int rv = PT_NO_CAND;
    if (raw) {
        double v2 = 0.0; int r2 = PT_NO_CAND;
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
        corr2 = rv == PT_NO_CAND ? 0.0 : bestv[0];
    }
    MatchDecision dec = { maxVal, 0.0, 0.0, 0.0, 0.0, corr2, 0, 0 };
    if (tid != 0) return dec;
    int flags = 0, ok = 0;
    double zx = 0.0, zy = 0.0, z2x = 0.0, z2y = 0.0;
    if (raw) {                                                                                          // 1989
        flags = 1;
        if (rv != PT_NO_CAND) { z2x = (rv % wx) - half_x + px; z2y = (rv / wx) - half_y + py; }         // 1991-1992
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
    dec.zx = zx; dec.zy = zy; dec.z2x = z2x; dec.z2y = z2y; dec.flags = flags; dec.ok = ok;
    return dec;
}

// res: the packed result block the host exports in one piece (match_res, srukf_patch.h); scores: the score buffer (PT_SCORE_*)
// z / matched / corr: the filter's own buffers, left as k_associate leaves them
__global__ __launch_bounds__(256) void k_associate_checked(KDims d, srukf_params p, MatchArgs ma, const unsigned char* __restrict__ image,
                                                           const double* __restrict__ h, const double* __restrict__ Si, const int* __restrict__ vis,
                                                           const int* __restrict__ has_app, const unsigned char* __restrict__ matchPatch,
                                                           double* __restrict__ z, int* __restrict__ matched, double* __restrict__ corr,
                                                           double* __restrict__ res, double* __restrict__ scores)
{
    __shared__ double tm[PT_TMPL_BYTES];
    __shared__ double red[8];
    __shared__ double bestv[256];
    __shared__ int besti[256];
    __shared__ double rg[PT_REGION_W * PT_REGION_W];
    __shared__ double smap[PT_SCORE_W * PT_SCORE_W];
    const int k = blockIdx.x, tid = threadIdx.x, N = d.N;
    const MatchRes at = match_res(N);
    double* rz = res + at.z; double* rcorr = res + at.corr; double* rcorr2 = res + at.corr2; double* rz2 = res + at.z2;
    int* rmatched = (int*)(res + at.matched); int* rflags = rmatched + at.flags_ints;
    double* sc = scores + (size_t)k * PT_SCORE_STRIDE;
    if (!vis[k] || !has_app[k]) {                                                                       // 1946
        if (tid == 0) {
            matched[k] = 0; corr[k] = 0.0; z[2 * k] = 0.0; z[2 * k + 1] = 0.0;
            rz[2 * k] = 0.0; rz[2 * k + 1] = 0.0; rcorr[k] = 0.0; rcorr2[k] = 0.0; rz2[2 * k] = 0.0; rz2[2 * k + 1] = 0.0; rmatched[k] = 0; rflags[k] = 0;
            sc[PT_SCORE_WX] = 0.0; sc[PT_SCORE_WY] = 0.0; sc[PT_SCORE_X0] = 0.0; sc[PT_SCORE_Y0] = 0.0;
        }
        return;
    }
    // k_associate's front, every score kept (c < PT_SCORE_W^2: inside both); the barriers of its reduction also complete smap
    const MatchWindow w = match_front(k, p, image, h, Si, matchPatch, tm, red, rg, bestv, besti, [&](int c, double cc) { smap[c] = sc[c] = cc; });
    const MatchDecision dec = match_decide(w, ma, smap, bestv, besti);
    if (tid != 0) return;
    corr[k] = dec.maxVal; z[2 * k] = dec.zx; z[2 * k + 1] = dec.zy; matched[k] = dec.ok;
    rz[2 * k] = dec.zx; rz[2 * k + 1] = dec.zy; rcorr[k] = dec.maxVal; rcorr2[k] = dec.corr2; rz2[2 * k] = dec.z2x; rz2[2 * k + 1] = dec.z2y;
    rmatched[k] = dec.ok; rflags[k] = dec.flags;
    sc[PT_SCORE_WX] = (double)w.wx; sc[PT_SCORE_WY] = (double)w.wy; sc[PT_SCORE_X0] = (double)w.x0; sc[PT_SCORE_Y0] = (double)w.y0;
}

// k_associate_checked_staged: k_associate_checked for a frame of an image run (srukf_run_images_checked*).  The frame is image fs->frame of the
// staged stack; z / matched go into that frame's rows of z_seq / m_seq, where k_gain and the joint kernels read them, corr / visible / the predicted pixels into the
// record as k_associate_staged writes them, corr2 / z2 / flags into the checked record beside it, the score map into the filter's score buffer (one map per landmark:
// after a run, the last frame's).  The parameters are read from a.ma, written in stream order in front of the run (launch_set_match_args): a captured frame holds the
// pointer, not the values.  The same front and the same decisions as k_associate_checked; every dependency is a launch boundary on the stream.  A frame counter
// outside the staged stack writes nothing.
__global__ __launch_bounds__(256) void k_associate_checked_staged(KDims d, srukf_params p, StagedChecked a, const double* __restrict__ h, const double* __restrict__ Si,
                                                                  const int* __restrict__ vis, const int* __restrict__ has_app, const unsigned char* __restrict__ matchPatch)
{
    __shared__ double tm[PT_TMPL_BYTES];
    __shared__ double red[8];
    __shared__ double bestv[256];
    __shared__ int besti[256];
    __shared__ double rg[PT_REGION_W * PT_REGION_W];
    __shared__ double smap[PT_SCORE_W * PT_SCORE_W];
    const int k = blockIdx.x, tid = threadIdx.x, N = d.N;
    const int f = a.rec.fs->frame;
    if (f < 0 || f >= a.rec.frames) return;
    const MatchArgs ma = *a.ma;
    const size_t r1 = (size_t)f * N + k, r2 = (size_t)f * 2 * N + 2 * k;      // this landmark's slot in a [F][N] / [F][2N] array
    double* sc = a.scores + (size_t)k * PT_SCORE_STRIDE;
    const int v = vis[k];
    if (tid == 0) { a.rec.vis_seq[r1] = v; a.rec.h_seq[r2] = h[2 * k]; a.rec.h_seq[r2 + 1] = h[2 * k + 1]; }
    if (!v || !has_app[k]) {                                                                            // 1946
        if (tid == 0) {
            a.rec.m_seq[r1] = 0; a.rec.corr_seq[r1] = 0.0; a.rec.z_seq[r2] = 0.0; a.rec.z_seq[r2 + 1] = 0.0;
            a.corr2_seq[r1] = 0.0; a.z2_seq[r2] = 0.0; a.z2_seq[r2 + 1] = 0.0; a.flags_seq[r1] = 0;
            sc[PT_SCORE_WX] = 0.0; sc[PT_SCORE_WY] = 0.0; sc[PT_SCORE_X0] = 0.0; sc[PT_SCORE_Y0] = 0.0;
        }
        return;
    }
    const unsigned char* image = a.rec.images + (size_t)f * (size_t)((int)p.image_w * (int)p.image_h);
    const MatchWindow w = match_front(k, p, image, h, Si, matchPatch, tm, red, rg, bestv, besti, [&](int c, double cc) { smap[c] = sc[c] = cc; });
    const MatchDecision dec = match_decide(w, ma, smap, bestv, besti);
    if (tid != 0) return;
    a.rec.corr_seq[r1] = dec.maxVal; a.rec.z_seq[r2] = dec.zx; a.rec.z_seq[r2 + 1] = dec.zy; a.rec.m_seq[r1] = dec.ok;
    a.corr2_seq[r1] = dec.corr2; a.z2_seq[r2] = dec.z2x; a.z2_seq[r2 + 1] = dec.z2y; a.flags_seq[r1] = dec.flags;
    sc[PT_SCORE_WX] = (double)w.wx; sc[PT_SCORE_WY] = (double)w.wy; sc[PT_SCORE_X0] = (double)w.x0; sc[PT_SCORE_Y0] = (double)w.y0;
}

// the parameters of the checked image frames that follow on the stream
__global__ void k_set_match_args(MatchArgs* dst, MatchArgs v) { *dst = v; }

extern "C" {
void srukf_launch_associate_checked(hipStream_t st, KDims d, srukf_params p, MatchArgs ma, const unsigned char* image, const double* h, const double* Si, const int* vis,
                                    const int* has_app, const unsigned char* matchPatch, double* z, int* matched, double* corr, double* res, double* scores)
{
    hipLaunchKernelGGL(k_associate_checked, dim3(d.N), dim3(256), 0, st, d, p, ma, image, h, Si, vis, has_app, matchPatch, z, matched, corr, res, scores);
}
void srukf_launch_associate_checked_staged(hipStream_t st, KDims d, srukf_params p, StagedChecked a, const double* h, const double* Si, const int* vis, const int* has_app,
                                           const unsigned char* matchPatch)
{
    hipLaunchKernelGGL(k_associate_checked_staged, dim3(d.N), dim3(256), 0, st, d, p, a, h, Si, vis, has_app, matchPatch);
}
void srukf_launch_set_match_args(hipStream_t st, MatchArgs* dst, MatchArgs v)
{
    hipLaunchKernelGGL(k_set_match_args, dim3(1), dim3(1), 0, st, dst, v);
}
}  // extern "C"
