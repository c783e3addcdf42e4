// srukf_patch.h — the appearance record's geometry and the front of the patch search, each ONCE: the sizes of initPatch / matchPatch and of the buffers built
// on them, the layout of the checked association's result block and score buffer (what a kernel writes and the host decodes), and the device pieces the three
// search kernels share.  gfx950 only.  Included by srukf_assoc, srukf_unique and srukf_archive for the device pieces and, through srukf_launch.h, by every
// file of the host layer (srukf_map, srukf_detect, srukf_loop); include/srukf.h states the same sizes as array lengths of the ABI (out[441], out[289]).
//
// One matching front (dataAssociation, SLAM.cpp:1946-1987, with calculateCrossCorrelation, 3141-3166), two consumers: k_associate (srukf_assoc.hip) keeps the
// first maximum, k_associate_checked (srukf_unique.hip) keeps every candidate's score too and decides on the whole map (each with a twin for the frames of an image run:
// k_associate_staged, k_associate_checked_staged).  match_front is that front; the two
// kernels differ in the hook it calls per candidate and in what they do with the first maximum.  k_archive_search (srukf_archive.hip) has a window rule, a
// score (exact integer sums) and a byte staging of its own and takes the gate, block_first_max and the constants only.
// Every arithmetic function below switches contraction off itself: the bits do not depend on the including file's compiler flags.
#pragma once
#include "srukf_device.h"

// ---- geometry of an appearance record ----
constexpr int PT_INIT_HALF = 10;                               // SLAM.cpp:41-42: half width of initPatch, and of the widest search window
constexpr int PT_MATCH_HALF = 8;                               // SLAM.cpp:43-44: half width of matchPatch (the template), and of the narrowest search window
constexpr int PT_PATCH_W = 2 * PT_INIT_HALF + 1;               // 21
constexpr int PT_TMPL_W = 2 * PT_MATCH_HALF + 1;               // 17
constexpr int PT_PATCH_BYTES = PT_PATCH_W * PT_PATCH_W;        // 441
constexpr int PT_TMPL_BYTES = PT_TMPL_W * PT_TMPL_W;           // 289
constexpr int PT_PATCH_STRIDE = 448;                           // bytes per landmark in an initPatch array
constexpr int PT_TMPL_STRIDE = 320;                            // bytes per landmark in a matchPatch array
constexpr int PT_SCORE_W = 2 * PT_INIT_HALF + 1;               // 21: the widest score window (1953-1956)
constexpr int PT_REGION_W = PT_SCORE_W + 2 * PT_MATCH_HALF;    // 37: side of the pixels every candidate of the widest window can touch
// the score buffer of the checked association, doubles per landmark: the map row-major | wx | wy | x0 | y0 | 3 unused
constexpr int PT_SCORE_STRIDE = 448;
constexpr int PT_SCORE_WX = PT_SCORE_W * PT_SCORE_W, PT_SCORE_WY = PT_SCORE_WX + 1, PT_SCORE_X0 = PT_SCORE_WX + 2, PT_SCORE_Y0 = PT_SCORE_WX + 3;
static_assert(PT_PATCH_STRIDE >= PT_PATCH_BYTES && PT_PATCH_STRIDE % 8 == 0 && PT_TMPL_STRIDE >= PT_TMPL_BYTES && PT_TMPL_STRIDE % 8 == 0, "whole doubles per record");
static_assert(PT_SCORE_STRIDE > PT_SCORE_Y0, "the score buffer holds the widest map and its four slots");

// ---- the checked association (srukf_unique.hip) ----
struct MatchArgs { double corr_threshold, ratio; int exclusion, subpixel; };
// its packed result block, what the host exports in one piece: z[2N] | corr[N] | corr2[N] | z2[2N] | matched[N ints] flags[N ints].  Offsets in doubles (flags: in
// ints behind matched), and the block's size
struct MatchRes { size_t z, corr, corr2, z2, matched, flags_ints, doubles; };
constexpr MatchRes match_res(size_t N) { return { .z = 0, .corr = 2 * N, .corr2 = 3 * N, .z2 = 4 * N, .matched = 6 * N, .flags_ints = N, .doubles = 7 * N }; }
constexpr int PT_NO_CAND = 0x7fffffff;                         // index of "no candidate": loses every tie

// ---- the gate: Pi = Si^T Si (1951), its closed-form inverse (cv 2x2; singular: zero), the Mahalanobis distance under it (1975) ----
struct PatchGate { double p00, p11, i00, i01, i10, i11; };
__device__ __forceinline__ PatchGate patch_gate(const double* __restrict__ Si4)
{
#pragma clang fp contract(off)
    const double s00 = Si4[0], s01 = Si4[1], s10 = Si4[2], s11 = Si4[3];
    const double p00 = s00 * s00 + s10 * s10, p01 = s00 * s01 + s10 * s11, p10 = s01 * s00 + s11 * s10, p11 = s01 * s01 + s11 * s11;
    PatchGate g = { p00, p11, 0, 0, 0, 0 };
    double det = p00 * p11 - p01 * p10;
    if (det != 0.0) { det = 1.0 / det; g.i00 = p11 * det; g.i01 = -p01 * det; g.i10 = -p10 * det; g.i11 = p00 * det; }
    return g;
}
__device__ __forceinline__ double patch_gate_dist(const PatchGate& g, double ex, double ey)
{
#pragma clang fp contract(off)
    return (ex * g.i00 + ey * g.i10) * ex + (ex * g.i01 + ey * g.i11) * ey;
}

// the block's maximum of (bv, bi), ties to the lower index (cv::minMaxLoc's first maximum when bi is the row-major index).  256 threads; result in bestv[0] /
// besti[0], valid for every thread after the call
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

// ---- the association's search window (1953-1956): candidate c (row-major) has the centre (x0 + c % wx, y0 + c / wx) ----
struct MatchWindow { double px, py; int half_x, half_y, wx, wy, x0, y0; };
__device__ __forceinline__ MatchWindow match_window(const double* __restrict__ h2, const double* __restrict__ Si4)
{
#pragma clang fp contract(off)
    MatchWindow w;
    w.px = h2[0]; w.py = h2[1];
    w.half_x = min(PT_INIT_HALF, max(PT_MATCH_HALF, (int)ceil(2 * Si4[0])));                            // 1953, 1955
    w.half_y = min(PT_INIT_HALF, max(PT_MATCH_HALF, (int)ceil(2 * Si4[3])));                            // 1954, 1956
    w.wx = 2 * w.half_x + 1; w.wy = 2 * w.half_y + 1;
    w.x0 = (int)w.px - w.half_x; w.y0 = (int)w.py - w.half_y;
    return w;
}

// template statistics (calculateCrossCorrelation, 3151-3161): cv::mean, subtract, cv::norm.  tm [PT_TMPL_BYTES] gets the template minus its mean, red [8] is
// block_sum's; returns the norm.  Ends with a barrier
__device__ __forceinline__ double match_tmpl_stats(const unsigned char* __restrict__ mp, double* tm, double* red)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    double s[1] = { 0.0 };
    for (int e = tid; e < PT_TMPL_BYTES; e += 256) s[0] += mp[e];
    block_sum<1>(s, red);
    const double a2 = s[0] / PT_TMPL_BYTES;
    double q[1] = { 0.0 };
    for (int e = tid; e < PT_TMPL_BYTES; e += 256) { const double v = mp[e] - a2; tm[e] = v; q[0] += v * v; }
    block_sum<1>(q, red);
    const double std2 = sqrt(q[0]);
    __syncthreads();
    return std2;
}

// The pixels every candidate of the window can touch — the window plus the template's half width on every side, <= 37 x 37 — go to rg [PT_REGION_W^2] once (as
// doubles: what the sums take); the candidates' two passes over their 17 x 17 patch then read LDS instead of issuing 578 single-byte global loads each.  Pixels
// outside the image are staged as 0: a candidate whose patch would touch them is skipped by the border test.  Ends with a barrier
__device__ __forceinline__ void match_stage_region(const unsigned char* __restrict__ image, int W, int H, const MatchWindow& w, double* rg)
{
    const int rw = w.wx + 2 * PT_MATCH_HALF, rh = w.wy + 2 * PT_MATCH_HALF, rx0 = w.x0 - PT_MATCH_HALF, ry0 = w.y0 - PT_MATCH_HALF;
    for (int e = threadIdx.x; e < rw * rh; e += 256) {
        const int yy = ry0 + e / rw, xx = rx0 + e % rw;
        rg[(e / rw) * PT_REGION_W + e % rw] = (xx >= 0 && xx < W && yy >= 0 && yy < H) ? (double)image[(size_t)yy * W + xx] : 0.0;
    }
    __syncthreads();
}

// the score of candidate c: 0 when its patch leaves the image (1962, 1969) or its centre lies outside the chi-square gate (1977), else the normalised cross
// correlation of the template with image(j - 8 .., i - 8 ..) = rg(j - y0 .., i - x0 ..) in two passes (3151-3166), every sum in row-major order
__device__ __forceinline__ double match_candidate_score(int c, const MatchWindow& w, int W, int H, const PatchGate& g, const double* rg, const double* tm, double std2)
{
#pragma clang fp contract(off)
    const int j = w.y0 + c / w.wx, i = w.x0 + c % w.wx;                                                 // row-major index of `correlation`
    if ((i < PT_MATCH_HALF || i > W - PT_MATCH_HALF - 1) || (j < PT_MATCH_HALF || j > H - PT_MATCH_HALF - 1)) return 0.0;
    if (!(patch_gate_dist(g, i - w.px, j - w.py) < 5.99146454710798)) return 0.0;
    const double* roi = rg + (j - w.y0) * PT_REGION_W + (i - w.x0);                                     // 1979
    double s1 = 0.0;
    for (int r = 0; r < PT_TMPL_W; r++) for (int cl = 0; cl < PT_TMPL_W; cl++) s1 += roi[r * PT_REGION_W + cl];
    const double a1 = s1 / PT_TMPL_BYTES;
    double q1 = 0.0, dot = 0.0;
    for (int r = 0; r < PT_TMPL_W; r++) for (int cl = 0; cl < PT_TMPL_W; cl++) { const double v1 = roi[r * PT_REGION_W + cl] - a1; q1 += v1 * v1; dot += v1 * tm[r * PT_TMPL_W + cl]; }
    const double std1 = sqrt(q1);
    return (std1 == 0.0 || std2 == 0.0) ? 0.0 : dot / std1 / std2;                                      // 3163-3166
}

// The front for landmark k of a 256-thread workgroup whose landmark is visible and has a record: statistics, gate, window, staging, every candidate scored, the
// first maximum reduced.  keep(c, cc) sees every candidate's score.  Returns the window; the maximum and its index are in bestv[0] / besti[0] (start value -1)
template <class Keep>
__device__ __forceinline__ MatchWindow match_front(int k, const srukf_params& p, const unsigned char* __restrict__ image, const double* __restrict__ h,
                                                   const double* __restrict__ Si, const unsigned char* __restrict__ matchPatch, double* tm, double* red, double* rg,
                                                   double* bestv, int* besti, Keep keep)
{
    const int W = p.image_w, H = p.image_h;
    const double std2 = match_tmpl_stats(matchPatch + (size_t)k * PT_TMPL_STRIDE, tm, red);
    const PatchGate g = patch_gate(Si + 4 * k);
    const MatchWindow w = match_window(h + 2 * k, Si + 4 * k);
    match_stage_region(image, W, H, w, rg);
    double bv = -1.0; int bi = PT_NO_CAND;
    for (int c = threadIdx.x; c < w.wx * w.wy; c += 256) {
        const double cc = match_candidate_score(c, w, W, H, g, rg, tm, std2);
        keep(c, cc);
        if (cc > bv) { bv = cc; bi = c; }                       // candidates of one thread come in increasing index: first maximum kept
    }
    block_first_max(bv, bi, bestv, besti);
    return w;
}
