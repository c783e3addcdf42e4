// srukf_detect.hip — finding new landmarks on the device: Shi-Tomasi "good features to track" (the GoodFeaturesToTrackDetector of
// detectAndfilteringFeatures, SLAM.cpp:599-600), the reference's filter pass over its key points (574-768), and the appearance record
// integrateFeaturesInformation gives every new landmark (918-926).  gfx950 only.
//
// One pass over a 640 x 480 frame that stays in L2:
//   k_det_response   3x3 Sobel gradients + block x block box sums of their products as exact integers (BORDER_REFLECT_101 on the frame and
//                    on the product maps), the minimum eigenvalue r = 0.5 ((A + C) - sqrt((A - C)^2 + 4 B^2)) in fp64, r_max by atomicMax
//   k_det_flags      candidates: interior pixels with r > quality r_max that equal the 3x3 maximum of the thresholded map; count per block
//   k_det_scan       exclusive prefix of the block counts (one workgroup)
//   k_det_scatter    candidates compacted in raster order (no atomics: the order is the tie rule's)
//   k_det_rank       rank of every candidate under (r descending, raster index ascending): a deterministic total order; k_det_place writes each
//   k_det_select     one workgroup: greedy minimum-distance selection up to max_corners, then the filter pass (border, map veto, archived
//                    features -> loop points, pairwise distance)
// For block sizes 3 and 5 every sum below the sqrt is an integer below 2^53 ((A - C)^2 + 4 B^2 <= (A + C)^2 <= (2 * 25 * 1020^2)^2 < 2^53):
// exact in fp64, so the device and a numpy restatement (tests/np_detect.py) agree bit for bit.  OpenCV's cornerMinEigenVal is r s^2 with the
// constant s = 1 / (4 block 255): the same ranking.  This file is built with -ffp-contract=off (the distance tests must round as written).
#include "srukf_ctx.h"
#include "srukf_crtrig.h"
using namespace srukf_impl;

#define DET_T 16                        // output tile edge of k_det_response
#define DET_BLK 256                     // pixels per workgroup of the flag / scatter launches

__device__ __forceinline__ int det_reflect(int v, int n)     // BORDER_REFLECT_101, clamped (tiles past the image edge compute values nobody reads)
{
    if (v < 0) v = -v;
    if (v >= n) v = 2 * n - 2 - v;
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
}

template <int R>
__global__ __launch_bounds__(256) void k_det_response(const unsigned char* __restrict__ img, int W, int H, double* __restrict__ resp,
                                                      unsigned long long* __restrict__ rmax_bits)
{
    constexpr int PW = DET_T + 2 * R, IW = PW + 2;
    __shared__ int si[IW * IW];
    __shared__ int sa[PW * PW], sb[PW * PW], sc[PW * PW];
    __shared__ unsigned long long wmax[4];
    const int tid = threadIdx.x, x0 = blockIdx.x * DET_T, y0 = blockIdx.y * DET_T;
    // the frame around the tile: virtual position v holds I(reflect(v))
    for (int e = tid; e < IW * IW; e += 256) {
        const int vx = x0 - R - 1 + e % IW, vy = y0 - R - 1 + e / IW;
        si[e] = img[(size_t)det_reflect(vy, H) * W + det_reflect(vx, W)];
    }
    __syncthreads();
    // the product maps at virtual positions q: the products of the in-image pixel reflect(q) (its Sobel taps reflect on their own)
    for (int e = tid; e < PW * PW; e += 256) {
        const int qx = det_reflect(x0 - R + e % PW, W) - (x0 - R), qy = det_reflect(y0 - R + e / PW, H) - (y0 - R);
        int a = 0, b = 0, c = 0;
        if (qx >= 0 && qx < PW && qy >= 0 && qy < PW) {
            const int* s = si + qy * IW + qx;                  // top-left tap (image-local centre = q + 1)
            const int gx = (s[2] - s[0]) + 2 * (s[IW + 2] - s[IW]) + (s[2 * IW + 2] - s[2 * IW]);
            const int gy = (s[2 * IW] - s[0]) + 2 * (s[2 * IW + 1] - s[1]) + (s[2 * IW + 2] - s[2]);
            a = gx * gx; b = gx * gy; c = gy * gy;
        }
        sa[e] = a; sb[e] = b; sc[e] = c;
    }
    __syncthreads();
    const int tx = tid % DET_T, ty = tid / DET_T, ox = x0 + tx, oy = y0 + ty;
    double r = 0.0;
    if (ox < W && oy < H) {
        int A = 0, B = 0, C = 0;
        for (int j = 0; j <= 2 * R; j++)
            for (int i = 0; i <= 2 * R; i++) { const int e = (ty + j) * PW + tx + i; A += sa[e]; B += sb[e]; C += sc[e]; }
        const double a = (double)A, b = (double)B, c = (double)C, d = a - c;
        r = 0.5 * ((a + c) - sqrt(d * d + 4.0 * b * b));
        r = r > 0.0 ? r : 0.0;                                 // where AC = B^2 the rounded sqrt can leave a tiny negative: its bit pattern would win the max
        resp[(size_t)oy * W + ox] = r;
    }
    unsigned long long m = (unsigned long long)__double_as_longlong(r);   // non-negative doubles order like their bit patterns
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(m, o); m = t > m ? t : m; }
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++) m = wmax[w] > m ? wmax[w] : m;
        atomicMax(rmax_bits, m);
    }
}

// header words of a pass (unsigned long long): [0] r_max bits, [1] candidates, [2] GFTT corners, [3] accepted key points, [4] loop points
struct DetHdr { unsigned long long rmax, ncand, ngftt, nuv, nloop, pad[3]; };

__device__ __forceinline__ bool det_is_cand(const double* __restrict__ resp, int W, int H, int p, double thr)
{
    const int x = p % W, y = p / W;
    if (x < 1 || x > W - 2 || y < 1 || y > H - 2) return false;
    const double v = resp[p];
    if (!(v > thr)) return false;                              // THRESH_TOZERO: values <= thr are 0 and never a candidate
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) if (resp[p + dy * W + dx] > v) return false;      // v == 3x3 maximum of the thresholded map
    return true;
}

__global__ __launch_bounds__(DET_BLK) void k_det_flags(const double* __restrict__ resp, int W, int H, double quality, const DetHdr* __restrict__ hdr,
                                                       int* __restrict__ blkcnt)
{
    const int p = blockIdx.x * DET_BLK + threadIdx.x;
    const double thr = quality * __longlong_as_double((long long)hdr->rmax);
    const bool f = p < W * H && det_is_cand(resp, W, H, p, thr);
    const int cnt = __syncthreads_count(f);
    if (threadIdx.x == 0) blkcnt[blockIdx.x] = cnt;
}

// exclusive prefix of a flag over a 256-thread block (wave64 ballots); *total = the block's count
__device__ __forceinline__ int det_block_scan(bool f, int* sh4, int* total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) sh4[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int q = 0; q < 4; q++) { if (q < w) off += sh4[q]; tot += sh4[q]; }
    *total = tot;
    return off + pre;
}

__global__ __launch_bounds__(256) void k_det_scan(int* __restrict__ blk, int nb, DetHdr* __restrict__ hdr)
{
    __shared__ int sh4[4];
    __shared__ int sbase;
    if (threadIdx.x == 0) sbase = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? blk[b] : 0;
        // inclusive scan of 256 ints: wave shuffles, then the wave totals
        int s = v;
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(s, o); if ((threadIdx.x & 63) >= o) s += t; }
        __syncthreads();
        if ((threadIdx.x & 63) == 63) sh4[threadIdx.x >> 6] = s;
        __syncthreads();
        int off = sbase;
        for (int q = 0; q < (int)(threadIdx.x >> 6); q++) off += sh4[q];
        if (b < nb) blk[b] = off + s - v;
        __syncthreads();
        if (threadIdx.x == 0) sbase += sh4[0] + sh4[1] + sh4[2] + sh4[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) hdr->ncand = (unsigned long long)sbase;
}

__global__ __launch_bounds__(DET_BLK) void k_det_scatter(const double* __restrict__ resp, int W, int H, double quality, const DetHdr* __restrict__ hdr,
                                                         const int* __restrict__ blkoff, int* __restrict__ cand_pix, double* __restrict__ cand_r,
                                                         int* __restrict__ rank)
{
    __shared__ int sh4[4];
    const int p = blockIdx.x * DET_BLK + threadIdx.x;
    const double thr = quality * __longlong_as_double((long long)hdr->rmax);
    const bool f = p < W * H && det_is_cand(resp, W, H, p, thr);
    int tot;
    const int pos = blkoff[blockIdx.x] + det_block_scan(f, sh4, &tot);
    if (f) { cand_pix[pos] = p; cand_r[pos] = resp[p]; rank[pos] = 0; }
}

// rank(i) = #{j : r_j > r_i} + #{j < i : r_j == r_i}: candidates are in raster order, so equal responses keep ascending y w + x.  The j range
// is cut into DET_SLICES slices (grid.y) so that a few thousand candidates still fill the GPU; the partial counts are integer atomics (the sum
// does not depend on their order), k_det_place then writes every candidate to its rank.
#define DET_SLICES 32
__global__ __launch_bounds__(256) void k_det_rank(const DetHdr* __restrict__ hdr, const double* __restrict__ cand_r, int* __restrict__ rank)
{
    __shared__ double sr[256];
    const int n = (int)hdr->ncand;
    if ((int)(blockIdx.x * 256) >= n) return;
    const int per = (n + DET_SLICES - 1) / DET_SLICES, jb = blockIdx.y * per, je = min(n, jb + per);
    if (jb >= je) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool act = i < n;
    const double ri = act ? cand_r[i] : 0.0;
    int cnt = 0;
    for (int j0 = jb; j0 < je; j0 += 256) {
        __syncthreads();
        if (j0 + (int)threadIdx.x < je) sr[threadIdx.x] = cand_r[j0 + threadIdx.x];
        __syncthreads();
        const int m = min(256, je - j0);
        for (int q = 0; q < m; q++) { const double rj = sr[q]; cnt += (rj > ri) || (rj == ri && j0 + q < i); }
    }
    if (act && cnt) atomicAdd(rank + i, cnt);
}

__global__ __launch_bounds__(256) void k_det_place(const DetHdr* __restrict__ hdr, const int* __restrict__ cand_pix, const int* __restrict__ rank,
                                                   int* __restrict__ sorted_pix)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < (int)hdr->ncand) sorted_pix[rank[i]] = cand_pix[i];
}

struct DetArgs {
    int W, H, limit, use_dist, unfiltered, map_gate, project_archived, n_map, n_arch, uv_cap, loop_cap, n;
    double min_dist2, border;
};

// One workgroup.  GFTT's greedy selection over the sorted candidates in chunks of 256 (each checked against the corners accepted before the
// chunk in parallel, the survivors then in order against the ones the chunk added), then the filter pass of detectAndfilteringFeatures
// (SLAM.cpp:647-752) over the GFTT corners in order.
__global__ __launch_bounds__(256) void k_det_select(DetArgs a, srukf_params p, DetHdr* __restrict__ hdr, const int* __restrict__ sorted_pix,
                                                    int* __restrict__ gxy, int* __restrict__ kxy, const double* __restrict__ map_px, const double* __restrict__ arch,
                                                    double* __restrict__ arch_px, const double* __restrict__ X, double* __restrict__ out_uv,
                                                    int* __restrict__ out_loop)
{
    __shared__ int cx[256], cy[256], ck[256];
    __shared__ int s_nacc, s_nout, s_nloop;
    __shared__ int sh4[4];
    const int tid = threadIdx.x, W = a.W;
    const int n = (int)hdr->ncand;
    if (tid == 0) { s_nacc = 0; s_nout = 0; s_nloop = 0; }
    // archived pixels: projected under the current robot pose (srukf_project, zero pixel error) or the reference's zeroed pixelPos
    for (int j = tid; j < a.n_arch; j += 256) {
        double u = 0.0, v = 0.0;
        if (a.project_archived) {
            double f[6];
            for (int e = 0; e < 6; e++) f[e] = arch[6 * j + e];
            double sn, cs;
            sincos(X[a.n - 1], &sn, &cs);
            srukf_project(p, p.cam_f / p.cam_dx, p.cam_f / p.cam_dy, f, X[a.n - 4], X[a.n - 3], X[a.n - 2], cs, sn, 0.0, 0.0, u, v);
        }
        arch_px[2 * j] = u; arch_px[2 * j + 1] = v;
    }
    __syncthreads();
    // ---- GFTT selection ----
    for (int base = 0; base < n; base += 256) {
        const int nacc0 = s_nacc;
        if (nacc0 >= a.limit) break;
        const int i = base + tid;
        int ok = 0, x = 0, y = 0;
        if (i < n) {
            const int pix = sorted_pix[i];
            x = pix % W; y = pix / W; ok = 1;
            if (a.use_dist)
                for (int q = 0; q < nacc0; q++) {
                    const double dx = (double)(x - gxy[2 * q]), dy = (double)(y - gxy[2 * q + 1]);
                    if (dx * dx + dy * dy < a.min_dist2) { ok = 0; break; }
                }
        }
        cx[tid] = x; cy[tid] = y; ck[tid] = ok;
        __syncthreads();
        if (tid == 0) {
            int nacc = nacc0;
            for (int t = 0; t < 256 && nacc < a.limit; t++) {
                if (!ck[t]) continue;
                bool good = true;
                if (a.use_dist)
                    for (int q = nacc0; q < nacc; q++) {
                        const double dx = (double)(cx[t] - gxy[2 * q]), dy = (double)(cy[t] - gxy[2 * q + 1]);
                        if (dx * dx + dy * dy < a.min_dist2) { good = false; break; }
                    }
                if (good) { gxy[2 * nacc] = cx[t]; gxy[2 * nacc + 1] = cy[t]; nacc++; }
            }
            s_nacc = nacc;
        }
        __syncthreads();
    }
    __syncthreads();
    const int ng = s_nacc;
    // ---- filter pass (SLAM.cpp:639-752), key point i in GFTT order ----
    for (int i = 0; i < ng; i++) {
        const double kx = gxy[2 * i], ky = gxy[2 * i + 1];
        if (!(kx >= a.border && kx <= a.W - a.border && ky >= a.border && ky <= a.H - a.border)) continue;     // 650-651
        bool rej = false;
        if (!a.unfiltered) {                                                                                     // 653
            if (a.map_gate) {                                                                                    // 660-697
                bool hit = false;
                for (int m = tid; m < a.n_map; m += 256) {
                    const double mx = map_px[4 * m], my = map_px[4 * m + 1], px = map_px[4 * m + 2], py = map_px[4 * m + 3];
                    if (mx != 0.0 && my != 0.0 && px != 0.0 && py != 0.0) {
                        const double dmx = kx - mx, dmy = ky - my, dpx = kx - px, dpy = ky - py;
                        if (a.min_dist2 > dmx * dmx + dmy * dmy || a.min_dist2 > dpx * dpx + dpy * dpy) hit = true;
                    } else hit = true;                                                                           // 690-693: an entry with a zero rejects
                }
                rej = __syncthreads_or(hit);
            }
            if (!rej && a.n_arch > 0) {                                                                          // 699-729: every archived point, no break
                for (int j0 = 0; j0 < a.n_arch; j0 += 256) {
                    const int j = j0 + tid;
                    bool h = false;
                    if (j < a.n_arch) {
                        const double dx = kx - arch_px[2 * j], dy = ky - arch_px[2 * j + 1];
                        h = dx * dx + dy * dy < a.min_dist2;
                    }
                    int tot;
                    const int pos = s_nloop + det_block_scan(h, sh4, &tot);
                    if (h && pos < a.loop_cap) { out_loop[2 * pos] = i; out_loop[2 * pos + 1] = j; }
                    __syncthreads();
                    if (tid == 0) s_nloop += tot;
                    if (tot) rej = true;
                    __syncthreads();
                }
            }
            if (!rej) {                                                                                          // 731-750
                bool hit = false;
                const int nout = s_nout;
                for (int q = tid; q < nout; q += 256) {
                    const double dx = kx - kxy[2 * q], dy = ky - kxy[2 * q + 1];
                    if (a.min_dist2 > dx * dx + dy * dy) hit = true;
                }
                rej = __syncthreads_or(hit);
            }
        }
        if (!rej) {
            if (tid == 0) {
                const int q = s_nout;
                kxy[2 * q] = (int)kx; kxy[2 * q + 1] = (int)ky;
                if (q < a.uv_cap) { out_uv[2 * q] = kx; out_uv[2 * q + 1] = ky; }
                s_nout = q + 1;
            }
        }
        __syncthreads();
    }
    if (tid == 0) { hdr->ngftt = (unsigned long long)ng; hdr->nuv = (unsigned long long)s_nout; hdr->nloop = (unsigned long long)s_nloop; }
}

// integrateFeaturesInformation's appearance fields (SLAM.cpp:918-926) for landmarks first .. first + K - 1: initPatch = the 21 x 21 window at
// cvRound(uv) (round half to even), initRotation = Rwc of the current heading (getTransferMatrix 1031-1037; correctly rounded sin / cos, as the
// warp reads its own pose), initTrans = the robot x, y, z (834-836), matchPatch zeroed, has_app = 1.  One workgroup per landmark, one thread per byte of a patch record.
__global__ __launch_bounds__(PT_PATCH_STRIDE) void k_capture_patch(const unsigned char* __restrict__ img, int W, int first, const double* __restrict__ uv,
                                                       const double* __restrict__ X, int n, unsigned char* __restrict__ app_patch, int patch_stride,
                                                       unsigned char* __restrict__ app_tmpl, int tmpl_stride, double* __restrict__ appR,
                                                       double* __restrict__ appT, double* __restrict__ appPx, int* __restrict__ has_app)
{
    const int q = blockIdx.x, k = first + q, t = threadIdx.x;
    const int u = (int)rint(uv[2 * q]), v = (int)rint(uv[2 * q + 1]);
    if (t < PT_PATCH_BYTES) app_patch[(size_t)k * patch_stride + t] = img[(size_t)(v - PT_INIT_HALF + t / PT_PATCH_W) * W + (u - PT_INIT_HALF + t % PT_PATCH_W)];
    if (t < tmpl_stride) app_tmpl[(size_t)k * tmpl_stride + t] = 0;
    if (t == 0) {
        double sn, cs;
        crt_sincos(X[n - 1], &sn, &cs);
        const double R[9] = { cs, -sn, 0, sn, cs, 0, 0, 0, 1 };
        for (int e = 0; e < 9; e++) appR[9 * k + e] = R[e];
        for (int e = 0; e < 3; e++) appT[3 * k + e] = X[n - 4 + e];
        appPx[2 * k] = uv[2 * q]; appPx[2 * k + 1] = uv[2 * q + 1];
        has_app[k] = 1;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------

namespace srukf_impl {

void det_scratch_free(DetScratch& s, hipStream_t st)
{
    for (void* b : { (void*)s.resp, (void*)s.cand_r, (void*)s.cand_pix, (void*)s.sorted, (void*)s.rank, (void*)s.gxy, (void*)s.blk, (void*)s.hdr, (void*)s.in, (void*)s.out })
        if (b) srukf_dfree_on(b, st);
    s = DetScratch();
}

void launch_capture_patch(hipStream_t st, const unsigned char* img, int W, int first, int K, const double* uv, const double* X, int n,
                          unsigned char* app_patch, unsigned char* app_tmpl, double* appR, double* appT, double* appPx, int* has_app)
{
    hipLaunchKernelGGL(k_capture_patch, dim3(K), dim3(PT_PATCH_STRIDE), 0, st, img, W, first, uv, X, n, app_patch, PT_PATCH_STRIDE, app_tmpl,
                       PT_TMPL_STRIDE, appR, appT, appPx, has_app);
}

int ensure_image(srukf_ctx* c)
{
    if (c->d_image) return SRUKF_OK;
    HIPCHK(c, srukf_dmalloc((void**)&c->d_image, (size_t)c->p.image_w * c->p.image_h));
    return SRUKF_OK;
}

// the frame `gray` becomes the one the handle holds; NULL: the held one (SRUKF_ERR_SEQUENCE if there is none)
int take_frame(srukf_ctx* c, const unsigned char* gray)
{
    if (!gray) {
        if (!c->frame_valid || !c->d_image) { c->err = "no frame held: pass the gray frame"; return SRUKF_ERR_SEQUENCE; }
        return SRUKF_OK;
    }
    int rc = ensure_image(c); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_image, gray, (size_t)c->p.image_w * c->p.image_h, hipMemcpyHostToDevice, c->stream));
    c->frame_valid = true; c->bgr_valid = false;                 // (a gray frame of the caller's: the held colour frame is no longer its colour)
    return SRUKF_OK;
}

}  // namespace srukf_impl

static int det_grow(srukf_ctx* c, void** buf, size_t* have, size_t need)
{
    if (*have >= need && *buf) return SRUKF_OK;
    if (*buf) srukf_dfree_on(*buf, c->stream);
    *buf = nullptr; *have = 0;
    HIPCHK(c, srukf_dmalloc_on(buf, need, c->stream));
    *have = need;
    return SRUKF_OK;
}

extern "C" {

int srukf_detect_features(srukf_ctx* c, const unsigned char* gray, const srukf_detect_params* dp, int n_map, const double* map_px, int n_archived,
                          const double* archived_state6, double* uv_out, int uv_cap, int* n_uv, int* loop_out, int loop_cap, int* n_loop)
{
    if (!c || !dp || !n_uv || n_map < 0 || n_archived < 0 || uv_cap < 0 || loop_cap < 0) return SRUKF_ERR_BAD_ARG;
    if ((n_map > 0 && !map_px) || (n_archived > 0 && !archived_state6) || (uv_cap > 0 && !uv_out) || (loop_cap > 0 && !loop_out)) return SRUKF_ERR_BAD_ARG;
    if (!(dp->quality_level >= 0.0) || !(dp->min_dist == dp->min_dist) || !(dp->dist_to_border == dp->dist_to_border)) return SRUKF_ERR_BAD_ARG;
    if (dp->block_size != 3 && dp->block_size != 5) { c->err = "detect_features: block_size must be 3 or 5 (exact integer sums)"; return SRUKF_ERR_UNSUPPORTED; }
    const int W = (int)c->p.image_w, H = (int)c->p.image_h;
    if (W < 8 || H < 8) { c->err = "detect_features: image smaller than 8 x 8"; return SRUKF_ERR_BAD_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    step_commit_motion(c);                                               // (the archived projection reads the robot pose)
    int rc = take_frame(c, gray); if (rc) return rc;
    DetScratch& s = c->det;
    const size_t WH = (size_t)W * H;
    const int nb = (int)((WH + DET_BLK - 1) / DET_BLK);
    if (!s.resp) {                                                       // the scratch of the handle scope, on its first pass
        if (srukf_dmalloc_on(&s.resp, sizeof(double) * WH, c->stream) != hipSuccess || srukf_dmalloc_on(&s.cand_r, sizeof(double) * WH, c->stream) != hipSuccess ||
            srukf_dmalloc_on(&s.cand_pix, sizeof(int) * WH, c->stream) != hipSuccess || srukf_dmalloc_on(&s.sorted, sizeof(int) * WH, c->stream) != hipSuccess ||
            srukf_dmalloc_on(&s.rank, sizeof(int) * WH, c->stream) != hipSuccess ||
            srukf_dmalloc_on(&s.gxy, sizeof(int) * 4 * WH, c->stream) != hipSuccess || srukf_dmalloc_on(&s.blk, sizeof(int) * nb, c->stream) != hipSuccess ||
            srukf_dmalloc_on(&s.hdr, sizeof(DetHdr), c->stream) != hipSuccess) {
            det_scratch_free(s, c->stream); c->err = "detect_features: out of device memory"; return SRUKF_ERR_NOMEM;
        }
    }
    const int limit = dp->max_corners > 0 ? dp->max_corners : (uv_cap > 0 ? uv_cap : 1);
    const size_t in_d = 4 * (size_t)n_map + 8 * (size_t)n_archived;      // map_px | archived states | their pixels
    const size_t out_b = sizeof(double) * 2 * (size_t)uv_cap + sizeof(int) * 2 * (size_t)loop_cap;
    rc = det_grow(c, &s.in, &s.in_bytes, sizeof(double) * (in_d ? in_d : 1)); if (rc) return rc;
    rc = det_grow(c, &s.out, &s.out_bytes, out_b ? out_b : 8); if (rc) return rc;
    double* din = (double*)s.in;
    double* d_map = din; double* d_arch = din + 4 * (size_t)n_map; double* d_apx = d_arch + 6 * (size_t)n_archived;
    double* d_uv = (double*)s.out; int* d_loop = (int*)(d_uv + 2 * (size_t)uv_cap);
    if (n_map) HIPCHK(c, hipMemcpyAsync(d_map, map_px, sizeof(double) * 4 * n_map, hipMemcpyHostToDevice, c->stream));
    if (n_archived) HIPCHK(c, hipMemcpyAsync(d_arch, archived_state6, sizeof(double) * 6 * n_archived, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(s.hdr, 0, sizeof(DetHdr), c->stream));
    DetHdr* hdr = (DetHdr*)s.hdr;
    {
        ProfScope ps(c, KC_DET_RESPONSE, 0, (double)WH * (1.0 + 8.0));
        const dim3 g((W + DET_T - 1) / DET_T, (H + DET_T - 1) / DET_T);
        if (dp->block_size == 3) hipLaunchKernelGGL(k_det_response<1>, g, dim3(256), 0, c->stream, c->d_image, W, H, s.resp, &hdr->rmax);
        else hipLaunchKernelGGL(k_det_response<2>, g, dim3(256), 0, c->stream, c->d_image, W, H, s.resp, &hdr->rmax);
    }
    {
        ProfScope ps(c, KC_DET_CAND, 0, (double)WH * 8.0 * 2.0);
        hipLaunchKernelGGL(k_det_flags, dim3(nb), dim3(DET_BLK), 0, c->stream, s.resp, W, H, dp->quality_level, hdr, s.blk);
        hipLaunchKernelGGL(k_det_scan, dim3(1), dim3(256), 0, c->stream, s.blk, nb, hdr);
        hipLaunchKernelGGL(k_det_scatter, dim3(nb), dim3(DET_BLK), 0, c->stream, s.resp, W, H, dp->quality_level, hdr, s.blk, s.cand_pix, s.cand_r, s.rank);
    }
    {
        ProfScope ps(c, KC_DET_RANK, 0, 0);
        hipLaunchKernelGGL(k_det_rank, dim3(nb, DET_SLICES), dim3(256), 0, c->stream, hdr, s.cand_r, s.rank);
        hipLaunchKernelGGL(k_det_place, dim3(nb), dim3(256), 0, c->stream, hdr, s.cand_pix, s.rank, s.sorted);
    }
    {
        ProfScope ps(c, KC_DET_SELECT, 0, 0);
        DetArgs a;
        a.W = W; a.H = H; a.limit = limit; a.use_dist = dp->min_dist >= 1.0; a.unfiltered = dp->unfiltered != 0; a.map_gate = dp->map_gate != 0;
        a.project_archived = dp->project_archived != 0; a.n_map = n_map; a.n_arch = n_archived; a.uv_cap = uv_cap; a.loop_cap = loop_cap; a.n = c->d.n;
        a.min_dist2 = dp->min_dist * dp->min_dist; a.border = dp->dist_to_border;
        hipLaunchKernelGGL(k_det_select, dim3(1), dim3(256), 0, c->stream, a, c->p, hdr, s.sorted, s.gxy, s.gxy + 2 * WH, d_map, d_arch, d_apx, c->X, d_uv, d_loop);
    }
    HIPCHK(c, hipGetLastError());
    DetHdr h;
    HIPCHK(c, hipMemcpyAsync(&h, hdr, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int nuv = (int)h.nuv, nl = (int)h.nloop;
    if (nuv && uv_cap) HIPCHK(c, hipMemcpy(uv_out, d_uv, sizeof(double) * 2 * std::min(nuv, uv_cap), hipMemcpyDeviceToHost));
    if (nl && loop_cap) HIPCHK(c, hipMemcpy(loop_out, d_loop, sizeof(int) * 2 * std::min(nl, loop_cap), hipMemcpyDeviceToHost));
    *n_uv = nuv;
    if (n_loop) *n_loop = nl;
    return SRUKF_OK;
}

}  // extern "C"
