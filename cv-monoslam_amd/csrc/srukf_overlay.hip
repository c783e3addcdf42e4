// Colour-frame intake and the 2-D feature overlay: loadPictures (SLAM.cpp:529-543) and display2DFeatureModel / draw2DEllipse (3009-3083) on frames the device holds.
//
// k_bgr2gray      W x H x 3 interleaved bytes (B, G, R; no row padding) -> the held gray frame, OpenCV 2.4's fixed-point CV_RGB2GRAY applied to B, G, R in memory
//                 order as the reference applies it (channel 0 gets the weight of red): gray = (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14, integer and exact.
// k_overlay_prep  one thread per landmark: the rounded centres, Pi = Si^T Si, its eigenvalues in closed form, the integer semi-axes and the unit eigenvector of the
//                 larger eigenvalue -> one OvRec.  fp64 + - * / sqrt in the order written, no contraction (-ffp-contract=off): tests/np_overlay.py restates it.
// k_overlay       one workgroup per tile of 1024 pixels; the source pixel, then every landmark whose boxes meet the tile, in state order, later over earlier and
//                 within a landmark predicted cross, matched cross, ellipse.  Every pixel has one owner: no atomics, nothing depends on scheduling.
// k_overlay_prep_block / k_overlay_block  the same two for a run of staged frames, the frame a grid dimension (srukf_render_image_overlays).
//                 They call the bodies the single-frame kernels call (ov_prep_one, ov_raster_tile): the painted bytes are equal by construction.
// A stack of colour frames needs no kernel of its own: frames are tight in both stacks (3 W H and W H bytes), so F frames are ONE run of F W H pixels to k_bgr2gray,
// whose groups of four are dword-aligned from the start of the stack whatever W H is (srukf_stage_images_bgr walks the run in chunks that are multiples of four).
//
// The frames have no row padding, so both pixel kernels walk the frame as ONE run of W H pixels in groups of four: 12 colour bytes = three dwords, 4 gray bytes =
// one dword, every group dword-aligned whatever W is (a row-based split would be aligned only when W is a multiple of four).  A group may straddle two rows; each
// pixel derives its own (x, y).  The colour and output buffers are the library's own and padded to whole groups; the gray frame (d_image) is exactly W H bytes, so
// the last group, when W H is no multiple of four, takes its gray bytes one by one.
#include "srukf_ctx.h"

#define OV_THREADS 256
#define OV_TILE    (4 * OV_THREADS)                             // pixels per workgroup
#define OV_CHUNK   64                                           // landmarks compacted per pass: one wave's ballot
#define OV_CROSS   10                                           // half length of a cross arm (3035-3041)

namespace {

struct OvRec {
    int flags;                                                  // bit 0: drawn, bit 1: ellipse
    int px, py, mx, my, a, b, pad_;
    double c, s;
};

__device__ __forceinline__ unsigned gray_of(unsigned c0, unsigned c1, unsigned c2) { return (4899u * c0 + 9617u * c1 + 1868u * c2 + 8192u) >> 14; }

__device__ __forceinline__ bool box_meets(int cx, int cy, int r, int x0, int x1, int y0, int y1)
{
    return cx + r >= x0 && cx - r <= x1 && cy + r >= y0 && cy - r <= y1;                       // |cx|, |cy| < 2^30 and r < 2^22: no overflow
}

}  // namespace

__global__ __launch_bounds__(OV_THREADS) void k_bgr2gray(int npix, const unsigned int* __restrict__ bgr, unsigned char* __restrict__ gray)
{
    const int g = blockIdx.x * OV_THREADS + threadIdx.x, p0 = 4 * g;
    if (p0 >= npix) return;
    // bytes b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3 (little endian)
    const unsigned w0 = bgr[3 * (size_t)g], w1 = bgr[3 * (size_t)g + 1], w2 = bgr[3 * (size_t)g + 2];
    const unsigned y0 = gray_of(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
    const unsigned y1 = gray_of(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
    const unsigned y2 = gray_of((w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
    const unsigned y3 = gray_of((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
    if (p0 + 3 < npix) {
        *(unsigned int*)(gray + p0) = y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);
    } else {                                                    // the frame's last one to three pixels: gray is exactly npix bytes
        gray[p0] = (unsigned char)y0;
        if (p0 + 1 < npix) gray[p0 + 1] = (unsigned char)y1;
        if (p0 + 2 < npix) gray[p0 + 2] = (unsigned char)y2;
    }
}

namespace {

// landmark k's record: the body of both prep kernels
__device__ __forceinline__ OvRec ov_prep_one(int k, const double* __restrict__ h, const double* __restrict__ Si, const double* __restrict__ z, const int* __restrict__ matched)
{
    OvRec r;
    r.flags = 0; r.px = r.py = r.mx = r.my = 0; r.a = r.b = 1; r.pad_ = 0; r.c = 1.0; r.s = 0.0;
    const double hx = h[2 * k], hy = h[2 * k + 1], zx = z[2 * k], zy = z[2 * k + 1];
    const double lim = 1073741824.0;                            // 2^30 (a NaN or an infinity fails the comparison too)
    const bool drawn = matched[k] != 0 && fabs(hx) < lim && fabs(hy) < lim && fabs(zx) < lim && fabs(zy) < lim;
    if (drawn) {
        r.flags = 1;
        r.px = (int)rint(hx); r.py = (int)rint(hy); r.mx = (int)rint(zx); r.my = (int)rint(zy);     // cvRound: to nearest, ties to even
        const double s00 = Si[4 * k], s01 = Si[4 * k + 1], s10 = Si[4 * k + 2], s11 = Si[4 * k + 3];
        const double p00 = s00 * s00 + s10 * s10, p01 = s00 * s01 + s10 * s11, p11 = s01 * s01 + s11 * s11;   // Pi = Si.t() * Si (3031)
        const double t = 0.5 * (p00 + p11), d = 0.5 * (p00 - p11), rr = sqrt(d * d + p01 * p01);
        const double l0 = t + rr, l1 = fmax(t - rr, 0.0);
        if (l0 < 1e12) {                                        // finite and below 1e12: a NaN or an infinity fails the comparison (eigen "fails": 3073)
            r.flags |= 2;
            const double chi = sqrt(5.99146454710798);          // CHI2INV_TABLE(0, 2) (3076-3077)
            r.a = max(1, (int)(sqrt(l0) * chi)); r.b = max(1, (int)(sqrt(l1) * chi));
            if (rr == 0.0) { r.c = 1.0; r.s = 0.0; }
            else {
                double vx, vy;
                if (d >= 0.0) { vx = d + rr; vy = p01; } else { vx = p01; vy = rr - d; }
                const double m = fmax(fabs(vx), fabs(vy));      // > 0: d + rr >= rr, rr - d > rr.  Scaled first: no overflow or underflow in the squares
                const double ux = vx / m, uy = vy / m, nn = sqrt(ux * ux + uy * uy);
                r.c = ux / nn; r.s = uy / nn;
            }
        }
    }
    return r;
}

// tile `tile` of one frame: the body of both raster kernels.  list [OV_CHUNK] and nlist are the calling kernel's own LDS
__device__ __forceinline__ void ov_raster_tile(OvRec* list, int& nlist, int tile, int W, int npix, int N, const unsigned int* __restrict__ bgr,
                                               const unsigned char* __restrict__ gray, const OvRec* __restrict__ rec, unsigned int* __restrict__ out)
{
    const int tile0 = tile * OV_TILE, tile1 = min(tile0 + OV_TILE, npix) - 1;                  // first and last pixel of the tile (tile0 < npix by the grid)
    const int ty0 = tile0 / W, ty1 = tile1 / W;
    const int tx0 = ty0 == ty1 ? tile0 - ty0 * W : 0, tx1 = ty0 == ty1 ? tile1 - ty1 * W : W - 1;
    const int g = tile * OV_THREADS + threadIdx.x, p0 = 4 * g;
    const bool live = p0 < npix;
    // the source: the held colour frame, or the gray byte three times.  col[j] = B | G << 8 | R << 16
    unsigned col[4] = { 0, 0, 0, 0 };
    int x[4], y[4];
    if (live) {
        if (bgr) {
            const unsigned w0 = bgr[3 * (size_t)g], w1 = bgr[3 * (size_t)g + 1], w2 = bgr[3 * (size_t)g + 2];
            col[0] = w0 & 0xffffffu; col[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8); col[2] = (w1 >> 16) | ((w2 & 0xffu) << 16); col[3] = w2 >> 8;
        } else {
            unsigned v;
            if (p0 + 3 < npix) v = *(const unsigned int*)(gray + p0);
            else { v = gray[p0]; if (p0 + 1 < npix) v |= (unsigned)gray[p0 + 1] << 8; if (p0 + 2 < npix) v |= (unsigned)gray[p0 + 2] << 16; }
#pragma unroll
            for (int j = 0; j < 4; j++) col[j] = ((v >> (8 * j)) & 255u) * 0x010101u;
        }
        y[0] = p0 / W; x[0] = p0 - y[0] * W;
#pragma unroll
        for (int j = 1; j < 4; j++) { x[j] = x[j - 1] + 1; y[j] = y[j - 1]; if (x[j] == W) { x[j] = 0; y[j]++; } }
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) { x[j] = 0; y[j] = 0; }
    }
    for (int base = 0; base < N; base += OV_CHUNK) {
        // wave 0 compacts, in index order, the landmarks of this chunk whose boxes meet the tile
        if (threadIdx.x < 64) {
            const int k = base + (int)threadIdx.x;
            OvRec r = {}; bool hit = false;
            if (k < N) {
                r = rec[k];
                if (r.flags & 1) {
                    const int rm = (r.flags & 2) ? max(OV_CROSS, r.a + 1) : OV_CROSS;
                    hit = box_meets(r.px, r.py, OV_CROSS, tx0, tx1, ty0, ty1) || box_meets(r.mx, r.my, rm, tx0, tx1, ty0, ty1);
                }
            }
            const unsigned long long mask = __ballot(hit);
            const int pos = __popcll(mask & ((1ull << threadIdx.x) - 1ull));
            if (hit) list[pos] = r;
            if (threadIdx.x == 0) nlist = __popcll(mask);
        }
        __syncthreads();
        const int n = nlist;
        if (live) {
            for (int q = 0; q < n; q++) {
                const int flags = list[q].flags, px = list[q].px, py = list[q].py, mx = list[q].mx, my = list[q].my, a = list[q].a, b = list[q].b;
                const double c = list[q].c, s = list[q].s;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int dxp = abs(x[j] - px), dyp = abs(y[j] - py), dxm = abs(x[j] - mx), dym = abs(y[j] - my);
                    const bool hp = (dxp <= OV_CROSS && dyp <= 1) || (dyp <= OV_CROSS && dxp <= 1);
                    bool hm = (dxm <= OV_CROSS && dym <= 1) || (dym <= OV_CROSS && dxm <= 1);
                    if (!hm && (flags & 2) && dxm <= a + 1 && dym <= a + 1) {                   // (b <= a: the band lies inside the circle of radius a + 1)
                        const double dx = (double)(x[j] - mx), dy = (double)(y[j] - my);
                        const double p = c * dx + s * dy, qq = c * dy - s * dx;
                        const double A1 = (double)(a + 1), B1 = (double)(b + 1);
                        const double u1 = p / A1, v1 = qq / B1;
                        if (u1 * u1 + v1 * v1 <= 1.0) {
                            hm = true;
                            if (a >= 2 && b >= 2) {
                                const double A0 = (double)(a - 1), B0 = (double)(b - 1);
                                const double u0 = p / A0, v0 = qq / B0;
                                if (u0 * u0 + v0 * v0 <= 1.0) hm = false;
                            }
                        }
                    }
                    if (hm) col[j] = 0xff0000u;                 // B, G, R = (0, 0, 255): CV_RGB(255, 0, 0)
                    else if (hp) col[j] = 0x0000ffu;            // (255, 0, 0): CV_RGB(0, 0, 255)
                }
            }
        }
        __syncthreads();
    }
    if (live) {                                                 // out is padded to whole groups: three dwords whatever npix is
        out[3 * (size_t)g] = col[0] | (col[1] << 24);
        out[3 * (size_t)g + 1] = (col[1] >> 8) | (col[2] << 16);
        out[3 * (size_t)g + 2] = (col[2] >> 16) | (col[3] << 8);
    }
}

}  // namespace

__global__ __launch_bounds__(64) void k_overlay_prep(int N, const double* __restrict__ h, const double* __restrict__ Si, const double* __restrict__ z,
                                                     const int* __restrict__ matched, OvRec* __restrict__ rec)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k < N) rec[k] = ov_prep_one(k, h, Si, z, matched);
}

__global__ __launch_bounds__(OV_THREADS) void k_overlay(int W, int npix, int N, const unsigned int* __restrict__ bgr, const unsigned char* __restrict__ gray,
                                                        const OvRec* __restrict__ rec, unsigned int* __restrict__ out)
{
    __shared__ OvRec list[OV_CHUNK];
    __shared__ int nlist;
    ov_raster_tile(list, nlist, blockIdx.x, W, npix, N, bgr, gray, rec, out);
}

// The two kernels for a run of staged frames: blockIdx.y is the frame.  Frame q reads its own rows (strides in elements), writes its own slab of N records, and the
// raster reads frame q's source and writes frame q's output.  npix is a multiple of four (srukf_render_image_overlays refuses anything else), so every frame of the
// tight stacks starts on a dword: 3 npix / 4 dwords of colour and of output per frame, npix bytes of gray
struct OvBlockRows { const double *h, *Si, *z; const int* matched; size_t h_stride, Si_stride, z_stride, m_stride; };

__global__ __launch_bounds__(64) void k_overlay_prep_block(int N, OvBlockRows rows, OvRec* __restrict__ rec)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    const size_t q = blockIdx.y;
    if (k < N) rec[q * (size_t)N + k] = ov_prep_one(k, rows.h + q * rows.h_stride, rows.Si + q * rows.Si_stride, rows.z + q * rows.z_stride, rows.matched + q * rows.m_stride);
}

__global__ __launch_bounds__(OV_THREADS) void k_overlay_block(int W, int npix, int N, const unsigned int* __restrict__ bgr, const unsigned char* __restrict__ gray,
                                                              const OvRec* __restrict__ rec, unsigned int* __restrict__ out)
{
    __shared__ OvRec list[OV_CHUNK];
    __shared__ int nlist;
    const size_t q = blockIdx.y, dwords = 3 * ((size_t)npix / 4);
    ov_raster_tile(list, nlist, blockIdx.x, W, npix, N, bgr ? bgr + q * dwords : nullptr, gray + q * (size_t)npix, rec + q * (size_t)N, out + q * dwords);
}

namespace srukf_impl {

size_t overlay_rec_bytes(int N) { return sizeof(OvRec) * (size_t)(N > 0 ? N : 1); }
// bytes of a W x H x 3 buffer the pixel kernels may touch: whole groups of four pixels
size_t overlay_bgr_bytes(int npix) { return 12 * (((size_t)npix + 3) / 4); }

void launch_bgr2gray(hipStream_t st, int npix, const unsigned char* bgr, unsigned char* gray)
{
    const int groups = (npix + 3) / 4;
    hipLaunchKernelGGL(k_bgr2gray, dim3((groups + OV_THREADS - 1) / OV_THREADS), dim3(OV_THREADS), 0, st, npix, (const unsigned int*)bgr, gray);
}

void launch_overlay(hipStream_t st, int W, int H, int N, const double* h, const double* Si, const double* z, const int* matched, void* rec,
                    const unsigned char* bgr, const unsigned char* gray, unsigned char* out)
{
    const int npix = W * H;
    if (N > 0) hipLaunchKernelGGL(k_overlay_prep, dim3((N + 63) / 64), dim3(64), 0, st, N, h, Si, z, matched, (OvRec*)rec);
    hipLaunchKernelGGL(k_overlay, dim3((npix + OV_TILE - 1) / OV_TILE), dim3(OV_THREADS), 0, st, W, npix, N, (const unsigned int*)bgr, gray, (const OvRec*)rec,
                       (unsigned int*)out);
}

// count staged frames in two launches.  Every pointer is the first frame's; the strides of the rows are in elements, the stacks are tight (bgr and out: 3 npix
// bytes per frame, gray: npix), rec holds count slabs of N records.  W H is a multiple of four, N >= 1 and 1 <= count <= OVERLAY_BLOCK_MAX: the frame is
// gridDim.y (srukf_render_image_overlays refuses a larger count)
void launch_overlay_block(hipStream_t st, int W, int H, int N, int count, const double* h, size_t h_stride, const double* Si, size_t Si_stride, const double* z, size_t z_stride,
                          const int* matched, size_t m_stride, void* rec, const unsigned char* bgr, const unsigned char* gray, unsigned char* out)
{
    const int npix = W * H;
    const OvBlockRows rows = { h, Si, z, matched, h_stride, Si_stride, z_stride, m_stride };
    hipLaunchKernelGGL(k_overlay_prep_block, dim3((N + 63) / 64, count), dim3(64), 0, st, N, rows, (OvRec*)rec);
    hipLaunchKernelGGL(k_overlay_block, dim3((npix + OV_TILE - 1) / OV_TILE, count), dim3(OV_THREADS), 0, st, W, npix, N, (const unsigned int*)bgr, gray, (const OvRec*)rec,
                       (unsigned int*)out);
}

}  // namespace srukf_impl

using namespace srukf_impl;

extern "C" {

// loadPictures (SLAM.cpp:529-543): the colour frame becomes the held colour frame, its conversion the held gray frame
int srukf_set_frame_bgr(srukf_ctx* c, const unsigned char* bgr, unsigned char* gray_out)
{
    if (!c || !bgr) return SRUKF_ERR_BAD_ARG;
    const int W = (int)c->p.image_w, H = (int)c->p.image_h;
    if (W < 1 || H < 1 || (double)W * H > 268435456.0) { c->err = "set_frame_bgr: image size"; return SRUKF_ERR_BAD_ARG; }
    const int npix = W * H;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_image(c); if (rc) return rc;
    if (!c->d_bgr) HIPCHK(c, srukf_dmalloc((void**)&c->d_bgr, overlay_bgr_bytes(npix)));
    HIPCHK(c, hipMemcpyAsync(c->d_bgr, bgr, 3 * (size_t)npix, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, KC_BGR2GRAY, 0, 4.0 * npix);
        launch_bgr2gray(c->stream, npix, c->d_bgr, c->d_image);
    }
    HIPCHK(c, hipGetLastError());
    c->frame_valid = true; c->bgr_valid = true;
    if (gray_out) HIPCHK(c, hipMemcpyAsync(gray_out, c->d_image, (size_t)npix, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                  // (bgr and gray_out are the caller's pageable memory)
    return SRUKF_OK;
}

// display2DFeatureModel + draw2DEllipse (SLAM.cpp:3009-3083) over the held frame, from the caller's arrays: nothing of the filter is read or written
int srukf_render_overlay(srukf_ctx* c, const double* h, const double* Si, const double* z, const int* matched, unsigned char* out_bgr)
{
    if (!c || !out_bgr) return SRUKF_ERR_BAD_ARG;
    const int N = c->d.N;
    if (N > 0 && (!h || !Si || !z || !matched)) return SRUKF_ERR_BAD_ARG;
    if (!c->frame_valid || !c->d_image) { c->err = "render_overlay: no frame held"; return SRUKF_ERR_SEQUENCE; }
    const int W = (int)c->p.image_w, H = (int)c->p.image_h;
    if (W < 1 || H < 1 || (double)W * H > 268435456.0) { c->err = "render_overlay: image size"; return SRUKF_ERR_BAD_ARG; }
    const int npix = W * H;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_ovl) HIPCHK(c, srukf_dmalloc((void**)&c->d_ovl, overlay_bgr_bytes(npix)));
    const size_t in_doubles = 8 * (size_t)N + ((size_t)N + 1) / 2;
    std::vector<double> in(in_doubles);                          // h | Si | z | matched: one copy
    if (N > 0) {
        if (!c->ov_in) HIPCHK(c, srukf_dmalloc((void**)&c->ov_in, sizeof(double) * in_doubles));
        if (!c->ov_rec) HIPCHK(c, srukf_dmalloc(&c->ov_rec, overlay_rec_bytes(N)));
        memcpy(in.data(), h, sizeof(double) * 2 * N); memcpy(in.data() + 2 * (size_t)N, Si, sizeof(double) * 4 * N);
        memcpy(in.data() + 6 * (size_t)N, z, sizeof(double) * 2 * N); memcpy(in.data() + 8 * (size_t)N, matched, sizeof(int) * N);
        HIPCHK(c, hipMemcpyAsync(c->ov_in, in.data(), sizeof(double) * in_doubles, hipMemcpyHostToDevice, c->stream));
    }
    {
        ProfScope ps(c, KC_OVERLAY, 0, (c->bgr_valid ? 6.0 : 4.0) * npix);
        const double* d = c->ov_in;
        launch_overlay(c->stream, W, H, N, d, d + 2 * (size_t)N, d + 6 * (size_t)N, (const int*)(d + 8 * (size_t)N), c->ov_rec,
                       c->bgr_valid ? c->d_bgr : nullptr, c->d_image, c->d_ovl);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_bgr, c->d_ovl, 3 * (size_t)npix, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                  // (in and out_bgr are pageable host memory)
    return SRUKF_OK;
}

}  // extern "C"
