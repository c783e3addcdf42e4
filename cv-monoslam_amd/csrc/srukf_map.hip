// srukf_map.hip — map changes on the device (srukf_add_landmarks: integrateFeaturesInformation, SLAM.cpp:818-871; srukf_delete_landmark: deleteOneFeature, 2637-2668;
// srukf_insert_landmarks / srukf_get_landmark_record: loop points, 948-1015 and 1357-1378)
// and data association (wrapPatch + dataAssociation, 1803-2009).  A map change swaps the map-size scope behind the handle (adopt_context).

#include "srukf_ctx.h"
#include <chrono>
#include <cmath>
using namespace srukf_impl;

// srukf_debug_set(0, "timing", 1): wall time of the phases of a map change on stderr (measurement: where do the milliseconds of srukf_add_landmarks /
// srukf_delete_landmark go — the device work or the context that is rebuilt around it?)
namespace {
struct MapTimer {
    bool on; const char* what; std::chrono::steady_clock::time_point t0, tl; std::string line;
    explicit MapTimer(const char* w) : on(g_sw.timing.load() != 0), what(w), t0(std::chrono::steady_clock::now()), tl(t0) {}
    void mark(const char* label) {
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        char b[64]; snprintf(b, sizeof b, " %s %.0f", label, std::chrono::duration<double, std::micro>(t - tl).count()); line += b; tl = t;
    }
    ~MapTimer() { if (on) fprintf(stderr, "[map timing] %s: total %.0f us:%s\n", what, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), line.c_str()); }
};
}

namespace srukf_impl {
int ensure_appearance(srukf_ctx* c)
{
    int rc = ensure_image(c); if (rc) return rc;               // (the frame buffer is the handle scope's, the records are per map size: either may exist without the other)
    if (c->app_patch) return SRUKF_OK;
    const size_t N = c->d.N > 0 ? c->d.N : 1;
    HIPCHK(c, srukf_dmalloc((void**)&c->app_patch, N * PT_PATCH_STRIDE));
    HIPCHK(c, srukf_dmalloc((void**)&c->app_tmpl, N * PT_TMPL_STRIDE));
    HIPCHK(c, srukf_dmalloc((void**)&c->appR, sizeof(double) * 9 * N));
    HIPCHK(c, srukf_dmalloc((void**)&c->appT, sizeof(double) * 3 * N));
    HIPCHK(c, srukf_dmalloc((void**)&c->appPx, sizeof(double) * 2 * N));
    HIPCHK(c, srukf_dmalloc((void**)&c->corr, sizeof(double) * N));
    HIPCHK(c, srukf_dmalloc((void**)&c->has_app, sizeof(int) * N));
    HIPCHK(c, hipMemsetAsync(c->app_patch, 0, N * PT_PATCH_STRIDE, c->stream));
    HIPCHK(c, hipMemsetAsync(c->app_tmpl, 0, N * PT_TMPL_STRIDE, c->stream));
    HIPCHK(c, hipMemsetAsync(c->has_app, 0, sizeof(int) * N, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SRUKF_OK;
}
}  // namespace srukf_impl

// the appearance records of landmarks `from` .. `from + count - 1` of `a` become the ones of landmarks `to` .. of `b` (map changes)
static void copy_appearance(srukf_ctx* a, int from, srukf_ctx* b, int to, int count = 1)
{
    if (count < 1) return;
    const size_t ps = PT_PATCH_STRIDE, ts = PT_TMPL_STRIDE, m = (size_t)count;
    hipMemcpyAsync(b->app_patch + to * ps, a->app_patch + from * ps, ps * m, hipMemcpyDeviceToDevice, b->stream);
    hipMemcpyAsync(b->app_tmpl + to * ts, a->app_tmpl + from * ts, ts * m, hipMemcpyDeviceToDevice, b->stream);
    hipMemcpyAsync(b->appR + 9 * to, a->appR + 9 * from, sizeof(double) * 9 * m, hipMemcpyDeviceToDevice, b->stream);
    hipMemcpyAsync(b->appT + 3 * to, a->appT + 3 * from, sizeof(double) * 3 * m, hipMemcpyDeviceToDevice, b->stream);
    hipMemcpyAsync(b->appPx + 2 * to, a->appPx + 2 * from, sizeof(double) * 2 * m, hipMemcpyDeviceToDevice, b->stream);
    hipMemcpyAsync(b->has_app + to, a->has_app + from, sizeof(int) * m, hipMemcpyDeviceToDevice, b->stream);
}

// no appearance record for landmarks `to` .. `to + count - 1` of `b`: has_app = 0, every field zeroed (a revived context holds a past life's records there)
static void clear_appearance(srukf_ctx* b, int to, int count)
{
    if (count < 1) return;
    const size_t ps = PT_PATCH_STRIDE, ts = PT_TMPL_STRIDE, m = (size_t)count;
    hipMemsetAsync(b->app_patch + to * ps, 0, ps * m, b->stream);
    hipMemsetAsync(b->app_tmpl + to * ts, 0, ts * m, b->stream);
    hipMemsetAsync(b->appR + 9 * to, 0, sizeof(double) * 9 * m, b->stream);
    hipMemsetAsync(b->appT + 3 * to, 0, sizeof(double) * 3 * m, b->stream);
    hipMemsetAsync(b->appPx + 2 * to, 0, sizeof(double) * 2 * m, b->stream);
    hipMemsetAsync(b->has_app + to, 0, sizeof(int) * m, b->stream);
}

// k_appearance_gather: landmark src_of[a]'s appearance record of one scope becomes landmark a's of another (a map change moves every kept record in one launch; six
// copies per landmark before).  One workgroup (one wave) per destination landmark: lanes 0 .. 27 the initPatch, 28 .. 47 the matchPatch, 16 bytes each (the strides
// are multiples of 16 and the arrays start at an allocation), lanes 48 .. 62 the fifteen scalars.  Pure copies; no workgroup reads what another one writes
constexpr int AG_PATCH_V = PT_PATCH_STRIDE / 16, AG_TMPL_V = PT_TMPL_STRIDE / 16, AG_SCALARS = AG_PATCH_V + AG_TMPL_V;
static_assert(PT_PATCH_STRIDE % 16 == 0 && PT_TMPL_STRIDE % 16 == 0 && AG_SCALARS + 15 <= 64, "one wave moves a record in 16-byte accesses");
__global__ __launch_bounds__(64) void k_appearance_gather(int M, const int* __restrict__ src_of, AppearanceArrays src, AppearanceArrays dst)
{
    const int a = blockIdx.x, t = threadIdx.x;
    if (a >= M) return;
    const size_t k = (size_t)src_of[a];
    if (t < AG_PATCH_V) ((uint4*)(dst.patch + (size_t)a * PT_PATCH_STRIDE))[t] = ((const uint4*)(src.patch + k * PT_PATCH_STRIDE))[t];
    else if (t < AG_SCALARS) ((uint4*)(dst.tmpl + (size_t)a * PT_TMPL_STRIDE))[t - AG_PATCH_V] = ((const uint4*)(src.tmpl + k * PT_TMPL_STRIDE))[t - AG_PATCH_V];
    else if (t < AG_SCALARS + 9) dst.R[9 * (size_t)a + (t - AG_SCALARS)] = src.R[9 * k + (t - AG_SCALARS)];
    else if (t < AG_SCALARS + 12) dst.T[3 * (size_t)a + (t - AG_SCALARS - 9)] = src.T[3 * k + (t - AG_SCALARS - 9)];
    else if (t < AG_SCALARS + 14) dst.px[2 * (size_t)a + (t - AG_SCALARS - 12)] = src.px[2 * k + (t - AG_SCALARS - 12)];
    else if (t == AG_SCALARS + 14) dst.has[a] = src.has[k];
}

void launch_appearance_gather(hipStream_t st, int M, const int* src_of, AppearanceArrays src, AppearanceArrays dst)
{
    if (M > 0) hipLaunchKernelGGL(k_appearance_gather, dim3(M), dim3(64), 0, st, M, src_of, src, dst);
}

static AppearanceArrays appearance_arrays(srukf_ctx* c) { return { c->app_patch, c->app_tmpl, c->appR, c->appT, c->appPx, c->has_app }; }

namespace srukf_impl {

void match_drop(srukf_ctx* c)
{
    if (c->match_res) srukf_dfree_on(c->match_res, c->stream);
    if (c->match_scores) srukf_dfree_on(c->match_scores, c->stream);
    c->match_res = nullptr; c->match_scores = nullptr; c->match_valid = false;
}

int match_ensure(srukf_ctx* c, const char* who)
{
    if (c->match_res) return SRUKF_OK;
    const int N = c->d.N;
    if (srukf_dmalloc(&c->match_res, sizeof(double) * match_res(N).doubles) != hipSuccess || srukf_dmalloc(&c->match_scores, sizeof(double) * PT_SCORE_STRIDE * (size_t)N) != hipSuccess) {
        (void)hipGetLastError(); match_drop(c); c->err = std::string(who) + ": out of device memory"; return SRUKF_ERR_NOMEM;
    }
    return SRUKF_OK;
}

// The handle keeps its identity when the map changes size: the map-size scope of the context built for the new size comes in, the handle's own goes out with c2
// and is retired.  Nothing of the handle scope moves ("who owns what across a map change"); what is written out below is neither "stays" nor "goes".
void adopt_context(srukf_ctx* c, srukf_ctx* c2)
{
    prof_collect(c);                                             // (the events pending on the handle were recorded around launches on the scope that leaves)
    std::swap(static_cast<srukf_map_scope&>(*c), static_cast<srukf_map_scope&>(*c2));
    std::swap(c->err, c2->err);                                  // (the text is the map change's: what its factorisation on c2 left, empty when nothing was abandoned)
    const int shared = c2->gmw_shared, tenants = c2->shared_tenants;      // (sharing the GPU is the handle's choice, the plans built for it are per map size: below)
    match_drop(c2);                                              // (the score maps of srukf_associate_checked go with the map they were made for)
    images_drop(c2, c2->stream);                                 // (and the staged images: the scope that comes in has no staged sequence either)
    ctx_retire(c, c2);                                           // (not destroyed: revived when the map has this size again — ctx_obtain)
    c->phase = 0; c->frame_updated = false;                      // (whatever call sequence the numeric part ran on the new scope: the handle is between frames)
    if (shared != c->gmw_shared) set_shared(c, shared, tenants);
}

}  // namespace srukf_impl

extern "C" {

// PointsMap::initPatch / initRotation / initTrans / initPixel as set at creation (SLAM.cpp:920-925): patch = the
// PT_PATCH_W^2 = 21 x 21 gray window image(Rect(round(u) - 10, round(v) - 10, 21, 21)), row-major as cv::Mat;
// R = Rwc (3x3 row-major), t = camera position, px = the distorted pixel.  matchPatch is zeroed (926).
int srukf_set_landmark_appearance(srukf_ctx* c, int k, const unsigned char* patch, const double R[9], const double t[3], const double px[2])
{
    if (!c || !patch || !R || !t || !px || k < 0 || k >= c->d.N) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_appearance(c); if (rc) return rc;
    const int one = 1;
    c->img.ck_clean = false;                                             // (a matchPatch is written: srukf_images_rewind)
    HIPCHK(c, hipMemcpy(c->app_patch + (size_t)k * PT_PATCH_STRIDE, patch, PT_PATCH_BYTES, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->app_tmpl + (size_t)k * PT_TMPL_STRIDE, 0, PT_TMPL_STRIDE));
    HIPCHK(c, hipMemcpy(c->appR + 9 * k, R, sizeof(double) * 9, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->appT + 3 * k, t, sizeof(double) * 3, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->appPx + 2 * k, px, sizeof(double) * 2, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->has_app + k, &one, sizeof(int), hipMemcpyHostToDevice));
    return SRUKF_OK;
}

// integrateFeaturesInformation's appearance fields (SLAM.cpp:918-926) of landmarks first .. first + K - 1 cut on the device from `gray` (NULL: the
// frame the handle holds): what srukf_set_landmark_appearance records for a host-cut initPatch at cvRound(uv), Rwc of the current heading and the
// robot position, byte for byte.
int srukf_capture_appearance(srukf_ctx* c, int first, int K, const double* uv, const unsigned char* gray)
{
    if (!c || !uv || K < 1 || first < 0 || first + K > c->d.N) return SRUKF_ERR_BAD_ARG;
    const int W = (int)c->p.image_w, H = (int)c->p.image_h;
    for (int q = 0; q < K; q++) {                                        // the 21 x 21 window must lie inside the frame
        if (!(std::fabs(uv[2 * q]) < 1e9) || !(std::fabs(uv[2 * q + 1]) < 1e9)) { c->err = "capture_appearance: pixel is not finite"; return SRUKF_ERR_BAD_ARG; }
        const int u = (int)std::nearbyint(uv[2 * q]), v = (int)std::nearbyint(uv[2 * q + 1]);
        if (u - PT_INIT_HALF < 0 || u + PT_INIT_HALF > W - 1 || v - PT_INIT_HALF < 0 || v + PT_INIT_HALF > H - 1) { c->err = "capture_appearance: the 21 x 21 window leaves the image"; return SRUKF_ERR_BAD_ARG; }
    }
    HIPCHK(c, hipSetDevice(c->device));
    step_commit_motion(c);
    c->img.ck_clean = false;                                             // (matchPatches are written: srukf_images_rewind)
    int rc = ensure_appearance(c); if (rc) return rc;
    rc = take_frame(c, gray); if (rc) return rc;
    double* d_uv = nullptr;
    HIPCHK(c, srukf_dmalloc_on(&d_uv, sizeof(double) * 2 * K, c->stream));
    hipError_t e = hipMemcpyAsync(d_uv, uv, sizeof(double) * 2 * K, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        ProfScope ps(c, KC_CAPTURE, 0, (double)PT_PATCH_BYTES * K);
        launch_capture_patch(c->stream, c->d_image, W, first, K, d_uv, c->X, c->d.n, c->app_patch, c->app_tmpl, c->appR, c->appT, c->appPx, c->has_app);
        e = hipGetLastError();
    }
    srukf_dfree_on(d_uv, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { c->err = std::string("capture_appearance: ") + hipGetErrorString(e); return SRUKF_ERR_HIP; }
    return SRUKF_OK;
}

int srukf_get_match_patch(srukf_ctx* c, int k, unsigned char* out)
{
    if (!c || !out || k < 0 || k >= c->d.N) return SRUKF_ERR_BAD_ARG;
    if (!c->app_tmpl) { c->err = "get_match_patch: no appearance records"; return SRUKF_ERR_SEQUENCE; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->app_tmpl + (size_t)k * PT_TMPL_STRIDE, PT_TMPL_BYTES, hipMemcpyDeviceToHost));
    return SRUKF_OK;
}

// wrapPatch + dataAssociation (SLAM.cpp:1803-2009) between srukf_predict_measurement and srukf_update: gray = the
// image_h x image_w frame (row-major uchar).  Out (host, any may be NULL): z[2N] = matchLocation, matched[N] =
// isMatching, corr[N] = best normalised cross correlation.  Landmarks without an appearance record never match.
// (gray == NULL: the frame the handle holds, no upload — srukf_associate_held, which has checked that there is one)
// chk != NULL: srukf_associate_checked — the same launches with k_associate_checked (srukf_unique.hip) in k_associate's place, its seven result arrays in one export
static int associate_frame(srukf_ctx* c, const unsigned char* gray, double* z, int* matched, double* corr,
                           const srukf_match_params* chk = nullptr, double* corr2 = nullptr, double* z2 = nullptr, int* flags = nullptr)
{
    if (c->phase < 2) { c->err = "associate before predict_measurement"; return SRUKF_ERR_SEQUENCE; }
    const int N = c->d.N;
    if (N == 0) return SRUKF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_appearance(c); if (rc) return rc;
    if (chk) { rc = match_ensure(c, "associate_checked"); if (rc) return rc; }
    const size_t img = (size_t)c->p.image_w * c->p.image_h;
    const size_t mp = c->d.mp, zm = mp + ((size_t)N + 1) / 2;             // zcur | mcur: one device allocation of zm doubles
    const size_t res_doubles = chk ? match_res(N).doubles : zm + (size_t)N;      // what the export writes to the front of the staging buffer: match_res, or zcur | mcur | corr
    // What does not need the frame goes out first — the warp uses the PREDICTED robot pose (wrapPatch reads m_X_k after predictMotion, SLAM.cpp:1812-1830) — and runs while
    // the host copies the frame into pinned memory: a hipMemcpyAsync from the caller's pageable buffer is staged by the runtime, synchronously, in front of everything.
    step_commit_motion(c);
    c->img.ck_clean = false;                                             // (the warp writes every matchPatch: srukf_images_rewind)
    double* dxyz = c->G;                                                 // G is free outside the refactorisation
    srukf_launch_landmarks_cartesian(c->stream, c->d, c->X, c->S, dxyz, nullptr);                           // PointsMap::xyz (2574): the points only, no covariances
    srukf_launch_warp_patch(c->stream, c->d, c->p, c->X, dxyz, c->h, c->appR, c->appT, c->appPx, c->app_patch, c->has_app, c->app_tmpl);
    double* hs = c->hstage;
    const size_t img_off = (res_doubles + 7) & ~(size_t)7;              // (doubles) behind the results' place in the staging buffer
    if (!gray) {
    } else if ((img_off + (img + 7) / 8) * sizeof(double) <= c->hstage_bytes) {
        unsigned char* himg = (unsigned char*)(hs + img_off);
        memcpy(himg, gray, img);
        HIPCHK(c, hipMemcpyAsync(c->d_image, himg, img, hipMemcpyHostToDevice, c->stream));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->d_image, gray, img, hipMemcpyHostToDevice, c->stream));
    }
    if (gray) { c->frame_valid = true; c->bgr_valid = false; }
    if (chk) {
        ProfScope ps(c, KC_ASSOC_CHECKED, 0, (double)(PT_REGION_W * PT_REGION_W + PT_TMPL_BYTES + 8 * PT_SCORE_STRIDE) * N);
        const MatchArgs ma = { .corr_threshold = chk->corr_threshold, .ratio = chk->ratio, .exclusion = chk->exclusion, .subpixel = chk->subpixel };
        srukf_launch_associate_checked(c->stream, c->d, c->p, ma, c->d_image, c->h, c->Si, c->vis, c->has_app, c->app_tmpl, c->zcur, c->mcur, c->corr, c->match_res,
                                       c->match_scores);
        c->match_valid = true;
    } else
    srukf_launch_associate(c->stream, c->d, c->p, c->d_image, c->h, c->Si, c->vis, c->has_app, c->app_tmpl, c->zcur, c->mcur, c->corr);
    // z | matched | corr written into the pinned buffer by ONE short launch, flag behind them: three small device-to-host copies were three blit kernels with their gaps
    const unsigned long long seq = ++c->step_seq;
    if (chk) launch_export(c->stream, c->match_res, sizeof(double) * match_res(N).doubles, nullptr, 0, hs, c->dbg.step_spin ? step_flag(c) : nullptr, seq);
    else launch_export(c->stream, c->zcur, sizeof(double) * zm, c->corr, sizeof(double) * N, hs, c->dbg.step_spin ? step_flag(c) : nullptr, seq);
    rc = step_wait_export(c, seq); if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    if (chk) {
        const MatchRes at = match_res(N);
        const int* hm = (const int*)(hs + at.matched);
        if (z) memcpy(z, hs + at.z, sizeof(double) * 2 * N);
        if (corr) memcpy(corr, hs + at.corr, sizeof(double) * N);
        if (corr2) memcpy(corr2, hs + at.corr2, sizeof(double) * N);
        if (z2) memcpy(z2, hs + at.z2, sizeof(double) * 2 * N);
        if (matched) memcpy(matched, hm, sizeof(int) * N);
        if (flags) memcpy(flags, hm + at.flags_ints, sizeof(int) * N);
        return SRUKF_OK;
    }
    if (z) memcpy(z, hs, sizeof(double) * 2 * N);
    if (matched) memcpy(matched, hs + mp, sizeof(int) * N);
    if (corr) memcpy(corr, hs + zm, sizeof(double) * N);
    return SRUKF_OK;
}

int srukf_associate(srukf_ctx* c, const unsigned char* gray, double* z, int* matched, double* corr)
{
    if (!c || !gray) return SRUKF_ERR_BAD_ARG;
    return associate_frame(c, gray, z, matched, corr);
}

// srukf_associate on the frame the handle holds (loadPictures ran before: srukf_set_frame_bgr, or any call that brought a gray frame): no upload
int srukf_associate_held(srukf_ctx* c, double* z, int* matched, double* corr)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (c->phase < 2) { c->err = "associate before predict_measurement"; return SRUKF_ERR_SEQUENCE; }
    if (!c->frame_valid || !c->d_image) { c->err = "associate_held: no frame held"; return SRUKF_ERR_SEQUENCE; }
    return associate_frame(c, nullptr, z, matched, corr);
}

// srukf_associate / srukf_associate_held with the score map kept (srukf_unique.hip): the same phase rule and the same launches, k_associate_checked
// in k_associate's place, one export, one wait.  matchPatch evolves identically whichever call a frame uses
int srukf_associate_checked(srukf_ctx* c, const unsigned char* gray, const srukf_match_params* params, double* z, int* matched, double* corr, double* corr2, double* z2, int* flags)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    srukf_match_params mp = { 0.8, 0.9, 4, 0 };
    if (params) mp = *params;
    if (!std::isfinite(mp.ratio) || mp.ratio <= 0.0) { c->err = "associate_checked: ratio must be finite and positive"; return SRUKF_ERR_BAD_ARG; }
    if (mp.exclusion < 1 || mp.exclusion > 20) { c->err = "associate_checked: exclusion outside [1, 20]"; return SRUKF_ERR_BAD_ARG; }
    if (!std::isfinite(mp.corr_threshold)) { c->err = "associate_checked: corr_threshold is not finite"; return SRUKF_ERR_BAD_ARG; }
    if (c->phase < 2) { c->err = "associate before predict_measurement"; return SRUKF_ERR_SEQUENCE; }
    if (!gray && (!c->frame_valid || !c->d_image)) { c->err = "associate_checked: no frame held"; return SRUKF_ERR_SEQUENCE; }
    return associate_frame(c, gray, z, matched, corr, &mp, corr2, z2, flags);
}

// the score map the last srukf_associate_checked left for landmark k: out[wx * wy] row-major, (x0, y0) = the pixel of the window's top-left candidate centre
int srukf_get_match_scores(srukf_ctx* c, int k, double out[PT_SCORE_W * PT_SCORE_W], int* wx, int* wy, int* x0, int* y0)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (!c->match_valid || !c->match_scores) { c->err = "get_match_scores: no checked association since the last map change or reset"; return SRUKF_ERR_SEQUENCE; }
    if (k < 0 || k >= c->d.N) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double buf[PT_SCORE_STRIDE];
    HIPCHK(c, hipMemcpy(buf, c->match_scores + (size_t)k * PT_SCORE_STRIDE, sizeof buf, hipMemcpyDeviceToHost));
    const int w = (int)buf[PT_SCORE_WX], hgt = (int)buf[PT_SCORE_WY];
    if (w < 0 || hgt < 0 || w * hgt > PT_SCORE_W * PT_SCORE_W) { c->err = "get_match_scores: corrupt window"; return SRUKF_ERR_HIP; }
    if (out) memcpy(out, buf, sizeof(double) * (size_t)(w * hgt));
    if (wx) *wx = w; if (wy) *wy = hgt; if (x0) *x0 = (int)buf[PT_SCORE_X0]; if (y0) *y0 = (int)buf[PT_SCORE_Y0];
    return SRUKF_OK;
}

}  // extern "C"

// ---- what the map changes share around their numeric parts ---------------------------------------------------------------------------------------
// begin: the frame in flight is committed, the fast path's chain ends, the stream is idle, c2 is a context for N2 landmarks (ctx_obtain).  From here to
// map_change_finish the handle is untouched: a failure ends in map_change_fail (the caller frees its temporaries first).
static int map_change_begin(srukf_ctx* c, MapTimer& mt, int N2, srukf_ctx** c2)
{
    step_commit_motion(c); step_invalidate(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    mt.mark("sync");
    const int rc = ctx_obtain(c, c2, N2);
    if (rc) { c->err = std::string(mt.what) + ": " + g_create_error; return rc; }
    mt.mark("create");
    return SRUKF_OK;
}

static int map_change_fail(srukf_ctx* c, srukf_ctx* c2, int rc, std::string text)
{
    srukf_destroy(c2);
    c->err = std::move(text);
    return rc;
}
static int map_change_fail(srukf_ctx* c, srukf_ctx* c2, const MapTimer& mt, hipError_t e) { return map_change_fail(c, c2, SRUKF_ERR_HIP, std::string(mt.what) + ": " + hipGetErrorString(e)); }

// the n2 x n2 matrix src (leading dimension lds), its rows and columns taken in the order d_map names, factored into c2->S: on the fast path, and again on the exact
// path if a row was clamped.  zero_fast: S is cleared in front of the fast pass too (the exact pass always starts from zeros)
static int map_change_factor(srukf_ctx* c, srukf_ctx* c2, int n2, const double* src, int lds, const int* d_map, bool zero_fast)
{
    const int ldn = c2->d.np;
    for (int slow = 0; slow < 2; slow++) {
        launch_set_run(c->stream, c2->fs, 0, 1, nullptr);
        launch_refactor_reset(c->stream, ldn, c2->theta, c2->fs, 1);
        launch_sym_permute(c->stream, n2, ldn, src, lds, c2->Gbak, d_map);
        srukf_launch_gmw_stats(c->stream, n2, ldn, c2->Gbak, c2->fs);
        if (slow || zero_fast) hipMemsetAsync(c2->S, 0, sizeof(double) * (size_t)ldn * ldn, c->stream);
        run_gmw(c2, c2->Gbak, c2->S, slow != 0);
        if (slow) break;
        const int rc = read_fs(c2);
        if (rc) return rc;
        if (c2->hfs->clamp_rows == 0) break;
    }
    return SRUKF_OK;
}

// finish: c2's map-size scope becomes the handle's (adopt_context), in the handle's storage mode, with its null set, and with k_new landmarks armed for NEED_REORDER
static int map_change_finish(srukf_ctx* c, srukf_ctx* c2, MapTimer& mt, int k_new)
{
    const int storage = c->storage;                              // (per map size, F64 in a context just obtained; the mode itself is the caller's)
    mt.mark("appearance");
    adopt_context(c, c2);
    mt.mark("adopt+destroy");
    int rc = srukf_set_storage(c, storage); if (rc) return rc;
    mt.mark("set_storage");
    rc = update_null_set(c); if (rc) return rc;
    canonicalize_null_rows(c);
    mt.mark("null_set");
    return srukf_set_new_landmarks(c, k_new);
}

extern "C" {

// integrateFeaturesInformation, numeric part (SLAM.cpp:826-871): K new landmarks at the distorted pixels uv[K][2] are
// appended to the map (normal order: before the robot block).  The context is rebuilt for N + K landmarks in place
// (the handle stays valid; staged sequences and captured graphs are dropped) and K_new = K is armed for the
// FLAG_4_NEED_REORDER update that follows (SLAM.cpp:2083-2090).  See srukf_augment.hip.
int srukf_add_landmarks(srukf_ctx* c, int K, const double* uv)
{
    if (!c || K < 1 || !uv) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    MapTimer mt("add_landmarks");
    const int dim = c->d.n, ld = c->d.np;
    const int Na = dim + 3 * K, L = 2 * Na + 1, dimn = dim + 6 * K;                          // 827-828
    srukf_ctx* c2 = nullptr;
    int rc = map_change_begin(c, mt, c->d.N + K, &c2); if (rc) return rc;
    const int ldn = c2->d.np, rows_p = round_up(2 * Na, 16);
    KWeights wa; host_weights(Na, c->p, wa);                                                 // 867
    std::vector<int> perm(dimn);
    {   // getPermutationMatrix, 1303-1334 (dim = new dimension)
        const int dimOld = dimn - 6 * K;
        for (int i = 0; i < dimOld - 4; i++) perm[i] = i;
        for (int e = 0; e < 4; e++) perm[dimn - 4 + e] = dimOld - 4 + e;
        for (int id = 0; id < K; id++) {
            for (int e = 0; e < 3; e++) perm[dimOld - 4 + 6 * id + e] = dimOld + 3 * K + 3 * id + e;
            for (int e = 0; e < 3; e++) perm[dimOld - 4 + 6 * id + 3 + e] = dimOld + 3 * id + e;
        }
    }
    double *d_uv = nullptr, *d_ang = nullptr, *d_A = nullptr, *d_mu = nullptr; int* d_perm = nullptr;
    auto cleanup = [&]() { for (void* b : { (void*)d_uv, (void*)d_ang, (void*)d_A, (void*)d_mu, (void*)d_perm }) if (b) srukf_dfree(b); };
    if (srukf_dmalloc((void**)&d_uv, sizeof(double) * 2 * K) != hipSuccess || srukf_dmalloc((void**)&d_ang, sizeof(double) * (size_t)L * 3 * K) != hipSuccess ||
        srukf_dmalloc((void**)&d_A, sizeof(double) * (size_t)rows_p * ldn) != hipSuccess || srukf_dmalloc((void**)&d_mu, sizeof(double) * 3 * K) != hipSuccess ||
        srukf_dmalloc((void**)&d_perm, sizeof(int) * dimn) != hipSuccess) {
        cleanup(); return map_change_fail(c, c2, SRUKF_ERR_NOMEM, "add_landmarks: out of device memory");
    }
    hipMemcpyAsync(d_uv, uv, sizeof(double) * 2 * K, hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(d_perm, perm.data(), sizeof(int) * dimn, hipMemcpyHostToDevice, c->stream);
    hipStreamSynchronize(c->stream);                                                         // uv / perm are pageable host memory
    srukf_launch_aug_map(c->stream, c->p, dim, ld, K, Na, wa.gamma, c->X, c->S, d_uv, d_ang);
    srukf_launch_aug_x(c->stream, dim, K, Na, wa.wm0, wa.wi, c->X, d_ang, d_perm, d_mu, c2->X, dimn, ldn);
    srukf_launch_aug_build(c->stream, dim, ld, K, Na, wa.gamma, wa.wi_sr, c->X, c->S, d_ang, d_A, rows_p, dimn, ldn);
    srukf_launch_gram(c->stream, rows_p, ldn, d_A, c2->G);                                   // A^T A, disordered layout
    rc = map_change_factor(c, c2, dimn, c2->G, ldn, d_perm, false);                          // Pi (A^T A) Pi^T
    if (rc) { cleanup(); return map_change_fail(c, c2, rc, c2->err); }
    hipError_t e = hipStreamSynchronize(c->stream);
    cleanup();
    mt.mark("numeric");
    if (e != hipSuccess) return map_change_fail(c, c2, mt, e);
    if (c->app_patch) {                                      // the old landmarks keep their appearance records
        rc = ensure_appearance(c2);
        if (rc) return map_change_fail(c, c2, rc, c2->err);
        int* d_src = nullptr;                                // the identity table: the same launch a deletion issues with its keep table
        std::vector<int> ident(c->d.N);
        for (int k = 0; k < c->d.N; k++) ident[k] = k;
        if (c->d.N > 0 && srukf_dmalloc((void**)&d_src, sizeof(int) * c->d.N) != hipSuccess) return map_change_fail(c, c2, SRUKF_ERR_NOMEM, "add_landmarks: out of device memory");
        if (d_src) hipMemcpy(d_src, ident.data(), sizeof(int) * c->d.N, hipMemcpyHostToDevice);
        launch_appearance_gather(c->stream, c->d.N, d_src, appearance_arrays(c), appearance_arrays(c2));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (d_src) srukf_dfree(d_src);
        if (e != hipSuccess) return map_change_fail(c, c2, mt, e);
    }
    return map_change_finish(c, c2, mt, K);
}

// deleteOneFeature, numeric part (SLAM.cpp:2637-2668): a landmark (0-based, state order) leaves the state.  The
// reference drops its 6 rows and columns from S and folds the 6 removed rows V back in with six
// S <- gmw(S^T S + v v^T); the sum of those is the remaining block of P = S^T S, so the device takes S^T S
// (k_syrk), compacts it and factors it once (the batched form of the six updates, as in srukf_update).  K deletions in any order rebuild the same remaining block,
// P[keep, keep]: K landmarks leave in one pass of the same launches with the keep map of all of them.
// rec != NULL: the records of the K landmarks (srukf_get_landmark_record's, in the order of ids) are taken before anything moves — one launch, one copy.
}  // extern "C"

namespace {
struct LmRecordsOut { double* X6; double* S66; unsigned char* patch; double* R; double* t; double* px; int* has_app; };
}

// one record of k_lm_record's staging block into the caller's arrays at entry q
static void unpack_lm_record(const double* h, const LmRecordsOut& o, size_t q)
{
    if (o.X6) memcpy(o.X6 + 6 * q, h, sizeof(double) * 6);
    if (o.S66) memcpy(o.S66 + 36 * q, h + 6, sizeof(double) * 36);
    if (o.R) memcpy(o.R + 9 * q, h + 42, sizeof(double) * 9);
    if (o.t) memcpy(o.t + 3 * q, h + 51, sizeof(double) * 3);
    if (o.px) memcpy(o.px + 2 * q, h + 54, sizeof(double) * 2);
    if (o.has_app) o.has_app[q] = h[LM_REC_DOUBLES - 1] != 0.0 ? 1 : 0;
    if (o.patch) memcpy(o.patch + (size_t)PT_PATCH_BYTES * q, h + LM_REC_DOUBLES, PT_PATCH_BYTES);
}

// the one body of srukf_delete_landmark (K = 1, no records) and srukf_delete_landmarks.  who: the call's name, in c->err and on the timing line
static int delete_landmarks_body(srukf_ctx* c, const char* who, int K, const int* ids, const LmRecordsOut* rec)
{
    const int N = c->d.N, n = c->d.n, np = c->d.np;
    std::vector<char> gone(N > 0 ? N : 1, 0);
    for (int q = 0; q < K; q++) {
        if (ids[q] < 0 || ids[q] >= N) { c->err = std::string(who) + ": no such landmark"; return SRUKF_ERR_BAD_ARG; }
        if (gone[ids[q]]) { c->err = std::string(who) + ": a landmark is named twice"; return SRUKF_ERR_BAD_ARG; }
        gone[ids[q]] = 1;
    }
    HIPCHK(c, hipSetDevice(c->device));
    MapTimer mt(who);
    srukf_ctx* c2 = nullptr;
    int rc = map_change_begin(c, mt, N - K, &c2); if (rc) return rc;
    const int N2 = N - K, nn = n - 6 * K, ldn = c2->d.np;
    // one table, one copy: the keep map of the state's rows [nn] | the kept landmarks' old positions [N2] | the landmarks that leave [K]
    std::vector<int> tab((size_t)nn + N2 + K);
    int k_new = c->K_new > 0 ? c->K_new : 0;                  // m_nFilters-- for each of the landmarks added last that goes (SLAM.cpp:2468-2492)
    for (int k = 0, a = 0; k < N; k++) {
        if (gone[k]) { if (k >= N - c->K_new && k_new > 0) k_new--; continue; }
        for (int e = 0; e < 6; e++) tab[6 * a + e] = 6 * k + e;
        tab[nn + a] = k; a++;
    }
    for (int e = 0; e < 4; e++) tab[6 * N2 + e] = 6 * N + e;  // the robot block
    for (int q = 0; q < K; q++) tab[(size_t)nn + N2 + q] = ids[q];
    int* d_map = nullptr;
    if (srukf_dmalloc((void**)&d_map, sizeof(int) * tab.size()) != hipSuccess) return map_change_fail(c, c2, SRUKF_ERR_NOMEM, std::string(who) + ": out of device memory");
    const int *d_src = d_map + nn, *d_ids = d_map + nn + N2;
    hipMemcpy(d_map, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice);
    // the records first: they read X, S and the appearance arrays of the scope that leaves, and G is free until k_syrk writes it (stream order)
    const size_t rec_bytes = sizeof(double) * SRUKF_LM_RECORD_DOUBLES * (size_t)K, scratch_bytes = rec_bytes + sizeof(double) * 36 * (size_t)K;      // records | the K blocks of P
    double* d_rec = nullptr; bool own_rec = false; std::vector<double> h_own; const double* h_rec = nullptr;
    if (rec) {
        if (scratch_bytes <= sizeof(double) * (size_t)np * np) d_rec = c->G;
        else if (srukf_dmalloc((void**)&d_rec, scratch_bytes) != hipSuccess) { srukf_dfree(d_map); return map_change_fail(c, c2, SRUKF_ERR_NOMEM, std::string(who) + ": out of device memory"); }
        else own_rec = true;
        double* h = c->hstage;
        if (rec_bytes > c->hstage_bytes) { h_own.resize(SRUKF_LM_RECORD_DOUBLES * (size_t)K); h = h_own.data(); }
        h_rec = h;
        launch_lm_records(c->stream, K, c->d, c->S, c->X, d_ids, c->p.epsilon, c->app_patch, c->appR, c->appT, c->appPx, c->has_app,
                          d_rec + SRUKF_LM_RECORD_DOUBLES * (size_t)K, d_rec);
        hipMemcpyAsync(h, d_rec, rec_bytes, hipMemcpyDeviceToHost, c->stream);
    }
    launch_refactor_reset(c->stream, np, c->theta, c->fs, 1);
    srukf_launch_syrk(c->stream, c->d, c->S, c->Ut, 0, 0, c->G, c->fs, c->syrk_tiles, c->n_syrk_tiles, SyrkRider{});   // P = S^T S
    launch_gather(c->stream, nn, ldn, c->X, c2->X, d_map);
    rc = map_change_factor(c, c2, nn, c->G, np, d_map, true);
    if (rc) { srukf_dfree(d_map); if (own_rec) srukf_dfree(d_rec); return map_change_fail(c, c2, rc, c2->err); }
    hipError_t e = hipStreamSynchronize(c->stream);
    if (own_rec) srukf_dfree(d_rec);
    mt.mark("numeric");
    if (e != hipSuccess) { srukf_dfree(d_map); return map_change_fail(c, c2, mt, e); }
    if (rec) for (int q = 0; q < K; q++) unpack_lm_record(h_rec + SRUKF_LM_RECORD_DOUBLES * (size_t)q, *rec, (size_t)q);
    if (c->app_patch) {                                      // the kept landmarks keep their appearance records: one launch
        rc = ensure_appearance(c2);
        if (rc) { srukf_dfree(d_map); return map_change_fail(c, c2, rc, c2->err); }
        launch_appearance_gather(c->stream, N2, d_src, appearance_arrays(c), appearance_arrays(c2));
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { srukf_dfree(d_map); return map_change_fail(c, c2, mt, e); }
    }
    srukf_dfree(d_map);
    return map_change_finish(c, c2, mt, k_new);
}

extern "C" {

int srukf_delete_landmark(srukf_ctx* c, int id)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    return delete_landmarks_body(c, "delete_landmark", 1, &id, nullptr);
}

// K landmarks leave together; the records of the ones that leave (any array may be NULL) arrive with the call.  See include/srukf.h
int srukf_delete_landmarks(srukf_ctx* c, int K, const int* ids, double* records_X6, double* records_S66, unsigned char* patches, double* R, double* t, double* px, int* has_app)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (K < 1 || !ids) { c->err = "delete_landmarks: K < 1 or no ids"; return SRUKF_ERR_BAD_ARG; }
    const LmRecordsOut rec = { records_X6, records_S66, patches, R, t, px, has_app };
    const bool any = records_X6 || records_S66 || patches || R || t || px || has_app;
    return delete_landmarks_body(c, "delete_landmarks", K, ids, any ? &rec : nullptr);
}

// What an archived landmark takes along (FeatureInfo, SLAM.cpp:1357-1378, 2516-2532): its six rows of X, the upper Cholesky factor of its marginal block
// P66 = (S^T S)[6k:6k+6, 6k:6k+6] (k_block_cov, then k_lm_record factors it in the order include/srukf.h states) and its appearance record, in one round trip.
int srukf_get_landmark_record(srukf_ctx* c, int k, double X6[6], double S66[36], unsigned char* patch, double R[9], double t[3], double px[2], int* has_app)
{
    if (!c || k < 0 || k >= c->d.N) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    step_commit_motion(c);
    double* dout = c->G;                                                 // G is scratch outside the refactorisation
    srukf_launch_block_cov(c->stream, c->d, c->S, 6 * k, 6, c->small, nullptr);
    launch_lm_record(c->stream, c->small, c->X, k, c->p.epsilon, c->app_patch, c->appR, c->appT, c->appPx, c->has_app, dout);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->hstage, dout, sizeof(double) * SRUKF_LM_RECORD_DOUBLES, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double* h = c->hstage;
    if (X6) memcpy(X6, h, sizeof(double) * 6);
    if (S66) memcpy(S66, h + 6, sizeof(double) * 36);
    if (R) memcpy(R, h + 42, sizeof(double) * 9);
    if (t) memcpy(t, h + 51, sizeof(double) * 3);
    if (px) memcpy(px, h + 54, sizeof(double) * 2);
    if (has_app) *has_app = h[LM_REC_DOUBLES - 1] != 0.0 ? 1 : 0;
    if (patch) memcpy(patch, h + LM_REC_DOUBLES, PT_PATCH_BYTES);
    return SRUKF_OK;
}

// integrateFeaturesInformation's loop points (SLAM.cpp:948-1015) with stated semantics: L landmarks with known means X6 and upper-triangular square-root blocks
// S66 and no cross-covariance enter the state at landmark positions [N - K_new, N - K_new + L), in front of the landmarks the last srukf_add_landmarks armed.
// X' and S' are copies (k_lm_insert): P' = Pi (P (+) S66_0^T S66_0 (+) ...) Pi^T.  The context is rebuilt for N + L landmarks in place as srukf_add_landmarks
// rebuilds it; K_new is kept.  The new slots get exactly the appearance record passed (patches NULL: none, whatever a revived context held there).
int srukf_insert_landmarks(srukf_ctx* c, int L, const double* X6, const double* S66, const unsigned char* patches, const double* R, const double* t, const double* px)
{
    if (!c || L < 1 || !X6 || !S66) return SRUKF_ERR_BAD_ARG;
    if (patches && (!R || !t || !px)) { c->err = "insert_landmarks: a patch needs R, t and px"; return SRUKF_ERR_BAD_ARG; }
    auto finite = [](const double* a, size_t m) { for (size_t i = 0; i < m; i++) if (!std::isfinite(a[i])) return false; return true; };
    if (!finite(X6, 6 * (size_t)L) || !finite(S66, 36 * (size_t)L) || (R && !finite(R, 9 * (size_t)L)) || (t && !finite(t, 3 * (size_t)L)) ||
        (px && !finite(px, 2 * (size_t)L))) { c->err = "insert_landmarks: an input is not finite"; return SRUKF_ERR_BAD_ARG; }
    for (int j = 0; j < L; j++)
        for (int a = 1; a < 6; a++)
            for (int b = 0; b < a; b++)
                if (S66[36 * (size_t)j + 6 * a + b] != 0.0) { c->err = "insert_landmarks: S66 is not upper triangular"; return SRUKF_ERR_BAD_ARG; }
    HIPCHK(c, hipSetDevice(c->device));
    MapTimer mt("insert_landmarks");
    const int N = c->d.N, k_new = c->K_new, p0 = N - k_new;
    srukf_ctx* c2 = nullptr;
    int rc = map_change_begin(c, mt, N + L, &c2); if (rc) return rc;
    double* d_blk = nullptr;
    if (srukf_dmalloc_on(&d_blk, sizeof(double) * 42 * (size_t)L, c->stream) != hipSuccess) return map_change_fail(c, c2, SRUKF_ERR_NOMEM, "insert_landmarks: out of device memory");
    hipError_t e = hipMemcpyAsync(d_blk, X6, sizeof(double) * 6 * (size_t)L, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blk + 6 * (size_t)L, S66, sizeof(double) * 36 * (size_t)L, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_lm_insert(c->stream, c->S, c->d.np, c->X, 6 * p0, L, d_blk, c2->S, c2->X, c2->d.n, c2->d.np);
        e = hipGetLastError();
    }
    srukf_dfree_on(d_blk, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    mt.mark("numeric");
    if (e != hipSuccess) return map_change_fail(c, c2, mt, e);
    if (c->app_patch || patches || c2->app_patch) {
        rc = ensure_appearance(c2);
        if (rc) return map_change_fail(c, c2, rc, c2->err);
        if (c->app_patch) {                                              // the old landmarks keep their records
            copy_appearance(c, 0, c2, 0, p0);
            copy_appearance(c, p0, c2, p0 + L, k_new);
        } else {
            clear_appearance(c2, 0, N + L);
        }
        if (patches) {
            std::vector<int> one(L, 1);
            e = hipMemcpy2DAsync(c2->app_patch + (size_t)p0 * PT_PATCH_STRIDE, PT_PATCH_STRIDE, patches, PT_PATCH_BYTES, PT_PATCH_BYTES, L, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemsetAsync(c2->app_tmpl + (size_t)p0 * PT_TMPL_STRIDE, 0, PT_TMPL_STRIDE * (size_t)L, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c2->appR + 9 * p0, R, sizeof(double) * 9 * (size_t)L, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c2->appT + 3 * p0, t, sizeof(double) * 3 * (size_t)L, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c2->appPx + 2 * p0, px, sizeof(double) * 2 * (size_t)L, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c2->has_app + p0, one.data(), sizeof(int) * (size_t)L, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);     // (pageable host memory)
        } else {
            clear_appearance(c2, p0, L);
            e = hipStreamSynchronize(c->stream);
        }
        if (e != hipSuccess) return map_change_fail(c, c2, mt, e);
    }
    return map_change_finish(c, c2, mt, k_new);
}

}  // extern "C"
