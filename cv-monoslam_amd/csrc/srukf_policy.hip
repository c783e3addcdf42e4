// srukf_policy.hip — the map policy's verdict on the device: the counters of predictMeasurement / KalmanUpdate (cslam.cpp:713-723, 751), the
// deletion tests of updateFeaturesInformation (cslam.cpp:446-462; SLAM.cpp:2443-2459) and the addFeatures trigger (SLAM.cpp:556), per landmark and per frame, from
// the posterior X and the frame's association.  Read-only for the filter: it writes the policy state, the verdicts and the summary, nothing else.
//   srukf_map_policy              step-wise: k_map_policy on the filter's current X with the caller's association
//   srukf_images_policy           the switch of the image runs: k_map_policy_staged behind every frame (issue_image_policy: srukf_images.hip)
//   srukf_images_set_policy_state / srukf_get_image_policy / srukf_images_rewind: srukf_images.hip
// One workgroup of 256 threads, landmarks strided over the threads; the four counts are reduced by wave shuffles and through LDS.  No atomics, no flags: every
// dependency is a launch boundary on the stream.  gfx950 only.
#include "srukf_ctx.h"
using namespace srukf_impl;

// what one launch reads and writes: X (n entries, landmark k at 6k, the robot block last), this frame's h [2N], visible [N], z [2N], matched [N]; the state [N],
// the verdicts [N] and the summary
struct PolicyIO {
    const double* X; const double* h; const int* vis; const double* z; const int* m;
    srukf_policy_state* st; int* verdict; srukf_policy_summary* sum;
};

// The one text of the policy.  Verdicts are per landmark and independent (the reference's list walk skips the node that slides into a deleted position,
// cslam.cpp:475-481: that only happens in a frame that has a deletion already, so `change` is exact without it)
__device__ __forceinline__ void map_policy_body(int N, int n, double W, double H, const srukf_policy_params prm, const PolicyIO io)
{
    __shared__ int red[4][4];
    const int tid = threadIdx.x;
    int cnt[4] = { 0, 0, 0, 0 };                               // visible, matched, deleted, stored
    const double zr = io.X[n - 2];
    for (int k = tid; k < N; k += 256) {
        srukf_policy_state s = io.st[k];
        const int v = io.vis[k] != 0, mt = io.m[k] != 0;
        if (v) { s.nPredictTimes++; s.predictLocation[0] = io.h[2 * k]; s.predictLocation[1] = io.h[2 * k + 1]; }      // cslam.cpp:716-720 (invisible: the last value stays)
        if (mt) s.nMatchTimes++;                                                                                           // cslam.cpp:751
        io.st[k] = s;
        const double zi = io.X[6 * k + 2], theta = io.X[6 * k + 3], phi = io.X[6 * k + 4], rho = io.X[6 * k + 5];
        const double Hlr_z = rho * (zi - zr) + cos(phi) * cos(theta);                                                      // cslam.cpp:447
        const double px = s.predictLocation[0], py = s.predictLocation[1];
        const bool unmatched = s.nPredictTimes > 2 * s.nMatchTimes && s.nPredictTimes >= prm.min_predictions;              // cslam.cpp:449
        const bool rho_low = rho < prm.rho_min, behind = Hlr_z < 0.0;
        const bool predB = px < prm.border || py < prm.border || W - px < prm.border || H - py < prm.border;               // cslam.cpp:450
        bool matchB = false;
        if (mt) {                                                                                                          // cslam.cpp:453-456
            const double mx = io.z[2 * k], my = io.z[2 * k + 1];
            matchB = mx < prm.border || my < prm.border || W - mx < prm.border || H - my < prm.border;
        }
        const bool hard = unmatched || rho_low || behind;
        const bool store = !hard && ((predB && mt) || (!predB && matchB));                                                 // cslam.cpp:460-462
        const int bits = (unmatched ? SRUKF_POLICY_UNMATCHED : 0) | (rho_low ? SRUKF_POLICY_RHO : 0) | (behind ? SRUKF_POLICY_BEHIND : 0) |
                         (predB ? SRUKF_POLICY_PRED_BORDER : 0) | (matchB ? SRUKF_POLICY_MATCH_BORDER : 0) | (store ? SRUKF_POLICY_STORE : 0);
        io.verdict[k] = bits;
        cnt[0] += v; cnt[1] += mt; cnt[2] += (hard || predB || matchB) ? 1 : 0; cnt[3] += store ? 1 : 0;
    }
    for (int q = 0; q < 4; q++)
        for (int off = 32; off > 0; off >>= 1) cnt[q] += __shfl_down(cnt[q], off, 64);
    if ((tid & 63) == 0) for (int q = 0; q < 4; q++) red[tid >> 6][q] = cnt[q];
    __syncthreads();
    if (tid == 0) {
        int t[4];
        for (int q = 0; q < 4; q++) t[q] = red[0][q] + red[1][q] + red[2][q] + red[3][q];
        srukf_policy_summary o;
        o.n_predicts = t[0]; o.n_matches = t[1]; o.n_deletes = t[2]; o.n_stores = t[3];
        o.n_predicts_after = t[0] - t[2]; o.n_matches_after = t[1] - t[3];                                                 // every deletion takes a prediction, every store a match
        o.need_add = o.n_matches_after < prm.min_matches ? 1 : 0;                                                          // SLAM.cpp:556
        o.change = (o.n_deletes > 0 || o.need_add) ? 1 : 0;
        *io.sum = o;
    }
}

// step-wise: the caller's association, the filter's X
__global__ __launch_bounds__(256) void k_map_policy(int N, int n, double W, double H, const srukf_policy_params* __restrict__ prm, PolicyIO io)
{
    map_policy_body(N, n, W, H, *prm, io);
}

// behind a frame of an image run: row `frame` of the association's record and of the policy record.  The frame index is a kernel argument (fs->frame has advanced
// behind the tail, and the launch is eager: issue_image_policy).  A frame outside the staged stack writes nothing
__global__ __launch_bounds__(256) void k_map_policy_staged(int N, int n, double W, double H, const srukf_policy_params* __restrict__ prm, StagedPolicy a, int frame)
{
    if (frame < 0 || frame >= a.frames) return;
    const size_t f = (size_t)frame;
    const PolicyIO io = { a.X, a.h_seq + f * 2 * N, a.vis_seq + f * N, a.z_seq + f * 2 * N, a.m_seq + f * N, a.st, a.verdict + f * N, a.sum + f };
    map_policy_body(N, n, W, H, *prm, io);
}

__global__ void k_set_policy_params(srukf_policy_params* dst, srukf_policy_params v) { *dst = v; }

void launch_map_policy(hipStream_t st, KDims d, srukf_params p, const srukf_policy_params* prm, const double* X, const double* h, const int* vis, const double* z, const int* m,
                       srukf_policy_state* state, int* verdict, srukf_policy_summary* sum)
{
    const PolicyIO io = { X, h, vis, z, m, state, verdict, sum };
    hipLaunchKernelGGL(k_map_policy, dim3(1), dim3(256), 0, st, d.N, d.n, (double)p.image_w, (double)p.image_h, prm, io);
}
void launch_map_policy_staged(hipStream_t st, KDims d, srukf_params p, const srukf_policy_params* prm, StagedPolicy a, int frame)
{
    hipLaunchKernelGGL(k_map_policy_staged, dim3(1), dim3(256), 0, st, d.N, d.n, (double)p.image_w, (double)p.image_h, prm, a, frame);
}
void launch_set_policy_params(hipStream_t st, srukf_policy_params* dst, srukf_policy_params v) { hipLaunchKernelGGL(k_set_policy_params, dim3(1), dim3(1), 0, st, dst, v); }

namespace srukf_impl {

// srukf_policy_params' rules (pp null: the defaults) for the step-wise call and the switch of the image runs
int policy_params(srukf_ctx* c, const srukf_policy_params* pp, srukf_policy_params* out, const char* who)
{
    srukf_policy_params prm = SRUKF_POLICY_DEFAULTS;
    if (pp) prm = *pp;
    if (!std::isfinite(prm.border) || prm.border < 0.0 || !std::isfinite(prm.rho_min) || prm.min_predictions < 0 || prm.min_matches < 0) {
        c->err = std::string(who) + ": border must be finite and >= 0, rho_min finite, min_predictions and min_matches >= 0"; return SRUKF_ERR_BAD_ARG;
    }
    *out = prm;
    return SRUKF_OK;
}

}  // namespace srukf_impl

extern "C" {

// cslam.cpp:446-462 + 713-723 + 751 for one frame, on the filter's current X (a motion step that waits beside the state is committed first, as for a state getter)
int srukf_map_policy(srukf_ctx* c, const srukf_policy_params* pp, srukf_policy_state* state, const double* h, const int* visible, const double* z, const int* matched,
                     int* verdict, srukf_policy_summary* summary)
{
    if (!c || !state || !h || !visible || !z || !matched || !verdict || !summary) return SRUKF_ERR_BAD_ARG;
    srukf_policy_params prm;
    int rc = policy_params(c, pp, &prm, "map_policy"); if (rc) return rc;
    const size_t N = (size_t)c->d.N;
    if (N < 1) { c->err = "map_policy: the map is empty"; return SRUKF_ERR_DIM_MISMATCH; }
    if (c->async_pending) { c->err = "map_policy: staged frames are in flight (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    HIPCHK(c, hipSetDevice(c->device));
    step_commit_motion(c);
    // one scratch allocation: params | summary | state [N] | h [2N] | z [2N] | visible [N] | matched [N] | verdict [N]
    const size_t o_sum = sizeof(srukf_policy_params), o_st = o_sum + sizeof(srukf_policy_summary), o_h = o_st + sizeof(srukf_policy_state) * N, o_z = o_h + sizeof(double) * 2 * N,
                 o_v = o_z + sizeof(double) * 2 * N, o_m = o_v + sizeof(int) * N, o_o = o_m + sizeof(int) * N, bytes = o_o + sizeof(int) * N;
    static_assert(sizeof(srukf_policy_params) % 8 == 0 && sizeof(srukf_policy_summary) % 8 == 0 && sizeof(srukf_policy_state) == 24, "the scratch keeps doubles aligned");
    char* d = nullptr;
    if (srukf_dmalloc((void**)&d, bytes) != hipSuccess) { (void)hipGetLastError(); c->err = "map_policy: out of device memory"; return SRUKF_ERR_NOMEM; }
    hipError_t e = hipMemcpyAsync(d, &prm, sizeof prm, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_st, state, sizeof(srukf_policy_state) * N, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_h, h, sizeof(double) * 2 * N, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_z, z, sizeof(double) * 2 * N, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_v, visible, sizeof(int) * N, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_m, matched, sizeof(int) * N, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_map_policy(c->stream, c->d, c->p, (const srukf_policy_params*)d, c->X, (const double*)(d + o_h), (const int*)(d + o_v), (const double*)(d + o_z), (const int*)(d + o_m),
                          (srukf_policy_state*)(d + o_st), (int*)(d + o_o), (srukf_policy_summary*)(d + o_sum));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(state, d + o_st, sizeof(srukf_policy_state) * N, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(verdict, d + o_o, sizeof(int) * N, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(summary, d + o_sum, sizeof(srukf_policy_summary), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    else (void)hipStreamSynchronize(c->stream);
    srukf_dfree(d);
    HIPCHK(c, e);
    return SRUKF_OK;
}

// The switch of the image runs: on the handle, like srukf_images_search_archive.  Touches no device: the values reach it in stream order in
// front of the next image run (run_images_issue)
int srukf_images_policy(srukf_ctx* c, int on, const srukf_policy_params* pp)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    srukf_policy_params prm = SRUKF_POLICY_DEFAULTS;
    if (on) { const int rc = policy_params(c, pp, &prm, "images_policy"); if (rc) return rc; }
    if (c->async_pending && c->img.pending) { c->err = "images_policy: an image run is in flight (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    c->img_policy = on != 0;
    c->img_policy_args = prm;
    return SRUKF_OK;
}

}  // extern "C"
