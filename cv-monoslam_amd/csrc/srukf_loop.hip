// srukf_loop.hip — loop points on the device: what an archived landmark takes along (FeatureInfo, SLAM.cpp:1357-1378, 2516-2532) and its re-insertion into the
// state with the archived mean and square-root block (integrateFeaturesInformation's isLoop branch, 948-1015).  gfx950 only.
//   k_lm_record   the upper Cholesky factor of the landmark's marginal block P66 (left in `small` by k_block_cov), its six rows of X and its appearance
//                 record packed into one staging block: srukf_get_landmark_record needs one device-to-host copy
//   k_lm_records  the same for K landmarks in one launch, behind k_block_cov over the same K landmarks
//   k_lm_insert   the grown X' and S': old rows / columns at their new indices, the new landmarks' blocks on the diagonal, zero elsewhere.  Pure copies
// This file is built with -ffp-contract=off: the factor must round as written (tests/np_loop.py restates it bit for bit).
#include "srukf_ctx.h"
using namespace srukf_impl;

// lm_record_body: one landmark's record, ONE text for its two callers (k_lm_record: one workgroup; k_lm_records: one per landmark).
// Thread 0 factors, all nt threads copy the patch.  P66 symmetric row-major; eps = params.epsilon.
//   d_j = max(eps, P_jj - sum_{m<j} S_mj^2),  S_jj = sqrt(d_j),  S_ji = (P_ji - sum_{m<j} S_mj S_mi) / S_jj  (i > j), sums in ascending m
__device__ __forceinline__ void lm_record_body(int nt, const double* P66, const double* __restrict__ X, int k, double eps,
                                               const unsigned char* __restrict__ app_patch, int patch_stride, const double* __restrict__ appR,
                                               const double* __restrict__ appT, const double* __restrict__ appPx, const int* __restrict__ has_app,
                                               double* __restrict__ out)
{
    const int t = threadIdx.x;
    const bool app = has_app && has_app[k] != 0;
    unsigned char* pb = (unsigned char*)(out + LM_REC_DOUBLES);
    for (int i = t; i < 8 * LM_REC_PATCH_DOUBLES; i += nt) pb[i] = (app && i < PT_PATCH_BYTES) ? app_patch[(size_t)k * patch_stride + i] : 0;
    if (t != 0) return;
    double S[36];
    for (int e = 0; e < 36; e++) S[e] = 0.0;
    for (int j = 0; j < 6; j++) {
        double s = 0.0;
        for (int m = 0; m < j; m++) s += S[6 * m + j] * S[6 * m + j];
        double d = P66[6 * j + j] - s;
        d = d > eps ? d : eps;
        const double sjj = sqrt(d);
        S[6 * j + j] = sjj;
        for (int i = j + 1; i < 6; i++) {
            double q = 0.0;
            for (int m = 0; m < j; m++) q += S[6 * m + j] * S[6 * m + i];
            S[6 * j + i] = (P66[6 * j + i] - q) / sjj;
        }
    }
    for (int e = 0; e < 6; e++) out[e] = X[6 * k + e];
    for (int e = 0; e < 36; e++) out[6 + e] = S[e];
    for (int e = 0; e < 9; e++) out[42 + e] = app ? appR[9 * k + e] : 0.0;
    for (int e = 0; e < 3; e++) out[51 + e] = app ? appT[3 * k + e] : 0.0;
    for (int e = 0; e < 2; e++) out[54 + e] = app ? appPx[2 * k + e] : 0.0;
    out[LM_REC_DOUBLES - 1] = app ? 1.0 : 0.0;
}

__global__ __launch_bounds__(64) void k_lm_record(const double* __restrict__ P66, const double* __restrict__ X, int k, double eps,
                                                  const unsigned char* __restrict__ app_patch, int patch_stride, const double* __restrict__ appR,
                                                  const double* __restrict__ appT, const double* __restrict__ appPx, const int* __restrict__ has_app,
                                                  double* __restrict__ out)
{
    lm_record_body(64, P66, X, k, eps, app_patch, patch_stride, appR, appT, appPx, has_app, out);
}

// k_lm_records: the records of K landmarks in one launch (srukf_delete_landmarks).  Workgroup q packs landmark ids[q]'s record at
// out + q * SRUKF_LM_RECORD_DOUBLES from its block P66 + 36 q (k_block_cov with the same ids, the launch in front).  No workgroup reads what another one writes.
// ids[q] in [0, N): the host has checked them
__global__ __launch_bounds__(64) void k_lm_records(const double* __restrict__ P66, const double* __restrict__ X, const int* __restrict__ ids, double eps,
                                                   const unsigned char* __restrict__ app_patch, int patch_stride, const double* __restrict__ appR,
                                                   const double* __restrict__ appT, const double* __restrict__ appPx, const int* __restrict__ has_app,
                                                   double* __restrict__ out)
{
    lm_record_body(64, P66 + 36 * (size_t)blockIdx.x, X, ids[blockIdx.x], eps, app_patch, patch_stride, appR, appT, appPx, has_app,
                   out + (size_t)blockIdx.x * SRUKF_LM_RECORD_DOUBLES);
}

// state index of the grown state -> index of the old one: landmarks before the insertion point keep theirs, the L new ones have none (-1),
// the rest (the armed landmarks and the robot block) move up by 6 L; padding (-2)
__device__ __forceinline__ int lm_src(int r, int p6, int L6, int n2)
{
    return r < p6 ? r : (r < p6 + L6 ? -1 : (r < n2 ? r - L6 : -2));
}

// one thread per element of the ld2 x ld2 matrix S' (row blockIdx.y, columns along x: coalesced) and, in the extra row ld2, of X'.  blk = X6 (6 L) | S66 (36 L).
__global__ __launch_bounds__(256) void k_lm_insert(const double* __restrict__ S, int ld, const double* __restrict__ X, int p6, int L, const double* __restrict__ blk,
                                                   double* __restrict__ S2, double* __restrict__ X2, int n2, int ld2)
{
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, L6 = 6 * L;
    if (c >= ld2) return;
    const int sc = lm_src(c, p6, L6, n2);
    if (r == ld2) {                                                      // X'
        X2[c] = sc >= 0 ? X[sc] : (sc == -1 ? blk[c - p6] : 0.0);
        return;
    }
    const int sr = lm_src(r, p6, L6, n2);
    double v = 0.0;
    if (r <= c) {
        if (sr >= 0 && sc >= 0) v = S[(size_t)sr * ld + sc];
        else if (sr == -1 && sc == -1 && (r - p6) / 6 == (c - p6) / 6) {
            const int j = (r - p6) / 6;
            v = blk[L6 + 36 * j + 6 * ((r - p6) % 6) + (c - p6) % 6];
        }
    }
    S2[(size_t)r * ld2 + c] = v;
}

namespace srukf_impl {

void launch_lm_record(hipStream_t st, const double* P66, const double* X, int k, double eps, const unsigned char* app_patch, const double* appR,
                      const double* appT, const double* appPx, const int* has_app, double* out)
{
    hipLaunchKernelGGL(k_lm_record, dim3(1), dim3(64), 0, st, P66, X, k, eps, app_patch, PT_PATCH_STRIDE, appR, appT, appPx, has_app, out);
}

void launch_lm_insert(hipStream_t st, const double* S, int ld, const double* X, int p6, int L, const double* blk, double* S2, double* X2, int n2, int ld2)
{
    hipLaunchKernelGGL(k_lm_insert, dim3((ld2 + 255) / 256, ld2 + 1), dim3(256), 0, st, S, ld, X, p6, L, blk, S2, X2, n2, ld2);
}

}  // namespace srukf_impl

void launch_lm_records(hipStream_t st, int K, KDims d, const double* S, const double* X, const int* ids, double eps, const unsigned char* app_patch, const double* appR,
                       const double* appT, const double* appPx, const int* has_app, double* P66, double* out)
{
    srukf_launch_block_cov_many(st, d, S, ids, K, P66);
    hipLaunchKernelGGL(k_lm_records, dim3(K), dim3(64), 0, st, P66, X, ids, eps, app_patch, PT_PATCH_STRIDE, appR, appT, appPx, has_app, out);
}
