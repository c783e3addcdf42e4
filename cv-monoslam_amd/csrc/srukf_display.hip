// Display ellipsoids of the landmarks: get3DdisplayInformation (SLAM.cpp:2791-2806) with calculateEigenvaluesAndEigenvectors (2815-2892) and
// matrix2Quaternion (2903-2948) for ALL landmarks in one launch, on the 3 x 3 Cartesian covariances k_landmarks_cartesian left on the device.
//
// The arithmetic is the facade's (host/cslam.cpp, CSLAM::calculateEigenvaluesAndEigenvectors / matrix2Quaternion), operation for operation and in its order:
// classical Jacobi — the off-diagonal entry of largest magnitude below the diagonal (scan (1,0), (2,0), (2,1); strict >, so the first largest wins and a NaN never
// does) is annihilated by a plane rotation A <- R^T A R, V <- V R, until that magnitude is below epsilon or 30 n^2 + 1 passes have run.  All nine entries of A are
// carried (the input need not be symmetric to the last bit, and the host updates row and column separately).  This file is built without contraction
// (-ffp-contract=off); sqrt and / are the correctly rounded fp64 ones, nothing else is called — tests/np_display.py restates it on Python floats bit for bit.
//
// One thread per landmark; A and V live in 18 named registers.  Which of them a rotation touches is decided by a 3-way switch over the pivot, so every access is
// resolved at compile time (a private array indexed by p / q would live in scratch memory).
#include "srukf_ctx.h"

namespace {

// the plane rotation in the (p, q) plane, r the third index: (app, aqq, apq, aqp) the 2 x 2 block, (apr, aqr) / (arp, arq) the rest of rows / columns p and q
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& aqp, double& apr, double& aqr, double& arp, double& arq,
                                              double& v0p, double& v0q, double& v1p, double& v1q, double& v2p, double& v2q)
{
    const double x = -apq, y = 0.5 * (aqq - app);
    double omega = x / sqrt(x * x + y * y);
    if (y < 0.0) omega = -omega;
    const double sn = omega / sqrt(2.0 * (1.0 + sqrt(1.0 - omega * omega)));
    const double cn = sqrt(1.0 - sn * sn);
    const double pp = app, qq = aqq, pq = apq;
    app = pp * cn * cn + qq * sn * sn + pq * omega;
    aqq = pp * sn * sn + qq * cn * cn - pq * omega;
    apq = 0.0; aqp = 0.0;
    { const double ap = apr, aq = aqr; apr = ap * cn + aq * sn; aqr = -ap * sn + aq * cn; }      // row p, row q: column r
    { const double ap = arp, aq = arq; arp = ap * cn + aq * sn; arq = -ap * sn + aq * cn; }      // column p, column q: row r
    { const double vp = v0p, vq = v0q; v0p = vp * cn + vq * sn; v0q = -vp * sn + vq * cn; }
    { const double vp = v1p, vq = v1q; v1p = vp * cn + vq * sn; v1q = -vp * sn + vq * cn; }
    { const double vp = v2p, vq = v2q; v2p = vp * cn + vq * sn; v2q = -vp * sn + vq * cn; }
}

}  // namespace

#define LM_ELLIPSOID_PASSES (30 * 3 * 3 + 1)

__global__ __launch_bounds__(64) void k_lm_ellipsoid(int N, double eps, const double* __restrict__ cov, double* __restrict__ axis, double* __restrict__ sigma,
                                                     int* __restrict__ rot)
{
    const int id = blockIdx.x * 64 + threadIdx.x;
    if (id >= N) return;
    const double* c = cov + 9 * (size_t)id;
    double a00 = c[0], a01 = c[1], a02 = c[2], a10 = c[3], a11 = c[4], a12 = c[5], a20 = c[6], a21 = c[7], a22 = c[8];
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    int nrot = -1;
    for (int it = 0; it < LM_ELLIPSOID_PASSES; it++) {
        int piv = 0; double big = 0.0;
        if (fabs(a10) > big) { big = fabs(a10); piv = 1; }
        if (fabs(a20) > big) { big = fabs(a20); piv = 2; }
        if (fabs(a21) > big) { big = fabs(a21); piv = 3; }
        if (big < eps || piv == 0) { nrot = it; break; }          // (piv == 0 with big >= eps: epsilon <= 0, where the host has no pivot either)
        switch (piv) {
        case 1:  jacobi_rotate(a11, a00, a10, a01, a12, a02, a21, a20, v01, v00, v11, v10, v21, v20); break;      // p = 1, q = 0, r = 2
        case 2:  jacobi_rotate(a22, a00, a20, a02, a21, a01, a12, a10, v02, v00, v12, v10, v22, v20); break;      // p = 2, q = 0, r = 1
        default: jacobi_rotate(a22, a11, a21, a12, a20, a10, a02, a01, v02, v01, v12, v11, v22, v21); break;      // p = 2, q = 1, r = 0
        }
    }
    rot[id] = nrot;
    // 1-sigma semi-axes in the positions the rotations left them (a negative eigenvalue: NaN, as on the host)
    sigma[3 * (size_t)id + 0] = sqrt(a00); sigma[3 * (size_t)id + 1] = sqrt(a11); sigma[3 * (size_t)id + 2] = sqrt(a22);
    // matrix2Quaternion(V): m11 .. m33 = v00 .. v22, element pairing as in the reference
    double qr, qx, qy, qz;
    const double tr = v00 + v11 + v22;
    if (tr > 0.0) {
        const double t = 0.5 / sqrt(tr + 1);
        qr = 0.25 / t; qx = (v12 - v21) * t; qy = (v20 - v02) * t; qz = (v01 - v10) * t;
    } else if (v00 > v11 && v00 > v22) {
        const double t = 2.0 * sqrt(1.0 + v00 - v11 - v22);
        qr = (v21 - v12) / t; qx = 0.25 * t; qy = (v01 + v10) / t; qz = (v02 + v20) / t;
    } else if (v11 > v22) {
        const double t = 2.0 * sqrt(1.0 + v11 - v00 - v22);
        qr = (v02 - v20) / t; qx = (v01 + v10) / t; qy = 0.25 * t; qz = (v12 + v21) / t;
    } else {
        const double t = 2.0 * sqrt(1.0 + v22 - v00 - v11);
        qr = (v10 - v01) / t; qx = (v02 + v20) / t; qy = (v12 + v21) / t; qz = 0.25 * t;
    }
    double* q = axis + 4 * (size_t)id;
    q[0] = qr; q[1] = qx; q[2] = qy; q[3] = qz;
}

namespace srukf_impl {

void launch_lm_ellipsoid(hipStream_t st, int N, double eps, const double* cov, double* axis, double* sigma, int* rot)
{
    if (N <= 0) return;
    hipLaunchKernelGGL(k_lm_ellipsoid, dim3((N + 63) / 64), dim3(64), 0, st, N, eps, cov, axis, sigma, rot);
}

}  // namespace srukf_impl
