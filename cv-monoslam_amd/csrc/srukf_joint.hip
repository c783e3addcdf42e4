// srukf_joint.hip — the joint measurement update (srukf_update_joint): ONE Kalman update over all of a frame's matches with the full innovation
// covariance, where KalmanUpdate (SLAM.cpp:2070-2080; k_gain) takes every landmark's gain from the same prior with that landmark's own 2 x 2 Si and adds them.  gfx950 only.
//
//   Pzz = wi sum_{i not noise} dZ_i dZ_i^T + blockdiag_k( wi sum_{i in noise} dZ_i[2k:2k+2] dZ_i[2k:2k+2]^T ),   dZ_i = Z_i - Z_0 (i >= 1; no centre term: 1769-1773)
//   Pzz = R^T R,   U^T = R^-T Pxy^T,   w = R^-T (z - h),   X += U w;   S <- gmw(S^T S - U U^T) is the refactorisation the filter has (seq_refactor on c->Ut)
//
// noise: the sigma points 1 + a and 1 + Na + a of the two pixel-noise directions a = n+3, n+4.  The reference adds the same two err components to every landmark
// (1637-1662), which a joint covariance would read as pixel noise perfectly correlated across landmarks; here every landmark keeps its own: the 2 x 2 diagonal blocks are
// exactly the reference's Si^T Si, the motion-noise points (n .. n+2, common to all landmarks) stay in the off-diagonal blocks.  The row pair of a landmark that is not
// matched, not visible or has a singular Si — and the padding rows up to mp — are identity rows / columns of Pzz, zero columns of Pxy and a zero innovation: exact, no compaction.
//
// One blocked right-looking upper Cholesky on the augmented matrix  W = [ Pzz | Pxy^T | z - h ]  (mp x ldw, ldw = mp + np + 32) in 64-row panels: the row operations that
// factor the left block leave R, U^T and w in place, no triangular solve of its own.  Launches, all on the context's stream — no workgroup waits for another, every
// dependency is a launch boundary:
//   k_joint_dev    dZ (rows of the noise points and columns of inactive rows zero)
//   k_joint_form   W: the upper 32 x 32 tiles of Pzz on the FP64 matrix pipe (4-way split-K over the sigma index, summed in fixed wave order), the noise blocks and the
//                  identity rows in the diagonal tiles' epilogue; Pxy^T with k_gain's scaling (wi gamma Ut for the rows < n-4, PxyR for the robot rows); z - h
//   per panel p:   k_joint_panel  every workgroup factors the 64 x 64 diagonal block in LDS (the same arithmetic in each: nobody waits for anybody) and solves
//                                 R_pp^-T against its 256 columns of the row block, one column per thread; workgroup 0 keeps R_pp (Rd)
//                  k_joint_trail  A_q,x -= R_p,q^T R_p,x for the rows q > p: Pzz columns >= q and all Pxy^T / innovation columns, one wave per 32 x 32 tile
//   k_joint_dx     dX = U w in fixed order, X += dX, U^T -> c->Ut in state order (rows of inactive landmarks are zero), the gamma / xi accumulators of the k_syrk
//                  launch that follows cleared as k_gain's block (0, 0) does; R_pp back into W's diagonal blocks (srukf_debug_copy "joint_R")
// A non-positive pivot (Pzz is a Gram matrix plus the noise blocks: the inputs were not finite) sets *status = 1 + its row and the pivot is replaced by 1; an innovation
// z - h that is not finite (Pzz does not depend on z) sets it the same way and enters W as zero.  k_joint_dx then leaves X alone and writes U^T = 0 (both copies), and
// records frame + 1 and the row in the frame scalars' sticky pair (first hit only; k_set_run clears it with the clamp counters): nothing loops, no NaN
// reaches the state, and the later frames of a replayed block run to their end on finite data.  The step-wise call reads *status and returns SRUKF_ERR_UNSUPPORTED with
// the row in srukf_last_error; the staged replay needs no host inside a block: srukf_synchronize reads the pair with the frame scalars.
// Staged replay ("the joint frame of the replay"): z_cur / m_cur null -> this frame's rows of the staged z_seq / m_seq through fs->frame, as k_gain
// reads them, so that one captured frame replays for every frame; k_joint_dx also writes U^T with permuted columns (ra.Utp through ra.iperm, k_gain's duty in the plain
// frame form: the frame-tail refactor forms on the permuted operands read U^T there and nowhere else).
#include "srukf_launch.h"
#include "srukf_tiles.h"

// The landmark of measurement row m takes part in the update: matched, visible, and its Si is not singular.  (A landmark whose sigma points all leave the image
// projects every one of them to the same pixel: h != 0, so "visible", with Si = 0.  KalmanUpdate's closed-form inverse of a singular Si is the zero matrix — k_gain,
// srukf_gain_lm: the landmark contributes nothing — and the same determinant decides here.)
__device__ __forceinline__ bool joint_active(int m, int N, const int* __restrict__ vis, const int* __restrict__ mt, const double* __restrict__ Si)
{
    const int k = m >> 1;
    return k < N && mt[k] != 0 && vis[k] != 0 && fma(Si[4 * k], Si[4 * k + 3], -(Si[4 * k + 1] * Si[4 * k + 2])) != 0.0;
}

// this frame's measurements and matches: the step-wise call's own, or the staged sequence's rows of the frame in hand (gain_body reads them the same way)
__device__ __forceinline__ const double* joint_z(const double* z_cur, const double* __restrict__ z_seq, const FrameScalars* __restrict__ fs, int N) { return z_cur ? z_cur : z_seq + (size_t)fs->frame * 2 * N; }
__device__ __forceinline__ const int* joint_m(const int* m_cur, const int* __restrict__ m_seq, const FrameScalars* __restrict__ fs, int N) { return m_cur ? m_cur : m_seq + (size_t)fs->frame * N; }

// *status = 1 + row unless an earlier row holds it already (several rows of one launch may report: the smallest stays, whatever the order)
__device__ __forceinline__ void joint_report(int* status, int row)
{
    int old = atomicCAS(status, 0, 1 + row);
    while (old != 0 && old > 1 + row) { const int seen = atomicCAS(status, old, 1 + row); if (seen == old) break; old = seen; }
}

// dZ[i][m] = Z[i + 1][m] - Z[0][m], i < 2 Na; zero: the four noise rows, the columns of inactive rows, the padding rows up to Kp.  grid = Kp, one row each; the first one clears the status word
__global__ __launch_bounds__(256) void k_joint_dev(KDims d, int Kp, const double* __restrict__ Z, const int* __restrict__ vis, const int* m_cur, const int* __restrict__ m_seq,
                                                   const FrameScalars* __restrict__ fs, const double* __restrict__ Si, double* __restrict__ Zd, int* __restrict__ status)
{
    const int i = blockIdx.x, mp = d.mp;
    const int* mt = joint_m(m_cur, m_seq, fs, d.N);
    if (i == 0 && threadIdx.x == 0) *status = 0;
    const int a = i < d.Na ? i : i - d.Na;
    const bool common = i < 2 * d.Na && a != d.n + 3 && a != d.n + 4;
    for (int m = threadIdx.x; m < mp; m += 256)
        Zd[(size_t)i * mp + m] = (common && joint_active(m, d.N, vis, mt, Si)) ? Z[(size_t)(i + 1) * mp + m] - Z[m] : 0.0;
}

// W = [ Pzz | Pxy^T | z - h ].  grid = (ldw / 32, mp / 32): one 32 x 32 tile of W per workgroup
__global__ __launch_bounds__(256) void k_joint_form(KDims d, KWeights w, int Kp, int ldw, const double* __restrict__ Zd, const double* __restrict__ Z,
                                                    const int* __restrict__ vis, const int* m_cur, const int* __restrict__ m_seq, const double* __restrict__ Si, const double* __restrict__ Ut,
                                                    const double* __restrict__ PxyR, const double* __restrict__ h, const double* z_cur, const double* __restrict__ z_seq,
                                                    const FrameScalars* __restrict__ fs, double* __restrict__ W, int* __restrict__ status)
{
    __shared__ double red[3][64][17];
    const int mp = d.mp, np = d.np, n = d.n, N = d.N;
    const int* mt = joint_m(m_cur, m_seq, fs, N);
    const double* z = joint_z(z_cur, z_seq, fs, N);
    const int m0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    if (c0 >= mp) {
        // Pxy^T as k_gain reads it, and the innovation in the first of the last 32 columns
        const double sc = w.wi * w.gamma;
        for (int e = threadIdx.x; e < 32 * 32; e += 256) {
            const int m = m0 + (e >> 5), c = c0 + (e & 31), r = c - mp;
            double v = 0.0;
            if (joint_active(m, N, vis, mt, Si)) {
                if (r < n - 4) v = sc * Ut[(size_t)m * np + r];
                else if (r < n) v = PxyR[(size_t)(r - (n - 4)) * mp + m];
                else if (r == np) {
                    v = z[m] - h[m];
                    if (!(fabs(v) <= 1.79769313486231570e308)) { joint_report(status, m); v = 0.0; }      // NaN or infinite: Pzz would never show it
                }
            }
            W[(size_t)m * ldw + c] = v;
        }
        return;
    }
    if (c0 < m0) {                                             // below the diagonal: zero (nothing reads it; R is read back as a whole)
        for (int e = threadIdx.x; e < 32 * 32; e += 256) W[(size_t)(m0 + (e >> 5)) * ldw + c0 + (e & 31)] = 0.0;
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    d4 acc[2][2];
    zero_acc(acc);
    const int ng = Kp >> 4;
    const int g0 = (ng * wv) >> 2, g1 = (ng * (wv + 1)) >> 2;
    tile32_tn<false>(acc, Zd, mp, Zd, mp, m0, c0, g0 << 4, g1 << 4, lane);
    splitk_reduce(acc, red, wv, lane);
    if (wv != 0) return;
    const int lr = lane & 15, lk = lane >> 4;
    const int Na = d.Na;
    const int nz[4] = { 1 + n + 3, 1 + n + 4, 1 + Na + n + 3, 1 + Na + n + 4 };      // sigma rows of Z
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int m = m0 + 16 * a + lk + 4 * t, c = c0 + 16 * b + lr;
                double v = w.wi * acc[a][b][t];
                if ((m >> 1) == (c >> 1)) {                    // the landmark's own 2 x 2 block (diagonal tiles only)
                    if (joint_active(m, N, vis, mt, Si)) {
                        double s = 0.0;
#pragma unroll
                        for (int q = 0; q < 4; q++) s += (Z[(size_t)nz[q] * mp + m] - Z[m]) * (Z[(size_t)nz[q] * mp + c] - Z[c]);
                        v += w.wi * s;
                    } else
                        v = m == c ? 1.0 : 0.0;
                }
                W[(size_t)m * ldw + c] = v;
            }
}

// Panel p: R_pp = chol(A_pp) in LDS, then row block  A_p,x <- R_pp^-T A_p,x  for the columns x >= 64 (p + 1).  grid = ceil((ldw - 64 (p + 1)) / 256), at least 1
__global__ __launch_bounds__(256) void k_joint_panel(int p, int ldw, double* __restrict__ W, double* __restrict__ Rd, int* __restrict__ status)
{
    __shared__ double Ls[64][65];
    const int t = threadIdx.x, j0 = 64 * p;
    for (int e = t; e < 64 * 64; e += 256) { const int i = e >> 6, c = e & 63; Ls[i][c] = c >= i ? W[(size_t)(j0 + i) * ldw + j0 + c] : 0.0; }
    int bad = 0;
    const int c = t & 63, i4 = t >> 6;
    for (int j = 0; j < 64; j++) {
        __syncthreads();
        double dj = Ls[j][j];
        if (!(dj > 0.0)) { if (!bad) bad = 1 + j0 + j; dj = 1.0; }
        const double rj = sqrt(dj);
        __syncthreads();
        if (t < 64 && c >= j) Ls[j][c] = c == j ? rj : Ls[j][c] / rj;
        __syncthreads();
        for (int i = i4 + 4 * ((j + 1 - i4 + 3) >> 2); i < 64; i += 4)      // rows i > j with i = i4 (mod 4)
            if (c >= i) Ls[i][c] -= Ls[j][i] * Ls[j][c];
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int e = t; e < 64 * 64; e += 256) Rd[(size_t)(j0 + (e >> 6)) * 64 + (e & 63)] = Ls[e >> 6][e & 63];
        if (t == 0 && bad && *status == 0) *status = bad;
    }
    const int x = j0 + 64 + blockIdx.x * 256 + t;
    if (x >= ldw) return;
    double y[64];
#pragma unroll
    for (int i = 0; i < 64; i++) y[i] = W[(size_t)(j0 + i) * ldw + x];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        double s = y[i];
#pragma unroll
        for (int j = 0; j < i; j++) s -= Ls[j][i] * y[j];
        y[i] = s / Ls[i][i];
    }
#pragma unroll
    for (int i = 0; i < 64; i++) W[(size_t)(j0 + i) * ldw + x] = y[i];
}

// Trailing update behind panel p: A_q,x -= R_p,q^T R_p,x, rows q > p, Pzz columns >= q (upper tiles) and every column behind Pzz.  One wave per 32 x 32 tile:
// grid = (ceil(column tiles / 4), row tiles), tiles counted from 2 (p + 1)
__global__ __launch_bounds__(256) void k_joint_trail(int p, int ldw, double* __restrict__ W)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int rt = 2 * (p + 1) + blockIdx.y, ct = 2 * (p + 1) + blockIdx.x * 4 + wv;
    if (ct < rt || ct * 32 >= ldw) return;
    d4 acc[2][2];
    zero_acc(acc);
    tile32_tn<true>(acc, W, ldw, W, ldw, rt * 32, ct * 32, 64 * p, 64 * p + 64, lane);
    const int lr = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int t = 0; t < 4; t++)
                W[(size_t)(rt * 32 + 16 * a + lk + 4 * t) * ldw + ct * 32 + 16 * b + lr] += acc[a][b][t];
}

// dX = U w, X += dX, U^T -> Ut (mp x np, state order) and, where the rank-aware operands exist, -> ra.Utp with permuted columns.  grid = np / 64 workgroups of 64 (one
// state row per thread), then mp / 64 that put R_pp back into W.  A frame whose status word is set: zero U^T, X untouched, the sticky pair of the frame scalars
__global__ __launch_bounds__(64) void k_joint_dx(KDims d, int ldw, double* __restrict__ W, const double* __restrict__ Rd, const int* __restrict__ status,
                                                 double* __restrict__ Ut, double* __restrict__ X, FrameScalars* __restrict__ fs, double* __restrict__ Utp, const int* __restrict__ iperm)
{
    const int mp = d.mp, np = d.np, nb = np / 64;
    if ((int)blockIdx.x >= nb) {
        const int j0 = 64 * ((int)blockIdx.x - nb);
        for (int i = 0; i < 64; i++) W[(size_t)(j0 + i) * ldw + j0 + threadIdx.x] = Rd[(size_t)(j0 + i) * 64 + threadIdx.x];
        return;
    }
    const int st = *status;
    const bool ok = st == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        fs->gmax_bits = 0ull; fs->ximax_bits = 0ull;
        if (!ok && fs->joint_bad_frame == 0) { fs->joint_bad_frame = fs->frame + 1; fs->joint_bad_row = st - 1; }
    }
    const int r = blockIdx.x * 64 + threadIdx.x;
    const int rp = Utp ? iperm[r] : 0;
    double dx = 0.0;
    for (int m = 0; m < mp; m++) {
        const double u = ok ? W[(size_t)m * ldw + mp + r] : 0.0;
        Ut[(size_t)m * np + r] = u;
        if (Utp) Utp[(size_t)m * np + rp] = u;
        if (ok) dx = fma(u, W[(size_t)m * ldw + mp + np], dx);
    }
    if (ok && r < d.n) X[r] += dx;
}

int joint_dev_rows(int Na) { return (2 * Na + 15) & ~15; }
int joint_work_ld(int mp, int np) { return mp + np + 32; }

void launch_joint_form(hipStream_t st, KDims d, KWeights w, const JointFrame& f, const double* Z, const int* vis, const double* Si, const double* Ut, const double* PxyR, const double* h,
                       double* Zd, double* W, int* status)
{
    const int Kp = joint_dev_rows(d.Na), ldw = joint_work_ld(d.mp, d.np);
    hipLaunchKernelGGL(k_joint_dev, dim3(Kp), dim3(256), 0, st, d, Kp, Z, vis, f.m_cur, f.m_seq, f.fs, Si, Zd, status);
    hipLaunchKernelGGL(k_joint_form, dim3(ldw / 32, d.mp / 32), dim3(256), 0, st, d, w, Kp, ldw, Zd, Z, vis, f.m_cur, f.m_seq, Si, Ut, PxyR, h, f.z_cur, f.z_seq, f.fs, W, status);
}

void launch_joint_factor(hipStream_t st, KDims d, double* W, double* Rd, int* status)
{
    const int ldw = joint_work_ld(d.mp, d.np), P = d.mp / 64;
    for (int p = 0; p < P; p++) {
        const int cols = ldw - 64 * (p + 1);
        hipLaunchKernelGGL(k_joint_panel, dim3((cols + 255) / 256), dim3(256), 0, st, p, ldw, W, Rd, status);
        if (p + 1 < P) {
            const int ct = ldw / 32 - 2 * (p + 1), rt = d.mp / 32 - 2 * (p + 1);
            hipLaunchKernelGGL(k_joint_trail, dim3((ct + 3) / 4, rt), dim3(256), 0, st, p, ldw, W);
        }
    }
}

void launch_joint_dx(hipStream_t st, KDims d, double* W, const double* Rd, const int* status, double* Ut, double* X, FrameScalars* fs, const RankArgs& ra)
{
    hipLaunchKernelGGL(k_joint_dx, dim3(d.np / 64 + d.mp / 64), dim3(64), 0, st, d, joint_work_ld(d.mp, d.np), W, Rd, status, Ut, X, fs, ra.Utp, ra.iperm);
}
