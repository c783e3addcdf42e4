// srukf_gmw_pivot.h — the arithmetic phases of ONE 64-pivot panel of the critical-path ("pivot") workgroup of the blocked GMW
// factorisation: apply the previous panel to the 64x64 diagonal region R (three-stage slab, K = 64 update of tiles (0,0), (0,1),
// (1,1)), factor R as two 32-pivot sub-panels (srukf_gmw_cols.h) with C1 / C2 between them, write the S rows and the panel buffer.
// gfx950 only.
//
// Three bodies run these phases and must give the same bits — the same products in the same order, K ascending on every accumulator:
//   gmw_step64_block00 (srukf_factor.hip)       one launch per panel: operands from global memory, plain stores
//   gmw_pivot_persist  (srukf_gmw_persist.hip)  the resident pivot: previous panel from LDS, tiles staged behind version flags
//   gmw_pivot_relay    (srukf_gmw_persist.hip)  two pivots alternate: previous panel from the panel buffer, K ranges cut at 32
// They differ in where an operand comes from (a template parameter or a functor here), in who stores what with which scope, and in
// their protocol.  The protocol is NOT here: no function of this file contains a barrier, a wait, a flag store, an abandon or a time
// stamp.  A barrier under wave-divergent control flow hangs the launch, and several phases below run in some waves only; as long as
// every __syncthreads, gmw_wait_ge, gmw_set_panel_flag*, gmw_abandon, GMW_TS and STAMP stands in the three bodies, a reader checks
// that by reading one loop body.  No function here asks which body calls it either.
//
// Workgroup = 4 waves.  Wave w owns columns 16w .. 16w+15 of the slab and quarter (qa, qb) = (w >> 1, w & 1) of a 32x32 block;
// waves 1 / 3 own the 32x32 tiles (0,1) / (1,1) of R (rows ro .., columns 32 ..).  Lr / Wc [64][G64_LS]: the slab rows L = W / D and W.
#pragma once
#include "srukf_device.h"
#include "srukf_gmw_cols.h"
#include "srukf_gmw_panel.h"

// lr / lk: column and k index of this lane in a 16x16x4 MFMA fragment; wvu: wave-uniform copy of wv (scalar branches)
struct GmwLane { int lane, wv, lr, lk, qa, qb, ro, wvu; };
__device__ __forceinline__ GmwLane gmw_lane_view(int tid)
{
    GmwLane L;
    L.lane = tid & 63; L.wv = tid >> 6; L.lr = L.lane & 15; L.lk = L.lane >> 4;
    L.qa = L.wv >> 1; L.qb = L.wv & 1;
    L.ro = (L.wv == 1) ? 0 : 32;
    L.wvu = __builtin_amdgcn_readfirstlane(L.wv);
    return L;
}

// ---- where the A fragment of a slab stage comes from: element (k = 4u + lk, column 16h + lr) of a 32x32 panel matrix ----
// (the LDS forms take the row pointer first and index it: as ONE index expression the swizzled column is or-ed into the row offset,
//  the constant part of the row no longer folds into the instruction's offset and the paired ds_read2st64 reads are lost)
struct GmwAFromLds33 {                          // LDS, [k][33] (the T wave's layout)
    const double* M; int lk, lr;
    __device__ __forceinline__ GmwAFromLds33(const double* m, const GmwLane& L) : M(m), lk(L.lk), lr(L.lr) {}
    __device__ __forceinline__ double operator()(int u, int h) const { const double* rowp = &M[(4 * u + lk) * 33]; return rowp[16 * h + lr]; }
};
struct GmwAFromLdsSwz {                         // LDS, [k][32] with column ^ 16 * (k & 1);  (4u + lk) & 1 == lk & 1
    const double* M; int lk, lr;
    __device__ __forceinline__ GmwAFromLdsSwz(const double* m, const GmwLane& L) : M(m), lk(L.lk), lr(L.lr) {}
    __device__ __forceinline__ double operator()(int u, int h) const { const double* rowp = &M[(4 * u + lk) * 32]; return rowp[(16 * h + lr) ^ (16 * (lk & 1))]; }
};
template <bool TRI> struct GmwAFromBuffer {     // registers, requested from the panel buffer [k][32] by agent-scope loads before the first MFMA
    double h0[TRI ? 4 : 8], h1[8];
    __device__ __forceinline__ GmwAFromBuffer(const double* M, const GmwLane& L)
    {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int o = (4 * u + L.lk) * 32 + L.lr;
            if (!TRI || u < 4) h0[u] = ld_dev(&M[o]);
            h1[u] = ld_dev(&M[o + 16]);
        }
    }
    __device__ __forceinline__ double operator()(int u, int h) const { return h ? h1[u] : h0[u]; }
};

// One slab stage for this wave's 16 columns: W[h] += (NEG ? -A : A)(., 16h ..)^T-fragment x B over 8 k-steps, B[u >> 2][u & 3] = row 4u + lk.
// TRI: A is a transposed triangular factor, Tt[k][j] = 0 for k > j, so the k-steps u >= 4 contribute nothing to columns 0..15.
//   stage 1  W1 = T1' G1 (TRI)      stage 2  G2' = G2 - E'^T W1 (NEG)      stage 3  W2 = T2' G2' (TRI)
template <bool TRI, bool NEG, class ASrc>
__device__ __forceinline__ void gmw_slab_stage(const ASrc& A, const d4 (&B)[2], d4 (&W)[2])
{
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const double b = B[u >> 2][u & 3];
        if (!TRI || u < 4) W[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(NEG ? -A(u, 0) : A(u, 0), b, W[0], 0, 0, 0);
        W[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(NEG ? -A(u, 1) : A(u, 1), b, W[1], 0, 0, 0);
    }
}
// the two halves of a staged 64-row tile column as stage operands: G[h][a][t] = row 32h + 16a + lk + 4t, column 16 wv + lr
__device__ __forceinline__ void gmw_slab_operands(const GmwLane& L, const double (*Lr)[G64_LS], d4 (&G)[2][2])
{
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int t = 0; t < 4; t++) G[h][a][t] = Lr[32 * h + 16 * a + L.lk + 4 * t][16 * L.wv + L.lr];
}
// rows 32 HALF .. 32 HALF + 31 of the slab: Wc = W, Lr = W * (1/D);  dr[a][t] = 1/D of row 32 HALF + 16a + lk + 4t
template <int HALF>
__device__ __forceinline__ void gmw_slab_store(const GmwLane& L, double (*Lr)[G64_LS], double (*Wc)[G64_LS], const d4 (&W)[2], const double (&dr)[2][4])
{
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int jj = 32 * HALF + 16 * a + L.lk + 4 * t, cc = 16 * L.wv + L.lr;
            Wc[jj][cc] = W[a][t];       Lr[jj][cc] = W[a][t] * dr[a][t];
        }
}

// ---- quarters and the waves 1 / 3 tiles ----
template <class Arr> __device__ __forceinline__ d4 gmw_quarter_load(const GmwLane& L, const Arr& M)
{
    d4 g;
#pragma unroll
    for (int t = 0; t < 4; t++) g[t] = M[16 * L.qa + L.lk + 4 * t][16 * L.qb + L.lr];
    return g;
}
__device__ __forceinline__ void gmw_quarter_store(const GmwLane& L, double (*Xm)[32], const d4& g)
{
#pragma unroll
    for (int t = 0; t < 4; t++) Xm[16 * L.qa + L.lk + 4 * t][16 * L.qb + L.lr] = g[t];
}
// waves 1 / 3: tile (0,1) / (1,1) of the staged region -> acc
__device__ __forceinline__ void gmw_side_load(const GmwLane& L, const double (*Wc)[G64_LS], d4 (&acc)[2][2])
{
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int t = 0; t < 4; t++) acc[a][b][t] = Wc[L.ro + 16 * a + L.lk + 4 * t][32 + 16 * b + L.lr];
}
// quarter (qa, qb):  g -= L^T W over slab rows K0 .. K1-1 (tile (0,0) with the slab; C2 with E' / W1d in rows 0..31)
template <int K0, int K1>
__device__ __forceinline__ void gmw_quarter_update(const GmwLane& L, const double (*Lr)[G64_LS], const double (*Wc)[G64_LS], d4& g)
{
#pragma unroll
    for (int k = K0; k < K1; k += 4)
        g = __builtin_amdgcn_mfma_f64_16x16x4f64(-Lr[k + L.lk][16 * L.qa + L.lr], Wc[k + L.lk][16 * L.qb + L.lr], g, 0, 0, 0);
}
// waves 1 / 3:  acc -= L^T W over slab rows K0 .. K1-1
template <int K0, int K1>
__device__ __forceinline__ void gmw_side_update(const GmwLane& L, const double (*Lr)[G64_LS], const double (*Wc)[G64_LS], d4 (&acc)[2][2])
{
#pragma unroll
    for (int k = K0; k < K1; k += 4) {
        const double a0 = -Lr[k + L.lk][L.ro + L.lr], a1 = -Lr[k + L.lk][L.ro + 16 + L.lr];
        const double b0 = Wc[k + L.lk][32 + L.lr], b1 = Wc[k + L.lk][48 + L.lr];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
}
// waves 1 / 3 park their updated tile for C1 / C2
__device__ __forceinline__ void gmw_side_park(const GmwLane& L, double (*X)[32], const d4 (&acc)[2][2])
{
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int t = 0; t < 4; t++) X[16 * a + L.lk + 4 * t][16 * b + L.lr] = acc[a][b][t];
}

// ---- S rows ----
// sqrt(D)/D of the previous panel's rows, for gmw_panel_s_rows: from memory (LDS copy or panel buffer; the loop stays rolled by 4) or
// requested ahead into registers (the loop must unroll completely)
struct GmwSqFromMem {
    static constexpr int UNROLL = 4;
    const double* sq;
    __device__ __forceinline__ double operator()(int i, int row) const { return sq[row]; }
};
struct GmwSqFromBuffer {
    static constexpr int UNROLL = 8;
    double v[8];
    __device__ __forceinline__ void load(const GmwLane& L, const double* sq)
    {
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = ld_dev(&sq[L.ro + 4 * i + L.lk]);
    }
    __device__ __forceinline__ double operator()(int i, int row) const { return v[i]; }
};
// waves 1 / 3: the S rows of the previous panel for R's columns, from the LDS slab: wave 1 rows j0 .. j0+31, wave 3 rows j0+32 .. j0+63
// (rows / columns >= n carry zeros: G is zero there)
template <class Sq>
__device__ __forceinline__ void gmw_panel_s_rows(const GmwLane& L, const double (*Wc)[G64_LS], double* __restrict__ Sout, int ld, int j0, int base, const Sq& sqsrc)
{
    const int c4 = L.lr * 4;
#pragma unroll Sq::UNROLL
    for (int i = 0; i < 8; i++) {
        const int row = L.ro + 4 * i + L.lk;
        const double sq = sqsrc(i, row);
        d4 w = *(const d4*)&Wc[row][c4];
        w[0] *= sq; w[1] *= sq; w[2] *= sq; w[3] *= sq;
        *(d4*)&Sout[(size_t)(j0 + row) * ld + base + c4] = w;
    }
}
// one wave: S rows base .. base+31, columns base+32 .. base+63 (the (0,1) tile: W1d in Wc, scaled by sqrt(D)/D of factor 1)
__device__ __forceinline__ void gmw_s01_rows(const GmwLane& L, const double* Dv, const double (*Wc)[G64_LS], double* __restrict__ Sout, int n, int ld, int base)
{
    const int c4 = (L.lane & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = 8 * i + (L.lane >> 3);
        const double Dr = Dv[row];
        const double sq = (base + row < n) ? sqrt(Dr) * gmw_pivot_rcp(Dr) : 0.0;
        d4 w = *(const d4*)&Wc[row][c4];
        w[0] *= sq; w[1] *= sq; w[2] *= sq; w[3] *= sq;
        *(d4*)&Sout[(size_t)(base + row) * ld + base + 32 + c4] = w;
    }
}

// ---- between the two factors ----
// C1: quarter (qa, qb) of W1d = T1' X01 -> Wc and of E' = W1d / D' -> Lr (the slabs are dead by now).  also(k, cc, e): a further home for E'.
struct GmwNoAlso { __device__ __forceinline__ void operator()(int, int, double) const {} };
template <class Also = GmwNoAlso>
__device__ __forceinline__ void gmw_c1(const GmwLane& L, const double* T1, const double (*X01)[32], const double* Dv, double (*Lr)[G64_LS], double (*Wc)[G64_LS],
                                       Also&& also = Also())
{
    d4 wq = (d4){0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 8; u++)
        wq = __builtin_amdgcn_mfma_f64_16x16x4f64(T1[(4 * u + L.lk) * 33 + 16 * L.qa + L.lr], X01[4 * u + L.lk][16 * L.qb + L.lr], wq, 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int k = 16 * L.qa + L.lk + 4 * t, cc = 16 * L.qb + L.lr;
        const double e = wq[t] * gmw_pivot_rcp(Dv[k]);
        Wc[k][cc] = wq[t];
        Lr[k][cc] = e;
        also(k, cc, e);
    }
}
// C2: quarter of X11 -= E'^T W1d -> Xm of factor 2
__device__ __forceinline__ void gmw_c2(const GmwLane& L, const double (*X11)[32], const double (*Lr)[G64_LS], const double (*Wc)[G64_LS], double (*Xm2)[32])
{
    d4 x = gmw_quarter_load(L, X11);
    gmw_quarter_update<0, 32>(L, Lr, Wc, x);
    gmw_quarter_store(L, Xm2, x);
}

// ---- panel buffer ----
// one wave: E' (rows 0..31 of Lr) -> nxt->E
template <bool DEV>
__device__ __forceinline__ void gmw_store_e(const GmwLane& L, const double (*Lr)[G64_LS], double* __restrict__ E)
{
    const int c4 = (L.lane & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int row = 8 * i + (L.lane >> 3);
        st_d4<DEV>(&E[row * 32 + c4], *(const d4*)&Lr[row][c4]);
    }
}
// Waves 1 / 3 of a persistent pivot while factor 2 runs, in the order of who is waiting for what:
//   1. the first half of the panel buffer, agent scope (wave 1: E' and the pivots of sub-panel 1; wave 3: T1');
//   2. half_stored(): the caller waits for these stores and raises its half flag there;
//   3. the (0,1) tile of S (wave 3) and the S rows / pivots of both factors as the pivot wave produces them (lsq / lrc: workgroup-local
//      copies of sqrt(D)/D and 1/D, or null; before_last(): gmw_cols_out_wave's hook, factor 2 only).
template <class Half, class Hook = GmwNoHook>
__device__ __forceinline__ void gmw_factor2_outputs(const GmwLane& L, const GmwColsLds& ws, const GmwColsLds& ws2, bool half_only, const double* T1,
                                                    const double (*Lr)[G64_LS], const double (*Wc)[G64_LS], GmwPanel64* __restrict__ nxt, int n, int ld, int base,
                                                    double* __restrict__ Dall, double* __restrict__ Sout, double* lsq, double* lrc,
                                                    Half&& half_stored, Hook&& before_last = Hook())
{
    const bool wv1 = L.wvu == 1;
    if (wv1) {
        gmw_store_e<true>(L, Lr, nxt->E);
        if (L.lane < 32) {
            const double D = ws.Dv[L.lane], rc = gmw_pivot_rcp(D), sq = sqrt(D) * rc;
            st_dev(&nxt->D[L.lane], D); st_dev(&nxt->sq[L.lane], sq); st_dev(&nxt->rD[L.lane], rc);
        }
    } else gmw_copy_t<true>(T1, nxt->Tt1, L.lane);
    half_stored();
    if (!wv1) gmw_s01_rows(L, ws.Dv, Wc, Sout, n, ld, base);
    gmw_cols_out_wave<true>(ws, wv1 ? 0 : 1, L.lane, n, ld, base, nxt->D, nxt->sq, nxt->rD, Dall, Sout, lsq, lrc);
    if (!half_only) gmw_cols_out_wave<true>(ws2, wv1 ? 0 : 1, L.lane, n, ld, base + 32, nxt->D + 32, nxt->sq + 32, nxt->rD + 32, Dall, Sout,
                                            lsq ? lsq + 32 : nullptr, lsq ? lrc + 32 : nullptr, before_last);
}
