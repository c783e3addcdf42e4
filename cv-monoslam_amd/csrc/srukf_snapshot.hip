// srukf_snapshot.hip — the state a block of image frames can be resumed from (srukf_images_snapshots / srukf_images_resume).
// k_image_snapshot is the first launch of a frame of an image run with the switch on: while the device knows of no stop in the block, it copies X, S, the matchPatch
// array and the policy state into slot (frame & 1) and tags the slot with the frame.  Nothing else in the frame reads what it writes.
// The guard G(f) — "as far as the device knows, the host will still consume frame f - 1" — is a latch, double-buffered by frame parity:
//   G(b0) = true,  G(f) = G(f - 1) && !outlier[f - 1] && !(f - 2 >= b0 && change[f - 2])
// (while the rescue gate is on, DESIGN.md section 27: n_high[f - 1] > 0, "frame f - 1 rescued a match", in outlier[f - 1]'s place; written behind that frame's tail)
// Every workgroup of frame f's launch forms G(f) from latch[(f - 1) & 1] (written by frame f - 1's launch), the consensus summary of frame f - 1 (written inside that
// frame) and the policy summary of frame f - 2 (its launch sits in front of frame f - 1); thread 0 of workgroup 0 stores it in latch[f & 1] for frame f + 1's launch.
// The only dependencies are launch boundaries on the stream: no polling, no atomics, and no word one workgroup of a launch writes and another of the same launch reads
// (latch[f & 1] and latch[(f - 1) & 1] are different words).

#include "srukf_launch.h"

// 16 bytes per lane and trip; `bytes` need not be a multiple of 16: the last < 16 bytes go one by one (workgroup 0).  src / dst are 16-byte aligned (device allocations)
static __device__ __forceinline__ void snap_copy(void* __restrict__ dst, const void* __restrict__ src, size_t bytes, size_t tid, size_t nthreads)
{
    const size_t n16 = bytes >> 4;
    const uint4* __restrict__ s = (const uint4*)src;
    uint4* __restrict__ d = (uint4*)dst;
    for (size_t i = tid; i < n16; i += nthreads) d[i] = s[i];
    const size_t done = n16 << 4;
    if (tid < bytes - done) ((unsigned char*)dst)[done + tid] = ((const unsigned char*)src)[done + tid];
}

__global__ __launch_bounds__(256) void k_image_snapshot(const FrameScalars* __restrict__ fs, const SnapshotArgs* __restrict__ args, SnapshotCtl* __restrict__ ctl, ImageSnapshot sn)
{
    const int f = fs->frame;
    const int b0 = args->b0;
    bool g = true;
    if (f > b0) {
        g = ctl->latch[(f - 1) & 1] != 0;
        const RansacSummary* rs = args->rs_sum;
        const RescueSummary* rq = args->rq_sum;                 // the rescue gate is on: frame f - 1 stops the block only if it rescued a match
        if (rs && (rq ? rq[f - 1].n_high > 0 : rs[f - 1].outlier != 0)) g = false;
        const srukf_policy_summary* ps = args->pol_sum;
        if (ps && f - 2 >= b0 && ps[f - 2].change) g = false;
    }
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (first) ctl->latch[f & 1] = g ? 1 : 0;
    if (!g) return;
    const int slot = f & 1;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
    snap_copy(sn.S[slot], sn.S_src, sn.S_bytes, tid, nth);
    snap_copy(sn.X[slot], sn.X_src, sn.X_bytes, tid, nth);
    snap_copy(sn.tmpl[slot], sn.tmpl_src, sn.tmpl_bytes, tid, nth);
    const srukf_policy_state* pst = args->pol_state;
    if (pst) snap_copy(sn.pol[slot], pst, sn.pol_bytes, tid, nth);
    if (first) ctl->tag[slot] = f;
}

// *dst = v in stream order, as the other parameter blocks of an image run are written; begin: a block begins — no slot holds a state of it, the latch is open
__global__ void k_set_snapshot_args(SnapshotArgs* dst, SnapshotArgs v, SnapshotCtl* ctl, int begin)
{
    *dst = v;
    if (begin) { ctl->tag[0] = -1; ctl->tag[1] = -1; ctl->latch[0] = 1; ctl->latch[1] = 1; }
}

int image_snapshot_blocks(size_t S_bytes)
{
    const size_t want = (S_bytes / 16 + 256 * SNAPSHOT_TRIPS - 1) / (256 * SNAPSHOT_TRIPS);
    return (int)(want < 1 ? 1 : want > SNAPSHOT_MAX_BLOCKS ? SNAPSHOT_MAX_BLOCKS : want);
}

void launch_image_snapshot(hipStream_t st, const FrameScalars* fs, const SnapshotArgs* args, SnapshotCtl* ctl, const ImageSnapshot& sn)
{
    hipLaunchKernelGGL(k_image_snapshot, dim3(image_snapshot_blocks(sn.S_bytes)), dim3(256), 0, st, fs, args, ctl, sn);
}
void launch_set_snapshot_args(hipStream_t st, SnapshotArgs* dst, SnapshotArgs v, SnapshotCtl* ctl, int begin)
{
    hipLaunchKernelGGL(k_set_snapshot_args, dim3(1), dim3(1), 0, st, dst, v, ctl, begin);
}
