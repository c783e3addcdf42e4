// srukf_images.hip — image runs of the staged replay (DESIGN.md sections 20 - 27, 29): the staged gray frames and the frames that associate on the device
// (srukf_stage_images / srukf_run_images*), their per-frame options — the checked association (srukf_run_images_checked*), the archive search
// (srukf_images_search_archive), the map policy's verdict (srukf_images_policy), the 1-point RANSAC consensus (srukf_images_ransac), its rescue gate
// (srukf_images_rescue_gate), the snapshots (srukf_images_snapshots / _resume) and the display view (srukf_images_display, with the overlay of any staged frame,
// srukf_render_image_overlay), colour frames in the staged stack and the overlays of a run of frames (srukf_stage_images_bgr, srukf_get_staged_image,
// srukf_render_image_overlays; section 29) — and the getters of their records.  No kernel: the launch sequences, the graph cache and srukf_synchronize are srukf_replay.hip's;
// what the two files share is declared once in srukf_ctx.h.
// A further per-frame option is: its switch on the handle and its members of ImageReplay (srukf_ctx.h); one group of image_group, each record column with its row
// and whether a restored block's rows stand; in run_images_issue one image_group_ensure and the parameters' launch; a captured launch: one bit of ImageForm and one
// branch of replay_one_image_frame, an eager one behind each frame: one issue_image_* at the three issue sites; a getter built from image_getter_front and
// image_rows_get.  Allocation, freeing, images_restore and the row arithmetic need no line

#include "srukf_ctx.h"
using namespace srukf_impl;

namespace srukf_impl {

// Every device buffer of the image runs, by group, named ONCE.  buf: { address of the pointer, bytes, zeroed when allocated }.  col: a per-frame record column —
// frames rows of `row` bytes, zeroed (rows no run has written read as zero); THE place a column's row width is written: allocation, images_restore and the getters
// take it from here (image_col).  block: the rows a restored block wrote do not stand (images_restore zeroes them); the association's and the checked record keep
// them.  The archive record is the one exception: a single allocation laid out column-major over frames (ImageArchiveRecord, srukf_launch.h), invalidated whole
// (ar_valid) — srukf_get_image_archive and seq_archive_search do its arithmetic.
// image_buffers_alloc allocates a group, images_drop and images_archive_drop free through the same lists: a buffer added HERE is freed without anyone remembering
// to list it.  The sizes are the allocation's (image_bytes: of one staged frame, L: the archive's; whoever only frees passes neither).  Not zeroed: the parameter
// blocks (written in stream order in front of every run that reads them), the images, xyz and the copies of the state
enum ImageGroup { IMG_STAGED, IMG_CHECKED, IMG_ARCHIVE, IMG_POLICY, IMG_RANSAC, IMG_SNAPSHOT, IMG_RESCUE, IMG_DISPLAY, IMG_COLOUR, IMG_OVERLAYS, IMG_GROUPS };
struct ImageBuf { void** p; size_t bytes; bool zero; size_t row; bool block; };
struct ImageStateBytes { size_t X, S, tmpl, pol; };
static ImageStateBytes image_state_bytes(const KDims& d)
{
    const size_t np = d.np, N = d.N;
    return { sizeof(double) * np, sizeof(double) * np * np, N * PT_TMPL_STRIDE, sizeof(srukf_policy_state) * N };
}
static std::vector<ImageBuf> image_group(srukf_map_scope* c, ImageGroup g, size_t image_bytes = 0, size_t L = 0)
{
    ImageReplay& im = c->img;
    const size_t N = c->d.N, mp = c->d.mp, f = (size_t)im.frames, D = sizeof(double), I = sizeof(int);
    const ImageStateBytes sb = image_state_bytes(c->d);
    auto buf = [](auto** p, size_t bytes, bool zero = false) { return ImageBuf{ (void**)p, bytes, zero, 0, false }; };
    auto col = [f](auto** p, size_t row, bool block) { return ImageBuf{ (void**)p, f * row, true, row, block }; };
    switch (g) {
    case IMG_STAGED: return { buf(&im.images, f * image_bytes), col(&im.corr_seq, D * N, false), col(&im.vis_seq, I * N, false), col(&im.h_seq, D * 2 * N, false),
                              buf(&im.xyz, D * 3 * N), buf(&im.ck.tmpl, sb.tmpl), buf(&im.ck.S, sb.S), buf(&im.ck.X, sb.X) };
    case IMG_CHECKED: return { col(&im.corr2_seq, D * N, false), col(&im.z2_seq, D * 2 * N, false), col(&im.flags_seq, I * N, false), buf(&im.match_args, sizeof(MatchArgs)) };
    case IMG_ARCHIVE: return { buf(&im.ar_rec, D * image_archive_record(f, L).doubles, true), buf(&im.ar_args, sizeof(ArchiveArgs)) };
    case IMG_POLICY: return { buf(&im.pol_state, sb.pol, true), buf(&im.ck.pol, sb.pol, true), col(&im.pol_verdict, I * N, true),
                              col(&im.pol_sum, sizeof(srukf_policy_summary), true), buf(&im.pol_args, sizeof(srukf_policy_params)) };
    case IMG_RANSAC: return { buf(&im.rs_D, D * N * N, true), buf(&im.rs_F, (N * N + 7) / 8 * 8, true), buf(&im.rs_votes, I * N, true), col(&im.rs_flags, I * N, true),
                              col(&im.rs_rvotes, I * N, true), col(&im.rs_dist, D * N, true), col(&im.rs_sum, sizeof(RansacSummary), true), buf(&im.rs_args, sizeof(RansacArgs)) };
    case IMG_SNAPSHOT: return { buf(&im.sn[0].S, sb.S), buf(&im.sn[1].S, sb.S), buf(&im.sn[0].X, sb.X), buf(&im.sn[1].X, sb.X), buf(&im.sn[0].tmpl, sb.tmpl), buf(&im.sn[1].tmpl, sb.tmpl),
                                buf(&im.sn[0].pol, sb.pol), buf(&im.sn[1].pol, sb.pol), buf(&im.sn_ctl, sizeof(SnapshotCtl)), buf(&im.sn_args, sizeof(SnapshotArgs)) };
    case IMG_RESCUE: return { col(&im.rq_flags, I * N, true), col(&im.rq_h2, D * 2 * N, true), col(&im.rq_Si2, D * 4 * N, true), col(&im.rq_chi2, D * N, true),
                              col(&im.rq_sum, sizeof(RescueSummary), true), buf(&im.rq_vis, I * N, true), buf(&im.rq_PxyR, D * 5 * mp, true), buf(&im.rq_args, sizeof(RescueArgs)) };
    case IMG_DISPLAY: return { col(&im.dp_rec, D * image_display_row(N).doubles, true), col(&im.dp_rot, I * N, true) };
    case IMG_COLOUR: return { buf(&im.bgr, 12 * ((im.bgr_pix + 3) / 4)) };      // (whole groups of four pixels: what k_bgr2gray and k_overlay* may read)
    case IMG_OVERLAYS: return { buf(&im.ovs_out, (size_t)im.ovs_count * 3 * image_bytes), buf(&im.ovs_rec, (size_t)im.ovs_count * overlay_rec_bytes((int)N)) };
    default: return {};
    }
}

// the entry of record column *col in its group's list, and where a frame's row of it begins
template <class T> static const ImageBuf& image_col(const std::vector<ImageBuf>& cols, T* const* col)
{
    for (const ImageBuf& b : cols) if ((const void*)b.p == (const void*)col && b.row) return b;
    fprintf(stderr, "image_col: not a record column of this group\n");
    abort();
}
template <class T> static T* image_row(const std::vector<ImageBuf>& cols, T* const* col, size_t frame) { return (T*)((char*)*col + frame * image_col(cols, col).row); }

static void image_buffers_free(const std::vector<ImageBuf>& bufs, hipStream_t st)
{
    for (const ImageBuf& b : bufs) if (*b.p) { srukf_dfree_on(*b.p, st); *b.p = nullptr; }
}

// a group allocated outside any capture, zeroed in stream order where marked; on any failure the whole group is freed and nulled, the sticky HIP error cleared
static int image_buffers_alloc(srukf_ctx* c, const std::vector<ImageBuf>& bufs, const char* who)
{
    hipError_t e = hipSuccess;
    for (const ImageBuf& b : bufs) if (e == hipSuccess) e = srukf_dmalloc_raw(b.p, b.bytes);
    for (const ImageBuf& b : bufs) if (e == hipSuccess && b.zero) e = hipMemsetAsync(*b.p, 0, b.bytes, c->stream);
    if (e == hipSuccess) return SRUKF_OK;
    (void)hipGetLastError();
    image_buffers_free(bufs, c->stream);
    c->err = std::string(who) + ": out of device memory"; return SRUKF_ERR_NOMEM;
}

// what an option needs beyond srukf_stage_images' buffers, allocated in front of the first run that needs it, never inside a capture (the captured frames hold the
// pointers): a group is all there or not at all, so its first buffer answers for it
static int image_group_ensure(srukf_ctx* c, ImageGroup g, const char* who, size_t L = 0)
{
    const std::vector<ImageBuf> bufs = image_group(c, g, 0, L);
    return *bufs.front().p ? SRUKF_OK : image_buffers_alloc(c, bufs, who);
}

// the archive changes (srukf_archive_set): the searching frames were captured with its pointers and L workgroups, the record is sized by L.  The next searching run
// builds both again (images_archive_ensure)
void images_archive_drop(srukf_map_scope* c, hipStream_t st)
{
    ImageReplay& im = c->img;
    for (int i = 0; i < IMAGE_FORM_ROWS; i++) if (ImageForm::at(i).search) for (int m = 0; m < 2; m++) graphs_destroy(im.graphs[i][m]);
    image_buffers_free(image_group(c, IMG_ARCHIVE), st);
    im.ar_L = 0; im.ar_valid = false;
}

void images_drop(srukf_map_scope* c, hipStream_t st)
{
    ImageReplay& im = c->img;
    if (im.images) drop_graphs(c);                               // (the captured image frames hold these pointers)
    for (int g = 0; g < IMG_GROUPS; g++) image_buffers_free(image_group(c, (ImageGroup)g), st);
    im = ImageReplay{};
}

// { X, S, the matchPatch array, the policy state } from one place to another in stream order (the matchPatches' pixels persist from frame to frame, so a block that
// does not stand must not leave its own behind); the policy state only while the policy group exists.  The first error, every copy issued
static ImageState image_state_live(srukf_ctx* c) { return ImageState{ c->X, c->S, c->app_tmpl, c->img.pol_state }; }
static hipError_t image_state_copy(srukf_ctx* c, const ImageState& to, const ImageState& from)
{
    const ImageStateBytes sb = image_state_bytes(c->d);
    const hipError_t e[4] = { hipMemcpyAsync(to.S, from.S, sb.S, hipMemcpyDeviceToDevice, c->stream), hipMemcpyAsync(to.X, from.X, sb.X, hipMemcpyDeviceToDevice, c->stream),
                              hipMemcpyAsync(to.tmpl, from.tmpl, sb.tmpl, hipMemcpyDeviceToDevice, c->stream),
                              c->img.pol_state ? hipMemcpyAsync(to.pol, from.pol, sb.pol, hipMemcpyDeviceToDevice, c->stream) : hipSuccess };
    for (const hipError_t q : e) if (q != hipSuccess) return q;
    return hipSuccess;
}

// A frame of an image run (srukf_run_images*): the plain frame form as in replay_one_frame_joint, whatever "fused_motion" and its neighbours say,
// with the association between k_pxy and what stands in k_gain's place.  Behind seq_pxy(FORM_PLAIN) the device holds h, Si, visible and the predicted pose in X: what
// k_warp_patch and the matching front read (srukf_associate finds the same behind srukf_predict_measurement).  k_associate_staged writes this frame's rows of z_seq /
// m_seq, which k_gain / the joint kernels then read as they read staged rows.  BATCHED: seq_gain_only — seq_gain is seq_pxy + seq_gain_only in this form (no gain fold
// below "fused tail" mode), and k_pxy has run.  The points go to the image state's own scratch, not c->G.
// joint_ensure has run for JOINT (run_images_async: never inside a capture)
// form (ImageForm, srukf_ctx.h):
// checked: a frame of a checked image run — the same frame with k_associate_checked_staged in k_associate_staged's place; images_checked_ensure has run
// search: a frame of a searching image run — the same frame with the archive search behind its tail, on the posterior (seq_archive_search: it
// writes the archive's own buffers and the search record, nothing the filter reads); images_archive_ensure has run
// ransac: a frame with the 1-point RANSAC consensus in it (srukf_images_ransac) — two more launches between the association and what stands in
// k_gain's place: c->Ut is still S^T DZ there, PxyR / h / Si / vis / X are the predicted frame's, and this frame's rows of z_seq / m_seq are written: what
// k_ransac_votes reads.  The pick launch rewrites the m_seq row to the consensus set, which the update then takes for its matches
// rescue (only with ransac): a frame with the rescue gate behind its tail (srukf_images_rescue_gate) — two more launches on the posterior, in
// front of the archive search: they read X, S, the frame's row of z_seq and of the consensus record and write the gate's own record
// snap: a frame that keeps the state it starts from while no stop of the block is on record (srukf_images_snapshots) — k_image_snapshot in front
// of everything else: it reads X, S, the matchPatch array, the policy state and fs->frame as the frame before left them
// (every form's group is allocated: run_images_issue's image_group_ensure, never inside a capture)
static void replay_one_image_frame(srukf_ctx* c, int mode, ImageForm form)
{
    ImageReplay& im = c->img;
    const KDims& d = c->d;
    if (form.snap) {
        const ImageStateBytes sb = image_state_bytes(d);
        const ImageState* sn = im.sn;
        ProfScope ps(c, KC_MISC, 0, 2.0 * sb.S);
        launch_image_snapshot(c->stream, c->fs, im.sn_args, im.sn_ctl, ImageSnapshot{ c->X, c->S, c->app_tmpl, sb.X, sb.S, sb.tmpl, sb.pol,
                              { sn[0].X, sn[1].X }, { sn[0].S, sn[1].S }, { sn[0].tmpl, sn[1].tmpl }, { sn[0].pol, sn[1].pol } });
    }
    seq_predict_motion(c, nullptr);
    seq_predict_measurement(c, FORM_PLAIN);
    seq_pxy(c, FORM_PLAIN);
    {
        ProfScope ps(c, KC_MISC, 0, (double)(PT_REGION_W * PT_REGION_W + PT_TMPL_BYTES + PT_PATCH_BYTES) * d.N);
        srukf_launch_landmarks_cartesian(c->stream, d, c->X, c->S, im.xyz, nullptr);      // the points only
        srukf_launch_warp_patch(c->stream, d, c->p, c->X, im.xyz, c->h, c->appR, c->appT, c->appPx, c->app_patch, c->has_app, c->app_tmpl);
        const StagedAssoc rec = { im.images, im.frames, c->z_seq, c->m_seq, im.corr_seq, im.vis_seq, im.h_seq, c->fs };
        if (form.checked)
            srukf_launch_associate_checked_staged(c->stream, d, c->p, StagedChecked{ rec, im.corr2_seq, im.z2_seq, im.flags_seq, c->match_scores, im.match_args },
                                                  c->h, c->Si, c->vis, c->has_app, c->app_tmpl);
        else
        srukf_launch_associate_staged(c->stream, d, c->p, rec, c->h, c->Si, c->vis, c->has_app, c->app_tmpl);
    }
    if (form.ransac) {
        ProfScope ps(c, KC_MISC, 60.0 * d.N * d.N, 9.0 * d.N * d.N + 16.0 * 12 * d.N * d.N);
        launch_ransac_staged(c->stream, d, c->w, c->p, StagedRansac{ im.frames, c->z_seq, c->m_seq, c->fs, im.rs_args, im.rs_D, im.rs_F, im.rs_votes,
                                                                     im.rs_flags, im.rs_rvotes, im.rs_dist, im.rs_sum }, c->X, c->Ut, c->PxyR, c->h, c->Si, c->vis);
    }
    if (mode == SRUKF_UPDATE_JOINT) seq_joint_launches(c, nullptr, nullptr);
    else seq_gain_only(c, nullptr, nullptr, FORM_PLAIN);
    seq_refactor(c, refactor_frame_tail(c), FORM_PLAIN);
    if (form.ransac && form.rescue) {
        ProfScope ps(c, KC_MISC, 0, 16.0 * d.np);
        launch_rescue_gate_staged(c->stream, d, c->w, c->p, StagedRescue{ im.frames, c->z_seq, c->fs, im.rq_args, im.rs_flags, im.rs_sum,
                                  RescueRow{ im.rq_flags, im.rq_h2, im.rq_Si2, im.rq_chi2 }, im.rq_sum, RescueScratch{ im.rq_vis, im.rq_PxyR } }, c->X, c->S);
    }
    if (form.search) seq_archive_search(c);
}

// ---- what the getters of the records are built from ----
// The common front: rows [first, first + count) of the staged stack are asked for.  no_record: the getter refuses without its record, in these words (null: there
// is one, or the getter reads an unallocated record as zeros); wait: the stream is waited for, as srukf_get_image_matches waits (flags of frames in flight are
// still srukf_synchronize's to report)
static int image_getter_front(srukf_ctx* c, const char* who, int first, int count, const char* no_record = nullptr, bool wait = true)
{
    if (!c || first < 0 || count < 1) return SRUKF_ERR_BAD_ARG;
    const std::string w = who;
    if (!c->img.images) { c->err = w + ": no staged images (srukf_stage_images)"; return SRUKF_ERR_SEQUENCE; }
    if (no_record) { c->err = w + ": " + no_record; return SRUKF_ERR_SEQUENCE; }
    if (first + count > c->img.frames) { c->err = w + ": frames outside the staged images"; return SRUKF_ERR_DIM_MISMATCH; }
    if (!wait) return SRUKF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SRUKF_OK;
}

// rows [first, first + count) of `row` bytes from src to the host, when the caller wants them; a column no run has allocated reads as zeros
static int image_rows_copy(srukf_ctx* c, void* dst, const void* src, size_t row, int first, int count)
{
    if (!dst) return SRUKF_OK;
    if (!src) { memset(dst, 0, (size_t)count * row); return SRUKF_OK; }
    HIPCHK(c, hipMemcpy(dst, (const char*)src + (size_t)first * row, (size_t)count * row, hipMemcpyDeviceToHost));
    return SRUKF_OK;
}
template <class T> static int image_rows_get(srukf_ctx* c, const std::vector<ImageBuf>& cols, T* const* col, int first, int count, T* dst)
{
    return image_rows_copy(c, dst, *col, image_col(cols, col).row, first, count);
}

// rows [first, first + count) of a summary column into sm; *first_hit (may be null): the lowest frame of the range whose summary satisfies hit, or -1
template <class S, class Hit> static int image_summaries_get(srukf_ctx* c, const std::vector<ImageBuf>& cols, S* const* col, int first, int count, std::vector<S>& sm, int* first_hit, Hit hit)
{
    sm.resize((size_t)count);
    const int rc = image_rows_get(c, cols, col, first, count, sm.data()); if (rc) return rc;
    if (!first_hit) return SRUKF_OK;
    *first_hit = -1;
    for (int q = 0; q < count && *first_hit < 0; q++) if (hit(sm[(size_t)q])) *first_hit = first + q;
    return SRUKF_OK;
}

// the state the block of image frames started from comes back (the checkpoint), as srukf_run_frames' checkpoint comes back, and every block-scoped record column is
// zeroed from the block's first row on: what its frames wrote are no verdicts, consensus sets or views any more (DESIGN.md sections 23 - 27).  Keeps c->err
// slot >= 0 (srukf_images_resume): snapshot slot `slot` in the checkpoint's place — the state frame `stop` of the stack started from; rows
// >= stop go, the rows in front of it stand, and the null rows are what the block's frames left (stop lies behind its first frame)
static void images_restore(srukf_ctx* c, int slot = -1, int stop = 0)
{
    ImageReplay& im = c->img;
    const std::string why = c->err;
    const bool ck = slot < 0;
    const size_t r0 = ck ? 0 : (size_t)stop, rows = (size_t)im.frames - r0;
    (void)image_state_copy(c, image_state_live(c), ck ? im.ck : im.sn[slot]);
    for (int g = 0; g < IMG_GROUPS; g++)
        for (const ImageBuf& b : image_group(c, (ImageGroup)g)) if (b.block && *b.p && rows) hipMemsetAsync((char*)*b.p + r0 * b.row, 0, rows * b.row, c->stream);
    if (im.dp_rec) std::fill(im.dp_rows.begin() + (std::ptrdiff_t)r0, im.dp_rows.end(), (unsigned char)0);      // (the host's marks of the display rows)
    if (ck && c->null_canonical != im.ck_canon) { c->null_canonical = im.ck_canon; drop_graphs(c); }
    shadow_rebuild(c);
    hipStreamSynchronize(c->stream);
    c->err = why;
}

void images_block_end(srukf_ctx* c, bool read, bool flagged)
{
    ImageReplay& im = c->img;
    const bool image_run = im.pending, checked_run = im.checked, search_run = im.searching;
    im.pending = false; im.checked = false; im.searching = false;
    if (!image_run || !read) return;
    if (!flagged) { im.ck_clean = true; return; }                // the block ended clean: its checkpoint is what srukf_images_rewind puts back
    images_restore(c);
    c->joint_bad_host = false;
    if (checked_run) c->match_valid = false;                     // a checked run among the frames: a flagged block leaves no valid score map ...
    if (search_run) im.ar_valid = false;                         // ... a searching run: no valid search record
}

}  // namespace srukf_impl

extern "C" {

// ---- image runs: the staged replay with the association on the device ----

// The gray frames of the staged sequence, copied to the device once; with them the per-frame record, the scratch for the Cartesian points and the block's checkpoint
// (X, S, matchPatch): everything an image run needs that can fail for want of memory is allocated here, outside any capture.
// One body behind srukf_stage_images (colour < 0: src is the gray stack) and srukf_stage_images_bgr (colour = keep_colour: src is F frames of B, G, R bytes).
// The colour route: both stacks are tight, so the F frames are one run of F W H pixels and k_bgr2gray converts it as it converts one frame — its groups of four
// pixels count from the start of the STACK, dword-aligned in both buffers wherever a frame begins, and only the stack's last group can be a partial one (its gray
// bytes go one by one, inside [0, F W H)).  The run is walked in chunks of STAGE_CHUNK pixels, a multiple of four, each copied and converted in stream order:
// with keep_colour = 0 the colour bytes pass through ONE transit buffer of min(F W H, STAGE_CHUNK) pixels — at most 12 MiB — which the next chunk's copy
// overwrites behind this chunk's launch; it is freed before the call returns.  The chunk also keeps every index of a launch below 2^31
constexpr size_t STAGE_CHUNK = (size_t)1 << 22;                  // pixels; a multiple of four
static int stage_images_any(srukf_ctx* c, int F, const unsigned char* src, int colour, const char* who)
{
    const std::string w = who;
    if (!c->odo_seq) { c->err = w + ": no staged sequence (srukf_stage_sequence first)"; return SRUKF_ERR_SEQUENCE; }
    if (F != c->seqF) { c->err = w + ": n_frames is not the staged sequence's"; return SRUKF_ERR_DIM_MISMATCH; }
    if (c->d.N < 1) { c->err = w + ": the map is empty"; return SRUKF_ERR_DIM_MISMATCH; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));             // frames in flight may still read the images staged before
    images_drop(c, c->stream);
    int rc = ensure_appearance(c); if (rc) return rc;
    ImageReplay& im = c->img;
    const size_t img = (size_t)c->p.image_w * (size_t)c->p.image_h, total = (size_t)F * img;
    im.frames = F;                                          // (the group's sizes)
    rc = image_buffers_alloc(c, image_group(c, IMG_STAGED, img), who);
    if (rc) { images_drop(c, c->stream); return rc; }
    hipError_t e = hipSuccess;
    if (colour < 0) e = hipMemcpy(im.images, src, total, hipMemcpyHostToDevice);
    else {
        im.bgr_kept = colour != 0;
        im.bgr_pix = im.bgr_kept ? total : std::min(total, STAGE_CHUNK);
        rc = image_buffers_alloc(c, image_group(c, IMG_COLOUR), who);
        if (rc) { images_drop(c, c->stream); return rc; }
        for (size_t off = 0; off < total && e == hipSuccess; off += STAGE_CHUNK) {
            const size_t n = std::min(total - off, STAGE_CHUNK);
            unsigned char* d = im.bgr_kept ? im.bgr + 3 * off : im.bgr;
            e = hipMemcpyAsync(d, src + 3 * off, 3 * n, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) break;
            ProfScope ps(c, KC_BGR2GRAY, 0, 4.0 * (double)n);
            launch_bgr2gray(c->stream, (int)n, d, im.images + off);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // (src is the caller's pageable memory)
    if (e != hipSuccess) { images_drop(c, c->stream); c->err = w + ": " + hipGetErrorString(e); return SRUKF_ERR_HIP; }
    if (colour == 0) { image_buffers_free(image_group(c, IMG_COLOUR), c->stream); im.bgr_pix = 0; }      // the transit buffer
    return SRUKF_OK;
}

int srukf_stage_images(srukf_ctx* c, int F, const unsigned char* gray)
{
    if (!c || F < 1 || !gray) return SRUKF_ERR_BAD_ARG;
    return stage_images_any(c, F, gray, -1, "stage_images");
}

// loadPictures (SLAM.cpp:529-543) for the whole stack: F colour frames become the staged gray frames, by srukf_set_frame_bgr's rule (k_bgr2gray), and with
// keep_colour the colour stack stays beside them as the overlays' source.  Behind the call the handle is what srukf_stage_images with the converted bytes leaves;
// the held frame (d_image, d_bgr) is neither read nor written
int srukf_stage_images_bgr(srukf_ctx* c, int F, const unsigned char* bgr, int keep_colour)
{
    if (!c || F < 1 || !bgr || (keep_colour != 0 && keep_colour != 1)) return SRUKF_ERR_BAD_ARG;
    return stage_images_any(c, F, bgr, keep_colour, "stage_images_bgr");
}

// frame `frame` of the staged stack: its gray bytes and, from a kept colour stack, its colour bytes.  Waits for the stream
int srukf_get_staged_image(srukf_ctx* c, int frame, unsigned char* gray_out, unsigned char* bgr_out)
{
    if (!c || frame < 0 || (!gray_out && !bgr_out)) return SRUKF_ERR_BAD_ARG;
    const ImageReplay& im = c->img;
    if (!im.images) { c->err = "get_staged_image: no staged images (srukf_stage_images)"; return SRUKF_ERR_SEQUENCE; }
    if (frame >= im.frames) { c->err = "get_staged_image: frame outside the staged images"; return SRUKF_ERR_BAD_ARG; }
    if (bgr_out && !im.bgr_kept) { c->err = "get_staged_image: no colour stack is kept (srukf_stage_images_bgr with keep_colour)"; return SRUKF_ERR_SEQUENCE; }
    const size_t img = (size_t)c->p.image_w * (size_t)c->p.image_h, f = (size_t)frame;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (gray_out) HIPCHK(c, hipMemcpy(gray_out, im.images + f * img, img, hipMemcpyDeviceToHost));
    if (bgr_out) HIPCHK(c, hipMemcpy(bgr_out, im.bgr + 3 * f * img, 3 * img, hipMemcpyDeviceToHost));
    return SRUKF_OK;
}

// The three options whose first run needs more than their group (image_group_ensure):
// a checked image run — the filter's score buffer if no srukf_associate_checked has made it.  Captured checked frames hold the score buffer's pointer: they are
// dropped when it is not the one they were captured with (match_drop has run in between)
static int images_checked_ensure(srukf_ctx* c, const char* who)
{
    ImageReplay& im = c->img;
    int rc = match_ensure(c, who); if (rc) return rc;
    if (im.chk_scores != c->match_scores) {
        for (int i = 0; i < IMAGE_FORM_ROWS; i++) if (ImageForm::at(i).checked && (im.graphs[i][0].one_exec || im.graphs[i][1].one_exec)) { HIPCHK(c, hipStreamSynchronize(c->stream)); drop_graphs(c); break; }
        im.chk_scores = c->match_scores;
    }
    return image_group_ensure(c, IMG_CHECKED, who);
}

// a searching image run — the record is sized by the archive's L, kept in ar_L.  srukf_archive_set drops both with the captured searching frames (images_archive_drop)
static int images_archive_ensure(srukf_ctx* c, const char* who)
{
    ImageReplay& im = c->img;
    const bool had = im.ar_rec != nullptr;
    const int rc = image_group_ensure(c, IMG_ARCHIVE, who, (size_t)c->archive.L);
    if (rc == SRUKF_OK && !had) im.ar_L = c->archive.L;
    return rc;
}

// a run with the display view — the host's marks of the record's rows
static int images_display_ensure(srukf_ctx* c, const char* who)
{
    ImageReplay& im = c->img;
    const bool had = im.dp_rec != nullptr;
    const int rc = image_group_ensure(c, IMG_DISPLAY, who);
    if (rc == SRUKF_OK && !had) im.dp_rows.assign((size_t)im.frames, 0);
    return rc;
}

// the display view behind staged frame `frame` (srukf_images_display; updateFeaturesInformation -> refreshFeaturesDisplay, SLAM.cpp:2566-2575, behind every frame):
// two eager launches with the host's row pointers, as the policy's launch carries its frame index — k_image_view (xyz, cov, the robot block and the Si the frame's
// association read, from the posterior X and S), then k_lm_ellipsoid on the row's cov.  They read X, S and c->Si and write the record only
static void issue_image_display(srukf_ctx* c, int frame)
{
    ImageReplay& im = c->img;
    const size_t N = (size_t)c->d.N;
    const ImageDisplayRow r = image_display_row(N);
    double* row = im.dp_rec + (size_t)frame * r.doubles;
    {
        ProfScope ps(c, KC_MISC, 126.0 * N * N, 144.0 * N * N + 8.0 * r.doubles);      // landmark k walks 6 k + 6 rows of S: 21 products and 6 doubles each
        launch_image_view(c->stream, c->d, c->X, c->S, c->Si, row + r.xyz, row + r.cov, row + r.robot, row + r.Si);
    }
    {
        ProfScope ps(c, KC_LM_ELLIPSOID, 0, 8.0 * 16 * N + 4.0 * N);
        launch_lm_ellipsoid(c->stream, (int)N, c->p.epsilon, row + r.cov, row + r.axis, row + r.sigma, im.dp_rot + (size_t)frame * N);
    }
    im.dp_rows[(size_t)frame] = 1;
}

// the map policy's verdict behind staged frame `frame` (srukf_images_policy): an eager launch with the frame index as a kernel argument — fs->frame has advanced
// behind the tail, and a captured frame could not carry the index.  It reads the posterior X and row `frame` of the association's record
static void issue_image_policy(srukf_ctx* c, int frame)
{
    const ImageReplay& im = c->img;
    ProfScope ps(c, KC_MISC, 0, 80.0 * c->d.N);
    launch_map_policy_staged(c->stream, c->d, c->p, im.pol_args, StagedPolicy{ c->X, im.frames, im.h_seq, im.vis_seq, c->z_seq, c->m_seq, im.pol_state, im.pol_verdict, im.pol_sum }, frame);
}

// srukf_run_images_async (chk null) and srukf_run_images_checked_async (chk: the validated parameters): one body, the frames differ in the association launch
static int run_images_issue(srukf_ctx* c, int first, int count, int mode, double* d_traj, const MatchArgs* chk, const char* who)
{
    if (!c || first < 0 || count < 1) return SRUKF_ERR_BAD_ARG;
    const std::string w = who;
    { const int rcm = replay_mode_check(c, mode, who); if (rcm) return rcm; }
    if (c->storage != SRUKF_STORAGE_F64) { c->err = w + ": image runs are available in SRUKF_STORAGE_F64 only"; return SRUKF_ERR_UNSUPPORTED; }
    ImageReplay& im = c->img;
    if (!im.images) { c->err = w + ": no staged images (srukf_stage_images)"; return SRUKF_ERR_SEQUENCE; }
    if (!c->odo_seq || im.frames != c->seqF || first + count > c->seqF) { c->err = "frames outside the staged sequence"; return SRUKF_ERR_DIM_MISMATCH; }
    if (c->async_pending && !im.pending) { c->err = w + ": frames of srukf_run_frames_async are in flight (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    c->joint_bad_host = false;
    HIPCHK(c, hipSetDevice(c->device));
    if (mode == SRUKF_UPDATE_JOINT) { const int rcj = joint_ensure(c, who); if (rcj) return rcj; }      // (before any capture begins)
    const ImageForm form{ chk != nullptr, c->img_search && c->archive.L > 0, c->img_ransac, c->img_snap, c->img_ransac && c->img_rescue };
    if (form.checked) {
        const int rce = images_checked_ensure(c, who); if (rce) return rce;                           // (idem)
        srukf_launch_set_match_args(c->stream, im.match_args, *chk);      // in stream order: behind the frames of an earlier run of the block, in front of this run's
        im.checked = true; c->match_valid = true;
    }
    // the archive search behind every frame (srukf_images_search_archive).  An empty archive: a plain run, and a record of L = 0
    if (c->img_search) {
        if (form.search) {
            const int rca = images_archive_ensure(c, who); if (rca) return rca;                        // (idem)
            launch_set_archive_args(c->stream, im.ar_args, c->img_search_args);      // in stream order, as the checked run's parameters
            im.searching = true;
        }
        im.ar_valid = true;
    }
    // the map policy's verdict behind every frame (srukf_images_policy): no captured frames of its own — the run is issued frame by frame, the one-frame graph
    // followed by the policy launch
    const bool policy = c->img_policy;
    if (policy) {
        const int rcp = image_group_ensure(c, IMG_POLICY, who); if (rcp) return rcp;      // (idem)
        launch_set_policy_params(c->stream, im.pol_args, c->img_policy_args);      // in stream order, as the checked run's parameters
        im.pol_valid = true;
    }
    // the display view behind every frame (srukf_images_display): like the policy no captured frames of its own — the run is issued frame by frame, the one-frame
    // graph followed by the display launches, then the policy's.  The two read the same posterior and write records of their own: their order is fixed (display
    // first), not needed
    const bool display = c->img_display;
    if (display) { const int rcd = images_display_ensure(c, who); if (rcd) return rcd; }                // (idem)
    else if (im.dp_rec) std::fill(im.dp_rows.begin() + first, im.dp_rows.begin() + first + count, (unsigned char)0);      // frames run again without the switch: their rows are an earlier run's, kept but not drawable
    const bool single = policy || display;
    // the 1-point RANSAC consensus inside every frame (srukf_images_ransac): captured frames of their own
    if (form.ransac) {
        const int rcr = image_group_ensure(c, IMG_RANSAC, who); if (rcr) return rcr;      // (idem)
        launch_set_ransac_args(c->stream, im.rs_args, RansacArgs{ c->img_ransac_thr });      // in stream order, as the checked run's parameters
        im.rs_valid = true;
    }
    // the rescue gate behind every such frame (srukf_images_rescue_gate): captured frames of their own; chi2 in stream order, so that changing it needs no recapture
    if (form.rescue) {
        const int rcq = image_group_ensure(c, IMG_RESCUE, who); if (rcq) return rcq;      // (idem)
        launch_set_rescue_args(c->stream, im.rq_args, RescueArgs{ c->img_rescue_chi2 });
        im.rq_valid = true;
    }
    // the state in front of every frame, kept while no stop is on record (srukf_images_snapshots): captured frames of their own.  The guard's parameters go to the
    // device in stream order, as the checked run's; a run that begins a block also closes both slots and opens the latch
    if (form.snap) {
        const int rcs = image_group_ensure(c, IMG_SNAPSHOT, who); if (rcs) return rcs;      // (idem)
        launch_set_snapshot_args(c->stream, im.sn_args, SnapshotArgs{ im.pending ? im.blk_first : first, policy ? im.pol_sum : nullptr, form.ransac ? im.rs_sum : nullptr, im.pol_state,
                                               form.rescue ? im.rq_sum : nullptr },
                                 im.sn_ctl, im.pending ? 0 : 1);
    }
    // the block as srukf_images_resume needs it: resumable while every run of it has the switch on and begins where the one before ended
    if (!im.pending) { im.blk_first = first; im.blk_snap = form.snap; }
    else im.blk_snap = im.blk_snap && form.snap && first == im.blk_end;
    im.blk_end = first + count;
    replay_prologue(c);
    if (!im.pending) {
        // the block's checkpoint: a block is every image run since the last srukf_synchronize
        HIPCHK(c, image_state_copy(c, im.ck, image_state_live(c)));
        im.ck_canon = c->null_canonical;
    }
    double* traj = d_traj ? d_traj - (size_t)8 * first : nullptr;
    int clear = c->async_pending ? 0 : 1;
    if (c->red_r > 0 && !c->null_canonical) {
        // null rows that are not (yet) sqrt(EPSILON) e_k: the run's first frame eagerly, as in srukf_run_frames_async (the plain form reads the rows as they are)
        launch_set_run(c->stream, c->fs, first, clear, traj);
        replay_one_image_frame(c, mode, form);
        if (display) issue_image_display(c, first);
        if (policy) issue_image_policy(c, first);
        set_null_canonical(c);
        im.pending = true; clear = 0;
        first += 1; count -= 1;
        { const int rc = replay_epilogue(c); if (rc) return rc; }
        if (count == 0) return SRUKF_OK;
    }
    launch_set_run(c->stream, c->fs, first, clear, traj);
    if (c->use_graph && !c->profiling) {
        // (the form's own captured frames, per update mode: never a frame captured for another form, nor one without the association)
        ReplayGraphs& g = im.graphs[form.index()][mode == SRUKF_UPDATE_JOINT ? 1 : 0];
        const auto frame = [=] { replay_one_image_frame(c, mode, form); };
        if (!g.one_exec) { const int rc = capture_frames(c, 1, &g.one, &g.one_exec, frame); if (rc) return rc; }
        if (!single && !g.eight_exec) { const int rc = capture_frames(c, SRUKF_GRAPH_FRAMES, &g.eight, &g.eight_exec, frame); if (rc) return rc; }      // (a policy or display run launches single frames only)
        if (single) for (int f = 0; f < count; f++) {
            HIPCHK(c, hipGraphLaunch(g.one_exec, c->stream));
            if (display) issue_image_display(c, first + f);
            if (policy) issue_image_policy(c, first + f);
        }
        else { const int rc = replay_launch_graphs(c, g, count); if (rc) return rc; }
    } else {
        for (int f = 0; f < count; f++) {
            replay_one_image_frame(c, mode, form);
            if (display) issue_image_display(c, first + f);
            if (policy) issue_image_policy(c, first + f);
        }
    }
    im.pending = true;
    return replay_epilogue(c);
}

int srukf_run_images_async(srukf_ctx* c, int first, int count, int mode, double* d_traj) { return run_images_issue(c, first, count, mode, d_traj, nullptr, "run_images_async"); }

// ---- checked image runs: the ambiguity veto and the sub-pixel peak inside an image run ----
// srukf_associate_checked's parameter rules (params null: its defaults)
static int checked_args(srukf_ctx* c, const srukf_match_params* params, MatchArgs* ma)
{
    srukf_match_params mp = { 0.8, 0.9, 4, 0 };
    if (params) mp = *params;
    if (!std::isfinite(mp.ratio) || mp.ratio <= 0.0) { c->err = "run_images_checked: ratio must be finite and positive"; return SRUKF_ERR_BAD_ARG; }
    if (mp.exclusion < 1 || mp.exclusion > 20) { c->err = "run_images_checked: exclusion outside [1, 20]"; return SRUKF_ERR_BAD_ARG; }
    if (!std::isfinite(mp.corr_threshold)) { c->err = "run_images_checked: corr_threshold is not finite"; return SRUKF_ERR_BAD_ARG; }
    *ma = { .corr_threshold = mp.corr_threshold, .ratio = mp.ratio, .exclusion = mp.exclusion, .subpixel = mp.subpixel };
    return SRUKF_OK;
}

int srukf_run_images_checked_async(srukf_ctx* c, int first, int count, int mode, const srukf_match_params* params, double* d_traj)
{
    if (!c || first < 0 || count < 1) return SRUKF_ERR_BAD_ARG;
    MatchArgs ma;
    const int rc = checked_args(c, params, &ma); if (rc) return rc;
    return run_images_issue(c, first, count, mode, d_traj, &ma, "run_images_checked_async");
}

// Synchronous form: as srukf_run_images, no recovery inside the call
int srukf_run_images_checked(srukf_ctx* c, int first, int count, int mode, const srukf_match_params* params, double* traj_host)
{
    if (!c || first < 0 || count < 1) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return with_device_traj(c, count, traj_host, [=](double* dt) { const int rc = srukf_run_images_checked_async(c, first, count, mode, params, dt); return rc ? rc : srukf_synchronize(c); });
}

// rows [first, first + count) of the checked record, after waiting for the stream like srukf_get_image_matches.  Rows no checked run has written are zero (all of
// them before the first checked run); a row a plain image run wrote after a checked one keeps the checked run's values
int srukf_get_image_checks(srukf_ctx* c, int first, int count, double* corr2, double* z2, int* flags)
{
    int rc = image_getter_front(c, "get_image_checks", first, count, nullptr, c && c->img.corr2_seq);
    if (rc) return rc;
    const ImageReplay& im = c->img;
    const std::vector<ImageBuf> cols = image_group(c, IMG_CHECKED);
    rc = image_rows_get(c, cols, &im.corr2_seq, first, count, corr2);
    if (!rc) rc = image_rows_get(c, cols, &im.z2_seq, first, count, z2);
    if (!rc) rc = image_rows_get(c, cols, &im.flags_seq, first, count, flags);
    return rc;
}

// rows [first, first + count) of the record the searching image runs wrote (srukf_images_search_archive), after waiting for the stream like srukf_get_image_matches.
// Rows no searching run has written are zero.  No record (no searching run since the images were staged or the archive was set; a flagged block restored since the
// last one): SRUKF_ERR_SEQUENCE, the rule of srukf_get_match_scores
int srukf_get_image_archive(srukf_ctx* c, int first, int count, int* L, double* h, double* Si, int* visible, double* z, int* matched, double* corr, int* hits)
{
    const size_t n = c && c->img.ar_rec ? (size_t)c->img.ar_L : 0, a = (size_t)first, m = (size_t)count;
    const int rc = image_getter_front(c, "get_image_archive", first, count, c && !c->img.ar_valid ? "no record of a searching image run (srukf_images_search_archive; a flagged block leaves none)" : nullptr,
                                      n > 0);                  // (an empty archive: the runs were plain ones, nothing to wait for)
    if (rc) return rc;
    const ImageReplay& im = c->img;
    if (L) *L = (int)n;
    if (hits) memset(hits, 0, sizeof(int) * m);
    if (n == 0) return SRUKF_OK;
    // (the one record that is no set of columns of image_group: ImageArchiveRecord's blocks, frames x n each)
    const ImageArchiveRecord r = image_archive_record((size_t)im.frames, n);
    const double* rec = im.ar_rec; const int* reci = (const int*)(rec + r.ints);
    if (h) HIPCHK(c, hipMemcpy(h, rec + r.h + a * 2 * n, sizeof(double) * m * 2 * n, hipMemcpyDeviceToHost));
    if (Si) HIPCHK(c, hipMemcpy(Si, rec + r.Si + a * 4 * n, sizeof(double) * m * 4 * n, hipMemcpyDeviceToHost));
    if (z) HIPCHK(c, hipMemcpy(z, rec + r.z + a * 2 * n, sizeof(double) * m * 2 * n, hipMemcpyDeviceToHost));
    if (corr) HIPCHK(c, hipMemcpy(corr, rec + r.corr + a * n, sizeof(double) * m * n, hipMemcpyDeviceToHost));
    if (visible) HIPCHK(c, hipMemcpy(visible, reci + r.vis_i + a * n, sizeof(int) * m * n, hipMemcpyDeviceToHost));
    if (matched) HIPCHK(c, hipMemcpy(matched, reci + r.m_i + a * n, sizeof(int) * m * n, hipMemcpyDeviceToHost));
    if (hits) HIPCHK(c, hipMemcpy(hits, reci + r.hits_i + a, sizeof(int) * m, hipMemcpyDeviceToHost));
    return SRUKF_OK;
}

// ---- the map policy's verdict behind image frames (the kernel and the switch: srukf_policy.hip) ----
// the counters map[] holds (cslam.cpp:713-723) become the device state the next policy run advances
int srukf_images_set_policy_state(srukf_ctx* c, const srukf_policy_state* state)
{
    if (!c || !state) return SRUKF_ERR_BAD_ARG;
    ImageReplay& im = c->img;
    if (!im.images) { c->err = "images_set_policy_state: no staged images (srukf_stage_images)"; return SRUKF_ERR_SEQUENCE; }
    if (c->async_pending) { c->err = "images_set_policy_state: a run is in flight (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    HIPCHK(c, hipSetDevice(c->device));
    const int rc = image_group_ensure(c, IMG_POLICY, "images_set_policy_state"); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(im.pol_state, state, sizeof(srukf_policy_state) * (size_t)c->d.N, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                 // (pageable host memory)
    im.ck_clean = false;                                        // the checkpoint's copy of the state is not this one: no srukf_images_rewind behind a seed
    return SRUKF_OK;
}

// rows [first, first + count) of the policy record (what SLAM.cpp:2443-2459 and 556 would decide behind each frame), after waiting for the stream like
// srukf_get_image_matches; the device state as it stands; the lowest frame of the range that asks for a map change
int srukf_get_image_policy(srukf_ctx* c, int first, int count, int* verdict, srukf_policy_summary* summary, srukf_policy_state* state_out, int* first_change)
{
    int rc = image_getter_front(c, "get_image_policy", first, count, c && !(c->img.pol_state && c->img.pol_valid) ? "no record of a policy run (srukf_images_policy)" : nullptr);
    if (rc) return rc;
    const ImageReplay& im = c->img;
    const std::vector<ImageBuf> cols = image_group(c, IMG_POLICY);
    rc = image_rows_get(c, cols, &im.pol_verdict, first, count, verdict);
    if (!rc) rc = image_rows_copy(c, state_out, im.pol_state, image_state_bytes(c->d).pol, 0, 1);      // (no per-frame column: the state as it stands)
    if (!rc && (summary || first_change)) {
        std::vector<srukf_policy_summary> sm;
        rc = image_summaries_get(c, cols, &im.pol_sum, first, count, sm, first_change, [](const srukf_policy_summary& s) { return s.change != 0; });
        if (!rc && summary) std::copy(sm.begin(), sm.end(), summary);
    }
    return rc;
}

// ---- the 1-point RANSAC consensus inside image frames (the kernels: srukf_ransac.hip) ----
// The switch: on the handle, like srukf_images_policy.  Touches no device: the threshold reaches it in stream order in front of the next image run (run_images_issue)
int srukf_images_ransac(srukf_ctx* c, int on, double threshold)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (on && (!std::isfinite(threshold) || threshold <= 0.0)) { c->err = "images_ransac: threshold must be finite and positive"; return SRUKF_ERR_BAD_ARG; }
    if (c->async_pending) { c->err = "images_ransac: a run is in flight (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    c->img_ransac = on != 0;
    if (on) c->img_ransac_thr = threshold;
    return SRUKF_OK;
}

// rows [first, first + count) of the consensus record, after waiting for the stream like srukf_get_image_matches; the lowest frame of the range whose consensus
// dropped a match
int srukf_get_image_ransac(srukf_ctx* c, int first, int count, int* flags, int* votes, double* dist, int* best, int* n_active, int* n_low, int* first_outlier)
{
    int rc = image_getter_front(c, "get_image_ransac", first, count, c && !(c->img.rs_flags && c->img.rs_valid) ? "no record of a run with the consensus in it (srukf_images_ransac)" : nullptr);
    if (rc) return rc;
    const ImageReplay& im = c->img;
    const std::vector<ImageBuf> cols = image_group(c, IMG_RANSAC);
    rc = image_rows_get(c, cols, &im.rs_flags, first, count, flags);
    if (!rc) rc = image_rows_get(c, cols, &im.rs_rvotes, first, count, votes);
    if (!rc) rc = image_rows_get(c, cols, &im.rs_dist, first, count, dist);
    if (!rc && (best || n_active || n_low || first_outlier)) {
        std::vector<RansacSummary> sm;
        rc = image_summaries_get(c, cols, &im.rs_sum, first, count, sm, first_outlier, [](const RansacSummary& s) { return s.outlier != 0; });
        for (size_t q = 0; !rc && q < sm.size(); q++) {
            if (best) best[q] = sm[q].best;
            if (n_active) n_active[q] = sm[q].n_active;
            if (n_low) n_low[q] = sm[q].n_low;
        }
    }
    return rc;
}

// ---- the rescue gate behind the frames that hold the consensus (the kernels: srukf_rescue.hip) ----
// The switch: on the handle, like srukf_images_ransac.  Touches no device: chi2 reaches it in stream order in front of the next image run (run_images_issue).  It takes
// effect only in frames whose consensus runs: with srukf_images_ransac off a run issues the plain frames
int srukf_images_rescue_gate(srukf_ctx* c, int on, double chi2)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (on && (!std::isfinite(chi2) || chi2 <= 0.0)) { c->err = "images_rescue_gate: chi2 must be finite and positive"; return SRUKF_ERR_BAD_ARG; }
    if (c->async_pending) { c->err = "images_rescue_gate: a run is in flight (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    c->img_rescue = on != 0;
    if (on) c->img_rescue_chi2 = chi2;
    return SRUKF_OK;
}

// rows [first, first + count) of the gate's record, after waiting for the stream like srukf_get_image_matches; the lowest frame of the range that would rescue a match
int srukf_get_image_rescue(srukf_ctx* c, int first, int count, int* flags, double* h2, double* Si2, double* chi2, int* n_cand, int* n_high, int* first_rescue)
{
    int rc = image_getter_front(c, "get_image_rescue", first, count,
                                c && !(c->img.rq_flags && c->img.rq_valid) ? "no record of a run with the rescue gate in it (srukf_images_ransac and srukf_images_rescue_gate)" : nullptr);
    if (rc) return rc;
    const ImageReplay& im = c->img;
    const std::vector<ImageBuf> cols = image_group(c, IMG_RESCUE);
    rc = image_rows_get(c, cols, &im.rq_flags, first, count, flags);
    if (!rc) rc = image_rows_get(c, cols, &im.rq_h2, first, count, h2);
    if (!rc) rc = image_rows_get(c, cols, &im.rq_Si2, first, count, Si2);
    if (!rc) rc = image_rows_get(c, cols, &im.rq_chi2, first, count, chi2);
    if (!rc && (n_cand || n_high || first_rescue)) {
        std::vector<RescueSummary> sm;
        rc = image_summaries_get(c, cols, &im.rq_sum, first, count, sm, first_rescue, [](const RescueSummary& s) { return s.n_high > 0; });
        for (size_t q = 0; !rc && q < sm.size(); q++) {
            if (n_cand) n_cand[q] = sm[q].n_cand;
            if (n_high) n_high[q] = sm[q].n_high;
        }
    }
    return rc;
}

// The checkpoint of the image block the last srukf_synchronize ended clean comes back (X, S, the matchPatch array, the policy state: images_restore), so that a host
// can stop a block at the frame whose verdict asks for a map change (SLAM.cpp:552-562) by running the frames up to it again.  Only while nothing has written X, S or
// a matchPatch since that srukf_synchronize (ImageReplay::ck_clean)
int srukf_images_rewind(srukf_ctx* c)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    ImageReplay& im = c->img;
    if (c->async_pending) { c->err = "images_rewind: a run is in flight (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    if (!im.images || !im.ck_clean) { c->err = "images_rewind: no image block that srukf_synchronize ended clean, or the state has been written since"; return SRUKF_ERR_SEQUENCE; }
    HIPCHK(c, hipSetDevice(c->device));
    step_state_replaced(c);                                     // (clears ck_clean: one rewind per block)
    c->err.clear();
    images_restore(c);
    c->phase = 0; c->frame_updated = false;
    HIPCHK(c, hipGetLastError());
    return SRUKF_OK;
}

// ---- the state at a block's stop (the kernel: srukf_snapshot.hip) ----
// The switch: on the handle, like srukf_images_ransac.  Touches no device: the slots are allocated in front of the next image run (run_images_issue).  Not inside
// a block: a block is resumable only if every run of it had the switch on
int srukf_images_snapshots(srukf_ctx* c, int on)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (c->async_pending || c->img.pending) { c->err = "images_snapshots: a run is in flight or a block is pending (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    c->img_snap = on != 0;
    return SRUKF_OK;
}

// the two tags, after waiting for the stream: the staged frames whose start the slots hold (-1: none of this block, or no run with the switch on yet)
int srukf_get_image_snapshots(srukf_ctx* c, int frames[2])
{
    if (!c || !frames) return SRUKF_ERR_BAD_ARG;
    const ImageReplay& im = c->img;
    frames[0] = frames[1] = -1;
    if (!im.sn_ctl) return SRUKF_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    SnapshotCtl ctl;
    HIPCHK(c, hipMemcpy(&ctl, im.sn_ctl, sizeof ctl, hipMemcpyDeviceToHost));
    frames[0] = ctl.tag[0]; frames[1] = ctl.tag[1];
    return SRUKF_OK;
}

// The block the last srukf_synchronize ended clean is cut to its first `keep` frames without running them again: the slot that holds the state frame
// blk_first + keep started from comes back in the checkpoint's place (images_restore).  Legal where srukf_images_rewind is, in a block whose every run had the
// switch on; one resume or one rewind per block.  A slot that does not hold that frame: SRUKF_ERR_SEQUENCE, nothing moved, the block can still be rewound
int srukf_images_resume(srukf_ctx* c, int keep)
{
    if (!c || keep < 0) return SRUKF_ERR_BAD_ARG;
    ImageReplay& im = c->img;
    if (c->async_pending) { c->err = "images_resume: a run is in flight (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    if (!im.images || !im.ck_clean) { c->err = "images_resume: no image block that srukf_synchronize ended clean, or the state has been written since"; return SRUKF_ERR_SEQUENCE; }
    if (keep < 0 || keep > im.blk_end - im.blk_first) { c->err = "images_resume: keep outside [0, frames the block ran]"; return SRUKF_ERR_BAD_ARG; }
    if (!im.blk_snap || !im.sn_ctl) { c->err = "images_resume: the block ran without srukf_images_snapshots"; return SRUKF_ERR_SEQUENCE; }
    if (keep == 0) return srukf_images_rewind(c);
    if (keep == im.blk_end - im.blk_first) return SRUKF_OK;       // (the state is the one behind the block's last frame)
    const int stop = im.blk_first + keep;
    int tags[2];
    { const int rc = srukf_get_image_snapshots(c, tags); if (rc) return rc; }
    if (tags[stop & 1] != stop) { c->err = "images_resume: no slot holds the state in front of that frame (srukf_images_rewind and the frames again)"; return SRUKF_ERR_SEQUENCE; }
    step_state_replaced(c);                                     // (clears ck_clean: one resume or one rewind per block)
    c->err.clear();
    images_restore(c, stop & 1, stop);
    c->phase = 0; c->frame_updated = false;
    HIPCHK(c, hipGetLastError());
    return SRUKF_OK;
}

// ---- the display view behind image frames, the overlay of any staged frame (the kernels: srukf_predict.hip, srukf_display.hip, srukf_overlay.hip) ----
// The switch: on the handle, like srukf_images_snapshots.  Touches no device: the record is allocated in front of the next image run (run_images_issue).  Not inside
// a block: a block's rows are all written or none
int srukf_images_display(srukf_ctx* c, int on)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    if (c->async_pending || c->img.pending) { c->err = "images_display: a run is in flight or a block is pending (srukf_synchronize first)"; return SRUKF_ERR_SEQUENCE; }
    c->img_display = on != 0;
    return SRUKF_OK;
}

// rows [first, first + count) of the display record (what updateFeaturesInformation -> refreshFeaturesDisplay, SLAM.cpp:2566-2575, and recordRobotInformation would
// have refreshed behind each frame), after waiting for the stream like srukf_get_image_matches.  A record no run has allocated reads as zeros (the rule of
// srukf_get_image_checks)
int srukf_get_image_display(srukf_ctx* c, int first, int count, double* xyz, double* cov, double* axis, double* sigma, int* rot, double* pose4, double* P4, double* Si)
{
    if (!xyz && !cov && !axis && !sigma && !rot && !pose4 && !P4 && !Si) return SRUKF_ERR_BAD_ARG;
    int rc = image_getter_front(c, "get_image_display", first, count, nullptr, c && c->img.dp_rec);
    if (rc) return rc;
    const ImageReplay& im = c->img;
    const std::vector<ImageBuf> cols = image_group(c, IMG_DISPLAY);
    const size_t N = c->d.N, m = (size_t)count, doubles = image_col(cols, &im.dp_rec).row / sizeof(double);
    const ImageDisplayRow r = image_display_row(N);
    std::vector<double> rec(m * doubles);
    rc = image_rows_get(c, cols, &im.dp_rec, first, count, rec.data());
    if (!rc) rc = image_rows_get(c, cols, &im.dp_rot, first, count, rot);
    if (rc) return rc;
    for (size_t q = 0; q < m; q++) {
        const double* row = rec.data() + q * doubles;
        if (xyz) memcpy(xyz + q * 3 * N, row + r.xyz, sizeof(double) * 3 * N);
        if (cov) memcpy(cov + q * 9 * N, row + r.cov, sizeof(double) * 9 * N);
        if (axis) memcpy(axis + q * 4 * N, row + r.axis, sizeof(double) * 4 * N);
        if (sigma) memcpy(sigma + q * 3 * N, row + r.sigma, sizeof(double) * 3 * N);
        if (P4) memcpy(P4 + q * 16, row + r.robot, sizeof(double) * 16);
        if (pose4) memcpy(pose4 + q * 4, row + r.robot + 16, sizeof(double) * 4);
        if (Si) memcpy(Si + q * 4 * N, row + r.Si, sizeof(double) * 4 * N);
    }
    return SRUKF_OK;
}

// display2DFeatureModel + draw2DEllipse (SLAM.cpp:3009-3083) for staged frame `frame`, from what the device holds and with nothing uploaded: srukf_render_overlay's
// two launches on the frame's rows of h_seq, the display record's Si, z_seq and m_seq (behind a consensus run the masked row: what the filter used), over the
// frame's place in the staged stack, gray byte three times (srukf_stage_images).  Which rows are drawable is the host's mark per row (ImageReplay::dp_rows): set when a run with the
// display switch issues the row's launches, cleared when images_restore zeroes the row.  It writes the overlay's own buffers (ov_rec, d_ovl) only.
// (k_overlay reads the gray frame in dwords: a stack whose frames are no multiple of four bytes has frames that do not start on one)
// With a kept colour stack (srukf_stage_images_bgr) the frame's colour bytes are the source instead.
// The refusals of both overlay calls, in one order: frames [first, first + count) must lie in the stack and every one of them be drawable
static int image_overlay_front(srukf_ctx* c, const char* who, int first, int count)
{
    const ImageReplay& im = c->img;
    const std::string w = who;
    if (!im.images) { c->err = w + ": no staged images (srukf_stage_images)"; return SRUKF_ERR_SEQUENCE; }
    if (first >= im.frames || count > im.frames - first) { c->err = w + ": frame outside the staged images"; return SRUKF_ERR_BAD_ARG; }
    for (int q = first; q < first + count; q++)
        if (!im.dp_rec || !im.dp_rows[(size_t)q]) { c->err = w + ": no run with srukf_images_display on has written that frame's row (frame " + std::to_string(q) + ")"; return SRUKF_ERR_SEQUENCE; }
    const int W = (int)c->p.image_w, H = (int)c->p.image_h;
    if (W < 1 || H < 1 || (double)W * H > 268435456.0) { c->err = w + ": image size"; return SRUKF_ERR_BAD_ARG; }
    if ((W * H) % 4) { c->err = w + ": image_w * image_h must be a multiple of four"; return SRUKF_ERR_UNSUPPORTED; }
    return SRUKF_OK;
}

int srukf_render_image_overlay(srukf_ctx* c, int frame, unsigned char* out_bgr)
{
    if (!c || !out_bgr || frame < 0) return SRUKF_ERR_BAD_ARG;
    { const int rc = image_overlay_front(c, "render_image_overlay", frame, 1); if (rc) return rc; }
    const ImageReplay& im = c->img;
    const int W = (int)c->p.image_w, H = (int)c->p.image_h, N = c->d.N, npix = W * H;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!c->d_ovl) HIPCHK(c, srukf_dmalloc((void**)&c->d_ovl, overlay_bgr_bytes(npix)));
    if (!c->ov_rec) HIPCHK(c, srukf_dmalloc(&c->ov_rec, overlay_rec_bytes(N)));
    const size_t f = (size_t)frame, n = (size_t)N;
    const ImageDisplayRow r = image_display_row(n);
    {
        ProfScope ps(c, KC_OVERLAY, 0, (im.bgr_kept ? 6.0 : 4.0) * npix);
        // (z_seq / m_seq: the staged sequence's own rows, srukf_stage_sequence)
        launch_overlay(c->stream, W, H, N, image_row(image_group(c, IMG_STAGED), &im.h_seq, f), image_row(image_group(c, IMG_DISPLAY), &im.dp_rec, f) + r.Si, c->z_seq + f * 2 * n, c->m_seq + f * n, c->ov_rec,
                       im.bgr_kept ? im.bgr + f * 3 * (size_t)npix : nullptr, im.images + f * (size_t)npix, c->d_ovl);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_bgr, c->d_ovl, 3 * (size_t)npix, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                  // (out_bgr is pageable host memory)
    return SRUKF_OK;
}

// srukf_render_image_overlay for frames [first, first + count) in two launches and one copy: out_bgr holds count tight frames, frame
// first + q of it byte for byte the single call's.  A row of the range that is not drawable refuses the whole call and leaves out_bgr untouched.  The scratch
// (count output frames and record slabs) is a group of image_group that grows to the largest count asked for
int srukf_render_image_overlays(srukf_ctx* c, int first, int count, unsigned char* out_bgr)
{
    if (!c || !out_bgr || first < 0 || count < 1) return SRUKF_ERR_BAD_ARG;
    { const int rc = image_overlay_front(c, "render_image_overlays", first, count); if (rc) return rc; }
    if (count > OVERLAY_BLOCK_MAX) { c->err = "render_image_overlays: more than 65535 frames in one call"; return SRUKF_ERR_UNSUPPORTED; }
    ImageReplay& im = c->img;
    const int W = (int)c->p.image_w, H = (int)c->p.image_h, N = c->d.N, npix = W * H;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (count > im.ovs_count) {
        image_buffers_free(image_group(c, IMG_OVERLAYS), c->stream);
        im.ovs_count = count;
        const int rc = image_buffers_alloc(c, image_group(c, IMG_OVERLAYS, (size_t)npix), "render_image_overlays");
        if (rc) { im.ovs_count = 0; return rc; }
    }
    const size_t f = (size_t)first, n = (size_t)N, m = (size_t)count;
    const std::vector<ImageBuf> staged = image_group(c, IMG_STAGED), display = image_group(c, IMG_DISPLAY);
    {
        ProfScope ps(c, KC_OVERLAY, 0, (im.bgr_kept ? 6.0 : 4.0) * npix * m);
        launch_overlay_block(c->stream, W, H, N, count, image_row(staged, &im.h_seq, f), image_col(staged, &im.h_seq).row / sizeof(double),
                             image_row(display, &im.dp_rec, f) + image_display_row(n).Si, image_col(display, &im.dp_rec).row / sizeof(double), c->z_seq + f * 2 * n, 2 * n,
                             c->m_seq + f * n, n, im.ovs_rec, im.bgr_kept ? im.bgr + f * 3 * (size_t)npix : nullptr, im.images + f * (size_t)npix, im.ovs_out);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_bgr, im.ovs_out, m * 3 * (size_t)npix, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                  // (out_bgr is pageable host memory)
    return SRUKF_OK;
}

// Synchronous form.  No recovery inside the call: a flagged block comes back to its checkpoint (srukf_synchronize) and SRUKF_ERR_CLAMP_PENDING is returned
int srukf_run_images(srukf_ctx* c, int first, int count, int mode, double* traj_host)
{
    if (!c || first < 0 || count < 1) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return with_device_traj(c, count, traj_host, [=](double* dt) { const int rc = srukf_run_images_async(c, first, count, mode, dt); return rc ? rc : srukf_synchronize(c); });
}

// rows [first, first + count) of what the association wrote (rows no image run has written: z / matched as staged, the rest zero).  Waits for the stream only: flags
// of frames in flight are still srukf_synchronize's to report
int srukf_get_image_matches(srukf_ctx* c, int first, int count, double* z, int* matched, double* corr, int* visible, double* h)
{
    int rc = image_getter_front(c, "get_image_matches", first, count);
    if (rc) return rc;
    const ImageReplay& im = c->img;
    const std::vector<ImageBuf> cols = image_group(c, IMG_STAGED);
    // (z_seq / m_seq are the staged sequence's own, srukf_stage_sequence: a pair and a flag per landmark, the rows of h_seq and vis_seq)
    rc = image_rows_copy(c, z, c->z_seq, image_col(cols, &im.h_seq).row, first, count);
    if (!rc) rc = image_rows_copy(c, matched, c->m_seq, image_col(cols, &im.vis_seq).row, first, count);
    if (!rc) rc = image_rows_get(c, cols, &im.corr_seq, first, count, corr);
    if (!rc) rc = image_rows_get(c, cols, &im.vis_seq, first, count, visible);
    if (!rc) rc = image_rows_get(c, cols, &im.h_seq, first, count, h);
    return rc;
}

}  // extern "C"
