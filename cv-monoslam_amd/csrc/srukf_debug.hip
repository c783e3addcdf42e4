// srukf_debug.hip — srukf_debug_* (measurement / test switches, diagnostic read-outs; none of them is needed to use the library) and the stand-alone numeric
// primitives the parity tests call (srukf_gmw_host, srukf_project_host).

#include "srukf_ctx.h"
#include <climits>
using namespace srukf_impl;

// ---- the switches of srukf_debug_set: ONE row per key (storage: srukf_switches.h) ----
// range: what is stored for a value v — SW_ONOFF: v ? 1 : 0; SW_CLAMP: the nearest value of lo..hi; SW_REFUSE: v, and outside lo..hi nothing (SRUKF_ERR_BAD_ARG).
// after: what a change invalidates — SW_KEEP: nothing (the switch is read when something is built later); SW_DROP: the captured graphs and the step-wise chain of the
// filter in hand (a process-wide key: if a filter was passed); SW_DROP_NULL_SET: ... and its null set is looked for again (update_null_set's result is the call's);
// SW_DROP_VIEW: ... and 0 also forgets the cached display view; SW_DROP_BATCH: the captured graphs of every batch
enum SwKind : unsigned char { SW_ONOFF, SW_CLAMP, SW_REFUSE };
struct SwRange { SwKind kind; int lo, hi; };
constexpr SwRange ONOFF{ SW_ONOFF, 0, 1 }, RAW{ SW_CLAMP, INT_MIN, INT_MAX }, FROM0{ SW_CLAMP, 0, INT_MAX };
enum SwAfter : unsigned char { SW_KEEP, SW_DROP, SW_DROP_NULL_SET, SW_DROP_VIEW, SW_DROP_BATCH };
struct SwitchRow {
    const char* key;
    std::atomic<int> ProcessSwitches::* proc;      // process-wide (ctx may be NULL): the member of g_sw
    int DbgSwitches::* filt;                        // per filter: the member of c->dbg (both null: c->use_graph)
    int def; SwRange range; SwAfter after;
};
#define SW_P(member) &ProcessSwitches::member, nullptr
#define SW_F(member) nullptr, &DbgSwitches::member
static const SwitchRow k_switches[] = {
    // process-wide
    { "gmw_persist", SW_P(gmw_persist), 1, ONOFF, SW_DROP },            // 0: one launch per 64-row panel instead of one persistent launch per factorisation
    { "gmw_fused", SW_P(gmw_fused), 1, ONOFF, SW_DROP },                // 0: the persistent launch reads every tile from G (k_syrk computes all of them)
    { "rank_fused", SW_P(rank_fused), 1, ONOFF, SW_DROP },              // 0: the rank-aware form always goes through the full k_syrk + permutation pass
    { "rank_fold", SW_P(rank_fold), 1, ONOFF, SW_DROP },                // 0: the owners never form their tiles themselves in the rank-aware replay (k_syrk over all kept rows instead)
    { "rank_aware", SW_P(rank_aware), 1, ONOFF, SW_DROP_NULL_SET },     // 0: no context looks for structurally null directions (per filter: srukf_set_rank_aware)
    { "graphs", SW_P(graphs), 1, ONOFF, SW_DROP },                      // 0: contexts created from now on launch eagerly (profilers with --pmc; per filter: "use_graph")
    { "mem_split", SW_P(mem_split), 1, RAW, SW_DROP },                  // 0: sizes beyond two tiles per worker keep the memory-tile instance of k_gmw_persist instead of the split form; 2 (measurements): the split form also where the workers own two register tiles each
    { "head_fold_free", SW_P(head_fold_free), 0, { SW_REFUSE, 1, INT_MAX }, SW_DROP },      // CUs a plan must leave beside the pivot and the workers for the head fold; 0: SRUKF_HEAD_FOLD_MIN_FREE_CUS and the rounds rule — the default, which cannot be set back (values below 1 are refused)
    { "batch_split", SW_P(batch_split), 1, ONOFF, SW_DROP_BATCH },      // 0: one k_gmw_step64_b launch per panel in the batched replay (every tile recomputes its slabs) instead of slabs + plain updates
    { "batch_k128", SW_P(batch_k128), 1, ONOFF, SW_DROP_BATCH },        // 0: every panel's trailing update a pass of its own over G (K = 64)
    { "batch_xcd", SW_P(batch_xcd), 1, ONOFF, SW_DROP_BATCH },          // 0: k_syrk_b walks the head tiles in the solo launch's order
    { "batch_wide", SW_P(batch_wide), 1, ONOFF, SW_KEEP },              // 0: srukf_run_frames_batch never takes the batched launches (one stream per filter, persistent launches behind the gate: round 3's form)
    { "timing", SW_P(timing), 0, ONOFF, SW_KEEP },                      // 1: phases of map changes and of flagged frames on stderr
    { "fold_force", SW_P(fold_force), 0, ONOFF, SW_KEEP },              // 1: split fold also where the tile workgroups do not all fit
    { "pivot_relay", SW_P(pivot_relay), SRUKF_PIVOT_RELAY_DEFAULT, ONOFF, SW_KEEP },    // two pivot workgroups in the register-tile persistent launch; read when a plan is built
    { "batch_groups", SW_P(batch_groups), 0, { SW_REFUSE, 0, SRUKF_BATCH_GROUPS_MAX }, SW_KEEP },       // groups the batched filters are cut into (0: as many as pay)
    { "shared_tenants", SW_P(shared_tenants), 2, { SW_REFUSE, 2, 8 }, SW_KEEP },            // persistent launches that share the GPU, for filters switched to SRUKF_GPU_SHARED afterwards
    { "fold_head", SW_P(fold_head), 0, FROM0, SW_KEEP },                // split fold: block rows formed in front of the pair (0: the rule); before the state is set
    { "ctx_keep", SW_P(ctx_keep), 24, FROM0, SW_KEEP },                 // contexts a handle keeps across map changes (and at most ~16 GB of them)
    { "exact_rl", SW_P(exact_rl), 1, RAW, SW_KEEP },                    // 0: k_gmw_col, the left-looking exact path (one row per launch); 1: right-looking, as many pivots per launch as fit; 1 + B: B pivots per launch
    // per filter (their measurement notes: DbgSwitches)
    { "use_graph", nullptr, nullptr, 1, ONOFF, SW_DROP },               // 0: eager launches
    { "pxy2", SW_F(pxy2), 1, ONOFF, SW_DROP },                          // 0: k_pxy instead of k_pxy2 in "table" mode
    { "nullskip", SW_F(nullskip), 1, ONOFF, SW_DROP },                  // 0: with pxy2, structurally null directions are projected for every landmark
    { "head_fold", SW_F(head_fold), 1, ONOFF, SW_DROP },                // 0: k_syrk launch in front of the persistent launch
    { "tail_fuse", SW_F(tail_fuse), 1, ONOFF, SW_DROP },                // 0: k_project_table in front of every frame
    { "table_perm", SW_F(table_perm), 1, ONOFF, SW_DROP },              // 0: k_project_motion + k_pxy where the owners do not fold
    { "f32_fuse", SW_F(f32_fuse), 1, ONOFF, SW_DROP },                  // 0: fp32 storage stays out of "fused tail" mode
    { "split_record", SW_F(split_record), 0, ONOFF, SW_DROP },          // 1: every split-form factorisation first copies its input matrix to Gbak
    { "gain_fold", SW_F(gain_fold), 0, ONOFF, SW_DROP },                // 1: U^T and the state update in the tile epilogue of k_pxy2 instead of k_gain
    { "null_canon", SW_F(null_canon), 1, ONOFF, SW_DROP },              // 0: null rows that NEED_REORDER or a map change produced wait for a frame tail
    { "mixed_rank", SW_F(mixed_rank), 1, ONOFF, SW_DROP },              // 0: round 2's full-rank form of SRUKF_STORAGE_F32_MIXED
    { "mixed_f64_robot", SW_F(mixed_f64_robot), 1, ONOFF, SW_DROP },    // 0: every tile of the mixed downdate on the fp32 pipe
    { "mixed_bf16", SW_F(mixed_bf16), 0, ONOFF, SW_DROP },              // 1: the mixed downdate's fp32 products from three bf16 pieces
    { "step_fast", SW_F(step_fast), 1, ONOFF, SW_DROP },                // 0: the step-wise API keeps to its own launch sequences
    { "step_spin", SW_F(step_spin), 1, ONOFF, SW_DROP },                // 0: hipStreamSynchronize instead of spinning on the pinned flag word
    { "step_fuse_export", SW_F(step_fuse_export), 1, ONOFF, SW_DROP },  // 0: the fast path's results leave through export launches of their own
    { "view_auto", SW_F(view_auto), 1, ONOFF, SW_DROP_VIEW },           // 0: the display view is never exported with an update's status
    { "split_fold", SW_F(split_fold), 1, { SW_CLAMP, 0, 2 }, SW_DROP },     // 0: k_syrk forms everything in front of the split form's pair; 2 (measurements): the fold's launch behind a k_syrk that has formed everything
    { "step_early", SW_F(step_early), 2, { SW_CLAMP, 0, 2 }, SW_DROP },     // what srukf_update submits of the next frame: 0 nothing, 1 checkpoint copy + frame scalars, 2 also its first launch
    { "fused_motion", SW_F(fused_motion), 2, { SW_CLAMP, 0, 2 }, SW_DROP }, // the replay's motion step: 0 k_motion + k_project, 1 k_project_motion, 2 "table" mode
    { "mixed_null_ppm", SW_F(mixed_null_ppm), 1, FROM0, SW_DROP },      // 1e-6 of G_aa the mixed mode's null-direction check allows on top of 1e-12
};
#undef SW_P
#undef SW_F
static int switch_value(const SwitchRow& r, const srukf_ctx* c) { return r.proc ? (g_sw.*r.proc).load() : r.filt ? c->dbg.*r.filt : c->use_graph ? 1 : 0; }

// the filter at rest: its step-wise motion committed, its chain forgotten, its stream idle
static int quiesce(srukf_ctx* c)
{
    HIPCHK(c, hipSetDevice(c->device));
    step_commit_motion(c); step_invalidate(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SRUKF_OK;
}
// the plan the next frame's factorisation runs on
static const GmwPlan& frame_plan(const srukf_ctx* c) { return c->red_r > 0 ? c->gplan_red : c->gplan; }
// word `word` of that plan's sync block pad, cleared by the read (0 where the plan has no sync block)
static int take_pad_word(srukf_ctx* c, int word, long long* value)
{
    const GmwPlan& gp = frame_plan(c);
    unsigned long long v = 0, zero = 0;
    const size_t off = offsetof(GmwSync, pad) + 8 * (size_t)word;
    if (gp.sync) { HIPCHK(c, hipMemcpy(&v, (char*)gp.sync + off, sizeof v, hipMemcpyDeviceToHost)); HIPCHK(c, hipMemcpy((char*)gp.sync + off, &zero, sizeof zero, hipMemcpyHostToDevice)); }
    *value = (long long)v;
    return SRUKF_OK;
}

// The device work buffers srukf_debug_copy / srukf_debug_upload know: "Z" (L x mp), "DZ" (np x mp), "sigR" ((L + 1) x 8), "Cmat" (n x 4),
// "Xr1" (4), "Utp" / "P1" (mp x np), "h" (2N), "Si" (4N), ...
static bool debug_buffer(srukf_ctx* c, const char* key, double** ptr, long long* cap)
{
    const KDims& d = c->d;
    const GmwPlan& gp = frame_plan(c);
    double* src = nullptr; long long n = 0;
    if (!strcmp(key, "Z")) { src = c->Z; n = (long long)d.L * d.mp; }
    else if (!strcmp(key, "DZ")) { src = c->DZ; n = (long long)d.np * d.mp; }
    else if (!strcmp(key, "sigR")) { src = c->sigR; n = (long long)(d.L + 1) * 8; }
    else if (!strcmp(key, "Cmat")) { src = c->Cmat; n = (long long)d.n * 4; }
    else if (!strcmp(key, "Xr1")) { src = (double*)((char*)c->fs + offsetof(FrameScalars, Xr1)); n = 4; }
    else if (!strcmp(key, "Utp")) { src = c->Utp; n = c->Utp ? (long long)d.mp * d.np : 0; }
    else if (!strcmp(key, "P1")) { src = c->P1; n = c->P1 ? (long long)d.mp * d.np : 0; }
    else if (!strcmp(key, "h")) { src = c->h; n = 2LL * d.N; }
    else if (!strcmp(key, "Si")) { src = c->Si; n = 4LL * d.N; }
    else if (!strcmp(key, "Ut")) { src = c->Ut; n = (long long)d.mp * d.np; }
    else if (!strcmp(key, "PxyR")) { src = c->PxyR; n = 5LL * d.mp; }
    else if (!strcmp(key, "joint_R")) { src = c->jointW; n = c->jointW ? (long long)d.mp * joint_work_ld(d.mp, d.np) : 0; }      // R | U^T | w as srukf_update_joint left them
    else if (!strcmp(key, "det_resp")) { src = c->det.resp; n = c->det.resp ? (long long)c->p.image_w * (long long)c->p.image_h : 0; }   // the response map of the last srukf_detect_features
    // the operands of one factorisation (scripts/split_replay.py: a split-form pair recorded from a real frame, each launch then replayed alone under the counters)
    else if (!strcmp(key, "Wf")) { src = c->Wf; n = (long long)d.np * d.np; }
    else if (!strcmp(key, "Gbak")) { src = c->Gbak; n = (long long)d.np * d.np; }
    else if (!strcmp(key, "G")) { src = c->G; n = (long long)d.np * d.np; }
    else if (!strcmp(key, "D")) { src = c->D; n = d.np; }
    else if (!strcmp(key, "fold_dbg")) { src = c->fold_sync ? (double*)(c->fold_sync + ((srukf_fold_words(d.mp / 64, d.np / 64) + 1) & ~1)) : nullptr; n = c->fold_sync ? FOLD_DBG_STAMPS : 0; }      // -DSRUKF_FOLD_DBG: time stamps of the gain fold
    else if (!strcmp(key, "gsW")) { src = c->gsW; n = c->gsW ? (long long)c->gs_panels * 64 * d.np : 0; }
    else if (!strcmp(key, "gsL")) { src = c->gsL; n = c->gsL ? (long long)c->gs_panels * 64 * d.np : 0; }
    else if (!strcmp(key, "pans")) { src = (double*)gp.pans; n = gp.pans ? (long long)srukf_gmw_panel_bytes() * gp.T / 8 : 0; }
    else if (!strcmp(key, "sync")) { src = (double*)gp.sync; n = gp.sync ? (long long)srukf_gmw_sync_bytes(gp.T) / 8 : 0; }
    else return false;
    *ptr = src; *cap = n;
    return true;
}

extern "C" {

// Kept for ABI compatibility and for the study scripts that still call it (rounds 2 - 5: let srukf_set_storage accept SRUKF_STORAGE_F32_MIXED below its then
// epsilon floor): no effect since round 6.
int srukf_debug_allow_mixed(srukf_ctx* c, int on) { return c ? SRUKF_OK : SRUKF_ERR_BAD_ARG; }

// Test hook: S[row][col] = value on the device, behind the back of everything that tracks S (the null set of the rank-aware
// refactorisation, the permuted copy): the next frame has to notice by itself.
int srukf_debug_poke_state(srukf_ctx* c, int row, int col, double value)
{
    if (!c || row < 0 || col < row || col >= c->d.n) return SRUKF_ERR_BAD_ARG;
    if (const int rc = quiesce(c)) return rc;
    HIPCHK(c, hipMemcpy(c->S + (size_t)row * c->d.np + col, &value, sizeof(double), hipMemcpyHostToDevice));
    return SRUKF_OK;
}

// Measurement / test switches behind ONE entry point: the row of k_switches the key names says what is stored and what the change invalidates.
int srukf_debug_set(srukf_ctx* c, const char* key, int value)
{
    if (!key) return SRUKF_ERR_BAD_ARG;
    const SwitchRow* r = std::find_if(std::begin(k_switches), std::end(k_switches), [key](const SwitchRow& s) { return !strcmp(s.key, key); });
    if (r == std::end(k_switches)) { if (c) c->err = std::string("srukf_debug_set: unknown key ") + key; return SRUKF_ERR_BAD_ARG; }
    if (!r->proc && !c) return SRUKF_ERR_BAD_ARG;
    const SwRange& g = r->range;
    if (g.kind == SW_ONOFF) value = value ? 1 : 0;
    else if (value < g.lo || value > g.hi) { if (g.kind == SW_REFUSE) return SRUKF_ERR_BAD_ARG; value = value < g.lo ? g.lo : g.hi; }
    // a filter's own switch changes while the filter is at rest; a process-wide one at once (another thread's filter sees it when it builds or captures next)
    if (!r->proc) { if (const int rc = quiesce(c)) return rc; }
    if (r->proc) (g_sw.*r->proc).store(value); else if (r->filt) c->dbg.*r->filt = value; else c->use_graph = value != 0;
    if (r->after == SW_DROP_VIEW && !value) { c->view_auto = false; c->view_cached = false; }
    if (r->after == SW_DROP_BATCH) batch_drop_all_graphs();
    else if (r->after != SW_KEEP && c) {
        if (r->proc) quiesce(c);
        drop_graphs(c);
        if (r->after == SW_DROP_NULL_SET) return update_null_set(c);
    }
    return SRUKF_OK;
}

int srukf_debug_switch_at(srukf_ctx* c, int index, const char** key, int* per_filter, int* default_value, int* value)
{
    if (index < 0 || index >= (int)(sizeof k_switches / sizeof k_switches[0])) return SRUKF_ERR_BAD_ARG;
    const SwitchRow& r = k_switches[index];
    if (key) *key = r.key;
    if (per_filter) *per_filter = r.proc ? 0 : 1;
    if (default_value) *default_value = r.def;
    if (value) *value = r.proc || c ? switch_value(r, c) : r.def;
    return SRUKF_OK;
}

// Diagnostic builds only (make EXTRA=-DSRUKF_GMW_DBG): host-visible time stamps of the persistent factorisation launch of THIS context's rank-aware
// plan (GMW_TS in srukf_gmw_persist.hip).  buf receives 4096 unsigned long longs: [2048 + 8 p + slot] = s_memrealtime (10 ns ticks) of pivot iteration p.
int srukf_debug_gmw_stamps(srukf_ctx* c, unsigned long long* buf)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    // (device memory: stamps written to pinned host memory cross PCIe, and every later s_waitcnt vmcnt(0) of the stamping wave waits for them — the timeline of the
    //  diagnostic build then shows 17.9 us per panel where the product runs 14.5)
    static unsigned long long* dbuf = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const GmwPlan& g = frame_plan(c);
    if (!g.sync) return SRUKF_ERR_SEQUENCE;
    if (!dbuf) { HIPCHK(c, hipMalloc((void**)&dbuf, 8 * 4096)); HIPCHK(c, hipMemset(dbuf, 0, 8 * 4096)); }
    if (buf) HIPCHK(c, hipMemcpy(buf, dbuf, 8 * 4096, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy((char*)g.sync + offsetof(GmwSync, dbg), &dbuf, 8, hipMemcpyHostToDevice));      // armed for the launches that follow
    return SRUKF_OK;
}

// Diagnostic read-out of the device-resident frame scalars (synchronises the stream): "gmw_aborts", "clamp_rows", "frame", "frozen", "gate_timeouts"; "gmw_shared", "split_form";
// of the filter's own switches: "split_off", "use_graph" (what srukf_debug_set(ctx, "use_graph", v) or the process-wide "graphs" left: tests follow it through map changes)
int srukf_debug_get(srukf_ctx* c, const char* key, long long* value)
{
    if (!c || !key || !value) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->hfs, c->fs, sizeof(FrameScalars), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!strcmp(key, "gmw_aborts")) *value = c->hfs->gmw_aborts;
    else if (!strcmp(key, "clamp_rows")) *value = c->hfs->clamp_rows;
    else if (!strcmp(key, "frame")) *value = c->hfs->frame;
    else if (!strcmp(key, "frozen")) *value = c->hfs->frozen;
    else if (!strcmp(key, "gate_timeouts")) *value = c->hfs->gate_timeouts;
    else if (!strcmp(key, "gmw_shared")) *value = c->gmw_shared;
    else if (!strcmp(key, "split_off")) *value = c->split_off ? 1 : 0;
    else if (!strcmp(key, "use_graph")) *value = c->use_graph ? 1 : 0;
    // diagnostic builds (-DSRUKF_GMW_DBG): words 1..7 of the sync block's pad (helpers started / finished, head counters at the last exit, grid, helpers); cleared by the read
    else if (!strncmp(key, "pad", 3) && key[3] >= '1' && key[3] <= '7' && !key[4]) return take_pad_word(c, key[3] - '0', value);
    // who abandoned a persistent launch first, and where (gmw_abandon, srukf_gmw_persist.hip: site << 32 | blockIdx + 1; 0: nobody since the last read); cleared by the read
    else if (!strcmp(key, "abort_code")) return take_pad_word(c, 0, value);
    else if (!strcmp(key, "step_fast")) *value = c->step_fast_frames;          // frames the step-wise API ran on the staged replay's launch sequence / on its own
    else if (!strcmp(key, "step_slow")) *value = c->step_slow_frames;
    else if (!strcmp(key, "exact_frames")) *value = c->exact_frames;
    else if (!strcmp(key, "fold_seqs")) *value = c->fold_seqs;
    else if (!strcmp(key, "split_fold_seqs")) *value = c->split_fold_seqs;
    else if (!strncmp(key, "pxy2_stamp", 10) && key[10] >= '1' && key[10] <= '7') { const unsigned long long* t = (const unsigned long long*)(c->hmeas + c->d.mp + 5 * (size_t)c->d.N); *value = (long long)(t[key[10] - '0'] - t[0]); }   // diagnostic build (-DSRUKF_PXY2_DBG): 2 motion end, 4..7 sampled tiles' ends
    else if (!strcmp(key, "meas_flag_ticks")) { const unsigned long long* t = (const unsigned long long*)(c->hmeas + c->d.mp + 5 * (size_t)c->d.N); *value = (long long)(t[1] - t[0]); }   // last fast-path k_pxy2: first workgroup's start -> statistics flag, 10 ns ticks
    else if (!strcmp(key, "view_hits")) *value = c->view_hits;                     // srukf_get_frame_view calls served from the view an update exported with its status
    else if (!strcmp(key, "view_auto")) *value = c->view_auto ? 1 : 0;
    else if (!strcmp(key, "split_form")) *value = split_form(c, frame_plan(c)) ? 1 : 0;       // would the next persistent factorisation be the split form?
    else if (!strncmp(key, "plan_", 5)) {
        // which launch plan the next staged frame takes (tests assert it next to the oracle comparison: every N is a product size, SLAM.cpp:552-562, 2443-2460)
        const GmwPlan& gp = frame_plan(c);
        const RefactorPlan rp = refactor_form(c, refactor_frame_tail(c));
        const bool persist = plan_persists(c, gp);
        const char* k = key + 5;
        if (!strcmp(k, "T")) *value = gp.T;
        else if (!strcmp(k, "Tp")) *value = gp.Tp;
        else if (!strcmp(k, "tiles")) *value = gp.nreal;
        else if (!strcmp(k, "workers")) *value = gp.workers;
        else if (!strcmp(k, "persist")) *value = persist ? 1 : 0;                                        // 0: one launch per 64-row panel
        else if (!strcmp(k, "register_form")) *value = (persist && !split_form(c, gp) && srukf_gmw_register_form(gp.T, gp.Tp, gp.ntiles, gp.workers)) ? 1 : 0;
        else if (!strcmp(k, "relay")) *value = (persist && !split_form(c, gp) && gp.relay && srukf_gmw_register_form(gp.T, gp.Tp, gp.ntiles, gp.workers)) ? 1 : 0;      // two pivot workgroups
        else if (!strcmp(k, "tiles_per_worker")) *value = gp.workers > 0 ? (gp.nreal + gp.workers - 1) / gp.workers : -1;
        else if (!strcmp(k, "fold")) *value = rp.form == RF_OWNERS_FOLD ? 1 : 0;                         // the owners form their tiles of S^T S - U U^T themselves
        else if (!strcmp(k, "head_fold")) *value = rp.head_fold ? 1 : 0;                                 // ... and the head tiles ride on the persistent launch
        else if (!strcmp(k, "red_perm")) *value = replay_red_perm(c) ? 1 : 0;     // RF_PERMUTED_SYRK as "table" mode may build on it: 0 with "table_perm" 0, though the form still runs
        else if (!strcmp(k, "motion")) *value = replay_motion_mode(c);                                   // 2: "table" mode
        else if (!strcmp(k, "fuse")) *value = frame_form(c).fused_tail() ? 1 : 0;                               // "fused tail" mode
        else if (!strcmp(k, "kept")) *value = c->red_r;
        else if (!strcmp(k, "sync_doubles")) *value = gp.sync ? srukf_gmw_sync_bytes(gp.T) / 8 : 0;      // sizes of the byte buffers srukf_debug_copy counts in doubles
        else if (!strcmp(k, "pans_doubles")) *value = gp.pans ? (long long)srukf_gmw_panel_bytes() * gp.T / 8 : 0;
        else if (!strcmp(k, "slab_panels")) *value = c->gs_panels;
        else return SRUKF_ERR_BAD_ARG;
    }
    else return SRUKF_ERR_BAD_ARG;
    return SRUKF_OK;
}

// Diagnostic copy of a device work buffer (synchronises the stream; the keys: debug_buffer): `count` doubles from the start of the buffer, in either direction
static int debug_transfer(srukf_ctx* c, const char* key, double* host, long long count, hipMemcpyKind kind)
{
    if (!c || !key || !host || count < 0) return SRUKF_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double* dev = nullptr; long long cap = 0;
    if (!debug_buffer(c, key, &dev, &cap)) return SRUKF_ERR_BAD_ARG;
    if (!dev || count > cap) return SRUKF_ERR_DIM_MISMATCH;
    const bool up = kind == hipMemcpyHostToDevice;
    HIPCHK(c, hipMemcpy(up ? dev : host, up ? host : dev, sizeof(double) * (size_t)count, kind));
    return SRUKF_OK;
}
int srukf_debug_copy(srukf_ctx* c, const char* key, double* out, long long count) { return debug_transfer(c, key, out, count, hipMemcpyDeviceToHost); }
int srukf_debug_upload(srukf_ctx* c, const char* key, const double* in, long long count) { return debug_transfer(c, key, const_cast<double*>(in), count, hipMemcpyHostToDevice); }

// Tests only: persistent factorisation launches of this context start WITHOUT their worker workgroups, as if another
// process held the GPU — exercises the bounded waits and the fallback to per-panel launches.

int srukf_debug_starve_workers(srukf_ctx* c, int on)
{
    if (!c) return SRUKF_ERR_BAD_ARG;
    c->debug_starve = on == 2 ? 2 : on ? 1 : 0;              // 2: only split-form pairs start without their tile launch (the single persistent launch below them is not starved)
    step_invalidate(c);
    drop_graphs(c);                                    // the captured frames contain one or the other launch sequence
    return SRUKF_OK;
}

int srukf_gmw_host(int device, int n, const double* G, double* S_out, double* D_out, double epsilon, int force_slow, int* clamp_hit)
{
    if (n < 1 || !G || !S_out) return SRUKF_ERR_BAD_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return SRUKF_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return SRUKF_ERR_NO_DEVICE;
    const int np = round_up(n, SRUKF_PAD);
    const size_t bytes = sizeof(double) * (size_t)np * np;
    std::vector<double> hG((size_t)np * np, 0.0), hS((size_t)np * np, 0.0), hD(np, 0.0);
    for (int r = 0; r < n; r++) for (int c = r; c < n; c++) hG[(size_t)r * np + c] = G[(size_t)r * n + c];
    // every device resource of the call in one holder: released on every path out
    struct Res {
        double *dG = nullptr, *dS = nullptr, *dD = nullptr, *dWf = nullptr; unsigned long long* dTh = nullptr; FrameScalars* dFs = nullptr;
        GmwPanel64* pan[2] = { nullptr, nullptr }; GmwPlan gp;
        ~Res() { for (void* b : { (void*)dG, (void*)dS, (void*)dD, (void*)dWf, (void*)dTh, (void*)dFs, (void*)pan[0], (void*)pan[1] }) if (b) srukf_dfree(b); gmw_plan_destroy(gp); }
    } r;
#define GH(call) do { if ((call) != hipSuccess) return SRUKF_ERR_HIP; } while (0)
    GH(srukf_dmalloc((void**)&r.dG, bytes)); GH(srukf_dmalloc((void**)&r.dS, bytes)); GH(srukf_dmalloc((void**)&r.dWf, bytes));
    GH(srukf_dmalloc((void**)&r.dD, sizeof(double) * np)); GH(srukf_dmalloc((void**)&r.dTh, sizeof(unsigned long long) * np)); GH(srukf_dmalloc((void**)&r.dFs, sizeof(FrameScalars)));
    GH(hipMemcpy(r.dG, hG.data(), bytes, hipMemcpyHostToDevice));
    GH(hipMemset(r.dS, 0, bytes)); GH(hipMemset(r.dWf, 0, bytes)); GH(hipMemset(r.dTh, 0, sizeof(unsigned long long) * np));
    GH(hipMemset(r.dFs, 0, sizeof(FrameScalars))); GH(hipMemset(r.dD, 0, sizeof(double) * np));
    hipStream_t st = nullptr;
    srukf_launch_gmw_stats(st, n, np, r.dG, r.dFs);
    FrameScalars fs;
    if (!force_slow) {
        // the plan knows how many workgroups THIS device can keep resident (CU count); workers < 0: per-panel launches
        if (g_sw.gmw_persist) { const int rc = gmw_plan_create(r.gp, np, st); if (rc) return rc; }
        // every panel pivoted, every row kept, no gate
        const GmwLaunch g = { .n = n, .ld = np, .eps = epsilon, .G = r.dG, .pans = r.gp.pans, .D = r.dD, .Sout = r.dS, .sync = r.gp.sync, .tiles = r.gp.tiles, .ntiles = r.gp.ntiles,
                              .workers = r.gp.workers, .fs = r.dFs, .Tp = 0, .krows = 0, .gate_limit = 0, .relay = r.gp.relay };
        if (g_sw.gmw_persist && r.gp.workers >= 0) {
            srukf_launch_gmw_persist(st, g, nullptr, nullptr);
        } else {
            GH(srukf_dmalloc(&r.pan[0], srukf_gmw_panel_bytes())); GH(srukf_dmalloc(&r.pan[1], srukf_gmw_panel_bytes()));
            GH(hipMemset(r.pan[0], 0, srukf_gmw_panel_bytes())); GH(hipMemset(r.pan[1], 0, srukf_gmw_panel_bytes()));
            gmw_per_panel(st, g, r.pan);
        }
        GH(hipDeviceSynchronize());
        srukf_launch_gmw_check(st, n, np, r.dD, r.dS, r.dFs, nullptr, 0, nullptr);
        GH(hipMemcpy(&fs, r.dFs, sizeof fs, hipMemcpyDeviceToHost));
        if (clamp_hit) *clamp_hit = fs.clamp_rows;
        if (fs.clamp_rows > 0) force_slow = 2;   // same contract as srukf_update: redo on the exact path
    }
    if (force_slow) {
        GH(hipMemcpy(r.dG, hG.data(), bytes, hipMemcpyHostToDevice));
        GH(hipMemset(r.dTh, 0, sizeof(unsigned long long) * np));
        GH(hipMemset(r.dS, 0, bytes));
        for (int j = 0; j < n; j++) srukf_launch_gmw_col(st, n, np, j, epsilon, r.dG, r.dWf, r.dD, r.dTh, r.dFs, r.dS);
        GH(hipMemcpy(&fs, r.dFs, sizeof fs, hipMemcpyDeviceToHost));
        if (clamp_hit && force_slow == 1) *clamp_hit = fs.clamp_rows;
    }
    GH(hipDeviceSynchronize());
    GH(hipMemcpy(hS.data(), r.dS, bytes, hipMemcpyDeviceToHost));
    GH(hipMemcpy(hD.data(), r.dD, sizeof(double) * np, hipMemcpyDeviceToHost));
#undef GH
    for (int rr = 0; rr < n; rr++) memcpy(S_out + (size_t)rr * n, hS.data() + (size_t)rr * np, sizeof(double) * n);
    if (D_out) memcpy(D_out, hD.data(), sizeof(double) * n);
    return SRUKF_OK;
}

int srukf_project_host(int device, const srukf_params* p, int count, const double* feat6, const double* pos3, const double* psi,
                       const double* err2, double* uv_out)
{
    if (!p || count < 1 || !feat6 || !pos3 || !psi || !err2 || !uv_out) return SRUKF_ERR_BAD_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return SRUKF_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return SRUKF_ERR_NO_DEVICE;
    double *df, *dp, *ds, *de, *dout;
    srukf_dmalloc((void**)&df, sizeof(double) * 6 * count); srukf_dmalloc((void**)&dp, sizeof(double) * 3 * count);
    srukf_dmalloc((void**)&ds, sizeof(double) * count); srukf_dmalloc((void**)&de, sizeof(double) * 2 * count); srukf_dmalloc((void**)&dout, sizeof(double) * 2 * count);
    hipMemcpy(df, feat6, sizeof(double) * 6 * count, hipMemcpyHostToDevice); hipMemcpy(dp, pos3, sizeof(double) * 3 * count, hipMemcpyHostToDevice);
    hipMemcpy(ds, psi, sizeof(double) * count, hipMemcpyHostToDevice); hipMemcpy(de, err2, sizeof(double) * 2 * count, hipMemcpyHostToDevice);
    srukf_launch_project_points(nullptr, *p, count, df, dp, ds, de, dout);
    hipError_t e = hipDeviceSynchronize();
    hipMemcpy(uv_out, dout, sizeof(double) * 2 * count, hipMemcpyDeviceToHost);
    srukf_dfree(df); srukf_dfree(dp); srukf_dfree(ds); srukf_dfree(de); srukf_dfree(dout);
    return e == hipSuccess ? SRUKF_OK : SRUKF_ERR_HIP;
}

}  // extern "C"
