// cslam_step_bench — wall-clock frame rate of the DROP-IN path: what a host that binds this library the way the MFC view binds the reference's
// CSLAM gets per frame (SLAM.cpp:87-112, called from MonoSLAMView.cpp:499-572): predict, host (or device) data association, update — one frame at a
// time, with the host round trips in between.  bench.py's headline is the staged replay (inputs resident in HBM, no host in the loop); this is the other number.
//   cslam_step_bench scene.bin odometry.txt mode=<capi|facade|assoc|replay|assoc_replay> [frames=K] [warmup=W] [hint=0|1] [set=key:value ...]
//     capi   : srukf_predict_motion -> srukf_predict_measurement (D->H h, Si, visible) -> host association (matched = visible, z from the scene)
//              -> srukf_update (H->D) -> srukf_get_robot (the pose and robot block RobotPath.txt records, SLAM.cpp:3539-3556)
//     facade : monoslam::CSLAM::SLAM() with the same association as a callback (what cslam_replay does), display refresh and mirrors included
//     assoc  : capi with srukf_associate (wrapPatch + dataAssociation on the device, SLAM.cpp:1803-2009) on a 640 x 480 gray frame between predict and
//              update.  The frame is a static synthetic texture the landmarks' init patches were cut from, so the templates stop correlating as the
//              robot moves: the launches and their D->H copy are what is timed, the filter itself is driven by the scene's z / matched (stated in the output).
//     replay : the staged replay, for comparison on the same scene file: srukf_stage_sequence (every landmark offered as matched; the device's visibility decides,
//              as in capi), then srukf_run_frames_async + srukf_synchronize in blocks of `frames` (the warm-up frames first, as one block of their own), srukf_get_robot
//              at the end.  Honours joint=1 (SRUKF_UPDATE_JOINT frames) and set=key:value; prints the same keys as capi (the per-call host times are zero)
//     assoc_replay : the staged replay with the association on the device, on assoc's scene, gray frame and appearance set-up: the frame is staged once
//              per staged frame (srukf_stage_images), then srukf_run_images_async + srukf_synchronize in blocks of `block` frames (default 8: the churn leg changes the
//              map every ten frames), the warm-up frames first.  The filter is driven by what the device's association finds.  A flagged block comes back restored and
//              is run step-wise (srukf_associate + srukf_update / srukf_update_joint), inside the timed region; "flagged_blocks" counts them.  Honours joint=1 and set=
//              unique=<ratio>[,<exclusion>] and / or subpix=1 (assoc_replay only): the blocks are checked image runs (srukf_run_images_checked_async, DESIGN.md §21;
//              subpix=1 alone: ratio 2, nothing vetoed; exclusion defaults to 4), a restored block runs srukf_associate_checked, and srukf_get_image_checks is read
//              with the record after every block.  Adds, and only with them, "checked": {ratio, exclusion, subpixel, ambiguous, refined} to the output
//              archive=<L>[,<half_cap>] (assoc_replay only): L records are archived from the bench's own frame — landmarks created on a context of their own at the
//              pixels farthest from every landmark's, srukf_capture_appearance + srukf_get_landmark_record — and searched in every frame on the device
//              (srukf_images_search_archive); hits are read after every block (srukf_get_image_archive).  archive_step=1 with it: the step-wise
//              route instead — the switch stays off and srukf_archive_search runs on the frame after every block (with block=1: once per frame, what a host had
//              to do before the switch).  Adds "archive": {records, half_cap, route, matched_records} to the output
//              policy=1 (assoc_replay only): the map policy's verdict behind every frame (srukf_images_policy with the default parameters); the
//              record's summaries are read after every block (srukf_get_image_policy).  The bench's map never changes: a block is not cut at first_change.  Adds
//              "policy": {change_frames, deletes, need_add_frames} to the output
//              ransac=<threshold> (assoc_replay): the 1-point RANSAC consensus inside every frame (srukf_images_ransac; threshold in pixels, 8 is the
//              reference's); the record's summaries are read after every block (srukf_get_image_ransac).  The bench runs no rescue: a block is not cut at
//              first_outlier.  A restored block runs srukf_ransac_consensus step-wise.  Adds "ransac": {threshold, outlier_frames, low_inliers} to the output
//              rescue=1 (assoc_replay with ransac=<threshold>): the rescue gate behind every such frame (srukf_images_rescue_gate with CHI2INV_TABLE(0,2));
//              the record's summaries are read after every block (srukf_get_image_rescue) and "rescue_frames" (frames with n_high > 0) joins "ransac" in the output
//              resume=1 (assoc_replay only): the blocks run with srukf_images_snapshots on: every frame begins with k_image_snapshot.  This measures
//              the switch's price.  Adds "resume": 1 to the output
//              stop=<k> with resume=0|1 (assoc_replay only; 0 < k < block): behind every timed block of `block` frames comes what a host does when the block has to
//              stop behind its first k frames, timed with the block — resume=0: srukf_images_rewind and the first k frames again; resume=1: srukf_images_resume(k) —
//              and the next block begins at the stop.  Two stops exist without inventing one: with policy=1 every block stops behind its first frame (the bench's
//              texture flags every landmark in every frame), k = 1; without the policy the slots hold the starts of the block's last two frames,
//              k = block - 1.  The tool runs BOTH legs on fresh handles, the other one first and untimed in the report, and exits with status 3 unless both end
//              at the same pose and robot covariance, bit for bit.  Adds "stop": {k, resume, blocks} to the output
//              display=1 (assoc_replay only): the blocks run with srukf_images_display on: every frame is followed by k_image_view + k_lm_ellipsoid and
//              the run is issued frame by frame.  This measures the switch's price: with policy=1 the two launches alone, without it also the eight-frame graphs the
//              run gives up.  Adds "display": 1 to the output
//              colour=1 (assoc_replay only): the frames are staged as B = G = R colour frames through srukf_stage_images_bgr (the conversion keeps such
//              a frame byte for byte, so the run is the gray one's).  Adds "staging_ms": the wall time of srukf_stage_images on the gray stack, of the same
//              conversion done on the host in front of it, and of srukf_stage_images_bgr with keep_colour 0 and 1 (the last one stays staged), each for the
//              W + K frames of the run
//              profile=1 (assoc_replay only): the timed blocks run with srukf_set_profiling on (eager launches); adds "profile_ms_per_frame" by kernel class
//     hint=1 : capi / assoc announce the NEXT frame's odometry with srukf_predict_motion_next before every update (a host that has its odometry
//              file loaded, as the reference has: loadOdometryData reads it whole, SLAM.cpp:363-496)
//     set=key:value : srukf_debug_set(ctx, key, value) after the context exists (capi / assoc; measurement switches, e.g. set=step_fuse_export:0)
//     churn=P (facade): the map changes while the filter runs, through the reference's OWN policy (SLAM.cpp:2443-2460 deletions in updateFeaturesInformation,
//              552-562 additions through the addFeatures callback): every P frames the host stops matching one landmark and zeroes its match count, so that the
//              policy's "predicted often, matched rarely" rule (nPredictTimes > 2 nMatchTimes, >= 10 predictions) removes it in that frame's
//              updateFeaturesInformation -> deleteOneFeature, and sets isAdding, so that the same frame's addFeatures hands one key point to
//              integrateFeaturesInformation (joint initialisation on the device); the next frame's KalmanUpdate then runs FLAG_4_NEED_REORDER.  N stays where it
//              was.  Every landmark is "found" at its predicted pixel + 0.5 px of noise (new landmarks have no entry in the scene's z).  Prints frames/s,
//              the map changes and their wall time per operation, and how many frames ran on the step-wise fast path / on the other one
//              drop=<k> (default 1: the above): every change starves k landmarks, no two of them neighbours in the state (the walk of updateFeaturesInformation
//              does not test the node behind a deleted one in the same frame), and addFeatures hands k key points.  together=1: CSLAM::deleteTogether on — the
//              landmarks of a frame leave in one device call.  With either, "deletion_calls" and "landmarks_deleted" follow "ms_per_deletion"
//              (which is per call)
//     ransac=1 (facade): CSLAM::isUseRANSAC on (KalmanUpdate runs the 1-point RANSAC steps: consensus, update, and the rescue when matches remain outside it)
//     joint=1 : every update is the joint measurement update (capi / assoc: srukf_update_joint; facade: CSLAM::jointUpdate).  Adds, and only with it,
//              "joint": 1 and "joint_flagged_frames" (updates whose refactorisation was flagged and went to the exact path) to the output
//     ellipsoids=1 (facade): CSLAM::ellipsoidsOnDevice on (axis / sigma of every landmark come from the device with the frame view, srukf_get_frame_view_display,
//              instead of the host's Jacobi iteration per landmark); the run's figures are then also printed under "facade_ellipsoids_on_device"
// scene.bin: int32 N, int32 F, double a1..a4, double X0[n], double S0[n*n], double z[F][2N]   (the file cslam_replay reads)
// Prints ONE JSON object.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "cslam.hpp"

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv)
{
    if (argc < 4) { fprintf(stderr, "usage: %s scene.bin odometry.txt mode=<capi|facade|assoc|replay> [frames=K] [warmup=W] [hint=0|1]\n"
                                "       (mode=assoc_replay [block=B] [archive=L[,half_cap]] [archive_step=1] [policy=1] [profile=1] [resume=0|1 [stop=k]]: the staged replay with the association on the device)\n", argv[0]); return 2; }
    std::string mode = "capi";
    int K = 200, W = 20, hint = 0, churn = 0, ransac = 0, ellipsoids = 0, joint = 0, block_frames = 8;
    bool checked = false; srukf_match_params mpar = { 0.8, 2.0, 4, 0 };      // unique= / subpix=: checked image runs (assoc_replay)
    long long ambiguous = 0, refined = 0;
    int arcL = 0, arc_step = 0, profile = 0; srukf_archive_params apar = { 40, 0.8, 5.99146454710798 };      // archive= / archive_step= / profile= (assoc_replay)
    long long arc_hits = 0;
    int policy = 0; long long pol_change = 0, pol_deletes = 0, pol_adds = 0;      // policy= (assoc_replay)
    double ransac_thr = 0.0; long long rs_outlier = 0, rs_low = 0;      // ransac=<threshold> (assoc_replay)
    int rescue = 0; long long rq_high = 0;                              // rescue=1 (assoc_replay with ransac=)
    int resume = -1, stop_k = 0; long long stop_blocks = 0;      // resume= / stop= (assoc_replay)
    int display = 0;      // display= (assoc_replay)
    int colour = 0; char col_json[240] = "";      // colour= (assoc_replay)
    int drop = 1, together = 0; long long landmarks_deleted = 0;      // drop= / together= (facade with churn=)
    std::vector<std::pair<std::string, int>> sets;
    for (int a = 3; a < argc; a++) {
        if (!strncmp(argv[a], "mode=", 5)) mode = argv[a] + 5;
        else if (!strncmp(argv[a], "frames=", 7)) K = atoi(argv[a] + 7);
        else if (!strncmp(argv[a], "warmup=", 7)) W = atoi(argv[a] + 7);
        else if (!strncmp(argv[a], "hint=", 5)) hint = atoi(argv[a] + 5);
        else if (!strncmp(argv[a], "churn=", 6)) churn = atoi(argv[a] + 6);
        else if (!strncmp(argv[a], "ransac=", 7)) { ransac = atoi(argv[a] + 7); ransac_thr = atof(argv[a] + 7); }
        else if (!strncmp(argv[a], "rescue=", 7)) rescue = atoi(argv[a] + 7);
        else if (!strncmp(argv[a], "ellipsoids=", 11)) ellipsoids = atoi(argv[a] + 11);
        else if (!strncmp(argv[a], "joint=", 6)) joint = atoi(argv[a] + 6);
        else if (!strncmp(argv[a], "block=", 6)) block_frames = atoi(argv[a] + 6);
        else if (!strncmp(argv[a], "unique=", 7)) { checked = true; char* e = nullptr; mpar.ratio = strtod(argv[a] + 7, &e); if (e && *e == ',') mpar.exclusion = atoi(e + 1); }
        else if (!strncmp(argv[a], "archive=", 8)) { char* e = nullptr; arcL = (int)strtol(argv[a] + 8, &e, 10); if (e && *e == ',') apar.half_cap = atoi(e + 1); }
        else if (!strncmp(argv[a], "archive_step=", 13)) arc_step = atoi(argv[a] + 13);
        else if (!strncmp(argv[a], "profile=", 8)) profile = atoi(argv[a] + 8);
        else if (!strncmp(argv[a], "policy=", 7)) policy = atoi(argv[a] + 7);
        else if (!strncmp(argv[a], "resume=", 7)) resume = atoi(argv[a] + 7) != 0;
        else if (!strncmp(argv[a], "stop=", 5)) stop_k = atoi(argv[a] + 5);
        else if (!strncmp(argv[a], "display=", 8)) display = atoi(argv[a] + 8) != 0;
        else if (!strncmp(argv[a], "colour=", 7)) colour = atoi(argv[a] + 7) != 0;
        else if (!strncmp(argv[a], "drop=", 5)) drop = atoi(argv[a] + 5);
        else if (!strncmp(argv[a], "together=", 9)) together = atoi(argv[a] + 9) != 0;
        else if (!strncmp(argv[a], "subpix=", 7)) { if (atoi(argv[a] + 7)) { checked = true; mpar.subpixel = 1; } }
        else if (!strncmp(argv[a], "set=", 4)) { const char* q = strchr(argv[a] + 4, ':'); if (!q) { fprintf(stderr, "set=key:value\n"); return 2; } sets.emplace_back(std::string((const char*)argv[a] + 4, (size_t)(q - (argv[a] + 4))), atoi(q + 1)); }
    }
    for (auto& kv : sets) (void)srukf_debug_set(nullptr, kv.first.c_str(), kv.second);      // process-wide keys (e.g. set=timing:1) apply in every mode; per-filter keys: mode=capi, below
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int N = 0, F = 0; double a4[4];
    if (fread(&N, 4, 1, f) != 1 || fread(&F, 4, 1, f) != 1 || fread(a4, 8, 4, f) != 4) return 2;
    const int n = 6 * N + 4;
    std::vector<double> X0(n), S0((size_t)n * n), z((size_t)F * 2 * N);
    if (fread(X0.data(), 8, n, f) != (size_t)n || fread(S0.data(), 8, (size_t)n * n, f) != (size_t)n * n || fread(z.data(), 8, z.size(), f) != z.size()) { fprintf(stderr, "short scene file\n"); return 2; }
    fclose(f);
    if (W + K > F) { fprintf(stderr, "scene has %d frames, need %d\n", F, W + K); return 2; }
    // odometry: the reference's text format "%d : %*lf %lf %lf %lf" (SLAM.cpp:462-496)
    std::vector<double> odo;
    {
        FILE* o = fopen(argv[2], "r");
        if (!o) { perror(argv[2]); return 2; }
        char line[500];
        while (fgets(line, sizeof line, o)) { int id; double x, y, th; if (sscanf(line, "%d : %*f %lf %lf %lf", &id, &x, &y, &th) == 4) { odo.push_back(x); odo.push_back(y); odo.push_back(th); } }
        fclose(o);
    }
    if ((int)odo.size() / 3 < F + 1) { fprintf(stderr, "odometry has %d poses, need %d\n", (int)odo.size() / 3, F + 1); return 2; }

    double t_timed = 0.0, pose[4] = { 0, 0, 0, 0 }, P4[16] = { 0 };
    double tcall[5] = { 0, 0, 0, 0, 0 };                      // capi / assoc: host time inside predict_motion, predict_measurement, the association, update, get_robot
    long long matches_dev = 0;
    long long flag_ticks = -1;                                       // last frame: start of the frame's first launch -> h / Si / visible flagged to the host (10 ns ticks)
    char churn_json[900] = "";
    char ell_json[200] = "";
    char prof_json[1600] = "", arc_json[200] = "", pol_json[760] = "";
    int joint_flagged = 0;
    const char* replay_form = "run_frames_async + synchronize";
    int flagged_blocks = 0;
    const bool areplay = mode == "assoc_replay";
    if (checked && !areplay) { fprintf(stderr, "unique= / subpix= belong to mode=assoc_replay\n"); return 2; }
    if ((arcL || arc_step || profile || policy) && !areplay) { fprintf(stderr, "archive= / archive_step= / profile= / policy= belong to mode=assoc_replay\n"); return 2; }
    if (arcL < 0 || arcL > 64 || (arc_step && !arcL)) { fprintf(stderr, "archive=<L>: 1 <= L <= 64 (archive_step=1 needs it)\n"); return 2; }
    if (display && !areplay) { fprintf(stderr, "display= belongs to mode=assoc_replay\n"); return 2; }
    if (colour && !areplay) { fprintf(stderr, "colour= belongs to mode=assoc_replay\n"); return 2; }
    if ((resume >= 0 || stop_k) && !areplay) { fprintf(stderr, "resume= / stop= belong to mode=assoc_replay\n"); return 2; }
    if (stop_k && (resume < 0 || stop_k < 1 || stop_k >= block_frames || arcL || profile)) { fprintf(stderr, "stop=<k> needs resume=0|1 and 0 < k < block, without archive= and profile=\n"); return 2; }
    const int legs = stop_k ? 2 : 1;                                // stop=: both routes, the one asked for last (it is the one reported)
    double leg_pose[2][4 + 16] = { { 0 } };
    if (areplay && (block_frames < 1 || W < 1)) { fprintf(stderr, "assoc_replay: block >= 1 and warmup >= 1 (frame 0 sets the appearance records up)\n"); return 2; }
    if ((drop != 1 || together) && !(mode == "facade" && churn > 0)) { fprintf(stderr, "drop= / together= belong to mode=facade churn=P\n"); return 2; }
    if (drop < 1 || drop > 16) { fprintf(stderr, "drop=<k>: 1 <= k <= 16\n"); return 2; }
    if (mode == "facade") {
        monoslam::CSLAM SLAM;
        SLAM.deleteTogether = together != 0;
        SLAM.m_params.a1 = a4[0]; SLAM.m_params.a2 = a4[1]; SLAM.m_params.a3 = a4[2]; SLAM.m_params.a4 = a4[3];
        SLAM.isUseRANSAC = ransac != 0;
        SLAM.jointUpdate = joint != 0;
        SLAM.ellipsoidsOnDevice = ellipsoids != 0;
        if (!SLAM.setMap(N, X0.data(), S0.data(), nullptr)) { fprintf(stderr, "%s\n", SLAM.lastError.c_str()); return 1; }
        SLAM.MIN_STEP_X = SLAM.MIN_STEP_Y = 0.0;
        if (!SLAM.loadOdometryData(argv[2])) { fprintf(stderr, "%s\n", SLAM.lastError.c_str()); return 1; }
        unsigned long long rs = 0x9E3779B97F4A7C15ull;
        auto rnd = [&rs]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (double)(rs >> 11) / 9007199254740992.0; };      // xorshift, [0, 1)
        auto gauss = [&rnd]() { double s = 0; for (int q = 0; q < 12; q++) s += rnd(); return s - 6.0; };
        int victim_turn = 0;
        if (churn > 0) {
            SLAM.dataAssociation = [&](monoslam::CSLAM& s) {
                const int fr = s.m_frame.counter - 1;
                const bool change = fr >= 10 && fr % churn == 0;
                int idx = 0, victim = -1;
                std::vector<int> more;                                                                          // drop > 1: the victims behind the first
                if (change) {
                    // the next landmark (from a rotating start) that has been predicted often enough for the rule to remove it in THIS frame
                    const int start = (victim_turn * 7) % s.m_nMapFeatures; victim_turn++;
                    for (int q = 0; q < s.m_nMapFeatures && (victim < 0 || (int)more.size() < drop - 1); q++) {
                        const int k = (start + q) % s.m_nMapFeatures;
                        if (s.map[k].nPredictTimes < 10) continue;
                        if (victim < 0) { victim = k; continue; }
                        bool neighbour = std::abs(k - victim) <= 1;                                             // (the walk skips the node behind a deleted one)
                        for (int v : more) neighbour = neighbour || std::abs(k - v) <= 1;
                        if (!neighbour) more.push_back(k);
                    }
                    s.isAdding = true;
                }
                for (monoslam::PointsMap* mp = s.map; NULL != mp; mp = mp->next, idx++) {
                    mp->isMatching = mp->isVisible;
                    mp->matchLocation.x = mp->predictLocation.x + 0.5 * gauss(); mp->matchLocation.y = mp->predictLocation.y + 0.5 * gauss();
                    const bool starve = idx == victim || std::find(more.begin(), more.end(), idx) != more.end();
                    if (starve && mp->nPredictTimes >= 10) { mp->isMatching = false; mp->nMatchTimes = 0; }      // the policy's rule 2443: it leaves in this frame
                }
            };
            SLAM.addFeatures = [&](monoslam::CSLAM& s, std::vector<double>& kp) {
                s.isAdding = false;
                kp.assign({ 60.0 + 520.0 * rnd(), 60.0 + 360.0 * rnd() });                                  // one key point where the detector "found" a corner
                for (int q = 1; q < drop; q++) { kp.push_back(60.0 + 520.0 * rnd()); kp.push_back(60.0 + 360.0 * rnd()); }      // (drop=<k>: k of them)
                return drop;
            };
        } else
        SLAM.dataAssociation = [&](monoslam::CSLAM& s) {
            const int fr = s.m_frame.counter - 1;
            for (monoslam::PointsMap* mp = s.map; NULL != mp; mp = mp->next) {
                const double* zz = &z[(size_t)fr * 2 * N + 2 * ((mp->ID - 1) % N)];
                mp->isMatching = mp->isVisible; mp->matchLocation.x = zz[0]; mp->matchLocation.y = zz[1];
            }
        };
        for (int fr = 0; fr < W; fr++) SLAM.SLAM();
        long long fast0 = 0, slow0 = 0, fast1 = 0, slow1 = 0;
        srukf_debug_get(SLAM.context(), "step_fast", &fast0); srukf_debug_get(SLAM.context(), "step_slow", &slow0);
        const double add0 = SLAM.m_addTime, del0 = SLAM.m_deleteTime; const int na0 = SLAM.m_nAddCalls, nd0 = SLAM.m_nDeleteCalls;
        const double t0 = now_s();
        double by_phase[4] = { 0, 0, 0, 0 }; int n_phase[4] = { 0, 0, 0, 0 };      // churn: frames by distance from the last map change (0: the frame that changes the map, 1: the NEED_REORDER frame, 2, 3+)
        for (int fr = 0; fr < K; fr++) {
            const int counter = SLAM.m_frame.counter - 1;
            const double f0 = now_s();
            SLAM.SLAM();
            landmarks_deleted += SLAM.m_nDeletes;
            if (churn > 0) { const int ph = counter >= 10 ? (counter % churn < 3 ? counter % churn : 3) : 3; by_phase[ph] += now_s() - f0; n_phase[ph]++; }
        }
        t_timed = now_s() - t0;
        if (ellipsoids) snprintf(ell_json, sizeof ell_json, "\"facade_ellipsoids_on_device\": {\"frames_per_s\": %.2f, \"us_per_frame\": %.2f}, ", K / t_timed, t_timed / K * 1e6);
        // (the counters live in the context, and a map change rebuilds the context behind the handle: they restart with it — so the split is read from the facade's
        //  own bookkeeping where the library cannot give it: frames since the last rebuild)
        srukf_debug_get(SLAM.context(), "step_fast", &fast1); srukf_debug_get(SLAM.context(), "step_slow", &slow1);
        if (churn > 0) {
            const int na = SLAM.m_nAddCalls - na0, nd = SLAM.m_nDeleteCalls - nd0;
            snprintf(churn_json, sizeof churn_json, "\"churn\": {\"every_frames\": %d, \"additions\": %d, \"deletions\": %d, \"ms_per_addition\": %.3f, \"ms_per_deletion\": %.3f, "
                     "\"map_change_share_of_wall\": %.3f, \"landmarks_at_end\": %d, \"step_fast_since_last_rebuild\": %lld, \"step_slow_since_last_rebuild\": %lld, "
                     "\"us_per_frame_by_distance_from_the_change\": {\"0_changes_the_map\": %.1f, \"1_need_reorder\": %.1f, \"2\": %.1f, \"3_and_later\": %.1f}}, ",
                     churn, na, nd, na ? (SLAM.m_addTime - add0) / na * 1e3 : 0.0, nd ? (SLAM.m_deleteTime - del0) / nd * 1e3 : 0.0,
                     (SLAM.m_addTime - add0 + SLAM.m_deleteTime - del0) / t_timed, SLAM.m_nMapFeatures, fast1, slow1,
                     n_phase[0] ? by_phase[0] / n_phase[0] * 1e6 : 0.0, n_phase[1] ? by_phase[1] / n_phase[1] * 1e6 : 0.0, n_phase[2] ? by_phase[2] / n_phase[2] * 1e6 : 0.0,
                     n_phase[3] ? by_phase[3] / n_phase[3] * 1e6 : 0.0);
            if (drop != 1 || together) {                                                                        // beside ms_per_deletion (per call), and only then
                char extra[120];
                snprintf(extra, sizeof extra, "\"deletion_calls\": %d, \"landmarks_deleted\": %lld, \"drop\": %d, \"together\": %d, ", nd, landmarks_deleted, drop, together);
                std::string cj = churn_json; const size_t at = cj.find("\"map_change_share_of_wall\"");
                if (at != std::string::npos) { cj.insert(at, extra); snprintf(churn_json, sizeof churn_json, "%s", cj.c_str()); }
            }
        }
        if (!SLAM.lastError.empty()) { fprintf(stderr, "%s\n", SLAM.lastError.c_str()); return 1; }
        joint_flagged = SLAM.m_nJointFlagged;
        const int nn = SLAM.m_X_k.rows;
        for (int e = 0; e < 4; e++) pose[e] = SLAM.m_X_k.at(nn - 4 + e, 0);
        P4[0] = SLAM.m_P_k.at(nn - 4, nn - 4); P4[1] = SLAM.m_P_k.at(nn - 4, nn - 3); P4[4] = SLAM.m_P_k.at(nn - 3, nn - 4); P4[5] = SLAM.m_P_k.at(nn - 3, nn - 3);
        if (!churn && SLAM.m_nMapFeatures != N) { fprintf(stderr, "the map changed size (%d landmarks left)\n", SLAM.m_nMapFeatures); return 1; }
    } else if (mode == "replay") {
        srukf_params p;
        srukf_default_params(&p);
        p.a1 = a4[0]; p.a2 = a4[1]; p.a3 = a4[2]; p.a4 = a4[3];
        srukf_ctx* c = nullptr;
        int rc = srukf_create(&c, N, &p, 0, nullptr);
        if (rc) { fprintf(stderr, "srukf_create: %d %s\n", rc, srukf_last_error(nullptr)); return 1; }
#define CK(call) do { rc = (call); if (rc) { fprintf(stderr, "%s: %d %s\n", #call, rc, srukf_last_error(c)); return 1; } } while (0)
        for (auto& kv : sets) CK(srukf_debug_set(c, kv.first.c_str(), kv.second));
        CK(srukf_set_state(c, X0.data(), S0.data()));
        const int upd = joint ? SRUKF_UPDATE_JOINT : SRUKF_UPDATE_BATCHED;
        std::vector<int> m((size_t)(W + K) * N, 1);               // the host's association of capi: every visible landmark found where the scene put it
        CK(srukf_stage_sequence(c, W + K, odo.data(), z.data(), m.data()));
        // rc of a block: 0, 1 (error, reported) or 2: a frame was flagged (theta clamp; srukf_synchronize's SRUKF_ERR_CLAMP_PENDING) and the state is no longer valid
        auto block = [&](int first, int count) -> int {
            rc = srukf_run_frames_async(c, first, count, upd, nullptr);
            if (rc == SRUKF_OK) rc = srukf_synchronize(c);
            if (rc == SRUKF_ERR_CLAMP_PENDING) return 2;
            if (rc) { fprintf(stderr, "replay block [%d, %d): %d %s\n", first, first + count, rc, srukf_last_error(c)); return 1; }
            return 0;
        };
        int st = W > 0 ? block(0, W) : 0;
        double t0 = now_s();
        if (st == 0) st = block(W, K);
        if (st == 1) return 1;
        if (st == 2) {
            // as a host of the asynchronous calls is told to: back to the state the run started from, and through srukf_run_frames, which repeats a flagged frame on the
            // exact path by itself; the timed block is then that call ("replay_form" says which one was timed)
            replay_form = "run_frames (a block was flagged)";
            CK(srukf_set_state(c, X0.data(), S0.data()));
            if (W > 0) CK(srukf_run_frames(c, 0, W, upd, nullptr));
            long long e0 = 0, e1 = 0;
            srukf_debug_get(c, "exact_frames", &e0);
            t0 = now_s();
            CK(srukf_run_frames(c, W, K, upd, nullptr));
            srukf_debug_get(c, "exact_frames", &e1);
            joint_flagged = (int)(e1 - e0);
        }
        CK(srukf_get_robot(c, pose, P4));
        t_timed = now_s() - t0;
        srukf_destroy(c);
#undef CK
    } else for (int leg = 0; leg < legs; leg++) {
        const int snap = legs == 2 ? (leg == 0 ? !resume : resume) : (resume > 0 ? 1 : 0);
        matches_dev = 0; ambiguous = refined = 0; pol_change = pol_deletes = pol_adds = 0; rs_outlier = rs_low = 0; rq_high = 0; stop_blocks = 0; flagged_blocks = 0;
        srukf_params p;
        srukf_default_params(&p);
        p.a1 = a4[0]; p.a2 = a4[1]; p.a3 = a4[2]; p.a4 = a4[3];
        srukf_ctx* c = nullptr;
        int rc = srukf_create(&c, N, &p, 0, nullptr);
        if (rc) { fprintf(stderr, "srukf_create: %d %s\n", rc, srukf_last_error(nullptr)); return 1; }
#define CK(call) do { rc = (call); if (rc) { fprintf(stderr, "%s: %d %s\n", #call, rc, srukf_last_error(c)); return 1; } } while (0)
        for (auto& kv : sets) CK(srukf_debug_set(c, kv.first.c_str(), kv.second));
        CK(srukf_set_state(c, X0.data(), S0.data()));
        std::vector<double> h(2 * N), Si(4 * N), zc(2 * N), corr(N);
        std::vector<int> vis(N), m(N), md(N);
        std::vector<unsigned char> gray;
        const bool assoc = mode == "assoc" || areplay;
        if (assoc) {
            // texture: box-filtered noise (11 x 11), 640 x 480; every landmark's init patch is cut from it around its first predicted pixel, "created" at the start pose
            const int Wd = 640, Hd = 480;
            std::vector<double> t((size_t)Wd * Hd);
            unsigned long long s = 88172645463325252ull;
            for (auto& v : t) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; v = (double)(s & 0xffff); }
            std::vector<double> b((size_t)Wd * Hd, 0.0);
            for (int y = 0; y < Hd; y++) for (int x = 0; x < Wd; x++) {
                double acc = 0; for (int dy = -5; dy <= 5; dy++) for (int dx = -5; dx <= 5; dx++) acc += t[(size_t)((y + dy + Hd) % Hd) * Wd + (x + dx + Wd) % Wd];
                b[(size_t)y * Wd + x] = acc;
            }
            double lo = b[0], hi = b[0]; for (double v : b) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
            gray.resize((size_t)Wd * Hd);
            for (size_t q = 0; q < gray.size(); q++) gray[q] = (unsigned char)((b[q] - lo) / (hi - lo) * 255.0);
            CK(srukf_predict_motion(c, &odo[0], &odo[3]));
            CK(srukf_predict_measurement(c, h.data(), Si.data(), vis.data()));
            for (int k = 0; k < N; k++) zc[2 * k] = z[2 * k], zc[2 * k + 1] = z[2 * k + 1];
            for (int k = 0; k < N; k++) m[k] = vis[k];
            const double th = X0[n - 1], R[9] = { cos(th), -sin(th), 0, sin(th), cos(th), 0, 0, 0, 1 }, tr[3] = { X0[n - 4], X0[n - 3], X0[n - 2] };
            for (int k = 0; k < N; k++) {
                double px[2] = { h[2 * k], h[2 * k + 1] };
                int cu = (int)lround(px[0]), cv = (int)lround(px[1]);
                if (!(cu >= 20 && cu < Wd - 20 && cv >= 20 && cv < Hd - 20)) { cu = 320; cv = 240; px[0] = 320; px[1] = 240; }
                unsigned char patch[441];
                for (int i = 0; i < 21; i++) for (int j = 0; j < 21; j++) patch[21 * i + j] = gray[(size_t)(cv - 10 + i) * Wd + cu - 10 + j];
                CK(srukf_set_landmark_appearance(c, k, patch, R, tr, px));
            }
            CK(srukf_update(c, zc.data(), m.data(), SRUKF_NEEDNOT_REORDER, SRUKF_UPDATE_BATCHED));
        }
        const int f0 = assoc ? 1 : 0;
        double t0 = 0.0;
        if (areplay) {
            const int upd = joint ? SRUKF_UPDATE_JOINT : SRUKF_UPDATE_BATCHED;
            const size_t img = gray.size();
            {
                std::vector<double> z0((size_t)(W + K) * 2 * N, 0.0);       // the rows the image runs write
                std::vector<int> m0((size_t)(W + K) * N, 0);
                CK(srukf_stage_sequence(c, W + K, odo.data(), z0.data(), m0.data()));
                std::vector<unsigned char> stack((size_t)(W + K) * img);
                for (int fr = 0; fr < W + K; fr++) memcpy(stack.data() + (size_t)fr * img, gray.data(), img);
                auto ms = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count() * 1e3; };
                auto ta = std::chrono::steady_clock::now();
                CK(srukf_stage_images(c, W + K, stack.data()));
                const double t_gray = ms(ta);
                if (colour) {
                    std::vector<unsigned char> bgr(3 * stack.size()), back(stack.size());
                    for (size_t q = 0; q < stack.size(); q++) bgr[3 * q] = bgr[3 * q + 1] = bgr[3 * q + 2] = stack[q];
                    ta = std::chrono::steady_clock::now();                   // what a host without the call does: loadPictures' rule on the CPU
                    for (size_t q = 0; q < stack.size(); q++) back[q] = (unsigned char)((4899u * bgr[3 * q] + 9617u * bgr[3 * q + 1] + 1868u * bgr[3 * q + 2] + 8192u) >> 14);
                    const double t_host = ms(ta);
                    if (back != stack) { fprintf(stderr, "colour=1: the host conversion changed a B = G = R frame\n"); return 3; }
                    double t_bgr[2];
                    for (int keep = 0; keep < 2; keep++) { ta = std::chrono::steady_clock::now(); CK(srukf_stage_images_bgr(c, W + K, bgr.data(), keep)); t_bgr[keep] = ms(ta); }
                    snprintf(col_json, sizeof col_json, "\"staging_ms\": {\"frames\": %d, \"stage_images\": %.3f, \"host_conversion\": %.3f, \"stage_images_bgr_keep0\": %.3f, \"stage_images_bgr_keep1\": %.3f}, ",
                             W + K, t_gray, t_host, t_bgr[0], t_bgr[1]);
                }
            }
            if (arcL) {
                // the archive: arcL landmarks created on a context of their own at the robot's start state, at the grid pixels farthest from every landmark's first
                // predicted pixel (h still holds frame 0's), their appearance captured from the bench's frame, their records read back
                std::vector<double> uv;
                std::vector<std::pair<double, std::pair<int, int>>> cand;
                for (int y = 40; y <= 440; y += 20) for (int x = 40; x <= 600; x += 20) {
                    double dmin = 1e30;
                    for (int k = 0; k < N; k++) { const double d = hypot(h[2 * k] - x, h[2 * k + 1] - y); dmin = d < dmin ? d : dmin; }
                    cand.push_back({ -dmin, { x, y } });
                }
                std::sort(cand.begin(), cand.end());
                for (auto& cd : cand) {
                    if ((int)uv.size() == 2 * arcL) break;
                    bool ok = true;
                    for (size_t q = 0; q < uv.size(); q += 2) if (hypot(uv[q] - cd.second.first, uv[q + 1] - cd.second.second) < 30.0) ok = false;
                    if (ok) { uv.push_back(cd.second.first); uv.push_back(cd.second.second); }
                }
                if ((int)uv.size() != 2 * arcL) { fprintf(stderr, "archive=: no room for %d records\n", arcL); return 2; }
                srukf_ctx* c2 = nullptr;
                rc = srukf_create(&c2, 0, &p, 0, nullptr);
                if (rc) { fprintf(stderr, "srukf_create (archive): %d %s\n", rc, srukf_last_error(nullptr)); return 1; }
                const double X4[4] = { X0[n - 4], X0[n - 3], X0[n - 2], X0[n - 1] };
                double S4[16] = { 0 }; S4[0] = p.sigma_x; S4[5] = p.sigma_y; S4[10] = p.sigma_z; S4[15] = p.sigma_theta;
                std::vector<double> aX((size_t)6 * arcL), aS((size_t)36 * arcL), aR((size_t)9 * arcL), aT((size_t)3 * arcL), aP((size_t)2 * arcL);
                std::vector<unsigned char> aPatch((size_t)441 * arcL);
                rc = srukf_set_state(c2, X4, S4);
                if (!rc) rc = srukf_add_landmarks(c2, arcL, uv.data());
                if (!rc) rc = srukf_capture_appearance(c2, 0, arcL, uv.data(), gray.data());
                for (int k = 0; k < arcL && !rc; k++) {
                    int has = 0;
                    rc = srukf_get_landmark_record(c2, k, &aX[6 * k], &aS[36 * k], &aPatch[441 * k], &aR[9 * k], &aT[3 * k], &aP[2 * k], &has);
                    if (!rc && !has) rc = SRUKF_ERR_SEQUENCE;
                }
                if (rc) { fprintf(stderr, "archive records: %d %s\n", rc, srukf_last_error(c2)); return 1; }
                srukf_destroy(c2);
                CK(srukf_archive_set(c, arcL, aX.data(), aS.data(), aPatch.data(), aR.data(), aT.data(), aP.data()));
                if (!arc_step) CK(srukf_images_search_archive(c, 1, &apar));
            }
            if (policy) CK(srukf_images_policy(c, 1, nullptr));
            if (ransac_thr > 0.0) CK(srukf_images_ransac(c, 1, ransac_thr));
            if (ransac_thr > 0.0 && rescue) CK(srukf_images_rescue_gate(c, 1, 5.99146454710798));
            if (snap) CK(srukf_images_snapshots(c, 1));
            if (display) CK(srukf_images_display(c, 1));
            std::vector<int> rlow(block_frames), ract(block_frames), rinl(N), rhigh(block_frames);
            std::vector<srukf_policy_summary> prow(block_frames);
            std::vector<int> mrow((size_t)block_frames * N), frow(checked ? (size_t)block_frames * N : 0), fl(checked ? N : 0), hrow(block_frames), am(arcL);
            auto run = [&](int first, int end, bool timed) -> int {
                int step = block_frames;
                for (int b = first; b < end; b += step) {
                    const int cnt = end - b < block_frames ? end - b : block_frames;
                    step = block_frames;
                    rc = checked ? srukf_run_images_checked_async(c, b, cnt, upd, &mpar, nullptr) : srukf_run_images_async(c, b, cnt, upd, nullptr);
                    if (rc == SRUKF_OK) rc = srukf_synchronize(c);
                    const bool clean = rc == SRUKF_OK;
                    if (rc == SRUKF_ERR_CLAMP_PENDING) {
                        // the block came back restored (X, S, matchPatch): its frames step by step, the device's association driving the filter as in the block
                        if (timed) flagged_blocks++;
                        for (int fr = b; fr < b + cnt; fr++) {
                            CK(srukf_predict_motion(c, &odo[3 * fr], &odo[3 * fr + 3]));
                            CK(srukf_predict_measurement(c, h.data(), Si.data(), vis.data()));
                            if (checked) {
                                CK(srukf_associate_checked(c, gray.data(), &mpar, zc.data(), md.data(), corr.data(), nullptr, nullptr, fl.data()));
                                if (timed) for (int k = 0; k < N; k++) { ambiguous += (fl[k] >> 1) & 1; refined += (fl[k] >> 2) & 1; }
                            } else
                            CK(srukf_associate(c, gray.data(), zc.data(), md.data(), corr.data()));
                            if (ransac_thr > 0.0) {              // (the consensus step-wise: the update takes matched & inlier, as the frames of a block do)
                                int na = 0; for (int k = 0; k < N; k++) na += (md[k] != 0 && vis[k] != 0) ? 1 : 0;
                                if (na >= 2) {
                                    CK(srukf_ransac_consensus(c, zc.data(), md.data(), ransac_thr, rinl.data(), nullptr, nullptr, nullptr));
                                    int nl = 0; for (int k = 0; k < N; k++) { md[k] = (md[k] != 0 && rinl[k] != 0) ? 1 : 0; nl += md[k]; }
                                    if (timed) { rs_low += nl; rs_outlier += nl < na ? 1 : 0; }
                                }
                            }
                            if (timed) for (int k = 0; k < N; k++) matches_dev += md[k];
                            if (joint) CK(srukf_update_joint(c, zc.data(), md.data(), SRUKF_NEEDNOT_REORDER));
                            else CK(srukf_update(c, zc.data(), md.data(), SRUKF_NEEDNOT_REORDER, SRUKF_UPDATE_BATCHED));
                            if (arcL) {                          // (a restored block leaves no search record either: the step-wise search, per frame)
                                CK(srukf_archive_search(c, gray.data(), &apar, nullptr, nullptr, nullptr, nullptr, am.data(), nullptr));
                                if (timed) for (int q = 0; q < arcL; q++) arc_hits += am[q];
                            }
                        }
                    } else if (rc) { fprintf(stderr, "image block [%d, %d): %d %s\n", b, b + cnt, rc, srukf_last_error(c)); return 1; }
                    else if (timed) {
                        // (the record is the host's to read after every block: nPredictTimes / nMatchTimes and the border test need it)
                        CK(srukf_get_image_matches(c, b, cnt, nullptr, mrow.data(), nullptr, nullptr, nullptr));
                        for (int q = 0; q < cnt * N; q++) matches_dev += mrow[q];
                        if (checked) {
                            CK(srukf_get_image_checks(c, b, cnt, nullptr, nullptr, frow.data()));
                            for (int q = 0; q < cnt * N; q++) { ambiguous += (frow[q] >> 1) & 1; refined += (frow[q] >> 2) & 1; }
                        }
                        if (policy) {                            // "does the map have to change?": cnt summaries
                            int fc = -1;
                            CK(srukf_get_image_policy(c, b, cnt, nullptr, prow.data(), nullptr, &fc));
                            for (int q = 0; q < cnt; q++) { pol_change += prow[q].change; pol_deletes += prow[q].n_deletes; pol_adds += prow[q].need_add; }
                        }
                        if (ransac_thr > 0.0) {                  // "which frame needs the rescue?": cnt summaries
                            int fo = -1;
                            CK(srukf_get_image_ransac(c, b, cnt, nullptr, nullptr, nullptr, nullptr, ract.data(), rlow.data(), &fo));
                            for (int q = 0; q < cnt; q++) if (ract[q] >= 2) { rs_low += rlow[q]; rs_outlier += rlow[q] < ract[q] ? 1 : 0; }
                            if (rescue) {                        // "which frame really needs it?": cnt summaries more
                                int fr = -1;
                                CK(srukf_get_image_rescue(c, b, cnt, nullptr, nullptr, nullptr, nullptr, nullptr, rhigh.data(), &fr));
                                for (int q = 0; q < cnt; q++) rq_high += rhigh[q] > 0 ? 1 : 0;
                            }
                        }
                        if (arcL && !arc_step) {                 // "did anything come back?": cnt ints
                            CK(srukf_get_image_archive(c, b, cnt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, hrow.data()));
                            for (int q = 0; q < cnt; q++) arc_hits += hrow[q];
                        }
                    }
                    if (clean && timed && stop_k && cnt > stop_k) {      // the block has to stop behind its first stop_k frames
                        if (snap) CK(srukf_images_resume(c, stop_k));
                        else {
                            CK(srukf_images_rewind(c));
                            rc = checked ? srukf_run_images_checked_async(c, b, stop_k, upd, &mpar, nullptr) : srukf_run_images_async(c, b, stop_k, upd, nullptr);
                            if (rc == SRUKF_OK) rc = srukf_synchronize(c);
                            if (rc) { fprintf(stderr, "image block [%d, %d) again: %d %s\n", b, b + stop_k, rc, srukf_last_error(c)); return 1; }
                        }
                        stop_blocks++;
                        step = stop_k;
                    }
                    if (clean && arcL && arc_step) {    // the step-wise route: one search on the posterior of the block's last frame
                        CK(srukf_archive_search(c, gray.data(), &apar, nullptr, nullptr, nullptr, nullptr, am.data(), nullptr));
                        if (timed) for (int q = 0; q < arcL; q++) arc_hits += am[q];
                    }
                }
                return 0;
            };
            if (run(f0, W, false)) return 1;
            if (profile) { CK(srukf_set_profiling(c, 1)); CK(srukf_profile_reset(c)); }
            t0 = now_s();
            if (run(W, W + K, true)) return 1;
            CK(srukf_get_robot(c, pose, P4));
            if (profile) {
                size_t o = (size_t)snprintf(prof_json, sizeof prof_json, "\"profile_ms_per_frame\": {");
                bool first_class = true;
                for (int i = 0; i < srukf_profile_count(c); i++) {
                    const char* name = nullptr; double ms = 0, fl_ = 0, by_ = 0; long long ln = 0;
                    CK(srukf_profile_get(c, i, &name, &ms, &ln, &fl_, &by_));
                    if (ln > 0 && o < sizeof prof_json - 80) { o += (size_t)snprintf(prof_json + o, sizeof prof_json - o, "%s\"%s\": %.5f", first_class ? "" : ", ", name, ms / K); first_class = false; }
                }
                snprintf(prof_json + o, sizeof prof_json - o, "}, ");
            }
        } else
        for (int fr = f0; fr < W + K; fr++) {
            if (fr == W) t0 = now_s();
            const double s0 = now_s();
            if (hint && fr + 2 <= F) CK(srukf_predict_motion_next(c, &odo[3 * fr + 3], &odo[3 * fr + 6]));      // (before the predict: its first launch then carries the third pose too)
            CK(srukf_predict_motion(c, &odo[3 * fr], &odo[3 * fr + 3]));
            const double s1 = now_s();
            CK(srukf_predict_measurement(c, h.data(), Si.data(), vis.data()));
            const double s2 = now_s();
            if (assoc) { CK(srukf_associate(c, gray.data(), zc.data(), md.data(), corr.data())); for (int k = 0; k < N; k++) matches_dev += md[k]; }
            const double* zz = &z[(size_t)fr * 2 * N];
            for (int k = 0; k < N; k++) m[k] = vis[k];                 // the host's association: every visible landmark found where the scene put it
            const double s3 = now_s();
            if (joint) { CK(srukf_update_joint(c, zz, m.data(), SRUKF_NEEDNOT_REORDER)); int ffr = -1; if (srukf_clamp_info(c, &ffr, nullptr) == SRUKF_OK && ffr >= 0) joint_flagged++; }
            else CK(srukf_update(c, zz, m.data(), SRUKF_NEEDNOT_REORDER, SRUKF_UPDATE_BATCHED));
            const double s4 = now_s();
            CK(srukf_get_robot(c, pose, P4));
            if (fr >= W) { tcall[0] += s1 - s0; tcall[1] += s2 - s1; tcall[2] += s3 - s2; tcall[3] += s4 - s3; tcall[4] += now_s() - s4; }
        }
        t_timed = now_s() - t0;
        srukf_debug_get(c, "meas_flag_ticks", &flag_ticks);
        srukf_destroy(c);
        memcpy(leg_pose[leg], pose, sizeof pose); memcpy(leg_pose[leg] + 4, P4, sizeof P4);
    }
    if (legs == 2 && memcmp(leg_pose[0], leg_pose[1], sizeof leg_pose[0]) != 0) {
        fprintf(stderr, "stop=%d: the two routes end at different poses: resume=%d %.17g %.17g %.17g %.17g, resume=%d %.17g %.17g %.17g %.17g\n", stop_k, !resume, leg_pose[0][0], leg_pose[0][1],
                leg_pose[0][2], leg_pose[0][3], resume, leg_pose[1][0], leg_pose[1][1], leg_pose[1][2], leg_pose[1][3]);
        return 3;
    }
    char joint_json[420] = "";
    if (joint) snprintf(joint_json, sizeof joint_json, "\"joint\": 1, \"joint_flagged_frames\": %d, ", joint_flagged);
    if (areplay) snprintf(joint_json + strlen(joint_json), sizeof joint_json - strlen(joint_json), "\"block_frames\": %d, \"flagged_blocks\": %d, ", block_frames, flagged_blocks);
    if (checked) snprintf(joint_json + strlen(joint_json), sizeof joint_json - strlen(joint_json), "\"checked\": {\"ratio\": %.6g, \"exclusion\": %d, \"subpixel\": %d, \"ambiguous\": %lld, \"refined\": %lld}, ",
                          mpar.ratio, mpar.exclusion, mpar.subpixel, ambiguous, refined);
    if (arcL) snprintf(arc_json, sizeof arc_json, "\"archive\": {\"records\": %d, \"half_cap\": %d, \"route\": \"%s\", \"matched_records\": %lld}, ", arcL, apar.half_cap,
                       arc_step ? "srukf_archive_search after every block" : "srukf_images_search_archive", arc_hits);
    if (policy) snprintf(pol_json, sizeof pol_json, "\"policy\": {\"change_frames\": %lld, \"deletes\": %lld, \"need_add_frames\": %lld}, ", pol_change, pol_deletes, pol_adds);
    if (areplay && ransac_thr > 0.0 && rescue)
        snprintf(pol_json + strlen(pol_json), sizeof pol_json - strlen(pol_json), "\"ransac\": {\"threshold\": %.6g, \"outlier_frames\": %lld, \"low_inliers\": %lld, \"rescue_gate\": 1, \"rescue_frames\": %lld}, ",
                 ransac_thr, rs_outlier, rs_low, rq_high);
    else if (areplay && ransac_thr > 0.0) snprintf(pol_json + strlen(pol_json), sizeof pol_json - strlen(pol_json), "\"ransac\": {\"threshold\": %.6g, \"outlier_frames\": %lld, \"low_inliers\": %lld}, ",
                                              ransac_thr, rs_outlier, rs_low);
    if (areplay && resume >= 0) snprintf(pol_json + strlen(pol_json), sizeof pol_json - strlen(pol_json), "\"resume\": %d, ", resume);
    if (areplay && display) snprintf(pol_json + strlen(pol_json), sizeof pol_json - strlen(pol_json), "\"display\": 1, ");
    if (colour) snprintf(pol_json + strlen(pol_json), sizeof pol_json - strlen(pol_json), "%s", col_json);
    if (stop_k) snprintf(pol_json + strlen(pol_json), sizeof pol_json - strlen(pol_json), "\"stop\": {\"k\": %d, \"resume\": %d, \"blocks\": %lld, \"poses_equal\": 1}, ", stop_k, resume, stop_blocks);
    if (mode == "replay") snprintf(joint_json + strlen(joint_json), sizeof joint_json - strlen(joint_json), "\"replay_form\": \"%s\", \"exact_frames\": %d, ", replay_form, joint_flagged);
    printf("{\"mode\": \"%s\", %s%s%s%s%s%s\"hint\": %d, \"landmarks\": %d, \"frames\": %d, \"warmup\": %d, \"frames_per_s\": %.2f, \"us_per_frame\": %.2f, "
           "\"pose\": [%.17g, %.17g, %.17g, %.17g], \"P_robot\": [%.17g, %.17g, %.17g, %.17g], \"device_matches\": %lld, \"stats_flag_us_into_first_launch\": %.2f, \"host_us_per_call\": {\"predict_motion\": %.2f, \"predict_measurement\": %.2f, \"association\": %.2f, \"update\": %.2f, \"get_robot\": %.2f}, "
           "\"filter_driven_by\": \"%s\"}\n",
           mode.c_str(), churn_json, ell_json, joint_json, arc_json, pol_json, prof_json, hint, N, K, W, K / t_timed, t_timed / K * 1e6, pose[0], pose[1], pose[2], pose[3], P4[0], P4[1], P4[4], P4[5], matches_dev, flag_ticks * 0.01,
           tcall[0] / K * 1e6, tcall[1] / K * 1e6, tcall[2] / K * 1e6, tcall[3] / K * 1e6, tcall[4] / K * 1e6,
           areplay ? "device association" : "scene z / matched (host association)");
    fflush(stdout);                                                // (the line must not depend on what the runtimes' exit handlers do)
    return 0;
}
