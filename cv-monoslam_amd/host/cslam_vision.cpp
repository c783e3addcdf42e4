// cslam_vision — C++ host that runs the CSLAM facade as the reference runs: gray frame in, pose out.  The host points m_gryImage at each
// frame and installs no addFeatures callback, so SLAM() finds new landmarks on the device (detectAndfilteringFeatures / insureEnoughFeatures
// -> integrateFeaturesInformation -> srukf_capture_appearance) and associates them on the device (dataAssociationOnDevice).
//   cslam_vision frames.bin odometry.txt [redirect=<counter>] [warmup] [loops] [archive=<half_cap>] [ransac=<threshold>] [colour=1|2] [overlay=<file>] [unique=<ratio>[,<exclusion>]] [subpix=1] [joint=1] [block=<F>] [resume=1] [rescue=1] [display=<file>] [overlays=<file>] [together=1]
// frames.bin: int32 W, int32 H, int32 F, then F frames of H x W uint8.  Frame f of the loop (0-based) sees image f % F.
// redirect=<counter>: flags that odometry sample as a heading jump: predictMotion takes the redirection restart (SLAM.cpp:1354-1428), whose
//   addFeatures runs with isAdding (archived features projected, empty map).
// loops: CSLAM::reinsertLoopPoints on (the restart's isAdding addFeatures puts the archived landmarks its last pass met again back into the filter).
//   Adds, and only with it, a "reinsert" line per restart (the archive's IDs before the frame, the IDs put back, map and archive size behind the
//   restart's addFeatures, the archived X6 and sr of what was put back) and an
//   "ids" line per frame (ID and isLoop of every map node, state order).
// archive=<half_cap>: CSLAM::searchArchivedLandmarks on, together with loops (archiveSearchHalfCap = half_cap, 10 .. 40): every frame the archived landmarks are
//   looked for in the frame by appearance and the matched ones put back.  Adds, and only with it, an "archive" line per search that looked at
//   records (frame counter, records searched, map and archive size around it, the IDs put back), "reacquired <n>" on the frame line's next line, and the run's
//   counters m_nArchiveMatches / m_nArchiveRejected / m_nArchiveReacquired at the end.
// ransac=<threshold>: KalmanUpdate runs 1-point RANSAC (CSLAM::isUseRANSAC, THRESHOLD_RANSAC = threshold in pixels; 8 is the reference's constant).  Adds, and
//   only with it, a "ransac" line per frame (low- and high-innovation inliers).
// joint=1: CSLAM::jointUpdate (every update of the frame is the joint measurement update).  Adds, and only with it, a last line "joint flagged <n>".
// colour=1: every gray frame is fed as a B = G = R colour frame through CSLAM::loadPictures (srukf_set_frame_bgr) and associated on the held frame
//   (dataAssociationOnDeviceHeld).  The conversion keeps such a frame byte for byte (the weights sum to 2^14), so the output equals the default run's.
//   With block=<F> the blocks' frames go the same way through CSLAM::SLAMBlockColour.
// colour=2: frames.bin holds B, G, R frames, F frames of H x W x 3 uint8, as cvQueryFrame / cvLoadImage deliver them.  Step-wise they go through
//   CSLAM::loadPictures, with block=<F> through CSLAM::SLAMBlockColour; the output is that of the run on the frames loadPictures makes of them.
// overlay=<file>: after the last frame, CSLAM::display2DFeatureModel's bytes (H x W x 3, B G R) go to <file> and the rows they were drawn from to <file>.in:
//   per map node "h.x h.y Si00 Si01 Si10 Si11 z.x z.y matched" (%a).  Nothing else changes.
// unique=<ratio>[,<exclusion>]: CSLAM::rejectAmbiguousMatches on (AMBIGUITY_RATIO = ratio, AMBIGUITY_EXCLUSION = exclusion, default 4).  Adds, and
//   only with it, an "ambiguous <n> <IDs...>" line per frame: the landmarks this frame's association vetoed.
// subpix=1: CSLAM::subpixelMatches on.
// block=<F>: frames run through CSLAM::SLAMBlock, up to F at a time, with SLAM() for every frame a block cannot stand for (the first, a frame
//   behind an addition, a restart, a flagged block); frames.bin is then not wrapped round: at most its F frames run.  Adds, and only when given (block=1 too: the
//   step-wise route with the same lines), per frame a "policy" line (frame, the IDs updateFeaturesInformation deleted, landmarks added) and a "path" line (frame, pose and
//   the 2 x 2 position block of P, %.17g), and at the end "blocks <n> early <n> full <n> fallback <n>".  Without it nothing changes.  With ransac=<threshold> the
//   consensus runs inside the blocks and every frame's "ransac" line follows its "path" line, the same through either route; a block ends in
//   front of a frame whose consensus dropped a match, and SLAM() runs that frame with its rescue (a fallback).
// resume=1 (with block=<F>): CSLAM::resumeStoppedBlocks on: a block that stops early takes the state at the stop from its first run instead of
//   running the frames in front of the stop again; " resumed=<count>" is appended to the "blocks" line.  Without it the output is what it was.
// rescue=1 (with ransac=<threshold>): CSLAM::rescueGateOnDevice on: the rescue's chi-square test runs on the device, a block ends only in front of
//   a frame that would rescue a match, and SLAM() calls srukf_repredict_measurement only in such a frame.  With block=<F> " gate_skips=<count>" is appended to the
//   "blocks" line (the repredictions SLAM() saved).  Every other line is what it is without it.
// display=<file> (with block=<F>, block=1 too): CSLAM::blockDisplay and ellipsoidsOnDevice on; <file> gets, per frame and per landmark of the map
//   behind that frame's tail, one line "frame ID" and xyz, cov, axis, sigma as %a (a NaN as "nan" whatever its sign): for the last consumed frame of a block (and
//   every frame of block=1) from map[], for the frames in front of it from m_blockDisplay.  The same file through either route.  With overlay=<file> the overlay of
//   the last block's last consumed frame goes to <file> (CSLAM::blockOverlayLast: drawn in front of that frame's tail); stdout is what it is without both.
// overlays=<file> (with block=<F> display=<file>): CSLAM::blockOverlayAll on: the overlay of every frame a block consumed is appended to <file>,
//   H x W x 3 bytes each, in frame order (frames SLAM() ran are not among them); with colour= they are drawn on the colour frames.  Adds, and only with it, a
//   last line "overlay_frames" with the frames whose overlays the file holds.
// together=1: CSLAM::deleteTogether on: the landmarks a frame's updateFeaturesInformation deletes leave in one device call.  Every line is what it
//   is without it (the pose and covariance figures within rounding when a frame deletes more than one landmark).
// set=key:value: srukf_debug_set(NULL, key, value) for a process-wide measurement switch (set=timing:1: the phases of every map change on stderr).
// min_matches=<n>: CSLAM::m_minNUM = n (addFeatures when fewer landmarks matched, SLAM.cpp:179, 556; default 5).
// warmup: one frame of a throwaway facade first (code objects loaded, device memory pool grown), so that the timings printed are steady-state ones.
// Prints every detection pass with its inputs ("pass" blocks) and, after every frame, the map ("frame" lines + the init pixels of every landmark).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "cslam.hpp"

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s frames.bin odometry.txt [redirect=<counter>] [warmup] [loops] [archive=<half_cap>] [ransac=<threshold>] [colour=1|2] [overlay=<file>] [unique=<ratio>[,<exclusion>]] [subpix=1] [joint=1] [block=<F>] [resume=1] [rescue=1] [display=<file>] [overlays=<file>] [min_matches=<n>] [together=1]\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int W = 0, H = 0, F = 0;
    if (fread(&W, 4, 1, f) != 1 || fread(&H, 4, 1, f) != 1 || fread(&F, 4, 1, f) != 1 || W < 8 || H < 8 || F < 1) { fprintf(stderr, "bad frames file\n"); return 2; }
    int colour = 0;                                                                          // (colour=2 says what the file holds: before it is read)
    for (int a = 3; a < argc; a++) if (!strncmp(argv[a], "colour=", 7)) colour = atoi(argv[a] + 7);
    if (colour < 0 || colour > 2) { fprintf(stderr, "colour=1 or colour=2\n"); return 2; }
    const size_t fb = (size_t)W * H * (colour == 2 ? 3 : 1);                                 // bytes of one frame of the file
    std::vector<unsigned char> frames(fb * F);
    if (fread(frames.data(), 1, frames.size(), f) != frames.size()) { fprintf(stderr, "short frames file\n"); return 2; }
    fclose(f);
    int redirect = 0, archiveCap = 0; bool warmup = false, loops = false, ransac = false; double ransacThr = 8.0; std::string overlay, display, overlays;
    bool unique = false, subpix = false, joint = false, resume = false, rescue = false; double uniqueRatio = 0.9; int uniqueExcl = 4;
    bool together = false;
    int minMatches = 0, block = 0, nBlocks = 0, nEarly = 0, nFull = 0, nFallback = 0;
    for (int a = 3; a < argc; a++)
        if (!strncmp(argv[a], "redirect=", 9)) redirect = atoi(argv[a] + 9); else if (!strcmp(argv[a], "warmup")) warmup = true; else if (!strcmp(argv[a], "loops")) loops = true;
        else if (!strncmp(argv[a], "archive=", 8)) { archiveCap = atoi(argv[a] + 8); loops = true; }
        else if (!strncmp(argv[a], "ransac=", 7)) { ransac = true; ransacThr = atof(argv[a] + 7); }
        else if (!strncmp(argv[a], "colour=", 7)) {}                                          // (read above)
        else if (!strncmp(argv[a], "overlays=", 9)) overlays = argv[a] + 9;
        else if (!strncmp(argv[a], "overlay=", 8)) overlay = argv[a] + 8;
        else if (!strncmp(argv[a], "unique=", 7)) { unique = true; uniqueRatio = atof(argv[a] + 7); const char* cm = strchr(argv[a] + 7, ','); if (cm) uniqueExcl = atoi(cm + 1); }
        else if (!strncmp(argv[a], "subpix=", 7)) subpix = atoi(argv[a] + 7) != 0;
        else if (!strncmp(argv[a], "joint=", 6)) joint = atoi(argv[a] + 6) != 0;
        else if (!strncmp(argv[a], "block=", 6)) block = atoi(argv[a] + 6);
        else if (!strncmp(argv[a], "resume=", 7)) resume = atoi(argv[a] + 7) != 0;
        else if (!strncmp(argv[a], "rescue=", 7)) rescue = atoi(argv[a] + 7) != 0;
        else if (!strncmp(argv[a], "display=", 8)) display = argv[a] + 8;
        else if (!strncmp(argv[a], "min_matches=", 12)) minMatches = atoi(argv[a] + 12);
        else if (!strncmp(argv[a], "together=", 9)) together = atoi(argv[a] + 9) != 0;
        else if (!strncmp(argv[a], "set=", 4)) { const char* q = strchr(argv[a] + 4, ':'); if (!q) { fprintf(stderr, "set=key:value\n"); return 2; } (void)srukf_debug_set(nullptr, std::string((const char*)argv[a] + 4, (size_t)(q - (argv[a] + 4))).c_str(), atoi(q + 1)); }
    if (!overlays.empty() && (block < 1 || display.empty())) { fprintf(stderr, "overlays=<file> needs block=<F> and display=<file>\n"); return 2; }
    if (warmup) {
        monoslam::CSLAM w;
        w.m_params.image_w = W; w.m_params.image_h = H; w.MIN_STEP_X = w.MIN_STEP_Y = 0.0;
        if (!w.loadOdometryData(argv[2])) { fprintf(stderr, "%s\n", w.lastError.c_str()); return 1; }
        std::vector<unsigned char> g0((size_t)W * H);                                        // (any gray frame will do: colour=2 has none on the host)
        w.m_gryImage = colour == 2 ? g0.data() : frames.data();
        w.SLAM();
        if (!w.lastError.empty()) { fprintf(stderr, "warmup: %s\n", w.lastError.c_str()); return 1; }
    }

    monoslam::CSLAM SLAM;
    SLAM.m_params.image_w = W; SLAM.m_params.image_h = H;
    SLAM.MIN_STEP_X = SLAM.MIN_STEP_Y = 0.0;
    if (!SLAM.loadOdometryData(argv[2])) { fprintf(stderr, "%s\n", SLAM.lastError.c_str()); return 1; }
    if (redirect > 0) SLAM.m_odoTheta.at(2, redirect) = 1;
    SLAM.logDetectPasses = true;
    SLAM.reinsertLoopPoints = loops;
    if (archiveCap > 0) { SLAM.searchArchivedLandmarks = true; SLAM.archiveSearchHalfCap = archiveCap; }
    if (ransac) { SLAM.isUseRANSAC = true; SLAM.THRESHOLD_RANSAC = ransacThr; }
    if (unique) { SLAM.rejectAmbiguousMatches = true; SLAM.AMBIGUITY_RATIO = uniqueRatio; SLAM.AMBIGUITY_EXCLUSION = uniqueExcl; }
    SLAM.subpixelMatches = subpix;
    SLAM.jointUpdate = joint;
    SLAM.resumeStoppedBlocks = resume;
    SLAM.rescueGateOnDevice = rescue;
    SLAM.deleteTogether = together;
    if (minMatches > 0) SLAM.m_minNUM = minMatches;
    const unsigned char* cur = nullptr;
    std::vector<unsigned char> bgr;
    auto asColour = [&](const unsigned char* gray, int n) {                                  // n gray frames as B = G = R frames, in bgr
        bgr.resize((size_t)3 * W * H * n);
        for (size_t q = 0; q < (size_t)W * H * n; q++) bgr[3 * q] = bgr[3 * q + 1] = bgr[3 * q + 2] = gray[q];
        return bgr.data();
    };
    SLAM.dataAssociation = [&](monoslam::CSLAM& s) {                                         // loadPictures + dataAssociation (SLAM.cpp:95-97)
        if (!colour) { s.dataAssociationOnDevice(cur); return; }
        if (s.loadPictures(colour == 2 ? cur : asColour(cur, 1))) s.dataAssociationOnDeviceHeld();
    };
    // the gray frame the host shows the facade.  colour=2: the host has none — loadPictures fills m_grayStore and points m_gryImage at it; until the first one has
    // run the pointer only says that frames come from a camera (predictMotion builds the filter on it)
    if (colour == 2) SLAM.m_grayStore.assign((size_t)W * H, 0);
    auto showFrame = [&](const unsigned char* fr) { cur = fr; SLAM.m_gryImage = colour == 2 ? SLAM.m_grayStore.data() : fr; };
    int steps = SLAM.m_odoCounter - 1 - (redirect > 0 ? 1 : 0);
    double addWall = -1.0;
    if (block > 0) {
        // the block-wise loop: SLAMBlock where it can stand for SLAM(), SLAM() with the association installed for the frame otherwise
        if (block > 1 && (loops || archiveCap > 0)) { fprintf(stderr, "block=<F> runs without loops and archive=\n"); return 2; }
        if (steps > F) steps = F;
        const auto assoc = SLAM.dataAssociation;
        FILE* fd = nullptr;
        if (!display.empty()) {
            fd = fopen(display.c_str(), "w");
            if (!fd) { perror(display.c_str()); return 1; }
            SLAM.blockDisplay = true; SLAM.ellipsoidsOnDevice = true;
            SLAM.blockOverlayLast = !overlay.empty();
            SLAM.blockOverlayAll = !overlays.empty();
        }
        FILE* fall = nullptr;
        std::vector<int> overlayFrames;
        if (SLAM.blockOverlayAll) {
            fall = fopen(overlays.c_str(), "wb");
            if (!fall) { perror(overlays.c_str()); return 1; }
        }
        auto num = [&](double v) { if (std::isnan(v)) fprintf(fd, " nan"); else fprintf(fd, " %a", v); };
        auto displayLine = [&](int fr, int id, const double* xyz, const double* cov, const double* axis, const double* sigma) {
            fprintf(fd, "%d %d", fr, id);
            for (int e = 0; e < 3; e++) num(xyz[e]);
            for (int e = 0; e < 9; e++) num(cov[e]);
            for (int e = 0; e < 4; e++) num(axis[e]);
            for (int e = 0; e < 3; e++) num(sigma[e]);
            fprintf(fd, "\n");
        };
        auto displayFromMap = [&](int fr) {
            if (!fd) return;
            for (const monoslam::PointsMap* m = SLAM.map; m; m = m->next) {
                const double xyz[3] = { m->xyz.x, m->xyz.y, m->xyz.z }, axis[4] = { m->axis.r, m->axis.x, m->axis.y, m->axis.z }, sigma[3] = { m->sigma.x, m->sigma.y, m->sigma.z };
                displayLine(fr, m->ID, xyz, m->cov, axis, sigma);
            }
        };
        bool overlayDrawn = false;
        auto report = [&](int fr, int nBefore) {
            printf("policy frame %d deleted %d", fr, SLAM.m_nDeletes); for (int id : SLAM.m_deleteID) printf(" %d", id);
            printf(" added %d\n", SLAM.m_nMapFeatures - (nBefore - SLAM.m_nDeletes));
            printf("frame %d n_map %d matches %d\n", fr, SLAM.m_nMapFeatures, SLAM.m_nMatches);
            printf("ids"); for (const monoslam::PointsMap* m = SLAM.map; m; m = m->next) printf(" %d", m->ID); printf("\n");
            const int n = SLAM.m_X_k.rows;
            printf("path %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", fr, SLAM.m_X_k.at(n - 4, 0), SLAM.m_X_k.at(n - 3, 0), SLAM.m_X_k.at(n - 2, 0), SLAM.m_X_k.at(n - 1, 0),
                   SLAM.m_P_k.at(n - 4, n - 4), SLAM.m_P_k.at(n - 4, n - 3), SLAM.m_P_k.at(n - 3, n - 4), SLAM.m_P_k.at(n - 3, n - 3));
            if (ransac) printf("ransac low %d high %d\n", SLAM.m_nLowInliers, SLAM.m_nHighInliers);
        };
        double wall = 0.0;
        for (int fr = 0; fr < steps;) {
            const int want = steps - fr < block ? steps - fr : block, nBefore = SLAM.m_nMapFeatures;
            SLAM.dataAssociation = nullptr;
            const unsigned char* blk = frames.data() + (size_t)fr * fb;
            const int used = block <= 1 ? 0 : colour == 2 ? SLAM.SLAMBlockColour(blk, want) : colour ? SLAM.SLAMBlockColour(asColour(blk, want), want) : SLAM.SLAMBlock(blk, want);
            if (!SLAM.lastError.empty()) { fprintf(stderr, "block at frame %d: %s\n", fr, SLAM.lastError.c_str()); return 1; }
            if (used > 0) {
                nBlocks++; if (used < want) nEarly++; if (used == block) nFull++;
                wall += SLAM.m_frameTime * used;
                for (int q = 0; q < used - 1; q++) {                                                             // (frames inside a block change nothing: the verdict said so)
                    const double* t = &SLAM.m_blockPath[8 * (size_t)q];
                    printf("policy frame %d deleted 0 added 0\n", fr + q);
                    printf("path %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", fr + q, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
                    if (ransac) printf("ransac low %d high 0\n", SLAM.m_blockLowInliers[q]);
                    if (fd) {
                        const auto& d = SLAM.m_blockDisplay[(size_t)q];
                        for (size_t k = 0; k < SLAM.m_blockDisplayIDs.size(); k++) displayLine(fr + q, SLAM.m_blockDisplayIDs[k], &d.xyz[3 * k], &d.cov[9 * k], &d.axis[4 * k], &d.sigma[3 * k]);
                    }
                }
                report(fr + used - 1, nBefore);
                displayFromMap(fr + used - 1);
                overlayDrawn = SLAM.blockOverlayLast;
                if (fall && fwrite(SLAM.m_blockOverlays.data(), 1, SLAM.m_blockOverlays.size(), fall) != SLAM.m_blockOverlays.size()) { perror(overlays.c_str()); return 1; }
                if (fall) for (int q = 0; q < used; q++) overlayFrames.push_back(fr + q);
                fr += used;
                continue;
            }
            if (block > 1) nFallback++;
            showFrame(frames.data() + (size_t)fr * fb);
            SLAM.dataAssociation = assoc;
            SLAM.SLAM();
            if (!SLAM.lastError.empty()) { fprintf(stderr, "frame %d: %s\n", fr, SLAM.lastError.c_str()); return 1; }
            wall += SLAM.m_frameTime;
            report(fr, nBefore);
            displayFromMap(fr);
            fr++;
        }
        if (fd) fclose(fd);
        if (fall) fclose(fall);
        if (fd && !overlay.empty()) {
            if (!overlayDrawn) { fprintf(stderr, "overlay: no block consumed a frame\n"); return 1; }
            FILE* fo = fopen(overlay.c_str(), "wb");
            if (!fo || fwrite(SLAM.m_srcImage.data(), 1, SLAM.m_srcImage.size(), fo) != SLAM.m_srcImage.size()) { perror(overlay.c_str()); return 1; }
            fclose(fo);
        }
        printf("blocks %d early %d full %d fallback %d", nBlocks, nEarly, nFull, nFallback);
        if (resume) printf(" resumed=%d", SLAM.m_nBlocksResumed);
        if (rescue) printf(" gate_skips=%d", SLAM.m_nGateSkips);
        printf("\n");
        printf("block_frames %d frames %d us_per_frame %.2f\n", block, steps, wall / steps * 1e6);
        if (SLAM.blockOverlayAll) { printf("overlay_frames"); for (int q : overlayFrames) printf(" %d", q); printf("\n"); }
        return 0;
    }
    for (int fr = 0; fr < steps; fr++) {
        showFrame(frames.data() + (size_t)(fr % F) * fb);
        const size_t logged = SLAM.m_detectLog.size(), searches = SLAM.m_archiveLog.size();
        const int reacquiredBefore = SLAM.m_nArchiveReacquired;
        const double addBefore = SLAM.m_detectTime;
        std::vector<monoslam::FeatureInfo> archive;
        if (loops) archive = SLAM.m_featuresAllInfo;                                // (what the restart of this frame may put back)
        SLAM.SLAM();
        if (!SLAM.lastError.empty()) { fprintf(stderr, "frame %d: %s\n", fr, SLAM.lastError.c_str()); return 1; }
        if (fr == 0) addWall = SLAM.m_detectTime - addBefore;
        for (size_t q = logged; q < SLAM.m_detectLog.size(); q++) {
            const auto& p = SLAM.m_detectLog[q];
            const auto& d = p.params;
            printf("pass image %d call %d frame %d n_map %d n_matches %d running %d mc %d q %.17g md %.17g bs %d border %.17g unf %d gate %d proj %d pose %.17g %.17g %.17g %.17g\n",
                   fr % F, p.call, p.frame, p.n_map, p.n_matches, p.running, d.max_corners, d.quality_level, d.min_dist, d.block_size, d.dist_to_border,
                   d.unfiltered, d.map_gate, d.project_archived, p.pose[0], p.pose[1], p.pose[2], p.pose[3]);
            printf("map"); for (double v : p.map_px) printf(" %.17g", v); printf("\n");
            printf("arch"); for (double v : p.archived) printf(" %.17g", v); printf("\n");
            printf("uv"); for (double v : p.uv) printf(" %.17g", v); printf("\n");
            printf("loops"); for (int v : p.loops) printf(" %d", v); printf("\n");
            if (loops && p.reinsertRan) {
                printf("reinsert call %d archive %d", p.call, (int)archive.size()); for (const auto& fi : archive) printf(" %d", fi.ID);
                printf(" ids %d", (int)p.reinserted.size()); for (int id : p.reinserted) printf(" %d", id);
                printf(" n_after %d archived_after %d", p.n_after, p.archived_after);
                printf(" x6"); for (double v : p.reinsertedX6) printf(" %.17g", v);
                printf(" sr"); for (double v : p.reinsertedSr) printf(" %.17g", v);
                printf("\n");
            }
        }
        printf("frame %d n_map %d map_size %d archived %d matches %d loops %d\n", fr, SLAM.m_nMapFeatures, (int)SLAM.mapStore.size(),
               (int)SLAM.m_featuresAllInfo.size(), SLAM.m_nMatches, SLAM.m_loopPointCounter);
        if (archiveCap > 0) {
            for (size_t q = searches; q < SLAM.m_archiveLog.size(); q++) {
                const auto& a = SLAM.m_archiveLog[q];
                printf("archive frame %d searched %d n_before %d n_after %d archived_before %d archived_after %d ids", a.frame, a.searched, a.n_before, a.n_after,
                       a.archived_before, a.archived_after);
                for (int id : a.ids) printf(" %d", id);
                printf("\n");
            }
            printf("reacquired %d\n", SLAM.m_nArchiveReacquired - reacquiredBefore);
        }
        if (unique) {
            printf("ambiguous %d", SLAM.m_nAmbiguous);
            for (int id : SLAM.m_ambiguousID) printf(" %d", id);
            printf("\n");
        }
        if (ransac) printf("ransac low %d high %d\n", SLAM.m_nLowInliers, SLAM.m_nHighInliers);
        printf("init"); for (const monoslam::PointsMap* m = SLAM.map; m; m = m->next) printf(" %.17g %.17g", m->initPixel.x, m->initPixel.y); printf("\n");
        if (loops) { printf("ids"); for (const monoslam::PointsMap* m = SLAM.map; m; m = m->next) printf(" %d %d", m->ID, m->isLoop ? 1 : 0); printf("\n"); }
        const int n = SLAM.m_X_k.rows;
        printf("pose %.17g %.17g %.17g %.17g\n", SLAM.m_X_k.at(n - 4, 0), SLAM.m_X_k.at(n - 3, 0), SLAM.m_X_k.at(n - 2, 0), SLAM.m_X_k.at(n - 1, 0));
    }
    if (!overlay.empty()) {
        if (!SLAM.display2DFeatureModel()) { fprintf(stderr, "overlay: %s\n", SLAM.lastError.c_str()); return 1; }
        FILE* fo = fopen(overlay.c_str(), "wb");
        if (!fo || fwrite(SLAM.m_srcImage.data(), 1, SLAM.m_srcImage.size(), fo) != SLAM.m_srcImage.size()) { perror(overlay.c_str()); return 1; }
        fclose(fo);
        fo = fopen((overlay + ".in").c_str(), "w");
        if (!fo) { perror((overlay + ".in").c_str()); return 1; }
        for (const monoslam::PointsMap* m = SLAM.map; m; m = m->next)
            fprintf(fo, "%a %a %a %a %a %a %a %a %d\n", m->predictLocation.x, m->predictLocation.y, m->Si[0], m->Si[1], m->Si[2], m->Si[3], m->matchLocation.x,
                    m->matchLocation.y, m->isMatching ? 1 : 0);
        fclose(fo);
    }
    if (archiveCap > 0) printf("archive_matches %d archive_rejected %d archive_reacquired %d\n", SLAM.m_nArchiveMatches, SLAM.m_nArchiveRejected, SLAM.m_nArchiveReacquired);
    if (joint) printf("joint flagged %d\n", SLAM.m_nJointFlagged);
    printf("add_features_frame1_ms %.3f  frame_time_ms %.3f\n", addWall * 1e3, SLAM.m_frameTime * 1e3);
    return 0;
}
