// cslam.cpp — CSLAM facade implementation (see cslam.hpp).  Host-side bookkeeping only; every
// numeric step is a C-ABI call into the gfx950 kernels.  No CPU fallback.
#include "cslam.hpp"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>

namespace monoslam {

static const double kPi = 3.14159265358979323846;

CSLAM::CSLAM(int device) : device_(device)
{
    initializeParameters();
}

CSLAM::~CSLAM()
{
    if (ctx_) srukf_destroy(ctx_);
    if (robotFile_) fclose(robotFile_);
}

bool CSLAM::check(int rc)
{
    if (rc == SRUKF_OK) return true;
    const char* m = srukf_last_error(ctx_);
    lastError = std::string("srukf error ") + std::to_string(rc) + ": " + (m ? m : "");
    return false;
}

// SLAM.cpp:158-353: numeric defaults; the image / video / dialog parts are the host's.
void CSLAM::initializeParameters()
{
    srukf_default_params(&m_params);
    m_X_k.create(4, 1);
    m_S_k.create(4, 4);
    m_S_k.at(0, 0) = m_params.sigma_x; m_S_k.at(1, 1) = m_params.sigma_y;        // 226-231
    m_S_k.at(2, 2) = m_params.sigma_z; m_S_k.at(3, 3) = m_params.sigma_theta;
    m_P_k.create(4, 4);
    m_odoXY.assign(2 * (CAPACITY + 1), 0.0);
    m_path.assign(2 * (CAPACITY + 1), 0.0);
    m_odoTheta.create(3, CAPACITY + 1);                                            // 235
    m_frame = FrameInfo();
    m_frame.stop = m_frame.start + CAPACITY;                                       // 244-246
    m_frame.index = m_frame.start;
    m_frame.counter = 1;
    m_odoCounter = 0; m_showCounter = 1; ID = 1;                                   // 248
    m_nMapFeatures = m_nPredicts = m_nMatches = m_nAddings = 0;
    m_nDeletes = m_nStores = 0; m_deleteID.clear(); isAdding = false;
    m_frameTime = m_totalTime = 0;
    m_blockSize = 3; m_qualityLevel = 0.1; m_nInitialRaws = 8; m_nProcessRaws = 8; m_minDist = 15.0; m_minDist2 = m_minDist * m_minDist;   // 175-181
    m_keyPoints.clear(); m_loopPointID.clear(); m_loopPointCounter = 0; m_nFilters = 0; firstDetect_ = true; runningCount_ = 0;
    mapStore.clear(); relinkMap();
    m_nArchiveMatches = m_nArchiveRejected = m_nArchiveReacquired = 0;
    m_nAmbiguous = m_nAmbiguousTotal = 0; m_ambiguousID.clear();
    archiveMirror_.clear(); archiveVerdict_.clear(); reacquire_.clear(); reacquired_.clear(); frameHeld_ = false; m_archiveLog.clear();
}

// `map` = head of the singly linked list over mapStore (state order), NULL when the map is empty (SLAM.h:69, 154)
void CSLAM::relinkMap()
{
    for (size_t k = 0; k < mapStore.size(); k++) mapStore[k].next = (k + 1 < mapStore.size()) ? &mapStore[k + 1] : nullptr;
    map = mapStore.empty() ? nullptr : mapStore.data();
}

void CSLAM::resetAllParameters()
{
    if (ctx_) { srukf_destroy(ctx_); ctx_ = nullptr; }
    if (robotFile_) { fclose(robotFile_); robotFile_ = nullptr; }
    initializeParameters();
}

bool CSLAM::setMap(int N, const double* X, const double* S, const double* px, int n_added)
{
    if (ctx_) { srukf_destroy(ctx_); ctx_ = nullptr; }
    if (!check(srukf_create(&ctx_, N, &m_params, device_, nullptr))) return false;
    if (!check(srukf_set_state(ctx_, X, S))) return false;
    const int n = 6 * N + 4;
    m_X_k.create(n, 1); m_S_k.create(n, n); m_P_k.create(n, n);
    mapStore.assign(N, PointsMap()); relinkMap();
    ID = 1;
    for (int k = 0; k < N; k++) { map[k].ID = ID++; if (px) { map[k].initPixel.x = px[2 * k]; map[k].initPixel.y = px[2 * k + 1]; } }
    m_nMapFeatures = N;
    m_nAddings = n_added;    // 0 = steady state: FLAG_4_NEEDNOT_REORDER (SLAM.cpp:2083-2090)
    if (n_added > 0 && !check(srukf_set_new_landmarks(ctx_, n_added))) return false;                           // m_nFilters, 758-766
    refreshMirrors();
    return true;
}

namespace { struct Stopwatch { double& acc; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                              explicit Stopwatch(double& a) : acc(a) {} ~Stopwatch() { acc += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } }; }

bool CSLAM::integrateFeaturesInformation(int K, const double* kp)
{
    if (K <= 0) { m_nAddings = 0; return true; }                                                                // SLAM.cpp:820-821
    Stopwatch sw(m_addTime); m_nAddCalls++;
    if (!ctx_) {                                                                                                // frame 1: robot block only (221-231)
        if (!check(srukf_create(&ctx_, 0, &m_params, device_, nullptr))) return false;
        m_nMapFeatures = 0; mapStore.clear(); relinkMap();
    }
    if (!check(srukf_add_landmarks(ctx_, K, kp))) return false;
    const int N = m_nMapFeatures + K, n = 6 * N + 4;
    m_X_k.create(n, 1); m_S_k.create(n, n); m_P_k.create(n, n);
    for (int k = 0; k < K; k++) { PointsMap pm; pm.ID = ID++; pm.initPixel.x = kp[2 * k]; pm.initPixel.y = kp[2 * k + 1]; mapStore.push_back(pm); }
    relinkMap();
    m_nMapFeatures = N;                                                                                         // 766
    m_nAddings = K;                                                                                             // 758-765 (m_nFilters = m_nAddings = counter)
    refreshMirrors();
    return true;
}

bool CSLAM::deleteOneFeature(int id)
{
    if (!ctx_ || id < 0 || id >= m_nMapFeatures) { lastError = "deleteOneFeature: no such landmark"; return false; }
    Stopwatch sw(m_deleteTime); m_nDeleteCalls++;
    mirrorsFresh_ = false;
    if (!check(srukf_delete_landmark(ctx_, id))) return false;                                                  // 2643-2668
    mapStore.erase(mapStore.begin() + id); relinkMap();                                                                                // 2670-2705
    m_nMapFeatures--;                                                                                           // 2664
    if (m_nAddings > 0 && id >= m_nMapFeatures + 1 - m_nAddings) m_nAddings--;                                  // 2468-2492
    const int n = 6 * m_nMapFeatures + 4;
    m_X_k.create(n, 1); m_S_k.create(n, n); m_P_k.create(n, n);
    refreshMirrors();
    return true;
}

// Ours, beside deleteOneFeature: the landmarks at the positions `ids` (distinct, state order of the map as it is) leave the filter and the map in ONE device call
// (srukf_delete_landmarks), one compaction of mapStore and one refresh of the mirrors.  stored (may be NULL): ids.size() entries; entry q gets
// what recordFeature gives for landmark ids[q] on the state before the call (sr, initPatch, initRotation, initTrans, hasInitPatch, hasRecord)
bool CSLAM::deleteFeatures(const std::vector<int>& ids, std::vector<FeatureInfo>* stored)
{
    const int K = (int)ids.size(), N = m_nMapFeatures;
    if (!ctx_ || K < 1) { lastError = "deleteFeatures: no landmarks named"; return false; }
    if (stored && (int)stored->size() != K) { lastError = "deleteFeatures: one FeatureInfo per landmark"; return false; }
    std::vector<char> gone(N, 0);
    for (int id : ids) {
        if (id < 0 || id >= N || gone[id]) { lastError = "deleteFeatures: no such landmark, or one named twice"; return false; }
        gone[id] = 1;
    }
    Stopwatch sw(m_deleteTime); m_nDeleteCalls++;
    mirrorsFresh_ = false;
    if (stored) {
        std::vector<double> sr(36 * (size_t)K), R(9 * (size_t)K), t(3 * (size_t)K); std::vector<unsigned char> patch(441 * (size_t)K); std::vector<int> has(K);
        if (!check(srukf_delete_landmarks(ctx_, K, ids.data(), nullptr, sr.data(), patch.data(), R.data(), t.data(), nullptr, has.data()))) return false;
        for (int q = 0; q < K; q++) {
            FeatureInfo& fi = (*stored)[q];
            memcpy(fi.sr, &sr[36 * (size_t)q], sizeof fi.sr); memcpy(fi.initPatch, &patch[441 * (size_t)q], 441);
            memcpy(fi.initRotation, &R[9 * (size_t)q], sizeof fi.initRotation); memcpy(fi.initTrans, &t[3 * (size_t)q], sizeof fi.initTrans);
            fi.hasInitPatch = has[q] != 0; fi.hasRecord = true;
        }
    } else if (!check(srukf_delete_landmarks(ctx_, K, ids.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))) return false;
    size_t a = 0;
    const int armed = m_nAddings;
    for (int k = 0; k < N; k++) {
        if (!gone[k]) { if (a != (size_t)k) mapStore[a] = mapStore[k]; a++; }
        else if (armed > 0 && k >= N - armed) m_nAddings--;                                                     // 2468-2492, once per armed landmark that leaves
    }
    mapStore.resize(a); relinkMap();
    m_nMapFeatures = N - K;
    const int n = 6 * m_nMapFeatures + 4;
    m_X_k.create(n, 1); m_S_k.create(n, n); m_P_k.create(n, n);
    refreshMirrors();
    return true;
}

// ---- data association on the device ------------------------------------------------------------------------------
bool CSLAM::setFeatureAppearance(int id, const unsigned char* patch, const double R[9], const double t[3], const double px[2])
{
    if (!ctx_ || id < 0 || id >= m_nMapFeatures) { lastError = "setFeatureAppearance: no such landmark"; return false; }
    map[id].initPixel.x = px[0]; map[id].initPixel.y = px[1];
    return check(srukf_set_landmark_appearance(ctx_, id, patch, R, t, px));
}

bool CSLAM::dataAssociationOnDevice(const unsigned char* gray)
{
    const int N = m_nMapFeatures;
    clearAmbiguity();
    if (!ctx_ || N == 0) return true;
    if (rejectAmbiguousMatches || subpixelMatches) { if (!associateChecked(gray)) return false; frameHeld_ = true; return true; }
    std::vector<double> z(2 * (size_t)N); std::vector<int> m(N);
    if (!check(srukf_associate(ctx_, gray, z.data(), m.data(), nullptr))) return false;
    frameHeld_ = true;
    m_nMatches = 0;
    for (int k = 0; k < N; k++) {                                                                               // 1989-2000
        map[k].isMatching = m[k] != 0;
        if (m[k]) { map[k].matchLocation.x = z[2 * k]; map[k].matchLocation.y = z[2 * k + 1]; m_nMatches++; }
    }
    return true;
}

// dataAssociationOnDevice's bookkeeping (1989-2000) on the frame the handle holds (loadPictures ran before): no upload
bool CSLAM::dataAssociationOnDeviceHeld()
{
    const int N = m_nMapFeatures;
    clearAmbiguity();
    if (!ctx_ || N == 0) return true;
    if (rejectAmbiguousMatches || subpixelMatches) return associateChecked(nullptr);
    std::vector<double> z(2 * (size_t)N); std::vector<int> m(N);
    if (!check(srukf_associate_held(ctx_, z.data(), m.data(), nullptr))) return false;
    m_nMatches = 0;
    for (int k = 0; k < N; k++) {
        map[k].isMatching = m[k] != 0;
        if (m[k]) { map[k].matchLocation.x = z[2 * k]; map[k].matchLocation.y = z[2 * k + 1]; m_nMatches++; }
    }
    return true;
}

// dataAssociationOnDevice / dataAssociationOnDeviceHeld with rejectAmbiguousMatches or subpixelMatches on (srukf_associate_checked; gray == NULL: the
// held frame).  A vetoed landmark is simply not matched this frame; with only subpixelMatches on the ratio is 2.0, which never vetoes
// every association through the facade starts from "nothing vetoed": a frame run with the switches off leaves no flag of an earlier frame behind
void CSLAM::clearAmbiguity()
{
    m_nAmbiguous = 0; m_ambiguousID.clear();
    for (PointsMap& pm : mapStore) pm.isAmbiguous = false;
}

bool CSLAM::associateChecked(const unsigned char* gray)
{
    const int N = m_nMapFeatures;
    srukf_match_params mp = { 0.8, rejectAmbiguousMatches ? AMBIGUITY_RATIO : 2.0, AMBIGUITY_EXCLUSION, subpixelMatches ? 1 : 0 };
    std::vector<double> z(2 * (size_t)N), corr(N), corr2(N), z2(2 * (size_t)N); std::vector<int> m(N), fl(N);
    if (!check(srukf_associate_checked(ctx_, gray, &mp, z.data(), m.data(), corr.data(), corr2.data(), z2.data(), fl.data()))) return false;
    m_nMatches = 0;
    for (int k = 0; k < N; k++) {                                                                               // 1989-2000
        map[k].isMatching = m[k] != 0;
        map[k].isAmbiguous = (fl[k] & 2) != 0;
        map[k].corr = corr[k]; map[k].corr2 = corr2[k];
        map[k].rivalLocation.x = z2[2 * k]; map[k].rivalLocation.y = z2[2 * k + 1];
        if (m[k]) { map[k].matchLocation.x = z[2 * k]; map[k].matchLocation.y = z[2 * k + 1]; m_nMatches++; }
        if (map[k].isAmbiguous) { m_nAmbiguous++; m_ambiguousID.push_back(map[k].ID); }
    }
    m_nAmbiguousTotal += m_nAmbiguous;
    return true;
}

// ---- colour-frame intake and the 2-D feature overlay ----------------------------------------------------------------------------------------
// loadPictures (529-543): the colour frame goes to the device, comes back as the gray frame the reference's cvCvtColor(CV_RGB2GRAY) makes of B, G, R data
bool CSLAM::loadPictures(const unsigned char* bgr)
{
    if (!ctx_ || !bgr) { lastError = "loadPictures: no context or no frame"; return false; }
    m_grayStore.resize((size_t)m_params.image_w * (size_t)m_params.image_h);
    if (!check(srukf_set_frame_bgr(ctx_, bgr, m_grayStore.data()))) return false;
    frameHeld_ = true;
    m_gryImage = m_grayStore.data();
    return true;
}

// display2DFeatureModel (3009-3051): m_srcImage = the held frame with every matched landmark's predicted cross, matched cross and chi-square ellipse
bool CSLAM::display2DFeatureModel()
{
    if (!ctx_) { lastError = "display2DFeatureModel: no context"; return false; }
    const int N = m_nMapFeatures;
    std::vector<double> h(2 * (size_t)N), Si(4 * (size_t)N), z(2 * (size_t)N); std::vector<int> m(N);
    for (int k = 0; k < N; k++) {                                                                               // 3024-3031
        h[2 * k] = map[k].predictLocation.x; h[2 * k + 1] = map[k].predictLocation.y;
        memcpy(&Si[4 * k], map[k].Si, sizeof map[k].Si);
        z[2 * k] = map[k].matchLocation.x; z[2 * k + 1] = map[k].matchLocation.y;
        m[k] = map[k].isMatching ? 1 : 0;
    }
    m_srcImage.resize(3 * (size_t)m_params.image_w * (size_t)m_params.image_h);
    return check(srukf_render_overlay(ctx_, h.data(), Si.data(), z.data(), m.data(), m_srcImage.data()));
}

// ---- finding new landmarks on the device ------------------------------------------------------------------------------------------------
// SLAM.cpp:574-768.  The GFTT budget (590-599), the filter switches (653, 660, 614) and the map / archive inputs go to srukf_detect_features; the
// key points it accepts become m_keyPoints, the archived features it met again m_loopPointID; counter = both (719, 748), and the running map
// count moves as 758-766 move m_nMapFeatures (the facade's m_nMapFeatures stays the true map size).
bool CSLAM::detectAndfilteringFeatures()
{
    if (!ctx_ || !m_gryImage) { lastError = "detectAndfilteringFeatures: no context or no m_gryImage"; return false; }
    srukf_detect_params dp;
    dp.max_corners = (1 == m_frame.counter || isAdding) ? m_nInitialRaws : m_nProcessRaws;                     // 590-597
    dp.quality_level = m_qualityLevel; dp.min_dist = m_minDist; dp.block_size = m_blockSize; dp.dist_to_border = DIST_2_BORDER;
    dp.unfiltered = (1 == m_frame.counter || firstDetect_) ? 1 : 0;                                             // 653
    dp.map_gate = (0 != m_nMatches) ? 1 : 0;                                                                    // 660
    dp.project_archived = isAdding ? 1 : 0;                                                                     // 614-635
    std::vector<double> mp, ar;
    for (const PointsMap* map_p = map; NULL != map_p; map_p = map_p->next) {
        const double e[4] = { map_p->matchLocation.x, map_p->matchLocation.y, map_p->predictLocation.x, map_p->predictLocation.y };
        mp.insert(mp.end(), e, e + 4);
    }
    for (const FeatureInfo& fi : m_featuresAllInfo) ar.insert(ar.end(), fi.state, fi.state + 6);
    const int cap = std::max(dp.max_corners, 1);
    const int nA = (int)m_featuresAllInfo.size(), loopCap = std::max(1, cap * nA);
    std::vector<double> uv(2 * (size_t)cap);
    std::vector<int> loops(2 * (size_t)loopCap);
    int nUv = 0, nLoop = 0;
    if (!check(srukf_detect_features(ctx_, m_gryImage, &dp, (int)(mp.size() / 4), mp.data(), nA, ar.data(), uv.data(), cap, &nUv,
                                     loops.data(), loopCap, &nLoop))) return false;
    firstDetect_ = false;                                                                                       // 754
    nUv = std::min(nUv, cap); nLoop = std::min(nLoop, loopCap);
    m_keyPoints.clear();
    for (int k = 0; k < nUv; k++) { Point2d p; p.x = uv[2 * k]; p.y = uv[2 * k + 1]; m_keyPoints.push_back(p); }
    if (isAdding) m_loopPointID.clear();                                                                        // 618
    m_loopPointCounter = nLoop;                                                                                 // 604, 721
    if ((int)m_loopPointID.size() < nLoop) m_loopPointID.resize(nLoop);
    for (int q = 0; q < nLoop; q++) m_loopPointID[q] = m_featuresAllInfo[loops[2 * q + 1]].ID;                 // 719
    loopArchive_.clear();
    for (int q = 0; q < nLoop; q++) loopArchive_.push_back(loops[2 * q + 1]);
    const int counter = nUv + nLoop;
    m_nFilters = counter;                                                                                       // 756-766
    runningCount_ = isAdding ? counter : runningCount_ + counter;
    if (logDetectPasses) {
        DetectPass dpass; dpass.call = addCalls_; dpass.frame = m_frame.counter; dpass.n_map = m_nMapFeatures; dpass.n_matches = m_nMatches;
        dpass.params = dp; dpass.map_px = mp; dpass.archived = ar;
        double P4[16];
        if (!check(srukf_get_robot(ctx_, dpass.pose, P4))) return false;
        dpass.uv.assign(uv.begin(), uv.begin() + 2 * nUv); dpass.loops.assign(loops.begin(), loops.begin() + 2 * nLoop); dpass.running = runningCount_;
        m_detectLog.push_back(dpass);
    }
    return true;
}

// SLAM.cpp:777-808
bool CSLAM::insureEnoughFeatures()
{
    const int numberStore = m_nInitialRaws;
    const double qualityLevelStore = m_qualityLevel;
    bool ok = true;
    while (runningCount_ < m_minNUM) {
        m_nInitialRaws += m_minNUM;
        if (m_nInitialRaws > 30) break;
        m_keyPoints.clear();
        if (!(ok = detectAndfilteringFeatures())) break;
    }
    m_nInitialRaws = numberStore;
    m_qualityLevel = qualityLevelStore;
    return ok;
}

// addFeatures (552-562) on the device: detect, then integrate the accepted key points and capture their appearance from the frame the
// detection left on the device (it survives the map change)
bool CSLAM::addFeaturesOnDevice()
{
    Stopwatch swd(m_detectTime); m_nDetectCalls++;
    m_nAddings = 0;
    addCalls_++;
    if (!ctx_) {                                                                                                // frame 1: robot block only (221-231)
        if (!check(srukf_create(&ctx_, 0, &m_params, device_, nullptr))) return false;
        m_nMapFeatures = 0; mapStore.clear(); relinkMap();
    }
    runningCount_ = m_nMapFeatures;
    m_keyPoints.clear();
    if (!detectAndfilteringFeatures() || !insureEnoughFeatures()) return false;
    const bool reinsert = isAdding && reinsertLoopPoints;
    if (reinsert && !reinsertLoops()) return false;                                                             // 948-1015: in front of the key points
    const int K = (int)m_keyPoints.size(), first = m_nMapFeatures;
    if (K > 0) {
        std::vector<double> kp(2 * (size_t)K);
        for (int k = 0; k < K; k++) { kp[2 * k] = m_keyPoints[k].x; kp[2 * k + 1] = m_keyPoints[k].y; }
        if (!integrateFeaturesInformation(K, kp.data())) return false;
        if (!check(srukf_capture_appearance(ctx_, first, K, kp.data(), nullptr))) return false;                 // 918-926
    }
    if (reinsert && logDetectPasses && !m_detectLog.empty()) { m_detectLog.back().n_after = m_nMapFeatures; m_detectLog.back().archived_after = (int)m_featuresAllInfo.size(); }
    return true;
}

// What an archived landmark takes along for re-insertion (the reference's FeatureInfo::sr / initPatch / initRotation / initTrans, read back at 961-973):
// landmark k of the current state, one device round trip.  fi.state keeps the rows the archive site copied from m_X_k (the same values).
bool CSLAM::recordFeature(FeatureInfo& fi, int k)
{
    double X6[6], px[2]; int has = 0;
    if (!check(srukf_get_landmark_record(ctx_, k, X6, fi.sr, fi.initPatch, fi.initRotation, fi.initTrans, px, &has))) return false;
    fi.hasInitPatch = has != 0;
    fi.hasRecord = true;
    return true;
}

// The isLoop branch of integrateFeaturesInformation (SLAM.cpp:948-1015) with the semantics of DESIGN.md §12: the archived entries the last detection pass
// reported as loop points, each once, in the order first reported, go back into the filter with their archived state and sr (srukf_insert_landmarks) and
// their appearance record, behind the map and in front of the key points integrated next.  Entries without a record stay archived (they are still reported).
// The new nodes keep their archived ID (ID is not advanced) with isLoop = true; their archive entries are erased.
bool CSLAM::reinsertLoops()
{
    std::vector<int> take, seen;
    for (int a : loopArchive_) {
        if (a < 0 || a >= (int)m_featuresAllInfo.size() || !m_featuresAllInfo[a].hasRecord || std::find(seen.begin(), seen.end(), a) != seen.end()) continue;
        seen.push_back(a);
        // searchArchivedLandmarks: the geometric test alone does not put a landmark back; the search of this frame has to have matched it (the matched entries
        // went back when it ran, so what a pass still meets here was refused)
        if (searchArchivedLandmarks && std::find(archiveVerdict_.begin(), archiveVerdict_.end(), m_featuresAllInfo[a].ID) == archiveVerdict_.end()) { m_nArchiveRejected++; continue; }
        take.push_back(a);
    }
    std::vector<int> ids;
    std::vector<double> x6s, srs;
    if (!reinsertEntries(take, ids, x6s, srs)) return false;
    if (logDetectPasses && !m_detectLog.empty()) {
        DetectPass& d = m_detectLog.back();
        d.reinsertRan = true; d.reinserted = ids; d.reinsertedX6 = x6s; d.reinsertedSr = srs;
    }
    return true;
}

// the archive entries `take` (indices, each once) go behind the map as isLoop nodes with their archived state, sr and appearance record; their entries are erased
bool CSLAM::reinsertEntries(const std::vector<int>& take, std::vector<int>& ids, std::vector<double>& x6s, std::vector<double>& srs)
{
    if (!take.empty()) {
        mirrorsFresh_ = false;
        if (!check(srukf_set_new_landmarks(ctx_, 0))) return false;             // m_nAddings = 0 here: the loop points go behind the whole map
        // one srukf_insert_landmarks per run of entries with / without an appearance record (a call gives records to all of its landmarks or to none)
        for (size_t q = 0; q < take.size();) {
            const bool app = m_featuresAllInfo[take[q]].hasInitPatch;
            size_t e = q;
            while (e < take.size() && m_featuresAllInfo[take[e]].hasInitPatch == app) e++;
            const int L = (int)(e - q);
            std::vector<double> X6(6 * (size_t)L), S66(36 * (size_t)L), R(9 * (size_t)L), t(3 * (size_t)L), px(2 * (size_t)L);
            std::vector<unsigned char> patches(app ? 441 * (size_t)L : 0);
            for (int j = 0; j < L; j++) {
                const FeatureInfo& fi = m_featuresAllInfo[take[q + j]];
                memcpy(&X6[6 * j], fi.state, sizeof fi.state); memcpy(&S66[36 * j], fi.sr, sizeof fi.sr);
                memcpy(&R[9 * j], fi.initRotation, sizeof fi.initRotation); memcpy(&t[3 * j], fi.initTrans, sizeof fi.initTrans);
                px[2 * j] = fi.initPixel.x; px[2 * j + 1] = fi.initPixel.y;
                if (app) memcpy(&patches[441 * (size_t)j], fi.initPatch, 441);
            }
            if (!check(srukf_insert_landmarks(ctx_, L, X6.data(), S66.data(), app ? patches.data() : nullptr, app ? R.data() : nullptr,
                                              app ? t.data() : nullptr, app ? px.data() : nullptr))) return false;
            q = e;
        }
        for (int a : take) {
            const FeatureInfo& fi = m_featuresAllInfo[a];
            PointsMap pm; pm.ID = fi.ID; pm.isLoop = true; pm.xyz = fi.initXYZ; pm.initPixel = fi.initPixel;
            mapStore.push_back(pm); ids.push_back(fi.ID);
            x6s.insert(x6s.end(), fi.state, fi.state + 6); srs.insert(srs.end(), fi.sr, fi.sr + 36);
        }
        relinkMap();
        m_nMapFeatures += (int)take.size();
        std::vector<int> gone = take;
        std::sort(gone.rbegin(), gone.rend());
        for (int a : gone) m_featuresAllInfo.erase(m_featuresAllInfo.begin() + a);
        const int n = 6 * m_nMapFeatures + 4;
        m_X_k.create(n, 1); m_S_k.create(n, n); m_P_k.create(n, n);
        refreshMirrors();
    }
    return true;
}

// ---- display accessors -----------------------------------------------------------------------------------------
bool CSLAM::refreshFeaturesDisplay(bool withMirrors)
{
    const int N = m_nMapFeatures;
    if (!ctx_ || N == 0) return true;
    std::vector<double> xyz(3 * (size_t)N), cov(9 * (size_t)N), axis, sigma;
    const bool dev = ellipsoidsOnDevice;
    if (dev) { axis.resize(4 * (size_t)N); sigma.resize(3 * (size_t)N); }
    if (withMirrors && !fullCovariance) {
        double pose[4], P4[16];
        if (!check(dev ? srukf_get_frame_view_display(ctx_, m_X_k.data.data(), xyz.data(), cov.data(), axis.data(), sigma.data(), pose, P4)
                       : srukf_get_frame_view(ctx_, m_X_k.data.data(), xyz.data(), cov.data(), pose, P4))) return false;
        const int n = m_X_k.rows;
        for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) m_P_k.at(n - 4 + a, n - 4 + b) = P4[4 * a + b];
        mirrorsFresh_ = true;
    } else {
        if (withMirrors && !check(srukf_get_state(ctx_, m_X_k.data.data(), nullptr))) return false;
        if (!check(dev ? srukf_get_landmarks_display(ctx_, xyz.data(), cov.data(), axis.data(), sigma.data(), nullptr)
                       : srukf_get_landmarks_cartesian(ctx_, xyz.data(), cov.data()))) return false;
    }
    Mat c; c.create(3, 3);
    for (int k = 0; k < N; k++) {
        map[k].xyz.x = xyz[3 * k]; map[k].xyz.y = xyz[3 * k + 1]; map[k].xyz.z = xyz[3 * k + 2];
        for (int e = 0; e < 9; e++) { map[k].cov[e] = cov[9 * (size_t)k + e]; c.data[e] = map[k].cov[e]; }
        if (dev) {                                                                                             // k_lm_ellipsoid: the same arithmetic on the device
            const double* q = &axis[4 * (size_t)k]; const double* sg = &sigma[3 * (size_t)k];
            map[k].axis.r = q[0]; map[k].axis.x = q[1]; map[k].axis.y = q[2]; map[k].axis.z = q[3];
            map[k].sigma.x = sg[0]; map[k].sigma.y = sg[1]; map[k].sigma.z = sg[2];
        } else get3DdisplayInformation(map[k].axis, map[k].sigma, c);                                          // 2575
    }
    return true;
}

// SLAM.cpp:2397-2621.  m_P_k = S^T S (2404) is what refreshMirrors / the device accessors stand for.
// deleteTogether: the same walk with no device call in it (pass 1: the tests read only X, which a deletion gathers, and the nodes' counters, so the frame's
// deletion set is known before the first landmark leaves; positions are collected in the indexing the frame began with), then ONE deleteFeatures call for
// all of them (pass 2), whose records fill the entries recordFeature fills in the walk otherwise.  Same deleted IDs, counters and map IDs afterwards
bool CSLAM::updateFeaturesInformation()
{
    if (!m_nMapFeatures || !ctx_) return true;                                                                  // 2399-2402
    // m_X_k, xyz / cov / axis / sigma from the posterior (2566-2567; also what an archived landmark takes along, 2528-2529) and the robot block the
    // mirrors show (2404): one device round trip (srukf_get_frame_view)
    if (!refreshFeaturesDisplay(true)) return false;
    const double imageWidth = m_params.image_w, imageHeight = m_params.image_h;
    m_nDeletes = 0; m_nStores = 0; m_deleteID.clear();                                                           // 2419-2422
    const bool together = deleteTogether;
    std::vector<int> leave; std::vector<FeatureInfo> infos; std::vector<char> store;                            // pass 1's collection (together)
    int id = 0, gone = 0;                                                                                       // id: position in the state as it is; id + gone: as the frame began
    int nLeft = m_nMapFeatures;                                                                                 // landmarks left (== m_nMapFeatures when every deletion runs at once)
    PointsMap* map_p = map;
    while (NULL != map_p) {                                                                                      // 2425
        const int dim = m_X_k.rows, at = together ? id + gone : id;                                              // (together: m_X_k is still the frame's)
        const double zi = m_X_k.at(6 * at + 2, 0), theta = m_X_k.at(6 * at + 3, 0), phi = m_X_k.at(6 * at + 4, 0), rho = m_X_k.at(6 * at + 5, 0);
        const double Hlr_z = rho * (zi - m_X_k.at(dim - 2, 0)) + cos(phi) * cos(theta);                          // 2435
        const double px = map_p->predictLocation.x, py = map_p->predictLocation.y, dpx = imageWidth - px, dpy = imageHeight - py;
        const bool unmatched = map_p->nPredictTimes > 2 * map_p->nMatchTimes && map_p->nPredictTimes >= 10;
        const bool predBorder = px < DIST_2_BORDER || py < DIST_2_BORDER || dpx < DIST_2_BORDER || dpy < DIST_2_BORDER;
        bool isDelete = unmatched || rho < 0.01 || Hlr_z < 0.0 || predBorder;                                    // 2443-2446
        bool matchBorder = false;
        if (map_p->isMatching) {                                                                                 // 2448-2459
            const double mx = map_p->matchLocation.x, my = map_p->matchLocation.y;
            matchBorder = mx < DIST_2_BORDER || my < DIST_2_BORDER || imageWidth - mx < DIST_2_BORDER || imageHeight - my < DIST_2_BORDER;
            isDelete = isDelete || matchBorder;
        }
        if (isDelete) {
            bool isNeedStore = false;
            if (unmatched || rho < 0.01 || Hlr_z < 0.0) m_nPredicts--;                                           // 2465-2488
            else if (predBorder) { m_nPredicts--; if (map_p->isMatching) { isNeedStore = true; m_nStores++; m_nMatches--; } }      // 2489-2502
            else if (matchBorder) { isNeedStore = true; m_nStores++; m_nPredicts--; m_nMatches--; }              // 2503-2512
            m_deleteID.push_back(map_p->ID);                                                                     // 2514
            FeatureInfo fi;
            if (isNeedStore) {                                                                                   // 2516-2532
                fi.ID = map_p->ID; fi.isLoop = map_p->isLoop; fi.nPredictTimes = map_p->nPredictTimes; fi.nMatchTimes = map_p->nMatchTimes;
                fi.initXYZ = map_p->xyz; fi.initPixel = map_p->initPixel;
                for (int e = 0; e < 6; e++) fi.state[e] = m_X_k.at(6 * at + e, 0);
                fi.position = map_p->xyz; memcpy(fi.cov, map_p->cov, sizeof fi.cov); fi.axis = map_p->axis; fi.sigma = map_p->sigma;
                if (!together) {
                    if (reinsertLoopPoints && !recordFeature(fi, id)) return false;                               // before the landmark leaves
                    m_featuresAllInfo.push_back(fi);
                }
            }
            if (together) {                                                                                      // pass 1: the landmark leaves with the others, below
                leave.push_back(at); infos.push_back(fi); store.push_back(isNeedStore ? 1 : 0);
                gone++; nLeft--;
                map_p = map_p->next;                                                                             // the node that would now be at position id
            } else {
                if (!deleteOneFeature(id)) return false;                                                         // 2554 (m_nDeletes++, m_nMapFeatures--: 2662-2664)
                nLeft = m_nMapFeatures;
                map_p = (id < m_nMapFeatures) ? &mapStore[id] : nullptr;                                         // 2555-2570: the node now at position id
            }
            m_nDeletes++;
        } else {
            map_p->isVisible = false;                                                                            // 2598
        }
        if (id == nLeft || !map_p) break;                                                                        // 2607-2615 (a NULL node is dereferenced there)
        id++;
        map_p = map_p->next;
    }
    if (together && !leave.empty()) {                                                                            // pass 2: one device call, one compaction, one refresh
        if (!deleteFeatures(leave, reinsertLoopPoints ? &infos : nullptr)) return false;
        for (size_t q = 0; q < infos.size(); q++) if (store[q]) m_featuresAllInfo.push_back(infos[q]);
    }
    return true;
}

void CSLAM::getFeatureCartesianInformation(Point3d& xyz, Mat& sr, Mat& cov, const int& id) const
{
    xyz = map[id].xyz;
    cov.create(3, 3);
    for (int e = 0; e < 9; e++) cov.data[e] = map[id].cov[e];
    sr.create(0, 0);
    if (fullCovariance && m_S_k.rows >= 6 * id + 6) {
        sr.create(6, 6);
        for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) sr.at(a, b) = m_S_k.at(6 * id + a, 6 * id + b);
    }
}

void CSLAM::get3DdisplayInformation(Quaternion& axis, Point3d& sigma, const Mat& matrix) const
{
    static thread_local Mat values, vectors;                   // (called once per landmark and frame: the buffers are kept)
    calculateEigenvaluesAndEigenvectors(matrix, values, vectors);
    matrix2Quaternion(axis, vectors);
    sigma.x = sqrt(values.at(0, 0)); sigma.y = sqrt(values.at(1, 1)); sigma.z = sqrt(values.at(2, 2));       // 1-sigma semi-axes
}

// Classical Jacobi method for a real symmetric matrix: repeatedly annihilate the off-diagonal element of largest
// magnitude with a plane rotation A <- R^T A R, accumulating V <- V R.  On return the diagonal of `eigenvalues` holds
// the eigenvalues (in the positions the rotations left them, not sorted) and column j of `eigenvectors` is the
// eigenvector of eigenvalues(j, j).  Stops when every off-diagonal magnitude is below EPSILON (false after 30 n^2 sweeps).
bool CSLAM::calculateEigenvaluesAndEigenvectors(const Mat& src, Mat& eigenvalues, Mat& eigenvectors) const
{
    const int n = src.rows;
    eigenvalues = src;
    eigenvectors.create(n, n);
    for (int i = 0; i < n; i++) eigenvectors.at(i, i) = 1.0;
    Mat& A = eigenvalues; Mat& V = eigenvectors;
    for (int it = 0; it <= 30 * n * n; it++) {
        int p = -1, q = -1; double big = 0.0;
        for (int i = 1; i < n; i++) for (int j = 0; j < i; j++) if (fabs(A.at(i, j)) > big) { big = fabs(A.at(i, j)); p = i; q = j; }
        if (big < m_params.epsilon) return true;
        // rotation angle phi with tan(2 phi) = 2 a_pq / (a_qq - a_pp), written through omega = sin(2 phi) so that the
        // half-angle formulas need no atan
        const double x = -A.at(p, q), y = 0.5 * (A.at(q, q) - A.at(p, p));
        double omega = x / sqrt(x * x + y * y);
        if (y < 0.0) omega = -omega;
        const double sn = omega / sqrt(2.0 * (1.0 + sqrt(1.0 - omega * omega)));
        const double cn = sqrt(1.0 - sn * sn);
        const double app = A.at(p, p), aqq = A.at(q, q), apq = A.at(p, q);
        A.at(p, p) = app * cn * cn + aqq * sn * sn + apq * omega;
        A.at(q, q) = app * sn * sn + aqq * cn * cn - apq * omega;
        A.at(p, q) = 0.0; A.at(q, p) = 0.0;
        for (int j = 0; j < n; j++) if (j != p && j != q) {
            const double ap = A.at(p, j), aq = A.at(q, j);
            A.at(p, j) = ap * cn + aq * sn; A.at(q, j) = -ap * sn + aq * cn;
        }
        for (int i = 0; i < n; i++) if (i != p && i != q) {
            const double ap = A.at(i, p), aq = A.at(i, q);
            A.at(i, p) = ap * cn + aq * sn; A.at(i, q) = -ap * sn + aq * cn;
        }
        for (int i = 0; i < n; i++) {
            const double vp = V.at(i, p), vq = V.at(i, q);
            V.at(i, p) = vp * cn + vq * sn; V.at(i, q) = -vp * sn + vq * cn;
        }
    }
    return false;
}

// rotation matrix -> unit quaternion (r, x, y, z), branching on the largest of trace / diagonal entries so that the
// square root argument stays away from zero; element pairing as in the reference (SLAM.cpp:2902-2948)
void CSLAM::matrix2Quaternion(Quaternion& qn, const Mat& m) const
{
    const double m11 = m.at(0, 0), m12 = m.at(0, 1), m13 = m.at(0, 2);
    const double m21 = m.at(1, 0), m22 = m.at(1, 1), m23 = m.at(1, 2);
    const double m31 = m.at(2, 0), m32 = m.at(2, 1), m33 = m.at(2, 2);
    const double tr = m11 + m22 + m33;
    if (tr > 0.0) {
        const double t = 0.5 / sqrt(tr + 1);
        qn.r = 0.25 / t; qn.x = (m23 - m32) * t; qn.y = (m31 - m13) * t; qn.z = (m12 - m21) * t;
    } else if (m11 > m22 && m11 > m33) {
        const double t = 2.0 * sqrt(1.0 + m11 - m22 - m33);
        qn.r = (m32 - m23) / t; qn.x = 0.25 * t; qn.y = (m12 + m21) / t; qn.z = (m13 + m31) / t;
    } else if (m22 > m33) {
        const double t = 2.0 * sqrt(1.0 + m22 - m11 - m33);
        qn.r = (m13 - m31) / t; qn.x = (m12 + m21) / t; qn.y = 0.25 * t; qn.z = (m23 + m32) / t;
    } else {
        const double t = 2.0 * sqrt(1.0 + m33 - m11 - m22);
        qn.r = (m21 - m12) / t; qn.x = (m13 + m31) / t; qn.y = (m23 + m32) / t; qn.z = 0.25 * t;
    }
}

// SLAM.cpp:462-496 + 363-450: "%d : %*lf %lf %lf %lf" lines, first sample is the origin, samples
// closer than MIN_STEP in both x and y are skipped, turns above MIN_STEP_THETA flag a redirection.
bool CSLAM::loadOdometryData(const std::string& path)
{
    FILE* f = fopen(path.c_str(), "r");
    if (!f) { lastError = "cannot open " + path; return false; }
    char line[500];
    m_odoCounter = 0;
    auto one = [&](int counter) -> bool {
        if (!fgets(line, sizeof line, f)) return false;
        int id = 0; double x = 0, y = 0, th = 0;
        if (sscanf(line, "%d : %*lf %lf %lf %lf", &id, &x, &y, &th) < 4) return false;
        m_odoTheta.at(0, counter) = id; m_odoTheta.at(1, counter) = th;
        if (counter == 0) {
            initOdo_[0] = x; initOdo_[1] = y;
            initPos_[0] = m_X_k.rows >= 4 ? m_X_k.at(m_X_k.rows - 4, 0) : 0; initPos_[1] = m_X_k.rows >= 4 ? m_X_k.at(m_X_k.rows - 3, 0) : 0;
            m_odoXY[0] = initPos_[0]; m_odoXY[1] = initPos_[1];
        } else {
            m_odoXY[2 * counter] = initPos_[0] + (x - initOdo_[0]);
            m_odoXY[2 * counter + 1] = initPos_[1] + (y - initOdo_[1]);
        }
        return true;
    };
    for (int skip = 1; skip < m_frame.start; skip++) if (!one(0)) break;                                       // 372-395: the origin is line m_frame.start
    if (!one(0)) { fclose(f); lastError = "empty odometry file"; return false; }
    m_odoCounter = 1;
    // 397: the robot heading starts at the first sample's heading
    if (m_X_k.rows >= 4) {
        m_X_k.at(m_X_k.rows - 1, 0) = m_odoTheta.at(1, 0);
        if (ctx_) {
            const int dim = m_X_k.rows;
            std::vector<double> X(dim), S((size_t)dim * dim);
            if (!check(srukf_get_state(ctx_, X.data(), S.data()))) { fclose(f); return false; }
            X[dim - 1] = m_odoTheta.at(1, 0);
            if (!check(srukf_set_state(ctx_, X.data(), S.data()))) { fclose(f); return false; }
            if (m_nAddings > 0 && !check(srukf_set_new_landmarks(ctx_, m_nAddings))) { fclose(f); return false; }
        }
    }
    m_odoTheta.at(2, 0) = 0;
    for (int i = 0; i < m_frame.stop - m_frame.start && m_odoCounter <= CAPACITY; i++) {                       // 400
        if (!one(m_odoCounter)) break;
        bool ok = true;
        while (std::fabs(m_odoXY[2 * m_odoCounter] - m_odoXY[2 * m_odoCounter - 2]) < MIN_STEP_X &&
               std::fabs(m_odoXY[2 * m_odoCounter + 1] - m_odoXY[2 * m_odoCounter - 1]) < MIN_STEP_Y) {          // 419-432
            if (!one(m_odoCounter)) { ok = false; break; }
        }
        if (!ok) break;
        double d = m_odoTheta.at(1, m_odoCounter) - m_odoTheta.at(1, m_odoCounter - 1);
        if (d > kPi) d -= 2 * kPi; else if (d < -kPi) d += 2 * kPi;                                              // wrapAngle 507-519
        m_odoTheta.at(2, m_odoCounter) = (std::fabs(d) > MIN_STEP_THETA * kPi / 180) ? 1 : 0;                    // 438-445
        m_odoCounter++;
    }
    fclose(f);
    return true;
}

// The redirection branch of predictMotion (SLAM.cpp:1354-1428): the odometry heading jumped by more than MIN_STEP_THETA
// (flag in m_odoTheta row 2, loadOdometryData 438-445).  The current map is archived landmark by landmark in
// m_featuresAllInfo (1357-1378), a fresh 4-state filter starts at the current x / y with the odometry heading and the
// initial robot sqrt covariance (1396-1406), the host's key points are joint-initialised (addFeatures, 1414-1416), and
// the frame counter moves on to the next odometry sample whose heading replaces the robot heading (1420-1427).
bool CSLAM::redirection()
{
    const int c = m_frame.counter, n = m_X_k.rows;
    if (m_nMapFeatures > 0 && !refreshFeaturesDisplay()) return false;                                         // xyz / cov / axis / sigma of every landmark
    if (!check(srukf_get_state(ctx_, m_X_k.data.data(), nullptr))) return false;
    int id = 0;
    for (const PointsMap* map_p = map; NULL != map_p; map_p = map_p->next, id++) {                             // 1357-1378
        FeatureInfo fi;
        fi.ID = map_p->ID; fi.isLoop = map_p->isLoop; fi.nPredictTimes = map_p->nPredictTimes; fi.nMatchTimes = map_p->nMatchTimes;
        fi.initXYZ = map_p->xyz; fi.initPixel = map_p->initPixel;
        for (int e = 0; e < 6; e++) fi.state[e] = m_X_k.at(6 * id + e, 0);
        fi.position = map_p->xyz;
        memcpy(fi.cov, map_p->cov, sizeof fi.cov);
        fi.axis = map_p->axis; fi.sigma = map_p->sigma;
        if (reinsertLoopPoints && !recordFeature(fi, id)) return false;                                           // before srukf_destroy
        m_featuresAllInfo.push_back(fi);
    }
    const double X4[4] = { m_X_k.at(n - 4, 0), m_X_k.at(n - 3, 0), 0.0, m_odoTheta.at(1, c) };                 // 1396-1400
    const double S4[16] = { m_params.sigma_x, 0, 0, 0,  0, m_params.sigma_y, 0, 0,  0, 0, m_params.sigma_z, 0,  0, 0, 0, m_params.sigma_theta };   // 1402-1406
    srukf_destroy(ctx_); ctx_ = nullptr;
    if (!check(srukf_create(&ctx_, 0, &m_params, device_, nullptr))) return false;
    if (!check(srukf_set_state(ctx_, X4, S4))) return false;
    m_nStoreMap = m_nMapFeatures; m_nStorePredicts = m_nPredicts; m_nStoreMatches = m_nMatches;                // 1408-1410
    m_nMapFeatures = 0; m_nPredicts = 0; m_nMatches = 0; m_nAddings = 0;                                       // 1412-1416
    mapStore.clear(); relinkMap();
    m_X_k.create(4, 1); m_S_k.create(4, 4); m_P_k.create(4, 4);
    std::vector<double> keyPoints;
    if (!addFeatures && m_gryImage) {                                                                          // 1418-1420 on the device: isAdding semantics
        isAdding = true;
        frameHeld_ = false;                                                                                    // (a new handle holds nothing)
        const bool ok = (!searchArchivedLandmarks || searchArchive()) && addFeaturesOnDevice();
        isAdding = false;
        if (!ok) return false;
    } else {
        const int K = addFeatures ? addFeatures(*this, keyPoints) : 0;                                         // 1418-1420 (isAdding; addFeatures 552-562)
        if (K > 0 && !integrateFeaturesInformation(K, keyPoints.data())) return false;
    }
    m_nShowMap = m_nMapFeatures + m_nStoreMap;                                                                 // 1422
    m_frame.counter++;                                                                                         // 1424-1425
    m_frame.index = (int)m_odoTheta.at(0, m_frame.counter);
    const int dim = 6 * m_nMapFeatures + 4;                                                                    // 1427-1428: heading of the next odometry sample
    std::vector<double> X(dim), S((size_t)dim * dim);
    if (!check(srukf_get_state(ctx_, X.data(), S.data()))) return false;
    X[dim - 1] = m_odoTheta.at(1, m_frame.counter);
    if (!check(srukf_set_state(ctx_, X.data(), S.data()))) return false;
    if (m_nAddings > 0 && !check(srukf_set_new_landmarks(ctx_, m_nAddings))) return false;                     // set_state keeps K_new; explicit for clarity
    refreshMirrors();
    return true;
}

// SLAM.cpp:1343-1465: the redirection restart, then the numeric tail 1430-1465 on the device.
void CSLAM::predictMotion()
{
    if (!ctx_ && m_gryImage && !addFeatures) {                                                                 // on-device detection from frame 1: the 4-state filter of
        if (!check(srukf_create(&ctx_, 0, &m_params, device_, nullptr))) return;                               // initializeParameters (221-231, heading of loadOdometryData 397)
        if (!check(srukf_set_state(ctx_, m_X_k.data.data(), m_S_k.data.data()))) return;
    }
    if (!ctx_) { lastError = "predictMotion before setMap"; return; }
    m_frame.index = (int)m_odoTheta.at(0, m_frame.counter);                                                    // 1351
    if (m_odoTheta.at(2, m_frame.counter) == 1 && !redirection()) return;                                      // 1354-1428
    const int c = m_frame.counter;
    const double prev[3] = { m_odoXY[2 * c - 2], m_odoXY[2 * c - 1], m_odoTheta.at(1, c - 1) };               // 1444-1450
    const double cur[3]  = { m_odoXY[2 * c], m_odoXY[2 * c + 1], m_odoTheta.at(1, c) };
    // the odometry file is loaded whole before the first frame (loadOdometryData): the next frame's pair is known, and announcing it lets this frame's
    // update leave the next frame's sigma points projected (include/srukf.h: srukf_predict_motion_next).  Not across a redirection restart.
    if (c + 1 < m_odoCounter && c + 1 <= CAPACITY && m_odoTheta.at(2, c + 1) != 1) {
        const double next[3] = { m_odoXY[2 * c + 2], m_odoXY[2 * c + 3], m_odoTheta.at(1, c + 1) };
        if (!check(srukf_predict_motion_next(ctx_, cur, next))) return;
    }
    check(srukf_predict_motion(ctx_, prev, cur));
}

// SLAM.cpp:1604-1608 + the bookkeeping of QrAndCholeskyForMeasurement (1724-1745)
void CSLAM::predictMeasurement()
{
    if (!ctx_) return;
    const int N = m_nMapFeatures;
    std::vector<double> h(2 * N), Si(4 * N);
    std::vector<int> vis(N);
    if (!check(srukf_predict_measurement(ctx_, h.data(), Si.data(), vis.data()))) return;
    m_nPredicts = 0;
    for (int k = 0; k < N; k++) {
        PointsMap& p = map[k];
        p.isVisible = vis[k] != 0;
        if (p.isVisible) {                                                                                     // 1727-1738
            m_nPredicts++;
            p.isMatching = false;
            p.nPredictTimes++;
            p.predictLocation.x = h[2 * k]; p.predictLocation.y = h[2 * k + 1];
            memcpy(p.Si, &Si[4 * k], sizeof p.Si);
        }
    }
}

// every update of the facade: the reference's form in m_updateMode, or with jointUpdate the joint form
int CSLAM::filterUpdate(const double* z, const int* matched, int reorder)
{
    if (!jointUpdate) return srukf_update(ctx_, z, matched, reorder, m_updateMode);
    const int rc = srukf_update_joint(ctx_, z, matched, reorder);
    int fr = -1;
    if (rc == SRUKF_OK && reorder == FLAG_4_NEEDNOT_REORDER && srukf_clamp_info(ctx_, &fr, nullptr) == SRUKF_OK && fr >= 0) m_nJointFlagged++;
    return rc;
}

// SLAM.cpp:2048-2104
void CSLAM::KalmanUpdate()
{
    if (!ctx_) return;
    const int N = m_nMapFeatures;
    std::vector<double> z(2 * N, 0.0);
    std::vector<int> m(N, 0);
    m_nMatches = 0; m_nLowInliers = 0; m_nHighInliers = 0;
    for (int k = 0; k < N; k++) {
        map[k].inliner_L = map[k].inliner_H = false;
        if (!map[k].isMatching || std::find(reacquired_.begin(), reacquired_.end(), k) != reacquired_.end()) continue;   // (those come last, one at a time)
        m[k] = 1; z[2 * k] = map[k].matchLocation.x; z[2 * k + 1] = map[k].matchLocation.y; m_nMatches++;
    }
    if (m_nMatches == 0) { updateReacquiredLoopNodes(false); return; }                                         // 2050-2051
    if (!isUseRANSAC || m_nMatches < 2) {                                                                      // 2058-2095 (one match cannot out-vote itself)
        for (int k = 0; k < N; k++) if (m[k]) map[k].nMatchTimes++;
        const int reorder = (m_nAddings != 0) ? FLAG_4_NEED_REORDER : FLAG_4_NEEDNOT_REORDER;                  // 2083-2090
        if (check(filterUpdate(z.data(), m.data(), reorder))) updateReacquiredLoopNodes(true);
        return;
    }
    ransacZ_.swap(z); ransacM_.swap(m);                                                                        // 2097-2103
    if (onePointRansacHypotheses() && updateLowInnovationInliers() && rescueHighInnovationInliers()) updateHighInnovationInliers();
    // what the filter really used: the deletion policy (2443) and addFeatures' trigger (556) read these
    for (int k = 0; k < N; k++) {
        if (!ransacM_[k]) continue;
        if (map[k].inliner_L || map[k].inliner_H) map[k].nMatchTimes++;
        else map[k].isMatching = false;
    }
    m_nMatches = m_nLowInliers + m_nHighInliers;
    if (lastError.empty()) updateReacquiredLoopNodes(m_nMatches > 0);
}

// ---- archived landmarks found in the frame by appearance ---------------------------------------------------------------------
// After updateFeaturesInformation and before addFeatures (and in front of a redirection restart's addFeatures).  The entries with a record and an init patch are
// the device's archive, sent again only when their IDs or the handle's count differ from what the last mirror sent; the search runs on the held frame (on
// m_gryImage when nothing uploaded this frame yet); every matched entry goes back by the loop-point route
bool CSLAM::searchArchive()
{
    archiveVerdict_.clear(); reacquire_.clear();
    if (!ctx_ || !reinsertLoopPoints) return true;
    std::vector<int> idx, ids;
    for (int a = 0; a < (int)m_featuresAllInfo.size(); a++)
        if (m_featuresAllInfo[a].hasRecord && m_featuresAllInfo[a].hasInitPatch) { idx.push_back(a); ids.push_back(m_featuresAllInfo[a].ID); }
    const int L = (int)idx.size();
    if (ids != archiveMirror_ || srukf_archive_count(ctx_) != L) {
        std::vector<double> X6(6 * (size_t)L), S66(36 * (size_t)L), R(9 * (size_t)L), t(3 * (size_t)L), px(2 * (size_t)L);
        std::vector<unsigned char> patches(441 * (size_t)L);
        for (int j = 0; j < L; j++) {
            const FeatureInfo& fi = m_featuresAllInfo[idx[j]];
            memcpy(&X6[6 * j], fi.state, sizeof fi.state); memcpy(&S66[36 * j], fi.sr, sizeof fi.sr);
            memcpy(&R[9 * j], fi.initRotation, sizeof fi.initRotation); memcpy(&t[3 * j], fi.initTrans, sizeof fi.initTrans);
            px[2 * j] = fi.initPixel.x; px[2 * j + 1] = fi.initPixel.y;
            memcpy(&patches[441 * (size_t)j], fi.initPatch, 441);
        }
        if (!check(srukf_archive_set(ctx_, L, X6.data(), S66.data(), patches.data(), R.data(), t.data(), px.data()))) return false;
        archiveMirror_ = ids;
    }
    if (L == 0 || (!frameHeld_ && !m_gryImage)) return true;
    srukf_archive_params ap; ap.half_cap = archiveSearchHalfCap; ap.corr_threshold = 0.8; ap.chi2 = 5.99146454710798;
    std::vector<int> matched(L);
    if (!check(srukf_archive_search(ctx_, frameHeld_ ? nullptr : m_gryImage, &ap, nullptr, nullptr, nullptr, nullptr, matched.data(), nullptr))) return false;
    frameHeld_ = true;
    std::vector<int> take;
    for (int j = 0; j < L; j++) if (matched[j]) { take.push_back(idx[j]); archiveVerdict_.push_back(ids[j]); reacquire_.push_back(std::make_pair(ids[j], j)); }
    ArchiveSearch log; log.frame = m_frame.counter; log.searched = L; log.n_before = m_nMapFeatures; log.archived_before = (int)m_featuresAllInfo.size();
    std::vector<double> x6s, srs;
    if (!reinsertEntries(take, log.ids, x6s, srs)) return false;
    m_nArchiveMatches += (int)take.size();
    log.n_after = m_nMapFeatures; log.archived_after = (int)m_featuresAllInfo.size();
    if (logDetectPasses) m_archiveLog.push_back(log);
    return true;
}

// The frame after a search put nodes back: the ordinary association looks +- 10 px around the prediction (HP_INIT, 1955-1956), the drift that archived landmarks
// are looked for across is larger.  Their records are still on the device in their slots, with the state and factor the nodes went back with, so one more search
// of this frame (pose and P4 of the predicted state) finds them with the gate's window; its z becomes the match of every such node the association left unmatched
bool CSLAM::reacquireLoopNodes()
{
    reacquired_.clear();
    std::vector<std::pair<int, int>> want; want.swap(reacquire_);
    const int L = (int)archiveMirror_.size();
    if (want.empty() || !ctx_ || srukf_archive_count(ctx_) != L || (!frameHeld_ && !m_gryImage)) return true;
    srukf_archive_params ap; ap.half_cap = archiveSearchHalfCap; ap.corr_threshold = 0.8; ap.chi2 = 5.99146454710798;
    std::vector<int> matched(L); std::vector<double> z(2 * (size_t)L);
    if (!check(srukf_archive_search(ctx_, frameHeld_ ? nullptr : m_gryImage, &ap, nullptr, nullptr, nullptr, z.data(), matched.data(), nullptr))) return false;
    frameHeld_ = true;
    for (const auto& w : want) {
        if (!matched[w.second]) continue;
        for (int k = 0; k < m_nMapFeatures; k++) {
            if (map[k].ID != w.first || !map[k].isLoop) continue;
            if (map[k].isVisible && !map[k].isMatching) {
                map[k].isMatching = true; map[k].matchLocation.x = z[2 * w.second]; map[k].matchLocation.y = z[2 * w.second + 1];
                reacquired_.push_back(k);
            }
            break;
        }
    }
    return true;
}

// KalmanUpdate's part for the nodes reacquireLoopNodes matched: one srukf_update each, predicted again from the posterior in between, behind the frame's ordinary
// matches.  The reference's update forms every landmark's gain from the same prior and sums the corrections (2070-2080): landmarks that agree on an innovation of
// tens of pixels, which is what a re-found landmark brings, overshoot together; taken one at a time each sees what the ones before left.  From the second update of
// the frame on, a node must pass dataAssociation's chi-square gate (1977) at the prediction from the posterior, as a rescued RANSAC match must
bool CSLAM::updateReacquiredLoopNodes(bool updated)
{
    if (reacquired_.empty()) return true;
    std::vector<int> nodes; nodes.swap(reacquired_);
    const int N = m_nMapFeatures;
    const double CHI2INV_0_2 = 5.99146454710798;
    const int reorder = (m_nAddings != 0) ? FLAG_4_NEED_REORDER : FLAG_4_NEEDNOT_REORDER;
    std::vector<double> z(2 * (size_t)N, 0.0), h(2 * (size_t)N), Si(4 * (size_t)N); std::vector<int> m(N, 0), vis(N);
    if (jointUpdate) {
        // the joint form has the cross terms the one-at-a-time order stands in for: all nodes in ONE update; behind an update of this frame each must still pass the
        // gate at the prediction from the posterior
        if (updated && !check(srukf_repredict_measurement(ctx_, h.data(), Si.data(), vis.data()))) return false;
        int taken = 0;
        for (int k : nodes) {
            bool take = true;
            if (updated) {
                const double s00 = Si[4 * k], s01 = Si[4 * k + 1], s11 = Si[4 * k + 3];
                take = vis[k] && s00 != 0.0 && s11 != 0.0;
                if (take) {
                    const double v0 = map[k].matchLocation.x - h[2 * k], v1 = map[k].matchLocation.y - h[2 * k + 1];
                    const double y0 = v0 / s00, y1 = (v1 - s01 * y0) / s11;
                    take = y0 * y0 + y1 * y1 < CHI2INV_0_2;
                }
            }
            if (!take) { map[k].isMatching = false; continue; }
            m[k] = 1; z[2 * k] = map[k].matchLocation.x; z[2 * k + 1] = map[k].matchLocation.y; taken++;
        }
        if (taken == 0) return true;
        if (!check(filterUpdate(z.data(), m.data(), reorder))) return false;
        for (int k = 0; k < N; k++) if (m[k]) { map[k].nMatchTimes++; m_nMatches++; m_nArchiveReacquired++; }
        return true;
    }
    for (int k : nodes) {
        bool take = true;
        if (updated) {
            if (!check(srukf_repredict_measurement(ctx_, h.data(), Si.data(), vis.data()))) return false;
            const double s00 = Si[4 * k], s01 = Si[4 * k + 1], s11 = Si[4 * k + 3];
            take = vis[k] && s00 != 0.0 && s11 != 0.0;
            if (take) {
                const double v0 = map[k].matchLocation.x - h[2 * k], v1 = map[k].matchLocation.y - h[2 * k + 1];
                const double y0 = v0 / s00, y1 = (v1 - s01 * y0) / s11;
                take = y0 * y0 + y1 * y1 < CHI2INV_0_2;
            }
        }
        if (!take) { map[k].isMatching = false; continue; }
        std::fill(m.begin(), m.end(), 0); m[k] = 1;
        z[2 * k] = map[k].matchLocation.x; z[2 * k + 1] = map[k].matchLocation.y;
        if (!check(filterUpdate(z.data(), m.data(), reorder))) return false;
        updated = true;
        map[k].nMatchTimes++; m_nMatches++; m_nArchiveReacquired++;
    }
    return true;
}

// Civera's 1-point hypotheses, all of them (srukf_ransac_consensus): the low-innovation inliers are the consensus set of the best one
bool CSLAM::onePointRansacHypotheses()
{
    const int N = m_nMapFeatures;
    std::vector<int> inl(N, 0);
    int best = -1;
    if (!check(srukf_ransac_consensus(ctx_, ransacZ_.data(), ransacM_.data(), THRESHOLD_RANSAC, inl.data(), nullptr, nullptr, &best))) return false;
    for (int k = 0; k < N; k++) { map[k].inliner_L = inl[k] != 0; m_nLowInliers += inl[k] ? 1 : 0; }
    return true;
}

bool CSLAM::updateLowInnovationInliers()
{
    if (m_nLowInliers == 0) return true;
    const int N = m_nMapFeatures;
    std::vector<int> m(N, 0);
    for (int k = 0; k < N; k++) m[k] = map[k].inliner_L ? 1 : 0;
    const int reorder = (m_nAddings != 0) ? FLAG_4_NEED_REORDER : FLAG_4_NEEDNOT_REORDER;                      // as the plain branch, 2083-2090
    return check(filterUpdate(ransacZ_.data(), m.data(), reorder));
}

// a match outside the consensus set is rescued when, seen from the posterior of the first update, it is still visible and passes the chi-square gate
// dataAssociation uses (1977): (z - h)^T (Si^T Si)^-1 (z - h) < CHI2INV_TABLE(0, 2)
bool CSLAM::rescueHighInnovationInliers()
{
    const int N = m_nMapFeatures;
    if (m_nLowInliers == 0 || m_nLowInliers == m_nMatches) return true;
    const double CHI2INV_0_2 = 5.99146454710798;
    if (rescueGateOnDevice) {
        // the same rule on the device, from the posterior in place; the full prediction only when the second update will need it
        std::vector<int> inl(N), fl(N);
        int nh = 0;
        for (int k = 0; k < N; k++) inl[k] = map[k].inliner_L ? 1 : 0;
        if (!check(srukf_rescue_gate(ctx_, ransacZ_.data(), ransacM_.data(), inl.data(), CHI2INV_0_2, fl.data(), nullptr, nullptr, nullptr, &nh))) return false;
        for (int k = 0; k < N; k++) if (fl[k] & SRUKF_RESCUE_RESCUED) { map[k].inliner_H = true; m_nHighInliers++; }
        if (nh == 0) { m_nGateSkips++; return true; }
        return check(srukf_repredict_measurement(ctx_, nullptr, nullptr, nullptr));
    }
    std::vector<double> h(2 * N), Si(4 * N);
    std::vector<int> vis(N);
    if (!check(srukf_repredict_measurement(ctx_, h.data(), Si.data(), vis.data()))) return false;
    for (int k = 0; k < N; k++) {
        if (!ransacM_[k] || map[k].inliner_L || !vis[k]) continue;
        const double s00 = Si[4 * k], s01 = Si[4 * k + 1], s11 = Si[4 * k + 3];
        if (s00 == 0.0 || s11 == 0.0) continue;
        // y = Si^-T (z - h) by forward substitution (Si is upper triangular: the library stores Si[2] = 0): the distance is |y|^2
        const double v0 = ransacZ_[2 * k] - h[2 * k], v1 = ransacZ_[2 * k + 1] - h[2 * k + 1];
        const double y0 = v0 / s00, y1 = (v1 - s01 * y0) / s11;
        if (y0 * y0 + y1 * y1 < CHI2INV_0_2) { map[k].inliner_H = true; m_nHighInliers++; }
    }
    return true;
}

bool CSLAM::updateHighInnovationInliers()
{
    if (m_nHighInliers == 0) return true;
    const int N = m_nMapFeatures;
    std::vector<int> m(N, 0);
    for (int k = 0; k < N; k++) m[k] = map[k].inliner_H ? 1 : 0;
    // (a frame that follows a landmark addition keeps FLAG_4_NEED_REORDER for this update too, as every per-landmark update of such a frame does in the reference, 2083-2090)
    const int reorder = (m_nAddings != 0) ? FLAG_4_NEED_REORDER : FLAG_4_NEEDNOT_REORDER;
    return check(filterUpdate(ransacZ_.data(), m.data(), reorder));
}

void CSLAM::refreshMirrors()
{
    if (!ctx_) return;
    const int n = m_X_k.rows;
    if (mirrorsFresh_ && !fullCovariance) { mirrorsFresh_ = false; return; }      // updateFeaturesInformation fetched them with the display refresh, and the map has not changed since
    if (fullCovariance) {
        check(srukf_get_state(ctx_, m_X_k.data.data(), m_S_k.data.data()));
        check(srukf_get_covariance(ctx_, m_P_k.data.data()));                                                  // 2404
    } else {
        check(srukf_get_state(ctx_, m_X_k.data.data(), nullptr));
        double pose[4], P4[16];
        check(srukf_get_robot(ctx_, pose, P4));                                                                // the 2x2 / 4x4 block the host reads (3539-3556)
        for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) m_P_k.at(n - 4 + a, n - 4 + b) = P4[4 * a + b];
    }
}

// SLAM.cpp:2957-3000: trajectory buffer the OpenGL view draws (m_path)
void CSLAM::updateRobotInformation()
{
    const int n = m_X_k.rows, c = m_frame.counter;
    if (c <= CAPACITY) { m_path[2 * c] = m_X_k.at(n - 4, 0); m_path[2 * c + 1] = m_X_k.at(n - 3, 0); }
}

// SLAM.cpp:3512-3562: idx \t odoX \t odoY \t x \t y \t P00 \t P01 \t P10 \t P11
void CSLAM::recordRobotInformation()
{
    if (!isRecordRobotInfo) return;
    const int n = m_X_k.rows, c = m_frame.counter;
    if (!robotFile_) {
        robotFile_ = fopen(m_recordRobotDir.c_str(), "a");
        if (!robotFile_) { lastError = "cannot open " + m_recordRobotDir; return; }
    }
    fprintf(robotFile_, "%d\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t%f\t\n", m_showCounter, m_odoXY[2 * c], m_odoXY[2 * c + 1],
            m_X_k.at(n - 4, 0), m_X_k.at(n - 3, 0), m_P_k.at(n - 4, n - 4), m_P_k.at(n - 4, n - 3), m_P_k.at(n - 3, n - 4), m_P_k.at(n - 3, n - 3));
    fflush(robotFile_);
}

// SLAM.cpp:87-112
void CSLAM::SLAM()
{
    const auto t0 = std::chrono::steady_clock::now();                                                          // startTimer 122-132
    m_showCounter++;
    mirrorsFresh_ = false;
    frameHeld_ = false;
    predictMotion();
    predictMeasurement();
    if (dataAssociation) dataAssociation(*this);                                                               // loadPictures + dataAssociation (95-97)
    if (searchArchivedLandmarks) reacquireLoopNodes();
    KalmanUpdate();
    updateFeaturesInformation();                                                                               // deletion policy + display refresh (2397-2621)
    if (searchArchivedLandmarks) searchArchive();
    refreshMirrors();                                                                                          // m_P_k (2404), m_X_k, m_S_k
    updateRobotInformation();
    recordRobotInformation();
    m_nAddings = 0;                                                                                            // addFeatures (552-562)
    if ((m_nMatches < m_minNUM || isAdding) && addFeatures) {                                                  // 556: the host detects, the facade joint-initialises
        std::vector<double> keyPoints;
        const int K = addFeatures(*this, keyPoints);
        if (K > 0) integrateFeaturesInformation(K, keyPoints.data());
    } else if ((m_nMatches < m_minNUM || isAdding) && m_gryImage) {
        addFeaturesOnDevice();                                                                                 // 556-561 on the device
    }
    m_frame.counter++;                                                                                         // stopTimer 142-151
    m_frameTime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    m_totalTime += m_frameTime;
}

// Up to F frames of SLAM() as ONE image block on the device: the association (dataAssociationOnDevice's) and the update run inside the block, the
// map policy's verdict (updateFeaturesInformation's tests 2443-2459, the addFeatures trigger 556) behind every frame; the block stops at the first frame whose
// verdict asks for a map change, and that change is made by the unchanged host code on that frame.  With isUseRANSAC the consensus runs inside every frame
//  and the block also stops IN FRONT OF the first frame whose consensus dropped a match: its rescue step is SLAM()'s — with rescueGateOnDevice
//  in front of the first frame that would rescue one, and a frame whose dropped matches stay dropped is consumed.  gray: F frames of image_h x image_w, frame f for
// m_frame.counter + f.  Returns the frames consumed, or 0 with nothing done where a block cannot stand for SLAM(): the caller then calls SLAM() for the frame.
int CSLAM::SLAMBlock(const unsigned char* gray, int F) { return slamBlock(gray, F, false); }

// The same for the frames cvQueryFrame / cvLoadImage deliver: bgr = F frames of image_h x image_w x 3 bytes, B, G, R.  The device makes of them
// what loadPictures makes (srukf_stage_images_bgr); with blockDisplay the colour stack stays and the overlays are drawn on it
int CSLAM::SLAMBlockColour(const unsigned char* bgr, int F) { return slamBlock(bgr, F, true); }

// the one body behind both: frames = gray, or with colour the B, G, R frames
int CSLAM::slamBlock(const unsigned char* frames, int F, bool colour)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int N = m_nMapFeatures, c0 = m_frame.counter;
    if (!ctx_ || !frames || N < 1 || c0 < 1) return 0;
    if (c0 + F > m_odoCounter) F = m_odoCounter - c0;
    if (c0 + F > CAPACITY + 1) F = CAPACITY + 1 - c0;
    if (F < 1) return 0;
    if (m_nAddings != 0 || isAdding || searchArchivedLandmarks || reinsertLoopPoints || dataAssociation || addFeatures) return 0;
    if (!jointUpdate && m_updateMode != SRUKF_UPDATE_BATCHED) return 0;
    for (int f = 0; f < F; f++) if (m_odoTheta.at(2, c0 + f) == 1) return 0;                                   // a redirection restart inside the range
    const size_t img = (size_t)m_params.image_w * (size_t)m_params.image_h;
    // 1. odometry rows [c0 - 1, c0 + F) and the F frames
    std::vector<double> odo(3 * (size_t)(F + 1)), z0(2 * (size_t)F * N, 0.0);
    std::vector<int> m0((size_t)F * N, 0);
    for (int f = 0; f <= F; f++) { const int c = c0 - 1 + f; odo[3 * f] = m_odoXY[2 * c]; odo[3 * f + 1] = m_odoXY[2 * c + 1]; odo[3 * f + 2] = m_odoTheta.at(1, c); }
    if (!check(srukf_stage_sequence(ctx_, F, odo.data(), z0.data(), m0.data()))) return 0;
    int rc = colour ? srukf_stage_images_bgr(ctx_, F, frames, blockDisplay ? 1 : 0) : srukf_stage_images(ctx_, F, frames);
    if (rc == SRUKF_ERR_UNSUPPORTED) return 0;
    if (!check(rc)) return 0;
    // 2. the counters map[] holds
    std::vector<srukf_policy_state> st(N);
    for (int k = 0; k < N; k++) st[k] = { map[k].nPredictTimes, map[k].nMatchTimes, { map[k].predictLocation.x, map[k].predictLocation.y } };
    const srukf_policy_params pp = { (double)DIST_2_BORDER, 0.01, 10, m_minNUM };
    if (!check(srukf_images_policy(ctx_, 1, &pp)) || !check(srukf_images_set_policy_state(ctx_, st.data()))) return 0;
    if (!check(srukf_images_ransac(ctx_, isUseRANSAC ? 1 : 0, THRESHOLD_RANSAC))) return 0;                     // the consensus inside every frame, or not
    const bool gate = isUseRANSAC && rescueGateOnDevice;                                                        // the rescue gate behind every such frame
    if ((gate || rescueSet_) && !check(srukf_images_rescue_gate(ctx_, gate ? 1 : 0, 5.99146454710798))) return 0;
    rescueSet_ = gate;
    if ((resumeStoppedBlocks || snapshotsSet_) && !check(srukf_images_snapshots(ctx_, resumeStoppedBlocks ? 1 : 0))) return 0;      // the state at the stop, kept by the first run
    snapshotsSet_ = resumeStoppedBlocks;
    if ((blockDisplay || displaySet_) && !check(srukf_images_display(ctx_, blockDisplay ? 1 : 0))) return 0;                // the display view behind every frame
    displaySet_ = blockDisplay;
    m_blockDisplay.clear(); m_blockDisplayIDs.clear(); m_blockOverlays.clear();
    // 3. one image block in jointUpdate's mode, checked with the switches of associateChecked
    const int mode = jointUpdate ? SRUKF_UPDATE_JOINT : SRUKF_UPDATE_BATCHED;
    const bool checked = rejectAmbiguousMatches || subpixelMatches;
    const srukf_match_params mp = { 0.8, rejectAmbiguousMatches ? AMBIGUITY_RATIO : 2.0, AMBIGUITY_EXCLUSION, subpixelMatches ? 1 : 0 };
    std::vector<double> traj(8 * (size_t)F);
    auto run = [&](int count) { return checked ? srukf_run_images_checked(ctx_, 0, count, mode, &mp, traj.data()) : srukf_run_images(ctx_, 0, count, mode, traj.data()); };
    rc = run(F);
    if (rc == SRUKF_ERR_CLAMP_PENDING || rc == SRUKF_ERR_UNSUPPORTED) return 0;                                 // a flagged block (its restore has run), the float-stored modes
    if (!check(rc)) return 0;
    // 4. / 5. the records; a frame in front of the last asks for a map change, or a frame's consensus dropped a match (that frame needs the rescue: it is not the
    // block's): back to the block's start and up to the stop
    int fc = -1, fo = -1, used = F;
    if (!check(srukf_get_image_policy(ctx_, 0, F, nullptr, nullptr, nullptr, &fc))) return 0;
    if (gate) { if (!check(srukf_get_image_rescue(ctx_, 0, F, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &fo))) return 0; }      // first_rescue: a frame that only dropped matches stands
    else if (isUseRANSAC && !check(srukf_get_image_ransac(ctx_, 0, F, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &fo))) return 0;
    if (fc >= 0) used = std::min(used, fc + 1);
    if (fo >= 0) used = std::min(used, fo);
    // resumeStoppedBlocks: the first run kept the state at the stop (srukf_images_resume); where no slot holds it, the rewind and the frames again
    bool resumed = false;
    if (resumeStoppedBlocks && used > 0 && used < F) {
        rc = srukf_images_resume(ctx_, used);
        if (rc == SRUKF_OK) { resumed = true; m_nBlocksResumed++; }
        else if (rc != SRUKF_ERR_SEQUENCE) { check(rc); return 0; }
    }
    if (used < F && !resumed) {
        if (!check(srukf_images_rewind(ctx_))) return 0;
        if (used == 0) return 0;                                                                                // the first frame is SLAM()'s: nothing done
        rc = run(used);
        if (rc == SRUKF_ERR_CLAMP_PENDING) return 0;
        if (!check(rc)) return 0;
    }
    // 6. SLAM()'s bookkeeping for every consumed frame, from the records
    std::vector<double> z(2 * (size_t)used * N), h(2 * (size_t)used * N), corr((size_t)used * N), corr2, z2;
    std::vector<int> m((size_t)used * N), vis((size_t)used * N), fl;
    if (!check(srukf_get_image_matches(ctx_, 0, used, z.data(), m.data(), corr.data(), vis.data(), h.data()))) return 0;
    if (checked) {
        corr2.resize((size_t)used * N); z2.resize(2 * (size_t)used * N); fl.resize((size_t)used * N);
        if (!check(srukf_get_image_checks(ctx_, 0, used, corr2.data(), z2.data(), fl.data()))) return 0;
    }
    if (!check(srukf_get_image_policy(ctx_, 0, used, nullptr, nullptr, st.data(), nullptr))) return 0;
    std::vector<int> rfl, ract, rlow;
    if (isUseRANSAC) {
        rfl.resize((size_t)used * N); ract.resize(used); rlow.resize(used);
        if (!check(srukf_get_image_ransac(ctx_, 0, used, rfl.data(), nullptr, nullptr, nullptr, ract.data(), rlow.data(), nullptr))) return 0;
    }
    if (blockDisplay) {                                                                                         // the display view of every consumed frame, IDs in state order
        const size_t U = (size_t)used;
        std::vector<double> xyz(U * 3 * N), cov(U * 9 * N), axis(U * 4 * N), sigma(U * 3 * N), pose(U * 4), P4(U * 16), Si(U * 4 * N);
        std::vector<int> rot(U * N);
        if (!check(srukf_get_image_display(ctx_, 0, used, xyz.data(), cov.data(), axis.data(), sigma.data(), rot.data(), pose.data(), P4.data(), Si.data()))) return 0;
        m_blockDisplay.resize(U);
        for (size_t f = 0; f < U; f++) {
            BlockDisplayFrame& d = m_blockDisplay[f];
            d.xyz.assign(xyz.begin() + f * 3 * N, xyz.begin() + (f + 1) * 3 * N); d.cov.assign(cov.begin() + f * 9 * N, cov.begin() + (f + 1) * 9 * N);
            d.axis.assign(axis.begin() + f * 4 * N, axis.begin() + (f + 1) * 4 * N); d.sigma.assign(sigma.begin() + f * 3 * N, sigma.begin() + (f + 1) * 3 * N);
            d.Si.assign(Si.begin() + f * 4 * N, Si.begin() + (f + 1) * 4 * N); d.rot.assign(rot.begin() + f * N, rot.begin() + (f + 1) * N);
            std::copy(pose.begin() + f * 4, pose.begin() + (f + 1) * 4, d.pose); std::copy(P4.begin() + f * 16, P4.begin() + (f + 1) * 16, d.P4);
        }
        for (int k = 0; k < N; k++) m_blockDisplayIDs.push_back(map[k].ID);
        if (blockOverlayLast) {                                                                                 // (in front of the tail: a map change drops the staged frames)
            m_srcImage.resize(3 * img);
            if (!check(srukf_render_image_overlay(ctx_, used - 1, m_srcImage.data()))) return 0;
        }
        if (blockOverlayAll) {                                                                                  // every consumed frame's, in one device call
            m_blockOverlays.resize(U * 3 * img);
            if (!check(srukf_render_image_overlays(ctx_, 0, used, m_blockOverlays.data()))) return 0;
        }
    }
    if (colour) {                                                                                               // the gray frame the tail reads, as loadPictures leaves it; read
        m_grayStore.resize(img);                                                                                // here, where a refusal still leaves the facade as it was
        if (!check(srukf_get_staged_image(ctx_, used - 1, m_grayStore.data(), nullptr))) return 0;
    }
    const int n = m_X_k.rows;
    m_blockPath.assign(traj.begin(), traj.begin() + 8 * (size_t)used);
    m_blockLowInliers.assign(used, 0);
    for (int f = 0; f < used; f++) {
        const bool last = f == used - 1;
        m_showCounter++;
        mirrorsFresh_ = false;
        clearAmbiguity();
        m_nPredicts = 0; m_nMatches = 0; m_nLowInliers = 0; m_nHighInliers = 0;
        for (int k = 0; k < N; k++) {
            const size_t r = (size_t)f * N + k;
            PointsMap& p = map[k];
            p.isVisible = vis[r] != 0; p.isMatching = m[r] != 0;
            p.inliner_L = isUseRANSAC && ract[f] >= 2 && (rfl[r] & SRUKF_RANSAC_INLIER) != 0;                   // (one match cannot out-vote itself: KalmanUpdate's m_nMatches < 2 branch)
            p.inliner_H = false;
            if (p.isVisible) m_nPredicts++;
            if (p.isMatching) { p.matchLocation.x = z[2 * r]; p.matchLocation.y = z[2 * r + 1]; m_nMatches++; }
            if (checked) {
                p.isAmbiguous = (fl[r] & 2) != 0; p.corr = corr[r]; p.corr2 = corr2[r]; p.rivalLocation.x = z2[2 * r]; p.rivalLocation.y = z2[2 * r + 1];
                if (p.isAmbiguous) { m_nAmbiguous++; m_ambiguousID.push_back(p.ID); }
            }
            if (last) { p.nPredictTimes = st[k].nPredictTimes; p.nMatchTimes = st[k].nMatchTimes; p.predictLocation.x = st[k].predictLocation[0]; p.predictLocation.y = st[k].predictLocation[1]; }
        }
        m_nAmbiguousTotal += m_nAmbiguous;
        if (isUseRANSAC && ract[f] >= 2) m_nLowInliers = rlow[f];
        m_blockLowInliers[f] = m_nLowInliers;
        m_frame.index = (int)m_odoTheta.at(0, m_frame.counter);
        if (!last) {
            const double* t = &traj[8 * (size_t)f];                                                              // pose + the 2 x 2 block of P, as the trajectory holds them
            for (int e = 0; e < 4; e++) m_X_k.at(n - 4 + e, 0) = t[e];
            m_P_k.at(n - 4, n - 4) = t[4]; m_P_k.at(n - 4, n - 3) = t[5]; m_P_k.at(n - 3, n - 4) = t[6]; m_P_k.at(n - 3, n - 3) = t[7];
            updateRobotInformation();
            recordRobotInformation();
            m_nAddings = 0;
            m_frame.counter++;
        }
    }
    // 7. the last consumed frame: SLAM()'s own tail on that frame (997-1010)
    m_gryImage = colour ? m_grayStore.data() : frames + (size_t)(used - 1) * img;                              // (colour: read back in front of step 6)
    frameHeld_ = false;
    updateFeaturesInformation();
    refreshMirrors();
    {
        const int nl = m_X_k.rows; double* t = &m_blockPath[8 * (size_t)(used - 1)];                           // (the last frame's row as the mirrors have it, behind the deletions)
        for (int e = 0; e < 4; e++) t[e] = m_X_k.at(nl - 4 + e, 0);
        t[4] = m_P_k.at(nl - 4, nl - 4); t[5] = m_P_k.at(nl - 4, nl - 3); t[6] = m_P_k.at(nl - 3, nl - 4); t[7] = m_P_k.at(nl - 3, nl - 3);
    }
    updateRobotInformation();
    recordRobotInformation();
    m_nAddings = 0;
    if (m_nMatches < m_minNUM && m_gryImage) addFeaturesOnDevice();                                            // 556-561 on the device
    m_frame.counter++;
    m_frameTime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / used;
    m_totalTime += m_frameTime * used;
    return used;
}

// display2DFeatureModel (SLAM.cpp:3009-3051) for consumed frame f of the last SLAMBlock, from the device's own rows
bool CSLAM::renderBlockOverlay(int f, unsigned char* out_bgr)
{
    if (!ctx_ || !out_bgr || f < 0 || f >= (int)m_blockDisplay.size()) return false;
    return srukf_render_image_overlay(ctx_, f, out_bgr) == SRUKF_OK;
}

}  // namespace monoslam
