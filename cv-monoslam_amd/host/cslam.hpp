// cslam.hpp — CSLAM-shaped C++ facade over the C-ABI (include/srukf.h).
//
// The reference host (MFC view, MonoSLAMView.h:44) embeds `CSLAM SLAM;` by value, calls
// SLAM.SLAM() per frame (MonoSLAMView.cpp:513,554), initializeParameters() / resetAllParameters()
// (:377,:577) and reads public fields (m_X_k, m_S_k, m_P_k, m_frame, m_nMapFeatures, m_nPredicts,
// m_nMatches, m_frameTime, m_totalTime, m_path, m_odoXY, map ...; MonoSLAMView.cpp:76-93,
// OpenGlDisplay.cpp:386-571).  This class keeps those names and meanings for the SRUKF path and
// routes the numerics to the MI355X kernels.  What is NOT here (out of scope): image
// I/O, drawing, MFC controls.  Feature detection runs on the device when the host points m_gryImage at its
// gray frame and installs no addFeatures callback (detectAndfilteringFeatures / insureEnoughFeatures below).  The step between
// predictMeasurement() and KalmanUpdate() — loadPictures() + dataAssociation() in the reference
// (SLAM.cpp:95-97) — is a host callback: it receives the predicted pixels / Si / visibility the
// reference's dataAssociation consumes and fills matchLocation / isMatching.
#pragma once
#include <functional>
#include <string>
#include <vector>
#include "../../include/srukf.h"

namespace monoslam {

// minimal row-major fp64 stand-in for the cv::Mat members the host reads (rows/cols/ptr(i))
struct Mat {
    int rows = 0, cols = 0;
    std::vector<double> data;
    void create(int r, int c) { rows = r; cols = c; data.assign((size_t)r * c, 0.0); }
    double* ptr(int i) { return data.data() + (size_t)i * cols; }
    const double* ptr(int i) const { return data.data() + (size_t)i * cols; }
    double& at(int i, int j) { return data[(size_t)i * cols + j]; }
    double at(int i, int j) const { return data[(size_t)i * cols + j]; }
};

struct Point2d { double x = 0, y = 0; };
struct Point3d { double x = 0, y = 0, z = 0; };
struct Quaternion { double r = 1, x = 0, y = 0, z = 0; };      // SLAM.h:39-45

// SLAM.h:47-70 (numeric fields only)
struct PointsMap {
    int     ID = 0;
    bool    isVisible = false;
    bool    isMatching = false;
    bool    isLoop = false;           // delayed deletion flag the OpenGL view colours by (OpenGlDisplay.cpp:497)      (SLAM.h:52)
    bool    inliner_L = false;        // 1-point RANSAC: low-innovation inlier of this frame (SLAM.cpp:2599-2603)
    bool    inliner_H = false;        // ... high-innovation inlier (rescued after the first update)
    int     nPredictTimes = 0;
    int     nMatchTimes = 0;
    Point2d predictLocation;
    Point2d matchLocation;
    bool    isAmbiguous = false;      // the last association through the facade (dataAssociationOnDevice / ...Held) vetoed this landmark's match: a second correlation
                                      // peak as good as the best (CSLAM::rejectAmbiguousMatches).  Cleared by every such association; a host-installed association
                                      // that does not call them leaves it as it was
    double  corr = 0, corr2 = 0;      // best and second-peak normalised cross correlation of the last association that ran with a switch on (not cleared otherwise)
    Point2d rivalLocation;            // where that second peak sat ((0, 0) without one)
    double  Si[4] = {0, 0, 0, 0};     // 2x2 upper-triangular sqrt innovation covariance
    Point2d initPixel;
    Point3d xyz;                      // Cartesian mean                                  (SLAM.h:64)
    Quaternion axis;                  // orientation of the 1-sigma ellipsoid            (SLAM.h:66)
    Point3d sigma;                    // its semi-axes = sqrt of the eigenvalues of cov  (SLAM.h:67)
    double  cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // Cartesian 3x3 covariance
    PointsMap* next = nullptr;        // singly linked list in state order, NULL-terminated                           (SLAM.h:69)
};

// SLAM.h:94-112 (numeric fields): what the redirection restart archives per landmark of the map it leaves behind
struct FeatureInfo {
    bool    isLoop = false;
    int     ID = 0, nPredictTimes = 0, nMatchTimes = 0;
    Point3d initXYZ;
    Point2d initPixel;
    double  state[6] = {0, 0, 0, 0, 0, 0};   // the landmark's six rows of m_X_k
    Point3d position;                        // Cartesian mean
    double  cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    Quaternion axis;
    Point3d sigma;
    // what the reference's isLoop branch of integrateFeaturesInformation reads back (SLAM.cpp:961-973), filled by srukf_get_landmark_record when
    // CSLAM::reinsertLoopPoints is on (hasRecord): sr = upper Cholesky factor of the landmark's marginal 6x6 block of P (row-major), the appearance record
    double  sr[36] = {0};
    unsigned char initPatch[441] = {0};
    double  initRotation[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double  initTrans[3] = {0, 0, 0};
    bool    hasInitPatch = false;            // the landmark had an appearance record (initPatch / initRotation / initTrans / initPixel)
    bool    hasRecord = false;
};

// SLAM.h:85-92
struct FrameInfo { int rate = 0, start = 1, stop = 0, index = 0, counter = 1; };

class CSLAM {
public:
    static const int CAPACITY = 3000;                          // SLAM.h:127
    const int FLAG_4_NEED_REORDER = 0, FLAG_4_NEEDNOT_REORDER = 1;   // SLAM.cpp:36-37

    explicit CSLAM(int device = 0);
    ~CSLAM();
    CSLAM(const CSLAM&) = delete;
    CSLAM& operator=(const CSLAM&) = delete;

    // ---- members the reference host calls (same names) ------------------------------------
    void initializeParameters();                               // SLAM.cpp:158-353 (numeric defaults only)
    void resetAllParameters();                                 // SLAM.cpp:3090-3128
    void SLAM();                                               // SLAM.cpp:87-112
    // Up to F frames of SLAM() as one image block on the device that stops at the first frame whose map-policy verdict asks for a map change:
    // gray = F frames of image_h x image_w (frame f belongs to m_frame.counter + f).  Stages the odometry rows and the frames, seeds the policy state from map[],
    // runs srukf_run_images* (jointUpdate's mode; checked with rejectAmbiguousMatches / subpixelMatches), rewinds and reruns up to first_change when that is not
    // the last frame, then does SLAM()'s bookkeeping for every consumed frame from the records (counters, isMatching, matchLocation, predictLocation, m_nPredicts,
    // m_nMatches, m_path and the RobotPath row from the trajectory; PointsMap::Si is not refreshed) and SLAM()'s own tail — updateFeaturesInformation,
    // the mirrors, addFeatures on the device — on the last consumed frame, which m_gryImage then points at.  Returns the frames consumed (m_frame.counter has
    // advanced by as many).  Returns 0 with nothing done — call SLAM() for the frame instead — with an empty map, a redirection flag inside the range,
    // m_nAddings != 0 (the next update reorders), isAdding, searchArchivedLandmarks, reinsertLoopPoints, a dataAssociation or addFeatures callback
    // installed, an update mode the image runs do not have, float storage, and for a flagged block (srukf_synchronize has restored it).
    // isUseRANSAC: the 1-point RANSAC consensus runs inside every frame of the block (srukf_images_ransac with THRESHOLD_RANSAC) and the block also
    // ends IN FRONT OF the first frame whose consensus dropped a match: that frame needs the rescue step (rescueHighInnovationInliers), which only SLAM() has, so
    // it is not consumed — the next call returns 0 for it and the caller's SLAM() runs it.  Consumed frames: inliner_L and m_nLowInliers from the consensus record,
    // m_nHighInliers = 0
    // resumeStoppedBlocks: the block's frames keep the state they start from while no stop is on record (srukf_images_snapshots), and a block
    // that stops at 0 < used < F takes the state at the stop from the first run (srukf_images_resume) in place of the rewind and the second run; where no slot
    // holds it (SRUKF_ERR_SEQUENCE) the rewind and the rerun follow as before.  m_nBlocksResumed counts the resumes.  Off: exactly the calls above
    // blockDisplay: the block's frames leave the display view SLAM() refreshes after every update (updateFeaturesInformation ->
    // refreshFeaturesDisplay, SLAM.cpp:2566-2575) in a record on the device (srukf_images_display); behind step 6 the rows of the consumed frames are read into
    // m_blockDisplay, one BlockDisplayFrame each, with the block's landmark IDs in state order in m_blockDisplayIDs.  The last frame's tail is unchanged (its row
    // is the view in front of that tail's map changes).  renderBlockOverlay(f, out): display2DFeatureModel (3009-3051) for consumed frame f of the last block over
    // its gray image, image_h x image_w x 3 bytes (srukf_render_image_overlay); false where no block with blockDisplay has consumed that frame, or the map has
    // changed since — the last frame's tail may change it, so with blockOverlayLast SLAMBlock itself leaves the last consumed frame's overlay in m_srcImage, drawn
    // in front of that tail.  Off and never on: exactly the calls above
    // SLAMBlockColour: SLAMBlock for the frames the reference's host has — bgr = F frames of image_h x image_w x 3 bytes, B, G, R, as
    // cvQueryFrame / cvLoadImage deliver them.  The device converts them as loadPictures does (srukf_stage_images_bgr) and, with blockDisplay, keeps the colour
    // stack: the overlays are then drawn on the colour frames.  The tail's gray frame is read back into m_grayStore, which m_gryImage then points at.
    // blockOverlayAll (with blockDisplay): either call leaves the overlays of all consumed frames in m_blockOverlays, `used` tight frames of
    // image_h x image_w x 3 bytes from one srukf_render_image_overlays, drawn where blockOverlayLast draws.  Off: exactly the calls above
    int  SLAMBlock(const unsigned char* gray, int F);
    int  SLAMBlockColour(const unsigned char* bgr, int F);
    struct BlockDisplayFrame {
        std::vector<double> xyz, cov, axis, sigma, Si;         // [3N], [9N], [4N] (quaternion r, x, y, z), [3N], [4N]
        std::vector<int> rot;                                  // [N]
        double pose[4], P4[16];
    };
    bool blockDisplay = false, blockOverlayLast = false, blockOverlayAll = false;
    std::vector<unsigned char> m_blockOverlays;                // the last block's overlays, one per consumed frame (blockOverlayAll; empty without)
    std::vector<BlockDisplayFrame> m_blockDisplay;             // the last SLAMBlock's display view per consumed frame (blockDisplay; empty without)
    std::vector<int> m_blockDisplayIDs;                        // ... and the block's landmark IDs in state order
    bool renderBlockOverlay(int f, unsigned char* out_bgr);
    bool resumeStoppedBlocks = false;
    int  m_nBlocksResumed = 0;
    // rescueGateOnDevice (with isUseRANSAC): the test "would a dropped match be rescued?" runs on the device.  SLAMBlock switches
    // srukf_images_rescue_gate on with CHI2INV_TABLE(0,2) and stops in front of the first frame that WOULD RESCUE a match (first_rescue) instead of the first that
    // dropped one: a consumed frame with dropped, un-rescued matches is what SLAM() leaves for it (inliner_L from the consensus record, inliner_H false,
    // m_nHighInliers 0).  rescueHighInnovationInliers asks srukf_rescue_gate first and calls srukf_repredict_measurement only when a match is rescued (the second
    // update needs the full prediction); m_nGateSkips counts the repredictions saved.  Off: exactly the calls above
    bool rescueGateOnDevice = false;
    int  m_nGateSkips = 0;
    std::vector<double> m_blockPath;                           // the last SLAMBlock's RobotPath numbers, 8 per consumed frame: x, y, z, theta, P00, P01, P10, P11
    std::vector<int> m_blockLowInliers;                        // ... and with isUseRANSAC its m_nLowInliers per consumed frame
    void predictMotion();                                      // SLAM.cpp:1343-1466 (numeric tail 1430-1465)
    void predictMeasurement();                                 // SLAM.cpp:1604-1608
    void KalmanUpdate();                                       // SLAM.cpp:2048-2104
    // ---- 1-point RANSAC: the four steps KalmanUpdate's isUseRANSAC branch names (2097-2103) and the reference never wrote.  They run in this
    //      order inside KalmanUpdate when isUseRANSAC is on and at least two landmarks matched; a match that is neither kind of inlier is dropped for the frame
    //      (isMatching = false, nMatchTimes not incremented, m_nMatches = m_nLowInliers + m_nHighInliers)
    bool onePointRansacHypotheses();                           // srukf_ransac_consensus: inliner_L, m_nLowInliers
    bool updateLowInnovationInliers();                         // srukf_update with the low-innovation inliers
    bool rescueHighInnovationInliers();                        // srukf_repredict_measurement + dataAssociation's chi-square gate (1977): inliner_H, m_nHighInliers
    bool updateHighInnovationInliers();                        // srukf_update with the rescued matches (skipped when there are none)
    bool   isUseRANSAC = false;                                // SLAM.cpp:185
    double THRESHOLD_RANSAC = 8.0;                             // SLAM.cpp:186, SLAM.h:249: Euclidean pixel distance between measurement and prediction
    int    m_nLowInliers = 0, m_nHighInliers = 0;              // SLAM.h:227-228
    // ---- the joint measurement update (ours).  On: KalmanUpdate's plain branch and the RANSAC inlier updates are ONE update over all of their
    //      matches with the full innovation covariance (srukf_update_joint; m_updateMode is not consulted), and updateReacquiredLoopNodes measures all re-acquired
    //      nodes in one such update instead of one update each.  Off (default): nothing changes
    bool   jointUpdate = false;
    int    m_nJointFlagged = 0;                                // joint updates whose refactorisation was flagged and went to the exact path (srukf_clamp_info)
    int    filterUpdate(const double* z, const int* matched, int reorder);   // srukf_update(m_updateMode), or srukf_update_joint
    void updateRobotInformation();                             // SLAM.cpp:2957-3000 (m_path only)
    void recordRobotInformation();                             // SLAM.cpp:3512-3562 (RobotPath.txt rows)
    bool loadOdometryData(const std::string& path);            // SLAM.cpp:363-496 ("%d : %*lf %lf %lf %lf")

    // ---- map set-up (the reference builds it inside addFeatures -> integrateFeaturesInformation,
    //      SLAM.cpp:552-562, 818-1018; landmark augmentation on the device is a "next" row, so the
    //      host supplies the augmented state) ------------------------------------------------
    //      n_added = m_nFilters: the last n_added landmarks are new; the next KalmanUpdate then takes the
    //      FLAG_4_NEED_REORDER path (SLAM.cpp:2083-2090), as the reference does after integrateFeaturesInformation
    bool setMap(int n_landmarks, const double* X, const double* S, const double* init_pixels /*2N or null*/, int n_added = 0);
    // integrateFeaturesInformation (SLAM.cpp:818-871) for K key points the host detected (m_keyPoints[i].pt, distorted
    // pixels): joint initialisation on the device, the map and the mirrors grow by K, m_nFilters = m_nAddings = K so that
    // the next KalmanUpdate runs FLAG_4_NEED_REORDER.  Works from the empty map of initializeParameters (frame 1).
    bool integrateFeaturesInformation(int K, const double* keyPoints /*2K*/);
    // deleteOneFeature (SLAM.cpp:2637-2706): the id-th landmark of the state (0-based) leaves the filter and the map
    bool deleteOneFeature(int id);
    // ours, beside it: the landmarks at the positions ids (distinct, any order) leave the filter and the map in one device call (srukf_delete_landmarks),
    // one compaction of the map and one refresh of the mirrors.  stored (may be NULL; ids.size() entries): entry q receives the record recordFeature reads for
    // ids[q] (sr, initPatch, initRotation, initTrans, hasInitPatch, hasRecord), taken on the state before the call
    bool deleteFeatures(const std::vector<int>& ids, std::vector<FeatureInfo>* stored = nullptr);
    // true: updateFeaturesInformation decides the frame's deletions in a walk without device calls (same tests, same traversal, same counters) and lets them
    // leave together through deleteFeatures.  false (default): one deleteOneFeature per landmark inside the walk, as the reference
    bool   deleteTogether = false;

    // ---- data association on the device ----------------------------------------------------------------
    // the appearance fields of PointsMap the reference fills at creation (SLAM.cpp:920-925): initPatch = the 21 x 21 gray
    // window around cvRound(initPixel) (row-major), initRotation = Rwc, initTrans = camera position
    bool setFeatureAppearance(int id, const unsigned char* initPatch, const double initRotation[9], const double initTrans[3], const double initPixel[2]);
    // wrapPatch() + dataAssociation() (SLAM.cpp:1803-2009) for the current gray frame (image_h x image_w uchar): fills
    // isMatching / matchLocation / nMatchTimes of every map entry and m_nMatches.  Install it as the association step:
    //   SLAM.dataAssociation = [&](monoslam::CSLAM& s) { s.dataAssociationOnDevice(grabGrayFrame()); };
    bool dataAssociationOnDevice(const unsigned char* gray);
    // the same on the frame the handle holds (after loadPictures): srukf_associate_held, no upload
    bool dataAssociationOnDeviceHeld();
    // ---- ambiguity veto and sub-pixel matches (opt-in).  With either switch on, the two calls above go through srukf_associate_checked, which keeps
    //      every candidate's correlation.  rejectAmbiguousMatches: a landmark whose second peak (a local maximum more than AMBIGUITY_EXCLUSION pixels, Chebyshev,
    //      from the best) reaches AMBIGUITY_RATIO times the best is not matched this frame: isMatching = false, isAmbiguous = true, not in m_nMatches.
    //      KalmanUpdate therefore does not count it in nMatchTimes, and the reference's own deletion policy (nPredictTimes > 2 nMatchTimes with >= 10 predictions,
    //      updateFeaturesInformation) retires a landmark that stays ambiguous.  subpixelMatches: matchLocation = the integer peak + the offset of the parabola
    //      through its 4-neighbours, WITHOUT the fraction of the prediction the reference adds (1991-1992); alone, it passes ratio 2.0 (no veto).
    //      The defaults 0.9 and 4 are reasoned, not tuned (4 = half the template's half-width).  With both switches off none of this runs
    bool   rejectAmbiguousMatches = false;
    double AMBIGUITY_RATIO = 0.9;
    int    AMBIGUITY_EXCLUSION = 4;
    bool   subpixelMatches = false;
    int    m_nAmbiguous = 0, m_nAmbiguousTotal = 0;            // landmarks vetoed in this frame's association / since initializeParameters
    std::vector<int> m_ambiguousID;                            // their IDs, in state order at the time of the association (later deletions do not touch the list)

    // ---- colour-frame intake and the 2-D feature overlay.  SLAM() calls none of them by itself ------------------------------------
    // loadPictures (SLAM.cpp:529-543): bgr = the image_h x image_w x 3 colour frame (B, G, R interleaved, as cvLoadImage / cvQueryFrame deliver it) goes to the
    // device (srukf_set_frame_bgr); m_gryImage then points at m_grayStore, its conversion as the reference converts it (CV_RGB2GRAY on B, G, R data: the blue
    // byte gets 0.299).  Hosts that set m_gryImage themselves need not call it
    bool loadPictures(const unsigned char* bgr);
    std::vector<unsigned char> m_grayStore;
    // display2DFeatureModel + draw2DEllipse (3009-3083): m_srcImage (image_h x image_w x 3, B, G, R) = the held frame with the predicted cross (blue), the matched
    // cross and the chi-square ellipse of Si^T Si (red) of every map node with isMatching, from predictLocation / Si / matchLocation (srukf_render_overlay; the ID
    // text is not drawn)
    bool display2DFeatureModel();
    std::vector<unsigned char> m_srcImage;

    // ---- display accessors (what OpenGlDisplay.cpp:449-583 reads per paint) ------------------------------
    // updateFeaturesInformation (SLAM.cpp:2397-2621), as SLAM() calls it after KalmanUpdate: the deletion policy (2443-2460:
    // nPredictTimes > 2 nMatchTimes with >= 10 predictions, rho < 0.01, Hlr_z < 0, predicted or matched pixel within
    // DIST_2_BORDER of the image border) -> deleteOneFeature, landmarks that leave while matched are archived in
    // m_featuresAllInfo (2516-2532); the landmarks that stay get xyz / axis / sigma refreshed (2566-2580) and isVisible
    // cleared (2598).  The loop keeps the reference's traversal: the node that moves into a deleted node's place is not
    // examined in the same call (2554-2570, 2607-2615).
    bool updateFeaturesInformation();
    // the display part alone (2566-2580): xyz, cov, axis, sigma of every landmark of `map`, from ONE device call
    // (srukf_get_landmarks_cartesian) instead of a pass over the n x n m_P_k per landmark
    bool refreshFeaturesDisplay(bool withMirrors = false);   // withMirrors: m_X_k and the robot block of m_P_k in the same device round trip
    // getFeatureCartesianInformation (2721-2751): xyz and cov (3x3) of landmark id from the last refresh; sr (the 6x6
    // diagonal block of m_S_k) only when fullCovariance mirrors are on, otherwise left empty
    void getFeatureCartesianInformation(Point3d& xyz, Mat& sr, Mat& cov, const int& id) const;
    // get3DdisplayInformation (2791-2802), calculateEigenvaluesAndEigenvectors (2816-2891: classical Jacobi rotations,
    // largest off-diagonal pivot, eigenvalues left on the diagonal in place), matrix2Quaternion (2902-2948)
    void get3DdisplayInformation(Quaternion& axis, Point3d& sigma, const Mat& matrix) const;
    bool calculateEigenvaluesAndEigenvectors(const Mat& src, Mat& eigenvalues, Mat& eigenvectors) const;
    void matrix2Quaternion(Quaternion& quaternion, const Mat& matrix) const;

    // the reference's loadPictures()+dataAssociation() slot (SLAM.cpp:95-97)
    std::function<void(CSLAM&)> dataAssociation;
    // the reference's addFeatures() -> detectAndfilteringFeatures / insureEnoughFeatures slot (SLAM.cpp:552-562, 574-808):
    // the host detects key points on its current image and returns them as (u, v) pairs (distorted pixels); the facade
    // joint-initialises them (integrateFeaturesInformation).  Used by the redirection restart of predictMotion.
    std::function<int(CSLAM&, std::vector<double>& keyPoints)> addFeatures;
    // ---- finding new landmarks on the device (addFeatures 552-562) --------------------------------------------------------------------------
    // With m_gryImage set and no addFeatures callback installed, SLAM() and the redirection restart detect on the device: detectAndfilteringFeatures,
    // insureEnoughFeatures, then integrateFeaturesInformation for the accepted key points and srukf_capture_appearance for the new landmarks
    // (initPatch / initRotation / initTrans, 918-926).  Loop points are reported (m_loopPointID, m_loopPointCounter); with reinsertLoopPoints on, the
    // archived landmarks an isAdding pass met again go back into the filter in front of the new key points (isLoop nodes).  m_nMapFeatures stays the
    // true map size.
    const unsigned char* m_gryImage = nullptr;          // the current gray frame, image_h x image_w, row-major (SLAM.h: m_gryImage); set by the host
    int    m_blockSize = 3;                             // SLAM.cpp:175
    double m_qualityLevel = 0.1;                        // 176
    int    m_nInitialRaws = 8, m_nProcessRaws = 8;      // 177-178: corner budget at frame 1 / isAdding, otherwise
    double m_minDist = 15.0, m_minDist2 = 225.0;        // 180-181
    std::vector<Point2d> m_keyPoints;                   // the accepted key points of the last pass (SLAM.h:169)
    std::vector<int> m_loopPointID;                     // IDs of the archived features the last pass met again (SLAM.cpp:719)
    int    m_loopPointCounter = 0;                      // their number (603, 721)
    int    m_nFilters = 0;                              // key points + loop points of the last pass (758-765)
    // detectAndfilteringFeatures (574-768) on m_gryImage: GFTT + the filter pass on the device (srukf_detect_features); fills m_keyPoints, the loop
    // points and the running count the pass schedule reads
    bool detectAndfilteringFeatures();
    // insureEnoughFeatures (777-808): further passes while the running count is below m_minNUM, m_nInitialRaws += m_minNUM each, until it exceeds 30
    bool insureEnoughFeatures();
    // every pass of detectAndfilteringFeatures with its inputs, when logDetectPasses is on (hosts that check or replay detection)
    struct DetectPass {
        int call = 0, frame = 0, n_map = 0, n_matches = 0, running = 0;   // which addFeatures, m_frame.counter, true map size, m_nMatches, running count after the pass
        srukf_detect_params params{}; double pose[4] = {0, 0, 0, 0};     // the switches and the robot pose the archive was projected under
        std::vector<double> map_px, archived, uv; std::vector<int> loops;
        bool reinsertRan = false; std::vector<int> reinserted;           // (last pass of an isAdding call with reinsertLoopPoints on) the IDs put back,
        std::vector<double> reinsertedX6, reinsertedSr;                   // their archived state (6 each) and sr (36 each)
        int n_after = 0, archived_after = 0;                              // the map size and the archive size when the call returned
    };
    bool logDetectPasses = false;
    double m_detectTime = 0; int m_nDetectCalls = 0;    // wall time of the on-device addFeatures (detection passes + integration + capture) and their number
    std::vector<DetectPass> m_detectLog;
    // ---- redirection (SLAM.cpp:1354-1428): when the odometry heading jumps by more than MIN_STEP_THETA the reference
    //      archives the current map in m_featuresAllInfo and restarts a fresh 4-state filter at the current position ----
    std::vector<FeatureInfo> m_featuresAllInfo;          // SLAM.h:170
    int m_nStoreMap = 0, m_nStorePredicts = 0, m_nStoreMatches = 0, m_nShowMap = 0;   // 1408-1410, 1418

    // ---- public state, reference names (SLAM.h:154-290) -----------------------------------------
    // The reference's map is a singly linked list the host walks (`PointsMap* map_p = SLAM->map; while (NULL != map_p)
    // { ... map_p = map_p->next; }`, OpenGlDisplay.cpp:403-424, 460-509; SLAM.h:154).  Same here: `map` is the head (NULL
    // for an empty map), `next` links the nodes in state order.  The nodes live contiguously in mapStore, so map[k] is
    // also the k-th landmark; the links are rebuilt whenever landmarks are added or deleted.
    PointsMap* map = nullptr;
    std::vector<PointsMap> mapStore;
    FrameInfo m_frame;
    srukf_params m_params;               // the tunables of SLAM.cpp:172-198, 221-224, 329-337
    int    m_updateMode = SRUKF_UPDATE_BATCHED;
    int    m_nMapFeatures = 0, m_nPredicts = 0, m_nMatches = 0, m_nAddings = 0, m_odoCounter = 0, m_showCounter = 1;
    int    m_nDeletes = 0, m_nStores = 0;    // landmarks deleted / archived by the last updateFeaturesInformation (2419-2420)
    std::vector<int> m_deleteID;             // their IDs (m_deleteID, SLAM.h:278)
    int    ID = 1;                           // running landmark ID (SLAM.h:202, SLAM.cpp:248, 912)
    int    m_minNUM = 5;                     // addFeatures when fewer landmarks matched (SLAM.cpp:179, 556)
    bool   isAdding = false;                 // forces addFeatures (SLAM.cpp:268, 556)
    int    DIST_2_BORDER = 20;               // SLAM.cpp:48
    double m_frameTime = 0, m_totalTime = 0;
    std::vector<double> m_odoXY, m_path; // 2*(CAPACITY+1) each (SLAM.h:188-189)
    Mat    m_odoTheta;                   // 3 x (CAPACITY+1): index, theta, redirection flag (SLAM.cpp:235)
    Mat    m_X_k, m_S_k, m_P_k;          // host mirrors, refreshed after every frame (m_P_k: robot block only unless fullCovariance)
    bool   fullCovariance = false;       // true: m_P_k = S^T S in full (SLAM.cpp:2404), false: only the blocks the host reads
    // true: the archive sites (redirection, updateFeaturesInformation) keep each landmark's record (srukf_get_landmark_record) and an isAdding
    // addFeatures puts the loop points of its last pass back into the filter (srukf_insert_landmarks, SLAM.cpp:948-1015).
    // false (default): loop points are only reported
    bool   reinsertLoopPoints = false;
    // true (needs reinsertLoopPoints, which provides the records, and m_gryImage / a held frame): SLAM() looks for every archived landmark in the frame by
    // appearance (srukf_archive_search) after updateFeaturesInformation and before addFeatures.  The archive entries with a record and an init patch
    // are mirrored to the device when the archive changed; every matched entry goes back into the filter by the loop-point route (archived ID kept, isLoop = true,
    // archive entry erased); the geometric loop points of a detection pass are filtered by the same verdict (an entry the search of that frame did not match stays
    // archived).  The frame after, the nodes put back are looked for once more with the search's window (the ordinary association's ends at 10 px) and
    // KalmanUpdate measures those one at a time (updateReacquiredLoopNodes).  false (default): none of this runs
    bool   searchArchivedLandmarks = false;
    int    archiveSearchHalfCap = 40;                          // srukf_archive_params::half_cap, [10, 40]
    int    m_nArchiveMatches = 0, m_nArchiveRejected = 0;      // entries the searches put back / geometric loop points the searches refused, since initializeParameters
    int    m_nArchiveReacquired = 0;                           // nodes measured through the wide search the frame after they went back
    bool searchArchive();                                      // mirror, search the held frame, re-insert the matched entries
    struct ArchiveSearch { int frame = 0, n_before = 0, n_after = 0, archived_before = 0, archived_after = 0, searched = 0; std::vector<int> ids; };
    std::vector<ArchiveSearch> m_archiveLog;                   // every search that looked at records, when logDetectPasses is on: m_frame.counter, map and archive
                                                               // size around it, the records searched and the IDs put back
    bool reacquireLoopNodes();                                 // between dataAssociation and KalmanUpdate of the frame after
    bool updateReacquiredLoopNodes(bool updated);              // one srukf_update per re-acquired node, re-predicted in between (updated: an update ran this frame); jointUpdate: one joint update of all
    // true: refreshFeaturesDisplay takes axis / sigma of every map node from the device with the frame view (srukf_get_frame_view_display /
    // srukf_get_landmarks_display: k_lm_ellipsoid runs this class's Jacobi and quaternion arithmetic operation for operation, same bits)
    // instead of calling get3DdisplayInformation per landmark.  false (default): the host computes them
    bool   ellipsoidsOnDevice = false;
    bool   isRecordRobotInfo = false;
    std::string m_recordRobotDir = "RobotPath.txt";
    double MIN_STEP_X = 0.01, MIN_STEP_Y = 0.01, MIN_STEP_THETA = 45;   // SLAM.cpp:45-47
    std::string lastError;
    // wall time spent inside the map changes (integrateFeaturesInformation / deleteOneFeature: the device call and the host bookkeeping around it) and how many
    // there were: what a host that watches its frame rate under map churn wants to see (cslam_step_bench churn=P)
    double m_addTime = 0, m_deleteTime = 0; int m_nAddCalls = 0, m_nDeleteCalls = 0;
    srukf_ctx* context() const { return ctx_; }          // for srukf_debug_get / srukf_last_error next to the facade (diagnostics: the facade owns the handle)

private:
    bool redirection();
    bool addFeaturesOnDevice();
    bool associateChecked(const unsigned char* gray);
    void clearAmbiguity();
    bool recordFeature(FeatureInfo& fi, int k);
    bool reinsertLoops();
    bool reinsertEntries(const std::vector<int>& take, std::vector<int>& ids, std::vector<double>& x6s, std::vector<double>& srs);
    void relinkMap();
    void refreshMirrors();
    bool check(int rc);
    srukf_ctx* ctx_ = nullptr;
    int  slamBlock(const unsigned char* frames, int F, bool colour);      // the one body behind SLAMBlock and SLAMBlockColour
    bool displaySet_ = false;            // srukf_images_display is on on the handle (SLAMBlock switches it off again when blockDisplay goes off)
    bool rescueSet_ = false;             // srukf_images_rescue_gate is on on the handle (SLAMBlock switches it off again when rescueGateOnDevice or isUseRANSAC goes off)
    bool snapshotsSet_ = false;          // srukf_images_snapshots is on on the handle (SLAMBlock switches it off again when resumeStoppedBlocks goes off)
    bool mirrorsFresh_ = false;          // m_X_k / the robot block of m_P_k were fetched by this frame's display refresh
    int device_ = 0;
    FILE* robotFile_ = nullptr;
    double initOdo_[2] = {0, 0}, initPos_[2] = {0, 0};
    bool firstDetect_ = true;            // the reference's `static bool flag` of detectAndfilteringFeatures (590, 653-656), per facade instance
    int runningCount_ = 0;               // the reference's running m_nMapFeatures of the pass schedule (758-766, 782)
    int addCalls_ = 0;                   // addFeaturesOnDevice calls (DetectPass::call)
    std::vector<double> ransacZ_; std::vector<int> ransacM_;   // the frame's matches as KalmanUpdate gathered them (the RANSAC steps share them)
    std::vector<int> loopArchive_;       // archive indices of the loop points of the last detection pass, in the order reported
    // searchArchivedLandmarks: the IDs of the records on the device in their order there (what the last mirror sent), the IDs the last search matched, whether
    // the handle holds this frame (an association or loadPictures uploaded it), and the nodes put back last frame with their slot on the device (the records stay
    // there until the next mirror)
    std::vector<int> archiveMirror_, archiveVerdict_; bool frameHeld_ = false;
    std::vector<std::pair<int, int>> reacquire_;         // (ID, device slot)
    std::vector<int> reacquired_;                        // map indices whose match of this frame came from the wide search, in slot order
};

}  // namespace monoslam
