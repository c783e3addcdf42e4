/*
 * srukf.h — C-ABI of the MI355X-native SRUKF predict/update hot path.
 *
 * This is the drop-in boundary for ONE path of junliu111/CV-MonoSLAM: the per-frame
 * square-root unscented Kalman filter inside class CSLAM (reference MonoSLAM/SLAM.cpp,
 * MonoSLAM/SLAM.h:118-398).  The reference has no plugin/FFI interface: CSLAM is a concrete
 * class embedded by value in the MFC view (MonoSLAMView.h:44) whose methods are called and
 * whose public fields are read directly.  The entry points below are what a CSLAM facade
 * (cv-monoslam_amd/host/cslam.hpp) binds to; each one cites the reference member(s) it
 * replaces.  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *   - every function returns an int: SRUKF_OK (0) or a negative srukf_status; never aborts,
 *     never prints (the reference prints + system("pause"), SLAM.cpp:297,324,2702,3526).
 *   - one context = one filter = one HIP stream; a context is not thread-safe, independent
 *     contexts are fully concurrent (multi-GPU / Monte-Carlo model).
 *   - the caller owns every pointer it passes; nothing is retained past the call.
 *   - all matrices are row-major fp64.  State layout (SLAM.cpp:226-231,1371,2427-2435):
 *       X = [ N x (xi yi zi theta phi rho) | x y z theta ]      n = 6N+4
 *       S = n x n upper triangular, P = S^T S                   (SLAM.h:272, SLAM.cpp:2118,2404)
 *   - there is NO CPU fallback: if the HIP device/kernels are unavailable srukf_create fails
 *     with SRUKF_ERR_NO_DEVICE.
 */
#ifndef SRUKF_H_
#define SRUKF_H_

#ifdef __cplusplus
extern "C" {
#endif

#define SRUKF_ABI_VERSION 6


typedef enum srukf_status {
    SRUKF_OK                =  0,
    SRUKF_ERR_BAD_ARG       = -1,  /* NULL pointer, negative size, unknown enum            */
    SRUKF_ERR_DIM_MISMATCH  = -2,  /* sizes inconsistent with the context                  */
    SRUKF_ERR_HIP           = -3,  /* a HIP runtime call failed; see srukf_last_error      */
    SRUKF_ERR_NO_DEVICE     = -4,  /* no gfx950 device / code object not loadable          */
    SRUKF_ERR_SEQUENCE      = -5,  /* call order violated (e.g. update before predict)     */
    SRUKF_ERR_UNSUPPORTED   = -6,  /* feature outside the built hot path   */
    SRUKF_ERR_CLAMP_PENDING = -7,  /* async replay hit the GMW theta-clamp; rerun sync      */
    SRUKF_ERR_NOMEM         = -8
} srukf_status;

/* Tunables of the hot path.  Defaults = the reference's debug-model values
 * (SLAM.cpp:172-198, 221-224, 238, 241-242, 263-264, 329-337, 52, 3186). */
typedef struct srukf_params {
    double cam_dx, cam_dy;          /* 0.0028, 0.0028          SLAM.cpp:329-330 */
    double cam_cx, cam_cy;          /* 310.1129, 236.7526      SLAM.cpp:331-332 */
    double cam_k1, cam_k2;          /* 1e-4, 0                 SLAM.cpp:333-334 */
    double cam_f;                   /* 2.1735                  SLAM.cpp:335     */
    double image_w, image_h;        /* 640, 480                SLAM.cpp:312-313 */
    double a1, a2, a3, a4;          /* 8,8,8,8                 SLAM.cpp:195-198 */
    double sigma_measure;           /* 3.0 (Qt = 3*I2)         SLAM.cpp:189,238 */
    double rho0, sigma_rho;         /* 1/3, 1/6                SLAM.cpp:173,190 */
    double sigma_x, sigma_y, sigma_z, sigma_theta; /* .02 .02 .005 .02  SLAM.cpp:221-224 */
    double epsilon;                 /* 1e-13 (EPSILON)         SLAM.cpp:52      */
    double ut_alpha, ut_beta;       /* 1e-3, 2                 SLAM.cpp:263-264 */
    int    weight_type;             /* 0 (FLAG_4_WEIGHT1)      SLAM.cpp:241     */
    int    noise_type;              /* 0 (FLAG_4_NOISE1); others unsupported  SLAM.cpp:242 */
    int    newton_iters;            /* 100                     SLAM.cpp:3186    */
    int    reserved_;
} srukf_params;

/* How the square-root covariance is maintained in srukf_update.
 *  SEQUENTIAL: the reference's structure — for every matched landmark and each of its two
 *              measurement columns u:  S <- gmw(S^T S - u u^T)   (SLAM.cpp:2066-2095, 2116-2154).
 *  BATCHED   : one  S <- gmw(S^T S - U U^T)  per frame (gains do not depend on the S updates,
 *              SLAM.cpp:2070-2080; see DESIGN.md for the equivalence evidence).               */
/* SRUKF_UPDATE_JOINT: the joint measurement update (below) as a mode of the staged replay (srukf_run_frames, srukf_run_frames_async, srukf_prepare_frames_mode).  srukf_update
 * does not take it (its step-wise entry is srukf_update_joint), nor does srukf_run_frames_batch (SRUKF_ERR_UNSUPPORTED). */
typedef enum srukf_update_mode { SRUKF_UPDATE_SEQUENTIAL = 0, SRUKF_UPDATE_BATCHED = 1, SRUKF_UPDATE_JOINT = 2 } srukf_update_mode;

/* SLAM.cpp:36-37 FLAG_4_NEED_REORDER(0) / FLAG_4_NEEDNOT_REORDER(1) */
typedef enum srukf_reorder { SRUKF_NEED_REORDER = 0, SRUKF_NEEDNOT_REORDER = 1 } srukf_reorder;

/* Precision of the filter state that lives from frame to frame (arithmetic is fp64 in both).  F32 is BASELINE
 * configs[4] ("500 landmarks fp32 SRUKF ..., tolerance study"): X and S are kept as float and every frame computes
 * from exactly those rounded values. */
/* F32_MIXED adds the mixed-precision downdate of that config: the covariance that is re-factorised, S^T S - U U^T
 * (SLAM.cpp:2118-2120, 2149), is formed on the fp32 matrix pipe from the fp32 state and U^T rounded once, in K chunks of
 * <= 1024 summed in FP64; pivots, diagonal blocks and trailing updates of the modified Cholesky stay FP64.  BATCHED
 * updates only use it (a SEQUENTIAL / single-column refactor keeps the FP64 contraction).
 * Round 6: offered at every epsilon, the reference's 1e-13 included (rounds 2 - 5 refused it below 1e-9).  Its fp32 accumulators are flushed into FP64 every 32
 * rows of K, and in the rank-aware form (the default wherever a null set exists) only the kept pivots are factored and the tiles of the robot block and of the
 * map's shared anchor are formed in FP64: within ~1e-6 m of the fp64 filter over 3 000 frames at N = 500 (7.3e-7 / 1.2e-6 in two runs) (fp32 storage with FP64 arithmetic: 6.8e-7;
 * DESIGN.md, row g).  On MI355X the FP32 matrix peak is 2 x the FP64 one and the mode's extra passes use that up: it is NOT faster than SRUKF_STORAGE_F32. */
typedef enum srukf_storage { SRUKF_STORAGE_F64 = 0, SRUKF_STORAGE_F32 = 1, SRUKF_STORAGE_F32_MIXED = 2 } srukf_storage;

typedef struct srukf_ctx srukf_ctx;   /* opaque; owns all device buffers + pinned staging */

int  srukf_abi_version(void);

/* Fill *p with the reference defaults.  Replaces the constant block of
 * CSLAM::initializeParameters (SLAM.cpp:158-343). */
int  srukf_default_params(srukf_params* p);

/* Create a filter for N >= 0 landmarks (n = 6N+4) on HIP device `device`.
 * `stream` is an existing hipStream_t to launch on (so a host can time with its own events) or
 * NULL to let the context create one.  Replaces CSLAM::CSLAM + the allocation side of
 * initializeParameters (SLAM.cpp:21-57, 226-239).  Initial state: robot X=0, S=diag(sigma_x,
 * sigma_y, sigma_z, sigma_theta) in the robot block, landmark rows zero until srukf_set_state. */
int  srukf_create(srukf_ctx** out, int n_landmarks, const srukf_params* p, int device, void* stream);
int  srukf_destroy(srukf_ctx* ctx);                                  /* CSLAM::~CSLAM, SLAM.cpp:64-78      */
int  srukf_reset(srukf_ctx* ctx);                                    /* resetAllParameters, SLAM.cpp:3090-3128 */
const char* srukf_last_error(const srukf_ctx* ctx);                  /* NULL ctx -> last create() error    */

/* Upload / download the filter state (host pointers).  m_X_k / m_S_k mirrors, SLAM.h:271-272.
 * S is n*n row-major; only the upper triangle is read.  S may be NULL in get. */
int  srukf_set_state(srukf_ctx* ctx, const double* X, const double* S);
int  srukf_get_state(srukf_ctx* ctx, double* X, double* S);
/* Same, from/to DEVICE pointers on the context's device (e.g. a tensor that arrived by RCCL
 * broadcast); S_ld = row stride of the device matrix in elements (>= n). */
int  srukf_set_state_device(srukf_ctx* ctx, const double* dX, const double* dS, int S_ld);
int  srukf_get_state_device(srukf_ctx* ctx, double* dX, double* dS, int S_ld);

/* Robot pose X[n-4:n] and the 4x4 robot block of P = S^T S.  Replaces the reads at
 * SLAM.cpp:2963-2965, 3539-3556 and OpenGlDisplay.cpp:386-391 without forming the full
 * m_P_k = S^T S of SLAM.cpp:2404. */
int  srukf_get_robot(srukf_ctx* ctx, double pose4[4], double P4[16]);
/* Landmark k: its 6 state rows and the 6x6 diagonal block of P (SLAM.cpp:2427-2432, 2748). */
int  srukf_get_landmark_block(srukf_ctx* ctx, int k, double X6[6], double P66[36]);
/* getFeatureCartesianInformation (SLAM.cpp:2721-2751) for every landmark at once: xyz[3N] = anchor + m(theta, phi)/rho,
 * cov[9N] = J P66 J^T (row-major 3x3 each) with P66 the landmark's block of P = S^T S.  What the OpenGL view reads on
 * every paint (OpenGlDisplay.cpp:449-583) without ever forming the n x n P.  Either pointer may be NULL. */
int  srukf_get_landmarks_cartesian(srukf_ctx* ctx, double* xyz, double* cov);

/* What CSLAM::SLAM() refreshes for the display after every update (updateFeaturesInformation 2397-2621: m_X_k, xyz / Cartesian covariance of every landmark;
 * recordRobotInformation 3539-3556: the robot block) in ONE device round trip instead of one per accessor: X[n], xyz[3N], cov[9N], pose4[4], P4[16]; any may be NULL.
 * A host that calls it right after srukf_update gets the view exported with the status of its following updates (the call is then a copy from pinned memory; three
 * views nobody fetched end that).  Same values either way. */
int  srukf_get_frame_view(srukf_ctx* ctx, double* X, double* xyz, double* cov, double pose4[4], double P4[16]);

/* getFeatureCartesianInformation + get3DdisplayInformation (SLAM.cpp:2721-2806) for all landmarks: besides xyz / cov as above, the display ellipsoid of each
 * covariance — axis[4N], the unit quaternion (r, x, y, z) of the eigenvector matrix (matrix2Quaternion, 2903-2948), and sigma[3N], the square roots of the
 * eigenvalues in the positions the Jacobi rotations left them (calculateEigenvaluesAndEigenvectors, 2815-2892: not sorted; a negative eigenvalue gives NaN) —
 * and rot[N], the number of plane rotations applied (-1: the limit of 30 * 9 + 1 passes ran out).  The device runs the host facade's arithmetic operation for
 * operation: same bits.  Any pointer may be NULL (all of them: SRUKF_ERR_BAD_ARG).  One device round trip. */
int  srukf_get_landmarks_display(srukf_ctx* ctx, double* xyz, double* cov, double* axis, double* sigma, int* rot);
/* srukf_get_frame_view plus axis[4N], sigma[3N]: updateFeaturesInformation's display part in one round trip.  Always formed from the committed state by two
 * launches of its own (same values as srukf_get_frame_view, whose exported view and accounting it neither uses nor changes). */
int  srukf_get_frame_view_display(srukf_ctx* ctx, double* X, double* xyz, double* cov, double* axis, double* sigma,
                                  double pose4[4], double P4[16]);

/* Full covariance m_P_k = S^T S (SLAM.cpp:2404), n*n row-major, for hosts that want it. */
int  srukf_get_covariance(srukf_ctx* ctx, double* P);

/* ---- the per-frame numeric seam (CSLAM::SLAM, SLAM.cpp:87-112) -------------------------- */

/* predictMotion numeric tail (SLAM.cpp:1430-1465): control from two consecutive odometry
 * poses (x, y, theta), sigma points, motion model, re-triangularisation of S.            */
int  srukf_predict_motion(srukf_ctx* ctx, const double odo_prev[3], const double odo_cur[3]);
/* Optional look-ahead for hosts that know their odometry in advance (the reference does: loadOdometryData reads the whole file into m_odoXY / m_odoTheta
 * before the first frame, SLAM.cpp:363-496): the pair srukf_predict_motion will be called with for the NEXT frame, announced any time before this frame's
 * srukf_update.  The update's frame tail then also projects the next frame's sigma points (as the staged replay's tail does) and srukf_update submits the
 * next frame's first launch behind its own: the next srukf_predict_motion has nothing left to launch and srukf_predict_measurement only waits for the
 * statistics.  A next call whose pair differs from the announced one (or a state / map change in between) has that work ignored and projects again:
 * results never depend on the hint.  No reference counterpart (predictMotion reads m_odoXY[counter], SLAM.cpp:1444-1450). */
int  srukf_predict_motion_next(srukf_ctx* ctx, const double odo_prev[3], const double odo_cur[3]);

/* predictMeasurement (SLAM.cpp:1604-1608): h[2N] predicted pixels (m_allPredictSet),
 * Si[4N] per-landmark 2x2 upper-triangular sqrt innovation covariance (PointsMap::Si),
 * visible[N] (PointsMap::isVisible, SLAM.cpp:1727).  Outputs are host pointers, any may be NULL. */
int  srukf_predict_measurement(srukf_ctx* ctx, double* h, double* Si, int* visible);

/* KalmanUpdate (SLAM.cpp:2048-2104): z[2N] matched pixels (PointsMap::matchLocation),
 * matched[N] (PointsMap::isMatching).  reorder = SRUKF_NEEDNOT_REORDER for steady state;
 * SRUKF_NEED_REORDER on the frames that follow a landmark addition (the reference passes
 * `m_nAddings != 0 ? NEED_REORDER : NEEDNOT_REORDER`, SLAM.cpp:2084-2090): the rank-aware path
 * GSLCholeskyUpdate 2122-2138 + CholeskyDecompositionWithPivoting 2158-2179 with
 * m_covRank = n - 3*K_new; K_new must have been set with srukf_set_new_landmarks
 * (SRUKF_ERR_SEQUENCE otherwise). */
int  srukf_update(srukf_ctx* ctx, const double* z, const int* matched, int reorder, int mode);

/* ---- the joint measurement update (ours: the reference has no counterpart) ----
 * srukf_update_joint: in srukf_update's place for a frame (same phase rules, same z / matched / reorder).  ONE Kalman update over all matched and visible landmarks whose Si is not singular (the reference's closed-form inverse of a singular Si is zero, 2073: no gain)
 *   with the full 2N x 2N innovation covariance
 *       Pzz = wi sum_{i not noise} dZ_i dZ_i^T + blockdiag_k(wi sum_{i in noise} dZ_i,k dZ_i,k^T),   dZ_i = Z_i - Z_0   (no centre term, as 1769-1773)
 *       Pzz = R^T R,  U^T = R^-T Pxy^T,  w = R^-T (z - h),  X += U w,  S <- gmw(S^T S - U U^T)
 *   where KalmanUpdate (2070-2080; SRUKF_UPDATE_BATCHED) takes every landmark's gain from the same prior with that landmark's own 2 x 2 Si and adds them, so that
 *   landmarks which agree on a large innovation overshoot together.  noise = the four sigma points of the two pixel-noise directions: every landmark keeps its own
 *   pixel noise (the diagonal blocks are exactly the reference's Si^T Si; taken literally the reference's shared err components would be perfectly correlated
 *   across landmarks); the motion-noise points stay in the off-diagonal blocks.  Pxy is what SRUKF_UPDATE_BATCHED forms from the single prior.  With one active
 *   landmark the call equals srukf_update(BATCHED) for that landmark.  The refactorisation is srukf_update's own (theta check, exact path behind it;
 *   SRUKF_NEED_REORDER as there).  No match: no-op (2050-2051).  Runs on the step-wise path's slow form (a frame predicted on the fast path is predicted again);
 *   srukf_repredict_measurement and the RANSAC calls work behind it.  SRUKF_ERR_UNSUPPORTED: SRUKF_STORAGE_F32_MIXED; or a non-positive pivot in Pzz or an innovation
 *   z - h that is not finite (inputs not finite: the state is left as predicted, srukf_last_error names the row).  srukf_clamp_info behind a SRUKF_NEEDNOT_REORDER call: (0, first flagged pivot row)
 *   when the refactorisation was flagged and went to the exact path, (-1, -1) when it was not.
 *   In the staged replay the same update is the mode SRUKF_UPDATE_JOINT of srukf_run_frames / srukf_run_frames_async / srukf_prepare_frames_mode (captured frames of its own,
 *   no host inside a block; see there); the step-wise fast path and srukf_run_frames_batch do not have it. */
int  srukf_update_joint(srukf_ctx* ctx, const double* z, const int* matched, int reorder);

/* ---- 1-point RANSAC (KalmanUpdate's isUseRANSAC branch, SLAM.cpp:2097-2103: onePointRansacHypotheses, updateLowInnovationInliers, rescueHighInnovationInliers,
 * updateHighInnovationInliers are named there and never written; isUseRANSAC / THRESHOLD_RANSAC 185-186, m_nLowInliers / m_nHighInliers SLAM.h:227-228) ----
 * srukf_ransac_consensus: between srukf_predict_measurement and srukf_update (SRUKF_ERR_SEQUENCE otherwise).  A = { k : matched[k] != 0 and visible[k] }.  Every
 *   i in A is a hypothesis — all of them, where the paper draws a random subset: the result is deterministic —: x(i) = X + K_i (z_i - h_i) with Pxy_i as
 *   calculateOneFeatureCrossCovariance forms it (2020-2038) around the predicted state and K_i = Pxy_i sii sii^T, sii = Si_i^-1 (2077-2079); the mean only.  For
 *   every j in A, d_ij = |z_j - h(x(i))_j|_2 with landmark j of x(i) projected from the robot rows of x(i) (passSigmaThroughMesaurementFunction 1615-1690, zero pixel
 *   noise); the pair is an inlier when both coordinates of that pixel are non-zero (predictMeasurement's visibility test, 1727) and d_ij < threshold (THRESHOLD_RANSAC
 *   8.0: the Euclidean pixel distance of the comment at SLAM.h:249).  votes[i] = inliers of hypothesis i (0 outside A); *best = the i with the most votes, the lowest
 *   index among equals, -1 when A is empty; inlier[j] = 1 for the inliers of *best; dist[j] = d_best,j for j in A, 0 elsewhere.  Outputs are host pointers, any may be
 *   NULL.  The call changes nothing of the filter: the srukf_update that follows returns bit for bit what it returns without it.
 *   A frame predicted on the step-wise fast path (srukf_predict_motion_next announced) keeps its motion step beside the state; there the consensus forms X, h, Si and
 *   visible once more, with the other path's launch sequence on a copy of the state before the frame, and uses THOSE: they equal what srukf_predict_measurement
 *   returned to rounding (1e-8 px; in SRUKF_STORAGE_F32 the copy is the rounded state, the predicted one is not rounded again), so a landmark whose predicted pixel
 *   lies within that of the image border could belong to A for one and not for the other.
 * srukf_repredict_measurement: after a srukf_update, in the same frame (SRUKF_ERR_SEQUENCE otherwise): predictMeasurement (1604-1608) once more from the posterior
 *   (X, S), no motion step; outputs as srukf_predict_measurement.  A second srukf_update may follow (the rescue of high-innovation inliers).  What the first update
 *   prepared for the next frame (srukf_predict_motion_next) is dropped and formed again by the next frame. */
int  srukf_ransac_consensus(srukf_ctx* ctx, const double* z, const int* matched, double threshold, int* inlier, int* votes, double* dist, int* best);
int  srukf_repredict_measurement(srukf_ctx* ctx, double* h, double* Si, int* visible);

/* m_nFilters (SLAM.cpp:826-830, 2126-2131): the number of landmarks added by the last augmentation, i.e. the LAST
 * K_new landmarks of the map.  Defines the permutation of getPermutationMatrix (SLAM.cpp:1303-1334) and the rank
 * n - 3*K_new used by SRUKF_NEED_REORDER updates.  0 clears it. */
int  srukf_set_new_landmarks(srukf_ctx* ctx, int K_new);

/* integrateFeaturesInformation, numeric part (SLAM.cpp:826-871, with passSigmaThroughMapingFunction 1177-1250,
 * QrAndCholeskyForInitilization 1260-1300, getPermutationMatrix 1303-1334): K new landmarks first seen at the
 * distorted pixels uv[K][2] (m_keyPoints[i].pt) are joint-initialised and appended to the map (inverse depth rho0,
 * sigma_rho; pixel noise sigma_measure).  The context grows to N + K landmarks in place — the handle stays valid,
 * staged sequences are dropped — and K_new = K is armed for the SRUKF_NEED_REORDER update that follows.  A context
 * created with N = 0 holds the robot block only (initializeParameters 221-231) and is the reference's frame-1 state. */
int  srukf_add_landmarks(srukf_ctx* ctx, int K, const double* uv);

/* ---- data association on the device (wrapPatch 1803-1906, dataAssociation 1915-2009, calculateCrossCorrelation
 * 3141-3166) ----
 * srukf_set_landmark_appearance: the PointsMap fields set when landmark k was created (SLAM.cpp:920-925): patch =
 *   initPatch, the 21 x 21 gray window image(Rect(cvRound(u) - 10, cvRound(v) - 10, 21, 21)) row-major; R = initRotation
 *   (Rwc, 3x3 row-major); t = initTrans (camera position); px = initPixel (distorted).  Records follow their landmark
 *   through srukf_add_landmarks / srukf_delete_landmark.
 * srukf_associate: between srukf_predict_measurement and srukf_update.  gray = the image_h x image_w frame (uchar,
 *   row-major).  Warps every init patch to the current pose (matchPatch, persistent as in the reference) and searches
 *   the chi-square gated window around the predicted pixel for the best normalised cross correlation; a landmark
 *   matches when it exceeds THRESHOLD_MATCH_PATCH = 0.8.  Out (host, any may be NULL): z[2N] matchLocation,
 *   matched[N] isMatching, corr[N] the best correlation.
 * srukf_get_match_patch: the 17 x 17 matchPatch of landmark k (row-major, 289 bytes). */
int  srukf_set_landmark_appearance(srukf_ctx* ctx, int k, const unsigned char* patch, const double R[9], const double t[3], const double px[2]);
int  srukf_associate(srukf_ctx* ctx, const unsigned char* gray, double* z, int* matched, double* corr);
int  srukf_get_match_patch(srukf_ctx* ctx, int k, unsigned char* out);

/* ---- finding new landmarks on the device (addFeatures 552-562: detectAndfilteringFeatures 574-768, integrateFeaturesInformation 918-926) ----
 * srukf_detect_features: Shi-Tomasi "good features to track" as OpenCV 2.4's goodFeaturesToTrack(gray, max_corners, quality_level, min_dist,
 *   no mask, block_size, useHarris = false) computes it (GoodFeaturesToTrackDetector, SLAM.cpp:599-600), then the reference's filter pass over
 *   its key points in order.  One change makes it exactly reproducible: the 3x3 Sobel gradients and their block x block box sums are exact
 *   integers (BORDER_REFLECT_101 on the frame and on the product maps) and the response r = 0.5 ((A + C) - sqrt((A - C)^2 + 4 B^2)) is fp64
 *   with a correctly rounded sqrt (OpenCV's cornerMinEigenVal is r / (4 block_size 255)^2: the same ranking).  block_size 3 or 5, otherwise
 *   SRUKF_ERR_UNSUPPORTED.  Candidates: 1 <= x <= w - 2, 1 <= y <= h - 2, r > quality_level r_max, r = the 3x3 maximum of the thresholded map
 *   (plateaus all kept); sorted by r descending, EQUAL r IN ASCENDING RASTER ORDER y w + x (std::sort leaves ties unspecified: this rule is
 *   ours); greedy: rejected when dx^2 + dy^2 < min_dist^2 to a corner accepted before (no test when min_dist < 1); at most max_corners
 *   (<= 0: no limit but uv_cap).  Key points are integer (x = column, y = row).  The filter pass (SLAM.cpp:647-752), per key point:
 *     border     DIST_2_BORDER <= x <= w - DIST_2_BORDER, the same for y, or it is dropped;
 *     unfiltered accept (frame 1 / the first call: the `static flag` of 590, 653-656);
 *     map veto   (map_gate: m_nMatches != 0, 660) map_px[4 n_map] = (matchLocation.x, .y, predictLocation.x, .y) per map entry: rejected when
 *                any entry has a zero among its four values (the isThereNoZero else branch, 690-693) or an all-nonzero entry lies within
 *                min_dist^2 on either location;
 *     archived   archived_state6[6 n_archived] = FeatureInfo::state of m_featuresAllInfo: with project_archived (isAdding) projected under
 *                the context's current robot pose (srukf_project, zero pixel error), otherwise at (0, 0) (the zeroed pixelPos, 614-635); every
 *                archived pixel within min_dist^2 rejects the key point and is reported as a loop point (key point index in GFTT order,
 *                archived index), all of them (no break, 726);
 *     pairwise   rejected within min_dist^2 of a key point accepted before in this call (731-750).
 *   gray = the image_h x image_w frame, or NULL for the frame the handle holds (the last one passed to srukf_associate / srukf_detect_features /
 *   srukf_capture_appearance; it survives map changes, srukf_reset drops it): SRUKF_ERR_SEQUENCE when it holds none.  uv_out[2 uv_cap] receives
 *   the accepted key points, *n_uv their number; loop_out[2 loop_cap] the loop points in the order the reference records them (719-723), *n_loop
 *   their number (either pointer pair may be NULL / 0: what does not fit is counted, not written).  The scratch is allocated on the first call.
 *   Loop points are reported, not added by this call: the caller integrates the *n_uv key points and may put the archived landmarks back
 *   with srukf_insert_landmarks.
 * srukf_capture_appearance: integrateFeaturesInformation's appearance fields (918-926) for landmarks [first, first + K) on the device: initPatch
 *   = the 21 x 21 window of gray (NULL: the held frame) at cvRound(uv) (round half to even), initRotation = Rwc of the current heading
 *   (getTransferMatrix 1031-1037), initTrans = the robot x, y, z (834-836), initPixel = uv (the pixels passed to srukf_add_landmarks), matchPatch
 *   zeroed.  Byte for byte what srukf_set_landmark_appearance records for a host-cut patch.  SRUKF_ERR_BAD_ARG when a window leaves the image. */
typedef struct srukf_detect_params {
    int    max_corners;       /* m_nInitialRaws at frame 1 / isAdding, m_nProcessRaws otherwise: 8 and 8      SLAM.cpp:177-178, 590-599 */
    double quality_level;     /* m_qualityLevel 0.1                                                          SLAM.cpp:176 */
    double min_dist;          /* m_minDist 15.0 (m_minDist2 = min_dist^2)                                    SLAM.cpp:180-181 */
    int    block_size;        /* m_blockSize 3 (3 or 5 supported)                                            SLAM.cpp:175 */
    double dist_to_border;    /* DIST_2_BORDER 20.0                                                          SLAM.cpp:48 */
    int    unfiltered;        /* 1 == m_frame.counter || the first call (static flag)                        SLAM.cpp:590, 653 */
    int    map_gate;          /* 0 != m_nMatches                                                             SLAM.cpp:660 */
    int    project_archived;  /* isAdding: archived features projected under the current pose               SLAM.cpp:614-635 */
} srukf_detect_params;
int  srukf_detect_features(srukf_ctx* ctx, const unsigned char* gray, const srukf_detect_params* params, int n_map, const double* map_px,
                           int n_archived, const double* archived_state6, double* uv_out, int uv_cap, int* n_uv,
                           int* loop_out, int loop_cap, int* n_loop);
int  srukf_capture_appearance(srukf_ctx* ctx, int first, int K, const double* uv, const unsigned char* gray);

/* ---- colour-frame intake and the 2-D feature overlay (loadPictures 529-543; display2DFeatureModel 3009-3051, draw2DEllipse 3067-3083) ----
 * srukf_set_frame_bgr: loadPictures (529-543).  bgr = the image_h x image_w x 3 colour frame, interleaved B, G, R bytes, row-major, no row padding (what
 *   cvLoadImage / cvQueryFrame deliver).  It is uploaded, converted into the held gray frame as the reference converts it — cvCvtColor(CV_RGB2GRAY) on B, G, R
 *   data, so with c0, c1, c2 a pixel's bytes in memory order gray = (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14 (OpenCV 2.4's fixed-point weights: the BLUE
 *   byte gets red's 0.299) — and kept on the handle beside it.  gray_out (NULL ok) receives the image_h x image_w gray bytes.  The held frame is then what
 *   srukf_associate_held, srukf_detect_features(gray = NULL) and srukf_capture_appearance(gray = NULL) read.  The colour frame survives map changes as the gray
 *   one does; srukf_reset drops both; a later call that passes a gray frame replaces the gray one and invalidates the colour one.
 * srukf_associate_held: srukf_associate (wrapPatch + dataAssociation, 1803-2009) on the held frame, no upload.  SRUKF_ERR_SEQUENCE before
 *   srukf_predict_measurement or when no frame is held.
 * srukf_render_overlay: display2DFeatureModel (3009-3051) with draw2DEllipse (3067-3083) into out_bgr[image_h x image_w x 3]: the held colour frame (the held
 *   gray byte three times when no colour frame is held) with, for every landmark k of the context's N with matched[k] != 0 and finite h, z of magnitude below
 *   2^30, in state order, later over earlier: the predicted cross at cvRound(h) in B, G, R = (255, 0, 0) (3035-3036), the matched cross at cvRound(z) in
 *   (0, 0, 255) (3040-3041), the chi-square ellipse of Pi = Si^T Si (3031) around cvRound(z) in (0, 0, 255) (3042).  Our raster rules (OpenCV's line and
 *   ellipse polygons are not reproducible outside it): a cross is |dx| <= 10 && |dy| <= 1 or |dy| <= 10 && |dx| <= 1; the ellipse has the integer semi-axes
 *   a = max(1, (int)(sqrt(l0) sqrt(5.99146454710798))), b likewise from l1 (3076-3079), l0 >= l1 the eigenvalues of Pi in closed form, (c, s) the unit
 *   eigenvector of l0, and with p = c dx + s dy, q = c dy - s dx a pixel is painted when (p/(a+1))^2 + (q/(b+1))^2 <= 1 and not (a >= 2 && b >= 2 &&
 *   (p/(a-1))^2 + (q/(b-1))^2 <= 1).  No ellipse when l0 is not finite or >= 1e12 (eigen fails, 3073).  The ID text (cvPutText, 3034, 3039) is not drawn.
 *   h[2N], Si[4N] (row-major 2 x 2), z[2N], matched[N] are the caller's (host; NULL allowed when N = 0): the call reads and writes nothing of the filter, is
 *   valid in any phase and changes no later result.  SRUKF_ERR_SEQUENCE when no frame is held. */
int  srukf_set_frame_bgr(srukf_ctx* ctx, const unsigned char* bgr, unsigned char* gray_out);
int  srukf_associate_held(srukf_ctx* ctx, double* z, int* matched, double* corr);
int  srukf_render_overlay(srukf_ctx* ctx, const double* h, const double* Si, const double* z, const int* matched, unsigned char* out_bgr);

/* ---- association that rejects ambiguous matches and refines matches to sub-pixel (opt-in) ----
 * srukf_associate_checked: srukf_associate (gray != NULL) / srukf_associate_held (gray == NULL) with every candidate's score kept.  Same phase rule, same launches
 *   (k_associate_checked in k_associate's place), one export and one wait: matchPatch evolves identically whichever call a frame uses.  Per landmark, with s[c] the
 *   normalised cross correlation of candidate c (row-major over the wx x wy window; 0 for a candidate the border test or the chi-square gate skips):
 *     best       the first maximum in row-major order, as srukf_associate finds it; corr = s[best]; raw = corr > corr_threshold;
 *     rival      (only when raw) a candidate with Chebyshev distance > exclusion from best, s > 0 and s >= every neighbour of the window at Chebyshev distance 1
 *                (plateaus count; gated neighbours count with their 0); corr2 = the largest rival score, first in row-major order among equals, z2 = its location
 *                by the reference's formula (1991-1992); both 0 without a rival;
 *     ambiguous  raw && corr2 >= ratio * corr (a ratio > 1 never vetoes: corr2 <= corr);
 *     flags[k]   bit 0 raw, bit 1 ambiguous, bit 2 sub-pixel refinement applied;  matched[k] = raw && !ambiguous;
 *     z[k]       the best's location whenever raw (also when vetoed), (0, 0) otherwise.  subpixel == 0: the reference's form, integer offset + h (1991-1992).
 *                subpixel != 0: the integer centre ((int)h.x - half_x + bx, (int)h.y - half_y + by) plus (dx, dy) — this mode deliberately DROPS the reference's
 *                + frac(h): a refinement on top of an arbitrary fractional offset means nothing.  dx = dy = 0 unless best is off the window's edge and its four
 *                4-neighbours all score > 0 (then bit 2): den = (sL - 2 s0) + sR, dx = den < 0 ? (0.5 (sL - sR)) / den : 0, clamped to [-0.5, 0.5]; dy likewise
 *                from the upper and lower neighbours.
 *   A landmark that is not visible or has no appearance record gets all outputs zero.  params == NULL: { 0.8, 0.9, 4, 0 }.  Any output pointer may be NULL.
 *   SRUKF_ERR_BAD_ARG: ratio not finite or <= 0, exclusion outside [1, 20], corr_threshold not finite.  SRUKF_ERR_SEQUENCE: as srukf_associate / _held.
 * srukf_get_match_scores: the map the last srukf_associate_checked left for landmark k: out[wx * wy] row-major, (x0, y0) the pixel of the window's top-left
 *   candidate centre (wx = wy = 0 for a landmark that was not searched).  SRUKF_ERR_SEQUENCE when there is none (no checked call yet, or a map change or
 *   srukf_reset since). */
typedef struct srukf_match_params {
    double corr_threshold;    /* THRESHOLD_MATCH_PATCH 0.8                                                    SLAM.cpp:1989 */
    double ratio;             /* 0.9: a second peak within 10 % of the best vetoes the match */
    int    exclusion;         /* 4: half the template's half-width — nearer maxima share most of their 289 pixels with the best's patch */
    int    subpixel;          /* 0 */
} srukf_match_params;
int  srukf_associate_checked(srukf_ctx* ctx, const unsigned char* gray, const srukf_match_params* params,
                             double* z, int* matched, double* corr, double* corr2, double* z2, int* flags);
int  srukf_get_match_scores(srukf_ctx* ctx, int k, double out[441], int* wx, int* wy, int* x0, int* y0);

/* ---- loop points: archived landmarks put back into the filter (the redirection archive, SLAM.cpp:1357-1378, 2516-2532; integrateFeaturesInformation's
 * isLoop branch, 948-1015) ----
 * srukf_get_landmark_record: what an archived landmark takes along, in one device round trip.  X6 = rows 6k .. 6k+5 of X; S66 = the upper Cholesky
 *   factor of the landmark's MARGINAL block P66 = (S^T S)[6k:6k+6, 6k:6k+6] (the P66 of srukf_get_landmark_block), with eps = params.epsilon and
 *   sums in ascending m: d_j = max(eps, P_jj - sum_{m<j} S_mj^2), S_jj = sqrt(d_j), S_ji = (P_ji - sum_{m<j} S_mj S_mi) / S_jj for i > j, zeros
 *   below the diagonal (row-major).  patch[441] / R[9] / t[3] / px[2] = the landmark's appearance record as srukf_set_landmark_appearance or
 *   srukf_capture_appearance left it; *has_app = 0 (and zeros) when it has none.  Any output pointer may be NULL.
 * srukf_insert_landmarks: L landmarks with means X6[6L] and upper-triangular square-root blocks S66[36L] (row-major) and no cross-covariance enter the
 *   state at landmark positions [N - K_new, N - K_new + L): after the older landmarks, before the K_new landmarks the last srukf_add_landmarks armed
 *   (which stay the last K_new; K_new is unchanged) and the robot block.  X and S are copied, no arithmetic: P' = Pi (P (+) S66_0^T S66_0 (+) ...) Pi^T.
 *   The context grows in place like srukf_add_landmarks (staged sequences are dropped).  Old landmarks keep their appearance records; the new ones get
 *   patches[441 L] / R[9L] / t[3L] / px[2L] (matchPatch zeroed), or with patches == NULL no record (they never match in srukf_associate).
 *   SRUKF_ERR_BAD_ARG: L < 1, a non-finite input, a nonzero entry below the diagonal of an S66, patches without R, t and px. */
int  srukf_get_landmark_record(srukf_ctx* ctx, int k, double X6[6], double S66[36], unsigned char* patch, double R[9], double t[3], double px[2], int* has_app);
int  srukf_insert_landmarks(srukf_ctx* ctx, int L, const double* X6, const double* S66, const unsigned char* patches, const double* R, const double* t,
                            const double* px);

/* ---- archived landmarks found in the frame by appearance (no reference counterpart: the reference meets an archived landmark again only when a
 * corner of a detection pass lies within m_minDist of its projected mean, SLAM.cpp:699-727) ----
 * srukf_archive_set: the archive the search covers, on the handle: it survives map changes as the held frame does, srukf_reset and srukf_destroy drop it.  The call
 *   replaces the whole archive; L = 0 clears it.  Layouts as srukf_insert_landmarks: X6[6L], S66[36L] (row-major upper triangular), patches[441L], R[9L], t[3L],
 *   px[2L]; every record has an appearance (the caller leaves the others out).  SRUKF_ERR_BAD_ARG: L < 0, a non-finite number, a nonzero entry below the diagonal
 *   of an S66, a NULL array with L > 0; such a call leaves the archive as it was.  A call that fails with SRUKF_ERR_NOMEM or SRUKF_ERR_HIP leaves it empty.
 *   srukf_archive_count: L.
 * srukf_archive_search: valid in any phase; gray = the image_h x image_w frame, or NULL for the held one (SRUKF_ERR_SEQUENCE when none is held).  params NULL:
 *   half_cap 40, corr_threshold 0.8 (THRESHOLD_MATCH_PATCH), chi2 5.99146454710798.  SRUKF_ERR_BAD_ARG: half_cap outside [10, 40], chi2 not a finite number > 0,
 *   corr_threshold not finite.  Outputs (host, any may be NULL):
 *   h[2L], Si[4L], visible[L], z[2L], matched[L], corr[L].  The robot pose and its 4 x 4 covariance P4 are what srukf_get_robot returns at that moment.  Per record j:
 *   (a) the unscented transform over the 12-vector [record 6 | robot 4 | pixel noise 2] with the weights of Na = 12 (weight type 0: wm0 = -3, wi = 1/6, gamma =
 *       sqrt 3) and S_aug = blockdiag(S66_j, S_rr, sigma_measure I2), S_rr the upper Cholesky factor of P4 by srukf_get_landmark_record's rule.  Sigma points
 *       mu, mu + gamma row_i, mu - gamma row_i (25), each through the device's projection (the one srukf_project_host runs) with its two noise entries as the
 *       pixel error: Z_0 .. Z_24.  h = wm0 Z_0 + wi sum_{i>=1} Z_i;  Pi = wi sum_{i>=1} (Z_i - Z_0)(Z_i - Z_0)^T (deviations from the centre point, no centre
 *       term: predictMeasurement's form, 1769-1773);  Si = the upper Cholesky factor of Pi by the same rule;  visible = both coordinates of all 25 pixels >= 1:
 *       a sigma point outside the projection's validity border has its undistorted pixel zeroed, which the distortion maps to a fraction of a pixel from the origin,
 *       and such a point would drag the mean (stricter than the reference's test of the mean, 1727).  The threshold 1 assumes what holds for any usable camera
 *       model here: a valid pixel (>= 10 px inside the image) is moved by the distortion by less than 9 px, and the image of the zeroed pixel, c (1 - 1/d) per
 *       coordinate with c the principal point and d the distortion factor at the origin, stays below 1 px (0.037, 0.028 with the default intrinsics).  Sums in
 *       ascending sigma index.
 *   (b) wrapPatch (1803-1906) of every visible record under the current pose around h, with the record's Cartesian mean (x + cos phi sin theta / rho, y - sin phi /
 *       rho, z + cos phi cos theta / rho), into the archive's template buffer, which is zeroed at the start of every search.  srukf_archive_get_template returns the
 *       17 x 17 template of record j (zeros before any search, for records not visible, and where the warp leaves the init patch).
 *   (c) the search.  Pi = Si^T Si; half_x = clamp(ceil(sqrt(chi2 Pi00)), 8, half_cap), half_y from Pi11; candidate centres (i, j) = ((int)h_x - half_x + c % wx,
 *       (int)h_y - half_y + c / wx), c row-major over wx x wy = (2 half_x + 1) x (2 half_y + 1).  A candidate scores 0 when its 17 x 17 patch leaves the image or
 *       e^T Pi^-1 e >= chi2, e = (i - h_x, j - h_y) (closed-form 2 x 2 inverse).  Otherwise, with v the frame bytes, t the template bytes, NP = 289 and exact integer
 *       sums, A = NP sum vt - sum v sum t, B = NP sum v^2 - (sum v)^2, C = NP sum t^2 - (sum t)^2: score = (B == 0 || C == 0) ? 0 : (double)A / sqrt((double)B *
 *       (double)C) — the normalised cross correlation of calculateCrossCorrelation (3141-3166) without its rounding.  corr = the maximum score, the first one in
 *       row-major order; matched = corr > corr_threshold; z = that centre (integers), (0, 0) when not matched.  Not visible: matched 0, corr 0, z (0, 0).
 *   The call writes nothing the filter reads: every later result of the filter is bit for bit what it is without the call, in any phase, and what an update
 *   submitted ahead for the next frame stays valid.  Matched records are the caller's to put back (srukf_insert_landmarks). */
typedef struct srukf_archive_params { int half_cap; double corr_threshold; double chi2; } srukf_archive_params;
int  srukf_archive_set(srukf_ctx* ctx, int L, const double* X6, const double* S66, const unsigned char* patches, const double* R, const double* t, const double* px);
int  srukf_archive_count(srukf_ctx* ctx);
int  srukf_archive_get_template(srukf_ctx* ctx, int j, unsigned char out[289]);
int  srukf_archive_search(srukf_ctx* ctx, const unsigned char* gray, const srukf_archive_params* params, double* h, double* Si, int* visible, double* z,
                          int* matched, double* corr);

/* Select the storage precision (default SRUKF_STORAGE_F64).  With SRUKF_STORAGE_F32 the state is rounded to float at
 * the end of every refactorisation (and by srukf_set_state); srukf_get_state returns those values widened to double,
 * srukf_get_state_f32 the float arrays themselves (X[n], S[n*n] row-major). */
/* How the filter shares the GPU.  No reference counterpart (the reference is single-threaded host code).
 * SRUKF_GPU_EXCLUSIVE (default, any value other than the two below): this filter has the GPU to itself while it runs; the
 *   refactorisation is ONE persistent launch that may use every CU and whose workgroups all have to be resident.
 * SRUKF_GPU_SHARED: several filters replay concurrently on this GPU (one context and stream each).  The persistent launch keeps
 *   to half the CUs and starts behind an admission gate that lets at most two such launches of the process run at a time, so
 *   the launches that run together are always resident together (measured at N = 200: one filter 4 500 frames/s, two 8 000,
 *   three 10 600 aggregate).  Each filter's stream should have a hardware queue of its own: the ROCm runtime maps streams onto
 *   GPU_MAX_HW_QUEUES = 4 queues by default, and streams that share one serialise — export GPU_MAX_HW_QUEUES=8 before the process
 *   initialises HIP when it holds more than four streams.
 * SRUKF_GPU_SHARED_PER_PANEL: one launch per 64-row panel, no residency assumption at all (other kernels of unknown size and
 *   duration on the GPU).  A persistent launch that cannot get its workgroups in time gives up (bounded waits), its frame is
 *   repeated on the exact path, and the context switches to this mode by itself. */
#define SRUKF_GPU_SHARED 0
#define SRUKF_GPU_EXCLUSIVE 1
#define SRUKF_GPU_SHARED_PER_PANEL 2
int  srukf_set_exclusive(srukf_ctx* ctx, int exclusive);
/* Rank-aware refactorisation (default on).  The anchors of landmarks initialised in one batch are copies of one robot
 * position (SLAM.cpp:1223, 1247) and stay identical random variables for the life of the filter, so 3 (K - 1) pivots per
 * batch are null by construction: the reference's modified Cholesky meets them as c_jj = 0 and clamps them to EPSILON
 * (SLAM.cpp:2279-2285).  Whenever a state arrives (srukf_set_state*, map changes) the rows of S with energy < 1e-12 are
 * taken as such directions; the refactorisation then pivots only the others (same relative order: the kept rows are the
 * reference's rows) and writes sqrt(EPSILON) e_k for the rest, which changes no entry of P = S^T S by more than 1e-12.
 * Every frame verifies that the skipped directions are still null in its S^T S - U U^T and otherwise takes the exact path.
 * srukf_null_directions: how many pivots are skipped at present.  No reference counterpart. */
int  srukf_set_rank_aware(srukf_ctx* ctx, int on);
int  srukf_null_directions(srukf_ctx* ctx);
int  srukf_set_storage(srukf_ctx* ctx, int storage);
int  srukf_get_state_f32(srukf_ctx* ctx, float* X, float* S);

/* deleteOneFeature, numeric part (SLAM.cpp:2637-2668): landmark `id` (0-based position in the state) leaves the map:
 * X and S lose its 6 entries / rows / columns and the removed rows are folded back in (GSLCholeskyUpdate with
 * FLAG_4_UPDATING), i.e. S becomes the factor of the remaining block of P = S^T S.  The context shrinks to N - 1
 * landmarks in place. */
int  srukf_delete_landmark(srukf_ctx* ctx, int id);
/* K landmarks leave in one call: ids[K] are distinct 0-based positions in the current state, in any order.  X' = X[keep] with the kept landmarks in their
 * old order, S' = the upper factor of (S^T S)[keep, keep] — what K calls of srukf_delete_landmark rebuild, in any order, by one product, one compaction
 * and one factorisation.  The context shrinks to N - K landmarks in place, once (K = N leaves the robot block); of the landmarks the last srukf_add_landmarks
 * armed, the ones with ids >= N - K_new leave K_new too.  srukf_delete_landmark(ctx, id) is the K = 1 call.
 * records_X6 [K][6], records_S66 [K][36], patches [K][441], R [K][9], t [K][3], px [K][2], has_app [K] (each may be NULL): entry q holds what
 * srukf_get_landmark_record(ctx, ids[q], ...) returns on the state before the call, byte for byte; all K arrive in one device round trip.
 * SRUKF_ERR_BAD_ARG, with the handle left as it was: a NULL handle, K < 1, NULL ids, an id outside [0, N), an id named twice. */
int  srukf_delete_landmarks(srukf_ctx* ctx, int K, const int* ids, double* records_X6, double* records_S66,
                            unsigned char* patches, double* R, double* t, double* px, int* has_app);

/* ---- benchmark seam: whole frames with inputs pre-staged in HBM --------------------------- */

/* Stage F frames of inputs on the device: odo[(F+1)*3] odometry poses (frame f uses f, f+1),
 * z[F*2N] measurements, matched[F*N].  Host pointers. */
int  srukf_stage_sequence(srukf_ctx* ctx, int n_frames, const double* odo, const double* z, const int* matched);
/* Run frames [first, first+count) back to back (predictMotion + predictMeasurement +
 * KalmanUpdate per frame, no host round trip in between), asynchronously on the context's
 * stream.  traj, if not NULL, is a DEVICE buffer of count*8 doubles receiving per frame
 * (x, y, z, theta, P00, P01, P10, P11) — the RobotPath.txt columns of SLAM.cpp:3549-3556.
 * mode: SRUKF_UPDATE_BATCHED, or SRUKF_UPDATE_JOINT: every frame's update is the joint measurement update (srukf_update_joint's) on the plain frame form
 *   (k_motion, k_project, k_pxy, the joint launches, the frame-tail refactorisation), whatever the launch switches say, from captured frames of its own: calls in the two
 *   modes may alternate.  SRUKF_ERR_UNSUPPORTED for SRUKF_UPDATE_SEQUENTIAL, and for JOINT in SRUKF_STORAGE_F32_MIXED (as srukf_update_joint) and in SRUKF_STORAGE_F32
 *   (the replay's frame tails round in other launches than the step-wise call's checked refactorisation; the two are not shown to round at the same points, so the mode
 *   is refused there: use srukf_update_joint). */
int  srukf_run_frames_async(srukf_ctx* ctx, int first, int count, int mode, double* d_traj);
/* Synchronous form: runs the frames, waits, and copies the trajectory to the HOST buffer traj_host[count*8] (may be
 * NULL).  Never returns SRUKF_ERR_CLAMP_PENDING: the state before the block is kept on the device, and when a frame
 * needs the reference's theta-clamp branch of the modified Cholesky (SLAM.cpp:2279-2285) the block is rewound, the
 * frames before it are replayed, that frame runs on the exact column-by-column path (as srukf_update does) and the
 * replay continues behind it (a JOINT frame repeats with the joint update in front of the checked refactorisation).  SRUKF_ERR_UNSUPPORTED from a JOINT block whose
 * inputs were not finite (srukf_synchronize, below): the state the block started from is restored. */
int  srukf_run_frames(srukf_ctx* ctx, int first, int count, int mode, double* traj_host);
/* Wait for the stream; reports SRUKF_ERR_CLAMP_PENDING if any async frame needed the reference's theta-clamp branch of
 * the modified Cholesky: the frames BEFORE the first such frame are valid, that frame and the later ones are not
 * (srukf_clamp_info names it; restore the state the block started from and use srukf_run_frames or the step-wise API).
 * SRUKF_ERR_UNSUPPORTED behind SRUKF_UPDATE_JOINT frames: a frame's innovation covariance had a non-positive pivot, or its innovation was not finite — the frame's
 * inputs were not finite.  srukf_last_error names "frame f, row r" (the first such frame); that frame kept its predicted mean and took no update, the later ones ran to
 * their end on finite data, nothing in the state is NaN: the frames before f are valid, f and the later ones are not. */
int  srukf_synchronize(srukf_ctx* ctx);
/* Optional: capture a block of `count` staged frames as ONE graph for the following srukf_run_frames_async calls with that count
 * (default: graphs of 8 frames + single frames; the device idles ~10 us between two graph launches, which shows in short blocks).
 * Nothing is executed.  1 <= count <= 512. */
int  srukf_prepare_frames(srukf_ctx* ctx, int count);
/* ... for the frames of `mode` (SRUKF_UPDATE_BATCHED: srukf_prepare_frames; SRUKF_UPDATE_JOINT): each mode keeps its own block graph. */
int  srukf_prepare_frames_mode(srukf_ctx* ctx, int count, int mode);
/* B filters (independent sequences over the same frame range: the Monte-Carlo use, MonoSLAMView.cpp:526-572 once per run) replayed
 * concurrently on one GPU: frames are issued round-robin in chunks so that the filters' launches interleave, then all are awaited;
 * filters still in SRUKF_GPU_EXCLUSIVE are switched to SRUKF_GPU_SHARED.  A filter with a flagged frame in its block is rerun
 * alone through srukf_run_frames.  ctxs[b] must have its own sequence staged (srukf_stage_sequence) and must live on the same
 * device.  traj_host: [B][count][8] or NULL; status: [B] per-filter return codes or NULL.  Returns the first error.
 * SRUKF_UPDATE_JOINT: SRUKF_ERR_UNSUPPORTED, nothing runs (srukf_last_error of every filter says so). */
int  srukf_run_frames_batch(srukf_ctx* const* ctxs, int B, int first, int count, int mode, double* traj_host, int* status);
/* First flagged staged frame / pivot row of the last SRUKF_ERR_CLAMP_PENDING (-1, -1: none).  Either may be NULL. */
int  srukf_clamp_info(srukf_ctx* ctx, int* frame, int* row);

/* ---- image runs: staged frames with the association on the device ---------------------------
 * The staged replay for a host that has the camera frames but not z / matched: every frame runs wrapPatch + dataAssociation (what srukf_associate runs, the
 * same matching front) on its own staged image, between the measurement prediction and the update, and the update reads what that wrote.  No host inside a
 * block; the map is fixed over a block; the host reads the per-frame record afterwards and applies its add / delete policy between blocks.
 * srukf_stage_images: gray[n_frames][image_h][image_w] (host) is copied to the device once.  Needs a sequence of exactly n_frames frames staged with
 *   srukf_stage_sequence (SRUKF_ERR_SEQUENCE when there is none, SRUKF_ERR_DIM_MISMATCH when the count differs or the map is empty); its odometry is used, and ITS
 *   z / matched ROWS ARE OVERWRITTEN by every image run, frame by frame, with what the association found (a later srukf_run_frames of those frames replays the
 *   association's matches, not the host's).  The images live as long as that sequence: the next srukf_stage_sequence, a map change, srukf_reset and
 *   srukf_destroy drop them.  The frame the handle holds (srukf_associate_held, srukf_set_frame_bgr) is neither read nor written by any of these calls.
 * srukf_run_images_async: frames [first, first + count) of the staged images; d_traj as in srukf_run_frames_async.  mode: SRUKF_UPDATE_BATCHED or
 *   SRUKF_UPDATE_JOINT (anything else: SRUKF_ERR_UNSUPPORTED, as srukf_run_frames_async).  SRUKF_STORAGE_F64 only (the float-stored modes: SRUKF_ERR_UNSUPPORTED).
 *   Every frame is the plain frame form (k_motion, k_project, k_pxy, then k_landmarks_cartesian, k_warp_patch, k_associate_staged, then k_gain or the joint
 *   launches, then the frame-tail refactorisation) whatever the launch switches say, from captured frames of its own per mode: an image run never replays a
 *   captured frame of srukf_run_frames_async, nor the other way round.  SRUKF_ERR_SEQUENCE: nothing staged with srukf_stage_images, or frames of
 *   srukf_run_frames_async still in flight; SRUKF_ERR_DIM_MISMATCH: frames outside the staged sequence.
 *   Flagged frames: there is no recovery inside the call.  The first image run after a srukf_synchronize keeps a checkpoint of X, S and every landmark's
 *   matchPatch (its pixels persist from frame to frame); a block is every image run up to the next srukf_synchronize.  When that srukf_synchronize finds a
 *   frame of the block flagged (SRUKF_ERR_CLAMP_PENDING; srukf_clamp_info names the frame) or a joint frame's inputs not finite (SRUKF_ERR_UNSUPPORTED, as for
 *   srukf_run_frames_async), IT restores the checkpoint before it returns: a host of the asynchronous form asks for nothing else, and runs that block
 *   step-wise (srukf_predict_motion .. srukf_associate .. srukf_update).  The record rows and the trajectory rows of the block are then not valid.
 * srukf_run_images: srukf_run_images_async + srukf_synchronize, the trajectory copied to traj_host[count*8] (may be NULL) when the block was clean.  Unlike
 *   srukf_run_frames it can return SRUKF_ERR_CLAMP_PENDING: X, S and every matchPatch are then what they were before the call.
 * srukf_get_image_matches: rows [first, first + count) of what the association wrote, after waiting for the stream (it does not collect the flags of frames in
 *   flight: srukf_synchronize still reports them): z[count][2N], matched[count][N], corr[count][N], visible[count][N] (the frame's visibility), h[count][2N] (the
 *   predicted pixels).  Any may be NULL.  Rows no image run has written hold z / matched as staged and zeros in the rest. */
int  srukf_stage_images(srukf_ctx* ctx, int n_frames, const unsigned char* gray);
int  srukf_run_images_async(srukf_ctx* ctx, int first, int count, int mode, double* d_traj);
int  srukf_run_images(srukf_ctx* ctx, int first, int count, int mode, double* traj_host);
int  srukf_get_image_matches(srukf_ctx* ctx, int first, int count, double* z, int* matched, double* corr, int* visible, double* h);

/* ---- checked image runs: the ambiguity veto and the sub-pixel peak inside an image run ----
 * srukf_run_images_checked_async / srukf_run_images_checked: srukf_run_images_async / srukf_run_images with srukf_associate_checked's association in every frame
 *   (k_associate_checked_staged in k_associate_staged's place, nothing else differs: the same frame form, the same wrapPatch, so matchPatch evolves identically
 *   whichever kind of image run a frame uses).  The reference's part is dataAssociation, SLAM.cpp:1915-2009, as for srukf_associate; the rival test, the veto and the
 *   parabola are ours (§17), with exactly the rules written out at srukf_associate_checked above: best, rival, ambiguous = raw && corr2 >= ratio * corr,
 *   matched = raw && !ambiguous, the flag bits, the two forms of z (non-zero for a vetoed landmark; without + frac(h) under subpixel), zeros for a landmark that is
 *   not visible or has no record.  The update reads that matched / z.  params == NULL: { 0.8, 0.9, 4, 0 }.  The parameters live in a small device struct written in
 *   stream order in front of each run, so one set of captured frames (their own per update mode: never a plain image run's, nor the other way round) serves every
 *   parameter value.  Plain and checked image runs may alternate inside one block; checkpoint and restore are srukf_run_images_async's.
 *   Refusals: those of srukf_run_images_async with the same codes (SEQUENTIAL and the float-stored modes SRUKF_ERR_UNSUPPORTED, nothing staged SRUKF_ERR_SEQUENCE,
 *   frames outside the stack SRUKF_ERR_DIM_MISMATCH), and SRUKF_ERR_BAD_ARG for ratio not finite or <= 0, exclusion outside [1, 20], corr_threshold not finite.
 *   Nothing runs and no state changes in any of them.
 *   Score maps: one per landmark, in the buffer of srukf_associate_checked — after a clean srukf_synchronize srukf_get_match_scores answers for the LAST frame the
 *   last checked run executed (maps are not kept per frame).  A flagged block leaves no valid map: srukf_get_match_scores then returns SRUKF_ERR_SEQUENCE.
 * srukf_get_image_checks: rows [first, first + count) of the checked record, after waiting for the stream like srukf_get_image_matches: corr2[count][N],
 *   z2[count][2N], flags[count][N].  Any may be NULL.  Rows no checked run has written are zero; a row a plain image run wrote AFTER a checked one keeps the checked
 *   run's values (the host knows which kind of run it issued for a frame).  SRUKF_ERR_SEQUENCE / SRUKF_ERR_DIM_MISMATCH as srukf_get_image_matches. */
int  srukf_run_images_checked_async(srukf_ctx* ctx, int first, int count, int mode, const srukf_match_params* params, double* d_traj);
int  srukf_run_images_checked(srukf_ctx* ctx, int first, int count, int mode, const srukf_match_params* params, double* traj_host);
int  srukf_get_image_checks(srukf_ctx* ctx, int first, int count, double* corr2, double* z2, int* flags);

/* ---- searching image runs: the archive searched by appearance behind every frame of an image run ----
 * srukf_images_search_archive: a switch on the handle, like the archive itself: it survives map changes, srukf_reset and srukf_destroy clear it.  params == NULL:
 *   { 40, 0.8, 5.99146454710798 }; the checks are srukf_archive_search's, with its messages (SRUKF_ERR_BAD_ARG: half_cap outside [10, 40], chi2 not a finite number
 *   > 0, corr_threshold not finite); a refused call changes nothing.  Valid in any phase, but not while an image run is in flight (SRUKF_ERR_SEQUENCE:
 *   srukf_synchronize first).  The call touches no device.
 *   While on, every frame of every later image run — srukf_run_images* and srukf_run_images_checked*, BATCHED and JOINT — is followed by one srukf_archive_search of
 *   the whole archive on that frame's own staged image, behind the frame's refactorisation: it sees the POSTERIOR pose and robot block, exactly what
 *   srukf_archive_search(ctx, frame_f, ..) returns between frame f's srukf_update and frame f + 1's srukf_predict_motion, bit for bit (P4 by the launch
 *   srukf_get_robot makes; stages (a), (b), (c) above, letter for letter: the two search kernels share one text).  The search writes nothing the filter reads:
 *   trajectory, X, S, the association's record and every matchPatch are bit for bit those of the run without it.  The parameters live in a small device struct
 *   written in stream order in front of each run; searching frames are captured frames of their own per kind of image run and update mode (a searching run never
 *   replays a frame captured without the search, nor the other way round), and searching and non-searching runs may alternate inside one block.  Checkpoint and
 *   restore are srukf_run_images_async's: the search owns every buffer it writes.  With the switch off an image run is exactly what it was.
 *   srukf_archive_set drops the record and the captured searching frames (both depend on L); the switch stays on and the next image run builds both for the new
 *   L.  With L = 0 a searching run is a plain one.  srukf_archive_get_template after a clean srukf_synchronize answers for the LAST frame the last searching run
 *   executed (templates are not kept per frame).
 * srukf_get_image_archive: rows [first, first + count) of the per-frame record, after waiting for the stream like srukf_get_image_matches.  *L: the archive size
 *   the rows were written with; h[count][2L], Si[count][4L], visible[count][L], z[count][2L], matched[count][L], corr[count][L] as srukf_archive_search returns them
 *   per frame; hits[count]: the number of matched records of the frame.  Any pointer may be NULL.  Rows no searching run has written are zero.  With an empty
 *   archive *L = 0 and hits are zero.  SRUKF_ERR_SEQUENCE: no images staged, no record (no searching run since the images were staged or the archive was set), or a
 *   block that srukf_synchronize found flagged and restored, until the next searching run (the rule of srukf_get_match_scores).  SRUKF_ERR_DIM_MISMATCH: rows
 *   outside the staged stack.
 * Both: SRUKF_ERR_BAD_ARG for a NULL handle (srukf_get_image_archive: first < 0, count < 1) before any device is touched. */
int  srukf_images_search_archive(srukf_ctx* ctx, int on, const srukf_archive_params* params);
int  srukf_get_image_archive(srukf_ctx* ctx, int first, int count, int* L, double* h, double* Si, int* visible, double* z, int* matched, double* corr, int* hits);

/* ---- the map policy's verdict: which frame of an image run asks for a map change ----
 * The deletion policy of CSLAM::updateFeaturesInformation (cslam.cpp:446-462; SLAM.cpp:2443-2459) and the addFeatures trigger (SLAM.cpp:556) as a read-only
 * verdict: nothing is deleted or added, the filter's data are untouched.
 * srukf_policy_state, per landmark: the counters of predictMeasurement / KalmanUpdate (cslam.cpp:713-723, 751) — visible: nPredictTimes++, predictLocation = h;
 *   not visible: predictLocation keeps its last value; matched: nMatchTimes++.
 * verdict[k], the tests of cslam.cpp:446-457 on the updated counters and the posterior X, each on its own:
 *   SRUKF_POLICY_UNMATCHED     nPredictTimes > 2 nMatchTimes && nPredictTimes >= min_predictions
 *   SRUKF_POLICY_RHO           rho < rho_min
 *   SRUKF_POLICY_BEHIND        rho (zi - X[n - 2]) + cos(phi) cos(theta) < 0
 *   SRUKF_POLICY_PRED_BORDER   predictLocation within `border` of an image edge
 *   SRUKF_POLICY_MATCH_BORDER  matched, and z within `border` of an edge
 *   SRUKF_POLICY_STORE         the landmark would be archived (isNeedStore, cslam.cpp:461-462): none of the first three, and PRED_BORDER with a match, or
 *                              MATCH_BORDER without PRED_BORDER
 *   Any of the first five bits is a deletion.  Verdicts are per landmark and independent: the reference's list walk skips the node that slides into a deleted
 *   position (cslam.cpp:475-481), which only happens in a frame that already has a deletion, so `change` is exact; the host applies the walk when it deletes.
 * srukf_policy_summary, per frame: n_predicts / n_matches as the host counts them (visible / matched landmarks), n_deletes, n_stores, n_predicts_after =
 *   n_predicts - n_deletes and n_matches_after = n_matches - n_stores (the decrements of cslam.cpp:460-462), need_add = n_matches_after < min_matches
 *   (SLAM.cpp:556), change = n_deletes > 0 || need_add.
 * srukf_map_policy (step-wise; cslam.cpp:446-462, 713-723, 751 for one frame): the kernel on the filter's current X with the caller's association — h[2N],
 *   visible[N] as srukf_predict_measurement returned them, z[2N], matched[N] as the update took them; state_inout[N] is advanced, verdict[N] and *summary are
 *   written.  params NULL: { 20, 0.01, 10, 5 } (DIST_2_BORDER, 0.01, 10, the 5 of SLAM.cpp:556).  SRUKF_ERR_BAD_ARG: a NULL pointer; border not finite or < 0,
 *   rho_min not finite, a negative count.  SRUKF_ERR_DIM_MISMATCH: an empty map.  SRUKF_ERR_SEQUENCE: staged frames in flight.
 * srukf_images_policy: a switch on the handle, like srukf_images_search_archive: it survives map changes, srukf_reset and srukf_destroy clear it; params NULL: the
 *   defaults; srukf_map_policy's parameter checks; not while an image run is in flight (SRUKF_ERR_SEQUENCE).  The call touches no device.  While on, every frame of
 *   every later image run (srukf_run_images* and srukf_run_images_checked*, BATCHED and JOINT, searching or not) is followed by the same kernel on that frame's
 *   posterior and its row of the association's record; it writes row `frame` of the policy record and advances the policy state the staged images own.  Such runs
 *   are issued as the one-frame captured graph per frame with the policy launch behind it (no captured frames of their own; the parameters live in a device struct
 *   written in stream order in front of each run, so changing one needs no recapture).  With the switch off an image run is exactly what it was.
 * srukf_images_set_policy_state (the counters map[] holds, cslam.cpp:713-723): seeds the device state from state[N].  Legal with images staged and no run pending
 *   (SRUKF_ERR_SEQUENCE otherwise).  Without it the state starts at zero.  A seed ends the block before it: srukf_images_rewind is refused until the next block.  The state lives and dies with the staged images (a map change, srukf_stage_images,
 *   srukf_stage_sequence and srukf_reset drop it).
 * srukf_get_image_policy (what updateFeaturesInformation, SLAM.cpp:2443-2459, and the trigger of SLAM.cpp:556 would decide behind frames [first, first + count)):
 *   waits for the stream like srukf_get_image_matches.  verdict[count][N], summary[count], state_out[N] (the device state now) may each be NULL.  *first_change: the
 *   lowest frame index in the range whose summary has `change`, or -1.  Rows no policy run has written are zero.  SRUKF_ERR_SEQUENCE: no images staged or no policy
 *   run since they were; SRUKF_ERR_DIM_MISMATCH: rows outside the staged stack.
 * srukf_images_rewind (the undo a host needs to stop a block at the frame whose verdict asks for a map change, SLAM.cpp:552-562): puts back the checkpoint of the
 *   image block that the last srukf_synchronize ended clean — X, S, every matchPatch and the policy state, as a flagged block's automatic restore does (which puts
 *   the policy state back too).  Either restore also zeroes every verdict and summary row: what the restored frames wrote is no verdict any more, and
 *   srukf_get_image_policy reads such rows as rows no policy run has written (first_change -1) until frames run again.  SRUKF_ERR_SEQUENCE: a run is pending, no image block has been synchronised clean, or anything has written X, S or a matchPatch
 *   since (srukf_predict_motion, srukf_set_state, srukf_run_frames*, srukf_associate*, an appearance capture, srukf_images_set_policy_state, ...; a second rewind of the same block).
 * All: SRUKF_ERR_BAD_ARG for a NULL handle (srukf_get_image_policy: first < 0, count < 1; srukf_images_set_policy_state: state NULL) before any device is touched. */
#define SRUKF_POLICY_UNMATCHED     1
#define SRUKF_POLICY_RHO           2
#define SRUKF_POLICY_BEHIND        4
#define SRUKF_POLICY_PRED_BORDER   8
#define SRUKF_POLICY_MATCH_BORDER 16
#define SRUKF_POLICY_STORE        32
typedef struct srukf_policy_params { double border; double rho_min; int min_predictions; int min_matches; } srukf_policy_params;
#define SRUKF_POLICY_DEFAULTS { 20.0, 0.01, 10, 5 }
typedef struct srukf_policy_state { int nPredictTimes; int nMatchTimes; double predictLocation[2]; } srukf_policy_state;
typedef struct srukf_policy_summary { int n_predicts, n_matches, n_deletes, n_stores, n_predicts_after, n_matches_after, need_add, change; } srukf_policy_summary;
int  srukf_map_policy(srukf_ctx* ctx, const srukf_policy_params* params, srukf_policy_state* state_inout, const double* h, const int* visible, const double* z,
                      const int* matched, int* verdict, srukf_policy_summary* summary);
int  srukf_images_policy(srukf_ctx* ctx, int on, const srukf_policy_params* params);
int  srukf_images_set_policy_state(srukf_ctx* ctx, const srukf_policy_state* state);
int  srukf_get_image_policy(srukf_ctx* ctx, int first, int count, int* verdict, srukf_policy_summary* summary, srukf_policy_state* state_out, int* first_change);
int  srukf_images_rewind(srukf_ctx* ctx);

/* ---- 1-point RANSAC consensus inside the frames of an image run ----
 * srukf_images_ransac: a switch on the handle, like srukf_images_policy: it survives map changes and srukf_reset (which drop the record with the staged
 *   images); srukf_destroy ends it.  threshold: srukf_ransac_consensus' pixel distance (8 is the reference's constant); with `on` != 0 it must be finite and
 *   positive (SRUKF_ERR_BAD_ARG); not while a run is in flight (SRUKF_ERR_SEQUENCE).  The call touches no device.  While on, every frame of every later image run
 *   (srukf_run_images* and srukf_run_images_checked*, BATCHED and JOINT, with the archive search and / or the map policy behind them) runs srukf_ransac_consensus'
 *   two kernels between its association and its update, on the operands the frame holds at that point (S^T DZ, the robot rows of the cross covariances, h, Si,
 *   visible, the predicted X; this frame's rows of the association's record): A = { k : matched and visible }, every member a hypothesis, the one with the most
 *   votes wins (lowest index among equals).  The frame's `matched` row is then REWRITTEN to the winner's consensus set and the update uses that set only;
 *   srukf_get_image_matches and the map policy therefore see what the filter used (z is left as the association wrote it).  With fewer than two members of A
 *   nothing is rewritten (one match cannot out-vote itself).  There is no rescue step on the device: a frame whose consensus dropped a match is marked
 *   `outlier`, and a host that wants the rescue (srukf_repredict_measurement, the chi-square test, a second update) ends its block in front of that frame
 *   (srukf_images_rewind, the frames up to it again) and runs it step-wise.  Such frames are captured frames of their own per kind of image run and update mode
 *   (a run never replays a frame captured the other way); the threshold lives in a device struct written in stream order in front of each run, so changing it
 *   needs no recapture.  With the switch off an image run is exactly what it was.
 * srukf_get_image_ransac: rows [first, first + count) of the consensus record, after waiting for the stream like srukf_get_image_matches.  flags[count][N]: bit 0
 *   (SRUKF_RANSAC_ACTIVE) the landmark was in A, bit 1 (SRUKF_RANSAC_INLIER) a low-innovation inlier; votes[count][N] and dist[count][N] as
 *   srukf_ransac_consensus returns them (votes of every member of A; the distances under the winner); best / n_active / n_low [count]; *first_outlier: the lowest
 *   frame of the range with n_active >= 2 && n_low < n_active, or -1.  A frame with n_active < 2: inlier = active, votes 0, dist 0, best -1, n_low = n_active.
 *   Any pointer may be NULL.  Rows no such frame has written are zero, and so are all rows after a flagged block's restore or srukf_images_rewind (their frames'
 *   results do not stand: first_outlier -1) until frames run again.  SRUKF_ERR_SEQUENCE: no images staged, or no run with the switch on since they were;
 *   SRUKF_ERR_DIM_MISMATCH: rows outside the staged stack.
 * Both: SRUKF_ERR_BAD_ARG for a NULL handle (srukf_get_image_ransac: first < 0, count < 1) before any device is touched. */
#define SRUKF_RANSAC_ACTIVE 1
#define SRUKF_RANSAC_INLIER 2
int  srukf_images_ransac(srukf_ctx* ctx, int on, double threshold);
int  srukf_get_image_ransac(srukf_ctx* ctx, int first, int count, int* flags, int* votes, double* dist, int* best, int* n_active, int* n_low, int* first_outlier);

/* ---- the state at a block's stop: resume without running frames again ----
 * A block is every image run between two srukf_synchronize calls.  A host that stops a block inside it (the policy's first_change, the consensus' first_outlier)
 *   can put the checkpoint back and run the frames in front of the stop again (srukf_images_rewind), or, with this switch, take the state the first run already
 *   passed through.
 * srukf_images_snapshots: a switch on the handle, like srukf_images_ransac: it survives map changes and srukf_reset (which drop the slots with the staged images);
 *   srukf_destroy ends it.  Not while a run is in flight or a block is pending (SRUKF_ERR_SEQUENCE).  The call touches no device.  While on, every frame of
 *   every later image run (all kinds, BATCHED and JOINT) begins with one more launch, k_image_snapshot: while no frame of the block in [first frame, f) is an
 *   `outlier` frame of the consensus and none in [first frame, f - 1) has the policy's `change`, it copies X, S, every matchPatch and the policy state into slot
 *   f & 1 and tags the slot with f; otherwise it writes nothing.  So behind a policy stop at frame k the slot (k + 1) & 1 holds the state frame k + 1 started
 *   from (k + 1 frames are kept), behind an outlier at frame k the slot k & 1 holds the state frame k started from, and behind a block without a stop the slots
 *   hold the starts of its last two frames.  Such frames are captured frames of their own; the guard's parameters live in a device struct written in stream
 *   order in front of each run.  The frames compute exactly what they compute without the launch.  With the switch off an image run is exactly what it was.
 * srukf_get_image_snapshots: waits for the stream; frames[0], frames[1]: the staged frame each slot is tagged with, -1 for none (a new block clears both).
 * srukf_images_resume(keep), keep counted from the block's first frame: legal exactly where srukf_images_rewind is, in a block whose every run had the switch
 *   on (and began where the one before ended); SRUKF_ERR_SEQUENCE otherwise, the state untouched.  keep == 0 is srukf_images_rewind.  keep == the frames the
 *   block ran: nothing moves, SRUKF_OK.  Any other keep: the slot (first + keep) & 1 must be tagged first + keep — if not, SRUKF_ERR_SEQUENCE, the state is
 *   untouched and the block can still be rewound.  Then X, S, every matchPatch and the policy state come from the slot; rows >= keep of the policy record and of
 *   the consensus record are zeroed, rows < keep stay; every other record (matches, checks, archive search) and the caller's trajectory rows are what the first run
 *   wrote.  Afterwards the handle holds, byte for byte, what srukf_images_rewind followed by a run of the first keep frames leaves.  One resume or one rewind per
 *   block.  keep < 0 or > the frames run: SRUKF_ERR_BAD_ARG.  A flagged block is restored by srukf_synchronize as before, and a resume is refused there.
 * All: SRUKF_ERR_BAD_ARG for a NULL handle (srukf_get_image_snapshots: frames NULL; srukf_images_resume: keep < 0) before any device is touched. */
int  srukf_images_snapshots(srukf_ctx* ctx, int on);
int  srukf_get_image_snapshots(srukf_ctx* ctx, int frames[2]);
int  srukf_images_resume(srukf_ctx* ctx, int keep);

/* ---- the rescue gate on the device: would a match the consensus dropped be rescued? ----
 * The rule, in all three calls.  A frame has candidates when n_active >= 2 and 0 < n_low < n_active (rescueHighInnovationInliers' condition); its candidates are
 *   the landmarks in A (matched and visible) that are no low-innovation inliers.  For a candidate k the gate forms h', Si' and visible' as
 *   srukf_repredict_measurement defines them for the posterior (X, S) of the frame's update; k is RESCUED when visible', Si'[0] != 0, Si'[3] != 0 and
 *   y = Si'^-T (z - h') (forward substitution: y0 = v0 / Si'[0], y1 = (v1 - Si'[1] y0) / Si'[3]) has y0^2 + y1^2 < chi2, strictly (dataAssociation's gate, 1977;
 *   CHI2INV_TABLE(0, 2) = 5.99146454710798).  flags: bit 0 (SRUKF_RESCUE_CANDIDATE), bit 1 (SRUKF_RESCUE_RESCUED); h2 [2N], Si2 [4N], chi2 [N] (y0^2 + y1^2; 0 where
 *   the test was not formed) hold values for candidates and zeros for everybody else.  The gate decides, it updates nothing: the second update stays the host's.
 * srukf_images_rescue_gate: a switch on the handle, like srukf_images_ransac: it survives map changes and srukf_reset (which drop the record with the staged
 *   images).  With `on` != 0 chi2 must be finite and positive (SRUKF_ERR_BAD_ARG); not while a run is in flight (SRUKF_ERR_SEQUENCE).  The call touches no device.
 *   It takes effect only in frames whose consensus runs: with srukf_images_ransac off it adds no launch.  While both are on, every frame of every later image run
 *   has the gate behind its tail (two launches, in front of the archive search; captured frames of their own; chi2 in a device struct written in stream order in
 *   front of each run, so changing it needs no recapture), the frames compute exactly what they compute without it, and the snapshot guard of
 *   srukf_images_snapshots reads "frame f - 1 rescued a match" where it read "frame f - 1 dropped a match": behind a rescue at frame k the slot k & 1 holds the
 *   state frame k started from and srukf_images_resume(k - first frame of the block) is legal; a frame that only dropped matches stops nothing.
 * srukf_get_image_rescue: rows [first, first + count) of the gate's record, after waiting for the stream like srukf_get_image_matches.  n_cand / n_high [count]:
 *   candidates and rescued candidates of each frame; *first_rescue: the lowest frame of the range with n_high > 0, or -1.  Any pointer may be NULL.  Rows no such
 *   frame has written are zero, and so are the rows a flagged block's restore, srukf_images_rewind or srukf_images_resume zeroes in the consensus record.  SRUKF_ERR_SEQUENCE: no images staged, or no run with both
 *   switches on since they were; SRUKF_ERR_DIM_MISMATCH: rows outside the staged stack.
 * srukf_rescue_gate: step-wise, where srukf_repredict_measurement is legal (after a srukf_update, in the same frame; SRUKF_ERR_SEQUENCE otherwise).  z, matched:
 *   what the consensus was given (matched: the set A, i.e. matched and visible); inlier: its low-innovation inliers.  One launch that reads the posterior in place
 *   and a copy of the results; outputs are host pointers, any may be NULL.  It changes neither phase nor state and drops nothing the first update prepared for the
 *   next frame: srukf_repredict_measurement (when *n_high > 0: the second update needs the full prediction) or the next srukf_predict_motion follow as before.
 *   chi2 not finite and positive, or a NULL z / matched / inlier: SRUKF_ERR_BAD_ARG before any device is touched. */
#define SRUKF_RESCUE_CANDIDATE 1
#define SRUKF_RESCUE_RESCUED 2
int  srukf_images_rescue_gate(srukf_ctx* ctx, int on, double chi2);
int  srukf_get_image_rescue(srukf_ctx* ctx, int first, int count, int* flags, double* h2, double* Si2, double* chi2, int* n_cand, int* n_high, int* first_rescue);
int  srukf_rescue_gate(srukf_ctx* ctx, const double* z, const int* matched, const int* inlier, double chi2, int* flags, double* h2, double* Si2, double* chi2_out, int* n_high);

/* ---- the display view behind every frame of an image run, the overlay of any staged frame ----
 * srukf_images_display: a switch on the handle, like srukf_images_snapshots: it survives map changes and srukf_reset (which drop the record with the staged
 *   images); srukf_destroy ends it.  Not while a run is in flight or a block is pending (SRUKF_ERR_SEQUENCE).  The call touches no device.  While on, every frame
 *   of every later image run (all kinds, BATCHED and JOINT) is followed by what the reference's SLAM() refreshes for its display after every update
 *   (updateFeaturesInformation -> refreshFeaturesDisplay, SLAM.cpp:2566-2575; recordRobotInformation 3539-3556), written into the frame's row of a record:
 *   srukf_get_frame_view_display's xyz, cov, axis, sigma, pose4 and P4 and srukf_get_landmarks_display's rot on the frame's posterior, bit for bit, and Si, the
 *   innovation factors the frame's association read (srukf_predict_measurement's).  Two launches behind the frame (k_image_view, k_lm_ellipsoid); the run is
 *   issued frame by frame as a policy run is, so a run without the policy gives up its eight-frame graphs.  The launches read the state and write the record
 *   only: the filter computes exactly what it computes without them.  With the switch off an image run is exactly what it was.
 * srukf_get_image_display: rows [first, first + count) of that record, after waiting for the stream like srukf_get_image_matches: xyz[count][N][3],
 *   cov[count][N][9], axis[count][N][4] (quaternion r, x, y, z), sigma[count][N][3], rot[count][N], pose4[count][4], P4[count][16], Si[count][N][4].  Any
 *   pointer may be NULL, not all of them (SRUKF_ERR_BAD_ARG).  Rows no such frame has written are zero — all of them before the first run with the switch on —
 *   and so are rows >= the stop after srukf_images_resume and all rows after a flagged block's restore or srukf_images_rewind, until frames run again.  A row
 *   whose frame a run without the switch has run again keeps the earlier run's values (srukf_get_image_checks' rule) and is no longer drawable.
 *   SRUKF_ERR_SEQUENCE: no images staged; SRUKF_ERR_DIM_MISMATCH: rows outside the staged stack.
 * srukf_render_image_overlay: srukf_render_overlay (display2DFeatureModel, SLAM.cpp:3009-3051) for staged frame `frame` with nothing uploaded: the frame's
 *   predicted pixels, the record's Si row, the frame's z and `matched` rows (behind a consensus run the rewritten row: what the filter used) drawn over the
 *   frame's gray image in the staged stack, gray byte three times, into out_bgr[image_h][image_w][3].  Waits for the stream first; reads and writes nothing the
 *   filter reads.  SRUKF_ERR_SEQUENCE: no images staged, or no run with the switch on has written that frame's row since it was last zeroed (the library keeps a
 *   mark per row on the host); SRUKF_ERR_BAD_ARG: frame outside the stack, out_bgr NULL; SRUKF_ERR_UNSUPPORTED: image_w * image_h is no multiple of four.
 * All: SRUKF_ERR_BAD_ARG for a NULL handle (srukf_get_image_display: first < 0, count < 1) before any device is touched. */
int  srukf_images_display(srukf_ctx* ctx, int on);
int  srukf_get_image_display(srukf_ctx* ctx, int first, int count, double* xyz, double* cov, double* axis, double* sigma, int* rot, double* pose4, double* P4, double* Si);
int  srukf_render_image_overlay(srukf_ctx* ctx, int frame, unsigned char* out_bgr);

/* ---- colour frames in the staged stack, the overlays of a run of frames ----
 * srukf_stage_images_bgr: srukf_stage_images for the frames the reference's host has: bgr[n_frames][image_h][image_w][3], interleaved B, G, R bytes, no row
 *   padding (cvQueryFrame / cvLoadImage).  The device converts them with srukf_set_frame_bgr's rule — OpenCV 2.4's fixed-point CV_RGB2GRAY applied to B, G, R
 *   in memory order as loadPictures applies it (SLAM.cpp:529-543), gray = (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14 — into the staged gray stack.  Behind the
 *   call the handle is what srukf_stage_images with the converted bytes leaves: every run, record, getter, rewind, resume and refusal of the image runs behaves
 *   the same.  The refusals are srukf_stage_images', in its order and with its codes; keep_colour outside {0, 1}: SRUKF_ERR_BAD_ARG.  keep_colour = 1 keeps the
 *   colour stack beside the gray one (3 bytes per pixel more) as the source of srukf_render_image_overlay(s); keep_colour = 0 passes the colour bytes through
 *   a transit buffer of at most 12 MiB.  Whatever drops the staged images drops the colour stack: a map change, srukf_reset, srukf_stage_sequence, a later
 *   srukf_stage_images or srukf_stage_images_bgr.  The frame the handle holds (srukf_set_frame_bgr, srukf_associate_held) is neither read nor written.
 * srukf_get_staged_image: frame `frame` of the staged stack, after waiting for the stream: gray_out[image_h][image_w] and / or, from a kept colour stack,
 *   bgr_out[image_h][image_w][3].  Either pointer may be NULL, not both (SRUKF_ERR_BAD_ARG).  SRUKF_ERR_SEQUENCE: no images staged, or bgr_out without a kept
 *   colour stack; SRUKF_ERR_BAD_ARG: frame outside the stack.
 * srukf_render_image_overlay draws over the frame's colour bytes when a colour stack is kept, otherwise over the gray byte three times.  Its refusals and
 *   their codes are what they were; the text srukf_last_error gives for a row that is not drawable now ends in " (frame <q>)".
 * srukf_render_image_overlays: srukf_render_image_overlay for frames [first, first + count) in two launches and one copy: out_bgr[count][image_h][image_w][3],
 *   frame first + q of it byte for byte the single call's.  The refusals are the single call's (frames outside the stack: SRUKF_ERR_BAD_ARG); when any row of
 *   the range is not drawable: SRUKF_ERR_SEQUENCE, srukf_last_error names the first such frame, and out_bgr is untouched; count > 65 535: SRUKF_ERR_UNSUPPORTED.  Its device scratch grows to the
 *   largest count asked for and goes with the staged images.
 * All: SRUKF_ERR_BAD_ARG for a NULL handle or NULL frames / out_bgr (first or frame < 0, count or n_frames < 1) before any device is touched. */
int  srukf_stage_images_bgr(srukf_ctx* ctx, int n_frames, const unsigned char* bgr, int keep_colour);
int  srukf_get_staged_image(srukf_ctx* ctx, int frame, unsigned char* gray_out, unsigned char* bgr_out);
int  srukf_render_image_overlays(srukf_ctx* ctx, int first, int count, unsigned char* out_bgr);

/* ---- instrumentation ------------------------------------------------------------------------ */

/* When on, every kernel launch is bracketed by HIP events on the context's stream and the
 * durations are accumulated per kernel class (no graph replay in this mode). */
int  srukf_set_profiling(srukf_ctx* ctx, int on);
/* Number of kernel classes; then name / total ms / launch count / algorithmic flops and bytes
 * (summed over launches) of class i since the last srukf_profile_reset. */
int  srukf_profile_count(srukf_ctx* ctx);
int  srukf_profile_get(srukf_ctx* ctx, int i, const char** name, double* total_ms, long long* launches,
                       double* alg_flops, double* alg_bytes);
int  srukf_profile_reset(srukf_ctx* ctx);

/* Test hooks, not for hosts.  poke_state: one entry of S behind the back of everything that tracks S.  starve_workers: persistent
 * factorisation launches of this context start without their worker workgroups, as if another process held the GPU (exercises the
 * bounded waits and the fallback to per-panel launches). */
int  srukf_debug_poke_state(srukf_ctx* ctx, int row, int col, double value);
int  srukf_debug_starve_workers(srukf_ctx* ctx, int on);      /* on = 2: only the split form's pair is starved (the tier it falls back to runs undisturbed) */
/* Kept for ABI compatibility (rounds 2 - 5: let srukf_set_storage accept SRUKF_STORAGE_F32_MIXED below its then epsilon floor): no effect since round 6. */
int  srukf_debug_allow_mixed(srukf_ctx* ctx, int on);

/* Measurement / test switches, not for hosts (every one defaults to the product path; captured graphs are dropped).
 * Process-wide keys (ctx may be NULL; they apply to what is built or captured afterwards):
 *   "gmw_persist" (0: one launch per 64-row panel), "gmw_fused", "rank_fused", "rank_fold" (0: the owners of the persistent launch never form
 *   their tiles of S^T S - U U^T themselves), "rank_aware", "graphs" (0: contexts created afterwards launch eagerly, which rocprofv3 --pmc needs),
 *   "shared_tenants" (2..8: persistent launches that share the GPU after srukf_set_exclusive(SRUKF_GPU_SHARED); srukf_run_frames_batch picks its own),
 *   "batch_wide" (0: srukf_run_frames_batch never takes the batched launches), "batch_groups" (1..4: groups the batched filters are cut into; 0, the default: as many as pay),
 *   "batch_split" (0: one launch per panel in the batched replay instead of slabs + plain trailing updates),
 *   "mem_split" (0: sizes beyond two register tiles per worker — N >= 400 — keep the memory-tile instance of k_gmw_persist instead of the split form
 *   k_gmw_pivslab_persist + k_gmw_tiles_persist; 2: the split form also where a worker would own two register tiles),
 *   round 6: "exact_rl" (0: the left-looking exact path k_gmw_col, one row per launch; 1: right-looking, as many pivots per launch as fit — default; 1 + B: B pivots per
 *   launch), "fold_head" (block rows the k_syrk launch in front of the split fold forms; 0: the rule 2 (Tp - 17)), "fold_force" (the split fold also where the tile workgroups
 *   do not all fit beside the pivot / slab launch), "timing" (1: phases of map changes and of flagged frames on stderr), "ctx_keep" (contexts a handle keeps across map
 *   changes: default 24), "batch_xcd" (0: k_syrk_b walks the head tiles in the solo launch's order), "batch_k128" (0: one pass over G per panel in the batched replay's
 *   trailing updates instead of one per pair of panels), "head_fold_free" (>= 1: CUs a plan must leave beside the pivot and the workers for the head fold, in place of
 *   the built-in rule — which, once replaced, cannot be set back), "pivot_relay" (0: one pivot workgroup instead of two in the register-tile persistent launch; read when
 *   a plan is built).
 * Per-context keys: "use_graph" (0: eager launches), "fused_motion" (0: k_motion + k_project as two launches, 1: k_project_motion, 2: "table"
 *   mode), "pxy2" (0: k_pxy instead of k_pxy2), "nullskip", "head_fold" (0: k_syrk launch in front of the persistent launch), "tail_fuse"
 *   (0: k_project_table in front of every frame), "table_perm", "f32_fuse", "step_fast" (0: the step-wise API keeps to its own launch sequences instead of the
 *   staged replay's cut at the association step), "step_fuse_export" (0: the fast path's results leave through export launches of their own instead of from the
 *   launches that form them), "step_early" (what srukf_update submits of the NEXT frame behind its own tail: 0 nothing, 1 checkpoint copy + frame scalars, 2 (default)
 *   also the announced frame's first launch), "step_spin" (0: wait with hipStreamSynchronize instead of spinning on the pinned flag word), "view_auto" (0: the display
 *   view is never exported with an update's status), "split_record"; round 6: "gain_fold" (1: k_gain's work in the tile epilogue of k_pxy2_fold — three launches per frame,
 *   slower: off), "split_fold" (0: k_syrk over all kept rows in front of the split form's pair instead of forming jobs inside its tile launch), "mixed_rank" (0: round 2's
 *   full-rank form of SRUKF_STORAGE_F32_MIXED), "mixed_f64_robot" (0: every tile of the mixed downdate on the fp32 pipe), "mixed_bf16" (1: its fp32 products from three bf16
 *   pieces), "mixed_null_ppm", "null_canon" (0: the null rows of a factor that NEED_REORDER or a map operation produced are left as they are until a frame tail rewrites them).
 *   Every key with its range, its default and what a change invalidates: the table in srukf_debug.hip; the measurements behind them: srukf_switches.h. */
int  srukf_debug_set(srukf_ctx* ctx, const char* key, int value);
/* Row `index` of the switch table (0 .. count-1; SRUKF_ERR_BAD_ARG beyond). Any out pointer may be NULL.
 * value: the current setting; for a per-filter row with ctx == NULL, the default. Touches no stream. */
int  srukf_debug_switch_at(srukf_ctx* ctx, int index, const char** key, int* per_filter, int* default_value, int* value);
/* Diagnostic read-out of device-resident counters ("gmw_aborts", "clamp_rows", "frame", "frozen", "gate_timeouts", "gmw_shared", "split_form", "split_off",
 * "step_fast" / "step_slow": frames the step-wise API ran on the fast / the other path, "view_hits": srukf_get_frame_view calls served from an exported view,
 * "meas_flag_ticks": 10-ns ticks from the start of the fast path's last k_pxy2 to the moment the host had its statistics) and of the launch plan the next staged frame takes ("plan_persist",
 * "plan_register_form", "plan_tiles_per_worker", "plan_fold", "plan_head_fold", "plan_red_perm", "plan_motion", "plan_fuse", "plan_T", "plan_Tp", "plan_tiles",
 * "plan_workers", "plan_kept"). */
int  srukf_debug_get(srukf_ctx* ctx, const char* key, long long* value);
/* Diagnostic copy of a device work buffer (tests compare the launch sequences stage by stage): key = "Z", "DZ", "sigR", "Cmat", "Xr1",
 * "Utp", "P1", "h", "Si", "det_resp" (the response map r of the last srukf_detect_features, image_h x image_w), "Ut" (mp x np: U^T in state order behind an update of the
 * slow form), "PxyR" (5 x mp), "joint_R" (behind srukf_update_joint: mp rows of mp + np + 32 doubles, R | U^T | w); `count` doubles from the start of the buffer. */
int  srukf_debug_copy(srukf_ctx* ctx, const char* key, double* out, long long count);
/* ... and the other way (same keys, plus the operands of one factorisation: "Wf", "Gbak", "G", "D", "gsW", "gsL", "pans", "sync" — byte buffers counted in doubles).
 * srukf_debug_split_replay: ONE launch of the split form's pair (0: k_gmw_pivslab_persist, 1: k_gmw_tiles_persist) `reps` times ALONE against the buffers and flags a
 * real frame left behind (recorded with the "split_record" switch, moved between processes with debug_copy / debug_upload): the pair itself cannot run under
 * rocprofv3's counter passes, which serialise dispatches (scripts/split_replay.py). */
int  srukf_debug_upload(srukf_ctx* ctx, const char* key, const double* in, long long count);
int  srukf_debug_split_replay(srukf_ctx* ctx, int which, int reps);
/* Diagnostic builds (-DSRUKF_GMW_DBG) only: arms / reads the time stamps of the persistent factorisation launch (4096 values). */
int  srukf_debug_gmw_stamps(srukf_ctx* ctx, unsigned long long* buf);

/* Problem sizes of a context: N, n, Na, L. */
int  srukf_dims(const srukf_ctx* ctx, int* N, int* n, int* Na, int* L);

/* Stand-alone numeric primitives on DEVICE buffers (used by the parity tests; same kernels the
 * frame path launches).
 *   gmw   : S_out(upper) = modifiedCholeskyDecomposition(G)      SLAM.cpp:2197-2327
 *           G is n*n row-major symmetric (upper triangle read). force_slow=1 takes the
 *           column-by-column path that evaluates theta_j exactly as the reference does.
 *           clamp_hit (host int*, may be NULL) reports whether the theta clamp was active.  */
int  srukf_gmw_host(int device, int n, const double* G, double* S_out, double* D_out, double epsilon,
                    int force_slow, int* clamp_hit);
/*   project: one camera projection, SLAM.cpp:1634-1674 + 3177-3347 (host in/out, runs the device fn) */
int  srukf_project_host(int device, const srukf_params* p, int count, const double* feat6, const double* pos3,
                        const double* psi, const double* err2, double* uv_out);

#ifdef __cplusplus
}
#endif
#endif /* SRUKF_H_ */
