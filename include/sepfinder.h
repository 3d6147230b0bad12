/*
 * sepfinder.h -- C-ABI boundary of the MI355X-native inter-robot separator finder.
 *
 * This is the drop-in surface for ONE hot path of bramtoula/multi_robot_SLAM_separators
 * (SURVEY.md section 8): NetVLAD nearest-neighbour candidate search + binary local-descriptor
 * matching + RANSAC relative pose (3D-3D, or 3D-2D PnP with estimation_type = 1).  Everything is `extern "C"`, plain pointers and sizes,
 * no torch / ROS / OpenCV types.  All citations are relative to the reference tree, with
 * PKG = ros_ws/src/multi_robot_separators.
 *
 * Reference interface each group of entry points replaces:
 *   sf_nn_*            PKG/scripts/data_handler.py:166-209   DataHandler.find_matches
 *                      PKG/scripts/data_handler.py:297-301   find_matches_service (descriptor append)
 *                      PKG/scripts/data_handler.py:402-408,437-438  mask bookkeeping
 *                      wire: PKG/srv/FindMatches.srv:1 (float64[] new_netvlad_descriptors)
 *   sf_store_*         PKG/scripts/data_handler.py:268,421-422  geometric_feats cache of one keyframe's
 *                      (descriptors, kpts3D, kpts); layouts PKG/msg/Descriptors.msg:1-3,
 *                      KeyPoint3DVec.msg:1-2, KeyPointVec.msg:1-2, PKG/src/MsgConversion.cpp:8-42,113-116
 *   sf_estimate_*      PKG/src/stereoCamGeometricTools.cpp:122-178  estimateTransformation service
 *                      (PKG/srv/EstTransform.srv:1-9), which drives
 *                      PKG/src/myRegistration.cpp:225-303 and PKG/src/myRegistrationVis.cpp:441-1410
 *   sf_verify_*_device, sf_find_matches_and_verify_device, sf_compact_accepted_device
 *                      PKG/scripts/find_separators.py:59-133  the caller's loop body (find_matches, then one
 *                      estimate_transformation per returned candidate, then the accepted separators) for
 *                      keyframes that already live in the handle's device store
 *   sf_result          geometry_msgs/PoseWithCovariance + bool success (EstTransform.srv:8-9),
 *                      packed as PKG/src/MsgConversion.cpp:61-64,71-81 do
 *   sf_separator       one row of PKG/srv/ReceiveSeparators.srv:1-10 (what the back-end consumes,
 *                      PKG/src/factorGraph.cpp:98-118)
 *
 * Ownership: every input pointer is BORROWED for the duration of the call; every output is
 * written into CALLER-allocated memory; the handle owns all device memory.  No allocation
 * crosses the ABI.  A handle is single-caller (not thread-safe), like the reference's
 * single-threaded geometry node (stereoCamGeometricTools.cpp:212).
 *
 * Errors: every function returns an int status.  A failed pose estimation is NOT an error
 * (success=0, zero pose, covariance as the reference leaves it).  Size mismatches on which the
 * reference UASSERT-aborts (myRegistrationVis.cpp:482-483,859-860,878-880) return SF_EINVAL.
 */
#ifndef SEPFINDER_H
#define SEPFINDER_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: sf_params.reserved[5] became bundle_adjustment / ba_* / stereo_baseline, sf_find_matches_and_verify_device accepts
      d_out = NULL, sf_debug_correspondences needs SF_OPT_DEBUG_CORR, sf_step_* added, the accepted-result stream and the
      indexed compactions moved to sf_experimental.h.  A binding checks sf_abi_version() against the header it was
      written for (multi_robot_slam_separators_amd/lib.py does).                                                   */
/* 3: sf_params grew force_3dof / forward_est_only (appended), sf_nn_row_minima_device, sf_allgather_bytes_device,
      sf_netvlad_infer_batch_device, sf_get_features_and_descriptor_batch_device added.                                                                          */
/* 4: sf_step_mirror_pair, sf_step_mirror_streams, SF_OPT_STEP_SPLIT added (nothing existing changed).                */
/* 5: sf_step_issue no longer waits for the device (SF_OPT_STEP_DEVICE_WALK, _DEPTH, _LANES), sf_nn_walk_device added; 
      sf_step_result pointers stay valid until the next sf_step_retire; sf_params grew desc_type (appended).         */
/* 6: SF_K_BA added to the kernel ids of sf_prof_get (SF_K_COUNT 10 -> 11): the bundle adjustment is a launch of its
      own; sf_step_issue refuses more steps in flight than a mirror has buffers for.                                */
/* 7: sf_params.reserved0 became guess_match_to_projection (same offset, same size); SF_K_GUIDED_TP added to the kernel
      ids of sf_prof_get (SF_K_COUNT 11 -> 12).                                                                     */
/* 8: sf_orb_params, sf_orb_defaults, sf_set_feature_type, sf_get_feature_type, sf_orb_set_pattern, sf_orb_get_pattern
      added (GFTT/ORB descriptors, Vis/FeatureType 8), nothing existing changed.                                      */
/* 8, additions: sf_fast_params, sf_fast_defaults, sf_fast_set_params, sf_fast_get_params, sf_detect_fast_device;
      sf_set_feature_type accepts 4 (FAST/BRIEF).  Nothing existing changed, the version number stays.               */
/* 8, additions: sf_orb_detector_params, sf_orb_detector_defaults, sf_set_feature_type_orb, sf_get_orb_detector,
      sf_detect_orb_device (ORB on a pyramid, Vis/FeatureType 2).  sf_set_feature_type still refuses 2; nothing existing
      changed, the version number, sizeof(sf_params) and SF_K_COUNT stay.                                            */
/* 8, additions: sf_image_format, sf_image_set_gray_rule, sf_image_get_gray_rule, sf_image_to_gray_device,
      sf_netvlad_infer_u8_batch_device, sf_get_features_and_descriptor_u8, sf_add_keyframes_u8_batch_device (keyframes from
      the camera's rgb8 / bgr8 / mono8 images).  Nothing existing changed, the version number, sizeof(sf_params) and
      SF_K_COUNT stay.                                                                                                */
/* 8, additions: sf_get_features_and_descriptor_orb_batch_device, sf_add_keyframes_orb_u8_batch_device (the batch forms of
      Vis/FeatureType 2).  The generic batch calls still refuse a type-2 handle, with a message that now names these two;
      nothing existing changed, the version number, sizeof(sf_params) and SF_K_COUNT stay.                            */
/* 8, additions: sf_front_params, sf_front_defaults, sf_front_set_params, sf_front_get_params, sf_compute_roi,
      sf_corner_subpix_device (Vis/RoiRatios and the Vis/SubPix* refinement around every detector).  Both steps are off on
      a fresh handle; nothing existing changed, the version number, sizeof(sf_params) and SF_K_COUNT stay.             */
/* 8, additions: sf_stereo_params, sf_stereo_defaults, sf_stereo_set_params, sf_stereo_get_params,
      sf_stereo_block_match_device (Stereo/OpticalFlow false: block-matching stereo correspondence).  A fresh handle runs
      pyramidal LK as before; nothing existing changed, the version number, sizeof(sf_params) and SF_K_COUNT stay.     */
/* 8, additions: sf_grid_params, sf_grid_defaults, sf_grid_set_params, sf_grid_get_params, sf_compute_grid (Vis/GridRows x
      Vis/GridCols: the detector per cell of the ROI; 1 x 1 on a fresh handle, which changes nothing); the version
      number, sizeof(sf_front_params), sizeof(sf_params) and SF_K_COUNT stay.                                          */
/* 8, additions: sf_freak_params, sf_freak_defaults, sf_set_feature_type_freak, sf_get_freak_params, sf_freak_set_pairs,
      sf_freak_get_pairs, sf_freak_build_pattern, sf_freak_default_pairs (FAST/FREAK and GFTT/FREAK, Vis/FeatureType 3 and
      5: 64-byte rows).  sf_set_feature_type still refuses 3 and 5; nothing existing changed, the version number,
      sizeof(sf_params) and SF_K_COUNT stay.                                                                           */
/* 8, additions: sf_surf_params, sf_surf_defaults, sf_set_feature_type_surf, sf_get_surf_params, sf_detect_surf_device
      (SURF, Vis/FeatureType 0: float32 rows of 64 or 128 dimensions on a handle with desc_type 1).  sf_set_feature_type
      still refuses 0; nothing existing changed, the version number, sizeof(sf_params) and SF_K_COUNT stay.            */
/* 8, additions: sf_get_features_and_descriptor_surf_batch_device, sf_add_keyframes_surf_u8_batch_device,
      sf_surf_batch_status (the batch forms of Vis/FeatureType 0).  The four existing batch calls still refuse a type-0
      handle, now naming these; nothing existing changed, the version number, sizeof(sf_params) and SF_K_COUNT stay.  */
/* 8, additions: sf_sift_params, sf_sift_defaults, sf_set_feature_type_sift, sf_get_sift_params, sf_detect_sift_device
      (SIFT, Vis/FeatureType 1: float32 rows of 128 dimensions on a handle with desc_type 1 and desc_bytes 512; the single
      calls only).  sf_set_feature_type still refuses 1; nothing existing changed, the version number, sizeof(sf_params)
      and SF_K_COUNT stay.                                                                                             */
/* 8, additions: sf_get_features_and_descriptor_sift_batch_device, sf_add_keyframes_sift_u8_batch_device,
      sf_sift_batch_status (the batch forms of Vis/FeatureType 1).  The six existing batch calls still refuse a type-1
      handle, now naming these; nothing existing changed, the version number, sizeof(sf_params) and SF_K_COUNT stay.  */
/* 8, additions: sf_params.desc_type 2 (uint8 rows of 128 dimensions compared by L2, desc_bytes 128; sf_create refused the
      value before), SF_DESC_BYTES_U8, sf_set_feature_type_sift on such a handle (SIFT rows as uint8), sf_debug_knn2_u8
      (sf_experimental.h).  Handles with desc_type 0 or 1 are untouched; the version number, sizeof(sf_params) and
      SF_K_COUNT stay.                                                                                                 */
/* 8, additions: sf_gftt_params, sf_gftt_defaults, sf_gftt_set_params, sf_gftt_get_params (GFTT/BlockSize,
      GFTT/UseHarrisDetector, GFTT/K: the response of the GFTT detector, handle state read by sf_detect_corners_device and
      by every extraction call under Vis/FeatureType 5, 6 and 8), sf_gftt_check_params (sf_experimental.h).  A fresh handle
      holds (3, 0, 0.04), with which nothing existing changed; the version number, sizeof(sf_params) and SF_K_COUNT stay. */
/* 8, additions: sf_depth_format, sf_depth_params, sf_depth_defaults, sf_depth_set_params, sf_depth_get_params,
      sf_depth_mask_device, sf_depth_points_device, sf_detect_corners_masked_device, sf_detect_fast_masked_device,
      sf_extract_keyframe_depth_device, sf_get_features_and_descriptor_depth,
      sf_get_features_and_descriptor_depth_batch_device, sf_add_keyframes_depth_batch_device (RGB-D keyframes: 3D points
      from a registered depth image, Vis/DepthAsMask).  New calls only: every existing call keeps its behaviour and its
      messages; the version number, sizeof(sf_params) and SF_K_COUNT stay.                                             */
/* 8, additions: sf_kfblob_header, sf_kfblob_entry, SF_KFBLOB_MAGIC, sf_store_export_plan, sf_store_export_keyframes_device,
      sf_store_import_keyframes_device, sf_store_wire_status (store slots as one block of bytes, both directions on the
      device).  New calls only; the version number, sizeof(sf_params) and SF_K_COUNT stay.                             */
/* 8, additions: sf_depth_size, sf_depth_set_size, sf_depth_get_size, sf_depth_interpolate_device,
      sf_depth_interpolation_factor (RGB-D keyframes from a decimated depth image, upstream's util2d::interpolate path).
      A fresh handle holds {0, 0}, with which every depth call behaves and refuses as before; the version number,
      sizeof(sf_params) and SF_K_COUNT stay.                                                                           */
/* 8, additions: sf_camera_info, SF_MAX_RECTIFY_PLANS, sf_rectify_plan_create, sf_rectify_plan_from_maps,
      sf_rectify_plan_count, sf_rectify_plan_get, sf_rectify_plan_clear, sf_rectify_maps_device, sf_image_rectify_device,
      sf_stereo_camera_from_info, SF_OPT_RECTIFY_TABLE, sf_rectify_check_info (sf_experimental.h) (raw camera images:
      undistortion and rectification on the device).  New calls only; the version number, sizeof(sf_params) and
      SF_K_COUNT stay.                                                                                                  */
/* 8, additions: sf_depth_registration, sf_depth_registration_defaults, sf_depth_register_check, sf_depth_register_device,
      sf_depth_fill_holes_device, sf_debug_depth_register_limits (sf_experimental.h) (a depth image registered to the
      colour camera on the device).  New calls only; the version number, sizeof(sf_params) and SF_K_COUNT stay.        */
#define SF_ABI_VERSION 8

/* ---- status codes ---------------------------------------------------------------------- */
enum {
  SF_OK = 0,
  SF_EINVAL = 1,   /* bad argument / size mismatch (reference: UASSERT abort)            */
  SF_EHIP = 2,     /* HIP runtime error; text via sf_last_error                          */
  SF_ENOMEM = 3,   /* host or device allocation failed                                   */
  SF_ERANGE = 4,   /* index out of range / capacity exceeded / IDL limit exceeded         */
  SF_ENODEV = 5,   /* no GPU visible: the product path has NO CPU fallback                */
  SF_ERCCL = 6     /* RCCL error (or librccl.so not loadable); text via sf_last_error        */
};

/* ---- limits inherited from the reference IDL --------------------------------------------- */
#define SF_MAX_FEATURES   32767  /* KeyPoint3DVec.msg:1 / KeyPointVec.msg:1  `int16 size`   */
#define SF_MAX_DESC_BYTES 64     /* 512-bit binary descriptors (BASELINE.json configs[4])   */
#define SF_MAX_DESC_BYTES_F32 512 /* float32 descriptors (desc_type 1): 64 or 128 dimensions  */
#define SF_DESC_BYTES_U8 128     /* uint8 descriptors compared by L2 (desc_type 2): 128 dimensions */

/* ---- parameters -------------------------------------------------------------------------- */
typedef struct sf_params {
  /* NetVLAD NN stage: data_handler.py:96-100, defaults multi_robot_separators.launch:19-22 */
  double  netvlad_distance;        /* 0.13 ; accept iff dist <  this (data_handler.py:202)  */
  int32_t netvlad_dimensions;      /* 128                                                   */
  int32_t netvlad_max_matches_nb;  /* 20                                                    */
  int32_t nn_precision;            /* 0 = fp32 MFMA ranks every column, f64 re-evaluation of the
                                          row minima (all rows exact);
                                      1 = fp16 MFMA FILTER with a rigorous error band + f64
                                          evaluation of every surviving (row, column): identical
                                          matches; rows whose minimum is >= netvlad_distance
                                          report +inf in sf_nn_last_row_minima
                                          (BASELINE configs[4]: fp16 NetVLAD on MFMA)           */
  /* Registration: myRegistrationVis.cpp:52-71 reads rtabmap's compiled-in defaults [upstream];
     stereoCamGeometricTools.cpp:87 overrides only Vis/MinInliers                           */
  int32_t min_inliers;             /* 5    separators_min_inliers -> Vis/MinInliers          */
  float   inlier_distance;         /* 0.1  Vis/InlierDistance (m)                            */
  int32_t iterations;              /* 300  Vis/Iterations                                    */
  int32_t refine_iterations;       /* 5    Vis/RefineIterations                              */
  double  refine_sigma;            /* 3.0  refineModelSigma (rtabmap util3d_registration)    */
  int32_t estimation_type;         /* 0 = 3D->3D (north_star; myRegistrationVis.cpp:1113-1152),
                                      1 = 3D->2D PnP (:1055-1112; rtabmap's compiled-in default),
                                      2 = epipolar is NOT implemented: sf_create -> SF_EINVAL   */
  float   nndr;                    /* 0.6  Vis/CorNNDR                                       */
  int32_t guess_win_size;          /* 20   Vis/CorGuessWinSize (px); 0 disables guided pass  */
  int32_t ransac_adaptive_stop;    /* 1 = PCL RandomSampleConsensus adaptive k (p=0.99);
                                      0 = evaluate exactly iterations+1 hypotheses           */
  int32_t max_sample_checks;       /* 1000 PCL SampleConsensusModel::max_sample_checks_      */
  uint64_t seed;                   /* sampler key (PCL uses a fixed mt19937 seed 12345)      */
  /* Camera model `cam_` used for BOTH frames (stereoCamGeometricTools.cpp:76,142-143)       */
  double  fx, fy, cx, cy;          /* left().K()                                             */
  int32_t image_width, image_height; /* left().imageSize(); 0 => uncalibrated => no guided pass */
  float   local_transform[12];     /* left().localTransform(): base->optical, row-major 3x4  */
  /* Capacity hints (device memory is grown on demand; these avoid regrowth)                 */
  int32_t store_capacity;          /* keyframes                                              */
  int32_t max_features;            /* per keyframe (rounded up to a multiple of 64)          */
  int32_t desc_bytes;              /* descriptor bytes per feature, 1..64 (32 = ORB/BRIEF)   */
  /* PnP branch (estimation_type = 1): myRegistrationVis.cpp:59-61,1083-1085 [upstream defaults]  */
  float   pnp_reproj_error;        /* 2.0  Vis/PnPReprojError (px); inlier iff error <= this  */
  int32_t pnp_flags;               /* 0    Vis/PnPFlags: only 0 (cv::SOLVEPNP_ITERATIVE)      */
  int32_t pnp_refine_iterations;   /* 0    Vis/PnPRefineIterations (rtabmap util3d::solvePnPRansac
                                           re-solve / re-select rounds, 3-sigma threshold)        */
  /* Two-view bundle adjustment after each pass's motion estimate (myRegistrationVis.cpp:1192-1370; rtabmap
     Vis/BundleAdjustment, upstream default 1 when built with g2o): the inliers' 3D points (from-frame) and the pose of
     the "to" camera are refined against both frames' keypoints, the "from" pose fixed, Huber kernel; words whose
     reprojection stays beyond the kernel width are removed from the inliers (sbaOutliers, :1314-1330) and the
     min_inliers test is repeated (:1331-1336).                                                              */
  int32_t bundle_adjustment;       /* 0 (default here; north_star's path) = off, 1 = on (needs a calibrated camera) */
  int32_t ba_iterations;           /* 20   Optimizer/Iterations                                             */
  float   ba_robust_kernel_delta;  /* 8.0  g2o/RobustKernelDelta (pixels)                                   */
  float   ba_pixel_variance;       /* 1.0  g2o/PixelVariance                                                */
  float   stereo_baseline;         /* metres; > 0 adds the stereo (disparity) residual of points with depth  */
  /* Reg/Force3DoF (myRegistration.cpp:245-248,269-276; myRegistrationVis.cpp:1100-1102,1141-1143; rtabmap default
     false): guess and estimates are reduced to (x, y, yaw) -- Transform::to3DoF [upstream] = Transform(x, y, 0, 0, 0,
     yaw) with yaw = atan2(r21, r11), computed here as the rotation (r11, r21) / |(r11, r21)| about z.            */
  int32_t force_3dof;              /* 0 */
  /* Vis/ForwardEstOnly (myRegistrationVis.cpp:936-978,1155-1197,1369,1376-1394; rtabmap default true).  0: every pass
     also estimates to -> from (the frames' roles swapped, each direction behind its own gate); the pass's transform is
     interpolate(0.5) of the forward estimate and the inverse of the backward one, its covariance their mean, inliers /
     matches the union of both directions' ids.  With bundle_adjustment the forward transform is adjusted over the union
     of the inliers and the backward transform is dropped (:1369).  Both estimators; runs on the stage kernels.   */
  int32_t forward_est_only;        /* 1 */
  /* Descriptor type of every keyframe of this handle (rtabmap Vis/FeatureType is fixed per run).  0 = binary rows
     (CV_8U: BRIEF / ORB, Hamming distance -- the only kind the reference's own wire carries, MsgConversion.cpp:113-129);
     1 = float32 rows (SURF / SIFT: `desc` points at rows x dims float32, `cols` = 4 * dims with dims = 64 or 128):
     brute-force kNN-2 on the L2 distance with the same NNDR / uniqueness / window rules -- squared distances in the
     global matching (myRegistrationVis.cpp:839-854 -> VWDictionary::addNewWords [upstream]), cv::BFMatcher(NORM_L2)
     distances in the guided matching (:739-749).  north_star's "ORB/SURF ... Hamming/L2 matching".
     2 = uint8 rows compared by L2 (SIFT: `desc` points at rows x 128 uint8, `cols` = desc_bytes = 128; sf_create turns
     the default desc_bytes 32 into 128, any other width is SF_EINVAL): the rules and the results of type 1 on the same
     integers held as float32 -- a squared distance of 128 such differences is an integer below 2^24, exact in float32
     in any order -- computed in int32, the global matching on the int8 matrix cores (k_match_u8.hip).  A quarter of
     the bytes of type 1, and rows the reference's CV_8U wire can carry.  Stage kernels only, as type 1.             */
  int32_t desc_type;               /* 0 */
  /* Vis/CorGuessMatchToProjection: 0 = the guided pass matches every projected "from" point to the "to" keypoints in
     its window (myRegistrationVis.cpp:667-818); 1 = it matches every "to" keypoint to the projections in its window
     (:521-666; squared L2 distances for float32 rows, :580).  Any other value: sf_create -> SF_EINVAL.  With 1 every
     verification call runs on the stage kernels (or their two-stream halves under SF_OVERLAP).                      */
  int32_t guess_match_to_projection; /* 0 */
} sf_params;

/* ---- wire layouts ------------------------------------------------------------------------ */
/* rtabmap_ros/KeyPoint as carried by KeyPointVec.msg (fields per MsgConversion.cpp:50-56)   */
typedef struct sf_keypoint {
  float   x, y;        /* pt.x, pt.y (pixels) */
  float   size;
  float   angle;
  float   response;
  int32_t octave;
  int32_t class_id;
} sf_keypoint;         /* 28 bytes */

/* One keyframe's geometric features = (Descriptors, KeyPoint3DVec, KeyPointVec)            */
typedef struct sf_features {
  const uint8_t*     desc;      /* rows x cols, row-major (Descriptors.msg, zero-copy view
                                   exactly as MsgConversion.cpp:113-116)                     */
  uint16_t           rows;      /* Descriptors.rows */
  uint16_t           cols;      /* Descriptors.cols (bytes per descriptor) */
  const float*       xyz;       /* n3d x 3 float32, base frame (KeyPoint3DVec.kpts3DVec)     */
  int32_t            n3d;       /* KeyPoint3DVec.size ; must be 0 or rows                    */
  const sf_keypoint* kpts;      /* nkp entries (KeyPointVec.kptsVec)                         */
  int32_t            nkp;       /* KeyPointVec.size ; must equal rows (or 0 when rows==0)    */
} sf_features;

/* EstTransform.srv response + the RegistrationInfo fields the node keeps (info_)           */
typedef struct sf_result {
  double  position[3];     /* geometry_msgs/Pose.position                                   */
  double  orientation[4];  /* quaternion x,y,z,w (w >= 0, tf::poseEigenToMsg)               */
  double  covariance[36];  /* row-major 6x6, as memcpy'd by MsgConversion.cpp:61-64         */
  int32_t inliers;         /* RegistrationInfo.inliers of pass 2                            */
  int32_t matches;         /* RegistrationInfo.matches of pass 2                            */
  int32_t inliers_pass1;
  int32_t matches_pass1;
  uint8_t success;         /* !result2.isNull()  (stereoCamGeometricTools.cpp:168-175)      */
  uint8_t pass1_success;
  uint8_t pass2_guided;    /* 1 if pass 2 took the guess-guided branch                      */
  uint8_t pad[5];
} sf_result;               /* 368 bytes */

/* One row of ReceiveSeparators.srv, the record all-gathered across GPUs                    */
typedef struct sf_separator {
  int8_t  robot_from_id, robot_to_id;
  int16_t kf_id_from, kf_id_to;
  int16_t frame_id_from, frame_id_to;      /* frames_kepts_ids_* */
  uint8_t transform_est_success;
  uint8_t pad[5];
  double  position[3];
  double  orientation[4];
  double  covariance[36];
} sf_separator;            /* 360 bytes */

typedef struct sf_match {  /* one element of DataHandler.find_matches' return value         */
  int32_t idx_local;
  int32_t idx_other;
  double  distance;        /* Euclidean distance of the pair (float64)                      */
} sf_match;

typedef struct sf_context* sf_handle;

/* ---- lifecycle ----------------------------------------------------------------------------- */
int  sf_abi_version(void);
void sf_default_params(sf_params* p);
/* device: HIP device ordinal.  Fails with SF_ENODEV when no GPU is visible (no CPU fallback). */
int  sf_create(const sf_params* p, int device, sf_handle* out);
void sf_destroy(sf_handle h);
const char* sf_last_error(sf_handle h);   /* h may be NULL: last create() error              */
int  sf_get_params(sf_handle h, sf_params* out);
/* Make the handle issue all work on a caller-owned hipStream_t (e.g. torch's current stream).  Call it before the first
   sf_step_issue: the step pipeline picks its further streams relative to this one, once (see sf_stream_placement in
   sf_experimental.h); a stream set later is used, but the other streams are not picked again. */
int  sf_set_stream(sf_handle h, void* hip_stream);
int  sf_synchronize(sf_handle h);

/* ---- NetVLAD nearest-neighbour stage (data_handler.py:166-209, 297-301, 402-408, 437-438) --- */
/* Append n descriptors of `dim` float64 values (FindMatches.srv:1 wire type) to the local
   (self.local_descriptors) or received (self.received_descriptors) database.                */
int  sf_nn_append_local(sf_handle h, const double* desc, int32_t n, int32_t dim);
int  sf_nn_append_received(sf_handle h, const double* desc, int32_t n, int32_t dim);
/* Same, from float32 rows already resident in device memory (bulk ingest; MI355X-native).   */
int  sf_nn_append_local_f32_device(sf_handle h, const float* d_desc, int32_t n, int32_t dim);
int  sf_nn_append_received_f32_device(sf_handle h, const float* d_desc, int32_t n, int32_t dim);
/* The same for IEEE binary16 descriptors (BASELINE configs[4] ships NetVLAD in fp16): n x dim halfs in device
   memory, converted exactly to the fp32 database rows.                                                    */
int  sf_nn_append_local_f16_device(sf_handle h, const uint16_t* d_desc, int32_t n, int32_t dim);
int  sf_nn_append_received_f16_device(sf_handle h, const uint16_t* d_desc, int32_t n, int32_t dim);
int  sf_nn_sizes(sf_handle h, int32_t* n_local, int32_t* n_received);
/* local_kf_already_used.append / other_kf_already_used.append / add_frames_kept_pairs_to_ignore
   These three change the state every query reads: while sf_step_issue has steps in flight they first wait for ALL of
   them on the host (the steps were issued on the masks as they were) -- a caller that marks after every accepted
   match serialises the step pipeline; mark between retiring a batch of steps and issuing the next.  Arguments are
   validated before that wait; a step whose re-run failed makes the call return that error (the mask is untouched). */
int  sf_nn_mark_local_used(sf_handle h, int32_t idx_local);
int  sf_nn_mark_other_used(sf_handle h, int32_t idx_other);
int  sf_nn_ignore_pair(sf_handle h, int32_t idx_local, int32_t idx_other);
int  sf_nn_reset(sf_handle h);
/* Switch sf_params.nn_precision (0 / 1, see above) on a live handle; databases are kept.        */
int  sf_nn_set_precision(sf_handle h, int32_t nn_precision);
/* DataHandler.find_matches(): writes up to `cap` matches, *n_out = number found.
   Returns SF_EINVAL when either database is empty (the reference guards this at
   data_handler.py:308).                                                                     */
int  sf_nn_find_matches(sf_handle h, sf_match* out, int32_t cap, int32_t* n_out);
/* Per-row minima of the last find_matches call (diagnostics / tests): n_local entries.      */
int  sf_nn_last_row_minima(sf_handle h, double* dist, int32_t* idx, int32_t cap);
/* The sequential tail of DataHandler.find_matches (data_handler.py:191-205: rows sorted by their minimum, the
   walk with its "idx_other already taken" and break rules) on caller-provided per-row minima -- host work only.
   For a node that shards the LOCAL rows of one query over its GPUs: every rank searches its
   block (sf_nn_row_minima_device below), the minima are all-gathered, and every rank runs this
   identical walk.  row_min: n_local float64 (+inf = no candidate under the threshold), row_arg: column of each. */
int  sf_nn_walk(sf_handle h, const double* row_min, const int32_t* row_arg, int32_t n_local, int32_t n_received,
                sf_match* out, int32_t cap, int32_t* n_out);
/* The NN kernels of this handle's local rows (data_handler.py:166-189 on ONE rank's block of rows) WITHOUT the walk
   and without a host round trip: d_row_min[n_local] (float64) and d_row_arg[n_local] (int32) are DEVICE buffers
   (typically a slice of the all-gather's send block), filled asynchronously on the handle's stream; rows with no
   column under netvlad_distance report (+inf, 0) on the filter path.  With nn_precision 1 the prefix filter runs at
   the ladder level the handle last settled on; d_status[0] (device int32) = 1 when the candidate set was denser than
   that level's sparse limit -- the minima are then undefined and the caller takes sf_nn_find_matches +
   sf_nn_last_row_minima (which walks the ladder) -- and 0 otherwise.                                           */
int  sf_nn_row_minima_device(sf_handle h, double* d_row_min, int32_t* d_row_arg, int32_t* d_status);
/* The walk of sf_nn_walk ON THE DEVICE (data_handler.py:191-205), asynchronous on the handle's stream, for minima that
   are already there: d_row_min / d_row_arg as sf_nn_row_minima_device leaves them (or the all-gathered minima of a node
   that shards the local rows), d_status (may be NULL) a device int32 that voids the walk (0 matches) when non-zero.
   Writes up to `cap` matches, walk order, to d_matches and their number to d_n_matches[0]; both may be device memory
   or host-pinned memory the device can write.  netvlad_distance and netvlad_max_matches_nb are the handle's.     */
int  sf_nn_walk_device(sf_handle h, const double* d_row_min, const int32_t* d_row_arg, const int32_t* d_status,
                       int32_t n_local, int32_t n_received, sf_match* d_matches, int32_t cap, int32_t* d_n_matches);
/* Descriptor dimensions the fp16 filter contracted in the last find_matches call (0: exact path). */
int  sf_nn_last_filter_dims(sf_handle h, int32_t* dims);

/* ---- device-resident keyframe feature store (data_handler.py:268 geometric_feats) ----------- */
int  sf_store_add_keyframe(sf_handle h, const sf_features* f, int32_t* out_slot);
/* Bulk ingest from device memory: n keyframes, each with exactly `rows` features of `cols`
   bytes; d_desc [n][rows][cols] u8, d_xyz [n][rows][3] f32, d_kp [n][rows] sf_keypoint.     */
int  sf_store_add_keyframes_device(sf_handle h, int32_t n, int32_t rows, int32_t cols,
                                   const uint8_t* d_desc, const float* d_xyz,
                                   const sf_keypoint* d_kp, int32_t* out_first_slot);
int  sf_store_size(sf_handle h, int32_t* n_slots);
int  sf_store_clear(sf_handle h);

/* ---- store slots as bytes: export, import (csrc/k_store_wire.hip) --------------------------------------------------- */
/* A store slot holds exactly what verification reads -- descriptor rows, 3D points, {x, y, octave byte} per keypoint --
   so n consecutive slots are a complete message by themselves: the features one robot ships to another
   (GetFeatsAndDesc.srv), and what replicates a store over the GPUs of a node.  The blob is ONE contiguous,
   position-independent, little-endian block of bytes:

     [sf_kfblob_header][sf_kfblob_entry x n_keyframes][block of keyframe 0][block of keyframe 1] ...

   The block of a keyframe, at `offset` from the start of the blob:
     rows x cols descriptor bytes, tight (without the store's zero padding of a row to whole dwords);
     rows x 12 bytes of float xyz, absent when n3d == 0;
     rows x 12 bytes of {float x, float y, int32 octave}, the octave the sign-extended byte the store keeps;
   every part padded with zero bytes to a multiple of 16; a keyframe of 0 rows has an empty block.
   Canonical form (what export writes): blocks in slot order, tight, the first directly behind the table; all padding
   and reserved bytes zero -- the blob is a pure function of the slots' contents.  Float payloads are copied bit for
   bit.  size / angle / response / class_id of sf_keypoint are not in it: the store never held them.              */
#define SF_KFBLOB_MAGIC   0x424B4653u   /* "SFKB" */
#define SF_KFBLOB_VERSION 1
typedef struct sf_kfblob_header {
  uint32_t magic;        /* SF_KFBLOB_MAGIC; 0 in the header of an export that did not fit its buffer */
  uint16_t version;      /* SF_KFBLOB_VERSION */
  uint8_t  desc_type;    /* sf_params.desc_type of the exporting handle */
  uint8_t  reserved;     /* 0 */
  int32_t  n_keyframes;
  int32_t  max_rows;     /* the largest `rows` of the table */
  uint64_t total_bytes;  /* header + table + blocks (at byte 16: naturally aligned, so the struct has no hidden padding
                            and is 32 bytes under every compiler; a further int32 in front of it would make it 40) */
  uint64_t reserved2;    /* 0 */
} sf_kfblob_header;      /* 32 bytes */
typedef struct sf_kfblob_entry {
  int32_t  rows;
  int32_t  n3d;          /* 0 or rows */
  int32_t  cols;         /* descriptor bytes per row */
  int32_t  reserved;     /* 0 */
  uint64_t offset;       /* of the keyframe's block from the start of the blob; a multiple of 16 */
  uint64_t bytes;        /* length of the block */
} sf_kfblob_entry;       /* 32 bytes */
/* The size of the blob of slots [first_slot, first_slot + n): waits for the stream, *total_bytes and *max_rows (either
   may be NULL) are the header's.  n = 0 is SF_OK (a blob of 32 bytes); a range outside [0, sf_store_size) or
   n > 65535: SF_ERANGE.                                                                                           */
int  sf_store_export_plan(sf_handle h, int32_t first_slot, int32_t n, uint64_t* total_bytes, int32_t* max_rows);
/* Writes the blob of slots [first_slot, first_slot + n) to d_blob (device memory, 16-byte aligned, cap_bytes long):
   asynchronous on the handle's stream, no host wait, and independent of an earlier sf_store_export_plan (it plans again
   on the device).  A blob longer than cap_bytes is not written: only its header is (when cap_bytes >= 32), with magic
   0 and the total_bytes it would have taken, nothing else of d_blob is touched, and sf_store_wire_status reports bit 1. */
int  sf_store_export_keyframes_device(sf_handle h, int32_t first_slot, int32_t n, void* d_blob, uint64_t cap_bytes);
/* Appends the n keyframes of the blob at d_blob (device memory, 16-byte aligned, `bytes` long) to the store: the ragged
   form of sf_store_add_keyframes_device, asynchronous, no host wait.  n, max_rows and cols (a descriptor width of the
   store's class, e.g. the blob's largest) are what the caller knows of the blob on the host -- from
   sf_store_export_plan, or from the record that travelled ahead of the blob; they size the store exactly as
   sf_store_add_keyframes_device's do, with its refusals.  The call ALWAYS appends n slots.  The kernel checks the blob
   against these arguments and reads nothing outside [d_blob, d_blob + bytes), whatever the blob says:
     header: magic, version, desc_type of this handle, n_keyframes == n, 32 + 32 n <= total_bytes <= bytes -- else all
             n slots are left empty (status bit 2);
     entry:  0 <= rows <= max_rows, n3d 0 or rows, cols of the store's width class, offset a multiple of 16 and at or
             behind the table, offset + bytes <= total_bytes, bytes what rows, cols and n3d imply -- else this slot is
             left empty (status bit 4).
   An empty slot has meta {0, 0, 0, cols}.  An imported slot equals, bit for bit, the slot sf_store_add_keyframe makes
   of the same features.  n = 0 is SF_OK; n > 65535: SF_ERANGE.                                                     */
int  sf_store_import_keyframes_device(sf_handle h, const void* d_blob, uint64_t bytes, int32_t n, int32_t max_rows,
                                      int32_t cols, int32_t* out_first_slot);
/* What the most recent sf_store_export_keyframes_device or sf_store_import_keyframes_device call reported (each of the
   two resets it; sf_store_export_plan does not touch it): waits for the stream.  out[0]: bits 1 = the
   export did not fit cap_bytes, 2 = bad header, 4 = bad entry; out[1]: slots the import left empty; out[2]: the first of
   them (index into the blob), or -1; out[3]: 0.  SF_OK when out[0] is 0, else SF_ERANGE (out is filled either way).  */
int  sf_store_wire_status(sf_handle h, int32_t out[4]);

/* ---- a camera model per keyframe: stores that hold the keyframes of unlike cameras -------------------------------- */
/* The reference's registration takes two camera models, computeTransformationFromFeats(stereoCameraModelTo,
   stereoCameraModelFrom, ..) (myRegistrationVis.cpp:441-443); its service hands it one robot's camera for both
   (stereoCamGeometricTools.cpp:142-143), and sf_params carries that one camera.  A store that verifies across robots
   holds keyframes whose 3D points are in their own robot's base frame and whose keypoints are pixels of their own
   camera: the handle keeps a table of camera models and every store slot carries the id of the one it was taken with.
   Id 0 is the sf_params camera; a store whose slots all carry id 0 behaves exactly as a handle without a table.
   For a pair (from slot of camera X, to slot of camera Y):
     guided matching (both forms): eligible iff Y is valid for projection (:474); guessCameraRef = (guess L_Y)^-1
       (:486-487), projected through K_Y (:494) into Y's image (:505-506);
     PnP: camera B of the direction -- forward Y, backward (forward_est_only = 0) X (:950-978, :1058-1073) -- with that
       camera's calibrated gate;
     bundle adjustment: view 1 is X's model if X is valid, else Y's (:1277); view 2 is Y's; each view has its own K and
       baseline; invLocalTransformFrom comes from the TO model, as :1253 is written;
     3D-3D estimates read no camera.
   As soon as a slot of the store carries a non-zero id, verification calls on the store run the stage kernels
   (SF_FUSED=0's launches).  The scratch slots of sf_estimate_transform(_batch) always carry id 0.
   The blob of sf_store_export_* does not carry the ids: the camera is the receiver's knowledge.                    */
typedef struct sf_camera_model {
  double  fx, fy, cx, cy;
  int32_t image_width, image_height;   /* 0 => not valid for projection, as in sf_params */
  float   local_transform[12];         /* base <- camera optical frame, row-major 3x4 */
  float   stereo_baseline;             /* metres, >= 0; read by the bundle adjustment only */
  int32_t reserved;                    /* 0 */
} sf_camera_model;                     /* 96 bytes */
#define SF_MAX_CAMERAS 255             /* ids 1 .. 255 */
/* Adds a model to the handle's table and uploads it: *id_out = 1, 2, ..  Non-finite or negative intrinsics, a negative
   image size or baseline, a non-finite local_transform, reserved != 0: SF_EINVAL; a full table: SF_ERANGE.  Nothing
   changes on a refusal.                                                                                             */
int  sf_camera_add(sf_handle h, const sf_camera_model* m, int32_t* id_out);
/* The model behind an id; id 0 = the handle's sf_params camera.  An id outside the table: SF_EINVAL.                */
int  sf_camera_get(sf_handle h, int32_t id, sf_camera_model* out);
int  sf_camera_count(sf_handle h, int32_t* n_out);        /* models added (id 0 not counted) */
/* Slots appended from now on -- by sf_store_add_keyframe(s_device), every extraction and batch call,
   sf_store_import_keyframes_device -- carry this id.  A fresh handle: 0.                                            */
int  sf_camera_select(sf_handle h, int32_t id);
/* The id of slots [first_slot, first_slot + n) / of one slot.  A range outside the store: SF_EINVAL.  sf_store_clear
   drops the ids with the slots and keeps the table and the selection.                                               */
int  sf_store_set_camera(sf_handle h, int32_t first_slot, int32_t n, int32_t id);
int  sf_store_get_camera(sf_handle h, int32_t slot, int32_t* id_out);

/* ---- features of one stereo keyframe -------------------------------- */
/* replaces: RegistrationVis::getFeaturesImpl (myRegistrationVis.cpp:343-436: descriptors for the given keypoints,
   3D keypoints of the stereo pair, removal of keypoints without a finite 3D point) as called by
   StereoCamGeometricTools::getFeaturesAndDescriptor (stereoCamGeometricTools.cpp:100-120), writing the keyframe
   straight into the device-resident store.  Corner detection (sf_detect_corners_device) and the right-image
   position of every corner (sf_stereo_correspondences_device) are the two calls before this one.  */
typedef struct sf_stereo_camera {
  float fx, fy, cx, cy;        /* left camera (StereoCameraModel::left())                                  */
  float cx_right;              /* right camera cx (0: unknown, no principal-point correction)              */
  float baseline;              /* metres, > 0                                                              */
  float local_transform[12];   /* base <- camera optical frame, row-major 3x4 (CameraModel::localTransform) */
  float min_depth, max_depth;  /* Vis/MinDepth, Vis/MaxDepth; both 0 (the reference's defaults) keeps the
                                  keypoints whose 3D point is NaN                                          */
} sf_stereo_camera;
/* BRIEF test locations: [8 * bytes][4] int8 {x1, y1, x2, y2}, each within +-24 (the 48 px patch); bytes = 16, 32
   or 64.  A fresh handle holds a seeded Gaussian set (NOT OpenCV's table, which is not in the reference tree):
   install OpenCV's generated_<bytes>.i values here for descriptors identical to the reference build's.       */
int  sf_brief_set_pattern(sf_handle h, const int8_t* tests, int32_t bytes);
int  sf_brief_get_pattern(sf_handle h, int8_t* tests, int32_t cap_bytes, int32_t* bytes);
/* Vis/FeatureType of the three extraction calls (sf_extract_keyframe_device, sf_get_features_and_descriptor,
   sf_get_features_and_descriptor_batch_device).  6 = GFTT/BRIEF (a fresh handle; the BRIEF table above), 8 = GFTT/ORB:
   cv::ORB::compute on the given corners with rtabmap's ORB/ parameters, 32-byte rows -- one pyramid level, the 7 x 7
   sigma 2 blur in OpenCV's 8-bit fixed point, the pattern rotated by each keypoint's own angle (-1 degree for GFTT
   corners), the border filter KeyPointsFilter::runByImageBorder(ORB/EdgeThreshold) on cvRound(pt).  Corners whose
   octave & 255 is not 0 are dropped like border corners (one level: the pyramid is type 2's, sf_set_feature_type_orb
   below).  orb NULL = defaults.
   4 = FAST/BRIEF: the corners of sf_get_features_and_descriptor and its batch form come from the FAST detector below
   (the handle's sf_fast_params, det->max_features; quality_level / min_distance are validated and unused), everything
   after the detector is type 6's -- the same BRIEF table, the same border rule; a non-NULL orb is ignored.
   Any other feature_type or parameter, and 4 or 8 on a handle with desc_type 1, return SF_EINVAL -- 2 (ORB) included:
   it takes detector parameters and is selected by sf_set_feature_type_orb; 3 and 5 (FAST/FREAK, GFTT/FREAK) likewise
   take parameters of their own and are selected by sf_set_feature_type_freak, and 0 (SURF) by
   sf_set_feature_type_surf.                                                                                         */
typedef struct sf_orb_params {
  int32_t edge_threshold; /* ORB/EdgeThreshold, 19; 1 .. 64                                                         */
  int32_t patch_size;     /* ORB/PatchSize, 31 (only value accepted)                                                */
  int32_t wta_k;          /* ORB/WTA_K, 2 (only value accepted): 32-byte rows                                       */
  int32_t orientation;    /* 0 = the keypoint's own angle (rtabmap GFTT/ORB; GFTT gives -1);
                             1 = ORB's intensity-centroid angle on the unblurred image (radius-15 patch, fastAtan2),
                             written back into the keypoint of the wire copies; needs edge_threshold >= 16.  Not
                             rtabmap's GFTT/ORB: rows that do not change with an in-plane rotation of the image      */
} sf_orb_params;
void sf_orb_defaults(sf_orb_params* p);
int  sf_set_feature_type(sf_handle h, int32_t feature_type, const sf_orb_params* orb);   /* 4, 6 or 8 */
int  sf_get_feature_type(sf_handle h, int32_t* feature_type, sf_orb_params* orb);       /* orb may be NULL */
/* ORB test locations: [8 * bytes][4] int8 {x1, y1, x2, y2}, each within +-15 (the 31 px patch); bytes = 32.  Bit k of
   byte i is I(x1, y1) < I(x2, y2) of test 8 i + k, LSB first.  A fresh handle holds OpenCV's makeRandomPattern(31, 512)
   set (cv::RNG(0x34985739)) -- NOT OpenCV's bit_pattern_31_ table, which ORB uses: install that table here for
   descriptors identical to a reference build's.  Out-of-range coordinates or another size return SF_EINVAL.        */
int  sf_orb_set_pattern(sf_handle h, const int8_t* tests, int32_t bytes);
int  sf_orb_get_pattern(sf_handle h, int8_t* tests, int32_t cap_bytes, int32_t* bytes);
/* ---- NetVLAD descriptor inference --------------------------------- */
/* replaces: DataHandler.compute_descriptors (data_handler.py:143-164): `self.sess.run(self.net_out, ...)` of
   `nets.vgg16NetvladPca` (data_handler.py:63; netvlad_tf_open: VGG16 trunk to conv5_3, NetVLAD layer, WPCA), keeping
   the first n_out of the 4096 values like data_handler.py:157-158.  Weights come from the caller (the reference
   restores netvlad_tf_open's checkpoint, data_handler.py:70) in TensorFlow's own layouts:
     conv_kernel[i]   [3][3][Cin][Cout] (HWIO) of conv1_1, conv1_2, conv2_1, ... conv5_3 (13 layers), conv_bias[i] [Cout]
     average_rgb      [3]              assignment [512][clusters] (the 1 x 1 kernel, no bias)
     cluster_centers  [512][clusters]  wpca_kernel [512 * clusters][pca_dim], wpca_bias [pca_dim]                  */
typedef struct sf_netvlad_weights {
  const float* conv_kernel[13];
  const float* conv_bias[13];
  const float* average_rgb;
  const float* assignment;
  const float* cluster_centers;
  const float* wpca_kernel;
  const float* wpca_bias;
  int32_t      clusters;   /* 64 in the reference's network */
  int32_t      pca_dim;    /* 4096 */
} sf_netvlad_weights;
int  sf_netvlad_load(sf_handle h, const sf_netvlad_weights* w);      /* host pointers; copies and transposes */
/* d_image_rgb: [height][width][3] float32 on the device (the values the reference feeds its placeholder,
   data_handler.py:60-61); d_out: n_out floats = the first n_out values of the unit-norm descriptor, ready for
   sf_nn_append_local_f32_device.  Asynchronous on the handle's stream -- except the FIRST call at an image size,
   which measures every convolution layer in its tile / K-step configurations (about 40 ms, synchronous) and keeps
   the fastest for that size (neither changes the order of a pixel's sums: the descriptor's bits do not depend on it).                                                                                     */
int  sf_netvlad_infer_device(sf_handle h, const float* d_image_rgb, int32_t width, int32_t height, float* d_out,
                             int32_t n_out);
/* A batch, as DataHandler.compute_descriptors feeds the network (data_handler.py:149-156: up to netvlad_batch_size = 3
   queued images per call): n_images images of one size back to back in d_images_rgb, d_out [n_images][n_out].  Same
   bits per image as the single-image call; the WPCA matrix (537 MB) is read once per group of up to four images, and
   when the image height is a multiple of 16 the group's trunk runs as one vertical stack of its images (three times the
   workgroups in the late layers: 0.89 instead of 1.12 ms per 640 x 480 image at n_images = 3).  The first call with a
   given (size, stack height) measures its layer configurations like the single-image call does.                     */
int  sf_netvlad_infer_batch_device(sf_handle h, const float* d_images_rgb, int32_t n_images, int32_t width,
                                   int32_t height, float* d_out, int32_t n_out);

/* Corner detection of the reference's default feature type (rtabmap GFTT/BRIEF: Feature2D::generateKeypoints ->
   cv::goodFeaturesToTrack, called from myRegistrationVis.cpp:281-283), on the device: the response of the handle's
   sf_gftt_params below (a fresh handle: minimum eigenvalue, blockSize 3; Sobel 3 always), corners = local maxima above
   quality_level * max, strongest first, at least min_distance apart, at most max_corners (<= 0: no limit).  d_kpts_out
   receives up to `cap` keypoints {x, y, size = block_size (3), angle -1, response 0, octave 0, class_id -1} in that
   order; *n_out = corners found.  rtabmap's defaults: max_corners = Vis/MaxFeatures (1000), quality_level 0.001,
   min_distance 3.  width, height >= max(3, block_size).  Synchronises the stream twice (candidate count, result
   count).                                                                                                      */
int  sf_detect_corners_device(sf_handle h, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                              int32_t max_corners, double quality_level, double min_distance,
                              sf_keypoint* d_kpts_out, int32_t cap, int32_t* n_out);
/* The FAST detector of rtabmap's Vis/FeatureType 4 (FAST/BRIEF; also inside 2, sf_detect_orb_device below, and behind 3,
   FAST/FREAK, sf_set_feature_type_freak below):
   cv::FastFeatureDetector (FAST-9/16, TYPE_9_16) followed by Feature2D::limitKeypoints [both upstream, restated in
   tests/fast_ref.py].  With d_k = I(p) - I(p + ring_k) over the 16 pixels of the radius-3 circle, m(p) = the maximum
   over the 16 cyclic arcs of 9 consecutive k of max(min d, min -d); p is a corner iff m(p) > threshold, for
   3 <= x < width - 3 and 3 <= y < height - 3 (smaller images: no corners, not an error); its score is m(p) - 1.
   nonmax_suppression 1 keeps a corner iff its score is strictly greater than that of each of its 8 neighbours (plateaus
   vanish entirely); 0 keeps every corner, with response 0.  Keypoints {x, y, size 7, angle -1, response = score,
   octave 0, class_id -1}: in raster order (y, then x) when they number <= max_features or max_features <= 0, otherwise
   the max_features strongest by descending response, ties by descending raster index.  The grid-adaptive thresholds
   (FAST/GridRows, GridCols, MinThreshold, MaxThreshold) are not built: this is what a grid of 0 gives.             */
typedef struct sf_fast_params {
  int32_t threshold;           /* FAST/Threshold, 20; 1 .. 254                  */
  int32_t nonmax_suppression;  /* FAST/NonmaxSuppression, 1; 0 or 1             */
} sf_fast_params;
void sf_fast_defaults(sf_fast_params* p);
/* The handle's FAST parameters (what feature type 4 detects with); out-of-range values return SF_EINVAL and change
   nothing.                                                                                                        */
int  sf_fast_set_params(sf_handle h, const sf_fast_params* params);
int  sf_fast_get_params(sf_handle h, sf_fast_params* params);
/* The response of the GFTT detector (sf_detect_corners_device; Vis/FeatureType 5, 6 and 8): cv::cornerMinEigenVal /
   cv::cornerHarris of OpenCV 3.2 as cv::goodFeaturesToTrack calls them [upstream, restated in tests/gftt_ref.py; DESIGN.md
   section 3 lists what the restatement decides].  Sobel derivatives scaled by 1 / (4 * block_size * 255), their three
   products A = sum dx dx, B = sum dx dy, C = sum dy dy over the block_size x block_size window whose first row and column
   are y - block_size / 2 and x - block_size / 2 (BORDER_REFLECT_101; an even block leans up and left), float32, each
   window row summed left to right, the rows top to bottom.  use_harris_detector 0: (A / 2 + C / 2) -
   sqrt((A / 2 - C / 2)^2 + B^2); 1: A C - B^2 - k (A + C)^2, the products in float32, the term with k in double.  What
   follows the response (threshold, local maxima, order, min_distance) does not depend on the block; a Harris image with
   no positive response gives no corners, which is not an error.  Keypoints carry size = block_size, as
   cv::GFTTDetector's do.  Handle state: a fresh handle holds the defaults; out-of-range values (block_size 1 and above 15
   included) return SF_EINVAL, say why and change nothing.  An image, Vis/RoiRatios ROI or grid cell with a side below
   block_size is refused with SF_EINVAL by the call that detects on it.  Feature types 0 .. 4 do not read the block.   */
typedef struct sf_gftt_params {
  int32_t block_size;           /* GFTT/BlockSize, 3; 2 .. 15            */
  int32_t use_harris_detector;  /* GFTT/UseHarrisDetector, 0; 0 or 1     */
  double  k;                    /* GFTT/K, 0.04; finite, 0 <= k <= 1     */
} sf_gftt_params;
void sf_gftt_defaults(sf_gftt_params* p);
int  sf_gftt_set_params(sf_handle h, const sf_gftt_params* params);
int  sf_gftt_get_params(sf_handle h, sf_gftt_params* params);
/* Conventions of sf_detect_corners_device: d_kpts_out receives up to `cap` keypoints, *n_out = keypoints of the result
   (after the limit); width, height >= 3.  params NULL = the handle's.  Any image size up to 2^26 pixels.  Synchronises
   the stream twice (corner count, result count).                                                                  */
int  sf_detect_fast_device(sf_handle h, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                           int32_t max_features, const sf_fast_params* params, sf_keypoint* d_kpts_out, int32_t cap,
                           int32_t* n_out);
/* ORB on an image pyramid: rtabmap's Vis/FeatureType 2, cv::ORB (OpenCV 3.2) as rtabmap's ORB feature type drives it
   [both upstream, restated in tests/orb2_ref.py; DESIGN.md section 3 lists what the restatement decides].
   Detector: level l has scale_l = (float)pow(scale_factor, l) and cvRound(width / scale_l) x cvRound(height / scale_l)
   pixels, resized from level l - 1 with cv::resize(INTER_LINEAR)'s 8-bit arithmetic (the 2 x 2 mean when the level
   halves exactly, 11-bit fixed-point bilinear otherwise).  Per level: FAST-9/16 with fast_threshold and suppression,
   the border filter runByImageBorder(level size, edge_threshold), the per-level quota of nfeatures = max_features
   (geometric in 1 / scale_factor, float arithmetic, the last level takes the remainder), retainBest(2 quota) on the FAST
   score and retainBest(quota) on the Harris measure (block 7, k 0.04) under score_type 0, retainBest(quota) on the FAST
   score under score_type 1 -- ties at a cut all stay; survivors in raster order, levels ascending.  Keypoints {level
   position * scale_l, size 31 scale_l, intensity-centroid angle of the level, response, octave l, class_id -1}, then
   Feature2D::limitKeypoints(max_features) keyed by |response|: order unchanged up to max_features keypoints, otherwise
   the strongest first, ties by descending index.
   Descriptors (sf_extract_keyframe_device under type 2): cv::ORB::compute on the given keypoints -- border filter on
   the level-0 position; keypoints whose octave & 255 is not a level are dropped like border corners; rows grouped by
   level, ascending, order kept within a level (the row order of the keyframe); type 8's blur and steered pattern on the
   keypoint's own level around cvRound(position * (1.f / scale_l)), steered by the keypoint's own angle.
   sf_get_features_and_descriptor runs detector -> stereo correspondence (level-0 positions) -> descriptors;
   sf_orb_set_pattern serves type 2 as it serves 8.  A batch of keyframes under type 2 goes through calls of its own,
   sf_get_features_and_descriptor_orb_batch_device and sf_add_keyframes_orb_u8_batch_device (the generic batch calls
   return SF_EINVAL and name them).  NOT built for type 2: first_level != 0, WTA_K 3 / 4.                            */
typedef struct sf_orb_detector_params {
  float   scale_factor;    /* ORB/ScaleFactor, 2 (rtabmap's default, not OpenCV's 1.2); (1, 4]    */
  int32_t n_levels;        /* ORB/NLevels, 3 (rtabmap's default, not OpenCV's 8); 1 .. 8          */
  int32_t first_level;     /* ORB/FirstLevel, 0 (only value accepted)                             */
  int32_t score_type;      /* ORB/ScoreType, 0 = Harris, 1 = FAST                                 */
  int32_t fast_threshold;  /* ORB/FastThreshold, 20; 1 .. 254                                     */
} sf_orb_detector_params;
void sf_orb_detector_defaults(sf_orb_detector_params* p);
/* Selects Vis/FeatureType 2.  det NULL = defaults; orb NULL = defaults; orb->edge_threshold 16 .. 64 here (the
   radius-15 centroid patch and the radius-4 Harris window stay inside a level), orb->orientation is ignored: always
   the centroid (sf_get_feature_type reports 1).  sf_get_feature_type reports 2 afterwards; sf_set_feature_type(h, 4 | 6
   | 8, ...) switches back.  Out-of-range values and a handle with desc_type 1 return SF_EINVAL and change nothing.   */
int  sf_set_feature_type_orb(sf_handle h, const sf_orb_detector_params* det, const sf_orb_params* orb);
int  sf_get_orb_detector(sf_handle h, sf_orb_detector_params* out);
/* Conventions of sf_detect_fast_device.  det NULL = the handle's detector parameters, orb NULL = the handle's ORB
   parameters (both the defaults on a fresh handle).  Images smaller than 7 x 7 and levels not larger than 2
   edge_threshold give no keypoints, not an error.  Synchronises the stream twice (corner counts, result count).     */
int  sf_detect_orb_device(sf_handle h, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                          int32_t max_features, const sf_orb_detector_params* det, const sf_orb_params* orb,
                          sf_keypoint* d_kpts_out, int32_t cap, int32_t* n_out);
/* FREAK descriptors: rtabmap's Vis/FeatureType 3 (FAST/FREAK: the corners of the FAST detector above) and 5 (GFTT/FREAK:
   the corners of sf_detect_corners_device), cv::xfeatures2d::FREAK::compute on the given keypoints [upstream opencv_contrib,
   restated in tests/freak_ref.py; DESIGN.md section 3 item 17g lists what the restatement decides].  Rows are 64 bytes
   (512 bits) -- the store's one-width rule applies: a store that already holds 32-byte rows refuses them.
   Pattern: 43 receptive fields (rings of 6 6 6 6 6 6 6 1, the centre last) at 64 scales x 256 orientations; scale s
   multiplies the pattern by 2^(s n_octaves / 64).  Per keypoint: the scale index from its `size` (scale_normalized 1:
   max((int)(log(size / 7) * 64 / (LOG2 n_octaves) + 0.5), 0), at most 63; 0: the fixed index of size 21), the border test
   against that scale's pattern size (the keypoint is dropped when x <= P, y <= P, x >= width - P or y >= height - P), the
   43 field means (a box on BRIEF's integral image; 10-bit bilinear interpolation for fields with sigma < 0.5), the angle
   from 45 symmetric field pairs (orientation_normalized 1; else 0) -- written into the keypoint whatever it held -- and 512
   comparisons mean_i >= mean_j on the fields of the nearest of the 256 orientations.  Bit layout: upstream's SSE order,
   pair c = 128 q + 16 r + u (q < 4, r < 8, u < 16) is bit r (LSB = 0) of byte 16 q + 15 - u.
   Everything around the descriptor -- ROI, grid, sub-pixel refinement, LK or block matching, the camera-image forms, the
   3D points and the depth filter -- is what types 4 and 6 do; the keypoint's octave is not looked at.                */
typedef struct sf_freak_params {
  int32_t orientation_normalized;  /* FREAK/OrientationNormalized, 1; 0 or 1   */
  int32_t scale_normalized;        /* FREAK/ScaleNormalized, 1; 0 or 1         */
  float   pattern_scale;           /* FREAK/PatternScale, 22; (0, 64]          */
  int32_t n_octaves;               /* FREAK/NOctaves, 4; 1 .. 8                */
} sf_freak_params;                 /* 16 bytes */
void sf_freak_defaults(sf_freak_params* p);
/* Selects Vis/FeatureType 3 or 5 (freak NULL = defaults).  Another feature_type, out-of-range parameters and a handle
   with desc_type 1 return SF_EINVAL and change nothing.  sf_get_feature_type reports 3 / 5 afterwards;
   sf_set_feature_type(h, 4 | 6 | 8, ...) and sf_set_feature_type_orb switch back.  The pattern (8.4 MB of device memory)
   is built and uploaded by the first extraction after the parameters changed; a handle that never selects FREAK
   reserves nothing.  The two _orb_ batch calls refuse these types as they refuse every type but 2.                   */
int  sf_set_feature_type_freak(sf_handle h, int32_t feature_type /* 3 or 5 */, const sf_freak_params* freak);
int  sf_get_freak_params(sf_handle h, sf_freak_params* out);
/* The 512 description pairs in OpenCV's own format (cv::xfeatures2d::FREAK::create's selectedPairs, the values of
   FREAK_DEF_PAIRS): indices into the enumeration `for i in 1..42: for j in 0..i-1` of the 903 field pairs, index =
   i (i - 1) / 2 + j.  n != 512 or an index outside [0, 903) returns SF_ERANGE and changes nothing; duplicates are
   allowed, as upstream.  A fresh handle holds a GENERATED selection (sf_freak_default_pairs) -- NOT OpenCV's
   FREAK_DEF_PAIRS, which is in neither the reference tree nor OpenCV's main repository: install that table here for
   descriptors identical to a reference build's.  sf_freak_get_pairs: *n = 512; selected may be NULL, cap < 512 with
   selected set returns SF_ERANGE.                                                                                    */
int  sf_freak_set_pairs(sf_handle h, const int32_t* selected, int32_t n);
int  sf_freak_get_pairs(sf_handle h, int32_t* selected, int32_t cap, int32_t* n);
/* Handle-free host functions, usable without a GPU.  sf_freak_build_pattern: the table the kernel samples with, table
   [64 scales][256 orientations][43 points][3] = {x, y, sigma} float32 (float64 arithmetic, rounded once) and sizes [64],
   the border every scale asks for; p NULL = defaults; SF_EINVAL for out-of-range parameters.  Either output may be NULL.
   sf_freak_default_pairs: the first 512 values of a Fisher-Yates shuffle of 0 .. 902 -- for k = 0 .. 511: swap a[k] with
   a[k + next() % (903 - k)] -- driven by cv::RNG's multiply-with-carry step (s = (uint32)s * 4164903690 + (s >> 32),
   next() = (uint32)s) from the seed 0x46524B21.                                                                       */
int  sf_freak_build_pattern(const sf_freak_params* p, float* table, int32_t* sizes);
void sf_freak_default_pairs(int32_t* selected /* [512] */);
/* SURF: rtabmap's Vis/FeatureType 0, cv::xfeatures2d::SURF of OpenCV 3.2 with rtabmap's SURF/ parameters [upstream
   opencv_contrib, restated in tests/surf_ref.py; DESIGN.md section 3 item 17h lists what the restatement decides].  The
   only type with float32 rows: 64 dimensions (256 bytes), or 128 (512 bytes) with extended = 1, for a handle created
   with desc_type 1 and that desc_bytes -- the L2 matcher's rows.
   Detector (sf_detect_surf_device; usable on any handle, it writes no descriptor): box-filter Hessian layers of size
   (9 + 6 l) << o sampled every 1 << o pixels on the int32 integral image, l = 0 .. n_octave_layers + 1, o = 0 ..
   n_octaves - 1 (a layer larger than the image is skipped); det = dxx dyy - 0.81 dxy^2; a sample of a middle layer is a
   keypoint when its det exceeds hessian_threshold and all 26 neighbours, and the 3 x 3 solve for the sub-sample offset
   gives no component beyond 1.  Keypoint: the interpolated position, size = cvRound(size + offset ds), angle -1,
   response = det, octave = o, class_id = the sign of the trace.  Order: descending response, equal responses by layer
   then sample; then rtabmap's limitKeypoints (max_features <= 0: no limit), the rule of sf_detect_fast_device.  An image
   with more than 262144 maxima returns SF_ERANGE.  surf NULL = the handle's parameters.
   Under type 0 sf_extract_keyframe_device is SURF::compute on the given keypoints: it reads x, y and size and writes
   angle -- the dominant direction of the 109 Haar responses of side 2 cvRound(2 s), s = size 1.2 / 9, within radius 6 s
   (270 with upright = 1) -- and drops a keypoint whose wavelet is larger than the image, whose samples all fall outside
   it, or whose size is not in (0, 1e6); the row is the 4 x 4 x (4 | 8) sums of Gaussian-weighted gradients over the
   (int)(21 s) window reduced to 21 x 21, normalised to unit length.  d_desc_out receives rows x dims float32 through
   its uint8_t pointer.  3D points, the depth filter and the store slot are every other type's.
   sf_get_features_and_descriptor and its _u8 form run detector, sub-pixel refinement when it is on, LK or block matching,
   extraction.  NOT BUILT under type 0 and refused with SF_EINVAL: Vis/RoiRatios and a grid of cells (as under type 2).
   The batch forms are sf_get_features_and_descriptor_surf_batch_device and sf_add_keyframes_surf_u8_batch_device; the
   generic batch calls and the _orb_ ones refuse a type-0 handle with SF_EINVAL and name them.                        */
typedef struct sf_surf_params {
  float   hessian_threshold;   /* SURF/HessianThreshold, 500; >= 0 and finite  */
  int32_t n_octaves;           /* SURF/Octaves, 4; 1 .. 8                      */
  int32_t n_octave_layers;     /* SURF/OctaveLayers, 2; 1 .. 8                 */
  int32_t upright;             /* SURF/Upright, 0; 0 or 1                      */
  int32_t extended;            /* SURF/Extended, 0; 0 or 1: 128 dimensions     */
} sf_surf_params;              /* 20 bytes */
void sf_surf_defaults(sf_surf_params* p);
/* Selects Vis/FeatureType 0 (surf NULL = defaults).  Out-of-range parameters, a handle with desc_type 0, and a
   desc_bytes that is not 256 (extended 0) / 512 (extended 1) return SF_EINVAL and change nothing.  sf_get_feature_type
   reports 0 afterwards.  On a handle with desc_type 1 every other type stays refused: there is no way back, and none is
   needed.                                                                                                            */
int  sf_set_feature_type_surf(sf_handle h, const sf_surf_params* surf);
int  sf_get_surf_params(sf_handle h, sf_surf_params* out);
int  sf_detect_surf_device(sf_handle h, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                           int32_t max_features, const sf_surf_params* surf, sf_keypoint* d_kpts_out, int32_t cap,
                           int32_t* n_out);
/* SIFT: rtabmap's Vis/FeatureType 1, cv::xfeatures2d::SIFT of OpenCV 3.2 with rtabmap's SIFT/ parameters
   [upstream opencv_contrib, restated in tests/sift_ref.py; DESIGN.md section 3 item 17i lists what the restatement
   decides].  Rows are 128 float32 holding the integers 0 .. 255 (512 bytes), for a handle created with desc_type 1 and
   desc_bytes 512 -- the L2 matcher's rows.
   Detector (sf_detect_sift_device; usable on any handle, it writes no descriptor).  The uint8 image times 48 is enlarged
   2 x bilinearly into int16 fixed point and blurred to sigma; every octave (cvRound(log2(min side of the enlarged
   image) - 2) + 1 of them) holds n_octave_layers + 3 Gaussian planes, each blurred from its predecessor, and their
   n_octave_layers + 2 differences; the next octave starts from every second pixel of plane n_octave_layers.  A sample of
   a middle difference plane at least 5 pixels inside is a candidate when it exceeds floor(0.5 contrast_threshold /
   n_octave_layers 255 48) in magnitude and is >= (<=) all 26 neighbours; up to 5 steps of the 3 x 3 solve move it to the
   sample its offset is within half a step of, where |contrast| n_octave_layers >= contrast_threshold and the edge test
   tr^2 e < (e + 1)^2 det must hold.  Two candidates that converge to one sample give one keypoint.  A 36-bin gradient
   histogram of the keypoint's own Gaussian plane gives one keypoint per peak >= 0.8 of the maximum.  Keypoint: position
   and size in image pixels (halved from the enlarged image), angle in degrees, response = |contrast|, octave = (octave -
   1) & 255 | layer << 8 | cvRound((offset + 0.5) 255) << 16, class_id -1.  Order: descending response, equal responses
   by sample of the difference pyramid, then histogram bin; then one cut at the smaller positive of n_features
   (retainBest) and max_features (rtabmap's limitKeypoints; <= 0: no limit), with the rule of sf_detect_fast_device for
   equal responses.  An image with more than 262144 extrema or keypoints, or more than 2^26 difference samples, returns
   SF_ERANGE and writes nothing.  sift NULL = the handle's parameters (the defaults until sf_set_feature_type_sift).
   Under type 1 sf_extract_keyframe_device is SIFT::compute on the given keypoints: it builds the pyramid of the enlarged
   image (always: octave byte -1 is its first octave, whatever octaves the keypoints name), reads x, y, size, angle and
   octave (octave byte and layer name the Gaussian plane) and leaves the keypoint as it is; the row is the 4 x 4 x 8
   histogram of Gaussian-weighted gradients over the window of radius cvRound(3 scl sqrt(2) 2.5), scl = size / 2 in the
   plane's pixels, rotated by the angle, with trilinear votes; normalised, clamped at 0.2 of the norm, and scaled to
   0 .. 255.  Dropped: a keypoint whose octave byte or layer names no plane, whose size is not in (0, 1e6), whose |x| or
   |y| is not below 1e6, or whose angle is not in [0, 360].  d_desc_out receives rows x 128 float32 through its uint8_t
   pointer.  3D points, the depth filter and the store slot are every other type's.
   sf_get_features_and_descriptor and its _u8 form run detector, sub-pixel refinement when it is on, LK or block matching,
   extraction (which reuses the detector's pyramid).  The batch forms are sf_get_features_and_descriptor_sift_batch_device
   and sf_add_keyframes_sift_u8_batch_device; the batch calls of the other types refuse a type-1 handle (the batch form of
   type 1 is not built into them).  NOT BUILT under type 1 and refused with SF_EINVAL: Vis/RoiRatios and a grid of cells.
   On a handle created with desc_type 2 (desc_bytes 128) every one of these calls does the same and writes the row's 128
   integers as uint8 (128 bytes): the same keypoints, 3D points and row values, d_desc_out rows x 128 uint8.            */
typedef struct sf_sift_params {
  int32_t n_features;          /* SIFT/NFeatures, 0; >= 0                         */
  int32_t n_octave_layers;     /* SIFT/NOctaveLayers, 3; 1 .. 8                   */
  float   contrast_threshold;  /* SIFT/ContrastThreshold, 0.04; finite, >= 0      */
  float   edge_threshold;      /* SIFT/EdgeThreshold, 10; finite, > 0             */
  float   sigma;               /* SIFT/Sigma, 1.6; finite, in [0.8, 8]            */
} sf_sift_params;              /* 20 bytes */
void sf_sift_defaults(sf_sift_params* p);
/* Selects Vis/FeatureType 1 (sift NULL = defaults) on any handle with desc_type 1 and desc_bytes 512, whatever its current
   type (6, 0 with extended rows, or 1); sf_set_feature_type_surf with extended = 1 leads back likewise.  Also on a
   handle with desc_type 2 (uint8 rows; type 6 before, 1 after: no other type writes such rows).  Out-of-range
   parameters and any other handle return SF_EINVAL and change nothing.  sf_get_feature_type reports 1 afterwards.      */
int  sf_set_feature_type_sift(sf_handle h, const sf_sift_params* sift);
int  sf_get_sift_params(sf_handle h, sf_sift_params* out);
int  sf_detect_sift_device(sf_handle h, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                           int32_t max_features, const sf_sift_params* sift, sf_keypoint* d_kpts_out, int32_t cap,
                           int32_t* n_out);
/* The two steps rtabmap's Feature2D::generateKeypoints puts around every detector, whatever the feature type
   [upstream rtabmap / OpenCV 3.2, restated in tests/subpix_ref.py; DESIGN.md section 3 item 17d lists what the restatement
   decides].  The reference reaches that function at myRegistrationVis.cpp:282 and leaves both steps off (INTEGRATION.md
   section 12), and so does a fresh handle.
   ROI, Vis/RoiRatios {left, right, top, bottom}, each in [0, 1]: the detector is handed the sub-image
     x = 0; if (r0 > 0 && r0 < 1 - r1) x = (int)(W * r0);   w = W - x; if (r1 > 0 && r1 < 1 - r0) w = (int)((float)w - W * r1);
   (y, h alike from r2, r3, H; float arithmetic, truncating) as an image of its own -- pointer at its first pixel, its
   size, the parent's pitch -- and every keypoint is shifted back by (x, y).  The result equals a detection on a copy of the
   crop plus the offset: upstream's behaviour for FAST and ORB; for GFTT upstream's Sobel reads the parent's pixels
   across an interior ROI edge, which this does not (a listed deviation).  A ROI with a side below 3: SF_EINVAL.
   NOT built: a ROI under feature type 2 -- its batch form reuses the detector's pyramid for the descriptors, and a ROI
   would need a second pyramid; the extraction calls on a type-2 handle with any ratio != 0 return SF_EINVAL, say so
   and change nothing.
   Refinement, Vis/SubPixWinSize / Vis/SubPixIterations / Vis/SubPixEps: when subpix_win_size > 0 and
   subpix_iterations > 0, cv::cornerSubPix(image, pts, Size(win, win), Size(-1, -1), {COUNT + EPS, iterations, eps}) moves
   the kept keypoints on the FULL image; only x and y change.  Stereo correspondence, 3D points, the border filters
   and the descriptors see the refined positions.  Under type 2 the positions are level-0 coordinates.
   Both steps sit between the detector and the stereo correspondence of sf_get_features_and_descriptor, its _u8 form,
   sf_get_features_and_descriptor_batch_device, sf_add_keyframes_u8_batch_device and the two _orb_ batch calls (the batch
   forms stay one launch sequence with no host wait); with refinement on these calls need width, height >= 2 win + 5.
   The explicit sf_detect_*_device calls are untouched: their caller passes a sub-image itself.                      */
typedef struct sf_front_params {
  float   roi_ratios[4];      /* Vis/RoiRatios "0.0 0.0 0.0 0.0": left, right, top, bottom; each in [0, 1]        */
  int32_t subpix_win_size;    /* Vis/SubPixWinSize, 3; 0 .. 15, 0 = no refinement                                  */
  int32_t subpix_iterations;  /* Vis/SubPixIterations, 0 = no refinement; >= 0, clamped to 100 like cv::TermCriteria */
  float   subpix_eps;         /* Vis/SubPixEps, 0.02; compared squared with |step|^2, negative values count as 0     */
} sf_front_params;            /* 28 bytes */
void sf_front_defaults(sf_front_params* p);
/* The handle's parameters; out-of-range values (a ratio outside [0, 1] or NaN, win outside 0 .. 15, negative
   iterations, NaN eps) return SF_EINVAL and change nothing.                                                        */
int  sf_front_set_params(sf_handle h, const sf_front_params* params);
int  sf_front_get_params(sf_handle h, sf_front_params* params);
/* Feature2D::computeRoi as above, pure host code: roi_xywh = {x, y, width, height}.  SF_EINVAL for a ratio outside
   [0, 1], an image side < 1 or a ROI side < 3 (the rectangle is written whenever the ratios are valid).             */
int  sf_compute_roi(int32_t width, int32_t height, const float ratios[4], int32_t roi_xywh[4]);
/* The third step of Feature2D::generateKeypoints, Vis/GridRows x Vis/GridCols [upstream rtabmap 0.19 / 0.20, restated in
   tests/grid_ref.py; DESIGN.md section 3 item 17f lists what the restatement decides; the reference forwards both keys at
   myRegistrationVis.cpp:84-85 and 171-178].  With R = grid_rows, C = grid_cols and (X, Y, W, H) the rectangle of
   sf_compute_roi:
     row_size = H / R;  col_size = W / C;      (integer division: the W % C right-most columns and the H % R bottom rows of
                                                the ROI are seen by no cell)
     quota    = ceil((float)max_features / (float)(R * C))
     for i in 0 .. R-1, for j in 0 .. C-1:     (row-major)
       the detector on image(X + j col_size, Y + i row_size, col_size, row_size) as an image of its own, at most `quota`
       keypoints, shifted by the cell's origin, appended
   and then the refinement above on the full image.  A keyframe holds up to rows_cap = R C quota keypoints, which can
   exceed max_features (1000 on 3 x 3: 9 x 112 = 1008); upstream does not truncate and neither does this.
   Type 4: sf_detect_fast_device on the cell with max_features = quota (limitKeypoints); no corner within 3 px of a cell
   edge, cells below 7 x 7 give none.  Types 6 and 8: sf_detect_corners_device on the cell with max_corners = quota -- the
   cell's strongest corners at min_distance, against quality_level x the CELL's own maximum, the cell edge reflecting.
   That is a listed deviation: upstream hands GFTT the full Vis/MaxFeatures per cell and limitKeypoints then keeps the
   LAST quota of a list whose responses are all 0, the cell's weakest corners.
   NOT built: a grid under feature type 2 (as the ROI: a second pyramid); the extraction calls on a type-2 handle with a
   grid other than 1 x 1 return SF_EINVAL, say so and change nothing.  Not FAST/GridRows, FAST/GridCols (per-cell
   adaptive thresholds inside the FAST detector) either.
   The grid is honoured by sf_get_features_and_descriptor, its _u8 form, sf_get_features_and_descriptor_batch_device and
   sf_add_keyframes_u8_batch_device.  The batch forms stay one launch sequence with no host wait: the cells are the images
   of the detector's one batch launch, one more kernel joins their lists.  UNDER A GRID THE ROW STRIDE of the batch calls'
   per-keyframe outputs (d_desc_out, d_xyz_out, d_kpts_out) and the row capacity the store is given is rows_cap, not
   max_features (sf_compute_grid tells).  A call whose cells fall below 3 px returns SF_EINVAL, one whose rows_cap exceeds
   SF_MAX_FEATURES or whose n_keyframes R C exceeds 65535 SF_ERANGE, before the store or the NN database change.  A fresh
   handle has 1 x 1: no cell, no new launch, every byte as before.  The explicit sf_detect_*_device calls are untouched.  */
typedef struct sf_grid_params {
  int32_t grid_rows;      /* Vis/GridRows, 1; 1 .. 16                                                                  */
  int32_t grid_cols;      /* Vis/GridCols, 1; 1 .. 16                                                                  */
} sf_grid_params;         /* 8 bytes */
void sf_grid_defaults(sf_grid_params* p);
/* A value outside 1 .. 16 returns SF_EINVAL and changes nothing.                                                      */
int  sf_grid_set_params(sf_handle h, const sf_grid_params* params);
int  sf_grid_get_params(sf_handle h, sf_grid_params* params);
/* The cells as above, pure host code: out = {x, y, col_size, row_size, quota, rows_cap}, (x, y) the first cell's origin
   (the ROI's).  roi_ratios NULL = no ROI, grid NULL = 1 x 1.  SF_EINVAL for what sf_compute_roi refuses, a grid value
   outside 1 .. 16, max_features < 1 or a cell side below 3; SF_ERANGE when rows_cap > SF_MAX_FEATURES (out is written
   whenever the arguments before it are valid).                                                                        */
int  sf_compute_grid(int32_t width, int32_t height, const float roi_ratios[4], const sf_grid_params* grid,
                     int32_t max_features, int32_t out[6]);
/* cv::cornerSubPix on n keypoints of a device image, in place and asynchronous on the handle's stream; writes only x and
   y of each 28-byte record.  Per corner, from c = c0: the (2 win + 3)^2 float patch of cv::getRectSubPix around c
   (bilinear, taps outside the image clamped to the edge), central differences, the separable Gaussian mask
   exp(-(k - win)^2 / win^2) (evaluated on the host), five double sums over the (2 win + 1)^2 window in raster order, the 2 x 2
   solve; stops when |det| <= DBL_EPSILON^2, when c leaves the image, after clamp(iterations, 1, 100) steps or when a
   step's squared length is <= max(eps, 0)^2; a corner that moved more than win in x or y returns to c0.
   win 1 .. 15, iterations >= 1, width and height >= 2 win + 5 (OpenCV asserts this), else SF_EINVAL; n = 0 is SF_OK.     */
int  sf_corner_subpix_device(sf_handle h, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                             sf_keypoint* d_kpts, int32_t n, int32_t win, int32_t iterations, float eps);
/* Stereo correspondence of the corners: replaces Feature2D::generateKeypoints3D's call of
   StereoOpticalFlow::computeCorrespondences [upstream rtabmap] behind myRegistrationVis.cpp:382 --
   cv::calcOpticalFlowPyrLK(left, right, corners, winSize, maxLevel, {COUNT + EPS, iterations, epsilon},
   OPTFLOW_LK_GET_MIN_EIGENVALS, min_eig_threshold) followed by the disparity gate (status = 0 where left.x - right.x
   is <= min_disparity or > max_disparity).  sf_stereo_flow_defaults fills rtabmap's defaults: Stereo/WinWidth 15,
   Stereo/WinHeight 3, Stereo/MaxLevel 5 (3 before rtabmap 0.20), Stereo/Iterations 30, Stereo/Eps 0.01,
   Stereo/MinDisparity 0.5, Stereo/MaxDisparity 128, threshold 1e-4.                                              */
typedef struct sf_stereo_flow_params {
  int32_t win_width, win_height;    /* > 2 each, win_width * win_height <= 1024                      */
  int32_t max_level;                /* 0 .. 15; fewer levels are used when the image is small         */
  int32_t iterations;               /* clamped to 0 .. 100 like cv::TermCriteria in calcOpticalFlowPyrLK */
  double  epsilon;                  /* clamped to 0 .. 10, compared squared with |delta|^2            */
  float   min_disparity, max_disparity;
  float   min_eig_threshold;
} sf_stereo_flow_params;
void sf_stereo_flow_defaults(sf_stereo_flow_params* p);
/* d_left / d_right: rectified 8-bit images on the device (height rows of `pitch` bytes); d_kpts: n corners of the
   left image (sf_detect_corners_device's output).  Outputs on the device, asynchronous on the handle's stream:
   d_right_xy [n][2] (cv::Point2f of every corner in the right image), d_status [n], d_right_x [n] (optional: the x
   alone, the layout sf_extract_keyframe_device takes), d_err [n] (optional: the minimum eigenvalue of the level-0
   window, what calcOpticalFlowPyrLK returns as err under OPTFLOW_LK_GET_MIN_EIGENVALS).  params NULL = defaults.  */
int  sf_stereo_correspondences_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right, int32_t width,
                                      int32_t height, int32_t pitch, const sf_keypoint* d_kpts, int32_t n,
                                      const sf_stereo_flow_params* params, float* d_right_xy, uint8_t* d_status,
                                      float* d_right_x, float* d_err);
/* The second stereo correspondence of rtabmap's Stereo class, Stereo/OpticalFlow = false: Stereo::computeCorrespondences
   -> util2d::calcStereoCorrespondences [upstream rtabmap, restated in tests/stereo_bm_ref.py; DESIGN.md section 3 item
   17e lists what the restatement decides].  Block matching along the row of a rectified pair: on the pyramid of the LK path,
   from the last level down, the window of win_width x win_height around (int)(x / 2^level) is compared with the
   right-image windows of every disparity candidate of the level's range (exact integer sums of squared or absolute
   differences; the smallest POSITIVE score wins, the earliest on a tie) and a winner above level 0 narrows the range; the
   level-0 winner is refined by bisection (step 0.5, halved whenever neither neighbour is better, `iterations` steps,
   clamped to 0 .. 100) on float32 scores of bilinear patches; a step that leaves left.x - right.x <= min_disparity ends the
   loop with status 0.  There is no maximum-disparity gate behind the search (upstream has none).  A corner without a
   level-0 winner -- window outside the image, empty range, no positive score, a coordinate that is not finite -- gets
   status 0, position (0, 0), right_x 0 and score -1.
   The handle's sf_stereo_params choose between the two for sf_get_features_and_descriptor, its _u8 form,
   sf_get_features_and_descriptor_batch_device, sf_add_keyframes_u8_batch_device and the two _orb_ batch calls: with
   optical_flow = 0 their stereo stage is block matching on the same `flow` argument (NULL = the same defaults), the batch
   forms stay one launch sequence with no host wait, and a `flow` that block matching refuses makes the call return
   SF_EINVAL before the store or the NN database change.  A fresh handle has {1, 1}: pyramidal LK, as before.          */
typedef struct sf_stereo_params {
  int32_t optical_flow;   /* Stereo/OpticalFlow, 1 = pyramidal LK, 0 = block matching                                  */
  int32_t ssd;            /* Stereo/SSD, 1 = squared differences, 0 = absolute differences; block matching only       */
} sf_stereo_params;       /* 8 bytes */
void sf_stereo_defaults(sf_stereo_params* p);
/* Values other than 0 or 1 return SF_EINVAL and change nothing.                                                      */
int  sf_stereo_set_params(sf_handle h, const sf_stereo_params* params);
int  sf_stereo_get_params(sf_handle h, sf_stereo_params* params);
/* Block matching on n corners, the conventions of sf_stereo_correspondences_device: asynchronous on the handle's stream,
   params NULL = sf_stereo_flow_defaults, d_right_x [n] and d_score [n] optional (d_score: the score at the position found,
   the level-0 integer score when no bisection step improved on it).  Reads win_width, win_height, max_level, iterations,
   min_disparity and max_disparity of `params`; epsilon and min_eig_threshold are ignored.  ssd: 1 or 0 as above.
   SF_EINVAL for an even window side, a window above 1024 pixels, disparities that are not finite or violate
   0 <= min <= max, floor(max_disparity) > 1024 or ssd outside {0, 1}; SF_ERANGE for max_level outside 0 .. 15; a refused
   call changes nothing.  n = 0 is SF_OK.  Windows whose right-image strip does not fit the kernel's LDS budget run on
   a slower path that reads global memory.                                                                             */
int  sf_stereo_block_match_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right, int32_t width, int32_t height,
                                  int32_t pitch, const sf_keypoint* d_kpts, int32_t n, const sf_stereo_flow_params* params,
                                  int32_t ssd, float* d_right_xy, uint8_t* d_status, float* d_right_x, float* d_score);
/* d_left: 8-bit image on the device (height rows of `pitch` bytes); d_kpts: n corners; d_right_x: their x in the
   right image (NULL: no 3D); d_status: per-corner validity of d_right_x (NULL: all valid).  Appends ONE keyframe
   to the store; *out_slot = its slot, *out_rows = features kept (the call synchronises the stream to read it;
   pass NULL to stay asynchronous).  Optional copies for the wire (GetFeatsAndDesc response), device pointers
   sized for n rows, any may be NULL: d_desc_out [n][bytes], d_xyz_out [n][3], d_kpts_out [n].               */
int  sf_extract_keyframe_device(sf_handle h, const uint8_t* d_left, int32_t width, int32_t height, int32_t pitch,
                                const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status,
                                int32_t n, const sf_stereo_camera* cam, int32_t* out_slot, int32_t* out_rows,
                                uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out);
/* The GetFeatsAndDesc service handler in ONE call on host buffers -- replaces the body of
   StereoCamGeometricTools::getFeaturesAndDescriptor (stereoCamGeometricTools.cpp:100-120: SensorData(img_l, img_r, cam_),
   registrationPipeline_->getFeatures(...) = myRegistrationVis.cpp:190-439, then the three ...ToROS conversions):
   sf_detect_corners_device -> sf_stereo_correspondences_device -> sf_extract_keyframe_device on device copies of the
   pair.  left / right: rectified MONO8 images in host memory (what cv_bridge::toCvCopy returns at :104-105), `pitch`
   bytes per row.  det NULL = rtabmap's defaults (Vis/MaxFeatures 1000, GFTT/QualityLevel 0.001, GFTT/MinDistance 3),
   flow NULL = its Stereo/ defaults.  Outputs in host memory, sized for cap_rows rows (any may be NULL): desc_out
   [rows][bytes of the active feature type: the BRIEF table's, 32 for ORB], xyz_out [rows][3], kpts_out [rows];
   *rows_out = features of the keyframe (may exceed cap_rows: only cap_rows are copied); *slot_out (optional) = its slot in the device-resident store, what
   sf_verify_pairs refers to later.  Synchronous.                                                              */
typedef struct sf_detector_params {
  int32_t max_features;      /* 1 .. 32767 (KeyPointVec.size is an int16) */
  double  quality_level;
  double  min_distance;
} sf_detector_params;
void sf_detector_defaults(sf_detector_params* p);
int  sf_get_features_and_descriptor(sf_handle h, const uint8_t* left, const uint8_t* right, int32_t width, int32_t height,
                                    int32_t pitch, const sf_stereo_camera* cam, const sf_detector_params* det,
                                    const sf_stereo_flow_params* flow, uint8_t* desc_out, float* xyz_out,
                                    sf_keypoint* kpts_out, int32_t cap_rows, int32_t* rows_out, int32_t* slot_out);

/* A batch of keyframes: n_keyframes rectified MONO8 pairs of one size already in DEVICE memory
   (pair i at d_left / d_right + i * image_stride bytes), through the same three stages as sf_get_features_and_descriptor
   in ONE launch sequence -- every stage runs once over the whole batch, the corner counts stay in device memory between
   the stages, and the host is never waited for (asynchronous on the handle's stream).  The keyframes land in the store
   slots *first_slot_out .. + n_keyframes - 1; per keyframe the results are the single call's, byte for byte.  Optional
   device outputs, each sized for n_keyframes x det->max_features rows (keyframe i at row i * max_features; any may be
   NULL): d_rows_out [n_keyframes] features kept, d_desc_out, d_xyz_out, d_kpts_out as in the single call.  Images up to
   about 1.2 Mpixel (the corner selection keeps its bitmap in LDS); no such limit under feature type 4.
   Feature types 2, 0 and 1 have batch calls of their own, sf_get_features_and_descriptor_orb_batch_device,
   sf_get_features_and_descriptor_surf_batch_device and sf_get_features_and_descriptor_sift_batch_device: on a handle of
   one of these types this one returns SF_EINVAL, says so and changes nothing.                                                                                                 */
int  sf_get_features_and_descriptor_batch_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right,
                                                 int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                                 size_t image_stride, const sf_stereo_camera* cam,
                                                 const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                                 int32_t* first_slot_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                 float* d_xyz_out, sf_keypoint* d_kpts_out);
/* The same under Vis/FeatureType 2 (sf_set_feature_type_orb; the handle's detector and ORB parameters): arguments,
   outputs, limits and refusals of sf_get_features_and_descriptor_batch_device, and per keyframe the bytes of
   sf_get_features_and_descriptor under type 2 -- keypoint order, rows grouped by level and the store slot included.  One
   launch sequence with no host wait: the pyramids of all images are built once (the extraction reads the detector's),
   FAST runs once per level over the batch, the per-level counts, cuts and segment bounds stay on the device and the
   three sorts of the selection are segmented sorts.  The workspace is sized from the image size, n_keyframes and
   max_features alone and never truncates an image's candidates (6.7 MB per 752 x 480 pair at three levels of scale 2:
   DESIGN.md section 3 item 17b).  It also refuses what sf_detect_orb_device refuses (an empty pyramid level:
   SF_ERANGE).  On a handle of any other feature type: SF_EINVAL, the message names the generic call, nothing changes.
   A refused call leaves the store, the NN database, the feature type and the detector parameters as they were.       */
int  sf_get_features_and_descriptor_orb_batch_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right,
                                                     int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                                     size_t image_stride, const sf_stereo_camera* cam,
                                                     const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                                     int32_t* first_slot_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                     float* d_xyz_out, sf_keypoint* d_kpts_out);
/* The same under Vis/FeatureType 0 (sf_set_feature_type_surf; the handle's SURF parameters): arguments and outputs of
   sf_get_features_and_descriptor_batch_device, and per keyframe the bytes of sf_get_features_and_descriptor under type 0
   -- the row count, float32 rows of 256 or 512 bytes (d_desc_out receives them through its uint8_t pointer, keyframe i
   at row i * max_features), 3D points with their NaNs, keypoints with all seven fields, the store slot.  One launch
   sequence with no host wait: the integral images of all left images are built once (the extraction reads the
   detector's); the fast-Hessian layers, the maxima, the per-image decisions the single call takes on the host (the cut
   at max_features and the order of equal responses that goes with it), a segmented sort and the keypoints run over
   chunks of images whose planes and keys fit a fixed workspace of 256 MB (one image always runs; the chunks are
   consecutive launches on the handle's stream); sub-pixel refinement, LK or block matching and the extraction follow as
   in the single call.
   An image's key capacity is min(262144, B), B a bound on the maxima an image of this size can have (two maxima of a
   layer are never 8-adjacent: DESIGN.md section 3 item 17h); up to about a megapixel B is the smaller and nothing can
   overflow.  Beyond that, a keyframe with more maxima than the capacity is NOT truncated and does not fail the call,
   which cannot wait for the count: it gets 0 rows and an empty store slot, and sf_surf_batch_status reports it.
   Refusals, all before the first launch and without a change to the store, the NN database or the handle: what
   sf_get_features_and_descriptor_batch_device refuses; Vis/RoiRatios and a grid (SF_EINVAL); n_keyframes > 65535
   (SF_ERANGE: the image is a grid dimension); what sf_detect_surf_device refuses (the parameter ranges, more than 2^31
   plane samples, an image too large for a 32-bit integral image).  On a handle of any other feature type: SF_EINVAL, the
   message names the call to use.  n_keyframes = 0: SF_OK with *first_slot_out = sf_store_size.                      */
int  sf_get_features_and_descriptor_surf_batch_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right,
                                                      int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                                      size_t image_stride, const sf_stereo_camera* cam,
                                                      const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                                      int32_t* first_slot_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                      float* d_xyz_out, sf_keypoint* d_kpts_out);
/* Waits for the handle's stream and writes how many keyframes of the most recent SURF batch call (either form) had more
   maxima than their key capacity and therefore hold no rows.  SF_OK when none did (and on a handle that has run no such
   call); SF_ERANGE when some did, with a message that says to raise hessian_threshold.  n_overflowed_out may be NULL.  */
int  sf_surf_batch_status(sf_handle h, int32_t* n_overflowed_out);
/* The same under Vis/FeatureType 1 (sf_set_feature_type_sift; the handle's SIFT parameters): arguments and outputs of
   sf_get_features_and_descriptor_batch_device, and per keyframe the bytes of sf_get_features_and_descriptor under type 1
   -- the row count, 128 float32 per row (d_desc_out receives them through its uint8_t pointer, keyframe i at row i *
   max_features), 3D points with their NaNs, keypoints with all seven fields, the store slot.  One launch sequence with
   no host wait.  The Gaussian planes the rows are computed from are too large to keep for a whole batch (23 MB per
   752 x 480 image), so the WHOLE chain -- pyramid, extrema, orientation, the per-image decisions the single call takes
   on the host (overflow, the one cut at the smaller of n_features and max_features with the order of equal responses
   that goes with it), a segmented sort, the keypoints, sub-pixel refinement, LK or block matching, the rows -- runs over
   chunks of images whose planes and keys fit a fixed workspace of 1 GB (one image always runs; the chunks are
   consecutive launches on the handle's stream; every kernel of the pyramid takes the image of the chunk as a grid
   dimension).  The one wait: when n_octave_layers or sigma differ from the blur tables on the handle, the tables are
   uploaded before the first launch.
   An image holds at most 262144 extrema and 262144 keypoints (no smaller bound is known: equal neighbours count as
   extrema).  A keyframe with more of either is NOT truncated and does not fail the call, which cannot wait for the
   count: it gets 0 rows and an empty store slot, and sf_sift_batch_status reports it.
   Refusals, all before the first launch and without a change to the store, the NN database or the handle: what
   sf_get_features_and_descriptor_batch_device refuses; Vis/RoiRatios and a grid (SF_EINVAL, "not built"); n_keyframes >
   65535 (SF_ERANGE); what sf_detect_sift_device refuses (the parameter ranges, an image side outside 3 .. 16384, more
   than 2^26 difference samples).  On a handle of any other feature type: SF_EINVAL, the message names the call to use.
   n_keyframes = 0: SF_OK with *first_slot_out = sf_store_size.                                                        */
int  sf_get_features_and_descriptor_sift_batch_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right,
                                                      int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                                      size_t image_stride, const sf_stereo_camera* cam,
                                                      const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                                      int32_t* first_slot_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                      float* d_xyz_out, sf_keypoint* d_kpts_out);
/* Waits for the handle's stream and writes how many keyframes of the most recent SIFT batch call (either form) had more
   extrema or keypoints than an image holds and therefore hold no rows.  SF_OK when none did (and on a handle that has
   run no such call); SF_ERANGE when some did, with a message that says to raise contrast_threshold.  n_overflowed_out
   may be NULL.                                                                                                        */
int  sf_sift_batch_status(sf_handle h, int32_t* n_overflowed_out);

/* ---- keyframes from the camera's own images (first step) ------------------------- */
/* The reference keeps every image as cv_bridge's "rgb8" (data_handler.py:114-141).  For a keyframe it converts both stereo
   images with cv2.cvtColor(image, cv2.COLOR_RGB2GRAY) before GetFeatsAndDesc (data_handler.py:424-428) and feeds the uint8
   RGB image, unscaled, to the network's float placeholder (data_handler.py:60-61, 149-154).  The calls below take such
   images -- 8-bit, interleaved, `pitch` bytes per row -- and do both conversions on the device; no float image and, in the
   batch form, no host step lies between the camera's bytes and the keyframe.                                       */
enum sf_image_format {
  SF_IMAGE_RGB8 = 0,   /* 3 bytes per pixel: R, G, B (what the reference's queues hold); pitch >= 3 * width          */
  SF_IMAGE_BGR8 = 1,   /* 3 bytes per pixel: B, G, R; pitch >= 3 * width                                            */
  SF_IMAGE_MONO8 = 2   /* 1 byte per pixel; pitch >= width.  Gray = the byte; the network sees it in all 3 channels   */
};
/* The coefficients of the colour-to-gray conversion, gray = (R kr + G kg + B kb + (1 << (shift - 1))) >> shift in int32
   [upstream OpenCV, restated in tests/image_ref.py; as remembered, not from the reference tree: DESIGN.md section 3]:
     rule 0 (a fresh handle)  OpenCV 3.x: kr 4899, kg 9617, kb 1868, shift 14 -- the reference's python2 / ROS1 era and
                              the OpenCV 3.2 the rest of the front end restates
     rule 1                   OpenCV 4.x: kr 9798, kg 19235, kb 3735, shift 15
   Both sets sum to 1 << shift: (v, v, v) gives v, which is why mono8 is a copy.  Any other rule: SF_EINVAL, nothing
   changes.                                                                                                         */
int  sf_image_set_gray_rule(sf_handle h, int32_t rule);
int  sf_image_get_gray_rule(sf_handle h, int32_t* rule);
/* cv2.cvtColor(..., COLOR_RGB2GRAY / COLOR_BGR2GRAY) of n_images device images of one size under the handle's rule, one
   launch, asynchronous on the handle's stream: image i at d_src + i * src_stride (rows of src_pitch bytes) to the plane at
   d_dst + i * dst_stride (rows of dst_pitch >= width bytes).  Any pitches, strides (>= the rows they hold; ignored when
   n_images = 1) and base alignments; bytes outside the width x height planes are not written.  SF_IMAGE_MONO8: a pitched
   copy.  The planes are what sf_detect_*_device, sf_stereo_correspondences_device, sf_extract_keyframe_device and
   sf_get_features_and_descriptor_batch_device take.  Unknown format, pitch below a row: SF_EINVAL.                  */
int  sf_image_to_gray_device(sf_handle h, const uint8_t* d_src, int32_t format, int32_t width, int32_t height,
                             int32_t src_pitch, size_t src_stride, int32_t n_images, uint8_t* d_dst, int32_t dst_pitch,
                             size_t dst_stride);
/* sf_netvlad_infer_batch_device on 8-bit images: image i at d_images + i * image_stride, rows of `pitch` bytes.  The
   first convolution reads the bytes itself ((float)byte - average_rgb[c]; channels exchanged for bgr8, the one channel
   three times for mono8): the descriptors carry the bits of sf_netvlad_infer_batch_device on a float32 copy of the same
   values, at a quarter of the image bytes.  Same limits, same first-call measurement per image size.                */
int  sf_netvlad_infer_u8_batch_device(sf_handle h, const uint8_t* d_images, int32_t format, int32_t n_images,
                                      int32_t width, int32_t height, int32_t pitch, size_t image_stride, float* d_out,
                                      int32_t n_out);
/* sf_get_features_and_descriptor on the images DataHandler.compute_geom_features receives (data_handler.py:424-435):
   left / right in HOST memory in `format`, `pitch` bytes per row.  The pair is uploaded as it is and converted on the
   device under the handle's rule; from there on it is sf_get_features_and_descriptor's own code, under every feature type
   that call serves (6, 8, 4, 2): outputs, store slot and limits are the same, byte for byte what the gray call returns
   for the converted pair.  Synchronous.                                                                            */
int  sf_get_features_and_descriptor_u8(sf_handle h, const uint8_t* left, const uint8_t* right, int32_t format,
                                       int32_t width, int32_t height, int32_t pitch, const sf_stereo_camera* cam,
                                       const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                       uint8_t* desc_out, float* xyz_out, sf_keypoint* kpts_out, int32_t cap_rows,
                                       int32_t* rows_out, int32_t* slot_out);
/* What get_keyframes + compute_descriptors leave behind for n_keyframes keyframes (data_handler.py:143-164, 268) in ONE
   launch sequence with no host wait, asynchronous on the handle's stream: device images in `format` of one size, keyframe
   i's left / right / rgb image at d_left / d_right / d_rgb + i * image_stride (rows of `pitch` bytes; d_rgb NULL = the
   left images, as on a robot without a separate colour camera).
     geometric_feats   all 2 n stereo images become gray planes in one launch, then the stages of
                       sf_get_features_and_descriptor_batch_device write n store slots from *first_slot_out on
     local_descriptors the network runs on d_rgb; the first params.netvlad_dimensions values of every descriptor are
                       appended as n local NN rows from *first_nn_row_out on
   Slot first_slot + i and local row first_nn_row + i are the same keyframe: the reference's one index
   geometric_feats[i] <-> local_descriptors[i].  d_rows_out, d_desc_out, d_xyz_out, d_kpts_out: the optional device
   outputs of sf_get_features_and_descriptor_batch_device.
   All or nothing: arguments, the loaded model against netvlad_dimensions and the NN database's dimension are checked, and
   the store slots, the NN rows and the call's own buffers reserved, before the first launch; the store and the NN
   database grow last, together.  A refused call leaves sf_store_size and sf_nn_sizes as they were.  It refuses what sf_get_features_and_descriptor_batch_device
   refuses, with the same code and message (feature type 2 among them: its twin is sf_add_keyframes_orb_u8_batch_device),
   and what sf_netvlad_infer_u8_batch_device refuses; no model, or netvlad_dimensions beyond the model's WPCA width:
   SF_EINVAL.                                                                                                         */
int  sf_add_keyframes_u8_batch_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right, const uint8_t* d_rgb,
                                      int32_t format, int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                      size_t image_stride, const sf_stereo_camera* cam, const sf_detector_params* det,
                                      const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                      int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out,
                                      sf_keypoint* d_kpts_out);
/* The same under Vis/FeatureType 2: sf_add_keyframes_u8_batch_device with the feature stages of
   sf_get_features_and_descriptor_orb_batch_device -- the same formats and gray rule, the same network call, n store slots
   and n NN rows under one index, all or nothing.  Slot first_slot + i holds the bytes of sf_get_features_and_descriptor_u8
   on pair i.  Refuses what either of the two refuses; on a handle of another feature type: SF_EINVAL, nothing changes. */
int  sf_add_keyframes_orb_u8_batch_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right, const uint8_t* d_rgb,
                                          int32_t format, int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                          size_t image_stride, const sf_stereo_camera* cam, const sf_detector_params* det,
                                          const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                          int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                          float* d_xyz_out, sf_keypoint* d_kpts_out);
/* The same under Vis/FeatureType 0: sf_add_keyframes_u8_batch_device with the feature stages of
   sf_get_features_and_descriptor_surf_batch_device -- the same formats and gray rule, the same network call, n store slots
   and n NN rows under one index, all or nothing.  Slot first_slot + i holds the bytes of sf_get_features_and_descriptor_u8
   on pair i; a keyframe whose maxima exceed the key capacity keeps its slot and its NN row, holds no rows, and is counted
   by sf_surf_batch_status.  Refuses what either of the two refuses; on a handle of another feature type: SF_EINVAL,
   nothing changes.                                                                                                    */
int  sf_add_keyframes_surf_u8_batch_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right, const uint8_t* d_rgb,
                                           int32_t format, int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                           size_t image_stride, const sf_stereo_camera* cam, const sf_detector_params* det,
                                           const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                           int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                           float* d_xyz_out, sf_keypoint* d_kpts_out);
/* The same under Vis/FeatureType 1: sf_add_keyframes_u8_batch_device with the feature stages of
   sf_get_features_and_descriptor_sift_batch_device -- the same formats and gray rule, the same network call (both over
   all n images, before the chunks of the feature stages), n store slots and n NN rows under one index, all or nothing.
   Slot first_slot + i holds the bytes of sf_get_features_and_descriptor_u8 on pair i; a keyframe with more extrema or
   keypoints than an image holds keeps its slot and its NN row, holds no rows, and is counted by sf_sift_batch_status.
   Refuses what either of the two refuses; on a handle of another feature type: SF_EINVAL, nothing changes.            */
int  sf_add_keyframes_sift_u8_batch_device(sf_handle h, const uint8_t* d_left, const uint8_t* d_right, const uint8_t* d_rgb,
                                           int32_t format, int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                           size_t image_stride, const sf_stereo_camera* cam, const sf_detector_params* det,
                                           const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                           int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                           float* d_xyz_out, sf_keypoint* d_kpts_out);

/* ---- raw camera images: undistortion and rectification on the device ---------------------------------------------- */
/* Every call above takes rectified images: the reference's launch files subscribe to image_rect topics.  A raw stereo
   head (EuRoC-style cam0/image_raw with a radial-tangential calibration) leaves that job to stereo_image_proc, or to
   rtabmap under Rtabmap/ImagesAlreadyRectified = false: cv::initUndistortRectifyMap + cv::remap(INTER_LINEAR,
   BORDER_CONSTANT, 0) per image on a CPU core [upstream OpenCV 3.2, restated in tests/rectify_ref.py; as remembered, not
   from the reference tree: DESIGN.md section 3 lists what the restatement decides].  The calls below do it on the device,
   in front of sf_image_to_gray_device and the keyframe calls, whose device images with a pitch and a stride they write.
     map of output pixel (column j, row i), float64, every step one rounded operation in this order:
       iR = (P[:, :3] R)^-1 (host, adjugate over determinant)
       X = ((iR00 j) + (iR01 i)) + iR02, likewise Y, W;  w = 1 / W;  x = X w;  y = Y w;  x2 = x x;  y2 = y y;
       r2 = x2 + y2;  t = 2 x y;  kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2)
       xd = x kr + p1 t + p2 (r2 + 2 x2);  yd = y kr + p1 (r2 + 2 y2) + p2 t
       mapx = (float)(fx xd + cx);  mapy = (float)(fy yd + cy)            (fx, fy, cx, cy of K)
     fixed point: sx = round-half-even(mapx * 32) with the product in float32, ix = sx >> 5, a = sx & 31 (sy, iy, b
       likewise); a map value that is not finite or whose 32-fold reaches 2^30 in magnitude gives the pixel 0
     taps: (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) with the weights 32 (32 - a)(32 - b), 32 a (32 - b),
       32 (32 - a) b, 32 a b (their sum is 32768); a tap outside the source reads 0; the pixel is
       (sum of weight x tap + 16384) >> 15 per channel.                                                              */
typedef struct sf_camera_info {
  int32_t width, height;          /* the raw image, 1 .. 8192 each                                                   */
  int32_t out_width, out_height;  /* the rectified image, 1 .. 8192; 0 = the raw size                                */
  int32_t model;                  /* 0 = plumb_bob (D[0 .. 4]), 1 = rational_polynomial (D[0 .. 7])                   */
  int32_t reserved;               /* 0                                                                               */
  double  K[9];                   /* row-major 3 x 3: fx 0 cx / 0 fy cy / 0 0 1; fx, fy > 0, K[1] (skew) = 0          */
  double  D[8];                   /* k1, k2, p1, p2, k3, k4, k5, k6                                                   */
  double  R[9];                   /* row-major 3 x 3 rectification rotation                                          */
  double  P[12];                  /* row-major 3 x 4 projection of the rectified camera; P[0], P[5] > 0               */
} sf_camera_info;                 /* 328 bytes */
#define SF_MAX_RECTIFY_PLANS 64   /* ids 1 .. 64 */
/* Validates a block, derives the plan's constants (iR, K, D) and stores them on the handle and on the device:
   *plan_out = 1, 2, ..  A value that is not finite, fx or fy <= 0 in K or P, a skew, a singular P[:, :3] R, a size outside
   1 .. 8192, an unknown model, reserved != 0: SF_EINVAL with a message, nothing changes; a full table: SF_ERANGE.    */
int  sf_rectify_plan_create(sf_handle h, const sf_camera_info* info, int32_t* plan_out);
/* A plan from the caller's own float32 maps in HOST memory (row i of the out_width x out_height maps at byte i *
   map_pitch; source pixel coordinates in a src_width x src_height image): for models the library does not compute -- an
   equidistant fisheye, a vendor's table.  The maps are converted to the fixed-point form above as they are uploaded and
   are not kept as floats.  Sizes outside 1 .. 8192, map_pitch below a row: SF_EINVAL; a full table: SF_ERANGE.       */
int  sf_rectify_plan_from_maps(sf_handle h, const float* mapx, const float* mapy, int32_t out_width, int32_t out_height,
                               int32_t map_pitch, int32_t src_width, int32_t src_height, int32_t* plan_out);
int  sf_rectify_plan_count(sf_handle h, int32_t* n_out);
/* The block a plan was created from; *from_maps (may be NULL) = 1 for a plan of caller maps, whose block holds the four
   sizes and zeros.  An id outside 1 .. count: SF_EINVAL.                                                              */
int  sf_rectify_plan_get(sf_handle h, int32_t plan, sf_camera_info* out, int32_t* from_maps);
/* Drops every plan (after the work queued on them has finished); ids start at 1 again.  sf_store_clear keeps the plans. */
int  sf_rectify_plan_clear(sf_handle h);
/* The float32 maps of a computed plan, for inspection: row i of either map at byte i * pitch_bytes (>= 4 * out_width) of
   the device arrays.  Asynchronous on the handle's stream.  A plan of caller maps: SF_EINVAL (its floats are not kept). */
int  sf_rectify_maps_device(sf_handle h, int32_t plan, float* d_mapx, float* d_mapy, int32_t pitch_bytes);
/* Rectifies n_images raw device images under plan_a -- image i at d_src_a + i * src_stride to d_dst_a + i * dst_stride --
   and, when d_src_b is not NULL, as many under plan_b (d_src_b to d_dst_b: the right camera of a stereo head) in ONE launch,
   asynchronous on the handle's stream, with no host wait.  Both plans hold the same raw and the same output size.  format
   is an sf_image_format; out_format is format, or SF_IMAGE_MONO8 from a colour format: the rectified colour pixel goes
   straight through the handle's gray rule and the planes hold, byte for byte, what sf_image_to_gray_device makes of the
   rectified colour images.  Any pitches (>= a row), strides (>= the rows they hold; ignored when n_images = 1) and base
   alignments; bytes outside the out_width x out_height images are never written.  n_images = 0: SF_OK.  A plan id
   outside the table, plans of unlike sizes, another out_format, a pitch below a row, a missing array: SF_EINVAL.
   A computed plan runs the computed form (every thread derives its map values from the plan's 21 constants) or the
   table form (a fixed-point map built once per plan, 8 bytes per output pixel) as SF_OPT_RECTIFY_TABLE says; a plan of
   caller maps, and the plan beside it in the same call, the table form.  The bytes are the same.                    */
int  sf_image_rectify_device(sf_handle h, int32_t plan_a, const uint8_t* d_src_a, int32_t plan_b, const uint8_t* d_src_b,
                             int32_t format, int32_t out_format, int32_t n_images, int32_t src_pitch, size_t src_stride,
                             uint8_t* d_dst_a, uint8_t* d_dst_b, int32_t dst_pitch, size_t dst_stride);
/* Host only: the camera of the rectified pair for the extraction calls -- fx = P[0], fy = P[5], cx = P[2], cy = P[6] of
   the left block, cx_right = P[2] of the right block, baseline = -P_right[3] / P_right[0] (not > 0: SF_EINVAL), the
   given local_transform (NULL = identity), min_depth = max_depth = 0.                                                */
int  sf_stereo_camera_from_info(const sf_camera_info* left, const sf_camera_info* right, const float local_transform[12],
                                sf_stereo_camera* out);

/* ---- RGB-D keyframes: 3D points from a registered depth image, Vis/DepthAsMask ------------------------------------ */
/* replaces: the depth branch of Feature2D::generateKeypoints3D (called at myRegistrationVis.cpp:382) -- util3d::
   generateKeypoints3DDepth -> projectDepthTo3D(smoothing = true) -> util2d::getDepth(depthErrorRatio 0.02,
   estWithNeighborsIfNull false) -- and the detector mask Feature2D::generateKeypoints makes of the depth image
   (myRegistrationVis.cpp:271-284, Vis/DepthAsMask) [upstream rtabmap, restated in tests/depth_ref.py; DESIGN.md section 3
   lists what the restatement decides].  The depth image is registered to the image and has its width and height, or,
   after sf_depth_set_size, a size of its own that is not larger (a decimated depth image, upstream's util2d::interpolate
   path: below); its rows are depth_pitch bytes apart.  The camera is read as an sf_stereo_camera: fx, fy, cx, cy, local_transform, min_depth and max_depth are used,
   baseline and cx_right ignored.
     3D point of keypoint (x, y), float32 in this order: u = (int)(x + 0.5f), v = (int)(y + 0.5f) (u == width && x < width:
     u = width - 1, likewise v; outside the image, or a coordinate that is not finite: no depth).  d = the depth at (u, v) in
     metres; 0 or not finite: no point.  Smoothing over the 3 x 3 neighbours inside the image (columns outer, rows inner,
     centre skipped): a neighbour dn counts iff dn != 0, finite and |dn - d| < 0.02f * d, with weight 2 and value dn * 2
     in the centre's row or column, else weight 1; depth = (d * 4 + sum of values) / (sum of weights + 4).  cx_ = cx > 0 ?
     cx : width / 2 - 0.5f (integer division), cy_ likewise; X = (x - cx_) * depth / fx, Y = (y - cy_) * depth / fy, Z =
     depth; kept iff Z is finite, (min_depth < 0 or Z > min_depth) and (max_depth <= 0 or Z <= max_depth); then
     local_transform as for stereo points.  Otherwise the point is three quiet NaNs.
     mask of a pixel: 255 iff value > min_depth and (max_depth == 0 or value <= max_depth), else 0 (NaN compares false).   */
enum sf_depth_format {
  SF_DEPTH_U16_MM = 0,   /* CV_16UC1, millimetres; 0 and 65535 = no depth (value 0); metres = (float)v * 0.001f; pitch >= 2 * width */
  SF_DEPTH_F32_M = 1     /* CV_32FC1, metres; 0, NaN and +-inf = no depth; pitch >= 4 * width                                        */
};
typedef struct sf_depth_params {
  int32_t depth_as_mask;   /* Vis/DepthAsMask: 1 = the detector of the depth keyframe calls sees the mask of the depth image */
} sf_depth_params;         /* 4 bytes */
void sf_depth_defaults(sf_depth_params* p);     /* {1}: rtabmap's default */
/* Values other than 0 or 1 return SF_EINVAL and change nothing.                                                      */
int  sf_depth_set_params(sf_handle h, const sf_depth_params* params);
int  sf_depth_get_params(sf_handle h, sf_depth_params* params);
/* A decimated depth image (myRegistrationVis.cpp:271-284: a depth image whose size divides the image's is enlarged with
   util2d::interpolate(depth, factor, 0.1f) for the detector mask; generateKeypoints3D at :382 reads the small image with
   scaled intrinsics).  The size is handle state like sf_depth_params: once set, width and height of EVERY depth call stay
   the image's, the depth image is read as depth_width x depth_height, and depth_pitch and depth_stride are checked
   against that size.  The host call uploads depth_height rows of depth_width elements.  A size equal to the image's gives
   the bytes of {0, 0}.  At a call, a depth image larger than the image in either dimension returns SF_EINVAL ("not
   built") and changes nothing.
     the factor: f = height / depth_height iff height % depth_height == 0, width % depth_width == 0 and height /
     depth_height == width / depth_width (:274-276); else 0.  f = 1: nothing is interpolated.  f = 0: the depth keyframe
     calls build NO mask -- the detector runs unmasked whatever depth_as_mask says, as in the reference, where depthMask
     stays empty -- and the 3D points are still taken from the small image; sf_depth_mask_device returns SF_EINVAL.
     (A handle of type 0, 1 or 2 with depth_as_mask = 1 is refused as before, at every size.)
     interpolation, as remembered from upstream rtabmap, not from the reference tree (restated in tests/depth_interp_ref.py;
     DESIGN.md section 3): D the dw x dh input, f >= 2, the output dw f x dh f, zero at the start; float32 in the order
     written, unfused.  A sample is present iff 0 < v < 65535 (uint16; its value (float)v, raw millimetres) or finite and
     > 0 (float32).  Cell (a, b), 1 <= a < dw, 1 <= b < dh, has the corners TL = D[b-1][a-1], TR = D[b-1][a], BL =
     D[b][a-1], BR = D[b][a]; it is valid iff all four are present and, with e = 0.1f * (((TL + TR) + BL) + BR) / 4.0f,
     each of |TL-TR|, |TL-BL|, |TL-BR|, |TR-BL|, |TR-BR|, |BL-BR| is <= e.  A valid cell writes the pixels x = (a-1) f + p,
     y = (b-1) f + q, p and q in 0 .. f: st = (TR - TL) / (float)f, sb = (BR - BL) / (float)f, top = TL + st * (float)p,
     bot = BL + sb * (float)p, value = top + ((bot - top) / (float)f) * (float)q; a uint16 output holds
     (uint16_t)(int)value.  Cells are visited with b outer and a inner and a later cell overwrites an earlier one: a pixel
     holds the value of the last valid cell among the at most four that cover it.  Pixels with x > (dw-1) f or y >
     (dh-1) f, and pixels no valid cell covers, stay 0.  The mask is the mask above of that image (uint16: value * 0.001f).
     3D point from a small image: rx = 1.0f / ((float)width / (float)depth_width), ry likewise; the keypoint is read at
     xs = x * rx, ys = y * ry; pixel and smoothing as above on the depth_width x depth_height image; cx_ = cx * rx, and
     if that is not > 0, depth_width / 2 - 0.5f; fx_ = fx * rx; X = (xs - cx_) * depth / fx_, Y alike; limits and
     local_transform as above.  At the image's size rx = ry = 1.0f.                                                      */
typedef struct sf_depth_size {
  int32_t depth_width, depth_height;   /* {0, 0} on a fresh handle: the depth image has the image's size */
} sf_depth_size;                       /* 8 bytes */
/* NULL or {0, 0}: the depth image has the image's size; else both >= 1.  One zero or a negative value returns SF_EINVAL
   and changes nothing.                                                                                                */
int  sf_depth_set_size(sf_handle h, const sf_depth_size* size);
int  sf_depth_get_size(sf_handle h, sf_depth_size* out);
/* No handle, no GPU: the factor above; 0 = none.                                                                      */
int  sf_depth_interpolation_factor(int32_t width, int32_t height, int32_t depth_width, int32_t depth_height);
/* util2d::interpolate for n_images depth images of depth_width x depth_height in one launch, asynchronous on the handle's
   stream: image i at d_depth + i * depth_stride bytes to d_out + i * out_stride, enlarged to depth_width factor x
   depth_height factor elements of the input's own format, rows out_pitch bytes apart; bytes outside the planes are not
   written.  Pitches, strides and both addresses are multiples of the element size, nothing more; strides are ignored
   when n_images = 1.  The handle's sf_depth_size is not read.  factor = 1 is a pitched copy.  SF_EINVAL: factor < 1, an
   unknown format, a pitch below a row, a pitch, stride or address that is no multiple of the element size, a stride
   below the rows it holds.  n_images = 0 is SF_OK.                                                                    */
int  sf_depth_interpolate_device(sf_handle h, const void* d_depth, int32_t depth_format, int32_t depth_width,
                                 int32_t depth_height, int32_t depth_pitch, size_t depth_stride, int32_t n_images,
                                 int32_t factor, void* d_out, int32_t out_pitch, size_t out_stride);
/* The masks of n_images depth images of one size, one launch, asynchronous on the handle's stream: image i at d_depth + i *
   depth_stride bytes to the uint8 plane at d_mask + i * mask_stride (rows of mask_pitch >= width bytes; bytes outside the
   width x height planes are not written).  Strides are ignored when n_images = 1.  SF_EINVAL: unknown format, depth_pitch
   below a row (2 * width or 4 * width), a depth pitch or stride that is no multiple of the element size, a stride below
   the rows it holds.  n_images = 0 is SF_OK.  After sf_depth_set_size the depth images have that size, the masks stay
   width x height: the masks of the interpolated images, which are never in memory (factor 0: SF_EINVAL).              */
int  sf_depth_mask_device(sf_handle h, const void* d_depth, int32_t depth_format, int32_t width, int32_t height,
                          int32_t depth_pitch, size_t depth_stride, int32_t n_images, float min_depth, float max_depth,
                          uint8_t* d_mask, int32_t mask_pitch, size_t mask_stride);
/* The 3D points of n keypoints (x and y are read) of one depth image, asynchronous: d_xyz_out [n][3], d_valid_out [n]
   (optional; 1 = the point is finite).  cam->min_depth / max_depth filter as above.  n = 0 is SF_OK.                   */
int  sf_depth_points_device(sf_handle h, const void* d_depth, int32_t depth_format, int32_t width, int32_t height,
                            int32_t depth_pitch, const sf_keypoint* d_kpts, int32_t n, const sf_stereo_camera* cam,
                            float* d_xyz_out, uint8_t* d_valid_out);
/* sf_detect_corners_device as cv::goodFeaturesToTrack(image, ..., mask): d_mask is a uint8 plane of the image's size, rows
   of mask_pitch >= width bytes.  The maximum that scales quality_level is taken over the pixels with mask != 0 (max(0, ..)
   as without a mask), a corner must lie on such a pixel, and the 3 x 3 dilation still sees every pixel: a masked-out larger
   neighbour suppresses a masked-in pixel.  A mask of zeros gives 0 corners and SF_OK.  Everything else -- parameters,
   order, refusals -- is sf_detect_corners_device's; a mask without a zero gives that call's bytes.                       */
int  sf_detect_corners_masked_device(sf_handle h, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                     const uint8_t* d_mask, int32_t mask_pitch, int32_t max_corners, double quality_level,
                                     double min_distance, sf_keypoint* d_kpts_out, int32_t cap, int32_t* n_out);
/* sf_detect_fast_device as FastFeatureDetector::detect(image, keypoints, mask): score and 3 x 3 suppression run on every
   pixel, corners with mask[y][x] == 0 are then dropped, before rtabmap's limitKeypoints.                              */
int  sf_detect_fast_masked_device(sf_handle h, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                  const uint8_t* d_mask, int32_t mask_pitch, int32_t max_features,
                                  const sf_fast_params* params, sf_keypoint* d_kpts_out, int32_t cap, int32_t* n_out);
/* sf_extract_keyframe_device with the registered depth image of the keyframe in place of d_right_x / d_status: the same
   descriptors under every feature type (0, 1, 2, 3, 4, 5, 6, 8), the 3D point of every corner from the depth image.  A
   corner is kept iff its descriptor patch lies inside the image and, when cam->min_depth > 0 or cam->max_depth > 0, its
   point is finite; with both limits 0 the rows and keypoints are those of sf_extract_keyframe_device on the same image.  */
int  sf_extract_keyframe_depth_device(sf_handle h, const uint8_t* d_left, int32_t width, int32_t height, int32_t pitch,
                                      const sf_keypoint* d_kpts, const void* d_depth, int32_t depth_format,
                                      int32_t depth_pitch, int32_t n, const sf_stereo_camera* cam, int32_t* out_slot,
                                      int32_t* out_rows, uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out);
/* sf_get_features_and_descriptor_u8 for a SensorData(rgb, depth, model) caller: image (in image_format, an
   sf_image_format, converted on the device as that call does) and depth in HOST memory.  Stages: the mask of the depth
   image (when the handle's depth_as_mask is 1; limits cam->min_depth / max_depth), the detector of the handle's feature
   type under that mask, sub-pixel refinement, extraction with depth points.  There is no stereo stage.  Under a ROI or a
   grid the mask is cropped like the image; per-cell maxima and quotas apply as without a mask.  The mask is built for the
   two corner detectors (types 3, 4, 5, 6, 8): on a handle of type 0, 1 or 2 with depth_as_mask = 1 the call returns
   SF_EINVAL ("DepthAsMask ... not built"; sf_depth_set_params with 0 is the way out), with depth_as_mask = 0 those types
   work.  Outputs and limits as sf_get_features_and_descriptor.  A refused call changes nothing.  Synchronous.          */
int  sf_get_features_and_descriptor_depth(sf_handle h, const uint8_t* image, int32_t image_format, const void* depth,
                                          int32_t depth_format, int32_t width, int32_t height, int32_t image_pitch,
                                          int32_t depth_pitch, const sf_stereo_camera* cam, const sf_detector_params* det,
                                          uint8_t* desc_out, float* xyz_out, sf_keypoint* kpts_out, int32_t cap_rows,
                                          int32_t* rows_out, int32_t* slot_out);
/* n_keyframes depth keyframes from DEVICE memory in one launch sequence with no host wait: MONO8 planes (image i at
   d_images + i * image_stride) and depth planes (at d_depth + i * depth_stride bytes), each with its own pitch and stride.
   One call serves every feature type (it dispatches on the handle's family; SIFT runs chunk by chunk); per keyframe the
   bytes are sf_get_features_and_descriptor_depth's.  Outputs as sf_get_features_and_descriptor_batch_device.            */
int  sf_get_features_and_descriptor_depth_batch_device(sf_handle h, const uint8_t* d_images, const void* d_depth,
                                                       int32_t depth_format, int32_t n_keyframes, int32_t width,
                                                       int32_t height, int32_t image_pitch, size_t image_stride,
                                                       int32_t depth_pitch, size_t depth_stride,
                                                       const sf_stereo_camera* cam, const sf_detector_params* det,
                                                       int32_t* first_slot_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                       float* d_xyz_out, sf_keypoint* d_kpts_out);
/* The same from the camera's colour images (image_format, an sf_image_format), which also feed the network
   (sf_netvlad_infer_u8_batch_device): n store slots and n NN rows under one index, all or nothing, as
   sf_add_keyframes_u8_batch_device.                                                                                   */
int  sf_add_keyframes_depth_batch_device(sf_handle h, const uint8_t* d_images, int32_t image_format, const void* d_depth,
                                         int32_t depth_format, int32_t n_keyframes, int32_t width, int32_t height,
                                         int32_t image_pitch, size_t image_stride, int32_t depth_pitch, size_t depth_stride,
                                         const sf_stereo_camera* cam, const sf_detector_params* det, int32_t* first_slot_out,
                                         int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                         float* d_xyz_out, sf_keypoint* d_kpts_out);
/* Depth registration: a depth image measured in the depth (IR) camera's frame -- other intrinsics, another size, a few
   centimetres beside the colour camera -- made the registered image the calls above take.  replaces: util2d::registerDepth
   and util2d::fillRegisteredDepthHoles(fillDoubleHoles = false) of rtabmap's camera drivers, one CPU pass per pixel
   [upstream rtabmap, as remembered, not from the reference tree; restated in tests/depth_register_ref.py; DESIGN.md
   section 3 lists what the restatement decides].  A forward scatter with a z-test: a minimum does not depend on the order
   of arrival, so the result is compared byte for byte.  All arithmetic is float32, unfused, in the order written.
     in: a depth_width x depth_height image D in a format above; the depth camera's fx, fy, cx, cy; the colour camera's rfx,
     rfy, rcx, rcy and its size W x H = width x height; T = transform, row-major 3 x 4, which takes a point in the depth
     camera's frame into the colour camera's.  out: a W x H image of the input's format, 0 where nothing lands.
     presence: uint16 0 < v < 65535, dz = (float)v * 0.001f; float32 finite and > 0, dz = v.
     depth pixel at column x, row y: X = (((float)x - cx) * dz) / fx, Y = (((float)y - cy) * dz) / fy;
       px = ((T[0] * X + T[1] * Y) + T[2] * dz) + T[3], py and pz alike with T[4 .. 7] and T[8 .. 11];
       dropped unless pz > 0; iz = 1.0f / pz; u = (rfx * px) * iz + rcx; v = (rfy * py) * iz + rcy;
       dropped unless -1 < u < W and -1 < v < H (NaN compares false); column = (int)u, row = (int)v: truncation toward zero
       as upstream, values between -1 and 0 land in column or row 0.
     key: uint16: m = pz * 1000.0f, dropped unless m < 65535.0f, k = (int)m, dropped if k == 0; float32: k = the bits of pz
       (positive, so their unsigned order is the float order).
     result: the pixel holds the smallest k of all points that land on it, or 0.
     hole filling, optional, one flag for the vertical and one for the horizontal pair; OUT OF PLACE on the registered
     image A: pixels with 1 <= x <= W - 2 and 1 <= y <= H - 2 are candidates, all others are copied.  With b = A[y][x]:
     first the vertical pair a = A[y - 1][x], c = A[y + 1][x] if its flag is set, then the horizontal pair a = A[y][x - 1],
     c = A[y][x + 1] if its flag is set and the vertical pair did not set the pixel.  A pair sets the pixel to m iff a != 0,
     c != 0, close, and b == 0 or far --
       uint16: m = (a + c) / 2 in integers, e = 0.01f * (float)m, close: (float)|a - c| <= e, far: (float)b > (float)a + e and
       (float)b > (float)c + e; float32: m = (a + c) / 2.0f, e = 0.01f * m, close: |a - c| <= e, far: b > a + e and b > c + e.
     far removes background that shows through the gaps of a sparser foreground.
   Truncation of u and v is upstream's: an identity registration moves about one pixel in ten to its left or upper
   neighbour, because u falls a rounding error short of x.                                        */
typedef struct sf_depth_registration {
  int32_t depth_width, depth_height;       /* the depth images, 1 .. 8192 each                                       */
  int32_t width, height;                   /* the colour camera's images W x H, 1 .. 8192 each                       */
  float   fx, fy, cx, cy;                  /* the depth camera; fx, fy > 0                                           */
  float   rfx, rfy, rcx, rcy;              /* the colour camera; rfx, rfy > 0                                        */
  float   transform[12];                   /* T, row-major 3 x 4: depth camera frame to colour camera frame          */
  int32_t fill_vertical, fill_horizontal;  /* 0 or 1 each: the pairs of the hole filling                             */
  int32_t reserved;                        /* must be 0                                                              */
} sf_depth_registration;                   /* 108 bytes */
/* Zero sizes and intrinsics (to be filled in), the identity transform, both fills 0.                                 */
void sf_depth_registration_defaults(sf_depth_registration* reg);
/* What sf_depth_register_device holds a block to, host only, without a handle or a GPU: SF_OK, or SF_EINVAL (text via
   sf_last_error with a NULL handle) for a size outside 1 .. 8192, a value that is not finite, an fx, fy, rfx or rfy <= 0,
   a flag other than 0 or 1, reserved != 0.                                                                          */
int  sf_depth_register_check(const sf_depth_registration* reg);
/* n_images depth images registered in one launch sequence, asynchronous on the handle's stream with no host wait: image i
   at d_depth + i * depth_stride bytes (rows depth_pitch bytes apart) to the width x height image of the same format at
   d_out + i * out_stride (rows out_pitch bytes apart); bytes outside the planes are never written.  Pitches, strides and both
   addresses are multiples of the element size, nothing more; strides are ignored when n_images = 1.  The handle's
   sf_depth_size is not read.  The z-buffer, 4 width height bytes per image, is the handle's; a batch whose z-buffers pass
   256 MB runs in chunks of images, queued back to back.  The one host wait there can be: a call that needs a larger
   z-buffer than any before it (the first, or a larger shape or batch) waits for the stream before the buffer is replaced.  n_images = 0 is SF_OK.  SF_EINVAL, changing nothing: a block the
   check refuses, an unknown format, a pitch below a row, a pitch, stride or address that is no multiple of the element size,
   a stride below the rows it holds, a missing array, an output that overlaps the input.                              */
int  sf_depth_register_device(sf_handle h, const sf_depth_registration* reg, const void* d_depth, int32_t depth_format,
                              int32_t depth_pitch, size_t depth_stride, int32_t n_images, void* d_out, int32_t out_pitch,
                              size_t out_stride);
/* The hole filling alone on n_images images of width x height (1 .. 8192 each) registered elsewhere: the device function of
   the call above, so the bytes are the same.  Out of place: an output that overlaps the input is refused; everything else
   as above, without a workspace: no host wait, any number of images (65535 per launch).                                                                                                         */
int  sf_depth_fill_holes_device(sf_handle h, const void* d_depth, int32_t depth_format, int32_t width, int32_t height,
                                int32_t depth_pitch, size_t depth_stride, int32_t n_images, int32_t fill_vertical,
                                int32_t fill_horizontal, void* d_out, int32_t out_pitch, size_t out_stride);

/* ---- geometric verification (stereoCamGeometricTools.cpp:122-178) ---------------------------- */
/* One estimate_transformation service call on host buffers.                                  */
int  sf_estimate_transform(sf_handle h, const sf_features* from, const sf_features* to,
                           sf_result* out);
/* n service calls in one launch sequence, host buffers (features are staged into scratch
   store slots).                                                                              */
int  sf_estimate_transform_batch(sf_handle h, const sf_features* from, const sf_features* to,
                                 int32_t n, sf_result* out);
/* n candidate pairs given as store slots (from_slot[i] -> to_slot[i]); results to host.      */
int  sf_verify_pairs(sf_handle h, const int32_t* from_slot, const int32_t* to_slot, int32_t n,
                     sf_result* out);
/* Fully device-resident variant: slot arrays and results live in device memory (e.g. a torch
   tensor's data_ptr()); asynchronous on the handle's stream.                                 */
int  sf_verify_pairs_device(sf_handle h, const int32_t* d_from_slot, const int32_t* d_to_slot,
                            int32_t n, sf_result* d_out);
/* Verify the candidates an NN query returned: candidate i is the pair (store slot slot_base_other +
   matches[i].idx_other  ->  slot slot_base_local + matches[i].idx_local), i.e. the (frame of the
   querying robot, frame of the computing robot) pair find_separators.py:85-91 sends to
   estimate_transformation.  `matches` is HOST memory (the output of sf_nn_find_matches), d_out device
   memory for n records.  Asynchronous on the handle's stream; `matches` may be reused on return.   */
int  sf_verify_matches_device(sf_handle h, const sf_match* matches, int32_t n, int32_t slot_base_other,
                              int32_t slot_base_local, sf_result* d_out);
/* Compact the ACCEPTED results (success != 0) of a verification, in candidate order, into d_accepted
   (device, room for n records) and write every candidate's success flag to d_flags (device, n bytes,
   may be NULL): what find_separators.py:97-131 forwards as separators, resp. feeds back as failures.
   Returns the number of accepted records in *n_accepted (host); synchronises the stream.           */
int  sf_compact_accepted_device(sf_handle h, const sf_result* d_results, int32_t n, sf_result* d_accepted,
                                uint8_t* d_flags, int32_t* n_accepted);
/* The same compaction without the synchronisation: the count is left in device memory at d_n_accepted
   (int32), everything asynchronous on the handle's stream -- for callers that ship count, flags and a
   speculative prefix of the accepted records to the host (or stamp the count into an exchange buffer) behind
   ONE synchronisation of their own.                                                                    */
int  sf_compact_accepted_device_async(sf_handle h, const sf_result* d_results, int32_t n, sf_result* d_accepted,
                                      uint8_t* d_flags, int32_t* d_n_accepted);
/* Correspondences found by the two matching passes of the LAST verify call for pair `i`
   (tests / diagnostics): pairs (from_feature, to_feature), ascending from_feature.  Calls with more
   than 131072 pairs are processed in chunks; `pair` then indexes the LAST chunk.  Needs SF_OPT_DEBUG_CORR
   set BEFORE that verify call (SF_EINVAL otherwise) when the fused kernel ran it.                  */
int  sf_debug_correspondences(sf_handle h, int32_t pair, int32_t pass, uint16_t* from_idx,
                              uint16_t* to_idx, int32_t cap, int32_t* n_out);

/* ---- separator records ------------------------------------------------------------------------ */
/* Pack accepted/failed results into ReceiveSeparators rows (host side, no GPU work).          */
int  sf_pack_separators(const sf_result* res, int32_t n, int8_t robot_from, int8_t robot_to,
                        const int16_t* kf_from, const int16_t* kf_to, const int16_t* frame_from,
                        const int16_t* frame_to, sf_separator* out);

/* ---- multi-GPU exchange (RCCL over xGMI) ------------------------------------------------------- */
/* The path shards with no collective in the compute (pairs are independent); the one exchange is an
   all-gather of accepted separator records, what the reference moves between robots as
   ReceiveSeparators requests (communication.cpp:15-52).  One handle (one GPU) per rank.          */
#define SF_COMM_ID_BYTES 128
int  sf_comm_unique_id(uint8_t* out, int32_t cap);          /* rank 0 creates, the host distributes */
int  sf_comm_init(sf_handle h, const uint8_t* unique_id, int32_t rank, int32_t world);
int  sf_comm_destroy(sf_handle h);
/* d_local: n_local records in device memory.  d_all: world * cap_per_rank records in device memory,
   rank r's records at d_all + r * cap_per_rank; counts (host): world entries.  Synchronous; one collective (the
   count travels in a header slot of the block).                                                       */
int  sf_allgather_separators(sf_handle h, const sf_separator* d_local, int32_t n_local,
                             sf_separator* d_all, int32_t cap_per_rank, int32_t* counts);
/* The same exchange with no host in it: d_send = cap_per_rank + 1 record slots, slot 0 a header whose first int32
   is this rank's count STAMPED ON THE DEVICE (e.g. by sf_compact_accepted_device_async writing its count there),
   slots 1.. the records; d_all = world such blocks (block r = rank r).  ONE collective, asynchronous on the handle's
   stream; the caller reads the counts out of the gathered headers behind its own synchronisation.            */
/* The same collective on an opaque block of bytes_per_rank bytes (device memory, asynchronous on the handle's
   stream): the row minima of the row-sharded NN stage travel this way.  d_all: world * bytes_per_rank bytes.   */
int  sf_allgather_bytes_device(sf_handle h, const void* d_send, void* d_all, size_t bytes_per_rank);
int  sf_allgather_separators_device(sf_handle h, const sf_separator* d_send, sf_separator* d_all,
                                    int32_t cap_per_rank);

/* sf_nn_find_matches followed by sf_verify_matches_device of what it returned, as ONE call (the loop body of
   find_separators.py:59-133 when both robots' keyframes live in this handle): `out` / `*n_out` as
   sf_nn_find_matches, d_out[i] (device, caller-allocated, >= cap records) = result of match i, asynchronous
   on the handle's stream.  Same outputs as the two calls; when the walk may return every local row
   (cap and netvlad_max_matches_nb >= local rows, nn_precision = 1) the candidates of the NN filter are
   verified SPECULATIVELY on the device while the host still reduces / sorts / walks them, which takes the
   host part of the NN stage off the critical path.                                                     */
int  sf_find_matches_and_verify_device(sf_handle h, int32_t slot_base_other, int32_t slot_base_local,
                                       sf_match* out, int32_t cap, int32_t* n_out, sf_result* d_out);
/* d_out may be NULL: the results then stay in the handle's own block (sf_step_* and sf_experimental.h consume them
   there without a gathered copy of all records).                                                                  */

/* ---- the caller's loop body as a begin / retire pair ------------------------------------------------------------ */
/* replaces: one iteration of find_separators.py:59-133 when both robots' keyframes live in this handle --
     sf_step_issue   = s_find_matches_query (:63) + one s_ans_est_transform per returned candidate (:83-95), QUEUED: the
                       NN kernels, the argsort + walk of DataHandler.find_matches (data_handler.py:187-205) ON THE DEVICE
                       and the verification of the walk's matches are all queued on one stream and the call returns
                       without waiting for any of it (SF_OPT_STEP_DEVICE_WALK);
     sf_step_retire  = what the loop then does with the outcomes (:97-133): for every match, in the order
                       DataHandler.find_matches returned them, whether the estimation succeeded and, if so, its
                       PoseWithCovariance -- the rows of the ReceiveSeparators request (sf_pack_separators packs them).
                       It is the only call of the pair that waits for the device.
   Up to SF_OPT_STEP_DEPTH steps (default 6) may be in flight, so the device never waits for the host (bench.py,
   examples/bench_cli.cpp):  issue(0) .. issue(D-1); then retire(k), issue(k + D) ...; retire the rest.
   The steps in flight are dealt over SF_OPT_STEP_LANES streams (SF_OPT_STEP_OVERLAP): work the caller queued on the
   handle's stream before sf_step_issue is waited for, and every call that changes a database or a mask
   (sf_store_*, sf_nn_append_*, sf_nn_mark_*, sf_nn_ignore_pair, sf_nn_reset) first waits for the steps in flight:
   a step sees the databases and masks as they were when it was issued.
   Accepted results leave the verification kernel for host-pinned memory the moment they are final (no compaction
   launch, no copy); launch shapes the stream does not cover (stage kernels, more than 131 072 matches) end with an
   ordered compaction inside the same two calls.  With nn_precision 1 the NN filter runs at the prefix level the
   handle last settled on; a candidate set too dense for that level is detected on the device, and sf_step_retire then
   runs that one query again through the prefix ladder (sf_nn_find_matches' path) before it returns -- results are
   identical either way; only with a mirror set (below) such a step returns SF_ERANGE, since the mirror missed it.
   Pointers in sf_step_result are owned by the handle and stay valid until the next sf_step_retire.               */
typedef struct sf_step_result {
  const sf_match*  matches;          /* n_matches candidates, walk order (data_handler.py:191-205)                   */
  const int32_t*   record_of_match;  /* n_matches: index into `records` of the match's result, -1 = estimation failed
                                        (transform_est_success = 0: find_separators.py:119-126 feeds the ignore list) */
  const sf_result* records;          /* accepted results (success = 1) in host-pinned memory; completion order when
                                        streamed, match order otherwise: always go through record_of_match           */
  int32_t          n_matches;
  int32_t          n_records;        /* accepted results present (>= n_accepted: a local row with two candidates under
                                        the threshold had both verified, the walk kept one)                          */
  int32_t          n_accepted;       /* matches whose estimation succeeded                                           */
  int32_t          streamed;         /* 1: the records streamed out of the kernel, 0: compacted behind it            */
  const sf_result* d_records;        /* the same n_records records, same order, in DEVICE memory (NULL while a mirror is
                                        set): what a multi-GPU host hands to its all-gather after the retire -- by a
                                        device-to-device copy into its send buffer (sf_memcpy_device_async) or directly;
                                        valid until the next sf_step_retire like the other pointers                     */
} sf_step_result;
int  sf_step_issue(sf_handle h, int32_t slot_base_other, int32_t slot_base_local);
int  sf_step_retire(sf_handle h, sf_step_result* out);      /* the OLDEST step in flight; waits for its verification */
/* bytes from device memory to device memory, asynchronous on `hip_stream` (NULL: the handle's stream) -- e.g. a retired
   step's sf_step_result.d_records -> the send buffer of the caller's collective, on the stream the caller runs its
   collectives from (a stream of its own keeps that traffic out of the way of the steps in flight).  A copy out of a
   step's d_records is remembered: the step that next uses that block waits for it before it writes the buffer again,
   whatever stream the copy was queued on. */
int  sf_memcpy_device_async(sf_handle h, void* d_dst, const void* d_src, size_t bytes, void* hip_stream);
/* Optional second destination of every accepted record, on the device -- e.g. the send buffer of the all-gather that
   follows (sf_allgather_separators_device: slot 0 = header, records from slot 1): d_records2[slot] receives the record
   the host block receives at the same slot and *d_counter (a device word the CALLER zeroes before each sf_step_issue,
   e.g. the count in that header) counts the slots taken.  cap = record slots behind d_records2; a cap below the number
   of verified candidates of a query (local rows * 9 / 8 + 256) switches that query to the compaction (nothing is ever
   dropped).  NULL, NULL, 0 removes the mirror.  Not while a step is in flight.
   While a mirror is set sf_step_issue admits as many steps in flight as the mirror has buffers (1 here, 2 with
   sf_step_mirror_pair) and fails with SF_EINVAL beyond -- step k + 2 would zero and overwrite what step k wrote:
   the loop is issue, [issue,] retire + hand the buffer to the collective, issue, ... (ABI 6).                       */
int  sf_step_mirror(sf_handle h, sf_result* d_records2, uint32_t* d_counter, int32_t cap);
/* The same with TWO destinations that alternate with the steps (the first sf_step_issue after this call writes the
   even pair, the next one the odd pair, ...): with two send buffers the all-gather of step k runs beside the
   verification of step k + 1 instead of in front of it -- the caller orders only the REUSE of a buffer (step k + 2)
   behind the collective that read it.  Both pairs NULL removes the mirror.  Not while a step is in flight.        */
int  sf_step_mirror_pair(sf_handle h, sf_result* d_records_even, uint32_t* d_counter_even,
                         sf_result* d_records_odd, uint32_t* d_counter_odd, int32_t cap);
/* After sf_step_mirror_pair: lets the odd steps run on the handle's second stream as they do without a mirror
   (SF_OPT_STEP_OVERLAP) and returns the two hipStream_t.  From here on the caller orders everything it does with the
   even pair -- zeroing the counter, the collective that reads the buffer -- on *stream_even and everything with the
   odd pair on *stream_odd.  With SF_OPT_STEP_OVERLAP off both are the handle's stream.  Ends with the next
   sf_step_mirror / sf_step_mirror_pair call.  Not while a step is in flight.                                     */
int  sf_step_mirror_streams(sf_handle h, void** stream_even, void** stream_odd);

/* ---- measurement ------------------------------------------------------------------------------ */
/* Kernel ids for sf_prof_get */
enum {
  SF_K_MATCH = 0,      /* global Hamming kNN-2 + NNDR + uniqueness (pass 1)                   */
  SF_K_RANSAC1 = 1,    /* RANSAC 3D-3D + refine, pass 1                                       */
  SF_K_GUIDED = 2,     /* guess-guided window matching (pass 2)                               */
  SF_K_RANSAC2 = 3,    /* RANSAC 3D-3D + refine, pass 2                                       */
  SF_K_NN = 4,         /* NetVLAD distance matrix + fused row arg-min                         */
  SF_K_NN_SELECT = 5,  /* f64 re-evaluation of the row minima                                 */
  SF_K_NN_FILTER = 6,  /* fp16 MFMA candidate filter (nn_precision = 1)                       */
  SF_K_NN_REFINE = 7,  /* exact f64 distance of every filter survivor                         */
  SF_K_FUSED = 8,      /* fused per-pair pipeline: match + RANSAC + guided + RANSAC + result    */
  SF_K_NN_WALK = 9,    /* argsort of the row minima + the walk (data_handler.py:191-205), on the device */
  SF_K_BA = 10,        /* two-view bundle adjustment of a pass's estimate (a launch of its own since ABI 6) */
  SF_K_GUIDED_TP = 11, /* guided matching of the "to" keypoints to the projections (guess_match_to_projection = 1) */
  SF_K_COUNT = 12
};
/* When enabled every kernel launch is bracketed by hipEvents on the handle's stream.          */
int  sf_prof_enable(sf_handle h, int on);
int  sf_prof_reset(sf_handle h);
int  sf_prof_get(sf_handle h, int kernel, int64_t* launches, double* total_ms);
const char* sf_kernel_name(int kernel);

/* Execution options of a live handle (none changes any output byte; the same switches are read from the
   environment at sf_create: SF_MATCH_MFMA, SF_FUSED, SF_OVERLAP).  Returns SF_EINVAL for an unknown option. */
enum {
  SF_OPT_MATCH_MFMA = 0,  /* 1 (default): Hamming table on the fp4 matrix cores; 0: xor + popcount on the VALU   */
  SF_OPT_FUSED = 1,       /* 1 (default): one fused launch per chunk (3D-3D estimator); 0: the stage kernels     */
  SF_OPT_OVERLAP = 2,     /* 1: batches >= 4096 pairs as two halves on two streams; 0 (default): one stream     */
  SF_OPT_CHAIN_WAVES = 3, /* round 1's narrower motion-estimation chains (measured slower, removed): accepted, no effect */
  SF_OPT_NN_FULL_FILTER = 5, /* 1: the fp16 NN filter (nn_precision = 1) always contracts the FULL descriptor length
                             instead of climbing its adaptive prefix ladder (128 / 512 / full): the cost of a data set
                             whose prefixes are uninformative; matches are identical either way                        */
  SF_OPT_STEP_OVERLAP = 6, /* 1 (default): the two steps sf_step_issue keeps in flight run on two streams (the odd ones on a
                              stream and workspace of the handle's own), so that the emptying tail of one step's
                              verification overlaps the NN stage and the first workgroups of the next: +9-12 % steps per
                              second (3D-3D), +14 % (PnP), results unchanged.  0: every step on the handle's stream.
                              Ignored while sf_step_mirror is set (the caller's collective is ordered on the handle's
                              stream) unless sf_step_mirror_streams handed the two streams to the caller.  Either way a step's results are complete when sf_step_retire returns.            */
  SF_OPT_STEP_SPLIT = 7,  /* 1: while the steps are dealt over several streams (SF_OPT_STEP_OVERLAP) the 3D-3D verification
                             of a step runs as one matching launch over all candidates + one chain launch over the
                             survivors instead of the fused kernel (256-bit descriptors, K <= 512 features, 2 048 .. 65 536
                             candidates -- other shapes keep the fused kernel).  Default 1 again since round 5: the matching
                             launch's scan is software-pipelined inside a wavefront and the form is the faster one by
                             1-1.5 % (23.0 against 22.7 M pairs/s, profiles/r05u_*; round 4, before that: the fused
                             kernel 22.0 against 20.3).  0: always the fused kernel.  Results unchanged.              */
  SF_OPT_STEP_DEPTH = 8,  /* steps sf_step_issue keeps in flight, 1 .. 16 (default 6).  Not while a step is in flight.  */
  SF_OPT_STEP_LANES = 9,  /* streams the steps in flight are dealt over, 1 .. 4 (default 3; step k runs on stream
                             k mod lanes; with a mirror set at most 2).  Not while a step is in flight.              */
  SF_OPT_STEP_DEVICE_WALK = 10, /* 1 (default): sf_step_issue never waits for the device -- the argsort + walk of
                             data_handler.py:191-205 run on the device between the NN kernels and the verification;
                             0: round 3's form (the call returns once the host has walked the row minima).  Results
                             unchanged.  Not while a step is in flight.                                              */
  SF_OPT_STEP_SPECULATE = 11, /* 1 (default): a device-resident step whose walk may return every local row
                             (netvlad_max_matches_nb >= local rows, nn_precision 1) queues the verification of EVERY NN
                             filter candidate straight behind the filter and runs the exact re-evaluation, the row
                             minima and the walk on a second stream beside it; 0: always NN -> walk -> verification of
                             the walk's matches on one stream.  Results unchanged.  Not while a step is in flight.   */
  SF_OPT_CHAIN_NARROW_EST = 12, /* 1 (default): where the 3D-3D verification takes the split form without the bundle
                             adjustment and with ransac_adaptive_stop on, a survivor's two motion estimates run one wavefront wide in a 16 KB LDS slot of their own
                             (lists of up to 256 correspondences; longer ones stay in the wide kernel), as launches before
                             and behind the guided matching: three chain launches instead of one.  0: one launch, four
                             wavefronts per survivor.  Results unchanged.  Environment twin: SF_CHAIN_NARROW_EST.
                             Measured faster on the bench step (docs/chain_narrow_estimates.md).                     */
  SF_OPT_RECTIFY_TABLE = 13, /* the form sf_image_rectify_device runs a computed plan in: 1 (default): a fixed-point map
                             built on the stream by the plan's first such call, 8 bytes per output pixel; 0: every thread
                             derives its map values from the plan's constants in float64, no map in memory.  Results
                             unchanged.  Environment twin: SF_RECTIFY_TABLE.  The default is the measured choice: 2.4
                             against 3.1 us per 752 x 480 stereo pair in a batch of 64 (profiles/rectify_latency.json). */
  SF_OPT_DEBUG_CORR = 4  /* 1: the fused kernel also copies every pair's correspondence lists, headers and pass states
                             to the global workspace, which sf_debug_correspondences reads (default 0: they never
                             leave the workgroup's LDS; the stage kernels always keep them in the workspace)       */
};
int  sf_set_option(sf_handle h, int32_t option, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* SEPFINDER_H */
