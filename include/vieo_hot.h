/* vieo_hot.h -- C-ABI of the MI355X-native VIEO_SLAM hot path (libvieo_hot.so).
 *
 * The reference has no FFI layer: its boundary is three C++ classes.  Each entry
 * point below names the reference interface it replaces (file:line relative to the reference
 * root); INTEGRATION.md shows the C++ shim (VIEO_SLAM::ORBextractor / ORBmatcher / Optimizer with
 * the reference signatures) that forwards to these.  Plain pointers and sizes only; no C++ /
 * torch / OpenCV types.  Every function returns an int status: VIEO_OK (0) or a negative
 * VIEO_E_* code, unless stated otherwise.  Nothing here falls back to a CPU implementation: when
 * no gfx950 device (or no kernel image for it) is present, create() fails with VIEO_E_NO_DEVICE.
 *
 * Pointer naming: h_* = host memory, d_* = device (HBM) memory.
 */
#ifndef VIEO_HOT_H
#define VIEO_HOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIEO_OK 0
#define VIEO_E_INVALID (-1)    /* bad argument */
#define VIEO_E_NO_DEVICE (-2)  /* no HIP device / kernels unavailable: there is NO CPU fallback */
#define VIEO_E_HIP (-3)        /* a HIP runtime call failed; see vieo_last_error() */
#define VIEO_E_CAPACITY (-4)   /* caller buffer too small; required size reported */
#define VIEO_E_EMPTY (-5)      /* empty image (reference: operator() returns -1) */

const char* vieo_last_error(void);
/* 1 if a usable gfx950 device is visible, 0 otherwise (never throws, never computes). */
int vieo_device_available(void);
/* One process per GPU: every host thread that calls into the library selects the process's GPU first
 * (the HIP current device is per thread; torch.cuda.set_device covers only the calling thread). */
int vieo_set_device(int device);
int vieo_get_device(void);
const char* vieo_version(void);

/* ---- device memory / stream helpers (so a C, C++ or ctypes host needs no other runtime) ---- */
int vieo_dev_malloc(void** d_ptr, size_t bytes);
int vieo_dev_free(void* d_ptr);
int vieo_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int vieo_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int vieo_device_synchronize(void);
/* HIP events on a given stream (NULL = default): kernel timing without any other runtime. */
int vieo_event_create(void** ev);
int vieo_event_destroy(void* ev);
int vieo_event_record(void* ev, void* stream);
int vieo_event_elapsed_ms(void* ev0, void* ev1, float* ms);
/* Streams (hipStream_t, non-blocking), pinned host memory and asynchronous copies: frames travel over PCIe on a copy
 * stream while the previous batch is processed; vieo_stream_wait_event orders the two streams. */
int vieo_stream_create(void** stream);
int vieo_stream_destroy(void* stream);
int vieo_stream_synchronize(void* stream);
int vieo_stream_wait_event(void* stream, void* ev);
int vieo_host_alloc_pinned(void** h_ptr, size_t bytes);
int vieo_host_free_pinned(void* h_ptr);
int vieo_memcpy_h2d_async(void* d_dst, const void* h_src, size_t bytes, void* stream);
int vieo_memcpy_d2h_async(void* h_dst, const void* d_src, size_t bytes, void* stream);

/* ---------------------------------------------------------------- ORB extractor ------------
 * Replaces VIEO_SLAM::ORBextractor (include/ORBextractor.h:27-80, src/ORBextractor.cc:391-1081).
 */

/* Same memory layout as cv::KeyPoint (28 bytes): the C++ shim memcpy's. */
typedef struct vieo_keypoint {
  float x, y;     /* level-0 pixel coordinates */
  float size;     /* 31 * scale[octave] truncated (ORBextractor.cc:787) */
  float angle;    /* degrees, cv::fastAtan2 of the intensity centroid */
  float response; /* FAST score */
  int32_t octave;
  int32_t class_id; /* always -1 */
} vieo_keypoint;

typedef struct vieo_orb vieo_orb; /* opaque */

/* ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (ORBextractor.cc:391-456).  Device buffers are sized lazily at the first extract call. */
int vieo_orb_create(vieo_orb** out, int nfeatures, float scale_factor, int nlevels,
                    int ini_th_fast, int min_th_fast);
void vieo_orb_destroy(vieo_orb* e);

/* Getters of include/ORBextractor.h:42-52 (tables are float[nlevels]). */
int vieo_orb_levels(const vieo_orb* e);
float vieo_orb_scale_factor(const vieo_orb* e);
int vieo_orb_scale_factors(const vieo_orb* e, float* h_out);
int vieo_orb_inv_scale_factors(const vieo_orb* e, float* h_out);
int vieo_orb_level_sigma2(const vieo_orb* e, float* h_out);
int vieo_orb_inv_level_sigma2(const vieo_orb* e, float* h_out);
int vieo_orb_features_per_level(const vieo_orb* e, int* h_out);
/* Upper bound on keypoints one image can return (nfeatures + 3*nlevels + slack). */
int vieo_orb_max_keypoints(const vieo_orb* e);

/* int ORBextractor::operator()(image, mask, keypoints, descriptors, pvLappingArea)
 * (ORBextractor.cc:968-1058), host buffers in/out, synchronous.
 *   h_image: 8-bit grey, `stride` bytes per row.        h_lapping: NULL or int[2].
 *   h_keypoints[capacity], h_descriptors[capacity*32].
 *   *n_keypoints = number written; *mono_index = the reference's return value (0 without
 *   lapping area).  Returns VIEO_E_EMPTY for an empty image (reference returns -1). */
int vieo_orb_extract(vieo_orb* e, const uint8_t* h_image, int width, int height, int stride,
                     const int* h_lapping, vieo_keypoint* h_keypoints, uint8_t* h_descriptors,
                     int capacity, int* n_keypoints, int* mono_index);

/* Batched, device-resident form of the same call: n_images frames of identical size, image i at
 * d_images + i*image_pitch_bytes.  Asynchronous on the extractor's stream; outputs stay in HBM:
 *   d_keypoints  [n_images][capacity]      d_descriptors [n_images][capacity][32]
 *   d_counts     [n_images][2] int32 = {n_keypoints, mono_index}
 * This is the form the frame-sharded throughput path (bench.py) uses. */
int vieo_orb_extract_batch_device(vieo_orb* e, const uint8_t* d_images, int n_images, int width,
                                  int height, int stride, size_t image_pitch_bytes,
                                  const int* h_lapping, vieo_keypoint* d_keypoints,
                                  uint8_t* d_descriptors, int capacity, int32_t* d_counts);
int vieo_orb_sync(vieo_orb* e);

/* mvImagePyramid (include/ORBextractor.h:54, read by Frame.cc:457,536-557): size and pixels of
 * pyramid level `level` of image `image_index` of the LAST call, valid until the next call.
 * with_border != 0 returns the (w+38)x(h+38) plane with the 19-px BORDER_REFLECT_101 frame that
 * ComputePyramid builds (ORBextractor.cc:1060-1081); the ROI origin is then at (+19,+19). */
int vieo_orb_level_size(const vieo_orb* e, int level, int* width, int* height);
int vieo_orb_get_level(vieo_orb* e, int image_index, int level, int with_border, uint8_t* h_dst,
                       int dst_stride);
/* Device view of the same plane (borderless): pointer + pitch, for device-side consumers
 * (the rectified stereo matcher reads it in place). */
int vieo_orb_level_device(vieo_orb* e, int image_index, int level, const uint8_t** d_ptr,
                          int* pitch);

/* Wall-clock-free timing of the kernels of the last batch call, measured with HIP events on the
 * extractor's own stream: milliseconds for {pyramid, fast, quadtree, blur, describe, total}. */
#define VIEO_ORB_NSTAGES 6
int vieo_orb_enable_timing(vieo_orb* e, int on); /* also resets the step counter */
int vieo_orb_last_stage_ms(vieo_orb* e, float* h_ms /*[VIEO_ORB_NSTAGES]*/);
/* The stamps of the last 64 batch calls are kept, so K steps can be timed with no host sync in
 * between: steps_back = 0 is the most recent call. */
int vieo_orb_timed_steps(vieo_orb* e);
int vieo_orb_stage_ms(vieo_orb* e, int steps_back, float* h_ms /*[VIEO_ORB_NSTAGES]*/);

/* ---------------------------------------------------------------- Hamming matching ---------
 * Replaces the descriptor searches of src/Frame.cc (stereo) on top of
 * ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1645-1667: Hamming distance of 32-byte rows).
 */

/* cv::BFMatcher(cv::NORM_HAMMING).knnMatch(query, train, matches, 2) as called by
 * Frame::ComputeStereoFishEyeMatches (src/Frame.cc:18,620-628): for every query row the two
 * nearest train rows, ascending distance, ties -> lower train index first.
 * idx/dist are [nq][2] int32; a missing neighbour is (-1, INT_MAX). */
int vieo_hamming_knn2(const uint8_t* h_query, int nq, const uint8_t* h_train, int nt,
                      int32_t* h_idx, int32_t* h_dist);
/* Batched device form over the output arrays of vieo_orb_extract_batch_device: pair p searches
 * image h_pairs[2p] (query) against image h_pairs[2p+1] (train), both restricted to rows
 * [mono_index, n) like the reference (descriptors.rowRange(num_mono, n)); h_counts is the host
 * copy of d_counts.  Results of pair p start at row p*capacity; indices are relative to the
 * train sub-matrix.  Asynchronous on `stream` (a hipStream_t, may be NULL). */
int vieo_hamming_knn2_batch_device(const uint8_t* d_descriptors, const int32_t* h_counts,
                                   int capacity, const int32_t* h_pairs, int n_pairs,
                                   int32_t* d_idx, int32_t* d_dist, void* stream);
/* The same search for a batch of camera-rig frames with the counts read ON THE DEVICE (no host copy, no synchronisation):
 * d_descriptors [n_frames][n_cams][capacity][32], d_counts [n_frames][n_cams][2] = {n, num_mono}; every camera pair
 * (i < j) of every frame, rows [num_mono, n) of camera i against those of camera j (src/Frame.cc:618-628); results of
 * (frame f, pair p) start at row (f * n_pairs + p) * capacity, n_pairs = n_cams (n_cams - 1) / 2.  One launch: a lane
 * owns a query row, the train rows pass through LDS in tiles of 256 (k_knn2, matching.hip). */
int vieo_hamming_knn2_rig_batch_device(const uint8_t* d_descriptors, const int32_t* d_counts, int capacity, int n_cams,
                                       int n_frames, int32_t* d_idx, int32_t* d_dist, void* stream);

/* void Frame::ComputeStereoFishEyeMatches(const float th_far_pts) (src/Frame.cc:613-779), the stereo stage of
 * the distorted multi-camera configurations: dense knn-2 between every camera pair (rows [num_mono, n)),
 * Lowe ratio 0.7 / (<75 and 0.9) (:661-663), camm::GeometricCamera::FillMatchesFromPair with
 * USE_STRATEGY_MIN_DIST (common/config.h:12; camera_base.h:408-574: UnProject, parallax gate, DLT triangulation
 * :576-608, positive depth, reprojection chi2 5.991*sigma2), the second pass with the far-point parallax
 * threshold when fewer than 30 matches survive, the all-camera re-triangulation of every group when
 * n_cams > 2 (:704-737), and vdepth_ of the concatenated key list (:742-764).
 *   device: everything -- the knn-2 searches, every pair / group triangulation and (round 4) the order-dependent group
 *   bookkeeping; this host-pointer form is one upload, the device stage below, one download.
 * Outputs: h_depth / h_key_group [sum n_keys] in mvKeys order (camera-major): depth in the key's own camera
 * (-1: none) and mapcamidx2idxs_ (-1: none); the groups mvidxsMatches (h_group_idx [n_groups][n_cams], -1:
 * none), goodmatches_, v3dpoints_ (reference-camera frame).  VIEO_E_CAPACITY when more than group_capacity
 * groups form. */
typedef struct vieo_fisheye_params {
  int32_t n_cams;   /* 2..4 */
  int32_t n_levels; /* entries of level_sigma2 */
  float bf;         /* stereoinfo_.baseline_bf_[1] */
  float th_far_pts; /* <= 0: the two parallax thresholds stay 0.9998 and 1 - 1e-6 */
  const struct vieo_camera* cams; /* model + float parameters of mpCameras[i] (Rcb / tcb unused here) */
  const double* Trc;         /* [n_cams][12] row-major 3x4 of mpCameras[i]->GetTrc().cast<double>() */
  const double* Tcr;         /* [n_cams][12] row-major 3x4 of mpCameras[i]->GetTcr().cast<double>() */
  const float* level_sigma2; /* scalepyrinfo_.vlevelsigma2_ */
} vieo_fisheye_params;

int vieo_stereo_fisheye_match(const vieo_fisheye_params* params, const vieo_keypoint* const* h_keys /*[n_cams]*/,
                              const uint8_t* const* h_descriptors /*[n_cams] rows of 32 bytes*/,
                              const int32_t* n_keys /*[n_cams]*/, const int32_t* num_mono /*[n_cams]*/,
                              int32_t group_capacity, float* h_depth, int32_t* h_key_group,
                              int32_t* h_group_idx, uint8_t* h_group_good, double* h_group_p3d,
                              int32_t* n_groups, int32_t* n_matches);

/* Device-resident form (round 4): the whole stage -- knn-2 of every camera pair, ratio test + pair triangulation, the
 * group tables of FillMatchesFromPair, the all-camera re-triangulation, mvKeys / mDescriptors / vdepth_ -- as five
 * launches on `stream` with no host round trip: the key counts are read on the device, and the order-dependent group
 * bookkeeping runs as a speculative-parallel walk on one wavefront per frame (rows that touch disjoint keys / groups
 * are applied 64 at a time with the sequential result; fisheye_stereo.hip).  A handle carries the rig's constants and
 * the scratch for up to max_frames frames of key_cap_per_camera (<= 8191) keys per camera.
 * Inputs are the extractor's batch arrays: d_keys / d_desc [n_frames][n_cams][key_cap_per_camera], d_counts
 * [n_frames][n_cams][2] = {n, num_mono} (vieo_orb_extract_batch_device with n_images = n_frames * n_cams).
 * Outputs, per frame: d_keys_cat / d_desc_cat / d_depth / d_uright / d_key_group [n_cams * key_cap_per_camera] in mvKeys
 * (camera-major) order, d_cam_first [n_cams + 1], d_frame_counts [2] = {N, 0} (the counts layout the vieo_track_* glue
 * reads); the groups d_group_idx [gcap][n_cams], d_group_good [gcap],
 * d_group_p3d [gcap][3] with gcap = vieo_fisheye_group_capacity(); d_hdr [8] = {n_groups, n_matches, threshold used
 * (0 / 1), status (1: more than gcap groups, the frame's tables are void), -, rows walked, wavefront steps, -}. */
typedef struct vieo_fisheye vieo_fisheye;
int vieo_fisheye_create(vieo_fisheye** out, const vieo_fisheye_params* params, int key_cap_per_camera, int max_frames);
void vieo_fisheye_destroy(vieo_fisheye* h);
int vieo_fisheye_group_capacity(const vieo_fisheye* h);
int vieo_stereo_fisheye_match_batch_device(vieo_fisheye* h, const vieo_keypoint* d_keys, const uint8_t* d_desc,
                                           const int32_t* d_counts, int n_frames, vieo_keypoint* d_keys_cat,
                                           uint8_t* d_desc_cat, int32_t* d_cam_first, int32_t* d_frame_counts,
                                           float* d_depth, float* d_uright, int32_t* d_key_group, int32_t* d_group_idx, uint8_t* d_group_good,
                                           double* d_group_p3d, int32_t* d_hdr, void* stream);
/* The same stage in two parts, for a caller that lets the tracking of a frame run beside its stereo bookkeeping: what
 * tracking reads of a rig frame -- the concatenated keys / descriptors, the cameras' ranges, uright = -1 -- does not
 * depend on the matches (VIEO_FISHEYE_CONCAT, one short kernel); the matches, the groups and the keys' depths
 * (VIEO_FISHEYE_GROUPS) are outputs of the frame only and may run on another stream.  CONCAT + GROUPS = ALL. */
#define VIEO_FISHEYE_ALL 0
#define VIEO_FISHEYE_CONCAT 1
#define VIEO_FISHEYE_GROUPS 2
int vieo_stereo_fisheye_match_batch_device_part(vieo_fisheye* h, const vieo_keypoint* d_keys, const uint8_t* d_desc,
                                           const int32_t* d_counts, int n_frames, vieo_keypoint* d_keys_cat,
                                           uint8_t* d_desc_cat, int32_t* d_cam_first, int32_t* d_frame_counts,
                                           float* d_depth, float* d_uright, int32_t* d_key_group, int32_t* d_group_idx, uint8_t* d_group_good,
                                           double* d_group_p3d, int32_t* d_hdr, int part, void* stream);
/* test tap: rows walked / wavefront steps of this thread's last vieo_stereo_fisheye_match */
void vieo_fisheye_last_walk(int32_t* rows, int32_t* steps);

/* int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, vMatchedPairs, bOnlyStereo)
 * (src/ORBmatcher.cc:896-1150; LocalMapping::CreateNewMapPoints, LocalMapping.cc:709): per shared vocabulary node,
 * every unmatched key of pKF1 against the unmatched keys of pKF2 -- Hamming <= TH_LOW (50), best per image of pKF2,
 * the epipole gate for two monocular keys, the epipolar constraint (GeometricCamera::epipolarConstrain,
 * camera_base.h:287-406, fundamental-matrix branch, 3.84 sigma2; distorted keys are un-projected first) -- then
 * FillMatchesFromPair (USE_STRATEGY_MIN_DIST) and the rotation-histogram filter.
 *   device: all gates of all (key1, key2) pairs of the shared nodes, for a batch of pKF2 at once;
 *   host (inside the library): the order-dependent part (skip keys already taken, best distance, group tables).
 * mFeatVec comes from vieo_bow_transform (or from the caller's DBoW2): nodes ascending, CSR over feature indices.
 * Both key frames of a pair are of one kind: n_cams == 0 (usedistort_ false: one undistorted pinhole camera, keys =
 * mvKeysUn) or n_cams 1..4 (a distorted rig: keys = mvKeys, camera-major). */
typedef struct vieo_tri_keyframe {
  double Tcw[12];              /* GetTcw() of the reference camera: row-major 3x4 */
  float fx, fy, cx, cy;        /* mpCameras[0] (pinhole), n_cams == 0 */
  int32_t n_keys, n_nodes;
  const vieo_keypoint* keys;   /* mvKeysUn / mvKeys (pt, angle, octave) */
  const uint8_t* descriptors;  /* mDescriptors, 32 bytes per key */
  const float* uright;         /* stereoinfo_.vuright_ (< 0: monocular key) */
  const uint8_t* has_mappoint; /* GetMapPoint(idx) != NULL */
  const uint32_t* node_id;     /* mFeatVec: node ids, ascending */
  const int32_t* node_first;   /* [n_nodes + 1] offsets into node_feat */
  const int32_t* node_feat;    /* feature indices of each node, in the vector's order */
  const float* scale_factor;   /* scalepyrinfo_.vscalefactor_ */
  const float* level_sigma2;   /* scalepyrinfo_.vlevelsigma2_ */
  int32_t n_levels, n_cams;
  const struct vieo_camera* cams; /* [n_cams] model + parameters of mpCameras[i] (Rcb / tcb unused here) */
  const double* Tcr;           /* [n_cams][12] mpCameras[i]->GetTcr() as row-major 3x4 */
  const double* Trc;           /* [n_cams][12] mpCameras[i]->GetTrc() */
  const uint8_t* key_cam;      /* [n_keys] get<0>(mapn2in_[idx]): the camera of each key */
} vieo_tri_keyframe;           /* 232 bytes */
/* kf2s[n_kf2]: the neighbours of kf1, each an independent call of the reference.  Outputs per neighbour p:
 * h_pairs[(p * pair_capacity + m) * pair_stride + c] = the key of camera c in match m of vMatchedPairs (its
 * order; cameras of pKF1 first, then those of pKF2; -1: none; pair_stride >= the number of cameras of the pair,
 * 2 for undistorted key frames), h_n_pairs[p] their count, h_n_matches[p] the reference's return value.
 * VIEO_E_CAPACITY when a neighbour has more matches than pair_capacity. */
int vieo_search_for_triangulation(const vieo_tri_keyframe* kf1, const vieo_tri_keyframe* kf2s, int n_kf2,
                                  int only_stereo, int check_orientation, int32_t pair_capacity, int32_t pair_stride,
                                  int32_t* h_pairs, int32_t* h_n_pairs, int32_t* h_n_matches);

/* LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:650-830), what it does with the rows SearchForTriangulation
 * returns -- PrepareDatasForTraingulate (:560-649), GeometricCamera::TriangulateMatches (camera_base.h:199-285; the
 * DLT of Triangulate :576-608 over all keys of the row, up to 8 cameras) or KeyFrame::UnprojectStereo of the side with
 * the larger stereo parallax checked by TriangulateMatches(just_check_p3d), then the distance, th_far_pts and scale
 * consistency gates (:781-806) -- one lane per row, every neighbour in one launch.  The host keeps `new MapPoint`,
 * AddObservation / AddMapPoint and the two batched map-point calls (vieo_distinctive_descriptors_batch,
 * vieo_update_normal_and_depth_batch).  The monocular baseline test (ComputeSceneMedianDepth, :699-705) is not
 * provided: no configuration is monocular; the stereo / RGB-D / rig test of :698 is. */
typedef struct vieo_tri_stereo {   /* per key frame, beside its vieo_tri_keyframe */
  float Ow[3];                     /* GetCameraCenter() */
  float baseline, bf;              /* stereoinfo_.baseline_bf_[0], [1] */
  const float* depth;              /* stereoinfo_.vdepth_ [n_keys] */
  const int32_t* key_group;        /* rigs: GetMapn2idxs(i), -1 none; NULL for n_cams == 0 (or a rig without groups) */
  const double* group_p3d;         /* rigs: stereoinfo_.v3dpoints_ [n_groups][3], n_groups > every key_group entry */
} vieo_tri_stereo;                 /* 48 bytes */
/* status of a row: >= 0 accepted (a new map point), < 0 the reason it is not */
#define VIEO_NEWPT_DLT 0            /* triangulated from all keys of the row */
#define VIEO_NEWPT_STEREO1 1        /* pKF1->UnprojectStereo(first key), checked against all keys */
#define VIEO_NEWPT_STEREO2 2        /* pKF2->UnprojectStereo(first key), checked against all keys */
#define VIEO_NEWPT_NO_KEY (-1)      /* a side of the row has no key */
#define VIEO_NEWPT_LOW_PARALLAX (-2) /* no stereo key and the rays' parallax is too low (or >= 90 degrees) */
#define VIEO_NEWPT_TRI_EMPTY (-3)   /* TriangulateMatches returned empty (parallax, x4[3] == 0, depth <= 0, chi2), or
                                     * UnprojectStereo had no point (the reference asserts there) */
#define VIEO_NEWPT_ZERO_DIST (-4)   /* the point is a camera centre */
#define VIEO_NEWPT_FAR (-5)         /* th_far_pts > 0 and max(dist1, dist2) >= th_far_pts */
#define VIEO_NEWPT_SCALE (-6)       /* scale consistency, ratioFactor = 1.5f * scale_factor[1] of pKF1 */
#define VIEO_NEWPT_SKIPPED (-7)     /* the neighbour's baseline is shorter than its stereo baseline (:698) */
/* Takes the rows in the layout vieo_search_for_triangulation writes (h_pairs, h_n_pairs; same pair_capacity and
 * pair_stride).  Per row m of neighbour p, at index p * pair_capacity + m: h_status (VIEO_NEWPT_*), h_x3d[3] the
 * point (double, as TriangulateMatches leaves it) and h_x3d_f[3] = what MapPoint stores (float); both zero unless
 * accepted.  h_n_new[p] = accepted rows of neighbour p.  A neighbour that fails the baseline test is skipped: its rows
 * get VIEO_NEWPT_SKIPPED and h_n_new[p] = 0.  n_kf2 == 0 is VIEO_OK and writes nothing.  VIEO_E_INVALID: null pointer,
 * mixed key-frame kinds, n_cams > 4, a key index out of range; VIEO_E_CAPACITY: h_n_pairs[p] > pair_capacity.
 * Re-entrant per host thread like the search. */
int vieo_triangulate_new_points(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1,
                                const vieo_tri_keyframe* kf2s, const vieo_tri_stereo* st2s, int n_kf2,
                                float th_far_pts, int32_t pair_capacity, int32_t pair_stride, const int32_t* h_pairs,
                                const int32_t* h_n_pairs, int8_t* h_status, double* h_x3d, float* h_x3d_f,
                                int32_t* h_n_new);
/* The search and the triangulation in one call: the outputs of vieo_search_for_triangulation (h_pairs, h_n_pairs,
 * h_n_matches) and those of vieo_triangulate_new_points, byte for byte what the two calls give one after the other
 * for every neighbour that passes the baseline test.  A neighbour that fails it is not searched, as in the reference:
 * its three counts are 0.  The key arrays and cameras uploaded for the gates stay on the device for the
 * triangulation; only the rows go up after the host bookkeeping. */
int vieo_create_new_map_points(const vieo_tri_keyframe* kf1, const vieo_tri_stereo* st1, const vieo_tri_keyframe* kf2s,
                               const vieo_tri_stereo* st2s, int n_kf2, int only_stereo, int check_orientation,
                               float th_far_pts, int32_t pair_capacity, int32_t pair_stride, int32_t* h_pairs,
                               int32_t* h_n_pairs, int32_t* h_n_matches, int8_t* h_status, double* h_x3d,
                               float* h_x3d_f, int32_t* h_n_new);

/* void Frame::ComputeStereoMatches() (src/Frame.cc:451-611), rectified stereo: row-band Hamming
 * search (octave +-1, disparity window [0, bf/baseline]), 11 SADs of 11x11 patches on the
 * left key's pyramid level, parabola sub-pixel fit, rejection above 1.5*1.4*median SAD.
 * Outputs stereoinfo_.vuright_ / vdepth_ (-1 = no match).  `left`/`right` are the two
 * extractors that just processed the frame's images (their mvImagePyramid is read in place on
 * the device); `baseline` = stereoinfo_.baseline_bf_[0], `bf` = baseline_bf_[1]. */
int vieo_stereo_match_rectified(vieo_orb* left, vieo_orb* right, const vieo_keypoint* h_kpL,
                                const uint8_t* h_descL, int nL, const vieo_keypoint* h_kpR,
                                const uint8_t* h_descR, int nR, float baseline, float bf,
                                float* h_uright, float* h_depth);
/* Batched device form: the extractor's last batch holds 2*n_frames images, image 2f = left and
 * 2f+1 = right camera of frame f; keypoints/descriptors/counts are that batch's outputs.
 * d_uright / d_depth are [n_frames][capacity].  Asynchronous on the extractor's stream. */
int vieo_stereo_match_rectified_batch_device(vieo_orb* e, int n_frames,
                                             const vieo_keypoint* d_keypoints,
                                             const uint8_t* d_descriptors, const int32_t* d_counts,
                                             int capacity, float baseline, float bf,
                                             float* d_uright, float* d_depth);

/* camm::Camera of one physical camera as an EdgeReproject sees it (a20: common/camera_models/
 * camera_pinhole.h:70-106, camera_radtan.h:61-129, camera_kb8.h:68-157), with EdgeReproject::SetParams
 * (g2otypes.h:409-416) already applied to the extrinsics: Rcb = Rccr * Rcrb, tcb = Rccr * tcrb + tcr. */
#define VIEO_CAM_PINHOLE 0
#define VIEO_CAM_RADTAN 1
#define VIEO_CAM_KB8 2
typedef struct vieo_camera {
  int32_t model;   /* VIEO_CAM_* */
  int32_t num_k;   /* Radtan: number of radial coefficients (parameters.size() - 6), else unused */
  float fx, fy, cx, cy;
  float dist[8];   /* Radtan: k1..k_num_k, p1, p2;  KB8: k1..k4 */
  double Rcb[9], tcb[3];
} vieo_camera;

/* ---------------------------------------------------------------- projection search ---------
 * Replaces the tracking-side ORBmatcher::SearchByProjection overloads (src/ORBmatcher.cc:230-335
 * and :1303-1467) on flattened inputs.  The window query is FrameBase::GetFeaturesInArea
 * (src/FrameBase.cpp:95-141, 64x48 grid order: cell column, cell row, key index).
 */
typedef struct vieo_proj_query { /* one map point projected into one camera: 64 bytes */
  float u, v, ur;                /* projection; ur is compared with stereo keypoints only */
  float radius;                  /* window half-size in pixels (th * scale already applied) */
  int32_t level_min, level_max;  /* GetFeaturesInArea(minlevel, maxlevel); level_max < 0: no max */
  float angle;                   /* angle of the query's own keypoint (rotation check, a12) */
  int32_t flags;                 /* bit0: valid; bit1: the map point has Observations() > 0;
                                  * bits 8..11: camera of a rig frame (0 for the single-camera entries) */
  uint8_t desc[32];              /* MapPoint::GetDescriptor() */
} vieo_proj_query;

typedef struct vieo_last_frame_point { /* LastFrame.mvpMapPoints[i] flattened: 64 bytes */
  float Xw[3];       /* MapPoint::GetWorldPos() */
  int32_t octave;    /* LastFrame.mvKeys[i].octave */
  float angle;       /* LastFrame.mvKeys[i].angle */
  int32_t flags;     /* bit0: pMP != NULL && !LastFrame.mvbOutlier[i]; bit1: Observations() > 0 */
  int32_t reserved[2]; /* [0]: read by the frame tracker only -- 1 + the index of the FIRST key of LastFrame that holds the
                        * same MapPoint (a rig frame's point is held by one key per camera), 0: this key */
  uint8_t desc[32];
} vieo_last_frame_point;

typedef struct vieo_sbp_camera {
  double Tcw_cur[12], Tcw_last[12]; /* 3x4 row-major [R|t] of CurrentFrame / LastFrame */
  float fx, fy, cx, cy;
  float bounds[4];                  /* gridinfo_.minmax_xy_: min_x, max_x, min_y, max_y */
  float bf, baseline;               /* stereoinfo_.baseline_bf_[1], [0] */
  float th, th_far;                 /* window threshold; far-point cut (<= 0: off) */
  int32_t mono, nlevels;
  float scale[16];                  /* scalepyrinfo_.vscalefactor_ */
} vieo_sbp_camera;

#define VIEO_SBP_LAST_FRAME 0 /* accept best <= TH_HIGH, rotation histogram (ORBmatcher.cc:1303-1467) */
#define VIEO_SBP_LOCAL_MAP 1  /* best/second ratio test when same level (ORBmatcher.cc:230-335) */
#define VIEO_SBP_RELOC 2      /* a14 ORBmatcher.cc:1471-1606: SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th,
                                * ORBdist): keys holding ANY map point are skipped, no stereo gate, best only,
                                * accepted if dist <= ORBdist (passed in nn_ratio), rotation histogram as mode 0;
                                * queries = the key frame's map points (not in sAlreadyFound) projected with
                                * levels [L-1, L+1], radius th*scale[L], angle = pKF->mvKeys[i].angle */
#define VIEO_SBP_UNCHANGED (-1)
#define VIEO_SBP_ERASED (-2)

/* Projection part of SearchByProjection(Frame&, const Frame&, th, bMono, th_far)
 * (ORBmatcher.cc:1313-1378): last frame's valid map points -> window queries. */
int vieo_sbp_project_last_frame(const vieo_last_frame_point* h_points, int n,
                                const vieo_sbp_camera* h_cam, vieo_proj_query* h_queries);
/* The search + sequential assignment of both overloads.  h_taken[i] != 0 when keypoint i already
 * holds a map point with Observations() > 0.  h_assign[n_keys]: VIEO_SBP_UNCHANGED, VIEO_SBP_ERASED
 * (EraseMapPointMatch by the rotation check) or the index of the query whose map point
 * AddMapPoint() put there.  *nmatches = the reference's return value. */
int vieo_search_by_projection(int mode, const vieo_proj_query* h_queries, int nq,
                              const vieo_keypoint* h_keys, const float* h_uright,
                              const uint8_t* h_desc, const uint8_t* h_taken, int n_keys,
                              const float* h_bounds /*[4]*/, float nn_ratio, int check_orientation,
                              int32_t* h_assign, int32_t* nmatches);
/* Batched device form: frame f owns queries [f*q_cap, f*q_cap + d_nq[f]) and the key arrays of
 * image img_first + f*img_step of an extractor batch (d_counts as written by the extractor).
 * The search entries keep their scratch (candidate pool, cursors, grid CSRs) per HOST THREAD, not per stream: a thread
 * issues its searches on ONE stream, or synchronises between searches it issues on different streams. */
int vieo_search_by_projection_batch_device(int mode, const vieo_proj_query* d_queries,
                                           const int32_t* d_nq, int q_cap, int n_frames,
                                           const vieo_keypoint* d_keys, const float* d_uright,
                                           const uint8_t* d_desc, const uint8_t* d_taken,
                                           const int32_t* d_counts, int key_cap, int img_first,
                                           int img_step, const float* h_bounds, float nn_ratio,
                                           int check_orientation, int32_t* d_assign,
                                           int32_t* d_nmatches, void* stream);
int vieo_sbp_project_last_frame_batch_device(const vieo_last_frame_point* d_points,
                                             const int32_t* d_n, int p_cap, int n_frames,
                                             const vieo_sbp_camera* d_cams,
                                             vieo_proj_query* d_queries, void* stream);

/* ---- the same searches for frames of a camera rig (Frame::mpCameras.size() cameras, distorted or not) -------
 * The reference loops the cameras inside every overload: SearchByProjection(Frame&, const Frame&) projects each
 * last-frame point into every camera camj with mpCameras[camj]->GetTcr() and, when Frame::usedistort_, the camera
 * model's Project() (ORBmatcher.cc:1339-1366); the local-map overload walks the point's vtrack_cami_ list
 * (:257-266); the relocalisation overload loops cami (:1491-1543).  Every (point, camera) pair is one query, in
 * point-major order -- that is the order in which keys are claimed -- and its camera travels in bits 8..11 of
 * vieo_proj_query.flags.  The window query is GetFeaturesInArea(cami, ...) on that camera's 64 x 48 grid
 * (FrameBase.cpp:95-141); the frame's keys are mvKeys in camera-major order (Frame.cc:738-764), camera c owning
 * the keys [cam_first[c], cam_first[c + 1]).  One rotation histogram is shared by all cameras. */
typedef struct vieo_sbp_rig {
  int32_t n_cams;      /* 1..4 */
  int32_t use_distort; /* Frame::usedistort_: 1 -> mpCameras[c]->Project(), 0 -> K * (x/z, y/z, 1) in float */
  vieo_camera cams[4]; /* model + float parameters of mpCameras[c] (Rcb / tcb unused here) */
  double Tcr[4][12];   /* mpCameras[c]->GetTcr().cast<double>(), row-major 3x4 (identity for the reference camera) */
  double trc[4][3];    /* mpCameras[c]->GetTrc().translation().cast<double>() (camera centre, relocalisation variant) */
  float bounds[4][4];  /* gridinfo_.minmax_xy_[c]: min_x, max_x, min_y, max_y */
} vieo_sbp_rig;        /* 1160 bytes */

/* pKF->GetMapPointMatches()[i] of the relocalisation overload, flattened: 64 bytes, the layout of
 * vieo_last_frame_point with the two distances in place of `reserved`. */
typedef struct vieo_keyframe_point {
  float Xw[3];       /* MapPoint::GetWorldPos() */
  int32_t octave;    /* unused (the level is predicted from the distance) */
  float angle;       /* pKF->mvKeys[i].angle */
  int32_t flags;     /* bit0: pMP != NULL && !isBad() && not in sAlreadyFound; bit1: Observations() > 0 */
  float max_distance, min_distance; /* mfMaxDistance, mfMinDistance (the 1.2 / 0.8 factors are applied here) */
  uint8_t desc[32];
} vieo_keyframe_point;

/* ORBmatcher.cc:1313-1378 with the camera loop: h_queries[i * n_cams + camj].  h_cam supplies the poses, bf,
 * baseline, th, th_far, mono and the scale factors; its fx..cy / bounds are not read (h_rig has them). */
int vieo_sbp_project_last_frame_rig(const vieo_last_frame_point* h_points, int n, const vieo_sbp_camera* h_cam,
                                    const vieo_sbp_rig* h_rig, vieo_proj_query* h_queries /*[n * n_cams]*/);
/* Projection part of SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist, th_far)
 * (ORBmatcher.cc:1487-1543): Tcr, Project / K, IsInImage, the scale-invariance distances, MapPoint::PredictScale,
 * window th * scale[level], levels [L-1, L+1].  h_cam: Tcw_cur, th, th_far, nlevels, scale;
 * log_scale_factor = scalepyrinfo_.flogscalefactor_.  h_rig == NULL: the one rectified camera of h_cam. */
int vieo_sbp_project_keyframe(const vieo_keyframe_point* h_points, int n, const vieo_sbp_camera* h_cam,
                              const vieo_sbp_rig* h_rig, float log_scale_factor,
                              vieo_proj_query* h_queries /*[n * n_cams]*/);
/* vieo_search_by_projection on the camera-major key list of a rig frame.  h_bounds: [n_cams][4]. */
int vieo_search_by_projection_rig(int mode, const vieo_proj_query* h_queries, int nq, const vieo_keypoint* h_keys,
                                  const float* h_uright, const uint8_t* h_desc, const uint8_t* h_taken, int n_keys,
                                  const int32_t* h_cam_first /*[n_cams + 1]*/, const float* h_bounds, int n_cams,
                                  float nn_ratio, int check_orientation, int32_t* h_assign, int32_t* nmatches);
/* Batched device forms.  Frame f owns the queries [f * q_cap, f * q_cap + d_nq[f]) and the key arrays
 * [f * key_cap, f * key_cap + d_cam_first[f * (n_cams + 1) + n_cams]) (already concatenated camera-major);
 * d_rigs: one vieo_sbp_rig per frame; h_bounds [n_cams][4] shared by all frames. */
int vieo_sbp_project_last_frame_rig_batch_device(const vieo_last_frame_point* d_points, const int32_t* d_n,
                                                 int p_cap, int n_frames, const vieo_sbp_camera* d_cams,
                                                 const vieo_sbp_rig* d_rigs, int n_cams,
                                                 vieo_proj_query* d_queries /*[n_frames][p_cap * n_cams]*/,
                                                 void* stream);
int vieo_search_by_projection_rig_batch_device(int mode, const vieo_proj_query* d_queries, const int32_t* d_nq,
                                               int q_cap, int n_frames, const vieo_keypoint* d_keys,
                                               const float* d_uright, const uint8_t* d_desc,
                                               const uint8_t* d_taken, const int32_t* d_cam_first, int key_cap,
                                               const float* h_bounds, int n_cams, float nn_ratio,
                                               int check_orientation, int32_t* d_assign, int32_t* d_nmatches,
                                               void* stream);

/* The window grid of a search (Frame::mGrid as a CSR, built on the device by every *_batch_device search call) depends on
 * the frame's keys only.  vieo_sbp_keep_grid(1) tells the NEXT search call of this host thread that its key arrays hold what
 * the previous call's held (same device pointers, geometry and stream are checked, the contents are the caller's promise):
 * the grid is then not rebuilt -- TrackLocalMap's search after TrackWithIMU's in the one-call tracker.  One call only. */
int vieo_sbp_keep_grid(int on);

/* ---- the resident frame: the drop-in path's fast form (round 5) -------------------------------------------------
 * The reference's callers reach this library one class member at a time -- Frame::Frame -> ExtractORB per camera thread
 * (src/Frame.cc:259-278) -> ComputeStereoMatches (:451-611) -> ORBmatcher::SearchByProjection (src/Tracking.cc:296, :2599)
 * -> Optimizer::PoseOptimization (:321,333) -- and every member's signature hands over host objects.  Nothing in those
 * signatures says the data must travel: vieo_orb_extract LEAVES the image's keys, descriptors and pyramid in HBM, in the
 * extractor handle the Frame already points at (mpORBextractors[c]), and the entries below read them there.  A call
 * uploads only what the pointer graph forces (the last frame's map points, the window queries, the taken flags), runs on
 * the handle's stream and returns behind ONE synchronisation; the frame's window grid (Frame::mGrid as a CSR) is built by
 * its first search and kept for the later ones.  The shim decides per call with vieo_orb_holds whether the handle still
 * holds the frame it was given (a Frame copied long ago does not: the host-pointer entries above serve it).
 * Results are those of the host-pointer entries bit for bit (same kernels, same inputs). */
/* 1 when the handle's resident frame is the one these keys describe (count + first / last eight keys compared with what
 * the last vieo_orb_extract of this handle returned), else 0. */
int vieo_orb_holds(const vieo_orb* e, const vieo_keypoint* h_keys, int n_keys);
/* number of keys of the resident frame, -1: none */
int vieo_orb_resident_keys(const vieo_orb* e);
/* Frame::ComputeStereoMatches (src/Frame.cc:451-611) of the frame the two handles have just extracted.
 * h_uright / h_depth [vieo_orb_resident_keys(left)]; uright also stays in the left handle for the searches. */
int vieo_stereo_match_rectified_resident(vieo_orb* left, vieo_orb* right, float baseline, float bf,
                                         float* h_uright, float* h_depth);
/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono, th_far_pts)
 * (src/ORBmatcher.cc:1303-1467) as one call: vieo_sbp_project_last_frame + vieo_search_by_projection(VIEO_SBP_LAST_FRAME)
 * on the resident keys.  h_uright: NULL = the resident values of vieo_stereo_match_rectified_resident, else
 * stereoinfo_.vuright_ of the frame.  h_assign [vieo_orb_resident_keys(frame)] as in vieo_search_by_projection. */
int vieo_search_by_projection_last_frame_resident(vieo_orb* frame, const vieo_last_frame_point* h_points, int n_points,
                                                  const vieo_sbp_camera* h_cam, const float* h_uright, float nn_ratio,
                                                  int check_orientation, int32_t* h_assign, int32_t* nmatches);
/* vieo_search_by_projection on the resident keys: the local-map overload (src/ORBmatcher.cc:230-335, queries from
 * MapPoint::GetTrackInfoRef()) and the relocalisation overload (queries from vieo_sbp_project_keyframe). */
int vieo_search_by_projection_resident(int mode, vieo_orb* frame, const vieo_proj_query* h_queries, int nq,
                                       const float* h_uright, const uint8_t* h_taken, const float* h_bounds /*[4]*/,
                                       float nn_ratio, int check_orientation, int32_t* h_assign, int32_t* nmatches);

/* ---------------------------------------------------------------- pose optimisation --------
 * Replaces Optimizer::PoseOptimization (motion-only BA with fixed map points).  The host shim
 * flattens Frame / MapPoint objects into the POD structs below and writes the results back
 * (mvbOutlier, NavState, pose) exactly where the reference does (Optimizer.cc:1716,1824-1871).
 */

/* VIEO_SLAM::NavState (src/Odom/NavState.h:18-85): 22 doubles. */
typedef struct vieo_navstate {
  double p[3];  /* mpwb */
  double q[4];  /* mRwb as unit quaternion (w, x, y, z) */
  double v[3];  /* mvwb */
  double bg[3], ba[3], dbg[3], dba[3];
} vieo_navstate;


/* One 3D-2D correspondence = one EdgeReprojectPR / PRStereo (src/Odom/g2otypes.h:321-547). */
typedef struct vieo_pose_obs {
  float Xw[3];      /* MapPoint::mWorldPos, stored as float32 (include/MapPoint.h:52-53) */
  float u, v, ur;   /* mvKeysUn[i].pt and stereoinfo_.vuright_[i]; ur < 0 => monocular edge */
  float inv_sigma2; /* scalepyrinfo_.vinvlevelsigma2_[octave] */
  int32_t flags;    /* bit 0: close point (track_depth_ < max(10, ThDepth)), VIO variant only */
} vieo_pose_obs;    /* 32 bytes */

typedef struct vieo_enc_preint { /* EncPreIntegrator (src/Odom/OdomPreIntegrator.h:66-100) */
  double dt;          /* mdeltatij; 0 => no encoder edge */
  double delx[6];     /* mdelxEij: delta~Phi_ij (3), delta~p_ij (3) */
  double Sigma[36];   /* mSigmaEij, row-major */
} vieo_enc_preint;    /* 344 bytes */
/* The optional encoder edge of the pose optimisations (EdgeEncNavStatePR / PVR between the last frame and the
 * current one, Optimizer.cc:1650-1674, Optimizer.h:345-372): measurement, extrinsics, and the last frame's pose. */
typedef struct vieo_pose_enc {
  vieo_enc_preint enc;     /* pFrame->GetEncPreInt() */
  double qRbe[4], pbe[3];  /* Tbe = Frame::mTbc * Frame::mTce: rotation (w, x, y, z), translation */
  double p_last[3], q_last[4]; /* pLastF->GetNavStateRef(): mpwb, mRwb (w, x, y, z) -- the fixed vertex of a15 */
} vieo_pose_enc;           /* 456 bytes */

typedef struct vieo_pose_frame {
  vieo_navstate nav;     /* initial estimate (Frame::mNavState after UpdateNavStatePVRFromTcw) */
  double Rcb[9], tcb[3]; /* FrameBase::meigRcb (row-major) / meigtcb */
  float fx, fy, cx, cy;  /* pinhole intrinsics, float like camm::Camera::parameters_ */
  float bf;              /* stereoinfo_.baseline_bf_[1] */
  int32_t obs_begin;     /* first observation of this frame in the flat obs array */
  int32_t n_obs;
  int32_t n_cams;        /* 0: the rectified pinhole camera above; 1..4: `cams` (a20, Frame::usedistort_), and
                          * bits 8..11 of vieo_pose_obs.flags select the observation's camera (monocular edges) */
  const vieo_camera* cams; /* host pointer for the host entry points, device pointer for *_batch_device */
  const vieo_pose_enc* enc; /* NULL or enc->enc.dt == 0: no encoder edge; host / device pointer like `cams` */
} vieo_pose_frame;

/* The batched device forms cannot see n_cams from the host, so by default they launch both kernel instances
 * (rectified pinhole frames, camera-rig frames); each instance skips the other's frames.  A caller whose
 * frames are all of one kind says so once and saves the empty launch; a frame of the other kind then
 * comes back with status VIEO_E_INVALID instead of being optimised. */
#define VIEO_POSE_CAMS_AUTO 0
#define VIEO_POSE_CAMS_RECTIFIED 1 /* every frame has n_cams == 0 (Frame::usedistort_ false) */
#define VIEO_POSE_CAMS_RIG 2       /* every frame has n_cams > 0 */
int vieo_pose_set_camera_mode(int mode);
/* The same for the encoder edge of vieo_pose_optimization_vio_batch_device (EdgeEncNavStatePVR, Optimizer.h:345-363):
 * frames with base.enc->enc.dt != 0 run in their own kernel instance.  (The vision-only kernel branches at run
 * time and ignores this mode.) */
#define VIEO_POSE_ENC_AUTO 0
#define VIEO_POSE_ENC_NONE 1 /* no frame carries an encoder measurement (Frame::GetEncPreInt().mdeltatij == 0) */
#define VIEO_POSE_ENC_ALL 2  /* every frame carries one */
int vieo_pose_set_encoder_mode(int mode);

#define VIEO_POSE_OK 0
#define VIEO_POSE_TOO_FEW 1 /* < 3 correspondences: the reference returns 0 and leaves the pose */
typedef struct vieo_pose_result {
  vieo_navstate nav;  /* optimised state (p, q updated; other fields copied) */
  int32_t n_inliers;  /* return value of the reference: nInitialCorrespondences - nBad */
  int32_t status;     /* VIEO_POSE_* */
  int32_t lm_iterations; /* total LM iterations executed over the 4 rounds (diagnostic) */
  int32_t reserved;   /* visual-inertial variant: total lambda trials over the 4 rounds (diagnostic); else 0 */
} vieo_pose_result;

/* int Optimizer::PoseOptimization(Frame* pFrame, Frame* pLastF = NULL) (src/Optimizer.cc:1611-1874),
 * vision-only motion BA (the optional encoder edge to the last frame: `enc`): 4 rounds of optimize(10) from the
 * initial estimate, chi2 classification 5.991 / 7.815 after each round, Huber off after round 3.
 * h_outlier[n_obs] receives mvbOutlier of the matched keypoints. */
int vieo_pose_optimization(const vieo_pose_frame* h_frame, const vieo_pose_obs* h_obs,
                           uint8_t* h_outlier, vieo_pose_result* h_result);
/* Batched device form: one workgroup per frame, the whole 4x10 LM loop runs on the device.
 * d_obs / d_outlier are flat arrays indexed by obs_begin + i.  Asynchronous on `stream`. */
int vieo_pose_optimization_batch_device(const vieo_pose_frame* d_frames, int n_frames,
                                        const vieo_pose_obs* d_obs, uint8_t* d_outlier,
                                        vieo_pose_result* d_results, void* stream);

/* ---- visual-inertial variant --------------------------------------------------------------
 * template<class KeyFrame> int Optimizer::PoseOptimization(Frame*, KeyFrame* pLastKF,
 *     const cv::Mat& gw, bool bComputeMarg = false, bool bNoMPs = false)
 * (include/Optimizer.h:208-816), instantiated for Frame and KeyFrame by Tracking.cc:321,333,475,479.
 * Vertices: PVR_j (9) + Bias_j (6) free; PVR_i + Bias_i of the last (key)frame fixed unless it
 * carries a prior (mbPrior).  Edges: EdgeNavStatePVR (IMU pre-integration, g2otypes.h:703-884),
 * EdgeNavStateBias (g2otypes.cpp:14-34), EdgeNavStatePriorPVRBias (g2otypes.cpp:84-124),
 * EdgeReprojectPVR / PVRStereo per correspondence, and EdgeEncNavStatePVR (g2otypes.h:591-668, Optimizer.h:345-363)
 * when base.enc carries a measurement: between PVR_i and PVR_j (base.enc->p_last / q_last are not read here, the
 * last state is nav_last), Huber sqrt(12.592), information Sigma_E^-1; it also enters the marginal prior
 * (FillCovInv, Optimizer.h:195-204) and counts as the odometry edge that keeps the estimate between the rounds. */
typedef struct vieo_imu_preint { /* IMUPreIntegratorBase (src/Odom/OdomPreIntegrator.h:108-147) */
  double dt;                     /* mdeltatij; 0 => no IMU edge */
  double Rij[9];                 /* mRij, row-major */
  double vij[3], pij[3];         /* mvij, mpij */
  double JgR[9], Jgv[9], Jav[9], Jgp[9], Jap[9]; /* bias Jacobians, row-major */
  double Sigma[81];              /* mSigmaij, order (p, v, Phi), row-major */
} vieo_imu_preint;

typedef struct vieo_vio_frame {
  vieo_pose_frame base;     /* current frame: nav = nsj, extrinsics, camera, observations */
  vieo_navstate nav_last;   /* pLastKF->GetNavState() */
  vieo_navstate nav_prior;  /* pLastKF->mNavStatePrior   (used when last_has_prior) */
  double H_prior[225];      /* pLastKF->mMargCovInv, 15x15 row-major, order (p, v, Phi, bg, ba) */
  vieo_imu_preint imu;      /* pFrame->GetIMUPreInt() */
  double gw[3];             /* gravity in the world frame */
  double inv_sigma_bg2, inv_sigma_ba2; /* IMUDataBase::mInvSigmabg2 / mInvSigmaba2 */
  double dt_frames;         /* pFrame->ftimestamp_ - pLastKF->ftimestamp_ (used when imu.dt == 0) */
  float th_depth;           /* pFrame->mThDepth: close points use the 1.5x chi2 gate */
  int32_t last_has_prior;   /* pLastKF->mbPrior: last state is optimised too (30-dim system) */
  int32_t compute_marg;     /* bComputeMarg */
  int32_t no_mps;           /* bNoMPs */
} vieo_vio_frame;

typedef struct vieo_vio_result {
  vieo_pose_result base;   /* nav: p, q, v, dbg, dba updated */
  double H_marg[225];      /* pFrame->mMargCovInv when compute_marg (nav is then mNavStatePrior) */
  int32_t has_marg;        /* pFrame->mbPrior set */
  int32_t reserved;
} vieo_vio_result;

int vieo_pose_optimization_vio(const vieo_vio_frame* h_frame, const vieo_pose_obs* h_obs,
                               uint8_t* h_outlier, vieo_vio_result* h_result);
/* Rig frames (n_cams > 0) of a call with at most 4 frames -- the one-call tracker's case -- are optimised by 16
 * workgroups each: replicas that run the same optimisation and share the passes over the visual edges (thousands per
 * rig frame), exchanging partial sums through device memory; a frame below 700 edges is left to one of them.  The
 * result differs from the one-workgroup form only in the association order of those sums (1e-12 relative on the
 * pose); the status VIEO_E_HIP on a frame means a replica never arrived (never on a healthy device).
 * vieo_pose_set_replicas(0) keeps one workgroup per frame on this host thread (measurements; also the environment
 * variable VIEO_POSE_REPLICAS=0 at start-up), (1) restores the default.  Returns the previous setting. */
int vieo_pose_set_replicas(int on);
/* Capacity: a frame's edges are one bit per edge in a 64-bit mask per lane.  The host entry above always runs the
 * 256-thread instance (16384 observations per frame).  The batched device entry picks its instance from the batch
 * size -- more than 256 non-rig frames per call run one wavefront per frame (4096 observations per frame), smaller
 * batches and rig frames the 256-thread instance (16384) -- and reports a frame beyond the limit through that
 * frame's status (VIEO_E_CAPACITY), not through the return value. */
int vieo_pose_optimization_vio_batch_device(const vieo_vio_frame* d_frames, int n_frames,
                                            const vieo_pose_obs* d_obs, uint8_t* d_outlier,
                                            vieo_vio_result* d_results, void* stream);

/* ---------------------------------------------------------------- local bundle adjustment ---
 * void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int Nlocal)
 * (src/Optimizer.cc:1876-2307), vision-only LBA without encoder edges.  The host shim collects the
 * window exactly as the reference does (:1880-1953) and flattens it:
 *   key frames  : local (free unless nid_ == 0) first, then the fixed observers;
 *   map points  : lLocalMapPoints order; XYZ float32 as stored by MapPoint;
 *   observations: in the reference's edge insertion order = per map point, per observing key frame
 *                 (so a point's edges are contiguous: obs must be sorted by mp).
 * BlockSolver_6_3 semantics: points are marginalised (Schur complement, block_solver.hpp:353-486),
 * LM as in g2o, optimize(its0=5) -> chi2 / depth outlier levels, Huber off -> optimize(its1=10).
 * Outputs: optimised NavStates of the free key frames, float32 points, and h_erase[n_obs] = 1 for
 * the observations the reference puts in vToErase (chi2 > 5.991 / 7.815 or non-positive depth). */
typedef struct vieo_lba_keyframe {
  vieo_navstate nav;
  int32_t fixed;
  int32_t reserved;
} vieo_lba_keyframe;

typedef struct vieo_lba_obs {
  int32_t kf, mp;   /* indices into the key-frame / point arrays */
  float u, v, ur;   /* ur < 0 => monocular edge */
  float inv_sigma2;
} vieo_lba_obs;

typedef struct vieo_lba_params {
  double Rcb[9], tcb[3];
  float fx, fy, cx, cy, bf;
  int32_t its0, its1;     /* 5 and 10 in the reference */
  int32_t n_cams;         /* 0: one rectified pinhole camera = the fields above (Frame::usedistort_ == false);
                           * 1..4: `cams`, and bits 24..27 of vieo_lba_obs.kf select the observation's camera
                           * (get<0>(pKFi->mapn2in_[idx])); distorted observations are monocular (ur < 0) */
  const vieo_camera* cams; /* host pointer, n_cams entries */
} vieo_lba_params;

#define VIEO_LBA_OK 0
#define VIEO_LBA_ABORTED 1       /* *stop was set (Optimizer.cc:2174-2186) */
#define VIEO_LBA_NO_FREE_POSE 2  /* Optimizer.cc:1993 */
typedef struct vieo_lba_result {
  int32_t status;
  int32_t n_erase;
  int32_t lm_iterations;
  int32_t lm_trials;
  double chi2_initial, chi2_final; /* robust chi2 at the first / after the last accepted step */
} vieo_lba_result;

/* Host-pointer entry (synchronous).  `stop` may be NULL; it is polled before the first
 * optimisation, between the two optimisations and between LM iterations. */
int vieo_local_bundle_adjustment(const vieo_lba_params* params, const vieo_lba_keyframe* h_kfs,
                                 int n_kf, const float* h_points, int n_mp,
                                 const vieo_lba_obs* h_obs, int n_obs, volatile const int* stop,
                                 vieo_navstate* h_navs_out, float* h_points_out, uint8_t* h_erase,
                                 vieo_lba_result* h_result);

/* Priority of the calling host thread's bundle-adjustment stream from its next call on: -1 lowest (the default, or
 * VIEO_LBA_PRIORITY: batches of windows beside a batched front end fill what it leaves free), 0 default priority (one
 * window beside a tracker: the LocalMapping thread of a sequential host -- examples/replay_common.hpp -- asks for this;
 * 1.03 against 1.08 ms per frame), 1 highest. */
int vieo_lba_set_stream_priority(int priority);

/* Several independent windows (one per map / per LocalMapping thread of a multi-session server)
 * advanced in lock step: every kernel launch covers all windows and the host reads one small
 * record per window and LM trial.  Each array argument has n_windows entries; per-window results
 * are identical to n_windows calls of vieo_local_bundle_adjustment.  `stop` is shared.
 * A batch advances at the pace of its slowest window: windows of very different size (ordinary windows of ten free key
 * frames and bLarge ones of twenty-five, which take another solve kernel and six Schur tiles instead of one) are better
 * given to separate calls from separate host threads -- 205 such windows: 18.9 ms as one mixed call, 13.6 ms as two. */
int vieo_local_bundle_adjustment_batch(int n_windows, const vieo_lba_params* const* params,
                                       const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                       const float* const* h_points, const int* n_mp,
                                       const vieo_lba_obs* const* h_obs, const int* n_obs,
                                       volatile const int* stop, vieo_navstate* const* h_navs_out,
                                       float* const* h_points_out, uint8_t* const* h_erase,
                                       vieo_lba_result* h_results);

/* ---- LocalBundleAdjustmentNavStatePRV (a18) -----------------------------------------------------
 * void Optimizer::LocalBundleAdjustmentNavStatePRV(KeyFrame*, int Nlocal, bool* pbStopFlag, Map*,
 *   cv::Mat gw, bool bLarge, bool bRecInit, float th_dist_far) (src/Optimizer.cc:21-769), the local BA
 * of the visual-inertial configurations.  Per local key frame three vertices PR (6) + V (3) + Bias (6)
 * (g2otypes.h:287-288,553-567); between consecutive key frames an EdgeNavStatePRV (g2otypes.h:703-884,
 * residual order p, Phi, v) and an EdgeNavStateBias (g2otypes.cpp:14-34); the same EdgeReprojectPR /
 * PRStereo edges and marginalised points as the vision-only LBA; Chi2LargeSetLevel pre-pass
 * (optimizer_ba/g2o_graph_operator.h:23-40); user lambda init; divergence check (:660-666).
 * Key frames: local ones first, oldest to newest (= lLocalKeyFrames order), then the fixed observers;
 * the key frame before the window (pKFPrevLocal) is a fixed one whose full nav state is used.
 * Encoder edges (EdgeEncNavStatePR, g2otypes.h:591-668; Optimizer.cc:323-347): one per pair whose enc.dt != 0. */
typedef struct vieo_lba_imu_edge {
  int32_t kf_i, kf_j;  /* previous / current key frame of the pre-integration (indices) */
  double dt_kf;        /* pKF1->ftimestamp_ - pKF0->ftimestamp_, used when imu.dt == 0 */
  vieo_imu_preint imu; /* GetIMUPreInt() of kf_j; Sigma = mSigmaijPRV, order (p, Phi, v) */
  vieo_enc_preint enc; /* GetEncPreInt() of kf_j */
} vieo_lba_imu_edge;

typedef struct vieo_lba_vio_params {
  vieo_lba_params base;  /* extrinsics, camera, its0 / its1 = optit[0] / optit[1] (4 and 6; 2 and 2 if bLarge) */
  double gw[3];
  double inv_sigma_bg2, inv_sigma_ba2; /* IMUDataBase::mInvSigmabg2 / mInvSigmaba2 */
  double lambda_init;    /* setUserLambdaInit: 1e0, 1e-2 if bLarge (Optimizer.cc:131-138) */
  int32_t rec_init;      /* bRecInit: Huber kernels on the inertial edges of free key frames too */
  int32_t large;         /* bLarge: the divergence check is skipped */
  float th_dist_far;     /* th_dist_far (Optimizer.cc:395,454,513-517): a point none of whose monocular edges sees it
                          * closer than this has all its monocular edges excluded; <= 0 or inf: no such rule */
  int32_t reserved;
  double qRbe[4], pbe[3]; /* Tbe = Frame::mTbc * Frame::mTce: rotation (w, x, y, z) and translation (encoder edges) */
} vieo_lba_vio_params;

#define VIEO_LBA_DIVERGED 3 /* 2*err < err_end or NaN: returns without write-back (Optimizer.cc:660-666) */

/* h_close[n_mp]: 1 where pMP->GetTrackInfoRef().track_depth_ < thresh_depth_close (chi2 gate x1.5 for
 * monocular edges, Optimizer.cc:603-611,677-681).  h_navs_out[k] of a free key frame carries p, q, v,
 * dbg, dba of the optimised vertices (bg, ba unchanged); result.chi2_initial / chi2_final = err / err_end. */
int vieo_local_bundle_adjustment_vio(const vieo_lba_vio_params* params, const vieo_lba_keyframe* h_kfs,
                                     int n_kf, const float* h_points, const uint8_t* h_close, int n_mp,
                                     const vieo_lba_obs* h_obs, int n_obs,
                                     const vieo_lba_imu_edge* h_imu, int n_imu, volatile const int* stop,
                                     vieo_navstate* h_navs_out, float* h_points_out, uint8_t* h_erase,
                                     vieo_lba_result* h_result);

/* several windows in lock step, see vieo_local_bundle_adjustment_batch */
int vieo_local_bundle_adjustment_vio_batch(int n_windows, const vieo_lba_vio_params* const* params,
                                           const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                           const float* const* h_points, const uint8_t* const* h_close,
                                           const int* n_mp, const vieo_lba_obs* const* h_obs, const int* n_obs,
                                           const vieo_lba_imu_edge* const* h_imu, const int* n_imu,
                                           volatile const int* stop, vieo_navstate* const* h_navs_out,
                                           float* const* h_points_out, uint8_t* const* h_erase,
                                           vieo_lba_result* h_results);

/* Encoder edges of the vision-only BAs: EdgeEncNavStatePR (g2otypes.h:591-668) between pKF1->GetPrevKeyFrame() and
 * pKF1 for every pair with GetEncPreInt().mdeltatij != 0 (LocalBundleAdjustment: Optimizer.cc:2008-2042, local key
 * frames only; BundleAdjustment with bEnc: :1401-1438).  Both key frames must be in the window (indices), the edges
 * chain the key frames (at most one into and one out of each).  Information Sigma_E^-1, x 1e-2 when kf_i is fixed;
 * Huber sqrt(12.592) -- always in the local BA (kept through both optimisations), iff `robust` in the full BA. */
typedef struct vieo_lba_enc_edge {
  int32_t kf_i, kf_j;  /* previous / current key frame (indices into the key-frame array) */
  vieo_enc_preint enc; /* GetEncPreInt() of kf_j */
} vieo_lba_enc_edge;   /* 352 bytes */
typedef struct vieo_lba_enc {
  int32_t n_edges, reserved;
  const vieo_lba_enc_edge* edges; /* host pointer */
  double qRbe[4], pbe[3];         /* Tbe = Frame::mTbc * Frame::mTce: rotation (w, x, y, z), translation */
} vieo_lba_enc;                   /* 72 bytes */
/* vieo_local_bundle_adjustment / vieo_bundle_adjustment with those edges; enc == NULL or n_edges == 0: identical to
 * the plain entries. */
int vieo_local_bundle_adjustment_enc(const vieo_lba_params* params, const vieo_lba_keyframe* h_kfs, int n_kf,
                                     const float* h_points, int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                     const vieo_lba_enc* enc, volatile const int* stop, vieo_navstate* h_navs_out,
                                     float* h_points_out, uint8_t* h_erase, vieo_lba_result* h_result);
/* lock-step batch: encs[w] may be NULL (a window without encoder edges); encs itself may be NULL */
int vieo_local_bundle_adjustment_batch_enc(int n_windows, const vieo_lba_params* const* params,
                                           const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                           const float* const* h_points, const int* n_mp,
                                           const vieo_lba_obs* const* h_obs, const int* n_obs,
                                           const vieo_lba_enc* const* encs, volatile const int* stop,
                                           vieo_navstate* const* h_navs_out, float* const* h_points_out,
                                           uint8_t* const* h_erase, vieo_lba_result* h_results);
int vieo_bundle_adjustment_enc(const vieo_lba_params* params, int n_iterations, int robust,
                               const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                               const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_enc* enc,
                               volatile const int* stop, vieo_navstate* h_navs_out, float* h_points_out,
                               vieo_lba_result* h_result);

/* void Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust, bEnc = false)
 * (src/Optimizer.cc:1353-1609; GlobalBundleAdjustment :1346-1351 passes the whole map) and
 * int Optimizer::GlobalBundleAdjustmentNavStatePRV(pMap, gw, nIterations, pbStopFlag, nLoopKF, bRobust,
 * bScaleOpt = false, pimu_initiator = nullptr) (:771-1345) -- "full BA" -- on the flattened layout of the local
 * BAs: every key frame free except the flagged ones (nid_ == 0), ONE optimize(n_iterations) with g2o's own
 * initial lambda, Huber kernels (sqrt(5.99) / sqrt(7.815); sqrt(16.919) / sqrt(12.592) on the inertial / bias
 * edges) on every edge iff `robust`, no outlier classification, every point written back.  The visual-inertial
 * form weighs the inertial and bias edges leaving a fixed key frame by 1e-2 like the reference.  The reduced
 * system is factorised by one of three kernels (lba_solve_device.h) according to its size n (lba.hip solver_class, the
 * same for the local BAs): n <= 159 k_lba_ldlt16 (one workgroup, whole triangle in LDS, blocked on the FP64 matrix
 * cores), n <= 639
 * k_lba_ldltg (one workgroup, left-looking, the factor in L2 as 16 x 16 blocks), beyond that the tiled LDL^T over many
 * workgroups (k_big_*) up to 16320 unknowns (1088 visual-inertial key frames); past that, the same tiled LDL^T over
 * the stored 64 x 64 tiles of the symbolic fill pattern only (tile-sparse, no reordering: the same results as the
 * dense tiled solve; VIEO_LBA_SPARSE_SOLVE=1 selects it at any size), limited by device memory (VIEO_E_CAPACITY with
 * the byte count when it does not fit).  The landmark-sharded entries keep the 16320 limit.
 * params->its0 / its1 (and lambda_init / rec_init / large of the VIO params) are ignored.  Not covered: the gravity
 * vertex of the IMU initialiser (pimu_initiator, SURVEY 2 row 14: out of scope).  bScaleOpt: the _scale entries
 * below.  Encoder edges: vieo_lba_imu_edge.enc in the
 * visual-inertial form, vieo_bundle_adjustment_enc (bEnc = true) in the vision-only one. */
int vieo_bundle_adjustment(const vieo_lba_params* params, int n_iterations, int robust,
                           const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                           const vieo_lba_obs* h_obs, int n_obs, volatile const int* stop, vieo_navstate* h_navs_out,
                           float* h_points_out, vieo_lba_result* h_result);
int vieo_global_bundle_adjustment_vio(const vieo_lba_vio_params* params, int n_iterations, int robust,
                                      const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                                      const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu, int n_imu,
                                      volatile const int* stop, vieo_navstate* h_navs_out, float* h_points_out,
                                      vieo_lba_result* h_result);
/* The full BA as System::FinalGBA runs it (src/System.cc:24-33: bScaleOpt = true; Examples/Stereo/stereo_euroc.cc:334-351
 * "FullBA"), BASELINE configs[4].  scale_opt != 0 adds the VertexScale (src/Odom/g2otypes.h:292-311; estimate 1, id after
 * every key-frame vertex, src/Optimizer.cc:842-851) and turns every visual edge into the three-vertex EdgeReprojectPRS /
 * EdgeReprojectPRSStereo (g2otypes.h:321-541 with MODE_OPT_VAR == 1, typedefs :548-550; Optimizer.cc:1131-1137,
 * 1190-1196): the edge projects s * Xh, the point vertex stays unscaled.  Write-back as the reference's
 * (Optimizer.cc:1256-1335): points = (float)s * (float)Xh, key-frame states unscaled; *h_scale_out (may be NULL) = s.
 * With the scale vertex a map whose key frames are all fixed is still optimised (bdimPoses, :850).
 * scale_opt == 0: identical to vieo_global_bundle_adjustment_vio. */
int vieo_global_bundle_adjustment_vio_scale(const vieo_lba_vio_params* params, int n_iterations, int robust, int scale_opt,
                                            const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points, int n_mp,
                                            const vieo_lba_obs* h_obs, int n_obs, const vieo_lba_imu_edge* h_imu,
                                            int n_imu, volatile const int* stop, vieo_navstate* h_navs_out,
                                            float* h_points_out, vieo_lba_result* h_result, double* h_scale_out);

/* ---- one window over several GPUs ---------------------------------------------------
 * Landmark-sharded LocalBundleAdjustmentNavStatePRV: every rank passes ALL key frames and inertial
 * edges of a window but only ITS share of the points (and their observations).  Per LM trial the ranks
 * exchange exactly one thing, the sum of their visual contributions to the reduced pose system (Schur
 * product, H_pp, b_p), and once more three scalars (chi2 before / after, gain-ratio scale); everything
 * else -- inertial edges, the dense solve, the LM policy -- is replicated and therefore identical on all
 * ranks.  `allreduce(ctx, d_buf, n)` must return 0 after the IN-PLACE sum over all ranks of the n
 * doubles at device pointer d_buf has completed (RCCL: ncclAllReduce(sum, f64) + stream synchronise).
 * d_reduce_buf: device memory of at least vieo_lba_sharded_buffer_doubles(...) doubles.  Key-frame
 * outputs are identical on all ranks, h_points_out / h_erase cover the rank's own points.  No stop flag
 * (the ranks must take the same decisions). */
typedef int (*vieo_allreduce_sum_f64_fn)(void* ctx, double* d_buf, size_t n);
/* In-library RCCL (north_star: "RCCL all-reduce over xGMI on the pose-block Hessian"): librccl.so is loaded with dlopen at
 * first use.  Rank 0 draws the 128-byte unique id, the host carries it to the other ranks (torch.distributed broadcast,
 * MPI, ...), every rank creates its communicator on its own GPU.  Passing allreduce == NULL and ctx == that communicator to
 * the sharded entries makes the library issue ncclAllReduce(sum, f64) itself on its bundle-adjustment stream, between the
 * pack and the assemble kernels, with no host synchronisation in between. */
int vieo_rccl_available(void);
int vieo_rccl_unique_id(uint8_t* id128);
int vieo_rccl_comm_create(void** comm, const uint8_t* id128, int n_ranks, int rank);
int vieo_rccl_comm_destroy(void* comm);
size_t vieo_lba_sharded_buffer_doubles(int n_windows, const int* n_free_kf);

/* Measurement hook of the bundle-adjustment engine (no reference counterpart): with timing on, every kernel launch
 * of the local / full BA entries is bracketed by HIP events on the engine's own stream and folded into process-wide
 * totals per kernel class (vieo_lba_kernel_class_name: "lba.build", "lba.schur", ...).  enable(on) also clears the
 * totals; on == 2 counts the launches (and the Schur FLOPs) per class without recording events, for a timed region
 * that must not carry the events' markers on the stream.  schur_flops: dense FLOPs 2 np (np + 1) 3 n_mp of the windows the timed k_lba_schur launches worked on. */
void vieo_lba_enable_timing(int on);
int vieo_lba_kernel_classes(void);
const char* vieo_lba_kernel_class_name(int i);
void vieo_lba_kernel_times(double* ms /*[classes]*/, long long* launches /*[classes]*/, double* schur_flops);
/* The last full BA of the process that took the tile-sparse solve: stored tiles, tiles of the dense lower triangle
 * (bordered system), planned Schur tiles, upper Schur tiles of the dense grid, bytes of the plan (tile pool, Schur
 * tiles, panel, lists), bytes of the whole device arena. */
void vieo_lba_sparse_stats(long long* out /*[6]*/);
int vieo_local_bundle_adjustment_vio_sharded(int n_windows, const vieo_lba_vio_params* const* params,
                                             const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                             const float* const* h_points, const uint8_t* const* h_close,
                                             const int* n_mp, const vieo_lba_obs* const* h_obs, const int* n_obs,
                                             const vieo_lba_imu_edge* const* h_imu, const int* n_imu,
                                             double* d_reduce_buf, size_t reduce_cap_doubles,
                                             vieo_allreduce_sum_f64_fn allreduce, void* ctx,
                                             vieo_navstate* const* h_navs_out, float* const* h_points_out,
                                             uint8_t* const* h_erase, vieo_lba_result* h_results);
/* The same with pbStopFlag (src/Optimizer.cc:524-528,570-571,590-592): `stop` is this rank's flag (NULL: none).  A sharded
 * run never acts on its own copy: the ranks' requests are summed in the exchanges the run makes anyway (the agreement at
 * entry, the spare fourth scalar of every trial's exchange), so a flag raised on ONE rank aborts the call on ALL ranks at
 * the same trial -- nobody is left waiting in a collective. */
int vieo_local_bundle_adjustment_vio_sharded_stop(int n_windows, const vieo_lba_vio_params* const* params,
                                                  const vieo_lba_keyframe* const* h_kfs, const int* n_kf,
                                                  const float* const* h_points, const uint8_t* const* h_close,
                                                  const int* n_mp, const vieo_lba_obs* const* h_obs, const int* n_obs,
                                                  const vieo_lba_imu_edge* const* h_imu, const int* n_imu,
                                                  double* d_reduce_buf, size_t reduce_cap_doubles,
                                                  vieo_allreduce_sum_f64_fn allreduce, void* ctx, volatile const int* stop,
                                                  vieo_navstate* const* h_navs_out, float* const* h_points_out,
                                                  uint8_t* const* h_erase, vieo_lba_result* h_results);
/* The same exchange for the full BA (BASELINE configs[4]: "full BA with RCCL pose-Hessian all-reduce"): this rank's
 * landmark shard of GlobalBundleAdjustmentNavStatePRV; per LM trial one all-reduce of the packed reduced visual
 * system ((6n)(6n+1) + 42n doubles for n free key frames) and one of three scalars. */
int vieo_global_bundle_adjustment_vio_sharded(const vieo_lba_vio_params* params, int n_iterations, int robust,
                                              const vieo_lba_keyframe* h_kfs, int n_kf, const float* h_points,
                                              int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                              const vieo_lba_imu_edge* h_imu, int n_imu, double* d_reduce_buf,
                                              size_t reduce_cap_doubles, vieo_allreduce_sum_f64_fn allreduce,
                                              void* ctx, vieo_navstate* h_navs_out, float* h_points_out,
                                              vieo_lba_result* h_result);
/* ... and of System::FinalGBA's form (scale_opt, see vieo_global_bundle_adjustment_vio_scale): the scale vertex's row of
 * the reduced visual system and its H_ps / H_ss / b_s travel in the same all-reduce ((6n+1)(6n+2) + 48n + 2 doubles). */
int vieo_global_bundle_adjustment_vio_sharded_scale(const vieo_lba_vio_params* params, int n_iterations, int robust,
                                                    int scale_opt, const vieo_lba_keyframe* h_kfs, int n_kf,
                                                    const float* h_points, int n_mp, const vieo_lba_obs* h_obs, int n_obs,
                                                    const vieo_lba_imu_edge* h_imu, int n_imu, double* d_reduce_buf,
                                                    size_t reduce_cap_doubles, vieo_allreduce_sum_f64_fn allreduce,
                                                    void* ctx, vieo_navstate* h_navs_out, float* h_points_out,
                                                    vieo_lba_result* h_result, double* h_scale_out);

/* ---- replay glue (device-resident batches) -------------------------------------------------
 * What Tracking.cc does between the calls above, on flattened arrays, so a batch of frames runs
 * extract -> stereo -> search -> pose optimisation with no host round trip (bench.py):
 * keypoint -> point bookkeeping (Frame::mvpMapPoints), the observation gathering at the top of
 * PoseOptimization (Optimizer.cc:1704-1786), "Discard outliers" (Tracking.cc:1903-1921).
 * d_mp_ref[f][key_cap]: index into frame f's point table d_point_xyz[f][p_cap][3], -1 = none. */
int vieo_track_merge_assign_batch_device(const int32_t* d_assign, int32_t* d_mp_ref,
                                         const int32_t* d_counts, int key_cap, int n_frames,
                                         int img_first, int img_step, int point_offset, int reset,
                                         void* stream);
/* Fills d_obs[f][key_cap] / d_obs_key and writes n_obs, obs_begin (= f*key_cap) into the frame
 * structs (vieo_pose_frame or vieo_vio_frame array). */
int vieo_track_build_obs_batch_device(const int32_t* d_mp_ref, const float* d_point_xyz, int p_cap,
                                      const vieo_keypoint* d_keys, const float* d_uright,
                                      const int32_t* d_counts, int key_cap, int n_frames,
                                      int img_first, int img_step, const float* d_inv_sigma2,
                                      vieo_pose_obs* d_obs, int32_t* d_obs_key, void* d_frames,
                                      int frames_are_vio, void* stream);
/* Drops outlier matches from d_mp_ref, exports d_taken (may be NULL) for the next search and
 * copies the optimised NavState into d_next_frames[f].nav (may be NULL). */
int vieo_track_after_pose_batch_device(int32_t* d_mp_ref, const int32_t* d_obs_key,
                                       const uint8_t* d_outlier, const void* d_frames,
                                       const void* d_results, int frames_are_vio, int key_cap,
                                       int n_frames, void* d_next_frames, uint8_t* d_taken,
                                       void* stream);
/* ... and vieo_track_mark_held_batch_device (below) in the same launch: d_held[f][p_cap] from the entries left. */
int vieo_track_after_pose_held_batch_device(int32_t* d_mp_ref, const int32_t* d_obs_key, const uint8_t* d_outlier,
                                            const void* d_frames, const void* d_results, int frames_are_vio, int key_cap,
                                            int n_frames, void* d_next_frames, uint8_t* d_taken, const int32_t* d_counts,
                                            int img_first, int img_step, uint8_t* d_held, int p_cap, void* stream);
/* vieo_track_merge_assign[_rig]_batch_device + vieo_track_build_obs[_depth | _rig]_batch_device as ONE launch (the one-call
 * tracker's chain is a launch shorter per search): the assignment is merged into d_mp_ref key by key and the observations
 * are gathered from the merged entries.  d_same_point / d_query_src / d_point_depth / d_cam_first may be NULL (the plain
 * forms); same outputs as the two calls. */
int vieo_track_merge_build_obs_batch_device(const int32_t* d_assign, int32_t* d_mp_ref, int point_offset, int reset, int query_div,
                                            const vieo_last_frame_point* d_same_point, const int32_t* d_query_src, int q_cap,
                                            const float* d_point_xyz, const float* d_point_depth, float close_depth, int p_cap,
                                            const vieo_keypoint* d_keys, const float* d_uright, const int32_t* d_counts,
                                            const int32_t* d_cam_first, int n_cams, int key_cap, int n_frames, int img_first,
                                            int img_step, const float* d_inv_sigma2, vieo_pose_obs* d_obs, int32_t* d_obs_key,
                                            void* d_frames, int frames_are_vio, void* stream);
/* The same with the `close` bit of the observations (vieo_pose_obs.flags bit 0) taken from the depth at which the
 * point was tracked: d_point_depth[f][p_cap] < close_depth (Frame::mvpMapPoints[i]->mTrackDepth against
 * max(10, ThDepth), the stereo chi2 gate of the visual-inertial PoseOptimization, include/Optimizer.h:406-490). */
int vieo_track_build_obs_depth_batch_device(const int32_t* d_mp_ref, const float* d_point_xyz,
                                            const float* d_point_depth, float close_depth, int p_cap,
                                            const vieo_keypoint* d_keys, const float* d_uright,
                                            const int32_t* d_counts, int key_cap, int n_frames,
                                            int img_first, int img_step, const float* d_inv_sigma2,
                                            vieo_pose_obs* d_obs, int32_t* d_obs_key, void* d_frames,
                                            int frames_are_vio, void* stream);
/* The two glue steps for camera-rig frames: a search's query (point i, camera c) is i * query_div + c (query_div =
 * n_cams), and an observation carries its key's camera in bits 8..11 of vieo_pose_obs.flags (mapn2in_,
 * include/Optimizer.h:424-426) -- the camera found from d_cam_first [f][n_cams + 1]; keys [f][key_cap] camera-major,
 * d_counts [f][2] = {N, -} (d_frame_counts of vieo_stereo_fisheye_match_batch_device); d_point_depth may be NULL. */
int vieo_track_merge_assign_rig_batch_device(const int32_t* d_assign, int32_t* d_mp_ref, const int32_t* d_counts,
                                             int key_cap, int n_frames, int img_first, int img_step, int point_offset,
                                             int reset, int query_div,
                                             const vieo_last_frame_point* d_same_point /*[f][key_cap] or NULL: reserved[0]
                                             > 0 names (1 +) the first point-table entry of the same MapPoint*/,
                                             const int32_t* d_query_src /*[f][q_cap] or NULL: the searched list was
                                             compacted, entry a came from query d_query_src[a]*/, int q_cap, void* stream);
/* The valid queries (flags bit 0) of every frame moved to the front of d_queries_out in their order, d_src[f][k] = the
 * index the k-th one had, d_nq_out[f] = their number.  A rig frame's first search holds one query per (last-frame key,
 * camera) pair and most of them project outside their camera; the search walks the list several times. */
int vieo_track_compact_queries_batch_device(const vieo_proj_query* d_queries, const int32_t* d_nq, int q_cap, int n_frames,
                                            vieo_proj_query* d_queries_out, int32_t* d_src, int32_t* d_nq_out, void* stream);
int vieo_track_build_obs_rig_batch_device(const int32_t* d_mp_ref, const float* d_point_xyz,
                                          const float* d_point_depth, float close_depth, int p_cap,
                                          const vieo_keypoint* d_keys, const float* d_uright,
                                          const int32_t* d_counts, const int32_t* d_cam_first, int n_cams, int key_cap,
                                          int n_frames, const float* d_inv_sigma2, vieo_pose_obs* d_obs,
                                          int32_t* d_obs_key, void* d_frames, int frames_are_vio, void* stream);
/* d_held[f][p_cap] = 1 for the entries of frame f's point table that a key holds (the points
 * Tracking::SearchLocalPoints takes out of the local-map search, src/Tracking.cc:2318-2334). */
int vieo_track_mark_held_batch_device(const int32_t* d_mp_ref, const int32_t* d_counts, int key_cap,
                                      int n_frames, int img_first, int img_step, uint8_t* d_held, int p_cap,
                                      void* stream);
/* The extractor's own hipStream_t, so the calls above can be chained on it. */
void* vieo_orb_stream(vieo_orb* e);

/* ---- test taps (parity tests only; not part of the drop-in surface) ---- */
/* which: 1 = blurred level.  FAST candidates: int32 triplets (x, y, response) in
 * vToDistributeKeys order; level keys: vieo_keypoint in DistributeOctTree output order. */
int vieo_orb_tap_plane(vieo_orb* e, int image_index, int level, int which, uint8_t* h_dst,
                       int dst_stride);
int vieo_orb_tap_candidates(vieo_orb* e, int image_index, int level, int32_t* h_dst, int cap);
int vieo_orb_tap_level_keys(vieo_orb* e, int image_index, int level, vieo_keypoint* h_dst,
                            int cap);

/* ---------------------------------------------------------------- map-point side --------------
 * The per-point steps either side of SearchByProjection(local map) and of the local BA write-back. */

/* bool Frame::isInFrustum(MapPoint* pMP, float viewingCosLimit) (src/Frame.cc:335-416) for a batch of points:
 * per camera positive depth, image bounds, distance inside [0.8 mfMinDistance, 1.2 mfMaxDistance], viewing
 * cosine against the mean normal, MapPoint::PredictScale (src/MapPoint.cc:491-509).  All float, as the
 * reference computes it; Sophus SE3f products are taken through their 3x4 matrices. */
typedef struct vieo_frustum_frame {
  float Rcrw[9], tcrw[3]; /* Tcw_ rotation (row-major) and mtcw, cast to float (Frame.cc:348-351) */
  float Ow[3];            /* mOw */
  int32_t n_cams;         /* 1..4 */
  int32_t use_distort;    /* Frame::usedistort_: 0 -> K * (x/z, y/z, 1) in float, 1 -> camera Project() */
  const struct vieo_camera* cams; /* host pointer, n_cams entries (Rcb / tcb unused) */
  float Tcr[4][12];       /* mpCameras[i]->GetTcr().matrix3x4() row-major (identity for camera 0) */
  float trc[4][3];        /* mpCameras[i]->GetTrc().translation() */
  float bounds[4][4];     /* gridinfo_.minmax_xy_[i] = {min_x, max_x, min_y, max_y} */
  float bf;               /* stereoinfo_.baseline_bf_[1] */
  float log_scale_factor; /* scalepyrinfo_.flogscalefactor_ */
  int32_t n_levels;
  float viewing_cos_limit;
} vieo_frustum_frame;

typedef struct vieo_frustum_point {
  float Xw[3], normal[3];           /* GetWorldPos(), GetNormal() */
  float max_distance, min_distance; /* mfMaxDistance, mfMinDistance (the 1.2 / 0.8 factors are applied here) */
} vieo_frustum_point;               /* 32 bytes */

typedef struct vieo_track_info {    /* MapPoint::_TrackFastMatchInfo after the call */
  float u[4], v[4], ur[4], viewcos[4]; /* vtrack_proj_[0..2], vtrack_viewcos_ (entries 0..n-1, push order) */
  int32_t level[4], cam[4];         /* vtrack_scalelevel_, vtrack_cami_ */
  int32_t n;                        /* cameras that see the point; btrack_inview_ = n > 0 */
  float track_depth;                /* mean dist3D over those cameras; -1 when n == 0 (the member keeps its value) */
} vieo_track_info;                  /* 104 bytes */

int vieo_is_in_frustum_batch(const vieo_frustum_frame* h_frame, const vieo_frustum_point* h_points, int n_points,
                             vieo_track_info* h_info);
/* The head of Tracking::SearchLocalPoints (src/Tracking.cc:2308-2370) for ONE frame whose pose is still in HBM, so
 * that TrackWithIMU -> TrackLocalMapWithIMU runs as one chain of launches (no host round trip between the first
 * PoseOptimization and the local-map search): the pose is d_result->base.nav when d_result->base.status == 0, else
 * d_frame->base.nav, with d_frame->base.Rcb / tcb (h_frame's Rcrw / tcrw / Ow are ignored, the rest of h_frame is used
 * as in vieo_is_in_frustum_batch); isInFrustum of the n_points candidates; their window queries in the order of
 * SearchByProjection(Frame&, vector<MapPoint*>&, th, th_far) (src/ORBmatcher.cc:237-266): d_queries[p * n_cams + k]
 * is the k-th camera that sees candidate p (flags = 0 in the unused slots), *d_nq = n_points * n_cams.
 * d_alias[p] >= 0 (may be NULL): candidate p is the same map point as entry d_alias[p] of the frame's point table;
 * it gets no query when d_held[d_alias[p]] != 0 (vieo_track_mark_held_batch_device; d_held has held_cap entries,
 * larger indices count as not held).  d_track_depth[p] = mTrackDepth
 * (-1 when no camera sees the point).  d_scale: scalepyrinfo_.vscalefactor_ (n_levels floats). */
int vieo_track_local_queries_device(const vieo_frustum_frame* h_frame, const vieo_vio_frame* d_frame,
                                    const vieo_vio_result* d_result, const vieo_frustum_point* d_points,
                                    const uint8_t* d_desc, const int32_t* d_alias, const uint8_t* d_held, int held_cap,
                                    int n_points, float th, float th_far, const float* d_scale, vieo_proj_query* d_queries,
                                    float* d_track_depth, int32_t* d_nq, void* stream);

/* The same for a batch of frames (bench.py's batched step): frame f reads d_frames[f] / d_results[f], its candidates
 * d_points / d_desc / d_alias [f][p_cap] (d_counts[f] of them), d_held [f][held_cap]; writes d_queries [f][p_cap * n_cams],
 * d_track_depth + f * depth_stride, d_nq[f] = d_counts[f] * n_cams. */
int vieo_track_local_queries_batch_device(const vieo_frustum_frame* h_frame, const vieo_vio_frame* d_frames,
                                          const vieo_vio_result* d_results, int n_frames, const vieo_frustum_point* d_points,
                                          const uint8_t* d_desc, const int32_t* d_alias, const int32_t* d_counts, int p_cap,
                                          const uint8_t* d_held, int held_cap, float th, float th_far, const float* d_scale,
                                          vieo_proj_query* d_queries, float* d_track_depth, size_t depth_stride,
                                          int32_t* d_nq, void* stream);
/* The same for frames of several live sequences (vieo_track_frames): frame f's candidates are in the table of its
 * sequence's slot, d_points / d_desc [d_pos_slot[f]][p_cap]; d_alias [f][p_cap], d_counts[f], d_held [f][held_cap],
 * d_queries, d_track_depth and d_nq as above.  d_frames / d_results hold vieo_vio_frame / vieo_vio_result records, or
 * vieo_pose_frame / vieo_pose_result ones (vision-only), frame_stride / result_stride bytes apart. */
int vieo_track_local_queries_slot_batch_device(const vieo_frustum_frame* h_frame, const void* d_frames, size_t frame_stride,
                                               const void* d_results, size_t result_stride, int n_frames,
                                               const int32_t* d_pos_slot, const vieo_frustum_point* d_points,
                                               const uint8_t* d_desc, const int32_t* d_alias, const int32_t* d_counts,
                                               int p_cap, const uint8_t* d_held, int held_cap, float th, float th_far,
                                               const float* d_scale, vieo_proj_query* d_queries, float* d_track_depth,
                                               size_t depth_stride, int32_t* d_nq, void* stream);

/* void MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cc:314-378) for a batch of points: point p owns
 * the descriptor rows [h_first[p], h_first[p + 1]) of h_descriptors (its observations in map order); h_best[p]
 * receives the row (relative to h_first[p]) with the least median Hamming distance to the others, first such
 * row on ties; -1 for a point without observations.  At most 128 observations per point. */
int vieo_distinctive_descriptors_batch(const uint8_t* h_descriptors, const int32_t* h_first, int n_points,
                                       int32_t* h_best);

/* void MapPoint::UpdateNormalAndDepth() (src/MapPoint.cc:424-480) for a batch of points: observation i of point
 * p looks from the camera centre h_centres[h_obs_centre[i]] (twc of the (key frame, camera) pair, float[3]);
 * outputs the mean viewing direction and mfMaxDistance / mfMinDistance from the reference key frame
 * (h_ref_centre[p] index into h_centres, h_ref_scale[p] = vscalefactor_[octave of the key in it]). */
int vieo_update_normal_and_depth_batch(const float* h_points /*[n][3]*/, const int32_t* h_first,
                                       const int32_t* h_obs_centre, const float* h_centres, int n_centres,
                                       const int32_t* h_ref_centre, const float* h_ref_scale,
                                       float scale_last_level, int n_points, float* h_normal /*[n][3]*/,
                                       float* h_max_distance, float* h_min_distance);

/* The search of ORBmatcher::SearchByProjectionBase (src/ORBmatcher.cc:26-227) -- what ORBmatcher::Fuse (:1152-1165,
 * LocalMapping::SearchInNeighbors) and the Sim3 / loop-closing callers run per map point: projection into every
 * camera of the key frame (positive depth, FrameBase::IsInImage, scale-invariance distances, optional 60 degree
 * viewing cone), MapPoint::PredictScale, FrameBase::GetFeaturesInArea (FrameBase.cpp:95-141) with radius
 * th_radius * scale[level], octave in [level-1, level], the chi2 gate on the reprojection error (7.8 stereo /
 * 5.99 mono, only when use_bf), best Hamming distance (first minimum in the reference's candidate order).
 * Per (point, camera): h_best_idx (index into that camera's keys, -1: none) and h_best_dist.  The thresholds on
 * the distance, KeyFrame::FuseMP and the only-one-match bookkeeping (:195-224) stay with the caller: they are
 * order-dependent mutations of the map.  A point whose skip_mask has bit 31 set is not searched at all
 * (isBad / IsInKeyFrame), bit c skips camera c (pvbAlreadyMatched1). */
typedef struct vieo_fuse_frame {
  vieo_frustum_frame base;     /* Rcrw, tcrw, Ow = GetCameraCenter(), cameras, bounds, bf, log scale factor, n_levels */
  float scale_factors[16];     /* scalepyrinfo_.vscalefactor_ */
  float inv_level_sigma2[16];  /* scalepyrinfo_.vinvlevelsigma2_ */
  float th_radius;
  int32_t check_viewing_angle; /* bCheckViewingAngle */
  int32_t use_bf;              /* pbf != nullptr: chi2 gate with the stereo coordinate */
  int32_t reserved;
} vieo_fuse_frame;

typedef struct vieo_fuse_point {
  float Xw[3], normal[3];
  float max_distance, min_distance; /* mfMaxDistance, mfMinDistance */
  uint8_t desc[32];                 /* GetDescriptor() */
  int32_t skip_mask;
  int32_t reserved;
} vieo_fuse_point;                  /* 72 bytes */

int vieo_fuse_search(const vieo_fuse_frame* h_frame, const vieo_keypoint* const* h_keys /*[n_cams]*/,
                     const float* const* h_uright /*[n_cams], may be NULL entries: all monocular*/,
                     const uint8_t* const* h_descriptors /*[n_cams]*/, const int32_t* n_keys /*[n_cams]*/,
                     const vieo_fuse_point* h_points, int n_points, int32_t* h_best_idx /*[n_points][n_cams]*/,
                     int32_t* h_best_dist /*[n_points][n_cams]*/);

/* ---------------------------------------------------------------- IMU pre-integration ----------
 * int IMUPreIntegratorBase::PreIntegration(timeStampi, timeStampj, bgi_bar, bai_bar, iterBegin, iterEnd, breset =
 * true) + update() (src/Odom/OdomPreIntegrator.h:226-506; mid-point samples, the partial intervals at both ends
 * interpolated as the reference does, USE_PREINT_EULA off) for a batch of intervals, one lane per interval:
 * delta R / v / p, the five bias Jacobians, Sigma in both orders (mSigmaij: p v Phi; mSigmaijPRV: p Phi v).
 * Interval k owns the samples [h_first[k], h_first[k + 1]) (time-ordered).  h_ti[k] > h_tj[k] is the reference's
 * backward order (map reuse, :241-262): the samples are walked from the end with negative steps.  h_status[k]: */
#define VIEO_PREINT_OK 0
#define VIEO_PREINT_EMPTY 1       /* no samples: PreIntegration() does nothing (outputs zeroed, dt = 0; the seed, see _ex) */
#define VIEO_PREINT_GAP 2         /* |dt| > 1.5 s between samples: "CheckIMU", mdeltatij = 0, returns -1 */
#define VIEO_PREINT_UNSUPPORTED 3 /* (not returned any more: the backward order of map reuse, timeStampi > timeStampj, is built) */
typedef struct vieo_imu_sample {
  double t;            /* IMUData::mtm */
  double w[3], a[3];   /* mw, ma */
} vieo_imu_sample;     /* 56 bytes */
typedef struct vieo_imu_noise {
  double sigma_g[9], sigma_a[9]; /* IMUDataBase::mSigmag, mSigmaa (row-major) */
  double freq_ref;               /* IMUDataBase::mFreqRef */
  int32_t dt_cov_noise_fixed;    /* IMUDataBase::mdt_cov_noise_fixed */
  int32_t reserved;
} vieo_imu_noise;
int vieo_imu_preintegrate_batch(const vieo_imu_noise* noise, const vieo_imu_sample* h_samples,
                                const int32_t* h_first, const double* h_ti, const double* h_tj,
                                const double* h_bg /*[n][3]*/, const double* h_ba /*[n][3]*/, int n,
                                vieo_imu_preint* h_out, double* h_sigma_prv /*[n][81], may be NULL*/,
                                int32_t* h_status);

/* Device form of the same call (the chained frame below runs it on its own stream next to the extraction): every
 * array in HBM, asynchronous on `stream`; n < 1024 intervals get a wavefront each. */
int vieo_imu_preintegrate_batch_device(const vieo_imu_noise* d_noise, const vieo_imu_sample* d_samples,
                                       const int32_t* d_first, const double* d_ti, const double* d_tj,
                                       const double* d_bg, const double* d_ba, int n, vieo_imu_preint* d_out,
                                       double* d_sigma_prv, int32_t* d_status, void* stream);

/* PreIntegration(..., breset) per interval: where h_breset[k] == 0, reset() is skipped and update() continues from
 * h_seed[k] (mdeltatij, mRij, mvij, mpij, the bias Jacobians, mSigmaij) and h_seed_sigma_prv[k] (mSigmaijPRV, [81]);
 * an empty list then returns the seed unchanged (status VIEO_PREINT_EMPTY), a gap dt = 0 with the members advanced up
 * to it (VIEO_PREINT_GAP).  h_seed == NULL: every interval resets (h_seed_sigma_prv and h_breset are then ignored), the
 * same bytes as vieo_imu_preintegrate_batch; otherwise all three are required.  h_out may be the same array as h_seed
 * and h_sigma_prv the same as h_seed_sigma_prv (the seeds are read before anything is written). */
int vieo_imu_preintegrate_batch_ex(const vieo_imu_noise* noise, const vieo_imu_sample* h_samples,
                                   const int32_t* h_first, const double* h_ti, const double* h_tj,
                                   const double* h_bg /*[n][3]*/, const double* h_ba /*[n][3]*/, int n,
                                   const vieo_imu_preint* h_seed /*[n], may be NULL*/,
                                   const double* h_seed_sigma_prv /*[n][81]*/, const int32_t* h_breset /*[n]*/,
                                   vieo_imu_preint* h_out, double* h_sigma_prv /*[n][81], may be NULL*/,
                                   int32_t* h_status);
/* Device form: as above, every array in HBM; d_out / d_sigma_prv must not overlap d_seed / d_seed_sigma_prv. */
int vieo_imu_preintegrate_batch_device_ex(const vieo_imu_noise* d_noise, const vieo_imu_sample* d_samples,
                                          const int32_t* d_first, const double* d_ti, const double* d_tj,
                                          const double* d_bg, const double* d_ba, int n,
                                          const vieo_imu_preint* d_seed, const double* d_seed_sigma_prv,
                                          const int32_t* d_breset, vieo_imu_preint* d_out, double* d_sigma_prv,
                                          int32_t* d_status, void* stream);

/* ---------------------------------------------------------------- IMU initialisation -------------------------
 * bool IMUInitialization::TryInitVIO() (src/Odom/IMUInitialization.cpp:1068-1480, USE_FAST_IMU_INIT undefined) for a
 * batch of sequences in one call: ONE copy up, one chain of launches (k_imu_init_gyro -> pre-integration ->
 * k_imu_init_solve -> pre-integration -> k_imu_init_apply; one more pre-integration in front when h_preint == NULL),
 * ONE copy back, ONE host synchronisation.  FP64 throughout, from inputs the caller widens (the reference runs steps
 * 3-5 on CV_32F matrices with OpenCV's float SVD).
 *   1. Optimizer::OptimizeInitialGyroBias (include/Optimizer.h:820-892, EdgeGyrBias src/Odom/g2otypes.h:940-973): one
 *      Gauss-Newton step from bg = 0 over the key frames 1 .. n_kf_init - 1 whose stored pre-integration has dt != 0,
 *      information = inverse of the Phi block of mSigmaijPRV.  No edge, or a 3 x 3 system that is not positive
 *      definite (g2o's solver fails and leaves the estimate): bg* = 0.
 *   2. every interval re-integrated with (bg*, 0).
 *   3. [lambda | beta I3] x = gamma (:1154-1225), x = (s*, gw*), by a one-sided Jacobi SVD; a triple with an interval of
 *      dt == 0 leaves three zero rows and is not counted in n_eq.
 *   4. RwI from gw*, [lambda | phi(:, 0:2) | zeta] y = psi (:1246-1314), y = (s, dtheta_x, dtheta_y, ba).
 *      Both solves: x = V diag(1 / w) U^T B with |w_k| < 1e-10 raised by 1e-10; w and w2 come back sorted descending.
 *   5. when `apply` is set (the caller's mdFinalTime gate, :1347) and the status is OK: every key frame of the list at
 *      the update (n_kf >= n_kf_init) gets its scaled Tcw and its NavState, every interval is re-integrated with
 *      (bg*, ba*), every point is scaled by (float)s (:1393-1459, MapPoint::UpdateScale).  A key frame whose relevant
 *      interval has dt == 0 (its successor's; the last key frame's own) hits the reference's `continue`: its Tcw is
 *      scaled, its NavState is not set (nav_set = 0, the record zero).
 * Key frame i of a sequence sits at kf_first + i of every per-key-frame array; its interval is (i - 1) -> i, so the
 * entry of key frame 0 is an interval without samples (h_first[k + 1] == h_first[k]; h_preint[k] is not read).  The
 * sample lists are those of vieo_imu_preintegrate_batch.
 * Limits: n_seq 1 .. VIEO_IMU_INIT_MAX_SEQ; n_kf 1 .. VIEO_IMU_INIT_MAX_KF (the 3 (n_kf_init - 2) x 7 rows of a
 * sequence live in the 160 KiB of LDS of one workgroup: 85 680 bytes at the cap); beyond either: VIEO_E_INVALID, as
 * for a null pointer, n_kf_init outside 0 .. n_kf, a range outside the flat arrays or a descending h_first -- before
 * anything is written or launched.  A sequence whose status is not OK never changes the return value and never
 * disturbs the other sequences of the batch. */
#define VIEO_IMU_INIT_MAX_KF 512
#define VIEO_IMU_INIT_MAX_SEQ 256
#define VIEO_IMU_INIT_MAX_SWEEPS 30 /* Jacobi sweeps per solve (a sweep in which no pair rotates ends it earlier) */
#define VIEO_IMU_INIT_OK 0
#define VIEO_IMU_INIT_FEW_KF 1        /* n_kf_init < 4 (:1072); nothing is computed */
#define VIEO_IMU_INIT_FEW_EQUATIONS 2 /* fewer than 4 valid triples (:1198); bg and n_eq_gyro are set */
/* |gw*| == 0 or |gI x gwn| == 0 (gwn = gw* over its norm): TryInitVIO divides by zero here. A deliberate departure from the reference: the
 * guard is InitIMU's (:712-719).  Everything up to gw* and w is set. */
#define VIEO_IMU_INIT_DEGENERATE_GRAVITY 3
typedef struct vieo_imu_init_seq {
  int32_t n_kf;        /* the key frames at the update (GetAllKeyFrames() after the gate), in time order */
  int32_t n_kf_init;   /* <= n_kf: the snapshot steps 1-4 work on */
  int32_t kf_first;    /* key frame 0 in the per-key-frame arrays */
  int32_t point_first, n_points; /* the sequence's points in h_points */
  int32_t apply;       /* timestamp - mdStartTime >= mdFinalTime */
  double Rcb[9], pcb[3]; /* from Frame::mTbc: Rcb = Rbc^T, pcb = -Rcb pbc */
  double ref_g;        /* IMUData::mdRefG (9.810) */
} vieo_imu_init_seq;
typedef struct vieo_imu_init_point {
  float pos[3];        /* mWorldPos */
  float max_dist, min_dist; /* mfMaxDistance, mfMinDistance */
} vieo_imu_init_point;
typedef struct vieo_imu_init_result {
  int32_t status;      /* VIEO_IMU_INIT_* */
  int32_t n_eq_gyro;   /* edges of step 1 */
  int32_t n_eq;        /* numEquations of step 3 */
  int32_t inited;      /* status == OK && apply: step 5 ran */
  int32_t sweeps[2];   /* Jacobi sweeps of the two solves */
  double bg[3];        /* bg* */
  double s_star, gw_star[3], w[4], RwI[9];
  double s, dtheta[2], ba[3], w2[6], RwI_opt[9], gw[3]; /* RwI_opt = RwI Exp((dtheta, 0)), gw = RwI_opt gI G */
} vieo_imu_init_result;
#ifdef __cplusplus
static_assert(sizeof(vieo_imu_init_seq) == 128 && sizeof(vieo_imu_init_point) == 20 && sizeof(vieo_imu_init_result) == 376,
              "vieo_imu_init");
#else
_Static_assert(sizeof(vieo_imu_init_seq) == 128 && sizeof(vieo_imu_init_point) == 20 && sizeof(vieo_imu_init_result) == 376,
               "vieo_imu_init");
#endif
/* h_Twc[n][12]: rows of (Rwc | pwc), the CV_32F mTwc widened; h_t[n]: the key frames' timestamps; n = total_kf.
 * h_first[total_kf + 1] / h_samples: the interval lists.  h_preint / h_preint_sigma_prv[n][81]: the key frames' stored
 * pre-integrations (step 1 reads mRij, mJgRij, mdeltatij and mSigmaijPRV), both NULL: they are integrated here with zero
 * bias.  h_points[total_points] may be NULL when total_points == 0.
 * Outputs: h_results[n_seq]; per key frame h_Tcw_out[n][12] (Rcw | s tcw), h_nav_out[n], h_nav_set[n],
 * h_preint_out[n] + h_sigma_prv_out[n][81] (the intervals re-integrated with (bg*, ba*): the bytes
 * vieo_imu_preintegrate_batch returns for those biases); h_points_out[total_points].  Where step 5 did not run (apply ==
 * 0 or a status other than OK) every per-key-frame and per-point output of the sequence is zero. */
int vieo_imu_init(const vieo_imu_init_seq* seqs, int n_seq, int total_kf, const double* h_Twc, const double* h_t,
                  const vieo_imu_noise* noise, const vieo_imu_sample* h_samples, const int32_t* h_first,
                  const vieo_imu_preint* h_preint, const double* h_preint_sigma_prv,
                  const vieo_imu_init_point* h_points, int total_points, vieo_imu_init_result* h_results,
                  double* h_Tcw_out, vieo_navstate* h_nav_out, int32_t* h_nav_set, vieo_imu_preint* h_preint_out,
                  double* h_sigma_prv_out, vieo_imu_init_point* h_points_out);

/* ---------------------------------------------------------------- one frame's tracking as ONE call -----------
 * What Tracking::Track does for a stereo-inertial frame in the steady state -- Frame::Frame (ExtractORB x 2,
 * src/Frame.cc:259-320; ComputeStereoMatches :451-611), PreIntegration + PredictNavStateByIMU (src/Tracking.cc:385-451),
 * TrackWithIMU (:261-378: SearchByProjection(last frame) -> PoseOptimization), TrackLocalMapWithIMU (:453-488:
 * SearchLocalPoints :2308-2370 -> PoseOptimization(bComputeMarg)) -- as one chain of launches on one stream: ONE copy
 * up from pinned memory (two when the local map changed), the kernels of the entries above back to back with the
 * bookkeeping between them on the device (vieo_track_* glue), the IMU pre-integration on a second stream beside the
 * extraction, ONE copy back, ONE host synchronisation.  The caller keeps the reference's object graph (Frame /
 * KeyFrame / MapPoint / Map) and hands over flattened views of what the calls read; outputs point into pinned memory
 * owned by the tracker and stay valid until its next call.  Thread model: one tracker per tracking thread; other
 * threads (LocalMapping, LoopClosing) call the other entries concurrently on their own streams.
 * Three kinds of tracker (round 4): rectified stereo + IMU (BASELINE configs[1] / [2]; vieo_tracker_create); a distorted
 * camera rig of 2..4 cameras + IMU (the reference's default EuRoC_VIO_dist* set-up, configs[3] / [4];
 * vieo_tracker_create_rig): ExtractORB x n_cams with the KB8 lapping area, Frame::ComputeStereoFishEyeMatches
 * (Frame.cc:613-779) instead of the rectified matcher, the camera loop in both searches, the rig instances of the
 * optimiser; and rectified stereo WITHOUT the IMU (configs[0]; params.vision_only): Tracking::TrackWithMotionModel
 * (Tracking.cc:1844-1928) + TrackLocalMap (:1930-1945) with Optimizer::PoseOptimization(Frame*, Frame*)
 * (Optimizer.cc:1611-1874); the predicted pose (mVelocity * mLastFrame.Tcw, a 4x4 product) is the caller's. */
typedef struct vieo_tracker vieo_tracker;
typedef struct vieo_tracker_params {
  int32_t width, height;                /* image size; both cameras */
  int32_t n_features, n_levels, ini_th_fast, min_th_fast;
  float scale_factor;                   /* ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) */
  float fx, fy, cx, cy, bf, baseline;   /* rectified pinhole, stereoinfo_.baseline_bf_ */
  float th_depth;                       /* Frame::mThDepth */
  float th_last, th_local;              /* th of SearchByProjection(last frame) / (local map): Tracking.cc:296,2365 */
  float nn_last, nn_local;              /* ORBmatcher(nnratio): 0.9 / 0.8 */
  int32_t max_local_points;             /* capacity of the local-map candidate table */
  double Rcb[9], tcb[3];                /* camera <- body */
  double gw[3];                         /* gravity in the world frame */
  double inv_sigma_bg2, inv_sigma_ba2;  /* IMUDataBase::mInvSigmabg2 / mInvSigmaba2 */
  vieo_imu_noise noise;
  int32_t vision_only;                  /* 1: no IMU -- nav_ref of the input is the PREDICTED state of the frame (p, q; the
                                         * rest is carried along), imu / prior inputs are ignored, the two optimisations are
                                         * the vision-only ones and `first` / `second` hold their vieo_pose_result in .base */
  int32_t reserved;
} vieo_tracker_params;

/* The rig of a distorted multi-camera tracker (Frame::usedistort_, mpCameras).  params.fx..cy are not read (camera 0's
 * are used where the reference takes mpCameras[0]->toK()); params.Rcb / tcb: body -> reference camera; params.bf /
 * baseline: stereoinfo_.baseline_bf_. */
typedef struct vieo_tracker_rig {
  int32_t n_cams;                       /* 2..4 */
  int32_t use_lapping;                  /* KB8 cameras hand their lapping area to ExtractORB (Frame.cc:269-273) */
  int32_t lapping[2];                   /* GetvLappingArea() */
  float th_far_pts;                     /* mpLocalMapper->th_far_pts_ (<= 0: off) */
  float reserved;
  vieo_camera cams[4];                  /* model + parameters; Rcb / tcb: body -> camera c (pose optimisation) */
  double Trc[4][12], Tcr[4][12];        /* mpCameras[c]->GetTrc() / GetTcr() (Sophus::SE3<float>) cast to double, 3x4 */
} vieo_tracker_rig;

typedef struct vieo_track_input {
  const uint8_t *left, *right;          /* 8-bit grey images, `stride` bytes per row (or the tracker's own pinned
                                         * planes from vieo_tracker_image_buffers: then no host copy is made) */
  int32_t stride;
  int32_t n_imu;
  const vieo_imu_sample* imu;           /* the samples PreIntegration hands over for [t_ref, t_cur] */
  double t_ref, t_cur;
  vieo_navstate nav_ref;                /* the state the prediction starts from: the last key frame's after a map update,
                                         * else the last frame's (Tracking.cc:392-409) */
  vieo_navstate nav_last;               /* mLastFrame's state (Tcw of the projection search's LastFrame) */
  const vieo_navstate* nav_prior;       /* mNavStatePrior / mMargCovInv of the reference state, NULL: none (mbPrior) */
  const double* H_prior;                /* 15 x 15 row-major */
  int32_t n_last;
  const vieo_last_frame_point* last_points; /* mLastFrame.mvpMapPoints flattened (n_last = its key count) */
  const float* last_track_depth;        /* mTrackDepth of those points (inf: unknown) */
  int32_t n_local;                      /* local-map candidates (all points of the local key frames; the ones the frame
                                         * already holds are dropped on the device through local_alias) */
  int32_t local_version;                /* change it whenever the candidate arrays differ from the previous call's:
                                         * equal versions skip the re-upload (the local map changes per key frame) */
  const vieo_frustum_point* local_points;
  const uint8_t* local_desc;            /* [n_local][32] */
  const int32_t* local_alias;           /* candidate j is last_points[local_alias[j]] (-1: not in the last frame) */
  const uint8_t* images[4];             /* rig trackers: camera c's image (left / right are not read); n_last then counts
                                         * mLastFrame's keys in mvKeys (camera-major) order, up to vieo_tracker_key_capacity */
  /* Frame pipelining (a replay or any caller that has the NEXT frame's images in hand -- a camera
   * driver one frame ahead, a dataset player): the next frame's ExtractORB x 2 + ComputeStereoMatches are queued on a
   * third stream BEHIND this frame's stereo stage and run beside this frame's searches and optimisations (which keep one
   * CU busy; the extraction wants all of them for ~0.2 ms).  The NEXT call then finds its frame extracted: its
   * left / right are not read, and it says so with use_prefetched = 1 -- a call with use_prefetched = 0 discards a pending
   * prefetch.  Outputs are those of the unpipelined call bit for bit (same kernels on the same data).  NULL: off. */
  const uint8_t *next_left, *next_right; /* `stride` bytes per row like left / right */
  int32_t use_prefetched;
  /* ... and the next frame's pre-integration (IMU trackers): with the extraction out of the way it is the 75 us serial
   * chain at the head of the next call.  next_imu = the samples PreIntegration will hand over for [t_cur, next_t_cur],
   * i.e. with THIS frame as the next call's reference: they are integrated beside this frame's tail with the bias this
   * frame's prediction produced (bj_bar = bi_bar + dbi).  The next call uses the result when -- and only when -- its own
   * t_ref / t_cur / samples / nav_ref.bg / nav_ref.ba are bit for bit what was integrated (after a map update the
   * reference is the key frame: the comparison fails and the call integrates as usual).  NULL / 0: off. */
  int32_t next_n_imu;
  const vieo_imu_sample* next_imu;
  double next_t_cur;
  const uint8_t* next_images[4];        /* rig trackers: the next frame's camera images instead of next_left / next_right
                                         * (all of them or none); its extraction runs ahead, its stereo stage in its call */
  /* ... and when the NEXT call's reference will not be this frame: the caller is about to apply a local-BA write-back, so
   * the next prediction starts at the last key frame (Tracking.cc:392-409) and integrates every sample since -- 0.5 ms at
   * the head of that frame's chain.  The run-ahead integration can be told its reference: next_imu = the samples for
   * [next_t_ref, next_t_cur], next_ref_bias = that key frame's (bg, ba) as they will be AFTER the write-back.  Same rule:
   * the next call uses the result only if its own t_ref / t_cur / samples / nav_ref.bg / nav_ref.ba are bit for bit what was
   * integrated.  NULL: the reference is this frame (above). */
  const double* next_ref_bias;          /* [6] bg, ba */
  double next_t_ref;
} vieo_track_input;

#define VIEO_TRACK_OK 0
#define VIEO_TRACK_PREINT_FAILED 1      /* mdeltatij == 0 / CheckIMU: PredictNavStateByIMU returns false; extraction and
                                         * stereo outputs are valid, the tracking outputs are not */
#define VIEO_TRACK_LOST 2               /* fewer than 10 (vision-only: 20) matches after the widened search: TrackWithIMU /
                                         * TrackWithMotionModel return false before the optimisations (Tracking.cc:311,1878);
                                         * extraction, stereo and search outputs are valid, `first` / `second` are not.
                                         * (The inlier gates behind the optimisations -- nmatchesMap, mnMatchesInliers --
                                         * need MapPoint::Observations() and stay with the caller.) */
typedef struct vieo_track_output {
  int32_t status;                       /* VIEO_TRACK_* */
  int32_t n_keys, key_cap;              /* left image: N, and the offset that separates the two point tables */
  const vieo_keypoint* keys;            /* [n_keys] */
  const uint8_t* desc;                  /* [n_keys][32] */
  const float *uright, *depth;          /* ComputeStereoMatches */
  const int32_t* point_ref;             /* per key: -1 none; < key_cap: last_points[i]; else local_points[i - key_cap] */
  const uint8_t* outlier;               /* per key: mvbOutlier after the second optimisation */
  const float* local_track_depth;       /* [n_local] mTrackDepth of the candidates (isInFrustum) */
  int32_t n_matches_last, n_matches_local; /* return values of the two searches */
  int32_t widened;                      /* 1: the first search ran again with 2 * th_last (Tracking.cc:301-309) */
  vieo_navstate nav_pred;               /* PredictNavStateByIMU */
  vieo_imu_preint imu;                  /* the pre-integration [t_ref, t_cur] (Sigma in (p, v, Phi) order) */
  int32_t preint_status;                /* VIEO_PREINT_* */
  int32_t reserved;
  vieo_vio_result first, second;        /* TrackWithIMU's / TrackLocalMapWithIMU's PoseOptimization */
  float ms_gpu;                         /* HIP-event time of the chain, upload to download */
  float ms_host;                        /* wall time of the call */
  /* rig trackers: keys / desc / uright (-1) / depth / point_ref / outlier are in mvKeys order (camera-major) */
  int32_t cam_first[5];                 /* first key of camera c, [n_cams] = n_keys (mapn2in_) */
  int32_t mono_index[4];                /* num_mono of ExtractORB per camera */
  int32_t stereo_status;                /* != 0: more stereo groups than vieo_tracker_group_capacity, no depths */
  int32_t n_groups, n_stereo_matches;   /* ComputeStereoFishEyeMatches: mvidxsMatches.size(), nMatches */
  const int32_t* key_group;             /* [n_keys] mapcamidx2idxs_ (-1: none) */
  const int32_t* group_idx;             /* [n_groups][n_cams] mvidxsMatches */
  const uint8_t* group_good;            /* [n_groups] goodmatches_ */
  const double* group_p3d;              /* [n_groups][3] v3dpoints_ (reference-camera frame) */
} vieo_track_output;

int vieo_tracker_create(vieo_tracker** out, const vieo_tracker_params* params);
int vieo_tracker_create_rig(vieo_tracker** out, const vieo_tracker_params* params, const vieo_tracker_rig* rig /*NULL: rectified*/);
void vieo_tracker_destroy(vieo_tracker* t);
int vieo_tracker_key_capacity(const vieo_tracker* t);   /* keys of a frame at most (n_cams x the extractor's capacity) */
int vieo_tracker_group_capacity(const vieo_tracker* t); /* stereo groups of a rig frame at most */
/* pinned planes the caller may decode the next frame's images into (stride = width) */
int vieo_tracker_image_buffers(vieo_tracker* t, uint8_t** left, uint8_t** right);
int vieo_tracker_image_buffer(vieo_tracker* t, int image_index, uint8_t** plane);
int vieo_tracker_scale_factors(const vieo_tracker* t, float* h_out /*[n_levels]*/);
int vieo_track_frame(vieo_tracker* t, const vieo_track_input* in, vieo_track_output* out);
/* What the tracker knows about its two streams and its replicated optimisations.  A tracker runs its frame on two HIP
 * streams (pre-integration, a rig frame's stereo bookkeeping and the copies back beside the extraction); they overlap only
 * when the runtime serves them from different hardware queues, which it decides from the streams the PROCESS holds.  The
 * second stream is therefore chosen by measurement at creation, the measured figure is kept here, and the choice is made
 * again -- vieo_tracker_reprobe, or by the tracker itself when eight frames in a row take 30 % more GPU time than the
 * running median of the last 32 -- when streams created later have changed the mapping. */
typedef struct vieo_tracker_stats {
  float side_stream_ratio;        /* elapsed(two ~40 us spin kernels started together, one per stream) / elapsed(one):
                                   * ~1 = side by side, ~2 = one hardware queue; > 1.35: no better stream was to be had */
  int32_t side_stream_selections; /* times a second stream was chosen (1 = at creation only) */
  int32_t side_stream_checks;     /* times the ratio was measured again */
  int32_t replica_repeats;        /* rig frames whose optimisations were repeated on one workgroup because a replica
                                   * workgroup never became resident (vieo_pose_set_replicas) */
  float ms_gpu_median;            /* running median of vieo_track_output.ms_gpu (last 32 frames) */
  int32_t slow_frames_in_a_row;   /* frames in a row above 1.3 x that median */
  int32_t frames_prefetched;      /* frames extracted ahead (vieo_track_input.next_left / next_right) */
  int32_t preints_ahead_used;     /* calls that found their pre-integration done by the previous call (next_imu) */
} vieo_tracker_stats;
int vieo_tracker_get_stats(const vieo_tracker* t, vieo_tracker_stats* out);
int vieo_tracker_reprobe(vieo_tracker* t);
/* mvImagePyramid of the frame just tracked, lazily (only Frame::ComputeStereoMatches reads it, src/Frame.cc:457,536-557,
 * and that ran on the device): image 0 = left, 1 = right; see vieo_orb_get_level */
int vieo_tracker_get_level(vieo_tracker* t, int image_index, int level, int with_border, uint8_t* h_dst, int dst_stride);

/* ---- several live sequences in lock step: one call tracks one frame of each of n sequences -------------------------
 * A host that runs several sequences at once (several robots, several camera pairs, a dataset evaluated in parallel)
 * hands the next frame of each to ONE call; the chain of vieo_track_frame runs once over all n frames (each stage one
 * launch over the batch), so n frames cost about what one frame's chain costs plus the extraction of 2n images.
 * A sequence lives in a slot of the handle: the slot keeps that sequence's device-side local map between calls.
 * Contract:
 *  - Byte-identical outputs: every field of out[i], and every array it points to, is byte for byte what a vieo_tracker
 *    created with the same params returns from vieo_track_frame(in[i]) after that sequence's earlier calls -- except
 *    ms_gpu and ms_host, which are the times of the whole call.
 *  - One call, one synchronisation: one upload block, one chain of launches over all n frames, one download and one
 *    host synchronisation -- plus one more only when some frame takes the wider search window (Tracking.cc:301-309):
 *    the tail then runs again from the projection over all n frames (the others recompute the same bytes).
 *  - Configurations: rectified stereo + IMU and params.vision_only.  No rigs: a vieo_tracker_params that
 *    vieo_tracker_create refuses is refused here too (VIEO_E_INVALID); max_sequences is 1..256 (above 256 frames the
 *    pose optimisation switches to another kernel instance, whose bytes differ from the one-frame tracker's).
 *  - Validation before any launch: invalid input in any frame fails the whole call with no slot advanced.
 *    VIEO_E_INVALID: n outside 1..max_sequences, a duplicate or out-of-range slot, an input vieo_track_frame refuses, or
 *    next_left / next_right / next_imu / next_images / use_prefetched set (no frame pipelining here).  VIEO_E_CAPACITY:
 *    the per-frame capacities of vieo_track_frame; vieo_last_error names the slot.
 *  - Per-frame statuses: a frame's VIEO_TRACK_PREINT_FAILED / VIEO_TRACK_LOST is its own; the other frames of the call
 *    are unaffected.
 *  - Outputs point into the handle's pinned download block and stay valid until its next call.
 * Thread model: one handle per host thread, as vieo_tracker. */
typedef struct vieo_tracker_multi vieo_tracker_multi;
/* one vieo_tracker_params for all sequences (same cameras / IMU model); max_sequences 1..256 */
int vieo_tracker_multi_create(vieo_tracker_multi** out, const vieo_tracker_params* params, int max_sequences);
void vieo_tracker_multi_destroy(vieo_tracker_multi* m);
/* pinned planes of slot s the caller may decode that sequence's next images into (stride = width): no host copy then */
int vieo_tracker_multi_image_buffer(vieo_tracker_multi* m, int slot, int image_index, uint8_t** plane);
/* forget slot s's device-side local map (a new sequence starts in that slot) */
int vieo_tracker_multi_reset_slot(vieo_tracker_multi* m, int slot);
/* n frames, frame i belongs to the sequence of slot slots[i] (distinct, < max_sequences); in[i] / out[i] as for
 * vieo_track_frame */
int vieo_track_frames(vieo_tracker_multi* m, int n, const int32_t* slots, const vieo_track_input* in,
                      vieo_track_output* out);

/* Per-call form of the kernel-instance choice (vieo_pose_set_camera_mode / _encoder_mode above are per host thread
 * and kept for old callers): cams_mode VIEO_POSE_CAMS_*, enc_mode VIEO_POSE_ENC_*. */
int vieo_pose_optimization_vio_batch_device_ex(const vieo_vio_frame* d_frames, int n_frames, const vieo_pose_obs* d_obs,
                                               uint8_t* d_outlier, vieo_vio_result* d_results, int cams_mode,
                                               int enc_mode, void* stream);
int vieo_pose_optimization_batch_device_ex(const vieo_pose_frame* d_frames, int n_frames, const vieo_pose_obs* d_obs,
                                           uint8_t* d_outlier, vieo_pose_result* d_results, int cams_mode, void* stream);

/* ---- relocalisation: int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches)
 * (src/ORBmatcher.cc:344-505; Tracking::Relocalization, Tracking.cc:2554; TrackReferenceKeyFrame, :1731) for a batch
 * of key frames against one frame, rectified configuration (F.mapn2in_ empty: every key is of image 0).
 *   device: the Hamming distance of every (key-frame key that holds a map point, frame key) pair of every vocabulary
 *           node both share, all key frames in one launch;
 *   host (inside the library): the walk that depends on its own earlier matches -- frame keys already matched are
 *           skipped, best / second best, TH_LOW (50), the ratio test, the (map point, image) table with its histogram
 *           erasures (an entry is never overwritten once emplaced, as in the reference), the rotation histogram.
 * mFeatVec of both sides is what vieo_bow_transform writes, in the layout of vieo_tri_keyframe. */
typedef struct vieo_bow_keys {
  int32_t n_keys, n_nodes;
  const vieo_keypoint* keys;   /* mvKeys / mvKeysUn: the angle only is read */
  const uint8_t* descriptors;  /* mDescriptors, 32 bytes per key */
  const int32_t* mp_id;        /* key frames: [n_keys] GetMapPointMatches() as ids, -1 = NULL or isBad(), equal ids = the
                                * same MapPoint*; not read for the frame (may be NULL) */
  const uint32_t* node_id;     /* mFeatVec: node ids, ascending */
  const int32_t* node_first;   /* [n_nodes + 1] offsets into node_feat */
  const int32_t* node_feat;    /* feature indices of each node, in the vector's order */
} vieo_bow_keys;               /* 56 bytes */
/* h_match[n_kfs][frame->n_keys]: per key frame, the key-frame key whose map point vpMapPointMatches[i] holds (-1:
 * NULL); h_n_matches[n_kfs]: the return values.  nn_ratio = mfNNratio, check_orientation = mbCheckOrientation.
 * VIEO_E_INVALID before anything is written: a null pointer, nodes not ascending, a feature index out of range, a key
 * angle outside [0, 360). */
int vieo_search_by_bow(const vieo_bow_keys* frame, const vieo_bow_keys* kfs, int n_kfs, float nn_ratio,
                       int check_orientation, int32_t* h_match, int32_t* h_n_matches);
/* The same for a rig frame (F.mapn2in_ filled: the MATCH_KNN_IN_EACH_IMG branch, ORBmatcher.cc:344-505).
 * key_cam[frame->n_keys] = get<0>(mapn2in_[j]), the image of every frame key, each < n_cams (1..4).  Best and second
 * best are kept per image of the frame -- slot img_id exists once a key of an image >= img_id has been looked at, an
 * empty slot holds 256 --, so one key-frame key can hand its map point to one frame key per camera, images ascending;
 * the (map point, image) table is keyed by the real image id.  Outputs as above.  VIEO_E_INVALID before anything is
 * written: as above, n_cams outside 1..4, a key_cam[j] >= n_cams.  With key_cam all zero: vieo_search_by_bow. */
int vieo_search_by_bow_rig(const vieo_bow_keys* frame, const uint8_t* key_cam, int n_cams, const vieo_bow_keys* kfs,
                           int n_kfs, float nn_ratio, int check_orientation, int32_t* h_match, int32_t* h_n_matches);

/* ---- relocalisation: PnPsolver for a batch of candidates (src/PnPsolver.cc; Tracking::Relocalization,
 * Tracking.cc:2567-2604), rectified configuration (Frame::usedistort_ false: mvKeysUn, one pinhole K) ----------------
 * The constructor (:48-105) flattened: per candidate the n correspondences it collects from vpMapPointMatches.
 * vieo_pnp_create evaluates EVERY row of the sample table of every candidate in one launch (pass A: compute_pose on
 * the row's 4 correspondences, CheckInliers over all n) and Refine once per row that raises the best-so-far inlier
 * set in a second launch (pass B); vieo_pnp_iterate then replays PnPsolver::iterate (:154-233) over the two tables.
 * Random draws are the caller's: samples[n_cands][n_rows][4] holds, per row, 4 distinct indices < n drawn in the
 * reference's swap-with-back manner (:174-186); samples == NULL makes the library draw them with a counter-based
 * generator from `seed`.  n_rows is at most 512.  A 4-point hypothesis of the reference is not defined beyond
 * round-off (MtM has a 4-dimensional null space), so no parity per hypothesis exists; see DESIGN.md. */
typedef struct vieo_pnp_candidate {
  int32_t n;                /* correspondences: map points of vpMapPointMatches that are not bad */
  int32_t n_frame_keys;     /* vpMapPointMatches.size(): the length of vbInliers */
  const float* Xw;          /* [n][3] mvP3Dw */
  const float* uv;          /* [n][2] mvP2D (mvKeysUn[i].pt) */
  const float* sigma2;      /* [n] mvSigma2 */
  const int32_t* key_index; /* [n] mvKeyPointIndices */
  float fx, fy, cx, cy;     /* mpCameras[0]->toK() */
} vieo_pnp_candidate;       /* 56 bytes */
typedef struct vieo_pnp_params { /* SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2) */
  double probability;
  int32_t min_inliers, max_iterations, min_set; /* min_set must be 4 */
  float epsilon, th2;
  int32_t reserved;
} vieo_pnp_params;          /* 32 bytes */
typedef struct vieo_pnp_info {
  int32_t n, n_frame_keys;
  int32_t min_inliers, max_its; /* mRansacMinInliers, mRansacMaxIts after SetRansacParameters */
  int32_t n_rows, n_records, mask_words; /* mask_words = (n + 63) / 64 uint64 per inlier mask, bit i = correspondence i */
  int32_t iterations, best_inliers, best_row; /* mnIterations, mnBestInliers, the row that holds mvbBestInliers (-1) */
} vieo_pnp_info;            /* 40 bytes */
typedef struct vieo_pnp vieo_pnp; /* opaque: the tables of all candidates and each candidate's iterate state */
/* VIEO_E_INVALID (nothing is created or launched): a null pointer, n_cands <= 0, n_rows outside 1..512,
 * min_set != 4, a key index outside the frame, a sample index out of range or drawn twice in a row. */
int vieo_pnp_create(vieo_pnp** out, const vieo_pnp_candidate* cands, int n_cands, const vieo_pnp_params* params,
                    const int32_t* samples, int n_rows, uint64_t seed);
void vieo_pnp_destroy(vieo_pnp* h);
int vieo_pnp_get_info(const vieo_pnp* h, int cand, vieo_pnp_info* info);
/* cv::Mat PnPsolver::iterate(nIterations, bNoMore, vbInliers, nInliers) of candidate `cand`: *found = the returned
 * matrix is not empty, Tcw[16] = it (row-major 4x4, rounded to float as :200-206 / :264-270 do), inliers[n_frame_keys]
 * = vbInliers (all zero unless found), *row_used (may be NULL) = the sample row at which Refine succeeded, or the best
 * row when the pose is mBestTcw at bNoMore; -1 otherwise.  VIEO_E_CAPACITY: the call needs a row beyond n_rows. */
int vieo_pnp_iterate(vieo_pnp* h, int cand, int n_iterations, int32_t* found, float* Tcw, uint8_t* inliers,
                     int32_t* n_inliers, int32_t* no_more, int32_t* row_used);
/* test taps (any pointer may be NULL).  Rows of pass A: samples[n_rows][4], Rt[n_rows][12] = R row-major then t
 * (double), count[n_rows], mask[n_rows][mask_words].  Records of pass B: rec_row[n_records] = the row that opened the
 * record, then the same three tables per record. */
int vieo_pnp_tap_rows(const vieo_pnp* h, int cand, int32_t* samples, double* Rt, int32_t* count, uint64_t* mask);
int vieo_pnp_tap_records(const vieo_pnp* h, int cand, int32_t* rec_row, double* Rt, int32_t* count, uint64_t* mask);
/* test tap: pass B alone on given inlier sets of one candidate -- masks[n_masks][mask_words], each with >= 4 bits */
int vieo_pnp_tap_refine(const vieo_pnp_candidate* cand, const vieo_pnp_params* params, const uint64_t* masks, int n_masks,
                        double* Rt, int32_t* count, uint64_t* out_masks);

/* ---- PnPsolver with Frame::usedistort_ (a frame of a 1- to 4-camera rig, distorted or not) -------------------------
 * mvP2D are the raw mvKeys pixels and mapidx2cami_ the camera of every correspondence.  add_correspondence
 * (PnPsolver.cc:340-365) un-projects the pixel through its own camera (UnProject to the plane z = 1, 10 iterations,
 * precision 1e-8f), moves it into the reference camera with GetTrc(), applies toK() of camera 0 and divides: `usun`,
 * which fill_M reads.  Getuv (:277-291) maps a point of the reference camera by GetTcr() of the correspondence's
 * camera and calls that camera model's Project; it serves reprojection_error inside compute_pose (against the raw
 * pixel) and CheckInliers.  A projection that is not finite (z = 0, a point behind a pinhole-like camera whose
 * quotient overflows) makes the correspondence an outlier. */
typedef struct vieo_pnp_rig {
  int32_t n_cams;        /* 1..4 */
  int32_t reserved;
  vieo_camera cams[4];   /* model + float parameters of mpCameras[c]; Rcb / tcb not read here */
  double Tcr[4][12];     /* GetTcr().cast<double>(), row-major 3x4 */
  double Trc[4][12];     /* GetTrc().cast<double>() -- given, not inverted by the library */
} vieo_pnp_rig;          /* 1384 bytes */
/* vieo_pnp_create for such a frame: cam_of[c] = [cands[c].n] mapidx2cami_ of candidate c (each < rig->n_cams),
 * cands[c].uv = the mvKeys pixels, cands[c].fx..cy = cams[0]'s toK().  The handle is the same: iterate, get_info, the
 * taps and destroy work on it as they are.  VIEO_E_INVALID in addition: a null rig or cam_of, n_cams outside 1..4, an
 * unknown camera model, a camera index >= n_cams. */
int vieo_pnp_create_rig(vieo_pnp** out, const vieo_pnp_candidate* cands, int n_cands, const uint8_t* const* cam_of,
                        const vieo_pnp_rig* rig, const vieo_pnp_params* params, const int32_t* samples, int n_rows,
                        uint64_t seed);
/* test taps: pass B alone as vieo_pnp_tap_refine; usun[n][2] of candidate `cand` of a handle made by
 * vieo_pnp_create_rig (VIEO_E_INVALID for a rectified handle) */
int vieo_pnp_tap_refine_rig(const vieo_pnp_candidate* cand, const uint8_t* cam_of, const vieo_pnp_rig* rig,
                            const vieo_pnp_params* params, const uint64_t* masks, int n_masks, double* Rt, int32_t* count,
                            uint64_t* out_masks);
int vieo_pnp_tap_usun(const vieo_pnp* h, int cand, double* usun /*[n][2]*/);

/* ---- relocalisation: bool Tracking::Relocalization() (src/Tracking.cc:2541-2663) for one lost frame: the
 * rectified configuration here, a frame of a camera rig below (vieo_relocalize_rig).  SearchByBoW of every candidate (ORBmatcher(0.75, true); fewer than 15 matches: discarded), one
 * PnPsolver per kept candidate (SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)), and then the reference's
 * round-robin while: iterate(5) per candidate; on a pose ReplaceMapPointMatch / EraseMapPointMatch by the inlier
 * flags, PoseOptimization, nGood < 10 -> next candidate, erase outliers; below 50 the search with th = 10,
 * ORBdist = 100 against sFound and a second optimisation; for 30 < nGood < 50 the search with th = 3, ORBdist = 64
 * against all points held and the last optimisation; success at nGood >= 50.  The two searches and the PnP stage run
 * ahead for all candidates in one call each; the decisions between the stages stay sequential on the host.  The
 * candidates come from vieo_kfdb_detect_reloc and both mFeatVec from vieo_bow_transform (or from the caller's DBoW2);
 * the IMU bookkeeping after success (:2668-2684) is the caller's.  A frame of a vieo_tracker enters through the arrays of
 * its vieo_track_output (keys, descriptors, uright). */
typedef struct vieo_reloc_frame {
  int32_t n_keys, n_levels;        /* N; scalepyrinfo_ levels, 1..16 */
  const vieo_keypoint* keys;       /* mvKeysUn */
  const float* uright;             /* stereoinfo_.vuright_ (< 0: monocular key) */
  const uint8_t* descriptors;      /* mDescriptors */
  const float* level_sigma2;       /* vlevelsigma2_ */
  const float* inv_level_sigma2;   /* vinvlevelsigma2_ */
  const float* scale_factor;       /* vscalefactor_ */
  float log_scale_factor;          /* flogscalefactor_ */
  float fx, fy, cx, cy, bf;
  float bounds[4];                 /* gridinfo_.minmax_xy_: min_x, max_x, min_y, max_y */
  int32_t n_nodes, n_cams;         /* mFeatVec's nodes; n_cams: 0 for vieo_relocalize, the rig's 1..4 for vieo_relocalize_rig */
  double Rcb[9], tcb[3];           /* meigRcb (row-major), meigtcb */
  const uint32_t* node_id;         /* mFeatVec as for vieo_bow_keys */
  const int32_t* node_first;
  const int32_t* node_feat;
} vieo_reloc_frame;                /* 224 bytes */
typedef struct vieo_reloc_candidate {
  vieo_bow_keys kf;                   /* the key frame as for vieo_search_by_bow */
  const vieo_keyframe_point* points;  /* [kf.n_keys] GetMapPointMatches() flattened; bit 0 of flags is ANDed with
                                       * kf.mp_id[k] >= 0 and with "not in sFound" by the library */
} vieo_reloc_candidate;               /* 64 bytes */
typedef struct vieo_reloc_visit {  /* one line of the trace */
  int32_t cand;
  int32_t call;          /* 0: the SearchByBoW stage (n_inliers = its return value, no_more = 1: discarded);
                          * k >= 1: the candidate's k-th iterate(5) */
  int32_t row;           /* the sample row the returned pose belongs to, -1 none */
  int32_t no_more;       /* bNoMore (2: the sample table is used up, the candidate is discarded like bNoMore) */
  int32_t found;         /* iterate returned a pose */
  int32_t n_inliers;     /* nInliers */
  int32_t n_good[3];     /* nGood after the first, second and last PoseOptimization; -1: not run */
  int32_t n_additional[2]; /* nadditional of the th = 10 and of the th = 3 search; -1: not run */
  int32_t reserved;
} vieo_reloc_visit;      /* 48 bytes */
typedef struct vieo_reloc_result {
  int32_t found, cand, n_good, n_visits; /* bMatch, the candidate that matched (-1), its last nGood, lines of the trace */
  vieo_navstate nav;     /* the optimised state (p, q; the other fields zero) */
  float Tcw[16];         /* mCurrentFrame's pose after UpdatePoseFromNS, row-major 4x4 */
} vieo_reloc_result;     /* 256 bytes */
/* samples[n_cands][n_rows][4] as for vieo_pnp_create (rows of discarded candidates are not read), or NULL and `seed`.
 * Outputs: mp_ref[n_keys] = the matched candidate's key whose map point frame key j holds (-1 none; all -1 when not
 * found), outlier[n_keys] = mvbOutlier, trace[trace_capacity].  VIEO_E_INVALID before anything is written: null
 * pointers, n_cams != 0 (a rig frame goes to vieo_relocalize_rig), n_rows outside 1..512, levels or octaves out of
 * range.  VIEO_E_CAPACITY: more visits than
 * trace_capacity (the outputs are complete, the trace is cut). */
int vieo_relocalize(const vieo_reloc_frame* frame, const vieo_reloc_candidate* cands, int n_cands,
                    const int32_t* samples, int n_rows, uint64_t seed, vieo_reloc_result* result, int32_t* mp_ref,
                    uint8_t* outlier, vieo_reloc_visit* trace, int32_t trace_capacity);
/* The same for a frame of a 1- to 4-camera rig (Frame::usedistort_, mapn2in_ filled).  frame: as above with keys =
 * mvKeys in camera-major order, n_cams = rig->pnp.n_cams, fx..cy = toK() of camera 0, Rcb / tcb = body -> reference
 * camera, bounds unused (rig->sbp has them per camera).  The stages: vieo_search_by_bow_rig with each key's camera
 * from cam_first, vieo_pnp_create_rig, vieo_pose_optimization with n_cams / pose_cams and the observation's camera in
 * bits 8..11 of its flags, vieo_sbp_project_keyframe(rig->sbp) + vieo_search_by_projection_rig(VIEO_SBP_RELOC) for
 * both widening searches.  sFound is a set of map-point ids: a point held by keys of two cameras is one element.
 * Trace, result and return codes as above; VIEO_E_INVALID in addition: a null rig member, n_cams outside 1..4 or
 * different in frame / rig->pnp / rig->sbp, cam_first not starting at 0, decreasing, or not ending at n_keys. */
typedef struct vieo_reloc_rig {
  vieo_pnp_rig pnp;
  const int32_t* cam_first;     /* [n_cams + 1], camera c owns keys [cam_first[c], cam_first[c+1]) */
  const vieo_sbp_rig* sbp;      /* for the two widening searches */
  const vieo_camera* pose_cams; /* [n_cams] with Rcb / tcb composed, as vieo_pose_frame.cams */
} vieo_reloc_rig;               /* 1408 bytes */
int vieo_relocalize_rig(const vieo_reloc_frame* frame, const vieo_reloc_rig* rig, const vieo_reloc_candidate* cands,
                        int n_cands, const int32_t* samples, int n_rows, uint64_t seed, vieo_reloc_result* result,
                        int32_t* mp_ref, uint8_t* outlier, vieo_reloc_visit* trace, int32_t trace_capacity);

/* ---- place recognition: the vocabulary (loop/DBoW2/DBoW2/TemplatedVocabulary.h), FrameBase::ComputeBoW
 * (src/FrameBase.cpp:83-93) and KeyFrameDatabase (src/KeyFrameDatabase.cc) -------------------------------------------
 * vieo_vocabulary: the tree, uploaded once and resident.  Only L1_NORM scoring (0) with TF_IDF weighting (0) -- what
 * ORBvoc uses -- is supported; anything else is VIEO_E_INVALID before any allocation. */
typedef struct vieo_voc_node { /* node `row + 1` of the table, in file order (the root, node 0, is not in the table) */
  int32_t parent;              /* node id, 0 <= parent < own id; a node's children are in row order */
  int32_t is_leaf;             /* != 0: a word; word ids are handed out in row order over the leaves */
  uint8_t descriptor[32];
  double weight;
} vieo_voc_node;               /* 48 bytes */
typedef struct vieo_voc_info {
  int32_t k, L, n_nodes, n_words; /* n_nodes counts the table's rows (without the root) */
} vieo_voc_info;               /* 16 bytes */
typedef struct vieo_vocabulary vieo_vocabulary; /* opaque */
/* VIEO_E_INVALID (*out untouched): a null pointer, k outside 0..20, L outside 1..10, scoring != 0 or weighting != 0,
 * a parent >= its own id or < 0, an inner node without children, a leaf with children, more than k children. */
int vieo_vocabulary_create(vieo_vocabulary** out, int k, int L, int scoring, int weighting, const vieo_voc_node* nodes,
                           int n_nodes);
/* The reference's two files, chosen as System.cc:515-519 does: ".txt" in the name is the text form (header
 * "k L scoring weighting", then "parent is_leaf d0 .. d31 weight" per node), anything else the binary form (uint32
 * nb_nodes, uint32 size_node = 41, int32 k, L, scoring, weighting, then nb_nodes - 1 records of int32 parent, 32 bytes,
 * float weight, uint8 is_leaf).  Unlike both reference loaders no node is appended after the last record (theirs loop on
 * !eof(); the extra node is a duplicate sibling the strict < of the descent never selects).  VIEO_E_INVALID (*out
 * untouched): the file cannot be read, a header outside the reference's limits, size_node != 41, a short or malformed
 * record, and whatever vieo_vocabulary_create refuses. */
int vieo_vocabulary_load(vieo_vocabulary** out, const char* path);
int vieo_vocabulary_info(const vieo_vocabulary* voc, vieo_voc_info* info);
void vieo_vocabulary_destroy(vieo_vocabulary* voc);

/* TemplatedVocabulary::transform(features, v, fv, levelsup) for a batch of frames: one kernel descends every key of
 * every frame, one sorts and run-length-compresses each frame's (word, node, index) triples (one workgroup per frame).
 * The descent is greedy from the root, the first child wins ties; it stops at the first node without children.  The
 * reported node is the one reached at level L - levelsup, the root (0) when L - levelsup <= 0, and THE LEAF'S OWN NODE
 * ID when the leaf is shallower than that level (the reference leaves nid uninitialised there).  A word of weight <= 0
 * contributes to neither vector; the values are L1-normalised. */
typedef struct vieo_bow_frame {
  int32_t n_keys, reserved;
  const uint8_t* descriptors;  /* [n_keys][32] */
} vieo_bow_frame;              /* 16 bytes */
typedef struct vieo_bow_vectors { /* the caller's arrays: n_keys entries each (node_first: n_keys + 1) are enough */
  int32_t n_words, n_nodes;    /* out */
  uint32_t* word_id;           /* mBowVec: word ids, ascending */
  double* word_value;
  uint32_t* node_id;           /* mFeatVec in the layout vieo_bow_keys / vieo_tri_keyframe / vieo_reloc_frame read */
  int32_t* node_first;
  int32_t* node_feat;          /* within a node the feature indices ascend */
} vieo_bow_vectors;            /* 48 bytes */
#define VIEO_BOW_MAX_KEYS 8192
/* VIEO_E_INVALID: a null pointer, n_frames <= 0, n_keys < 0.  VIEO_E_CAPACITY: a frame of more than VIEO_BOW_MAX_KEYS
 * keys.  Nothing is written in either case. */
int vieo_bow_transform(const vieo_vocabulary* voc, const vieo_bow_frame* frames, int n_frames, int levelsup,
                       vieo_bow_vectors* out);

/* KeyFrameDatabase: every added key frame's BowVector lives on the device (CSR); a query is ONE launch that computes, for
 * every stored key frame, the number of words it shares with the query, the smallest shared word id and
 * L1Scoring::score (one wavefront per key frame).  The sequential tail (the list in the order of the inverted file's
 * walk = ascending (smallest shared word id, insertion sequence), minCommonWords, the accumulation over the covisible
 * key frames, 0.75 * bestAccScore) runs on the host inside the library.  mRelocScore / mLoopScore are kept per key frame
 * across queries as the reference's members are (initial value 0, which the reference leaves undefined).  Each call is a
 * fresh query id: the reference's double counting when one nid_ queries twice is not reproduced.  A query holds at
 * most VIEO_BOW_MAX_KEYS words (VIEO_E_CAPACITY), ascending (VIEO_E_INVALID). */
typedef struct vieo_kfdb vieo_kfdb; /* opaque */
int vieo_kfdb_create(vieo_kfdb** out, const vieo_vocabulary* voc);
void vieo_kfdb_destroy(vieo_kfdb* db);
int vieo_kfdb_clear(vieo_kfdb* db);
int vieo_kfdb_size(const vieo_kfdb* db); /* stored key frames (< 0: an error code) */
/* VIEO_E_INVALID (nothing changes): a null pointer, an id already stored, words not ascending or >= the vocabulary's. */
int vieo_kfdb_add(vieo_kfdb* db, int64_t kf_id, const uint32_t* word_id, const double* word_value, int n_words);
int vieo_kfdb_erase(vieo_kfdb* db, int64_t kf_id); /* VIEO_E_INVALID: the id is not stored */
/* GetBestCovisibilityKeyFrames(10) of the key frame, n <= 10; the caller refreshes it when the graph changes.  Ids
 * that are not stored when a query runs are skipped. */
int vieo_kfdb_set_covisible(vieo_kfdb* db, int64_t kf_id, const int64_t* ids, int n);
/* out[i] = mpVoc->score(query, key frame kf_ids[i]) (double); VIEO_E_INVALID and nothing written: an id not stored */
int vieo_kfdb_scores(vieo_kfdb* db, const uint32_t* word_id, const double* word_value, int n_words,
                     const int64_t* kf_ids, int n_ids, double* out);
/* DetectRelocalizationCandidates (KeyFrameDatabase.cc:175-279).  VIEO_E_CAPACITY: more candidates than `capacity`;
 * *n_out holds the number needed, out_ids and the kept scores are untouched. */
int vieo_kfdb_detect_reloc(vieo_kfdb* db, const uint32_t* word_id, const double* word_value, int n_words,
                           int64_t* out_ids, int capacity, int32_t* n_out);
/* DetectLoopCandidates (:52-173): connected_ids = pKF->GetConnectedKeyFrames() (not listed, never a neighbour) */
int vieo_kfdb_detect_loop(vieo_kfdb* db, const uint32_t* word_id, const double* word_value, int n_words,
                          const int64_t* connected_ids, int n_connected, float min_score, int64_t* out_ids, int capacity,
                          int32_t* n_out);
/* test tap: the device's table of the last query, stored key frames in insertion order (first_word 0xFFFFFFFF: shares
 * nothing); every array holds the size the database had at that query.  VIEO_E_EMPTY: no query since the last change. */
int vieo_kfdb_tap_query(const vieo_kfdb* db, int64_t* kf_ids, int32_t* n_common, uint32_t* first_word, double* score);

/* ------------------------------------------------------------------------------------------------------------------
 * Pose-graph optimisation: Optimizer::OptimizeEssentialGraph (Optimizer.cc:2309-2687), the numeric call of
 * LoopClosing::CorrectLoop.  One Sim3 vertex per key frame, one EdgeSim3 per edge, g2o's Levenberg-Marquardt with
 * numeric (central-difference, delta = 1e-9) Jacobians, then every key-frame pose and every map point is transformed.
 * All arrays are host pointers; the call is synchronous. */
typedef struct vieo_sim3 {
  double q[4]; /* Eigen's coefficient order: x, y, z, w */
  double t[3];
  double s;
} vieo_sim3; /* 64 bytes */

#define VIEO_PG_EDGE_LOOP 0  /* a new loop connection: measurement Scw[j] * Scw[i]^-1 (:2400-2417) */
#define VIEO_PG_EDGE_PRIOR 1 /* spanning tree / old loop / covisibility: Scw_prior[j] * Scw_prior[i]^-1 (:2477-2611) */

typedef struct vieo_pose_graph {
  int32_t n_kf;         /* key frames 0 .. n_kf-1 in the order of nid_ */
  int32_t n_edges;
  int32_t n_mp;
  int32_t fixed_kf;     /* pLoopKF */
  int32_t fix_scale;    /* bFixScale */
  int32_t n_iterations; /* 20 in the reference */
  double lambda_init;   /* setUserLambdaInit: 1e-16 in the reference */
  const uint8_t* valid;       /* [n_kf] 0: a bad key frame (no vertex; an edge that names it is VIEO_E_INVALID) */
  const vieo_sim3* Scw;       /* [n_kf] vScw: CorrectedSim3 where there is one, else (Rcw, tcw, 1) */
  const vieo_sim3* Scw_prior; /* [n_kf] NonCorrectedSim3 where there is one, else Scw */
  const int32_t* edge_i;      /* [n_edges] vertex 0 */
  const int32_t* edge_j;      /* [n_edges] vertex 1 */
  const int32_t* edge_kind;   /* [n_edges] VIEO_PG_EDGE_* */
  const double* edge_info;    /* [2 n_edges] (w_r, w_t): information diag(w_r I3, w_t I3, 1); (1, 1) but for odometry edges */
  const float* Pw;            /* [3 n_mp] */
  const int32_t* ref_kf;      /* [n_mp] nIDr of :2658-2668; -1: a bad point, left as it is */
} vieo_pose_graph; /* 104 bytes */

typedef struct vieo_pg_trial { /* one line of the trace: one lambda trial */
  double chi2_before, chi2_after, lambda;
  int32_t accepted;
  int32_t solved; /* 0: a non-positive pivot, the trial failed */
} vieo_pg_trial; /* 32 bytes */

typedef struct vieo_pose_graph_result {
  int32_t status; /* VIEO_OK */
  int32_t n_unknowns;
  int32_t lm_iterations, lm_trials;
  double chi2_initial, chi2_final;
  int32_t n_trace;   /* lines written: min(lm_trials, trace_cap) */
  int32_t trace_cap; /* in */
  vieo_sim3* Scw_opt;   /* [n_kf]; an invalid key frame's entry is a copy of Scw */
  double* Tcw;          /* [12 n_kf] rows of R | t / s (:2636-2644); zeros for an invalid key frame */
  float* Pw_out;        /* [3 n_mp] Scw_opt[r]^-1.map(Scw[r].map(double(Pw))) (:2670-2679) */
  double* Pw_out_d;     /* test tap, NULL in production: [3 n_mp] the same points before their cast to float */
  vieo_pg_trial* trace; /* [trace_cap], may be NULL with trace_cap 0 */
  uint64_t bytes_needed; /* VIEO_E_CAPACITY: the device memory the call needs */
} vieo_pose_graph_result; /* 88 bytes */

/* Duplicate (i, j) pairs are legal and summed in edge order.  No free vertex or no edge: VIEO_OK, poses unchanged, points
 * mapped through the identity correction.  VIEO_E_INVALID before anything is written: a null pointer, an index out of
 * range, an edge with i == j or one that names an invalid key frame, an invalid fixed_kf, a kind other than 0 / 1.
 * VIEO_E_CAPACITY (bytes_needed set, nothing else written): the factor does not fit into device memory.  A trial whose
 * factorisation meets a non-positive pivot fails as a trial (g2o: lambda grows), not as a call.  Two calls on the same
 * input return byte-identical output; so does a call under VIEO_PG_GEOMETRY=alt, a test switch that runs the per-edge
 * and per-vertex kernels with a second block size. */
int vieo_optimize_essential_graph(const vieo_pose_graph* g, vieo_pose_graph_result* out);
/* test tap: e[7 n_edges] and both Jacobians Ji, Jj [49 n_edges] (row-major, d e / d vertex 0, d e / d vertex 1) of every
 * edge at the estimates Scw, as the first linearisation of the call above computes them. */
int vieo_pose_graph_linearize(const vieo_pose_graph* g, double* e, double* Ji, double* Jj);
/* test tap: one linear solve of the call above at the estimates Scw -- measure, linearise, assemble, one factorisation of
 * H + lambda I and one back substitution, through the launches the optimisation uses.  With n = (6 or 7) x the free key
 * frames (valid, not fixed_kf, with an edge; unknowns in key-frame order): x[n] the step, b[n] the right-hand side,
 * H_lower[n * n] the assembled H gathered from its tiles as a dense row-major lower triangle (zeros above the diagonal
 * and outside the envelope), *ok 0 where a pivot was not positive (x is finite all the same).  n_iterations and
 * lambda_init are not read.  n = 0: *ok = 1, nothing else is written. */
int vieo_pose_graph_solve(const vieo_pose_graph* g, double lambda, double* x, double* b, double* H_lower, int32_t* ok);

/* ---- loop verification, first half: what LoopClosing::ComputeSim3 (src/LoopClosing.cc:308-489) does for every loop
 * candidate before any decision depends on another candidate -- SearchByBoW(KeyFrame*, KeyFrame*) and the Sim3Solver.
 * SearchBySim3, OptimizeSim3 and the final SearchByProjection(KeyFrame*, Scw, ...) follow below (vieo_search_by_sim3,
 * vieo_optimize_sim3, vieo_search_by_projection_scw), and so does the round-robin while that strings them together
 * (vieo_compute_sim3); the gather of the loop points is the caller's.
 *
 * int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (src/ORBmatcher.cc:726-905) of the current
 * key frame kf1 against n_kf2 candidates in one call.  Device: the Hamming distance of every (key of kf1 that holds a
 * map point, key of a candidate) pair of every vocabulary node both share, all candidates in one launch.  Host: the
 * reference's walk -- the outer loop over kf1's keys of the node (mp_id < 0 skipped), the inner one skipping
 * vbMatched2 and candidate keys without a map point, one best / second best slot (MATCH_KNN_IN_EACH_IMG is undefined),
 * best < TH_LOW (50, strictly), the ratio test in float, the (pMP1, 0) table (equal mp_id = the same MapPoint*; a hit
 * rejects with <=, a strictly smaller distance clears vpMatches12 / vbMatched2 of the entry, counts nmatches down and
 * lists the entry's histogram slot for erasure; emplace never overwrites the entry), the rotation histogram.
 * h_match12[n_kf2][kf1->n_keys]: per candidate, the candidate's key whose map point vpMatches12[i1] holds (-1: NULL);
 * h_n_matches[n_kf2]: the return values.  mp_id is read on both sides.  VIEO_E_INVALID before anything is written, as
 * for vieo_search_by_bow. */
int vieo_search_by_bow_kf(const vieo_bow_keys* kf1, const vieo_bow_keys* kf2s, int n_kf2, float nn_ratio,
                          int check_orientation, int32_t* h_match12, int32_t* h_n_matches);

/* Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h) for a batch of candidates.  The constructor (:22-116) flattened:
 * per candidate the n correspondences it collects (one per index of GetIndexInKeyFrame, so a map point seen by several
 * cameras of a rig gives several with the same index1).  vieo_sim3_create evaluates EVERY row of the sample table of
 * every candidate in one launch -- ComputeSim3 (Horn's closed form, :220-322) on the row's 3 pairs, CheckInliers
 * (:324-344) over all n --; vieo_sim3_iterate replays Sim3Solver::iterate (:143-204) over that table.
 * max_err1 / max_err2 are INTEGERS: mvnMaxError1/2 are std::vector<size_t> (Sim3Solver.h:61-62), so the threshold of
 * a correspondence is (size_t)(9.210 * sigma2) with the product taken in double, and the test `float err < size_t`
 * compares with that integer converted to float.  The camera tables hold pcams_[0] / pcams_[1] with GetTcr() in
 * Rcb / tcb (the reference's SE3f product is taken in FP64 here); the rectified configuration (usedistort_ false) is one
 * pinhole with the identity.  Horn's form runs in FP64 from the float inputs (the reference: CV_32F and cv::eigen), so
 * a hypothesis agrees with the reference's to its float round-off, not bit for bit; see DESIGN.md.
 * Random draws are the caller's: samples[n_cands][n_rows][3] holds, per row, 3 distinct indices < n drawn in the
 * reference's swap-with-back manner (:164-178); samples == NULL makes the library draw them with its counter-based
 * generator from `seed`.  n_rows is at most 512 (the reference's cap on iterations is 300). */
typedef struct vieo_sim3_candidate {
  int32_t n;               /* correspondences (N) */
  int32_t n1;              /* vpMatched12.size() (mN1): the length of vbInliers */
  const float* X1;         /* [n][3] mvX3Dc1: the point of kf1 in kf1's rig frame */
  const float* X2;         /* [n][3] mvX3Dc2: the matched point in the candidate's rig frame */
  const int32_t* max_err1; /* [n] mvnMaxError1 = (size_t)(9.210 * sigma2 of kp1's octave) */
  const int32_t* max_err2; /* [n] mvnMaxError2 */
  const int32_t* index1;   /* [n] mvnIndices1, each in [0, n1) */
  const int32_t* cam1;     /* [n] mapidx2cami_[0], each in [0, n_cams1) */
  const int32_t* cam2;     /* [n] mapidx2cami_[1], each in [0, n_cams2) */
  const vieo_camera* cams1; /* [n_cams1] pcams_[0]; Rcb / tcb = GetTcr() */
  const vieo_camera* cams2; /* [n_cams2] pcams_[1] */
  int32_t n_cams1, n_cams2; /* 1 ... 8 */
  int32_t fix_scale;       /* mbFixScale */
  int32_t reserved;
} vieo_sim3_candidate;     /* 96 bytes */
typedef struct vieo_sim3_params { /* SetRansacParameters(probability, minInliers, maxIterations) */
  double probability;
  int32_t min_inliers, max_iterations; /* min_inliers >= 3: the minimal set */
} vieo_sim3_params;        /* 16 bytes */
typedef struct vieo_sim3_info {
  int32_t n, n1;
  int32_t min_inliers, max_its; /* mRansacMinInliers, mRansacMaxIts after SetRansacParameters (:118-141); a candidate
                                 * with n < min_inliers has no solver (bNoMore at :148) and reports max_its 1 */
  int32_t n_rows, mask_words;   /* mask_words = (n + 63) / 64 uint64 per inlier mask, bit i = correspondence i */
  int32_t iterations, best_inliers, best_row; /* mnIterations, mnBestInliers, the row that holds mBestT12 (-1) */
  int32_t reserved;
} vieo_sim3_info;          /* 40 bytes */
typedef struct vieo_sim3_solver vieo_sim3_solver; /* opaque: the table of all candidates and each one's iterate state */
/* VIEO_E_INVALID (nothing is created or launched): a null pointer, n_cands <= 0, n_rows outside 1..512, parameters out
 * of range, an index1 outside n1, a camera index outside its table, an unknown camera model, a negative max_err, a
 * sample index out of range or drawn twice in a row. */
int vieo_sim3_create(vieo_sim3_solver** out, const vieo_sim3_candidate* cands, int n_cands, const vieo_sim3_params* params,
                     const int32_t* samples, int n_rows, uint64_t seed);
void vieo_sim3_destroy(vieo_sim3_solver* h);
int vieo_sim3_get_info(const vieo_sim3_solver* h, int cand, vieo_sim3_info* info);
/* cv::Mat Sim3Solver::iterate(nIterations, bNoMore, vbInliers, nInliers) of candidate `cand`: *found = the returned
 * matrix is not empty, T12[16] = it (row-major 4x4: s R | t, rounded to float), inliers[n1] = vbInliers, *row_used (may
 * be NULL) = the sample row that was returned, -1 otherwise.  find() is iterate(max_its).  VIEO_E_CAPACITY: the call
 * needs a row beyond n_rows. */
int vieo_sim3_iterate(vieo_sim3_solver* h, int cand, int n_iterations, int32_t* found, float* T12, uint8_t* inliers,
                      int32_t* n_inliers, int32_t* no_more, int32_t* row_used);
/* GetEstimatedRotation / Translation / Scale: mBestRotation, mBestTranslation, mBestScale of the best row so far, rounded
 * to float.  VIEO_E_EMPTY (nothing written) before the first iteration. */
int vieo_sim3_get_estimate(const vieo_sim3_solver* h, int cand, float* R12, float* t12, float* s12);
/* test tap (any pointer may be NULL): samples[n_rows][3], sRt[n_rows][13] = R row-major, t, s (double), count[n_rows],
 * mask[n_rows][mask_words]; zeros for a candidate without a solver. */
int vieo_sim3_tap_rows(const vieo_sim3_solver* h, int cand, int32_t* samples, double* sRt, int32_t* count, uint64_t* mask);

/* ---- loop verification: int ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)
 * (src/ORBmatcher.cc:1222-1301) for a list of visits in one call.  A visit is (the current key frame kf1, a candidate,
 * a Sim3, match12 in/out); the visits of a call may name one candidate several times with different Sim3.
 *
 * vieo_loop_keyframe is a key frame as loop verification reads it: the vieo_bow_keys record (keys: x, y, octave of
 * mvKeysUn -- mvKeys when use_distort --, descriptors, mp_id) plus, per key, its camera and its map point, the pose,
 * the rig and the pyramid tables.  points[i] is read only where mp_id[i] >= 0; its skip_mask is ignored.
 *   host, float as the reference's CV_32F expressions (:1233-1236, :1265, :1274): sR12 = s12 * R12, sR21 =
 *           (float)(1.0 / s12) * R12^T, t21 = -(sR21 * t12), the transforms sR21 * R1w, sR21 * t1w + t21 and sR12 * R2w,
 *           sR12 * t2w + t12 (every product row times column, summed left to right); vbAlreadyMatched1 / 2 (:1246-1261)
 *           from match12, cam_of_key and mp_id (GetIndexInKeyFrame = every key of the key frame with that id).  As in
 *           the reference the camera of a key counts in its OWN key frame and gates that camera index of the OTHER one.
 *   device: the search of SearchByProjectionBase (:26-192) for every (visit, direction, map point, camera) in one
 *           launch -- th_radius = th, no viewing-angle test, pbf = nullptr, mode (char)~SBPMatchMultiCam (only1match and
 *           fuselater: no IsInKeyFrame skip) -- over the grids of all key frames, each built once per (key frame, camera).
 *   host, after one copy back (:193-225, :1282-1298): over the cameras the strictly smaller bestDist wins, and only if
 *           the key at bestIdx holds a map point (a best key without one is dropped, not replaced by the next best);
 *           <= TH_HIGH (100); vnMatch = all keys that hold that map point, ascending; the first idx2 of vnMatch[0][i1]
 *           whose vnMatch[1][idx2] contains i1 sets match12[i1] = idx2.
 * match12[i1] is, as for vieo_search_by_bow_kf, the candidate's key whose map point vpMatches12[i1] holds (-1: NULL;
 * a key without a map point counts as NULL). */
typedef struct vieo_loop_keyframe {
  vieo_bow_keys bow;                 /* n_keys <= 8192; node_* are not read by vieo_search_by_sim3 */
  const int32_t* cam_of_key;         /* [n_keys] get<0>(mapn2in_[i]); NULL: every key is of camera 0 */
  const vieo_fuse_point* points;     /* [n_keys] the map point of key i: GetWorldPos, GetNormal, mfMaxDistance,
                                      * mfMinDistance, GetDescriptor */
  const struct vieo_camera* cams;    /* [n_cams] mpCameras (Rcb / tcb unused) */
  float Rcw[9], tcw[3], Ow[3];       /* GetRotation(), GetTranslation(), GetCameraCenter() */
  int32_t n_cams;                    /* 1..4 */
  int32_t use_distort;               /* usedistort_: 0 -> K * (x/z, y/z, 1) in float, 1 -> camera Project() */
  float Tcr[4][12];                  /* GetTcr().matrix3x4() row-major */
  float trc[4][3];                   /* GetTrc().translation() */
  float bounds[4][4];                /* gridinfo_.minmax_xy_[i] = {min_x, max_x, min_y, max_y} */
  float scale_factors[16];           /* scalepyrinfo_.vscalefactor_ */
  float level_sigma2[16];            /* vlevelsigma2_ */
  float inv_level_sigma2[16];        /* vinvlevelsigma2_ */
  float log_scale_factor;            /* flogscalefactor_ */
  int32_t n_levels;                  /* 1..16 */
} vieo_loop_keyframe;                /* 656 bytes */
typedef struct vieo_sim3_visit {
  int32_t kf2;                       /* index into kf2s */
  float s12, R12[9], t12[3];
  int32_t* match12;                  /* [kf1->bow.n_keys] in / out */
  int32_t n_found;                   /* out: the return value */
  int32_t reserved;
} vieo_sim3_visit;                   /* 72 bytes */
/* VIEO_E_INVALID before anything is written or launched: a null pointer, n_cams outside 1..4 or not the same in all key
 * frames of the call, image bounds that differ between them (the grids are built in one launch), n_levels outside 1..16,
 * a key octave outside the levels, a camera index outside the rig, an unknown camera model, kf2 outside the table, a
 * match12 entry outside the candidate's keys.  VIEO_E_CAPACITY: a key frame with more than 8192 keys, more than 16384
 * visits. */
int vieo_search_by_sim3(const vieo_loop_keyframe* kf1, const vieo_loop_keyframe* kf2s, int n_kf2, vieo_sim3_visit* visits,
                        int n_visits, float th);
/* test tap: the device stage of the last vieo_search_by_sim3 of this thread -- per (visit, direction: 0 = kf1's points
 * into the candidate, 1 = back) best_idx / best_dist [n_points][n_cams] as vieo_fuse_search gives them, the index being
 * the key's index in the target key frame.  VIEO_E_EMPTY without such a call, VIEO_E_INVALID for a visit out of range. */
int vieo_search_by_sim3_tap(int visit, int direction, int32_t* best_idx, int32_t* best_dist);

/* ---- loop verification: int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale)
 * (src/Optimizer.cc:2689-2918) for a list of visits in one call: the whole of every visit -- both optimize() calls,
 * every lambda trial, both classifications -- in ONE kernel launch, one wavefront per visit.
 *   vertices: VertexNavStatePR mRwb = R12^-1, mpwb = -(mRwb t12) (retraction NavState::IncSmall: p += R dp, R <- R Exp(dphi))
 *           and VertexScale s12 (s += ds; fixed when fix_scale).  R12 makes the reference's quaternion round trip on the
 *           way in and out.
 *   host:   the correspondences.  match12[i] >= 0 with mp_id >= 0 on both sides; i2 = the SMALLEST key of the candidate that
 *           holds the map point of key match12[i] (GetIndexInKeyFrame is a std::set); P3D1c = R1w Xw1 + t1w and
 *           P3D2c = R2w Xw2 + t2w in float; observation = the key (mvKeysUn, or mvKeys when use_distort); information =
 *           inv_level_sigma2[octave]; camera = the key's own when use_distort, camera 0 otherwise, with Rcb / tcb =
 *           Tcr of that camera; Huber delta = (float)sqrt(th2).  MapPoint::isBad() is not represented: a map point is
 *           present exactly where mp_id >= 0, as for vieo_search_by_sim3.
 *   device: EdgeReprojectPRS (kf2's point into kf1 through S12) and EdgeReprojectPRSInv (kf1's point into kf2 through
 *           S12^-1) of src/Odom/g2otypes.h:321-549 as written there -- MODE 2 scales tcb by 1 / s, multiplies only the
 *           position block by -Rbw and forms the scale column as (J_s + Jproj tcw) (-scale^2) --, BaseMultiEdge's quadratic
 *           form with rho[1] only, g2o's Levenberg-Marquardt on the dense 7 x 7 (6 x 6) system, optimize(5), the erasure of
 *           every correspondence with chi2_12 > th2 || chi2_21 > th2, nMore = nBad > 0 ? 10 : 5, `return 0` when fewer
 *           than 10 are left (S12 stays the input, the first-round erasures stay in match12), optimize(nMore), the second
 *           erasure.  Both checks read the errors the last lambda trial left in the edges, accepted or not.
 * A visit without a correspondence returns 0 and nothing of it is written but the counters. */
typedef struct vieo_sim3_opt_visit {
  int32_t kf2;                       /* index into kf2s */
  int32_t reserved;
  double s12, R12[9], t12[3];        /* g2oS12, in / out (R12 row-major) */
  int32_t* match12;                  /* [kf1->bow.n_keys] in / out: erased correspondences become -1 */
  int32_t n_inliers;                 /* out: the return value */
  int32_t n_correspondences, n_bad;  /* out: nCorrespondences, nBad of the first check */
  int32_t iterations[2], trials[2];  /* out: per optimize() call, the iterations g2o ran and their lambda trials */
  int32_t reserved2;
} vieo_sim3_opt_visit;               /* 152 bytes */
#ifdef __cplusplus
static_assert(sizeof(vieo_sim3_opt_visit) == 152, "vieo_sim3_opt_visit");
#else
_Static_assert(sizeof(vieo_sim3_opt_visit) == 152, "vieo_sim3_opt_visit");
#endif
#define VIEO_SIM3_OPT_MAX_TRIALS 150 /* 5 x 10 + 10 x 10 lambda trials at most */
/* VIEO_E_INVALID before anything is written or launched: the grounds of vieo_search_by_sim3, a non-finite or non-positive
 * s12, a non-finite R12 / t12, th2 <= 0 or not finite.  VIEO_E_CAPACITY: a key frame with more than 8192 keys, more than
 * 16384 visits. */
int vieo_optimize_sim3(const vieo_loop_keyframe* kf1, const vieo_loop_keyframe* kf2s, int n_kf2, vieo_sim3_opt_visit* visits,
                       int n_visits, float th2, int fix_scale);
/* test tap: visit `visit` of the last vieo_optimize_sim3 of this thread.  *n_trials and trials[n_trials][4] = per lambda
 * trial (chi2 before, chi2 after, lambda, accepted) -- room for VIEO_SIM3_OPT_MAX_TRIALS rows --; *n_corr, corr_i1[n_corr]
 * = the key of kf1 of every correspondence; chi2[2][n_corr][2] = (chi2_12, chi2_21) as read at the first and at the second
 * check (zeros where a check did not read: erased before, or the call returned 0).  Any pointer may be NULL.
 * VIEO_E_EMPTY without such a call, VIEO_E_INVALID for a visit out of range. */
int vieo_optimize_sim3_trace(int visit, int32_t* n_trials, double* trials, int32_t* n_corr, int32_t* corr_i1, double* chi2);

/* ---- loop closing: the two projection searches that take a Sim3 world pose Scw, each for a list of visits (key frame,
 * Scw) in one call over ONE table of loop map points shared by all visits: points[n_points] with point_id[n_points].
 * point_id lives in the id space of mp_id (equal id = the same MapPoint*, every id >= 0); bit 31 of a point's skip_mask
 * is isBad(), its other bits are not read.  isBad() of a key frame's own map point is not represented: a key holds a
 * point exactly where mp_id >= 0.  Scw is the reference's cv::Mat, 3 x 4 float, row-major: s R | t.
 *
 * Device, shared by both (arithmetic in float as SearchByProjectionBase, see vieo_fuse_search): all key frames resident
 * side by side with one grid per (key frame, camera), as for vieo_search_by_sim3; then TWO launches over the items
 * (visit, point, camera): the gates -- positive depth, IsInImage, the 0.8 / 1.2 distance test, the 60 degree viewing cone,
 * PredictScale, the radius -- one lane per item, the survivors compacted; then one wavefront per survivor for its window.
 * The order of the survivors is not fixed, every output is addressed by item: equal input gives byte-identical output.
 * VIEO_E_INVALID before anything is written or launched (the previous call's tap stays): the grounds of
 * vieo_search_by_sim3 (all key frames of the call against kfs[0]), a visit whose kf is outside the table, a null table
 * with n_points > 0, a negative point_id, n_visits < 0, th <= 0, a non-finite Scw or one whose first row is zero.
 * VIEO_E_CAPACITY: a key frame with more than 8192 keys, more than 16384 visits, n_points x n_visits > 2^20 (the survivor
 * records are sized for every item passing: 24 bytes x n_points x n_visits x n_cams).
 *
 * int ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:507-626).
 *   host, Eigen float as :510-515: scw = sqrtf((r00 r00 + r01 r01) + r02 r02); Rcrw = sRcw / scw and tcrw = t / scw by
 *           float division; twcr = -(Rcrw^T tcrw), every row times column summed left to right.  The camera centre behind
 *           PO is that twcr (+ Rcrw^T trc), NOT the record's Ow.  spAlreadyFound = the ids >= 0 in `matched` at entry: a
 *           point whose id is in it, or whose bit 31 is set, is not searched (:528).  A `matched` entry is only compared:
 *           any value >= 0 counts as a map point (it needs to be no id of the table), any value < 0 as NULL.
 *   device: the gates, then per surviving item the LIST of every window key in [level - 1, level] with Hamming distance
 *           <= TH_LOW (50), in the reference's candidate order.  The list is exact: the window is walked twice (count,
 *           reserve with one atomic, fill); if the pool is too small the call reads the exact total, grows the pool and
 *           repeats the window launch.  (VIEO_SCW_POOL=<entries>, read at every call, pins the first pool size: tests.)
 *   host, after the copy back, :524-623 in the reference's order -- points ascending, cameras ascending: the smallest
 *           distance among the item's listed keys with matched[key] < 0 (the earlier candidate on equal distance) gets
 *           matched[key] = point_id and counts; an item whose listed keys are all taken matches nothing.  (The reference
 *           tests vpMatched[idx] inside its candidate loop: a key further than 50 can never be taken, so the list is all
 *           that loop can choose from.) */
typedef struct vieo_scw_visit {
  int32_t kf;          /* index into kfs */
  float Scw[12];
  int32_t* matched;    /* [kfs[kf].bow.n_keys] in / out: vpMatched as point ids, < 0 = NULL */
  int32_t n_matches;   /* out: the return value */
} vieo_scw_visit;      /* 72 bytes */
int vieo_search_by_projection_scw(const vieo_loop_keyframe* kfs, int n_kf, const vieo_fuse_point* points,
                                  const int32_t* point_id, int n_points, vieo_scw_visit* visits, int n_visits,
                                  float th);
/* test tap: the device stage of visit `visit` of the last vieo_search_by_projection_scw of this thread.  count[n_points]
 * [n_cams] = listed candidates per item (0 for an item that was not searched or did not pass a gate); with cap > 0,
 * key / dist / order [n_points][n_cams][cap] = the first min(count, cap) of them in candidate order: the key frame's key,
 * the Hamming distance, the key's position in the walk over ALL keys of the window's cells (GetFeaturesInArea's loops,
 * before its distance test: ascending along the reference's candidate order).  Any pointer may be NULL.  VIEO_E_EMPTY without
 * such a call, VIEO_E_INVALID for a visit out of range. */
int vieo_search_by_projection_scw_tap(int visit, int32_t* count, int32_t* key, int32_t* dist, int32_t* order, int cap);

/* int ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:1167-1220) for every
 * key frame of a LoopClosing::SearchAndFuse (src/LoopClosing.cc:682-707) in one call.
 *   host, cv::Mat as :1170-1173 -- ASSUMED OpenCV arithmetic, stated from memory (no OpenCV where this was written):
 *           Mat::dot of CV_32F accumulates the exact products in double, ((r00 r00 + r01 r01) + r02 r02), sqrt in double,
 *           the result rounded to float = scw; Mat / scalar multiplies by the double reciprocal 1.0 / (double)scw and
 *           rounds every element to float once.  The camera centre behind PO is the record's Ow (GetCameraCenter(), :42).
 *           vbAlreadyMatched1 AS WRITTEN at :1177-1187: the camera looked up for point iMP is that of KEY index iMP,
 *           cam_of_key[iMP], or 0 when iMP >= n_keys; if a key of that camera holds point_id[iMP], that one camera is
 *           skipped for the point.  (The index of a loop point is used as a key index there; restated, not repaired.)
 *   device: the gates with the viewing cone, then per survivor the best key as vieo_fuse_search gives it: pbf = nullptr,
 *           no IsInKeyFrame skip (fuselater), every camera on its own (MatchMultiCam).
 *   host, :193-203 and :1193-1217: a best distance <= TH_LOW enters the point's set (match_key); points ascending and the
 *           keys of a set ascending: a key that holds a point sets replace[iMP] to that id (a later key of the set
 *           overwrites it), a free key is marked `added` (AddObservation / AddMapPoint) and holds the loop point for the
 *           rest of THIS visit; n_fused counts both.
 * One visit is the reference's Fuse exactly.  Several visits in one call are all searched with the tables as given at
 * the call and each classified against its own key frame's mp_id at the call: what pRep->Replace(loopMP) after key
 * frame k changes in later key frames' mvpMapPoints, and the descriptor MapPoint::Replace ->
 * ComputeDistinctiveDescriptors (src/MapPoint.cc:245-291) may give a loop point before key frame k + 1 is searched, are
 * not seen.  A caller who wants the reference's sequence calls with one visit at a time; Replace and the map stay the
 * caller's. */
typedef struct vieo_fuse_scw_visit {
  int32_t kf;          /* index into kfs */
  float Scw[12];
  int32_t* match_key;  /* out [n_points][n_cams]: vnMatch as the best key per camera, -1 none */
  int32_t* replace;    /* out [n_points]: vpReplacePoint as the id the key frame's key held, -1 NULL */
  uint8_t* added;      /* out [n_points][n_cams]: 1 where the reference adds the loop point at match_key */
  int32_t n_fused;     /* out: the return value */
  int32_t reserved;
} vieo_fuse_scw_visit; /* 88 bytes */
int vieo_fuse_scw(const vieo_loop_keyframe* kfs, int n_kf, const vieo_fuse_point* points, const int32_t* point_id,
                  int n_points, vieo_fuse_scw_visit* visits, int n_visits, float th);
/* test tap: best_idx (the key frame's key, -1) / best_dist (INT_MAX) [n_points][n_cams] of visit `visit` of the last
 * vieo_fuse_scw of this thread, before the threshold. */
int vieo_fuse_scw_tap(int visit, int32_t* best_idx, int32_t* best_dist);
/* (visit, point, camera) items and gate survivors of the last vieo_search_by_projection_scw or vieo_fuse_scw of this
 * thread.  VIEO_E_EMPTY without such a call. */
int vieo_scw_gate_stats(int64_t* n_items, int64_t* n_survivors);

/* ---- bool LoopClosing::ComputeSim3() (src/LoopClosing.cc:308-444) up to bMatch, as ONE call: host code around the
 * library's own entries.  kf1 = mpCurrentKF, cands = mvpEnoughConsistentCandidates without the bad ones, both as
 * vieo_loop_keyframe with bow.node_* filled; thresh_matches / min_inliers = the thresh_matches_ / thresh_inliers_ entry the
 * caller picked; samples [n_cands][n_rows][3] / n_rows / seed as for vieo_sim3_create (a row's indices count the
 * correspondences of ITS candidate as listed below; NULL: the library draws).
 *   1. vieo_search_by_bow_kf(0.75, orientation on) of all candidates; nmatches < thresh_matches discards a candidate.
 *   2. the Sim3Solver constructor (src/Sim3Solver.cc:22-116) from the records: for every key i1 of kf1, ascending, with
 *      mp_id >= 0 and a matched candidate key whose mp_id >= 0, one correspondence per candidate key that holds that
 *      map point, ascending; X = Rcw Xw + tcw in float, every row times column summed left to right; max_err =
 *      (size_t)(9.210 * level_sigma2[octave]) with the product in double; cameras = the rig with Tcr in Rcb / tcb and the
 *      key's own camera when use_distort, else one pinhole (camera 0's fx, fy, cx, cy) with the identity and camera 0.
 *      Then vieo_sim3_create with (0.99, min_inliers, 300).
 *   3. the while of :368-432.  The visits of one pass over the candidates do not depend on one another (each works on a
 *      fresh copy of its vvpMapPointMatches[i] masked by the inlier flags), so a pass is vieo_sim3_iterate(5) of every
 *      live candidate, ONE vieo_search_by_sim3 (th 7.5) and ONE vieo_optimize_sim3 (th2 10) over the visits that returned
 *      a Sim3, and then the first visit in candidate order with nInliers >= 20 wins; the visits behind it in that pass,
 *      which the reference never makes, are dropped.  bNoMore discards as at :385-389; a used-up sample table discards
 *      the same way and is reported as no_more = 2.
 *   4. on a match mg2oScw = gScm * gSmw (:422-425) in double: R = R12 R2w, t = s12 (R12 t2w) + t12, s = s12 (gSmw has
 *      scale 1; g2o multiplies unit quaternions, here the rotation matrices are multiplied, row times column summed left
 *      to right); Scw = mScw, every element of s R | t rounded to float; match12[n_keys1] = mvpCurrentMatchedPoints as the
 *      matched candidate's key (-1: NULL).  Without a match: found = 0, cand = -1, match12 all -1.
 * trace: one line per candidate for step 1 (call 0, n_inliers = nmatches, no_more = 1 where it is discarded), then one
 * per visit of the while in the reference's order.  VIEO_E_CAPACITY when the trace holds fewer than n_visits lines, with
 * every other output complete.  VIEO_E_INVALID (nothing written): a null pointer, n_cands <= 0, n_rows outside 1..512,
 * min_inliers < 3, a key frame with a null array, n_levels outside 1..16, an octave or a camera index out of range; and
 * whatever the entries it calls refuse.  The loop points of :446-463 come from the map: the final search is the caller's
 * second call, vieo_search_by_projection_scw with Scw and match12 turned into ids, and so is nTotalMatches >= 40. */
typedef struct vieo_compute_sim3_visit {
  int32_t cand, call;      /* candidate; 0 = the SearchByBoW line, k = its k-th iterate(5) */
  int32_t row;             /* the sample row iterate returned, -1 */
  int32_t no_more, found;  /* bNoMore (2: sample table used up), !Scm.empty() */
  int32_t n_inliers;       /* of the RANSAC (call 0: nmatches of SearchByBoW) */
  int32_t n_found;         /* SearchBySim3's return value, -1 when it was not called */
  int32_t n_opt_inliers;   /* OptimizeSim3's return value, -1 when it was not called */
} vieo_compute_sim3_visit; /* 32 bytes */
typedef struct vieo_compute_sim3_result {
  int32_t found, cand;     /* bMatch, the index of mpMatchedKF in cands (-1) */
  int32_t n_inliers;       /* OptimizeSim3's nInliers of the match */
  int32_t n_visits;        /* trace lines the call produced */
  double s, R[9], t[3];    /* mg2oScw */
  float Scw[12];           /* mScw, 3 x 4 row-major */
} vieo_compute_sim3_result; /* 168 bytes */
int vieo_compute_sim3(const vieo_loop_keyframe* kf1, const vieo_loop_keyframe* cands, int n_cands, int thresh_matches,
                      int min_inliers, int fix_scale, const int32_t* samples, int n_rows, uint64_t seed,
                      vieo_compute_sim3_result* result, int32_t* match12, vieo_compute_sim3_visit* trace,
                      int32_t trace_capacity);
#ifdef __cplusplus
static_assert(sizeof(vieo_compute_sim3_visit) == 32 && sizeof(vieo_compute_sim3_result) == 168, "vieo_compute_sim3");
#else
_Static_assert(sizeof(vieo_compute_sim3_visit) == 32 && sizeof(vieo_compute_sim3_result) == 168, "vieo_compute_sim3");
#endif
#ifdef __cplusplus
static_assert(sizeof(vieo_scw_visit) == 72 && sizeof(vieo_fuse_scw_visit) == 88, "vieo_scw_visit");
#else
_Static_assert(sizeof(vieo_scw_visit) == 72 && sizeof(vieo_fuse_scw_visit) == 88, "vieo_scw_visit");
#endif

/* ---------------------------------------------------------------- monocular initialisation: the matcher ----
 * int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vbPrevMatched, vnMatches12, windowSize)
 * (src/ORBmatcher.cc:628-723) for n_pairs independent pairs (F1, F2) in one call: the first step of
 * Tracking::MonocularInitialization (src/Tracking.cc:1481-1544) of every sequence that is initialising.
 *   input:  keys1 / keys2 = mvKeysUn of both frames (neither frame uses distortion, :631,638), desc1 / desc2 their
 *           descriptor rows, prev_matched[i1] = vbPrevMatched[i1] (x, y), window_size = windowSize; bounds[4] =
 *           gridinfo_.minmax_xy_[0] (min x, max x, min y, max y) of the second frames' grid, ONE for the call;
 *           nn_ratio = mfNNratio (0.9 in MonocularInitialization), check_orientation = mbCheckOrientation (true there).
 *   device: the 64 x 48 grid of every second frame (FrameBase::AssignFeaturesToGrid), then per octave-0 key of a
 *           first frame, one wavefront: the window GetFeaturesInArea(0, x, y, windowSize, 0, 0) of ITS pair's second
 *           frame in the reference's cell order -- octave 0 only, |dx| < r and |dy| < r -- the Hamming distance of
 *           every candidate, and the LIST of the candidates with distance <= cut in that order, where
 *           cut = max(TH_LOW, the largest d with (float)d * nn_ratio <= 50.f) (55 for 0.9).  A candidate beyond cut can
 *           be neither a best (:676 asks bestDist <= TH_LOW) nor a second best that fails :677 for any bestDist <= 50:
 *           56 * 0.9f = 50.399998 > 50.  The list is exact: the window is walked twice (count, reserve with one atomic,
 *           fill); if the pool is too small the call reads the exact total, grows the pool and repeats the launch.
 *           (VIEO_INIT_POOL=<entries>, read at every call, pins the first pool size: tests.)
 *   host, after the copy back, :642-722 in the reference's order over the lists: the vMatchedDistance[i2] <= dist skip,
 *           best / second best (the earlier candidate on equal distance), the steal of a key that an earlier i1 holds,
 *           the rotation histogram (a stolen match stays counted in its bin, as rotHist keeps the entry) with
 *           ComputeThreeMaxima, and vbPrevMatched[i1] = the matched key's position for every surviving match.
 * Every output equals the reference's bit for bit.  VIEO_E_INVALID before anything is written: a null pointer, a
 * negative count or window, bounds empty or not finite, nn_ratio <= 0, a prev_matched that is not finite, a key with a
 * negative octave (second frame: above 32767) or an angle outside [0, 360), a second-frame key at a non-finite position.
 * VIEO_E_CAPACITY: more than 4096 pairs, a frame with more than 8192 keys, more than 2^27 listed candidates.
 * n_pairs == 0 is VIEO_OK. */
typedef struct vieo_init_pair {
  const vieo_keypoint* keys1;  /* [n1] F1.mvKeysUn */
  const uint8_t* desc1;        /* [n1][32] */
  const vieo_keypoint* keys2;  /* [n2] F2.mvKeysUn */
  const uint8_t* desc2;        /* [n2][32] */
  float* prev_matched;         /* [n1][2] in / out: vbPrevMatched */
  int32_t* matches12;          /* [n1] out: vnMatches12, -1 none */
  int32_t n1, n2;
  int32_t window_size;
  int32_t n_matches;           /* out: the return value */
} vieo_init_pair;              /* 64 bytes */
int vieo_search_for_initialization(vieo_init_pair* pairs, int n_pairs, const float* bounds, float nn_ratio,
                                   int check_orientation);
/* test tap: the device stage of pair `pair` of the last vieo_search_for_initialization of this thread.  count[n1] =
 * listed candidates per key of the first frame (0 for a key above octave 0); with cap > 0, key / dist / order [n1][cap] =
 * the first min(count, cap) of them in candidate order: the second frame's key, the Hamming distance, the key's
 * position in the walk over ALL keys of the window's cells (GetFeaturesInArea's loops, before its octave and distance
 * tests).  Any pointer may be NULL.  VIEO_E_EMPTY without such a call, VIEO_E_INVALID for a pair out of range. */
int vieo_search_for_initialization_tap(int pair, int32_t* count, int32_t* key, int32_t* dist, int32_t* order, int cap);
#ifdef __cplusplus
static_assert(sizeof(vieo_init_pair) == 64, "vieo_init_pair");
#else
_Static_assert(sizeof(vieo_init_pair) == 64, "vieo_init_pair");
#endif

#ifdef __cplusplus
}
#endif
#endif /* VIEO_HOT_H */
