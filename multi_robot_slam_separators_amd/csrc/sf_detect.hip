// sf_detect.hip -- the five corner detectors' entry points, what the extraction calls do around a detector (Vis/RoiRatios, the
// grid of cells, sub-pixel refinement: parameters and plans) and the two stereo correspondence calls.
#include <cmath>

#include "sf_host.hpp"

int sf_check_gftt(sf_context* c, double quality_level, double min_distance) {
  if (!(quality_level > 0.0) || !(min_distance >= 0.0))
    return sf_fail(c, SF_EINVAL, "qualityLevel must be > 0 and minDistance >= 0 (cv::goodFeaturesToTrack asserts the same)");
  return SF_OK;
}

// ---- GFTT/BlockSize, GFTT/UseHarrisDetector, GFTT/K: the response of k_gftt.hip, handle state as the FAST parameters are ----
extern "C" void sf_gftt_defaults(sf_gftt_params* p) {
  if (!p) return;
  p->block_size = 3;           // GFTT/BlockSize [upstream rtabmap Parameters.h]
  p->use_harris_detector = 0;  // GFTT/UseHarrisDetector
  p->k = 0.04;                 // GFTT/K
}

int sf_gftt_validate(sf_context* c, const sf_gftt_params& g) {
  if (g.block_size == 1)
    return sf_fail(c, SF_EINVAL, "GFTT block_size 1: the response of a single product is rounding noise (2 .. 15)");
  if (g.block_size < 1) return sf_fail(c, SF_EINVAL, "GFTT block_size %d outside 2 .. 15", g.block_size);
  if (g.block_size > 15) return sf_fail(c, SF_EINVAL, "GFTT block_size %d is not built (2 .. 15)", g.block_size);
  if (g.use_harris_detector != 0 && g.use_harris_detector != 1)
    return sf_fail(c, SF_EINVAL, "GFTT use_harris_detector %d is neither 0 nor 1", g.use_harris_detector);
  if (!std::isfinite(g.k) || g.k < 0.0 || g.k > 1.0) return sf_fail(c, SF_EINVAL, "GFTT k %g: finite, 0 <= k <= 1", g.k);
  return SF_OK;
}

// the same ranges without a handle (sf_experimental.h; NULL = the defaults)
extern "C" int sf_gftt_check_params(const sf_gftt_params* params) { return sf_gftt_validate(nullptr, arg_or_defaults(params, sf_gftt_defaults)); }

extern "C" int sf_gftt_set_params(sf_handle c, const sf_gftt_params* params) {
  if (!c || !params) return SF_EINVAL;
  int rc = sf_gftt_validate(c, *params);
  if (rc != SF_OK) return rc;
  c->gftt = *params;
  return SF_OK;
}

extern "C" int sf_gftt_get_params(sf_handle c, sf_gftt_params* params) { return get_block(c, params, &sf_context::gftt); }

int sf_check_gftt_side(sf_context* c, int width, int height, const char* what) {
  const int b = c->gftt.block_size;
  if (width < b || height < b)
    return sf_fail(c, SF_EINVAL, "GFTT block_size %d needs %s of at least %d x %d, not %d x %d", b, what, b, b, width, height);
  return SF_OK;
}

extern "C" void sf_detector_defaults(sf_detector_params* p) {
  if (!p) return;
  p->max_features = 1000;      // Vis/MaxFeatures [upstream rtabmap Parameters.h]; the reference sets only Vis/MinInliers
  p->quality_level = 0.001;    // GFTT/QualityLevel
  p->min_distance = 3.0;       // GFTT/MinDistance
}

// ---- the five detectors: detect_prologue, the call's own parameters, detect_ready, the launch -----------------------------
static int detect_prologue(sf_context* c, const uint8_t* d_image, int width, int height, int pitch, const sf_keypoint* d_kpts_out,
                           int cap, int32_t* n_out) {
  if (!c || !n_out || cap < 0 || (cap > 0 && !d_kpts_out)) return SF_EINVAL;
  *n_out = 0;
  return sf_check_image(c, d_image, width, height, pitch, 3, "image");
}

// validated: what the call's check of its own parameters gave; integral: the detector reads an integral image (SURF)
static int detect_ready(sf_context* c, int validated, int width, int height, bool integral = false) {
  int rc = validated;
  if (rc != SF_OK || (rc = sf_check_pixels(c, width, height)) != SF_OK) return rc;
  if (integral && (rc = sf_check_integral(c, width, height)) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  return SF_OK;
}

// Each entry point runs its detector's launcher on ONE image (d_kpts_out [1][cap], the count in a device word of the
// handle's) and brings to the host what it returns: the keypoint count, read behind the last kernel (GFTT, FAST, ORB: the
// call returns with its keypoints written, as it always has), or what came with the one wait of the image's sort
// (SfDetectOne; SURF, SIFT: the candidate counts, from which the refusal and the keypoint count follow).
static int single_count_word(sf_context* c, int32_t** d_n) {
  const int rc = sf_buf_reserve(c, c->ft_counts, sizeof(int32_t));
  *d_n = (int32_t*)c->ft_counts.p;
  return rc;
}

static int detect_corners_one(sf_context* c, const uint8_t* d_image, int width, int height, int pitch, int max_corners,
                              double quality_level, double min_distance, sf_keypoint* d_kpts_out, int cap, int32_t* n_out,
                              const SfMask& mask) {
  int32_t* d_n = nullptr;
  int rc;
  if ((rc = single_count_word(c, &d_n)) != SF_OK) return rc;
  if ((rc = sf_launch_detect_corners(c, d_image, 0, 1, width, height, pitch, max_corners, quality_level, min_distance, d_kpts_out,
                                     cap, d_n, SfCells(), mask)) != SF_OK)
    return rc;
  return sf_word_to_host(c, d_n, n_out);                 // (the selection decides it: minDistance drops candidates)
}

static int detect_fast_one(sf_context* c, const uint8_t* d_image, int width, int height, int pitch, int max_features,
                           const sf_fast_params& prm, sf_keypoint* d_kpts_out, int cap, int32_t* n_out, const SfMask& mask) {
  int32_t* d_n = nullptr;
  int rc;
  if ((rc = single_count_word(c, &d_n)) != SF_OK) return rc;
  if ((rc = sf_launch_detect_fast(c, d_image, 0, 1, width, height, pitch, max_features, &prm, d_kpts_out, cap, d_n, SfCells(),
                                  mask)) != SF_OK)
    return rc;
  return sf_word_to_host(c, d_n, n_out);
}

extern "C" int sf_detect_corners_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                        int32_t max_corners, double quality_level, double min_distance,
                                        sf_keypoint* d_kpts_out, int32_t cap, int32_t* n_out) {
  int rc;
  if ((rc = detect_prologue(c, d_image, width, height, pitch, d_kpts_out, cap, n_out)) != SF_OK) return rc;
  if ((rc = sf_check_gftt_side(c, width, height, "an image")) != SF_OK) return rc;
  if ((rc = detect_ready(c, sf_check_gftt(c, quality_level, min_distance), width, height)) != SF_OK) return rc;
  return detect_corners_one(c, d_image, width, height, pitch, max_corners, quality_level, min_distance, d_kpts_out, cap, n_out,
                            SfMask());
}

extern "C" int sf_detect_fast_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                     int32_t max_features, const sf_fast_params* params, sf_keypoint* d_kpts_out,
                                     int32_t cap, int32_t* n_out) {
  int rc;
  if ((rc = detect_prologue(c, d_image, width, height, pitch, d_kpts_out, cap, n_out)) != SF_OK) return rc;
  const sf_fast_params prm = params ? *params : c->fast;
  if ((rc = detect_ready(c, sf_fast_validate(c, prm), width, height)) != SF_OK) return rc;
  return detect_fast_one(c, d_image, width, height, pitch, max_features, prm, d_kpts_out, cap, n_out, SfMask());
}

// ---- the two corner detectors under a mask (cv's `mask` argument; Vis/DepthAsMask makes one of a depth image) --------------
static int check_mask(sf_context* c, const char* call, const uint8_t* d_mask, int width, int mask_pitch) {
  if (!d_mask || mask_pitch < width) return sf_fail(c, SF_EINVAL, "%s: mask missing or malformed (width %d, mask_pitch %d)", call, width, mask_pitch);
  return SF_OK;
}

static SfMask single_mask(const uint8_t* d_mask, int mask_pitch) {
  SfMask m;
  m.p = d_mask; m.pitch = mask_pitch;
  return m;
}

extern "C" int sf_detect_corners_masked_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                               const uint8_t* d_mask, int32_t mask_pitch, int32_t max_corners,
                                               double quality_level, double min_distance, sf_keypoint* d_kpts_out, int32_t cap,
                                               int32_t* n_out) {
  int rc;
  if ((rc = detect_prologue(c, d_image, width, height, pitch, d_kpts_out, cap, n_out)) != SF_OK) return rc;
  if ((rc = check_mask(c, "sf_detect_corners_masked_device", d_mask, width, mask_pitch)) != SF_OK) return rc;
  if ((rc = sf_check_gftt_side(c, width, height, "an image")) != SF_OK) return rc;
  if ((rc = detect_ready(c, sf_check_gftt(c, quality_level, min_distance), width, height)) != SF_OK) return rc;
  return detect_corners_one(c, d_image, width, height, pitch, max_corners, quality_level, min_distance, d_kpts_out, cap, n_out,
                            single_mask(d_mask, mask_pitch));
}

extern "C" int sf_detect_fast_masked_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                            const uint8_t* d_mask, int32_t mask_pitch, int32_t max_features,
                                            const sf_fast_params* params, sf_keypoint* d_kpts_out, int32_t cap, int32_t* n_out) {
  int rc;
  if ((rc = detect_prologue(c, d_image, width, height, pitch, d_kpts_out, cap, n_out)) != SF_OK) return rc;
  if ((rc = check_mask(c, "sf_detect_fast_masked_device", d_mask, width, mask_pitch)) != SF_OK) return rc;
  const sf_fast_params prm = params ? *params : c->fast;
  if ((rc = detect_ready(c, sf_fast_validate(c, prm), width, height)) != SF_OK) return rc;
  return detect_fast_one(c, d_image, width, height, pitch, max_features, prm, d_kpts_out, cap, n_out, single_mask(d_mask, mask_pitch));
}

// ---- depth images (kernels in k_depth.hip): Vis/DepthAsMask as handle state, the mask and the 3D points as calls --------------
extern "C" void sf_depth_defaults(sf_depth_params* p) {
  if (!p) return;
  p->depth_as_mask = 1;        // Vis/DepthAsMask [upstream rtabmap Parameters.h]
}

extern "C" int sf_depth_set_params(sf_handle c, const sf_depth_params* params) {
  if (!c || !params) return SF_EINVAL;
  if (params->depth_as_mask != 0 && params->depth_as_mask != 1)
    return sf_fail(c, SF_EINVAL, "Vis/DepthAsMask %d is neither 0 nor 1", params->depth_as_mask);
  c->depth = *params;
  return SF_OK;
}

extern "C" int sf_depth_get_params(sf_handle c, sf_depth_params* params) { return get_block(c, params, &sf_context::depth); }

extern "C" int sf_depth_set_size(sf_handle c, const sf_depth_size* size) {
  if (!c) return SF_EINVAL;
  const sf_depth_size v = size ? *size : sf_depth_size{0, 0};
  if (!((v.depth_width == 0 && v.depth_height == 0) || (v.depth_width >= 1 && v.depth_height >= 1)))
    return sf_fail(c, SF_EINVAL, "sf_depth_set_size: %d x %d is neither {0, 0} (the image's size) nor a size", v.depth_width, v.depth_height);
  c->depth_size = v;
  return SF_OK;
}

extern "C" int sf_depth_get_size(sf_handle c, sf_depth_size* out) { return get_block(c, out, &sf_context::depth_size); }

// myRegistrationVis.cpp:274-276: the factor by which a depth image divides the image, both ways alike; 0: it does not
extern "C" int sf_depth_interpolation_factor(int32_t width, int32_t height, int32_t depth_width, int32_t depth_height) {
  if (width < 1 || height < 1 || depth_width < 1 || depth_height < 1) return 0;
  if (height % depth_height != 0 || width % depth_width != 0 || height / depth_height != width / depth_width) return 0;
  return height / depth_height;
}

// what every depth call refuses of its depth images (`call` opens the message): n images of width x height, `stride` bytes apart
static int sf_check_depth(sf_context* c, const char* call, bool present, int format, int width, int height, int pitch, size_t stride, int n) {
  if (format != SF_DEPTH_U16_MM && format != SF_DEPTH_F32_M)
    return sf_fail(c, SF_EINVAL, "%s: depth format %d unknown (0 = uint16 millimetres, 1 = float32 metres)", call, format);
  const int elem = format == SF_DEPTH_F32_M ? 4 : 2;
  if (!present || width < 1 || height < 1) return sf_fail(c, SF_EINVAL, "%s: depth image missing or malformed (%d x %d)", call, width, height);
  if ((long long)pitch < (long long)elem * width)
    return sf_fail(c, SF_EINVAL, "%s: depth_pitch %d is less than a row of %d pixels of %d bytes", call, pitch, width, elem);
  if (pitch % elem) return sf_fail(c, SF_EINVAL, "%s: depth_pitch %d is no multiple of the %d bytes of a pixel", call, pitch, elem);
  if (n > 1) {
    if (stride % (size_t)elem) return sf_fail(c, SF_EINVAL, "%s: depth stride %zu is no multiple of the %d bytes of a pixel", call, stride, elem);
    if (stride < (size_t)pitch * (height - 1) + (size_t)elem * width)
      return sf_fail(c, SF_EINVAL, "%s: depth stride %zu is less than an image (%d rows of pitch %d)", call, stride, height, pitch);
  }
  return SF_OK;
}

int sf_depth_in(sf_context* c, const char* call, SfDepthIn* D, int width, int height, int n) {
  if (n == 0) return sf_check_depth(c, call, true, D->format, 1, 1, 4, 0, 0);   // (the format alone)
  const sf_depth_size& s = c->depth_size;
  D->w = s.depth_width ? s.depth_width : width;
  D->h = s.depth_height ? s.depth_height : height;
  if (D->w > width || D->h > height)
    return sf_fail(c, SF_EINVAL, "%s: a depth image of %d x %d (sf_depth_set_size) larger than the %d x %d image is not built", call,
                   D->w, D->h, width, height);
  return sf_check_depth(c, call, D->p != nullptr, D->format, D->w, D->h, D->pitch, D->stride, n);
}

extern "C" int sf_depth_mask_device(sf_handle c, const void* d_depth, int32_t depth_format, int32_t width, int32_t height,
                                    int32_t depth_pitch, size_t depth_stride, int32_t n_images, float min_depth, float max_depth,
                                    uint8_t* d_mask, int32_t mask_pitch, size_t mask_stride) {
  if (!c || n_images < 0) return SF_EINVAL;
  SfDepthIn D;
  D.p = d_depth; D.format = depth_format; D.pitch = depth_pitch; D.stride = n_images > 1 ? depth_stride : 0;
  int rc = sf_depth_in(c, "sf_depth_mask_device", &D, width, height, n_images);
  if (rc != SF_OK || n_images == 0) return rc;
  if (sf_depth_interpolation_factor(width, height, D.w, D.h) == 0)
    return sf_fail(c, SF_EINVAL, "sf_depth_mask_device: a depth image of %d x %d (sf_depth_set_size) does not divide the %d x %d image: "
                   "no mask (the depth keyframe calls run their detector without one)", D.w, D.h, width, height);
  if (n_images > 65535) return sf_fail(c, SF_ERANGE, "sf_depth_mask_device: %d images (at most 65535 per call)", n_images);
  if (!d_mask || mask_pitch < width) return sf_fail(c, SF_EINVAL, "sf_depth_mask_device: mask missing or malformed (width %d, mask_pitch %d)", width, mask_pitch);
  if (n_images > 1 && mask_stride < (size_t)mask_pitch * (height - 1) + (size_t)width)
    return sf_fail(c, SF_EINVAL, "sf_depth_mask_device: mask stride %zu is less than a plane (%d rows of pitch %d)", mask_stride, height, mask_pitch);
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_depth_mask(c, D, n_images, width, height, min_depth, max_depth, d_mask, mask_pitch, n_images > 1 ? mask_stride : 0);
}

extern "C" int sf_depth_points_device(sf_handle c, const void* d_depth, int32_t depth_format, int32_t width, int32_t height,
                                      int32_t depth_pitch, const sf_keypoint* d_kpts, int32_t n, const sf_stereo_camera* cam,
                                      float* d_xyz_out, uint8_t* d_valid_out) {
  if (!c || !cam || n < 0) return SF_EINVAL;
  SfDepthIn D;
  D.p = d_depth; D.format = depth_format; D.pitch = depth_pitch;
  int rc = sf_depth_in(c, "sf_depth_points_device", &D, width, height, 1);
  if (rc != SF_OK) return rc;
  if (n > 0 && (!d_kpts || !d_xyz_out)) return sf_fail(c, SF_EINVAL, "sf_depth_points_device: keypoints or output array missing");
  if (n == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_depth_points_only(c, D, width, height, d_kpts, n, cam, d_xyz_out, d_valid_out);
}

extern "C" int sf_depth_interpolate_device(sf_handle c, const void* d_depth, int32_t depth_format, int32_t depth_width,
                                           int32_t depth_height, int32_t depth_pitch, size_t depth_stride, int32_t n_images,
                                           int32_t factor, void* d_out, int32_t out_pitch, size_t out_stride) {
  static const char* const call = "sf_depth_interpolate_device";
  if (!c || n_images < 0) return SF_EINVAL;
  if (n_images == 0) return sf_check_depth(c, call, true, depth_format, 1, 1, 4, 0, 0);   // (the format alone)
  int rc = sf_check_depth(c, call, d_depth, depth_format, depth_width, depth_height, depth_pitch, depth_stride, n_images);
  if (rc != SF_OK) return rc;
  if (factor < 1) return sf_fail(c, SF_EINVAL, "%s: factor %d is below 1", call, factor);
  if (n_images > 65535) return sf_fail(c, SF_ERANGE, "%s: %d images (at most 65535 per call)", call, n_images);
  const long long ow = (long long)depth_width * factor, oh = (long long)depth_height * factor;
  if (ow > 262140 || oh > 262140) return sf_fail(c, SF_ERANGE, "%s: an enlarged image of %lld x %lld pixels (at most 262140 a side)", call, ow, oh);
  const int elem = depth_format == SF_DEPTH_F32_M ? 4 : 2;
  if (((uintptr_t)d_depth | (uintptr_t)d_out) % (uintptr_t)elem)
    return sf_fail(c, SF_EINVAL, "%s: an image address is no multiple of the %d bytes of a pixel", call, elem);
  // the enlarged images: what the input's own checks ask of a pitch and a stride, under the output's name
  if (!d_out || (long long)out_pitch < elem * ow)
    return sf_fail(c, SF_EINVAL, "%s: output missing or out_pitch %d less than a row of %lld pixels of %d bytes", call, out_pitch, ow, elem);
  if (out_pitch % elem) return sf_fail(c, SF_EINVAL, "%s: out_pitch %d is no multiple of the %d bytes of a pixel", call, out_pitch, elem);
  if (n_images > 1) {
    if (out_stride % (size_t)elem) return sf_fail(c, SF_EINVAL, "%s: output stride %zu is no multiple of the %d bytes of a pixel", call, out_stride, elem);
    if (out_stride < (size_t)out_pitch * (size_t)(oh - 1) + (size_t)(elem * ow))
      return sf_fail(c, SF_EINVAL, "%s: output stride %zu is less than an image (%lld rows of pitch %d)", call, out_stride, oh, out_pitch);
  }
  SF_HIP(c, hipSetDevice(c->device));
  SfDepthIn D;
  D.p = d_depth; D.format = depth_format; D.pitch = depth_pitch; D.stride = n_images > 1 ? depth_stride : 0;
  D.w = depth_width; D.h = depth_height;
  return sf_launch_depth_interp(c, D, n_images, factor, d_out, out_pitch, n_images > 1 ? out_stride : 0);
}

extern "C" int sf_detect_orb_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                    int32_t max_features, const sf_orb_detector_params* det, const sf_orb_params* orb,
                                    sf_keypoint* d_kpts_out, int32_t cap, int32_t* n_out) {
  int rc;
  if ((rc = detect_prologue(c, d_image, width, height, pitch, d_kpts_out, cap, n_out)) != SF_OK) return rc;
  if (max_features < 1) return sf_fail(c, SF_EINVAL, "ORB shares out max_features = %d keypoints over its levels: it must be >= 1", max_features);
  const sf_orb_detector_params d = det ? *det : c->orb_det;
  const sf_orb_params o = orb ? *orb : c->orb;
  if ((rc = detect_ready(c, sf_orb_detector_validate(c, d, o), width, height)) != SF_OK) return rc;
  int32_t* d_n = nullptr;
  if ((rc = single_count_word(c, &d_n)) != SF_OK) return rc;
  if ((rc = sf_launch_detect_orb(c, d_image, 0, 1, width, height, pitch, max_features, &d, &o, d_kpts_out, cap, d_n)) != SF_OK) return rc;
  return sf_word_to_host(c, d_n, n_out);
}

extern "C" int sf_detect_surf_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                     int32_t max_features, const sf_surf_params* surf, sf_keypoint* d_kpts_out, int32_t cap,
                                     int32_t* n_out) {
  int rc;
  if ((rc = detect_prologue(c, d_image, width, height, pitch, d_kpts_out, cap, n_out)) != SF_OK) return rc;
  const sf_surf_params prm = surf ? *surf : c->surf;
  if ((rc = detect_ready(c, sf_surf_validate(c, prm), width, height, true)) != SF_OK) return rc;
  int32_t* d_n = nullptr;
  SfDetectOne one;
  if ((rc = single_count_word(c, &d_n)) != SF_OK) return rc;
  if ((rc = sf_launch_detect_surf(c, d_image, 0, 1, width, height, pitch, max_features, &prm, d_kpts_out, cap, d_n, &one)) != SF_OK)
    return rc;
  const unsigned cand_cap = sf_surf_candidate_cap(c);     // (the image kept no keypoint: nothing was written)
  if (one.count[0] > cand_cap)
    return sf_fail(c, SF_ERANGE, "SURF: %u maxima in a %d x %d image exceed the candidate capacity %u; raise hessian_threshold",
                   one.count[0], width, height, cand_cap);
  *n_out = sf_limit_keypoints((int)one.count[0], max_features);
  return SF_OK;
}

extern "C" int sf_detect_sift_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                     int32_t max_features, const sf_sift_params* sift, sf_keypoint* d_kpts_out, int32_t cap,
                                     int32_t* n_out) {
  int rc;
  if ((rc = detect_prologue(c, d_image, width, height, pitch, d_kpts_out, cap, n_out)) != SF_OK) return rc;
  const sf_sift_params prm = sift ? *sift : c->sift;
  if ((rc = detect_ready(c, sf_sift_validate(c, prm), width, height)) != SF_OK) return rc;
  int32_t* d_n = nullptr;
  SfDetectOne one;
  if ((rc = single_count_word(c, &d_n)) != SF_OK) return rc;
  if ((rc = sf_sift_batch_reserve(c, width, height, prm, 1)) != SF_OK) return rc;              // a chunk of one
  if ((rc = sf_launch_detect_sift(c, d_image, 0, 1, width, height, pitch, max_features, &prm, d_kpts_out, cap, d_n, &one)) != SF_OK)
    return rc;
  const unsigned cand_cap = c->sift_batch.cap_img;        // (past it the image kept no keypoint: nothing was written)
  if (one.count[0] > cand_cap)
    return sf_fail(c, SF_ERANGE, "SIFT: %u extrema in a %d x %d image exceed the capacity %u; raise contrast_threshold", one.count[0],
                   width, height, cand_cap);
  if (one.count[1] > cand_cap)
    return sf_fail(c, SF_ERANGE, "SIFT: %u keypoints in a %d x %d image exceed the capacity %u; raise contrast_threshold", one.count[1],
                   width, height, cand_cap);
  *n_out = sf_limit_keypoints((int)one.count[1], sf_sift_limit(prm.n_features, max_features));
  return SF_OK;
}

extern "C" int sf_debug_sift_plane(sf_handle c, int32_t octave, int32_t layer, int32_t dog, int16_t* d_out) {
  if (!c) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_sift_copy_plane(c, octave, layer, dog, d_out);
}

// ---- around every detector: Vis/RoiRatios and cv::cornerSubPix (Feature2D::generateKeypoints; kernel in k_subpix.hip) ----
extern "C" void sf_front_defaults(sf_front_params* p) {
  if (!p) return;
  for (float& r : p->roi_ratios) r = 0.f;   // Vis/RoiRatios "0.0 0.0 0.0 0.0" [upstream rtabmap Parameters.h]
  p->subpix_win_size = 3;                   // Vis/SubPixWinSize
  p->subpix_iterations = 0;                 // Vis/SubPixIterations: 0 = no refinement
  p->subpix_eps = 0.02f;                    // Vis/SubPixEps
}

static bool roi_ratios_valid(const float* r) {
  for (int k = 0; k < 4; ++k)
    if (!(r[k] >= 0.f && r[k] <= 1.f)) return false;
  return true;
}

// Feature2D::computeRoi: float arithmetic, C++'s truncating assignment
extern "C" int sf_compute_roi(int32_t width, int32_t height, const float* ratios, int32_t* roi_xywh) {
  if (!ratios || !roi_xywh || width < 1 || height < 1 || !roi_ratios_valid(ratios)) return SF_EINVAL;
  const float r0 = ratios[0], r1 = ratios[1], r2 = ratios[2], r3 = ratios[3];
  int x = 0, y = 0;
  if (r0 > 0.f && r0 < 1.f - r1) x = (int)(width * r0);
  int w = width - x;
  if (r1 > 0.f && r1 < 1.f - r0) w = (int)((float)w - width * r1);
  if (r2 > 0.f && r2 < 1.f - r3) y = (int)(height * r2);
  int h = height - y;
  if (r3 > 0.f && r3 < 1.f - r2) h = (int)((float)h - height * r3);
  roi_xywh[0] = x; roi_xywh[1] = y; roi_xywh[2] = w; roi_xywh[3] = h;
  return (w < 3 || h < 3) ? SF_EINVAL : SF_OK;
}

static int front_validate(sf_context* c, const sf_front_params& f) {
  if (!roi_ratios_valid(f.roi_ratios))
    return sf_fail(c, SF_EINVAL, "Vis/RoiRatios %g %g %g %g: every ratio must lie in [0, 1]", (double)f.roi_ratios[0],
                   (double)f.roi_ratios[1], (double)f.roi_ratios[2], (double)f.roi_ratios[3]);
  if (f.subpix_win_size < 0 || f.subpix_win_size > 15) return sf_fail(c, SF_EINVAL, "subpix_win_size %d outside 0 .. 15", f.subpix_win_size);
  if (f.subpix_iterations < 0) return sf_fail(c, SF_EINVAL, "subpix_iterations %d is negative", f.subpix_iterations);
  if (!(f.subpix_eps == f.subpix_eps)) return sf_fail(c, SF_EINVAL, "subpix_eps is NaN");
  return SF_OK;
}

extern "C" int sf_front_set_params(sf_handle c, const sf_front_params* params) {
  if (!c || !params) return SF_EINVAL;
  int rc = front_validate(c, *params);
  if (rc != SF_OK) return rc;
  c->front = *params;
  return SF_OK;
}

extern "C" int sf_front_get_params(sf_handle c, sf_front_params* params) { return get_block(c, params, &sf_context::front); }

static int check_subpix(sf_context* c, int width, int height, int win, int iterations) {
  if (win < 1 || win > 15) return sf_fail(c, SF_EINVAL, "cornerSubPix window %d outside 1 .. 15", win);
  if (iterations < 1) return sf_fail(c, SF_EINVAL, "cornerSubPix iterations %d: at least 1", iterations);
  if (width < 2 * win + 5 || height < 2 * win + 5)
    return sf_fail(c, SF_EINVAL, "cornerSubPix with window %d needs an image of at least %d x %d, not %d x %d (cv::cornerSubPix asserts the same)",
                   win, 2 * win + 5, 2 * win + 5, width, height);
  return SF_OK;
}

extern "C" int sf_corner_subpix_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                       sf_keypoint* d_kpts, int32_t n, int32_t win, int32_t iterations, float eps) {
  if (!c || n < 0) return SF_EINVAL;
  int rc = sf_check_image(c, d_image, width, height, pitch, 1, "image");
  if (rc != SF_OK) return rc;
  if ((rc = check_subpix(c, width, height, win, iterations)) != SF_OK) return rc;
  if (!(eps == eps)) return sf_fail(c, SF_EINVAL, "cornerSubPix eps is NaN");
  if (n > 0 && !d_kpts) return sf_fail(c, SF_EINVAL, "keypoints missing");
  if (n == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_corner_subpix(c, d_image, 0, 1, width, height, pitch, d_kpts, n, nullptr, n, 0, 0, win, iterations, eps);
}

static bool roi_is_zero(const float* r) { return r[0] == 0.f && r[1] == 0.f && r[2] == 0.f && r[3] == 0.f; }

int sf_front_plan(sf_context* c, int width, int height, FrontPlan* fp) {
  const sf_front_params& f = c->front;
  const SfFeatureType& t = sf_type_of(c);
  int32_t roi[4] = {0, 0, 0, 0};
  const int rc = sf_compute_roi(width, height, f.roi_ratios, roi);
  if (t.no_roi && !roi_is_zero(f.roi_ratios))
    return sf_fail(c, SF_EINVAL, "Vis/RoiRatios under Vis/FeatureType %d (%s) is not built%s", t.type, t.name, t.no_roi);
  if (rc != SF_OK)
    return sf_fail(c, SF_EINVAL, "Vis/RoiRatios %g %g %g %g leave a ROI of %d x %d in a %d x %d image: both sides must be >= 3",
                   (double)f.roi_ratios[0], (double)f.roi_ratios[1], (double)f.roi_ratios[2], (double)f.roi_ratios[3], roi[2], roi[3], width, height);
  if (t.corners == CORNERS_GFTT) {                         // (the ROI is the image when the ratios are zero)
    const int side = sf_check_gftt_side(c, roi[2], roi[3], roi_is_zero(f.roi_ratios) ? "an image" : "a ROI");
    if (side != SF_OK) return side;
  }
  fp->x = roi[0]; fp->y = roi[1]; fp->w = roi[2]; fp->h = roi[3];
  fp->refine = f.subpix_win_size > 0 && f.subpix_iterations > 0;
  return fp->refine ? check_subpix(c, width, height, f.subpix_win_size, f.subpix_iterations) : SF_OK;
}

// ---- Vis/GridRows x Vis/GridCols: the detector per cell of the ROI (Feature2D::generateKeypoints; kernel in k_grid.hip) ----
extern "C" void sf_grid_defaults(sf_grid_params* p) {
  if (!p) return;
  p->grid_rows = 1;            // Vis/GridRows [upstream rtabmap Parameters.h]
  p->grid_cols = 1;            // Vis/GridCols
}

static bool grid_valid(const sf_grid_params& g) {
  return g.grid_rows >= 1 && g.grid_rows <= 16 && g.grid_cols >= 1 && g.grid_cols <= 16;
}

extern "C" int sf_grid_set_params(sf_handle c, const sf_grid_params* params) {
  if (!c || !params) return SF_EINVAL;
  if (!grid_valid(*params))
    return sf_fail(c, SF_EINVAL, "Vis/GridRows %d, Vis/GridCols %d: each lies in 1 .. 16", params->grid_rows, params->grid_cols);
  c->grid = *params;
  return SF_OK;
}

extern "C" int sf_grid_get_params(sf_handle c, sf_grid_params* params) { return get_block(c, params, &sf_context::grid); }

extern "C" int sf_compute_grid(int32_t width, int32_t height, const float* roi_ratios, const sf_grid_params* grid,
                               int32_t max_features, int32_t* out) {
  static const float no_roi[4] = {0.f, 0.f, 0.f, 0.f};
  const sf_grid_params g = arg_or_defaults(grid, sf_grid_defaults);
  if (!out || !grid_valid(g) || max_features < 1) return SF_EINVAL;
  int32_t roi[4];
  const int rc = sf_compute_roi(width, height, roi_ratios ? roi_ratios : no_roi, roi);
  if (rc != SF_OK) return rc;
  const int cells = g.grid_rows * g.grid_cols;
  const int quota = (int)std::ceil((float)max_features / (float)cells);
  const long long rows_cap = (long long)cells * quota;
  out[0] = roi[0]; out[1] = roi[1];
  out[2] = roi[2] / g.grid_cols; out[3] = roi[3] / g.grid_rows;
  out[4] = quota;
  out[5] = (int32_t)std::min(rows_cap, (long long)INT32_MAX);
  if (out[2] < 3 || out[3] < 3) return SF_EINVAL;
  return rows_cap > SF_MAX_FEATURES ? SF_ERANGE : SF_OK;
}

// The cells of an extraction call, behind sf_front_plan and the check of max_features: nothing to do on a 1 x 1 grid (one
// "cell", the ROI, with the whole of max_features), else what sf_compute_grid says -- refused before anything is touched
int sf_grid_plan(sf_context* c, int width, int height, int max_features, FrontPlan* fp) {
  fp->rows = fp->cols = 1;
  fp->col_size = fp->w; fp->row_size = fp->h;
  fp->quota = fp->rows_cap = max_features;
  const sf_grid_params& g = c->grid;
  if (g.grid_rows == 1 && g.grid_cols == 1) return SF_OK;
  const SfFeatureType& t = sf_type_of(c);
  if (t.no_grid)
    return sf_fail(c, SF_EINVAL, "Vis/GridRows x Vis/GridCols %d x %d under Vis/FeatureType %d (%s) is not built%s", g.grid_rows,
                   g.grid_cols, t.type, t.name, t.no_grid);
  int32_t o[6];
  const int rc = sf_compute_grid(width, height, c->front.roi_ratios, &g, max_features, o);
  if (rc == SF_ERANGE)
    return sf_fail(c, SF_ERANGE, "a grid of %d x %d cells with %d keypoints apiece holds %d rows > %d (KeyPointVec.size is an int16)",
                   g.grid_rows, g.grid_cols, o[4], o[5], SF_MAX_FEATURES);
  if (rc != SF_OK)
    return sf_fail(c, SF_EINVAL, "a grid of %d x %d on a ROI of %d x %d leaves cells of %d x %d: both sides must be >= 3", g.grid_rows,
                   g.grid_cols, fp->w, fp->h, o[2], o[3]);
  if (t.corners == CORNERS_GFTT) {
    const int side = sf_check_gftt_side(c, o[2], o[3], "a grid cell");
    if (side != SF_OK) return side;
  }
  fp->rows = g.grid_rows; fp->cols = g.grid_cols;
  fp->col_size = o[2]; fp->row_size = o[3]; fp->quota = o[4]; fp->rows_cap = o[5];
  return SF_OK;
}

// The detection stage under a grid, for n images (the single calls: n = 1): the launchers with the cells as their
// images, then k_grid_gather -- d_kpts [n][rows_cap] in full-image coordinates, d_n [n], nothing waited for
int sf_grid_detect(sf_context* c, const FrontPlan& fp, const sf_detector_params& dp, const uint8_t* d_left, size_t image_stride,
                   int n, int pitch, sf_keypoint* d_kpts, int32_t* d_n, const SfMask& mask) {
  const int cells = fp.rows * fp.cols;
  const size_t count_bytes = ((size_t)n * cells * 4 + 255) & ~(size_t)255;
  int rc;
  if ((rc = sf_buf_reserve(c, c->ft_cells, count_bytes + (size_t)n * fp.rows_cap * sizeof(sf_keypoint))) != SF_OK) return rc;
  int32_t* d_cell_n = (int32_t*)c->ft_cells.p;
  sf_keypoint* d_cell_kpts = (sf_keypoint*)((char*)c->ft_cells.p + count_bytes);
  SfCells g;
  g.per_image = cells; g.cols = fp.cols;
  g.row_step = (size_t)fp.row_size * pitch; g.col_step = (size_t)fp.col_size;
  const uint8_t* d_roi = d_left + (size_t)fp.y * pitch + fp.x;
  SfMask m = sf_mask_at(mask, fp.x, fp.y);               // the mask cropped and cut like the image, at its own pitch
  m.cells = g;
  m.cells.row_step = (size_t)fp.row_size * mask.pitch;
  if (sf_type_of(c).corners == CORNERS_FAST)
    rc = sf_launch_detect_fast(c, d_roi, image_stride, n * cells, fp.col_size, fp.row_size, pitch, fp.quota, &c->fast, d_cell_kpts,
                               fp.quota, d_cell_n, g, m);
  else
    rc = sf_launch_detect_corners(c, d_roi, image_stride, n * cells, fp.col_size, fp.row_size, pitch, fp.quota, dp.quality_level,
                                  dp.min_distance, d_cell_kpts, fp.quota, d_cell_n, g, m);
  if (rc != SF_OK) return rc;
  return sf_launch_grid_gather(c, d_cell_kpts, d_cell_n, n, fp.rows, fp.cols, fp.quota, fp.x, fp.y, fp.col_size, fp.row_size, d_kpts,
                               fp.rows_cap, d_n);
}

extern "C" void sf_stereo_flow_defaults(sf_stereo_flow_params* p) {
  if (!p) return;
  p->win_width = 15; p->win_height = 3;        // Stereo/WinWidth, Stereo/WinHeight [upstream rtabmap Parameters.h]
  p->max_level = 5;                            // Stereo/MaxLevel
  p->iterations = 30;                          // Stereo/Iterations
  p->epsilon = 0.01;                           // Stereo/Eps
  p->min_disparity = 0.5f; p->max_disparity = 128.0f;
  p->min_eig_threshold = 1e-4f;                // the literal in StereoOpticalFlow::computeCorrespondences
}

extern "C" int sf_stereo_correspondences_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right, int32_t width,
                                                int32_t height, int32_t pitch, const sf_keypoint* d_kpts, int32_t n,
                                                const sf_stereo_flow_params* params, float* d_right_xy,
                                                uint8_t* d_status, float* d_right_x, float* d_err) {
  if (!c || n < 0) return SF_EINVAL;
  int rc = sf_check_image(c, d_left && d_right, width, height, pitch, 1, "stereo pair");
  if (rc != SF_OK) return rc;
  if (n > 0 && (!d_kpts || !d_right_xy || !d_status)) return sf_fail(c, SF_EINVAL, "corners or output arrays missing");
  const sf_stereo_flow_params prm = arg_or_defaults(params, sf_stereo_flow_defaults);
  if (prm.win_width <= 2 || prm.win_height <= 2)           // (one by one what sf_stereo_flow_ok refuses, the last by what is left)
    return sf_fail(c, SF_EINVAL, "window of %d x %d: both sides must be > 2 (cv::calcOpticalFlowPyrLK asserts the same)", prm.win_width, prm.win_height);
  if ((long long)prm.win_width * prm.win_height > 1024) return sf_fail(c, SF_ERANGE, "window of %d x %d exceeds 1024 pixels", prm.win_width, prm.win_height);
  if (prm.max_level < 0 || prm.max_level > 15) return sf_fail(c, SF_ERANGE, "max_level %d outside 0 .. 15", prm.max_level);
  if (!sf_stereo_flow_ok(prm)) return sf_fail(c, SF_EINVAL, "epsilon is NaN");
  if (n == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_stereo_flow(c, d_left, d_right, width, height, pitch, d_kpts, n, &prm, d_right_xy, d_status, d_right_x, d_err);
}

// ---- block matching (Stereo/OpticalFlow false; kernel in k_stereo_bm.hip) ------------------------------------------
extern "C" void sf_stereo_defaults(sf_stereo_params* p) {
  if (!p) return;
  p->optical_flow = 1;                         // Stereo/OpticalFlow [upstream rtabmap Parameters.h]
  p->ssd = 1;                                  // Stereo/SSD
}

extern "C" int sf_stereo_set_params(sf_handle c, const sf_stereo_params* params) {
  if (!c || !params) return SF_EINVAL;
  if ((params->optical_flow != 0 && params->optical_flow != 1) || (params->ssd != 0 && params->ssd != 1))
    return sf_fail(c, SF_EINVAL, "Stereo/OpticalFlow %d, Stereo/SSD %d: each is 0 or 1", params->optical_flow, params->ssd);
  c->stereo = *params;
  return SF_OK;
}

extern "C" int sf_stereo_get_params(sf_handle c, sf_stereo_params* params) { return get_block(c, params, &sf_context::stereo); }

// what block matching refuses of the flow parameters (epsilon and min_eig_threshold are not read)
int sf_check_block_match(sf_context* c, const sf_stereo_flow_params& prm) {
  if (prm.win_width < 1 || prm.win_height < 1 || !(prm.win_width & 1) || !(prm.win_height & 1))
    return sf_fail(c, SF_EINVAL, "block matching window of %d x %d: both sides must be odd", prm.win_width, prm.win_height);
  if ((long long)prm.win_width * prm.win_height > 1024)
    return sf_fail(c, SF_EINVAL, "block matching window of %d x %d exceeds 1024 pixels", prm.win_width, prm.win_height);
  if (prm.max_level < 0 || prm.max_level > 15) return sf_fail(c, SF_ERANGE, "max_level %d outside 0 .. 15", prm.max_level);
  if (!std::isfinite(prm.min_disparity) || !std::isfinite(prm.max_disparity) || prm.min_disparity < 0.f ||
      prm.min_disparity > prm.max_disparity)
    return sf_fail(c, SF_EINVAL, "block matching disparities %g .. %g: finite, 0 <= min <= max", (double)prm.min_disparity,
                   (double)prm.max_disparity);
  if (std::floor(prm.max_disparity) > 1024.f)
    return sf_fail(c, SF_EINVAL, "block matching max_disparity %g: at most 1024 whole pixels", (double)prm.max_disparity);
  return SF_OK;
}

extern "C" int sf_stereo_block_match_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right, int32_t width,
                                            int32_t height, int32_t pitch, const sf_keypoint* d_kpts, int32_t n,
                                            const sf_stereo_flow_params* params, int32_t ssd, float* d_right_xy,
                                            uint8_t* d_status, float* d_right_x, float* d_score) {
  if (!c || n < 0) return SF_EINVAL;
  int rc = sf_check_image(c, d_left && d_right, width, height, pitch, 1, "stereo pair");
  if (rc != SF_OK) return rc;
  if (n > 0 && (!d_kpts || !d_right_xy || !d_status)) return sf_fail(c, SF_EINVAL, "corners or output arrays missing");
  if (ssd != 0 && ssd != 1) return sf_fail(c, SF_EINVAL, "ssd %d: 1 = squared, 0 = absolute differences", ssd);
  const sf_stereo_flow_params prm = arg_or_defaults(params, sf_stereo_flow_defaults);
  if ((rc = sf_check_block_match(c, prm)) != SF_OK) return rc;
  if (n == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_stereo_bm_batch(c, d_left, d_right, 0, 1, width, height, pitch, d_kpts, n, nullptr, &prm, ssd, d_right_xy,
                                   d_status, d_right_x, d_score);
}
