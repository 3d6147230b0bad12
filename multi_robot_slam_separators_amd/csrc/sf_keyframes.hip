// sf_keyframes.hip -- images to keyframes of the store: sf_extract_keyframe_device, the full call on host images, the batch
// pipeline of the four families of batch calls, the camera's own images and the calls that add keyframes with NetVLAD rows.
// A stereo keyframe and a depth keyframe differ in their second input alone (SecondInput): every path here is written once
// and branches on it -- get_features_host, features_batch, add_keyframes_batch -- and the public calls are argument adapters.
#include "sf_host.hpp"

// A keyframe's second input: the right image with the stereo stage that reads it (flow: its parameters), or a depth image --
// under Vis/DepthAsMask with the detector's mask -- and no stereo stage.  Host or device pointers, as the call's left image.
// `call`: the name that a depth call's refusals carry in front; the stereo calls carry none.  { right, flow } is a stereo
// keyframe's, { nullptr, nullptr, &depth, call } a depth keyframe's (the call's checks fill in the depth images' own size)
struct SecondInput {
  const uint8_t* right = nullptr;
  const sf_stereo_flow_params* flow = nullptr;
  SfDepthIn* depth = nullptr;
  const char* call = "";
};

static const char* colon(const char* call) { return *call ? ": " : ""; }   // "call: text", or "text" alone

// a camera image (sf_image_format): a row holds 3 bytes per pixel for the colour formats
static int check_format(sf_context* c, int format) {
  if (format != SF_IMAGE_RGB8 && format != SF_IMAGE_BGR8 && format != SF_IMAGE_MONO8)
    return sf_fail(c, SF_EINVAL, "image format %d unknown (0 = rgb8, 1 = bgr8, 2 = mono8)", format);
  return SF_OK;
}

static long long image_row_bytes(int format, int width) { return (long long)width * (format == SF_IMAGE_MONO8 ? 1 : 3); }

static int check_camera_image(sf_context* c, const char* call, bool present, int format, int width, int height, int pitch,
                              int min_side, const char* what) {
  int rc = check_format(c, format);
  if (rc != SF_OK) return rc;
  if (!present || width < min_side || height < min_side || pitch < image_row_bytes(format, width))
    return sf_fail(c, SF_EINVAL, "%s%s%s missing or malformed (%d x %d, pitch %d, %d byte(s) per pixel)", call, colon(call), what,
                   width, height, pitch, format == SF_IMAGE_MONO8 ? 1 : 3);
  return SF_OK;
}

static int check_max_features(sf_context* c, const char* call, int max_features) {
  if (max_features <= 0 || max_features > SF_MAX_FEATURES)
    return sf_fail(c, SF_ERANGE, "%s%smax_features %d outside 1 .. %d (KeyPointVec.size is an int16)", call, colon(call), max_features,
                   SF_MAX_FEATURES);
  return SF_OK;
}

static int extract_keyframe(sf_context* c, const uint8_t* d_left, int32_t width, int32_t height, int32_t pitch,
                            const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status, int32_t n,
                            const sf_stereo_camera* cam, int32_t* out_slot, int32_t* out_rows, uint8_t* d_desc_out,
                            float* d_xyz_out, sf_keypoint* d_kpts_out, bool reuse_sift_pyramid, const SfDepthIn* depth = nullptr) {
  if (!c || !cam || n < 0) return SF_EINVAL;
  int rc = sf_check_image(c, d_left, width, height, pitch, 1, "left image");
  if (rc != SF_OK) return rc;
  if (n > 0 && !d_kpts) return sf_fail(c, SF_EINVAL, "keypoints missing");
  if (n > SF_MAX_FEATURES) return sf_fail(c, SF_ERANGE, "%d corners > int16 limit of KeyPointVec.size", n);
  if ((rc = sf_check_integral(c, width, height)) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  ExtractKind kind;
  if ((rc = sf_extract_kind(c, &kind)) != SF_OK) return rc;
  kind.sift.reuse = reuse_sift_pyramid;                    // (the full call: the SIFT detector has just run on this image)
  if ((rc = sf_store_reserve(c, c->store, c->store.slots + 1, n, kind.bytes)) != SF_OK) return rc;
  if (out_rows && (rc = sf_buf_reserve(c, c->ex_rows, 16)) != SF_OK) return rc;
  const int slot = c->store.slots;
  if ((rc = sf_launch_extract_batch(c, d_left, 0, 1, width, height, pitch, d_kpts, d_right_x, d_status, n, nullptr, cam, kind,
                                    slot, d_desc_out, d_xyz_out, d_kpts_out,
                                    out_rows ? (int32_t*)c->ex_rows.p : nullptr, depth)) != SF_OK)
    return rc;
  c->store.slots += 1;
  if (out_slot) *out_slot = slot;
  return out_rows ? sf_word_to_host(c, c->ex_rows.p, out_rows) : SF_OK;
}

extern "C" int sf_extract_keyframe_device(sf_handle c, const uint8_t* d_left, int32_t width, int32_t height,
                                          int32_t pitch, const sf_keypoint* d_kpts, const float* d_right_x,
                                          const uint8_t* d_status, int32_t n, const sf_stereo_camera* cam,
                                          int32_t* out_slot, int32_t* out_rows, uint8_t* d_desc_out,
                                          float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return extract_keyframe(c, d_left, width, height, pitch, d_kpts, d_right_x, d_status, n, cam, out_slot, out_rows, d_desc_out,
                          d_xyz_out, d_kpts_out, false);
}

extern "C" int sf_extract_keyframe_depth_device(sf_handle c, const uint8_t* d_left, int32_t width, int32_t height, int32_t pitch,
                                                const sf_keypoint* d_kpts, const void* d_depth, int32_t depth_format,
                                                int32_t depth_pitch, int32_t n, const sf_stereo_camera* cam, int32_t* out_slot,
                                                int32_t* out_rows, uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out) {
  if (!c || !cam || n < 0) return SF_EINVAL;
  SfDepthIn D{d_depth, depth_format, depth_pitch};
  const int rc = sf_depth_in(c, "sf_extract_keyframe_depth_device", &D, width, height, 1);
  if (rc != SF_OK) return rc;
  return extract_keyframe(c, d_left, width, height, pitch, d_kpts, nullptr, nullptr, n, cam, out_slot, out_rows, d_desc_out,
                          d_xyz_out, d_kpts_out, false, &D);
}

// ---- what differs between the families of batch calls (the generic calls of types 3 .. 8; the _orb_, _surf_ and _sift_ calls of
// types 2, 0 and 1): what the family's detector refuses, what it reserves, its launch -- three switches side by side ---------
struct BatchPlan {
  sf_detector_params dp;
  sf_stereo_flow_params prm;
  ExtractKind kind;
  FrontPlan front;
};

// behind a detector's own parameters (`validated`): the pixels of an image, the images of a grid dimension
static int batch_limits(sf_context* c, int validated, const char* name, int n_keyframes, int width, int height) {
  if (validated != SF_OK || (validated = sf_check_pixels(c, width, height)) != SF_OK) return validated;
  return n_keyframes <= 65535 ? SF_OK : sf_fail(c, SF_ERANGE, "%s batch of %d keyframes (at most 65535)", name, n_keyframes);
}

// what sf_detect_orb_device, sf_detect_surf_device and sf_detect_sift_device refuse, then what the family's batch layout does
static int family_check(sf_context* c, BatchFamily family, int n_keyframes, int width, int height) {
  int rc;
  switch (family) {
    case BATCH_GENERIC: break;                             // (GFTT's parameters: batch_check; FAST's pixels: family_reserve)
    case BATCH_ORB: {
      if ((rc = batch_limits(c, sf_orb_detector_validate(c, c->orb_det, c->orb), "ORB", n_keyframes, width, height)) != SF_OK) return rc;
      const SfOrbPyr P = sf_orb_pyr_layout(width, height, c->orb_det.scale_factor, c->orb_det.n_levels);
      for (int l = 0; l < P.n; ++l)
        if (P.w[l] < 1 || P.h[l] < 1)
          return sf_fail(c, SF_ERANGE, "pyramid level %d of a %d x %d image at scale %g is empty", l, width, height, (double)P.scale[l]);
      break;
    }
    case BATCH_SURF: {                                     // (the layout's 2^31 plane samples)
      SfSurfBatchPlan sp;
      if ((rc = batch_limits(c, sf_surf_validate(c, c->surf), "SURF", n_keyframes, width, height)) != SF_OK) return rc;
      return sf_surf_batch_plan_host(c, width, height, c->surf, n_keyframes, 0, 0, &sp);
    }
    case BATCH_SIFT: {                                     // (the image's sides, the 2^26 difference samples)
      SfSiftBatchPlan sp;
      if ((rc = batch_limits(c, sf_sift_validate(c, c->sift), "SIFT", n_keyframes, width, height)) != SF_OK) return rc;
      return sf_sift_batch_plan_host(c, width, height, c->sift, n_keyframes, 0, 0, &sp);
    }
  }
  return SF_OK;
}

static int family_reserve(sf_context* c, const SfFeatureType& t, int n, int width, int height) {
  SfSurfBatchPlan surf;
  switch (t.family) {
    case BATCH_GENERIC: return t.corners == CORNERS_FAST ? sf_check_pixels(c, width, height) : SF_OK;
    case BATCH_ORB: return SF_OK;                          // (the detector's launcher reserves its pyramids)
    case BATCH_SURF: return sf_surf_batch_reserve(c, width, height, c->surf, n, &surf);   // planes, keys and integral images
    case BATCH_SIFT: return sf_sift_batch_reserve(c, width, height, c->sift, n);          // the chunk's planes and keys; the blur tables
  }
  return SF_OK;
}

// The detector on images [i0, i0 + m) of a batch, into that sub-range of c->ft_kpts / c->ft_counts; `kind`: what it leaves the extraction
static int family_detect(sf_context* c, const SfFeatureType& t, const BatchPlan& plan, ExtractKind* kind, const uint8_t* d_left,
                         size_t image_stride, int i0, int m, int width, int height, int pitch, const SfMask& mask_all = SfMask()) {
  const FrontPlan& fp = plan.front;
  SfMask mask = mask_all;                                  // (a depth call's mask, types 3 .. 8 only: planes laid out like the images)
  if (mask.p) mask.p += (size_t)i0 * mask.stride;
  const int maxf = fp.rows_cap;                            // rows per keyframe: max_features, or the grid's R C quota
  const uint8_t* d_images = d_left + (size_t)i0 * image_stride;
  const uint8_t* d_roi = d_images + (size_t)fp.y * pitch + fp.x;   // the ROI, at the parent's pitch and stride
  sf_keypoint* d_kpts = (sf_keypoint*)c->ft_kpts.p + (size_t)i0 * maxf;
  int32_t* d_n = (int32_t*)c->ft_counts.p + i0;
  switch (t.family) {
    case BATCH_ORB:                                        // (keypoints in level-0 coordinates; the pyramids stay for the extraction;
      kind->pyr_stride = sf_orb_pyr_layout(width, height, c->orb_det.scale_factor, c->orb_det.n_levels).total;   // no ROI: sf_front_plan)
      return sf_launch_detect_orb(c, d_images, image_stride, m, width, height, pitch, maxf, &c->orb_det, &c->orb, d_kpts, maxf, d_n);
    case BATCH_SURF:                                       // (no ROI, no grid: sf_front_plan, sf_grid_plan; the integral images stay
      kind->integral_ready = true;                         // for the extraction)
      return sf_launch_detect_surf(c, d_images, image_stride, m, width, height, pitch, maxf, &c->surf, d_kpts, maxf, d_n);
    case BATCH_SIFT:                                       // (likewise; the chunk's pyramids stay for the extraction)
      kind->sift.batch = true;
      return sf_launch_detect_sift(c, d_images, image_stride, m, width, height, pitch, maxf, &c->sift, d_kpts, maxf, d_n);
    case BATCH_GENERIC:
      if (fp.grid())                                       // the cells as the detector's images, joined by k_grid_gather
        return sf_grid_detect(c, fp, plan.dp, d_images, image_stride, m, pitch, d_kpts, d_n, mask);
      if (t.corners == CORNERS_FAST)
        return sf_launch_detect_fast(c, d_roi, image_stride, m, fp.w, fp.h, pitch, maxf, &c->fast, d_kpts, maxf, d_n, SfCells(),
                                     sf_mask_at(mask, fp.x, fp.y));
      return sf_launch_detect_corners(c, d_roi, image_stride, m, fp.w, fp.h, pitch, maxf, plan.dp.quality_level,
                                      plan.dp.min_distance, d_kpts, maxf, d_n, SfCells(), sf_mask_at(mask, fp.x, fp.y));
  }
  return SF_EINVAL;
}

// ---- depth keyframes: SensorData(rgb, depth, model) in place of a stereo pair (kernels in k_depth.hip) --------------------
// Vis/DepthAsMask is built for the two corner detectors: a type with a detector of its own takes no mask
static int check_depth_as_mask(sf_context* c, const char* call) {
  const SfFeatureType& t = sf_type_of(c);
  if (c->depth.depth_as_mask && t.corners == CORNERS_OWN)
    return sf_fail(c, SF_EINVAL, "%s: Vis/DepthAsMask under Vis/FeatureType %d (%s) is not built (its detector takes no mask); "
                   "sf_depth_set_params with depth_as_mask = 0 runs it on the whole image", call, t.type, t.name);
  return SF_OK;
}

// A host call's images on the device.  The left image, and the right image if there is one, as gray planes in c->ft_images:
// rows `width` bytes apart, planes img_bytes apart.  format < 0 or mono8: the pitched copy is the upload; a colour format: the
// images as they are (rows padded to 16 bytes: the conversion's wide path), then all planes in one launch.  Behind them the
// depth image if there is one, its own h rows of w elements, in c->dp_depth: *d_depth describes the copy
static int upload_inputs(sf_context* c, const uint8_t* left, const SecondInput& in, int format, int width, int height, int pitch,
                         size_t img_bytes, SfDepthIn* d_depth) {
  const uint8_t* const src[2] = {left, in.right};
  const int count = in.right ? 2 : 1;
  const int elem = in.depth && in.depth->format == SF_DEPTH_F32_M ? 4 : 2;
  const int dz_pitch = in.depth ? (elem * in.depth->w + 15) & ~15 : 0;   // rows padded to 16 bytes: k_depth_mask's wide loads
  int rc = sf_buf_reserve(c, c->ft_images, count * img_bytes);
  if (rc != SF_OK) return rc;
  if (in.depth && (rc = sf_buf_reserve(c, c->dp_depth, (size_t)dz_pitch * in.depth->h)) != SF_OK) return rc;
  uint8_t* d_planes = (uint8_t*)c->ft_images.p;
  if (format == SF_IMAGE_RGB8 || format == SF_IMAGE_BGR8) {
    const int src_pitch = (3 * width + 15) & ~15;
    const size_t src_bytes = ((size_t)src_pitch * height + 255) & ~(size_t)255;
    if ((rc = sf_buf_reserve(c, c->img_src, count * src_bytes)) != SF_OK) return rc;
    uint8_t* d_src = (uint8_t*)c->img_src.p;
    for (int i = 0; i < count; ++i)
      SF_HIP(c, hipMemcpy2DAsync(d_src + i * src_bytes, src_pitch, src[i], pitch, 3 * (size_t)width, height, hipMemcpyHostToDevice, c->stream));
    if ((rc = sf_launch_image_gray(c, d_src, nullptr, count, format, c->gray_rule, width, height, src_pitch, src_bytes, count, d_planes,
                                   width, img_bytes)) != SF_OK)
      return rc;
  } else {
    for (int i = 0; i < count; ++i)
      SF_HIP(c, hipMemcpy2DAsync(d_planes + i * img_bytes, width, src[i], pitch, width, height, hipMemcpyHostToDevice, c->stream));
  }
  if (!in.depth) return SF_OK;
  *d_depth = SfDepthIn{c->dp_depth.p, in.depth->format, dz_pitch, 0, in.depth->w, in.depth->h};
  SF_HIP(c, hipMemcpy2DAsync(c->dp_depth.p, dz_pitch, in.depth->p, in.depth->pitch, (size_t)elem * in.depth->w, in.depth->h,
                             hipMemcpyHostToDevice, c->stream));
  return SF_OK;
}

// The detector on one device plane of pitch `width`, the count on the host: every cell of a grid in one launch sequence and
// one wait for the keyframe's count; or the public detector call of the type's family on the ROI; or, under a mask (types
// 3 .. 8: check_depth_as_mask), the masked call of the type's corner detector
static int detect_single(sf_context* c, const FrontPlan& fp, const sf_detector_params& dp, const uint8_t* d_left, int width,
                         const SfMask& mask, sf_keypoint* d_kpts, int32_t* n) {
  const int maxf = fp.rows_cap;
  int rc;
  if (fp.grid()) {
    if ((rc = sf_buf_reserve(c, c->ft_counts, 4)) != SF_OK) return rc;
    if ((rc = sf_grid_detect(c, fp, dp, d_left, 0, 1, width, d_kpts, (int32_t*)c->ft_counts.p, mask)) != SF_OK) return rc;
    return sf_word_to_host(c, c->ft_counts.p, n);
  }
  const SfFeatureType& t = sf_type_of(c);
  const uint8_t* d_roi = d_left + (size_t)fp.y * width + fp.x;   // the detector's image: the ROI, at the parent's pitch
  if (t.family == BATCH_GENERIC && mask.p) {
    const uint8_t* d_mask_roi = sf_mask_at(mask, fp.x, fp.y).p;
    return t.corners == CORNERS_FAST
               ? sf_detect_fast_masked_device(c, d_roi, fp.w, fp.h, width, d_mask_roi, mask.pitch, maxf, nullptr, d_kpts, maxf, n)
               : sf_detect_corners_masked_device(c, d_roi, fp.w, fp.h, width, d_mask_roi, mask.pitch, maxf, dp.quality_level,
                                                 dp.min_distance, d_kpts, maxf, n);
  }
  switch (t.family) {
    case BATCH_ORB: return sf_detect_orb_device(c, d_roi, fp.w, fp.h, width, maxf, nullptr, nullptr, d_kpts, maxf, n);
    case BATCH_SURF: return sf_detect_surf_device(c, d_roi, fp.w, fp.h, width, maxf, nullptr, d_kpts, maxf, n);   // (no ROI: sf_front_plan)
    case BATCH_SIFT: return sf_detect_sift_device(c, d_roi, fp.w, fp.h, width, maxf, nullptr, d_kpts, maxf, n);   // (likewise)
    case BATCH_GENERIC:
      return t.corners == CORNERS_FAST ? sf_detect_fast_device(c, d_roi, fp.w, fp.h, width, maxf, nullptr, d_kpts, maxf, n)
                                       : sf_detect_corners_device(c, d_roi, fp.w, fp.h, width, maxf, dp.quality_level, dp.min_distance, d_kpts, maxf, n);
  }
  return SF_EINVAL;
}

// A host call's response in c->ft_wire: descriptors, 3D points, keypoints, maxf rows each
struct Wire {
  uint8_t* desc;
  float* xyz;
  sf_keypoint* kpts;
};

static int wire_reserve(sf_context* c, int maxf, int desc_bytes, Wire* w) {
  const size_t row_bytes = (size_t)desc_bytes + 12 + sizeof(sf_keypoint);
  const int rc = sf_buf_reserve(c, c->ft_wire, (size_t)maxf * row_bytes + 64);
  if (rc != SF_OK) return rc;
  w->desc = (uint8_t*)c->ft_wire.p;
  w->xyz = (float*)(w->desc + (((size_t)maxf * desc_bytes + 15) & ~(size_t)15));
  w->kpts = (sf_keypoint*)(w->xyz + 3 * (size_t)maxf);
  return SF_OK;
}

static int wire_download(sf_context* c, const Wire& w, int desc_bytes, int32_t k, uint8_t* desc_out, float* xyz_out, sf_keypoint* kpts_out) {
  if (k <= 0) return SF_OK;
  if (desc_out) SF_HIP(c, hipMemcpyAsync(desc_out, w.desc, (size_t)k * desc_bytes, hipMemcpyDeviceToHost, c->stream));
  if (xyz_out) SF_HIP(c, hipMemcpyAsync(xyz_out, w.xyz, (size_t)k * 12, hipMemcpyDeviceToHost, c->stream));
  if (kpts_out) SF_HIP(c, hipMemcpyAsync(kpts_out, w.kpts, (size_t)k * sizeof(sf_keypoint), hipMemcpyDeviceToHost, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));
  return SF_OK;
}

// The GetFeatsAndDesc handler in one call on HOST buffers: upload the image and its second input, detect, refine, track (a
// stereo pair) or mask the detector (a depth image, Vis/DepthAsMask), extract, download the response.  Everything between the
// two copies stays on the device; the keyframe is in the store when it returns.  A depth image whose size does not divide the
// image's makes no mask (sf_depth_masks): the detector runs as under Vis/DepthAsMask 0.  format < 0: rectified MONO8 planes
// (sf_get_features_and_descriptor); otherwise the camera's images in that sf_image_format, converted on the device behind the
// upload.  Everything an argument can be refused for is refused before the first reservation and the first upload.
static int get_features_host(sf_context* c, const uint8_t* left, const SecondInput& in, int format, int32_t width, int32_t height,
                             int32_t pitch, const sf_stereo_camera* cam, const sf_detector_params* det, uint8_t* desc_out,
                             float* xyz_out, sf_keypoint* kpts_out, int32_t cap_rows, int32_t* rows_out, int32_t* slot_out) {
  if (!c || !cam || !rows_out || cap_rows < 0) return SF_EINVAL;
  *rows_out = 0;
  SfDepthIn* depth = in.depth;                            // (the host's depth image)
  const bool present = left && (depth || in.right);
  const char* what = depth ? "image" : "stereo pair";
  int rc = format < 0 && !depth ? sf_check_image(c, present, width, height, pitch, 3, what)
                                : check_camera_image(c, in.call, present, format, width, height, pitch, 3, what);
  if (rc != SF_OK) return rc;
  if (depth) {
    if ((rc = sf_depth_in(c, in.call, depth, width, height, 1)) != SF_OK) return rc;
    if ((rc = check_depth_as_mask(c, in.call)) != SF_OK) return rc;
  }
  FrontPlan fp;
  if ((rc = sf_front_plan(c, width, height, &fp)) != SF_OK) return rc;
  const sf_detector_params dp = arg_or_defaults(det, sf_detector_defaults);
  if ((rc = check_max_features(c, in.call, dp.max_features)) != SF_OK) return rc;
  if ((rc = sf_grid_plan(c, width, height, dp.max_features, &fp)) != SF_OK) return rc;
  // (the GFTT parameters are checked under every feature type, FAST and ORB included, which do not use them)
  if ((rc = sf_check_gftt(c, dp.quality_level, dp.min_distance)) != SF_OK) return rc;
  if (fp.grid() && (rc = sf_check_pixels(c, fp.col_size, fp.row_size)) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  ExtractKind kind;
  if ((rc = sf_extract_kind(c, &kind)) != SF_OK) return rc;
  const size_t img_bytes = ((size_t)width * height + 255) & ~(size_t)255;
  const int maxf = fp.rows_cap;                            // the rows of the call's buffers: max_features, or the grid's R C quota
  const bool masked = depth && sf_depth_masks(c, *depth, width, height);
  Wire wire;
  if ((rc = sf_buf_reserve(c, c->ft_kpts, (size_t)maxf * sizeof(sf_keypoint))) != SF_OK) return rc;
  if (!depth && (rc = sf_buf_reserve(c, c->ft_flow, (size_t)maxf * 16)) != SF_OK) return rc;
  if (masked && (rc = sf_buf_reserve(c, c->dp_mask, img_bytes)) != SF_OK) return rc;
  if ((rc = wire_reserve(c, maxf, kind.bytes, &wire)) != SF_OK) return rc;
  SfDepthIn D;                                             // the device's copy of the depth image
  if ((rc = upload_inputs(c, left, in, format, width, height, pitch, img_bytes, &D)) != SF_OK) return rc;
  const uint8_t* d_left = (const uint8_t*)c->ft_images.p;
  const uint8_t* d_right = d_left + img_bytes;
  SfMask mask;                                             // the image's pitch: cropped and cut into cells like the image
  if (masked) {
    if ((rc = sf_launch_depth_mask(c, D, 1, width, height, cam->min_depth, cam->max_depth, (uint8_t*)c->dp_mask.p, width, 0)) != SF_OK)
      return rc;
    mask.p = (const uint8_t*)c->dp_mask.p; mask.pitch = width;
  }
  sf_keypoint* d_kpts = (sf_keypoint*)c->ft_kpts.p;
  int32_t n = 0;
  if ((rc = detect_single(c, fp, dp, d_left, width, mask, d_kpts, &n)) != SF_OK) return rc;
  n = std::min(n, maxf);
  if (fp.launch() &&
      (rc = sf_launch_corner_subpix(c, d_left, 0, 1, width, height, width, d_kpts, n, nullptr, maxf, fp.off_x(), fp.off_y(),
                                    fp.refine ? c->front.subpix_win_size : 0, c->front.subpix_iterations, c->front.subpix_eps)) != SF_OK)
    return rc;
  float* d_rx = nullptr;
  uint8_t* d_status = nullptr;
  if (!depth) {
    float* d_xy = (float*)c->ft_flow.p;                  // [n][2], then x [n], then status [n]
    d_rx = d_xy + 2 * (size_t)maxf;
    d_status = (uint8_t*)(d_rx + maxf);
    rc = c->stereo.optical_flow
             ? sf_stereo_correspondences_device(c, d_left, d_right, width, height, width, d_kpts, n, in.flow, d_xy, d_status, d_rx, nullptr)
             : sf_stereo_block_match_device(c, d_left, d_right, width, height, width, d_kpts, n, in.flow, c->stereo.ssd, d_xy, d_status, d_rx, nullptr);
    if (rc != SF_OK) return rc;
  }
  int32_t slot = -1, rows = 0;
  if ((rc = extract_keyframe(c, d_left, width, height, width, d_kpts, d_rx, d_status, n, cam, &slot, &rows, wire.desc, wire.xyz, wire.kpts,
                             kind.has_sift, depth ? &D : nullptr)) != SF_OK)   // (SIFT: the detector's pyramid serves, the refinement
    return rc;                                                                 // moved x and y only)
  *rows_out = rows;
  if (slot_out) *slot_out = slot;
  return wire_download(c, wire, kind.bytes, std::min(rows, cap_rows), desc_out, xyz_out, kpts_out);
}

extern "C" int sf_get_features_and_descriptor(sf_handle c, const uint8_t* left, const uint8_t* right, int32_t width,
                                              int32_t height, int32_t pitch, const sf_stereo_camera* cam,
                                              const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                              uint8_t* desc_out, float* xyz_out, sf_keypoint* kpts_out, int32_t cap_rows,
                                              int32_t* rows_out, int32_t* slot_out) {
  return get_features_host(c, left, {right, flow}, -1, width, height, pitch, cam, det, desc_out, xyz_out, kpts_out, cap_rows,
                           rows_out, slot_out);
}

extern "C" int sf_get_features_and_descriptor_u8(sf_handle c, const uint8_t* left, const uint8_t* right, int32_t format,
                                                 int32_t width, int32_t height, int32_t pitch, const sf_stereo_camera* cam,
                                                 const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                                 uint8_t* desc_out, float* xyz_out, sf_keypoint* kpts_out, int32_t cap_rows,
                                                 int32_t* rows_out, int32_t* slot_out) {
  if (!c) return SF_EINVAL;
  const int rc = check_format(c, format);
  if (rc != SF_OK) return rc;
  return get_features_host(c, left, {right, flow}, format, width, height, pitch, cam, det, desc_out, xyz_out, kpts_out, cap_rows,
                           rows_out, slot_out);
}

// (no right image, no stereo stage: the depth image gives the 3D points and, under Vis/DepthAsMask, the detector's mask)
extern "C" int sf_get_features_and_descriptor_depth(sf_handle c, const uint8_t* image, int32_t image_format, const void* depth,
                                                    int32_t depth_format, int32_t width, int32_t height, int32_t image_pitch,
                                                    int32_t depth_pitch, const sf_stereo_camera* cam,
                                                    const sf_detector_params* det, uint8_t* desc_out, float* xyz_out,
                                                    sf_keypoint* kpts_out, int32_t cap_rows, int32_t* rows_out, int32_t* slot_out) {
  SfDepthIn D{depth, depth_format, depth_pitch};
  return get_features_host(c, image, {nullptr, nullptr, &D, "sf_get_features_and_descriptor_depth"}, image_format, width, height,
                           image_pitch, cam, det, desc_out, xyz_out, kpts_out, cap_rows, rows_out, slot_out);
}

// what a depth batch call refuses of its n depth images, behind the images' own checks (n = 0: of the format alone)
static int depth_batch_check(sf_context* c, const char* call, SfDepthIn* depth, int n, int width, int height) {
  const int rc = sf_depth_in(c, call, depth, width, height, n);
  return rc != SF_OK ? rc : check_depth_as_mask(c, call);
}

// the masks of the n depth images, with the planes' pitch and stride (family_detect crops and cuts them like the images);
// none of depth images whose size does not divide the image's
static int depth_batch_mask(sf_context* c, const SfDepthIn& D, int n, int width, int height, int pitch, size_t image_stride,
                            const sf_stereo_camera* cam, SfMask* mask) {
  if (!sf_depth_masks(c, D, width, height)) return SF_OK;
  mask->p = (const uint8_t*)c->dp_mask.p; mask->pitch = pitch; mask->stride = image_stride;
  return sf_launch_depth_mask(c, D, n, width, height, cam->min_depth, cam->max_depth, (uint8_t*)c->dp_mask.p, pitch, image_stride);
}

// n keyframes from device images to n store slots in ONE launch sequence: detector, stereo correspondence and
// extraction each run once over the batch (blockIdx = image), the corner counts stay in device memory between them, the
// host never waits.  Same per-keyframe results as sf_get_features_and_descriptor.  In three parts, shared by the eight stereo
// batch calls (`family`) and the two depth batch calls (`in`: depth images in place of the right images, under every family):
// batch_check refuses (nothing is touched; n_keyframes = 0 passes without a look at the images), batch_reserve takes the
// store slots and the call's buffers, batch_launch queues the three stages, chunk by chunk.
static int batch_check(sf_context* c, BatchFamily family, const SecondInput& in, bool images, int n_keyframes, int width, int height,
                       int pitch, size_t image_stride, const sf_detector_params* det, BatchPlan* plan) {
  const SfFeatureType& t = sf_type_of(c);
  if (t.family != family && t.other_call) return sf_fail(c, SF_EINVAL, "%s", t.other_call);   // a type with calls of its own
  if (t.family != family) {
    const SfFeatureType& need = sf_type_of_family(family);
    return sf_fail(c, SF_EINVAL, "Vis/FeatureType %d: the %s batch calls need type %d (%s); use %s / %s", t.type, need.name, need.type,
                   need.setter, t.get_features_batch, t.add_keyframes_batch);
  }
  int rc;
  if (n_keyframes > 0) {
    if (!images || width < 3 || height < 3 || pitch < width)
      return sf_fail(c, SF_EINVAL, "%s%s%s missing or malformed (%d x %d, pitch %d)", in.call, colon(in.call),
                     in.depth ? "images" : "stereo pairs", width, height, pitch);
    if (image_stride < (size_t)pitch * height)
      return sf_fail(c, SF_EINVAL, "%s%simage stride %zu is less than an image (%d rows of pitch %d)", in.call, colon(in.call),
                     image_stride, height, pitch);
  }
  if (in.depth && (rc = depth_batch_check(c, in.call, in.depth, n_keyframes, width, height)) != SF_OK) return rc;
  if (n_keyframes == 0) return SF_OK;
  if ((rc = sf_front_plan(c, width, height, &plan->front)) != SF_OK) return rc;
  plan->dp = arg_or_defaults(det, sf_detector_defaults);
  if ((rc = check_max_features(c, "", plan->dp.max_features)) != SF_OK) return rc;
  if ((rc = sf_check_gftt(c, plan->dp.quality_level, plan->dp.min_distance)) != SF_OK) return rc;
  if ((rc = sf_grid_plan(c, width, height, plan->dp.max_features, &plan->front)) != SF_OK) return rc;
  if (plan->front.grid() && (long long)n_keyframes * plan->front.rows * plan->front.cols > 65535)
    return sf_fail(c, SF_ERANGE, "%d keyframes of %d x %d cells: at most 65535 cells per call", n_keyframes, plan->front.rows, plan->front.cols);
  plan->prm = arg_or_defaults(in.flow, sf_stereo_flow_defaults);
  if (!c->stereo.optical_flow) {
    if ((rc = sf_check_block_match(c, plan->prm)) != SF_OK) return rc;
  } else if (!sf_stereo_flow_ok(plan->prm)) {
    return sf_fail(c, SF_EINVAL, "stereo flow parameters out of range (see sf_stereo_correspondences_device)");
  }
  if ((rc = sf_check_integral(c, width, height)) != SF_OK) return rc;
  return family_check(c, family, n_keyframes, width, height);
}

static int batch_reserve(sf_context* c, const SecondInput& in, int n, int width, int height, size_t image_stride, BatchPlan* plan) {
  int rc;
  SF_HIP(c, hipSetDevice(c->device));
  if (in.depth && c->depth.depth_as_mask && (rc = sf_buf_reserve(c, c->dp_mask, (size_t)n * image_stride)) != SF_OK) return rc;
  if ((rc = sf_extract_kind(c, &plan->kind)) != SF_OK) return rc;
  const int maxf = plan->front.rows_cap;                   // rows per keyframe: max_features, or the grid's R C quota
  const size_t rows_all = (size_t)maxf * n;
  if ((rc = sf_buf_reserve(c, c->ft_kpts, rows_all * sizeof(sf_keypoint))) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->ft_flow, rows_all * 16)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->ft_counts, (size_t)n * 4)) != SF_OK) return rc;
  if ((rc = sf_store_reserve(c, c->store, c->store.slots + n, maxf, plan->kind.bytes)) != SF_OK) return rc;
  return family_reserve(c, sf_type_of(c), n, width, height);
}

// The stages behind the detector -- refinement, stereo correspondence, extraction -- for the m images from i0 on of a batch
// of n whose keypoints and counts the detector has left in c->ft_kpts / c->ft_counts: every array at that sub-range, the
// store slots from slot + i0 on
static int batch_follow(sf_context* c, const BatchPlan& plan, const ExtractKind& kind, const uint8_t* d_left, const uint8_t* d_right,
                        int n, int i0, int m, int width, int height, int pitch, size_t image_stride, const sf_stereo_camera* cam,
                        int slot, int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out,
                        const SfDepthIn* depth_all = nullptr) {
  const int maxf = plan.front.rows_cap;
  const size_t rows_all = (size_t)maxf * n, r0 = (size_t)maxf * i0;
  const FrontPlan& fp = plan.front;
  int rc;
  d_left += (size_t)i0 * image_stride;
  if (d_right) d_right += (size_t)i0 * image_stride;
  sf_keypoint* d_kpts = (sf_keypoint*)c->ft_kpts.p + r0;
  const int32_t* d_n = (const int32_t*)c->ft_counts.p + i0;
  if (fp.launch() &&
      (rc = sf_launch_corner_subpix(c, d_left, image_stride, m, width, height, pitch, d_kpts, maxf, d_n, maxf, fp.off_x(), fp.off_y(),
                                    fp.refine ? c->front.subpix_win_size : 0, c->front.subpix_iterations, c->front.subpix_eps)) != SF_OK)
    return rc;
  if (depth_all) {                                       // a depth keyframe: no stereo stage, the 3D points inside the extraction
    SfDepthIn depth = *depth_all;
    depth.p = (const char*)depth.p + (size_t)i0 * depth.stride;
    return sf_launch_extract_batch(c, d_left, image_stride, m, width, height, pitch, d_kpts, nullptr, nullptr, maxf, d_n, cam, kind,
                                   slot + i0, d_desc_out ? d_desc_out + r0 * kind.bytes : nullptr, d_xyz_out ? d_xyz_out + 3 * r0 : nullptr,
                                   d_kpts_out ? d_kpts_out + r0 : nullptr, d_rows_out ? d_rows_out + i0 : nullptr, &depth);
  }
  float* d_xy = (float*)c->ft_flow.p;                    // [n][maxf][2], then x [n][maxf], then status [n][maxf]
  float* d_rx = d_xy + 2 * rows_all;
  uint8_t* d_status = (uint8_t*)(d_rx + rows_all);
  d_xy += 2 * r0; d_rx += r0; d_status += r0;
  rc = c->stereo.optical_flow
           ? sf_launch_stereo_flow_batch(c, d_left, d_right, image_stride, m, width, height, pitch, d_kpts, maxf, d_n, &plan.prm, d_xy,
                                         d_status, d_rx, nullptr)
           : sf_launch_stereo_bm_batch(c, d_left, d_right, image_stride, m, width, height, pitch, d_kpts, maxf, d_n, &plan.prm,
                                       c->stereo.ssd, d_xy, d_status, d_rx, nullptr);
  if (rc != SF_OK) return rc;
  return sf_launch_extract_batch(c, d_left, image_stride, m, width, height, pitch, d_kpts, d_rx, d_status, maxf, d_n, cam, kind,
                                 slot + i0, d_desc_out ? d_desc_out + r0 * kind.bytes : nullptr, d_xyz_out ? d_xyz_out + 3 * r0 : nullptr,
                                 d_kpts_out ? d_kpts_out + r0 : nullptr, d_rows_out ? d_rows_out + i0 : nullptr);
}

// One loop over chunks, detector then the stages behind it.  A batch is one chunk, but under SIFT: its Gaussian planes are too
// large to keep for a whole batch, so a chunk's extraction reads them before the next chunk's detector overwrites them
static int batch_launch(sf_context* c, const BatchPlan& plan, const uint8_t* d_left, const uint8_t* d_right, int n, int width,
                        int height, int pitch, size_t image_stride, const sf_stereo_camera* cam, int32_t* first_slot_out,
                        int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out,
                        const SfDepthIn* depth = nullptr, const SfMask& mask = SfMask()) {
  const SfFeatureType& t = sf_type_of(c);
  const int slot = c->store.slots;
  ExtractKind kind = plan.kind;
  int rc, chunk = n;
  if (t.family == BATCH_SIFT) {
    chunk = c->sift_batch.chunk;
    if ((rc = sf_sift_batch_begin(c)) != SF_OK) return rc;
  }
  for (int i0 = 0; i0 < n; i0 += chunk) {
    const int m = std::min(chunk, n - i0);
    if ((rc = family_detect(c, t, plan, &kind, d_left, image_stride, i0, m, width, height, pitch, mask)) != SF_OK) return rc;
    if ((rc = batch_follow(c, plan, kind, d_left, d_right, n, i0, m, width, height, pitch, image_stride, cam, slot, d_rows_out,
                           d_desc_out, d_xyz_out, d_kpts_out, depth)) != SF_OK)
      return rc;
  }
  c->store.slots += n;
  if (first_slot_out) *first_slot_out = slot;
  return SF_OK;
}

static int features_batch(sf_context* c, BatchFamily family, const uint8_t* d_left, const SecondInput& in, int32_t n_keyframes,
                          int32_t width, int32_t height, int32_t pitch, size_t image_stride, const sf_stereo_camera* cam,
                          const sf_detector_params* det, int32_t* first_slot_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                          float* d_xyz_out, sf_keypoint* d_kpts_out) {
  if (!c || !cam || n_keyframes < 0) return SF_EINVAL;
  BatchPlan plan;
  int rc = batch_check(c, family, in, d_left && (in.depth || in.right), n_keyframes, width, height, pitch, image_stride, det, &plan);
  if (rc != SF_OK) return rc;
  if (n_keyframes == 0) { if (first_slot_out) *first_slot_out = c->store.slots; return SF_OK; }
  if ((rc = batch_reserve(c, in, n_keyframes, width, height, image_stride, &plan)) != SF_OK) return rc;
  SfMask mask;
  if (in.depth && (rc = depth_batch_mask(c, *in.depth, n_keyframes, width, height, pitch, image_stride, cam, &mask)) != SF_OK) return rc;
  return batch_launch(c, plan, d_left, in.right, n_keyframes, width, height, pitch, image_stride, cam, first_slot_out, d_rows_out,
                      d_desc_out, d_xyz_out, d_kpts_out, in.depth, mask);
}

extern "C" int sf_get_features_and_descriptor_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                           int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                                           size_t image_stride, const sf_stereo_camera* cam,
                                                           const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                                           int32_t* first_slot_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                           float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return features_batch(c, BATCH_GENERIC, d_left, {d_right, flow}, n_keyframes, width, height, pitch, image_stride, cam, det, first_slot_out,
                        d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_get_features_and_descriptor_orb_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                               int32_t n_keyframes, int32_t width, int32_t height,
                                                               int32_t pitch, size_t image_stride, const sf_stereo_camera* cam,
                                                               const sf_detector_params* det,
                                                               const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                               int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out,
                                                               sf_keypoint* d_kpts_out) {
  return features_batch(c, BATCH_ORB, d_left, {d_right, flow}, n_keyframes, width, height, pitch, image_stride, cam, det, first_slot_out,
                        d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_get_features_and_descriptor_surf_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                                int32_t n_keyframes, int32_t width, int32_t height,
                                                                int32_t pitch, size_t image_stride, const sf_stereo_camera* cam,
                                                                const sf_detector_params* det,
                                                                const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                                int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out,
                                                                sf_keypoint* d_kpts_out) {
  return features_batch(c, BATCH_SURF, d_left, {d_right, flow}, n_keyframes, width, height, pitch, image_stride, cam, det, first_slot_out,
                        d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

// How many keyframes of the most recent SURF / SIFT batch call overflowed and hold no rows (word 0 of the family's control
// buffer): waits for the stream, `message` says what overflowed, with the count
static int batch_status(sf_context* c, Buf sf_context::*control, const char* message, int32_t* n_overflowed_out) {
  if (!c) return SF_EINVAL;
  if (n_overflowed_out) *n_overflowed_out = 0;
  SF_HIP(c, hipSetDevice(c->device));
  int32_t n = 0;
  const Buf& ctl = c->*control;
  if (ctl.p) {
    const int rc = sf_word_to_host(c, ctl.p, &n);
    if (rc != SF_OK) return rc;
  } else {
    SF_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (n_overflowed_out) *n_overflowed_out = n;
  return n > 0 ? sf_fail(c, SF_ERANGE, message, n) : SF_OK;
}

extern "C" int sf_surf_batch_status(sf_handle c, int32_t* n_overflowed_out) {
  return batch_status(c, &sf_context::surf_ctl, "SURF: %d keyframe(s) of the last batch call had more maxima than the candidate capacity and hold no rows; raise hessian_threshold",
                      n_overflowed_out);
}

extern "C" int sf_get_features_and_descriptor_sift_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                                int32_t n_keyframes, int32_t width, int32_t height,
                                                                int32_t pitch, size_t image_stride, const sf_stereo_camera* cam,
                                                                const sf_detector_params* det,
                                                                const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                                int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out,
                                                                sf_keypoint* d_kpts_out) {
  return features_batch(c, BATCH_SIFT, d_left, {d_right, flow}, n_keyframes, width, height, pitch, image_stride, cam, det, first_slot_out,
                        d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_sift_batch_status(sf_handle c, int32_t* n_overflowed_out) {
  return batch_status(c, &sf_context::sift_ctl, "SIFT: %d keyframe(s) of the last batch call had more extrema or keypoints than the capacity of an image and hold no rows; raise contrast_threshold",
                      n_overflowed_out);
}

// ---- the camera's own images (kernels in k_image.hip, k_cnn.hip) ---------------------------------------------------
extern "C" int sf_image_set_gray_rule(sf_handle c, int32_t rule) {
  if (!c) return SF_EINVAL;
  int k[4];
  if (!sf_gray_rule(rule, &k[0], &k[1], &k[2], &k[3]))
    return sf_fail(c, SF_EINVAL, "gray rule %d unknown (0 = OpenCV 3.x, 1 = OpenCV 4.x)", rule);
  c->gray_rule = rule;
  return SF_OK;
}

extern "C" int sf_image_get_gray_rule(sf_handle c, int32_t* rule) {
  if (!c || !rule) return SF_EINVAL;
  *rule = c->gray_rule;
  return SF_OK;
}

// an array of n images `stride` bytes apart: the last image needs its rows only, not a whole stride
static int check_stride(sf_context* c, int n, size_t stride, int pitch, int height, long long last_row, const char* what) {
  if (n > 1 && stride < (size_t)pitch * (height - 1) + (size_t)last_row)
    return sf_fail(c, SF_EINVAL, "%s stride %zu is less than an image (%d rows of pitch %d)", what, stride, height, pitch);
  return SF_OK;
}

extern "C" int sf_image_to_gray_device(sf_handle c, const uint8_t* d_src, int32_t format, int32_t width, int32_t height,
                                       int32_t src_pitch, size_t src_stride, int32_t n_images, uint8_t* d_dst,
                                       int32_t dst_pitch, size_t dst_stride) {
  if (!c || n_images < 0) return SF_EINVAL;
  int rc = check_format(c, format);
  if (rc != SF_OK) return rc;
  if (n_images == 0) return SF_OK;
  if ((rc = check_camera_image(c, "", d_src, format, width, height, src_pitch, 1, "source images")) != SF_OK) return rc;
  if ((rc = sf_check_image(c, d_dst, width, height, dst_pitch, 1, "gray planes")) != SF_OK) return rc;
  if ((rc = check_stride(c, n_images, src_stride, src_pitch, height, image_row_bytes(format, width), "source")) != SF_OK) return rc;
  if ((rc = check_stride(c, n_images, dst_stride, dst_pitch, height, width, "destination")) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_image_gray(c, d_src, nullptr, n_images, format, c->gray_rule, width, height, src_pitch, src_stride, n_images,
                              d_dst, dst_pitch, dst_stride);
}

extern "C" int sf_netvlad_infer_u8_batch_device(sf_handle c, const uint8_t* d_images, int32_t format, int32_t n_images,
                                                int32_t width, int32_t height, int32_t pitch, size_t image_stride,
                                                float* d_out, int32_t n_out) {
  if (!c || !d_out) return SF_EINVAL;
  int rc = check_camera_image(c, "", d_images, format, width, height, pitch, 1, "images");
  if (rc != SF_OK) return rc;
  if ((rc = check_stride(c, n_images, image_stride, pitch, height, image_row_bytes(format, width), "image")) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_netvlad_infer_u8_batch_impl(c, d_images, format, n_images, height, width, pitch, image_stride, d_out, n_out);
}

extern "C" int sf_netvlad_load(sf_handle c, const sf_netvlad_weights* w) {
  if (!c) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_netvlad_load_impl(c, w);
}

extern "C" int sf_netvlad_infer_device(sf_handle c, const float* d_image_rgb, int32_t width, int32_t height, float* d_out,
                                       int32_t n_out) {
  if (!c || !d_image_rgb || !d_out) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_netvlad_infer_impl(c, d_image_rgb, height, width, d_out, n_out);
}

extern "C" int sf_netvlad_infer_batch_device(sf_handle c, const float* d_images_rgb, int32_t n_images, int32_t width,
                                             int32_t height, float* d_out, int32_t n_out) {
  if (!c || !d_images_rgb || !d_out) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_netvlad_infer_batch_impl(c, d_images_rgb, n_images, height, width, d_out, n_out);
}

// what the calls that add NetVLAD rows need of the loaded model; *dims_out: the columns of a row
static int check_netvlad_rows(sf_context* c, const char* call, int n, int width, int height, int* dims_out) {
  const int dims = *dims_out = c->params.netvlad_dimensions, pca_dim = sf_netvlad_pca_dim(c);
  if (pca_dim == 0) return sf_fail(c, SF_EINVAL, "%s%sno NetVLAD model loaded (sf_netvlad_load)", call, colon(call));
  if (dims < 1 || dims > pca_dim)
    return sf_fail(c, SF_EINVAL, "%s%snetvlad_dimensions %d is beyond the loaded model's %d WPCA outputs", call, colon(call), dims, pca_dim);
  return sf_netvlad_check(c, n, height, width, dims);
}

// get_keyframes + compute_descriptors for n keyframes (data_handler.py:143-164, 212-295): gray planes of all 2 n stereo
// images, or of the n images of depth keyframes (one launch), the network on the colour images, the batch feature stages on
// the planes, the descriptors' prefix into the local NN rows.  Everything that can refuse does so before the first launch;
// the store and the NN database grow last, together.
static int add_keyframes_batch(sf_context* c, BatchFamily family, const uint8_t* d_left, const SecondInput& in, const uint8_t* d_rgb,
                               int32_t format, int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                               size_t image_stride, const sf_stereo_camera* cam, const sf_detector_params* det,
                               int32_t* first_slot_out, int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                               float* d_xyz_out, sf_keypoint* d_kpts_out) {
  if (!c || !cam || n_keyframes < 0) return SF_EINVAL;
  const int n = n_keyframes, planes = in.depth ? n : 2 * n;
  int rc;
  if ((rc = check_format(c, format)) != SF_OK) return rc;
  if (n > 0) {
    if ((rc = check_camera_image(c, in.call, d_left && (in.depth || in.right), format, width, height, pitch, 3,
                                 in.depth ? "images" : "stereo pairs")) != SF_OK)
      return rc;
    if (image_stride < (size_t)pitch * height)
      return sf_fail(c, SF_EINVAL, "%s%simage stride %zu is less than an image (%d rows of pitch %d)", in.call, colon(in.call),
                     image_stride, height, pitch);
  }
  // the planes this call makes: rows padded to 16 bytes, n left then, of stereo pairs, n right
  const int g_pitch = n > 0 ? (width + 15) & ~15 : 0;
  const size_t g_stride = ((size_t)g_pitch * (n > 0 ? height : 0) + 255) & ~(size_t)255;
  BatchPlan plan;
  if ((rc = batch_check(c, family, in, true, n, width, height, g_pitch, g_stride, det, &plan)) != SF_OK) return rc;
  if (n == 0) {
    if (first_slot_out) *first_slot_out = c->store.slots;
    if (first_nn_row_out) *first_nn_row_out = c->nn_local.n;
    return SF_OK;
  }
  int dims;
  if ((rc = check_netvlad_rows(c, in.call, n, width, height, &dims)) != SF_OK) return rc;
  if ((rc = sf_nn_reserve_rows(c, c->nn_local, n, dims)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->img_gray, (size_t)planes * g_stride)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->img_desc, (size_t)n * dims * sizeof(float))) != SF_OK) return rc;
  if ((rc = batch_reserve(c, in, n, width, height, g_stride, &plan)) != SF_OK) return rc;
  uint8_t* g_left = (uint8_t*)c->img_gray.p;
  uint8_t* g_right = in.depth ? nullptr : g_left + (size_t)n * g_stride;
  if ((rc = sf_launch_image_gray(c, d_left, in.right, n, format, c->gray_rule, width, height, pitch, image_stride, planes, g_left,
                                 g_pitch, g_stride)) != SF_OK)
    return rc;
  if ((rc = sf_netvlad_infer_u8_batch_impl(c, d_rgb ? d_rgb : d_left, format, n, height, width, pitch, image_stride,
                                           (float*)c->img_desc.p, dims)) != SF_OK)
    return rc;
  SfMask mask;
  if (in.depth && (rc = depth_batch_mask(c, *in.depth, n, width, height, g_pitch, g_stride, cam, &mask)) != SF_OK) return rc;
  int32_t slot = -1;
  if ((rc = batch_launch(c, plan, g_left, g_right, n, width, height, g_pitch, g_stride, cam, &slot, d_rows_out, d_desc_out,
                         d_xyz_out, d_kpts_out, in.depth, mask)) != SF_OK)
    return rc;
  const int row = c->nn_local.n;
  if ((rc = sf_nn_append(c, c->nn_local, c->img_desc.p, n, dims, 1)) != SF_OK) {
    c->store.slots -= n;             // (the slots' rows stay behind the end of the store: the keyframes were never added)
    return rc;
  }
  if (first_slot_out) *first_slot_out = slot;
  if (first_nn_row_out) *first_nn_row_out = row;
  return SF_OK;
}

extern "C" int sf_add_keyframes_u8_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                const uint8_t* d_rgb, int32_t format, int32_t n_keyframes, int32_t width,
                                                int32_t height, int32_t pitch, size_t image_stride,
                                                const sf_stereo_camera* cam, const sf_detector_params* det,
                                                const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return add_keyframes_batch(c, BATCH_GENERIC, d_left, {d_right, flow}, d_rgb, format, n_keyframes, width, height, pitch, image_stride, cam, det,
                             first_slot_out, first_nn_row_out, d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_add_keyframes_orb_u8_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                    const uint8_t* d_rgb, int32_t format, int32_t n_keyframes, int32_t width,
                                                    int32_t height, int32_t pitch, size_t image_stride,
                                                    const sf_stereo_camera* cam, const sf_detector_params* det,
                                                    const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                    int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                    float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return add_keyframes_batch(c, BATCH_ORB, d_left, {d_right, flow}, d_rgb, format, n_keyframes, width, height, pitch, image_stride, cam, det,
                             first_slot_out, first_nn_row_out, d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_add_keyframes_surf_u8_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                     const uint8_t* d_rgb, int32_t format, int32_t n_keyframes, int32_t width,
                                                     int32_t height, int32_t pitch, size_t image_stride,
                                                     const sf_stereo_camera* cam, const sf_detector_params* det,
                                                     const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                     int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                     float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return add_keyframes_batch(c, BATCH_SURF, d_left, {d_right, flow}, d_rgb, format, n_keyframes, width, height, pitch, image_stride, cam, det,
                             first_slot_out, first_nn_row_out, d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_add_keyframes_sift_u8_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                     const uint8_t* d_rgb, int32_t format, int32_t n_keyframes, int32_t width,
                                                     int32_t height, int32_t pitch, size_t image_stride,
                                                     const sf_stereo_camera* cam, const sf_detector_params* det,
                                                     const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                     int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                     float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return add_keyframes_batch(c, BATCH_SIFT, d_left, {d_right, flow}, d_rgb, format, n_keyframes, width, height, pitch, image_stride, cam, det,
                             first_slot_out, first_nn_row_out, d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

// ---- the batch forms of the depth keyframes: one call for every family (the handle's own), the stages of
// sf_get_features_and_descriptor_depth in one launch sequence -- masks of all n depth images, detector under them, refinement,
// extraction with depth points; the flow defaults stand in for the stereo stage's parameters --------------------------------
extern "C" int sf_get_features_and_descriptor_depth_batch_device(sf_handle c, const uint8_t* d_images, const void* d_depth,
                                                                 int32_t depth_format, int32_t n_keyframes, int32_t width,
                                                                 int32_t height, int32_t image_pitch, size_t image_stride,
                                                                 int32_t depth_pitch, size_t depth_stride,
                                                                 const sf_stereo_camera* cam, const sf_detector_params* det,
                                                                 int32_t* first_slot_out, int32_t* d_rows_out,
                                                                 uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out) {
  if (!c) return SF_EINVAL;
  SfDepthIn D{d_depth, depth_format, depth_pitch, depth_stride};
  return features_batch(c, sf_type_of(c).family, d_images, {nullptr, nullptr, &D, "sf_get_features_and_descriptor_depth_batch_device"},
                        n_keyframes, width, height, image_pitch, image_stride, cam, det, first_slot_out, d_rows_out, d_desc_out,
                        d_xyz_out, d_kpts_out);
}

extern "C" int sf_add_keyframes_depth_batch_device(sf_handle c, const uint8_t* d_images, int32_t image_format, const void* d_depth,
                                                   int32_t depth_format, int32_t n_keyframes, int32_t width, int32_t height,
                                                   int32_t image_pitch, size_t image_stride, int32_t depth_pitch,
                                                   size_t depth_stride, const sf_stereo_camera* cam,
                                                   const sf_detector_params* det, int32_t* first_slot_out,
                                                   int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                   float* d_xyz_out, sf_keypoint* d_kpts_out) {
  if (!c) return SF_EINVAL;
  SfDepthIn D{d_depth, depth_format, depth_pitch, depth_stride};
  return add_keyframes_batch(c, sf_type_of(c).family, d_images, {nullptr, nullptr, &D, "sf_add_keyframes_depth_batch_device"}, nullptr,
                             image_format, n_keyframes, width, height, image_pitch, image_stride, cam, det, first_slot_out,
                             first_nn_row_out, d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}
