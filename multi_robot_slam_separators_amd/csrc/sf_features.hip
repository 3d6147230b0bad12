// sf_features.hip -- entry points of the feature front-end: BRIEF / ORB test tables, the FREAK tables, Vis/FeatureType, NetVLAD, corner
// detection (GFTT, FAST, ORB, SURF, SIFT), the ROI, the grid of cells and the sub-pixel refinement around it, stereo correspondence,
// keyframe extraction and the camera-image forms of these calls (kernels in k_extract.hip, k_gftt.hip, k_fast.hip,
// k_orb_detect.hip, k_freak.hip, k_surf.hip, k_sift.hip, k_subpix.hip, k_grid.hip, k_lk.hip, k_stereo_bm.hip, k_cnn.hip, k_image.hip; the detectors' sort in
// sf_sort.hip).
#include <cmath>
#include <vector>

#include "sf_host.hpp"

// ---- the checks the entry points below share ---------------------------------------------------------------------
// `present`: every image pointer of the call is there; min_side 3 where a detector runs (its 3 x 3 neighbourhoods)
static int check_image(sf_context* c, bool present, int width, int height, int pitch, int min_side, const char* what) {
  if (!present || width < min_side || height < min_side || pitch < width)
    return sf_fail(c, SF_EINVAL, "%s missing or malformed (%d x %d, pitch %d)", what, width, height, pitch);
  return SF_OK;
}

// a camera image (sf_image_format): a row holds 3 bytes per pixel for the colour formats
static int check_format(sf_context* c, int format) {
  if (format != SF_IMAGE_RGB8 && format != SF_IMAGE_BGR8 && format != SF_IMAGE_MONO8)
    return sf_fail(c, SF_EINVAL, "image format %d unknown (0 = rgb8, 1 = bgr8, 2 = mono8)", format);
  return SF_OK;
}

static long long image_row_bytes(int format, int width) { return (long long)width * (format == SF_IMAGE_MONO8 ? 1 : 3); }

static int check_camera_image(sf_context* c, bool present, int format, int width, int height, int pitch, int min_side,
                              const char* what) {
  int rc = check_format(c, format);
  if (rc != SF_OK) return rc;
  if (!present || width < min_side || height < min_side || pitch < image_row_bytes(format, width))
    return sf_fail(c, SF_EINVAL, "%s missing or malformed (%d x %d, pitch %d, %d byte(s) per pixel)", what, width, height, pitch,
                   format == SF_IMAGE_MONO8 ? 1 : 3);
  return SF_OK;
}

// the detectors' sort keys hold a pixel index beside a score
static int check_pixels(sf_context* c, int width, int height) {
  if ((long long)width * height > (1ll << 26)) return sf_fail(c, SF_ERANGE, "image of %d x %d pixels is too large", width, height);
  return SF_OK;
}

// every feature type here writes binary rows into the keyframe store
static int check_binary_rows(sf_context* c, int feature_type) {
  const char* name = feature_type == 2 ? "ORB" : feature_type == 4 ? "FAST/BRIEF" : feature_type == 8 ? "GFTT/ORB" :
                     feature_type == 3 ? "FAST/FREAK" : feature_type == 5 ? "GFTT/FREAK" : "GFTT/BRIEF";
  if (c->params.desc_type != 0)
    return sf_fail(c, SF_EINVAL, "%s writes binary descriptors: a handle with desc_type %d cannot store them", name, c->params.desc_type);
  return SF_OK;
}

static int check_gftt(sf_context* c, double quality_level, double min_distance) {
  if (!(quality_level > 0.0) || !(min_distance >= 0.0))
    return sf_fail(c, SF_EINVAL, "qualityLevel must be > 0 and minDistance >= 0 (cv::goodFeaturesToTrack asserts the same)");
  return SF_OK;
}

// the types whose corners come from the FAST detector (the others of 3 .. 8: GFTT)
static bool fast_corners(int feature_type) { return feature_type == 4 || feature_type == 3; }

// the caller's parameter block, or the defaults when it passed none
template <class T>
static T arg_or_defaults(const T* given, void (*defaults)(T*)) {
  T v;
  if (given) v = *given; else defaults(&v);
  return v;
}

// ---- feature extraction (kernels in k_extract.hip) ----------------------------------
static int brief_upload(sf_context* c) {
  int rc;
  if ((rc = sf_buf_reserve(c, c->brief_tests, sizeof c->brief_host)) != SF_OK) return rc;
  SF_HIP(c, hipMemcpyAsync(c->brief_tests.p, c->brief_host, (size_t)c->brief_bytes * 32, hipMemcpyHostToDevice, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));   // (the host table may change right after the call returns)
  return SF_OK;
}

extern "C" int sf_brief_set_pattern(sf_handle c, const int8_t* tests, int32_t bytes) {
  if (!c || !tests) return SF_EINVAL;
  if (bytes != 16 && bytes != 32 && bytes != 64) return sf_fail(c, SF_ERANGE, "BRIEF descriptors are 16, 32 or 64 bytes, not %d", bytes);
  for (int t = 0; t < bytes * 32; ++t)
    if (tests[t] < -24 || tests[t] > 24) return sf_fail(c, SF_ERANGE, "BRIEF test offset %d outside the 48 px patch", (int)tests[t]);
  SF_HIP(c, hipSetDevice(c->device));
  memcpy(c->brief_host, tests, (size_t)bytes * 32);
  c->brief_bytes = bytes;
  return brief_upload(c);
}

static int brief_ensure(sf_context* c) {
  int rc = check_binary_rows(c, c->feature_type);
  if (rc != SF_OK) return rc;
  if (c->brief_bytes) return SF_OK;
  const int want = c->params.desc_bytes;
  c->brief_bytes = (want == 16 || want == 64) ? want : 32;
  sf_brief_default_pattern(c->brief_host, c->brief_bytes);
  return brief_upload(c);
}

extern "C" int sf_brief_get_pattern(sf_handle c, int8_t* tests, int32_t cap_bytes, int32_t* bytes) {
  if (!c || !bytes) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  int rc = brief_ensure(c);
  if (rc != SF_OK) return rc;
  *bytes = c->brief_bytes;
  if (tests) {
    if (cap_bytes < c->brief_bytes) return sf_fail(c, SF_ERANGE, "pattern buffer holds %d of %d descriptor bytes", cap_bytes, c->brief_bytes);
    memcpy(tests, c->brief_host, (size_t)c->brief_bytes * 32);
  }
  return SF_OK;
}

// ---- GFTT/ORB (Vis/FeatureType 8) --------------------------------------------------------------------------------
extern "C" void sf_orb_defaults(sf_orb_params* p) {
  if (!p) return;
  p->edge_threshold = 19;      // ORB/EdgeThreshold [upstream rtabmap Parameters.h]
  p->patch_size = 31;          // ORB/PatchSize
  p->wta_k = 2;                // ORB/WTA_K
  p->orientation = 0;          // rtabmap's GFTT/ORB: the keypoint's own angle
}

static int orb_validate(sf_context* c, const sf_orb_params& o) {
  if (o.edge_threshold < 1 || o.edge_threshold > 64)
    return sf_fail(c, SF_EINVAL, "ORB edge_threshold %d outside 1 .. 64", o.edge_threshold);
  if (o.patch_size != 31) return sf_fail(c, SF_EINVAL, "ORB patch_size %d: only 31 is built", o.patch_size);
  if (o.wta_k != 2) return sf_fail(c, SF_EINVAL, "ORB wta_k %d: only 2 (32-byte rows) is built", o.wta_k);
  if (o.orientation != 0 && o.orientation != 1)
    return sf_fail(c, SF_EINVAL, "ORB orientation %d unknown (0 = the keypoint's angle, 1 = intensity centroid)", o.orientation);
  if (o.orientation == 1 && o.edge_threshold < 16)
    return sf_fail(c, SF_EINVAL, "ORB orientation 1 needs edge_threshold >= 16 (the radius-15 patch), not %d", o.edge_threshold);
  return SF_OK;
}

static int orb_upload(sf_context* c) {
  int rc;
  if ((rc = sf_buf_reserve(c, c->orb_tests, sizeof c->orb_host)) != SF_OK) return rc;
  SF_HIP(c, hipMemcpyAsync(c->orb_tests.p, c->orb_host, sizeof c->orb_host, hipMemcpyHostToDevice, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));   // (the host table may change right after the call returns)
  c->orb_loaded = true;
  return SF_OK;
}

extern "C" int sf_set_feature_type(sf_handle c, int32_t feature_type, const sf_orb_params* orb) {
  if (!c) return SF_EINVAL;
  int rc;
  switch (feature_type) {
    case 6:                      // (a handle with desc_type 1 starts here and may stay; none goes back from SURF)
      if (c->feature_type != 6 && (rc = check_binary_rows(c, 6)) != SF_OK) return rc;
      break;
    case 4:
      if ((rc = check_binary_rows(c, 4)) != SF_OK) return rc;
      break;
    case 8: {
      if ((rc = check_binary_rows(c, 8)) != SF_OK) return rc;
      const sf_orb_params o = arg_or_defaults(orb, sf_orb_defaults);
      if ((rc = orb_validate(c, o)) != SF_OK) return rc;
      c->orb = o;
      break;
    }
    case 2:
      return sf_fail(c, SF_EINVAL, "Vis/FeatureType 2 (ORB) takes detector parameters: select it with sf_set_feature_type_orb");
    case 0:
      return sf_fail(c, SF_EINVAL, "Vis/FeatureType 0 (SURF) takes parameters of its own and a handle with desc_type 1: select it with sf_set_feature_type_surf");
    case 3:
    case 5:
      return sf_fail(c, SF_EINVAL, "Vis/FeatureType %d (%s/FREAK) takes parameters of its own: select it with sf_set_feature_type_freak",
                     feature_type, feature_type == 3 ? "FAST" : "GFTT");
    case 1:
      return sf_fail(c, SF_EINVAL, "Vis/FeatureType 1 (SIFT) takes parameters of its own and a handle with desc_type 1 and desc_bytes 512: select it with sf_set_feature_type_sift");
    default:
      return sf_fail(c, SF_EINVAL, "Vis/FeatureType %d is not built (1 = SIFT by sf_set_feature_type_sift, 0 = SURF by sf_set_feature_type_surf, 2 = ORB by sf_set_feature_type_orb, 3 = FAST/FREAK and 5 = GFTT/FREAK by sf_set_feature_type_freak, 4 = FAST/BRIEF, 6 = GFTT/BRIEF, 8 = GFTT/ORB)",
                     feature_type);
  }
  c->feature_type = feature_type;
  return SF_OK;
}

// ---- ORB (Vis/FeatureType 2; detector kernels in k_orb_detect.hip) ------------------------------------------------
extern "C" void sf_orb_detector_defaults(sf_orb_detector_params* p) {
  if (!p) return;
  p->scale_factor = 2.0f;      // ORB/ScaleFactor [upstream rtabmap Parameters.h; OpenCV's own default is 1.2]
  p->n_levels = 3;             // ORB/NLevels [rtabmap; OpenCV 8]
  p->first_level = 0;          // ORB/FirstLevel
  p->score_type = 0;           // ORB/ScoreType: HARRIS_SCORE
  p->fast_threshold = 20;      // ORB/FastThreshold
}

static int orb_detector_validate(sf_context* c, const sf_orb_detector_params& d, const sf_orb_params& o) {
  if (!(d.scale_factor > 1.0f) || !(d.scale_factor <= 4.0f))
    return sf_fail(c, SF_EINVAL, "ORB scale_factor %g outside (1, 4]", (double)d.scale_factor);
  if (d.n_levels < 1 || d.n_levels > SF_ORB_MAX_LEVELS)
    return sf_fail(c, SF_EINVAL, "ORB n_levels %d outside 1 .. %d", d.n_levels, SF_ORB_MAX_LEVELS);
  if (d.first_level != 0) return sf_fail(c, SF_EINVAL, "ORB first_level %d: only 0 is built", d.first_level);
  if (d.score_type != 0 && d.score_type != 1)
    return sf_fail(c, SF_EINVAL, "ORB score_type %d unknown (0 = Harris, 1 = FAST)", d.score_type);
  if (d.fast_threshold < 1 || d.fast_threshold > 254)
    return sf_fail(c, SF_EINVAL, "ORB fast_threshold %d outside 1 .. 254", d.fast_threshold);
  // the detector always computes the intensity-centroid angle: the descriptor's parameters as under orientation 1 (the
  // radius-15 patch must stay inside a level, edge_threshold 16 .. 64), whatever the caller's orientation says
  sf_orb_params as_centroid = o;
  as_centroid.orientation = 1;
  return orb_validate(c, as_centroid);
}

extern "C" int sf_set_feature_type_orb(sf_handle c, const sf_orb_detector_params* det, const sf_orb_params* orb) {
  if (!c) return SF_EINVAL;
  int rc = check_binary_rows(c, 2);
  if (rc != SF_OK) return rc;
  const sf_orb_detector_params d = arg_or_defaults(det, sf_orb_detector_defaults);
  sf_orb_params o = arg_or_defaults(orb, sf_orb_defaults);
  if ((rc = orb_detector_validate(c, d, o)) != SF_OK) return rc;
  o.orientation = 1;           // always the intensity centroid, computed by the detector
  c->orb_det = d;
  c->orb = o;
  c->feature_type = 2;
  return SF_OK;
}

extern "C" int sf_get_orb_detector(sf_handle c, sf_orb_detector_params* out) {
  if (!c || !out) return SF_EINVAL;
  *out = c->orb_det;
  return SF_OK;
}

extern "C" int sf_detect_orb_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                    int32_t max_features, const sf_orb_detector_params* det, const sf_orb_params* orb,
                                    sf_keypoint* d_kpts_out, int32_t cap, int32_t* n_out) {
  if (!c || !n_out || cap < 0 || (cap > 0 && !d_kpts_out)) return SF_EINVAL;
  *n_out = 0;
  int rc = check_image(c, d_image, width, height, pitch, 3, "image");
  if (rc != SF_OK) return rc;
  if (max_features < 1) return sf_fail(c, SF_EINVAL, "ORB shares out max_features = %d keypoints over its levels: it must be >= 1", max_features);
  const sf_orb_detector_params d = det ? *det : c->orb_det;
  const sf_orb_params o = orb ? *orb : c->orb;
  if ((rc = orb_detector_validate(c, d, o)) != SF_OK) return rc;
  if ((rc = check_pixels(c, width, height)) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_detect_orb(c, d_image, width, height, pitch, max_features, &d, &o, d_kpts_out, cap, n_out);
}

extern "C" int sf_get_feature_type(sf_handle c, int32_t* feature_type, sf_orb_params* orb) {
  if (!c || !feature_type) return SF_EINVAL;
  *feature_type = c->feature_type;
  if (orb) *orb = c->orb;
  return SF_OK;
}

extern "C" int sf_orb_set_pattern(sf_handle c, const int8_t* tests, int32_t bytes) {
  if (!c || !tests) return SF_EINVAL;
  if (bytes != 32) return sf_fail(c, SF_EINVAL, "ORB descriptors (WTA_K 2) are 32 bytes, not %d", bytes);
  for (int t = 0; t < bytes * 32; ++t)
    if (tests[t] < -15 || tests[t] > 15) return sf_fail(c, SF_EINVAL, "ORB test coordinate %d outside the 31 px patch", (int)tests[t]);
  SF_HIP(c, hipSetDevice(c->device));
  memcpy(c->orb_host, tests, sizeof c->orb_host);
  return orb_upload(c);
}

static int orb_ensure(sf_context* c) {
  if (c->orb_loaded) return SF_OK;
  sf_orb_default_pattern(c->orb_host);
  return orb_upload(c);
}

extern "C" int sf_orb_get_pattern(sf_handle c, int8_t* tests, int32_t cap_bytes, int32_t* bytes) {
  if (!c || !bytes) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  int rc = orb_ensure(c);
  if (rc != SF_OK) return rc;
  *bytes = 32;
  if (tests) {
    if (cap_bytes < 32) return sf_fail(c, SF_ERANGE, "pattern buffer holds %d of 32 descriptor bytes", cap_bytes);
    memcpy(tests, c->orb_host, sizeof c->orb_host);
  }
  return SF_OK;
}

// ---- FAST/FREAK and GFTT/FREAK (Vis/FeatureType 3 and 5; kernel and table builders in k_freak.hip) -------------------
static int freak_validate(sf_context* c, const sf_freak_params& f) {
  if ((f.orientation_normalized != 0 && f.orientation_normalized != 1) || (f.scale_normalized != 0 && f.scale_normalized != 1))
    return sf_fail(c, SF_EINVAL, "FREAK orientation_normalized %d, scale_normalized %d: each is 0 or 1", f.orientation_normalized,
                   f.scale_normalized);
  if (!(f.pattern_scale > 0.0f) || !(f.pattern_scale <= 64.0f))
    return sf_fail(c, SF_EINVAL, "FREAK pattern_scale %g outside (0, 64]", (double)f.pattern_scale);
  if (f.n_octaves < 1 || f.n_octaves > 8) return sf_fail(c, SF_EINVAL, "FREAK n_octaves %d outside 1 .. 8", f.n_octaves);
  return SF_OK;
}

extern "C" int sf_set_feature_type_freak(sf_handle c, int32_t feature_type, const sf_freak_params* freak) {
  if (!c) return SF_EINVAL;
  if (feature_type != 3 && feature_type != 5)
    return sf_fail(c, SF_EINVAL, "sf_set_feature_type_freak selects Vis/FeatureType 3 (FAST/FREAK) or 5 (GFTT/FREAK), not %d", feature_type);
  int rc = check_binary_rows(c, feature_type);
  if (rc != SF_OK) return rc;
  const sf_freak_params f = arg_or_defaults(freak, sf_freak_defaults);
  if ((rc = freak_validate(c, f)) != SF_OK) return rc;
  if (memcmp(&f, &c->freak, sizeof f) != 0) c->freak_pattern_ok = c->freak_tables_ok = false;   // rebuilt by the next extraction
  c->freak = f;
  c->feature_type = feature_type;
  return SF_OK;
}

extern "C" int sf_get_freak_params(sf_handle c, sf_freak_params* out) {
  if (!c || !out) return SF_EINVAL;
  *out = c->freak;
  return SF_OK;
}

static const int32_t* freak_pairs(sf_context* c) {
  if (!c->freak_pairs_set) {
    sf_freak_default_pairs(c->freak_pairs);
    c->freak_pairs_set = true;
  }
  return c->freak_pairs;
}

extern "C" int sf_freak_set_pairs(sf_handle c, const int32_t* selected, int32_t n) {
  if (!c || !selected) return SF_EINVAL;
  if (n != FREAK_PAIRS) return sf_fail(c, SF_ERANGE, "FREAK descriptors are %d pairs, not %d", FREAK_PAIRS, n);
  for (int k = 0; k < n; ++k)
    if (selected[k] < 0 || selected[k] >= FREAK_ALL_PAIRS)
      return sf_fail(c, SF_ERANGE, "FREAK pair index %d (entry %d) outside [0, %d)", selected[k], k, FREAK_ALL_PAIRS);
  memcpy(c->freak_pairs, selected, sizeof c->freak_pairs);
  c->freak_pairs_set = true;
  c->freak_tables_ok = false;
  return SF_OK;
}

extern "C" int sf_freak_get_pairs(sf_handle c, int32_t* selected, int32_t cap, int32_t* n) {
  if (!c || !n) return SF_EINVAL;
  *n = FREAK_PAIRS;
  if (selected) {
    if (cap < FREAK_PAIRS) return sf_fail(c, SF_ERANGE, "pair buffer holds %d of %d indices", cap, FREAK_PAIRS);
    memcpy(selected, freak_pairs(c), sizeof c->freak_pairs);
  }
  return SF_OK;
}

// The device tables of the handle's FREAK parameters and pairs, built and uploaded when either has changed since the
// last upload (the pattern, 8.4 MB, only with the parameters)
static int freak_ensure(sf_context* c) {
  if (c->freak_pattern_ok && c->freak_tables_ok) return SF_OK;
  int rc;
  if ((rc = sf_buf_reserve(c, c->freak_pattern, FREAK_PATTERN_FLOATS * sizeof(float))) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->freak_tables, FREAK_TABLE_BYTES)) != SF_OK) return rc;
  uint8_t* tables = c->freak_tables_host;
  std::vector<float> pattern;
  if (!c->freak_pattern_ok) {
    pattern.resize(FREAK_PATTERN_FLOATS);
    if (sf_freak_build_pattern(&c->freak, pattern.data(), (int32_t*)(tables + FREAK_TABLE_SIZES)) != SF_OK)
      return sf_fail(c, SF_EINVAL, "FREAK parameters out of range");
    sf_freak_orientation_table(pattern.data(), (int32_t*)(tables + FREAK_TABLE_ORIENT));
    SF_HIP(c, hipMemcpyAsync(c->freak_pattern.p, pattern.data(), FREAK_PATTERN_FLOATS * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  sf_freak_bit_table(freak_pairs(c), tables + FREAK_TABLE_PAIRS);
  SF_HIP(c, hipMemcpyAsync(c->freak_tables.p, tables, FREAK_TABLE_BYTES, hipMemcpyHostToDevice, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));   // (the host pattern goes away with this call)
  SfFreakTables& T = c->freak_dev;
  T.pattern = (const float*)c->freak_pattern.p;
  T.pairs = (const uint8_t*)c->freak_tables.p + FREAK_TABLE_PAIRS;
  T.orient = (const int32_t*)((const uint8_t*)c->freak_tables.p + FREAK_TABLE_ORIENT);
  T.sizes = (const int32_t*)((const uint8_t*)c->freak_tables.p + FREAK_TABLE_SIZES);
  T.size_cst = (float)(FREAK_SCALES / (0.693147180559945 * c->freak.n_octaves));
  T.fixed_idx = std::min(std::max((int)(1.0986122886681 * T.size_cst + 0.5), 0), FREAK_SCALES - 1);   // (upstream does not clamp: n_octaves 1)
  T.orientation_normalized = c->freak.orientation_normalized;
  T.scale_normalized = c->freak.scale_normalized;
  c->freak_pattern_ok = c->freak_tables_ok = true;
  return SF_OK;
}

// ---- SURF (Vis/FeatureType 0; kernels and table builder in k_surf.hip) -------------------------------------------------
static int surf_validate(sf_context* c, const sf_surf_params& p) {
  if (!(p.hessian_threshold >= 0.0f) || !std::isfinite(p.hessian_threshold))
    return sf_fail(c, SF_EINVAL, "SURF hessian_threshold %g: finite and >= 0", (double)p.hessian_threshold);
  if (p.n_octaves < 1 || p.n_octaves > SURF_MAX_OCTAVES) return sf_fail(c, SF_EINVAL, "SURF n_octaves %d outside 1 .. %d", p.n_octaves, SURF_MAX_OCTAVES);
  if (p.n_octave_layers < 1 || p.n_octave_layers > SURF_MAX_LAYERS)
    return sf_fail(c, SF_EINVAL, "SURF n_octave_layers %d outside 1 .. %d", p.n_octave_layers, SURF_MAX_LAYERS);
  if ((p.upright != 0 && p.upright != 1) || (p.extended != 0 && p.extended != 1))
    return sf_fail(c, SF_EINVAL, "SURF upright %d, extended %d: each is 0 or 1", p.upright, p.extended);
  return SF_OK;
}

// the same ranges without a handle (sf_experimental.h; NULL = the defaults)
extern "C" int sf_surf_check_params(const sf_surf_params* params) {
  return surf_validate(nullptr, arg_or_defaults(params, sf_surf_defaults));
}

extern "C" int sf_set_feature_type_surf(sf_handle c, const sf_surf_params* surf) {
  if (!c) return SF_EINVAL;
  if (c->params.desc_type != 1)
    return sf_fail(c, SF_EINVAL, "SURF writes float32 descriptors: a handle with desc_type %d cannot store them (create it with desc_type 1 and desc_bytes 256, or 512 for extended rows)",
                   c->params.desc_type);
  const sf_surf_params p = arg_or_defaults(surf, sf_surf_defaults);
  int rc = surf_validate(c, p);
  if (rc != SF_OK) return rc;
  const int bytes = p.extended ? 512 : 256;
  if (c->params.desc_bytes != bytes)
    return sf_fail(c, SF_EINVAL, "SURF rows with extended %d are %d bytes: the handle was created with desc_bytes %d", p.extended, bytes,
                   c->params.desc_bytes);
  c->surf = p;
  c->feature_type = 0;
  return SF_OK;
}

extern "C" int sf_get_surf_params(sf_handle c, sf_surf_params* out) {
  if (!c || !out) return SF_EINVAL;
  *out = c->surf;
  return SF_OK;
}

extern "C" int sf_detect_surf_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                     int32_t max_features, const sf_surf_params* surf, sf_keypoint* d_kpts_out, int32_t cap,
                                     int32_t* n_out) {
  if (!c || !n_out || cap < 0 || (cap > 0 && !d_kpts_out)) return SF_EINVAL;
  *n_out = 0;
  int rc;
  if ((rc = check_image(c, d_image, width, height, pitch, 3, "image")) != SF_OK) return rc;
  const sf_surf_params prm = surf ? *surf : c->surf;
  if ((rc = surf_validate(c, prm)) != SF_OK) return rc;
  if ((rc = check_pixels(c, width, height)) != SF_OK) return rc;
  if ((long long)(width + 1) * (height + 1) * 255 > 0x7FFFFFFFll) return sf_fail(c, SF_ERANGE, "image too large for a 32-bit integral image");
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_detect_surf(c, d_image, width, height, pitch, max_features, &prm, d_kpts_out, cap, n_out);
}

// ---- the SIFT detector (kernels, tables and plan in k_sift.hip) ------------------------------------------------------------
extern "C" int sf_sift_check_params(const sf_sift_params* params) {
  return sf_sift_validate(nullptr, arg_or_defaults(params, sf_sift_defaults));
}

extern "C" int sf_set_feature_type_sift(sf_handle c, const sf_sift_params* sift) {
  if (!c) return SF_EINVAL;
  if (c->params.desc_type != 1 || c->params.desc_bytes != 512)
    return sf_fail(c, SF_EINVAL, "SIFT writes 128 float32 per row: a handle with desc_type %d and desc_bytes %d cannot store them (create it with desc_type 1 and desc_bytes 512)",
                   c->params.desc_type, c->params.desc_bytes);
  const sf_sift_params p = arg_or_defaults(sift, sf_sift_defaults);
  const int rc = sf_sift_validate(c, p);
  if (rc != SF_OK) return rc;
  c->sift = p;
  c->feature_type = 1;
  return SF_OK;
}

extern "C" int sf_get_sift_params(sf_handle c, sf_sift_params* out) {
  if (!c || !out) return SF_EINVAL;
  *out = c->sift;
  return SF_OK;
}

extern "C" int sf_detect_sift_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                     int32_t max_features, const sf_sift_params* sift, sf_keypoint* d_kpts_out, int32_t cap,
                                     int32_t* n_out) {
  if (!c || !n_out || cap < 0 || (cap > 0 && !d_kpts_out)) return SF_EINVAL;
  *n_out = 0;
  int rc;
  if ((rc = check_image(c, d_image, width, height, pitch, 3, "image")) != SF_OK) return rc;
  const sf_sift_params prm = sift ? *sift : c->sift;
  if ((rc = sf_sift_validate(c, prm)) != SF_OK) return rc;
  if ((rc = check_pixels(c, width, height)) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_detect_sift(c, d_image, width, height, pitch, max_features, &prm, d_kpts_out, cap, n_out);
}

extern "C" int sf_debug_sift_limits(sf_handle c, int32_t candidate_cap) {
  if (!c) return SF_EINVAL;
  if (candidate_cap < 0 || (unsigned)candidate_cap > SIFT_MAX_CANDIDATES)
    return sf_fail(c, SF_EINVAL, "sf_debug_sift_limits: candidate_cap %d outside 0 .. %u", candidate_cap, SIFT_MAX_CANDIDATES);
  c->sift_debug_cap = candidate_cap;
  return SF_OK;
}

extern "C" int sf_debug_sift_batch_chunk(sf_handle c, int32_t batch_chunk) {
  if (!c) return SF_EINVAL;
  if (batch_chunk < 0 || batch_chunk > 65535)
    return sf_fail(c, SF_EINVAL, "sf_debug_sift_batch_chunk: batch_chunk %d outside 0 .. 65535", batch_chunk);
  c->sift_debug_chunk = batch_chunk;
  return SF_OK;
}

extern "C" int sf_sift_batch_plan(int32_t width, int32_t height, const sf_sift_params* params, int32_t n_keyframes,
                                  int32_t* cap_img_out, int32_t* chunk_out, int64_t* workspace_bytes_out) {
  const sf_sift_params p = arg_or_defaults(params, sf_sift_defaults);
  if (n_keyframes < 1 || n_keyframes > 65535) return SF_EINVAL;
  int rc = sf_sift_validate(nullptr, p);
  if (rc != SF_OK) return rc;
  SfSiftBatchPlan sp;
  if ((rc = sf_sift_batch_plan_host(nullptr, width, height, p, n_keyframes, 0, 0, &sp)) != SF_OK) return rc;
  if (cap_img_out) *cap_img_out = (int32_t)sp.cap_img;
  if (chunk_out) *chunk_out = sp.chunk;
  if (workspace_bytes_out) *workspace_bytes_out = (int64_t)sp.workspace_bytes;
  return SF_OK;
}

extern "C" int sf_debug_sift_plane(sf_handle c, int32_t octave, int32_t layer, int32_t dog, int16_t* d_out) {
  if (!c) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_sift_copy_plane(c, octave, layer, dog, d_out);
}

// The two Gaussian tables on the device, uploaded once: they depend on no parameter
static int surf_ensure(sf_context* c) {
  c->surf_dev.upright = c->surf.upright;
  c->surf_dev.extended = c->surf.extended;
  if (c->surf_tables_ok) return SF_OK;
  int rc;
  if ((rc = sf_buf_reserve(c, c->surf_tables, SURF_TABLE_BYTES)) != SF_OK) return rc;
  alignas(16) uint8_t host[SURF_TABLE_BYTES] = {};
  sf_surf_build_tables((float*)(host + SURF_TABLE_ORI_W), (int8_t*)(host + SURF_TABLE_ORI_XY), (float*)(host + SURF_TABLE_DESC_W));
  SF_HIP(c, hipMemcpyAsync(c->surf_tables.p, host, SURF_TABLE_BYTES, hipMemcpyHostToDevice, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));   // (the host copy goes away with this call)
  const uint8_t* d = (const uint8_t*)c->surf_tables.p;
  c->surf_dev.ori_w = (const float*)(d + SURF_TABLE_ORI_W);
  c->surf_dev.ori_xy = (const int8_t*)(d + SURF_TABLE_ORI_XY);
  c->surf_dev.desc_w = (const float*)(d + SURF_TABLE_DESC_W);
  c->surf_tables_ok = true;
  return SF_OK;
}

// The descriptor of the handle's feature type (ExtractKind: sf_internal.hpp)
static int extract_kind(sf_context* c, ExtractKind* k) {
  int rc;
  if (c->feature_type == 1) {                              // (selected on a handle with desc_type 1 and 512-byte rows only)
    c->sift_kind = {c->sift, c->sift_reuse_pyramid};
    *k = {512, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &c->sift_kind};
    return SF_OK;
  }
  if (c->feature_type == 0) {                              // (selected on a handle with desc_type 1 and these row bytes only)
    if ((rc = surf_ensure(c)) != SF_OK) return rc;
    *k = {c->surf.extended ? 512 : 256, nullptr, nullptr, nullptr, 0, nullptr, &c->surf_dev};
    return SF_OK;
  }
  if (c->feature_type == 3 || c->feature_type == 5) {
    if ((rc = check_binary_rows(c, c->feature_type)) != SF_OK) return rc;
    if ((rc = freak_ensure(c)) != SF_OK) return rc;
    *k = {FREAK_BYTES, nullptr, nullptr, nullptr, 0, &c->freak_dev};
    return SF_OK;
  }
  if (c->feature_type == 8 || c->feature_type == 2) {
    if ((rc = check_binary_rows(c, c->feature_type)) != SF_OK) return rc;
    if ((rc = orb_ensure(c)) != SF_OK) return rc;
    *k = {32, (const int8_t*)c->orb_tests.p, &c->orb, c->feature_type == 2 ? &c->orb_det : nullptr, 0};
    return SF_OK;
  }
  if ((rc = brief_ensure(c)) != SF_OK) return rc;
  *k = {c->brief_bytes, (const int8_t*)c->brief_tests.p, nullptr, nullptr, 0};
  return SF_OK;
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

extern "C" int sf_detect_corners_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                        int32_t max_corners, double quality_level, double min_distance,
                                        sf_keypoint* d_kpts_out, int32_t cap, int32_t* n_out) {
  if (!c || !n_out || cap < 0 || (cap > 0 && !d_kpts_out)) return SF_EINVAL;
  *n_out = 0;
  int rc;
  if ((rc = check_image(c, d_image, width, height, pitch, 3, "image")) != SF_OK) return rc;
  if ((rc = check_gftt(c, quality_level, min_distance)) != SF_OK) return rc;
  if ((rc = check_pixels(c, width, height)) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_detect_corners(c, d_image, width, height, pitch, max_corners, quality_level, min_distance, d_kpts_out,
                                  cap, n_out);
}

// ---- FAST (Vis/FeatureType 4; kernels in k_fast.hip) ---------------------------------------------------------------
extern "C" void sf_fast_defaults(sf_fast_params* p) {
  if (!p) return;
  p->threshold = 20;           // FAST/Threshold [upstream rtabmap Parameters.h]
  p->nonmax_suppression = 1;   // FAST/NonmaxSuppression
}

static int fast_validate(sf_context* c, const sf_fast_params& f) {
  if (f.threshold < 1 || f.threshold > 254) return sf_fail(c, SF_EINVAL, "FAST threshold %d outside 1 .. 254", f.threshold);
  if (f.nonmax_suppression != 0 && f.nonmax_suppression != 1)
    return sf_fail(c, SF_EINVAL, "FAST nonmax_suppression %d is neither 0 nor 1", f.nonmax_suppression);
  return SF_OK;
}

extern "C" int sf_fast_set_params(sf_handle c, const sf_fast_params* params) {
  if (!c || !params) return SF_EINVAL;
  int rc = fast_validate(c, *params);
  if (rc != SF_OK) return rc;
  c->fast = *params;
  return SF_OK;
}

extern "C" int sf_fast_get_params(sf_handle c, sf_fast_params* params) {
  if (!c || !params) return SF_EINVAL;
  *params = c->fast;
  return SF_OK;
}

extern "C" int sf_detect_fast_device(sf_handle c, const uint8_t* d_image, int32_t width, int32_t height, int32_t pitch,
                                     int32_t max_features, const sf_fast_params* params, sf_keypoint* d_kpts_out,
                                     int32_t cap, int32_t* n_out) {
  if (!c || !n_out || cap < 0 || (cap > 0 && !d_kpts_out)) return SF_EINVAL;
  *n_out = 0;
  int rc;
  if ((rc = check_image(c, d_image, width, height, pitch, 3, "image")) != SF_OK) return rc;
  const sf_fast_params prm = params ? *params : c->fast;
  if ((rc = fast_validate(c, prm)) != SF_OK) return rc;
  if ((rc = check_pixels(c, width, height)) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_detect_fast(c, d_image, width, height, pitch, max_features, &prm, d_kpts_out, cap, n_out);
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

extern "C" int sf_front_get_params(sf_handle c, sf_front_params* params) {
  if (!c || !params) return SF_EINVAL;
  *params = c->front;
  return SF_OK;
}

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
  int rc = check_image(c, d_image, width, height, pitch, 1, "image");
  if (rc != SF_OK) return rc;
  if ((rc = check_subpix(c, width, height, win, iterations)) != SF_OK) return rc;
  if (!(eps == eps)) return sf_fail(c, SF_EINVAL, "cornerSubPix eps is NaN");
  if (n > 0 && !d_kpts) return sf_fail(c, SF_EINVAL, "keypoints missing");
  if (n == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_corner_subpix(c, d_image, 0, 1, width, height, pitch, d_kpts, n, nullptr, n, 0, 0, win, iterations, eps);
}

// What the extraction calls do around their detector: the ROI of the handle's ratios on a width x height image and
// whether the corners are refined.  Refuses, before anything is touched, what the two steps cannot do.
struct FrontPlan {
  int x = 0, y = 0, w = 0, h = 0;
  bool refine = false;
  // Vis/GridRows x Vis/GridCols (grid_plan): the cells, what each may keep, the rows a keyframe can hold (1 x 1: the ROI,
  // max_features, max_features).  Under a grid k_grid_gather shifts the keypoints, not k_corner_subpix
  int rows = 1, cols = 1, col_size = 0, row_size = 0, quota = 0, rows_cap = 0;
  bool grid() const { return rows * cols > 1; }
  bool launch() const { return refine || (!grid() && (x || y)); }   // (an offset of zero and no refinement: no launch at all)
  int off_x() const { return grid() ? 0 : x; }
  int off_y() const { return grid() ? 0 : y; }
};

static int front_plan(sf_context* c, int width, int height, FrontPlan* fp) {
  const sf_front_params& f = c->front;
  int32_t roi[4] = {0, 0, 0, 0};
  const int rc = sf_compute_roi(width, height, f.roi_ratios, roi);
  if (c->feature_type == 2 && (f.roi_ratios[0] != 0.f || f.roi_ratios[1] != 0.f || f.roi_ratios[2] != 0.f || f.roi_ratios[3] != 0.f))
    return sf_fail(c, SF_EINVAL, "Vis/RoiRatios under Vis/FeatureType 2 (ORB) is not built: the batch form reuses the detector's pyramid for the descriptors; set the ratios to 0 or choose feature type 3, 4, 5, 6 or 8");
  if (c->feature_type == 0 && (f.roi_ratios[0] != 0.f || f.roi_ratios[1] != 0.f || f.roi_ratios[2] != 0.f || f.roi_ratios[3] != 0.f))
    return sf_fail(c, SF_EINVAL, "Vis/RoiRatios under Vis/FeatureType 0 (SURF) is not built; set the ratios to 0");
  if (c->feature_type == 1 && (f.roi_ratios[0] != 0.f || f.roi_ratios[1] != 0.f || f.roi_ratios[2] != 0.f || f.roi_ratios[3] != 0.f))
    return sf_fail(c, SF_EINVAL, "Vis/RoiRatios under Vis/FeatureType 1 (SIFT) is not built; set the ratios to 0");
  if (rc != SF_OK)
    return sf_fail(c, SF_EINVAL, "Vis/RoiRatios %g %g %g %g leave a ROI of %d x %d in a %d x %d image: both sides must be >= 3",
                   (double)f.roi_ratios[0], (double)f.roi_ratios[1], (double)f.roi_ratios[2], (double)f.roi_ratios[3], roi[2], roi[3], width, height);
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

extern "C" int sf_grid_get_params(sf_handle c, sf_grid_params* params) {
  if (!c || !params) return SF_EINVAL;
  *params = c->grid;
  return SF_OK;
}

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

// The cells of an extraction call, behind front_plan and the check of max_features: nothing to do on a 1 x 1 grid (one
// "cell", the ROI, with the whole of max_features), else what sf_compute_grid says -- refused before anything is touched
static int grid_plan(sf_context* c, int width, int height, int max_features, FrontPlan* fp) {
  fp->rows = fp->cols = 1;
  fp->col_size = fp->w; fp->row_size = fp->h;
  fp->quota = fp->rows_cap = max_features;
  const sf_grid_params& g = c->grid;
  if (g.grid_rows == 1 && g.grid_cols == 1) return SF_OK;
  if (c->feature_type == 2)
    return sf_fail(c, SF_EINVAL, "Vis/GridRows x Vis/GridCols %d x %d under Vis/FeatureType 2 (ORB) is not built: every cell would need a pyramid of its own; set the grid to 1 x 1 or choose feature type 3, 4, 5, 6 or 8",
                   g.grid_rows, g.grid_cols);
  if (c->feature_type == 0)
    return sf_fail(c, SF_EINVAL, "Vis/GridRows x Vis/GridCols %d x %d under Vis/FeatureType 0 (SURF) is not built; set the grid to 1 x 1",
                   g.grid_rows, g.grid_cols);
  if (c->feature_type == 1)
    return sf_fail(c, SF_EINVAL, "Vis/GridRows x Vis/GridCols %d x %d under Vis/FeatureType 1 (SIFT) is not built; set the grid to 1 x 1",
                   g.grid_rows, g.grid_cols);
  int32_t o[6];
  const int rc = sf_compute_grid(width, height, c->front.roi_ratios, &g, max_features, o);
  if (rc == SF_ERANGE)
    return sf_fail(c, SF_ERANGE, "a grid of %d x %d cells with %d keypoints apiece holds %d rows > %d (KeyPointVec.size is an int16)",
                   g.grid_rows, g.grid_cols, o[4], o[5], SF_MAX_FEATURES);
  if (rc != SF_OK)
    return sf_fail(c, SF_EINVAL, "a grid of %d x %d on a ROI of %d x %d leaves cells of %d x %d: both sides must be >= 3", g.grid_rows,
                   g.grid_cols, fp->w, fp->h, o[2], o[3]);
  fp->rows = g.grid_rows; fp->cols = g.grid_cols;
  fp->col_size = o[2]; fp->row_size = o[3]; fp->quota = o[4]; fp->rows_cap = o[5];
  return SF_OK;
}

// The detection stage under a grid, for n images (the single calls: n = 1): the batch launchers with the cells as their
// images, then k_grid_gather -- d_kpts [n][rows_cap] in full-image coordinates, d_n [n], nothing waited for
static int grid_detect(sf_context* c, const FrontPlan& fp, const sf_detector_params& dp, const uint8_t* d_left, size_t image_stride,
                       int n, int pitch, sf_keypoint* d_kpts, int32_t* d_n) {
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
  if (fast_corners(c->feature_type))
    rc = sf_launch_detect_fast_batch(c, d_roi, image_stride, n * cells, fp.col_size, fp.row_size, pitch, fp.quota, &c->fast,
                                     d_cell_kpts, fp.quota, d_cell_n, g);
  else
    rc = sf_launch_detect_corners_batch(c, d_roi, image_stride, n * cells, fp.col_size, fp.row_size, pitch, fp.quota,
                                        dp.quality_level, dp.min_distance, d_cell_kpts, fp.quota, d_cell_n, g);
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
  int rc = check_image(c, d_left && d_right, width, height, pitch, 1, "stereo pair");
  if (rc != SF_OK) return rc;
  if (n > 0 && (!d_kpts || !d_right_xy || !d_status)) return sf_fail(c, SF_EINVAL, "corners or output arrays missing");
  const sf_stereo_flow_params prm = arg_or_defaults(params, sf_stereo_flow_defaults);
  if (prm.win_width <= 2 || prm.win_height <= 2)
    return sf_fail(c, SF_EINVAL, "window of %d x %d: both sides must be > 2 (cv::calcOpticalFlowPyrLK asserts the same)", prm.win_width, prm.win_height);
  if ((long long)prm.win_width * prm.win_height > 1024) return sf_fail(c, SF_ERANGE, "window of %d x %d exceeds 1024 pixels", prm.win_width, prm.win_height);
  if (prm.max_level < 0 || prm.max_level > 15) return sf_fail(c, SF_ERANGE, "max_level %d outside 0 .. 15", prm.max_level);
  if (!(prm.epsilon == prm.epsilon)) return sf_fail(c, SF_EINVAL, "epsilon is NaN");
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

extern "C" int sf_stereo_get_params(sf_handle c, sf_stereo_params* params) {
  if (!c || !params) return SF_EINVAL;
  *params = c->stereo;
  return SF_OK;
}

// what block matching refuses of the flow parameters (epsilon and min_eig_threshold are not read)
static int check_block_match(sf_context* c, const sf_stereo_flow_params& prm) {
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
  int rc = check_image(c, d_left && d_right, width, height, pitch, 1, "stereo pair");
  if (rc != SF_OK) return rc;
  if (n > 0 && (!d_kpts || !d_right_xy || !d_status)) return sf_fail(c, SF_EINVAL, "corners or output arrays missing");
  if (ssd != 0 && ssd != 1) return sf_fail(c, SF_EINVAL, "ssd %d: 1 = squared, 0 = absolute differences", ssd);
  const sf_stereo_flow_params prm = arg_or_defaults(params, sf_stereo_flow_defaults);
  if ((rc = check_block_match(c, prm)) != SF_OK) return rc;
  if (n == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_stereo_bm_batch(c, d_left, d_right, 0, 1, width, height, pitch, d_kpts, n, nullptr, &prm, ssd, d_right_xy,
                                   d_status, d_right_x, d_score);
}

extern "C" int sf_extract_keyframe_device(sf_handle c, const uint8_t* d_left, int32_t width, int32_t height,
                                          int32_t pitch, const sf_keypoint* d_kpts, const float* d_right_x,
                                          const uint8_t* d_status, int32_t n, const sf_stereo_camera* cam,
                                          int32_t* out_slot, int32_t* out_rows, uint8_t* d_desc_out,
                                          float* d_xyz_out, sf_keypoint* d_kpts_out) {
  if (!c || !cam || n < 0) return SF_EINVAL;
  int rc = check_image(c, d_left, width, height, pitch, 1, "left image");
  if (rc != SF_OK) return rc;
  if (n > 0 && !d_kpts) return sf_fail(c, SF_EINVAL, "keypoints missing");
  if (n > SF_MAX_FEATURES) return sf_fail(c, SF_ERANGE, "%d corners > int16 limit of KeyPointVec.size", n);
  if ((long long)(width + 1) * (height + 1) * 255 > 0x7FFFFFFFll) return sf_fail(c, SF_ERANGE, "image too large for a 32-bit integral image");
  SF_HIP(c, hipSetDevice(c->device));
  ExtractKind kind;
  if ((rc = extract_kind(c, &kind)) != SF_OK) return rc;
  if ((rc = sf_store_reserve(c, c->store, c->store.slots + 1, n, kind.bytes)) != SF_OK) return rc;
  if (out_rows && (rc = sf_buf_reserve(c, c->ex_rows, 16)) != SF_OK) return rc;
  const int slot = c->store.slots;
  if ((rc = sf_launch_extract_batch(c, d_left, 0, 1, width, height, pitch, d_kpts, d_right_x, d_status, n, nullptr, cam, kind,
                                    slot, d_desc_out, d_xyz_out, d_kpts_out,
                                    out_rows ? (int32_t*)c->ex_rows.p : nullptr)) != SF_OK)
    return rc;
  c->store.slots += 1;
  if (out_slot) *out_slot = slot;
  return out_rows ? sf_word_to_host(c, c->ex_rows.p, out_rows) : SF_OK;
}

extern "C" void sf_detector_defaults(sf_detector_params* p) {
  if (!p) return;
  p->max_features = 1000;      // Vis/MaxFeatures [upstream rtabmap Parameters.h]; the reference sets only Vis/MinInliers
  p->quality_level = 0.001;    // GFTT/QualityLevel
  p->min_distance = 3.0;       // GFTT/MinDistance
}

// The GetFeatsAndDesc handler in one call on HOST buffers: upload the pair, detect, track, extract, download the
// response.  Everything between the two copies stays on the device; the keyframe is in the store when it returns.
// format < 0: rectified MONO8 planes (sf_get_features_and_descriptor); otherwise the camera's images in that
// sf_image_format (sf_get_features_and_descriptor_u8), converted on the device behind the upload.
static int get_features_host(sf_context* c, const uint8_t* left, const uint8_t* right, int format, int32_t width,
                             int32_t height, int32_t pitch, const sf_stereo_camera* cam, const sf_detector_params* det,
                             const sf_stereo_flow_params* flow, uint8_t* desc_out, float* xyz_out, sf_keypoint* kpts_out,
                             int32_t cap_rows, int32_t* rows_out, int32_t* slot_out) {
  if (!c || !cam || !rows_out || cap_rows < 0) return SF_EINVAL;
  *rows_out = 0;
  int rc = format < 0 ? check_image(c, left && right, width, height, pitch, 3, "stereo pair")
                      : check_camera_image(c, left && right, format, width, height, pitch, 3, "stereo pair");
  if (rc != SF_OK) return rc;
  FrontPlan fp;
  if ((rc = front_plan(c, width, height, &fp)) != SF_OK) return rc;
  const sf_detector_params dp = arg_or_defaults(det, sf_detector_defaults);
  if (dp.max_features <= 0 || dp.max_features > SF_MAX_FEATURES)
    return sf_fail(c, SF_ERANGE, "max_features %d outside 1 .. %d (KeyPointVec.size is an int16)", dp.max_features, SF_MAX_FEATURES);
  if ((rc = grid_plan(c, width, height, dp.max_features, &fp)) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  ExtractKind kind;
  if ((rc = extract_kind(c, &kind)) != SF_OK) return rc;
  const size_t img_bytes = ((size_t)width * height + 255) & ~(size_t)255;
  const int maxf = fp.rows_cap;                            // the rows of the call's buffers: max_features, or the grid's R C quota
  if ((rc = sf_buf_reserve(c, c->ft_images, 2 * img_bytes)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->ft_kpts, (size_t)maxf * sizeof(sf_keypoint))) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->ft_flow, (size_t)maxf * 16)) != SF_OK) return rc;
  const size_t row_bytes = (size_t)kind.bytes + 12 + sizeof(sf_keypoint);
  if ((rc = sf_buf_reserve(c, c->ft_wire, (size_t)maxf * row_bytes + 64)) != SF_OK) return rc;
  uint8_t* d_left = (uint8_t*)c->ft_images.p;
  uint8_t* d_right = d_left + img_bytes;
  if (format == SF_IMAGE_RGB8 || format == SF_IMAGE_BGR8) {
    // the colour pair as it is (rows padded to 16 bytes: the conversion's wide path), then both planes in one launch
    const int src_pitch = (3 * width + 15) & ~15;
    const size_t src_bytes = ((size_t)src_pitch * height + 255) & ~(size_t)255;
    if ((rc = sf_buf_reserve(c, c->img_src, 2 * src_bytes)) != SF_OK) return rc;
    uint8_t* d_src = (uint8_t*)c->img_src.p;
    SF_HIP(c, hipMemcpy2DAsync(d_src, src_pitch, left, pitch, 3 * (size_t)width, height, hipMemcpyHostToDevice, c->stream));
    SF_HIP(c, hipMemcpy2DAsync(d_src + src_bytes, src_pitch, right, pitch, 3 * (size_t)width, height, hipMemcpyHostToDevice, c->stream));
    if ((rc = sf_launch_image_gray(c, d_src, nullptr, 2, format, c->gray_rule, width, height, src_pitch, src_bytes, 2, d_left,
                                   width, img_bytes)) != SF_OK)
      return rc;
  } else {                                                 // MONO8 planes, or mono8 camera images: the pitched copy is the upload
    SF_HIP(c, hipMemcpy2DAsync(d_left, width, left, pitch, width, height, hipMemcpyHostToDevice, c->stream));
    SF_HIP(c, hipMemcpy2DAsync(d_right, width, right, pitch, width, height, hipMemcpyHostToDevice, c->stream));
  }
  sf_keypoint* d_kpts = (sf_keypoint*)c->ft_kpts.p;
  int32_t n = 0;
  // (the GFTT parameters are checked under every feature type, FAST and ORB included, which do not use them)
  if ((rc = check_gftt(c, dp.quality_level, dp.min_distance)) != SF_OK) return rc;
  const uint8_t* d_roi = d_left + (size_t)fp.y * width + fp.x;   // the detector's image: the ROI, at the parent's pitch
  if (fp.grid()) {                                       // every cell in one launch sequence, one wait for the keyframe's count
    if ((rc = check_pixels(c, fp.col_size, fp.row_size)) != SF_OK) return rc;
    if ((rc = sf_buf_reserve(c, c->ft_counts, 4)) != SF_OK) return rc;
    if ((rc = grid_detect(c, fp, dp, d_left, 0, 1, width, d_kpts, (int32_t*)c->ft_counts.p)) != SF_OK) return rc;
    rc = sf_word_to_host(c, c->ft_counts.p, &n);
  } else switch (c->feature_type) {
    case 3:
    case 4: rc = sf_detect_fast_device(c, d_roi, fp.w, fp.h, width, maxf, nullptr, d_kpts, maxf, &n); break;
    case 2: rc = sf_detect_orb_device(c, d_roi, fp.w, fp.h, width, maxf, nullptr, nullptr, d_kpts, maxf, &n); break;
    case 0: rc = sf_detect_surf_device(c, d_roi, fp.w, fp.h, width, maxf, nullptr, d_kpts, maxf, &n); break;   // (no ROI: front_plan)
    case 1: rc = sf_detect_sift_device(c, d_roi, fp.w, fp.h, width, maxf, nullptr, d_kpts, maxf, &n); break;   // (likewise)
    default:
      rc = sf_detect_corners_device(c, d_roi, fp.w, fp.h, width, maxf, dp.quality_level, dp.min_distance, d_kpts, maxf, &n);
  }
  if (rc != SF_OK) return rc;
  n = std::min(n, maxf);
  if (fp.launch() &&
      (rc = sf_launch_corner_subpix(c, d_left, 0, 1, width, height, width, d_kpts, n, nullptr, maxf, fp.off_x(), fp.off_y(),
                                    fp.refine ? c->front.subpix_win_size : 0, c->front.subpix_iterations, c->front.subpix_eps)) != SF_OK)
    return rc;
  float* d_xy = (float*)c->ft_flow.p;                    // [n][2], then x [n], then status [n]
  float* d_rx = d_xy + 2 * (size_t)maxf;
  uint8_t* d_status = (uint8_t*)(d_rx + maxf);
  rc = c->stereo.optical_flow
           ? sf_stereo_correspondences_device(c, d_left, d_right, width, height, width, d_kpts, n, flow, d_xy, d_status, d_rx, nullptr)
           : sf_stereo_block_match_device(c, d_left, d_right, width, height, width, d_kpts, n, flow, c->stereo.ssd, d_xy, d_status, d_rx, nullptr);
  if (rc != SF_OK) return rc;
  uint8_t* d_desc = (uint8_t*)c->ft_wire.p;
  float* d_xyz = (float*)(d_desc + (((size_t)maxf * kind.bytes + 15) & ~(size_t)15));
  sf_keypoint* d_kp_out = (sf_keypoint*)(d_xyz + 3 * (size_t)maxf);
  int32_t slot = -1, rows = 0;
  c->sift_reuse_pyramid = c->feature_type == 1;          // the detector's pyramid of this image: the refinement moved x and y only
  rc = sf_extract_keyframe_device(c, d_left, width, height, width, d_kpts, d_rx, d_status, n, cam, &slot, &rows, d_desc, d_xyz,
                                  d_kp_out);
  c->sift_reuse_pyramid = false;
  if (rc != SF_OK) return rc;
  *rows_out = rows;
  if (slot_out) *slot_out = slot;
  const int32_t k = std::min(rows, cap_rows);
  if (k > 0) {
    if (desc_out) SF_HIP(c, hipMemcpyAsync(desc_out, d_desc, (size_t)k * kind.bytes, hipMemcpyDeviceToHost, c->stream));
    if (xyz_out) SF_HIP(c, hipMemcpyAsync(xyz_out, d_xyz, (size_t)k * 12, hipMemcpyDeviceToHost, c->stream));
    if (kpts_out) SF_HIP(c, hipMemcpyAsync(kpts_out, d_kp_out, (size_t)k * sizeof(sf_keypoint), hipMemcpyDeviceToHost, c->stream));
    SF_HIP(c, hipStreamSynchronize(c->stream));
  }
  return SF_OK;
}

extern "C" int sf_get_features_and_descriptor(sf_handle c, const uint8_t* left, const uint8_t* right, int32_t width,
                                              int32_t height, int32_t pitch, const sf_stereo_camera* cam,
                                              const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                              uint8_t* desc_out, float* xyz_out, sf_keypoint* kpts_out, int32_t cap_rows,
                                              int32_t* rows_out, int32_t* slot_out) {
  return get_features_host(c, left, right, -1, width, height, pitch, cam, det, flow, desc_out, xyz_out, kpts_out, cap_rows,
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
  return get_features_host(c, left, right, format, width, height, pitch, cam, det, flow, desc_out, xyz_out, kpts_out, cap_rows,
                           rows_out, slot_out);
}

// n keyframes from device images to n store slots in ONE launch sequence: detector, stereo correspondence and
// extraction each run once over the batch (blockIdx = image), the corner counts stay in device memory between them, the
// host never waits.  Same per-keyframe results as sf_get_features_and_descriptor.
// The batch form in three parts, shared by sf_get_features_and_descriptor_batch_device, sf_add_keyframes_u8_batch_device
// and their Vis/FeatureType 2, 0 and 1 twins (the _orb_, _surf_ and _sift_ calls; `family`): batch_check refuses (nothing is
// touched; n_keyframes = 0 passes without a look at the images), batch_reserve takes the store slots and the call's buffers,
// batch_launch queues the three stages (under type 1 chunk by chunk: batch_launch_sift).  Types 2, 0 and 1 are reached
// through their own calls only, as they are selected through their own.
enum BatchFamily { BATCH_GENERIC, BATCH_ORB, BATCH_SURF, BATCH_SIFT };

// the batch calls of a feature type, for the message of a call that is not one of them
static const char* batch_calls_of(int feature_type) {
  switch (feature_type) {
    case 2: return "sf_get_features_and_descriptor_orb_batch_device / sf_add_keyframes_orb_u8_batch_device";
    case 0: return "sf_get_features_and_descriptor_surf_batch_device / sf_add_keyframes_surf_u8_batch_device";
    case 1: return "sf_get_features_and_descriptor_sift_batch_device / sf_add_keyframes_sift_u8_batch_device";
    default: return "sf_get_features_and_descriptor_batch_device / sf_add_keyframes_u8_batch_device";
  }
}

struct BatchPlan {
  sf_detector_params dp;
  sf_stereo_flow_params prm;
  ExtractKind kind;
  FrontPlan front;
};

static int batch_check(sf_context* c, BatchFamily family, bool images, int n_keyframes, int width, int height, int pitch,
                       size_t image_stride, const sf_detector_params* det, const sf_stereo_flow_params* flow, BatchPlan* plan) {
  const bool orb_call = family == BATCH_ORB, surf_call = family == BATCH_SURF, sift_call = family == BATCH_SIFT;
  if (c->feature_type == 2 && !orb_call)
    return sf_fail(c, SF_EINVAL, "Vis/FeatureType 2 (ORB on a pyramid) has batch forms of its own: sf_get_features_and_descriptor_orb_batch_device, sf_add_keyframes_orb_u8_batch_device");
  if (c->feature_type == 1 && !sift_call)
    return sf_fail(c, SF_EINVAL, "Vis/FeatureType 1 (SIFT): the batch form of type 1 is not built into this call: use %s", batch_calls_of(1));
  if (c->feature_type == 0 && !surf_call)
    return sf_fail(c, SF_EINVAL, "Vis/FeatureType 0 (SURF) has batch forms of its own: sf_get_features_and_descriptor_surf_batch_device, sf_add_keyframes_surf_u8_batch_device");
  if (c->feature_type != 2 && orb_call)
    return sf_fail(c, SF_EINVAL, "Vis/FeatureType %d: the ORB batch calls need type 2 (sf_set_feature_type_orb); use %s",
                   c->feature_type, batch_calls_of(c->feature_type));
  if (c->feature_type != 0 && surf_call)
    return sf_fail(c, SF_EINVAL, "Vis/FeatureType %d: the SURF batch calls need type 0 (sf_set_feature_type_surf); use %s",
                   c->feature_type, batch_calls_of(c->feature_type));
  if (c->feature_type != 1 && sift_call)
    return sf_fail(c, SF_EINVAL, "Vis/FeatureType %d: the SIFT batch calls need type 1 (sf_set_feature_type_sift); use %s",
                   c->feature_type, batch_calls_of(c->feature_type));
  if (n_keyframes == 0) return SF_OK;
  int rc = check_image(c, images, width, height, pitch, 3, "stereo pairs");
  if (rc != SF_OK) return rc;
  if (image_stride < (size_t)pitch * height)
    return sf_fail(c, SF_EINVAL, "image stride %zu is less than an image (%d rows of pitch %d)", image_stride, height, pitch);
  if ((rc = front_plan(c, width, height, &plan->front)) != SF_OK) return rc;
  plan->dp = arg_or_defaults(det, sf_detector_defaults);
  if (plan->dp.max_features <= 0 || plan->dp.max_features > SF_MAX_FEATURES)
    return sf_fail(c, SF_ERANGE, "max_features %d outside 1 .. %d (KeyPointVec.size is an int16)", plan->dp.max_features, SF_MAX_FEATURES);
  if ((rc = check_gftt(c, plan->dp.quality_level, plan->dp.min_distance)) != SF_OK) return rc;
  if ((rc = grid_plan(c, width, height, plan->dp.max_features, &plan->front)) != SF_OK) return rc;
  if (plan->front.grid() && (long long)n_keyframes * plan->front.rows * plan->front.cols > 65535)
    return sf_fail(c, SF_ERANGE, "%d keyframes of %d x %d cells: at most 65535 cells per call", n_keyframes, plan->front.rows, plan->front.cols);
  plan->prm = arg_or_defaults(flow, sf_stereo_flow_defaults);
  const sf_stereo_flow_params& prm = plan->prm;
  if (!c->stereo.optical_flow) {
    if ((rc = check_block_match(c, prm)) != SF_OK) return rc;
  } else if (prm.win_width <= 2 || prm.win_height <= 2 || (long long)prm.win_width * prm.win_height > 1024 || prm.max_level < 0 ||
      prm.max_level > 15 || !(prm.epsilon == prm.epsilon))
    return sf_fail(c, SF_EINVAL, "stereo flow parameters out of range (see sf_stereo_correspondences_device)");
  if ((long long)(width + 1) * (height + 1) * 255 > 0x7FFFFFFFll) return sf_fail(c, SF_ERANGE, "image too large for a 32-bit integral image");
  if (orb_call) {                                        // what sf_detect_orb_device refuses
    if ((rc = orb_detector_validate(c, c->orb_det, c->orb)) != SF_OK) return rc;
    if ((rc = check_pixels(c, width, height)) != SF_OK) return rc;
    if (n_keyframes > 65535) return sf_fail(c, SF_ERANGE, "ORB batch of %d keyframes (at most 65535)", n_keyframes);
    const SfOrbPyr P = sf_orb_pyr_layout(width, height, c->orb_det.scale_factor, c->orb_det.n_levels);
    for (int l = 0; l < P.n; ++l)
      if (P.w[l] < 1 || P.h[l] < 1)
        return sf_fail(c, SF_ERANGE, "pyramid level %d of a %d x %d image at scale %g is empty", l, width, height, (double)P.scale[l]);
  }
  if (surf_call) {                                       // what sf_detect_surf_device refuses
    if ((rc = surf_validate(c, c->surf)) != SF_OK) return rc;
    if ((rc = check_pixels(c, width, height)) != SF_OK) return rc;
    if (n_keyframes > 65535) return sf_fail(c, SF_ERANGE, "SURF batch of %d keyframes (at most 65535)", n_keyframes);
    SfSurfBatchPlan sp;                                  // (the layout's 2^31 plane samples)
    if ((rc = sf_surf_batch_plan_host(c, width, height, c->surf, n_keyframes, 0, 0, &sp)) != SF_OK) return rc;
  }
  if (sift_call) {                                       // what sf_detect_sift_device refuses
    if ((rc = sf_sift_validate(c, c->sift)) != SF_OK) return rc;
    if ((rc = check_pixels(c, width, height)) != SF_OK) return rc;
    if (n_keyframes > 65535) return sf_fail(c, SF_ERANGE, "SIFT batch of %d keyframes (at most 65535)", n_keyframes);
    SfSiftBatchPlan sp;                                  // (the image's sides, the 2^26 difference samples)
    if ((rc = sf_sift_batch_plan_host(c, width, height, c->sift, n_keyframes, 0, 0, &sp)) != SF_OK) return rc;
  }
  return SF_OK;
}

static int batch_reserve(sf_context* c, int n, int width, int height, BatchPlan* plan) {
  int rc;
  SF_HIP(c, hipSetDevice(c->device));
  if ((rc = extract_kind(c, &plan->kind)) != SF_OK) return rc;
  const int maxf = plan->front.rows_cap;                   // rows per keyframe: max_features, or the grid's R C quota
  const size_t rows_all = (size_t)maxf * n;
  if ((rc = sf_buf_reserve(c, c->ft_kpts, rows_all * sizeof(sf_keypoint))) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->ft_flow, rows_all * 16)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->ft_counts, (size_t)n * 4)) != SF_OK) return rc;
  if ((rc = sf_store_reserve(c, c->store, c->store.slots + n, maxf, plan->kind.bytes)) != SF_OK) return rc;
  if (fast_corners(c->feature_type) && (rc = check_pixels(c, width, height)) != SF_OK) return rc;
  if (c->feature_type == 0) {                              // the detector's planes, keys and integral images
    SfSurfBatchPlan sp;
    if ((rc = sf_surf_batch_reserve(c, width, height, c->surf, n, &sp)) != SF_OK) return rc;
  }
  // the chunk's planes, keys and counters; the blur tables, uploaded with the call's one wait when they are not the handle's
  if (c->feature_type == 1 && (rc = sf_sift_batch_reserve(c, width, height, c->sift, n)) != SF_OK) return rc;
  return SF_OK;
}

// The stages behind the detector -- refinement, stereo correspondence, extraction -- for the m images from i0 on of a batch
// of n whose keypoints and counts the detector has left in c->ft_kpts / c->ft_counts: every array at that sub-range, the
// store slots from slot + i0 on.  The whole batch is i0 = 0, m = n; type 1 comes here chunk by chunk.
static int batch_follow(sf_context* c, const BatchPlan& plan, const ExtractKind& kind, const uint8_t* d_left, const uint8_t* d_right,
                        int n, int i0, int m, int width, int height, int pitch, size_t image_stride, const sf_stereo_camera* cam,
                        int slot, int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out) {
  const int maxf = plan.front.rows_cap;
  const size_t rows_all = (size_t)maxf * n, r0 = (size_t)maxf * i0;
  const FrontPlan& fp = plan.front;
  int rc;
  d_left += (size_t)i0 * image_stride; d_right += (size_t)i0 * image_stride;
  sf_keypoint* d_kpts = (sf_keypoint*)c->ft_kpts.p + r0;
  const int32_t* d_n = (const int32_t*)c->ft_counts.p + i0;
  if (fp.launch() &&
      (rc = sf_launch_corner_subpix(c, d_left, image_stride, m, width, height, pitch, d_kpts, maxf, d_n, maxf, fp.off_x(), fp.off_y(),
                                    fp.refine ? c->front.subpix_win_size : 0, c->front.subpix_iterations, c->front.subpix_eps)) != SF_OK)
    return rc;
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

// Vis/FeatureType 1: the Gaussian planes the rows are computed from are too large to keep for a whole batch, so detector
// AND the stages behind it run chunk by chunk -- consecutive launches on the one stream, each chunk's extraction reading
// the pyramids before the next chunk's detector overwrites them
static int batch_launch_sift(sf_context* c, const BatchPlan& plan, const uint8_t* d_left, const uint8_t* d_right, int n, int width,
                             int height, int pitch, size_t image_stride, const sf_stereo_camera* cam, int slot, int32_t* d_rows_out,
                             uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out) {
  const int maxf = plan.front.rows_cap, chunk = c->sift_batch.chunk;
  SfSiftKind sift = {c->sift, false, true};
  ExtractKind kind = plan.kind;
  kind.sift = &sift;
  int rc;
  if ((rc = sf_sift_batch_begin(c)) != SF_OK) return rc;
  for (int i0 = 0; i0 < n; i0 += chunk) {
    const int m = std::min(chunk, n - i0);
    if ((rc = sf_launch_detect_sift_batch(c, d_left + (size_t)i0 * image_stride, image_stride, m, width, height, pitch, maxf, &c->sift,
                                          (sf_keypoint*)c->ft_kpts.p + (size_t)i0 * maxf, maxf, (int32_t*)c->ft_counts.p + i0)) != SF_OK)
      return rc;
    if ((rc = batch_follow(c, plan, kind, d_left, d_right, n, i0, m, width, height, pitch, image_stride, cam, slot, d_rows_out,
                           d_desc_out, d_xyz_out, d_kpts_out)) != SF_OK)
      return rc;
  }
  return SF_OK;
}

static int batch_launch(sf_context* c, const BatchPlan& plan, const uint8_t* d_left, const uint8_t* d_right, int n, int width,
                        int height, int pitch, size_t image_stride, const sf_stereo_camera* cam, int32_t* first_slot_out,
                        int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out) {
  const sf_detector_params& dp = plan.dp;
  const int maxf = plan.front.rows_cap;                    // rows per keyframe, everywhere below: max_features, or R C quota
  const int slot = c->store.slots;
  int rc;
  sf_keypoint* d_kpts = (sf_keypoint*)c->ft_kpts.p;
  int32_t* d_n = (int32_t*)c->ft_counts.p;
  ExtractKind kind = plan.kind;
  const FrontPlan& fp = plan.front;
  const uint8_t* d_roi = d_left + (size_t)fp.y * pitch + fp.x;   // the detector's images: the ROI, at the parent's pitch and stride
  if (c->feature_type == 1) {                            // (no ROI, no grid: front_plan, grid_plan)
    if ((rc = batch_launch_sift(c, plan, d_left, d_right, n, width, height, pitch, image_stride, cam, slot, d_rows_out, d_desc_out,
                                d_xyz_out, d_kpts_out)) != SF_OK)
      return rc;
    c->store.slots += n;
    if (first_slot_out) *first_slot_out = slot;
    return SF_OK;
  }
  if (c->feature_type == 2) {                            // (keypoints in level-0 coordinates; the pyramids stay for the extraction;
    rc = sf_launch_detect_orb_batch(c, d_left, image_stride, n, width, height, pitch, maxf, &c->orb_det, &c->orb, d_kpts, maxf, d_n);
    kind.pyr_stride = sf_orb_pyr_layout(width, height, c->orb_det.scale_factor, c->orb_det.n_levels).total;   // no ROI: front_plan)
  } else if (c->feature_type == 0) {                     // (no ROI, no grid: front_plan, grid_plan; the integral images stay
    rc = sf_launch_detect_surf_batch(c, d_left, image_stride, n, width, height, pitch, maxf, &c->surf, d_kpts, maxf, d_n);
    kind.integral_ready = true;                          // for the extraction)
  } else if (fp.grid()) {                                // the cells as the detector's images, joined by k_grid_gather
    rc = grid_detect(c, fp, dp, d_left, image_stride, n, pitch, d_kpts, d_n);
  } else if (fast_corners(c->feature_type)) {
    rc = sf_launch_detect_fast_batch(c, d_roi, image_stride, n, fp.w, fp.h, pitch, maxf, &c->fast, d_kpts, maxf, d_n);
  } else {
    rc = sf_launch_detect_corners_batch(c, d_roi, image_stride, n, fp.w, fp.h, pitch, maxf, dp.quality_level,
                                        dp.min_distance, d_kpts, maxf, d_n);
  }
  if (rc != SF_OK) return rc;
  if ((rc = batch_follow(c, plan, kind, d_left, d_right, n, 0, n, width, height, pitch, image_stride, cam, slot, d_rows_out, d_desc_out,
                         d_xyz_out, d_kpts_out)) != SF_OK)
    return rc;
  c->store.slots += n;
  if (first_slot_out) *first_slot_out = slot;
  return SF_OK;
}

static int features_batch(sf_context* c, BatchFamily family, const uint8_t* d_left, const uint8_t* d_right, int32_t n_keyframes,
                          int32_t width, int32_t height, int32_t pitch, size_t image_stride, const sf_stereo_camera* cam,
                          const sf_detector_params* det, const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                          int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out) {
  if (!c || !cam || n_keyframes < 0) return SF_EINVAL;
  BatchPlan plan;
  int rc = batch_check(c, family, d_left && d_right, n_keyframes, width, height, pitch, image_stride, det, flow, &plan);
  if (rc != SF_OK) return rc;
  if (n_keyframes == 0) { if (first_slot_out) *first_slot_out = c->store.slots; return SF_OK; }
  if ((rc = batch_reserve(c, n_keyframes, width, height, &plan)) != SF_OK) return rc;
  return batch_launch(c, plan, d_left, d_right, n_keyframes, width, height, pitch, image_stride, cam, first_slot_out, d_rows_out,
                      d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_get_features_and_descriptor_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                           int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                                                           size_t image_stride, const sf_stereo_camera* cam,
                                                           const sf_detector_params* det, const sf_stereo_flow_params* flow,
                                                           int32_t* first_slot_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                           float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return features_batch(c, BATCH_GENERIC, d_left, d_right, n_keyframes, width, height, pitch, image_stride, cam, det, flow, first_slot_out,
                        d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_get_features_and_descriptor_orb_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                               int32_t n_keyframes, int32_t width, int32_t height,
                                                               int32_t pitch, size_t image_stride, const sf_stereo_camera* cam,
                                                               const sf_detector_params* det,
                                                               const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                               int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out,
                                                               sf_keypoint* d_kpts_out) {
  return features_batch(c, BATCH_ORB, d_left, d_right, n_keyframes, width, height, pitch, image_stride, cam, det, flow, first_slot_out,
                        d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_get_features_and_descriptor_surf_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                                int32_t n_keyframes, int32_t width, int32_t height,
                                                                int32_t pitch, size_t image_stride, const sf_stereo_camera* cam,
                                                                const sf_detector_params* det,
                                                                const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                                int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out,
                                                                sf_keypoint* d_kpts_out) {
  return features_batch(c, BATCH_SURF, d_left, d_right, n_keyframes, width, height, pitch, image_stride, cam, det, flow, first_slot_out,
                        d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

// How many keyframes of the most recent SURF batch call had more maxima than their key capacity (they hold no rows)
extern "C" int sf_surf_batch_status(sf_handle c, int32_t* n_overflowed_out) {
  if (!c) return SF_EINVAL;
  if (n_overflowed_out) *n_overflowed_out = 0;
  SF_HIP(c, hipSetDevice(c->device));
  int32_t n = 0;
  if (c->surf_ctl.p) {
    const int rc = sf_word_to_host(c, c->surf_ctl.p, &n);
    if (rc != SF_OK) return rc;
  } else {
    SF_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (n_overflowed_out) *n_overflowed_out = n;
  if (n > 0)
    return sf_fail(c, SF_ERANGE, "SURF: %d keyframe(s) of the last batch call had more maxima than the candidate capacity and hold no rows; raise hessian_threshold",
                   n);
  return SF_OK;
}

extern "C" int sf_get_features_and_descriptor_sift_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                                int32_t n_keyframes, int32_t width, int32_t height,
                                                                int32_t pitch, size_t image_stride, const sf_stereo_camera* cam,
                                                                const sf_detector_params* det,
                                                                const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                                int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out,
                                                                sf_keypoint* d_kpts_out) {
  return features_batch(c, BATCH_SIFT, d_left, d_right, n_keyframes, width, height, pitch, image_stride, cam, det, flow, first_slot_out,
                        d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

// How many keyframes of the most recent SIFT batch call had more extrema or keypoints than an image holds (they hold no rows)
extern "C" int sf_sift_batch_status(sf_handle c, int32_t* n_overflowed_out) {
  if (!c) return SF_EINVAL;
  if (n_overflowed_out) *n_overflowed_out = 0;
  SF_HIP(c, hipSetDevice(c->device));
  int32_t n = 0;
  if (c->sift_ctl.p) {
    const int rc = sf_word_to_host(c, c->sift_ctl.p, &n);
    if (rc != SF_OK) return rc;
  } else {
    SF_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (n_overflowed_out) *n_overflowed_out = n;
  if (n > 0)
    return sf_fail(c, SF_ERANGE, "SIFT: %d keyframe(s) of the last batch call had more extrema or keypoints than the capacity of an image and hold no rows; raise contrast_threshold",
                   n);
  return SF_OK;
}

// ---- sf_experimental.h: small shapes for the tests of SURF's batch form ----------------------------------------------
extern "C" int sf_debug_surf_limits(sf_handle c, int32_t candidate_cap, int32_t batch_chunk) {
  if (!c) return SF_EINVAL;
  if (candidate_cap < 0 || (unsigned)candidate_cap > SURF_MAX_CANDIDATES || batch_chunk < 0 || batch_chunk > 65535)
    return sf_fail(c, SF_EINVAL, "sf_debug_surf_limits: candidate_cap %d outside 0 .. %u or batch_chunk %d outside 0 .. 65535", candidate_cap,
                   SURF_MAX_CANDIDATES, batch_chunk);
  c->surf_debug_cap = candidate_cap;
  c->surf_debug_chunk = batch_chunk;
  return SF_OK;
}

extern "C" int sf_surf_batch_plan(int32_t width, int32_t height, const sf_surf_params* surf, int32_t n_keyframes,
                                  int32_t* cap_img_out, int32_t* chunk_out, int64_t* workspace_bytes_out) {
  const sf_surf_params p = arg_or_defaults(surf, sf_surf_defaults);
  if (width < 3 || height < 3 || n_keyframes < 1 || n_keyframes > 65535) return SF_EINVAL;
  int rc = surf_validate(nullptr, p);
  if (rc != SF_OK) return rc;
  if ((long long)width * height > (1ll << 26) || (long long)(width + 1) * (height + 1) * 255 > 0x7FFFFFFFll) return SF_ERANGE;
  SfSurfBatchPlan sp;
  if ((rc = sf_surf_batch_plan_host(nullptr, width, height, p, n_keyframes, 0, 0, &sp)) != SF_OK) return rc;
  if (cap_img_out) *cap_img_out = (int32_t)sp.cap_img;
  if (chunk_out) *chunk_out = sp.chunk;
  if (workspace_bytes_out) *workspace_bytes_out = (int64_t)sp.workspace_bytes;
  return SF_OK;
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
  if ((rc = check_camera_image(c, d_src, format, width, height, src_pitch, 1, "source images")) != SF_OK) return rc;
  if ((rc = check_image(c, d_dst, width, height, dst_pitch, 1, "gray planes")) != SF_OK) return rc;
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
  int rc = check_camera_image(c, d_images, format, width, height, pitch, 1, "images");
  if (rc != SF_OK) return rc;
  if ((rc = check_stride(c, n_images, image_stride, pitch, height, image_row_bytes(format, width), "image")) != SF_OK) return rc;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_netvlad_infer_u8_batch_impl(c, d_images, format, n_images, height, width, pitch, image_stride, d_out, n_out);
}

// get_keyframes + compute_descriptors for n keyframes (data_handler.py:143-164, 212-295): gray planes of all 2 n stereo
// images (one launch), the network on the colour images, the batch feature stages on the planes, the descriptors' prefix
// into the local NN rows.  Everything that can refuse does so before the first launch; the store and the NN database
// grow last, together.
static int add_keyframes_batch(sf_context* c, BatchFamily family, const uint8_t* d_left, const uint8_t* d_right, const uint8_t* d_rgb,
                               int32_t format, int32_t n_keyframes, int32_t width, int32_t height, int32_t pitch,
                               size_t image_stride, const sf_stereo_camera* cam, const sf_detector_params* det,
                               const sf_stereo_flow_params* flow, int32_t* first_slot_out, int32_t* first_nn_row_out,
                               int32_t* d_rows_out, uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out) {
  if (!c || !cam || n_keyframes < 0) return SF_EINVAL;
  const int n = n_keyframes;
  int rc;
  if ((rc = check_format(c, format)) != SF_OK) return rc;
  if (n > 0) {
    if ((rc = check_camera_image(c, d_left && d_right, format, width, height, pitch, 3, "stereo pairs")) != SF_OK) return rc;
    if (image_stride < (size_t)pitch * height)
      return sf_fail(c, SF_EINVAL, "image stride %zu is less than an image (%d rows of pitch %d)", image_stride, height, pitch);
  }
  // the planes this call makes: rows padded to 16 bytes, n left then n right
  const int g_pitch = n > 0 ? (width + 15) & ~15 : 0;
  const size_t g_stride = ((size_t)g_pitch * (n > 0 ? height : 0) + 255) & ~(size_t)255;
  BatchPlan plan;
  if ((rc = batch_check(c, family, true, n, width, height, g_pitch, g_stride, det, flow, &plan)) != SF_OK) return rc;
  if (n == 0) {
    if (first_slot_out) *first_slot_out = c->store.slots;
    if (first_nn_row_out) *first_nn_row_out = c->nn_local.n;
    return SF_OK;
  }
  const int dims = c->params.netvlad_dimensions, pca_dim = sf_netvlad_pca_dim(c);
  if (pca_dim == 0) return sf_fail(c, SF_EINVAL, "no NetVLAD model loaded (sf_netvlad_load)");
  if (dims < 1 || dims > pca_dim)
    return sf_fail(c, SF_EINVAL, "netvlad_dimensions %d is beyond the loaded model's %d WPCA outputs", dims, pca_dim);
  if ((rc = sf_netvlad_check(c, n, height, width, dims)) != SF_OK) return rc;
  if ((rc = sf_nn_reserve_rows(c, c->nn_local, n, dims)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->img_gray, 2 * (size_t)n * g_stride)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->img_desc, (size_t)n * dims * sizeof(float))) != SF_OK) return rc;
  if ((rc = batch_reserve(c, n, width, height, &plan)) != SF_OK) return rc;
  uint8_t* g_left = (uint8_t*)c->img_gray.p;
  uint8_t* g_right = g_left + (size_t)n * g_stride;
  if ((rc = sf_launch_image_gray(c, d_left, d_right, n, format, c->gray_rule, width, height, pitch, image_stride, 2 * n, g_left,
                                 g_pitch, g_stride)) != SF_OK)
    return rc;
  if ((rc = sf_netvlad_infer_u8_batch_impl(c, d_rgb ? d_rgb : d_left, format, n, height, width, pitch, image_stride,
                                           (float*)c->img_desc.p, dims)) != SF_OK)
    return rc;
  int32_t slot = -1;
  if ((rc = batch_launch(c, plan, g_left, g_right, n, width, height, g_pitch, g_stride, cam, &slot, d_rows_out, d_desc_out,
                         d_xyz_out, d_kpts_out)) != SF_OK)
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
  return add_keyframes_batch(c, BATCH_GENERIC, d_left, d_right, d_rgb, format, n_keyframes, width, height, pitch, image_stride, cam, det,
                             flow, first_slot_out, first_nn_row_out, d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_add_keyframes_orb_u8_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                    const uint8_t* d_rgb, int32_t format, int32_t n_keyframes, int32_t width,
                                                    int32_t height, int32_t pitch, size_t image_stride,
                                                    const sf_stereo_camera* cam, const sf_detector_params* det,
                                                    const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                    int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                    float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return add_keyframes_batch(c, BATCH_ORB, d_left, d_right, d_rgb, format, n_keyframes, width, height, pitch, image_stride, cam, det,
                             flow, first_slot_out, first_nn_row_out, d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_add_keyframes_surf_u8_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                     const uint8_t* d_rgb, int32_t format, int32_t n_keyframes, int32_t width,
                                                     int32_t height, int32_t pitch, size_t image_stride,
                                                     const sf_stereo_camera* cam, const sf_detector_params* det,
                                                     const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                     int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                     float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return add_keyframes_batch(c, BATCH_SURF, d_left, d_right, d_rgb, format, n_keyframes, width, height, pitch, image_stride, cam, det,
                             flow, first_slot_out, first_nn_row_out, d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}

extern "C" int sf_add_keyframes_sift_u8_batch_device(sf_handle c, const uint8_t* d_left, const uint8_t* d_right,
                                                     const uint8_t* d_rgb, int32_t format, int32_t n_keyframes, int32_t width,
                                                     int32_t height, int32_t pitch, size_t image_stride,
                                                     const sf_stereo_camera* cam, const sf_detector_params* det,
                                                     const sf_stereo_flow_params* flow, int32_t* first_slot_out,
                                                     int32_t* first_nn_row_out, int32_t* d_rows_out, uint8_t* d_desc_out,
                                                     float* d_xyz_out, sf_keypoint* d_kpts_out) {
  return add_keyframes_batch(c, BATCH_SIFT, d_left, d_right, d_rgb, format, n_keyframes, width, height, pitch, image_stride, cam, det,
                             flow, first_slot_out, first_nn_row_out, d_rows_out, d_desc_out, d_xyz_out, d_kpts_out);
}
