// sf_feature_types.hip -- Vis/FeatureType: the table of the built types, their test tables, parameter blocks, validators and
// setters, the uploads of a type's device tables and the descriptor an extraction runs with (detectors: sf_detect.hip).
#include <cmath>
#include <vector>

#include "sf_host.hpp"

// ---- the feature types that are built (SfFeatureType: sf_host.hpp); a row ends where the rest is NULL ---------------------
#define GENERIC_CALLS "sf_get_features_and_descriptor_batch_device", "sf_add_keyframes_u8_batch_device"
static const SfFeatureType feature_types[] = {
    {0, "SURF", BATCH_SURF, CORNERS_OWN, ROWS_SURF, "sf_set_feature_type_surf", "sf_get_features_and_descriptor_surf_batch_device",
     "sf_add_keyframes_surf_u8_batch_device", "parameters of its own and a handle with desc_type 1",
     "Vis/FeatureType 0 (SURF) has batch forms of its own: sf_get_features_and_descriptor_surf_batch_device, sf_add_keyframes_surf_u8_batch_device",
     "; set the ratios to 0", "; set the grid to 1 x 1"},
    {1, "SIFT", BATCH_SIFT, CORNERS_OWN, ROWS_SIFT, "sf_set_feature_type_sift", "sf_get_features_and_descriptor_sift_batch_device",
     "sf_add_keyframes_sift_u8_batch_device", "parameters of its own and a handle with desc_type 1 and desc_bytes 512",
     "Vis/FeatureType 1 (SIFT): the batch form of type 1 is not built into this call: use sf_get_features_and_descriptor_sift_batch_device / sf_add_keyframes_sift_u8_batch_device",
     "; set the ratios to 0", "; set the grid to 1 x 1"},
    {2, "ORB", BATCH_ORB, CORNERS_OWN, ROWS_ORB, "sf_set_feature_type_orb", "sf_get_features_and_descriptor_orb_batch_device",
     "sf_add_keyframes_orb_u8_batch_device", "detector parameters",
     "Vis/FeatureType 2 (ORB on a pyramid) has batch forms of its own: sf_get_features_and_descriptor_orb_batch_device, sf_add_keyframes_orb_u8_batch_device",
     ": the batch form reuses the detector's pyramid for the descriptors; set the ratios to 0 or choose feature type 3, 4, 5, 6 or 8",
     ": every cell would need a pyramid of its own; set the grid to 1 x 1 or choose feature type 3, 4, 5, 6 or 8"},
    {3, "FAST/FREAK", BATCH_GENERIC, CORNERS_FAST, ROWS_FREAK, "sf_set_feature_type_freak", GENERIC_CALLS, "parameters of its own"},
    {4, "FAST/BRIEF", BATCH_GENERIC, CORNERS_FAST, ROWS_BRIEF, "sf_set_feature_type", GENERIC_CALLS},
    {5, "GFTT/FREAK", BATCH_GENERIC, CORNERS_GFTT, ROWS_FREAK, "sf_set_feature_type_freak", GENERIC_CALLS, "parameters of its own"},
    {6, "GFTT/BRIEF", BATCH_GENERIC, CORNERS_GFTT, ROWS_BRIEF, "sf_set_feature_type", GENERIC_CALLS},
    {8, "GFTT/ORB", BATCH_GENERIC, CORNERS_GFTT, ROWS_ORB, "sf_set_feature_type", GENERIC_CALLS},
};
// the same rows as sf_set_feature_type lists them to a caller who asked for a type that is not among them
static const char built_types[] = "1 = SIFT by sf_set_feature_type_sift, 0 = SURF by sf_set_feature_type_surf, 2 = ORB by sf_set_feature_type_orb, 3 = FAST/FREAK and 5 = GFTT/FREAK by sf_set_feature_type_freak, 4 = FAST/BRIEF, 6 = GFTT/BRIEF, 8 = GFTT/ORB";

const SfFeatureType* sf_feature_type_info(int feature_type) {
  for (const SfFeatureType& t : feature_types)
    if (t.type == feature_type) return &t;
  return nullptr;
}

const SfFeatureType& sf_type_of_family(BatchFamily family) {
  const SfFeatureType* t = feature_types;
  while (t->family != family) ++t;                         // (every family has a type)
  return *t;
}

// the types of binary rows need a keyframe store that holds them
static int check_binary_rows(sf_context* c, const SfFeatureType& t) {
  if (c->params.desc_type == 0) return SF_OK;
  return sf_fail(c, SF_EINVAL, "%s writes binary descriptors: a handle with desc_type %d cannot store them", t.name, c->params.desc_type);
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
  if (c->brief_bytes) return SF_OK;
  const int want = c->params.desc_bytes;
  c->brief_bytes = (want == 16 || want == 64) ? want : 32;
  sf_brief_default_pattern(c->brief_host, c->brief_bytes);
  return brief_upload(c);
}

extern "C" int sf_brief_get_pattern(sf_handle c, int8_t* tests, int32_t cap_bytes, int32_t* bytes) {
  if (!c || !bytes) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  int rc = check_binary_rows(c, sf_type_of(c).binary_rows() ? sf_type_of(c) : *sf_feature_type_info(6));   // (6: where a float handle starts)
  if (rc != SF_OK || (rc = brief_ensure(c)) != SF_OK) return rc;
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
  const SfFeatureType* t = sf_feature_type_info(feature_type);
  if (!t) return sf_fail(c, SF_EINVAL, "Vis/FeatureType %d is not built (%s)", feature_type, built_types);
  if (t->takes)
    return sf_fail(c, SF_EINVAL, "Vis/FeatureType %d (%s) takes %s: select it with %s", t->type, t->name, t->takes, t->setter);
  // (the handle's own type needs no second look: a handle with desc_type 1 starts at GFTT/BRIEF and may stay; on a
  //  handle with desc_type 2 the starting type is asked like any other: only SIFT writes its rows)
  if ((t != &sf_type_of(c) || c->params.desc_type == 2) && (rc = check_binary_rows(c, *t)) != SF_OK) return rc;
  if (t->rows == ROWS_ORB) {
    const sf_orb_params o = arg_or_defaults(orb, sf_orb_defaults);
    if ((rc = orb_validate(c, o)) != SF_OK) return rc;
    c->orb = o;
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

int sf_orb_detector_validate(sf_context* c, const sf_orb_detector_params& d, const sf_orb_params& o) {
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
  int rc = check_binary_rows(c, sf_type_of_family(BATCH_ORB));
  if (rc != SF_OK) return rc;
  const sf_orb_detector_params d = arg_or_defaults(det, sf_orb_detector_defaults);
  sf_orb_params o = arg_or_defaults(orb, sf_orb_defaults);
  if ((rc = sf_orb_detector_validate(c, d, o)) != SF_OK) return rc;
  o.orientation = 1;           // always the intensity centroid, computed by the detector
  c->orb_det = d;
  c->orb = o;
  c->feature_type = 2;
  return SF_OK;
}

extern "C" int sf_get_orb_detector(sf_handle c, sf_orb_detector_params* out) { return get_block(c, out, &sf_context::orb_det); }

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
  const SfFeatureType* t = sf_feature_type_info(feature_type);
  if (!t || t->rows != ROWS_FREAK)
    return sf_fail(c, SF_EINVAL, "sf_set_feature_type_freak selects Vis/FeatureType 3 (FAST/FREAK) or 5 (GFTT/FREAK), not %d", feature_type);
  int rc = check_binary_rows(c, *t);
  if (rc != SF_OK) return rc;
  const sf_freak_params f = arg_or_defaults(freak, sf_freak_defaults);
  if ((rc = freak_validate(c, f)) != SF_OK) return rc;
  if (memcmp(&f, &c->freak, sizeof f) != 0) c->freak_pattern_ok = c->freak_tables_ok = false;   // rebuilt by the next extraction
  c->freak = f;
  c->feature_type = feature_type;
  return SF_OK;
}

extern "C" int sf_get_freak_params(sf_handle c, sf_freak_params* out) { return get_block(c, out, &sf_context::freak); }

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
int sf_surf_validate(sf_context* c, const sf_surf_params& p) {
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
extern "C" int sf_surf_check_params(const sf_surf_params* params) { return sf_surf_validate(nullptr, arg_or_defaults(params, sf_surf_defaults)); }

extern "C" int sf_set_feature_type_surf(sf_handle c, const sf_surf_params* surf) {
  if (!c) return SF_EINVAL;
  if (c->params.desc_type != 1)
    return sf_fail(c, SF_EINVAL, "SURF writes float32 descriptors: a handle with desc_type %d cannot store them (create it with desc_type 1 and desc_bytes 256, or 512 for extended rows)",
                   c->params.desc_type);
  const sf_surf_params p = arg_or_defaults(surf, sf_surf_defaults);
  int rc = sf_surf_validate(c, p);
  if (rc != SF_OK) return rc;
  const int bytes = p.extended ? 512 : 256;
  if (c->params.desc_bytes != bytes)
    return sf_fail(c, SF_EINVAL, "SURF rows with extended %d are %d bytes: the handle was created with desc_bytes %d", p.extended, bytes,
                   c->params.desc_bytes);
  c->surf = p;
  c->feature_type = 0;
  return SF_OK;
}

extern "C" int sf_get_surf_params(sf_handle c, sf_surf_params* out) { return get_block(c, out, &sf_context::surf); }

// ---- the SIFT detector (kernels, tables and plan in k_sift.hip) ------------------------------------------------------------
extern "C" int sf_sift_check_params(const sf_sift_params* params) { return sf_sift_validate(nullptr, arg_or_defaults(params, sf_sift_defaults)); }

extern "C" int sf_set_feature_type_sift(sf_handle c, const sf_sift_params* sift) {
  if (!c) return SF_EINVAL;
  const bool u8_rows = c->params.desc_type == 2 && c->params.desc_bytes == SF_DESC_BYTES_U8;   // (the same 128 integers as bytes)
  if (!u8_rows && (c->params.desc_type != 1 || c->params.desc_bytes != 512))
    return sf_fail(c, SF_EINVAL, "SIFT writes 128 float32 per row: a handle with desc_type %d and desc_bytes %d cannot store them (create it with desc_type 1 and desc_bytes 512)",
                   c->params.desc_type, c->params.desc_bytes);
  const sf_sift_params p = arg_or_defaults(sift, sf_sift_defaults);
  const int rc = sf_sift_validate(c, p);
  if (rc != SF_OK) return rc;
  c->sift = p;
  c->feature_type = 1;
  return SF_OK;
}

extern "C" int sf_get_sift_params(sf_handle c, sf_sift_params* out) { return get_block(c, out, &sf_context::sift); }

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

// what the two *_batch_plan calls hand back of a plan
template <class Plan>
static int batch_plan_out(const Plan& sp, int32_t* cap_img_out, int32_t* chunk_out, int64_t* workspace_bytes_out) {
  if (cap_img_out) *cap_img_out = (int32_t)sp.cap_img;
  if (chunk_out) *chunk_out = sp.chunk;
  if (workspace_bytes_out) *workspace_bytes_out = (int64_t)sp.workspace_bytes;
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
  return batch_plan_out(sp, cap_img_out, chunk_out, workspace_bytes_out);
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
  int rc = sf_surf_validate(nullptr, p);
  if (rc != SF_OK) return rc;
  if (!sf_pixels_fit(width, height) || !sf_integral_fits(width, height)) return SF_ERANGE;   // (no handle: the bare code)
  SfSurfBatchPlan sp;
  if ((rc = sf_surf_batch_plan_host(nullptr, width, height, p, n_keyframes, 0, 0, &sp)) != SF_OK) return rc;
  return batch_plan_out(sp, cap_img_out, chunk_out, workspace_bytes_out);
}

// ---- FAST (Vis/FeatureType 4; kernels in k_fast.hip) ---------------------------------------------------------------
extern "C" void sf_fast_defaults(sf_fast_params* p) {
  if (!p) return;
  p->threshold = 20;           // FAST/Threshold [upstream rtabmap Parameters.h]
  p->nonmax_suppression = 1;   // FAST/NonmaxSuppression
}

int sf_fast_validate(sf_context* c, const sf_fast_params& f) {
  if (f.threshold < 1 || f.threshold > 254) return sf_fail(c, SF_EINVAL, "FAST threshold %d outside 1 .. 254", f.threshold);
  if (f.nonmax_suppression != 0 && f.nonmax_suppression != 1)
    return sf_fail(c, SF_EINVAL, "FAST nonmax_suppression %d is neither 0 nor 1", f.nonmax_suppression);
  return SF_OK;
}

extern "C" int sf_fast_set_params(sf_handle c, const sf_fast_params* params) {
  if (!c || !params) return SF_EINVAL;
  int rc = sf_fast_validate(c, *params);
  if (rc != SF_OK) return rc;
  c->fast = *params;
  return SF_OK;
}

extern "C" int sf_fast_get_params(sf_handle c, sf_fast_params* params) { return get_block(c, params, &sf_context::fast); }

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

// The descriptor of the handle's feature type (ExtractKind: sf_internal.hpp), its tables on the device
int sf_extract_kind(sf_context* c, ExtractKind* k) {
  const SfFeatureType& t = sf_type_of(c);
  int rc;
  *k = ExtractKind();
  if (t.binary_rows() && (rc = check_binary_rows(c, t)) != SF_OK) return rc;
  switch (t.rows) {
    case ROWS_SIFT:                                        // (selected on a handle with desc_type 1 and 512-byte rows, or desc_type 2, only)
      k->sift.u8 = c->params.desc_type == 2;
      k->bytes = k->sift.u8 ? SF_DESC_BYTES_U8 : 512; k->has_sift = true; k->sift.prm = c->sift;
      return SF_OK;
    case ROWS_SURF:                                        // (selected on a handle with desc_type 1 and these row bytes only)
      k->bytes = c->surf.extended ? 512 : 256; k->surf = &c->surf_dev;
      return surf_ensure(c);
    case ROWS_FREAK:
      k->bytes = FREAK_BYTES; k->freak = &c->freak_dev;
      return freak_ensure(c);
    case ROWS_ORB:                                         // (type 2: a keypoint's rows on its own level of the detector's pyramid)
      if ((rc = orb_ensure(c)) != SF_OK) return rc;
      k->bytes = 32; k->d_tests = (const int8_t*)c->orb_tests.p; k->orb = &c->orb;
      if (t.family == BATCH_ORB) k->pyr = &c->orb_det;
      return SF_OK;
    case ROWS_BRIEF:
      if ((rc = brief_ensure(c)) != SF_OK) return rc;
      k->bytes = c->brief_bytes; k->d_tests = (const int8_t*)c->brief_tests.p;
      return SF_OK;
  }
  return SF_EINVAL;
}
