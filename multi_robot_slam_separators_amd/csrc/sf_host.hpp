// sf_host.hpp -- what the host translation units (sf_handle.hip, sf_store.hip, sf_feature_types.hip, sf_detect.hip,
// sf_keyframes.hip, sf_verify_host.hip, sf_step.hip, sf_placement.hip) need from each other; the kernel translation units
// do not include it.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>

#include "sf_internal.hpp"

// ---- sf_handle.hip ------------------------------------------------------------------------------------------------------
int sf_fill_device_params(sf_context* c);      // validates c->params and derives c->dparams
void sf_env_knobs(sf_context* c);              // the SF_* environment knobs of a handle, applied to `c`
void sf_guided_grid(int image_width, int image_height, int guess_win_size, int32_t* gx, int32_t* gy, float* inv_cell);
void sf_camera_derive(const sf_camera_model& m, int guess_win_size, CameraBlock* b);   // a table entry from a model

// ---- sf_store.hip -------------------------------------------------------------------------------------------------------
int sf_validate_features(sf_context* c, const sf_features* f);
int sf_store_reserve(sf_context* c, Store& s, int slots_needed, int rows, int cols);
int sf_store_add_host_batch(sf_context* c, Store& st, const sf_features* const* feats, int n, int* first_slot);
void sf_ingest_pool_destroy(sf_context* c);

// ---- the feature front end: sf_feature_types.hip, sf_detect.hip, sf_keyframes.hip ------------------------------------------
#pragma GCC visibility push(hidden)            // (shared by the three; the library exports none of it)
// What the front end knows about a Vis/FeatureType, said once: a row of the table in sf_feature_types.hip
enum BatchFamily { BATCH_GENERIC, BATCH_ORB, BATCH_SURF, BATCH_SIFT };   // whose batch calls reach the type
enum CornerSource { CORNERS_GFTT, CORNERS_FAST, CORNERS_OWN };           // OWN: the family's detector
enum RowKind { ROWS_BRIEF, ROWS_ORB, ROWS_FREAK, ROWS_SURF, ROWS_SIFT };
struct SfFeatureType {
  int type;
  const char* name;
  BatchFamily family; CornerSource corners; RowKind rows;
  const char *setter, *get_features_batch, *add_keyframes_batch;   // the call that selects the type, its two batch calls
  const char* takes;                           // what sf_set_feature_type says the setter takes; NULL: it selects the type itself
  const char* other_call;                      // the refusal of a batch call of another family; NULL: the call's family words it
  const char *no_roi, *no_grid;                // how the refusal of a ROI / a grid under the type ends; NULL: built
  bool binary_rows() const { return rows == ROWS_BRIEF || rows == ROWS_ORB || rows == ROWS_FREAK; }
};
const SfFeatureType* sf_feature_type_info(int feature_type);   // NULL: not built
inline const SfFeatureType& sf_type_of(const sf_context* c) { return *sf_feature_type_info(c->feature_type); }   // (always built)
const SfFeatureType& sf_type_of_family(BatchFamily family);    // the type behind the _orb_, _surf_ and _sift_ calls
int sf_orb_detector_validate(sf_context* c, const sf_orb_detector_params& d, const sf_orb_params& o);
int sf_surf_validate(sf_context* c, const sf_surf_params& p);
int sf_fast_validate(sf_context* c, const sf_fast_params& f);
int sf_extract_kind(sf_context* c, ExtractKind* k);            // the descriptor of the handle's type, its tables uploaded

// `present`: every image pointer of the call is there; min_side 3 where a detector runs (its 3 x 3 neighbourhoods)
inline int sf_check_image(sf_context* c, bool present, int width, int height, int pitch, int min_side, const char* what) {
  if (!present || width < min_side || height < min_side || pitch < width)
    return sf_fail(c, SF_EINVAL, "%s missing or malformed (%d x %d, pitch %d)", what, width, height, pitch);
  return SF_OK;
}
// the detectors' sort keys hold a pixel index beside a score; the integral image of 8-bit pixels holds int32 sums
inline bool sf_pixels_fit(int width, int height) { return (long long)width * height <= (1ll << 26); }
inline bool sf_integral_fits(int width, int height) { return (long long)(width + 1) * (height + 1) * 255 <= 0x7FFFFFFFll; }
inline int sf_check_pixels(sf_context* c, int width, int height) {
  return sf_pixels_fit(width, height) ? SF_OK : sf_fail(c, SF_ERANGE, "image of %d x %d pixels is too large", width, height);
}
inline int sf_check_integral(sf_context* c, int width, int height) {
  return sf_integral_fits(width, height) ? SF_OK : sf_fail(c, SF_ERANGE, "image too large for a 32-bit integral image");
}
// what the pyramidal flow refuses of its parameters (the single call says which, the batch calls in one message)
inline bool sf_stereo_flow_ok(const sf_stereo_flow_params& p) {
  return p.win_width > 2 && p.win_height > 2 && (long long)p.win_width * p.win_height <= 1024 && p.max_level >= 0 && p.max_level <= 15 &&
         p.epsilon == p.epsilon;
}
// the caller's parameter block, or the defaults when it passed none
template <class T>
static T arg_or_defaults(const T* given, void (*defaults)(T*)) {
  T v;
  if (given) v = *given; else defaults(&v);
  return v;
}
// the sf_get_* / sf_*_get_params calls: the handle's copy of a parameter block
template <class T>
static int get_block(const sf_context* c, T* out, T sf_context::*held) {
  if (!c || !out) return SF_EINVAL;
  *out = c->*held;
  return SF_OK;
}

// What the extraction calls do around their detector (sf_detect.hip): the ROI of the handle's ratios on a width x height
// image and whether the corners are refined.  Refuses, before anything is touched, what the two steps cannot do.
struct FrontPlan {
  int x = 0, y = 0, w = 0, h = 0;
  bool refine = false;
  // Vis/GridRows x Vis/GridCols (sf_grid_plan): the cells, what each may keep, the rows a keyframe can hold (1 x 1: the ROI,
  // max_features, max_features).  Under a grid k_grid_gather shifts the keypoints, not k_corner_subpix
  int rows = 1, cols = 1, col_size = 0, row_size = 0, quota = 0, rows_cap = 0;
  bool grid() const { return rows * cols > 1; }
  bool launch() const { return refine || (!grid() && (x || y)); }   // (an offset of zero and no refinement: no launch at all)
  int off_x() const { return grid() ? 0 : x; }
  int off_y() const { return grid() ? 0 : y; }
};
int sf_front_plan(sf_context* c, int width, int height, FrontPlan* fp);
int sf_grid_plan(sf_context* c, int width, int height, int max_features, FrontPlan* fp);
int sf_grid_detect(sf_context* c, const FrontPlan& fp, const sf_detector_params& dp, const uint8_t* d_left, size_t image_stride,
                   int n, int pitch, sf_keypoint* d_kpts, int32_t* d_n, const SfMask& mask = SfMask());
// a detector mask on the ROI whose first pixel is (x, y) of its planes (no mask stays no mask)
inline SfMask sf_mask_at(const SfMask& mask, int x, int y) {
  SfMask m = mask;
  if (m.p) m.p += (size_t)y * mask.pitch + x;
  return m;
}
// The n depth images of a depth call on width x height images (sf_detect.hip): D's own size from the handle (sf_depth_set_size;
// unset: the image's), then what the depth calls refuse of such images; `call` opens the message.  n = 0: the format alone
int sf_depth_in(sf_context* c, const char* call, SfDepthIn* D, int width, int height, int n);
// whether the depth keyframe calls make a mask of D on width x height images: Vis/DepthAsMask, and a size that divides the image's
inline bool sf_depth_masks(const sf_context* c, const SfDepthIn& D, int width, int height) {
  return c->depth.depth_as_mask && sf_depth_interpolation_factor(width, height, D.w ? D.w : width, D.h ? D.h : height) != 0;
}
int sf_check_gftt(sf_context* c, double quality_level, double min_distance);
int sf_gftt_validate(sf_context* c, const sf_gftt_params& g);
// the GFTT window on what the detector is given (`what`: an image, a ROI, a grid cell): a side below GFTT/BlockSize is refused
int sf_check_gftt_side(sf_context* c, int width, int height, const char* what);
int sf_check_block_match(sf_context* c, const sf_stereo_flow_params& prm);   // what sf_stereo_block_match_device refuses
#pragma GCC visibility pop

// ---- sf_verify_host.hip -------------------------------------------------------------------------------------------------
// ONE object decides the launch form of a verification call AND what its workspace must hold: it is made once per call
// from the call's total pair count, the workspace is reserved from it and every chunk is launched from it.  (Round 3 made
// the form decision per chunk and the reservation per call: the second chunk of a 140 000-candidate step took the split
// form, which writes correspondence lists, on a workspace reserved for the fused form, which has none -- a device
// out-of-bounds write; tests/test_gpu_step.py::test_step_queries_across_the_form_and_chunk_boundaries.)
struct VerifyPlan {
  enum Form { STAGES = 0, FUSED = 1, SPLIT = 2, SPLIT_PNP = 3, HALVES = 4 } form = STAGES;
  bool lists = true;        // the correspondence lists live in HBM (every form but the plain fused kernel)
  bool single = false;      // one launch sequence on one stream: a pair's index IS its position in the call
  bool narrow_est = false;  // SPLIT only: the survivors' chains as three launches, the estimates one wavefront wide (k_chain_est)
  bool cameras = false;     // a slot of the store carries a camera id: STAGES / HALVES, their kernels in the camera forms
  bool streams() const { return single && (form == FUSED || form == SPLIT || form == SPLIT_PNP); }   // chain kernels that can
};                                                                                                // stream accepted results
VerifyPlan sf_verify_plan(const sf_context* c, const StoreView& v, int n);
int sf_verify_device(sf_context* c, const Store& st, const int32_t* d_from, const int32_t* d_to, int n, sf_result* d_out,
                     const VerifyPlan* given = nullptr);
int sf_compact_launch(sf_context* c, const sf_result* d_results, int n, sf_result* d_accepted, uint8_t* d_flags,
                      int32_t* d_count, const int32_t* index = nullptr, sf_result* d_accepted2 = nullptr,
                      uint8_t* d_flags2 = nullptr, int32_t* d_count2 = nullptr, int cap2 = 0x7FFFFFFF);

// ---- sf_placement.hip ---------------------------------------------------------------------------------------------------
// A stream beside the handle's own: the copy stream of the synchronous speculative call, the main stream of step lane k, or
// lane k's second stream (the device walk beside the verification)
enum SideStream { SF_STREAM_COPY, SF_STREAM_LANE, SF_STREAM_AUX };
int sf_side_stream(sf_context* c, SideStream role, int k, hipStream_t* out);
