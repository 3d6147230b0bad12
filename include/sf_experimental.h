/*
 * sf_experimental.h -- entry points of libsepfinder.so that are NOT part of the drop-in surface (include/sepfinder.h).
 *
 * They are the building blocks sf_step_issue / sf_step_retire are made of, exported for the library's own tests, for
 * tools/ and for bench.py's diagnostic variants (BENCH_NO_STREAM, the N > 1 fallbacks).  No reference interface
 * corresponds to them one to one (the loop they serve is PKG/scripts/find_separators.py:59-133); a host written against
 * the reference needs none of them, and they may change without a bump of SF_ABI_VERSION.
 */
#ifndef SF_EXPERIMENTAL_H
#define SF_EXPERIMENTAL_H

#include "sepfinder.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sf_find_matches_and_verify_device with d_out = NULL leaves the results where the verification wrote them, and
   sf_last_match_results says where: the record of match i is d_results[index ? index[i] : i] (index, if not NULL, is
   device-readable pinned host memory owned by the handle, valid until the next sf_find_matches_and_verify_device).
   sf_compact_accepted_indexed_device_async consumes exactly that pair (any index == NULL means "in order"), so a
   caller that only needs the ACCEPTED separators saves the gathered copy of all of them.                        */
int  sf_last_match_results(sf_handle h, const sf_result** d_results, const int32_t** index, int32_t* n);
int  sf_compact_accepted_indexed_device_async(sf_handle h, const sf_result* d_results, const int32_t* index,
                                              int32_t n, sf_result* d_accepted, uint8_t* d_flags,
                                              int32_t* d_n_accepted);
/* The same with every output written TWICE: accepted records, flags and count also go to d_accepted2 / d_flags2
   (optional) / d_n_accepted2 -- e.g. a collective's send buffer on the device AND this rank's own copy in pinned host
   memory, without a copy behind the kernel (bench.py, N > 1).                                                     */
int  sf_compact_accepted_indexed_mirrored_device_async(sf_handle h, const sf_result* d_results, const int32_t* index,
                                                       int32_t n, sf_result* d_accepted, uint8_t* d_flags,
                                                       int32_t* d_n_accepted, sf_result* d_accepted2, uint8_t* d_flags2,
                                                       int32_t* d_n_accepted2);

/* Accepted results STREAMED out of the verification kernels (both estimators; the speculative path of
   sf_find_matches_and_verify_device): every pair whose result is accepted writes its record into the selected block
   the moment it is final -- posted writes beside the other pairs' work -- instead of a compaction kernel behind the
   launch.  A block = host-pinned (device-accessible) arrays: records [cap], index [cap] (the record's slot in the
   sf_last_match_results block, i.e. match i owns the record whose index equals index_of_match[i]), flags [pairs]
   (optional: success of EVERY verified slot, 0 for slots without a candidate -- if that array is host memory every
   pair ends on a 1-byte PCIe write its workgroup has to see acknowledged, measured as +10 us on a 10 000-pair launch:
   pass NULL and derive the flags from the index list, whose entries beyond the streamed count keep their old value).  Records arrive in completion order and
   cover every verified candidate (a superset of the matches when a row had several candidates): the host keeps those
   whose index is a match's.  Their number is the sum of flags over the `pairs` slots sf_accept_stream_status reports.
   Two blocks can be registered and selected alternately, so that one query's separators stay untouched while the
   next one runs.  `streamed` = 0 after a call that could not stream (fallback paths): use the compaction then.     */
/* d_records2 (optional): every record is written there too, at the same slot -- e.g. a collective's send buffer on the
   device.  d_counter (optional): the slot counter is this device word instead of the handle's own; the CALLER zeroes
   it before each query (e.g. the count header of that send buffer, so that the all-gather can start behind the
   verification with nothing in between).                                                                       */
int  sf_accept_stream_set(sf_handle h, int32_t which, sf_result* records, int32_t* index, uint8_t* flags, int32_t cap,
                          sf_result* d_records2, uint32_t* d_counter);
int  sf_accept_stream_select(sf_handle h, int32_t which);      /* 0 / 1, -1 = off (default) */
int  sf_accept_stream_status(sf_handle h, int32_t* streamed, int32_t* pairs);

/* Which kernels are bracketed (bit k = kernel k of the enum above; default all).  Two timing events per launch cost
   host time and a marker on the queue -- about 4 us per bracketed launch in a 0.6 ms step -- so a throughput
   measurement brackets only the kernel it prices (bench.py: the dominant one) and surveys the rest separately.  */
int  sf_prof_select(sf_handle h, uint32_t kernel_mask);
/* One line on where the step pipeline's streams were placed on the hardware's dispatch pipes (measured once per handle at
   the first step that needs a second stream: sf_placement.hip place_streams; SF_STREAM_PLACEMENT=0 in the environment turns the
   measurement off, =2 also prints the line to stderr). */
int  sf_stream_placement(sf_handle h, char* buf, size_t n);
/* Runs that measurement now instead of inside the first step that needs a second stream (60-100 ms once per handle:
   ~100 short chip-filling launches on the handle's stream and on streams of the library's own; it waits for the
   handle's own streams only).  Work of other streams or processes on the GPU at that moment changes what is measured:
   call it at a quiet moment, read sf_stream_placement for what was picked or why it was abandoned.  Idempotent;
   SF_STREAM_PLACEMENT=0 makes it a no-op.                                                                        */
int  sf_streams_prepare(sf_handle h);

/* Pass state of pair `pair` of the last verification (diagnostics, tools/diag_pair_index.py): pose of the pass (row-major
   3 x 4, p_from = T p_to; all zero when null), is_null / inliers / matches.  Needs SF_OPT_DEBUG_CORR like
   sf_debug_correspondences.                                                                                     */
int  sf_debug_pass_state(sf_handle h, int32_t pair, int32_t pass, float* T12, int32_t* is_null, int32_t* inliers,
                         int32_t* matches);
/* Diagnostic counters the kernels bump when the process runs with SF_DIAG set (experiments; zero otherwise).      */
int  sf_debug_counters(sf_handle h, unsigned long long* out, int32_t n);
int  sf_debug_guided_points(sf_handle h, int32_t pair, unsigned long long* plane0, unsigned long long* plane1,
                            int32_t* kcap_out);

/* The launch plan of a verification call of n_pairs pairs on keyframes of `kcap` feature slots (a multiple of 64) and
   `desc_words` dwords per descriptor row, and its workspace -- computed on the host, no device needed (a test without a
   GPU holds the reservation against what each launch form writes: the out-of-bounds write of round 3 was a form that
   writes correspondence lists on a workspace reserved without them).  out (>= 22 values): [0] form (0 stages, 1 fused,
   2 split, 3 split PnP, 4 two-stream halves), [1] lists in HBM, [2] one chunk, [3] pairs of the largest launch
   sequence, [4..12] bytes reserved for corr1, corr2, hdr1, hdr2, pass1, pass2, list1, list3, flags, [13..21] bytes the
   form's launches write to them; with n_out >= 23 also [22] = 1 where the split form runs its estimates as the
   one-wavefront launches of SF_OPT_CHAIN_NARROW_EST.                                                             */
int  sf_debug_plan_workspace(const sf_params* p, int32_t kcap, int32_t desc_words, int32_t n_pairs,
                             int32_t in_overlapped_step, int32_t debug_corr, int64_t* out, int32_t n_out);
/* What the library's handles hold at this moment, over the whole process: out[0] device blocks, [1] their bytes, [2]
   pinned host blocks, [3] events (the profiling brackets' recycled timing events apart).  Counted where the handle's owning
   types allocate and free, not read from the driver: a test on any machine can hold "sf_destroy returns everything" to
   it, also on a card that other work shares.  No handle, no GPU needed.                                           */
void sf_debug_live_resources(int64_t out[4]);

/* The two Gaussian tables of SURF (Vis/FeatureType 0), handle-free and usable without a GPU; float64 arithmetic, every
   weight rounded to float32 once.  ori_xy [109][2] int8 {x, y}: the lattice points with x^2 + y^2 < 36, x outer, y
   inner; ori_w [109]: g13[x + 6] g13[y + 6], g13 = the normalised 13-tap Gaussian of sigma 2.5; desc_w [400]:
   g20[i] g20[j] at 20 i + j, sigma 3.3.  Any output may be NULL.                                                  */
void sf_surf_build_tables(float* ori_w, int8_t* ori_xy, float* desc_w);
/* The ranges sf_set_feature_type_surf and sf_detect_surf_device hold sf_surf_params to, without a handle: SF_OK or
   SF_EINVAL; NULL = the defaults.                                                                                 */
int  sf_surf_check_params(const sf_surf_params* params);
/* The ranges sf_gftt_set_params holds sf_gftt_params to, without a handle: SF_OK or SF_EINVAL; NULL = the defaults.   */
int  sf_gftt_check_params(const sf_gftt_params* params);
/* What sf_rectify_plan_create holds an sf_camera_info to, without a handle or a GPU: SF_OK or SF_EINVAL.  iR_out (may be
   NULL) receives the nine values of (P[:, :3] R)^-1, row-major, as the plan keeps them.                             */
int  sf_rectify_check_info(const sf_camera_info* info, double* iR_out);
/* Small shapes and single stages for the tests and the latency tool of sf_depth_register_device; a fresh handle behaves as
   if it had not been called.  batch_chunk (0 = what the 256 MB workspace allows, at most 65535): the images per chunk.
   stages (0 = all, else a sum of 1 = the z-buffer's initialisation, 2 = the scatter, 4 = the resolve): what a call
   queues -- a call without stage 4 writes no output.  Out of range: SF_EINVAL, nothing changes.                   */
int  sf_debug_depth_register_limits(sf_handle h, int32_t batch_chunk, int32_t stages);
/* Small shapes for the tests of SURF's batch form; a fresh handle behaves as if neither had been called.  candidate_cap
   (0 = the default, at most 262144) takes the place of the 262144 maxima an image may have, in sf_detect_surf_device
   and the single extraction calls (more: SF_ERANGE) and in the batch forms (more: the keyframe holds no rows, see
   sf_surf_batch_status); batch_chunk (0 = what the 256 MB workspace allows, at most 65535) is the number of images the
   batch detector runs per chunk.  Out of range: SF_EINVAL, nothing changes.                                       */
int  sf_debug_surf_limits(sf_handle h, int32_t candidate_cap, int32_t batch_chunk);
/* The host arithmetic of the SURF batch forms for n_keyframes images of width x height, without a GPU or a handle (surf
   NULL = the defaults): *cap_img_out = min(262144, B), B = the sum over octaves o and middle layers l = 1 ..
   n_octave_layers of ceil(r / 2) ceil(c / 2) with r = max((height >> o) - 2 m, 0), c = max((width >> o) - 2 m, 0) and
   m = (((9 + 6 (l + 1)) << o) / 2 >> o) + 1; *chunk_out = the images per chunk, min(n_keyframes, 65535, 2^31 - 1 keys,
   the 256 MB workspace / bytes per image), at least 1; bytes per image = 8 per plane sample + 16 per key (at least one
   key) + 16; *workspace_bytes_out = chunk x bytes per image.  Any output may be NULL.  SF_EINVAL: parameters out of
   range, an image below 3 x 3, n_keyframes outside 1 .. 65535; SF_ERANGE: what sf_detect_surf_device refuses of an
   image's size.                                                                                                   */
int  sf_surf_batch_plan(int32_t width, int32_t height, const sf_surf_params* surf, int32_t n_keyframes,
                        int32_t* cap_img_out, int32_t* chunk_out, int64_t* workspace_bytes_out);


/* The SIFT detector's host arithmetic, handle-free and usable without a GPU (params NULL = the defaults; out-of-range
   parameters: SF_EINVAL).  sf_sift_check_params: the ranges sf_detect_sift_device holds sf_sift_params to.
   sf_sift_build_tables, for i = 0 .. n_octave_layers + 2: sigmas[i] = the blur (float64, libm) that makes the enlarged
   image's first plane (i = 0: sqrt(max(sigma^2 - 1, 0.01))) or Gaussian plane i from plane i - 1 (sigma k^(i-1)
   sqrt(k^2 - 1), k = 2^(1/n)); lengths[i] = cvRound(8 sigmas[i] + 1) | 1; coef[520 i + t] = tap t of
   cv::getGaussianKernel: float64 exp, divided by the sum taken in index order, rounded to float32 once (zero beyond the
   length).  Any output may be NULL.
   sf_sift_plan: the octaves of a width x height image -- their number, widths[16] and heights[16] (zero beyond it), and
   the int16 samples of all Gaussian and all difference planes.  SF_EINVAL: a side below 3; SF_ERANGE: a side above
   16384 or more than 2^26 difference samples.                                                                       */
int  sf_sift_check_params(const sf_sift_params* params);
int  sf_sift_build_tables(const sf_sift_params* params, double* sigmas, int32_t* lengths, float* coef);
int  sf_sift_plan(int32_t width, int32_t height, const sf_sift_params* params, int32_t* n_octaves_out, int32_t* widths,
                  int32_t* heights, int64_t* gauss_samples_out, int64_t* dog_samples_out);
/* candidate_cap (0 = the default, at most 262144) takes the place of the 262144 extrema, and keypoints, an image may have
   in sf_detect_sift_device (more: SF_ERANGE) and in every image of the batch forms (more: the keyframe holds no rows, see
   sf_sift_batch_status).  Out of range: SF_EINVAL, nothing changes.                                                */
int  sf_debug_sift_limits(sf_handle h, int32_t candidate_cap);
/* batch_chunk (0 = what the 1 GB workspace allows, at most 65535) is the number of images the SIFT batch forms run per
   chunk; a fresh handle behaves as if it had not been called.  Out of range: SF_EINVAL, nothing changes.           */
int  sf_debug_sift_batch_chunk(sf_handle h, int32_t batch_chunk);
/* The host arithmetic of the SIFT batch forms for n_keyframes images of width x height, without a GPU or a handle (params
   NULL = the defaults).  With g, d the Gaussian and difference samples of sf_sift_plan, b the samples of the enlarged
   image and a(x) = x rounded up to a multiple of 256, an image needs a(a(a(2 g) + 2 d) + 4 b) bytes of planes (Gaussian,
   difference, the row pass's float32 plane), a(4 ceil(d / 32)) bytes of claim bits, 20 bytes per key (key, sorted key,
   list entry) and 32 bytes of counters.  *cap_img_out = 262144 keys; *chunk_out = the images per chunk, min(n_keyframes,
   65535, (2^31 - 1) / 262144, the 1 GB workspace / bytes per image), at least 1; *workspace_bytes_out = chunk x bytes
   per image.  Any output may be NULL.  SF_EINVAL: parameters out of range, n_keyframes outside 1 .. 65535; otherwise what
   sf_sift_plan refuses.                                                                                            */
int  sf_sift_batch_plan(int32_t width, int32_t height, const sf_sift_params* params, int32_t n_keyframes,
                        int32_t* cap_img_out, int32_t* chunk_out, int64_t* workspace_bytes_out);
/* Copies one int16 plane of the pyramid the most recent sf_detect_sift_device call on this handle built to d_out (dense,
   the octave's width x height; on the handle's stream): dog = 0, layer 0 .. n_octave_layers + 2: a Gaussian plane;
   dog = 1, layer 0 .. n_octave_layers + 1: a difference plane.  A failing keypoint comparison can be narrowed to the
   pyramid with it.  SF_EINVAL: no such call, or no such plane.                                                       */
int  sf_debug_sift_plane(sf_handle h, int32_t octave, int32_t layer, int32_t dog, int16_t* d_out);

/* The kNN-2 scan of the global matching of uint8 L2 rows (desc_type 2; k_match_u8.hip) for one pair of store slots,
   without the acceptance test: for every row t of the keyframe in slot_to, d_best[t] / d_second[t] = the smallest /
   second smallest squared L2 distance to the rows of slot_from (equal where the smallest occurs twice; 2^31 - 1 where
   there is no such row) and i_best[t] = the lowest row of slot_from at the smallest distance (-1: slot_from is empty).
   Host arrays of at least the "to" keyframe's rows; waits for the stream.  SF_EINVAL: another desc_type, a slot outside
   the store.                                                                                                          */
int  sf_debug_knn2_u8(sf_handle h, int32_t slot_from, int32_t slot_to, int32_t* d_best, int32_t* d_second, int32_t* i_best);

#ifdef __cplusplus
}
#endif

#endif /* SF_EXPERIMENTAL_H */
