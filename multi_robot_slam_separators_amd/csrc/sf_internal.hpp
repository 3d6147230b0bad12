// sf_internal.hpp -- host-side context and device views shared by the kernel translation units.
// Product code (gfx950 only). No CPU fallback exists anywhere in this library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/sepfinder.h"
#include "../../include/sf_experimental.h"

#define SF_BLOCK 256            // every verification kernel runs 256-thread workgroups (4 waves)
#define SF_MAX_KCAP 4096        // per-keyframe feature capacity ceiling of the GPU kernels
#define SF_STEP_MAX_DEPTH 16     // sf_step_issue: steps in flight at most (SF_OPT_STEP_DEPTH)
#define SF_CHAIN_NARROW_EST_DEFAULT true   // SF_OPT_CHAIN_NARROW_EST as a handle starts (docs/chain_narrow_estimates.md)
#define SF_STEP_MAX_LANES 4      // ... dealt over at most this many streams (SF_OPT_STEP_LANES)
#define SF_RECTIFY_TABLE_DEFAULT true      // SF_OPT_RECTIFY_TABLE as a handle starts: the measured choice (profiles/rectify_latency.json)

// ---- device-resident keyframe store (one arena per field, fixed per-slot stride) ---------------
// desc : [slots][kcap][W] uint32   W = 8 (<=256-bit descriptors) or 16 (<=512-bit), zero padded; float32 rows (desc_type 1)
//                                  W = 64 or 128, one dimension per dword; uint8 L2 rows (desc_type 2) W = 32, four per dword
// xyz  : [slots][kcap][3] float    wire layout of KeyPoint3DVec (base frame)
// kp   : [slots][kcap]    float4   {pt.x, pt.y, bit-cast sign-extended (octave & 255), 0}
// meta : [slots]          int4     {rows, n3d, nkp, cols}
struct StoreView {
  const uint32_t* desc;
  const float* xyz;
  const float4* kp;
  const int4* meta;
  int kcap;   // features per slot (multiple of 64)
  int w;      // dwords per descriptor
  int n_slots;  // valid slots (device-side guard for caller-provided slot indices)
};

// Outcome of one registration pass for one pair (RegistrationVis result + RegistrationInfo)
struct PassState {
  float T[12];      // row-major 3x4, p_from = T p_to ; all zero when null
  double var;       // covariance diagonal before the 1e-9 clamp: linear block (all six for 3D-3D)
  double var_ang;   // angular block (PnP estimator; equals var for 3D-3D)
  int32_t is_null;
  int32_t inliers;
  int32_t matches;
  int32_t pad;
};

// Header written by the matching kernels in front of each pair's correspondence list
struct CorrHeader {
  int32_t n_corr;        // id-aligned correspondences (ascending "from" index)
  int32_t words_from;    // words3From.size()
  int32_t words_to;      // words3To.size()
  int32_t words_to_2d;   // wordsTo.size()
};

// Accepted results streamed out of the fused kernel (device-resident block the kernel reads at the END of a pair):
// records / index / flags are host-pinned (device-accessible) arrays, counter a device word zeroed before the launch.
struct AcceptStream {
  sf_result* records;      // [cap] accepted results in the order they were produced
  int32_t* index;          // [cap] pair index of each record
  uint8_t* flags;          // [pairs] success of every pair (may be null)
  unsigned* counter;       // device
  sf_result* records2;     // [cap] optional second copy of every record (e.g. a collective's send buffer on the device)
  int32_t cap;
  int32_t ext_counter;     // the counter is the caller's (zeroed by the caller before each query)
};

struct DeviceParams {
  float nndr;
  int32_t min_inliers;
  int32_t iterations;
  int32_t refine_iterations;
  double refine_sigma;
  double inlier_thr;       // (double)inlier_distance
  int32_t adaptive_stop;
  int32_t max_sample_checks;
  uint64_t seed;
  int32_t guess_win;
  int32_t calibrated;
  double fx, fy, cx, cy;
  float wlim, hlim;        // image_width-1, image_height-1
  float L[12];             // local transform
  int32_t dbg_stop;        // diagnostics only: truncate k_ransac after phase N (0 = full kernel)
  int32_t grid_gx, grid_gy;   // guided matching: uniform grid over the image (cell >= window radius)
  float grid_inv_cell;
  int32_t estimation_type;    // 0 = 3D->3D, 1 = PnP
  float pnp_thr2f;            // (float)(pnp_reproj_error^2)
  float pnp_reproj_error;
  int32_t pnp_refine_iterations;
  int32_t bundle_adjustment;  // two-view BA after each pass's estimate (k_ba.hip)
  int32_t ba_iterations;
  float ba_robust_kernel_delta, ba_pixel_variance, stereo_baseline;
  int32_t force_3dof;         // Reg/Force3DoF
  int32_t bidirectional;      // Vis/ForwardEstOnly = false (stage pipeline only)
  int32_t guess_match_to_projection;   // Vis/CorGuessMatchToProjection: pass 2 by k_guided_tp (stage pipeline only)
  int32_t dbg_corr;           // fused kernel: also copy correspondence lists / headers / pass states to the global
                              // workspace (SF_OPT_DEBUG_CORR; sf_debug_correspondences)
  int32_t accept_on;          // chain kernels: accepted results also stream to the host as they are produced, into ...
  AcceptStream accept;        // ... this block (by value in the kernel arguments: nothing to upload, nothing to keep in step)
  unsigned long long* dbg_trace;   // SF_CHAIN_TRACE builds only (tools/chain_trace.py): [pair][SF_TRACE_SLOTS] timestamps; else null
};

// ---- a camera model per store slot (sf_camera_add; include/sepfinder.h) ---------------------------------------------------
// What DeviceParams derives from the sf_params camera, once per model of the handle's table: entry 0 is the sf_params
// camera itself, entry id the model sf_camera_add returned id for.  `tags` holds one id per store slot, beside the
// store's row counts.  The stage kernels' camera forms (k_guided_cam -- TP: k_guided_tp's --, k_pnp_cam, k_ba_pass_cam, ...) take
// the view and lay the block of the slot whose camera they read over their DeviceParams; a handle none of whose slots
// carries a non-zero id never launches them.
struct CameraBlock {
  double fx, fy, cx, cy;
  int32_t calibrated;
  float wlim, hlim;
  int32_t grid_gx, grid_gy;
  float grid_inv_cell;
  float stereo_baseline;
  int32_t pad;
  float L[12];
};
struct CameraView {
  const CameraBlock* table = nullptr;   // [SF_MAX_CAMERAS + 1]; nullptr: the call reads the sf_params camera only
  const uint8_t* tags = nullptr;        // [n_slots]
  int n_slots = 0;
};
#define SF_CAMERA_MAX_CELLS (48 * 48)   // every model's grid stays within it (sf_camera_derive): the guided passes' LDS bound

#ifdef __HIPCC__
// The block of the camera slot `slot` was taken with.  `slot` is uniform over the workgroup (a pair's "from" or "to"
// slot), so the id and the block sit in scalar registers; a slot outside the store reads the sf_params camera (the pair
// is void anyway: the bodies' own guards).
__device__ __forceinline__ const CameraBlock& sf_camera_of(const CameraView& cv, int slot) {
  int id = 0;
  if ((unsigned)slot < (unsigned)cv.n_slots) id = cv.tags[slot];
  id = __builtin_amdgcn_readfirstlane(id);
  return cv.table[id];
}
// DeviceParams with the camera fields replaced by the block's
__device__ __forceinline__ void sf_camera_apply(DeviceParams& P, const CameraBlock& b) {
  P.calibrated = b.calibrated;
  P.fx = b.fx; P.fy = b.fy; P.cx = b.cx; P.cy = b.cy;
  P.wlim = b.wlim; P.hlim = b.hlim;
  P.grid_gx = b.grid_gx; P.grid_gy = b.grid_gy; P.grid_inv_cell = b.grid_inv_cell;
  P.stereo_baseline = b.stereo_baseline;
#pragma unroll
  for (int i = 0; i < 12; ++i) P.L[i] = b.L[i];
}
#endif

// Phase timestamps of the fused kernel's chain (diagnostic build -DSF_CHAIN_TRACE, libsepfinder_trace.so; the product
// build compiles these to nothing): thread 0 of the pair's workgroup stores the 100 MHz wall clock.
#ifdef SF_CHAIN_TRACE
#define SF_TRACE_SLOTS 48
#define SF_TRACE_MARK(P, pair, slot)                                                              \
  do {                                                                                            \
    if (threadIdx.x == 0 && (P).dbg_trace) (P).dbg_trace[(size_t)(pair) * SF_TRACE_SLOTS + (slot)] = wall_clock64(); \
  } while (0)
// (the same with the pair's row pointer, for bodies that do not see the parameter block)
#define SF_TRACE_ROW_MARK(row, slot) do { if (threadIdx.x == 0 && (row)) (row)[slot] = wall_clock64(); } while (0)
#else
#define SF_TRACE_SLOTS 48
#define SF_TRACE_MARK(P, pair, slot) do { } while (0)
#define SF_TRACE_ROW_MARK(row, slot) do { } while (0)
#endif

// Where the fused verification kernel takes its pairs from when they are NN candidates still on the device
// (sf_find_matches_and_verify_device): candidate i = (local row, received column) -> pair (slot_other + column,
// slot_local + row); slots past *count, and candidates outside the databases / the store, are void pairs (-1, -1).
// cand == nullptr: the pair_from / pair_to arrays are used.
struct PairSource {
  const uint2* cand = nullptr;
  const unsigned* count = nullptr;
  int n_l = 0, n_r = 0, slot_other = 0, slot_local = 0, n_slots = 0;
};

// ---- owning types: a device block, a pinned host block, an event ------------------------------------------------------------
// Whoever holds one as a member owns the resource: move-only, freed by the destructor when non-null, no HIP call when null
// (a device-free context constructs and destructs without one).  Nothing lists them: sf_destroy drains the streams and
// selects the device, `delete c` frees.  Their allocate and free paths (sf_handle.hip) keep the process-wide counts of
// sf_debug_live_resources.
struct sf_context;
struct Buf;
struct Pinned;
struct Event;
int sf_buf_reserve(sf_context* c, Buf& b, size_t bytes, bool keep = false);   // grow-only: max(bytes, 1.5 x the old size)
void sf_buf_free(Buf& b);
// grow-only: a block smaller than `need` is replaced by one of `alloc` >= need bytes (the site's growth rule), contents lost
int sf_pinned_reserve(sf_context* c, Pinned& b, size_t need, size_t alloc);
void sf_pinned_free(Pinned& b);
int sf_event_ensure(sf_context* c, Event& ev);     // created on first use, timing disabled
void sf_event_free(Event& ev);

struct Buf {              // hipMalloc
  void* p = nullptr;
  size_t bytes = 0;
  Buf() = default;
  Buf(Buf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { sf_buf_free(*this); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { sf_buf_free(*this); }
};
struct Pinned {           // hipHostMalloc
  void* p = nullptr;
  size_t bytes = 0;
  Pinned() = default;
  Pinned(Pinned&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  Pinned& operator=(Pinned&& o) noexcept {
    if (this != &o) { sf_pinned_free(*this); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  Pinned(const Pinned&) = delete;
  Pinned& operator=(const Pinned&) = delete;
  ~Pinned() { sf_pinned_free(*this); }
};
struct Event {            // hipEventDisableTiming; reads as the hipEvent_t it holds (nullptr: not created yet)
  hipEvent_t e = nullptr;
  operator hipEvent_t() const { return e; }
  Event() = default;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) { sf_event_free(*this); e = o.e; o.e = nullptr; }
    return *this;
  }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { sf_event_free(*this); }
};
static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "Buf is move-only");
static_assert(!std::is_copy_constructible<Pinned>::value && !std::is_copy_assignable<Pinned>::value, "Pinned is move-only");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value, "Event is move-only");

// ---- rectification plans (sf_rectify_plan_create; include/sepfinder.h) ------------------------------------------------------
// What a computed plan's kernels read with uniform loads: iR = (P[:, :3] R)^-1, K's fx fy cx cy and the eight distortion
// terms (k4 k5 k6 zero under plumb_bob).  `table` is the fixed-point map {sx, sy} per output pixel: the upload of a plan of
// caller maps, built on first use (k_rectify_map) for a computed plan that runs the table form.
struct RectifyBlock {
  double iR[9];
  double fx, fy, cx, cy;
  double D[8];
};
struct RectifyPlan {
  sf_camera_info info;
  bool from_maps = false;
  int src_w = 0, src_h = 0, out_w = 0, out_h = 0;
  Buf table;
  bool table_ready = false;
};

struct Store {
  Buf desc, xyz, kp, meta;
  // (slots only grows, except in sf_store_clear and inside one call that takes back what it has just appended: the slots'
  //  camera ids are written out lazily, from cam_tags.size() up to `slots` -- camera_settle, sf_store.hip -- so a path that
  //  drops slots and returns must drop their ids with them, as sf_store_clear does)
  int kcap = 0, w = 0, slots = 0, cap_slots = 0;
};

struct NNDb {
  Buf rows;        // float32 [cap][dim]
  Buf norms;       // float32 [cap]
  Buf rows_h;      // fp16 [cap][dim] (nn_precision == 1)
  int n = 0, cap = 0;
  int ld = 0;      // row pitch (floats) `rows` was allocated and zero-padded for; a change re-allocates (nn_reserve)
  Buf norms_k;     // float32 [cap] squared norm of the first h_kprefix elements (filter stage)
  int h_n = -1, h_ld = 0, h_kprefix = 0;   // rows / pitch / prefix covered by the fp16 copy
  float h_scale = 1.f;      // power-of-two scale applied before the fp16 conversion
};

struct ProfSlot {
  int64_t launches = 0;
  double total_ms = 0.0;
};

// Everything one stream of verification / NN-stage work writes or owns: the handle's own (lane 0 of the step pipeline and
// the first half of a two-stream batch), step lanes 1..3 and the second half of a two-stream batch each have one.
struct Workspace {
  hipStream_t stream = nullptr;
  hipStream_t aux = nullptr;             // speculative device step: exact re-evaluation + minima + walk beside the verification
  Event ev_filter, ev_walk;
  Event ev_main;                         // "the handle's stream up to here": awaited when the databases changed

  // verification (sized for `ws_pairs` pairs)
  int ws_pairs = 0, ws_kcap = 0;
  Buf pair_from, pair_to;       // int32[n]
  Buf corr1, corr2;             // uint32[n][kcap]
  Buf hdr1, hdr2;               // CorrHeader[n]
  Buf pass1, pass2;             // PassState[n]
  Buf pass_back, dir_mask;      // Vis/ForwardEstOnly = false: the backward estimate's PassState[n], inlier masks [2][n][kcap]
  Buf list1, list3;             // int32[n] work lists (RANSAC pass 1, RANSAC pass 2)
  Buf counters;                 // int32[8]
  Buf results;                  // sf_result[n]
  Buf flags;                    // uint8[n] pass2_guided
  bool last_lists_valid = false;   // the last verification left correspondence lists in this workspace
  // the verification buffers, typed.  sel: work list 1 (the matching's survivors) or 3 (pass 2's); pass: 1 or 2
  int32_t* list(int sel) const { return (int32_t*)(sel == 1 ? list1 : list3).p; }
  int32_t* counter(int sel) const { return (int32_t*)counters.p + (sel == 1 ? 0 : 2); }
  uint32_t* corr(int pass) const { return (uint32_t*)(pass == 1 ? corr1 : corr2).p; }
  CorrHeader* hdr(int pass) const { return (CorrHeader*)(pass == 1 ? hdr1 : hdr2).p; }
  PassState* pass(int pass) const { return (PassState*)(pass == 1 ? pass1 : pass2).p; }
  uint8_t* guided_flags() const { return (uint8_t*)flags.p; }
  PassState* back() const { return (PassState*)pass_back.p; }
  uint8_t* masks() const { return (uint8_t*)dir_mask.p; }
  const int32_t* from() const { return (const int32_t*)pair_from.p; }
  const int32_t* to() const { return (const int32_t*)pair_to.p; }
  sf_result* out() const { return (sf_result*)results.p; }

  // NN stage and speculative verification
  Buf nn_cand;       // filter path: two 64-byte counter blocks (alternating per launch) + candidate (row, col) pairs + exact distances
  int nn_count_idx = 0;          // counter block of the next filter launch
  bool nn_count_primed = false;  // ... and whether the previous k128 launch already zeroed it
  Buf spec_from, spec_to, spec_results, spec_index;
  Buf compact_scratch;          // per-chunk counts of sf_compact_accepted_device
  unsigned compact_epoch = 0;   // k_compact_chain: tag of the current launch's prefix entries
  int compact_state_chunks = 0; // ... and how many state entries have been initialised
  void* compact_state_ptr = nullptr;
  Buf step_nn;                  // device walk: row minima (f64) | row arg (i32) | row candidate (i32) | packed arg (u64) | status
  Buf walk_scratch;             // device walk: tile keys / rows, sorted rows, column claims (sf_nn_walk_dev)

  uint64_t seen_db_epoch = ~0ull;   // sf_context::db_epoch this lane last waited for
  uint64_t seen_prep = 0;           // sf_context::prep_epoch this lane last waited for
};

// FREAK rows (types 3 and 5): the tables of k_freak_points -- the integral image is BRIEF's, the rows are 64 bytes
struct SfFreakTables {
  const float* pattern;        // [64][256][43] {x, y, sigma}: sf_freak_build_pattern's table
  const uint8_t* pairs;        // [64 bytes][8 bits] {i, j}: the pair behind every descriptor bit (sf_freak_bit_table)
  const int32_t* orient;       // [45] {i, j, weight_dx, weight_dy}
  const int32_t* sizes;        // [64]: the border every scale asks for
  float size_cst;              // (float)(64 / (LOG2 n_octaves))
  int fixed_idx;               // the scale index of every keypoint when scale_normalized is 0
  int orientation_normalized, scale_normalized;
};
constexpr int FREAK_SCALES = 64, FREAK_ORIENTATIONS = 256, FREAK_POINTS = 43, FREAK_PAIRS = 512, FREAK_ORIENT_PAIRS = 45,
              FREAK_ALL_PAIRS = 903, FREAK_BYTES = 64;
constexpr size_t FREAK_PATTERN_FLOATS = (size_t)FREAK_SCALES * FREAK_ORIENTATIONS * FREAK_POINTS * 3;
constexpr size_t FREAK_TABLE_PAIRS = 0, FREAK_TABLE_ORIENT = 1024, FREAK_TABLE_SIZES = 1792, FREAK_TABLE_BYTES = 2048;

// SURF rows (type 0): what k_surf_describe reads beside the integral image -- the two Gaussian tables of
// sf_surf_build_tables in one device buffer, and the two flags of sf_surf_params that shape the rows
struct SfSurfTables {
  const float* ori_w;          // [109] weights of the orientation samples
  const int8_t* ori_xy;        // [109] {x, y}
  const float* desc_w;         // [400] weights of the 20 x 20 gradient samples
  int upright, extended;
};
constexpr int SURF_ORI_SAMPLES = 109, SURF_PATCH = 20, SURF_MAX_OCTAVES = 8, SURF_MAX_LAYERS = 8;
constexpr unsigned SURF_MAX_CANDIDATES = 1u << 18;   // maxima per image; more is SF_ERANGE, never a truncated list
// The detector (sf_launch_detect_surf) runs over chunks of images whose det / trace planes and keys
// fit this much workspace: the size of the Infinity Cache, so that the planes k_surf_hessian writes are still on the die
// when k_surf_maxima and k_surf_emit read them, and two orders of magnitude more workgroups per launch than the chip
// has compute units.  One image always runs, whatever it needs.
constexpr size_t SURF_BATCH_WORKSPACE_BYTES = (size_t)256 << 20;
// What sf_surf_batch_plan_host computes for n images of one size: the bound on an image's maxima, its key capacity
// cap_img = min(candidate capacity, bound) (key_stride: at least one key), the images per chunk and their workspace
struct SfSurfBatchPlan {
  unsigned long long bound;
  unsigned cap_img, key_stride;
  int chunk;
  size_t plane_floats, per_image, workspace_bytes;
};
constexpr size_t SURF_TABLE_ORI_W = 0, SURF_TABLE_DESC_W = 512, SURF_TABLE_ORI_XY = 2112, SURF_TABLE_BYTES = 2368;

// The SIFT detector (k_sift.hip).  The pyramid of an image enlarged 2 x: octave o holds n_layers + 3 Gaussian planes of
// w[o] x h[o] int16 from gauss_off[o] on and n_layers + 2 difference planes from dog_off[o] on (offsets in samples);
// pos_off[o] = dog_off[o] as the 32-bit sample number the sort key carries (at most 2^26 samples: sf_sift_plan_host)
constexpr int SIFT_MAX_OCTAVES = 16, SIFT_MAX_LAYERS = 8, SIFT_MAX_KLEN = 520;   // sigma <= 8: the longest kernel has 515 taps
constexpr unsigned SIFT_MAX_CANDIDATES = 1u << 18;   // extrema, and keypoints, per image; more is SF_ERANGE
// SIFT rows (type 1): the handle's parameters, and whether the pyramid the detector has just left is this image's
// (batch: the pyramids of the launch's images are the batch detector's, c->sift_batch describes them)
struct SfSiftKind {
  sf_sift_params prm = {};
  bool reuse = false;
  bool batch = false;
  bool u8 = false;             // the rows as 128 uint8 (a handle with desc_type 2), not as 128 float32
};
struct SfSiftPlan {
  int n_octaves = 0, n_layers = 0;
  int w[SIFT_MAX_OCTAVES] = {}, h[SIFT_MAX_OCTAVES] = {};
  unsigned long long gauss_off[SIFT_MAX_OCTAVES] = {}, dog_off[SIFT_MAX_OCTAVES] = {};
  unsigned pos_off[SIFT_MAX_OCTAVES + 1] = {};
  unsigned long long gauss_samples = 0, dog_samples = 0;
};
// The batch form runs its whole chain -- pyramid, keypoints, refinement, stereo correspondence, rows -- over chunks of
// images whose planes and keys fit this much workspace.  One image always runs.  SURF's 256 MB (the Infinity Cache) gives
// chunks of 4 camera images here, and the chain is about 130 launches per chunk whatever its size: timed alternately in
// one run, 64 pairs of 752 x 480 took 0.745 ms per keyframe in chunks of 4 and 0.465 ms in chunks of 18, the 1 GB kept
// here.
constexpr size_t SIFT_BATCH_WORKSPACE_BYTES = (size_t)1 << 30;
// What sf_sift_batch_plan_host computes for n images of one size.  Image i of a chunk: its Gaussian planes at
// c->sift_planes + i plane_bytes, its difference planes off_dog bytes and the row pass's float32 plane off_tmp bytes
// behind them; behind the chunk's planes the claim bitmaps, claim_words apart; in c->sift_keys the chunk's keys, sorted
// keys and extrema lists, cap_img apart
struct SfSiftBatchPlan {
  SfSiftPlan P;
  unsigned cap_img = 0;
  int chunk = 0;
  size_t off_dog = 0, off_tmp = 0, plane_bytes = 0, claim_words = 0, per_image = 0, workspace_bytes = 0;
};

struct sf_context {
  sf_params params;
  DeviceParams dparams;
  int device = 0;
  hipStream_t stream = nullptr;   // the stream the launchers queue on: ws[0].stream, or another inside a UseWorkspace scope
  bool own_stream = false;
  int cu_count = 0;         // compute units of the device (grids sized to the chip); read through sf_cu_count (k_nn.hip), which fills it on first use
  // [0]: the handle's own; [1 .. SF_STEP_MAX_LANES - 1]: step lanes (SF_OPT_STEP_OVERLAP); [SF_STEP_MAX_LANES]: the second
  // half of a two-stream batch (sf_verify_device)
  Workspace ws[SF_STEP_MAX_LANES + 1];
  Workspace* w = ws;              // the workspace the launchers use
  std::string err;

  Store store;        // persistent keyframes
  Store scratch;      // staging slots for host-buffer calls
  // a camera model per store slot (sf_store.hip, "camera models").  cam_models[id - 1]: what sf_camera_add took; cam_blocks:
  // the derived blocks, [0] the sf_params camera (host copy of cam_table, uploaded by sf_camera_add).  cam_tags: the id of
  // every slot below cam_tags.size(); the slots behind it, up to store.slots, were appended since and carry cam_sel
  // (sf_camera_settle writes them out, before the selection changes and before anything reads a tag).  cam_nonzero: tags
  // != 0 among cam_tags.  cam_tags_dev: the device copy, cam_dev_n entries of it current (sf_camera_sync, ahead of a
  // verification).  cam_view: what the launchers of the sequence being queued hand their kernels (table nullptr: the
  // forms without cameras).
  std::vector<sf_camera_model> cam_models;
  std::vector<CameraBlock> cam_blocks;
  std::vector<uint8_t> cam_tags;
  int cam_sel = 0, cam_nonzero = 0, cam_dev_n = 0, cam_max_cells = 0;
  bool cam_mixed_calibration = false;     // some model of the table is valid for projection and another (or sf_params') is not
  Buf cam_table, cam_tags_dev;
  CameraView cam_view;
  Buf stage_desc, stage_xyz, stage_kp;   // H2D bounce buffers of the host-buffer ingest path
  // store slots as bytes (sf_store_export_* / sf_store_import_keyframes_device; k_store_wire.hip): header and table of the
  // most recent plan, and the four status words of the most recent export or import (sf_store_wire_status)
  Buf wire_plan, wire_status;
  // host-buffer batch ingest (store_add_host_batch): pinned staging, table scratch and the packing workers all
  // belong to the handle and end with it (sf_destroy)
  Pinned ingest_pinned;
  struct IngestPool* ingest_pool = nullptr;

  Buf ft_counts;                // batched feature extraction: corners per image (device)
  // feature extraction (k_extract.hip): integral image, per-corner scratch, the BRIEF test table
  Buf ex_integral, ex_desc, ex_xyz, ex_keep, ex_rows, brief_tests;
  // corner detection (k_gftt.hip): derivative-product / response planes, candidate keys (in + sorted), sort scratch,
  // the selection's cell lists, three scalars
  Buf gf_planes, gf_keys, gf_tmp, gf_lists, gf_scalar;
  Buf lk_pyr;                      // pyramid levels >= 1 of both images (k_lk.hip)
  Buf ft_images, ft_kpts, ft_flow, ft_wire;   // sf_get_features_and_descriptor: device copies of the pair, corners, LK outputs, response
  // camera images (k_image.hip): the uploaded rgb8 / bgr8 / mono8 pair of sf_get_features_and_descriptor_u8, the gray
  // planes of a batch (sf_add_keyframes_u8_batch_device: n left, then n right) and its NetVLAD rows; the colour-to-gray
  // coefficients (sf_image_set_gray_rule: 0 = OpenCV 3.x, 1 = OpenCV 4.x)
  Buf img_src, img_gray, img_desc;
  int gray_rule = 0;
  // raw camera images (sf_rectify.hip, k_rectify.hip): rect_plans[id - 1], the device blocks of all of them
  // ([SF_MAX_RECTIFY_PLANS] RectifyBlock, reserved once) and the form computed plans run in (SF_OPT_RECTIFY_TABLE)
  std::vector<RectifyPlan> rect_plans;
  Buf rect_blocks;
  bool rect_table = SF_RECTIFY_TABLE_DEFAULT;
  struct sf_netvlad_model* netvlad = nullptr;   // NetVLAD inference (k_cnn.hip): weights + activation buffers
  int brief_bytes = 0;                 // 0: table not uploaded yet
  int8_t brief_host[64 * 8 * 4] = {};
  // Vis/FeatureType of the extraction (sf_set_feature_type; 2 by sf_set_feature_type_orb): 6 = GFTT/BRIEF, 4 = FAST/BRIEF, 8 = GFTT/ORB with `orb` and the ORB test
  // table (orb_host, uploaded to orb_tests; orb_loaded false: the default set, not generated yet); ex_blur / ex_kpts:
  // the blurred level-0 images and the keypoints with their ORB angles
  int feature_type = 6;
  sf_orb_params orb = {19, 31, 2, 0};
  bool orb_loaded = false;
  int8_t orb_host[32 * 8 * 4] = {};
  Buf orb_tests, ex_blur, ex_kpts;
  // 2 = ORB: the detector is k_orb_detect.hip's (FAST per pyramid level, Harris or FAST score, per-level quotas) with these
  // parameters and `orb`; the descriptors are type 8's on the keypoint's own level.  orb_pyr: pyramid levels >= 1 of
  // the image at hand; orb_work: the detector's candidate lists
  sf_orb_detector_params orb_det = {2.0f, 3, 0, 0, 20};
  Buf orb_pyr, orb_work;
  // 4 = FAST/BRIEF: the detector is k_fast.hip's with these parameters (sf_fast_set_params), the rest is type 6's
  sf_fast_params fast = {20, 1};
  // 5, 6, 8 and sf_detect_corners_device: the GFTT response of k_gftt.hip -- block size, Harris or minimum eigenvalue, k
  // (sf_gftt_set_params); the defaults run the kernels the detector had before the block existed
  sf_gftt_params gftt = {3, 0, 0.04};
  // 3 = FAST/FREAK, 5 = GFTT/FREAK (sf_set_feature_type_freak; k_freak.hip): type 4's / type 6's corners with 64-byte FREAK
  // rows.  freak_pairs: the 512 selected pairs in OpenCV's selectedPairs format (freak_pairs_set false: the generated
  // default selection, not made yet).  On the device, reserved by the first extraction under a FREAK type only:
  // freak_pattern [64 scales][256 orientations][43 points] {x, y, sigma} and freak_tables (FREAK_TABLE_BYTES: the pairs of
  // every descriptor byte, the 45 orientation pairs with their weights, the 64 pattern sizes); freak_pattern_ok /
  // freak_tables_ok false: what is there was built for other parameters / pairs
  sf_freak_params freak = {1, 1, 22.0f, 4};
  bool freak_pairs_set = false, freak_pattern_ok = false, freak_tables_ok = false;
  int32_t freak_pairs[512] = {};
  Buf freak_pattern, freak_tables;
  alignas(16) uint8_t freak_tables_host[FREAK_TABLE_BYTES] = {};   // the host copy of freak_tables
  SfFreakTables freak_dev = {};                // the kernel's view of the two buffers and the parameters
  // 0 = SURF (sf_set_feature_type_surf; k_surf.hip), on a handle with desc_type 1 only: float32 rows of 64 or 128
  // dimensions.  surf_planes: the det and trace planes of every layer; surf_keys: the maxima's sort keys, unsorted then
  // sorted, and the counter; surf_tables: the Gaussian tables (uploaded once, they depend on no parameter)
  sf_surf_params surf = {500.0f, 4, 2, 0, 0};
  bool surf_tables_ok = false;
  Buf surf_planes, surf_keys, surf_tables;
  // the batch form: surf_ctl holds the number of keyframes of the most recent batch call whose maxima exceeded the key
  // capacity (word 0) and, from byte 64 on, every image's count, segment bounds and rekey flag.  surf_debug_cap /
  // surf_debug_chunk (sf_debug_surf_limits; 0 = the defaults): the candidate capacity and the images per chunk
  Buf surf_ctl;
  int surf_debug_cap = 0, surf_debug_chunk = 0;
  SfSurfTables surf_dev = {};
  // the SIFT detector (sf_detect_sift_device; k_sift.hip).  sift_planes: the int16 Gaussian and difference planes of every
  // octave, the row pass's float32 plane and the bitmap of claimed samples; sift_keys: sort keys, sorted keys, the list of
  // extrema and two counters; sift_tables: the blur kernels of the parameter set last used (sift_klen their lengths).
  // sift_last: the layout of the most recent call's pyramid (sf_debug_sift_plane); sift_debug_cap: sf_debug_sift_limits
  sf_sift_params sift = {0, 3, 0.04f, 10.0f, 1.6f};
  Buf sift_planes, sift_keys, sift_tables;
  bool sift_tables_ok = false, sift_last_ok = false;
  int sift_tables_n = 0, sift_debug_cap = 0;
  float sift_tables_sigma = 0.0f;
  int32_t sift_klen[SIFT_MAX_LAYERS + 3] = {};
  std::vector<float> sift_coef_host;
  SfSiftPlan sift_last;
  size_t sift_last_off_dog = 0, sift_last_off_claim = 0;
  sf_sift_params sift_last_prm = {};
  int sift_last_width = 0, sift_last_height = 0;
  // the batch form: sift_ctl holds the number of keyframes of the most recent batch call with more extrema or keypoints
  // than an image holds (word 0) and, from byte 64 on, the chunk's per-image words -- both counters, segment bounds,
  // rekey flag; sift_batch: the plan of that call (the extraction reads the chunk's pyramids by it); sift_debug_chunk
  // (sf_debug_sift_batch_chunk; 0 = the default): the images per chunk
  Buf sift_ctl;
  SfSiftBatchPlan sift_batch;
  int sift_debug_chunk = 0;
  // every type: what Feature2D::generateKeypoints puts around the detector (sf_front_set_params; k_subpix.hip) -- the ROI
  // the detector sees and cv::cornerSubPix on the kept corners; both off on a fresh handle
  sf_front_params front = {{0.f, 0.f, 0.f, 0.f}, 3, 0, 0.02f};
  // which stereo correspondence the extraction calls run (sf_stereo_set_params): pyramidal LK (k_lk.hip) or block
  // matching (k_stereo_bm.hip) with SSD or SAD scores
  sf_stereo_params stereo = {1, 1};
  // the depth keyframe calls (sf_depth_set_params; k_depth.hip): Vis/DepthAsMask, the detector mask made of the depth image.
  // dp_depth / dp_mask: the device copy of the host call's depth image, the mask planes of a call (the images' pitch and stride)
  // depth_size: the depth images' own size (sf_depth_set_size), {0, 0} = the image's
  sf_depth_params depth = {1};
  sf_depth_size depth_size = {0, 0};
  Buf dp_depth, dp_mask;
  // depth registration (sf_depth_register.hip, k_depth_register.hip): the z-buffer, one uint32 key per output pixel of a
  // chunk's images.  dreg_debug_chunk / dreg_debug_stages (sf_debug_depth_register_limits; 0 = the defaults): the images per
  // chunk, and which of memset (1), scatter (2) and resolve (4) a call queues
  Buf dreg_keys;
  int dreg_debug_chunk = 0, dreg_debug_stages = 0;
  // Vis/GridRows x Vis/GridCols (sf_grid_set_params; k_grid.hip): the detector of types 4, 6 and 8 runs per cell of the
  // ROI; 1 x 1 = no cells.  ft_cells: every cell's count, then every cell's keypoints, before k_grid_gather joins them
  sf_grid_params grid = {1, 1};
  Buf ft_cells;
  Buf trace;                    // SF_CHAIN_TRACE builds: uint64[n][32] phase timestamps of the fused kernel

  // NN stage
  NNDb nn_local, nn_recv;
  int nn_dim = 0;
  std::vector<uint8_t> mask_local, mask_other;         // host mirrors
  std::vector<int32_t> ignored;                        // pairs (local, other)
  Buf d_mask_local, d_mask_other, d_ign_ptr, d_ign_col;
  bool masks_dirty = true;
  Buf nn_rowmin;     // per-row packed (dist bits, idx) uint64 [n_local]
  Buf nn_exact;      // double [n_local]
  Buf nn_scalar;     // small reduction scratch
  int nn_level = 0, nn_level_cooldown = 32, nn_last_kdims = 0;   // adaptive prefix ladder of the filter
  bool nn_force_full = false;   // SF_OPT_NN_FULL_FILTER: always contract the full descriptor length
  int nn_coef_level = -1, nn_coef_nl = 0, nn_coef_nr = 0;         // what the cached filter coefficients were built for
  double nn_coef_thr = 0.0;
  float nn_coef_scale = 0.f;
  const void* nn_coef_ptr = nullptr;
  std::vector<double> last_row_min;
  std::vector<int32_t> last_row_arg;
  std::vector<int32_t> last_row_cand;   // candidate-list index of each row's minimum (filter path)
  std::vector<uint64_t> nn_sort_keys, nn_sort_keys2;   // host scratch of the walk (kept to avoid reallocation)
  std::vector<int32_t> nn_sort_rows, nn_sort_rows2;
  std::vector<uint32_t> nn_sort_hist;
  std::vector<uint8_t> nn_taken;
  // per-tick NetVLAD append from host float64 rows (sf_nn_append): grow-only pinned + device staging, re-used once
  // the previous append's copy has left it (nn_stage_done), so the path neither allocates nor synchronises
  Pinned nn_stage_pinned;
  Buf nn_stage_dev;
  Event nn_stage_done;
  bool nn_stage_busy = false;
  Pinned nn_pinned;            // pinned host staging of the NN filter's small D2H copies

  int match_variant = 0;   // 0 = default geometry; see sf_launch_match_global
  std::vector<const void*> dyn_lds_kernels;   // kernels whose dynamic LDS limit this handle has raised (sf_dyn_lds)
  bool debug_corr = false;      // SF_OPT_DEBUG_CORR: the fused kernel also writes lists / headers / states to HBM
  bool fused = true;        // fused per-pair verification kernel (SF_FUSED=0 selects the stage kernels)
  bool split = false;       // SF_FUSED=2: one matching launch + one chain launch over the survivors (k_verify.hip)
  bool split_auto = true;   // SF_OPT_STEP_SPLIT: the split form inside overlapped steps (sf_use_split, sf_verify_host.hip); on again since
                            // round 5 (its matcher is software-pipelined: 23.0 against 22.7 M pairs/s, profiles/r05u_*)
  int split_auto_min = 2048;   // ... for queries of at least this many candidates (SF_STEP_SPLIT_MIN): below, one launch wins
  bool in_overlapped_step = false;   // set around sf_step_issue's body while the steps alternate between two streams
  int chain_nw = 4;                // wavefronts per motion-estimation chain of the split forms: 1, 2 (round 5), or 4 = the
                                   // 256-thread workgroup of rounds 2-4 (SF_CHAIN_NW)
  bool chain_narrow_est = SF_CHAIN_NARROW_EST_DEFAULT;   // SF_OPT_CHAIN_NARROW_EST: the 3D-3D split form's estimates on one wavefront
                                   // each, around the wide kernel's guided matching (k_chain_est, k_verify.hip)
  int chain_pnp_nw = 2;            // wavefronts per PnP chain (SF_CHAIN_PNP_NW; 2 measured fastest: profiles/r05i_pnp_chain_width.txt)
  int ba_occ = 0;                  // wavefronts per SIMD the SMALL adjustment kernel is compiled for (SF_BA_OCC; 1 = 512 registers,
                                   // no scratch; 2 = 256 registers + 256 B of scratch; 0 = by estimator: PnP 1, 3D-3D 2 -- measured,
                                   // profiles/r05e_ba_occupancy.txt)
  int ba_nw = 1;                   // wavefronts per bundle adjustment (k_ba_pass; SF_BA_NW): 1 measured fastest (profiles/r05c_ba_width.txt)
  bool chain_pnp = true;           // PnP estimator: k_match_split + k_chain_pnp instead of the five stage launches
                                   // (SF_CHAIN_PNP=0: the stage launches)
  bool match_mfma = true;   // Hamming table on the fp4 matrix cores (SF_MATCH_MFMA=0 selects the VALU matcher)

  // sf_verify_matches_device / sf_compact_accepted_device staging
  Pinned pairs_pinned;
  Event pairs_staged;
  Pinned count_pinned;          // 64 bytes: the count of sf_compact_accepted_device

  // multi-GPU exchange (sf_comm.hip)
  void* comm = nullptr;    // ncclComm_t
  int comm_rank = 0, comm_world = 1;
  int32_t comm_count_host = 0;
  Buf comm_scratch;

  // Two-stream verification of large batches (sf_verify_host.hip, sf_verify_device): the second half of a batch runs
  // its stage kernels on ws[SF_STEP_MAX_LANES] -- a stream, workspace and counters of its own -- so that the
  // latency-bound motion-estimation kernels of one half overlap the issue-bound matching kernel of the other.
  // Off unless SF_OVERLAP=1 (+3-6 %).
  Event ev_fork, ev_join;
  bool overlap = false;
  int overlap_min_pairs = 4096;
  int ws_split = 0;             // pairs [0, ws_split) of the last batch live in ws[0], the rest in ws[SF_STEP_MAX_LANES]

  // Speculative verification (sf_find_matches_and_verify_device): every candidate (row, column) the NN filter
  // emits is verified on the device while the host still reduces the candidates to row minima, sorts and
  // walks them; the walk's matches then pick their results out of the speculative ones.
  // results of the last sf_find_matches_and_verify_device: record of match i = last_results[index ? index[i] : i]
  const sf_result* last_results = nullptr;
  const int32_t* last_results_index = nullptr;
  int last_results_n = 0;
  PairSource pair_src;          // candidate list the fused kernel derives its pairs from (speculative path), or empty
  struct Spec {
    bool requested = false;     // set by the entry point for the duration of one sf_nn_run
    bool launched = false;      // the candidates of some filter level were handed to the verification
    bool valid = false;         // ... and that level's candidate set was accepted (n_cand <= grid)
    int32_t slot_other = 0, slot_local = 0;
    unsigned grid = 0;          // speculative pair slots (candidates beyond it invalidate the speculation)
    hipStream_t copy_stream = nullptr;
    Event ev_refined, ev_copied;
  } spec;
  Pinned spec_index_pinned;     // the matches' candidate slots (sf_find_matches_and_verify_device), read by the gather ...
  Event spec_index_staged;      // ... recorded behind it: the block may be rewritten after this
  // accepted-result streams (sf_accept_stream_set / _select): two registered blocks, the one selected for the next
  // speculative query is handed to the fused kernel; `streamed` says whether the last query used it
  struct AcceptHost { AcceptStream s = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0}; bool set = false; } accept_blocks[3];   // [2]: the step pair's own
  int accept_sel = -1;
  bool accept_streamed = false;     // the last query's results are in the selected block (keyed by verified slot)
  bool accept_armed = false;        // the selected block was handed to a verification launch of the last query (it may
                                    // hold records even when the query then fell back: streamed = false)
  // sf_step_issue / sf_step_retire: the caller's loop body (find_separators.py:59-133) as a begin / retire pair.  A ring
  // of `step_depth + 1` blocks: up to `step_depth` steps in flight, and the block of the step retired last stays
  // untouched until the next retire.
  struct StepBlock {
    Pinned pinned;                     // ONE host-pinned allocation: records | index | flags | count | matches | walk words
    sf_result* records = nullptr;      // [cap] accepted results (streamed: completion order; compacted: match order)
    int32_t* index = nullptr;          // [cap] streamed: verified slot of each record, -1 = unused entry
    uint8_t* flags = nullptr;          // [cap] compacted: success of every match
    int32_t* count = nullptr;          // compacted: number of accepted matches
    sf_match* walk_matches = nullptr;  // [cap] device walk: the matches, written by k_walk_emit
    int32_t* walk_slots = nullptr;     // [cap] speculative device step: the verification slot (= candidate index) of each match
    int32_t* walk_n = nullptr;         // device walk: their number ...
    int32_t* walk_status = nullptr;    // ... and the NN stage's status (0, or 1 = candidate set denser than the filter level allows)
    int32_t cap = 0;
    Buf dev;                           // device: 64-byte counter block {matches, -, -, -, accept slot counter} + (row, column)[cap]
    Buf dev_records;                   // device: [cap] the accepted records once more, same slots as `records` (sf_step_result.d_records)
    std::vector<sf_match> matches;     // host walk: the matches
    std::vector<int32_t> slot_of_match, record_of_match, rec_of_slot;
    int32_t n = 0, pairs = 0;
    bool streamed = false, armed = false, issued = false;
    bool speculative = false;          // device walk, speculative form: record of match i = the record of slot walk_slots[i]
    bool device_walk = false;          // the NN walk ran on the device: matches / n come from the pinned block at retire
    bool settled = false;              // its `done` event has been waited for (and a fallback, if needed, has run)
    int32_t slot_other = 0, slot_local = 0, parity = 0;   // (what a fallback needs to run the query again)
    int settle_rc = 0;
    Event done;
    // a caller's copy out of dev_records (sf_memcpy_device_async, on ANY stream) is recorded here; the step that next
    // uses the block waits for it before its kernels may write the buffer again
    Event copied;
    bool copy_pending = false;
  } step_blocks[SF_STEP_MAX_DEPTH + 1];
  int step_depth = 6;                      // SF_OPT_STEP_DEPTH: steps in flight
  int step_lanes = 3;                      // SF_OPT_STEP_LANES: streams the steps in flight are dealt over (step k on lane k mod lanes)
  bool step_device_walk = true;            // SF_OPT_STEP_DEVICE_WALK: no host wait inside sf_step_issue
  uint64_t step_seq = 0;                   // steps issued so far (the next step's number)
  int step_inflight = 0;
  // Where the pipeline's streams sit on the hardware (sf_placement.hip: place_streams).  Measured once, at the first step that
  // needs a second stream: a launch that does not fit on the chip keeps the dispatcher of its queue's PIPE busy until
  // its last workgroup is placed, and every other queue of that pipe waits -- so the lanes' main streams are picked
  // from candidates on different pipes and the second streams (short chains of small launches) from a pipe none of
  // them uses.  Streams are handed out once; what is left over is destroyed with the handle.
  struct StreamPlacement {
    bool tried = false, done = false;
    hipStream_t main[SF_STEP_MAX_LANES] = {};   // [0] unused: lane 0 runs on the handle's stream
    hipStream_t aux[SF_STEP_MAX_LANES] = {};
    hipStream_t copy = nullptr;                  // the second stream of the synchronous speculative call
    char report[384] = {0};
  } placement;
  bool step_speculate = true;              // SF_OPT_STEP_SPECULATE: batch-mode steps verify every filter candidate beside the walk
  // Work that prepares state ALL lanes read (fp16 copies of the databases, filter coefficients, masks) is queued by
  // whichever lane first needs it; it bumps prep_count, the issuing step records ev_prep behind it and the other lanes
  // wait for that event once (Workspace::seen_prep).
  uint64_t prep_count = 0, prep_epoch = 0;
  Event ev_prep;
  // SF_OPT_STEP_OVERLAP: the steps in flight run on `step_lanes` streams -- lane k on ws[k], with its own stream and its
  // own copy of every device buffer a step writes -- so that the tail of one step's verification (its last
  // motion-estimation chains on an emptying chip) and the NN stage of the next overlap.
  bool step_overlap = true;                // the option (SF_STEP_OVERLAP=0 / sf_set_option turn it off)
  uint64_t db_epoch = 0;                   // bumped by every call that writes a database through the handle's stream
  sf_result* step_mirror_records[2] = {nullptr, nullptr};   // sf_step_mirror[_pair]: second (device) destination of every
  uint32_t* step_mirror_counter[2] = {nullptr, nullptr};    // accepted record and the caller's slot counter, per step parity
  int32_t step_mirror_cap = 0;
  bool step_mirror_lanes = false;             // sf_step_mirror_streams: the odd steps of a mirror pair run on lane 1

  // profiling
  bool prof = false;
  uint32_t prof_mask = 0xFFFFFFFFu;      // bit k: kernel k is bracketed when profiling is on (sf_prof_select)
  std::vector<hipEvent_t> prof_event_pool;   // timing events are reused, not created per launch
  ProfSlot prof_slots[SF_K_COUNT];
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending_events;
};

// Points the launchers at workspace `ws` and queues them on `stream` (by default the workspace's own) until the scope
// ends; a stream-only scope names the workspace already in use and another of its streams.
struct UseWorkspace {
  sf_context* c;
  Workspace* w;          // what the scope restores
  hipStream_t stream;
  UseWorkspace(sf_context* c_, Workspace& ws, hipStream_t s) : c(c_), w(c_->w), stream(c_->stream) { c->w = &ws; c->stream = s; }
  UseWorkspace(sf_context* c_, Workspace& ws) : UseWorkspace(c_, ws, ws.stream) {}
  ~UseWorkspace() { c->w = w; c->stream = stream; }
  UseWorkspace(const UseWorkspace&) = delete;
  UseWorkspace& operator=(const UseWorkspace&) = delete;
};

// ---- helpers implemented in sf_handle.hip, sf_store.hip, sf_step.hip (the host files share more: sf_host.hpp) ----
int sf_fail(sf_context* c, int code, const char* fmt, ...);
// a database is about to change (SF_OPT_STEP_OVERLAP): `drain` also waits for the step in flight on the second stream
int sf_lanes_touch(sf_context* c, bool drain);
struct sf_netvlad_model;
void sf_netvlad_free(sf_context* c);
int sf_netvlad_load_impl(sf_context* c, const sf_netvlad_weights* w);
int sf_netvlad_infer_impl(sf_context* c, const float* d_image, int H, int W, float* d_out, int n_out);
int sf_netvlad_infer_batch_impl(sf_context* c, const float* d_images, int n_img, int H, int W, float* d_out, int n_out);
// the same from 8-bit camera images (format: sf_image_format; rows of `pitch` bytes, images `stride` bytes apart);
// sf_netvlad_check: the argument checks of both, without a launch
int sf_netvlad_infer_u8_batch_impl(sf_context* c, const uint8_t* d_images, int format, int n_img, int H, int W, int pitch,
                                   size_t stride, float* d_out, int n_out);
int sf_netvlad_check(sf_context* c, int n_img, int H, int W, int n_out);
int sf_netvlad_pca_dim(const sf_context* c);   // 0: no model loaded
// k_image.hip
bool sf_gray_rule(int rule, int* kr, int* kg, int* kb, int* shift);
int sf_launch_image_gray(sf_context* c, const uint8_t* d_src0, const uint8_t* d_src1, int n_first, int format, int rule,
                         int width, int height, int src_pitch, size_t src_stride, int n_images, uint8_t* d_dst, int dst_pitch,
                         size_t dst_stride);
// k_rectify.hip: the two launches of the rectification calls, asynchronous on the context's stream; the caller
// (sf_rectify.hip) has validated everything.  sf_launch_rectify_maps writes a computed plan's float32 maps (d_mapx, rows of
// pitch_bytes) or, with d_table, its fixed-point table [out_h][out_w] {sx, sy}.  sf_launch_rectify: n_a images under block /
// table a, n_b under b; tab_a / tab_b nullptr = the computed form (both or neither).
struct RectifyImages {
  const uint8_t* src_a; const uint8_t* src_b;
  uint8_t* dst_a; uint8_t* dst_b;
  int n_a, n_b;
  int src_w, src_h, out_w, out_h;
  int src_pitch, dst_pitch;
  size_t src_stride, dst_stride;
};
int sf_launch_rectify_maps(sf_context* c, const RectifyBlock* d_block, int out_w, int out_h, float* d_mapx, float* d_mapy,
                           int pitch_bytes, int32_t* d_table);
int sf_launch_rectify(sf_context* c, const RectifyImages& im, int format, int out_format, int rule, const RectifyBlock* blk_a,
                      const RectifyBlock* blk_b, const int32_t* tab_a, const int32_t* tab_b);
// k_nn.hip: room for n more rows of `dim` values in a database, without appending (SF_EINVAL: another dimension)
int sf_nn_reserve_rows(sf_context* c, NNDb& db, int n, int dim);
StoreView sf_store_view(const Store& s);
// camera models (sf_store.hip): whether a slot of the store carries a non-zero id (what sends a verification of the store
// to the stage kernels' camera forms), and the device copy of the ids brought up to date -- a synchronous upload through
// the handle's own stream, needed only after slots were appended or re-tagged
bool sf_camera_active(const sf_context* c);
int sf_camera_sync(sf_context* c);
void sf_prof_begin(sf_context* c, int kernel);
void sf_prof_end(sf_context* c, int kernel);

// gate selector of the matching kernels: 0 = 3D->3D, 1 = PnP, 2 = PnP without a calibrated camera, 3 = PnP with
// Vis/ForwardEstOnly = false (either direction's gate sends the pair on; each estimate then checks its own)
// With a camera id per slot (cam_view set: the stage sequence of a store with cameras) the gate is the pair's: the matcher
// runs the PnP gate if ANY model of the table is valid, and the pairs whose camera B is not are closed behind it --
// forward only by k_camera_gate, with both directions by each direction's estimate (k_pnp_cam) and their merge.
inline int sf_est_mode(const sf_context* c) {
  if (c->dparams.estimation_type != 1) return 0;
  bool calibrated = c->dparams.calibrated != 0;
  if (c->cam_view.table)
    for (const CameraBlock& b : c->cam_blocks) calibrated = calibrated || b.calibrated != 0;
  return calibrated ? (c->dparams.bidirectional ? 3 : 1) : 2;
}

// The argument list of the pass-1 stage kernels (k_match.hip, k_match_u8.hip):
// kern(st, pair_from, pair_to, nndr, min_inliers, est, extra..., corr, hdr, pass, list, counter), one workgroup of `nt`
// threads with `lds` bytes per pair, on the context's stream into its first-pass workspace.
template <class Kern, class... Extra>
void sf_launch_pass1(sf_context* c, Kern kern, int nt, size_t lds, StoreView st, const int32_t* d_from, const int32_t* d_to,
                     int n, Extra... extra) {
  const Workspace& w = *c->w;
  hipLaunchKernelGGL(kern, dim3(n), dim3(nt), lds, c->stream, st, d_from, d_to, c->dparams.nndr, c->dparams.min_inliers,
                     sf_est_mode(c), extra..., w.corr(1), w.hdr(1), w.pass(1), w.list(1), w.counter(1));
}

// One pass's buffers out of the current workspace, as the estimators, the adjustment and the merges take them: the work
// list `list_sel` (Workspace::list) with its counter, the pass's lists, headers and states, the guided matcher's flags
// (pass 2 only: pass 1 always matches globally), Reg/Force3DoF's applications behind the pass (myRegistration.cpp:269-276,
// and for pass 1 the one its result meets as the guess of pass 2, :245-248) and the estimate's profiling slot.
struct PassBufs {
  const int32_t* list;
  const int32_t* counter;
  uint32_t* corr;
  CorrHeader* hdr;
  PassState* ps;
  const uint8_t* guided_flag;
  int end_3dof;
  int prof;
};
inline PassBufs sf_pass_bufs(const sf_context* c, int pass, int list_sel) {
  const Workspace& w = *c->w;
  return {w.list(list_sel), w.counter(list_sel), w.corr(pass), w.hdr(pass), w.pass(pass),
          pass == 2 ? w.guided_flags() : nullptr, c->dparams.force_3dof ? (pass == 1 ? 2 : 1) : 0,
          pass == 1 ? SF_K_RANSAC1 : SF_K_RANSAC2};
}

// ---- run-time value -> template argument: f gets the value as a std::integral_constant ---------------------------------
template <int V> using sf_int = std::integral_constant<int, V>;
// dwords per binary descriptor row of the matching / chain kernels
template <class F> int sf_with_w(int w, F&& f) { return w == 8 ? f(sf_int<8>{}) : f(sf_int<16>{}); }
// wavefronts per chain / adjustment (SF_CHAIN_NW, SF_CHAIN_PNP_NW, SF_BA_NW)
template <class F> int sf_with_nw(int nw, F&& f) { return nw == 1 ? f(sf_int<1>{}) : nw == 2 ? f(sf_int<2>{}) : f(sf_int<4>{}); }
template <class F> int sf_with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// the guided matchers' rows <W, L2, U8>: uint8 L2 rows (desc_type 2) of 32 dwords, float32 rows (1) of 64 / 128, binary rows of 8 / 16
template <class F> int sf_with_desc(int desc_type, int w, F&& f) {
  if (desc_type == 2) return f(sf_int<32>{}, std::true_type{}, std::true_type{});
  if (desc_type == 1) return w == 64 ? f(sf_int<64>{}, std::true_type{}, std::false_type{}) : f(sf_int<128>{}, std::true_type{}, std::false_type{});
  return w == 8 ? f(sf_int<8>{}, std::false_type{}, std::false_type{}) : f(sf_int<16>{}, std::false_type{}, std::false_type{});
}

// Gate of one direction of the PnP estimate (myRegistrationVis.cpp:1059, :1070-1071 with A / B as :936-977 set them):
// dir 0: 3D words of "from" and 2D words of "to"; dir 1: 3D words of "to" and 2D words of "from" -- every "from" row
// after global matching (:856-875), the rows with a finite point after guided matching (:766-774).
__host__ __device__ inline bool sf_pnp_dir_gate(int dir, const CorrHeader& h, int rows_from, bool guided, int min_inliers) {
  if (h.words_to_2d <= 0) return false;                                   // :928
  if (dir == 0) return h.words_from >= min_inliers && h.words_to_2d >= min_inliers;
  return h.words_to >= min_inliers && (guided ? h.words_from : rows_from) >= min_inliers;
}

// ---- ORB pyramid (Vis/FeatureType 2): the level table the kernels take BY VALUE ---------------------------------
// Level 0 is the caller's image (its own pitch); level l >= 1 lives at pyr + off[l] with pitch w[l].  The blurred
// copies of the extraction use the same offsets (off[0] = 0, level 0 included).
#define SF_ORB_MAX_LEVELS 8
struct SfOrbPyr {
  int n;
  int w[SF_ORB_MAX_LEVELS], h[SF_ORB_MAX_LEVELS];
  unsigned off[SF_ORB_MAX_LEVELS];
  float scale[SF_ORB_MAX_LEVELS], inv_scale[SF_ORB_MAX_LEVELS];   // scale_l = (float)pow((double)scale_factor, l); 1.f / scale_l
  unsigned total;                                                  // bytes of all levels, level 0 included
};
struct SfOrbLevel { int w, h; unsigned off; float scale, inv_scale; };
// (masks OR-ed together, not an index and not a chain of selects: the compiler turns both into a copy of the kernel
//  argument in scratch, indexed at run time.  A level past the table gives an empty level.)
__device__ __forceinline__ SfOrbLevel sf_orb_level(const SfOrbPyr& P, int l) {
  int w = 0, h = 0, sc = 0, inv = 0;
  unsigned off = 0u;
#pragma unroll
  for (int i = 0; i < SF_ORB_MAX_LEVELS; ++i) {
    const int m = -(int)(l == i);
    w |= m & P.w[i];
    h |= m & P.h[i];
    off |= (unsigned)m & P.off[i];
    sc |= m & __float_as_int(P.scale[i]);
    inv |= m & __float_as_int(P.inv_scale[i]);
  }
  return {w, h, off, __int_as_float(sc), __int_as_float(inv)};
}
inline SfOrbPyr sf_orb_single_level(int w, int h) {
  SfOrbPyr P = {};
  P.n = 1; P.w[0] = w; P.h[0] = h; P.scale[0] = 1.f; P.inv_scale[0] = 1.f; P.total = (unsigned)((size_t)w * h);
  return P;
}

#define SF_HIP(c, expr)                                                                      \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) return sf_fail((c), SF_EHIP, "%s -> %s", #expr, hipGetErrorString(_e)); \
  } while (0)

// Dynamic LDS above the 64 KB every kernel may ask for: the first launcher of `kernel` on this handle raises the kernel's
// limit to the 160 KB of a CU (an upper bound, not a request; `max_bytes`: less for a kernel with static LDS of its own, which
// counts against the same 160 KB -- the runtime refuses a limit the two exceed together).  Every launcher whose request can
// pass 64 KB comes through here; a handful of kernels ever do, so the list is scanned.
template <class... A> int sf_dyn_lds(sf_context* c, void (*kernel)(A...), size_t lds_bytes, size_t max_bytes = 160 * 1024) {
  if (lds_bytes <= 64 * 1024) return SF_OK;
  for (const void* k : c->dyn_lds_kernels)
    if (k == (const void*)kernel) return SF_OK;
  SF_HIP(c, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_bytes));
  c->dyn_lds_kernels.push_back((const void*)kernel);
  return SF_OK;
}

// one 32-bit word from the device, waited for: the counts that size a launch and the counts a caller asked for
inline int sf_word_to_host(sf_context* c, const void* d_word, void* h_word) {
  SF_HIP(c, hipMemcpyAsync(h_word, d_word, 4, hipMemcpyDeviceToHost, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));
  return SF_OK;
}

// ---- the cells of Vis/GridRows x Vis/GridCols as the images of a detector launch (k_fast.hip, k_gftt.hip, k_grid.hip) ----
// Image z of the launch is cell z % per_image (row-major, `cols` per row) of caller's image z / per_image: its first pixel
// lies at (z / per_image) * img_stride + i * row_step + j * col_step.  per_image 1 (the default): no cells, z * img_stride.
struct SfCells {
  int per_image = 1, cols = 1;
  size_t row_step = 0, col_step = 0;           // bytes: row_size * pitch, col_size
};

// ---- a detector mask (Vis/DepthAsMask; cv's `mask` argument): uint8 planes beside the images of a detector launch, 0 = no
// corner here.  Image z's plane starts at p + sf_cell_base(z, stride, cells): planes with the images' pitch and stride share
// the images' cells.  p null: no mask, today's kernels.
struct SfMask {
  const uint8_t* p = nullptr;
  int pitch = 0;
  size_t stride = 0;
  SfCells cells;
};
// the depth images of an extraction launch (sf_depth_format): image i at p + i * stride bytes, rows `pitch` bytes apart.
// w x h: their own size (sf_depth_set_size; sf_depth_in fills it), 0 = the image's
struct SfDepthIn {
  const void* p = nullptr;
  int format = 0, pitch = 0;
  size_t stride = 0;
  int w = 0, h = 0;
};

// ---- workspace of the corner detectors (k_gftt.hip, k_fast.hip), one image and a batch alike --------------------------
// c->gf_planes: plane_bytes per image for the detector's own planes.  c->gf_keys: the candidate keys of image i at keys +
// i * key_cap, and as much again for their sorted copy.  c->gf_scalar: the per-image arrays max_bits, count, seg_begin,
// seg_end; the first two are zeroed on the stream.
struct SfDetectorWork {
  unsigned key_cap;                            // = pixels of one image
  unsigned long long *keys, *keys_sorted;      // [n_img][key_cap] each
  int* max_bits;                               // [n_img] GFTT: float bits of max(eig)
  unsigned *count, *seg_begin, *seg_end;       // [n_img] candidates found; the image's segment for sf_sort_segments
};
inline int sf_detector_work(sf_context* c, int width, int height, int n_img, size_t plane_bytes, SfDetectorWork* W) {
  const size_t np = (size_t)width * height;
  if (np * (size_t)n_img > 0xFFFFFFFFull) return sf_fail(c, SF_ERANGE, "corner detection: %d images of %zu pixels", n_img, np);
  int rc;
  if ((rc = sf_buf_reserve(c, c->gf_planes, plane_bytes * n_img)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->gf_keys, np * 2 * sizeof(unsigned long long) * n_img)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->gf_scalar, (size_t)n_img * 16)) != SF_OK) return rc;
  W->key_cap = (unsigned)np;
  W->keys = (unsigned long long*)c->gf_keys.p;
  W->keys_sorted = W->keys + np * n_img;
  W->max_bits = (int*)c->gf_scalar.p;
  W->count = (unsigned*)(W->max_bits + n_img);
  W->seg_begin = W->count + n_img;
  W->seg_end = W->seg_begin + n_img;
  SF_HIP(c, hipMemsetAsync(W->max_bits, 0, (size_t)n_img * 8, c->stream));
  return SF_OK;
}

// ---- kernel launchers (one per translation unit) -----------------------------------------------
// Pass-1 global matching for n pairs; also writes PassState defaults and the RANSAC work list.
int sf_launch_match_global(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n);
// the same for uint8 rows compared by L2 (desc_type 2; k_match_u8.hip), which sf_launch_match_global hands on to it
int sf_launch_match_global_u8(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n);
// The stage pipeline's motion estimate of pass 1 or 2 (3D-3D RANSAC or PnP by estimation_type) for the pairs in that
// pass's work list, with the second direction, the merge and the bundle adjustment the parameters ask for (k_verify.hip).
int sf_launch_estimate(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n, int pass);
int sf_launch_camera_gate(sf_context* c, const int32_t* d_to, int n);   // behind the matcher, on a store with camera ids (k_verify.hip)
// Guided matching for pairs whose pass 1 succeeded; builds the pass-2 RANSAC work list.
int sf_launch_guided(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n);
// The bundle adjustment of a pass's estimates as a launch of its own (k_verify.hip)
int sf_launch_ba_pass(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n, int pass, int list_sel,
                      const uint8_t* mask, const uint8_t* run, bool fin, sf_result* d_out);
// Vis/ForwardEstOnly = false with bundle adjustment: merge of a pass's two estimates + adjustment over the union (k_ba.hip)
int sf_launch_merge_directions_ba(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n, int pass,
                                  bool pnp, const uint8_t* mask_f, const uint8_t* mask_b);
// Fused per-pair pipeline (k_verify.hip): match -> RANSAC -> guided -> RANSAC -> result in one launch.
size_t sf_fused_lds_bytes(const sf_context* c, const StoreView& st);
bool sf_split_applicable(const sf_context* c, const StoreView& st);
bool sf_split_pnp_applicable(const sf_context* c, const StoreView& st);
int sf_launch_verify_split(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n,
                           sf_result* d_out, bool narrow_est = false);
int sf_launch_verify_fused(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n,
                           sf_result* d_out);
size_t sf_ransac_lds_bytes(int kcap, int iterations);
size_t sf_ba_lds_bytes(int kcap);
size_t sf_pnp_lds_bytes(int kcap, int iterations);
size_t sf_guided_lds_bytes(int kcap, int n_cells, bool narrow = false);   // narrow: the one- / two-wavefront chains' shorter candidate list
void sf_brief_default_pattern(int8_t* tests, int bytes);
void sf_orb_default_pattern(int8_t* tests);     // [256][4]: 32-byte ORB rows
// The detectors' one library call (sf_sort.hip): radix sort of 64-bit keys by bits [bit0, bit1) on the handle's stream,
// temporary storage in c->gf_tmp.  Every segment [d_begin[s], d_end[s]) is sorted on its own.  Several segments: the bounds
// are read on the device.  ONE segment (a detector on one image): its two bounds cross to the host, with one wait, for a
// device-wide sort of that range, and stay in *hb (hb->known on entry: they are there already, no wait).
// d_also: up to two further words of the detector's control block to bring along with the bounds (-> also).
struct SfSortBounds {
  unsigned begin = 0, end = 0;
  bool known = false;
  const unsigned* d_also[2] = {nullptr, nullptr};
  unsigned also[2] = {0, 0};
  int n() const { return (int)(end - begin); }
};
int sf_sort_segments(sf_context* c, const unsigned long long* in, unsigned long long* out, unsigned n_total, unsigned n_segments,
                     const unsigned* d_begin, const unsigned* d_end, unsigned bit0, unsigned bit1, bool descending,
                     SfSortBounds* hb);
// ---- the five detectors, one launcher each: n_img >= 1 images of one size img_stride bytes apart, d_kpts_out [n_img][cap]
// and d_n_out [n_img] on the device.  Counts, bounds and flags of every image stay on the device, where the kernels read
// them; only the sort of a lone image (sf_sort_segments) waits for the host.  max_features <= 0 (no limit) is for n_img
// == 1 alone: several images' emit grids are sized by it, a lone image's by the count that its sort has brought.
// SfDetectOne: the counts that the single-image entry points of SURF and SIFT (sf_detect.hip; n_img == 1) get back with
// that same wait, so that they wait no more often than they must.  Passing one says that the call is a single call, not
// a batch's chunk: its overflow goes to a word of its own and (SIFT) its pyramid is remembered.
struct SfDetectOne {
  unsigned count[2] = {0, 0};                  // SURF: the maxima found; SIFT: the extrema and the keypoints found
};
// limitKeypoints: what an image keeps of the n it found
inline int sf_limit_keypoints(int n, int max_features) { return max_features > 0 && n > max_features ? max_features : n; }
// SIFT cuts its list once, at the smaller positive of retainBest(n_features) and limitKeypoints(max_features); 0: no cut
__host__ __device__ inline int sf_sift_limit(int n_features, int max_features) {
  int limit = n_features > 0 ? n_features : 0;
  if (max_features > 0 && (limit == 0 || max_features < limit)) limit = max_features;
  return limit;
}
inline int sf_check_limit(sf_context* c, int n_img, int max_features) {
  if (n_img > 1 && max_features < 1) return sf_fail(c, SF_EINVAL, "a detector on %d images needs max_features >= 1, not %d", n_img, max_features);
  return SF_OK;
}
int sf_launch_detect_corners(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height,
                             int pitch, int max_corners, double quality_level, double min_distance,
                             sf_keypoint* d_kpts_out, int cap, int32_t* d_n_out, const SfCells& cells = SfCells(),
                             const SfMask& mask = SfMask());
// the pyramid of the two stereo paths (k_lk.hip builds it, k_lk_track and k_stereo_bm read it)
constexpr int LK_MAX_LEVELS = 16;
struct LkLevel {
  const uint8_t* l;
  const uint8_t* r;
  int w, h, pitch, pad_;
};
struct LkLevels {
  LkLevel v[LK_MAX_LEVELS];
  int n;
  int per_image;                  // batch (blockIdx.y = image): corners / outputs of consecutive images this many apart
  size_t stride0, stride_pyr;     // bytes between consecutive images at level 0 / between their pyramid blocks
  const int32_t* d_n;             // batch: corners of every image (device); null: the scalar n
};
int sf_lk_build_pyramid(sf_context* c, const uint8_t* d_left, const uint8_t* d_right, size_t img_stride, int n_img, int width,
                        int height, int pitch, int ww, int wh, int max_level, int n, const int32_t* d_n, LkLevels* out);
// block matching (k_stereo_bm.hip), the arguments of sf_launch_stereo_flow_batch; prm validated by the caller
int sf_launch_stereo_bm_batch(sf_context* c, const uint8_t* d_left, const uint8_t* d_right, size_t img_stride, int n_img,
                              int width, int height, int pitch, const sf_keypoint* d_kpts, int n, const int32_t* d_n,
                              const sf_stereo_flow_params* prm, int ssd, float* d_right_xy, uint8_t* d_status,
                              float* d_right_x, float* d_score);
int sf_launch_stereo_flow_batch(sf_context* c, const uint8_t* d_left, const uint8_t* d_right, size_t img_stride, int n_img,
                                int width, int height, int pitch, const sf_keypoint* d_kpts, int n, const int32_t* d_n,
                                const sf_stereo_flow_params* prm, float* d_right_xy, uint8_t* d_status, float* d_right_x,
                                float* d_err);
// The descriptor of the handle's feature type: row bytes, device test table, ORB parameters (NULL: BRIEF rows, else ORB
// rows), the pyramid of ORB (NULL: one level; else ORB rows on the keypoint's own level, type 2), the FREAK tables (NULL
// unless the type is 3 or 5).  pyr_stride 0: the
// extraction builds the pyramid of its one image; else sf_launch_detect_orb has left the pyramids of the call's
// images in c->orb_pyr, pyr_stride bytes apart, and the extraction reads them there
struct ExtractKind {
  int bytes = 0;
  const int8_t* d_tests = nullptr;
  const sf_orb_params* orb = nullptr;
  const sf_orb_detector_params* pyr = nullptr;
  size_t pyr_stride = 0;
  const SfFreakTables* freak = nullptr;   // not null: FREAK rows (bytes 64; d_tests, orb and pyr unused)
  const SfSurfTables* surf = nullptr;     // not null: SURF rows (bytes 256 or 512, float32; the rest unused)
  bool has_sift = false;                  // true: SIFT rows (bytes 512, float32, or 128 with sift.u8; `sift` says how, the rest unused)
  SfSiftKind sift;                        // read under has_sift: one image per call, or the chunk the batch detector has left
  // sf_launch_detect_surf has left the integral images of the call's images in c->ex_integral: the extraction reads
  // them there and builds none (as pyr_stride for ORB's pyramids)
  bool integral_ready = false;
};
// the integral image of one image into c->ex_integral (k_extract.hip): (height + 1) x (width + 1) int32
int sf_launch_integral(sf_context* c, const uint8_t* d_image, int width, int height, int pitch, const int32_t** S_out);
// the integral images of n_img images img_stride bytes apart into c->ex_integral, *s_stride entries apart (k_extract.hip)
int sf_launch_integral_batch(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height,
                             int pitch, const int32_t** S_out, size_t* s_stride);
// the SIFT detector + limitKeypoints (k_sift.hip); prm validated by the caller
int sf_sift_validate(sf_context* c, const sf_sift_params& p);
int sf_sift_plan_host(sf_context* c, int width, int height, const sf_sift_params& p, SfSiftPlan* P);
int sf_sift_build_pyramid(sf_context* c, const uint8_t* d_image, int width, int height, int pitch, const sf_sift_params* prm);
int sf_sift_copy_plane(sf_context* c, int octave, int layer, int dog, int16_t* d_out);
// the host arithmetic of SIFT's batch form, no device call (c may be null); candidate_cap 0 = SIFT_MAX_CANDIDATES,
// forced_chunk 0 = what SIFT_BATCH_WORKSPACE_BYTES allows
int sf_sift_batch_plan_host(sf_context* c, int width, int height, const sf_sift_params& p, int n, unsigned candidate_cap,
                            int forced_chunk, SfSiftBatchPlan* out);
// the plan under the handle's limits into c->sift_batch, every buffer of the detector, and the blur tables of p (the one
// wait, when they differ from the handle's): a call's last step before its first launch
int sf_sift_batch_reserve(sf_context* c, int width, int height, const sf_sift_params& p, int n_img);
// resets the call's counter of overflowed keyframes and retires the single call's pyramid (on the stream, no wait)
int sf_sift_batch_begin(sf_context* c);
// the SIFT detector + limitKeypoints on ONE chunk (n_img <= c->sift_batch.chunk images of the size reserved for); the
// chunk's pyramids stay in c->sift_planes for the extraction
int sf_launch_detect_sift(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                          int max_features, const sf_sift_params* prm, sf_keypoint* d_kpts_out, int cap, int32_t* d_n_out,
                          SfDetectOne* one = nullptr);
// the host arithmetic of SURF's batch form, no device call (c may be null); candidate_cap 0 = SURF_MAX_CANDIDATES,
// forced_chunk 0 = what SURF_BATCH_WORKSPACE_BYTES allows
int sf_surf_batch_plan_host(sf_context* c, int width, int height, const sf_surf_params& p, int n, unsigned candidate_cap,
                            int forced_chunk, SfSurfBatchPlan* out);
// the plan under the handle's limits (sf_debug_surf_limits) and every buffer sf_launch_detect_surf takes
int sf_surf_batch_reserve(sf_context* c, int width, int height, const sf_surf_params& p, int n_img, SfSurfBatchPlan* plan);
// the candidate capacity of one image: SURF_MAX_CANDIDATES, or what sf_debug_surf_limits has put in its place
unsigned sf_surf_candidate_cap(const sf_context* c);
// the fast-Hessian detector of SURF + limitKeypoints (k_surf.hip); prm validated by the caller.  The integral images of all
// images stay in c->ex_integral for the extraction
int sf_launch_detect_surf(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                          int max_features, const sf_surf_params* prm, sf_keypoint* d_kpts_out, int cap, int32_t* d_n_out,
                          SfDetectOne* one = nullptr);
// host halves of the FREAK tables (k_freak.hip): the orientation pairs' weights from scale 0 / orientation 0 of a pattern,
// and the device layout of the selected pairs
void sf_freak_orientation_table(const float* pattern, int32_t* orient /* [45][4] */);
void sf_freak_bit_table(const int32_t* selected /* [512] */, uint8_t* table /* [64][8][2] */);
// keyframes into the slots of c->store from `slot` on (k_extract.hip); one keyframe: img_stride 0, n_img 1, d_n null
int sf_launch_extract_batch(sf_context* c, const uint8_t* d_left, size_t img_stride, int n_img, int width, int height,
                            int pitch, const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status, int n,
                            const int32_t* d_n, const sf_stereo_camera* cam, const ExtractKind& kind, int slot,
                            uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out, int32_t* d_rows_out,
                            const SfDepthIn* depth = nullptr);
// depth keyframes (k_depth.hip).  The masks of n depth images of one size (Feature2D::generateKeypoints); the 3D points of
// n keypoints of one depth image, xyz [n][3] and valid [n] (the building block: no keep flags, no store)
int sf_launch_depth_mask(sf_context* c, const SfDepthIn& depth, int n_img, int width, int height, float min_depth, float max_depth,
                         uint8_t* d_mask, int mask_pitch, size_t mask_stride);
// util2d::interpolate: n depth images of depth.w x depth.h enlarged by `factor` >= 1 in their own format (factor 1: copied)
int sf_launch_depth_interp(sf_context* c, const SfDepthIn& depth, int n_img, int factor, void* d_out, int out_pitch, size_t out_stride);
int sf_launch_depth_points_only(sf_context* c, const SfDepthIn& depth, int width, int height, const sf_keypoint* d_kpts, int n,
                                const sf_stereo_camera* cam, float* d_xyz, uint8_t* d_valid);
// depth registration (k_depth_register.hip).  The block as the scatter kernel takes it, a kernel argument: the depth camera,
// the colour camera, the row-major 3 x 4 transform between them, and both sizes (dw x dh depth images to W x H keys)
struct SfDepthRegister {
  float fx, fy, cx, cy, rfx, rfy, rcx, rcy;
  float T[12];
  int dw, dh, W, H;
};
// The keys of a batch fit this much workspace, or the batch runs in chunks of images (one image always runs): the size of
// the Infinity Cache, as the SURF batch keeps it, so that the keys the scatter leaves are still on the die for the resolve
constexpr size_t DEPTH_REGISTER_WORKSPACE_BYTES = (size_t)256 << 20;
// n depth images (depth.w x depth.h = R.dw x R.dh) scattered into d_keys [n][R.H][R.W], which hold 0xFFFFFFFF; the keys
// resolved and filled (fill bit 0: the vertical pair, bit 1: the horizontal pair) into n images of `format`; the fill alone
// on n images of depth.w x depth.h.  Asynchronous on the context's stream; the caller has validated everything
int sf_launch_depth_register_scatter(sf_context* c, const SfDepthIn& depth, int n_img, const SfDepthRegister& R, unsigned* d_keys);
int sf_launch_depth_register_resolve(sf_context* c, const unsigned* d_keys, int format, int w, int h, int n_img, int fill, void* d_out,
                                     int out_pitch, size_t out_stride);
int sf_launch_depth_fill_holes(sf_context* c, const SfDepthIn& depth, int n_img, int fill, void* d_out, int out_pitch, size_t out_stride);
// FAST-9/16 + limitKeypoints (k_fast.hip); prm validated by the caller
int sf_launch_detect_fast(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                          int max_features, const sf_fast_params* prm, sf_keypoint* d_kpts_out, int cap, int32_t* d_n_out,
                          const SfCells& cells = SfCells(), const SfMask& mask = SfMask());
// one level of FAST on n_img images img_stride bytes apart: k_fast_score + k_fast_candidates (image i: score plane at
// + i * plane_stride, keys at + i * key_cap, keys = score << 32 | pixel index in arrival order, count[i] the corners found;
// zeroed by the caller)
void sf_launch_fast_level(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                          int threshold, int nonmax, uint8_t* score, size_t plane_stride, unsigned long long* keys, unsigned* count,
                          unsigned key_cap, const SfCells& cells = SfCells(), const SfMask& mask = SfMask());
// ORB detector (k_orb_detect.hip); det / orb validated by the caller
SfOrbPyr sf_orb_pyr_layout(int width, int height, float scale_factor, int n_levels);
void sf_orb_quotas(int nfeatures, float scale_factor, int n_levels, int* quota);
// levels >= 1 of n_img images (img_stride bytes apart) into c->orb_pyr, image i's at + i * P.total
int sf_launch_orb_pyramid(sf_context* c, const uint8_t* d_image, int pitch, const SfOrbPyr& P, int n_img, size_t img_stride);
// max_features >= 1; the pyramids stay in c->orb_pyr (P.total bytes apart) for the extraction
int sf_launch_detect_orb(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                         int max_features, const sf_orb_detector_params* det, const sf_orb_params* orb, sf_keypoint* d_kpts_out,
                         int cap, int32_t* d_n_out);
// k_orb_angle (k_extract.hip) on keypoints in LEVEL coordinates whose octave names their level: n_img images img_stride
// apart, their pyramids pyr_stride apart in c->orb_pyr, n_max keypoints apiece, d_n [n_img] read on the device
int sf_launch_orb_angle_levels(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int pitch, const SfOrbPyr& P,
                               size_t pyr_stride, const sf_keypoint* d_kpts, int n_max, const int32_t* d_n, int edge,
                               sf_keypoint* d_kpts_out);
// ROI offset + cv::cornerSubPix in place (k_subpix.hip): n keypoints per image, or min(d_n[image], kp_stride) read on the
// device; win 0 or iterations 0: the offset alone
int sf_launch_corner_subpix(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                            sf_keypoint* d_kpts, int n, const int32_t* d_n, int kp_stride, int off_x, int off_y, int win,
                            int iterations, float eps);
// Vis/GridRows x Vis/GridCols (k_grid.hip): the keypoints a detector left per cell -- cell q of keyframe f: d_cell_n[f * cells
// + q] of them at d_cell_kpts + (f * cells + q) * quota -- into the keyframe's list d_kpts + f * rows_cap in cell order, the
// cell's origin (x0 + j * col_size, y0 + i * row_size) added; d_n[f] = the keyframe's count
int sf_launch_grid_gather(sf_context* c, const sf_keypoint* d_cell_kpts, const int32_t* d_cell_n, int n_img, int rows, int cols,
                          int quota, int x0, int y0, int col_size, int row_size, sf_keypoint* d_kpts, int rows_cap, int32_t* d_n);
int sf_launch_stereo_flow(sf_context* c, const uint8_t* d_left, const uint8_t* d_right, int width, int height, int pitch,
                          const sf_keypoint* d_kpts, int n, const sf_stereo_flow_params* prm, float* d_right_xy,
                          uint8_t* d_status, float* d_right_x, float* d_err);
// Assemble sf_result records.
int sf_launch_finalize(sf_context* c, int n, sf_result* d_out);
// Ingest kernels
int sf_launch_ingest(sf_context* c, Store& st, int first_slot, int n, int rows, int cols,
                     const uint8_t* d_desc, const float* d_xyz, const sf_keypoint* d_kp);
// Store slots as one block of bytes (k_store_wire.hip; the layout: include/sepfinder.h, sf_kfblob_header).  All three are
// asynchronous on the context's stream.  d_status: int32[4] {bits, emptied slots, first emptied keyframe or -1, 0}.
// plan: header and table of slots [first_slot, first_slot + n) into d_plan (32 + 32 n bytes); resets d_status unless NULL
int sf_launch_kfblob_plan(sf_context* c, const Store& st, int first_slot, int n, void* d_plan, int32_t* d_status);
// pack: d_plan and the blocks it describes into d_blob, or -- the blob exceeds cap_bytes -- a header with magic 0 alone
int sf_launch_kfblob_pack(sf_context* c, const Store& st, int first_slot, int n, const void* d_plan, void* d_blob,
                          uint64_t cap_bytes, int32_t* d_status);
// unpack: the n keyframes of the blob into slots first_slot ..., every one checked against (bytes, n, max_rows, the
// handle's descriptor type and the store's width class); resets d_status
int sf_launch_kfblob_unpack(sf_context* c, Store& st, int first_slot, int n, int max_rows, int cols, const void* d_blob,
                            uint64_t bytes, int32_t* d_status);
// NN stage
int sf_nn_run(sf_context* c, sf_match* out, int cap, int* n_out);
int sf_nn_row_minima_dev(sf_context* c, double* d_row_min, int32_t* d_row_arg, int32_t* d_status);
int sf_nn_walk_dev(sf_context* c, const double* d_row_min, const int32_t* d_row_arg, const int32_t* d_status, int n_l,
                   int n_r, double thr, int max_matches_nb, int cap, void* d_match_rc, unsigned* d_count_block,
                   sf_match* out_matches, int32_t* out_n, int32_t* out_status, const int32_t* d_row_cand = nullptr,
                   int32_t* out_slot = nullptr, const unsigned* d_cand_count = nullptr, unsigned cand_grid = 0);
// the filter path of sf_nn_row_minima_dev in its two halves (k_nn.hip)
struct NnFilterOut {
  const void* cand = nullptr;       // uint2 (row, column)[]
  const unsigned* count = nullptr;  // its length (device), word 4 of the same 64-byte block: the accept stream's slot counter
  double* cdist = nullptr;          // exact distances, filled by the second half
  unsigned limit = 0, typical = 0;
};
int sf_nn_filter_dev(sf_context* c, NnFilterOut* out);
int sf_nn_minima_of_candidates_dev(sf_context* c, const NnFilterOut& fo, double* d_row_min, int32_t* d_row_arg,
                                   int32_t* d_status, int32_t* d_row_cand, unsigned long long* d_arg64, bool throttle);
int sf_nn_walk_host(sf_context* c, const double* row_min, const int32_t* row_arg, int n_l, int n_r, double thr,
                    int max_matches_nb, sf_match* out, int cap, int* n_out);
// Speculation hook (sf_step.hip), called by the NN filter right behind the refinement launch of a prefix level:
// builds the candidate pair list on the device and queues the verification of every candidate.
int sf_spec_launch(sf_context* c, const void* d_cand, const unsigned* d_count);
int sf_nn_append(sf_context* c, NNDb& db, const void* src, int n, int dim, int src_kind);
