// sf_handle.hip -- the handle of include/sepfinder.h: errors, device buffers, profiling brackets, parameters and
// environment knobs, sf_create / sf_destroy, options.  gfx950 only; there is no CPU path: sf_create fails with
// SF_ENODEV when no GPU is visible.
#include <math.h>
#include <stdarg.h>

#include <atomic>

#include "sf_host.hpp"

static thread_local std::string g_create_error;

int sf_fail(sf_context* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_error = buf;
  return code;
}

// ---- the owning types' allocate and free paths (sf_internal.hpp), and the counts of what is live -----------------------------
static std::atomic<int64_t> g_live[4];   // device blocks, device bytes, pinned blocks, events (sf_debug_live_resources)
static void live_add(int what, int64_t n) { g_live[what].fetch_add(n, std::memory_order_relaxed); }

extern "C" void sf_debug_live_resources(int64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = g_live[i].load(std::memory_order_relaxed);
}

int sf_buf_reserve(sf_context* c, Buf& b, size_t bytes, bool keep) {
  if (bytes <= b.bytes) return SF_OK;
  size_t want = std::max(bytes, b.bytes + b.bytes / 2);
  Buf n;
  hipError_t e = hipMalloc(&n.p, want);
  if (e != hipSuccess) return sf_fail(c, SF_ENOMEM, "hipMalloc(%zu) -> %s", want, hipGetErrorString(e));
  n.bytes = want;
  live_add(0, 1); live_add(1, (int64_t)want);
  if (b.p) {
    if (keep && b.bytes) {
      e = hipMemcpyAsync(n.p, b.p, b.bytes, hipMemcpyDeviceToDevice, c->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
      if (e != hipSuccess) return sf_fail(c, SF_EHIP, "grow copy -> %s", hipGetErrorString(e));
    } else {
      (void)hipStreamSynchronize(c->stream);
    }
  }
  b = std::move(n);
  return SF_OK;
}

void sf_buf_free(Buf& b) {
  if (b.p) { (void)hipFree(b.p); live_add(0, -1); live_add(1, -(int64_t)b.bytes); }
  b.p = nullptr;
  b.bytes = 0;
}

int sf_pinned_reserve(sf_context* c, Pinned& b, size_t need, size_t alloc) {
  if (need <= b.bytes) return SF_OK;
  sf_pinned_free(b);
  if (hipHostMalloc(&b.p, alloc, hipHostMallocDefault) != hipSuccess) { b.p = nullptr; return sf_fail(c, SF_ENOMEM, "hipHostMalloc(%zu) failed", alloc); }
  b.bytes = alloc;
  live_add(2, 1);
  return SF_OK;
}

void sf_pinned_free(Pinned& b) {
  if (b.p) { (void)hipHostFree(b.p); live_add(2, -1); }
  b.p = nullptr;
  b.bytes = 0;
}

int sf_event_ensure(sf_context* c, Event& ev) {
  if (ev.e) return SF_OK;
  SF_HIP(c, hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
  live_add(3, 1);
  return SF_OK;
}

void sf_event_free(Event& ev) {
  if (ev.e) { (void)hipEventDestroy(ev.e); live_add(3, -1); }
  ev.e = nullptr;
}

// ---- profiling ------------------------------------------------------------------------------
static const char* k_names[SF_K_COUNT] = {"k_match_global", "k_ransac(pass1)", "k_guided",
                                          "k_ransac(pass2)", "k_nn_argmin", "k_nn_select",
                                          "k_nn_filter_f16", "k_nn_refine", "k_verify_fused", "k_nn_walk", "k_ba_pass",
                                          "k_guided_tp"};
const char* sf_kernel_name(int k) { return (k >= 0 && k < SF_K_COUNT) ? k_names[k] : "?"; }

// A completed bracket: its elapsed time goes to its kernel's slot, its two events back to the pool
static void prof_book(sf_context* c, const std::pair<int, std::pair<hipEvent_t, hipEvent_t>>& pe) {
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, pe.second.first, pe.second.second) == hipSuccess) {
    c->prof_slots[pe.first].launches += 1;
    c->prof_slots[pe.first].total_ms += (double)ms;
  }
  c->prof_event_pool.push_back(pe.second.first);
  c->prof_event_pool.push_back(pe.second.second);
}

// Brackets that have completed are booked and their events reused without waiting for anything: a long profiled
// run then lives on a handful of events (creating two per launch made the runtime grow its signal pool in the
// middle of a timed region: one 7 ms step every few hundred launches).
static void prof_harvest(sf_context* c) {
  size_t done = 0;
  while (done < c->pending_events.size() && hipEventQuery(c->pending_events[done].second.second) == hipSuccess)
    prof_book(c, c->pending_events[done++]);
  if (done) c->pending_events.erase(c->pending_events.begin(), c->pending_events.begin() + (long)done);
}

void sf_prof_begin(sf_context* c, int kernel) {
  if (!c->prof || !((c->prof_mask >> kernel) & 1u)) return;
  if (c->prof_event_pool.size() < 2 && c->pending_events.size() >= 4) prof_harvest(c);
  hipEvent_t a = nullptr, b = nullptr;
  for (hipEvent_t* e : {&a, &b}) {
    if (!c->prof_event_pool.empty()) { *e = c->prof_event_pool.back(); c->prof_event_pool.pop_back(); }
    else if (hipEventCreate(e) != hipSuccess) { if (a) c->prof_event_pool.push_back(a); return; }
  }
  (void)hipEventRecord(a, c->stream);
  c->pending_events.push_back({kernel, {a, b}});
}

void sf_prof_end(sf_context* c, int kernel) {
  if (!c->prof || c->pending_events.empty()) return;
  auto& pe = c->pending_events.back();
  if (pe.first != kernel) return;
  (void)hipEventRecord(pe.second.second, c->stream);
}

static void prof_resolve(sf_context* c) {
  if (c->pending_events.empty()) return;
  (void)hipStreamSynchronize(c->stream);
  for (auto& pe : c->pending_events) prof_book(c, pe);
  c->pending_events.clear();
}

// ---- parameters ---------------------------------------------------------------------------------
extern "C" int sf_abi_version(void) { return SF_ABI_VERSION; }

extern "C" void sf_default_params(sf_params* p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->netvlad_distance = 0.13;        // multi_robot_separators.launch:19
  p->netvlad_dimensions = 128;       // :20
  p->netvlad_max_matches_nb = 20;    // :22
  p->nn_precision = 1;               // fp16 filter + exact f64 refinement (identical matches)
  p->min_inliers = 5;                // :23 separators_min_inliers
  p->inlier_distance = 0.1f;         // rtabmap Vis/InlierDistance [upstream default]
  p->iterations = 300;               // Vis/Iterations
  p->refine_iterations = 5;          // Vis/RefineIterations
  p->refine_sigma = 3.0;
  p->estimation_type = 0;            // 3D->3D (BASELINE.json north_star)
  p->nndr = 0.6f;                    // Vis/CorNNDR
  p->guess_win_size = 20;            // Vis/CorGuessWinSize
  p->ransac_adaptive_stop = 1;
  p->max_sample_checks = 1000;
  p->seed = 12345;
  const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  memcpy(p->local_transform, I, sizeof(I));
  p->store_capacity = 1024;
  p->max_features = 512;
  p->desc_bytes = 32;
  p->pnp_reproj_error = 2.0f;        // Vis/PnPReprojError
  p->pnp_flags = 0;                  // Vis/PnPFlags (cv::SOLVEPNP_ITERATIVE)
  p->pnp_refine_iterations = 0;      // Vis/PnPRefineIterations
  p->bundle_adjustment = 0;          // Vis/BundleAdjustment (rtabmap: 1 with g2o; off here: north_star's path has none)
  p->ba_iterations = 20;             // Optimizer/Iterations
  p->ba_robust_kernel_delta = 8.f;   // g2o/RobustKernelDelta
  p->ba_pixel_variance = 1.f;        // g2o/PixelVariance
  p->stereo_baseline = 0.f;
  p->force_3dof = 0;                 // Reg/Force3DoF
  p->forward_est_only = 1;           // Vis/ForwardEstOnly
  p->desc_type = 0;                  // binary descriptors (the reference's wire carries nothing else)
  p->guess_match_to_projection = 0;  // Vis/CorGuessMatchToProjection
}

int sf_fill_device_params(sf_context* c) {
  const sf_params& p = c->params;
  if (p.estimation_type != 0 && p.estimation_type != 1)
    return sf_fail(c, SF_EINVAL, "estimation_type %d not implemented (0 = 3D->3D, 1 = PnP)", p.estimation_type);
  if (p.estimation_type == 1) {
    if (p.pnp_flags != 0) return sf_fail(c, SF_EINVAL, "pnp_flags %d not implemented (0 = SOLVEPNP_ITERATIVE only)", p.pnp_flags);
    if (p.pnp_refine_iterations < 0) return sf_fail(c, SF_EINVAL, "pnp_refine_iterations must be >= 0");
    if (!(p.pnp_reproj_error > 0.f)) return sf_fail(c, SF_EINVAL, "pnp_reproj_error must be > 0");
  }
  if (p.min_inliers < 1) return sf_fail(c, SF_EINVAL, "min_inliers must be >= 1 (myRegistrationVis.cpp:117)");
  if (!(p.inlier_distance > 0.f)) return sf_fail(c, SF_EINVAL, "inlier_distance must be > 0 (:118)");
  if (p.iterations < 1) return sf_fail(c, SF_EINVAL, "iterations must be > 0 (:119)");
  if (p.iterations > 30000) return sf_fail(c, SF_ERANGE, "iterations > 30000");
  if (p.max_sample_checks < 1) return sf_fail(c, SF_EINVAL, "max_sample_checks must be >= 1");
  if (p.netvlad_max_matches_nb < 0) return sf_fail(c, SF_EINVAL, "netvlad_max_matches_nb < 0");
  if (p.bundle_adjustment != 0) {
    if (p.bundle_adjustment != 1) return sf_fail(c, SF_EINVAL, "bundle_adjustment %d not implemented (0 = off, 1 = on)", p.bundle_adjustment);
    if (!(p.image_width > 0 && p.image_height > 0 && p.fx > 0.0 && p.fy > 0.0))
      return sf_fail(c, SF_EINVAL, "bundle adjustment needs a calibrated camera (myRegistrationVis.cpp:1230 UASSERT)");
    if (p.ba_iterations < 0 || !(p.ba_pixel_variance > 0.f) || !(p.ba_robust_kernel_delta > 0.f) || !(p.stereo_baseline >= 0.f))
      return sf_fail(c, SF_EINVAL, "bundle adjustment: ba_iterations >= 0, ba_pixel_variance > 0, ba_robust_kernel_delta > 0, stereo_baseline >= 0");
  }
  if (p.desc_type != 0 && p.desc_type != 1 && p.desc_type != 2)
    return sf_fail(c, SF_EINVAL, "desc_type %d unknown (0 = binary rows, 1 = float32 rows, 2 = uint8 rows compared by L2)", p.desc_type);
  if (p.desc_type == 1 && p.desc_bytes != 256 && p.desc_bytes != 512 && p.desc_bytes != 32)
    return sf_fail(c, SF_EINVAL, "desc_type 1: desc_bytes %d (float32 rows of 64 or 128 dimensions: 256 or 512)", p.desc_bytes);
  if (p.desc_type == 2 && p.desc_bytes != SF_DESC_BYTES_U8 && p.desc_bytes != 32)
    return sf_fail(c, SF_EINVAL, "desc_type 2: desc_bytes %d (uint8 rows of 128 dimensions: %d)", p.desc_bytes, SF_DESC_BYTES_U8);
  // float32 descriptors with the width left at sf_default_params' 32 (a binary width): 64 dimensions.  The width only
  // matters before the first non-empty keyframe arrives -- an EMPTY first keyframe (the reference tolerates them: the
  // fake-words path) takes it for its row pitch, and 32 bytes per float row was refused by the store (round 4).
  if (p.desc_type == 1 && p.desc_bytes == 32) c->params.desc_bytes = 256;
  if (p.desc_type == 2 && p.desc_bytes == 32) c->params.desc_bytes = SF_DESC_BYTES_U8;   // (the same for uint8 rows: the one width)
  if (p.guess_match_to_projection != 0 && p.guess_match_to_projection != 1)
    return sf_fail(c, SF_EINVAL, "guess_match_to_projection %d unknown (0 = projections to frame, 1 = frame to projections)",
                   p.guess_match_to_projection);
  DeviceParams& d = c->dparams;
  memset(&d, 0, sizeof(d));
  d.force_3dof = p.force_3dof != 0;
  d.bidirectional = p.forward_est_only == 0;
  d.guess_match_to_projection = p.guess_match_to_projection;
  d.nndr = p.nndr;
  d.min_inliers = p.min_inliers;
  d.iterations = p.iterations;
  d.refine_iterations = p.refine_iterations;
  d.refine_sigma = p.refine_sigma;
  d.inlier_thr = (double)p.inlier_distance;
  d.adaptive_stop = p.ransac_adaptive_stop;
  d.max_sample_checks = p.max_sample_checks;
  d.seed = p.seed;
  d.guess_win = p.guess_win_size;
  d.calibrated = (p.image_width > 0 && p.image_height > 0 && p.fx > 0.0 && p.fy > 0.0) ? 1 : 0;
  d.fx = p.fx; d.fy = p.fy; d.cx = p.cx; d.cy = p.cy;
  d.wlim = (float)(p.image_width - 1);
  d.hlim = (float)(p.image_height - 1);
  memcpy(d.L, p.local_transform, sizeof(d.L));
  d.estimation_type = p.estimation_type;
  d.pnp_reproj_error = p.pnp_reproj_error;
  d.pnp_refine_iterations = p.pnp_refine_iterations;
  d.bundle_adjustment = p.bundle_adjustment;
  d.ba_iterations = p.ba_iterations;
  d.ba_robust_kernel_delta = p.ba_robust_kernel_delta;
  d.ba_pixel_variance = p.ba_pixel_variance;
  d.stereo_baseline = p.stereo_baseline;
  {
    const double thr = (double)p.pnp_reproj_error;
    d.pnp_thr2f = (float)(thr * thr);     // OpenCV: float t = (float)(thresh*thresh); err <= t
  }
  if (const char* v = getenv("SF_RANSAC_STOP")) d.dbg_stop = atoi(v);
  sf_guided_grid(p.image_width, p.image_height, p.guess_win_size, &d.grid_gx, &d.grid_gy, &d.grid_inv_cell);
  return SF_OK;
}

// grid for the guided pass over an image: cell >= window radius, at most 48 x 48 cells
void sf_guided_grid(int image_width, int image_height, int guess_win_size, int32_t* gx, int32_t* gy, float* inv_cell) {
  const float w = (float)std::max(image_width, 1), h = (float)std::max(image_height, 1);
  float cell = std::max((float)std::max(guess_win_size, 1), std::max(ceilf(w / 48.f), ceilf(h / 48.f)));
  cell *= 1.001f;   // strictly larger than the padded reach used by the kernel
  *gx = std::max(1, std::min(48, (int)ceilf(w / cell)));
  *gy = std::max(1, std::min(48, (int)ceilf(h / cell)));
  *inv_cell = 1.f / cell;
}

// What DeviceParams derives from the sf_params camera, for one model of the handle's table (same expressions)
void sf_camera_derive(const sf_camera_model& m, int guess_win_size, CameraBlock* b) {
  memset(b, 0, sizeof(*b));
  b->calibrated = (m.image_width > 0 && m.image_height > 0 && m.fx > 0.0 && m.fy > 0.0) ? 1 : 0;
  b->fx = m.fx; b->fy = m.fy; b->cx = m.cx; b->cy = m.cy;
  b->wlim = (float)(m.image_width - 1);
  b->hlim = (float)(m.image_height - 1);
  memcpy(b->L, m.local_transform, sizeof(b->L));
  b->stereo_baseline = m.stereo_baseline;
  sf_guided_grid(m.image_width, m.image_height, guess_win_size, &b->grid_gx, &b->grid_gy, &b->grid_inv_cell);
}

// The environment's knobs of a handle (sf_create; the device-free planner sf_debug_plan_workspace applies them too, so
// that it plans what a handle created in the same environment would do)
void sf_env_knobs(sf_context* c) {
  if (const char* v = getenv("SF_MATCH_VARIANT")) c->match_variant = atoi(v);
  if (const char* v = getenv("SF_FUSED")) {   // 0: stage kernels (A/B reference), 1: fused kernel, 2: split pipeline
    c->fused = atoi(v) != 0;
    c->split = atoi(v) == 2;
  }
  if (const char* v = getenv("SF_STEP_SPLIT_MIN")) c->split_auto_min = std::max(1, atoi(v));
  if (const char* v = getenv("SF_STEP_SPLIT")) c->split_auto = atoi(v) != 0;   // 0: overlapped steps keep the fused kernel
  if (const char* v = getenv("SF_CHAIN_PNP")) c->chain_pnp = atoi(v) != 0;      // 0: PnP on the five stage launches
  if (const char* v = getenv("SF_BA_OCC")) c->ba_occ = atoi(v) == 1 ? 1 : atoi(v) == 2 ? 2 : 0;
  if (const char* v = getenv("SF_BA_NW")) { const int nw = atoi(v); c->ba_nw = (nw == 1 || nw == 2) ? nw : 4; }
  if (const char* v = getenv("SF_CHAIN_PNP_NW")) { const int nw = atoi(v); c->chain_pnp_nw = (nw == 1 || nw == 2) ? nw : 4; }
  if (const char* v = getenv("SF_CHAIN_NW")) { const int nw = atoi(v); c->chain_nw = (nw == 1 || nw == 2) ? nw : 4; }
  if (const char* v = getenv("SF_CHAIN_NARROW_EST")) c->chain_narrow_est = atoi(v) != 0;   // the three-launch 3D-3D chain
  if (const char* v = getenv("SF_RECTIFY_TABLE")) c->rect_table = atoi(v) != 0;   // 1: computed rectification plans run the table form
  if (const char* v = getenv("SF_MATCH_MFMA")) c->match_mfma = atoi(v) != 0;   // 0: VALU matcher (A/B reference)
  if (const char* v = getenv("SF_DEBUG_CORR")) c->debug_corr = atoi(v) != 0;   // 1: correspondence lists kept in HBM
  if (const char* v = getenv("SF_OVERLAP")) c->overlap = atoi(v) != 0;         // 1: two-stream halves (sf_verify_device)
  if (const char* v = getenv("SF_STEP_OVERLAP")) c->step_overlap = atoi(v) != 0;   // 1: SF_OPT_STEP_OVERLAP from the start
  if (const char* v = getenv("SF_OVERLAP_MIN")) c->overlap_min_pairs = std::max(2, atoi(v));
  if (const char* v = getenv("SF_STEP_DEPTH")) c->step_depth = std::max(1, std::min(SF_STEP_MAX_DEPTH, atoi(v)));
  if (const char* v = getenv("SF_STEP_LANES")) c->step_lanes = std::max(1, std::min(SF_STEP_MAX_LANES, atoi(v)));
  if (const char* v = getenv("SF_STEP_SPECULATE")) c->step_speculate = atoi(v) != 0;   // 0: every device step in the serial form
  if (const char* v = getenv("SF_STEP_DEVICE_WALK")) c->step_device_walk = atoi(v) != 0;   // 0: round 3's host walk inside sf_step_issue
}

// ---- lifecycle ----------------------------------------------------------------------------------
extern "C" int sf_create(const sf_params* p, int device, sf_handle* out) {
  if (!out) return SF_EINVAL;
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return sf_fail(nullptr, SF_ENODEV, "no HIP device visible (%s); this library has no CPU fallback",
                   e == hipSuccess ? "count = 0" : hipGetErrorString(e));
  if (device < 0 || device >= ndev) return sf_fail(nullptr, SF_EINVAL, "device %d out of range (%d visible)", device, ndev);
  sf_context* c = new (std::nothrow) sf_context();
  if (!c) return SF_ENOMEM;
  if (p) c->params = *p; else sf_default_params(&c->params);
  c->device = device;
  int rc = sf_fill_device_params(c);
  if (rc != SF_OK) { g_create_error = c->err; delete c; return rc; }
  if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
    sf_fail(nullptr, SF_EHIP, "device init -> %s", hipGetErrorString(e));
    delete c;
    return SF_EHIP;
  }
  c->own_stream = true;
  c->ws[0].stream = c->stream;
  sf_env_knobs(c);
  if ((rc = sf_buf_reserve(c, c->w->counters, 64)) != SF_OK) { g_create_error = c->err; sf_destroy(c); return rc; }
  *out = c;
  return SF_OK;
}

// Orders, does not enumerate: every buffer, pinned block and event is a member of an owning type and goes with `delete c`.
// Nothing may be freed before the streams have drained, and the device is selected before the destructors run.
extern "C" void sf_destroy(sf_handle c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (Workspace& w : c->ws) {
    if (w.stream) (void)hipStreamSynchronize(w.stream);
    if (w.aux) (void)hipStreamSynchronize(w.aux);
  }
  if (c->spec.copy_stream) (void)hipStreamSynchronize(c->spec.copy_stream);
  prof_resolve(c);
  for (hipEvent_t e : c->prof_event_pool) (void)hipEventDestroy(e);
  (void)sf_comm_destroy(c);
  sf_netvlad_free(c);
  sf_ingest_pool_destroy(c);
  // the streams stay explicit: whose they are depends on own_stream, the lane and the placement's hand-out
  for (int k = 0; k <= SF_STEP_MAX_LANES; ++k) {
    Workspace& w = c->ws[k];
    if (w.aux) (void)hipStreamDestroy(w.aux);
    if (w.stream && (k > 0 || c->own_stream)) (void)hipStreamDestroy(w.stream);
  }
  for (int k = 0; k < SF_STEP_MAX_LANES; ++k) {                 // (placed streams nobody asked for)
    if (c->placement.main[k]) (void)hipStreamDestroy(c->placement.main[k]);
    if (c->placement.aux[k]) (void)hipStreamDestroy(c->placement.aux[k]);
  }
  if (c->placement.copy) (void)hipStreamDestroy(c->placement.copy);
  if (c->spec.copy_stream) (void)hipStreamDestroy(c->spec.copy_stream);
  delete c;
}

extern "C" const char* sf_last_error(sf_handle c) { return c ? c->err.c_str() : g_create_error.c_str(); }

extern "C" int sf_get_params(sf_handle c, sf_params* out) {
  if (!c || !out) return SF_EINVAL;
  *out = c->params;
  return SF_OK;
}

extern "C" int sf_set_stream(sf_handle c, void* hip_stream) {
  if (!c) return SF_EINVAL;
  (void)sf_lanes_touch(c, true);
  SF_HIP(c, hipStreamSynchronize(c->stream));
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  c->stream = c->ws[0].stream = (hipStream_t)hip_stream;
  c->own_stream = false;
  return SF_OK;
}

extern "C" int sf_synchronize(sf_handle c) {
  if (!c) return SF_EINVAL;
  for (Workspace& w : c->ws) {
    if (w.stream || &w == c->ws) SF_HIP(c, hipStreamSynchronize(w.stream));   // (the handle's own may be the null stream)
    if (w.aux) SF_HIP(c, hipStreamSynchronize(w.aux));
  }
  return SF_OK;
}

// ---- separator records ----------------------------------------------------------------------------
extern "C" int sf_pack_separators(const sf_result* res, int32_t n, int8_t robot_from, int8_t robot_to,
                                  const int16_t* kf_from, const int16_t* kf_to, const int16_t* frame_from,
                                  const int16_t* frame_to, sf_separator* out) {
  if (n < 0 || (n > 0 && (!res || !out))) return SF_EINVAL;
  for (int i = 0; i < n; ++i) {
    sf_separator s;
    memset(&s, 0, sizeof(s));
    s.robot_from_id = robot_from;
    s.robot_to_id = robot_to;
    s.kf_id_from = kf_from ? kf_from[i] : 0;
    s.kf_id_to = kf_to ? kf_to[i] : 0;
    s.frame_id_from = frame_from ? frame_from[i] : 0;
    s.frame_id_to = frame_to ? frame_to[i] : 0;
    s.transform_est_success = res[i].success;
    memcpy(s.position, res[i].position, sizeof(s.position));
    memcpy(s.orientation, res[i].orientation, sizeof(s.orientation));
    memcpy(s.covariance, res[i].covariance, sizeof(s.covariance));
    out[i] = s;
  }
  return SF_OK;
}

// ---- measurement ----------------------------------------------------------------------------------
extern "C" int sf_prof_enable(sf_handle c, int on) {
  if (!c) return SF_EINVAL;
  prof_resolve(c);
  c->prof = on != 0;
  return SF_OK;
}

extern "C" int sf_prof_select(sf_handle c, uint32_t kernel_mask) {
  if (!c) return SF_EINVAL;
  prof_resolve(c);
  c->prof_mask = kernel_mask;
  return SF_OK;
}

extern "C" int sf_prof_reset(sf_handle c) {
  if (!c) return SF_EINVAL;
  prof_resolve(c);
  for (auto& s : c->prof_slots) s = ProfSlot();
  return SF_OK;
}

extern "C" int sf_prof_get(sf_handle c, int kernel, int64_t* launches, double* total_ms) {
  if (!c || kernel < 0 || kernel >= SF_K_COUNT) return SF_EINVAL;
  prof_resolve(c);
  if (launches) *launches = c->prof_slots[kernel].launches;
  if (total_ms) *total_ms = c->prof_slots[kernel].total_ms;
  return SF_OK;
}

extern "C" int sf_set_option(sf_handle c, int32_t option, int32_t value) {
  if (!c) return SF_EINVAL;
  switch (option) {
    case SF_OPT_MATCH_MFMA: c->match_mfma = value != 0; return SF_OK;
    case SF_OPT_FUSED: c->fused = value != 0; return SF_OK;
    case SF_OPT_OVERLAP: c->overlap = value != 0; return SF_OK;
    case SF_OPT_CHAIN_WAVES: return SF_OK;   // (round 1's narrower chains are gone: accepted, no effect)
    case SF_OPT_DEBUG_CORR: c->debug_corr = value != 0; return SF_OK;
    case SF_OPT_NN_FULL_FILTER: c->nn_force_full = value != 0; c->nn_coef_level = -1; return SF_OK;
    case SF_OPT_STEP_SPLIT: c->split_auto = value != 0; return SF_OK;
    case SF_OPT_CHAIN_NARROW_EST: c->chain_narrow_est = value != 0; return SF_OK;
    case SF_OPT_RECTIFY_TABLE: c->rect_table = value != 0; return SF_OK;
    case SF_OPT_STEP_OVERLAP:
      if (c->step_inflight) return sf_fail(c, SF_EINVAL, "SF_OPT_STEP_OVERLAP cannot change while steps are in flight");
      c->step_overlap = value != 0;
      return SF_OK;
    case SF_OPT_STEP_DEPTH:
      if (c->step_inflight) return sf_fail(c, SF_EINVAL, "SF_OPT_STEP_DEPTH cannot change while steps are in flight");
      if (value < 1 || value > SF_STEP_MAX_DEPTH) return sf_fail(c, SF_ERANGE, "SF_OPT_STEP_DEPTH %d not in 1..%d", value, SF_STEP_MAX_DEPTH);
      c->step_depth = value;
      c->step_seq = 0;
      return SF_OK;
    case SF_OPT_STEP_LANES:
      if (c->step_inflight) return sf_fail(c, SF_EINVAL, "SF_OPT_STEP_LANES cannot change while steps are in flight");
      if (value < 1 || value > SF_STEP_MAX_LANES) return sf_fail(c, SF_ERANGE, "SF_OPT_STEP_LANES %d not in 1..%d", value, SF_STEP_MAX_LANES);
      c->step_lanes = value;
      return SF_OK;
    case SF_OPT_STEP_SPECULATE:
      if (c->step_inflight) return sf_fail(c, SF_EINVAL, "SF_OPT_STEP_SPECULATE cannot change while steps are in flight");
      c->step_speculate = value != 0;
      return SF_OK;
    case SF_OPT_STEP_DEVICE_WALK:
      if (c->step_inflight) return sf_fail(c, SF_EINVAL, "SF_OPT_STEP_DEVICE_WALK cannot change while steps are in flight");
      c->step_device_walk = value != 0;
      return SF_OK;
    default: return sf_fail(c, SF_EINVAL, "unknown option %d", option);
  }
}
