// sf_verify_host.hip -- host side of the verification: the plan of a call and its workspace, sf_verify_device and the
// sf_verify_* / sf_estimate_transform* entry points, the ordered compaction of accepted results, the sf_debug_* readers.
#include "sf_host.hpp"

// ---- verification pipeline ------------------------------------------------------------------------
// lists: the correspondence lists live in HBM (stage kernels, or the fused kernel with SF_OPT_DEBUG_CORR); the fused
// kernel otherwise keeps them in LDS and the two kcap-entry arrays per pair are not needed
// Bytes of each workspace array for a launch sequence of n pairs: what ws_reserve reserves, as a pure function (also what
// sf_debug_plan_workspace reports, so that a test without a GPU can hold it against what each launch form writes).
struct WsBytes { size_t corr1, corr2, hdr1, hdr2, pass1, pass2, list1, list3, flags; };
// ... its rows in the order sf_debug_plan_workspace reports them, and the workspace buffer behind each
static size_t WsBytes::* const WS_ROW[9] = {&WsBytes::corr1, &WsBytes::corr2, &WsBytes::hdr1, &WsBytes::hdr2, &WsBytes::pass1,
                                            &WsBytes::pass2, &WsBytes::list1, &WsBytes::list3, &WsBytes::flags};
static Buf Workspace::* const WS_BUF[9] = {&Workspace::corr1, &Workspace::corr2, &Workspace::hdr1, &Workspace::hdr2, &Workspace::pass1,
                                           &Workspace::pass2, &Workspace::list1, &Workspace::list3, &Workspace::flags};
static WsBytes ws_bytes(int n, int kcap, bool lists) {
  const size_t np = (size_t)n;
  WsBytes w;
  w.corr1 = w.corr2 = lists ? np * kcap * 4 : 0;
  w.hdr1 = w.hdr2 = np * sizeof(CorrHeader);
  w.pass1 = w.pass2 = np * sizeof(PassState);
  w.list1 = w.list3 = np * 4;
  w.flags = np;
  return w;
}

static int ws_reserve(sf_context* c, int n, int kcap, bool lists) {
  int rc;
  const size_t np = (size_t)n;
  const WsBytes w = ws_bytes(n, kcap, lists);
  for (int i = 0; i < 9; ++i)      // (without lists corr1 / corr2 ask for zero bytes: nothing is reserved)
    if ((rc = sf_buf_reserve(c, c->w->*WS_BUF[i], w.*WS_ROW[i])) != SF_OK) return rc;
#ifndef SF_CHAIN_TRACE
  if (getenv("SF_DIAG")) {     // experiment: eight 64-bit diagnostic counters the kernels may bump (sf_debug_counters)
    // [0..511]: counters; then two 64-bit planes of [pair][kcap] per-point records of the guided pass
    const size_t need = 4096 + 2 * np * (size_t)kcap * 8;
    if (c->trace.bytes < need) {
      if ((rc = sf_buf_reserve(c, c->trace, need)) != SF_OK) return rc;
      SF_HIP(c, hipMemsetAsync(c->trace.p, 0, c->trace.bytes, c->stream));
    }
    c->dparams.dbg_trace = (unsigned long long*)c->trace.p;
  }
#endif
#ifdef SF_CHAIN_TRACE
  if ((rc = sf_buf_reserve(c, c->trace, np * SF_TRACE_SLOTS * 8)) != SF_OK) return rc;
  SF_HIP(c, hipMemsetAsync(c->trace.p, 0, np * SF_TRACE_SLOTS * 8, c->stream));
  c->dparams.dbg_trace = (unsigned long long*)c->trace.p;
#endif
  c->w->ws_pairs = n;
  c->w->ws_kcap = kcap;
  return SF_OK;
}

static const int SF_CHUNK = 131072;  // pairs per launch sequence (bounds the workspace: ~4 KiB / pair at K = 500);
                                     // every launch ends with the latency tail of its last surviving pairs, so few, big chunks

// Which form the 3D-3D verification of n pairs takes: the fused kernel (one workgroup carries a pair through matching
// and both motion-estimation chains) or the split form (k_match_split over all pairs + k_chain over the survivors).
// On one stream the fused kernel wins (its chains overlap other pairs' matching inside the launch: 19.5 against 17.1 M
// pairs/s at the bench shape); when sf_step_issue deals the steps over several streams the neighbouring step fills a
// launch's tail anyway and the split form is faster (21.9 against 20.7 M pairs/s; 18.3 against 16.8 M at 40 000
// keyframes): its matching kernel keeps four "to" tiles per wavefront at three workgroups per CU.  Frames that put
// the fused kernel into its WIDE form (K = 1000), 512-bit descriptors and queries of more than 65 536 candidates
// measured equal or slower in the split form and stay fused, and so do small queries (the reference's own cadence of 20
// candidates per tick: one launch instead of three).  SF_FUSED=2 forces the split form everywhere.
static bool sf_use_split(const sf_context* c, const StoreView& v, int n) {
  if (c->split) return sf_split_applicable(c, v);
  // bundle adjustment on: the fused kernel does not apply (the adjustment is a launch of its own, the chain is cut around
  // it); the split form wherever it exists, else the stage kernels
  if (c->dparams.bundle_adjustment && c->dparams.estimation_type == 0 && c->fused) return sf_split_applicable(c, v);
  if (!c->split_auto || !c->in_overlapped_step) return false;
  if (c->dparams.estimation_type != 0 || v.w != 8 || n > 65536 || n < c->split_auto_min || !sf_split_applicable(c, v))
    return false;
  return sf_fused_lds_bytes(c, v) * 4 <= 160 * 1024;       // (not the WIDE form: sf_launch_verify_fused)
}

VerifyPlan sf_verify_plan(const sf_context* c, const StoreView& v, int n) {
  VerifyPlan p;
  // a camera id on a slot of the store (not the scratch slots of sf_estimate_transform: always id 0): the stage kernels
  // carry the per-pair camera, as they carry Vis/CorGuessMatchToProjection; the fused, split and chain forms do not
  p.cameras = v.desc != nullptr && v.desc == (const uint32_t*)c->store.desc.p && sf_camera_active(c);
  if (c->overlap && n >= c->overlap_min_pairs) { p.form = VerifyPlan::HALVES; p.lists = true; p.single = false; return p; }
  p.single = n <= SF_CHUNK;
  if (p.cameras) { p.form = VerifyPlan::STAGES; p.lists = true; return p; }
  // Vis/CorGuessMatchToProjection = true: pass 2 is k_guided_tp, a stage kernel; the fused, split and chain forms carry
  // only the other branch (guided_body) inline
  if (c->dparams.guess_match_to_projection) { p.form = VerifyPlan::STAGES; p.lists = true; return p; }
  if (c->chain_pnp && sf_split_pnp_applicable(c, v)) { p.form = VerifyPlan::SPLIT_PNP; p.lists = true; }
  else if (sf_use_split(c, v, n)) {
    p.form = VerifyPlan::SPLIT; p.lists = true;
    // (SPLIT is the 3D-3D estimator's, without Vis/CorGuessMatchToProjection; the bundle adjustment cuts the chain its own
    //  way.  With PCL's adaptive stop off every pass evaluates all its hypotheses, 64 per wavefront and round: that work is
    //  data-parallel and keeps the four-wavefront chain: docs/chain_narrow_estimates.md, "What lost".)
    p.narrow_est = c->chain_narrow_est && !c->dparams.bundle_adjustment && c->dparams.adaptive_stop != 0;
  }
  else if (sf_fused_lds_bytes(c, v) != 0 && !c->dparams.bundle_adjustment) { p.form = VerifyPlan::FUSED; p.lists = c->debug_corr; }
  else { p.form = VerifyPlan::STAGES; p.lists = true; }
  return p;
}

// What the launches of a form WRITE into the workspace for a sequence of m pairs -- stated here independently of
// ws_bytes / ws_reserve, from the kernels' own indexing (k_verify.hip, k_match.hip, k_ransac.hip, k_pnp.hip,
// k_guided.hip): lists are [pair][kcap] words, headers / states / flags one entry per pair, work lists one int per pair.
// (The `4822be5` fault of round 3 was a form that writes lists on a workspace reserved without them.)
static WsBytes form_writes(VerifyPlan::Form form, int m, int kcap, bool debug_corr, bool ba, bool narrow_est) {
  const size_t np = (size_t)m, list = np * (size_t)kcap * 4;
  WsBytes w = {};
  switch (form) {
    case VerifyPlan::FUSED:            // lists / headers / states only with SF_OPT_DEBUG_CORR; flags with it too
      if (debug_corr) { w.corr1 = w.corr2 = list; w.hdr1 = w.hdr2 = np * sizeof(CorrHeader); w.pass1 = w.pass2 = np * sizeof(PassState); w.flags = np; }
      break;
    case VerifyPlan::SPLIT:            // k_match_split: corr1, hdr1, pass1, list1 (+ hdr2 / pass2 / flags of non-survivors with
      w.corr1 = list; w.hdr1 = np * sizeof(CorrHeader); w.pass1 = np * sizeof(PassState); w.list1 = np * 4;   // the debug option)
      // (narrow_est: k_chain<.., 3> hands the second list, header, state and flag to k_chain_est<2> through the workspace)
      if (debug_corr || ba || narrow_est) { w.corr2 = list; w.hdr2 = np * sizeof(CorrHeader); w.pass2 = np * sizeof(PassState); w.flags = np; }
      break;
    case VerifyPlan::SPLIT_PNP:        // k_chain_pnp hands everything over through the workspace
    case VerifyPlan::STAGES:
    case VerifyPlan::HALVES:
      w.corr1 = w.corr2 = list; w.hdr1 = w.hdr2 = np * sizeof(CorrHeader); w.pass1 = w.pass2 = np * sizeof(PassState);
      w.list1 = w.list3 = np * 4; w.flags = np;
      break;
  }
  return w;
}

// include/sf_experimental.h: the plan of a verification call and its workspace, computed WITHOUT a device (no HIP call):
// out[0] = form, out[1] = lists, out[2] = single, out[3] = pairs of the largest launch sequence, out[4..12] = bytes
// ws_reserve reserves (corr1, corr2, hdr1, hdr2, pass1, pass2, list1, list3, flags), out[13..21] = bytes the form's
// launches write for that sequence; with n_out >= 23, out[22] = the split form's estimates run as k_chain_est (three launches).
extern "C" int sf_debug_plan_workspace(const sf_params* p, int32_t kcap, int32_t desc_words, int32_t n_pairs,
                                       int32_t in_overlapped_step, int32_t debug_corr, int64_t* out, int32_t n_out) {
  if (!p || !out || n_out < 22 || kcap <= 0 || (kcap & 63) || (desc_words != 8 && desc_words != 16 && desc_words != 64 && desc_words != 128) || n_pairs <= 0)
    return SF_EINVAL;
  sf_context* c = new (std::nothrow) sf_context();
  if (!c) return SF_ENOMEM;
  c->params = *p;
  int rc = sf_fill_device_params(c);
  if (rc == SF_OK) {
    sf_env_knobs(c);        // (what a handle created in this environment would plan)
    c->in_overlapped_step = in_overlapped_step != 0;
    c->debug_corr = debug_corr != 0;
    StoreView v = {};
    v.kcap = kcap; v.w = desc_words; v.n_slots = 1;
    const VerifyPlan plan = sf_verify_plan(c, v, n_pairs);
    const int seq = plan.form == VerifyPlan::HALVES ? std::min((std::min(n_pairs, 2 * SF_CHUNK) + 1) / 2, SF_CHUNK)
                                                    : std::min(n_pairs, SF_CHUNK);
    const bool lists = plan.form == VerifyPlan::HALVES ? true : plan.lists;
    const WsBytes r = ws_bytes(seq, kcap, lists);
    const WsBytes w = form_writes(plan.form == VerifyPlan::HALVES ? VerifyPlan::STAGES : plan.form, seq, kcap, c->debug_corr,
                                  c->dparams.bundle_adjustment != 0, plan.narrow_est);
    if (n_out >= 23) out[22] = plan.narrow_est;
    out[0] = (int64_t)plan.form; out[1] = plan.lists; out[2] = plan.single; out[3] = seq;
    for (int i = 0; i < 9; ++i) { out[4 + i] = (int64_t)(r.*WS_ROW[i]); out[13 + i] = (int64_t)(w.*WS_ROW[i]); }
  }
  delete c;
  return rc;
}

// One launch sequence for m <= SF_CHUNK pairs on the current stream and workspace, in the form the call's plan names.
static int verify_sequence(sf_context* c, const StoreView& view, const int32_t* d_from, const int32_t* d_to, int m,
                           sf_result* d_out, const VerifyPlan& plan) {
  int rc;
  c->dparams.dbg_corr = c->debug_corr ? 1 : 0;
  switch (plan.form) {
    case VerifyPlan::SPLIT_PNP:
      c->w->last_lists_valid = true;
      return sf_launch_verify_split(c, view, d_from, d_to, m, d_out);
    case VerifyPlan::SPLIT:
      // (pass-2 lists only with the option or the bundle adjustment, whose launches read them; pass-1 lists always)
      c->w->last_lists_valid = c->debug_corr || c->dparams.bundle_adjustment != 0;
      return sf_launch_verify_split(c, view, d_from, d_to, m, d_out, plan.narrow_est);
    case VerifyPlan::FUSED:
      // one launch: every pair's whole two-pass pipeline inside its workgroup (k_verify.hip); no work lists
      c->w->last_lists_valid = c->debug_corr;
      return sf_launch_verify_fused(c, view, d_from, d_to, m, d_out);
    default: break;
  }
  c->w->last_lists_valid = true;
  SF_HIP(c, hipMemsetAsync(c->w->counters.p, 0, 64, c->stream));   // work-list counters of the stage kernels
  // (the launchers of this sequence take the camera forms of their kernels iff the view names a table)
  c->cam_view = CameraView();
  if (plan.cameras) {
    c->cam_view.table = (const CameraBlock*)c->cam_table.p;
    c->cam_view.tags = (const uint8_t*)c->cam_tags_dev.p;
    c->cam_view.n_slots = std::min(view.n_slots, c->cam_dev_n);
  }
  if ((rc = sf_launch_match_global(c, view, d_from, d_to, m)) == SF_OK &&
      (rc = sf_launch_camera_gate(c, d_to, m)) == SF_OK &&
      (rc = sf_launch_estimate(c, view, d_from, d_to, m, 1)) == SF_OK &&
      (rc = sf_launch_guided(c, view, d_from, d_to, m)) == SF_OK &&
      (rc = sf_launch_estimate(c, view, d_from, d_to, m, 2)) == SF_OK)
    rc = sf_launch_finalize(c, m, d_out);
  c->cam_view = CameraView();
  return rc;
}

// The stream of the second half of the two-stream path (ws[SF_STEP_MAX_LANES]): created on first use.
static int half_create(sf_context* c) {
  Workspace& h = c->ws[SF_STEP_MAX_LANES];
  if (h.stream) return SF_OK;
  // (a lowest-priority stream was tried so that the first half would match first and its estimation kernels
  //  overlap the second half's matching: no gain -- both matching kernels still share the chip)
  SF_HIP(c, hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking));
  int rc = sf_buf_reserve(c, h.counters, 64);
  if (rc != SF_OK) return rc;
  if ((rc = sf_event_ensure(c, c->ev_fork)) != SF_OK) return rc;
  return sf_event_ensure(c, c->ev_join);
}

// d_from / d_to / d_out: device pointers. Asynchronous on the handle's stream.
//
// With SF_OVERLAP=1 batches of at least `overlap_min_pairs` pairs are cut in two halves that run the STAGE
// kernels on two streams, so that the motion-estimation kernels (a few thousand workgroups of latency-bound
// fp64 chains, issue ports idle) of one half can overlap the matching kernel (issue-bound, indifferent to
// 2 / 3 / 4 resident workgroups per CU) of the other.  Measured on the bench step (10 000 pairs): +4-6 % with
// the 3D-3D estimator, +3 % with PnP -- the two matching kernels start together and share the chip, so most
// of the estimation work still runs after both.  Off by default: one launch sequence per chunk keeps the
// per-kernel durations exclusive (what the roofline is computed from) for a gain inside the box-to-box spread.
// The second stream starts after everything already queued on the handle's stream and the handle's stream
// continues only after the second has finished, so the call keeps its single-stream semantics either way.
int sf_verify_device(sf_context* c, const Store& st, const int32_t* d_from, const int32_t* d_to, int n, sf_result* d_out,
                     const VerifyPlan* given) {
  if (n <= 0) return SF_OK;
  if (st.slots <= 0) return sf_fail(c, SF_EINVAL, "keyframe store is empty");
  const StoreView view = sf_store_view(st);
  const VerifyPlan plan = given ? *given : sf_verify_plan(c, view, n);
  int rc;
  if (plan.cameras && (rc = sf_camera_sync(c)) != SF_OK) return rc;      // the slots' camera ids, current on the device
  if (plan.form == VerifyPlan::HALVES) {
    if ((rc = half_create(c)) != SF_OK) return rc;
    Workspace& h = c->ws[SF_STEP_MAX_LANES];
    VerifyPlan stages;                                   // (two FUSED halves on two streams were measured too and gain nothing)
    stages.cameras = plan.cameras;
    const int span = std::min(n, 2 * SF_CHUNK);          // pairs per round: one chunk per stream
    const int half0 = (std::min(span, n) + 1) / 2;
    if ((rc = ws_reserve(c, std::min(half0, SF_CHUNK), st.kcap, stages.lists)) != SF_OK) return rc;
    {
      UseWorkspace on(c, h);
      if ((rc = ws_reserve(c, std::min(half0, SF_CHUNK), st.kcap, stages.lists)) != SF_OK) return rc;
    }
    SF_HIP(c, hipEventRecord(c->ev_fork, c->stream));
    SF_HIP(c, hipStreamWaitEvent(h.stream, c->ev_fork, 0));
    c->ws_split = 0;
    for (int off = 0; off < n; off += span) {
      const int m = std::min(span, n - off);
      const int ma = (m + 1) / 2, mb = m - ma;
      if (off == 0) c->ws_split = ma;
      if ((rc = verify_sequence(c, view, d_from + off, d_to + off, ma, d_out + off, stages)) != SF_OK) return rc;
      if (mb > 0) {
        UseWorkspace on(c, h);
        if ((rc = verify_sequence(c, view, d_from + off + ma, d_to + off + ma, mb, d_out + off + ma, stages)) != SF_OK) return rc;
      }
    }
    SF_HIP(c, hipEventRecord(c->ev_join, h.stream));
    SF_HIP(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return SF_OK;
  }
  if ((rc = ws_reserve(c, std::min(n, SF_CHUNK), st.kcap, plan.lists)) != SF_OK) return rc;
  c->ws_split = 0;
  for (int off = 0; off < n; off += SF_CHUNK) {
    const int m = std::min(SF_CHUNK, n - off);
    if ((rc = verify_sequence(c, view, d_from + off, d_to + off, m, d_out + off, plan)) != SF_OK) return rc;
  }
  return SF_OK;
}

extern "C" int sf_verify_pairs_device(sf_handle c, const int32_t* d_from, const int32_t* d_to, int32_t n,
                                      sf_result* d_out) {
  if (!c || n < 0 || (n > 0 && (!d_from || !d_to || !d_out))) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_verify_device(c, c->store, d_from, d_to, n, d_out);
}

extern "C" int sf_verify_matches_device(sf_handle c, const sf_match* matches, int32_t n, int32_t slot_base_other,
                                        int32_t slot_base_local, sf_result* d_out) {
  if (!c || n < 0 || (n > 0 && (!matches || !d_out))) return SF_EINVAL;
  if (n == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  int rc;
  if ((rc = sf_buf_reserve(c, c->w->pair_from, (size_t)n * 4)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->w->pair_to, (size_t)n * 4)) != SF_OK) return rc;
  // pinned staging of the two slot lists; the previous call's copies must have left it
  if (c->pairs_staged) SF_HIP(c, hipEventSynchronize(c->pairs_staged));
  const size_t need = (size_t)n * 8;
  if ((rc = sf_pinned_reserve(c, c->pairs_pinned, need, need + need / 2)) != SF_OK) return rc;
  int32_t* hf = (int32_t*)c->pairs_pinned.p;
  int32_t* ht = hf + n;
  for (int i = 0; i < n; ++i) {
    hf[i] = slot_base_other + matches[i].idx_other;   // "from" = the querying robot's frame
    ht[i] = slot_base_local + matches[i].idx_local;   // "to"   = the computing robot's frame
    if (hf[i] < 0 || hf[i] >= c->store.slots || ht[i] < 0 || ht[i] >= c->store.slots)
      return sf_fail(c, SF_ERANGE, "match %d: slot (%d,%d) outside the store (%d slots)", i, hf[i], ht[i], c->store.slots);
  }
  SF_HIP(c, hipMemcpyAsync(c->w->pair_from.p, hf, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  SF_HIP(c, hipMemcpyAsync(c->w->pair_to.p, ht, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if ((rc = sf_event_ensure(c, c->pairs_staged)) != SF_OK) return rc;
  SF_HIP(c, hipEventRecord(c->pairs_staged, c->stream));
  return sf_verify_device(c, c->store, c->w->from(), c->w->to(), n, d_out);
}

static int verify_host_indices(sf_context* c, const Store& st, const int32_t* from, const int32_t* to, int n,
                               sf_result* out) {
  if (n == 0) return SF_OK;
  for (int i = 0; i < n; ++i)
    if (from[i] < 0 || from[i] >= st.slots || to[i] < 0 || to[i] >= st.slots)
      return sf_fail(c, SF_ERANGE, "pair %d: slot (%d,%d) outside the store (%d slots)", i, from[i], to[i], st.slots);
  int rc;
  if ((rc = sf_buf_reserve(c, c->w->pair_from, (size_t)n * 4)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->w->pair_to, (size_t)n * 4)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->w->results, (size_t)n * sizeof(sf_result))) != SF_OK) return rc;
  SF_HIP(c, hipMemcpyAsync(c->w->pair_from.p, from, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  SF_HIP(c, hipMemcpyAsync(c->w->pair_to.p, to, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if ((rc = sf_verify_device(c, st, c->w->from(), c->w->to(), n, c->w->out())) != SF_OK) return rc;
  SF_HIP(c, hipMemcpyAsync(out, c->w->results.p, (size_t)n * sizeof(sf_result), hipMemcpyDeviceToHost, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));
  return SF_OK;
}

extern "C" int sf_verify_pairs(sf_handle c, const int32_t* from_slot, const int32_t* to_slot, int32_t n,
                               sf_result* out) {
  if (!c || n < 0 || (n > 0 && (!from_slot || !to_slot || !out))) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return verify_host_indices(c, c->store, from_slot, to_slot, n, out);
}

extern "C" int sf_estimate_transform_batch(sf_handle c, const sf_features* from, const sf_features* to,
                                           int32_t n, sf_result* out) {
  if (!c || n < 0 || (n > 0 && (!from || !to || !out))) return SF_EINVAL;
  if (n == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  int rc;
  for (int i = 0; i < n; ++i) {
    if ((rc = sf_validate_features(c, from + i)) != SF_OK) return rc;
    if ((rc = sf_validate_features(c, to + i)) != SF_OK) return rc;
    if (from[i].rows > 0 && to[i].rows > 0 && from[i].cols != to[i].cols)
      return sf_fail(c, SF_EINVAL, "pair %d: descriptor widths differ (%d vs %d; myRegistrationVis.cpp:683)", i,
                     (int)from[i].cols, (int)to[i].cols);
  }
  SF_HIP(c, hipStreamSynchronize(c->stream));
  c->scratch.slots = 0;
  std::vector<int32_t> fi(n), ti(n);
  std::vector<const sf_features*> all(2 * (size_t)n);
  for (int i = 0; i < n; ++i) { all[2 * i] = from + i; all[2 * i + 1] = to + i; }
  int first = 0;
  if ((rc = sf_store_add_host_batch(c, c->scratch, all.data(), 2 * n, &first)) != SF_OK) return rc;
  for (int i = 0; i < n; ++i) { fi[i] = first + 2 * i; ti[i] = first + 2 * i + 1; }
  return verify_host_indices(c, c->scratch, fi.data(), ti.data(), n, out);
}

extern "C" int sf_estimate_transform(sf_handle c, const sf_features* from, const sf_features* to, sf_result* out) {
  return sf_estimate_transform_batch(c, from, to, 1, out);
}

namespace {

// Ordered compaction of the accepted results, 1024 candidates per workgroup: k_compact_count leaves the
// number of accepted candidates of every chunk (and the per-candidate flags), k_compact_move lets each
// workgroup sum the counts of the chunks before it (at most a few hundred values) and moves its records
// as 23 x 16 bytes each, consecutive threads taking consecutive pieces.
__global__ void __launch_bounds__(1024)
k_compact_count(const sf_result* __restrict__ res, int n, uint8_t* __restrict__ flags, int32_t* __restrict__ chunk_count) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x * 1024 + tid;
  const bool ok = i < n && res[i].success != 0;
  if (i < n && flags) flags[i] = ok ? 1 : 0;
  const unsigned long long bal = __ballot(ok);
  if (lane == 0) wsum[wave] = __popcll(bal);
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += wsum[w];
    chunk_count[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(1024)
k_compact_move(const sf_result* __restrict__ res, int n, sf_result* __restrict__ acc,
               const int32_t* __restrict__ chunk_count, int32_t* __restrict__ total) {
  __shared__ int wsum[16];
  __shared__ int s_dst[1024];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = blockIdx.x * 1024;
  // offset of this chunk = accepted candidates of all earlier chunks
  int part = 0;
  for (int b = tid; b < (int)blockIdx.x; b += 1024) part += chunk_count[b];
  for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
  if (lane == 0) wsum[wave] = part;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += wsum[w];
    s_base = t;
    if (blockIdx.x == gridDim.x - 1) *total = t + chunk_count[blockIdx.x];
  }
  __syncthreads();
  const int i = base + tid;
  const bool ok = i < n && res[i].success != 0;
  const unsigned long long bal = __ballot(ok);
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __popcll(bal);
  __syncthreads();
  int woff = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) woff += (w < wave) ? wsum[w] : 0;
  s_dst[tid] = ok ? s_base + woff + before : -1;
  __syncthreads();
  const int m = min(1024, n - base);
  for (int e = tid; e < m * 23; e += 1024) {
    const int c = e / 23, piece = e - c * 23;
    const int dst = s_dst[c];
    if (dst >= 0) reinterpret_cast<uint4*>(acc + dst)[piece] = reinterpret_cast<const uint4*>(res + base + c)[piece];
  }
}

}  // namespace

// The two compaction kernels, asynchronous: the number of accepted results is left at d_count (device).
// Ordered compaction in ONE launch: a chunk of 256 candidates per workgroup; every chunk publishes its own number of
// accepted candidates as {epoch, count} and sums the counts of the chunks before it (all chunks are resident -- at
// most 1024 of 256 threads -- and a chunk only ever waits for earlier ones).  The epoch (one per launch, kept by the
// handle) makes stale entries of the previous launch unreadable without a memset in between.  Replaces
// k_compact_count + k_compact_move (kept for batches with more chunks than can be resident at once).
constexpr int COMPACT_CHUNK = 256;        // records per workgroup of k_compact_chain
constexpr int COMPACT_MAX_CHUNKS = 1024;  // all resident at once (256 CUs x 8 workgroups of 256 threads)
// state[0 .. chunks): the chunks' {epoch, own count}; state[chunks]: the launch's arrival word {arrived:16, timed out:16,
// sum:32}, zero between launches (the chunk that arrives last reads the total, publishes it and clears the word).
// cap2: record slots behind acc2 (a mirror smaller than the batch: what does not fit is dropped THERE only and shows in
// *total2, which still carries the full count -- the owner's overflow path)
__global__ void __launch_bounds__(COMPACT_CHUNK)
k_compact_chain(const sf_result* __restrict__ res, const int32_t* __restrict__ index, int n, sf_result* __restrict__ acc,
                uint8_t* __restrict__ flags, unsigned long long* __restrict__ state, unsigned epoch,
                int32_t* __restrict__ total, sf_result* __restrict__ acc2, uint8_t* __restrict__ flags2,
                int32_t* __restrict__ total2, int cap2) {
  __shared__ int wsum[COMPACT_CHUNK / 64];
  __shared__ int s_dst[COMPACT_CHUNK];
  __shared__ int s_src[COMPACT_CHUNK];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = blockIdx.x * COMPACT_CHUNK;
  const int i = base + tid;
  const int src = i < n ? (index ? index[i] : i) : 0;      // candidate i's record (index: e.g. its speculative slot)
  s_src[tid] = src;
  const bool ok = i < n && res[src].success != 0;
  if (i < n && flags) flags[i] = ok ? 1 : 0;
  if (i < n && flags2) flags2[i] = ok ? 1 : 0;
  const unsigned long long bal = __ballot(ok);
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wave] = __popcll(bal);
  __syncthreads();
  int woff = 0, own = 0;
#pragma unroll
  for (int w = 0; w < COMPACT_CHUNK / 64; ++w) { woff += (w < wave) ? wsum[w] : 0; own += wsum[w]; }
  // every chunk publishes its OWN count at once (tagged with the launch's epoch) and sums its predecessors' -- two
  // hops however many chunks there are, where a chain of inclusive prefixes costs one per chunk; the word itself is
  // the message, so relaxed agent-scope accesses do and no cache is flushed between XCDs
  if (tid == 0)
    __hip_atomic_store(&state[blockIdx.x], ((unsigned long long)epoch << 32) | (unsigned long long)(unsigned)own,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (wave == 0) {
    // (the look-back assumes every earlier chunk gets to run: at most COMPACT_MAX_CHUNKS workgroups, all resident.  It
    //  is bounded all the same -- about a second of polling -- so that a launch whose earlier chunks never start, for
    //  whatever reason, ends with the count -1 (the host reports SF_EHIP) instead of spinning forever)
    unsigned sum = 0;
    bool timed_out = false;
    for (int j = lane; j < (int)blockIdx.x; j += 64) {
      unsigned long long v;
      unsigned spins = 0;
      do {
        v = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)(v >> 32) == epoch) break;
        __builtin_amdgcn_s_sleep(8);
      } while (++spins < (1u << 22));
      timed_out = timed_out || (unsigned)(v >> 32) != epoch;
      sum += (unsigned)v;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    const bool any_timeout = __any(timed_out);
    if (lane == 0) {
      s_base = (int)sum;
      // the total is published by whichever chunk ARRIVES last, and a time-out anywhere in the launch makes it -1: a
      // chunk that gave up on a predecessor has moved its records to wrong places whatever the other chunks saw
      const unsigned long long mine = (1ull << 48) | ((unsigned long long)(any_timeout ? 1u : 0u) << 32) |
                                      (unsigned long long)(unsigned)own;
      const unsigned long long old = atomicAdd(&state[gridDim.x], mine);
      if ((unsigned)(old >> 48) + 1u == gridDim.x) {
        const unsigned long long tot = old + mine;
        const int t = ((tot >> 32) & 0xFFFFull) ? -1 : (int)(unsigned)(tot & 0xFFFFFFFFull);
        *total = t;
        if (total2) *total2 = t;
        __hip_atomic_store(&state[gridDim.x], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  __syncthreads();
  s_dst[tid] = ok ? s_base + woff + before : -1;
  __syncthreads();
  const int m = min(COMPACT_CHUNK, n - base);
  for (int e = tid; e < m * 23; e += COMPACT_CHUNK) {
    const int c = e / 23, piece = e - c * 23;
    const int dst = s_dst[c];
    if (dst >= 0) {
      const uint4 v = reinterpret_cast<const uint4*>(res + s_src[c])[piece];
      reinterpret_cast<uint4*>(acc + dst)[piece] = v;
      if (acc2 && dst < cap2) reinterpret_cast<uint4*>(acc2 + dst)[piece] = v;
    }
  }
}

int sf_compact_launch(sf_context* c, const sf_result* d_results, int n, sf_result* d_accepted, uint8_t* d_flags,
                      int32_t* d_count, const int32_t* index, sf_result* d_accepted2, uint8_t* d_flags2, int32_t* d_count2,
                      int cap2) {
  const int chunks = (n + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
  int rc;
  if ((rc = sf_buf_reserve(c, c->w->compact_scratch, (size_t)(chunks + 2) * 8)) != SF_OK) return rc;
  if (chunks <= COMPACT_MAX_CHUNKS) {
    if (c->w->compact_state_chunks != chunks || c->w->compact_state_ptr != c->w->compact_scratch.p) {
      // fresh (or regrown / reallocated) state, or another chunk count (the arrival word sits behind the chunks' words):
      // make every epoch tag invalid and the arrival word zero once
      SF_HIP(c, hipMemsetAsync(c->w->compact_scratch.p, 0, (size_t)(chunks + 2) * 8, c->stream));
      c->w->compact_state_chunks = chunks;
      c->w->compact_state_ptr = c->w->compact_scratch.p;
    }
    if (++c->w->compact_epoch == 0) c->w->compact_epoch = 1;
    hipLaunchKernelGGL(k_compact_chain, dim3(chunks), dim3(COMPACT_CHUNK), 0, c->stream, d_results, index, n, d_accepted, d_flags,
                       (unsigned long long*)c->w->compact_scratch.p, c->w->compact_epoch, d_count, d_accepted2, d_flags2, d_count2, cap2);
    SF_HIP(c, hipGetLastError());
    if (index && index == (const int32_t*)c->spec_index_pinned.p)
      SF_HIP(c, hipEventRecord(c->spec_index_staged, c->stream));   // the pinned index block may be rewritten after this
    return SF_OK;
  }
  if (index || d_accepted2) return sf_fail(c, SF_ERANGE, "indexed / mirrored compaction of %d records: more than %d chunks", n, COMPACT_MAX_CHUNKS);
  c->w->compact_state_chunks = 0;                  // (the two-kernel form reuses the buffer as plain counts)
  int32_t* d_chunk = (int32_t*)c->w->compact_scratch.p;
  const int chunks2 = (n + 1023) / 1024;
  hipLaunchKernelGGL(k_compact_count, dim3(chunks2), dim3(1024), 0, c->stream, d_results, n, d_flags, d_chunk);
  hipLaunchKernelGGL(k_compact_move, dim3(chunks2), dim3(1024), 0, c->stream, d_results, n, d_accepted,
                     (const int32_t*)d_chunk, d_count);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

extern "C" int sf_compact_accepted_device_async(sf_handle c, const sf_result* d_results, int32_t n,
                                                sf_result* d_accepted, uint8_t* d_flags, int32_t* d_n_accepted) {
  if (!c || n < 0 || !d_n_accepted || (n > 0 && (!d_results || !d_accepted))) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  if (n == 0) {
    SF_HIP(c, hipMemsetAsync(d_n_accepted, 0, 4, c->stream));
    return SF_OK;
  }
  return sf_compact_launch(c, d_results, n, d_accepted, d_flags, d_n_accepted);
}

extern "C" int sf_compact_accepted_indexed_device_async(sf_handle c, const sf_result* d_results, const int32_t* index,
                                                        int32_t n, sf_result* d_accepted, uint8_t* d_flags,
                                                        int32_t* d_n_accepted) {
  if (!c || n < 0 || !d_n_accepted || (n > 0 && (!d_results || !d_accepted))) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  if (n == 0) {
    SF_HIP(c, hipMemsetAsync(d_n_accepted, 0, 4, c->stream));
    return SF_OK;
  }
  return sf_compact_launch(c, d_results, n, d_accepted, d_flags, d_n_accepted, index);
}

extern "C" int sf_compact_accepted_indexed_mirrored_device_async(sf_handle c, const sf_result* d_results,
                                                                 const int32_t* index, int32_t n, sf_result* d_accepted,
                                                                 uint8_t* d_flags, int32_t* d_n_accepted,
                                                                 sf_result* d_accepted2, uint8_t* d_flags2,
                                                                 int32_t* d_n_accepted2) {
  if (!c || n < 0 || !d_n_accepted || !d_n_accepted2 || (n > 0 && (!d_results || !d_accepted || !d_accepted2))) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  if (n == 0) {
    SF_HIP(c, hipMemsetAsync(d_n_accepted, 0, 4, c->stream));
    SF_HIP(c, hipMemsetAsync(d_n_accepted2, 0, 4, c->stream));
    return SF_OK;
  }
  return sf_compact_launch(c, d_results, n, d_accepted, d_flags, d_n_accepted, index, d_accepted2, d_flags2, d_n_accepted2);
}

extern "C" int sf_compact_accepted_device(sf_handle c, const sf_result* d_results, int32_t n, sf_result* d_accepted,
                                          uint8_t* d_flags, int32_t* n_accepted) {
  if (!c || n < 0 || !n_accepted || (n > 0 && (!d_results || !d_accepted))) return SF_EINVAL;
  *n_accepted = 0;
  if (n == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  const int chunks = (n + COMPACT_CHUNK - 1) / COMPACT_CHUNK;
  int rc;
  if ((rc = sf_buf_reserve(c, c->w->compact_scratch, (size_t)(chunks + 2) * 8)) != SF_OK) return rc;
  int32_t* d_count = (int32_t*)((char*)c->w->compact_scratch.p + (size_t)(chunks + 1) * 8);   // behind the chunk states
  if ((rc = sf_compact_launch(c, d_results, n, d_accepted, d_flags, d_count)) != SF_OK) return rc;
  if ((rc = sf_pinned_reserve(c, c->count_pinned, 64, 64)) != SF_OK) return rc;
  const int32_t* count = (const int32_t*)c->count_pinned.p;
  SF_HIP(c, hipMemcpyAsync(c->count_pinned.p, d_count, 4, hipMemcpyDeviceToHost, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));
  if (*count < 0) return sf_fail(c, SF_EHIP, "ordered compaction: the look-back over earlier chunks timed out");
  *n_accepted = *count;
  return SF_OK;
}

// The workspace pair `pair` of the last verification lives in, and its index there (the second half of a two-stream
// batch has one of its own)
static const Workspace& debug_workspace(const sf_context* c, int32_t* pair) {
  if (c->ws_split > 0 && *pair >= c->ws_split) {
    *pair -= c->ws_split;
    return c->ws[SF_STEP_MAX_LANES];
  }
  return *c->w;
}

extern "C" int sf_debug_correspondences(sf_handle c, int32_t pair, int32_t pass, uint16_t* from_idx,
                                        uint16_t* to_idx, int32_t cap, int32_t* n_out) {
  if (!c || !n_out || pair < 0 || (pass != 1 && pass != 2)) return SF_EINVAL;
  SF_HIP(c, hipStreamSynchronize(c->stream));
  const Workspace& w = debug_workspace(c, &pair);
  if (pair >= w.ws_pairs) return SF_EINVAL;
  if (!w.last_lists_valid)
    return sf_fail(c, SF_EINVAL, "the fused kernel keeps correspondence lists in LDS: set SF_OPT_DEBUG_CORR (or "
                                 "SF_DEBUG_CORR=1) before the verification call");
  CorrHeader h;
  SF_HIP(c, hipMemcpy(&h, w.hdr(pass) + pair, sizeof(h), hipMemcpyDeviceToHost));
  int n = std::min(h.n_corr, cap);
  std::vector<uint32_t> tmp(std::max(n, 1));
  if (n > 0) SF_HIP(c, hipMemcpy(tmp.data(), w.corr(pass) + (size_t)pair * w.ws_kcap, (size_t)n * 4, hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) {
    if (from_idx) from_idx[i] = (uint16_t)(tmp[i] & 0xFFFFu);
    if (to_idx) to_idx[i] = (uint16_t)(tmp[i] >> 16);
  }
  *n_out = h.n_corr;
  return SF_OK;
}

// Pass state of pair `pair` of the LAST verification (diagnostics; needs SF_OPT_DEBUG_CORR like the lists): the pass's
// pose (row-major 3 x 4, p_from = T p_to, all zero when null), is_null / inliers / matches.
extern "C" int sf_debug_pass_state(sf_handle c, int32_t pair, int32_t pass, float* T12, int32_t* is_null, int32_t* inliers,
                                   int32_t* matches) {
  if (!c || pair < 0 || (pass != 1 && pass != 2)) return SF_EINVAL;
  SF_HIP(c, hipStreamSynchronize(c->stream));
  const Workspace& w = debug_workspace(c, &pair);
  if (pair >= w.ws_pairs) return SF_EINVAL;
  if (!w.last_lists_valid) return sf_fail(c, SF_EINVAL, "set SF_OPT_DEBUG_CORR before the verification call");
  PassState ps;
  SF_HIP(c, hipMemcpy(&ps, w.pass(pass) + pair, sizeof(ps), hipMemcpyDeviceToHost));
  if (T12) memcpy(T12, ps.T, sizeof(ps.T));
  if (is_null) *is_null = ps.is_null;
  if (inliers) *inliers = ps.inliers;
  if (matches) *matches = ps.matches;
  return SF_OK;
}

extern "C" int sf_debug_counters(sf_handle c, unsigned long long* out, int32_t n) {
  if (!c || !out || n < 0) return SF_EINVAL;
  memset(out, 0, (size_t)n * 8);
  if (!c->trace.p) return SF_OK;
  SF_HIP(c, hipStreamSynchronize(c->stream));
  if ((size_t)n * 8 > c->trace.bytes) return SF_ERANGE;
  SF_HIP(c, hipMemcpy(out, c->trace.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return SF_OK;
}
// (experiment) per-point records of the guided pass of pair `pair` of the last verification: two planes of kcap words
extern "C" int sf_debug_guided_points(sf_handle c, int32_t pair, unsigned long long* plane0, unsigned long long* plane1,
                                      int32_t* kcap_out) {
  if (!c || pair < 0 || pair >= c->w->ws_pairs || !c->trace.p) return SF_EINVAL;
  SF_HIP(c, hipStreamSynchronize(c->stream));
  const size_t k = (size_t)c->w->ws_kcap, np = (size_t)c->w->ws_pairs;
  if (c->trace.bytes < 4096 + 2 * np * k * 8) return SF_EINVAL;
  const char* base = (const char*)c->trace.p + 4096;
  SF_HIP(c, hipMemcpy(plane0, base + ((size_t)pair * k) * 8, k * 8, hipMemcpyDeviceToHost));
  SF_HIP(c, hipMemcpy(plane1, base + ((np + (size_t)pair) * k) * 8, k * 8, hipMemcpyDeviceToHost));
  if (kcap_out) *kcap_out = (int32_t)k;
  return SF_OK;
}

#ifdef SF_CHAIN_TRACE
// diagnostic build only: phase timestamps of the last verification ([n][32] uint64, 100 MHz ticks)
extern "C" int sf_debug_chain_trace(sf_handle c, unsigned long long* out, int32_t n) {
  if (!c || !out || n < 0 || n > c->w->ws_pairs) return SF_EINVAL;
  SF_HIP(c, hipStreamSynchronize(c->stream));
  SF_HIP(c, hipMemcpy(out, c->trace.p, (size_t)n * SF_TRACE_SLOTS * 8, hipMemcpyDeviceToHost));
  return SF_OK;
}
#endif
