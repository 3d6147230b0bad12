// sf_step.hip -- queries that verify what the NN stage finds: the speculation hook and the accepted-result stream,
// sf_find_matches_and_verify_device, the step ring (sf_step_issue / sf_step_retire and its lanes), the sf_nn_* entry points.
#include "sf_host.hpp"

namespace {

// Speculative verification (sf_find_matches_and_verify_device): candidate i of the NN filter, (local row r,
// received column c), becomes pair slot i = (slot_other + c, slot_local + r); slots past the candidate count
// (and candidates outside the store) get -1, which every verification kernel answers with a null result.
__global__ void __launch_bounds__(256)
k_spec_pairs(const uint2* __restrict__ cand, const unsigned* __restrict__ count, unsigned grid, int n_l, int n_r,
             int slot_other, int slot_local, int n_slots, int32_t* __restrict__ from, int32_t* __restrict__ to) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= grid) return;
  int f = -1, t = -1;
  if (i < *count) {
    const uint2 rc = cand[i];
    if ((int)rc.x < n_l && (int)rc.y < n_r) {
      f = slot_other + (int)rc.y;
      t = slot_local + (int)rc.x;
      if ((unsigned)f >= (unsigned)n_slots || (unsigned)t >= (unsigned)n_slots) { f = -1; t = -1; }
    }
  }
  from[i] = f;
  to[i] = t;
}

// out[m] = spec[index[m]]: the results of the walk's matches, in walk order (23 x 16 bytes per record)
__global__ void __launch_bounds__(256)
k_spec_gather(const sf_result* __restrict__ spec, const int32_t* __restrict__ index, int n, sf_result* __restrict__ out) {
  static_assert(sizeof(sf_result) % 16 == 0, "sf_result is moved in 16-byte pieces");
  constexpr int PIECES = sizeof(sf_result) / 16;
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int m = g / PIECES, piece = g % PIECES;
  if (m >= n) return;
  const uint4* src = reinterpret_cast<const uint4*>(spec + index[m]);
  reinterpret_cast<uint4*>(out + m)[piece] = src[piece];
}

}  // namespace

// Called by the NN filter behind the refinement launch of a prefix level (k_nn.hip): candidate pair list on
// the device, then the verification of every candidate slot, all on the handle's stream.
// Hands the selected accepted-result block to the verification kernels of the launch that follows (fused kernel, chain
// kernels) -- by value, in their kernel arguments: the counter is word 4 of the candidate list's header, zeroed with the
// candidate count before the filter ran (or the caller's own word).
static int arm_accept_stream(sf_context* c, const unsigned* d_count) {
  c->accept_streamed = false;
  if (c->accept_sel < 0 || !c->accept_blocks[c->accept_sel].set) return SF_OK;
  sf_context::AcceptHost& ab = c->accept_blocks[c->accept_sel];
  // Every verified slot may be accepted: a block with fewer record slots than the launch has pairs could lose
  // records (the kernel drops what does not fit and the slot counter is not the caller's to read), so such a block
  // is not armed -- sf_accept_stream_status then reports streamed = 0 and the caller takes the compaction.
  if ((unsigned)ab.s.cap < c->spec.grid) return SF_OK;
  c->dparams.accept = ab.s;
  if (!ab.s.ext_counter) c->dparams.accept.counter = const_cast<unsigned*>(d_count) + 4;
  c->dparams.accept_on = 1;
  c->accept_streamed = true;
  c->accept_armed = true;
  return SF_OK;
}

// The verification of `grid` pair slots taken from a (row, column) list on the device -- the NN filter's candidates
// (speculative path) or the device walk's matches -- with the accepted-result stream armed where the launch form has it.
int sf_spec_launch(sf_context* c, const void* d_cand, const unsigned* d_count) {
  const unsigned grid = c->spec.grid;
  if (c->store.slots <= 0) return sf_fail(c, SF_EINVAL, "keyframe store is empty");
  const StoreView view = sf_store_view(c->store);
  const VerifyPlan plan = sf_verify_plan(c, view, (int)grid);
  int rc = SF_OK;
  if (plan.form == VerifyPlan::FUSED && plan.single) {
    // one chunk on the fused kernel: it derives the pairs from the list itself (one launch and its gap less between
    // the NN stage and the verification)
    c->pair_src.cand = (const uint2*)d_cand;
    c->pair_src.count = d_count;
    c->pair_src.n_l = c->nn_local.n; c->pair_src.n_r = c->nn_recv.n;
    c->pair_src.slot_other = c->spec.slot_other; c->pair_src.slot_local = c->spec.slot_local;
    c->pair_src.n_slots = c->store.slots;
  } else {
    hipLaunchKernelGGL(k_spec_pairs, dim3((grid + 255) / 256), dim3(256), 0, c->stream, (const uint2*)d_cand, d_count, grid,
                       c->nn_local.n, c->nn_recv.n, c->spec.slot_other, c->spec.slot_local, c->store.slots,
                       (int32_t*)c->w->spec_from.p, (int32_t*)c->w->spec_to.p);
    SF_HIP(c, hipGetLastError());
  }
  // (one chunk, one stream: a pair's index is its slot in the list -- the fused kernel, the 3D-3D chain kernel of the
  //  split form and the PnP estimator's chain kernel stream their accepted results)
  if (plan.streams()) rc = arm_accept_stream(c, d_count);
  if (rc == SF_OK)
    rc = sf_verify_device(c, c->store, (const int32_t*)c->w->spec_from.p, (const int32_t*)c->w->spec_to.p, (int)grid,
                       (sf_result*)c->w->spec_results.p, &plan);
  c->dparams.accept_on = 0;
  c->pair_src = PairSource();
  return rc;
}

// Pair slots of a speculative verification over n_l local rows: room for rows with more than one candidate.  The step's
// block, the plan of a device step and arm_accept_stream's capacity check all count on this one figure.
static inline unsigned spec_grid(int n_l) { return (unsigned)(n_l + n_l / 8 + 256); }

// `grid` pair slots for the next sf_spec_launch on the current workspace, their rows and columns offset into the store
static int spec_reserve(sf_context* c, unsigned grid, int32_t slot_other, int32_t slot_local) {
  int rc;
  c->spec.grid = grid;
  c->spec.slot_other = slot_other;
  c->spec.slot_local = slot_local;
  if ((rc = sf_buf_reserve(c, c->w->spec_from, (size_t)grid * 4)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->w->spec_to, (size_t)grid * 4)) != SF_OK) return rc;
  return sf_buf_reserve(c, c->w->spec_results, (size_t)grid * sizeof(sf_result));
}

extern "C" int sf_find_matches_and_verify_device(sf_handle c, int32_t slot_base_other, int32_t slot_base_local,
                                                 sf_match* out, int32_t cap, int32_t* n_out, sf_result* d_out) {
  if (!c || !n_out || cap < 0 || (cap > 0 && !out)) return SF_EINVAL;
  *n_out = 0;
  c->last_results = nullptr; c->last_results_index = nullptr; c->last_results_n = 0;
  c->accept_streamed = false;
  c->accept_armed = false;
  if (c->nn_local.n <= 0 || c->nn_recv.n <= 0)
    return sf_fail(c, SF_EINVAL, "empty descriptor database (data_handler.py:308 guards this case)");
  SF_HIP(c, hipSetDevice(c->device));
  const int n_l = c->nn_local.n;
  int rc;
  // Speculate only when the walk may return (almost) every local row -- otherwise verifying every candidate
  // would do far more work than the few matches need -- and on the filter path, which has a candidate list.
  const bool speculate = c->params.nn_precision == 1 && c->store.slots > 0 &&
                         std::min(cap, c->params.netvlad_max_matches_nb) >= n_l && getenv("SF_SPECULATE_OFF") == nullptr;
  if (speculate) {
    if (!c->spec.copy_stream) {
      if ((rc = sf_side_stream(c, SF_STREAM_COPY, 0, &c->spec.copy_stream)) != SF_OK) return rc;
      for (Event* ev : {&c->spec.ev_refined, &c->spec.ev_copied, &c->spec_index_staged})
        if ((rc = sf_event_ensure(c, *ev)) != SF_OK) return rc;
    }
    if ((rc = spec_reserve(c, spec_grid(n_l), slot_base_other, slot_base_local)) != SF_OK) return rc;
  }
  c->spec.requested = speculate;
  c->spec.launched = false;
  c->spec.valid = false;
  rc = sf_nn_run(c, out, cap, n_out);
  c->spec.requested = false;
  if (rc != SF_OK) return rc;
  const int n = *n_out;
  if (n == 0) return SF_OK;
  if (!(c->spec.launched && c->spec.valid)) {
    // no speculation, or its candidate set was not the one the matches came from: verify the matches now
    // (a wasted speculative verification, if any, is simply queued in front -- what it streamed into the selected
    //  accepted-result block is not this query's answer: streamed = 0, the block's owner resets it)
    c->accept_streamed = false;
    if (!d_out) {       // the caller only wants sf_last_match_results: an internal block takes the results
      if ((rc = sf_buf_reserve(c, c->w->results, (size_t)n * sizeof(sf_result))) != SF_OK) return rc;
      d_out = c->w->out();
    }
    if ((rc = sf_verify_matches_device(c, out, n, slot_base_other, slot_base_local, d_out)) != SF_OK) return rc;
    c->last_results = d_out; c->last_results_index = nullptr; c->last_results_n = n;
    return SF_OK;
  }
  // the matches' results are among the speculative ones: index of each match's candidate, then one gather
  for (int i = 0; i < n; ++i) {
    const int f = slot_base_other + out[i].idx_other, t = slot_base_local + out[i].idx_local;
    if (f < 0 || f >= c->store.slots || t < 0 || t >= c->store.slots)
      return sf_fail(c, SF_ERANGE, "match %d: slot (%d,%d) outside the store (%d slots)", i, f, t, c->store.slots);
  }
  SF_HIP(c, hipEventSynchronize(c->spec_index_staged));   // (never recorded: returns at once) previous upload done
  const size_t need = (size_t)n * 4;
  if ((rc = sf_pinned_reserve(c, c->spec_index_pinned, need, need + need / 2)) != SF_OK) return rc;
  int32_t* hi = (int32_t*)c->spec_index_pinned.p;
  for (int i = 0; i < n; ++i) {
    const int ci = c->last_row_cand[out[i].idx_local];
    if (ci < 0 || (unsigned)ci >= c->spec.grid) return sf_fail(c, SF_EHIP, "speculation: match %d has no candidate slot", i);
    hi[i] = ci;
  }
  // The gather reads the index list straight from the pinned host block (40 KB over PCIe inside the kernel): an
  // H2D copy queued on the handle's stream would run AFTER the verification it sits behind -- ~15 us of copy
  // engine latency on the step's critical path for nothing.
  c->last_results = (const sf_result*)c->w->spec_results.p; c->last_results_index = hi; c->last_results_n = n;
  if (!d_out) return SF_OK;       // no gathered copy wanted: sf_last_match_results + an indexed consumer
  constexpr int PIECES = sizeof(sf_result) / 16;
  hipLaunchKernelGGL(k_spec_gather, dim3(((size_t)n * PIECES + 255) / 256), dim3(256), 0, c->stream,
                     (const sf_result*)c->w->spec_results.p, (const int32_t*)hi, n, d_out);
  SF_HIP(c, hipGetLastError());
  SF_HIP(c, hipEventRecord(c->spec_index_staged, c->stream));   // the block may be rewritten after this
  return SF_OK;
}

extern "C" int sf_accept_stream_set(sf_handle c, int32_t which, sf_result* records, int32_t* index, uint8_t* flags,
                                    int32_t cap, sf_result* d_records2, uint32_t* d_counter) {
  if (!c || which < 0 || which > 1) return SF_EINVAL;
  if (!records || !index || cap < 1) { c->accept_blocks[which] = sf_context::AcceptHost(); return SF_OK; }   // (unregister)
  sf_context::AcceptHost& ab = c->accept_blocks[which];
  ab.s.records = records; ab.s.index = index; ab.s.flags = flags; ab.s.cap = cap;
  ab.s.records2 = d_records2;
  ab.s.counter = d_counter; ab.s.ext_counter = d_counter ? 1 : 0;
  ab.set = true;
  return SF_OK;
}

extern "C" int sf_accept_stream_select(sf_handle c, int32_t which) {
  if (!c || which < -1 || which > 1) return SF_EINVAL;
  c->accept_sel = which;
  return SF_OK;
}

extern "C" int sf_accept_stream_status(sf_handle c, int32_t* streamed, int32_t* pairs) {
  if (!c || !streamed) return SF_EINVAL;
  *streamed = c->accept_streamed ? 1 : 0;
  if (pairs) *pairs = c->accept_streamed ? (int32_t)c->spec.grid : 0;
  return SF_OK;
}

// ---- the caller's loop body as a begin / retire pair (find_separators.py:59-133) -------------------------------------
// sf_step_issue = s_find_matches_query + the estimate_transformation calls of every returned candidate, QUEUED;
// sf_step_retire = the per-candidate outcome the loop forwards (find_separators.py:97-133).
//
// Round 4: the step is device-resident.  sf_step_issue queues, on ONE stream and with no host wait,
//     NN filter (or fp32 ranking) -> exact re-evaluation -> per-row minima -> argsort + walk (k_walk_*: data_handler.py:
//     191-205) -> verification of the walk's matches, taken from the device list -> accepted separators streaming
//     into the step's host-pinned block,
// and returns; up to `step_depth` steps are in flight, dealt over `step_lanes` streams, and sf_step_retire is the only
// wait.  (Round 3 waited inside sf_step_issue for the row minima and walked them on the host, with the verification of
// EVERY filter candidate running speculatively beside it: any host hiccup landed in the step time -- one 6.9 ms step of
// 20 halved the driver's figure.)  What the device cannot decide -- a candidate set denser than the filter level the handle
// last settled on allows, which takes the prefix ladder of nn_run_filter -- is reported through the pinned status word; the
// retire then runs the query again on the synchronous path below (step_issue_sync: round 3's body), once, and the ladder
// level it settles on serves the following steps.
static int step_block_reserve(sf_context* c, sf_context::StepBlock& b, int32_t cap) {
  int rc = sf_event_ensure(c, b.done);
  if (rc != SF_OK) return rc;
  if (cap <= b.cap) return SF_OK;
  b.cap = 0;
  const int32_t want = cap + cap / 4 + 64;
  const size_t rec_bytes = (size_t)want * sizeof(sf_result);
  const size_t idx_off = rec_bytes, flag_off = idx_off + (size_t)want * 4, cnt_off = (flag_off + (size_t)want + 63) & ~(size_t)63;
  const size_t match_off = cnt_off + 64, slot_off = match_off + (size_t)want * sizeof(sf_match);
  const size_t word_off = (slot_off + (size_t)want * 4 + 63) & ~(size_t)63;
  const size_t total = word_off + 64;
  sf_pinned_free(b.pinned);                 // (a larger cap: the block is replaced, by one of exactly `total` bytes)
  if ((rc = sf_pinned_reserve(c, b.pinned, total, total)) != SF_OK) return rc;
  char* base = (char*)b.pinned.p;
  b.records = (sf_result*)base;
  b.index = (int32_t*)(base + idx_off);
  b.flags = (uint8_t*)base + flag_off;
  b.count = (int32_t*)(base + cnt_off);
  b.walk_matches = (sf_match*)(base + match_off);
  b.walk_slots = (int32_t*)(base + slot_off);
  b.walk_n = (int32_t*)(base + word_off);
  b.walk_status = b.walk_n + 1;
  b.cap = want;
  for (int32_t i = 0; i < want; ++i) b.index[i] = -1;
  memset(b.flags, 0, (size_t)want);
  *b.count = 0;
  *b.walk_n = 0;
  *b.walk_status = 0;
  if ((rc = sf_buf_reserve(c, b.dev, 64 + (size_t)want * 8)) != SF_OK) return rc;
  return sf_buf_reserve(c, b.dev_records, (size_t)want * sizeof(sf_result));
}

// The block of the step issued `back` steps ago (0: the block the next step will use) in the ring of step_depth + 1
static sf_context::StepBlock& step_block(sf_context* c, int back) {
  return c->step_blocks[(c->step_seq - (uint64_t)back) % (uint64_t)(c->step_depth + 1)];
}

// The second (device) destination of a step's accepted records: the caller's mirror of the step's parity, else the
// block's own device buffer
struct StepMirror { sf_result* rec; uint32_t* cnt; int32_t cap; };

// Makes block `b` the step pair's own accepted-result block (accept_blocks[2]) and returns its mirror
static StepMirror step_accept_block(sf_context* c, sf_context::StepBlock& b) {
  StepMirror m;
  m.rec = c->step_mirror_records[b.parity];
  m.cnt = c->step_mirror_counter[b.parity];
  m.cap = m.rec ? c->step_mirror_cap : b.cap;
  // no caller mirror: every accepted record also lands in the block's own device buffer (sf_step_result.d_records), so
  // that a multi-GPU host can hand a RETIRED step's separators to its collective without tying buffers to steps in flight
  if (!m.rec) m.rec = (sf_result*)b.dev_records.p;
  sf_context::AcceptHost& ab = c->accept_blocks[2];
  ab.s.records = b.records; ab.s.index = b.index; ab.s.flags = nullptr; ab.s.cap = std::min(b.cap, m.cap);
  ab.s.records2 = m.rec; ab.s.counter = m.cnt; ab.s.ext_counter = m.cnt ? 1 : 0;
  ab.set = true;
  return m;
}

// Selects the step pair's own block for the verification launches queued until the scope ends.  `clear`: also clears
// the two flags the launch reports through (the synchronous body leaves that to sf_find_matches_and_verify_device).
struct UseStepBlock {
  sf_context* c;
  int sel_before;
  UseStepBlock(sf_context* c_, bool clear) : c(c_), sel_before(c_->accept_sel) {
    c->accept_sel = 2;
    if (clear) c->accept_armed = c->accept_streamed = false;
  }
  ~UseStepBlock() { c->accept_sel = sel_before; }
  UseStepBlock(const UseStepBlock&) = delete;
  UseStepBlock& operator=(const UseStepBlock&) = delete;
};

// ---- the synchronous body (round 3's step): the NN stage is walked on the host inside the call -----------------------
// Used when the device walk does not apply (SF_OPT_STEP_DEVICE_WALK off, the two-halves verification) and as the fallback
// of a device step whose candidate set was too dense for the filter level.
static int step_issue_sync(sf_context* c, sf_context::StepBlock& b, int32_t slot_base_other, int32_t slot_base_local) {
  const int n_l = c->nn_local.n;
  int rc;
  const StepMirror mirror = step_accept_block(c, b);
  b.matches.resize((size_t)std::max(n_l, 1));
  int32_t n = 0;
  {
    UseStepBlock sel(c, false);
    rc = sf_find_matches_and_verify_device(c, slot_base_other, slot_base_local, b.matches.data(), n_l, &n, nullptr);
  }
  b.device_walk = false;
  b.armed = c->accept_armed;                  // the block may hold streamed records (also of an abandoned speculation)
  if (rc != SF_OK) return rc;
  b.n = n;
  b.streamed = c->accept_streamed && n > 0;
  b.pairs = b.armed ? (int32_t)c->spec.grid : 0;
  if (b.streamed) {
    b.slot_of_match.resize((size_t)n);
    const int32_t* ix = c->last_results_index;
    for (int i = 0; i < n; ++i) b.slot_of_match[i] = ix ? ix[i] : i;
  } else if (n > 0) {
    // not streamed (no speculation for this query, or a launch shape the stream does not cover): the accepted results of
    // the matches are compacted, in match order, straight into the block (mirror writes beyond its capacity are dropped
    // and show in the mirror's count: the exchange's overflow path)
    if (n > b.cap) return sf_fail(c, SF_ERANGE, "sf_step_issue: %d matches exceed the block's %d records", n, b.cap);
    if ((rc = sf_compact_launch(c, c->last_results, n, b.records, b.flags, b.count, c->last_results_index,
                                mirror.rec, nullptr, (int32_t*)mirror.cnt, mirror.cap)) != SF_OK) return rc;
  }
  SF_HIP(c, hipEventRecord(b.done, c->stream));
  return SF_OK;
}

// Waits for a step and, if its device walk reported a candidate set too dense for the filter level, runs the query again
// on the synchronous path (the handle is idle by then: every step in flight is waited for first, since the ladder rewrites
// state all lanes read).  Idempotent.
static int step_settle(sf_context* c, sf_context::StepBlock& b) {
  if (b.settled) return b.settle_rc;
  b.settled = true;
  hipError_t e = hipEventSynchronize(b.done);
  if (e != hipSuccess) return b.settle_rc = sf_fail(c, SF_EHIP, "hipEventSynchronize(step) -> %s", hipGetErrorString(e));
  if (!b.device_walk || *b.walk_status == 0) return b.settle_rc = SF_OK;
  for (auto& o : c->step_blocks)
    if (o.issued && o.done) (void)hipEventSynchronize(o.done);
  // (what the void verification may have streamed: nothing -- the walk emitted no match -- but the entries are the next
  //  query's, so make sure)
  for (int32_t r = 0; r < b.cap && b.index[r] >= 0; ++r) b.index[r] = -1;
  const bool mirrored = c->step_mirror_records[b.parity] != nullptr;
  c->in_overlapped_step = false;
  int rc = step_issue_sync(c, b, b.slot_other, b.slot_local);        // (on the handle's own stream and buffers)
  if (rc == SF_OK && (e = hipEventSynchronize(b.done)) != hipSuccess)
    rc = sf_fail(c, SF_EHIP, "hipEventSynchronize(step fallback) -> %s", hipGetErrorString(e));
  if (rc == SF_OK && mirrored)
    rc = sf_fail(c, SF_ERANGE, "sf_step_retire: the NN candidate set outgrew the filter level while a mirror was set -- the "
                               "mirror (parity %d) missed this step's records.  The level is settled now; the step counter has "
                               "advanced, so a re-issued step writes the mirror of parity %d: retire everything in flight, "
                               "re-zero both counters and issue the step again", b.parity, (int)(c->step_seq & 1));
  return b.settle_rc = rc;
}

static int step_settle_all(sf_context* c) {
  int rc = SF_OK;
  for (int k = c->step_inflight; k >= 1; --k) {          // oldest first
    sf_context::StepBlock& b = step_block(c, k);
    const int r = step_settle(c, b);
    if (rc == SF_OK) rc = r;
  }
  return rc;
}

// ---- SF_OPT_STEP_OVERLAP: the further lanes of the step pipeline ----------------------------------------------------
// A database (or a mask) is about to change: every step in flight is settled first -- waited for, and re-run on the
// synchronous path if its device walk asked for that -- so that no queued kernel reads what the caller is about to
// write and a fallback still sees the state its step was issued on.  `drain` also waits for the lanes' streams.
int sf_lanes_touch(sf_context* c, bool drain) {
  c->db_epoch += 1;
  const int rc = step_settle_all(c);      // (a step whose fallback re-run failed: the error is the caller's to see)
  if (drain)
    for (int k = 1; k < SF_STEP_MAX_LANES; ++k)
      if (c->ws[k].stream) SF_HIP(c, hipStreamSynchronize(c->ws[k].stream));
  return rc;
}

extern "C" int sf_step_mirror_pair(sf_handle c, sf_result* d_records_even, uint32_t* d_counter_even,
                                   sf_result* d_records_odd, uint32_t* d_counter_odd, int32_t cap) {
  if (!c || cap < 0 || ((d_records_even == nullptr) != (d_counter_even == nullptr)) ||
      ((d_records_odd == nullptr) != (d_counter_odd == nullptr)) || ((d_records_even == nullptr) != (d_records_odd == nullptr)))
    return SF_EINVAL;
  if (c->step_inflight) return sf_fail(c, SF_EINVAL, "sf_step_mirror: %d step(s) in flight, retire them first", c->step_inflight);
  c->step_mirror_records[0] = d_records_even;
  c->step_mirror_counter[0] = d_counter_even;
  c->step_mirror_records[1] = d_records_odd;
  c->step_mirror_counter[1] = d_counter_odd;
  c->step_mirror_cap = d_records_even ? cap : 0;
  c->step_mirror_lanes = false;
  c->step_seq = 0;                                                      // the next step is an even one
  return SF_OK;
}

extern "C" int sf_step_mirror(sf_handle c, sf_result* d_records2, uint32_t* d_counter, int32_t cap) {
  return sf_step_mirror_pair(c, d_records2, d_counter, d_records2, d_counter, cap);
}

// Lane k's stream, counters and event, created on first use
static int lane_create(sf_context* c, int k) {
  Workspace& L = c->ws[k];
  if (L.stream) return SF_OK;
  int rc0 = sf_side_stream(c, SF_STREAM_LANE, k, &L.stream);
  if (rc0 != SF_OK) return rc0;
  if ((rc0 = sf_event_ensure(c, L.ev_main)) != SF_OK) return rc0;
  return sf_buf_reserve(c, L.counters, 64);          // (the work-list counters of the stage kernels; the handle's own
}                                                    //  are reserved at sf_create)

// Before lane k issues: the databases were written through the handle's stream since this lane last looked?  Wait for
// that work once.
static int lane_prepare(sf_context* c, int k) {
  int rc0 = lane_create(c, k);
  if (rc0 != SF_OK) return rc0;
  Workspace& L = c->ws[k];
  if (L.seen_db_epoch != c->db_epoch) {
    SF_HIP(c, hipEventRecord(L.ev_main, c->stream));
    SF_HIP(c, hipStreamWaitEvent(L.stream, L.ev_main, 0));
    L.seen_db_epoch = c->db_epoch;
  }
  return SF_OK;
}

extern "C" int sf_step_mirror_streams(sf_handle c, void** stream_even, void** stream_odd) {
  if (!c || !stream_even || !stream_odd) return SF_EINVAL;
  if (c->step_inflight) return sf_fail(c, SF_EINVAL, "sf_step_mirror_streams: %d step(s) in flight, retire them first", c->step_inflight);
  if (!c->step_mirror_records[0] || c->step_mirror_records[0] == c->step_mirror_records[1])
    return sf_fail(c, SF_EINVAL, "sf_step_mirror_streams: needs two distinct mirrors (sf_step_mirror_pair)");
  SF_HIP(c, hipSetDevice(c->device));
  *stream_even = *stream_odd = (void*)c->stream;
  if (c->step_overlap && !c->overlap && c->step_lanes >= 2) {
    int rc = lane_create(c, 1);
    if (rc != SF_OK) return rc;
    *stream_odd = (void*)c->ws[1].stream;
    c->step_mirror_lanes = true;
  }
  return SF_OK;
}

// ---- the device-resident bodies --------------------------------------------------------------------------------------

// Batch mode (the walk may return every local row) on the fp16 filter: the verification of EVERY filter candidate goes
// onto the step's stream straight behind the filter, and the exact re-evaluation, the row minima and the walk run on a
// second stream beside it -- off the chain of dependent launches that decides how soon the lane is free for its next
// step.  The walk's matches then name their candidate's verification slot (walk_slots); round 3 did the same with the
// host in the middle.  A step of the reference's cadence (20 matches of 10 000 rows) would verify 500 x too much this way
// and takes step_issue_serial.
static int step_issue_speculative(sf_context* c, sf_context::StepBlock& b, int lane, int32_t slot_base_other,
                                  int32_t slot_base_local, int lim) {
  const int n_l = c->nn_local.n, n_r = c->nn_recv.n;
  int rc;
  if (!c->w->aux) {
    if ((rc = sf_side_stream(c, SF_STREAM_AUX, lane, &c->w->aux)) != SF_OK) return rc;
    if ((rc = sf_event_ensure(c, c->w->ev_filter)) != SF_OK || (rc = sf_event_ensure(c, c->w->ev_walk)) != SF_OK) return rc;
  }
  const size_t min_b = ((size_t)n_l * 8 + 63) & ~(size_t)63, i32_b = ((size_t)n_l * 4 + 63) & ~(size_t)63;
  if ((rc = sf_buf_reserve(c, c->w->step_nn, 2 * min_b + 2 * i32_b + 64)) != SF_OK) return rc;
  char* base = (char*)c->w->step_nn.p;
  double* d_min = (double*)base;
  int32_t* d_arg = (int32_t*)(base + min_b);
  int32_t* d_cand = (int32_t*)(base + min_b + i32_b);
  unsigned long long* d_arg64 = (unsigned long long*)(base + min_b + 2 * i32_b);
  int32_t* d_status = (int32_t*)(base + 2 * min_b + 2 * i32_b);
  NnFilterOut fo;
  if ((rc = sf_nn_filter_dev(c, &fo)) != SF_OK) return rc;
  SF_HIP(c, hipEventRecord(c->w->ev_filter, c->stream));
  // the step's stream: every candidate slot verified (slots past the device-side count are void)
  if ((rc = spec_reserve(c, spec_grid(n_l), slot_base_other, slot_base_local)) != SF_OK) return rc;
  step_accept_block(c, b);
  {
    UseStepBlock sel(c, true);
    rc = sf_spec_launch(c, fo.cand, fo.count);
  }
  b.armed = c->accept_armed;
  b.streamed = c->accept_streamed;
  b.pairs = (int32_t)c->spec.grid;
  if (rc != SF_OK) return rc;
  // the second stream: exact distances -> row minima (with each minimum's candidate index) -> argsort + walk
  SF_HIP(c, hipStreamWaitEvent(c->w->aux, c->w->ev_filter, 0));
  {
    UseWorkspace on_aux(c, *c->w, c->w->aux);   // (the launchers queue on, and bracket for, the handle's current stream)
    rc = sf_nn_minima_of_candidates_dev(c, fo, d_min, d_arg, d_status, d_cand, d_arg64, c->store.kcap >= 256);
    if (rc == SF_OK)
      rc = sf_nn_walk_dev(c, d_min, d_arg, d_status, n_l, n_r, c->params.netvlad_distance, c->params.netvlad_max_matches_nb,
                          lim, nullptr, nullptr, b.walk_matches, b.walk_n, b.walk_status, d_cand, b.walk_slots, fo.count,
                          c->spec.grid);
  }
  if (rc != SF_OK) { (void)hipStreamSynchronize(c->w->aux); return rc; }
  SF_HIP(c, hipEventRecord(c->w->ev_walk, c->w->aux));
  SF_HIP(c, hipStreamWaitEvent(c->stream, c->w->ev_walk, 0));      // the step is done when both streams are
  if (!b.streamed)      // (step_issue_device picks this form only where the launch streams: a plan / arm mismatch)
    return sf_fail(c, SF_EHIP, "speculative step: the verification launch did not arm the accepted-result stream");
  SF_HIP(c, hipEventRecord(b.done, c->stream));
  return SF_OK;
}

// Everything on one stream: NN kernels -> row minima -> argsort + walk -> verification of the walk's matches, taken from
// the device list.  Any query shape (the reference's cadence of 20 matches per tick included), both NN precisions.
static int step_issue_serial(sf_context* c, sf_context::StepBlock& b, int32_t slot_base_other, int32_t slot_base_local, int lim) {
  const int n_l = c->nn_local.n, n_r = c->nn_recv.n;
  int rc;
  const size_t min_bytes = ((size_t)n_l * 8 + 63) & ~(size_t)63, arg_bytes = ((size_t)n_l * 4 + 63) & ~(size_t)63;
  if ((rc = sf_buf_reserve(c, c->w->step_nn, min_bytes + arg_bytes + 64)) != SF_OK) return rc;
  double* d_min = (double*)c->w->step_nn.p;
  int32_t* d_arg = (int32_t*)((char*)c->w->step_nn.p + min_bytes);
  int32_t* d_status = (int32_t*)((char*)c->w->step_nn.p + min_bytes + arg_bytes);
  unsigned* d_count = (unsigned*)b.dev.p;                       // {matches, -, -, -, accept slot counter, ...}
  void* d_match_rc = (char*)b.dev.p + 64;
  if ((rc = sf_nn_row_minima_dev(c, d_min, d_arg, d_status)) != SF_OK) return rc;
  if ((rc = sf_nn_walk_dev(c, d_min, d_arg, d_status, n_l, n_r, c->params.netvlad_distance, c->params.netvlad_max_matches_nb,
                           lim, d_match_rc, d_count, b.walk_matches, b.walk_n, b.walk_status)) != SF_OK) return rc;
  // verification of the walk's matches: `lim` pair slots, those past the device-side count are void
  if ((rc = spec_reserve(c, (unsigned)lim, slot_base_other, slot_base_local)) != SF_OK) return rc;
  const StepMirror mirror = step_accept_block(c, b);
  {
    UseStepBlock sel(c, true);
    rc = sf_spec_launch(c, d_match_rc, d_count);
  }
  b.armed = c->accept_armed;
  b.streamed = c->accept_streamed;
  b.pairs = lim;
  if (rc != SF_OK) return rc;
  if (!b.streamed) {
    // a launch shape the stream does not cover (stage kernels, more than one chunk, a mirror smaller than the query):
    // ordered compaction of the `lim` slots, match order -- the void slots past the match count carry success = 0
    if (lim > b.cap) return sf_fail(c, SF_ERANGE, "sf_step_issue: %d pair slots exceed the block's %d records", lim, b.cap);
    if ((rc = sf_compact_launch(c, (const sf_result*)c->w->spec_results.p, lim, b.records, b.flags, b.count, nullptr, mirror.rec,
                                nullptr, (int32_t*)mirror.cnt, mirror.cap)) != SF_OK) return rc;
  }
  SF_HIP(c, hipEventRecord(b.done, c->stream));
  return SF_OK;
}

static int step_issue_device(sf_context* c, sf_context::StepBlock& b, int lane, int32_t slot_base_other,
                             int32_t slot_base_local) {
  const int n_l = c->nn_local.n;
  const int lim = std::min(n_l, c->params.netvlad_max_matches_nb);     // the walk looks at `lim` rows: at most `lim` matches
  b.device_walk = true;
  b.speculative = false;
  b.streamed = false; b.armed = false; b.n = 0; b.pairs = 0;
  *b.walk_status = 0;
  *b.walk_n = 0;
  if (lim <= 0) {                                   // (netvlad_max_matches_nb = 0: the walk returns nothing)
    SF_HIP(c, hipEventRecord(b.done, c->stream));
    return SF_OK;
  }
  // the speculative form where round 3 speculated (the walk may return every local row, filter path) and where every
  // verified slot can stream: one chunk, a chain-type launch, a block / mirror with a record slot for every candidate slot
  if (c->step_speculate && c->params.nn_precision == 1 && lim >= n_l) {
    const int grid = (int)spec_grid(n_l);
    const VerifyPlan plan = sf_verify_plan(c, sf_store_view(c->store), grid);
    sf_result* const mirror_rec = c->step_mirror_records[b.parity];
    const int32_t cap = std::min(b.cap, mirror_rec ? c->step_mirror_cap : b.cap);
    if (plan.streams() && cap >= grid) {
      b.speculative = true;
      return step_issue_speculative(c, b, lane, slot_base_other, slot_base_local, lim);
    }
  }
  return step_issue_serial(c, b, slot_base_other, slot_base_local, lim);
}

extern "C" int sf_step_issue(sf_handle c, int32_t slot_base_other, int32_t slot_base_local) {
  if (!c) return SF_EINVAL;
  if (c->step_inflight >= c->step_depth)
    return sf_fail(c, SF_EINVAL, "%d steps are in flight (SF_OPT_STEP_DEPTH): call sf_step_retire first", c->step_inflight);
  if (c->nn_local.n <= 0 || c->nn_recv.n <= 0)
    return sf_fail(c, SF_EINVAL, "empty descriptor database (data_handler.py:308 guards this case)");
  SF_HIP(c, hipSetDevice(c->device));
  // camera ids of slots appended or re-tagged since the last step: uploaded through the handle's stream before a lane is
  // picked (the steps in flight were settled by whatever changed the store)
  if (sf_camera_active(c)) { const int rc0 = sf_camera_sync(c); if (rc0 != SF_OK) return rc0; }
  const bool mirrored = c->step_mirror_records[0] != nullptr;
  if (mirrored) {
    // A mirror has ONE caller buffer (and one caller-zeroed counter) per parity: step k + 2 writes where step k wrote.  The
    // ring's depth (default 6) would let step k + 2 zero and overwrite the mirror before step k is retired and its collective
    // enqueued, so with a mirror set no more steps may be in flight than the mirror has buffers.
    const int mirror_buffers = (c->step_mirror_records[1] && c->step_mirror_records[1] != c->step_mirror_records[0]) ? 2 : 1;
    if (c->step_inflight >= mirror_buffers)
      return sf_fail(c, SF_EINVAL, "%d step(s) in flight with a %d-buffer mirror set (sf_step_mirror%s): retire before issuing -- "
                                   "step k + %d would overwrite the records of step k", c->step_inflight, mirror_buffers,
                     mirror_buffers == 2 ? "_pair" : "", mirror_buffers);
  }
  int lanes = (c->step_overlap && !c->overlap && (!mirrored || c->step_mirror_lanes)) ? c->step_lanes : 1;
  if (mirrored) lanes = std::min(lanes, 2);          // (a mirror's buffer and its collective live on the stream of its parity)
  if (c->params.nn_precision == 0) lanes = 1;        // (the fp32-ranking path keeps its partial minima in ONE workspace)
  const int lane = (int)(c->step_seq % (uint64_t)lanes);
  sf_context::StepBlock& b = step_block(c, 0);
  const int n_l = c->nn_local.n;
  int rc;
  // every slot of a speculative verification may be accepted: the block holds them all (see arm_accept_stream)
  if ((rc = step_block_reserve(c, b, (int32_t)spec_grid(n_l))) != SF_OK) return rc;
  b.parity = (int)(c->step_seq & 1);
  b.slot_other = slot_base_other; b.slot_local = slot_base_local;
  b.settled = false; b.settle_rc = SF_OK;
  c->in_overlapped_step = lanes > 1;            // (sf_use_split: the form the verification takes)
  const bool device = c->step_device_walk && !c->overlap && c->store.slots > 0;
  if (lane > 0 && (rc = lane_prepare(c, lane)) != SF_OK) { c->in_overlapped_step = false; return rc; }
  Workspace& L = c->ws[lane];
  UseWorkspace on(c, L);
  if (b.copy_pending) {            // (sf_memcpy_device_async out of this block's records, possibly on a stream of the caller's)
    hipError_t e = hipStreamWaitEvent(c->stream, b.copied, 0);
    if (e != hipSuccess) rc = sf_fail(c, SF_EHIP, "hipStreamWaitEvent(copy of d_records) -> %s", hipGetErrorString(e));
    b.copy_pending = false;
  }
  // state every lane reads (fp16 copies, coefficients, masks) prepared by another lane since this one last looked?
  if (L.seen_prep != c->prep_epoch && c->ev_prep) {
    hipError_t e = hipStreamWaitEvent(c->stream, c->ev_prep, 0);
    if (e != hipSuccess) rc = sf_fail(c, SF_EHIP, "hipStreamWaitEvent -> %s", hipGetErrorString(e));
  }
  L.seen_prep = c->prep_epoch;
  const uint64_t prep_before = c->prep_count;
  if (rc == SF_OK) rc = device ? step_issue_device(c, b, lane, slot_base_other, slot_base_local)
                               : step_issue_sync(c, b, slot_base_other, slot_base_local);
  if (c->prep_count != prep_before) {
    (void)sf_event_ensure(c, c->ev_prep);
    if (c->ev_prep) (void)hipEventRecord(c->ev_prep, c->stream);
    c->prep_epoch += 1;
    L.seen_prep = c->prep_epoch;
  }
  if (rc != SF_OK) {
    // nothing of a failed issue may stay behind: whatever was queued is waited for and the block's streamed entries are
    // reset, so the next step starts from a clean block
    (void)hipStreamSynchronize(c->stream);
    for (int32_t r = 0; r < b.cap && b.index[r] >= 0; ++r) b.index[r] = -1;
  }
  c->in_overlapped_step = false;
  if (rc != SF_OK) return rc;
  b.issued = true;
  c->step_seq += 1;
  c->step_inflight += 1;
  return SF_OK;
}

extern "C" int sf_step_retire(sf_handle c, sf_step_result* out) {
  if (!c || !out) return SF_EINVAL;
  memset(out, 0, sizeof(*out));
  if (c->step_inflight <= 0) return sf_fail(c, SF_EINVAL, "sf_step_retire: no step in flight");
  sf_context::StepBlock& b = step_block(c, c->step_inflight);   // the OLDEST
  SF_HIP(c, hipSetDevice(c->device));
  int rc = step_settle(c, b);                    // its verification (and compaction) has left the device
  // whatever happens below, the step leaves the pipeline and its block is clean for its next use
  b.issued = false;
  c->step_inflight -= 1;
  int32_t n_streamed = 0;
  if (b.armed) {
    // streamed records: completion order, one per ACCEPTED verified slot; the used entries of the index list are its
    // prefix.  They are reset here for the block's next step -- also when the query fell back and never read them.
    while (n_streamed < b.cap && b.index[n_streamed] >= 0) ++n_streamed;
    if (b.streamed) b.rec_of_slot.assign((size_t)std::max(b.pairs, 1), -1);
    for (int32_t r = 0; r < n_streamed; ++r) {
      const int32_t slot = b.index[r];
      if (b.streamed && slot < b.pairs) b.rec_of_slot[slot] = r;
      b.index[r] = -1;
    }
  }
  if (rc != SF_OK) return rc;
  const sf_match* matches = b.matches.data();
  int n = b.n;
  if (b.device_walk) {
    n = *b.walk_n;
    if (n < 0 || n > std::max(b.pairs, c->nn_local.n)) return sf_fail(c, SF_EHIP, "sf_step_retire: the device walk reports %d matches of %d slots", n, b.pairs);
    matches = b.walk_matches;
  }
  b.record_of_match.assign((size_t)std::max(n, 1), -1);
  int32_t n_records = 0, n_accepted = 0;
  if (b.streamed) {
    n_records = n_streamed;
    for (int i = 0; i < n; ++i) {
      // (serial device step: pair slot i IS match i; speculative: the slot of the match's candidate)
      const int32_t slot = b.device_walk ? (b.speculative ? b.walk_slots[i] : i) : b.slot_of_match[i];
      const int32_t r = (slot >= 0 && slot < b.pairs) ? b.rec_of_slot[slot] : -1;
      b.record_of_match[i] = r;
      n_accepted += r >= 0;
    }
  } else if (n > 0) {
    n_records = *b.count;
    if (n_records < 0) return sf_fail(c, SF_EHIP, "sf_step_retire: the ordered compaction's look-back timed out");
    int32_t run = 0;
    for (int i = 0; i < n; ++i) b.record_of_match[i] = b.flags[i] ? run++ : -1;
    n_accepted = run;
    if (run != n_records) return sf_fail(c, SF_EHIP, "sf_step_retire: %d flags set, %d records compacted", run, n_records);
  }
  out->matches = matches;
  out->n_matches = n;
  out->record_of_match = b.record_of_match.data();
  out->records = b.records;
  out->d_records = c->step_mirror_records[b.parity] ? nullptr : (const sf_result*)b.dev_records.p;
  out->n_records = n_records;
  out->n_accepted = n_accepted;
  out->streamed = b.streamed ? 1 : 0;
  return SF_OK;
}

extern "C" int sf_memcpy_device_async(sf_handle c, void* d_dst, const void* d_src, size_t bytes, void* hip_stream) {
  if (!c || (bytes > 0 && (!d_dst || !d_src))) return SF_EINVAL;
  if (bytes == 0) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
  SF_HIP(c, hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, s));
  // out of a step block's record buffer: the block's next step must not overwrite it before this copy has run
  for (auto& b : c->step_blocks) {
    const char* lo = (const char*)b.dev_records.p;
    if (!lo || (const char*)d_src < lo || (const char*)d_src >= lo + b.dev_records.bytes) continue;
    const int rc = sf_event_ensure(c, b.copied);
    if (rc != SF_OK) return rc;
    SF_HIP(c, hipEventRecord(b.copied, s));
    b.copy_pending = true;
    break;
  }
  return SF_OK;
}

extern "C" int sf_last_match_results(sf_handle c, const sf_result** d_results, const int32_t** index, int32_t* n) {
  if (!c || !d_results || !index || !n) return SF_EINVAL;
  *d_results = c->last_results; *index = c->last_results_index; *n = c->last_results_n;
  return SF_OK;
}

// ---- NN stage entry points (implementation in k_nn.hip) --------------------------------------------
extern "C" int sf_nn_append_local(sf_handle c, const double* desc, int32_t n, int32_t dim) {
  if (!c) return SF_EINVAL;
  return sf_nn_append(c, c->nn_local, desc, n, dim, 0);
}
extern "C" int sf_nn_append_received(sf_handle c, const double* desc, int32_t n, int32_t dim) {
  if (!c) return SF_EINVAL;
  return sf_nn_append(c, c->nn_recv, desc, n, dim, 0);
}
extern "C" int sf_nn_append_local_f16_device(sf_handle c, const uint16_t* d, int32_t n, int32_t dim) {
  if (!c) return SF_EINVAL;
  return sf_nn_append(c, c->nn_local, d, n, dim, 2);
}
extern "C" int sf_nn_append_received_f16_device(sf_handle c, const uint16_t* d, int32_t n, int32_t dim) {
  if (!c) return SF_EINVAL;
  return sf_nn_append(c, c->nn_recv, d, n, dim, 2);
}
extern "C" int sf_nn_append_local_f32_device(sf_handle c, const float* d, int32_t n, int32_t dim) {
  if (!c) return SF_EINVAL;
  return sf_nn_append(c, c->nn_local, d, n, dim, 1);
}
extern "C" int sf_nn_append_received_f32_device(sf_handle c, const float* d, int32_t n, int32_t dim) {
  if (!c) return SF_EINVAL;
  return sf_nn_append(c, c->nn_recv, d, n, dim, 1);
}

extern "C" int sf_nn_sizes(sf_handle c, int32_t* n_local, int32_t* n_received) {
  if (!c) return SF_EINVAL;
  if (n_local) *n_local = c->nn_local.n;
  if (n_received) *n_received = c->nn_recv.n;
  return SF_OK;
}

// A mask is about to change: steps in flight were issued on the masks as they are and are waited for first (the callers
// validate their arguments before this drain; a settle error -- a step whose re-run failed -- is the call's error: the
// mask is not touched then)
static int masks_settle(sf_context* c) { return c->step_inflight ? sf_lanes_touch(c, false) : SF_OK; }

extern "C" int sf_nn_mark_local_used(sf_handle c, int32_t idx) {
  if (!c) return SF_EINVAL;
  if (idx < 0 || idx >= c->nn_local.n) return sf_fail(c, SF_ERANGE, "local index %d outside [0,%d)", idx, c->nn_local.n);
  if (const int rc = masks_settle(c); rc != SF_OK) return rc;
  if ((int)c->mask_local.size() < c->nn_local.n) c->mask_local.resize(c->nn_local.n, 0);
  c->mask_local[idx] = 1;
  c->masks_dirty = true;
  return SF_OK;
}

extern "C" int sf_nn_mark_other_used(sf_handle c, int32_t idx) {
  if (!c) return SF_EINVAL;
  if (idx < 0 || idx >= c->nn_recv.n) return sf_fail(c, SF_ERANGE, "other index %d outside [0,%d)", idx, c->nn_recv.n);
  if (const int rc = masks_settle(c); rc != SF_OK) return rc;
  if ((int)c->mask_other.size() < c->nn_recv.n) c->mask_other.resize(c->nn_recv.n, 0);
  c->mask_other[idx] = 1;
  c->masks_dirty = true;
  return SF_OK;
}

extern "C" int sf_nn_ignore_pair(sf_handle c, int32_t il, int32_t io) {
  if (!c) return SF_EINVAL;
  if (il < 0 || il >= c->nn_local.n || io < 0 || io >= c->nn_recv.n)
    return sf_fail(c, SF_ERANGE, "pair (%d,%d) outside the %d x %d distance matrix", il, io, c->nn_local.n, c->nn_recv.n);
  if (const int rc = masks_settle(c); rc != SF_OK) return rc;
  c->ignored.push_back(il);
  c->ignored.push_back(io);
  c->masks_dirty = true;
  return SF_OK;
}

extern "C" int sf_nn_reset(sf_handle c) {
  if (!c) return SF_EINVAL;
  (void)sf_lanes_touch(c, true);
  SF_HIP(c, hipStreamSynchronize(c->stream));
  // the row buffers are sized, pitched and zero-padded for the old dimension: release them, the next append
  // re-allocates for its own (nn_reserve); the fp16 copies and cached filter coefficients go with them
  for (NNDb* db : {&c->nn_local, &c->nn_recv}) {
    sf_buf_free(db->rows); sf_buf_free(db->norms); sf_buf_free(db->rows_h); sf_buf_free(db->norms_k);
    db->n = 0; db->cap = 0; db->ld = 0; db->h_n = -1; db->h_ld = 0; db->h_kprefix = 0;
  }
  c->nn_coef_level = -1;
  c->nn_level = 0;
  c->nn_level_cooldown = 32;
  c->nn_dim = 0;
  c->mask_local.clear();
  c->mask_other.clear();
  c->ignored.clear();
  c->masks_dirty = true;
  return SF_OK;
}

extern "C" int sf_nn_set_precision(sf_handle c, int32_t nn_precision) {
  if (!c) return SF_EINVAL;
  if (nn_precision != 0 && nn_precision != 1) return sf_fail(c, SF_EINVAL, "nn_precision must be 0 or 1");
  c->params.nn_precision = nn_precision;
  return SF_OK;
}

extern "C" int sf_nn_find_matches(sf_handle c, sf_match* out, int32_t cap, int32_t* n_out) {
  if (!c || !n_out || cap < 0 || (cap > 0 && !out)) return SF_EINVAL;
  *n_out = 0;
  if (c->nn_local.n <= 0 || c->nn_recv.n <= 0)
    return sf_fail(c, SF_EINVAL, "empty descriptor database (data_handler.py:308 guards this case)");
  SF_HIP(c, hipSetDevice(c->device));
  return sf_nn_run(c, out, cap, n_out);
}

extern "C" int sf_nn_row_minima_device(sf_handle c, double* d_row_min, int32_t* d_row_arg, int32_t* d_status) {
  if (!c || !d_row_min || !d_row_arg || !d_status) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return sf_nn_row_minima_dev(c, d_row_min, d_row_arg, d_status);
}

extern "C" int sf_nn_walk_device(sf_handle c, const double* d_row_min, const int32_t* d_row_arg, const int32_t* d_status,
                                 int32_t n_local, int32_t n_received, sf_match* d_matches, int32_t cap, int32_t* d_n_matches) {
  if (!c || !d_row_min || !d_row_arg || !d_n_matches || cap < 0 || (cap > 0 && !d_matches)) return SF_EINVAL;
  if (n_local <= 0 || n_received <= 0) return sf_fail(c, SF_EINVAL, "sf_nn_walk_device over %d x %d minima", n_local, n_received);
  SF_HIP(c, hipSetDevice(c->device));
  return sf_nn_walk_dev(c, d_row_min, d_row_arg, d_status, n_local, n_received, c->params.netvlad_distance,
                        c->params.netvlad_max_matches_nb, cap, nullptr, nullptr, d_matches, d_n_matches, nullptr);
}

extern "C" int sf_nn_walk(sf_handle c, const double* row_min, const int32_t* row_arg, int32_t n_local, int32_t n_received,
                          sf_match* out, int32_t cap, int32_t* n_out) {
  if (!c || !n_out || n_local < 0 || n_received < 0 || cap < 0 || (cap > 0 && !out) || (n_local > 0 && (!row_min || !row_arg)))
    return SF_EINVAL;
  *n_out = 0;
  if (n_local == 0 || n_received == 0) return SF_OK;
  return sf_nn_walk_host(c, row_min, row_arg, n_local, n_received, c->params.netvlad_distance,
                         c->params.netvlad_max_matches_nb, out, cap, n_out);
}

extern "C" int sf_nn_last_filter_dims(sf_handle c, int32_t* dims) {
  if (!c || !dims) return SF_EINVAL;
  *dims = c->nn_last_kdims;
  return SF_OK;
}

extern "C" int sf_nn_last_row_minima(sf_handle c, double* dist, int32_t* idx, int32_t cap) {
  if (!c) return SF_EINVAL;
  const int n = std::min<int>(cap, (int)c->last_row_min.size());
  for (int i = 0; i < n; ++i) {
    if (dist) dist[i] = c->last_row_min[i];
    if (idx) idx[i] = c->last_row_arg[i];
  }
  return SF_OK;
}
