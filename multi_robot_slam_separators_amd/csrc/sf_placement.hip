// sf_placement.hip -- where the library's streams sit on the hardware: the placement measurement (k_place_hog,
// k_place_probe) and the one creator of every side stream (copy, lane, second stream of a lane).
#include <chrono>

#include "sf_host.hpp"

// ---- where the step pipeline's streams sit on the hardware ----------------------------------------------------------
// The runtime multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 per priority level by default) and
// the queues onto the FOUR dispatch pipes of the command processor.  A launch whose workgroups do not all fit on the
// chip (every verification launch of a batch step) keeps its pipe's dispatcher busy until the last workgroup is placed:
// a launch on another queue of the SAME pipe waits for that, one on another pipe starts at once
// (tools/ubench/pipe_probe.hip, profiles/r04v_placement/pipe_probe_*.txt: 0.93-1.01 of the blocking launch's duration against
// 0.07).  Which pipe a new stream lands on depends on every stream the process created before -- torch's, RCCL's, the
// caller's -- so the same library ran a step in 0.44 ms or 0.50-0.56 ms depending on whether ONE other stream had been
// used first (profiles/r04v_placement, run k).  Hence: measure.  Twelve candidate streams (six per priority level) are sorted into
// classes by "a long launch on X delays a one-wavefront launch on Y"; the lanes' main streams are taken from classes
// other than the handle's own stream's (and each other's), the second streams -- the nine small dependent launches of
// the device walk, which must never sit behind a verification's dispatch -- from a class no main stream uses,
// highest priority first and on different queues where the class has several.  ~10-20 ms, once per handle.
__global__ void __launch_bounds__(512) k_place_hog(int* sink, int spins) {
  __shared__ int pad[16384];                           // 64 KB: two workgroups per CU, far fewer than the grid holds
  pad[threadIdx.x] = (int)threadIdx.x;
  for (int i = 0; i < spins; ++i) __builtin_amdgcn_s_sleep(127);
  __syncthreads();
  if (pad[(threadIdx.x + 1) & 511] == -1) sink[0] = 1;
}
__global__ void k_place_probe(int* sink) {
  if (threadIdx.x == 999) sink[1] = 1;
}

namespace {
struct PlaceProbe {
  int* d = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  int tests = 0;
  // (end of a one-wavefront launch on y - start of a chip-filling launch on x) / duration of the latter; < 0: failed
  float ratio(hipStream_t x, hipStream_t y) {
    ++tests;
    if (hipEventRecord(e0, x) != hipSuccess) return -1.f;
    hipLaunchKernelGGL(k_place_hog, dim3(4096), dim3(512), 0, x, d, 5);
    if (hipEventRecord(e1, x) != hipSuccess) return -1.f;
    hipLaunchKernelGGL(k_place_probe, dim3(1), dim3(64), 0, y, d);
    if (hipEventRecord(e2, y) != hipSuccess) return -1.f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventSynchronize(e2) != hipSuccess) return -1.f;
    float t_h = 0.f, t_y = 0.f;
    if (hipEventElapsedTime(&t_h, e0, e1) != hipSuccess || t_h <= 0.f) return -1.f;
    if (hipEventElapsedTime(&t_y, e0, e2) != hipSuccess) return 0.f;      // (the probe ran before the other queue started)
    return std::max(0.f, t_y / t_h);
  }
};
}  // namespace

static int place_streams(sf_context* c) {
  sf_context::StreamPlacement& P = c->placement;
  if (P.tried) return SF_OK;
  P.tried = true;
  if (const char* v = getenv("SF_STREAM_PLACEMENT")) if (atoi(v) == 0) return SF_OK;
  const auto t_begin = std::chrono::steady_clock::now();
  constexpr int NC = 12, MAXCLS = 8;
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  hipStream_t S[NC + 1] = {};
  bool high[NC + 1] = {};
  int cls[NC + 1], queue_of[NC + 1];
  PlaceProbe pr;
  auto cleanup = [&](int rc) {
    for (int i = 1; i <= NC; ++i) if (S[i]) { (void)hipStreamSynchronize(S[i]); (void)hipStreamDestroy(S[i]); }
    if (pr.e0) (void)hipEventDestroy(pr.e0);
    if (pr.e1) (void)hipEventDestroy(pr.e1);
    if (pr.e2) (void)hipEventDestroy(pr.e2);
    if (pr.d) (void)hipFree(pr.d);
    return rc;
  };
  S[0] = c->stream;
  for (int i = 1; i <= NC; ++i) {
    high[i] = (i & 1) == 0;
    if (hipStreamCreateWithPriority(&S[i], hipStreamNonBlocking, high[i] ? prio_greatest : 0) != hipSuccess) { S[i] = nullptr; return cleanup(SF_OK); }
  }
  if (hipMalloc((void**)&pr.d, 64) != hipSuccess || hipEventCreate(&pr.e0) != hipSuccess || hipEventCreate(&pr.e1) != hipSuccess ||
      hipEventCreate(&pr.e2) != hipSuccess) return cleanup(SF_OK);
  // every stream's hardware queue exists before anything is measured (the runtime creates it at the stream's first use).
  // Only THIS handle's streams are waited for (rounds 3-4 waited for the whole device, which also stalled on the work of
  // every other stream of the process -- RCCL's, torch's): work of other streams or processes that runs during the
  // measurement reads as "blocked" and is what the once-more rule below and the abandon path are for; a host that wants the
  // measurement at a quiet moment calls sf_streams_prepare (include/sf_experimental.h) when it has one.
  (void)hipStreamSynchronize(c->stream);
  for (Workspace& w : c->ws) if (w.stream) (void)hipStreamSynchronize(w.stream);
  for (int i = 1; i <= NC; ++i) {
    hipLaunchKernelGGL(k_place_probe, dim3(1), dim3(64), 0, S[i], pr.d);
    (void)hipStreamSynchronize(S[i]);
  }
  if (const char* v = getenv("SF_STREAM_PLACEMENT")) if (atoi(v) >= 3) {
    fprintf(stderr, "sepfinder: placement matrix (row: chip-filling launch on X; column: small launch on Y; 0 = the handle's stream, even = highest priority)\n      ");
    for (int y = 0; y <= NC; ++y) fprintf(stderr, " %c%-4d", high[y] ? 'H' : 'n', y);
    fprintf(stderr, "\n");
    for (int x = 0; x <= NC; ++x) {
      fprintf(stderr, "%c%-4d ", high[x] ? 'H' : 'n', x);
      for (int y = 0; y <= NC; ++y) { if (x == y) fprintf(stderr, "    - "); else fprintf(stderr, " %5.2f", pr.ratio(S[x], S[y])); }
      fprintf(stderr, "\n");
    }
  }
  // classes: streams a chip-filling launch on one of which delays the others (same pipe, or same queue)
  int rep[MAXCLS], n_cls = 0;
  bool failed = false;
  for (int i = 0; i <= NC && !failed; ++i) {
    cls[i] = -1;
    for (int k = 0; k < n_cls && cls[i] < 0; ++k) {
      float r = pr.ratio(S[rep[k]], S[i]);
      if (r > 0.3f && r < 0.6f) r = pr.ratio(S[rep[k]], S[i]);      // (something else ran in between: once more)
      if (r < 0.f) { failed = true; break; }
      if (r >= 0.5f) cls[i] = k;
    }
    if (cls[i] < 0 && !failed) {
      if (n_cls == MAXCLS) { failed = true; break; }
      rep[n_cls] = i; cls[i] = n_cls++;
    }
  }
  if (failed || n_cls < 2) {
    snprintf(P.report, sizeof(P.report), "placement: measurement %s (%d classes): streams as created", failed ? "failed" : "found one class", n_cls);
    return cleanup(SF_OK);
  }
  const int lanes = std::min(std::max(c->step_lanes, 1), SF_STEP_MAX_LANES);
  bool cls_main[MAXCLS] = {};
  cls_main[cls[0]] = true;
  bool taken[NC + 1] = {};
  auto take = [&](int i) { hipStream_t s = S[i]; S[i] = nullptr; taken[i] = true; return s; };
  // main streams of lanes 1..: a class no earlier main stream uses, default priority where the class offers it
  int main_cls[SF_STEP_MAX_LANES] = {}; main_cls[0] = cls[0];
  for (int k = 1; k < lanes; ++k) {
    int best = -1;
    for (int pass = 0; pass < 2 && best < 0; ++pass)
      for (int i = 1; i <= NC && best < 0; ++i)
        if (!taken[i] && !cls_main[cls[i]] && (pass == 1 || !high[i])) best = i;
    if (best < 0) break;                       // (fewer classes than lanes: the remaining lanes get streams as before)
    main_cls[k] = cls[best];
    cls_main[cls[best]] = true;
    P.main[k] = take(best);
  }
  // second streams: a class without a main stream -- the one with most candidates -- else the least bad: the fullest class
  int cnt[MAXCLS] = {}, aux_cls = -1;
  for (int i = 1; i <= NC; ++i) if (!taken[i]) cnt[cls[i]] += 1;
  for (int k = 0; k < n_cls; ++k) if (!cls_main[k] && cnt[k] > 0 && (aux_cls < 0 || cnt[k] > cnt[aux_cls])) aux_cls = k;
  const bool aux_free_pipe = aux_cls >= 0;
  if (aux_cls < 0) for (int k = 0; k < n_cls; ++k) if (cnt[k] > 0 && (aux_cls < 0 || cnt[k] > cnt[aux_cls])) aux_cls = k;
  int n_queues = 0;
  if (aux_cls >= 0) {
    // queues inside the class: a launch on the SAME queue ends behind the blocking one (ratio >= 1), one on another queue
    // of the pipe starts when the last workgroup has been placed (ratio ~ 1 - 1 / generations)
    int members[NC], n_m = 0, qrep[NC];
    for (int pass = 0; pass < 2; ++pass)       // highest priority first
      for (int i = 1; i <= NC; ++i) if (!taken[i] && cls[i] == aux_cls && high[i] == (pass == 0)) members[n_m++] = i;
    for (int m = 0; m < n_m; ++m) {
      const int i = members[m];
      queue_of[i] = -1;
      for (int q = 0; q < n_queues && queue_of[i] < 0; ++q) {
        const float r = pr.ratio(S[qrep[q]], S[i]);
        if (r >= 0.985f) queue_of[i] = q;
      }
      if (queue_of[i] < 0) { qrep[n_queues] = i; queue_of[i] = n_queues++; }
    }
    // deal them out queue by queue: lanes' second streams first, then the synchronous call's
    hipStream_t* want[SF_STEP_MAX_LANES + 1];
    int n_w = 0;
    for (int k = 0; k < lanes; ++k) want[n_w++] = &P.aux[k];
    want[n_w++] = &P.copy;
    int w = 0;
    for (int round = 0; round < n_m && w < n_w; ++round)
      for (int q = 0; q < n_queues && w < n_w; ++q)
        for (int m = 0; m < n_m; ++m)
          if (queue_of[members[m]] == q && !taken[members[m]]) { *want[w++] = take(members[m]); break; }
  }
  P.done = true;
  const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  int off = snprintf(P.report, sizeof(P.report), "placement: %d classes, %d tests, %.1f ms; main classes", n_cls, pr.tests, ms);
  for (int k = 0; k < lanes && off < (int)sizeof(P.report) - 8; ++k)
    off += snprintf(P.report + off, sizeof(P.report) - off, " %d%s", main_cls[k], (k == 0 || P.main[k]) ? "" : "?");
  int n_aux = 0;
  for (int k = 0; k < SF_STEP_MAX_LANES; ++k) n_aux += P.aux[k] != nullptr;
  if (off < (int)sizeof(P.report) - 8)
    snprintf(P.report + off, sizeof(P.report) - off, "; second streams: class %d (%s), %d stream(s) on %d queue(s)%s", aux_cls,
             aux_free_pipe ? "no main stream on it" : "SHARED with a main stream", n_aux, n_queues, P.copy ? " + 1 for the synchronous call" : "");
  if (const char* v = getenv("SF_STREAM_PLACEMENT")) if (atoi(v) >= 2) fprintf(stderr, "sepfinder: %s\n", P.report);
  return cleanup(SF_OK);
}

// Runs the stream placement measurement NOW (idempotent; otherwise it runs inside the first step that needs a second
// stream): 60-100 ms, ~100 short chip-filling launches on the handle's stream and on twelve streams of the library's own.
extern "C" int sf_streams_prepare(sf_handle c) {
  if (!c) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return place_streams(c);
}

extern "C" int sf_stream_placement(sf_handle c, char* buf, size_t n) {
  if (!c || !buf || n == 0) return SF_EINVAL;
  snprintf(buf, n, "%s", c->placement.tried ? (c->placement.report[0] ? c->placement.report : "placement: off") : "placement: not measured yet");
  return SF_OK;
}

// A side stream of the handle -- the copy stream of the synchronous speculative call, lane k's main stream or lane k's
// second stream: its measured place first (place_streams), else created blind as follows.
//
// The runtime multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and a stream that lands
// on the queue of another runs BEHIND it, not beside it (seen as soon as another library -- RCCL -- had created streams of
// its own: +0.17 ms per step).  Streams of another priority level draw from queues of their own, so unless the process
// raised the queue budget (bench.py sets GPU_MAX_HW_QUEUES=8, measured slightly better than the priority) the library's
// extra streams get the highest priority; the copy stream's work (exact NN re-evaluation, small copies) is what the host
// waits for.
// The second stream of a speculative step (exact re-evaluation, row minima, walk: a chain of nine small dependent
// launches) ALWAYS gets it: beside a matching launch, which holds every register of every CU, a launch of default
// priority waits for hundreds of microseconds for its first workgroup slot (k_walk_tile_sort: 435 us instead of 32,
// profiles/r04d_timeline_*), and the step is not done before its walk is.
int sf_side_stream(sf_context* c, SideStream role, int k, hipStream_t* out) {
  const bool aux = role == SF_STREAM_AUX;
  if (!c->placement.tried) (void)place_streams(c);
  hipStream_t& slot = role == SF_STREAM_COPY ? c->placement.copy : aux ? c->placement.aux[k] : c->placement.main[k];
  if (slot) { *out = slot; slot = nullptr; return SF_OK; }
  int prio_least = 0, prio_greatest = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  const char* hwq = getenv("GPU_MAX_HW_QUEUES");
  int prio = (hwq && atoi(hwq) >= 8 && !aux) ? 0 : prio_greatest;
  if (role != SF_STREAM_COPY)
    if (const char* v = getenv(aux ? "SF_AUX_PRIO" : "SF_LANE_PRIO")) prio = atoi(v) > 0 ? prio_greatest : (atoi(v) < 0 ? prio_least : 0);
  SF_HIP(c, hipStreamCreateWithPriority(out, hipStreamNonBlocking, prio));
  return SF_OK;
}
