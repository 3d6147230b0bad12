// sf_match_device.hpp -- what the matching stages share around their scans.
//
// General pieces (pass 1, pass 2 in k_guided.hip, the estimators in k_ransac.hip / k_pnp.hip): write_null_pass, the
// id-ordered compaction corr_compact, the finite-point count corr_count_finite, worklist_append; behind the estimators
// (and in k_ba.hip) pass_to3dof and merge_backward_pose.
//
// Pass 1 (global matching) has three scans -- k_match_global (scalar-load Hamming, float32 L2), match_v2_body (LDS + u16,
// fp4 matrix cores; both k_match.hip) and k_match_global_u8 (int8 matrix cores, k_match_u8.hip).  All three share
//   match_claim   an accepted "to" row takes its "from" word;
//   match_gates   the gates of the motion estimation: the part that maps line by line onto the reference's result assembly;
// and the general pieces.  k_match_global and k_match_global_u8 take everything else from here too:
//   match_slot_outside, match_report_outside   the guard of caller-provided slots and its report;
//   match_begin                                the pair's meta rows, the zeroed bookkeeping;
//   match_finish                               rejected rows, compaction, gates, count, header, pass state, work list.
// match_v2_body spells its guard, prologue, compaction loop and header write out: it is inlined into k_verify_fused and
// k_match_split, whose register allocation (the whole chain, in the fused kernel) moves with any of them behind a function
// boundary; what it calls from here leaves those kernels' vector code as it was (profiles/match_finish_isa.txt).
#pragma once
#include "sf_device_math.hpp"
#include "sf_internal.hpp"

// The "no transform" state of a pass (identity covariance scale, `matches` correspondences seen): built where it is
// written, so that no copy of it stays live in registers across the pass.
constexpr double SF_NULL_VAR = 1.0;     // var and var_ang of a null pass (write_null_result clamps it as finalize_one does)
__device__ __forceinline__ void write_null_pass(PassState& out, int matches) {
  PassState ps;
#pragma unroll
  for (int i = 0; i < 12; ++i) ps.T[i] = 0.f;
  ps.var = SF_NULL_VAR; ps.var_ang = SF_NULL_VAR;
  ps.is_null = 1;
  ps.inliers = 0;
  ps.matches = matches;
  ps.pad = 0;
  out = ps;
}

// The end-of-pass to3DoF of myRegistration.cpp:269-276 and, for pass 1, the one its result meets as the guess of
// pass 2 (:245-248): `times` applications by the thread that wrote the pass state.
__device__ inline void pass_to3dof(PassState& ps, int times) {
  if (ps.is_null) return;
  for (int t = 0; t < times; ++t) sfd::to3dof_canon(ps.T);
}

// Vis/ForwardEstOnly = false, myRegistrationVis.cpp:1376-1394: the backward estimate b enters the forward one a as its
// inverse -- taken as it is where a has no transform, else interpolate(0.5) with the two covariances' mean.
__device__ inline void merge_backward_pose(PassState& a, const PassState& b) {
  if (b.is_null) return;
  float inv[12];
  sfd::rigid_inverse_canon(b.T, inv);
  if (a.is_null) {
#pragma unroll
    for (int i = 0; i < 12; ++i) a.T[i] = inv[i];
    a.is_null = 0;
    a.var = b.var;
    a.var_ang = b.var_ang;
  } else {
    float mid[12];
    sfd::interpolate_half_canon(a.T, inv, mid);
#pragma unroll
    for (int i = 0; i < 12; ++i) a.T[i] = mid[i];
    a.var = (a.var + b.var) / 2.0;
    a.var_ang = (a.var_ang + b.var_ang) / 2.0;
  }
}

// The id-ordered compaction of the matches (wavefront ballots): out[k] = from | to << 16 for every "from" index i in
// ascending order whose to_of(i) >= 0; returns the list's length.  misc[4 .. 4 + NW) is its scratch.  Ends with a barrier.
template <int NW, class ToOf>
__device__ __forceinline__ int corr_compact(int Kf, uint32_t* out, int* misc, ToOf to_of) {
  constexpr int NT = 64 * NW;
  const int tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int running = 0;
  for (int base = 0; base < Kf; base += NT) {
    const int i = base + tid;
    const int m = (i < Kf) ? to_of(i) : -1;
    const bool flag = m >= 0;
    const unsigned long long bal = __ballot(flag);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) misc[4 + wave] = __popcll(bal);
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      int c = misc[4 + w];
      if (w < wave) woff += c;
      total += c;
    }
    if (flag) out[running + woff + before] = (uint32_t)i | ((uint32_t)m << 16);
    running += total;
    __syncthreads();
  }
  return running;
}

// `matches` of a pair that has correspondences but no estimate (what util3d::findCorrespondences would still report):
// *count (LDS, 0 on entry) += the list's entries whose "from" point is finite; with_to (3D-3D) also needs the "to" point
// and drops zero points.  xF / xT: the two slots' point rows.  Ends with a barrier.
template <int NT>
__device__ __forceinline__ void corr_count_finite(const float* xF, const float* xT, const uint32_t* out, int n_corr,
                                                  bool with_to, int* count) {
  for (int i = (int)threadIdx.x; i < n_corr; i += NT) {
    uint32_t c = out[i];
    const float* a = xF + 3 * (c & 0xFFFFu);
    const float* b = xT + 3 * (c >> 16);
    bool ok = isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]);
    if (with_to)
      ok = ok && isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && (a[0] != 0.f || a[1] != 0.f || a[2] != 0.f) &&
           (b[0] != 0.f || b[1] != 0.f || b[2] != 0.f);
    if (ok) atomicAdd(count, 1);
  }
  __syncthreads();
}

// a surviving pair joins the next stage's work list (one thread)
__device__ __forceinline__ void worklist_append(int32_t* __restrict__ list, int32_t* __restrict__ counter, int pair) {
  int pos = atomicAdd(counter, 1);
  list[pos] = pair;
}

// ---- pass 1 ---------------------------------------------------------------------------------------------------------
// The workgroup's bookkeeping in LDS, [2 kcap + 16] ints:
//   cnt   [kcap] "to" rows that matched each "from" word
//   owner [kcap] the matching "to" row (meaningful when cnt == 1)
//   misc  [16]   0: rejected "to" rows, 2: finite corr, 4..7 wave totals (k_match_split: 4..11, two words of per-trip
//                byte counts per wavefront, match_v2_body's LEAN compaction)

// "to" row t, accepted by the ratio test, takes "from" word f
__device__ __forceinline__ void match_claim(int* cnt, int* owner, int f, int t) {
  atomicAdd(&cnt[f], 1);
  owner[f] = t;
}

// Gate of the motion estimation from the pair's counts (mF / mT: the slots' meta rows, Kf / Kt their rows; rejected_to:
// "to" rows the ratio test decided against; n_corr: "from" words matched by exactly one "to" row).
// est: 0 = 3D->3D gate (myRegistrationVis.cpp:928,1117-1118); 1 = PnP gate (:1070-1071, 2D words of the "to" frame);
//      2 = PnP without a calibrated camera (:1059-1065): the estimation never runs
//      3 = PnP, both directions (Vis/ForwardEstOnly = false): either gate; every pair with a correspondence goes on,
//          the estimates count their own matches (the union of the two is not this kernel's to know)
// motion && !survivor: RANSAC will not run, and `matches` is the count util3d::findCorrespondences would still report.
struct MatchGates {
  int unique_to, words_from, words_to;      // wordsTo.size(), words3From.size(), words3To.size()
  bool motion, survivor;
};
__device__ __forceinline__ MatchGates match_gates(int Kf, int Kt, const int4& mF, const int4& mT, int rejected_to, int n_corr,
                                                  int min_inliers, int est) {
  MatchGates g;
  g.unique_to = (Kf > 0 && Kt > 0) ? rejected_to + n_corr : 0;
  g.words_from = (Kf > 0 && mF.y > 0) ? Kf : 0;
  g.words_to = (mT.y > 0) ? g.unique_to : 0;
  const int unique_to = g.unique_to, words_from = g.words_from, words_to = g.words_to;
  g.motion = est == 0 ? (unique_to > 0 && words_from >= min_inliers && words_to >= min_inliers)
           : est == 1 ? (unique_to > 0 && words_from >= min_inliers && unique_to >= min_inliers)
                      : (est == 3 && unique_to > 0 && ((words_from >= min_inliers && unique_to >= min_inliers) ||
                                                       (words_to >= min_inliers && Kf >= min_inliers)));
  g.survivor = est == 3 ? (g.motion && n_corr > 0) : (g.motion && n_corr >= min_inliers && n_corr >= (est == 0 ? 3 : 4));
  return g;
}

// ---- the rest of pass 1 for the kernels that are nothing but a scan: k_match_global, k_match_global_u8 -----------------
// One pair between match_begin and match_finish: its slots, their meta rows, and the bookkeeping.
struct MatchPair {
  int sF, sT;
  int4 mF, mT;     // {rows, n3d, nkp, cols} of the two slots
  int* cnt;
  int* owner;
  int* misc;
};

// The guard of caller-provided slots, `if (match_slot_outside(..)) { match_report_outside(..); return; }` in the kernel
// (block-uniform; the return stays there: with it behind a function boundary k_match_global<128, 1, 256, true>'s scan
// came out laid differently and 6 % slower).  The report is a failed estimation -- null header, null pass state, by
// thread 0 -- and the pair touches nothing else.
__device__ __forceinline__ bool match_slot_outside(const StoreView& st, int sF, int sT) {
  return (unsigned)sF >= (unsigned)st.n_slots || (unsigned)sT >= (unsigned)st.n_slots;
}
__device__ __forceinline__ void match_report_outside(CorrHeader& hdr_out, PassState& pass_out) {
  if (threadIdx.x == 0) {
    CorrHeader h = {0, 0, 0, 0};
    hdr_out = h;
    write_null_pass(pass_out, 0);
  }
}

// Slots inside the store: the pair's meta rows are loaded and the bookkeeping at `book` is zeroed; the barrier behind it
// is the caller's.
template <int NT>
__device__ __forceinline__ void match_begin(const StoreView& st, int sF, int sT, int* book, MatchPair& M) {
  M.sF = sF; M.sT = sT;
  M.mF = st.meta[sF]; M.mT = st.meta[sT];
  M.cnt = book;
  M.owner = book + st.kcap;
  M.misc = book + 2 * st.kcap;
  const int tid = threadIdx.x;
  for (int i = tid; i < M.mF.x; i += NT) M.cnt[i] = 0;
  if (tid < 16) M.misc[tid] = 0;
}

// Epilogue, called by the whole workgroup behind its scan.  `rejected`: the "to" rows this lane decided against.  `out` /
// hdr_out / pass_out: the pair's correspondence list (kcap entries), header and pass-1 state.
template <int NT>
__device__ __forceinline__ void match_finish(const StoreView& st, int pair, const MatchPair& M, int min_inliers, int est,
                                             int rejected, uint32_t* out, CorrHeader& hdr_out, PassState& pass_out,
                                             int32_t* __restrict__ list, int32_t* __restrict__ counter) {
  const int tid = threadIdx.x;
  const int kcap = st.kcap;
  const int Kf = M.mF.x, Kt = M.mT.x;
  int* cnt = M.cnt;
  int* owner = M.owner;
  int* misc = M.misc;
  // wave-reduce the rejected count, one LDS atomic per wave
  for (int off = 32; off >= 1; off >>= 1) rejected += __shfl_xor(rejected, off);
  if ((tid & 63) == 0 && rejected) atomicAdd(&misc[0], rejected);
  __syncthreads();

  // the "from" words matched by exactly one "to" row
  const int n_corr = corr_compact<NT / 64>(Kf, out, misc, [&](int f) { return cnt[f] == 1 ? owner[f] : -1; });
  const MatchGates G = match_gates(Kf, Kt, M.mF, M.mT, misc[0], n_corr, min_inliers, est);
  if (G.motion && !G.survivor)
    corr_count_finite<NT>(st.xyz + (size_t)M.sF * kcap * 3, st.xyz + (size_t)M.sT * kcap * 3, out, n_corr, est == 0, &misc[2]);
  if (tid == 0) {
    CorrHeader h;
    h.n_corr = n_corr;
    h.words_from = G.words_from;
    h.words_to = G.words_to;
    h.words_to_2d = G.unique_to;
    hdr_out = h;
    write_null_pass(pass_out, (G.motion && !G.survivor) ? misc[2] : 0);
    if (G.survivor) worklist_append(list, counter, pair);
  }
}
