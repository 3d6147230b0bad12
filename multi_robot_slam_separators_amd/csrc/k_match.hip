// k_match.hip -- pass-1 GLOBAL matching: brute-force Hamming kNN (k=2) + NNDR + uniqueness.
//
// Replaces the dictionary round trip at myRegistrationVis.cpp:826-895 of the reference
// (VWDictionary::addNewWords in brute-force mode [upstream rtabmap] = cv::BFMatcher NORM_HAMMING
// knnMatch k=2, accept nearest id unless d1 > nndr*d2, keep ids occurring exactly once per side).
//
// Three formulations of the same integers, all one 256-thread workgroup per candidate pair:
//   variant 3 (default, NQ == 0, further down): the K_from x K_to distance table as an exact +-1 product
//             on the fp4 matrix cores; variant 2 ("LDS + u16", SF_MATCH_MFMA=0): xor + popcount on the VALU
//             with the "from" block in LDS; variant 1 (frames too large for the LDS copy): below.
// Variant 1, CDNA4 mapping:
//   * every lane keeps TWO "to" descriptors resident in VGPRs (8 or 16 dwords each);
//   * the "from" descriptors are wave-uniform, so they are fetched with SCALAR loads
//     (s_load_dwordx8/x16 through the scalar cache) and fed to v_xor_b32 as SGPR operands --
//     no LDS traffic and no per-lane address math in the K_from x K_to inner product;
//   * v_bcnt_u32_b32 accumulates the popcount; distance and index are packed into one 32-bit
//     key (dist << 16 | from_idx) so best/second-best tracking is 3 integer min/max ops and ties
//     resolve to the lowest index (BFMatcher order);
//   * uniqueness uses LDS counters; the id-ordered compaction uses wavefront ballots.
// The kernel is VALU-bound (~19 lane-ops per descriptor pair); HBM traffic is the two descriptor
// blocks, read once (the "to" block coalesced 16 B/lane, the "from" block via the scalar cache).
#include "sf_internal.hpp"
#include "sf_match_device.hpp"
#include <type_traits>

namespace {

// popcount(x) + acc in ONE VALU op; written as asm because LLVM's reassociation otherwise turns the
// accumulate chain into `v_bcnt x, 0` + `v_add3` trees (+3 VALU ops per 256-bit descriptor pair).
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}

// Scan all "from" descriptors (wave-uniform -> scalar loads, SGPR operands) against the NQ "to"
// descriptors this lane keeps in VGPRs; track best / second-best keys (dist << 16 | from_idx).
template <int W, int NQ>
__device__ __forceinline__ void knn2_scan(const uint32_t* __restrict__ dF, int Kf, const uint32_t (&q)[NQ][W],
                                          uint32_t (&k1)[NQ], uint32_t (&k2)[NQ]) {
#pragma unroll 4
  for (int f = 0; f < Kf; ++f) {
    const uint32_t* r = dF + (size_t)f * W;
    uint32_t x[W];
#pragma unroll
    for (int c = 0; c < W; ++c) x[c] = r[c];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      uint32_t d = 0;
#pragma unroll
      for (int c = 0; c < W; ++c) d = bcnt_acc(x[c] ^ q[j][c], d);
      const uint32_t key = (d << 16) | (uint32_t)f;
      k2[j] = min(max(key, k1[j]), k2[j]);
      k1[j] = min(k1[j], key);
    }
  }
}

// Float32 descriptor rows (desc_type 1: SURF / SIFT, W = dimensions): squared L2 distance of every "from" row to the ONE
// "to" row this lane keeps in VGPRs, accumulated in float32 in dimension order, multiply and add unfused (the
// translation unit is built with -ffp-contract=off) -- the oracle's loop, bit for bit.  Strict comparisons: ties keep
// the lower "from" index (BFMatcher order); a NaN distance is never taken.
template <int W>
__device__ __forceinline__ void knn2_scan_l2(const uint32_t* __restrict__ dF, int Kf, const uint32_t (&q)[W], float& d1,
                                             float& d2, int& i1) {
#pragma unroll 1
  for (int f = 0; f < Kf; ++f) {
    const uint32_t* r = dF + (size_t)f * W;         // wave-uniform: scalar loads
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < W; ++c) {
      const float d = __uint_as_float(q[c]) - __uint_as_float(r[c]);
      s = s + d * d;
    }
    if (s < d1) { d2 = d1; d1 = s; i1 = f; }
    else if (s < d2) { d2 = s; }
  }
}

// The same scan for rows of more than 64 dimensions (SIFT: 128) without keeping the whole "to" row in registers: the
// 128 registers of the resident row left two wavefronts per SIMD to cover the scalar loads (9.8 ms per 2 048 pairs of
// K = 500 against an issue bound of 6.2, profiles/r05zb_float_descriptors.txt).  Here a lane walks the "from" rows in blocks
// of FB: the first 64 dimensions of the block's rows against the first half of its "to" row, then the second half -- one
// 64-register half resident at a time, re-read from L2 per block (256 B per lane against 3 x 64 x FB vector instructions),
// FB partial sums carried between the halves.  Per (from, to) pair the sum still runs over the dimensions in order: the
// same operations on the same values, the same bits.
template <int W>
__device__ __forceinline__ void knn2_scan_l2_halves(const uint32_t* __restrict__ dF, int Kf,
                                                    const uint32_t* __restrict__ qrow, float& d1, float& d2, int& i1) {
  static_assert(W == 128, "two halves of 64 dimensions");
  constexpr int H = 64, FB = 16;
#pragma unroll 1
  for (int f0 = 0; f0 < Kf; f0 += FB) {
    float s[FB];
#pragma unroll
    for (int j = 0; j < FB; ++j) s[j] = 0.f;
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      uint32_t q[H];
      {
        const uint4* p = reinterpret_cast<const uint4*>(qrow + half * H);
#pragma unroll
        for (int c = 0; c < H / 4; ++c) {
          const uint4 v = p[c];
          q[4 * c] = v.x; q[4 * c + 1] = v.y; q[4 * c + 2] = v.z; q[4 * c + 3] = v.w;
        }
      }
#pragma unroll
      for (int j = 0; j < FB; ++j) {
        if (f0 + j < Kf) {                                       // wave-uniform
          const uint32_t* r = dF + (size_t)(f0 + j) * W + half * H;   // wave-uniform: scalar loads
          float a = s[j];
#pragma unroll
          for (int c = 0; c < H; ++c) {
            const float d = __uint_as_float(q[c]) - __uint_as_float(r[c]);
            a = a + d * d;
          }
          s[j] = a;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < FB; ++j) {
      if (f0 + j < Kf) {
        if (s[j] < d1) { d2 = d1; d1 = s[j]; i1 = f0 + j; }
        else if (s[j] < d2) { d2 = s[j]; }
      }
    }
  }
}

template <int W>
__device__ __forceinline__ void load_desc(const uint32_t* __restrict__ base, int row, bool valid, uint32_t (&q)[W]) {
  const uint4* p = reinterpret_cast<const uint4*>(base + (size_t)(valid ? row : 0) * W);
#pragma unroll
  for (int c = 0; c < W / 4; ++c) {
    uint4 v = p[c];
    q[4 * c + 0] = v.x; q[4 * c + 1] = v.y; q[4 * c + 2] = v.z; q[4 * c + 3] = v.w;
  }
}

// W  : dwords per descriptor (8 / 16)
// NQ : "to" descriptors resident per lane
// NT : threads per workgroup (one workgroup per candidate pair)
// L2 : float32 descriptor rows of W dimensions (squared L2, NQ = 1) instead of binary rows of W dwords (Hamming)
template <int W, int NQ, int NT, bool L2 = false>
__global__ void __launch_bounds__(NT)
k_match_global(StoreView st, const int32_t* __restrict__ pair_from, const int32_t* __restrict__ pair_to,
               float nndr, int min_inliers, int est, uint32_t* __restrict__ corr, CorrHeader* __restrict__ hdr,
               PassState* __restrict__ pass, int32_t* __restrict__ list, int32_t* __restrict__ counter) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  const int pair = blockIdx.x;
  const int tid = threadIdx.x;
  const int kcap = st.kcap;
  MatchPair M;
  if (match_slot_outside(st, pair_from[pair], pair_to[pair])) { match_report_outside(hdr[pair], pass[pair]); return; }
  match_begin<NT>(st, pair_from[pair], pair_to[pair], smem, M);
  const int Kf = M.mF.x, Kt = M.mT.x;
  const uint32_t* dF = st.desc + (size_t)M.sF * kcap * W;
  const uint32_t* dT = st.desc + (size_t)M.sT * kcap * W;
  __syncthreads();

  int rejected = 0;
  if constexpr (L2) {
    static_assert(!L2 || NQ == 1, "one resident float row per lane");
    if (Kf > 0) {
      for (int base = 0; base < Kt; base += NT) {
        const int t = base + tid;
        float d1 = __int_as_float(0x7F800000), d2 = __int_as_float(0x7F800000);
        int i1 = -1;
        if constexpr (W > 64) {
          if (Kt - base - (tid & ~63) > 0)        // (wave-uniform: this wavefront holds at least one valid row)
            knn2_scan_l2_halves<W>(dF, Kf, dT + (size_t)(t < Kt ? t : 0) * W, d1, d2, i1);
        } else {
          uint32_t q[W];
          load_desc<W>(dT, t, t < Kt, q);
          if (Kt - base - (tid & ~63) > 0)
            knn2_scan_l2<W>(dF, Kf, q, d1, d2, i1);
        }
        if (t < Kt) {
          const bool acc = (Kf >= 2) && i1 >= 0 && !(d1 > nndr * d2);
          if (acc) match_claim(M.cnt, M.owner, i1, t);
          else ++rejected;
        }
      }
    }
  } else
  if (Kf > 0) {
    for (int base = 0; base < Kt; base += NQ * NT) {
      uint32_t q[NQ][W], k1[NQ], k2[NQ];
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const int t = base + j * NT + tid;
        load_desc<W>(dT, t, t < Kt, q[j]);
        k1[j] = 0xFFFFFFFFu;
        k2[j] = 0xFFFFFFFFu;
      }
      // wave-uniform: how many of this wave's NQ row groups hold at least one valid row?
      const int wave_rows = Kt - base - (tid & ~63);
      const int groups = wave_rows <= 0 ? 0 : min(NQ, (wave_rows + NT - 1) / NT);
      if (groups == NQ) {
        knn2_scan<W, NQ>(dF, Kf, q, k1, k2);
      } else if (groups > 0) {
        // ragged tail: scan only the populated groups (compile-time indices keep q[] in registers)
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          if (j < groups) {
            uint32_t qq[1][W], a1[1] = {0xFFFFFFFFu}, a2[1] = {0xFFFFFFFFu};
#pragma unroll
            for (int c = 0; c < W; ++c) qq[0][c] = q[j][c];
            knn2_scan<W, 1>(dF, Kf, qq, a1, a2);
            k1[j] = a1[0];
            k2[j] = a2[0];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const int t = base + j * NT + tid;
        if (t < Kt) {
          const bool acc = (Kf >= 2) && !((float)(k1[j] >> 16) > nndr * (float)(k2[j] >> 16));
          if (acc) match_claim(M.cnt, M.owner, (int)(k1[j] & 0xFFFFu), t);
          else ++rejected;
        }
      }
    }
  }
  match_finish<NT>(st, pair, M, min_inliers, est, rejected, corr + (size_t)pair * kcap, hdr[pair], pass[pair], list, counter);
}

// ------------------------------------------------------------------------------------------------
// Variant 2 ("LDS + u16"), shaped by the measured gfx950 VALU issue rates (tools/ubench/valu_rate.hip:
// v_xor_b32 VGPR,VGPR / v_min_u16 / v_max_u16 issue at full rate; v_bcnt_u32_b32, every 32-bit
// min/max, v_lshl_or_b32 and any VALU op with an SGPR operand at HALF rate):
//   * the "from" block is staged once into LDS and broadcast-read into VGPRs (uniform address: one
//     LDS cycle group, no conflicts), so the xor is VGPR x VGPR;
//   * best and second-best are tracked as 16-bit DISTANCES only (3 full-rate ops, no key packing);
//   * which "from" row holds the minimum is recovered afterwards, for accepted lanes only, by
//     re-scanning the 16-row chunk in which the running minimum last decreased (first row whose
//     distance equals the minimum = lowest index, the tie rule of the packed-key variant).
__device__ __forceinline__ uint32_t min_u16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ uint32_t max_u16(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

constexpr int MATCH_CH = 16;   // rows per index-recovery chunk

template <int W, int NQ>
__device__ __forceinline__ void knn2_step_lds(const uint32_t* fromD, int f, const uint32_t (&q)[NQ][W],
                                              uint32_t (&d1)[NQ], uint32_t (&d2)[NQ]) {
  const uint4* r = reinterpret_cast<const uint4*>(fromD + (size_t)f * W);   // same address in every lane
  uint32_t x[W];
#pragma unroll
  for (int c = 0; c < W / 4; ++c) {
    const uint4 v = r[c];
    x[4 * c] = v.x; x[4 * c + 1] = v.y; x[4 * c + 2] = v.z; x[4 * c + 3] = v.w;
  }
#pragma unroll
  for (int j = 0; j < NQ; ++j) {
    uint32_t d = 0;
#pragma unroll
    for (int c = 0; c < W; ++c) d = bcnt_acc(x[c] ^ q[j][c], d);
    d2[j] = min_u16(d2[j], max_u16(d, d1[j]));
    d1[j] = min_u16(d1[j], d);
  }
}

template <int W, int NQ>
__device__ __forceinline__ void knn2_scan_lds(const uint32_t* fromD, int Kf, const uint32_t (&q)[NQ][W],
                                              uint32_t (&d1)[NQ], uint32_t (&d2)[NQ], uint32_t (&chunk)[NQ]) {
  int c0 = 0;
  // full chunks: compile-time trip count, so the LDS reads of several rows are issued ahead
  for (; c0 + MATCH_CH <= Kf; c0 += MATCH_CH) {
    uint32_t prev[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) prev[j] = d1[j];
#pragma unroll 4
    for (int u = 0; u < MATCH_CH; ++u) knn2_step_lds<W, NQ>(fromD, c0 + u, q, d1, d2);
#pragma unroll
    for (int j = 0; j < NQ; ++j) chunk[j] = ((d1[j] & 0xFFFFu) != (prev[j] & 0xFFFFu)) ? (uint32_t)c0 : chunk[j];
  }
  if (c0 < Kf) {   // ragged last chunk
    uint32_t prev[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) prev[j] = d1[j];
    for (int f = c0; f < Kf; ++f) knn2_step_lds<W, NQ>(fromD, f, q, d1, d2);
#pragma unroll
    for (int j = 0; j < NQ; ++j) chunk[j] = ((d1[j] & 0xFFFFu) != (prev[j] & 0xFFFFu)) ? (uint32_t)c0 : chunk[j];
  }
}

// ------------------------------------------------------------------------------------------------
// Variant 3 ("fp4 matrix cores", NQ == 0): the K_from x K_to Hamming table as a matrix product.
// With every descriptor bit b mapped to the fp4 (E2M1) value 1 - 2b, the dot product of two rows is
// (bits - 2 * hamming); the coding actually used (fp4_spread_from / fp4_spread_to below) gives the same number
// minus a constant of the "to" row for 4 instead of 7 VALU ops per streamed dword.  The products are exact in
// fp4 and their sums (|.| <= 1024) are exact in the f32 accumulator, so the distances are the integers the VALU
// variants compute.  v_mfma_f32_32x32x64_f8f6f4
// does 32 x 32 x 64 of them per instruction (tools/ubench/mfma_fp4_hamming.hip pins operand layout and
// exactness on the device); the order of the 64 bits inside one instruction is irrelevant as long as
// both operands use the same one, so a lane simply spreads the raw dwords it loaded.
//   * "from" rows = matrix rows (A, re-read from the LDS copy per 32-row tile), "to" rows = columns
//     (B, kept in VGPRs for the whole scan); a wavefront owns 32-column tiles, two at a time;
//   * the accumulator starts at -(from row index)/2048 instead of 0, so one f32 per (from, to) cell
//     orders by distance first (steps of 2) and by the LOWER from index second (fraction < 1): the
//     BFMatcher tie rule with no separate index bookkeeping;
//   * best per column exactly, second best optimistically (top2_update16: 10 ops per 16 cells), one cross-half merge,
//     and, for a column that passes NNDR, the decision again on the best row's class (mf_repair_accept: once per group).
typedef int mf_v8i __attribute__((ext_vector_type(8)));
typedef float mf_v16f __attribute__((ext_vector_type(16)));
constexpr float MF_FR = 1.f / 2048.f;        // index fraction (kcap <= 2048 rows on this path)
constexpr int MF_MAX_ROWS = 2048;

// 32 descriptor bits -> 32 fp4 (E2M1) values, 4 dwords of nibbles.  The streamed operand (the "from" rows, spread
// once per tile by every wavefront) must be cheap, so its bits stay where they are: dword k of the result keeps
// the bits at nibble position 3 - k of the raw dword,
//   position 3: sign bit of 1.0          -> +1 / -1          (x & 0x8888.. | 0x2222..)
//   position 2: exponent bit, code 0100  ->  0 / 2.0         (x & 0x4444..)
//   position 1: exponent bit, code 0010  ->  0 / 1.0         (x & 0x2222..)
//   position 0: mantissa bit, code 0001  ->  0 / 0.5         (x & 0x1111..)
// 4 VALU ops per raw dword (the all-sign form ((x << k) & 0x8888..) | 0x2222.. costs 7).  With t = +1 / -1 for a
// bit 0 / 1, an element of the last three classes is a = d (1 - tx), d = 1, 1/2, 1/4; the resident operand (the
// "to" rows, spread once per pass) answers with b = -ty / d = -+1, -+2, -+4 (codes 0x2, 0x4, 0x6 under the sign),
// so a b = tx ty - ty, and the sign class contributes tx ty directly:
//   dot = (bits - 2 hamming) - sum_{classes 2,1,0} ty = (bits - 2 hamming) - (3 bits / 4 - 2 popc(y & 0x7777..)).
// The second term is a constant of the "to" row: it shifts every score of a column alike (best / second best and
// the tie rule are untouched) and is taken out when the distances are decoded.  Products and sums are exact.
// m88 / c22 hold 0x88888888 / 0x22222222 in VGPRs the compiler cannot see through (knn2_mfma): a VOP3 cannot
// encode a literal on gfx9, so v_and_or_b32 needs them in registers.  No asm on this path: the results are MFMA
// operands and the hazard recogniser must see the instructions that write them.
__device__ __forceinline__ mf_v8i fp4_spread_from(uint32_t x, uint32_t m88, uint32_t c22) {
  mf_v8i o = {0, 0, 0, 0, 0, 0, 0, 0};
  o[0] = (int)((x & m88) | c22);
  o[1] = (int)(x & 0x44444444u);
  o[2] = (int)(x & 0x22222222u);
  o[3] = (int)(x & 0x11111111u);
  return o;
}
// The three shifted classes carry the NEGATED bit under the sign: (~y << k) & 0x8888.. | code.  Written as the bit-field
// insert code' ^ ((y << k) & (code ^ code')) with code' = code | 0x8888.. -- where the shifted bit is set the code alone,
// elsewhere the code under a set sign -- it is one three-input instruction behind the shift (v_bfi_b32 / v_bitop3_b32) and
// needs no ~y: 7 VALU ops per raw dword instead of 8.  The compiler forms it only from constants it cannot see through
// (FpB: the codes in scalar registers, the signed codes in VGPRs, mf_load_b); with literals it folds the expression
// back into a negation and three v_and_or_b32.
struct FpB {
  uint32_t c2, c4, c6;   // 0x2222.., 0x4444.., 0x6666..
  uint32_t e2, e4, e6;   // the same under 0x8888..
};
__device__ __forceinline__ mf_v8i fp4_spread_to(uint32_t y, uint32_t m88, uint32_t c22, const FpB& K) {
  mf_v8i o = {0, 0, 0, 0, 0, 0, 0, 0};
  o[0] = (int)((y & m88) | c22);
  o[1] = (int)(K.e2 ^ ((y << 1) & (K.c2 ^ K.e2)));
  o[2] = (int)(K.e4 ^ ((y << 2) & (K.c4 ^ K.e4)));
  o[3] = (int)(K.e6 ^ ((y << 3) & (K.c6 ^ K.e6)));
  return o;
}

// Dynamic LDS of the LDS-staged matching body: the staged "from" descriptors, the per-row counters / owners and 16 words.
// The MFMA scan requests a tile's rows one tile ahead without clamping the row number, i.e. up to 32 rows past the
// staged block: the words behind it must exist (they are the counters, or padding when kcap is small).
static inline size_t sf_match_lds_bytes(int kcap, int w) {
  const int behind = 2 * kcap + 16;
  return (size_t)(kcap * w + (behind > 32 * w ? behind : 32 * w)) * sizeof(int);
}

template <int KS>
__device__ __forceinline__ void load_raw(const uint32_t* p, uint32_t (&raw)[KS]) {
#pragma unroll
  for (int c = 0; c < KS / 4; ++c) {
    const uint4 v = reinterpret_cast<const uint4*>(p)[c];
    raw[4 * c] = v.x; raw[4 * c + 1] = v.y; raw[4 * c + 2] = v.z; raw[4 * c + 3] = v.w;
  }
}

// The scan's running pair per lane and column tile: b, the best score, EXACT; s, an OPTIMISTIC second best (<= the exact
// one).  A tuple v[0..15] (one 32-row "from" tile, one lane half) meets (b, s) as two values, the maximum m of v[0..14]
// and v[15]:  x = med3(b, m, v15) is the second largest of {b, m, v15}, b' = max3(b, m, v15), s' = max(s, x) -- 10 VALU
// ops per tuple in the pipelined statements below (7 for m + 3) against the 20 of an exact top-2 per value pair.
//   CLASS MAP.  Register i of a tuple holds row (i & 3) + 8 * (i >> 2) + 4 * h of its tile (h = lane half), so the rows of
//   one "from" tile T fall into four classes: for h = 0, 1 the 15 rows T * 32 + 4 * h + {0..3, 8..11, 16..19, 24..26}
//   (registers 0..14) and the single row T * 32 + 27 + 4 * h (register 15).  b is the maximum over all rows, as before;
//   s is the second largest of the CLASS MAXIMA, i.e. the best score among the rows outside the best row's class.
// The exact second best is therefore max(s, best of the OTHER rows of the best row's class): s decodes to a distance
// d2' >= d2, the only consumer of d2 is the NNDR test of match_v2_body, a column that fails it against d2' fails it
// against d2, and a column that passes has its class looked at again there (mf_repair_accept: certified on half rows,
// exactly otherwise -- mf_repair_d2) -- docs/match_second_best.md, docs/match_repair_once.md,
// tests/test_match_lazy_second_model.py, tests/test_match_half_bound_model.py.
// Written as asm because fmaxf() costs a canonicalising self-max per operand; the FIRST read of the accumulator is
// left to the compiler (a builtin: med3(v0, v1, +inf) = max(v0, v1), hence 11 ops on this unpipelined path), which
// places the MFMA-result wait states in front of it -- the hazard recogniser does not look inside an asm statement.
__device__ __forceinline__ void top2_update16(const mf_v16f& v, float& b, float& s) {
  float t = __builtin_amdgcn_fmed3f(v[0], v[1], INFINITY);
  float x;
  asm("v_max3_f32 %[t], %[t], %[o2], %[o3]\n\t"
      "v_max3_f32 %[t], %[t], %[o4], %[o5]\n\t"
      "v_max3_f32 %[t], %[t], %[o6], %[o7]\n\t"
      "v_max3_f32 %[t], %[t], %[o8], %[o9]\n\t"
      "v_max3_f32 %[t], %[t], %[o10], %[o11]\n\t"
      "v_max3_f32 %[t], %[t], %[o12], %[o13]\n\t"
      "v_max_f32 %[t], %[t], %[o14]\n\t"
      "v_med3_f32 %[x], %[b], %[t], %[o15]\n\t"
      "v_max3_f32 %[b], %[b], %[t], %[o15]\n\t"
      "v_max_f32 %[s], %[s], %[x]"
      : [b] "+v"(b), [s] "+v"(s), [t] "+v"(t), [x] "=&v"(x)
      : [o2] "v"(v[2]), [o3] "v"(v[3]), [o4] "v"(v[4]), [o5] "v"(v[5]), [o6] "v"(v[6]), [o7] "v"(v[7]), [o8] "v"(v[8]),
        [o9] "v"(v[9]), [o10] "v"(v[10]), [o11] "v"(v[11]), [o12] "v"(v[12]), [o13] "v"(v[13]), [o14] "v"(v[14]),
        [o15] "v"(v[15]));
}

// One 32-row "from" tile against the NTL resident "to" tiles of this wavefront.
// `raw` holds this tile's rows, requested one tile ahead (an LDS round trip, ~100 cycles, no longer opens every
// iteration of a wavefront's scan: k_verify_fused 0.469 -> 0.457 ms per 10 000 pairs); the next tile's are requested
// here, behind the spread that consumes these.
template <int W, int NTL, bool TAIL>
__device__ __forceinline__ void knn2_mfma_tile(const uint32_t* fromD, int Kf, int mt, int r, int h,
                                               const mf_v8i (&Bf)[NTL][W / 2], const float (&cin)[16],
                                               float (&b)[NTL], float (&s)[NTL], uint32_t m88, uint32_t c22,
                                               uint32_t (&raw)[W / 2], const uint32_t*& nxt) {
  constexpr int KS = W / 2;
  // every tile starts from the SAME accumulator tuple (the MFMA reads it as its C operand: no copy).  The ragged last
  // tile's copy has -inf in its missing rows (-inf + any finite product sum = -inf: the top-2 update never takes them,
  // whatever the LDS words behind the staged block hold); it is made here, from the tuple's own values, for the one tile
  // that needs it -- kept across the scan it cost 16 registers.
  mf_v16f c0;
#pragma unroll
  for (int i = 0; i < 16; ++i) c0[i] = cin[i];
  if (TAIL) {
    // register i holds -(its row in the tile) / 2048: the row exists when that is above -(rows left) / 2048
    const float lim = -(float)(Kf - mt * 32) * MF_FR;
#pragma unroll
    for (int i = 0; i < 16; ++i) c0[i] = c0[i] > lim ? c0[i] : -INFINITY;
  }
  mf_v8i Af[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) Af[k] = fp4_spread_from(raw[k], m88, c22);
  if (!TAIL) {
    // the next tile's rows: a running address, no clamp -- rows past Kf (the ragged last tile's missing ones, or a whole
    // tile that is never used when Kf is a multiple of 32) lie inside the workgroup's LDS block (at most 32 rows past
    // the staged descriptors: the counters behind them, sf_match_lds_bytes), spread to valid fp4 whatever their bits,
    // and are masked behind the products
    nxt += 32 * W;
    load_raw<KS>(nxt, raw);
  }
  // the scores kept so far move with the origin (the first row of the current tile).  Plain adds: rounds 2-4 paired them
  // in v_pk_add_f32 with the step in an SGPR pair -- packed f32 beside MFMAs costs more issue time than the two adds it
  // replaces (MI355X_MICROARCH.md, cycle constants), and since round 5 no packed-f32 instruction with a scalar source is
  // left in this translation unit (tools/pk_isa_scan.py --strict: the build gate of DESIGN.md section 3).
#pragma unroll
  for (int j = 0; j < NTL; ++j) {
    b[j] += 32.f * MF_FR;
    s[j] += 32.f * MF_FR;
  }
#pragma unroll
  for (int j = 0; j < NTL; ++j) {
    mf_v16f acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(Af[0], Bf[j][0], c0, 4, 4, 0, 0, 0, 0);
#pragma unroll
    for (int k = 1; k < KS; ++k)
      acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(Af[k], Bf[j][k], acc, 4, 4, 0, 0, 0, 0);
    top2_update16(acc, b[j], s[j]);
  }
}

// kNN-2 of the "to" rows of NTL 32-column tiles over all "from" rows; on return lanes 0..31 hold, for
// column tile[j] * 32 + lane: d1 / d2 (Hamming, 0xFFFF when absent) and the from index of d1.
// The resident "to" operands of one scan: NTL column tiles spread to fp4, the columns' constants.
template <int W, int NTL>
struct MfB {
  mf_v8i Bf[NTL][W / 2];
  uint32_t psum;   // popc(row & 0x7777...) of the NTL tiles' columns, 8 bits per tile (NTL == 1: the whole word)
};

// Loads and spreads the "to" rows of the tiles tile[0..NTL); Kt >= 1.  A column past the frame's rows holds the
// frame's last row: its scores are computed and never read (the callers decide for columns < Kt only), which costs
// nothing and spares the branch around the load.  All tiles' loads are issued before the first is waited for: one
// HBM round trip per group instead of one per tile.
template <int W, int NTL>
__device__ __forceinline__ void mf_load_b(const uint32_t* __restrict__ dT, int Kt, const int (&tile)[NTL], int lane,
                                          MfB<W, NTL>& B) {
  constexpr int KS = W / 2;
  const int r = lane & 31, h = lane >> 5;
  uint32_t m88, c22;   // constants pinned in VGPRs (see fp4_spread)
  asm volatile("v_mov_b32 %0, 0x88888888" : "=v"(m88));
  asm volatile("v_mov_b32 %0, 0x22222222" : "=v"(c22));
  FpB K;
  asm volatile("s_mov_b32 %0, 0x22222222" : "=s"(K.c2));
  asm volatile("s_mov_b32 %0, 0x44444444" : "=s"(K.c4));
  asm volatile("s_mov_b32 %0, 0x66666666" : "=s"(K.c6));
  asm volatile("v_mov_b32 %0, 0xaaaaaaaa" : "=v"(K.e2));
  asm volatile("v_mov_b32 %0, 0xcccccccc" : "=v"(K.e4));
  asm volatile("v_mov_b32 %0, 0xeeeeeeee" : "=v"(K.e6));
  uint32_t raw[NTL][KS];
#pragma unroll
  for (int j = 0; j < NTL; ++j) load_raw<KS>(dT + (size_t)min(tile[j] * 32 + r, Kt - 1) * W + KS * h, raw[j]);
  // the columns' constants (see fp4_spread_from) travel as their popcounts, one byte per tile: one register across the
  // scan and one exchange between the row halves instead of NTL of each
  static_assert(NTL == 1 || 24 * W < 256, "a tile's popcount fits its byte");
  uint32_t pk = 0;
#pragma unroll
  for (int j = 0; j < NTL; ++j) {
    uint32_t p = 0;
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      B.Bf[j][k] = fp4_spread_to(raw[j][k], m88, c22, K);
      p += __popc(raw[j][k] & 0x77777777u);
    }
    pk |= p << (8 * j);
  }
  B.psum = pk + __shfl_xor(pk, 32);         // both halves of the row
}

// ---- round 5: the scan software-pipelined inside a wavefront (256-bit descriptors) -------------------------------------
// knn2_mfma_tile above runs, per column tile, 4 dependent MFMAs, waits for the result (s_nop 11), then the dependent
// vector instructions that consume it (20 when this was written, 11 now), on ONE accumulator tuple: nothing of a wavefront's
// own stream overlaps -- matrix-pipe time (4 x 32 cycles per 32 x 32 tile pair) and vector issue time (MI355X_MICROARCH.md,
// cycle constants) only overlap between the wavefronts that share a SIMD.
// Here the update of tile j - 1 is issued in the gaps of tile j's MFMAs, from a SECOND accumulator tuple: three vector
// instructions per 32-cycle gap (five to six with the exact top-2 update; their issue cost 8 + 3 x 4 leaves the gap to the
// matrix pipe, docs/match_second_best.md), so a tile pair costs the matrix pipe's 128 cycles plus what stays outside (the
// spread of the "from" tile, the loop).  Measured (profiles/r05s_*, r05zc_*): the
// cfg3-shaped launch 10.8 -> 10.0 ms per 100 000 pairs with the matrix pipe 75 % busy at the 1.69 GHz the chip sustains
// under it, and ONE workgroup per CU now reaches 96 % of the rate of three.  The MFMAs have to sit in the asm statements
// with the vector instructions (the compiler does not interleave an asm block with builtins), so the wait states are
// written out by hand (cdna_hip_programming.md section 5.7 item 2):
//   * a VALU-written A operand -> MFMA: s_nop 1 opens the first half (the spread is compiler code right in front); the
//     second half's A operands are inputs of the first half too, so they are written before it;
//   * an MFMA result -> a VALU reader: 12 states after the LAST MFMA of the tuple.  The old tuple's last MFMA is followed
//     by 3 vector instructions (the end of the second half), then s_nop 1 (2), the new tile's first MFMA (1), the two
//     origin shifts (2) and s_nop 4 (5) stand in front of the first read: 13.  The drain opens with s_nop 11;
//   * an accumulate chain (the MFMA takes the previous result whole as C) needs none.
// A statement's operands are limited to 30, hence two halves per tile (2 MFMAs each; the first reduces registers 0..8 of
// the old tuple, the second 9..14 and merges the maximum and register 15 into b and s).  The same classes as
// top2_update16: b is the same value, s the same second largest of the class maxima.
typedef int mf_v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void mf_pipe_half1(mf_v16f& acc, const mf_v4i& a0, const mf_v4i& a1, const mf_v4i& a2,
                                              const mf_v4i& a3, const mf_v4i& b0, const mf_v4i& b1, const mf_v16f& cin,
                                              const mf_v16f& old, float& b, float& s, float& t) {
  asm volatile(
      "s_nop 1\n\t"
      "v_mfma_f32_32x32x64_f8f6f4 %[acc], %[a0], %[b0], %[cin] cbsz:4 blgp:4\n\t"
      "v_add_f32 %[b], 0x3c800000, %[b]\n\t"            // the origin moves by one tile: 32 / 2048
      "v_add_f32 %[s], 0x3c800000, %[s]\n\t"
      "s_nop 4\n\t"
      "v_max3_f32 %[t], %[o0], %[o1], %[o2]\n\t"
      "v_mfma_f32_32x32x64_f8f6f4 %[acc], %[a1], %[b1], %[acc] cbsz:4 blgp:4\n\t"
      "v_max3_f32 %[t], %[t], %[o3], %[o4]\n\t"
      "v_max3_f32 %[t], %[t], %[o5], %[o6]\n\t"
      "v_max3_f32 %[t], %[t], %[o7], %[o8]"
      : [acc] "=&v"(acc), [b] "+v"(b), [s] "+v"(s), [t] "=&v"(t)
      : [a0] "v"(a0), [a1] "v"(a1), "v"(a2), "v"(a3), [b0] "v"(b0), [b1] "v"(b1), [cin] "v"(cin), [o0] "v"(old[0]),
        [o1] "v"(old[1]), [o2] "v"(old[2]), [o3] "v"(old[3]), [o4] "v"(old[4]), [o5] "v"(old[5]), [o6] "v"(old[6]),
        [o7] "v"(old[7]), [o8] "v"(old[8]));
}
__device__ __forceinline__ void mf_pipe_half2(mf_v16f& acc, const mf_v4i& a2, const mf_v4i& a3, const mf_v4i& b2,
                                              const mf_v4i& b3, const mf_v16f& old, float& b, float& s, float& t) {
  float x;
  asm volatile(
      "v_mfma_f32_32x32x64_f8f6f4 %[acc], %[a2], %[b2], %[acc] cbsz:4 blgp:4\n\t"
      "v_max3_f32 %[t], %[t], %[o9], %[o10]\n\t"
      "v_max3_f32 %[t], %[t], %[o11], %[o12]\n\t"
      "v_max3_f32 %[t], %[t], %[o13], %[o14]\n\t"
      "v_mfma_f32_32x32x64_f8f6f4 %[acc], %[a3], %[b3], %[acc] cbsz:4 blgp:4\n\t"
      "v_med3_f32 %[x], %[b], %[t], %[o15]\n\t"
      "v_max3_f32 %[b], %[b], %[t], %[o15]\n\t"
      "v_max_f32 %[s], %[s], %[x]"
      : [acc] "+v"(acc), [b] "+v"(b), [s] "+v"(s), [t] "+v"(t), [x] "=&v"(x)
      : [a2] "v"(a2), [a3] "v"(a3), [b2] "v"(b2), [b3] "v"(b3), [o9] "v"(old[9]), [o10] "v"(old[10]), [o11] "v"(old[11]),
        [o12] "v"(old[12]), [o13] "v"(old[13]), [o14] "v"(old[14]), [o15] "v"(old[15]));
}
// the pending tuple's update with no tile behind it (end of the full tiles)
__device__ __forceinline__ void mf_pipe_drain(const mf_v16f& old, float& b, float& s) {
  float t, x;
  asm volatile(
      "s_nop 11\n\t"
      "v_add_f32 %[b], 0x3c800000, %[b]\n\t"
      "v_add_f32 %[s], 0x3c800000, %[s]\n\t"
      "v_max3_f32 %[t], %[o0], %[o1], %[o2]\n\t"
      "v_max3_f32 %[t], %[t], %[o3], %[o4]\n\t"
      "v_max3_f32 %[t], %[t], %[o5], %[o6]\n\t"
      "v_max3_f32 %[t], %[t], %[o7], %[o8]\n\t"
      "v_max3_f32 %[t], %[t], %[o9], %[o10]\n\t"
      "v_max3_f32 %[t], %[t], %[o11], %[o12]\n\t"
      "v_max3_f32 %[t], %[t], %[o13], %[o14]\n\t"
      "v_med3_f32 %[x], %[b], %[t], %[o15]\n\t"
      "v_max3_f32 %[b], %[b], %[t], %[o15]\n\t"
      "v_max_f32 %[s], %[s], %[x]"
      : [b] "+v"(b), [s] "+v"(s), [t] "=&v"(t), [x] "=&v"(x)
      : [o0] "v"(old[0]), [o1] "v"(old[1]), [o2] "v"(old[2]), [o3] "v"(old[3]), [o4] "v"(old[4]), [o5] "v"(old[5]),
        [o6] "v"(old[6]), [o7] "v"(old[7]), [o8] "v"(old[8]), [o9] "v"(old[9]), [o10] "v"(old[10]), [o11] "v"(old[11]),
        [o12] "v"(old[12]), [o13] "v"(old[13]), [o14] "v"(old[14]), [o15] "v"(old[15]));
}

// all "from" tiles of a scan in the pipelined form (W = 8, NTL even: tile j writes tuple j & 1 and consumes the other).
// The ragged last tile (Kf & 31 rows) goes through the same statements as a peeled last iteration: its missing rows are
// masked in the ORIGIN tuple (-inf + any finite product sum = -inf, so the top-2 update never takes them, whatever the
// LDS words behind the staged block hold), 16 selects per "from" tile instead of 16 per column tile behind the
// products.  The origin tuple is dead after the last tile, so it is masked in place: no second tuple lives across the
// scan (docs/notebook_r05.md section 13 lost to that one's scratch).  `tail` = Kf & 31 (wave-uniform).
template <int NTL>
__device__ __forceinline__ void mf_scan_tiles_pipe(const uint32_t* fromD, int n_full, int tail, const MfB<8, NTL>& B,
                                                   const float (&cin)[16], float (&b)[NTL], float (&s)[NTL],
                                                   uint32_t m88, uint32_t c22, uint32_t (&raw)[4],
                                                   const uint32_t*& nxt) {
  static_assert(NTL == 2 || NTL == 4, "tiles alternate between two accumulator tuples");
  mf_v4i B4[NTL][4];
#pragma unroll
  for (int j = 0; j < NTL; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) B4[j][k] = mf_v4i{B.Bf[j][k][0], B.Bf[j][k][1], B.Bf[j][k][2], B.Bf[j][k][3]};
  }
  mf_v16f c0, acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { c0[i] = cin[i]; acc1[i] = -INFINITY; }     // nothing pending: an update that changes nothing
  // two passes over ONE loop body: the full tiles, then the ragged tile with its missing rows masked in the origin tuple
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    int n = n_full, step = 32 * 8;       // words to the next tile's rows; the ragged tile has none behind it
    if (pass) {
      if (!tail) break;
      // register i holds -(its row in the tile) / 2048: the row exists when that is above -tail / 2048 (exact in f32).
      // Compared as floats against the tuple itself, so that the 16 masks are made here and not kept in 32 scalar
      // registers across the kernel.  The selects are compiler code: the wait states of a VALU-written C operand are
      // the ones the A operands need anyway (s_nop 1 opens mf_pipe_half1).
      const float lim = -(float)tail * MF_FR;
#pragma unroll
      for (int i = 0; i < 16; ++i) c0[i] = c0[i] > lim ? c0[i] : -INFINITY;
      n = 1; step = 0;
    }
    for (int mt = 0; mt < n; ++mt) {
      mf_v4i A4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const mf_v8i a = fp4_spread_from(raw[k], m88, c22);
        A4[k] = mf_v4i{a[0], a[1], a[2], a[3]};
      }
      nxt += step;                       // the next tile's rows (see knn2_mfma_tile)
      load_raw<4>(nxt, raw);
#pragma unroll
      for (int j = 0; j < NTL; j += 2) {
        constexpr int JP = NTL - 1;      // tile 0 consumes the LAST tile of the previous "from" tile
        float t;
        const int jp = j == 0 ? JP : j - 1;
        mf_pipe_half1(acc0, A4[0], A4[1], A4[2], A4[3], B4[j][0], B4[j][1], c0, acc1, b[jp], s[jp], t);
        mf_pipe_half2(acc0, A4[2], A4[3], B4[j][2], B4[j][3], acc1, b[jp], s[jp], t);
        mf_pipe_half1(acc1, A4[0], A4[1], A4[2], A4[3], B4[j + 1][0], B4[j + 1][1], c0, acc0, b[j], s[j], t);
        mf_pipe_half2(acc1, A4[2], A4[3], B4[j + 1][2], B4[j + 1][3], acc0, b[j], s[j], t);
      }
    }
  }
  mf_pipe_drain(acc1, b[NTL - 1], s[NTL - 1]);
}

// v_max_f32 / v_min_f32 / v_max3_f32 as they are: fmaxf() and fminf() put a canonicalising self-max in front of every
// operand the compiler cannot prove quiet, and the scores are never NaN.
__device__ __forceinline__ float mf_max(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float mf_min(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float mf_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// decode passes of a scan over NTL column tiles: a pass decides two tiles, one per lane half
constexpr int mf_passes(int ntl) { return ntl == 1 ? 1 : ntl / 2; }

// kNN-2 of the resident "to" columns over all "from" rows.  On return, NTL == 1: lanes 0..31 hold, for column
// tile[0] * 32 + lane, d1 / d2 (Hamming, 0xFFFF when absent) and the from index of d1.  NTL even: in pass p ALL lanes
// hold them, for column tile[2 p + (lane >> 5)] * 32 + (lane & 31) -- a column's scores live in lanes r and r + 32 (one
// half of a tile's rows each), so each half sends the other the tile that one decodes: one exchange per value and pass,
// one decode for two tiles.
// d1 and its index are exact; d2 is the OPTIMISTIC second best (>= the exact one: the best distance among the rows outside
// the best row's class, top2_update16) -- its one consumer, the NNDR test of match_v2_body, decides again on the class
// where it matters.
template <int W, int NTL, bool PIPE = false>
__device__ __forceinline__ void mf_scan(const uint32_t* fromD, int Kf, const MfB<W, NTL>& B, int lane,
                                        uint32_t (&d1)[mf_passes(NTL)], uint32_t (&d2)[mf_passes(NTL)],
                                        int (&idx)[mf_passes(NTL)]) {
  constexpr int KS = W / 2;
  const int r = lane & 31, h = lane >> 5;
  uint32_t m88, c22;
  asm volatile("v_mov_b32 %0, 0x88888888" : "=v"(m88));
  asm volatile("v_mov_b32 %0, 0x22222222" : "=v"(c22));
  float cin[16], b[NTL], s[NTL];
  // the origin tuple is rebuilt by every scan (16 subtractions; knn2_mfma made `lane` opaque): hoisted out of the
  // column-group loop it would have to survive the in-place masking of the ragged tile as a second tuple
  // (mf_scan_tiles_pipe)
  const float hoff = h ? 4.f * MF_FR : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) cin[i] = -(float)((i & 3) + 8 * (i >> 2)) * MF_FR - hoff;   // a literal minus 4 h / 2048: exact
#pragma unroll
  for (int j = 0; j < NTL; ++j) { b[j] = -INFINITY; s[j] = -INFINITY; }
  const int n_full = Kf >> 5;
  uint32_t raw[KS];
  load_raw<KS>(fromD + (size_t)min(r, Kf - 1) * W + KS * h, raw);
  const uint32_t* nxt = fromD + (size_t)r * W + KS * h;
  if constexpr (PIPE && W == 8 && (NTL == 2 || NTL == 4)) {
    mf_scan_tiles_pipe<NTL>(fromD, n_full, Kf & 31, B, cin, b, s, m88, c22, raw, nxt);
  } else {
    for (int mt = 0; mt < n_full; ++mt) knn2_mfma_tile<W, NTL, false>(fromD, Kf, mt, r, h, B.Bf, cin, b, s, m88, c22, raw, nxt);
    if (Kf & 31) knn2_mfma_tile<W, NTL, true>(fromD, Kf, n_full, r, h, B.Bf, cin, b, s, m88, c22, raw, nxt);
  }
  const float org = (float)(32 * (((Kf + 31) >> 5) - 1)) * MF_FR;
#pragma unroll
  for (int p = 0; p < mf_passes(NTL); ++p) {
    float mb, ms, ob, os;      // this lane's half of the column's rows, the other half's
    int ts;                    // the column's constant
    if constexpr (NTL == 1) {
      mb = b[0]; ms = s[0]; ts = 24 * W - 2 * (int)B.psum;
      ob = __shfl_xor(mb, 32); os = __shfl_xor(ms, 32);
    } else {
      const int j0 = 2 * p, j1 = 2 * p + 1;
      mb = h ? b[j1] : b[j0]; ms = h ? s[j1] : s[j0]; ts = 24 * W - 2 * (int)((B.psum >> (16 * p + 8 * h)) & 0xFFu);
      ob = __shfl_xor(h ? b[j0] : b[j1], 32); os = __shfl_xor(h ? s[j0] : s[j1], 32);
    }
    const float nb = mf_max(mb, ob) - org;
    const float ns = mf_max3(mf_min(mb, ob), ms, os) - org;
    const float dot1 = 2.f * ceilf(nb * 0.5f), dot2 = 2.f * ceilf(ns * 0.5f);
    idx[p] = (int)((dot1 - nb) * 2048.f);
    d1[p] = (uint32_t)((32 * W - ts - (int)dot1) >> 1);
    d2[p] = ns == -INFINITY ? 0xFFFFu : (uint32_t)((32 * W - ts - (int)dot2) >> 1);
  }
}

template <int W, int NTL, bool PIPE = false>
__device__ __forceinline__ void knn2_mfma(const uint32_t* fromD, int Kf, const uint32_t* __restrict__ dT, int Kt,
                                          const int (&tile)[NTL], int lane, uint32_t (&d1)[mf_passes(NTL)],
                                          uint32_t (&d2)[mf_passes(NTL)], int (&idx)[mf_passes(NTL)]) {
  // what a scan derives from the lane number (row, lane half, LDS addresses) is derived again by every scan: kept across
  // the column-group loop it would sit in registers that the scan itself is short of, i.e. in scratch
  asm volatile("" : "+v"(lane));
  MfB<W, NTL> B;
  mf_load_b<W, NTL>(dT, Kt, tile, lane, B);
  mf_scan<W, NTL, PIPE>(fromD, Kf, B, lane, d1, d2, idx);
}

// The exact second-best distance of a column that passed NNDR against the scan's optimistic one (top2_update16: CLASS
// MAP).  The scan's d2 is the best distance among the rows outside the best row's class, so the exact one is the minimum
// of it and the distances of the class's OTHER rows, computed here by xor + popcount from the staged "from" block and the
// column's own row `q_row` (global, L2-warm: mf_load_b has just read it).  The class of best row idx: its tile
// idx & ~31, its lane half idx & 4, registers 0..14 = rows + {0..3, 8..11, 16..19, 24..26}; row 27 of the half (register
// 15) is a class of its own, with nothing to repair.  Rows >= Kf are left out (the LDS behind the staged rows holds the
// counters; the reads stay inside the block, sf_match_lds_bytes), and so is the best row itself.  Per lane: only lanes
// that the half-row certificate of mf_repair_accept left undecided call it (all repairing lanes when nndr < 0).
template <int W>
__device__ __forceinline__ uint32_t mf_repair_d2(const uint32_t* fromD, int Kf, const uint32_t* __restrict__ q_row, int idx,
                                                 uint32_t d2) {
  if ((idx & 27) == 27) return d2;             // rows 27 and 31 of a tile
  uint32_t q[W];
  load_raw<W>(q_row, q);
  const int base = (idx & ~31) + (idx & 4);
#pragma unroll 1
  for (int g = 0; g < 32; g += 8) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int row = base + g + k;
      uint32_t x[W];
      load_raw<W>(fromD + (size_t)row * W, x);
      uint32_t d = 0;
#pragma unroll
      for (int c = 0; c < W; ++c) d = bcnt_acc(x[c] ^ q[c], d);
      const bool other = row < Kf && row != idx && (g + k) != 27;
      d2 = other ? min(d2, d) : d2;
    }
  }
  return d2;
}

// popc(mask & lanes below this one)
__device__ __forceinline__ int mf_rank_below(unsigned long long mask) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// The NNDR decision of a column that passed against the optimistic d2 -- the decision, not a distance: the exact d2 has no
// other consumer (docs/match_repair_once.md).  For nndr >= 0 the predicate !((float)d1 > nndr * (float)d2) is monotone
// non-decreasing in d2, and the Hamming distance p over a row's first four dwords is <= the row's distance d.  So with
// pmin = the minimum of p over the class's other rows (the exclusions of mf_repair_d2), min(d2, pmin) <= the exact second
// best: a column that passes against it passes against the exact one, on one ds_read_b128 and four xor / popcount per row
// and ONE conversion, multiply and compare for the class.  A column that does not pass is not rejected: it is
// uncertified, and under a wave-uniform ballot the uncertified lanes run the exact loop and decide as before.  A negative
// (or NaN) nndr keeps the exact path as a whole: the predicate is not monotone there.
// Called under wave-uniform control flow with the lanes that repair in `active`; returns the decision of those lanes.
template <int W>
__device__ __forceinline__ bool mf_repair_accept(const uint32_t* fromD, int Kf, const uint32_t* __restrict__ q_row, int idx,
                                                 uint32_t d1, uint32_t d2, float nndr, bool active) {
  bool acc = false, exact = active;
  if (nndr >= 0.f) {                             // a kernel argument: wave-uniform
    if (active) {
      uint32_t pmin = d2;
      if ((idx & 27) != 27) {                    // (rows 27 and 31 of a tile: nothing to repair, d2 is exact)
        uint32_t q[4];
        load_raw<4>(q_row, q);
        const int base = (idx & ~31) + (idx & 4);
        // The exclusions as ONE instruction per row: bit j of `no` is set where row base + j is left out (rows >= Kf: bits
        // Kf - base and up, at least 1 as idx < Kf; the best row; bit 27, register 15's row), and a row's popcount chain
        // starts from its bit moved to 512 or above instead of from 0.  A row left out then counts 512 or more: no less
        // than any distance of up to 512 bits, so the minimum with d2 is untouched (a second best that is absent, 0xFFFF,
        // comes out at 512 or more instead: smaller, i.e. at worst uncertified, never wrongly certified).  `no` is kept
        // rotated left by 9, and right by 8 per trip: row g + k sits at bit 9 + k.
        const uint32_t ok = ((1u << min(Kf - base, 31)) - 1u) & ~(1u << (idx - base)) & ~(1u << 27);
        uint32_t no = __builtin_amdgcn_alignbit(~ok, ~ok, 23);
#pragma unroll 1
        for (int g = 0; g < 32; g += 8) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            uint32_t x[4];
            load_raw<4>(fromD + (size_t)(base + g + k) * W, x);
            uint32_t p = no & (512u << k);
#pragma unroll
            for (int c = 0; c < 4; ++c) p = bcnt_acc(x[c] ^ q[c], p);
            pmin = min(pmin, p);
          }
          no = __builtin_amdgcn_alignbit(no, no, 8);
        }
      }
      acc = !((float)d1 > nndr * (float)pmin);
      exact = !acc;
    }
  }
  if (__ballot(exact)) {                         // wave-uniform: no certified wavefront takes it
    if (exact) acc = !((float)d1 > nndr * (float)mf_repair_d2<W>(fromD, Kf, q_row, idx, d2));
  }
  return acc;
}

// Body of the matching stage for ONE pair (the calling workgroup); `smem` is the workgroup's dynamic
// LDS.  Returns whether the pair goes on to motion estimation (block-uniform).  With list == nullptr
// the pair is not appended to a work list (fused pipeline, k_verify.hip).
// `out` = the pair's correspondence list (kcap entries; global in the stage kernels, LDS -- it may alias the
// staged "from" block, which is dead by the time the list is written -- in the fused kernel); hdr_out / pass_out
// = the pair's header and pass-1 state (same two homes).
// Guard, prologue, compaction loop and header write are spelt out here and not taken from sf_match_device.hpp as
// k_match_global does: this body is inlined into k_verify_fused and k_match_split, whose vector code and register
// allocation move with any of them behind a function boundary (profiles/match_finish_isa.txt); the calls below do not.
// LEAN (k_match_split): the prologue and the compaction in the forms of docs/match_tail.md -- one staging loop with up to
// four loads in flight that also zeroes cnt, all of a wavefront's ballots in front of ONE barrier -- and *null_matches =
// the `matches` of the null pass state written here, for the caller's write_null_result (every thread; meaningful when
// the return value is false).  Same bytes; the other callers keep the statements their register allocation was tuned on.
template <int W, int NQ, int NT, int MF_NTL = 2, bool MF_PIPE = false, bool LEAN = false>
__device__ __forceinline__ bool match_v2_body(const StoreView& st, int pair, int sF, int sT, float nndr, int min_inliers,
                                              int est, uint32_t* out, CorrHeader& hdr_out, PassState& pass_out,
                                              int32_t* __restrict__ list, int32_t* __restrict__ counter, int* smem,
                                              unsigned long long* trace_row = nullptr, int* null_matches = nullptr) {
  constexpr int NW = NT / 64;
  const int tid = threadIdx.x;
  // the wavefront's number as a scalar: the loop over its column groups is then scalar control flow, not a divergent
  // loop under exec masks with its counters in vector registers
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kcap = st.kcap;
  if ((unsigned)sF >= (unsigned)st.n_slots || (unsigned)sT >= (unsigned)st.n_slots) {
    if (tid == 0) {
      CorrHeader h = {0, 0, 0, 0};
      hdr_out = h;
      write_null_pass(pass_out, 0);
    }
    if constexpr (LEAN) *null_matches = 0;
    return false;
  }
  const int4 mF = st.meta[sF], mT = st.meta[sT];
  const int Kf = mF.x, Kt = mT.x;
  const uint32_t* dF = st.desc + (size_t)sF * kcap * W;
  const uint32_t* dT = st.desc + (size_t)sT * kcap * W;

  uint32_t* fromD = reinterpret_cast<uint32_t*>(smem);   // [kcap * W] staged "from" descriptors
  int* cnt = smem + kcap * W;                              // [kcap]
  int* owner = cnt + kcap;                                 // [kcap]
  int* misc = owner + kcap;                                // [16]

  // (Round 5 measured the staging by LDS-DMA with the first group's "to" rows loaded and spread beside it -- one memory
  //  latency in front of a pair's first MFMA instead of two, at 128 registers and no scratch: 22.6 against 22.8 M pairs/s,
  //  profiles/r05p_preload_ab.txt.  With four to five workgroups of other pairs on the CU a pair's own staging latency is
  //  already covered; not kept.)
  if constexpr (LEAN) {
    // one loop: four 16-byte items per thread and trip, their loads issued before the first LDS store waits (one memory
    // latency per 512 rows of W = 8 instead of one per 128), `cnt` zeroed beside the stores
    // (the loads are unconditional, an item past the block re-reads the block's last one: loads under a condition came out
    //  as one branch per item with the stores behind them laid out twice, and as an array written under a condition in scratch)
    const int n16 = Kf * (W / 4);
    const uint4* src = reinterpret_cast<const uint4*>(dF);
    uint4* dst = reinterpret_cast<uint4*>(fromD);
    for (int i = tid; i < n16; i += 4 * NT) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)       // (a 32-bit byte offset from the block's scalar base: two instructions per address)
        v[u] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(src) + (uint32_t)min(i + u * NT, n16 - 1) * 16u);
      // (the four values exist HERE: without this the compiler sinks each load into the condition of its store and waits
      //  for it there, four latencies one after the other again)
      asm volatile("" ::"v"(v[0].x), "v"(v[0].y), "v"(v[0].z), "v"(v[0].w), "v"(v[1].x), "v"(v[1].y), "v"(v[1].z), "v"(v[1].w),
                   "v"(v[2].x), "v"(v[2].y), "v"(v[2].z), "v"(v[2].w), "v"(v[3].x), "v"(v[3].y), "v"(v[3].z), "v"(v[3].w));
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i + u * NT < n16) dst[i + u * NT] = v[u];
        if (i + u * NT < Kf) cnt[i + u * NT] = 0;
      }
    }
  } else {
    const uint4* src = reinterpret_cast<const uint4*>(dF);
    uint4* dst = reinterpret_cast<uint4*>(fromD);
    for (int i = tid; i < Kf * (W / 4); i += NT) dst[i] = src[i];
    for (int i = tid; i < Kf; i += NT) cnt[i] = 0;
  }
  if (tid < 16) misc[tid] = 0;
  __syncthreads();
  SF_TRACE_ROW_MARK(trace_row, 32);   // "from" rows staged

  int rejected = 0;
  if constexpr (NQ == 0) {
    if (Kf > 0) {
      // "to" tiles resident per wavefront and scan: 2 keeps the fused kernel within 128 VGPRs (4 workgroups
      // per CU, which its motion-estimation chains need); the stage kernel takes 4 at 2 workgroups per CU
      // (the spread of the "from" tile is then shared by twice the columns: 0.293 -> 0.276 ms per 10 000 pairs)
      constexpr int NTL = W == 8 ? MF_NTL : 1;
      const int n_nt = (Kt + 31) >> 5;
      // a wavefront owns tiles wave, wave + NW, ...; it scans them in groups of up to NTL (a group that is
      // short of tiles drops to the next smaller instantiation; a 3-tile group runs as 4 with an empty tile)
      auto group = [&](auto g, int t0) {
        constexpr int G = decltype(g)::value, NP = mf_passes(G);
        int tl[G], f[NP];
        uint32_t a1[NP], a2[NP];
#pragma unroll
        for (int j = 0; j < G; ++j) tl[j] = t0 + j * NW;
        knn2_mfma<W, G, MF_PIPE>(fromD, Kf, dT, Kt, tl, lane, a1, a2, f);
        // a pass decides the columns of two tiles, one per lane half (mf_scan); `rejected` counts lanes, so it is a
        // wave-uniform sum of ballots, not a per-lane counter to be reduced
        int t[NP];
        bool on[NP], acc[NP], redo[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          t[p] = G == 1 ? tl[0] * 32 + lane : (tl[2 * p] + (lane >> 5) * NW) * 32 + (lane & 31);
          on[p] = (G > 1 || lane < 32) && t[p] < Kt;
          // a2 is optimistic (>= the exact second-best distance, top2_update16): a column rejected against it is
          // rejected; one that passes is decided again on its best row's class (mf_repair_accept).  (A negative nndr,
          // which accepts only d1 = d2 = 0, turns the inequality round: such a column repairs whatever the first test
          // says.)
          acc[p] = (Kf >= 2) && !((float)a1[p] > nndr * (float)a2[p]);
          redo[p] = on[p] && Kf >= 2 && (acc[p] || !(nndr >= 0.f));
        }
        if constexpr (NP == 1) {
          if (__ballot(redo[0])) {               // wave-uniform: no pass of an alias pair takes it
            const bool r = mf_repair_accept<W>(fromD, Kf, dT + (size_t)t[0] * W, f[0], a1[0], a2[0], nndr, redo[0]);
            acc[0] = redo[0] ? r : acc[0];
          }
        } else {
          // ONE repair per group: where the two passes' repairing columns fit one set of 64 lanes, those of pass 1 move
          // into lanes that have none of pass 0 and the decisions come back to the lanes that own the columns (claims
          // and `rejected` stay with the owner).  The hand-over is four lane permutations, each a bijection of the 64
          // lanes issued with all of them active (docs/chain_lane_sums.md), and no LDS of its own:
          //   slot: the lanes without a pass-0 repair in order (then the others), pushed by their rank;
          //   tgt : a pass-1 lane of rank r pulls slot[r] (a lane without a pass-1 repair: what is left, in order);
          //   the column travels to tgt packed in two words, the decision is pulled back from tgt.
          // Otherwise (more than 64 columns, one pass with nothing to repair, nndr < 0) the passes go one after the other
          // through the same statements.
          static_assert(NP == 2, "a group has one or two decode passes");
          const unsigned long long bal0 = __ballot(redo[0]), bal1 = __ballot(redo[1]);
          const int n0 = __popcll(bal0), n1 = __popcll(bal1);
          // (a pass with nothing to repair needs no hand-over: the trips below skip it at the price of a ballot)
          const bool merged = nndr >= 0.f && n0 != 0 && n1 != 0 && n0 + n1 <= 64;      // wave-uniform
          int tgt = 0;
          uint32_t m0 = 0, m1 = 0;
          bool mine = false;
          if (merged) {
            const int jf = mf_rank_below(~bal0), r1 = mf_rank_below(bal1);
            const int dest = redo[0] ? 64 - n0 + lane - jf : jf;
            const int slot = __builtin_amdgcn_ds_permute(dest << 2, lane);
            tgt = __builtin_amdgcn_ds_bpermute((redo[1] ? r1 : n1 + lane - r1) << 2, slot);
            m0 = (uint32_t)__builtin_amdgcn_ds_permute(tgt << 2, (int)((uint32_t)t[1] | ((uint32_t)f[1] << 16)));
            m1 = (uint32_t)__builtin_amdgcn_ds_permute(tgt << 2, (int)(a1[1] | (a2[1] << 16)));
            mine = !redo[0] && jf < n1;
          }
#pragma unroll 1
          for (int it = 0; it < 2; ++it) {
            bool act = it ? redo[1] : redo[0];
            int wt = it ? t[1] : t[0], wf = it ? f[1] : f[0];
            uint32_t w1 = it ? a1[1] : a1[0], w2 = it ? a2[1] : a2[0];
            if (mine) {                          // (set in the merged form only)
              act = true;
              wt = (int)(m0 & 0xFFFFu); wf = (int)(m0 >> 16);
              w1 = m1 & 0xFFFFu; w2 = m1 >> 16;
            }
            if (__ballot(act)) {
              const bool r = mf_repair_accept<W>(fromD, Kf, dT + (size_t)wt * W, wf, w1, w2, nndr, act);
              if (merged) {
                const bool back = __builtin_amdgcn_ds_bpermute(tgt << 2, (int)r) != 0;
                acc[0] = redo[0] ? r : acc[0];
                acc[1] = redo[1] ? back : acc[1];
              } else if (it) {
                acc[1] = redo[1] ? r : acc[1];
              } else {
                acc[0] = redo[0] ? r : acc[0];
              }
            }
            if (merged) break;
          }
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if (on[p] && acc[p]) match_claim(cnt, owner, f[p], t[p]);
          rejected += __popcll(__ballot(on[p] && !acc[p]));
        }
      };
      for (int t0 = wave; t0 < n_nt; t0 += NW * NTL) {
        const int avail = (n_nt - t0 + NW - 1) / NW;
        if constexpr (NTL >= 4) {
          if (avail >= 3) { group(std::integral_constant<int, 4>{}, t0); continue; }
        }
        if constexpr (NTL >= 2) {
          if (avail >= 2) { group(std::integral_constant<int, 2>{}, t0); continue; }
        }
        group(std::integral_constant<int, 1>{}, t0);
      }
    }
  } else if (Kf > 0) {
    for (int base = 0; base < Kt; base += NQ * NT) {

      uint32_t q[NQ][W], d1[NQ], d2[NQ], chunk[NQ];
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const int t = base + j * NT + tid;
        load_desc<W>(dT, t, t < Kt, q[j]);
        d1[j] = 0xFFFFu;
        d2[j] = 0xFFFFu;
        chunk[j] = 0;
      }
      const int wave_rows = Kt - base - (tid & ~63);
      const int groups = wave_rows <= 0 ? 0 : min(NQ, (wave_rows + NT - 1) / NT);
      if (groups == NQ) {
        knn2_scan_lds<W, NQ>(fromD, Kf, q, d1, d2, chunk);
      } else if (groups > 0) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          if (j < groups) {
            uint32_t qq[1][W], a1[1] = {0xFFFFu}, a2[1] = {0xFFFFu}, ch[1] = {0};
#pragma unroll
            for (int c = 0; c < W; ++c) qq[0][c] = q[j][c];
            knn2_scan_lds<W, 1>(fromD, Kf, qq, a1, a2, ch);
            d1[j] = a1[0]; d2[j] = a2[0]; chunk[j] = ch[0];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const int t = base + j * NT + tid;
        if (t < Kt) {
          const uint32_t b1 = d1[j] & 0xFFFFu, b2 = d2[j] & 0xFFFFu;
          const bool acc = (Kf >= 2) && !((float)b1 > nndr * (float)b2);
          if (acc) {
            // index recovery inside the chunk where the minimum was reached
            int f = (int)chunk[j];
            const int fend = min(f + MATCH_CH, Kf);
            for (; f < fend; ++f) {
              const uint32_t* r = fromD + (size_t)f * W;
              uint32_t d = 0;
#pragma unroll
              for (int c = 0; c < W; ++c) d += __popc(r[c] ^ q[j][c]);
              if (d == b1) break;
            }
            match_claim(cnt, owner, f, t);
          } else {
            ++rejected;
          }
        }
      }
    }
  }
  if constexpr (NQ != 0) {   // (the matrix-core path counted whole wavefronts)
    for (int off = 32; off >= 1; off >>= 1) rejected += __shfl_xor(rejected, off);
  }
  if (lane == 0 && rejected) atomicAdd(&misc[0], rejected);
  SF_TRACE_ROW_MARK(trace_row, 33);   // wavefront 0 done with its scans
  __syncthreads();
  SF_TRACE_ROW_MARK(trace_row, 34);   // all wavefronts done

  int running = 0;
  if constexpr (LEAN) {
    // All ballots first: trip t of this wavefront covers "from" rows t * NT + tid; its mask stays in scalar registers and
    // its count travels as one byte (<= 64) of two words per wavefront, misc[4 + 2 wave], misc[5 + 2 wave].  Behind ONE
    // barrier every wavefront sums the bytes of the NW rows in 16-bit fields (<= 256 per trip) -- the entries in front of
    // its own, per trip -- and writes: the order of out[] (ascending "from" index) and n_corr are those of the loop below.
    constexpr int MAXT = MF_MAX_ROWS / NT;
    static_assert(MAXT <= 8 && NW <= 4, "two words of byte counts per wavefront in misc[4..12)");
    const int ntrip = (Kf + NT - 1) / NT;          // (scalar; Kf <= kcap <= MF_MAX_ROWS on this path)
    unsigned long long bal[MAXT];
    uint32_t pk[2] = {0u, 0u};
#pragma unroll
    for (int t = 0; t < MAXT; ++t) bal[t] = 0ull;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      if (t >= ntrip) break;
      const int f = t * NT + tid;
      bal[t] = __ballot((f < Kf) && (cnt[f] == 1));
      pk[t >> 2] |= (uint32_t)__popcll(bal[t]) << (8 * (t & 3));
    }
    if (lane == 0) { misc[4 + 2 * wave] = (int)pk[0]; misc[5 + 2 * wave] = (int)pk[1]; }
    __syncthreads();
    uint32_t tot[2][2] = {{0u, 0u}, {0u, 0u}}, mine[2][2] = {{0u, 0u}, {0u, 0u}};   // [word][even / odd trips of it]
#pragma unroll
    for (int w = 0; w < NW; ++w) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j == 1 && ntrip <= 4) continue;
        const uint32_t x = (uint32_t)__builtin_amdgcn_readfirstlane(misc[4 + 2 * w + j]);
        const uint32_t e = x & 0x00FF00FFu, o = (x >> 8) & 0x00FF00FFu;
        tot[j][0] += e; tot[j][1] += o;
        if (w < wave) { mine[j][0] += e; mine[j][1] += o; }
      }
    }
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      if (t >= ntrip) break;
      const int sh = 16 * ((t & 3) >> 1);
      const int total = (int)((tot[t >> 2][t & 1] >> sh) & 0xFFFFu), woff = (int)((mine[t >> 2][t & 1] >> sh) & 0xFFFFu);
      const int f = t * NT + tid;
      // (the mask is the condition: it goes to exec as it is, no per-lane flag is kept across the barrier)
      if (__builtin_amdgcn_inverse_ballot_w64(bal[t])) out[running + woff + mf_rank_below(bal[t])] = (uint32_t)f | ((uint32_t)owner[f] << 16);
      running += total;
    }
  } else
  for (int base = 0; base < Kf; base += NT) {
    const int f = base + tid;
    const bool flag = (f < Kf) && (cnt[f] == 1);
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
    if (flag) out[running + woff + before] = (uint32_t)f | ((uint32_t)owner[f] << 16);
    running += total;
    __syncthreads();
  }
  const int n_corr = running;
  SF_TRACE_ROW_MARK(trace_row, 35);   // list compacted

  const MatchGates G = match_gates(Kf, Kt, mF, mT, misc[0], n_corr, min_inliers, est);
  const bool motion = G.motion, survivor = G.survivor;
  if (motion && !survivor) {
    if constexpr (LEAN) __syncthreads();         // the list's entries are other threads' (the old loop ended with a barrier)
    corr_count_finite<NT>(st.xyz + (size_t)sF * kcap * 3, st.xyz + (size_t)sT * kcap * 3, out, n_corr, est == 0, &misc[2]);
  }
  if (tid == 0) {
    CorrHeader h;
    h.n_corr = n_corr;
    h.words_from = G.words_from;
    h.words_to = G.words_to;
    h.words_to_2d = G.unique_to;
    hdr_out = h;
    write_null_pass(pass_out, (motion && !survivor) ? misc[2] : 0);
    if (survivor && list) worklist_append(list, counter, pair);
  }
  if constexpr (LEAN) *null_matches = (motion && !survivor) ? misc[2] : 0;     // (misc[2]: final behind corr_count_finite's barrier)
  return survivor;
}

template <int W, int NQ, int NT>
__global__ void __launch_bounds__(NT)
k_match_global_v2(StoreView st, const int32_t* __restrict__ pair_from, const int32_t* __restrict__ pair_to,
                  float nndr, int min_inliers, int est, uint32_t* __restrict__ corr, CorrHeader* __restrict__ hdr,
                  PassState* __restrict__ pass, int32_t* __restrict__ list, int32_t* __restrict__ counter) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  const int pair = (int)blockIdx.x;
  match_v2_body<W, NQ, NT>(st, pair, pair_from[pair], pair_to[pair], nndr, min_inliers, est, corr + (size_t)pair * st.kcap,
                           hdr[pair], pass[pair], list, counter, smem);
}

// the matrix-core variant as a stage kernel: 4 column tiles per scan at 2 workgroups per CU (<= 256
// VGPRs; measured equal to 3 and 4 workgroups per CU -- the kernel is bound by VALU issue, not by
// occupancy).  A register budget <= 256 also keeps the MFMA results in VGPRs: with the full 512 the
// compiler accumulates in AGPRs and pays a v_accvgpr_read per value in the epilogue.
template <int W, int NT>
__global__ void __launch_bounds__(NT, 2)
k_match_global_mf(StoreView st, const int32_t* __restrict__ pair_from, const int32_t* __restrict__ pair_to,
                  float nndr, int min_inliers, int est, uint32_t* __restrict__ corr, CorrHeader* __restrict__ hdr,
                  PassState* __restrict__ pass, int32_t* __restrict__ list, int32_t* __restrict__ counter) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  const int pair = (int)blockIdx.x;
  match_v2_body<W, 0, NT, 4>(st, pair, pair_from[pair], pair_to[pair], nndr, min_inliers, est,
                             corr + (size_t)pair * st.kcap, hdr[pair], pass[pair], list, counter, smem);
}

// pass-1 stage launches: sf_launch_pass1 (sf_internal.hpp) holds the argument list
template <int W, int NQ, int NT>
void launch_match_v2(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n) {
  size_t lds = sf_match_lds_bytes(st.kcap, W);
  if (const char* v = getenv("SF_MATCH_LDS_PAD")) lds += (size_t)atoi(v);   // occupancy experiment (diagnostic)
  if constexpr (NQ == 0) sf_launch_pass1(c, k_match_global_mf<W, NT>, NT, lds, st, d_from, d_to, n);
  else sf_launch_pass1(c, k_match_global_v2<W, NQ, NT>, NT, lds, st, d_from, d_to, n);
}

// variant 1 and its float32 form: the bookkeeping is all the LDS they take
template <int W, int NQ, int NT, bool L2 = false>
void launch_match(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n) {
  sf_launch_pass1(c, k_match_global<W, NQ, NT, L2>, NT, (size_t)(2 * st.kcap + 16) * sizeof(int), st, d_from, d_to, n);
}

}  // namespace

int sf_launch_match_global(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n) {
  if (n <= 0) return SF_OK;
  if (c->params.desc_type == 2) return sf_launch_match_global_u8(c, st, d_from, d_to, n);   // uint8 rows, L2: k_match_u8.hip
  if (c->params.desc_type == 1) {       // float32 rows: exact L2 on the VALU (north_star: MFMA only for the NetVLAD matrix)
    sf_prof_begin(c, SF_K_MATCH);
    if (st.w == 64) launch_match<64, 1, 256, true>(c, st, d_from, d_to, n);
    else launch_match<128, 1, 256, true>(c, st, d_from, d_to, n);
    sf_prof_end(c, SF_K_MATCH);
    SF_HIP(c, hipGetLastError());
    return SF_OK;
  }
  // geometry: variant = NQ * 1000 + NT of k_match_global, 10000 more for match_v2_body (SF_MATCH_VARIANT forces one for
  // A/B runs; the geometries no rule chooses were retired)
  int variant = c->match_variant;
  if (variant == 0) {
    // default: LDS + u16 variant while the staged "from" block keeps >= 2 workgroups per CU
    const size_t lds_v2 = sf_match_lds_bytes(st.kcap, st.w);
    variant = lds_v2 <= 64 * 1024 ? (c->match_mfma && st.kcap <= MF_MAX_ROWS ? 10256 : 12256) : 2256;
  }
  sf_prof_begin(c, SF_K_MATCH);
  switch (variant) {
    case 2256:
      if (st.w == 8) launch_match<8, 2, 256>(c, st, d_from, d_to, n);
      else launch_match<16, 2, 256>(c, st, d_from, d_to, n);
      break;
    case 10256:   // NQ = 0: fp4 matrix-core variant
      if (st.w == 8) launch_match_v2<8, 0, 256>(c, st, d_from, d_to, n);
      else launch_match_v2<16, 0, 256>(c, st, d_from, d_to, n);
      break;
    case 12256:
      if (st.w == 8) launch_match_v2<8, 2, 256>(c, st, d_from, d_to, n);
      else launch_match_v2<16, 2, 256>(c, st, d_from, d_to, n);
      break;
    default:
      sf_prof_end(c, SF_K_MATCH);
      return sf_fail(c, SF_EINVAL, "unknown match kernel variant %d", variant);
  }
  sf_prof_end(c, SF_K_MATCH);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
