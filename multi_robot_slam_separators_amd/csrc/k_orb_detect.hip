// k_orb_detect.hip -- SURVEY.md section 8 row f3, the third detector: ORB on an image pyramid as rtabmap's
// Vis/FeatureType 2 runs it -- cv::ORB::detect of OpenCV 3.2 (pyramid by cv::resize INTER_LINEAR, FAST-9/16 per level,
// border filter, per-level quotas, retainBest on the FAST score and on the Harris measure, intensity-centroid angle),
// then rtabmap's Feature2D::limitKeypoints.  Neither upstream text is in the reference tree: the semantics are restated
// in tests/orb2_ref.py (DESIGN.md section 3 item 17b lists what the restatement decides).  Everything is 8-bit / int32
// work except the Harris expression and the angle, which are float32 in the order written (this file is compiled with
// -ffp-contract=off), so the kernels equal the restatement byte for byte.
//
//   k_orb_resize     one level from the level below: the 2 x 2 mean when it halves exactly, else 8-bit bilinear in 11-bit
//                    fixed point; the coefficients of a pixel are computed by its thread (two double divisions)
//   k_fast_score / k_fast_candidates (k_fast.hip, unchanged) per level -> keys (score << 32 | pixel) and a count per level
//   k_orb_gather     every candidate (C of them in an image: the sum of its levels' counts, taken on the device): border
//                    filter, key (level << 40 | pixel << 8 | score), histogram of the FAST scores of its level
//   k_orb_cut_a      per level: the score at rank 2 quota (Harris) or quota (FAST) from the histogram -- retainBest on
//                    8-bit scores needs no sort -- and the level's segment in the sorted list
//   k_orb_filter_a   drops the candidates below their level's cut
//   sf_sort_segments (sf_sort.hip) ascending by (level, pixel): survivors first, raster order within a level
//   k_orb_harris     (score type Harris) one candidate per wavefront: lanes 0 .. 48 own one pixel of the 7 x 7 block each,
//                    three integer wave reductions, one float32 expression; key (level, inverted order-preserving bits)
//   sort ascending -> per level descending response; k_orb_cut_b reads the response at rank quota - 1
//   k_orb_compact    ONE workgroup: stable compaction of the survivors (response >= cut: ties stay) in (level, raster)
//                    order, then the keys of limitKeypoints: the index when the survivors fit max_features, else
//                    (|response|, index)
//   sort descending -> the final order
//   k_orb_emit       keypoints in LEVEL coordinates; k_orb_angle (k_extract.hip) adds the centroid angle on the level;
//   k_orb_finish     position * scale_l into the caller's array
// About forty short launches for three levels: latency-bound like the rest of the front end, not tuned yet.
//
// One launcher over these kernels, sf_launch_detect_orb, for n >= 1 images of one size: the image is a grid axis
// (blockIdx.y; blockIdx.x for the one-workgroup kernels), every list has a fixed capacity per image (3 x 3 strict
// maxima: a level of w x h pixels holds at most ceil(w / 2) ceil(h / 2) corners, so nothing is ever truncated), the
// per-level segments of an image come from the counts on the device, and the three sorts take their bounds from the
// kernels before them (k_orb_gather, k_orb_cut_a, k_orb_compact).  Two or more images never wait for the host.  A lone
// image's sorts (a single call's, and a batch call's with one keyframe alike) are device-wide and sized by C, which crosses to the host once, with the first of them (sf_sort_segments):
// k_orb_harris and k_orb_compact fill their lists up to C with keys that sort behind the stage's own bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sf_front_device.hpp"

namespace {

constexpr unsigned long long ORB_NONE = ~0ull;
constexpr unsigned long long ORB_RASTER = 1ull << 63, ORB_LIMITED = 1ull << 62;
// the scalar block of an image (ints): per-level arrays of 8, then the histograms; S_NCAND = the image's candidates
constexpr int S_CUT_A = 8, S_BEGIN = 16, S_KEPT = 24, S_TOTAL = 32, S_NCAND = 33, S_NFINAL = 34, S_CUT_B = 40, S_HIST = 64;
constexpr int S_WORDS = S_HIST + SF_ORB_MAX_LEVELS * 256;
constexpr int ORB_HARRIS_BLOCKS = 1024;    // k_orb_harris: workgroups per image at the most (4 candidates each per step)

struct OrbSel {
  int n_levels, score_type, edge, max_features;
  int quota[SF_ORB_MAX_LEVELS];
};

// Where the lists of the n_img >= 1 images are: image i's source at + i * img_stride, its pyramid at + i * pyr_stride, its
// entries of every work list at + i * cand_cap, its scalar block at + i * S_WORDS, its keypoints at + i * kp_cap.
struct OrbBatch {
  size_t img_stride, pyr_stride;
  unsigned cand_cap;
  int n_img, kp_cap;
  unsigned key_off[SF_ORB_MAX_LEVELS];   // the FAST keys of (image i, level l) at keys_f + key_off[l] + i * key_cap[l]
  unsigned key_cap[SF_ORB_MAX_LEVELS];
  const unsigned* d_count;               // [level][n_img] corners found by FAST
  unsigned* seg;                         // [6][n_img] begin / end of the image's segment in each of the three sorts
  int32_t* n_out;                        // [n_img] keypoints of every image
};

__device__ __forceinline__ int orb_quota_of(const OrbSel& S, int l) {
  int r = S.quota[0];
#pragma unroll
  for (int k = 1; k < SF_ORB_MAX_LEVELS; ++k) r = l == k ? S.quota[k] : r;
  return r;
}

// One axis of cv::resize(INTER_LINEAR) for 8-bit images: source index and the two 11-bit coefficients of destination d
__device__ __forceinline__ void orb_lin_axis(int d, int dst, int src, int& s, int& c0, int& c1) {
  const double scale = 1.0 / ((double)dst / (double)src);
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int si = (int)floorf(f);
  f -= (float)si;
  if (si < 0) { si = 0; f = 0.f; }
  if (si >= src - 1) { si = src - 1; f = 0.f; }
  s = si;
  c0 = (int)rintf((1.f - f) * 2048.f);
  c1 = (int)rintf(f * 2048.f);
}

__global__ void __launch_bounds__(256)
k_orb_resize(const uint8_t* __restrict__ src, int sw, int sh, int spitch, uint8_t* __restrict__ dst, int dw, int dh,
             size_t src_stride, size_t dst_stride) {
  // (blockIdx.z = image of a batch)
  src += blockIdx.z * src_stride;
  dst += blockIdx.z * dst_stride;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  int v;
  if (sw == 2 * dw && sh == 2 * dh) {
    const uint8_t* p = src + (size_t)(2 * y) * spitch + 2 * x;
    v = ((int)p[0] + (int)p[1] + (int)p[spitch] + (int)p[spitch + 1] + 2) >> 2;
  } else {
    int sx, a0, a1, sy, b0, b1;
    orb_lin_axis(x, dw, sw, sx, a0, a1);
    orb_lin_axis(y, dh, sh, sy, b0, b1);
    const int sx1 = min(sx + 1, sw - 1), sy1 = min(sy + 1, sh - 1);
    const uint8_t* r0 = src + (size_t)sy * spitch;
    const uint8_t* r1 = src + (size_t)sy1 * spitch;
    const int S0 = a0 * (int)r0[sx] + a1 * (int)r0[sx1], S1 = a0 * (int)r1[sx] + a1 * (int)r1[sx1];
    v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
  }
  dst[(size_t)y * dw + x] = (uint8_t)v;
}

// keys_f: the FAST keys of level l of image blockIdx.y at keys_f + B.key_off[l] + blockIdx.y * B.key_cap[l] (arrival order)
__global__ void __launch_bounds__(256)
k_orb_gather(const unsigned long long* __restrict__ keys_f, SfOrbPyr P, OrbSel S, unsigned long long* __restrict__ cand,
             int* __restrict__ sc, OrbBatch B) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
  // candidate i's level, the level's first candidate and its FAST keys: the running sum of the image's counts
  int l = 0;
  unsigned first = 0u, koff = B.key_off[0], kcap = B.key_cap[0], run = 0u;
#pragma unroll
  for (int k = 0; k < SF_ORB_MAX_LEVELS; ++k) {
    const unsigned b = k < S.n_levels ? run : 0xFFFFFFFFu;
    if (k > 0 && i >= b) { l = k; first = b; koff = B.key_off[k]; kcap = B.key_cap[k]; }
    if (k < S.n_levels) run += min(B.d_count[(unsigned)k * (unsigned)B.n_img + img], B.key_cap[k]);
  }
  const unsigned C = run;
  sc += (size_t)img * S_WORDS;
  cand += (size_t)img * B.cand_cap;
  if (i == 0) {
    sc[S_NCAND] = (int)C;
    B.seg[img] = img * B.cand_cap;
    B.seg[B.n_img + img] = img * B.cand_cap + C;
  }
  if (i >= C) return;
  const SfOrbLevel L = sf_orb_level(P, l);
  const unsigned long long key = keys_f[(size_t)koff + (size_t)img * kcap + (i - first)];
  const unsigned idx = (unsigned)key, score = (unsigned)(key >> 32) & 255u;
  const int y = (int)(idx / (unsigned)L.w), x = (int)(idx - (unsigned)y * (unsigned)L.w), e = S.edge;
  const bool inside = L.w > 2 * e && L.h > 2 * e && x >= e && x < L.w - e && y >= e && y < L.h - e;
  cand[i] = inside ? ((unsigned long long)l << 40) | ((unsigned long long)idx << 8) | score : ORB_NONE;
  if (inside) atomicAdd(&sc[S_HIST + l * 256 + (int)score], 1);
}

// ONE workgroup per image, thread l = level l
__global__ void __launch_bounds__(64)
k_orb_cut_a(OrbSel S, int* __restrict__ sc, OrbBatch B) {
  __shared__ int s_kept[SF_ORB_MAX_LEVELS];
  const int l = threadIdx.x;
  const unsigned img = blockIdx.x;
  sc += (size_t)img * S_WORDS;
  if (l < SF_ORB_MAX_LEVELS) {
    int kept = 0, cut = 256;
    if (l < S.n_levels) {
      const int q = orb_quota_of(S, l), want = S.score_type == 0 ? 2 * q : q;
      int cum = 0;
      bool found = false;
      for (int s = 255; s >= 1; --s) {
        cum += sc[S_HIST + l * 256 + s];
        if (!found && want > 0 && cum >= want) { found = true; cut = s; kept = cum; }
      }
      if (want > 0 && !found) { cut = 1; kept = cum; }
    }
    sc[S_CUT_A + l] = cut;
    s_kept[l] = kept;
  }
  __syncthreads();
  if (l == 0) {
    int run = 0;
    for (int k = 0; k < SF_ORB_MAX_LEVELS; ++k) {
      sc[S_BEGIN + k] = run;
      sc[S_KEPT + k] = s_kept[k];
      run += s_kept[k];
    }
    sc[S_TOTAL] = run;
    B.seg[2 * B.n_img + img] = img * B.cand_cap;                  // the Harris sort's segment: the survivors of the first cut
    B.seg[3 * B.n_img + img] = img * B.cand_cap + (unsigned)run;
  }
}

__global__ void __launch_bounds__(256)
k_orb_filter_a(unsigned long long* __restrict__ cand, const int* __restrict__ sc, OrbBatch B) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  sc += (size_t)blockIdx.y * S_WORDS;
  cand += (size_t)blockIdx.y * B.cand_cap;
  if (i >= (unsigned)sc[S_NCAND]) return;
  const unsigned long long key = cand[i];
  if (key == ORB_NONE) return;
  if ((int)(key & 255ull) < sc[S_CUT_A + (int)(key >> 40)]) cand[i] = ORB_NONE;
}

// ascending unsigned order = ascending float order
__device__ __forceinline__ unsigned orb_order_bits(float r) {
  const unsigned u = __float_as_uint(r);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float orb_order_float(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// one candidate per wavefront and step (HarrisResponses, block 7, k 0.04); edge >= 16 keeps the radius-4 window inside the
// level.  The grid strides over the image's C candidates; past the survivors of the first cut the keys are ORB_NONE, which
// sorts behind them: a lone image's sort covers all C entries (the range the host knows), a segment ends at the survivors.
__global__ void __launch_bounds__(256)
k_orb_harris(const uint8_t* __restrict__ img, int pitch, const uint8_t* __restrict__ pyr, SfOrbPyr P,
             const unsigned long long* __restrict__ cand_s, const int* __restrict__ sc, float* __restrict__ resp,
             unsigned long long* __restrict__ key_b, OrbBatch B) {
  const int lane = threadIdx.x & 63;
  const size_t o = (size_t)blockIdx.y * B.cand_cap;
  sc += (size_t)blockIdx.y * S_WORDS;
  img += blockIdx.y * B.img_stride;
  pyr += blockIdx.y * B.pyr_stride;
  cand_s += o; resp += o; key_b += o;
  const unsigned C = (unsigned)sc[S_NCAND], total = (unsigned)sc[S_TOTAL];
  for (unsigned i = blockIdx.x * 4 + (threadIdx.x >> 6); i < C; i += gridDim.x * 4) {
    if (i >= total) {
      if (lane == 0) key_b[i] = ORB_NONE;
      continue;
    }
    const unsigned long long key = cand_s[i];
    const int l = (int)(key >> 40);
    const unsigned idx = (unsigned)(key >> 8);
    const SfOrbLevel L = sf_orb_level(P, l);
    const uint8_t* base = l == 0 ? img : pyr + L.off;
    const int lp = l == 0 ? pitch : L.w;
    const int y = (int)(idx / (unsigned)L.w), x = (int)(idx - (unsigned)y * (unsigned)L.w);
    int a = 0, b = 0, cc = 0;
    if (lane < 49) {
      const int by = lane / 7, bx = lane - 7 * by;
      const uint8_t* p = base + (size_t)(y + by - 3) * lp + (x + bx - 3);
      const int mm = p[-lp - 1], m0 = p[-lp], mp = p[-lp + 1], zm = p[-1], zp = p[1], pm = p[lp - 1], p0 = p[lp], pp = p[lp + 1];
      const int ix = (zp - zm) * 2 + (mp - mm) + (pp - pm);
      const int iy = (p0 - m0) * 2 + (pm - mm) + (pp - mp);
      a = ix * ix; b = iy * iy; cc = ix * iy;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off);
      b += __shfl_xor(b, off);
      cc += __shfl_xor(cc, off);
    }
    if (lane == 0) {
      const float fa = (float)a, fb = (float)b, fc = (float)cc;
      const float s = 1.f / (4 * 7 * 255.f);
      const float s4 = s * s * s * s;
      const float sum = fa + fb;
      const float r = ((fa * fb - fc * fc) - 0.04f * sum * sum) * s4;
      resp[i] = r;
      key_b[i] = ((unsigned long long)l << 32) | (unsigned)~orb_order_bits(r);
    }
  }
}

// ONE workgroup per image, thread l = level l: the response at rank quota - 1 of the level's segment (float bits)
__global__ void __launch_bounds__(64)
k_orb_cut_b(OrbSel S, const unsigned long long* __restrict__ key_bs, int* __restrict__ sc, OrbBatch B) {
  const int l = threadIdx.x;
  sc += (size_t)blockIdx.x * S_WORDS;
  key_bs += (size_t)blockIdx.x * B.cand_cap;
  if (l >= S.n_levels) return;
  const int q = orb_quota_of(S, l), m = sc[S_KEPT + l];
  float cut = -INFINITY;
  if (S.score_type == 0) {
    if (q == 0) cut = INFINITY;
    else if (m > q) cut = orb_order_float(~(unsigned)key_bs[sc[S_BEGIN + l] + q - 1]);
  }
  sc[S_CUT_B + l] = __float_as_int(cut);
}

// ONE workgroup per image: stable compaction of the survivors, then the sort keys of limitKeypoints (C entries, 0 past the
// end)
__global__ void __launch_bounds__(256)
k_orb_compact(OrbSel S, const unsigned long long* __restrict__ cand_s, const float* __restrict__ resp,
              unsigned long long* __restrict__ fin_key, float* __restrict__ fin_resp, unsigned long long* __restrict__ key_c,
              int* __restrict__ sc, OrbBatch B) {
  __shared__ int wave_cnt[4];
  const int tid = threadIdx.x;
  const unsigned img = blockIdx.x;
  const size_t off = (size_t)img * B.cand_cap;
  sc += (size_t)img * S_WORDS;
  cand_s += off; resp += off; fin_key += off; fin_resp += off; key_c += off;
  const unsigned C = (unsigned)sc[S_NCAND];
  const int total = sc[S_TOTAL];
  int running = 0;
  for (int base = 0; base < total; base += 256) {
    const int i = base + tid;
    unsigned long long key = 0ull;
    float r = 0.f;
    bool f = false;
    if (i < total) {
      key = cand_s[i];
      r = S.score_type == 0 ? resp[i] : (float)(unsigned)(key & 255ull);
      f = r >= __int_as_float(sc[S_CUT_B + (int)(key >> 40)]);
    }
    const SfRank rank = sf_block_rank(f, wave_cnt);
    if (f) {
      const int o = running + rank.before;
      fin_key[o] = key;
      fin_resp[o] = r;
    }
    running += rank.total;
    __syncthreads();
  }
  const bool limited = S.max_features > 0 && running > S.max_features;
  for (unsigned o = tid; o < C; o += 256) {
    unsigned long long k = 0ull;
    if (o < (unsigned)running)
      k = limited ? ORB_LIMITED | ((unsigned long long)(__float_as_uint(fin_resp[o]) & 0x7FFFFFFFu) << 31) | o
                  : ORB_RASTER | (0x7FFFFFFFu - o);
    key_c[o] = k;
  }
  if (tid == 0) {
    const int n_final = limited ? S.max_features : running;
    sc[S_NFINAL] = n_final;
    B.seg[4 * B.n_img + img] = img * B.cand_cap;                  // the last sort's segment: the survivors;
    B.seg[5 * B.n_img + img] = img * B.cand_cap + (unsigned)running;
    B.n_out[img] = n_final;                                       // the image's count for the caller
  }
}

// keypoints in LEVEL coordinates, final order
__global__ void __launch_bounds__(256)
k_orb_emit(SfOrbPyr P, const unsigned long long* __restrict__ key_cs, const unsigned long long* __restrict__ fin_key,
           const float* __restrict__ fin_resp, const int* __restrict__ sc, int cap, sf_keypoint* __restrict__ kp, OrbBatch B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const size_t off = (size_t)blockIdx.y * B.cand_cap;
  sc += (size_t)blockIdx.y * S_WORDS;
  key_cs += off; fin_key += off; fin_resp += off;
  kp += (size_t)blockIdx.y * B.kp_cap;
  if (i >= sc[S_NFINAL] || i >= cap) return;
  const unsigned long long kc = key_cs[i];
  const unsigned low = (unsigned)kc & 0x7FFFFFFFu;
  const unsigned o = (kc & ORB_RASTER) ? 0x7FFFFFFFu - low : low;
  const unsigned long long key = fin_key[o];
  const int l = (int)(key >> 40);
  const unsigned idx = (unsigned)(key >> 8);
  const SfOrbLevel L = sf_orb_level(P, l);
  const int y = (int)(idx / (unsigned)L.w), x = (int)(idx - (unsigned)y * (unsigned)L.w);
  kp[i] = sf_make_keypoint((float)x, (float)y, 31.f * L.scale, fin_resp[o], l);
}

__global__ void __launch_bounds__(256)
k_orb_finish(SfOrbPyr P, const sf_keypoint* __restrict__ kp, const int* __restrict__ sc, int cap, sf_keypoint* __restrict__ out,
             OrbBatch B, int out_cap) {
  // (image blockIdx.y's keypoints to out + blockIdx.y * out_cap)
  const int i = blockIdx.x * 256 + threadIdx.x;
  sc += (size_t)blockIdx.y * S_WORDS;
  kp += (size_t)blockIdx.y * B.kp_cap;
  out += (size_t)blockIdx.y * out_cap;
  if (i >= sc[S_NFINAL] || i >= cap) return;
  sf_keypoint k = kp[i];
  const SfOrbLevel L = sf_orb_level(P, k.octave);
  k.x = k.x * L.scale;
  k.y = k.y * L.scale;
  out[i] = k;
}

}  // namespace

// Level sizes and offsets: scale_l = (float)pow((double)scale_factor, l), size cvRound(W / scale_l) in float
SfOrbPyr sf_orb_pyr_layout(int width, int height, float scale_factor, int n_levels) {
  SfOrbPyr P = {};
  P.n = n_levels;
  size_t off = 0;
  for (int l = 0; l < SF_ORB_MAX_LEVELS; ++l) {
    const float s = l < n_levels ? (float)std::pow((double)scale_factor, (double)l) : 1.f;
    P.scale[l] = s;
    P.inv_scale[l] = 1.f / s;
    P.w[l] = l < n_levels ? (int)lrintf((float)width / s) : 0;
    P.h[l] = l < n_levels ? (int)lrintf((float)height / s) : 0;
    P.off[l] = (unsigned)off;
    off += ((size_t)P.w[l] * P.h[l] + 15) & ~(size_t)15;
  }
  P.total = (unsigned)off;
  return P;
}

// cv::ORB's features per level, float arithmetic: n_0 = nfeatures (1 - f) / (1 - f^n_levels), f = 1 / scale_factor
void sf_orb_quotas(int nfeatures, float scale_factor, int n_levels, int* quota) {
  const float factor = 1.0f / scale_factor;
  float nd = (float)nfeatures * (1.0f - factor) / (1.0f - (float)std::pow((double)factor, (double)n_levels));
  int sum = 0;
  for (int l = 0; l < SF_ORB_MAX_LEVELS; ++l) quota[l] = 0;
  for (int l = 0; l < n_levels - 1; ++l) {
    quota[l] = (int)lrintf(nd);
    sum += quota[l];
    nd *= factor;
  }
  quota[n_levels - 1] = std::max(nfeatures - sum, 0);
}

// Levels >= 1 of n_img images of one size (img_stride bytes apart) into c->orb_pyr, image i's at + i * P.total
int sf_launch_orb_pyramid(sf_context* c, const uint8_t* d_image, int pitch, const SfOrbPyr& P, int n_img, size_t img_stride) {
  for (int l = 0; l < P.n; ++l)
    if (P.w[l] < 1 || P.h[l] < 1)
      return sf_fail(c, SF_ERANGE, "pyramid level %d of a %d x %d image at scale %g is empty", l, P.w[0], P.h[0], (double)P.scale[l]);
  int rc;
  if ((rc = sf_buf_reserve(c, c->orb_pyr, std::max<size_t>((size_t)P.total * n_img, 16))) != SF_OK) return rc;
  uint8_t* pyr = (uint8_t*)c->orb_pyr.p;
  for (int l = 1; l < P.n; ++l) {
    const uint8_t* src = l == 1 ? d_image : pyr + P.off[l - 1];
    hipLaunchKernelGGL(k_orb_resize, dim3((P.w[l] + 63) / 64, (P.h[l] + 3) / 4, n_img), dim3(256), 0, c->stream, src, P.w[l - 1],
                       P.h[l - 1], l == 1 ? pitch : P.w[l - 1], pyr + P.off[l], P.w[l], P.h[l], l == 1 ? img_stride : (size_t)P.total,
                       (size_t)P.total);
  }
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

// The work lists of both launchers in c->orb_work: `entries` candidates (all images), `kp_entries` keypoints.  Four key
// arrays serve the seven lists -- a list takes the place of one that nothing reads any more (cand is dead after the first
// sort, key_b after the second, key_bs after k_orb_cut_b) and no sort runs in place.
struct OrbLists {
  unsigned long long *cand, *cand_s, *key_b, *key_bs, *key_c, *key_cs, *fin_key;
  float *resp, *fin_resp;
  sf_keypoint *kp1, *kp2;
};
static size_t orb_lists_bytes(size_t entries, size_t kp_entries) {
  return entries * (4 * 8 + 2 * 4) + 2 * ((kp_entries * sizeof(sf_keypoint) + 15) & ~(size_t)15) + 64;
}
static int orb_lists(sf_context* c, size_t entries, size_t kp_entries, OrbLists* W) {
  const size_t kp_bytes = (kp_entries * sizeof(sf_keypoint) + 15) & ~(size_t)15;
  int rc = sf_buf_reserve(c, c->orb_work, orb_lists_bytes(entries, kp_entries));
  if (rc != SF_OK) return rc;
  unsigned long long* a = (unsigned long long*)c->orb_work.p;
  W->cand = a;                 W->key_b = a;                 W->key_cs = a;
  W->cand_s = a + entries;
  W->key_bs = a + 2 * entries; W->key_c = a + 2 * entries;
  W->fin_key = a + 3 * entries;
  W->resp = (float*)(a + 4 * entries);
  W->fin_resp = W->resp + entries;
  W->kp1 = (sf_keypoint*)(((uintptr_t)(W->fin_resp + entries) + 15) & ~(uintptr_t)15);
  W->kp2 = (sf_keypoint*)((char*)W->kp1 + kp_bytes);
  return SF_OK;
}

static OrbSel orb_selection(const SfOrbPyr& P, int max_features, const sf_orb_detector_params* det, const sf_orb_params* orb) {
  OrbSel S = {};
  S.n_levels = P.n; S.score_type = det->score_type; S.edge = orb->edge_threshold; S.max_features = max_features;
  sf_orb_quotas(max_features, det->scale_factor, det->n_levels, S.quota);
  return S;
}

// What sf_launch_detect_orb keeps on the device for n_img images, from the image size, n_img and max_features alone
// (a level of w x h pixels holds at most ceil(w / 2) ceil(h / 2) strict 3 x 3 maxima):
//   c->orb_pyr     P.total bytes per image            the pyramid (the extraction reuses it)
//   c->gf_planes   P.total bytes per image            FAST score planes
//   c->gf_keys     8 bytes per candidate              FAST keys, level by level
//   c->orb_work    40 bytes per candidate + 2 x 28 bytes per keypoint (min(candidates, max_features) per image)
//   c->gf_scalar   S_WORDS + 8 + 6 words per image    scalar blocks, FAST counts, segment bounds
static unsigned orb_level_cap(const SfOrbPyr& P, int l) { return (unsigned)(((P.w[l] + 1) / 2) * ((P.h[l] + 1) / 2)); }

// The detector on n_img images of one size (see the head of the file).  d_kpts_out [n_img][cap], d_n_out [n_img] (device):
// the keypoints of every image, their number (which `cap` does not clip).  max_features >= 1.  The three sorts share one
// SfSortBounds: a lone image's candidate count C comes to the host with the first sort and sizes all three -- past their
// own bounds the stage kernels have filled the lists up to C with keys that sort last.
int sf_launch_detect_orb(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                         int max_features, const sf_orb_detector_params* det, const sf_orb_params* orb, sf_keypoint* d_kpts_out,
                         int cap, int32_t* d_n_out) {
  const SfOrbPyr P = sf_orb_pyr_layout(width, height, det->scale_factor, det->n_levels);
  int rc;
  if (n_img < 1 || n_img > 65535) return sf_fail(c, SF_ERANGE, "ORB batch of %d images (1 .. 65535)", n_img);
  if ((rc = sf_launch_orb_pyramid(c, d_images, pitch, P, n_img, img_stride)) != SF_OK) return rc;
  OrbBatch B = {};
  B.img_stride = img_stride; B.pyr_stride = P.total; B.n_img = n_img; B.n_out = d_n_out;
  size_t per_image = 0;
  for (int l = 0; l < P.n; ++l) {
    B.key_cap[l] = orb_level_cap(P, l);
    per_image += B.key_cap[l];
  }
  const size_t entries = per_image * n_img;
  if (entries > 0xFFFFFFFFull) return sf_fail(c, SF_ERANGE, "ORB batch: %d images of up to %zu candidates", n_img, per_image);
  B.cand_cap = (unsigned)per_image;
  for (int l = 0, run = 0; l < P.n; ++l) {
    B.key_off[l] = (unsigned)run * (unsigned)n_img;
    run += (int)B.key_cap[l];
  }
  const int cap_tmp = (int)std::min<size_t>(per_image, (size_t)max_features);
  B.kp_cap = cap_tmp;
  const size_t sc_words = (size_t)n_img * (S_WORDS + SF_ORB_MAX_LEVELS + 6);
  if ((rc = sf_buf_reserve(c, c->gf_planes, (size_t)P.total * n_img)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->gf_keys, entries * sizeof(unsigned long long))) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->gf_scalar, sc_words * 4)) != SF_OK) return rc;
  OrbLists W;
  if ((rc = orb_lists(c, entries, (size_t)cap_tmp * n_img, &W)) != SF_OK) return rc;
  const uint8_t* pyr = (const uint8_t*)c->orb_pyr.p;
  uint8_t* score = (uint8_t*)c->gf_planes.p;
  unsigned long long* keys_f = (unsigned long long*)c->gf_keys.p;
  int* sc = (int*)c->gf_scalar.p;
  unsigned* count = (unsigned*)(sc + (size_t)n_img * S_WORDS);
  B.d_count = count;
  B.seg = count + (size_t)n_img * SF_ORB_MAX_LEVELS;
  // histograms, counts and bounds of the call before are gone before the first kernel reads them
  SF_HIP(c, hipMemsetAsync(sc, 0, sc_words * 4, c->stream));
  for (int l = 0; l < P.n; ++l) {
    if (P.w[l] < 7 || P.h[l] < 7) continue;            // (no FAST domain)
    sf_launch_fast_level(c, l == 0 ? d_images : pyr + P.off[l], l == 0 ? img_stride : (size_t)P.total, n_img, P.w[l], P.h[l],
                         l == 0 ? pitch : P.w[l], det->fast_threshold, 1, score + P.off[l], (size_t)P.total, keys_f + B.key_off[l],
                         count + (size_t)l * n_img, B.key_cap[l]);
  }
  SF_HIP(c, hipGetLastError());
  const OrbSel S = orb_selection(P, max_features, det, orb);
  const unsigned n = (unsigned)n_img, cap_all = (unsigned)entries;
  const dim3 block(256), grid((B.cand_cap + 255) / 256, n);
  SfSortBounds hb;
  hipLaunchKernelGGL(k_orb_gather, grid, block, 0, c->stream, (const unsigned long long*)keys_f, P, S, W.cand, sc, B);
  hipLaunchKernelGGL(k_orb_cut_a, dim3(n), dim3(64), 0, c->stream, S, sc, B);
  hipLaunchKernelGGL(k_orb_filter_a, grid, block, 0, c->stream, W.cand, (const int*)sc, B);
  SF_HIP(c, hipGetLastError());
  if ((rc = sf_sort_segments(c, W.cand, W.cand_s, cap_all, n, B.seg, B.seg + n, 8, 44, false, &hb)) != SF_OK) return rc;
  if (det->score_type == 0) {
    const unsigned most = n == 1 ? (unsigned)hb.n() : B.cand_cap;   // (a lone image's candidates are known by now)
    const unsigned blocks = std::max(std::min((most + 3) / 4, (unsigned)ORB_HARRIS_BLOCKS), 1u);
    hipLaunchKernelGGL(k_orb_harris, dim3(blocks, n), block, 0, c->stream, d_images, pitch, pyr, P,
                       (const unsigned long long*)W.cand_s, (const int*)sc, W.resp, W.key_b, B);
    SF_HIP(c, hipGetLastError());
    if ((rc = sf_sort_segments(c, W.key_b, W.key_bs, cap_all, n, B.seg + 2 * n, B.seg + 3 * n, 0, 36, false, &hb)) != SF_OK)
      return rc;
  }
  hipLaunchKernelGGL(k_orb_cut_b, dim3(n), dim3(64), 0, c->stream, S, (const unsigned long long*)W.key_bs, sc, B);
  hipLaunchKernelGGL(k_orb_compact, dim3(n), block, 0, c->stream, S, (const unsigned long long*)W.cand_s, (const float*)W.resp,
                     W.fin_key, W.fin_resp, W.key_c, sc, B);
  SF_HIP(c, hipGetLastError());
  if ((rc = sf_sort_segments(c, W.key_c, W.key_cs, cap_all, n, B.seg + 4 * n, B.seg + 5 * n, 0, 64, true, &hb)) != SF_OK) return rc;
  hipLaunchKernelGGL(k_orb_emit, dim3((cap_tmp + 255) / 256, n), block, 0, c->stream, P, (const unsigned long long*)W.key_cs,
                     (const unsigned long long*)W.fin_key, (const float*)W.fin_resp, (const int*)sc, cap_tmp, W.kp1, B);
  SF_HIP(c, hipGetLastError());
  if ((rc = sf_launch_orb_angle_levels(c, d_images, img_stride, n_img, pitch, P, P.total, W.kp1, cap_tmp, d_n_out,
                                       orb->edge_threshold, W.kp2)) != SF_OK)
    return rc;
  const int written = std::min(cap_tmp, cap);
  if (written > 0)
    hipLaunchKernelGGL(k_orb_finish, dim3((written + 255) / 256, n), block, 0, c->stream, P, (const sf_keypoint*)W.kp2,
                       (const int*)sc, written, d_kpts_out, B, cap);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
