// k_fast.hip -- SURVEY.md section 8 row f3, the second detector: FAST-9/16 as rtabmap's Vis/FeatureType 4 (FAST/BRIEF)
// runs it -- OpenCV's FAST_t<16> with its corner score and 3 x 3 non-maximum suppression, then rtabmap's
// Feature2D::limitKeypoints -- on the device, for the same three extraction calls that k_gftt.hip serves.  Neither
// upstream text is in the reference tree: the semantics are restated in tests/fast_ref.py, and
// because all of it is 8-bit integer work the kernels equal that restatement byte for byte with no summation order to
// decide.
//
//   k_fast_score       a 64 x 16 tile of the image plus a 3-pixel halo in LDS (dword loads).  Per pixel: the 16 ring
//                      differences d_k = I(p) - I(p + ring_k), a 16-bit mask of d_k > t (ring darker) and one of
//                      d_k < -t (ring brighter), "9 consecutive bits" by shift-and-AND on the doubled mask.  Only
//                      corners compute the score m(p) - 1, m = max over the 16 arcs of max(min d, min -d): 16 sliding
//                      minima (and maxima) of 9 by doubling -- 4 x 16 min, 4 x 16 max, two 16-way reductions: 160
//                      operations, 112 instructions per pixel in the compiled kernel (v_min3 / v_max3 fold pairs).  The
//                      alternative, a binary search on the threshold that reuses the mask test, costs 8 rounds of the
//                      mask build (32 compares + 32 selects and ORs: 95 instructions as compiled) + the test, about
//                      800: not chosen.  One byte per pixel: the score plane, 0 = no corner (a corner's score is >=
//                      threshold >= 1).
//   k_fast_candidates  3 x 3 suppression on the score plane (strictly greater than all 8 neighbours) -> 64-bit keys
//                      (score << 32 | pixel index), one global atomic per workgroup.  Without suppression every corner
//                      is a candidate with score 0 (upstream reads a score buffer it only fills under suppression).
//                      k_fast_candidates_masked: the same under a mask (sf_detect_fast_masked_device, the depth keyframe
//                      calls), corners on mask == 0 dropped.
//   k_fast_rekey       decides the order ON THE DEVICE once the count is known: corners <= max_features (or no limit)
//                      -> raster order, the keys become (1 << 40 | (2^32 - 1 - index) << 8 | score); otherwise they
//                      stay, and the descending sort below gives descending response with ties by descending index.
//                      It also writes the image's segment of the key array, which the sort reads.
//   sf_sort_segments (sf_sort.hip) descending (bits 0 .. 40), every image's segment on its own.  Keys are unique (the
//                      pixel index), so the order does not depend on the arrival order of the atomics.
//   k_fast_emit        the first min(count, max_features) keys -> sf_keypoint {x, y, 7, -1, score, 0, -1}
// FAST has no minimum-distance rule: no selection bitmap, no image-size limit beyond the 2^26 pixels of the index.
// One launcher, sf_launch_detect_fast, for one image and for many (blockIdx.y or .z = image): counts, bounds and the
// choice of order are read on the device; the sort alone treats a lone image differently (sf_sort_segments).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sf_front_device.hpp"

namespace {

constexpr int FAST_TW = 64, FAST_TH = 16;            // pixels per workgroup (256 threads, 4 rows each)
constexpr int FAST_LW = FAST_TW + 8;                 // LDS row: 4 bytes left of the tile (a whole dword), 4 right
constexpr int FAST_LH = FAST_TH + 6;
constexpr int FAST_KEY_BITS = 41;
constexpr unsigned long long FAST_RASTER = 1ull << 40;

__device__ __forceinline__ bool fast_run9(unsigned m) {
  m |= m << 16;                                      // the ring is cyclic: runs may wrap
  unsigned a = m & (m >> 1);                         // 2 in a row
  a &= a >> 2;                                       // 4
  a &= a >> 4;                                       // 8
  return (a & (m >> 8)) != 0u;                       // 9
}

__global__ void __launch_bounds__(256)
k_fast_score(const uint8_t* __restrict__ img, int w, int h, int pitch, int t, uint8_t* __restrict__ score, size_t img_stride,
             size_t plane_stride, SfCells cells) {
  // (blockIdx.z = image of a batch: images img_stride bytes apart -- or the cells of a grid inside them, sf_cell_base --
  // score planes plane_stride bytes apart.  The dword path is chosen per image: cells of one launch differ in alignment)
  __shared__ __attribute__((aligned(4))) uint8_t tile[FAST_LH * FAST_LW];
  img += sf_cell_base(blockIdx.z, img_stride, cells);
  score += blockIdx.z * plane_stride;
  const int x0 = blockIdx.x * FAST_TW, y0 = blockIdx.y * FAST_TH;
  const bool aligned = (((uintptr_t)img | (uintptr_t)pitch) & 3u) == 0u;
  for (int i = threadIdx.x; i < FAST_LH * (FAST_LW / 4); i += 256) {
    const int row = i / (FAST_LW / 4), col = i - row * (FAST_LW / 4);
    const int gy = y0 - 3 + row, gx = x0 - 4 + 4 * col;
    unsigned v = 0u;
    if (gy >= 0 && gy < h) {
      const uint8_t* p = img + (size_t)gy * pitch;
      if (aligned && gx >= 0 && gx + 4 <= w) {
        v = *(const unsigned*)(p + gx);
      } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
          if (gx + b >= 0 && gx + b < w) v |= (unsigned)p[gx + b] << (8 * b);
      }
    }
    ((unsigned*)tile)[i] = v;
  }
  __syncthreads();
  const int lx = threadIdx.x & 63, x = x0 + lx;
#pragma unroll
  for (int j = 0; j < FAST_TH / 4; ++j) {
    const int ly = (threadIdx.x >> 6) + 4 * j, y = y0 + ly;
    if (x >= w || y >= h) continue;
    int s = 0;
    if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
      const uint8_t* c = tile + (ly + 3) * FAST_LW + lx + 4;
      const int v = c[0];
      constexpr int RX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
      constexpr int RY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
      int d[16];
      unsigned dark = 0u, bright = 0u;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        d[k] = v - (int)c[RY[k] * FAST_LW + RX[k]];
        dark |= (d[k] > t ? 1u : 0u) << k;
        bright |= (d[k] < -t ? 1u : 0u) << k;
      }
      if (fast_run9(dark) || fast_run9(bright)) {
        int lo[16], hi[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { lo[k] = min(d[k], d[(k + 1) & 15]); hi[k] = max(d[k], d[(k + 1) & 15]); }
        int lo4[16], hi4[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { lo4[k] = min(lo[k], lo[(k + 2) & 15]); hi4[k] = max(hi[k], hi[(k + 2) & 15]); }
        int best_lo = -256, best_hi = 256;           // max over arcs of min d; min over arcs of max d
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const int lo8 = min(lo4[k], lo4[(k + 4) & 15]), hi8 = max(hi4[k], hi4[(k + 4) & 15]);
          best_lo = max(best_lo, min(lo8, d[(k + 8) & 15]));
          best_hi = min(best_hi, max(hi8, d[(k + 8) & 15]));
        }
        s = max(best_lo, -best_hi) - 1;              // m(p) - 1; m(p) > t >= 1 here
      }
    }
    score[(size_t)y * w + x] = (uint8_t)s;
  }
}

constexpr int FAST_CAND_ROWS = 16;                   // 64 x 16 pixels per workgroup of k_fast_candidates
// The body of the two candidate kernels.  MASKED (FastFeatureDetector::detect(image, keypoints, mask)): score and suppression
// have seen every pixel; a corner on a pixel whose mask byte is 0 is dropped here, before the count that limitKeypoints
// reads.  false: the kernel as it was, argument list included
template <bool MASKED>
__device__ __forceinline__ void
fast_candidates(const uint8_t* __restrict__ score, int w, int h, int nonmax, unsigned long long* __restrict__ keys,
                unsigned* __restrict__ count, unsigned cap, size_t plane_stride, const SfMask& mask) {
  const uint8_t* mk = MASKED ? mask.p + sf_cell_base(blockIdx.z, mask.stride, mask.cells) : nullptr;
  score += blockIdx.z * plane_stride;
  keys += (size_t)blockIdx.z * cap;
  count += blockIdx.z;
  __shared__ unsigned long long s_keys[64 * FAST_CAND_ROWS];
  __shared__ unsigned s_n, s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
#pragma unroll
  for (int j = 0; j < FAST_CAND_ROWS / 4; ++j) {
    const int y = blockIdx.y * FAST_CAND_ROWS + 4 * j + (threadIdx.x >> 6);
    // (the score plane is 0 outside 3 <= x < w - 3, 3 <= y < h - 3: every neighbour read below is inside the plane)
    if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
      const uint8_t* p = score + (size_t)y * w + x;
      const unsigned v = p[0];
      if (v && (!MASKED || mk[(size_t)y * mask.pitch + x] != 0)) {
        bool keep = true;
        if (nonmax) {
          const unsigned m = max(max(max(p[-w - 1], p[-w]), max(p[-w + 1], p[-1])),
                                 max(max(p[1], p[w - 1]), max(p[w], p[w + 1])));
          keep = v > m;
        }
        if (keep) {
          const unsigned q = atomicAdd(&s_n, 1u);
          s_keys[q] = ((unsigned long long)(nonmax ? v : 0u) << 32) | (unsigned)(y * w + x);
        }
      }
    }
  }
  sf_flush_staged_keys(s_keys, &s_n, &s_base, keys, count, cap);
}

__global__ void __launch_bounds__(256)
k_fast_candidates(const uint8_t* __restrict__ score, int w, int h, int nonmax, unsigned long long* __restrict__ keys,
                  unsigned* __restrict__ count, unsigned cap, size_t plane_stride) {
  fast_candidates<false>(score, w, h, nonmax, keys, count, cap, plane_stride, SfMask());
}

__global__ void __launch_bounds__(256)
k_fast_candidates_masked(const uint8_t* __restrict__ score, int w, int h, int nonmax, unsigned long long* __restrict__ keys,
                         unsigned* __restrict__ count, unsigned cap, size_t plane_stride, SfMask mask) {
  fast_candidates<true>(score, w, h, nonmax, keys, count, cap, plane_stride, mask);
}

// blockIdx.y = image.  Raster order when the corners fit the limit; the image's segment of the key array for the sort.
__global__ void __launch_bounds__(256)
k_fast_rekey(unsigned long long* __restrict__ keys, const unsigned* __restrict__ count, unsigned key_cap, int limit,
             unsigned* __restrict__ seg_begin, unsigned* __restrict__ seg_end) {
  const unsigned img = blockIdx.y;
  const unsigned n = min(count[img], key_cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) { seg_begin[img] = img * key_cap; seg_end[img] = img * key_cap + n; }
  if (limit > 0 && n > (unsigned)limit) return;
  keys += (size_t)img * key_cap;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned long long k = keys[i];
    keys[i] = FAST_RASTER | ((unsigned long long)(0xFFFFFFFFu - (unsigned)k) << 8) | (k >> 32);
  }
}

__global__ void __launch_bounds__(256)
k_fast_emit(const unsigned long long* __restrict__ keys, int w, int limit, sf_keypoint* __restrict__ kp_out, int cap,
            int32_t* __restrict__ n_out, const unsigned* __restrict__ count, unsigned key_cap) {
  // blockIdx.y = image, its corner count read here
  keys += (size_t)blockIdx.y * key_cap;
  const int n = (int)min(count[blockIdx.y], key_cap);
  kp_out += (size_t)blockIdx.y * cap;
  n_out += blockIdx.y;
  const int total = (limit > 0 && n > limit) ? limit : n;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *n_out = total;
  if (i >= total || i >= cap) return;
  const unsigned long long key = keys[i];
  const bool raster = (key & FAST_RASTER) != 0ull;
  const unsigned idx = raster ? 0xFFFFFFFFu - (unsigned)(key >> 8) : (unsigned)key;
  const unsigned s = raster ? (unsigned)(key & 0xFFull) : (unsigned)(key >> 32);
  const int y = (int)(idx / (unsigned)w), x = (int)(idx - (unsigned)y * (unsigned)w);
  kp_out[i] = sf_make_keypoint((float)x, (float)y, 7.0f, (float)s, 0);
}

constexpr int FAST_REKEY_BLOCKS = 32;

}  // namespace

// One level on n_img images of one size (blockIdx.z = image): the two launches every detector shares (FAST/BRIEF here,
// ORB's pyramid levels in k_orb_detect.hip)
void sf_launch_fast_level(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                          int threshold, int nonmax, uint8_t* score, size_t plane_stride, unsigned long long* keys, unsigned* count,
                          unsigned key_cap, const SfCells& cells, const SfMask& mask) {
  const dim3 block(256);
  hipLaunchKernelGGL(k_fast_score, dim3((width + FAST_TW - 1) / FAST_TW, (height + FAST_TH - 1) / FAST_TH, n_img), block, 0,
                     c->stream, d_images, width, height, pitch, threshold, score, img_stride, plane_stride, cells);
  const dim3 grid_c((width + 63) / 64, (height + FAST_CAND_ROWS - 1) / FAST_CAND_ROWS, n_img);
  if (mask.p)
    hipLaunchKernelGGL(k_fast_candidates_masked, grid_c, block, 0, c->stream, (const uint8_t*)score, width, height, nonmax, keys,
                       count, key_cap, plane_stride, mask);
  else
    hipLaunchKernelGGL(k_fast_candidates, grid_c, block, 0, c->stream, (const uint8_t*)score, width, height, nonmax, keys, count,
                       key_cap, plane_stride);
}

// The detector on n_img images of one size: corner counts and the choice of order stay on the device, every image's keys
// are its segment of the sort, k_fast_emit reads the counts there.  d_kpts_out [n_img][cap], d_n_out [n_img] (device).
// With `cells` the n_img images are the cells of a grid inside n_img / cells.per_image images (width x height: one cell),
// keypoints in the cell's own coordinates.  The emit grid is sized by max_features, or -- one image, whose corner count
// the sort has brought to the host -- by the keypoints there are.
int sf_launch_detect_fast(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                          int max_features, const sf_fast_params* prm, sf_keypoint* d_kpts_out, int cap, int32_t* d_n_out,
                          const SfCells& cells, const SfMask& mask) {
  SfDetectorWork F;
  SfSortBounds hb;
  int rc;
  if ((rc = sf_check_limit(c, n_img, max_features)) != SF_OK) return rc;
  if ((rc = sf_detector_work(c, width, height, n_img, (size_t)width * height, &F)) != SF_OK) return rc;
  sf_launch_fast_level(c, d_images, img_stride, n_img, width, height, pitch, prm->threshold, prm->nonmax_suppression,
                       (uint8_t*)c->gf_planes.p, (size_t)F.key_cap, F.keys, F.count, F.key_cap, cells, mask);
  hipLaunchKernelGGL(k_fast_rekey, dim3(FAST_REKEY_BLOCKS, n_img), dim3(256), 0, c->stream, F.keys, (const unsigned*)F.count,
                     F.key_cap, max_features, F.seg_begin, F.seg_end);
  SF_HIP(c, hipGetLastError());
  if ((rc = sf_sort_segments(c, F.keys, F.keys_sorted, (unsigned)((size_t)F.key_cap * n_img), (unsigned)n_img, F.seg_begin,
                             F.seg_end, 0, FAST_KEY_BITS, true, &hb)) != SF_OK)
    return rc;
  const int written = std::min(n_img == 1 ? sf_limit_keypoints(hb.n(), max_features) : max_features, cap);
  hipLaunchKernelGGL(k_fast_emit, dim3(std::max((written + 255) / 256, 1), n_img), dim3(256), 0, c->stream,
                     (const unsigned long long*)F.keys_sorted, width, max_features, d_kpts_out, cap, d_n_out,
                     (const unsigned*)F.count, F.key_cap);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
