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
//                      It also writes the segment bounds that a batch's segmented sort reads.
//   sf_sort_keys (sf_sort.hip) descending (bits 0 .. 40), segmented for a batch.  Keys are unique (the pixel index), so
//                      the order does not depend on the arrival order of the atomics.
//   k_fast_emit        the first min(count, max_features) keys -> sf_keypoint {x, y, 7, -1, score, 0, -1}
// FAST has no minimum-distance rule: no selection bitmap, no image-size limit beyond the 2^26 pixels of the index.
// The two launchers share fast_front (workspace, score / candidates / rekey); their tails differ: the single call sizes
// a plain sort by the corner count on the host, the batch sorts the segments whose bounds k_fast_rekey wrote.
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

// blockIdx.y = image.  Raster order when the corners fit the limit; segment bounds for the batch's sort.
__global__ void __launch_bounds__(256)
k_fast_rekey(unsigned long long* __restrict__ keys, const unsigned* __restrict__ count, unsigned key_cap, int limit,
             unsigned* __restrict__ seg_begin, unsigned* __restrict__ seg_end) {
  const unsigned img = blockIdx.y;
  const unsigned n = min(count[img], key_cap);
  if (seg_begin && blockIdx.x == 0 && threadIdx.x == 0) { seg_begin[img] = img * key_cap; seg_end[img] = img * key_cap + n; }
  if (limit > 0 && n > (unsigned)limit) return;
  keys += (size_t)img * key_cap;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const unsigned long long k = keys[i];
    keys[i] = FAST_RASTER | ((unsigned long long)(0xFFFFFFFFu - (unsigned)k) << 8) | (k >> 32);
  }
}

__global__ void __launch_bounds__(256)
k_fast_emit(const unsigned long long* __restrict__ keys, int n, int w, int limit, sf_keypoint* __restrict__ kp_out, int cap,
            int32_t* __restrict__ n_out, const unsigned* __restrict__ d_count, unsigned key_cap) {
  if (d_count) {     // batch: blockIdx.y = image, the corner count read on the device
    keys += (size_t)blockIdx.y * key_cap;
    n = (int)min(d_count[blockIdx.y], key_cap);
    kp_out += (size_t)blockIdx.y * cap;
    n_out += blockIdx.y;
  }
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

// The front half of both launchers -- workspace and the three front kernels for n_img images of one size: every image's
// keys, in the form of the order that applies to it, their count and its segment of the key array are on the device when
// the stream gets there
static int fast_front(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                      int max_features, const sf_fast_params* prm, const SfCells& cells, const SfMask& mask, SfDetectorWork* F) {
  int rc = sf_detector_work(c, width, height, n_img, (size_t)width * height, F);
  if (rc != SF_OK) return rc;
  sf_launch_fast_level(c, d_images, img_stride, n_img, width, height, pitch, prm->threshold, prm->nonmax_suppression,
                       (uint8_t*)c->gf_planes.p, (size_t)F->key_cap, F->keys, F->count, F->key_cap, cells, mask);
  hipLaunchKernelGGL(k_fast_rekey, dim3(FAST_REKEY_BLOCKS, n_img), dim3(256), 0, c->stream, F->keys, (const unsigned*)F->count,
                     F->key_cap, max_features, F->seg_begin, F->seg_end);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

// Launch sequence on the handle's stream.  The corner count crosses to the host once (the sort is sized by it); which
// order applies is decided on the device before that.
int sf_launch_detect_fast(sf_context* c, const uint8_t* d_image, int width, int height, int pitch, int max_features,
                          const sf_fast_params* prm, sf_keypoint* d_kpts_out, int cap, int32_t* n_out, const SfMask& mask) {
  SfDetectorWork F;
  int rc;
  if ((rc = fast_front(c, d_image, 0, 1, width, height, pitch, max_features, prm, SfCells(), mask, &F)) != SF_OK) return rc;
  unsigned h_count = 0;
  if ((rc = sf_word_to_host(c, F.count, &h_count)) != SF_OK) return rc;
  const int n = (int)std::min(h_count, F.key_cap);
  if (n > 0 && (rc = sf_sort_keys(c, F.keys, F.keys_sorted, (size_t)n, 0, FAST_KEY_BITS, true)) != SF_OK) return rc;
  const int total = (max_features > 0 && n > max_features) ? max_features : n;
  const int written = std::min(total, cap);
  hipLaunchKernelGGL(k_fast_emit, dim3(std::max((written + 255) / 256, 1), 1), dim3(256), 0, c->stream,
                     (const unsigned long long*)F.keys_sorted, n, width, max_features, d_kpts_out, cap, F.n_single,
                     (const unsigned*)nullptr, 0u);
  SF_HIP(c, hipGetLastError());
  return n_out ? sf_word_to_host(c, F.n_single, n_out) : SF_OK;
}

// The detector on a batch of images of one size, no host round trip: corner counts and the choice of order stay on the
// device, a segmented sort takes the place of the sort sized by the host.  d_kpts_out [n_img][cap], d_n_out [n_img]
// (device).  max_features > 0 here (the batch's outputs are sized by it).  With `cells` the n_img images are the cells of
// a grid inside n_img / cells.per_image images (width x height: one cell), keypoints in the cell's own coordinates.
int sf_launch_detect_fast_batch(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height,
                                int pitch, int max_features, const sf_fast_params* prm, sf_keypoint* d_kpts_out, int cap,
                                int32_t* d_n_out, const SfCells& cells, const SfMask& mask) {
  SfDetectorWork F;
  int rc;
  if ((rc = fast_front(c, d_images, img_stride, n_img, width, height, pitch, max_features, prm, cells, mask, &F)) != SF_OK) return rc;
  if ((rc = sf_sort_keys_segmented_desc(c, F.keys, F.keys_sorted, (unsigned)((size_t)F.key_cap * n_img), (unsigned)n_img,
                                        F.seg_begin, F.seg_end, 0, FAST_KEY_BITS)) != SF_OK)
    return rc;
  const int written = std::min(max_features, cap);
  hipLaunchKernelGGL(k_fast_emit, dim3(std::max((written + 255) / 256, 1), n_img), dim3(256), 0, c->stream,
                     (const unsigned long long*)F.keys_sorted, 0, width, max_features, d_kpts_out, cap, d_n_out,
                     (const unsigned*)F.count, F.key_cap);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
