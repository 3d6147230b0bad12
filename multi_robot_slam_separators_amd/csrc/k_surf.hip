// k_surf.hip -- SURF of the keyframe front end (Vis/FeatureType 0): cv::xfeatures2d::SURF of OpenCV 3.2 as rtabmap drives
// it, the only type with float32 rows (64 or 128 dimensions, a handle with desc_type 1).  opencv_contrib is not in the
// reference tree; the algorithm is restated in DESIGN.md section 3 item 17h and in tests/surf_ref.py, which the tests
// compare with byte for byte.  Arithmetic: the float operations in the order written, no contraction (compiled with
// -ffp-contract=off); float64 where upstream accumulates in double (the Haar sums, the squared magnitude) and for the
// window's sampling positions; integers for the box sums and for the area reduction of the window, which therefore
// needs no summation order.
//
//   k_surf_hessian   one thread per (layer, sample), all n_octaves (n_octave_layers + 2) layers in one launch (blockIdx.y
//                    = layer): 10 box sums on the int32 integral image that BRIEF and FREAK build -> det and trace
//                    planes of (h >> o) x (w >> o) floats; the box corners follow from the layer's size, no table.
//                    Samples whose filter leaves the image, and layers larger than the image, are written as zero.
//   k_surf_maxima    one thread per middle-layer sample: threshold, the 26-neighbour test, the 3 x 3 solve; a keypoint
//                    appends ONE 64-bit key (response bits << 32 | 2^32 - 1 - position) through a wave-aggregated
//                    atomic.  position = the sample's offset in the enumeration of all middle layers, so keys are
//                    unique and a descending sort gives descending response, then layer, then sample -- whatever
//                    order the atomics arrived in.  The counter counts past the capacity.
//   k_surf_segments  the decisions about an image's list (blockIdx.y = image): reads the image's count; more than the key
//                    capacity: the image is counted as overflowed and gets an empty segment; else, where limitKeypoints
//                    will cut the list, the rekey (position bits flipped: equal responses by DESCENDING position), and
//                    the image's segment of the key array for the sort
//   sf_sort_segments (sf_sort.hip) descending, 64 bits
//   k_surf_emit      the first min(count, max_features) keys -> keypoints, the interpolation done again from the planes
//                    (blockIdx.y = image, count and rekey flag read on the device, the count written)
// One launcher, sf_launch_detect_surf, for one image and for many; sf_detect_surf_device runs it on one image and turns
// an overflow into its refusal.
//   k_surf_describe  one workgroup of 512 per keypoint.  Wavefront 0: the 109 orientation samples over its lanes in two
//                    rounds (Haar responses, weights, cvRound(fastAtan2)) into LDS; lanes 0 .. 63 and 0 .. 7 again sum
//                    the 72 windows, each in sample order; the best window by a butterfly that prefers the lower
//                    index.  All eight wavefronts: the (int)(21 s) window -- hundreds of pixels square for large
//                    keypoints, never stored -- is cut into work items (patch cell, slice of the cell's rows); a thread
//                    samples its item bilinearly on the fly and adds overlap x value to the cell's 64-bit integer in LDS
//                    (ds_add_u64: integers, so no order to keep); 441 exact means make the 21 x 21 patch.  Wavefront 0
//                    again: lane 4 c + q sums component q of cell c over its 25 gradients in raster order (two
//                    components with extended = 1); then a thread per dimension adds the squares in row order, in
//                    float64, and scales its own value.  LDS: the patch 441 bytes, its accumulators 3528, X, Y and the
//                    angles 1308 (the row reuses X).  Thread 0 writes the keypoint with its angle and does the 3D point
//                    (extract_point).  One wavefront per keypoint was tried first: a keypoint of size 200 has 217 000
//                    samples, each four dependent byte loads, and its one wavefront took 1.9 ms while the chip idled.
// The integral image before k_surf_describe and k_extract_commit behind it are k_extract.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "sf_extract_device.hpp"
#include "sf_front_device.hpp"

namespace {

constexpr int SURF_HAAR0 = 9, SURF_HAAR_INC = 6;
constexpr int SURF_PW = SURF_PATCH + 1;             // the patch is 21 x 21: 20 x 20 gradients
constexpr float SURF_MAX_SIZE = 1.0e6f;             // keypoint sizes and coordinates beyond it are dropped

// The planes of a width x height image: octave o holds n_layers + 2 planes of (h >> o) x (w >> o) floats from
// plane_off[o] on; the samples of its n_layers middle layers are numbered from pos_off[o] on (the sort's tie-break)
struct SurfLayout {
  int w, h, n_octaves, n_layers;
  unsigned plane_off[SURF_MAX_OCTAVES], pos_off[SURF_MAX_OCTAVES + 1];
};

// Image blockIdx.z of a detector launch: its integral image, its det and trace planes and its keys lie this many
// entries behind those of image 0 (one image: all zero); its count, segment bounds and flag at index blockIdx.z
struct SurfBatch {
  size_t s_stride, plane_stride, key_stride;
};

__host__ __device__ __forceinline__ int surf_size(int o, int l) { return (SURF_HAAR0 + SURF_HAAR_INC * l) << o; }

// (float)(the box sum) * weight; unsigned arithmetic: the four terms may wrap, the box itself fits an int
__device__ __forceinline__ float surf_box(const int32_t* __restrict__ S, size_t w1, int y, int x, int x1, int y1, int x2, int y2,
                                          float wt) {
  const unsigned a = (unsigned)S[(size_t)(y + y1) * w1 + (x + x1)], d = (unsigned)S[(size_t)(y + y2) * w1 + (x + x2)];
  const unsigned b = (unsigned)S[(size_t)(y + y2) * w1 + (x + x1)], c = (unsigned)S[(size_t)(y + y1) * w1 + (x + x2)];
  return (float)(int)(a + d - b - c) * wt;
}

// resizeHaarPattern's weight: w / ((float)(x2 - x1) * (y2 - y1))
__device__ __forceinline__ float surf_weight(float wt, int dx, int dy) { return wt / ((float)dx * (float)dy); }

__global__ void __launch_bounds__(256)
k_surf_hessian(const int32_t* __restrict__ S, SurfLayout L, float* __restrict__ det, float* __restrict__ trace, SurfBatch B) {
  S += blockIdx.z * B.s_stride; det += blockIdx.z * B.plane_stride; trace += blockIdx.z * B.plane_stride;
  const int index = blockIdx.y;
  const int o = index / (L.n_layers + 2), l = index - o * (L.n_layers + 2);
  const int step = 1 << o, size = surf_size(o, l);
  const int rows = L.h >> o, cols = L.w >> o;
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= (unsigned)(rows * cols)) return;
  const int pi = (int)(e / (unsigned)cols), pj = (int)(e - (unsigned)pi * (unsigned)cols);
  float d = 0.0f, t = 0.0f;
  if (size <= L.h && size <= L.w) {
    const int ni = 1 + (L.h - size) / step, nj = 1 + (L.w - size) / step, margin = (size / 2) / step;
    const int i = pi - margin, j = pj - margin;
    if (i >= 0 && i < ni && j >= 0 && j < nj) {
      const float ratio = (float)size / 9.0f;
      const int r1 = (int)rintf(ratio * 1.0f), r2 = (int)rintf(ratio * 2.0f), r3 = (int)rintf(ratio * 3.0f),
                r4 = (int)rintf(ratio * 4.0f), r5 = (int)rintf(ratio * 5.0f), r6 = (int)rintf(ratio * 6.0f),
                r7 = (int)rintf(ratio * 7.0f), r8 = (int)rintf(ratio * 8.0f), r9 = (int)rintf(ratio * 9.0f);
      const size_t w1 = (size_t)(L.w + 1);
      const int y = i * step, x = j * step;
      // Dx {0 2 3 7 1} {3 2 6 7 -2} {6 2 9 7 1}; Dy the transpose; Dxy {1 1 4 4 1} {5 1 8 4 -1} {1 5 4 8 -1} {5 5 8 8 1}
      double s = 0.0;
      s += (double)surf_box(S, w1, y, x, 0, r2, r3, r7, surf_weight(1.0f, r3, r7 - r2));
      s += (double)surf_box(S, w1, y, x, r3, r2, r6, r7, surf_weight(-2.0f, r6 - r3, r7 - r2));
      s += (double)surf_box(S, w1, y, x, r6, r2, r9, r7, surf_weight(1.0f, r9 - r6, r7 - r2));
      const float dx = (float)s;
      s = 0.0;
      s += (double)surf_box(S, w1, y, x, r2, 0, r7, r3, surf_weight(1.0f, r7 - r2, r3));
      s += (double)surf_box(S, w1, y, x, r2, r3, r7, r6, surf_weight(-2.0f, r7 - r2, r6 - r3));
      s += (double)surf_box(S, w1, y, x, r2, r6, r7, r9, surf_weight(1.0f, r7 - r2, r9 - r6));
      const float dy = (float)s;
      s = 0.0;
      s += (double)surf_box(S, w1, y, x, r1, r1, r4, r4, surf_weight(1.0f, r4 - r1, r4 - r1));
      s += (double)surf_box(S, w1, y, x, r5, r1, r8, r4, surf_weight(-1.0f, r8 - r5, r4 - r1));
      s += (double)surf_box(S, w1, y, x, r1, r5, r4, r8, surf_weight(-1.0f, r4 - r1, r8 - r5));
      s += (double)surf_box(S, w1, y, x, r5, r5, r8, r8, surf_weight(1.0f, r8 - r5, r8 - r5));
      const float dxy = (float)s;
      d = dx * dy - 0.81f * dxy * dxy;
      t = dx + dy;
    }
  }
  const size_t out = (size_t)L.plane_off[o] + (size_t)l * rows * cols + e;
  det[out] = d;
  trace[out] = t;
}

// A middle-layer sample (octave o, layer l, plane position pi, pj; inside the margin of the layer above): whether it is a
// maximum of its 3 x 3 x 3 neighbourhood above thr and survives interpolateKeypoint, and the keypoint it gives
__device__ __forceinline__ bool surf_keypoint(const SurfLayout& L, const float* __restrict__ det, const float* __restrict__ trace,
                                              float thr, int o, int l, int pi, int pj, sf_keypoint* out) {
  const int step = 1 << o, size = surf_size(o, l), rows = L.h >> o, cols = L.w >> o;
  const size_t plane = (size_t)rows * cols;
  const float* c1 = det + (size_t)L.plane_off[o] + (size_t)l * plane + (size_t)pi * cols + pj;
  const float v = c1[0];
  if (!(v > thr)) return false;
  float N[3][3][3];                                  // [layer][row][column]
  bool is_max = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int di = 0; di < 3; ++di)
#pragma unroll
      for (int dj = 0; dj < 3; ++dj) {
        const float q = (c1 + (ptrdiff_t)(k - 1) * (ptrdiff_t)plane)[(di - 1) * cols + (dj - 1)];
        N[k][di][dj] = q;
        if (k != 1 || di != 1 || dj != 1) is_max = is_max && v > q;
      }
  if (!is_max) return false;
  // interpolateKeypoint: b and the symmetric A; Cramer's rule in the order of tests/surf_ref.py solve3
  const float b0 = -((N[1][1][2] - N[1][1][0]) * 0.5f), b1 = -((N[1][2][1] - N[1][0][1]) * 0.5f),
              b2 = -((N[2][1][1] - N[0][1][1]) * 0.5f);
  const float c2 = 2.0f * N[1][1][1];
  const float a00 = (N[1][1][0] - c2) + N[1][1][2], a11 = (N[1][0][1] - c2) + N[1][2][1], a22 = (N[0][1][1] - c2) + N[2][1][1];
  const float a01 = (((N[1][2][2] - N[1][2][0]) - N[1][0][2]) + N[1][0][0]) * 0.25f;
  const float a02 = (((N[2][1][2] - N[2][1][0]) - N[0][1][2]) + N[0][1][0]) * 0.25f;
  const float a12 = (((N[2][2][1] - N[2][0][1]) - N[0][2][1]) + N[0][0][1]) * 0.25f;
  const float a10 = a01, a20 = a02, a21 = a12;
  const float m0 = a11 * a22 - a12 * a21, m1 = a10 * a22 - a12 * a20, m2 = a10 * a21 - a11 * a20;
  const float dt = (a00 * m0 - a01 * m1) + a02 * m2;
  const float d = 1.0f / dt;
  const float p = b1 * a22 - a12 * b2, q = b1 * a21 - a11 * b2, r = a10 * b2 - b1 * a20;
  const float x0 = d * ((b0 * m0 - a01 * p) + a02 * q);
  const float x1 = d * ((a00 * p - b0 * m1) + a02 * r);
  const float x2 = d * ((b0 * m2 - a01 * r) - a00 * q);
  if (!(dt != 0.0f) || !isfinite(x0) || !isfinite(x1) || !isfinite(x2)) return false;
  if (!(x0 != 0.0f || x1 != 0.0f || x2 != 0.0f) || !(fabsf(x0) <= 1.0f && fabsf(x1) <= 1.0f && fabsf(x2) <= 1.0f)) return false;
  const int half = (size / 2) / step, ds = size - surf_size(o, l - 1);
  const float centre = (float)(size - 1) * 0.5f;
  const float tr = trace[(size_t)L.plane_off[o] + (size_t)l * plane + (size_t)pi * cols + pj];
  out->x = ((float)(step * (pj - half)) + centre) + x0 * (float)step;
  out->y = ((float)(step * (pi - half)) + centre) + x1 * (float)step;
  out->size = rintf((float)size + x2 * (float)ds);
  out->angle = -1.0f;
  out->response = v;
  out->octave = o;
  out->class_id = (tr > 0.0f) - (tr < 0.0f);
  return true;
}

__global__ void __launch_bounds__(256)
k_surf_maxima(SurfLayout L, const float* __restrict__ det, const float* __restrict__ trace, float thr,
              unsigned long long* __restrict__ keys, unsigned* __restrict__ count, unsigned cap, SurfBatch B) {
  det += blockIdx.z * B.plane_stride; trace += blockIdx.z * B.plane_stride;
  keys += blockIdx.z * B.key_stride; count += blockIdx.z;
  const int m = blockIdx.y;                          // middle layer l = 1 .. n_layers of octave o
  const int o = m / L.n_layers, l = 1 + m - o * L.n_layers;
  const int step = 1 << o, rows = L.h >> o, cols = L.w >> o;
  const int margin = (surf_size(o, l + 1) / 2) / step + 1;   // a 3 x 3 neighbourhood inside the layer above
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  bool found = false;
  sf_keypoint k;
  if (e < (unsigned)(rows * cols)) {
    const int pi = (int)(e / (unsigned)cols), pj = (int)(e - (unsigned)pi * (unsigned)cols);
    if (pi >= margin && pi < rows - margin && pj >= margin && pj < cols - margin)
      found = surf_keypoint(L, det, trace, thr, o, l, pi, pj, &k);
  }
  const unsigned long long bal = __ballot(found);
  if (bal == 0ull) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)bal) - 1;
  unsigned base = 0u;
  if (lane == leader) base = atomicAdd(count, (unsigned)__popcll(bal));
  base = (unsigned)__shfl((int)base, leader);
  if (!found) return;
  const unsigned slot = base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
  if (slot >= cap) return;                           // (the counter has counted it: the image is refused, or marked as overflowed)
  const unsigned pos = L.pos_off[o] + (unsigned)(l - 1) * (unsigned)(rows * cols) + e;
  keys[slot] = ((unsigned long long)__float_as_uint(k.response) << 32) | (unsigned long long)(0xFFFFFFFFu - pos);
}

// key i of a sorted list -> its keypoint, the interpolation done again from the planes
__device__ __forceinline__ sf_keypoint surf_emit_one(const SurfLayout& L, const float* __restrict__ det, const float* __restrict__ trace,
                                                     float thr, unsigned long long key, int flipped) {
  const unsigned low = (unsigned)key;
  const unsigned pos = flipped ? low : 0xFFFFFFFFu - low;
  int o = 0;
  while (o + 1 < L.n_octaves && pos >= L.pos_off[o + 1]) ++o;
  const unsigned plane = (unsigned)((L.h >> o) * (L.w >> o)), rel = pos - L.pos_off[o];
  const int l = 1 + (int)(rel / plane), cols = L.w >> o;
  const unsigned e = rel - (unsigned)(l - 1) * plane;
  sf_keypoint k;
  // (the same function on the same planes as k_surf_maxima: it finds the keypoint again)
  if (!surf_keypoint(L, det, trace, thr, o, l, (int)(e / (unsigned)cols), (int)(e % (unsigned)cols), &k))
    k = sf_make_keypoint(0.0f, 0.0f, 0.0f, 0.0f, 0);
  return k;
}

// ---- the decisions about an image's list, per image on the device -------------------------------------------------------
constexpr int SURF_SEGMENT_BLOCKS = 32;

// blockIdx.y = image.  count / seg_begin / seg_end / flipped: [images of the launch]; the segment bounds count from the
// launch's first key.  More maxima than cap_img: the image is counted in *overflowed and gets an empty segment.  More
// than max_features: limitKeypoints will cut the list, and the position bits are flipped, so that equal responses sort by
// DESCENDING position -- the rule FAST and ORB share (tests/orb2_ref.py limit_keypoints).
__global__ void __launch_bounds__(256)
k_surf_segments(unsigned long long* __restrict__ keys, const unsigned* __restrict__ count, unsigned cap_img, size_t key_stride,
                int max_features, unsigned* __restrict__ seg_begin, unsigned* __restrict__ seg_end, unsigned* __restrict__ flipped,
                unsigned* __restrict__ overflowed) {
  const unsigned img = blockIdx.y;
  const unsigned n = count[img];
  const bool over = n > cap_img;
  const bool cut = !over && max_features > 0 && n > (unsigned)max_features;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned begin = (unsigned)(img * key_stride);
    seg_begin[img] = begin;
    seg_end[img] = begin + (over ? 0u : n);
    flipped[img] = cut ? 1u : 0u;
    if (over) atomicAdd(overflowed, 1u);
  }
  if (!cut) return;
  keys += img * key_stride;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) keys[i] ^= 0xFFFFFFFFull;
}

// blockIdx.y = image: the first min(count, max_features) sorted keys of the image -> kp_out [image][cap], n_out [image];
// an overflowed image: no keypoint
__global__ void __launch_bounds__(256)
k_surf_emit(SurfLayout L, const float* __restrict__ det, const float* __restrict__ trace, float thr,
            const unsigned long long* __restrict__ keys, const unsigned* __restrict__ count, const unsigned* __restrict__ flipped,
            unsigned cap_img, int max_features, sf_keypoint* __restrict__ kp_out, int cap, int32_t* __restrict__ n_out, SurfBatch B) {
  const unsigned img = blockIdx.y;
  const unsigned n = count[img];
  int total = n > cap_img ? 0 : (int)n;
  if (max_features > 0 && total > max_features) total = max_features;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) n_out[img] = total;
  if (i >= total || i >= cap) return;
  det += img * B.plane_stride; trace += img * B.plane_stride;
  kp_out[(size_t)img * cap + i] = surf_emit_one(L, det, trace, thr, keys[img * B.key_stride + i], (int)flipped[img]);
}

// ---- orientation and descriptor ------------------------------------------------------------------------------------------
// One sample of the keypoint's window, the value of a uint8 pixel
struct SurfWindow {
  float start_x, start_y, sin_dir, cos_dir;          // rotated: float32 start and steps, positions in float64
  int sx, sy, upright;                               // upright: integer start
};

__device__ __forceinline__ int surf_sample(const uint8_t* __restrict__ img, int pitch, int w, int h, const SurfWindow& W, int i,
                                           int j) {
  if (W.upright) {
    const int x = min(max(W.sx + i, 0), w - 1), y = min(max(W.sy - j, 0), h - 1);
    return img[(size_t)y * pitch + x];
  }
  const double px = ((double)W.start_x + (double)i * (double)W.sin_dir) + (double)j * (double)W.cos_dir;
  const double py = ((double)W.start_y + (double)i * (double)W.cos_dir) - (double)j * (double)W.sin_dir;
  const double fx = floor(px), fy = floor(py);
  if (fx >= 0.0 && fx < (double)(w - 1) && fy >= 0.0 && fy < (double)(h - 1)) {
    const float a = (float)(px - fx), b = (float)(py - fy);
    const uint8_t* p = img + (size_t)(int)fy * pitch + (int)fx;
    float v = ((float)p[0] * (1.0f - a)) * (1.0f - b) + ((float)p[1] * a) * (1.0f - b) + ((float)p[pitch] * (1.0f - a)) * b;
    v = v + ((float)p[pitch + 1] * a) * b;
    return (int)rintf(v);
  }
  const int x = (int)fmin(fmax(rint(px), 0.0), (double)(w - 1)), y = (int)fmin(fmax(rint(py), 0.0), (double)(h - 1));
  return img[(size_t)y * pitch + x];
}

constexpr int SURF_DESCRIBE_THREADS = 512;          // 8 wavefronts: the window's samples are spread over all of them

__global__ void __launch_bounds__(SURF_DESCRIBE_THREADS)
k_surf_describe(const uint8_t* __restrict__ img, int pitch, const int32_t* __restrict__ S, int w, int h,
                const sf_keypoint* __restrict__ kpts, const float* __restrict__ right_x, const uint8_t* __restrict__ status, int n,
                SfSurfTables T, ExtractCam cam, sf_keypoint* __restrict__ kpts_out, float* __restrict__ desc_tmp,
                float* __restrict__ xyz_tmp, uint8_t* __restrict__ keep, ExtractBatch B) {
  __shared__ float s_xy[2 * SURF_ORI_SAMPLES];       // X then Y of the orientation samples; later the row (<= 128 floats)
  __shared__ int s_ang[SURF_ORI_SAMPLES];            // cvRound(angle); -1: the sample fell outside the image
  __shared__ unsigned long long s_acc[SURF_PW * SURF_PW];   // overlap x value of every patch cell, exact
  __shared__ uint8_t s_patch[SURF_PW * SURF_PW];
  __shared__ int s_ctl[2];                           // wavefront 0 -> all: the keypoint stays, its direction's bits
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x;
  if (B.d_n) n = min(n, B.d_n[blockIdx.y]);
  if (i >= n) return;                                // (the whole workgroup)
  const int dims = T.extended ? 128 : 64;
  {
    const size_t o = (size_t)blockIdx.y * B.per_image;
    img += blockIdx.y * B.img_stride;
    S += blockIdx.y * B.s_stride;
    kpts += o; kpts_out += o;
    if (right_x) right_x += o;
    if (status) status += o;
    desc_tmp += o * dims; xyz_tmp += 3 * o; keep += o;
  }
  sf_keypoint k = kpts[i];
  // (every thread holds the same keypoint: the conditions around the barriers below are the same in every thread)
  bool inside = k.size > 0.0f && k.size < SURF_MAX_SIZE && fabsf(k.x) < SURF_MAX_SIZE && fabsf(k.y) < SURF_MAX_SIZE;
  float s = 0.0f;
  int grad = 0;
  if (inside) {
    s = k.size * 1.2f / 9.0f;
    grad = 2 * (int)rintf(2.0f * s);                 // the gradient wavelet's side, even
    inside = grad >= 2 && h + 1 >= grad && w + 1 >= grad;
  }
  float dir = 270.0f;
  if (inside && !T.upright) {                        // orientation: wavefront 0, the others wait at the barriers
    if (wave == 0) {
      const float half = (float)(grad - 1) / 2.0f;
      const int g2 = grad / 2;
      const float wt = 1.0f / ((float)g2 * (float)grad);
      const size_t w1 = (size_t)(w + 1);
      bool any = false;
      for (int round = 0; round < 2; ++round) {      // (every lane runs both rounds: the ballot below needs them all)
        const int kk = lane + 64 * round;
        bool ok = false;
        float X = 0.0f, Y = 0.0f;
        int ang = -1;
        if (kk < SURF_ORI_SAMPLES) {
          const int x = (int)rintf((k.x + (float)T.ori_xy[2 * kk] * s) - half);
          const int y = (int)rintf((k.y + (float)T.ori_xy[2 * kk + 1] * s) - half);
          ok = !(y < 0 || y >= h + 1 - grad || x < 0 || x >= w + 1 - grad);
          if (ok) {
            double sum = 0.0;                        // dx {0 0 2 4 -1} {2 0 4 4 1}, dy {0 0 4 2 1} {0 2 4 4 -1} of the 4 x 4 frame
            sum += (double)surf_box(S, w1, y, x, 0, 0, g2, grad, -wt);
            sum += (double)surf_box(S, w1, y, x, g2, 0, grad, grad, wt);
            const float vx = (float)sum;
            sum = 0.0;
            sum += (double)surf_box(S, w1, y, x, 0, 0, grad, g2, wt);
            sum += (double)surf_box(S, w1, y, x, 0, g2, grad, grad, -wt);
            const float vy = (float)sum;
            const float g = T.ori_w[kk];
            X = vx * g; Y = vy * g;
            ang = (int)rintf(sf_fast_atan2(Y, X));
          }
          s_xy[kk] = X; s_xy[SURF_ORI_SAMPLES + kk] = Y; s_ang[kk] = ang;
        }
        any = any || __ballot(ok) != 0ull;
      }
      if (lane == 0) s_ctl[0] = any;
    }
    __syncthreads();
    if (wave == 0 && s_ctl[0]) {
      float best_mod = 0.0f, best_x = 0.0f, best_y = 0.0f;
      int best_i = 1 << 30;
      for (int wi = lane; wi < 360 / 5; wi += 64) {   // window wi: the samples within 30 degrees of 5 wi
        const int deg = 5 * wi;
        float sumx = 0.0f, sumy = 0.0f;
        for (int j = 0; j < SURF_ORI_SAMPLES; ++j) {
          const int a = s_ang[j], d = abs(a - deg);
          if (a >= 0 && (d < 30 || d > 330)) { sumx += s_xy[j]; sumy += s_xy[SURF_ORI_SAMPLES + j]; }
        }
        const float mod = sumx * sumx + sumy * sumy;
        if (mod > best_mod) { best_mod = mod; best_x = sumx; best_y = sumy; best_i = wi; }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {      // the largest; of equal ones the lowest window, as upstream's strict >
        const float om = __shfl_xor(best_mod, off), ox = __shfl_xor(best_x, off), oy = __shfl_xor(best_y, off);
        const int oi = __shfl_xor(best_i, off);
        if (om > best_mod || (om == best_mod && oi < best_i)) { best_mod = om; best_x = ox; best_y = oy; best_i = oi; }
      }
      if (lane == 0) s_ctl[1] = __float_as_int(sf_fast_atan2(-best_y, best_x));
    }
    __syncthreads();
    inside = s_ctl[0] != 0;
    if (inside) dir = __int_as_float(s_ctl[1]);
  }
  for (int p = tid; p < SURF_PW * SURF_PW; p += SURF_DESCRIBE_THREADS) s_acc[p] = 0ull;
  __syncthreads();
  int win = 1;
  if (inside) {
    k.angle = dir;
    win = (int)((float)SURF_PW * s);                 // >= 5: 2 s > 0.5 above
    const float off = -((float)(win - 1) / 2.0f);
    SurfWindow W;
    W.upright = T.upright;
    W.sx = W.sy = 0;
    W.start_x = W.start_y = W.sin_dir = W.cos_dir = 0.0f;
    if (T.upright) {
      W.sx = (int)rintf(k.x + off);
      W.sy = (int)rintf(k.y - off);
    } else {
      const float rad = dir * (float)(3.14159265358979323846 / 180.0);
      W.sin_dir = -(float)sin((double)rad);
      W.cos_dir = (float)cos((double)rad);
      W.start_x = (k.x + off * W.cos_dir) + off * W.sin_dir;
      W.start_y = (k.y - off * W.sin_dir) + off * W.cos_dir;
    }
    // work item = (patch cell p, slice q of its window rows): integer sums, so the order the slices arrive in changes nothing
    const int slices = min(max(win / SURF_PW, 1), 8);
    for (int item = tid; item < SURF_PW * SURF_PW * slices; item += SURF_DESCRIBE_THREADS) {
      const int q = item / (SURF_PW * SURF_PW), p = item - q * (SURF_PW * SURF_PW);
      const int r = p / SURF_PW, c = p - r * SURF_PW;
      // cell r covers [r win, (r + 1) win) in units of 1 / 21 window pixel, pixel i covers [21 i, 21 i + 21)
      const int i0 = (r * win) / SURF_PW, i1 = ((r + 1) * win - 1) / SURF_PW;
      const int j0 = (c * win) / SURF_PW, j1 = ((c + 1) * win - 1) / SURF_PW;
      unsigned long long acc = 0ull;
      for (int wi = i0 + q; wi <= i1; wi += slices) {
        const int ovi = min((r + 1) * win, SURF_PW * wi + SURF_PW) - max(r * win, SURF_PW * wi);
        unsigned long long row = 0ull;
        for (int wj = j0; wj <= j1; ++wj) {
          const int ovj = min((c + 1) * win, SURF_PW * wj + SURF_PW) - max(c * win, SURF_PW * wj);
          row += (unsigned long long)(unsigned)(ovj * surf_sample(img, pitch, w, h, W, wi, wj));
        }
        acc += (unsigned long long)(unsigned)ovi * row;
      }
      if (acc) atomicAdd(&s_acc[p], acc);
    }
  }
  __syncthreads();
  {
    const unsigned long long den = (unsigned long long)win * (unsigned long long)win;
    for (int p = tid; p < SURF_PW * SURF_PW; p += SURF_DESCRIBE_THREADS)
      s_patch[p] = (uint8_t)((2ull * s_acc[p] + den) / (2ull * den));   // the exact mean of the cell, halves up
  }
  __syncthreads();
  if (inside && wave == 0) {
    const int cell = lane >> 2, q = lane & 3, ci = cell >> 2, cj = cell & 3;
    float a0 = 0.0f, a1 = 0.0f;
    for (int y = 5 * ci; y < 5 * ci + 5; ++y)
      for (int x = 5 * cj; x < 5 * cj + 5; ++x) {
        const int p00 = s_patch[y * SURF_PW + x], p01 = s_patch[y * SURF_PW + x + 1];
        const int p10 = s_patch[(y + 1) * SURF_PW + x], p11 = s_patch[(y + 1) * SURF_PW + x + 1];
        const float dw = T.desc_w[y * SURF_PATCH + x];
        const float tx = (float)(p01 - p00 + p11 - p10) * dw, ty = (float)(p10 - p00 + p11 - p01) * dw;
        if (!T.extended) {                           // {sum dx, sum dy, sum |dx|, sum |dy|}
          a0 += q == 0 ? tx : q == 1 ? ty : q == 2 ? fabsf(tx) : fabsf(ty);
        } else if (q < 2) {                          // dx and |dx| where dy >= 0 (q 0) or dy < 0 (q 1)
          if ((ty >= 0.0f) == (q == 0)) { a0 += tx; a1 += fabsf(tx); }
        } else {                                     // dy and |dy| where dx >= 0 (q 2) or dx < 0 (q 3)
          if ((tx >= 0.0f) == (q == 2)) { a0 += ty; a1 += fabsf(ty); }
        }
      }
    if (!T.extended) {
      s_xy[lane] = a0;
    } else {
      s_xy[2 * lane] = a0; s_xy[2 * lane + 1] = a1;
    }
  }
  __syncthreads();
  if (inside && tid < dims) {
    double mag = 0.0;
    for (int kk = 0; kk < dims; ++kk) {
      const float f = s_xy[kk];
      mag += (double)(f * f);
    }
    const float scale = (float)(1.0 / (sqrt(mag) + (double)FLT_EPSILON));
    desc_tmp[(size_t)i * dims + tid] = s_xy[tid] * scale;
  }
  if (tid != 0) return;
  kpts_out[i] = k;
  extract_point(k, i, inside, right_x, status, cam, xyz_tmp, keep);
}

// the normalised n-tap Gaussian of cv::getGaussianKernel, kept in float64
void surf_gaussian(int n, double sigma, double* g) {
  double sum = 0.0;
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    g[i] = std::exp(-0.5 / (sigma * sigma) * x * x);
    sum += g[i];
  }
  for (int i = 0; i < n; ++i) g[i] /= sum;
}

int surf_layout(sf_context* c, int width, int height, const sf_surf_params& p, SurfLayout* L, size_t* floats) {
  L->w = width; L->h = height; L->n_octaves = p.n_octaves; L->n_layers = p.n_octave_layers;
  unsigned long long planes = 0, pos = 0;
  for (int o = 0; o < SURF_MAX_OCTAVES; ++o) {
    L->plane_off[o] = (unsigned)planes;
    L->pos_off[o] = (unsigned)pos;
    if (o >= p.n_octaves) continue;
    const unsigned long long plane = (unsigned long long)(height >> o) * (unsigned long long)(width >> o);
    planes += plane * (unsigned long long)(p.n_octave_layers + 2);
    pos += plane * (unsigned long long)p.n_octave_layers;
  }
  L->pos_off[SURF_MAX_OCTAVES] = (unsigned)pos;
  if (planes > 0x7FFFFFFFull)
    return sf_fail(c, SF_ERANGE, "SURF: %d octaves of %d layers on %d x %d pixels need %llu plane samples (at most 2^31)", p.n_octaves,
                   p.n_octave_layers + 2, width, height, planes);
  *floats = (size_t)planes;
  return SF_OK;
}

}  // namespace

extern "C" void sf_surf_defaults(sf_surf_params* p) {
  if (!p) return;
  p->hessian_threshold = 500.0f;   // SURF/HessianThreshold [upstream rtabmap Parameters.h]
  p->n_octaves = 4;                // SURF/Octaves
  p->n_octave_layers = 2;          // SURF/OctaveLayers
  p->upright = 0;                  // SURF/Upright
  p->extended = 0;                 // SURF/Extended
}

extern "C" void sf_surf_build_tables(float* ori_w, int8_t* ori_xy, float* desc_w) {
  double g13[13], g20[SURF_PATCH];
  surf_gaussian(13, 2.5, g13);
  surf_gaussian(SURF_PATCH, 3.3, g20);
  int n = 0;
  for (int i = -6; i <= 6; ++i)
    for (int j = -6; j <= 6; ++j) {
      if (i * i + j * j >= 36) continue;
      if (ori_xy) { ori_xy[2 * n] = (int8_t)i; ori_xy[2 * n + 1] = (int8_t)j; }
      if (ori_w) ori_w[n] = (float)(g13[i + 6] * g13[j + 6]);
      ++n;
    }
  if (desc_w)
    for (int i = 0; i < SURF_PATCH; ++i)
      for (int j = 0; j < SURF_PATCH; ++j) desc_w[i * SURF_PATCH + j] = (float)(g20[i] * g20[j]);
}

// The candidate capacity of one image: SURF_MAX_CANDIDATES, or what sf_debug_surf_limits has put in its place
unsigned sf_surf_candidate_cap(const sf_context* c) { return c->surf_debug_cap > 0 ? (unsigned)c->surf_debug_cap : SURF_MAX_CANDIDATES; }

// The host arithmetic of the detector's workspace (no device, c may be null).  B bounds the maxima an image of this layout
// can have: surf_keypoint demands v > q of all 26 neighbours, so two maxima of one layer are never 8-adjacent, and a layer
// whose interior (the samples k_surf_maxima looks at) is r x c holds at most ceil(r / 2) ceil(c / 2) of them.  An image's
// key capacity is the smaller of B and the candidate capacity: where B is the smaller (up to about a megapixel under the
// defaults) no image can overflow.  "More maxima than cap_img" is therefore the same refusal as "more than the candidate
// capacity", which is what a single call reports: no image has more than B.
int sf_surf_batch_plan_host(sf_context* c, int width, int height, const sf_surf_params& p, int n, unsigned candidate_cap,
                            int forced_chunk, SfSurfBatchPlan* out) {
  SurfLayout L;
  size_t floats = 0;
  const int rc = surf_layout(c, width, height, p, &L, &floats);
  if (rc != SF_OK) return rc;
  unsigned long long bound = 0;
  for (int o = 0; o < p.n_octaves; ++o)
    for (int l = 1; l <= p.n_octave_layers; ++l) {
      const int step = 1 << o, margin = (surf_size(o, l + 1) / 2) / step + 1;
      const long long r = std::max((height >> o) - 2 * margin, 0), q = std::max((width >> o) - 2 * margin, 0);
      bound += (unsigned long long)(((r + 1) / 2) * ((q + 1) / 2));
    }
  if (candidate_cap == 0) candidate_cap = SURF_MAX_CANDIDATES;
  out->bound = bound;
  out->cap_img = (unsigned)std::min<unsigned long long>(candidate_cap, bound);
  out->key_stride = std::max(out->cap_img, 1u);
  out->plane_floats = std::max<size_t>(floats, 1);
  // per image: det and trace planes, the keys and their sorted copy, count / segment bounds / flag
  out->per_image = out->plane_floats * 2 * sizeof(float) + (size_t)out->key_stride * 16 + 16;
  long long chunk = forced_chunk > 0 ? forced_chunk : (long long)(SURF_BATCH_WORKSPACE_BYTES / out->per_image);
  chunk = std::min<long long>(chunk, 0x7FFFFFFFll / out->key_stride);   // (the segmented sort counts its keys in 32 bits)
  chunk = std::min<long long>(chunk, 65535);                            // (the image is a grid dimension)
  out->chunk = (int)std::max<long long>(std::min<long long>(chunk, n), 1);
  out->workspace_bytes = (size_t)out->chunk * out->per_image;
  return SF_OK;
}

// The plan of a batch under the handle's limits and its buffers (a caller reserves before its first launch; the launcher
// below asks again and finds them there)
int sf_surf_batch_reserve(sf_context* c, int width, int height, const sf_surf_params& p, int n_img, SfSurfBatchPlan* plan) {
  int rc;
  if ((rc = sf_surf_batch_plan_host(c, width, height, p, n_img, sf_surf_candidate_cap(c), c->surf_debug_chunk, plan)) != SF_OK) return rc;
  const size_t ctl_words = ((size_t)n_img + 15) & ~(size_t)15;
  if ((rc = sf_buf_reserve(c, c->surf_planes, (size_t)plan->chunk * plan->plane_floats * 2 * sizeof(float))) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->surf_keys, (size_t)plan->chunk * plan->key_stride * 16)) != SF_OK) return rc;
  const bool fresh = !c->surf_ctl.p;
  if ((rc = sf_buf_reserve(c, c->surf_ctl, 64 + 4 * ctl_words * sizeof(unsigned))) != SF_OK) return rc;
  if (fresh) SF_HIP(c, hipMemsetAsync(c->surf_ctl.p, 0, 64, c->stream));     // (no batch call yet: none of its keyframes overflowed)
  return sf_buf_reserve(c, c->ex_integral, (size_t)(width + 1) * (height + 1) * sizeof(int32_t) * n_img);
}

// The fast-Hessian detector + limitKeypoints on n_img images of one size: d_kpts_out [n_img][cap], d_n_out [n_img] on the
// device.  The integral images of ALL images are built first and stay in c->ex_integral for the extraction; the rest runs
// over chunks of plan.chunk images -- consecutive launches on the handle's stream -- so that planes and keys keep to
// SURF_BATCH_WORKSPACE_BYTES.  An image with more maxima than its key capacity keeps no keypoint and is counted in the first
// word of c->surf_ctl (sf_surf_batch_status: the most recent BATCH call's); the per-image words follow from byte 64 on.
// `one` (the single-image entry point, n_img == 1): the count of maxima comes to the host with the wait of the image's
// sort, the entry point refuses an overflow itself, and the overflow is counted in the second word, which nobody reads --
// what the status call reports stays the batch call's.
int sf_launch_detect_surf(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                          int max_features, const sf_surf_params* prm, sf_keypoint* d_kpts_out, int cap, int32_t* d_n_out,
                          SfDetectOne* one) {
  SurfLayout L;
  size_t floats = 0;
  SfSurfBatchPlan plan;
  int rc;
  if ((rc = sf_check_limit(c, n_img, max_features)) != SF_OK) return rc;
  if ((rc = surf_layout(c, width, height, *prm, &L, &floats)) != SF_OK) return rc;
  if ((rc = sf_surf_batch_reserve(c, width, height, *prm, n_img, &plan)) != SF_OK) return rc;   // (a batch caller's: nothing moves)
  const size_t ctl_words = ((size_t)n_img + 15) & ~(size_t)15;
  float* planes = (float*)c->surf_planes.p;
  unsigned long long* keys = (unsigned long long*)c->surf_keys.p;
  unsigned long long* keys_sorted = keys + (size_t)plan.chunk * plan.key_stride;
  unsigned* overflowed = (unsigned*)c->surf_ctl.p + (one ? 1 : 0);
  unsigned* count = (unsigned*)c->surf_ctl.p + 16;
  unsigned *seg_begin = count + ctl_words, *seg_end = seg_begin + ctl_words, *flipped = seg_end + ctl_words;
  const int32_t* S = nullptr;
  size_t s_stride = 0;
  if ((rc = sf_launch_integral_batch(c, d_images, img_stride, n_img, width, height, pitch, &S, &s_stride)) != SF_OK) return rc;
  SF_HIP(c, hipMemsetAsync(overflowed, 0, (size_t)(count + ctl_words - overflowed) * sizeof(unsigned), c->stream));   // the call's counter and every count
  const unsigned blocks = (unsigned)(((size_t)width * height + 255) / 256);
  const int n_all = prm->n_octaves * (prm->n_octave_layers + 2), n_middle = prm->n_octaves * prm->n_octave_layers;
  const SurfBatch B = {s_stride, 2 * plan.plane_floats, plan.key_stride};
  float* det = planes;
  float* trace = planes + plan.plane_floats;
  for (int i0 = 0; i0 < n_img; i0 += plan.chunk) {
    const int m = std::min(plan.chunk, n_img - i0);
    hipLaunchKernelGGL(k_surf_hessian, dim3(blocks, n_all, m), dim3(256), 0, c->stream, S + (size_t)i0 * s_stride, L, det, trace, B);
    hipLaunchKernelGGL(k_surf_maxima, dim3(blocks, n_middle, m), dim3(256), 0, c->stream, L, (const float*)det, (const float*)trace,
                       prm->hessian_threshold, keys, count + i0, plan.cap_img, B);
    hipLaunchKernelGGL(k_surf_segments, dim3(SURF_SEGMENT_BLOCKS, m), dim3(256), 0, c->stream, keys, (const unsigned*)(count + i0),
                       plan.cap_img, plan.key_stride, max_features, seg_begin + i0, seg_end + i0, flipped + i0, overflowed);
    SF_HIP(c, hipGetLastError());
    SfSortBounds hb;
    if (one) hb.d_also[0] = count;                       // (the count of maxima arrives with the bounds)
    if ((rc = sf_sort_segments(c, keys, keys_sorted, (unsigned)((size_t)m * plan.key_stride), (unsigned)m, seg_begin + i0,
                               seg_end + i0, 0, 64, true, &hb)) != SF_OK)
      return rc;
    if (one) one->count[0] = hb.also[0];
    // the emit grid: sized by max_features, or -- a lone image, whose count the sort has brought to the host -- by its keypoints
    const int written = std::min(m == 1 ? sf_limit_keypoints(hb.n(), max_features) : max_features, cap);
    hipLaunchKernelGGL(k_surf_emit, dim3(std::max((written + 255) / 256, 1), m), dim3(256), 0, c->stream, L, (const float*)det,
                       (const float*)trace, prm->hessian_threshold, (const unsigned long long*)keys_sorted, (const unsigned*)(count + i0),
                       (const unsigned*)(flipped + i0), plan.cap_img, max_features, d_kpts_out + (size_t)i0 * cap, cap, d_n_out + i0, B);
    SF_HIP(c, hipGetLastError());
  }
  return SF_OK;
}

// k_surf_describe for sf_launch_extract_batch (k_extract.hip): S is the batch's integral images, B its layout
void sf_launch_surf_describe(sf_context* c, const uint8_t* d_left, int pitch, const int32_t* S, int width, int height,
                             const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status, int n, int n_img,
                             const SfSurfTables& T, const ExtractCam& cam, sf_keypoint* d_kpts_angle, float* desc_tmp,
                             float* xyz_tmp, uint8_t* keep, const ExtractBatch& B) {
  hipLaunchKernelGGL(k_surf_describe, dim3((unsigned)n, n_img), dim3(SURF_DESCRIBE_THREADS), 0, c->stream, d_left, pitch, S, width, height, d_kpts,
                     d_right_x, d_status, n, T, cam, d_kpts_angle, desc_tmp, xyz_tmp, keep, B);
}
