// k_sift.hip -- SIFT of the keyframe front end (Vis/FeatureType 1; sf_detect_sift_device, k_sift_describe under
// sf_extract_keyframe_device): cv::xfeatures2d::SIFT of OpenCV 3.2 as rtabmap drives it, float32 rows of 128 dimensions.  opencv_contrib is not in the reference tree; the algorithm is restated in DESIGN.md section 3 item 17i
// and in tests/sift_ref.py, which the tests compare with byte for byte.  Arithmetic: the float operations in the order
// written, no contraction (compiled with -ffp-contract=off); the planes are int16 fixed point of scale 48; the sigma and
// kernel tables are host arithmetic in double (sf_sift_build_tables); the Gaussian weights of orientation and descriptor go
// through sift_exp (double + - x and exponent arithmetic only); histogram votes are summed as integers, so no kernel
// has a summation order to keep.
//
//   k_sift_base       uint8 -> x 48 -> 2 x bilinear enlargement (weights 1/4, 3/4, clamped edges): 3 (wx wy v ...) with
//                     w in {1, 3} is an integer, nothing is rounded
//   k_sift_blur_rows  int16 -> float32, k_sift_blur_cols float32 -> int16 (cvRound, saturated): one thread per sample, the
//                     taps in index order, BORDER_REFLECT_101 reflected repeatedly (the top octaves are a few pixels wide);
//                     the kernel length is a launch argument, the coefficients sit in a device table
//   k_sift_half       every second pixel of Gaussian plane n -> plane 0 of the next octave
//   k_sift_dog        plane l + 1 - plane l, all n + 2 planes of an octave in one launch
//   k_sift_extrema    one thread per sample of DoG planes 1 .. n of all octaves (blockIdx.y = octave n + layer - 1):
//                     contrast floor, the 26-neighbour test, adjustLocalExtrema.  A survivor claims its CONVERGED sample in
//                     a bitmap (atomicOr): two candidates that converge to one sample give bit-identical keypoints, the
//                     first claim appends the sample to the list (wave-aggregated), the second does nothing -- whichever
//                     comes first, the list holds the same set
//   k_sift_orient     a wavefront per listed sample, SIFT_ORIENT_BLOCKS of them striding over an image's list: the
//                     refinement again (it converges at once: the sample is the one the loop ended on), the 36-bin
//                     histogram as 64-bit integers in LDS, smoothing, one sort key per peak: response bits << 32 |
//                     ~(sample << 6 | bin)
//   k_sift_segments   one thread per image of a chunk: overflow, the cut and its rekey flag, the image's sort segment, its
//                     row count
//   k_sift_rekey      a cut list: the position bits flipped (as k_surf_segments does), sf_sort_segments (sf_sort.hip), then
//   k_sift_emit       one wavefront per sorted key: refinement and histogram again, the lane of the key's bin writes the
//                     keypoint
//   k_sift_describe   (Vis/FeatureType 1) one workgroup of 256 per given keypoint: calcSIFTDescriptor on the Gaussian plane the
//                     keypoint's octave field names.  The window's samples are spread over the threads; a sample's 8
//                     trilinear votes (float32 as upstream) go as rint(vote 2^20) into 360 64-bit bins in LDS (ds_add_u64:
//                     integers, so no order to keep); the orientation wrap is folded in integers, a bin goes back to
//                     float32 once; then a thread per dimension adds the 128 float32 squares in index order in float64,
//                     clamps at 0.2 of the norm, adds again and scales to 0 .. 255.  Thread 0 does the 3D point
//                     (extract_point).  LDS: 2880 + 512 bytes.
// Every kernel takes the image of a chunk as its last grid dimension (SiftBatch) and reads that image's counts on the
// device; one launcher, sf_launch_detect_sift, runs a chunk, and sf_detect_sift_device runs it on a chunk of one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "sf_extract_device.hpp"
#include "sf_front_device.hpp"

namespace {

constexpr int SIFT_BORDER = 5, SIFT_STEPS = 5, SIFT_BINS = 36;
constexpr float SIFT_IMG_SCALE = 1.0f / (255 * 48);
constexpr double SIFT_VOTE_SCALE = 1048576.0;       // votes are summed as rint(vote 2^20) in 64-bit integers

// Every kernel below takes the image of the chunk as its last grid dimension and finds that image's data these strides
// behind image 0's.
struct SiftBatch {
  size_t img_stride;          // bytes between the uint8 images
  size_t plane_stride;        // int16 samples between the images' plane blocks (Gaussian | difference | row plane)
  size_t claim_stride;        // words between the claim bitmaps
  size_t key_stride;          // entries between the images' keys, sorted keys and extrema lists
};

__device__ __forceinline__ short sift_sat16(float v) {
  const float r = rintf(v);
  return (short)(r < -32768.0f ? -32768.0f : (r > 32767.0f ? 32767.0f : r));
}

// exp(x) from double + - x, rint and ldexp only (tests/sift_ref.py sift_exp64); the callers round to float once
__device__ __forceinline__ double sift_exp64(double x) {
  if (x < -700.0) return 0.0;
  const double k = rint(x * 1.4426950408889634);
  const double r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
  double p = 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 1.0 / 2.0;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return ldexp(p, (int)k);
}

__global__ void __launch_bounds__(256)
k_sift_base(const uint8_t* __restrict__ img, int pitch, int w, int h, short* __restrict__ out, SiftBatch B) {
  img += blockIdx.z * B.img_stride; out += blockIdx.z * B.plane_stride;
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  const int W = 2 * w, H = 2 * h;
  if (e >= (unsigned)W * (unsigned)H) return;
  const int y = (int)(e / (unsigned)W), x = (int)(e - (unsigned)y * (unsigned)W);
  const int kx = x >> 1, ky = y >> 1;
  const bool ex = !(x & 1), ey = !(y & 1);
  const int xa = min(max(ex ? kx - 1 : kx, 0), w - 1), xb = min(max(ex ? kx : kx + 1, 0), w - 1);
  const int ya = min(max(ey ? ky - 1 : ky, 0), h - 1), yb = min(max(ey ? ky : ky + 1, 0), h - 1);
  const int wxa = ex ? 1 : 3, wya = ey ? 1 : 3;
  const uint8_t* ra = img + (size_t)ya * pitch;
  const uint8_t* rb = img + (size_t)yb * pitch;
  const int top = ra[xa] * wxa + ra[xb] * (4 - wxa), bot = rb[xa] * wxa + rb[xb] * (4 - wxa);
  out[e] = (short)(3 * (top * wya + bot * (4 - wya)));
}

__global__ void __launch_bounds__(256)
k_sift_blur_rows(const short* __restrict__ in, float* __restrict__ tmp, int w, int h, const float* __restrict__ coef, int klen,
                 SiftBatch B) {
  in += blockIdx.z * B.plane_stride; tmp += blockIdx.z * (B.plane_stride / 2);   // (the stride counts int16 samples)
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= (unsigned)w * (unsigned)h) return;
  const int y = (int)(e / (unsigned)w), x = (int)(e - (unsigned)y * (unsigned)w);
  const int r = klen >> 1;
  const short* row = in + (size_t)y * w;
  float s;
  if (x - r >= 0 && x + r < w) {
    s = (float)row[x - r] * coef[0];
    for (int t = 1; t < klen; ++t) s += (float)row[x - r + t] * coef[t];
  } else {
    s = (float)row[reflect101(x - r, w)] * coef[0];
    for (int t = 1; t < klen; ++t) s += (float)row[reflect101(x - r + t, w)] * coef[t];
  }
  tmp[e] = s;
}

__global__ void __launch_bounds__(256)
k_sift_blur_cols(const float* __restrict__ tmp, short* __restrict__ out, int w, int h, const float* __restrict__ coef, int klen,
                 SiftBatch B) {
  tmp += blockIdx.z * (B.plane_stride / 2); out += blockIdx.z * B.plane_stride;
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= (unsigned)w * (unsigned)h) return;
  const int y = (int)(e / (unsigned)w), x = (int)(e - (unsigned)y * (unsigned)w);
  const int r = klen >> 1;
  float s;
  if (y - r >= 0 && y + r < h) {
    s = tmp[(size_t)(y - r) * w + x] * coef[0];
    for (int t = 1; t < klen; ++t) s += tmp[(size_t)(y - r + t) * w + x] * coef[t];
  } else {
    s = tmp[(size_t)reflect101(y - r, h) * w + x] * coef[0];
    for (int t = 1; t < klen; ++t) s += tmp[(size_t)reflect101(y - r + t, h) * w + x] * coef[t];
  }
  out[e] = sift_sat16(s);
}

__global__ void __launch_bounds__(256)
k_sift_half(const short* __restrict__ in, int w_in, short* __restrict__ out, int w, int h, SiftBatch B) {
  in += blockIdx.z * B.plane_stride; out += blockIdx.z * B.plane_stride;
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= (unsigned)w * (unsigned)h) return;
  const int y = (int)(e / (unsigned)w), x = (int)(e - (unsigned)y * (unsigned)w);
  out[e] = in[(size_t)(2 * y) * w_in + 2 * x];
}

// d [n_dog planes] = g [plane + 1] - g [plane]; total = n_dog x plane samples
__global__ void __launch_bounds__(256)
k_sift_dog(const short* __restrict__ g, short* __restrict__ d, unsigned plane, unsigned total, SiftBatch B) {
  g += blockIdx.z * B.plane_stride; d += blockIdx.z * B.plane_stride;
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  if (e >= total) return;
  const int v = (int)g[(size_t)e + plane] - (int)g[e];
  d[e] = (short)min(max(v, -32768), 32767);
}

struct SiftPrm {
  int n;                      // n_octave_layers
  int floor_thr;              // floor(0.5 contrast_threshold / n * 255 * 48)
  float contrast, edge, sigma;
};

// adjustLocalExtrema from sample (layer, r, c) of octave o: true when it converges and passes the contrast and edge tests;
// layer, r, c then hold the converged sample, xc / xr / xi the offsets, contr the contrast
__device__ __forceinline__ bool sift_refine(const SfSiftPlan& P, const short* __restrict__ dog, const SiftPrm& prm, int o, int& layer,
                                            int& r, int& c, float& xc, float& xr, float& xi, float& contr) {
  const int w = P.w[o], h = P.h[o];
  const size_t plane = (size_t)w * h;
  const short* D = dog + P.dog_off[o];
  const float deriv = SIFT_IMG_SCALE * 0.5f, second = SIFT_IMG_SCALE, cross = SIFT_IMG_SCALE * 0.25f;
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, dxx = 0.f, dyy = 0.f, dxy = 0.f;
  int centre = 0;
  bool converged = false;
  for (int step = 0; step < SIFT_STEPS; ++step) {
    const short* img = D + (size_t)layer * plane + (size_t)r * w + c;
    const short* prev = img - plane;
    const short* next = img + plane;
    centre = img[0];
    d0 = (float)((int)img[1] - (int)img[-1]) * deriv;
    d1 = (float)((int)img[w] - (int)img[-w]) * deriv;
    d2 = (float)((int)next[0] - (int)prev[0]) * deriv;
    const int v2 = 2 * centre;
    dxx = (float)((int)img[1] + (int)img[-1] - v2) * second;
    dyy = (float)((int)img[w] + (int)img[-w] - v2) * second;
    const float dss = (float)((int)next[0] + (int)prev[0] - v2) * second;
    dxy = (float)((int)img[w + 1] - (int)img[w - 1] - (int)img[-w + 1] + (int)img[-w - 1]) * cross;
    const float dxs = (float)((int)next[1] - (int)next[-1] - (int)prev[1] + (int)prev[-1]) * cross;
    const float dys = (float)((int)next[w] - (int)next[-w] - (int)prev[w] + (int)prev[-w]) * cross;
    // H x = dD by Cramer's rule in the order of tests/surf_ref.py solve3; the offsets are -x
    const float a00 = dxx, a01 = dxy, a02 = dxs, a10 = dxy, a11 = dyy, a12 = dys, a20 = dxs, a21 = dys, a22 = dss;
    const float m0 = a11 * a22 - a12 * a21, m1 = a10 * a22 - a12 * a20, m2 = a10 * a21 - a11 * a20;
    const float dt = (a00 * m0 - a01 * m1) + a02 * m2;
    const float d = 1.0f / dt;
    const float p = d1 * a22 - a12 * d2, q = d1 * a21 - a11 * d2, rr = a10 * d2 - d1 * a20;
    xc = -(d * ((d0 * m0 - a01 * p) + a02 * q));
    xr = -(d * ((a00 * p - d0 * m1) + a02 * rr));
    xi = -(d * ((d0 * m2 - a01 * rr) - a00 * q));
    if (fabsf(xc) < 0.5f && fabsf(xr) < 0.5f && fabsf(xi) < 0.5f) { converged = true; break; }
    const float big = (float)(2147483647 / 3);
    if (!(fabsf(xc) <= big && fabsf(xr) <= big && fabsf(xi) <= big)) return false;     // (NaN too)
    c += (int)rintf(xc); r += (int)rintf(xr); layer += (int)rintf(xi);
    if (layer < 1 || layer > prm.n || c < SIFT_BORDER || c >= w - SIFT_BORDER || r < SIFT_BORDER || r >= h - SIFT_BORDER) return false;
  }
  if (!converged) return false;
  const float t = ((d0 * xc) + (d1 * xr)) + (d2 * xi);
  contr = (float)centre * SIFT_IMG_SCALE + t * 0.5f;
  if (fabsf(contr) * (float)prm.n < prm.contrast) return false;
  const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
  const float e = prm.edge;
  if (det <= 0.0f || (tr * tr) * e >= ((e + 1.0f) * (e + 1.0f)) * det) return false;
  return true;
}

__global__ void __launch_bounds__(256)
k_sift_extrema(SfSiftPlan P, const short* __restrict__ dog, SiftPrm prm, unsigned* __restrict__ claimed, unsigned* __restrict__ list,
               unsigned* __restrict__ count, unsigned cap, SiftBatch B) {
  dog += blockIdx.z * B.plane_stride; claimed += blockIdx.z * B.claim_stride;
  list += blockIdx.z * B.key_stride; count += blockIdx.z;
  const int o = blockIdx.y / prm.n, l0 = 1 + (int)blockIdx.y - o * prm.n;
  const int w = P.w[o], h = P.h[o];
  const unsigned e = blockIdx.x * 256u + threadIdx.x;
  bool found = false;
  unsigned pos = 0;
  if (e < (unsigned)w * (unsigned)h) {                    // (uniform exit is not possible: the ballot below)
    const int r0 = (int)(e / (unsigned)w), c0 = (int)(e - (unsigned)r0 * (unsigned)w);
    if (r0 >= SIFT_BORDER && r0 < h - SIFT_BORDER && c0 >= SIFT_BORDER && c0 < w - SIFT_BORDER) {
      const size_t plane = (size_t)w * h;
      const short* ctr = dog + P.dog_off[o] + (size_t)l0 * plane + e;
      const int v = ctr[0];
      if (abs(v) > prm.floor_thr) {
        bool is_max = v > 0, is_min = v < 0;
#pragma unroll
        for (int k = -1; k <= 1; ++k)
#pragma unroll
          for (int di = -1; di <= 1; ++di)
#pragma unroll
            for (int dj = -1; dj <= 1; ++dj) {
              const int q = (ctr + (ptrdiff_t)k * (ptrdiff_t)plane)[di * w + dj];
              is_max = is_max && v >= q;
              is_min = is_min && v <= q;
            }
        if (is_max || is_min) {
          int layer = l0, r = r0, c = c0;
          float xc, xr, xi, contr;
          if (sift_refine(P, dog, prm, o, layer, r, c, xc, xr, xi, contr)) {
            pos = P.pos_off[o] + (unsigned)((size_t)layer * plane + (size_t)r * w + c);
            const unsigned bit = 1u << (pos & 31u);
            found = !(atomicOr(&claimed[pos >> 5], bit) & bit);
          }
        }
      }
    }
  }
  const unsigned long long bal = __ballot(found);
  if (bal == 0ull) return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)bal) - 1;
  unsigned base = 0u;
  if (lane == leader) base = atomicAdd(count, (unsigned)__popcll(bal));
  base = (unsigned)__shfl((int)base, leader);
  if (!found) return;
  const unsigned slot = base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
  if (slot < cap) list[slot] = pos;                      // (the counter has counted it: the image is refused, or marked as overflowed)
}

// One wavefront on the converged sample `pos`: the keypoint without its angle, and the smoothed histogram in hist[36]
// (LDS, this wavefront's).  raw: this wavefront's 36 64-bit bins.  False when the refinement does not hold (never, for a
// listed sample).
__device__ __forceinline__ bool sift_keypoint(const SfSiftPlan& P, const short* __restrict__ gauss, const short* __restrict__ dog,
                                              const SiftPrm& prm, unsigned pos, int lane, unsigned long long* raw, float* hist,
                                              sf_keypoint* out) {
  int o = 0;
  while (o + 1 < P.n_octaves && pos >= P.pos_off[o + 1]) ++o;
  const int w = P.w[o], h = P.h[o];
  const unsigned plane = (unsigned)w * (unsigned)h, rel = pos - P.pos_off[o];
  int layer = (int)(rel / plane);
  const unsigned in_plane = rel - (unsigned)layer * plane;
  int r = (int)(in_plane / (unsigned)w), c = (int)(in_plane - (unsigned)r * (unsigned)w);
  if (layer < 1 || layer > prm.n || c < SIFT_BORDER || c >= w - SIFT_BORDER || r < SIFT_BORDER || r >= h - SIFT_BORDER) return false;
  float xc, xr, xi, contr;
  const int l_in = layer, r_in = r, c_in = c;
  if (!sift_refine(P, dog, prm, o, layer, r, c, xc, xr, xi, contr)) return false;
  if (layer != l_in || r != r_in || c != c_in) return false;
  const float step = (float)(1 << o);
  const float x = ((float)c + xc) * step, y = ((float)r + xr) * step;
  const float t = ((float)layer + xi) / (float)prm.n;
  const float p2 = (float)sift_exp64((double)t * 0.6931471805599453);
  const float size = ((prm.sigma * p2) * step) * 2.0f;
  const int octave = o + (layer << 8) + ((int)rintf((xi + 0.5f) * 255.0f) << 16);
  out->x = x * 0.5f; out->y = y * 0.5f; out->size = size * 0.5f;
  out->angle = -1.0f;
  out->response = fabsf(contr);
  out->octave = (octave & ~255) | ((octave - 1) & 255);
  out->class_id = -1;
  // calcOrientationHist on the keypoint's own Gaussian plane
  const float scl = (size * 0.5f) / step;
  const int radius = (int)rintf(4.5f * scl);
  const float sigma = 1.5f * scl;
  const float escale = -1.0f / ((2.0f * sigma) * sigma);
  if (lane < SIFT_BINS) raw[lane] = 0ull;
  __syncthreads();
  const short* G = gauss + P.gauss_off[o] + (size_t)layer * plane;
  const int side = 2 * radius + 1, samples = side * side;
  for (int k = lane; k < samples; k += 64) {
    const int i = k / side - radius, j = k - (k / side) * side - radius;
    const int yy = r + i, xx = c + j;
    if (yy <= 0 || yy >= h - 1 || xx <= 0 || xx >= w - 1) continue;
    const short* g = G + (size_t)yy * w + xx;
    const float dx = (float)((int)g[1] - (int)g[-1]), dy = (float)((int)g[-w] - (int)g[w]);
    const float wt = (float)sift_exp64((double)((float)(i * i + j * j) * escale));
    const float mag = sqrtf(dx * dx + dy * dy);
    const float ang = sf_fast_atan2(dy, dx);
    int bin = (int)rintf((float)(SIFT_BINS / 360.0) * ang);
    if (bin >= SIFT_BINS) bin -= SIFT_BINS;
    if (bin < 0) bin += SIFT_BINS;
    const float vote = wt * mag;
    atomicAdd(&raw[bin], (unsigned long long)llrint((double)vote * SIFT_VOTE_SCALE));
  }
  __syncthreads();
  float tj = 0.0f;
  if (lane < SIFT_BINS) {
    tj = (float)((double)(long long)raw[lane] * (1.0 / SIFT_VOTE_SCALE));
    hist[lane + SIFT_BINS] = tj;                        // hist[36 .. 71]: the unsmoothed bins
  }
  __syncthreads();
  if (lane < SIFT_BINS) {
    const float* u = hist + SIFT_BINS;
    const int a2 = (lane + 34) % SIFT_BINS, a1 = (lane + 35) % SIFT_BINS, b1 = (lane + 1) % SIFT_BINS, b2 = (lane + 2) % SIFT_BINS;
    hist[lane] = ((u[a2] + u[b2]) * (1.0f / 16.0f) + (u[a1] + u[b1]) * (4.0f / 16.0f)) + u[lane] * (6.0f / 16.0f);
  }
  __syncthreads();
  return true;
}

// lane j < 36: whether bin j is a peak, and its angle
__device__ __forceinline__ bool sift_peak(const float* hist, int j, float* angle) {
  float omax = hist[0];
  for (int k = 1; k < SIFT_BINS; ++k) omax = fmaxf(omax, hist[k]);
  const float thr = omax * 0.8f;
  const float l = hist[(j + 35) % SIFT_BINS], r2 = hist[(j + 1) % SIFT_BINS], v = hist[j];
  if (!(v > l && v > r2 && v >= thr)) return false;
  float b = (float)j + (0.5f * (l - r2)) / ((l - 2.0f * v) + r2);
  b = b < 0.0f ? b + (float)SIFT_BINS : (b >= (float)SIFT_BINS ? b - (float)SIFT_BINS : b);
  float a = 360.0f - (float)(360.0 / SIFT_BINS) * b;
  if (fabsf(a - 360.0f) < FLT_EPSILON) a = 0.0f;
  *angle = a;
  return true;
}

// What is decided per image on the device (k_sift_extrema's counter, k_sift_segments), [images of the chunk] each
struct SiftCounts {
  const unsigned* n_list;     // k_sift_orient: the image's extrema (more than cap: none of them is read)
  const unsigned* n_keys;     // k_sift_rekey: the image's keys, and
  const unsigned* flipped;    // ... whether the cut at the limit rekeys them (k_sift_emit: how to read a key)
  const int32_t* total;       // k_sift_emit: the image's keypoints behind the cut
};

// blocks of ONE wavefront: the __syncthreads() of sift_keypoint are this wavefront's own.  The wavefront takes the listed
// samples blockIdx.x, + gridDim.x, ... of its image's list, whose length it reads on the device
__global__ void __launch_bounds__(64)
k_sift_orient(SfSiftPlan P, const short* __restrict__ gauss, const short* __restrict__ dog, SiftPrm prm,
              const unsigned* __restrict__ list, unsigned long long* __restrict__ keys, unsigned* __restrict__ count, unsigned cap,
              SiftCounts C, SiftBatch B) {
  __shared__ unsigned long long raw[SIFT_BINS];
  __shared__ float hist[2 * SIFT_BINS];
  const unsigned n_list = C.n_list[blockIdx.z];
  if (n_list > cap) return;                            // (an overflowed image: its list is not whole)
  gauss += blockIdx.z * B.plane_stride; dog += blockIdx.z * B.plane_stride;
  list += blockIdx.z * B.key_stride; keys += blockIdx.z * B.key_stride; count += blockIdx.z;
  const int lane = threadIdx.x;
  for (unsigned item = blockIdx.x; item < n_list; item += gridDim.x) {
    const unsigned pos = list[item];
    sf_keypoint k;
    // (every lane holds the same sample: the conditions around the barriers are the same in every lane)
    if (sift_keypoint(P, gauss, dog, prm, pos, lane, raw, hist, &k)) {
      float angle = 0.0f;
      const bool peak = lane < SIFT_BINS && sift_peak(hist, lane, &angle);
      const unsigned long long bal = __ballot(peak);
      if (bal != 0ull) {
        const int leader = __ffsll((long long)bal) - 1;
        unsigned base = 0u;
        if (lane == leader) base = atomicAdd(count, (unsigned)__popcll(bal));
        base = (unsigned)__shfl((int)base, leader);
        const unsigned slot = base + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (peak && slot < cap)
          keys[slot] = ((unsigned long long)__float_as_uint(k.response) << 32) |
                       (unsigned long long)(0xFFFFFFFFu - ((pos << 6) | (unsigned)lane));
      }
    }
    __syncthreads();                                   // the next sample's histogram goes where this one's was read
  }
}

// (key, image) grid: a thread takes the keys blockIdx.x 256 + threadIdx.x, + gridDim.x 256, ... of its image
__global__ void __launch_bounds__(256)
k_sift_rekey(unsigned long long* __restrict__ keys, SiftCounts C, SiftBatch B) {
  if (!C.flipped[blockIdx.z]) return;
  const unsigned n = C.n_keys[blockIdx.z];
  keys += blockIdx.z * B.key_stride;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) keys[i] ^= 0xFFFFFFFFull;
}

// One thread per image of the chunk: the decisions about the image's list.  n_ext / n_kp: the counters of
// k_sift_extrema and k_sift_orient.  An image with more extrema or more keypoints than cap_img (as many is not more) is
// never truncated: it gets an empty segment and no keypoint, and the call's counter counts it.  Otherwise the image's
// keys are its segment of the segmented sort (bounds counted from the chunk's first key), and they are cut once, at the
// smaller positive of n_features and max_features; a cut list is rekeyed first (k_sift_rekey: equal responses by
// descending position).  total: the keypoints k_sift_emit writes, at most cap_rows.
__global__ void __launch_bounds__(256)
k_sift_segments(const unsigned* __restrict__ n_ext, unsigned* __restrict__ n_kp, int n_img, unsigned cap_img, size_t key_stride,
                int n_features, int max_features, int cap_rows, unsigned* __restrict__ seg_begin, unsigned* __restrict__ seg_end,
                unsigned* __restrict__ flipped, int32_t* __restrict__ total, unsigned* __restrict__ overflowed) {
  const int img = blockIdx.x * 256 + threadIdx.x;
  if (img >= n_img) return;
  const bool over = n_ext[img] > cap_img || n_kp[img] > cap_img;
  const unsigned n = over ? 0u : n_kp[img];
  const int limit = sf_sift_limit(n_features, max_features);
  const bool cut = limit > 0 && n > (unsigned)limit;
  const unsigned begin = (unsigned)(img * key_stride);
  seg_begin[img] = begin;
  seg_end[img] = begin + n;
  flipped[img] = cut ? 1u : 0u;                        // (k_sift_rekey reads n_kp under this flag alone: never an overflowed image's)
  total[img] = min((int)(cut ? (unsigned)limit : n), cap_rows);
  if (over) atomicAdd(overflowed, 1u);
}

// (keypoint, image) grid of one-wavefront blocks
__global__ void __launch_bounds__(64)
k_sift_emit(SfSiftPlan P, const short* __restrict__ gauss, const short* __restrict__ dog, SiftPrm prm,
            const unsigned long long* __restrict__ keys, sf_keypoint* __restrict__ kp_out, int kp_stride, SiftCounts C, SiftBatch B) {
  __shared__ unsigned long long raw[SIFT_BINS];
  __shared__ float hist[2 * SIFT_BINS];
  const int total = C.total[blockIdx.z], flipped = (int)C.flipped[blockIdx.z];
  const int item = blockIdx.x;
  if (item >= total) return;
  gauss += blockIdx.z * B.plane_stride; dog += blockIdx.z * B.plane_stride;
  keys += blockIdx.z * B.key_stride; kp_out += (size_t)blockIdx.z * kp_stride;
  const int lane = threadIdx.x;
  const unsigned low = (unsigned)keys[item];
  const unsigned posbin = flipped ? low : 0xFFFFFFFFu - low;
  const unsigned pos = posbin >> 6;
  const int bin = (int)(posbin & 63u);
  sf_keypoint k;
  const bool ok = sift_keypoint(P, gauss, dog, prm, pos, lane, raw, hist, &k);
  if (lane != bin) return;
  float angle = 0.0f;
  if (ok && bin < SIFT_BINS && sift_peak(hist, bin, &angle)) k.angle = angle;
  else k = sf_make_keypoint(0.0f, 0.0f, 0.0f, 0.0f, 0);
  kp_out[item] = k;
}

constexpr int SIFT_D = 4, SIFT_N = 8, SIFT_HIST = (SIFT_D + 2) * (SIFT_D + 2) * (SIFT_N + 2), SIFT_DIMS = SIFT_D * SIFT_D * SIFT_N;
constexpr float SIFT_MAX_SIZE = 1.0e6f;             // keypoint sizes and coordinates beyond it are dropped

__device__ __forceinline__ void sift_vote(unsigned long long* bins, int idx, float v) {
  atomicAdd(&bins[idx], (unsigned long long)llrint((double)v * SIFT_VOTE_SCALE));
}

__global__ void __launch_bounds__(256)
k_sift_describe(SfSiftPlan P, const short* __restrict__ gauss, const sf_keypoint* __restrict__ kpts, const float* __restrict__ right_x,
                const uint8_t* __restrict__ status, int n, ExtractCam cam, sf_keypoint* __restrict__ kpts_out,
                float* __restrict__ desc_tmp, float* __restrict__ xyz_tmp, uint8_t* __restrict__ keep, ExtractBatch B,
                size_t plane_stride, int rows_u8) {
  // rows_u8: desc_tmp holds rows of SIFT_DIMS uint8 (a handle with desc_type 2), not of SIFT_DIMS float32
  __shared__ unsigned long long s_bins[SIFT_HIST];
  __shared__ float s_row[SIFT_DIMS];
  const int tid = threadIdx.x, i = blockIdx.x;
  if (B.d_n) n = min(n, B.d_n[blockIdx.y]);
  if (i >= n) return;                                // (the whole workgroup)
  {                                                  // blockIdx.y = image: its pyramid plane_stride samples behind the first's
    const size_t o = (size_t)blockIdx.y * B.per_image;
    gauss += blockIdx.y * plane_stride;
    kpts += o; kpts_out += o;
    if (right_x) right_x += o;
    if (status) status += o;
    desc_tmp += rows_u8 ? o * (SIFT_DIMS / 4) : o * SIFT_DIMS; xyz_tmp += 3 * o; keep += o;
  }
  const sf_keypoint k = kpts[i];
  // (every thread holds the same keypoint: the conditions around the barriers below are the same in every thread)
  int o = k.octave & 255;
  const int layer = (k.octave >> 8) & 255;
  o = o < 128 ? o : o - 256;
  const bool inside = o >= -1 && o + 1 < P.n_octaves && layer <= P.n_layers + 2 && k.size > 0.0f && k.size < SIFT_MAX_SIZE &&
                      fabsf(k.x) < SIFT_MAX_SIZE && fabsf(k.y) < SIFT_MAX_SIZE && k.angle >= 0.0f && k.angle <= 360.0f;
  for (int b = tid; b < SIFT_HIST; b += 256) s_bins[b] = 0ull;
  __syncthreads();
  if (inside) {
    const float scale = o >= 0 ? 1.0f / (float)(1 << o) : (float)(1 << -o);
    const int w = P.w[o + 1], h = P.h[o + 1];
    const short* G = gauss + P.gauss_off[o + 1] + (size_t)layer * ((size_t)w * h);
    const int px = (int)rintf(k.x * scale), py = (int)rintf(k.y * scale);
    float ori = 360.0f - k.angle;
    if (fabsf(ori - 360.0f) < FLT_EPSILON) ori = 0.0f;
    const float scl = (k.size * scale) * 0.5f;
    const float rad = ori * (float)(3.14159265358979323846 / 180.0);
    float cos_t = (float)cos((double)rad), sin_t = (float)sin((double)rad);
    const float bins_per_deg = (float)SIFT_N / 360.0f;
    const float hist_width = 3.0f * scl;
    int radius = (int)rintf(((hist_width * 1.4142135623730951f) * (float)(SIFT_D + 1)) * 0.5f);
    radius = min(radius, (int)sqrt((double)w * w + (double)h * h));
    cos_t /= hist_width; sin_t /= hist_width;
    const long long side = 2ll * radius + 1, samples = side * side;
    for (long long s = tid; s < samples; s += 256) {
      const int si = (int)(s / side);
      const int ii = si - radius, jj = (int)(s - (long long)si * side) - radius;
      const float c_rot = (float)jj * cos_t - (float)ii * sin_t, r_rot = (float)jj * sin_t + (float)ii * cos_t;
      float rbin = (r_rot + (float)(SIFT_D / 2)) - 0.5f, cbin = (c_rot + (float)(SIFT_D / 2)) - 0.5f;
      const int r = py + ii, c = px + jj;
      if (!(rbin > -1.0f && rbin < (float)SIFT_D && cbin > -1.0f && cbin < (float)SIFT_D && r > 0 && r < h - 1 && c > 0 && c < w - 1)) continue;
      const short* g = G + (size_t)r * w + c;
      const float dx = (float)((int)g[1] - (int)g[-1]), dy = (float)((int)g[-w] - (int)g[w]);
      const float wt = (float)sift_exp64((double)((c_rot * c_rot + r_rot * r_rot) * -0.125f));
      const float mag = sqrtf(dx * dx + dy * dy) * wt;
      float obin = (sf_fast_atan2(dy, dx) - ori) * bins_per_deg;
      const float fr = floorf(rbin), fc = floorf(cbin), fo = floorf(obin);
      rbin -= fr; cbin -= fc; obin -= fo;
      const int r0 = (int)fr, c0 = (int)fc;
      int o0 = (int)fo;
      if (o0 < 0) o0 += SIFT_N;
      if (o0 >= SIFT_N) o0 -= SIFT_N;
      if (o0 < 0 || o0 >= SIFT_N) continue;           // (not reached: both angles lie in [0, 360])
      const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
      const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11;
      const float v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
      const float v111 = v_rc11 * obin, v110 = v_rc11 - v111;
      const float v101 = v_rc10 * obin, v100 = v_rc10 - v101;
      const float v011 = v_rc01 * obin, v010 = v_rc01 - v011;
      const float v001 = v_rc00 * obin, v000 = v_rc00 - v001;
      const int idx = ((r0 + 1) * (SIFT_D + 2) + c0 + 1) * (SIFT_N + 2) + o0;
      constexpr int ROW = (SIFT_D + 2) * (SIFT_N + 2), COL = SIFT_N + 2;
      sift_vote(s_bins, idx, v000); sift_vote(s_bins, idx + 1, v001);
      sift_vote(s_bins, idx + COL, v010); sift_vote(s_bins, idx + COL + 1, v011);
      sift_vote(s_bins, idx + ROW, v100); sift_vote(s_bins, idx + ROW + 1, v101);
      sift_vote(s_bins, idx + ROW + COL, v110); sift_vote(s_bins, idx + ROW + COL + 1, v111);
    }
  }
  __syncthreads();
  float own = 0.0f;
  if (tid < SIFT_DIMS) {
    const int cell = tid >> 3, kk = tid & 7, ci = cell >> 2, cj = cell & 3;
    const int idx = ((ci + 1) * (SIFT_D + 2) + cj + 1) * (SIFT_N + 2) + kk;
    long long v = (long long)s_bins[idx];
    if (kk < 2) v += (long long)s_bins[idx + SIFT_N];
    own = (float)((double)v * (1.0 / SIFT_VOTE_SCALE));
    s_row[tid] = own;
  }
  __syncthreads();
  float val = 0.0f;
  if (tid < SIFT_DIMS) {
    double nrm2 = 0.0;
    for (int q = 0; q < SIFT_DIMS; ++q) {
      const float f = s_row[q];
      nrm2 += (double)(f * f);
    }
    const float thr = (float)sqrt(nrm2) * 0.2f;
    val = fminf(own, thr);
  }
  __syncthreads();
  if (tid < SIFT_DIMS) s_row[tid] = val;
  __syncthreads();
  if (inside && tid < SIFT_DIMS) {
    double nrm2 = 0.0;
    for (int q = 0; q < SIFT_DIMS; ++q) {
      const float f = s_row[q];
      nrm2 += (double)(f * f);
    }
    const float scale = 512.0f / fmaxf((float)sqrt(nrm2), FLT_EPSILON);
    const float r = rintf(val * scale);
    const float clamped = r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r);
    if (rows_u8) reinterpret_cast<uint8_t*>(desc_tmp)[(size_t)i * SIFT_DIMS + tid] = (uint8_t)(int)clamped;   // (an integer in 0 .. 255: exact)
    else desc_tmp[(size_t)i * SIFT_DIMS + tid] = clamped;
  }
  if (tid != 0) return;
  kpts_out[i] = k;
  extract_point(k, i, inside, right_x, status, cam, xyz_tmp, keep);
}

void sift_gaussian_kernel(double sigma, int* klen, float* coef) {
  const int n = (int)std::nearbyint(sigma * 8.0 + 1.0) | 1;
  *klen = n;
  if (!coef) return;
  const double scale = -0.5 / (sigma * sigma);
  double sum = 0.0;
  double t[SIFT_MAX_KLEN];
  for (int i = 0; i < n; ++i) {
    const double x = i - (n - 1) * 0.5;
    t[i] = std::exp(scale * x * x);
    sum += t[i];
  }
  for (int i = 0; i < n; ++i) coef[i] = (float)(t[i] / sum);
}

void sift_sigmas(const sf_sift_params& p, double* sig) {
  const int n = p.n_octave_layers;
  const double sigma = (double)p.sigma;
  sig[0] = std::sqrt(std::max(sigma * sigma - 1.0, 0.01));
  const double k = std::pow(2.0, 1.0 / n);
  for (int i = 1; i < n + 3; ++i) {
    const double prev = std::pow(k, (double)(i - 1)) * sigma, total = prev * k;
    sig[i] = std::sqrt(total * total - prev * prev);
  }
}

unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

SiftPrm sift_kernel_params(const sf_sift_params& p) {
  SiftPrm K;
  K.n = p.n_octave_layers;
  K.floor_thr = (int)std::floor(0.5 * (double)p.contrast_threshold / p.n_octave_layers * 255 * 48);
  K.contrast = p.contrast_threshold; K.edge = p.edge_threshold; K.sigma = p.sigma;
  return K;
}

// k_sift_orient in the batch form: this many one-wavefront blocks per image share the image's extrema (a few thousand on a
// camera image), whose number stays on the device
constexpr unsigned SIFT_ORIENT_BLOCKS = 1024;

}  // namespace

extern "C" void sf_sift_defaults(sf_sift_params* p) {
  if (!p) return;
  p->n_features = 0;               // SIFT/NFeatures [upstream rtabmap Parameters.h]
  p->n_octave_layers = 3;          // SIFT/NOctaveLayers
  p->contrast_threshold = 0.04f;   // SIFT/ContrastThreshold
  p->edge_threshold = 10.0f;       // SIFT/EdgeThreshold
  p->sigma = 1.6f;                 // SIFT/Sigma
}

int sf_sift_validate(sf_context* c, const sf_sift_params& p) {
  if (p.n_features < 0) return sf_fail(c, SF_EINVAL, "SIFT n_features %d: >= 0", p.n_features);
  if (p.n_octave_layers < 1 || p.n_octave_layers > SIFT_MAX_LAYERS)
    return sf_fail(c, SF_EINVAL, "SIFT n_octave_layers %d outside 1 .. %d", p.n_octave_layers, SIFT_MAX_LAYERS);
  if (!std::isfinite(p.contrast_threshold) || !(p.contrast_threshold >= 0.0f))
    return sf_fail(c, SF_EINVAL, "SIFT contrast_threshold %g: finite and >= 0", (double)p.contrast_threshold);
  if (!std::isfinite(p.edge_threshold) || !(p.edge_threshold > 0.0f))
    return sf_fail(c, SF_EINVAL, "SIFT edge_threshold %g: finite and > 0", (double)p.edge_threshold);
  if (!std::isfinite(p.sigma) || !(p.sigma >= 0.8f && p.sigma <= 8.0f))
    return sf_fail(c, SF_EINVAL, "SIFT sigma %g outside 0.8 .. 8", (double)p.sigma);
  return SF_OK;
}

extern "C" int sf_sift_build_tables(const sf_sift_params* params, double* sigmas, int32_t* lengths, float* coef) {
  sf_sift_params p;
  if (params) p = *params; else sf_sift_defaults(&p);
  const int rc = sf_sift_validate(nullptr, p);
  if (rc != SF_OK) return rc;
  double sig[SIFT_MAX_LAYERS + 3];
  sift_sigmas(p, sig);
  for (int i = 0; i < p.n_octave_layers + 3; ++i) {
    int klen = 0;
    if (coef) std::fill(coef + (size_t)i * SIFT_MAX_KLEN, coef + (size_t)(i + 1) * SIFT_MAX_KLEN, 0.0f);
    sift_gaussian_kernel(sig[i], &klen, coef ? coef + (size_t)i * SIFT_MAX_KLEN : nullptr);
    if (sigmas) sigmas[i] = sig[i];
    if (lengths) lengths[i] = klen;
  }
  return SF_OK;
}

// The pyramid of a width x height image (host arithmetic; c may be null)
int sf_sift_plan_host(sf_context* c, int width, int height, const sf_sift_params& p, SfSiftPlan* P) {
  if (width < 3 || height < 3 || width > 16384 || height > 16384)
    return sf_fail(c, width < 3 || height < 3 ? SF_EINVAL : SF_ERANGE, "SIFT: image %d x %d outside 3 .. 16384 a side", width, height);
  *P = SfSiftPlan();
  int w = 2 * width, h = 2 * height;
  const int n_oct = (int)std::nearbyint(std::log((double)std::min(w, h)) / std::log(2.0) - 2.0) + 1;
  if (n_oct < 1 || n_oct > SIFT_MAX_OCTAVES) return sf_fail(c, SF_ERANGE, "SIFT: %d octaves", n_oct);
  P->n_octaves = n_oct;
  P->n_layers = p.n_octave_layers;
  unsigned long long g = 0, d = 0;
  for (int o = 0; o < n_oct; ++o) {
    P->w[o] = w; P->h[o] = h;
    P->gauss_off[o] = g; P->dog_off[o] = d;
    P->pos_off[o] = (unsigned)d;
    const unsigned long long plane = (unsigned long long)w * h;
    g += plane * (p.n_octave_layers + 3);
    d += plane * (p.n_octave_layers + 2);
    w /= 2; h /= 2;
  }
  for (int o = n_oct; o <= SIFT_MAX_OCTAVES; ++o) P->pos_off[o] = (unsigned)d;
  P->gauss_samples = g; P->dog_samples = d;
  if (d >= (1ull << 26))
    return sf_fail(c, SF_ERANGE, "SIFT: %llu difference-of-Gaussian samples on %d x %d pixels (the sort key holds 2^26)", d, width, height);
  return SF_OK;
}

extern "C" int sf_sift_plan(int32_t width, int32_t height, const sf_sift_params* params, int32_t* n_octaves_out, int32_t* widths,
                            int32_t* heights, int64_t* gauss_samples_out, int64_t* dog_samples_out) {
  sf_sift_params p;
  if (params) p = *params; else sf_sift_defaults(&p);
  int rc = sf_sift_validate(nullptr, p);
  if (rc != SF_OK) return rc;
  SfSiftPlan P;
  if ((rc = sf_sift_plan_host(nullptr, width, height, p, &P)) != SF_OK) return rc;
  if (n_octaves_out) *n_octaves_out = P.n_octaves;
  for (int o = 0; o < SIFT_MAX_OCTAVES; ++o) {
    if (widths) widths[o] = P.w[o];
    if (heights) heights[o] = P.h[o];
  }
  if (gauss_samples_out) *gauss_samples_out = (int64_t)P.gauss_samples;
  if (dog_samples_out) *dog_samples_out = (int64_t)P.dog_samples;
  return SF_OK;
}

// The host arithmetic of the batch form (no device, c may be null): the layout of one image's planes, claim bits, keys and
// counters, and how many images fit SIFT_BATCH_WORKSPACE_BYTES.  An image's capacity is the candidate capacity: k_sift_extrema
// takes >= plateaus, so no adjacency argument bounds the extrema of an image below its samples.
int sf_sift_batch_plan_host(sf_context* c, int width, int height, const sf_sift_params& p, int n, unsigned candidate_cap,
                            int forced_chunk, SfSiftBatchPlan* out) {
  const int rc = sf_sift_plan_host(c, width, height, p, &out->P);
  if (rc != SF_OK) return rc;
  const SfSiftPlan& P = out->P;
  const auto a256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
  out->off_dog = a256((size_t)P.gauss_samples * 2);
  out->off_tmp = a256(out->off_dog + (size_t)P.dog_samples * 2);
  out->plane_bytes = a256(out->off_tmp + (size_t)P.w[0] * P.h[0] * 4);
  out->claim_words = a256((size_t)((P.dog_samples + 31) / 32) * 4) / 4;
  out->cap_img = candidate_cap == 0 ? SIFT_MAX_CANDIDATES : std::min(candidate_cap, SIFT_MAX_CANDIDATES);
  // per image: the planes, the claim bits, key + sorted key + list entry per candidate, 32 bytes of counters and bounds
  out->per_image = out->plane_bytes + out->claim_words * 4 + (size_t)out->cap_img * 20 + 32;
  long long chunk = forced_chunk > 0 ? forced_chunk : (long long)(SIFT_BATCH_WORKSPACE_BYTES / out->per_image);
  chunk = std::min<long long>(chunk, 0x7FFFFFFFll / out->cap_img);      // (the segmented sort counts its keys in 32 bits)
  chunk = std::min<long long>(chunk, 65535);                            // (the image is a grid dimension)
  out->chunk = (int)std::max<long long>(std::min<long long>(chunk, n), 1);
  out->workspace_bytes = (size_t)out->chunk * out->per_image;
  return SF_OK;
}

// the kernel tables of a parameter set (host arithmetic) on the device; uploaded, with a wait, when n_octave_layers or
// sigma differ from the tables there
static int sift_upload_tables(sf_context* c, const sf_sift_params* prm) {
  int rc;
  if ((rc = sf_buf_reserve(c, c->sift_tables, (size_t)(SIFT_MAX_LAYERS + 3) * SIFT_MAX_KLEN * 4)) != SF_OK) return rc;
  if (c->sift_tables_ok && c->sift_tables_n == prm->n_octave_layers && c->sift_tables_sigma == prm->sigma) return SF_OK;
  c->sift_tables_ok = false;
  c->sift_coef_host.assign((size_t)(SIFT_MAX_LAYERS + 3) * SIFT_MAX_KLEN, 0.0f);
  if ((rc = sf_sift_build_tables(prm, nullptr, c->sift_klen, c->sift_coef_host.data())) != SF_OK) return rc;
  SF_HIP(c, hipMemcpyAsync(c->sift_tables.p, c->sift_coef_host.data(), c->sift_coef_host.size() * 4, hipMemcpyHostToDevice, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));
  c->sift_tables_ok = true; c->sift_tables_n = prm->n_octave_layers; c->sift_tables_sigma = prm->sigma;
  return SF_OK;
}

// The Gaussian and difference pyramids of m images (B.img_stride apart) into c->sift_planes, laid out by bp, and their
// claim bitmaps cleared: one launch per plane and pass for all m images (blockIdx.z).  The tables on the handle are the
// parameters' (sift_upload_tables).
static int sift_launch_pyramids(sf_context* c, const SfSiftBatchPlan& bp, int n, const uint8_t* d_images, int width, int height,
                                int pitch, int m, const SiftBatch& B) {
  const SfSiftPlan& P = bp.P;
  short* gauss = (short*)c->sift_planes.p;
  short* dog = (short*)((uint8_t*)c->sift_planes.p + bp.off_dog);
  float* tmp = (float*)((uint8_t*)c->sift_planes.p + bp.off_tmp);
  unsigned* claimed = (unsigned*)((uint8_t*)c->sift_planes.p + (size_t)bp.chunk * bp.plane_bytes);   // behind the chunk's planes
  const float* coef = (const float*)c->sift_tables.p;
  const unsigned z = (unsigned)m;
  SF_HIP(c, hipMemsetAsync(claimed, 0, (size_t)m * bp.claim_words * 4, c->stream));
  hipLaunchKernelGGL(k_sift_base, dim3(blocks_of((size_t)P.w[0] * P.h[0]), 1, z), dim3(256), 0, c->stream, d_images, pitch, width, height,
                     gauss, B);
  for (int o = 0; o < P.n_octaves; ++o) {
    const int w = P.w[o], h = P.h[o];
    const size_t plane = (size_t)w * h;
    short* g = gauss + P.gauss_off[o];
    const unsigned nb = blocks_of(plane);
    if (o > 0)
      hipLaunchKernelGGL(k_sift_half, dim3(nb, 1, z), dim3(256), 0, c->stream,
                         (const short*)(gauss + P.gauss_off[o - 1] + (size_t)n * P.w[o - 1] * P.h[o - 1]), P.w[o - 1], g, w, h, B);
    for (int i = (o == 0 ? 0 : 1); i < n + 3; ++i) {      // octave 0, i = 0: the enlarged image blurred in place
      const short* src = i == 0 ? g : g + (size_t)(i - 1) * plane;
      hipLaunchKernelGGL(k_sift_blur_rows, dim3(nb, 1, z), dim3(256), 0, c->stream, src, tmp, w, h, coef + (size_t)i * SIFT_MAX_KLEN,
                         c->sift_klen[i], B);
      hipLaunchKernelGGL(k_sift_blur_cols, dim3(nb, 1, z), dim3(256), 0, c->stream, (const float*)tmp, g + (size_t)i * plane, w, h,
                         coef + (size_t)i * SIFT_MAX_KLEN, c->sift_klen[i], B);
    }
    hipLaunchKernelGGL(k_sift_dog, dim3(blocks_of(plane * (n + 2)), 1, z), dim3(256), 0, c->stream, (const short*)g, dog + P.dog_off[o],
                       (unsigned)plane, (unsigned)(plane * (n + 2)), B);
  }
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

// c->sift_last: the pyramid of ONE image that a chunk of one, planned by bp, has left in c->sift_planes
static void sift_remember_pyramid(sf_context* c, const SfSiftBatchPlan& bp, const sf_sift_params* prm, int width, int height) {
  c->sift_last = bp.P; c->sift_last_off_dog = bp.off_dog; c->sift_last_off_claim = bp.plane_bytes; c->sift_last_ok = true;
  c->sift_last_prm = *prm; c->sift_last_width = width; c->sift_last_height = height;
}

// The Gaussian and difference pyramids of an image into c->sift_planes, on the handle's stream; c->sift_last describes them
int sf_sift_build_pyramid(sf_context* c, const uint8_t* d_image, int width, int height, int pitch, const sf_sift_params* prm) {
  SfSiftBatchPlan bp;
  int rc;
  c->sift_last_ok = false;
  if ((rc = sf_sift_batch_plan_host(c, width, height, *prm, 1, 0, 1, &bp)) != SF_OK) return rc;   // a chunk of one
  // sift_planes: Gaussian planes | DoG planes (int16) | the row pass's float32 plane | the claim bitmap
  if ((rc = sf_buf_reserve(c, c->sift_planes, bp.plane_bytes + bp.claim_words * 4)) != SF_OK) return rc;
  if ((rc = sift_upload_tables(c, prm)) != SF_OK) return rc;
  const SiftBatch one = {0, 0, 0, 0};
  if ((rc = sift_launch_pyramids(c, bp, prm->n_octave_layers, d_image, width, height, pitch, 1, one)) != SF_OK) return rc;
  sift_remember_pyramid(c, bp, prm, width, height);
  return SF_OK;
}

// The plan of n_img images under the handle's limits, its buffers and the blur tables
int sf_sift_batch_reserve(sf_context* c, int width, int height, const sf_sift_params& p, int n_img) {
  SfSiftBatchPlan& bp = c->sift_batch;
  int rc;
  if ((rc = sf_sift_batch_plan_host(c, width, height, p, n_img, (unsigned)c->sift_debug_cap, c->sift_debug_chunk, &bp)) != SF_OK) return rc;
  const size_t ctl_words = ((size_t)bp.chunk + 15) & ~(size_t)15;
  if ((rc = sf_buf_reserve(c, c->sift_planes, (size_t)bp.chunk * (bp.plane_bytes + bp.claim_words * 4))) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->sift_keys, (size_t)bp.chunk * bp.cap_img * 20)) != SF_OK) return rc;
  const bool fresh = !c->sift_ctl.p;
  if ((rc = sf_buf_reserve(c, c->sift_ctl, 64 + 5 * ctl_words * sizeof(unsigned))) != SF_OK) return rc;
  if (fresh) SF_HIP(c, hipMemsetAsync(c->sift_ctl.p, 0, 64, c->stream));      // (no batch call yet: none of its keyframes overflowed)
  return sift_upload_tables(c, &p);
}

int sf_sift_batch_begin(sf_context* c) {
  c->sift_last_ok = false;                               // (the chunks overwrite the single call's pyramid)
  SF_HIP(c, hipMemsetAsync(c->sift_ctl.p, 0, 64, c->stream));
  return SF_OK;
}

// The detector on ONE chunk (n_img <= c->sift_batch.chunk images of the size sf_sift_batch_reserve has planned for).  Every
// count stays on the device: k_sift_orient reads the image's extrema count and shares its list among SIFT_ORIENT_BLOCKS
// wavefronts, k_sift_segments takes the decisions, every image's keys are its segment of the sort, k_sift_rekey and
// k_sift_emit exit past their image's counts.  sift_ctl from byte 64 on, [chunk] words each: extrema, keypoints, segment
// begin, segment end, rekey flag -- the two counters are cleared per chunk, as the claim bitmaps are.  An image with more
// extrema or keypoints than cap_img keeps no keypoint and is counted in word 0 of sift_ctl (sf_sift_batch_status: the most
// recent BATCH call's, which sf_sift_batch_begin clears).
// `one` (the single-image entry point; a chunk of one): both counts come to the host with the wait of the image's sort and
// the entry point refuses an overflow itself; the overflow is counted in word 1, which nobody reads, and c->sift_last
// describes the image's pyramid afterwards.
int sf_launch_detect_sift(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                          int max_features, const sf_sift_params* prm, sf_keypoint* d_kpts_out, int cap, int32_t* d_n_out,
                          SfDetectOne* one) {
  const SfSiftBatchPlan& bp = c->sift_batch;
  const SfSiftPlan& P = bp.P;
  const int n = prm->n_octave_layers, m = n_img;
  const size_t ctl_words = ((size_t)bp.chunk + 15) & ~(size_t)15;
  if (one) c->sift_last_ok = false;
  if (m < 1 || m > bp.chunk || P.w[0] != 2 * width || P.h[0] != 2 * height || P.n_layers != n || !c->sift_tables_ok ||
      c->sift_tables_n != n || c->sift_tables_sigma != prm->sigma || (m > 1 && max_features < 1) ||
      c->sift_planes.bytes < (size_t)bp.chunk * (bp.plane_bytes + bp.claim_words * 4) ||
      c->sift_keys.bytes < (size_t)bp.chunk * bp.cap_img * 20 || c->sift_ctl.bytes < 64 + 5 * ctl_words * sizeof(unsigned))
    return sf_fail(c, SF_EINVAL, "SIFT batch: a chunk of %d images of %d x %d is not what sf_sift_batch_reserve has planned", m, width, height);
  int rc;
  const SiftBatch B = {img_stride, bp.plane_bytes / 2, bp.claim_words, bp.cap_img};
  if ((rc = sift_launch_pyramids(c, bp, n, d_images, width, height, pitch, m, B)) != SF_OK) return rc;
  short* gauss = (short*)c->sift_planes.p;
  short* dog = (short*)((uint8_t*)c->sift_planes.p + bp.off_dog);
  unsigned* claimed = (unsigned*)((uint8_t*)c->sift_planes.p + (size_t)bp.chunk * bp.plane_bytes);
  unsigned long long* keys = (unsigned long long*)c->sift_keys.p;
  unsigned long long* keys_sorted = keys + (size_t)bp.chunk * bp.cap_img;
  unsigned* list = (unsigned*)(keys_sorted + (size_t)bp.chunk * bp.cap_img);
  unsigned* overflowed = (unsigned*)c->sift_ctl.p + (one ? 1 : 0);
  unsigned *n_ext = (unsigned*)c->sift_ctl.p + 16, *n_kp = n_ext + ctl_words, *seg_begin = n_kp + ctl_words,
           *seg_end = seg_begin + ctl_words, *flipped = seg_end + ctl_words;
  if (one) SF_HIP(c, hipMemsetAsync(overflowed, 0, 4, c->stream));
  SF_HIP(c, hipMemsetAsync(n_ext, 0, 2 * ctl_words * sizeof(unsigned), c->stream));
  const SiftPrm K = sift_kernel_params(*prm);
  const SiftCounts C = {n_ext, n_kp, flipped, d_n_out};
  const unsigned z = (unsigned)m;
  const int rows = max_features > 0 ? std::min(max_features, cap) : cap;      // what an image writes at the most
  hipLaunchKernelGGL(k_sift_extrema, dim3(blocks_of((size_t)P.w[0] * P.h[0]), P.n_octaves * n, z), dim3(256), 0, c->stream, P,
                     (const short*)dog, K, claimed, list, n_ext, bp.cap_img, B);
  hipLaunchKernelGGL(k_sift_orient, dim3(std::min(SIFT_ORIENT_BLOCKS, bp.cap_img), 1, z), dim3(64), 0, c->stream, P, (const short*)gauss,
                     (const short*)dog, K, (const unsigned*)list, keys, n_kp, bp.cap_img, C, B);
  hipLaunchKernelGGL(k_sift_segments, dim3(blocks_of(m)), dim3(256), 0, c->stream, (const unsigned*)n_ext, n_kp, m, bp.cap_img,
                     (size_t)bp.cap_img, prm->n_features, max_features, rows, seg_begin, seg_end, flipped, d_n_out, overflowed);
  hipLaunchKernelGGL(k_sift_rekey, dim3(blocks_of(std::max(rows, 1)), 1, z), dim3(256), 0, c->stream, keys, C, B);
  SF_HIP(c, hipGetLastError());
  SfSortBounds hb;
  if (one) { hb.d_also[0] = n_ext; hb.d_also[1] = n_kp; }   // (both counts arrive with the bounds)
  if ((rc = sf_sort_segments(c, keys, keys_sorted, (unsigned)((size_t)m * bp.cap_img), (unsigned)m, seg_begin, seg_end, 0, 64, true,
                             &hb)) != SF_OK)
    return rc;
  // the emit grid, a wavefront per keypoint: sized by the rows an image may write, or -- a lone image, whose count the
  // sort has brought to the host -- by its keypoints
  const int written = m == 1 ? std::min(sf_limit_keypoints(hb.n(), sf_sift_limit(prm->n_features, max_features)), cap) : rows;
  if (written > 0)
    hipLaunchKernelGGL(k_sift_emit, dim3(written, 1, z), dim3(64), 0, c->stream, P, (const short*)gauss, (const short*)dog, K,
                       (const unsigned long long*)keys_sorted, d_kpts_out, cap, C, B);
  SF_HIP(c, hipGetLastError());
  if (one) {
    one->count[0] = hb.also[0];
    one->count[1] = hb.also[1];
    sift_remember_pyramid(c, bp, prm, width, height);
  }
  return SF_OK;
}

// k_sift_describe for sf_launch_extract_batch (k_extract.hip).  One image: the pyramid is the detector's when the full call
// has just run it on this image with these parameters (reuse), else it is built here.  kind.batch: the n_img images of the
// chunk sf_launch_detect_sift has just run -- their pyramids are read where it left them.
int sf_launch_sift_describe(sf_context* c, const uint8_t* d_left, int pitch, int width, int height, const SfSiftKind& kind,
                            const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status, int n, int n_img,
                            const ExtractCam& cam, sf_keypoint* d_kpts_out, float* desc_tmp, float* xyz_tmp, uint8_t* keep,
                            const ExtractBatch& B) {
  const sf_sift_params& a = kind.prm;
  if (kind.batch) {
    const SfSiftBatchPlan& bp = c->sift_batch;
    if (n_img > bp.chunk || bp.P.w[0] != 2 * width || bp.P.h[0] != 2 * height || bp.P.n_layers != a.n_octave_layers ||
        c->sift_planes.bytes < (size_t)bp.chunk * bp.plane_bytes)
      return sf_fail(c, SF_EINVAL, "SIFT batch: the chunk's pyramids are not the detector's");
    hipLaunchKernelGGL(k_sift_describe, dim3((unsigned)n, (unsigned)n_img), dim3(256), 0, c->stream, bp.P, (const short*)c->sift_planes.p,
                       d_kpts, d_right_x, d_status, n, cam, d_kpts_out, desc_tmp, xyz_tmp, keep, B, bp.plane_bytes / 2, (int)kind.u8);
    return SF_OK;
  }
  const sf_sift_params& b = c->sift_last_prm;
  const bool reuse = kind.reuse && c->sift_last_ok && c->sift_last_width == width && c->sift_last_height == height &&
                     a.n_octave_layers == b.n_octave_layers && a.sigma == b.sigma;
  int rc;
  if (!reuse && (rc = sf_sift_build_pyramid(c, d_left, width, height, pitch, &kind.prm)) != SF_OK) return rc;
  hipLaunchKernelGGL(k_sift_describe, dim3((unsigned)n), dim3(256), 0, c->stream, c->sift_last, (const short*)c->sift_planes.p, d_kpts,
                     d_right_x, d_status, n, cam, d_kpts_out, desc_tmp, xyz_tmp, keep, B, (size_t)0, (int)kind.u8);
  return SF_OK;
}

// One plane of the most recent detector call -> d_out (int16, w x h of the octave, dense)
int sf_sift_copy_plane(sf_context* c, int octave, int layer, int dog, int16_t* d_out) {
  if (!c->sift_last_ok) return sf_fail(c, SF_EINVAL, "sf_debug_sift_plane: no SIFT detector call has built a pyramid on this handle");
  const SfSiftPlan& P = c->sift_last;
  const int planes = P.n_layers + (dog ? 2 : 3);
  if (octave < 0 || octave >= P.n_octaves || layer < 0 || layer >= planes || !d_out)
    return sf_fail(c, SF_EINVAL, "sf_debug_sift_plane: octave %d outside 0 .. %d or layer %d outside 0 .. %d", octave, P.n_octaves - 1, layer,
                   planes - 1);
  const size_t plane = (size_t)P.w[octave] * P.h[octave];
  const uint8_t* base = (const uint8_t*)c->sift_planes.p + (dog ? c->sift_last_off_dog : 0);
  const short* src = (const short*)base + (dog ? P.dog_off[octave] : P.gauss_off[octave]) + (size_t)layer * plane;
  SF_HIP(c, hipMemcpyAsync(d_out, src, plane * 2, hipMemcpyDeviceToDevice, c->stream));
  return SF_OK;
}
