// k_extract.hip -- SURVEY.md section 8 row f3: the features of one stereo keyframe for given corners, written
// straight into the device-resident keyframe store.
//
// What it replaces: RegistrationVis::getFeaturesImpl (myRegistrationVis.cpp:343-436) as called by
// StereoCamGeometricTools::getFeaturesAndDescriptor (stereoCamGeometricTools.cpp:100-120):
//   :343-354  descriptors for the given keypoints      -> BRIEF from the integral image of the left image
//   :356-383  3D keypoints of the stereo pair          -> disparity projection + local transform
//   :384-425  drop keypoints without a finite 3D point when a depth range is set
// The bodies of generateDescriptors / generateKeypoints3D are rtabmap / opencv_contrib code that is not in the
// reference tree; the algorithm restated here is documented next to the CPU restatement the tests compare with.
// Arithmetic: the float operations in the order written, no contraction (this file is compiled with
// -ffp-contract=off), IEEE division -- the outputs are compared byte for byte.
//
// GFTT/ORB (Vis/FeatureType 8) replaces the integral image and the BRIEF tests by k_orb_blur / k_orb_angle /
// k_orb_points below (cv::ORB::compute on the given keypoints); the 3D points and the commit are shared.
// FREAK (Vis/FeatureType 3 and 5) keeps the integral image and replaces k_extract_points by k_freak_points (k_freak.hip).
// SURF (Vis/FeatureType 0) does the same with k_surf_describe (k_surf.hip) and float32 rows.
// SIFT (Vis/FeatureType 1) reads no integral image: k_sift_describe (k_sift.hip) works on the Gaussian pyramid, float32 rows.
//
// Kernels (one keyframe = a few hundred to a few thousand corners of one 752 x 480 .. 1280 x 720 image):
//   k_integral_rows   one workgroup per image row: wavefront scans of 256-pixel segments, running carry
//   k_integral_cols   one thread per column: the running column sum (coalesced across the row)
//   k_extract_points  one thread per (corner, descriptor byte): 8 tests = 64 integral-image reads; byte 0's thread
//                     also does the border test and the 3D point
//   k_extract_commit  ONE workgroup: order-preserving compaction of the kept corners (block scan of the keep
//                     flags) into the store slot -- descriptor words, xyz, reduced keypoints, meta -- and into the
//                     optional wire copies
// The image is HBM-resident input (W*H bytes read once by the row pass, 4 (W+1)(H+1) bytes of integral image written
// and re-read through L2 by the tests); at these sizes every kernel is launch-latency-bound, which is why the
// per-keyframe work is three short launches and not a pipeline.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sf_extract_device.hpp"
#include "sf_front_device.hpp"

namespace {

constexpr int BRIEF_PATCH = 48;
constexpr int BRIEF_KERNEL = 9;
constexpr int BRIEF_BORDER = BRIEF_PATCH / 2 + BRIEF_KERNEL / 2;   // KeyPointsFilter::runByImageBorder margin

// S is (h + 1) x (w + 1); this pass leaves ROW prefix sums in rows 1..h and zeroes row 0 / column 0.
__global__ void __launch_bounds__(256)
k_integral_rows(const uint8_t* __restrict__ img, int w, int h, int pitch, int32_t* __restrict__ S, ExtractBatch B) {
  __shared__ int wave_sum[4];
  img += blockIdx.y * B.img_stride;
  S += blockIdx.y * B.s_stride;
  const int y = blockIdx.x;          // 0..h: row y of S
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* row = S + (size_t)y * (w + 1);
  if (y == 0) {
    for (int x = tid; x <= w; x += 256) row[x] = 0;
    return;
  }
  const uint8_t* src = img + (size_t)(y - 1) * pitch;
  if (tid == 0) row[0] = 0;
  int carry = 0;
  for (int base = 0; base < w; base += 256) {
    const int x = base + tid;
    int v = x < w ? (int)src[x] : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(v, off);
      if (lane >= off) v += u;
    }
    if (lane == 63) wave_sum[wave] = v;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int s = wave_sum[q];
      if (q < wave) before += s;
      total += s;
    }
    if (x < w) row[x + 1] = carry + before + v;
    carry += total;
    __syncthreads();
  }
}

// One thread per column; the rows are taken 16 at a time so that 16 loads are in flight per dependent step (a
// load-add-store per row was ~480 serial L2 round trips: 120 of the call's 154 us at 752 x 480).
__global__ void __launch_bounds__(64)
k_integral_cols(int w, int h, int32_t* __restrict__ S, ExtractBatch B) {
  const int x = blockIdx.x * 64 + threadIdx.x;   // column 1..w of S
  if (x < 1 || x > w) return;
  S += blockIdx.y * B.s_stride;
  const size_t pitch = (size_t)(w + 1);
  int32_t run = 0;
  int y = 1;
  for (; y + 15 <= h; y += 16) {
    int32_t v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = S[(size_t)(y + u) * pitch + x];
#pragma unroll
    for (int u = 0; u < 16; ++u) { run += v[u]; v[u] = run; }
#pragma unroll
    for (int u = 0; u < 16; ++u) S[(size_t)(y + u) * pitch + x] = v[u];
  }
  for (; y <= h; ++y) {
    int32_t* p = S + (size_t)y * pitch + x;
    run += *p;
    *p = run;
  }
}

// (row h + 1 / column w + 1 -- asked for by a +24 offset at a corner that rounds onto the border limit, out of bounds
//  upstream -- repeat the last row / column)
__device__ __forceinline__ int32_t smoothed(const int32_t* __restrict__ S, int w1, int h1, int px, int py, int dx, int dy) {
  constexpr int hk = BRIEF_KERNEL / 2;
  const int y = py + dy, x = px + dx;
  const int y1 = min(y + hk + 1, h1 - 1), x1 = min(x + hk + 1, w1 - 1);
  return S[(size_t)y1 * w1 + x1] - S[(size_t)y1 * w1 + x - hk] - S[(size_t)(y - hk) * w1 + x1] +
         S[(size_t)(y - hk) * w1 + x - hk];
}

// one thread per (corner, descriptor byte)
__global__ void __launch_bounds__(256)
k_extract_points(const int32_t* __restrict__ S, int w, int h, const sf_keypoint* __restrict__ kpts,
                 const float* __restrict__ right_x, const uint8_t* __restrict__ status, int n, int bytes,
                 const int8_t* __restrict__ tests, ExtractCam cam, uint8_t* __restrict__ desc_tmp,
                 float* __restrict__ xyz_tmp, uint8_t* __restrict__ keep, ExtractBatch B) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int i = g / bytes, b = g - i * bytes;
  if (B.d_n) n = min(n, B.d_n[blockIdx.y]);
  if (i >= n) return;
  {
    const size_t o = (size_t)blockIdx.y * B.per_image;
    S += blockIdx.y * B.s_stride;
    kpts += o;
    if (right_x) right_x += o;
    if (status) status += o;
    desc_tmp += o * bytes; xyz_tmp += 3 * o; keep += o;
  }
  const sf_keypoint k = kpts[i];
  const bool inside = k.x >= (float)BRIEF_BORDER && k.x < (float)(w - BRIEF_BORDER) && k.y >= (float)BRIEF_BORDER &&
                      k.y < (float)(h - BRIEF_BORDER);
  if (inside) {
    const int px = (int)(k.x + 0.5f), py = (int)(k.y + 0.5f);
    unsigned v = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const char4 q = reinterpret_cast<const char4*>(tests)[8 * b + t];   // x1, y1, x2, y2
      v = (v << 1) | (unsigned)(smoothed(S, w + 1, h + 1, px, py, q.x, q.y) < smoothed(S, w + 1, h + 1, px, py, q.z, q.w));
    }
    desc_tmp[(size_t)i * bytes + b] = (uint8_t)v;
  }
  if (b != 0) return;
  extract_point(k, i, inside, right_x, status, cam, xyz_tmp, keep);
}

// ---- GFTT/ORB descriptors (Vis/FeatureType 8): cv::ORB::compute on provided keypoints, one pyramid level ----------
// DESIGN.md section 4 restates the arithmetic; tests/orb_ref.py is the NumPy restatement the tests compare with.
//   k_orb_blur    one workgroup per band of ORB_BLUR_ROWS rows (blockIdx.y = image): the 7 x 7, sigma 2 Gaussian of
//                 the level-0 image in OpenCV's 8-bit fixed point (row pass into an LDS tile with a 3-row halo,
//                 column pass to u8), reflect-101 beyond the image
//   k_orb_angle   (orientation = 1 only) one wavefront per corner: ORB's intensity-centroid angle on the unblurred
//                 image, lanes 0..30 one patch row each, moments reduced with shuffles, lane 0 writes the keypoint
//   k_orb_points  one thread per (corner, descriptor byte): border / octave test, 16 rotated samples; byte 0's thread
//                 also does the 3D point (extract_point)
// k_extract_commit then compacts the kept corners exactly as for BRIEF (32-byte rows).
constexpr int ORB_HALF = 15;           // PatchSize 31 / 2
constexpr int ORB_BYTES = 32;          // WTA_K 2
constexpr int ORB_BLUR_ROWS = 8;

struct OrbTaps { int t[7]; };          // getGaussianKernel(7, 2) * 256, rounded (host: orb_blur_taps)
struct OrbUmax { int u[ORB_HALF + 1]; };   // the circular patch's half widths (host: orb_umax)

// KeyPointsFilter::runByImageBorder(kpts, size, e): Rect(e, e, w - 2e, h - 2e).contains(Point(cvRound(pt))), and
// nothing survives when w <= 2e or h <= 2e; corners whose octave is not one of the n_levels levels are dropped as well
// (one level for GFTT/ORB: another octave than 0)
__device__ __forceinline__ bool orb_inside(const sf_keypoint& k, int w, int h, int e, int n_levels) {
  if (w <= 2 * e || h <= 2 * e || (k.octave & 255) >= n_levels) return false;
  const float rx = rintf(k.x), ry = rintf(k.y);
  return rx >= (float)e && rx < (float)(w - e) && ry >= (float)e && ry < (float)(h - e);
}

// blur: W x H per image, B.s_stride bytes apart
__global__ void __launch_bounds__(256)
k_orb_blur(const uint8_t* __restrict__ img, int w, int h, int pitch, uint8_t* __restrict__ blur, OrbTaps T, ExtractBatch B) {
  __shared__ int rows[ORB_BLUR_ROWS + 6][256];
  img += blockIdx.y * B.img_stride;
  blur += blockIdx.y * B.s_stride;
  const int y0 = blockIdx.x * ORB_BLUR_ROWS, tid = threadIdx.x;
  for (int x0 = 0; x0 < w; x0 += 256) {
    const int x = x0 + tid;
    if (x < w) {
      int xs[7];
#pragma unroll
      for (int d = 0; d < 7; ++d) xs[d] = reflect101(x + d - 3, w);
      for (int r = 0; r < ORB_BLUR_ROWS + 6; ++r) {
        const uint8_t* src = img + (size_t)reflect101(y0 + r - 3, h) * pitch;
        int s = 0;
#pragma unroll
        for (int d = 0; d < 7; ++d) s += T.t[d] * (int)src[xs[d]];
        rows[r][tid] = s;
      }
    }
    __syncthreads();
    if (x < w) {
      for (int r = 0; r < ORB_BLUR_ROWS && y0 + r < h; ++r) {
        int s = 0;
#pragma unroll
        for (int d = 0; d < 7; ++d) s += T.t[d] * rows[r + d][tid];
        blur[(size_t)(y0 + r) * w + x] = (uint8_t)min((s + (1 << 15)) >> 16, 255);
      }
    }
    __syncthreads();
  }
}

// one wavefront per corner; every corner's keypoint goes to kpts_out, the kept ones with their angle.  The corner lies
// on level (octave & 255) of P, in that level's coordinates (GFTT/ORB: one level, the image; the ORB detector: its pyramid)
__global__ void __launch_bounds__(256)
k_orb_angle(const uint8_t* __restrict__ img, int pitch, const uint8_t* __restrict__ pyr, SfOrbPyr P,
            const sf_keypoint* __restrict__ kpts, int n, int edge, OrbUmax U, sf_keypoint* __restrict__ kpts_out, ExtractBatch B) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (B.d_n) n = min(n, B.d_n[blockIdx.y]);
  if (i >= n) return;
  img += blockIdx.y * B.img_stride;
  if (pyr) pyr += blockIdx.y * B.pyr_stride;
  kpts += (size_t)blockIdx.y * B.per_image;
  kpts_out += (size_t)blockIdx.y * B.per_image;
  sf_keypoint k = kpts[i];
  const int l = k.octave & 255;
  const SfOrbLevel L = sf_orb_level(P, l);
  const bool inside = orb_inside(k, L.w, L.h, edge, P.n);
  int m01 = 0, m10 = 0;
  if (inside && lane <= 2 * ORB_HALF) {       // edge >= 16: the whole patch lies in the level
    const int v = lane - ORB_HALF, d = U.u[v < 0 ? -v : v];
    const uint8_t* row = (l == 0 ? img : pyr + L.off) + (size_t)((int)rintf(k.y) + v) * (l == 0 ? pitch : L.w) + (int)rintf(k.x);
    int s = 0;
    for (int u = -d; u <= d; ++u) {
      const int val = row[u];
      s += val;
      m10 += u * val;
    }
    m01 = v * s;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    m01 += __shfl_xor(m01, off);
    m10 += __shfl_xor(m10, off);
  }
  if (lane == 0) {
    if (inside) k.angle = sf_fast_atan2((float)m01, (float)m10);
    kpts_out[i] = k;
  }
}

// one thread per (corner, descriptor byte); samples inside the image read the blurred copy, the others the
// reflect-101 padding of the source, which ORB never blurs.  The border filter is level 0's (w x h); the samples are
// taken on level (octave & 255) of P around cvRound(position * (1.f / scale_l)) -- one level for GFTT/ORB, where this is
// the image around cvRound(position)
__global__ void __launch_bounds__(256)
k_orb_points(const uint8_t* __restrict__ img, const uint8_t* __restrict__ blur, int w, int h, int pitch,
             const uint8_t* __restrict__ pyr, SfOrbPyr P, const sf_keypoint* __restrict__ kpts, const float* __restrict__ right_x, const uint8_t* __restrict__ status,
             int n, int edge, const int8_t* __restrict__ tests, ExtractCam cam, uint8_t* __restrict__ desc_tmp,
             float* __restrict__ xyz_tmp, uint8_t* __restrict__ keep, ExtractBatch B) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int i = g / ORB_BYTES, b = g - i * ORB_BYTES;
  if (B.d_n) n = min(n, B.d_n[blockIdx.y]);
  if (i >= n) return;
  {
    const size_t o = (size_t)blockIdx.y * B.per_image;
    img += blockIdx.y * B.img_stride;
    blur += blockIdx.y * B.s_stride;
    if (pyr) pyr += blockIdx.y * B.pyr_stride;
    kpts += o;
    if (right_x) right_x += o;
    if (status) status += o;
    desc_tmp += o * ORB_BYTES; xyz_tmp += 3 * o; keep += o;
  }
  const sf_keypoint k = kpts[i];
  const bool inside = orb_inside(k, w, h, edge, P.n);
  if (inside) {
    const int l = k.octave & 255;
    const SfOrbLevel L = sf_orb_level(P, l);
    const uint8_t* lim = l == 0 ? img : pyr + L.off;
    const uint8_t* lbl = blur + L.off;
    const int lw = L.w, lh = L.h, lp = l == 0 ? pitch : L.w;
    const int cx = (int)rintf(k.x * L.inv_scale), cy = (int)rintf(k.y * L.inv_scale);
    const float ang = k.angle * (float)(3.14159265358979323846 / 180.0);
    const float ca = (float)cos((double)ang), sa = (float)sin((double)ang);
    auto sample = [&](int px, int py) -> int {
      const int ix = (int)rintf((float)px * ca - (float)py * sa), iy = (int)rintf((float)px * sa + (float)py * ca);
      const int X = cx + ix, Y = cy + iy;
      if (X >= 0 && X < lw && Y >= 0 && Y < lh) return lbl[(size_t)Y * lw + X];
      return lim[(size_t)reflect101(Y, lh) * lp + reflect101(X, lw)];
    };
    unsigned v = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const char4 q = reinterpret_cast<const char4*>(tests)[8 * b + t];   // x1, y1, x2, y2
      v |= (unsigned)(sample(q.x, q.y) < sample(q.z, q.w)) << t;          // LSB first
    }
    desc_tmp[(size_t)i * ORB_BYTES + b] = (uint8_t)v;
  }
  if (b != 0) return;
  extract_point(k, i, inside, right_x, status, cam, xyz_tmp, keep);
}

// ONE workgroup: stable compaction into the store slot (and the optional wire copies)
__global__ void __launch_bounds__(256)
k_extract_commit(const sf_keypoint* __restrict__ kpts, const uint8_t* __restrict__ desc_tmp,
                 const float* __restrict__ xyz_tmp, const uint8_t* __restrict__ keep, int n, int bytes, int has3d,
                 uint32_t* __restrict__ st_desc, float* __restrict__ st_xyz, float4* __restrict__ st_kp,
                 int4* __restrict__ st_meta, int kcap, int w_dwords, int slot, uint8_t* __restrict__ desc_out,
                 float* __restrict__ xyz_out, sf_keypoint* __restrict__ kp_out, int32_t* __restrict__ rows_out,
                 ExtractBatch B, int group_levels) {
  // (group_levels > 1, the ORB pyramid: the rows of level 0 first, then level 1, ... -- one compaction pass per level)
  __shared__ int wave_cnt[4];
  const int tid = threadIdx.x;
  if (B.d_n) n = min(n, B.d_n[blockIdx.x]);
  {
    const size_t o = (size_t)blockIdx.x * B.per_image;
    slot += blockIdx.x;
    kpts += o; desc_tmp += o * bytes; xyz_tmp += 3 * o; keep += o;
    if (desc_out) desc_out += o * bytes;
    if (xyz_out) xyz_out += 3 * o;
    if (kp_out) kp_out += o;
    if (rows_out) rows_out += blockIdx.x;
  }
  uint8_t* d8 = reinterpret_cast<uint8_t*>(st_desc + (size_t)slot * kcap * w_dwords);
  float* dx = st_xyz + (size_t)slot * kcap * 3;
  float4* dk = st_kp + (size_t)slot * kcap;
  const int rowb = w_dwords * 4;
  int running = 0;
  const int chunks = (n + 255) / 256;
  for (int it = 0; it < chunks * max(group_levels, 1); ++it) {
    const int lv = it / max(chunks, 1), i = (it - lv * chunks) * 256 + tid;
    const bool f = i < n && keep[i] && (group_levels <= 1 || (kpts[i].octave & 255) == lv);
    const SfRank rank = sf_block_rank(f, wave_cnt);
    if (f) {
      const int o = running + rank.before;
      const sf_keypoint k = kpts[i];
      for (int b = 0; b < rowb; ++b) d8[(size_t)o * rowb + b] = b < bytes ? desc_tmp[(size_t)i * bytes + b] : (uint8_t)0;
      const float p0 = xyz_tmp[3 * i], p1 = xyz_tmp[3 * i + 1], p2 = xyz_tmp[3 * i + 2];
      dx[3 * o] = p0; dx[3 * o + 1] = p1; dx[3 * o + 2] = p2;
      int oc = k.octave & 255;
      oc = oc < 128 ? oc : (-128 | oc);
      dk[o] = make_float4(k.x, k.y, __int_as_float(oc), 0.f);
      if (desc_out) for (int b = 0; b < bytes; ++b) desc_out[(size_t)o * bytes + b] = desc_tmp[(size_t)i * bytes + b];
      if (xyz_out) { xyz_out[3 * o] = p0; xyz_out[3 * o + 1] = p1; xyz_out[3 * o + 2] = p2; }
      if (kp_out) kp_out[o] = k;
    }
    running += rank.total;
    __syncthreads();
  }
  if (tid == 0) {
    st_meta[slot] = make_int4(running, has3d ? running : 0, running, bytes);
    if (rows_out) *rows_out = running;
  }
}

}  // namespace

// Default test set of a fresh handle: isotropic Gaussian offsets (sigma = patch / 5, the "G II" construction of the
// BRIEF paper), clipped to the patch, from a fixed linear congruential stream -- NOT OpenCV's table.
void sf_brief_default_pattern(int8_t* tests, int bytes) {
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto uni = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)((s >> 11) + 1) / 9007199254740993.0;   // (0, 1)
  };
  for (int t = 0; t < 8 * bytes * 4; t += 2) {
    const double r = std::sqrt(-2.0 * std::log(uni())), a = 6.283185307179586 * uni();
    const double sigma = BRIEF_PATCH / 5.0;
    int x = (int)std::lround(sigma * r * std::cos(a)), y = (int)std::lround(sigma * r * std::sin(a));
    x = x < -BRIEF_PATCH / 2 ? -BRIEF_PATCH / 2 : (x > BRIEF_PATCH / 2 ? BRIEF_PATCH / 2 : x);
    y = y < -BRIEF_PATCH / 2 ? -BRIEF_PATCH / 2 : (y > BRIEF_PATCH / 2 ? BRIEF_PATCH / 2 : y);
    tests[t] = (int8_t)x;
    tests[t + 1] = (int8_t)y;
  }
}

// Default ORB test set of a fresh handle: OpenCV's own makeRandomPattern(31, 512) -- cv::RNG(0x34985739), uniform(-15, 16)
// for x then y of each of the 512 points, test k = (point 2k, point 2k + 1).  NOT OpenCV's bit_pattern_31_ table.
void sf_orb_default_pattern(int8_t* tests) {
  uint64_t s = 0x34985739u;
  auto next = [&]() {                       // cv::RNG::next: multiply-with-carry
    s = (uint64_t)(uint32_t)s * 4164903690ull + (s >> 32);
    return (uint32_t)s;
  };
  for (int t = 0; t < 8 * ORB_BYTES * 4; ++t) tests[t] = (int8_t)((int)(next() % 31u) - ORB_HALF);
}

// getGaussianKernel(7, 2, CV_32F), every tap times 256 rounded to an integer (OpenCV 3.x's 8-bit fixed point): the
// taps are 18 34 49 55 49 34 18 and sum to 257
static OrbTaps orb_blur_taps() {
  float cf[7];
  double sum = 0.0;
  for (int i = 0; i < 7; ++i) {
    const double x = i - 3.0;
    cf[i] = (float)std::exp((-0.5 / (2.0 * 2.0)) * x * x);
    sum += cf[i];
  }
  sum = 1.0 / sum;
  OrbTaps T;
  for (int i = 0; i < 7; ++i) T.t[i] = (int)std::lrint((double)((float)(cf[i] * sum) * 256.0f));
  return T;
}

// ORB's umax: the half width of every row of the radius-15 circular patch, made symmetric about the diagonal
static OrbUmax orb_umax() {
  int umax[ORB_HALF + 2] = {};
  const int vmax = (int)std::floor(ORB_HALF * std::sqrt(2.f) / 2 + 1);
  const int vmin = (int)std::ceil(ORB_HALF * std::sqrt(2.f) / 2);
  for (int v = 0; v <= vmax; ++v) umax[v] = (int)std::lrint(std::sqrt((double)ORB_HALF * ORB_HALF - v * v));
  for (int v = ORB_HALF, v0 = 0; v >= vmin; --v) {
    while (umax[v0] == umax[v0 + 1]) ++v0;
    umax[v] = v0;
    ++v0;
  }
  OrbUmax U;
  for (int v = 0; v <= ORB_HALF; ++v) U.u[v] = umax[v];
  return U;
}

// The integral images of n_img images (B->img_stride apart) into c->ex_integral, B->s_stride entries apart
static int integral_images(sf_context* c, const uint8_t* d_left, int n_img, int width, int height, int pitch, ExtractBatch* B,
                           int32_t** S_out) {
  const size_t s_entries = (size_t)(width + 1) * (height + 1);
  const int rc = sf_buf_reserve(c, c->ex_integral, s_entries * sizeof(int32_t) * n_img);
  if (rc != SF_OK) return rc;
  int32_t* S = (int32_t*)c->ex_integral.p;
  B->s_stride = s_entries;
  hipLaunchKernelGGL(k_integral_rows, dim3(height + 1, n_img), dim3(256), 0, c->stream, d_left, width, height, pitch, S, *B);
  hipLaunchKernelGGL(k_integral_cols, dim3((width + 1 + 63) / 64, n_img), dim3(64), 0, c->stream, width, height, S, *B);
  *S_out = S;
  return SF_OK;
}

// One image's integral image for a detector that reads it (SURF, k_surf.hip); the extraction call behind builds its own
int sf_launch_integral(sf_context* c, const uint8_t* d_image, int width, int height, int pitch, const int32_t** S_out) {
  ExtractBatch B;
  B.img_stride = 0; B.s_stride = 0; B.pyr_stride = 0; B.per_image = 0; B.d_n = nullptr;
  int32_t* S = nullptr;
  const int rc = integral_images(c, d_image, 1, width, height, pitch, &B, &S);
  if (rc != SF_OK) return rc;
  SF_HIP(c, hipGetLastError());
  *S_out = S;
  return SF_OK;
}

// The same for the n_img images of a batch, *s_stride entries apart: the detector reads them, and so does the extraction
// behind it (ExtractKind::integral_ready)
int sf_launch_integral_batch(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height,
                             int pitch, const int32_t** S_out, size_t* s_stride) {
  ExtractBatch B;
  B.img_stride = img_stride; B.s_stride = 0; B.pyr_stride = 0; B.per_image = 0; B.d_n = nullptr;
  int32_t* S = nullptr;
  const int rc = integral_images(c, d_images, n_img, width, height, pitch, &B, &S);
  if (rc != SF_OK) return rc;
  SF_HIP(c, hipGetLastError());
  *S_out = S;
  *s_stride = B.s_stride;
  return SF_OK;
}

// Launch sequence on the handle's stream; the store slots from `slot` on (c->store: kcap >= n, w dwords) have been
// reserved by the caller.  Image i at d_left + i * img_stride, its corners / right_x / status / optional copies at + i * n
// entries, its store slot = slot + i.  d_n (device): the corner count of every image, `n` is then the per-image
// capacity; null (one image): n is the count.
int sf_launch_extract_batch(sf_context* c, const uint8_t* d_left, size_t img_stride, int n_img, int width, int height,
                            int pitch, const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status, int n,
                            const int32_t* d_n, const sf_stereo_camera* cam, const ExtractKind& kind, int slot,
                            uint8_t* d_desc_out, float* d_xyz_out, sf_keypoint* d_kpts_out, int32_t* d_rows_out,
                            const SfDepthIn* depth) {
  const int bytes = kind.bytes;
  const sf_orb_params* orb = kind.orb;
  const sf_orb_detector_params* pyr = kind.pyr;
  const Store& st = c->store;
  int rc;
  if (pyr && (!orb || (!kind.pyr_stride && n_img != 1)))
    return sf_fail(c, SF_EINVAL, "ORB on a pyramid: one keyframe per call unless the detector has left the batch's pyramids");
  if (orb && bytes != ORB_BYTES) return sf_fail(c, SF_EINVAL, "ORB rows are %d bytes, not %d", ORB_BYTES, bytes);
  if (kind.freak && (orb || bytes != FREAK_BYTES)) return sf_fail(c, SF_EINVAL, "FREAK rows are %d bytes, not %d", FREAK_BYTES, bytes);
  if (kind.surf && (orb || kind.freak || bytes != (kind.surf->extended ? 512 : 256)))
    return sf_fail(c, SF_EINVAL, "SURF rows are %d bytes, not %d", kind.surf->extended ? 512 : 256, bytes);
  if (kind.has_sift && (orb || kind.freak || kind.surf || bytes != (kind.sift.u8 ? SF_DESC_BYTES_U8 : 512) || (n_img != 1 && !kind.sift.batch)))
    return sf_fail(c, SF_EINVAL, "SIFT rows are %d bytes, one keyframe per call unless the detector has left the chunk's pyramids (not %d bytes, %d keyframes)",
                   kind.sift.u8 ? SF_DESC_BYTES_U8 : 512, bytes, n_img);
  const size_t rows_all = (size_t)std::max(n, 1) * n_img;
  if ((rc = sf_buf_reserve(c, c->ex_desc, rows_all * bytes)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->ex_xyz, rows_all * 12)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->ex_keep, rows_all)) != SF_OK) return rc;
  ExtractBatch B;
  B.img_stride = img_stride; B.pyr_stride = 0; B.per_image = n; B.d_n = d_n;
  SfOrbPyr P = sf_orb_single_level(width, height);
  int32_t* S = nullptr;
  if (kind.integral_ready) {                             // the detector's, of these images: nothing has written the buffer since
    B.s_stride = (size_t)(width + 1) * (height + 1);
    if (orb || c->ex_integral.bytes < B.s_stride * sizeof(int32_t) * n_img)
      return sf_fail(c, SF_EINVAL, "the batch's integral images are not the detector's");
    S = (int32_t*)c->ex_integral.p;
  } else if (kind.has_sift) {                            // (no integral image: k_sift_describe reads the Gaussian pyramid)
  } else if (!orb) {
    if ((rc = integral_images(c, d_left, n_img, width, height, pitch, &B, &S)) != SF_OK) return rc;
  } else if (!pyr) {
    B.s_stride = (size_t)width * height;                 // the blurred level-0 images, back to back
    if ((rc = sf_buf_reserve(c, c->ex_blur, B.s_stride * n_img)) != SF_OK) return rc;
    hipLaunchKernelGGL(k_orb_blur, dim3((height + ORB_BLUR_ROWS - 1) / ORB_BLUR_ROWS, n_img), dim3(256), 0, c->stream,
                       d_left, width, height, pitch, (uint8_t*)c->ex_blur.p, orb_blur_taps(), B);
  } else {                                               // the pyramid and a blurred copy of every level, same offsets
    P = sf_orb_pyr_layout(width, height, pyr->scale_factor, pyr->n_levels);
    if (!kind.pyr_stride) {
      if ((rc = sf_launch_orb_pyramid(c, d_left, pitch, P, 1, 0)) != SF_OK) return rc;
    } else if (kind.pyr_stride != P.total || c->orb_pyr.bytes < (size_t)P.total * n_img) {
      return sf_fail(c, SF_EINVAL, "ORB on a pyramid: the batch's pyramids are not the detector's");
    }
    B.s_stride = B.pyr_stride = P.total;                 // image i's blurred levels at ex_blur + i * P.total + off[l]
    if ((rc = sf_buf_reserve(c, c->ex_blur, (size_t)P.total * n_img)) != SF_OK) return rc;
    for (int l = 0; l < P.n; ++l) {
      ExtractBatch Bl = B;                               // level 0 is the caller's image, the others the pyramid's
      if (l > 0) Bl.img_stride = P.total;
      hipLaunchKernelGGL(k_orb_blur, dim3((P.h[l] + ORB_BLUR_ROWS - 1) / ORB_BLUR_ROWS, n_img), dim3(256), 0, c->stream,
                         l == 0 ? d_left : (const uint8_t*)c->orb_pyr.p + P.off[l], P.w[l], P.h[l], l == 0 ? pitch : P.w[l],
                         (uint8_t*)c->ex_blur.p + P.off[l], orb_blur_taps(), Bl);
    }
  }
  ExtractCam ec = sf_extract_cam(cam);
  const ExtractCam ec_depth = ec;                          // a keyframe with a depth image: the describe kernel runs without right_x
  if (depth) { d_right_x = nullptr; d_status = nullptr; ec.filter = 0; }   // and without the filter, k_depth_points behind it
  const sf_keypoint* kp_commit = d_kpts;
  if (n > 0) {
    const long long threads = (long long)n * bytes;
    if (kind.has_sift) {
      if ((rc = sf_buf_reserve(c, c->ex_kpts, rows_all * sizeof(sf_keypoint))) != SF_OK) return rc;
      if ((rc = sf_launch_sift_describe(c, d_left, pitch, width, height, kind.sift, d_kpts, d_right_x, d_status, n, n_img, ec,
                                        (sf_keypoint*)c->ex_kpts.p, (float*)c->ex_desc.p, (float*)c->ex_xyz.p,
                                        (uint8_t*)c->ex_keep.p, B)) != SF_OK)
        return rc;
      kp_commit = (const sf_keypoint*)c->ex_kpts.p;
    } else if (kind.surf) {                               // the keypoints with their angles, for the commit
      if ((rc = sf_buf_reserve(c, c->ex_kpts, rows_all * sizeof(sf_keypoint))) != SF_OK) return rc;
      sf_launch_surf_describe(c, d_left, pitch, S, width, height, d_kpts, d_right_x, d_status, n, n_img, *kind.surf, ec,
                              (sf_keypoint*)c->ex_kpts.p, (float*)c->ex_desc.p, (float*)c->ex_xyz.p, (uint8_t*)c->ex_keep.p, B);
      kp_commit = (const sf_keypoint*)c->ex_kpts.p;
    } else if (kind.freak) {                              // the keypoints with their angles, for the commit
      if ((rc = sf_buf_reserve(c, c->ex_kpts, rows_all * sizeof(sf_keypoint))) != SF_OK) return rc;
      sf_launch_freak_points(c, d_left, pitch, S, width, height, d_kpts, d_right_x, d_status, n, n_img, *kind.freak, ec,
                             (sf_keypoint*)c->ex_kpts.p, (uint8_t*)c->ex_desc.p, (float*)c->ex_xyz.p, (uint8_t*)c->ex_keep.p, B);
      kp_commit = (const sf_keypoint*)c->ex_kpts.p;
    } else if (!orb) {
      hipLaunchKernelGGL(k_extract_points, dim3((unsigned)((threads + 255) / 256), n_img), dim3(256), 0, c->stream, S, width,
                         height, d_kpts, d_right_x, d_status, n, bytes, kind.d_tests, ec, (uint8_t*)c->ex_desc.p,
                         (float*)c->ex_xyz.p, (uint8_t*)c->ex_keep.p, B);
    } else {
      if (orb->orientation && !pyr) {                     // the keypoints with their angles, for the samples and the commit
        if ((rc = sf_buf_reserve(c, c->ex_kpts, rows_all * sizeof(sf_keypoint))) != SF_OK) return rc;
        hipLaunchKernelGGL(k_orb_angle, dim3((unsigned)((n + 3) / 4), n_img), dim3(256), 0, c->stream, d_left, pitch,
                           (const uint8_t*)nullptr, P, d_kpts, n, orb->edge_threshold, orb_umax(), (sf_keypoint*)c->ex_kpts.p, B);
        kp_commit = (const sf_keypoint*)c->ex_kpts.p;
      }
      hipLaunchKernelGGL(k_orb_points, dim3((unsigned)((threads + 255) / 256), n_img), dim3(256), 0, c->stream, d_left,
                         (const uint8_t*)c->ex_blur.p, width, height, pitch, (const uint8_t*)(pyr ? c->orb_pyr.p : nullptr), P,
                         kp_commit, d_right_x, d_status, n,
                         orb->edge_threshold, kind.d_tests, ec, (uint8_t*)c->ex_desc.p, (float*)c->ex_xyz.p,
                         (uint8_t*)c->ex_keep.p, B);
    }
    if (depth)
      sf_launch_depth_points(c, *depth, width, height, d_kpts, n, n_img, ec_depth, (float*)c->ex_xyz.p, (uint8_t*)c->ex_keep.p,
                             nullptr, B);
  }
  hipLaunchKernelGGL(k_extract_commit, dim3(n_img), dim3(256), 0, c->stream, kp_commit, (const uint8_t*)c->ex_desc.p,
                     (const float*)c->ex_xyz.p, (const uint8_t*)c->ex_keep.p, n, bytes, depth != nullptr || d_right_x != nullptr,
                     (uint32_t*)st.desc.p, (float*)st.xyz.p, (float4*)st.kp.p, (int4*)st.meta.p, st.kcap, st.w, slot,
                     d_desc_out, d_xyz_out, d_kpts_out, d_rows_out, B, pyr ? P.n : 0);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

// The ORB detector's angles (k_orb_detect.hip): keypoints in level coordinates, their number read on the device
int sf_launch_orb_angle_levels(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int pitch, const SfOrbPyr& P,
                               size_t pyr_stride, const sf_keypoint* d_kpts, int n_max, const int32_t* d_n, int edge,
                               sf_keypoint* d_kpts_out) {
  if (n_max <= 0) return SF_OK;
  ExtractBatch B;
  B.img_stride = img_stride; B.s_stride = 0; B.pyr_stride = pyr_stride; B.per_image = n_max; B.d_n = d_n;
  hipLaunchKernelGGL(k_orb_angle, dim3((unsigned)((n_max + 3) / 4), n_img), dim3(256), 0, c->stream, d_images, pitch,
                     (const uint8_t*)c->orb_pyr.p, P, d_kpts, n_max, edge, orb_umax(), d_kpts_out, B);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
