// k_freak.hip -- FREAK descriptors of the keyframe front end (Vis/FeatureType 3 = FAST/FREAK, 5 = GFTT/FREAK):
// cv::xfeatures2d::FREAK::compute on given keypoints, 64-byte rows.  opencv_contrib is not in the reference tree; the
// algorithm is restated in DESIGN.md section 3 item 17g and in tests/freak_ref.py, which the tests compare with byte for
// byte.  Arithmetic: the float operations in the order written, no contraction (compiled with -ffp-contract=off); the one
// log and the one atan2 of a keypoint in float64, rounded to float once.
//
//   k_freak_points  one wavefront per corner, four corners per workgroup (blockIdx.y = image): lanes 0 .. 42 own one
//                   receptive field each -- four reads of BRIEF's integral image, or four pixels for the fields below
//                   half a pixel -- and keep its mean in a register; the other lanes fetch means with ds_bpermute (no LDS
//                   is allocated, nothing is spilled).  Orientation: lanes 0 .. 44 one weighted pair each, two integer
//                   wavefront sums (exact in any order), lane 0 the atan2.  Descriptor: after the second sampling lane L
//                   builds byte L from the eight pairs of one 16-byte table entry; the wavefront stores one coalesced
//                   64-byte row.  Lane 0 writes the keypoint with its angle and does the 3D point (extract_point).
// The integral image before it and k_extract_commit behind it are k_extract.hip's (sf_launch_extract_batch).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "sf_extract_device.hpp"

namespace {

// The mean of one receptive field {px, py, sigma} around the keypoint (FREAK's meanIntensity).  The border test has put
// every field inside the image; the clamps below never act on such a field and are there for memory safety alone.
__device__ __forceinline__ int freak_mean(const uint8_t* __restrict__ img, int pitch, const int32_t* __restrict__ S, int w, int h,
                                          float kx, float ky, float px, float py, float sigma) {
  const float xf = px + kx, yf = py + ky;
  if (sigma < 0.5f) {                       // 10-bit bilinear interpolation, as upstream writes it
    int ix = (int)xf, iy = (int)yf;
    const int rx = (int)((xf - (float)ix) * 1024.0f), ry = (int)((yf - (float)iy) * 1024.0f);
    const int rx1 = 1024 - rx, ry1 = 1024 - ry;
    ix = min(max(ix, 0), w - 2); iy = min(max(iy, 0), h - 2);
    const uint8_t* p = img + (size_t)iy * pitch + ix;
    unsigned v = (unsigned)(rx1 * ry1) * (unsigned)p[0];
    v += (unsigned)(rx * ry1) * (unsigned)p[1];
    v += (unsigned)(rx * ry) * (unsigned)p[pitch + 1];
    v += (unsigned)(rx1 * ry) * (unsigned)p[pitch];
    v += 2u * 1024u * 1024u;
    return (int)(uint8_t)(v / (4u * 1024u * 1024u));
  }
  int xl = (int)((double)(xf - sigma) + 0.5), yt = (int)((double)(yf - sigma) + 0.5);
  int xr = (int)((double)(xf + sigma) + 1.5), yb = (int)((double)(yf + sigma) + 1.5);
  xl = min(max(xl, 0), w - 1); yt = min(max(yt, 0), h - 1);
  xr = min(max(xr, xl + 1), w); yb = min(max(yb, yt + 1), h);
  const size_t w1 = (size_t)(w + 1);
  const int v = S[yb * w1 + xr] - S[yb * w1 + xl] + S[yt * w1 + xl] - S[yt * w1 + xr];
  const int area = (xr - xl) * (yb - yt);
  return (int)(uint8_t)((v + area / 2) / area);
}

__global__ void __launch_bounds__(256)
k_freak_points(const uint8_t* __restrict__ img, int pitch, const int32_t* __restrict__ S, int w, int h,
               const sf_keypoint* __restrict__ kpts, const float* __restrict__ right_x, const uint8_t* __restrict__ status, int n,
               SfFreakTables T, ExtractCam cam, sf_keypoint* __restrict__ kpts_out, uint8_t* __restrict__ desc_tmp,
               float* __restrict__ xyz_tmp, uint8_t* __restrict__ keep, ExtractBatch B) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (B.d_n) n = min(n, B.d_n[blockIdx.y]);
  if (i >= n) return;                       // (per wavefront: everything below runs with all 64 lanes)
  {
    const size_t o = (size_t)blockIdx.y * B.per_image;
    img += blockIdx.y * B.img_stride;
    S += blockIdx.y * B.s_stride;
    kpts += o; kpts_out += o;
    if (right_x) right_x += o;
    if (status) status += o;
    desc_tmp += o * FREAK_BYTES; xyz_tmp += 3 * o; keep += o;
  }
  sf_keypoint k = kpts[i];
  // the scale index: one lane, float64 log rounded to float once; a size that is no positive number gives scale 0
  int idx = T.fixed_idx;
  if (T.scale_normalized) {
    if (lane == 0) {
      const float l = (float)log((double)(k.size / 7.0f));
      const double v = (double)(l * T.size_cst) + 0.5;
      idx = v > 0.0 ? (v < 63.0 ? (int)v : 63) : 0;
    }
    idx = __builtin_amdgcn_readfirstlane(idx);
  }
  const int P = T.sizes[idx];
  // (upstream drops on x <= P || ...; the positive form drops a NaN position as well)
  const bool inside = k.x > (float)P && k.y > (float)P && k.x < (float)(w - P) && k.y < (float)(h - P);
  if (inside) {
    const float* pat = T.pattern + (size_t)idx * FREAK_ORIENTATIONS * FREAK_POINTS * 3;
    int v = 0, t = 0;
    float angle = 0.0f;
    if (T.orientation_normalized) {
      if (lane < FREAK_POINTS) {
        const float* q = pat + 3 * lane;    // orientation 0
        v = freak_mean(img, pitch, S, w, h, k.x, k.y, q[0], q[1], q[2]);
      }
      int4 op = make_int4(0, 0, 0, 0);
      if (lane < FREAK_ORIENT_PAIRS) op = reinterpret_cast<const int4*>(T.orient)[lane];
      const int delta = __shfl(v, op.x) - __shfl(v, op.y);
      int d0 = delta * op.z / 2048, d1 = delta * op.w / 2048;   // (truncating, term by term; zero weights beyond lane 44)
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        d0 += __shfl_xor(d0, off);
        d1 += __shfl_xor(d1, off);
      }
      if (lane == 0) {
        angle = (float)(atan2((double)d1, (double)d0) * (180.0 / 3.1415926535897932384626433832795));
        const double s = (double)(256.0f * angle) * (1 / 360.0);
        t = angle < 0.0f ? (int)(s - 0.5) : (int)(s + 0.5);
        if (t < 0) t += FREAK_ORIENTATIONS;
        if (t >= FREAK_ORIENTATIONS) t -= FREAK_ORIENTATIONS;
      }
      t = __builtin_amdgcn_readfirstlane(t) & (FREAK_ORIENTATIONS - 1);
      angle = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(angle)));
    }
    k.angle = angle;
    v = 0;
    if (lane < FREAK_POINTS) {
      const float* q = pat + ((size_t)t * FREAK_POINTS + lane) * 3;
      v = freak_mean(img, pitch, S, w, h, k.x, k.y, q[0], q[1], q[2]);
    }
    const uint4 pr = reinterpret_cast<const uint4*>(T.pairs)[lane];   // byte `lane`: bit r = pair {i, j} at bytes 2r, 2r + 1
    const unsigned word[4] = {pr.x, pr.y, pr.z, pr.w};
    unsigned byte = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const unsigned ij = word[r >> 1] >> (16 * (r & 1));
      byte |= (unsigned)(__shfl(v, (int)(ij & 255u)) >= __shfl(v, (int)((ij >> 8) & 255u))) << r;
    }
    desc_tmp[(size_t)i * FREAK_BYTES + lane] = (uint8_t)byte;
  }
  if (lane != 0) return;
  kpts_out[i] = k;
  extract_point(k, i, inside, right_x, status, cam, xyz_tmp, keep);
}

// the receptive fields' rings, outer to inner: points per ring, radius, sigma (in units of the pattern scale)
struct FreakRings {
  int n[8];
  double radius[8], sigma[8];
};

FreakRings freak_rings() {
  FreakRings R = {{6, 6, 6, 6, 6, 6, 6, 1}, {}, {}};
  const double bigR = 2.0 / 3.0, smallR = 2.0 / 24.0, unit = (bigR - smallR) / 21.0;
  const double radius[8] = {bigR, bigR - 6 * unit, bigR - 11 * unit, bigR - 15 * unit, bigR - 18 * unit, bigR - 20 * unit, smallR, 0.0};
  for (int i = 0; i < 8; ++i) {
    R.radius[i] = radius[i];
    R.sigma[i] = radius[i < 7 ? i : 6] / 2.0;
  }
  return R;
}

bool freak_params_valid(const sf_freak_params& p) {
  return (p.orientation_normalized == 0 || p.orientation_normalized == 1) && (p.scale_normalized == 0 || p.scale_normalized == 1) &&
         p.pattern_scale > 0.0f && p.pattern_scale <= 64.0f && p.n_octaves >= 1 && p.n_octaves <= 8;
}

}  // namespace

extern "C" void sf_freak_defaults(sf_freak_params* p) {
  if (!p) return;
  p->orientation_normalized = 1;   // FREAK/OrientationNormalized [upstream rtabmap Parameters.h]
  p->scale_normalized = 1;         // FREAK/ScaleNormalized
  p->pattern_scale = 22.0f;        // FREAK/PatternScale
  p->n_octaves = 4;                // FREAK/NOctaves
}

// FREAK::buildPattern's lookup table: float64 arithmetic in upstream's order, every value rounded to float once
extern "C" int sf_freak_build_pattern(const sf_freak_params* given, float* table, int32_t* sizes) {
  sf_freak_params p;
  if (given) p = *given; else sf_freak_defaults(&p);
  if (!freak_params_valid(p)) return SF_EINVAL;
  const double pi = 3.1415926535897932384626433832795;
  const FreakRings R = freak_rings();
  const double pattern_scale = (double)p.pattern_scale;
  const double scale_step = std::pow(2.0, (double)p.n_octaves / FREAK_SCALES);
  for (int s = 0; s < FREAK_SCALES; ++s) {
    const double f = std::pow(scale_step, (double)s);
    if (sizes) {
      int size = 0;
      for (int i = 0; i < 8; ++i) size = std::max(size, (int)std::ceil((R.radius[i] + R.sigma[i]) * f * pattern_scale) + 1);
      sizes[s] = size;
    }
    if (!table) continue;
    for (int o = 0; o < FREAK_ORIENTATIONS; ++o) {
      const double theta = (double)o * 2 * pi / (double)FREAK_ORIENTATIONS;
      float* q = table + ((size_t)s * FREAK_ORIENTATIONS + o) * FREAK_POINTS * 3;
      for (int i = 0; i < 8; ++i)
        for (int k = 0; k < R.n[i]; ++k, q += 3) {
          const double beta = pi / R.n[i] * (i % 2);
          const double alpha = (double)k * 2 * pi / (double)R.n[i] + beta + theta;
          q[0] = (float)(R.radius[i] * std::cos(alpha) * f * pattern_scale);
          q[1] = (float)(R.radius[i] * std::sin(alpha) * f * pattern_scale);
          q[2] = (float)(R.sigma[i] * f * pattern_scale);
        }
    }
  }
  return SF_OK;
}

// The 45 orientation pairs and their weights, from the float points of scale 0 / orientation 0
void sf_freak_orientation_table(const float* pattern, int32_t* orient) {
  static const int base[9][2] = {{0, 3}, {1, 4}, {2, 5}, {0, 2}, {1, 3}, {2, 4}, {3, 5}, {4, 0}, {5, 1}};
  static const int inner[9][2] = {{24, 27}, {25, 28}, {26, 29}, {30, 33}, {31, 34}, {32, 35}, {36, 39}, {37, 40}, {38, 41}};
  for (int m = 0; m < FREAK_ORIENT_PAIRS; ++m) {
    const int i = m < 36 ? base[m % 9][0] + 6 * (m / 9) : inner[m - 36][0];
    const int j = m < 36 ? base[m % 9][1] + 6 * (m / 9) : inner[m - 36][1];
    const float dx = pattern[3 * i] - pattern[3 * j], dy = pattern[3 * i + 1] - pattern[3 * j + 1];
    const float nsq = dx * dx + dy * dy;
    orient[4 * m] = i;
    orient[4 * m + 1] = j;
    orient[4 * m + 2] = (int)((double)(dx / nsq) * 4096.0 + 0.5);
    orient[4 * m + 3] = (int)((double)(dy / nsq) * 4096.0 + 0.5);
  }
}

// Pair c = 128 q + 16 r + u is bit r of byte 16 q + 15 - u (upstream's SSE order): the kernel's table holds, for every
// byte, the {i, j} of its eight bits.  selected[c] indexes the enumeration for i in 1..42: for j in 0..i-1
void sf_freak_bit_table(const int32_t* selected, uint8_t* table) {
  uint8_t all[FREAK_ALL_PAIRS][2];
  int e = 0;
  for (int i = 1; i < FREAK_POINTS; ++i)
    for (int j = 0; j < i; ++j, ++e) { all[e][0] = (uint8_t)i; all[e][1] = (uint8_t)j; }
  for (int c = 0; c < FREAK_PAIRS; ++c) {
    const int q = c >> 7, r = (c >> 4) & 7, u = c & 15;
    uint8_t* d = table + ((size_t)(16 * q + 15 - u) * 8 + r) * 2;
    d[0] = all[selected[c]][0];
    d[1] = all[selected[c]][1];
  }
}

// Default selection of a fresh handle -- NOT OpenCV's FREAK_DEF_PAIRS: the first 512 values of a Fisher-Yates shuffle of
// 0 .. 902 driven by cv::RNG's multiply-with-carry step (as sf_orb_default_pattern) from the seed 0x46524B21
extern "C" void sf_freak_default_pairs(int32_t* selected) {
  if (!selected) return;
  uint64_t s = 0x46524B21u;
  auto next = [&]() {
    s = (uint64_t)(uint32_t)s * 4164903690ull + (s >> 32);
    return (uint32_t)s;
  };
  int32_t a[FREAK_ALL_PAIRS];
  for (int k = 0; k < FREAK_ALL_PAIRS; ++k) a[k] = k;
  for (int k = 0; k < FREAK_PAIRS; ++k) {
    const int r = k + (int)(next() % (uint32_t)(FREAK_ALL_PAIRS - k));
    std::swap(a[k], a[r]);
    selected[k] = a[k];
  }
}

// k_freak_points for sf_launch_extract_batch (k_extract.hip): S is the batch's integral images, B its layout
void sf_launch_freak_points(sf_context* c, const uint8_t* d_left, int pitch, const int32_t* S, int width, int height,
                            const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status, int n, int n_img,
                            const SfFreakTables& T, const ExtractCam& cam, sf_keypoint* d_kpts_angle, uint8_t* desc_tmp,
                            float* xyz_tmp, uint8_t* keep, const ExtractBatch& B) {
  hipLaunchKernelGGL(k_freak_points, dim3((unsigned)((n + 3) / 4), n_img), dim3(256), 0, c->stream, d_left, pitch, S, width, height,
                     d_kpts, d_right_x, d_status, n, T, cam, d_kpts_angle, desc_tmp, xyz_tmp, keep, B);
}
