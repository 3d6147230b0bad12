// k_stereo_bm.hip -- stereo correspondence of the corners by block matching: rtabmap's Stereo/OpticalFlow = false,
// Stereo::computeCorrespondences -> util2d::calcStereoCorrespondences [upstream rtabmap], the second implementation
// behind the Stereo/* group the reference forwards to its detector (myRegistrationVis.cpp:125).  A coarse-to-fine
// SSD / SAD window search along the row on the pyramid of the LK path (sf_lk_build_pyramid, k_lk.hip), then a bisection
// to a sub-pixel minimum.  Arithmetic and order are those of tests/stereo_bm_ref.py, which the tests compare with byte
// for byte (DESIGN.md section 3 item 17e lists what that restatement decides); compiled with -ffp-contract=off.
//
//   k_stereo_bm   one 64-lane workgroup per corner, grid (corners, images), all levels inside the kernel.  Per level the
//                 left window and the right strip (window rows x the columns every candidate touches) go to LDS once;
//                 lanes own disparity candidates (and loop when there are more than 64); scores are exact integer sums;
//                 the winner is the minimum of the packed key (score << 32 | candidate index) over the positive scores,
//                 so the earliest candidate wins a tie; the range update is wave-uniform scalar work.  A strip beyond
//                 BM_STRIP_CAP bytes (tall windows with a wide disparity range) is read from global memory instead.
//                 Sub-pixel stage: the left float patch sits in LDS; lanes own the window elements of BOTH probes of a
//                 bisection step and leave their terms in LDS; lanes 0 and 1 add one probe's terms each in raster order
//                 (the float32 sum the restatement fixes); the decisions are wave uniform.  The right image's taps come
//                 from global memory (the probe position walks, at most 0.5 px a step).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "sf_internal.hpp"

namespace {

constexpr int BM_STRIP_CAP = 32768;

__device__ __forceinline__ unsigned long long bm_wave_min(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, o));
  return v;
}

template <bool SSD>
__device__ __forceinline__ int bm_score(const unsigned char* __restrict__ lw, const unsigned char* __restrict__ r, int rpitch,
                                        int ww, int wh) {
  int s = 0;
  for (int v = 0; v < wh; ++v) {
    const unsigned char* a = lw + v * ww;
    const unsigned char* b = r + (size_t)v * rpitch;
    for (int u = 0; u < ww; ++u) {
      const int t = (int)a[u] - (int)b[u];
      s += SSD ? t * t : (t < 0 ? -t : t);
    }
  }
  return s;
}

// one element (ex, ey) of the ww x wh patch of cv::getRectSubPix centred on (cx, cy), taps clamped to the edge
__device__ __forceinline__ float bm_rect(const uint8_t* __restrict__ img, int w, int h, int pitch, float cx, float cy,
                                         float half_x, float half_y, int ex, int ey) {
  const float qx = cx - half_x, qy = cy - half_y;
  const float fx = floorf(qx), fy = floorf(qy);
  const float a = qx - fx, b = qy - fy;
  const float w00 = (1.f - a) * (1.f - b), w01 = a * (1.f - b), w10 = (1.f - a) * b, w11 = a * b;
  const int ix = (int)fx + ex, iy = (int)fy + ey;
  const int x0 = min(max(ix, 0), w - 1), x1 = min(max(ix + 1, 0), w - 1);
  const int y0 = min(max(iy, 0), h - 1), y1 = min(max(iy + 1, 0), h - 1);
  const uint8_t* r0 = img + (size_t)y0 * pitch;
  const uint8_t* r1 = img + (size_t)y1 * pitch;
  return (((float)r0[x0] * w00 + (float)r0[x1] * w01) + (float)r1[x0] * w10) + (float)r1[x1] * w11;
}

template <bool SSD>
__global__ __launch_bounds__(64) void k_stereo_bm(const LkLevels P, const sf_keypoint* __restrict__ kp, int n, int ww, int wh,
                                                  int iterations, int minD, int maxD, float min_disp, int strip_cap,
                                                  float* __restrict__ xy_out, uint8_t* __restrict__ st_out,
                                                  float* __restrict__ rx_out, float* __restrict__ sc_out) {
  extern __shared__ unsigned char bm_smem[];
  const int p = blockIdx.x;
  const int img = blockIdx.y;
  if (P.d_n) n = min(n, P.d_n[img]);
  if (p >= n) return;
  {
    const size_t o = (size_t)img * P.per_image;
    kp += o; xy_out += 2 * o; st_out += o;
    if (rx_out) rx_out += o;
    if (sc_out) sc_out += o;
  }
  const int lane = threadIdx.x;
  const int area = ww * wh;
  const int hw = (ww - 1) / 2, hh = (wh - 1) / 2;
  float* WL = reinterpret_cast<float*>(bm_smem);           // the left float patch of the sub-pixel stage
  float* terms = WL + area;                                // [2][area]: the terms of a step's two probes
  unsigned char* lwin = reinterpret_cast<unsigned char*>(terms + 2 * area);
  unsigned char* strip = lwin + ((area + 15) & ~15);

  const float kx = kp[p].x, ky = kp[p].y;
  // (not finite or beyond +-2^30: no level's window test passes)
  const bool usable = fabsf(kx) < 1073741824.f && fabsf(ky) < 1073741824.f;
  int tmin = minD, tmax = maxD, best = -1, best_score = -1;
  for (int level = usable ? P.n - 1 : -1; level >= 0; --level) {
    LkLevel L = P.v[level];
    {
      const size_t o = (size_t)img * (level == 0 ? P.stride0 : P.stride_pyr);
      L.l += o; L.r += o;
    }
    const int scale = 1 << level;
    const int cx = (int)(kx / (float)scale), cy = (int)(ky / (float)scale);
    best = -1; best_score = -1;
    int lmax = (-tmax) / scale;
    const int lmin = (-tmin) / scale;
    const int m = level == 0 ? 1 : 0;
    if (!(cx - hw - m >= 0 && cx + hw + m < L.w && cy - hh >= 0 && cy + hh < L.h)) continue;
    const int min_col = cx + lmax - hw - 1;
    if (min_col < 0) lmax -= min_col;
    const int ncand = lmin - lmax;                         // d = lmin, lmin - 1, ..., lmax + 1
    if (ncand <= 0) continue;
    // The pixels read: the left window is inside the image by the test above; the right columns are
    // [cx + lmax + 1 - hw, cx + lmin + hw], whose first is min_col + 2 >= 2 after the clamp and whose last is
    // <= cx + hw < L.w because tmin >= minD >= 0 makes lmin <= 0.
    const int sw = ncand + ww - 1;
    const int c0 = cx + lmax + 1 - hw;
    const uint8_t* lrow = L.l + (size_t)(cy - hh) * L.pitch + (cx - hw);
    const uint8_t* rrow = L.r + (size_t)(cy - hh) * L.pitch + c0;
    const bool staged = sw * wh <= strip_cap;
    __syncthreads();                                       // (the previous level's readers are done)
    for (int e = lane; e < area; e += 64) {
      const int yy = e / ww, xx = e - yy * ww;
      lwin[e] = lrow[(size_t)yy * L.pitch + xx];
    }
    if (staged)
      for (int e = lane; e < sw * wh; e += 64) {
        const int yy = e / sw, xx = e - yy * sw;
        strip[e] = rrow[(size_t)yy * L.pitch + xx];
      }
    __syncthreads();
    unsigned long long key = ~0ull;
    for (int oi = lane; oi < ncand; oi += 64) {
      const int col = ncand - 1 - oi;                      // candidate oi is d = lmin - oi: strip column d - lmax - 1
      const int s = staged ? bm_score<SSD>(lwin, strip + col, sw, ww, wh) : bm_score<SSD>(lwin, rrow + col, L.pitch, ww, wh);
      if (s > 0) key = min(key, ((unsigned long long)(unsigned)s << 32) | (unsigned)oi);
    }
    key = bm_wave_min(key);
    const unsigned k_lo = __builtin_amdgcn_readfirstlane((unsigned)key), k_hi = __builtin_amdgcn_readfirstlane((unsigned)(key >> 32));
    if (k_hi != 0xffffffffu) { best = (int)k_lo; best_score = (int)k_hi; }
    if (best >= 0 && level > 0) {
      int nmax = tmin + (best + 1) * scale;
      nmax += nmax % level;                                // (modulo the level NUMBER: upstream's quirk, kept)
      if (nmax > maxD) nmax = maxD;
      int nmin = tmin + (best - 1) * scale;
      nmin -= nmin % level;
      if (nmin < minD) nmin = minD;
      tmax = nmax; tmin = nmin;
    }
  }
  if (best < 0) {
    if (lane == 0) {
      xy_out[2 * p] = 0.f; xy_out[2 * p + 1] = 0.f;
      st_out[p] = 0;
      if (rx_out) rx_out[p] = 0.f;
      if (sc_out) sc_out[p] = -1.f;
    }
    return;
  }

  // sub-pixel stage on level 0, float32 in the order written
  LkLevel L = P.v[0];
  L.l += (size_t)img * P.stride0; L.r += (size_t)img * P.stride0;
  const float half_x = (float)(ww - 1) * 0.5f, half_y = (float)(wh - 1) * 0.5f;
  __syncthreads();
  for (int e = lane; e < area; e += 64) {
    const int yy = e / ww, xx = e - yy * ww;
    WL[e] = bm_rect(L.l, L.w, L.h, L.pitch, kx, ky, half_x, half_y, xx, yy);
  }
  __syncthreads();
  // score(xa), score(xb): the terms of both probes to LDS, then one lane per probe adds its terms in raster order
  auto probes = [&](float xa, float xb, float& va, float& vb) {
    for (int e = lane; e < 2 * area; e += 64) {
      const int second = e >= area ? 1 : 0;
      const int ee = e - second * area;
      const int yy = ee / ww, xx = ee - yy * ww;
      const float t = WL[ee] - bm_rect(L.r, L.w, L.h, L.pitch, second ? xb : xa, ky, half_x, half_y, xx, yy);
      terms[e] = SSD ? t * t : fabsf(t);
    }
    __syncthreads();
    float s = 0.f;
    if (lane < 2) {
      const float* q = terms + lane * area;
      for (int i = 0; i < area; ++i) s += q[i];
    }
    va = __shfl(s, 0); vb = __shfl(s, 1);
    __syncthreads();
  };
  const float d = (float)(-(tmin + best));
  float vc = (float)best_score;
  if (kx != (float)(int)kx) {                              // (a fractional x alone recomputes the start score: upstream, kept)
    float v0, unused;
    probes(kx + d, kx + d, v0, unused);
    vc = v0;
  }
  float xc = kx + d, step = 0.5f;
  bool reject = false;
  for (int it = 0; it < iterations; ++it) {
    const float x1 = xc - step, x2 = xc + step;
    float v1, v2;
    probes(x1, x2, v1, v2);
    const float prev = xc;
    if (v1 < vc && v1 < v2) { xc = x1; vc = v1; }
    else if (v2 < vc && v2 < v1) { xc = x2; vc = v2; }
    if (prev == xc) step = step / 2.f;
    if (kx - xc <= min_disp) { reject = true; break; }
  }
  if (lane == 0) {
    xy_out[2 * p] = xc; xy_out[2 * p + 1] = ky;
    st_out[p] = reject ? 0 : 1;
    if (rx_out) rx_out[p] = xc;
    if (sc_out) sc_out[p] = vc;
  }
}

}  // namespace

// The arguments of sf_launch_stereo_flow_batch (k_lk.hip); prm validated by the caller (sf_detect.hip, sf_keyframes.hip).
int sf_launch_stereo_bm_batch(sf_context* c, const uint8_t* d_left, const uint8_t* d_right, size_t img_stride, int n_img,
                              int width, int height, int pitch, const sf_keypoint* d_kpts, int n, const int32_t* d_n,
                              const sf_stereo_flow_params* prm, int ssd, float* d_right_xy, uint8_t* d_status,
                              float* d_right_x, float* d_score) {
  const int ww = prm->win_width, wh = prm->win_height;
  LkLevels P;
  int rc;
  if ((rc = sf_lk_build_pyramid(c, d_left, d_right, img_stride, n_img, width, height, pitch, ww, wh, prm->max_level, n, d_n, &P)) != SF_OK)
    return rc;
  const int minD = (int)std::floor(prm->min_disparity), maxD = (int)std::floor(prm->max_disparity);
  const int iterations = std::min(std::max(prm->iterations, 0), 100);
  const int area = ww * wh;
  // a level has at most maxD - minD + 1 candidates, its strip that many columns + ww - 1
  const long long strip_need = (long long)wh * (maxD - minD + ww);
  const int strip_cap = (int)std::min<long long>((strip_need + 15) & ~15ll, BM_STRIP_CAP);
  const size_t smem = (size_t)area * 12 + (size_t)((area + 15) & ~15) + (size_t)strip_cap;
  if (ssd)
    hipLaunchKernelGGL(k_stereo_bm<true>, dim3(n, n_img), dim3(64), smem, c->stream, P, d_kpts, n, ww, wh, iterations, minD, maxD,
                       prm->min_disparity, strip_cap, d_right_xy, d_status, d_right_x, d_score);
  else
    hipLaunchKernelGGL(k_stereo_bm<false>, dim3(n, n_img), dim3(64), smem, c->stream, P, d_kpts, n, ww, wh, iterations, minD, maxD,
                       prm->min_disparity, strip_cap, d_right_xy, d_status, d_right_x, d_score);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
