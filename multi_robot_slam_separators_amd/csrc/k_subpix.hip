// k_subpix.hip -- the two steps rtabmap's Feature2D::generateKeypoints puts around every detector (Vis/RoiRatios,
// Vis/SubPixWinSize / SubPixIterations / SubPixEps): the keypoints of a detector that ran on a sub-image are shifted back
// into the full image, and cv::cornerSubPix (OpenCV 3.2) refines them there, in place, before the stereo correspondence
// and the descriptors see them.  Neither upstream text is in the reference tree: the semantics are restated in
// tests/subpix_ref.py, and the kernel equals that restatement byte for byte -- every
// floating-point operation below is written in the restatement's order and the file is compiled without contraction.
//
//   k_corner_subpix   one wavefront (a workgroup of 64) per corner: corners with different iteration counts never
//                     diverge inside a wave, and every branch of the iteration is wave-uniform.  Per iteration:
//                       1. the (2 win + 3)^2 float patch of cv::getRectSubPix around the current position into LDS, one
//                          sample per lane and pass (4 byte loads, taps clamped to the image);
//                       2. per window sample the five products gxx, gxy, gyy, gxx px + gxy py, gxy px + gyy py in double,
//                          one sample per lane and pass, into LDS as [sample][5];
//                       3. lanes 0 .. 4 each add one column in raster order -- the order of upstream's double loop -- one
//                          ds_read_b64 and one v_add_f64 per sample; five shuffles hand the sums to every lane;
//                       4. every lane computes the same determinant, step and stop conditions.
//                     The Gaussian mask is v[i] * v[j] (a float product); the 2 win + 1 values v come from the host
//                     (exp in double, rounded once) as a kernel argument: the device never evaluates exp.
//                     blockIdx.y = image of a batch, the per-image corner count read on the device.  max_iters 0: only
//                     the ROI offset is applied (a ROI without refinement costs this one launch).
//                     LDS (dynamic): (2 win + 1)^2 * 40 + ((2 win + 3)^2 + 2 win + 1) * 4 bytes -- 2 312 at win 3, 42 920 at
//                     win 15 (the products, the patch, the taps).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sf_internal.hpp"

namespace {

constexpr int SUBPIX_MAX_WIN = 15;
struct SubpixTaps { float v[2 * SUBPIX_MAX_WIN + 1]; };   // v[k] = (float)exp(-t t), t = (float)(k - win) / win

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

__global__ void __launch_bounds__(64)
k_corner_subpix(const uint8_t* __restrict__ img, size_t img_stride, int w, int h, int pitch, sf_keypoint* __restrict__ kpts, int n,
                const int32_t* __restrict__ d_n, int kp_stride, float off_x, float off_y, int win, int max_iters, double eps2,
                SubpixTaps taps) {
  extern __shared__ __attribute__((aligned(16))) double s_terms[];   // [S][5] doubles, then the patch [PW][PW] floats
  if (d_n) n = min(d_n[blockIdx.y], kp_stride);
  if ((int)blockIdx.x >= n) return;
  const int lane = threadIdx.x;
  img += blockIdx.y * img_stride;
  sf_keypoint* kp = kpts + (size_t)blockIdx.y * kp_stride + blockIdx.x;
  const float x0 = kp->x + off_x, y0 = kp->y + off_y;
  float cx = x0, cy = y0;
  if (max_iters > 0) {
    const int PW = 2 * win + 3, WW = 2 * win + 1, S = WW * WW;
    float* patch = (float*)(s_terms + 5 * S);
    float* s_v = patch + PW * PW;                        // the taps, out of the argument block once
    if (lane < WW) s_v[lane] = taps.v[lane];
    const float half = (float)(win + 1);                 // (patch side - 1) * 0.5f
    int iter = 0;
    double err = 0.0;
    do {
      __syncthreads();
      const float qx = cx - half, qy = cy - half;
      const float fx = floorf(qx), fy = floorf(qy);
      const int ix = (int)fx, iy = (int)fy;
      const float a = qx - fx, b = qy - fy;
      const float a11 = (1.f - a) * (1.f - b), a12 = a * (1.f - b), a21 = (1.f - a) * b, a22 = a * b;
      for (int k = lane; k < PW * PW; k += 64) {
        const int r = k / PW, col = k - r * PW;
        const int xa = clampi(ix + col, w - 1), xb = clampi(ix + col + 1, w - 1);
        const uint8_t* p0 = img + (size_t)clampi(iy + r, h - 1) * pitch;
        const uint8_t* p1 = img + (size_t)clampi(iy + r + 1, h - 1) * pitch;
        patch[k] = (((float)p0[xa] * a11 + (float)p0[xb] * a12) + (float)p1[xa] * a21) + (float)p1[xb] * a22;
      }
      __syncthreads();
      for (int s = lane; s < S; s += 64) {
        const int i = s / WW, j = s - i * WW;
        const float* P = patch + (i + 1) * PW + (j + 1);
        const float gxf = P[1] - P[-1], gyf = P[PW] - P[-PW];
        const float mf = s_v[i] * s_v[j];
        const double m = mf, tgx = gxf, tgy = gyf;
        const double gxx = tgx * tgx * m, gxy = tgx * tgy * m, gyy = tgy * tgy * m;
        const double px = (double)(j - win), py = (double)(i - win);
        double* t = s_terms + 5 * s;
        t[0] = gxx; t[1] = gxy; t[2] = gyy;
        t[3] = gxx * px + gxy * py;
        t[4] = gxy * px + gyy * py;
      }
      __syncthreads();
      const int column = lane < 5 ? lane : 0;              // (lanes 5 .. 63 add column 0 again: no divergence)
      double acc = 0.0;
      for (int s = 0; s < S; ++s) acc += s_terms[5 * s + column];
      const double A = __shfl(acc, 0), B = __shfl(acc, 1), C = __shfl(acc, 2), bb1 = __shfl(acc, 3), bb2 = __shfl(acc, 4);
      const double det = A * C - B * B;
      if (fabs(det) <= 2.220446049250313e-16 * 2.220446049250313e-16) break;
      const double scale = 1.0 / det;
      const float nx = (float)((double)cx + C * scale * bb1 - B * scale * bb2);
      const float ny = (float)((double)cy - B * scale * bb1 + A * scale * bb2);
      err = (double)((nx - cx) * (nx - cx) + (ny - cy) * (ny - cy));
      cx = nx; cy = ny;
      if (cx < 0.f || cx >= (float)w || cy < 0.f || cy >= (float)h) break;
    } while (++iter < max_iters && err > eps2);
    if (fabsf(cx - x0) > (float)win || fabsf(cy - y0) > (float)win) { cx = x0; cy = y0; }
  }
  if (lane == 0) { kp->x = cx; kp->y = cy; }
}

}  // namespace

// In place on the handle's stream: keypoint i of image b (d_kpts + b * kp_stride; n of them, or min(d_n[b], kp_stride) read
// on the device) moves by (off_x, off_y) and, with win >= 1 and iterations >= 1, to cv::cornerSubPix's position on the
// image (width x height, images img_stride bytes apart).  The caller has checked win <= 15 and the image size.
int sf_launch_corner_subpix(sf_context* c, const uint8_t* d_images, size_t img_stride, int n_img, int width, int height, int pitch,
                            sf_keypoint* d_kpts, int n, const int32_t* d_n, int kp_stride, int off_x, int off_y, int win,
                            int iterations, float eps) {
  if (n <= 0 || n_img <= 0) return SF_OK;
  const bool refine = win > 0 && iterations > 0;
  SubpixTaps taps = {};
  size_t lds = 0;
  if (refine) {
    for (int k = 0; k <= 2 * win; ++k) {
      const float t = (float)(k - win) / win;
      taps.v[k] = (float)exp((double)(-t * t));
    }
    const size_t S = (size_t)(2 * win + 1) * (2 * win + 1), PP = (size_t)(2 * win + 3) * (2 * win + 3);
    lds = S * 5 * sizeof(double) + (PP + 2 * win + 1) * sizeof(float);
  }
  const double e = std::max((double)eps, 0.0);
  hipLaunchKernelGGL(k_corner_subpix, dim3(n, n_img), dim3(64), lds, c->stream, d_images, img_stride, width, height, pitch, d_kpts, n,
                     d_n, kp_stride, (float)off_x, (float)off_y, win, refine ? std::min(std::max(iterations, 1), 100) : 0, e * e, taps);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
