// k_depth.hip -- RGB-D keyframes: what rtabmap does with a registered depth image where a stereo pair has a right image.
//   k_depth_mask    the detector mask Feature2D::generateKeypoints makes of the depth image (Vis/DepthAsMask): per pixel
//                   value = the depth in metres (u16 millimetres: (float)v * 0.001f for 0 < v < 65535, else 0; float32: the
//                   float itself), mask = 255 iff value > min_depth && (max_depth == 0 || value <= max_depth), NaN compares
//                   false.  Four pixels of a row per thread (one 8- or 16-byte load, one 4-byte store where the planes are
//                   aligned), all images of a batch in one launch (blockIdx.z).
//   k_depth_points  util3d::generateKeypoints3DDepth -> projectDepthTo3D(smoothing = true) -> util2d::getDepth(depthErrorRatio
//                   0.02, estWithNeighborsIfNull false) for one keypoint per thread (blockIdx.y = image, the count read on the
//                   device through ExtractBatch::d_n): the depth at the rounded pixel, smoothed over the 3 x 3 neighbours
//                   within 2 % of it, projected with the left camera, filtered by Vis/MinDepth / Vis/MaxDepth, moved by
//                   localTransform -- extract_point's place in a depth keyframe (sf_extract_device.hpp).
// Neither upstream text is in the reference tree: the semantics are restated in tests/depth_ref.py (DESIGN.md section 3
// lists what the restatement decides) and the kernels equal it byte for byte: float32 in the order written, compiled with
// -ffp-contract=off.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_extract_device.hpp"

namespace {

__device__ __forceinline__ float depth_of_mm(unsigned v) { return (v > 0u && v < 65535u) ? (float)v * 0.001f : 0.0f; }

__device__ __forceinline__ uint8_t depth_mask_of(float value, float min_depth, float max_depth) {
  return (value > min_depth && (max_depth == 0.0f || value <= max_depth)) ? (uint8_t)255 : (uint8_t)0;
}

template <bool F32>
__global__ void __launch_bounds__(256)
k_depth_mask(const uint8_t* __restrict__ depth, int w, int h, int pitch, size_t stride, float min_depth, float max_depth,
             uint8_t* __restrict__ mask, int mask_pitch, size_t mask_stride) {
  const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  depth += blockIdx.z * stride;
  mask += blockIdx.z * mask_stride;
  constexpr int ELEM = F32 ? 4 : 2;
  const uint8_t* row = depth + (size_t)y * pitch;
  uint8_t* out = mask + (size_t)y * mask_pitch + x;
  // (the wide forms are chosen per image: uniform per workgroup but for the row's last, partial group of four)
  const bool whole = x + 4 <= w;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (whole && (((uintptr_t)depth | (uintptr_t)pitch) & (uintptr_t)(4 * ELEM - 1)) == 0u) {
    if (F32) {
      const float4 q = *(const float4*)(row + (size_t)x * 4);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      const ushort4 q = *(const ushort4*)(row + (size_t)x * 2);
      v[0] = depth_of_mm(q.x); v[1] = depth_of_mm(q.y); v[2] = depth_of_mm(q.z); v[3] = depth_of_mm(q.w);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < w) v[j] = F32 ? ((const float*)row)[x + j] : depth_of_mm(((const uint16_t*)row)[x + j]);
  }
  uint8_t m[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = depth_mask_of(v[j], min_depth, max_depth);
  if (whole && (((uintptr_t)mask | (uintptr_t)mask_pitch) & 3u) == 0u) {
    *(unsigned*)out = (unsigned)m[0] | ((unsigned)m[1] << 8) | ((unsigned)m[2] << 16) | ((unsigned)m[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < w) out[j] = m[j];
  }
}

// the depth in metres at pixel (u, v) of the image, u and v inside it
__device__ __forceinline__ float depth_at(const uint8_t* __restrict__ img, int format, int pitch, int u, int v) {
  const uint8_t* row = img + (size_t)v * pitch;
  return format == SF_DEPTH_F32_M ? ((const float*)row)[u] : depth_of_mm(((const uint16_t*)row)[u]);
}

// getDepth's pixel of a coordinate: (int)(x + 0.5f), x just inside the last column or row rounds back into it; -1 =
// outside the image.  The cast is made only where C defines it: a coordinate that is not finite, or whose x + 0.5f is
// not inside (-1, len + 1), is outside whatever the cast would give.
__device__ __forceinline__ int depth_pixel(float x, int len) {
  const float r = x + 0.5f;
  if (!(r > -1.0f && r < (float)(len + 1))) return -1;
  int u = (int)r;
  if (u == len && x < (float)len) u = len - 1;
  return u < len ? u : -1;
}

__global__ void __launch_bounds__(256)
k_depth_points(const uint8_t* __restrict__ depth, int format, int pitch, size_t stride, int w, int h,
               const sf_keypoint* __restrict__ kpts, int n, ExtractCam cam, float* __restrict__ xyz_tmp,
               uint8_t* __restrict__ keep, uint8_t* __restrict__ valid, ExtractBatch B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (B.d_n) n = min(n, B.d_n[blockIdx.y]);
  if (i >= n) return;
  {
    const size_t o = (size_t)blockIdx.y * B.per_image;
    depth += blockIdx.y * stride;
    kpts += o; xyz_tmp += 3 * o;
    if (keep) keep += o;
    if (valid) valid += o;
  }
  const float x = kpts[i].x, y = kpts[i].y;
  const float qnan = __int_as_float(0x7FC00000);
  float p0 = qnan, p1 = qnan, p2 = qnan;
  const int u = depth_pixel(x, w), v = depth_pixel(y, h);
  const float d = (u >= 0 && v >= 0) ? depth_at(depth, format, pitch, u, v) : 0.0f;
  if (d != 0.0f && isfinite(d)) {
    float sum_weights = 0.0f, sum_depths = 0.0f;
    const float err = 0.02f * d;
    const int u0 = max(u - 1, 0), u1 = min(u + 1, w - 1), v0 = max(v - 1, 0), v1 = min(v + 1, h - 1);
    for (int uu = u0; uu <= u1; ++uu)
      for (int vv = v0; vv <= v1; ++vv) {
        if (uu == u && vv == v) continue;
        float dn = depth_at(depth, format, pitch, uu, vv);
        if (dn != 0.0f && isfinite(dn) && fabsf(dn - d) < err) {
          if (uu == u || vv == v) { sum_weights = sum_weights + 2.0f; dn = dn * 2.0f; }
          else sum_weights = sum_weights + 1.0f;
          sum_depths = sum_depths + dn;
        }
      }
    const float z = (d * 4.0f + sum_depths) / (sum_weights + 4.0f);
    const float cx = cam.cx > 0.0f ? cam.cx : (float)(w / 2) - 0.5f;
    const float cy = cam.cy > 0.0f ? cam.cy : (float)(h / 2) - 0.5f;
    const float px = (x - cx) * z / cam.fx, py = (y - cy) * z / cam.fy;
    if (isfinite(z) && (cam.min_depth < 0.0f || z > cam.min_depth) && (cam.max_depth <= 0.0f || z <= cam.max_depth)) {
      if (cam.identity_local) {
        p0 = px; p1 = py; p2 = z;
      } else {
        p0 = ((cam.L[0] * px + cam.L[1] * py) + cam.L[2] * z) + cam.L[3];
        p1 = ((cam.L[4] * px + cam.L[5] * py) + cam.L[6] * z) + cam.L[7];
        p2 = ((cam.L[8] * px + cam.L[9] * py) + cam.L[10] * z) + cam.L[11];
      }
    }
  }
  xyz_tmp[3 * i] = p0; xyz_tmp[3 * i + 1] = p1; xyz_tmp[3 * i + 2] = p2;
  const bool finite = isfinite(p0) && isfinite(p1) && isfinite(p2);
  if (keep) keep[i] = (uint8_t)(keep[i] && (!cam.filter || finite));
  if (valid) valid[i] = (uint8_t)finite;
}

}  // namespace

int sf_launch_depth_mask(sf_context* c, const SfDepthIn& depth, int n_img, int width, int height, float min_depth, float max_depth,
                         uint8_t* d_mask, int mask_pitch, size_t mask_stride) {
  const dim3 grid((((width + 3) / 4) + 63) / 64, (height + 3) / 4, n_img), block(256);
  if (depth.format == SF_DEPTH_F32_M)
    hipLaunchKernelGGL(k_depth_mask<true>, grid, block, 0, c->stream, (const uint8_t*)depth.p, width, height, depth.pitch,
                       depth.stride, min_depth, max_depth, d_mask, mask_pitch, mask_stride);
  else
    hipLaunchKernelGGL(k_depth_mask<false>, grid, block, 0, c->stream, (const uint8_t*)depth.p, width, height, depth.pitch,
                       depth.stride, min_depth, max_depth, d_mask, mask_pitch, mask_stride);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

void sf_launch_depth_points(sf_context* c, const SfDepthIn& depth, int width, int height, const sf_keypoint* d_kpts, int n, int n_img,
                            const ExtractCam& cam, float* xyz_tmp, uint8_t* keep, uint8_t* valid, const ExtractBatch& B) {
  hipLaunchKernelGGL(k_depth_points, dim3((n + 255) / 256, n_img), dim3(256), 0, c->stream, (const uint8_t*)depth.p, depth.format,
                     depth.pitch, depth.stride, width, height, d_kpts, n, cam, xyz_tmp, keep, valid, B);
}

int sf_launch_depth_points_only(sf_context* c, const SfDepthIn& depth, int width, int height, const sf_keypoint* d_kpts, int n,
                                const sf_stereo_camera* cam, float* d_xyz, uint8_t* d_valid) {
  ExtractBatch B;
  B.img_stride = 0; B.s_stride = 0; B.pyr_stride = 0; B.per_image = 0; B.d_n = nullptr;
  sf_launch_depth_points(c, depth, width, height, d_kpts, n, 1, sf_extract_cam(cam), d_xyz, nullptr, d_valid, B);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
