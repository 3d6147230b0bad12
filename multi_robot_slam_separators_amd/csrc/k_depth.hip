// k_depth.hip -- RGB-D keyframes: what rtabmap does with a registered depth image where a stereo pair has a right image.
//   k_depth_mask    the detector mask Feature2D::generateKeypoints makes of the depth image (Vis/DepthAsMask): per pixel
//                   value = the depth in metres (u16 millimetres: (float)v * 0.001f for 0 < v < 65535, else 0; float32: the
//                   float itself), mask = 255 iff value > min_depth && (max_depth == 0 || value <= max_depth), NaN compares
//                   false.  Four pixels of a row per thread (one 8- or 16-byte load, one 4-byte store where the planes are
//                   aligned), all images of a batch in one launch (blockIdx.z).
//   k_depth_interp  util2d::interpolate(depth, factor, 0.1f): a decimated depth image enlarged by an integer factor, in its
//                   own format (the rule: include/sepfinder.h, restated in tests/depth_interp_ref.py).  Four output pixels
//                   of a row per thread, each the last valid one of the at most four cells that cover it: the sequential
//                   loops' result without their order, every cell tested once per thread.  factor 1 copies.  k_depth_interp_mask is the same
//                   grid straight to the mask of the enlarged image, which is never in memory.
//   k_depth_points  util3d::generateKeypoints3DDepth -> projectDepthTo3D(smoothing = true) -> util2d::getDepth(depthErrorRatio
//                   0.02, estWithNeighborsIfNull false) for one keypoint per thread (blockIdx.y = image, the count read on the
//                   device through ExtractBatch::d_n): the depth at the rounded pixel, smoothed over the 3 x 3 neighbours
//                   within 2 % of it, projected with the left camera, filtered by Vis/MinDepth / Vis/MaxDepth, moved by
//                   localTransform -- extract_point's place in a depth keyframe (sf_extract_device.hpp).  A depth image
//                   smaller than the image (dw x dh) is read at the keypoint scaled by rx = 1 / (width / dw) and ry, with
//                   the camera scaled alike; at the image's size both are 1.0f and every product is its operand.
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

// ---- util2d::interpolate -------------------------------------------------------------------------------------------------
// a sample as the cell test reads it: its raw value (uint16: millimetres), 0 = absent (uint16 0 and 65535; float32 <= 0, NaN, inf)
template <bool F32>
__device__ __forceinline__ float interp_sample(const uint8_t* __restrict__ row, int a) {
  if (F32) {
    const float v = ((const float*)row)[a];
    return (isfinite(v) && v > 0.0f) ? v : 0.0f;
  }
  const unsigned v = ((const uint16_t*)row)[a];
  return (v > 0u && v < 65535u) ? (float)v : 0.0f;
}

// The cell test and the value in one place.  Cell (a, b) of the dw x dh image `img` reads the samples (a - 1 .. a, b - 1 .. b);
// ok: inside the image, its four corners present and within a tenth of their mean of each other.  What the value needs of it:
// the left corners and the two slopes
struct InterpCell {
  float tl, bl, st, sb;
  bool ok;
};

template <bool F32>
__device__ __forceinline__ InterpCell interp_cell(const uint8_t* __restrict__ img, int pitch, int dw, int dh, float ff, int a, int b) {
  InterpCell c = {0.f, 0.f, 0.f, 0.f, false};
  if (a < 1 || a >= dw || b < 1 || b >= dh) return c;
  const uint8_t* r0 = img + (size_t)(b - 1) * pitch;
  const uint8_t* r1 = r0 + pitch;
  const float tl = interp_sample<F32>(r0, a - 1), tr = interp_sample<F32>(r0, a);
  const float bl = interp_sample<F32>(r1, a - 1), br = interp_sample<F32>(r1, a);
  if (!(tl > 0.0f && tr > 0.0f && bl > 0.0f && br > 0.0f)) return c;
  const float e = 0.1f * (((tl + tr) + bl) + br) / 4.0f;
  if (!(fabsf(tl - tr) <= e && fabsf(tl - bl) <= e && fabsf(tl - br) <= e && fabsf(tr - bl) <= e && fabsf(tr - br) <= e &&
        fabsf(bl - br) <= e))
    return c;
  c.tl = tl; c.bl = bl; c.st = (tr - tl) / ff; c.sb = (br - bl) / ff; c.ok = true;
  return c;
}

// a valid cell's pixel (p, q), both in 0 .. f
__device__ __forceinline__ float interp_value(const InterpCell& c, float ff, int p, int q) {
  const float top = c.tl + c.st * (float)p, bot = c.bl + c.sb * (float)p;
  return top + ((bot - top) / ff) * (float)q;
}

// what the enlarged uint16 image holds of a value: (uint16_t)(int)value
__device__ __forceinline__ unsigned interp_mm(float value) { return (unsigned)(int)value & 0xFFFFu; }

// MASK: the uint8 mask of the enlarged image (min_depth, max_depth: k_depth_mask's rule) in place of the image itself
template <bool F32, bool MASK>
__global__ void __launch_bounds__(256)
k_depth_interp(const uint8_t* __restrict__ depth, int dw, int dh, int pitch, size_t stride, int f, float min_depth, float max_depth,
               uint8_t* __restrict__ out, int out_pitch, size_t out_stride) {
  const int w = dw * f, h = dh * f;
  const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  depth += blockIdx.z * stride;
  out += blockIdx.z * out_stride;
  constexpr int ELEM = MASK ? 1 : F32 ? 4 : 2;
  uint8_t* dst = out + (size_t)y * out_pitch + (size_t)x * ELEM;
  const bool whole = x + 4 <= w;
  const bool wide = whole && (((uintptr_t)out | (uintptr_t)out_pitch) & (uintptr_t)(4 * ELEM - 1)) == 0u;
  if (f == 1) {                                            // (the copy: no cell, every bit as it is)
    const uint8_t* src = depth + (size_t)y * pitch;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < w) {
        if (MASK) dst[j] = depth_mask_of(F32 ? ((const float*)src)[x + j] : depth_of_mm(((const uint16_t*)src)[x + j]), min_depth, max_depth);
        else if (F32) ((uint32_t*)dst)[j] = ((const uint32_t*)src)[x + j];
        else ((uint16_t*)dst)[j] = ((const uint16_t*)src)[x + j];
      }
    return;
  }
  // Pixel (x, y) holds the last valid cell, rows outer and columns inner, among those that cover it: column a = x / f + 1 at
  // p = x % f and, on a cell's left edge (p = 0, x > 0), a = x / f at p = f; rows alike.  The thread walks its columns with
  // the cells of the row b = y / f + 1 (hi) and, on a cell's top edge, of b = y / f (lo): `cur` at a = xb + 1, `prev` at a =
  // xb -- every cell is tested once, all of them inside the 3 x 3 samples around a pixel
  const float ff = (float)f;
  const InterpCell none = {0.f, 0.f, 0.f, 0.f, false};
  const int yb = y / f, q = y - yb * f;
  const bool top_edge = q == 0 && yb > 0;
  int xb = x / f, p = x - xb * f;
  InterpCell hi_cur = interp_cell<F32>(depth, pitch, dw, dh, ff, xb + 1, yb + 1);
  InterpCell lo_cur = top_edge ? interp_cell<F32>(depth, pitch, dw, dh, ff, xb + 1, yb) : none;
  InterpCell hi_prev = p == 0 ? interp_cell<F32>(depth, pitch, dw, dh, ff, xb, yb + 1) : none;
  InterpCell lo_prev = p == 0 && top_edge ? interp_cell<F32>(depth, pitch, dw, dh, ff, xb, yb) : none;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool left_edge = p == 0;                         // (a = xb = 0 is no cell: interp_cell)
    if (hi_cur.ok) v[j] = interp_value(hi_cur, ff, p, q);
    else if (left_edge && hi_prev.ok) v[j] = interp_value(hi_prev, ff, f, q);
    else if (lo_cur.ok) v[j] = interp_value(lo_cur, ff, p, f);
    else if (left_edge && lo_prev.ok) v[j] = interp_value(lo_prev, ff, f, f);
    if (++p == f && j < 3) {
      p = 0; ++xb;
      hi_prev = hi_cur; lo_prev = lo_cur;
      hi_cur = interp_cell<F32>(depth, pitch, dw, dh, ff, xb + 1, yb + 1);
      lo_cur = top_edge ? interp_cell<F32>(depth, pitch, dw, dh, ff, xb + 1, yb) : none;
    }
  }
  if (MASK) {
    uint8_t m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = depth_mask_of(F32 ? v[j] : depth_of_mm(interp_mm(v[j])), min_depth, max_depth);
    if (wide) {
      *(unsigned*)dst = (unsigned)m[0] | ((unsigned)m[1] << 8) | ((unsigned)m[2] << 16) | ((unsigned)m[3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < w) dst[j] = m[j];
    }
  } else if (F32) {
    if (wide) {
      *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < w) ((float*)dst)[j] = v[j];
    }
  } else {
    if (wide) {
      *(uint2*)dst = make_uint2(interp_mm(v[0]) | (interp_mm(v[1]) << 16), interp_mm(v[2]) | (interp_mm(v[3]) << 16));
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < w) ((uint16_t*)dst)[j] = (uint16_t)interp_mm(v[j]);
    }
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
k_depth_points(const uint8_t* __restrict__ depth, int format, int pitch, size_t stride, int w, int h, float rx, float ry,
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
  const float x = kpts[i].x * rx, y = kpts[i].y * ry;      // (w x h: the depth image's size, the keypoint on it)
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
    const float cxs = cam.cx * rx, cys = cam.cy * ry;
    const float cx = cxs > 0.0f ? cxs : (float)(w / 2) - 0.5f;
    const float cy = cys > 0.0f ? cys : (float)(h / 2) - 0.5f;
    const float px = (x - cx) * z / (cam.fx * rx), py = (y - cy) * z / (cam.fy * ry);
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
  const int dw = depth.w ? depth.w : width, dh = depth.h ? depth.h : height;
  if (dw != width || dh != height) {                       // a decimated depth image: the mask of its enlargement, fused
    const int f = sf_depth_interpolation_factor(width, height, dw, dh);
    if (f < 2) return sf_fail(c, SF_EINVAL, "a %d x %d depth image makes no mask of %d x %d pixels", dw, dh, width, height);
    if (depth.format == SF_DEPTH_F32_M)
      hipLaunchKernelGGL((k_depth_interp<true, true>), grid, block, 0, c->stream, (const uint8_t*)depth.p, dw, dh, depth.pitch,
                         depth.stride, f, min_depth, max_depth, d_mask, mask_pitch, mask_stride);
    else
      hipLaunchKernelGGL((k_depth_interp<false, true>), grid, block, 0, c->stream, (const uint8_t*)depth.p, dw, dh, depth.pitch,
                         depth.stride, f, min_depth, max_depth, d_mask, mask_pitch, mask_stride);
    SF_HIP(c, hipGetLastError());
    return SF_OK;
  }
  if (depth.format == SF_DEPTH_F32_M)
    hipLaunchKernelGGL(k_depth_mask<true>, grid, block, 0, c->stream, (const uint8_t*)depth.p, width, height, depth.pitch,
                       depth.stride, min_depth, max_depth, d_mask, mask_pitch, mask_stride);
  else
    hipLaunchKernelGGL(k_depth_mask<false>, grid, block, 0, c->stream, (const uint8_t*)depth.p, width, height, depth.pitch,
                       depth.stride, min_depth, max_depth, d_mask, mask_pitch, mask_stride);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

int sf_launch_depth_interp(sf_context* c, const SfDepthIn& depth, int n_img, int factor, void* d_out, int out_pitch, size_t out_stride) {
  const int width = depth.w * factor, height = depth.h * factor;
  const dim3 grid((((width + 3) / 4) + 63) / 64, (height + 3) / 4, n_img), block(256);
  if (depth.format == SF_DEPTH_F32_M)
    hipLaunchKernelGGL((k_depth_interp<true, false>), grid, block, 0, c->stream, (const uint8_t*)depth.p, depth.w, depth.h, depth.pitch,
                       depth.stride, factor, 0.0f, 0.0f, (uint8_t*)d_out, out_pitch, out_stride);
  else
    hipLaunchKernelGGL((k_depth_interp<false, false>), grid, block, 0, c->stream, (const uint8_t*)depth.p, depth.w, depth.h, depth.pitch,
                       depth.stride, factor, 0.0f, 0.0f, (uint8_t*)d_out, out_pitch, out_stride);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

void sf_launch_depth_points(sf_context* c, const SfDepthIn& depth, int width, int height, const sf_keypoint* d_kpts, int n, int n_img,
                            const ExtractCam& cam, float* xyz_tmp, uint8_t* keep, uint8_t* valid, const ExtractBatch& B) {
  const int dw = depth.w ? depth.w : width, dh = depth.h ? depth.h : height;   // (its own size: sf_depth_set_size)
  const float rx = 1.0f / ((float)width / (float)dw), ry = 1.0f / ((float)height / (float)dh);
  hipLaunchKernelGGL(k_depth_points, dim3((n + 255) / 256, n_img), dim3(256), 0, c->stream, (const uint8_t*)depth.p, depth.format,
                     depth.pitch, depth.stride, dw, dh, rx, ry, d_kpts, n, cam, xyz_tmp, keep, valid, B);
}

int sf_launch_depth_points_only(sf_context* c, const SfDepthIn& depth, int width, int height, const sf_keypoint* d_kpts, int n,
                                const sf_stereo_camera* cam, float* d_xyz, uint8_t* d_valid) {
  ExtractBatch B;
  B.img_stride = 0; B.s_stride = 0; B.pyr_stride = 0; B.per_image = 0; B.d_n = nullptr;
  sf_launch_depth_points(c, depth, width, height, d_kpts, n, 1, sf_extract_cam(cam), d_xyz, nullptr, d_valid, B);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
