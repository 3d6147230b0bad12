// k_depth_register.hip -- a depth image measured in the depth (IR) camera's frame registered to the colour camera: upstream
// rtabmap's util2d::registerDepth + util2d::fillRegisteredDepthHoles(fillDoubleHoles = false), a forward scatter with a z-test.
// Neither function is in the reference tree: the rule is written out in include/sepfinder.h ("depth registration"), restated in
// tests/depth_register_ref.py (DESIGN.md section 3 lists what the restatement decides) and the kernels equal it byte for byte:
// float32 in the order written, compiled with -ffp-contract=off.  A minimum does not depend on the order of arrival, so the
// z-buffer is one uint32 key per output pixel under an atomic minimum (uint16: the millimetres; float32: the bits of a positive
// float, whose unsigned order is the float order), 0xFFFFFFFF = nothing landed.
//
//   k_depth_register_scatter<F32>  blockIdx.z = image.  A thread takes four consecutive depth pixels of a row (one 8- or 16-byte
//                  load where base and pitch allow, elements otherwise), a wavefront 256 consecutive depth pixels of a row: under
//                  a near-identity rotation its atomics fall into one or two short row segments of the key plane.  The
//                  registration block is a kernel argument (scalar registers).  Every surviving point issues one 32-bit atomic
//                  minimum at agent scope whose result is not read (the form without a return value).
//   k_depth_register_resolve<F32, FILL>  four output pixels of a row per thread: the keys of rows y - 1, y and y + 1 through the
//                  cache, 0xFFFFFFFF -> 0, the hole filling (FILL bit 0: the vertical pair, bit 1: the horizontal pair; out of
//                  place: it reads unfilled values only, and the unfilled image is never in memory), one 8- or 16-byte store
//                  where base and pitch allow.
//   k_depth_fill_holes<F32, FILL>  the same body reading an image instead of keys (sf_depth_fill_holes_device).
// No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_internal.hpp"

namespace {

constexpr unsigned KEY_EMPTY = 0xFFFFFFFFu;

// ---- the scatter ---------------------------------------------------------------------------------------------------------
// depth pixel (x, y) holding the sample `raw` (uint16: the value; float32: the bits): projected, tested and keyed as
// include/sepfinder.h writes it, then the minimum of its key plane's pixel
template <bool F32>
__device__ __forceinline__ void register_point(const SfDepthRegister& R, int x, int y, unsigned raw, unsigned* __restrict__ keys) {
  float dz;
  if (F32) {
    dz = __uint_as_float(raw);
    if (!(isfinite(dz) && dz > 0.0f)) return;
  } else {
    if (!(raw > 0u && raw < 65535u)) return;
    dz = (float)raw * 0.001f;
  }
  const float X = (((float)x - R.cx) * dz) / R.fx;
  const float Y = (((float)y - R.cy) * dz) / R.fy;
  const float px = ((R.T[0] * X + R.T[1] * Y) + R.T[2] * dz) + R.T[3];
  const float py = ((R.T[4] * X + R.T[5] * Y) + R.T[6] * dz) + R.T[7];
  const float pz = ((R.T[8] * X + R.T[9] * Y) + R.T[10] * dz) + R.T[11];
  if (!(pz > 0.0f)) return;
  const float iz = 1.0f / pz;
  const float u = (R.rfx * px) * iz + R.rcx;
  const float v = (R.rfy * py) * iz + R.rcy;
  if (!(u > -1.0f && u < (float)R.W && v > -1.0f && v < (float)R.H)) return;     // (NaN compares false)
  const int dx = (int)u, dy = (int)v;                      // truncation: (-1, 0) lands in column / row 0; both inside the plane
  unsigned k;
  if (F32) {
    k = __float_as_uint(pz);
  } else {
    const float m = pz * 1000.0f;
    if (!(m < 65535.0f)) return;
    k = (unsigned)(int)m;
    if (k == 0u) return;
  }
  (void)__hip_atomic_fetch_min(keys + (size_t)dy * R.W + dx, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool F32>
__global__ void __launch_bounds__(256)
k_depth_register_scatter(const uint8_t* __restrict__ depth, int pitch, size_t stride, const SfDepthRegister R,
                         unsigned* __restrict__ keys) {
  const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= R.dw || y >= R.dh) return;
  depth += blockIdx.z * stride;
  keys += (size_t)blockIdx.z * R.W * R.H;
  constexpr int ELEM = F32 ? 4 : 2;
  const uint8_t* row = depth + (size_t)y * pitch;
  unsigned raw[4] = {0u, 0u, 0u, 0u};                       // (0 is absent in both formats)
  if (x + 4 <= R.dw && (((uintptr_t)depth | (uintptr_t)pitch) & (uintptr_t)(4 * ELEM - 1)) == 0u) {
    if (F32) {
      const uint4 q = *(const uint4*)(row + (size_t)x * 4);
      raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
    } else {
      const ushort4 q = *(const ushort4*)(row + (size_t)x * 2);
      raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < R.dw) raw[j] = F32 ? ((const uint32_t*)row)[x + j] : (unsigned)((const uint16_t*)row)[x + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) register_point<F32>(R, x + j, y, raw[j], keys);
}

// ---- the resolve and the fill --------------------------------------------------------------------------------------------
// One pair of fillRegisteredDepthHoles on raw values (uint16: the value; float32: the bits): whether (a, c) sets the pixel
// that holds b, and to what
// KEEP THIS STRAIGHT-LINE: every condition is computed, the value is always written, and the caller picks with selects.
// A form with early returns, called as `if (vertical pair sets) .. else if (horizontal pair sets) ..`, gave wrong bytes on
// gfx950 with FILL = 3 only: every value that the horizontal pair alone replaces (b != 0, far) stayed, while holes (b == 0)
// were filled, FILL = 1 and FILL = 2 were right, and the same source built for the host was right in all four.  The source
// holds no undefined behaviour that would explain it, so it is held to be the compiler's; what guards against its return
// are the both-flags byte comparisons of tests/test_gpu_depth_register.py, whose scenes all hold such values.
template <bool F32>
__device__ __forceinline__ bool fill_pair(unsigned a, unsigned b, unsigned c, unsigned* out) {
  if (F32) {
    const float fa = __uint_as_float(a), fb = __uint_as_float(b), fc = __uint_as_float(c);
    const float m = (fa + fc) / 2.0f;
    const float e = 0.01f * m;
    const bool both = fa != 0.0f && fc != 0.0f;
    const bool close = fabsf(fa - fc) <= e;
    const bool far = fb > fa + e && fb > fc + e;
    *out = __float_as_uint(m);
    return both && close && (fb == 0.0f || far);
  }
  const int ia = (int)a, ic = (int)c;
  const int m = (ia + ic) / 2;
  const float e = 0.01f * (float)m;
  const float fa = (float)ia, fb = (float)b, fc = (float)ic;
  const bool both = a != 0u && c != 0u;
  const bool close = (float)(ia > ic ? ia - ic : ic - ia) <= e;
  const bool far = fb > fa + e && fb > fc + e;
  *out = (unsigned)m;
  return both && close && (b == 0u || far);
}

// the raw value of a source element: a key (0xFFFFFFFF -> 0) or an image element
template <bool F32, bool KEYS>
__device__ __forceinline__ unsigned source_at(const uint8_t* __restrict__ row, int x) {
  if (KEYS) {
    const unsigned k = ((const uint32_t*)row)[x];
    return k == KEY_EMPTY ? 0u : k;
  }
  return F32 ? ((const uint32_t*)row)[x] : (unsigned)((const uint16_t*)row)[x];
}

// four consecutive source elements from x on (x + j < w read, the rest 0); wide: x + 4 <= w and the row allows one load
template <bool F32, bool KEYS>
__device__ __forceinline__ void source_four(const uint8_t* __restrict__ row, int x, int w, bool wide, unsigned v[4]) {
  if (wide) {
    if (KEYS || F32) {
      const uint4 q = *(const uint4*)(row + (size_t)x * 4);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      if (KEYS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] == KEY_EMPTY ? 0u : v[j];
      }
    } else {
      const ushort4 q = *(const ushort4*)(row + (size_t)x * 2);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = x + j < w ? source_at<F32, KEYS>(row, x + j) : 0u;
}

// The body of both kernels.  src: the plane of image blockIdx.z (KEYS: uint32 keys, rows of src_pitch = 4 w bytes; else an
// image in the output's format).  FILL bit 0: the vertical pair, bit 1: the horizontal pair.
template <bool F32, int FILL, bool KEYS>
__device__ __forceinline__ void resolve_body(const uint8_t* __restrict__ src, int src_pitch, int w, int h, uint8_t* __restrict__ out,
                                             int out_pitch) {
  const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  constexpr int SRC_ELEM = KEYS || F32 ? 4 : 2, ELEM = F32 ? 4 : 2;
  const bool whole = x + 4 <= w;
  const bool src_wide = whole && (((uintptr_t)src | (uintptr_t)src_pitch) & (uintptr_t)(4 * SRC_ELEM - 1)) == 0u;
  const uint8_t* row = src + (size_t)y * src_pitch;
  unsigned b[4], res[4];
  source_four<F32, KEYS>(row, x, w, src_wide, b);
#pragma unroll
  for (int j = 0; j < 4; ++j) res[j] = b[j];
  if (FILL != 0 && y >= 1 && y <= h - 2) {                  // (border rows are copied)
    unsigned up[4] = {0u, 0u, 0u, 0u}, dn[4] = {0u, 0u, 0u, 0u};
    if (FILL & 1) {
      source_four<F32, KEYS>(row - src_pitch, x, w, src_wide, up);
      source_four<F32, KEYS>(row + src_pitch, x, w, src_wide, dn);
    }
    unsigned left = 0u, right = 0u;                         // the row's elements x - 1 and x + 4
    if (FILL & 2) {
      if (x >= 1) left = source_at<F32, KEYS>(row, x - 1);
      if (x + 4 < w) right = source_at<F32, KEYS>(row, x + 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (x + j < 1 || x + j > w - 2) continue;             // (border columns are copied)
      unsigned mv = 0u, mh = 0u;
      bool set_v = false, set_h = false;
      if (FILL & 1) set_v = fill_pair<F32>(up[j], b[j], dn[j], &mv);
      if (FILL & 2) set_h = fill_pair<F32>(j == 0 ? left : b[j - 1], b[j], j == 3 ? right : b[j + 1], &mh);
      res[j] = set_v ? mv : set_h ? mh : b[j];
    }
  }
  uint8_t* dst = out + (size_t)y * out_pitch + (size_t)x * ELEM;
  if (whole && (((uintptr_t)out | (uintptr_t)out_pitch) & (uintptr_t)(4 * ELEM - 1)) == 0u) {
    if (F32) *(uint4*)dst = make_uint4(res[0], res[1], res[2], res[3]);
    else *(uint2*)dst = make_uint2(res[0] | (res[1] << 16), res[2] | (res[3] << 16));
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < w) {
        if (F32) ((uint32_t*)dst)[j] = res[j];
        else ((uint16_t*)dst)[j] = (uint16_t)res[j];
      }
  }
}

template <bool F32, int FILL>
__global__ void __launch_bounds__(256)
k_depth_register_resolve(const unsigned* __restrict__ keys, int w, int h, uint8_t* __restrict__ out, int out_pitch, size_t out_stride) {
  resolve_body<F32, FILL, true>((const uint8_t*)(keys + (size_t)blockIdx.z * w * h), 4 * w, w, h, out + blockIdx.z * out_stride, out_pitch);
}

template <bool F32, int FILL>
__global__ void __launch_bounds__(256)
k_depth_fill_holes(const uint8_t* __restrict__ depth, int pitch, size_t stride, int w, int h, uint8_t* __restrict__ out, int out_pitch,
                   size_t out_stride) {
  resolve_body<F32, FILL, false>(depth + blockIdx.z * stride, pitch, w, h, out + blockIdx.z * out_stride, out_pitch);
}

dim3 rows_of_four(int w, int h, int n_img) { return dim3((((w + 3) / 4) + 63) / 64, (h + 3) / 4, n_img); }

}  // namespace

int sf_launch_depth_register_scatter(sf_context* c, const SfDepthIn& depth, int n_img, const SfDepthRegister& R, unsigned* d_keys) {
  const dim3 grid = rows_of_four(R.dw, R.dh, n_img);
  if (depth.format == SF_DEPTH_F32_M)
    hipLaunchKernelGGL(k_depth_register_scatter<true>, grid, dim3(256), 0, c->stream, (const uint8_t*)depth.p, depth.pitch, depth.stride, R, d_keys);
  else
    hipLaunchKernelGGL(k_depth_register_scatter<false>, grid, dim3(256), 0, c->stream, (const uint8_t*)depth.p, depth.pitch, depth.stride, R, d_keys);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

int sf_launch_depth_register_resolve(sf_context* c, const unsigned* d_keys, int format, int w, int h, int n_img, int fill, void* d_out,
                                     int out_pitch, size_t out_stride) {
  void (*kern)(const unsigned*, int, int, uint8_t*, int, size_t);
  static const decltype(kern) table[2][4] = {
      {k_depth_register_resolve<false, 0>, k_depth_register_resolve<false, 1>, k_depth_register_resolve<false, 2>, k_depth_register_resolve<false, 3>},
      {k_depth_register_resolve<true, 0>, k_depth_register_resolve<true, 1>, k_depth_register_resolve<true, 2>, k_depth_register_resolve<true, 3>}};
  kern = table[format == SF_DEPTH_F32_M ? 1 : 0][fill & 3];
  hipLaunchKernelGGL(kern, rows_of_four(w, h, n_img), dim3(256), 0, c->stream, d_keys, w, h, (uint8_t*)d_out, out_pitch, out_stride);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

int sf_launch_depth_fill_holes(sf_context* c, const SfDepthIn& depth, int n_img, int fill, void* d_out, int out_pitch, size_t out_stride) {
  void (*kern)(const uint8_t*, int, size_t, int, int, uint8_t*, int, size_t);
  static const decltype(kern) table[2][4] = {
      {k_depth_fill_holes<false, 0>, k_depth_fill_holes<false, 1>, k_depth_fill_holes<false, 2>, k_depth_fill_holes<false, 3>},
      {k_depth_fill_holes<true, 0>, k_depth_fill_holes<true, 1>, k_depth_fill_holes<true, 2>, k_depth_fill_holes<true, 3>}};
  kern = table[depth.format == SF_DEPTH_F32_M ? 1 : 0][fill & 3];
  hipLaunchKernelGGL(kern, rows_of_four(depth.w, depth.h, n_img), dim3(256), 0, c->stream, (const uint8_t*)depth.p, depth.pitch, depth.stride,
                     depth.w, depth.h, (uint8_t*)d_out, out_pitch, out_stride);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
