// k_image.hip -- the first step of SURVEY.md section 8 rows f3 / f4: the camera's images as the reference holds them
// (cv_bridge "rgb8", data_handler.py:114-141) to the rectified gray planes the feature calls take -- what
// cv2.cvtColor(image, cv2.COLOR_RGB2GRAY) does to both stereo images before GetFeatsAndDesc (data_handler.py:424-428).
// OpenCV's 8-bit colour-to-gray is integer work: (c0 k0 + c1 k1 + c2 k2 + (1 << (shift - 1))) >> shift in int32, with the
// coefficient set of the OpenCV generation (restated in tests/image_ref.py).  bgr8 is rgb8 with k0 and
// k2 exchanged (the launcher does that), mono8 a pitched copy.
//
//   k_image_gray   n images per launch (blockIdx.y = image; images [0, n_first) from src0, the rest from src1: the left
//                  and right images of a batch are one launch).  A thread owns 16 consecutive pixels of a row: 48 source
//                  bytes as three 16-byte loads, one 16-byte store.  Lane i's loads start 48 bytes after lane i - 1's,
//                  so a wavefront's three load instructions each touch all 48 cache lines of its 3 KiB run; the first
//                  brings them in, the other two hit.  The one-line-per-lane alternative needs an exchange through LDS
//                  for a kernel that moves 4 bytes per pixel; not taken.
//                  A row's chunks are cut where the DESTINATION is 16-byte aligned: chunk 0 is the row's head (0 .. 15
//                  pixels, byte path), chunk c >= 1 starts at head + 16 (c - 1).  The 16-byte path serves a full chunk
//                  of a row whose source is 16-byte aligned at the same pixel (3 head + row address); every other chunk
//                  -- heads, tails, rows of odd pitches or base pointers -- goes byte by byte.  Bytes outside the
//                  width x height planes are never written.
//   k_image_copy   the same chunks for one-channel images (mono8): a pitched copy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_internal.hpp"

namespace {

struct ImageGeom {
  const uint8_t* src0;
  const uint8_t* src1;       // images n_first .. of the launch (src0 when there is one array)
  int n_first;
  int width, height;
  int src_pitch;
  size_t src_stride;
  uint8_t* dst;
  int dst_pitch;
  size_t dst_stride;
  int chunks;                // per row: the head + ceil(width / 16)
};

struct RowChunk {
  const uint8_t* s;          // the row's source and destination
  uint8_t* d;
  int x0, x1;                // pixels of this thread's chunk
  bool wide;                 // a full chunk with both addresses 16-byte aligned
};

template <int CH>
__device__ __forceinline__ bool row_chunk(const ImageGeom& g, RowChunk* r) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(idx / g.chunks), ch = (int)(idx - (long long)row * g.chunks);
  if (row >= g.height) return false;
  const int img = blockIdx.y;
  const uint8_t* base = img < g.n_first ? g.src0 + (size_t)img * g.src_stride : g.src1 + (size_t)(img - g.n_first) * g.src_stride;
  r->s = base + (size_t)row * g.src_pitch;
  r->d = g.dst + (size_t)img * g.dst_stride + (size_t)row * g.dst_pitch;
  const int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(r->d) & 15u)) & 15u);
  r->x0 = ch == 0 ? 0 : head + 16 * (ch - 1);
  r->x1 = min(ch == 0 ? head : r->x0 + 16, g.width);
  r->wide = ch > 0 && r->x0 + 16 <= g.width && ((reinterpret_cast<uintptr_t>(r->s) + (size_t)CH * head) & 15u) == 0;
  return r->x0 < r->x1;
}

__device__ __forceinline__ unsigned gray_of(unsigned c0, unsigned c1, unsigned c2, int k0, int k1, int k2, int half, int shift) {
  return (unsigned)(((int)c0 * k0 + (int)c1 * k1 + (int)c2 * k2 + half) >> shift);
}

__global__ void __launch_bounds__(256)
k_image_gray(const ImageGeom g, int k0, int k1, int k2, int shift) {
  RowChunk r;
  if (!row_chunk<3>(g, &r)) return;
  const int half = 1 << (shift - 1);
  if (r.wide) {
    const uint4* s4 = reinterpret_cast<const uint4*>(r.s + 3 * (size_t)r.x0);
    const uint4 a = s4[0], b = s4[1], c = s4[2];
    const unsigned w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    unsigned o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int b0 = 3 * p, b1 = 3 * p + 1, b2 = 3 * p + 2;
      const unsigned c0 = (w[b0 >> 2] >> (8 * (b0 & 3))) & 255u;
      const unsigned c1 = (w[b1 >> 2] >> (8 * (b1 & 3))) & 255u;
      const unsigned c2 = (w[b2 >> 2] >> (8 * (b2 & 3))) & 255u;
      o[p >> 2] |= (gray_of(c0, c1, c2, k0, k1, k2, half, shift) & 255u) << (8 * (p & 3));
    }
    *reinterpret_cast<uint4*>(r.d + r.x0) = make_uint4(o[0], o[1], o[2], o[3]);
    return;
  }
  for (int x = r.x0; x < r.x1; ++x) {
    const uint8_t* q = r.s + 3 * (size_t)x;
    r.d[x] = (uint8_t)gray_of(q[0], q[1], q[2], k0, k1, k2, half, shift);
  }
}

__global__ void __launch_bounds__(256)
k_image_copy(const ImageGeom g) {
  RowChunk r;
  if (!row_chunk<1>(g, &r)) return;
  if (r.wide) {
    *reinterpret_cast<uint4*>(r.d + r.x0) = *reinterpret_cast<const uint4*>(r.s + r.x0);
    return;
  }
  for (int x = r.x0; x < r.x1; ++x) r.d[x] = r.s[x];
}

}  // namespace

// The gray coefficients of a rule for the channels of an rgb8 pixel, in memory order
bool sf_gray_rule(int rule, int* kr, int* kg, int* kb, int* shift) {
  if (rule == 0) { *kr = 4899; *kg = 9617; *kb = 1868; *shift = 14; return true; }      // OpenCV 3.x
  if (rule == 1) { *kr = 9798; *kg = 19235; *kb = 3735; *shift = 15; return true; }     // OpenCV 4.x
  return false;
}

// n_images images of `format` -> gray planes, asynchronous on the handle's stream.  Images [0, n_first) lie at
// d_src0 + i * src_stride, images [n_first, n_images) at d_src1 + (i - n_first) * src_stride; image i's plane at
// d_dst + i * dst_stride.  The caller has validated the geometry (sf_keyframes.hip).
int sf_launch_image_gray(sf_context* c, const uint8_t* d_src0, const uint8_t* d_src1, int n_first, int format, int rule,
                         int width, int height, int src_pitch, size_t src_stride, int n_images, uint8_t* d_dst, int dst_pitch,
                         size_t dst_stride) {
  int kr, kg, kb, shift;
  if (!sf_gray_rule(rule, &kr, &kg, &kb, &shift)) return sf_fail(c, SF_EINVAL, "gray rule %d unknown (0 = OpenCV 3.x, 1 = OpenCV 4.x)", rule);
  if (n_images > 65535) return sf_fail(c, SF_ERANGE, "%d images in one conversion (at most 65535)", n_images);
  ImageGeom g;
  g.src0 = d_src0; g.src1 = d_src1 ? d_src1 : d_src0; g.n_first = d_src1 ? n_first : n_images;
  g.width = width; g.height = height;
  g.src_pitch = src_pitch; g.src_stride = src_stride;
  g.dst = d_dst; g.dst_pitch = dst_pitch; g.dst_stride = dst_stride;
  g.chunks = (width + 15) / 16 + 1;
  const long long threads = (long long)g.chunks * height;
  const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)n_images);
  if (format == SF_IMAGE_MONO8)
    hipLaunchKernelGGL(k_image_copy, grid, dim3(256), 0, c->stream, g);
  else if (format == SF_IMAGE_BGR8)
    hipLaunchKernelGGL(k_image_gray, grid, dim3(256), 0, c->stream, g, kb, kg, kr, shift);
  else
    hipLaunchKernelGGL(k_image_gray, grid, dim3(256), 0, c->stream, g, kr, kg, kb, shift);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
