// k_rectify.hip -- raw camera images to the rectified ones every other call takes: cv::initUndistortRectifyMap (float32 maps)
// + cv::remap(INTER_LINEAR, BORDER_CONSTANT, 0) on 8-bit images of one or three channels [upstream OpenCV 3.2, restated in
// tests/rectify_ref.py; DESIGN.md section 3 lists what the restatement decides].  The arithmetic is written out in
// include/sepfinder.h ("raw camera images"); the float64 steps run in the order written there, one rounded operation each
// (this file is compiled without FMA contraction), the rest is integer work.
//
//   k_rectify<CH, GRAY, TABLE>  n_a + n_b images per launch (blockIdx.y = image; images [0, n_a) from array a under plan a,
//                  the rest from array b under plan b: the left and right cameras of a stereo head are one launch).  A
//                  workgroup owns a tile of 64 x 4 output pixels, a wavefront 64 consecutive pixels of one row, a thread
//                  one pixel: the wavefront's stores are one run of 64 (gray, mono8) or 192 (colour) bytes, and since
//                  neighbouring output pixels map to neighbouring source pixels its two rows of taps fall in the two or
//                  three 128-byte lines that hold 65 neighbouring source pixels per row; the four wavefronts of the tile
//                  read rows that overlap (row i's lower taps are row i + 1's upper ones) and hit the CU's cache.
//                  TABLE = false, the computed form: the thread derives (mapx, mapy) from the plan's 21 doubles, which
//                  sit in scalar registers (the block's address is uniform); no map is read.  TABLE = true: {sx, sy} of the
//                  pixel from the plan's fixed-point table, one 8-byte load per thread, 512 bytes in a row per wavefront.
//                  GRAY: the three rectified channels go through the gray rule (k_image.hip's expression) to one byte.
//                  No LDS, no scratch; every tap and every store is guarded by its own bounds.  Where all four taps are
//                  inside, a row's two taps (2 CH bytes in a row) are one or two loads of any alignment instead of 2 CH byte
//                  loads: the gather is the kernel's time (5.6 -> 2.4 us per 752 x 480 stereo pair in a batch of 64, table
//                  form; profiles/rectify_latency.json), and the table form is the measured default (sf_internal.hpp).
//   k_rectify_map<TABLE>  the maps of one computed plan: float32 (mapx, mapy) for sf_rectify_maps_device, or the
//                  fixed-point table the table form reads.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_internal.hpp"

namespace {

constexpr int RECT_INVALID = -(1 << 30);   // {sx, sy} of a pixel the non-finite rule sets to 0: ix = -2^25, every tap outside
constexpr int TILE_W = 64, TILE_H = 4;

struct RectifyGeom {
  RectifyImages im;
  const RectifyBlock* blk_a;
  const RectifyBlock* blk_b;
  const int2* tab_a;
  const int2* tab_b;
  int k0, k1, k2, shift;     // the gray rule for the channels in memory order (GRAY forms)
  int tiles_x;
};

// (mapx, mapy) of output pixel (column j, row i): include/sepfinder.h, in that order
__device__ __forceinline__ void rect_map(const RectifyBlock* __restrict__ B, int j, int i, float* mapx, float* mapy) {
  const double dj = (double)j, di = (double)i;
  const double X = ((B->iR[0] * dj) + (B->iR[1] * di)) + B->iR[2];
  const double Y = ((B->iR[3] * dj) + (B->iR[4] * di)) + B->iR[5];
  const double W = ((B->iR[6] * dj) + (B->iR[7] * di)) + B->iR[8];
  const double w = 1.0 / W;
  const double x = X * w;
  const double y = Y * w;
  const double x2 = x * x;
  const double y2 = y * y;
  const double r2 = x2 + y2;
  const double t = (2.0 * x) * y;
  const double k1 = B->D[0], k2 = B->D[1], p1 = B->D[2], p2 = B->D[3], k3 = B->D[4], k4 = B->D[5], k5 = B->D[6], k6 = B->D[7];
  const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
  const double xd = (x * kr + p1 * t) + p2 * (r2 + 2.0 * x2);
  const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * t;
  *mapx = (float)(B->fx * xd + B->cx);
  *mapy = (float)(B->fy * yd + B->cy);
}

// the fixed-point coordinates of a map value: round-half-even of the float32 product
__device__ __forceinline__ int2 rect_fixed(float mapx, float mapy) {
  const float vx = mapx * 32.f, vy = mapy * 32.f;
  if (!(fabsf(vx) < 1073741824.f && fabsf(vy) < 1073741824.f)) return make_int2(RECT_INVALID, RECT_INVALID);   // (NaN too)
  return make_int2((int)rintf(vx), (int)rintf(vy));
}

// the four taps of one output pixel; a tap outside the source reads 0
template <int CH>
__device__ __forceinline__ void rect_taps(const uint8_t* __restrict__ src, int pitch, int sw, int sh, int2 s, int out[CH]) {
  const int ix = s.x >> 5, iy = s.y >> 5, a = s.x & 31, b = s.y & 31;
  const int w00 = 32 * (32 - a) * (32 - b), w01 = 32 * a * (32 - b), w10 = 32 * (32 - a) * b, w11 = 32 * a * b;
  const bool x0 = (unsigned)ix < (unsigned)sw, x1 = (unsigned)(ix + 1) < (unsigned)sw;
  const bool y0 = (unsigned)iy < (unsigned)sh, y1 = (unsigned)(iy + 1) < (unsigned)sh;
  const long long at = (long long)iy * pitch + (long long)CH * ix;     // (only dereferenced where the tap is inside)
  if (x0 && x1 && y0 && y1) {
    // all four inside, the usual case: a row's two taps are 2 CH bytes in a row, read as one (mono8) or two (colour)
    // loads of whatever alignment instead of 2 CH byte loads -- the gather is what this kernel spends its time on
    const uint8_t* p0 = src + at;
    const uint8_t* p1 = p0 + pitch;
    unsigned long long r0, r1;
    if constexpr (CH == 1) {
      uint16_t a0, a1;
      __builtin_memcpy(&a0, p0, 2);
      __builtin_memcpy(&a1, p1, 2);
      r0 = a0; r1 = a1;
    } else {
      uint32_t a0, a1;
      uint16_t b0, b1;
      __builtin_memcpy(&a0, p0, 4);
      __builtin_memcpy(&b0, p0 + 4, 2);
      __builtin_memcpy(&a1, p1, 4);
      __builtin_memcpy(&b1, p1 + 4, 2);
      r0 = a0 | ((unsigned long long)b0 << 32); r1 = a1 | ((unsigned long long)b1 << 32);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c)
      out[c] = (16384 + w00 * (int)((r0 >> (8 * c)) & 255u) + w01 * (int)((r0 >> (8 * (c + CH))) & 255u) +
                w10 * (int)((r1 >> (8 * c)) & 255u) + w11 * (int)((r1 >> (8 * (c + CH))) & 255u)) >> 15;
    return;
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    int acc = 16384;
    if (y0 && x0) acc += w00 * (int)src[at + c];
    if (y0 && x1) acc += w01 * (int)src[at + CH + c];
    if (y1 && x0) acc += w10 * (int)src[at + pitch + c];
    if (y1 && x1) acc += w11 * (int)src[at + pitch + CH + c];
    out[c] = acc >> 15;
  }
}

template <int CH, bool GRAY, bool TABLE>
__global__ void __launch_bounds__(256)
k_rectify(const RectifyGeom g) {
  const int tx = (int)(blockIdx.x % (unsigned)g.tiles_x), ty = (int)(blockIdx.x / (unsigned)g.tiles_x);
  const int j = tx * TILE_W + (int)(threadIdx.x & (TILE_W - 1)), i = ty * TILE_H + (int)(threadIdx.x / TILE_W);
  if (j >= g.im.out_w || i >= g.im.out_h) return;
  const int img = blockIdx.y;
  const bool second = img >= g.im.n_a;
  const int k = second ? img - g.im.n_a : img;
  const uint8_t* src = (second ? g.im.src_b : g.im.src_a) + (size_t)k * g.im.src_stride;
  uint8_t* dst = (second ? g.im.dst_b : g.im.dst_a) + (size_t)k * g.im.dst_stride + (size_t)i * g.im.dst_pitch;
  int2 s;
  if (TABLE) {
    s = (second ? g.tab_b : g.tab_a)[(size_t)i * g.im.out_w + j];
  } else {
    float mapx, mapy;
    rect_map(second ? g.blk_b : g.blk_a, j, i, &mapx, &mapy);
    s = rect_fixed(mapx, mapy);
  }
  int px[CH];
  rect_taps<CH>(src, g.im.src_pitch, g.im.src_w, g.im.src_h, s, px);
  if constexpr (CH == 1) {
    dst[j] = (uint8_t)px[0];
  } else if constexpr (GRAY) {
    dst[j] = (uint8_t)((px[0] * g.k0 + px[1] * g.k1 + px[2] * g.k2 + (1 << (g.shift - 1))) >> g.shift);
  } else {
#pragma unroll
    for (int c = 0; c < CH; ++c) dst[(size_t)CH * j + c] = (uint8_t)px[c];
  }
}

template <bool TABLE>
__global__ void __launch_bounds__(256)
k_rectify_map(const RectifyBlock* __restrict__ B, int out_w, int out_h, int tiles_x, float* mapx_out, float* mapy_out,
              int pitch_bytes, int2* table) {
  const int tx = (int)(blockIdx.x % (unsigned)tiles_x), ty = (int)(blockIdx.x / (unsigned)tiles_x);
  const int j = tx * TILE_W + (int)(threadIdx.x & (TILE_W - 1)), i = ty * TILE_H + (int)(threadIdx.x / TILE_W);
  if (j >= out_w || i >= out_h) return;
  float mapx, mapy;
  rect_map(B, j, i, &mapx, &mapy);
  if (TABLE) {
    table[(size_t)i * out_w + j] = rect_fixed(mapx, mapy);
  } else {
    reinterpret_cast<float*>(reinterpret_cast<char*>(mapx_out) + (size_t)i * pitch_bytes)[j] = mapx;
    reinterpret_cast<float*>(reinterpret_cast<char*>(mapy_out) + (size_t)i * pitch_bytes)[j] = mapy;
  }
}

dim3 tile_grid(int out_w, int out_h, int n_images, int* tiles_x) {
  *tiles_x = (out_w + TILE_W - 1) / TILE_W;
  return dim3((unsigned)(*tiles_x * ((out_h + TILE_H - 1) / TILE_H)), (unsigned)n_images);
}

}  // namespace

int sf_launch_rectify_maps(sf_context* c, const RectifyBlock* d_block, int out_w, int out_h, float* d_mapx, float* d_mapy,
                           int pitch_bytes, int32_t* d_table) {
  int tiles_x;
  const dim3 grid = tile_grid(out_w, out_h, 1, &tiles_x);
  if (d_table)
    hipLaunchKernelGGL(k_rectify_map<true>, grid, dim3(256), 0, c->stream, d_block, out_w, out_h, tiles_x, nullptr, nullptr, 0,
                       reinterpret_cast<int2*>(d_table));
  else
    hipLaunchKernelGGL(k_rectify_map<false>, grid, dim3(256), 0, c->stream, d_block, out_w, out_h, tiles_x, d_mapx, d_mapy,
                       pitch_bytes, nullptr);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

int sf_launch_rectify(sf_context* c, const RectifyImages& im, int format, int out_format, int rule, const RectifyBlock* blk_a,
                      const RectifyBlock* blk_b, const int32_t* tab_a, const int32_t* tab_b) {
  int kr, kg, kb, shift;
  if (!sf_gray_rule(rule, &kr, &kg, &kb, &shift)) return sf_fail(c, SF_EINVAL, "gray rule %d unknown (0 = OpenCV 3.x, 1 = OpenCV 4.x)", rule);
  const int n = im.n_a + im.n_b;
  if (n > 65535) return sf_fail(c, SF_ERANGE, "%d images in one rectification (at most 65535, both arrays together)", n);
  RectifyGeom g;
  g.im = im;
  g.blk_a = blk_a; g.blk_b = blk_b;
  g.tab_a = reinterpret_cast<const int2*>(tab_a); g.tab_b = reinterpret_cast<const int2*>(tab_b);
  g.k0 = format == SF_IMAGE_BGR8 ? kb : kr; g.k1 = kg; g.k2 = format == SF_IMAGE_BGR8 ? kr : kb; g.shift = shift;
  const dim3 grid = tile_grid(im.out_w, im.out_h, n, &g.tiles_x);
  const bool table = tab_a != nullptr, gray = format != SF_IMAGE_MONO8 && out_format == SF_IMAGE_MONO8;
  void (*kern)(const RectifyGeom);
  if (format == SF_IMAGE_MONO8) kern = table ? k_rectify<1, false, true> : k_rectify<1, false, false>;
  else if (gray) kern = table ? k_rectify<3, true, true> : k_rectify<3, true, false>;
  else kern = table ? k_rectify<3, false, true> : k_rectify<3, false, false>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, c->stream, g);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
