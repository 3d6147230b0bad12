// sf_front_device.hpp -- device helpers that two or more kernel files of the feature front end (k_gftt.hip, k_fast.hip,
// k_orb_detect.hip, k_extract.hip) share.  Everything here is forced inline: no kernel changes by calling it.
#pragma once
#include <hip/hip_runtime.h>

#include "sf_internal.hpp"

// cv::borderInterpolate(p, len, BORDER_REFLECT_101)
// (k_gftt.hip asks only for offsets of +-1 on sides >= 3, where one reflection is all the loop does)
__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// cv::fastAtan2 (OpenCV 3.x): degrees, float (ORB's centroid angle in k_extract.hip, SURF's orientation in k_surf.hip)
__device__ __forceinline__ float sf_fast_atan2(float y, float x) {
  constexpr float deg = (float)(180.0 / 3.14159265358979323846);
  constexpr float p1 = 0.9997878412794807f * deg, p3 = -0.3258083974640975f * deg, p5 = 0.1555786518463281f * deg,
                  p7 = -0.04432655554792128f * deg;
  constexpr float eps = (float)2.220446049250313080847263336181640625e-16;   // (float)DBL_EPSILON
  const float ax = fabsf(x), ay = fabsf(y);
  float a;
  if (ax >= ay) {
    const float c = ay / (ax + eps), c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    const float c = ax / (ay + eps), c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

// Byte offset of image z of a detector launch (SfCells: sf_internal.hpp): z * img_stride, or with cells the cell's first
// pixel inside its image.  Uniform per workgroup: scalar arithmetic.
__device__ __forceinline__ size_t sf_cell_base(unsigned z, size_t img_stride, const SfCells& g) {
  if (g.per_image == 1) return z * img_stride;
  const unsigned image = z / (unsigned)g.per_image, cell = z - image * (unsigned)g.per_image;
  const unsigned i = cell / (unsigned)g.cols, j = cell - i * (unsigned)g.cols;
  return image * img_stride + i * g.row_step + j * g.col_step;
}

__device__ __forceinline__ sf_keypoint sf_make_keypoint(float x, float y, float size, float response, int octave) {
  sf_keypoint k;
  k.x = x; k.y = y; k.size = size; k.angle = -1.0f; k.response = response; k.octave = octave; k.class_id = -1;
  return k;
}

// The tail of a candidate kernel (256 threads): the *s_n keys its workgroup staged in LDS go to the image's list with ONE
// global atomic on the image's counter; keys past `cap` are dropped (the counter still counts them).
__device__ __forceinline__ void sf_flush_staged_keys(const unsigned long long* s_keys, const unsigned* s_n, unsigned* s_base,
                                                     unsigned long long* __restrict__ keys, unsigned* __restrict__ count,
                                                     unsigned cap) {
  __syncthreads();
  if (threadIdx.x == 0 && *s_n) *s_base = atomicAdd(count, *s_n);
  __syncthreads();
  for (unsigned i = threadIdx.x; i < *s_n; i += 256)
    if (*s_base + i < cap) keys[*s_base + i] = s_keys[i];
}

// Stable compaction rank in a workgroup of 256 threads: the number of threads before this one whose flag is set, and the
// workgroup's total.  wave_cnt is a __shared__ int[4]; the caller ends its loop body with a __syncthreads() before the
// next call overwrites it.
struct SfRank { int before, total; };
__device__ __forceinline__ SfRank sf_block_rank(bool flag, int* wave_cnt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(flag);
  if (lane == 0) wave_cnt[wave] = __popcll(bal);
  __syncthreads();
  SfRank r = {0, 0};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = wave_cnt[q];
    if (q < wave) r.before += n;
    r.total += n;
  }
  r.before += __popcll(bal & ((1ull << lane) - 1ull));
  return r;
}
