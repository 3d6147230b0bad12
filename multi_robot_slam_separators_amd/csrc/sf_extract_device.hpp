// sf_extract_device.hpp -- what the descriptor kernels of keyframe extraction share (k_extract.hip: BRIEF and ORB rows;
// k_freak.hip: FREAK rows): the batch layout of a launch sequence, the camera of the 3D points and the 3D point itself.
// Everything here is forced inline: no kernel changes by calling it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_internal.hpp"

// A batch of keyframes in one launch sequence (blockIdx.y = image, except k_extract_commit: blockIdx.x): images
// img_stride bytes apart, integral images s_stride entries apart, per-corner arrays per_image entries apart, the corner
// count of every image in d_n (device; null = the scalar n of the single-image call).  ORB on a pyramid: the pyramids
// (levels >= 1) pyr_stride bytes apart.
struct ExtractBatch {
  size_t img_stride, s_stride, pyr_stride;
  int per_image;
  const int32_t* d_n;
};

struct ExtractCam {
  float fx, fy, cx, cy, cx_right, baseline, L[12], min_depth, max_depth;
  int identity_local, filter;
};

// the kernels' view of the caller's camera; filter: a corner without a finite 3D point is dropped
inline ExtractCam sf_extract_cam(const sf_stereo_camera* cam) {
  ExtractCam ec;
  ec.fx = cam->fx; ec.fy = cam->fy; ec.cx = cam->cx; ec.cy = cam->cy; ec.cx_right = cam->cx_right;
  ec.baseline = cam->baseline; ec.min_depth = cam->min_depth; ec.max_depth = cam->max_depth;
  ec.identity_local = 1;
  for (int e = 0; e < 12; ++e) {
    ec.L[e] = cam->local_transform[e];
    ec.identity_local = ec.identity_local && (ec.L[e] == ((e == 0 || e == 5 || e == 10) ? 1.0f : 0.0f));
  }
  ec.filter = cam->min_depth > 0.0f || cam->max_depth > 0.0f;
  return ec;
}

// k_depth_points (k_depth.hip) between the describe kernel and k_extract_commit of sf_launch_extract_batch, for a keyframe
// with a depth image: the 3D point of every corner from `depth` into xyz_tmp, keep[i] &= !cam.filter || the point is finite
// (the describe kernel has run without right_x and without the filter: keep = "patch inside")
void sf_launch_depth_points(sf_context* c, const SfDepthIn& depth, int width, int height, const sf_keypoint* d_kpts, int n, int n_img,
                            const ExtractCam& cam, float* xyz_tmp, uint8_t* keep, uint8_t* valid, const ExtractBatch& B);

// Byte 0's thread of a corner: the 3D point of the stereo pair (NaN when there is none) and the keep flag -- shared by
// the BRIEF and the ORB descriptor kernels
__device__ __forceinline__ void extract_point(const sf_keypoint& k, int i, bool inside, const float* __restrict__ right_x,
                                              const uint8_t* __restrict__ status, const ExtractCam& cam,
                                              float* __restrict__ xyz_tmp, uint8_t* __restrict__ keep) {
  const float qnan = __int_as_float(0x7FC00000);
  float p0 = qnan, p1 = qnan, p2 = qnan;
  if (inside && right_x && (!status || status[i])) {
    const float disparity = k.x - right_x[i];
    if (disparity != 0.0f && disparity > 0.0f && cam.baseline > 0.0f && cam.fx > 0.0f) {
      float c = 0.0f;
      if (cam.cx_right > 0.0f && cam.cx > 0.0f) c = cam.cx_right - cam.cx;
      const float W = cam.baseline / (disparity + c);
      const float x = (k.x - cam.cx) * W, y = (k.y - cam.cy) * W, z = cam.fx * W;
      if (isfinite(x) && isfinite(y) && isfinite(z) && (cam.min_depth < 0.0f || z > cam.min_depth) &&
          (cam.max_depth <= 0.0f || z <= cam.max_depth)) {
        if (cam.identity_local) {
          p0 = x; p1 = y; p2 = z;
        } else {
          p0 = ((cam.L[0] * x + cam.L[1] * y) + cam.L[2] * z) + cam.L[3];
          p1 = ((cam.L[4] * x + cam.L[5] * y) + cam.L[6] * z) + cam.L[7];
          p2 = ((cam.L[8] * x + cam.L[9] * y) + cam.L[10] * z) + cam.L[11];
        }
      }
    }
  }
  xyz_tmp[3 * i] = p0; xyz_tmp[3 * i + 1] = p1; xyz_tmp[3 * i + 2] = p2;
  keep[i] = (uint8_t)(inside && (!cam.filter || (isfinite(p0) && isfinite(p1) && isfinite(p2))));
}

// k_freak_points (k_freak.hip) between the integral image and k_extract_commit of sf_launch_extract_batch: FREAK rows into
// desc_tmp, every corner's keypoint (the kept ones with their FREAK angle) into d_kpts_angle, 3D points and keep flags
void sf_launch_freak_points(sf_context* c, const uint8_t* d_left, int pitch, const int32_t* S, int width, int height,
                            const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status, int n, int n_img,
                            const SfFreakTables& T, const ExtractCam& cam, sf_keypoint* d_kpts_angle, uint8_t* desc_tmp,
                            float* xyz_tmp, uint8_t* keep, const ExtractBatch& B);

// k_surf_describe (k_surf.hip) in the same place: SURF rows (float32, 64 or 128 per keypoint) into desc_tmp, every
// keypoint (the kept ones with their SURF angle) into d_kpts_angle, 3D points and keep flags
void sf_launch_surf_describe(sf_context* c, const uint8_t* d_left, int pitch, const int32_t* S, int width, int height,
                             const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status, int n, int n_img,
                             const SfSurfTables& T, const ExtractCam& cam, sf_keypoint* d_kpts_angle, float* desc_tmp,
                             float* xyz_tmp, uint8_t* keep, const ExtractBatch& B);

// k_sift_describe (k_sift.hip) in the same place: SIFT rows (128 float32 holding 0 .. 255) into desc_tmp, every keypoint
// unchanged into d_kpts_out, 3D points and keep flags.  One image (n_img 1): it builds or reuses the Gaussian pyramid;
// kind.batch: the n_img images of the chunk sf_launch_detect_sift has just run, whose pyramids it reads
int sf_launch_sift_describe(sf_context* c, const uint8_t* d_left, int pitch, int width, int height, const SfSiftKind& kind,
                            const sf_keypoint* d_kpts, const float* d_right_x, const uint8_t* d_status, int n, int n_img,
                            const ExtractCam& cam, sf_keypoint* d_kpts_out, float* desc_tmp, float* xyz_tmp, uint8_t* keep,
                            const ExtractBatch& B);
