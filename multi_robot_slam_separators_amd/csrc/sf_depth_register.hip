// sf_depth_register.hip -- the C-ABI of "depth registration" (include/sepfinder.h): the block's defaults and validation (host
// only, no handle), and the argument checks and launch sequences in front of k_depth_register.hip.  Nothing here computes in
// canonical arithmetic: the block's floats go to the kernel as they are.
#include <cmath>
#include <cstring>

#include "sf_internal.hpp"

namespace {

constexpr int MAX_SIDE = 8192;

bool side_ok(int v) { return v >= 1 && v <= MAX_SIDE; }

int check_block(sf_context* c, const char* call, const sf_depth_registration* r) {
  if (!side_ok(r->depth_width) || !side_ok(r->depth_height))
    return sf_fail(c, SF_EINVAL, "%s: depth image of %d x %d (both sides 1 .. %d)", call, r->depth_width, r->depth_height, MAX_SIDE);
  if (!side_ok(r->width) || !side_ok(r->height))
    return sf_fail(c, SF_EINVAL, "%s: registered image of %d x %d (both sides 1 .. %d)", call, r->width, r->height, MAX_SIDE);
  const float k[8] = {r->fx, r->fy, r->cx, r->cy, r->rfx, r->rfy, r->rcx, r->rcy};
  for (float v : k) if (!std::isfinite(v)) return sf_fail(c, SF_EINVAL, "%s: an intrinsic parameter is not finite", call);
  for (float v : r->transform) if (!std::isfinite(v)) return sf_fail(c, SF_EINVAL, "%s: transform holds a non-finite value", call);
  if (!(r->fx > 0.0f) || !(r->fy > 0.0f)) return sf_fail(c, SF_EINVAL, "%s: fx and fy of the depth camera must be > 0", call);
  if (!(r->rfx > 0.0f) || !(r->rfy > 0.0f)) return sf_fail(c, SF_EINVAL, "%s: rfx and rfy of the colour camera must be > 0", call);
  if ((r->fill_vertical != 0 && r->fill_vertical != 1) || (r->fill_horizontal != 0 && r->fill_horizontal != 1))
    return sf_fail(c, SF_EINVAL, "%s: fill_vertical %d and fill_horizontal %d must each be 0 or 1", call, r->fill_vertical, r->fill_horizontal);
  if (r->reserved != 0) return sf_fail(c, SF_EINVAL, "%s: reserved must be 0", call);
  return SF_OK;
}

// n planes of w x h elements of `elem` bytes at p, rows `pitch` and planes `stride` bytes apart, under the name `what`
int check_planes(sf_context* c, const char* call, const char* what, const void* p, int elem, int w, int h, int pitch, size_t stride, int n) {
  if (!p) return sf_fail(c, SF_EINVAL, "%s: the %s array is missing", call, what);
  if ((uintptr_t)p % (uintptr_t)elem) return sf_fail(c, SF_EINVAL, "%s: the %s address is no multiple of the %d bytes of a pixel", call, what, elem);
  if ((long long)pitch < (long long)elem * w)
    return sf_fail(c, SF_EINVAL, "%s: %s pitch %d is less than a row of %d pixels of %d bytes", call, what, pitch, w, elem);
  if (pitch % elem) return sf_fail(c, SF_EINVAL, "%s: %s pitch %d is no multiple of the %d bytes of a pixel", call, what, pitch, elem);
  if (n > 1) {
    if (stride % (size_t)elem) return sf_fail(c, SF_EINVAL, "%s: %s stride %zu is no multiple of the %d bytes of a pixel", call, what, stride, elem);
    if (stride < (size_t)pitch * (h - 1) + (size_t)elem * w)
      return sf_fail(c, SF_EINVAL, "%s: %s stride %zu is less than an image (%d rows of pitch %d)", call, what, stride, h, pitch);
  }
  return SF_OK;
}

// the bytes n planes span, first to one past the last
size_t span(int elem, int w, int h, int pitch, size_t stride, int n) {
  return (size_t)(n - 1) * (n > 1 ? stride : 0) + (size_t)pitch * (h - 1) + (size_t)elem * w;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

int check_format(sf_context* c, const char* call, int format) {
  if (format != SF_DEPTH_U16_MM && format != SF_DEPTH_F32_M)
    return sf_fail(c, SF_EINVAL, "%s: depth format %d unknown (0 = uint16 millimetres, 1 = float32 metres)", call, format);
  return SF_OK;
}

}  // namespace

extern "C" void sf_depth_registration_defaults(sf_depth_registration* r) {
  if (!r) return;
  memset(r, 0, sizeof(*r));
  r->transform[0] = r->transform[5] = r->transform[10] = 1.0f;
}

extern "C" int sf_depth_register_check(const sf_depth_registration* reg) {
  if (!reg) return SF_EINVAL;
  return check_block(nullptr, "sf_depth_register_check", reg);
}

extern "C" int sf_debug_depth_register_limits(sf_handle c, int32_t batch_chunk, int32_t stages) {
  if (!c) return SF_EINVAL;
  if (batch_chunk < 0 || batch_chunk > 65535 || stages < 0 || stages > 7)
    return sf_fail(c, SF_EINVAL, "sf_debug_depth_register_limits: batch_chunk %d outside 0 .. 65535 or stages %d outside 0 .. 7", batch_chunk, stages);
  c->dreg_debug_chunk = batch_chunk;
  c->dreg_debug_stages = stages;
  return SF_OK;
}

extern "C" int sf_depth_register_device(sf_handle c, const sf_depth_registration* reg, const void* d_depth, int32_t depth_format,
                                        int32_t depth_pitch, size_t depth_stride, int32_t n_images, void* d_out, int32_t out_pitch,
                                        size_t out_stride) {
  static const char* const call = "sf_depth_register_device";
  if (!c || !reg || n_images < 0) return SF_EINVAL;
  int rc = check_block(c, call, reg);
  if (rc != SF_OK || (rc = check_format(c, call, depth_format)) != SF_OK || n_images == 0) return rc;
  const int elem = depth_format == SF_DEPTH_F32_M ? 4 : 2;
  const int dw = reg->depth_width, dh = reg->depth_height, W = reg->width, H = reg->height;
  if ((rc = check_planes(c, call, "depth", d_depth, elem, dw, dh, depth_pitch, depth_stride, n_images)) != SF_OK) return rc;
  if ((rc = check_planes(c, call, "output", d_out, elem, W, H, out_pitch, out_stride, n_images)) != SF_OK) return rc;
  if (overlap(d_depth, span(elem, dw, dh, depth_pitch, depth_stride, n_images), d_out, span(elem, W, H, out_pitch, out_stride, n_images)))
    return sf_fail(c, SF_EINVAL, "%s: the output overlaps the depth images (the registration is out of place)", call);
  SF_HIP(c, hipSetDevice(c->device));
  // one uint32 key per output pixel; a batch whose keys pass the workspace runs in chunks of images, queued back to back
  const size_t plane = (size_t)W * H * sizeof(unsigned);
  size_t chunk = std::max<size_t>(1, DEPTH_REGISTER_WORKSPACE_BYTES / plane);
  if (c->dreg_debug_chunk) chunk = (size_t)c->dreg_debug_chunk;
  chunk = std::min<size_t>(std::min<size_t>(chunk, 65535), (size_t)n_images);
  if ((rc = sf_buf_reserve(c, c->dreg_keys, plane * chunk)) != SF_OK) return rc;
  SfDepthRegister R;
  R.fx = reg->fx; R.fy = reg->fy; R.cx = reg->cx; R.cy = reg->cy;
  R.rfx = reg->rfx; R.rfy = reg->rfy; R.rcx = reg->rcx; R.rcy = reg->rcy;
  memcpy(R.T, reg->transform, sizeof(R.T));
  R.dw = dw; R.dh = dh; R.W = W; R.H = H;
  const int fill = (reg->fill_vertical ? 1 : 0) | (reg->fill_horizontal ? 2 : 0);
  const int stages = c->dreg_debug_stages ? c->dreg_debug_stages : 7;
  const size_t ds = n_images > 1 ? depth_stride : 0, os = n_images > 1 ? out_stride : 0;
  unsigned* keys = (unsigned*)c->dreg_keys.p;
  for (size_t i0 = 0; i0 < (size_t)n_images; i0 += chunk) {
    const int n = (int)std::min<size_t>(chunk, (size_t)n_images - i0);
    SfDepthIn D;
    D.p = (const uint8_t*)d_depth + i0 * ds; D.format = depth_format; D.pitch = depth_pitch; D.stride = ds; D.w = dw; D.h = dh;
    if (stages & 1) SF_HIP(c, hipMemsetAsync(keys, 0xFF, plane * n, c->stream));
    if ((stages & 2) && (rc = sf_launch_depth_register_scatter(c, D, n, R, keys)) != SF_OK) return rc;
    if ((stages & 4) && (rc = sf_launch_depth_register_resolve(c, keys, depth_format, W, H, n, fill, (uint8_t*)d_out + i0 * os, out_pitch, os)) != SF_OK)
      return rc;
  }
  return SF_OK;
}

extern "C" int sf_depth_fill_holes_device(sf_handle c, const void* d_depth, int32_t depth_format, int32_t width, int32_t height,
                                          int32_t depth_pitch, size_t depth_stride, int32_t n_images, int32_t fill_vertical,
                                          int32_t fill_horizontal, void* d_out, int32_t out_pitch, size_t out_stride) {
  static const char* const call = "sf_depth_fill_holes_device";
  if (!c || n_images < 0) return SF_EINVAL;
  int rc = check_format(c, call, depth_format);
  if (rc != SF_OK) return rc;
  if ((fill_vertical != 0 && fill_vertical != 1) || (fill_horizontal != 0 && fill_horizontal != 1))
    return sf_fail(c, SF_EINVAL, "%s: fill_vertical %d and fill_horizontal %d must each be 0 or 1", call, fill_vertical, fill_horizontal);
  if (n_images == 0) return SF_OK;
  if (!side_ok(width) || !side_ok(height)) return sf_fail(c, SF_EINVAL, "%s: image of %d x %d (both sides 1 .. %d)", call, width, height, MAX_SIDE);
  const int elem = depth_format == SF_DEPTH_F32_M ? 4 : 2;
  if ((rc = check_planes(c, call, "depth", d_depth, elem, width, height, depth_pitch, depth_stride, n_images)) != SF_OK) return rc;
  if ((rc = check_planes(c, call, "output", d_out, elem, width, height, out_pitch, out_stride, n_images)) != SF_OK) return rc;
  if (overlap(d_depth, span(elem, width, height, depth_pitch, depth_stride, n_images), d_out,
              span(elem, width, height, out_pitch, out_stride, n_images)))
    return sf_fail(c, SF_EINVAL, "%s: the output overlaps the input (the fill is out of place)", call);
  SF_HIP(c, hipSetDevice(c->device));
  const int fill = (fill_vertical ? 1 : 0) | (fill_horizontal ? 2 : 0);
  const size_t ds = n_images > 1 ? depth_stride : 0, os = n_images > 1 ? out_stride : 0;
  for (size_t i0 = 0; i0 < (size_t)n_images; i0 += 65535) {                  // (a launch takes 65535 images)
    SfDepthIn D;
    D.p = (const uint8_t*)d_depth + i0 * ds; D.format = depth_format; D.pitch = depth_pitch; D.stride = ds; D.w = width; D.h = height;
    const int n = (int)std::min<size_t>(65535, (size_t)n_images - i0);
    if ((rc = sf_launch_depth_fill_holes(c, D, n, fill, (uint8_t*)d_out + i0 * os, out_pitch, os)) != SF_OK) return rc;
  }
  return SF_OK;
}
