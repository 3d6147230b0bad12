// sf_rectify.hip -- the C-ABI of "raw camera images" (include/sepfinder.h): rectification plans on the handle, their
// validation and host arithmetic, and the argument checks in front of k_rectify.hip's two launches.  The plan's inverse
// (P[:, :3] R)^-1 is float64 in the order written below, one rounded operation per step: this file is compiled without FMA
// contraction, like the kernels that read the result (tests/rectify_ref.py restates both).
#include <cmath>
#include <cstring>

#include "sf_internal.hpp"

namespace {

constexpr int MAX_SIDE = 8192;

bool side_ok(int v) { return v >= 1 && v <= MAX_SIDE; }

// Validates a block and derives iR; `call` starts every message
int check_info(sf_context* c, const char* call, const sf_camera_info* m, double iR[9]) {
  for (double v : m->K) if (!std::isfinite(v)) return sf_fail(c, SF_EINVAL, "%s: K holds a non-finite value", call);
  for (double v : m->D) if (!std::isfinite(v)) return sf_fail(c, SF_EINVAL, "%s: D holds a non-finite value", call);
  for (double v : m->R) if (!std::isfinite(v)) return sf_fail(c, SF_EINVAL, "%s: R holds a non-finite value", call);
  for (double v : m->P) if (!std::isfinite(v)) return sf_fail(c, SF_EINVAL, "%s: P holds a non-finite value", call);
  if (m->reserved != 0) return sf_fail(c, SF_EINVAL, "%s: reserved must be 0", call);
  if (m->model != 0 && m->model != 1)
    return sf_fail(c, SF_EINVAL, "%s: distortion model %d unknown (0 = plumb_bob, 1 = rational_polynomial)", call, m->model);
  if (!side_ok(m->width) || !side_ok(m->height))
    return sf_fail(c, SF_EINVAL, "%s: raw image of %d x %d (both sides 1 .. %d)", call, m->width, m->height, MAX_SIDE);
  if ((m->out_width != 0 && !side_ok(m->out_width)) || (m->out_height != 0 && !side_ok(m->out_height)))
    return sf_fail(c, SF_EINVAL, "%s: rectified image of %d x %d (both sides 1 .. %d, 0 = the raw size)", call, m->out_width,
                   m->out_height, MAX_SIDE);
  if (!(m->K[0] > 0.0) || !(m->K[4] > 0.0)) return sf_fail(c, SF_EINVAL, "%s: fx and fy of K must be > 0", call);
  if (!(m->P[0] > 0.0) || !(m->P[5] > 0.0)) return sf_fail(c, SF_EINVAL, "%s: fx and fy of P must be > 0", call);
  if (m->K[1] != 0.0) return sf_fail(c, SF_EINVAL, "%s: K has a skew of %g (not built)", call, m->K[1]);
  // M = P[:, :3] R, every entry ((p0 r0) + (p1 r1)) + (p2 r2)
  double M[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      M[3 * i + j] = (m->P[4 * i] * m->R[j] + m->P[4 * i + 1] * m->R[3 + j]) + m->P[4 * i + 2] * m->R[6 + j];
  // the adjugate over the determinant
  const double a = M[0], b = M[1], cc = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
  const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
  const double det = (a * c00 + b * c01) + cc * c02;
  if (!std::isfinite(det) || det == 0.0) return sf_fail(c, SF_EINVAL, "%s: P[:, :3] R is singular (determinant %g)", call, det);
  const double adj[9] = {c00, cc * h - b * i, b * f - cc * e, c01, a * i - cc * g, cc * d - a * f, c02, b * g - a * h, a * e - b * d};
  for (int k = 0; k < 9; ++k) iR[k] = adj[k] / det;
  return SF_OK;
}

int plan_of(sf_context* c, int id, const RectifyPlan** out) {
  if (id < 1 || id > (int)c->rect_plans.size())
    return sf_fail(c, SF_EINVAL, "rectification plan %d outside the table (1 .. %d)", id, (int)c->rect_plans.size());
  *out = &c->rect_plans[id - 1];
  return SF_OK;
}

int table_full(sf_context* c, const char* call) {
  if ((int)c->rect_plans.size() >= SF_MAX_RECTIFY_PLANS)
    return sf_fail(c, SF_ERANGE, "%s: the table holds %d plans", call, SF_MAX_RECTIFY_PLANS);
  return SF_OK;
}

const RectifyBlock* block_of(const sf_context* c, int id) { return (const RectifyBlock*)c->rect_blocks.p + (id - 1); }

// the fixed-point table of a computed plan, built on the stream the first time the table form asks for it
int table_ready(sf_context* c, int id) {
  RectifyPlan& p = c->rect_plans[id - 1];
  if (p.table_ready) return SF_OK;
  int rc = sf_buf_reserve(c, p.table, (size_t)p.out_w * p.out_h * 2 * sizeof(int32_t));
  if (rc != SF_OK) return rc;
  if ((rc = sf_launch_rectify_maps(c, block_of(c, id), p.out_w, p.out_h, nullptr, nullptr, 0, (int32_t*)p.table.p)) != SF_OK) return rc;
  p.table_ready = true;
  return SF_OK;
}

}  // namespace

extern "C" int sf_rectify_check_info(const sf_camera_info* info, double* iR_out) {
  if (!info) return SF_EINVAL;
  double iR[9];
  const int rc = check_info(nullptr, "sf_rectify_check_info", info, iR);
  if (rc == SF_OK && iR_out) memcpy(iR_out, iR, sizeof(iR));
  return rc;
}

extern "C" int sf_rectify_plan_create(sf_handle c, const sf_camera_info* info, int32_t* plan_out) {
  if (!c || !info || !plan_out) return SF_EINVAL;
  RectifyBlock b;
  int rc = check_info(c, "sf_rectify_plan_create", info, b.iR);
  if (rc != SF_OK || (rc = table_full(c, "sf_rectify_plan_create")) != SF_OK) return rc;
  b.fx = info->K[0]; b.fy = info->K[4]; b.cx = info->K[2]; b.cy = info->K[5];
  for (int k = 0; k < 8; ++k) b.D[k] = (info->model == 0 && k >= 5) ? 0.0 : info->D[k];   // plumb_bob: k1 k2 p1 p2 k3
  SF_HIP(c, hipSetDevice(c->device));
  // the whole table is reserved once: the kernels of earlier calls keep reading valid memory while another entry is written
  if ((rc = sf_buf_reserve(c, c->rect_blocks, (size_t)SF_MAX_RECTIFY_PLANS * sizeof(RectifyBlock))) != SF_OK) return rc;
  const int id = (int)c->rect_plans.size() + 1;
  SF_HIP(c, hipMemcpyAsync((RectifyBlock*)c->rect_blocks.p + (id - 1), &b, sizeof(b), hipMemcpyHostToDevice, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));
  RectifyPlan p;
  p.info = *info;
  p.src_w = info->width; p.src_h = info->height;
  p.out_w = info->out_width ? info->out_width : info->width;
  p.out_h = info->out_height ? info->out_height : info->height;
  c->rect_plans.push_back(std::move(p));
  *plan_out = id;
  return SF_OK;
}

extern "C" int sf_rectify_plan_from_maps(sf_handle c, const float* mapx, const float* mapy, int32_t out_width, int32_t out_height,
                                         int32_t map_pitch, int32_t src_width, int32_t src_height, int32_t* plan_out) {
  if (!c || !plan_out) return SF_EINVAL;
  if (!mapx || !mapy) return sf_fail(c, SF_EINVAL, "sf_rectify_plan_from_maps: a map is missing");
  if (!side_ok(out_width) || !side_ok(out_height) || !side_ok(src_width) || !side_ok(src_height))
    return sf_fail(c, SF_EINVAL, "sf_rectify_plan_from_maps: maps of %d x %d into a source of %d x %d (every side 1 .. %d)", out_width,
                   out_height, src_width, src_height, MAX_SIDE);
  if (map_pitch < 4 * out_width || (map_pitch & 3))
    return sf_fail(c, SF_EINVAL, "sf_rectify_plan_from_maps: map_pitch %d is below a row of %d floats or no multiple of 4", map_pitch, out_width);
  int rc = table_full(c, "sf_rectify_plan_from_maps");
  if (rc != SF_OK) return rc;
  // the fixed-point form of the kernels (k_rectify.hip, rect_fixed): round-half-even of the float32 product
  std::vector<int32_t> table((size_t)out_width * out_height * 2);
  for (int i = 0; i < out_height; ++i) {
    const float* rx = (const float*)((const char*)mapx + (size_t)i * map_pitch);
    const float* ry = (const float*)((const char*)mapy + (size_t)i * map_pitch);
    int32_t* t = table.data() + (size_t)i * out_width * 2;
    for (int j = 0; j < out_width; ++j) {
      const float vx = rx[j] * 32.f, vy = ry[j] * 32.f;
      const bool ok = std::fabs(vx) < 1073741824.f && std::fabs(vy) < 1073741824.f;     // (false for NaN)
      t[2 * j] = ok ? (int32_t)std::nearbyint(vx) : -(1 << 30);
      t[2 * j + 1] = ok ? (int32_t)std::nearbyint(vy) : -(1 << 30);
    }
  }
  SF_HIP(c, hipSetDevice(c->device));
  RectifyPlan p;
  memset(&p.info, 0, sizeof(p.info));
  p.info.width = src_width; p.info.height = src_height; p.info.out_width = out_width; p.info.out_height = out_height;
  p.from_maps = true;
  p.src_w = src_width; p.src_h = src_height; p.out_w = out_width; p.out_h = out_height;
  if ((rc = sf_buf_reserve(c, p.table, table.size() * sizeof(int32_t))) != SF_OK) return rc;
  hipError_t e = hipMemcpyAsync(p.table.p, table.data(), table.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return sf_fail(c, SF_EHIP, "sf_rectify_plan_from_maps: upload -> %s", hipGetErrorString(e));
  p.table_ready = true;
  c->rect_plans.push_back(std::move(p));
  *plan_out = (int32_t)c->rect_plans.size();
  return SF_OK;
}

extern "C" int sf_rectify_plan_count(sf_handle c, int32_t* n_out) {
  if (!c || !n_out) return SF_EINVAL;
  *n_out = (int32_t)c->rect_plans.size();
  return SF_OK;
}

extern "C" int sf_rectify_plan_get(sf_handle c, int32_t plan, sf_camera_info* out, int32_t* from_maps) {
  if (!c || !out) return SF_EINVAL;
  const RectifyPlan* p;
  const int rc = plan_of(c, plan, &p);
  if (rc != SF_OK) return rc;
  *out = p->info;
  if (from_maps) *from_maps = p->from_maps ? 1 : 0;
  return SF_OK;
}

extern "C" int sf_rectify_plan_clear(sf_handle c) {
  if (!c) return SF_EINVAL;
  if (c->rect_plans.empty()) return SF_OK;
  SF_HIP(c, hipSetDevice(c->device));
  SF_HIP(c, hipStreamSynchronize(c->stream));            // the launches queued on the plans' tables
  c->rect_plans.clear();                                 // (each plan's table goes with it)
  return SF_OK;
}

extern "C" int sf_rectify_maps_device(sf_handle c, int32_t plan, float* d_mapx, float* d_mapy, int32_t pitch_bytes) {
  if (!c) return SF_EINVAL;
  const RectifyPlan* p;
  int rc = plan_of(c, plan, &p);
  if (rc != SF_OK) return rc;
  if (p->from_maps) return sf_fail(c, SF_EINVAL, "sf_rectify_maps_device: plan %d holds the caller's maps in fixed point only", plan);
  if (!d_mapx || !d_mapy) return sf_fail(c, SF_EINVAL, "sf_rectify_maps_device: a map array is missing");
  if (pitch_bytes < 4 * p->out_w || (pitch_bytes & 3))
    return sf_fail(c, SF_EINVAL, "sf_rectify_maps_device: pitch of %d bytes is below a row of %d floats or no multiple of 4", pitch_bytes, p->out_w);
  SF_HIP(c, hipSetDevice(c->device));
  return sf_launch_rectify_maps(c, block_of(c, plan), p->out_w, p->out_h, d_mapx, d_mapy, pitch_bytes, nullptr);
}

extern "C" int sf_image_rectify_device(sf_handle c, int32_t plan_a, const uint8_t* d_src_a, int32_t plan_b, const uint8_t* d_src_b,
                                       int32_t format, int32_t out_format, int32_t n_images, int32_t src_pitch, size_t src_stride,
                                       uint8_t* d_dst_a, uint8_t* d_dst_b, int32_t dst_pitch, size_t dst_stride) {
  if (!c || n_images < 0) return SF_EINVAL;
  if (format != SF_IMAGE_RGB8 && format != SF_IMAGE_BGR8 && format != SF_IMAGE_MONO8)
    return sf_fail(c, SF_EINVAL, "sf_image_rectify_device: image format %d unknown (0 = rgb8, 1 = bgr8, 2 = mono8)", format);
  if (out_format != format && !(out_format == SF_IMAGE_MONO8 && format != SF_IMAGE_MONO8))
    return sf_fail(c, SF_EINVAL, "sf_image_rectify_device: out_format %d from format %d (the same, or mono8 from a colour format)",
                   out_format, format);
  const RectifyPlan* pa;
  const RectifyPlan* pb = nullptr;
  int rc = plan_of(c, plan_a, &pa);
  if (rc != SF_OK) return rc;
  const bool two = d_src_b != nullptr;
  if (two) {
    if ((rc = plan_of(c, plan_b, &pb)) != SF_OK) return rc;
    if (pa->src_w != pb->src_w || pa->src_h != pb->src_h || pa->out_w != pb->out_w || pa->out_h != pb->out_h)
      return sf_fail(c, SF_EINVAL, "sf_image_rectify_device: plan %d (%d x %d -> %d x %d) and plan %d (%d x %d -> %d x %d) differ in size",
                     plan_a, pa->src_w, pa->src_h, pa->out_w, pa->out_h, plan_b, pb->src_w, pb->src_h, pb->out_w, pb->out_h);
  }
  if (n_images == 0) return SF_OK;
  if (!d_src_a || !d_dst_a || (two && !d_dst_b)) return sf_fail(c, SF_EINVAL, "sf_image_rectify_device: a source or destination array is missing");
  const long long src_row = (long long)pa->src_w * (format == SF_IMAGE_MONO8 ? 1 : 3);
  const long long dst_row = (long long)pa->out_w * (out_format == SF_IMAGE_MONO8 ? 1 : 3);
  if (src_pitch < src_row) return sf_fail(c, SF_EINVAL, "sf_image_rectify_device: source pitch %d is below a row of %lld bytes", src_pitch, src_row);
  if (dst_pitch < dst_row) return sf_fail(c, SF_EINVAL, "sf_image_rectify_device: destination pitch %d is below a row of %lld bytes", dst_pitch, dst_row);
  if (n_images > 1 && src_stride < (size_t)src_pitch * (pa->src_h - 1) + (size_t)src_row)
    return sf_fail(c, SF_EINVAL, "sf_image_rectify_device: source stride %zu is less than an image (%d rows of pitch %d)", src_stride, pa->src_h, src_pitch);
  if (n_images > 1 && dst_stride < (size_t)dst_pitch * (pa->out_h - 1) + (size_t)dst_row)
    return sf_fail(c, SF_EINVAL, "sf_image_rectify_device: destination stride %zu is less than an image (%d rows of pitch %d)", dst_stride, pa->out_h, dst_pitch);
  if ((long long)n_images * (two ? 2 : 1) > 65535)
    return sf_fail(c, SF_ERANGE, "sf_image_rectify_device: %d images per array (at most 65535 in one call, both arrays together)", n_images);
  SF_HIP(c, hipSetDevice(c->device));
  const bool table = c->rect_table || pa->from_maps || (pb && pb->from_maps);
  if (table) {
    if ((rc = table_ready(c, plan_a)) != SF_OK) return rc;
    if (two && (rc = table_ready(c, plan_b)) != SF_OK) return rc;
  }
  RectifyImages im;
  im.src_a = d_src_a; im.src_b = two ? d_src_b : d_src_a;
  im.dst_a = d_dst_a; im.dst_b = two ? d_dst_b : d_dst_a;
  im.n_a = n_images; im.n_b = two ? n_images : 0;
  im.src_w = pa->src_w; im.src_h = pa->src_h; im.out_w = pa->out_w; im.out_h = pa->out_h;
  im.src_pitch = src_pitch; im.dst_pitch = dst_pitch;
  im.src_stride = n_images > 1 ? src_stride : 0; im.dst_stride = n_images > 1 ? dst_stride : 0;
  const int id_b = two ? plan_b : plan_a;
  const RectifyPlan& qa = c->rect_plans[plan_a - 1];
  const RectifyPlan& qb = c->rect_plans[id_b - 1];
  return sf_launch_rectify(c, im, format, out_format, c->gray_rule, block_of(c, plan_a), block_of(c, id_b),
                           table ? (const int32_t*)qa.table.p : nullptr, table ? (const int32_t*)qb.table.p : nullptr);
}

extern "C" int sf_stereo_camera_from_info(const sf_camera_info* left, const sf_camera_info* right, const float local_transform[12],
                                          sf_stereo_camera* out) {
  if (!left || !right || !out) return SF_EINVAL;
  const double baseline = -right->P[3] / right->P[0];
  if (!(baseline > 0.0) || !std::isfinite(baseline))
    return sf_fail(nullptr, SF_EINVAL, "sf_stereo_camera_from_info: baseline -P_right[3] / P_right[0] = %g is not > 0", baseline);
  static const float identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  memset(out, 0, sizeof(*out));
  out->fx = (float)left->P[0]; out->fy = (float)left->P[5]; out->cx = (float)left->P[2]; out->cy = (float)left->P[6];
  out->cx_right = (float)right->P[2];
  out->baseline = (float)baseline;
  memcpy(out->local_transform, local_transform ? local_transform : identity, sizeof(out->local_transform));
  return SF_OK;
}
