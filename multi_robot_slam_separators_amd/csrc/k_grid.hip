// k_grid.hip -- the cell loop of rtabmap's Feature2D::generateKeypoints (Vis/GridRows x Vis/GridCols): the ROI is cut into
// rows x cols cells of one size, the detector runs on every cell as an image of its own and keeps `quota` keypoints there,
// and the cells' lists are joined in row-major cell order with the cell's origin added.  The detectors run the cells as
// the images of one batch launch (SfCells: k_fast.hip, k_gftt.hip); this file joins what they left.  The upstream text is
// not in the reference tree: the semantics are restated in tests/grid_ref.py.
//
//   k_grid_gather   one wavefront (a workgroup of 64) per keyframe.  An exclusive scan of the keyframe's rows * cols cell
//                   counts (64 per pass, wave_scan_add, the carry in a scalar) leaves every cell's count and first output
//                   row in LDS.  Then the rows * cols * quota record slots of the cells are walked 64 at a time: the lane
//                   whose slot holds a keypoint copies the 28-byte record (seven dword loads and stores, no byte
//                   access) to its place and adds the cell's origin -- ROI offset included -- to x and y.  Both are whole
//                   numbers in float, so the sum is exact and equals the shift k_corner_subpix applies for a ROI.  Lane
//                   0 writes the keyframe's count.  LDS: 2 KB.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_device_math.hpp"
#include "sf_internal.hpp"

namespace {

constexpr int GRID_MAX_CELLS = 16 * 16;      // sf_grid_set_params: 1 .. 16 each way

struct GridKp { uint32_t w[7]; };            // sf_keypoint as the dwords it is moved by
static_assert(sizeof(GridKp) == sizeof(sf_keypoint), "sf_keypoint is seven dwords");

__global__ void __launch_bounds__(64)
k_grid_gather(const GridKp* __restrict__ cell_kpts, const int32_t* __restrict__ cell_n, int cells, int cols, int quota, int x0,
              int y0, int col_size, int row_size, GridKp* __restrict__ kpts, int rows_cap, int32_t* __restrict__ n_out) {
  __shared__ int s_cnt[GRID_MAX_CELLS], s_off[GRID_MAX_CELLS];
  const int lane = threadIdx.x;
  cell_n += (size_t)blockIdx.x * cells;
  cell_kpts += (size_t)blockIdx.x * cells * quota;
  kpts += (size_t)blockIdx.x * rows_cap;
  int total = 0;
  for (int base = 0; base < cells; base += 64) {           // (a wave-uniform loop: all 64 lanes active in the scan)
    const int q = base + lane;
    const int cnt = q < cells ? min(max(cell_n[q], 0), quota) : 0;
    const int incl = sfd::wave_scan_add(cnt);
    if (q < cells) { s_cnt[q] = cnt; s_off[q] = total + incl - cnt; }
    total += __builtin_amdgcn_readlane(incl, 63);
  }
  __syncthreads();
  if (lane == 0) n_out[blockIdx.x] = total;
  const int slots = cells * quota;                         // = rows_cap: every output row below lies inside the list
  for (int s = lane; s < slots; s += 64) {
    const int q = s / quota, r = s - q * quota;
    if (r >= s_cnt[q]) continue;
    const int i = q / cols, j = q - i * cols;
    GridKp k = cell_kpts[s];
    k.w[0] = __float_as_uint(__uint_as_float(k.w[0]) + (float)(x0 + j * col_size));
    k.w[1] = __float_as_uint(__uint_as_float(k.w[1]) + (float)(y0 + i * row_size));
    kpts[s_off[q] + r] = k;
  }
}

}  // namespace

int sf_launch_grid_gather(sf_context* c, const sf_keypoint* d_cell_kpts, const int32_t* d_cell_n, int n_img, int rows, int cols,
                          int quota, int x0, int y0, int col_size, int row_size, sf_keypoint* d_kpts, int rows_cap, int32_t* d_n) {
  const int cells = rows * cols;
  if (n_img <= 0) return SF_OK;
  if (cells < 1 || cells > GRID_MAX_CELLS || quota < 1 || (long long)cells * quota != rows_cap)
    return sf_fail(c, SF_EINVAL, "grid of %d x %d cells with %d keypoints apiece into lists of %d rows", rows, cols, quota, rows_cap);
  hipLaunchKernelGGL(k_grid_gather, dim3(n_img), dim3(64), 0, c->stream, (const GridKp*)d_cell_kpts, d_cell_n, cells, cols, quota, x0,
                     y0, col_size, row_size, (GridKp*)d_kpts, rows_cap, d_n);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
