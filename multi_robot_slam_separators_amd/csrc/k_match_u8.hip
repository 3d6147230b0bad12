// k_match_u8.hip -- pass-1 GLOBAL matching of uint8 descriptor rows compared by L2 (desc_type 2: SIFT rows, 128 bytes).
//
// A row holds 128 integers in 0 .. 255, so the oracle's float32 distance (the ordered, unfused sum of 128 squared
// differences, desc_type 1 on the float twin) is an integer below 2^24 and exact in any order: the kNN-2 scan is an integer
// dot-product problem and runs on the int8 matrix cores.
//   * operands: x - 128 (XOR 0x80 per byte) as signed int8; differences are unchanged by the shift;
//   * d^2 = |f|^2 + |t|^2 - 2 f.t in int32 (|dot| and the norms <= 128 x 128^2, d^2 <= 128 x 255^2 = 8 323 200); the norms
//     come from the rows the kernel has loaded, nothing is kept per keyframe;
//   * v_mfma_i32_16x16x64_i8, two k-steps per 16 x 16 tile.  "from" rows are the A operand (staged in LDS, FB rows at a
//     time, 144-byte pitch: a wavefront's 64 16-byte fragment reads cover the banks once), "to" rows the B operand
//     (registers, loaded once per 512 "to" rows).  A lane's bytes: row lane & 15, bytes 16 (lane >> 4) .. + 15 of each
//     64-byte half, the SAME bytes for A and B, so whichever k the hardware gives them the products pair up.  C/D: column
//     (= "to" row) lane & 15, row (= "from" row) 4 (lane >> 4) + register: a lane's four results are four "from" rows
//     against its one "to" row, in ascending order tile after tile, so (best, second best, best index) is the sequential
//     scan of that lane's quarter of the rows; the four quarters are merged once per "to" row with two lane exchanges;
//   * ties as knn2_scan_l2 (k_match.hip): strict comparisons, of equal distances the lower "from" index is best, the
//     second best is the next distance (equal to the best where the best occurs twice).  The merge compares
//     (distance, index) as two fields: a packed key would need 23 + 12 bits.
// Everything around the scan -- the cnt / owner bookkeeping, the compaction, the gates, the survivor list -- is
// match_slot_outside / match_begin / match_claim / match_finish (sf_match_device.hpp), the calls k_match_global makes.
// No float arithmetic besides the accept test (both conversions exact), so no -ffp-contract=off.
#include <climits>

#include "sf_internal.hpp"
#include "sf_match_device.hpp"

namespace {

using i32x4 = __attribute__((ext_vector_type(4))) int;

constexpr int U8_W = 32;                 // dwords per row
constexpr int U8_PITCH = 36;             // dwords per staged "from" row in LDS
constexpr int U8_NT = 256;               // threads per workgroup (one workgroup per pair)
constexpr int U8_NTT = 8;                // "to" tiles of 16 rows per wavefront and sweep: 4 x 8 x 16 = 512 "to" rows
constexpr int U8_PAD = 0x50000000;       // "norm" of the rows that pad the last tile: never the best of a real row
constexpr int U8_NONE = 0x40000000;      // what is at least this is a padding row's

__device__ __forceinline__ int dot4_self(uint32_t v, int acc) {
  const int a = (int)(int8_t)(v & 255u), b = (int)(int8_t)((v >> 8) & 255u), c = (int)(int8_t)((v >> 16) & 255u),
            d = (int)(int8_t)(v >> 24);
  return acc + a * a + b * b + c * c + d * d;
}
__device__ __forceinline__ int norm4(const uint4& v, int acc) {
  return dot4_self(v.w, dot4_self(v.z, dot4_self(v.y, dot4_self(v.x, acc))));
}
__device__ __forceinline__ uint4 shift128(uint4 v) {
  v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
  return v;
}
__device__ __forceinline__ i32x4 as_frag(const uint4& v) {
  i32x4 r;
  r[0] = (int)v.x; r[1] = (int)v.y; r[2] = (int)v.z; r[3] = (int)v.w;
  return r;
}

// kNN-2 of every "to" row over the "from" rows; finish(t, d1, d2, i1) is called once per "to" row t < Kt by one lane:
// d1 / d2 the best / second-best squared distance (INT_MAX where there is none), i1 the best's "from" row (-1: none).
// fnorm: [FB] ints, frow: [FB][U8_PITCH] dwords of LDS, 16-byte aligned; FB a multiple of 16, at most U8_NT.
// Every thread of the workgroup calls it (barriers inside).
template <class Finish>
__device__ __forceinline__ void knn2_scan_u8(const uint32_t* __restrict__ dF, int Kf, const uint32_t* __restrict__ dT, int Kt,
                                             int FB, int* fnorm, uint32_t* frow, Finish&& finish) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, g = lane >> 4;
  for (int tb = 0; tb < Kt; tb += 4 * U8_NTT * 16) {
    // this wavefront's tiles: "to" rows wt0 + 64 j .. + 15 (the four wavefronts interleaved, so a short frame spreads)
    const int wt0 = tb + wave * 16;
    const int ntiles = wt0 < Kt ? min(U8_NTT, (Kt - wt0 + 63) / 64) : 0;   // wave-uniform
    i32x4 b0[U8_NTT], b1[U8_NTT];
    int nT[U8_NTT], d1[U8_NTT], d2[U8_NTT], i1[U8_NTT];
#pragma unroll
    for (int j = 0; j < U8_NTT; ++j) {
      const int t = wt0 + 64 * j + col;
      const uint4* p = reinterpret_cast<const uint4*>(dT + (size_t)(t < Kt ? t : 0) * U8_W);
      const uint4 v0 = shift128(p[g]), v1 = shift128(p[4 + g]);
      b0[j] = as_frag(v0); b1[j] = as_frag(v1);
      int n = norm4(v1, norm4(v0, 0));
      n += __shfl_xor(n, 16);
      n += __shfl_xor(n, 32);
      nT[j] = n;
      d1[j] = INT_MAX; d2[j] = INT_MAX; i1[j] = -1;
    }
    for (int fb = 0; fb < Kf; fb += FB) {
      const int nrows = min(FB, Kf - fb), nr16 = (nrows + 15) & ~15;
      __syncthreads();                                     // (the block before this one has been read)
      for (int u = tid; u < nr16 * 8; u += U8_NT) {
        const int r = u >> 3, q = u & 7;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (r < nrows) v = shift128(reinterpret_cast<const uint4*>(dF + (size_t)(fb + r) * U8_W)[q]);
        *reinterpret_cast<uint4*>(frow + r * U8_PITCH + 4 * q) = v;
      }
      __syncthreads();
      for (int r = tid; r < nr16; r += U8_NT) {
        int n = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) n = norm4(*reinterpret_cast<const uint4*>(frow + r * U8_PITCH + 4 * q), n);
        fnorm[r] = r < nrows ? n : U8_PAD;
      }
      __syncthreads();
      for (int ft = 0; ft < nr16; ft += 16) {
        const uint32_t* ar = frow + (ft + col) * U8_PITCH + 4 * g;
        const i32x4 a0 = as_frag(*reinterpret_cast<const uint4*>(ar));
        const i32x4 a1 = as_frag(*reinterpret_cast<const uint4*>(ar + 16));
        const int4 nf4 = *reinterpret_cast<const int4*>(fnorm + ft + 4 * g);
        const int nf[4] = {nf4.x, nf4.y, nf4.z, nf4.w};
        const int f0 = fb + ft + 4 * g;
#pragma unroll
        for (int j = 0; j < U8_NTT; ++j) {
          if (j < ntiles) {
            i32x4 acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0[j], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1[j], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int s = nf[r] - 2 * acc[r];            // (the "to" row's norm is the same for all: added at the end)
              if (s < d1[j]) { d2[j] = d1[j]; d1[j] = s; i1[j] = f0 + r; }
              else if (s < d2[j]) { d2[j] = s; }
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < U8_NTT; ++j) {
      if (j < ntiles) {
        int a1 = d1[j], a2 = d2[j], ai = i1[j];
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {         // the four quarters of the "from" rows
          const int o1 = __shfl_xor(a1, off), o2 = __shfl_xor(a2, off), oi = __shfl_xor(ai, off);
          const bool other = o1 < a1 || (o1 == a1 && oi < ai);
          a2 = other ? min(o2, a1) : min(a2, o1);
          ai = other ? oi : ai;
          a1 = other ? o1 : a1;
        }
        if (a1 >= U8_NONE) { a1 = INT_MAX; ai = -1; } else { a1 += nT[j]; }
        if (a2 >= U8_NONE) a2 = INT_MAX; else a2 += nT[j];
        const int t = wt0 + 64 * j + col;
        if (g == 0 && t < Kt) finish(t, a1, a2, ai);
      }
    }
  }
}

__global__ void __launch_bounds__(U8_NT)
k_match_global_u8(StoreView st, const int32_t* __restrict__ pair_from, const int32_t* __restrict__ pair_to, float nndr,
                  int min_inliers, int est, int FB, uint32_t* __restrict__ corr, CorrHeader* __restrict__ hdr,
                  PassState* __restrict__ pass, int32_t* __restrict__ list, int32_t* __restrict__ counter) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  const int pair = blockIdx.x;
  const int kcap = st.kcap;
  MatchPair M;
  if (match_slot_outside(st, pair_from[pair], pair_to[pair])) { match_report_outside(hdr[pair], pass[pair]); return; }
  match_begin<U8_NT>(st, pair_from[pair], pair_to[pair], smem, M);
  const int Kf = M.mF.x, Kt = M.mT.x;
  const uint32_t* dF = st.desc + (size_t)M.sF * kcap * U8_W;
  const uint32_t* dT = st.desc + (size_t)M.sT * kcap * U8_W;
  int* fnorm = M.misc + 16;      // [FB]   norms of the staged "from" rows, behind the bookkeeping
  uint32_t* frow = reinterpret_cast<uint32_t*>(fnorm + FB);   // [FB][U8_PITCH]
  __syncthreads();

  int rejected = 0;
  if (Kf > 0) {
    knn2_scan_u8(dF, Kf, dT, Kt, FB, fnorm, frow, [&](int t, int d1, int d2, int i1) {
      const bool acc = (Kf >= 2) && i1 >= 0 && !((float)d1 > nndr * (float)d2);
      if (acc) match_claim(M.cnt, M.owner, i1, t);
      else ++rejected;
    });
  }
  match_finish<U8_NT>(st, pair, M, min_inliers, est, rejected, corr + (size_t)pair * kcap, hdr[pair], pass[pair], list,
                      counter);
}

// the scan alone, one pair: what it found per "to" row (sf_debug_knn2_u8)
__global__ void __launch_bounds__(U8_NT)
k_knn2_u8_debug(StoreView st, int sF, int sT, int FB, int32_t* __restrict__ d_best, int32_t* __restrict__ d_second,
                int32_t* __restrict__ i_best) {
  extern __shared__ __attribute__((aligned(16))) int smem[];
  const int Kf = st.meta[sF].x, Kt = st.meta[sT].x;
  const uint32_t* dF = st.desc + (size_t)sF * st.kcap * U8_W;
  const uint32_t* dT = st.desc + (size_t)sT * st.kcap * U8_W;
  int* fnorm = smem;
  uint32_t* frow = reinterpret_cast<uint32_t*>(fnorm + FB);
  knn2_scan_u8(dF, Kf, dT, Kt, FB, fnorm, frow, [&](int t, int d1, int d2, int i1) {
    d_best[t] = d1; d_second[t] = d2; i_best[t] = i1;
  });
}

// "from" rows staged per block: 256 while the pair's LDS stays within the 64 KB a launch gets without asking, else 128
int u8_block_rows(int kcap) { return ((size_t)(2 * kcap + 16) * 4 + 256 * (U8_PITCH + 1) * 4 <= 64 * 1024) ? 256 : 128; }

}  // namespace

int sf_launch_match_global_u8(sf_context* c, StoreView st, const int32_t* d_from, const int32_t* d_to, int n) {
  if (n <= 0) return SF_OK;
  if (st.w != U8_W) return sf_fail(c, SF_EINVAL, "uint8 L2 rows are %d dwords, the store holds %d", U8_W, st.w);
  const int FB = u8_block_rows(st.kcap);
  const size_t lds = (size_t)(2 * st.kcap + 16 + FB * (U8_PITCH + 1)) * sizeof(int);
  sf_prof_begin(c, SF_K_MATCH);
  sf_launch_pass1(c, k_match_global_u8, U8_NT, lds, st, d_from, d_to, n, FB);
  sf_prof_end(c, SF_K_MATCH);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

extern "C" int sf_debug_knn2_u8(sf_handle c, int32_t slot_from, int32_t slot_to, int32_t* d_best, int32_t* d_second,
                                int32_t* i_best) {
  if (!c || !d_best || !d_second || !i_best) return SF_EINVAL;
  if (c->params.desc_type != 2) return sf_fail(c, SF_EINVAL, "sf_debug_knn2_u8 needs a handle with desc_type 2, not %d", c->params.desc_type);
  const Store& s = c->store;
  if (slot_from < 0 || slot_from >= s.slots || slot_to < 0 || slot_to >= s.slots)
    return sf_fail(c, SF_EINVAL, "sf_debug_knn2_u8: slots %d, %d outside the store's %d", slot_from, slot_to, s.slots);
  SF_HIP(c, hipSetDevice(c->device));
  (void)sf_lanes_touch(c, false);
  const StoreView st = sf_store_view(s);
  int4 meta;
  SF_HIP(c, hipMemcpyAsync(&meta, st.meta + slot_to, sizeof(meta), hipMemcpyDeviceToHost, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));
  const int Kt = meta.x;
  if (Kt <= 0) return SF_OK;
  if (Kt > st.kcap) return sf_fail(c, SF_EINVAL, "sf_debug_knn2_u8: slot %d holds %d rows of %d", slot_to, Kt, st.kcap);
  int32_t* d = nullptr;
  SF_HIP(c, hipMalloc((void**)&d, (size_t)3 * Kt * sizeof(int32_t)));
  const int FB = u8_block_rows(st.kcap);
  hipLaunchKernelGGL(k_knn2_u8_debug, dim3(1), dim3(U8_NT), (size_t)FB * (U8_PITCH + 1) * sizeof(int), c->stream, st, slot_from,
                     slot_to, FB, d, d + Kt, d + 2 * Kt);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(d_best, d, (size_t)Kt * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_second, d + Kt, (size_t)Kt * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(i_best, d + 2 * Kt, (size_t)Kt * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return sf_fail(c, SF_EHIP, "sf_debug_knn2_u8 -> %s", hipGetErrorString(e));
  return SF_OK;
}
