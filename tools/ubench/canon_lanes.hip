// The register-resident lane exchanges of sf_device_math.hpp (v_permlane32_swap / v_permlane16_swap / DPP moves) against
// the __shfl_xor form they replace, on the device:
//   1. directions: with lane numbers as payload, every distance 1 .. 8 of lane_xor_dpp returns the value of lane ^ off
//      and lane_swap<32 / 16> trades exactly the registers its comment says (32-bit and both words of a double);
//   2. sums: block_sum_canon (256 threads, and one wavefront over zeroed rows 1 .. 3) and canon_reduce on 1 / 2 / 4
//      wavefronts, register form, bit-equal to the reference below for N = 1, 2, 3, 6, 11, 16, 28 -- random doubles over
//      the whole exponent range, +-0, denormals, +-inf; where the reference's total is a NaN only NaN-ness is compared;
//   3. integers: wave_scan_add / wave_scan_max / wave_sum / wave_max against values computed on the host.
// The reference (namespace ref) is a verbatim copy of the form this project shipped before the register form.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-vectorize -fno-slp-vectorize tools/ubench/canon_lanes.hip -o canon_lanes
// prints one line per group and "canon_lanes: PASS" (exit status 0) or the first mismatches (exit status 1).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../multi_robot_slam_separators_amd/csrc/sf_device_math.hpp"

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

namespace ref {
template <int C>
__device__ __forceinline__ void sum_stage(double (&w)[32], int& idx, int lane, int off) {
  if constexpr (C > 1) {
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int k = 0; k < C / 2; ++k) {
      const double send = up ? w[k] : w[k + C / 2];
      const double keep = up ? w[k + C / 2] : w[k];
      w[k] = keep + __shfl_xor(send, off);
    }
    idx += up ? C / 2 : 0;
  } else {
    w[0] = w[0] + __shfl_xor(w[0], off);
  }
}

template <int N, int STRIDE>
__device__ __forceinline__ void block_sum_canon(double (&v)[N], double* red, int tid) {
  static_assert(N >= 1 && N <= 32 && STRIDE >= N, "at most 32 values");
  constexpr int P = N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : N <= 16 ? 16 : 32;
  static_assert(STRIDE >= P, "scratch rows must hold the padded count");
  const int lane = tid & 63, wave = tid >> 6;
  double w[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) w[k] = k < N ? v[k] : 0.0;
  int idx = 0;
  sum_stage<P>(w, idx, lane, 32);
  sum_stage<(P / 2 > 1 ? P / 2 : 1)>(w, idx, lane, 16);
  sum_stage<(P / 4 > 1 ? P / 4 : 1)>(w, idx, lane, 8);
  sum_stage<(P / 8 > 1 ? P / 8 : 1)>(w, idx, lane, 4);
  sum_stage<(P / 16 > 1 ? P / 16 : 1)>(w, idx, lane, 2);
  sum_stage<(P / 32 > 1 ? P / 32 : 1)>(w, idx, lane, 1);
  __syncthreads();  // previous users of `red` are done
  red[wave * STRIDE + idx] = w[0];   // every lane of a group holds the same total: identical writes
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = ((red[k] + red[STRIDE + k]) + red[2 * STRIDE + k]) + red[3 * STRIDE + k];
}
}  // namespace ref

// ---- 1. directions -----------------------------------------------------------------------------------------------------
// out[0..4)[64]: lane_xor_dpp<1, 2, 4, 8>(lane); out[4..8)[64]: a, b after lane_swap<32>, a, b after lane_swap<16> of
// (a, b) = (lane, 64 + lane); out[8..12)[64] (64-bit): the same four through the double overloads of lane_swap with
// both words carrying the lane, and out64[4..8): lane_xor_dpp<1, 2, 4, 8> of such a double.
__device__ __forceinline__ double tag(int hi_base, int lane) { return __hiloint2double(hi_base + lane, 0x1000 + lane); }
__global__ void k_directions(int* out, unsigned long long* out64) {
  const int lane = threadIdx.x;
  out[0 * 64 + lane] = sfd::lane_xor_dpp<1>(lane);
  out[1 * 64 + lane] = sfd::lane_xor_dpp<2>(lane);
  out[2 * 64 + lane] = sfd::lane_xor_dpp<4>(lane);
  out[3 * 64 + lane] = sfd::lane_xor_dpp<8>(lane);
  unsigned a = lane, b = 64 + lane;
  sfd::lane_swap<32>(a, b);
  out[4 * 64 + lane] = (int)a; out[5 * 64 + lane] = (int)b;
  a = lane; b = 64 + lane;
  sfd::lane_swap<16>(a, b);
  out[6 * 64 + lane] = (int)a; out[7 * 64 + lane] = (int)b;
  double da = tag(0x40000000, lane), db = tag(0x40000040, lane);
  sfd::lane_swap<32>(da, db);
  out64[0 * 64 + lane] = (unsigned long long)__double_as_longlong(da);
  out64[1 * 64 + lane] = (unsigned long long)__double_as_longlong(db);
  da = tag(0x40000000, lane); db = tag(0x40000040, lane);
  sfd::lane_swap<16>(da, db);
  out64[2 * 64 + lane] = (unsigned long long)__double_as_longlong(da);
  out64[3 * 64 + lane] = (unsigned long long)__double_as_longlong(db);
  const double d = tag(0x40000000, lane);
  out64[4 * 64 + lane] = (unsigned long long)__double_as_longlong(sfd::lane_xor_dpp<1>(d));
  out64[5 * 64 + lane] = (unsigned long long)__double_as_longlong(sfd::lane_xor_dpp<2>(d));
  out64[6 * 64 + lane] = (unsigned long long)__double_as_longlong(sfd::lane_xor_dpp<4>(d));
  out64[7 * 64 + lane] = (unsigned long long)__double_as_longlong(sfd::lane_xor_dpp<8>(d));
}

// ---- 2. sums -----------------------------------------------------------------------------------------------------------
constexpr int STRIDE = 32;
constexpr int MAXN = 28;
constexpr int M_MAX = 700;                      // elements of the canon_reduce cases
// FORM 0: the reference; 1: the register form; 2: the __shfl_xor form kept selectable in sf_device_math.hpp.
// in: [blockDim.x][MAXN]; out: [blockDim.x][N] (every thread's copy of the totals).  One wavefront: rows 1 .. 3 of `red`
// hold +0.0, as they do for the wavefronts without an element.
template <int N, int FORM>
__global__ void k_block_sum(const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double red[4 * STRIDE];
  const int tid = threadIdx.x;
  for (int i = tid; i < 4 * STRIDE; i += blockDim.x) red[i] = 0.0;
  __syncthreads();
  double v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = in[tid * MAXN + k];
  if constexpr (FORM == 0) ref::block_sum_canon<N, STRIDE>(v, red, tid);
  else sfd::block_sum_canon<N, STRIDE, FORM == 1>(v, red, tid);
#pragma unroll
  for (int k = 0; k < N; ++k) out[tid * N + k] = v[k];
}

// canon_reduce over m elements ([M_MAX][MAXN]) on NW wavefronts (NW = 0: the reference -- strided partials of 256
// threads, then ref::block_sum_canon).  out: [64 * max(NW, 4 for the reference)][N].
template <int N, int NW>
__global__ void k_reduce(const double* __restrict__ in, int m, double* __restrict__ out) {
  __shared__ double red[4 * STRIDE];
  const int tid = threadIdx.x;
  double v[N];
  if constexpr (NW == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = 0.0;
    for (int i = tid; i < m; i += 256)
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] += in[i * MAXN + k];
    ref::block_sum_canon<N, STRIDE>(v, red, tid);
  } else {
    sfd::canon_reduce<N, STRIDE, NW, true>(m, tid, red, v, [&](int i, double (&a)[N]) {
#pragma unroll
      for (int k = 0; k < N; ++k) a[k] += in[i * MAXN + k];
    });
  }
#pragma unroll
  for (int k = 0; k < N; ++k) out[tid * N + k] = v[k];
}

// ---- 3. integers ---------------------------------------------------------------------------------------------------------
// in: [256] ints, in64: [256]; out: [5][256] = scan_add, scan_max, sum, max per thread; out64: [256] = 64-bit sum
__global__ void k_ints(const int* __restrict__ in, const unsigned long long* __restrict__ in64, int* __restrict__ out,
                       unsigned long long* __restrict__ out64) {
  const int tid = threadIdx.x;
  const int x = in[tid];
  out[0 * 256 + tid] = sfd::wave_scan_add(x);
  out[1 * 256 + tid] = sfd::wave_scan_max(x);
  out[2 * 256 + tid] = sfd::wave_sum(x);
  out[3 * 256 + tid] = sfd::wave_max(x);
  out64[tid] = sfd::wave_sum(in64[tid]);
}

// ---- host --------------------------------------------------------------------------------------------------------------
static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
  rng_state += 0x9E3779B97F4A7C15ull;
  uint64_t z = rng_state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double from_bits(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static uint64_t to_bits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }
static bool is_nan_bits(uint64_t b) { return (b & 0x7FF0000000000000ull) == 0x7FF0000000000000ull && (b & 0x000FFFFFFFFFFFFFull) != 0; }

// kind 0: any finite double (exponent field 0 .. 2046: denormals included); 1: exponents near 1 (every addition rounds);
// 2: kind 1 with +-0, denormals and +inf sprinkled in; 3: kind 0 with +inf and -inf (NaN totals); 4: +-0 and denormals only
static double draw(int kind) {
  const uint64_t r = rnd();
  const uint64_t sign = r & 0x8000000000000000ull, frac = r & 0x000FFFFFFFFFFFFFull;
  const uint64_t pick = (r >> 52) & 0x7FF;
  auto near1 = [&]() { return from_bits(sign | ((uint64_t)(1023 - 20 + pick % 41) << 52) | frac); };
  switch (kind) {
    case 0: return from_bits(sign | ((uint64_t)(pick % 2047) << 52) | frac);
    case 1: return near1();
    case 2: {
      const unsigned s = (unsigned)(rnd() % 16);
      if (s == 0) return from_bits(sign);                          // +-0
      if (s == 1) return from_bits(sign | frac);                   // a denormal
      if (s == 2 && (rnd() % 8) == 0) return from_bits(0x7FF0000000000000ull);   // +inf, rarely
      return near1();
    }
    case 3: {
      const unsigned s = (unsigned)(rnd() % 64);
      if (s == 0) return from_bits(sign | 0x7FF0000000000000ull);  // +-inf
      return from_bits(sign | ((uint64_t)(pick % 2047) << 52) | frac);
    }
    default: return (rnd() & 1) ? from_bits(sign) : from_bits(sign | frac);
  }
}

// got against want, bit for bit; a NaN in `want` asks for a NaN only
static int compare(const char* what, int n_case, int kind, const std::vector<double>& got, const std::vector<double>& want,
                   size_t n, int& printed) {
  int bad = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t g = to_bits(got[i]), w = to_bits(want[i]);
    const bool ok = is_nan_bits(w) ? is_nan_bits(g) : g == w;
    if (!ok) {
      ++bad;
      if (printed < 12) { printf("  MISMATCH %s N=%d data=%d word %zu: got %016llx want %016llx\n", what, n_case, kind, i,
                                 (unsigned long long)g, (unsigned long long)w); ++printed; }
    }
  }
  return bad;
}

template <int N>
static int run_sums(double* d_in, double* d_out, int& printed, int& n_nan, int& n_words) {
  int bad = 0;
  std::vector<double> h_in((size_t)M_MAX * MAXN), want(256 * N), got(256 * N);
  for (int kind = 0; kind < 5; ++kind) {
    for (auto& x : h_in) x = draw(kind);
    CHECK(hipMemcpy(d_in, h_in.data(), h_in.size() * 8, hipMemcpyHostToDevice));
    // block_sum_canon: 256 threads, then one wavefront
    for (int nt : {256, 64}) {
      hipLaunchKernelGGL((k_block_sum<N, 0>), dim3(1), dim3(nt), 0, 0, d_in, d_out);
      CHECK(hipMemcpy(want.data(), d_out, (size_t)nt * N * 8, hipMemcpyDeviceToHost));
      for (size_t i = 0; i < (size_t)nt * N; ++i) n_nan += is_nan_bits(to_bits(want[i])) ? 1 : 0;
      n_words += nt * N;
      hipLaunchKernelGGL((k_block_sum<N, 1>), dim3(1), dim3(nt), 0, 0, d_in, d_out);
      CHECK(hipMemcpy(got.data(), d_out, (size_t)nt * N * 8, hipMemcpyDeviceToHost));
      bad += compare(nt == 256 ? "block_sum_canon/256" : "block_sum_canon/64", N, kind, got, want, (size_t)nt * N, printed);
      hipLaunchKernelGGL((k_block_sum<N, 2>), dim3(1), dim3(nt), 0, 0, d_in, d_out);
      CHECK(hipMemcpy(got.data(), d_out, (size_t)nt * N * 8, hipMemcpyDeviceToHost));
      bad += compare(nt == 256 ? "kept shfl form/256" : "kept shfl form/64", N, kind, got, want, (size_t)nt * N, printed);
    }
    // canon_reduce at the element counts where a wavefront of the canonical scheme runs empty, partly filled, or loops
    for (int m : {3, 64, 65, 129, 200, 256, 257, M_MAX}) {
      hipLaunchKernelGGL((k_reduce<N, 0>), dim3(1), dim3(256), 0, 0, d_in, m, d_out);
      CHECK(hipMemcpy(want.data(), d_out, (size_t)256 * N * 8, hipMemcpyDeviceToHost));
      hipLaunchKernelGGL((k_reduce<N, 4>), dim3(1), dim3(256), 0, 0, d_in, m, d_out);
      CHECK(hipMemcpy(got.data(), d_out, (size_t)256 * N * 8, hipMemcpyDeviceToHost));
      bad += compare("canon_reduce/4", N, kind, got, want, (size_t)256 * N, printed);
      hipLaunchKernelGGL((k_reduce<N, 2>), dim3(1), dim3(128), 0, 0, d_in, m, d_out);
      CHECK(hipMemcpy(got.data(), d_out, (size_t)128 * N * 8, hipMemcpyDeviceToHost));
      bad += compare("canon_reduce/2", N, kind, got, want, (size_t)128 * N, printed);
      hipLaunchKernelGGL((k_reduce<N, 1>), dim3(1), dim3(64), 0, 0, d_in, m, d_out);
      CHECK(hipMemcpy(got.data(), d_out, (size_t)64 * N * 8, hipMemcpyDeviceToHost));
      bad += compare("canon_reduce/1", N, kind, got, want, (size_t)64 * N, printed);
    }
  }
  printf("sums N=%2d: %s\n", N, bad ? "FAIL" : "ok");
  return bad ? 1 : 0;
}

int main() {
  int fails = 0, printed = 0;
  // 1. directions
  {
    int* d32; unsigned long long* d64;
    CHECK(hipMalloc(&d32, 8 * 64 * 4));
    CHECK(hipMalloc(&d64, 8 * 64 * 8));
    hipLaunchKernelGGL(k_directions, dim3(1), dim3(64), 0, 0, d32, d64);
    std::vector<int> h32(8 * 64);
    std::vector<unsigned long long> h64(8 * 64);
    CHECK(hipMemcpy(h32.data(), d32, h32.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(h64.data(), d64, h64.size() * 8, hipMemcpyDeviceToHost));
    auto tagbits = [](unsigned hi_base, int lane) { return ((unsigned long long)(hi_base + lane) << 32) | (unsigned)(0x1000 + lane); };
    int bad = 0;
    const int offs[4] = {1, 2, 4, 8};
    for (int lane = 0; lane < 64; ++lane) {
      for (int s = 0; s < 4; ++s) {
        if (h32[s * 64 + lane] != (lane ^ offs[s])) { ++bad; if (printed++ < 12) printf("  lane_xor_dpp<%d> lane %d reads lane %d\n", offs[s], lane, h32[s * 64 + lane]); }
        if (h64[(4 + s) * 64 + lane] != tagbits(0x40000000u, lane ^ offs[s])) { ++bad; if (printed++ < 12) printf("  lane_xor_dpp<%d>(double) lane %d got %016llx\n", offs[s], lane, h64[(4 + s) * 64 + lane]); }
      }
      for (int s = 0; s < 2; ++s) {
        const int off = s == 0 ? 32 : 16;
        const bool up = (lane & off) != 0;
        const int want_a = up ? 64 + (lane ^ off) : lane, want_b = up ? 64 + lane : (lane ^ off);
        if (h32[(4 + 2 * s) * 64 + lane] != want_a || h32[(5 + 2 * s) * 64 + lane] != want_b) {
          ++bad;
          if (printed++ < 12) printf("  lane_swap<%d> lane %d holds (%d, %d), expected (%d, %d)\n", off, lane, h32[(4 + 2 * s) * 64 + lane], h32[(5 + 2 * s) * 64 + lane], want_a, want_b);
        }
        const unsigned long long wa = up ? tagbits(0x40000040u, lane ^ off) : tagbits(0x40000000u, lane);
        const unsigned long long wb = up ? tagbits(0x40000040u, lane) : tagbits(0x40000000u, lane ^ off);
        if (h64[(2 * s) * 64 + lane] != wa || h64[(2 * s + 1) * 64 + lane] != wb) {
          ++bad;
          if (printed++ < 12) printf("  lane_swap<%d>(double) lane %d holds (%016llx, %016llx)\n", off, lane, h64[(2 * s) * 64 + lane], h64[(2 * s + 1) * 64 + lane]);
        }
      }
    }
    printf("directions: %s\n", bad ? "FAIL" : "ok");
    fails += bad ? 1 : 0;
    CHECK(hipFree(d32)); CHECK(hipFree(d64));
  }
  // 2. sums
  {
    double *d_in, *d_out;
    CHECK(hipMalloc(&d_in, (size_t)M_MAX * MAXN * 8));
    CHECK(hipMalloc(&d_out, (size_t)256 * MAXN * 8));
    int n_nan = 0, n_words = 0;
    fails += run_sums<1>(d_in, d_out, printed, n_nan, n_words);
    fails += run_sums<2>(d_in, d_out, printed, n_nan, n_words);
    fails += run_sums<3>(d_in, d_out, printed, n_nan, n_words);
    fails += run_sums<6>(d_in, d_out, printed, n_nan, n_words);
    fails += run_sums<11>(d_in, d_out, printed, n_nan, n_words);
    fails += run_sums<16>(d_in, d_out, printed, n_nan, n_words);
    fails += run_sums<28>(d_in, d_out, printed, n_nan, n_words);
    printf("block_sum_canon reference totals: %d words, %d of them NaN (compared by NaN-ness)\n", n_words, n_nan);
    CHECK(hipFree(d_in)); CHECK(hipFree(d_out));
  }
  // 3. integers
  {
    std::vector<int> h_in(256), h_out(4 * 256);
    std::vector<unsigned long long> h_in64(256), h_out64(256);
    int *d_in, *d_out; unsigned long long *d_in64, *d_out64;
    CHECK(hipMalloc(&d_in, 256 * 4)); CHECK(hipMalloc(&d_out, 4 * 256 * 4));
    CHECK(hipMalloc(&d_in64, 256 * 8)); CHECK(hipMalloc(&d_out64, 256 * 8));
    int bad = 0;
    for (int trial = 0; trial < 4; ++trial) {
      for (int i = 0; i < 256; ++i) {
        // trial 0: small counts (the call sites' range); 1: signed values; 2: lane numbers; 3: large, the sum wraps
        h_in[i] = trial == 0 ? (int)(rnd() % 5) : trial == 1 ? (int)(rnd() % 2001) - 1000 : trial == 2 ? i : (int)(uint32_t)rnd();
        h_in64[i] = trial == 0 ? ((rnd() % 3) | ((rnd() % 3) << 13) | ((rnd() % 3) << 26)) : rnd();
      }
      CHECK(hipMemcpy(d_in, h_in.data(), 256 * 4, hipMemcpyHostToDevice));
      CHECK(hipMemcpy(d_in64, h_in64.data(), 256 * 8, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_ints, dim3(1), dim3(256), 0, 0, d_in, d_in64, d_out, d_out64);
      CHECK(hipMemcpy(h_out.data(), d_out, 4 * 256 * 4, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(h_out64.data(), d_out64, 256 * 8, hipMemcpyDeviceToHost));
      for (int w = 0; w < 4; ++w) {
        uint32_t run = 0; int mx = INT32_MIN; unsigned long long run64 = 0;
        uint32_t tot = 0; int tmx = INT32_MIN;
        for (int l = 0; l < 64; ++l) { tot += (uint32_t)h_in[64 * w + l]; tmx = h_in[64 * w + l] > tmx ? h_in[64 * w + l] : tmx; run64 += h_in64[64 * w + l]; }
        for (int l = 0; l < 64; ++l) {
          const int i = 64 * w + l;
          run += (uint32_t)h_in[i];
          mx = h_in[i] > mx ? h_in[i] : mx;
          const bool ok = h_out[i] == (int)run && h_out[256 + i] == mx && h_out[512 + i] == (int)tot && h_out[768 + i] == tmx &&
                          h_out64[i] == run64;
          if (!ok) {
            ++bad;
            if (printed++ < 12) printf("  integers trial %d thread %d: scan_add %d (%d) scan_max %d (%d) sum %d (%d) max %d (%d) sum64 %llx (%llx)\n",
                                       trial, i, h_out[i], (int)run, h_out[256 + i], mx, h_out[512 + i], (int)tot, h_out[768 + i], tmx,
                                       h_out64[i], run64);
          }
        }
      }
    }
    printf("integers: %s\n", bad ? "FAIL" : "ok");
    fails += bad ? 1 : 0;
    CHECK(hipFree(d_in)); CHECK(hipFree(d_out)); CHECK(hipFree(d_in64)); CHECK(hipFree(d_out64));
  }
  CHECK(hipDeviceSynchronize());
  printf(fails ? "canon_lanes: FAIL\n" : "canon_lanes: PASS\n");
  return fails ? 1 : 0;
}
