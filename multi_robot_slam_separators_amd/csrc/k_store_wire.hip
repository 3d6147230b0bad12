// k_store_wire.hip -- store slots as one block of bytes and back (sf_store_export_* / sf_store_import_keyframes_device;
// the layout is fixed in include/sepfinder.h: sf_kfblob_header, sf_kfblob_entry, the keyframe block).  A slot keeps the
// descriptor rows padded to w dwords, xyz dense and a float4 per keypoint; the blob keeps the rows tight, xyz as it is and
// 12 bytes per keypoint, every part padded to 16 bytes -- so both sides of every copy are 16-byte aligned and the kernels
// move one 16-byte unit per lane and step (64 lanes: 1 KiB per instruction), except where the row width says otherwise.
//
//   k_kfblob_plan     one workgroup.  Reads meta[first_slot .. first_slot + n) 256 at a time, scans the padded block sizes
//                     in 64 bits (an inclusive scan over 2 KB of LDS, the carry in a register: n is any number up to 65535)
//                     and writes the header and the table.  Resets the status words when it opens an export (status != NULL).
//   k_kfblob_pack     workgroup (keyframe k, piece p) writes the units p * 1024 + tid, + pieces * 1024, ... of keyframe k's
//                     block, so a keyframe of 4096 rows is spread over many workgroups and one of 0 rows costs a workgroup
//                     that reads its table entry and leaves; keyframe n stands for the header and the table.  A blob that
//                     exceeds cap_bytes is not written: one lane writes its header with magic 0 and sets status bit 1.
//   k_kfblob_status_reset   one lane: the status words of an import, whose workgroups have no first among them.
//   k_kfblob_unpack   the same cut over the units of the slot.  EVERY workgroup checks the header and its own table entry
//                     before it reads anything else (64 bytes, cached after the first), so no workgroup waits for another;
//                     what it then reads lies inside [offset, offset + bytes) of a checked entry, inside total_bytes <=
//                     bytes.  The first lane of piece 0 writes meta, or empties the slot and reports.  Rows are padded
//                     again to w dwords with zeros and kp.w is 0: the slot equals what k_ingest makes of the same features.
//
// Rows of cols % 16 == 0 bytes (32, 64, 128, 256, 512) move as whole units; cols % 4 == 0 by dwords; any other width by
// bytes on the blob side, as in k_ingest_ragged -- the store side is always whole units.  No LDS beyond the scan, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sf_internal.hpp"

namespace {

constexpr int WIRE_BLOCK = 256;
constexpr unsigned WIRE_PIECE_UNITS = 1024;    // 16 KB of 16-byte units per workgroup and step

static_assert(sizeof(sf_kfblob_header) == 32 && sizeof(sf_kfblob_entry) == 32, "the blob's header and entry are 32 bytes");

// the units of workgroup `piece`: 1024 in a row (four per lane, a wavefront's 64 side by side), then `stride` further on
#define WIRE_FOR_UNITS(u, piece, units, stride, tid)                                            \
  for (unsigned base_ = (piece) * WIRE_PIECE_UNITS; base_ < (units); base_ += (stride))         \
    for (unsigned u = base_ + (tid), end_ = min(base_ + WIRE_PIECE_UNITS, (units)); u < end_; u += WIRE_BLOCK)

__host__ __device__ inline unsigned long long pad16(unsigned long long v) { return (v + 15ull) & ~15ull; }
// bytes of a keyframe's block (rows >= 0, cols >= 0)
__host__ __device__ inline unsigned long long block_bytes(int rows, int cols, int n3d) {
  const unsigned long long r = (unsigned long long)rows;
  return pad16(r * (unsigned long long)cols) + (n3d > 0 ? pad16(r * 12ull) : 0ull) + pad16(r * 12ull);
}
__host__ __device__ inline unsigned long long table_end(int n) { return 32ull + 32ull * (unsigned long long)n; }

__global__ void __launch_bounds__(WIRE_BLOCK)
k_kfblob_plan(const int4* __restrict__ meta, int first_slot, int n, int desc_type, uint8_t* __restrict__ plan,
              int32_t* __restrict__ status) {
  __shared__ unsigned long long s_scan[WIRE_BLOCK];
  __shared__ int s_max;
  const int tid = threadIdx.x;
  if (tid == 0) {
    s_max = 0;
    if (status) { status[0] = 0; status[1] = 0; status[2] = -1; status[3] = 0; }
  }
  __syncthreads();
  sf_kfblob_entry* tab = reinterpret_cast<sf_kfblob_entry*>(plan + 32);
  unsigned long long carry = table_end(n);
  int my_max = 0;
  for (int base = 0; base < n; base += WIRE_BLOCK) {       // (workgroup-uniform)
    const int i = base + tid;
    int rows = 0, n3d = 0, cols = 0;
    if (i < n) {
      const int4 m = meta[first_slot + i];
      rows = m.x; n3d = m.y > 0 ? m.x : 0; cols = m.w;
    }
    const unsigned long long b = block_bytes(rows, cols, n3d);
    s_scan[tid] = b;
    __syncthreads();
    for (int d = 1; d < WIRE_BLOCK; d <<= 1) {
      const unsigned long long v = tid >= d ? s_scan[tid - d] : 0ull;
      __syncthreads();
      s_scan[tid] += v;
      __syncthreads();
    }
    const unsigned long long incl = s_scan[tid], sum = s_scan[WIRE_BLOCK - 1];
    if (i < n) {
      sf_kfblob_entry e;
      e.rows = rows; e.n3d = n3d; e.cols = cols; e.reserved = 0;
      e.offset = carry + incl - b; e.bytes = b;
      tab[i] = e;
    }
    carry += sum;
    my_max = max(my_max, rows);
    __syncthreads();                                       // s_scan is written again by the next pass
  }
  atomicMax(&s_max, my_max);
  __syncthreads();
  if (tid == 0) {
    sf_kfblob_header h;
    h.magic = SF_KFBLOB_MAGIC; h.version = SF_KFBLOB_VERSION; h.desc_type = (uint8_t)desc_type; h.reserved = 0;
    h.n_keyframes = n; h.max_rows = s_max; h.total_bytes = carry; h.reserved2 = 0;
    *reinterpret_cast<sf_kfblob_header*>(plan) = h;
  }
}

__global__ void k_kfblob_status_reset(int32_t* __restrict__ status) {
  status[0] = 0; status[1] = 0; status[2] = -1; status[3] = 0;
}

// 16 bytes of a keyframe's tight descriptor rows from byte `off` on (a multiple of 16), out of rows of w dwords
__device__ __forceinline__ uint4 pack_desc_unit(const uint32_t* __restrict__ src32, int w, int rows, int cols, unsigned off) {
  const unsigned lim = (unsigned)rows * (unsigned)cols;
  if ((cols & 15) == 0) {
    const unsigned r = off / (unsigned)cols, b = off - r * (unsigned)cols;
    return *reinterpret_cast<const uint4*>(src32 + (size_t)r * w + (b >> 2));
  }
  uint32_t v[4];
  if ((cols & 3) == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned o = off + 4u * j, r = o / (unsigned)cols, b = o - r * (unsigned)cols;
      v[j] = o < lim ? src32[(size_t)r * w + (b >> 2)] : 0u;
    }
  } else {
    const uint8_t* src8 = reinterpret_cast<const uint8_t*>(src32);
    const unsigned rowb = (unsigned)w * 4u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t d = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned o = off + 4u * j + q, r = o / (unsigned)cols, b = o - r * (unsigned)cols;
        const uint32_t byte = o < lim ? (uint32_t)src8[(size_t)r * rowb + b] : 0u;
        d |= byte << (8 * q);
      }
      v[j] = d;
    }
  }
  return make_uint4(v[0], v[1], v[2], v[3]);
}

__global__ void __launch_bounds__(WIRE_BLOCK)
k_kfblob_pack(const uint32_t* __restrict__ desc, const uint32_t* __restrict__ xyz, const uint32_t* __restrict__ kp, int kcap,
              int w, int first_slot, int n, unsigned pieces, const uint8_t* __restrict__ plan, uint8_t* __restrict__ blob,
              unsigned long long cap_bytes, int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  const unsigned k = blockIdx.x / pieces, piece = blockIdx.x - k * pieces;
  const sf_kfblob_header h = *reinterpret_cast<const sf_kfblob_header*>(plan);
  if (h.total_bytes > cap_bytes) {
    if (k == (unsigned)n && piece == 0 && tid == 0) {
      atomicOr(status, 1);
      if (cap_bytes >= 32ull) {
        sf_kfblob_header z = h;
        z.magic = 0u;
        *reinterpret_cast<sf_kfblob_header*>(blob) = z;
      }
    }
    return;
  }
  const unsigned stride = pieces * WIRE_PIECE_UNITS;
  if (k == (unsigned)n) {                                  // header and table
    const unsigned units = 2u + 2u * (unsigned)n;
    const uint4* s = reinterpret_cast<const uint4*>(plan);
    uint4* d = reinterpret_cast<uint4*>(blob);
    WIRE_FOR_UNITS(u, piece, units, stride, tid) d[u] = s[u];
    return;
  }
  const sf_kfblob_entry e = reinterpret_cast<const sf_kfblob_entry*>(plan + 32)[k];
  if (e.rows <= 0) return;
  const size_t slot = (size_t)first_slot + k;
  const unsigned dbytes = (unsigned)pad16((unsigned long long)e.rows * e.cols);
  const unsigned pbytes = (unsigned)pad16((unsigned long long)e.rows * 12ull);
  const unsigned xbytes = e.n3d > 0 ? pbytes : 0u;
  const unsigned units = (dbytes + xbytes + pbytes) >> 4;
  const unsigned lim3 = (unsigned)e.rows * 3u;             // dwords of xyz, and of the keypoints
  const uint32_t* sd = desc + slot * kcap * w;
  const uint32_t* sx = xyz + slot * kcap * 3;
  const uint32_t* sk = kp + slot * kcap * 4;
  uint4* out = reinterpret_cast<uint4*>(blob + e.offset);
  WIRE_FOR_UNITS(u, piece, units, stride, tid) {
    const unsigned off = u << 4;
    uint4 v;
    if (off < dbytes) {
      v = pack_desc_unit(sd, w, e.rows, e.cols, off);
    } else if (off < dbytes + xbytes) {
      const unsigned d0 = (off - dbytes) >> 2;
      if (d0 + 4u <= lim3) {
        v = *reinterpret_cast<const uint4*>(sx + d0);
      } else {
        v.x = d0 + 0u < lim3 ? sx[d0 + 0u] : 0u;
        v.y = d0 + 1u < lim3 ? sx[d0 + 1u] : 0u;
        v.z = d0 + 2u < lim3 ? sx[d0 + 2u] : 0u;
        v.w = 0u;
      }
    } else {
      const unsigned d0 = (off - dbytes - xbytes) >> 2;
      uint32_t t[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned d = d0 + j, i = d / 3u, c = d - i * 3u;
        t[j] = d < lim3 ? sk[(size_t)i * 4 + c] : 0u;
      }
      v = make_uint4(t[0], t[1], t[2], t[3]);
    }
    out[u] = v;
  }
}

// 16 bytes of a stored row (byte b of row r, b a multiple of 16) out of the blob's tight rows
__device__ __forceinline__ uint4 unpack_desc_unit(const uint8_t* __restrict__ src, int cols, unsigned r, unsigned b) {
  const size_t at = (size_t)r * (unsigned)cols + b;
  if ((cols & 15) == 0) return b < (unsigned)cols ? *reinterpret_cast<const uint4*>(src + at) : make_uint4(0u, 0u, 0u, 0u);
  uint32_t v[4];
  if ((cols & 3) == 0) {
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src + at);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = b + 4u * j < (unsigned)cols ? s32[j] : 0u;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t d = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned o = 4u * j + q;
        const uint32_t byte = b + o < (unsigned)cols ? (uint32_t)src[at + o] : 0u;
        d |= byte << (8 * q);
      }
      v[j] = d;
    }
  }
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// a descriptor width the store of this handle holds: desc_dwords(cols) == w and the type's own limits (sf_store_reserve)
__device__ __forceinline__ bool cols_in_class(int desc_type, int w, int cols) {
  if (desc_type == 0) return cols >= 1 && cols <= SF_MAX_DESC_BYTES && (cols <= 32 ? 8 : 16) == w;
  if (desc_type == 1) return (cols == 256 || cols == 512) && cols / 4 == w;
  return cols == SF_DESC_BYTES_U8 && cols / 4 == w;
}

__global__ void __launch_bounds__(WIRE_BLOCK)
k_kfblob_unpack(uint32_t* __restrict__ desc, uint32_t* __restrict__ xyz, uint4* __restrict__ kp, int4* __restrict__ meta, int kcap,
                int w, int first_slot, int n, int max_rows, int cols_empty, int desc_type, unsigned pieces,
                const uint8_t* __restrict__ blob, unsigned long long bytes, int32_t* __restrict__ status) {
  const int tid = threadIdx.x;
  const unsigned k = blockIdx.x / pieces, piece = blockIdx.x - k * pieces;
  const size_t slot = (size_t)first_slot + k;
  const bool lead = piece == 0 && tid == 0;
  const unsigned long long tend = table_end(n);
  int bad = bytes >= tend ? 0 : 2;
  sf_kfblob_header h = {};
  if (!bad) {
    h = *reinterpret_cast<const sf_kfblob_header*>(blob);
    if (h.magic != SF_KFBLOB_MAGIC || h.version != SF_KFBLOB_VERSION || (int)h.desc_type != desc_type || h.n_keyframes != n ||
        h.total_bytes > bytes || h.total_bytes < tend)
      bad = 2;
  }
  sf_kfblob_entry e = {};
  if (!bad) {
    e = reinterpret_cast<const sf_kfblob_entry*>(blob + 32)[k];
    const bool ok = e.rows >= 0 && e.rows <= max_rows && (e.n3d == 0 || e.n3d == e.rows) && cols_in_class(desc_type, w, e.cols) &&
                    (e.offset & 15ull) == 0ull && e.offset >= tend && e.offset <= h.total_bytes &&
                    e.bytes <= h.total_bytes - e.offset && e.bytes == block_bytes(e.rows, e.cols, e.n3d);
    if (!ok) bad = 4;
  }
  if (bad) {
    if (lead) {
      meta[slot] = make_int4(0, 0, 0, cols_empty);
      atomicOr(status, bad);
      atomicAdd(status + 1, 1);
      atomicMin(reinterpret_cast<unsigned*>(status + 2), k);      // (-1 is the largest unsigned)
    }
    return;
  }
  if (lead) meta[slot] = make_int4(e.rows, e.n3d, e.rows, e.cols);
  if (e.rows == 0) return;
  const unsigned rows = (unsigned)e.rows;
  const unsigned dbytes = (unsigned)pad16((unsigned long long)rows * e.cols);
  const unsigned pbytes = (unsigned)pad16((unsigned long long)rows * 12ull);
  const unsigned xbytes = e.n3d > 0 ? pbytes : 0u;
  const unsigned row_units = (unsigned)w >> 2;             // (w is 8, 16, 32, 64 or 128)
  const unsigned dunits = rows * row_units, xunits = xbytes >> 4;
  const unsigned units = dunits + xunits + rows;
  const unsigned lim3 = rows * 3u;
  const uint8_t* src = blob + e.offset;
  const uint32_t* sx = reinterpret_cast<const uint32_t*>(src + dbytes);
  const uint32_t* sk = reinterpret_cast<const uint32_t*>(src + dbytes + xbytes);
  uint4* dd = reinterpret_cast<uint4*>(desc + slot * kcap * w);
  uint32_t* dx = xyz + slot * kcap * 3;
  uint4* dk = kp + slot * kcap;
  const unsigned stride = pieces * WIRE_PIECE_UNITS;
  WIRE_FOR_UNITS(u, piece, units, stride, tid) {
    if (u < dunits) {
      const unsigned r = u / row_units, b = (u - r * row_units) << 4;
      dd[u] = unpack_desc_unit(src, e.cols, r, b);
    } else if (u < dunits + xunits) {
      const unsigned d0 = (u - dunits) << 2;
      if (d0 + 4u <= lim3) {
        *reinterpret_cast<uint4*>(dx + d0) = *reinterpret_cast<const uint4*>(sx + d0);
      } else {
        for (unsigned d = d0; d < lim3; ++d) dx[d] = sx[d];
      }
    } else {
      const unsigned i = u - dunits - xunits;
      int o = (int)sk[3u * i + 2u] & 255;
      o = o < 128 ? o : (-128 | o);
      dk[i] = make_uint4(sk[3u * i], sk[3u * i + 1u], (uint32_t)o, 0u);
    }
  }
}

// workgroups per keyframe for blocks of at most `units` 16-byte units
inline unsigned pieces_for(unsigned long long units) {
  return (unsigned)std::max<unsigned long long>(1ull, (units + WIRE_PIECE_UNITS - 1) / WIRE_PIECE_UNITS);
}

}  // namespace

int sf_launch_kfblob_plan(sf_context* c, const Store& st, int first_slot, int n, void* d_plan, int32_t* d_status) {
  hipLaunchKernelGGL(k_kfblob_plan, dim3(1), dim3(WIRE_BLOCK), 0, c->stream, (const int4*)st.meta.p, first_slot, n,
                     c->params.desc_type, (uint8_t*)d_plan, d_status);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

int sf_launch_kfblob_pack(sf_context* c, const Store& st, int first_slot, int n, const void* d_plan, void* d_blob,
                          uint64_t cap_bytes, int32_t* d_status) {
  // a slot holds at most kcap rows: its block is at most this long
  const unsigned long long units = (pad16((unsigned long long)st.kcap * st.w * 4ull) + 2ull * pad16((unsigned long long)st.kcap * 12ull)) >> 4;
  const unsigned pieces = pieces_for(units);               // (the table's workgroups loop over what is longer than that)
  hipLaunchKernelGGL(k_kfblob_pack, dim3(pieces * (unsigned)(n + 1)), dim3(WIRE_BLOCK), 0, c->stream, (const uint32_t*)st.desc.p,
                     (const uint32_t*)st.xyz.p, (const uint32_t*)st.kp.p, st.kcap, st.w, first_slot, n, pieces,
                     (const uint8_t*)d_plan, (uint8_t*)d_blob, (unsigned long long)cap_bytes, d_status);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

int sf_launch_kfblob_unpack(sf_context* c, Store& st, int first_slot, int n, int max_rows, int cols, const void* d_blob,
                            uint64_t bytes, int32_t* d_status) {
  hipLaunchKernelGGL(k_kfblob_status_reset, dim3(1), dim3(1), 0, c->stream, d_status);
  SF_HIP(c, hipGetLastError());
  if (n <= 0) return SF_OK;
  const unsigned long long units = (unsigned long long)max_rows * (st.w >> 2) + (pad16((unsigned long long)max_rows * 12ull) >> 4) + (unsigned long long)max_rows;
  const unsigned pieces = pieces_for(units);
  hipLaunchKernelGGL(k_kfblob_unpack, dim3(pieces * (unsigned)n), dim3(WIRE_BLOCK), 0, c->stream, (uint32_t*)st.desc.p,
                     (uint32_t*)st.xyz.p, (uint4*)st.kp.p, (int4*)st.meta.p, st.kcap, st.w, first_slot, n, max_rows, cols,
                     c->params.desc_type, pieces, (const uint8_t*)d_blob, (unsigned long long)bytes, d_status);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}
