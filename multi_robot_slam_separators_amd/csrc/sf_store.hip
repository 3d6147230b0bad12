// sf_store.hip -- the device-resident keyframe store: wire layout -> store layout (k_ingest, k_ingest_ragged), growth,
// the host-buffer ingest with its packing workers, the sf_store_* entry points -- those that move slots as bytes included
// (sf_store_export_*, sf_store_import_keyframes_device; their kernels are in k_store_wire.hip).
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "sf_host.hpp"

StoreView sf_store_view(const Store& s) {
  StoreView v;
  v.desc = (const uint32_t*)s.desc.p;
  v.xyz = (const float*)s.xyz.p;
  v.kp = (const float4*)s.kp.p;
  v.meta = (const int4*)s.meta.p;
  v.kcap = s.kcap;
  v.w = s.w;
  v.n_slots = s.slots;
  return v;
}

// ---- ingest kernel: wire layout -> store layout ---------------------------------------------------
namespace {

// one workgroup per keyframe.  desc rows are zero padded to w dwords; keypoints are reduced to
// {x, y, sign-extended (octave & 255)} (myRegistrationVis.cpp:709-710 compares only that byte).
__global__ void __launch_bounds__(SF_BLOCK)
k_ingest(uint32_t* __restrict__ desc, float* __restrict__ xyz, float4* __restrict__ kp, int4* __restrict__ meta,
         int kcap, int w, int first_slot, int rows, int cols, int n3d, const uint8_t* __restrict__ s_desc,
         const float* __restrict__ s_xyz, const sf_keypoint* __restrict__ s_kp) {
  const int k = blockIdx.x;
  const int slot = first_slot + k;
  const int tid = threadIdx.x;
  uint8_t* d8 = reinterpret_cast<uint8_t*>(desc + (size_t)slot * kcap * w);
  const uint8_t* sd = s_desc + (size_t)k * rows * cols;
  const int rowb = w * 4;
  for (int i = tid; i < rows * rowb; i += SF_BLOCK) {
    const int r = i / rowb, b = i - r * rowb;
    d8[i] = (b < cols) ? sd[(size_t)r * cols + b] : (uint8_t)0;
  }
  float* dx = xyz + (size_t)slot * kcap * 3;
  if (n3d > 0) {
    const float* sx = s_xyz + (size_t)k * rows * 3;
    for (int i = tid; i < rows * 3; i += SF_BLOCK) dx[i] = sx[i];
  }
  float4* dk = kp + (size_t)slot * kcap;
  const sf_keypoint* sk = s_kp + (size_t)k * rows;
  for (int i = tid; i < rows; i += SF_BLOCK) {
    const sf_keypoint q = sk[i];
    int o = q.octave & 255;
    o = o < 128 ? o : (-128 | o);
    dk[i] = make_float4(q.x, q.y, __int_as_float(o), 0.f);
  }
  if (tid == 0) meta[slot] = make_int4(rows, n3d > 0 ? rows : 0, rows, cols);
}

// ragged variant for host-buffer batches: per-keyframe table of byte offsets into ONE packed
// staging buffer.  The host packs each keyframe as [descriptors | xyz | keypoints reduced to
// {x, y, raw octave} (12 of the wire's 28 bytes)], every part 16-byte aligned.
struct IngestEntry {
  int32_t rows, cols, n3d, pad;
  uint64_t desc_off, xyz_off, kp_off;   // byte offsets from the start of the staging buffer
};
struct PackedKp { float x, y; int32_t octave; };

__global__ void __launch_bounds__(SF_BLOCK)
k_ingest_ragged(uint32_t* __restrict__ desc, float* __restrict__ xyz, float4* __restrict__ kp, int4* __restrict__ meta,
                int kcap, int w, int first_slot, const IngestEntry* __restrict__ table,
                const uint8_t* __restrict__ stage) {
  const int k = blockIdx.x;
  const int slot = first_slot + k;
  const int tid = threadIdx.x;
  const IngestEntry e = table[k];
  const uint8_t* sd = stage + e.desc_off;
  if ((e.cols & 3) == 0) {
    // dword path (descriptor bytes a multiple of 4; rows start 16-byte aligned in the staging buffer)
    uint32_t* d32 = desc + (size_t)slot * kcap * w;
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(sd);
    const int cw = e.cols >> 2;
    for (int i = tid; i < e.rows * w; i += SF_BLOCK) {
      const int r = i / w, b = i - r * w;
      d32[i] = (b < cw) ? s32[(size_t)r * cw + b] : 0u;
    }
  } else {
    uint8_t* d8 = reinterpret_cast<uint8_t*>(desc + (size_t)slot * kcap * w);
    const int rowb = w * 4;
    for (int i = tid; i < e.rows * rowb; i += SF_BLOCK) {
      const int r = i / rowb, b = i - r * rowb;
      d8[i] = (b < e.cols) ? sd[(size_t)r * e.cols + b] : (uint8_t)0;
    }
  }
  if (e.n3d > 0) {
    float* dx = xyz + (size_t)slot * kcap * 3;
    const float* sx = reinterpret_cast<const float*>(stage + e.xyz_off);
    for (int i = tid; i < e.rows * 3; i += SF_BLOCK) dx[i] = sx[i];
  }
  float4* dk = kp + (size_t)slot * kcap;
  const PackedKp* sk = reinterpret_cast<const PackedKp*>(stage + e.kp_off);
  for (int i = tid; i < e.rows; i += SF_BLOCK) {
    const PackedKp q = sk[i];
    int o = q.octave & 255;
    o = o < 128 ? o : (-128 | o);
    dk[i] = make_float4(q.x, q.y, __int_as_float(o), 0.f);
  }
  if (tid == 0) meta[slot] = make_int4(e.rows, e.n3d > 0 ? e.rows : 0, e.rows, e.cols);
}

}  // namespace

// dwords per stored descriptor row: binary rows 8 (<= 256 bits) or 16; float32 rows (desc_type 1) one per dimension;
// uint8 L2 rows (desc_type 2) four dimensions per dword
static int desc_dwords(const sf_context* c, int cols) {
  if (c->params.desc_type != 0) return cols / 4;
  return cols <= 32 ? 8 : 16;
}
// the widest row a keyframe of the handle's descriptor type may have
static int max_desc_bytes(const sf_context* c) {
  return c->params.desc_type == 1 ? SF_MAX_DESC_BYTES_F32 : c->params.desc_type == 2 ? SF_DESC_BYTES_U8 : SF_MAX_DESC_BYTES;
}

int sf_store_reserve(sf_context* c, Store& s, int slots_needed, int rows, int cols) {
  if (c->params.desc_type == 1) {
    if (cols != 256 && cols != 512)
      return sf_fail(c, SF_ERANGE, "float32 descriptors: %d bytes per row (64 or 128 dimensions = 256 or 512 bytes)", cols);
  } else if (c->params.desc_type == 2) {
    if (cols != SF_DESC_BYTES_U8)
      return sf_fail(c, SF_ERANGE, "uint8 L2 descriptors: %d bytes per row (128 dimensions = %d bytes)", cols, SF_DESC_BYTES_U8);
  } else if (cols < 1 || cols > SF_MAX_DESC_BYTES) {
    return sf_fail(c, SF_ERANGE, "descriptor bytes %d not in 1..%d", cols, SF_MAX_DESC_BYTES);
  }
  if (rows > SF_MAX_FEATURES) return sf_fail(c, SF_ERANGE, "rows %d > int16 limit of KeyPointVec.size", rows);
  const int w = desc_dwords(c, cols);
  int kcap = s.kcap ? s.kcap : std::max(64, (c->params.max_features + 63) & ~63);
  while (kcap < rows) kcap *= 2;
  if (kcap > SF_MAX_KCAP) return sf_fail(c, SF_ERANGE, "%d features per keyframe exceed the kernel capacity %d", rows, SF_MAX_KCAP);
  if (s.slots > 0 && s.w != w) return sf_fail(c, SF_EINVAL, "descriptor width %d B differs from the store's (%d dwords)", cols, s.w);
  int cap = s.cap_slots;
  if (cap < slots_needed) cap = std::max(slots_needed, std::max(cap * 2, &s == &c->store ? c->params.store_capacity : 64));
  if (&s == &c->store) (void)sf_lanes_touch(c, false);     // (a slot of the store is about to be written)
  if (kcap == s.kcap && cap == s.cap_slots && s.w == w) return SF_OK;
  if (&s == &c->store) (void)sf_lanes_touch(c, true);      // the old buffers are freed below: nothing may still read them
  // (re)allocate; keep old contents slot by slot (pitch copy when kcap grew)
  Store n;
  n.kcap = kcap; n.w = w; n.cap_slots = cap; n.slots = s.slots;
  int rc;
  if ((rc = sf_buf_reserve(c, n.desc, (size_t)cap * kcap * w * 4)) != SF_OK ||
      (rc = sf_buf_reserve(c, n.xyz, (size_t)cap * kcap * 12)) != SF_OK ||
      (rc = sf_buf_reserve(c, n.kp, (size_t)cap * kcap * 16)) != SF_OK ||
      (rc = sf_buf_reserve(c, n.meta, (size_t)cap * 16)) != SF_OK)
    return rc;                      // (every early return frees what `n` holds; the old store stays valid)
  if (s.slots > 0) {
    SF_HIP(c, hipMemcpy2DAsync(n.desc.p, (size_t)kcap * w * 4, s.desc.p, (size_t)s.kcap * w * 4, (size_t)s.kcap * w * 4, s.slots, hipMemcpyDeviceToDevice, c->stream));
    SF_HIP(c, hipMemcpy2DAsync(n.xyz.p, (size_t)kcap * 12, s.xyz.p, (size_t)s.kcap * 12, (size_t)s.kcap * 12, s.slots, hipMemcpyDeviceToDevice, c->stream));
    SF_HIP(c, hipMemcpy2DAsync(n.kp.p, (size_t)kcap * 16, s.kp.p, (size_t)s.kcap * 16, (size_t)s.kcap * 16, s.slots, hipMemcpyDeviceToDevice, c->stream));
    SF_HIP(c, hipMemcpyAsync(n.meta.p, s.meta.p, (size_t)s.slots * 16, hipMemcpyDeviceToDevice, c->stream));
    SF_HIP(c, hipStreamSynchronize(c->stream));
  }
  s = std::move(n);
  return SF_OK;
}

int sf_launch_ingest(sf_context* c, Store& st, int first_slot, int n, int rows, int cols,
                     const uint8_t* d_desc, const float* d_xyz, const sf_keypoint* d_kp) {
  if (n <= 0) return SF_OK;
  hipLaunchKernelGGL(k_ingest, dim3(n), dim3(SF_BLOCK), 0, c->stream, (uint32_t*)st.desc.p, (float*)st.xyz.p,
                     (float4*)st.kp.p, (int4*)st.meta.p, st.kcap, st.w, first_slot, rows, cols, d_xyz ? rows : 0,
                     d_desc, d_xyz, d_kp);
  SF_HIP(c, hipGetLastError());
  return SF_OK;
}

int sf_validate_features(sf_context* c, const sf_features* f) {
  if (!f) return sf_fail(c, SF_EINVAL, "null sf_features");
  if (f->rows > SF_MAX_FEATURES) return sf_fail(c, SF_ERANGE, "rows %d exceed int16", (int)f->rows);
  if (f->rows > 0 && (!f->desc || f->cols == 0)) return sf_fail(c, SF_EINVAL, "descriptors missing");
  if (f->n3d != 0 && f->n3d != (int32_t)f->rows)
    return sf_fail(c, SF_EINVAL, "kpts3D size %d != descriptor rows %d (myRegistrationVis.cpp:859)", f->n3d, (int)f->rows);
  if (f->nkp != (int32_t)f->rows)
    return sf_fail(c, SF_EINVAL, "kpts size %d != descriptor rows %d (myRegistrationVis.cpp:879)", f->nkp, (int)f->rows);
  if (f->n3d > 0 && !f->xyz) return sf_fail(c, SF_EINVAL, "kpts3D missing");
  if (f->nkp > 0 && !f->kpts) return sf_fail(c, SF_EINVAL, "kpts missing");
  return SF_OK;
}

// host features -> one store slot (staged through a device bounce buffer on the handle's stream)
struct Staging {
  Buf &desc, &xyz, &kp;
};
static Staging staging(sf_context* c) { return Staging{c->stage_desc, c->stage_xyz, c->stage_kp}; }

static int store_add_host(sf_context* c, Store& st, const sf_features* f, int* out_slot) {
  int rc = sf_validate_features(c, f);
  if (rc != SF_OK) return rc;
  const int rows = f->rows;
  int cols = f->cols;
  if (rows == 0 && cols == 0) cols = st.slots > 0 ? st.w * 4 : std::max(1, c->params.desc_bytes);
  if ((rc = sf_store_reserve(c, st, st.slots + 1, rows, cols)) != SF_OK) return rc;
  if (st.slots > 0 || rows > 0) {
    // all keyframes of one store share the descriptor width class
    if (st.w != desc_dwords(c, cols)) return sf_fail(c, SF_EINVAL, "descriptor width mismatch");
  }
  Staging sg = staging(c);
  const uint8_t* dd = nullptr; const float* dx = nullptr; const sf_keypoint* dk = nullptr;
  if (rows > 0) {
    if ((rc = sf_buf_reserve(c, sg.desc, (size_t)rows * cols)) != SF_OK) return rc;
    if ((rc = sf_buf_reserve(c, sg.kp, (size_t)rows * sizeof(sf_keypoint))) != SF_OK) return rc;
    SF_HIP(c, hipMemcpyAsync(sg.desc.p, f->desc, (size_t)rows * cols, hipMemcpyHostToDevice, c->stream));
    SF_HIP(c, hipMemcpyAsync(sg.kp.p, f->kpts, (size_t)rows * sizeof(sf_keypoint), hipMemcpyHostToDevice, c->stream));
    dd = (const uint8_t*)sg.desc.p; dk = (const sf_keypoint*)sg.kp.p;
    if (f->n3d > 0) {
      if ((rc = sf_buf_reserve(c, sg.xyz, (size_t)rows * 12)) != SF_OK) return rc;
      SF_HIP(c, hipMemcpyAsync(sg.xyz.p, f->xyz, (size_t)rows * 12, hipMemcpyHostToDevice, c->stream));
      dx = (const float*)sg.xyz.p;
    }
  }
  if ((rc = sf_launch_ingest(c, st, st.slots, 1, rows, cols, dd, dx, dk)) != SF_OK) return rc;
  // the bounce buffers are reused by the next call: drain before returning
  SF_HIP(c, hipStreamSynchronize(c->stream));
  if (out_slot) *out_slot = st.slots;
  st.slots += 1;
  return SF_OK;
}

// n host keyframes -> consecutive slots.  Features are packed into ONE pinned staging buffer in
// chunks of a few MB: worker threads pack chunk k+1 while the H2D copy of chunk k is in flight, then
// ONE ragged ingest launch converts everything (no per-keyframe synchronisation).  Small batches
// (a single service call) are packed inline by the calling thread.
static inline size_t pad16(size_t v) { return (v + 15) & ~(size_t)15; }

static void pack_keyframe(uint8_t* hp, const IngestEntry& e, const sf_features* f) {
  if (f->rows == 0) return;
  memcpy(hp + e.desc_off, f->desc, (size_t)f->rows * f->cols);
  if (f->n3d > 0) memcpy(hp + e.xyz_off, f->xyz, (size_t)f->rows * 12);
  PackedKp* k = reinterpret_cast<PackedKp*>(hp + e.kp_off);
  const sf_keypoint* src = f->kpts;
  for (int i = 0; i < (int)f->rows; ++i) { k[i].x = src[i].x; k[i].y = src[i].y; k[i].octave = src[i].octave; }
}


// Packing workers of the host-buffer batch ingest: started once per handle (first large batch), parked on a
// condition variable between batches, joined by sf_destroy.  A batch is cut into chunks; worker t packs the
// keyframes lo + t, lo + t + workers, ... of every chunk in turn and bumps done[k]; the calling thread ships
// chunk k to the device as soon as every worker has passed it.
struct IngestPool {
  std::vector<std::thread> threads;
  std::mutex mu;
  std::condition_variable cv_start, cv_idle;
  uint64_t generation = 0;
  int running = 0;
  bool quit = false;
  // the job of the current generation
  uint8_t* hp = nullptr;
  const IngestEntry* tab = nullptr;
  const sf_features* const* feats = nullptr;
  const std::pair<size_t, int>* chunks = nullptr;
  int n_chunks = 0;
  std::vector<std::atomic<int>> done;
  std::vector<IngestEntry> tab_storage;
  std::vector<std::pair<size_t, int>> chunk_storage;

  explicit IngestPool(int workers) : done(0) {
    for (int t = 0; t < workers; ++t) threads.emplace_back([this, t]() { work(t); });
  }
  ~IngestPool() {
    {
      std::lock_guard<std::mutex> lk(mu);
      quit = true;
    }
    cv_start.notify_all();
    for (auto& th : threads) th.join();
  }
  void work(int t) {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(mu);
        cv_start.wait(lk, [&] { return quit || generation != seen; });
        if (quit) return;
        seen = generation;
      }
      const int nw = (int)threads.size();
      int lo = 0;
      for (int k = 0; k < n_chunks; ++k) {
        const int hi = chunks[k].second;
        for (int i = lo + t; i < hi; i += nw) pack_keyframe(hp, tab[i], feats[i]);
        done[k].fetch_add(1, std::memory_order_release);
        lo = hi;
      }
      {
        std::lock_guard<std::mutex> lk(mu);
        if (--running == 0) cv_idle.notify_all();
      }
    }
  }
  void start() {
    if ((int)done.size() < n_chunks) done = std::vector<std::atomic<int>>(n_chunks);
    for (int k = 0; k < n_chunks; ++k) done[k].store(0, std::memory_order_relaxed);
    {
      std::lock_guard<std::mutex> lk(mu);
      running = (int)threads.size();
      ++generation;
    }
    cv_start.notify_all();
  }
  void wait_idle() {
    std::unique_lock<std::mutex> lk(mu);
    cv_idle.wait(lk, [&] { return running == 0; });
  }
};

void sf_ingest_pool_destroy(sf_context* c) {
  delete c->ingest_pool;
  c->ingest_pool = nullptr;
}

int sf_store_add_host_batch(sf_context* c, Store& st, const sf_features* const* feats, int n, int* first_slot) {
  if (n <= 0) return SF_OK;
  int rc;
  int max_rows = 0, cols = 0;
  for (int i = 0; i < n; ++i) {
    if ((rc = sf_validate_features(c, feats[i])) != SF_OK) return rc;
    max_rows = std::max<int>(max_rows, feats[i]->rows);
    if (feats[i]->rows > 0) {
      if (cols == 0) cols = feats[i]->cols;
      if (desc_dwords(c, feats[i]->cols) != desc_dwords(c, cols)) return sf_fail(c, SF_EINVAL, "descriptor width classes differ inside one batch");
      if (feats[i]->cols > max_desc_bytes(c))
        return sf_fail(c, SF_ERANGE, "descriptor bytes %d > %d", (int)feats[i]->cols, max_desc_bytes(c));
    }
  }
  if (cols == 0) cols = st.slots > 0 ? st.w * 4 : std::max(1, c->params.desc_bytes);
  if ((rc = sf_store_reserve(c, st, st.slots + n, max_rows, cols)) != SF_OK) return rc;

  // layout: [table][keyframe 0: desc | xyz | kp][keyframe 1 ...], chunk boundaries every ~4 MB
  // (table / chunk scratch lives in the pool object when there is one, else on this call's stack vectors)
  std::vector<IngestEntry> tab_local;
  std::vector<std::pair<size_t, int>> chunks_local;   // (end offset, end keyframe)
  std::vector<IngestEntry>& tab = c->ingest_pool ? c->ingest_pool->tab_storage : tab_local;
  std::vector<std::pair<size_t, int>>& chunks = c->ingest_pool ? c->ingest_pool->chunk_storage : chunks_local;
  tab.resize(n);
  chunks.clear();
  const size_t tb = pad16((size_t)n * sizeof(IngestEntry));
  const size_t chunk_bytes = (size_t)4 << 20;
  size_t off = tb, chunk_start = tb;
  for (int i = 0; i < n; ++i) {
    const sf_features* f = feats[i];
    IngestEntry& e = tab[i];
    e.rows = f->rows; e.cols = f->rows > 0 ? f->cols : cols; e.n3d = f->n3d; e.pad = 0;
    e.desc_off = off; off += pad16((size_t)f->rows * f->cols);
    e.xyz_off = off;  off += f->n3d > 0 ? pad16((size_t)f->rows * 12) : 0;
    e.kp_off = off;   off += pad16((size_t)f->rows * sizeof(PackedKp));
    if (off - chunk_start >= chunk_bytes || i == n - 1) { chunks.push_back({off, i + 1}); chunk_start = off; }
  }
  const size_t total = off;
  // pinned host staging owned by the handle
  if ((rc = sf_pinned_reserve(c, c->ingest_pinned, total, total + total / 2)) != SF_OK) return rc;
  if ((rc = sf_buf_reserve(c, c->stage_desc, total)) != SF_OK) return rc;
  uint8_t* hp = (uint8_t*)c->ingest_pinned.p;
  uint8_t* dp = (uint8_t*)c->stage_desc.p;
  memcpy(hp, tab.data(), (size_t)n * sizeof(IngestEntry));

  const int n_chunks = (int)chunks.size();
  int workers = 0;
  if (n_chunks >= 2) workers = (int)std::min<unsigned>(8u, std::max(1u, std::thread::hardware_concurrency() / 2));
  hipError_t herr = hipSuccess;
  if (workers <= 1) {
    for (int i = 0; i < n; ++i) pack_keyframe(hp, tab[i], feats[i]);
    herr = hipMemcpyAsync(dp, hp, total, hipMemcpyHostToDevice, c->stream);
  } else {
    if (!c->ingest_pool) {
      // first large batch of this handle: start the workers, and move the table / chunk lists into the pool
      c->ingest_pool = new IngestPool(workers);
      c->ingest_pool->tab_storage.swap(tab_local);
      c->ingest_pool->chunk_storage.swap(chunks_local);
    }
    IngestPool& pool = *c->ingest_pool;
    pool.hp = hp;
    pool.tab = pool.tab_storage.data();
    pool.feats = feats;
    pool.chunks = pool.chunk_storage.data();
    pool.n_chunks = n_chunks;
    pool.start();
    const int nw = (int)pool.threads.size();
    size_t sent = 0;
    for (int k = 0; k < n_chunks; ++k) {
      while (pool.done[k].load(std::memory_order_acquire) < nw) std::this_thread::yield();
      const size_t end = pool.chunk_storage[k].first;
      if (herr == hipSuccess) herr = hipMemcpyAsync(dp + sent, hp + sent, end - sent, hipMemcpyHostToDevice, c->stream);
      sent = end;
    }
    pool.wait_idle();
  }
  if (herr != hipSuccess) return sf_fail(c, SF_EHIP, "staging H2D copy -> %s", hipGetErrorString(herr));
  hipLaunchKernelGGL(k_ingest_ragged, dim3(n), dim3(SF_BLOCK), 0, c->stream, (uint32_t*)st.desc.p, (float*)st.xyz.p,
                     (float4*)st.kp.p, (int4*)st.meta.p, st.kcap, st.w, st.slots, (const IngestEntry*)dp, dp);
  SF_HIP(c, hipGetLastError());
  // the pinned staging is reused by the next call: the copies must have left host memory
  SF_HIP(c, hipStreamSynchronize(c->stream));
  if (first_slot) *first_slot = st.slots;
  st.slots += n;
  return SF_OK;
}

// ---- keyframe store -----------------------------------------------------------------------------
extern "C" int sf_store_add_keyframe(sf_handle c, const sf_features* f, int32_t* out_slot) {
  if (!c) return SF_EINVAL;
  SF_HIP(c, hipSetDevice(c->device));
  return store_add_host(c, c->store, f, out_slot);
}

extern "C" int sf_store_add_keyframes_device(sf_handle c, int32_t n, int32_t rows, int32_t cols,
                                             const uint8_t* d_desc, const float* d_xyz,
                                             const sf_keypoint* d_kp, int32_t* out_first_slot) {
  if (!c || n < 0 || rows < 0) return SF_EINVAL;
  if (n == 0) return SF_OK;
  if (rows > 0 && (!d_desc || !d_kp)) return sf_fail(c, SF_EINVAL, "device descriptor / keypoint pointers missing");
  SF_HIP(c, hipSetDevice(c->device));
  int rc = sf_store_reserve(c, c->store, c->store.slots + n, rows, cols);
  if (rc != SF_OK) return rc;
  if ((rc = sf_launch_ingest(c, c->store, c->store.slots, n, rows, cols, d_desc, d_xyz, d_kp)) != SF_OK) return rc;
  if (out_first_slot) *out_first_slot = c->store.slots;
  c->store.slots += n;
  return SF_OK;
}

// ---- store slots as bytes (kernels in k_store_wire.hip) -------------------------------------------
#define SF_KFBLOB_MAX_KEYFRAMES 65535     // per call, as the batch calls

// the range of an export, and the handle's plan and status buffers for it
static int wire_export_begin(sf_context* c, int32_t first_slot, int32_t n) {
  if (first_slot < 0 || n < 0 || (long long)first_slot + n > c->store.slots)
    return sf_fail(c, SF_ERANGE, "slots %d .. %lld lie outside the store's %d", first_slot, (long long)first_slot + n, c->store.slots);
  if (n > SF_KFBLOB_MAX_KEYFRAMES) return sf_fail(c, SF_ERANGE, "%d keyframes in one blob (at most %d)", n, SF_KFBLOB_MAX_KEYFRAMES);
  SF_HIP(c, hipSetDevice(c->device));
  int rc;
  if ((rc = sf_buf_reserve(c, c->wire_plan, 32 + 32 * (size_t)n)) != SF_OK) return rc;
  return sf_buf_reserve(c, c->wire_status, 16);
}

extern "C" int sf_store_export_plan(sf_handle c, int32_t first_slot, int32_t n, uint64_t* total_bytes, int32_t* max_rows) {
  if (!c) return SF_EINVAL;
  int rc = wire_export_begin(c, first_slot, n);
  if (rc != SF_OK) return rc;
  // (a size question: the status of the last export or import stays as it is)
  if ((rc = sf_launch_kfblob_plan(c, c->store, first_slot, n, c->wire_plan.p, nullptr)) != SF_OK) return rc;
  sf_kfblob_header h;
  SF_HIP(c, hipMemcpyAsync(&h, c->wire_plan.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));
  if (total_bytes) *total_bytes = h.total_bytes;
  if (max_rows) *max_rows = h.max_rows;
  return SF_OK;
}

extern "C" int sf_store_export_keyframes_device(sf_handle c, int32_t first_slot, int32_t n, void* d_blob, uint64_t cap_bytes) {
  if (!c) return SF_EINVAL;
  if (!d_blob || ((uintptr_t)d_blob & 15)) return sf_fail(c, SF_EINVAL, "the blob's buffer is missing or not 16-byte aligned");
  int rc = wire_export_begin(c, first_slot, n);
  if (rc != SF_OK) return rc;
  int32_t* status = (int32_t*)c->wire_status.p;
  if ((rc = sf_launch_kfblob_plan(c, c->store, first_slot, n, c->wire_plan.p, status)) != SF_OK) return rc;
  return sf_launch_kfblob_pack(c, c->store, first_slot, n, c->wire_plan.p, d_blob, cap_bytes, status);
}

extern "C" int sf_store_import_keyframes_device(sf_handle c, const void* d_blob, uint64_t bytes, int32_t n, int32_t max_rows,
                                                int32_t cols, int32_t* out_first_slot) {
  if (!c || n < 0 || max_rows < 0) return SF_EINVAL;
  if (!d_blob || ((uintptr_t)d_blob & 15)) return sf_fail(c, SF_EINVAL, "the blob is missing or not 16-byte aligned");
  if (n > SF_KFBLOB_MAX_KEYFRAMES) return sf_fail(c, SF_ERANGE, "%d keyframes in one blob (at most %d)", n, SF_KFBLOB_MAX_KEYFRAMES);
  SF_HIP(c, hipSetDevice(c->device));
  int rc;
  if ((rc = sf_buf_reserve(c, c->wire_status, 16)) != SF_OK) return rc;
  if (n > 0 && (rc = sf_store_reserve(c, c->store, c->store.slots + n, max_rows, cols)) != SF_OK) return rc;
  if ((rc = sf_launch_kfblob_unpack(c, c->store, c->store.slots, n, max_rows, cols, d_blob, bytes, (int32_t*)c->wire_status.p)) != SF_OK)
    return rc;
  if (out_first_slot) *out_first_slot = c->store.slots;
  c->store.slots += n;
  return SF_OK;
}

extern "C" int sf_store_wire_status(sf_handle c, int32_t out[4]) {
  if (!c || !out) return SF_EINVAL;
  out[0] = 0; out[1] = 0; out[2] = -1; out[3] = 0;
  SF_HIP(c, hipSetDevice(c->device));
  if (c->wire_status.p) SF_HIP(c, hipMemcpyAsync(out, c->wire_status.p, 16, hipMemcpyDeviceToHost, c->stream));
  SF_HIP(c, hipStreamSynchronize(c->stream));
  if (out[0] == 0) return SF_OK;
  return sf_fail(c, SF_ERANGE, "store wire:%s%s%s (%d slot(s) left empty, the first is keyframe %d of the blob)",
                 (out[0] & 1) ? " the export did not fit its buffer" : "", (out[0] & 2) ? " bad header" : "",
                 (out[0] & 4) ? " bad entry" : "", out[1], out[2]);
}

extern "C" int sf_store_size(sf_handle c, int32_t* n_slots) {
  if (!c || !n_slots) return SF_EINVAL;
  *n_slots = c->store.slots;
  return SF_OK;
}

extern "C" int sf_store_clear(sf_handle c) {
  if (!c) return SF_EINVAL;
  (void)sf_lanes_touch(c, true);
  SF_HIP(c, hipStreamSynchronize(c->stream));
  c->store.slots = 0;
  c->cam_tags.clear();           // (the ids go with the slots; the table and the selection stay)
  c->cam_nonzero = 0;
  c->cam_dev_n = 0;
  return SF_OK;
}

// ---- camera models: a table per handle, an id per store slot ------------------------------------------------------------
// No append path stamps its slots itself: the slots behind cam_tags.size() are the ones appended since the ids were last
// written out, and they carry the id selected then -- written out here, before the selection changes and before an id is
// read.
static void camera_settle(sf_context* c) {
  const size_t n = (size_t)std::max(c->store.slots, 0);
  if (c->cam_tags.size() > n) {          // (slots were dropped without their ids -- see Store::slots: the ids go now)
    c->cam_tags.resize(n);
    c->cam_nonzero = (int)(n - (size_t)std::count(c->cam_tags.begin(), c->cam_tags.end(), (uint8_t)0));
    c->cam_dev_n = 0;
  }
  if (c->cam_tags.size() >= n) return;
  if (c->cam_sel) c->cam_nonzero += (int)(n - c->cam_tags.size());
  c->cam_tags.resize(n, (uint8_t)c->cam_sel);
}

bool sf_camera_active(const sf_context* c) {
  return c->cam_nonzero > 0 || (c->cam_sel != 0 && (size_t)std::max(c->store.slots, 0) > c->cam_tags.size());
}

int sf_camera_sync(sf_context* c) {
  camera_settle(c);
  const int n = c->store.slots;
  if (c->cam_nonzero == 0 || c->cam_dev_n >= n) return SF_OK;     // (no kernel reads an id / the copy is current)
  hipStream_t s0 = c->ws[0].stream;
  if (c->cam_tags_dev.bytes < (size_t)n) {
    (void)sf_lanes_touch(c, true);                                  // the old array is freed: nothing may still read it
    SF_HIP(c, hipStreamSynchronize(s0));
    const int rc = sf_buf_reserve(c, c->cam_tags_dev, (size_t)std::max(n, c->store.cap_slots));
    if (rc != SF_OK) return rc;
  }
  // (every step in flight was settled by the append or by sf_store_set_camera; what is queued on the handle's stream is
  //  ordered before the copy, and the wait makes the ids visible to whichever stream the verification runs on)
  SF_HIP(c, hipMemcpyAsync(c->cam_tags_dev.p, c->cam_tags.data(), (size_t)n, hipMemcpyHostToDevice, s0));
  SF_HIP(c, hipStreamSynchronize(s0));
  c->cam_dev_n = n;
  return SF_OK;
}

static sf_camera_model camera_of_params(const sf_params& p) {
  sf_camera_model m;
  memset(&m, 0, sizeof(m));
  m.fx = p.fx; m.fy = p.fy; m.cx = p.cx; m.cy = p.cy;
  m.image_width = p.image_width; m.image_height = p.image_height;
  memcpy(m.local_transform, p.local_transform, sizeof(m.local_transform));
  m.stereo_baseline = p.stereo_baseline;
  return m;
}

static void camera_table_facts(sf_context* c) {
  c->cam_max_cells = 0;
  bool any_cal = false, any_uncal = false;
  for (const CameraBlock& b : c->cam_blocks) {
    c->cam_max_cells = std::max(c->cam_max_cells, b.grid_gx * b.grid_gy);
    (b.calibrated ? any_cal : any_uncal) = true;
  }
  c->cam_mixed_calibration = any_cal && any_uncal;
}

extern "C" int sf_camera_add(sf_handle c, const sf_camera_model* m, int32_t* id_out) {
  if (!c || !m || !id_out) return SF_EINVAL;
  const double k[4] = {m->fx, m->fy, m->cx, m->cy};
  for (double v : k)
    if (!std::isfinite(v) || v < 0.0) return sf_fail(c, SF_EINVAL, "sf_camera_add: fx, fy, cx, cy must be finite and >= 0");
  if (m->image_width < 0 || m->image_height < 0) return sf_fail(c, SF_EINVAL, "sf_camera_add: image size %d x %d", m->image_width, m->image_height);
  if (!std::isfinite(m->stereo_baseline) || m->stereo_baseline < 0.f) return sf_fail(c, SF_EINVAL, "sf_camera_add: stereo_baseline must be finite and >= 0");
  for (float v : m->local_transform)
    if (!std::isfinite(v)) return sf_fail(c, SF_EINVAL, "sf_camera_add: local_transform holds a non-finite value");
  if (m->reserved != 0) return sf_fail(c, SF_EINVAL, "sf_camera_add: reserved must be 0");
  if ((int)c->cam_models.size() >= SF_MAX_CAMERAS) return sf_fail(c, SF_ERANGE, "sf_camera_add: the table holds %d models", SF_MAX_CAMERAS);
  SF_HIP(c, hipSetDevice(c->device));
  int rc;
  // the whole table is reserved once, so the kernels of earlier calls keep reading valid memory while an entry no slot
  // of theirs names is written
  if ((rc = sf_buf_reserve(c, c->cam_table, (size_t)(SF_MAX_CAMERAS + 1) * sizeof(CameraBlock))) != SF_OK) return rc;
  CameraBlock b0, b;
  sf_camera_derive(camera_of_params(c->params), c->params.guess_win_size, &b0);
  sf_camera_derive(*m, c->params.guess_win_size, &b);
  const bool first = c->cam_blocks.empty();
  const int id = (int)c->cam_models.size() + 1;
  hipStream_t s0 = c->ws[0].stream;
  if (first) SF_HIP(c, hipMemcpyAsync(c->cam_table.p, &b0, sizeof(b0), hipMemcpyHostToDevice, s0));
  SF_HIP(c, hipMemcpyAsync((CameraBlock*)c->cam_table.p + id, &b, sizeof(b), hipMemcpyHostToDevice, s0));
  SF_HIP(c, hipStreamSynchronize(s0));
  if (first) c->cam_blocks.push_back(b0);
  c->cam_blocks.push_back(b);
  c->cam_models.push_back(*m);
  camera_table_facts(c);
  *id_out = id;
  return SF_OK;
}

extern "C" int sf_camera_get(sf_handle c, int32_t id, sf_camera_model* out) {
  if (!c || !out) return SF_EINVAL;
  if (id < 0 || id > (int)c->cam_models.size()) return sf_fail(c, SF_EINVAL, "camera id %d outside the table (0 .. %d)", id, (int)c->cam_models.size());
  *out = id == 0 ? camera_of_params(c->params) : c->cam_models[id - 1];
  return SF_OK;
}

extern "C" int sf_camera_count(sf_handle c, int32_t* n_out) {
  if (!c || !n_out) return SF_EINVAL;
  *n_out = (int32_t)c->cam_models.size();
  return SF_OK;
}

extern "C" int sf_camera_select(sf_handle c, int32_t id) {
  if (!c) return SF_EINVAL;
  if (id < 0 || id > (int)c->cam_models.size()) return sf_fail(c, SF_EINVAL, "camera id %d outside the table (0 .. %d)", id, (int)c->cam_models.size());
  camera_settle(c);
  c->cam_sel = id;
  return SF_OK;
}

extern "C" int sf_store_set_camera(sf_handle c, int32_t first_slot, int32_t n, int32_t id) {
  if (!c) return SF_EINVAL;
  if (id < 0 || id > (int)c->cam_models.size()) return sf_fail(c, SF_EINVAL, "camera id %d outside the table (0 .. %d)", id, (int)c->cam_models.size());
  if (first_slot < 0 || n < 0 || (long long)first_slot + n > c->store.slots)
    return sf_fail(c, SF_EINVAL, "slots %d .. %lld lie outside the store's %d", first_slot, (long long)first_slot + n, c->store.slots);
  if (n == 0) return SF_OK;
  // the steps in flight were issued on the ids as they are: settled and drained before the device copy is written again
  (void)sf_lanes_touch(c, true);
  SF_HIP(c, hipStreamSynchronize(c->ws[0].stream));
  camera_settle(c);
  for (int i = first_slot; i < first_slot + n; ++i) {
    c->cam_nonzero += (id != 0) - (c->cam_tags[i] != 0);
    c->cam_tags[i] = (uint8_t)id;
  }
  c->cam_dev_n = 0;
  return SF_OK;
}

extern "C" int sf_store_get_camera(sf_handle c, int32_t slot, int32_t* id_out) {
  if (!c || !id_out) return SF_EINVAL;
  if (slot < 0 || slot >= c->store.slots) return sf_fail(c, SF_EINVAL, "slot %d outside the store's %d", slot, c->store.slots);
  camera_settle(c);
  *id_out = c->cam_tags[slot];
  return SF_OK;
}
