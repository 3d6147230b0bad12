// sf_sort.hip -- the one library call of the product's compute path: rocprim's radix sort of 64-bit keys, for the
// detectors of the feature front end (k_gftt.hip, k_fast.hip, k_orb_detect.hip).  This is the only translation unit that
// includes rocprim, so its sort kernels are compiled once.  All functions size the temporary storage, keep it in
// c->gf_tmp and sort on the handle's stream; the keys are integers, so the file needs no floating-point flags.
#include <hip/hip_runtime.h>

#include <cstring>   // (rocprim's texture_cache_iterator.hpp calls memset without declaring it)

#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "sf_internal.hpp"

// sort(tmp, tmp_bytes) is one rocprim call: asked for the size first (tmp null), then run with c->gf_tmp
template <class Sort>
static int sort_with_tmp(sf_context* c, Sort sort) {
  size_t tmp_bytes = 0;
  SF_HIP(c, sort(nullptr, tmp_bytes));
  int rc = sf_buf_reserve(c, c->gf_tmp, std::max<size_t>(tmp_bytes, 16));
  if (rc != SF_OK) return rc;
  SF_HIP(c, sort(c->gf_tmp.p, tmp_bytes));
  return SF_OK;
}

// n keys by their bits [bit0, bit1), ascending or descending: one device-wide sort
static int sort_keys(sf_context* c, const unsigned long long* in, unsigned long long* out, size_t n, unsigned bit0, unsigned bit1,
                     bool descending) {
  return sort_with_tmp(c, [&](void* tmp, size_t& tmp_bytes) {
    return descending ? rocprim::radix_sort_keys_desc(tmp, tmp_bytes, in, out, n, bit0, bit1, c->stream)
                      : rocprim::radix_sort_keys(tmp, tmp_bytes, in, out, n, bit0, bit1, c->stream);
  });
}

// The detectors' sort: image s's keys are the segment [d_begin[s], d_end[s]) of the n_total keys, bounds its decide kernel
// has written on the device; keys outside every segment are neither read nor written.  Several images: rocprim's segmented
// sort reads the bounds on the device, nothing waits.  It gives each segment to ONE workgroup, though, and a lone image
// has tens of thousands of keys in its one segment -- so one image is a device-wide sort sized by the host: its two
// bounds cross to the host here, with the one wait a single call has for its count anyway, and come back in `hb` for
// whatever else the caller sizes by them.  The rule goes by n_segments alone, so a batch call with one keyframe, the last
// one-image chunk of a SURF or SIFT batch and a grid of one cell wait once here too.  A caller with several sorts over one range (ORB) passes the same `hb` again:
// bounds that are known are not fetched twice.
int sf_sort_segments(sf_context* c, const unsigned long long* in, unsigned long long* out, unsigned n_total, unsigned n_segments,
                     const unsigned* d_begin, const unsigned* d_end, unsigned bit0, unsigned bit1, bool descending,
                     SfSortBounds* hb) {
  if (n_segments > 1)
    return sort_with_tmp(c, [&](void* tmp, size_t& tmp_bytes) {
      return descending ? rocprim::segmented_radix_sort_keys_desc(tmp, tmp_bytes, in, out, n_total, n_segments, d_begin, d_end,
                                                                  bit0, bit1, c->stream)
                        : rocprim::segmented_radix_sort_keys(tmp, tmp_bytes, in, out, n_total, n_segments, d_begin, d_end, bit0,
                                                             bit1, c->stream);
    });
  if (!hb->known) {
    // The bounds, and the further words that the caller wants with them (hb->d_also), with ONE wait.  A single call's
    // words lie in one control block, within 64 words of each other, and then cross in one copy as the parent's count
    // did; words further apart (the last one-image chunk of a large batch) cross one by one.  The addresses are compared
    // as integers: they need not belong to one allocation.  That one copy is cheaper than four has not been measured.
    const unsigned* src[4] = {d_begin, d_end, hb->d_also[0], hb->d_also[1]};
    unsigned* dst[4] = {&hb->begin, &hb->end, &hb->also[0], &hb->also[1]};
    uintptr_t lo = (uintptr_t)d_begin, hi = lo;
    for (const unsigned* p : src)
      if (p) { lo = std::min(lo, (uintptr_t)p); hi = std::max(hi, (uintptr_t)p); }
    unsigned words[64];
    const bool one_copy = hi - lo < sizeof(words);
    if (one_copy) SF_HIP(c, hipMemcpyAsync(words, (const void*)lo, hi - lo + 4, hipMemcpyDeviceToHost, c->stream));
    for (int i = 0; i < 4 && !one_copy; ++i)
      if (src[i]) SF_HIP(c, hipMemcpyAsync(dst[i], src[i], 4, hipMemcpyDeviceToHost, c->stream));
    SF_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 4 && one_copy; ++i)
      if (src[i]) *dst[i] = words[((uintptr_t)src[i] - lo) / 4];
    hb->known = true;
  }
  if (hb->end <= hb->begin) return SF_OK;
  return sort_keys(c, in + hb->begin, out + hb->begin, (size_t)(hb->end - hb->begin), bit0, bit1, descending);
}
