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

// n keys by their bits [bit0, bit1), ascending or descending
int sf_sort_keys(sf_context* c, const unsigned long long* in, unsigned long long* out, size_t n, unsigned bit0, unsigned bit1,
                 bool descending) {
  return sort_with_tmp(c, [&](void* tmp, size_t& tmp_bytes) {
    return descending ? rocprim::radix_sort_keys_desc(tmp, tmp_bytes, in, out, n, bit0, bit1, c->stream)
                      : rocprim::radix_sort_keys(tmp, tmp_bytes, in, out, n, bit0, bit1, c->stream);
  });
}

// every segment [d_begin[s], d_end[s]) of the n_total keys on its own, ascending or descending; the bounds are read on the
// device, keys outside every segment are neither read nor written
int sf_sort_keys_segmented(sf_context* c, const unsigned long long* in, unsigned long long* out, unsigned n_total,
                           unsigned n_segments, const unsigned* d_begin, const unsigned* d_end, unsigned bit0, unsigned bit1,
                           bool descending) {
  return sort_with_tmp(c, [&](void* tmp, size_t& tmp_bytes) {
    return descending ? rocprim::segmented_radix_sort_keys_desc(tmp, tmp_bytes, in, out, n_total, n_segments, d_begin, d_end,
                                                                bit0, bit1, c->stream)
                      : rocprim::segmented_radix_sort_keys(tmp, tmp_bytes, in, out, n_total, n_segments, d_begin, d_end, bit0,
                                                           bit1, c->stream);
  });
}

int sf_sort_keys_segmented_desc(sf_context* c, const unsigned long long* in, unsigned long long* out, unsigned n_total,
                                unsigned n_segments, const unsigned* d_begin, const unsigned* d_end, unsigned bit0,
                                unsigned bit1) {
  return sf_sort_keys_segmented(c, in, out, n_total, n_segments, d_begin, d_end, bit0, bit1, true);
}
