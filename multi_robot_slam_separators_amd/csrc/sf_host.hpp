// sf_host.hpp -- what the host translation units (sf_handle.hip, sf_store.hip, sf_features.hip, sf_verify_host.hip,
// sf_step.hip, sf_placement.hip) need from each other; the kernel translation units do not include it.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>

#include "sf_internal.hpp"

// ---- sf_handle.hip ------------------------------------------------------------------------------------------------------
int sf_fill_device_params(sf_context* c);      // validates c->params and derives c->dparams
void sf_env_knobs(sf_context* c);              // the SF_* environment knobs of a handle, applied to `c`

// ---- sf_store.hip -------------------------------------------------------------------------------------------------------
int sf_validate_features(sf_context* c, const sf_features* f);
int sf_store_reserve(sf_context* c, Store& s, int slots_needed, int rows, int cols);
int sf_store_add_host_batch(sf_context* c, Store& st, const sf_features* const* feats, int n, int* first_slot);
void sf_ingest_pool_destroy(sf_context* c);

// ---- sf_verify_host.hip -------------------------------------------------------------------------------------------------
// ONE object decides the launch form of a verification call AND what its workspace must hold: it is made once per call
// from the call's total pair count, the workspace is reserved from it and every chunk is launched from it.  (Round 3 made
// the form decision per chunk and the reservation per call: the second chunk of a 140 000-candidate step took the split
// form, which writes correspondence lists, on a workspace reserved for the fused form, which has none -- a device
// out-of-bounds write; tests/test_gpu_step.py::test_step_queries_across_the_form_and_chunk_boundaries.)
struct VerifyPlan {
  enum Form { STAGES = 0, FUSED = 1, SPLIT = 2, SPLIT_PNP = 3, HALVES = 4 } form = STAGES;
  bool lists = true;        // the correspondence lists live in HBM (every form but the plain fused kernel)
  bool single = false;      // one launch sequence on one stream: a pair's index IS its position in the call
  bool narrow_est = false;  // SPLIT only: the survivors' chains as three launches, the estimates one wavefront wide (k_chain_est)
  bool streams() const { return single && (form == FUSED || form == SPLIT || form == SPLIT_PNP); }   // chain kernels that can
};                                                                                                // stream accepted results
VerifyPlan sf_verify_plan(const sf_context* c, const StoreView& v, int n);
int sf_verify_device(sf_context* c, const Store& st, const int32_t* d_from, const int32_t* d_to, int n, sf_result* d_out,
                     const VerifyPlan* given = nullptr);
int sf_compact_launch(sf_context* c, const sf_result* d_results, int n, sf_result* d_accepted, uint8_t* d_flags,
                      int32_t* d_count, const int32_t* index = nullptr, sf_result* d_accepted2 = nullptr,
                      uint8_t* d_flags2 = nullptr, int32_t* d_count2 = nullptr, int cap2 = 0x7FFFFFFF);

// ---- sf_placement.hip ---------------------------------------------------------------------------------------------------
// A stream beside the handle's own: the copy stream of the synchronous speculative call, the main stream of step lane k, or
// lane k's second stream (the device walk beside the verification)
enum SideStream { SF_STREAM_COPY, SF_STREAM_LANE, SF_STREAM_AUX };
int sf_side_stream(sf_context* c, SideStream role, int k, hipStream_t* out);
