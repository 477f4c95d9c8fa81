// Launch interface of the translation / peptidome kernels (kernels_pep.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pep.hpp"

namespace mp {
// Key arrays are u64 words, key_words(L) of them per key (pep.hpp); buffers of two-word keys must be 16-byte aligned (hipMalloc is).
void device_translate(const uint8_t* d_nt, const uint64_t* d_off, const uint8_t* d_rev, uint64_t n, uint32_t L, uint8_t* d_aa,
                      uint64_t* d_keys, uint32_t* d_err, hipStream_t stream);
// the keys of the n_win windows of n_src sources (k4_translate_sources): d_win_at gets the exclusive scan of their window counts
// (n_src words); a source names a record of the arena at d_recs (rec_stride bytes apart) or a merge_len-byte sequence at d_merge
void device_translate_sources(const PepSource* d_src, uint64_t* d_win_at, uint64_t n_src, uint64_t n_win, const uint8_t* d_recs, uint32_t rec_stride,
                              const uint8_t* d_merge, uint32_t merge_len, uint32_t L, uint64_t* d_keys, uint32_t* d_err, hipStream_t stream);
// sort + unique of n keys of peptide length L; returns the number of distinct keys (in d_out)
uint64_t device_sort_unique(uint64_t* d_keys, uint64_t* d_tmp, uint64_t* d_out, uint64_t n, uint32_t L, hipStream_t stream);
}  // namespace mp
