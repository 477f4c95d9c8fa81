// K4: codon -> peptide translation and reference-peptidome keys (reference: src/peptides.rs:85-146 to_protein /
// to_aminoacid / make_pairs, :148-186 build). One thread per peptide window; integer/byte work, HBM-bound:
// reads 3L nucleotide bytes (neighbouring windows overlap by 3L-3, so the stream is read once through L2),
// writes L amino-acid bytes + one key (a u64 for L <= 12, a 16-byte uint128 for 13 <= L <= 25: pep.hpp). De-duplication = radix sort
// + unique on the keys (rocPRIM device primitives, called directly).
// k4_translate_sources: the same translation for the records of a `normal` run, read from the device record arena (and a small
// buffer of host-merged sequences) instead of a parsed FASTA: `normal` -> `build_reference` without the nucleotide text.
#include <hip/hip_runtime.h>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/functional.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "kernels_pep.hpp"
#include "pep.hpp"

namespace mp {

[[noreturn]] void throw_hip(hipError_t e, const char* file, int line);
#define HIP_OK_(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw_hip(e_, __FILE__, __LINE__); } while (0)

// index = 16*b0 + 4*b1 + b2 with A=0 C=1 G=2 T=3; stop codons -> 'X' (src/peptides.rs:85-117)
__constant__ char CODON_AA[65] = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVVXYXYSSSSXCWCLFLF";

__device__ __forceinline__ int base2(uint8_t c, bool complement) {
    if (c >= 'a' && c <= 'z') c -= 32;  // to_ascii_uppercase (:129)
    int b;
    switch (c) { case 'A': b = 0; break; case 'C': b = 1; break; case 'G': b = 2; break; case 'T': b = 3; break; default: return -1; }
    return complement ? 3 - b : b;
}

// codon -> residue -> key of one window of 3L bases at s, reverse-complemented first when rev (src/peptides.rs:128-146): the step K4
// and k4_translate_sources share. kAA: also store the L residues at aa. A codon outside the table sets `bad` (its residue reads '?').
template <class K, bool kAA>
__device__ __forceinline__ K translate_window(const uint8_t* __restrict__ s, bool rev, uint32_t L, uint8_t* __restrict__ aa, bool& bad) {
    const uint32_t n3 = 3 * L;
    K key = 0;
    for (uint32_t j = 0; j < L; j++) {
        int b0, b1, b2;
        if (!rev) { b0 = base2(s[3 * j], false); b1 = base2(s[3 * j + 1], false); b2 = base2(s[3 * j + 2], false); }
        else { b0 = base2(s[n3 - 1 - 3 * j], true); b1 = base2(s[n3 - 2 - 3 * j], true); b2 = base2(s[n3 - 3 - 3 * j], true); }  // dna::revcomp (:133)
        char a = '?';
        if ((b0 | b1 | b2) < 0) bad = true;  // codon not in the table: the reference unwraps an Err (:136-139)
        else a = CODON_AA[16 * b0 + 4 * b1 + b2];
        if (kAA) aa[j] = uint8_t(a);
        key = (key << 5) | K((a - 'A') & 31);
    }
    return key;
}

// K = uint64_t (L <= 12) or rocprim::uint128_t (13 <= L <= 25): the key is built in registers and written with one store per window
template <class K>
__global__ __launch_bounds__(256) void k4_translate(const uint8_t* __restrict__ nt, const uint64_t* __restrict__ win_off,
                                                    const uint8_t* __restrict__ win_rev, uint64_t n, uint32_t L,
                                                    uint8_t* __restrict__ aa, K* __restrict__ keys, uint32_t* __restrict__ err) {
    uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    bool bad = false;
    keys[i] = translate_window<K, true>(nt + win_off[i], win_rev[i] != 0, L, aa + i * L, bad);
    if (bad) atomicOr(err, 1u);
}

// the last source s in [lo, hi) with win_at[s] <= w: the one that holds window w (sources without windows share their successor's offset)
__device__ __forceinline__ uint64_t source_of(const uint64_t* __restrict__ win_at, uint64_t lo, uint64_t hi, uint64_t w) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (win_at[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

// The peptide windows of `normal` records, read where they lie: one thread per window. win_at = exclusive scan of the sources' window
// counts. The block finds the sources of its first and last window, every thread then searches that short range for its own.
template <class K>
__global__ __launch_bounds__(256) void k4_translate_sources(const PepSource* __restrict__ src, const uint64_t* __restrict__ win_at, uint64_t n_src,
                                                            uint64_t n_win, const uint8_t* __restrict__ recs, uint32_t rec_stride,
                                                            const uint8_t* __restrict__ merge, uint32_t merge_len, uint32_t L,
                                                            K* __restrict__ keys, uint32_t* __restrict__ err) {
    __shared__ uint64_t s_range[2];
    const uint64_t w0 = uint64_t(blockIdx.x) * 256;
    if (threadIdx.x < 2) {
        const uint64_t w = threadIdx.x == 0 ? w0 : (w0 + 255 < n_win ? w0 + 255 : n_win - 1);
        s_range[threadIdx.x] = source_of(win_at, 0, n_src, w);
    }
    __syncthreads();
    const uint64_t i = w0 + threadIdx.x;
    if (i >= n_win) return;
    const uint64_t s = source_of(win_at, s_range[0], s_range[1] + 1, i);
    const PepSource ps = src[s];
    const uint8_t* base = (ps.flags & SRC_MERGE) ? merge + uint64_t(ps.idx) * merge_len : recs + uint64_t(ps.idx) * rec_stride + 32 + ps.off;
    bool bad = false;
    keys[i] = translate_window<K, false>(base + 3 * (i - win_at[s]), (ps.flags & SRC_REV) != 0, L, nullptr, bad);
    if (bad) atomicOr(err, 1u);
}

struct SourceWindows {   // scan input: a source's window count
    uint32_t L;
    __host__ __device__ uint64_t operator()(const PepSource& s) const { return s.len >= 3 * L ? (uint64_t(s.len) - 3 * L) / 3 + 1 : 0; }
};

void device_translate(const uint8_t* d_nt, const uint64_t* d_off, const uint8_t* d_rev, uint64_t n, uint32_t L, uint8_t* d_aa,
                      uint64_t* d_keys, uint32_t* d_err, hipStream_t stream) {
    if (!n) return;
    dim3 grid(uint32_t((n + 255) / 256)), block(256);
    if (key_words(L) == 1)
        hipLaunchKernelGGL(k4_translate<uint64_t>, grid, block, 0, stream, d_nt, d_off, d_rev, n, L, d_aa, d_keys, d_err);
    else
        hipLaunchKernelGGL(k4_translate<rocprim::uint128_t>, grid, block, 0, stream, d_nt, d_off, d_rev, n, L, d_aa,
                           reinterpret_cast<rocprim::uint128_t*>(d_keys), d_err);
    HIP_OK_(hipGetLastError());
}

void device_translate_sources(const PepSource* d_src, uint64_t* d_win_at, uint64_t n_src, uint64_t n_win, const uint8_t* d_recs, uint32_t rec_stride,
                              const uint8_t* d_merge, uint32_t merge_len, uint32_t L, uint64_t* d_keys, uint32_t* d_err, hipStream_t stream) {
    if (!n_src || !n_win) return;
    auto counts = rocprim::make_transform_iterator(d_src, SourceWindows{L});
    size_t bytes = 0;
    HIP_OK_(rocprim::exclusive_scan(nullptr, bytes, counts, d_win_at, uint64_t(0), size_t(n_src), rocprim::plus<uint64_t>(), stream));
    void* d_ws = nullptr;
    HIP_OK_(hipMalloc(&d_ws, bytes + 16));
    hipError_t e = rocprim::exclusive_scan(d_ws, bytes, counts, d_win_at, uint64_t(0), size_t(n_src), rocprim::plus<uint64_t>(), stream);
    if (e == hipSuccess) {
        dim3 grid(uint32_t((n_win + 255) / 256)), block(256);
        if (key_words(L) == 1)
            hipLaunchKernelGGL(k4_translate_sources<uint64_t>, grid, block, 0, stream, d_src, d_win_at, n_src, n_win, d_recs, rec_stride, d_merge,
                               merge_len, L, d_keys, d_err);
        else
            hipLaunchKernelGGL(k4_translate_sources<rocprim::uint128_t>, grid, block, 0, stream, d_src, d_win_at, n_src, n_win, d_recs, rec_stride,
                               d_merge, merge_len, L, reinterpret_cast<rocprim::uint128_t*>(d_keys), d_err);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);   // (before the scan's workspace goes)
    (void)hipFree(d_ws);
    HIP_OK_(e);
}

// sort + unique of keys of K over the bit range [0, key_bits); returns the number of distinct keys (in d_out[0..n_unique))
template <class K>
uint64_t sort_unique(K* d_keys, K* d_tmp, K* d_out, uint64_t n, uint32_t key_bits, hipStream_t stream) {
    const size_t count = size_t(n);   // (64-bit sizes throughout: a whole-exome normal peptidome has > 2^31 / 8 windows within reach)
    size_t bytes1 = 0, bytes2 = 0;
    HIP_OK_(rocprim::radix_sort_keys(nullptr, bytes1, d_keys, d_tmp, count, 0u, key_bits, stream));
    HIP_OK_(rocprim::unique(nullptr, bytes2, d_tmp, d_out, static_cast<uint64_t*>(nullptr), count, rocprim::equal_to<K>(), stream));
    const size_t ws_bytes = (std::max(bytes1, bytes2) + 255) & ~size_t(255);
    char* d_ws = nullptr;   // one allocation: workspace + the count word behind it
    HIP_OK_(hipMalloc(&d_ws, ws_bytes + 256));
    uint64_t* d_count = reinterpret_cast<uint64_t*>(d_ws + ws_bytes);
    uint64_t cnt = 0;
    hipError_t e = rocprim::radix_sort_keys(d_ws, bytes1, d_keys, d_tmp, count, 0u, key_bits, stream);
    if (e == hipSuccess) e = rocprim::unique(d_ws, bytes2, d_tmp, d_out, d_count, count, rocprim::equal_to<K>(), stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&cnt, d_count, 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d_ws);
    HIP_OK_(e);
    return cnt;
}

uint64_t device_sort_unique(uint64_t* d_keys, uint64_t* d_tmp, uint64_t* d_out, uint64_t n, uint32_t L, hipStream_t stream) {
    if (!n) return 0;
    if (key_words(L) == 1) return sort_unique(d_keys, d_tmp, d_out, n, 5 * L, stream);
    using K = rocprim::uint128_t;
    return sort_unique(reinterpret_cast<K*>(d_keys), reinterpret_cast<K*>(d_tmp), reinterpret_cast<K*>(d_out), n, 5 * L, stream);
}

}  // namespace mp
