// `microphaser build_reference` on the device (reference: src/peptides.rs:148-186, src/main.rs:146-169).
#pragma once
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

#include "model.hpp"

namespace mp {

// ---- peptide keys: the one place that defines their format
// key = sum_j ((aa_j - 'A') & 31) << 5 (L - 1 - j): 5 bits per residue, first residue most significant, so that keys of one length
// sort in string order. L <= 12 fits one u64 word; 13 <= L <= 25 takes two words (125 bits at most), stored as an unsigned 128-bit
// little-endian integer - low word first, the bytes of `unsigned __int128` / rocprim::uint128_t.
constexpr uint32_t MAX_PEPTIDE_LEN = 25;
constexpr uint32_t key_words(uint32_t L) { return L <= 12 ? 1u : 2u; }
void check_peptide_len(uint32_t L);   // throws unless 1 <= L <= MAX_PEPTIDE_LEN

using key128 = unsigned __int128;
key128 peptide_to_key(const char* pep, size_t L);
std::string peptide_from_key(key128 key, uint32_t L);
// key i of an array of `w`-word keys
inline key128 key_at(const uint64_t* words, size_t i, uint32_t w) {
    return w == 1 ? key128(words[i]) : (key128(words[2 * i + 1]) << 64) | words[2 * i];
}
inline void push_key(std::vector<uint64_t>& words, key128 k, uint32_t w) {
    words.push_back(uint64_t(k));
    if (w == 2) words.push_back(uint64_t(k >> 64));
}

struct PeptideResult {
    std::string fasta;                // translated FASTA (stdout of `build_reference`)
    std::vector<uint64_t> keys;       // sorted distinct peptide keys, key_words(peptide_len) words each
    uint32_t peptide_len = 9;
    uint64_t n_peptides = 0;          // translated windows
    float translate_ms = 0, dedup_ms = 0;
    size_t n_keys() const { return keys.size() / key_words(peptide_len); }
    std::string binary() const;       // bincode v1 HashSet<Vec<u8>> of the distinct peptides (order = key order)
};

// Translate every 3-nt-step window of every record of a nucleotide FASTA and de-duplicate, on HIP device `device`.
// want_fasta = false: the peptidome (keys, binary) only - what a pipeline that feeds `filter` needs; the translated FASTA stays empty.
void build_reference_device(int device, std::string_view fasta_text, uint32_t peptide_len, PeptideResult& out, bool want_fasta = true);   // (the text is read in place)

// ---- `normal` -> `build_reference` without the FASTA text: one source per record the `normal` consumer would print
// (consume.cpp), translated straight from the device record arena (kernels_pep.hip k4_translate_sources).
enum : uint8_t { SRC_REV = 1, SRC_MERGE = 2 };
struct PepSource {       // 8 bytes; 100 M of them stand in for ~5 GB of FASTA text
    uint32_t idx;        // SRC_MERGE clear: record slot in the device arena (GroupSum::rec); set: index of a window_len-byte sequence in the merge buffer
    uint8_t off;         // first base within the record's sequence (device records only)
    uint8_t flags;       // SRC_REV: reverse-complement (the printed id does not end in 'F', src/peptides.rs:161-164)
    uint16_t len;        // bases
};
static_assert(sizeof(PepSource) == 8, "PepSource layout");
// windows of a record of `len` bases: peptides::build's `while i + 3L <= len` loop, step 3 (src/peptides.rs:165-174)
inline uint64_t source_windows(uint64_t len, uint32_t L) { return len >= 3ull * L ? (len - 3ull * L) / 3 + 1 : 0; }
struct PepSources {      // the records of a batch in gene order, and the host-built sequences of its splice-side merges
    PodVec<PepSource> src;
    PodVec<uint8_t> merge;        // n_merge * merge_len bytes
    uint32_t merge_len = 0;       // the batch's window length
    uint64_t n_merge = 0;
};
// The device arena the sources name: record i's sequence starts at recs + i * rec_stride + 32 (HapRecHdr), seq_cap bytes at most.
struct RecArena {
    const uint8_t* recs = nullptr;
    uint64_t n_slots = 0;
    uint32_t rec_stride = 0, seq_cap = 0;
};
// Translate every window of every source and de-duplicate on HIP device `device` (the one that holds the arena): the keys, count and
// bincode image build_reference_device gives on the FASTA those records would have been printed as.
void peptidome_from_sources(int device, const PepSources& s, const RecArena& arena, uint32_t peptide_len, PeptideResult& out);

}  // namespace mp
