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

}  // namespace mp
