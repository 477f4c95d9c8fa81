// `microphaser filter` (reference: src/peptides.rs:188-709, src/main.rs:170-214): removes neopeptides that also occur in
// the normal peptidome and annotates the rest with a maximum-likelihood frequency and a 95 % credible interval.
// Translation + peptidome membership (K5) and the per-group statistics (K6) run on the device; the row-stream
// bookkeeping of the reference (stop-gain suppression, per-variant-region grouping, de-duplication) stays on the host.
#pragma once
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#include "model.hpp"
#include "pep.hpp"

namespace mp {

// One row of info.tsv (IDRecord, src/common.rs:350-373): text fields as views (into the TSV text, the unescaped form of a quoted
// field, or - for rows captured by the `somatic` consumer - the gene model, a capture's TextArena or the downloaded record arena),
// numbers as values.
// a string_view without a constructor, so that a Row can be created uninitialised (the parsing threads fill 8.8 M of them in place)
struct SV {
    const char* p;
    size_t n;
    SV& operator=(std::string_view v) { p = v.data(); n = v.size(); return *this; }
    operator std::string_view() const { return std::string_view(p, n); }
    bool empty() const { return n == 0; }
    size_t size() const { return n; }
    const char* data() const { return p; }
    char back() const { return p[n - 1]; }
    size_t find(char c) const { return std::string_view(p, n).find(c); }
};
inline bool operator==(const SV& a, const SV& b) { return std::string_view(a) == std::string_view(b); }
inline bool operator!=(const SV& a, const SV& b) { return !(a == b); }
inline bool operator==(const SV& a, const char* b) { return std::string_view(a) == std::string_view(b); }

struct Row {
    SV id, transcript, gene_id, gene_name, chrom, strand, variant_sites, somatic_positions, somatic_aa_change, germline_positions,
        germline_aa_change, normal_sequence, mutant_sequence;
    uint64_t offset, frame;
    double freq;
    uint32_t depth, nvar, nsomatic, nvariant_sites, nsomvariant_sites;
};
using RowVec = PodVec<Row>;   // rows are sized once and filled in place (no zero fill: 250 bytes x 8.8 M rows)

// ---- `somatic` -> `filter` without the TSV text: the rows the `somatic` consumer would write, captured as Rows (consume.cpp), and
// for each the place of its two nucleotide windows, which K5 reads where they lie (kernels_filter.hip k5_translate_row_sources).
enum : uint8_t { SRC_GERM = 4 };   // (beside pep.hpp's SRC_REV, SRC_MERGE)
struct RowSeq {          // 16 bytes; row r's mutant window is seq[2r], its normal window seq[2r + 1]
    uint64_t at;         // SRC_MERGE clear: record slot in the device arena (GroupSum::rec); set: byte offset in RowCapture::side
    uint32_t len;        // bases (0: no normal window)
    uint16_t off;        // first base within the record's half (device records only)
    uint8_t flags;       // SRC_GERM: the record's germline half (rec_germ); SRC_REV: reverse-complement (the row id does not end in 'F')
    uint8_t pad;
};
static_assert(sizeof(RowSeq) == 16, "RowSeq layout");

// Stable storage for the text fields of captured rows (the consumer's list fields live in per-thread scratch): blocks that never move.
struct TextArena {
    std::vector<std::unique_ptr<char[]>> blocks;
    char* at = nullptr;
    size_t left = 0;
    std::string_view put(std::string_view s) {
        if (s.empty()) return std::string_view();
        if (s.size() > left) {
            const size_t n = std::max<size_t>(s.size(), size_t(1) << 20);
            blocks.emplace_back(new char[n]);
            at = blocks.back().get();
            left = n;
        }
        std::memcpy(at, s.data(), s.size());
        const std::string_view v(at, s.size());
        at += s.size();
        left -= s.size();
        return v;
    }
};

struct RowCapture {      // the rows of a `somatic` batch in TSV order
    RowVec rows;
    PodVec<RowSeq> seq;                          // 2 per row
    PodVec<uint8_t> side;                        // the sequences of the splice-side merges' rows, back to back
    std::vector<TextArena> text;                 // owns the copied text fields
};

struct FilterResult {
    PodVec<char> fasta;          // stdout: kept tumor peptides
    PodVec<char> normal_fasta;   // --normal-output
    PodVec<char> tsv;            // --tsv-output (header always present)
    PodVec<char> removed_tsv;    // --similar-removed
    PodVec<char> removed_fasta;  // --removed-peptides
    uint64_t n_rows = 0, n_peptides = 0, n_groups = 0, n_kept = 0, n_removed = 0;
    float translate_ms = 0, stats_ms = 0;
};

// The filter of a row stream that arrives in parts, in TSV (GTF) order: every add translates its rows on the device (K5) and advances
// the reference's row stream over them (stop-gain suppression, de-duplication, per-variant-region groups), whose state carries over from
// one add to the next; finish scores the groups (K6) and writes the five streams. Adds may run on different devices; each part's rows,
// amino acids and whatever their views point into are owned by the stream until finish. The result is byte for byte that of ONE add of
// all the rows - and an add that throws reports what that one add would have thrown first.
// reference_binary: bytes of the bincode HashSet<Vec<u8>> written by build_reference (decoded here, once; a decoding error is reported
// where the one-part filter reports it: by the first add or by finish) - or, with reference_keys != nullptr, the peptidome as sorted
// distinct keys of peptide_len residues, key_words(peptide_len) words each (PeptideResult::keys, not copied: it must outlive the stream).
// The reference goes to each device the stream meets once.
class FilterStream {
public:
    FilterStream(std::string_view reference_binary, const std::vector<uint64_t>* reference_keys, uint32_t peptide_len);
    ~FilterStream();
    FilterStream(const FilterStream&) = delete;
    FilterStream& operator=(const FilterStream&) = delete;
    // Rows captured from a `somatic` batch that is resident on `device`: the windows are read from its record arena and from cap.side
    // (k5_translate_row_sources) - no TSV text, no parse, no upload of the windows. `hold` keeps alive what else the rows' views point
    // into (the downloaded records, a batch's copies of split genes); the data set's gene model must outlive the stream.
    void add_captured(int device, RowCapture&& cap, const RecArena& arena, std::shared_ptr<const void> hold);
    // The rows of an info.tsv text (header first), read in place: the text must stay valid until finish.
    void add_text(int device, std::string_view tsv_text);
    void finish(int device, FilterResult& out);
private:
    struct State;
    std::unique_ptr<State> s;
};

// reference_binary / reference_keys as for FilterStream; tsv_text: info.tsv of `somatic`. Both buffers are read in place and must stay
// valid for the call.
// (one FilterStream::add_text, then finish). Rows captured from `somatic` batches take the same stream through add_captured: same bytes,
// counts and errors as filter_device on the TSV those rows would have been written as.
void filter_device(int device, std::string_view reference_binary, const std::vector<uint64_t>* reference_keys, std::string_view tsv_text,
                   uint32_t peptide_len, FilterResult& out);

}  // namespace mp
