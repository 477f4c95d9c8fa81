#include "filter.hpp"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <charconv>
#include <deque>
#include <exception>
#include <limits>
#include <map>
#include <set>
#include <string_view>
#include <thread>
#include <tuple>
#include <vector>

#include "batch.hpp"
#include "kernels_filter.hpp"
#include "kernels_pep.hpp"
#include "pep.hpp"
#include "rowfmt.hpp"

namespace mp {

[[noreturn]] void throw_hip(hipError_t e, const char* file, int line);
#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) throw_hip(e_, __FILE__, __LINE__); } while (0)

namespace {

uint64_t field_u64(std::string_view s, const char* name) {
    uint64_t v = 0;
    const auto r = std::from_chars(s.data(), s.data() + s.size(), v);
    if (s.empty() || r.ptr != s.data() + s.size() || r.ec == std::errc::invalid_argument)
        throw Error(std::string("CSV deserialize error: field ") + name + ": invalid digit found in string");
    if (r.ec == std::errc::result_out_of_range)
        throw Error(std::string("CSV deserialize error: field ") + name + ": number too large to fit in target type");
    return v;
}
uint32_t field_u32(std::string_view s, const char* name) {
    const uint64_t v = field_u64(s, name);
    if (v > 0xFFFFFFFFull) throw Error(std::string("CSV deserialize error: field ") + name + ": number too large to fit in target type");
    return uint32_t(v);
}
double field_f64(std::string_view s, const char* name) {
    char buf[64];
    std::string big;
    const char* z = buf;
    if (s.size() < sizeof buf) { std::memcpy(buf, s.data(), s.size()); buf[s.size()] = 0; }
    else { big.assign(s); z = big.c_str(); }
    char* e = nullptr;
    const double v = std::strtod(z, &e);
    if (s.empty() || *e) throw Error(std::string("CSV deserialize error: field ") + name + ": invalid float literal");
    return v;
}
void row_from_fields(const std::string_view* f, size_t n, Row& r) {   // serde positional deserialize of IDRecord
    if (n != 21) throw Error("CSV deserialize error: found record with " + std::to_string(n) + " fields, but expected 21");
    r.id = f[0]; r.transcript = f[1]; r.gene_id = f[2]; r.gene_name = f[3]; r.chrom = f[4];
    r.offset = field_u64(f[5], "offset");
    r.frame = field_u64(f[6], "frame");
    r.freq = field_f64(f[7], "freq");
    r.depth = field_u32(f[8], "depth");
    r.nvar = field_u32(f[9], "nvar");
    r.nsomatic = field_u32(f[10], "nsomatic");
    r.nvariant_sites = field_u32(f[11], "nvariant_sites");
    r.nsomvariant_sites = field_u32(f[12], "nsomvariant_sites");
    r.strand = f[13]; r.variant_sites = f[14]; r.somatic_positions = f[15]; r.somatic_aa_change = f[16];
    r.germline_positions = f[17]; r.germline_aa_change = f[18]; r.normal_sequence = f[19]; r.mutant_sequence = f[20];
}

// csv::ReaderBuilder::new().delimiter(b'\t') with default quoting over [p, end): every record after the first `skip` ones becomes a Row.
// Unquoted fields (all of them in what `somatic` writes, unless a value holds a tab, a quote or a line break) are byte ranges of the
// buffer; a field that starts with a quote is unescaped into `arena` ("" is a quote; the closing quote ends the quoting, further bytes
// up to the delimiter are appended).
void parse_rows(const char* p, const char* const end, size_t skip, RowVec& rows, std::deque<std::string>& arena) {
    std::vector<std::string_view> rec;
    rec.reserve(32);
    bool started = false;        // the current record holds at least one field or delimiter
    std::string_view field;
    auto end_record = [&]() {
        if (started || !field.empty()) {
            rec.push_back(field);
            if (skip) skip--;
            else { rows.emplace_back(); row_from_fields(rec.data(), rec.size(), rows.back()); }
            rec.clear();
        }
        field = std::string_view();
        started = false;
    };
    while (p < end) {
        if (*p == '"') {
            started = true;
            p++;
            std::string text;
            bool quoted = true;
            while (p < end) {
                const char c = *p;
                if (quoted) {
                    if (c != '"') { text.push_back(c); p++; }
                    else if (p + 1 < end && p[1] == '"') { text.push_back('"'); p += 2; }
                    else { quoted = false; p++; }
                } else if (c == '\t' || c == '\n' || c == '\r') break;
                else { text.push_back(c); p++; }
            }
            arena.push_back(std::move(text));
            field = arena.back();
        } else {
            const char* q = p;
            while (q < end && *q != '\t' && *q != '\n' && *q != '\r') q++;
            if (q > p) { field = std::string_view(p, size_t(q - p)); started = true; }
            p = q;
        }
        if (p >= end) break;
        if (*p == '\t') { rec.push_back(field); field = std::string_view(); started = true; p++; }
        else if (*p == '\n') { end_record(); p++; }
        else { if (p + 1 < end && p[1] == '\n') p++; end_record(); p++; }   // '\r' or "\r\n"
    }
    end_record();
}

// The same for a text without a quote and without a carriage return (what `somatic` writes): lines end at '\n', fields at '\t' - both
// found with memchr instead of a byte loop.
// A record of such a text = a non-empty line; counted first so that every part's rows get their place in the one row array.
size_t count_plain_records(const char* p, const char* const end) {
    size_t n = 0;
    while (p < end) {
        const char* nl = static_cast<const char*>(std::memchr(p, '\n', size_t(end - p)));
        const char* const le = nl ? nl : end;
        n += le > p;
        p = nl ? nl + 1 : end;
    }
    return n;
}
void parse_rows_plain(const char* p, const char* const end, size_t skip, Row* out, size_t n_out) {
    std::string_view rec[32];
    size_t k = 0;
    while (p < end) {
        const char* nl = static_cast<const char*>(std::memchr(p, '\n', size_t(end - p)));
        const char* const le = nl ? nl : end;
        if (le > p) {   // (an empty line is no record)
            size_t nf = 0;
            std::vector<std::string_view> many;   // a record with more fields than the fixed array holds (reported as malformed anyway)
            for (const char* q = p;;) {
                const char* tab = static_cast<const char*>(std::memchr(q, '\t', size_t(le - q)));
                const std::string_view f(q, size_t((tab ? tab : le) - q));
                if (nf < 32) rec[nf] = f; else { if (many.empty()) many.assign(rec, rec + 32); many.push_back(f); }
                nf++;
                if (!tab) break;
                q = tab + 1;
            }
            if (skip) skip--;
            else {
                if (k >= n_out) throw Error("internal error: TSV record count changed between the two passes");
                row_from_fields(many.empty() ? rec : many.data(), nf, out[k++]);
            }
        }
        p = nl ? nl + 1 : end;
    }
    if (k != n_out) throw Error("internal error: TSV record count changed between the two passes");
}

// Threads of the host legs, in order: the error of the earliest part is the one reported (what a sequential pass would have hit first).
template <class F> void run_parts(size_t n, F f) {
    std::vector<std::exception_ptr> errors(n);
    std::vector<std::thread> th;
    auto guarded = [&](size_t t) { try { f(t); } catch (...) { errors[t] = std::current_exception(); } };
    for (size_t t = 1; t < n; t++) th.emplace_back(guarded, t);
    guarded(0);
    for (auto& x : th) x.join();
    for (auto& e : errors) if (e) std::rethrow_exception(e);
}

// All rows of the TSV (first record = header). Without a quote anywhere in the text no field spans lines, so the text is cut at line
// breaks and the parts are parsed by all host threads; rows stay in file order.
void parse_tsv(std::string_view text, RowVec& rows, std::deque<std::string>& arena) {
    const char* const b = text.data();
    const char* const e = b + text.size();
    size_t parts = std::min<size_t>(host_threads(), text.size() / (4u << 20) + 1);
    // the threaded form needs records that are lines: no quote (a quoted field may hold a line break), no carriage return; and part 0
    // must hold the header (the first record that holds anything): a text that opens with a blank line is parsed in one piece
    if (parts > 1 && (*b == '\n' || std::memchr(b, '"', text.size()) != nullptr || std::memchr(b, '\r', text.size()) != nullptr)) parts = 1;
    if (parts <= 1) {
        size_t nl = 0;
        for (const char* q = b; (q = static_cast<const char*>(std::memchr(q, '\n', size_t(e - q)))) != nullptr; q++) nl++;
        rows.reserve(nl + 1);
        parse_rows(b, e, 1, rows, arena);
        return;
    }
    std::vector<const char*> cut(parts + 1, e);
    cut[0] = b;
    for (size_t t = 1; t < parts; t++) {
        const char* q = b + text.size() / parts * t;
        if (q < cut[t - 1]) q = cut[t - 1];
        const char* nl = static_cast<const char*>(std::memchr(q, '\n', size_t(e - q)));
        cut[t] = nl ? nl + 1 : e;
    }
    // pass 1: the parts' record counts -> every part's slice of the row array; pass 2: the rows, parsed in place
    std::vector<size_t> at(parts + 1, 0);
    run_parts(parts, [&](size_t t) { at[t + 1] = count_plain_records(cut[t], cut[t + 1]); });
    if (at[1] == 0) throw Error("internal error: TSV header not in the first part");
    at[1] -= 1;   // the header
    for (size_t t = 0; t < parts; t++) at[t + 1] += at[t];
    rows.resize(at[parts]);
    advise_huge(rows.data(), rows.size() * sizeof(Row));
    run_parts(parts, [&](size_t t) { parse_rows_plain(cut[t], cut[t + 1], t == 0 ? 1 : 0, rows.data() + at[t], at[t + 1] - at[t]); });
}

// FilteredRecord::FIELD_NAMES_AS_ARRAY (src/peptides.rs:21-47)
const char* const FILTERED_HEADER =
    "id\ttranscript\tgene_id\tgene_name\tchrom\toffset\tframe\tfreq\tcredible_interval\tdepth\tnvar\tnsomatic\tnvariant_sites\tnsomvariant_sites\t"
    "strand\tvariant_sites\tsomatic_positions\tsomatic_aa_change\tgermline_positions\tgermline_aa_change\tnormal_sequence\tmutant_sequence\t"
    "normal_peptide\ttumor_peptide\n";

// One filtered row (FilteredRecord, src/peptides.rs:21-47), formatted in place at the end of its stream (rowfmt.hpp cursor writers)
void write_filtered_record(TextBuf& t, const Row& r, double freq, std::string_view id, std::string_view ci, std::string_view normal_pep,
                           std::string_view tumor_pep) {
    const std::string_view text[] = {id, r.transcript, r.gene_id, r.gene_name, r.chrom, ci, r.strand, r.variant_sites, r.somatic_positions,
                                     r.somatic_aa_change, r.germline_positions, r.germline_aa_change, r.normal_sequence, r.mutant_sequence,
                                     normal_pep, tumor_pep};
    size_t bound = 7 * 21 + 33 + 1;
    for (std::string_view f : text) bound += field_bound(f);
    char* const b = t.room(bound);
    char* q = b;
    auto S = [&](std::string_view f) { q = cur_field(q, f); *q++ = '\t'; };
    auto U = [&](uint64_t v) { q = cur_u64(q, v); *q++ = '\t'; };
    S(id); S(r.transcript); S(r.gene_id); S(r.gene_name); S(r.chrom); U(r.offset); U(r.frame);
    q = cur_f64(q, freq); *q++ = '\t';
    S(ci); U(r.depth); U(r.nvar); U(r.nsomatic); U(r.nvariant_sites); U(r.nsomvariant_sites);
    S(r.strand); S(r.variant_sites); S(r.somatic_positions); S(r.somatic_aa_change); S(r.germline_positions); S(r.germline_aa_change);
    S(r.normal_sequence); S(r.mutant_sequence); S(normal_pep);
    q = cur_field(q, tumor_pep);
    *q++ = '\n';
    t.advance(size_t(q - b));
}

// The peptides already seen in the current (transcript, somatic_positions, germline_positions) run (seen_peptides, :262-400): a handful
// per run, so a flat list; a run that grows past it gets an ordered set.
struct SeenPeptides {
    std::vector<std::string_view> few;
    std::set<std::string_view> many;
    bool contains(std::string_view p) const {
        if (!many.empty()) return many.count(p) != 0;
        for (std::string_view q : few) if (q == p) return true;
        return false;
    }
    void insert(std::string_view p) {
        if (!many.empty()) { many.insert(p); return; }
        few.push_back(p);
        if (few.size() > 48) { many.insert(few.begin(), few.end()); few.clear(); }
    }
    void clear() { few.clear(); many.clear(); }
};

template <class V>
typename V::value_type* to_device(const V& v, hipStream_t stream, std::vector<void*>& owned, size_t pad = 0) {
    void* p = nullptr;
    using T = typename V::value_type;
    HIP_OK(hipMalloc(&p, v.size() * sizeof(T) + pad + 16));
    owned.push_back(p);
    if (!v.empty()) HIP_OK(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return static_cast<T*>(p);
}

// Wall times of the phases on stderr (MP_DEBUG)
struct Laps {
    bool dbg = std::getenv("MP_DEBUG") != nullptr;
    std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        const auto now = std::chrono::steady_clock::now();
        if (dbg) std::fprintf(stderr, "[mp]   filter: %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_prev).count());
        t_prev = now;
    }
};

// A stream on one device with the device memory of one step: everything is released when the step ends, whether it throws or not
struct DeviceStep {
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    std::vector<void*> owned;
    DeviceStep() {
        HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
    }
    ~DeviceStep() {
        for (void* p : owned) (void)hipFree(p);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        (void)hipStreamDestroy(stream);
    }
    template <class T> T* alloc(size_t bytes) {
        void* p = nullptr;
        HIP_OK(hipMalloc(&p, bytes));
        owned.push_back(p);
        return static_cast<T*>(p);
    }
};

// The reference peptidome - bincode v1 HashSet<Vec<u8>> (deserialize_from(...).unwrap(), :242) -> keys of the length-L members, of
// key_words(L) words each (pep.hpp)
void decode_reference(std::string_view reference_binary, uint32_t L, std::vector<uint64_t>& ref_keys) {
    const uint32_t w = key_words(L);
    size_t p = 0;
    auto u64 = [&]() {
        if (p + 8 > reference_binary.size())
            throw Error("reference would panic: called `Result::unwrap()` on an `Err` value (bincode: unexpected end of file)");
        uint64_t v = 0;
        for (int i = 0; i < 8; i++) v |= uint64_t(uint8_t(reference_binary[p + i])) << (8 * i);
        p += 8;
        return v;
    };
    const uint64_t n = u64();
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t l = u64();
        if (l > reference_binary.size() - p)
            throw Error("reference would panic: called `Result::unwrap()` on an `Err` value (bincode: unexpected end of file)");
        if (l == L) {  // only a member of the same length can equal a tumor peptide
            bool letters = true;
            for (uint64_t k = 0; k < l; k++) { const char c = reference_binary[p + k]; letters &= c >= 'A' && c <= 'Z'; }
            if (letters) push_key(ref_keys, peptide_to_key(reference_binary.data() + p, l), w);
        }
        p += l;
    }
}

// ---- the row stream (:262-563): which (row, i) peptides survive, and the groups they are scored in
struct Entry { uint32_t chunk; uint32_t row; uint32_t i1; uint32_t normal_len; uint64_t tumor_at; const uint8_t* normal_pep; uint64_t group; };
// records / frequencies / depth of the current region, by (frame, somatic_positions, germline_positions): the reference's BTreeMaps.
// A region holds a few keys; the slots keep their buffers from region to region and are put in key order when the region is flushed
struct Key {
    uint64_t frame; std::string_view som, germ;
    bool operator==(const Key& o) const { return frame == o.frame && som == o.som && germ == o.germ; }
    bool operator<(const Key& o) const { return std::tie(frame, som, germ) < std::tie(o.frame, o.som, o.germ); }
};
struct Pending { Key key; std::vector<double> alt; std::vector<uint32_t> depth; std::vector<Entry> recs; };

}  // namespace

struct FilterStream::State {
    uint32_t L, w;
    const std::vector<uint64_t>* reference_keys;
    std::vector<uint64_t> ref_keys;   // the decoded bincode members (unsorted; empty with reference_keys)
    std::string ref_error;            // a bincode image that does not decode: reported where the one-part filter reports it
    struct DevRef { int device; uint64_t* keys; uint64_t n; };   // the sorted distinct reference keys on one device
    std::vector<DevRef> dev_refs;
    // one part of the row stream: its rows (and what their views point into), their amino acids and K5's flags
    struct Chunk {
        RowCapture cap;                      // (a TSV's rows are in cap.rows; its quoted fields in `quoted`)
        std::deque<std::string> quoted;
        std::shared_ptr<const void> hold;
        PodVec<uint8_t> aa, flags;
        PodVec<uint64_t> aa_off;             // n_seq + 1 entries: sequence 2r mutant, 2r + 1 normal of row r
    };
    std::vector<std::unique_ptr<Chunk>> chunks;
    uint64_t n_rows = 0;
    float translate_ms = 0;
    // ---- the row stream's state, carried from one part to the next
    std::vector<Entry> entries;                 // in output order
    std::vector<uint64_t> grp_off{0};
    std::vector<uint8_t> grp_final;
    std::vector<double> g_alt;
    std::vector<uint32_t> g_depth;
    std::vector<Pending> slots;
    size_t n_used = 0;
    std::map<Key, size_t> slot_index;           // only for a region with more keys than a scan should look through
    static constexpr size_t SCAN_LIMIT = 12;
    std::vector<size_t> order;
    // `current` (transcript, somatic_positions, germline_positions) and `region_sites` (transcript, variant_sites) of the reference are
    // kept as the row that last set them; both start as tuples of empty strings
    const Row* current = &empty_row();
    const Row* region = &empty_row();
    SeenPeptides seen_peptides;
    // stop_gained: (transcript, frame) -> offset of the stop-gain row. Rows come in runs of one (transcript, frame), so the entry
    // of the previous row is remembered.
    std::map<std::pair<std::string_view, uint64_t>, size_t> stop_gained;
    const Row* sg_row = nullptr;                // the row the remembered look-up was made for
    size_t* sg_at = nullptr;                    // its entry (nullptr: none)

    static const Row& empty_row() { static const Row r{}; return r; }

    ~State() { free_references(); }

    void free_references() {
        if (dev_refs.empty()) return;   // (a stream that never reached a device makes no HIP call)
        int cur = -1;
        const bool restore = hipGetDevice(&cur) == hipSuccess;
        for (const DevRef& r : dev_refs)
            if (r.keys && hipSetDevice(r.device) == hipSuccess) (void)hipFree(r.keys);
        if (restore) (void)hipSetDevice(cur);
        dev_refs.clear();
    }

    // What every add and finish does first: the device, and the reference (its decoding error, if any)
    void begin(int device) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
            throw Error("no HIP device available: `filter` translates and scores on the GPU, there is no CPU fallback");
        HIP_OK(hipSetDevice(device));
        if (!ref_error.empty()) throw Error(ref_error);
    }

    // The sorted distinct reference keys on `device`: uploaded (and, decoded from bincode, radix-sorted + de-duplicated) on first use
    const DevRef& reference_on(int device) {
        for (const DevRef& r : dev_refs) if (r.device == device) return r;
        DevRef r{device, nullptr, 0};
        DeviceStep st;
        if (reference_keys) {
            r.n = reference_keys->size() / w;
            if (r.n) {
                r.keys = to_device(*reference_keys, st.stream, st.owned);
                st.owned.pop_back();   // (kept: freed by ~State)
            }
        } else if (!ref_keys.empty()) {
            uint64_t* d_in = to_device(ref_keys, st.stream, st.owned);
            uint64_t* d_tmp = st.alloc<uint64_t>(ref_keys.size() * 8);
            void* d_out = nullptr;
            HIP_OK(hipMalloc(&d_out, ref_keys.size() * 8));
            r.keys = static_cast<uint64_t*>(d_out);
            try { r.n = device_sort_unique(d_in, d_tmp, r.keys, ref_keys.size() / w, L, st.stream); }
            catch (...) { (void)hipFree(d_out); throw; }
        }
        try { HIP_OK(hipStreamSynchronize(st.stream)); }
        catch (...) { if (r.keys) (void)hipFree(r.keys); throw; }
        dev_refs.push_back(r);
        return dev_refs.back();
    }

    // K5 over the rows of chunk c on `device`, in two steps supplied by its source: offsets(stream, owned) fills c.aa_off and returns it on
    // the device; launch(stream, d_aa_off, d_ref, n_ref, d_aa, d_flags, d_err) enqueues the translation. Returns K5's error word.
    template <class Offsets, class Launch>
    uint32_t translate(int device, Chunk& c, Offsets offsets, Launch launch) {
        const DevRef& ref = reference_on(device);
        DeviceStep st;
        const uint64_t* d_aa_off = offsets(st.stream, st.owned);
        const uint64_t n_aa = c.aa_off[c.cap.rows.size() * 2];
        uint8_t* d_aa = st.alloc<uint8_t>(n_aa + 16);
        uint8_t* d_flags = st.alloc<uint8_t>(n_aa + 16);
        uint32_t* d_err = st.alloc<uint32_t>(4);
        HIP_OK(hipMemsetAsync(d_err, 0, 4, st.stream));
        HIP_OK(hipMemsetAsync(d_flags, 0, n_aa + 16, st.stream));
        HIP_OK(hipEventRecord(st.e0, st.stream));
        launch(st.stream, d_aa_off, ref.keys, ref.n, d_aa, d_flags, d_err);
        HIP_OK(hipEventRecord(st.e1, st.stream));
        c.aa.resize(n_aa);
        c.flags.resize(n_aa);
        uint32_t err = 0;
        if (n_aa) {
            HIP_OK(hipMemcpyAsync(c.aa.data(), d_aa, n_aa, hipMemcpyDeviceToHost, st.stream));
            HIP_OK(hipMemcpyAsync(c.flags.data(), d_flags, n_aa, hipMemcpyDeviceToHost, st.stream));
        }
        HIP_OK(hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, st.stream));
        HIP_OK(hipStreamSynchronize(st.stream));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, st.e0, st.e1));
        translate_ms += ms;
        return err;
    }

    Pending* find_slot(const Key& k) {
        if (n_used > SCAN_LIMIT) {
            auto it = slot_index.find(k);
            return it == slot_index.end() ? nullptr : &slots[it->second];
        }
        for (size_t i = 0; i < n_used; i++) if (slots[i].key == k) return &slots[i];
        return nullptr;
    }
    Pending& add_slot(const Key& k) {
        if (n_used == slots.size()) slots.emplace_back();
        Pending& p = slots[n_used];
        p.key = k; p.alt.clear(); p.depth.clear(); p.recs.clear();
        n_used++;
        if (n_used == SCAN_LIMIT + 1) for (size_t i = 0; i + 1 < n_used; i++) slot_index[slots[i].key] = i;
        if (n_used > SCAN_LIMIT) slot_index[k] = n_used - 1;
        return p;
    }
    void flush(bool final_pass) {
        order.resize(n_used);
        for (size_t i = 0; i < n_used; i++) order[i] = i;
        if (n_used > 1) std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return slots[a].key < slots[b].key; });
        for (size_t i : order) {
            Pending& p = slots[i];
            const uint64_t g = grp_final.size();
            grp_final.push_back(final_pass ? 1 : 0);
            g_alt.insert(g_alt.end(), p.alt.begin(), p.alt.end());
            g_depth.insert(g_depth.end(), p.depth.begin(), p.depth.end());
            grp_off.push_back(g_alt.size());
            for (Entry& e : p.recs) { e.group = g; entries.push_back(e); }
        }
        n_used = 0;
        slot_index.clear();
    }

    // The row stream over the rows of chunk ci (translated; err: K5's error word), continuing where the previous chunk left it
    void advance(uint32_t ci, uint32_t err) {
        const Chunk& c = *chunks[ci];
        const RowVec& rows = c.cap.rows;
        const PodVec<uint64_t>& aa_off = c.aa_off;
        n_rows += rows.size();
        if (entries.capacity() < entries.size() + rows.size())   // (geometric: a stream of many small parts must not copy them all each time)
            entries.reserve(std::max(2 * entries.capacity(), entries.size() + rows.size()));
        // the hot members as locals, stored back after the last row: the loop's stores through vectors would otherwise make the compiler
        // load them again for every peptide
        const uint32_t L = this->L;
        const Row* current = this->current;
        const Row* region = this->region;
        const Row* sg_row = this->sg_row;
        size_t* sg_at = this->sg_at;
        for (size_t r = 0; r < rows.size(); r++) {
            const Row& row = rows[r];
            if (row.mutant_sequence.size() < 2 || (!row.normal_sequence.empty() && row.normal_sequence.size() < 2))  // `r.len() - 2` (:139)
                throw Error("reference would panic: attempt to subtract with overflow (to_protein)");
            size_t som_pos = 0;
            if (!row.somatic_positions.empty() && row.somatic_positions.find('|') == std::string_view::npos) {
                uint64_t v = 0;
                const auto pr = std::from_chars(row.somatic_positions.data(), row.somatic_positions.data() + row.somatic_positions.size(), v);
                if (pr.ec != std::errc() || pr.ptr != row.somatic_positions.data() + row.somatic_positions.size())
                    throw Error("reference would panic: called `Result::unwrap()` on an `Err` value (somatic_positions)");
                som_pos = size_t(v);
            }
            const size_t offset = size_t(row.offset);
            const uint8_t* tp = c.aa.data() + aa_off[2 * r];
            const size_t tlen = size_t(aa_off[2 * r + 1] - aa_off[2 * r]);
            const uint8_t* np = c.aa.data() + aa_off[2 * r + 1];
            const size_t nlen = size_t(aa_off[2 * r + 2] - aa_off[2 * r + 1]);
            if (err & 1)   // some codon held a base other than A, C, G, T: find the first row it is in
                for (size_t k = 0; k < tlen + nlen; k++)
                    if ((k < tlen ? tp[k] : np[k - tlen]) == '?')
                        throw Error("reference would panic: called `Result::unwrap()` on an `Err` value (codon with a base other than A, C, G, T)");
            const bool fwd = row.strand == "Forward", rvs = row.strand == "Reverse";
            if (!(sg_row && sg_row->frame == row.frame && sg_row->transcript == row.transcript)) {
                auto sg = stop_gained.find({row.transcript, row.frame});
                sg_at = sg == stop_gained.end() ? nullptr : &sg->second;
            }
            sg_row = &row;
            if (sg_at) {  // :304-317
                const bool downstream = fwd ? offset > *sg_at : rvs ? offset < *sg_at : false;
                if (downstream) continue;
            }
            bool has_x = false;
            for (size_t k = 0; k < tlen; k++) has_x |= tp[k] == 'X';
            if (has_x && (std::fabs(row.freq - 1.0) < std::numeric_limits<double>::epsilon() || row.frame > 0)) {
                if (sg_at) *sg_at = offset;
                else sg_at = &(stop_gained[{row.transcript, row.frame}] = offset);
            }
            const uint8_t* tf = c.flags.data() + aa_off[2 * r];
            size_t i = 0;
            while (i + L <= tlen) {
                if (tf[i] & 1) break;  // the peptide contains a stop (:330-332)
                const bool normal_full = nlen >= i + L;
                const size_t nl = normal_full ? L : nlen;
                const uint8_t* npep = normal_full ? np + i : np;
                if (nl == 0 && som_pos > 0) {  // :343-360
                    if (fwd) {
                        if ((i + L) * 3 + offset <= som_pos) { i += 1; continue; }
                    } else if (rvs) {
                        if ((tlen - (i + L)) * 3 + offset > som_pos) { i += 1; continue; }
                    }
                }
                const size_t i0 = i;
                i += 1;
                if (nl == L && std::equal(tp + i0, tp + i0 + L, npep)) continue;  // self-similar (:363-365)
                const std::string_view tumor_pep(reinterpret_cast<const char*>(tp + i0), L);
                if (row.transcript == current->transcript && row.somatic_positions == current->somatic_positions &&
                    row.germline_positions == current->germline_positions) {
                    if (seen_peptides.contains(tumor_pep)) continue;
                } else {
                    current = &row;
                    seen_peptides.clear();
                }
                seen_peptides.insert(tumor_pep);
                const Entry e{ci, uint32_t(r), uint32_t(i), uint32_t(nl), aa_off[2 * r] + i0, npep, 0};
                const Key key{row.frame, row.somatic_positions, row.germline_positions};
                const double alt = row.freq * double(row.depth);
                if (row.transcript != region->transcript || row.variant_sites != region->variant_sites) {  // :398-541
                    flush(false);
                    Pending& p = add_slot(key);
                    p.alt.push_back(alt); p.depth.push_back(row.depth); p.recs.push_back(e);
                    region = &row;
                } else {
                    // entry(key).or_insert_with(|| vec![x]).push(x): a key first seen here holds its first value twice (:548-560)
                    Pending* p = find_slot(key);
                    if (!p) { p = &add_slot(key); p->alt.push_back(alt); p->depth.push_back(row.depth); p->recs.push_back(e); }
                    p->alt.push_back(alt); p->depth.push_back(row.depth); p->recs.push_back(e);
                }
            }
        }
        this->current = current;
        this->region = region;
        this->sg_row = sg_row;
        this->sg_at = sg_at;
    }

    // The last region (:541), K6 on `device`, and the emission (:483-533, :662-706)
    void finish(int device, FilterResult& out) {
        Laps lap;
        begin(device);
        out = FilterResult();
        const size_t threads = host_threads();
        flush(true);
        lap("row stream: last region");
        out.n_rows = n_rows;
        out.translate_ms = translate_ms;
        out.n_peptides = entries.size();
        out.n_groups = grp_final.size();

        // ---- K6
        std::vector<CredibleInterval> ci(grp_final.size());
        if (!grp_final.empty()) {
            std::vector<double> ln_fact(171);
            {
                double f = 1.0;   // statrs FCACHE: f64 factorials by repeated multiplication, then .ln()
                ln_fact[0] = std::log(1.0);
                for (int k = 1; k < 171; k++) { f *= double(k); ln_fact[k] = std::log(f); }
            }
            DeviceStep st;
            uint64_t* d_goff = to_device(grp_off, st.stream, st.owned);
            uint8_t* d_gfin = to_device(grp_final, st.stream, st.owned);
            double* d_alt = to_device(g_alt, st.stream, st.owned);
            uint32_t* d_dep = to_device(g_depth, st.stream, st.owned);
            double* d_lf = to_device(ln_fact, st.stream, st.owned);
            CredibleInterval* d_ci = st.alloc<CredibleInterval>(ci.size() * sizeof(CredibleInterval));
            HIP_OK(hipEventRecord(st.e0, st.stream));
            device_credible_intervals(d_goff, d_gfin, d_alt, d_dep, ci.size(), d_lf, d_ci, st.stream);
            HIP_OK(hipEventRecord(st.e1, st.stream));
            HIP_OK(hipMemcpyAsync(ci.data(), d_ci, ci.size() * sizeof(CredibleInterval), hipMemcpyDeviceToHost, st.stream));
            HIP_OK(hipStreamSynchronize(st.stream));
            HIP_OK(hipEventElapsedTime(&out.stats_ms, st.e0, st.e1));
        }
        lap("K6 credible intervals");

        // ---- emission: the entries in order, written by all host threads (entry ranges) and joined
        for (const Entry& e : entries)
            if (ci[e.group].status) throw Error("reference would panic: called `Option::unwrap()` on a `None` value (partial_cmp of a NaN likelihood)");
        struct Streams { TextBuf tsv, removed_tsv, fasta, normal_fasta, removed_fasta; uint64_t kept = 0, removed = 0; };
        const size_t parts = std::max<size_t>(1, std::min<size_t>(threads, entries.size() / 2048 + 1));
        std::vector<Streams> part(parts);
        run_parts(parts, [&](size_t t) {
            Streams& o = part[t];
            const size_t lo = entries.size() * t / parts, hi = entries.size() * (t + 1) / parts;
            o.tsv.reserve((hi - lo) * 320);
            std::string id;
            const Chunk* cp = nullptr;
            uint32_t c_at = 0xFFFFFFFFu;
            for (size_t k = lo; k < hi; k++) {
                const Entry& e = entries[k];
                if (e.chunk != c_at) { c_at = e.chunk; cp = chunks[c_at].get(); }   // (entries come chunk by chunk)
                const Chunk& c = *cp;
                const Row& row = c.cap.rows[e.row];
                const CredibleInterval& g = ci[e.group];
                char buf[64];
                std::snprintf(buf, sizeof buf, "%.2f-%.2f", g.a, g.b);
                id.clear();
                append_u64(id, e.i1);
                id.push_back('_');
                id.append(row.id.data(), row.id.size());
                const double freq = row.depth == 0 ? 0.0 : double(g.ml) * 0.01;
                const uint8_t* tumor = c.aa.data() + e.tumor_at;
                const std::string_view tumor_pep(reinterpret_cast<const char*>(tumor), L);
                const std::string_view normal_pep(reinterpret_cast<const char*>(e.normal_pep), e.normal_len);
                if (c.flags[e.tumor_at] & 2) {
                    put_fasta(o.removed_fasta, id, tumor, L);
                    write_filtered_record(o.removed_tsv, row, freq, id, buf, normal_pep, tumor_pep);
                    o.removed++;
                } else {
                    put_fasta(o.fasta, id, tumor, L);
                    if (e.normal_len) put_fasta(o.normal_fasta, id, e.normal_pep, e.normal_len);
                    write_filtered_record(o.tsv, row, freq, id, buf, normal_pep, tumor_pep);
                    o.kept++;
                }
            }
        });
        for (const Streams& o : part) { out.n_kept += o.kept; out.n_removed += o.removed; }
        const std::string_view header(FILTERED_HEADER);
        auto join = [&](PodVec<char>& dst, TextBuf Streams::*m, bool with_header) {
            std::vector<size_t> at(parts + 1, with_header ? header.size() : 0);
            for (size_t t = 0; t < parts; t++) at[t + 1] = at[t] + (part[t].*m).size();
            dst.resize(at[parts]);
            advise_huge(dst.data(), dst.size());
            if (with_header) std::memcpy(dst.data(), header.data(), header.size());
            run_parts(parts, [&](size_t t) {
                TextBuf& src = part[t].*m;
                if (!src.empty()) std::memcpy(dst.data() + at[t], src.data(), src.size());
                src = TextBuf();
            });
        };
        join(out.tsv, &Streams::tsv, true);
        join(out.removed_tsv, &Streams::removed_tsv, out.n_removed > 0);   // its header is written with its first record
        join(out.fasta, &Streams::fasta, false);
        join(out.normal_fasta, &Streams::normal_fasta, false);
        join(out.removed_fasta, &Streams::removed_fasta, false);
        lap("emission");
        // Nothing is read any more. The row stream's own state and the reference keys go first, here (as the one-call filter freed its
        // locals); then the parts' rows and downloaded records go to the reaper thread - unmapped while this thread unmaps too, they
        // would contend for the same lock
        std::vector<Entry>().swap(entries);
        std::vector<Pending>().swap(slots);
        std::vector<double>().swap(g_alt);
        std::vector<uint32_t>().swap(g_depth);
        std::vector<uint64_t>().swap(grp_off);
        std::vector<uint8_t>().swap(grp_final);
        stop_gained.clear();
        seen_peptides.clear();
        free_references();
        release_later(std::move(chunks));
    }
};

FilterStream::FilterStream(std::string_view reference_binary, const std::vector<uint64_t>* reference_keys, uint32_t L) : s(new State()) {
    check_peptide_len(L);
    s->L = L;
    s->w = key_words(L);
    s->reference_keys = reference_keys;
    if (!reference_keys) {
        try { decode_reference(reference_binary, L, s->ref_keys); }
        catch (const std::exception& e) { s->ref_error = e.what(); s->ref_keys.clear(); }
    }
}

FilterStream::~FilterStream() = default;

void FilterStream::add_captured(int device, RowCapture&& cap, const RecArena& arena, std::shared_ptr<const void> hold) {
    Laps lap;
    s->begin(device);
    // every sequence must lie inside what it names: K5 reads [off, off + len) of a record's half, or [at, at + len) of the side buffer
    const size_t n_seq = cap.rows.size() * 2;
    if (cap.seq.size() != n_seq) throw Error("internal error: captured rows and sequences disagree");
    for (const RowSeq& rs : cap.seq) {
        const bool ok = (rs.flags & SRC_MERGE) ? (rs.at <= cap.side.size() && rs.len <= cap.side.size() - rs.at)
                                               : (rs.len == 0 || (rs.at < arena.n_slots && uint64_t(rs.off) + rs.len <= arena.seq_cap));
        if (!ok) throw Error("internal error: captured sequence outside the record arena");
    }
    if (n_seq && !arena.recs) throw Error("internal error: no device record arena");
    std::unique_ptr<State::Chunk> c(new State::Chunk());
    c->cap = std::move(cap);
    c->hold = std::move(hold);
    c->aa_off.resize(n_seq + 1);
    c->aa_off[0] = 0;
    lap("captured rows checked");
    const RowSeq* d_seq = nullptr;
    const uint8_t* d_side = nullptr;
    State::Chunk& C = *c;
    const uint32_t err = s->translate(device, C,
        [&](hipStream_t stream, std::vector<void*>& owned) -> const uint64_t* {
            d_seq = to_device(C.cap.seq, stream, owned);
            d_side = to_device(C.cap.side, stream, owned);
            uint64_t* d_aa_off = nullptr;
            HIP_OK(hipMalloc(&d_aa_off, (n_seq + 1) * 8)); owned.push_back(d_aa_off);
            device_row_codon_offsets(d_seq, n_seq, d_aa_off, stream);
            HIP_OK(hipMemcpyAsync(C.aa_off.data(), d_aa_off, (n_seq + 1) * 8, hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            return d_aa_off;
        },
        [&](hipStream_t stream, const uint64_t* d_aa_off, const uint64_t* d_ref, uint64_t n_ref, uint8_t* d_aa, uint8_t* d_flags, uint32_t* d_err) {
            device_translate_row_sources(d_seq, n_seq, arena.recs, arena.rec_stride, arena.seq_cap, d_side, d_aa_off, s->L, d_ref, n_ref, d_aa,
                                         d_flags, d_err, stream);
        });
    lap("reference + K5 + copies");
    s->chunks.push_back(std::move(c));
    s->advance(uint32_t(s->chunks.size() - 1), err);
    lap("row stream");
}

void FilterStream::add_text(int device, std::string_view tsv_text) {
    Laps lap;
    s->begin(device);
    std::unique_ptr<State::Chunk> c(new State::Chunk());
    // ---- rows and their two nucleotide windows, laid out back to back for the upload
    RowVec& rows = c->cap.rows;
    parse_tsv(tsv_text, rows, c->quoted);
    lap("tsv parsed");
    const size_t n_seq = rows.size() * 2;   // 2r = mutant, 2r + 1 = normal
    PodVec<uint8_t> nt, rev(n_seq);
    PodVec<uint64_t> nt_off(n_seq);
    PodVec<uint64_t>& aa_off = c->aa_off;
    aa_off.resize(n_seq + 1);
    PodVec<uint32_t> nt_len(n_seq);
    aa_off[0] = 0;
    {
        uint64_t at = 0;
        for (size_t r = 0; r < rows.size(); r++) {
            const uint8_t rv = (!rows[r].id.empty() && rows[r].id.back() == 'F') ? 0 : 1;  // :291-294
            const std::string_view seqs[2] = {rows[r].mutant_sequence, rows[r].normal_sequence};
            for (int k = 0; k < 2; k++) {
                const size_t q = 2 * r + k;
                if (seqs[k].size() > 0xFFFFFFFFull) throw Error("sequence too long");
                nt_off[q] = at;
                nt_len[q] = uint32_t(seqs[k].size());
                rev[q] = rv;
                at += seqs[k].size();
                aa_off[q + 1] = aa_off[q] + (seqs[k].size() > 2 ? (seqs[k].size() - 2 + 2) / 3 : 0);
            }
        }
        nt.resize(at);
        advise_huge(nt.data(), nt.size());
        const size_t parts = std::min<size_t>(host_threads(), rows.size() / 65536 + 1);
        run_parts(parts, [&](size_t t) {
            for (size_t r = rows.size() * t / parts, e = rows.size() * (t + 1) / parts; r < e; r++) {
                if (nt_len[2 * r]) std::memcpy(nt.data() + nt_off[2 * r], rows[r].mutant_sequence.data(), nt_len[2 * r]);
                if (nt_len[2 * r + 1]) std::memcpy(nt.data() + nt_off[2 * r + 1], rows[r].normal_sequence.data(), nt_len[2 * r + 1]);
            }
        });
    }
    lap("windows laid out");
    const uint8_t* d_nt = nullptr;
    const uint64_t* d_nt_off = nullptr;
    const uint32_t* d_nt_len = nullptr;
    const uint8_t* d_rev = nullptr;
    const uint32_t err = s->translate(device, *c,
        [&](hipStream_t stream, std::vector<void*>& owned) -> const uint64_t* {
            d_nt = to_device(nt, stream, owned, 64);
            d_nt_off = to_device(nt_off, stream, owned);
            d_nt_len = to_device(nt_len, stream, owned);
            d_rev = to_device(rev, stream, owned);
            return to_device(aa_off, stream, owned);
        },
        [&](hipStream_t stream, const uint64_t* d_aa_off, const uint64_t* d_ref, uint64_t n_ref, uint8_t* d_aa, uint8_t* d_flags, uint32_t* d_err) {
            device_translate_records(d_nt, d_nt_off, d_nt_len, d_rev, d_aa_off, n_seq, s->L, d_ref, n_ref, d_aa, d_flags, d_err, stream);
        });
    lap("reference + K5 + copies");
    s->chunks.push_back(std::move(c));
    s->advance(uint32_t(s->chunks.size() - 1), err);
    lap("row stream");
}

void FilterStream::finish(int device, FilterResult& out) { s->finish(device, out); }

void filter_device(int device, std::string_view reference_binary, const std::vector<uint64_t>* reference_keys, std::string_view tsv_text,
                   uint32_t L, FilterResult& out) {
    FilterStream stream(reference_binary, reference_keys, L);
    stream.add_text(device, tsv_text);
    stream.finish(device, out);
}

}  // namespace mp
