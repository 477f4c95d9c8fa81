// Consumer entry point, see consume.cpp.
#pragma once
#include "batch.hpp"
#include "device.hpp"
#include "filter.hpp"
#include "pep.hpp"

namespace mp {

// Walk every planned transcript of the batch and emit FASTA / normal FASTA / TSV exactly as
// microphasing::phase_gene would (reference: src/microphasing.rs:882-1941), answering every
// print_haplotypes call from the device results. streams: STREAM_* mask (model.hpp) - the text of a stream that is not asked for is
// not produced (it stays empty, and its per-gene offsets stay 0). rows != nullptr: also every row of the TSV stream (whether or not
// its text is asked for), in TSV order, as FilterStream::add_captured takes them; their sequence views point into res, their gene and
// transcript text into the gene model (for a deep gene: the batch's copies, b.split_inputs), which must outlive them.
void consume_batch(const Batch& b, const HostResults& res, PhasedStreams& out, uint32_t streams = STREAM_ALL, RowCapture* rows = nullptr);

// The same for `microphaser normal` (reference: src/normal_microphasing.rs:650-1279); the batch must have been planned
// with normal = true. sources != nullptr: also one PepSource per record of the FASTA stream (whether or not its text is asked for),
// in gene order - what peptidome_from_sources translates.
void consume_batch_normal(const Batch& b, const HostResults& res, PhasedStreams& out, uint32_t streams = STREAM_ALL, PepSources* sources = nullptr);

}  // namespace mp
