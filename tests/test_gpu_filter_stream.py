"""The filter stream (mp_filter_stream_* / FilterStream / pipeline.filter_chunked): `somatic` batches of gene chunks, added one at a
time on one or two contexts, end in byte for byte the five streams, the counts and the errors of Batch.filter on one batch of all
the added genes - and of the text filter on the chunks' TSVs concatenated (header once)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, SOMATIC_FIXTURES

pytestmark = pytest.mark.gpu

REF_BIN = os.path.join(GOLDEN, "test_filter", "reference.binary")


@pytest.fixture(scope="module")
def ctx(built):
    import microphaser_amd as m
    return m.Context(0)


@pytest.fixture(scope="module")
def ctx2(built):
    import microphaser_amd as m
    return m.Context(0)   # a second context of the same device: what a second GPU would be to the stream


def streams(f):
    return (f.fasta, f.normal_fasta, f.tsv, f.removed_tsv, f.removed_fasta)


def counts(f):
    return (f.rows, f.peptides, f.groups, f.kept, f.removed)


def outcome(call):
    """("ok", streams, counts) of a filter call, or ("error", message)."""
    import microphaser_amd as m
    try:
        f = call()
    except m.MicrophaserError as e:
        return ("error", str(e))
    return ("ok", streams(f), counts(f))


def batch_on(c, ds, genes, w):
    """A `somatic` batch of ds's genes (ascending ordinals) created on context c (which need not be the data set's)."""
    import microphaser_amd as m
    genes = list(genes)
    arr = (ctypes.c_uint32 * max(1, len(genes)))(*genes)
    h = ctypes.c_void_p()
    c._check(m.lib().mp_batch_create_genes(c._h, ds._h, m.MODE_SOMATIC, w, arr, len(genes), ctypes.byref(h)))
    return m.Batch(c, h, ds)


def one_batch(ds, genes, reference, L, w):
    """Batch.filter of one batch of `genes` (outcome) and that batch's TSV (None if the run failed)."""
    import microphaser_amd as m
    b = batch_on(ds.ctx, ds, genes, w)
    try:
        b.run()
        tsv = b.results(m.STREAM_TSV).tsv
    except m.MicrophaserError as e:
        return ("error", str(e)), None
    got = outcome(lambda: b.filter(reference, L)[0])
    b.close()
    return got, tsv


def streamed(ds, chunks, reference, L, w, contexts, check_results=False):
    """The chunks (lists of gene ordinals) added to one FilterStream, chunk i on contexts[i % len]; each batch is freed right after its
    add. Returns (outcome of the whole stream, the chunks' TSVs). check_results: every add's Results of STREAM_TSV | STREAM_NORMAL_FASTA
    equal that batch's own results()."""
    import microphaser_amd as m
    want = m.STREAM_TSV | m.STREAM_NORMAL_FASTA
    fs = m.FilterStream(contexts[0], reference, L)
    tsvs = []
    try:
        for i, genes in enumerate(chunks):
            b = batch_on(contexts[i % len(contexts)], ds, genes, w)
            b.run()
            r = fs.add(b, want)
            if check_results:
                own = b.results(want)
                assert (r.tsv, r.normal_fasta, r.fasta) == (own.tsv, own.normal_fasta, b"")
            tsvs.append(r.tsv)
            b.close()
    except m.MicrophaserError as e:
        return ("error", str(e)), tsvs
    got = outcome(lambda: fs.finish(contexts[-1]))
    fs.close()
    return got, tsvs


def concat_tsvs(tsvs):
    """The chunks' info.tsv texts as one file: the header once."""
    body = [t.split(b"\n", 1)[1] if t else b"" for t in tsvs]
    head = next((t.split(b"\n", 1)[0] + b"\n" for t in tsvs if t), b"")
    return head + b"".join(body)


def ranges_to_chunks(ranges):
    return [list(range(lo, hi)) for lo, hi in ranges]


@pytest.fixture(scope="module")
def exome(ctx):
    """synth(303, 30) with indels and its own normal peptidome, at (9, 27) and (15, 45)."""
    import microphaser_amd as m
    ds = ctx.synth(303, 30, indel_rate=0.03)
    peps = {}
    for L, w in ((9, 27), (15, 45)):
        peps[L] = ctx.build_reference(ds.phase(window_len=w, mode=m.MODE_NORMAL).fasta, L)
    return ds, peps


@pytest.mark.parametrize("kind", ["peptides", "bincode"])
@pytest.mark.parametrize("L,w", [(9, 27), (15, 45)])
def test_chunked_stream_equals_one_batch_and_the_text_filter(ctx, ctx2, exome, L, w, kind):
    from microphaser_amd.pipeline import cost_ranges
    ds, peps = exome
    reference = peps[L] if kind == "peptides" else peps[L].binary
    n = ds.num_genes
    want, tsv = one_batch(ds, range(n), reference, L, w)
    assert want[0] == "ok" and want[2][3] > 0 and want[2][4] > 0, want[:1]
    assert outcome(lambda: ctx.filter(tsv, reference, L)) == want
    costs = ds.gene_costs()
    chunkings = [ranges_to_chunks(cost_ranges(costs, k)) for k in (1, 2, 5)] + [[[g] for g in range(n)]]
    assert len(chunkings[0]) == 1 and len(chunkings[1]) == 2 and len(chunkings[2]) >= 4 and len(chunkings[3]) == n
    for chunks in chunkings:
        for contexts in ([ctx], [ctx, ctx2]):
            got, tsvs = streamed(ds, chunks, reference, L, w, contexts, check_results=chunks is chunkings[2])
            assert got == want, (len(chunks), len(contexts))
            assert concat_tsvs(tsvs) == tsv
            assert outcome(lambda: ctx.filter(concat_tsvs(tsvs), reference, L)) == want


def test_chunks_with_skipped_genes(ctx, ctx2, exome):
    """Gaps between the chunks' genes and inside them: the stream equals one batch of the genes it was given."""
    ds, peps = exome
    L, w = 9, 27
    chunks = [[0, 1, 3], [4, 5, 6, 9], [14], [15, 17, 18, 19, 20], [26, 29]]
    genes = [g for c in chunks for g in c]
    for reference in (peps[L], peps[L].binary):
        want, tsv = one_batch(ds, genes, reference, L, w)
        assert want[0] == "ok" and want[2][0] > 0
        for contexts in ([ctx], [ctx2, ctx]):
            got, tsvs = streamed(ds, chunks, reference, L, w, contexts)
            assert got == want
            assert concat_tsvs(tsvs) == tsv


def test_a_chunk_without_rows_and_a_stream_without_adds(ctx):
    """A batch whose run writes no row (the forward fixture against an empty VCF), and a stream finished without any add: the text
    filter of an empty TSV."""
    import microphaser_amd as m
    d, bam, _vcf, gtf, fa, _stem = SOMATIC_FIXTURES["test_forward"]
    base = os.path.join(GOLDEN, d)
    ds = ctx.load(os.path.join(base, bam), os.path.join(GOLDEN, "test_empty", "empty_test.vcf"), os.path.join(base, fa),
                  os.path.join(base, gtf))
    for reference in (open(REF_BIN, "rb").read(), ctx.peptides_union([], 9)):
        want = outcome(lambda: ctx.filter(b"", reference, 9))
        assert want[0] == "ok" and want[2][0] == 0 and want[1][2].startswith(b"id\ttranscript")
        fs = m.FilterStream(ctx, reference, 9)
        assert outcome(fs.finish) == want
        got, tsvs = streamed(ds, [list(range(ds.num_genes))], reference, 9, 27, [ctx])
        assert tsvs == [b""]
        assert got == want
        b = ds.batch(window_len=27)
        b.run()
        assert outcome(lambda: b.filter(reference, 9)[0]) == want


def test_a_stream_without_adds_reports_a_broken_reference_at_finish(ctx):
    """The bincode image is decoded once, at create; its error comes where the one-batch filter reports it: here, at finish."""
    import microphaser_amd as m
    broken = open(REF_BIN, "rb").read()[:-3]
    want = outcome(lambda: ctx.filter(b"", broken, 9))
    assert want[0] == "error" and "unexpected end of file" in want[1]
    fs = m.FilterStream(ctx, broken, 9)
    assert outcome(fs.finish) == want


def _normal_peptidome(ctx, ds, w, L):
    """build_reference of the `normal` FASTA of ds, gene by gene (genes the reference would panic on, and records with a base outside
    ACGT, left out)."""
    import microphaser_amd as m
    fas = []
    for g in range(ds.num_genes):
        try:
            b = ds.batch(window_len=w, gene_lo=g, gene_hi=g + 1, mode=m.MODE_NORMAL)
            b.run()
            fas.append(b.results(m.STREAM_FASTA).fasta)
        except m.MicrophaserError as e:
            assert str(e).startswith("reference would panic"), str(e)
    lines = b"".join(fas).split(b"\n")
    keep = [(i, s) for i, s in zip(lines[0:-1:2], lines[1::2]) if not s.upper().translate(None, b"ACGT")]
    return ctx.peptidome(b"".join(i + b"\n" + s + b"\n" for i, s in keep), L)


def test_genes_split_into_read_subsets_in_chunks(ctx, ctx2, monkeypatch):
    """MP_TEST_ROW_SLOTS=24 plans nearly every gene as 2..3 copies with disjoint read subsets; the captured rows of those genes view the
    batch's copies, which the stream keeps after the batch is freed."""
    from microphaser_amd.pipeline import cost_ranges
    ds = ctx.synth(1717, 40, indel_rate=0.08, multiallelic_rate=0.05, softmask_rate=0.2, mate_rate=0.3)
    planned_tx = lambda: batch_on(ctx, ds, range(ds.num_genes), 27).run().n_transcripts   # (a read-subset copy plans its transcripts again)
    unsplit = planned_tx()
    monkeypatch.setenv("MP_TEST_ROW_SLOTS", "24")
    assert planned_tx() > unsplit   # genes are split
    pep = _normal_peptidome(ctx, ds, 27, 9)
    # the genes the reference does not panic on, as one batch and in chunks
    genes = [g for g in range(ds.num_genes) if one_batch(ds, [g], pep, 9, 27)[0][0] == "ok"]
    assert len(genes) > ds.num_genes // 2
    want, _tsv = one_batch(ds, genes, pep, 9, 27)
    assert want[0] == "ok" and want[2][3] > 0 and want[2][4] > 0
    chunks = [genes[lo:hi] for lo, hi in cost_ranges([1] * len(genes), 4)]
    for contexts in ([ctx], [ctx, ctx2]):
        got, _ = streamed(ds, chunks, pep, 9, 27, contexts)
        assert got == want
    monkeypatch.delenv("MP_TEST_ROW_SLOTS")


def test_4000_transcripts_in_8_streamed_chunks_match_the_oracle_verified_checksums(ctx, ctx2):
    """tests/golden/config_e/checksums_4000.json with the somatic half in 8 chunks on two contexts, streamed into one filter."""
    import microphaser_amd as m
    from microphaser_amd.pipeline import cost_ranges
    gold = json.load(open(os.path.join(GOLDEN, "config_e", "checksums_4000.json")))
    L = gold["peptide_len"]
    md5 = lambda x: hashlib.md5(x).hexdigest()
    ds = ctx.synth(gold["seed"], gold["transcripts"], gold["depth"], gold["spacing"], gene_streams=True)
    nb = ds.batch(window_len=3 * L, mode=m.MODE_NORMAL)
    nb.run()
    pep = nb.peptidome(L)[0]
    nb.close()
    chunks = ranges_to_chunks(cost_ranges(ds.gene_costs(), 8))
    assert len(chunks) == 8
    fs = m.FilterStream(ctx, pep, L)
    tsvs = []
    for i, genes in enumerate(chunks):
        b = batch_on((ctx, ctx2)[i % 2], ds, genes, 3 * L)
        b.run()
        tsvs.append(fs.add(b, m.STREAM_TSV).tsv)
        b.close()
    f = fs.finish()
    assert md5(concat_tsvs(tsvs)) == gold["md5"]["somatic_tsv"]
    got = {"filter_fasta": md5(f.fasta), "filter_normal_fasta": md5(f.normal_fasta), "filter_tsv": md5(f.tsv),
           "filter_removed_tsv": md5(f.removed_tsv), "filter_removed_fasta": md5(f.removed_fasta)}
    assert got == {k: gold["md5"][k] for k in got}
    c = gold["counts"]
    assert (f.rows, f.kept, f.removed, f.groups) == (c["somatic_tsv_rows"], c["filter_kept"], c["filter_removed"], c["filter_groups"])


def test_a_non_acgt_coding_base_in_the_second_chunk_fails_like_one_batch(ctx, ctx2):
    """One coding base set to N inside the window of a TSV row of a gene in the second of three chunks (through the phase_gene seam):
    the first add goes through, the second fails with Batch.filter's message on all genes; the stream then refuses further use, and
    both contexts still work."""
    import microphaser_amd as m
    from microphaser_amd.pipeline import cost_ranges
    L, w = 9, 27
    src = ctx.synth(303, 30, indel_rate=0.03)
    chunks = ranges_to_chunks(cost_ranges(src.gene_costs(), 3))
    assert len(chunks) == 3
    arr = src.to_arrays(mode=m.MODE_SOMATIC)
    refseq = np.array(arr["refseq"], copy=True)
    target = None
    for g in chunks[1]:
        b = src.batch(window_len=w, gene_lo=g, gene_hi=g + 1)
        b.run()
        lo, hi = int(arr["ref_off"][g]), int(arr["ref_off"][g + 1])
        at = lambda pos: lo + pos - int(arr["gene_start"][g])
        for c in (l.split(b"\t") for l in b.results(m.STREAM_TSV).tsv.split(b"\n")[1:] if l):
            # a Forward row whose 27 bases lie contiguously in the reference (no splice inside), away from its variant sites
            if c[13] != b"Forward" or len(c[20]) != 27:
                continue
            pos0 = int(c[5]) - 1
            if not all(lo <= at(pos0 + k) < hi for k in range(27)):
                continue
            sites = {int(x) for x in c[14].split(b"|") if x}
            same = all(pos0 + k + 1 in sites or chr(refseq[at(pos0 + k)]).upper() == chr(c[20][k]).upper() for k in range(27))
            free = [k for k in range(9, 18) if pos0 + k + 1 not in sites]
            if same and free:
                target = at(pos0 + free[0])
                break
        if target is not None:
            break
    assert target is not None
    refseq[target] = ord("N")
    arr["refseq"] = refseq
    ds = ctx.from_arrays(arr)
    ref_bin = open(REF_BIN, "rb").read()
    want, _tsv = one_batch(ds, range(ds.num_genes), ref_bin, L, w)
    assert want[0] == "error" and "Result::unwrap()" in want[1] and "other than A, C, G, T" in want[1], want
    fs = m.FilterStream(ctx, ref_bin, L)
    b1 = batch_on(ctx, ds, chunks[0], w)
    b1.run()
    fs.add(b1)
    b2 = batch_on(ctx2, ds, chunks[1], w)
    b2.run()
    with pytest.raises(m.MicrophaserError) as e:
        fs.add(b2)
    assert str(e.value) == want[1]
    b3 = batch_on(ctx, ds, chunks[2], w)
    b3.run()
    with pytest.raises(m.MicrophaserError, match="an earlier add on this stream failed"):
        fs.add(b3)
    with pytest.raises(m.MicrophaserError, match="an earlier add on this stream failed"):
        fs.finish()
    # both contexts still work: the untouched exome, chunked over them, equals its one batch
    want, _ = one_batch(src, range(src.num_genes), ref_bin, L, w)
    got, _ = streamed(src, chunks, ref_bin, L, w, [ctx, ctx2])
    assert want[0] == "ok" and got == want


def test_adding_a_batch_after_another_batch_ran_on_its_context_fails_like_results(ctx):
    import microphaser_amd as m
    ds = ctx.synth(5, 6)
    ref_bin = open(REF_BIN, "rb").read()
    b1 = ds.batch(gene_hi=3)
    b1.run()
    b2 = ds.batch(gene_lo=3)
    b2.run()
    with pytest.raises(m.MicrophaserError) as res_err:
        b1.results()
    fs = m.FilterStream(ctx, ref_bin, 9)
    with pytest.raises(m.MicrophaserError) as add_err:
        fs.add(b1)
    assert "another batch" in str(res_err.value) and str(add_err.value) == str(res_err.value)
    # run again, it is resident: a new stream takes it and the batch after it
    want, _ = one_batch(ds, range(ds.num_genes), ref_bin, 9, 27)
    fs = m.FilterStream(ctx, ref_bin, 9)
    b1.run()
    fs.add(b1)
    b2.run()
    fs.add(b2)
    assert outcome(fs.finish) == want


@pytest.mark.parametrize("n_chunks", [1, 3])
def test_filter_chunked_equals_the_one_batch_filter(ctx, ctx2, exome, n_chunks):
    import microphaser_amd as m
    from microphaser_amd.pipeline import cost_ranges, filter_chunked
    ds, peps = exome
    L, w = 9, 27
    want, tsv = one_batch(ds, range(ds.num_genes), peps[L], L, w)
    f, res = filter_chunked(ds, peps[L], n_chunks=n_chunks, peptide_len=L, contexts=[ctx, ctx2], streams=m.STREAM_TSV)
    assert ("ok", streams(f), counts(f)) == want
    assert len(res) == len(cost_ranges(ds.gene_costs(), n_chunks)) and concat_tsvs([r.tsv for r in res]) == tsv
    f, res = filter_chunked(ds, peps[L].binary, n_chunks=n_chunks, peptide_len=L, contexts=[ctx, ctx2])
    assert res is None and ("ok", streams(f), counts(f)) == want
    # a handle's own peptide length sets the windows (3 L nt), whatever peptide_len says
    want15, _ = one_batch(ds, range(ds.num_genes), peps[15], 15, 45)
    f, _ = filter_chunked(ds, peps[15], n_chunks=n_chunks, contexts=[ctx, ctx2])
    assert ("ok", streams(f), counts(f)) == want15 and want15[2][3] > 0
