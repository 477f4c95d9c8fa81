"""`somatic` -> `filter` without the info.tsv text (mp_batch_filter / mp_batch_filter_binary / Batch.filter / `somatic
--filter-reference`): byte for byte the five streams, the counts and the errors of the text path `Batch.results().tsv` -> ctx.filter."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ORACLE_CLI, SOMATIC_FIXTURES

pytestmark = pytest.mark.gpu

REF_BIN = os.path.join(GOLDEN, "test_filter", "reference.binary")


@pytest.fixture(scope="module")
def ctx(built):
    import microphaser_amd as m
    return m.Context(0)


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


def compare_batch(ctx, b, reference, L):
    """Text path and fused path on one run of batch b (reference: Peptides handle or bincode bytes). Returns the text path's Filtered."""
    import microphaser_amd as m
    tsv = b.results(m.STREAM_TSV).tsv
    text = ctx.filter(tsv, reference, L)
    fused, res = b.filter(reference, L)
    assert res is None
    assert streams(fused) == streams(text)
    assert counts(fused) == counts(text)
    assert fused.rows == max(0, tsv.count(b"\n") - 1)
    return text


def load(ctx, name):
    d, bam, vcf, gtf, fa, _stem = SOMATIC_FIXTURES[name]
    base = os.path.join(GOLDEN, d)
    return ctx.load(os.path.join(base, bam), os.path.join(base, vcf), os.path.join(base, fa), os.path.join(base, gtf))


@pytest.mark.parametrize("L", [8, 9])
@pytest.mark.parametrize("name", sorted(SOMATIC_FIXTURES))
def test_fused_filter_equals_the_text_path_on_the_reference_fixtures(ctx, name, L):
    import microphaser_amd as m
    ds = load(ctx, name)
    own = _normal_peptidome(ctx, ds, 27, L)   # the fixture's own `normal` run -> build_reference
    b = ds.batch(window_len=27)
    b.run()
    ref_bin = open(REF_BIN, "rb").read()
    f_own = compare_batch(ctx, b, own, L)                  # mp_batch_filter
    f_bin = compare_batch(ctx, b, ref_bin, L)              # mp_batch_filter_binary
    assert f_own.rows > 5 and f_own.peptides > 0 and f_bin.rows == f_own.rows
    full = b.results()
    fused, res = b.filter(ref_bin, L, m.STREAM_ALL)        # the somatic streams of the same consumer pass
    assert (res.fasta, res.normal_fasta, res.tsv, res.windows) == (full.fasta, full.normal_fasta, full.tsv, full.windows)
    assert res.gene_offsets(2) == full.gene_offsets(2)
    assert streams(fused) == streams(f_bin)
    fused, res = b.filter(own, streams=m.STREAM_NORMAL_FASTA)
    assert res.normal_fasta == full.normal_fasta and res.tsv == b"" and res.fasta == b""
    assert streams(fused) == streams(f_own)


def test_fused_filter_of_a_batch_without_rows_equals_the_empty_tsv(ctx):
    import microphaser_amd as m
    d, bam, _vcf, gtf, fa, _stem = SOMATIC_FIXTURES["test_forward"]
    base = os.path.join(GOLDEN, d)
    b = ctx.load(os.path.join(base, bam), os.path.join(GOLDEN, "test_empty", "empty_test.vcf"), os.path.join(base, fa),
                 os.path.join(base, gtf)).batch(window_len=27)
    b.run()
    assert b.results().tsv == b""
    for reference in (open(REF_BIN, "rb").read(), ctx.peptides_union([], 9)):
        want = outcome(lambda: ctx.filter(b"", reference, 9))
        got = outcome(lambda: b.filter(reference, 9)[0])
        assert got == want
        assert want[0] == "ok" and want[2][0] == 0 and want[1][2].startswith(b"id\ttranscript")


def _acgt_records(fasta):
    """The records of a one-line-per-record FASTA whose bases are all A, C, G, T (any case): what build_reference translates without
    the reference's panic on another base."""
    lines = fasta.split(b"\n")
    keep = [(i, s) for i, s in zip(lines[0:-1:2], lines[1::2]) if not s.upper().translate(None, b"ACGT")]
    return b"".join(i + b"\n" + s + b"\n" for i, s in keep)


def _normal_peptidome(ctx, ds, w, L):
    """build_reference of the `normal` FASTA of ds (genes the reference would panic on, and records with a base outside ACGT, left out)."""
    import microphaser_amd as m
    try:
        b = ds.batch(window_len=w, mode=m.MODE_NORMAL)
        b.run()
        return ctx.peptidome(_acgt_records(b.results(m.STREAM_FASTA).fasta), L)
    except m.MicrophaserError as e:
        assert str(e).startswith("reference would panic"), str(e)
    fas = []
    for g in range(ds.num_genes):
        try:
            b = ds.batch(window_len=w, gene_lo=g, gene_hi=g + 1, mode=m.MODE_NORMAL)
            b.run()
            fas.append(b.results(m.STREAM_FASTA).fasta)
        except m.MicrophaserError as e:
            assert str(e).startswith("reference would panic"), str(e)
    return ctx.peptidome(_acgt_records(b"".join(fas)), L)


def _compare_dataset(ctx, ds, pep, L, w):
    """The whole data set as one `somatic` batch; if the reference would panic on a gene, both paths must fail alike, and then the
    genes are compared one by one (the panicking ones left out). Returns (kept, removed) summed over what was compared."""
    import microphaser_amd as m
    b = ds.batch(window_len=w)
    b.run()
    want = outcome(lambda: ctx.filter(b.results(m.STREAM_TSV).tsv, pep, L))
    b.run()
    got = outcome(lambda: b.filter(pep, L)[0])
    assert got == want
    if want[0] == "ok":
        return want[2][3], want[2][4]
    kept = removed = skipped = 0
    for g in range(ds.num_genes):
        b = ds.batch(window_len=w, gene_lo=g, gene_hi=g + 1)
        try:
            b.run()
            tsv = b.results(m.STREAM_TSV).tsv
        except m.MicrophaserError as e:
            assert str(e).startswith("reference would panic"), str(e)
            skipped += 1
            continue
        want = outcome(lambda: ctx.filter(tsv, pep, L))
        got = outcome(lambda: b.filter(pep, L)[0])
        assert got == want
        if want[0] == "ok":
            kept, removed = kept + want[2][3], removed + want[2][4]
    assert skipped < ds.num_genes // 2
    return kept, removed


SYNTH = dict(indel_rate=0.04, multiallelic_rate=0.1, softmask_rate=0.3, mate_rate=0.1, isoform_rate=0.3)


@pytest.mark.parametrize("L,w", [(9, 27), (15, 45), (25, 75), (9, 30), (10, 27)])
def test_fused_filter_equals_the_text_path_on_synthetic_exomes(ctx, L, w):
    """Indels, multi-allelic sites, soft-masked reference, mates and second isoforms: merged rows from the splice-side merge, '-'
    strands, windows that are not a multiple of 3 (w = 30), and one-word (L = 9, 10) and two-word (L = 15, 25) keys. At w = 27,
    L = 10 only rows lengthened by an insertion hold a 10-mer, so kept and removed are only required where w >= 3L."""
    kept = removed = 0
    for seed in (11, 29):
        ds = ctx.synth(seed, 24, 20.0, 4.0, **SYNTH)
        k, r = _compare_dataset(ctx, ds, _normal_peptidome(ctx, ds, w, L), L, w)
        kept, removed = kept + k, removed + r
    if w >= 3 * L:
        assert kept > 0 and removed > 0


def test_fused_filter_on_the_threaded_host_legs(ctx, monkeypatch):
    """An exome large enough for the threaded consumer and filter legs (as test_gpu_filter_host_legs_threaded_quoted_and_by_handle
    sizes it), on default threads and on one."""
    import microphaser_amd as m
    L = 9
    ds = ctx.synth(515, 80, 30.0, 5.4, gene_streams=True)
    pep = ctx.build_reference(ds.phase(window_len=3 * L, mode=m.MODE_NORMAL).fasta, L)
    b = ds.batch(window_len=3 * L)
    b.run()
    assert len(b.results(m.STREAM_TSV).tsv) > 2 * (4 << 20)
    f = compare_batch(ctx, b, pep, L)
    assert f.kept > 1000 and f.removed > 100
    monkeypatch.setenv("MP_THREADS", "1")
    fused1, _ = b.filter(pep.binary, L)
    monkeypatch.delenv("MP_THREADS")
    assert streams(fused1) == streams(f) and counts(fused1) == counts(f)


def test_fused_filter_with_genes_split_into_read_subsets(ctx, monkeypatch):
    """MP_TEST_ROW_SLOTS=24 plans nearly every gene as 2..3 copies with disjoint read subsets (test_gpu_parity's deep-gene test): the
    captured rows then name the record slots of the first copy that holds each group."""
    monkeypatch.setenv("MP_TEST_ROW_SLOTS", "24")
    ds = ctx.synth(1717, 40, indel_rate=0.08, multiallelic_rate=0.05, softmask_rate=0.2, mate_rate=0.3)
    pep = _normal_peptidome(ctx, ds, 27, 9)
    kept, removed = _compare_dataset(ctx, ds, pep, 9, 27)
    monkeypatch.delenv("MP_TEST_ROW_SLOTS")
    assert kept > 0 and removed > 0


def test_fused_filter_at_4000_transcripts_matches_the_oracle_verified_checksums(ctx):
    """Config E at 4000 transcripts (tests/golden/config_e/checksums_4000.json, recorded in a run where the oracle's stages produced
    the same bytes): the fused filter's five streams and its kept / removed / group counts."""
    import microphaser_amd as m
    gold = json.load(open(os.path.join(GOLDEN, "config_e", "checksums_4000.json")))
    L = gold["peptide_len"]
    md5 = lambda x: hashlib.md5(x).hexdigest()
    ds = ctx.synth(gold["seed"], gold["transcripts"], gold["depth"], gold["spacing"], gene_streams=True)
    nb = ds.batch(window_len=3 * L, mode=m.MODE_NORMAL)
    nb.run()
    pep = nb.peptidome(L)[0]
    nb.close()
    b = ds.batch(window_len=3 * L)
    b.run()
    f, res = b.filter(pep, streams=m.STREAM_TSV)
    assert md5(res.tsv) == gold["md5"]["somatic_tsv"]
    got = {"filter_fasta": md5(f.fasta), "filter_normal_fasta": md5(f.normal_fasta), "filter_tsv": md5(f.tsv),
           "filter_removed_tsv": md5(f.removed_tsv), "filter_removed_fasta": md5(f.removed_fasta)}
    assert got == {k: gold["md5"][k] for k in got}
    c = gold["counts"]
    assert (f.kept, f.removed, f.groups) == (c["filter_kept"], c["filter_removed"], c["filter_groups"])


def _oracle_filter(tmp_path, tsv, ref_bin, L):
    info = tmp_path / "o.info.tsv"
    info.write_bytes(tsv)
    r = subprocess.run([ORACLE_CLI, "filter", "-r", str(ref_bin), "-l", str(L), "-t", str(info), "-o", str(tmp_path / "o.tsv"),
                        "-n", str(tmp_path / "o.normal.fa"), "-s", str(tmp_path / "o.removed.tsv"), "-p", str(tmp_path / "o.removed.fa")],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    return (r.stdout, (tmp_path / "o.normal.fa").read_bytes(), (tmp_path / "o.tsv").read_bytes(), (tmp_path / "o.removed.tsv").read_bytes(),
            (tmp_path / "o.removed.fa").read_bytes())


def test_fused_filter_at_15_mers_matches_the_oracle(ctx, tmp_path):
    """`normal -w 45` -> `build_reference -l 15` -> `somatic -w 45` -> fused filter, against the oracle's `filter -l 15` on the TSV."""
    import microphaser_amd as m
    L, W = 15, 45
    ds = ctx.synth(303, 30, indel_rate=0.03)
    pep = ctx.build_reference(ds.phase(window_len=W, mode=m.MODE_NORMAL).fasta, L)
    ref_bin = tmp_path / "reference.binary"
    ref_bin.write_bytes(pep.binary)
    b = ds.batch(window_len=W)
    b.run()
    want = _oracle_filter(tmp_path, b.results(m.STREAM_TSV).tsv, ref_bin, L)
    f_bin, _ = b.filter(pep.binary, L)
    f_pep, _ = b.filter(pep)
    assert streams(f_bin) == want and streams(f_pep) == want
    assert f_bin.kept > 100 and f_bin.removed > 100


def test_a_non_acgt_coding_base_fails_alike_on_both_paths(ctx):
    """A somatic fixture handed over through the phase_gene seam with one coding base of refseq set to N, inside the window of a TSV
    row: the text filter and the fused filter refuse the codon with the same message, and the context still works afterwards."""
    import microphaser_amd as m
    ds = load(ctx, "splice_forward_test")
    b = ds.batch(window_len=27)
    b.run()
    rows = [l.split(b"\t") for l in b.results(m.STREAM_TSV).tsv.split(b"\n")[1:] if l]
    arr = ds.to_arrays(mode=m.MODE_SOMATIC)
    refseq = np.array(arr["refseq"], copy=True)
    at = lambda pos: int(arr["ref_off"][0]) + pos - int(arr["gene_start"][0])
    target = None
    for c in rows:   # a Forward row whose 27 bases lie contiguously in the reference (no splice inside), away from its variant sites
        if c[13] != b"Forward" or len(c[20]) != 27:
            continue
        pos0 = int(c[5]) - 1
        sites = {int(x) for x in c[14].split(b"|") if x}
        same = all(pos0 + k + 1 in sites or chr(refseq[at(pos0 + k)]).upper() == chr(c[20][k]).upper() for k in range(27))
        free = [k for k in range(9, 18) if pos0 + k + 1 not in sites]
        if same and free:
            target = at(pos0 + free[0])
            break
    assert target is not None
    refseq[target] = ord("N")
    arr["refseq"] = refseq
    b = ctx.from_arrays(arr).batch(window_len=27)
    b.run()
    ref_bin = open(REF_BIN, "rb").read()
    tsv = b.results(m.STREAM_TSV).tsv
    with pytest.raises(m.MicrophaserError) as text_err:
        ctx.filter(tsv, ref_bin, 9)
    with pytest.raises(m.MicrophaserError) as fused_err:
        b.filter(ref_bin, 9)
    assert "Result::unwrap()" in str(text_err.value) and "other than A, C, G, T" in str(text_err.value)
    assert str(fused_err.value) == str(text_err.value)
    b.run()   # the context is still good
    assert b.results(m.STREAM_TSV).tsv == tsv
    good = load(ctx, "splice_forward_test").batch(window_len=27)
    good.run()
    compare_batch(ctx, good, ref_bin, 9)


def test_fused_filter_after_another_batch_ran_fails_like_results(ctx):
    import microphaser_amd as m
    ds = ctx.synth(5, 6)
    ref_bin = open(REF_BIN, "rb").read()
    b1 = ds.batch()
    b1.run()
    b2 = ds.batch(gene_hi=3)
    b2.run()
    with pytest.raises(m.MicrophaserError) as res_err:
        b1.results()
    with pytest.raises(m.MicrophaserError) as filt_err:
        b1.filter(ref_bin, 9)
    assert "another batch" in str(res_err.value) and str(filt_err.value) == str(res_err.value)
    b1.run()
    compare_batch(ctx, b1, ref_bin, 9)


@pytest.mark.parametrize("L,w", [(9, 27), (15, 45)])
def test_cli_filter_reference_equals_somatic_then_filter(built, tmp_path, L, w):
    import microphaser_amd as m
    ds = m.Context(-1).synth(303, 30, indel_rate=0.03)
    prefix = str(tmp_path / "s")
    ds.write(prefix)
    base = [prefix + ".bam", "-r", prefix + ".fa", "-b", prefix + ".vcf", "-w", str(w)]

    def run(args, cwd):
        os.makedirs(str(cwd), exist_ok=True)
        with open(prefix + ".gtf", "rb") as g:
            r = subprocess.run([m.CLI_PATH] + args, stdin=g, capture_output=True, cwd=str(cwd), timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r.stdout

    files = lambda d, names: {n: (d / n).read_bytes() for n in names}
    FILTER_OUT = ["info.filtered.tsv", "info.removed.tsv", "peptides.removed.fasta", "normal.filtered.fa"]
    text = tmp_path / "text"
    (text / "n.fa").parent.mkdir()
    (text / "n.fa").write_bytes(run(["normal"] + base, text))
    run(["build_reference", "-r", "n.fa", "-o", "q.bin", "-l", str(L)], text)
    som_fa = run(["somatic"] + base + ["--tsv", "info.tsv", "-n", "normal.fasta"], text)
    som = files(text, ["info.tsv", "normal.fasta"])
    filt_fa = run(["filter", "-t", "info.tsv", "-r", "q.bin", "-l", str(L)], text)
    want = files(text, FILTER_OUT)
    assert som["info.tsv"].count(b"\n") > 1000 and len(filt_fa) > 0 and b"\n" in want["info.removed.tsv"]
    ref = str(text / "q.bin")
    fused = tmp_path / "fused"
    assert run(["somatic"] + base + ["--filter-reference", ref, "-l", str(L)], fused) == filt_fa
    assert sorted(os.listdir(str(fused))) == sorted(FILTER_OUT)            # no info.tsv, no normal.fasta
    assert files(fused, FILTER_OUT) == want
    named = tmp_path / "named"
    out = run(["somatic"] + base + ["--filter-reference", ref, "--peptide-length", str(L), "--filtered-tsv", "f.tsv", "-s", "r.tsv",
                                    "-p", "r.fa", "--filtered-normal-output", "n.fa", "--tsv", "t.tsv", "-n", "nn.fa"], named)
    assert out == filt_fa
    got = files(named, ["f.tsv", "r.tsv", "r.fa", "n.fa", "t.tsv", "nn.fa"])
    assert (got["f.tsv"], got["r.tsv"], got["r.fa"], got["n.fa"]) == (want["info.filtered.tsv"], want["info.removed.tsv"],
                                                                      want["peptides.removed.fasta"], want["normal.filtered.fa"])
    assert (got["t.tsv"], got["nn.fa"]) == (som["info.tsv"], som["normal.fasta"])
    assert som_fa.count(b">") > 100
