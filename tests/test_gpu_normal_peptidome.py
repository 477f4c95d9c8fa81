"""`normal` -> `build_reference` without the nucleotide FASTA (mp_batch_peptidome / Batch.peptidome / `normal --peptidome-output`):
byte for byte the peptidome of the text path `Batch.results(STREAM_FASTA).fasta` -> ctx.peptidome / ctx.build_reference."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, NORMAL_FIXTURES, REVERSE_GERMLINE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built):
    import microphaser_amd as m
    return m.Context(0)


def fasta_windows(fasta, L):
    """(records, windows, records with 0 / 1 / several windows, ids ending in 'R') of a one-line-per-record FASTA."""
    lines = fasta.split(b"\n")
    ids, seqs = lines[0:-1:2], lines[1::2]
    n = [len(s) // 3 - L + 1 if len(s) >= 3 * L else 0 for s in seqs]   # == (len - 3L) / 3 + 1
    return dict(records=len(seqs), windows=sum(n), zero=sum(1 for k in n if k == 0), one=sum(1 for k in n if k == 1),
                several=sum(1 for k in n if k > 1), reverse=sum(1 for i in ids if not i.endswith(b"F")))


def assert_same_peptidome(fused, text):
    assert fused.key_words == text.key_words
    assert fused.count == text.count
    assert np.array_equal(fused.keys_np, text.keys_np)
    assert fused.binary == text.binary
    assert fused.fasta == b""


def compare_batch(ctx, b, L):
    """Text path and fused path on one run of batch b; returns the FASTA the text path went through."""
    import microphaser_amd as m
    fasta = b.results(m.STREAM_FASTA).fasta
    text = ctx.peptidome(fasta, L)
    fused, res = b.peptidome(L)
    assert res is None
    assert_same_peptidome(fused, text)
    assert fused.count == fasta_windows(fasta, L)["windows"]
    assert ctx.build_reference(fasta, L).binary == fused.binary   # the FASTA-translating entry point agrees as well
    return fasta


def load(ctx, d, bam, vcf, fa, gtf):
    return ctx.load(os.path.join(d, bam), os.path.join(d, vcf), os.path.join(d, fa), os.path.join(d, gtf))


@pytest.mark.parametrize("L", [8, 9])
@pytest.mark.parametrize("name", sorted(NORMAL_FIXTURES))
def test_fused_peptidome_equals_the_text_path_on_the_normal_fixtures(ctx, name, L):
    import microphaser_amd as m
    bam, vcf, gtf, fa, _exp = NORMAL_FIXTURES[name]
    b = load(ctx, os.path.join(GOLDEN, name), bam, vcf, fa, gtf).batch(window_len=27, mode=m.MODE_NORMAL)
    b.run()
    fasta = compare_batch(ctx, b, L)
    st = fasta_windows(fasta, L)
    assert st["windows"] > 50
    if L == 8:
        assert st["several"] > 0   # a 27-nt record holds two 8-mers


@pytest.mark.parametrize("L", [8, 9])
@pytest.mark.parametrize("gtf_key", ["gtf", "last_exon_gtf"])
def test_fused_peptidome_equals_the_text_path_on_the_reverse_strand_fixture(ctx, gtf_key, L):
    import microphaser_amd as m
    R = REVERSE_GERMLINE
    b = load(ctx, R["dir"], R["bam"], R["vcf"], R["fasta"], R[gtf_key]).batch(window_len=27, mode=m.MODE_NORMAL)
    b.run()
    fasta = compare_batch(ctx, b, L)
    assert fasta_windows(fasta, L)["reverse"] > 40


def _compare_dataset(ctx, ds, L, w):
    """The whole data set as one batch; if the reference would panic on a gene, both paths must fail alike, and then the genes are
    compared one by one (the panicking ones left out). Returns the FASTA statistics of what was compared."""
    import microphaser_amd as m
    b = ds.batch(window_len=w, mode=m.MODE_NORMAL)
    b.run()
    try:
        return fasta_windows(compare_batch(ctx, b, L), L)
    except m.MicrophaserError as e:
        msg = str(e)
    b.run()
    with pytest.raises(m.MicrophaserError) as fused_err:
        b.peptidome(L)
    assert str(fused_err.value) == msg
    tot, skipped = {}, 0
    for g in range(ds.num_genes):
        b = ds.batch(window_len=w, gene_lo=g, gene_hi=g + 1, mode=m.MODE_NORMAL)
        b.run()
        try:
            st = fasta_windows(compare_batch(ctx, b, L), L)
        except m.MicrophaserError as e:
            assert str(e).startswith("reference would panic"), str(e)
            b.run()
            with pytest.raises(m.MicrophaserError, match="reference would panic"):
                b.peptidome(L)
            skipped += 1
            continue
        for k, v in st.items():
            tot[k] = tot.get(k, 0) + v
    assert skipped < ds.num_genes // 2
    return tot


SYNTH = dict(indel_rate=0.04, multiallelic_rate=0.1, softmask_rate=0.3, mate_rate=0.1, isoform_rate=0.3)


@pytest.mark.parametrize("L,w", [(9, 27), (15, 45), (25, 75), (9, 30), (10, 27)])
def test_fused_peptidome_equals_the_text_path_on_synthetic_exomes(ctx, L, w):
    """Indels, multi-allelic sites, soft-masked reference, mates and second isoforms: merged records, '-' strands, records with
    one window (w = 3L), several (w = 30, L = 9) and, at w = 27, L = 10, mostly none (only records lengthened by an insertion hold a
    30-nt window); one-word (L = 9, 10) and two-word (L = 15, 25) keys."""
    tot = {}
    for seed in (11, 29):
        ds = ctx.synth(seed, 24, 20.0, 4.0, **SYNTH)
        for k, v in _compare_dataset(ctx, ds, L, w).items():
            tot[k] = tot.get(k, 0) + v
    assert tot["records"] > 1000 and tot["reverse"] > 100
    if w < 3 * L:
        assert tot["zero"] > 1000 and 0 < tot["windows"] < tot["records"]
    elif w == 3 * L:
        assert tot["one"] > 1000
    else:
        assert tot["several"] > 1000


def test_streams_of_the_fused_pass_equal_batch_results(ctx):
    import microphaser_amd as m
    ds = ctx.synth(11, 24, 20.0, 4.0, **SYNTH)
    b = ds.batch(window_len=27, gene_hi=8, mode=m.MODE_NORMAL)
    b.run()
    fa = b.results(m.STREAM_FASTA).fasta
    full = b.results()
    pep_fa, res_fa = b.peptidome(9, m.STREAM_FASTA)
    assert res_fa.fasta == fa and res_fa.tsv == b""
    pep_all, res_all = b.peptidome(9, m.STREAM_ALL)
    assert (res_all.fasta, res_all.tsv, res_all.windows) == (full.fasta, full.tsv, full.windows)
    assert res_all.gene_offsets(0) == full.gene_offsets(0) and res_all.gene_offsets(2) == full.gene_offsets(2)
    assert_same_peptidome(pep_fa, pep_all)
    assert_same_peptidome(pep_fa, ctx.peptidome(fa, 9))


def test_a_non_acgt_coding_base_fails_alike_on_both_paths(ctx):
    """A data set handed over through the phase_gene seam with one coding base of refseq set to N: the text path's build_reference
    and the fused path both refuse the codon with the reference's unwrap panic."""
    import microphaser_amd as m
    bam, vcf, gtf, fa, _exp = NORMAL_FIXTURES["splice_forward_test"]
    arr = load(ctx, os.path.join(GOLDEN, "splice_forward_test"), bam, vcf, fa, gtf).to_arrays(mode=m.MODE_NORMAL)
    e0, e1 = int(arr["exon_off"][0]), int(arr["exon_off"][1])
    k = max(range(e0, e1), key=lambda e: int(arr["exon_end"][e]) - int(arr["exon_start"][e]))   # the first transcript's longest exon
    pos = (int(arr["exon_start"][k]) + int(arr["exon_end"][k])) // 2
    refseq = np.array(arr["refseq"], copy=True)
    refseq[int(arr["ref_off"][0]) + pos - int(arr["gene_start"][0])] = ord("N")
    arr["refseq"] = refseq
    b = ctx.from_arrays(arr).batch(window_len=27, mode=m.MODE_NORMAL)
    b.run()
    with pytest.raises(m.MicrophaserError) as text_err:
        ctx.peptidome(b.results(m.STREAM_FASTA).fasta, 9)
    with pytest.raises(m.MicrophaserError) as fused_err:
        b.peptidome(9)
    assert "Result::unwrap()" in str(text_err.value)
    assert str(fused_err.value) == str(text_err.value)
    b.run()   # the context is still good
    assert b.results(m.STREAM_FASTA).windows > 0


def test_fused_peptidome_after_another_batch_ran_fails_like_results(ctx):
    import microphaser_amd as m
    ds = ctx.synth(5, 6)
    b1 = ds.batch(mode=m.MODE_NORMAL)
    b1.run()
    b2 = ds.batch(gene_hi=3, mode=m.MODE_NORMAL)
    b2.run()
    with pytest.raises(m.MicrophaserError) as res_err:
        b1.results()
    with pytest.raises(m.MicrophaserError) as pep_err:
        b1.peptidome(9)
    assert "another batch" in str(res_err.value) and str(pep_err.value) == str(res_err.value)
    b1.run()
    compare_batch(ctx, b1, 9)


def test_cli_peptidome_output_equals_normal_then_build_reference(built, tmp_path):
    import microphaser_amd as m
    ds = m.Context(-1).synth(77, 24, mate_rate=0.1, isoform_rate=0.3)
    prefix = str(tmp_path / "s")
    ds.write(prefix)
    base = [prefix + ".bam", "-r", prefix + ".fa", "-b", prefix + ".vcf", "-w", "27"]

    def run(args):
        with open(prefix + ".gtf", "rb") as g:
            r = subprocess.run([m.CLI_PATH] + args, stdin=g, capture_output=True, cwd=str(tmp_path), timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r.stdout

    fa = run(["normal"] + base + ["--tsv", "n.tsv"])
    (tmp_path / "n.fa").write_bytes(fa)
    run(["build_reference", "-r", "n.fa", "-o", "q.bin", "-l", "9"])
    q = (tmp_path / "q.bin").read_bytes()
    plain_tsv = (tmp_path / "n.tsv").read_bytes()
    assert plain_tsv.count(b"\n") > 1000 and len(q) > 10000
    for extra in ([], ["--devices", "0,0,0"]):
        for d in ("p.bin", "t.tsv", "info.tsv"):
            if (tmp_path / d).exists():
                (tmp_path / d).unlink()
        assert run(["normal"] + base + ["--peptidome-output", "p.bin", "-l", "9"] + extra) == b""
        assert (tmp_path / "p.bin").read_bytes() == q
        assert not (tmp_path / "info.tsv").exists()   # the TSV only when --tsv is given
        assert run(["normal"] + base + ["--peptidome-output", "p.bin", "--peptide-length", "9", "--tsv", "t.tsv"] + extra) == b""
        assert (tmp_path / "p.bin").read_bytes() == q
        assert (tmp_path / "t.tsv").read_bytes() == plain_tsv


def test_config_e_rank_fused_peptidome_equals_the_default(ctx):
    import microphaser_amd as m
    from microphaser_amd.pipeline import config_e_rank
    ds = ctx.synth(2020, 1000, 30.0, 5.4, gene_streams=True)
    genes = list(range(ds.num_genes))
    merged, pep, filt = config_e_rank(ctx, ds, genes, genes, peptide_len=9)
    merged_f, pep_f, filt_f = config_e_rank(ctx, ds, genes, genes, peptide_len=9, fused_peptidome=True)
    assert np.array_equal(pep.keys_np, pep_f.keys_np) and pep.keys_np.size > 100000
    assert pep.binary == pep_f.binary
    assert merged == merged_f
    assert (filt.fasta, filt.tsv, filt.removed_tsv) == (filt_f.fasta, filt_f.tsv, filt_f.removed_tsv)
