"""Peptide lengths 13..25 (MHC class II, two-word keys) on the GPU: K4 translation, build_reference, config E at 15-mers
(`normal -w 45` -> `build_reference -l 15` -> `somatic -w 45` -> `filter -l 15`) and the CLI, against a Python translation and
the CPU oracle on the same bytes."""
import json
import random
import subprocess

import pytest

from conftest import ORACLE_CLI

pytestmark = pytest.mark.gpu

CODONS = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVVXYXYSSSSXCWCLFLF"   # 16 b0 + 4 b1 + b2, A C G T = 0 1 2 3
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def translate_py(nt, reverse):
    s = nt.upper()
    if reverse:
        s = "".join(COMPLEMENT[c] for c in reversed(s))
    return "".join(CODONS[16 * "ACGT".index(s[i]) + 4 * "ACGT".index(s[i + 1]) + "ACGT".index(s[i + 2])] for i in range(0, len(s), 3))


def key_py(pep):
    k = 0
    for c in pep:
        k = (k << 5) | ((ord(c) - 65) & 31)
    return k


@pytest.fixture(scope="module")
def ctx(built):
    import microphaser_amd as m
    return m.Context(0)


@pytest.mark.parametrize("L", [13, 15, 25])
def test_gpu_translate_two_word_keys_match_a_python_translation(ctx, L):
    import microphaser_amd as m
    rnd = random.Random(L)
    n = 3000
    wins = ["".join(rnd.choice("ACGTacgt") for _ in range(3 * L)) for _ in range(n)]
    rev = [rnd.randrange(2) for _ in range(n)]
    aa, keys = ctx.translate("".join(wins).encode(), rev, L)
    want = [translate_py(w, r) for w, r in zip(wins, rev)]
    assert aa.decode() == "".join(want)
    assert keys == [key_py(p) for p in want]
    assert max(keys) >= 1 << 64 and all(m.key_to_peptide(k, L) == p for k, p in zip(keys[:50], want))


def phased_fasta(ds, window_len):
    import microphaser_amd as m
    try:
        return ds.phase(window_len=window_len).fasta
    except m.MicrophaserError:   # a gene the reference would panic on: phase gene by gene and leave it out
        parts = []
        for g in range(ds.num_genes):
            try:
                b = ds.batch(window_len=window_len, gene_lo=g, gene_hi=g + 1)
                b.run()
                parts.append(b.results().fasta)
            except m.MicrophaserError:
                pass
        return b"".join(parts)


@pytest.mark.parametrize("L", [12, 13, 15, 25])
def test_gpu_build_reference_at_long_peptide_lengths_matches_oracle(ctx, tmp_path, L):
    import microphaser_amd as m
    fa = tmp_path / "tumor.fa"
    fa.write_bytes(phased_fasta(ctx.synth(77, 30), 3 * L))
    assert fa.read_bytes().count(b">") > 1000
    out = tmp_path / "o.bin"
    r = subprocess.run([ORACLE_CLI, "build_reference", "-r", str(fa), "-l", str(L), "-o", str(out)], capture_output=True, check=True)
    pep = ctx.build_reference(str(fa), L)
    assert pep.fasta == r.stdout
    want = m.decode_bincode_set(out.read_bytes())
    assert m.decode_bincode_set(pep.binary) == want and len(want) > 1000
    assert pep.keys == sorted(set(pep.keys)) and len(pep.keys) == len(want)
    assert m.keys_to_bincode(pep.keys, L) == pep.binary
    assert pep.key_words == (1 if L <= 12 else 2)
    assert pep.keys_np.shape == ((len(want),) if L <= 12 else (len(want), 2))


def oracle_filter(tmp_path, info, ref_bin, L, tag):
    r = subprocess.run([ORACLE_CLI, "filter", "-r", str(ref_bin), "-l", str(L), "-t", str(info), "-o", str(tmp_path / (tag + ".tsv")),
                        "-n", str(tmp_path / (tag + ".normal.fa")), "-s", str(tmp_path / (tag + ".removed.tsv")),
                        "-p", str(tmp_path / (tag + ".removed.fa"))], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    return (r.stdout, (tmp_path / (tag + ".normal.fa")).read_bytes(), (tmp_path / (tag + ".tsv")).read_bytes(),
            (tmp_path / (tag + ".removed.tsv")).read_bytes(), (tmp_path / (tag + ".removed.fa")).read_bytes())


def test_gpu_config_e_at_15_mers_matches_oracle(ctx, tmp_path):
    """Config E for MHC class II: `normal -w 45` -> `build_reference -l 15` -> `somatic -w 45` -> `filter -l 15`, every stage on the
    GPU and compared with the oracle on the same bytes; the filter through the files (mp_filter) and through the peptidome handle
    (mp_filter_peptides); kept and removed peptides both present, so membership hits in two-word keys are exercised. Then the CLI."""
    import microphaser_amd as m
    L, W = 15, 45
    ds = ctx.synth(303, 30, indel_rate=0.03)

    def oracle_synth(mode):   # the oracle's `normal` / `somatic` on the same exome, in memory
        prefix = str(tmp_path / mode)
        r = subprocess.run([ORACLE_CLI, "synth", "--mode", mode, "--seed", "303", "--transcripts", "30", "--indel-rate", "0.03",
                            "--window-len", str(W), "--skip-panics", "--prefix", prefix], capture_output=True, check=True)
        assert json.loads(r.stdout)["skipped"] == []
        return {e: open(prefix + "." + e, "rb").read() for e in ("fa", "normal.fa", "tsv")}

    # normal
    nres = ds.phase(window_len=W, mode=m.MODE_NORMAL)
    exp = oracle_synth("normal")
    assert (nres.fasta, nres.tsv) == (exp["fa"], exp["tsv"]) and nres.fasta.count(b">") > 10000
    normal_fa = tmp_path / "normal.fa"
    normal_fa.write_bytes(nres.fasta)
    # build_reference
    pep = ctx.build_reference(str(normal_fa), L)
    ref_bin = tmp_path / "reference.binary"
    r = subprocess.run([ORACLE_CLI, "build_reference", "-r", str(normal_fa), "-l", str(L), "-o", str(ref_bin)], capture_output=True, check=True)
    assert pep.fasta == r.stdout
    assert m.decode_bincode_set(pep.binary) == m.decode_bincode_set(ref_bin.read_bytes())
    assert pep.key_words == 2 and pep.keys == sorted(set(pep.keys))
    # somatic
    sres = ds.phase(window_len=W)
    exp = oracle_synth("somatic")
    assert (sres.fasta, sres.normal_fasta, sres.tsv) == (exp["fa"], exp["normal.fa"], exp["tsv"])
    info = tmp_path / "info.tsv"
    info.write_bytes(sres.tsv)
    assert sres.tsv.count(b"\n") > 5000
    # filter: files, then the peptidome handle
    want = oracle_filter(tmp_path, info, ref_bin, L, "o")
    streams = lambda f: (f.fasta, f.normal_fasta, f.tsv, f.removed_tsv, f.removed_fasta)
    f = ctx.filter(str(info), str(ref_bin), L)
    assert streams(f) == want
    assert f.kept > 100 and f.removed > 100
    assert streams(ctx.filter(sres.tsv, pep)) == want
    # the CLI on files
    cli = m.CLI_PATH
    r = subprocess.run([cli, "build_reference", "-r", str(normal_fa), "-l", str(L), "-o", str(tmp_path / "cli.bin")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == pep.fasta
    assert m.decode_bincode_set((tmp_path / "cli.bin").read_bytes()) == m.decode_bincode_set(ref_bin.read_bytes())
    r = subprocess.run([cli, "filter", "-r", str(tmp_path / "cli.bin"), "-l", str(L), "-t", str(info), "-o", str(tmp_path / "c.tsv"),
                        "-n", str(tmp_path / "c.normal.fa"), "-s", str(tmp_path / "c.removed.tsv"), "-p", str(tmp_path / "c.removed.fa")],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    got = (r.stdout, (tmp_path / "c.normal.fa").read_bytes(), (tmp_path / "c.tsv").read_bytes(), (tmp_path / "c.removed.tsv").read_bytes(),
           (tmp_path / "c.removed.fa").read_bytes())
    assert got == want


def test_gpu_config_e_rank_at_15_mers(ctx):
    """pipeline.config_e_rank(peptide_len=15) on one rank: the two-word peptidome flows through union_keys and mp_filter_peptides."""
    import microphaser_amd as m
    from microphaser_amd.pipeline import config_e_rank
    ds = ctx.synth(303, 30, indel_rate=0.03)
    genes = list(range(ds.num_genes))
    merged, peptidome, filtered = config_e_rank(ctx, ds, genes, genes, peptide_len=15)
    assert peptidome.key_words == 2 and peptidome.keys_np.shape[1] == 2
    f = ctx.filter(merged["tsv"], peptidome.binary, 15)
    assert (filtered.fasta, filtered.tsv, filtered.removed_tsv) == (f.fasta, f.tsv, f.removed_tsv)
    assert filtered.kept > 100 and filtered.removed > 100
