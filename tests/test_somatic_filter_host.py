"""`somatic` -> `filter` in one step (mp_batch_filter / mp_batch_filter_binary, `somatic --filter-reference`): what can be checked
without a GPU - the symbols, the loud failures before any device work, the CLI's argument errors and the new kernel's resource use."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT, SOMATIC_FIXTURES

LLVM = "/opt/rocm/lib/llvm/bin"


def test_batch_filter_symbols_are_exported_and_declared(built):
    import microphaser_amd as m
    so = ctypes.CDLL(m.LIB_PATH)
    for name in ("mp_batch_filter", "mp_batch_filter_binary"):
        assert name in m.C_ABI_SYMBOLS
        assert hasattr(so, name)
    hdr = open(os.path.join(ROOT, "include", "microphaser_hip.h")).read()
    assert re.search(r"int mp_batch_filter\(mp_ctx\* ctx, mp_batch\* batch, const mp_peptides\* reference, uint32_t streams, "
                     r"mp_results\*\* results,\s+mp_filtered\*\* out\);", hdr)
    assert re.search(r"int mp_batch_filter_binary\(mp_ctx\* ctx, mp_batch\* batch, const char\* reference_binary, size_t len, "
                     r"uint32_t peptide_len, uint32_t streams,\s+mp_results\*\* results, mp_filtered\*\* out\);", hdr)


def _reference_binary():
    return open(os.path.join(GOLDEN, "test_filter", "reference.binary"), "rb").read()


def test_batch_filter_on_a_host_only_context_fails_loudly(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    b = ctx.synth(5, 4).batch(mode=m.MODE_SOMATIC)
    pep = ctx.peptides_union([], 9)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        b.filter(_reference_binary(), 9)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        b.filter(pep, streams=m.STREAM_TSV)


def test_batch_filter_refuses_a_normal_batch(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    b = ctx.synth(5, 4).batch(mode=m.MODE_NORMAL)
    with pytest.raises(m.MicrophaserError, match="normal batch"):
        b.filter(_reference_binary(), 9)
    with pytest.raises(m.MicrophaserError, match="normal batch"):
        b.filter(ctx.peptides_union([], 9))


@pytest.mark.parametrize("L", [0, 26])
def test_batch_filter_binary_refuses_a_peptide_length_outside_1_to_25(built, L):
    import microphaser_amd as m
    ctx = m.Context(-1)
    b = ctx.synth(5, 4).batch(mode=m.MODE_SOMATIC)
    with pytest.raises(m.MicrophaserError, match="1..25"):
        b.filter(_reference_binary(), L)


def _cli(args, cwd):
    import microphaser_amd as m
    d, bam, vcf, gtf, fa, _stem = SOMATIC_FIXTURES["test_forward"]
    base = os.path.join(GOLDEN, d)
    with open(os.path.join(base, gtf), "rb") as g:
        return subprocess.run([m.CLI_PATH, args[0], os.path.join(base, bam), "-r", os.path.join(base, fa), "-b", os.path.join(base, vcf)] + args[1:],
                              stdin=g, capture_output=True, cwd=str(cwd), timeout=120)


REF = os.path.join(GOLDEN, "test_filter", "reference.binary")


@pytest.mark.parametrize("args,message", [
    (["normal", "--filter-reference", REF], "`somatic` option"),
    (["normal", "--filter-reference", REF, "-l", "9"], "`somatic` option"),
    (["somatic", "-l", "9"], "needs --filter-reference"),
    (["somatic", "-l9"], "needs --filter-reference"),
    (["somatic", "--peptide-length", "9"], "needs --filter-reference"),
    (["somatic", "--filter-reference", REF, "--devices", "0,1"], "more than one"),
    (["somatic", "--filter-reference", REF, "-l", "0"], "must be 1..25"),
    (["somatic", "--filter-reference", REF, "-l", "26"], "must be 1..25"),
    (["somatic", "-s", "r.tsv"], "need --filter-reference"),
    (["somatic", "--filtered-tsv", "f.tsv"], "need --filter-reference"),
    (["somatic", "--filter-reference", "no_such_reference.bin"], "cannot open"),
])
def test_cli_filter_argument_errors_exit_1_before_any_gpu_work(built, tmp_path, args, message):
    r = _cli(args, tmp_path)
    assert r.returncode == 1
    assert message in r.stderr.decode()
    assert r.stdout == b""
    assert os.listdir(str(tmp_path)) == []   # nothing written


@pytest.mark.parametrize("args,message", [
    (["normal", "-l", "9"], "needs --peptidome-output"),
    (["somatic", "--peptidome-output", "p.bin"], "`normal` option"),
])
def test_cli_peptidome_messages_stay_as_they_were(built, tmp_path, args, message):
    r = _cli(args, tmp_path)
    assert r.returncode == 1 and message in r.stderr.decode() and os.listdir(str(tmp_path)) == []


def test_row_source_translation_kernel_uses_no_scratch(built, tmp_path):
    """Both instantiations of k5_translate_row_sources (u64 and unsigned __int128 keys) keep the rolling key in registers, as K5 does."""
    import microphaser_amd as m
    lib = str(tmp_path / "lib.so")
    shutil.copy(m.LIB_PATH, lib)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", lib], check=True, capture_output=True, cwd=str(tmp_path))
    objs = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert objs, os.listdir(tmp_path)
    seen = {}
    for f in objs:
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / f)], check=True, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if name and scratch and name.group(1).startswith("_ZN2mp24k5_translate_row_sources"):
                seen[name.group(1)] = int(scratch.group(1))
    assert len(seen) == 2, sorted(seen)
    assert all(v == 0 for v in seen.values()), seen
