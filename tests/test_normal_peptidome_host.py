"""`normal` -> peptidome in one step (mp_batch_peptidome, `normal --peptidome-output`): what can be checked without a GPU - the
symbol, the loud failures before any device work, the CLI's argument errors and the new kernel's resource use."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, NORMAL_FIXTURES, ROOT

LLVM = "/opt/rocm/lib/llvm/bin"


def test_batch_peptidome_is_exported_and_declared(built):
    import microphaser_amd as m
    assert "mp_batch_peptidome" in m.C_ABI_SYMBOLS
    assert hasattr(ctypes.CDLL(m.LIB_PATH), "mp_batch_peptidome")
    hdr = open(os.path.join(ROOT, "include", "microphaser_hip.h")).read()
    assert re.search(r"int mp_batch_peptidome\(mp_ctx\* ctx, mp_batch\* batch, uint32_t peptide_len, uint32_t streams, mp_results\*\* results,\s+"
                     r"mp_peptides\*\* out\);", hdr)


def test_batch_peptidome_on_a_host_only_context_fails_loudly(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    b = ctx.synth(5, 4).batch(mode=m.MODE_NORMAL)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        b.peptidome(9)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        b.peptidome(9, m.STREAM_FASTA)


def test_batch_peptidome_refuses_a_somatic_batch(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    b = ctx.synth(5, 4).batch(mode=m.MODE_SOMATIC)
    with pytest.raises(m.MicrophaserError, match="somatic batch"):
        b.peptidome(9)


@pytest.mark.parametrize("L", [0, 26])
def test_batch_peptidome_refuses_a_peptide_length_outside_1_to_25(built, L):
    import microphaser_amd as m
    ctx = m.Context(-1)
    b = ctx.synth(5, 4).batch(mode=m.MODE_NORMAL)
    with pytest.raises(m.MicrophaserError, match="1..25"):
        b.peptidome(L)


def _cli(args, cwd):
    import microphaser_amd as m
    bam, vcf, gtf, fa, _exp = NORMAL_FIXTURES["splice_forward_test"]
    d = os.path.join(GOLDEN, "splice_forward_test")
    with open(os.path.join(d, gtf), "rb") as g:
        return subprocess.run([m.CLI_PATH, args[0], os.path.join(d, bam), "-r", os.path.join(d, fa), "-b", os.path.join(d, vcf)] + args[1:],
                              stdin=g, capture_output=True, cwd=str(cwd), timeout=120)


@pytest.mark.parametrize("args,message", [
    (["normal", "--peptidome-output", "p.bin", "-l", "0"], "must be 1..25"),
    (["normal", "--peptidome-output", "p.bin", "-l", "26"], "must be 1..25"),
    (["normal", "--peptidome-output", "p.bin", "--peptide-length", "x"], "must be 1..25"),
    (["normal", "-l", "9"], "needs --peptidome-output"),
    (["normal", "-l9"], "needs --peptidome-output"),
    (["somatic", "--peptidome-output", "p.bin"], "`normal` option"),
])
def test_cli_peptidome_argument_errors_exit_1_before_any_gpu_work(built, tmp_path, args, message):
    r = _cli(args, tmp_path)
    assert r.returncode == 1
    assert message in r.stderr.decode()
    assert r.stdout == b""
    assert os.listdir(str(tmp_path)) == []   # nothing written, no TSV either


def test_source_translation_kernel_uses_no_scratch(built, tmp_path):
    """Every instantiation of k4_translate_sources (one- and two-word keys) keeps its state in registers, as K4 does."""
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
            if name and scratch and name.group(1).startswith("_ZN2mp20k4_translate_sources"):
                seen[name.group(1)] = int(scratch.group(1))
    assert len(seen) == 2, sorted(seen)   # K = uint64_t, rocprim::uint128_t
    assert all(v == 0 for v in seen.values()), seen
