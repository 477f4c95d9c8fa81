"""The filter stream (mp_filter_stream_*, FilterStream): what can be checked without a GPU - the symbols, the argument checks that
come before any device work (mode, data set, gene order, peptide length), the one-shot finish and the loud failure on a host-only
context."""
import ctypes
import os
import re

import pytest

from conftest import GOLDEN, ROOT


def _reference_binary():
    return open(os.path.join(GOLDEN, "test_filter", "reference.binary"), "rb").read()


def _stream(ctx):
    import microphaser_amd as m
    return m.FilterStream(ctx, _reference_binary(), 9)


def test_filter_stream_symbols_are_exported_and_declared(built):
    import microphaser_amd as m
    so = ctypes.CDLL(m.LIB_PATH)
    names = ("mp_filter_stream_create", "mp_filter_stream_create_binary", "mp_filter_stream_add", "mp_filter_stream_finish",
             "mp_filter_stream_free")
    for name in names:
        assert name in m.C_ABI_SYMBOLS
        assert hasattr(so, name)
    hdr = open(os.path.join(ROOT, "include", "microphaser_hip.h")).read()
    assert "typedef struct mp_filter_stream mp_filter_stream;" in hdr
    assert re.search(r"int mp_filter_stream_create\(mp_ctx\* ctx, const mp_peptides\* reference, mp_filter_stream\*\* out\);", hdr)
    assert re.search(r"int mp_filter_stream_create_binary\(mp_ctx\* ctx, const char\* reference_binary, size_t len, uint32_t peptide_len, "
                     r"mp_filter_stream\*\* out\);", hdr)
    assert re.search(r"int mp_filter_stream_add\(mp_ctx\* ctx, mp_filter_stream\* s, mp_batch\* batch, uint32_t streams, "
                     r"mp_results\*\* results\);", hdr)
    assert re.search(r"int mp_filter_stream_finish\(mp_ctx\* ctx, mp_filter_stream\* s, mp_filtered\*\* out\);", hdr)
    assert re.search(r"void mp_filter_stream_free\(mp_filter_stream\* s\);", hdr)


def test_a_correct_add_on_a_host_only_context_fails_loudly(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    ds = ctx.synth(5, 6)
    for reference in (_reference_binary(), ctx.peptides_union([], 9)):
        fs = m.FilterStream(ctx, reference, 9)
        with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
            fs.add(ds.batch(gene_hi=3))
        # the failed add ends the stream
        with pytest.raises(m.MicrophaserError, match="an earlier add on this stream failed"):
            fs.add(ds.batch(gene_lo=3))
        with pytest.raises(m.MicrophaserError, match="an earlier add on this stream failed"):
            fs.finish()
        fs.close()


def test_a_normal_batch_is_refused(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    ds = ctx.synth(5, 4)
    fs = _stream(ctx)
    with pytest.raises(m.MicrophaserError) as e:
        fs.add(ds.batch(mode=m.MODE_NORMAL))
    assert str(e.value) == ("mp_filter_stream_add: the batch is a normal batch - the filter reads the rows of a `somatic` run "
                            "(MP_MODE_SOMATIC)")
    with pytest.raises(m.MicrophaserError, match="normal batch"):
        ds.batch(mode=m.MODE_NORMAL).filter(_reference_binary(), 9)   # (the one-batch message, unchanged)


def test_batches_of_two_data_sets_are_refused(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    ds1, ds2 = ctx.synth(5, 6), ctx.synth(5, 6)
    fs = _stream(ctx)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        fs.add(ds1.batch(gene_hi=3))
    with pytest.raises(m.MicrophaserError, match="another data set than the stream's earlier batches"):
        fs.add(ds2.batch(gene_lo=3))
    with pytest.raises(m.MicrophaserError, match="another data set"):
        fs.add(ds2.batch_genes([4, 5]))


@pytest.mark.parametrize("first,second,message", [
    ((0, 3), (2, 5), "gene 2 does not come after gene 2"),       # overlapping ranges
    ((3, 6), (0, 2), "gene 0 does not come after gene 5"),       # out of order
    ((2, 4), (3, 6), "gene 3 does not come after gene 3"),
    ([1, 4], [2, 5], "gene 2 does not come after gene 4"),       # interleaved gene lists
    ([1, 4], [4], "gene 4 does not come after gene 4"),          # the same gene twice
])
def test_genes_that_do_not_come_after_the_added_ones_are_refused(built, first, second, message):
    import microphaser_amd as m
    ctx = m.Context(-1)
    ds = ctx.synth(5, 8)
    mk = lambda g: ds.batch(gene_lo=g[0], gene_hi=g[1]) if isinstance(g, tuple) else ds.batch_genes(g)
    fs = _stream(ctx)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        fs.add(mk(first))
    with pytest.raises(m.MicrophaserError) as e:
        fs.add(mk(second))
    assert message in str(e.value) and "add the batches in gene order" in str(e.value)


def test_gaps_and_empty_batches_pass_the_order_check(built):
    """A later gene range with a gap, and a batch without genes, get past the order check (to the state check of the failed stream)."""
    import microphaser_amd as m
    ctx = m.Context(-1)
    ds = ctx.synth(5, 8)
    fs = _stream(ctx)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        fs.add(ds.batch_genes([0, 2]))
    for b in (ds.batch_genes([5, 7]), ds.batch(gene_lo=8, gene_hi=8), ds.batch_genes([])):
        with pytest.raises(m.MicrophaserError, match="an earlier add on this stream failed"):
            fs.add(b)


def test_add_after_finish_is_refused(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    ds = ctx.synth(5, 4)
    fs = _stream(ctx)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        fs.finish()
    with pytest.raises(m.MicrophaserError, match="mp_filter_stream_add: the stream has been finished"):
        fs.add(ds.batch())


def test_a_stream_is_finished_once(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    fs = _stream(ctx)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        fs.finish()
    with pytest.raises(m.MicrophaserError, match="mp_filter_stream_finish: the stream has been finished already"):
        fs.finish()


@pytest.mark.parametrize("L", [0, 26])
def test_a_peptide_length_outside_1_to_25_is_refused(built, L):
    import microphaser_amd as m
    ctx = m.Context(-1)
    with pytest.raises(m.MicrophaserError, match="1..25"):
        m.FilterStream(ctx, _reference_binary(), L)



def test_a_batch_refused_by_the_argument_checks_leaves_the_stream_as_it_was(built):
    """Mode, data set and gene order are checked before the stream's state: a batch they refuse changes nothing, so the next correct
    add gets as far as the device (here: the host-only context's message, not the refusal of a failed stream)."""
    import microphaser_amd as m
    ctx = m.Context(-1)
    ds, other = ctx.synth(5, 6), ctx.synth(5, 6)
    fs = _stream(ctx)
    with pytest.raises(m.MicrophaserError, match="normal batch"):
        fs.add(ds.batch(mode=m.MODE_NORMAL))
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        fs.add(ds.batch(gene_hi=3))
    fs = _stream(ctx)
    with pytest.raises(m.MicrophaserError, match="no CPU fallback"):
        fs.add(ds.batch(gene_hi=3))
    with pytest.raises(m.MicrophaserError, match="another data set"):
        fs.add(other.batch(gene_lo=3))
    with pytest.raises(m.MicrophaserError, match="does not come after"):
        fs.add(ds.batch(gene_lo=1, gene_hi=4))


@pytest.mark.parametrize("L", [9, 15])
def test_a_peptidome_handle_reports_its_peptide_length(built, L):
    import microphaser_amd as m
    assert m.Context(-1).peptides_union([], L).peptide_len == L
