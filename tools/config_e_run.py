#!/usr/bin/env python3
"""BASELINE.json config E at full size on ONE GPU, stage by stage, with wall times (measurement tool):

  normal (germline + somatic calls, every haplotype of every window) -> build_reference -l L -> somatic -> filter

on the synthetic 20k-transcript exome (seed 2020, per-gene random streams). `normal` emits every window (~4x the text of `somatic`),
so the exome is walked in gene chunks - exactly what the ranks of a multi-GPU run do with their shards (microphaser_amd/pipeline.py):
per chunk normal -> FASTA -> build_reference -> sorted distinct keys; the chunks' key arrays are merged by mp_peptides_union; then
`somatic` per chunk, shards merged by gene, and one `filter` over the merged TSV.

  python tools/config_e_run.py [--transcripts 20000] [--chunks 8] [--peptide-len 9] [--fused-peptidome] [--fused-filter [--somatic-chunks N]]
                                [--out config_e.json]

(--fused-peptidome: per chunk `normal` -> Batch.peptidome, the records translated where they lie in device memory, no nucleotide
FASTA; normal_s then includes the peptidome, build_reference_s is 0, and wall_s["fused_peptidome_s"] is the peptidome call alone)

(--fused-filter: `somatic` as ONE batch over all genes, then Batch.filter against the peptidome - the rows filtered where their windows
lie in device memory, no info.tsv; somatic_s then includes the filter, filter_s is 0, and wall_s["fused_filter_s"] is the filter call
alone. --skip-panics, which phases gene by gene, is refused: a gene left out would not be what the filter of the exome sees)

(--somatic-chunks N with --fused-filter: the tumor half in N gene chunks on pipeline.filter_chunked's overlapped two-context schedule,
every chunk added to one filter stream; somatic_s then covers the chunks' runs, adds and the stream's finish; default: one batch)

stats["md5"] holds the md5 of the filter's five streams (fasta, normal_fasta, tsv, removed_tsv, removed_fasta), taken after the timing.

(--peptide-len L: windows of 3L nt in `normal` and `somatic`; 13..25 are the MHC class II lengths, with two-word peptide keys)
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import microphaser_amd as m
from microphaser_amd.pipeline import filter_chunked
from microphaser_amd.shard import merge_by_gene, shard_of


def phased(ds, genes, window_len, mode, streams, skip_panics, skipped, take=None):
    """(genes, RunStats, Results) of one batch of `genes`; with skip_panics, a batch that holds a gene the reference would panic on
    (the oracle's --skip-panics) is phased gene by gene instead, that gene left out and recorded in `skipped`. take(batch): what to
    return in place of the Results (default: batch.results(streams))."""
    take = take or (lambda b: b.results(streams))
    try:
        b = ds.batch_genes(genes, window_len=window_len, mode=mode)
        st = b.run()
        return [(genes, st, take(b))]
    except m.MicrophaserError as e:
        if not (skip_panics and str(e).startswith("reference would panic")):
            raise
    out = []
    for g in genes:
        try:
            b = ds.batch_genes([g], window_len=window_len, mode=mode)
            st = b.run()
            out.append(([g], st, take(b)))
        except m.MicrophaserError as e:
            if not str(e).startswith("reference would panic"):
                raise
            skipped.append(g)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--transcripts", type=int, default=20000)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--peptide-len", type=int, default=9)
    ap.add_argument("--skip-panics", action="store_true", help="leave out genes the reference would panic on (phased gene by gene)")
    ap.add_argument("--fused-peptidome", action="store_true", help="normal -> peptidome on the device (Batch.peptidome), no nucleotide FASTA")
    ap.add_argument("--fused-filter", action="store_true", help="somatic -> filter on the device (Batch.filter), no info.tsv")
    ap.add_argument("--somatic-chunks", type=int, default=0,
                    help="with --fused-filter: the tumor half in this many gene chunks, all added to one filter stream (default: one batch)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.somatic_chunks and not a.fused_filter:
        ap.error("--somatic-chunks is a --fused-filter option")
    if a.fused_filter and a.skip_panics:
        ap.error("--fused-filter phases all genes as one batch (the filter's row stream runs over all of them); --skip-panics phases gene by gene")
    L = a.peptide_len
    ctx = m.Context(0)
    t = {}
    t0 = time.perf_counter()
    ds = ctx.synth(2020, a.transcripts, 30.0, 5.4, gene_streams=True)
    t["generate_s"] = time.perf_counter() - t0
    n = ds.num_genes
    cuts = [n * k // a.chunks for k in range(a.chunks + 1)]
    stats = dict(normal_windows=0, normal_fasta_bytes=0, normal_tsv_bytes=0, k2n_ms=0.0, k3_ms=0.0, k3b_ms=0.0, k1_ms=0.0, peptide_windows=0)
    key_arrays = []
    skipped = {"normal": [], "somatic": []}
    t_normal = t_build = t_fused = 0.0
    for c in range(a.chunks):
        genes = list(range(cuts[c], cuts[c + 1]))
        t0 = time.perf_counter()
        if a.fused_peptidome:
            def fused(b):
                tp = time.perf_counter()
                pep, _ = b.peptidome(L)
                return pep, time.perf_counter() - tp
            for _g, st, (pep, dt) in phased(ds, genes, 3 * L, m.MODE_NORMAL, 0, a.skip_panics, skipped["normal"], take=fused):
                stats["k1_ms"] += st.k1_ms; stats["k2n_ms"] += st.k2seq_ms; stats["k3_ms"] += st.k3_ms; stats["k3b_ms"] += st.k3b_ms
                stats["peptide_windows"] += pep.count
                key_arrays.append(pep.keys_np)
                t_fused += dt
                pep.close()
            t_normal += time.perf_counter() - t0
            print("chunk %d/%d: normal + fused peptidome %.1f s so far" % (c + 1, a.chunks, t_normal), flush=True)
            continue
        parts = []
        for _g, st, res in phased(ds, genes, 3 * L, m.MODE_NORMAL, m.STREAM_FASTA, a.skip_panics, skipped["normal"]):
            parts.append(res.fasta)           # build_reference reads the FASTA only
            stats["normal_windows"] += res.windows
            stats["normal_tsv_bytes"] += res.size("tsv")
            stats["k1_ms"] += st.k1_ms; stats["k2n_ms"] += st.k2seq_ms; stats["k3_ms"] += st.k3_ms; stats["k3b_ms"] += st.k3b_ms
            res.close()
        fa = parts[0] if len(parts) == 1 else b"".join(parts)
        del parts
        stats["normal_fasta_bytes"] += len(fa)
        t_normal += time.perf_counter() - t0
        t0 = time.perf_counter()
        pep = ctx.peptidome(fa, L)            # keys only: nobody reads the translated FASTA in this pipeline
        stats["peptide_windows"] += pep.count
        key_arrays.append(pep.keys_np)
        del fa, pep
        t_build += time.perf_counter() - t0
        print("chunk %d/%d: normal %.1f s, build_reference %.1f s so far" % (c + 1, a.chunks, t_normal, t_build), flush=True)
    t["normal_s"], t["build_reference_s"] = t_normal, t_build
    if a.fused_peptidome:
        t["fused_peptidome_s"] = t_fused
    t0 = time.perf_counter()
    peptidome = ctx.peptides_union(key_arrays, L)
    t["peptides_union_s"] = time.perf_counter() - t0
    stats["peptidome_size"] = int(peptidome.keys_np.size)
    if a.fused_filter and a.somatic_chunks:
        ctx2 = m.Context(0)   # the second context of the overlapped schedule (created outside the timing, as ctx is)
        t0 = time.perf_counter()
        f, _ = filter_chunked(ds, peptidome, n_chunks=a.somatic_chunks, peptide_len=L, contexts=[ctx, ctx2])
        t["somatic_s"], t["filter_s"] = time.perf_counter() - t0, 0.0
        ctx2.close()
        stats["somatic_tsv_rows"] = f.rows
    elif a.fused_filter:
        t0 = time.perf_counter()
        b = ds.batch(window_len=3 * L)
        b.run()
        tf = time.perf_counter()
        f, _ = b.filter(peptidome)                  # the rows' windows are read in device memory: no TSV text
        t["fused_filter_s"] = time.perf_counter() - tf
        t["somatic_s"], t["filter_s"] = time.perf_counter() - t0, 0.0
        b.close()
        stats["somatic_tsv_rows"] = f.rows
    else:
        t0 = time.perf_counter()
        shards = []
        som_windows = 0
        for c in range(a.chunks):
            genes = list(range(cuts[c], cuts[c + 1]))
            # windows of L codons: a 27-nt window holds no 15-mer
            for gs, _st, r in phased(ds, genes, 3 * L, m.MODE_SOMATIC, m.STREAM_ALL, a.skip_panics, skipped["somatic"]):
                som_windows += r.windows
                shards.append(shard_of(r, gs))
                r.close()
        merged = merge_by_gene(shards)
        del shards
        t["somatic_s"] = time.perf_counter() - t0
        stats["somatic_windows"] = som_windows
        stats["somatic_tsv_rows"] = merged["tsv"].count(b"\n") - 1
        t0 = time.perf_counter()
        f = ctx.filter(merged["tsv"], peptidome)        # the peptidome handle: its keys go to the GPU as they are
        t["filter_s"] = time.perf_counter() - t0
    stats["md5"] = {k: hashlib.md5(getattr(f, k)).hexdigest() for k in ("fasta", "normal_fasta", "tsv", "removed_tsv", "removed_fasta")}
    stats.update(filter_rows=f.rows, filter_kept=f.kept, filter_removed=f.removed, filter_groups=f.groups, skipped_genes=skipped)
    t["total_s"] = sum(v for k, v in t.items() if k not in ("generate_s", "fused_peptidome_s", "fused_filter_s"))   # (inside normal_s / somatic_s)
    out = {"config": "E: normal + build_reference -l %d + somatic + filter, %d transcripts, %d gene chunks, one MI355X%s" %
                     (L, a.transcripts, a.chunks, (", fused normal -> peptidome" if a.fused_peptidome else "") +
                                                        (", fused somatic -> filter" if a.fused_filter else "") +
                                                        (" over %d streamed gene chunks" % a.somatic_chunks if a.somatic_chunks else "")),
           "wall_s": t, "stats": stats}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
