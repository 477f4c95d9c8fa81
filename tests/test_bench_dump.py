"""bench.py --dump-outputs on the CPU: dump_outputs() writes what a batch's caller receives (window count, the three streams) as
float .npy files that pin the whole output, on results consumed from a committed device dump (tests/test_consumer_replay.py)."""
import os
import subprocess
import sys
import zlib

import numpy as np

from conftest import ROOT
from test_consumer_replay import CASES, unpack


def test_dump_outputs_pins_every_byte_of_the_streams(built, tmp_path):
    import microphaser_amd as m
    sys.path.insert(0, ROOT)
    import bench
    case = next(c for c in CASES if c["name"] == "somatic_indels")
    ctx = m.Context(-1)
    ds = ctx.synth(case["seed"], case["transcripts"], case["depth"], case["spacing"], indel_rate=case["indel_rate"],
                   multiallelic_rate=case["multiallelic_rate"], softmask_rate=case["softmask_rate"], mate_rate=case["mate_rate"])
    res = ds.batch(window_len=case["window_len"]).results_from_dump(unpack(case["name"], tmp_path))
    got = {}
    for run in ("a", "b"):
        bench.dump_outputs(res, str(tmp_path / run), threads=2 if run == "a" else 1)
        got[run] = {f[:-4]: np.load(str(tmp_path / run / f)) for f in os.listdir(str(tmp_path / run))}
    a = got["a"]
    assert sorted(a) == sorted(got["b"]) and all(np.array_equal(a[k], got["b"][k]) for k in a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(str(tmp_path / "a" / (k + ".npy"))) for k in a) < 64 << 20
    assert a["windows"].tolist() == [res.windows] and res.windows > 1000
    n_genes = ds.num_genes
    genes = [int(g) for g in a["sample_genes"]]
    assert len(genes) == min(bench.DUMP_SAMPLE_GENES, n_genes) and genes == sorted(set(genes))
    for name in bench.DUMP_STREAMS:
        data = getattr(res, name)
        off = [int(x) for x in a[name + "_gene_offsets"]]
        assert len(off) == n_genes + 1 and off[-1] <= len(data)
        cuts = [0] + off + [len(data)]
        assert a[name + "_crc32"].tolist() == [zlib.crc32(data[cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1)]
        sample = b"".join(data[off[g]:off[g + 1]][:bench.DUMP_SAMPLE_BYTES] for g in genes)
        assert len(sample) > 0 and a[name + "_sample"].astype(np.uint8).tobytes() == sample


def test_bench_has_the_full_and_dump_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, check=True)
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr
