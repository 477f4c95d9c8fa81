"""Peptide lengths 13..25 (MHC class II) on the host: two-word keys in the multi-rank peptidome union (mp_peptides_union, the gloo
all-gather of shard.allgather_keys) and the scratch-free K4 / K5 instantiations of both key widths. No GPU needed."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_kernel_resources import LLVM


def as_words(keys):
    """Python int keys -> (n, 2) uint64 array, columns [lo, hi] (the C ABI's two-word layout)."""
    a = np.zeros((len(keys), 2), dtype=np.uint64)
    a[:, 0] = np.fromiter((k & (2 ** 64 - 1) for k in keys), dtype=np.uint64, count=len(keys))
    a[:, 1] = np.fromiter((k >> 64 for k in keys), dtype=np.uint64, count=len(keys))
    return a


def random_keys(rng, n, L):
    """n distinct sorted keys of L residues (5L bits), as Python ints."""
    hi = rng.integers(0, 1 << (5 * L - 64), size=n, dtype=np.uint64)
    lo = rng.integers(0, 2 ** 64 - 1, size=n, dtype=np.uint64, endpoint=True)
    return sorted({(int(h) << 64) | int(l) for h, l in zip(hi, lo)})


@pytest.mark.parametrize("L", [13, 15, 25])
def test_two_word_union_equals_the_python_set_union(built, L):
    import microphaser_amd as m
    ctx = m.Context(-1)
    rng = np.random.default_rng(L)
    sets = [random_keys(rng, n, L) for n in (300000, 180000, 7, 90000)]
    sets.append(sets[0][::3])                     # overlaps the first array
    sets.append(sets[1][5:40000])
    arrs = [as_words(s) for s in sets] + [np.zeros((0, 2), dtype=np.uint64)]
    u = ctx.peptides_union(arrs, L)
    want = sorted(set().union(*map(set, sets)))
    assert u.key_words == 2 and u.keys_np.shape == (len(want), 2) and u.keys_np.dtype == np.uint64
    assert u.keys == want
    assert np.array_equal(u.keys_np, as_words(want))
    assert all(k < 1 << (5 * L) for k in u.keys[-3:])


@pytest.mark.parametrize("L", [13, 15, 25])
def test_two_word_keys_order_by_the_high_word_first(built, L):
    import microphaser_amd as m
    ctx = m.Context(-1)
    a = [(1 << 64) | 5, (1 << 64) | (1 << 63), (2 << 64) | 0, (2 << 64) | 3]   # differ only in the low word, then only in the high word
    b = [3, (1 << 64) | 4, (1 << 64) | (1 << 63), (2 << 64) | 1]
    u = ctx.peptides_union([as_words(a), as_words(b)], L)
    assert u.keys == sorted(set(a) | set(b))
    assert u.keys_np[:, 1].tolist() == [k >> 64 for k in u.keys]
    assert u.binary == m.keys_to_bincode(u.keys, L)
    assert m.decode_bincode_set(u.binary) == {m.key_to_peptide(k, L).encode() for k in u.keys}
    assert all(len(p) == L for p in m.decode_bincode_set(u.binary))


@pytest.mark.parametrize("bad", [[(2 << 64) | 1, (1 << 64) | 7],     # high word descends, low word ascends
                                 [(1 << 64) | 7, (1 << 64) | 6],     # same high word, low word descends
                                 [(1 << 64) | 7, (1 << 64) | 7]])    # a repeated key
def test_two_word_union_refuses_unsorted_arrays_in_either_word(built, bad):
    import microphaser_amd as m
    ctx = m.Context(-1)
    with pytest.raises(m.MicrophaserError, match="sorted and distinct"):
        ctx.peptides_union([as_words(bad)], 15)
    long_bad = as_words(random_keys(np.random.default_rng(3), 200000, 15))
    long_bad[150000] = long_bad[149999]
    with pytest.raises(m.MicrophaserError, match="sorted and distinct"):
        ctx.peptides_union([as_words([5, 9]), long_bad], 15)


def test_peptide_length_limits(built):
    import microphaser_amd as m
    ctx = m.Context(-1)
    for L in (0, 26):
        with pytest.raises(m.MicrophaserError, match=r"1\.\.25"):
            ctx.peptides_union([as_words([1, 2])], L)
        assert m.lib().mp_key_words(L) == 0
    assert [m.lib().mp_key_words(L) for L in (1, 9, 12, 13, 15, 25)] == [1, 1, 1, 2, 2, 2]
    with pytest.raises(ValueError, match="two-word"):
        ctx.peptides_union([np.array([1, 2], dtype=np.uint64)], 15)
    # 12-mers keep the one-word layout
    u = ctx.peptides_union([np.array([3, 1 << 59], dtype=np.uint64), np.array([4], dtype=np.uint64)], 12)
    assert u.key_words == 1 and u.keys_np.ndim == 1 and u.keys == [3, 4, 1 << 59]
    assert u.binary == m.keys_to_bincode(u.keys, 12)


UNION_WORKER = r'''
import json, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch.distributed as dist
import microphaser_amd as m
from microphaser_amd.shard import allgather_keys, union_keys
dist.init_process_group(backend="gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=2)
rank = dist.get_rank()
keys = json.load(open(%(tmp)r + "/keys%%d.json" %% rank))
local = np.array([[k & (2 ** 64 - 1), k >> 64] for k in keys], dtype=np.uint64).reshape(-1, 2)
got = allgather_keys(local, dist)
assert [a.shape[1] for a in got] == [2, 2] and [a.shape[0] for a in got] == %(sizes)r
assert np.array_equal(got[rank], local)
u = union_keys(m.Context(-1), local, 15, dist)         # tensors over gloo, merged by mp_peptides_union
open(%(tmp)r + "/union%%d.json" %% rank, "w").write(json.dumps({"keys": [str(k) for k in u.keys], "words": u.key_words,
                                                              "binary_ok": u.binary == m.keys_to_bincode(u.keys, 15)}))
dist.barrier()
dist.destroy_process_group()
'''


def test_two_rank_gloo_union_of_two_word_keys(built, tmp_path):
    import microphaser_amd as m
    rng = np.random.default_rng(11)
    k0 = random_keys(rng, 120000, 15)
    k1 = sorted(set(random_keys(rng, 70000, 15)) | {k0[17], k0[18]})     # two keys on both ranks
    (tmp_path / "keys0.json").write_text(json.dumps(k0))
    (tmp_path / "keys1.json").write_text(json.dumps(k1))
    single = m.Context(-1).peptides_union([as_words(k0), as_words(k1)], 15)
    port = 33500 + (os.getpid() % 2000)
    script = tmp_path / "uworker.py"
    script.write_text(UNION_WORKER % dict(root=ROOT, port=port, tmp=str(tmp_path), sizes=[len(k0), len(k1)]))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.PIPE) for r in range(2)]
    for p in procs:
        out, err = p.communicate(timeout=240)
        assert p.returncode == 0, err.decode()[-2000:]
    assert single.keys == sorted(set(k0) | set(k1))
    for r in range(2):
        got = json.loads((tmp_path / ("union%d.json" % r)).read_text())
        assert [int(k) for k in got["keys"]] == single.keys and got["words"] == 2 and got["binary_ok"]


def test_peptide_kernels_of_both_key_widths_use_no_scratch(built, tmp_path):
    """K4 (k4_translate) and K5 (k5_translate_records), u64 and 128-bit keys: a rolling 128-bit key must stay in registers."""
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
            if name and scratch:
                seen[name.group(1)] = int(scratch.group(1))
    # template arguments in the mangled names: m = unsigned long (uint64_t), o = unsigned __int128
    want = ["_ZN2mp12k4_translateImEEv", "_ZN2mp12k4_translateIoEEv", "_ZN2mp20k5_translate_recordsImEEv", "_ZN2mp20k5_translate_recordsIoEEv"]
    found = {w: [k for k in seen if k.startswith(w)] for w in want}
    assert all(len(v) == 1 for v in found.values()), found
    assert {v[0]: seen[v[0]] for v in found.values()} == {v[0]: 0 for v in found.values()}
