"""bench.dump_outputs (--dump-outputs) on synthetic records, without a GPU: one float64 array per record field, and a fixed
seeded sample of humeri when the whole set would exceed the size limit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from shoulder_amd import _lib  # noqa: E402


def _records(n, rows=16):
    rec = np.zeros(n, dtype=_lib.record_dtype(rows))
    rng = np.random.default_rng(5)
    for f in rec.dtype.names:
        v = rec[f]
        rec[f] = rng.integers(-5, 5, v.shape) if v.dtype.kind == "i" else rng.standard_normal(v.shape)
    return rec


def test_every_field_as_float64(tmp_path):
    rec = _records(6)
    idx = bench.dump_outputs(str(tmp_path), rec)
    assert list(idx) == list(range(6)) and not (tmp_path / "humerus_index.npy").exists()
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f + ".npy" for f in rec.dtype.names)
    assert bench.DUMP_MAX_BYTES == 64_000_000
    for f in rec.dtype.names:
        v = np.load(tmp_path / (f + ".npy"))
        assert v.dtype == np.float64 and np.array_equal(v, rec[f].astype(np.float64)), f


def test_sample_above_the_limit(tmp_path):
    rec = _records(40)
    per = 8 * sum(int(np.prod(rec.dtype.fields[f][0].shape)) for f in rec.dtype.names)
    limit = 10 * per + bench.NPY_HEADER_BYTES * (len(rec.dtype.names) + 1) + 100
    idx = bench.dump_outputs(str(tmp_path), rec, max_bytes=limit)
    assert len(idx) == 10 and list(idx) == sorted(set(idx)) and idx.max() < 40
    assert sum(os.path.getsize(p) for p in tmp_path.iterdir()) <= limit      # (the files as written, headers included)
    assert np.array_equal(np.load(tmp_path / "humerus_index.npy"), idx.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "canal_axis.npy"), rec["canal_axis"][idx])
    again = bench.dump_outputs(str(tmp_path / "again"), rec, max_bytes=limit)
    assert np.array_equal(again, idx)                       # the same sample every time
    bench.dump_outputs(str(tmp_path), rec[:3], max_bytes=limit)
    assert not (tmp_path / "humerus_index.npy").exists()    # no stale index beside an unsampled dump


def test_default_cap_counts_the_files_as_written(tmp_path):
    """Records of the benchmark's wire format (2 560 anatomic-neck rows), a few more humeri than fit in 64 MB: the sampled dump's
    files, headers included, stay within DUMP_MAX_BYTES (decimal)."""
    rec = np.zeros(920, dtype=_lib.record_dtype(2560))
    rec["n_anp"] = np.arange(920)
    idx = bench.dump_outputs(str(tmp_path), rec)
    assert 900 < len(idx) < 920 and (tmp_path / "humerus_index.npy").exists()
    assert sum(os.path.getsize(p) for p in tmp_path.iterdir()) <= 64_000_000
    assert np.array_equal(np.load(tmp_path / "n_anp.npy"), idx.astype(np.float64))
