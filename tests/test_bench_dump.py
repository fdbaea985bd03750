"""CPU: bench.py --dump-outputs.  The records of the last timed step go out as one float32 / float64 array per leaf field of RESULT_DTYPE (padding left out,
values unchanged), and above the size cap as a fixed, seeded, ascending sample of the frames — the same sample on every run."""
import numpy as np

import bench
from eagle_amd import lib


def _records(n, seed=3):
    raw = np.random.default_rng(seed).integers(0, 256, n * lib.RESULT_DTYPE.itemsize, dtype=np.uint8)
    return np.frombuffer(raw.tobytes(), lib.RESULT_DTYPE).copy()


def _leaf(rec, name):
    top, _, sub = name.partition("_")
    if top in ("kp", "det") and sub:
        return rec[top][sub]
    return rec[name]


def test_every_field_is_written_as_float_with_its_values(tmp_path):
    rec = _records(5)
    bench.dump_outputs(rec, str(tmp_path))
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    want = [n for n in rec.dtype.names if n not in ("kp", "det", "pad")]
    want += [f"{t}_{f}" for t in ("kp", "det") for f in rec.dtype[t].base.names if f != "pad"]
    assert sorted(got) == sorted(want)
    for name, v in got.items():
        src = _leaf(rec, name)
        assert v.shape == src.shape and v.dtype == (np.float32 if src.dtype == np.float32 else np.float64), name
        assert np.array_equal(v, src.astype(v.dtype), equal_nan=True), name


def test_a_larger_output_is_a_fixed_seeded_sample_of_frames(tmp_path, monkeypatch):
    rec = _records(40)
    per_frame = sum(v.nbytes for v in (np.load(p) for p in _dump(rec[:1], tmp_path / "one")))
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * per_frame + 1)
    a = {p.stem: np.load(p) for p in _dump(rec, tmp_path / "a")}
    b = {p.stem: np.load(p) for p in _dump(rec, tmp_path / "b")}
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_MAX_BYTES
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    rows = [int(np.flatnonzero(rec["H"].view(np.uint64)[:, 0] == np.float64(h).view(np.uint64))[0]) for h in a["H"][:, 0]]
    assert len(rows) == 10 and rows == sorted(set(rows))
    assert np.array_equal(a["hm_idx"], rec["hm_idx"][rows].astype(np.float64))


def _dump(rec, d):
    bench.dump_outputs(rec, str(d))
    return sorted(d.glob("*.npy"))
