"""Rate of the clip post-processor (include/eagle.h eagle_postprocess; csrc/post.hip) on a synthetic match-length table:

    python tools/post_rate.py [--rows 135000] [--cols 600] [--occupancy 0.2] [--repeats 7] [--smooth] [--fragments 40] [--merge-ids]

135 000 rows = a 90-minute match at 25 frames/s; `cols` person ids, each present in runs on `occupancy` of the rows (two table columns per id, plus
the boundary and ball columns).  Times the whole call (host bookkeeping + uploads + both launches) and, through the library's profiling mode, each
kernel; prints medians over the repeats after a warm-up call, and TB/s of the kernels' algorithmic table bytes (scatter: the raw table written once;
series: the raw table read twice + the processed table written once).  With pandas importable it also times the same passes done the reference's
way (interpolate_df of eagle/processor.py:30-45 restated here: per-column ``apply`` + ``interpolate`` + the tuple rebuild) on the same table.

``--fragments F`` swaps the table for a fragmented clip: `cols` persons (at most 200) in steady motion on every frame, each cut at random rows into F
pieces under fresh ids with up to 3 frames lost at a cut, so 2 F `cols` person columns, each about 1 / F full.  ``--merge-ids`` turns the id merge on
(include/eagle.h): the pieces of a person become one column again.  The series kernel's bytes are then compared with its traffic bound: every raw
cell once for the statistics, and in each of its two passes at most two raw cells per output cell, plus the output written once."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eagle_amd import lib  # noqa: E402


def synthetic_records(rows, cols, occupancy, seed=0):
    rng = np.random.default_rng(seed)
    present = np.zeros((rows, cols), bool)
    run = max(25, rows // 200)
    for c in range(cols):                                   # runs of ~`run` rows, each present with probability `occupancy`
        edges = np.concatenate([[0], np.cumsum(rng.integers(run // 2, 2 * run, size=2 * rows // run + 2))])
        on = rng.random(len(edges)) < occupancy
        present[:, c] = on[np.searchsorted(edges, np.arange(rows), side="right") - 1]
    present[:, 0] = True                                    # every frame is kept
    present &= np.cumsum(present, 1) <= lib.MAX_DET - 1
    recs = np.zeros(rows, lib.RESULT_DTYPE)
    t, c = np.nonzero(present)
    k = (np.cumsum(present, 1) - 1)[t, c]
    det = recs["det"]
    x, y = rng.integers(0, 1200, len(t)), rng.integers(60, 700, len(t))
    for name, val in (("cls", 0), ("id", c), ("reported", 1), ("in_bounds", 1), ("bx1", x), ("bx2", x + 20), ("by1", y - 40), ("by2", y),
                      ("pitch_x", x % 106), ("pitch_y", y % 69), ("conf", 0.9)):
        det[name][t, k] = val
    nd = present.sum(1)
    ball = rng.random(rows) < 0.5
    for name, val in (("cls", 2), ("id", 0), ("reported", 1), ("in_bounds", 1), ("bx1", 600), ("bx2", 606), ("by1", 300), ("by2", 306), ("pitch_x", 50),
                      ("pitch_y", 30), ("conf", 0.8)):
        det[name][np.flatnonzero(ball), nd[ball]] = val
    recs["n_det"] = nd + ball
    recs["H_valid"] = 1
    recs["bounds_valid"] = 1
    recs["bounds"] = (10.0, 12.0, 90.0, 95.0)
    return recs


def fragmented_records(rows, cols, fragments, seed=0):
    rng = np.random.default_rng(seed)
    if cols > 200:
        print(f"--fragments: {cols} persons asked for, 200 used (a frame holds at most {lib.MAX_DET} detections)", file=sys.stderr)
        cols = 200
    need = int(np.ceil(0.01 * rows)) + 4                    # a piece passes the 1 % filter after losing up to 3 frames
    if fragments * need > rows:
        raise SystemExit(f"--fragments {fragments}: a piece needs {need} of the {rows} rows")
    t = np.arange(rows)
    tri = np.abs((2 * t) % 4000 - 2000)                     # 2 px per frame, back and forth
    recs = np.zeros(rows, lib.RESULT_DTYPE)
    det = recs["det"]
    next_id = 1
    for k in range(cols):
        extra = np.sort(rng.integers(0, rows - fragments * need + 1, fragments - 1))
        cuts = np.concatenate([[0], (np.arange(1, fragments) * need + extra), [rows]]).astype(int)
        pid = np.zeros(rows, np.int32)
        on = np.ones(rows, bool)
        for i in range(fragments):
            pid[cuts[i]:cuts[i + 1]] = next_id
            next_id += 1
            if i:
                on[cuts[i]:cuts[i] + int(rng.integers(0, 4))] = False
        on[0] = on[0] or k == 0
        if k == 0:
            on[:] = True                                    # every frame is kept
        x, y = 100 + 2500 * (k % 20) + tri, 300 + 2800 * (k // 20) + tri // 2
        for name, val in (("cls", 0), ("id", pid), ("reported", 1), ("in_bounds", 1), ("bx1", x), ("bx2", x + 20), ("by1", y - 40), ("by2", y), ("pitch_x", x % 106),
                          ("pitch_y", y % 69), ("conf", 0.9)):
            det[name][:, k] = np.where(on, val, 0)
    recs["n_det"] = cols
    recs["H_valid"] = 1
    recs["bounds_valid"] = 1
    recs["bounds"] = (10.0, 12.0, 90.0, 95.0)
    return recs


def pandas_way(values, names):
    """interpolate_df (proc.py:30-45) over every column of the raw table, as process_data's loop does."""
    import math
    import pandas as pd
    df = pd.DataFrame({n: pd.Series([tuple(v) if not math.isnan(v[0]) else np.nan for v in values[c]], dtype=object) for c, n in enumerate(names)})
    t0 = time.perf_counter()
    for col in df.columns:
        s = df[col]
        x = s.apply(lambda v: v[0] if isinstance(v, (list, tuple)) else np.nan).interpolate(method="linear", limit_area="inside")
        y = s.apply(lambda v: v[1] if isinstance(v, (list, tuple)) else np.nan).interpolate(method="linear", limit_area="inside")
        df[col] = pd.Series([(xi, yi) if not (math.isnan(xi) and math.isnan(yi)) else np.nan for xi, yi in zip(x, y)], index=s.index)
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=135000)
    ap.add_argument("--cols", type=int, default=600)
    ap.add_argument("--occupancy", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--smooth", action="store_true")
    ap.add_argument("--fragments", type=int, default=0, help="a fragmented clip instead: every person cut into this many pieces under fresh ids")
    ap.add_argument("--merge-ids", action="store_true", help="stitch fragmented ids (eagle_postprocess's merge_ids = 1)")
    ap.add_argument("--pandas-cols", type=int, default=40, help="columns of the table handed to the pandas restatement (its time is scaled to all columns)")
    a = ap.parse_args(argv)
    recs = fragmented_records(a.rows, a.cols, a.fragments) if a.fragments else synthetic_records(a.rows, a.cols, a.occupancy)
    h = lib.Handle(batch=1)
    raw_cols = None
    if a.merge_ids:
        # the raw table's width: 4 boundary and 2 ball columns and two per (class, id) seen in the records (the kernel reads them all, kept or not)
        det = recs["det"]
        seen = det["reported"].astype(bool) & (det["cls"] < 2) & (np.arange(det.shape[1])[None, :] < recs["n_det"][:, None])
        raw_cols = 6 + 2 * len(np.unique(det["cls"][seen].astype(np.int64) << 32 | det["id"][seen].astype(np.int64)))
    calls, kern = [], {}
    shape = None
    for rep in range(a.repeats + 1):                        # the first call is the warm-up
        h.set_profiling(True)
        t0 = time.perf_counter()
        t = h.postprocess(recs, 25, 1280, {}, smooth=a.smooth, merge_ids=a.merge_ids)
        dt = time.perf_counter() - t0
        merges = len(t.merges)
        shape = (len(t.rows), len(t.columns))
        if rep == a.repeats and a.pandas_cols:
            sample = (t.values[: a.pandas_cols].copy(), t.names[: a.pandas_cols])
            t.close()
        else:                                               # (close() copies the table to the host first: not wanted for 2.6 GB per repeat)
            h.L.eagle_post_free(t._t); t._t = None
        if rep:
            calls.append(dt)
            for name, ms, launches, nbytes, _ in h.kernel_times():
                if name.startswith("post_"):
                    kern.setdefault(name, []).append((ms / max(launches, 1), nbytes / max(launches, 1)))
    out = {"rows": shape[0], "columns": shape[1], "fragments": a.fragments, "merge_ids": bool(a.merge_ids), "merges": merges, "smooth": bool(a.smooth), "repeats": a.repeats, "call_ms_median": round(1e3 * statistics.median(calls), 3)}
    for name, v in kern.items():
        ms = statistics.median(x[0] for x in v)
        out[name] = {"us_median": round(1e3 * ms, 1), "tb_per_s": round(v[0][1] / (ms * 1e-3) / 1e12, 3), "algorithmic_bytes": v[0][1]}
    if raw_cols is not None and "post_series" in out:
        bound = 16.0 * shape[0] * (raw_cols + 2 * 2 * shape[1] + shape[1])
        out["post_series"]["traffic_bound_bytes"] = bound
        out["post_series"]["tb_per_s_of_bound"] = round(bound / (out["post_series"]["us_median"] * 1e-6) / 1e12, 3)
    try:
        import pandas  # noqa: F401
        if a.pandas_cols:
            sec = pandas_way(*sample)
            out["pandas_interpolate_s_all_columns"] = round(sec * shape[1] / len(sample[1]), 2)
            out["pandas_columns_timed"] = len(sample[1])
    except ImportError:
        out["pandas_interpolate_s_all_columns"] = None
    print(json.dumps(out))
    h.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
