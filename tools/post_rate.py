"""Rate of the clip post-processor (include/eagle.h eagle_postprocess; csrc/post.hip) on a synthetic match-length table:

    python tools/post_rate.py [--rows 135000] [--cols 600] [--occupancy 0.2] [--repeats 7] [--smooth]

135 000 rows = a 90-minute match at 25 frames/s; `cols` person ids, each present in runs on `occupancy` of the rows (two table columns per id, plus
the boundary and ball columns).  Times the whole call (host bookkeeping + uploads + both launches) and, through the library's profiling mode, each
kernel; prints medians over the repeats after a warm-up call, and TB/s of the kernels' algorithmic table bytes (scatter: the raw table written once;
series: the raw table read twice + the processed table written once).  With pandas importable it also times the same passes done the reference's
way (interpolate_df of eagle/processor.py:30-45 restated here: per-column ``apply`` + ``interpolate`` + the tuple rebuild) on the same table."""
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
    ap.add_argument("--pandas-cols", type=int, default=40, help="columns of the table handed to the pandas restatement (its time is scaled to all columns)")
    a = ap.parse_args(argv)
    recs = synthetic_records(a.rows, a.cols, a.occupancy)
    h = lib.Handle(batch=1)
    calls, kern = [], {}
    shape = None
    for rep in range(a.repeats + 1):                        # the first call is the warm-up
        h.set_profiling(True)
        t0 = time.perf_counter()
        t = h.postprocess(recs, 25, 1280, {}, smooth=a.smooth)
        dt = time.perf_counter() - t0
        shape = (len(t.rows), len(t.columns))
        if rep == a.repeats and a.pandas_cols:
            sample = (t.values[: a.pandas_cols].copy(), t.names[: a.pandas_cols])
        t.handle.L.eagle_post_free(t._t); t._t = None
        if rep:
            calls.append(dt)
            for name, ms, launches, nbytes, _ in h.kernel_times():
                if name.startswith("post_"):
                    kern.setdefault(name, []).append((ms / max(launches, 1), nbytes / max(launches, 1)))
    out = {"rows": shape[0], "columns": shape[1], "smooth": bool(a.smooth), "repeats": a.repeats, "call_ms_median": round(1e3 * statistics.median(calls), 3)}
    for name, v in kern.items():
        ms = statistics.median(x[0] for x in v)
        out[name] = {"us_median": round(1e3 * ms, 1), "tb_per_s": round(v[0][1] / (ms * 1e-3) / 1e12, 3), "algorithmic_bytes": v[0][1]}
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
