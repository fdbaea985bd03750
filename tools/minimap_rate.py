#!/usr/bin/env python3
"""Cost of the minimap (include/eagle.h, eagle_minimap_device_frames; csrc/minimap.hip): one JSON line.

    python tools/minimap_rate.py [--rows 1000] [--batch 100] [--reps 10]

A processed table of --rows rows and 23 pitch columns (4 boundary corners, 16 players, 2 goalkeepers, the ball) is built by eagle_postprocess from
constructed records; --batch rows at a time are drawn into HBM at 8 pixels per metre (872 x 576).  Reported per output format (bgr, nv12, i420), with
the Voronoi layer on and off: us per call (HIP events of the profiling mode around both launches, mean of --reps calls after a warm-up), frames/s and
output GB/s, next to the write-bandwidth bound (output bytes per frame over the measured 6.3 TB/s of HBM).  In the same run: annotate_kernel's plain
conversion (empty overlays) of 720p frames, as output bytes per second, for comparison per output byte."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagle_amd import lib, synth, weights  # noqa: E402

HBM_TBS = 6.3


def records(n, seed=0):
    """n records: 16 players and 2 goalkeepers wandering over the pitch, one ball, the camera's bounds on every frame"""
    r = np.random.default_rng(seed)
    recs = np.zeros(n, lib.RESULT_DTYPE)
    pos = np.stack([r.uniform(5, 100, 19), r.uniform(5, 63, 19)], 1)
    for rec in recs:
        pos = np.clip(pos + r.normal(0, 0.3, pos.shape), 0, [105, 68])
        rec["n_det"], rec["H_valid"], rec["bounds_valid"] = 19, 1, 1
        rec["bounds"] = (20.0, 10.0, 85.0, 75.0)
        for j in range(19):
            d = rec["det"][j]
            d["reported"], d["in_bounds"], d["cls"], d["id"] = 1, 1, (2 if j == 18 else 1 if j >= 16 else 0), j + 1
            d["bx1"], d["bx2"], d["by1"], d["by2"] = 40 + 60 * j, 60 + 60 * j, 300, 340
            d["pitch_x"], d["pitch_y"], d["conf"] = int(pos[j, 0]), int(pos[j, 1]), 0.9
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    B = min(a.batch, a.rows)
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    t = h.postprocess(records(a.rows), 25, 1280, {i + 1: i % 2 for i in range(16)})
    pitch_cols = int((t.columns["video"] == 0).sum())
    w, hh = lib.minimap_size(lib.minimap_params(8))
    res = {"rows": len(t.rows), "pitch_columns": pitch_cols, "batch": B, "frame": [hh, w], "reps": a.reps, "hbm_TB_per_s": HBM_TBS}
    d_out = h.upload(np.zeros(B * hh * w * 3, np.uint8))
    try:
        for fmt in ("bgr", "nv12", "i420"):
            out_b = hh * w * (3.0 if fmt == "bgr" else 1.5)
            res[fmt] = {"bound_frames_per_s": round(HBM_TBS * 1e12 / out_b)}
            for vor in (0, 1):
                par = lib.minimap_params(8, voronoi=bool(vor))
                h.minimap_device(t, d_out, par, 0, B, fmt)                      # warm-up (and the marking mask)
                h.set_profiling(1)
                for k in range(a.reps):
                    h.minimap_device(t, d_out, par, (k * B) % max(len(t.rows) - B + 1, 1), B, fmt)
                row = [x for x in h.kernel_times() if x[0] == "minimap"][0]
                h.set_profiling(0)
                us = 1e3 * row[1] / row[2]
                res[fmt]["voronoi" if vor else "plain"] = {"us_per_call": round(us, 1), "frames_per_s": round(B / (us * 1e-6)), "out_GB_per_s": round(B * out_b / (us * 1e-6) / 1e9, 1)}
        # annotate_kernel's plain conversion in the same build, per output byte
        fh, fw, nb = h.cfg.frame_h, h.cfg.frame_w, 10
        d = h.upload(synth.clip(0, nb))
        d_o = h.upload(np.zeros(nb * fh * fw * 3, np.uint8))
        empty = np.zeros(nb, lib.RESULT_DTYPE)
        res["annotate_plain"] = {}
        try:
            for fmt in ("bgr", "nv12", "i420"):
                h.annotate_device(d, nb, empty, d_o, None, fmt)
                h.set_profiling(1)
                for _ in range(a.reps):
                    h.annotate_device(d, nb, empty, d_o, None, fmt)
                row = [x for x in h.kernel_times() if x[0] == "annotate"][0]
                h.set_profiling(0)
                us = 1e3 * row[1] / row[2]
                out_b = nb * fh * fw * (3.0 if fmt == "bgr" else 1.5)
                res["annotate_plain"][fmt] = {"us_per_call": round(us, 1), "out_GB_per_s": round(out_b / (us * 1e-6) / 1e9, 1),
                                              "frames_per_s_at_minimap_size": round(out_b / (us * 1e-6) / (hh * w * (3.0 if fmt == "bgr" else 1.5)))}
        finally:
            h.free(d); h.free(d_o)
    finally:
        h.free(d_out)
        t.close()
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
