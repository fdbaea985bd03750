#!/usr/bin/env python3
"""Cost of annotated output (include/eagle.h, eagle_annotate_device_frames; csrc/annotate.hip): one JSON line.

    python tools/annotate_rate.py [--batch 50] [--reps 20]

One launch annotates --batch frames of a clip resident in HBM.  Reported per output format (bgr, nv12, i420), with realistic overlays (25 persons,
1 ball and 30 key-points per frame) and with empty overlays (the plain copy / conversion): us per launch (HIP events of the profiling mode, mean of
--reps launches after a warm-up) and TB/s of the kernel's algorithmic bytes (the BGR frame read once + the output written once) against the
measured 6.3 TB/s of HBM.  In the same run: yuv_to_bgr_kernel, the nearest existing kernel by bytes moved (1.5 B read + 3 B written per pixel), from
one profiled eagle_process_device_frames_yuv call per repetition."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagle_amd import lib, synth, weights  # noqa: E402

HBM_TBS = 6.3


def realistic_records(n, h, w, seed=0):
    """records as a broadcast frame gives them: 25 reported persons (2 goalkeepers), a ball, 30 key-points without a homography"""
    r = np.random.default_rng(seed)
    recs = np.zeros(n, lib.RESULT_DTYPE)
    for rec in recs:
        rec["n_det"], rec["n_kp"] = 26, 30
        for j in range(26):
            d = rec["det"][j]
            d["reported"], d["cls"], d["id"] = 1, (2 if j == 25 else 1 if j < 2 else 0), j + 1
            d["foot_x"], d["foot_y"] = int(r.integers(40, w - 40)), int(r.integers(h // 4, h - 20))
        for k in range(30):
            kp = rec["kp"][k]
            kp["label"], kp["x"], kp["y"] = k, int(r.integers(0, w)), int(r.integers(0, h))
    return recs


def row(rows, name):
    for nm, ms, launches, nbytes, _ in rows:
        if nm == name and launches:
            tbs = nbytes / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            return {"us_per_launch": round(1e3 * ms / launches, 1), "launches": launches, "TB_per_s": round(tbs, 3), "fraction_of_hbm": round(tbs / HBM_TBS, 3)}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    B = a.batch
    h = lib.Handle(batch=B)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    fh, fw = h.cfg.frame_h, h.cfg.frame_w
    base = synth.clip(0, min(10, B))
    frames = np.concatenate([base] * ((B + len(base) - 1) // len(base)))[:B]
    overlays = {"realistic": realistic_records(B, fh, fw), "empty": np.zeros(B, lib.RESULT_DTYPE)}
    mapping = {i: i % 2 for i in range(1, 27)}
    res = {"batch": B, "frame": [fh, fw], "reps": a.reps, "hbm_TB_per_s": HBM_TBS,
           "primitives_per_frame": {k: len(lib.overlay_from_record(v[0], mapping)) for k, v in overlays.items()}}
    d = h.upload(frames)
    d_out = h.upload(np.zeros(B * fh * fw * 3, np.uint8))
    nv12 = synth.bgr_to_nv12(frames)
    d_yuv = h.upload(nv12)
    out = np.zeros(B, lib.RESULT_DTYPE)
    try:
        for fmt in ("bgr", "nv12", "i420"):
            res[fmt] = {}
            for name, recs in overlays.items():
                h.annotate_device(d, B, recs, d_out, mapping, fmt)              # warm-up
                h.set_profiling(1)
                for _ in range(a.reps):
                    h.annotate_device(d, B, recs, d_out, mapping, fmt)
                res[fmt][name] = row(h.kernel_times(), "annotate")
                h.set_profiling(0)
            e, r = res[fmt]["empty"], res[fmt]["realistic"]
            res[fmt]["realistic_over_empty"] = round(r["us_per_launch"] / e["us_per_launch"], 3) if e and r and e["us_per_launch"] else None
        h.process_device_yuv(d_yuv, B, "nv12", out=out)                         # warm-up
        h.set_profiling(1)
        for _ in range(3):
            h.process_device_yuv(d_yuv, B, "nv12", out=out)
        res["yuv_to_bgr_nv12"] = row(h.kernel_times(), "yuv_to_bgr")
        h.set_profiling(0)
    finally:
        h.free(d); h.free(d_out); h.free(d_yuv)
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
