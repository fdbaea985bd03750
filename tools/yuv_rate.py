#!/usr/bin/env python3
"""Cost of decoder-native input (include/eagle.h, eagle_process_frames_yuv): one JSON line.

    python tools/yuv_rate.py [--frames 1000] [--batch 50] [--reps 3]

* host-fed frames/s of BGR, NV12 and I420 on the same synthetic clip (default handle, B = --batch), from pageable memory and from pinned memory
  (eagle_host_alloc), formats interleaved per repetition, best of --reps;
* the one-frame call (a batch-1 handle, what the reference's per-frame loop does): median ms per call of each format;
* the yuv_to_bgr rows of eagle_get_kernel_times (profiling mode, one call of B frames): us per launch and achieved GB/s on the kernel's own bytes
  (1.5 B read + 3 B written per pixel) against the measured 6.3 TB/s of HBM, and the kernel's share of the profiled step.
The clip tiles 50 distinct synthetic frames (every frame still goes through the whole path)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagle_amd import lib, synth, weights  # noqa: E402

HBM_TBS = 6.3


def encode(fmt, bgr):
    return bgr if fmt == "bgr" else synth.bgr_to_nv12(bgr) if fmt == "nv12" else synth.bgr_to_i420(bgr)


def call(h, fmt, src, out):
    return h.process(src, out) if fmt == "bgr" else h.process_yuv(src, fmt, out=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--latency-calls", type=int, default=30)
    a = ap.parse_args()
    sds = [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)]
    base = synth.clip(0, min(50, a.frames))
    fmts = ["bgr", "nv12", "i420"]
    reps = (a.frames + len(base) - 1) // len(base)
    clips = {f: np.concatenate([encode(f, base)] * reps)[: a.frames] for f in fmts}
    res = {"frames": a.frames, "batch": a.batch, "unit": "frames/s, host-fed, records back on the host (best of reps)"}

    h = lib.Handle(batch=a.batch)
    weights.load_into(h, sds)
    out = np.zeros(a.frames, lib.RESULT_DTYPE)
    for f in fmts:                                                       # warm-up: copy pool, staging buffers, first launches
        call(h, f, clips[f][: 2 * a.batch], out)
    pinned = {}
    for f in fmts:
        buf = h.host_buffer(clips[f].nbytes)
        buf[:] = clips[f].reshape(-1)
        pinned[f] = buf.reshape(clips[f].shape)
    for src_name, srcs in (("pageable", clips), ("pinned", pinned)):
        best = {f: 0.0 for f in fmts}
        for _ in range(a.reps):
            for f in fmts:
                t0 = time.perf_counter()
                call(h, f, srcs[f], out)
                best[f] = max(best[f], a.frames / (time.perf_counter() - t0))
        res[src_name] = {f: round(best[f], 1) for f in fmts}
        res[src_name + "_ratio_to_bgr"] = {f: round(best[f] / best["bgr"], 4) for f in fmts[1:]}
    for f in fmts:
        h.host_free(pinned[f].reshape(-1))

    # kernel rows: one profiled call of B frames per format
    kt = {}
    for f in ("nv12", "i420"):
        h.set_profiling(1)
        call(h, f, clips[f][: a.batch], out)
        rows = h.kernel_times()
        h.set_profiling(0)
        step_ms = sum(r[1] for r in rows)
        for name, ms, launches, nbytes, _ in rows:
            if name == "yuv_to_bgr":
                us = 1e3 * ms / max(launches, 1)
                gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
                kt[f] = {"us_per_launch": round(us, 1), "frames_per_launch": a.batch, "GB_per_s": round(gbs, 1),
                         "fraction_of_hbm": round(gbs / (HBM_TBS * 1e3), 3), "share_of_profiled_step": round(ms / step_ms, 5) if step_ms else None}
    res["kernel_yuv_to_bgr"] = kt
    h.close()

    h1 = lib.Handle(batch=1)
    weights.load_into(h1, sds)
    o1 = np.zeros(1, lib.RESULT_DTYPE)
    lat = {}
    for f in fmts:
        for i in range(3):
            call(h1, f, clips[f][i: i + 1], o1)
    for f in fmts:
        ts = []
        for i in range(a.latency_calls):
            t0 = time.perf_counter()
            call(h1, f, clips[f][i % len(base): i % len(base) + 1], o1)
            ts.append(time.perf_counter() - t0)
        lat[f] = round(1e3 * float(np.median(ts)), 3)
    res["one_frame_call_ms_median"] = lat
    h1.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
