#!/usr/bin/env python3
"""Cost of the top-view kernels (include/eagle.h, eagle_topview_*; csrc/topview.hip): one JSON line.

    python tools/topview_rate.py [--frames 200] [--scale 8] [--margin 16] [--reps 5]

A clip of 720 x 1280 frames resident in HBM (--distinct generated frames, repeated) is put through eagle_topview_device_frames (BGR and I420 output),
eagle_topview_mosaic_device and eagle_topview_residual_device, every frame under its own pinhole map whose footprint covers most of the pitch.  The
kernels are timed by the HIP events of the profiling mode around their launches: --reps calls after a warm-up call, reported as the median with the
minimum and the maximum.  The yardstick of each is the time to read the clip once and write its output once at the chip's streaming rate of
6.29 TB/s (the measured float4 copy rate, the one tools/shots_rate.py uses): `of_streaming_bound` is that time over the measured one.  The kernels
gather only the source pixels under the canvas, so the yardstick is an upper bound of the bytes they must move; the double-precision projective map
(two IEEE divisions per pixel and frame) is what they actually pay for.  --boxes N adds N detection boxes per frame to the mosaic and residual."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagle_amd import lib  # noqa: E402

STREAM = 6.29e12
FH, FW = 720, 1280


def pinhole_h(k):
    """H of a camera on the stand, panning with k: pitch -> image P, H = P^-1"""
    C, T = np.array([52.5, -30.0, 22.0]), np.array([40.0 + 0.1 * (k % 250), 30.0, 0.0])
    fw = (T - C) / np.linalg.norm(T - C)
    r = np.cross(fw, [0, 0, 1.0])
    r /= np.linalg.norm(r)
    d = np.cross(fw, r)
    Rm = np.stack([r, d, fw])
    K = np.array([[700.0, 0, (FW - 1) / 2], [0, 700.0, (FH - 1) / 2], [0, 0, 1.0]])
    return np.linalg.inv(K @ np.stack([Rm[:, 0], Rm[:, 1], -Rm @ C], 1)).reshape(9)


def timed(h, reps, name, call):
    call()
    ms = []
    for _ in range(reps):
        h.set_profiling(1)
        call()
        rows = h.kernel_times()
        h.set_profiling(0)
        ms.append(sum(x[1] for x in rows if x[0] == name))
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(min(ms)), 4), "ms_max": round(float(max(ms)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--scale", type=int, default=8)
    ap.add_argument("--margin", type=int, default=16)
    ap.add_argument("--distinct", type=int, default=10)
    ap.add_argument("--boxes", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = a.frames
    p = lib.topview_params(a.scale, a.margin, markings=True, mask_boxes=a.boxes > 0, box_pad=2.0)
    W, Hc = lib.topview_size(p)
    h = lib.Handle(batch=1, frame_h=FH, frame_w=FW)
    r = np.random.default_rng(0)
    base = r.integers(0, 256, (min(a.distinct, n), FH, FW, 3), np.uint8)
    Hs, valid = np.stack([pinhole_h(k) for k in range(n)]), np.ones(n, np.uint8)
    recs = None
    if a.boxes:
        recs = np.zeros(n, lib.RESULT_DTYPE)
        recs["n_det"] = a.boxes
        x, y = r.uniform(0, FW - 60, (n, a.boxes)), r.uniform(0, FH - 120, (n, a.boxes))
        for key, v in (("x1", x), ("y1", y), ("x2", x + 40), ("y2", y + 100)):
            recs["det"][key][:, :a.boxes] = v
    clip_bytes, canvas = n * FH * FW * 3, W * Hc
    res = {"frames": n, "scale": a.scale, "margin": a.margin, "canvas": [W, Hc], "boxes": a.boxes, "reps": a.reps, "streaming_rate": STREAM, "clip_bytes": clip_bytes}
    d = h.upload(base[np.arange(n) % len(base)])
    d_out = h.device_alloc(n * canvas * 3)
    d_acc = h.topview_accumulator(p)
    try:
        for fmt, bpp in (("bgr", 3.0), ("i420", 1.5)):
            t = timed(h, a.reps, "topview_frames", lambda: h.topview_device(d, n, Hs, valid, p, d_out, fmt))
            t["ms_at_streaming_rate"] = round((clip_bytes + n * canvas * bpp) / STREAM * 1e3, 4)
            t["of_streaming_bound"] = round(t["ms_at_streaming_rate"] / t["ms_median"], 4)
            t["canvas_pixels_per_s"] = float("%.4g" % (n * canvas / (t["ms_median"] * 1e-3)))
            res["video_" + fmt] = t
        t = timed(h, a.reps, "topview_accumulate", lambda: h.topview_mosaic_add(d, Hs, valid, p, d_acc, recs, n=n))
        t["ms_at_streaming_rate"] = round((clip_bytes + canvas * 32) / STREAM * 1e3, 4)
        t["of_streaming_bound"] = round(t["ms_at_streaming_rate"] / t["ms_median"], 4)
        res["accumulate"] = t
        t = timed(h, a.reps, "topview_residual", lambda: h.topview_residuals(d, Hs, valid, p, d_acc, recs, n=n))
        t["ms_at_streaming_rate"] = round((clip_bytes + n * canvas * 4) / STREAM * 1e3, 4)      # (the packed means: 4 bytes per pixel and frame)
        t["of_streaming_bound"] = round(t["ms_at_streaming_rate"] / t["ms_median"], 4)
        res["residual"] = t
        rs, rc, cv = h.topview_residuals(d, Hs, valid, p, d_acc, recs, n=n)
        res["mean_coverage"] = round(float(cv.mean()) / (105 * a.scale * 68 * a.scale), 4)
    finally:
        for x in (d, d_out, d_acc):
            h.free(x)
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
