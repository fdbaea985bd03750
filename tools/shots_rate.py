#!/usr/bin/env python3
"""Cost of the shots kernels (include/eagle.h, eagle_shots_device_frames; csrc/shots.hip): one JSON line.

    python tools/shots_rate.py [--frames-720 200] [--frames-1080 100] [--reps 5]

Per frame size a clip resident in HBM is put through eagle_shots_device_frames, once with random pixels (--distinct generated frames, repeated: every
pixel a bin of its own choosing, the most LDS atomics) and once with one colour everywhere (every pixel in one bin: the worst case for contention).
The signature and the distance kernel are timed apart: HIP events of the profiling mode around the launches, --reps calls after a warm-up call,
reported as the median with the minimum and the maximum.  The clips are larger than the 256 MB Infinity Cache, so the signature kernel reads HBM.
Its yardstick is one read of the clip at the chip's streaming rate, n h w 3 bytes over 6.29 TB/s (the measured float4 copy rate; 8 TB/s is the
specification): `of_streaming_bound` is that time over the measured one.  `one_colour_over_random` compares the two inputs of the same kernel: well
above 2 would say that the folding of equal bins is not doing its work."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagle_amd import lib  # noqa: E402

STREAM = 6.29e12
NAMES = ("shot_signature", "shot_distance")


def timed(h, reps, call):
    """ms of the launches accumulated under each of NAMES in one call: reps calls after one warm-up -> {name: {median, min, max}}"""
    call()
    ms = {k: [] for k in NAMES}
    for _ in range(reps):
        h.set_profiling(1)
        call()
        rows = h.kernel_times()
        h.set_profiling(0)
        for k in NAMES:
            ms[k].append(sum(x[1] for x in rows if x[0] == k))
    return {k: {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(min(v)), 4), "ms_max": round(float(max(v)), 4)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-720", type=int, default=200)
    ap.add_argument("--frames-1080", type=int, default=100)
    ap.add_argument("--distinct", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    res = {"reps": a.reps, "streaming_rate": STREAM}
    p = lib.shot_params(fps=25)
    for (fh, fw), n in (((720, 1280), a.frames_720), ((1080, 1920), a.frames_1080)):
        h = lib.Handle(batch=1, frame_h=fh, frame_w=fw)
        out = {"frames": n, "clip_bytes": n * fh * fw * 3, "ms_at_streaming_rate": round(n * fh * fw * 3 / STREAM * 1e3, 4)}
        r = np.random.default_rng(0)
        base = r.integers(0, 256, (min(a.distinct, n), fh, fw, 3), np.uint8)
        for name, clip in (("random", base[np.arange(n) % len(base)]), ("one_colour", np.full((n, fh, fw, 3), (40, 140, 50), np.uint8))):
            d = h.upload(clip)
            del clip
            try:
                t = timed(h, a.reps, lambda: h.shots_device(d, n, p))
                rows, shots = h.shots_device(d, n, p)
            finally:
                h.free(d)
            t["shot_signature"]["of_streaming_bound"] = round(out["ms_at_streaming_rate"] / t["shot_signature"]["ms_median"], 4)
            t["shot_signature"]["bytes_per_s"] = float("%.4g" % (out["clip_bytes"] / (t["shot_signature"]["ms_median"] * 1e-3)))
            t["shots"] = int(len(shots))
            out[name] = t
        out["one_colour_over_random"] = round(out["one_colour"]["shot_signature"]["ms_median"] / out["random"]["shot_signature"]["ms_median"], 4)
        res["%dx%d" % (fh, fw)] = out
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
