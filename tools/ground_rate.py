#!/usr/bin/env python3
"""Cost of the ground kernel (include/eagle.h, eagle_ground_device_frames; csrc/ground.hip): one JSON line.

    python tools/ground_rate.py [--frames 200] [--reps 5]

A clip of 720 x 1280 frames resident in HBM (--distinct generated frames, repeated), every frame under its own pinhole map, is put through
eagle_ground_device_frames for three workloads: no shapes (the kernel copies the frame: pure pass-through), one line band, and 16 shapes (a zone, a
line and 14 rings spread over the pitch), each to BGR and to I420, with the kernel's per-tile cull and without it (no_cull).  The kernel is timed by
the HIP events of the profiling mode around its launch: --reps calls after a warm-up call, reported as the median with the minimum and the maximum.
The floor is a device-to-device copy of the clip's bytes (hipMemcpyAsync between the same two buffers, timed by HIP events in the same run):
`times_the_copy` is the kernel's median over the copy's.  What the kernel pays for beyond the copy is the double-precision projective map, eight
IEEE divisions per pixel of a tile that a shape may touch."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from eagle_amd import lib  # noqa: E402

FH, FW = 720, 1280
Q = 1024


def pinhole_h(k):
    """H of a camera on the stand, panning with k: pitch -> image P, H = P^-1"""
    Cc, T = np.array([52.5, -30.0, 22.0]), np.array([40.0 + 0.1 * (k % 250), 30.0, 0.0])
    fw = (T - Cc) / np.linalg.norm(T - Cc)
    r = np.cross(fw, [0, 0, 1.0])
    r /= np.linalg.norm(r)
    d = np.cross(fw, r)
    Rm = np.stack([r, d, fw])
    K = np.array([[700.0, 0, (FW - 1) / 2], [0, 700.0, (FH - 1) / 2], [0, 0, 1.0]])
    return np.linalg.inv(K @ np.stack([Rm[:, 0], Rm[:, 1], -Rm @ Cc], 1)).reshape(9)


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


def copy_ms(dst, src, nbytes, reps):
    """a device-to-device copy of nbytes on the null stream between HIP events -> the same three figures"""
    hip = C.CDLL("libamdhip64.so")
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    ms = []
    for k in range(reps + 1):
        t = C.c_float(0)
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemcpyAsync(dst, src, C.c_size_t(nbytes), 3, None) == 0          # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        if k:
            ms.append(t.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(min(ms)), 4), "ms_max": round(float(max(ms)), 4)}


def workloads(n):
    line = lib.ground_band(60 * Q - 128, 60 * Q + 128, 0, 68 * Q, 0xFF0000, 208, True)
    zone = lib.ground_band(60 * Q, 105 * Q, 0, 68 * Q, 0xFF0000, 48, True)
    rings = [lib.ground_ring((8 + 13 * (k % 7)) * Q, (14 + 34 * (k // 7)) * Q, 614, 922, 0xFFFF00, 160, True) for k in range(14)]
    return {"no_shapes": lib.ground_shape_lists([[]] * n), "line": lib.ground_shape_lists([[line]] * n), "shapes_16": lib.ground_shape_lists([[zone, line] + rings] * n)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = a.frames
    h = lib.Handle(batch=1, frame_h=FH, frame_w=FW)
    r = np.random.default_rng(0)
    base = r.integers(0, 64, (min(a.distinct, n), FH, FW, 3), np.uint8)
    base[..., 1] += 100                                          # grass under the default key
    Hs, valid = np.stack([pinhole_h(k) for k in range(n)]), np.ones(n, np.uint8)
    clip_bytes = n * FH * FW * 3
    res = {"frames": n, "size": [FW, FH], "reps": a.reps, "clip_bytes": clip_bytes}
    d = h.upload(base[np.arange(n) % len(base)])
    d_out = h.device_alloc(clip_bytes)
    try:
        res["copy"] = copy_ms(d_out, d, clip_bytes, a.reps)
        for name, (shapes, off) in workloads(n).items():
            for fmt in ("bgr", "i420"):
                for no_cull in ((False,) if name == "no_shapes" else (False, True)):
                    p = lib.ground_params(no_cull=no_cull)
                    cov = h.ground_device(d, n, Hs, valid, shapes, off, d_out, p, fmt)
                    t = timed(h, a.reps, "ground_frames", lambda: h.ground_device(d, n, Hs, valid, shapes, off, d_out, p, fmt))
                    t["times_the_copy"] = round(t["ms_median"] / res["copy"]["ms_median"], 3)
                    t["us_per_frame"] = round(t["ms_median"] * 1e3 / n, 3)
                    t["mean_covered"] = round(float(cov.mean()), 1)
                    res["%s_%s%s" % (name, fmt, "_no_cull" if no_cull else "")] = t
    finally:
        h.free(d)
        h.free(d_out)
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
