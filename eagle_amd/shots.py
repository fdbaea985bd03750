"""Shots (K31): where a clip is cut, and which of its shots look at the pitch.  Every other stage assumes one continuous shot of the main camera; a
broadcast is cut every few seconds.  The library (csrc/shots.hip; include/eagle.h has the rule) reads the clip once, builds an integer colour
signature per frame and scores frame pairs; this module picks the parameters from the frame rate, runs the stage and hands the shots on.  The
thresholds are conventional choices: nothing here is fitted to or validated on broadcast footage.  The stage finds boundaries and says whether a shot
shows grass; it does not classify camera angles, and a wipe longer than the window shows only through the grass share of what follows it."""
import collections

import numpy as np

from . import lib

ONE = 65536
Result = collections.namedtuple("Result", "frames shots params")       # SHOT_FRAME_DTYPE [n], SHOT_DTYPE [m], the parameters as a dict (with fps, pixels)


def default_params(fps):
    """cut 0.30, low 0.10 and grass_thr 0.35 in 1 / 65536; W = max(2, round(0.4 fps)) frames, halves up; min_len = fps frames."""
    fps = int(fps)
    if fps < 1:
        raise ValueError(f"fps {fps} must be at least 1")
    return {"cut": (30 * ONE + 50) // 100, "low": (10 * ONE + 50) // 100, "grass_thr": (35 * ONE + 50) // 100, "window": max(2, (4 * fps + 5) // 10), "min_len": fps}


def _params(fps, overrides):
    p = default_params(fps)
    for k, v in overrides.items():
        if k not in p:
            raise TypeError(f"unknown shot parameter {k}")
        if v is not None:
            p[k] = int(v)
    return p


def find_shots(handle, frames, fps, pixel_format="bgr", **overrides):
    """frames: uint8 [n, h, w, 3] BGR, or [n, 3h/2, w] NV12 / I420 (converted on the GPU) -> Result.  overrides: cut, low, grass_thr (1 / 65536),
    window, min_len (frames)."""
    p = _params(fps, overrides)
    cp = lib.EagleShotParams(p["cut"], p["low"], p["grass_thr"], p["window"], p["min_len"])
    if pixel_format == "bgr":
        rows, shots = handle.shots(frames, cp)
    else:
        d = handle.upload_bgr(frames, pixel_format)
        try:
            rows, shots = handle.shots_device(d, len(frames), cp)
        finally:
            handle.free(d)
    return Result(rows, shots, dict(p, fps=int(fps), pixels=int(handle.cfg.frame_h) * int(handle.cfg.frame_w)))


def usable(result):
    """the indices of the usable shots: they look at the pitch and are at least min_len frames long"""
    return [k for k, s in enumerate(result.shots) if int(s["flags"]) & lib.SHOT_USABLE]


def longest_usable(result):
    """the index of the longest usable shot, the earliest on a tie; None without one"""
    best = None
    for k in usable(result):
        if best is None or int(result.shots[k]["count"]) > int(result.shots[best]["count"]):
            best = k
    return best


def split(frames, result, usable_only=True):
    """yields (first, count, frames[first:first + count]) per shot, in clip order"""
    keep = set(usable(result)) if usable_only else None
    for k, s in enumerate(result.shots):
        if keep is None or k in keep:
            first, count = int(s["first"]), int(s["count"])
            yield first, count, frames[first:first + count]


def to_json(result):
    """the parameters, per shot first / count / seconds / kind / pitch / short / usable and the mean grass share, and the flash frames"""
    p = result.params
    shots = []
    for s in result.shots:
        fl, count = int(s["flags"]), int(s["count"])
        shots.append({"first": int(s["first"]), "count": count, "seconds": count / p["fps"], "kind": lib.SHOT_KIND_NAMES[int(s["kind"])],
                      "pitch": bool(fl & lib.SHOT_PITCH), "short": bool(fl & lib.SHOT_SHORT), "usable": bool(fl & lib.SHOT_USABLE),
                      "grass_share": int(s["grass_sum"]) / (p["pixels"] * count)})
    flashes = [int(i) for i in np.flatnonzero(result.frames["flags"] & lib.SHOT_FRAME_FLASH)]
    return {"params": {k: int(p[k]) for k in ("cut", "low", "grass_thr", "window", "min_len", "fps")}, "frames": int(len(result.frames)), "shots": shots, "flashes": flashes}
