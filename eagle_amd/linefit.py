"""Line registration (K39): each frame's homography moved until the frame's painted-line pixels lie on the pitch model's centre lines.  It is the one
stage that measures a homography against something absolute, and it runs before anything is projected with the matrix.  The library (csrc/linefit.hip;
include/eagle.h has the rule, tests/linefit_ref.py defines every bit) does the work; this module holds the defaults, the call and the host arithmetic of
lines.json: RMS residuals in metres are the integer e^2 sums over 1024^2.  It is opt-in; without it every output is what it was.

Conventional choices, not fitted to data: k = 4 pixels and tau = 200 (50 grey levels) for a line pixel, boxes widened by 3 pixels, five rounds with the
inlier radius falling from 2.5 m by 0.6 per round to 0.5 m, 20 inliers for a line to count, 200 inliers and at most 3 m of shift for a refined matrix, at
most 4 m per unknown and round.  Limits: straight centre lines and three arcs only; no lens distortion; a line pixel is a colour-and-contrast rule, so
white boots outside a box and advertising on grass-coloured ground are candidates until the radius shuts them out; a view with fewer than two line
directions can only be shifted; a wrong but self-consistent match (the goal-area line taken for the penalty-area line) is possible and bounded only by
radius and max_shift; frames are independent, nothing is carried from one to the next; nothing is validated on real footage."""
import collections
import math

import numpy as np

from . import lib

Q = 1024
PARAMS = ("k", "tau", "rounds", "model", "min_points", "min_per_line", "box_pad", "radius", "radius_min", "radius_factor", "max_shift", "max_step")
Result = collections.namedtuple("Result", "Hs frames masks params")


def default_params(**kw):
    """lib.EagleLineFitParams with the library's defaults and the given fields replaced; model also by name ("projective", "affine", "translation")."""
    if isinstance(kw.get("model"), str):
        if kw["model"] not in lib.LINEFIT_MODEL[1:]:
            raise ValueError(f"linefit: model {kw['model']!r} is none of {lib.LINEFIT_MODEL[1:]}")
        kw["model"] = lib.LINEFIT_MODEL.index(kw["model"])
    return lib.linefit_params(**kw)


def params_dict(p):
    d = {k: (float if k in ("box_pad", "radius", "radius_min", "radius_factor", "max_shift", "max_step") else int)(getattr(p, k)) for k in PARAMS}
    d["model"] = lib.LINEFIT_MODEL[d["model"]]
    return d


def refine(handle, frames, Hs, valid, records=None, masks=False, max_staging_bytes=0, n=None, **kw):
    """frames uint8 [n, h, w, 3] in host memory, or a device pointer with ``n``; Hs [n, 9] image -> pitch, valid [n]; records (lib.RESULT_DTYPE): their
    detections are the boxes that hide players from the line-pixel rule -> Result(Hs float64 [n, 9], frames lib.LINEFIT_FRAME_DTYPE [n], masks, params).
    kw: default_params' keywords, or params=."""
    p = kw.pop("params") if "params" in kw else default_params(**kw)
    if isinstance(frames, lib.C.c_void_p):
        out, fr, mk = handle.linefit_device(frames, n, Hs, valid, records, p, masks)
    else:
        out, fr, mk = handle.linefit(frames, Hs, valid, records, p, masks, max_staging_bytes)
    return Result(out, fr, mk, params_dict(p))


def apply(handle, records, result):
    """In place: the records of the accepted frames are re-projected with their refined matrix by the library's own arithmetic (Handle.reproject), so foot
    points, integer pitch cells, in_bounds and boundaries follow it and the record's H is the refined one -> the records."""
    recs = np.ascontiguousarray(records, lib.RESULT_DTYPE).reshape(-1)
    flags = (result.frames["status"] == lib.LINEFIT_ACCEPTED).astype(np.uint8)
    if len(recs) != len(flags):
        raise ValueError(f"linefit: {len(flags)} refined frames but {len(recs)} records")
    if flags.any():
        handle.reproject(recs, result.Hs, flags)
    return recs


def _rms(e2, n):
    return math.sqrt(int(e2) / int(n)) / Q if int(n) else 0.0


def _causes(fall):
    return [f"{lib.LINEFIT_MODEL[r + 1]}:{lib.LINEFIT_CAUSE[c]}" for r in range(3) for c in range(3) if int(fall) >> (3 * r + c) & 1]


def to_json(result, rows=False, far=1.0):
    """lines.json: the parameters; the totals (frames per status and per model, fall-backs by cause, the RMS residual in metres before and after over the
    accepted frames, the largest shift in metres); the frames whose shift exceeds ``far`` metres; with ``rows`` a record per frame."""
    fr = result.frames
    acc = fr["status"] == lib.LINEFIT_ACCEPTED
    shift = [None if int(s) < 0 else math.sqrt(int(s)) / Q for s in fr["shift2"]]
    falls = collections.Counter(c for f in fr["fall"] for c in _causes(f))
    totals = {"frames": int(len(fr)), "status": {name: int((fr["status"] == i).sum()) for i, name in enumerate(lib.LINEFIT_STATUS)},
              "model": {name: int(((fr["model"] == i) & (fr["status"] != lib.LINEFIT_NO_MAP)).sum()) for i, name in enumerate(lib.LINEFIT_MODEL)},
              "fall_backs": dict(sorted(falls.items())),
              "rms_before": _rms(fr["e2_before"][acc].sum(dtype=object), fr["n_before"][acc].sum(dtype=object)),
              "rms_after": _rms(fr["e2_after"][acc].sum(dtype=object), fr["n_after"][acc].sum(dtype=object)),
              "largest_shift": max([s for s, a in zip(shift, acc) if a and s is not None], default=0.0)}
    out = {"params": result.params, "totals": totals,
           "far_frames": [{"frame": i, "shift": s, "status": lib.LINEFIT_STATUS[int(fr["status"][i])]} for i, s in enumerate(shift) if s is None or s > far]}
    if rows:
        out["rows"] = [{"frame": i, "status": lib.LINEFIT_STATUS[int(e["status"])], "model": lib.LINEFIT_MODEL[int(e["model"])], "rounds": int(e["rounds"]),
                        "line_pixels": int(e["n_line"]), "inliers_before": int(e["n_before"]), "inliers_after": int(e["n_after"]),
                        "rms_before": _rms(e["e2_before"], e["n_before"]), "rms_after": _rms(e["e2_after"], e["n_after"]), "shift": shift[i],
                        "fall_backs": _causes(e["fall"])} for i, e in enumerate(fr)]
    return out
