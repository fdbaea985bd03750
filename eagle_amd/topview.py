"""Top view (K32): the frames warped onto the pitch plane with the homography of their records, the pitch model's markings drawn over them, the
mean of the warped frames (a mosaic of the pitch without the players) and per frame the distance of its warp from that mosaic.  Every stage behind
the key-point network trusts the homography H of a frame; this is the picture that shows whether H puts the painted lines where the model has them,
and the figure that says which frames of a clip have an H that jumped.  The library (csrc/topview.hip; include/eagle.h has the rule,
tests/topview_ref.py defines every byte) does the work; this module takes H from the records, runs the stage and writes the results.

Conventional choices, not fitted to footage: a frame is ``suspect`` when its residual exceeds 2.0 times the clip's median, a mosaic pixel counts from
one contribution (min_count = 1), the background is black and the markings are red.  Limits: bilinear sampling only, no anti-aliasing where the view
is minified, no lens distortion; the mosaic is a plain mean, not a median, so a player who stands still through the clip and is not box-masked leaves a
ghost; the residual of a frame includes that frame's own contribution to the mosaic; nothing is validated on real footage."""
import collections

import numpy as np

from . import lib
from .occupancy import write_ppm  # noqa: F401  (the mosaic is written through it)

KIND_NONE, KIND_OWN, KIND_CARRIED = 0, 1, 2
SUSPECT = 2.0
Result = collections.namedtuple("Result", "mosaic cnt res_sum res_cnt covered kind params")


def homographies(records, carry=False):
    """records (lib.RESULT_DTYPE) -> (Hs float64 [n, 9], valid uint8 [n], kind uint8 [n]): kind 0 none, 1 the record's own H, 2 carried.  With
    ``carry`` a frame without its own H uses the latest earlier valid one, which is what the reference projects with."""
    recs = np.ascontiguousarray(records, lib.RESULT_DTYPE).reshape(-1)
    n = len(recs)
    Hs, valid, kind = np.zeros((n, 9), np.float64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    last = None
    for i in range(n):
        if recs[i]["H_valid"]:
            last = np.array(recs[i]["H"], np.float64).reshape(9)
            Hs[i], valid[i], kind[i] = last, 1, KIND_OWN
        elif carry and last is not None:
            Hs[i], valid[i], kind[i] = last, 1, KIND_CARRIED
    return Hs, valid, kind


def _params(kw):
    return kw.pop("params") if "params" in kw else lib.topview_params(**kw)


def topview(handle, frames, records, carry=False, out_format="bgr", **kw):
    """The warped frames of a clip in host memory: uint8 [n, Hc, W, 3] ("bgr") or [n, 3 Hc / 2, W] ("nv12" / "i420").  frames uint8 [n, h, w, 3] BGR;
    kw: lib.topview_params' keywords (scale, margin, background, markings, marking_colour), or params=."""
    Hs, valid, _ = homographies(records, carry)
    return handle.topview(frames, Hs, valid, _params(kw), out_format)


def mosaic(handle, frames, records, carry=False, max_staging_bytes=0, **kw):
    """-> Result: the mosaic picture uint8 [Hc, W, 3], cnt uint32 [Hc, W], and the residual triples of every frame.  kw as topview, plus mask_boxes,
    box_pad, first, step, min_count."""
    p = _params(kw)
    recs = np.ascontiguousarray(records, lib.RESULT_DTYPE).reshape(-1)
    Hs, valid, kind = homographies(recs, carry)
    boxes = recs if p.mask_boxes else None
    d_acc = handle.topview_accumulator(p)
    try:
        handle.topview_mosaic_add(frames, Hs, valid, p, d_acc, boxes, True, max_staging_bytes=max_staging_bytes)
        pic, cnt = handle.topview_mosaic_finish(d_acc, p)
        rs, rc, cv = handle.topview_residuals(frames, Hs, valid, p, d_acc, boxes, max_staging_bytes=max_staging_bytes)
    finally:
        handle.free(d_acc)
    return Result(pic, cnt, rs, rc, cv, kind, {k: getattr(p, k) for k in ("scale", "margin", "background", "markings", "marking_colour", "mask_boxes", "box_pad", "first",
                                                                            "step", "min_count")})


def residuals(result):
    """per frame res_sum / (3 res_cnt), None where res_cnt == 0"""
    return [int(s) / (3 * int(c)) if c else None for s, c in zip(result.res_sum, result.res_cnt)]


def to_json(result, carry=False, suspect=SUSPECT):
    """topview.json: the parameters; per frame the kind, covered, the coverage share covered / (105 S 68 S) and the residual (None when res_cnt == 0);
    the clip's median residual; the frames whose residual exceeds ``suspect`` times that median (2.0: a conventional choice, not fitted to footage)."""
    p = result.params
    res = residuals(result)
    area = 105 * p["scale"] * 68 * p["scale"]
    have = sorted(r for r in res if r is not None)
    median = None if not have else have[len(have) // 2] if len(have) % 2 else (have[len(have) // 2 - 1] + have[len(have) // 2]) / 2
    frames = [{"kind": int(k), "covered": int(c), "coverage": int(c) / area, "residual": r} for k, c, r in zip(result.kind, result.covered, res)]
    bad = [] if median is None else [i for i, r in enumerate(res) if r is not None and r > suspect * median]
    params = {k: (float(v) if k == "box_pad" else int(v)) for k, v in p.items()}
    return {"params": dict(params, carry=bool(carry), suspect=float(suspect)), "frames": frames, "median_residual": median, "suspect_frames": bad}
