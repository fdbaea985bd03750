"""Ground layer / offside view (K34): the offside line of a processed clip table drawn into the camera picture, lying on the grass under the players
as a broadcaster shows it.  The library (csrc/ground.hip; include/eagle.h has the rule, tests/ground_ref.py defines every byte) maps every pixel of a
frame to the pitch with the frame's homography and blends shapes that are defined on the pitch plane, bands and rings in q = 1 / 1024 m, where the
source pixel is grass.  This module turns the offside result of a table (eagle_amd/offside.py) into such shapes and runs the stages, keeping the frames
in HBM between them: selection of the kept frames, the ground stage, the table's annotation primitives on top.

Conventional choices, not fitted to footage: the line is 0.25 m wide at alpha 208, the zone behind it has alpha 48, a ring has the radii 0.6 and
0.9 m at alpha 160; team value 0 is red and every other team blue, as in the annotated video; a ring under an attacker in an offside position is
yellow; in a still the ring under the receiver is green (onside), yellow (close) or red (offside).  The grass key is the shots stage's (g >= 48 and
g - max(r, b) >= 16).

Limits: the key is a colour rule per pixel of the source frame, with no matting and no smoothing over time, so green kits and shadows key wrongly; the
line is only as good as the frame's homography (--topview shows that); no lens distortion; four sub-samples per pixel, so a band narrower than a
far-side pixel thins out instead of staying one pixel wide; bands are axis-aligned on the pitch, which serves offside lines and zones, not pass lanes;
only the foot point of a player is known, as in the offside stage; a frame takes at most 16 shapes, rings under attackers beyond that are left out;
nothing is validated on real footage."""
import numpy as np

from . import lib, topview

Q = lib.SHAPE_Q
X_MAX, Y_MAX = 105 * Q, 68 * Q                                   # 107520, 69632
GROUP_COLOURS = (0xFF0000, 0x0000FF)                             # B | G << 8 | R << 16: team value 0 red, every other team blue (the annotated video's)
WARNING, SECOND = 0xFFFF00, 0xFFFFFF                             # yellow, white
VERDICT_COLOURS = {lib.OFFSIDE_ONSIDE: 0x00FF00, lib.OFFSIDE_CLOSE: 0xFFFF00, lib.OFFSIDE_OFFSIDE: 0xFF0000}
WIDTH, ZONE_ALPHA, LINE_ALPHA, RING_ALPHA, RING_R0, RING_R1 = 0.25, 48, 208, 160, 0.6, 0.9


def q(v):
    """metres -> the quantisation of the team-shape, space and offside stages"""
    return int(np.floor(np.float64(v) * 1024.0 + 0.5))


def attacks_right(group, direction):
    """whether ``group`` attacks towards x = 105 when group 0 has ``direction`` (lib.OFFSIDE_DIR_RIGHT or _LEFT)"""
    return (group == 0) == (int(direction) == lib.OFFSIDE_DIR_RIGHT)


def line_shapes(line_qx, group, right, width=WIDTH, zone=True, keyed=True):
    """the zone band from the line to the attacked goal line (left out when it would be empty) and the line itself, wq = q(width) wide"""
    wq = q(width)
    if wq < 1:
        raise lib.EagleError(f"the width {width} of the line is below one unit of 1 / 1024 m")
    out = []
    x0, x1 = (line_qx, X_MAX) if right else (0, line_qx)
    if zone and x0 < x1:
        out.append(lib.ground_band(x0, x1, 0, Y_MAX, GROUP_COLOURS[group], ZONE_ALPHA, keyed))
    out.append(lib.ground_band(line_qx - wq // 2, line_qx - wq // 2 + wq, 0, Y_MAX, GROUP_COLOURS[group], LINE_ALPHA, keyed))
    return out


def _ring(values, col, row, colour, keyed):
    x, y = values[int(col), int(row)]
    if not (np.isfinite(x) and np.isfinite(y) and abs(x) <= 1024 and abs(y) <= 1024):
        return None
    return lib.ground_ring(q(x), q(y), q(RING_R0), q(RING_R1), colour, RING_ALPHA, keyed)


def offside_shapes(table, offside_result, team="possession", width=WIDTH, zone=True, rings=True, keyed=True, owner=None):
    """The shapes of every kept row -> (shapes lib.GROUND_SHAPE_DTYPE [off[rows]], off int32 [rows + 1]).  ``table`` gives ``values`` (float64
    [columns][rows][2]); ``offside_result`` is Handle.offside's (records [rows, 2], margins [members, rows], totals [members], clip [1]).  team: 0, 1,
    "both", or "possession": on each row the group of the ball's owner (``owner`` int32 [rows] of table columns, -1: nobody; None: the table's
    possession result), nothing on rows without one.  For a chosen attacking group whose record of the row is OFFSIDE_OK: the keyed zone, the line,
    a ring under the second-last opponent and a warning ring under every attacker with a margin > 0, in this order; at most GROUND_MAX_SHAPES per
    row, the last warning rings giving way."""
    rec, margins, totals, clip = offside_result
    rows = len(rec)
    direction = int(clip[0]["direction"])
    group_of = {int(t["col"]): int(t["group"]) for t in totals}
    if team == "possession":
        if owner is None:
            owner = table.handle.possession_values(table)[1]
        owner = np.asarray(owner).reshape(-1)
        if len(owner) != rows:
            raise lib.EagleError(f"{rows} rows but {len(owner)} owners")
        chosen = [[group_of[int(c)]] if int(c) in group_of else [] for c in owner]
    elif team == "both":
        chosen = [[0, 1]] * rows
    elif team in (0, 1):
        chosen = [[int(team)]] * rows
    else:
        raise lib.EagleError(f"unknown team {team!r} (possession, 0, 1 or both)")
    values = table.values if rings else None
    lists = []
    for r in range(rows):
        per = []
        for a in chosen[r]:
            o = rec[r, a]
            if int(o["status"]) != lib.OFFSIDE_OK or not direction:
                continue
            per += line_shapes(int(o["line_qx"]), a, attacks_right(a, direction), width, zone, keyed)
            if rings:
                per.append(_ring(values, o["second_col"], r, SECOND, keyed))
                per += [_ring(values, t["col"], r, WARNING, keyed) for m, t in enumerate(totals)
                        if int(t["group"]) == a and int(margins[m, r]) != lib.OFFSIDE_NONE and int(margins[m, r]) > 0]
        lists.append([s for s in per if s is not None][: lib.GROUND_MAX_SHAPES])
    return lib.ground_shape_lists(lists)


def stored_offside(handle, table):
    """the offside result kept with the table (Handle.offside's tuple), an EagleError before the first offside call"""
    nm = handle.offside_device(table)
    if nm[0] is None:
        raise lib.EagleError("the table has no offside result: run Handle.offside (Processor.offside, --offside) first")
    rows = len(table.rows)
    rec, mg, totals, clip = np.zeros((rows, 2), lib.OFFSIDE_ROW_DTYPE), np.zeros((nm[5], rows), np.int32), np.zeros(nm[5], lib.OFFSIDE_TOTALS_DTYPE), np.zeros(1, lib.OFFSIDE_CLIP_DTYPE)
    keep = np.zeros(8, np.float64)
    handle._check(handle.L.eagle_post_offside_values(table._t, lib._ptr(rec, keep), lib._ptr(mg, keep), lib._ptr(totals, keep), lib._ptr(clip, keep)), "post_offside_values")
    return rec, mg, totals, clip


def _run(model, sel, Hs, valid, shapes, off, prim_lists, params, pixel_format, out_format):
    """selected frames -> ground stage -> annotation primitives, the frames staying in HBM in between -> (pictures, covered)"""
    hd = model.handle
    n = len(sel)
    h, w = hd.cfg.frame_h, hd.cfg.frame_w
    if n == 0:
        return np.zeros((0, h, w, 3) if out_format == "bgr" else (0, h * 3 // 2, w), np.uint8), np.zeros(0, np.uint32)
    d = model._upload(sel, pixel_format)
    try:
        d_mid = hd.device_alloc(n * h * w * 3)
        try:
            cov = hd.ground_device(d, n, Hs, valid, shapes, off, d_mid, params)
            offsets = np.concatenate([[0], np.cumsum([len(p) for p in prim_lists])]).astype(np.int32)
            prims = np.concatenate(prim_lists) if offsets[-1] else np.zeros(0, lib.PRIM_DTYPE)
            return hd.annotate_prims(d_mid, n, prims, offsets, out_format), cov
        finally:
            hd.free(d_mid)
    finally:
        hd.free(d)


def offside_view(model, frames, records, table, team="possession", width=WIDTH, zone=True, rings=True, keyed=True, pixel_format="bgr", out_format="bgr", params=None,
                 offside_result=None, shape_lists=None):
    """The annotated video of a processed table (CoordinateModel.annotate(table=...)) with the offside line of the chosen team under the players:
    one picture per kept row -> (pictures uint8 [rows, h, w, 3] or [rows, 3h / 2, w], the dict offside_view.json holds).  ``records`` as annotate
    takes them; the homography of a row is topview.homographies(records, carry=True) at its frame, the one the reference projects with.
    offside_result: Handle.offside's tuple (None: the result kept with the table); shape_lists: (shapes, off) in place of offside_shapes' output."""
    recs = model._records_of(records, carried_as_plain=True)
    if len(recs) != len(frames):
        raise ValueError(f"{len(frames)} frames but {len(recs)} records")
    rows = np.asarray(table.rows, np.int64)
    Hs, valid, kind = topview.homographies(recs, carry=True)
    Hs, valid, kind = Hs[rows], valid[rows], kind[rows]
    if shape_lists is None:
        res = stored_offside(model.handle, table) if offside_result is None else offside_result
        shape_lists = offside_shapes(table, res, team, width, zone, rings, keyed)
    shapes, off = shape_lists
    p = lib.ground_params() if params is None else params
    prim_lists = [table.overlay(r, recs[int(f)]) for r, f in enumerate(rows)]
    pics, cov = _run(model, np.asarray(frames)[rows], Hs, valid, shapes, off, prim_lists, p, pixel_format, out_format)
    info = {"params": {"team": team, "width": float(width), "zone": bool(zone), "rings": bool(rings), "keyed": bool(keyed), "key_min": int(p.key_min), "key_lead": int(p.key_lead)},
            "rows": [{"frame": int(f), "homography": int(k), "shapes": int(off[r + 1] - off[r]), "covered": int(cov[r])} for r, (f, k) in enumerate(zip(rows, kind))]}
    return pics, info


def offside_stills(model, frames, records, table, width=WIDTH, zone=True, keyed=True, pixel_format="bgr", params=None):
    """One picture per pass event of the table's possession result whose offside record is OK: the release frame with the line of the receiver's group
    and a ring under the receiver in the colour of the verdict, under the table's annotation -> [(event index, picture uint8 [h, w, 3], dict)]."""
    hd = model.handle
    recs = model._records_of(records, carried_as_plain=True)
    if len(recs) != len(frames):
        raise ValueError(f"{len(frames)} frames but {len(recs)} records")
    events, off_ev = hd.events(table), hd.offside_events(table)
    _, _, _, clip = stored_offside(hd, table)
    direction = int(clip[0]["direction"])
    Hs, valid, kind = topview.homographies(recs, carry=True)
    picks = [k for k, (e, o) in enumerate(zip(events, off_ev)) if int(e["kind"]) == lib.EVENT_PASS and int(o["status"]) == lib.OFFSIDE_EV_OK]
    rel = [int(events[k]["release_row"]) for k in picks]
    fr = np.asarray([int(table.rows[r]) for r in rel], np.int64)
    lists = []
    for k, r in zip(picks, rel):
        o = off_ev[k]
        g = int(o["group"])
        ring = _ring(table.values, events[k]["to_col"], r, VERDICT_COLOURS[int(o["verdict"])], keyed)
        lists.append(line_shapes(int(o["line_qx"]), g, attacks_right(g, direction), width, zone, keyed) + ([] if ring is None else [ring]))
    shapes, off = lib.ground_shape_lists(lists)
    p = lib.ground_params() if params is None else params
    prim_lists = [table.overlay(r, recs[int(f)]) for r, f in zip(rel, fr)]
    pics, cov = _run(model, np.asarray(frames)[fr], Hs[fr], valid[fr], shapes, off, prim_lists, p, pixel_format, "bgr")
    return [(k, pics[i], {"event": k, "row": rel[i], "frame": int(fr[i]), "homography": int(kind[fr[i]]), "verdict": lib.OFFSIDE_VERDICT_NAMES[int(off_ev[k]["verdict"])],
                          "covered": int(cov[i])}) for i, k in enumerate(picks)]
