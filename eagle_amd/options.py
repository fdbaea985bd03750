"""Pass options of a processed clip table: where the owner of the ball could play in each kept frame.  Per row a grid over the pitch of how well a pass
from the ball to that cell would do (255: the lane is safe and a teammate receives it first; 0: no chance, or nobody to pass to), the same figure for
every teammate at the point they would run from, and the best of those; per PASS event of the possession step, how the pass that was played compares
with the ones that were open at its release row.

The model is this project's own (the reference leaves the question to the analyst: its examples/pass.py draws one pass between two hand-chosen rows):
the lane from the ball to the target is sampled ``samples`` times, the ball travels at ``v_ball``, a defender reacts for ``t_react`` seconds at their
velocity and then runs at ``v_max``; the lane is as safe as its worst sample, the reception as likely as the receiver's lead over the nearest defender,
both through a logistic of sharpness ``beta``.  16 samples, 0.7 s, 5 m/s, 4 / s and a 15 m/s ball are conventional choices, not fitted to data.
Goalkeepers neither pass, receive nor intercept; lofted passes and a slowing ball are not modelled.  Grids, options and records are computed on the GPU
from the table, its velocities and its possession result where they lie in HBM (include/eagle.h, eagle_pass_options; csrc/options.hip); this module
names the columns and derives the event figures on the host.  tests/options_ref.py defines every output bit."""
import numpy as np

from . import lib


def event_figures(events, site_cols, recs, options, row0=0):
    """events (lib.EVENT_DTYPE), the site columns and the records and options of the rows row0 .. as the library gives them -> per event of kind PASS
    {"event": its index, "chosen": the option byte of to_col at the release row, "best_byte", "best_col", "rank": 1 + the number of teammates with a
    strictly larger byte}; chosen = best_byte = -1 and best_col = rank = None when the release row is not among the rows or not active, its owner is not
    from_col, or to_col has no option there."""
    site_of = {int(c): s for s, c in enumerate(site_cols)}
    out = []
    for k, e in enumerate(events):
        if int(e["kind"]) != lib.EVENT_PASS:
            continue
        r = int(e["release_row"]) - int(row0)
        d = {"event": k, "chosen": -1, "best_byte": -1, "best_col": None, "rank": None}
        if 0 <= r < len(recs) and int(recs[r]["status"]) == lib.PASS_ACTIVE and int(recs[r]["owner_col"]) == int(e["from_col"]) and int(e["to_col"]) in site_of:
            chosen = int(options[r][site_of[int(e["to_col"])]])
            if chosen >= 0:
                d.update(chosen=chosen, best_byte=int(recs[r]["best_byte"]), best_col=int(recs[r]["best_col"]), rank=1 + int((options[r] > chosen).sum()))
        out.append(d)
    return out


def pass_options(handle, table, cells_per_metre=1, samples=16, t_react=0.7, v_max=5.0, beta=4.0, v_ball=15.0, rows=None, grids=True):
    """A lib.PostTable of ``handle`` with a team mapping, velocities (Handle.velocities) and possession (Handle.possession) -> {"grids": uint8 [n, 68 R,
    105 R] or None (grid row 0 is pitch y = 0), "rows": lib.PASS_ROW_DTYPE [n], "options": int16 [n, sites] (-1: no option), "site_cols": the table
    columns of the second axis, "site_ids": their ids, "row0", "cells_per_metre", "events": event_figures() of the table's PASS events}; rows: (first
    row, count), None: every row."""
    p = lib.pass_option_params(cells_per_metre, samples, t_react, v_max, beta, v_ball)
    row0, n = (0, len(table.rows)) if rows is None else (int(rows[0]), int(rows[1]))
    site_cols = handle.pass_options_layout(table)
    g, recs, opt = handle.pass_options(table, p, row0, n, grids=grids)
    return {"grids": g, "rows": recs, "options": opt, "site_cols": site_cols, "site_ids": [int(table.columns[c]["id"]) for c in site_cols], "row0": row0,
            "cells_per_metre": int(cells_per_metre), "events": event_figures(handle.events(table), site_cols, recs, opt, row0)}


def pictures(handle, table, result, scale=8, margin=None):
    """One still per PASS event whose release row has a grid in ``result``: [(event index, BGR uint8 [h, w, 3])], the release row's grid through the
    occupancy picture in the owner's team colour (team 0 red, other teams blue, as on the minimap)."""
    from .occupancy import TEAM0_BGR, TEAM_BGR
    out = []
    if result["grids"] is None:
        return out
    ev = handle.events(table)
    for f in result["events"]:
        r = int(ev[f["event"]]["release_row"]) - result["row0"]
        if 0 <= r < len(result["rows"]):
            colour = TEAM0_BGR if int(result["rows"][r]["group"]) == 0 else TEAM_BGR
            out.append((f["event"], lib.op_occupancy_picture(result["grids"][r], result["cells_per_metre"], scale, margin, colour, device=handle.cfg.device)))
    return out


def to_json(result, table):
    """The dict of pass_options() without its grids (they go to a .npy file), with ids for columns: {"cells_per_metre", "rows": per row {"frame", "status",
    "owner_id", "best_id", "best_byte", "options": {id: byte}}, "events": per PASS event {"event", "frame", "from_id", "to_id", "chosen", "best_byte",
    "best_id", "rank"}}."""
    ident = lambda c: None if c is None or int(c) < 0 else int(table.columns[int(c)]["id"])
    ev = table.handle.events(table) if result["events"] else []
    rows = []
    for i, rec in enumerate(result["rows"]):
        opts = {str(result["site_ids"][s]): int(v) for s, v in enumerate(result["options"][i]) if v >= 0}
        rows.append({"frame": int(table.rows[result["row0"] + i]), "status": lib.PASS_STATUS_NAMES[int(rec["status"])], "owner_id": ident(rec["owner_col"]),
                     "best_id": ident(rec["best_col"]), "best_byte": int(rec["best_byte"]), "options": opts})
    events = [{"event": f["event"], "frame": int(table.rows[int(ev[f["event"]]["row"])]), "from_id": ident(ev[f["event"]]["from_col"]),
               "to_id": ident(ev[f["event"]]["to_col"]), "chosen": f["chosen"], "best_byte": f["best_byte"], "best_id": ident(f["best_col"]), "rank": f["rank"]}
              for f in result["events"]]
    return {"cells_per_metre": result["cells_per_metre"], "rows": rows, "events": events}
