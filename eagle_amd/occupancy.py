"""Occupancy heat maps of a processed clip table: where every player, every team and the ball spent their time, as seconds per pitch cell smoothed by
a Gaussian, plus the shares of that time per third of the pitch's length and per channel of its width.

The maps are computed on the GPU from the table where the post-processor left it in HBM (include/eagle.h, eagle_post_occupancy; csrc/occupancy.hip):
integer frame counts per cell, a separable truncated Gaussian in float32, a byte form and still pictures.  This module chooses the selections, names
them and sums the shares on the host from the raw integer counts, so they are exact.  tests/occupancy_ref.py defines every output bit.  The rule is
this project's own (the reference's users draw such maps with mplsoccer from processed_data.json); the 2 m sigma is a conventional choice, not fitted
to data.  A map follows a person only as far as the ids do: build the table with merge_ids=True for that."""
import numpy as np

from . import lib

TEAM0_BGR, TEAM_BGR, BALL_BGR = (0, 0, 255), (255, 0, 0), (255, 255, 255)      # the minimap's colours: team 0 red, other teams blue, the ball white


def default_selections(columns, team_mapping):
    """columns lib.POSTCOL_DTYPE, team_mapping {id: team} or None -> (sel_off, sel_cols, names): one selection per Player / Goalkeeper pitch column in
    table order, one per team in ascending team value (the Player pitch columns with a mapping entry of that value: the Voronoi-site rule, so
    goalkeepers are not in it; none without a mapping), and the ball (every Ball pitch column; empty without one)."""
    off, cols, names = [0], [], []
    pitch = [(c, int(k["kind"]), int(k["id"])) for c, k in enumerate(columns) if not k["video"]]
    for c, kind, ident in pitch:
        if kind in (lib.POST_PLAYER, lib.POST_GOALKEEPER):
            cols.append(c); off.append(len(cols))
            names.append({"kind": "player" if kind == lib.POST_PLAYER else "goalkeeper", "id": ident})
    if team_mapping is not None:
        tm = {int(i): int(v) for i, v in team_mapping.items()}
        teams = {}
        for c, kind, ident in pitch:
            if kind == lib.POST_PLAYER and ident in tm:
                teams.setdefault(tm[ident], []).append(c)
        for t in sorted(teams):
            cols += teams[t]; off.append(len(cols))
            names.append({"kind": "team", "team": t})
    cols += [c for c, kind, _ in pitch if kind == lib.POST_BALL]
    off.append(len(cols))
    names.append({"kind": "ball"})
    return off, cols, names


def shares(count, cells_per_metre):
    """One selection's integer counts [gh, gw] -> (thirds [3], channels [3]): the shares of the inside time per 35 m third in x and per third of 68 m
    in y, a cell counted by its centre (at 1 cell per metre the x thirds fall on cell edges, the y thirds at 22.67 and 45.33 m do not).  Integer sums:
    exact."""
    R = int(cells_per_metre)
    count = np.asarray(count, np.int64)
    gh, gw = count.shape
    cx, cy = (np.arange(gw) + 0.5) / R, (np.arange(gh) + 0.5) / R
    tot = int(count.sum())
    px, py = count.sum(0), count.sum(1)
    thirds = [int(px[(cx >= 35.0 * k) & (cx < 35.0 * (k + 1))].sum()) for k in range(3)]
    chans = [int(py[(cy >= 68.0 * k / 3.0) & (cy < 68.0 * (k + 1) / 3.0)].sum()) for k in range(3)]
    return [n / tot if tot else 0.0 for n in thirds], [n / tot if tot else 0.0 for n in chans]


def summarise(grids, counts, total, outside, names, fps, cells_per_metre, sigma):
    """What the library returns for the selections `names` -> the dict occupancy() returns.  Pure host arithmetic."""
    sel = []
    for s, name in enumerate(names):
        thirds, chans = shares(counts[s], cells_per_metre)
        sel.append(dict(name, seconds=int(total[s]) / float(int(fps)), outside_seconds=int(outside[s]) / float(int(fps)), thirds=thirds, channels=chans))
    return {"grids": np.asarray(grids, np.float64) / float(int(fps)), "selections": sel, "fps": int(fps), "cells_per_metre": int(cells_per_metre), "sigma": float(sigma)}


def occupancy(handle, table, fps, cells_per_metre=1, sigma=2.0, max_gap=None):
    """A lib.PostTable of ``handle`` -> {"grids": float64 seconds [n_sel][68 R][105 R] (grid row 0 is pitch y = 0), "selections": per map {"kind":
    "player" | "goalkeeper" | "team" | "ball", "id" or "team", "seconds" (inside the pitch), "outside_seconds", "thirds": [3], "channels": [3]}, "fps",
    "cells_per_metre", "sigma"}; the selections are default_selections' (the table's last result, which Handle.occupancy_picture draws, is in this
    order).  max_gap None: fps frames."""
    p = lib.occupancy_params(fps, cells_per_metre, sigma, max_gap)
    off, cols, names = default_selections(table.columns, table.team_mapping)
    grids, _, counts, total, outside = handle.occupancy(table, p, off, cols)
    return summarise(grids, counts, total, outside, names, fps, cells_per_metre, sigma)


def pictures(handle, table, result, scale=8, margin=None):
    """The team and ball maps of occupancy()'s ``result`` (the table's last one) as still pictures: [(name, BGR uint8 [h, w, 3])], name "team<t>" or
    "ball"; team 0 red, other teams blue, the ball white, as on the minimap."""
    out = []
    for s, sel in enumerate(result["selections"]):
        if sel["kind"] == "team":
            out.append(("team%d" % sel["team"], handle.occupancy_picture(table, s, scale, margin, TEAM0_BGR if sel["team"] == 0 else TEAM_BGR)))
        elif sel["kind"] == "ball":
            out.append(("ball", handle.occupancy_picture(table, s, scale, margin, BALL_BGR)))
    return out


def write_ppm(path, bgr):
    """BGR uint8 [h, w, 3] -> a binary PPM (P6)"""
    h, w = bgr.shape[:2]
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(bgr[:, :, ::-1]).tobytes())


def to_json(d):
    """The dict of occupancy() without its grids (they go to a .npy file): JSON's types only."""
    return {k: v for k, v in d.items() if k != "grids"}


def from_json(j, grids=None):
    """The inverse of to_json; ``grids``: the array saved next to it."""
    out = dict(j)
    if grids is not None:
        out["grids"] = np.asarray(grids, np.float64)
    return out
