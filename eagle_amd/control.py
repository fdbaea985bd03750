"""Kinematics and pitch control of a processed clip table: per-player velocity, distance covered and top speed, and per kept frame a grid of the
share of each pitch cell that team 0 reaches first (the exponential time-to-intercept model; its constants are conventional choices, not fitted
to data).

Velocities and grids are computed on the GPU from the table where the post-processor left it in HBM (include/eagle.h, eagle_post_velocities /
eagle_control_*; csrc/post.hip, csrc/control.hip); this module passes arrays through and sums the per-player figures on the host.
tests/control_ref.py defines every output bit (own specification: the reference derives none of this)."""
import numpy as np

from . import lib


def kinematics(handle, table, fps, max_gap=None, speed_cap=12.0, keep=False):
    """A lib.PostTable of ``handle`` -> {"velocities": float64 [columns][rows][2], "players": [{"id", "type", "distance", "top_speed"}]}: one entry per
    Player / Goalkeeper pitch column in table order, distance in metres (the trapezoid sum of speed x dt over the steps between rows that are both
    present and at most max_gap frames apart) and top speed in m/s.  keep=True: the velocities the table already carries (those of the fits after
    eagle_amd.smooth.smooth_tracks) are summed instead of being replaced by differences."""
    vel = handle.velocity_values(table) if keep else handle.velocities(table, fps, max_gap, speed_cap)
    gap = int(fps if max_gap is None else max_gap)
    f = np.asarray(table.rows, np.int64)
    players = []
    for c, k in enumerate(table.columns):
        if k["video"] or int(k["kind"]) not in (lib.POST_PLAYER, lib.POST_GOALKEEPER):
            continue
        sp = np.sqrt(vel[c, :, 0] ** 2 + vel[c, :, 1] ** 2)
        ok = np.isfinite(sp)
        dist = 0.0
        if len(f) > 1:
            step = ok[1:] & ok[:-1] & (np.diff(f) <= gap)
            dist = float(np.sum(0.5 * (sp[1:] + sp[:-1])[step] * (np.diff(f)[step] / float(fps))))
        players.append({"id": int(k["id"]), "type": "Player" if int(k["kind"]) == lib.POST_PLAYER else "Goalkeeper", "distance": dist,
                        "top_speed": float(sp[ok].max()) if ok.any() else 0.0})
    return {"velocities": vel, "players": players}


def control(handle, table, cells_per_metre=1, t_react=0.7, v_max=5.0, beta=4.0, rows=None):
    """A lib.PostTable of ``handle`` with velocities (kinematics above) and a team mapping -> (grids uint8 [n, 68 R, 105 R], share float64 [n]): per
    row the control surface (255: team 0's, 0: the other team's; grid row 0 is pitch y = 0) and team 0's share of the pitch area."""
    p = lib.control_params(cells_per_metre, t_react, v_max, beta)
    row0, n = (0, len(table.rows)) if rows is None else (int(rows[0]), int(rows[1]))
    grids, sums = handle.control(table, p, row0, n)
    gw, gh = lib.control_size(p)
    return grids, sums.astype(np.float64) / float(255 * gw * gh)
