"""numpy / Python-integer restatement of the space stage (include/eagle.h, eagle_post_space / eagle_op_space / eagle_space_grids; csrc/space.hip): how
much room each player has.  It is the single written definition of every output bit: the kernels equal it bit for bit.  OWN SPEC: the reference's
examples/voronoi.py draws such a picture; nothing of it computes these figures.

GROUPS, MEMBERS, PRESENT, QUANTISE are shape_ref's (members, quantise): groups 0 (team value 0) and 1 (any other non-negative team value) hold the
Player pitch columns (video == 0) with a mapping entry (the first entry for an id counts; here the mapping is a dict, so there is one); a mapping is
required; a member is PRESENT on a row when x and y are finite and |x|, |y| <= 1024 m; q = floor(v * 1024 + 0.5), |q| <= 2^20.  The ball, boundary
columns, video columns and players without an entry (or with a negative one) are no members.

GOALKEEPERS.  With goalkeepers != 0 (the default) the Goalkeeper pitch columns, mapped or not, are the members of group 2, "neither team": they own
cells, they are nobody's opponent and they have no opponent.  With goalkeepers == 0 they are no members, as in shape and roles.  More than
shape_ref.MAX_MEMBERS members over the three groups are refused.

SITES of a row: its present members in table-column order, S of them.  status = EMPTY when S == 0, TOO_MANY when S > SITE_CAP (32), else ACTIVE.  The
row record always holds status, n_sites = S and n[g] = the present members of group g.  A row that is not ACTIVE has no site records (every slot is
unused), no cells, and an owner map of 255.  Unused site slots hold col = near_col = -1, near_d2 = -1 and zeros.

GRID.  cells_per_metre R in {1, 2, 4}, gw = 105 R, gh = 68 R (eagle_control_size's geometry; grid row 0 is pitch y = 0).  The centre of cell (i, j) in
q is X = (2 i + 1) (512 / R), Y = (2 j + 1) (512 / R): integers for all three R.  d2 = (X - qx)^2 + (Y - qy)^2; 0 <= X <= 105 * 1024 and |qx| <= 2^20
give |X - qx| < 2^21, so d2 < 2^43: exact in int64 (and in Python integers).  A cell's OWNER is the site of least d2; of equal d2 the earlier table
column, which is the earlier site.  So coincident sites leave everything to the earlier one, and a site off the pitch is a site like any other.

THIRDS.  Cell (i, j) lies in third 0 when i < 35 R, in third 1 when i < 70 R, else in third 2.  A site's cells[t] = the cells it owns in third t; the
row record's cells[g][t] = their sum over the sites of group g.  On an ACTIVE row all cells add up to gw gh exactly.

MARKING of a site of group 0 or 1, over the row's sites of the other of those two groups: near_d2 = the least squared distance between the two q (int64,
<= 2^43) and near_col = that site's column, the earlier column on a tie; -1, -1 without such a site.  within = the number of those sites with d2 <=
rq^2, inclusive, rq = floor(radius * 1024 + 0.5); radius must be finite, > 0 and <= 1024; the default of 3 m is a conventional choice, not fitted to
data.  A site of group 2 reports -1, -1, 0.

TOTALS per member, members in group order 0, 1, 2 and by column inside a group, over the ACTIVE rows on which the member is present: rows; the int64
sums of cells[3]; min and max of its cell total cells[0] + cells[1] + cells[2] (0 when rows == 0); opp_rows = the rows with near_col >= 0; within_rows
= the rows with within > 0; within_sum.  ROWS ARE COUNTED, not weighted by the frame step to the next row.

OWNER MAP of a row window (row0, n): uint8 [n][gh][gw] = the owner's index into the row's site list; 255 on a row that is not ACTIVE.

TWO DEFINITIONS: space() is vectorised over the cells of a row; space_scalar() is a plain loop over cells and sites in Python integers."""
import math

import numpy as np

import minimap_ref as R_
from shape_ref import MAX_MEMBERS, members, quantise

SITE_CAP = 32
EMPTY, ACTIVE, TOO_MANY = 0, 1, 2
NO_OWNER = 255
ROW_DTYPE = np.dtype([("status", "<i4"), ("n_sites", "<i4"), ("n", "<i4", 3), ("cells", "<i4", (3, 3)), ("reserved", "<i4", 2)])                       # EagleSpaceRow, 64 bytes
SITE_DTYPE = np.dtype([("near_d2", "<i8"), ("col", "<i4"), ("group", "<i4"), ("near_col", "<i4"), ("within", "<i4"), ("cells", "<i4", 3), ("qx", "<i4"),
                       ("qy", "<i4"), ("reserved", "<i4")])                                                                                               # EagleSpaceSite, 48 bytes
TOTALS_DTYPE = np.dtype([("cells", "<i8", 3), ("within_sum", "<i8"), ("col", "<i4"), ("group", "<i4"), ("rows", "<i4"), ("min", "<i4"), ("max", "<i4"),
                         ("opp_rows", "<i4"), ("within_rows", "<i4"), ("reserved", "<i4")])                                                               # EagleSpaceTotals, 64 bytes
assert (ROW_DTYPE.itemsize, SITE_DTYPE.itemsize, TOTALS_DTYPE.itemsize) == (64, 48, 64)


def space_params(cells_per_metre=1, goalkeepers=1, radius=3.0):
    return {"cells_per_metre": int(cells_per_metre), "goalkeepers": int(goalkeepers), "radius": float(radius)}


def check_params(p):
    if p["cells_per_metre"] not in (1, 2, 4):
        raise ValueError("cells_per_metre %r is not 1, 2 or 4" % (p["cells_per_metre"],))
    if not (math.isfinite(p["radius"]) and 0.0 < p["radius"] <= 1024.0):
        raise ValueError("radius %r outside (0, 1024]" % (p["radius"],))


def check_window(rows, row0, n):
    if n < 0 or row0 < 0 or row0 > rows or n > rows - row0:
        raise ValueError("rows %d .. %d lie outside the table's %d rows" % (row0, row0 + n - 1, rows))


def groups_of(columns, mapping, goalkeepers):
    """-> ([columns of group 0], [of group 1], [of group 2]) in table order each"""
    g0, g1 = members(columns, mapping)
    g2 = [c for c, (kind, _, video) in enumerate(columns) if kind == R_.GOALKEEPER and not video] if goalkeepers else []
    if len(g0) + len(g1) + len(g2) > MAX_MEMBERS:
        raise ValueError("more than %d members" % MAX_MEMBERS)
    return g0, g1, g2


def radius_q(p):
    return int(math.floor(p["radius"] * 1024.0 + 0.5))


def third_of(i, R):
    return 0 if i < 35 * R else 1 if i < 70 * R else 2


def _outputs(rows, groups, n, R):
    rec, sites = np.zeros(rows, ROW_DTYPE), np.zeros((rows, SITE_CAP), SITE_DTYPE)
    sites["col"], sites["near_col"], sites["near_d2"] = -1, -1, -1
    totals = np.zeros(sum(len(g) for g in groups), TOTALS_DTYPE)
    m = 0
    for g, cols in enumerate(groups):
        for c in cols:
            totals[m]["col"], totals[m]["group"] = c, g
            m += 1
    return rec, sites, totals, np.full((n, 68 * R, 105 * R), NO_OWNER, np.uint8)


def _row_sites(values, groups, r):
    """the present members of row r in table-column order -> [(qx, qy, column, group)]"""
    out = []
    for g, cols in enumerate(groups):
        if cols:
            qx, qy, ok = quantise(values[cols, r, 0], values[cols, r, 1])
            out += [(int(qx[k]), int(qy[k]), int(c), g) for k, c in enumerate(cols) if ok[k]]
    return sorted(out, key=lambda s: s[2])


def _totals(rec, sites, totals):
    """the totals from the records: Python integers, member by member"""
    member = {int(t["col"]): m for m, t in enumerate(totals)}
    seen = [[] for _ in totals]
    for r in np.nonzero(rec["status"] == ACTIVE)[0]:
        for s in sites[r, :rec[r]["n_sites"]]:
            seen[member[int(s["col"])]].append(s)
    for t, ss in zip(totals, seen):
        if not ss:
            continue
        tot = [int(s["cells"].sum()) for s in ss]
        t["rows"], t["min"], t["max"] = len(ss), min(tot), max(tot)
        t["cells"] = [sum(int(s["cells"][k]) for s in ss) for k in range(3)]
        t["opp_rows"], t["within_rows"] = sum(int(s["near_col"]) >= 0 for s in ss), sum(int(s["within"]) > 0 for s in ss)
        t["within_sum"] = sum(int(s["within"]) for s in ss)


# ---- definition one: vectorised over the cells of a row, int64 ---------------------------------------------------------------------------
def space(values, columns, mapping, p, row0=0, n=0):
    """values float64 [cols][rows][2] -> (ROW_DTYPE [rows], SITE_DTYPE [rows, 32], TOTALS_DTYPE [members], owner map uint8 [n, gh, gw])"""
    check_params(p)
    groups = groups_of(columns, mapping, p["goalkeepers"])
    rows = values.shape[1]
    check_window(rows, row0, n)
    R, rq2 = p["cells_per_metre"], radius_q(p) ** 2
    rec, sites, totals, grid = _outputs(rows, groups, n, R)
    X = ((2 * np.arange(105 * R, dtype=np.int64) + 1) * (512 // R))[None, :]
    Y = ((2 * np.arange(68 * R, dtype=np.int64) + 1) * (512 // R))[:, None]
    third = np.where(np.arange(105 * R) < 35 * R, 0, np.where(np.arange(105 * R) < 70 * R, 1, 2))
    for r in range(rows):
        ss = _row_sites(values, groups, r)
        o = rec[r]
        o["n_sites"], o["n"] = len(ss), [sum(s[3] == g for s in ss) for g in range(3)]
        o["status"] = EMPTY if not ss else TOO_MANY if len(ss) > SITE_CAP else ACTIVE
        if o["status"] != ACTIVE:
            continue
        q = np.array([s[:2] for s in ss], np.int64)
        grp = np.array([s[3] for s in ss])
        d2 = (X[None] - q[:, 0, None, None]) ** 2 + (Y[None] - q[:, 1, None, None]) ** 2
        owner = np.argmin(d2, 0)                                 # (the first of equal minima: the earlier site)
        if row0 <= r < row0 + n:
            grid[r - row0] = owner
        for k, s in enumerate(ss):
            rs = sites[r, k]
            rs["qx"], rs["qy"], rs["col"], rs["group"] = s
            rs["cells"] = [int(((owner == k) & (third[None, :] == t)).sum()) for t in range(3)]
            o["cells"][s[3]] += rs["cells"]
            rs["within"] = 0
            if s[3] < 2:
                opp = np.nonzero(grp == 1 - s[3])[0]
                if len(opp):
                    dd = ((q[opp] - q[k]) ** 2).sum(1)
                    rs["near_d2"], rs["near_col"], rs["within"] = dd.min(), ss[opp[np.argmin(dd)]][2], (dd <= rq2).sum()
    _totals(rec, sites, totals)
    return rec, sites, totals, grid


# ---- definition two: a plain loop over cells and sites, Python integers -------------------------------------------------------------------
def space_scalar(values, columns, mapping, p, row0=0, n=0):
    check_params(p)
    groups = groups_of(columns, mapping, p["goalkeepers"])
    rows = values.shape[1]
    check_window(rows, row0, n)
    R, rq = p["cells_per_metre"], radius_q(p)
    rec, sites, totals, grid = _outputs(rows, groups, n, R)
    half = 512 // R
    for r in range(rows):
        ss = _row_sites(values, groups, r)
        o = rec[r]
        o["n_sites"] = len(ss)
        for s in ss:
            o["n"][s[3]] += 1
        o["status"] = EMPTY if not ss else TOO_MANY if len(ss) > SITE_CAP else ACTIVE
        if o["status"] != ACTIVE:
            continue
        cells = [[0, 0, 0] for _ in ss]
        for j in range(68 * R):
            for i in range(105 * R):
                best, own = None, -1
                for k, (qx, qy, _, _) in enumerate(ss):
                    d2 = ((2 * i + 1) * half - qx) ** 2 + ((2 * j + 1) * half - qy) ** 2
                    if best is None or d2 < best:
                        best, own = d2, k
                cells[own][third_of(i, R)] += 1
                if row0 <= r < row0 + n:
                    grid[r - row0, j, i] = own
        for k, (qx, qy, col, g) in enumerate(ss):
            rs = sites[r, k]
            rs["qx"], rs["qy"], rs["col"], rs["group"], rs["cells"] = qx, qy, col, g, cells[k]
            for t in range(3):
                o["cells"][g][t] += cells[k][t]
            if g == 2:
                continue
            best, bcol, within = -1, -1, 0
            for ox, oy, ocol, og in ss:
                if og != 1 - g:
                    continue
                d2 = (ox - qx) ** 2 + (oy - qy) ** 2
                if best < 0 or d2 < best:
                    best, bcol = d2, ocol
                within += d2 <= rq * rq
            rs["near_d2"], rs["near_col"], rs["within"] = best, bcol, within
    _totals(rec, sites, totals)
    return rec, sites, totals, grid
