"""numpy restatement of the library's occupancy contract (include/eagle.h, eagle_post_occupancy / eagle_occupancy_picture / eagle_op_occupancy /
eagle_op_occupancy_picture; csrc/occupancy.hip): a processed table -> per SELECTION of its columns a map of where those columns spent their time, as
integer frame counts per pitch cell, as a Gaussian-smoothed float32 surface, as bytes for pictures, and as a still picture of the pitch.  It is the
single written definition of every output bit; the kernels equal it bit for bit, with no tolerances.

PARITY UNPINNED, OWN SPEC.  The reference derives no such map; its users draw one with mplsoccer's heatmap / kdeplot from processed_data.json.  The
binning, the frame weights, the truncated separable Gaussian and the picture are this project's own.

Selections.  A call computes n_sel maps.  Selection s is the list sel_cols[sel_off[s] : sel_off[s + 1]] of table column indices (CSR form; sel_off
ascends from 0).  Members must be pitch columns (video == 0) of kind Player, Goalkeeper or Ball.  A column may appear in several selections, not
twice in one.  An empty selection is legal and gives zeros.

Row weight (integer frames, shared by all columns): w[r] = f[r + 1] - f[r] when r + 1 < rows and that step is <= max_gap, otherwise 1 (the last row,
and the row in front of a hole).

Binning.  R in {1, 2, 4} cells per metre, gw = 105 R, gh = 68 R, grid row 0 is pitch y = 0 (the control grid's geometry, control_ref.size).  A cell of
the table is PRESENT when x and y are finite (the velocity rule).  A present cell with 0 <= x < 105 and 0 <= y < 68 (float64 comparisons) adds w[r] to
count[s][(int) floor(y R)][(int) floor(x R)] (x R and y R are exact: R is a power of two); any other present cell adds w[r] to outside[s]; an absent
cell adds nothing.  total[s] is the sum of what went inside.  -0.0 is inside; 105.0 and 68.0 are outside.  Counts are integers, so the result does not
depend on the order of accumulation.  Here they are int64; the library accumulates in 32 bits and therefore refuses a call in which
rows x max_gap x (the largest selection) reaches 2^31.

Smoothing (float32, no contraction, separable, zero outside the grid, no renormalisation at the borders).  s = (float) sigma * (float) R, rad = (int)
ceilf(3.0f * s), inv = 1.0f / (2.0f * s * s), t[k] = d_expf(-((float) (k * k)) * inv) for k = 0 .. rad (csrc/dmath.h; here oracle.prims.expf).  t[0]
is 1.0f: that is what the formula gives for every finite inv, and for a sigma so small (below about 4e-20 R) that s * s underflows and inv is
infinite it is the definition (the formula would be -0 x inf there).  sigma == 0 means rad = 0, t[0] = 1: the map is the counts converted to float32
(round to nearest even from 2^24 on).  Horizontal pass: hz[j][i] = the sum over k = -rad .. rad in ascending k, started from 0.0f, of t[|k|] * (float)
count[j][i + k]; terms whose i + k falls outside 0 .. gw - 1 are skipped; the multiply and the add round separately.  Vertical pass: v[j][i] = the
same sum over hz[j + k][i].  (Every term is >= +0, so adding a skipped term as t * 0.0f = +0.0f changes no bit: the kernel pads its tiles with zeros.)
The library accepts sigma in [0, 10] m, so rad <= 30 R <= 120, which is below gh = 68 R for every R; the functions here take any sigma, and
tests/test_occupancy_cpu.py checks the clipping of a rad beyond the grid on them.

Byte form (for pictures).  m = the largest v of the selection's grid; byte = m > 0 ? (int) floorf(v / m * 255.0f + 0.5f) : 0.

Picture.  A BGR canvas of the minimap's size for (scale S, margin M) (minimap_ref.size and its parameter checks), black.  A pixel (X, Y) of the pitch
rectangle reads cell i = ((X - M) R) / S, j = gh - 1 - ((Y - M) R) / S (integer divisions: the control layer's mapping in control_ref.py); with
a = c + (c >> 7) it takes per channel (colour_c * a + 128) >> 8 of a caller-given BGR colour.  The pitch markings minimap_ref.markings(S, M) go on top
in white.  No players, no ball, no footprint.

Host summary (eagle_amd/occupancy.py): seconds = v / fps in float64; thirds / channels = the shares of the inside time per 35 m third in x / per third
of 68 m in y, summed from the raw integer counts (exact), a cell counted by its centre."""
import numpy as np

import minimap_ref as MR
from oracle import prims

F = np.float32
PLAYER, GOALKEEPER, BALL, BOUNDARY = MR.PLAYER, MR.GOALKEEPER, MR.BALL, MR.BOUNDARY
RS = (1, 2, 4)
SIGMA, SIGMA_MAX = 2.0, 10.0                  # 2 m: a conventional choice, not fitted to data
PW, PH = 105, 68


def size(R):
    assert R in RS, R
    return PW * R, PH * R


def check_selections(columns, sel_off, sel_cols):
    sel_off, sel_cols = [int(v) for v in sel_off], [int(v) for v in sel_cols]
    assert len(sel_off) >= 1 and sel_off[0] == 0 and all(a <= b for a, b in zip(sel_off, sel_off[1:])) and sel_off[-1] == len(sel_cols)
    for s in range(len(sel_off) - 1):
        mem = sel_cols[sel_off[s]:sel_off[s + 1]]
        assert len(set(mem)) == len(mem), ("listed twice", s)
        for c in mem:
            assert 0 <= c < len(columns) and not columns[c][2] and columns[c][0] in (PLAYER, GOALKEEPER, BALL), (s, c)
    return sel_off, sel_cols


def weights(frames, max_gap):
    """int64 [rows]: the frames a row stands for"""
    f = np.asarray(frames, np.int64)
    assert max_gap >= 1 and (np.diff(f) > 0).all()
    w = np.ones(len(f), np.int64)
    if len(f) > 1:
        d = np.diff(f)
        w[:-1] = np.where(d <= max_gap, d, 1)
    return w


def histogram(values, frames, columns, sel_off, sel_cols, R, max_gap):
    """-> (count int64 [n_sel, gh, gw], total int64 [n_sel], outside int64 [n_sel])"""
    values = np.asarray(values, np.float64)
    sel_off, sel_cols = check_selections(columns, sel_off, sel_cols)
    gw, gh = size(R)
    n_sel = len(sel_off) - 1
    w = weights(frames, max_gap)
    count, outside = np.zeros((n_sel, gh * gw), np.int64), np.zeros(n_sel, np.int64)
    for s in range(n_sel):
        for c in sel_cols[sel_off[s]:sel_off[s + 1]]:
            x, y = values[c, :, 0], values[c, :, 1]
            present = np.isfinite(x) & np.isfinite(y)
            with np.errstate(invalid="ignore"):
                inside = present & (x >= 0.0) & (x < 105.0) & (y >= 0.0) & (y < 68.0)
            i = np.floor(x[inside] * np.float64(R)).astype(np.int64)
            j = np.floor(y[inside] * np.float64(R)).astype(np.int64)
            count[s] += _bincount(j * gw + i, w[inside], gh * gw)
            outside[s] += int(w[present & ~inside].sum())
    return count.reshape(n_sel, gh, gw), count.sum(1), outside


def _bincount(idx, w, n):
    out = np.zeros(n, np.int64)
    np.add.at(out, idx, w)                       # (integers: exact in any order)
    return out


def taps(sigma, R):
    """-> (rad, t float32 [rad + 1])"""
    if sigma == 0:
        return 0, np.ones(1, F)
    with np.errstate(all="ignore"):
        s = F(sigma) * F(R)
        rad = int(np.ceil(F(3.0) * s))
        inv = F(1.0) / (F(2.0) * s * s)
        k = np.arange(rad + 1, dtype=np.int64)
        t = prims.expf(-((k * k).astype(F)) * inv).astype(F)
    t[0] = F(1.0)
    return rad, t


def _pass(a, rad, t, axis):
    """one separable pass over float32 a [.., gh, gw] along `axis` (-1: horizontal, -2: vertical)"""
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1]
    out = np.zeros(a.shape, F)
    for k in range(-rad, rad + 1):
        lo, hi = max(0, -k), min(n, n - k)              # i with 0 <= i + k < n
        if lo >= hi:
            continue
        out[..., lo:hi] = out[..., lo:hi] + t[abs(k)] * a[..., lo + k:hi + k]
    assert out.dtype == F
    return np.moveaxis(out, -1, axis)


def smooth(count, sigma, R):
    """count int [n_sel, gh, gw] -> float32 [n_sel, gh, gw]"""
    rad, t = taps(sigma, R)
    c = np.asarray(count, np.int64).astype(F)
    return _pass(_pass(c, rad, t, -1), rad, t, -2)


def to_bytes(v):
    v = np.asarray(v, F)
    out = np.zeros(v.shape, np.uint8)
    for s in range(len(v)):
        m = v[s].max() if v[s].size else F(0)
        if m > 0:
            b = np.floor(v[s] / m * F(255.0) + F(0.5))
            assert b.dtype == F and b.min() >= 0 and b.max() <= 255
            out[s] = b.astype(np.int32).astype(np.uint8)
    return out


def occupancy(values, frames, columns, sel_off, sel_cols, R, sigma, max_gap):
    """values float64 [cols][rows][2], frames int [rows] strictly ascending, columns [(kind, id, video)] ->
    {"counts" int64 [n_sel, gh, gw], "total", "outside" int64 [n_sel], "grids" float32 [n_sel, gh, gw], "bytes" uint8 [n_sel, gh, gw]}"""
    count, total, outside = histogram(values, frames, columns, sel_off, sel_cols, R, max_gap)
    v = smooth(count, sigma, R)
    return {"counts": count, "total": total, "outside": outside, "grids": v, "bytes": to_bytes(v)}


def picture(byte_grid, R, S, M, colour):
    """a selection's bytes uint8 [gh, gw] -> BGR uint8 [h, w, 3]"""
    gw, gh = size(R)
    w, h = MR.size(S, M)
    byte_grid = np.asarray(byte_grid, np.uint8).reshape(gh, gw)
    img = np.zeros((h, w, 3), np.uint8)
    Y, X = np.mgrid[0:68 * S, 0:105 * S].astype(np.int64)
    c = byte_grid[gh - 1 - (Y * R) // S, (X * R) // S].astype(np.int64)
    a = c + (c >> 7)
    col = np.asarray(colour, np.int64)
    img[M:M + 68 * S, M:M + 105 * S] = ((col[None, None] * a[..., None] + 128) >> 8).astype(np.uint8)
    img[MR.markings(S, M)] = (255, 255, 255)
    return img


# ---- the host side of eagle_amd/occupancy.py ----------------------------------------------------------------------------------------------
def default_selections(columns, team_mapping):
    """-> (sel_off, sel_cols, names): one selection per Player / Goalkeeper pitch column in table order, one per team (the Player pitch columns with a
    mapping entry of that value, ascending team value: the Voronoi-site rule, goalkeepers are not in it; none without a mapping), and the ball (every
    Ball pitch column; an empty selection without one)"""
    off, cols, names = [0], [], []
    for c, (kind, ident, video) in enumerate(columns):
        if not video and kind in (PLAYER, GOALKEEPER):
            cols.append(c); off.append(len(cols))
            names.append({"kind": "player" if kind == PLAYER else "goalkeeper", "id": int(ident)})
    if team_mapping is not None:
        teams = {}
        for c, (kind, ident, video) in enumerate(columns):
            if not video and kind == PLAYER and ident in team_mapping:
                teams.setdefault(int(team_mapping[ident]), []).append(c)
        for t in sorted(teams):
            cols += teams[t]; off.append(len(cols))
            names.append({"kind": "team", "team": t})
    cols += [c for c, (kind, ident, video) in enumerate(columns) if not video and kind == BALL]
    off.append(len(cols))
    names.append({"kind": "ball"})
    return off, cols, names


def shares(count, R):
    """a selection's integer counts [gh, gw] -> (thirds [3], channels [3]): the shares of the inside time, a cell counted by its centre"""
    gw, gh = size(R)
    count = np.asarray(count, np.int64)
    cx, cy = (np.arange(gw) + 0.5) / R, (np.arange(gh) + 0.5) / R
    tot = int(count.sum())
    px, py = count.sum(0), count.sum(1)
    thirds = [int(px[(cx >= 35.0 * k) & (cx < 35.0 * (k + 1))].sum()) for k in range(3)]
    chans = [int(py[(cy >= 68.0 * k / 3.0) & (cy < 68.0 * (k + 1) / 3.0)].sum()) for k in range(3)]
    assert sum(thirds) == tot == sum(chans)
    return [n / tot if tot else 0.0 for n in thirds], [n / tot if tot else 0.0 for n in chans]
