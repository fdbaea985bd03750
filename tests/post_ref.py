"""Restatement, in numpy alone, of the reference's clip post-processor as its ``main.py`` runs it (eagle/processor.py:30-403 with
``filter_ball_detections=False``): ``Processor.process_data(smooth)`` and ``Processor.format_data``.  It is the contract of
``eagle_postprocess`` (include/eagle.h); tests/golden/post_golden.json holds what the reference itself (pandas 2.3.3) returns on the clips of
tests/post_cases.py, and tests/test_post_cpu.py holds this file to it bit for bit.

A table is {"rows": kept frame numbers, "columns": names in the reference's order, "values": float64 [columns][rows][2] (NaN = missing),
"flags": FLAG_*, "team_mapping": {id: team}}.

Where the reference raises or returns garbage, this file (and the library) does something defined instead:
  * fewer than two ball sightings: the ball columns are all NaN and FLAG_NO_BALL is set (the reference hands the candidate lists on and fails);
  * ``Ball`` / ``Ball_video`` and the four boundary columns are always kept (the reference's 1 % filter can drop them, and format_data then
    raises KeyError);
  * the goalkeeper fold of an id needs all four of its columns (the reference raises KeyError when ``Goalkeeper_<id>`` was dropped);
  * ``filter_ball_detections=True`` is refused (NotImplementedError): it needs cv2's Kalman gain, which nothing here can pin."""
import numpy as np

BOUNDARIES = ("Bottom_Left", "Top_Left", "Top_Right", "Bottom_Right")
FLAG_NO_BALL = 1            # fewer than two ball sightings in the clip: Ball / Ball_video are all NaN
NAN2 = (np.nan, np.nan)
TRANSITION = np.array([[1, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)        # proc.py:510


def kalman_predict(state_post):
    """cv2.KalmanFilter.predict() of the reference's 4-state filter, the one step of OpenCV this file leans on -> (statePre, new statePost).

    ASSUMPTION (unpinned: no cv2 here to check it): predict computes statePre = transitionMatrix * statePost in float32 and then copies statePre
    into statePost; statePost starts as zeros, and the reference only ever writes the filter's statePre (proc.py:509), which predict overwrites.
    With filter=False nothing calls correct(), so the prediction is this recursion on zeros: it stays at the origin."""
    pre = (TRANSITION @ state_post).astype(np.float32)
    return pre, pre.copy()


def parse_ball_detections(detections):
    """parse_ball_detections_with_kalman(detections, filter=False), proc.py:321-403 -> (positions: (x, y) float32 pairs or None, enough)."""
    init, non_none, i = [], 0, 0
    while i < len(detections):                   # the initialisation window: at least 5 entries with at least 2 sightings (proc.py:326-337)
        if non_none >= 2 and len(init) >= 5:
            break
        init.append(None if detections[i] is None else detections[i][0])
        non_none += detections[i] is not None
        i += 1
    if non_none < 2:
        return [None] * len(detections), False   # (the reference returns `detections` itself here)
    # the window's interpolated start and mean velocity go into statePre only (proc.py:343-352): no effect on the output, see kalman_predict
    state_post = np.zeros((4, 1), np.float32)
    out = []
    for cand in detections:
        if cand is None or len(cand) == 0:
            out.append(None)
            continue
        best = cand[0]
        if len(cand) > 1:
            pre, state_post = kalman_predict(state_post)
            pred = np.array((pre[0, 0], pre[1, 0]))
            dist = [np.sqrt((np.array(c, np.float64) - pred).dot(np.array(c, np.float64) - pred)) for c in cand]     # np.linalg.norm of a vector
            best = cand[int(np.argmin(dist))]                                                                       # first minimum
        out.append((np.float32(best[0]), np.float32(best[1])))
    return out, True


def interp_positions(v, fill):
    """pandas' Series.interpolate(method="linear") on one float64 series: np.interp over row positions, slope * (x - x0) + y0 in float64.
    fill: then bfill and ffill (every row gets a value if one exists); else limit_area="inside" (rows outside the valid span stay NaN)."""
    v = np.array(v, np.float64)
    ok = np.flatnonzero(~np.isnan(v))
    if len(ok) == 0:
        return v
    for r in np.flatnonzero(np.isnan(v)):
        j = np.searchsorted(ok, r)
        if j == 0:
            v[r] = v[ok[0]] if fill else np.nan
        elif j == len(ok):
            v[r] = v[ok[-1]] if fill else np.nan
        else:
            x0, x1 = float(ok[j - 1]), float(ok[j])
            slope = (v[ok[j]] - v[ok[j - 1]]) / (x1 - x0)
            v[r] = slope * (float(r) - x0) + v[ok[j - 1]]
    return v


def interpolate_col(col, fill=False):
    """interpolate_df on one column [rows][2]: x and y are interpolated apart (proc.py:30-45)."""
    return np.stack([interp_positions(col[:, 0], fill), interp_positions(col[:, 1], fill)], 1) if len(col) else col


def smooth_col(col):
    """smooth_df (proc.py:48-61): every other row, from the first, is forgotten and interpolated back from its neighbours."""
    col = col.copy()
    col[::2] = np.nan
    return interpolate_col(col, False)


def _present(col):
    return ~(np.isnan(col[:, 0]) & np.isnan(col[:, 1]))


def create_dataframe(coords):
    """proc.py:127-203 -> (rows, {name: [rows][2]} in column order, flags)."""
    keys = list(coords.keys())
    cells, kept, ball_img, ball_real = {}, [], [], []
    for fn in keys:
        cur = coords[fn]
        row = {}
        for name, b in zip(BOUNDARIES, cur["Boundaries"]):
            row[name] = NAN2 if b is None else (float(b[0]), float(b[1]))
        cd = cur.get("Coordinates", {})
        has_person = False
        for name in ("Player", "Goalkeeper"):
            for pid, item in cd.get(name, {}).items():
                x1, y1, x2, y2 = item["BBox"]
                tc = item.get("Transformed_Coordinates")
                row[f"{name}_{pid}"] = (float(tc[0]), float(tc[1])) if tc else NAN2
                row[f"{name}_{pid}_video"] = ((x1 + x2) / 2, float(y2))
                has_person = True
        if cd.get("Ball"):
            img, real = [], []
            for item in cd["Ball"].values():
                x1, y1, x2, y2 = item["BBox"]
                center = ((x1 + x2) / 2, y2)
                real.append((item["Transformed_Coordinates"] or center, float(item["Confidence"])))
                img.append((center, float(item["Confidence"])))
            ball_img.append([c for c, _ in sorted(img, key=lambda e: e[1], reverse=True)])          # stable: equal confidences keep their order
            ball_real.append([c for c, _ in sorted(real, key=lambda e: e[1], reverse=True)])
        else:
            ball_img.append(None)
            ball_real.append(None)
        if has_person:
            cells[fn] = row
            kept.append(fn)
    img, enough = parse_ball_detections(ball_img) if keys else ([], False)
    real, _ = parse_ball_detections(ball_real) if keys else ([], False)
    real = [r if i is not None else None for r, i in zip(real, img)]
    names = []
    for fn in kept:                              # pd.DataFrame(dict of dicts).T: columns in order of first appearance
        names += [n for n in cells[fn] if n not in names]
    table = {n: np.array([cells[fn].get(n, NAN2) for fn in kept], np.float64).reshape(len(kept), 2) for n in names}
    pos = {fn: k for k, fn in enumerate(keys)}
    for name, series in (("Ball", real), ("Ball_video", img)):
        table[name] = np.array([NAN2 if series[pos[fn]] is None else series[pos[fn]] for fn in kept], np.float64).reshape(len(kept), 2)
    always = BOUNDARIES + ("Ball", "Ball_video")
    table = {n: c for n, c in table.items() if n in always or _present(c).sum() >= 0.01 * len(kept)}      # proc.py:202
    return [int(k) for k in kept], table, 0 if enough else FLAG_NO_BALL


def merge_data(table):
    """proc.py:205-319: the goalkeeper fold.  The pairwise id merge behind it never merges: its "overlap" test (proc.py:245-250,
    last_col >= first_cand or last_cand >= first_col) holds for any two non-empty columns, and empty columns do not survive the 1 % filter."""
    for gk in [n for n in table if "Goalkeeper" in n and "video" in n]:
        pid = gk.split("_")[1]
        quad = (f"Player_{pid}", f"Player_{pid}_video", f"Goalkeeper_{pid}", f"Goalkeeper_{pid}_video")
        if all(n in table for n in quad):
            for p, g in ((quad[0], quad[2]), (quad[1], quad[3])):
                table[g] = np.where(_present(table[p])[:, None], table[p], table[g])       # Player.combine_first(Goalkeeper)
                del table[p]
    return table


def process_data(coords, team_mapping=None, smooth=False, filter_ball_detections=False):
    """Processor(coords, frames, fps, filter_ball_detections=False).process_data(smooth) with get_team_mapping's result handed in."""
    if filter_ball_detections:
        raise NotImplementedError("filter_ball_detections=True needs cv2's Kalman gain (unpinned); the post-processor refuses it")
    rows, table, flags = create_dataframe(coords)
    if not rows:
        table = {}                               # df.empty: the reference returns the empty frame and {} (proc.py:75-76)
    else:
        for n in ("Ball", "Ball_video"):
            table[n] = interpolate_col(table[n], fill=True)
        table = merge_data(table)
        for n in table:
            table[n] = interpolate_col(table[n], False)
            if smooth:
                table[n] = smooth_col(table[n])
    names = list(table)
    values = np.stack([table[n] for n in names]) if names else np.zeros((0, len(rows), 2))
    return {"rows": rows, "columns": names, "values": values.reshape(len(names), len(rows), 2), "flags": flags,
            "team_mapping": dict(team_mapping or {}) if rows else {}}


def _cell(v):
    return None if np.isnan(v[0]) and np.isnan(v[1]) else (float(v[0]), float(v[1]))


def raw_data_rows(table):
    """The records ``df.to_json(orient="records")`` serialises: one {column: [x, y] | None} per kept frame."""
    return [{n: _cell(table["values"][c, r]) for c, n in enumerate(table["columns"])} for r in range(len(table["rows"]))]


def format_data(table):
    """Processor.format_data (proc.py:89-125): the rows of processed_data.json."""
    out = []
    cols = table["columns"]
    for r in range(len(table["rows"])):
        row = {n: _cell(table["values"][c, r]) for c, n in enumerate(cols)}
        real, video = [], []
        for n in cols:
            if n in BOUNDARIES or row[n] is None or "ball" in n.lower():
                continue
            item = {"ID": int(n.split("_")[1]), "Coordinates": row[n], "Type": n.split("_")[0]}
            (video if "video" in n else real).append(item)
        real.append({"ID": "Ball", "Coordinates": row["Ball"]})
        video.append({"ID": "Ball", "Coordinates": row["Ball_video"]})
        out.append({"Boundaries": [row[n] for n in BOUNDARIES], "Coordinates": real, "Coordinates_video": video})
    return out


def overlay_of_row(table, r, rec=None):
    """The primitives main.py:44-77 draws for processed row r, as eagle_overlay_from_table lists them: per video column in table order a foot arc
    and the id (goalkeepers green, team 0 red, other teams blue, players without a team skipped), the ball marker, then the record's key-points
    (taken from the library's own eagle_overlay_from_record: the same three sources as before).  -> [(kind, a0 .. a5, (b, g, r))]"""
    from eagle_amd import lib
    green, red, blue = (0, 255, 0), (0, 0, 255), (255, 0, 0)
    out = []
    tm = table["team_mapping"]
    for c, n in enumerate(table["columns"]):
        x, y = table["values"][c, r]
        if "video" not in n or n in BOUNDARIES or np.isnan(x) or np.isnan(y):
            continue
        x, y = int(x), int(y)
        if "Ball" in n:
            out.append((lib.PRIM_TRI, x, y - 20, x - 5, y - 30, x + 5, y - 30, green))
            continue
        pid = int(n.split("_")[1])
        if "Goalkeeper" in n:
            color = green
        elif pid in tm:
            color = red if tm[pid] == 0 else blue
        else:
            continue
        out.append((lib.PRIM_ARC, x, y, 0, 0, 0, 0, color))
        out.append((lib.PRIM_LABEL, x, y, pid, 0, 0, 0, color))
    if rec is not None:
        out += [(int(p["kind"]), *map(int, p["a"]), (int(p["b"]), int(p["g"]), int(p["r"]))) for p in lib.overlay_from_record(rec, None) if p["kind"] == lib.PRIM_DISC]
    return out
