"""Constructed clips for the clip post-processor (eagle/processor.py:30-403 of the reference): each case is a list of frames given as the
detections the records would hold, from which both the library's input (EagleFrameResult records) and the reference's input (the
``get_coordinates`` dict, through eagle_amd/records.py) are built.  tests/golden/make_post_golden.py runs the reference on the dicts and writes
tests/golden/post_golden.json; tests/post_ref.py and the library are compared with that file.

A frame is {"persons": [(cls, id, x1, y1, x2, y2, pitch | None)], "balls": [(x1, y1, x2, y2, conf, pitch | None)], "bounds": (4 x) | None,
"H": bool}; cls 0 = Player, 1 = Goalkeeper."""
import numpy as np

from eagle_amd import lib, records

P, G = 0, 1


def person(cls, pid, fx, fy, pitch=(), wide=20):
    """A person whose foot point is (fx + wide / 2, fy); pitch () = derived from the foot point, None = no Transformed_Coordinates."""
    if pitch == ():
        pitch = (int(fx) % 106, int(fy) % 69)
    return (cls, pid, int(fx), int(fy) - 40, int(fx) + wide, int(fy), pitch)


def ball(cx, cy, conf=0.8, pitch=(), wide=6):
    if pitch == ():
        pitch = (int(cx) % 106, int(cy) % 69)
    return (int(cx), int(cy) - 6, int(cx) + wide, int(cy), conf, pitch)


def frame(persons=(), balls=(), bounds=(10.5, 12.25, 90.0, 95.75), H=True):
    return {"persons": list(persons), "balls": list(balls), "bounds": bounds, "H": H}


def _ball_track(t):
    return [ball(300 + 7 * t, 200 + 3 * t)]


def _base(T, ids=(3, 5), ball_every=3, bounds_rows=(1, 2)):
    """T frames, every id on every frame, a single ball candidate on every ball_every-th frame (0: never); boundaries on the frames bounds_rows
    only (None: on every frame), which keeps the golden small: the boundary columns then hold two cells and stay above the 1 % filter."""
    return [frame([person(P, i, 100 + 50 * k + 4 * t + (t * t) % 7, 400 + 10 * k + t, wide=20 + (k & 1)) for k, i in enumerate(ids)],
                  _ball_track(t) if ball_every and t % ball_every == 0 else [],
                  **({} if bounds_rows is None or t in bounds_rows else {"bounds": None})) for t in range(T)]


def _case(name, frames, fps=25, team_mapping=None, frame_w=1280):
    return {"name": name, "frames": frames, "fps": fps, "frame_w": frame_w, "team_mapping": dict(team_mapping or {})}


def _cases():
    out = []
    out.append(_case("empty", []))
    out.append(_case("no_persons", [frame([], _ball_track(t)) for t in range(8)]))
    out.append(_case("single_frame", [frame([person(P, 1, 100, 300)], [])]))

    fr = _base(24)
    for t in (5, 6, 7, 8, 14, 15):                 # id 5 vanishes twice and returns
        fr[t]["persons"] = [p for p in fr[t]["persons"] if p[1] != 5]
    out.append(_case("appear_vanish_return", fr, team_mapping={3: 0, 5: 1}))

    fr = _base(20, bounds_rows=None)
    for t in (0, 1, 2, 17, 18, 19):                # id 5 is missing at both ends: the inside rule leaves the gaps
        fr[t]["persons"] = [p for p in fr[t]["persons"] if p[1] != 5]
    for t in (9, 10):
        fr[t]["persons"] = [p for p in fr[t]["persons"] if p[1] != 5]
    for t in (0, 1, 19):
        fr[t]["bounds"] = None
    out.append(_case("gap_at_both_ends", fr, team_mapping={3: 0, 5: 1}))

    fr = _base(101, ids=(3,), ball_every=0)
    fr[0]["balls"] = fr[100]["balls"] = _ball_track(0)          # (a ball that does not move: short numbers in the golden)
    fr[40]["persons"].append(person(P, 77, 640, 360))           # 1 of 101 rows: below 1 % -> dropped
    fr[41]["persons"].append(person(P, 78, 640, 360))           # 2 of 101 rows: kept
    fr[42]["persons"].append(person(P, 78, 644, 361))
    out.append(_case("rare_id_dropped", fr, team_mapping={3: 0}))

    fr = _base(16, ids=(3,))
    for t in range(16):                            # id 9 is a Player on some frames, a Goalkeeper on others, nothing on a few
        if t in (0, 1, 2, 6, 7):
            fr[t]["persons"].append(person(P, 9, 700 + 3 * t, 500 + t))
        elif t in (4, 5, 10, 11, 12, 15):
            fr[t]["persons"].append(person(G, 9, 702 + 3 * t, 501 + t))
    out.append(_case("goalkeeper_fold", fr, team_mapping={3: 0, 9: 1}))

    fr = _base(14, ids=(3,))
    for t in range(14):                            # both on frames 4 .. 7: the Player value wins
        if t < 8:
            fr[t]["persons"].append(person(P, 9, 700 + 3 * t, 500 + t))
        if 4 <= t and t != 10:
            fr[t]["persons"].append(person(G, 9, 760 + 3 * t, 520 + t))
    out.append(_case("goalkeeper_fold_overlap", fr, team_mapping={3: 0, 9: 1}))

    fr = _base(12)
    for t in (2, 3, 7):                            # no pitch point: NaN on the pitch, present in the video columns
        fr[t]["persons"] = [person(c, i, x1, y2, pitch=None, wide=x2 - x1) if i == 5 else (c, i, x1, y1, x2, y2, p) for c, i, x1, y1, x2, y2, p in fr[t]["persons"]]
    out.append(_case("no_transformed_coordinates", fr, team_mapping={3: 0, 5: 0}))

    fr = _base(20)
    for t in (6, 7, 8, 9, 10, 13):                 # frames without persons leave the table: interpolation runs over row positions
        fr[t]["persons"] = []
    fr[4]["persons"] = fr[4]["persons"][:1]
    fr[5]["persons"] = fr[5]["persons"][:1]
    fr[11]["persons"] = fr[11]["persons"][:1]
    out.append(_case("frames_dropped", fr, team_mapping={3: 1, 5: 1}))

    out.append(_case("ball_none", _base(10, ball_every=0)))
    fr = _base(10, ball_every=0)
    fr[4]["balls"] = _ball_track(4)
    out.append(_case("ball_one_sighting", fr))
    fr = _base(10, ball_every=0)
    fr[2]["balls"] = _ball_track(2)
    fr[7]["balls"] = _ball_track(7)
    out.append(_case("ball_two_sightings", fr))

    fr = _base(12, ball_every=2)
    fr[2]["balls"] = [ball(300, 400, 0.9, pitch=(30, 40)), ball(400, 300, 0.7, pitch=(40, 30)), ball(500, 500, 0.5, pitch=(50, 50))]   # a tie at distance 500 / 50
    fr[4]["balls"] = [ball(400, 300, 0.6, pitch=(40, 30)), ball(300, 400, 0.95, pitch=(30, 40))]                                         # the same tie, confidence order swapped
    fr[6]["balls"] = [ball(900, 600, 0.9, pitch=(90, 60)), ball(120, 80, 0.4, pitch=(12, 8))]                                            # the less confident one is nearer
    out.append(_case("ball_candidates_tie", fr))

    fr = _base(12, ball_every=2)
    for t in (2, 4, 8):                            # no homography: the ball falls back to its image point on the pitch too
        fr[t]["H"] = False
    fr[6]["balls"] = [ball(310, 220, 0.9, pitch=None), ball(200, 100, 0.8)]
    out.append(_case("ball_no_homography", fr))

    fr = _base(14, ball_every=0)
    for t in (4, 6, 7, 9, 13):                     # four leading Nones: the initialisation window is 6 entries long
        fr[t]["balls"] = _ball_track(t)
    out.append(_case("ball_long_init_window", fr))

    out.append(_case("smooth_odd_rows", _gappy(15), team_mapping={3: 0, 5: 1}))
    out.append(_case("smooth_even_rows", _gappy(16), team_mapping={3: 0, 5: 1}))

    # ids 3 and 4 of one team at 5 frames/s: 4 appears one second after 3 left, 5 px away -> the intended rule would merge them; the reference's test never does
    for name, teams in (("would_merge_same_team", {3: 0, 4: 0, 8: 1}), ("would_merge_unknown_team", {8: 1})):
        fr = []
        for t in range(14):
            ps = [person(P, 8, 900 - 2 * t, 300 + t)]
            if t < 5:
                ps.append(person(P, 3, 200 + t, 400))
            if t >= 9:
                ps.append(person(P, 4, 208 + (t - 9), 403))
            fr.append(frame(ps, _ball_track(t) if t % 4 == 0 else [], bounds=(10.5, 12.25, 90.0, 95.75) if t in (1, 2) else None))
        out.append(_case(name, fr, fps=5, team_mapping=teams))
    return out


def _gappy(T):
    fr = _base(T)
    for t in (3, 4, 8):
        fr[t]["persons"] = [p for p in fr[t]["persons"] if p[1] != 5]
    fr[0]["persons"] = [p for p in fr[0]["persons"] if p[1] != 5]
    return fr


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


def records_of(case):
    """The EagleFrameResult records a clip with these detections would produce (the fields the post-processor reads)."""
    recs = np.zeros(len(case["frames"]), lib.RESULT_DTYPE)
    for r, f in zip(recs, case["frames"]):
        dets = [(c, i, x1, y1, x2, y2, 0.9, p) for c, i, x1, y1, x2, y2, p in f["persons"]]
        dets += [(2, k, x1, y1, x2, y2, conf, p) for k, (x1, y1, x2, y2, conf, p) in enumerate(f["balls"])]
        r["n_det"] = len(dets)
        r["H_valid"] = 1 if f["H"] else 0
        for d, (c, i, x1, y1, x2, y2, conf, p) in zip(r["det"], dets):
            d["cls"], d["id"], d["conf"], d["reported"] = c, i, conf, 1
            d["x1"], d["y1"], d["x2"], d["y2"] = x1, y1, x2, y2
            d["bx1"], d["by1"], d["bx2"], d["by2"] = x1, y1, x2, y2
            d["foot_x"], d["foot_y"] = int((x1 + x2) / 2), y2
            if p is not None:
                d["pitch_x"], d["pitch_y"], d["pitch_xf"], d["pitch_yf"], d["in_bounds"] = p[0], p[1], p[0], p[1], 1
        if f["bounds"] is not None:
            r["bounds_valid"] = 1
            r["bounds"] = f["bounds"]
    return recs


def coords_of(case, recs=None):
    """The reference's ``get_coordinates`` dict of the clip."""
    recs = records_of(case) if recs is None else recs
    return {i: records.to_reference_dict(r, i, case["fps"]) for i, r in enumerate(recs)}


def random_records(seed, rows, cols, occupancy):
    """A seeded random table as records: `rows` frames (every one kept: id 1 is always there), `cols` further person ids present with the given
    occupancy in runs, one id valid only in its first row, one only in its last, a goalkeeper / player pair, a ball every few frames."""
    rng = np.random.default_rng(seed)
    frames = [frame([person(P, 1, 50 + t % 900, 300 + t % 200)], bounds=(1.5 + t, 2.5, 80.0, 90.0 + t) if rng.random() < 0.9 else None) for t in range(rows)]
    for k in range(cols):
        pid, t = 10 + k, 0
        while t < rows:
            run = int(rng.integers(1, 2 + rows // 3 + 1))
            if rng.random() < occupancy:
                for u in range(t, min(rows, t + run)):
                    cls = G if (k % 5 == 4 and rng.random() < 0.5) else P
                    frames[u]["persons"].append(person(cls, pid, int(rng.integers(0, 1200)), int(rng.integers(60, 700)),
                                                       pitch=None if rng.random() < 0.1 else (), wide=int(rng.integers(10, 31))))
            t += run
    frames[0]["persons"].append(person(P, 5000, 640, 360))
    frames[-1]["persons"].append(person(P, 5001, 641, 361))
    if rows > 300:                                  # a gap that spans a whole 256-row block
        for t in list(range(1, 7)) + list(range(rows - 7, rows - 1)):       # (twelve rows: above the 1 % filter at 1025 rows)
            frames[t]["persons"].append(person(P, 5002, 7 * t % 1000, 100 + t % 500))
    for t in range(rows):
        if rng.random() < 0.3:
            frames[t]["balls"] = [ball(int(rng.integers(0, 1270)), int(rng.integers(10, 710)), float(rng.random())) for _ in range(int(rng.integers(1, 4)))]
    frames[0]["balls"] = frames[0]["balls"] or _ball_track(0)
    frames[-1]["balls"] = frames[-1]["balls"] or _ball_track(1)
    return _case(f"random_{seed}_{rows}x{cols}", frames, team_mapping={10 + k: k % 2 for k in range(0, cols, 2)})
