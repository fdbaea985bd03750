"""Constructed cases of line registration (K39) at the smallest shapes where the kernels can go wrong; tests/linefit_ref.py is the rule.  Each case is a
dict: name, frames uint8 [n, h, w, 3], Hs [n, 9], valid [n], boxes (None or a list of float32 [k, 4]), p (the contract's parameters) and expect, a function
of the contract's (Hs_out, records, masks) that asserts what the case is named after.  Two kinds of frames: DOTS, single white pixels on flat grass under a
matrix that maps pixel (x, y) to the Q point (X0 + step x, Y0 + step y), so a test chooses every q exactly; and VIEWS, the pitch lines drawn through an
axis-aligned matrix and then looked at through a disturbed one."""
import numpy as np

import linefit_ref as R

GRASS, WHITE, STANDS = (40, 120, 48), (235, 235, 235), (90, 70, 60)


def grass(h, w):
    f = np.empty((h, w, 3), np.uint8)
    f[:] = GRASS
    return f


def dots(h, w, pts, colour=WHITE):
    f = grass(h, w)
    for x, y in pts:
        f[y, x] = colour
    return f


def qmap(X0, Y0, step=1):
    """pixel (x, y) -> the Q point (X0 + step x, Y0 + step y), exactly"""
    return np.array([step / 1024.0, 0, X0 / 1024.0, 0, step / 1024.0, Y0 / 1024.0, 0, 0, 1.0])


def view(h, w, X0, Y0, s, half=0.13):
    """the pitch lines as seen by the matrix pixel -> (X0 + s x, Y0 + s y) metres: white where |e| <= half metres -> (frame, H)"""
    H = np.array([s, 0, X0, 0, s, Y0, 0, 0, 1.0])
    ys, xs = np.mgrid[0:h, 0:w]
    ok, qx, qy = R.points(H, xs.ravel().astype(float), ys.ravel().astype(float))
    prim, e = R.match(qx, qy)
    f = grass(h, w)
    f.reshape(-1, 3)[ok & (prim >= 0) & (np.abs(e) <= R.q(half))] = WHITE
    return f, H


def disturb(H, dx=0.0, dy=0.0, sx=1.0, sy=1.0, px=0.0):
    D = np.array([[sx, 0, dx], [0, sy, dy], [px, 0, 1.0]])
    return (D @ np.asarray(H).reshape(3, 3)).reshape(9)


def case(name, frames, Hs, p, expect=None, valid=None, boxes=None):
    frames = np.asarray(frames, np.uint8)
    if frames.ndim == 3:
        frames = frames[None]
    n = len(frames)
    Hs = np.asarray(Hs, np.float64).reshape(-1, 9)
    if len(Hs) == 1 and n > 1:
        Hs = np.repeat(Hs, n, 0)
    valid = np.ones(n, np.uint8) if valid is None else np.asarray(valid, np.uint8)
    return dict(name=name, frames=frames, Hs=Hs, valid=valid, boxes=boxes, p=p, expect=expect or (lambda out, rec, masks: None))


SMALL = dict(min_points=1, min_per_line=1)
CORNER = (16896, 14172)                                         # the left penalty area's lower outer corner: x = 16896 (prim 5) meets y = 14172 (prim 6)


def _n_line(*counts):
    def f(out, rec, masks):
        assert tuple(int(t) for t in rec["n_line"]) == counts, rec["n_line"]
        assert [int(np.unpackbits(m.view(np.uint8)).sum()) for m in masks] == list(counts)
    return f


def _status(*st, model=None, fall=None, kept=True):
    def f(out, rec, masks):
        assert tuple(int(t) for t in rec["status"]) == st, rec
        if model is not None:
            assert tuple(int(t) for t in rec["model"]) == model, rec["model"]
        if fall is not None:
            assert all(int(t) & fall == fall for t in rec["fall"]), rec["fall"]
    return f


def mask_cases():
    out = []
    p = R.params(rounds=1, **SMALL)
    out.append(case("smaller_than_2k_plus_1", dots(5, 7, [(3, 2)]), qmap(0, 0), p, _n_line(0)))
    # 0 / 1 / 63 / 64 / 65 / 257 line pixels: dots 2 k + 1 apart cannot vouch for each other
    for cnt in (0, 1, 63, 64, 65, 257):
        pts = [(4 + 9 * (i % 26), 4 + 9 * (i // 26)) for i in range(cnt)]
        out.append(case(f"dots_{cnt}", dots(9 * 10 + 9, 9 * 26 + 9, pts), qmap(CORNER[0] - 100, CORNER[1] - 50), p, _n_line(cnt)))
    # w = 70: three words per row, the last of 6 bits; pixels on both sides of each word seam and in the last admitted column
    pts = [(31, 4), (32, 13), (63, 4), (64, 13), (65, 22), (4, 22)]

    def seam(o, rec, masks):
        m = R.unpack_mask(masks[0], 70)
        assert masks.shape == (1, 30, 3) and sorted(zip(*np.nonzero(m)[::-1])) == sorted(pts)
    out.append(case("word_seams_w70", dots(30, 70, pts), qmap(CORNER[0] - 30, CORNER[1] - 10), p, seam))
    # the contrast at tau and one below (grass has Y = 328)
    f = dots(9, 30, [(5, 4)], (100, 150, 128))
    f[4, 15] = (100, 150, 127)
    out.append(case("tau_exact_and_one_below", f, qmap(0, 0), p, _n_line(1)))
    # the grass key at its two thresholds: g = 48 with a lead of 16 is grass; g = 47 and a lead of 15 are not
    f = dots(11, 60, [(8, 5), (24, 5), (40, 5)])
    f[:, :16], f[:, 16:32], f[:, 32:48] = (32, 48, 32), (31, 47, 31), (33, 48, 32)
    f[5, 8] = f[5, 24] = f[5, 40] = WHITE
    f[:, 48:] = STANDS
    out.append(case("grass_thresholds", f, qmap(0, 0), p, _n_line(1)))
    # a hit in one direction only
    f = dots(13, 40, [(10, 6), (28, 6)])
    f[2, 10], f[6, 24] = STANDS, STANDS                     # (10, 6): its upper neighbour is no grass; (28, 6): its left neighbour
    out.append(case("horizontal_only_and_vertical_only", f, qmap(0, 0), p, _n_line(2)))
    # a box widened by 3: x1 - 3 = 7 is inside (inclusive), 6 is outside; y likewise through y2 + 3 = 12
    f = dots(26, 40, [(6, 10), (7, 10), (15, 12), (15, 13), (20, 10)])

    def boxed(o, rec, masks):
        assert sorted(zip(*np.nonzero(R.unpack_mask(masks[0], 40))[::-1])) == [(6, 10), (15, 13)]
    out.append(case("box_inside_edge_outside", f, qmap(0, 0), p, boxed, boxes=[np.array([[10, 8, 25, 9]], np.float32)]))
    return out


def match_cases():
    out = []
    X0, Y0 = CORNER[0] - 20, CORNER[1] - 20
    tiny = R.params(rounds=1, radius=8 / 1024, radius_min=8 / 1024, **SMALL)
    # exactly on both lines (e = 0 twice, the earlier wins); just inside / outside a span; e^2 at rq^2 = 64 and one unit beyond
    pts = [(20, 20), (20, 19), (21, 20), (20, 29), (11, 20), (28, 40), (29, 4 + 20)]

    def units(o, rec, masks):
        assert R.match_scalar(X0 + 20, Y0 + 20) == (5, 0) and R.match_scalar(X0 + 20, Y0 + 19) == (6, -1) and R.match_scalar(X0 + 21, Y0 + 20)[0] == 5
        assert R.match_scalar(X0 + 28, Y0 + 40) == (5, 8) and R.match_scalar(X0 + 29, Y0 + 24) == (5, 9)
        assert int(rec["n_line"][0]) == 7 and int(rec["n_before"][0]) == 6 and int(rec["e2_before"][0]) == 66
    out.append(case("on_line_tie_span_radius", dots(48, 48, pts), qmap(X0, Y0), tiny, units))
    # either side of the left penalty arc's limit qx > 16896, at the arc's height there
    AX, AY = 16896 - 20, 27328 - 20

    def arc(o, rec, masks):
        assert R.match_scalar(AX + 21, AY + 20)[0] == 18 and R.match_scalar(AX + 20, AY + 20) == (5, 0) and R.match_scalar(AX + 19, AY + 20) == (5, -1)
    out.append(case("arc_limit", dots(40, 44, [(21, 20), (20, 29), (19, 11), (30, 20)]), qmap(AX, AY), R.params(rounds=1, **SMALL), arc))
    # every primitive as a target: a dot a quarter of a metre inside the pitch from a point of each (0.25 m per pixel)
    targets = []
    for o, c, a0, a1 in R.SEGMENTS:
        third = a0 + (a1 - a0) // 3                             # (a mid point of the touch lines lies on the halfway line)
        targets.append((c, third) if o == 0 else (third, c))
    targets += [(R.CX + 6626, R.CY + 6626), (11264 + 9370, R.CY), (96256 - 9370, R.CY)]
    pts = [(min(max(x // 256, 4), 423) + 8, min(max(y // 256, 4), 267) + 8) for x, y in targets]

    def every(o, rec, masks):
        hit = {R.match_scalar(*R.point_scalar([float(t) for t in qmap(-2048, -2048, 256)], x, y))[0] for x, y in pts}
        assert hit == set(range(R.NPRIM)), sorted(set(range(R.NPRIM)) - hit)
        assert int(rec["n_before"][0]) == len(set(pts))
    out.append(case("every_primitive", dots(290, 440, pts), qmap(-2048, -2048, 256), R.params(rounds=1, radius_min=2.5, **SMALL), every))
    # w' <= 0 for the upper half of the frame (w' = 2 y / (h - 1) - 1), a non-finite H, valid == 0
    f = dots(41, 48, [(20, 10), (20, 20), (20, 30)])
    Hw = qmap(X0, Y0)
    Hw[6:] = (0, 2 / 40, -1)
    Hn = qmap(X0, Y0)
    Hn[4] = np.nan

    def nomap(o, rec, masks):
        assert [int(t) for t in rec["status"]] == [R.UNCHANGED, R.NO_MAP, R.NO_MAP] or int(rec["status"][0]) != R.NO_MAP
        assert [int(t) for t in rec["status"][1:]] == [R.NO_MAP, R.NO_MAP] and [int(t) for t in rec["n_line"]] == [3, 3, 3]
        assert R.point_scalar([float(t) for t in Hw], 20, 20) is None and R.point_scalar([float(t) for t in Hw], 20, 30) is not None
        assert o[1].tobytes() == Hn.tobytes()
    out.append(case("w_nonpositive_nan_invalid", np.stack([f, f, f]), np.stack([Hw, Hn, qmap(X0, Y0)]), R.params(rounds=1, **SMALL), nomap, valid=[1, 1, 0]))
    return out


def ladder_cases():
    out = []
    p = dict(min_points=20, min_per_line=5)
    fa, Ha = view(96, 128, 2.0, 8.0, 0.25)                      # the left penalty and goal areas and the arc: two lines each way
    fb, Hb = view(96, 96, 10.0, 10.0, 0.25)                     # x = 16.5, y = 13.84 and the arc: three primitives
    fc, Hc = view(72, 64, 45.0, 2.0, 0.25)                      # the halfway line alone
    moved = lambda H: disturb(H, dx=0.4, dy=-0.3, sx=1.004)
    out.append(case("rung_projective", fa, moved(Ha), R.params(**p), _status(R.ACCEPTED, model=(3,))))
    out.append(case("rung_affine", fb, moved(Hb), R.params(**p), _status(R.ACCEPTED, model=(2,), fall=1 << (6 + R.LINES))))
    out.append(case("rung_translation_single_line", fc, moved(Hc), R.params(**p), _status(R.ACCEPTED, model=(1,), fall=(1 << (6 + R.LINES)) | (1 << (3 + R.LINES)))))
    out.append(case("rung_none_no_line", grass(40, 40), Ha, R.params(**p), _status(R.UNCHANGED, model=(0,), fall=0b001001001)))
    out.append(case("model_capped_at_translation", fa, moved(Ha), R.params(model=1, **p), _status(R.ACCEPTED, model=(1,), fall=0)))
    out.append(case("increment_beyond_cap", fa, moved(Ha), R.params(max_step=0.01, **p), _status(R.UNCHANGED, model=(0,), fall=0b100100100)))
    out.append(case("rejected_max_shift", fa, moved(Ha), R.params(max_shift=0.1, **p), _status(R.SHIFT)))
    out.append(case("rejected_min_points", fa, moved(Ha), R.params(min_points=100000, min_per_line=5), _status(R.FEW_POINTS)))
    # the true matrix and, besides the lines, a block of stray line pixels 1.5 m off the goal-area line: inside the round's radius, outside radius_min
    fn = fa.copy()
    for y in range(8, 90, 9):
        fn[y, 20] = WHITE
    out.append(case("rejected_no_gain", fn, Ha, R.params(rounds=1, **p), _status(R.NO_GAIN)))
    out.append(case("rounds_0", fa, moved(Ha), R.params(rounds=0, **p), _status(R.UNCHANGED, model=(0,))))
    out.append(case("rounds_1", fa, moved(Ha), R.params(rounds=1, **p), _status(R.ACCEPTED)))
    out.append(case("flipped_sign", fa, -moved(Ha), R.params(**p), _status(R.ACCEPTED, model=(3,))))
    # three dots on the goal line, the goal area's front line and its lower line: the affine rung has its lines and fails its pivot test
    out.append(case("pivot_three_dots", dots(48, 48, [(9, 30), (31, 40), (20, 19)]), qmap(-2048, 20480, 256), R.params(model=2, **SMALL),
                    _status(R.ACCEPTED, model=(1,), fall=1 << (3 + R.PIVOT))))
    # identical rows of stripes, mapped next to the far corner flag, where the rows of the normal matrix are longest
    fw = grass(40, 300)
    fw[:, 5::10] = WHITE
    out.append(case("long_rows_identical", fw, np.array([0.05, 0, 90.05, 0, 0.05, 66.0, 0, 0, 1.0]), R.params(radius=8, rounds=2, **p)))
    # frames side by side with different statuses: 3 and 65
    small, Hs_ = view(40, 48, 12.0, 10.0, 0.25)
    bad = Hs_.copy()
    bad[0] = np.inf
    trio = [(small, disturb(Hs_, dx=0.3), 1), (small, bad, 1), (grass(40, 48), Hs_, 1)]
    out.append(case("three_frames", np.stack([t[0] for t in trio]), np.stack([t[1] for t in trio]), R.params(**p), valid=[t[2] for t in trio]))
    many = [(small, disturb(Hs_, dx=0.05 * (i % 7), dy=-0.04 * (i % 5)), i % 11 != 3) for i in range(65)]
    many[9] = (grass(40, 48), Hs_, 1)
    many[20] = (small, bad, 1)

    def mixed(o, rec, masks):
        st = {int(t) for t in rec["status"]}
        assert {R.NO_MAP, R.ACCEPTED, R.UNCHANGED} <= st, st
    out.append(case("sixty_five_frames", np.stack([t[0] for t in many]), np.stack([t[1] for t in many]), R.params(**p), mixed, valid=[t[2] for t in many]))
    return out


def all_cases():
    return mask_cases() + match_cases() + ladder_cases()
