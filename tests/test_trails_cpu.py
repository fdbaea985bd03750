"""The contract of the minimap's trail, pass-arrow and owner layers and of the two stills (tests/trails_ref.py) and its cases (tests/trails_cases.py),
without a GPU: every case forces the edge it is named after; with every layer off the contract is minimap_ref's; a numpy emulation of the kernel's
chunked, culled tile walk equals the direct contract; the refusals of the contract; the command line's refusals; the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import annot_ref as A
import minimap_cases as MC
import minimap_ref as R
import trails_cases as TC
import trails_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW, TH, STRIP = 256, 16, 8                                      # csrc/pix_out.h: the tile and the strip of the draw kernel


def _segs(c, row):
    return T.trail_segments(c["values"], c["frames"], c["columns"], c["mapping"], c["sel"], row, c["S"], c["M"], c["p"])


def test_event_dtype_is_the_library_s():
    from eagle_amd import lib
    assert TC.EVENT_DTYPE == lib.EVENT_DTYPE and TC.MM_CHUNK == 256
    assert (T.TRAILS, T.PASSES, T.OWNER) == (lib.MM_TRAILS, lib.MM_PASSES, lib.MM_OWNER)


def test_geometry_cases_force_their_edges():
    for name, tiles in (("x_seam", "x"), ("y_seam", "y"), ("both_seams", "xy"), ("arrow_across_both_seams", "xy")):
        c = TC.BY_NAME[name]
        pic = TC.reference(name)[0]
        base = T.draw_row(c["values"], c["frames"], c["columns"], c["mapping"], c["row0"], c["S"], c["M"], **c["kw"])
        ys, xs = np.nonzero((pic != base).any(-1))
        assert len(xs)
        if "x" in tiles:
            assert xs.min() < TW <= xs.max()
        if "y" in tiles:
            assert ys.min() // TH != ys.max() // TH
    for name in ("horizontal", "oblique_at"):                   # a pixel exactly at the half width: equality of the exact rule
        c = TC.BY_NAME[name]
        ax, ay, bx, by, hw16 = c["seg"]
        X, Y = c["at"]
        px, py, dx, dy = 16 * X - ax, 16 * Y - ay, bx - ax, by - ay
        t, L2, cross = px * dx + py * dy, dx * dx + dy * dy, px * dy - py * dx
        assert 0 < t < L2 and cross * cross == hw16 * hw16 * L2
        assert tuple(TC.reference(name)[0][Y, X]) == A.RED
    assert TC.BY_NAME["oblique_at"]["seg"][2] - TC.BY_NAME["oblique_at"]["seg"][0] == 2 * 48
    for name in ("horizontal", "beyond_straight", "oblique_beyond"):      # one sixteenth (or one pixel) further: not covered
        c = TC.BY_NAME[name]
        X, Y = c["beyond"]
        assert tuple(TC.reference(name)[0][Y, X]) != A.RED
    z = TC.BY_NAME["zero_length"]["seg"]
    assert z[:2] == z[2:4] and (TC.reference("zero_length")[0] == A.RED).all(-1).sum() > 40           # a disc
    c = TC.BY_NAME["endpoint_off_canvas"]
    assert c["seg"][2] < 0 and (TC.reference("endpoint_off_canvas")[0] == A.RED).all(-1).any()
    far = TC.BY_NAME["far_line"]
    assert np.abs(far["values"]).min() >= 1000.0 and (TC.reference("far_line")[0] == A.BLUE).all(-1).sum() > 200
    assert {TC.BY_NAME[n]["p"]["half_width"] for n in ("half_width_1", "half_width_8")} == {1, 8}


def test_wide_product_differs_under_a_64_bit_product():
    c = TC.BY_NAME["wide_product"]
    (ax, ay, bx, by, _), = _segs(c, 1)
    w, h = R.size(c["S"], c["M"])
    hw16 = 16 * c["p"]["half_width"]
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    cross = (16 * X - ax) * (by - ay) - (16 * Y - ay) * (bx - ax)
    assert int(np.abs(cross).min()) ** 2 >= 2 ** 64
    exact, wrapped = T.capsule_mask(ax, ay, bx, by, hw16, w, h), T.capsule_mask(ax, ay, bx, by, hw16, w, h, "wrap64")
    assert not exact.any() and wrapped.any()
    assert not T.capsule_mask(ax, ay, bx, by, hw16, w, h, "object").any()


def test_isqrt_form_equals_the_object_product():
    r = np.random.default_rng(0)
    for _ in range(40):
        ax, ay, bx, by = (int(v) for v in r.integers(-3000, 6000, 4))
        hw16 = 16 * int(r.integers(1, 9))
        assert np.array_equal(T.capsule_mask(ax, ay, bx, by, hw16, 210, 136), T.capsule_mask(ax, ay, bx, by, hw16, 210, 136, "object"))


def test_count_cases_have_exactly_the_named_count():
    for count in (0, 1, 255, 256, 257, 3 * 256 + 1):
        c = TC.BY_NAME["count_%d" % count]
        drawn = [s for s in c["sel"] if T.column_color(c["columns"], c["mapping"], s) is not None]
        row = c["row0"]
        per = row - max(1, row - c["p"]["window"] + 1) + 1
        assert len(drawn) * per == count and len(_segs(c, row)) == count


def test_presence_window_and_order_cases():
    c = TC.BY_NAME["nan_inf_beyond_domain"]
    ok = {s: T.points(c["values"], s, c["S"], c["M"])[2] for s in c["sel"]}
    assert not ok[0][3] and not ok[3][4] and not ok[5][2] and ok[0][2] and ok[0][4]
    assert len(_segs(c, 7)) == 4 * 7 - 6
    c = TC.BY_NAME["gap_at_and_beyond"]                          # steps of 3 (kept) and 4 (broken) frames at max_gap 3
    d = np.diff(c["frames"])
    assert 3 in d and 4 in d and len(_segs(c, 7)) == 4 * (7 - 1)
    c = TC.BY_NAME["row_0_and_r_below_W"]
    assert [len(_segs(c, r)) for r in range(4)] == [0, 4, 8, 12]
    assert len(_segs(TC.BY_NAME["window_1"], 2)) == 4 and len(_segs(TC.BY_NAME["window_beyond_rows"], 7)) == 28
    c = TC.BY_NAME["unmapped_player"]
    assert T.column_color(c["columns"], c["mapping"], 2) is None and {s[4] for s in _segs(c, 7)} <= {tuple((ch * f) >> 8 for ch in A.RED) for f in range(257)}
    assert all(s[4][0] == s[4][1] == s[4][2] for s in _segs(TC.BY_NAME["no_mapping"], 7))               # white, dimmed
    cols = {s[4] for s in _segs(TC.BY_NAME["goalkeeper_and_ball"], 7)}
    assert A.WHITE in cols and A.GREEN in cols
    assert not np.array_equal(TC.reference("two_columns_cross")[0], TC.reference("two_columns_cross_swapped")[0])
    pics = [TC.reference("self_crossing_floor_%d" % f)[0] for f in (0, 64, 256)]
    assert not np.array_equal(pics[0], pics[1]) and not np.array_equal(pics[1], pics[2])
    fl = TC.BY_NAME["self_crossing_floor_0"]
    assert [s[4] for s in _segs(fl, 3)] == [tuple((ch * f) >> 8 for ch in A.BLUE) for f in (256 - (2 * 256) // 3, 256 - 256 // 3, 256)]


def test_event_and_owner_cases():
    c = TC.BY_NAME["three_kinds"]
    assert sorted(int(k) for k in c["events"]["kind"]) == [0, 1, 2] and T.visible_events(c["events"], 3, 3) == [0, 1, 2]
    pic = TC.reference("three_kinds")[0]
    for col in T.EVENT_COLOR.values():
        assert (pic == col).all(-1).any()
    assert T.arrow(TC.BY_NAME["zero_length_arrow"]["events"][0], 2, 0, 2)[4] is None
    ab = TC.BY_NAME["absent_release_cell"]
    assert all(T.arrow(e, 2, 0, 2) is None for e in ab["events"])
    base = T.draw_row(ab["values"], ab["frames"], ab["columns"], ab["mapping"], 2, 2, 0)
    assert np.array_equal(TC.reference("absent_release_cell")[0], base)
    h1 = TC.BY_NAME["hold_1"]
    assert [len(T.visible_events(h1["events"], r, 1)) for r in range(6)] == [0, 1, 1, 1, 0, 0]
    assert T.visible_events(TC.BY_NAME["two_visible_in_order"]["events"], 3, 3) == [0, 1]
    many = TC.BY_NAME["events_257_visible"]
    assert len(T.visible_events(many["events"], many["row0"], many["p"]["pass_hold"])) == 257 > TC.MM_CHUNK
    ba = TC.BY_NAME["before_and_after_events"]
    vis = [len(T.visible_events(ba["events"], r, 2)) for r in range(9)]
    assert vis[0] == 0 and vis[-1] == 0 and max(vis) == 1
    ow = TC.BY_NAME["owner_kinds"]
    ref = TC.reference("owner_kinds")
    plain = [T.draw_row(ow["values"], ow["frames"], ow["columns"], ow["mapping"], r, 2, 0) for r in range(6)]
    changed = [not np.array_equal(ref[r], plain[r]) for r in range(6)]
    assert changed == [False, True, True, False, False, True]    # -1; a player; the goalkeeper; an absent cell; a skipped column; a player


def test_layers_off_is_the_minimap_contract():
    for c in MC.CASES:
        frames = np.arange(c["values"].shape[1], dtype=np.int32)
        got = T.frames_bgr(c["values"], frames, c["columns"], c["mapping"], c["row0"], c["n"], c["S"], c["M"], **c["kw"])
        assert np.array_equal(got, MC.reference(c["name"])), c["name"]


def _tile_walk(c, row):
    """the draw kernel's walk of the trail and arrow sections in numpy: per tile, entries in chunks of MM_CHUNK, culled by their grown box against the tile,
    painted strip by strip; over the contract's picture without those sections"""
    S, M, p = c["S"], c["M"], c["p"]
    w, h = R.size(S, M)
    hw = 16 * p["half_width"]
    plain = T.draw_row(c["values"], c["frames"], c["columns"], c["mapping"], row, S, M, 0, **c["kw"])
    img = T.draw_row(np.full_like(c["values"], np.nan), c["frames"], c["columns"], c["mapping"], row, S, M, 0, **c["kw"])      # layers 1 and 4 (no footprint here)
    discs = (plain != img).any(-1)                              # the opaque layers above the two sections
    prims = []
    if c["layers"] & T.TRAILS:
        prims += [(s[:4], None, s[4]) for s in _segs(c, row)]
    if c["layers"] & T.PASSES:
        for k in T.visible_events(c["events"], row, p["pass_hold"]):
            arw = T.arrow(c["events"][k], S, M, p["half_width"])
            if arw is not None:
                prims.append((arw[:4], arw[4], arw[5]))
    for ty0 in range(0, h, TH):
        for tx0 in range(0, w, TW):
            tx1, ty1 = min(tx0 + TW, w) - 1, min(ty0 + TH, h) - 1
            for base in range(0, len(prims), TC.MM_CHUNK):
                for (ax, ay, bx, by), head, color in prims[base:base + TC.MM_CHUNK]:
                    xs, ys = [ax - hw, bx - hw, ax + hw, bx + hw], [ay - hw, by - hw, ay + hw, by + hw]
                    if head is not None:
                        xs += [head[0], head[2]]; ys += [head[1], head[3]]
                    if not (min(xs) <= 16 * tx1 and max(xs) >= 16 * tx0 and min(ys) <= 16 * ty1 and max(ys) >= 16 * ty0):
                        continue
                    m = T.capsule_mask(ax, ay, bx, by, hw, w, h)
                    if head is not None:
                        Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
                        m |= A.covers((A.TRI, bx, by, head[0], head[1], head[2], head[3], color), 16 * X, 16 * Y)
                    tile = np.zeros_like(m)
                    tile[ty0:ty1 + 1, tx0:tx1 + 1] = True
                    img[m & tile] = color
    img[discs] = plain[discs]
    return img


@pytest.mark.parametrize("name", ["x_seam", "y_seam", "both_seams", "arrow_across_both_seams", "count_257"])
def test_chunked_culled_tile_walk_equals_the_contract(name):
    c = TC.BY_NAME[name]
    assert not c["layers"] & T.OWNER
    assert np.array_equal(_tile_walk(c, c["row0"]), TC.reference(name)[0])


def test_stills():
    for name, _ in TC.TRAJ:
        pic = TC.trajectory_reference(name)
        c = TC.trajectory_case(name)
        assert pic.shape == R.size(c["S"], c["M"])[::-1] + (3,) and (pic != 0).any()
    one, two = TC.trajectory_reference("window_1_row"), TC.trajectory_reference("window_2_rows")
    assert not np.array_equal(one, two)
    c = TC.trajectory_case("window_with_hole")
    assert not T.points(c["values"], 0, c["S"], c["M"])[2][3] and not T.points(c["values"], 3, c["S"], c["M"])[2].any()
    c = TC.pass_case()
    pic = TC.pass_reference()
    q = [R.quantise(c["values"][k, 1, 0], c["values"][k, 1, 1], c["S"], c["M"]) for k in range(3)]
    centre = lambda k: tuple(pic[int(q[k][1]) >> 4, int(q[k][0]) >> 4])
    # the bystander's disc reaches both centres: blended over the passer, who is drawn before it, and under the receiver, who is drawn after it
    assert centre(0) == tuple(int(v) for v in R._blend(np.array(A.RED, np.uint8), A.BLUE, T.DIM_A)) and centre(2) == A.RED
    assert centre(1) == A.RED and (pic == (64, 0, 0)).all(-1).any() and not (pic == A.BLUE).all(-1).any()      # the bystander: a quarter of blue where it shows
    assert abs(int(q[0][0]) - int(q[1][0])) == abs(int(q[2][0]) - int(q[1][0])) < 2 * 16 * R.radii(c["S"])[0]


def test_ref_refusals():
    c = TC.BY_NAME["pictures_3"]
    base = dict(window=1, max_gap=1, half_width=1, pass_hold=1, dim_floor=0)
    for bad in (dict(window=0), dict(max_gap=0), dict(half_width=0), dict(half_width=9), dict(pass_hold=0), dict(dim_floor=-1), dict(dim_floor=257)):
        with pytest.raises(ValueError):
            T.trail_params(**dict(base, **bad))
    for sel in ([1], [6], [-1], [0, 0]):                         # a video column, out of range twice, repeated
        with pytest.raises(ValueError):
            T.check_selection(sel, c["columns"])
    with pytest.raises(ValueError):
        T.check_selection([0], [(R.BOUNDARY, 0, 0)])
    args = (c["values"], c["frames"], c["columns"], c["mapping"], 0, 1, 2, 0)
    for kw in (dict(layers=8, p=c["p"]), dict(layers=1, p=None, sel=[0]), dict(layers=1, p=c["p"], sel=[]), dict(layers=2, p=c["p"]), dict(layers=4, p=c["p"])):
        with pytest.raises(ValueError):
            T.frames_bgr(*args, **kw)
    with pytest.raises(ValueError):
        T.trajectory_picture(c["values"], c["frames"], c["columns"], c["mapping"], [0], 7, 2, 2, 0)
    with pytest.raises(ValueError):
        T.pass_picture(c["values"], c["frames"], c["columns"], c["mapping"], TC.events([]), 0, 2, 0)


def test_cli_refusals(capsys):
    from eagle_amd import cli
    common = ["--frames", "2", "--fps", "5", "--synthetic-weights", "--out", "unused"]
    needs_minimap = "--minimap-trails and --minimap-passes draw into the minimap: they need --minimap"
    needs_processed = "--trajectory and --pass-pictures work on the processed table: they need --processed"
    rows = "--minimap-trails takes a number of rows of at least 1"
    ids = "--trajectory takes a comma list of ids or `ball`"
    for extra, message in ((["--minimap-trails"], needs_minimap), (["--minimap-passes"], needs_minimap), (["--processed", "--minimap-trails", "3"], needs_minimap),
                           (["--trajectory", "1,ball"], needs_processed), (["--pass-pictures"], needs_processed),
                           (["--processed", "--trajectory", "one"], ids), (["--processed", "--trajectory", "1,--1"], ids), (["--processed", "--trajectory", ""], ids),
                           (["--processed", "--minimap", "--minimap-trails", "-2"], rows), (["--processed", "--minimap", "--minimap-trails", "0"], rows),
                           (["--processed", "--minimap", "--minimap-trails", "many"], rows)):
        with pytest.raises(SystemExit) as e:
            cli.main(common + extra)
        assert e.value.code == 2 and message in capsys.readouterr().err, extra


def test_abi():
    from eagle_amd import lib
    assert C.sizeof(lib.EagleMinimapParams) == 32 and C.sizeof(lib.EagleTrailParams) == 32
    assert lib.EagleMinimapParams.layers.offset == 28
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name in ("eagle_minimap_set_trails", "eagle_trajectory_picture", "eagle_pass_picture", "eagle_op_minimap_trails", "eagle_op_trajectory_picture", "eagle_op_pass_picture"):
        assert re.search(r"\bint %s\(" % name, head) and name in lib.EXPORTS
    body = re.search(r"typedef struct EagleMinimapParams \{(.*?)\} EagleMinimapParams;", head, re.S).group(1)
    assert len(re.findall(r"int32_t", body)) == 7 and "layers" in body and "reserved" not in body       # (voronoi, footprint share a line): 8 fields of 4 bytes
    so = os.path.join(ROOT, "eagle_amd", "libeagle_hip.so")
    if os.path.exists(so):
        L = C.CDLL(so)
        assert all(hasattr(L, n) for n in lib.EXPORTS)
