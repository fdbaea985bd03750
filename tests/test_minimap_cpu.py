"""The minimap contract (tests/minimap_ref.py) against itself and against independent arithmetic, without a GPU: every constructed case of
tests/minimap_cases.py forces the edge it was built for, the markings hit their anchors, the integer Voronoi labelling equals a float64 arg-min
wherever that is decidable, and the library's struct and size entry agree with the contract's formula."""
import ctypes as C

import numpy as np
import pytest

import annot_ref as A
import minimap_cases as MC
import minimap_ref as R


def _bgr(color):
    return np.array(color, np.uint8)


def test_all_nan_row_is_markings_only():
    c = MC.BY_NAME["all_nan"]
    img = MC.reference("all_nan")[0]
    m = R.markings(c["S"], c["M"])
    assert m.any() and (img[m] == 255).all() and (img[~m] == 0).all()
    assert R.draw_list(c["values"], c["columns"], c["mapping"], 0, c["S"], c["M"]) == []


def test_tables_without_a_drawable_column():
    for name in ("no_drawable_columns", "only_unmapped_player"):
        c = MC.BY_NAME[name]
        assert all(R.draw_list(c["values"], c["columns"], c["mapping"], r, c["S"], c["M"]) == [] for r in range(c["values"].shape[1]))
    fr = MC.reference("no_drawable_columns")
    m = R.markings(2, 0)
    assert (fr[0][~m] == 0).all() and (fr[1][~m] != 0).any()           # row 1 has its footprint, row 0 markings only
    assert (MC.reference("only_unmapped_player")[0][~R.markings(2, 2)] == 0).all()


def test_tie_goes_to_the_earlier_column_and_the_swap_flips_exactly_the_tie_pixels():
    a, b = MC.BY_NAME["tie"], MC.BY_NAME["tie_swapped"]
    S, M = a["S"], a["M"]
    sa = [e for e in R.draw_list(a["values"], a["columns"], a["mapping"], 0, S, M) if e[4]]
    sb = [e for e in R.draw_list(b["values"], b["columns"], b["mapping"], 0, S, M) if e[4]]
    assert [e[:2] for e in sa] == [e[:2] for e in sb][::-1] and sa[0][3] != sa[1][3]
    w, h = R.size(S, M)
    Y, X = np.mgrid[0:h, 0:w].astype(np.int64)
    d = [(16 * X - e[0]) ** 2 + (16 * Y - e[1]) ** 2 for e in sa]
    tie = d[0] == d[1]
    assert tie.sum() == h and (X[tie] == 102).all()                    # the whole pixel column, canvas high
    la, lb = R.voronoi_labels(sa, S, M), R.voronoi_labels(sb, S, M)
    assert (la[tie] == 0).all() and (lb[tie] == 0).all()
    changed = (MC.reference("tie") != MC.reference("tie_swapped")).any(-1)[0]
    inside = (X >= M) & (X < M + 105 * S) & (Y >= M) & (Y < M + 68 * S)
    visible = tie & inside & ~R.markings(S, M) & (np.minimum(d[0], d[1]) > (16 * 1) ** 2)       # (tinted pixels nothing later paints over)
    assert visible.sum() > 0 and np.array_equal(changed, visible)


@pytest.mark.parametrize("name,count", [("sites1", 1), ("sites22", 22), ("sites65", 65), ("sites257", 257), ("sites300", 300)])
def test_site_cases_have_their_sites(name, count):
    c = MC.BY_NAME[name]
    for row in range(c["row0"], c["row0"] + c["n"]):
        lst = R.draw_list(c["values"], c["columns"], c["mapping"], row, c["S"], c["M"])
        assert sum(e[4] for e in lst) == count and len(lst) == count + 1 and lst[-1][2] == R.BALL


def test_edge_case_list():
    c = MC.BY_NAME["edges_voronoi"]
    lst = R.draw_list(c["values"], c["columns"], c["mapping"], 0, c["S"], c["M"])
    # 14 players, 7 of them absent (beyond 1024 m twice, NaN twice, +-inf, 1e30); then goalkeeper 50, not player 99, not the NaN goalkeeper; the ball
    present = [e for e in lst if e[2] == R.PLAYER]
    assert len(present) == 7 and all(e[4] for e in present)
    assert [e[2] for e in lst[len(present):]] == [R.GOALKEEPER, R.BALL] and lst[len(present)][3] == A.GREEN and not lst[len(present)][4]
    assert {e[3] for e in present} == {A.RED, A.BLUE}
    w, h = R.size(c["S"], c["M"])
    assert any(e[0] < 0 for e in present) and any(e[0] > 16 * w for e in present) and any(e[1] > 16 * h for e in present)
    img = MC.reference("edges_voronoi")[0]
    assert ((img == _bgr(A.GREEN)).all(-1)).any()
    white = MC.reference("no_mapping")[0]
    assert not ((white == _bgr(A.RED)).all(-1) | (white == _bgr(A.BLUE)).all(-1)).any() and (white == _bgr(A.GREEN)).all(-1).any()


def test_footprint_cases():
    c = MC.BY_NAME["footprints_a"]
    S, M = c["S"], c["M"]
    cs = [R.corners(c["values"], c["columns"], r, S, M) for r in range(5)]
    assert cs[0] is not None and cs[1] is not None and cs[2] is not None and cs[3] is None and cs[4] is None
    assert cs[1][0][0] > cs[1][3][0]                                  # crossed: xBL > xBR
    normal, crossed, off = (R.footprint_mask(cs[r], S, M) for r in range(3))
    assert normal.sum() > 1000 and crossed.sum() > 0 and off.sum() == 0
    assert not np.array_equal(MC.reference("footprint_crossed")[0], MC.reference("footprint_uncrossed")[0])
    uncrossed = R.footprint_mask([cs[1][3], cs[1][1], cs[1][2], cs[1][0]], S, M)       # the same corners with BL and BR exchanged
    assert not np.array_equal(crossed, uncrossed)
    fb = MC.reference("footprints_b")                                 # rows 3 and 4: no footprint, so no blended white anywhere
    grey = (255 * R.FOOT_A + 128) >> 8
    assert not (fb == grey).all(-1).any() and (MC.reference("footprints_a")[0] == grey).all(-1).any()


def test_stack_order():
    for name, kw in (("stack_default", {}), ("stack_explicit", {"player_radius": 7, "ball_radius": 16})):
        c = MC.BY_NAME[name]
        S, M = c["S"], c["M"]
        r, rb, t = R.radii(S, **kw)
        img = MC.reference(name)[0]
        cx, cy = M + int(52.5 * S), M + 34 * S
        assert tuple(img[cy, cx]) == (A.RED if rb - t > 0 else A.WHITE)                # inside the ring's hole: the disc, over the centre mark
        assert tuple(img[cy, cx + rb]) == A.WHITE and tuple(img[cy - rb, cx]) == A.WHITE       # the ring, over the disc or over the line
        if r > rb:
            assert tuple(img[cy, cx + rb + 1]) == A.RED
        assert tuple(img[cy, M + 11 * S]) == A.GREEN                   # the goalkeeper on the penalty mark


@pytest.mark.parametrize("S", [2, 4, 8, 32])
def test_marking_anchors(S):
    M = 2
    m = R.markings(S, M)
    px = lambda x, y: (M + int(round(x * S)), M + int(round((68 - y) * S)))
    on = [(0, 0), (0, 68), (105, 0), (105, 68), (52.5, 34), (52.5 + 9.15, 34), (52.5, 34 + 9.15), (11, 34), (94, 34), (16.5, 34), (88.5, 20), (5.5, 30), (99.5, 40),
          (11 + 9.15, 34), (94 - 9.15, 34)]
    off = [(8.25, 48), (96.75, 20), (52.5 + 5, 34), (52.5 - 3.5, 34 - 3.5), (11 - 9.15 + 0.2, 34), (30, 50)]
    for x, y in on:
        X, Y = px(x, y)
        assert m[Y, X], (S, x, y)
    for x, y in off:
        X, Y = px(x, y)
        assert not m[Y, X], (S, x, y)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_voronoi_equals_float64_argmin_where_decidable(seed):
    """22 uniformly random sites at S = 4, M = 2: the integer labelling of the quantised sites equals the float64 arg-min over the unquantised positions
    on every pitch pixel whose two nearest sites differ by at least 1 / 8 px in distance; the excluded share stays below 1 % (0.31 - 0.49 % measured)."""
    S, M = 4, 2
    r = np.random.default_rng(seed)
    x, y = r.uniform(0, 105, 22), r.uniform(0, 68, 22)
    qx, qy, ok = R.quantise(x, y, S, M)
    assert ok.all()
    lab = R.voronoi_labels(list(zip(qx.tolist(), qy.tolist())), S, M)
    w, h = R.size(S, M)
    Y, X = np.mgrid[M:M + 68 * S, M:M + 105 * S].astype(np.float64)
    fx, fy = M + x * S, M + (68 - y) * S                              # unquantised positions in pixels
    d = np.sqrt((X[..., None] - fx) ** 2 + (Y[..., None] - fy) ** 2)
    order = np.sort(d, -1)
    decidable = order[..., 1] - order[..., 0] >= 0.125
    excluded = 1.0 - decidable.mean()
    print(f"seed {seed}: excluded share {100 * excluded:.2f} %")
    assert excluded <= 0.01
    got = lab[M:M + 68 * S, M:M + 105 * S]
    assert np.array_equal(got[decidable], d.argmin(-1)[decidable])


def test_struct_size_and_minimap_size_equal_the_contract():
    from eagle_amd import lib
    assert C.sizeof(lib.EagleMinimapParams) == 32
    for S in range(R.S_MIN, R.S_MAX + 1, 2):
        for M in range(0, R.M_MAX + 1, 2):
            assert lib.minimap_size(lib.minimap_params(S, M)) == R.size(S, M) == (105 * S + 2 * M, 68 * S + 2 * M)
    for S, M in ((0, 0), (3, 0), (34, 0), (8, 1), (8, 66), (8, -2)):
        with pytest.raises(lib.EagleError):
            lib.minimap_size(lib.minimap_params(S, M))
