"""The kinematics and pitch-control contract (tests/control_ref.py) means what it says, and the constructed tables (tests/control_cases.py) force the
edges they are named after; the argument checks that need no GPU.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import annot_ref as A
import control_cases as CC
import control_ref as CR
import minimap_ref as MR
from eagle_amd import lib

F = np.float32
P = MR.PLAYER


def _players(pts, teams):
    cols = [(P, i + 1, 0) for i in range(len(pts))]
    v = np.array(pts, np.float64).reshape(len(pts), 1, 2)
    return v, cols, {i + 1: t for i, t in enumerate(teams)}


def _times(values, vel, cols, mapping, R=1, **kw):
    q, team0 = CR.sites(values, vel, cols, mapping, 0, kw.get("t_react", CR.T_REACT))
    cx, cy = CR.centres(R)
    t = np.stack([F(kw.get("t_react", CR.T_REACT)) + np.sqrt((cx - x) * (cx - x) + (cy - y) * (cy - y)) / F(kw.get("v_max", CR.V_MAX)) for x, y in q])
    return t, team0


def _nearest_is_team0(values, cols, mapping):
    """minimap_ref's Voronoi label at every cell centre of the R = 1 grid: at S = 2, M = 0 pixel X = 2 i + 1 is x = (i + 0.5) m, Y = 136 - (2 j + 1)"""
    sites = [e for e in MR.draw_list(values, cols, mapping, 0, 2, 0) if e[4]]
    lab = MR.voronoi_labels(sites, 2, 0)
    i, j = np.meshgrid(np.arange(105), np.arange(68))
    return np.array([s[3] == A.RED for s in sites])[lab[136 - (2 * j + 1), 2 * i + 1]]


def test_standing_players_two_sites_agree_with_voronoi():
    values, cols, mapping = _players([(30.25, 20.0), (71.5, 44.75)], [0, 1])          # quarter metres: squared distances are exact in fp32
    vel = np.zeros_like(values)
    g = CR.grid(values, vel, cols, mapping, 0, 1)
    t, _ = _times(values, vel, cols, mapping)
    differ = t[0] != t[1]
    assert differ.sum() > 7000
    assert np.array_equal((g >= 128)[differ], _nearest_is_team0(values, cols, mapping)[differ])
    assert (g[~differ] == 128).all()


def test_standing_players_many_sites_sharp_softmin_agrees_with_voronoi():
    r = np.random.default_rng(3)
    pts = np.stack([r.integers(0, 420, 22) / 4.0, r.integers(0, 272, 22) / 4.0], 1)
    values, cols, mapping = _players(pts, [i % 2 for i in range(22)])
    vel = np.zeros_like(values)
    g = CR.grid(values, vel, cols, mapping, 0, 1, beta=1000.0)
    t, team0 = _times(values, vel, cols, mapping)
    clear = np.abs(t[team0].min(0) - t[~team0].min(0)) > 0.1                         # the two nearest opposing arrival times differ: e^-100 against 1
    assert clear.sum() > 5000
    near0 = _nearest_is_team0(values, cols, mapping)
    assert np.array_equal((g >= 128)[clear], near0[clear])
    assert set(np.unique(g[clear])) <= {0, 255}


def test_swapping_the_teams():
    c = CC.BY_NAME["sites22"]
    g = CC.grids("sites22", 1)[0][0].astype(int)
    swapped = {k: 1 - t for k, t in c["mapping"].items()}
    gs = CR.grid(c["values"], CC.velocities("sites22"), c["columns"], swapped, 0, 1).astype(int)
    assert np.abs(g + gs - 255).max() <= 1 and (g != gs).any()
    # a layout mirrored about the halfway line: the swapped grid is exactly the mirrored grid
    values, cols, mapping = _players([(40.25, 30.0), (64.75, 30.0)], [0, 1])
    vel = np.zeros_like(values); vel[0, 0], vel[1, 0] = (2.0, 1.0), (-2.0, 1.0)
    a = CR.grid(values, vel, cols, mapping, 0, 2)
    b = CR.grid(values, vel, cols, {1: 1, 2: 0}, 0, 2)
    assert np.array_equal(b, a[:, ::-1]) and a[60, 90] > 128 > a[60, 120]


def test_moving_toward_a_cell_owns_more_of_it():
    values, cols, mapping = _players([(40.0, 34.0), (60.0, 34.0)], [0, 1])
    still = np.zeros_like(values)
    moving = still.copy(); moving[0, 0] = (5.0, 0.0)
    a, b = CR.grid(values, still, cols, mapping, 0, 1), CR.grid(values, moving, cols, mapping, 0, 1)
    assert b[34, 50] > a[34, 50] and (b[:, 45:] >= a[:, 45:]).all()
    nanv = still.copy(); nanv[0, 0] = (np.nan, np.inf)
    assert np.array_equal(CR.grid(values, nanv, cols, mapping, 0, 1), a)               # a velocity that is not finite counts as 0


def test_cases_force_their_edges():
    B = CC.BY_NAME
    nsites = lambda name, row: len(CR.sites(B[name]["values"], CC.velocities(name), B[name]["columns"], B[name]["mapping"], row)[0])
    assert [nsites("sites_0_1_2", r) for r in range(3)] == [0, 1, 2]
    g, s = CC.grids("sites_0_1_2", 1)
    assert (g[0] == 128).all() and s[0] == 128 * 7140 and (g[1] == 255).all() and g[2].min() < 128 < g[2].max() and len(np.unique(g[2])) > 100
    assert (CC.grids("only_team0", 2)[0] == 255).all() and (CC.grids("only_others", 2)[0] == 0).all()
    assert nsites("sites22", 0) == 22 and nsites("sites257", 1) == 257 and nsites("rows65", 64) == 3
    assert B["rows257"]["values"].shape[1] == 257 and (B["rows257"]["row0"], B["rows257"]["n"]) == (0, 257)
    assert not np.any(CC.velocities("single_row")[np.isfinite(CC.velocities("single_row"))])
    # edges: 13 players, 3 beyond the domain, 4 not finite; on row 1 one more has left the domain; no goalkeeper, no unmapped player
    e = B["edges"]
    assert nsites("edges", 0) == 6 and nsites("edges", 1) == 5
    t, team0 = _times(e["values"][:, :1], CC.velocities("edges")[:, :1], e["columns"], e["mapping"])
    assert (-F(CR.BETA) * (t - t.min(0))).min() < -87.0                                # the exp argument passes its clamp
    assert np.array_equal(t[0], t[1]) and team0[0] != team0[1]                         # the two sites on one point
    v = CC.velocities("edges")
    assert np.hypot(*v[4 + 5, 0]) == pytest.approx(12.0) and np.isnan(v[4 + 7, 0]).all() and tuple(v[4 + 11, 0]) == (2.0, -1.0)
    # seams
    v, fr = CC.velocities("seams"), B["seams"]["frames"]
    assert fr[3] - fr[2] == 5 and fr[5] - fr[4] == 6
    assert tuple(v[0, 0]) == (3.0, 4.0) and tuple(v[0, 1]) == (3.0, 4.0)               # first row: one-sided; row 1: exactly at the cap, unscaled
    assert tuple(v[0, 3]) == (14.0 / 6.0, 0.0)                                         # a gap of exactly max_gap is differenced: (20 - 6) / (8 - 2)
    assert np.hypot(*v[0, 4]) == pytest.approx(5.0) and v[0, 4, 1] == 0.0              # 14 m/s, capped; the row behind it is 6 frames away
    assert tuple(v[0, 5]) == (3.0, 4.0) and tuple(v[0, 7]) == (4.0, 0.0)               # row 5 looks forward only; the last row looks back
    assert tuple(v[1, 1]) == (0.0, 0.0) and tuple(v[1, 6]) == (0.0, 0.0) and np.isnan(v[1, 4]).all() and np.isnan(v[1, 0]).all()
    assert np.allclose(np.hypot(v[2, :, 0], v[2, :, 1]), 5.0)                          # the video column, capped
    assert tuple(v[3, 0]) == (0.0, 0.0) and np.isnan(v[3, 1]).all()


def test_given_velocities_force_the_clamp_and_the_non_finite_rule():
    v, vel, cols, mapping = CC.given_velocities()
    q, team0 = CR.sites(v, vel, cols, mapping, 0)
    L = float(CR.Q_LIM)
    assert q.tolist() == [[L, -L], [80.0, 30.0], [50.0, 10.0], [float(F(50.0) + F(12.0) * F(0.7)), 60.0], [-L, float(F(50.0) + F(2.0) * F(0.7))]]
    assert CR.sites(v, vel, cols, mapping, 0, t_react=1000.0)[0][3].tolist() == [12050.0, 60.0]       # far, but inside the clamp
    g = CR.grid(v, vel, cols, mapping, 0, 1)
    still = vel.copy(); still[0, 0] = still[4, 0] = (0.0, 0.0)
    assert len(np.unique(g)) > 50 and (g != CR.grid(v, still, cols, mapping, 0, 1)).any()


def test_velocities_equal_numpy_gradient_on_a_gap_free_column():
    r = np.random.default_rng(1)
    for fps in (5, 25, 30):
        x = np.cumsum(r.normal(0, 0.2, (40, 2)), 0)
        v = CR.velocities(x[None], np.arange(40), fps, speed_cap=1e9)
        assert np.array_equal(v[0, :, 0], np.gradient(x[:, 0], 1.0 / fps)) and np.array_equal(v[0, :, 1], np.gradient(x[:, 1], 1.0 / fps))
    k = CR.kinematics(x[None], v, np.arange(40), [(P, 7, 0)], 30)
    sp = np.hypot(v[0, :, 0], v[0, :, 1])
    assert k[0]["id"] == 7 and k[0]["top_speed"] == sp.max() and k[0]["distance"] == pytest.approx(float(np.sum(0.5 * (sp[1:] + sp[:-1])) / 30.0))


def test_layer_colours():
    g = np.zeros((68, 105), np.uint8)
    g[:, 50:] = 255; g[:, 40:50] = 128
    col = CR.layer_colors(g, 1, 2, 0)
    assert tuple(col[0, 0]) == A.BLUE and tuple(col[0, 209]) == A.RED and tuple(col[0, 80]) == (127, 0, 128)      # a = 129: (255 * 127 + 128) >> 8, (255 * 129 + 128) >> 8
    assert CR.share([255 * 7140, 0, 128 * 7140], 1).tolist() == [1.0, 0.0, 128 / 255]


def test_parameter_checks_without_a_gpu():
    assert C.sizeof(lib.EagleMinimapParams) == 32 and C.sizeof(lib.EagleKinematicsParams) == 24 and C.sizeof(lib.EagleControlParams) == 32
    assert lib.control_size(lib.control_params(1)) == (105, 68) and lib.control_size(lib.control_params(4)) == (420, 272)
    for bad in (dict(cells_per_metre=3), dict(cells_per_metre=0), dict(cells_per_metre=8), dict(v_max=0.0), dict(v_max=-1.0), dict(beta=0.0), dict(beta=-4.0),
                dict(t_react=-0.1), dict(t_react=float("nan")), dict(v_max=float("inf")), dict(beta=float("nan"))):
        with pytest.raises(lib.EagleError):
            lib.control_size(lib.control_params(**bad))
    with pytest.raises(lib.EagleError, match="choose one"):
        lib.minimap_size(lib.minimap_params(2, 0, voronoi=True, control=True))
    assert lib.minimap_size(lib.minimap_params(2, 0, control=True)) == (210, 136)
    p = lib.minimap_params(2, 0)
    assert p.control == 0 and lib.kinematics_params(25).max_gap == 25 and lib.kinematics_params(25, 3, 9.0).speed_cap == 9.0


def test_cli_arguments(capsys):
    from eagle_amd import cli
    common = ["--frames", "2", "--synthetic-weights"]
    for extra, text in ((["--kinematics"], "need --processed"), (["--minimap-control"], "need --processed"), (["--control-grid", "2"], "need --processed"),
                        (["--processed", "--control-grid", "3"], "invalid choice: 3"),
                        (["--processed", "--minimap-control", "--minimap-voronoi"], "draw in the same slot")):
        with pytest.raises(SystemExit) as e:
            cli.main(common + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
