"""The pass-option contract on the CPU (tests/options_ref.py, tests/options_cases.py): its two formulations agree bit for bit, every constructed case
forces what it is named after, and the header, the bindings and the host-side derivation of eagle_amd/options.py state the same thing.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import control_ref as CR
import options_cases as OC
import options_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _state(c, r, p):
    return OR.row_state(c["values"], c["vel"], c["columns"], c["mapping"], c["cand"], c["owner"], r, p["t_react"])


@pytest.mark.parametrize("run", OC.RUNS, ids=OC.run_id)
def test_the_two_formulations_agree_on_sampled_cells_and_options(run):
    c, p = OC.BY_NAME[run[0]], OC.BY_NAME[run[0]]["variants"][run[1]]
    grids, recs, opts = OC.reference(*run)
    gw, gh = CR.size(p["R"])
    rng = np.random.default_rng(7)
    step = max(1, c["n"] // 6)
    checked = 0
    for i in range(0, c["n"], step):
        st = _state(c, c["row0"] + i, p)
        assert st["status"] == recs[i]["status"]
        if st["status"] != OR.ACTIVE:
            assert not grids[i].any() and (opts[i] == -1).all() and recs[i]["best_col"] == -1 and recs[i]["best_byte"] == -1
            assert recs[i]["n_mates"] == 0 and recs[i]["n_defenders"] == 0 and recs[i]["sum"] == 0
            continue
        few = len(st["A"]) + len(st["D"]) <= 64
        cells = [(0, 0), (gw - 1, gh - 1), (gw - 1, 0)] + [(int(rng.integers(gw)), int(rng.integers(gh))) for _ in range(9 if few else 3)]
        bx, by = float(st["b"][0]), float(st["b"][1])
        if 0 <= bx < 105 and 0 <= by < 68:
            cells.append((int(bx * p["R"]), int(by * p["R"])))                 # the cell the ball is in
        for ci, cj in cells:
            cx, cy = OR.centre(ci, cj, p["R"])
            assert OR.byte_scalar(st["b"], st["A"], st["D"], cx, cy, **p) == grids[i][cj, ci], (i, ci, cj)
        for k in range(len(st["A"]) if few else min(4, len(st["A"]))):
            assert OR.byte_scalar(st["b"], st["A"], st["D"], st["A"][k, 0], st["A"][k, 1], **p) == opts[i][st["A_site"][k]], (i, k)
        assert recs[i]["sum"] == grids[i].astype(np.int64).sum()
        checked += 1
    assert checked


def test_the_two_formulations_agree_on_random_rows():
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(200):
        nA, nD = int(rng.integers(0, 5)), int(rng.integers(0, 7))
        far = rng.random() < 0.15
        A = (rng.uniform(-20, 125, (nA, 2)) * (30.0 if far else 1.0)).astype(F)
        D = (rng.uniform(-20, 125, (nD, 2)) * (30.0 if rng.random() < 0.15 else 1.0)).astype(F)
        b = rng.uniform((0, 0), (105, 68)).astype(F)
        p = OR.params(1, int(rng.choice([1, 2, 3, 7, 16, 64])), float(rng.choice([0.0, 0.7, 2.0])), float(rng.choice([0.5, 5.0, 9.0])),
                      float(rng.choice([0.5, 4.0, 40.0])), float(rng.choice([2.0, 15.0, 30.0])))
        t = rng.uniform((-5, -5), (110, 73), (6, 2)).astype(F)
        t[0] = b                                                            # L = 0
        if nA:
            t[1] = A[0]
        if nD:
            t[2] = D[0]
        vec = OR.bytes_at(b, A, D, t[:, 0], t[:, 1], **p)
        for k in range(len(t)):
            assert OR.byte_scalar(b, A, D, t[k, 0], t[k, 1], **p) == vec[k], (b, A, D, t[k], p)
        seen.update(int(x) for x in vec)
    assert {0, 255} <= seen and len(seen) > 50                              # the model is exercised over its whole range


def test_every_status_is_forced_on_consecutive_rows():
    c = OC.BY_NAME["statuses"]
    _, recs, opts = OC.reference("statuses", 0)
    assert recs["status"].tolist() == c["status"] and set(c["status"]) == {OR.ACTIVE, OR.NO_OWNER, OR.IN_FLIGHT, OR.NO_TEAM, OR.OFF_DOMAIN}
    assert all(a != b for a, b in zip(c["status"], c["status"][1:]) if OR.ACTIVE in (a, b))        # active rows stand between rows that are not
    cols = c["columns"]
    gk, p4, p5 = OC.col_of(cols, 6, OC.G), OC.col_of(cols, 4), OC.col_of(cols, 5)
    no_team = recs["owner_col"][recs["status"] == OR.NO_TEAM].tolist()
    assert no_team == [gk, p4, p5] and (recs["group"][recs["status"] == OR.NO_TEAM] == -1).all()
    assert [s[0] for s in OR.site_columns(cols, c["mapping"])] == [OC.col_of(cols, i) for i in (1, 2, 3, 7)]          # 4: no entry, 5: negative, 6: a goalkeeper
    v = c["values"][OC.col_of(cols, 0, OC.BALL)]
    on = [r for r in range(len(v)) if recs["status"][r] == OR.ACTIVE and abs(v[r, 0]) == 1024.0 and abs(v[r, 1]) == 1024.0]
    off = [r for r in range(len(v)) if recs["status"][r] == OR.OFF_DOMAIN]
    assert len(on) == 2 and len(off) == 3 and 1024.0 < v[off[0], 0] < 1024.0000001 and np.isnan(v[off[2], 0])
    r = c["status"].index(OR.ACTIVE, 1)
    assert recs["group"][r] == 1 and recs["n_mates"][r] == 1 and recs["n_defenders"][r] == 2           # group 1 owns the ball: team 0 defends


def test_site_count_cases_force_their_counts():
    g, recs, opts = OC.reference("sites_0_1_2", 0)
    assert not g.any() and (opts == -1).all() and (recs["status"] == OR.ACTIVE).all() and (recs["n_mates"] == 0).all() and recs["n_defenders"].tolist() == [0, 0, 1]
    for name in ("no_defenders", "no_defenders_group1"):
        g, recs, opts = OC.reference(name, 0)
        assert (g == 255).all() and (recs["n_defenders"] == 0).all() and (recs["n_mates"] == 2).all() and (recs["best_byte"] == 255).all()
        assert sorted(opts[0].tolist()) == [-1, 255, 255] and recs["best_col"].tolist() == [5, 4]
        assert (recs["sum"] == 255 * 7140).all()
    _, recs, opts = OC.reference("sites22", 0)
    assert opts.shape[1] == 22 and (recs["n_mates"] == 10).all() and (recs["n_defenders"] == 11).all()
    _, recs, opts = OC.reference("sites257_one_group", 0)
    assert recs["n_defenders"][0] == 257 and recs["n_mates"][0] == 2 and opts.shape[1] == 260
    _, recs, opts = OC.reference("sites1024", 0)
    assert opts.shape[1] == OR.MAX_SITES and recs["n_mates"][0] == 511 and recs["n_defenders"][0] == 512 and (opts[0] >= 0).sum() == 511
    c = OC.BY_NAME["sites1025"]
    assert len(OR.site_columns(c["columns"], c["mapping"])) == OR.MAX_SITES + 1 and not c["variants"]
    assert {OC.BY_NAME[n]["n"] for n in ("row1", "rows65", "rows257")} == {1, 65, 257}
    w = OC.BY_NAME["rows65_window"]
    assert w["row0"] > 0 and w["row0"] + w["n"] < 65
    assert np.array_equal(OC.reference("rows65_window", 0)[0], OC.reference("rows65", 0)[0][3:62])
    assert {p["K"] for p in OC.BY_NAME["sites22"]["variants"]} >= {1, 2, 3, 16, 64} and {p["R"] for p in OC.BY_NAME["sites22"]["variants"]} == {1, 2, 4}
    for name in ("rows65", "rows257"):
        assert len(set(OC.reference(name, 0)[1]["status"].tolist())) >= 3


def test_geometry_cases_force_their_seams():
    c = OC.BY_NAME["geometry"]
    p = c["variants"][0]
    g, recs, opts = OC.reference("geometry", 0)
    # row 0: the defender sits exactly on sample 8 of the lane to teammate 2; teammate 3 is as far away with a free lane
    st = _state(c, 0, p)
    f = F(8) / F(16)
    dx = st["A"][0, 0] - st["b"][0]
    assert (st["b"][0] + dx * f, st["b"][1]) == tuple(st["D"][0]) and dx == 32.0
    assert opts[0, 1] < opts[0, 2] - 100 and g[0][34, 52] < g[0][66, 20] - 100 and g[0][34, 60] < g[0][44, 60]
    assert g[0][34, 20] == OR.byte_scalar(st["b"], st["A"], st["D"], F(20.5), F(34.5), **p) and tuple(st["b"]) == OR.centre(20, 34, 1)       # L = 0
    # row 1: a defender at b
    st = _state(c, 1, p)
    assert any(tuple(d) == tuple(st["b"]) for d in st["D"])
    # row 2: equal bytes, the earlier column wins
    assert opts[2, 1] == opts[2, 2] >= 0 and recs["best_col"][2] == 2 and recs["best_byte"][2] == opts[2, 1]
    # row 3: the argument of d_expf clamps at both ends
    st = _state(c, 3, p)
    tr, vm, be = F(p["t_react"]), F(p["v_max"]), F(p["beta"])

    def arg(x, y):
        tD = tr + np.sqrt(OR._min_d2(np.array([x], F), np.array([y], F), st["D"])) / vm
        tA = tr + np.sqrt(OR._min_d2(np.array([x], F), np.array([y], F), st["A"])) / vm
        return float((-(be * (tD - tA)))[0])

    assert arg(*OR.centre(50, 34, 1)) > 88.0 and arg(*st["A"][0]) < -87.0
    assert g[3][34, 50] == 0 and opts[3, 1] == 255


def test_given_velocities_force_the_clamp_and_the_non_finite_rule():
    c = OC.BY_NAME["given_velocities"]
    st = _state(c, 0, OR.params(1))
    q = np.concatenate([st["A"], st["D"]])
    assert np.isfinite(q).all() and (np.abs(q) == CR.Q_LIM).any() and len(st["A"]) == 2 and len(st["D"]) == 3
    assert tuple(st["A"][0]) == (50.0, 10.0) and tuple(st["D"][0]) == (80.0, 30.0)          # NaN / inf / beyond fp32 count as 0
    st = _state(c, 0, c["variants"][1])
    assert tuple(st["D"][1]) == (12050.0, 60.0)                                                # 12 m/s for 1000 s: inside the clamp
    assert len({OC.reference("given_velocities", i)[0].tobytes() for i in range(4)}) >= 3


def test_header_declares_the_entries_and_lib_binds_them():
    from eagle_amd import lib
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name in ("eagle_pass_options_size", "eagle_pass_options_layout", "eagle_pass_options_device", "eagle_pass_options", "eagle_op_pass_options"):
        assert re.search(r"^int %s\(" % name, head, re.M) and name in lib.EXPORTS, name
    for name, v in (("ACTIVE", lib.PASS_ACTIVE), ("NO_OWNER", lib.PASS_NO_OWNER), ("IN_FLIGHT", lib.PASS_IN_FLIGHT), ("NO_TEAM", lib.PASS_NO_TEAM),
                    ("OFF_DOMAIN", lib.PASS_OFF_DOMAIN), ("MAX_SITES", lib.PASS_MAX_SITES)):
        assert re.search(r"#define EAGLE_PASS_%s %d\b" % (name, v), head), name
    assert (OR.ACTIVE, OR.NO_OWNER, OR.IN_FLIGHT, OR.NO_TEAM, OR.OFF_DOMAIN, OR.MAX_SITES) == (lib.PASS_ACTIVE, lib.PASS_NO_OWNER, lib.PASS_IN_FLIGHT, lib.PASS_NO_TEAM,
                                                                                              lib.PASS_OFF_DOMAIN, lib.PASS_MAX_SITES)
    assert lib.PASS_ROW_DTYPE == OR.ROW_DTYPE and lib.PASS_ROW_DTYPE.itemsize == 40 and C.sizeof(lib.EaglePassOptionParams) == 32
    body = re.search(r"typedef struct EaglePassOptionRow \{(.*?)\} EaglePassOptionRow;", head, re.S).group(1)
    assert [n for n in re.findall(r"\b([a-z_]+)(?=[,;])", re.sub(r"/\*.*?\*/", "", body, flags=re.S))] == list(OR.ROW_DTYPE.names)
    p = lib.pass_option_params()
    assert (p.cells_per_metre, p.samples, p.t_react, p.v_max, p.beta, p.v_ball) == (1, OR.SAMPLES, F(OR.T_REACT), F(OR.V_MAX), F(OR.BETA), F(OR.V_BALL))
    for name in ("pass_options", "pass_options_device", "pass_options_layout"):
        assert callable(getattr(lib.Handle, name))
    assert callable(lib.op_pass_options)
    c = OC.BY_NAME["statuses"]
    assert lib.pass_site_columns(c["columns"], c["mapping"]).tolist() == [s[0] for s in OR.site_columns(c["columns"], c["mapping"])]


def test_module_derives_the_event_figures_from_a_result():
    from eagle_amd import lib, options as op
    c = OC.BY_NAME["sites22"]
    p = c["variants"][0]
    _, recs, opts = OC.reference("sites22", 0)
    site_cols = [s[0] for s in OR.site_columns(c["columns"], c["mapping"])]
    owner = int(recs["owner_col"][1])
    mates = [site_cols[s] for s in np.flatnonzero(opts[1] >= 0)]
    ev = np.zeros(5, lib.EVENT_DTYPE)
    ev["kind"] = [lib.EVENT_PASS, lib.EVENT_PASS, lib.EVENT_TURNOVER, lib.EVENT_PASS, lib.EVENT_PASS]
    ev["release_row"] = [1, 1, 1, 1, 2]
    ev["from_col"] = [owner, owner, owner, mates[0], owner]
    ev["to_col"] = [mates[3], int(recs["best_col"][1]), mates[0], mates[1], 4 + 2 * 22]          # the last: the goalkeeper's column, never an option
    ev["row"] = ev["release_row"] + 1
    got = op.event_figures(ev, site_cols, recs, opts)
    assert [g["event"] for g in got] == [0, 1, 3, 4]                                            # PASS events only
    exp = [OR.event_figures(ev[k], site_cols, recs, opts) for k in (0, 1, 3, 4)]
    assert [(g["chosen"], g["best_byte"], g["best_col"], g["rank"]) for g in got] == [e if e[0] >= 0 else (-1, -1, None, None) for e in exp]
    assert exp[1][3] == 1 and exp[1][0] == recs["best_byte"][1] and exp[0][3] == 1 + int((opts[1] > exp[0][0]).sum()) and exp[2] == exp[3] == (-1, -1, -1, -1)
    # a window that does not hold the release row gives no figures
    assert op.event_figures(ev[:1], site_cols, recs[2:], opts[2:], row0=2)[0]["chosen"] == -1
