"""The physical-report contract without a GPU (tests/physical_ref.py; the kernels of csrc/physical.hip are held against it in tests/test_gpu_physical.py):
its two formulations (max-scans; a row-by-row state machine) agree bit for bit on every constructed table of tests/physical_cases.py and on seeded
random tables; every named case forces the edge it is named after; the invariants of totals and efforts hold; the numpy mirrors of the C structs have
the sizes the header states; what eagle_amd/physical.py derives on the host equals the contract's aggregates, and physical.json round-trips."""
import json

import numpy as np
import pytest

import physical_cases as PC
import physical_ref as PR

NAMES = [c["name"] for c in PC.CASES]
BITS = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    return (a["persons"] == b["persons"] and np.array_equal(BITS(a["speed"]), BITS(b["speed"])) and np.array_equal(BITS(a["accel"]), BITS(b["accel"]))
            and np.array_equal(a["zone"], b["zone"]) and a["totals"].tobytes() == b["totals"].tobytes() and a["efforts"].dtype == b["efforts"].dtype
            and a["efforts"].tobytes() == b["efforts"].tobytes())


def _invariants(res, c):
    f = c["frames"].astype(np.int64)
    rows = len(f)
    ev = res["efforts"]
    order = [(res["persons"].index(int(e["col"])), int(e["kind"]), int(e["first_row"])) for e in ev]
    assert order == sorted(order) and len(set(order)) == len(order)                     # ascending (person order, kind, first_row)
    for i, col in enumerate(res["persons"]):
        t = res["totals"][i]
        link, pres = res["link"][i], res["pres"][i]
        assert t["col"] == col and t["rows_present"] == pres.sum() and (t["reserved"] == 0).all()
        assert t["zone_frames"].sum() == (np.diff(f)[link[1:]].sum() if rows > 1 else 0)        # every linked step lies in exactly one zone
        assert t["zone_dist_q"].sum() == res["q"][i].sum() and (res["q"][i][~link] == 0).all()
        assert (res["zone"][i] == PR.ABSENT_ZONE).sum() == rows - pres.sum() and not link[~pres].any()
        for k in range(4):
            mine = ev[(ev["col"] == col) & (ev["kind"] == k)]
            assert len(mine) == t["efforts"][k]
            assert np.all(mine["last_row"][:-1] < mine["first_row"][1:])                # the efforts of a kind are disjoint
            for e in mine:
                a, b = int(e["first_row"]), int(e["last_row"])
                assert 0 <= a < b < rows and res["hot"][i, k, a:b + 1].all() and link[a + 1:b + 1].all()
                assert res["head"][i, k, a] and res["tail"][i, k, b] and e["frames"] == f[b] - f[a] >= c["min_frames"][0 if k < 2 else 1]
                assert e["distance_q"] == res["q"][i][a + 1:b + 1].sum() and e["peak_speed"] == res["speed"][i][a:b + 1].max() and e["reserved0"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_formulations_agree_and_invariants_hold(name):
    c = PC.BY_NAME[name]
    res = PC.reference(name)
    assert _same(res, PR.state_machine(*PC.args(c)))
    _invariants(res, c)


@pytest.mark.parametrize("seed", range(40))
def test_formulations_agree_on_random_tables(seed):
    r = np.random.default_rng(seed)
    fps = int(r.choice([1, 5, 25]))
    edges = np.sort(r.uniform(0.5, 9.0, 4))
    c = PC.walkers("random", int(r.integers(1, 5)), int(r.integers(1, 300)), 5000 + seed, fps=fps, max_gap=int(r.integers(1, 2 * fps + 1)),
                   zone_edges=tuple(edges + np.arange(4) * 1e-3), effort_speed=tuple(r.uniform(3.0, 8.0, 2)), accel=float(r.uniform(0.5, 6.0)),
                   min_frames=(int(r.integers(1, fps + 2)), int(r.integers(1, fps + 2))))
    res = PR.physical(*PC.args(c))
    assert _same(res, PR.state_machine(*PC.args(c)))
    _invariants(res, c)


def _efforts(res, person, kind):
    ev = res["efforts"]
    return [(int(e["first_row"]), int(e["last_row"])) for e in ev[(ev["col"] == PC.col_of(person)) & (ev["kind"] == kind)]]


def test_every_named_case_forces_its_edge():
    ref = PC.reference
    assert _efforts(ref("run_across_lanes_63_64"), 0, PR.HSR) == [(58, 70)]
    r = ref("run_across_rows_1023_1024")
    assert _efforts(r, 0, PR.SPRINT) == [(1019, 1030)] and _efforts(r, 1, PR.HSR) == [(1023, 1028)] and _efforts(r, 2, PR.HSR) == [(1024, 1030)]
    assert all(a < 1024 <= b for a, b in _efforts(r, 0, PR.HSR) + _efforts(r, 1, PR.HSR))           # first_row < 1024 <= last_row
    assert _efforts(ref("run_over_two_chunks"), 0, PR.HSR) == [(1000, 3100)]                        # chunks 1024 .. 2047 and 2048 .. 3071 lie inside
    assert _efforts(ref("run_from_row_0"), 0, PR.HSR) == [(0, 9)]
    assert _efforts(ref("run_to_the_last_row"), 0, PR.SPRINT) == [(1015, 1024)] and len(PC.BY_NAME["run_to_the_last_row"]["frames"]) == 1025
    r = ref("all_rows_hot")
    assert r["hot"][0, :2].all() and _efforts(r, 0, PR.HSR) == _efforts(r, 0, PR.SPRINT) == [(0, 1024)] and r["totals"][0]["efforts"].tolist() == [1, 1, 0, 0]
    r = ref("no_row_hot")
    assert not r["hot"].any() and len(r["efforts"]) == 0 and r["totals"][0]["zone_frames"].tolist() == [129, 0, 0, 0, 0]
    r = ref("speed_on_an_edge")
    assert _efforts(r, 0, PR.HSR) == [(5, 12)] and _efforts(r, 1, PR.HSR) == [] and r["speed"][1, 5] < 5.5 == r["speed"][0, 5]
    assert r["zone"][0, 5] == 3 and r["zone"][1, 5] == 2 and r["zone"][2, 5] == 1 and r["zone"][2, 0] == 0 and r["speed"][2, 0] == np.nextafter(2.0, 0.0)
    r = ref("duration_exactly_min_frames")
    assert _efforts(r, 0, PR.HSR) == [(10, 15)] and r["efforts"][0]["frames"] == PC.MIN_FRAMES[0] and r["tail"][0, PR.HSR, 34] and r["start"][0, PR.HSR, 34] == 30
    r, c = ref("step_of_max_gap"), PC.BY_NAME["step_of_max_gap"]
    assert c["frames"][13] - c["frames"][12] == c["max_gap"] and c["frames"][33] - c["frames"][32] == c["max_gap"] + 1
    assert _efforts(r, 0, PR.HSR) == [(8, 18), (26, 32), (33, 40)] and r["link"][0, 13] and not r["link"][0, 33]     # the longer step splits rows 26 .. 40 in two
    assert r["efforts"][0]["frames"] == 10 + c["max_gap"] - 1 and r["head"][0, PR.HSR, 33] and r["tail"][0, PR.HSR, 32]
    r = ref("absent_cell_splits_a_run")
    assert _efforts(r, 0, PR.HSR) == [(10, 19), (21, 30)] and r["zone"][0, 20] == PR.ABSENT_ZONE and np.isnan(r["speed"][0, 20])
    r = ref("accelerations_alternate")
    for person in (0, 1):
        acc, dec = _efforts(r, person, PR.ACCEL), _efforts(r, person, PR.DECEL)
        assert len(acc) > 100 and len(dec) > 100 and abs(len(acc) - len(dec)) <= 1
        both = sorted([(a, 2) for a, _ in acc] + [(a, 3) for a, _ in dec])
        assert all(x[1] != y[1] for x, y in zip(both, both[1:]))                                   # they alternate
        assert any(a < 1024 <= b for a, b in acc) if person == 0 else any(a == 1024 for a, b in dec)      # an effort across the chunk seam, one starting on it
    r = ref("half_quantum")
    assert r["q"][0].tolist() == [0, 1, 1, 2, 2, 3, 5, 8, 504, 1001]                                # a step of two equal speeds (k + 0.5) / 2^20: q = k + 1
    r = ref("distance_clamp")
    assert r["q"][0, 3] == r["q"][0, 7] == PR.Q * PR.Q and r["speed"][0, 6] * 0.1 > PR.D_CLAMP and r["q"][0, 1] == 104858
    assert r["totals"][0]["top_speed"] == 1e150 and r["totals"][0]["zone_dist_q"][4] == 2 * PR.Q * PR.Q + 2 * r["q"][0, 2] + 2 * r["q"][0, 6]
    r = ref("one_sided_neighbours")
    acc = r["accel"][0]
    assert acc[0] == (4.0 - 1.0) / (1.0 / 10.0) == acc[1] and acc[3] == (2.0 - 6.0) / (1.0 / 10.0) and acc[8] == (5.0 - 1.0) / (1.0 / 10.0) and acc[12] == 0.0
    assert acc[7] == (9.0 - 3.0) / (1.0 / 10.0) and not r["link"][0, 8] and r["link"][0, 9]         # row 7's next row is 23 frames away


def test_rows_and_persons_of_the_walks():
    for rows in PC.ROWS:
        for n in PC.PERSONS:
            r = PC.reference("walk_%d_rows_%d_persons" % (rows, n))
            assert r["speed"].shape == (n, rows) and len(r["totals"]) == n
    big = PC.reference("walk_2049_rows_3_persons")
    assert len(big["efforts"]) > 20 and set(big["efforts"]["kind"]) == {0, 1, 2, 3} and (~big["pres"]).any() and (big["totals"]["zone_frames"] > 0).all()


def test_struct_mirrors_and_params():
    import ctypes as C
    from eagle_amd import lib
    assert lib.LOAD_TOTALS_DTYPE == PR.TOTALS_DTYPE and lib.LOAD_EFFORT_DTYPE == PR.EFFORT_DTYPE
    assert lib.LOAD_TOTALS_DTYPE.itemsize == 128 and lib.LOAD_EFFORT_DTYPE.itemsize == 48 and C.sizeof(lib.EagleLoadParams) == 88
    assert lib.LOAD_Q == PR.Q and lib.LOAD_ABSENT == PR.ABSENT_ZONE
    p = lib.load_params(25)
    assert (p.fps, p.max_gap, list(p.min_frames), list(p.zone_edges), list(p.effort_speed), p.accel) == (25, 25, [12, 12], list(PR.ZONE_EDGES), list(PR.EFFORT_SPEED),
                                                                                                           PR.ACCEL_EDGE)
    assert list(lib.load_params(1).min_frames) == [1, 1] and list(lib.load_params(10, min_frames=(5, 3)).min_frames) == [5, 3] and PR.default_min_frames(25) == 12
    for name in ("eagle_post_physical", "eagle_post_physical_values", "eagle_post_physical_totals", "eagle_post_physical_efforts", "eagle_post_device_physical",
                 "eagle_op_physical"):
        assert name in lib.EXPORTS


def test_module_derives_the_contract_aggregates_and_json_round_trips():
    from eagle_amd import lib, physical as ph
    name = "walk_1025_rows_3_persons"
    c, res = PC.BY_NAME[name], PC.reference(name)
    columns = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    p = lib.load_params(c["fps"], c["max_gap"], c["zone_edges"], c["effort_speed"], c["accel"], c["min_frames"])
    d = ph.derive(res["speed"], res["accel"], res["zone"], res["totals"], res["efforts"], columns, c["frames"], c["fps"], ph.params_dict(p))   # a faked GPU result
    exp = PR.aggregates(res, c["columns"], c["fps"])
    assert len(d["players"]) == 3 and [pl["type"] for pl in d["players"]] == ["Player", "Player", "Goalkeeper"]
    for got, want in zip(d["players"], exp):
        assert {k: got[k] for k in want} == want
        assert sum(got["zone_distance_q"]) == got["distance_q"] and got["distance"] == got["distance_q"] / 2 ** 20      # the zones add up exactly
    assert len(d["efforts"]) == len(res["efforts"]) > 0
    e, g = res["efforts"][0], d["efforts"][0]
    assert g == {"id": c["columns"][int(e["col"])][1], "kind": PR.KIND_NAMES[int(e["kind"])], "first_row": int(e["first_row"]), "last_row": int(e["last_row"]),
                 "first_frame": int(c["frames"][e["first_row"]]), "last_frame": int(c["frames"][e["last_row"]]), "seconds": int(e["frames"]) / c["fps"],
                 "distance_q": int(e["distance_q"]), "distance": int(e["distance_q"]) / 2 ** 20, "peak_speed": float(e["peak_speed"]), "peak_accel": float(e["peak_accel"])}
    short = json.loads(json.dumps(ph.to_json(d)))                                                   # the file without the per-row arrays
    assert set(short) == {"params", "players", "efforts"} and ph.from_json(short)["players"] == d["players"]
    j = json.loads(json.dumps(ph.to_json(d, rows=True)))
    assert set(j) == {"params", "players", "efforts", "speed", "accel", "zone"} and j["params"]["zone_edges"] == list(c["zone_edges"])
    assert j["speed"][0][int(np.flatnonzero(~res["pres"][0])[0])] is None and None in j["zone"][0]
    back = ph.from_json(j)
    assert back["players"] == d["players"] and back["efforts"] == d["efforts"] and np.array_equal(back["zone"], res["zone"])
    assert np.array_equal(BITS(back["speed"]), BITS(res["speed"])) and np.array_equal(BITS(back["accel"]), BITS(res["accel"]))


def test_contract_refuses_bad_parameters():
    c = PC.BY_NAME["run_from_row_0"]
    v, f, cols = c["velocities"], c["frames"], c["columns"]
    bad = [dict(fps=0), dict(max_gap=0), dict(min_frames=(0, 1)), dict(min_frames=(1, -1)), dict(zone_edges=(2.0, 2.0, 5.5, 7.0)), dict(zone_edges=(0.0, 2.0, 5.5, 7.0)),
           dict(zone_edges=(2.0, 4.0, 5.5, float("inf"))), dict(zone_edges=(2.0, float("nan"), 5.5, 7.0)), dict(effort_speed=(0.0, 7.0)), dict(effort_speed=(5.5, float("nan"))),
           dict(accel=0.0), dict(accel=float("inf"))]
    for kw in bad:
        args = dict(fps=10, max_gap=10, zone_edges=PR.ZONE_EDGES, effort_speed=PR.EFFORT_SPEED, accel=2.0, min_frames=(5, 5))
        args.update(kw)
        with pytest.raises(ValueError):
            PR.physical(v, f, cols, **args)
    with pytest.raises(ValueError):
        PR.physical(v, f, [(9, 1, 0)] + list(cols[1:]), 10)
