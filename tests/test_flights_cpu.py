"""The ball-flight contract on the host (tests/flights_ref.py): it agrees with itself (every integer and decision is computed twice), its dynamic program
finds the least total of every admissible segmentation of the short runs and the path the tie rule selects, its float64 cost quantises like the exact
rational cost, the constructed cases are what their names say, and the demonstration clip (flights_cases.demo, seed DEMO_SEED = 0) meets the stated
conditions.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import flights_cases as FC
import flights_ref as FR

NAMES = [c["name"] for c in FC.CASES]
SMALL = [c["name"] for c in FC.CASES if len(c["frames"]) <= 60]
TWICE = [c["name"] for c in FC.CASES if len(c["frames"]) * FC.params_of(c)["max_rows"] <= 30000]


def _paths(res):
    """the knot lists of the runs, from the flight records"""
    out = []
    for first, last in res["runs"]:
        fl = [f for f in res["flights"] if first <= f["row0"] and f["row1"] <= last]
        out.append([int(fl[0]["row0"])] + [int(f["row1"]) for f in fl])
    return out


@pytest.mark.parametrize("name", TWICE + ["demo"])
def test_reference_agrees_with_itself(name):
    if name == "demo":
        d = FC.demo(FC.DEMO_SEED)
        c, p = dict(values=d["values"], frames=d["frames"], columns=d["columns"], cuts=None), FR.params(d["fps"], 25)
        a = FR.flights(c["values"], c["frames"], c["columns"], p)
    else:
        c, p, a = FC.BY_NAME[name], FC.params_of(FC.BY_NAME[name]), FC.reference(name)
    b = FR.second(c["values"], c["frames"], c["columns"], p, c["cuts"])
    prep = a["prep"]
    assert [tuple(int(v) for v in row) for row in b["q"]] == [tuple(v) for v in prep["q"]]
    for k in ("present", "head", "spike"):
        assert b[k].tolist() == prep[k], k
    assert b["runs"] == a["runs"] and b["best"] == a["best"] and b["knots"] == _paths(a)
    # the costs: incrementally from every start row against the listed samples of the pair
    frames = [int(v) for v in c["frames"]]
    for first, last in a["runs"]:
        for i in range(first, last):
            if prep["used"][i]:
                for j, v in FR.costs_from(prep["q"], frames, prep["used"], i, last, p["max_rows"]).items():
                    assert v[0] == b["cost"][(i, j)], (i, j)
    assert int(a["totals"]["sum_c"][0]) == sum(int(f["c"]) for f in a["flights"]) and int(a["totals"]["flights"][0]) == len(a["flights"])
    assert int(a["totals"]["knots"][0]) == sum(len(k) - 2 for k in b["knots"]) and int(a["totals"]["spikes"][0]) == int(b["spike"].sum())


def test_dynamic_program_against_every_segmentation():
    tried = 0
    for name in SMALL:
        c, p, a = FC.BY_NAME[name], FC.params_of(FC.BY_NAME[name]), FC.reference(name)
        prep, frames = a["prep"], [int(v) for v in c["frames"]]
        for n, (first, last) in enumerate(a["runs"]):
            if sum(prep["used"][first:last + 1]) > 10:
                continue
            total, path = FR.brute_force(prep["q"], frames, prep["used"], first, last, p["max_rows"], FR.lam_of(p))
            assert total == a["best"][n] and path == _paths(a)[n], (name, first, last)
            tried += 1
    assert tried >= 12                                             # the 12 runs of `shots` at the least
    # and on short random runs with ties (positions on a coarse grid, penalty 0 and small)
    rng = np.random.default_rng(5)
    for k in range(40):
        n = int(rng.integers(3, 11))
        ball = np.round(rng.uniform(0, 3, (n, 2)) * 4) / 4 if k % 2 else np.cumsum(np.round(rng.uniform(-1, 1, (n, 2)) * 2) / 2, 0)
        values, frames, cols = FC.table(ball)
        p = FR.params(25.0, 4, max_rows=int(rng.integers(2, 6)), penalty=float(rng.choice([0.0, 1.0, 16.0])), spike=float(rng.choice([0.5, 1024.0])))
        a = FR.flights(values, frames, cols, p)
        total, path = FR.brute_force(a["prep"]["q"], list(map(int, frames)), a["prep"]["used"], 0, n - 1, p["max_rows"], FR.lam_of(p))
        assert total == a["best"][0] and path == _paths(a)[0], k


@pytest.mark.parametrize("name", SMALL)
def test_float_cost_quantises_like_the_exact_cost(name):
    c, p, a = FC.BY_NAME[name], FC.params_of(FC.BY_NAME[name]), FC.reference(name)
    prep, frames = a["prep"], [int(v) for v in c["frames"]]
    half = Fraction(1, 2)
    compared = near_half = 0
    for first, last in a["runs"]:
        urows = [r for r in range(first, last + 1) if prep["used"][r]]
        for i in urows:
            for j in urows:
                if not (i < j and j - i <= p["max_rows"]):
                    continue
                sums = FR.pair_sums(prep["q"], frames, prep["used"], i, j)
                exact = FR.line_cost_exact(*sums)
                got = FR.line_cost(*sums)[0]
                if exact >= 1 << 40:
                    assert got == 1 << 40
                    continue
                # the float solve's error: a few roundings of terms as large as Q_x + Q_y, each 2^-53 relative; 2^-46 (Q_x + Q_y + 1) is generous
                err = Fraction(sums[5] + sums[8] + 1, 1 << 46)
                frac = exact - (exact.numerator // exact.denominator)
                down = exact.numerator // exact.denominator
                if abs(frac - half) <= err:
                    # A half-integer within the float solve's error: neither rounding is wrong.  Such pairs cannot be drawn away: the cost of three
                    # evenly spaced samples is (ex^2 + ey^2) / 6 with e = q0 - 2 q1 + q2, an exact half-integer for one draw in six.
                    assert got in (down, down + 1), (i, j)
                    near_half += 1
                    continue
                assert got == (exact + half).numerator // (exact + half).denominator, (i, j)
                compared += 1
    assert compared >= near_half, (compared, near_half)           # the undecidable pairs are the exception, not the test


def test_the_cases_are_what_their_names_say():
    R = FC.reference
    assert all(len(R(n)["flights"]) == 0 and (R(n)["seg"] == -1).all() and np.isnan(R(n)["fitted"]).all() for n in ("empty", "no_ball_column", "ball_all_nan", "one_present_row"))
    assert not R("no_ball_column")["flags"].any() and R("one_present_row")["flags"].tolist() == [0, 0, 0, 3, 0, 0]
    assert len(R("two_present_rows")["flights"]) == 1 and R("two_present_rows")["seg"].tolist() == [-1, -1, 0, 0, -1, -1]
    assert (R("absent_kinds")["flags"][[4, 9, 10, 15, 16]] == 0).all() and R("absent_kinds")["flags"][20] & 1                 # |x| = 1024 is present
    for n in ("all_equal", "integer_slope", "right_angle", "reversal", "capped_300"):
        assert int(R(n)["totals"]["sum_c"][0]) == 0, n
    assert R("right_angle")["flights"]["row1"].tolist() == [12, 24] and R("reversal")["flights"]["row1"].tolist() == [10, 20]
    assert np.flatnonzero(R("spike_row1_and_last_but_one")["flags"] & 4).tolist() == [1, 14]
    assert np.flatnonzero(R("two_adjacent_displaced")["flags"] & 4).tolist() == [5]                     # equal A at rows 5 .. 8: the earliest
    assert np.flatnonzero(R("equal_A_neighbours")["flags"] & 4).tolist() == [1]
    assert np.flatnonzero(R("spike_next_to_knot")["flags"] & 4).tolist() == [11] and np.flatnonzero(R("spike_next_to_knot")["flags"] & 8).tolist() == [10]
    assert int(R("hole_max_gap_and_one_more")["totals"]["runs"][0]) == 2 and R("hole_max_gap_and_one_more")["flights"]["row0"].tolist() == [0, 11]
    assert R("cut_inside_run")["flights"]["row0"].tolist() == [0, 10] and R("cut_on_run_first_row")["flights"]["row0"].tolist() == [0, 9]
    assert (R("max_rows_2")["flights"]["row1"] - R("max_rows_2")["flights"]["row0"]).max() == 2
    cap = R("capped_300")["flights"]
    assert cap["row0"].tolist() == [0, 43, 171] and (cap["flags"] & 1).tolist() == [0, 1, 1] and int(R("capped_300")["totals"]["knots"][0]) == 2 and len(R("capped_300")["kicks"]) == 0
    assert R("tiles")["runs"] == [(0, 254), (256, 511), (513, 769)]
    assert int(R("cost_above_clamp")["flights"]["c"][0]) == 1 << 40
    assert len(R("penalty_zero")["flights"]) == 43 and len(R("penalty_at_bound")["flights"]) == 1 and FR.lam_of(FC.params_of(FC.BY_NAME["penalty_at_bound"])) == 1 << 40
    k = R("dv_exactly_kick_dv")["kicks"]
    assert len(k) == 1 and float(k["dv"][0]) == 5.0 and float(k["cos_turn"][0]) == 0.0 and len(R("dv_just_below_kick_dv")["kicks"]) == 0
    assert R("kicker_tie")["kicks"]["col"].tolist() == [2] and R("kick_nobody_in_radius")["kicks"]["col"].tolist() == [-1]
    assert R("no_person_columns")["kicks"]["col"].tolist() == [-1] and R("person_cells_absent")["kicks"]["col"].tolist() == [-1]
    f = R("near_exactly_half")["flights"][0]
    assert (int(f["used"]), int(f["near"]), int(f["kind"])) == (10, 5, FR.FREE) and int(R("near_one_more_than_half")["flights"]["kind"][0]) == FR.CARRIED
    assert float(R("speed_exactly_still_speed")["flights"]["speed"][0]) == 0.5 and int(R("speed_exactly_still_speed")["flights"]["kind"][0]) == FR.FREE
    assert int(R("speed_below_still_speed")["flights"]["kind"][0]) == FR.STILL
    s = R("shots")["flights"]
    assert s["shot"].tolist() == [2, 2, 1, 1, 0, 2, 0, 2, 0, 0, 0, 0]
    assert float(s["y_cross"][3]) == 40.0 and abs(float(s["y_cross"][3]) - 34.0) == 3.66 + (6.0 - 3.66)                  # exactly on post + margin
    assert float(s["y_cross"][1]) < 34.0 + 3.66 < float(s["y_cross"][2]) and float(s["y_cross"][2]) - float(s["y_cross"][1]) == 1 / 1024
    assert float(s["speed"][5]) * ((105.0 - float(s["x0"][5])) / float(s["vx"][5])) == 40.0                            # reach == shot_range
    assert np.isnan(s["y_cross"][[8, 11]]).all() and float(s["vx"][8]) == 0.0 and float(s["x0"][9]) == 110.0 and float(s["vx"][7]) < 0.0


def test_refused_parameters():
    good = dict(fps=25.0, max_gap=25)
    FR.params(**good)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(fps=0.0), dict(fps=nan), dict(fps=inf), dict(max_gap=0), dict(max_gap=1025), dict(max_rows=1), dict(max_rows=129), dict(noise=-1.0), dict(noise=nan),
               dict(noise=1025.0), dict(penalty=-1.0), dict(penalty=inf), dict(spike=-0.5), dict(spike=1025.0), dict(kick_dv=-1.0), dict(kick_dv=nan), dict(radius=0.0),
               dict(radius=1025.0), dict(radius=nan), dict(still_speed=-1.0), dict(shot_speed=nan), dict(shot_range=-1.0), dict(shot_margin=inf),
               dict(noise=1.0, penalty=2.0 ** 20 + 1.0)):
        with pytest.raises(ValueError):
            FR.params(**{**good, **kw})
    values, frames, cols = FC.table(np.zeros((4, 2)))
    p = FR.params(**good)
    for bad in (dict(frames=[0, 1, 1, 2]), dict(frames=[0, 2, 1, 3]), dict(cuts=[5, 5]), dict(cuts=[7, 3]), dict(columns=cols + [(FR.BALL, 1, 0)]), dict(columns=[(9, 0, 0)] + cols[1:])):
        kw = dict(frames=frames, columns=cols, cuts=None)
        kw.update(bad)
        v = np.zeros((len(kw["columns"]), 4, 2))
        with pytest.raises(ValueError):
            FR.flights(v, kw["frames"], kw["columns"], p, kw["cuts"])


# ---- the demonstration -------------------------------------------------------------------------------------------------------------------
MEASURED_RMS_FLIGHTS, MEASURED_RMS_CENTRAL = 0.140, 7.82        # m/s on the clip of seed 0, rows within 3 rows of a true change left out (README.md)


def test_demonstration():
    d = FC.demo(FC.DEMO_SEED)
    rows = len(d["frames"])
    assert rows == 500 and d["fps"] == 25.0 and len(d["displaced"]) == 10
    assert all(b - a > 3 for a, b in zip(d["displaced"], d["displaced"][1:]))
    ball = d["values"][0]
    r = FR.flights(d["values"], d["frames"], d["columns"], FR.params(d["fps"], 25))
    knots = np.flatnonzero(r["flags"] & FR.F_KNOT).tolist()
    changes = [c for c, _ in d["changes"]]
    big = [c for c, dv in d["changes"] if dv >= 4.0]
    assert len(big) >= 10
    assert all(any(abs(k - c) <= 2 for k in knots) for c in big)                                      # every large change has a knot within 2 rows
    assert np.flatnonzero(r["flags"] & FR.F_SPIKE).tolist() == d["displaced"]                          # exactly the displaced samples are spikes
    assert all(any(abs(k - c) <= 4 for c in changes) for k in knots)                                  # no stray knot
    keep = np.array([all(abs(i - c) > 3 for c in changes) for i in range(rows)]) & (r["seg"] >= 0)
    keep[0] = keep[-1] = False
    central = np.zeros((rows, 2))
    central[1:-1] = (ball[2:] - ball[:-2]) * d["fps"] / 2.0
    rms = lambda v: float(np.sqrt(np.mean(np.sum((v[keep] - d["truth"][keep]) ** 2, 1))))
    e_fit, e_cd = rms(r["velocity"]), rms(central)
    print(f"flight velocity RMS error {e_fit:.4f} m/s, central difference of the raw column {e_cd:.4f} m/s over {int(keep.sum())} rows; "
          f"{len(big)} large changes, {len(knots)} knots, {len(r['kicks'])} kicks, kinds {r['totals']['kinds'][0].tolist()}")
    assert e_cd / e_fit >= 0.75 * (MEASURED_RMS_CENTRAL / MEASURED_RMS_FLIGHTS)
    assert {int(k) for k in r["flights"]["kind"]} == {FR.STILL, FR.CARRIED, FR.FREE}
