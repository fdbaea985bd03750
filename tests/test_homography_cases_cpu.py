"""Every case of tests/homography_cases.py forces what its name says, proved through the oracle's trace (no GPU): the kernel test (tests/test_gpu_homography.py)
relies on these facts without repeating them.  Also: the trace entry returns what find_homography_ransac returns; the table-size facts about the older
homography tests; and one check of the oracle itself that does not go through its own solvers (an SVD DLT in numpy)."""
import numpy as np
import pytest

import homography_cases as HC

CASES = HC.cases()
HEAT = HC.heat_cases()
_cache = {}


def run(name):
    """(H | None, mask | None, trace) of one case, computed once"""
    if name not in _cache:
        from oracle import prims as P
        if name in HEAT:
            img, world, _ = HC.heat_points(HEAT[name])
            _cache[name] = P.find_homography_ransac_trace(img, world) + (img, world)
        else:
            c = CASES[name]
            _cache[name] = P.find_homography_ransac_trace(c["img"], c["world"], c["thresh"], c["max_iters"], 0.995, c["lm_iters"]) + (c["img"], c["world"])
    return _cache[name]


def trace(name):
    return run(name)[2]


def test_case_tables_agree():
    assert set(HC.TRACE) == set(CASES) | set(HEAT) and not set(CASES) & set(HEAT)
    assert set(HC.NOISY_CAMERA) <= set(CASES)
    for c in CASES.values():
        assert np.isfinite(c["img"]).all() and np.isfinite(c["world"]).all() and 4 <= len(c["img"]) == len(c["world"]) <= HC.MAX_KP


@pytest.mark.parametrize("name", list(CASES) + list(HEAT))
def test_trace_is_the_recorded_one_and_the_plain_entry_returns_the_same(name):
    from oracle import prims as P
    H, mask, t, img, world = run(name)
    got = {k: t[k] for k in HC.TRACE[name]}
    assert got == HC.TRACE[name], name
    c = CASES.get(name, dict(thresh=5.0, max_iters=2000, lm_iters=10))
    H0, m0 = P.find_homography_ransac(img, world, c["thresh"], c["max_iters"], 0.995, c["lm_iters"])
    assert (H is None) == (H0 is None)
    if H is not None:
        assert np.array_equal(H, H0) and np.array_equal(mask, m0) and int(mask.sum()) == t["inliers"]
    else:
        assert t["inliers"] == 0
    # the trace's own arithmetic
    assert t["improvements"] == len(t["imp_attempt"]) <= P.TRACE_IMPROVEMENTS and t["iterations"] <= t["attempts"] <= t["draws"] // 4 + (t["draws"] == 0)
    if t["improvements"]:
        assert t["imp_attempt"][-1] == t["last_imp_attempt"] and t["imp_draw"][-1] == t["last_imp_draw"] and t["imp_good"] == sorted(set(t["imp_good"]))


def test_python_stream_is_the_oracles():
    """rounds_of() partitions the stream that cv::RNG(-1) really gives"""
    import ctypes as C
    from oracle import prims as P
    out = np.empty(5000, np.uint32)
    P.lib().eo_rng_stream(out.ctypes.data_as(C.POINTER(C.c_uint32)), 5000)
    assert np.array_equal(out, HC.rng_stream(5000))
    for name in ("n5_attempt_of_11_draws", "bound_257_every_attempt_counts", "improvement_on_round_start"):      # ... and its attempts end where the oracle's do
        t = trace(name)
        assert HC.attempt_starts(len(run(name)[3]), t["attempts"])[-1] == t["draws"], name


# ---- sampler ------------------------------------------------------------------------------------------------------------
def test_sampler_cases():
    for name, n in (("n5_attempt_of_11_draws", 5), ("n5_no_valid_subset", 5), ("n6_attempt_of_13_draws", 6), ("n7_attempt_of_13_draws", 7), ("n87_garbage", 87)):
        assert len(CASES[name]["img"]) == n
    for name in ("n5_attempt_of_11_draws", "n5_no_valid_subset", "n6_attempt_of_13_draws", "n7_attempt_of_13_draws"):
        assert trace(name)["max_attempt_draws"] > 8, name                       # the eight-draw parse cannot finish it
    assert trace("n5_attempt_of_11_draws")["inliers"] == 4                      # (the 4-point inlier set of the DLT / LM list)
    assert trace("n5_no_valid_subset")["end"] == HC.END_REJECT_ITER0 and run("n5_no_valid_subset")[0] is None


# ---- (A) ----------------------------------------------------------------------------------------------------------------
def test_first_model_wins_and_ties_do_not_replace_it():
    t = trace("first_model_wins_later_ties")
    assert t["improvements"] == 1 and t["imp_iter"] == [1] and t["iterations"] > 1 and t["ties"] >= 1
    assert t["imp_good"] == [t["inliers"]] and t["inliers"] < len(CASES["first_model_wins_later_ties"]["img"])


@pytest.mark.parametrize("name,ordinal", [("improvement_on_lane_63", 63), ("improvement_on_lane_64", 64), ("improvement_on_attempt_255", 255),
                                          ("improvement_on_round_start", 256)])
def test_improvement_falls_on_a_boundary(name, ordinal):
    t = trace(name)
    ro = HC.rounds_of(len(CASES[name]["img"]), t["imp_attempt"][-1] + 1)
    hits = []
    for a in t["imp_attempt"]:
        r, o = ro[a]
        if ordinal == 256:
            hits.append(r > 0 and o == 0 and ro[a - 1][1] == HC.ROUND_ATTEMPTS - 1)      # the first attempt after a FULL round
        else:
            hits.append(o == ordinal)
    assert any(hits), (t["imp_attempt"], [tuple(ro[a]) for a in t["imp_attempt"]])
    assert t["improvements"] >= 3


def test_many_improvements():
    assert trace("improvement_on_round_start")["improvements"] == 7 and trace("improvement_on_lane_63")["improvements"] == 5


# ---- (B) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", HC.BOUNDS)
def test_bound_is_reached_at_that_iteration(m):
    for kind in ("every_attempt_counts", "garbage"):
        t = trace(f"bound_{m}_{kind}")
        assert t["end"] == HC.END_BOUND and t["iterations"] == m == t["final_niters"], kind      # no consensus: no improvement lowers the bound
    t = trace(f"bound_{m}_every_attempt_counts")
    if m <= 257:
        assert t["attempts"] == m and t["longest_reject_run"] == 0                                # iteration m IS attempt m - 1 ...
        r, o = HC.rounds_of(30, m)[m - 1]
        assert (r, o) == ((0, m - 1) if m <= 256 else (1, 0))                                     # ... lanes 62, 63, 0 of a replay step; 254, 255 and the next round's first
    assert trace(f"bound_{m}_garbage")["attempts"] > m                                            # rejected subsets in between: the bound falls inside a step


def test_adaptive_bound_already_passed():
    t = trace("adaptive_bound_below_count")
    assert t["end"] == HC.END_BOUND and 0 < t["imp_niters"][-1] < t["imp_iter"][-1] == t["iterations"] and t["final_niters"] == t["imp_niters"][-1]


# ---- (C) ----------------------------------------------------------------------------------------------------------------
def test_rule_c_cases():
    assert trace("reject_1000_at_iteration_0")["end"] == HC.END_REJECT_ITER0 and run("reject_1000_at_iteration_0")[0] is None
    for name, lo, hi in (("reject_1000_after_1_iteration", 1, 1), ("reject_1000_after_10_iterations", 8, 12), ("reject_1000_after_106_iterations", 100, 2000),
                         ("past_table_269270_draws", 100, 2000), ("heat_reject_1000_after_50_iterations", 2, 2000)):
        t = trace(name)
        assert t["end"] == HC.END_REJECT_LATER and lo <= t["iterations"] <= hi and t["longest_reject_run"] == 1000 and run(name)[0] is not None, name
        assert t["longest_run_attempt"] + 1000 == t["attempts"]                                   # the run that ends the loop


def test_rejected_run_spans_rounds_and_starts_inside_one():
    name = "reject_1000_after_10_iterations"
    t = trace(name)
    ro = HC.rounds_of(len(CASES[name]["img"]), t["attempts"])
    first, last = ro[t["longest_run_attempt"]], ro[t["attempts"] - 1]
    assert first[1] != 0 and last[0] - first[0] >= 3, (first, last)                               # carried over at least three round boundaries


# ---- thresholds ---------------------------------------------------------------------------------------------------------
def test_threshold_cases():
    t = trace("thresh_1e6_first_model_takes_all")
    assert t["end"] == HC.END_NITERS_ZERO and t["iterations"] == 1 and t["final_niters"] == 0 and t["inliers"] == len(CASES["thresh_1e6_first_model_takes_all"]["img"])
    t = trace("thresh_1e-13_models_lose_own_points")
    assert t["min_model_support"] < 4 and t["inliers"] == 4 and np.float32(1e-13 * 1e-13) > 0
    t = trace("thresh_1e-15_no_model_keeps_4")
    assert t["improvements"] == 0 and t["iterations"] == 2000 and run("thresh_1e-15_no_model_keeps_4")[0] is None and np.float32(1e-15 * 1e-15) > 0
    assert trace("thresh_0.5")["inliers"] < trace("thresh_20")["inliers"]


# ---- n == 4 -------------------------------------------------------------------------------------------------------------
def test_n4_cases():
    for name, ok in (("n4_general_position", True), ("n4_three_collinear", True), ("n4_equal_x_no_normalisation", False)):
        assert len(CASES[name]["img"]) == 4 and trace(name)["end"] == HC.END_NO_LOOP and trace(name)["draws"] == 0 and (run(name)[0] is not None) == ok, name
    p = CASES["n4_three_collinear"]["img"].astype(np.float64)
    assert np.linalg.det(np.c_[p[:3], np.ones(3)]) == 0.0
    assert np.ptp(CASES["n4_equal_x_no_normalisation"]["img"][:, 0]) == 0.0


# ---- DLT and LM ---------------------------------------------------------------------------------------------------------
def test_dlt_and_lm_cases():
    acc = {lm: trace(f"lm_iters_{lm}")["lm_accepted"] for lm in (0, 1, 10, 30)}
    assert acc[0] == 0 and acc[1] == 1 and acc[10] == 10 and acc[30] > 10, acc                    # 30 goes on where 10 stops
    for n in (5, 8, 9, 40, 87):
        assert trace(f"inliers_{n}")["inliers"] == n == len(CASES[f"inliers_{n}"]["img"])
    assert CASES["scale_3840x2160"]["img"].max(0)[0] > 3000 and CASES["scale_3840x2160"]["img"].max(0)[1] > 1500
    assert (CASES["scale_320x180"]["img"].max(0) < (320, 180)).all()
    for name in ("near_affine_camera", "steep_camera"):
        H = run(name)[0]
        assert H is not None and trace(name)["inliers"] >= 30
    Ha, Hs = run("near_affine_camera")[0], run("steep_camera")[0]
    assert np.abs(Ha[2, :2]).max() * 1280 < 1e-3                                                  # image -> pitch: the weight changes by < 0.1 % over the image
    w = np.c_[CASES["steep_camera"]["img"].astype(np.float64), np.ones(40)] @ Hs[2]
    assert w.min() > 0 and w.max() / w.min() > 10                                                 # by more than 10 x, and the horizon (w = 0) is not crossed


# ---- the end of the draw table ------------------------------------------------------------------------------------------
def test_stream_end_cases():
    under = [n for n in CASES if n.startswith("under_table")]
    before = [n for n in CASES if n.startswith("past_table_best_before")]
    after = [n for n in CASES if n.startswith("past_table_best_after")]
    assert len(under) == 3 and len(before) == 3 and len(after) >= 3
    for n in under:
        assert 60000 < trace(n)["draws"] < HC.TABLE, n
    for n in before:
        assert trace(n)["draws"] > HC.TABLE > trace(n)["last_imp_draw"] > 0, n
    for n in after + ["heat_past_table_best_after"]:
        assert trace(n)["draws"] >= trace(n)["last_imp_draw"] > HC.TABLE, n                       # best_draw > 65536: a solver that stops at the table returns another model
    assert trace("past_table_269270_draws")["draws"] > 250000 and trace("past_table_269270_draws")["last_imp_draw"] > HC.TABLE
    assert trace("reject_1000_after_106_iterations")["draws"] > HC.TABLE


def test_older_garbage_tests_stay_under_the_table():
    """tests/test_gpu_ops.py::test_find_homography_garbage_points_full_2000_iterations never reached the table's end"""
    from oracle import prims as P
    draws = []
    for seed, n in [(0, 5), (1, 9), (2, 30), (3, 57), (4, 87)]:
        rng = np.random.default_rng(100 + seed)
        img = np.floor(rng.uniform(0, 1280, (n, 2))).astype(np.float32)
        world = rng.uniform(0, 105, (n, 2)).astype(np.float32)
        draws.append(P.find_homography_ransac_trace(img, world, 5.0)[2]["draws"])
    assert draws == [6387, 2521, 47693, 46409, 42020] and max(draws) < HC.TABLE


def test_heat_cases():
    assert trace("heat_camera")["end"] == HC.END_NITERS_ZERO and trace("heat_camera")["improvements"] >= 2
    for name in HEAT:
        assert 5 <= len(run(name)[3]) <= HC.MAX_KP


def test_no_failed_solve_is_reached():
    assert all(trace(n)["solve_failures"] == 0 for n in HC.TRACE)              # (homography_cases.py: searched for, not found)


# ---- the oracle against an independent DLT ------------------------------------------------------------------------------
def _cost(H, src, dst):
    p = np.c_[src, np.ones(len(src))] @ H.T
    return float((((p[:, :2] / p[:, 2:3]) - dst) ** 2).sum())


def _svd_dlt(src, dst):
    """cv2's normalised DLT (centroid, mean absolute deviation per axis) with the null vector from numpy.linalg.svd"""
    n = len(src)
    cs, cd = src.mean(0), dst.mean(0)
    ss, sd = n / np.abs(src - cs).sum(0), n / np.abs(dst - cd).sum(0)
    S, D = (src - cs) * ss, (dst - cd) * sd
    A = np.zeros((2 * n, 9))
    A[0::2, 0:2] = S; A[0::2, 2] = 1; A[0::2, 6:8] = -D[:, :1] * S; A[0::2, 8] = -D[:, 0]
    A[1::2, 3:5] = S; A[1::2, 5] = 1; A[1::2, 6:8] = -D[:, 1:] * S; A[1::2, 8] = -D[:, 1]
    h = np.linalg.svd(A)[2][-1].reshape(3, 3)
    Ts = np.array([[ss[0], 0, -cs[0] * ss[0]], [0, ss[1], -cs[1] * ss[1]], [0, 0, 1]])
    iTd = np.array([[1 / sd[0], 0, cd[0]], [0, 1 / sd[1], cd[1]], [0, 0, 1]])
    H = iTd @ h @ Ts
    return H / H[2, 2]


# largest cost(returned H) / cost(SVD DLT on the returned inliers) over NOISY_CAMERA, measured on the CPU: LM only accepts decreases from its DLT start, so
# no ratio may exceed 1; the margin of 1e-9 (relative) covers the Jacobi and the SVD null vectors differing in their last digits
MEASURED_WORST_RATIO = 0.999186473408675          # near_affine_camera; the others: 0.247 (steep_camera) to 0.99898 (scale_320x180)


def test_oracle_does_not_lose_to_a_plain_svd_dlt():
    ratios = {}
    for name in HC.NOISY_CAMERA:
        H, mask, t, img, world = run(name)
        sel = mask.astype(bool)
        src, dst = img[sel].astype(np.float64), world[sel].astype(np.float64)
        ratios[name] = _cost(H, src, dst) / _cost(_svd_dlt(src, dst), src, dst)
    print({k: f"{v:.15f}" for k, v in ratios.items()})
    assert max(ratios.values()) <= MEASURED_WORST_RATIO * (1 + 1e-9), ratios
