"""Line registration without a GPU (K39): the two forms of tests/linefit_ref.py agree on every constructed case and on seeded random small frames; each
case of tests/linefit_cases.py forces what it is named after; the overflow bound fires one step beyond the admitted size; the header, the bindings and
the CLI's argument checks are in place; and THE DEMONSTRATION: on four synthetic 720p frames whose true homography is disturbed, the contract brings the
mean foot-point error of the 25 people from about 2.1 m to about 0.1 m.

Measured with the contract (mean distance in metres between the foot points projected with the true matrix inv(synth.camera) and with the matrix under
test; boxes from synth.player_boxes hide the players; default parameters):

    frame (seed, t)   disturbance C          0.7 m shift            true matrix
    (3, 0)            2.2271 -> 0.1014       0.7071 -> 0.1014       0 -> 0.1014
    (3, 200)          2.1813 -> 0.0656       0.7071 -> 0.0655       0 -> 0.0655
    (7, 90)           2.2146, kept (SHIFT)   0.7071 -> 0.0569       0 -> 0.0569
    (11, 400)         1.9894 -> 0.1171       0.7071 -> 0.1171       0 -> 0.1171

C moves a point of frame (7, 90)'s view by 3.43 m, beyond the default max_shift of 3 m, so that frame keeps its matrix: the stated protection at work; with
max_shift = 4 it reaches 0.0569 m.  What stays is of the size of synth.frame's integer truncation of the line positions, which is also why the true
matrix is moved by that much.  The tests assert three quarters of each measured ratio: the computation is deterministic, so that leaves room for nothing
but a change of the rule."""
import functools
import os
import re

import numpy as np
import pytest

import linefit_cases as LC
import linefit_ref as R
from eagle_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {c["name"]: c for c in LC.all_cases()}


def _equal(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name", list(CASES))
def test_the_two_forms_agree_and_the_case_forces_its_name(name):
    c = CASES[name]
    vec = R.linefit(c["frames"], c["Hs"], c["valid"], c["boxes"], c["p"])
    c["expect"](*vec)
    assert _equal(vec, R.linefit(c["frames"], c["Hs"], c["valid"], c["boxes"], c["p"], scalar=True))


def test_the_cases_cover_every_status_model_and_cause():
    st, md, fall = set(), set(), 0
    for c in CASES.values():
        _, rec, _ = R.linefit(c["frames"], c["Hs"], c["valid"], c["boxes"], c["p"])
        st |= {int(t) for t in rec["status"]}
        md |= {int(t) for t in rec["model"]}
        fall |= int(np.bitwise_or.reduce(rec["fall"])) if len(rec) else 0
    assert st == set(range(6)) and md == {0, 1, 2, 3}
    assert fall & 0b001001001 == 0b001001001 and fall & 0b100100100 == 0b100100100            # LINES and CAP at every rung


def test_a_failed_pivot_falls_to_the_next_rung():
    # sums of rank 1 (every row a multiple of one J) under facts that admit the affine rung: its pivot test and the translation's fail, nothing moves
    S = [0] * R.NSUM
    J = [512 * 128, 128 * 7, 128 * 9, 0, 0, 0, 0, 0]
    s = 0
    for i in range(8):
        for j in range(i, 8):
            S[s] = 50 * J[i] * J[j]
            s += 1
    for i in range(8):
        S[36 + i] = 50 * J[i] * 40
    S[44], S[45] = 50, 50 * 1600
    S[46 + 2], S[46 + 3], S[46 + 4], S[46 + 0] = 20, 20, 10, 20                                 # three vertical lines and a horizontal one
    M = [0.05, 0.0, 10.0, 0.0, 0.05, 10.0, 0.0, 0.0, 1.0]
    new, rung, fall = R.step(S, M, R.params(min_per_line=5))
    assert fall == (1 << (6 + R.LINES)) | (1 << (3 + R.PIVOT)) | (1 << R.PIVOT) and rung == 0 and new == M
    assert R.solve(S, [0, 3]) is None and R.solve(S, [0]) == [-40 / 65536]
    # the constructed case reaches the same branch through pixels: three dots on three lines cannot carry six unknowns
    _, rec, _ = R.linefit(*(CASES["pivot_three_dots"][k] for k in ("frames", "Hs", "valid", "boxes", "p")))
    assert int(rec["fall"][0]) & (1 << (3 + R.PIVOT)) and int(rec["model"][0]) == 1


def test_random_small_frames_agree_in_both_forms():
    rng = np.random.Generator(np.random.PCG64(39))
    seen = set()
    for trial in range(300):
        h, w = int(rng.integers(5, 16)), int(rng.integers(5, 40))
        f = LC.grass(h, w)
        f[rng.random((h, w)) < 0.15] = LC.WHITE
        f[rng.random((h, w)) < 0.05] = LC.STANDS
        f[rng.random((h, w)) < 0.05] = rng.integers(0, 256, 3)
        step = int(rng.choice([16, 64, 256, 1024]))
        X0, Y0 = rng.choice([(16896, 14172), (53760, 34816), (0, 0), (107520 - w * step, 69632 - h * step), (11264 + 6000, 34816 - 8000)])
        H = LC.qmap(int(X0) - step * w // 2, int(Y0) - step * h // 2, step)
        H[6:8] = rng.normal(0, 2e-3, 2) * (trial % 3 == 0)
        H *= rng.choice([1.0, -1.0, 3.0])
        p = R.params(k=int(rng.integers(1, 4)), tau=int(rng.choice([200, 600])), rounds=int(rng.integers(0, 4)), model=int(rng.integers(1, 4)),
                     min_points=int(rng.integers(1, 6)), min_per_line=int(rng.integers(1, 4)), radius=float(rng.choice([8.0, 2.5, 0.5])), radius_min=0.5,
                     max_shift=float(rng.choice([0.05, 3.0, 100.0])), box_pad=float(rng.choice([0.0, 1.5])))
        boxes = None if trial % 2 else [rng.uniform(0, max(h, w), (int(rng.integers(0, 3)), 4)).astype(np.float32)]
        valid = [int(trial % 17 != 0)]
        vec = R.linefit(f[None], H, valid, boxes, p)
        assert _equal(vec, R.linefit(f[None], H, valid, boxes, p, scalar=True)), trial
        seen.add((int(vec[1]["status"][0]), int(vec[1]["model"][0])))
    assert {s for s, _ in seen} >= {R.NO_MAP, R.ACCEPTED, R.UNCHANGED} and {m for _, m in seen} >= {0, 1}, seen


def test_the_overflow_bound_fires_one_step_beyond_the_admitted_size():
    R.check_size(16384, 16384)
    R.check_size(1, 1)
    for h, w in ((16385, 16384), (16384, 16385), (0, 5)):
        with pytest.raises(AssertionError):
            R.check_size(h, w)
    top = (1 << 63) // (R.ROW_MAX * R.ROW_MAX)
    assert R.overflow_bound(top - 1) and R.MAX_PIXELS <= top - 1
    with pytest.raises(AssertionError):
        R.overflow_bound(top)
    # one cell at its largest: a row of ROW_MAX - 1 in every place, summed over the largest frame, stays inside a signed 64-bit word
    assert R.MAX_PIXELS * (R.ROW_MAX - 1) ** 2 < 1 << 63 and R.MAX_PIXELS * (R.ROW_MAX - 1) * R.E_MAX < 1 << 63
    with pytest.raises(AssertionError):
        R.params(radius=8.5)                                                                     # |e| <= E_MAX rests on radius <= 8 m


def test_the_longest_rows_stay_below_row_max():
    # the far corner flag at the largest radius, and the arcs' steepest gradients
    worst = 0
    for qx, qy in ((107520 + 8192, 69632 + 8192), (-8192, -8192), (107520 + 8192, -8192)):
        prim, e = R.match_scalar(qx, min(max(qy, 0), 69632))
        worst = max(worst, max(abs(t) for t in R.row_scalar(qx, min(max(qy, 0), 69632), prim)))
    for j, (cx, cy, Rr, side, lim) in enumerate(R.ARCS):
        d = int(np.sqrt(Rr * Rr + 2 * Rr * 8192))                                               # e = rq at the largest radius
        worst = max(worst, max(abs(t) for t in R.row_scalar(cx + (d if side >= 0 else -d), cy, R.NSEG + j)))
        k = int(d / np.sqrt(2))
        worst = max(worst, max(abs(t) for t in R.row_scalar(cx + (k if side >= 0 else -k), cy + k, R.NSEG + j)))
    assert 1 << 16 < worst < R.ROW_MAX, worst


# ---- the demonstration -----------------------------------------------------------------------------------------------------------------
VIEWS = ((3, 0), (3, 200), (7, 90), (11, 400))
DISTURB = {"C": np.array([[1.012, .006, .9], [-.004, .99, -.6], [1e-4, -2e-4, 1]]), "0.7": np.array([[1, 0, .5], [0, 1, -.5], [0, 0, 1.0]]), "true": np.eye(3)}
MEASURED = {((3, 0), "C"): (2.2271, 0.1014), ((3, 0), "0.7"): (0.7071, 0.1014), ((3, 0), "true"): (0.0, 0.1014),
            ((3, 200), "C"): (2.1813, 0.0656), ((3, 200), "0.7"): (0.7071, 0.0655), ((3, 200), "true"): (0.0, 0.0655),
            ((7, 90), "C"): (2.2146, 2.2146), ((7, 90), "0.7"): (0.7071, 0.0569), ((7, 90), "true"): (0.0, 0.0569),
            ((11, 400), "C"): (1.9894, 0.1171), ((11, 400), "0.7"): (0.7071, 0.1171), ((11, 400), "true"): (0.0, 0.1171)}


@functools.lru_cache(None)
def _view(seed, t):
    boxes = np.array([b[1:] for b in synth.player_boxes(seed, t)], np.float32)
    feet = np.array([[(b[0] + b[2]) / 2, b[3]] for b in boxes], np.float64)
    truth = np.linalg.inv(synth.camera(seed, t))
    return R.line_mask(synth.frame(seed, t), boxes, R.params()), feet, truth


def _error(H, feet, truth):
    return float(np.linalg.norm(synth.project(truth, feet) - synth.project(np.asarray(H).reshape(3, 3), feet), axis=1).mean())


@pytest.mark.parametrize("view", VIEWS)
def test_demonstration_on_the_synthetic_frames(view):
    mask, feet, truth = _view(*view)
    assert 8000 < mask.sum() < 20000
    for name, D in DISTURB.items():
        H = (D @ truth).reshape(9)
        out, rec = R.refine_frame(mask, H, 1, R.params())
        before, after = _error(H, feet, truth), _error(out, feet, truth)
        print(view, name, "%.4f -> %.4f" % (before, after), rec)
        mb, ma = MEASURED[(view, name)]
        assert abs(before - mb) < 1e-3
        if (view, name) == ((7, 90), "C"):                                                       # C moves this view by 3.43 m: beyond max_shift, kept bit for bit
            assert int(rec["status"]) == R.SHIFT and out.tobytes() == H.tobytes() and 3.0 < np.sqrt(int(rec["shift2"])) / 1024 < 3.5
            out, rec = R.refine_frame(mask, H, 1, R.params(max_shift=4.0))
            assert int(rec["status"]) == R.ACCEPTED and before / _error(out, feet, truth) >= 0.75 * (2.2146 / 0.0569)
        elif name == "true":                                                                     # a good matrix is not damaged beyond the lines' own truncation
            assert int(rec["status"]) in (R.ACCEPTED, R.UNCHANGED, R.NO_GAIN) and after <= ma + 5e-4
        else:
            assert int(rec["status"]) == R.ACCEPTED and int(rec["model"]) == 3 and before / after >= 0.75 * (mb / ma)
            assert R.metres(int(rec["e2_after"]), int(rec["n_after"])) < 0.2 and int(rec["n_after"]) > 5 * int(rec["n_before"]) * (name == "C")


# ---- the layers a GPU is not needed for -------------------------------------------------------------------------------------------------
def test_abi_declarations_and_bindings():
    import ctypes as C
    from eagle_amd import lib
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name in ("eagle_linefit_params_default", "eagle_linefit_device_frames", "eagle_linefit_frames", "eagle_op_linefit"):
        assert re.search(r"^int %s\(" % name, head, re.M) and name in lib.EXPORTS, name
    assert C.sizeof(lib.EagleLineFitParams) == 88 and lib.LINEFIT_FRAME_DTYPE == R.FRAME_DTYPE
    for i, name in enumerate(("NO_MAP", "ACCEPTED", "UNCHANGED", "FEW_POINTS", "NO_GAIN", "SHIFT")):
        assert re.search(r"#define EAGLE_LINEFIT_%s %d\b" % (name, i), head) and getattr(R, name) == getattr(lib, "LINEFIT_" + name) == i
    for i, name in enumerate(("LINES", "PIVOT", "CAP")):
        assert re.search(r"#define EAGLE_LINEFIT_FALL_%s %d\b" % (name, i), head) and getattr(R, name) == i
    L = lib.load()
    p = lib.linefit_params()
    assert {k: getattr(p, k) for k in R.DEFAULTS} == R.DEFAULTS and not any(p.reserved)
    assert L.eagle_linefit_params_default(None) == lib.E_INVALID
    with pytest.raises(lib.EagleError, match="unknown parameter"):
        lib.linefit_params(radii=3)
    src = open(os.path.join(ROOT, "eagle_amd", "csrc", "linefit_accumulate.inc")).read()
    nums = lambda t: [int(v) for v in re.findall(r"-?\d+", t)]
    assert nums(re.search(r"c_seg\[LF_NSEG\] = (.*?);", src, re.S).group(1)) == [v for sg in R.SEGMENTS for v in sg]
    assert nums(re.search(r"c_arc\[LF_NARC\] = (.*?);", src, re.S).group(1)) == [v for cx, cy, _, side, lim in R.ARCS for v in (cx, cy, side, lim)]
    assert "LF_CX = %d, LF_CY = %d, LF_R = %d" % (R.CX, R.CY, R.ARCS[0][2]) in src


def test_report_json_from_the_contracts_records():
    import json
    from eagle_amd import lib, linefit
    c = CASES["sixty_five_frames"]
    out, rec, _ = R.linefit(c["frames"], c["Hs"], c["valid"], c["boxes"], c["p"])
    res = linefit.Result(out, rec.astype(lib.LINEFIT_FRAME_DTYPE), None, linefit.params_dict(lib.linefit_params(**c["p"])))
    d = linefit.to_json(res, rows=True)
    json.dumps(d)
    acc = rec["status"] == R.ACCEPTED
    assert d["totals"]["frames"] == 65 and d["totals"]["status"]["accepted"] == int(acc.sum()) and sum(d["totals"]["status"].values()) == 65
    assert sum(d["totals"]["model"].values()) == 65 - d["totals"]["status"]["no_map"]
    assert abs(d["totals"]["rms_after"] - np.sqrt(int(rec["e2_after"][acc].sum()) / int(rec["n_after"][acc].sum())) / 1024) < 1e-12
    assert d["totals"]["rms_after"] < d["totals"]["rms_before"] and d["totals"]["largest_shift"] == max(r["shift"] for r in d["rows"] if r["status"] == "accepted")
    assert "rows" not in linefit.to_json(res) and all(r["frame"] == i for i, r in enumerate(d["rows"]))
    assert d["params"]["model"] == "projective" and linefit.default_params(model="affine").model == 2
    with pytest.raises(ValueError):
        linefit.default_params(model="rigid")


def test_cli_refuses_sub_options_without_the_stage():
    from eagle_amd import cli
    for bad in (["--refine-lines-rows"], ["--refine-lines-model", "affine"], ["--refine-lines-contrast", "100"], ["--refine-lines", "--refine-lines-radius", "9"],
                ["--refine-lines", "--refine-lines-rounds", "17"], ["--refine-lines", "--refine-lines-min-radius", "3"]):
        with pytest.raises(SystemExit):
            cli.main(["--synthetic-weights", "--frames", "1", "--out", os.devnull] + bad)


def test_documents_state_the_rule_and_its_limits():
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    exps = open(os.path.join(ROOT, "docs", "experiments.md")).read()
    assert "**Line registration (K39).**" in readme and "not fitted to data" in readme and "lens distortion" in readme and "2.2271" in readme
    assert "f25" in design and "linefit_accumulate_kernel" in design and "Line registration (K39)" in exps
