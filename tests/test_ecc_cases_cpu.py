"""The constructed ECC cases (tests/ecc_cases.py) force what they are named after, shown with the references alone (no GPU): tests/ecc_ref.py (the
kernel's arithmetic and summation order, restated from csrc/ecc.hip) against oracle/ecc.py (numpy's sums, whole-image gradients) bit for bit, and
ecc_ref's trace for the exits, the rotation path, the negative fixed-point coordinates and the margins that make a comparison of bits with a
device legitimate.  Every assertion here is a condition on the case list."""
import os
import re

import numpy as np
import pytest

import ecc_cases
import ecc_ref
from ecc_cases import CASES, EXPECT, NAMES, expected
from oracle import ecc
from oracle import prims as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = np.array(ecc_ref.IDENT, np.float32)


def _iterations(name):
    return [t for t in expected(name)[4] if "M_in" in t]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def test_case_list_covers_the_sizes_motions_and_exits():
    assert {ecc_cases.size_of(n) for n in NAMES} == set(ecc_cases.SIZES)
    assert sum(ecc_cases.size_of(n) == (108, 192) for n in NAMES) <= 3
    for h, w in ecc_cases.SIZES[:4]:
        assert f"ident_{h}x{w}" in NAMES
    for h, w in ecc_cases.SIZES[1:4]:                        # (at 4 x 4 every moved pair fails: those are the failures deep in the loop)
        for kind in ("shift_a", "shift_b", "rot3", "rotm6"):
            assert f"{kind}_{h}x{w}" in NAMES and EXPECT[f"{kind}_{h}x{w}"][0] == 1
    assert any(ecc_cases.size_of(n) == (24, 37) for n in ecc_cases.CYCLES) and any(ecc_cases.size_of(n) == (108, 192) for n in ecc_cases.CYCLES)
    assert len(ecc_cases.QUICK) >= 5
    exits = {EXPECT[n][:2] for n in NAMES}
    assert exits == {(1, "eps"), (1, "count"), (0, "empty mask"), (0, "nan"), (0, "lambda")}
    for kind in ("empty mask", "nan", "lambda"):             # each failure also after more than one iteration
        assert any(EXPECT[n][1] == kind and EXPECT[n][2] > 1 for n in NAMES), kind
    assert sum(EXPECT[n][0] == 0 and EXPECT[n][2] > 1 and ecc_cases.size_of(n) == (4, 4) for n in NAMES) >= 4
    for n in NAMES:
        t, i, max_iter, eps = CASES[n]
        assert t.dtype == i.dtype == np.uint8 and t.shape == i.shape and t.flags.c_contiguous and i.flags.c_contiguous and 0 <= max_iter <= 100


@pytest.mark.parametrize("name", NAMES)
def test_case_takes_its_exit_and_the_reference_equals_the_oracle(name):
    t, i, max_iter, eps = CASES[name]
    ok, iters, rho, M, trace = expected(name)
    assert (ok, trace[-1]["exit"], iters) == EXPECT[name]
    otrace = []
    o = ecc.find_transform_ecc(t, i, max_iter, eps, trace=otrace)
    if o is None:
        assert ok == 0 and iters == len(otrace) + 1          # the oracle fails in the same iteration
    else:
        assert ok == 1 and iters == o[2]
        assert np.array_equal(_bits(M), _bits(o[1])), (M, o[1])
        assert abs(rho - o[0]) <= 1e-12
    done = [r for r in _iterations(name) if "M" in r]
    assert len(done) == len(otrace)
    for k, (r, (orho, oM)) in enumerate(zip(done, otrace)):  # ... and every iteration on the way
        assert np.array_equal(_bits(r["M"]), _bits(oM)), k
        assert abs(r["rho"] - orho) <= 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_no_float32_of_the_warp_depends_on_the_last_bits_of_asin_sin_or_cos(name):
    """asin's result, theta, and cos's and sin's results moved by up to 4 float64 ulps, in every iteration: the float32 values stored into M stay.
    This is the only place where the device's maths library and numpy's need not agree; a case that fails here gets another seed."""
    its = [r for r in _iterations(name) if "M" in r]
    assert all(r["libm_ok"] for r in its), [k for k, r in enumerate(its) if not r["libm_ok"]]


def test_exit_cases():
    ok, iters, rho, M, _ = expected("zero_iterations_24x37")
    assert (ok, iters, rho) == (1, 0, -1.0) and np.array_equal(_bits(M), _bits(IDENT))
    assert expected("count7_24x37")[1] == 7 and CASES["count7_24x37"][2:] == (7, 0.0)
    assert expected("rot3_24x37")[1] > 7                     # the same pair goes on where the count lets it
    for n in ecc_cases.STRIPES:
        ok, iters, rho, M, _ = expected(n)
        its = _iterations(n)
        assert (ok, iters) == (1, 2) and all(r["det"] == 0.0 for r in its)          # gy = 0 everywhere: the Hessian is singular, exactly
        assert np.array_equal(M, IDENT) and np.array_equal(_bits(M), _bits([1, -0.0, 0, 0, 1, 0]))      # (M[1] = -M[3] = -0.0)
    assert abs(expected("stripes_same_24x37")[2] - 1.0) < 1e-12 and 0 <expected("stripes_moved_16x32")[2] < 0.99
    for n in NAMES:
        if EXPECT[n][0] == 0 and EXPECT[n][2] == 1:
            assert np.array_equal(_bits(expected(n)[3]), _bits(IDENT))
    for n in ecc_cases.CYCLES:                               # the 1/32-pixel quantisation: rho keeps moving to the end, inside a small band
        r = [x["rho"] for x in _iterations(n)]
        assert len(r) == 100 and all(abs(a - b) >= 1e-5 for a, b in zip(r[1:], r[:-1])) and max(r[50:]) - min(r[50:]) < 2e-2


def test_rotation_cases_use_the_rotation_path():
    assert len(ecc_cases.ROTATIONS) >= 8
    for n, deg in ecc_cases.ROTATIONS.items():
        m3 = [float(r["M"][3]) for r in _iterations(n)]
        first = next(k for k in range(len(m3)) if all(abs(v) > 0.03 for v in m3[k:]))
        assert first < len(m3) - 2, n                        # |M[3]| > 0.03 from some iteration on, with iterations to follow
        assert np.sign(m3[-1]) == np.sign(deg) and abs(m3[-1] - np.sin(np.deg2rad(deg))) < 0.012, (n, m3[-1])
        # a kernel with h0 and h1 swapped in hat_x / hat_y would end elsewhere, or fail
        t, i, max_iter, eps = CASES[n]
        bad = ecc_ref.align(t, i, max_iter, eps, swap_h=True)
        assert bad[:2] != expected(n)[:2] or not np.array_equal(_bits(bad[3]), _bits(expected(n)[3])), n


def test_shifted_cases_reach_negative_coordinates_and_partly_covered_pixels():
    assert len(ecc_cases.SHIFTED) >= 8
    for n in ecc_cases.SHIFTED:
        its = _iterations(n)
        neg, part = sum(r["negative_coords"] for r in its), sum(r["outside_nonzero"] for r in its)
        print(f"{n}: {neg} negative fixed-point coordinates, {part} pixels outside the mask with a non-zero warped value")
        assert neg > 0 and part > 0
        t, i, max_iter, eps = CASES[n]
        bad = ecc_ref.align(t, i, max_iter, eps, round_16=0)                # without the + 16 rounding of the 1/32-pixel coordinates
        assert bad[:2] != expected(n)[:2] or not np.array_equal(_bits(bad[3]), _bits(expected(n)[3])), n
    # both signs of the translation, and coordinates beyond the kernel's -4 .. size + 4 clamp
    assert expected("shift_a_24x37")[3][2] < -1 and expected("shift_b_24x37")[3][2] > 1
    assert sum(r["clamped"] for n in NAMES for r in _iterations(n)) > 0
    assert sum(r["clamped"] for r in _iterations("rot3_108x192")) > 0


def test_reduction_order_is_pinned_where_it_can_be():
    """The waves added 7..0 instead of 0..7: no warp and no iteration count of any case changes, and rho changes in its last bits at 108 x 192 only
    where it changes at all.  The figures are printed; what is asserted is that the order cannot be seen in M or iters (so that the GPU test's
    equality of M does not hang on it) and whether rho shows it."""
    seen = []
    for n in NAMES:
        t, i, max_iter, eps = CASES[n]
        ok, iters, rho, M, _ = expected(n)
        b = ecc_ref.align(t, i, max_iter, eps, waves_backwards=True)
        assert (b[0], b[1]) == (ok, iters) and np.array_equal(_bits(b[3]), _bits(M)), n
        if ok and b[2] != rho:
            seen.append(n)
            assert abs(b[2] - rho) < 1e-15
    print("rho shows the order of the waves in:", seen)
    assert all(ecc_cases.size_of(n) == (108, 192) for n in seen)


def test_reduce_is_the_kernels_order():
    rng = np.random.default_rng(3)
    for npx in (16, 512, 650, 888, 20736):
        v = rng.standard_normal((2, npx)) * 10.0 ** rng.integers(-8, 8, (2, npx))
        got = ecc_ref.reduce(v)
        for k in range(2):                                   # the same order, spelled out with scalars
            acc = [0.0] * 512
            for p in range(npx):
                acc[p % 512] += float(v[k, p])
            tot = 0.0
            for wv in range(8):
                lane = acc[64 * wv:64 * wv + 64]
                off = 32
                while off:
                    lane = [lane[j] + lane[j + off] for j in range(off)]
                    off //= 2
                tot += lane[0]
            assert got[k] == tot


@pytest.mark.parametrize("hw", ecc_cases.SMALL_SIZES, ids=lambda hw: "%dx%d" % hw)
def test_small_image_reference_equals_the_oracles_preprocess(hw):
    g = ecc_cases.gray_frames(hw)
    dh, dw = ecc_cases.SMALL_DIMS[hw]
    assert (ecc_ref.small_size(hw[0], 0.15), ecc_ref.small_size(hw[1], 0.15)) == (dh, dw)
    for f in g:
        s = ecc_ref.small(f)
        assert s.shape == (dh, dw) and np.array_equal(s, ecc.preprocess(ecc_cases.bgr(f)))
        if (hw[0] * 15) % 100 or (hw[1] * 15) % 100:        # 0.15 * size is no integer: taps from ssize / dsize give another picture
            assert not np.array_equal(s, ecc_ref.small(f, size_ratio=True)), hw
        else:
            assert np.array_equal(s, ecc_ref.small(f, size_ratio=True))


def test_small_image_sizes():
    assert [ecc_ref.small_size(s, 0.15) for s in (30, 50, 150, 170)] == [4, 8, 22, 26]        # 4.5, 7.5, 22.5, 25.5: lrint rounds to even
    assert ecc_cases.SMALL_DIMS[(30, 50)] == (4, 8) and ecc_cases.SMALL_DIMS[(150, 170)] == (22, 26)
    assert len(ecc_cases.gray_frames((720, 1280))) == 1 and all(len(ecc_cases.gray_frames(hw)) == 2 for hw in ecc_cases.SMALL_SIZES[:-1])


def test_session_clips_align_and_fail_where_the_gpu_test_needs_them_to():
    g = ecc_cases.clip_gray()
    assert np.array_equal(P.bgr2gray(ecc_cases.bgr(g[0])), g[0])                 # gray-valued BGR frames: the session's gray level 0 is the frame
    sm = ecc_ref.small(np.concatenate([g, np.zeros_like(g[:1])]))
    assert sm.shape == (5, 24, 30)
    res = {}
    for a, b in ((0, 1), (1, 2), (2, 3), (1, 3), (0, 3)):
        res[a, b] = ecc_ref.align(sm[a], sm[b])
        assert res[a, b][0] == 1 and np.abs(res[a, b][3] - IDENT).max() > 0.1
    for a, b in ((1, 4), (4, 3), (0, 4), (4, 4)):            # against or from the black frame: NaN correlation
        assert ecc_ref.align(sm[a], sm[b])[0] == 0
    assert not np.array_equal(res[1, 3][3], res[2, 3][3]) and not np.array_equal(res[0, 3][3], res[2, 3][3])


def test_operator_entry_points_are_declared():
    from eagle_amd import lib
    head = open(os.path.join(ROOT, "include", "eagle.h")).read()
    for name in ("eagle_op_ecc_small", "eagle_op_ecc"):
        assert re.search(r"^int %s\(" % name, head, re.M) and name in lib.EXPORTS
    assert callable(lib.op_ecc_small) and callable(lib.op_ecc)
    assert lib.ECC_DTYPE.itemsize == 40 and [lib.ECC_DTYPE.fields[k][1] for k in ("ok", "iters", "rho", "M")] == [0, 4, 8, 16]
