"""-m gpu: the ECC camera-motion kernels (csrc/ecc.hip, K17) alone, through the handle-free operators eagle_op_ecc_small / eagle_op_ecc, on the
constructed cases of tests/ecc_cases.py against tests/ecc_ref.py bit for bit: the small image byte for byte, ok / iters / M / rho of every
alignment, the warp after every one of the first iterations, many pairs in one launch against solo launches, the operators' refusals, and the
clip session (eagle_clip_motion_ecc) against the operators, with its range that starts behind a failed alignment.
tests/test_ecc_cases_cpu.py shows what each case forces and why bits may be compared (no float32 of a warp depends on the last bits of asin / sin / cos)."""
import functools

import numpy as np
import pytest

import ecc_cases
import ecc_ref
from ecc_cases import CASES, NAMES, expected
from eagle_amd import lib

pytestmark = pytest.mark.gpu
IDENT = [1, 0, 0, 0, 1, 0]
SCALE = 0.15


@functools.lru_cache(maxsize=None)
def _solo_bytes(name, max_iter=None, eps=None):
    t, i, mi, e = CASES[name]
    return lib.op_ecc(np.stack([t, i]), [[0, 1]], max_iter=mi if max_iter is None else max_iter, eps=e if eps is None else eps).tobytes()


def _solo(name, max_iter=None, eps=None):
    return np.frombuffer(_solo_bytes(name, max_iter, eps), lib.ECC_DTYPE)[0]


def _u32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _u64(v):
    return np.array([v], np.float64).view(np.uint64)[0]


def test_small_image_is_byte_exact():
    for hw in ecc_cases.SMALL_SIZES:
        g = ecc_cases.gray_frames(hw)
        got = lib.op_ecc_small(g)                            # the n > 1 stack in one call
        exp = ecc_ref.small(g)
        assert got.shape == exp.shape == (len(g),) + ecc_cases.SMALL_DIMS[hw]
        assert np.array_equal(got, exp), (hw, np.argwhere(got != exp)[:5])


@pytest.mark.parametrize("name", NAMES)
def test_alignment_is_bit_exact(name):
    """ok and iters equal; where the alignment succeeds, M equal as uint32 and rho as uint64 (a failed alignment's rho and M are ignored by the host)."""
    ok, iters, rho, M, _ = expected(name)
    r = _solo(name)
    print(f"{name}: ok {r['ok']} iters {r['iters']} rho {float(r['rho'])!r} (reference {ok} {iters} {rho!r})")
    assert (int(r["ok"]), int(r["iters"])) == (ok, iters)
    if ok:
        assert np.array_equal(_u32(r["M"]), _u32(M)), (r["M"], M)
        assert _u64(r["rho"]) == _u64(rho), (float(r["rho"]), rho, float(r["rho"]) - rho)


@pytest.mark.parametrize("name", ["rotm6_16x32", "cycle_24x37", "rot3_108x192"])
def test_iteration_trace_is_bit_exact(name):
    """max_iter = 1 .. 12 with eps = 0: the warp after every prefix equals the reference's trace, so that a divergence names its iteration"""
    K = 12
    trace = [r for r in expected(name, max_iter=K, eps=0.0)[4] if "M" in r]
    assert len(trace) == K
    for k in range(1, K + 1):
        r = _solo(name, max_iter=k, eps=0.0)
        assert (int(r["ok"]), int(r["iters"])) == (1, k)
        assert np.array_equal(_u32(r["M"]), _u32(trace[k - 1]["M"])), f"first difference in iteration {k}: {r['M']} != {trace[k - 1]['M']}"
        assert _u64(r["rho"]) == _u64(trace[k - 1]["rho"]), f"rho of iteration {k}"


@pytest.mark.parametrize("hw", ecc_cases.SIZES, ids=lambda hw: "%dx%d" % hw)
def test_pairs_in_one_launch_equal_solo_runs(hw):
    """every case of one size in a single launch (max_iter and eps belong to the launch, so the two cases with their own are left to the solo test), with
    repeated pairs, an image against itself, a carried template and a mixed pair: each result equals the solo launch's byte for byte, twice"""
    names = [n for n in NAMES if ecc_cases.size_of(n) == hw and CASES[n][2:] == (100, 1e-5)]
    assert len(names) >= 3
    stack = np.stack([CASES[n][k] for n in names for k in (0, 1)])
    pairs = [(2 * k, 2 * k + 1) for k in range(len(names))]
    want = [_solo_bytes(n) for n in names]
    pairs += pairs[:2] + pairs[-1:]                           # repeated pairs
    want += want[:2] + want[-1:]
    pairs.append((3, 3))                                     # an image against itself
    want.append(lib.op_ecc(stack[3:4], [[0, 0]]).tobytes())
    pairs.append((-1, 2 * len(names) - 1))                   # the last case's template as the carried image
    want.append(want[len(names) - 1])
    pairs.append((0, 3))                                     # a template and an image of different cases
    want.append(lib.op_ecc(np.stack([stack[0], stack[3]]), [[0, 1]]).tobytes())
    assert len(pairs) <= 64
    got = lib.op_ecc(stack, pairs, carry=CASES[names[-1]][0])
    for k, (p, w) in enumerate(zip(pairs, want)):
        assert got[k:k + 1].tobytes() == w, (k, p, got[k], np.frombuffer(w, lib.ECC_DTYPE)[0])
    again = lib.op_ecc(stack, pairs, carry=CASES[names[-1]][0])
    assert again.tobytes() == got.tobytes()


def test_operators_refuse_bad_arguments():
    t, i, _, _ = CASES["shift_a_24x37"]
    st = np.stack([t, i])
    assert lib.op_ecc_small(np.zeros((1, 26, 27), np.uint8)).shape == (1, 4, 4)          # 3.9 -> 4, 4.05 -> 4
    for hw in ((23, 40), (40, 23), (20, 20)):                # 3.45 -> 3
        with pytest.raises(lib.EagleError):
            lib.op_ecc_small(np.zeros((1,) + hw, np.uint8))
    with pytest.raises(lib.EagleError):
        lib.op_ecc_small(np.zeros((0, 64, 64), np.uint8))
    for bad in (np.zeros((2, 3, 8), np.uint8), np.zeros((2, 8, 3), np.uint8)):          # h < 4, w < 4
        with pytest.raises(lib.EagleError):
            lib.op_ecc(bad, [[0, 1]])
    for pairs in ([[0, 2]], [[2, 0]], [[0, -1]], [[-2, 0]], [[0, 1], [0, 5]]):          # indices outside [0, n); -1 is a template only
        with pytest.raises(lib.EagleError):
            lib.op_ecc(st, pairs, carry=t)
    with pytest.raises(lib.EagleError):
        lib.op_ecc(st, [[-1, 1]])                            # -1 without a carried image
    for max_iter in (-1, 101):
        with pytest.raises(lib.EagleError):
            lib.op_ecc(st, [[0, 1]], max_iter=max_iter)
    with pytest.raises(lib.EagleError):
        lib.op_ecc(st, [[0, 1]] * 4097)
    assert lib.op_ecc(st, np.zeros((0, 2), np.int32)).shape == (0,)                      # no pairs: nothing to do
    ok = lib.op_ecc(st, [[-1, 1]], carry=t, max_iter=100)
    assert ok.tobytes() == _solo_bytes("shift_a_24x37")


# ---- the clip session against the operators --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle():
    from eagle_amd.coordinate_model import CoordinateModel
    h = CoordinateModel(batch=1, frame_hw=ecc_cases.CLIP_HW).handle
    yield h
    h.close()


@functools.lru_cache(maxsize=None)
def _clip_small():
    """the small images of f0 .. f3 and of a black frame (index 4), from the session's own gray kernel and ecc_small_kernel"""
    g = np.concatenate([ecc_cases.clip_gray(), np.zeros((1,) + ecc_cases.CLIP_HW, np.uint8)])
    g0 = lib.op_gray_pyramid(ecc_cases.bgr(g))[0][0]
    assert np.array_equal(g0, g)
    sm = lib.op_ecc_small(g0)
    assert np.array_equal(sm, ecc_ref.small(g))
    return sm


def _frames(idx):
    g = np.concatenate([ecc_cases.clip_gray(), np.zeros((1,) + ecc_cases.CLIP_HW, np.uint8)])
    return ecc_cases.bgr(g[list(idx)])


def _session(h, idx, ranges, carry=False):
    """the frames idx (4 = black) as one clip; clip_motion_ecc over each range in turn -> [(warps, ok)]"""
    d = h.upload(_frames(idx))
    try:
        h.clip_open(d, len(idx))
        out = [h.clip_motion_ecc(first, count, carry=carry, return_ok=True) for first, count in ranges]
        h.clip_close()
    finally:
        h.free(d)
    return out


def _warp(a, b):
    """what the session must return for image b aligned to template a: (ok, the operator's M with the translation divided by the scale as the library does)"""
    r = lib.op_ecc(_clip_small(), [[a, b]])[0]
    W = r["M"].astype(np.float64)
    W[2] = np.float64(np.float32(np.float64(r["M"][2]) / SCALE)); W[5] = np.float64(np.float32(np.float64(r["M"][5]) / SCALE))
    return int(r["ok"]), W


def test_clip_session_and_operators_agree(handle):
    (w, ok), = _session(handle, [0, 1, 2, 3], [(0, 4)])
    assert ok.tolist() == [1, 1, 1, 1] and np.array_equal(w[0], IDENT)
    for f in (1, 2, 3):
        o, W = _warp(f - 1, f)
        assert o == 1 and np.array_equal(w[f], W), (f, w[f], W)
        assert np.abs(w[f] - IDENT).max() > 0.5              # a real alignment: more than half a pixel of the full frame


def test_range_after_a_failed_alignment_keeps_the_old_template(handle):
    """eagle_clip_motion_ecc's branch for a range whose predecessor failed: the template is the last frame that aligned, not the frame before the range"""
    seq = [0, 1, 4, 2, 3]                                    # f0 f1 black f2 f3
    (wa, oka), (wb, okb) = _session(handle, seq, [(0, 3), (3, 2)])
    (w, ok), = _session(handle, seq, [(0, 5)])
    assert ok.tolist() == [1, 1, 0, 1, 1]
    assert np.concatenate([wa, wb]).tobytes() == w.tobytes() and np.concatenate([oka, okb]).tobytes() == ok.tobytes()
    o13, W13 = _warp(1, 2)                                   # clip frame 3 is f2, clip frame 1 is f1
    o23, _ = _warp(4, 2)
    assert o13 == 1 and o23 == 0                             # aligned to the black frame it would have failed
    assert np.array_equal(wb[0], W13) and np.array_equal(w[2], IDENT)
    assert np.array_equal(wb[1], _warp(2, 3)[1])
    # two failures in a row inside one call
    (w, ok), = _session(handle, [0, 4, 4, 1], [(0, 4)])
    assert ok.tolist() == [1, 0, 0, 1] and np.array_equal(w[3], _warp(0, 1)[1]) and np.array_equal(w[1], IDENT) and np.array_equal(w[2], IDENT)
    # a clip that ends behind a failure carries the last frame that aligned
    handle.track_open()
    (wa, oka), = _session(handle, [0, 1, 4], [(0, 3)], carry=True)
    (wb, okb), = _session(handle, [2], [(0, 1)], carry=True)
    assert oka.tolist() == [1, 1, 0] and okb.tolist() == [1]
    assert np.array_equal(wb[0], _warp(1, 2)[1]) and not np.array_equal(wb[0], IDENT)
    handle.track_open()
