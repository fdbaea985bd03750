"""The optical-flow kernels alone (gray_kernel, pyrdown_kernel, lk_kernel of csrc/flow.hip; flow_filter_kernel of geom.hip) on the small constructed cases of
tests/lk_cases.py, through the handle-free operators eagle_op_gray_pyramid / eagle_op_flow, against tests/lk_ref.py AND the oracle (oracle/eo_flow.c,
oracle/flow.py), bit for bit; both workgroup forms of K12 (256 threads, and the one-wave form behind eagle_debug("lk_threads", 64)).  What each case forces is
proven without a GPU by tests/test_lk_cases_cpu.py.  No case and no point is skipped."""
import os

os.environ["EAGLE_ENABLE_DEBUG"] = "1"          # eagle_debug (the lk_threads switch) is inert without it; read once, at its first call

import numpy as np
import pytest

import lk_cases
import lk_ref
from lk_cases import CASES, expected, key_points
from eagle_amd import lib
from oracle import flow
from oracle import prims as P

pytestmark = pytest.mark.gpu
NAMES = sorted(CASES)


def _clips():
    seen = {}
    for n in NAMES:
        seen.setdefault(id(CASES[n][0]), n)
    return sorted(seen.values())


def to_flowkp(kps):
    a = np.zeros(len(kps), lib.FLOWKP_DTYPE)
    for k, (lab, (x, y)) in enumerate(kps):
        a[k] = (lab, x, y, 0.0)
    return a


def from_flowkp(a):
    return [(int(k["label"]), (int(k["x"]), int(k["y"]))) for k in a]


@pytest.mark.parametrize("name", _clips())
def test_gray_pyramid_equals_reference(name):
    frames = CASES[name][0]
    n, h, w, _ = frames.shape
    g, levels = lib.op_gray_pyramid(frames)
    assert levels == lk_ref.levels(h, w)
    g0 = np.stack([lk_ref.gray(f) for f in frames])
    g1 = np.stack([lk_ref.pyrdown(x) for x in g0])
    g2 = np.stack([lk_ref.pyrdown(x) for x in g1])
    for l, (got, ref) in enumerate(zip(g, (g0, g1, g2))):
        assert got.shape == ref.shape and np.array_equal(got, ref), (name, "level", l, np.argwhere(got != ref)[:4])
    assert np.array_equal(g[0], np.stack([P.bgr2gray(f) for f in frames]))
    assert np.array_equal(g[2], np.stack([P.pyrdown(P.pyrdown(x)) for x in g[0]]))


@pytest.mark.parametrize("name", NAMES)
def test_flow_equals_reference_and_oracle(name):
    frames, src, dst, pts = CASES[name]
    kps = key_points(pts)
    exp, enxt, est, _ = expected(name)
    gs, gd = P.bgr2gray(frames[src]), P.bgr2gray(frames[dst])
    onxt, ost = P.calc_optical_flow_pyr_lk(gs, gd, np.array(pts, np.float32)) if pts else (np.zeros((0, 2), np.float32), np.zeros((0, 1), np.uint8))
    oexp = [(k, (int(v[0]), int(v[1]))) for k, v in flow.calculate_optical_flow(frames[dst], gs, dict(kps), gd).items()]
    runs = {}
    try:
        for threads in (256, 64):
            lib.debug("lk_threads", threads)
            got, nxt, st = lib.op_flow(frames, src, dst, dst, to_flowkp(kps))
            runs[threads] = (from_flowkp(got), nxt.copy(), st.copy())
    finally:
        lib.debug("lk_threads", 256)
    for threads, (got, nxt, st) in runs.items():
        assert len(st) == len(pts)
        assert np.array_equal(st, est), (name, threads, "status != lk_ref", [pts[k] for k in np.nonzero(st != est)[0]])
        assert np.array_equal(st, ost[:, 0]), (name, threads, "status != oracle")
        t = st == 1
        bad = np.nonzero((nxt[t].view(np.uint32) != enxt[t].view(np.uint32)).any(1))[0]
        assert len(bad) == 0, (name, threads, "LK points != lk_ref", [(np.array(pts)[t][k].tolist(), nxt[t][k].tolist(), enxt[t][k].tolist()) for k in bad[:4]])
        assert np.array_equal(nxt[t].view(np.uint32), onxt[t].view(np.uint32)), (name, threads, "LK points != oracle")
        assert got == exp, (name, threads, "filtered dict != lk_ref")
        assert got == oexp, (name, threads, "filtered dict != oracle")
    a, b = runs[256], runs[64]
    assert a[0] == b[0] and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2]), (name, "256 and 64 threads differ")


def test_operators_refuse_small_frames_and_too_many_points():
    one = to_flowkp([(0, (10, 10))])
    for h, w in ((31, 40), (40, 31)):
        frames = np.zeros((2, h, w, 3), np.uint8)
        with pytest.raises(lib.EagleError, match=r"\(-1\)"):
            lib.op_gray_pyramid(frames)
        with pytest.raises(lib.EagleError, match=r"\(-1\)"):
            lib.op_flow(frames, 0, 1, 1, one)
    frames = CASES["translate_32x32"][0]
    with pytest.raises(lib.EagleError, match=r"\(-1\)"):
        lib.op_flow(frames, 0, 1, 1, to_flowkp([(k % 57, (10, 10)) for k in range(58)]))
    with pytest.raises(lib.EagleError, match=r"\(-1\)"):
        lib.op_flow(frames, 0, 2, 1, one)                        # a frame outside the clip
    got, nxt, st = lib.op_flow(frames, 0, 1, 1, to_flowkp([(k, (10, 10)) for k in range(57)]))      # 57 points and 32 x 32 pixels are inside the limits
    assert len(st) == 57


def test_clip_session_and_operator_run_the_same_flow(state_dicts):
    """The level rule moved out of clip_open into one function: a 1280 x 720 pair through clip_open / clip_flow on a finalised handle and through
    eagle_op_flow must give identical bytes."""
    import flow_cases
    from eagle_amd.coordinate_model import CoordinateModel
    hs, ys = state_dicts
    frames = np.stack(flow_cases.frames_of("fps25")[:2])
    rng = np.random.default_rng(5)
    pts = [(int(x), int(y)) for x, y in zip(rng.integers(-20, 1300, 45), rng.integers(-20, 740, 45))]
    pts += [(int(x), int(y)) for _, (x, y) in sorted(flow_cases.synth.visible_landmarks(2, 60).items())[:12]]
    kps = to_flowkp(key_points(pts))
    m = CoordinateModel(precision="f16", batch=8, hrnet_state_dict=hs, detector_state_dict=ys)
    h = m.handle
    d = h.upload(frames)
    try:
        h.clip_open(d, len(frames))
        for (a, b) in ((0, 1), (1, 0), (1, 1)):
            got, nxt, st = h.clip_flow(a, b, b, kps, raw=True)
            ogot, onxt, ost = lib.op_flow(frames, a, b, b, kps)
            assert st.sum() >= 12
            assert got.tobytes() == ogot.tobytes() and nxt.tobytes() == onxt.tobytes() and st.tobytes() == ost.tobytes(), (a, b)
    finally:
        h.clip_close(); h.free(d)
        m.handle.close()
    g, levels = lib.op_gray_pyramid(frames[:1])
    assert levels == 2 and np.array_equal(g[0][0], P.bgr2gray(frames[0])) and np.array_equal(g[2][0], P.pyrdown(P.pyrdown(g[0][0])))
