"""The shots stage on the GPU (include/eagle.h, eagle_op_shots / eagle_shots_device_frames / eagle_shots_frames; csrc/shots.hip): signatures, per-frame
rows and shots equal the contract of tests/shots_ref.py — np.array_equal, no tolerance — for the constructed clips of tests/shots_cases.py; through a
handle at 720 x 1280 from a device pointer, from pageable host memory with padded strides, from NV12, and with the staging bound forced below the
clip; one colour at 1080p (2 073 600 pixels in one counter); a call between two process calls leaves the records as they were; every refusal names
the value and leaves poisoned outputs alone; the command line's shots.json and its trimmed run."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import shots_cases as SC
import shots_ref as SR
import yuv_ref
from eagle_amd import lib, shots, synth, weights

pytestmark = pytest.mark.gpu

vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
PARTS = ("signatures", "frames", "shots")


def _equal(got, exp, what):
    for a, b, part in zip(got, exp, PARTS):
        if a.dtype.names:
            for k in a.dtype.names:
                assert np.array_equal(a[k], b[k]), (what, part, k)
        assert a.shape == b.shape and np.array_equal(a, b), (what, part)


@pytest.mark.parametrize("name", [c["name"] for c in SC.CASES])
def test_op_shots_equals_contract(name):
    c = SC.BY_NAME[name]
    _equal(lib.op_shots(c["frames"], lib.EagleShotParams(*[c["p"][k] for k in ("cut", "low", "grass_thr", "window", "min_len")])), SC.reference(name), name)


def test_unaligned_band_starts_and_two_runs():
    """17 x 33 frames start 1683 bytes apart, so the bands of successive frames start at every residue of 16 that a multiple of 3 can take"""
    r = np.random.default_rng(5)
    frames = r.integers(0, 256, (19, 17, 33, 3), np.uint8)
    exp = SR.shots(frames, SC.BASE)
    a, b = lib.op_shots(frames, **SC.BASE), lib.op_shots(frames, **SC.BASE)
    _equal(a, exp, "first")
    _equal(b, exp, "second")


def _poisoned(n, cap):
    rows, sh, sig = np.zeros(n, lib.SHOT_FRAME_DTYPE), np.zeros(cap, lib.SHOT_DTYPE), np.full((n, lib.SHOT_SIGNATURE), 0x5A5A5A5A, np.uint32)
    rows["d1"], sh["count"] = 77, 55
    return rows, sh, sig


def _untouched(rows, sh, sig):
    return (rows["d1"] == 77).all() and not rows["flags"].any() and (sh["count"] == 55).all() and (sig == 0x5A5A5A5A).all()


def test_refusals_name_the_value_and_leave_the_outputs_alone():
    L = lib.load()
    frames = np.ascontiguousarray(SC.BY_NAME["cuts_back_to_back"]["frames"])
    n, h, w, _ = frames.shape
    rows, sh, sig = _poisoned(n, n)
    m = C.c_int(-5)

    def op(p=None, n_=n, h_=h, w_=w, frames_a=frames, rows_a=rows, cap=n, par=True, count=True):
        q = lib.EagleShotParams(*[dict(SC.BASE, **(p or {}))[k] for k in ("cut", "low", "grass_thr", "window", "min_len")])
        rc = L.eagle_op_shots(0, vp(frames_a), n_, h_, w_, C.byref(q) if par else None, vp(rows_a), vp(sh), cap, C.byref(m) if count else None, vp(sig))
        return rc, L.eagle_last_error(None).decode()

    for change, text in SC.REFUSALS:
        rc, msg = op(p=change)
        assert rc == lib.E_INVALID and text in msg and _untouched(rows, sh, sig) and m.value == -5, (change, msg)
    for bh, bw in SC.BAD_SIZES:
        rc, msg = op(h_=bh, w_=bw)
        assert rc == lib.E_INVALID and f"{bh} x {bw}" in msg and _untouched(rows, sh, sig), (bh, bw, msg)
    for kw, text in ((dict(n_=-1), "-1"), (dict(cap=-2), "-2"), (dict(par=False), "NULL"), (dict(count=False), "NULL"), (dict(frames_a=None), "NULL"), (dict(rows_a=None), "NULL")):
        rc, msg = op(**kw)
        assert rc == lib.E_INVALID and text in msg and _untouched(rows, sh, sig), (kw, msg)
    q = lib.EagleShotParams(*[SC.BASE[k] for k in ("cut", "low", "grass_thr", "window", "min_len")])
    q.reserved[1] = 4
    assert L.eagle_op_shots(0, vp(frames), n, h, w, C.byref(q), vp(rows), vp(sh), n, C.byref(m), vp(sig)) == lib.E_INVALID and _untouched(rows, sh, sig)
    rc, msg = op(cap=2)                                                    # three shots: refused with the count, the other outputs alone
    assert rc == lib.E_INVALID and m.value == 3 and "3 shots" in msg and _untouched(rows, sh, sig)
    m.value = -5
    assert op(n_=0)[0] == 0 and m.value == 0 and _untouched(rows, sh, sig)           # n == 0: zero shots, nothing written
    assert op()[0] == 0 and m.value == 3
    _equal((sig, rows, sh[:3]), SC.reference("cuts_back_to_back"), "after the refusals")


# ---- through a handle -----------------------------------------------------------------------------------------------------------
H, W = 720, 1280
P720 = dict(SC.BASE, window=3)


@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=H, frame_w=W)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _banded(top, bottom, split):
    f = SC.solid(H, W, top)
    f[split:] = bottom
    return f


@pytest.fixture(scope="module")
def clip720():
    """14 frames: a banded pitch picture, a one-frame flash, a cut to a solid crowd colour, a two-frame dissolve (by rows) into another banded picture"""
    a, b, c = _banded(SC.GRASS, SC.GRASS2, 500), SC.solid(H, W, SC.CROWD), _banded(SC.GRASS2, SC.RED, 181)
    d1, d2 = b.copy(), b.copy()
    d1[0::3] = c[0::3]                                                    # a third, two thirds of the rows
    d2[0::3] = c[0::3]
    d2[1::3] = c[1::3]
    frames = np.stack([a, a, SC.solid(H, W, SC.WHITE), a, a, b, b, b, d1, d2, c, c, c, c])
    p = dict(P720, cut=26214)                                              # 0.4: the dissolve's steps score a third
    exp = SR.shots(frames, p)
    assert SC.flags(exp[1], SR.FLASH) == [2] and SC.flags(exp[1], SR.HARD) == [5] and SC.flags(exp[1], SR.GRADUAL_END) == [10] and len(exp[2]) == 4
    return frames, p, exp


def _cp(p):
    return lib.EagleShotParams(*[p[k] for k in ("cut", "low", "grass_thr", "window", "min_len")])


def test_handle_from_a_device_pointer(handle, clip720):
    frames, p, exp = clip720
    d = handle.upload(frames)
    try:
        _equal((exp[0],) + handle.shots_device(d, len(frames), _cp(p)), exp, "device")
        odd = C.c_void_p(d.value + H * W * 3 * 3)                          # from the fourth frame on: another clip, another answer
        _equal((exp[0],) + handle.shots_device(odd, 6, _cp(p)), (exp[0],) + SR.shots(frames[3:9], p)[1:], "window")
    finally:
        handle.free(d)


def test_handle_from_pageable_memory_with_padded_strides_and_forced_passes(handle, clip720):
    frames, p, exp = clip720
    n = len(frames)
    _equal((exp[0],) + handle.shots(frames, _cp(p)), exp, "dense host")
    padded = np.full((n, H + 3, W + 5, 3), 0xEE, np.uint8)
    padded[:, :H, :W] = frames
    view = padded[:, :H, :W]
    assert view.strides[0] > H * view.strides[1] and view.strides[1] > 3 * W
    _equal((exp[0],) + handle.shots(view, _cp(p)), exp, "padded host")
    fb = H * W * 3
    for bound in (1, fb, 3 * fb + 17, 5 * fb):                            # one frame per pass (twice), three, five: below the clip's 14 frames
        _equal((exp[0],) + handle.shots(frames, _cp(p), max_staging_bytes=bound), exp, ("staging", bound))
        _equal((exp[0],) + handle.shots(view, _cp(p), max_staging_bytes=bound), exp, ("padded staging", bound))
    L, m = handle.L, C.c_int(-5)
    rows, sh, _ = _poisoned(n, n)
    q = _cp(p)
    for rs, fs in ((3 * W - 1, 0), (-1, 0), (0, fb - 1), (3 * W + 3, H * (3 * W + 3) - 4 - 3 * W)):
        assert L.eagle_shots_frames(handle._h, vp(frames), n, rs, fs, 0, C.byref(q), vp(rows), vp(sh), n, C.byref(m)) == lib.E_INVALID
        assert "stride" in L.eagle_last_error(handle._h).decode() and (rows["d1"] == 77).all() and m.value == -5
    assert L.eagle_shots_frames(handle._h, vp(frames), n, 0, 0, -1, C.byref(q), vp(rows), vp(sh), n, C.byref(m)) == lib.E_INVALID
    assert L.eagle_shots_frames(handle._h, vp(frames), n, 0, 0, 0, C.byref(q), vp(rows), vp(sh), 3, C.byref(m)) == lib.E_INVALID and m.value == 4 and (rows["d1"] == 77).all()


def test_handle_from_nv12(handle, clip720):
    frames, p, _ = clip720
    r = np.random.default_rng(7)
    n = 6
    yuv = np.zeros((n, H * 3 // 2, W), np.uint8)
    for i, (y, u, v) in enumerate(((120, 90, 100), (120, 90, 100), (200, 128, 128), (60, 160, 180), (60, 160, 180), (60, 160, 180))):
        yuv[i, :H] = y
        yuv[i, H:, 0::2], yuv[i, H:, 1::2] = u, v
    yuv[:, :H] += r.integers(0, 3, (n, H, W), np.uint8)
    bgr = yuv_ref.nv12_to_bgr(yuv)
    exp = SR.shots(bgr, dict(shots.default_params(5), min_len=2))
    assert len(exp[2]) == 3
    res = shots.find_shots(handle, yuv, 5, "nv12", min_len=2)
    _equal((exp[0], res.frames, res.shots), exp, "nv12")
    assert res.params == dict(shots.default_params(5), min_len=2, fps=5, pixels=H * W)


def test_a_call_between_two_process_calls_leaves_the_records_unchanged(handle, clip720):
    frames, p, exp = clip720
    two = np.stack([synth.frame(0, 3), synth.noise_frame(2)])
    before = handle.process(two)
    _equal((exp[0],) + handle.shots(frames, _cp(p)), exp, "between")
    d = handle.upload(frames[:4])
    try:
        handle.shots_device(d, 4, _cp(p))
    finally:
        handle.free(d)
    after = handle.process(two)
    assert before.tobytes() == after.tobytes()


def test_one_colour_at_1080p_through_a_handle():
    hd = lib.Handle(batch=1, frame_h=1080, frame_w=1920)
    try:
        frames = np.broadcast_to(np.array(SC.GRASS, np.uint8), (3, 1080, 1920, 3))
        rows, sh = hd.shots(np.ascontiguousarray(frames), **SC.BASE)
        assert (rows["grass"] == 2073600).all() and not rows["d1"].any() and not rows["flags"].any()
        assert len(sh) == 1 and (sh[0]["first"], sh[0]["count"], sh[0]["kind"], sh[0]["flags"], sh[0]["grass_sum"]) == (0, 3, 0, SR.PITCH | SR.USABLE, 3 * 2073600)
        sig, rows1, _ = lib.op_shots(np.ascontiguousarray(frames[:1]), **SC.BASE)
        assert sig[0].max() == 2073600 and sig[0, :512].sum() == 2073600 and (sig[0, 512:1536].reshape(16, 64).sum(1) == 270 * 480).all() and sig[0, 1536] == 2073600
    finally:
        hd.close()


def test_cli_shots_and_trim(tmp_path):
    """a clip of two synthetic halves: six frames of the synthetic pitch, four frames of one noise picture.  shots.json must be the contract's result put
    through to_json; --trim-to-shot auto keeps the pitch half, and raw_coordinates.json then equals the run on that slice alone"""
    from eagle_amd import cli
    clip = np.concatenate([synth.clip(0, 6), np.stack([synth.noise_frame(3)] * 4)])
    np.save(tmp_path / "clip.npy", clip)
    np.save(tmp_path / "slice.npy", clip[:6])
    p = dict(shots.default_params(5), min_len=4)
    sig, rows, sh = SR.shots(clip, p)
    assert SC.bounds(sh) == [(0, 6, SR.START), (6, 4, SR.AFTER_CUT)] and list(sh["flags"]) == [SR.PITCH | SR.USABLE, 0]
    common = ["--fps", "5", "--synthetic-weights", "--batch", "2"]
    out, alone = str(tmp_path / "out"), str(tmp_path / "alone")
    assert cli.main(common + ["--clip", str(tmp_path / "clip.npy"), "--out", out, "--shots", "--shots-min-len", "4", "--trim-to-shot", "auto"]) == 0
    assert cli.main(common + ["--clip", str(tmp_path / "slice.npy"), "--out", alone]) == 0
    assert json.load(open(os.path.join(out, "shots.json"))) == shots.to_json(shots.Result(rows, sh, dict(p, fps=5, pixels=720 * 1280)))
    raw = json.load(open(os.path.join(out, "raw_coordinates.json")))
    assert len(raw) == 6 and open(os.path.join(out, "raw_coordinates.json"), "rb").read() == open(os.path.join(alone, "raw_coordinates.json"), "rb").read()
    meta, meta_alone = json.load(open(os.path.join(out, "metadata.json"))), json.load(open(os.path.join(alone, "metadata.json")))
    assert meta["shots"] == 2 and meta["trim"] == {"shot": 0, "first": 0, "count": 6} and meta["frames"] == 6
    assert set(meta) - set(meta_alone) == {"shots", "trim"} and not os.path.exists(os.path.join(alone, "shots.json"))
    with pytest.raises(SystemExit) as e:
        cli.main(common + ["--clip", str(tmp_path / "clip.npy"), "--out", out, "--trim-to-shot", "2"])
    assert "2 shots" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(common + ["--clip", str(tmp_path / "clip.npy"), "--out", out, "--trim-to-shot", "auto", "--shots-grass", "1.0"])
    assert "looks at the pitch" in str(e.value)
