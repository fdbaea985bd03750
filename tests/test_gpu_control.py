"""Kinematics and pitch control on the GPU (include/eagle.h, eagle_post_velocities / eagle_control_* / eagle_op_velocities / eagle_op_control /
eagle_op_minimap_control; csrc/post.hip, csrc/control.hip, csrc/minimap.hip): every output bit equals the numpy contract of tests/control_ref.py — no
tolerances — for the constructed tables of tests/control_cases.py; the minimap's control layer in BGR and NV12, dense and padded; through a handle on a
table eagle_postprocess built (host and device entries); every refusal."""
import ctypes as C
import functools

import numpy as np
import pytest

import annot_ref as A
import control_cases as CC
import control_ref as CR
import minimap_cases as MC
import minimap_ref as MR
import post_cases
from eagle_amd import lib, postprocess, weights

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in CC.CASES]


def _kin(c):
    return lib.kinematics_params(c["fps"], c["max_gap"], c["speed_cap"])


def _same(got, exp):
    return got.shape == exp.shape and got.dtype == exp.dtype and np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(got, exp, equal_nan=True)


@pytest.mark.parametrize("name", NAMES)
def test_op_velocities_equals_contract(name):
    c = CC.BY_NAME[name]
    assert _same(lib.op_velocities(c["values"], c["frames"], _kin(c)), CC.velocities(name))


@pytest.mark.parametrize("R", CR.RS)
@pytest.mark.parametrize("name", NAMES)
def test_op_control_equals_contract(name, R):
    c = CC.BY_NAME[name]
    exp, sums = CC.grids(name, R)
    got, share = lib.op_control(c["values"], CC.velocities(name), c["columns"], c["mapping"], lib.control_params(R), c["row0"], c["n"])
    bad = np.argwhere(got != exp)
    assert got.shape == exp.shape and not len(bad), (len(bad), bad[:5], got[tuple(bad[0])], exp[tuple(bad[0])])
    assert share.dtype == np.int64 and np.array_equal(share, sums)


def test_op_control_other_constants_and_unaligned_windows():
    c = CC.BY_NAME["sites22"]
    kw = dict(t_react=0.25, v_max=7.5, beta=2.5)
    exp, sums = CR.grids(c["values"], CC.velocities("sites22"), c["columns"], c["mapping"], 1, 2, 1, **kw)
    got, share = lib.op_control(c["values"], CC.velocities("sites22"), c["columns"], c["mapping"], lib.control_params(1, **kw), 1, 2)
    assert np.array_equal(got, exp) and np.array_equal(share, sums)


def test_op_control_given_velocities_clamp_and_non_finite():
    v, vel, cols, mapping = CC.given_velocities()
    for kw in (dict(), dict(t_react=1000.0), dict(t_react=0.0, v_max=0.001, beta=1e6)):
        exp = CR.grid(v, vel, cols, mapping, 0, 2, **{k: kw.get(k, d) for k, d in (("t_react", CR.T_REACT), ("v_max", CR.V_MAX), ("beta", CR.BETA))})
        got, share = lib.op_control(v, vel, cols, mapping, lib.control_params(2, **kw))
        assert np.array_equal(got[0], exp) and share[0] == exp.astype(np.int64).sum(), kw


# ---- the minimap's control layer ---------------------------------------------------------------------------------------------------
LAYER = [("sites22", 2, 0, 1), ("sites22", 4, 2, 1), ("sites22", 2, 2, 2), ("edges", 4, 0, 2), ("sites_0_1_2", 2, 2, 4), ("edges", 2, 0, 4)]      # (case, S, M, R)


@functools.lru_cache(maxsize=None)
def _layer_ref(name, S, M, R):
    c = CC.BY_NAME[name]
    n = min(c["n"], 2)
    fr = CR.frames_bgr(c["values"], CC.velocities(name), c["columns"], c["mapping"], c["row0"], n, S, M, R)
    fr.setflags(write=False)
    return fr, n


def _layer(name, S, M, R, fmt, layout=None, out=None):
    c = CC.BY_NAME[name]
    n = min(c["n"], 2)
    return lib.op_minimap_control(c["values"], CC.velocities(name), c["columns"], c["mapping"], lib.minimap_params(S, M, control=True), lib.control_params(R),
                                  c["row0"], n, fmt, layout, out)


@pytest.mark.parametrize("case", LAYER, ids=lambda k: "%s-S%d-M%d-R%d" % k)
def test_minimap_control_layer_equals_contract(case):
    fr, n = _layer_ref(*case)
    got = _layer(*case, "bgr")
    assert got.shape == fr.shape and np.array_equal(got, fr)
    assert len(np.unique(fr.reshape(-1, 3), axis=0)) > 3 or case[0] == "sites_0_1_2"
    exp = A.annotate(fr, [[] for _ in fr], "nv12")
    assert np.array_equal(_layer(*case, "nv12").reshape(-1), exp)


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_minimap_control_layer_padded(fmt):
    case = ("sites22", 2, 2, 2)
    fr, n = _layer_ref(*case)
    w, h = MR.size(2, 2)
    lay = ({"y_pitch": 3 * w + 40, "frame_stride": (3 * w + 40) * (h + 3)} if fmt == "bgr" else
           {"y_pitch": w + 64, "c_offset": (w + 64) * (h + 16), "c_pitch": w + 64, "frame_stride": (w + 64) * (2 * h + 40)})
    exp = A.annotate(fr, [[] for _ in fr], fmt, lay, 0xA5)
    got = _layer(*case, fmt, lay, np.full(exp.size, 0xA5, np.uint8))
    assert np.array_equal(got, exp)


def test_minimap_without_control_is_unchanged():
    for name in ("sites22", "edges_voronoi", "footprints_a"):
        c = MC.BY_NAME[name]
        kw = c["kw"]
        p = lib.minimap_params(c["S"], c["M"], kw.get("voronoi", 0), kw.get("footprint", 1), kw.get("player_radius", 0), kw.get("ball_radius", 0), control=False)
        assert np.array_equal(lib.op_minimap(c["values"], c["columns"], c["mapping"], p, c["row0"], c["n"]), MC.reference(name))
        vel = np.zeros_like(c["values"])
        assert np.array_equal(lib.op_minimap_control(c["values"], vel, c["columns"], c["mapping"], p, lib.control_params(1), c["row0"], c["n"]), MC.reference(name))


# ---- through a handle ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handle(state_dicts):
    hd = lib.Handle(batch=2, frame_h=720, frame_w=1280)
    weights.load_into(hd, list(state_dicts))
    yield hd
    hd.close()


def _columns(table):
    return [(int(k["kind"]), int(k["id"]), int(k["video"])) for k in table.columns]


def test_handle_velocities_control_and_layer(handle):
    case = post_cases.BY_NAME["goalkeeper_fold"]
    tm = case["team_mapping"]
    t = postprocess.process_data(handle, post_cases.records_of(case), case["fps"], case["frame_w"], tm)
    reader = None
    try:
        values, cols, rows = np.array(t.values), _columns(t), len(t.rows)
        assert rows == 16
        fps = case["fps"]
        d_v = C.c_void_p(1)
        assert handle.L.eagle_post_device_velocity_values(t._t, C.byref(d_v)) == 0 and not d_v.value         # none before eagle_post_velocities
        vel = handle.velocities(t, fps, max_gap=3, speed_cap=9.0)
        assert handle.L.eagle_post_device_velocity_values(t._t, C.byref(d_v)) == 0 and d_v.value and d_v.value != t.device_values
        assert handle.L.eagle_post_device_velocity_values(t._t, None) == lib.E_INVALID
        exp_v = CR.velocities(values, t.rows, fps, 3, 9.0)
        assert _same(vel, exp_v) and np.isfinite(vel).any() and np.isnan(vel).any()
        assert _same(handle.velocities(t, fps), CR.velocities(values, t.rows, fps))          # a second call replaces the first
        exp_v = CR.velocities(values, t.rows, fps)
        from eagle_amd import control as ct
        k = ct.kinematics(handle, t, fps)
        assert _same(k["velocities"], exp_v) and k["players"] == CR.kinematics(values, exp_v, t.rows, cols, fps)
        for pl in k["players"]:                                                     # the same figures, step by step
            c = cols.index((MR.PLAYER if pl["type"] == "Player" else MR.GOALKEEPER, pl["id"], 0))
            sp = [float(np.sqrt(exp_v[c, r, 0] * exp_v[c, r, 0] + exp_v[c, r, 1] * exp_v[c, r, 1])) for r in range(rows)]      # (the contract's speed: not hypot)
            steps = [r for r in range(rows - 1) if sp[r] == sp[r] and sp[r + 1] == sp[r + 1] and t.rows[r + 1] - t.rows[r] <= fps]
            assert pl["distance"] == pytest.approx(sum((sp[r] + sp[r + 1]) / 2 * (int(t.rows[r + 1]) - int(t.rows[r])) / fps for r in steps), abs=1e-12)
            assert pl["top_speed"] == max([x for x in sp if x == x], default=0.0)
        # host entry: all rows, a window, n == 0
        p2 = lib.control_params(2)
        exp_g, exp_s = CR.grids(values, exp_v, cols, tm, 0, rows, 2)
        got, sums = handle.control(t, p2)
        assert np.array_equal(got, exp_g) and np.array_equal(sums, exp_s)
        got, sums = handle.control(t, p2, 5, 3)
        assert np.array_equal(got, exp_g[5:8]) and np.array_equal(sums, exp_s[5:8])
        assert handle.control(t, p2, 16, 0)[0].shape == (0, 136, 210)
        grids, share = ct.control(handle, t, 2, rows=(1, 15))
        assert np.array_equal(grids, exp_g[1:]) and np.array_equal(share, CR.share(exp_s[1:], 2))
        # device entry: 15 grids of 210 x 136 bytes and their 15 sums behind them, fetched byte for byte by a handle whose BGR frames are 204 x 140 (3 grids each)
        fb, ng = 140 * 204 * 3, 15
        assert fb == 3 * 210 * 136
        d_out = handle.upload(np.full(6 * fb, 0xA5, np.uint8))
        reader = lib.Handle(batch=6, frame_h=140, frame_w=204)
        try:
            handle.control_device(t, d_out, p2, 1, ng, C.c_void_p(d_out.value + 5 * fb))
            raw = reader.annotate(d_out, 6, np.zeros(6, lib.RESULT_DTYPE), None, "bgr").reshape(-1)
            assert np.array_equal(raw[: 5 * fb].reshape(ng, 136, 210), exp_g[1:])
            assert np.array_equal(raw[5 * fb: 5 * fb + 8 * ng].view(np.int64), exp_s[1:]) and (raw[5 * fb + 8 * ng:] == 0xA5).all()
        finally:
            handle.free(d_out)
        # the layer through the handle: host entry, a window, I420
        S, M = 2, 2
        par = lib.minimap_params(S, M, control=True)
        handle.minimap_set_control(t, p2)
        ref = CR.frames_bgr(values, exp_v, cols, tm, 0, rows, S, M, 2)
        assert np.array_equal(handle.minimap(t, par), ref)
        assert np.array_equal(handle.minimap(t, par, 5, 3, "i420").reshape(-1), A.annotate(ref[5:8], [[], [], []], "i420"))
        from eagle_amd.minimap import minimap
        assert np.array_equal(minimap(handle, t, S, M, control=lib.control_params(1), rows=(2, 2)), CR.frames_bgr(values, exp_v, cols, tm, 2, 2, S, M, 1))
        assert np.array_equal(handle.minimap(t, lib.minimap_params(S, M, voronoi=True)), MR.frames_bgr(values, cols, tm, 0, rows, S, M, voronoi=1))
    finally:
        t.close()
        if reader is not None:
            reader.close()


def test_refusals(handle):
    L = handle.L
    c = CC.BY_NAME["sites_0_1_2"]
    values, vel = np.ascontiguousarray(c["values"]), np.ascontiguousarray(CC.velocities("sites_0_1_2"))
    cols = np.array([(k, i, v, 0) for k, i, v in c["columns"]], lib.POSTCOL_DTYPE)
    ids, vals = np.array([1, 2], np.int32), np.array([0, 1], np.int32)
    frames = np.ascontiguousarray(c["frames"])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.full(3 * 7140, 0x5A, np.uint8)
    share = np.full(3, 0x5A5A, np.int64)
    vout = np.full(values.shape, 7.0)

    def op_c(params=lib.control_params(1), vel_p=vp(vel), ids_p=vp(ids), row0=0, n=1, out_p=vp(out)):
        rc = L.eagle_op_control(0, vp(values), vel_p, vp(cols), 3, len(cols), ids_p, vp(vals), 2, None if params is None else C.byref(params), row0, n, out_p, vp(share))
        assert (out == 0x5A).all() and (share == 0x5A5A).all()
        return rc, L.eagle_last_error(None).decode()

    bad = [dict(params=None), dict(params=lib.control_params(3)), dict(params=lib.control_params(0)), dict(params=lib.control_params(8)),
           dict(params=lib.control_params(1, v_max=0.0)), dict(params=lib.control_params(1, v_max=-5.0)), dict(params=lib.control_params(1, beta=0.0)),
           dict(params=lib.control_params(1, beta=-1.0)), dict(params=lib.control_params(1, t_react=-0.5)),
           dict(vel_p=None), dict(ids_p=None), dict(out_p=None), dict(row0=3, n=1), dict(row0=-1), dict(n=4), dict(n=-1), dict(row0=2, n=2)]
    for kw in bad:
        rc, msg = op_c(**kw)
        assert rc == lib.E_INVALID and msg, kw
    assert op_c(n=0)[0] == 0 and op_c(row0=3, n=0)[0] == 0

    def op_v(params=lib.kinematics_params(5), fr=frames, out_p=vp(vout)):
        rc = L.eagle_op_velocities(0, vp(values), vp(fr), 3, len(cols), None if params is None else C.byref(params), out_p)
        assert (vout == 7.0).all()
        return rc, L.eagle_last_error(None).decode()

    for kw in (dict(params=None), dict(params=lib.kinematics_params(0)), dict(params=lib.kinematics_params(-5)), dict(params=lib.kinematics_params(5, 0)),
               dict(params=lib.kinematics_params(5, -1)), dict(params=lib.kinematics_params(5, 5, 0.0)), dict(params=lib.kinematics_params(5, 5, -1.0)),
               dict(params=lib.kinematics_params(5, 5, float("nan"))), dict(fr=np.array([3, 3, 6], np.int32)), dict(out_p=None)):
        rc, msg = op_v(**kw)
        assert rc == lib.E_INVALID and msg, kw

    # the layer: with voronoi, without a mapping, without velocities (eagle_op_minimap has none), bad control parameters
    w, h = MR.size(2, 0)
    pic = np.full(w * h * 3, 0x5A, np.uint8)

    def op_m(entry_control=True, params=lib.minimap_params(2, 0, control=True), cp=lib.control_params(1), vel_p=vp(vel), ids_p=vp(ids), row0=0, n=1):
        if entry_control:
            rc = L.eagle_op_minimap_control(0, vp(values), vel_p, vp(cols), 3, len(cols), ids_p, vp(vals), 2, C.byref(params), None if cp is None else C.byref(cp), row0, n, 0, None, vp(pic))
        else:
            rc = L.eagle_op_minimap(0, vp(values), vp(cols), 3, len(cols), ids_p, vp(vals), 2, C.byref(params), row0, n, 0, None, vp(pic))
        assert (pic == 0x5A).all()
        return rc, L.eagle_last_error(None).decode()

    for kw in (dict(params=lib.minimap_params(2, 0, voronoi=True, control=True)), dict(ids_p=None), dict(vel_p=None), dict(entry_control=False), dict(cp=None),
               dict(cp=lib.control_params(3)), dict(cp=lib.control_params(1, beta=0.0)), dict(row0=3), dict(n=4)):
        rc, msg = op_m(**kw)
        assert rc == lib.E_INVALID and msg, kw
    assert op_m(n=0)[0] == 0 and op_m(entry_control=False, params=lib.minimap_params(2, 0), n=0)[0] == 0

    # the handle entries
    case = post_cases.BY_NAME["goalkeeper_fold"]
    t = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, case["team_mapping"])
    bare = postprocess.process_data(handle, post_cases.records_of(case), 25, 1280, None)             # no mapping
    try:
        big = np.full(16 * 7140, 0x5A, np.uint8)
        sh = np.full(16, 0x5A5A, np.int64)
        good = lib.control_params(1)
        par = lib.minimap_params(2, 0, control=True)
        pics = np.full(16 * w * h * 3, 0x5A, np.uint8)

        def hc(entry, table, params, row0, n, dst=vp(big)):
            rc = entry(handle._h, table, row0, n, None if params is None else C.byref(params), dst, vp(sh))
            assert (big == 0x5A).all() and (sh == 0x5A5A).all()
            return rc, L.eagle_last_error(handle._h).decode()

        def hm(entry, table, row0=0, n=1):
            rc = entry(handle._h, table, row0, n, C.byref(par), 0, None, vp(pics))
            assert (pics == 0x5A).all()
            return rc, L.eagle_last_error(handle._h).decode()

        entries = (L.eagle_control_grids, L.eagle_control_device_grids)
        draws = (L.eagle_minimap_frames, L.eagle_minimap_device_frames)
        for entry in entries:                                                      # control without velocities
            rc, msg = hc(entry, t._t, good, 0, 1)
            assert rc == lib.E_INVALID and "velocities" in msg
        for entry in draws:
            rc, msg = hm(entry, t._t)
            assert rc == lib.E_INVALID and "velocities" in msg
        for p in (None, lib.kinematics_params(0), lib.kinematics_params(25, 0), lib.kinematics_params(25, 25, 0.0)):
            assert L.eagle_post_velocities(handle._h, t._t, None if p is None else C.byref(p)) == lib.E_INVALID and L.eagle_last_error(handle._h)
        assert L.eagle_post_velocities(handle._h, None, C.byref(lib.kinematics_params(25))) == lib.E_INVALID
        assert L.eagle_post_velocity_values(t._t, vp(np.zeros(4))) == lib.E_INVALID
        handle.velocities(t, 25); handle.velocities(bare, 25)
        for entry in draws:                                                        # the layer without its parameters, then with voronoi, then without a mapping
            rc, msg = hm(entry, t._t)
            assert rc == lib.E_INVALID and "parameters" in msg
        assert L.eagle_minimap_set_control(t._t, C.byref(lib.control_params(3))) == lib.E_INVALID
        handle.minimap_set_control(t, good); handle.minimap_set_control(bare, good)
        par = lib.minimap_params(2, 0, voronoi=True, control=True)
        for entry in draws:
            assert hm(entry, t._t)[0] == lib.E_INVALID
        par = lib.minimap_params(2, 0, control=True)
        for entry in draws:
            rc, msg = hm(entry, bare._t)
            assert rc == lib.E_INVALID and "mapping" in msg
            assert hm(entry, t._t, 16, 1)[0] == lib.E_INVALID and hm(entry, t._t, 0, 17)[0] == lib.E_INVALID and hm(entry, t._t, 16, 0)[0] == 0
        for entry in entries:
            for args in ((bare._t, good, 0, 1), (t._t, None, 0, 1), (t._t, lib.control_params(3), 0, 1), (t._t, lib.control_params(1, v_max=0.0), 0, 1),
                         (t._t, lib.control_params(1, beta=0.0), 0, 1), (t._t, lib.control_params(1, t_react=-1.0), 0, 1), (None, good, 0, 1),
                         (t._t, good, 0, 17), (t._t, good, 16, 1), (t._t, good, -1, 1), (t._t, good, 0, -1)):
                rc, msg = hc(entry, *args)
                assert rc == lib.E_INVALID and msg, args
            assert hc(entry, t._t, good, 0, 1, dst=None)[0] == lib.E_INVALID
            assert hc(entry, t._t, good, 16, 0)[0] == 0 and hc(entry, t._t, good, 3, 0)[0] == 0
        assert handle.control(t, good, 0, 1)[0].shape == (1, 68, 105)               # the handle still works
    finally:
        t.close(); bare.close()


def test_cli_kinematics_and_control(tmp_path):
    import json
    import os
    from eagle_amd import cli
    out = str(tmp_path / "out")
    common = ["--frames", "6", "--fps", "5", "--seed", "0", "--synthetic-weights", "--batch", "3", "--out", out, "--processed"]
    assert cli.main(common + ["--kinematics", "--control-grid", "1", "--minimap-control", "--minimap-scale", "2"]) == 0
    rows = len(json.load(open(os.path.join(out, "processed_data.json"))))
    kin = json.load(open(os.path.join(out, "kinematics.json")))
    assert kin["fps"] == 5 and all(set(p) == {"id", "type", "distance", "top_speed"} and p["top_speed"] <= 12.0 + 1e-9 for p in kin["players"])
    g = np.load(os.path.join(out, "control.npy"))
    sh = json.load(open(os.path.join(out, "control_share.json")))
    assert g.shape == (rows, 68, 105) and g.dtype == np.uint8 and len(sh["team0_share"]) == rows
    assert np.allclose(sh["team0_share"], g.reshape(rows, -1).astype(np.int64).sum(1) / (255.0 * 7140))
    w, h = MR.size(2, 4)
    blob = open(os.path.join(out, "minimap.y4m"), "rb").read()
    assert len(blob.split(b"\n", 1)[1]) == rows * (6 + w * h * 3 // 2)
