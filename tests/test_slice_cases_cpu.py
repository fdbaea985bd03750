"""The references and case lists of tests/slice_cases.py checked on the CPU (no GPU): the pools against torch.nn.functional.max_pool2d, three chained 5 x 5
pools against windows 5 / 9 / 13 (SPPF), the nearest up-sampling against F.interpolate, and unslice against one overwritten sentinel and one NaN inside."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import slice_cases as S


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))


def _nhwc(t):
    return t.numpy().transpose(0, 2, 3, 1)


@pytest.mark.parametrize("h,w", S.POOL_MAPS)
def test_maxpool5_ref_is_torch_max_pool2d(h, w):
    x = S.pool_input(2, h, w, 16, "f32")
    assert np.array_equal(S.maxpool5_ref(x), _nhwc(F.max_pool2d(_nchw(x), 5, 1, 2)))
    assert (S.maxpool5_ref(x)[..., 1] < 0).all(), "zero padding won in the strictly negative channel"


@pytest.mark.parametrize("h,w", S.POOL_MAPS)
def test_three_chained_pools_are_windows_5_9_13(h, w):
    x = S.pool_input(3, h, w, 16, "f16")
    p1 = S.maxpool5_ref(x); p2 = S.maxpool5_ref(p1); p3 = S.maxpool5_ref(p2)
    for got, k in ((p1, 5), (p2, 9), (p3, 13)):
        assert np.array_equal(got, S.maxpool_ref(x, k))
        assert np.array_equal(got, _nhwc(F.max_pool2d(_nchw(x), k, 1, k // 2)))


@pytest.mark.parametrize("h,w", S.UP_MAPS)
def test_upsample2_ref_is_interpolate_nearest_cropped(h, w):
    x = S.tensor([1, h, w], (2, h, w, 16))
    full = _nhwc(F.interpolate(_nchw(x), scale_factor=2, mode="nearest"))
    sizes = S.up_sizes(h, w)
    assert len(sizes) == 4 and (2 * h - 1, 2 * w - 1) in sizes and (2 * h, 2 * w) in sizes      # a 1 x 1 map too: 1 x 1, 1 x 2, 2 x 1, 2 x 2
    for yh, yw in sizes:
        assert np.array_equal(S.upsample2_ref(x, yh, yw), full[:, :yh, :yw])
    with pytest.raises(AssertionError):
        S.upsample2_ref(x, 2 * h + 1, 2 * w)


def test_split_value_and_its_edges():
    v = S.split_value(S.SPLIT_EDGES)
    assert np.isfinite(v).all() and np.abs(v).max() == np.float32(4094.0)
    assert np.array_equal(S.split_value(v), v), "storing a stored value again keeps it"
    assert np.abs(v - S.SPLIT_EDGES).max() <= 2.0 ** -22 * 4094.0
    assert v[8] == 0 and v[9] == 0 and not np.signbit(v[9]), "-0 is stored as hi = -0, lo = +0: the sum is +0"
    s = S.SPLIT_EDGES[10:13] * np.float32(16)
    lo = (s - s.astype(np.float16).astype(np.float32)).astype(np.float16)
    assert ((lo != 0) & (np.abs(lo.astype(np.float32)) < 2.0 ** -14)).all(), "the subnormal-lo cases have a non-zero subnormal lo"
    assert np.isnan(S.split_value(S.buffer((1, 1, 1, 8)))).all() and np.isnan(S.stored(S.buffer((1, 1, 1, 8)), "f16")).all()


@pytest.mark.parametrize("fmt", S.FMTS)
def test_unslice_rejects_an_overwritten_sentinel_and_a_nan_inside(fmt):
    dense = S.tensor([2], (2, 3, 4, 16))
    whole = S.stored(S.place(S.buffer((2, 3, 4, 48)), 16, dense), fmt)
    assert np.array_equal(S.unslice(whole, 16, 16, fmt), S.stored(dense, fmt))
    for ch in (15, 32, 0, 47):                                  # either neighbour, the first and the last channel of the pixel
        bad = whole.copy(); bad[1, 2, 3, ch] = 0.0
        with pytest.raises(AssertionError, match="overwritten"):
            S.unslice(bad, 16, 16, fmt)
    bad = whole.copy(); bad[0, 0, 0, 16] = np.nan
    with pytest.raises(AssertionError, match="NaN inside"):
        S.unslice(bad, 16, 16, fmt)
    # a buffer with values outside the slice (the C2f residual next to the output): they must come back as they were stored
    before = S.place(S.place(S.buffer((2, 3, 4, 48)), 16, dense), 32, dense * np.float32(1.37))
    after = S.stored(before, fmt)
    assert np.array_equal(S.unslice(after, 16, 16, fmt, before=before), S.stored(dense, fmt))
    bad = after.copy(); bad[0, 1, 2, 40] = np.nextafter(bad[0, 1, 2, 40], np.float32(9)) if fmt == "f32" else bad[0, 1, 2, 40] * np.float32(1.5) + np.float32(1)
    with pytest.raises(AssertionError, match="overwritten"):
        S.unslice(bad, 16, 16, fmt, before=before)
    if fmt == "f32":                                            # fp32 keeps the payload: another NaN is not the sentinel
        bad = whole.copy(); bad[0, 0, 0, 0] = np.float32(np.nan)
        with pytest.raises(AssertionError, match="overwritten"):
            S.unslice(bad, 16, 16, fmt)


def test_case_lists_cover_what_they_claim():
    cases = S.conv_cases()
    assert len(cases) == len(set(cases))
    for ks, st in S.KS_STRIDE:
        for mode in S.MODES:
            sub = [c for c in cases if c[:3] == (ks, st, mode)]
            assert (len(sub) == 0) == (mode == "r_in_x" and st == 2)
            assert not sub or {c[3] for c in sub} == set(S.GEOMS)
    for mode in S.MODES:
        assert {c[4] for c in cases if c[2] == mode} == set(S.MAPS), "every mode meets every map"
    assert {g["c"] for g in S.GEOMS.values()} == {16, 32, 48, 64, 80}
    assert {g["x_cs"] for g in S.GEOMS.values()} | {g["y_cs"] for g in S.GEOMS.values()} == {48, 80, 144, 208}
    for g in S.GEOMS.values():
        c = g["c"]
        for cs, offs in ((g["x_cs"], (g["x_off"], g["rx"])), (g["y_cs"], (g["y_off"], g["ry"]))):
            assert cs & (cs - 1) and all(o % 16 == 0 and o + c <= cs for o in offs)
            assert offs[0] + c <= offs[1] or offs[1] + c <= offs[0], "the two slices of one buffer are disjoint"
    assert any(g["x_off"] == 0 for g in S.GEOMS.values()) and any(g["y_off"] == 0 for g in S.GEOMS.values())                         # a first slice
    assert any(g["x_off"] + g["c"] == g["x_cs"] for g in S.GEOMS.values()) and any(g["y_off"] + g["c"] == g["y_cs"] for g in S.GEOMS.values())   # a last slice
    assert any(w > 32 for _, _, w in S.MAPS)
    assert sorted(int(f.split(",")[2]) for p, f, *_ in S.AD_FORMS if p == "f16") == [6, 6, 7, 7, 8, 9, 10, 11]
    assert sorted(int(f.split(",")[2]) for p, f, *_ in S.AD_FORMS if p == "f32s") == [8, 9, 10, 11, 12, 13, 14, 15, 19, 21, 22, 23, 24]


def test_conv_operands_place_every_operand_where_the_mode_says():
    G = S.GEOMS["c48"]
    x, wt, b, rs = S.conv_data(3, 1, 48, 48, (2, 9, 13), 1)
    for mode in S.MODES + ("c2f_x",):
        op = S.conv_operands(mode, G, x, rs, 9, 13, 48)
        assert np.array_equal(op["x"][..., op["x_off"]:op["x_off"] + 48], x)
        assert np.isnan(op["y"][..., op["y_off"]:op["y_off"] + 48]).all()
        nan_x = np.isnan(op["x"]).sum(), np.isnan(op["y"]).sum()
        if mode in ("c2f", "c2f_x"):
            assert op["r1"][0] == 1 and np.array_equal(op["y"][..., G["ry"]:G["ry"] + 48], rs[0])
            assert nan_x[1] == op["y"].size - rs[0].size
        elif mode == "r_in_x":
            assert op["r1"][0] == 2 and np.array_equal(op["x"][..., G["rx"]:G["rx"] + 48], rs[0])
            assert nan_x[0] == op["x"].size - 2 * x.size
        elif mode == "both":
            assert op["r1"][0] == 0 and np.array_equal(op["r1"][1][..., op["r1"][2]:op["r1"][2] + 48], rs[0])
        else:
            assert op["r1"] is None and S.n_res(mode) == 0


def test_force_strings_name_instances_that_exist(monkeypatch):
    """A force string that fits no instance falls back to conv_choose's own pick silently.  The fused arg-max entry reports the tile of the configuration
    conv_choose returns (no GPU involved): every EAGLE_CONV_FORCE string of the case lists must give the tile of the form it names."""
    from eagle_amd import lib
    tile16 = {0: (8, 32), 2: (8, 32), 3: (4, 32), 4: (2, 32)}                    # generic forms at wo > 16: 4 pw / 2 rows x 32 columns
    tile_s = {0: (8, 32), 3: (4, 32), 18: (8, 48), 8: (4, 32), 9: (8, 32), 10: (4, 32), 11: (8, 32), 12: (8, 32), 13: (16, 32), 19: (16, 32), 14: (4, 32),
              15: (4, 32), 21: (4, 32), 22: (8, 32), 23: (2, 64), 24: (4, 64)}
    for fmt, forces in (("f16", S.FORCE_F16), ("f32s", S.FORCE_SPLIT)):
        for f in forces:
            monkeypatch.setenv("EAGLE_CONV_FORCE", f)
            got = lib.conv2d_argmax_tiles((5, 70), 48, 48, 3, 1, lib.PRECISIONS[fmt])[1:]
            assert got == (tile16 if fmt == "f16" else tile_s)[int(f.split(",")[2])], (fmt, f, got)
    for fmt, f, st, cin, cout in S.AD_FORMS:             # the entry takes cout <= 64; the fp16 family takes an A-direct force only with a plain epilogue, which it has not
        if fmt == "f32s" and cout <= 64:
            monkeypatch.setenv("EAGLE_CONV_FORCE", f)
            assert lib.conv2d_argmax_tiles(S.AD_MAP[1:], cin, cout, 3, st, lib.PREC_F32S)[1:] == tile_s[int(f.split(",")[2])], f
