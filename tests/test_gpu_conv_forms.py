"""-m gpu: every compiled generic and weight-stationary convolution instance, and every row of the three tuned tables, run alone.

The instance sweep forces each instance at each tile arrangement through conv_form_cases.run_forced, which first proves (lib.conv_config, host only) that the
named instance is what runs, on the smallest maps that still have partial tiles in both directions, two chunks and two Cout blocks, the second one ragged.
The tuned rows run unforced at their own key, two tile rows high: the arrangements a force string cannot set (16-column tiles on wide maps, 32-column tiles on
narrow ones) are reached only this way.  Data are conv_form_cases.exact_case's: every partial sum is exactly representable, so the float64 reference is the
result in all three families whatever the summation order and every comparison is array_equal.  Exact data cannot see a lost bit of precision: one Gaussian
case per (family, variant) and the tuned rows that need the SiLU epilogue are held to the bounds of tests/test_gpu_ops.py against the oracle.

tests/test_conv_forms_cpu.py holds the lists these tests walk against the library's tables: no instance and no reachable row is left out."""
import functools

import numpy as np
import pytest

import conv_form_cases as F
from eagle_amd import lib
from test_gpu_ops import F16_TOL, F32S_TOL, _rand

pytestmark = pytest.mark.gpu

TUNED = F.TUNED_TABLES


@functools.lru_cache(maxsize=None)
def _groups():
    """the sweep's cases per (family, ks, stride, variant), from the library's instance table.  Read when a test runs, never while the module is imported:
    nothing may load the library during collection (conv_form_cases.SWEEP_GROUPS)"""
    groups = F.sweep_cases(lib.conv_table("instances"))
    assert sorted(groups) == sorted(F.SWEEP_GROUPS), "conv_form_cases.SWEEP_GROUPS is not the instance table's classes"
    return groups


@functools.lru_cache(maxsize=None)
def _tuned_rows(table):
    rows = [r for r in lib.conv_table(table) if (table, r) not in F.SHADOWED]
    assert {(table, r[0], r[1]) for r in rows} == {g for g in F.TUNED_GROUPS if g[0] == table}, "conv_form_cases.TUNED_GROUPS is not the table's classes"
    return rows


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in ("EAGLE_CONV_FORCE", "EAGLE_F32_FORCE", "EAGLE_F32_STACK", "EAGLE_CONV_M32"):
        monkeypatch.delenv(k, raising=False)


def _differs(got, ref):
    bad = np.argwhere(got != ref)
    return f"{len(bad)} of {ref.size} values, first (n, y, x, c) = {tuple(bad[0])}: {got[tuple(bad[0])]!r} for {ref[tuple(bad[0])]!r}"


@pytest.mark.parametrize("fmt,ks,stride,variant", sorted(F.SWEEP_GROUPS))
def test_every_instance_alone_on_exact_data(fmt, ks, stride, variant, monkeypatch):
    """Every (kc, nt) instance of this (family, kernel size, stride, variant) at each tile arrangement: two frames (row stacking of the exact family straddles
    them), a 9 x 35 map for 32-column tiles, 17 x 13 for 16-column tiles, 9 x 50 for the 8 x 48 tile, odd inputs at stride 2; two residuals and ReLU (one
    residual for the weight-stationary forms).  Bit for bit the float64 reference."""
    bad = []
    for kc, nt, wx, cin, cout, nres, ho, wo, force in _groups()[(fmt, ks, stride, variant)]:
        x, wt, b, r1, r2, post, ref = F.exact_case(ks, stride, cin, cout, F.SWEEP_N, ho, wo, nres, 1)
        got = F.run_forced(monkeypatch, fmt, force, x, wt, b, stride, 0, r1, r2, post)
        if not np.array_equal(got, ref):
            bad.append(f"{fmt} {force} (kc {kc}, nt {nt}, wx {wx}) {cin}->{cout} @{ho}x{wo}: {_differs(got, ref)}")
    assert not bad, "\n".join(bad)


def _gaussian(ks, stride, cin, cout, n, ho, wo, nres, seed):
    h, w = F.in_size(ho, wo, ks, stride)
    x = _rand((n, h, w, cin), seed)
    wt = _rand((ks, ks, cin, cout), seed + 1, (2.0 / (cin * ks * ks)) ** 0.5)
    b = _rand((cout,), seed + 2, 0.1)
    rs = [_rand((n, ho, wo, cout), seed + 3 + k) for k in range(nres)] + [None, None]
    return x, wt, b, rs[0], rs[1]


def _against_oracle(fmt, got, x, wt, b, stride, pre, r1, r2, post, what):
    """the bounds of test_conv_parity: bit-exact (f32), F16_TOL on binary16-rounded operands (f16), F32S_TOL against the fp32 oracle itself (f32s)"""
    from oracle import prims as P
    if fmt == "f16":
        q = P.round_f16
        ref = P.conv2d(q(x), q(wt), b, stride=stride, pre=pre, r1=None if r1 is None else q(r1), r2=None if r2 is None else q(r2), post=post, f16_out=True)
    else:
        ref = P.conv2d(x, wt, b, stride=stride, pre=pre, r1=r1, r2=r2, post=post)
    if fmt == "f32":
        assert np.array_equal(ref, got), f"{what}: fp32 conv not bit-exact: max|d|={np.abs(ref - got).max()}"
        return
    err = np.abs(ref - got).max() / max(np.abs(ref).max(), 1e-6)
    assert err < (F16_TOL if fmt == "f16" else F32S_TOL), f"{what}: {fmt} conv error {err}"


def _gaussian_pick(fmt, variant):
    """one instance per (family, variant): 3 x 3 stride 1 where the variant has it, the largest chunk, three Cout tiles (two for the form that has no three)"""
    keys = sorted(k for k in F.SWEEP_GROUPS if k[0] == fmt and k[3] == variant)
    key = next((k for k in keys if k[1:3] == (3, 1)), keys[0])
    rows = _groups()[key]
    kc = max(r[0] for r in rows)
    return key, next((r for r in rows if r[0] == kc and r[1] == 3), next(r for r in rows if r[0] == kc))


@pytest.mark.parametrize("fmt,variant", sorted({(k[0], k[3]) for k in F.SWEEP_GROUPS}))
def test_one_gaussian_case_per_family_and_variant(fmt, variant, monkeypatch):
    (_, ks, stride, _), (kc, nt, wx, cin, cout, nres, ho, wo, force) = _gaussian_pick(fmt, variant)
    x, wt, b, r1, r2 = _gaussian(ks, stride, cin, cout, F.SWEEP_N, ho, wo, nres, 300 + variant)
    got = F.run_forced(monkeypatch, fmt, force, x, wt, b, stride, 0, r1, r2, 1)
    _against_oracle(fmt, got, x, wt, b, stride, 0, r1, r2, 1, f"{fmt} {force}")


@pytest.mark.parametrize("table,ks,stride", F.TUNED_GROUPS)
def test_every_tuned_row_at_its_own_key(table, ks, stride, monkeypatch):
    """Every reachable row unforced at its own (ks, stride, cin, cout, wo), tile_h + 1 rows high (two tile rows, the second with one row), one frame (two in the
    exact family): conv_config must report exactly the row, and the result is the float64 reference bit for bit (plain epilogue, one residual, ReLU).  A row
    that answers only with another epilogue (the A-direct rules take the plain one) runs the detector's SiLU epilogue on Gaussian data against the oracle."""
    fmt = TUNED[table]
    bad = []
    for row in _tuned_rows(table):
        if row[:2] != (ks, stride):
            continue
        _, _, cin, cout, wo, kc, nt, wx, v = row
        plain = None
        for p in (True, False):
            cfg = lib.conv_config(lib.PRECISIONS[fmt], ks, stride, cin, cout, wo, p, False)
            if (cfg["kc"], cfg["nt"], cfg["wx"], cfg["variant"]) == (kc, nt, wx, v):
                plain = p
                break
        assert plain is not None and cfg["supported"] == 1, f"{table} {row}: not the answer for its own key: {cfg}"
        n, ho = (2 if fmt == "f32" else 1), cfg["tile_h"] + 1
        if plain:
            x, wt, b, r1, r2, post, ref = F.exact_case.__wrapped__(ks, stride, cin, cout, n, ho, wo, 1, 2)      # (each row once: not worth a cache slot)
            got = lib.op_conv2d(x, wt, b, stride, 0, r1, None, post, lib.PRECISIONS[fmt])
            if not np.array_equal(got, ref):
                bad.append(f"{table} {row}: {_differs(got, ref)}")
        else:
            assert fmt != "f32", "every tiling of the exact family takes every epilogue"
            x, wt, b, r1, _ = _gaussian(ks, stride, cin, cout, n, ho, wo, 1, 400)
            got = lib.op_conv2d(x, wt, b, stride, F.SILU, r1, None, 0, lib.PRECISIONS[fmt])
            _against_oracle(fmt, got, x, wt, b, stride, F.SILU, r1, None, 0, f"{table} {row}")
    assert not bad, "\n".join(bad)
