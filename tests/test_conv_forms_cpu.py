"""Which convolution form a call runs, settled without a GPU (needs the built library): every force string of the GPU tests resolves to the form it names,
every compiled instance is reached by the sweep of tests/test_gpu_conv_forms.py or is provably unreachable, and every row of the tuned tables is either what
conv_choose answers for its own key or listed with the rule that answers before it.  The host-only entries eagle_op_conv_config / eagle_op_conv_table share
eagle_op_conv2d's channel padding and conv_choose call, so what they report is what a GPU call runs."""
import itertools

import numpy as np
import pytest

import conv_form_cases as F
from eagle_amd import lib

FMT_OF = {lib.PREC_F16: "f16", lib.PREC_F32: "f32", lib.PREC_F32S: "f32s"}
EPILOGUES = [(True, False), (True, True), (False, False), (False, True)]       # (plain_epilogue, second_residual)
TUNED = {"tuned_f16": "f16", "tuned_f32": "f32", "tuned_split": "f32s"}


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in ("EAGLE_CONV_FORCE", "EAGLE_F32_FORCE", "EAGLE_F32_STACK", "EAGLE_CONV_M32"):
        monkeypatch.delenv(k, raising=False)


def test_tables_have_the_documented_shape():
    inst = lib.conv_table("instances")
    assert len(inst) == len(set(inst)) and {r[0] for r in inst} == set(FMT_OF)
    assert all(ks in (1, 3) and st in (1, 2) and nt in (1, 2, 3, 4, 6) for _, ks, st, _, nt, _ in inst)
    assert {(FMT_OF[p], v) for p, _, _, _, _, v in inst} == {(f, v) for f, d in F.SUB_TILES.items() for v in d}
    ad = lib.conv_table("adirect")
    assert len(ad) == len({r[:2] for r in ad}) and all(0 < r[7] <= F.LDS_LIMIT for r in ad)
    for t in TUNED:
        rows = lib.conv_table(t)
        assert len(rows) >= 98 and all(r[0] in (1, 3) for r in rows)


def test_the_parametrisation_lists_are_the_tables_classes_and_collection_loads_no_library():
    """The GPU tests are parametrised from lists written out in conv_form_cases, not from lib.conv_table: a module that loads the library while pytest collects
    brings the system's HIP runtime into the process before the modules that import torch bring torch's bundled copy, and with two runtimes in one process a
    later test that opens libamdhip64.so by name gets the other one (its hipMemcpy of a library pointer then fails).  Importing these modules must load nothing."""
    import os
    import subprocess
    import sys
    assert sorted(F.sweep_cases(lib.conv_table("instances"))) == sorted(F.SWEEP_GROUPS) and len(set(F.SWEEP_GROUPS)) == len(F.SWEEP_GROUPS)
    assert {(t, r[0], r[1]) for t in F.TUNED_TABLES for r in lib.conv_table(t)} == set(F.TUNED_GROUPS) and F.TUNED_TABLES == TUNED
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import conv_form_cases, test_conv_forms_cpu, test_gpu_conv_forms, test_gpu_ops, test_gpu_conv_linear, test_gpu_slices\n"
            "from eagle_amd import lib\n"
            "assert lib._lib is None, 'a test module loaded the library at import'\n"
            "assert not any('libeagle_hip' in l or 'amdhip64' in l for l in open('/proc/self/maps')), 'a HIP runtime is mapped after the imports'\n") % (here, os.path.dirname(here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_conv_config_is_the_default_pick_and_reads_the_switches(monkeypatch):
    own = lib.conv_config(lib.PREC_F16, 3, 1, 48, 48, 70, False, False)
    assert own["supported"] == 1 and (own["tile_h"], own["tile_w"]) == F.tile_of("f16", own["variant"], own["wx"])
    monkeypatch.setenv("EAGLE_CONV_FORCE", "16,3,2")
    got = lib.conv_config(lib.PREC_F16, 3, 1, 48, 48, 70, False, False)
    assert (got["kc"], got["nt"], got["wx"], got["variant"]) == (16, 3, 2, 2)
    assert lib.conv_config(lib.PREC_F16, 3, 1, 48, 48, 13, False, False)["wx"] == 1
    assert lib.conv_config(lib.PREC_F32, 3, 1, 48, 48, 70) == lib.conv_config(lib.PREC_F32, 3, 1, 48, 48, 70, True, True)     # EAGLE_CONV_FORCE is not the exact family's
    monkeypatch.setenv("EAGLE_F32_FORCE", "3,1,4")
    got = lib.conv_config(lib.PREC_F32, 3, 1, 48, 48, 70)
    assert (got["kc"], got["nt"], got["wx"], got["variant"], got["tile_h"], got["tile_w"]) == (16, 3, 1, 4, 4, 16)
    # the entry pads channels as eagle_op_conv2d does: 3 input channels are a chunk of 8 (4 in the exact family), 57 outputs four 16-blocks
    monkeypatch.delenv("EAGLE_F32_FORCE")
    assert lib.conv_config(lib.PREC_F32, 3, 2, 3, 57, 30)["kc"] == 4 and lib.conv_config(lib.PREC_F32S, 3, 2, 3, 57, 30)["kc"] == 8
    with pytest.raises(lib.EagleError):
        lib.conv_config(lib.PREC_F16, 5, 1, 48, 48, 70)
    with pytest.raises(KeyError):
        lib.conv_table("no such table")


def test_an_unsupported_force_string_is_caught_not_ignored(monkeypatch):
    """the hole this file closes: split "32,3,0" on a 3x3 stride-2 layer names no instance, conv_choose says nothing and runs its own pick"""
    F.set_force(monkeypatch, "f32s", "32,3,0")
    with pytest.raises(AssertionError, match="does not apply"):
        F.assert_form(monkeypatch, "f32s", "32,3,0", 3, 2, 64, 192, 23, True, True)
    F.set_force(monkeypatch, "f16", "96,3,6")
    with pytest.raises(AssertionError, match="does not apply"):
        F.assert_form(monkeypatch, "f16", "96,3,6", 3, 1, 96, 96, 45, True, False)
    F.set_force(monkeypatch, "f32s", F.V21)               # ... and a string that does apply is no fall-through (the unforced pick at 30 columns is variant 27)
    with pytest.raises(AssertionError, match="expected to fall through"):
        F.assert_form(monkeypatch, "f32s", F.V21, 3, 1, 16, 192, 30, True, False, "default")


# ---- 1. the forced tests' lists -------------------------------------------------------------------------------------------------------------------------
def test_every_force_string_of_the_gpu_tests_resolves_to_the_form_it_names(monkeypatch):
    cases = F.forced_cases()
    assert {c[0].split(".")[0] for c in cases} == {"ops", "linear", "slices", "flow"}
    seen = set()
    for origin, fmt, force, ks, st, cin, cout, wo, plain, second, expect in cases:
        key = (fmt, force, ks, st, cin, cout, wo, plain, second, expect)
        if key in seen:
            continue
        seen.add(key)
        F.set_force(monkeypatch, fmt, force)
        F.assert_form(monkeypatch, fmt, force, ks, st, cin, cout, wo, plain, second, expect)
    assert len(seen) > 300


def test_the_split_variant_skips_are_pairs_that_cannot_run(monkeypatch):
    """test_conv_split_variants skips a (force, layer) pair that "does not fit this instance": conv_config must agree, and every other pair must resolve"""
    wo = {1: F.SPLIT_MAP[2], 2: F.out_size(F.SPLIT_MAP[1], F.SPLIT_MAP[2], 3, 2)[1]}
    skipped = 0
    for _, cin, cout, ks, st, force in F.split_variant_cases():
        F.set_force(monkeypatch, "f32s", force)
        cfg = lib.conv_config(lib.PREC_F32S, ks, st, cin, cout, wo[st], True, True)
        is_named = {k: cfg[k] for k in ("kc", "nt", "variant")} == F.named("f32s", force)
        assert is_named == F.split_variant_fits(force, cin, cout, ks, st), (force, cin, cout, ks, st, cfg)
        skipped += not is_named
    assert skipped == 6


def test_every_a_direct_form_is_named_by_a_forced_case():
    named = {(fmt, int(force.split(",")[2])) for _, fmt, force, *_, expect in F.forced_cases() if fmt != "f32" and expect == "named"}
    for prec, variant, *_ in lib.conv_table("adirect"):
        assert (FMT_OF[prec], variant) in named, f"A-direct form {FMT_OF[prec]} variant {variant} is forced by no test"


# ---- 2. the instance sweep ------------------------------------------------------------------------------------------------------------------------------
def test_every_instance_is_swept_or_provably_unreachable(monkeypatch):
    inst = lib.conv_table("instances")
    groups = F.sweep_cases(inst)
    swept = {(fmt, ks, st, kc, nt, v, wx) for (fmt, ks, st, v), rows in groups.items() for kc, nt, wx, *_ in rows}
    over = {}
    for prec, ks, st, kc, nt, v in inst:
        fmt = FMT_OF[prec]
        for wx in F.sweep_arrangements(fmt, v):
            key = (fmt, ks, st, kc, nt, v, wx)
            need = F.lds_bytes(*key)
            if need > F.LDS_LIMIT:
                over[key] = need
            else:
                assert key in swept, f"{key} fits ({need} bytes) and is not in the sweep"
        assert any((fmt, ks, st, kc, nt, v, wx) in swept for wx in F.sweep_arrangements(fmt, v)) or \
            all((fmt, ks, st, kc, nt, v, wx) in F.UNREACHABLE for wx in F.sweep_arrangements(fmt, v))
    assert over == F.UNREACHABLE, f"UNREACHABLE is not what lds_bytes gives: {over}"
    # every swept case resolves to its instance at its arrangement, with the LDS footprint computed above
    for (fmt, ks, st, v), rows in groups.items():
        for kc, nt, wx, cin, cout, nres, ho, wo, force in rows:
            F.set_force(monkeypatch, fmt, force)
            cfg = F.assert_form(monkeypatch, fmt, force, ks, st, cin, cout, wo, True, nres == 2)
            assert (cfg["kc"], cfg["nt"], cfg["wx"], cfg["variant"]) == (kc, nt, wx, v), (fmt, force, cfg)
            assert (cfg["tile_h"], cfg["tile_w"]) == F.tile_of(fmt, v, wx) and cfg["lds_bytes"] == F.lds_bytes(fmt, ks, st, kc, nt, v, wx), (fmt, force, cfg)
            assert ho % cfg["tile_h"] and wo % cfg["tile_w"] and ho > cfg["tile_h"], "a partial tile in both directions, two tile rows"
            assert wo > cfg["tile_w"] or wx == 1, "two tile columns (a map wider than 16 columns is never tiled 16 wide by a force string)"
            cin_pad = 8 if cin <= 8 else (cin + 15) // 16 * 16
            assert (cin_pad // kc == 2 or cin == 3 or v in F.WSTAT_VARIANTS) and (cout + 15) // 16 * 16 == 2 * 16 * nt and cout % 16


def test_unreachable_instances_fall_back_silently(monkeypatch):
    """what the UNREACHABLE list means in practice: forcing one of them gives another form, at either arrangement"""
    for (fmt, ks, st, kc, nt, v, wx), need in F.UNREACHABLE.items():
        assert need > F.LDS_LIMIT
        cin, cout, nres = F.sweep_layer(fmt, ks, st, kc, nt, v)
        F.set_force(monkeypatch, fmt, F.sweep_force(fmt, kc, nt, wx, v))
        cfg = lib.conv_config(lib.PRECISIONS[fmt], ks, st, cin, cout, F.SWEEP_MAPS[wx][1], True, nres == 2)
        assert cfg["supported"] == 1 and (cfg["kc"], cfg["nt"], cfg["variant"]) != (kc, nt, v)


# ---- 3. the tuned tables ---------------------------------------------------------------------------------------------------------------------------------
def tuned_answers(table, row):
    """the (plain_epilogue, second_residual) combinations under which conv_choose answers a tuned row's own key with exactly that row"""
    ks, st, cin, cout, wo, kc, nt, wx, v = row
    hits = []
    for plain, second in EPILOGUES:
        cfg = lib.conv_config(lib.PRECISIONS[TUNED[table]], ks, st, cin, cout, wo, plain, second)
        assert cfg["supported"] == 1 and cfg["lds_bytes"] <= F.LDS_LIMIT, (table, row, cfg)
        if (cfg["kc"], cfg["nt"], cfg["wx"], cfg["variant"]) == (kc, nt, wx, v):
            hits.append((plain, second))
    return hits


@pytest.mark.parametrize("table", list(TUNED))
def test_every_tuned_row_is_the_answer_for_its_key_or_listed_as_shadowed(table, monkeypatch):
    rows = lib.conv_table(table)
    inst = set(lib.conv_table("instances"))
    ad = {(r[0], r[1]): r for r in lib.conv_table("adirect")}
    prec = lib.PRECISIONS[TUNED[table]]
    assert len(rows) == len(set(rows)), "a duplicated row"
    for row in rows:
        ks, st, cin, cout, wo, kc, nt, wx, v = row
        # the row names something that exists, divides the layer and fits: a row that does not is skipped by conv_choose without a word
        if (prec, v) in ad:
            assert ad[(prec, v)][2:5] == (st, kc, nt) and ks == 3, (table, row)
        else:
            assert (prec, ks, st, kc, nt, v) in inst, f"{table} {row} names an instance that is not compiled"
            assert F.lds_bytes(TUNED[table], ks, st, kc, nt, v, wx) <= F.LDS_LIMIT, (table, row)
            assert wx in F.sweep_arrangements(TUNED[table], v), (table, row)
        assert cin % kc == 0 and cout % (16 * nt) == 0, (table, row)
        hits = tuned_answers(table, row)
        if (table, row) in F.SHADOWED:
            assert not hits, f"{table} {row} is listed as shadowed but is the answer under {hits}"
            if F.SHADOWED[(table, row)] == "EAGLE_CONV_M32":
                monkeypatch.setenv("EAGLE_CONV_M32", "0")
                assert (True, False) in tuned_answers(table, row), (table, row)
                monkeypatch.delenv("EAGLE_CONV_M32")
            else:                                        # shadowed by an earlier row of the same key
                first = next(r for r in rows if r[:5] == row[:5])
                assert first != row and tuned_answers(table, first), (table, row, first)
        else:
            assert hits, f"{table} {row}: conv_choose never answers this row for its own key; list it in SHADOWED with the rule that precedes it"
    assert {t for t, _ in F.SHADOWED} <= set(TUNED) and all(r in lib.conv_table(t) for t, r in F.SHADOWED)


def test_tuned_tables_use_the_arrangement_a_force_string_cannot_set():
    """the reason the tuned rows are run on their own: conv_choose derives wx from wo > 16, many rows use the other arrangement"""
    other = {t: sum(1 for r in lib.conv_table(t) if r[8] != 18 and r[7] != (2 if r[4] > 16 else 1)) for t in ("tuned_f16", "tuned_split")}
    assert other["tuned_f16"] >= 40 and other["tuned_split"] >= 40, other


# ---- the data builder -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks,stride,cin,cout,n,ho,wo,nres", [(3, 1, 32, 27, 2, 9, 35, 2), (3, 2, 3, 59, 2, 17, 13, 2), (1, 1, 128, 187, 2, 9, 35, 2), (3, 1, 96, 91, 2, 17, 13, 1),
                                                             (3, 1, 256, 48, 1, 3, 20, 0), (3, 2, 512, 64, 1, 3, 7, 1)])
def test_exact_case_is_exact_and_is_a_convolution(ks, stride, cin, cout, n, ho, wo, nres):
    import torch
    import torch.nn.functional as TF
    x, wt, b, r1, r2, post, ref = F.exact_case(ks, stride, cin, cout, n, ho, wo, nres, 7)
    assert post == 1 and x.shape[1:3] == F.in_size(ho, wo, ks, stride) and (r1 is not None) == (nres >= 1) and (r2 is not None) == (nres == 2)
    assert set(np.unique(x)) <= {-2, -1, 0, 1, 2} and set(np.unique(wt)) == {-0.5, 0, 0.5} and np.array_equal(b * 2, np.round(b * 2)) and np.abs(b).max() <= 2
    assert ref.dtype == np.float32 and np.array_equal(ref.astype(np.float16).astype(np.float32), ref) and ref.min() == 0 and ref.max() > 4
    y = TF.conv2d(torch.from_numpy(x.transpose(0, 3, 1, 2).astype(np.float64)), torch.from_numpy(wt.transpose(3, 2, 0, 1).astype(np.float64)),
                  torch.from_numpy(b.astype(np.float64)), stride=stride, padding=ks // 2).numpy().transpose(0, 2, 3, 1)
    for r in (r1, r2):
        y = y if r is None else y + r
    assert np.array_equal(np.maximum(y, 0), ref)
    # the fp32 sum in a scrambled order gives the same bits: no rounding anywhere
    cols = x.reshape(-1)[:4096].astype(np.float32)
    assert np.float32(np.sum(cols[::-1] * np.float32(0.5), dtype=np.float32)) == np.float32(cols.astype(np.float64).sum() * 0.5)
    assert F.exact_case(ks, stride, cin, cout, n, ho, wo, nres, 7)[6] is ref and not ref.flags.writeable
