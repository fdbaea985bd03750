"""Cases, data and the "which form ran" proof for the forced convolution tests (no GPU; tests/test_conv_forms_cpu.py checks the lists against the library's
own tables, tests/test_gpu_conv_forms.py and the forced tests of test_gpu_ops.py / test_gpu_conv_linear.py / test_gpu_slices.py / test_gpu_flow.py run them).

EAGLE_CONV_FORCE = "kc,nt,variant" (fp16 and split families) and EAGLE_F32_FORCE = "nt,wx,variant" (exact family) apply only where the named instance exists,
fits 160 KiB of LDS and suits the epilogue; otherwise conv_choose falls through to its own pick WITHOUT a word, and a forced test then checks the default form.
run_forced therefore asks lib.conv_config (host only) which configuration the call is going to run and asserts it is the one the string names.

exact_case builds operands whose every product and partial sum is exactly representable: the result is the same number in whatever order a kernel
accumulates it, in binary16, split and fp32 storage, so the reference is a float64 matrix product and every comparison is array_equal."""
import functools
import itertools

import numpy as np

FAMILIES = ("f16", "f32", "f32s")
SILU = 2
LDS_LIMIT = 160 * 1024


def _prec(fmt):
    from eagle_amd import lib
    return lib.PRECISIONS[fmt]


def out_size(h, w, ks, stride):
    return (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1


def in_size(ho, wo, ks, stride):
    """the input map that gives a ho x wo output: the same size at stride 1, the ODD size 2 o - 1 at stride 2"""
    assert stride == 1 or (stride == 2 and ks == 3)
    return (ho, wo) if stride == 1 else (2 * ho - 1, 2 * wo - 1)


# ---- which form runs ---------------------------------------------------------------------------------------------------------------------------------
def set_force(monkeypatch, fmt, force, stack=None, m32=None):
    """the developer switches for one call: EAGLE_F32_FORCE in the exact family, EAGLE_CONV_FORCE in the other two; None removes a switch"""
    name, other = ("EAGLE_F32_FORCE", "EAGLE_CONV_FORCE") if fmt == "f32" else ("EAGLE_CONV_FORCE", "EAGLE_F32_FORCE")
    monkeypatch.delenv(other, raising=False)
    for k, v in ((name, force), ("EAGLE_F32_STACK", stack), ("EAGLE_CONV_M32", m32)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def named(fmt, force):
    """the configuration fields a force string pins down"""
    a, b, c = (int(v) for v in force.split(","))
    return dict(nt=a, wx=b, variant=c) if fmt == "f32" else dict(kc=a, nt=b, variant=c)


def assert_form(monkeypatch, fmt, force, ks, stride, cin, cout, wo, plain, second, expect="named"):
    """With the switches of set_force in the environment: the configuration conv_choose gives this layer is the one `force` names (expect = "named"), or,
    for a string that is MEANT not to apply (expect = "default"), the unforced pick.  -> the configuration (lib.conv_config's dict)."""
    from eagle_amd import lib
    cfg = lib.conv_config(_prec(fmt), ks, stride, cin, cout, wo, plain, second)
    assert cfg["supported"] == 1 and 0 < cfg["lds_bytes"] <= LDS_LIMIT, f"{fmt} {ks}x{ks}/{stride} {cin}->{cout} @{wo}: no runnable configuration: {cfg}"
    if expect == "named":
        want = named(fmt, force)
        got = {k: cfg[k] for k in want}
        assert got == want, (f"{fmt} force {force!r} does not apply to {ks}x{ks}/{stride} {cin}->{cout} @{wo} (plain {plain}, two residuals {second}): "
                             f"conv_choose falls back to {cfg}")
    else:
        assert expect == "default"
        name = "EAGLE_F32_FORCE" if fmt == "f32" else "EAGLE_CONV_FORCE"
        with monkeypatch.context() as m:
            m.delenv(name, raising=False)
            own = lib.conv_config(_prec(fmt), ks, stride, cin, cout, wo, plain, second)
        assert cfg == own, f"{fmt} force {force!r} was expected to fall through on {ks}x{ks}/{stride} {cin}->{cout} @{wo}, but gives {cfg} instead of {own}"
    return cfg


def run_forced(monkeypatch, fmt, force, x, wt, b, stride, pre, r1, r2, post, stack=None, expect="named"):
    """lib.op_conv2d under the force switch, after the proof that the named form is what runs"""
    from eagle_amd import lib
    set_force(monkeypatch, fmt, force, stack)
    ks, cin, cout = wt.shape[0], wt.shape[2], wt.shape[3]
    wo = out_size(x.shape[1], x.shape[2], ks, stride)[1]
    if force is not None:
        assert_form(monkeypatch, fmt, force, ks, stride, cin, cout, wo, pre == 0 and post <= 1, r1 is not None and r2 is not None, expect)
    return lib.op_conv2d(x, wt, b, stride, pre, r1, r2, post, _prec(fmt))


# ---- exactly representable data ----------------------------------------------------------------------------------------------------------------------
def conv_ref64(x, wt, b, stride, r1=None, r2=None, relu=False):
    """float64 im2col x matmul: y = [relu](conv(x, wt) + b + r1 + r2), padding ks // 2"""
    n, h, w, cin = x.shape
    ks, _, _, cout = wt.shape
    p = ks // 2
    ho, wo = out_size(h, w, ks, stride)
    xp = np.zeros((n, h + 2 * p, w + 2 * p, cin))
    xp[:, p:p + h, p:p + w] = x
    cols = np.concatenate([xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] for ky in range(ks) for kx in range(ks)], axis=-1)
    y = cols.reshape(n * ho * wo, ks * ks * cin) @ wt.astype(np.float64).reshape(ks * ks * cin, cout) + b.astype(np.float64)
    y = y.reshape(n, ho, wo, cout)
    for r in (r1, r2):
        if r is not None:
            y = y + r
    return np.maximum(y, 0.0) if relu else y


@functools.lru_cache(maxsize=64)
def exact_case(ks, stride, cin, cout, n, ho, wo, nres, seed, relu=True):
    """-> (x, wt, b, r1, r2, post, ref), read-only and shared.  x: integers in [-2, 2]; weights from {-0.5, 0, 0, 0.5}; bias: multiples of 0.5 in [-2, 2]; residuals:
    integers in [-3, 3].  Every product is a multiple of 0.5 and every partial sum a multiple of 0.5 below 2^12: exact in fp32 in any order, and the operands
    are exact in binary16 and as split pairs.  The reference must survive binary16 unchanged, or the case is not what it claims."""
    rng = np.random.default_rng([seed, ks, stride, cin, cout, n, ho, wo, nres])
    h, w = in_size(ho, wo, ks, stride)
    x = rng.integers(-2, 3, (n, h, w, cin)).astype(np.float32)
    wt = rng.choice(np.array([-0.5, 0.0, 0.0, 0.5], np.float32), (ks, ks, cin, cout))
    b = (rng.integers(-4, 5, cout) * 0.5).astype(np.float32)
    rs = [rng.integers(-3, 4, (n, ho, wo, cout)).astype(np.float32) for _ in range(nres)] + [None, None]
    ref = conv_ref64(x, wt, b, stride, rs[0], rs[1], relu)
    assert ref.shape == (n, ho, wo, cout)
    assert np.array_equal(ref.astype(np.float16).astype(np.float64), ref), "the reference is not exact in binary16"
    assert np.abs(conv_ref64(np.abs(x), np.abs(wt), np.abs(b), stride)).max() < 4096, "a partial sum could leave the exact range"
    assert not relu or (0.2 < (ref > 0).mean() < 0.8), "ReLU leaves too few or too many outputs"
    ref = ref.astype(np.float32)
    for a in (x, wt, b, rs[0], rs[1], ref):
        if a is not None:
            a.setflags(write=False)
    return x, wt, b, rs[0], rs[1], 1 if relu else 0, ref


# ---- the forced tests' parameter lists (test_gpu_ops.py) ---------------------------------------------------------------------------------------------
# exact family: EAGLE_F32_FORCE "nt,wx,variant" x EAGLE_F32_STACK x layers ((n, h, w), ks, stride, cin, cout); one residual, ReLU
F32_TILINGS = ["3,2,0", "3,1,0", "6,2,3", "3,1,3", "2,2,4", "1,1,4"]
F32_STACKS = ["1", "0"]
F32_LAYERS = [((5, 17, 30), 3, 1, 48, 96), ((4, 7, 45), 3, 1, 32, 48), ((3, 34, 61), 3, 2, 48, 96), ((6, 12, 20), 1, 1, 64, 96),
              ((7, 1, 1), 3, 1, 16, 48), ((2, 33, 37), 3, 2, 3, 48), ((50, 17, 30), 3, 1, 32, 48)]


def f32_tiling_cases():
    """F32_TILINGS x F32_LAYERS x F32_STACKS -> [(id, shape, ks, stride, cin, cout, force, stack)].  Two kinds of pairs name no instance and used to run the
    default tiling instead: a Cout block that does not divide the layer's Cout (nt = 6 or 2 on 48 channels: the same variant and arrangement at nt = 3 runs),
    and a quarter tile (variant 4) on the 3-channel stem layer, whose chunk of 4 has full and half tiles only (the layer then has 16 input channels)."""
    out = []
    for k, (shape, ks, st, cin, cout) in enumerate(F32_LAYERS):
        for force in F32_TILINGS:
            nt, wx, v = (int(t) for t in force.split(","))
            if cout % (16 * nt):
                nt = 3
            c_in = 16 if (cin < 16 and v == 4) else cin
            for stack in F32_STACKS:
                f = f"{nt},{wx},{v}"
                out.append((f"shape{k}-{ks}-{st}-{c_in}-{cout}-{f}-{stack}", shape, ks, st, c_in, cout, f, stack))
    return out


# weight-stationary fp16 forms: (force, cin, cout) x maps; 3x3 stride 1, one residual, ReLU
# ("96,3,6", 96, 96) stood here: that instance needs 182352 bytes of LDS at wx = 2 and 179024 at wx = 1 (UNREACHABLE below), so the string never applied and
# the A-direct default ran; the 64-channel instance of the same variant is what the tuned table selects (64 -> 64 @240)
WS_FORMS = [("48,3,6", 48, 48), ("48,3,7", 48, 48), ("96,3,7", 96, 96), ("64,4,6", 64, 64), ("64,4,7", 64, 64), ("96,2,7", 96, 32)]
WS_MAPS = [(3, 37, 45), (2, 5, 70), (1, 16, 16)]
# split family, generic kernel: force x (cin, cout, ks, stride) on two frames of 19 x 45; two residuals, ReLU
SPLIT_FORCES = ["16,1,0", "16,2,0", "16,3,0", "16,4,0", "32,3,0", "32,4,0", "16,6,3", "32,6,3", "16,4,3", "32,2,3"]
SPLIT_LAYERS = [(96, 96, 3, 1), (64, 192, 3, 2), (192, 96, 1, 1)]
SPLIT_MAP = (2, 19, 45)
# pairs of the product that name no runnable instance, and what runs in their place: the split family's 3x3 stride-2 full tiles exist at kc = 8 and 16 only, and
# its half tile at kc = 32, nt = 6 needs more than 160 KiB (UNREACHABLE below); kc = 8 is the chunk the tuned table gives most stride-2 layers
SPLIT_REPLACED = {("32,3,0", (64, 192, 3, 2)): "8,3,0", ("32,4,0", (64, 192, 3, 2)): "8,4,0", ("32,6,3", (64, 192, 3, 2)): "8,6,3"}


def split_variant_cases():
    """SPLIT_FORCES x SPLIT_LAYERS -> [(id, cin, cout, ks, stride, force)]"""
    out = []
    for force in SPLIT_FORCES:
        for layer in SPLIT_LAYERS:
            f = SPLIT_REPLACED.get((force, layer), force)
            out.append(("-".join(map(str, layer)) + "-" + f, *layer, f))
    return out
# split family, A-direct forms forced by id: (cin, cout) x maps x (residuals, post)
M32_LAYERS = [(96, 96), (192, 192), (48, 192), (384, 384), (64, 96), (16, 192), (32, 288), (144, 96)]
M32_MAPS = [(3, 37, 45), (2, 5, 70), (1, 16, 16), (5, 17, 30), (1, 68, 120), (1, 1, 1), (2, 9, 33), (2, 34, 60), (1, 7, 65)]
M32_TILES = ["rows", "wide64"]
RES_POST_4 = [(True, 1), (False, 1), (False, 0), (2, 1)]
RES_POST_3 = [(True, 1), (False, 0), (2, 1)]
K48_MAPS = [(3, 37, 45), (1, 16, 16), (2, 135, 240)]
K48_FORMS = ["12", "13", "19"]
S2D_LAYERS = [(48, 96), (96, 192), (256, 96), (192, 384), (48, 192), (96, 96), (32, 96)]
S2D_MAPS = [(3, 37, 45), (2, 5, 70), (1, 16, 16), (2, 135, 240), (1, 1, 1)]
S2T_LAYERS = [(96, 192), (48, 192), (192, 384), (48, 384), (144, 192), (48, 96), (96, 96), (48, 288)]
S2T_MAPS = [(3, 37, 45), (2, 5, 70), (1, 16, 16), (2, 68, 120), (1, 1, 1), (2, 130, 129), (1, 9, 200)]
T48_MAPS = [(3, 37, 45), (1, 16, 16), (2, 135, 240), (2, 9, 100), (1, 8, 48), (1, 1, 1)]
FLOW_FORCE = "16,1,0"          # test_gpu_flow.py: the co-running handle's networks on the plain register-staged fp16 kernel wherever it is valid


def m32_force(cout, tile):
    v = (21 if cout % 192 == 0 else 22) + (2 if tile == "wide64" else 0)
    return f"16,{12 if cout % 192 == 0 else 6},{v}"


def s2d_force(cout):
    return "16,12,10" if cout % 192 == 0 else "16,6,11"


def s2t_force(cout):
    return "16,12,14" if cout % 192 == 0 else "16,6,15"


# ---- test_gpu_conv_linear.py --------------------------------------------------------------------------------------------------------------------------
V21 = "16,12,21"
LIN = {30: "16,12,27", 60: "16,12,27"}      # 60 columns: no linear form, the switch falls through
LIN_SHAPES = [(2, 17, 30, 32, 192), (3, 5, 30, 16, 384), (1, 1, 30, 16, 192), (2, 9, 30, 48, 192), (2, 34, 60, 32, 192), (1, 3, 60, 16, 192), (2, 7, 60, 48, 384)]
LIN_BIG = [(70, 17, 30, 16, 192)]
LIN_OTHER_WIDTHS = [(2, 9, 45, 16, 192), (2, 9, 60, 16, 192), (2, 9, 31, 16, 384), (2, 9, 29, 16, 192)]


def lin_expect(width):
    return "named" if width == 30 else "default"


# ---- every forced case as one flat list, for the CPU check ---------------------------------------------------------------------------------------------
def forced_cases():
    """(origin, fmt, force, ks, stride, cin, cout, wo, plain epilogue, two residuals, expect) of every forced call of the GPU tests"""
    import slice_cases as S
    out = []

    def add(origin, fmt, force, ks, st, cin, cout, hw, plain, second, expect="named"):
        out.append((origin, fmt, force, ks, st, cin, cout, out_size(hw[0], hw[1], ks, st)[1], plain, second, expect))

    for _, shape, ks, st, cin, cout, force, stack in f32_tiling_cases():
        add("ops.f32_tilings", "f32", force, ks, st, cin, cout, shape[1:], True, False)
    for (force, cin, cout), shape in itertools.product(WS_FORMS, WS_MAPS):
        add("ops.weight_stationary", "f16", force, 3, 1, cin, cout, shape[1:], True, False)
    for _, cin, cout, ks, st, force in split_variant_cases():
        if split_variant_fits(force, cin, cout, ks, st):
            add("ops.split_variants", "f32s", force, ks, st, cin, cout, SPLIT_MAP[1:], True, True)
    for (cin, cout), shape, (res, post), tile in itertools.product(M32_LAYERS, M32_MAPS, RES_POST_4, M32_TILES):
        add("ops.m32", "f32s", m32_force(cout, tile), 3, 1, cin, cout, shape[1:], True, res == 2)
    for shape, (res, post), form in itertools.product(K48_MAPS, RES_POST_3, K48_FORMS):
        add("ops.k_split_48", "f32s", f"16,3,{form}", 3, 1, 48, 48, shape[1:], True, res == 2)
    for (cin, cout), shape, (res, post) in itertools.product(S2D_LAYERS, S2D_MAPS, RES_POST_3):
        add("ops.split_stride2", "f32s", s2d_force(cout), 3, 2, cin, cout, shape[1:], True, res == 2)
    for (cin, cout), shape, (res, post) in itertools.product(S2T_LAYERS, S2T_MAPS, RES_POST_3):
        add("ops.split_true_stride2", "f32s", s2t_force(cout), 3, 2, cin, cout, shape[1:], True, res == 2)
    for shape, (res, post) in itertools.product(T48_MAPS, RES_POST_3):
        add("ops.split_8x48", "f32s", "16,3,18", 3, 1, 48, 48, shape[1:], True, res == 2)
    for (n, h, w, cin, cout), nres in itertools.product(LIN_SHAPES + LIN_BIG, (0, 1, 2)):
        add("linear.v21", "f32s", V21, 3, 1, cin, cout, (h, w), True, nres == 2)
        add("linear.lin", "f32s", LIN[w], 3, 1, cin, cout, (h, w), True, nres == 2, lin_expect(w))
    for n, h, w, cin, cout in LIN_OTHER_WIDTHS:
        add("linear.other_widths", "f32s", LIN[30], 3, 1, cin, cout, (h, w), True, False, "default")
    for shape in S.FORCE_MAPS:                             # SiLU before one residual: not a plain epilogue
        for fmt, forces in (("f32", S.FORCE_F32), ("f16", S.FORCE_F16), ("f32s", S.FORCE_SPLIT)):
            for force in forces:
                add("slices.tilings", fmt, force, 3, 1, 48, 48, shape[1:], False, False)
    for fmt, force, st, cin, cout in S.AD_FORMS:
        add("slices.ad_forms", fmt, force, 3, st, cin, cout, S.AD_MAP[1:], True, False)
    for ks, st, cin, cout, wo in ((3, 1, 16, 16, 160), (3, 2, 16, 32, 160), (1, 1, 64, 64, 80), (3, 1, 64, 64, 80)):      # yolov8n layers at 640 (SiLU)
        add("flow.co_runner", "f16", FLOW_FORCE, ks, st, cin, cout, (1, in_size(1, wo, ks, st)[1]), False, False)
    return out


def split_variant_fits(force, cin, cout, ks, stride):
    """test_conv_split_variants runs a (force, layer) pair only where the layer's channel counts fit the instance's chunk and Cout block and the instance class
    exists for the layer's kernel size (no kc = 8 for 1x1); test_conv_forms_cpu.py holds this rule against lib.conv_config"""
    kc, nt, _ = (int(v) for v in force.split(","))
    return not (cout % (16 * nt) or cin % kc or (ks == 1 and kc == 8))


# ---- the instance sweep (test_gpu_conv_forms.py) -------------------------------------------------------------------------------------------------------
# Output maps: the smallest with partial tiles in both directions at every tile the arrangement has.  wx = 2: tiles 8 / 4 / 2 x 32; wx = 1: 16 / 8 / 4 x 16;
# variant 18 of the split family: 8 x 48.
SWEEP_MAPS = {2: (9, 35), 1: (17, 13), 3: (9, 50)}
SWEEP_N = 2
WSTAT_VARIANTS = (6, 7)
# The (family, ks, stride, variant) classes of lib.conv_table("instances") and the (ks, stride) classes of the tuned tables, written out: the GPU tests are
# parametrised by them, and loading the library while pytest COLLECTS would put its HIP runtime into the process before the modules that import torch bring
# torch's own copy, leaving two runtimes side by side for the rest of the run.  test_conv_forms_cpu.py holds both lists against the tables.
SWEEP_GROUPS = ([("f16", 1, 1, v) for v in (0, 2, 3, 4)] + [("f16", 3, 1, v) for v in (0, 2, 3, 4, 6, 7)] + [("f16", 3, 2, v) for v in (0, 3, 4)] +
                [("f32", ks, st, v) for ks, st in ((1, 1), (3, 1), (3, 2)) for v in (0, 3, 4)] +
                [("f32s", 1, 1, 0), ("f32s", 1, 1, 3), ("f32s", 3, 1, 0), ("f32s", 3, 1, 3), ("f32s", 3, 1, 18), ("f32s", 3, 2, 0), ("f32s", 3, 2, 3)])
TUNED_TABLES = {"tuned_f16": "f16", "tuned_f32": "f32", "tuned_split": "f32s"}
TUNED_GROUPS = [(t, ks, st) for t in TUNED_TABLES for ks, st in ((1, 1), (3, 1), (3, 2))]


def sweep_layer(fmt, ks, stride, kc, nt, variant):
    """(cin, cout, residuals) of the sweep's layer for one instance: two chunks where the channel padding allows (cin = 3 for the stem instances, whose chunk
    is the whole padded input; cin = kc for the weight-stationary forms), two Cout blocks with the second one ragged"""
    ws = fmt == "f16" and variant in WSTAT_VARIANTS
    cin = 3 if kc < 16 else kc if ws else 2 * kc
    return cin, 32 * nt - 5, 1 if ws else 2


def sweep_force(fmt, kc, nt, wx, variant):
    return f"{nt},{wx},{variant}" if fmt == "f32" else f"{kc},{nt},{variant}"


def sweep_arrangements(fmt, variant):
    return (3,) if (fmt, variant) == ("f32s", 18) else (2, 1)


def sweep_cases(instances):
    """instances: lib.conv_table("instances") -> {(fmt, ks, stride, variant): [(kc, nt, wx, cin, cout, nres, ho, wo, force), ...]}"""
    fmt_of = {0: "f16", 1: "f32", 2: "f32s"}
    groups = {}
    for prec, ks, st, kc, nt, v in instances:
        fmt = fmt_of[prec]
        cin, cout, nres = sweep_layer(fmt, ks, st, kc, nt, v)
        for wx in sweep_arrangements(fmt, v):
            if (fmt, ks, st, kc, nt, v, wx) in UNREACHABLE:
                continue
            ho, wo = SWEEP_MAPS[wx]
            groups.setdefault((fmt, ks, st, v), []).append((kc, nt, wx, cin, cout, nres, ho, wo, sweep_force(fmt, kc, nt, wx, v)))
    return groups


SUB_TILES = {"f16": {0: 4, 2: 4, 3: 2, 4: 1, 6: 4, 7: 2}, "f32": {0: 4, 3: 2, 4: 1}, "f32s": {0: 4, 3: 2, 18: 6}}      # 16-pixel sub-tiles per wave (conv.hip g_forms)


def tile_of(fmt, variant, wx):
    pw = SUB_TILES[fmt][variant]
    return 4 * pw // wx, 16 * wx


def lds_bytes(fmt, ks, stride, kc, nt, variant, wx):
    """conv.hip lds_bytes for the generic and weight-stationary forms, restated: lib.conv_config reports the figure only for the configuration it returns, and
    the point of UNREACHABLE is the instances it never returns.  test_conv_forms_cpu.py holds this against conv_config for every instance that can run."""
    th, tw = tile_of(fmt, variant, wx)
    pw, bn = SUB_TILES[fmt][variant], 16 * nt
    halo = ((th - 1) * stride + ks) * ((tw - 1) * stride + ks)
    ps = lambda c: c * 2 + (16 if (c // 8) % 2 == 0 else 0)          # bytes per staged pixel, padded against bank conflicts
    ni = (ks * ks * (kc // 8) + 3) // 4                                # K-steps per chunk
    if fmt == "f16":
        operands, strips = ni * 4 * bn * 16 + halo * ps(kc), 4 * pw * 16 * (bn * 2 + 16)
        return operands + strips + 16 if variant in WSTAT_VARIANTS else max(operands + 16, strips)
    if fmt == "f32s":
        return max(ni * 2 * 4 * bn * 16 + halo * ps(2 * kc) + 16, 4 * pw * 16 * (bn * 4 + 16))
    return ks * ks * (kc // 4) * 4 * bn * 4 + halo * (kc + 1) * 4


# Instances that cannot be selected at a tile arrangement: lds_bytes is above 160 KiB = 163840 there.  (fmt, ks, stride, kc, nt, variant, wx): bytes
# (test_conv_forms_cpu.py recomputes them).  Every instance below is listed at BOTH arrangements: compiled, and never run by anything.
UNREACHABLE = {
    ("f16", 3, 1, 96, 3, 6, 2): 182352, ("f16", 3, 1, 96, 3, 6, 1): 179024,      # conv_f16_ws_kernel<96, 3, 4, 1>: the weight-stationary full tile at 96 channels
    ("f16", 3, 2, 48, 3, 0, 2): 166784, ("f16", 3, 2, 48, 3, 0, 1): 164992,      # fp16 3x3 stride 2, kc = 48, full tiles: the 17 x 65 / 33 x 33 halo at 112 bytes a pixel
    ("f16", 3, 2, 48, 4, 0, 2): 181120, ("f16", 3, 2, 48, 4, 0, 1): 179328,
    ("f16", 3, 2, 48, 6, 0, 2): 209792, ("f16", 3, 2, 48, 6, 0, 1): 208000,
    ("f32s", 3, 2, 32, 6, 3, 2): 194848, ("f32s", 3, 2, 32, 6, 3, 1): 191392,    # split 3x3 stride 2, kc = 32, nt = 6, half tiles
}

# Tuned rows that conv_choose never returns under the default switches, whatever the epilogue, and the rule that answers first.
# (table, (ks, stride, cin, cout, wo, kc, nt, wx, variant)): rule
SHADOWED = {
    ("tuned_split", (3, 1, 48, 48, 240, 16, 3, 1, 0)): "the row above it has the same key (8 x 48 tiles, variant 18) and is supported: rows of one shape are tried in order",
    ("tuned_split", (3, 1, 256, 48, 240, 32, 3, 1, 3)): "the row above it has the same key (8 x 48 tiles, variant 18) and is supported: rows of one shape are tried in order",
    ("tuned_split", (3, 1, 96, 96, 120, 16, 6, 2, 9)): "EAGLE_CONV_M32",
    ("tuned_split", (3, 1, 192, 192, 60, 16, 12, 2, 8)): "EAGLE_CONV_M32",
    ("tuned_split", (3, 1, 384, 384, 30, 16, 12, 2, 8)): "EAGLE_CONV_M32",
}
# "EAGLE_CONV_M32": with a plain epilogue the 32x32x16 A-direct rule before the table loop takes every 3x3 stride-1 layer with Cout = 96 k, and with any other
# epilogue the loop skips A-direct rows; the row is the answer only with EAGLE_CONV_M32=0 (what test_conv_split_a_direct runs)
