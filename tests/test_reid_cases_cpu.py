"""The references of tests/reid_cases.py are themselves checked (no GPU):
(1) each float64 reference, on its production-shaped case, agrees with the float32 routine of oracle/reid.py that the end-to-end test trusts, within the
    same derived bound gamma_k * S the GPU tests use (exact operators: exactly);
(2) the checks are not vacuous: a dropped border tap (conv7, dw3) violates the bound in every case, a gate that divides by HW + 1 violates it in every
    case but the one with 1024 adds per lane, where the bit-exact expectation rejects it (test_a_wrong_divisor_violates_the_gate_checks), so the GPU
    tests fail on these mistakes without a kernel ever being made to fail on purpose;
(3) the float32 kernel-order restatements (the bit-exact expectations of the GPU tests) lie within the bounds of the float64 references;
(4) the float64 references chained per eagle_amd/osnet.py's table reproduce oracle.reid.embed within the end-to-end tolerance of test_gpu_reid.py."""
import itertools

import numpy as np

import reid_cases as R
from oracle import reid

SQRT_VAR = np.float32(1.0 - 1e-5)          # running_var for which the oracle's float32 BatchNorm scale is exactly 1


def _identity_bn(sd, name, c, bias=None):
    sd["reid." + name + ".weight"] = np.ones(c, np.float32)
    sd["reid." + name + ".bias"] = np.zeros(c, np.float32) if bias is None else bias
    sd["reid." + name + ".running_mean"] = np.zeros(c, np.float32)
    sd["reid." + name + ".running_var"] = np.full(c, SQRT_VAR)
    assert np.array_equal(reid._bn(sd, name, np.ones((1, c), np.float32)), np.ones((1, c), np.float32) + sd["reid." + name + ".bias"])


def _within(got, ref, bound, what):
    ratio = float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, np.finfo(np.float64).tiny)).max())
    print(f"{what}: max |got - ref| / bound = {ratio:.3f}")
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (what, ratio)


def test_conv7_reference_against_the_oracle_routine():
    x, w, b = R.conv7_case(3, 256, 128)
    ref, bound = R.conv7_ref(x, w, np.zeros(16, np.float32))
    got = np.maximum(reid._conv7_s2(np.ascontiguousarray(x[..., :3]), np.ascontiguousarray(w.transpose(3, 2, 0, 1))), np.float32(0))
    assert got.shape == ref.shape == (3, 128, 64, 16) and (ref > 0).any() and (ref == 0).any()
    _within(got, ref, bound, "conv7 vs oracle.reid._conv7_s2")


def test_pool_references_against_the_oracle_routines():
    x = R.pool_case(3, 64, 32, 16)
    assert np.array_equal(R.maxpool3s2_ref(x), reid._maxpool3_s2(x))
    assert (R.maxpool3s2_ref(x)[..., 1] < 0).all()                     # the strictly negative channel: zero padding would have won at the border
    n, h, w, c = x.shape
    mean = x.reshape(n, h // 2, 2, w // 2, 2, c).mean((2, 4), dtype=np.float64)
    assert np.abs(R.avgpool2_ref(x) - mean).max() <= R.gamma(3) * np.abs(x).max()
    odd = R.pool_case(1, 5, 7, 16)
    poisoned = odd.copy(); poisoned[:, 4] = np.nan; poisoned[:, :, 6] = np.nan
    assert R.avgpool2_ref(odd).shape == (1, 2, 3, 16) and np.array_equal(R.avgpool2_ref(odd), R.avgpool2_ref(poisoned))


def test_dw3_reference_against_the_oracle_routine():
    """oracle.reid._light with an identity 1 x 1 convolution and an identity BatchNorm is its depthwise loop + bias + ReLU"""
    x, w, b = R.dw3_case(3, 64, 32, 16)
    sd = {"reid.l.conv1.weight": np.eye(16, dtype=np.float32).reshape(16, 16, 1, 1), "reid.l.conv2.weight": np.ascontiguousarray(w.T).reshape(16, 1, 3, 3)}
    _identity_bn(sd, "l.bn", 16, b)
    ref, bound = R.dw3_ref(x, w, b)
    _within(reid._light(sd, "l", x), ref, bound, "dw3 vs oracle.reid._light")


def test_gate_reference_against_the_oracle_routine():
    """a pixel of ones makes oracle.reid._gate (which returns x * g) hand out g itself"""
    streams, w1, b1, w2, b2 = R.gate_case(3, 64, 32, 16, 16, 1)
    for s in streams:
        s[:, 0, 0, :] = 1.0
    sd = {"reid.g.fc1.weight": w1.reshape(1, 16, 1, 1), "reid.g.fc1.bias": b1, "reid.g.fc2.weight": w2.reshape(16, 1, 1, 1), "reid.g.fc2.bias": b2}
    _, et, g = R.gate_ref(streams, w1, b1, w2, b2)
    got = np.stack([reid._gate(sd, "g", s)[:, 0, 0, :] for s in streams], 1)
    _within(got, g, R.gate_g_bound(et, g), "gate vs oracle.reid._gate")
    assert np.abs(g[:, 0] - g[:, 3]).max() > 1e-3                      # the four streams are distinct


def test_head_reference_against_the_oracle_lines():
    """the head lines of oracle.reid.embed (mean, Linear, BatchNorm1d, ReLU) with an identity BatchNorm1d: the fold is then exact"""
    x, w, b = R.head_case(3, 16, 8, 128, 512)
    sd = {}
    _identity_bn(sd, "fc.1", 512)
    v = x.mean((1, 2), dtype=np.float32)
    v = (v @ w.T + b).astype(np.float32)
    got = np.maximum(reid._bn(sd, "fc.1", v), np.float32(0))
    ref, bound = R.head_ref(x, w, b)
    assert (ref > 0).any() and (ref == 0).any()
    _within(got, ref, bound, "head vs the head lines of oracle.reid.embed")


def test_a_dropped_border_tap_violates_the_conv7_and_dw3_bounds():
    for (h, w), n, ones in itertools.product(R.CONV7_SIZES, R.NS, (False, True)):
        if (h, w) == (256, 128) and (ones or n == 3):
            continue                                        # (the production size once: the perturbation is the same statement at every n)
        x, wt, b = R.conv7_case(n, h, w, ones)
        ref, bound = R.conv7_ref(x, wt, b)
        bad, _ = R.conv7_ref(x, wt, b, skip_last_col=True)
        assert (np.abs(bad - ref) > bound).any(), ("conv7", h, w, n, ones)
    for (h, w), c, n, ones in itertools.product(R.MAPS, R.CHANNELS, R.NS, (False, True)):
        x, wt, b = R.dw3_case(n, h, w, c, ones)
        ref, bound = R.dw3_ref(x, wt, b)
        bad, _ = R.dw3_ref(x, wt, b, skip_last_col=True)
        assert (np.abs(bad - ref) > bound).any(), ("dw3", h, w, c, n, ones)


def test_a_wrong_divisor_violates_the_gate_checks():
    """HW -> HW + 1 must fail what the GPU test asserts of g in every case.  The derived bound alone rejects it in 38 of the 40 cases; at C = 128 on
    the 64 x 32 map each lane adds 1024 pixels (k1 = 1025, a map size the network never gates at this width), the worst-case bound is 1 % wider than
    the mistake's effect there, and the bit-exact kernel-order expectation (which the GPU test asserts in every case) is what rejects it."""
    loose = []
    for (c, c_real, r), (h, w), n in itertools.product(R.GATE_CFGS, R.GATE_MAPS, R.NS):
        streams, w1, b1, w2, b2 = R.gate_case(n, h, w, c, c_real, r)
        _, et, g = R.gate_ref(streams, w1, b1, w2, b2)
        _, _, bad = R.gate_ref(streams, w1, b1, w2, b2, divisor_plus=1)
        assert (g[..., c_real:] == 0).all() and (g[..., :c_real] > 0).all()
        if not (np.abs(bad - g) > R.gate_g_bound(et, g)).any():
            loose.append((c, h, w))
        assert not np.array_equal(R.gate_g_f32(streams, w1, b1, w2, b2, divisor_plus=1), R.gate_g_f32(streams, w1, b1, w2, b2)), (c, c_real, r, h, w, n)
    assert all(R.k_mean(h * w, c) > 1000 for c, h, w in loose), loose


def test_all_ones_cases_are_their_tap_counts():
    for h, w in R.CONV7_SIZES[:4]:
        x, wt, b = R.conv7_case(1, h, w, ones=True)
        assert np.array_equal(R.conv7_ref(x, wt, b)[0][0, :, :, 5], 3.0 * R.tap_counts(h, w, 7, 2, 3))
    for h, w in R.MAPS:
        x, wt, b = R.dw3_case(1, h, w, 16, ones=True)
        assert np.array_equal(R.dw3_ref(x, wt, b)[0][0, :, :, 7], R.tap_counts(h, w, 3, 1, 1))
    assert R.tap_counts(5, 7, 3, 1, 1).min() == 4 and R.tap_counts(5, 7, 3, 1, 1).max() == 9 and R.tap_counts(1, 1, 7, 2, 3).tolist() == [[1]]


def test_kernel_order_restatements_lie_within_the_bounds():
    x, w, b = R.conv7_case(1, 9, 6)
    _within(R.conv7_f32(x, w, b), *R.conv7_ref(x, w, b), "conv7_f32")
    x, w, b = R.dw3_case(3, 5, 7, 32)
    _within(R.dw3_f32(x, w, b), *R.dw3_ref(x, w, b), "dw3_f32")
    assert (R.dw3_f32(x, w, b)[..., 24:] == 0).all()
    for cfg, hw in (((32, 24, 1), (1, 5)), ((128, 100, 8), (16, 8)), ((16, 16, 1), (64, 32))):
        streams, w1, b1, w2, b2 = R.gate_case(3, *hw, *cfg)
        _, et, g = R.gate_ref(streams, w1, b1, w2, b2)
        _within(R.gate_g_f32(streams, w1, b1, w2, b2), g, R.gate_g_bound(et, g), f"gate_g_f32 {cfg} {hw}")
    x, w, b = R.head_case(3, 3, 5, 16, 300)
    _within(R.head_f32(x, w, b), *R.head_ref(x, w, b), "head_f32")


def test_crop_cases_cover_what_they_name():
    for (fh, fw), (oh, ow) in itertools.product(((720, 1280), (97, 61)), ((256, 128), (8, 4))):
        ok, bad = R.crop_cases(fh, fw, oh, ow)
        for name, (f, x1, y1, x2, y2) in ok:
            assert 0 <= f < 2 and 0 <= x1 < x2 <= fw and 0 <= y1 < y2 <= fh, name
        assert any(x2 == fw for _, (_, _, _, x2, _) in ok) and any(y2 == fh for _, (_, _, _, _, y2) in ok)
        assert any(x2 - x1 == 1 for _, (_, x1, _, x2, _) in ok) and any(y2 - y1 == 1 for _, (_, _, y1, _, y2) in ok)
        assert len(bad) == 6 and all(not (0 <= f < 2 and 0 <= x1 < x2 <= fw and 0 <= y1 < y2 <= fh) for _, (f, x1, y1, x2, y2) in bad)
    assert any(n == "exact 2x of the output" for n, _ in R.crop_cases(720, 1280, 256, 128)[0]) and any(n == "exact 2x of the output" for n, _ in R.crop_cases(97, 61, 8, 4)[0])
    f = R.frames(97, 61)
    assert np.array_equal(R.crop_f32(f[0], (3, 5, 40, 90), 256, 128), reid.prepare_crop(f[0], (3, 5, 40, 90)))


def test_composed_references_reproduce_the_oracle_embedding():
    from eagle_amd import osnet, synth
    sd = osnet.make_osnet_state_dict(0)
    frame = synth.frame(0, 3)
    crops = np.stack([reid.prepare_crop(frame, r) for r in ((100, 50, 356, 562), (600, 300, 640, 420))])
    ref = reid.embed(sd, crops)
    got = R.embed64(sd, crops)
    scale = np.abs(ref).max()
    assert got.shape == ref.shape == (2, 512) and scale > 0
    assert np.abs(got - ref).max() <= 2e-4 * scale, np.abs(got - ref).max() / scale
