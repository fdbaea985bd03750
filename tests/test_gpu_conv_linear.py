"""-m gpu: the linear-tiling form of the 32x32x16 A-direct kernel (conv_ad_split32.inc, MAPW = 30: variant 27 of the split family), whose items own 128
consecutive pixels of the frame's row-major sequence instead of a 4 x 32 rectangle.  The arithmetic per output pixel is variant 21's (same chunk, tap and
product order into the same accumulator), so the yardstick is exact: bit identity with variant 21, next to the family's bound against the fp32 oracle.

The form exists for 30-column maps only.  Its 60-column sibling passed these same checks, measured slower per launch and was taken out of the library
(docs/experiments.md 10.11); the 60-column cases stay: there the forced id has to fall through to conv_choose's own pick, which is variant 21, so the same
two checks hold for them."""
import functools

import numpy as np
import pytest

import conv_form_cases as F

pytestmark = pytest.mark.gpu

F32S_TOL = 4e-6          # the split family's bound against the fp32 oracle (tests/test_gpu_ops.py)
V21, LIN = F.V21, F.LIN  # 60 columns: no linear form, the switch falls through (conv_form_cases.run_forced proves which of the two happened)

# n, h, w, cin, cout (conv_form_cases.LIN_SHAPES):
#   (2, 17, 30, 32, 192)       HRNet's 17 x 30 map: 510 pixels = 4 items, the last one 126 pixels
#   (3, 5, 30, 16, 384)        150 pixels: a partial last item, two Cout blocks, several frames
#   (1, 1, 30, 16, 192)        a single row: 30 of 32 lanes of one block
#   (2, 9, 30, 48, 192)        270 pixels: items start in the middle of a row
#   (2, 34, 60, 32, 192)       HRNet's 34 x 60 map (fall-through, see above)
#   (1, 3, 60, 16, 192), (2, 7, 60, 48, 384)
SHAPES = F.LIN_SHAPES
# launches of more than 256 items run the RING = 3 instances (every shape above stays under 256 items: the deep ring, RING = 6): (70, 17, 30, 16, 192) is 280 items
BIG = F.LIN_BIG


def _rand(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def _maps(n, h, w, c, seed):
    """noise on a ramp over (frame, row, column): neighbouring pixels, rows and frames differ, so a wrong row wrap or a wrong frame shows"""
    ff, yy, xx = np.mgrid[0:n, 0:h, 0:w]
    ramp = (((ff * 5 + yy * 3 + xx * 2) % 17) / 8.0 - 1.0)[..., None].astype(np.float32)
    return (ramp + _rand((n, h, w, c), seed, 0.5)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(shape, nres, post):
    """operands and the fp32 oracle's result of one case, computed once and shared (read-only) by the tests below"""
    from oracle import prims as P
    n, h, w, cin, cout = shape
    x = _maps(n, h, w, cin, 81)
    wt = _rand((3, 3, cin, cout), 82, (2.0 / (cin * 9)) ** 0.5)
    b = _rand((cout,), 83, 0.1)
    r1 = _maps(n, h, w, cout, 84) if nres >= 1 else None
    r2 = _maps(n, h, w, cout, 85) if nres >= 2 else None
    ref = P.conv2d(x, wt, b, stride=1, pre=0, r1=r1, r2=r2, post=post)
    for a in (x, wt, b, r1, r2, ref):
        if a is not None:
            a.setflags(write=False)
    return x, wt, b, r1, r2, ref


_got = {}


def _run(shape, nres, post, force, monkeypatch):
    """the case through op_conv2d under EAGLE_CONV_FORCE = force (None: conv_choose's own pick); the switch is read on every call.  Variant 21 and, on a
    30-column map, variant 27 must be what runs; the linear form's id at any other width must give conv_choose's own pick."""
    key = (shape, nres, post, force)
    if key not in _got:
        x, wt, b, r1, r2, _ = _case(shape, nres, post)
        y = F.run_forced(monkeypatch, "f32s", force, x, wt, b, 1, 0, r1, r2, post, expect="named" if force == V21 else F.lin_expect(shape[2]))
        y.setflags(write=False)
        _got[key] = y
    return _got[key]


def _identical(shape, nres, post, monkeypatch):
    old = _run(shape, nres, post, V21, monkeypatch)
    new = _run(shape, nres, post, LIN[shape[2]], monkeypatch)
    assert old.shape == new.shape
    if not np.array_equal(old, new):
        bad = np.argwhere(old != new)
        raise AssertionError(f"linear form differs from variant 21 at {len(bad)} of {old.size} values, first (n, y, x, c) = {tuple(bad[0])}: "
                             f"{old[tuple(bad[0])]!r} vs {new[tuple(bad[0])]!r}")


def _oracle(shape, nres, post, monkeypatch):
    ref = _case(shape, nres, post)[5]
    got = _run(shape, nres, post, LIN[shape[2]], monkeypatch)
    err = np.abs(ref - got).max() / max(np.abs(ref).max(), 1e-6)
    print(f"linear form {shape} res {nres} post {post}: error {err:.3g} of max|y|")
    assert err < F32S_TOL, f"linear A-direct conv error {err}"


@pytest.mark.parametrize("post", [0, 1])
@pytest.mark.parametrize("nres", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_linear_form_is_bit_identical_to_variant_21(shape, nres, post, monkeypatch):
    """Variant 27 against variant 21 on the same operands: single rows, partial last items, items that start in the middle of a row, several frames and
    Cout blocks, 0 / 1 / 2 residual operands, with and without ReLU.  Every bit must agree."""
    _identical(shape, nres, post, monkeypatch)


@pytest.mark.parametrize("post", [0, 1])
@pytest.mark.parametrize("nres", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_linear_form_against_oracle(shape, nres, post, monkeypatch):
    """The same cases against the fp32 oracle at the split family's bound."""
    _oracle(shape, nres, post, monkeypatch)


@pytest.mark.parametrize("shape", BIG)
def test_linear_form_shallow_ring(shape, monkeypatch):
    """More than 256 items: the RING = 3 instances (the cases above run the deep ring), with one residual and ReLU, both checks."""
    _identical(shape, 1, 1, monkeypatch)
    _oracle(shape, 1, 1, monkeypatch)


@pytest.mark.parametrize("shape", F.LIN_OTHER_WIDTHS)
def test_linear_form_falls_through_at_other_widths(shape, monkeypatch):
    """The linear form forced at a width it is not compiled for: conv_choose's own pick runs instead, without an error."""
    default = _run(shape, 1, 1, None, monkeypatch)
    forced = _run(shape, 1, 1, LIN[30], monkeypatch)
    assert np.array_equal(default, forced)
    _oracle_err = np.abs(_case(shape, 1, 1)[5] - forced).max() / max(np.abs(_case(shape, 1, 1)[5]).max(), 1e-6)
    assert _oracle_err < F32S_TOL, f"fall-through result error {_oracle_err}"
