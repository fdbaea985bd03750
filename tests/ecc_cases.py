"""Constructed inputs for the ECC camera-motion kernels (csrc/ecc.hip, K17), shared by tests/test_ecc_cases_cpu.py (which proves, with the
references alone, that every case forces what it is named after) and tests/test_gpu_ecc_ops.py (which holds the kernels to tests/ecc_ref.py bit for bit).

CASES[name] = (template u8 [h, w], image u8 [h, w], max_iter, eps); EXPECT[name] = (ok, exit, iters) as tests/ecc_ref.py and oracle/ecc.py give them.
Everything is deterministic: numpy.random.default_rng(seed), a Gaussian-filtered random texture, and scipy.ndimage.affine_transform for the motion.

Sizes: 4 x 4 (16 pixels: seven of the workgroup's eight waves idle), 5 x 130 (a long row, few rows), 16 x 32 (exactly one pixel per thread), 24 x 37
(888 pixels: a ragged second round) and 108 x 192 (the production shape; three pairs, for time).

Many ordinary pairs never meet eps = 1e-5: the 1/32-pixel quantisation of the warp's coordinates puts rho into a small cycle, and the kernel runs all
100 iterations (the cases named cycle_*, and several of the rotations).  A comparison with a tolerance is ill-conditioned on such a pair, a comparison of
bits is not; tests/test_ecc_cases_cpu.py shows that no float32 of any warp here depends on the last 4 ulps of asin, sin or cos, the only operations on
which a device and numpy need not agree.

The mask-empty exit (no template pixel has its nearest source pixel inside the image) is reached by the 4 x 4 pairs fail_empty_* after 3 and 4
iterations and by rotm6_fails_5x130 after 4: a 200-seed search was not needed."""
import functools

import numpy as np
from scipy import ndimage

import ecc_ref

SIZES = [(4, 4), (5, 130), (16, 32), (24, 37), (108, 192)]
PAD = 8
SHIFT_A, SHIFT_B = dict(dx=1.3, dy=-0.8), dict(dx=-1.7, dy=0.6)      # the warp's translation comes out as (-1.3, 0.8) and (1.7, -0.6)
ROT3, ROTM6 = dict(deg=3.0, dx=0.4, dy=0.3), dict(deg=-6.0)


def texture(seed, h, w, sigma, pad=PAD):
    """float64 [h + 2 pad, w + 2 pad] in 0 .. 255"""
    t = ndimage.gaussian_filter(np.random.default_rng(seed).random((h + 2 * pad, w + 2 * pad)), sigma)
    return (t - t.min()) / (t.max() - t.min()) * 255.0


def _cut(a, h, w, pad=PAD):
    return np.clip(np.rint(a[pad:pad + h, pad:pad + w]), 0, 255).astype(np.uint8)


def moved(seed, h, w, dx=0.0, dy=0.0, deg=0.0, sigma=None):
    """(template, image): the image shows the texture rotated by deg about the centre and shifted by (dx, dy) pixels, bilinearly resampled"""
    sigma = (1.0 if min(h, w) < 8 else 2.0) if sigma is None else sigma
    tex = texture(seed, h, w, sigma)
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    A = np.array([[c, -s], [s, c]])
    ctr = np.array([PAD + (h - 1) / 2, PAD + (w - 1) / 2])
    img = ndimage.affine_transform(tex, A, offset=ctr - A @ ctr + np.array([dy, dx]), order=1, mode="nearest")
    return _cut(tex, h, w), _cut(img, h, w)


def stripes(h, w, phase):
    """vertical stripes: every row the same, so that the image's y gradient is 0 everywhere"""
    row = np.rint(127.5 + 100.0 * np.sin((np.arange(w) + phase) * 0.9)).astype(np.uint8)
    return np.repeat(row[None, :], h, 0)


# name -> (size, seed, motion, max_iter, eps, (ok, exit, iters))
_MOVED = {
    "ident_4x4": ((4, 4), 0, {}, 100, 1e-5, (1, "eps", 2)),
    "fail_lambda_4x4": ((4, 4), 0, SHIFT_A, 100, 1e-5, (0, "lambda", 2)),
    "fail_empty_a_4x4": ((4, 4), 1, SHIFT_A, 100, 1e-5, (0, "empty mask", 3)),
    "fail_empty_b_4x4": ((4, 4), 2, SHIFT_A, 100, 1e-5, (0, "empty mask", 4)),
    "fail_nan_4x4": ((4, 4), 1, SHIFT_B, 100, 1e-5, (0, "nan", 3)),
    "fail_rot3_4x4": ((4, 4), 1, ROT3, 100, 1e-5, (0, "lambda", 4)),
    "fail_rotm6_4x4": ((4, 4), 2, ROTM6, 100, 1e-5, (0, "empty mask", 14)),
    "ident_5x130": ((5, 130), 0, {}, 100, 1e-5, (1, "eps", 2)),
    "shift_a_5x130": ((5, 130), 0, SHIFT_A, 100, 1e-5, (1, "eps", 6)),
    "shift_b_5x130": ((5, 130), 0, SHIFT_B, 100, 1e-5, (1, "eps", 23)),
    "cycle_5x130": ((5, 130), 1, SHIFT_A, 100, 1e-5, (1, "count", 100)),
    "rot3_5x130": ((5, 130), 0, ROT3, 100, 1e-5, (1, "count", 100)),
    "rotm6_5x130": ((5, 130), 1, ROTM6, 100, 1e-5, (1, "count", 100)),
    "rotm6_fails_5x130": ((5, 130), 0, ROTM6, 100, 1e-5, (0, "empty mask", 4)),
    "ident_16x32": ((16, 32), 0, {}, 100, 1e-5, (1, "eps", 2)),
    "shift_a_16x32": ((16, 32), 1, SHIFT_A, 100, 1e-5, (1, "eps", 6)),
    "shift_b_16x32": ((16, 32), 0, SHIFT_B, 100, 1e-5, (1, "eps", 7)),
    "rot3_16x32": ((16, 32), 0, ROT3, 100, 1e-5, (1, "eps", 7)),
    "rotm6_16x32": ((16, 32), 0, ROTM6, 100, 1e-5, (1, "eps", 14)),
    "cycle_16x32": ((16, 32), 1, ROTM6, 100, 1e-5, (1, "count", 100)),
    "ident_24x37": ((24, 37), 0, {}, 100, 1e-5, (1, "eps", 2)),
    "shift_a_24x37": ((24, 37), 0, SHIFT_A, 100, 1e-5, (1, "eps", 4)),
    "shift_b_24x37": ((24, 37), 1, SHIFT_B, 100, 1e-5, (1, "eps", 17)),
    "rot3_24x37": ((24, 37), 0, ROT3, 100, 1e-5, (1, "eps", 9)),
    "rotm6_24x37": ((24, 37), 0, ROTM6, 100, 1e-5, (1, "eps", 8)),
    "cycle_24x37": ((24, 37), 2, SHIFT_A, 100, 1e-5, (1, "count", 100)),
    "cycle_rot3_24x37": ((24, 37), 1, ROT3, 100, 1e-5, (1, "count", 100)),
    "count7_24x37": ((24, 37), 0, ROT3, 7, 0.0, (1, "count", 7)),
    "zero_iterations_24x37": ((24, 37), 0, SHIFT_A, 0, 1e-5, (1, "count", 0)),
    "shift_a_108x192": ((108, 192), 0, SHIFT_A, 100, 1e-5, (1, "eps", 13)),
    "rot3_108x192": ((108, 192), 0, ROT3, 100, 1e-5, (1, "eps", 7)),
    "cycle_108x192": ((108, 192), 2, SHIFT_A, 100, 1e-5, (1, "count", 100)),
}
ROTATIONS = {n: (3.0 if "rot3" in n else -6.0) for n in _MOVED if ("rot3" in n or "rotm6" in n) and _MOVED[n][5][0] == 1 and "4x4" not in n}
SHIFTED = [n for n in _MOVED if n.startswith(("shift_", "cycle_")) and "rot" not in n]
CYCLES = [n for n in _MOVED if _MOVED[n][3] == 100 and _MOVED[n][5] == (1, "count", 100)]
QUICK = [n for n in _MOVED if _MOVED[n][5][1] == "eps" and 2 < _MOVED[n][5][2] < 15]


def _build():
    cases, expect = {}, {}
    for name, ((h, w), seed, motion, max_iter, eps, exp) in _MOVED.items():
        t, i = moved(seed, h, w, **motion)
        cases[name] = (t, i, max_iter, eps); expect[name] = exp
    t, i = moved(0, 24, 37, **SHIFT_A)
    other = moved(5, 24, 37)[0]

    def add(name, tt, ii, exp, max_iter=100, eps=1e-5):
        cases[name] = (np.ascontiguousarray(tt), np.ascontiguousarray(ii), max_iter, eps); expect[name] = exp

    add("flat_image_0_24x37", t, np.zeros_like(t), (0, "nan", 1))
    add("flat_image_255_24x37", t, np.full_like(t, 255), (0, "nan", 1))
    add("flat_template_24x37", np.full_like(t, 90), i, (0, "nan", 1))
    add("negative_24x37", t, 255 - t, (0, "lambda", 1))
    add("stripes_same_24x37", stripes(24, 37, 0.0), stripes(24, 37, 0.0), (1, "eps", 2))
    add("stripes_moved_16x32", stripes(16, 32, 0.0), stripes(16, 32, 0.7), (1, "eps", 2))
    add("unrelated_24x37", t, other, (0, "lambda", 1))
    return cases, expect


CASES, EXPECT = _build()
NAMES = list(CASES)
STRIPES = ["stripes_same_24x37", "stripes_moved_16x32"]


def size_of(name):
    return CASES[name][0].shape


@functools.lru_cache(maxsize=None)
def expected(name, max_iter=None, eps=None):
    """(ok, iters, rho, M float32 [6], trace) of tests/ecc_ref.py, computed once per process; max_iter / eps override the case's own"""
    t, i, mi, e = CASES[name]
    trace = []
    ok, iters, rho, M = ecc_ref.align(t, i, mi if max_iter is None else max_iter, e if eps is None else eps, trace=trace, check_libm=True)
    M.setflags(write=False)
    return ok, iters, rho, M, tuple(trace)


# ---- the 0.15-scale image ---------------------------------------------------------------------------------------------------------------------
SMALL_SIZES = [(27, 27), (30, 50), (47, 33), (150, 170), (64, 64), (720, 1280)]
SMALL_DIMS = {(27, 27): (4, 4), (30, 50): (4, 8), (47, 33): (7, 5), (150, 170): (22, 26), (64, 64): (10, 10), (720, 1280): (108, 192)}


@functools.lru_cache(maxsize=None)
def gray_frames(hw):
    """u8 [n, h, w]: random bytes and a smooth texture (720 x 1280: one frame, its upper half random bytes, its lower half smooth)"""
    h, w = hw
    rng = np.random.default_rng(1000 * h + w)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    smooth = _cut(texture(h + w, h, w, 3.0), h, w)
    if hw == (720, 1280):
        out = np.concatenate([noise[:360], smooth[360:]])[None]
    else:
        out = np.stack([noise, smooth])
    out.setflags(write=False)
    return out


# ---- clips for the session tests --------------------------------------------------------------------------------------------------------------
CLIP_HW = (160, 200)


@functools.lru_cache(maxsize=None)
def clip_gray():
    """f0 .. f3 u8 [4, 160, 200]: a smooth texture that moves by one or two pixels per frame; and a black frame"""
    h, w = CLIP_HW
    tex = texture(77, h, w, 5.0)
    offs = [(0, 0), (2, 1), (3, 3), (5, 4)]
    f = np.stack([np.clip(np.rint(tex[PAD - dy:PAD - dy + h, PAD - dx:PAD - dx + w]), 0, 255).astype(np.uint8) for dx, dy in offs])
    f.setflags(write=False)
    return f


def bgr(gray):
    """gray-valued BGR frames"""
    return np.ascontiguousarray(np.repeat(np.asarray(gray)[..., None], 3, axis=-1))
