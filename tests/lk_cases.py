"""Small constructed inputs for the optical-flow kernels (tests/test_lk_cases_cpu.py proves what each one forces, tests/test_gpu_lk.py runs them).

CASES[name] = (frames [n, h, w, 3] u8, src, dst, integer points [(x, y)]): the flow of frame src -> frame dst is computed for the points, which become
the key-points of labels 0, 1, ... in that order (key_points()); the hue windows are read from frame dst, as the loop does.  Everything is generated from
seeds.  Names say what a case forces:

  translate_*   a smooth random texture and the same texture moved by a known sub-pixel amount (SHIFTS[name] = (dx, dy)); `same_*` = identical frames
  odd3_*        33 x 95 with three DIFFERENT frames: 9405 pixels per clip (9405 % 4 == 1: the scalar tail of the gray kernel), odd at every level
  uncorrelated, far_shift   pairs on which the Newton steps are large and erratic: windows leave the neighbourhood of their start window
  final_window_*  points that lose their status by the last rule only: the rounded origin of the final window lies outside the frame
  flat_*, edge  nothing to track: constant frames and one straight edge (the aperture problem)
  extreme_*     the largest products a window sum can hold, all of one sign (see extreme_pair)
  count_*       0, 1 and 4 points;  every other case carries 57 or a handful
  filter_*      the status / z-score / hue rules of calculate_optical_flow"""
import numpy as np

SIZES = [(32, 32), (60, 60), (61, 61), (64, 61), (33, 95), (243, 321)]      # height x width


def _smooth(rng, h, w, sigma):
    """Periodic band-limited noise, zero mean and unit deviation: white noise times a Gaussian in the Fourier domain."""
    f = np.fft.fft2(rng.standard_normal((h, w)))
    ky, kx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    t = np.real(np.fft.ifft2(f * np.exp(-2 * np.pi ** 2 * sigma ** 2 * (ky ** 2 + kx ** 2))))
    return (t - t.mean()) / t.std()


def texture(seed, h, w, sigma=2.0):
    """A float BGR picture [h, w, 3]: smooth luminance of high contrast and a hue that changes every few pixels."""
    rng = np.random.default_rng(seed)
    lum = 128 + 60 * _smooth(rng, h, w, sigma)
    hue = (3.0 * _smooth(rng, h, w, 1.5)) % 6.0
    c = 70.0                                               # chroma
    x = c * (1 - np.abs(hue % 2 - 1))
    z = np.zeros_like(hue)
    sector = hue.astype(int)
    r = np.choose(sector, [c + z, x, z, z, x, c + z]); g = np.choose(sector, [x, c + z, c + z, x, z, z]); b = np.choose(sector, [z, z, x, c + z, c + z, x])
    return np.stack([b, g, r], -1) + (lum - c / 2)[..., None]


def moved(pic, dx, dy):
    """pic moved by (dx, dy) pixels (what was at x is at x + dx), exactly, as a periodic band-limited signal."""
    h, w = pic.shape[:2]
    ky, kx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    ramp = np.exp(-2j * np.pi * (ky * dy + kx * dx))[..., None]
    return np.real(np.fft.ifft2(np.fft.fft2(pic, axes=(0, 1)) * ramp, axes=(0, 1)))


def u8(pic):
    return np.clip(np.rint(pic), 0, 255).astype(np.uint8)


def gray3(g):
    """A BGR frame whose gray conversion is exactly g (B = G = R)."""
    return np.repeat(np.asarray(g, np.uint8)[..., None], 3, -1)


def boundary_values(size):
    """Coordinates around the two status boundaries of one axis.  The window origin is the coordinate - 7: -9 and size + 7, size + 8 put it outside [-15, size - 1];
    at -8 the window has no pixel inside the frame and at -7 / size + 6 only the frame's edge column, where the reflected Scharr derivative across the edge is 0,
    so these three never pass the determinant test either.  -6 and size + 5 are the outermost points that can be tracked."""
    return [-9, -8, -7, -6, size + 5, size + 6, size + 7, size + 8]


def interior_points(seed, h, w, count, margin=12):
    rng = np.random.default_rng(seed)
    return [(int(x), int(y)) for x, y in zip(rng.integers(margin, w - margin, count), rng.integers(margin, h - margin, count))]


def points57(seed, h, w):
    """57 integer points: the four corners, the status boundaries in x and in y, points far outside, duplicates, and interior points."""
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
    pts += [(x, h // 2) for x in boundary_values(w)] + [(w // 2, y) for y in boundary_values(h)]
    pts += [(-1000, h // 2), (w // 2, 100000), (3 * w, -3 * h)]
    inner = interior_points(seed, h, w, 57 - len(pts) - 2) if min(h, w) > 24 else [(w // 2, h // 2)] * (57 - len(pts) - 2)
    pts += inner + [inner[0], inner[3]]
    assert len(pts) == 57
    return pts


def is_interior(pt, h, w, margin=12):
    return margin <= pt[0] < w - margin and margin <= pt[1] < h - margin


def extreme_pair(sign, axis, h=60, w=60):
    """Two gray frames on which half of a window's pixels reach the largest |diff * derivative| a window sum can hold, all with one sign.

    Stripes two pixels wide (values 0 0 255 255 across `axis`) give |Ix| = 16 * 255 = 4080 (the Scharr weights 3 + 10 + 3 times the step), and the same
    stripes moved by one pixel give |J - I| = 255 * 32 = 8160 on every second pixel, always with the derivative's sign (or always against it: `sign`).
    Stripes alone have no second direction (A22 = 0: the determinant test rejects the point before any such sum is formed), so the stripes are inverted in
    bands of 8 rows; rows next to a band edge have |Ix| = 10 * 255.  Both upper pyramid levels see the stripes as a period of two pixels or as a constant,
    their derivative across the stripes is 0 and they reject every point, so level 0 starts at the integer point itself with weights (16384, 0, 0, 0).
    By construction a 64-pixel partial sum stays below 64 * 8160 * 4080 = 2,130,739,200 < 2^31.  Reached on these frames (test_lk_cases_cpu.py
    asserts the range and prints the figure): +-1,131,955,200 = 34 * 8160 * 4080 in the Ix sums (stripes across x) and
    +1,082,016,000 / -1,044,561,600 in the Iy sums (stripes across y: the 64-pixel runs cut the window row by row, so the two directions differ)."""
    y, x = np.mgrid[0:h, 0:w]
    def stripes(xx):
        return 255 * ((((xx % 4) >= 2) ^ ((y % 16) >= 8)).astype(np.int64))
    a, b = stripes(x), stripes(x - sign)
    if axis == "y":
        a, b = a.T, b.T
    return np.stack([gray3(a), gray3(b)])


SHIFTS = {}
CASES = {}


def _build():
    c = CASES
    # textured translation, every size; three different sub-pixel shifts at the largest one
    big = texture(1, 243, 321)
    big_shifts = [(0.4, -0.7), (-2.3, 1.6), (2.9, 2.2)]
    big_clip = np.stack([u8(big)] + [u8(moved(big, dx, dy)) for dx, dy in big_shifts])
    for k, s in enumerate(big_shifts):
        c[f"translate_243x321_{k}"] = (big_clip, 0, k + 1, points57(10 + k, 243, 321)); SHIFTS[f"translate_243x321_{k}"] = s
    c["same_243x321"] = (big_clip, 0, 0, points57(13, 243, 321)); SHIFTS["same_243x321"] = (0.0, 0.0)
    for seed, (h, w), s in [(2, (32, 32), (0.6, -0.4)), (3, (60, 60), (-1.2, 0.8)), (4, (61, 61), (1.7, 1.1)), (5, (64, 61), (-0.5, -2.4))]:
        pic = texture(seed, h, w)
        clip = np.stack([u8(pic), u8(moved(pic, *s))])
        c[f"translate_{h}x{w}"] = (clip, 0, 1, points57(20 + seed, h, w)); SHIFTS[f"translate_{h}x{w}"] = s
        c[f"same_{h}x{w}"] = (clip, 1, 1, points57(30 + seed, h, w)); SHIFTS[f"same_{h}x{w}"] = (0.0, 0.0)
    # three different frames, odd at every level: a wrong frame offset in K11 or K12 reads another frame
    pic = texture(6, 33, 95)
    odd = np.stack([u8(pic), u8(moved(pic, 1.3, -0.6)), u8(texture(7, 33, 95))])
    assert odd.size // 3 % 4 == 1
    c["odd3_33x95_translate"] = (odd, 0, 1, points57(40, 33, 95)); SHIFTS["odd3_33x95_translate"] = (1.3, -0.6)
    c["odd3_33x95_uncorrelated"] = (odd, 1, 2, points57(41, 33, 95))
    c["odd3_33x95_same_last"] = (odd, 2, 2, points57(42, 33, 95)); SHIFTS["odd3_33x95_same_last"] = (0.0, 0.0)
    c["odd3_33x95_backwards"] = (odd, 2, 0, points57(43, 33, 95))
    # large erratic steps
    noise = np.stack([u8(big), u8(texture(8, 243, 321, sigma=1.2))])
    c["uncorrelated_243x321"] = (noise, 0, 1, points57(50, 243, 321))
    smooth = texture(9, 243, 321, sigma=5.0)
    c["far_shift_243x321"] = (np.stack([u8(smooth), u8(moved(smooth, 40.0, 0.0))]), 0, 1, points57(51, 243, 321))
    # the last status rule (the rounded final window must start inside the frame): points just inside the right / lower boundary and a picture that moves
    # outwards, so that the iterations end with a window origin in [size - 0.5, size): floor() passed the loop's test, rint() fails the final one
    pic = texture(105, 64, 61)
    c["final_window_x_64x61"] = (np.stack([u8(pic), u8(moved(pic, 2.9, 0.0))]), 0, 1, [(61 + k, y) for k in (3, 4, 5) for y in range(10, 56, 3)] + interior_points(80, 64, 61, 6))
    pic = texture(111, 61, 61)
    c["final_window_y_61x61"] = (np.stack([u8(pic), u8(moved(pic, 0.0, 1.8))]), 0, 1, [(x, 61 + k) for k in (3, 4, 5) for x in range(10, 52, 3)] + interior_points(81, 61, 61, 6))
    # nothing to track
    c["flat_black_60x60"] = (np.zeros((2, 60, 60, 3), np.uint8), 0, 1, points57(60, 60, 60))
    c["flat_white_61x61"] = (np.full((2, 61, 61, 3), 255, np.uint8), 0, 1, points57(61, 61, 61))
    edge = np.full((64, 61), 40, np.uint8); edge[:, 30:] = 200
    edge2 = np.full((64, 61), 40, np.uint8); edge2[:, 31:] = 200
    c["edge_64x61"] = (np.stack([gray3(edge), gray3(edge2)]), 0, 1, points57(62, 64, 61))
    # extreme contrast
    ext = [(x, y) for y in (20, 23, 26, 29, 33) for x in (20, 21, 22, 23, 30)] + [(0, 0), (59, 59), (7, 52), (52, 7)]      # 25 inside, 4 at the frame's edge
    for axis in ("x", "y"):
        for name, sign in (("pos", -1), ("neg", 1)):
            c[f"extreme_{name}_{axis}_60x60"] = (extreme_pair(sign, axis), 0, 1, ext if axis == "x" else [(y, x) for x, y in ext])
    # point counts
    small = c["translate_32x32"][0]
    c["count_0_32x32"] = (small, 0, 1, [])
    c["count_1_32x32"] = (small, 0, 1, [(15, 16)])
    c["count_4_61x61"] = (c["translate_61x61"][0], 0, 1, [(30, 30), (20, 41), (-8, 30), (44, 18)])
    # filter rules
    c["filter_one_survivor_60x60"] = (c["translate_60x60"][0], 0, 1, [(-40, 10), (200, 30), (31, 28), (30, -30), (1000, 1000)])
    c["filter_identical_moves_61x61"] = (c["translate_61x61"][0], 0, 0, interior_points(70, 61, 61, 12, margin=14))
    # ten points, nine on a still picture and one inside a patch that moves: its z-score is (d - d/10) / (0.3 d) = 3
    still = u8(big)
    patch = u8(moved(big, 2.5, 0.0))
    outl = still.copy(); outl[90:150, 180:240] = patch[90:150, 180:240]
    ten = [(40, 40), (100, 30), (280, 50), (60, 120), (210, 120), (120, 200), (250, 210), (30, 215), (150, 60), (290, 150)]
    c["filter_outlier_243x321"] = (np.stack([still, outl]), 0, 1, ten)
    # hue: bands of two hues 6 pixels wide under a luminance texture; the picture moves by 3 pixels, so the 3 x 3 windows around the old and the new
    # place of a point lie in different bands for some points and in the same band for others
    lum = 128 + 50 * _smooth(np.random.default_rng(11), 64, 61, 2.0)
    band = ((np.arange(61) // 6) % 2)[None, :, None]
    tint = np.where(band == 1, np.array([40.0, 0.0, -40.0]), np.array([-40.0, 0.0, 40.0]))      # bluish / reddish
    huepic = lum[..., None] + tint
    c["filter_hue_change_64x61"] = (np.stack([u8(huepic), u8(np.roll(huepic, 3, axis=1))]), 0, 1, interior_points(71, 64, 61, 24, margin=14))
    # hue windows clipped at the corners and edges of the smallest frame (2 x 2 and 2 x 3 pixels)
    c["filter_corner_32x32"] = (small, 0, 1, [(0, 0), (31, 0), (0, 31), (31, 31), (1, 1), (30, 30), (0, 16), (16, 0), (31, 16), (16, 31), (16, 16), (33, 33)])


_build()


def key_points(pts):
    """The case's points as the key-point list the references take: [(label, (x, y))], labels 0, 1, ... in order."""
    return [(k, (int(x), int(y))) for k, (x, y) in enumerate(pts)]


_expected = {}


def expected(name):
    """lk_ref's answer for a case, computed once per process: (filtered [(label, (x, y))], next [n, 2] f32, status [n] u8, trace)."""
    if name not in _expected:
        import lk_ref
        frames, src, dst, pts = CASES[name]
        _expected[name] = lk_ref.flow(frames, src, dst, dst, key_points(pts))
    return _expected[name]
