"""Constructed cases for the team clustering (tests/kits_ref.py is the contract), each named after what it forces.  Two kinds: "pixels" (frames of
64 x 96, crops, slots: the whole stage) and "ids" (per-id sums and crop counts: steps 5 to 11 alone, for ties and degenerate distances that pixels cannot
reach).  FORCES[name] checks on the contract's own output that the case forces what its name says.

One case of the issue cannot exist as stated.  A window of zero width: the window's width is w - 2 (w // 4) >= w / 2, never 0 for a crop of w >= 1; what
can be empty is its height, h // 2 - h // 5 = 0 at h = 1, which ``window_of_no_height_h_1`` forces, and ``w_below_4_keeps_its_width`` shows the widths.
``hue_edges_and_wrap`` holds every one of the fifteen bin edges, its two neighbours, and 179 and 0, at two values of the lower band and, where a pixel
exists, two of the upper: a bright, saturated green keys away as grass, so the edges 54 and 66 and their neighbours exist in the lower band only (a dark
or weakly saturated green does not key away: BGR (29, 48, 33) has hue 54)."""
import functools

import numpy as np

import kits_ref as KR

FH, FW = 64, 96
GRASS = (40, 140, 50)                                                           # BGR


def _all_with_max(v):
    a = np.arange(v + 1)
    g1, g2 = np.meshgrid(a, a, indexing="ij")
    faces = [np.stack([g1, g2, np.full_like(g1, v)], -1), np.stack([g1, np.full_like(g1, v), g2], -1), np.stack([np.full_like(g1, v), g1, g2], -1)]
    return np.concatenate([f.reshape(-1, 3) for f in faces])


@functools.lru_cache(None)
def _table(v):
    px = _all_with_max(v)
    h, s, vv = KR.hsv_array(px)
    grass = (px[:, 1] >= 48) & (px[:, 1] - np.maximum(px[:, 2], px[:, 0]) >= 16)
    return px, h, s, grass


def bgr_of(h, v=200, s_min=64):
    """a BGR pixel of value v that is not grass, has hue h and saturation >= s_min, or None"""
    px, hh, ss, grass = _table(v)
    ok = np.nonzero((hh == h) & (ss >= s_min) & ~grass)[0]
    return None if len(ok) == 0 else tuple(int(c) for c in px[ok[0]])


def hues_of_the_upper_band():
    """every hue a pixel of v >= 144 and s >= 64 that is not grass can have (all values of v, nothing kept)"""
    out = set()
    for v in range(144, 256):
        px = _all_with_max(v)
        h, s, _ = KR.hsv_array(px)
        grass = (px[:, 1] >= 48) & (px[:, 1] - np.maximum(px[:, 2], px[:, 0]) >= 16)
        out |= set(np.unique(h[(s >= 64) & ~grass]).tolist())
    return out


class _Clip:
    """frames of grass; crops are laid side by side and their shirt windows painted row-major"""

    def __init__(self):
        self.frames, self.crops, self.slots = [self._blank()], [], []
        self.x = self.y = self.rowh = 0

    @staticmethod
    def _blank():
        return np.tile(np.array(GRASS, np.uint8), (FH, FW, 1))

    def place(self, w, h):
        if self.x + w > FW:
            self.x, self.y, self.rowh = 0, self.y + self.rowh + 1, 0
        if self.y + h > FH:
            self.frames.append(self._blank())
            self.x = self.y = self.rowh = 0
        box = (len(self.frames) - 1, self.x, self.y, self.x + w, self.y + h)
        self.x, self.rowh = self.x + w + 1, max(self.rowh, h)
        return box

    def add(self, w, h, slot, pixels=None, box=None):
        """pixels: one BGR for the whole window, or a list painted row-major (the rest of the window stays grass)"""
        box = box or self.place(w, h)
        f, x1, y1, x2, y2 = box
        flag, rows, cols = KR.window_of(box, len(self.frames), FH, FW)
        if not flag and pixels is not None:
            win = self.frames[f][rows[0]:rows[1], cols[0]:cols[1]]
            flat = win.reshape(-1, 3).copy()
            if isinstance(pixels, tuple):
                flat[:] = pixels
            else:
                flat[:len(pixels)] = np.array(pixels, np.uint8).reshape(-1, 3)
            win[:] = flat.reshape(win.shape)
        self.crops.append(box)
        self.slots.append(slot)
        return box

    def case(self, name, n_ids=None, **p):
        slots = np.array(self.slots, np.int32)
        return dict(name=name, kind="pixels", frames=np.stack(self.frames), crops=np.array(self.crops, np.int32).reshape(-1, 5), slots=slots,
                    n_ids=int(slots.max()) + 1 if n_ids is None else n_ids, p=p)


RED, BLUE, WHITE = (30, 30, 220), (220, 60, 30), (240, 240, 240)
CASES, FORCES = [], {}


def _add(case, force=None):
    CASES.append(case)
    if force is not None:
        FORCES[case["name"]] = force


# ---- windows ------------------------------------------------------------------------------------------------------------------------------------
def _sizes():
    c = _Clip()
    sizes = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 10), (4, 5), (5, 10), (7, 9), (12, 30), (96, 64)]
    for k, (w, h) in enumerate(sizes):
        c.add(w, h, k, RED if k % 2 else BLUE)

    def force(crops, ids, model):
        for (w, h), r in zip(sizes, crops):
            n = (w - 2 * (w // 4)) * (h // 2 - h // 5)
            assert (r["flags"], r["n"]) == ((KR.CROP_EMPTY, 0) if n == 0 else (0, n)), (w, h)
        assert crops[0]["flags"] == KR.CROP_EMPTY and crops[1]["n"] == 1 and ids[0]["team"] == -1 and ids[1]["team"] >= 0
    _add(c.case("crops_from_1x1_upward", min_pixels=1, min_crops=1), force)

    c = _Clip()
    for k, w in enumerate((1, 5, 40)):
        c.add(w, 1, k, RED)
    c.add(8, 10, 3, RED)

    def force(crops, ids, model):
        assert (crops["flags"][:3] == KR.CROP_EMPTY).all() and not crops["units"][:3].any() and (ids["skipped"][:3] == 1).all() and (ids["team"][:3] == -1).all()
    _add(c.case("window_of_no_height_h_1", min_pixels=1, min_crops=1), force)

    c = _Clip()
    for k, w in enumerate((1, 2, 3, 4, 5)):
        c.add(w, 10, k, BLUE)

    def force(crops, ids, model):
        assert [int(n) for n in crops["n"]] == [3, 6, 9, 6, 9] and not crops["flags"].any()
    _add(c.case("w_below_4_keeps_its_width", min_pixels=1, min_crops=1), force)

    c = _Clip()
    c.add(16, 20, 0, None)
    c.add(16, 20, 1, RED)

    def force(crops, ids, model):
        assert crops[0]["flags"] == KR.CROP_FEW and crops[0]["n"] == 0 and not crops[0]["units"].any() and ids[0]["team"] == -1 and ids[1]["used"] == 1
    _add(c.case("window_all_grass", min_crops=1), force)

    c = _Clip()
    c.add(16, 20, 0, [RED] * 31)                                                # a window of 8 x 6 = 48 pixels
    c.add(16, 20, 1, [RED] * 32)
    c.add(16, 20, 2, [RED] * 33)

    def force(crops, ids, model):
        assert [int(n) for n in crops["n"]] == [31, 32, 33] and [int(f) for f in crops["flags"]] == [KR.CROP_FEW, 0, 0]
        assert crops[0]["units"].sum() == 12 * 31 and [int(u) for u in ids["used"]] == [0, 1, 1] and ids[0]["skipped"] == 1
    _add(c.case("min_pixels_minus_1_and_min_pixels", min_crops=1), force)

    c = _Clip()
    c.add(12, 30, 0, RED)
    for k, box in enumerate([(0, 90, 0, 102, 30), (0, 10, 40, 22, 70), (0, -1, 0, 11, 30), (0, 0, -2, 12, 28), (1, 0, 0, 12, 30), (-1, 0, 0, 12, 30), (0, 20, 20, 20, 40), (0, 30, 30, 25, 50)]):
        c.add(0, 0, 1 + k, None, box=box)

    def force(crops, ids, model):
        assert [int(f) for f in crops["flags"]] == [0] + [KR.CROP_OUTSIDE] * 6 + [KR.CROP_EMPTY] * 2 and not crops["units"][1:].any() and (ids["team"][1:] == -1).all()
    _add(c.case("crops_leaving_the_frame_or_the_clip", min_crops=1), force)


# ---- pixels -------------------------------------------------------------------------------------------------------------------------------------
HUE_EDGES = [6 + 12 * k for k in range(15)]
HUES = sorted({(e + d) % 180 for e in HUE_EDGES for d in (-1, 0, 1)} | {179, 0})
LOWER_BAND_ONLY = [43, 53, 54, 55, 65, 66, 67]                                  # of HUES: no chromatic pixel of v >= 144 that is not grass has them (hues_of_the_upper_band)
HUE_VALUES = (200, 144, 76, 48)                                                 # two values of the upper band (v >= 144), two of the lower


def _pixels():
    c = _Clip()
    made = [(h, v, bgr_of(h, v)) for h in HUES for v in HUE_VALUES if bgr_of(h, v) is not None]
    for k, (h, v, px) in enumerate(made):
        c.add(4, 5, k, px)                                                      # a window of 2 x 1

    def force(crops, ids, model):
        lower, upper = {h for h, v, _ in made if v < 144}, {h for h, v, _ in made if v >= 144}
        assert lower == set(HUES) and set(HUES) - upper == set(LOWER_BAND_ONLY), (sorted(set(HUES) - lower), sorted(set(HUES) - upper))
        for (h, v, px), r in zip(made, crops):
            t = (h + 174) % 180
            k, f = t // 12, t % 12
            exp, base = np.zeros(KR.BINS, np.int64), (0 if v < 144 else 15)
            exp[base + k] += 2 * (12 - f); exp[base + (k + 1) % 15] += 2 * f
            assert np.array_equal(r["units"], exp) and r["n"] == 2, (h, v)
        i179, i0 = [m[:2] for m in made].index((179, 200)), [m[:2] for m in made].index((0, 200))
        assert crops[i179]["units"][15 + 14] == 14 and crops[i179]["units"][15] == 10 and crops[i0]["units"][15 + 14] == 12 and crops[i0]["units"][15] == 12
    _add(c.case("hue_edges_and_wrap", min_pixels=1, min_crops=1), force)

    c = _Clip()
    px = [(0, 0, 47), (0, 0, 48), (0, 0, 143), (0, 0, 144), (63, 63, 63), (64, 64, 64), (127, 127, 127), (128, 128, 128), (191, 191, 191), (192, 192, 192),
          (192, 192, 255), (191, 191, 255), (0, 0, 0), (255, 255, 255)]
    for k, p in enumerate(px):
        c.add(4, 5, k, p)

    def force(crops, ids, model):
        bins = [int(np.argmax(r["units"])) for r in crops]
        # v 47: black; v 48 and 143: hue 0 in the lower band (bins 14 and 0, six units each a pixel); v 144: the upper band; the greys across 63 / 64, 127 / 128,
        # 191 / 192; s 63: the white bin; s 64: hue 0 in the upper band; black; white
        assert bins == [30, 0, 0, 15, 30, 31, 31, 32, 32, 33, 33, 15, 30, 33] and (crops["n"] == 2).all()
        assert KR.hsv_px(192, 192, 255)[1] == 63 and KR.hsv_px(191, 191, 255)[1] == 64
    _add(c.case("value_and_saturation_thresholds", min_pixels=1, min_crops=1), force)


# ---- counts of crops ----------------------------------------------------------------------------------------------------------------------------
def _random_clip(name, n_crops, n_ids, seed, n_frames=3):
    r = np.random.default_rng(seed)
    frames = r.integers(0, 256, (n_frames, FH, FW, 3), dtype=np.uint8)
    frames[:, :, : FW // 2] //= 2                                               # a darker half: more of the lower hue band
    w, h = r.integers(1, 30, n_crops), r.integers(1, 50, n_crops)
    x, y = r.integers(0, FW - w + 1), r.integers(0, FH - h + 1)
    crops = np.stack([r.integers(0, n_frames, n_crops), x, y, x + w, y + h], 1).astype(np.int32).reshape(-1, 5)
    slots = r.integers(0, max(n_ids, 1), n_crops).astype(np.int32)
    return dict(name=name, kind="pixels", frames=frames, crops=crops, slots=slots, n_ids=n_ids, p={})


def _counts():
    for n in (0, 1, 4, 5, 1000):
        def force(crops, ids, model, n=n):
            assert len(crops) == n and ids["used"].sum() + ids["skipped"].sum() == n
            if n == 1000:
                assert model[0]["voters"] >= 8 and (crops["flags"] == 0).sum() > 400 and (crops["flags"] == KR.CROP_FEW).sum() > 50
        _add(_random_clip(f"crops_{n}", n, 12 if n == 1000 else 3, 100 + n), force)

    def force(crops, ids, model):
        assert len(crops) == 0 and len(ids) == 0 and model[0]["flags"] == KR.MODEL_SINGLE and model[0]["a"] == -1 and model[0]["voters"] == 0
    _add(_random_clip("ids_0_and_no_crops", 0, 0, 7), force)


# ---- ids ----------------------------------------------------------------------------------------------------------------------------------------
def _ids_case(name, sums, used, **p):
    return dict(name=name, kind="ids", sums=np.array(sums, np.int64).reshape(-1, KR.BINS), used=np.array(used, np.int32).reshape(-1), p=p)


def _row(**bins):
    v = [0] * KR.BINS
    for k, x in bins.items():
        v[int(k[1:])] = x
    return v


def _random_ids(n, seed):
    r = np.random.default_rng(seed)
    kit = r.integers(0, 2, n)
    base = np.zeros((2, KR.BINS), np.int64)
    base[0, [9, 24, 33]], base[1, [0, 15, 31]] = (9000, 2000, 1000), (7000, 3000, 2000)
    used = r.integers(1, 12, n)
    sums = base[kit] * used[:, None] + r.integers(0, 100, (n, KR.BINS)) * used[:, None]
    return sums, used


def _ids():
    for n in (0, 1, 2, 3, 63, 64, 65, 257, 1024):
        sums, used = _random_ids(n, 200 + n)
        if n >= 2:
            used = np.maximum(used, 3)                                          # every id votes: n voters

        def force(ids, model, n=n):
            assert len(ids) == n and model[0]["voters"] == (n if n >= 2 else int(n == 1 and ids[0]["used"] >= 3))
            assert bool(model[0]["flags"] & KR.MODEL_SINGLE) == (n < 2)
            if n >= 63:
                assert (ids["team"] == 0).sum() > n // 4 and (ids["team"] == 1).sum() > n // 4
        _add(_ids_case(f"ids_{n}", sums, used), force)

    # A, A', B, B' with A = A' and B = B': the pairs (0, 2), (0, 3), (1, 2), (1, 3) all cost 0
    def force(ids, model):
        assert (model[0]["a"], model[0]["b"], model[0]["cost"]) == (0, 2, 0) and [int(t) for t in ids["team"]] == [0, 0, 1, 1]
    _add(_ids_case("two_pairs_of_equal_cost", [_row(b3=100), _row(b3=200), _row(b20=50), _row(b20=70)], [3, 3, 3, 3]), force)

    def force(ids, model):
        assert (model[0]["a"], model[0]["b"]) == (0, 1) and ids[2]["d"][0] == ids[2]["d"][1] == 65536 and ids[2]["team"] == 0 and ids[2]["flags"] == KR.ID_WEAK
    _add(_ids_case("an_id_equidistant_from_both_medoids", [_row(b0=4), _row(b1=4), _row(b0=2, b1=2)], [50, 40, 1], outlier=0), force)

    def force(ids, model):
        assert model[0]["dab"] == 0 and model[0]["cost"] == 0 and (model[0]["a"], model[0]["b"]) == (0, 1) and (ids["team"] == 0).all() and model[0]["w"][1] == 0
    _add(_ids_case("all_signatures_identical", [_row(b5=3 * k, b31=k) for k in range(1, 6)], [3, 4, 5, 6, 7]), force)

    def force(ids, model):
        assert model[0]["w"][0] == model[0]["w"][1] == 3 and model[0]["team_of_a"] == 0 and [int(t) for t in ids["team"]] == [0, 1]
    _add(_ids_case("clusters_of_equal_weight", [_row(b2=9), _row(b17=9)], [3, 3]), force)

    def force(ids, model):
        assert model[0]["team_of_a"] == 1 and model[0]["flags"] == KR.MODEL_SWAPPED and [int(t) for t in ids["team"]] == [1, 0, 0] and ids[0]["d"][1] == 0
        assert (model[0]["w"][0], model[0]["w"][1]) == (9, 3)
    _add(_ids_case("team_0_is_the_heavier_cluster_of_b", [_row(b2=9), _row(b17=9), _row(b17=8, b18=1)], [3, 4, 5]), force)

    def force(ids, model):
        assert model[0]["voters"] == 1 and model[0]["flags"] == KR.MODEL_SINGLE and model[0]["w"][0] == 5 and model[0]["a"] == -1
        assert [int(t) for t in ids["team"]] == [0, 0, -1, 0] and [int(f) for f in ids["flags"]] == [KR.ID_SINGLE | KR.ID_WEAK, KR.ID_SINGLE, 0, KR.ID_SINGLE | KR.ID_WEAK]
    _add(_ids_case("exactly_one_voter", [_row(b2=9), _row(b17=9), _row(), _row(b30=1)], [2, 5, 0, 1]), force)

    def force(ids, model):
        assert model[0]["voters"] == 0 and [int(t) for t in ids["team"]] == [0, 0] and (ids["flags"] == (KR.ID_SINGLE | KR.ID_WEAK)).all()
    _add(_ids_case("no_voter", [_row(b2=9), _row(b17=9)], [2, 1]), force)

    # T = 65536 makes p the sums themselves: a = (65536, 0, 0), b = (0, 65536, 0), D(a, b) = 131072; x lies 65536 from a, exactly half: not neither;
    # y lies 65538 from a, the least step beyond (moving one unit of p from one bin to another moves D by 2): neither
    rows = [_row(b0=65536), _row(b1=65536), _row(b0=32768, b2=32768), _row(b0=32767, b2=32769)]

    def force(ids, model):
        assert (model[0]["a"], model[0]["b"], model[0]["dab"]) == (0, 1, 131072) and ids[2]["d"][0] == 65536 and ids[3]["d"][0] == 65538
        assert [int(t) for t in ids["team"]] == [0, 1, 0, -1] and ids[3]["flags"] == KR.ID_NEITHER and model[0]["neither"] == 1
    _add(_ids_case("an_id_at_the_outlier_bound_and_one_beyond", rows, [100, 100, 3, 3]), force)

    def force(ids, model):
        assert [int(t) for t in ids["team"]] == [0, 1, 0, 0] and model[0]["neither"] == 0
    _add(_ids_case("outlier_0_turns_the_rule_off", rows, [100, 100, 3, 3], outlier=0), force)

    def force(ids, model):
        assert model[0]["voters"] == 2 and [int(f) for f in ids["flags"]] == [0, 0, KR.ID_WEAK, KR.ID_WEAK, 0] and [int(t) for t in ids["team"]] == [0, 1, 0, 1, -1]
    _add(_ids_case("ids_with_1_or_2_crops_are_weak", [_row(b9=10, b33=1), _row(b24=10, b33=1), _row(b9=9, b33=2), _row(b24=9, b33=2), _row()], [5, 4, 1, 2, 0]), force)

    big = [_row(b0=KR.MAX_SUM), _row(b1=KR.MAX_SUM, b2=KR.MAX_SUM), _row(b0=KR.MAX_SUM, b1=1)]

    def force(ids, model):
        assert model[0]["cost"] < 1 << 39 and ids[0]["p"][0] == 65536 and ids[1]["p"][1] == 32768 and [int(t) for t in ids["team"]] == [0, 1, 0]
    _add(_ids_case("the_greatest_sums_and_weights", big, [KR.MAX_CROPS // 2, KR.MAX_CROPS // 4, KR.MAX_CROPS // 4]), force)


# ---- seeded clips -------------------------------------------------------------------------------------------------------------------------------
NAVY, SKY, YELLOW, SKIN = (125, 44, 22), (235, 170, 90), (30, 210, 230), (150, 170, 200)


def kit_clip(kits, per_kit, crops_each, seed, extra=(), stripes=None):
    """-> (frames, coords, truth {id: kit index}): ids 1 .. of 12 x 30 boxes on noisy grass, four to a frame.  In every box: a head of skin, the shirt in
    the kit's colour at a brightness gain of 0.8 .. 1.15 per crop with noise (shorts alike), a fifth of the pixels below the head grass and a twelfth skin.
    extra: further ids, one each, with the colours given; stripes: kit index -> a second colour on every other pair of columns"""
    r = np.random.default_rng(seed)
    colours = [(k, c) for k, c in enumerate(kits) for _ in range(per_kit)] + [(len(kits) + j, c) for j, c in enumerate(extra)]
    crops_of = [crops_each[k] if isinstance(crops_each, (list, tuple)) else crops_each for k in range(len(colours))]
    jobs = [pid for pid in range(len(colours)) for _ in range(crops_of[pid])]
    r.shuffle(jobs)
    groups = []                                                                 # four boxes to a frame, an id at most once in a frame
    for pid in jobs:
        for g in groups:
            if len(g) < 4 and pid not in g:
                g.append(pid)
                break
        else:
            groups.append([pid])
    frames, coords = [], {}
    for group in groups:
        f = np.clip(np.array(GRASS)[None, None] + r.integers(-8, 9, (FH, FW, 3)), 0, 255).astype(np.uint8)
        players = {}
        for k, pid in enumerate(group):
            x1, y1 = 6 + 22 * k + int(r.integers(0, 4)), 10 + int(r.integers(0, 20))
            gain = r.uniform(0.8, 1.15)
            box = f[y1:y1 + 30, x1:x1 + 12]
            kit, colour = colours[pid]
            body = np.tile(np.array(colour, np.float64), (30, 12, 1))
            if stripes and kit in stripes:
                body[:, (np.arange(12) // 2) % 2 == 1] = stripes[kit]
            body = body * gain + r.integers(-6, 7, (30, 12, 3))
            body[:5] = np.array(SKIN) + r.integers(-6, 7, (5, 12, 3))
            mix = r.uniform(0, 1, (30, 12))
            body[(mix < 0.08) & (np.arange(30)[:, None] < 16)] = SKIN
            keep = ((mix < 0.8) | (np.arange(30)[:, None] < 5)) & (np.abs(2 * np.arange(12)[None, :] - 11) < 8)    # the body: columns 2 .. 9, grass beside it
            keep &= (np.arange(30)[:, None] >= 5) | (np.abs(2 * np.arange(12)[None, :] - 11) < 4)                      # the head: columns 4 .. 7
            box[keep] = np.clip(body, 0, 255).astype(np.uint8)[keep]
            players[pid + 1] = {"BBox": [x1, y1, x1 + 12, y1 + 30]}
        frames.append(f)
        coords[len(frames) - 1] = {"Coordinates": {"Player": players}}
    return np.stack(frames), coords, {pid + 1: kit for pid, (kit, _) in enumerate(colours)}


def clip_case(name, frames, coords, **p):
    from eagle_amd import kits
    crops, slots, slot_ids = kits.crop_list(coords, len(frames))
    return dict(name=name, kind="pixels", frames=frames, crops=crops, slots=slots, n_ids=len(slot_ids), p=p, coords=coords, slot_ids=slot_ids)


def _split_is(ids, slot_ids, truth, kits=(0, 1)):
    m = KR.mapping_of(ids, slot_ids)
    teams = {k: {m.get(pid) for pid, kit in truth.items() if kit == k} for k in kits}
    return all(len(t) == 1 and None not in t for t in teams.values()) and teams[kits[0]] != teams[kits[1]]


@functools.lru_cache(None)
def two_blues(referee=False):
    return kit_clip([NAVY, SKY], 10, 6, 11, extra=(YELLOW,) if referee else ())


def _clips():
    frames, coords, truth = two_blues()

    def force(crops, ids, model, truth=truth):
        slot_ids = BY_NAME["two_blues"]["slot_ids"]
        assert len(ids) == 20 and model[0]["voters"] == 20 and model[0]["neither"] == 0 and _split_is(ids, slot_ids, truth)
        same = max(int(r["d"][r["team"]]) for r in ids)
        print("two blues: distance between the medoids", int(model[0]["dab"]), "greatest distance to the own medoid", same)
        assert same * 4 < model[0]["dab"]
    _add(clip_case("two_blues", frames, coords), force)

    frames, coords, truth = two_blues(True)

    def force(crops, ids, model, truth=truth):
        slot_ids = BY_NAME["two_blues_and_a_yellow_referee"]["slot_ids"]
        ref = ids[slot_ids.index(21)]
        assert _split_is(ids, slot_ids, truth) and ref["team"] == -1 and ref["flags"] & KR.ID_NEITHER and model[0]["neither"] == 1
        far = max(int(r["d"][r["team"]]) for r in ids if r["team"] >= 0)                                # the players stay well inside the bound he is beyond
        assert far * 1024 * 2 < 512 * int(model[0]["dab"]) < min(int(ref["d"][0]), int(ref["d"][1])) * 1024
    _add(clip_case("two_blues_and_a_yellow_referee", frames, coords), force)

    frames, coords, truth = kit_clip([NAVY, SKY], 4, [6, 6, 1, 2, 6, 6, 2, 1], 13)

    def force(crops, ids, model, truth=truth):
        slot_ids = BY_NAME["two_blues_with_weak_ids"]["slot_ids"]
        weak = {pid for pid, r in zip(slot_ids, ids) if r["flags"] & KR.ID_WEAK}
        assert weak == {3, 4, 7, 8} and model[0]["voters"] == 4 and _split_is(ids, slot_ids, truth)
    _add(clip_case("two_blues_with_weak_ids", frames, coords, outlier=0), force)

    frames, coords, truth = kit_clip([(240, 240, 240), (240, 240, 240)], 5, 5, 17, stripes={0: (40, 40, 215)})

    def force(crops, ids, model, truth=truth):
        assert _split_is(ids, BY_NAME["red_and_white_stripes_against_white"]["slot_ids"], truth)
    _add(clip_case("red_and_white_stripes_against_white", frames, coords, outlier=0), force)


_sizes()
_pixels()
_counts()
_ids()
_clips()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PIXEL_CASES = [c["name"] for c in CASES if c["kind"] == "pixels"]
ID_CASES = [c["name"] for c in CASES if c["kind"] == "ids"]


@functools.lru_cache(None)
def reference(name, loop=False):
    """the contract's output for a case, computed once: (crops, ids, model) or, for an ids case, (ids, model)"""
    c = BY_NAME[name]
    if c["kind"] == "ids":
        return (KR.cluster_ids_loop if loop else KR.cluster_ids)(c["sums"], c["used"], None, **c["p"])
    return KR.team_cluster(c["frames"], c["crops"], c["slots"], c["n_ids"], loop=loop, **c["p"])


# (what, changes to the call of eagle_op_team_cluster_ids on "clusters_of_equal_weight") and the same for eagle_op_team_cluster on "window_all_grass"
ID_REFUSALS = [("ids_1025", dict(n_ids=1025)), ("ids_negative", dict(n_ids=-1)), ("min_pixels_0", dict(p=dict(min_pixels=0))), ("min_pixels_above", dict(p=dict(min_pixels=(1 << 20) + 1))),
               ("min_crops_0", dict(p=dict(min_crops=0))), ("min_crops_above", dict(p=dict(min_crops=(1 << 16) + 1))), ("outlier_negative", dict(p=dict(outlier=-1))),
               ("outlier_above", dict(p=dict(outlier=(1 << 20) + 1))), ("reserved_word", dict(reserved=2)), ("params_null", dict(par=False)), ("sums_null", dict(sums=None)),
               ("used_null", dict(used=None)), ("used_negative", dict(used0=-1)), ("used_above", dict(used0=(1 << 22) + 1)), ("sum_negative", dict(sum0=-1)),
               ("sum_above", dict(sum0=(1 << 34) + 1)), ("crops_without_colour", dict(zero_row=0)),
               ("crops_in_all_above", dict(used_all=(1 << 21) + 1))]
PIXEL_REFUSALS = [("ids_1025", dict(n_ids=1025)), ("crops_above", dict(n_crops=(1 << 22) + 1)), ("crops_negative", dict(n_crops=-1)), ("slot_n_ids", dict(slot0=2)),
                  ("slot_negative", dict(slot0=-1)), ("min_pixels_0", dict(p=dict(min_pixels=0))), ("outlier_above", dict(p=dict(outlier=(1 << 20) + 1))),
                  ("params_null", dict(par=False)), ("crops_null", dict(crops=None)), ("slots_null", dict(slots=None)), ("frames_null", dict(frames=None)),
                  ("frame_height_0", dict(h=0))]
