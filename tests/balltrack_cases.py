"""Constructed clips for the ball track (tests/balltrack_ref.py is the contract; shared by the CPU and the GPU tests).  A case: counts per frame,
positions in half pixels and cq per candidate (flat, frame after frame, descending confidence), cuts, and the parameters as the C ABI takes them
(fps, frame_w, speed / reward / brk in pixels and gap in frames, 0: the default).  Each case is named after what it forces; FORCES holds, per name,
the property the CPU test asserts on the contract's result so that the name stays true.  Seeded where random."""
import functools

import numpy as np

import balltrack_ref as BR

PARTS = ("frames", "tracklets", "clip")


def _case(name, frames, cuts=(), det=None, **p):
    """frames: per frame a list of (qx, qy, cq)"""
    counts = np.array([len(f) for f in frames], np.int32)
    flat = [c for f in frames for c in f]
    pos = np.array([(c[0], c[1]) for c in flat], np.int32).reshape(-1, 2)
    cq = np.array([c[2] for c in flat], np.int32)
    par = dict(fps=25, frame_w=1280, speed=0.0, gap=0, reward=0.0, brk=0.0)
    par.update(p)
    return dict(name=name, counts=counts, pos=pos, cq=cq, cuts=list(cuts), det=det, p=par)


def _walk(n, x0=600, y0=400, dx=6, dy=2, cq=1024):
    return [[(x0 + dx * i, y0 + dy * i, cq)] for i in range(n)]


def sum_of_two_squares_below(k2):
    """the greatest d2 < k2 that is dx^2 + dy^2 (k^2 - 1 itself is none for k = 2, 255, 256, 65535: a prime 3 mod 4 divides it to an odd power)"""
    best = (0, 0, 0)
    for dy in range(0, 4000):
        if dy * dy >= k2:
            break
        dx = BR.isqrt(k2 - 1 - dy * dy)
        if dx * dx + dy * dy > best[0]:
            best = (dx * dx + dy * dy, dx, dy)
    return best


def _jump(name, dx, dy):
    """twenty sightings at one point pay for the break, the ball then jumps by (dx, dy) over two frames and is seen three times more: the track's length is
    isqrt(dx^2 + dy^2)"""
    frames = [[(0, 0, 1024)] for _ in range(20)] + [[]] + [[(dx, dy, 1024)] for _ in range(3)]
    return _case(name, frames, speed=65535.0, reward=65535.0, brk=float(1 << 20), gap=2)


def _cases():
    out = []
    for n in (0, 1, 2, 3):
        out.append(_case(f"n_{n}", _walk(n, dx=10, dy=0)))
    far = lambda i, count: [(5000 * (k + 1) + 900 * i, 1200, 1024 - k) for k in range(count)]     # confident, and never twice within V of one another
    out.append(_case("candidates_0", [[] for _ in range(5)]))
    out.append(_case("candidates_1", _walk(5)))
    out.append(_case("candidates_2", [f + [(40, 30, 700)] for f in _walk(5)]))
    out.append(_case("candidates_8", [far(i, 7) + [(600 + 6 * i, 400, 1000)] for i in range(5)]))
    out.append(_case("candidates_9_the_ninth_is_the_ball", [far(i, 8) + [(600 + 6 * i, 400, 1000)] if i == 2 else [(600 + 6 * i, 400, 1024)] for i in range(5)]))
    for g, name in ((3, "gap_of_G"), (4, "gap_of_G_plus_1")):
        w = _walk(4 + g + 3)
        out.append(_case(name, [f if i < 4 or i >= 4 + g - 1 else [] for i, f in enumerate(w)], gap=3))
    for extra, name in ((0, "step_of_exactly_V"), (1, "step_of_V_and_a_half_pixel")):
        # V = 20 half pixels; the third sighting lies 2 frames and 40 (+ 1) half pixels behind the second
        out.append(_case(name, [[(100, 100, 1024)], [(100, 100, 1024)], [(100, 100, 1024)], [], [(140 + extra, 100, 1024)], [(140 + extra, 100, 1024)], [(140 + extra, 100, 1024)]],
                         speed=10.0, reward=40.0, brk=50.0, gap=4))
    for k in (1, 2, 255, 256, 65535):
        _, dx, dy = sum_of_two_squares_below(k * k)
        out.append(_jump(f"d2_below_{k}_squared", dx, dy))
        out.append(_jump(f"d2_{k}_squared", k, 0))
        out.append(_jump(f"d2_{k}_squared_plus_1", k, 1))
    out.append(_jump("d2_largest", BR.MAX_Q, BR.MAX_Q))
    out.append(_case("cq_0_1023_1024", [[(600, 400, 1024)], [(602, 400, 1024)], [(604, 400, 1024)], [(606, 400, 0)], [(608, 400, 1023)], [(610, 400, 1024)]]))
    out.append(_case("singleton_R_equals_B", [[], [(300, 300, 1024)], []], reward=10.0, brk=10.0))
    out.append(_case("singleton_R_is_B_plus_1", [[], [(300, 300, 1024)], []], reward=10.5, brk=10.0))
    # two sightings 30 half pixels apart, B = 30: the link costs what the break costs and is taken
    out.append(_case("link_costs_exactly_B", [[(100, 100, 1024)], [(130, 100, 1024)]], speed=50.0, reward=100.0, brk=15.0))
    out.append(_case("link_costs_B_plus_1", [[(100, 100, 1024)], [(131, 100, 1024)]], speed=50.0, reward=100.0, brk=15.0))
    # two paths, mirror images about y = 400, of equal confidence: every comparison ties
    out.append(_case("mirror_images", [[(600 + 6 * i, 400 - 10 - i, 800), (600 + 6 * i, 400 + 10 + i, 800)] for i in range(7)]))
    out.append(_case("mirror_images_crossing_gaps", [[(600 + 6 * i, 390, 800), (600 + 6 * i, 410, 800)] if i % 3 != 1 else [] for i in range(9)], gap=2))
    for g in (1, 64):
        for n in (g + 1, 2 * g + 3):
            out.append(_case(f"ring_wrap_G_{g}_n_{n}", _walk(n, dx=2, dy=1), gap=g, brk=50.0))
    out.append(_case("ring_wrap_G_64_two_candidates", [[(600 + 2 * i, 400 + (i % 5), 900), (40 + (i * 7) % 50, 30, 1000)] for i in range(140)], gap=64))
    for run, name in ((4, "empty_run_of_G_minus_1"), (5, "empty_run_of_G")):
        w = _walk(5 + run + 5)
        out.append(_case(name, [f if i < 5 or i >= 5 + run else [] for i, f in enumerate(w)], gap=5))
    out.append(_case("cut_at_1", _walk(8), cuts=[1]))
    out.append(_case("cut_at_n_minus_1", _walk(8), cuts=[7]))
    out.append(_case("cuts_back_to_back", _walk(10), cuts=[4, 5]))
    out.append(_case("cut_inside_a_perfect_link", _walk(8, dx=0, dy=0), cuts=[4]))
    out.append(_case("segments_300", [([(600 + 4 * (i % 6), 400, 1024)] if i % 6 < 4 else []) for i in range(1800)], gap=2))
    r = np.random.default_rng(35)
    path = np.cumsum(r.integers(-30, 31, (5000, 2)), 0) + (60000, 60000)
    frames = []
    for i in range(5000):
        k = int(r.integers(1, 4))
        c = [(int(path[i, 0] + r.integers(-3, 4)), int(path[i, 1] + r.integers(-3, 4)), int(r.integers(300, 1025)))]
        c += [(int(r.integers(0, 2561)), int(r.integers(0, 1441)), int(r.integers(300, 1025))) for _ in range(k - 1)]
        frames.append(sorted(c, key=lambda v: -v[2]))
    out.append(_case("one_segment_of_5000_random_frames", frames, gap=8))
    out.append(_case("distractor_in_every_frame", [[(600 + 8 * i, 1000 + 3 * i + (600 if i % 2 else -600), 1000), (600 + 8 * i, 1000 + 3 * i, 800)] for i in range(40)]))
    # small random clips: every choice of them is enumerated
    for k in range(28):
        n = int(r.integers(2, 7))
        frames = [[(int(r.integers(0, 60)), int(r.integers(0, 60)), int(r.integers(0, 1025))) for _ in range(int(r.integers(0, 4)))] for _ in range(n)]
        frames = [sorted(f, key=lambda v: -v[2]) for f in frames]
        cuts = sorted(set(int(c) for c in r.integers(1, n, int(r.integers(0, 3))))) if n > 1 else []
        out.append(_case(f"small_random_{k}", frames, cuts=cuts, speed=float(r.choice([5.0, 10.0, 20.0])), reward=float(r.choice([10.0, 25.0])),
                         brk=float(r.choice([0.5, 2.5, 12.5, 37.5])), gap=int(r.integers(1, 4))))
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SMALL = [c["name"] for c in CASES if len(c["counts"]) <= 6 and (len(c["counts"]) == 0 or c["counts"].max() <= 3)]


def resolved(c):
    return BR.resolve(**c["p"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(frames, tracklets, clip) of the contract, computed once and shared; read only"""
    c = BY_NAME[name]
    out = BR.track_window(c["counts"], c["pos"], c["cq"], *resolved(c), cuts=c["cuts"], det=c["det"])
    for a in out:
        a.setflags(write=False)
    return out


def _one_track(length=None, sightings=None, lone=None):
    """lone: the frame whose one sighting the cut leaves without a track"""
    def check(fr, tr, clip):
        assert len(tr) == 1 and (length is None or tr[0]["length"] == length) and (sightings is None or tr[0]["sightings"] == sightings), tr
        assert lone is None or fr[lone]["cand"] == -1
    return check


def _eighth(fr, tr, clip):
    assert (fr["cand"] == 7).all() and not (fr["flags"] & BR.TOO_MANY).any() and clip[0]["ignored"] == 0


def _back_to_back(fr, tr, clip):
    assert len(tr) == 2 and fr[4]["cand"] == -1 and fr[4]["flags"] & BR.SHOT_START and fr[5]["flags"] & BR.SHOT_START and clip[0]["shots"] == 3


def _long(fr, tr, clip):
    assert clip[0]["frames_chosen"] > 4096 and tr["sightings"].max() > 4096                  # a chain of more than 2^12 predecessors


def _tracks(k):
    def check(fr, tr, clip):
        assert len(tr) == k and clip[0]["tracklets"] == k, tr
    return check


def _ninth(fr, tr, clip):
    assert fr[2]["flags"] & BR.TOO_MANY and fr[2]["cand"] == -1 and clip[0]["ignored"] == 1 and clip[0]["rejected"] == 8
    assert len(tr) == 1 and tr[0]["sightings"] == 4                     # (the track steps over the frame: 12 half pixels in two frames)


def _mirror(fr, tr, clip):
    assert (fr["cand"][fr["cand"] >= 0] == 0).all() and len(tr) == 1 and clip[0]["frames_chosen"] == clip[0]["frames_with"]


def _distractor(fr, tr, clip):
    assert (fr["cand"] == 1).all() and len(tr) == 1


def _cq(fr, tr, clip):
    assert len(tr) == 1 and tr[0]["sightings"] == 6 and tr[0]["sum_cq"] == 4 * 1024 + 1023 and tr[0]["gain"] == 4 * 256 + 255 - 10 - 640


def _second_rejected(fr, tr, clip):
    assert (fr["cand"] == 0).all() and clip[0]["rejected"] == 5 and clip[0]["frames_multi"] == 5 and len(tr) == 1


FORCES = {"candidates_2": _second_rejected, "ring_wrap_G_64_two_candidates": _one_track(None, 140), "n_0": _tracks(0), "n_1": _tracks(0), "n_2": _tracks(0), "n_3": _one_track(20, 3), "candidates_0": _tracks(0), "candidates_1": _one_track(None, 5),
          "candidates_8": _eighth,
          "candidates_9_the_ninth_is_the_ball": _ninth, "gap_of_G": _tracks(1), "gap_of_G_plus_1": _tracks(2), "step_of_exactly_V": _one_track(40, 6),
          "step_of_V_and_a_half_pixel": _tracks(2), "d2_largest": _one_track(BR.isqrt(2 * BR.MAX_Q ** 2), 23), "cq_0_1023_1024": _cq,
          "singleton_R_equals_B": _tracks(0), "singleton_R_is_B_plus_1": _one_track(0, 1), "link_costs_exactly_B": _one_track(30, 2), "link_costs_B_plus_1": _tracks(2),
          "mirror_images": _mirror, "mirror_images_crossing_gaps": _mirror, "empty_run_of_G_minus_1": _tracks(1), "empty_run_of_G": _tracks(2),
          "cut_at_1": _one_track(None, 7, 0), "cut_at_n_minus_1": _one_track(None, 7, 7), "cuts_back_to_back": _back_to_back,
          "cut_inside_a_perfect_link": _tracks(2), "segments_300": _tracks(300), "distractor_in_every_frame": _distractor,
          "one_segment_of_5000_random_frames": _long}
for _k in (1, 2, 255, 256, 65535):
    FORCES[f"d2_below_{_k}_squared"] = _one_track(_k - 1, 23)
    FORCES[f"d2_{_k}_squared"] = _one_track(_k, 23)
    FORCES[f"d2_{_k}_squared_plus_1"] = _one_track(_k, 23)
for _g in (1, 64):
    for _n in (_g + 1, 2 * _g + 3):
        FORCES[f"ring_wrap_G_{_g}_n_{_n}"] = _one_track(None, _n)

# what eagle_op_ball_track refuses: name -> changes to the arguments of the call (tests/test_gpu_balltrack.py applies them)
REFUSALS = [("params NULL", dict(par=None)), ("counts NULL", dict(counts=None)), ("positions NULL", dict(pos=None)), ("no confidences", dict(cq=None)),
            ("cuts NULL with n_cuts", dict(cuts=None, n_cuts=1)), ("n < 0", dict(n=-1)), ("n > 2^20", dict(n=(1 << 20) + 1)), ("n_cuts < 0", dict(n_cuts=-1)),
            ("count < 0", dict(count0=-1)), ("count beyond the range", dict(count0=301)), ("cut 0", dict(cuts=[0])), ("cut n", dict(cuts=["n"])), ("cuts unsorted", dict(cuts=[3, 2])),
            ("cuts repeated", dict(cuts=[2, 2])), ("gap -1", dict(p=dict(gap=-1))), ("gap 65", dict(p=dict(gap=65))), ("fps 0", dict(p=dict(fps=0))),
            ("frame_w 0", dict(p=dict(frame_w=0))), ("speed nan", dict(p=dict(speed=float("nan")))), ("speed < 0", dict(p=dict(speed=-1.0))),
            ("speed > 65535", dict(p=dict(speed=65535.5))), ("reward inf", dict(p=dict(reward=float("inf")))), ("reward < 0", dict(p=dict(reward=-0.5))),
            ("reward > 65535", dict(p=dict(reward=65536.0))), ("break nan", dict(p=dict(brk=float("nan")))), ("break < 0", dict(p=dict(brk=-2.0))),
            ("break > 2^20", dict(p=dict(brk=float((1 << 20) + 1)))), ("reserved word", dict(reserved=3)), ("max_bytes too small", dict(p=dict(max_bytes=64))),
            ("qx < 0", dict(pos0=(-1, 0))), ("qy beyond 131070", dict(pos0=(0, 131071))), ("cq 1025", dict(cq0=1025)), ("cq -1", dict(cq0=-1)),
            ("conf nan", dict(conf0=float("nan"))), ("conf 1.5", dict(conf0=1.5)), ("conf -0.1", dict(conf0=-0.1)), ("recover 3", dict(recover=3))]
