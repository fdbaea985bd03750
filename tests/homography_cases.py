"""Constructed inputs for find_homography_block (csrc/geom.hip), the workgroup restatement of cv2.findHomography(RANSAC): subset sampler, attempt chain,
256 four-point models per round, the one-wave replay with its three events — (A) a new best model, (B) the iteration bound reached, (C) the 1000th
consecutive rejected subset — then the all-inlier Jacobi DLT and the LM polish.  Shared by tests/test_homography_cases_cpu.py, which proves through the
oracle's trace (oracle.prims.find_homography_ransac_trace) that every case forces what its name says, and tests/test_gpu_homography.py, which requires the
kernel's result to equal the oracle's bit for bit.  Pure numpy, every seed fixed; the seeds were found on the CPU with the trace.

Vocabulary, as in the trace: an ATTEMPT is one drawn subset of four (numbered from 0 over the call); a counted ITERATION is an attempt whose subset passed
cv2's checkSubset; a DRAW is one output of cv::RNG(-1).  The kernel reads the first TABLE = 65536 draws from a table and generates the rest itself; it works
in ROUNDS of at most 256 attempts that start inside a window of 1536 draws, and replays a round 64 attempts (one per lane) at a time: rounds_of() restates
that partition, which depends on the point count alone.

All inputs are finite.  NaN and infinite coordinates are out of scope: the reference does not define what they give.

Searched for and not found:
  * a subset that passes checkSubset and whose 4-point solve then fails (code 254 in the kernel): none in 4060 inputs of the families below (garbage, near-line,
    exact-line, camera with outliers; 3.3 million counted iterations together, 8 s of CPU), none in the cases kept here.  checkSubset's collinearity test rejects what would make the 8 x 8 system
    singular before the solver sees it; the path is not reached by these tests."""
import numpy as np

TABLE = 65536
ROUND_ATTEMPTS, ROUND_WINDOW, LANES = 256, 1536, 64
MAX_KP = 87
END_BOUND, END_REJECT_ITER0, END_REJECT_LATER, END_NITERS_ZERO, END_NO_LOOP = range(5)


# ======================================================================================================================
# the sampler's partition of the stream (no data involved)
# ======================================================================================================================
def rng_stream(count):
    """the first `count` outputs of cv::RNG(-1) (multiply-with-carry, multiplier 4164903690)"""
    out = np.empty(count, np.uint32)
    st = 0xffffffffffffffff
    for i in range(count):
        st = (st & 0xffffffff) * 4164903690 + (st >> 32)
        out[i] = st & 0xffffffff
    return out


def attempt_starts(n, attempts):
    """draw position at which each of the first `attempts` attempts starts, for n points (getSubset: draw until four distinct indices), plus the end"""
    starts = np.empty(attempts + 1, np.int64)
    stream = rng_stream(int(attempts * (8 if n > 8 else 40)) + 64) % np.uint32(n)
    j = 0
    for a in range(attempts):
        starts[a] = j
        got = []
        while len(got) < 4:
            v = int(stream[j]); j += 1
            if v not in got:
                got.append(v)
    starts[attempts] = j
    return starts


def rounds_of(n, attempts):
    """(round, ordinal in the round) of each of the first `attempts` attempts: a round takes the attempts that start within ROUND_WINDOW draws of its first
    one, ROUND_ATTEMPTS at the most"""
    starts = attempt_starts(n, attempts)
    out = np.empty((attempts, 2), np.int64)
    rnd, first = 0, 0
    for a in range(attempts):
        if a - first == ROUND_ATTEMPTS or starts[a] - starts[first] >= ROUND_WINDOW:
            rnd += 1; first = a
        out[a] = (rnd, a - first)
    return out


# ======================================================================================================================
# point families
# ======================================================================================================================
def _project(Hm, pts):
    p = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ Hm.T
    return p[:, :2] / p[:, 2:3]


def broadcast_camera(seed):
    """pitch metres -> 1280 x 720 pixels: a broadcast view with a perspective term in y (the far touch-line is narrower)"""
    r = np.random.default_rng([seed, 77])
    cx, zoom, tilt = 52.5 + 18.0 * r.uniform(-1, 1), 13.0 + 3.0 * r.uniform(-1, 1), 0.0045 + 0.001 * r.uniform(-1, 1)
    return np.array([[zoom, 0.35 * zoom, 640.0 - zoom * cx - 0.35 * zoom * 34.0],
                     [0.0, -0.62 * zoom, 400.0 + 0.62 * zoom * 34.0],
                     [0.0, tilt, 1.0 - tilt * 34.0]], np.float64)


def near_affine_camera():
    """perspective terms of 1e-9 per metre: H's third row is (tiny, tiny, 1), the DLT's null vector is all but an affine map"""
    return np.array([[11.0, 1.5, 60.0], [-0.8, 9.5, 40.0], [1e-9, -2e-9, 1.0]], np.float64)


def steep_camera():
    """strong perspective: the homogeneous weight falls from 1 at y = 0 to 0.048 at y = 68 (objects at the far line are 21 times smaller); the horizon
    (weight 0) lies at y = 71.4, outside the pitch, so every point is finite"""
    return np.array([[14.0, 3.0, -80.0], [0.0, -1.5, 700.0], [0.0, -0.014, 1.0]], np.float64)


def landmark_points(seed, noise=0.0, n_out=0, scale=1.0):
    """the pitch's on-plane landmarks seen by broadcast_camera(seed) inside a (1280 x 720) * scale image, floored to pixels after Gaussian noise of `noise`
    pixels (times scale), with n_out of them moved to uniform positions"""
    from eagle_amd.pitch import LANDMARKS, on_plane_mask
    rng = np.random.default_rng(seed)
    m = on_plane_mask()
    world = np.array([[x, y] for (i, _, x, y, z) in LANDMARKS if m[i]], np.float64)
    img = _project(broadcast_camera(seed), world) * scale
    keep = (img[:, 0] >= 0) & (img[:, 0] < 1280 * scale) & (img[:, 1] >= 0) & (img[:, 1] < 720 * scale)
    img, world = img[keep], world[keep]
    img = np.floor(img + rng.normal(0, noise * scale, img.shape))
    for k in rng.choice(len(img), size=min(n_out, len(img)), replace=False):
        img[k] = rng.uniform(0, 700 * scale, 2)
    return img.astype(np.float32), world.astype(np.float32)


def scattered_points(seed, n, noise=0.0, n_out=0, cam=None, snap=0.0):
    """n uniform pitch positions (no three collinear, unlike the landmarks) seen by one camera, sub-pixel image coordinates (multiples of `snap` if given)
    with Gaussian noise, n_out of them moved to uniform positions: a smooth orientation-preserving map, so that checkSubset rejects next to nothing"""
    rng = np.random.default_rng(seed)
    Hm = broadcast_camera(seed) if cam is None else cam
    world = np.empty((0, 2)); img = np.empty((0, 2))
    while len(world) < n:
        w = rng.uniform((0, 0), (105, 68), (4 * n, 2))
        p = _project(Hm, w)
        keep = (p[:, 0] >= 0) & (p[:, 0] < 1280) & (p[:, 1] >= 0) & (p[:, 1] < 720)
        world = np.concatenate([world, w[keep]]); img = np.concatenate([img, p[keep]])
    world, img = world[:n], img[:n]
    img = img + rng.normal(0, noise, img.shape)
    if snap:
        img = np.floor(img / snap) * snap
    for k in rng.choice(n, size=min(n_out, n), replace=False):
        img[k] = rng.uniform(0, 700, 2)
    return img.astype(np.float32), world.astype(np.float32)


def garbage_points(seed, n):
    """uniform integer pixels against uniform pitch positions: no consensus, about three subsets in four fail checkSubset's orientation test"""
    rng = np.random.default_rng(seed)
    img = np.floor(rng.uniform(0, 1280, (n, 2))).astype(np.float32)
    world = rng.uniform(0, 105, (n, 2)).astype(np.float32)
    return img, world


def near_line_points(seed):
    """15 to 49 image points within half a pixel of one line plus 2 to 5 off it, against uniform pitch positions: most subsets have three near-collinear
    points that checkSubset ACCEPTS only now and then, so 2000 counted iterations cost 60 to 130 thousand draws"""
    rng = np.random.default_rng(seed)
    n_line = int(rng.integers(15, 50)); n_off = int(rng.integers(2, 6))
    t = np.sort(rng.uniform(0, 1200, n_line))
    img = np.stack([t, 0.5 * t + 30], 1)
    off = rng.uniform(0, 700, (n_off, 2))
    img = np.floor(np.concatenate([img, off]) * 2) / 2
    world = rng.uniform(0, 105, (len(img), 2))
    return img.astype(np.float32), world.astype(np.float32)


def exact_line_points(seed, n_line, n_off):
    """n_line integer image points EXACTLY on y = x + 30 plus n_off off it: a subset passes only with at most two points of the line, so runs of a thousand
    rejected subsets happen (event (C))"""
    rng = np.random.default_rng(seed * 100 + n_line)
    t = np.sort(rng.choice(1200, n_line, replace=False)).astype(float)
    img = np.stack([t, t + 30], 1)
    off = np.floor(rng.uniform(0, 700, (n_off, 2)))
    img = np.concatenate([img, off])
    world = rng.uniform(0, 105, (len(img), 2))
    return img.astype(np.float32), world.astype(np.float32)


# ======================================================================================================================
# the solver inside post_kernel: image points as heat-map maxima of on-plane landmarks
# ======================================================================================================================
HM = (135, 240)
FRAME = (720, 1280)


def plane_channels():
    from eagle_amd.pitch import LANDMARKS, NOT_ON_PLANE
    return [i for i, _, x, y, z in LANDMARKS if z == 0.0 and i not in NOT_ON_PLANE]


def heat_case(pixels):
    """{channel: (px, py)} heat-map maxima with score 0.9, every other channel below 0.01 -> dict(idx, score) of the 57 channels"""
    idx = np.zeros(57, np.int32); sc = np.full(57, 0.001, np.float32)
    for c, (px, py) in pixels.items():
        assert 0 <= px < HM[1] and 0 <= py < HM[0]
        idx[c] = py * HM[1] + px; sc[c] = 0.9
    return dict(idx=idx, score=sc)


def heat_camera(seed):
    """every on-plane landmark that broadcast_camera(seed) sees, at the nearest heat-map pixel"""
    from eagle_amd.pitch import LANDMARKS
    ch = plane_channels()
    world = np.array([[LANDMARKS[i][2], LANDMARKS[i][3]] for i in ch], np.float64)
    img = _project(broadcast_camera(seed), world)
    pix = {}
    for c, (u, v) in zip(ch, img):
        px, py = int(round(u * (HM[1] - 1) / FRAME[1])), int(round(v * (HM[0] - 1) / FRAME[0]))
        if 0 <= px < HM[1] and 0 <= py < HM[0]:
            pix[c] = (px, py)
    return heat_case(pix)


def heat_row(seed, n_row, n_off, rows=1):
    """n_row landmark channels with their maxima in `rows` adjacent heat-map rows (one row: exactly collinear frame pixels) and n_off anywhere; which
    landmark sits where is random, so the correspondences have no consensus"""
    rng = np.random.default_rng(seed)
    ch = rng.permutation(plane_channels())[:n_row + n_off]
    xs = rng.choice(HM[1], n_row, replace=False)
    pix = {int(c): (int(x), 60 + int(rng.integers(0, rows))) for c, x in zip(ch[:n_row], xs)}
    for c in ch[n_row:]:
        pix[int(c)] = (int(rng.integers(0, HM[1])), int(rng.integers(0, HM[0])))
    return heat_case(pix)


def heat_points(case, keypoint_conf=0.3):
    """the oracle's chain up to the solver's input: decode, dedup, synthesis, on-plane selection -> (img, world, labels used)"""
    from oracle import host
    dec = host.decode_heatmaps(case["idx"], case["score"], HM[0], HM[1])
    kps = host.keypoints_from_decoded(dec, FRAME[0], FRAME[1], keypoint_conf)
    if len(kps) >= 2:
        kps = host.synthesize_keypoints(kps)
    return host.select_plane_points(kps)


# ======================================================================================================================
# the cases
# ======================================================================================================================
BOUNDS = (1, 2, 63, 64, 65, 255, 256, 257, 2000)


def _case(img, world, thresh=5.0, max_iters=2000, lm_iters=10):
    return dict(img=np.ascontiguousarray(img, np.float32), world=np.ascontiguousarray(world, np.float32), thresh=thresh, max_iters=max_iters, lm_iters=lm_iters)


def _n4_cases():
    corners = np.array([[0, 0], [105, 0], [105, 68], [0, 68]], np.float32)
    return {
        "n4_general_position": _case(np.array([[100, 100], [900, 120], [880, 600], [150, 640]], np.float32), corners),
        "n4_three_collinear": _case(np.array([[100, 100], [500, 300], [900, 500], [150, 640]], np.float32), corners),     # rank-deficient system: both sides
        "n4_equal_x_no_normalisation": _case(np.array([[300, 100], [300, 200], [300, 450], [300, 640]], np.float32), corners),   # must take the same null vector
    }


def cases():
    """{name: dict(img, world, thresh, max_iters, lm_iters)}; TRACE[name] holds what the oracle's trace must show for it"""
    c = {}
    # --- sampler: few points, repeated indices
    c["n5_attempt_of_11_draws"] = _case(*garbage_points(0, 5))                   # more than 8 draws in one attempt: the byte-wise path; 4 inliers
    c["n5_no_valid_subset"] = _case(*garbage_points(3, 5))                       # an attempt of 23 draws; (C) at iteration 0
    c["n6_attempt_of_13_draws"] = _case(*garbage_points(2, 6))
    c["n7_attempt_of_13_draws"] = _case(*garbage_points(9, 7))
    c["n87_garbage"] = _case(*garbage_points(7, MAX_KP))
    # --- (A)
    c["first_model_wins_later_ties"] = _case(*landmark_points(1, 0.0, 3))        # noise-free camera, 3 outliers: later models tie with the first, none replaces it
    c["improvement_on_lane_63"] = _case(*garbage_points(58, MAX_KP))             # 5 improvements, one on the last lane of a replay step
    c["improvement_on_lane_64"] = _case(*landmark_points(3, 0.3, 18))            # 5 improvements, one on the first lane of the second step
    c["improvement_on_attempt_255"] = _case(*garbage_points(40, MAX_KP))         # the last attempt of a full round
    c["improvement_on_round_start"] = _case(*scattered_points(44, MAX_KP, 1.0, 60))      # global attempt 256: the first of round 1; 7 improvements
    # --- (B)
    for m in BOUNDS:
        c[f"bound_{m}_every_attempt_counts"] = _case(*scattered_points(7, 30, 1.0, 0), thresh=0.01, max_iters=m)   # no rejected subset: iteration k is attempt k - 1
        c[f"bound_{m}_garbage"] = _case(*garbage_points(102, 30), max_iters=m)
    c["adaptive_bound_below_count"] = _case(*garbage_points(45, 9))              # an improvement at iteration 63 sets the bound to 53
    # --- (C)
    c["reject_1000_at_iteration_0"] = _case(*exact_line_points(10, 24, 2))
    c["reject_1000_after_1_iteration"] = _case(*exact_line_points(6, 24, 2))
    c["reject_1000_after_10_iterations"] = _case(*exact_line_points(6, 50, 4))   # the run starts in the middle of a round and spans four more
    c["reject_1000_after_106_iterations"] = _case(*exact_line_points(22, 24, 3)) # ... and past the table
    # --- thresholds
    c["thresh_1e6_first_model_takes_all"] = _case(*landmark_points(5, 2.0, 14), thresh=1e6)
    c["thresh_1e-13_models_lose_own_points"] = _case(*landmark_points(1, 0.7, 0), thresh=1e-13)   # t^2 = 1e-26 in float: some models keep 0 of their 4 points
    c["thresh_1e-15_no_model_keeps_4"] = _case(*landmark_points(1, 0.7, 0), thresh=1e-15)         # ... none keeps 4: 2000 iterations, no result
    c["thresh_0.5"] = _case(*landmark_points(5, 2.0, 14), thresh=0.5)
    c["thresh_20"] = _case(*landmark_points(5, 2.0, 14), thresh=20.0)
    c.update(_n4_cases())
    # --- DLT and LM
    for lm in (0, 1, 10, 30):
        c[f"lm_iters_{lm}"] = _case(*garbage_points(102, 30), max_iters=257, lm_iters=lm)
    for n in (5, 8, 9, 40, MAX_KP):
        c[f"inliers_{n}"] = _case(*scattered_points(n, n, 0.0, 0, snap=0.25))
    c["scale_3840x2160"] = _case(*landmark_points(2, 0.5, 4, scale=3.0))
    c["scale_320x180"] = _case(*landmark_points(2, 0.5, 4, scale=0.25))
    c["near_affine_camera"] = _case(*scattered_points(3, 40, 0.5, 6, cam=near_affine_camera()))
    c["steep_camera"] = _case(*scattered_points(3, 40, 0.5, 6, cam=steep_camera()))
    # --- the end of the draw table
    for s in (30, 321, 233):
        c[f"under_table_seed_{s}"] = _case(*near_line_points(s))
    for s in (0, 1, 2):
        c[f"past_table_best_before_seed_{s}"] = _case(*near_line_points(s))
    for s in (28, 31, 44, 38):
        c[f"past_table_best_after_seed_{s}"] = _case(*near_line_points(s))        # (38: the last improvement is the last attempt, its bound ends the loop)
    c["past_table_269270_draws"] = _case(*exact_line_points(7, 24, 2))
    return c


NOISY_CAMERA = ("improvement_on_lane_64", "thresh_0.5", "thresh_20", "scale_3840x2160", "scale_320x180", "near_affine_camera", "steep_camera")


def heat_cases():
    """{name: dict(idx, score)} for the solver inside post_kernel; TRACE[name] as above, for the points heat_points() gives"""
    return {"heat_camera": heat_camera(2),
            "heat_reject_1000_after_50_iterations": heat_row(5, 12, 2),
            "heat_past_table_best_after": heat_row(64, 20, 2, rows=2)}


# what the oracle's trace shows for every case (tests/test_homography_cases_cpu.py asserts each value): written down from one run of the trace, so that a
# change of a generator, of numpy's streams or of the oracle shows as a changed case, not as a case that silently forces something else
TRACE = {
    "n5_attempt_of_11_draws": dict(draws=327, iterations=10, attempts=53, end=0, improvements=1, last_imp_attempt=1, last_imp_draw=9, longest_reject_run=17, longest_run_attempt=13, max_attempt_draws=11, solve_failures=0, min_model_support=4, inliers=4, lm_accepted=7, final_niters=10, ties=9, imp_attempt=[1]),
    "n5_no_valid_subset": dict(draws=6387, iterations=0, attempts=1000, end=1, improvements=0, last_imp_attempt=-1, last_imp_draw=-1, longest_reject_run=1000, longest_run_attempt=0, max_attempt_draws=23, solve_failures=0, min_model_support=6, inliers=0, lm_accepted=0, final_niters=2000, ties=0, imp_attempt=[]),
    "n6_attempt_of_13_draws": dict(draws=2315, iterations=24, attempts=408, end=0, improvements=1, last_imp_attempt=16, last_imp_draw=104, longest_reject_run=91, longest_run_attempt=82, max_attempt_draws=13, solve_failures=0, min_model_support=4, inliers=4, lm_accepted=1, final_niters=24, ties=23, imp_attempt=[16]),
    "n7_attempt_of_13_draws": dict(draws=3857, iterations=47, attempts=716, end=0, improvements=1, last_imp_attempt=16, last_imp_draw=86, longest_reject_run=70, longest_run_attempt=18, max_attempt_draws=13, solve_failures=0, min_model_support=4, inliers=4, lm_accepted=6, final_niters=47, ties=46, imp_attempt=[16]),
    "n87_garbage": dict(draws=43299, iterations=2000, attempts=10628, end=0, improvements=3, last_imp_attempt=561, last_imp_draw=2284, longest_reject_run=36, longest_run_attempt=6413, max_attempt_draws=7, solve_failures=0, min_model_support=4, inliers=8, lm_accepted=10, final_niters=2000, ties=7, imp_attempt=[1, 21, 561]),
    "first_model_wins_later_ties": dict(draws=25, iterations=4, attempts=6, end=0, improvements=1, last_imp_attempt=0, last_imp_draw=4, longest_reject_run=1, longest_run_attempt=1, max_attempt_draws=5, solve_failures=0, min_model_support=32, inliers=40, lm_accepted=7, final_niters=4, ties=2, imp_attempt=[0]),
    "improvement_on_lane_63": dict(draws=43555, iterations=2000, attempts=10691, end=0, improvements=5, last_imp_attempt=1100, last_imp_draw=4477, longest_reject_run=37, longest_run_attempt=1558, max_attempt_draws=7, solve_failures=0, min_model_support=4, inliers=8, lm_accepted=9, final_niters=2000, ties=12, imp_attempt=[3, 7, 63, 504, 1100]),
    "improvement_on_lane_64": dict(draws=1362, iterations=103, attempts=325, end=0, improvements=5, last_imp_attempt=324, last_imp_draw=1362, longest_reject_run=12, longest_run_attempt=215, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=15, lm_accepted=8, final_niters=94, ties=9, imp_attempt=[1, 12, 16, 64, 324]),
    "improvement_on_attempt_255": dict(draws=43781, iterations=2000, attempts=10747, end=0, improvements=3, last_imp_attempt=255, last_imp_draw=1040, longest_reject_run=32, longest_run_attempt=9770, max_attempt_draws=7, solve_failures=0, min_model_support=4, inliers=8, lm_accepted=8, final_niters=2000, ties=2, imp_attempt=[0, 211, 255]),
    "improvement_on_round_start": dict(draws=9826, iterations=569, attempts=2411, end=0, improvements=7, last_imp_attempt=256, last_imp_draw=1045, longest_reject_run=22, longest_run_attempt=1122, max_attempt_draws=6, solve_failures=0, min_model_support=4, inliers=27, lm_accepted=6, final_niters=569, ties=17, imp_attempt=[2, 30, 65, 84, 88, 113, 256]),
    "bound_1_every_attempt_counts": dict(draws=4, iterations=1, attempts=1, end=0, improvements=1, last_imp_attempt=0, last_imp_draw=4, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=4, solve_failures=0, min_model_support=4, inliers=4, lm_accepted=2, final_niters=1, ties=0, imp_attempt=[0]),
    "bound_1_garbage": dict(draws=9, iterations=1, attempts=2, end=0, improvements=1, last_imp_attempt=1, last_imp_draw=9, longest_reject_run=1, longest_run_attempt=0, max_attempt_draws=5, solve_failures=0, min_model_support=5, inliers=5, lm_accepted=10, final_niters=1, ties=0, imp_attempt=[1]),
    "bound_2_every_attempt_counts": dict(draws=9, iterations=2, attempts=2, end=0, improvements=1, last_imp_attempt=0, last_imp_draw=4, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=5, solve_failures=0, min_model_support=4, inliers=4, lm_accepted=2, final_niters=2, ties=1, imp_attempt=[0]),
    "bound_2_garbage": dict(draws=13, iterations=2, attempts=3, end=0, improvements=1, last_imp_attempt=1, last_imp_draw=9, longest_reject_run=1, longest_run_attempt=0, max_attempt_draws=5, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=2, ties=0, imp_attempt=[1]),
    "bound_63_every_attempt_counts": dict(draws=265, iterations=63, attempts=63, end=0, improvements=2, last_imp_attempt=7, last_imp_draw=34, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=6, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=6, final_niters=63, ties=8, imp_attempt=[0, 7]),
    "bound_63_garbage": dict(draws=1586, iterations=63, attempts=377, end=0, improvements=1, last_imp_attempt=1, last_imp_draw=9, longest_reject_run=22, longest_run_attempt=134, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=63, ties=3, imp_attempt=[1]),
    "bound_64_every_attempt_counts": dict(draws=269, iterations=64, attempts=64, end=0, improvements=2, last_imp_attempt=7, last_imp_draw=34, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=6, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=6, final_niters=64, ties=8, imp_attempt=[0, 7]),
    "bound_64_garbage": dict(draws=1602, iterations=64, attempts=381, end=0, improvements=1, last_imp_attempt=1, last_imp_draw=9, longest_reject_run=22, longest_run_attempt=134, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=64, ties=3, imp_attempt=[1]),
    "bound_65_every_attempt_counts": dict(draws=273, iterations=65, attempts=65, end=0, improvements=2, last_imp_attempt=7, last_imp_draw=34, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=6, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=6, final_niters=65, ties=8, imp_attempt=[0, 7]),
    "bound_65_garbage": dict(draws=1606, iterations=65, attempts=382, end=0, improvements=1, last_imp_attempt=1, last_imp_draw=9, longest_reject_run=22, longest_run_attempt=134, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=65, ties=3, imp_attempt=[1]),
    "bound_255_every_attempt_counts": dict(draws=1075, iterations=255, attempts=255, end=0, improvements=2, last_imp_attempt=7, last_imp_draw=34, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=6, final_niters=255, ties=12, imp_attempt=[0, 7]),
    "bound_255_garbage": dict(draws=6580, iterations=255, attempts=1564, end=0, improvements=2, last_imp_attempt=1237, last_imp_draw=5208, longest_reject_run=38, longest_run_attempt=1253, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=10, final_niters=255, ties=18, imp_attempt=[1, 1237]),
    "bound_256_every_attempt_counts": dict(draws=1080, iterations=256, attempts=256, end=0, improvements=2, last_imp_attempt=7, last_imp_draw=34, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=6, final_niters=256, ties=12, imp_attempt=[0, 7]),
    "bound_256_garbage": dict(draws=6624, iterations=256, attempts=1575, end=0, improvements=2, last_imp_attempt=1237, last_imp_draw=5208, longest_reject_run=38, longest_run_attempt=1253, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=10, final_niters=256, ties=18, imp_attempt=[1, 1237]),
    "bound_257_every_attempt_counts": dict(draws=1084, iterations=257, attempts=257, end=0, improvements=2, last_imp_attempt=7, last_imp_draw=34, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=6, final_niters=257, ties=13, imp_attempt=[0, 7]),
    "bound_257_garbage": dict(draws=6637, iterations=257, attempts=1578, end=0, improvements=2, last_imp_attempt=1237, last_imp_draw=5208, longest_reject_run=38, longest_run_attempt=1253, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=10, final_niters=257, ties=18, imp_attempt=[1, 1237]),
    "bound_2000_every_attempt_counts": dict(draws=8502, iterations=2000, attempts=2019, end=0, improvements=3, last_imp_attempt=1688, last_imp_draw=7104, longest_reject_run=1, longest_run_attempt=289, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=6, final_niters=2000, ties=41, imp_attempt=[0, 7, 1688]),
    "bound_2000_garbage": dict(draws=47693, iterations=2000, attempts=11302, end=0, improvements=2, last_imp_attempt=1237, last_imp_draw=5208, longest_reject_run=41, longest_run_attempt=6075, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=10, final_niters=2000, ties=30, imp_attempt=[1, 1237]),
    "adaptive_bound_below_count": dict(draws=1062, iterations=63, attempts=218, end=0, improvements=2, last_imp_attempt=217, last_imp_draw=1062, longest_reject_run=14, longest_run_attempt=35, max_attempt_draws=10, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=53, ties=61, imp_attempt=[1, 217]),
    "reject_1000_at_iteration_0": dict(draws=4242, iterations=0, attempts=1000, end=1, improvements=0, last_imp_attempt=-1, last_imp_draw=-1, longest_reject_run=1000, longest_run_attempt=0, max_attempt_draws=7, solve_failures=0, min_model_support=27, inliers=0, lm_accepted=0, final_niters=2000, ties=0, imp_attempt=[]),
    "reject_1000_after_1_iteration": dict(draws=5225, iterations=1, attempts=1232, end=2, improvements=1, last_imp_attempt=231, last_imp_draw=976, longest_reject_run=1000, longest_run_attempt=232, max_attempt_draws=7, solve_failures=0, min_model_support=4, inliers=4, lm_accepted=5, final_niters=2000, ties=0, imp_attempt=[231]),
    "reject_1000_after_10_iterations": dict(draws=15685, iterations=10, attempts=3819, end=2, improvements=1, last_imp_attempt=278, last_imp_draw=1145, longest_reject_run=1000, longest_run_attempt=2819, max_attempt_draws=7, solve_failures=0, min_model_support=4, inliers=4, lm_accepted=9, final_niters=2000, ties=9, imp_attempt=[278]),
    "reject_1000_after_106_iterations": dict(draws=80390, iterations=106, attempts=18943, end=2, improvements=2, last_imp_attempt=408, last_imp_draw=1722, longest_reject_run=1000, longest_run_attempt=17943, max_attempt_draws=9, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=2000, ties=16, imp_attempt=[267, 408]),
    "thresh_1e6_first_model_takes_all": dict(draws=4, iterations=1, attempts=1, end=3, improvements=1, last_imp_attempt=0, last_imp_draw=4, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=4, solve_failures=0, min_model_support=36, inliers=36, lm_accepted=10, final_niters=0, ties=0, imp_attempt=[0]),
    "thresh_1e-13_models_lose_own_points": dict(draws=8728, iterations=2000, attempts=2113, end=0, improvements=1, last_imp_attempt=0, last_imp_draw=4, longest_reject_run=3, longest_run_attempt=1721, max_attempt_draws=7, solve_failures=0, min_model_support=0, inliers=4, lm_accepted=7, final_niters=2000, ties=1973, imp_attempt=[0]),
    "thresh_1e-15_no_model_keeps_4": dict(draws=8728, iterations=2000, attempts=2113, end=0, improvements=0, last_imp_attempt=-1, last_imp_draw=-1, longest_reject_run=3, longest_run_attempt=1721, max_attempt_draws=7, solve_failures=0, min_model_support=0, inliers=0, lm_accepted=0, final_niters=2000, ties=0, imp_attempt=[]),
    "thresh_0.5": dict(draws=854, iterations=66, attempts=203, end=0, improvements=4, last_imp_attempt=71, last_imp_draw=306, longest_reject_run=11, longest_run_attempt=57, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=19, lm_accepted=6, final_niters=66, ties=2, imp_attempt=[0, 13, 30, 71]),
    "thresh_20": dict(draws=358, iterations=24, attempts=85, end=0, improvements=2, last_imp_attempt=13, last_imp_draw=61, longest_reject_run=11, longest_run_attempt=57, max_attempt_draws=6, solve_failures=0, min_model_support=10, inliers=24, lm_accepted=6, final_niters=24, ties=5, imp_attempt=[0, 13]),
    "n4_general_position": dict(draws=0, iterations=0, attempts=0, end=4, improvements=0, last_imp_attempt=-1, last_imp_draw=-1, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=0, solve_failures=0, min_model_support=5, inliers=4, lm_accepted=0, final_niters=2000, ties=0, imp_attempt=[]),
    "n4_three_collinear": dict(draws=0, iterations=0, attempts=0, end=4, improvements=0, last_imp_attempt=-1, last_imp_draw=-1, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=0, solve_failures=0, min_model_support=5, inliers=4, lm_accepted=0, final_niters=2000, ties=0, imp_attempt=[]),
    "n4_equal_x_no_normalisation": dict(draws=0, iterations=0, attempts=0, end=4, improvements=0, last_imp_attempt=-1, last_imp_draw=-1, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=0, solve_failures=0, min_model_support=5, inliers=0, lm_accepted=0, final_niters=2000, ties=0, imp_attempt=[]),
    "lm_iters_0": dict(draws=6637, iterations=257, attempts=1578, end=0, improvements=2, last_imp_attempt=1237, last_imp_draw=5208, longest_reject_run=38, longest_run_attempt=1253, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=0, final_niters=257, ties=18, imp_attempt=[1, 1237]),
    "lm_iters_1": dict(draws=6637, iterations=257, attempts=1578, end=0, improvements=2, last_imp_attempt=1237, last_imp_draw=5208, longest_reject_run=38, longest_run_attempt=1253, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=1, final_niters=257, ties=18, imp_attempt=[1, 1237]),
    "lm_iters_10": dict(draws=6637, iterations=257, attempts=1578, end=0, improvements=2, last_imp_attempt=1237, last_imp_draw=5208, longest_reject_run=38, longest_run_attempt=1253, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=10, final_niters=257, ties=18, imp_attempt=[1, 1237]),
    "lm_iters_30": dict(draws=6637, iterations=257, attempts=1578, end=0, improvements=2, last_imp_attempt=1237, last_imp_draw=5208, longest_reject_run=38, longest_run_attempt=1253, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=11, final_niters=257, ties=18, imp_attempt=[1, 1237]),
    "inliers_5": dict(draws=5, iterations=1, attempts=1, end=3, improvements=1, last_imp_attempt=0, last_imp_draw=5, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=5, solve_failures=0, min_model_support=5, inliers=5, lm_accepted=7, final_niters=0, ties=0, imp_attempt=[0]),
    "inliers_8": dict(draws=6, iterations=1, attempts=1, end=3, improvements=1, last_imp_attempt=0, last_imp_draw=6, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=6, solve_failures=0, min_model_support=8, inliers=8, lm_accepted=5, final_niters=0, ties=0, imp_attempt=[0]),
    "inliers_9": dict(draws=4, iterations=1, attempts=1, end=3, improvements=1, last_imp_attempt=0, last_imp_draw=4, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=4, solve_failures=0, min_model_support=9, inliers=9, lm_accepted=6, final_niters=0, ties=0, imp_attempt=[0]),
    "inliers_40": dict(draws=4, iterations=1, attempts=1, end=3, improvements=1, last_imp_attempt=0, last_imp_draw=4, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=4, solve_failures=0, min_model_support=40, inliers=40, lm_accepted=3, final_niters=0, ties=0, imp_attempt=[0]),
    "inliers_87": dict(draws=8, iterations=2, attempts=2, end=3, improvements=2, last_imp_attempt=1, last_imp_draw=8, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=4, solve_failures=0, min_model_support=86, inliers=87, lm_accepted=7, final_niters=0, ties=0, imp_attempt=[0, 1]),
    "scale_3840x2160": dict(draws=24, iterations=5, attempts=6, end=0, improvements=2, last_imp_attempt=1, last_imp_draw=8, longest_reject_run=1, longest_run_attempt=3, max_attempt_draws=4, solve_failures=0, min_model_support=8, inliers=37, lm_accepted=7, final_niters=5, ties=0, imp_attempt=[0, 1]),
    "scale_320x180": dict(draws=32, iterations=5, attempts=8, end=0, improvements=1, last_imp_attempt=0, last_imp_draw=4, longest_reject_run=2, longest_run_attempt=5, max_attempt_draws=4, solve_failures=0, min_model_support=21, inliers=37, lm_accepted=8, final_niters=5, ties=2, imp_attempt=[0]),
    "near_affine_camera": dict(draws=51, iterations=7, attempts=12, end=0, improvements=2, last_imp_attempt=1, last_imp_draw=8, longest_reject_run=3, longest_run_attempt=2, max_attempt_draws=5, solve_failures=0, min_model_support=4, inliers=34, lm_accepted=4, final_niters=7, ties=3, imp_attempt=[0, 1]),
    "steep_camera": dict(draws=39, iterations=7, attempts=9, end=0, improvements=3, last_imp_attempt=4, last_imp_draw=21, longest_reject_run=2, longest_run_attempt=2, max_attempt_draws=5, solve_failures=0, min_model_support=11, inliers=34, lm_accepted=10, final_niters=7, ties=1, imp_attempt=[0, 1, 4]),
    "under_table_seed_30": dict(draws=64191, iterations=1354, attempts=14787, end=0, improvements=2, last_imp_attempt=62, last_imp_draw=274, longest_reject_run=101, longest_run_attempt=671, max_attempt_draws=11, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=1354, ties=174, imp_attempt=[1, 62]),
    "under_table_seed_321": dict(draws=62726, iterations=1354, attempts=14907, end=0, improvements=5, last_imp_attempt=11292, last_imp_draw=47489, longest_reject_run=70, longest_run_attempt=468, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=8, lm_accepted=10, final_niters=1354, ties=16, imp_attempt=[4, 64, 131, 1771, 11292]),
    "under_table_seed_233": dict(draws=61768, iterations=1354, attempts=14229, end=0, improvements=2, last_imp_attempt=168, last_imp_draw=720, longest_reject_run=70, longest_run_attempt=8155, max_attempt_draws=11, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=1354, ties=120, imp_attempt=[3, 168]),
    "past_table_best_before_seed_0": dict(draws=84261, iterations=2000, attempts=20380, end=0, improvements=4, last_imp_attempt=5443, last_imp_draw=22498, longest_reject_run=63, longest_run_attempt=11135, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=7, lm_accepted=10, final_niters=2000, ties=21, imp_attempt=[61, 142, 1269, 5443]),
    "past_table_best_before_seed_1": dict(draws=75334, iterations=2000, attempts=18004, end=0, improvements=3, last_imp_attempt=1735, last_imp_draw=7278, longest_reject_run=73, longest_run_attempt=11053, max_attempt_draws=9, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=10, final_niters=2000, ties=34, imp_attempt=[2, 7, 1735]),
    "past_table_best_before_seed_2": dict(draws=88646, iterations=2000, attempts=21448, end=0, improvements=3, last_imp_attempt=1388, last_imp_draw=5724, longest_reject_run=83, longest_run_attempt=1638, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=10, final_niters=2000, ties=28, imp_attempt=[10, 41, 1388]),
    "past_table_best_after_seed_28": dict(draws=88640, iterations=2000, attempts=21384, end=0, improvements=4, last_imp_attempt=19109, last_imp_draw=79215, longest_reject_run=100, longest_run_attempt=13776, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=7, lm_accepted=10, final_niters=2000, ties=45, imp_attempt=[19, 29, 297, 19109]),
    "past_table_best_after_seed_31": dict(draws=94124, iterations=2000, attempts=22637, end=0, improvements=4, last_imp_attempt=17478, last_imp_draw=72678, longest_reject_run=73, longest_run_attempt=3214, max_attempt_draws=9, solve_failures=0, min_model_support=4, inliers=7, lm_accepted=10, final_niters=2000, ties=43, imp_attempt=[0, 58, 743, 17478]),
    "past_table_best_after_seed_44": dict(draws=133430, iterations=2000, attempts=32072, end=0, improvements=3, last_imp_attempt=18419, last_imp_draw=76617, longest_reject_run=127, longest_run_attempt=29361, max_attempt_draws=8, solve_failures=0, min_model_support=4, inliers=7, lm_accepted=10, final_niters=2000, ties=20, imp_attempt=[8, 264, 18419]),
    "past_table_best_after_seed_38": dict(draws=79381, iterations=1895, attempts=18689, end=0, improvements=3, last_imp_attempt=18688, last_imp_draw=79381, longest_reject_run=57, longest_run_attempt=165, max_attempt_draws=9, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=10, final_niters=1866, ties=119, imp_attempt=[14, 277, 18688]),
    "past_table_269270_draws": dict(draws=269270, iterations=273, attempts=63309, end=2, improvements=2, last_imp_attempt=15963, last_imp_draw=67817, longest_reject_run=1000, longest_run_attempt=62309, max_attempt_draws=9, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=2000, ties=70, imp_attempt=[481, 15963]),
    "heat_camera": dict(draws=8, iterations=2, attempts=2, end=3, improvements=2, last_imp_attempt=1, last_imp_draw=8, longest_reject_run=0, longest_run_attempt=0, max_attempt_draws=4, solve_failures=0, min_model_support=30, inliers=41, lm_accepted=7, final_niters=0, ties=0, imp_attempt=[0, 1]),
    "heat_reject_1000_after_50_iterations": dict(draws=35425, iterations=50, attempts=7851, end=2, improvements=1, last_imp_attempt=79, last_imp_draw=356, longest_reject_run=1000, longest_run_attempt=6851, max_attempt_draws=9, solve_failures=0, min_model_support=4, inliers=5, lm_accepted=10, final_niters=323, ties=17, imp_attempt=[79]),
    "heat_past_table_best_after": dict(draws=78701, iterations=1594, attempts=18438, end=0, improvements=3, last_imp_attempt=18144, last_imp_draw=77454, longest_reject_run=89, longest_run_attempt=16775, max_attempt_draws=9, solve_failures=0, min_model_support=4, inliers=6, lm_accepted=10, final_niters=1594, ties=184, imp_attempt=[6, 130, 18144]),
}
