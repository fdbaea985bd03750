"""Constructed inputs for the kernels behind the two networks (tests/test_tail_cases_cpu.py, tests/test_gpu_tail.py): the detector tail
(yolo_decode_kernel, nms_kernel), the heat-map arg-max (heat_argmax_kernel and the fused epilogue of the head convolution) and the decode, dedup,
synthesis, bounds and projection parts of post_kernel.  Pure numpy; every case is named after the tie or edge it forces, and test_tail_cases_cpu.py
asserts through the oracle that it really does.

How the detector cases are exact: a DFL side whose 16 logits are +30 on bin k and -30 elsewhere decodes to the integer distance k (exp(-60) vanishes
against 1 in fp32), so boxes are chosen in grid units; equal class logits are equal confidences.

All inputs are finite.  NaN and infinite logits are out of scope: the reference does not define what they decode to."""
import numpy as np

from eagle_amd.pitch import LANDMARKS, NOT_ON_PLANE

NC = 5
FLOOR = 0.15
OFF = -10.0                      # class logit of an anchor that is no candidate (sigmoid = 4.5e-5)


# ======================================================================================================================
# detector tail
# ======================================================================================================================
class Grid:
    """One pyramid level of one frame, built cell by cell: integer DFL distances (l, t, r, b) and class logits."""

    def __init__(self, gh, gw, stride=8.0):
        self.gh, self.gw, self.stride = gh, gw, float(stride)
        self.d = np.zeros((gh, gw, 4), np.int64)
        self.cls = np.full((gh, gw, NC), OFF, np.float32)

    def put(self, cell, ltrb, logit, c=0):
        gy, gx = divmod(int(cell), self.gw)
        self.d[gy, gx] = ltrb
        self.cls[gy, gx, c] = logit

    def tensors(self):
        box = np.full((self.gh, self.gw, 4, 16), -30.0, np.float32)
        np.put_along_axis(box, self.d[..., None], 30.0, axis=3)
        return box.reshape(self.gh, self.gw, 64), self.cls.copy()


def _unit_boxes(g, cells, logits, c=0):
    """disjoint boxes: cell (gy, gx) owns [gx + .5, gx + 1.5] x [gy + .5, gy + 1.5] (neighbours touch, IoU 0)"""
    for cell, lg in zip(cells, logits):
        g.put(cell, (0, 0, 1, 1), lg, c)


def _ranked(n, hi=3.0, lo=-1.5):
    """n distinct class logits, descending, all above the floor (sigmoid(-1.5) = 0.18); neighbours differ by >= 5e-5 after the sigmoid for n <= 4000"""
    return np.linspace(hi, lo, n).astype(np.float32)


def det_case(frames, nms_iou=0.5, detector_conf=0.35, frame_hw=None, in_hw=None, conf_floor=FLOOR):
    """frames: list of per-frame level lists [Grid, ...] (same shapes in every frame) -> the case dict the tests run"""
    nl = len(frames[0])
    levels = []
    for l in range(nl):
        t = [f[l].tensors() for f in frames]
        levels.append((np.stack([b for b, _ in t]), np.stack([c for _, c in t]), frames[0][l].stride))
    g0 = frames[0][0]
    in_hw = in_hw or (int(g0.gh * g0.stride), int(g0.gw * g0.stride))
    return dict(levels=levels, nc=NC, nms_iou=np.float32(nms_iou), detector_conf=detector_conf, conf_floor=np.float32(conf_floor),
                in_hw=in_hw, frame_hw=frame_hw or in_hw)


GH, GW = 48, 80                  # the stride-8 level of a 384 x 640 detector input: 3840 anchors


def case_counts():
    """candidate counts at the sort's edges, one frame each, side by side: 0, 1, 63, 64, 65, 1024, 1025 (and 2: the smallest sort that swaps)"""
    frames = []
    rng = np.random.default_rng(11)
    for k in (0, 1, 2, 63, 64, 65, 1024, 1025):
        g = Grid(GH, GW)
        cells = rng.permutation(GH * GW)[:k]          # candidates scattered over the anchors: the atomic append order is arbitrary
        _unit_boxes(g, cells, _ranked(max(k, 1))[:k])
        frames.append([g])
    return det_case(frames)


def case_all_candidates():
    """every anchor of the largest supported geometry (rect letterbox, det_imgsz 960: 68x120 + 34x60 + 17x30 = 10710 anchors) is a candidate (cnt == A), and
    a 1 x 1 one-level frame shape is covered by case_random_1x1.  Boxes are disjoint within a level; confidences descend with a stride-7 walk over the anchors."""
    frames = []
    for seed in (0, 1):
        lv = []
        a0 = 0
        A = 68 * 120 + 34 * 60 + 17 * 30
        rank = (np.arange(A) * 7 + seed * 3) % A       # 7 is coprime to 10710: a permutation
        lg = np.linspace(4.0, -1.5, A).astype(np.float32)
        for gh, gw, s in ((68, 120, 8), (34, 60, 16), (17, 30, 32)):
            g = Grid(gh, gw, s)
            n = gh * gw
            _unit_boxes(g, np.arange(n), lg[rank[a0:a0 + n]], c=len(lv) % 2)
            lv.append(g); a0 += n
        frames.append(lv)
    return det_case(frames, frame_hw=(720, 1280), in_hw=(544, 960))


def _cap_frame(suppressed):
    """> 300 disjoint survivors; `suppressed` of the first candidates in sorted order are duplicates of a better box, so that the 300th kept box sits at
    sorted position 299 + suppressed and the walk stops at the next alive one"""
    g = Grid(GH, GW)
    lg = _ranked(700)
    k = 0
    # pairs of horizontally adjacent cells with the SAME box [gx + .5, gx + 1.5]: (0, 0, 1, 1) from the left cell, (1, 0, 0, 1) from the right one
    for p in range(suppressed):
        left = p * 2
        g.put(left, (0, 0, 1, 1), lg[k]); g.put(left + 1, (1, 0, 0, 1), lg[k + 1]); k += 2
    cells = np.arange(2 * suppressed + 2, 2 * suppressed + 2 + 2 * (700 - k), 2)    # every other cell: disjoint, not touching the pairs
    _unit_boxes(g, cells, lg[k:])
    return [g]


def case_cap():
    """the 300-box cap: the 301st alive candidate in the middle of a 64-block (sorted position 300), on a block's last lane (319), on the first lane of the
    next block (320: s_stop is raised by a block that keeps nothing)"""
    return det_case([_cap_frame(0), _cap_frame(19), _cap_frame(20)])


def case_cross_block():
    """suppression across blocks with 3587 candidates (more than 1024 + 64) of which 16 survive, so the 300-box cap never ends the walk: every 16 x 16 block
    of cells but the first emits ONE box 15 cells wide from all of its 256 anchors (l = column in the block, r = 15 - l, likewise t / b), ranks scattered, so a
    box kept in an early 64-block kills copies thousands of sorted positions later (the dead[] pass and its j += 1024 stride).  The first block holds a chain:
    A (sorted position 5) kills B (130), B would have killed C (1300), A does not reach C: C survives.  -> (case, anchors of A, B, C)"""
    g = Grid(GH, GW)
    cells, ltrb = [], []
    for by in range(GH // 16):
        for bx in range(GW // 16):
            if by == 0 and bx == 0:
                continue
            for ly in range(16):
                for lx in range(16):
                    cells.append((by * 16 + ly) * GW + bx * 16 + lx); ltrb.append((lx, ly, 15 - lx, 15 - ly))
    # chain in row 4 of the first block (height 1): A = [.5, 4.5], B = [1.5, 5.5], C = [2.5, 6.5]: IoU(A, B) = IoU(B, C) = 3/5 > 0.5, IoU(A, C) = 2/6
    abc = (4 * GW + 0, 4 * GW + 1, 4 * GW + 2)
    n = len(cells) + 3
    lg = _ranked(n)
    chain_rank = (5, 130, 1300)
    free = [k for k in range(n) if k not in chain_rank]
    order = np.random.default_rng(3).permutation(len(cells))
    for k, o in zip(free, order):
        g.put(cells[o], ltrb[o], lg[k])
    for cell, rk in zip(abc, chain_rank):
        g.put(cell, (0, 0, 4, 1), lg[rk])
    return det_case([[g]]), abc


def case_ties():
    """confidence ties: runs of equal class logits (2, 64 and 130 anchors, the last crossing two block boundaries), scattered over the grid so that the append
    order differs from the anchor order; two tied copies of one box (the smaller anchor index must win); a tie across the 300-box cap"""
    rng = np.random.default_rng(5)
    g = Grid(GH, GW)
    cells = rng.permutation(np.arange(4 * GW, GH * GW))   # rows 4..: disjoint unit boxes
    k = 0
    for run, lg in ((2, 2.5), (64, 2.0), (130, 1.5), (150, 1.0), (40, 0.5)):      # 386 candidates, > 300 kept: the cap cuts the 150-run
        _unit_boxes(g, cells[k:k + run], np.full(run, lg, np.float32)); k += run
    g.put(10, (0, 0, 1, 1), 3.0); g.put(11, (1, 0, 0, 1), 3.0)                    # one box from two anchors, equal confidence
    g2 = Grid(GH, GW)                                                               # second frame: every candidate has the same confidence
    _unit_boxes(g2, rng.permutation(GH * GW)[:200], np.full(200, 1.25, np.float32))
    return det_case([[g], [g2]])


def case_iou_threshold():
    """IoU exactly at the threshold must not suppress (the test is >): nms_iou = 0.5, boxes 3 wide shifted by 1 (IoU 2/4); one step closer (IoU 3/5) does
    suppress; zero-area boxes (0/0) suppress nothing and are not suppressed"""
    g = Grid(12, 20)
    g.put(0 * 20 + 1, (1, 0, 2, 2), 3.0); g.put(0 * 20 + 2, (1, 0, 2, 2), 2.9)    # [.5, 3.5] and [1.5, 4.5]: inter 2, union 4
    g.put(4 * 20 + 1, (1, 0, 3, 2), 2.8); g.put(4 * 20 + 2, (1, 0, 3, 2), 2.7)    # [.5, 4.5] and [1.5, 5.5]: inter 3, union 5
    g.put(8 * 20 + 5, (0, 0, 0, 0), 2.6); g.put(8 * 20 + 5 + 1, (1, 0, 0, 0), 2.5)  # the same point twice: area 0, IoU 0/0
    g.put(8 * 20 + 9, (1, 1, 1, 1), 2.4); g.put(9 * 20 + 9, (0, 1, 0, 0), 2.3)    # a zero-width box inside a real one: inter 0
    return det_case([[g], [g]], nms_iou=0.5)


def case_classes():
    """class offset (one box from two anchors in two classes survives twice), ball ids (cls 2: the count of earlier kept balls, interleaved with players and
    unreported classes), classes 3 and 4 (reported = 0, id -1), confidences around detector_conf = 0.5 (sigmoid(0) = 0.5 exactly: reported; just below: kept,
    unreported), and clamping at the frame edge (players clamp to frame_w - 1 / frame_h - 1, balls do not).  Frame = detector input, gain 1."""
    g = Grid(12, 20)
    g.put(1, (0, 0, 1, 1), 3.0, 0); g.put(2, (1, 0, 0, 1), 2.9, 1)                # same box, classes 0 and 1
    g.put(20 + 2, (1, 1, 0, 0), 2.8, 1)                                           # ... and a third copy (from the cell below) in class 1: suppressed
    lg = iter(np.linspace(2.5, -0.2, 14).astype(np.float32))
    for i, c in enumerate((2, 0, 3, 2, 4, 1, 2, 2, 0, 2)):                        # five balls among other classes
        g.put(2 * 20 + 2 * i, (0, 0, 1, 1), next(lg), c)
    g.put(4 * 20 + 0, (0, 0, 1, 1), 0.0, 0)                                       # conf == detector_conf
    g.put(4 * 20 + 2, (0, 0, 1, 1), -1e-6, 0)                                     # sigmoid = 0.49999975
    g.put(4 * 20 + 4, (0, 0, 1, 1), -1e-3, 2)                                     # a ball below detector_conf still counts towards later ball ids
    g.put(4 * 20 + 6, (0, 0, 1, 1), -2e-3, 2)
    # boxes over the right / bottom edge of the 96 x 160 frame: x2 = (19.5 + 3) * 8 = 180 -> 160 (float clamp), ints 159 for a player, 160 for a ball
    g.put(6 * 20 + 19, (2, 0, 3, 1), 2.0, 0); g.put(8 * 20 + 19, (2, 0, 3, 1), 1.9, 2)
    g.put(11 * 20 + 5, (0, 2, 1, 3), 1.8, 1); g.put(11 * 20 + 9, (0, 2, 1, 3), 1.7, 2)
    g.put(0 * 20 + 0, (3, 3, 0, 0), 1.6, 0)                                       # over the top-left: negative coordinates clamp to 0
    return det_case([[g]], nms_iou=0.5, detector_conf=0.5)


def _random_levels(shapes, n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-12, 12, (n, gh, gw, 64)).astype(np.float32), rng.uniform(-12, 12, (n, gh, gw, NC)).astype(np.float32), float(s)) for gh, gw, s in shapes]


def case_random(which):
    """plain random logits in [-12, 12] at the real grids: fractional DFL expectations, boxes that overlap at every IoU, every class (the cls * 7680 offset
    rounds the low bits of a box), several hundred to several thousand candidates, the default thresholds"""
    if which == "384x640":
        return dict(levels=_random_levels(((48, 80, 8), (24, 40, 16), (12, 20, 32)), 2, 1), nc=NC, nms_iou=np.float32(0.7), detector_conf=0.35,
                    conf_floor=np.float32(FLOOR), in_hw=(384, 640), frame_hw=(720, 1280))
    if which == "544x960":
        return dict(levels=_random_levels(((68, 120, 8), (34, 60, 16), (17, 30, 32)), 2, 2), nc=NC, nms_iou=np.float32(0.7), detector_conf=0.35,
                    conf_floor=np.float32(FLOOR), in_hw=(544, 960), frame_hw=(1080, 1920))
    assert which == "1x1"
    return dict(levels=_random_levels(((1, 1, 32),), 3, 3), nc=NC, nms_iou=np.float32(0.7), detector_conf=0.35, conf_floor=np.float32(FLOOR),
                in_hw=(32, 32), frame_hw=(32, 32))


def detector_cases():
    cross, _ = case_cross_block()
    return {"counts": case_counts(), "all_candidates": case_all_candidates(), "cap": case_cap(), "cross_block": cross, "ties": case_ties(),
            "iou_threshold": case_iou_threshold(), "classes": case_classes(), "random_384x640": case_random("384x640"),
            "random_544x960": case_random("544x960"), "random_1x1": case_random("1x1")}


# ---- expected values (the oracle's plain functions) ------------------------------------------------------------------
def detector_rows(case, f):
    """[A, 4 + nc] rows (cx, cy, w, h, class probabilities) of frame f, levels concatenated as the anchors are numbered"""
    from oracle import prims as P
    return np.concatenate([P.yolo_decode_level(b[f], c[f], case["nc"], s) for b, c, s in case["levels"]], 0)


def decode_scratch(rows):
    """what yolo_decode_kernel leaves per anchor: xyxy boxes (the arithmetic of nms_and_scale), best probability, its class"""
    cx, cy, bw, bh = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    hw, hh = bw / np.float32(2), bh / np.float32(2)
    return np.stack([cx - hw, cy - hh, cx + hw, cy + hh], 1).astype(np.float32), rows[:, 4:].max(1), rows[:, 4:].argmax(1).astype(np.int32)


def detector_expected(case, f):
    """-> (dets [K, 6] of nms_and_scale, objects of objects_from_detections, candidate count)"""
    from oracle import host
    rows = detector_rows(case, f)
    fh, fw = case["frame_hw"]
    dets = host.nms_and_scale(rows, fh, fw, case["in_hw"][0], case["in_hw"][1], conf_thres=case["conf_floor"], iou_thres=case["nms_iou"])
    return dets, host.objects_from_detections(dets, fh, fw, case["detector_conf"]), int((rows[:, 4:].max(1) > case["conf_floor"]).sum())


def sorted_candidates(rows, floor=FLOOR):
    """anchor indices in the order the NMS walks them: descending confidence, ties by anchor index"""
    conf = rows[:, 4:].max(1)
    idx = np.nonzero(conf > np.float32(floor))[0]
    return idx[np.argsort(-conf[idx], kind="stable")]


# ======================================================================================================================
# heat maps
# ======================================================================================================================
HI, LO = 20.0, -30.0             # sigmoid(20) == 1.0f; sigmoid(-30) = 9.4e-14


def heat_patterns(h, w, chunks=64, tile=(8, 32)):
    """{channel: (name, pixels of a plateau of logit 20 on a background of -30)} for an h x w map; positions follow the chunk length of heat_argmax_kernel for
    `chunks` and the tile of the fused epilogue, reduced into the map where it is smaller"""
    HW = h * w
    per = (HW + chunks - 1) // chunks
    th, tw = tile
    px = lambda y, x: (min(y, h - 1)) * w + min(x, w - 1)
    pat = {
        0: ("two_chunks", [min(per - 1, HW - 1), min(per, HW - 1)]),                       # the first pixel is the last pixel of chunk 0
        1: ("four_phases", [min(p, HW - 1) for p in range(per + 1, per + 5)]),               # one pixel per wave of heat_argmax_kernel, the first not in wave 0
        2: ("whole_map", list(range(HW))),
        3: ("all_low", []),                                                                   # every pixel ties at sigmoid(-30): answer 0
        4: ("later_phase_first", [min(7, HW - 1), min(8, HW - 1)]),                           # pixel 7 (wave 3) before pixel 8 (wave 0)
        5: ("two_tiles_x", [px(th + 1, tw - 1), px(th + 1, tw)]),
        6: ("two_tiles_y", [px(th - 1, tw + 3), px(th, tw + 3)]),
        7: ("last_pixel", [HW - 1]),                                                          # the partial last chunk / tile
        8: ("far_apart", [min(3 * per + 2, HW - 1), HW - 1]),                                 # a tie between the partials of distant chunks
        9: ("tile_diagonal", [px(2 * th - 1, 2 * tw), px(2 * th, 2 * tw - 1)]),               # row-major order, not tile order: the tile to the right comes first
        10: ("last_row_and_column", [px(h - 1, 0), px(0, w - 1)]),
    }
    return pat


def heat_logits(h, w, n=2, chunks=64, tile=(8, 32), seed=0):
    """fp32 logits [n, h, w, 64]: channels 0 - 10 carry heat_patterns, 11 - 56 a random background in [-6, 6] with plateaus of 20 at three random pixels (frame 0)
    or a unique maximum (frame 1); channels 57 - 63 are padding and hold +25 everywhere (a kernel that lets padding leak into a real channel shows)"""
    rng = np.random.default_rng(seed)
    HW = h * w
    lg = np.full((n, HW, 64), LO, np.float32)
    for c, (_, pix) in heat_patterns(h, w, chunks, tile).items():
        lg[:, pix, c] = HI
    for c in range(11, 57):
        lg[:, :, c] = rng.uniform(-6, 6, (n, HW)).astype(np.float32)
        lg[0, rng.integers(0, HW, 3), c] = HI
    lg[:, :, 57:] = 25.0
    return lg.reshape(n, h, w, 64)


HEAT_SIZES = {"135x240": (135, 240), "1x1": (1, 1), "7x65": (7, 65), "5x9": (5, 9)}        # 5 x 9 = 45 pixels: fewer than 64 chunks
HEAT_CHUNKS = (1, 3, 64)


def chunk_first_max(sig_flat, chunks):
    """expected partials [chunks, C] (score, idx) of heat_argmax_kernel over sigmoid values [HW, C]"""
    HW, C = sig_flat.shape
    per = (HW + chunks - 1) // chunks
    score = np.full((chunks, C), -1.0, np.float32); idx = np.full((chunks, C), 0x7fffffff, np.int32)
    for k in range(chunks):
        p0, p1 = k * per, min(HW, (k + 1) * per)
        if p0 < p1:
            a = sig_flat[p0:p1].argmax(0)
            idx[k] = p0 + a; score[k] = sig_flat[p0:p1][a, np.arange(C)]
    return score, idx


def tile_first_max(sig, th, tw):
    """expected partials [tiles, C] of the fused epilogue over sigmoid values [h, w, C]: tiles row-major, first maximum in row-major pixel order"""
    h, w, C = sig.shape
    ty, tx = (h + th - 1) // th, (w + tw - 1) // tw
    score = np.empty((ty * tx, C), np.float32); idx = np.empty((ty * tx, C), np.int32)
    for t in range(ty * tx):
        y0, x0 = (t // tx) * th, (t % tx) * tw
        blk = sig[y0:y0 + th, x0:x0 + tw]
        bh, bw = blk.shape[:2]
        a = blk.reshape(-1, C).argmax(0)
        score[t] = blk.reshape(-1, C)[a, np.arange(C)]
        idx[t] = (y0 + a // bw) * w + x0 + a % bw
    return score, idx


def fused_case_1x1(h, w, cin=16, cout=57, seed=0):
    """a 1 x 1 head convolution whose logits are exact in both families: input channel k carries the map of output channels k, k + 16, ... as small integers
    (20 / -30 / a random integer background), the weights are 0 / 1 / 0.5, the bias a power of two -> (x, w_hwio, bias, exact logits)"""
    lg = heat_logits(h, w, 2, 64, (8, 32), seed)
    x = np.zeros((2, h, w, cin), np.float32)
    for k in range(cin):
        x[..., k] = np.rint(lg[..., k])                    # channels 0 - 10: the patterns; 11 - 15: integer backgrounds with plateaus
    wt = np.zeros((1, 1, cin, cout), np.float32)
    bias = np.zeros(cout, np.float32)
    for c in range(cout):
        wt[0, 0, c % cin, c] = 1.0 if c < 2 * cin else 0.5  # (0.5: plateaus of logit 10 + bias: still sigmoid == 1.0 with the bias below)
        bias[c] = 0.0 if c < cin else 8.0
    logits = np.einsum("nhwk,kc->nhwc", x, wt[0, 0]).astype(np.float32) + bias
    return x, wt, bias, logits


def fused_case_3x3(h=20, w=33, cin=16, cout=57, seed=7):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((2, h, w, cin)).astype(np.float32), (rng.standard_normal((3, 3, cin, cout)) * 0.2).astype(np.float32),
            rng.standard_normal(cout).astype(np.float32))


# ======================================================================================================================
# post stage: decode / dedup / synthesis / homography / bounds / projection
# ======================================================================================================================
HM = (135, 240)
FRAME = (720, 1280)
WORLD = {i: (x, y) for i, _, x, y, z in LANDMARKS if z == 0.0 and i not in NOT_ON_PLANE}


def _camera(kind):
    """pitch metres -> frame pixels.  "axis": an axis-aligned affine view (the frame's left and right edges map to lines of constant pitch x: find_x_at_y
    divides by zero, "no bounds"); "tilt": the same rotated by a few degrees (bounds exist)"""
    if kind == "axis":
        return lambda X, Y: (100.0 + 10.0 * X, 40.0 + 9.0 * Y)
    a = np.deg2rad(7.0)
    return lambda X, Y: (140.0 + 9.0 * (np.cos(a) * X - np.sin(a) * Y), 60.0 + 7.0 * (np.sin(a) * X + np.cos(a) * Y))


def _hm_index(u, v):
    """the heat-map pixel whose frame pixel (decode_dedup's mapping) is nearest to (u, v)"""
    px = int(round(u * (HM[1] - 1) / FRAME[1])); py = int(round(v * (HM[0] - 1) / FRAME[0]))
    assert 0 <= px < HM[1] and 0 <= py < HM[0], (u, v)
    return py * HM[1] + px


def post_case(labels, cam="tilt", score=0.9, overrides=None, keypoint_conf=0.3, feet=None):
    """heat-map maxima (idx, score) of 57 channels: `labels` at their projected positions, every other channel below 0.01; overrides: {channel: (idx, score)}"""
    idx = np.zeros(57, np.int32); sc = np.full(57, 0.001, np.float32)
    G = _camera(cam)
    for i in labels:
        idx[i] = _hm_index(*G(*WORLD[i])); sc[i] = score
    for c, (ix, s) in (overrides or {}).items():
        idx[c] = ix; sc[c] = s
    return dict(idx=idx, score=sc, keypoint_conf=keypoint_conf, feet=np.zeros((0, 2), np.int32) if feet is None else np.asarray(feet, np.int32), cam=cam)


# detected sets.  BASE: fourteen points that give the lines x = 0, 16.5, 52.5, 88.5, 105 and y = 0, 68, 13.84, 54.16, 34
BASE = (12, 13, 28, 29, 8, 9, 16, 17, 40, 41, 38, 39, 14, 15)


def _feet_sweep():
    """300 foot points: rows of the frame swept across the pitch's right and bottom limits in 1-pixel steps, and across its left / top limits (pitch
    coordinates in (-1, 0) truncate to 0 and count as inside)"""
    G = _camera("tilt")
    pts = []
    for X0, Y0, dx, dy in ((104.0, 30.0, 1, 0), (50.0, 67.0, 0, 1), (-1.2, 20.0, 1, 0), (60.0, -1.2, 0, 1)):
        u, v = G(X0, Y0)
        pts += [(int(u) + k * dx, int(v) + k * dy) for k in range(75)]
    return np.array(pts, np.int32)


def post_cases():
    nf = np.nextafter
    f32 = np.float32
    corner = HM[0] * HM[1] - 1
    cases = {
        # decode_dedup
        "dedup_different_scores": post_case(BASE, overrides={42: (_hm_index(*_camera("tilt")(*WORLD[14])), 0.95), 43: (_hm_index(*_camera("tilt")(*WORLD[15])), 0.5)}),
        "dedup_equal_scores": post_case(BASE, overrides={42: (_hm_index(*_camera("tilt")(*WORLD[14])), 0.9), 4: (_hm_index(*_camera("tilt")(*WORLD[40])), 0.9)}),
        "score_at_keypoint_conf": post_case(BASE[:10], keypoint_conf=0.5, overrides={38: (_hm_index(*_camera("tilt")(*WORLD[38])), 0.5),
                                                                                    39: (_hm_index(*_camera("tilt")(*WORLD[39])), nf(f32(0.5), f32(0)))}),
        "score_just_above_0_01": post_case(BASE[:10], keypoint_conf=0.005, overrides={38: (_hm_index(*_camera("tilt")(*WORLD[38])), nf(f32(0.01), f32(1))),
                                                                                     39: (_hm_index(*_camera("tilt")(*WORLD[39])), f32(0.01))}),
        "last_row_and_column": post_case(BASE, overrides={42: (corner, 0.9), 43: (corner - HM[1] + 1, 0.8), 48: (HM[1] - 1, 0.7)}),
        # synthesize_block
        "synth_most_candidates": post_case(BASE),
        "synth_one_keypoint": post_case((12,)),
        "synth_no_keypoint": post_case(()),
        "synth_two_point_line": post_case((12, 13, 28)),                                    # x = 0 and y = 0 have exactly two points each, nothing to add; 3 points: no H
        "synth_parallel_lines": post_case(BASE[:8], overrides={38: (30 * 240 + 40, 0.9), 39: (30 * 240 + 90, 0.9),        # y = 34 drawn horizontal ...
                                                                           40: (60 * 240 + 50, 0.9), 41: (60 * 240 + 100, 0.9)}),    # ... and x = 52.5 horizontal too
        # write_bounds / project_detections
        "bounds_none_axis_camera": post_case(BASE, cam="axis", feet=[(625, 346), (100, 40), (1150, 652), (99, 39), (1160, 660)]),
        "bounds_and_pitch_limits": post_case(BASE, cam="tilt", feet=_feet_sweep()),
    }
    return cases


def post_expected(case):
    """the oracle's chain on one case -> dict(idx, score, detected, synth, H, kept, bounds, pitch [(xf, yf, x, y, in_bounds)] per foot point).  The homography is
    cv2.RANSAC's restatement alone (the GPU runs no RHO / LMEDS fallback): a case on which it fails with four or more points is not a valid case."""
    from oracle import host, prims as P
    fh, fw = FRAME
    dec = host.decode_heatmaps(case["idx"], case["score"], HM[0], HM[1])
    kps = host.keypoints_from_decoded(dec, fh, fw, case["keypoint_conf"])
    detected = dict(kps)
    if len(kps) >= 2:
        kps = host.synthesize_keypoints(kps)
    synth = dict(kps)
    img, world, used = host.select_plane_points(kps)
    H = mask = None
    if len(img) >= 4:
        H, mask = P.find_homography_ransac(img, world, 5.0)
    pitch = []
    if H is not None and len(case["feet"]):
        tf = P.perspective_transform(case["feet"].astype(np.float32), H)
        for xf, yf in tf:
            tx, ty = int(xf), int(yf)
            pitch.append((xf, yf, tx, ty, not (tx < 0 or tx > 105 or ty < 0 or ty > 68)))
    return dict(detected=detected, synth=synth, H=H, mask=mask, used=used, n_plane=len(img), bounds=host.boundaries(H, fh, fw), pitch=pitch)


def synthesis_candidate_bound():
    """An upper bound on the points synthesis can add to ANY dict: a candidate is an undetected labelled point whose x-group and y-group each hold two OTHER,
    detected points, i.e. both groups have three or more members."""
    from oracle import host
    from eagle_amd.pitch import GROUND_TRUTH_POINTS
    _, xg, yg = host._GROUPS
    n = 0
    for lab, (x, y, z) in GROUND_TRUTH_POINTS.items():
        if z == 0.0 and len(xg[round(float(x), 2)]) >= 3 and len(yg[round(float(y), 2)]) >= 3:
            n += 1
    return n
