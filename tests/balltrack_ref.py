"""The ball track (K35) written down: which ball candidate of every frame lies on the best physically possible path through the clip.  This file is the
definition of every bit eagle_op_ball_track / eagle_ball_track return (include/eagle.h, csrc/balltrack.hip); the rule is the project's own and runs
in integers only, so no order of accumulation exists.

Inputs: per frame a count of candidates in descending confidence (the first MAX_CAND = 8 are nodes, the others are ignored and the frame is
flagged), per candidate a position in half pixels (qx, qy) and a confidence cq = floor(conf * 1024); the sorted frames that start a new shot.
Resolved parameters (resolve): V half pixels per frame, G frames, R0 and B half pixels.

    R(i, a) = (cq * R0) >> 10
    a link (i, a) -> (j, b): i < j <= i + G, one shot, d2 = dx^2 + dy^2 <= (V (j - i))^2; it costs isqrt(d2)
    f(j, b) = R(j, b) + max(P(j - 1) - B, max over links of f(i, a) - cost)          per shot, P(-1) = 0
    P(j)    = max(P(j - 1), max_b f(j, b))

A link is taken when it is at least as good as the break; among links the larger i wins, then the smaller a; P's arg-max moves only on a strictly
greater f, within a frame to the lowest b; a break's predecessor is that arg-max when P(j - 1) > 0, else none.  Per shot with P(end) > 0 the chosen
nodes are the predecessors back from the arg-max.  A tracklet is a maximal run of chosen nodes joined by links.

The rule is written twice: track_loop walks node by node in plain Python, track_window takes each node's whole window as numpy arrays and puts the
outputs together with array operations.  enumerate_best tries every choice of a tiny clip.  split_at_empty_runs is the argument the forward kernel
leans on: no link crosses G candidate-free frames, so the timeline may be cut there and every f behind the cut is f of the piece plus P before it."""
import itertools
import math

import numpy as np

MAX_CAND = 8
TOO_MANY, SHOT_START, TRACKLET_START = 1, 2, 4
MAX_FRAMES, MAX_GAP, MAX_Q, MAX_CQ = 1 << 20, 64, 2 * 65535, 1024
MAX_SPEED, MAX_REWARD, MAX_BREAK = 65535.0, 65535.0, float(1 << 20)

FRAME_DTYPE = np.dtype([("cand", "<i4"), ("det", "<i4"), ("tracklet", "<i4"), ("flags", "<i4"), ("qx", "<i4"), ("qy", "<i4"), ("f", "<i8")])     # EagleBallFrame (32 bytes)
TRACKLET_DTYPE = np.dtype([("first", "<i4"), ("last", "<i4"), ("shot", "<i4"), ("sightings", "<i4"), ("sum_cq", "<i8"), ("length", "<i8"), ("gain", "<i8"),
                           ("reserved", "<i4", 2)])                                                                                               # EagleBallTracklet (48 bytes)
CLIP_DTYPE = np.dtype([("frames_with", "<i4"), ("frames_chosen", "<i4"), ("rejected", "<i4"), ("frames_multi", "<i4"), ("tracklets", "<i4"), ("shots", "<i4"),
                       ("ignored", "<i4"), ("reserved", "<i4"), ("score", "<i8"), ("V", "<i4"), ("G", "<i4"), ("R0", "<i4"), ("B", "<i4"), ("reserved2", "<i4", 2)])  # EagleBallClip (64 bytes)


def quantise(v):
    """pixels -> half pixels"""
    return int(math.floor(2.0 * float(v) + 0.5))


def resolve(fps, frame_w, speed=0.0, gap=0, reward=0.0, brk=0.0):
    """-> (V, G, R0, B); 0 stands for the default.  The defaults are conventional choices, not fitted to data: a tenth of the frame's width per frame (the
    reference filter's threshold), a second of frames, a reward equal to the speed, a break of two and a half rewards."""
    if fps <= 0 or frame_w <= 0 or not 0 <= gap <= MAX_GAP:
        raise ValueError("fps, frame_w or gap")
    for v, top in ((speed, MAX_SPEED), (reward, MAX_REWARD), (brk, MAX_BREAK)):
        if not (math.isfinite(v) and 0 <= v <= top):
            raise ValueError("speed, reward or break")
    V = quantise(speed) if speed else quantise(0.1 * float(frame_w))
    G = gap if gap else min(MAX_GAP, fps)
    R0 = quantise(reward) if reward else V
    B = quantise(brk) if brk else (5 * R0) >> 1
    if V > 2 * 65535 or R0 > 2 * 65535:
        raise ValueError("frame_w")
    return V, G, R0, B


def cq_of_conf(conf):
    conf = np.asarray(conf, np.float32)
    if not (np.isfinite(conf).all() and (conf >= 0).all() and (conf <= 1).all()):
        raise ValueError("conf")
    return np.floor(conf.astype(np.float64) * 1024.0).astype(np.int32)                 # (float32 * 1024 is exact in either format)


def check_cuts(n, cuts):
    cuts = [int(c) for c in cuts]
    if any(c < 1 or c > n - 1 for c in cuts) or any(a >= b for a, b in zip(cuts, cuts[1:])):
        raise ValueError("cuts")
    return cuts


def _inputs(counts, pos, cq, det, cuts):
    counts = np.asarray(counts, np.int64).reshape(-1)
    n = len(counts)
    total = int(counts.sum())
    pos = np.asarray(pos, np.int64).reshape(total, 2)
    cq = np.asarray(cq, np.int64).reshape(total)
    det = np.full(total, -1, np.int64) if det is None else np.asarray(det, np.int64).reshape(total)
    if n > MAX_FRAMES or (counts < 0).any() or (pos < 0).any() or (pos > MAX_Q).any() or (cq < 0).any() or (cq > MAX_CQ).any():
        raise ValueError("counts, positions or confidences")
    return counts, pos, cq, det, check_cuts(n, cuts)


def _shots(n, cuts):
    edges = [0] + list(cuts) + [n]
    return [(edges[k], edges[k + 1]) for k in range(len(edges) - 1)] if n else []


def isqrt(v):
    return math.isqrt(int(v))


# ---- the first definition: node by node ------------------------------------------------------------------------------------------------------
def track_loop(counts, pos, cq, V, G, R0, B, cuts=(), det=None):
    counts, pos, cq, det, cuts = _inputs(counts, pos, cq, det, cuts)
    n = len(counts)
    start = [0] * (n + 1)
    for i in range(n):
        start[i + 1] = start[i] + int(counts[i])
    m = [min(int(c), MAX_CAND) for c in counts]
    f = [[0] * m[i] for i in range(n)]
    pred = [[None] * m[i] for i in range(n)]           # None | ("link", i, a) | ("break", i, a)
    frames = np.zeros(n, FRAME_DTYPE)
    frames["cand"] = frames["det"] = frames["tracklet"] = -1
    tracklets, score = [], 0
    for s, (s0, s1) in enumerate(_shots(n, cuts)):
        P, parg = 0, None
        for j in range(s0, s1):
            for b in range(m[j]):
                xb, yb = (int(v) for v in pos[start[j] + b])
                best = None                            # (value, i, a)
                for i in range(j - 1, max(s0, j - G) - 1, -1):
                    lim = (V * (j - i)) ** 2
                    for a in range(m[i]):
                        xa, ya = (int(v) for v in pos[start[i] + a])
                        d2 = (xb - xa) ** 2 + (yb - ya) ** 2
                        if d2 > lim:
                            continue
                        v = f[i][a] - isqrt(d2)
                        if best is None or v > best[0]:                    # the larger i, then the smaller a: the first met
                            best = (v, i, a)
                R = (int(cq[start[j] + b]) * R0) >> 10
                if best is not None and best[0] >= P - B:
                    f[j][b], pred[j][b] = R + best[0], ("link", best[1], best[2])
                else:
                    f[j][b], pred[j][b] = R + P - B, (("break",) + parg if P > 0 else None)
            for b in range(m[j]):
                if f[j][b] > P:
                    P, parg = f[j][b], (j, b)
        score += P
        if P <= 0:
            continue
        path, node = [], parg
        while node is not None:
            j, b = node
            p = pred[j][b]
            path.append((j, b, p is not None and p[0] == "link"))
            node = None if p is None else (p[1], p[2])
        for j, b, linked in path:
            r = frames[j]
            r["cand"], r["det"], r["qx"], r["qy"], r["f"] = b, det[start[j] + b], pos[start[j] + b][0], pos[start[j] + b][1], f[j][b]
            if not linked:
                r["flags"] |= TRACKLET_START
    for s0, _ in _shots(n, cuts):
        frames[s0]["flags"] |= SHOT_START
    shot_of = lambda j: sum(1 for c in cuts if c <= j)
    last = None
    for j in range(n):
        r = frames[j]
        if counts[j] > MAX_CAND:
            r["flags"] |= TOO_MANY
        if r["cand"] < 0:
            continue
        k = start[j] + int(r["cand"])
        R = (int(cq[k]) * R0) >> 10
        if r["flags"] & TRACKLET_START:
            tracklets.append(dict(first=j, last=j, shot=shot_of(j), sightings=0, sum_cq=0, length=0, gain=-B))
        else:
            c = isqrt((int(r["qx"]) - int(frames[last]["qx"])) ** 2 + (int(r["qy"]) - int(frames[last]["qy"])) ** 2)
            tracklets[-1]["length"] += c
            tracklets[-1]["gain"] -= c
        t = tracklets[-1]
        t["last"] = j; t["sightings"] += 1; t["sum_cq"] += int(cq[k]); t["gain"] += R
        r["tracklet"] = len(tracklets) - 1
        last = j
    tr = np.zeros(len(tracklets), TRACKLET_DTYPE)
    for k, t in enumerate(tracklets):
        for key, v in t.items():
            tr[k][key] = v
    clip = np.zeros(1, CLIP_DTYPE)
    c = clip[0]
    chosen = int((frames["cand"] >= 0).sum())
    c["frames_with"], c["frames_chosen"], c["rejected"], c["frames_multi"] = int((counts > 0).sum()), chosen, sum(m) - chosen, int((counts > 1).sum())
    c["tracklets"], c["shots"], c["ignored"], c["score"] = len(tracklets), len(_shots(n, cuts)), int(counts.sum()) - sum(m), score
    c["V"], c["G"], c["R0"], c["B"] = V, G, R0, B
    return frames, tr, clip


# ---- the second definition: a window of arrays per node, the outputs by array operations --------------------------------------------------------
def isqrt_array(d2):
    r = np.floor(np.sqrt(d2.astype(np.float64))).astype(np.int64)
    r -= (r * r > d2)
    r += ((r + 1) * (r + 1) <= d2)
    assert ((r * r <= d2) & ((r + 1) * (r + 1) > d2)).all()
    return r


def forward_window(counts, pos, cq, V, G, R0, B, s0, s1, start, m, f, pred, P0=0):
    """the recurrence over frames s0 .. s1 - 1 from P(s0 - 1) = P0 without an arg-max; fills f and pred (node index; -1: none; -2 - k: a break from
    node k) -> (P, arg-max node or -1).  The nodes in flat order: node = nstart[j] + b"""
    nstart, fr = start
    P, parg = P0, -1
    for j in range(s0, s1):
        if not m[j]:
            continue
        lo, hi = nstart[max(s0, j - G)], nstart[j]
        # the window newest frame first, within a frame a ascending: the first maximum is the tie rule
        order = np.lexsort((np.arange(lo, hi), -fr[lo:hi])) + lo if hi > lo else np.zeros(0, np.int64)
        wp, wf, wd = pos[order], f[order], j - fr[order]
        for b in range(m[j]):
            k = nstart[j] + b
            R = (int(cq[k]) * R0) >> 10
            link = None
            if len(order):
                d = wp - pos[k]
                d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
                ok = d2 <= (V * wd) ** 2
                if ok.any():
                    val = np.where(ok, wf - isqrt_array(d2), np.iinfo(np.int64).min)
                    w = int(np.argmax(val))
                    link = (int(val[w]), int(order[w]))
            if link is not None and link[0] >= P - B:
                f[k], pred[k] = R + link[0], link[1]
            else:
                f[k], pred[k] = R + P - B, (-2 - parg if P > 0 and parg >= 0 else -1)
        fj = f[nstart[j]:nstart[j] + m[j]]
        if fj.max() > P:
            parg = int(nstart[j] + np.argmax(fj))
            P = int(fj.max())
    return P, parg


def _nodes(counts, pos, cq, det):
    """the candidates that are nodes, flat: (first node of every frame [n + 1], frame of every node), positions, cq, det, candidate index"""
    n = len(counts)
    m = np.minimum(counts, MAX_CAND)
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    nstart = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    fr = np.repeat(np.arange(n), m)
    b = np.arange(int(m.sum())) - nstart[fr]
    src = first[fr] + b
    return m, (nstart, fr), pos[src], cq[src], det[src], b


def track_window(counts, pos, cq, V, G, R0, B, cuts=(), det=None, split=False):
    """split: cut every shot at its runs of at least G candidate-free frames and run each piece from P = 0 (split_at_empty_runs)"""
    counts, pos, cq, det, cuts = _inputs(counts, pos, cq, det, cuts)
    n = len(counts)
    m, start, npos, ncq, ndet, nb = _nodes(counts, pos, cq, det)
    nstart, fr = start
    N = len(fr)
    f, pred = np.zeros(N, np.int64), np.full(N, -1, np.int64)
    ends, score = [], 0
    for s0, s1 in _shots(n, cuts):
        if split:
            P, parg = 0, -1
            for p0, p1 in split_at_empty_runs(m, s0, s1, G):
                Pp, ap = forward_window(counts, npos, ncq, V, G, R0, B, p0, p1, start, m, f, pred)
                k0, k1 = nstart[p0], nstart[p1]
                if P > 0:                              # what the piece could not know: P before it, and the arg-max a break goes back to
                    f[k0:k1] += P
                    none = np.flatnonzero(pred[k0:k1] == -1) + k0
                    pred[none] = -2 - parg
                if Pp > 0:
                    P, parg = P + Pp, ap
        else:
            P, parg = forward_window(counts, npos, ncq, V, G, R0, B, s0, s1, start, m, f, pred)
        score += P
        if P > 0:
            ends.append(parg)
    chosen = np.zeros(N, bool)
    for k in ends:
        while k >= 0:
            chosen[k] = True
            k = pred[k] if pred[k] >= 0 else -2 - pred[k] if pred[k] <= -2 else -1
    frames = np.zeros(n, FRAME_DTYPE)
    frames["cand"] = frames["det"] = frames["tracklet"] = -1
    ck = np.flatnonzero(chosen)
    cf = fr[ck]
    assert len(np.unique(cf)) == len(cf)
    frames["cand"][cf], frames["det"][cf], frames["qx"][cf], frames["qy"][cf], frames["f"][cf] = nb[ck], ndet[ck], npos[ck, 0], npos[ck, 1], f[ck]
    starts = pred[ck] < 0
    frames["flags"][cf[starts]] |= TRACKLET_START
    if n:
        frames["flags"][[0] + cuts] |= SHOT_START
    frames["flags"][counts > MAX_CAND] |= TOO_MANY
    tid = np.cumsum(starts) - 1
    frames["tracklet"][cf] = tid
    nt = int(starts.sum())
    tr = np.zeros(nt, TRACKLET_DTYPE)
    if nt:
        R = (ncq[ck] * R0) >> 10
        prev = np.maximum(np.arange(len(ck)) - 1, 0)
        d = npos[ck] - npos[ck[prev]]
        cost = np.where(starts, 0, isqrt_array(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
        tr["first"] = cf[starts]
        tr["last"] = cf[np.concatenate([np.flatnonzero(starts)[1:] - 1, [len(ck) - 1]])]
        tr["shot"] = np.searchsorted(np.asarray(cuts, np.int64), tr["first"], side="right")
        tr["sightings"] = np.bincount(tid, minlength=nt)
        for key, w in (("sum_cq", ncq[ck]), ("length", cost), ("gain", R - cost)):
            acc = np.zeros(nt, np.int64)
            np.add.at(acc, tid, w)
            tr[key] = acc
        tr["gain"] -= B
    clip = np.zeros(1, CLIP_DTYPE)
    c = clip[0]
    c["frames_with"], c["frames_chosen"], c["rejected"], c["frames_multi"] = int((counts > 0).sum()), len(ck), N - len(ck), int((counts > 1).sum())
    c["tracklets"], c["shots"], c["ignored"], c["score"] = nt, len(_shots(n, cuts)), int(counts.sum()) - N, score
    c["V"], c["G"], c["R0"], c["B"] = V, G, R0, B
    return frames, tr, clip


def split_at_empty_runs(m, s0, s1, G):
    """the pieces [p0, p1) of the shot [s0, s1): from a frame with candidates to the last one before at least G frames without"""
    have = [j for j in range(s0, s1) if m[j]]
    pieces = []
    for j in have:
        if pieces and j - pieces[-1][1] <= G:          # (a link j - i <= G is possible)
            pieces[-1][1] = j
        else:
            pieces.append([j, j])
    return [(a, b + 1) for a, b in pieces]


# ---- every choice of a tiny clip --------------------------------------------------------------------------------------------------------------
def enumerate_best(counts, pos, cq, V, G, R0, B, cuts=()):
    """the greatest score over every way to choose at most one node per frame: a shot's score is the greatest prefix of its sightings' running total
    (reward, minus the link's cost where a link to the sighting before is admissible and no dearer than a break, minus B otherwise) or 0"""
    counts, pos, cq, _, cuts = _inputs(counts, pos, cq, None, cuts)
    n = len(counts)
    first = np.concatenate([[0], np.cumsum(counts)])
    total = 0
    for s0, s1 in _shots(n, cuts):
        best = 0
        options = [[None] + list(range(min(int(counts[j]), MAX_CAND))) for j in range(s0, s1)]
        for choice in itertools.product(*options):
            run, last = 0, None
            for j, b in zip(range(s0, s1), choice):
                if b is None:
                    continue
                k = first[j] + b
                step = B
                if last is not None and j - last[0] <= G:
                    d2 = int((pos[k][0] - pos[last[1]][0]) ** 2 + (pos[k][1] - pos[last[1]][1]) ** 2)
                    if d2 <= (V * (j - last[0])) ** 2:
                        step = min(B, isqrt(d2))
                run += ((int(cq[k]) * R0) >> 10) - step
                last = (j, k)
                best = max(best, run)
        total += best
    return total


# ---- the nodes of a clip's records ------------------------------------------------------------------------------------------------------------
def candidates_of_records(recs):
    """NODES of include/eagle.h: per record the reported ball detections, one per id (a later record of an id in the earlier one's place), stably by
    descending confidence -> (counts [n], positions [sum, 2] half pixels, cq [sum], det [sum]: the index in the record's det)"""
    counts, pos, conf, det = [], [], [], []
    for r in recs:
        ids, ks = [], []
        for k in range(int(r["n_det"])):
            d = r["det"][k]
            if int(d["cls"]) != 2 or not d["reported"]:
                continue
            if int(d["id"]) in ids:
                ks[ids.index(int(d["id"]))] = k
            else:
                ids.append(int(d["id"])); ks.append(k)
        ks.sort(key=lambda k: -float(r["det"][k]["conf"]))                 # (stable)
        counts.append(len(ks))
        for k in ks:
            d = r["det"][k]
            pos.append(((int(d["bx1"]) & 0xFFFF) + (int(d["bx2"]) & 0xFFFF), 2 * (int(d["by2"]) & 0xFFFF)))
            conf.append(d["conf"]); det.append(k)
    return (np.array(counts, np.int32), np.array(pos, np.int32).reshape(-1, 2), cq_of_conf(np.array(conf, np.float32)), np.array(det, np.int32))
