"""The contract of the team clustering (include/eagle.h, eagle_team_cluster; csrc/kits.hip), defined twice: vectorised (``team_cluster``,
``cluster_ids``) and pixel by pixel, id by id and pair by pair in plain loops (``team_cluster_loop``, ``cluster_ids_loop``).  The two must agree on
every bit; the kernels must equal them, tobytes(), no tolerance.  Everything is in integers, so no order of accumulation matters.

The rule (the constants are conventional choices, not fitted to data):
  1. a crop (frame, x1, y1, x2, y2) carries the slot of its id, 0 .. n_ids - 1;
  2. with w = x2 - x1 and h = y2 - y1 the shirt window is rows [y1 + h // 5, y1 + h // 2) and columns [x1 + w // 4, x2 - w // 4).  An empty crop or an
     empty window (flag EMPTY), a crop that leaves the frame or names a frame outside the clip (flag OUTSIDE) give zeros;
  3. a pixel with g >= 48 and g - max(r, b) >= 16 is grass and does not count.  Every other pixel gets OpenCV's 8-bit HSV in the fixed-point form of
     csrc/teams.hip.  With s >= 64 and v >= 48 it is chromatic: t = (h + 174) % 180, k = t // 12, f = t % 12, 12 - f units go to hue bin k and f units
     to hue bin (k + 1) % 15, in the lower 15 bins for v < 144 and in the upper 15 otherwise.  Any other pixel puts 12 units into bin 30 + v // 64;
  4. n is the number of counted pixels; a crop with n < min_pixels is skipped (flag FEW, its units and n are reported); otherwise
     q[b] = units[b] * 4096 // (12 n);
  5. per id sum[b] is the sum of q[b] over its used crops, ``used`` their number, ``skipped`` the number of its other crops; with used > 0,
     p[b] = sum[b] * 65536 // T with T the sum of sum[b];
  6. D(i, j) = sum_b |p_i[b] - p_j[b]| (at most 131072);
  7. the voters are the ids with used >= min_crops, of weight w_i = used;
  8. for every pair of voters a < b in slot order cost(a, b) = sum over the voters of w_i min(D(i, a), D(i, b)); the least cost wins, ties go to the
     earlier pair in (a, b) order;
  9. every id with used > 0 goes to the nearer medoid, equal distances to a; a non-voter is flagged WEAK; with outlier > 0 an id is NEITHER (team -1)
     when d_near * 1024 > outlier * D(a, b);
 10. team 0 is the cluster with the larger sum of w over its voters that are not neither, on a tie the cluster of a;
 11. with fewer than two voters every id with crops is team 0 and flagged SINGLE (a = b = -1); zero ids give empty records and that model."""
import numpy as np

BINS = 34
CROP_OUTSIDE, CROP_EMPTY, CROP_FEW = 1, 2, 4
ID_WEAK, ID_NEITHER, ID_SINGLE = 1, 2, 4
MODEL_SINGLE, MODEL_SWAPPED = 1, 2
MAX_IDS, MAX_CROPS = 1024, 1 << 22
DEFAULTS = dict(min_pixels=32, min_crops=3, outlier=512)
RANGES = dict(min_pixels=(1, 1 << 20), min_crops=(1, 1 << 16), outlier=(0, 1 << 20))
MAX_SUM = 1 << 34                                    # 4096 per crop, 2^22 crops

CROP_DTYPE = np.dtype([("units", "<u4", BINS), ("n", "<i4"), ("flags", "<i4")])                                                                   # EagleKitCrop (144 bytes)
ID_DTYPE = np.dtype([("used", "<i4"), ("skipped", "<i4"), ("team", "<i4"), ("flags", "<i4"), ("d", "<u4", 2), ("p", "<u4", BINS)])                # EagleKitId (160 bytes)
MODEL_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("dab", "<u4"), ("voters", "<i4"), ("cost", "<i8"), ("w", "<i8", 2), ("neither", "<i4"), ("flags", "<i4"),
                        ("team_of_a", "<i4"), ("reserved", "<i4", 3)])                                                                            # EagleKitModel (64 bytes)


def resolve(min_pixels=None, min_crops=None, outlier=None):
    """-> (min_pixels, min_crops, outlier); None: the default.  Out of range: ValueError, as the library refuses it."""
    got = dict(min_pixels=min_pixels, min_crops=min_crops, outlier=outlier)
    out = []
    for k in ("min_pixels", "min_crops", "outlier"):
        v = DEFAULTS[k] if got[k] is None else int(got[k])
        if not RANGES[k][0] <= v <= RANGES[k][1]:
            raise ValueError(f"{k} {v} is outside {RANGES[k][0]} .. {RANGES[k][1]}")
        out.append(v)
    return tuple(out)


# ---- pixels -------------------------------------------------------------------------------------------------------------------------------------
def hsv_px(b, g, r):
    """cv2's 8-bit BGR2HSV of one pixel, the fixed-point form of csrc/teams.hip (bgr2hsv_px)"""
    v, vmin = max(b, g, r), min(b, g, r)
    diff = v - vmin
    sdiv = int(np.rint((255 << 12) / float(v))) if v else 0
    hdiv = int(np.rint((180 << 12) / (6.0 * diff))) if diff else 0
    s = (diff * sdiv + (1 << 11)) >> 12
    if v == r:
        hh = g - b
    elif v == g:
        hh = b - r + 2 * diff
    else:
        hh = r - g + 4 * diff
    hh = (hh * hdiv + (1 << 11)) >> 12
    if hh < 0:
        hh += 180
    return hh & 255, s & 255, v


def hsv_array(bgr):
    """the same for int64 [..., 3]"""
    bgr = np.asarray(bgr).astype(np.int64)
    b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
    v, vmin = np.maximum(np.maximum(b, g), r), np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    sdiv = np.where(v > 0, np.rint((255 << 12) / np.maximum(v, 1).astype(np.float64)), 0).astype(np.int64)
    hdiv = np.where(diff > 0, np.rint((180 << 12) / (6.0 * np.maximum(diff, 1).astype(np.float64))), 0).astype(np.int64)
    s = (diff * sdiv + (1 << 11)) >> 12
    hh = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    hh = (hh * hdiv + (1 << 11)) >> 12
    hh = hh + np.where(hh < 0, 180, 0)
    return hh & 255, s & 255, v


def pixel_units(b, g, r):
    """-> [(bin, units)] of one pixel, [] for grass"""
    if g >= 48 and g - max(r, b) >= 16:
        return []
    h, s, v = hsv_px(b, g, r)
    if s >= 64 and v >= 48:
        t = (h + 174) % 180
        k, f = t // 12, t % 12
        base = 0 if v < 144 else 15
        return [(base + k, 12 - f), (base + (k + 1) % 15, f)]
    return [(30 + v // 64, 12)]


def window_of(crop, n_frames, fh, fw):
    """-> (flag, rows, columns): flag 0 and the half-open ranges of the shirt window, or the flag that skips the crop"""
    f, x1, y1, x2, y2 = (int(v) for v in crop)
    w, h = x2 - x1, y2 - y1
    if w <= 0 or h <= 0:
        return CROP_EMPTY, None, None
    if f < 0 or f >= n_frames or x1 < 0 or y1 < 0 or x2 > fw or y2 > fh:
        return CROP_OUTSIDE, None, None
    rows, cols = (y1 + h // 5, y1 + h // 2), (x1 + w // 4, x2 - w // 4)
    if rows[1] <= rows[0] or cols[1] <= cols[0]:
        return CROP_EMPTY, None, None
    return 0, rows, cols


def crop_record_loop(frames, crop, min_pixels):
    """-> (units [34], n, flags), pixel by pixel"""
    flag, rows, cols = window_of(crop, *frames.shape[:3])
    units, n = [0] * BINS, 0
    if flag:
        return units, 0, flag
    for y in range(*rows):
        for x in range(*cols):
            b, g, r = (int(v) for v in frames[int(crop[0]), y, x])
            got = pixel_units(b, g, r)
            for k, u in got:
                units[k] += u
            n += 1 if got else 0
    return units, n, CROP_FEW if n < min_pixels else 0


def crop_record(frames, crop, min_pixels):
    """the same, vectorised"""
    flag, rows, cols = window_of(crop, *frames.shape[:3])
    if flag:
        return np.zeros(BINS, np.int64), 0, flag
    px = frames[int(crop[0]), rows[0]:rows[1], cols[0]:cols[1]].reshape(-1, 3).astype(np.int64)
    b, g, r = px[:, 0], px[:, 1], px[:, 2]
    keep = ~((g >= 48) & (g - np.maximum(r, b) >= 16))
    h, s, v = hsv_array(px)
    chroma = keep & (s >= 64) & (v >= 48)
    grey = keep & ~chroma
    t = (h + 174) % 180
    k, f = t // 12, t % 12
    base = np.where(v < 144, 0, 15)
    units = np.zeros(BINS, np.int64)
    np.add.at(units, (base + k)[chroma], (12 - f)[chroma])
    np.add.at(units, (base + (k + 1) % 15)[chroma], f[chroma])
    np.add.at(units, (30 + v // 64)[grey], 12)
    n = int(keep.sum())
    return units, n, CROP_FEW if n < min_pixels else 0


def _accumulate(frames, crops, slots, n_ids, min_pixels, record):
    crops = np.asarray(crops, np.int64).reshape(-1, 5)
    slots = np.asarray(slots, np.int64).reshape(-1)
    if n_ids > MAX_IDS or len(crops) > MAX_CROPS or len(slots) != len(crops) or (len(slots) and not (0 <= slots.min() and slots.max() < n_ids)):
        raise ValueError("ids, crops or slots outside the caps")
    recs = np.zeros(len(crops), CROP_DTYPE)
    sums = [[0] * BINS for _ in range(n_ids)]
    used, skipped = [0] * n_ids, [0] * n_ids
    for i, (crop, slot) in enumerate(zip(crops, slots)):
        units, n, flag = record(frames, crop, min_pixels)
        recs[i]["units"], recs[i]["n"], recs[i]["flags"] = [int(u) for u in units], n, flag
        if flag:
            skipped[slot] += 1
            continue
        used[slot] += 1
        for b in range(BINS):
            sums[slot][b] += int(units[b]) * 4096 // (12 * n)
    return recs, np.array(sums, np.int64).reshape(n_ids, BINS), np.array(used, np.int64), np.array(skipped, np.int64)


# ---- ids ----------------------------------------------------------------------------------------------------------------------------------------
def _check_ids(sums, used):
    sums = np.asarray(sums, np.int64).reshape(-1, BINS)
    used = np.asarray(used, np.int64).reshape(-1)
    if len(sums) != len(used) or len(used) > MAX_IDS or (sums < 0).any() or (sums > MAX_SUM).any() or (used < 0).any() or (used > MAX_CROPS).any():
        raise ValueError("sums or used outside the caps")
    if used.sum() > MAX_CROPS:
        raise ValueError("more crops in all than the cap: the packed key would not hold the cost")
    if ((used > 0) & (sums.sum(1) == 0)).any():
        raise ValueError("an id with crops and no colour")
    return sums, used


def _single_model(voters, w0):
    m = np.zeros(1, MODEL_DTYPE)
    m[0]["a"], m[0]["b"], m[0]["voters"], m[0]["flags"] = -1, -1, voters, MODEL_SINGLE
    m[0]["w"][0] = w0
    return m


def cluster_ids_loop(sums, used, skipped=None, min_pixels=None, min_crops=None, outlier=None):
    """steps 5 to 11 in plain loops -> (ID_DTYPE [n_ids], MODEL_DTYPE [1]).  (Above 65 voters the inner sum over the voters of one pair's cost is a
    numpy dot product of int64: a thousand voters make half a million pairs.)"""
    _, min_crops, outlier = resolve(min_pixels, min_crops, outlier)
    sums, used = _check_ids(sums, used)
    n = len(used)
    skipped = np.zeros(n, np.int64) if skipped is None else np.asarray(skipped, np.int64)
    ids = np.zeros(n, ID_DTYPE)
    p = []
    for i in range(n):
        T = sum(int(v) for v in sums[i])
        p.append([int(v) * 65536 // T for v in sums[i]] if used[i] > 0 else [0] * BINS)
        ids[i]["used"], ids[i]["skipped"], ids[i]["team"], ids[i]["p"] = used[i], skipped[i], -1, p[i]
    dist = lambda i, j: sum(abs(x - y) for x, y in zip(p[i], p[j]))
    voters = [i for i in range(n) if used[i] >= min_crops]
    if len(voters) < 2:
        for i in range(n):
            if used[i] > 0:
                ids[i]["team"], ids[i]["flags"] = 0, ID_SINGLE | (0 if used[i] >= min_crops else ID_WEAK)
        return ids, _single_model(len(voters), sum(int(used[i]) for i in voters))
    D = [[dist(i, j) for j in voters] for i in voters]
    w = [int(used[i]) for i in voters]
    best = None
    if len(voters) <= 65:
        for x in range(len(voters)):
            for y in range(x + 1, len(voters)):
                cost = 0
                for t in range(len(voters)):
                    cost += w[t] * min(D[t][x], D[t][y])
                if best is None or cost < best[0]:
                    best = (cost, x, y)
    else:
        Dn, wn = np.array(D, np.int64), np.array(w, np.int64)
        for x in range(len(voters)):
            for y in range(x + 1, len(voters)):
                cost = int(np.minimum(Dn[x], Dn[y]).dot(wn))
                if best is None or cost < best[0]:
                    best = (cost, x, y)
    cost, a, b = best[0], voters[best[1]], voters[best[2]]
    dab = dist(a, b)
    cluster, neither, wsum = {}, {}, [0, 0]
    for i in range(n):
        if used[i] <= 0:
            continue
        da, db = dist(i, a), dist(i, b)
        cluster[i] = 1 if db < da else 0
        neither[i] = outlier > 0 and min(da, db) * 1024 > outlier * dab
        if used[i] >= min_crops and not neither[i]:
            wsum[cluster[i]] += int(used[i])
    swap = 1 if wsum[1] > wsum[0] else 0
    for i in cluster:
        team = cluster[i] ^ swap
        ids[i]["d"] = (dist(i, b), dist(i, a)) if swap else (dist(i, a), dist(i, b))          # d[k]: to the medoid of team k
        ids[i]["team"] = -1 if neither[i] else team
        ids[i]["flags"] = (0 if used[i] >= min_crops else ID_WEAK) | (ID_NEITHER if neither[i] else 0)
    m = np.zeros(1, MODEL_DTYPE)
    m[0]["a"], m[0]["b"], m[0]["dab"], m[0]["voters"], m[0]["cost"], m[0]["neither"] = a, b, dab, len(voters), cost, sum(neither.values())
    m[0]["w"], m[0]["flags"], m[0]["team_of_a"] = (wsum[swap], wsum[1 - swap]), MODEL_SWAPPED if swap else 0, swap
    return ids, m


def cluster_ids(sums, used, skipped=None, min_pixels=None, min_crops=None, outlier=None):
    """steps 5 to 11, vectorised -> (ID_DTYPE [n_ids], MODEL_DTYPE [1])"""
    _, min_crops, outlier = resolve(min_pixels, min_crops, outlier)
    sums, used = _check_ids(sums, used)
    n = len(used)
    ids = np.zeros(n, ID_DTYPE)
    ids["used"], ids["skipped"], ids["team"] = used, 0 if skipped is None else skipped, -1
    have = used > 0
    T = np.where(have, sums.sum(1), 1)
    p = np.where(have[:, None], sums * 65536 // T[:, None], 0)
    ids["p"] = p
    vot = np.nonzero(used >= min_crops)[0]
    weak = np.where(used >= min_crops, 0, ID_WEAK)
    if len(vot) < 2:
        ids["team"][have], ids["flags"][have] = 0, (ID_SINGLE | weak)[have]
        return ids, _single_model(len(vot), int(used[vot].sum()))
    pv, w = p[vot], used[vot]
    D = np.abs(pv[:, None, :] - pv[None, :, :]).sum(2)                       # [voter t, voter x]
    best = None
    for x in range(len(vot) - 1):
        cost = (np.minimum(D[:, x, None], D[:, x + 1:]) * w[:, None]).sum(0)
        y = int(np.argmin(cost))                                              # (the first of equal costs)
        if best is None or int(cost[y]) < best[0]:
            best = (int(cost[y]), x, x + 1 + y)
    a, b = int(vot[best[1]]), int(vot[best[2]])
    da, db = np.abs(p - p[a]).sum(1), np.abs(p - p[b]).sum(1)
    dab = int(da[b])
    cluster = (db < da).astype(np.int64)
    neither = have & (np.minimum(da, db) * 1024 > outlier * dab) if outlier > 0 else np.zeros(n, bool)
    counts = have & (used >= min_crops) & ~neither
    wsum = [int(used[counts & (cluster == k)].sum()) for k in (0, 1)]
    swap = 1 if wsum[1] > wsum[0] else 0
    team = cluster ^ swap
    d = np.stack([np.where(team == cluster, da, db), np.where(team == cluster, db, da)], 1)
    ids["d"][have] = d[have]
    ids["team"][have] = np.where(neither, -1, team)[have]
    ids["flags"][have] = (weak | np.where(neither, ID_NEITHER, 0))[have]
    m = np.zeros(1, MODEL_DTYPE)
    m[0]["a"], m[0]["b"], m[0]["dab"], m[0]["voters"], m[0]["cost"], m[0]["neither"] = a, b, dab, len(vot), best[0], int(neither.sum())
    m[0]["w"], m[0]["flags"], m[0]["team_of_a"] = (wsum[swap], wsum[1 - swap]), MODEL_SWAPPED if swap else 0, swap
    return ids, m


# ---- the whole stage ----------------------------------------------------------------------------------------------------------------------------
def team_cluster(frames, crops, slots, n_ids, min_pixels=None, min_crops=None, outlier=None, loop=False):
    """frames uint8 [n, h, w, 3] BGR, crops [k, 5] (frame, x1, y1, x2, y2), slots [k] -> (CROP_DTYPE [k], ID_DTYPE [n_ids], MODEL_DTYPE [1])"""
    par = resolve(min_pixels, min_crops, outlier)
    frames = np.asarray(frames, np.uint8)
    recs, sums, used, skipped = _accumulate(frames, crops, slots, int(n_ids), par[0], crop_record_loop if loop else crop_record)
    ids, model = (cluster_ids_loop if loop else cluster_ids)(sums, used, skipped, *par)
    return recs, ids, model


def team_cluster_loop(frames, crops, slots, n_ids, min_pixels=None, min_crops=None, outlier=None):
    return team_cluster(frames, crops, slots, n_ids, min_pixels, min_crops, outlier, loop=True)


def mapping_of(ids, slot_ids):
    """{tracker id: 0 | 1} of the id records: ids without crops and ids that are neither have no entry"""
    return {int(pid): int(r["team"]) for pid, r in zip(slot_ids, ids) if r["team"] >= 0}
