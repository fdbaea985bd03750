"""numpy / Python-integer restatement of the role stage (include/eagle.h, eagle_post_roles / eagle_op_roles; csrc/roles.hip).  It is the single written
definition of every output bit: the kernels equal it bit for bit.  OWN SPEC: nothing of the reference computes this.

MEMBERS AND QUANTISATION are shape_ref's (members, quantise): groups 0 and 1, the Player pitch columns with a non-negative mapping entry (the first
entry counts), no goalkeepers, a mapping required, more than shape_ref.MAX_MEMBERS refused; a member is PRESENT on a row when both values are finite and
|x|, |y| <= 1024 m; q = floor(v * 1024 + 0.5).  Everything after that step is integer arithmetic, so no result depends on an order of accumulation.

PARAMETERS (role_params): roles R in 2 .. ROLE_CAP (10), min_present in 2 .. R (8), iterations T in 1 .. 32 (8).  The defaults are conventional
choices (ten outfield players; a view that shows eight of them; a handful of rounds), not fitted to data.

PER (ROW, GROUP).  n = the present members.  status = EMPTY when n == 0, else TOO_FEW when n < min_present, TOO_MANY when n > R, else ACTIVE.  Centre
cx = floor((2 sum qx + n) / (2 n)) (Python's floor division; 0 when n == 0), cy likewise.  A present member's centred position is u = q - c, |u| <= 2^21.
The PLAYERS of a row are its present members in table-column order, player 0 first.

SEEDS.  Per member column: cnt = the ACTIVE rows on which it is present, S = the integer sums of u over them.  The columns of a group are ranked by
(cnt descending, column ascending); the first R with cnt > 0 seed roles 0 .. R-1 at floor((2 S + cnt) / (2 cnt)) per axis.  A group with fewer such
columns has model status NO_SEEDS: its rows report role -1 and cost 0 (n, centre and status as above), the group has no means, counts or sums.

ONE ITERATION, for every ACTIVE row of a seeded group.  c[i][j] = |u_i - M_j|^2 (differences <= 2^22, a row's total < 2^49: exact in int64).  The
assignment sigma is the injective map players -> roles of least total cost and, among those, the lexicographically smallest sequence (sigma(0),
sigma(1), ...).  The subset recurrence says the same: h[mask] = the least cost of giving players popcount(mask) .. n-1 distinct roles outside mask; h = 0
where popcount == n, else h[mask] = min over j not in mask of c[k][j] + h[mask | 1 << j] with k = popcount(mask); walking k upwards from mask 0, player
k takes the smallest j not in mask with c[k][j] + h[mask | 1 << j] == h[mask].  Then M_j becomes floor((2 S_j + cnt_j) / (2 cnt_j)) over the (row,
player) pairs that sigma gave role j; a role with cnt_j == 0 keeps its position.  changed[k] = the (row, group) pairs whose sigma differs from iteration
k-1's, over both groups; in iteration 0 every ACTIVE row of a seeded group counts.

RESULT after T iterations: the assignment of iteration T-1, its row costs, and the means it was computed AGAINST (mean), so costs and means belong
together; count, sum and sum2 are cnt_j and the sums of u and u^2 per axis over that final assignment.  Once changed[k] == 0 (k >= 1) nothing moves any
more (M(k+1) is made of sigma(k) == sigma(k-1), as M(k) was): an implementation may stop there, reporting 0 from then on.  roles() below runs all T.

OUTPUTS.  ROW_DTYPE [rows][2]: cost, n, status, cx, cy, col[ROLE_CAP] = the table column playing role j, or -1.  int8 [members][rows], members in group
order (group 0's columns, then group 1's): the member's role on the row, -1 when absent, when the row is not ACTIVE and in a NO_SEEDS group.  MODEL_DTYPE:
per group sum, sum2 [ROLE_CAP][2], mean [ROLE_CAP][2], count [ROLE_CAP], status, active_rows (entries at and beyond R are 0); changed[32].

TWO DEFINITIONS: roles() is vectorised over rows, subset layer by subset layer, in int64; roles_scalar() goes row by row in Python integers and takes
the minimum over the permutations in lexicographic order, the first of least cost: it walks them depth first and leaves a prefix as soon as its cost plus
the cheapest role of every later player cannot get strictly below the best so far (costs are >= 0, and a later sequence of equal cost never wins).
tests/test_roles_cpu.py holds the two to each other, to itertools.permutations and to scipy's cost."""
import numpy as np

from shape_ref import members, quantise

ROLE_CAP = 10
EMPTY, TOO_FEW, ACTIVE, TOO_MANY = 0, 1, 2, 3
MODEL_OK, NO_SEEDS = 0, 1
ROW_DTYPE = np.dtype([("cost", "<i8"), ("n", "<i4"), ("status", "<i4"), ("cx", "<i4"), ("cy", "<i4"), ("col", "<i4", ROLE_CAP)])                     # EagleRoleRow, 64 bytes
GROUP_DTYPE = np.dtype([("sum", "<i8", (ROLE_CAP, 2)), ("sum2", "<i8", (ROLE_CAP, 2)), ("mean", "<i4", (ROLE_CAP, 2)), ("count", "<i4", ROLE_CAP),
                        ("status", "<i4"), ("active_rows", "<i4")])                                                                                   # EagleRoleGroup, 448 bytes
MODEL_DTYPE = np.dtype([("group", GROUP_DTYPE, 2), ("changed", "<i4", 32)])                                                                            # EagleRoleModel, 1024 bytes
assert (ROW_DTYPE.itemsize, GROUP_DTYPE.itemsize, MODEL_DTYPE.itemsize) == (64, 448, 1024)


def role_params(roles=10, min_present=8, iterations=8):
    return {"roles": int(roles), "min_present": int(min_present), "iterations": int(iterations)}


def check_params(p):
    if not 2 <= p["roles"] <= ROLE_CAP:
        raise ValueError("roles %r outside 2 .. %d" % (p["roles"], ROLE_CAP))
    if not 2 <= p["min_present"] <= p["roles"]:
        raise ValueError("min_present %r outside 2 .. roles" % (p["min_present"],))
    if not 1 <= p["iterations"] <= 32:
        raise ValueError("iterations %r outside 1 .. 32" % (p["iterations"],))


def status_of(n, R, mp):
    return EMPTY if n == 0 else TOO_FEW if n < mp else TOO_MANY if n > R else ACTIVE


def rounded_mean(S, cnt):
    """floor((2 S + cnt) / (2 cnt)): Python integers, or int64 arrays with cnt > 0 (numpy's // floors too)"""
    return (2 * S + cnt) // (2 * cnt)


def _outputs(rows, nmem):
    rec = np.zeros((rows, 2), ROW_DTYPE)
    rec["col"] = -1
    return rec, np.full((nmem, rows), -1, np.int8), np.zeros(1, MODEL_DTYPE)


# ---- definition one: vectorised over rows, int64 ------------------------------------------------------------------------------------
def assign_layers(ux, uy, M, R):
    """ux, uy int64 [rows][n] (the players of rows that all have n of them), M int64 [R][2] -> (sigma int64 [rows][n], cost int64 [rows])"""
    return assign_costs((ux[:, :, None] - M[None, None, :, 0]) ** 2 + (uy[:, :, None] - M[None, None, :, 1]) ** 2, R)


def assign_costs(c, R):
    """c int64 [rows][n][R] >= 0 -> (sigma, cost): the subset recurrence layer by layer, then the walk from mask 0"""
    nr, n = c.shape[:2]
    masks = np.arange(1 << R, dtype=np.int64)
    pc = sum((masks >> j) & 1 for j in range(R))
    h = np.zeros((nr, 1 << R), np.int64)                        # (popcount == n: 0; above n: never read)
    for k in range(n - 1, -1, -1):
        ms = masks[pc == k]
        best = np.full((nr, len(ms)), np.iinfo(np.int64).max, np.int64)
        for j in range(R):
            free = ((ms >> j) & 1) == 0
            best[:, free] = np.minimum(best[:, free], c[:, k, j][:, None] + h[:, ms[free] | (1 << j)])
        h[:, ms] = best
    ar, mask, sigma = np.arange(nr), np.zeros(nr, np.int64), np.full((nr, n), -1, np.int64)
    for k in range(n):
        for j in range(R):
            take = (sigma[:, k] < 0) & (((mask >> j) & 1) == 0) & (c[:, k, j] + h[ar, mask | (1 << j)] == h[ar, mask])
            sigma[take, k] = j
        assert (sigma[:, k] >= 0).all()
        mask |= 1 << sigma[:, k]
    return sigma, h[:, 0].copy()


def roles(values, columns, mapping, p):
    """values float64 [cols][rows][2] -> (ROW_DTYPE [rows, 2], int8 [members, rows], MODEL_DTYPE [1])"""
    check_params(p)
    R, mp, T = p["roles"], p["min_present"], p["iterations"]
    groups = members(columns, mapping)
    rows = values.shape[1]
    rec, mrole, model = _outputs(rows, len(groups[0]) + len(groups[1]))
    G = []
    for g in (0, 1):
        cols = np.array(groups[g], np.int64)
        if len(cols):
            qx, qy, ok = quantise(values[cols, :, 0], values[cols, :, 1])
        else:
            qx, qy, ok = np.zeros((0, rows), np.int64), np.zeros((0, rows), np.int64), np.zeros((0, rows), bool)
        n = ok.sum(0).astype(np.int64)
        nn = np.maximum(n, 1)
        cx, cy = np.where(n > 0, (2 * qx.sum(0) + n) // (2 * nn), 0), np.where(n > 0, (2 * qy.sum(0) + n) // (2 * nn), 0)
        status = np.where(n == 0, EMPTY, np.where(n < mp, TOO_FEW, np.where(n > R, TOO_MANY, ACTIVE)))
        active = status == ACTIVE
        ux, uy = np.where(ok, qx - cx, 0), np.where(ok, qy - cy, 0)
        o = rec[:, g]
        o["n"], o["status"], o["cx"], o["cy"] = n, status, cx, cy
        mg = model["group"][0, g]
        mg["active_rows"] = active.sum()
        w = ok & active
        cnt, Sx, Sy = w.sum(1).astype(np.int64), (ux * w).sum(1), (uy * w).sum(1)
        seeds = [m for m in sorted(range(len(cols)), key=lambda m: (-cnt[m], m)) if cnt[m] > 0][:R]
        M = None
        if len(seeds) == R:
            M = np.array([[rounded_mean(Sx[m], cnt[m]), rounded_mean(Sy[m], cnt[m])] for m in seeds], np.int64)
        else:
            mg["status"] = NO_SEEDS
        G.append({"cols": cols, "ok": ok, "ux": ux, "uy": uy, "n": n, "active": active, "M": M, "rm": None, "base": 0 if g == 0 else len(groups[0])})
    for k in range(T):
        for s in G:
            if s["M"] is None:
                continue
            rm, cost = np.full(s["ok"].shape, -1, np.int64), np.zeros(rows, np.int64)
            for n in np.unique(s["n"][s["active"]]):
                idx = np.nonzero(s["active"] & (s["n"] == n))[0]
                pl = np.argsort(~s["ok"][:, idx], axis=0, kind="stable")[:n].T         # [rows of idx][n]: the present members, in order
                sigma, cost[idx] = assign_layers(s["ux"][pl, idx[:, None]], s["uy"][pl, idx[:, None]], s["M"], R)
                rm[pl, idx[:, None]] = sigma
            moved = s["active"] if s["rm"] is None else (rm != s["rm"]).any(0)
            model["changed"][0, k] += int(moved.sum())
            s["rm"], s["cost"], s["used"] = rm, cost, s["M"]
            nxt = s["M"].copy()
            s["cnt"], s["S"], s["S2"] = np.zeros(R, np.int64), np.zeros((R, 2), np.int64), np.zeros((R, 2), np.int64)
            for j in range(R):
                sel = rm == j
                s["cnt"][j] = sel.sum()
                s["S"][j] = (s["ux"] * sel).sum(), (s["uy"] * sel).sum()
                s["S2"][j] = (s["ux"] ** 2 * sel).sum(), (s["uy"] ** 2 * sel).sum()
                if s["cnt"][j]:
                    nxt[j] = rounded_mean(s["S"][j], s["cnt"][j])
            s["M"] = nxt
    for g, s in enumerate(G):
        if s["M"] is None:
            continue
        mg = model["group"][0, g]
        mg["mean"][:R], mg["count"][:R], mg["sum"][:R], mg["sum2"][:R] = s["used"], s["cnt"], s["S"], s["S2"]
        rec[:, g]["cost"] = s["cost"]
        mrole[s["base"]:s["base"] + len(s["cols"])] = s["rm"]
        for m, c in enumerate(s["cols"]):
            for r in np.nonzero(s["rm"][m] >= 0)[0]:
                rec[r, g]["col"][s["rm"][m, r]] = c
    return rec, mrole, model


# ---- definition two: row by row, Python integers, the minimum over the permutations ------------------------------------------------------
def assign_permutations(c, R):
    """c [n][R] of Python integers >= 0 -> (sigma tuple, cost): the first permutation of least cost in lexicographic order"""
    n = len(c)
    floor_ = [0] * (n + 1)
    for k in range(n - 1, -1, -1):
        floor_[k] = floor_[k + 1] + min(c[k])
    best = [None, None]

    def walk(k, used, cost, seq):
        if best[0] is not None and cost + floor_[k] >= best[0]:
            return
        if k == n:
            best[0], best[1] = cost, tuple(seq)
            return
        for j in range(R):
            if not (used >> j) & 1:
                walk(k + 1, used | (1 << j), cost + c[k][j], seq + [j])

    walk(0, 0, 0, [])
    return best[1], best[0]


def roles_scalar(values, columns, mapping, p, assign=assign_permutations):
    check_params(p)
    R, mp, T = p["roles"], p["min_present"], p["iterations"]
    groups = members(columns, mapping)
    rows = values.shape[1]
    rec, mrole, model = _outputs(rows, len(groups[0]) + len(groups[1]))
    G = []
    for g in (0, 1):
        cols, base = groups[g], 0 if g == 0 else len(groups[0])
        players = []                                            # per row: [(member, ux, uy)] or None when the row is not ACTIVE
        cnt, S = [0] * len(cols), [[0, 0] for _ in cols]
        for r in range(rows):
            if cols:
                qx, qy, ok = quantise(values[cols, r, 0], values[cols, r, 1])
            pts = [(m, int(qx[m]), int(qy[m])) for m in range(len(cols)) if ok[m]]
            n = len(pts)
            cx = (2 * sum(q[1] for q in pts) + n) // (2 * n) if n else 0
            cy = (2 * sum(q[2] for q in pts) + n) // (2 * n) if n else 0
            o = rec[r, g]
            o["n"], o["status"], o["cx"], o["cy"] = n, status_of(n, R, mp), cx, cy
            if o["status"] != ACTIVE:
                players.append(None)
                continue
            players.append([(m, x - cx, y - cy) for m, x, y in pts])
            for m, x, y in players[-1]:
                cnt[m] += 1; S[m][0] += x; S[m][1] += y
        mg = model["group"][0, g]
        mg["active_rows"] = sum(pl is not None for pl in players)
        seeds = [m for m in sorted(range(len(cols)), key=lambda m: (-cnt[m], m)) if cnt[m] > 0][:R]
        M = [(rounded_mean(S[m][0], cnt[m]), rounded_mean(S[m][1], cnt[m])) for m in seeds] if len(seeds) == R else None
        if M is None:
            mg["status"] = NO_SEEDS
        G.append({"cols": cols, "base": base, "players": players, "M": M, "sigma": None})
    for k in range(T):
        for s in G:
            if s["M"] is None:
                continue
            sig, cost = [None] * rows, [0] * rows
            cnt, S, S2 = [0] * R, [[0, 0] for _ in range(R)], [[0, 0] for _ in range(R)]
            for r, pl in enumerate(s["players"]):
                if pl is None:
                    continue
                c = [[(x - mx) ** 2 + (y - my) ** 2 for mx, my in s["M"]] for _, x, y in pl]
                sig[r], cost[r] = assign(c, R)
                for (_, x, y), j in zip(pl, sig[r]):
                    cnt[j] += 1; S[j][0] += x; S[j][1] += y; S2[j][0] += x * x; S2[j][1] += y * y
                if s["sigma"] is None or sig[r] != s["sigma"][r]:
                    model["changed"][0, k] += 1
            s["sigma"], s["cost"], s["used"], s["cnt"], s["S"], s["S2"] = sig, cost, s["M"], cnt, S, S2
            s["M"] = [(rounded_mean(S[j][0], cnt[j]), rounded_mean(S[j][1], cnt[j])) if cnt[j] else s["M"][j] for j in range(R)]
    for g, s in enumerate(G):
        if s["M"] is None:
            continue
        mg = model["group"][0, g]
        mg["mean"][:R], mg["count"][:R], mg["sum"][:R], mg["sum2"][:R] = s["used"], s["cnt"], s["S"], s["S2"]
        for r, pl in enumerate(s["players"]):
            if pl is None:
                continue
            rec[r, g]["cost"] = s["cost"][r]
            for (m, _, _), j in zip(pl, s["sigma"][r]):
                rec[r, g]["col"][j] = s["cols"][m]
                mrole[s["base"] + m, r] = j
    return rec, mrole, model
