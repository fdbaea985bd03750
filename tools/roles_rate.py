#!/usr/bin/env python3
"""Cost of the role kernels (include/eagle.h, eagle_post_roles; csrc/roles.hip): one JSON line.

    python tools/roles_rate.py [--rows 30000] [--reps 7] [--numpy-rows 300]

A processed table of --rows rows is built by eagle_postprocess from constructed records: two teams of ten outfield players round a 4-4-2 each, present
on every row; one player of each team changes his id half way, so the table has 22 member columns of which 10 per team are present.  With R = 10 every
(row, team) pair is ACTIVE with n = 10.  For R = 5 the mapping names five players per team (and the two replacements): 12 members, n = 5.  The prepare
launch and ONE assign round (iterations = 1) are timed over all rows: HIP events of the profiling mode around the launches, --reps calls after a warm-up
call, reported as the median with the minimum and the maximum.  Next to the assign kernel stand its subset updates per second (an update is one
candidate c[k][j] + h[mask | 1 << j] with j outside mask: sum over k < n of C(R, k) (R - k) per pair), the VALU bound of its inner loop estimated from the
instruction count in the gfx950 disassembly (see docs/experiments.md, "Roles (K29)"), and the time the numpy restatement (tests/roles_ref.py) takes
for one round on --numpy-rows of the same rows, scaled to the table."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eagle_amd import lib, weights  # noqa: E402
from control_rate import timed  # noqa: E402

# VALU bound of roles_assign_kernel's inner loop.  One pass of the loop handles one role j for the (up to 64) subsets the lanes hold, useful or not (j
# inside the subset is computed and not taken).  Counted in the gfx950 disassembly it issues 8 vector instructions (v_or, 2 v_lshl_add, v_and, v_cmp_eq,
# v_cmp_lt_u64, 2 v_cndmask; the 64-bit add is one of the v_lshl_add) beside 2 ds_read_b64: 16 cycles at 2 cycles per wave64 instruction.  A pair runs
# sum over k < n of ceil(C(R, k) / 64) R passes.  256 CUs x 4 SIMDs at 2.4 GHz: 2.458e12 SIMD-cycles/s
CYCLES_PER_PASS = 16
SIMD_CYCLES = 256 * 4 * 2.4e9
FORM = [(20, 8), (18, 26), (18, 42), (20, 60), (45, 10), (43, 27), (43, 41), (45, 58), (70, 24), (70, 44)]


def records(n, seed=0):
    """n records of 20 players (ids 1 .. 20, slot s of team g is detection 10 g + s) and the ball; slot 0 of each team is id 21 + g from row n / 2 on"""
    r = np.random.default_rng(seed)
    k = 21
    recs = np.zeros(n, lib.RESULT_DTYPE)
    recs["n_det"], recs["H_valid"], recs["bounds_valid"] = k, 1, 1
    recs["bounds"] = (20.0, 10.0, 85.0, 75.0)
    base = np.array([(x, y) for x, y in FORM] + [(105 - x, y) for x, y in FORM] + [(52, 34)], np.float64)
    pos = np.clip(base[None] + r.normal(0, 2.0, (n, k, 2)) + np.cumsum(r.normal(0, 0.2, (n, 1, 2)), 0), 0, [105, 68])
    d, j = recs["det"], np.arange(k)
    d["reported"][:, :k], d["in_bounds"][:, :k], d["conf"][:, :k] = 1, 1, 0.9
    d["cls"][:, :k] = np.where(j == k - 1, 2, 0)[None]
    d["id"][:, :k] = (j + 1)[None]
    d["id"][n // 2:, 0], d["id"][n // 2:, 10] = 21, 22
    d["bx1"][:, :k], d["bx2"][:, :k], d["by1"][:, :k], d["by2"][:, :k] = (4 * j)[None], (4 * j + 3)[None], 300, 340
    d["pitch_x"][:, :k], d["pitch_y"][:, :k] = pos[..., 0].astype(np.int32), pos[..., 1].astype(np.int32)
    return recs


def work(n_of_pairs, R):
    """the present counts of the ACTIVE pairs -> (subset updates, passes of the inner loop)"""
    upd = {n: sum(math.comb(R, k) * (R - k) for k in range(n)) for n in set(n_of_pairs)}
    pas = {n: sum(-(-math.comb(R, k) // 64) * R for k in range(n)) for n in set(n_of_pairs)}
    return float(sum(upd[n] for n in n_of_pairs)), float(sum(pas[n] for n in n_of_pairs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--numpy-rows", type=int, default=300)
    a = ap.parse_args()
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    res = {"reps": a.reps, "valu_cycles_per_pass": CYCLES_PER_PASS}
    recs = records(a.rows)
    import roles_ref as RR
    for R in (10, 5):
        team = lambda i: 0 if i <= 10 or i == 21 else 1
        ids = list(range(1, 23)) if R == 10 else [1, 2, 3, 4, 5, 11, 12, 13, 14, 15, 21, 22]
        t = h.postprocess(recs, 25, 1280, {i: team(i) for i in ids})
        try:
            rows = len(t.rows)
            p1 = lib.role_params(R, R, 1)
            call = lambda: h.roles(t, p1)
            out = {"roles_prepare": timed(h, "roles_prepare", a.reps, call), "roles_assign": timed(h, "roles_assign", a.reps, call)}
            rec, mr, model = h.roles(t, p1)
            act = rec["status"] == lib.ROLE_ACTIVE
            upd, passes = work([int(n) for n in rec["n"][act]], R)
            g = out["roles_assign"]
            sec = g["ms_median"] * 1e-3
            g.update(active_pairs=int(act.sum()), updates=float("%.4g" % upd), updates_per_s=float("%.4g" % (upd / sec)), passes=float("%.4g" % passes),
                     ms_at_valu_bound=round(passes * CYCLES_PER_PASS / SIMD_CYCLES * 1e3, 4), of_valu_bound=round(passes * CYCLES_PER_PASS / SIMD_CYCLES / sec, 4),
                     pairs_per_s=round(int(act.sum()) / sec))
            full = h.roles(t, lib.role_params(R, R, 8))[2]
            out.update(rows=rows, members=int(mr.shape[0]), changed_8_rounds=[int(v) for v in full["changed"][0][:8]])
            k = min(a.numpy_rows, rows)
            values = np.array(t.values)[:, :k]
            cols = [(int(c["kind"]), int(c["id"]), int(c["video"])) for c in t.columns]
            t0 = time.perf_counter()
            RR.roles(values, cols, t.team_mapping, RR.role_params(R, R, 1))
            dt = time.perf_counter() - t0
            out["numpy_one_round"] = {"rows": k, "seconds": round(dt, 3), "seconds_scaled_to_table": round(dt * rows / max(k, 1), 2)}
            res["R%d" % R] = out
        finally:
            t.close()
    h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
