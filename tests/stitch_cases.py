"""Constructed clips for the post-processor's id merge (contract: tests/stitch_ref.py), in tests/post_cases.py's frame format.  Every case carries
"links": the (from_id, to_id) pairs the rule must accept, in acceptance order, worked out by hand from the construction, and "heads": the ids
of the person video columns the merged table must hold, in table order.

Person 1 (the anchor, far from everything, on every frame that is kept) keeps rows in the table while the others are away; it spans the whole clip
and so can never be linked."""
import numpy as np

import post_cases
from post_cases import G, P, _case, frame, person

FAR = (9000, 5000)


def clip(T, spans, anchor=True, empty=(), no_h=()):
    """spans: (cls, id, t0, t1, x0, y0[, vx, vy[, opts]]): present on frames t0 .. t1 with its foot at (x0 + vx (t - t0), y0 + vy (t - t0)); x0 may be
    a half-integer.  opts: {"no_pitch": frames without a pitch point (True: all)}.  empty: frames without any person; no_h: frames without homography."""
    frames = []
    for t in range(T):
        ps = []
        if t not in empty:
            if anchor:
                ps.append(person(P, 1, FAR[0], FAR[1]))
            for s in spans:
                cls, pid, t0, t1, x0, y0 = s[:6]
                vx, vy = (s[6], s[7]) if len(s) > 7 else (0, 0)
                opts = s[8] if len(s) > 8 else {}
                if not t0 <= t <= t1:
                    continue
                fx, fy = x0 + vx * (t - t0), y0 + vy * (t - t0)
                wide = 21 if fx != int(fx) else 20           # foot x = left + wide / 2
                left = int(fx - wide / 2)
                assert left + wide / 2 == fx and fy == int(fy) and left >= 0
                npit = opts.get("no_pitch", ())
                ps.append(person(cls, pid, left, fy, pitch=None if npit is True or t in npit else (), wide=wide))
        frames.append(frame(ps, [], bounds=(10.5, 12.25, 90.0, 95.75) if t < 2 else None, H=t not in no_h))
    return frames


def _add(out, name, frames, links, heads, fps=25, team_mapping=None, teams=None):
    c = _case(name, frames, fps=fps, team_mapping=team_mapping)
    c["links"], c["heads"], c["teams"] = list(links), list(heads), dict(team_mapping or {}) if teams is None else teams
    out.append(c)


def _cases():
    out = []
    # 1. hand-over: id 5 on rows 0-9, id 9 on rows 12-20 nearby
    _add(out, "hand_over", clip(21, [(P, 5, 0, 9, 100, 400, 2, 0), (P, 9, 12, 20, 126, 402, 2, 0)]), [(5, 9)], [1, 5])
    # 2. the temporal threshold int(fps * 1.1): 27 at 25 frames/s, 26 at 24, 33 at 30
    for fps, lim in ((25, 27), (24, 26), (30, 33)):
        assert int(fps * 1.1) == lim
        for g, links, heads in ((lim, [(5, 9)], [1, 5]), (lim + 1, [], [1, 5, 9])):
            _add(out, f"temporal_fps{fps}_gap{g}", clip(g + 5, [(P, 5, 0, 2, 300, 400), (P, 9, 2 + g, g + 4, 300, 400)]), links, heads, fps=fps)
    # 3. frames without any person leave the table: one row apart, but 7 frames (fps 5: at most 5) -> no link; 5 frames and 40 px -> a link (10 px per FRAME)
    _add(out, "frame_gap_over", clip(12, [(P, 5, 0, 2, 300, 400), (P, 9, 9, 11, 300, 400)], empty=range(3, 9)), [], [1, 5, 9], fps=5)
    _add(out, "frame_gap_within", clip(10, [(P, 5, 0, 2, 300, 400), (P, 9, 7, 9, 340, 400)], empty=range(3, 7)), [(5, 9)], [1, 5], fps=5)
    # 4. the distance threshold d <= 10 g on exact triples
    _add(out, "distance_g3_at", clip(9, [(P, 5, 0, 2, 300, 400), (P, 9, 5, 8, 318, 424)]), [(5, 9)], [1, 5])
    _add(out, "distance_g3_over", clip(9, [(P, 5, 0, 2, 300, 400), (P, 9, 5, 8, 318, 425)]), [], [1, 5, 9])
    _add(out, "distance_g1_at", clip(6, [(P, 5, 0, 2, 300, 400), (P, 9, 3, 5, 306, 408)]), [(5, 9)], [1, 5])
    _add(out, "distance_g1_over", clip(6, [(P, 5, 0, 2, 300, 400), (P, 9, 3, 5, 306.5, 408)]), [], [1, 5, 9])
    _add(out, "distance_g2_half", clip(7, [(P, 5, 0, 2, 300.5, 400), (P, 9, 4, 6, 312.5, 416)]), [(5, 9)], [1, 5])       # 12, 16 -> 20 = 10 g
    # 5. both present in one single frame: no link
    _add(out, "overlap_one_frame", clip(11, [(P, 5, 0, 5, 300, 400), (P, 9, 5, 10, 300, 400)]), [], [1, 5, 9])
    # 6. teams
    two = [(P, 5, 0, 3, 300, 400), (P, 9, 5, 8, 304, 400)]
    _add(out, "teams_differ", clip(9, two), [], [1, 5, 9], team_mapping={5: 0, 9: 1})
    _add(out, "teams_same", clip(9, two), [(5, 9)], [1, 5], team_mapping={5: 1, 9: 1})
    _add(out, "teams_tail_unknown", clip(9, two), [(5, 9)], [1, 5], team_mapping={5: 0})
    _add(out, "teams_head_inherits", clip(9, two), [(5, 9)], [1, 5], team_mapping={9: 1}, teams={9: 1, 5: 1})
    _add(out, "teams_both_unknown", clip(9, two), [(5, 9)], [1, 5], team_mapping={1: 0})
    _add(out, "teams_no_mapping", clip(9, two), [(5, 9)], [1, 5], team_mapping={})
    three = lambda d1, d2: [(P, 5, 0, 3, 300, 400), (P, 7, 5, 8, 300 + d1, 400), (P, 9, 10, 13, 300 + d1 + d2, 400)]      # noqa: E731
    _add(out, "teams_chain_first_link_wins", clip(14, three(3, 6)), [(5, 7)], [1, 5, 9], team_mapping={5: 0, 9: 1})      # 5 -> 7 (d 3) makes the chain team 0: 7 -> 9 refused
    _add(out, "teams_chain_second_link_wins", clip(14, three(6, 3)), [(7, 9)], [1, 5, 7], team_mapping={5: 0, 9: 1}, teams={5: 0, 9: 1, 7: 1})
    # 7. competition: a track takes one successor and one predecessor, the nearest; the loser stays free
    _add(out, "two_successors", clip(12, [(P, 5, 0, 3, 300, 400), (P, 6, 0, 2, 300, 425), (P, 8, 5, 11, 300, 405), (P, 9, 5, 11, 300, 403)]),
         [(5, 9), (6, 8)], [1, 5, 6])               # 5 -> 9 (d 3) beats 5 -> 8 (d 5); 8 then goes to 6 (d 20, g 3), which 9 (d 22) can no longer have
    _add(out, "two_predecessors", clip(12, [(P, 5, 0, 4, 300, 400), (P, 6, 0, 4, 300, 407), (P, 8, 6, 11, 300, 403), (P, 9, 7, 11, 300, 420)]),
         [(5, 8), (6, 9)], [1, 5, 6])               # 5 -> 8 (d 3) beats 6 -> 8 (d 4); 6 then takes 9 (d 13, g 3)
    _add(out, "tie_on_distance_by_gap", clip(12, [(P, 5, 0, 2, 300, 400), (P, 6, 0, 3, 305, 405), (P, 9, 5, 11, 300, 405)]), [(6, 9)], [1, 5, 6])
    #   (two predecessors 5 px from 9: 5, in the earlier column, left 3 frames before, 6 only 2: the gap decides, against the column order)
    _add(out, "distance_before_gap", clip(12, [(P, 6, 0, 3, 300, 410), (P, 5, 0, 2, 300, 400), (P, 9, 5, 11, 300, 402)]), [(5, 9)], [1, 6, 5])
    #   (5 -> 9: d 2 over 3 frames; 6 -> 9: d 8 over 2 frames, and 6 holds the earlier column: the distance comes first)
    _add(out, "tie_on_both_by_column", clip(12, [(P, 5, 0, 3, 300, 400), (P, 9, 5, 11, 300, 405), (P, 8, 5, 11, 305, 400)]), [(5, 9)], [1, 5, 8])
    _add(out, "tie_on_both_crossed", clip(12, [(P, 5, 0, 3, 300, 400), (P, 6, 0, 3, 300, 440), (P, 8, 5, 11, 300, 435), (P, 9, 5, 11, 300, 405)]),
         [(5, 9), (6, 8)], [1, 5, 6])               # 5 -> 9 and 6 -> 8, both d 5 and g 2 (the straight pairs are 35 px apart): the column of a orders them, not that of b
    _add(out, "teams_negative_entry", clip(9, two), [(5, 9)], [1, 5], team_mapping={5: -1, 9: 1}, teams={5: 1, 9: 1})      # an entry below 0 is no team: replaced
    # 8. chain lengths: one person whose id changes every k frames
    for n, k in ((3, 3), (5, 2), (64, 1), (65, 1), (100, 1)):
        ids = [200 + (37 * i) % 101 for i in range(n)]              # (not in ascending order)
        fr = clip(n * k, [(P, ids[i], i * k, i * k + k - 1, 300 + 3 * i * k, 400 + i * k, 3, 1) for i in range(n)], anchor=False)
        _add(out, f"chain_{n}", fr, [(ids[i], ids[i + 1]) for i in range(n - 1)], [ids[0]])
    # 9. kinds: a Player never links to a Goalkeeper; a goalkeeper chain through a folded Player_7 / Goalkeeper_7 pair
    _add(out, "kinds_do_not_mix", clip(9, [(P, 5, 0, 3, 300, 400), (G, 9, 5, 8, 304, 400)]), [], [1, 5, 9])
    _add(out, "goalkeeper_chain_with_fold", clip(14, [(G, 6, 0, 2, 300, 400, 2, 0), (P, 7, 4, 6, 308, 400, 2, 0), (G, 7, 6, 9, 342, 400, 2, 0),
                                                     (G, 8, 11, 13, 351.5, 400, 2, 0)]), [(7, 8), (6, 7)], [1, 6])           # d 3.5 and 4
    # 10. a bridging fragment below the 1 % filter is no candidate: 5 -> 7 -> 9 would chain, 5 -> 9 is 31 frames
    _add(out, "filtered_bridge", clip(101, [(P, 5, 0, 9, 300, 400), (P, 7, 20, 20, 300, 400), (P, 9, 40, 60, 300, 400)]), [], [1, 5, 9])
    _add(out, "kept_bridge", clip(101, [(P, 5, 0, 9, 300, 400), (P, 7, 20, 21, 300, 400), (P, 9, 40, 60, 300, 400)]), [(5, 7), (7, 9)], [1, 5])
    # 11. missing pitch cells at the fragments' ends: the video point decides; the pitch column interpolates over the chain's present cells
    _add(out, "pitch_missing_at_ends", clip(16, [(P, 5, 0, 6, 300, 400, 2, 1, {"no_pitch": (5, 6)}), (P, 9, 8, 15, 316, 408, 2, 1, {"no_pitch": (8, 9)})]),
         [(5, 9)], [1, 5])
    _add(out, "no_homography_at_ends", clip(16, [(P, 5, 0, 6, 300, 400, 2, 1), (P, 9, 8, 15, 316, 408, 2, 1)], no_h=(5, 6, 7, 8, 9)), [(5, 9)], [1, 5])
    _add(out, "pitch_column_from_member", clip(16, [(P, 5, 0, 6, 300, 400, 2, 1, {"no_pitch": True}), (P, 9, 8, 15, 316, 408, 2, 1)]), [(5, 9)], [1, 5])
    # 12. members' spans that meet at the seams of the series kernel's 256-row blocks and 64-row waves
    walk = lambda T, cuts: clip(T, [(P, 300 + i, a, b - 1, 100 + 2 * a, 400 + a, 2, 1) for i, (a, b) in enumerate(zip([0] + cuts, cuts + [T]))], anchor=False)      # noqa: E731
    _add(out, "seam_64_256", walk(300, [64, 256]), [(300, 301), (301, 302)], [300])
    _add(out, "seam_257", walk(300, [257]), [(300, 301)], [300])
    gapped = clip(300, [(P, 300, 0, 62, 100, 400, 2, 1), (P, 301, 65, 254, 230, 465, 2, 1), (P, 302, 258, 299, 616, 658, 2, 1)])
    _add(out, "seam_gaps_across", gapped, [(300, 301), (301, 302)], [1, 300])
    # (a 1 % fragment of a clip this long holds 11 rows, so a seam at rows 1024 / 1025 needs 1036 rows)
    _add(out, "seam_1025", walk(1036, [1025]), [(300, 301)], [300])
    _add(out, "seam_1024", walk(1036, [512, 1024]), [(300, 301), (301, 302)], [300])
    return out


def fragmented(seed, rows, players, fragments, fps=25):
    """`players` well-separated trajectories in steady motion (2, 1) px per frame over `rows` frames, each cut at random rows into `fragments` pieces
    with fresh ids and up to 3 frames lost at each cut -> (case, restored case: the same clip under each trajectory's first id, {fragment id: first id}).
    Distance grows with the gap, so the nearest admissible successor of a fragment is the next one of its own trajectory; trajectories lie 3000 px
    apart, beyond 10 * int(fps * 1.1)."""
    rng = np.random.default_rng(seed)
    need = int(np.ceil(0.01 * rows)) + 1                    # rows a fragment needs to pass the 1 % filter, and one more
    ids = list(rng.permutation(np.arange(100, 100 + players * fragments)))
    spans, restored, head_of, teams = [], [], {}, {}
    for k in range(players):
        slack = rows - fragments * (need + 3)
        assert slack >= 0
        extra = np.sort(rng.integers(0, slack + 1, fragments - 1)) if fragments > 1 else np.zeros(0, int)
        cuts = [int((i + 1) * (need + 3) + e) for i, e in enumerate(extra)]
        x0, y0 = 200 + 3000 * k, 300 + 3000 * (k % 2)
        for i, (a, b) in enumerate(zip([0] + cuts, cuts + [rows])):
            a += int(rng.integers(0, 4)) if i else 0        # frames lost at the cut
            pid = int(ids[k * fragments + i])
            head_of[pid] = int(ids[k * fragments])
            spans.append((P, pid, a, b - 1, x0 + 2 * a, y0 + a, 2, 1))
            restored.append((P, head_of[pid], a, b - 1, x0 + 2 * a, y0 + a, 2, 1))
            if rng.random() < 0.5:
                teams[pid] = k % 2
    case = _case(f"fragmented_{seed}_{rows}x{players}x{fragments}", clip(rows, spans), fps=fps, team_mapping=teams)
    return case, _case(case["name"] + "_restored", clip(rows, restored), fps=fps, team_mapping=teams), head_of


FRAGMENTED = [(1, 60, 2, 6), (2, 257, 3, 12), (3, 1025, 6, 40)]       # (seed, rows, players, fragments per player)
CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
records_of, coords_of = post_cases.records_of, post_cases.coords_of
