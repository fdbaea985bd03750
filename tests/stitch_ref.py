"""The numpy contract of the post-processor's opt-in id merge (include/eagle.h, EaglePostParams.merge_ids = 1; csrc/post.hip), built on
tests/post_ref.py.  With the switch off ``process_data`` returns post_ref.process_data's table and nothing else.  The rule is this project's own:
the reference's ``Processor.merge_data`` (eagle/processor.py:218-319) states three conditions with two constants, which are kept, but its overlap
test never lets a pair through, and as intended it would union every admissible pair, overlapping ones included.

Where it sits: after create_dataframe's 1 % filter, the ball fill and the goalkeeper fold, before the per-column interpolation and smoothing.

Tracks: the person video columns of that table.  first(T) / last(T): the first / last ROW whose video cell is present; F[]: the kept FRAME numbers;
p_first / p_last: the video cells of those rows.

A link a -> b is admissible when
  * a and b are of one kind (Player with Player, Goalkeeper with Goalkeeper);
  * last(a) < first(b);
  * g = F[first(b)] - F[last(a)] <= int(fps * 1.1);
  * d = sqrt(dx * dx + dy * dy) <= 10.0 * g, in float64, every operation single, between p_last(a) and p_first(b);
  * not both ids have an entry in the team mapping with different teams (entries below 0 count as none).

Selection: the admissible links ascending by (d, g, table position of a, table position of b); a link is accepted when a has no successor yet, b no
predecessor yet, and the teams known for the two chains do not differ (a chain's team: the entry of any member, members agree by construction).

Result: a chain keeps the id, the kind and the column positions of its head, the member without predecessor (its pitch column sits right in front
of its video column; it exists when any member has a pitch column).  A cell holds the value of the member present in that row.  The other members'
columns leave the table.  Interpolation and smoothing run on the merged columns as on any other.  A head without a team entry whose chain's team
is known gains that entry (heads in table order).  ``merges``: one dict per accepted link in acceptance order, {kind (0 Player, 1 Goalkeeper),
from_id, to_id, head_id and team (-1: unknown) of the finished chain, gap_frames = g, dist = d}."""
import numpy as np

import post_ref

TEMPORAL_SECONDS, PIXELS_PER_FRAME = 1.1, 10.0            # proc.py:219, 272
MAX_CHAIN = 100                                            # every track holds >= 1 % of the rows and a chain's spans are disjoint


def _team(tm, pid):
    v = tm.get(pid, -1)
    return v if v >= 0 else -1


def tracks_of(table, team_mapping):
    """The person video columns of a (folded) table in table order -> [{name, kind, id, pos, first, last, p_first, p_last, team}]."""
    out = []
    for pos, n in enumerate(table):
        if not n.endswith("_video") or n.split("_")[0] not in ("Player", "Goalkeeper"):
            continue
        ok = np.flatnonzero(post_ref._present(table[n]))
        pid = int(n.split("_")[1])
        out.append({"name": n, "kind": 0 if n.startswith("Player") else 1, "id": pid, "pos": pos, "first": int(ok[0]), "last": int(ok[-1]),
                    "p_first": table[n][ok[0]].astype(np.float64), "p_last": table[n][ok[-1]].astype(np.float64), "team": _team(team_mapping, pid)})
    return out


def admissible_links(tracks, rows, fps):
    """-> [(d, g, a, b)]: indices into tracks, in no order that means anything (successor-major: the sort key alone decides)."""
    limit = int(fps * TEMPORAL_SECONDS)
    links = []
    for b, B in enumerate(tracks):
        for a, A in enumerate(tracks):
            if a == b or A["kind"] != B["kind"] or not A["last"] < B["first"]:
                continue
            g = rows[B["first"]] - rows[A["last"]]
            if g > limit:
                continue
            dx, dy = np.float64(B["p_first"][0]) - np.float64(A["p_last"][0]), np.float64(B["p_first"][1]) - np.float64(A["p_last"][1])
            d = np.sqrt(dx * dx + dy * dy)
            if d > PIXELS_PER_FRAME * g:
                continue
            if A["team"] >= 0 and B["team"] >= 0 and A["team"] != B["team"]:
                continue
            links.append((float(d), int(g), a, b))
    return links


def link_key(tracks):
    """The order the admissible links are walked in: ascending (d, g, table position of a, table position of b).  A total order: no two links tie."""
    return lambda l: (l[0], l[1], tracks[l[2]]["pos"], tracks[l[3]]["pos"])


def select_links(tracks, rows, fps, key=None):
    """-> (accepted [(d, g, a, b)] in acceptance order, succ, pred, head index per track, team per head index).  key: another order than link_key's,
    for tests that show the order matters."""
    links = sorted(admissible_links(tracks, rows, fps), key=key or link_key(tracks))
    n = len(tracks)
    succ, pred, head = [-1] * n, [-1] * n, list(range(n))
    team = [t["team"] for t in tracks]                     # valid at the heads
    accepted = []
    for d, g, a, b in links:
        if succ[a] >= 0 or pred[b] >= 0:
            continue
        ha = head[a]
        if team[ha] >= 0 and team[b] >= 0 and team[ha] != team[b]:
            continue
        succ[a], pred[b] = b, a
        if team[ha] < 0:
            team[ha] = team[b]
        m = b
        while m >= 0:                                      # b heads its chain: all of it now hangs behind a
            head[m] = ha
            m = succ[m]
        accepted.append((d, g, a, b))
    return accepted, succ, pred, head, team


def stitch(rows, table, fps, team_mapping):
    """merge_data's second half as specified above: (folded table) -> (merged table, merges, team mapping with the inherited entries)."""
    tracks = tracks_of(table, team_mapping)
    accepted, succ, pred, head, team = select_links(tracks, rows, fps)
    merges = [{"kind": tracks[a]["kind"], "from_id": tracks[a]["id"], "to_id": tracks[b]["id"], "head_id": tracks[head[a]]["id"], "gap_frames": g,
               "team": team[head[a]], "dist": d} for d, g, a, b in accepted]
    tm = dict(team_mapping)
    merged, gone = {}, set()
    for i, T in enumerate(tracks):
        if pred[i] >= 0:
            continue
        chain, m = [], i
        while m >= 0:
            chain.append(tracks[m])
            m = succ[m]
        assert len(chain) <= MAX_CHAIN
        vid = table[T["name"]].copy()
        pitch = [table[M["name"][:-6]] for M in chain if M["name"][:-6] in table]
        pit = np.full_like(vid, np.nan) if pitch else None
        for M in chain[1:]:
            vid = np.where(post_ref._present(table[M["name"]])[:, None], table[M["name"]], vid)
            gone |= {M["name"], M["name"][:-6]}
        for col in pitch:
            pit = np.where(post_ref._present(col)[:, None], col, pit)
        merged[T["name"]] = (pit, vid)
        if len(chain) > 1 and team[i] >= 0 and _team(tm, T["id"]) < 0:
            tm[T["id"]] = team[i]
    out = {}
    for n in table:
        if n in gone:
            continue
        if n in merged:
            pit, vid = merged[n]
            if pit is not None:
                out[n[:-6]] = pit
            out[n] = vid
        elif n + "_video" not in merged:                   # (a head's own pitch column is written with its video column)
            out[n] = table[n]
    return out, merges, tm


def accepted_ids(case_coords, team_mapping, fps, key=None):
    """The (from_id, to_id) pairs accepted on a clip, under link_key or another order `key(tracks)`."""
    rows, table, _ = post_ref.create_dataframe(case_coords)
    tracks = tracks_of(post_ref.merge_data(table), team_mapping)
    return [(tracks[a]["id"], tracks[b]["id"]) for _, _, a, b in select_links(tracks, rows, fps, key(tracks) if key else None)[0]]


def process_data(coords, team_mapping=None, smooth=False, fps=25, merge_ids=False):
    """post_ref.process_data with the id merge between the fold and the interpolation.  merge_ids False: post_ref's table plus "merges": []."""
    if not merge_ids:
        return dict(post_ref.process_data(coords, team_mapping, smooth=smooth), merges=[])
    rows, table, flags = post_ref.create_dataframe(coords)
    merges, tm = [], dict(team_mapping or {})
    if not rows:
        table, tm = {}, {}
    else:
        for n in ("Ball", "Ball_video"):
            table[n] = post_ref.interpolate_col(table[n], fill=True)
        table = post_ref.merge_data(table)
        table, merges, tm = stitch(rows, table, fps, tm)
        for n in table:
            table[n] = post_ref.interpolate_col(table[n], False)
            if smooth:
                table[n] = post_ref.smooth_col(table[n])
    names = list(table)
    values = np.stack([table[n] for n in names]) if names else np.zeros((0, len(rows), 2))
    return {"rows": rows, "columns": names, "values": values.reshape(len(names), len(rows), 2), "flags": flags, "team_mapping": tm, "merges": merges}
