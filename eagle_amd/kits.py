"""Team assignment by clustering kit colours over the clip (include/eagle.h, eagle_team_cluster; csrc/kits.hip; tests/kits_ref.py is the written
definition of every bit).

The default team mapping is the reference's (eagle_amd/teams.py): per crop a 2-means segmentation, every pixel of the player cluster counted into eleven
named HSV ranges, a vote of colour names per id, and the two most common names are the two teams.  That rule cannot separate two kits inside one named
range (navy and sky blue are both ``blue``), a striped kit votes for two names at once, and a misdetected referee is forced into a team.  This stage is
the project's own, opt-in answer: the shirt window of every eligible player crop (rows h/5 .. h/2, columns w/4 .. w - w/4 of the box) is described by an
integer histogram of 34 colour bins (two brightness bands of 15 soft hue bins, four grey levels; grass keyed away), the normalised histograms are
summed per tracker id, and the ids are split by an exact weighted 2-medoid clustering: every pair of ids with at least ``min_crops`` used crops is tried
as the two centres.  An id farther from its medoid than ``outlier`` / 1024 of the distance between the medoids is in neither team and gets no entry in
the mapping.  Integers throughout: no seeding, no iteration, no order of accumulation.

Which crops are eligible is the reference's bookkeeping (teams.py): Player boxes with integer coordinates, non-empty, skipped when another player box of
the frame covers more than 35 % of them; no overlap weights.  The constants (32 pixels, 3 crops, half the distance, the bin edges) are conventional
choices, not fitted to data.  Limits: the shirt window is a fixed fraction of the box; the grey bins are hard-edged, so white and grey kits under
changing light are the weak case; a kit the colour of the grass keys away; goalkeepers stay in neither team, as before; only two teams are found; at
most 1024 ids per clip; a team follows a tracker id, not a person; nothing is validated on real footage."""
import numpy as np

from . import lib
from .teams import eligible_crops


def crop_list(coords, n_frames=None):
    """coords as ``get_coordinates`` returns it -> (crops int32 [k, 5] (frame, x1, y1, x2, y2), slots int32 [k], ids [n_ids]): the eligible Player
    crops of teams.eligible_crops (the reference's walk), each with the slot of its id; slots count the ids in order of first appearance."""
    crops, slots, slot_of = [], [], {}
    for i, pid, bbox, _ in eligible_crops(coords, n_frames):
        slots.append(slot_of.setdefault(pid, len(slot_of)))
        crops.append((i, *bbox))
    return np.array(crops, np.int32).reshape(-1, 5), np.array(slots, np.int32), list(slot_of)


def mapping_of(ids, slot_ids):
    """{tracker id: 0 | 1} of the id records: an id without a used crop and an id that is neither have no entry"""
    return {int(pid): int(r["team"]) for pid, r in zip(slot_ids, ids) if r["team"] >= 0}


def cluster_team_mapping(handle, dptr, coords, n_frames=None, min_pixels=None, min_crops=None, outlier=None):
    """The clip of ``n_frames`` frames resident at ``dptr`` and its ``get_coordinates`` output -> (mapping {id: 0 | 1}, report).  ``outlier`` is a ratio
    of the distance between the medoids (default 0.5, 0: off).  report: dict(params, crops, ids, model, slot_ids), the records of include/eagle.h."""
    n_frames = len(coords) if n_frames is None else min(int(n_frames), len(coords))
    crops, slots, slot_ids = crop_list(coords, n_frames)
    par = lib.kit_params(min_pixels, min_crops, None if outlier is None else int(round(float(outlier) * 1024.0)))
    recs, ids, model = handle.team_cluster(dptr, n_frames, crops, slots, len(slot_ids), par)
    report = {"params": {"min_pixels": par.min_pixels, "min_crops": par.min_crops, "outlier": par.outlier}, "crops": recs, "ids": ids, "model": model, "slot_ids": slot_ids}
    return mapping_of(ids, slot_ids), report


HUE_NAMES = ["vermilion", "orange", "yellow", "lime", "green", "emerald", "spring green", "cyan", "azure", "blue", "indigo", "violet", "magenta", "pink", "red"]   # 12 + 24 k degrees
GREY_NAMES = ["black", "dark grey", "light grey", "white"]


def bin_name(b):
    """a readable name for colour bin b: the hue of its centre (bin k is centred on cv2 hue 6 + 12 k), "dark" in the lower band"""
    if b >= 30:
        return GREY_NAMES[b - 30]
    return ("dark " if b < 15 else "") + HUE_NAMES[b % 15]


def bin_bgr(b):
    """a representative BGR colour of bin b: its centre hue at full saturation and value 96 (lower band) or 224 (upper band); the greys at 32, 96, 160, 224"""
    if b >= 30:
        v = 32 + 64 * (b - 30)
        return [v, v, v]
    v, deg = (96 if b < 15 else 224), 2.0 * (6 + 12 * (b % 15))
    x = deg / 60.0
    k, f = int(x) % 6, x - int(x)
    lo, up, dn = 0, int(round(v * f)), int(round(v * (1.0 - f)))
    r, g, bl = [(v, up, lo), (dn, v, lo), (lo, v, up), (lo, dn, v), (up, lo, v), (v, lo, dn)][k]
    return [bl, g, r]


def to_json(report):
    """what teams.json holds: the parameters, the model, per team its size and the three heaviest bins of its medoid, per id its crops, team, distances
    and flags"""
    ids, m, slot_ids, par = report["ids"], report["model"][0], report["slot_ids"], report["params"]
    single = bool(m["flags"] & lib.KIT_MODEL_SINGLE)
    medoid = [None, None] if single else ([int(m["b"]), int(m["a"])] if m["team_of_a"] else [int(m["a"]), int(m["b"])])
    teams = []
    for k in (0, 1):
        t = {"team": k, "ids": int(sum(1 for r in ids if r["team"] == k)), "weight": int(m["w"][k]), "medoid": None if medoid[k] is None else int(slot_ids[medoid[k]])}
        if medoid[k] is not None:
            p = ids[medoid[k]]["p"]
            top = sorted(range(lib.KIT_BINS), key=lambda b: (-int(p[b]), b))[:3]
            t["colours"] = [{"bin": b, "name": bin_name(b), "bgr": bin_bgr(b), "share": int(p[b]) / 65536.0} for b in top]
        teams.append(t)
    return {"parameters": {"min_pixels": int(par["min_pixels"]), "min_crops": int(par["min_crops"]), "outlier_1024": int(par["outlier"]), "outlier": int(par["outlier"]) / 1024.0},
            "model": {"medoids": [None if v is None else int(slot_ids[v]) for v in medoid], "distance": int(m["dab"]), "cost": int(m["cost"]), "voters": int(m["voters"]),
                      "neither": int(m["neither"]), "single": single},
            "teams": teams,
            "ids": [{"id": int(pid), "crops_used": int(r["used"]), "crops_skipped": int(r["skipped"]),
                     "team": "neither" if r["flags"] & lib.KIT_ID_NEITHER else (None if r["team"] < 0 else int(r["team"])), "distances": [int(r["d"][0]), int(r["d"][1])],
                     "weak": bool(r["flags"] & lib.KIT_ID_WEAK), "single": bool(r["flags"] & lib.KIT_ID_SINGLE)} for pid, r in zip(slot_ids, ids)]}
