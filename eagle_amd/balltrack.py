"""The ball track: which ball detection of every frame lies on the best physically possible path through the clip (include/eagle.h, eagle_ball_track;
csrc/balltrack.hip; tests/balltrack_ref.py is the written definition of every bit).

The table's default ball is the reference's: a frame's only ball detection is taken whatever it is, and of several the one nearest the image origin.
This stage is the project's own, opt-in answer.  Every reported ball detection is a node with a reward in proportion to its confidence; two nodes at
most ``gap`` frames apart, in one shot and within ``speed`` pixels per frame of one another can be linked at the price of their distance; a path may
also break off and start again at a fixed price.  The best path over the whole clip is found on the GPU by a dynamic program in integers; the nodes
on it are the ball, every other detection is dropped and the table interpolates over the frames without one.  A camera cut breaks the path.

The defaults (a tenth of the frame's width per frame, a window of min(64, fps) frames, a reward equal to the speed, a break of two and a half
rewards) are conventional choices, not fitted to data: a sighting of confidence 1 pays for any admissible one-frame step, and a track needs about
three sightings to pay for itself.  Limits: the first 8 candidates of a frame in descending confidence take part; the gate is in image space and of
first order (no velocity model), so a confident detection that stands still for seconds is a perfectly good path; the path is not smoothed."""
import numpy as np

from . import lib


def params(fps, frame_w, speed=None, gap=None, reward=None, brk=None, max_bytes=0):
    """EagleBallTrackParams; None (or 0): the default"""
    return lib.ball_track_params(fps, frame_w, speed or 0.0, gap or 0, reward or 0.0, brk or 0.0, max_bytes)


def track(handle, records, fps, frame_w, cuts=None, speed=None, gap=None, reward=None, brk=None):
    """-> (lib.BALL_FRAME_DTYPE [n], lib.BALL_TRACKLET_DTYPE [tracklets], lib.BALL_CLIP_DTYPE [1]); ``frames["det"]`` is what
    postprocess.process_data takes as ball_det"""
    return handle.ball_track(records, params(fps, frame_w, speed, gap, reward, brk), cuts)


def cuts_of_shots(shots, first, count):
    """the first frames of the shots (eagle_amd/shots.py) that lie inside frames first + 1 .. first + count - 1, counted from ``first``"""
    return sorted({int(s["first"]) - first for s in shots if first < int(s["first"]) < first + count})


def to_json(frames, tracklets, clip, rows=False):
    """what ball_track.json holds: the resolved parameters (half pixels, and pixels), the totals, the tracklets, with rows the frame records"""
    c = clip[0]
    out = {"parameters": {"speed_half_px": int(c["V"]), "gap_frames": int(c["G"]), "reward_half_px": int(c["R0"]), "break_half_px": int(c["B"]),
                          "speed_px": int(c["V"]) / 2.0, "reward_px": int(c["R0"]) / 2.0, "break_px": int(c["B"]) / 2.0, "max_candidates": lib.BALL_MAX_CAND},
           "totals": {k: int(c[k]) for k in ("frames_with", "frames_chosen", "rejected", "frames_multi", "tracklets", "shots", "ignored", "score")},
           "tracklets": [{"first": int(t["first"]), "last": int(t["last"]), "shot": int(t["shot"]), "sightings": int(t["sightings"]),
                          "mean_confidence": int(t["sum_cq"]) / (1024.0 * int(t["sightings"])), "length_px": int(t["length"]) / 2.0, "gain": int(t["gain"])} for t in tracklets]}
    if rows:
        out["frames"] = [{"frame": i, "candidate": int(r["cand"]), "detection": int(r["det"]), "tracklet": int(r["tracklet"]),
                          "too_many": bool(r["flags"] & lib.BALL_TOO_MANY), "shot_start": bool(r["flags"] & lib.BALL_SHOT_START),
                          "tracklet_start": bool(r["flags"] & lib.BALL_TRACKLET_START), "x": int(r["qx"]) / 2.0, "y": int(r["qy"]) / 2.0, "f": int(r["f"])}
                         for i, r in enumerate(np.asarray(frames))]
    return out
