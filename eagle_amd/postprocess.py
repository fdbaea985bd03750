"""The clip post-processor: the reference's ``Processor.process_data`` / ``format_data`` (eagle/processor.py:30-403, what ``main.py:34-41`` writes
as raw_data.json and processed_data.json) on the records of a finished clip.  The table is built on the GPU by the library (include/eagle.h,
eagle_postprocess; csrc/post.hip) and stays there for the annotated video; this module passes arrays through and shapes the two JSON products.
tests/post_ref.py restates the reference and is what the library is held to; where the library is defined and the reference is not is listed in
include/eagle.h."""
import math

from . import lib


def process_data(handle, records, fps, frame_w, team_mapping, smooth=False, filter_ball_detections=False, merge_ids=False, ball_det=None):
    """records: the EagleFrameResult array of the clip (record i = frame i); team_mapping: {player id: 0 | 1} (Processor.get_team_mapping) or None.
    -> lib.PostTable.  filter_ball_detections=True is refused: it needs cv2's Kalman gain, which this project cannot pin.
    merge_ids=True stitches the fragments of one person under several tracker ids into one column (the merge the reference's ``merge_data`` was
    meant to do, as a rule of this project's own: include/eagle.h, tests/stitch_ref.py); the table's ``merges`` list the joins and its
    ``team_mapping`` holds the teams the chains' heads inherit.  The default is the reference as written: no id is ever merged.
    ball_det: per record -1 or the index of the one reported ball detection that counts (the ``det`` of eagle_amd/balltrack.py's frame records); the
    table is then the one built from records without any other ball detection.  None: the reference's choice of ball."""
    if filter_ball_detections:
        raise NotImplementedError("filter_ball_detections=True is not supported: the reference's ball filter needs cv2.KalmanFilter.correct (unpinned)")
    return handle.postprocess(records, fps, frame_w, team_mapping, smooth=smooth, merge_ids=merge_ids, ball_det=ball_det)


def _cell(v):
    return None if math.isnan(v[0]) and math.isnan(v[1]) else (float(v[0]), float(v[1]))


def raw_data_rows(table):
    """What ``df.to_json(orient="records")`` serialises (main.py:36): one {column name: [x, y] | None} per kept frame, columns in table order.
    (json.dump writes the doubles in full; pandas' to_json rounds to 10 decimals.)"""
    v = table.values
    return [{n: _cell(v[c, r]) for c, n in enumerate(table.names)} for r in range(len(table.rows))]


def format_data(table):
    """``Processor.format_data`` (proc.py:89-125): the rows of processed_data.json — per kept frame the four boundary points, the pitch coordinates
    and the video coordinates of every id present ({"ID", "Coordinates", "Type"}), each list closed by the ball's entry (its Coordinates may be None)."""
    out = []
    for row in raw_data_rows(table):
        real, video = [], []
        for n, val in row.items():
            if n in lib.BOUNDARY_NAMES or val is None or "ball" in n.lower():
                continue
            (video if "video" in n else real).append({"ID": int(n.split("_")[1]), "Coordinates": val, "Type": n.split("_")[0]})
        real.append({"ID": "Ball", "Coordinates": row["Ball"]})
        video.append({"ID": "Ball", "Coordinates": row["Ball_video"]})
        out.append({"Boundaries": [row[n] for n in lib.BOUNDARY_NAMES], "Coordinates": real, "Coordinates_video": video})
    return out


def _json_safe(v):
    """(x, nan) cells: NaN is not JSON; pandas writes null."""
    if isinstance(v, tuple):
        return [None if math.isnan(e) else e for e in v]
    if isinstance(v, dict):
        return {k: _json_safe(e) for k, e in v.items()}
    if isinstance(v, list):
        return [_json_safe(e) for e in v]
    return v


def json_rows(rows):
    return _json_safe(rows)
