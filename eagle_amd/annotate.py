"""Annotated output: the frames of a clip with the library's records drawn on them — what the reference's ``main.py:43-81`` writes as
``annotated.mp4``, its one aid for checking a run's output by eye: a foot ellipse and the id per player in the team colour, a triangle above
the ball, a disc per pitch key-point.

Everything is drawn on the GPU by one kernel over the clip resident in HBM (include/eagle.h, eagle_annotate_*; csrc/annotate.hip), which also
decides what a record's picture is; this module only passes arrays through and writes the container.  The rasterisation is the library's own
(parity with cv2.ellipse / cv2.putText pixels is not claimed; tests/annot_ref.py defines every pixel).  The picture shows the raw records, tracker ids as
they are; CoordinateModel.annotate(table=...) draws the post-processed table (eagle_amd/postprocess.py) instead, as main.py does."""
import numpy as np

from . import lib


def annotate(handle, d_bgr, recs, team_mapping=None, pixel_format="bgr"):
    """len(recs) frames of a dense BGR clip in HBM (handle.upload / upload_bgr) + their records -> the annotated frames on the host:
    uint8 [n, h, w, 3] ("bgr") or [n, 3h/2, w] ("nv12" / "i420").  team_mapping: {player id: 0 | 1} or None (neutral colour)."""
    return handle.annotate(d_bgr, len(recs), recs, team_mapping, pixel_format)


def overlay(rec, team_mapping=None):
    """The primitives drawn for one record, in drawing order: [(kind, a0 .. a5, (b, g, r))] with kind one of lib.PRIM_*."""
    return [(int(p["kind"]), *map(int, p["a"]), (int(p["b"]), int(p["g"]), int(p["r"]))) for p in lib.overlay_from_record(rec, team_mapping)]


def write_y4m(path, frames_i420, fps):
    """I420 frames uint8 [n, 3h/2, w] -> a YUV4MPEG2 file: one header line, then "FRAME\\n" + the frame's bytes per frame.  Common players
    open it as it is; it is how an annotated video leaves this project without an encoder library."""
    a = np.ascontiguousarray(frames_i420, np.uint8)
    if a.ndim != 3 or a.shape[1] % 3 or a.shape[2] % 2:
        raise ValueError(f"I420 frames [n, 3h/2, w] with even h and w expected (got shape {a.shape})")
    h, w = a.shape[1] * 2 // 3, a.shape[2]
    fps = int(fps) if float(fps) == int(fps) else fps
    num, den = (fps, 1) if isinstance(fps, int) else (int(round(float(fps) * 1000)), 1000)
    with open(path, "wb") as f:
        f.write(f"YUV4MPEG2 W{w} H{h} F{num}:{den} Ip A1:1 C420jpeg\n".encode())
        for fr in a:
            f.write(b"FRAME\n")
            f.write(fr.tobytes())
    return path
