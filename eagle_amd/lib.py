"""ctypes binding of ``libeagle_hip.so`` (C ABI: ``include/eagle.h``).

There is deliberately **no fallback**: if the shared library is missing or a call fails, an exception is raised.
torch is not imported here — the library talks to HIP directly."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EAGLE_HIP_LIB") or os.path.join(_HERE, "libeagle_hip.so")   # override: developer A/B builds only

MAX_DET, N_LANDMARKS, MAX_KP = 300, 57, 87
PREC_F16, PREC_F32, PREC_F32S = 0, 1, 2
PRECISIONS = {"f16": PREC_F16, "f32": PREC_F32, "f32s": PREC_F32S}      # include/eagle.h EAGLE_PREC_*
DET_VARIANTS = {"n": 0, "s": 1, "m": 2, "l": 3, "x": 4}
AUTO, SMALL_BATCH = -1, 32                                             # include/eagle.h EAGLE_AUTO / EAGLE_SMALL_BATCH (use_graph: 0 off, 1 every step, 2 inside calls of >= 3 steps; multi_stream)
LETTERBOX = {"rect": 0, "square": 1}                                    # include/eagle.h EAGLE_LETTERBOX_*: ultralytics LetterBox auto=True (the .pt predictor) / auto=False (the exported ONNX detector of cm.py:54-55)
DET_PREC_AUTO = -1                                                     # include/eagle.h EAGLE_DET_PREC_AUTO
DET_PREC_MIXED = 4                                                     # include/eagle.h EAGLE_DET_PREC_MIXED (split trunk, exact last C2f per level + Detect)


class EagleError(RuntimeError):
    pass


class EagleRangeError(EagleError):
    """EAGLE_E_RANGE: the split-precision family clipped an activation at +-4094 (include/eagle.h).  The records were written and are attached as
    ``.records`` (``pad[1]`` marks the frames); they are not fp32-grade."""
    records = None


class EagleConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("frame_h", C.c_int32), ("frame_w", C.c_int32), ("det_variant", C.c_int32),
                ("det_imgsz", C.c_int32), ("batch", C.c_int32), ("precision", C.c_int32),
                ("keypoint_conf", C.c_double), ("detector_conf", C.c_double), ("ransac_thresh", C.c_double),
                ("detector_floor", C.c_float), ("nms_iou", C.c_float),
                ("ransac_max_iters", C.c_int32), ("lm_iters", C.c_int32), ("use_graph", C.c_int32), ("det_precision", C.c_int32),
                ("allow_saturation", C.c_int32), ("multi_stream", C.c_int32), ("letterbox", C.c_int32), ("reserved", C.c_int32 * 3)]


class EagleTimings(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("conv_ms", C.c_float), ("n_launches", C.c_int32),
                ("n_conv_launches", C.c_int32), ("conv_flop", C.c_double), ("sat_events", C.c_int32), ("sat_frames", C.c_int32),
                ("graph_captures", C.c_int32), ("graph_skipped", C.c_int32), ("reserved", C.c_int32 * 4)]


class EagleTrackParams(C.Structure):
    _fields_ = [("track_high_thresh", C.c_float), ("track_low_thresh", C.c_float), ("new_track_thresh", C.c_float), ("match_thresh", C.c_float),
                ("track_buffer", C.c_int32), ("frame_rate", C.c_int32)]


class EagleYuvLayout(C.Structure):
    """include/eagle.h EagleYuvLayout: byte offsets / pitches of 4:2:0 frames; 0 = the dense default of that field."""
    _fields_ = [("frame_stride", C.c_int64), ("y_pitch", C.c_int64), ("c_offset", C.c_int64), ("c_pitch", C.c_int64), ("v_offset", C.c_int64)]


PIX_FORMATS = {"nv12": 1, "i420": 2}                                   # include/eagle.h EAGLE_PIX_*
OUT_FORMATS = {"bgr": 0, "nv12": 1, "i420": 2}                         # ... of annotated output (EAGLE_PIX_BGR is an output format only)
PRIM_ARC, PRIM_LABEL, PRIM_DISC, PRIM_TRI = 0, 1, 2, 3                 # include/eagle.h EAGLE_PRIM_*
MAX_PRIMS = 2 * MAX_DET + MAX_KP + 1                                   # include/eagle.h EAGLE_MAX_PRIMS
# numpy mirror of EaglePrim (32 bytes)
PRIM_DTYPE = np.dtype([("kind", "<i4"), ("a", "<i4", 6), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("pad", "u1")], align=True)


class EaglePostParams(C.Structure):
    _fields_ = [("fps", C.c_int32), ("frame_w", C.c_int32), ("smooth", C.c_int32), ("filter_ball", C.c_int32), ("team_ids", C.c_void_p),
                ("team_vals", C.c_void_p), ("n_team", C.c_int32), ("reserved", C.c_int32), ("max_bytes", C.c_int64)]


class EagleMinimapParams(C.Structure):
    """include/eagle.h EagleMinimapParams: pixels per metre, margin, the two optional layers, radii in pixels (0 = the default)."""
    _fields_ = [("scale", C.c_int32), ("margin", C.c_int32), ("voronoi", C.c_int32), ("footprint", C.c_int32), ("player_radius", C.c_int32),
                ("ball_radius", C.c_int32), ("control", C.c_int32), ("layers", C.c_int32)]


class EagleTrailParams(C.Structure):
    """include/eagle.h EagleTrailParams: rows a trail looks back, the largest frame step inside a trail, half the line width (px), rows an arrow stays
    after the receive row, the brightness (of 256) the oldest segment fades towards."""
    _fields_ = [("window", C.c_int32), ("max_gap", C.c_int32), ("half_width", C.c_int32), ("pass_hold", C.c_int32), ("dim_floor", C.c_int32), ("reserved", C.c_int32 * 3)]


MM_TRAILS, MM_PASSES, MM_OWNER, MM_HULLS = 1, 2, 4, 8                    # include/eagle.h EAGLE_MM_*


class EagleHullParams(C.Structure):
    """include/eagle.h EagleHullParams: half the line width (px) of the minimap's hull layer."""
    _fields_ = [("half_width", C.c_int32), ("reserved", C.c_int32 * 3)]


SHAPE_HULL_CAP, SHAPE_MAX_MEMBERS, SHAPE_CUT, SHAPE_Q = 32, 4096, 1, 1024   # include/eagle.h EAGLE_SHAPE_*; positions are quantised to 1 / SHAPE_Q metres
SHAPE_DTYPE = np.dtype([("sum_x", "<i8"), ("sum_y", "<i8"), ("sum_xx", "<i8"), ("sum_yy", "<i8"), ("area2", "<i8"), ("n", "<i4"), ("hull_n", "<i4"),
                        ("flags", "<i4"), ("reserved0", "<i4"), ("min_x", "<i4"), ("max_x", "<i4"), ("min_y", "<i4"), ("max_y", "<i4"),
                        ("col_min_x", "<i4"), ("col_max_x", "<i4"), ("col_min_y", "<i4"), ("col_max_y", "<i4"), ("reserved", "<i4", 2)])      # EagleTeamShape (96 bytes)


class EagleRoleParams(C.Structure):
    """include/eagle.h EagleRoleParams: the number of roles R (2 .. ROLE_CAP), the fewest present members of a row that is assigned (2 .. R), the rounds."""
    _fields_ = [("roles", C.c_int32), ("min_present", C.c_int32), ("iterations", C.c_int32), ("reserved", C.c_int32 * 5)]


ROLE_CAP = 10                                                                # include/eagle.h EAGLE_ROLE_*
ROLE_EMPTY, ROLE_TOO_FEW, ROLE_ACTIVE, ROLE_TOO_MANY = 0, 1, 2, 3
ROLE_STATUS_NAMES = ("empty", "too_few", "active", "too_many")
ROLE_MODEL_OK, ROLE_NO_SEEDS = 0, 1
ROLE_ROW_DTYPE = np.dtype([("cost", "<i8"), ("n", "<i4"), ("status", "<i4"), ("cx", "<i4"), ("cy", "<i4"), ("col", "<i4", ROLE_CAP)])            # EagleRoleRow (64 bytes)
ROLE_GROUP_DTYPE = np.dtype([("sum", "<i8", (ROLE_CAP, 2)), ("sum2", "<i8", (ROLE_CAP, 2)), ("mean", "<i4", (ROLE_CAP, 2)), ("count", "<i4", ROLE_CAP),
                             ("status", "<i4"), ("active_rows", "<i4")])                                                                          # EagleRoleGroup (448 bytes)
ROLE_MODEL_DTYPE = np.dtype([("group", ROLE_GROUP_DTYPE, 2), ("changed", "<i4", 32)])                                                             # EagleRoleModel (1024 bytes)
assert C.sizeof(EagleRoleParams) == 32 and (ROLE_ROW_DTYPE.itemsize, ROLE_GROUP_DTYPE.itemsize, ROLE_MODEL_DTYPE.itemsize) == (64, 448, 1024)     # roles.hip asserts them too


class EagleSpaceParams(C.Structure):
    """include/eagle.h EagleSpaceParams: the grid's cells per metre (1, 2 or 4), whether the goalkeepers are sites (group 2), the marking radius in metres."""
    _fields_ = [("cells_per_metre", C.c_int32), ("goalkeepers", C.c_int32), ("radius", C.c_double), ("reserved", C.c_int32 * 4)]


SPACE_SITE_CAP = 32                                                          # include/eagle.h EAGLE_SPACE_*
SPACE_EMPTY, SPACE_ACTIVE, SPACE_TOO_MANY, SPACE_NO_OWNER = 0, 1, 2, 255
SPACE_STATUS_NAMES = ("empty", "active", "too_many")
SPACE_ROW_DTYPE = np.dtype([("status", "<i4"), ("n_sites", "<i4"), ("n", "<i4", 3), ("cells", "<i4", (3, 3)), ("reserved", "<i4", 2)])              # EagleSpaceRow (64 bytes)
SPACE_SITE_DTYPE = np.dtype([("near_d2", "<i8"), ("col", "<i4"), ("group", "<i4"), ("near_col", "<i4"), ("within", "<i4"), ("cells", "<i4", 3), ("qx", "<i4"),
                             ("qy", "<i4"), ("reserved", "<i4")])                                                                                    # EagleSpaceSite (48 bytes)
SPACE_TOTALS_DTYPE = np.dtype([("cells", "<i8", 3), ("within_sum", "<i8"), ("col", "<i4"), ("group", "<i4"), ("rows", "<i4"), ("min", "<i4"), ("max", "<i4"),
                               ("opp_rows", "<i4"), ("within_rows", "<i4"), ("reserved", "<i4")])                                                    # EagleSpaceTotals (64 bytes)
assert C.sizeof(EagleSpaceParams) == 32 and (SPACE_ROW_DTYPE.itemsize, SPACE_SITE_DTYPE.itemsize, SPACE_TOTALS_DTYPE.itemsize) == (64, 48, 64)       # space.hip asserts them too


class EagleOffsideParams(C.Structure):
    """include/eagle.h EagleOffsideParams: which way group 0 attacks (OFFSIDE_DIR_*), whether an unseen keeper is taken to stand on the goal line, the
    tolerance of a verdict in metres."""
    _fields_ = [("direction", C.c_int32), ("assume_keeper", C.c_int32), ("tolerance", C.c_double), ("reserved", C.c_int32 * 4)]


OFFSIDE_DIR_AUTO, OFFSIDE_DIR_RIGHT, OFFSIDE_DIR_LEFT = 0, 1, 2                # include/eagle.h EAGLE_OFFSIDE_*
OFFSIDE_DIR_NAMES = ("unresolved", "right", "left")
OFFSIDE_OK, OFFSIDE_NO_DIRECTION, OFFSIDE_TOO_FEW = 0, 1, 2
OFFSIDE_STATUS_NAMES = ("ok", "no_direction", "too_few")
OFFSIDE_KEEPER_ASSUMED, OFFSIDE_BY_DEFENDER, OFFSIDE_BY_BALL, OFFSIDE_BY_HALF, OFFSIDE_NO_BALL = 1, 2, 4, 8, 16
OFFSIDE_EV_OK, OFFSIDE_EV_NOT_PASS, OFFSIDE_EV_NO_RECEIVER, OFFSIDE_EV_NO_LINE = 0, 1, 2, 3
OFFSIDE_EV_STATUS_NAMES = ("ok", "not_pass", "no_receiver", "no_line")
OFFSIDE_ONSIDE, OFFSIDE_CLOSE, OFFSIDE_OFFSIDE = 1, 2, 3
OFFSIDE_VERDICT_NAMES = (None, "onside", "close", "offside")
OFFSIDE_NONE, OFFSIDE_U_MAX, OFFSIDE_U_HALF = -2 ** 31, 107520, 53760
OFFSIDE_ROW_DTYPE = np.dtype([("status", "<i4"), ("flags", "<i4"), ("line_qx", "<i4"), ("second_col", "<i4"), ("n_att", "<i4"), ("n_def", "<i4"),
                              ("keepers_seen", "<i4"), ("n_off", "<i4"), ("max_margin", "<i4"), ("max_col", "<i4"), ("reserved", "<i4", 2)])          # EagleOffsideRow (48 bytes)
OFFSIDE_TOTALS_DTYPE = np.dtype([("col", "<i4"), ("group", "<i4"), ("rows", "<i4"), ("off_rows", "<i4"), ("max_margin", "<i4"), ("reserved", "<i4", 3)])  # EagleOffsideTotals (32 bytes)
OFFSIDE_EVENT_DTYPE = np.dtype([("status", "<i4"), ("verdict", "<i4"), ("margin", "<i4"), ("line_qx", "<i4"), ("n_off", "<i4"), ("bypassed", "<i4"),
                                ("group", "<i4"), ("reserved", "<i4")])                                                                                 # EagleOffsideEvent (32 bytes)
OFFSIDE_CLIP_DTYPE = np.dtype([("direction", "<i4"), ("requested", "<i4"), ("neg", "<i4"), ("pos", "<i4"), ("zero", "<i4"), ("n_members", "<i4", 2),
                               ("n_keepers", "<i4")])                                                                                                   # EagleOffsideClip (32 bytes)
assert C.sizeof(EagleOffsideParams) == 32 and (OFFSIDE_ROW_DTYPE.itemsize, OFFSIDE_TOTALS_DTYPE.itemsize, OFFSIDE_EVENT_DTYPE.itemsize,
                                               OFFSIDE_CLIP_DTYPE.itemsize) == (48, 32, 32, 32)                                                      # offside.hip asserts them too


class EagleBallTrackParams(C.Structure):
    """include/eagle.h EagleBallTrackParams: the clip's fps and frame width, the window in frames, speed / reward / break in pixels (0: the default), the
    device-memory budget."""
    _fields_ = [("fps", C.c_int32), ("frame_w", C.c_int32), ("gap", C.c_int32), ("reserved", C.c_int32 * 5), ("speed", C.c_double), ("reward", C.c_double),
                ("brk", C.c_double), ("max_bytes", C.c_int64)]


BALL_MAX_CAND = 8                                                              # include/eagle.h EAGLE_BALL_*
BALL_TOO_MANY, BALL_SHOT_START, BALL_TRACKLET_START = 1, 2, 4
BALL_RECOVER_DEFAULT, BALL_RECOVER_DOUBLING, BALL_RECOVER_CHASE = 0, 1, 2
BALL_FRAME_DTYPE = np.dtype([("cand", "<i4"), ("det", "<i4"), ("tracklet", "<i4"), ("flags", "<i4"), ("qx", "<i4"), ("qy", "<i4"), ("f", "<i8")])     # EagleBallFrame (32 bytes)
BALL_TRACKLET_DTYPE = np.dtype([("first", "<i4"), ("last", "<i4"), ("shot", "<i4"), ("sightings", "<i4"), ("sum_cq", "<i8"), ("length", "<i8"), ("gain", "<i8"),
                                ("reserved", "<i4", 2)])                                                                                               # EagleBallTracklet (48 bytes)
BALL_CLIP_DTYPE = np.dtype([("frames_with", "<i4"), ("frames_chosen", "<i4"), ("rejected", "<i4"), ("frames_multi", "<i4"), ("tracklets", "<i4"), ("shots", "<i4"),
                            ("ignored", "<i4"), ("reserved", "<i4"), ("score", "<i8"), ("V", "<i4"), ("G", "<i4"), ("R0", "<i4"), ("B", "<i4"), ("reserved2", "<i4", 2)])  # EagleBallClip (64 bytes)
assert C.sizeof(EagleBallTrackParams) == 64 and (BALL_FRAME_DTYPE.itemsize, BALL_TRACKLET_DTYPE.itemsize, BALL_CLIP_DTYPE.itemsize) == (32, 48, 64)    # balltrack.hip asserts them too


class EagleKitParams(C.Structure):
    """include/eagle.h EagleKitParams: the least counted pixels of a used crop, the least used crops of a voter, the outlier bound in 1/1024 of the
    distance between the medoids (0: off)."""
    _fields_ = [("min_pixels", C.c_int32), ("min_crops", C.c_int32), ("outlier", C.c_int32), ("reserved", C.c_int32 * 5)]


KIT_BINS, KIT_MAX_IDS = 34, 1024                                               # include/eagle.h EAGLE_KIT_*
KIT_CROP_OUTSIDE, KIT_CROP_EMPTY, KIT_CROP_FEW = 1, 2, 4
KIT_ID_WEAK, KIT_ID_NEITHER, KIT_ID_SINGLE = 1, 2, 4
KIT_MODEL_SINGLE, KIT_MODEL_SWAPPED = 1, 2
KIT_CROP_DTYPE = np.dtype([("units", "<u4", KIT_BINS), ("n", "<i4"), ("flags", "<i4")])                                                           # EagleKitCrop (144 bytes)
KIT_ID_DTYPE = np.dtype([("used", "<i4"), ("skipped", "<i4"), ("team", "<i4"), ("flags", "<i4"), ("d", "<u4", 2), ("p", "<u4", KIT_BINS)])        # EagleKitId (160 bytes)
KIT_MODEL_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("dab", "<u4"), ("voters", "<i4"), ("cost", "<i8"), ("w", "<i8", 2), ("neither", "<i4"), ("flags", "<i4"),
                            ("team_of_a", "<i4"), ("reserved", "<i4", 3)])                                                                        # EagleKitModel (64 bytes)
assert C.sizeof(EagleKitParams) == 32 and (KIT_CROP_DTYPE.itemsize, KIT_ID_DTYPE.itemsize, KIT_MODEL_DTYPE.itemsize) == (144, 160, 64)             # kits.hip asserts them too


class EagleShotParams(C.Structure):
    """include/eagle.h EagleShotParams: cut, low and grass_thr in 1 / 65536, the window W in frames, the least length of a usable shot in frames."""
    _fields_ = [("cut", C.c_int32), ("low", C.c_int32), ("grass_thr", C.c_int32), ("window", C.c_int32), ("min_len", C.c_int32), ("reserved", C.c_int32 * 3)]


SHOT_SIGNATURE = 1537                                                        # include/eagle.h EAGLE_SHOT_*
SHOT_START, SHOT_AFTER_CUT, SHOT_AFTER_TRANSITION, SHOT_TRANSITION = 0, 1, 2, 3
SHOT_KIND_NAMES = ("start", "after_cut", "after_transition", "transition")
SHOT_FRAME_FLASH, SHOT_FRAME_HARD, SHOT_FRAME_GRADUAL_END, SHOT_FRAME_IN_TRANSITION = 1, 2, 4, 8
SHOT_PITCH, SHOT_SHORT, SHOT_USABLE = 1, 2, 4
SHOT_FRAME_DTYPE = np.dtype([("d1", "<i4"), ("d2", "<i4"), ("dW", "<i4"), ("sg", "<i4"), ("st", "<i4"), ("grass", "<u4"), ("flags", "<i4"), ("reserved", "<i4")])  # EagleShotFrame (32 bytes)
SHOT_DTYPE = np.dtype([("first", "<i4"), ("count", "<i4"), ("kind", "<i4"), ("flags", "<i4"), ("grass_sum", "<i8"), ("reserved", "<i4", 2)])                      # EagleShot (32 bytes)
assert C.sizeof(EagleShotParams) == 32 and (SHOT_FRAME_DTYPE.itemsize, SHOT_DTYPE.itemsize) == (32, 32)                                                # shots.hip asserts them too


class EagleTopviewParams(C.Structure):
    """include/eagle.h EagleTopviewParams: the canvas (scale, margin), the colours as B | G << 8 | R << 16, whether the markings are painted, whether
    the detection boxes mask the mosaic (padded by box_pad pixels), the mosaic's frames (first, step) and the least count of a mosaic pixel."""
    _fields_ = [("scale", C.c_int32), ("margin", C.c_int32), ("background", C.c_uint32), ("markings", C.c_int32), ("marking_colour", C.c_uint32),
                ("mask_boxes", C.c_int32), ("box_pad", C.c_double), ("first", C.c_int32), ("step", C.c_int32), ("min_count", C.c_int32), ("reserved", C.c_int32 * 3)]


TOPVIEW_VIDEO, TOPVIEW_MOSAIC, TOPVIEW_RESIDUAL = 1, 2, 4                    # include/eagle.h EAGLE_TOPVIEW_*
TOPVIEW_MAX_FRAMES = 1 << 23
assert C.sizeof(EagleTopviewParams) == 56                                    # topview.hip asserts it too


class EagleGroundShape(C.Structure):
    """include/eagle.h EagleGroundShape: a band (a = x0, x1, y0, y1) or a ring (a = cx, cy, r0, r1) on the pitch plane in 1 / 1024 m, its colour as
    B | G << 8 | R << 16, alpha 0 .. 256 per sub-sample, GROUND_KEYED: only where the source pixel is grass."""
    _fields_ = [("kind", C.c_int32), ("a", C.c_int32 * 6), ("colour", C.c_uint32), ("alpha", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


class EagleGroundParams(C.Structure):
    """include/eagle.h EagleGroundParams: the grass key (g >= key_min and g - max(r, b) >= key_lead); no_cull = 1 for measurements (same bytes)."""
    _fields_ = [("key_min", C.c_int32), ("key_lead", C.c_int32), ("no_cull", C.c_int32), ("reserved", C.c_int32)]


GROUND_MAX_SHAPES = 16                                                       # include/eagle.h EAGLE_GROUND_*
GROUND_BAND, GROUND_RING, GROUND_KEYED = 0, 1, 1
GROUND_SHAPE_DTYPE = np.dtype([("kind", "<i4"), ("a", "<i4", 6), ("colour", "<u4"), ("alpha", "<i4"), ("flags", "<i4"), ("reserved", "<i4", 2)])          # EagleGroundShape (48 bytes)
assert C.sizeof(EagleGroundShape) == 48 == GROUND_SHAPE_DTYPE.itemsize and C.sizeof(EagleGroundParams) == 16                                           # ground.hip asserts them too


class EagleLineFitParams(C.Structure):
    """include/eagle.h EagleLineFitParams: the line-pixel rule (k, tau, box_pad), the rounds and the ladder's top rung, the inlier radius falling from
    radius by radius_factor per round to radius_min (metres), and what a refined matrix must meet (min_points, max_shift; max_step per round)."""
    _fields_ = [("k", C.c_int32), ("tau", C.c_int32), ("rounds", C.c_int32), ("model", C.c_int32), ("min_points", C.c_int32), ("min_per_line", C.c_int32),
                ("box_pad", C.c_double), ("radius", C.c_double), ("radius_min", C.c_double), ("radius_factor", C.c_double), ("max_shift", C.c_double),
                ("max_step", C.c_double), ("reserved", C.c_int32 * 4)]


LINEFIT_NO_MAP, LINEFIT_ACCEPTED, LINEFIT_UNCHANGED, LINEFIT_FEW_POINTS, LINEFIT_NO_GAIN, LINEFIT_SHIFT = range(6)          # include/eagle.h EAGLE_LINEFIT_*
LINEFIT_STATUS = ("no_map", "accepted", "unchanged", "few_points", "no_gain", "shift")
LINEFIT_MODEL = ("none", "translation", "affine", "projective")
LINEFIT_CAUSE = ("lines", "pivot", "cap")
LINEFIT_FRAME_DTYPE = np.dtype([("status", "<i4"), ("model", "<i4"), ("rounds", "<i4"), ("n_line", "<i4"), ("n_before", "<i4"), ("n_after", "<i4"), ("fall", "<i4"),
                                ("reserved", "<i4"), ("e2_before", "<i8"), ("e2_after", "<i8"), ("shift2", "<i8")])                    # EagleLineFitFrame (56 bytes)
assert C.sizeof(EagleLineFitParams) == 88 and LINEFIT_FRAME_DTYPE.itemsize == 56                                                       # linefit.hip asserts them too


class EagleKinematicsParams(C.Structure):
    """include/eagle.h EagleKinematicsParams: frames per second, the largest frame gap that is still differenced, the speed cap (m/s)."""
    _fields_ = [("fps", C.c_int32), ("max_gap", C.c_int32), ("speed_cap", C.c_double), ("reserved", C.c_int64)]


class EagleControlParams(C.Structure):
    """include/eagle.h EagleControlParams: cells per metre (1, 2, 4), reaction time (s), top speed (m/s), softmin sharpness (1/s)."""
    _fields_ = [("cells_per_metre", C.c_int32), ("t_react", C.c_float), ("v_max", C.c_float), ("beta", C.c_float), ("reserved", C.c_int32 * 4)]


class EaglePossessionParams(C.Structure):
    """include/eagle.h EaglePossessionParams: frames per second, rows to confirm a candidate, the largest frame step inside a segment, the radius (m)."""
    _fields_ = [("fps", C.c_int32), ("min_hold", C.c_int32), ("max_gap", C.c_int32), ("reserved0", C.c_int32), ("radius", C.c_double), ("reserved", C.c_int64)]


class EagleLoadParams(C.Structure):
    """include/eagle.h EagleLoadParams: frames per second, the largest frame step that links two rows, the shortest effort in frames (speed kinds,
    acceleration kinds), the four zone edges (m/s), the speeds a high-speed run and a sprint start at (m/s), the acceleration threshold (m/s^2)."""
    _fields_ = [("fps", C.c_int32), ("max_gap", C.c_int32), ("min_frames", C.c_int32 * 2), ("zone_edges", C.c_double * 4), ("effort_speed", C.c_double * 2),
                ("accel", C.c_double), ("reserved", C.c_int64 * 2)]


LOAD_HSR, LOAD_SPRINT, LOAD_ACCEL, LOAD_DECEL, LOAD_ABSENT, LOAD_Q = 0, 1, 2, 3, 255, 1 << 20    # include/eagle.h EAGLE_LOAD_*; distances are in 1 / LOAD_Q metres
LOAD_TOTALS_DTYPE = np.dtype([("zone_frames", "<i8", 5), ("zone_dist_q", "<i8", 5), ("top_speed", "<f8"), ("col", "<i4"), ("rows_present", "<i4"),
                              ("efforts", "<i4", 4), ("reserved", "<i4", 4)])                                      # EagleLoadTotals (128 bytes)
LOAD_EFFORT_DTYPE = np.dtype([("col", "<i4"), ("kind", "<i4"), ("first_row", "<i4"), ("last_row", "<i4"), ("frames", "<i4"), ("reserved0", "<i4"),
                              ("distance_q", "<i8"), ("peak_speed", "<f8"), ("peak_accel", "<f8")])                # EagleLoadEffort (48 bytes)
assert C.sizeof(EagleLoadParams) == 88 and LOAD_TOTALS_DTYPE.itemsize == 128 and LOAD_EFFORT_DTYPE.itemsize == 48  # the sizes physical.hip asserts of the C structs


class EagleSmoothParams(C.Structure):
    """include/eagle.h EagleSmoothParams: frames per second, the half-width in frames, the degree (1, 2), the ball's half-width (0: the ball stays),
    the velocity rule's gap, the multiple of the median residual (0: no trimming), the floor (m) and the speed cap (m/s)."""
    _fields_ = [("fps", C.c_int32), ("window", C.c_int32), ("degree", C.c_int32), ("ball_window", C.c_int32), ("max_gap", C.c_int32), ("reserved0", C.c_int32),
                ("outlier_k", C.c_double), ("outlier_floor", C.c_double), ("speed_cap", C.c_double), ("reserved", C.c_int64)]


SMOOTH_FITTED, SMOOTH_OUTLIER, SMOOTH_DEGREE_SHIFT, SMOOTH_RAW, SMOOTH_Q = 1, 2, 2, 16, 1024     # the bits of a cell's flags; residual_q is in 1 / (16 SMOOTH_Q) metres
SMOOTH_TOTALS_DTYPE = np.dtype([("sum_sq", "<i8"), ("present", "<i4"), ("outliers", "<i4"), ("low_degree", "<i4"), ("max_residual_q", "<i4"), ("window", "<i4"),
                                ("reserved", "<i4")])                                                             # EagleSmoothTotals (32 bytes)
assert C.sizeof(EagleSmoothParams) == 56 and SMOOTH_TOTALS_DTYPE.itemsize == 32                                  # the sizes smooth.hip asserts of the C structs


class EagleFlightParams(C.Structure):
    """include/eagle.h EagleFlightParams: frames per second, the largest frame step inside a run, the longest segment in rows (L), the sample noise (m) and
    the penalty per segment in units of its square, the spike threshold (m), the kick threshold (m/s), possession's radius (m), the speeds (m/s) below
    which a flight is still and from which it may be a shot, a shot's range and margin (m), and the layout of the cost table (FLIGHT_LAYOUT_*)."""
    _fields_ = [("fps", C.c_double), ("max_gap", C.c_int32), ("max_rows", C.c_int32), ("noise", C.c_double), ("penalty", C.c_double), ("spike", C.c_double),
                ("kick_dv", C.c_double), ("radius", C.c_double), ("still_speed", C.c_double), ("shot_speed", C.c_double), ("shot_range", C.c_double),
                ("shot_margin", C.c_double), ("layout", C.c_int32), ("reserved", C.c_int32)]


FLIGHT_STILL, FLIGHT_CARRIED, FLIGHT_FREE = 0, 1, 2                                                              # EagleBallFlight.kind
FLIGHT_KIND_NAMES = ("still", "carried", "free")
FLIGHT_ROW_PRESENT, FLIGHT_ROW_USED, FLIGHT_ROW_SPIKE, FLIGHT_ROW_KNOT, FLIGHT_ROW_KICK = 1, 2, 4, 8, 16          # the bits of a row's flags
FLIGHT_CAPPED, FLIGHT_CONTINUES = 1, 2                                                                           # EagleBallFlight.flags
FLIGHT_LAYOUT_DEFAULT, FLIGHT_LAYOUT_END_MAJOR, FLIGHT_LAYOUT_K_MAJOR = 0, 1, 2
FLIGHT_TIMES = ("prepare", "cost", "walk", "path", "fit", "events", "total")                                     # times_ms of eagle_op_ball_flights
FLIGHT_DTYPE = np.dtype([("row0", "<i4"), ("row1", "<i4"), ("used", "<i4"), ("spikes", "<i4"), ("near", "<i4"), ("kind", "<i4"), ("shot", "<i4"), ("flags", "<i4"),
                         ("x0", "<f8"), ("y0", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("vx", "<f8"), ("vy", "<f8"), ("speed", "<f8"), ("rms", "<f8"),
                         ("y_cross", "<f8"), ("c", "<i8")])                                                       # EagleBallFlight (112 bytes)
KICK_DTYPE = np.dtype([("row", "<i4"), ("seg_in", "<i4"), ("seg_out", "<i4"), ("col", "<i4"), ("speed_in", "<f8"), ("speed_out", "<f8"), ("dv", "<f8"),
                       ("cos_turn", "<f8")])                                                                      # EagleBallKick (48 bytes)
FLIGHT_TOTALS_DTYPE = np.dtype([("runs", "<i4"), ("flights", "<i4"), ("kinds", "<i4", 3), ("spikes", "<i4"), ("knots", "<i4"), ("kicks", "<i4"),
                                ("shots", "<i4", 3), ("capped", "<i4"), ("sum_c", "<i8"), ("reserved", "<i8")])   # EagleFlightTotals (64 bytes)
assert C.sizeof(EagleFlightParams) == 96 and FLIGHT_DTYPE.itemsize == 112 and KICK_DTYPE.itemsize == 48 and FLIGHT_TOTALS_DTYPE.itemsize == 64


class EagleGoalViewParams(C.Structure):
    """include/eagle.h EagleGoalViewParams: the direction group 0 attacks (OFFSIDE_DIR_RIGHT / _LEFT; 0: the table's offside result's), the grid's attacking
    group (0, 1, -1: the owner's), its cells per metre (1, 2, 4), the form of the grid kernel's weights (GOALVIEW_FORM_*), the grid's table rows (grid_rows 0:
    no grid), the radii of an outfield player and a keeper (m), the least depth and the largest range of an evaluated point (m), the angle of a chance (rad)."""
    _fields_ = [("direction", C.c_int32), ("group", C.c_int32), ("cells_per_metre", C.c_int32), ("form", C.c_int32), ("grid_row0", C.c_int32), ("grid_rows", C.c_int32),
                ("radius", C.c_double), ("keeper_radius", C.c_double), ("min_depth", C.c_double), ("max_range", C.c_double), ("chance", C.c_double),
                ("reserved", C.c_int32 * 2)]


GOALVIEW_BLOCKERS, GOALVIEW_SLICES = 32, 64
GOALVIEW_OK, GOALVIEW_TOO_MANY = 0, 1                                                                            # EagleGoalViewRow.status
GOALVIEW_PT_OK, GOALVIEW_PT_ABSENT, GOALVIEW_PT_ROW, GOALVIEW_PT_NEAR_LINE, GOALVIEW_PT_FAR = 0, 1, 2, 3, 4      # a point's status
GOALVIEW_PT_NAMES = ("ok", "absent", "too_many", "near_line", "far")
GOALVIEW_FORM_DEFAULT, GOALVIEW_FORM_DIRECT, GOALVIEW_FORM_TABLE = 0, 1, 2
GOALVIEW_TIMES = ("prepare", "points", "rows", "table", "grid", "total")                                         # times_ms of eagle_op_goal_view
GOALVIEW_ROW_DTYPE = np.dtype([("status", "<i4"), ("n_blockers", "<i4"), ("ball_status", "<i4"), ("ball_open", "<i4"), ("ball_full", "<i4"), ("best_col", "<i4"),
                               ("best_open", "<i4"), ("owner_col", "<i4"), ("owner_open", "<i4"), ("reserved", "<i4"), ("ball_mask", "<u8"),
                               ("owner_mask", "<u8")])                                                            # EagleGoalViewRow (56 bytes)
GOALVIEW_TOTALS_DTYPE = np.dtype([("col", "<i4"), ("group", "<i4"), ("rows", "<i4"), ("max_open", "<i4"), ("max_row", "<i4"), ("chance_rows", "<i4"),
                                  ("sum_open", "<i8")])                                                           # EagleGoalViewTotals (32 bytes)
assert C.sizeof(EagleGoalViewParams) == 72 and GOALVIEW_ROW_DTYPE.itemsize == 56 and GOALVIEW_TOTALS_DTYPE.itemsize == 32


class EagleStabParams(C.Structure):
    """include/eagle.h EagleStabParams: frames per second, the half-width in frames, the degree (1, 2), the model (0 translation, 1 affine), the fewest
    voters of a row, the rounds, the trimming multiple (0: none), its floor (m), the least spread
    of the inliers (m) and the largest gain of the affine map, and the shift (m) above which a row is flagged as a jump."""
    _fields_ = [("fps", C.c_int32), ("window", C.c_int32), ("degree", C.c_int32), ("model", C.c_int32), ("min_voters", C.c_int32), ("iterations", C.c_int32),
                ("reserved0", C.c_int32 * 2), ("trim_k", C.c_double), ("floor", C.c_double), ("min_spread", C.c_double),
                ("max_gain", C.c_double), ("jump", C.c_double), ("reserved", C.c_int64)]


STAB_OVER_CAP, STAB_FEW, STAB_SPREAD, STAB_CORR, STAB_GAIN, STAB_JUMP, STAB_Q = 1, 2, 4, 8, 16, 32, 1024     # the bits of a row's flags; shift_q is in 1 / STAB_Q metres
STAB_ROW_DTYPE = np.dtype([("voters", "<i4"), ("inliers", "<i4"), ("model", "<i4"), ("flags", "<i4"), ("shift_q", "<i4", (2,)), ("centre_q", "<i4", (2,)),
                           ("offset", "<f8", (2,)), ("gain", "<f8", (4,)), ("ss_before", "<i8"), ("ss_after", "<i8"), ("moved", "<i4"), ("reserved", "<i4")])   # EagleStabRow
STAB_TOTALS_DTYPE = np.dtype([("ss_before", "<i8"), ("ss_after", "<i8"), ("inliers", "<i8"), ("moved", "<i8"), ("rows", "<i4"), ("none", "<i4"), ("translation", "<i4"),
                              ("affine", "<i4"), ("few_inliers", "<i4"), ("low_spread", "<i4"), ("correlated", "<i4"), ("high_gain", "<i4"), ("jumps", "<i4"),
                              ("over_cap", "<i4"), ("iterations", "<i4"), ("window", "<i4")])                      # EagleStabTotals
assert C.sizeof(EagleStabParams) == 80 and STAB_ROW_DTYPE.itemsize == 104 and STAB_TOTALS_DTYPE.itemsize == 80      # the sizes stab.hip asserts of the C structs


class EaglePassOptionParams(C.Structure):
    """include/eagle.h EaglePassOptionParams: cells per metre (1, 2, 4), lane samples K (1 .. 64), reaction time (s), top speed (m/s), sharpness (1/s),
    ball speed (m/s)."""
    _fields_ = [("cells_per_metre", C.c_int32), ("samples", C.c_int32), ("t_react", C.c_float), ("v_max", C.c_float), ("beta", C.c_float), ("v_ball", C.c_float),
                ("reserved", C.c_int32 * 2)]


PASS_ACTIVE, PASS_NO_OWNER, PASS_IN_FLIGHT, PASS_NO_TEAM, PASS_OFF_DOMAIN = 0, 1, 2, 3, 4    # include/eagle.h EAGLE_PASS_*
PASS_STATUS_NAMES = ("active", "no_owner", "in_flight", "no_team", "off_domain")
PASS_MAX_SITES = 1024
PASS_ROW_DTYPE = np.dtype([("status", "<i4"), ("owner_col", "<i4"), ("group", "<i4"), ("n_mates", "<i4"), ("n_defenders", "<i4"), ("best_col", "<i4"),
                           ("best_byte", "<i4"), ("reserved", "<i4"), ("sum", "<i8")])                             # EaglePassOptionRow (40 bytes)
assert C.sizeof(EaglePassOptionParams) == 32 and PASS_ROW_DTYPE.itemsize == 40      # the sizes options.hip asserts of the C structs


class EagleOccupancyParams(C.Structure):
    """include/eagle.h EagleOccupancyParams: frames per second, the largest frame step a row may stand for, cells per metre, the Gaussian's sigma (m)."""
    _fields_ = [("fps", C.c_int32), ("max_gap", C.c_int32), ("cells_per_metre", C.c_int32), ("reserved0", C.c_int32), ("sigma", C.c_double), ("reserved", C.c_int64)]


POST_PLAYER, POST_GOALKEEPER, POST_BALL, POST_BOUNDARY = 0, 1, 2, 3    # include/eagle.h EAGLE_POST_*
POST_NO_BALL = 1                                                       # ... flag: fewer than two ball sightings
POSTCOL_DTYPE = np.dtype([("kind", "<i4"), ("id", "<i4"), ("video", "<i4"), ("reserved", "<i4")])      # EaglePostColumn
POSTMERGE_DTYPE = np.dtype([("kind", "<i4"), ("from_id", "<i4"), ("to_id", "<i4"), ("head_id", "<i4"), ("gap_frames", "<i4"), ("team", "<i4"),
                            ("dist", "<f8")])                                                          # EaglePostMerge
EVENT_PASS, EVENT_TURNOVER, EVENT_UNKNOWN = 0, 1, 2                    # include/eagle.h EAGLE_EVENT_*
EVENT_DTYPE = np.dtype([("row", "<i4"), ("from_col", "<i4"), ("to_col", "<i4"), ("release_row", "<i4"), ("receive_row", "<i4"), ("kind", "<i4"),
                        ("reserved", "<i4", 2), ("x0", "<f8"), ("y0", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("length", "<f8"),
                        ("duration", "<f8")])                                                          # EaglePossessionEvent (80 bytes)
E_INVALID = -1


class EagleKernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 40), ("ms", C.c_float), ("launches", C.c_int32), ("bytes", C.c_double), ("flop", C.c_double)]


# numpy mirrors of the record structs (C layout, natural alignment — checked against sizeof in tests)
DET_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("conf", "<f4"), ("cls", "<i4"),
                      ("id", "<i4"), ("bx1", "<i4"), ("by1", "<i4"), ("bx2", "<i4"), ("by2", "<i4"),
                      ("foot_x", "<i4"), ("foot_y", "<i4"), ("pitch_xf", "<f4"), ("pitch_yf", "<f4"),
                      ("pitch_x", "<i4"), ("pitch_y", "<i4"), ("reported", "u1"), ("in_bounds", "u1"), ("pad", "u1", 2)],
                     align=True)
KP_DTYPE = np.dtype([("label", "<i4"), ("x", "<i4"), ("y", "<i4"), ("score", "<f4"), ("synthesized", "u1"),
                     ("on_plane", "u1"), ("inlier", "u1"), ("pad", "u1")], align=True)
RESULT_DTYPE = np.dtype([("n_det", "<i4"), ("n_kp", "<i4"), ("n_candidates", "<i4"), ("H_valid", "u1"),
                         ("bounds_valid", "u1"), ("pad", "u1", 2), ("H", "<f8", 9), ("bounds", "<f8", 4),
                         ("hm_idx", "<i4", N_LANDMARKS), ("hm_score", "<f4", N_LANDMARKS),
                         ("kp", KP_DTYPE, MAX_KP), ("det", DET_DTYPE, MAX_DET)], align=True)

_lib = None


def require_torch_first():
    """One process must hold ONE ROCm runtime.  PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 / librccl (SONAMEs identical
    to /opt/rocm's): when torch is imported BEFORE this library is loaded, the dynamic loader binds libeagle_hip.so and the dlopen'ed RCCL to
    torch's copies by SONAME — one runtime.  The other order maps /opt/rocm's runtime first and torch's second copy next to it (torch asks for
    "libamdhip64.so", which matches no SONAME): two HSA runtimes in one process, which is what aborted at interpreter exit in round 3
    (DESIGN.md §8).  Called by every code path of this package that imports torch after the library may have been loaded.  The gate is the
    dlopen itself (``load()``: it is libeagle_hip.so's NEEDED entry that maps /opt/rocm's libamdhip64), not the first handle."""
    import sys
    if "torch" not in sys.modules and _lib is not None:
        raise EagleError("torch must be imported before eagle_amd.lib loads libeagle_hip.so in a process that uses both "
                         "(two ROCm runtimes would be mapped: torch's bundled one and /opt/rocm's); import torch first, or keep the process torch-free")


def load():
    """Load the shared library and declare the prototypes.  Raises EagleError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EagleError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(there is no CPU fallback for the product path)")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    fp, dp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    L.eagle_abi_sizes.argtypes = [C.POINTER(C.c_int32)]
    L.eagle_default_config.argtypes = [C.POINTER(EagleConfig)]
    L.eagle_create.argtypes = [C.POINTER(EagleConfig), C.POINTER(vp)]
    L.eagle_destroy.argtypes = [vp]
    L.eagle_destroy.restype = None
    L.eagle_last_error.argtypes = [vp]
    L.eagle_last_error.restype = C.c_char_p
    L.eagle_get_config.argtypes = [vp, C.POINTER(EagleConfig)]
    L.eagle_resolve_config.argtypes = [C.POINTER(EagleConfig)]
    L.eagle_load_weights.argtypes = [vp, C.c_char_p, fp, C.POINTER(i64), i32]
    L.eagle_finalize_weights.argtypes = [vp]
    L.eagle_process_frames.argtypes = [vp, u8p, i32, i64, i64, vp]
    L.eagle_process_device_frames.argtypes = [vp, vp, i32, vp]
    L.eagle_host_alloc.argtypes = [vp, i64, C.POINTER(vp)]
    L.eagle_host_free.argtypes = [vp, vp]
    L.eagle_device_alloc.argtypes = [vp, i64, C.POINTER(vp)]
    L.eagle_device_free.argtypes = [vp, vp]
    L.eagle_device_upload.argtypes = [vp, vp, vp, i64]
    L.eagle_reproject.argtypes = [vp, vp, i32, dp, u8p]
    L.eagle_clip_open.argtypes = [vp, vp, i32]
    L.eagle_clip_close.argtypes = [vp]
    L.eagle_clip_detect_keypoints.argtypes = [vp, i32, i32, i32]
    L.eagle_clip_get_keypoints.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.eagle_clip_set_keypoints.argtypes = [vp, i32, vp, i32]
    L.eagle_clip_flow.argtypes = [vp, i32, i32, i32, vp, i32, vp, C.POINTER(i32), fp, u8p]
    L.eagle_clip_run.argtypes = [vp, i32, i32, i32, i32, i32, i32, C.POINTER(i32)]
    L.eagle_clip_detect_objects.argtypes = [vp, i32, i32]
    L.eagle_clip_fetch.argtypes = [vp, vp]
    L.eagle_comm_id.argtypes = [vp]
    L.eagle_comm_init.argtypes = [vp, i32, i32, vp]
    L.eagle_gather.argtypes = [vp, vp, i32, vp]
    L.eagle_set_profiling.argtypes = [vp, i32]
    L.eagle_get_timings.argtypes = [vp, C.POINTER(EagleTimings)]
    L.eagle_get_kernel_times.argtypes = [vp, C.POINTER(EagleKernelTime), i32, C.POINTER(i32)]
    L.eagle_op_conv2d.argtypes = [i32, i32, fp, i32, i32, i32, i32, fp, fp, i32, i32, i32, i32, fp, fp, i32, fp]
    L.eagle_op_bottleneck.argtypes = [i32, fp, i32, i32, i32, i32, fp, fp, fp, fp, fp, fp, fp, fp, i32, fp, fp, fp]
    L.eagle_op_stem.argtypes = [i32, u8p, i32, i32, i32, i32, i32, fp, fp, fp, C.POINTER(C.c_uint32)]
    L.eagle_op_fuse_sum.argtypes = [i32, i32, fp, i32, i32, i32, i32, i32, C.POINTER(fp), C.POINTER(i32), C.POINTER(i32), i32, fp]
    L.eagle_op_preprocess.argtypes = [i32, i32, u8p, i32, i32, i32, i32, fp, fp, C.POINTER(i32)]
    L.eagle_op_preprocess_lb.argtypes = [i32, i32, u8p, i32, i32, i32, i32, i32, fp, fp, C.POINTER(i32)]
    L.eagle_op_find_homography.argtypes = [i32, fp, fp, i32, C.c_double, i32, i32, dp, u8p, C.POINTER(i32)]
    L.eagle_op_detect_tail.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i32), fp, C.POINTER(fp), C.POINTER(fp), i32, i32, C.c_float, C.c_float, C.c_double,
                                       i32, i32, i32, i32, vp, fp, fp, C.POINTER(C.c_int32)]
    L.eagle_op_post.argtypes = [i32, i32, i32, i32, i32, fp, vp, vp, vp, i32, i32, C.c_double, C.c_double, i32, i32]
    L.eagle_op_conv2d_argmax.argtypes = [i32, i32, fp, i32, i32, i32, i32, fp, fp, i32, i32, i32, fp, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.eagle_op_conv_config.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_int32)]
    L.eagle_op_conv_table.argtypes = [i32, C.POINTER(C.c_int32), i32]
    L.eagle_debug.argtypes = [C.c_char_p, i64, vp, i64]
    L.eagle_team_colors.argtypes = [vp, vp, i32, vp, i32, vp]
    L.eagle_track_open.argtypes = [vp, C.POINTER(EagleTrackParams)]
    L.eagle_track_frames.argtypes = [vp, vp, i32]
    L.eagle_track_frames_cmc.argtypes = [vp, vp, i32, C.POINTER(C.c_double)]
    L.eagle_clip_motion.argtypes = [vp, i32, i32, C.POINTER(C.c_double)]
    L.eagle_clip_motion_ecc.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_double), C.POINTER(i32)]
    L.eagle_reid_features.argtypes = [vp, vp, i32, vp, i32, fp]
    yl = C.POINTER(EagleYuvLayout)
    L.eagle_process_frames_yuv.argtypes = [vp, i32, u8p, i32, yl, vp]
    L.eagle_process_device_frames_yuv.argtypes = [vp, i32, vp, i32, yl, vp]
    L.eagle_yuv_to_bgr.argtypes = [vp, i32, vp, i32, yl, vp]
    L.eagle_op_yuv_to_bgr.argtypes = [i32, i32, u8p, i32, i32, i32, yl, u8p]
    L.eagle_track_frames_reid.argtypes = [vp, vp, i32, C.POINTER(C.c_double), fp, C.POINTER(i32), C.POINTER(i32)]
    L.eagle_annotate_device_frames.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, yl, vp]
    L.eagle_annotate_frames.argtypes = [vp, vp, i32, vp, vp, vp, i32, i32, yl, vp]
    L.eagle_overlay_from_record.argtypes = [vp, vp, vp, i32, vp, i32, C.POINTER(i32)]
    L.eagle_op_annotate.argtypes = [i32, u8p, i32, i32, i32, vp, vp, i32, yl, u8p]
    L.eagle_annotate_frames_prims.argtypes = [vp, vp, i32, vp, vp, i32, yl, vp]
    L.eagle_postprocess.argtypes = [vp, vp, i32, C.POINTER(EaglePostParams), C.POINTER(vp)]
    L.eagle_post_free.argtypes = [vp]
    L.eagle_post_free.restype = None
    L.eagle_post_shape.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.eagle_post_layout.argtypes = [vp, vp, vp]
    L.eagle_post_values.argtypes = [vp, vp]
    L.eagle_post_device_values.argtypes = [vp, C.POINTER(vp)]
    L.eagle_post_merges.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_overlay_from_table.argtypes = [vp, i32, vp, vp, i32, C.POINTER(i32)]
    mp = C.POINTER(EagleMinimapParams)
    L.eagle_minimap_size.argtypes = [mp, C.POINTER(i32), C.POINTER(i32)]
    L.eagle_minimap_device_frames.argtypes = [vp, vp, i32, i32, mp, i32, yl, vp]
    L.eagle_minimap_frames.argtypes = [vp, vp, i32, i32, mp, i32, yl, vp]
    L.eagle_op_minimap.argtypes = [i32, vp, vp, i32, i32, vp, vp, i32, mp, i32, i32, i32, yl, vp]
    kp, cp = C.POINTER(EagleKinematicsParams), C.POINTER(EagleControlParams)
    L.eagle_post_velocities.argtypes = [vp, vp, kp]
    L.eagle_post_velocity_values.argtypes = [vp, vp]
    L.eagle_post_device_velocity_values.argtypes = [vp, C.POINTER(vp)]
    L.eagle_control_size.argtypes = [cp, C.POINTER(i32), C.POINTER(i32)]
    L.eagle_control_device_grids.argtypes = [vp, vp, i32, i32, cp, vp, vp]
    L.eagle_control_grids.argtypes = [vp, vp, i32, i32, cp, vp, vp]
    L.eagle_minimap_set_control.argtypes = [vp, cp]
    L.eagle_op_velocities.argtypes = [i32, vp, vp, i32, i32, kp, vp]
    L.eagle_op_control.argtypes = [i32, vp, vp, vp, i32, i32, vp, vp, i32, cp, i32, i32, vp, vp]
    L.eagle_op_minimap_control.argtypes = [i32, vp, vp, vp, i32, i32, vp, vp, i32, mp, cp, i32, i32, i32, yl, vp]
    pp = C.POINTER(EaglePossessionParams)
    L.eagle_post_possession.argtypes = [vp, vp, pp]
    L.eagle_post_possession_values.argtypes = [vp, vp, vp, vp]
    L.eagle_post_device_possession.argtypes = [vp, C.POINTER(vp)]
    L.eagle_post_events.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_op_possession.argtypes = [i32, vp, vp, vp, i32, i32, vp, vp, i32, pp, vp, vp, vp, vp, i32, C.POINTER(C.c_int)]
    po = C.POINTER(EaglePassOptionParams)
    L.eagle_pass_options_size.argtypes = [po, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.eagle_pass_options_layout.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_pass_options_device.argtypes = [vp, vp, i32, i32, po, vp, vp, vp]
    L.eagle_pass_options.argtypes = [vp, vp, i32, i32, po, vp, vp, vp]
    L.eagle_op_pass_options.argtypes = [i32, vp, vp, vp, i32, i32, vp, vp, i32, vp, vp, po, i32, i32, vp, vp, vp]
    op = C.POINTER(EagleOccupancyParams)
    L.eagle_occupancy_size.argtypes = [op, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.eagle_post_occupancy.argtypes = [vp, vp, op, vp, vp, i32]
    L.eagle_post_occupancy_values.argtypes = [vp, vp, vp, vp, vp, vp]
    L.eagle_post_device_occupancy.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.eagle_occupancy_picture.argtypes = [vp, vp, i32, i32, i32, C.c_uint32, vp]
    L.eagle_op_occupancy.argtypes = [i32, vp, vp, vp, i32, i32, op, vp, vp, i32, vp, vp, vp, vp, vp]
    L.eagle_op_occupancy_picture.argtypes = [i32, vp, i32, i32, i32, C.c_uint32, vp]
    tp = C.POINTER(EagleTrailParams)
    L.eagle_minimap_set_trails.argtypes = [vp, tp, vp, i32]
    L.eagle_trajectory_picture.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.eagle_pass_picture.argtypes = [vp, vp, i32, i32, i32, i32, vp]
    L.eagle_op_minimap_trails.argtypes = [i32, vp, vp, vp, i32, i32, vp, vp, i32, mp, tp, vp, i32, vp, vp, i32, i32, i32, i32, yl, vp]
    L.eagle_op_trajectory_picture.argtypes = [i32, vp, vp, vp, i32, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, vp]
    L.eagle_op_pass_picture.argtypes = [i32, vp, vp, i32, i32, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp]
    hp = C.POINTER(EagleHullParams)
    L.eagle_post_team_shape.argtypes = [vp, vp]
    L.eagle_post_team_shape_values.argtypes = [vp, vp, vp]
    L.eagle_post_device_team_shape.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.eagle_minimap_set_hulls.argtypes = [vp, hp]
    L.eagle_op_team_shape.argtypes = [i32, vp, vp, i32, i32, vp, vp, i32, vp, vp]
    L.eagle_op_minimap_hulls.argtypes = [i32, vp, vp, vp, i32, i32, vp, vp, i32, mp, hp, tp, vp, i32, vp, vp, i32, i32, i32, i32, yl, vp]
    rp = C.POINTER(EagleRoleParams)
    L.eagle_post_roles.argtypes = [vp, vp, rp]
    L.eagle_post_roles_values.argtypes = [vp, vp, vp, vp]
    L.eagle_post_device_roles.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
    L.eagle_op_roles.argtypes = [i32, vp, vp, i32, i32, vp, vp, i32, rp, vp, vp, vp]
    sp = C.POINTER(EagleSpaceParams)
    L.eagle_post_space.argtypes = [vp, vp, sp]
    L.eagle_post_space_values.argtypes = [vp, vp, vp, vp]
    L.eagle_post_device_space.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int)]
    L.eagle_space_device_grids.argtypes = [vp, vp, i32, i32, sp, vp]
    L.eagle_space_grids.argtypes = [vp, vp, i32, i32, sp, vp]
    L.eagle_op_space.argtypes = [i32, vp, vp, i32, i32, vp, vp, i32, sp, i32, i32, vp, vp, vp, vp]
    ofp = C.POINTER(EagleOffsideParams)
    L.eagle_post_offside.argtypes = [vp, vp, ofp]
    L.eagle_post_offside_values.argtypes = [vp, vp, vp, vp, vp]
    L.eagle_post_offside_events.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_post_device_offside.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.eagle_op_offside.argtypes = [i32, vp, vp, vp, i32, i32, vp, vp, i32, ofp, vp, i32, vp, vp, vp, vp, vp]
    btp = C.POINTER(EagleBallTrackParams)
    L.eagle_ball_track.argtypes = [vp, vp, i32, vp, i32, btp, C.POINTER(vp)]
    L.eagle_ball_track_values.argtypes = [vp, vp, vp]
    L.eagle_ball_track_tracklets.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_ball_track_free.argtypes = [vp]
    L.eagle_ball_track_free.restype = None
    L.eagle_op_ball_track.argtypes = [i32, vp, i32, vp, vp, vp, vp, vp, i32, btp, i32, vp, vp, i32, vp, vp]
    L.eagle_postprocess_ball.argtypes = [vp, vp, i32, C.POINTER(EaglePostParams), vp, C.POINTER(vp)]
    ktp = C.POINTER(EagleKitParams)
    L.eagle_kit_params_default.argtypes = [ktp]
    L.eagle_team_cluster.argtypes = [vp, vp, i32, vp, vp, i32, i32, ktp, vp, vp, vp]
    L.eagle_op_team_cluster.argtypes = [i32, vp, i32, i32, i32, vp, vp, i32, i32, ktp, vp, vp, vp, vp]
    L.eagle_op_team_cluster_ids.argtypes = [i32, vp, vp, i32, ktp, vp, vp, vp]
    shp = C.POINTER(EagleShotParams)
    L.eagle_shots_device_frames.argtypes = [vp, vp, i32, shp, vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_shots_frames.argtypes = [vp, vp, i32, i64, i64, i64, shp, vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_op_shots.argtypes = [i32, vp, i32, i32, i32, shp, vp, vp, i32, C.POINTER(C.c_int), vp]
    tvp, lay = C.POINTER(EagleTopviewParams), C.POINTER(EagleYuvLayout)
    L.eagle_topview_size.argtypes = [tvp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.eagle_topview_device_frames.argtypes = [vp, vp, i32, vp, vp, tvp, i32, lay, vp]
    L.eagle_topview_frames.argtypes = [vp, vp, i32, vp, vp, tvp, i32, lay, vp]
    L.eagle_topview_mosaic_device.argtypes = [vp, vp, i32, vp, vp, vp, tvp, vp, i32]
    L.eagle_topview_mosaic_finish.argtypes = [vp, vp, tvp, vp, vp]
    L.eagle_topview_residual_device.argtypes = [vp, vp, i32, vp, vp, vp, tvp, vp, vp, vp, vp]
    L.eagle_topview_mosaic_frames.argtypes = [vp, vp, i32, i64, vp, vp, vp, tvp, vp, i32]
    L.eagle_topview_residual_frames.argtypes = [vp, vp, i32, i64, vp, vp, vp, tvp, vp, vp, vp, vp]
    L.eagle_op_topview.argtypes = [i32, vp, i32, i32, i32, vp, vp, vp, vp, tvp, i32, i32, lay, vp, vp, vp, vp, vp, vp]
    grp = C.POINTER(EagleGroundParams)
    L.eagle_ground_device_frames.argtypes = [vp, vp, i32, vp, vp, vp, vp, grp, i32, lay, vp, vp]
    L.eagle_ground_frames.argtypes = [vp, vp, i32, i64, vp, vp, vp, vp, grp, i32, lay, vp, vp]
    L.eagle_op_ground.argtypes = [i32, vp, i32, i32, i32, vp, vp, vp, vp, grp, i32, lay, vp, vp]
    lfp = C.POINTER(EagleLineFitParams)
    L.eagle_linefit_params_default.argtypes = [lfp]
    L.eagle_linefit_device_frames.argtypes = [vp, vp, i32, vp, vp, vp, lfp, vp, vp, vp]
    L.eagle_linefit_frames.argtypes = [vp, vp, i32, i64, vp, vp, vp, lfp, vp, vp, vp]
    L.eagle_op_linefit.argtypes = [i32, vp, i32, i32, i32, vp, vp, vp, vp, lfp, vp, vp, vp]
    lp = C.POINTER(EagleLoadParams)
    sp = C.POINTER(EagleSmoothParams)
    L.eagle_post_smooth_tracks.argtypes = [vp, vp, sp]
    L.eagle_post_smooth_values.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.eagle_post_device_smooth.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.eagle_post_raw_values.argtypes = [vp, vp]
    L.eagle_op_smooth_tracks.argtypes = [i32, vp, vp, vp, i32, i32, sp, vp, vp, vp, vp, vp, vp, vp, vp]
    stp = C.POINTER(EagleStabParams)
    L.eagle_post_stabilise.argtypes = [vp, vp, stp]
    L.eagle_post_stabilise_values.argtypes = [vp, vp, vp, vp]
    L.eagle_post_original_values.argtypes = [vp, vp]
    L.eagle_post_device_stabilise.argtypes = [vp, C.POINTER(vp)]
    L.eagle_op_stabilise.argtypes = [i32, vp, vp, vp, i32, i32, stp, vp, vp, vp, vp]
    L.eagle_post_physical.argtypes = [vp, vp, lp]
    L.eagle_post_physical_values.argtypes = [vp, vp, vp, vp]
    L.eagle_post_physical_totals.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_post_physical_efforts.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_post_device_physical.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.eagle_op_physical.argtypes = [i32, vp, vp, vp, i32, i32, lp, vp, vp, vp, vp, i32, C.POINTER(C.c_int), vp, i32, C.POINTER(C.c_int)]
    L.eagle_op_reid_crop.argtypes = [i32, u8p, i32, i32, i32, vp, i32, i32, i32, i32, i32, fp]
    L.eagle_op_reid_conv7.argtypes = [i32, fp, i32, i32, i32, i32, i32, fp, fp, i32, i32, fp]
    L.eagle_op_reid_maxpool3s2.argtypes = [i32, fp, i32, i32, i32, i32, i32, i32, i32, i32, fp]
    L.eagle_op_reid_avgpool2.argtypes = [i32, fp, i32, i32, i32, i32, i32, i32, i32, i32, fp]
    L.eagle_op_reid_dw3.argtypes = [i32, fp, i32, i32, i32, i32, i32, i32, fp, fp, i32, i32, fp]
    L.eagle_op_reid_gate.argtypes = [i32, C.POINTER(fp), i32, i32, i32, i32, i32, i32, fp, fp, fp, fp, i32, i32, i32, i32, fp, fp]
    L.eagle_op_reid_head.argtypes = [i32, fp, i32, i32, i32, i32, i32, i32, fp, fp, i32, fp]
    L.eagle_op_conv2d_sliced.argtypes = [i32, i32, fp, i32, i32, i32, i32, i32, i32, fp, fp, i32, i32, i32, i32, fp, i32, i32, i32, fp, i32, i32, i32, i32, i32, i32, fp]
    L.eagle_op_maxpool5.argtypes = [i32, i32, fp, i32, i32, i32, i32, i32, i32, i32, i32, i32, fp]
    L.eagle_op_upsample2.argtypes = [i32, i32, fp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, fp]
    L.eagle_op_split_to_f32.argtypes = [i32, fp, i32, i32, i32, i32, i32, i32, i32, i32, fp]
    L.eagle_op_gray_pyramid.argtypes = [i32, u8p, i32, i32, i32, u8p, u8p, u8p, C.POINTER(i32)]
    L.eagle_op_flow.argtypes = [i32, u8p, i32, i32, i32, i32, i32, i32, vp, i32, vp, C.POINTER(i32), fp, u8p]
    L.eagle_op_ecc_small.argtypes = [i32, u8p, i32, i32, i32, C.c_double, u8p, C.POINTER(i32), C.POINTER(i32)]
    L.eagle_op_ecc.argtypes = [i32, u8p, i32, i32, i32, u8p, C.POINTER(i32), i32, i32, C.c_double, vp]
    flp = C.POINTER(EagleFlightParams)
    L.eagle_flight_params_default.argtypes = [flp, C.c_double, i32]
    L.eagle_post_ball_flights.argtypes = [vp, vp, flp, vp, i32]
    L.eagle_post_ball_flight_values.argtypes = [vp, vp, vp, vp, vp, vp]
    L.eagle_post_ball_flight_records.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_post_ball_kicks.argtypes = [vp, vp, i32, C.POINTER(C.c_int)]
    L.eagle_post_device_ball_flights.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.eagle_op_ball_flights.argtypes = [i32, vp, vp, vp, i32, i32, vp, i32, flp, vp, vp, vp, vp, vp, i32, C.POINTER(C.c_int), vp, i32, C.POINTER(C.c_int), vp, vp]
    gvp = C.POINTER(EagleGoalViewParams)
    L.eagle_goal_view_params_default.argtypes = [gvp]
    L.eagle_post_goal_view.argtypes = [vp, vp, gvp]
    L.eagle_post_goal_view_values.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.eagle_post_device_goal_view.argtypes = [vp] + [C.POINTER(vp)] * 6 + [C.POINTER(C.c_int)] * 4
    L.eagle_op_goal_view.argtypes = [i32, vp, vp, i32, i32, vp, vp, i32, vp, gvp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int), vp]
    _lib = L
    return L


EXPORTS = ["eagle_abi_sizes", "eagle_default_config", "eagle_create", "eagle_destroy", "eagle_last_error", "eagle_get_config", "eagle_resolve_config", "eagle_load_weights",
           "eagle_finalize_weights", "eagle_process_frames", "eagle_process_device_frames", "eagle_device_alloc",
           "eagle_device_free", "eagle_device_upload", "eagle_host_alloc", "eagle_host_free", "eagle_reproject", "eagle_comm_id", "eagle_comm_init", "eagle_gather",
           "eagle_set_profiling", "eagle_get_timings", "eagle_get_kernel_times", "eagle_op_conv2d", "eagle_op_bottleneck", "eagle_op_stem", "eagle_op_fuse_sum", "eagle_op_preprocess", "eagle_op_preprocess_lb",
           "eagle_op_find_homography", "eagle_op_detect_tail", "eagle_op_post", "eagle_op_conv2d_argmax", "eagle_op_conv_config", "eagle_op_conv_table", "eagle_clip_open", "eagle_clip_close", "eagle_clip_detect_objects", "eagle_clip_detect_keypoints", "eagle_clip_get_keypoints",
           "eagle_clip_set_keypoints", "eagle_clip_flow", "eagle_clip_run", "eagle_clip_fetch", "eagle_debug", "eagle_track_open", "eagle_track_frames", "eagle_track_frames_cmc", "eagle_clip_motion_ecc", "eagle_clip_motion", "eagle_team_colors",
           "eagle_reid_features", "eagle_track_frames_reid", "eagle_process_frames_yuv", "eagle_process_device_frames_yuv", "eagle_yuv_to_bgr",
           "eagle_op_yuv_to_bgr", "eagle_annotate_device_frames", "eagle_annotate_frames", "eagle_overlay_from_record", "eagle_op_annotate",
           "eagle_annotate_frames_prims", "eagle_postprocess", "eagle_post_free", "eagle_post_shape", "eagle_post_layout", "eagle_post_values",
           "eagle_post_device_values", "eagle_post_merges", "eagle_overlay_from_table", "eagle_minimap_size", "eagle_minimap_device_frames", "eagle_minimap_frames",
           "eagle_op_minimap", "eagle_post_velocities", "eagle_post_velocity_values", "eagle_post_device_velocity_values", "eagle_control_size",
           "eagle_control_device_grids", "eagle_control_grids", "eagle_minimap_set_control", "eagle_op_velocities", "eagle_op_control",
           "eagle_op_minimap_control", "eagle_post_possession", "eagle_post_possession_values", "eagle_post_device_possession", "eagle_post_events",
           "eagle_op_possession", "eagle_pass_options_size", "eagle_pass_options_layout", "eagle_pass_options_device", "eagle_pass_options",
           "eagle_op_pass_options", "eagle_occupancy_size", "eagle_post_occupancy", "eagle_post_occupancy_values", "eagle_post_device_occupancy",
           "eagle_occupancy_picture", "eagle_op_occupancy", "eagle_op_occupancy_picture", "eagle_minimap_set_trails", "eagle_trajectory_picture",
           "eagle_pass_picture", "eagle_op_minimap_trails", "eagle_op_trajectory_picture", "eagle_op_pass_picture", "eagle_post_team_shape", "eagle_post_team_shape_values",
           "eagle_post_device_team_shape", "eagle_minimap_set_hulls", "eagle_op_team_shape", "eagle_op_minimap_hulls", "eagle_post_physical", "eagle_post_physical_values",
           "eagle_post_physical_totals", "eagle_post_physical_efforts", "eagle_post_device_physical", "eagle_op_physical", "eagle_post_roles",
           "eagle_post_roles_values", "eagle_post_device_roles", "eagle_op_roles", "eagle_post_space", "eagle_post_space_values", "eagle_post_device_space",
           "eagle_space_device_grids", "eagle_space_grids", "eagle_op_space", "eagle_post_offside", "eagle_post_offside_values", "eagle_post_offside_events",
           "eagle_post_device_offside", "eagle_op_offside", "eagle_ball_track", "eagle_ball_track_values", "eagle_ball_track_tracklets", "eagle_ball_track_free",
           "eagle_op_ball_track", "eagle_postprocess_ball", "eagle_kit_params_default", "eagle_team_cluster", "eagle_op_team_cluster", "eagle_op_team_cluster_ids",
           "eagle_shots_device_frames", "eagle_shots_frames", "eagle_op_shots", "eagle_topview_size", "eagle_topview_device_frames", "eagle_topview_frames",
           "eagle_topview_mosaic_device", "eagle_topview_mosaic_finish", "eagle_topview_residual_device", "eagle_topview_mosaic_frames", "eagle_topview_residual_frames",
           "eagle_op_topview", "eagle_ground_device_frames", "eagle_ground_frames", "eagle_op_ground", "eagle_op_reid_crop", "eagle_op_reid_conv7", "eagle_op_reid_maxpool3s2", "eagle_op_reid_avgpool2", "eagle_op_reid_dw3",
           "eagle_op_reid_gate", "eagle_op_reid_head", "eagle_op_conv2d_sliced", "eagle_op_maxpool5", "eagle_op_upsample2", "eagle_op_split_to_f32", "eagle_op_gray_pyramid",
           "eagle_op_flow", "eagle_op_ecc_small", "eagle_op_ecc", "eagle_post_smooth_tracks", "eagle_post_smooth_values", "eagle_post_device_smooth",
           "eagle_post_raw_values", "eagle_op_smooth_tracks", "eagle_post_stabilise", "eagle_post_stabilise_values", "eagle_post_original_values",
           "eagle_post_device_stabilise", "eagle_op_stabilise", "eagle_linefit_params_default", "eagle_linefit_device_frames", "eagle_linefit_frames",
           "eagle_op_linefit", "eagle_flight_params_default", "eagle_post_ball_flights", "eagle_post_ball_flight_values", "eagle_post_ball_flight_records",
           "eagle_post_ball_kicks", "eagle_post_device_ball_flights", "eagle_op_ball_flights", "eagle_goal_view_params_default", "eagle_post_goal_view",
           "eagle_post_goal_view_values", "eagle_post_device_goal_view", "eagle_op_goal_view"]

FLOWKP_DTYPE = np.dtype([("label", "<i4"), ("x", "<i4"), ("y", "<i4"), ("score", "<f4")], align=True)
ECC_DTYPE = np.dtype([("ok", "<i4"), ("iters", "<i4"), ("rho", "<f8"), ("M", "<f4", (6,))], align=True)      # EagleEccResult
E_REFERENCE_RAISES = -7
E_RANGE = -8


def debug(key, value=0, out=None):
    """Developer diagnostics (include/eagle.h, eagle_debug)."""
    rc = load().eagle_debug(key.encode(), int(value), None if out is None else out.ctypes.data_as(C.c_void_p), 0 if out is None else out.nbytes)
    if rc:
        raise EagleError(f"eagle_debug({key}) failed ({rc})")
    return out


def resolve_config(cfg):
    """A copy of cfg with the "auto" fields resolved the way eagle_create will (no GPU needed)."""
    out = EagleConfig.from_buffer_copy(cfg)
    rc = load().eagle_resolve_config(C.byref(out))
    if rc:
        raise EagleError(f"eagle_resolve_config failed ({rc}): {load().eagle_last_error(None).decode()}")
    return out


def abi_sizes():
    o = (C.c_int32 * 4)()
    load().eagle_abi_sizes(o)
    return list(o)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def default_config(**kw):
    """eagle_default_config + overrides: a thin pass-through.  The library's default ``det_precision`` is EAGLE_DET_PREC_AUTO (-1), which
    eagle_create resolves from ``precision``: the exact fp32 family next to split-family key-points, otherwise the key-point family
    (``Handle.cfg`` holds the resolved value)."""
    cfg = EagleConfig()
    load().eagle_default_config(C.byref(cfg))
    for k, v in kw.items():
        if k == "det_variant" and isinstance(v, str):
            v = DET_VARIANTS[v]
        if k == "letterbox" and isinstance(v, str):
            v = LETTERBOX[v]
        if not hasattr(cfg, k):
            raise TypeError(f"unknown config field {k}")
        setattr(cfg, k, v)
    return cfg


class Handle:
    """One library handle == one GPU worker (not thread-safe)."""

    def __init__(self, cfg=None, **kw):
        self.L = load()
        self.cfg = cfg or default_config(**kw)
        self._h = C.c_void_p()
        rc = self.L.eagle_create(C.byref(self.cfg), C.byref(self._h))
        if rc:
            raise EagleError(f"eagle_create failed ({rc}): {self.L.eagle_last_error(None).decode()}")
        resolved = EagleConfig()
        self._check(self.L.eagle_get_config(self._h, C.byref(resolved)), "get_config")
        self.cfg = resolved                                 # det_precision as the library resolved it (EAGLE_DET_PREC_AUTO -> a family)

    def _check(self, rc, what):
        if rc == E_RANGE:
            raise EagleRangeError(f"{what}: {self.L.eagle_last_error(self._h).decode()}")
        if rc:
            raise EagleError(f"{what} failed ({rc}): {self.L.eagle_last_error(self._h).decode()}")

    def _check_records(self, rc, what, out):
        try:
            self._check(rc, what)
        except EagleRangeError as e:
            e.records = out
            raise

    def close(self):
        if self._h:
            self.L.eagle_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_weight(self, name, arr):
        arr = np.ascontiguousarray(arr, np.float32)
        shape = (C.c_int64 * max(arr.ndim, 1))(*arr.shape)
        self._check(self.L.eagle_load_weights(self._h, name.encode(), _fp(arr), shape, arr.ndim), f"load_weights({name})")

    def finalize_weights(self):
        self._check(self.L.eagle_finalize_weights(self._h), "finalize_weights")

    def process(self, frames, out=None, strides=None):
        """frames: uint8 [n,h,w,3] BGR (host).  -> structured array [n] of RESULT_DTYPE (``out``: optional preallocated result array).

        The array is handed over AS THE VIEW IT IS (cm.py:568 passes whatever view the caller holds): a crop of a wider surface or a decoder's
        padded plane goes to eagle_process_frames with its own frame / row strides, no host-side copy.  Only views whose pixels are not packed
        BGR triples, whose strides are negative or whose frames overlap are made contiguous first.  ``strides=(frame_stride, row_stride)`` in
        bytes overrides what is passed (tests of the boundary's argument checks)."""
        frames = np.asarray(frames)
        if frames.dtype != np.uint8:
            frames = frames.astype(np.uint8)
        if frames.ndim == 3:
            frames = frames[None]
        n, h, w, c = frames.shape
        if (h, w, c) != (self.cfg.frame_h, self.cfg.frame_w, 3):
            raise EagleError(f"frame shape {(h, w, c)} does not match the handle ({self.cfg.frame_h}, {self.cfg.frame_w}, 3)")
        fs, rs, ps, cs = frames.strides
        if n == 1:
            fs = max(fs, rs * (h - 1) + 3 * w)              # numpy reports any stride for a length-1 axis
        if not (cs == 1 and ps == 3 and rs >= 3 * w and fs >= rs * (h - 1) + 3 * w):
            frames = np.ascontiguousarray(frames)
            fs, rs = h * w * 3, w * 3
        if strides is not None:
            fs, rs = strides
        if out is None:
            out = np.zeros(n, RESULT_DTYPE)
        assert out.dtype == RESULT_DTYPE and len(out) >= n and out.flags.c_contiguous
        self._check_records(self.L.eagle_process_frames(self._h, C.cast(frames.ctypes.data, C.POINTER(C.c_uint8)), n, int(fs), int(rs),
                                                        out.ctypes.data_as(C.c_void_p)), "process_frames", out)
        return out

    def host_frames(self, n):
        """uint8 [n,h,w,3] array in pinned host memory (eagle_host_alloc): what a decoder should write frames into so that
        eagle_process_frames can DMA them in place.  Release with host_free(array)."""
        shape = (n, self.cfg.frame_h, self.cfg.frame_w, 3)
        nbytes = int(np.prod(shape))
        p = C.c_void_p()
        self._check(self.L.eagle_host_alloc(self._h, nbytes, C.byref(p)), "host_alloc")
        buf = (C.c_uint8 * max(nbytes, 1)).from_address(p.value)
        a = np.frombuffer(buf, np.uint8, nbytes).reshape(shape)
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p
        return a

    def host_buffer(self, nbytes):
        """uint8 [nbytes] in pinned host memory (eagle_host_alloc) for callers that lay frames out themselves (row / frame pitch).  host_free(array)."""
        p = C.c_void_p()
        self._check(self.L.eagle_host_alloc(self._h, int(nbytes), C.byref(p)), "host_alloc")
        a = np.frombuffer((C.c_uint8 * max(int(nbytes), 1)).from_address(p.value), np.uint8, int(nbytes))
        self._pinned = getattr(self, "_pinned", {})
        self._pinned[a.ctypes.data] = p
        return a

    def host_free(self, a):
        p = self._pinned.pop(a.ctypes.data)
        self._check(self.L.eagle_host_free(self._h, p), "host_free")

    def upload(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        d = C.c_void_p()
        self._check(self.L.eagle_device_alloc(self._h, frames.nbytes, C.byref(d)), "device_alloc")
        self._check(self.L.eagle_device_upload(self._h, d, frames.ctypes.data_as(C.c_void_p), frames.nbytes), "device_upload")
        return d

    def free(self, d):
        self._check(self.L.eagle_device_free(self._h, d), "device_free")

    def process_device(self, dptr, n, out=None):
        if out is None:
            out = np.zeros(n, RESULT_DTYPE)
        self._check_records(self.L.eagle_process_device_frames(self._h, dptr, n, out.ctypes.data_as(C.c_void_p)), "process_device_frames", out)
        return out

    # --- decoder-native input: 4:2:0 frames (include/eagle.h, eagle_*_yuv) ---------------------------------
    def _yuv_frames(self, frames, fmt, layout, n):
        """-> (uint8 array the library reads, frame count, EagleYuvLayout or None).  [n, 3h/2, w] / [3h/2, w] is the cv2 / numpy convention
        (dense); a flat buffer (a decoder's surface, e.g. host_buffer()) needs its layout and n."""
        h, w = self.cfg.frame_h, self.cfg.frame_w
        a = np.asarray(frames)
        if a.dtype != np.uint8:
            raise EagleError(f"4:2:0 frames must be uint8 (got {a.dtype})")
        if a.ndim in (2, 3):
            if a.ndim == 2:
                a = a[None]
            if a.shape[1:] != (h * 3 // 2, w):
                raise EagleError(f"4:2:0 frame shape {a.shape[1:]} does not match the handle ({h * 3 // 2}, {w})")
            if n is not None and n != len(a):
                raise EagleError(f"n = {n} but {len(a)} frames were given")
            a, n = np.ascontiguousarray(a), len(a)
        elif a.ndim == 1:
            if layout is None or n is None:
                raise EagleError("a flat 4:2:0 buffer needs an explicit layout and frame count n")
            a = np.ascontiguousarray(a)
            need = yuv_span(fmt, h, w, layout, n)
            if a.nbytes < need:
                raise EagleError(f"the buffer holds {a.nbytes} bytes, {n} frames of this layout span {need}")
        else:
            raise EagleError(f"4:2:0 frames: [n, 3h/2, w], [3h/2, w] or a flat buffer (got shape {a.shape})")
        return a, n, _yuv_layout(layout)

    def process_yuv(self, frames, fmt="nv12", layout=None, out=None, n=None):
        """NV12 / I420 frames (host memory) -> records equal to process() of the BGR frames cv2.cvtColor(yuv, COLOR_YUV2BGR_NV12 / _I420) gives.
        ``frames``: uint8 [n, 3h/2, w] or [3h/2, w] (cv2 / numpy convention), or a flat buffer such as host_buffer() filled by a decoder together
        with ``layout`` (dict or EagleYuvLayout: frame_stride, y_pitch, c_offset, c_pitch, v_offset in bytes, 0 = dense default) and ``n``."""
        a, n, lay = self._yuv_frames(frames, fmt, layout, n)
        if out is None:
            out = np.zeros(n, RESULT_DTYPE)
        assert out.dtype == RESULT_DTYPE and len(out) >= n and out.flags.c_contiguous
        self._check_records(self.L.eagle_process_frames_yuv(self._h, _pix(fmt), C.cast(a.ctypes.data, C.POINTER(C.c_uint8)), n,
                                                            None if lay is None else C.byref(lay), out.ctypes.data_as(C.c_void_p)), "process_frames_yuv", out)
        return out

    def process_device_yuv(self, dptr, n, fmt="nv12", layout=None, out=None):
        """NV12 / I420 frames resident in HBM (read in place with their layout) -> records, as process_yuv."""
        if out is None:
            out = np.zeros(n, RESULT_DTYPE)
        assert out.dtype == RESULT_DTYPE and len(out) >= n and out.flags.c_contiguous
        lay = _yuv_layout(layout)
        self._check_records(self.L.eagle_process_device_frames_yuv(self._h, _pix(fmt), dptr, n, None if lay is None else C.byref(lay),
                                                                   out.ctypes.data_as(C.c_void_p)), "process_device_frames_yuv", out)
        return out

    def yuv_to_bgr_device(self, d_src, n, fmt="nv12", layout=None):
        """n NV12 / I420 frames in HBM -> a new dense BGR [n, h, w, 3] device buffer (free it with free()): the clip the entries that take
        resident BGR frames read (clip_open, reid_features, team_colors)."""
        d = C.c_void_p()
        self._check(self.L.eagle_device_alloc(self._h, max(n, 1) * self.cfg.frame_h * self.cfg.frame_w * 3, C.byref(d)), "device_alloc")
        lay = _yuv_layout(layout)
        try:
            self._check(self.L.eagle_yuv_to_bgr(self._h, _pix(fmt), d_src, n, None if lay is None else C.byref(lay), d), "yuv_to_bgr")
        except EagleError:
            self.free(d)
            raise
        return d

    def upload_bgr(self, frames, pixel_format="bgr"):
        """Frames (host) -> a dense BGR device clip (free it with free()): uploaded as they are for "bgr", converted on the GPU from "nv12" / "i420"
        ([n, 3h/2, w]) otherwise."""
        if pixel_format == "bgr":
            return self.upload(frames)
        a, n, _ = self._yuv_frames(frames, pixel_format, None, None)
        d = self.upload(a)
        try:
            return self.yuv_to_bgr_device(d, n, pixel_format)
        finally:
            self.free(d)

    # --- shots: cuts, transitions and flashes of a clip (include/eagle.h, eagle_shots_*) ---------------------------------------------
    def shots_device(self, dptr, n, params=None, cap=None, **kw):
        """n dense BGR frames of the handle's size resident in HBM -> (frames [n] of SHOT_FRAME_DTYPE, shots [m] of SHOT_DTYPE).  params: an
        EagleShotParams, or keywords for shot_params(...) (cut, low, grass_thr in 1 / 65536; window, min_len in frames; fps picks the defaults)."""
        p = shot_params(**kw) if params is None else params
        n = int(n)
        rows, shots, m = _shot_outputs(n, cap)
        self._check(self.L.eagle_shots_device_frames(self._h, dptr, n, C.byref(p), rows.ctypes.data_as(C.c_void_p), shots.ctypes.data_as(C.c_void_p), len(shots),
                                                     C.byref(m)), "shots_device_frames")
        return rows, shots[:m.value].copy()

    def shots(self, frames, params=None, cap=None, max_staging_bytes=0, strides=None, **kw):
        """frames: uint8 [n, h, w, 3] BGR in host memory, handed over as the view it is (process() has the rules), uploaded in passes of
        ``max_staging_bytes`` (0: 64 MB) -> (frames, shots) as shots_device."""
        p = shot_params(**kw) if params is None else params
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 4 or frames.shape[1:] != (self.cfg.frame_h, self.cfg.frame_w, 3):
            raise EagleError(f"shots: frames must be uint8 [n, {self.cfg.frame_h}, {self.cfg.frame_w}, 3] (got {frames.dtype} {frames.shape})")
        n, h, w, _ = frames.shape
        fs, rs, ps, cs = frames.strides
        if n == 1:
            fs = max(fs, rs * (h - 1) + 3 * w)
        if not (cs == 1 and ps == 3 and rs >= 3 * w and fs >= rs * (h - 1) + 3 * w):
            frames = np.ascontiguousarray(frames)
            fs, rs = h * w * 3, w * 3
        if strides is not None:
            fs, rs = strides
        rows, shots, m = _shot_outputs(n, cap)
        self._check(self.L.eagle_shots_frames(self._h, C.c_void_p(frames.ctypes.data), n, int(rs), int(fs), int(max_staging_bytes), C.byref(p),
                                              rows.ctypes.data_as(C.c_void_p), shots.ctypes.data_as(C.c_void_p), len(shots), C.byref(m)), "shots_frames")
        return rows, shots[:m.value].copy()

    # --- top view: the frames on the pitch plane, their mosaic and residuals (include/eagle.h, eagle_topview_*) -------------------------
    def device_alloc(self, nbytes):
        d = C.c_void_p()
        self._check(self.L.eagle_device_alloc(self._h, int(nbytes), C.byref(d)), "device_alloc")
        return d

    def _topview_clip(self, what, frames, Hs, valid, n=None):
        """-> (frames or None, n, Hs float64 [n, 9], valid uint8 [n]); frames None: a device clip of n frames"""
        if frames is not None:
            frames = np.ascontiguousarray(frames, np.uint8)
            if frames.ndim != 4 or frames.shape[1:] != (self.cfg.frame_h, self.cfg.frame_w, 3):
                raise EagleError(f"{what}: frames must be uint8 [n, {self.cfg.frame_h}, {self.cfg.frame_w}, 3] (got {frames.shape})")
            n = len(frames)
        return (frames, int(n)) + _topview_maps(what, Hs, valid, int(n))

    def topview_device(self, d_bgr, n, Hs, valid, params, d_out, fmt="bgr", layout=None):
        """n dense BGR frames resident in HBM + their homographies -> n warped frames at ``d_out`` (device) in ``fmt`` / ``layout``."""
        _, n, Hs, valid = self._topview_clip("topview_device", None, Hs, valid, n)
        lay = _yuv_layout(layout)
        keep = np.zeros(16, np.uint8)
        self._check(self.L.eagle_topview_device_frames(self._h, d_bgr, n, _ptr(Hs, keep), _ptr(valid, keep), C.byref(params), _out_pix(fmt),
                                                       None if lay is None else C.byref(lay), d_out), "topview_device_frames")

    def topview(self, frames, Hs, valid, params, fmt="bgr", layout=None, out=None):
        """frames uint8 [n, h, w, 3] (host) -> the warped frames in host memory: uint8 [n, Hc, W, 3] ("bgr") or [n, 3 Hc / 2, W] ("nv12" / "i420") with
        (W, Hc) = topview_size(params); with a ``layout`` a flat uint8 buffer of the layout's span (``out``: the caller's buffer)."""
        frames, n, Hs, valid = self._topview_clip("topview", frames, Hs, valid)
        w, h = topview_size(params)
        lay = _yuv_layout(layout)
        need = out_span(fmt, h, w, lay, n)
        if out is None:
            out = np.zeros(need, np.uint8)
            if lay is None:
                out = out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
        if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
            raise EagleError(f"topview: out must be a contiguous uint8 array of at least {need} bytes")
        keep = np.zeros(16, np.uint8)
        self._check(self.L.eagle_topview_frames(self._h, _ptr(frames, keep), n, _ptr(Hs, keep), _ptr(valid, keep), C.byref(params), _out_pix(fmt),
                                                None if lay is None else C.byref(lay), _ptr(out, keep)), "topview_frames")
        return out

    def topview_accumulator(self, params):
        """A device accumulator u32 [Hc][W][4] for these parameters (free it with free()); the first mosaic call zeroes it (reset=True)."""
        w, h = topview_size(params)
        return self.device_alloc(w * h * 16)

    def topview_mosaic_add(self, frames, Hs, valid, params, d_acc, recs=None, reset=True, n=None, max_staging_bytes=0):
        """Adds the frames first, first + step, ... to ``d_acc``.  frames: uint8 [n, h, w, 3] in host memory (uploaded in passes of ``max_staging_bytes``)
        or a device pointer with ``n``.  recs: the records, needed with params.mask_boxes."""
        dev, d_bgr = isinstance(frames, C.c_void_p), frames
        frames, n, Hs, valid = self._topview_clip("topview_mosaic_add", None if dev else frames, Hs, valid, n)
        recs = _topview_recs(recs, n)
        keep = np.zeros(16, np.uint8)
        if dev:
            rc = self.L.eagle_topview_mosaic_device(self._h, d_bgr, n, _ptr(Hs, keep), _ptr(valid, keep), _ptr(recs, keep), C.byref(params), d_acc, int(bool(reset)))
        else:
            rc = self.L.eagle_topview_mosaic_frames(self._h, _ptr(frames, keep), n, int(max_staging_bytes), _ptr(Hs, keep), _ptr(valid, keep), _ptr(recs, keep), C.byref(params),
                                                    d_acc, int(bool(reset)))
        self._check(rc, "topview_mosaic")

    def topview_mosaic_finish(self, d_acc, params):
        """-> (mosaic uint8 [Hc, W, 3], cnt uint32 [Hc, W])"""
        w, h = topview_size(params)
        pic, cnt = np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint32)
        self._check(self.L.eagle_topview_mosaic_finish(self._h, d_acc, C.byref(params), pic.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)), "topview_mosaic_finish")
        return pic, cnt

    def topview_residuals(self, frames, Hs, valid, params, d_acc, recs=None, n=None, max_staging_bytes=0):
        """The residual triples of every frame against the finished accumulator -> (res_sum uint64 [n], res_cnt uint32 [n], covered uint32 [n]);
        frames as topview_mosaic_add takes them."""
        dev, d_bgr = isinstance(frames, C.c_void_p), frames
        frames, n, Hs, valid = self._topview_clip("topview_residuals", None if dev else frames, Hs, valid, n)
        recs = _topview_recs(recs, n)
        rs, rc_, cv = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        keep = np.zeros(16, np.uint8)
        if dev:
            rc = self.L.eagle_topview_residual_device(self._h, d_bgr, n,_ptr(Hs, keep), _ptr(valid, keep), _ptr(recs, keep), C.byref(params), d_acc, _ptr(rs, keep),
                                                      _ptr(rc_, keep), _ptr(cv, keep))
        else:
            rc = self.L.eagle_topview_residual_frames(self._h, _ptr(frames, keep), n, int(max_staging_bytes), _ptr(Hs, keep), _ptr(valid, keep), _ptr(recs, keep),
                                                      C.byref(params), d_acc, _ptr(rs, keep), _ptr(rc_, keep), _ptr(cv, keep))
        self._check(rc, "topview_residual")
        return rs, rc_, cv

    # --- ground layer: shapes on the pitch plane blended into the camera picture (include/eagle.h, eagle_ground_*) ----------------------
    def ground_device(self, d_bgr, n, Hs, valid, shapes, off, d_out, params=None, fmt="bgr", layout=None):
        """n dense BGR frames resident in HBM + their homographies + the shapes of each (GROUND_SHAPE_DTYPE [off[n]], off [n + 1]) -> n pictures
        at ``d_out`` (device, another buffer) in ``fmt`` / ``layout``; returns covered uint32 [n]."""
        _, n, Hs, valid = self._topview_clip("ground_device", None, Hs, valid, n)
        shapes, off = _ground_lists("ground_device", shapes, off, n)
        p = ground_params() if params is None else params
        lay = _yuv_layout(layout)
        cov = np.zeros(n, np.uint32)
        keep = np.zeros(16, np.uint8)
        self._check(self.L.eagle_ground_device_frames(self._h, d_bgr, n, _ptr(Hs, keep), _ptr(valid, keep), _ptr(shapes, keep), _ptr(off, keep), C.byref(p), _out_pix(fmt),
                                                      None if lay is None else C.byref(lay), d_out, _ptr(cov, keep)), "ground_device_frames")
        return cov

    def ground(self, frames, Hs, valid, shapes, off, params=None, fmt="bgr", layout=None, out=None, max_staging_bytes=0):
        """frames uint8 [n, h, w, 3] (host) -> (the pictures in host memory: uint8 [n, h, w, 3] ("bgr") or [n, 3h / 2, w] ("nv12" / "i420"), with a
        ``layout`` a flat uint8 buffer of the layout's span (``out``: the caller's buffer); covered uint32 [n]).  Uploaded in passes of
        ``max_staging_bytes`` (0: 64 MB)."""
        frames, n, Hs, valid = self._topview_clip("ground", frames, Hs, valid)
        shapes, off = _ground_lists("ground", shapes, off, n)
        p = ground_params() if params is None else params
        h, w = self.cfg.frame_h, self.cfg.frame_w
        lay = _yuv_layout(layout)
        need = out_span(fmt, h, w, lay, n)
        if out is None:
            out = np.zeros(need, np.uint8)
            if lay is None:
                out = out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
        if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
            raise EagleError(f"ground: out must be a contiguous uint8 array of at least {need} bytes")
        cov = np.zeros(n, np.uint32)
        keep = np.zeros(16, np.uint8)
        self._check(self.L.eagle_ground_frames(self._h, _ptr(frames, keep), n, int(max_staging_bytes), _ptr(Hs, keep), _ptr(valid, keep), _ptr(shapes, keep), _ptr(off, keep),
                                               C.byref(p), _out_pix(fmt), None if lay is None else C.byref(lay), _ptr(out, keep), _ptr(cov, keep)), "ground_frames")
        return out, cov

    # --- line registration: each frame's homography refined on the painted lines (include/eagle.h, eagle_linefit_*) ---------------------
    def linefit_device(self, d_bgr, n, Hs, valid, recs=None, params=None, masks=False):
        """n dense BGR frames resident in HBM + their homographies (+ the records, whose detections are the boxes) -> (Hs_out float64 [n, 9], frames
        LINEFIT_FRAME_DTYPE [n], masks uint32 [n, h, (w + 31) // 32] or None)."""
        return self._linefit("linefit_device", None, d_bgr, n, Hs, valid, recs, params, masks, 0)

    def linefit(self, frames, Hs, valid, recs=None, params=None, masks=False, max_staging_bytes=0):
        """Same for frames uint8 [n, h, w, 3] in host memory, uploaded in passes of ``max_staging_bytes`` (0: 64 MB)."""
        return self._linefit("linefit", frames, None, None, Hs, valid, recs, params, masks, max_staging_bytes)

    def _linefit(self, what, frames, d_bgr, n, Hs, valid, recs, params, masks, max_staging_bytes):
        frames, n, Hs, valid = self._topview_clip(what, frames, Hs, valid, n)
        recs = _topview_recs(recs, n)
        p = linefit_params() if params is None else params
        out, fr = np.zeros((n, 9), np.float64), np.zeros(n, LINEFIT_FRAME_DTYPE)
        mk = np.zeros((n, self.cfg.frame_h, (self.cfg.frame_w + 31) // 32), np.uint32) if masks else None
        keep = np.zeros(16, np.uint8)
        if frames is None:
            rc = self.L.eagle_linefit_device_frames(self._h, d_bgr, n, _ptr(Hs, keep), _ptr(valid, keep), _ptr(recs, keep), C.byref(p), _ptr(out, keep), _ptr(fr, keep),
                                                    _ptr(mk, keep))
        else:
            rc = self.L.eagle_linefit_frames(self._h, _ptr(frames, keep), n, int(max_staging_bytes), _ptr(Hs, keep), _ptr(valid, keep), _ptr(recs, keep), C.byref(p),
                                             _ptr(out, keep), _ptr(fr, keep), _ptr(mk, keep))
        self._check(rc, what)
        return out, fr, mk

    # --- annotated output (include/eagle.h, eagle_annotate_*) --------------------------------------------------
    def annotate_device(self, d_bgr, n, recs, d_out, team_mapping=None, fmt="bgr", layout=None):
        """n frames of a dense BGR clip resident in HBM + their records -> n annotated frames at ``d_out`` (device: free()-able memory of this
        handle or an encoder's surface) as "bgr", "nv12" or "i420" in ``layout`` (dict or EagleYuvLayout, None = dense).  team_mapping:
        {player id: 0 | 1} (Processor.get_team_mapping) or None (every player in a neutral colour)."""
        recs, ids, vals, nt = _annot_args(recs, n, team_mapping)
        lay = _yuv_layout(layout)
        self._check(self.L.eagle_annotate_device_frames(self._h, d_bgr, n, recs.ctypes.data_as(C.c_void_p), None if ids is None else ids.ctypes.data_as(C.c_void_p),
                                                        None if vals is None else vals.ctypes.data_as(C.c_void_p), nt, _out_pix(fmt),
                                                        None if lay is None else C.byref(lay), d_out), "annotate_device_frames")

    def annotate(self, d_bgr, n, recs, team_mapping=None, fmt="bgr", layout=None, out=None):
        """As annotate_device, the result in host memory: uint8 [n, h, w, 3] ("bgr") or [n, 3h/2, w] ("nv12" / "i420"); with a ``layout`` a flat
        uint8 buffer of the layout's span (``out``: the caller's buffer, e.g. host_buffer(); bytes the layout does not cover are left alone)."""
        h, w = self.cfg.frame_h, self.cfg.frame_w
        recs, ids, vals, nt = _annot_args(recs, n, team_mapping)
        lay = _yuv_layout(layout)
        need = out_span(fmt, h, w, lay, n)
        if out is None:
            out = np.zeros(need, np.uint8)
            if lay is None:
                out = out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
        if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
            raise EagleError(f"annotate: out must be a contiguous uint8 array of at least {need} bytes")
        self._check(self.L.eagle_annotate_frames(self._h, d_bgr, n, recs.ctypes.data_as(C.c_void_p), None if ids is None else ids.ctypes.data_as(C.c_void_p),
                                                 None if vals is None else vals.ctypes.data_as(C.c_void_p), nt, _out_pix(fmt),
                                                 None if lay is None else C.byref(lay), out.ctypes.data_as(C.c_void_p)), "annotate_frames")
        return out

    def annotate_prims(self, d_bgr, n, prims, offsets, fmt="bgr", layout=None, out=None):
        """As annotate, drawing the caller's primitive lists (PRIM_DTYPE array + n + 1 offsets) instead of the records' (eagle_annotate_frames_prims)."""
        h, w = self.cfg.frame_h, self.cfg.frame_w
        prims = np.ascontiguousarray(prims, PRIM_DTYPE)
        offsets = np.ascontiguousarray(offsets, np.int32)
        if len(offsets) != n + 1 or (n and int(offsets[-1]) > len(prims)):
            raise EagleError("annotate_prims: offsets must have n + 1 entries inside the primitive array")
        lay = _yuv_layout(layout)
        need = out_span(fmt, h, w, lay, n)
        if out is None:
            out = np.zeros(need, np.uint8)
            if lay is None:
                out = out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
        if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
            raise EagleError(f"annotate_prims: out must be a contiguous uint8 array of at least {need} bytes")
        self._check(self.L.eagle_annotate_frames_prims(self._h, d_bgr, n, prims.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), _out_pix(fmt),
                                                       None if lay is None else C.byref(lay), out.ctypes.data_as(C.c_void_p)), "annotate_frames_prims")
        return out

    # --- the clip post-processor (include/eagle.h, eagle_postprocess) -------------------------------------------
    def postprocess(self, recs, fps, frame_w, team_mapping=None, smooth=False, filter_ball=False, max_bytes=0, merge_ids=False, ball_det=None):
        """The records of a finished clip -> a PostTable (the reference's Processor.process_data table, built on the GPU and resident there).
        merge_ids: stitch the fragments of one person under several tracker ids into one column (include/eagle.h; False, 0: the reference as written,
        which never merges); the table's ``merges`` list what was joined and its ``team_mapping`` gains the teams the heads inherit.
        ball_det: per record -1 or the index of the one reported ball detection that counts (ball_track's ``det``; include/eagle.h,
        eagle_postprocess_ball); None: the reference's choice."""
        recs = np.ascontiguousarray(recs, RESULT_DTYPE).reshape(-1)
        ids, vals, nt = _team_arrays(team_mapping)
        p = EaglePostParams(int(fps), int(frame_w), int(bool(smooth)), int(filter_ball), None if ids is None else ids.ctypes.data, None if vals is None else vals.ctypes.data,
                            nt, int(merge_ids), int(max_bytes))                 # (the struct's ``reserved`` field carries merge_ids)
        t = C.c_void_p()
        if ball_det is None:
            self._check(self.L.eagle_postprocess(self._h, recs.ctypes.data_as(C.c_void_p), len(recs), C.byref(p), C.byref(t)), "postprocess")
        else:
            ball_det = np.ascontiguousarray(ball_det, np.int32).reshape(-1)
            if len(ball_det) != len(recs):
                raise ValueError(f"ball_det has {len(ball_det)} entries for {len(recs)} records")
            self._check(self.L.eagle_postprocess_ball(self._h, recs.ctypes.data_as(C.c_void_p), len(recs), C.byref(p), ball_det.ctypes.data_as(C.c_void_p), C.byref(t)),
                        "postprocess_ball")
        return PostTable(self, t, team_mapping)

    # --- the ball track (include/eagle.h, eagle_ball_track) ---------------------------------------------------------------------
    def ball_track(self, recs, params, cuts=None):
        """Which reported ball detection of every record lies on the best path through the clip -> (BALL_FRAME_DTYPE [n], BALL_TRACKLET_DTYPE [tracklets],
        BALL_CLIP_DTYPE [1]); params ball_track_params(...), cuts the sorted frames that start a new shot.  ``frames["det"]`` is postprocess's ball_det."""
        recs = np.ascontiguousarray(recs, RESULT_DTYPE).reshape(-1)
        cuts = np.zeros(0, np.int32) if cuts is None else np.ascontiguousarray(cuts, np.int32).reshape(-1)
        t = C.c_void_p()
        self._check(self.L.eagle_ball_track(self._h, recs.ctypes.data_as(C.c_void_p), len(recs), cuts.ctypes.data_as(C.c_void_p) if len(cuts) else None, len(cuts),
                                            C.byref(params), C.byref(t)), "ball_track")
        try:
            frames, clip, n = np.zeros(len(recs), BALL_FRAME_DTYPE), np.zeros(1, BALL_CLIP_DTYPE), C.c_int(0)
            keep = np.zeros(4, np.float64)
            self._check(self.L.eagle_ball_track_values(t, _ptr(frames, keep), _ptr(clip, keep)), "ball_track_values")
            self._check(self.L.eagle_ball_track_tracklets(t, None, 0, C.byref(n)), "ball_track_tracklets")
            tracklets = np.zeros(n.value, BALL_TRACKLET_DTYPE)
            self._check(self.L.eagle_ball_track_tracklets(t, _ptr(tracklets, keep), n.value, C.byref(n)), "ball_track_tracklets")
        finally:
            self.L.eagle_ball_track_free(t)
        return frames, tracklets, clip

    # --- the minimap (include/eagle.h, eagle_minimap_*) ------------------------------------------------------------
    def minimap_device(self, table, d_out, params, row0=0, n=None, fmt="bgr", layout=None):
        """Rows row0 .. row0 + n - 1 of a PostTable of this handle -> n minimap pictures at ``d_out`` (device memory of this handle or an encoder's
        surface) as "bgr", "nv12" or "i420" in ``layout`` (None = dense).  params: EagleMinimapParams (minimap_params)."""
        n = len(table.rows) - row0 if n is None else n
        lay = _yuv_layout(layout)
        self._check(self.L.eagle_minimap_device_frames(self._h, table._t, int(row0), int(n), C.byref(params), _out_pix(fmt), None if lay is None else C.byref(lay), d_out),
                    "minimap_device_frames")

    def minimap(self, table, params, row0=0, n=None, fmt="bgr", layout=None, out=None):
        """As minimap_device, the result in host memory: uint8 [n, h, w, 3] ("bgr") or [n, 3h/2, w] ("nv12" / "i420") with (w, h) = minimap_size(params);
        with a ``layout`` a flat uint8 buffer of the layout's span (``out``: the caller's buffer; bytes the layout does not cover are left alone)."""
        n = len(table.rows) - row0 if n is None else n
        w, h = minimap_size(params)
        lay = _yuv_layout(layout)
        need = out_span(fmt, h, w, lay, n)
        if out is None:
            out = np.zeros(need, np.uint8)
            if lay is None:
                out = out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
        if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
            raise EagleError(f"minimap: out must be a contiguous uint8 array of at least {need} bytes")
        self._check(self.L.eagle_minimap_frames(self._h, table._t, int(row0), int(n), C.byref(params), _out_pix(fmt), None if lay is None else C.byref(lay),
                                                out.ctypes.data_as(C.c_void_p)), "minimap_frames")
        return out

    # --- kinematics and pitch control (include/eagle.h, eagle_post_velocities / eagle_control_*) -------------------
    def velocities(self, table, fps, max_gap=None, speed_cap=12.0):
        """The velocity of every cell of a PostTable of this handle, computed on the GPU and kept with the table -> float64 [columns][rows][2]
        (NaN where the cell is missing; m/s, px/s for video columns).  max_gap None: fps frames."""
        p = kinematics_params(fps, max_gap, speed_cap)
        self._check(self.L.eagle_post_velocities(self._h, table._t, C.byref(p)), "post_velocities")
        v = np.zeros((len(table.columns), len(table.rows), 2), np.float64)
        self._check(self.L.eagle_post_velocity_values(table._t, v.ctypes.data_as(C.c_void_p)), "post_velocity_values")
        table.kinematics_params = p
        return v

    def velocity_values(self, table):
        """The velocities the table carries (velocities above, or smooth_tracks' fits) -> float64 [columns][rows][2]; an EagleError without any."""
        v = np.zeros((len(table.columns), len(table.rows), 2), np.float64)
        self._check(self.L.eagle_post_velocity_values(table._t, _ptr(v, np.zeros(4, np.float64))), "post_velocity_values")
        return v

    def control_device(self, table, d_out, params, row0=0, n=None, d_share=None):
        """Rows row0 .. row0 + n - 1 -> n control grids [n][gh][gw] at ``d_out`` (device memory) and, with ``d_share``, n int64 byte sums."""
        n = len(table.rows) - row0 if n is None else n
        self._check(self.L.eagle_control_device_grids(self._h, table._t, int(row0), int(n), C.byref(params), d_out, d_share), "control_device_grids")

    def control(self, table, params, row0=0, n=None):
        """As control_device, to host memory -> (uint8 [n, gh, gw], int64 [n] sums of each grid's bytes); team 0's area share is sums / (255 gw gh)."""
        n = len(table.rows) - row0 if n is None else n
        gw, gh = control_size(params)
        out, share = np.zeros((max(n, 0), gh, gw), np.uint8), np.zeros(max(n, 0), np.int64)
        keep = np.zeros(2, np.int64)
        self._check(self.L.eagle_control_grids(self._h, table._t, int(row0), int(n), C.byref(params), (out if out.size else keep).ctypes.data_as(C.c_void_p),
                                               (share if share.size else keep).ctypes.data_as(C.c_void_p)), "control_grids")
        return out, share

    # --- ball possession and pass events (include/eagle.h, eagle_post_possession / eagle_post_events) ----------------
    def possession(self, table, params):
        """Candidate, owner and events of a PostTable of this handle, computed on the GPU and kept with the table (a second call replaces the first)
        -> (cand int32 [rows], owner int32 [rows]: table columns or -1, dist float64 [rows], events EVENT_DTYPE in row order)."""
        self._check(self.L.eagle_post_possession(self._h, table._t, C.byref(params)), "post_possession")
        return self.possession_values(table) + (self.events(table),)

    def possession_values(self, table):
        """(cand int32 [rows], owner int32 [rows], dist float64 [rows]) of the table's last possession result (an EagleError before it)."""
        rows = len(table.rows)
        cand, owner, dist = np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros(rows, np.float64)
        keep = np.zeros(4, np.float64)
        self._check(self.L.eagle_post_possession_values(table._t, _ptr(cand, keep), _ptr(owner, keep), _ptr(dist, keep)), "post_possession_values")
        return cand, owner, dist

    def events(self, table):
        """The events of the table's last possession result (EVENT_DTYPE, row order; empty before it)."""
        n = C.c_int(0)
        self._check(self.L.eagle_post_events(table._t, None, 0, C.byref(n)), "post_events")
        ev = np.zeros(n.value, EVENT_DTYPE)
        self._check(self.L.eagle_post_events(table._t, _ptr(ev, np.zeros(4, np.float64)), n.value, C.byref(n)), "post_events")
        return ev

    def possession_device(self, table):
        """owner int32 [rows] in HBM (None before the first possession call of the table)."""
        d = C.c_void_p()
        self._check(self.L.eagle_post_device_possession(table._t, C.byref(d)), "post_device_possession")
        return d.value

    # --- pass options (include/eagle.h, eagle_pass_options_*) ---------------------------------------------------------------
    def pass_options_layout(self, table):
        """The table columns of the site columns (mapped Player pitch columns with a team >= 0), in table order: the second axis of the options."""
        n = C.c_int(0)
        self._check(self.L.eagle_pass_options_layout(table._t, None, 0, C.byref(n)), "pass_options_layout")
        cols = np.zeros(n.value, np.int32)
        self._check(self.L.eagle_pass_options_layout(table._t, _ptr(cols, np.zeros(4, np.float64)), n.value, C.byref(n)), "pass_options_layout")
        return cols

    def pass_options_device(self, table, params, d_rows, row0=0, n=None, d_grid=None, d_options=None):
        """Rows row0 .. row0 + n - 1 -> n records at ``d_rows`` and, where given, n grids [n][gh][gw] at ``d_grid`` and options [n][n_sites] at
        ``d_options`` (device memory)."""
        n = len(table.rows) - row0 if n is None else n
        self._check(self.L.eagle_pass_options_device(self._h, table._t, int(row0), int(n), C.byref(params), d_grid, d_rows, d_options), "pass_options_device")

    def pass_options(self, table, params, row0=0, n=None, grids=True, options=True):
        """Where the ball owner of each row can play, for a PostTable of this handle with velocities (Handle.velocities) and possession
        (Handle.possession) -> (grids uint8 [n, gh, gw] or None, records PASS_ROW_DTYPE [n], options int16 [n, n_sites] or None).  Without grids the
        grid kernel is not launched and the records' sums are 0."""
        n = len(table.rows) - row0 if n is None else n
        gw, gh = pass_options_size(params)
        ns = len(self.pass_options_layout(table)) if options else 0
        g = np.zeros((max(n, 0), gh, gw), np.uint8) if grids else None
        recs = np.zeros(max(n, 0), PASS_ROW_DTYPE)
        opt = np.zeros((max(n, 0), ns), np.int16) if options else None
        keep = np.zeros(8, np.float64)
        self._check(self.L.eagle_pass_options(self._h, table._t, int(row0), int(n), C.byref(params), _ptr(g, keep), _ptr(recs, keep), _ptr(opt, keep)), "pass_options")
        return g, recs, opt

    # --- track smoothing (include/eagle.h, eagle_post_smooth_tracks) ------------------------------------------------------------
    def smooth_tracks(self, table, params):
        """Replaces the pitch positions of the person columns (and the ball, with params.ball_window > 0) of a PostTable of this handle by windowed
        least-squares fits, in HBM, sets the table's velocities to the fits' derivatives and keeps the rest with the table; it comes before every
        other result and once -> {"velocities", "acc": float64 [columns][rows][2]; "flags", "count": uint8 and "residual_q": int32 [columns][rows];
        "suspect": uint8 [rows]; "totals": SMOOTH_TOTALS_DTYPE [columns]}.  table.values is the smoothed table afterwards, raw_values(table) the old one."""
        self._check(self.L.eagle_post_smooth_tracks(self._h, table._t, C.byref(params)), "post_smooth_tracks")
        table._values = None
        table.kinematics_params = kinematics_params(params.fps, params.max_gap, params.speed_cap)
        cols, rows = len(table.columns), len(table.rows)
        out = {"velocities": np.zeros((cols, rows, 2), np.float64), "acc": np.zeros((cols, rows, 2), np.float64), "flags": np.zeros((cols, rows), np.uint8),
               "count": np.zeros((cols, rows), np.uint8), "residual_q": np.zeros((cols, rows), np.int32), "suspect": np.zeros(rows, np.uint8),
               "totals": np.zeros(cols, SMOOTH_TOTALS_DTYPE)}
        keep = np.zeros(8, np.float64)
        self._check(self.L.eagle_post_smooth_values(table._t, _ptr(out["acc"], keep), _ptr(out["flags"], keep), _ptr(out["count"], keep), _ptr(out["residual_q"], keep),
                                                    _ptr(out["suspect"], keep), _ptr(out["totals"], keep)), "post_smooth_values")
        self._check(self.L.eagle_post_velocity_values(table._t, _ptr(out["velocities"], keep)), "post_velocity_values")
        return out

    def raw_values(self, table):
        """The positions of the table from before smooth_tracks (the table's own without one) -> float64 [columns][rows][2]."""
        v = np.zeros((len(table.columns), len(table.rows), 2), np.float64)
        self._check(self.L.eagle_post_raw_values(table._t, _ptr(v, np.zeros(4, np.float64))), "post_raw_values")
        return v

    def smooth_device(self, table):
        """(acc float64 [columns][rows][2], flags uint8 [columns][rows], suspect uint8 [rows]) in HBM (None each before smooth_tracks)."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.L.eagle_post_device_smooth(table._t, C.byref(a), C.byref(b), C.byref(c)), "post_device_smooth")
        return a.value, b.value, c.value

    # --- ball flights (include/eagle.h, eagle_post_ball_flights) ------------------------------------------------------------
    def ball_flights(self, table, params, cuts=None):
        """Cuts the ball's pitch column of a PostTable of this handle into flights and kicks and keeps the result with the table (a later call replaces it)
        -> {"seg": int32 [rows], "flags": uint8 [rows], "fitted", "velocity": float64 [rows][2], "flights": FLIGHT_DTYPE, "kicks": KICK_DTYPE, "totals":
        FLIGHT_TOTALS_DTYPE [1]}; cuts: the ascending frame numbers that start a new shot."""
        cuts = np.zeros(0, np.int32) if cuts is None else np.ascontiguousarray(cuts, np.int32)
        self._check(self.L.eagle_post_ball_flights(self._h, table._t, C.byref(params), cuts.ctypes.data_as(C.c_void_p) if len(cuts) else None, len(cuts)), "post_ball_flights")
        return self.ball_flight_values(table)

    def ball_flight_values(self, table):
        """What ball_flights kept with the table; an EagleError before the call."""
        rows = len(table.rows)
        out = {"seg": np.zeros(rows, np.int32), "flags": np.zeros(rows, np.uint8), "fitted": np.zeros((rows, 2), np.float64), "velocity": np.zeros((rows, 2), np.float64),
               "totals": np.zeros(1, FLIGHT_TOTALS_DTYPE)}
        keep = np.zeros(8, np.float64)
        self._check(self.L.eagle_post_ball_flight_values(table._t, *(_ptr(out[k], keep) for k in ("seg", "flags", "fitted", "velocity", "totals"))), "post_ball_flight_values")
        n = C.c_int(0)
        self._check(self.L.eagle_post_ball_flight_records(table._t, None, 0, C.byref(n)), "post_ball_flight_records")
        out["flights"] = np.zeros(n.value, FLIGHT_DTYPE)
        self._check(self.L.eagle_post_ball_flight_records(table._t, _ptr(out["flights"], keep), n.value, C.byref(n)), "post_ball_flight_records")
        self._check(self.L.eagle_post_ball_kicks(table._t, None, 0, C.byref(n)), "post_ball_kicks")
        out["kicks"] = np.zeros(n.value, KICK_DTYPE)
        self._check(self.L.eagle_post_ball_kicks(table._t, _ptr(out["kicks"], keep), n.value, C.byref(n)), "post_ball_kicks")
        return out

    # --- goal view (include/eagle.h, eagle_post_goal_view) ------------------------------------------------------------------
    def goal_view(self, table, params):
        """How much of the goal mouth every member, the ball and (with params.grid_rows) every cell sees on a PostTable of this handle that has a team
        mapping; kept with the table (a later call replaces it) -> goal_view_values(table)."""
        self._check(self.L.eagle_post_goal_view(self._h, table._t, C.byref(params)), "post_goal_view")
        return self.goal_view_values(table)

    def goal_view_values(self, table):
        """What goal_view kept with the table -> {"rows": GOALVIEW_ROW_DTYPE [rows, 2], "open": int32, "mask": uint64, "status": uint8 [members, rows],
        "totals": GOALVIEW_TOTALS_DTYPE [members], "grid": uint8 [grid_rows, 68 R, 105 R], "grid_row0": int}; an EagleError before the call."""
        d = self.goal_view_device(table)
        if d[0] is None:
            self._check(self.L.eagle_post_goal_view_values(table._t, None, None, None, None, None, None), "post_goal_view_values")
        nm, row0, gr, R = d[6:]
        rows = len(table.rows)
        out = {"rows": np.zeros((rows, 2), GOALVIEW_ROW_DTYPE), "open": np.zeros((nm, rows), np.int32), "mask": np.zeros((nm, rows), np.uint64),
               "status": np.zeros((nm, rows), np.uint8), "totals": np.zeros(nm, GOALVIEW_TOTALS_DTYPE), "grid": np.zeros((gr, 68 * R, 105 * R), np.uint8)}
        keep = np.zeros(8, np.float64)
        self._check(self.L.eagle_post_goal_view_values(table._t, *(_ptr(out[k], keep) for k in ("rows", "open", "mask", "status", "totals", "grid"))), "post_goal_view_values")
        out["grid_row0"] = row0
        return out

    def goal_view_device(self, table):
        """(records, open, mask, status, totals, grid in HBM, members, grid_row0, grid_rows, cells per metre); (None,) * 6 + (0,) * 4 before goal_view."""
        d = [C.c_void_p() for _ in range(6)]
        n = [C.c_int(0) for _ in range(4)]
        self._check(self.L.eagle_post_device_goal_view(table._t, *[C.byref(x) for x in d], *[C.byref(x) for x in n]), "post_device_goal_view")
        return tuple(x.value for x in d) + tuple(x.value for x in n)

    def ball_flights_device(self, table):
        """(seg int32 [rows], flags uint8 [rows], fitted, velocity float64 [rows][2]) in HBM (None each before ball_flights)."""
        p = [C.c_void_p() for _ in range(4)]
        self._check(self.L.eagle_post_device_ball_flights(table._t, *(C.byref(v) for v in p)), "post_device_ball_flights")
        return tuple(v.value for v in p)

    # --- stabilisation (include/eagle.h, eagle_post_stabilise) ------------------------------------------------------------
    def stabilise(self, table, params):
        """Estimates and removes each row's common motion from the Player, Goalkeeper and Ball pitch columns of a PostTable of this handle, in HBM; it
        comes before smooth_tracks and every other result, and once -> {"rows": STAB_ROW_DTYPE [rows], "totals": STAB_TOTALS_DTYPE [1], "votes": int32
        [columns][rows][2]}.  table.values is the stabilised table afterwards, original_values(table) the old one."""
        self._check(self.L.eagle_post_stabilise(self._h, table._t, C.byref(params)), "post_stabilise")
        table._values = None
        cols, rows = len(table.columns), len(table.rows)
        out = {"rows": np.zeros(rows, STAB_ROW_DTYPE), "totals": np.zeros(1, STAB_TOTALS_DTYPE), "votes": np.zeros((cols, rows, 2), np.int32)}
        keep = np.zeros(8, np.float64)
        self._check(self.L.eagle_post_stabilise_values(table._t, _ptr(out["rows"], keep), _ptr(out["totals"], keep), _ptr(out["votes"], keep)), "post_stabilise_values")
        return out

    def original_values(self, table):
        """The positions of the table from before stabilise (the table's own without one) -> float64 [columns][rows][2]."""
        v = np.zeros((len(table.columns), len(table.rows), 2), np.float64)
        self._check(self.L.eagle_post_original_values(table._t, _ptr(v, np.zeros(4, np.float64))), "post_original_values")
        return v

    def stabilise_device(self, table):
        """The row records (STAB_ROW_DTYPE [rows]) in HBM; None before stabilise."""
        a = C.c_void_p()
        self._check(self.L.eagle_post_device_stabilise(table._t, C.byref(a)), "post_device_stabilise")
        return a.value

    # --- physical report (include/eagle.h, eagle_post_physical) ------------------------------------------------------------
    def physical(self, table, params):
        """Speed, its derivative and the speed zone per person and row, the totals per person and the efforts of a PostTable of this handle with
        velocities (Handle.velocities), computed on the GPU and kept with the table (a second call replaces the first) -> (speed float64, accel float64,
        zone uint8: [persons, rows] each; totals LOAD_TOTALS_DTYPE [persons]; efforts LOAD_EFFORT_DTYPE in (person, kind, first_row) order).  The persons
        are the Player and Goalkeeper pitch columns in table order (totals["col"]); without rows or persons everything is empty."""
        self._check(self.L.eagle_post_physical(self._h, table._t, C.byref(params)), "post_physical")
        keep = np.zeros(4, np.float64)
        n = C.c_int(0)
        self._check(self.L.eagle_post_physical_totals(table._t, None, 0, C.byref(n)), "post_physical_totals")
        totals = np.zeros(n.value, LOAD_TOTALS_DTYPE)
        self._check(self.L.eagle_post_physical_totals(table._t, _ptr(totals, keep), n.value, C.byref(n)), "post_physical_totals")
        persons, rows = len(totals), len(table.rows)
        speed, accel, zone = np.zeros((persons, rows), np.float64), np.zeros((persons, rows), np.float64), np.zeros((persons, rows), np.uint8)
        if persons and rows:
            self._check(self.L.eagle_post_physical_values(table._t, _ptr(speed, keep), _ptr(accel, keep), _ptr(zone, keep)), "post_physical_values")
        self._check(self.L.eagle_post_physical_efforts(table._t, None, 0, C.byref(n)), "post_physical_efforts")
        ev = np.zeros(n.value, LOAD_EFFORT_DTYPE)
        self._check(self.L.eagle_post_physical_efforts(table._t, _ptr(ev, keep), n.value, C.byref(n)), "post_physical_efforts")
        return speed, accel, zone, totals, ev

    def physical_device(self, table):
        """(speed float64, zone uint8) [persons, rows] in HBM (None, None before the first physical call of the table)."""
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self.L.eagle_post_device_physical(table._t, C.byref(a), C.byref(b)), "post_device_physical")
        return a.value, b.value

    # --- occupancy heat maps (include/eagle.h, eagle_post_occupancy / eagle_occupancy_picture) -------------------------------
    def occupancy(self, table, params, sel_off, sel_cols):
        """The maps of the selections (CSR: sel_off [n_sel + 1], sel_cols table column indices) of a PostTable of this handle, computed on the GPU and
        kept with the table (a second call replaces the first) -> (grids float32, bytes uint8, counts int32: [n_sel, gh, gw] each; total, outside
        int64 [n_sel]).  The grids are in frames."""
        sel_off, sel_cols = np.ascontiguousarray(sel_off, np.int32), np.ascontiguousarray(sel_cols, np.int32)
        n_sel = len(sel_off) - 1
        keep = np.zeros(4, np.float64)
        self._check(self.L.eagle_post_occupancy(self._h, table._t, C.byref(params), _ptr(sel_off, keep), _ptr(sel_cols, keep), n_sel), "post_occupancy")
        gw, gh = occupancy_size(params)
        grids, by, counts = np.zeros((n_sel, gh, gw), np.float32), np.zeros((n_sel, gh, gw), np.uint8), np.zeros((n_sel, gh, gw), np.int32)
        total, outside = np.zeros(n_sel, np.int64), np.zeros(n_sel, np.int64)
        self._check(self.L.eagle_post_occupancy_values(table._t, _ptr(grids, keep), _ptr(by, keep), _ptr(total, keep), _ptr(outside, keep), _ptr(counts, keep)),
                    "post_occupancy_values")
        return grids, by, counts, total, outside

    def occupancy_device(self, table):
        """(grids float32, bytes uint8) [n_sel, gh, gw] in HBM (None, None before the first occupancy call of the table)."""
        g, b = C.c_void_p(), C.c_void_p()
        self._check(self.L.eagle_post_device_occupancy(table._t, C.byref(g), C.byref(b)), "post_device_occupancy")
        return g.value, b.value

    def occupancy_picture(self, table, sel, scale=8, margin=None, colour=(255, 255, 255)):
        """Selection ``sel`` of the table's last occupancy result as a still picture of the pitch -> BGR uint8 [h, w, 3]; colour (b, g, r)."""
        mp = minimap_params(scale, margin)
        w, h = minimap_size(mp)
        out = np.zeros((h, w, 3), np.uint8)
        self._check(self.L.eagle_occupancy_picture(self._h, table._t, int(sel), mp.scale, mp.margin, _bgr(colour), out.ctypes.data_as(C.c_void_p)), "occupancy_picture")
        return out

    def minimap_set_trails(self, table, params, cols=()):
        """The parameters (trail_params) and the selected table columns the minimap's trail, pass and owner layers of this table are drawn with (params
        None: forget them; no columns: passes and owner only)."""
        cols = np.ascontiguousarray(cols, np.int32)
        keep = np.zeros(4, np.int32)
        self._check(self.L.eagle_minimap_set_trails(table._t, None if params is None else C.byref(params), _ptr(cols, keep), len(cols)), "minimap_set_trails")

    def trajectory_picture(self, table, cols, row0=0, n=None, scale=8, margin=None, half_width=1, max_gap=25):
        """The paths of the selected table columns over rows row0 .. row0 + n - 1 as a still picture of the pitch -> BGR uint8 [h, w, 3]."""
        mp = minimap_params(scale, margin)
        w, h = minimap_size(mp)
        cols = np.ascontiguousarray(cols, np.int32)
        keep = np.zeros(4, np.int32)
        n = len(table.rows) - row0 if n is None else n
        out = np.zeros((h, w, 3), np.uint8)
        self._check(self.L.eagle_trajectory_picture(self._h, table._t, _ptr(cols, keep), len(cols), int(row0), int(n), mp.scale, mp.margin, int(half_width), int(max_gap),
                                                    out.ctypes.data_as(C.c_void_p)), "trajectory_picture")
        return out

    def pass_picture(self, table, event, scale=8, margin=None, half_width=1):
        """Event ``event`` of the table's last possession result at its release row as a still picture -> BGR uint8 [h, w, 3]."""
        mp = minimap_params(scale, margin)
        w, h = minimap_size(mp)
        out = np.zeros((h, w, 3), np.uint8)
        self._check(self.L.eagle_pass_picture(self._h, table._t, int(event), mp.scale, mp.margin, int(half_width), out.ctypes.data_as(C.c_void_p)), "pass_picture")
        return out

    # --- team shape (include/eagle.h, eagle_post_team_shape / eagle_minimap_set_hulls) ---------------------------------------
    def team_shape(self, table):
        """The shape records and hulls of a PostTable of this handle (it needs a team mapping), computed on the GPU and kept with the table (a second
        call replaces the first) -> (SHAPE_DTYPE [rows, 2], int32 [rows, 2, SHAPE_HULL_CAP]: table columns, -1 padded).  eagle_amd.shape derives metres."""
        self._check(self.L.eagle_post_team_shape(self._h, table._t), "post_team_shape")
        rows = len(table.rows)
        rec, hull = np.zeros((rows, 2), SHAPE_DTYPE), np.zeros((rows, 2, SHAPE_HULL_CAP), np.int32)
        keep = np.zeros(4, np.float64)
        self._check(self.L.eagle_post_team_shape_values(table._t, _ptr(rec, keep), _ptr(hull, keep)), "post_team_shape_values")
        return rec, hull

    def team_shape_device(self, table):
        """(records, hull) in HBM (None, None before the first team_shape call of the table)."""
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self.L.eagle_post_device_team_shape(table._t, C.byref(a), C.byref(b)), "post_device_team_shape")
        return a.value, b.value

    # --- roles (include/eagle.h, eagle_post_roles) -------------------------------------------------------------------------------
    def roles(self, table, params=None):
        """The role assignment of a PostTable of this handle (it needs a team mapping), computed on the GPU and kept with the table (a second call
        replaces the first; a refused one leaves it) -> (ROLE_ROW_DTYPE [rows, 2], int8 [members, rows], ROLE_MODEL_DTYPE [1]); params role_params(...).
        The members are the table's member columns in group order (eagle_amd.shape.member_columns).  eagle_amd.roles derives lines and labels."""
        p = role_params() if params is None else params
        self._check(self.L.eagle_post_roles(self._h, table._t, C.byref(p)), "post_roles")
        nm = self.roles_device(table)[3]
        rows = len(table.rows)
        rec, mr, model = np.zeros((rows, 2), ROLE_ROW_DTYPE), np.full((nm, rows), -1, np.int8), np.zeros(1, ROLE_MODEL_DTYPE)
        keep = np.zeros(4, np.float64)
        self._check(self.L.eagle_post_roles_values(table._t, _ptr(rec, keep), _ptr(mr, keep), _ptr(model, keep)), "post_roles_values")
        return rec, mr, model

    def roles_device(self, table):
        """(records, member roles, model, members) in HBM ((None, None, None, 0) before the first roles call of the table)."""
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        self._check(self.L.eagle_post_device_roles(table._t, C.byref(a), C.byref(b), C.byref(c), C.byref(n)), "post_device_roles")
        return a.value, b.value, c.value, n.value

    # --- space per player (include/eagle.h, eagle_post_space / eagle_space_grids) ------------------------------------------------
    def space(self, table, params=None):
        """The dominant regions and the marking of a PostTable of this handle (it needs a team mapping), computed on the GPU and kept with the table (a
        second call replaces the first; a refused one leaves it) -> (SPACE_ROW_DTYPE [rows], SPACE_SITE_DTYPE [rows, 32], SPACE_TOTALS_DTYPE
        [members]); params space_params(...).  eagle_amd.space derives square metres and metres."""
        p = space_params() if params is None else params
        self._check(self.L.eagle_post_space(self._h, table._t, C.byref(p)), "post_space")
        nm = self.space_device(table)[3]
        rows = len(table.rows)
        rec, sites, totals = np.zeros(rows, SPACE_ROW_DTYPE), np.zeros((rows, SPACE_SITE_CAP), SPACE_SITE_DTYPE), np.zeros(nm, SPACE_TOTALS_DTYPE)
        keep = np.zeros(8, np.float64)
        self._check(self.L.eagle_post_space_values(table._t, _ptr(rec, keep), _ptr(sites, keep), _ptr(totals, keep)), "post_space_values")
        return rec, sites, totals

    def space_device(self, table):
        """(records, sites, totals, members) in HBM ((None, None, None, 0) before the first space call of the table)."""
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        self._check(self.L.eagle_post_device_space(table._t, C.byref(a), C.byref(b), C.byref(c), C.byref(n)), "post_device_space")
        return a.value, b.value, c.value, n.value

    def space_grids(self, table, params=None, row0=0, n=None):
        """The owner maps of rows row0 .. row0 + n - 1 -> uint8 [n, gh, gw]: the owner's index into the row's site list, SPACE_NO_OWNER on a row that is
        not active.  Computed from the table itself: the kept result is neither needed nor touched."""
        p = space_params() if params is None else params
        n = len(table.rows) - row0 if n is None else n
        g = np.zeros((max(n, 0), 68 * p.cells_per_metre, 105 * p.cells_per_metre), np.uint8)
        self._check(self.L.eagle_space_grids(self._h, table._t, int(row0), int(n), C.byref(p), _ptr(g, np.zeros(8, np.float64))), "space_grids")
        return g

    def space_device_grids(self, table, params, d_grid, row0=0, n=None):
        """space_grids into device memory: n maps [n][gh][gw] at ``d_grid``."""
        n = len(table.rows) - row0 if n is None else n
        self._check(self.L.eagle_space_device_grids(self._h, table._t, int(row0), int(n), C.byref(params), d_grid), "space_device_grids")

    # --- offside (include/eagle.h, eagle_post_offside) ----------------------------------------------------------------------------
    def offside(self, table, params=None):
        """The offside lines and margins of a PostTable of this handle (it needs a team mapping), computed on the GPU and kept with the table (a second
        call replaces the first; a refused one leaves it) -> (OFFSIDE_ROW_DTYPE [rows, 2], margins int32 [members, rows], OFFSIDE_TOTALS_DTYPE
        [members], OFFSIDE_CLIP_DTYPE [1]); params offside_params(...).  With a possession result on the table the passes get their verdicts
        (offside_events).  eagle_amd.offside derives metres."""
        p = offside_params() if params is None else params
        self._check(self.L.eagle_post_offside(self._h, table._t, C.byref(p)), "post_offside")
        nm = self.offside_device(table)[5]
        rows = len(table.rows)
        rec, mg, totals, clip = np.zeros((rows, 2), OFFSIDE_ROW_DTYPE), np.zeros((nm, rows), np.int32), np.zeros(nm, OFFSIDE_TOTALS_DTYPE), np.zeros(1, OFFSIDE_CLIP_DTYPE)
        keep = np.zeros(8, np.float64)
        self._check(self.L.eagle_post_offside_values(table._t, _ptr(rec, keep), _ptr(mg, keep), _ptr(totals, keep), _ptr(clip, keep)), "post_offside_values")
        return rec, mg, totals, clip

    def offside_events(self, table):
        """The event records of the table's last offside result (OFFSIDE_EVENT_DTYPE, one per possession event, in event order; empty before it)."""
        n = C.c_int(0)
        self._check(self.L.eagle_post_offside_events(table._t, None, 0, C.byref(n)), "post_offside_events")
        ev = np.zeros(n.value, OFFSIDE_EVENT_DTYPE)
        self._check(self.L.eagle_post_offside_events(table._t, _ptr(ev, np.zeros(4, np.float64)), n.value, C.byref(n)), "post_offside_events")
        return ev

    def offside_device(self, table):
        """(records, margins, totals, clip record, event records, members, events) in HBM ((None,) * 5 + (0, 0) before the first offside call)."""
        d = [C.c_void_p() for _ in range(5)]
        nm, ne = C.c_int(0), C.c_int(0)
        self._check(self.L.eagle_post_device_offside(table._t, *[C.byref(x) for x in d], C.byref(nm), C.byref(ne)), "post_device_offside")
        return tuple(x.value for x in d) + (nm.value, ne.value)

    def set_hulls(self, table, half_width=1):
        """The half width (pixels, 1 .. 8; or an EagleHullParams) the minimap's hull layer (MM_HULLS) of this table is drawn with; None: forget it."""
        p = half_width if isinstance(half_width, EagleHullParams) or half_width is None else hull_params(half_width)
        self._check(self.L.eagle_minimap_set_hulls(table._t, None if p is None else C.byref(p)), "minimap_set_hulls")

    def minimap_set_control(self, table, params):
        """The parameters the minimap's ``control`` layer of this table is computed with (None: forget them)."""
        self._check(self.L.eagle_minimap_set_control(table._t, None if params is None else C.byref(params)), "minimap_set_control")

    def reproject(self, recs, Hs, flags):
        """In place: re-project foot points / boundaries of the flagged records with the given homographies (cadence mode)."""
        Hs = np.ascontiguousarray(Hs, np.float64).reshape(-1, 9)
        flags = np.ascontiguousarray(flags, np.uint8)
        assert recs.flags.c_contiguous and len(Hs) == len(flags) == len(recs)
        self._check(self.L.eagle_reproject(self._h, recs.ctypes.data_as(C.c_void_p), len(recs), Hs.ctypes.data_as(C.POINTER(C.c_double)),
                                           flags.ctypes.data_as(C.POINTER(C.c_uint8))), "reproject")
        return recs

    # --- clip session: optical-flow key-point cadence (include/eagle.h, eagle_clip_*) --------------------
    def clip_open(self, dptr, n):
        self._check(self.L.eagle_clip_open(self._h, dptr, n), "clip_open")

    def clip_close(self):
        self._check(self.L.eagle_clip_close(self._h), "clip_close")

    def clip_detect_objects(self, first, count):
        self._check(self.L.eagle_clip_detect_objects(self._h, first, count), "clip_detect_objects")

    def clip_detect_keypoints(self, first, stride=1, count=1):
        self._check(self.L.eagle_clip_detect_keypoints(self._h, first, stride, count), "clip_detect_keypoints")

    def clip_get_keypoints(self, frame):
        """mem[frame] as a FLOWKP_DTYPE array in dict order, or None when the frame has no entry."""
        buf = np.zeros(N_LANDMARKS, FLOWKP_DTYPE); n = C.c_int(0)
        self._check(self.L.eagle_clip_get_keypoints(self._h, frame, buf.ctypes.data_as(C.c_void_p), C.byref(n)), "clip_get_keypoints")
        return None if n.value < 0 else buf[: n.value].copy()

    def clip_set_keypoints(self, frame, kps):
        kps = np.ascontiguousarray(kps, FLOWKP_DTYPE)
        self._check(self.L.eagle_clip_set_keypoints(self._h, frame, kps.ctypes.data_as(C.c_void_p), len(kps)), "clip_set_keypoints")

    def clip_flow(self, src_frame, dst_frame, hue_frame, kps, raw=False):
        """calculate_optical_flow (cm.py:419-478) on resident frames -> filtered FLOWKP_DTYPE array (+ raw LK output)."""
        kps = np.ascontiguousarray(kps, FLOWKP_DTYPE)
        out = np.zeros(N_LANDMARKS, FLOWKP_DTYPE); n = C.c_int(0)
        nxt = np.zeros((max(len(kps), 1), 2), np.float32); st = np.zeros(max(len(kps), 1), np.uint8)
        self._check(self.L.eagle_clip_flow(self._h, src_frame, dst_frame, hue_frame, kps.ctypes.data_as(C.c_void_p), len(kps),
                                           out.ctypes.data_as(C.c_void_p), C.byref(n), _fp(nxt), st.ctypes.data_as(C.POINTER(C.c_uint8))), "clip_flow")
        return (out[: n.value].copy(), nxt[: len(kps)], st[: len(kps)]) if raw else out[: n.value].copy()

    def clip_run(self, first, last, keypoint_interval, homography_interval, calibration=False, wait=True):
        """Enqueues the loop body for frames [first, last) on the GPU; wait=True -> index of a frame that needs an on-demand
        detection, or -1 when every frame enqueued so far is done."""
        stalled = C.c_int(-1)
        rc = self.L.eagle_clip_run(self._h, first, last, keypoint_interval, homography_interval, int(calibration), int(wait), C.byref(stalled))
        if rc == E_REFERENCE_RAISES:
            raise IndexError(self.L.eagle_last_error(self._h).decode())
        self._check(rc, "clip_run")
        return stalled.value

    def clip_fetch(self, n):
        out = np.zeros(n, RESULT_DTYPE)
        self._check(self.L.eagle_clip_fetch(self._h, out.ctypes.data_as(C.c_void_p)), "clip_fetch")
        return out

    def team_colors(self, dptr, n_frames, crops):
        """crops: int32 [k,5] (frame, x1, y1, x2, y2) of a clip resident in HBM -> int32 [k,12] colour-range counts (include/eagle.h)."""
        crops = np.ascontiguousarray(crops, np.int32).reshape(-1, 5)
        out = np.zeros((len(crops), 12), np.int32)
        self._check(self.L.eagle_team_colors(self._h, dptr, n_frames, crops.ctypes.data_as(C.c_void_p), len(crops), out.ctypes.data_as(C.c_void_p)), "team_colors")
        return out

    def team_cluster(self, dptr, n_frames, crops, slots, n_ids, params=None):
        """The team clustering on a clip resident in HBM (include/eagle.h, eagle_team_cluster): crops int32 [k, 5] (frame, x1, y1, x2, y2), slots int32 [k]
        (0 .. n_ids - 1) -> (KIT_CROP_DTYPE [k], KIT_ID_DTYPE [n_ids], KIT_MODEL_DTYPE [1]); params kit_params(...)."""
        crops = np.ascontiguousarray(crops, np.int32).reshape(-1, 5)
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        if len(slots) != len(crops):
            raise ValueError(f"team_cluster: {len(slots)} slots for {len(crops)} crops")
        params = params or kit_params()
        recs, ids, model = np.zeros(len(crops), KIT_CROP_DTYPE), np.zeros(int(n_ids), KIT_ID_DTYPE), np.zeros(1, KIT_MODEL_DTYPE)
        keep = np.zeros(64, np.float64)
        self._check(self.L.eagle_team_cluster(self._h, dptr, int(n_frames), _ptr(crops, keep), _ptr(slots, keep), len(crops), int(n_ids), C.byref(params),
                                              _ptr(recs, keep), _ptr(ids, keep), _ptr(model, keep)), "team_cluster")
        return recs, ids, model

    # --- track identities (include/eagle.h, eagle_track_*) -------------------------------------------------
    def track_open(self, **params):
        p = None
        if params:
            d = dict(track_high_thresh=0.5, track_low_thresh=0.1, new_track_thresh=0.6, match_thresh=0.8, track_buffer=30, frame_rate=30)
            d.update(params)
            p = C.byref(EagleTrackParams(**d))
        self._check(self.L.eagle_track_open(self._h, p), "track_open")

    def reid_features(self, dptr, n_frames, crops):
        """crops: int32 [k,5] (frame, x1, y1, x2, y2) of a clip resident in HBM -> float32 [k, 512] OSNet-x0.25 embeddings (needs the reid.* weights)."""
        crops = np.ascontiguousarray(crops, np.int32).reshape(-1, 5)
        out = np.zeros((len(crops), 512), np.float32)
        self._check(self.L.eagle_reid_features(self._h, dptr, n_frames, crops.ctypes.data_as(C.c_void_p), len(crops), out.ctypes.data_as(C.POINTER(C.c_float))), "reid_features")
        return out

    def track_frames_reid(self, recs, feats, feat_det, feat_count, warps=None):
        """track_frames with appearance: record i owns feat_count[i] consecutive rows of feats; feat_det = their detection indices."""
        assert recs.dtype == RESULT_DTYPE and recs.flags.c_contiguous
        feats = np.ascontiguousarray(feats, np.float32).reshape(-1, 512)
        feat_det = np.ascontiguousarray(feat_det, np.int32); feat_count = np.ascontiguousarray(feat_count, np.int32)
        assert len(feat_count) == len(recs) and int(feat_count.sum()) == len(feats) == len(feat_det)
        w = None if warps is None else np.ascontiguousarray(warps, np.float64).reshape(len(recs), 6)
        self._check(self.L.eagle_track_frames_reid(self._h, recs.ctypes.data_as(C.c_void_p), len(recs), None if w is None else w.ctypes.data_as(C.POINTER(C.c_double)),
                                                   feats.ctypes.data_as(C.POINTER(C.c_float)), feat_det.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   feat_count.ctypes.data_as(C.POINTER(C.c_int32))), "track_frames_reid")
        return recs

    def track_frames(self, recs, warps=None):
        """In place: the next records of the clip being tracked (frame order).  warps: optional [len(recs), 6] camera motions (clip_motion)."""
        assert recs.dtype == RESULT_DTYPE and recs.flags.c_contiguous
        w = None
        if warps is not None:
            w = np.ascontiguousarray(warps, np.float64).reshape(len(recs), 6)
        self._check(self.L.eagle_track_frames_cmc(self._h, recs.ctypes.data_as(C.c_void_p), len(recs),
                                                  w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None), "track_frames")
        return recs

    def clip_motion(self, first, count):
        """[count, 6] float64: row-major 2 x 3 camera motion of frame first+i-1 -> first+i of the open clip session (identity for frame 0)."""
        w = np.zeros((max(count, 0), 6), np.float64)
        self._check(self.L.eagle_clip_motion(self._h, first, count, w.ctypes.data_as(C.POINTER(C.c_double))), "clip_motion")
        return w

    def clip_motion_ecc(self, first, count, carry=False, return_ok=False):
        """boxmot's default camera-motion estimator (ECC on the 0.15-scale gray frame): [count, 6] float64 warps like clip_motion; carry=True
        keeps the estimator's template across clips (the tracker's lifetime; track_open forgets it)."""
        w = np.zeros((max(count, 0), 6), np.float64)
        ok = np.zeros(max(count, 0), np.int32)
        self._check(self.L.eagle_clip_motion_ecc(self._h, first, count, int(bool(carry)), w.ctypes.data_as(C.POINTER(C.c_double)),
                                                 ok.ctypes.data_as(C.POINTER(C.c_int32))), "clip_motion_ecc")
        return (w, ok) if return_ok else w

    def set_profiling(self, on):
        self._check(self.L.eagle_set_profiling(self._h, int(on)), "set_profiling")

    def timings(self):
        t = EagleTimings()
        self._check(self.L.eagle_get_timings(self._h, C.byref(t)), "get_timings")
        return t

    def kernel_times(self):
        """[(name, total ms, launches, algorithmic bytes, flop)] since set_profiling(1): one row per non-convolution kernel and one per
        convolution layer shape ("conv 3x3/1 96->96 @68x120")."""
        buf = (EagleKernelTime * 256)(); n = C.c_int(0)
        self._check(self.L.eagle_get_kernel_times(self._h, buf, 256, C.byref(n)), "get_kernel_times")
        return [(buf[i].name.decode(), float(buf[i].ms), int(buf[i].launches), float(buf[i].bytes), float(buf[i].flop)) for i in range(min(n.value, 256))]

    # --- multi-GPU -------------------------------------------------------------------------------------
    def comm_init(self, rank, world, uid_bytes):
        buf = C.create_string_buffer(bytes(uid_bytes), 128)
        self._check(self.L.eagle_comm_init(self._h, rank, world, buf), "comm_init")

    def gather(self, local, world, out=None):
        local = np.ascontiguousarray(local)
        if out is None:
            out = np.zeros(len(local) * world, RESULT_DTYPE)
        assert out.dtype == RESULT_DTYPE and len(out) == len(local) * world and out.flags.c_contiguous
        self._check(self.L.eagle_gather(self._h, local.ctypes.data_as(C.c_void_p), len(local), out.ctypes.data_as(C.c_void_p)), "gather")
        return out


BOUNDARY_NAMES = ("Bottom_Left", "Top_Left", "Top_Right", "Bottom_Right")


class PostTable:
    """A processed clip table (EaglePostTable): ``rows`` kept frame numbers, ``columns`` (POSTCOL_DTYPE, table order) and their reference ``names``,
    ``flags``, ``merges`` (the links of the id merge, one dict of POSTMERGE_DTYPE's fields each), ``team_mapping``; ``values`` copies the table to the host once: float64 [columns][rows][2], NaN = missing.  close() frees the device memory."""

    def __init__(self, handle, ptr, team_mapping=None):
        self.handle, self._t, self.team_mapping = handle, ptr, team_mapping
        L = handle.L
        r, c, f = C.c_int32(), C.c_int32(), C.c_int32()
        L.eagle_post_shape(ptr, C.byref(r), C.byref(c), C.byref(f))
        self.flags = f.value
        self.rows = np.zeros(r.value, np.int32)
        self.columns = np.zeros(c.value, POSTCOL_DTYPE)
        L.eagle_post_layout(ptr, self.rows.ctypes.data_as(C.c_void_p), self.columns.ctypes.data_as(C.c_void_p))
        self.names = [BOUNDARY_NAMES[int(k["id"])] if k["kind"] == POST_BOUNDARY else
                      ("Ball" if k["kind"] == POST_BALL else f"{'Player' if k['kind'] == POST_PLAYER else 'Goalkeeper'}_{int(k['id'])}") + ("_video" if k["video"] else "")
                      for k in self.columns]
        self._values = None
        n = C.c_int(0)
        L.eagle_post_merges(ptr, None, 0, C.byref(n))
        m = np.zeros(n.value, POSTMERGE_DTYPE)
        L.eagle_post_merges(ptr, m.ctypes.data_as(C.c_void_p), n.value, C.byref(n))
        self.merges = [{k: (float(e[k]) if k == "dist" else int(e[k])) for k in POSTMERGE_DTYPE.names} for e in m]
        if self.merges and team_mapping is not None:        # the heads' inherited teams (the library's own copy of the mapping holds them too)
            self.team_mapping = dict(team_mapping)
            heads = {(e["kind"], e["head_id"]): e["team"] for e in self.merges if e["team"] >= 0}
            for k in self.columns:                          # in table order, as the library adds them
                if k["video"] and (int(k["kind"]), int(k["id"])) in heads and self.team_mapping.get(int(k["id"]), -1) < 0:
                    self.team_mapping[int(k["id"])] = heads[(int(k["kind"]), int(k["id"]))]            # (an entry below 0 is no team: replaced)

    @property
    def values(self):
        if self._values is None:
            v = np.zeros((len(self.columns), len(self.rows), 2), np.float64)
            self.handle._check(self.handle.L.eagle_post_values(self._t, v.ctypes.data_as(C.c_void_p)), "post_values")
            self._values = v
        return self._values

    @property
    def device_values(self):
        d = C.c_void_p()
        self.handle._check(self.handle.L.eagle_post_device_values(self._t, C.byref(d)), "post_device_values")
        return d.value

    def overlay(self, row, rec=None):
        """The primitives drawn for processed row ``row`` (+ the key-points of ``rec``) -> PRIM_DTYPE array (eagle_overlay_from_table)."""
        cap = 2 * len(self.columns) + MAX_PRIMS
        out = np.zeros(cap, PRIM_DTYPE); n = C.c_int(0)
        rec = None if rec is None else np.ascontiguousarray(rec, RESULT_DTYPE).reshape(-1)[:1]
        self.handle._check(self.handle.L.eagle_overlay_from_table(self._t, int(row), None if rec is None else rec.ctypes.data_as(C.c_void_p),
                                                                  out.ctypes.data_as(C.c_void_p), cap, C.byref(n)), "overlay_from_table")
        return out[: n.value].copy()

    def close(self):
        if self._t:
            _ = self.values                     # (the host view outlives the device memory)
            self.handle.L.eagle_post_free(self._t)
            self._t = C.c_void_p()

    def __del__(self):
        try:
            if self._t and self.handle._h:
                self.handle.L.eagle_post_free(self._t)
        except Exception:
            pass


def comm_unique_id():
    buf = C.create_string_buffer(128)
    rc = load().eagle_comm_id(buf)
    if rc:
        raise EagleError(f"eagle_comm_id failed ({rc}): {load().eagle_last_error(None).decode()}")
    return buf.raw


# --- operator-level wrappers (parity tests) -------------------------------------------------------------------
def op_conv2d(x, w_hwio, bias, stride=1, pre=0, r1=None, r2=None, post=0, precision=PREC_F32, device=0):
    L = load()
    x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w_hwio, np.float32); b = np.ascontiguousarray(bias, np.float32)
    n, h, wd, cin = x.shape
    ks, _, _, cout = w.shape
    ho = (h + 2 * (ks // 2) - ks) // stride + 1
    wo = (wd + 2 * (ks // 2) - ks) // stride + 1
    y = np.empty((n, ho, wo, cout), np.float32)
    r1 = None if r1 is None else np.ascontiguousarray(r1, np.float32)
    r2 = None if r2 is None else np.ascontiguousarray(r2, np.float32)
    rc = L.eagle_op_conv2d(device, precision, _fp(x), n, h, wd, cin, _fp(w), _fp(b), cout, ks, stride, pre, _fp(r1), _fp(r2), post, _fp(y))
    if rc:
        raise EagleError(f"eagle_op_conv2d failed ({rc}): {L.eagle_last_error(None).decode()}")
    return y


def op_bottleneck(x, w1, b1, w2, b2, w3, b3, res=None, reps=0, device=0, wd=None, bd=None):
    """One fused Bottleneck launch of the split family (include/eagle.h eagle_op_bottleneck; csrc/bneck.hip).  Returns y, or (y, ms per launch) when reps > 0."""
    L = load()
    x = np.ascontiguousarray(x, np.float32)
    n, h, w, cin = x.shape
    arrs = [np.ascontiguousarray(a, np.float32) for a in (w1, b1, w2, b2, w3, b3)]
    assert arrs[0].shape == (1, 1, cin, 64) and arrs[2].shape == (3, 3, 64, 64) and arrs[4].shape == (1, 1, 64, 256), "HWIO weights of a 64-wide Bottleneck"
    res = None if res is None else np.ascontiguousarray(res, np.float32)
    y = np.empty((n, h, w, 256), np.float32)
    ms = C.c_float(0)
    wd = None if wd is None else np.ascontiguousarray(wd, np.float32)      # the 1x1 downsample branch [1][1][64][256] computed inside the launch (block 0)
    bd = None if bd is None else np.ascontiguousarray(bd, np.float32)
    rc = L.eagle_op_bottleneck(device, _fp(x), n, h, w, cin, *[_fp(a) for a in arrs], _fp(res), _fp(y), int(reps), C.byref(ms), _fp(wd), _fp(bd))
    if rc:
        raise EagleError(f"eagle_op_bottleneck failed ({rc}): {L.eagle_last_error(None).decode()}")
    return (y, ms.value) if reps > 0 else y


def op_stem(frames, w1, b1, out_hw=(540, 960), device=0):
    """The fused input launch of HRNet in the split family (include/eagle.h eagle_op_stem; csrc/stem.hip): BGR u8 frames [n, h, w, 3] -> relu(conv1(normalise(resize)))
    [n, ho, wo, 64].  Returns (y, sat): sat[i] = lanes of frame i that stored a value beyond the split format's range."""
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    w1 = np.ascontiguousarray(w1, np.float32); b1 = np.ascontiguousarray(b1, np.float32)
    assert w1.shape == (3, 3, 3, 64) and b1.shape == (64,), "HWIO weights of HRNet's conv1"
    dh, dw = out_hw
    y = np.empty((n, (dh - 1) // 2 + 1, (dw - 1) // 2 + 1, 64), np.float32)
    sat = np.zeros(n, np.uint32)
    rc = L.eagle_op_stem(device, frames.ctypes.data_as(C.POINTER(C.c_uint8)), n, h, w, dh, dw, _fp(w1), _fp(b1), _fp(y), sat.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc:
        raise EagleError(f"eagle_op_stem failed ({rc}): {L.eagle_last_error(None).decode()}")
    return y, sat


def op_fuse_sum(base, ups, relu=True, precision=PREC_F32, device=0):
    L = load()
    base = np.ascontiguousarray(base, np.float32)
    n, H, W, c = base.shape
    ups = [np.ascontiguousarray(u, np.float32) for u in ups]
    arr = (C.POINTER(C.c_float) * max(len(ups), 1))(*[_fp(u) for u in ups])
    uh = (C.c_int * max(len(ups), 1))(*[u.shape[1] for u in ups])
    uw = (C.c_int * max(len(ups), 1))(*[u.shape[2] for u in ups])
    y = np.empty_like(base)
    rc = L.eagle_op_fuse_sum(device, precision, _fp(base), n, H, W, c, len(ups), arr, uh, uw, int(relu), _fp(y))
    if rc:
        raise EagleError(f"eagle_op_fuse_sum failed ({rc}): {L.eagle_last_error(None).decode()}")
    return y


def op_preprocess(frames, det_imgsz=640, precision=PREC_F32, device=0, letterbox=0):
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    hw = (C.c_int * 2)()
    rc = L.eagle_op_preprocess_lb(device, precision, frames.ctypes.data_as(C.POINTER(C.c_uint8)), n, h, w, det_imgsz, int(letterbox), None, None, hw)
    if rc:
        raise EagleError(f"eagle_op_preprocess failed ({rc}): {L.eagle_last_error(None).decode()}")
    kp = np.empty((n, 540, 960, 3), np.float32)
    det = np.empty((n, hw[0], hw[1], 3), np.float32)
    rc = L.eagle_op_preprocess_lb(device, precision, frames.ctypes.data_as(C.POINTER(C.c_uint8)), n, h, w, det_imgsz, int(letterbox), _fp(kp), _fp(det), hw)
    if rc:
        raise EagleError(f"eagle_op_preprocess failed ({rc}): {L.eagle_last_error(None).decode()}")
    return kp, det


def op_find_homography(img_pts, world_pts, thresh=5.0, max_iters=2000, lm_iters=10, device=0):
    L = load()
    a = np.ascontiguousarray(img_pts, np.float32).reshape(-1, 2)
    b = np.ascontiguousarray(world_pts, np.float32).reshape(-1, 2)
    n = len(a)
    H = np.zeros(9, np.float64); mask = np.zeros(max(n, 1), np.uint8); ok = C.c_int(0)
    rc = L.eagle_op_find_homography(device, _fp(a), _fp(b), n, thresh, max_iters, lm_iters,
                                    H.ctypes.data_as(C.POINTER(C.c_double)), mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(ok))
    if rc:
        raise EagleError(f"eagle_op_find_homography failed ({rc}): {L.eagle_last_error(None).decode()}")
    return (H.reshape(3, 3), mask[:n]) if ok.value else (None, None)


PART_DTYPE = np.dtype([("score", "<f4"), ("idx", "<i4")], align=True)      # include/eagle.h EagleArgmaxPart


def op_detect_tail(levels, nc, in_hw, frame_hw, conf_floor=0.15, nms_iou=0.7, detector_conf=0.35, device=0):
    """yolo_decode_kernel + nms_kernel on chosen head tensors (include/eagle.h eagle_op_detect_tail; csrc/detect.hip).  levels: [(box [n, gh, gw, 64],
    cls [n, gh, gw, nc], stride)], 1 to 3 of them -> (records RESULT_DTYPE [n] with n_det / n_candidates / det written, boxes [n, A, 4], conf [n, A], cls [n, A])."""
    L = load()
    nl = len(levels)
    box = [np.ascontiguousarray(b, np.float32) for b, _, _ in levels]
    cls = [np.ascontiguousarray(c, np.float32) for _, c, _ in levels]
    n = box[0].shape[0]
    for b, c in zip(box, cls):
        assert b.ndim == 4 and b.shape[0] == n and b.shape[3] == 64 and c.shape == b.shape[:3] + (nc,), (b.shape, c.shape)
    gh = (C.c_int * nl)(*[b.shape[1] for b in box]); gw = (C.c_int * nl)(*[b.shape[2] for b in box])
    st = (C.c_float * nl)(*[float(s) for _, _, s in levels])
    bp = (C.POINTER(C.c_float) * nl)(*[_fp(b) for b in box]); cp = (C.POINTER(C.c_float) * nl)(*[_fp(c) for c in cls])
    A = sum(b.shape[1] * b.shape[2] for b in box)
    out = np.zeros(n, RESULT_DTYPE)
    boxes = np.zeros((n, A, 4), np.float32); conf = np.zeros((n, A), np.float32); cl = np.zeros((n, A), np.int32)
    rc = L.eagle_op_detect_tail(device, nl, gh, gw, st, bp, cp, n, nc, conf_floor, nms_iou, detector_conf, frame_hw[0], frame_hw[1], in_hw[0], in_hw[1],
                                out.ctypes.data_as(C.c_void_p), _fp(boxes), _fp(conf), cl.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc:
        raise EagleError(f"eagle_op_detect_tail failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out, boxes, conf, cl


def op_post(hm_hw, frame_hw, logits=None, chunks=64, parts=None, recs=None, keypoint_conf=0.3, ransac_thresh=5.0, ransac_max_iters=2000, lm_iters=10, device=0):
    """post_kernel on chosen inputs (include/eagle.h eagle_op_post; csrc/geom.hip): logits [n, h, w, 64] (heat_argmax_kernel makes ``chunks`` partials first)
    or parts PART_DTYPE [n, chunks, 64]; recs: optional RESULT_DTYPE [n] with n_det and det foot points filled in -> (records, the partials that were reduced)."""
    L = load()
    if logits is not None:
        logits = np.ascontiguousarray(logits, np.float32)
        n = logits.shape[0]
        assert logits.shape == (n, hm_hw[0], hm_hw[1], 64), logits.shape
    else:
        parts = np.ascontiguousarray(parts, PART_DTYPE)
        n, chunks = parts.shape[0], parts.shape[1]
        assert parts.shape == (n, chunks, 64), parts.shape
    out = np.zeros(n, RESULT_DTYPE) if recs is None else np.ascontiguousarray(recs, RESULT_DTYPE).copy()
    assert len(out) == n
    pout = np.zeros((n, chunks, 64), PART_DTYPE)
    rc = L.eagle_op_post(device, n, hm_hw[0], hm_hw[1], chunks, _fp(logits), None if parts is None else parts.ctypes.data_as(C.c_void_p),
                         pout.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), frame_hw[0], frame_hw[1], keypoint_conf, ransac_thresh, ransac_max_iters, lm_iters)
    if rc:
        raise EagleError(f"eagle_op_post failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out, pout


def conv2d_argmax_tiles(hw, cin, cout, ks=1, stride=1, precision=PREC_F32S):
    """(tiles per frame, tile_h, tile_w) of the head-convolution configuration op_conv2d_argmax runs for this shape (no GPU involved)."""
    L = load()
    tiles, th, tw = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = L.eagle_op_conv2d_argmax(0, precision, None, 1, hw[0], hw[1], cin, None, None, cout, ks, stride, None, None, C.byref(tiles), C.byref(th), C.byref(tw))
    if rc:
        raise EagleError(f"eagle_op_conv2d_argmax failed ({rc}): {L.eagle_last_error(None).decode()}")
    return tiles.value, th.value, tw.value


CONV_CONFIG_FIELDS = ("kc", "nt", "wx", "variant", "tile_h", "tile_w", "lds_bytes", "supported")
CONV_TABLES = {"instances": (0, ("prec", "ks", "stride", "kc", "nt", "variant")),
               "adirect": (1, ("prec", "variant", "stride", "kc", "nt", "tile_h", "tile_w", "lds_bytes")),
               "tuned_f16": (2, ("ks", "stride", "cin", "cout", "wo", "kc", "nt", "wx", "variant")),
               "tuned_f32": (3, ("ks", "stride", "cin", "cout", "wo", "kc", "nt", "wx", "variant")),
               "tuned_split": (4, ("ks", "stride", "cin", "cout", "wo", "kc", "nt", "wx", "variant"))}      # include/eagle.h EAGLE_CONV_TABLE_*


def conv_config(precision, ks, stride, cin, cout, wo, plain_epilogue=False, second_residual=False):
    """The configuration op_conv2d runs for a layer of real channel counts cin / cout on an output map wo columns wide, as a dict of CONV_CONFIG_FIELDS
    (include/eagle.h eagle_op_conv_config; no GPU involved).  EAGLE_CONV_FORCE / EAGLE_F32_FORCE are read from the environment as on every call."""
    L = load()
    out = (C.c_int32 * 8)()
    rc = L.eagle_op_conv_config(precision, ks, stride, cin, cout, wo, int(bool(plain_epilogue)), int(bool(second_residual)), out)
    if rc:
        raise EagleError(f"eagle_op_conv_config failed ({rc}): {L.eagle_last_error(None).decode()}")
    return dict(zip(CONV_CONFIG_FIELDS, (int(v) for v in out)))


def conv_table(which):
    """One of the tables the convolution choice is made from, as a list of tuples in CONV_TABLES[which][1]'s field order (eagle_op_conv_table; no GPU involved)."""
    L = load()
    code, fields = CONV_TABLES[which]
    n = L.eagle_op_conv_table(code, None, 0)
    if n < 0:
        raise EagleError(f"eagle_op_conv_table failed ({n}): {L.eagle_last_error(None).decode()}")
    buf = (C.c_int32 * (n * len(fields)))()
    assert L.eagle_op_conv_table(code, buf, len(buf)) == n
    return [tuple(int(v) for v in buf[k * len(fields):(k + 1) * len(fields)]) for k in range(n)]


def op_conv2d_argmax(x, w_hwio, bias, stride=1, precision=PREC_F32S, device=0):
    """The head convolution twice (include/eagle.h eagle_op_conv2d_argmax): -> (fp32 logits [n, ho, wo, cout], partials PART_DTYPE [n, tiles, cout_pad] of the fused
    arg-max epilogue, (tile_h, tile_w)); tiles are numbered row-major, ceil(wo / tile_w) per row."""
    L = load()
    x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w_hwio, np.float32); b = np.ascontiguousarray(bias, np.float32)
    n, h, wd, cin = x.shape
    ks, _, _, cout = w.shape
    ho = (h + 2 * (ks // 2) - ks) // stride + 1
    wo = (wd + 2 * (ks // 2) - ks) // stride + 1
    tiles, th, tw = C.c_int(0), C.c_int(0), C.c_int(0)
    args = (device, precision, _fp(x), n, h, wd, cin, _fp(w), _fp(b), cout, ks, stride)
    rc = L.eagle_op_conv2d_argmax(*args, None, None, C.byref(tiles), C.byref(th), C.byref(tw))
    if rc:
        raise EagleError(f"eagle_op_conv2d_argmax failed ({rc}): {L.eagle_last_error(None).decode()}")
    y = np.empty((n, ho, wo, cout), np.float32)
    parts = np.zeros((n, tiles.value, (cout + 15) // 16 * 16), PART_DTYPE)
    rc = L.eagle_op_conv2d_argmax(*args, _fp(y), parts.ctypes.data_as(C.c_void_p), C.byref(tiles), C.byref(th), C.byref(tw))
    if rc:
        raise EagleError(f"eagle_op_conv2d_argmax failed ({rc}): {L.eagle_last_error(None).decode()}")
    return y, parts, (th.value, tw.value)


# --- decoder-native input helpers -------------------------------------------------------------------------------
def _pix(fmt):
    if isinstance(fmt, str):
        if fmt.lower() not in PIX_FORMATS:
            raise EagleError(f"unknown pixel format {fmt!r} (nv12 or i420)")
        return PIX_FORMATS[fmt.lower()]
    return int(fmt)                          # an integer goes to the library as it is (which rejects unknown codes)


def _yuv_layout(layout):
    if layout is None or isinstance(layout, EagleYuvLayout):
        return layout
    lay = EagleYuvLayout()
    for k, v in dict(layout).items():
        if k not in dict(EagleYuvLayout._fields_):
            raise TypeError(f"unknown layout field {k}")
        setattr(lay, k, int(v))
    return lay


def yuv_span(fmt, h, w, layout, n):
    """Bytes that n frames of this layout span in the caller's buffer: (n - 1) * frame_stride + the last frame's extent, with the dense defaults of
    include/eagle.h for zero fields (the buffer-size check of the flat-buffer form; the layout itself is checked by the library)."""
    lay = _yuv_layout(layout) or EagleYuvLayout()
    nv12 = _pix(fmt) == PIX_FORMATS["nv12"]
    c_row = w if nv12 else w // 2
    yp = lay.y_pitch or w
    co = lay.c_offset or yp * h
    cp = lay.c_pitch or c_row
    planes = [(0, yp, h, w), (co, cp, h // 2, c_row)]
    if not nv12:
        planes.append((lay.v_offset or co + cp * (h // 2), cp, h // 2, c_row))
    extent = max(o + p * (r - 1) + b for o, p, r, b in planes)
    stride = lay.frame_stride or max(o + p * r for o, p, r, _ in planes)
    return 0 if n <= 0 else (n - 1) * stride + extent


def op_yuv_to_bgr(frames, fmt="nv12", layout=None, h=None, w=None, n=None, device=0):
    """One yuv_to_bgr launch on host buffers (include/eagle.h eagle_op_yuv_to_bgr): uint8 [n, 3h/2, w] / [3h/2, w], or a flat buffer with layout,
    h, w and n -> BGR uint8 [n, h, w, 3]."""
    L = load()
    a = np.asarray(frames)
    if a.ndim in (2, 3):
        if a.ndim == 2:
            a = a[None]
        n, h, w = a.shape[0], a.shape[1] * 2 // 3, a.shape[2]
    elif h is None or w is None or n is None:
        raise EagleError("a flat 4:2:0 buffer needs h, w and n")
    a = np.ascontiguousarray(a, np.uint8)
    lay = _yuv_layout(layout)
    if a.ndim == 1 and a.nbytes < yuv_span(fmt, h, w, lay, n):
        raise EagleError(f"the buffer holds {a.nbytes} bytes, {n} frames of this layout span {yuv_span(fmt, h, w, lay, n)}")
    out = np.empty((n, h, w, 3), np.uint8)
    rc = L.eagle_op_yuv_to_bgr(device, _pix(fmt), a.ctypes.data_as(C.POINTER(C.c_uint8)), n, h, w, None if lay is None else C.byref(lay),
                               out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc:
        raise EagleError(f"eagle_op_yuv_to_bgr failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out


# --- annotated output helpers -----------------------------------------------------------------------------------
def _out_pix(fmt):
    if isinstance(fmt, str):
        if fmt.lower() not in OUT_FORMATS:
            raise EagleError(f"unknown output pixel format {fmt!r} (bgr, nv12 or i420)")
        return OUT_FORMATS[fmt.lower()]
    return int(fmt)


def _team_arrays(team_mapping):
    if team_mapping is None:
        return None, None, 0
    ids = np.ascontiguousarray([int(k) for k in team_mapping], np.int32)
    vals = np.ascontiguousarray([int(v) for v in team_mapping.values()], np.int32)
    return ids, vals, len(ids)


def _annot_args(recs, n, team_mapping):
    recs = np.ascontiguousarray(recs, RESULT_DTYPE).reshape(-1)
    if len(recs) < n:
        raise EagleError(f"{n} frames but {len(recs)} records")
    return (recs,) + _team_arrays(team_mapping)


def out_span(fmt, h, w, layout, n):
    """Bytes n annotated frames of this output format and layout span (0 fields: the dense defaults of include/eagle.h)."""
    if _out_pix(fmt) != 0:
        return yuv_span(_out_pix(fmt), h, w, layout, n)
    lay = _yuv_layout(layout) or EagleYuvLayout()
    pitch = lay.y_pitch or 3 * w
    return 0 if n <= 0 else (n - 1) * (lay.frame_stride or pitch * h) + pitch * (h - 1) + 3 * w


def overlay_from_record(rec, team_mapping=None):
    """The primitive list the library draws for one record (include/eagle.h eagle_overlay_from_record; no GPU involved) -> PRIM_DTYPE array."""
    rec = np.ascontiguousarray(rec, RESULT_DTYPE).reshape(-1)[:1]
    ids, vals, nt = _team_arrays(team_mapping)
    out = np.zeros(MAX_PRIMS, PRIM_DTYPE); n = C.c_int(0)
    L = load()
    rc = L.eagle_overlay_from_record(rec.ctypes.data_as(C.c_void_p), None if ids is None else ids.ctypes.data_as(C.c_void_p),
                                     None if vals is None else vals.ctypes.data_as(C.c_void_p), nt, out.ctypes.data_as(C.c_void_p), MAX_PRIMS, C.byref(n))
    if rc:
        raise EagleError(f"eagle_overlay_from_record failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out[: n.value].copy()


def op_annotate(frames, prims, offsets, fmt="bgr", layout=None, out=None, device=0):
    """One annotate launch on host buffers (include/eagle.h eagle_op_annotate): BGR uint8 [n, h, w, 3], a PRIM_DTYPE array and n + 1 offsets into it
    -> the annotated frames: [n, h, w, 3] / [n, 3h/2, w] when dense, else the flat buffer ``out`` (or a zeroed one) written in ``layout``."""
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    prims = np.ascontiguousarray(prims, PRIM_DTYPE)
    offsets = np.ascontiguousarray(offsets, np.int32)
    if len(offsets) != n + 1 or (n and int(offsets[-1]) > len(prims)):
        raise EagleError("op_annotate: offsets must have n + 1 entries inside the primitive array")
    lay = _yuv_layout(layout)
    need = out_span(fmt, h, w, lay, n) if _out_pix(fmt) == 0 or (h % 2 == 0 and w % 2 == 0) else 0      # (odd 4:2:0 sizes: the library rejects them)
    if out is None:
        out = np.zeros(need, np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
        raise EagleError(f"op_annotate: out must be a contiguous uint8 array of at least {need} bytes")
    rc = L.eagle_op_annotate(device, frames.ctypes.data_as(C.POINTER(C.c_uint8)), n, h, w, prims.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p),
                             _out_pix(fmt), None if lay is None else C.byref(lay), out.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc:
        raise EagleError(f"eagle_op_annotate failed ({rc}): {L.eagle_last_error(None).decode()}")
    if lay is None:
        return out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
    return out


# --- the minimap ------------------------------------------------------------------------------------------------
def minimap_params(scale=8, margin=None, voronoi=False, footprint=True, player_radius=0, ball_radius=0, control=False, layers=0):
    """EagleMinimapParams; margin None: two metres' worth of pixels, at most 64.  control: the pitch-control layer (Handle.minimap_set_control /
    op_minimap_control say with which parameters).  layers: MM_TRAILS | MM_PASSES | MM_OWNER (Handle.minimap_set_trails / op_minimap_trails) | MM_HULLS
    (Handle.team_shape and Handle.set_hulls / op_minimap_hulls)."""
    if margin is None:
        margin = min(64, 2 * int(scale))
    return EagleMinimapParams(int(scale), int(margin), int(bool(voronoi)), int(bool(footprint)), int(player_radius), int(ball_radius), int(bool(control)), int(layers))


def minimap_size(params):
    """(w, h) of the pictures these parameters give (include/eagle.h eagle_minimap_size; no GPU involved)."""
    w, h = C.c_int(0), C.c_int(0)
    L = load()
    rc = L.eagle_minimap_size(C.byref(params), C.byref(w), C.byref(h))
    if rc:
        raise EagleError(f"eagle_minimap_size failed ({rc}): {L.eagle_last_error(None).decode()}")
    return w.value, h.value


def op_minimap(values, columns, team_mapping, params, row0=0, n=None, fmt="bgr", layout=None, out=None, device=0):
    """The two minimap launches on a constructed table (include/eagle.h eagle_op_minimap): values float64 [cols][rows][2], columns POSTCOL_DTYPE (or
    (kind, id, video) tuples), team_mapping {id: team} or None -> the pictures: [n, h, w, 3] / [n, 3h/2, w] when dense, else the flat buffer ``out``
    (or a zeroed one) written in ``layout``."""
    L = load()
    values = np.ascontiguousarray(values, np.float64)
    cols, rows = values.shape[0], values.shape[1]
    if not (isinstance(columns, np.ndarray) and columns.dtype == POSTCOL_DTYPE):
        columns = np.array([(k, i, v, 0) for k, i, v in columns], POSTCOL_DTYPE)
    columns = np.ascontiguousarray(columns)
    if len(columns) != cols or values.shape[2:] != (2,):
        raise EagleError("op_minimap: values must be [cols][rows][2] with one column descriptor per column")
    ids, vals, nt = _team_arrays(team_mapping)
    n = rows - row0 if n is None else n
    w, h = minimap_size(params)
    lay = _yuv_layout(layout)
    need = out_span(fmt, h, w, lay, n)
    if out is None:
        out = np.zeros(need, np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
        raise EagleError(f"op_minimap: out must be a contiguous uint8 array of at least {need} bytes")
    keep = np.zeros(4, np.float64)                       # (a table without cells still hands the library a valid pointer)
    rc = L.eagle_op_minimap(device, (values if values.size else keep).ctypes.data_as(C.c_void_p), (columns if len(columns) else keep).ctypes.data_as(C.c_void_p), rows, cols,
                            None if ids is None else (ids if len(ids) else keep).ctypes.data_as(C.c_void_p), None if vals is None else (vals if len(vals) else keep).ctypes.data_as(C.c_void_p),
                            nt, C.byref(params), int(row0), int(n), _out_pix(fmt), None if lay is None else C.byref(lay), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise EagleError(f"eagle_op_minimap failed ({rc}): {L.eagle_last_error(None).decode()}")
    if lay is None:
        return out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
    return out


# --- kinematics and pitch control ---------------------------------------------------------------------------------
def kinematics_params(fps, max_gap=None, speed_cap=12.0):
    """EagleKinematicsParams; max_gap None: fps frames (a neighbour row more than a second away is not differenced)."""
    return EagleKinematicsParams(int(fps), int(fps if max_gap is None else max_gap), float(speed_cap), 0)


def control_params(cells_per_metre=1, t_react=0.7, v_max=5.0, beta=4.0):
    """EagleControlParams: the conventional constants of the time-to-intercept model (not fitted to data)."""
    return EagleControlParams(int(cells_per_metre), float(t_react), float(v_max), float(beta))


def control_size(params):
    """(gw, gh) of the grids these parameters give (include/eagle.h eagle_control_size; no GPU involved)."""
    gw, gh = C.c_int(0), C.c_int(0)
    L = load()
    rc = L.eagle_control_size(C.byref(params), C.byref(gw), C.byref(gh))
    if rc:
        raise EagleError(f"eagle_control_size failed ({rc}): {L.eagle_last_error(None).decode()}")
    return gw.value, gh.value


def possession_params(fps, radius=2.0, min_hold=2, max_gap=None):
    """EaglePossessionParams; max_gap None: fps frames.  2 m, 2 rows and one second are conventional choices, not fitted to data."""
    return EaglePossessionParams(int(fps), int(min_hold), int(fps if max_gap is None else max_gap), 0, float(radius), 0)


def pass_option_params(cells_per_metre=1, samples=16, t_react=0.7, v_max=5.0, beta=4.0, v_ball=15.0):
    """EaglePassOptionParams; 16 samples, 0.7 s, 5 m/s, 4 / s and a 15 m/s ball are conventional choices, not fitted to data."""
    return EaglePassOptionParams(int(cells_per_metre), int(samples), float(t_react), float(v_max), float(beta), float(v_ball))


def pass_options_size(params):
    """(gw, gh) of the grids these parameters give (include/eagle.h eagle_pass_options_size; no GPU involved)."""
    gw, gh = C.c_int(0), C.c_int(0)
    L = load()
    rc = L.eagle_pass_options_size(C.byref(params), C.byref(gw), C.byref(gh))
    if rc:
        raise EagleError(f"eagle_pass_options_size failed ({rc}): {L.eagle_last_error(None).decode()}")
    return gw.value, gh.value


def load_params(fps, max_gap=None, zone_edges=(2.0, 4.0, 5.5, 7.0), effort_speed=(5.5, 7.0), accel=2.0, min_frames=None):
    """EagleLoadParams; max_gap None: fps frames; min_frames None: max(1, fps // 2) for both durations (one int: both).  The edges (m/s), the speeds a
    high-speed run and a sprint start at, 2 m/s^2 and half a second are conventional choices, not fitted to data."""
    if min_frames is None:
        min_frames = max(1, int(fps) // 2)
    mf = (int(min_frames),) * 2 if np.isscalar(min_frames) else tuple(int(m) for m in min_frames)
    if len(mf) != 2 or len(zone_edges) != 4 or len(effort_speed) != 2:
        raise EagleError("load_params: two min_frames, four zone_edges and two effort_speed values")
    return EagleLoadParams(int(fps), int(fps if max_gap is None else max_gap), (C.c_int32 * 2)(*mf), (C.c_double * 4)(*[float(x) for x in zone_edges]),
                           (C.c_double * 2)(*[float(x) for x in effort_speed]), float(accel), (C.c_int64 * 2)(0, 0))


def occupancy_params(fps, cells_per_metre=1, sigma=2.0, max_gap=None):
    """EagleOccupancyParams; max_gap None: fps frames.  The 2 m sigma is a conventional choice, not fitted to data."""
    return EagleOccupancyParams(int(fps), int(fps if max_gap is None else max_gap), int(cells_per_metre), 0, float(sigma), 0)


def occupancy_size(params):
    """(gw, gh) of the maps these parameters give (include/eagle.h eagle_occupancy_size; no GPU involved)."""
    gw, gh = C.c_int(0), C.c_int(0)
    L = load()
    rc = L.eagle_occupancy_size(C.byref(params), C.byref(gw), C.byref(gh))
    if rc:
        raise EagleError(f"eagle_occupancy_size failed ({rc}): {L.eagle_last_error(None).decode()}")
    return gw.value, gh.value


def _bgr(colour):
    b, g, r = (int(v) & 255 for v in colour)
    return b | g << 8 | r << 16


def _table_args(what, values, columns):
    values = np.ascontiguousarray(values, np.float64)
    if not (isinstance(columns, np.ndarray) and columns.dtype == POSTCOL_DTYPE):
        columns = np.array([(k, i, v, 0) for k, i, v in columns], POSTCOL_DTYPE)
    columns = np.ascontiguousarray(columns)
    if values.ndim != 3 or len(columns) != values.shape[0] or values.shape[2] != 2:
        raise EagleError(f"{what}: values must be [cols][rows][2] with one column descriptor per column")
    return values, columns


def _ptr(a, keep):
    return None if a is None else (a if a.size else keep).ctypes.data_as(C.c_void_p)


def op_velocities(values, frames, params, device=0):
    """post_velocity_kernel on a constructed table (include/eagle.h eagle_op_velocities): values float64 [cols][rows][2], frames int32 [rows]
    ascending, params EagleKinematicsParams -> float64 [cols][rows][2]."""
    L = load()
    values = np.ascontiguousarray(values, np.float64)
    frames = np.ascontiguousarray(frames, np.int32)
    if values.ndim != 3 or values.shape[2] != 2 or len(frames) != values.shape[1]:
        raise EagleError("op_velocities: values must be [cols][rows][2] with one frame number per row")
    out = np.zeros(values.shape, np.float64)
    keep = np.zeros(4, np.float64)
    rc = L.eagle_op_velocities(device, _ptr(values, keep), _ptr(frames, keep), values.shape[1], values.shape[0], C.byref(params), _ptr(out, keep))
    if rc:
        raise EagleError(f"eagle_op_velocities failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out


def op_control(values, velocities, columns, team_mapping, params, row0=0, n=None, device=0):
    """The two control launches on a constructed table (include/eagle.h eagle_op_control) -> (uint8 [n, gh, gw], int64 [n] byte sums)."""
    L = load()
    values, columns = _table_args("op_control", values, columns)
    velocities = np.ascontiguousarray(velocities, np.float64)
    if velocities.shape != values.shape:
        raise EagleError("op_control: velocities must have the shape of values")
    cols, rows = values.shape[:2]
    ids, vals, nt = _team_arrays(team_mapping)
    n = rows - row0 if n is None else n
    gw, gh = control_size(params)
    out, share = np.zeros((max(n, 0), gh, gw), np.uint8), np.zeros(max(n, 0), np.int64)
    keep = np.zeros(4, np.float64)
    rc = L.eagle_op_control(device, _ptr(values, keep), _ptr(velocities, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt, C.byref(params),
                            int(row0), int(n), _ptr(out, keep), _ptr(share, keep))
    if rc:
        raise EagleError(f"eagle_op_control failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out, share


def op_possession(values, frames, columns, team_mapping, params, cap=None, device=0):
    """The possession launches on a constructed table (include/eagle.h eagle_op_possession): values float64 [cols][rows][2], frames int32 [rows]
    strictly ascending, columns POSTCOL_DTYPE (or (kind, id, video) tuples), team_mapping {id: team} or None -> (cand, owner, dist, events, n_events);
    cap None: every event is fetched, else at most cap of the n_events."""
    L = load()
    values, columns = _table_args("op_possession", values, columns)
    frames = np.ascontiguousarray(frames, np.int32)
    cols, rows = values.shape[:2]
    if len(frames) != rows:
        raise EagleError("op_possession: one frame number per row")
    ids, vals, nt = _team_arrays(team_mapping)
    cand, owner, dist = np.zeros(rows, np.int32), np.zeros(rows, np.int32), np.zeros(rows, np.float64)
    ev = np.zeros(max(rows - 1, 0) if cap is None else int(cap), EVENT_DTYPE)
    keep = np.zeros(4, np.float64)
    n = C.c_int(0)
    rc = L.eagle_op_possession(device, _ptr(values, keep), _ptr(frames, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt, C.byref(params),
                               _ptr(cand, keep), _ptr(owner, keep), _ptr(dist, keep), _ptr(ev, keep), len(ev), C.byref(n))
    if rc:
        raise EagleError(f"eagle_op_possession failed ({rc}): {L.eagle_last_error(None).decode()}")
    return cand, owner, dist, ev[: min(n.value, len(ev))].copy(), n.value


def pass_site_columns(columns, team_mapping):
    """The site columns of a table as include/eagle.h states them: Player pitch columns whose mapping entry is >= 0, in table order."""
    if not (isinstance(columns, np.ndarray) and columns.dtype == POSTCOL_DTYPE):
        columns = np.array([(k, i, v, 0) for k, i, v in columns], POSTCOL_DTYPE)
    tm = {} if team_mapping is None else {int(k): int(v) for k, v in team_mapping.items()}
    return np.array([c for c, col in enumerate(columns) if col["kind"] == POST_PLAYER and not col["video"] and tm.get(int(col["id"]), -1) >= 0], np.int32)


def op_pass_options(values, velocities, columns, team_mapping, cand, owner, params, row0=0, n=None, grids=True, options=True, device=0):
    """The pass-option launches on a constructed table (include/eagle.h eagle_op_pass_options): cand / owner int32 [rows] as op_possession gives them
    -> (grids uint8 [n, gh, gw] or None, records PASS_ROW_DTYPE [n], options int16 [n, n_sites] or None)."""
    L = load()
    values, columns = _table_args("op_pass_options", values, columns)
    velocities = np.ascontiguousarray(velocities, np.float64)
    cand, owner = np.ascontiguousarray(cand, np.int32), np.ascontiguousarray(owner, np.int32)
    cols, rows = values.shape[:2]
    if velocities.shape != values.shape or cand.shape != (rows,) or owner.shape != (rows,):
        raise EagleError("op_pass_options: velocities must have the shape of values, cand and owner one entry per row")
    ids, vals, nt = _team_arrays(team_mapping)
    n = rows - row0 if n is None else n
    gw, gh = pass_options_size(params)
    ns = len(pass_site_columns(columns, team_mapping)) if options else 0
    g = np.zeros((max(n, 0), gh, gw), np.uint8) if grids else None
    recs = np.zeros(max(n, 0), PASS_ROW_DTYPE)
    opt = np.zeros((max(n, 0), ns), np.int16) if options else None
    keep = np.zeros(8, np.float64)
    rc = L.eagle_op_pass_options(device, _ptr(values, keep), _ptr(velocities, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt,
                                 _ptr(cand, keep), _ptr(owner, keep), C.byref(params), int(row0), int(n), _ptr(g, keep), _ptr(recs, keep), _ptr(opt, keep))
    if rc:
        raise EagleError(f"eagle_op_pass_options failed ({rc}): {L.eagle_last_error(None).decode()}")
    return g, recs, opt


def smooth_params(fps, window=None, degree=2, outlier_k=4.0, outlier_floor=0.25, ball_window=0, max_gap=None, speed_cap=12.0):
    """EagleSmoothParams; window None: max(2, round(0.4 fps)) frames; max_gap None: fps frames."""
    fps = int(fps)
    return EagleSmoothParams(fps, max(2, int(round(0.4 * fps))) if window is None else int(window), int(degree), int(ball_window), int(fps if max_gap is None else max_gap),
                             0, float(outlier_k), float(outlier_floor), float(speed_cap), 0)


def op_smooth_tracks(values, frames, columns, params, device=0):
    """The smoothing launches on a constructed table (include/eagle.h eagle_op_smooth_tracks): values float64 [cols][rows][2], frames int32 [rows]
    strictly ascending, columns POSTCOL_DTYPE (or (kind, id, video) tuples) -> {"values", "vel", "acc": float64 [cols][rows][2]; "flags", "count": uint8 and
    "residual_q": int32 [cols][rows]; "suspect": uint8 [rows]; "totals": SMOOTH_TOTALS_DTYPE [cols]}."""
    L = load()
    values, columns = _table_args("op_smooth_tracks", values, columns)
    frames = np.ascontiguousarray(frames, np.int32)
    cols, rows = values.shape[:2]
    if len(frames) != rows:
        raise EagleError("op_smooth_tracks: one frame number per row")
    out = {"values": np.zeros((cols, rows, 2), np.float64), "vel": np.zeros((cols, rows, 2), np.float64), "acc": np.zeros((cols, rows, 2), np.float64),
           "flags": np.zeros((cols, rows), np.uint8), "count": np.zeros((cols, rows), np.uint8), "residual_q": np.zeros((cols, rows), np.int32),
           "suspect": np.zeros(rows, np.uint8), "totals": np.zeros(cols, SMOOTH_TOTALS_DTYPE)}
    keep = np.zeros(8, np.float64)
    rc = L.eagle_op_smooth_tracks(device, _ptr(values, keep), _ptr(frames, keep), _ptr(columns, keep), rows, cols, C.byref(params),
                                  *(_ptr(out[k], keep) for k in ("values", "vel", "acc", "flags", "count", "residual_q", "suspect", "totals")))
    if rc:
        raise EagleError(f"eagle_op_smooth_tracks failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out


def flight_params(fps, max_gap=None, max_rows=64, noise=0.25, penalty=16.0, spike=1.0, kick_dv=3.0, radius=2.0, still_speed=0.5, shot_speed=10.0, shot_range=40.0,
                  shot_margin=2.0, layout=FLIGHT_LAYOUT_DEFAULT):
    """EagleFlightParams; max_gap None: min(1024, max(1, round(fps))) frames.  The defaults are conventional choices, not fitted to data."""
    fps = float(fps)
    gap = min(1024, max(1, int(round(fps)))) if max_gap is None else int(max_gap)
    return EagleFlightParams(fps, gap, int(max_rows), float(noise), float(penalty), float(spike), float(kick_dv), float(radius), float(still_speed), float(shot_speed),
                             float(shot_range), float(shot_margin), int(layout), 0)


def op_ball_flights(values, frames, columns, params, cuts=None, times=False, device=0):
    """The ball-flight launches on a constructed table (include/eagle.h eagle_op_ball_flights): values float64 [cols][rows][2], frames int32 [rows] strictly
    ascending, columns POSTCOL_DTYPE (or (kind, id, video) tuples), cuts ascending frame numbers -> {"seg": int32 [rows], "flags": uint8 [rows], "fitted",
    "velocity": float64 [rows][2], "flights": FLIGHT_DTYPE, "kicks": KICK_DTYPE, "totals": FLIGHT_TOTALS_DTYPE [1]} and, with times, "times": a dict of
    milliseconds per FLIGHT_TIMES name."""
    L = load()
    values, columns = _table_args("op_ball_flights", values, columns)
    frames = np.ascontiguousarray(frames, np.int32)
    cuts = np.zeros(0, np.int32) if cuts is None else np.ascontiguousarray(cuts, np.int32)
    cols, rows = values.shape[:2]
    if len(frames) != rows:
        raise EagleError("op_ball_flights: one frame number per row")
    out = {"seg": np.zeros(rows, np.int32), "flags": np.zeros(rows, np.uint8), "fitted": np.zeros((rows, 2), np.float64), "velocity": np.zeros((rows, 2), np.float64),
           "flights": np.zeros(max(rows, 1), FLIGHT_DTYPE), "kicks": np.zeros(max(rows, 1), KICK_DTYPE), "totals": np.zeros(1, FLIGHT_TOTALS_DTYPE)}
    tm = np.zeros(len(FLIGHT_TIMES), np.float32)
    keep = np.zeros(8, np.float64)
    nf, nk = C.c_int(0), C.c_int(0)
    rc = L.eagle_op_ball_flights(device, _ptr(values, keep), _ptr(frames, keep), _ptr(columns, keep), rows, cols, _ptr(cuts, keep) if len(cuts) else None, len(cuts),
                                 C.byref(params), *(_ptr(out[k], keep) for k in ("seg", "flags", "fitted", "velocity")), _ptr(out["flights"], keep), len(out["flights"]),
                                 C.byref(nf), _ptr(out["kicks"], keep), len(out["kicks"]), C.byref(nk), _ptr(out["totals"], keep), tm.ctypes.data_as(C.c_void_p) if times else None)
    if rc:
        raise EagleError(f"eagle_op_ball_flights failed ({rc}): {L.eagle_last_error(None).decode()}")
    out["flights"], out["kicks"] = out["flights"][:nf.value].copy(), out["kicks"][:nk.value].copy()
    if times:
        out["times"] = dict(zip(FLIGHT_TIMES, map(float, tm)))
    return out


def stab_params(fps, window=None, degree=2, model=1, min_voters=6, iterations=2, trim_k=3.0, floor=0.1, min_spread=5.0, max_gain=0.05, jump=1.0):
    """EagleStabParams; window None: min(64, max(2, round(1.0 fps))) frames; model 0 / 1 or "translation" / "affine"."""
    fps = int(fps)
    model = {"translation": 0, "affine": 1}.get(model, model)
    return EagleStabParams(fps, min(64, max(2, int(round(1.0 * fps)))) if window is None else int(window), int(degree), int(model), int(min_voters), int(iterations),
                           (C.c_int32 * 2)(0, 0), float(trim_k), float(floor), float(min_spread), float(max_gain), float(jump), 0)


def op_stabilise(values, frames, columns, params, device=0):
    """The stabilisation launches on a constructed table (include/eagle.h eagle_op_stabilise): values float64 [cols][rows][2], frames int32 [rows]
    strictly ascending, columns POSTCOL_DTYPE (or (kind, id, video) tuples) -> {"values": float64 [cols][rows][2]; "rows": STAB_ROW_DTYPE [rows];
    "votes": int32 [cols][rows][2]; "totals": STAB_TOTALS_DTYPE [1]}."""
    L = load()
    values, columns = _table_args("op_stabilise", values, columns)
    frames = np.ascontiguousarray(frames, np.int32)
    cols, rows = values.shape[:2]
    if len(frames) != rows:
        raise EagleError("op_stabilise: one frame number per row")
    out = {"values": np.zeros((cols, rows, 2), np.float64), "rows": np.zeros(rows, STAB_ROW_DTYPE), "votes": np.zeros((cols, rows, 2), np.int32),
           "totals": np.zeros(1, STAB_TOTALS_DTYPE)}
    keep = np.zeros(8, np.float64)
    rc = L.eagle_op_stabilise(device, _ptr(values, keep), _ptr(frames, keep), _ptr(columns, keep), rows, cols, C.byref(params),
                              *(_ptr(out[k], keep) for k in ("values", "rows", "votes", "totals")))
    if rc:
        raise EagleError(f"eagle_op_stabilise failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out


def op_physical(velocities, frames, columns, params, cap=None, device=0):
    """The physical-report launches on a constructed table (include/eagle.h eagle_op_physical): velocities float64 [cols][rows][2] (NaN where a cell is
    absent), frames int32 [rows] strictly ascending, columns POSTCOL_DTYPE (or (kind, id, video) tuples) -> (speed, accel, zone: [persons, rows] each,
    totals LOAD_TOTALS_DTYPE, efforts LOAD_EFFORT_DTYPE, n_efforts); cap None: every effort is fetched, else at most cap of the n_efforts."""
    L = load()
    velocities, columns = _table_args("op_physical", velocities, columns)
    frames = np.ascontiguousarray(frames, np.int32)
    cols, rows = velocities.shape[:2]
    if len(frames) != rows:
        raise EagleError("op_physical: one frame number per row")
    persons = int(((columns["video"] == 0) & ((columns["kind"] == POST_PLAYER) | (columns["kind"] == POST_GOALKEEPER))).sum()) if rows else 0
    speed, accel, zone = np.zeros((persons, rows), np.float64), np.zeros((persons, rows), np.float64), np.zeros((persons, rows), np.uint8)
    totals = np.zeros(persons, LOAD_TOTALS_DTYPE)
    keep = np.zeros(4, np.float64)
    np_, ne = C.c_int(0), C.c_int(0)
    want = 4096 if cap is None else int(cap)
    while True:                                                        # cap None: a second call when the first guess was too small
        ev = np.zeros(want, LOAD_EFFORT_DTYPE)
        rc = L.eagle_op_physical(device, _ptr(velocities, keep), _ptr(frames, keep), _ptr(columns, keep), rows, cols, C.byref(params), _ptr(speed, keep),
                                 _ptr(accel, keep), _ptr(zone, keep), _ptr(totals, keep), len(totals), C.byref(np_), _ptr(ev, keep), len(ev), C.byref(ne))
        if rc:
            raise EagleError(f"eagle_op_physical failed ({rc}): {L.eagle_last_error(None).decode()}")
        if cap is not None or ne.value <= want:
            break
        want = ne.value
    return speed, accel, zone, totals[: np_.value].copy(), ev[: min(ne.value, len(ev))].copy(), ne.value


def op_occupancy(values, frames, columns, params, sel_off, sel_cols, device=0):
    """The occupancy launches on a constructed table (include/eagle.h eagle_op_occupancy): values float64 [cols][rows][2], frames int32 [rows]
    strictly ascending, columns POSTCOL_DTYPE (or (kind, id, video) tuples), the selections in CSR form -> (grids float32, bytes uint8, counts int32:
    [n_sel, gh, gw] each; total, outside int64 [n_sel])."""
    L = load()
    values, columns = _table_args("op_occupancy", values, columns)
    frames = np.ascontiguousarray(frames, np.int32)
    cols, rows = values.shape[:2]
    if len(frames) != rows:
        raise EagleError("op_occupancy: one frame number per row")
    sel_off, sel_cols = np.ascontiguousarray(sel_off, np.int32), np.ascontiguousarray(sel_cols, np.int32)
    n_sel = len(sel_off) - 1
    gw, gh = occupancy_size(params)
    grids, by, counts = np.zeros((n_sel, gh, gw), np.float32), np.zeros((n_sel, gh, gw), np.uint8), np.zeros((n_sel, gh, gw), np.int32)
    total, outside = np.zeros(n_sel, np.int64), np.zeros(n_sel, np.int64)
    keep = np.zeros(4, np.float64)
    rc = L.eagle_op_occupancy(device, _ptr(values, keep), _ptr(frames, keep), _ptr(columns, keep), rows, cols, C.byref(params), _ptr(sel_off, keep), _ptr(sel_cols, keep),
                              n_sel, _ptr(grids, keep), _ptr(by, keep), _ptr(total, keep), _ptr(outside, keep), _ptr(counts, keep))
    if rc:
        raise EagleError(f"eagle_op_occupancy failed ({rc}): {L.eagle_last_error(None).decode()}")
    return grids, by, counts, total, outside


def op_occupancy_picture(byte_grid, cells_per_metre, scale=8, margin=None, colour=(255, 255, 255), device=0):
    """One selection's bytes uint8 [gh, gw] -> its picture, BGR uint8 [h, w, 3] (include/eagle.h eagle_op_occupancy_picture); colour (b, g, r)."""
    L = load()
    byte_grid = np.ascontiguousarray(byte_grid, np.uint8)
    if byte_grid.shape != (68 * int(cells_per_metre), 105 * int(cells_per_metre)):
        raise EagleError("op_occupancy_picture: the bytes must be [68 R, 105 R]")
    mp = minimap_params(scale, margin)
    w, h = minimap_size(mp)
    out = np.zeros((h, w, 3), np.uint8)
    rc = L.eagle_op_occupancy_picture(device, byte_grid.ctypes.data_as(C.c_void_p), int(cells_per_metre), mp.scale, mp.margin, _bgr(colour), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise EagleError(f"eagle_op_occupancy_picture failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out


def op_minimap_control(values, velocities, columns, team_mapping, params, control, row0=0, n=None, fmt="bgr", layout=None, out=None, device=0):
    """op_minimap with the ``control`` layer drawn from given velocities (include/eagle.h eagle_op_minimap_control); params: minimap_params(...,
    control=True), control: control_params(...)."""
    L = load()
    values, columns = _table_args("op_minimap_control", values, columns)
    velocities = np.ascontiguousarray(velocities, np.float64)
    if velocities.shape != values.shape:
        raise EagleError("op_minimap_control: velocities must have the shape of values")
    cols, rows = values.shape[:2]
    ids, vals, nt = _team_arrays(team_mapping)
    n = rows - row0 if n is None else n
    w, h = minimap_size(params)
    lay = _yuv_layout(layout)
    need = out_span(fmt, h, w, lay, n)
    if out is None:
        out = np.zeros(need, np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
        raise EagleError(f"op_minimap_control: out must be a contiguous uint8 array of at least {need} bytes")
    keep = np.zeros(4, np.float64)
    rc = L.eagle_op_minimap_control(device, _ptr(values, keep), _ptr(velocities, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt,
                                    C.byref(params), C.byref(control), int(row0), int(n), _out_pix(fmt), None if lay is None else C.byref(lay), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise EagleError(f"eagle_op_minimap_control failed ({rc}): {L.eagle_last_error(None).decode()}")
    if lay is None:
        return out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
    return out


# --- the OSNet (ReID) kernels one launch at a time (include/eagle.h eagle_op_reid_*; csrc/reid.hip) ------------------------------------------
# Activations go in dense ([n, h, w, c], c the kernel's padded channel count) and are placed at channel ``off`` of a buffer with ``cs`` floats per
# pixel; outputs come back whole ([n, ho, wo, cs]) with REID_OP_SENTINEL (a quiet NaN, compare through .view(np.uint32)) wherever the kernel did not write.
REID_OP_SENTINEL = 0x7FC5E171


def _reid_check(L, rc, what):
    if rc:
        raise EagleError(f"{what} failed ({rc}): {L.eagle_last_error(None).decode()}")


def op_reid_crop(frames, crops, out_hw, y_cs=4, y_off=0, device=0):
    """reid_crop_kernel: BGR uint8 frames [nf, fh, fw, 3], crops int32 [n, 5] (frame, x1, y1, x2, y2) -> float32 [n, oh, ow, y_cs]."""
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8); crops = np.ascontiguousarray(crops, np.int32).reshape(-1, 5)
    nf, fh, fw, _ = frames.shape
    y = np.empty((len(crops), out_hw[0], out_hw[1], y_cs), np.float32)
    _reid_check(L, L.eagle_op_reid_crop(device, frames.ctypes.data_as(C.POINTER(C.c_uint8)), nf, fh, fw, crops.ctypes.data_as(C.c_void_p), len(crops), out_hw[0], out_hw[1],
                                        y_cs, y_off, _fp(y)), "eagle_op_reid_crop")
    return y


def op_reid_conv7(x, w, b, x_cs=4, x_off=0, y_cs=16, y_off=0, device=0):
    """reid_conv7_kernel: x [n, h, w, 4], w [7, 7, 3, 16] and b [16] (BatchNorm folded) -> [n, (h-1)//2+1, (w-1)//2+1, y_cs]."""
    L = load()
    x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
    n, h, wd, c = x.shape
    assert c == 4 and w.shape == (7, 7, 3, 16) and b.shape == (16,)
    y = np.empty((n, (h - 1) // 2 + 1, (wd - 1) // 2 + 1, y_cs), np.float32)
    _reid_check(L, L.eagle_op_reid_conv7(device, _fp(x), n, h, wd, x_cs, x_off, _fp(w), _fp(b), y_cs, y_off, _fp(y)), "eagle_op_reid_conv7")
    return y


def _op_reid_pool(name, x, out_hw, x_cs, x_off, y_cs, y_off, device):
    L = load()
    x = np.ascontiguousarray(x, np.float32)
    n, h, w, c = x.shape
    x_cs = c if x_cs is None else x_cs; y_cs = c if y_cs is None else y_cs
    y = np.empty((n, out_hw[0], out_hw[1], y_cs), np.float32)
    _reid_check(L, getattr(L, name)(device, _fp(x), n, h, w, c, x_cs, x_off, y_cs, y_off, _fp(y)), name)
    return y


def op_reid_maxpool3s2(x, x_cs=None, x_off=0, y_cs=None, y_off=0, device=0):
    """MaxPool2d(3, 2, 1) on x [n, h, w, c] -> [n, (h-1)//2+1, (w-1)//2+1, y_cs]."""
    return _op_reid_pool("eagle_op_reid_maxpool3s2", x, ((x.shape[1] - 1) // 2 + 1, (x.shape[2] - 1) // 2 + 1), x_cs, x_off, y_cs, y_off, device)


def op_reid_avgpool2(x, x_cs=None, x_off=0, y_cs=None, y_off=0, device=0):
    """AvgPool2d(2, 2) on x [n, h, w, c] -> [n, h//2, w//2, y_cs]; a map without a 2 x 2 window is an EagleError."""
    return _op_reid_pool("eagle_op_reid_avgpool2", x, (x.shape[1] // 2, x.shape[2] // 2), x_cs, x_off, y_cs, y_off, device)


def op_reid_dw3(x, w, b, x_cs=None, x_off=0, y_cs=None, y_off=0, device=0):
    """depthwise 3 x 3 + bias + ReLU: x [n, h, w, c], w [9, c] and b [c] (BatchNorm folded) -> [n, h, w, y_cs]."""
    L = load()
    x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
    n, h, wd, c = x.shape
    assert w.shape == (9, c) and b.shape == (c,)
    x_cs = c if x_cs is None else x_cs; y_cs = c if y_cs is None else y_cs
    y = np.empty((n, h, wd, y_cs), np.float32)
    _reid_check(L, L.eagle_op_reid_dw3(device, _fp(x), n, h, wd, c, x_cs, x_off, _fp(w), _fp(b), y_cs, y_off, _fp(y)), "eagle_op_reid_dw3")
    return y


def op_reid_gate(streams, w1, b1, w2, b2, x_cs=None, x_off=0, y_cs=None, y_off=0, device=0):
    """reid_gate_kernel + the gated four-stream sum: streams 4 x [n, h, w, c], w1 [r, c_real], b1 [r], w2 [c_real, r], b2 [c_real]
    -> (g [n, 4, c], y [n, h, w, y_cs])."""
    L = load()
    st = [np.ascontiguousarray(s, np.float32) for s in streams]
    w1, b1, w2, b2 = (np.ascontiguousarray(a, np.float32) for a in (w1, b1, w2, b2))
    n, h, wd, c = st[0].shape
    r, c_real = w1.shape
    assert len(st) == 4 and all(s.shape == st[0].shape for s in st) and b1.shape == (r,) and w2.shape == (c_real, r) and b2.shape == (c_real,)
    x_cs = c if x_cs is None else x_cs; y_cs = c if y_cs is None else y_cs
    g = np.empty((n, 4, c), np.float32); y = np.empty((n, h, wd, y_cs), np.float32)
    ptrs = (C.POINTER(C.c_float) * 4)(*[_fp(s) for s in st])
    _reid_check(L, L.eagle_op_reid_gate(device, ptrs, n, h, wd, c, x_cs, x_off, _fp(w1), _fp(b1), _fp(w2), _fp(b2), c_real, r, y_cs, y_off, _fp(g), _fp(y)), "eagle_op_reid_gate")
    return g, y


def op_reid_head(x, w, b, x_cs=None, x_off=0, device=0):
    """reid_head_kernel: x [n, h, w, c], w [dim, c] and b [dim] (BatchNorm1d folded) -> relu(mean(x) @ w.T + b) [n, dim]."""
    L = load()
    x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32); b = np.ascontiguousarray(b, np.float32)
    n, h, wd, c = x.shape
    dim = len(b)
    assert w.shape == (dim, c)
    x_cs = c if x_cs is None else x_cs
    feats = np.empty((n, dim), np.float32)
    _reid_check(L, L.eagle_op_reid_head(device, _fp(x), n, h, wd, c, x_cs, x_off, _fp(w), _fp(b), dim, _fp(feats)), "eagle_op_reid_head")
    return feats


# --- the detector's concat-by-slice path one launch at a time (include/eagle.h eagle_op_conv2d_sliced ...; csrc/nets.hip build_yolo) ---------------
# Unlike the op_reid_* wrappers these take WHOLE buffers ([n, h, w, cs] float32; the caller owns what lies outside the slices) and return the whole
# output buffer; the library converts them to and from the family's storage format, where a NaN stays a NaN but loses its payload outside fp32.
RES_OWN, RES_IN_Y, RES_IN_X = 0, 1, 2


def _whole(a):
    a = np.ascontiguousarray(a, np.float32)
    assert a.ndim == 4
    return a


def op_conv2d_sliced(x, x_off, w_hwio, bias, y, y_off, stride=1, pre=0, r1=None, r2=None, post=0, precision=PREC_F32, device=0):
    """conv_launch on slice views: channels x_off .. x_off + cin of the buffer x [n, h, w, x_cs] -> channels y_off .. y_off + cout of a copy of the buffer
    y [n, ho, wo, y_cs], which is returned whole.  r1 / r2: None, or (where, buffer, off) with where RES_OWN (cout channels at off of its own buffer
    [n, ho, wo, cs]), RES_IN_Y or RES_IN_X (at off of the output / input buffer; buffer is None)."""
    L = load()
    x = _whole(x); y = _whole(y).copy(); w = np.ascontiguousarray(w_hwio, np.float32); b = np.ascontiguousarray(bias, np.float32)
    n, h, wd, x_cs = x.shape
    ks, _, cin, cout = w.shape
    ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (wd + 2 * (ks // 2) - ks) // stride + 1
    assert y.shape[:3] == (n, ho, wo) and b.shape == (cout,)
    res = []
    for r in (r1, r2):
        where, buf, off = (RES_OWN, None, 0) if r is None else r
        buf = None if buf is None else _whole(buf)
        assert buf is None or (where == RES_OWN and buf.shape[:3] == (n, ho, wo))
        res += [buf, _fp(buf), 0 if buf is None else buf.shape[3], off, where]
    _reid_check(L, L.eagle_op_conv2d_sliced(device, precision, _fp(x), n, h, wd, cin, x_cs, x_off, _fp(w), _fp(b), cout, ks, stride, pre, *res[1:5], *res[6:10], post,
                                            y.shape[3], y_off, _fp(y)), "eagle_op_conv2d_sliced")
    return y


def _op_slice_pair(name, precision, x, c, x_off, y, y_off, extra, device):
    L = load()
    x = _whole(x)
    same = y is None
    y = np.empty((x.shape[0],) + tuple(extra or x.shape[1:3]) + (x.shape[3],), np.float32) if same else _whole(y).copy()
    n, h, w, x_cs = x.shape
    assert y.shape[0] == n and (extra is None or y.shape[1:3] == tuple(extra))
    prec = [] if precision is None else [precision]
    mid = [] if precision is None else [int(same)]
    _reid_check(L, getattr(L, name)(device, *prec, _fp(x), n, h, w, c, x_cs, x_off, *mid, *(extra or ()), y.shape[3], y_off, _fp(y)), name)
    return y


def op_maxpool5(x, c, x_off, y, y_off, precision=PREC_F32, device=0):
    """maxpool5_kernel (MaxPool2d(5, 1, 2)): channels x_off .. x_off + c of the buffer x [n, h, w, x_cs] -> channels y_off .. of a copy of the buffer y
    [n, h, w, y_cs], returned whole.  y = None: input and output are slices of ONE buffer (SPPF); feed the result back as x for the next pool of the chain."""
    return _op_slice_pair("eagle_op_maxpool5", precision, x, c, x_off, y, y_off, None, device)


def op_upsample2(x, c, x_off, y, y_off, out_hw, precision=PREC_F32, device=0):
    """upsample2_kernel (nearest x2, cropped): channels x_off .. of x [n, h, w, x_cs] -> channels y_off .. of a copy of y [n, yh, yw, y_cs], returned whole;
    out_hw = (yh, yw) with yh in {2h - 1, 2h}, yw in {2w - 1, 2w}, anything else is an EagleError.  y = None: one buffer (only a 1 x 1 map keeps its size)."""
    return _op_slice_pair("eagle_op_upsample2", precision, x, c, x_off, y, y_off, tuple(out_hw), device)


def op_split_to_f32(x, c, x_off, y, y_off, device=0):
    """split_to_f32_kernel: channels x_off .. of x [n, h, w, x_cs], stored as split pairs, -> channels y_off .. of a copy of the fp32 buffer y [n, h, w, y_cs],
    returned whole with every bit outside the slice as it was."""
    assert y is not None, "the two storage formats differ: input and output cannot share a buffer"
    return _op_slice_pair("eagle_op_split_to_f32", None, x, c, x_off, y, y_off, None, device)


# --- the optical-flow kernels without a handle or weights (include/eagle.h eagle_op_gray_pyramid / eagle_op_flow) ----------------
def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def op_gray_pyramid(frames, device=0):
    """gray_kernel + pyrdown_kernel (csrc/flow.hip, K11) on BGR u8 frames [n, h, w, 3] -> ([g0, g1, g2] u8 [n, lh, lw], levels): the gray frames, their
    two pyrDown levels and the highest level the tracker uses, by the rule of eagle_clip_open."""
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    h1, w1 = (h + 1) // 2, (w + 1) // 2
    g = [np.zeros((n, h, w), np.uint8), np.zeros((n, h1, w1), np.uint8), np.zeros((n, (h1 + 1) // 2, (w1 + 1) // 2), np.uint8)]
    levels = C.c_int(-1)
    rc = L.eagle_op_gray_pyramid(device, _u8p(frames), n, h, w, _u8p(g[0]), _u8p(g[1]), _u8p(g[2]), C.byref(levels))
    if rc:
        raise EagleError(f"eagle_op_gray_pyramid failed ({rc}): {L.eagle_last_error(None).decode()}")
    return g, levels.value


def op_flow(frames, src_frame, dst_frame, hue_frame, kps, device=0):
    """calculate_optical_flow (cm.py:419-478) on BGR u8 frames [n, h, w, 3] as Handle.clip_flow(raw=True) runs it (K11, lk_kernel, flow_filter_kernel)
    -> (filtered FLOWKP_DTYPE array in dict order, next points [n_in, 2] f32, status [n_in] u8)."""
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, h, w, _ = frames.shape
    kps = np.ascontiguousarray(kps, FLOWKP_DTYPE)
    out = np.zeros(N_LANDMARKS, FLOWKP_DTYPE); n_out = C.c_int(0)
    nxt = np.zeros((max(len(kps), 1), 2), np.float32); st = np.zeros(max(len(kps), 1), np.uint8)
    rc = L.eagle_op_flow(device, _u8p(frames), n, h, w, src_frame, dst_frame, hue_frame, kps.ctypes.data_as(C.c_void_p), len(kps),
                         out.ctypes.data_as(C.c_void_p), C.byref(n_out), _fp(nxt), _u8p(st))
    if rc:
        raise EagleError(f"eagle_op_flow failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out[: n_out.value].copy(), nxt[: len(kps)], st[: len(kps)]


# --- the ECC camera-motion kernels without a handle (include/eagle.h eagle_op_ecc_small / eagle_op_ecc) --------------------------
def op_ecc_small(gray, scale=0.15, device=0):
    """ecc_small_kernel (csrc/ecc.hip, K17) on gray u8 frames [n, h, w] -> u8 [n, dh, dw], the scale-sized images of eagle_clip_motion_ecc
    (dh = round(h * scale), dw = round(w * scale)); an EagleError below 4 x 4."""
    L = load()
    gray = np.ascontiguousarray(gray, np.uint8)
    n, h, w = gray.shape
    dh, dw = C.c_int(0), C.c_int(0)
    rc = L.eagle_op_ecc_small(device, _u8p(gray), n, h, w, float(scale), None, C.byref(dh), C.byref(dw))
    out = np.zeros((n, dh.value, dw.value), np.uint8)
    if not rc:
        rc = L.eagle_op_ecc_small(device, _u8p(gray), n, h, w, float(scale), _u8p(out), C.byref(dh), C.byref(dw))
    if rc:
        raise EagleError(f"eagle_op_ecc_small failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out


def op_ecc(small, pairs, carry=None, max_iter=100, eps=1e-5, device=0):
    """ecc_kernel (csrc/ecc.hip, K17), one launch: small u8 [n, h, w], pairs int32 [n_pairs, 2] of (template, image) indices, the template -1
    being `carry` u8 [h, w] -> ECC_DTYPE [n_pairs], the kernel's raw results (M in the pixels of `small`)."""
    L = load()
    small = np.ascontiguousarray(small, np.uint8)
    n, h, w = small.shape
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    if carry is not None:
        carry = np.ascontiguousarray(carry, np.uint8)
        assert carry.shape == (h, w)
    out = np.zeros(len(pairs), ECC_DTYPE)
    rc = L.eagle_op_ecc(device, _u8p(small), n, h, w, None if carry is None else _u8p(carry), pairs.ctypes.data_as(C.POINTER(C.c_int32)), len(pairs),
                        int(max_iter), float(eps), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise EagleError(f"eagle_op_ecc failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out


# --- trails, pass arrows and the owner ring; the trajectory and the pass still -------------------------------------------------
def trail_params(window=25, max_gap=25, half_width=1, pass_hold=5, dim_floor=64):
    """EagleTrailParams.  One second of rows at 25 fps, a thin line, five rows of hold and a fade to a quarter are conventional choices."""
    return EagleTrailParams(int(window), int(max_gap), int(half_width), int(pass_hold), int(dim_floor))


def op_minimap_trails(values, frames, columns, team_mapping, params, trail, sel=(), owner=None, events=None, row0=0, n=None, fmt="bgr", layout=None, out=None, device=0):
    """op_minimap with the trail, pass-arrow and owner layers (include/eagle.h eagle_op_minimap_trails): frames int32 [rows], params minimap_params(...,
    layers=...), trail trail_params(...) (None with layers == 0), sel the selected table columns, owner int32 [rows] or None, events EVENT_DTYPE or None."""
    return _op_minimap_layers("op_minimap_trails", values, frames, columns, team_mapping, params, None, trail, sel, owner, events, row0, n, fmt, layout, out, device)


def hull_params(half_width=1):
    """EagleHullParams: a thin line is the conventional choice."""
    return EagleHullParams(int(half_width))


def op_team_shape(values, columns, team_mapping, device=0):
    """The team-shape launches on a constructed table (include/eagle.h eagle_op_team_shape): values float64 [cols][rows][2], columns [(kind, id, video)]
    -> (SHAPE_DTYPE [rows, 2], int32 [rows, 2, SHAPE_HULL_CAP])."""
    L = load()
    values, columns = _table_args("op_team_shape", values, columns)
    cols, rows = values.shape[:2]
    ids, vals, nt = _team_arrays(team_mapping)
    rec, hull = np.zeros((rows, 2), SHAPE_DTYPE), np.full((rows, 2, SHAPE_HULL_CAP), -1, np.int32)
    keep = np.zeros(16, np.float64)
    rc = L.eagle_op_team_shape(device, _ptr(values, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt, _ptr(rec, keep), _ptr(hull, keep))
    if rc:
        raise EagleError(f"eagle_op_team_shape failed ({rc}): {L.eagle_last_error(None).decode()}")
    return rec, hull


def role_params(roles=10, min_present=8, iterations=8):
    """EagleRoleParams.  Ten outfield roles, a view that shows eight of them and eight rounds are conventional choices, not fitted to data."""
    return EagleRoleParams(int(roles), int(min_present), int(iterations))


def op_roles(values, columns, team_mapping, params=None, device=0):
    """The role launches on a constructed table (include/eagle.h eagle_op_roles): values float64 [cols][rows][2], columns [(kind, id, video)]
    -> (ROLE_ROW_DTYPE [rows, 2], int8 [members, rows], ROLE_MODEL_DTYPE [1])."""
    L = load()
    values, columns = _table_args("op_roles", values, columns)
    cols, rows = values.shape[:2]
    ids, vals, nt = _team_arrays(team_mapping)
    first = {}
    for i, v in zip(() if ids is None else ids.tolist(), () if vals is None else vals.tolist()):
        first.setdefault(i, v)
    nm = sum(1 for k in columns if not k["video"] and int(k["kind"]) == POST_PLAYER and first.get(int(k["id"]), -1) >= 0)
    rec, mr, model = np.zeros((rows, 2), ROLE_ROW_DTYPE), np.full((nm, rows), -1, np.int8), np.zeros(1, ROLE_MODEL_DTYPE)
    rec["col"] = -1
    p = role_params() if params is None else params
    keep = np.zeros(16, np.float64)
    rc = L.eagle_op_roles(device, _ptr(values, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt, C.byref(p), _ptr(rec, keep), _ptr(mr, keep),
                          _ptr(model, keep))
    if rc:
        raise EagleError(f"eagle_op_roles failed ({rc}): {L.eagle_last_error(None).decode()}")
    return rec, mr, model


def space_params(cells_per_metre=1, goalkeepers=1, radius=3.0):
    """EagleSpaceParams.  A marking radius of 3 m is a conventional choice, not fitted to data."""
    return EagleSpaceParams(int(cells_per_metre), int(goalkeepers), float(radius))


def op_space(values, columns, team_mapping, params=None, row0=0, n=0, device=0):
    """The space launches on a constructed table (include/eagle.h eagle_op_space): values float64 [cols][rows][2], columns [(kind, id, video)] ->
    (SPACE_ROW_DTYPE [rows], SPACE_SITE_DTYPE [rows, 32], SPACE_TOTALS_DTYPE [members], owner maps uint8 [n, gh, gw] of rows row0 .. row0 + n - 1)."""
    L = load()
    values, columns = _table_args("op_space", values, columns)
    cols, rows = values.shape[:2]
    ids, vals, nt = _team_arrays(team_mapping)
    p = space_params() if params is None else params
    first = {}
    for i, v in zip(() if ids is None else ids.tolist(), () if vals is None else vals.tolist()):
        first.setdefault(i, v)
    nm = sum(1 for k in columns if not k["video"] and ((int(k["kind"]) == POST_PLAYER and first.get(int(k["id"]), -1) >= 0)
                                                       or (int(k["kind"]) == POST_GOALKEEPER and p.goalkeepers)))
    rec, sites, totals = np.zeros(rows, SPACE_ROW_DTYPE), np.zeros((rows, SPACE_SITE_CAP), SPACE_SITE_DTYPE), np.zeros(nm, SPACE_TOTALS_DTYPE)
    grid = np.zeros((max(int(n), 0), 68 * max(p.cells_per_metre, 0), 105 * max(p.cells_per_metre, 0)), np.uint8)
    keep = np.zeros(16, np.float64)
    rc = L.eagle_op_space(device, _ptr(values, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt, C.byref(p), int(row0), int(n),
                          _ptr(rec, keep), _ptr(sites, keep), _ptr(totals, keep), _ptr(grid, keep))
    if rc:
        raise EagleError(f"eagle_op_space failed ({rc}): {L.eagle_last_error(None).decode()}")
    return rec, sites, totals, grid


def offside_params(direction=OFFSIDE_DIR_AUTO, assume_keeper=1, tolerance=0.5):
    """EagleOffsideParams.  A tolerance of 0.5 m is a conventional choice, not fitted to data."""
    return EagleOffsideParams(int(direction), int(assume_keeper), float(tolerance))


def op_offside(values, columns, team_mapping, params=None, events=None, frames=None, device=0):
    """The offside launches on a constructed table (include/eagle.h eagle_op_offside): values float64 [cols][rows][2], columns [(kind, id, video)],
    team_mapping {id: team} or (id, team) pairs of which the first for an id counts, events EVENT_DTYPE or None -> (OFFSIDE_ROW_DTYPE [rows, 2], margins
    int32 [members, rows], OFFSIDE_TOTALS_DTYPE [members], OFFSIDE_CLIP_DTYPE [1], OFFSIDE_EVENT_DTYPE [events])."""
    L = load()
    values, columns = _table_args("op_offside", values, columns)
    cols, rows = values.shape[:2]
    pairs = None if team_mapping is None else list(team_mapping.items() if isinstance(team_mapping, dict) else team_mapping)
    ids = None if pairs is None else np.ascontiguousarray([int(k) for k, _ in pairs], np.int32)
    vals = None if pairs is None else np.ascontiguousarray([int(v) for _, v in pairs], np.int32)
    first = {}
    for i, v in pairs or ():
        first.setdefault(int(i), int(v))
    nm = sum(1 for k in columns if not k["video"] and int(k["kind"]) == POST_PLAYER and first.get(int(k["id"]), -1) >= 0)
    p = offside_params() if params is None else params
    events = np.zeros(0, EVENT_DTYPE) if events is None else np.ascontiguousarray(events, EVENT_DTYPE)
    frames = None if frames is None else np.ascontiguousarray(frames, np.int32)
    rec, mg, totals, clip = np.zeros((rows, 2), OFFSIDE_ROW_DTYPE), np.zeros((nm, rows), np.int32), np.zeros(nm, OFFSIDE_TOTALS_DTYPE), np.zeros(1, OFFSIDE_CLIP_DTYPE)
    ev = np.zeros(len(events), OFFSIDE_EVENT_DTYPE)
    keep = np.zeros(16, np.float64)
    rc = L.eagle_op_offside(device, _ptr(values, keep), _ptr(frames, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep),
                            0 if pairs is None else len(pairs), C.byref(p), _ptr(events, keep), len(events), _ptr(rec, keep), _ptr(mg, keep), _ptr(totals, keep),
                            _ptr(clip, keep), _ptr(ev, keep))
    if rc:
        raise EagleError(f"eagle_op_offside failed ({rc}): {L.eagle_last_error(None).decode()}")
    return rec, mg, totals, clip, ev


def goal_view_params(direction=OFFSIDE_DIR_AUTO, group=0, cells_per_metre=1, form=GOALVIEW_FORM_DEFAULT, grid_row0=0, grid_rows=0, radius=0.4, keeper_radius=1.0,
                     min_depth=1.0, max_range=40.0, chance=0.3):
    """EagleGoalViewParams.  The radii, the range and the angle of a chance are conventional choices, not fitted to data."""
    return EagleGoalViewParams(int(direction), int(group), int(cells_per_metre), int(form), int(grid_row0), int(grid_rows), float(radius), float(keeper_radius),
                               float(min_depth), float(max_range), float(chance))


def op_goal_view(values, columns, team_mapping, params, owner=None, times=False, device=0, fetch_grid=True):
    """The goal-view launches on a constructed table (include/eagle.h eagle_op_goal_view): values float64 [cols][rows][2], columns [(kind, id, video)],
    team_mapping as op_offside's, owner int32 [rows] (a column or -1) or None -> {"rows": GOALVIEW_ROW_DTYPE [rows, 2], "open": int32, "mask": uint64,
    "status": uint8 [members, rows], "totals": GOALVIEW_TOTALS_DTYPE [members], "grid": uint8 [grid_rows, 68 R, 105 R]} and, with times, "times": a dict of
    milliseconds per GOALVIEW_TIMES name.  fetch_grid=False leaves the grid on the device ("grid" is None): a measurement does not need the copy."""
    L = load()
    values, columns = _table_args("op_goal_view", values, columns)
    cols, rows = values.shape[:2]
    pairs = None if team_mapping is None else list(team_mapping.items() if isinstance(team_mapping, dict) else team_mapping)
    ids = None if pairs is None else np.ascontiguousarray([int(k) for k, _ in pairs], np.int32)
    vals = None if pairs is None else np.ascontiguousarray([int(v) for _, v in pairs], np.int32)
    owner = None if owner is None else np.ascontiguousarray(owner, np.int32)
    if owner is not None and owner.shape != (rows,):
        raise EagleError("op_goal_view: one owner per row")
    keep = np.zeros(16, np.float64)
    nm = C.c_int(0)
    args = (device, _ptr(values, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), 0 if pairs is None else len(pairs),
            None if owner is None else _ptr(owner, keep), C.byref(params))
    first = {}
    for i, v in pairs or ():
        first.setdefault(int(i), int(v))
    n = sum(1 for k in columns if not k["video"] and int(k["kind"]) == POST_PLAYER and first.get(int(k["id"]), -1) >= 0)       # the members, as op_offside counts them
    R = params.cells_per_metre if params.cells_per_metre in (1, 2, 4) else 1
    out = {"rows": np.zeros((rows, 2), GOALVIEW_ROW_DTYPE), "open": np.zeros((n, rows), np.int32), "mask": np.zeros((n, rows), np.uint64),
           "status": np.zeros((n, rows), np.uint8), "totals": np.zeros(n, GOALVIEW_TOTALS_DTYPE),
           "grid": np.zeros((max(int(params.grid_rows), 0) if rows and fetch_grid else 0, 68 * R, 105 * R), np.uint8)}
    tm = np.zeros(len(GOALVIEW_TIMES), np.float32)
    if not fetch_grid:
        out["grid"] = None
    rc = L.eagle_op_goal_view(*args, *(_ptr(out[k], keep) for k in ("rows", "open", "mask", "status", "totals", "grid")), C.byref(nm), _ptr(tm, keep) if times else None)
    if rc:
        raise EagleError(f"eagle_op_goal_view failed ({rc}): {L.eagle_last_error(None).decode()}")
    if nm.value != n:
        raise EagleError(f"op_goal_view: the library counts {nm.value} members, the caller {n}")
    if times:
        out["times"] = dict(zip(GOALVIEW_TIMES, map(float, tm)))
    return out


def ball_track_params(fps, frame_w, speed=0.0, gap=0, reward=0.0, brk=0.0, max_bytes=0):
    """EagleBallTrackParams; speed, reward and brk in pixels, gap in frames, 0: the default (a tenth of the frame's width, min(64, fps) frames, the speed, two
    and a half rewards: conventional choices, not fitted to data)."""
    p = EagleBallTrackParams()
    p.fps, p.frame_w, p.gap, p.speed, p.reward, p.brk, p.max_bytes = int(fps), int(frame_w), int(gap), float(speed), float(reward), float(brk), int(max_bytes)
    return p


def op_ball_track(counts, positions, cq, params, cuts=None, conf=None, det=None, recover=BALL_RECOVER_DEFAULT, times=False, device=0):
    """The ball-track launches on constructed candidates (include/eagle.h eagle_op_ball_track): counts int32 [n], positions int32 [sum, 2] half pixels, cq int32
    [sum] (or None with conf float32 [sum]), det int32 [sum] or None -> (BALL_FRAME_DTYPE [n], BALL_TRACKLET_DTYPE [tracklets], BALL_CLIP_DTYPE [1]), with
    times=True also the four device times in milliseconds (recurrence, recovery, rows, all)."""
    L = load()
    counts = np.ascontiguousarray(counts, np.int32).reshape(-1)
    n, total = len(counts), int(counts.astype(np.int64).sum())
    positions = np.ascontiguousarray(positions, np.int32).reshape(-1, 2)
    cq = None if cq is None else np.ascontiguousarray(cq, np.int32).reshape(-1)
    conf = None if conf is None else np.ascontiguousarray(conf, np.float32).reshape(-1)
    det = None if det is None else np.ascontiguousarray(det, np.int32).reshape(-1)
    for a, what in ((positions, "positions"), (cq, "cq"), (conf, "conf"), (det, "det")):
        if a is not None and len(a) != total:
            raise ValueError(f"op_ball_track: {what} has {len(a)} entries for {total} candidates")
    cuts = np.zeros(0, np.int32) if cuts is None else np.ascontiguousarray(cuts, np.int32).reshape(-1)
    frames, tracklets, clip, ms = np.zeros(n, BALL_FRAME_DTYPE), np.zeros(n, BALL_TRACKLET_DTYPE), np.zeros(1, BALL_CLIP_DTYPE), np.zeros(4, np.float32)
    keep = np.zeros(16, np.float64)
    rc = L.eagle_op_ball_track(device, _ptr(counts, keep), n, _ptr(positions, keep), _ptr(cq, keep), _ptr(conf, keep), _ptr(det, keep), _ptr(cuts, keep) if len(cuts) else None,
                               len(cuts), C.byref(params), int(recover), _ptr(frames, keep), _ptr(tracklets, keep), n, _ptr(clip, keep), _ptr(ms, keep) if times else None)
    if rc:
        raise EagleError(f"eagle_op_ball_track failed ({rc}): {L.eagle_last_error(None).decode()}")
    out = frames, tracklets[:int(clip[0]["tracklets"])].copy(), clip
    return out + (ms,) if times else out


def kit_params(min_pixels=None, min_crops=None, outlier=None):
    """EagleKitParams; None: the library's default (32 counted pixels, 3 used crops, 512 / 1024 of the distance between the medoids: conventional
    choices, not fitted to data).  outlier 0: nobody is neither."""
    p = EagleKitParams()
    load().eagle_kit_params_default(C.byref(p))
    for k, v in (("min_pixels", min_pixels), ("min_crops", min_crops), ("outlier", outlier)):
        if v is not None:
            setattr(p, k, int(v))
    return p


def op_team_cluster(frames, crops, slots, n_ids, params=None, times=False, device=0):
    """The team clustering on host frames uint8 [n, h, w, 3] (include/eagle.h eagle_op_team_cluster) -> (KIT_CROP_DTYPE [k], KIT_ID_DTYPE [n_ids],
    KIT_MODEL_DTYPE [1]), with times=True also the two device times in milliseconds (histograms, clustering)."""
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8)
    n, h, w = frames.shape[:3]
    crops = np.ascontiguousarray(crops, np.int32).reshape(-1, 5)
    slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
    if len(slots) != len(crops):
        raise ValueError(f"op_team_cluster: {len(slots)} slots for {len(crops)} crops")
    params = params or kit_params()
    recs, ids, model, ms = np.zeros(len(crops), KIT_CROP_DTYPE), np.zeros(int(n_ids), KIT_ID_DTYPE), np.zeros(1, KIT_MODEL_DTYPE), np.zeros(2, np.float32)
    keep = np.zeros(64, np.float64)
    rc = L.eagle_op_team_cluster(device, _ptr(frames, keep), n, h, w, _ptr(crops, keep), _ptr(slots, keep), len(crops), int(n_ids), C.byref(params), _ptr(recs, keep),
                                 _ptr(ids, keep), _ptr(model, keep), _ptr(ms, keep) if times else None)
    if rc:
        raise EagleError(f"eagle_op_team_cluster failed ({rc}): {L.eagle_last_error(None).decode()}")
    return (recs, ids, model, ms) if times else (recs, ids, model)


def op_team_cluster_ids(sums, used, params=None, times=False, device=0):
    """Steps 5 to 11 of the team clustering from given sums int64 [n_ids, 34] and used int32 [n_ids] (include/eagle.h eagle_op_team_cluster_ids)
    -> (KIT_ID_DTYPE [n_ids], KIT_MODEL_DTYPE [1]), with times=True also the device times."""
    L = load()
    sums = np.ascontiguousarray(sums, np.int64).reshape(-1, KIT_BINS)
    used = np.ascontiguousarray(used, np.int32).reshape(-1)
    if len(sums) != len(used):
        raise ValueError(f"op_team_cluster_ids: {len(sums)} rows of sums for {len(used)} ids")
    params = params or kit_params()
    ids, model, ms = np.zeros(len(used), KIT_ID_DTYPE), np.zeros(1, KIT_MODEL_DTYPE), np.zeros(2, np.float32)
    keep = np.zeros(64, np.float64)
    rc = L.eagle_op_team_cluster_ids(device, _ptr(sums, keep), _ptr(used, keep), len(used), C.byref(params), _ptr(ids, keep), _ptr(model, keep), _ptr(ms, keep) if times else None)
    if rc:
        raise EagleError(f"eagle_op_team_cluster_ids failed ({rc}): {L.eagle_last_error(None).decode()}")
    return (ids, model, ms) if times else (ids, model)


def shot_params(cut=None, low=None, grass_thr=None, window=None, min_len=None, fps=25):
    """EagleShotParams.  Unset fields take eagle_amd.shots.default_params(fps): cut 0.30, low 0.10 and grass_thr 0.35 in 1 / 65536, a window of
    max(2, round(0.4 fps)) frames and min_len = fps frames: conventional choices, not fitted to footage."""
    from . import shots as _shots
    d = _shots.default_params(fps)
    for k, v in (("cut", cut), ("low", low), ("grass_thr", grass_thr), ("window", window), ("min_len", min_len)):
        if v is not None:
            d[k] = int(v)
    return EagleShotParams(d["cut"], d["low"], d["grass_thr"], d["window"], d["min_len"])


def _shot_outputs(n, cap):
    """a clip of n frames has at most n shots"""
    return np.zeros(max(n, 0), SHOT_FRAME_DTYPE), np.zeros(max(n, 1) if cap is None else int(cap), SHOT_DTYPE), C.c_int(0)


def op_shots(frames, params=None, cap=None, signatures=True, device=0, **kw):
    """The shots launches on constructed frames (include/eagle.h eagle_op_shots): frames uint8 [n, h, w, 3], any h, w >= 4 ->
    (signatures u32 [n, 1537] or None, frames [n] of SHOT_FRAME_DTYPE, shots [m] of SHOT_DTYPE)."""
    L = load()
    p = shot_params(**kw) if params is None else params
    frames = np.ascontiguousarray(frames, np.uint8)
    if frames.ndim != 4 or frames.shape[3] != 3:
        raise EagleError(f"op_shots: frames must be [n, h, w, 3] (got {frames.shape})")
    n, h, w, _ = frames.shape
    rows, shots, m = _shot_outputs(n, cap)
    sig = np.zeros((n, SHOT_SIGNATURE), np.uint32) if signatures else None
    keep = np.zeros(8, np.uint8)
    rc = L.eagle_op_shots(device, _ptr(frames, keep), n, h, w, C.byref(p), _ptr(rows, keep), _ptr(shots, keep), len(shots), C.byref(m), None if sig is None else _ptr(sig, keep))
    if rc:
        raise EagleError(f"eagle_op_shots failed ({rc}): {L.eagle_last_error(None).decode()}")
    return sig, rows, shots[:m.value].copy()


def topview_params(scale=8, margin=None, background=0x000000, markings=False, marking_colour=0xFF0000, mask_boxes=False, box_pad=0.0, first=0, step=1, min_count=1):
    """EagleTopviewParams; margin None: two metres' worth of pixels, at most 64 (the minimap's default).  Colours are B | G << 8 | R << 16; black, red
    and min_count = 1 are conventional choices."""
    if margin is None:
        margin = min(64, 2 * int(scale))
    return EagleTopviewParams(int(scale), int(margin), int(background), int(bool(markings)), int(marking_colour), int(bool(mask_boxes)), float(box_pad), int(first),
                              int(step), int(min_count))


def topview_size(params):
    """(W, Hc) of the canvas these parameters give (include/eagle.h eagle_topview_size; no GPU involved)."""
    w, h = C.c_int(0), C.c_int(0)
    L = load()
    rc = L.eagle_topview_size(C.byref(params), C.byref(w), C.byref(h))
    if rc:
        raise EagleError(f"eagle_topview_size failed ({rc}): {L.eagle_last_error(None).decode()}")
    return w.value, h.value


def _topview_maps(what, Hs, valid, n):
    Hs = np.ascontiguousarray(Hs, np.float64).reshape(-1, 9)
    valid = np.ascontiguousarray(valid, np.uint8).reshape(-1)
    if len(Hs) != n or len(valid) != n:
        raise EagleError(f"{what}: {n} frames but {len(Hs)} homographies and {len(valid)} valid flags")
    return Hs, valid


def _topview_recs(recs, n):
    if recs is None:
        return None
    recs = np.ascontiguousarray(recs, RESULT_DTYPE).reshape(-1)
    if len(recs) != n:
        raise EagleError(f"topview: {n} frames but {len(recs)} records")
    return recs


def op_topview(frames, Hs, valid, params, boxes=None, mode=TOPVIEW_VIDEO, fmt="bgr", layout=None, out=None, device=0):
    """The top-view launches on constructed frames (include/eagle.h eagle_op_topview): frames uint8 [n, h, w, 3] of any size, Hs [n, 9], valid [n],
    boxes a list of n float32 [k, 4] arrays (or None) -> a dict with "video" (mode & TOPVIEW_VIDEO: [n, Hc, W, 3] / [n, 3 Hc / 2, W] when dense, else
    the flat buffer ``out`` or a zeroed one written in ``layout``), "mosaic" and "cnt" (TOPVIEW_MOSAIC), "res_sum", "res_cnt", "covered"
    (TOPVIEW_RESIDUAL)."""
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8)
    if frames.ndim != 4 or frames.shape[3] != 3:
        raise EagleError(f"op_topview: frames must be [n, h, w, 3] (got {frames.shape})")
    n, h, w, _ = frames.shape
    Hs, valid = _topview_maps("op_topview", Hs, valid, n)
    W, Hc = topview_size(params)
    keep = np.zeros(16, np.uint8)
    flat, off = None, None
    if boxes is not None:
        if len(boxes) != n:
            raise EagleError(f"op_topview: {n} frames but {len(boxes)} box lists")
        per = [np.ascontiguousarray(b, np.float32).reshape(-1, 4) for b in boxes]
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(b) for b in per])]), np.int32)
        flat = np.ascontiguousarray(np.concatenate(per) if per else np.zeros((0, 4)), np.float32)
    res = {}
    lay = _yuv_layout(layout)
    if mode & TOPVIEW_VIDEO:
        need = out_span(fmt, Hc, W, lay, n)
        if out is None:
            out = np.zeros(need, np.uint8)
        if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
            raise EagleError(f"op_topview: out must be a contiguous uint8 array of at least {need} bytes")
        res["video"] = out
    if mode & TOPVIEW_MOSAIC:
        res["mosaic"], res["cnt"] = np.zeros((Hc, W, 3), np.uint8), np.zeros((Hc, W), np.uint32)
    if mode & TOPVIEW_RESIDUAL:
        res["res_sum"], res["res_cnt"], res["covered"] = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    g = lambda k: _ptr(res.get(k), keep)
    rc = L.eagle_op_topview(device, _ptr(frames, keep), n, h, w, _ptr(Hs, keep), _ptr(valid, keep), _ptr(flat, keep), _ptr(off, keep), C.byref(params), int(mode),
                            _out_pix(fmt), None if lay is None else C.byref(lay), g("video"), g("mosaic"), g("cnt"), g("res_sum"), g("res_cnt"), g("covered"))
    if rc:
        raise EagleError(f"eagle_op_topview failed ({rc}): {L.eagle_last_error(None).decode()}")
    if (mode & TOPVIEW_VIDEO) and lay is None:
        res["video"] = out.reshape((n, Hc, W, 3) if _out_pix(fmt) == 0 else (n, Hc * 3 // 2, W))
    return res


def linefit_params(**kw):
    """EagleLineFitParams: the library's defaults (eagle_linefit_params_default: k 4, tau 200, rounds 5, model 3, min_points 200, min_per_line 20, box_pad 3,
    radius 2.5, radius_min 0.5, radius_factor 0.6, max_shift 3, max_step 4: conventional choices, not fitted to footage) with the given fields replaced."""
    p = EagleLineFitParams()
    load().eagle_linefit_params_default(C.byref(p))
    names = {f[0] for f in EagleLineFitParams._fields_} - {"reserved"}
    for k, v in kw.items():
        if k not in names:
            raise EagleError(f"linefit_params: unknown parameter {k!r}")
        setattr(p, k, v)
    return p


def op_linefit(frames, Hs, valid, params=None, boxes=None, masks=True, device=0):
    """The line-registration launches on constructed frames (include/eagle.h eagle_op_linefit): frames uint8 [n, h, w, 3] of any size, Hs [n, 9], valid [n],
    boxes a list of n float32 [k, 4] arrays (or None) -> (Hs_out float64 [n, 9], frames LINEFIT_FRAME_DTYPE [n], masks uint32 [n, h, (w + 31) // 32] or
    None)."""
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8)
    if frames.ndim != 4 or frames.shape[3] != 3:
        raise EagleError(f"op_linefit: frames must be [n, h, w, 3] (got {frames.shape})")
    n, h, w, _ = frames.shape
    Hs, valid = _topview_maps("op_linefit", Hs, valid, n)
    p = linefit_params() if params is None else params
    keep = np.zeros(16, np.uint8)
    flat, off = None, None
    if boxes is not None:
        if len(boxes) != n:
            raise EagleError(f"op_linefit: {n} frames but {len(boxes)} box lists")
        per = [np.ascontiguousarray(b, np.float32).reshape(-1, 4) for b in boxes]
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(b) for b in per])]), np.int32)
        flat = np.ascontiguousarray(np.concatenate(per) if per else np.zeros((0, 4)), np.float32)
    out, fr = np.zeros((n, 9), np.float64), np.zeros(n, LINEFIT_FRAME_DTYPE)
    mk = np.zeros((n, h, (w + 31) // 32), np.uint32) if masks else None
    rc = L.eagle_op_linefit(device, _ptr(frames, keep), n, h, w, _ptr(Hs, keep), _ptr(valid, keep), _ptr(flat, keep), _ptr(off, keep), C.byref(p), _ptr(out, keep),
                            _ptr(fr, keep), _ptr(mk, keep))
    if rc:
        raise EagleError(f"eagle_op_linefit failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out, fr, mk


def ground_params(key_min=48, key_lead=16, no_cull=False):
    """EagleGroundParams; 48 and 16 are the shots stage's grass rule, conventional choices that are not fitted to footage."""
    return EagleGroundParams(int(key_min), int(key_lead), int(bool(no_cull)), 0)


def ground_band(x0, x1, y0, y1, colour, alpha, keyed=False):
    """one GROUND_SHAPE_DTYPE record: the band x0 <= qx < x1, y0 <= qy < y1 (1 / 1024 m)"""
    s = np.zeros((), GROUND_SHAPE_DTYPE)
    s["kind"], s["a"][:4], s["colour"], s["alpha"], s["flags"] = GROUND_BAND, (x0, x1, y0, y1), colour, alpha, GROUND_KEYED if keyed else 0
    return s


def ground_ring(cx, cy, r0, r1, colour, alpha, keyed=False):
    """one GROUND_SHAPE_DTYPE record: the ring r0^2 <= (qx - cx)^2 + (qy - cy)^2 < r1^2 (1 / 1024 m)"""
    s = np.zeros((), GROUND_SHAPE_DTYPE)
    s["kind"], s["a"][:4], s["colour"], s["alpha"], s["flags"] = GROUND_RING, (cx, cy, r0, r1), colour, alpha, GROUND_KEYED if keyed else 0
    return s


def ground_shape_lists(lists):
    """a list of per-frame lists of GROUND_SHAPE_DTYPE records -> (shapes [off[n]], off int32 [n + 1])"""
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    flat = [np.asarray(s, GROUND_SHAPE_DTYPE).reshape(()) for x in lists for s in x]
    return (np.stack(flat) if flat else np.zeros(0, GROUND_SHAPE_DTYPE)), off


def _ground_lists(what, shapes, off, n):
    shapes = np.ascontiguousarray(shapes, GROUND_SHAPE_DTYPE).reshape(-1)
    off = np.ascontiguousarray(off, np.int32).reshape(-1)
    if len(off) != n + 1 or int(off[-1]) > len(shapes):
        raise EagleError(f"{what}: off must have n + 1 = {n + 1} entries that end inside the {len(shapes)} shapes (got {len(off)} entries)")
    return shapes, off


def op_ground(frames, Hs, valid, shapes, off, params=None, fmt="bgr", layout=None, out=None, device=0):
    """The ground launch on constructed frames (include/eagle.h eagle_op_ground): frames uint8 [n, h, w, 3] of any size, Hs [n, 9], valid [n], shapes
    GROUND_SHAPE_DTYPE [off[n]], off [n + 1] -> (the pictures: [n, h, w, 3] / [n, 3h / 2, w] when dense, else the flat buffer ``out`` or a zeroed one
    written in ``layout``; covered uint32 [n])."""
    L = load()
    frames = np.ascontiguousarray(frames, np.uint8)
    if frames.ndim != 4 or frames.shape[3] != 3:
        raise EagleError(f"op_ground: frames must be [n, h, w, 3] (got {frames.shape})")
    n, h, w, _ = frames.shape
    Hs, valid = _topview_maps("op_ground", Hs, valid, n)
    shapes, off = _ground_lists("op_ground", shapes, off, n)
    p = ground_params() if params is None else params
    lay = _yuv_layout(layout)
    need = out_span(fmt, h, w, lay, n)
    if out is None:
        out = np.zeros(need, np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
        raise EagleError(f"op_ground: out must be a contiguous uint8 array of at least {need} bytes")
    cov = np.zeros(n, np.uint32)
    keep = np.zeros(16, np.uint8)
    rc = L.eagle_op_ground(device, _ptr(frames, keep), n, h, w, _ptr(Hs, keep), _ptr(valid, keep), _ptr(shapes, keep), _ptr(off, keep), C.byref(p), _out_pix(fmt),
                           None if lay is None else C.byref(lay), _ptr(out, keep), _ptr(cov, keep))
    if rc:
        raise EagleError(f"eagle_op_ground failed ({rc}): {L.eagle_last_error(None).decode()}")
    if lay is None:
        out = out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
    return out, cov


def op_minimap_hulls(values, frames, columns, team_mapping, params, hull, trail=None, sel=(), owner=None, events=None, row0=0, n=None, fmt="bgr", layout=None, out=None,
                     device=0):
    """op_minimap_trails with the hull layer (include/eagle.h eagle_op_minimap_hulls): the entry computes the team shape itself; hull hull_params(...)
    (None without MM_HULLS in params.layers), trail None without the other three bits."""
    return _op_minimap_layers("op_minimap_hulls", values, frames, columns, team_mapping, params, hull, trail, sel, owner, events, row0, n, fmt, layout, out, device, True)


def _op_minimap_layers(name, values, frames, columns, team_mapping, params, hull, trail, sel, owner, events, row0, n, fmt, layout, out, device, hulls=False):
    L = load()
    values, columns = _table_args(name, values, columns)
    cols, rows = values.shape[:2]
    frames = None if frames is None else np.ascontiguousarray(frames, np.int32)
    sel = np.ascontiguousarray(sel, np.int32)
    owner = None if owner is None else np.ascontiguousarray(owner, np.int32)
    events = None if events is None else np.ascontiguousarray(events, EVENT_DTYPE)
    if (frames is not None and len(frames) != rows) or (owner is not None and len(owner) != rows):
        raise EagleError(f"{name}: one frame number and one owner per row")
    ids, vals, nt = _team_arrays(team_mapping)
    n = rows - row0 if n is None else n
    w, h = minimap_size(params)
    lay = _yuv_layout(layout)
    need = out_span(fmt, h, w, lay, n)
    if out is None:
        out = np.zeros(need, np.uint8)
    if out.dtype != np.uint8 or not out.flags.c_contiguous or out.nbytes < need:
        raise EagleError(f"{name}: out must be a contiguous uint8 array of at least {need} bytes")
    keep = np.zeros(16, np.float64)
    head = (device, _ptr(values, keep), _ptr(frames, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt, C.byref(params))
    tail = (None if trail is None else C.byref(trail), _ptr(sel, keep), len(sel), _ptr(owner, keep), _ptr(events, keep), 0 if events is None else len(events), int(row0),
            int(n), _out_pix(fmt), None if lay is None else C.byref(lay), out.ctypes.data_as(C.c_void_p))
    if hulls:
        rc = L.eagle_op_minimap_hulls(*head, None if hull is None else C.byref(hull), *tail)
    else:
        rc = L.eagle_op_minimap_trails(*head, *tail)
    if rc:
        raise EagleError(f"eagle_{name} failed ({rc}): {L.eagle_last_error(None).decode()}")
    if lay is None:
        return out.reshape((n, h, w, 3) if _out_pix(fmt) == 0 else (n, h * 3 // 2, w))
    return out


def op_trajectory_picture(values, frames, columns, team_mapping, sel, row0=0, n=None, scale=8, margin=None, half_width=1, max_gap=25, device=0):
    """The trajectory still of a constructed table (include/eagle.h eagle_op_trajectory_picture) -> BGR uint8 [h, w, 3]."""
    L = load()
    values, columns = _table_args("op_trajectory_picture", values, columns)
    cols, rows = values.shape[:2]
    frames = np.ascontiguousarray(frames, np.int32)
    if len(frames) != rows:
        raise EagleError("op_trajectory_picture: one frame number per row")
    sel = np.ascontiguousarray(sel, np.int32)
    ids, vals, nt = _team_arrays(team_mapping)
    n = rows - row0 if n is None else n
    mp = minimap_params(scale, margin)
    w, h = minimap_size(mp)
    out = np.zeros((h, w, 3), np.uint8)
    keep = np.zeros(16, np.float64)
    rc = L.eagle_op_trajectory_picture(device, _ptr(values, keep), _ptr(frames, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt, _ptr(sel, keep),
                                       len(sel), int(row0), int(n), mp.scale, mp.margin, int(half_width), int(max_gap), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise EagleError(f"eagle_op_trajectory_picture failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out


def op_pass_picture(values, columns, team_mapping, events, event, scale=8, margin=None, half_width=1, device=0):
    """The pass still of a constructed table (include/eagle.h eagle_op_pass_picture): events EVENT_DTYPE -> BGR uint8 [h, w, 3]."""
    L = load()
    values, columns = _table_args("op_pass_picture", values, columns)
    cols, rows = values.shape[:2]
    events = np.ascontiguousarray(events, EVENT_DTYPE)
    ids, vals, nt = _team_arrays(team_mapping)
    mp = minimap_params(scale, margin)
    w, h = minimap_size(mp)
    out = np.zeros((h, w, 3), np.uint8)
    keep = np.zeros(16, np.float64)
    rc = L.eagle_op_pass_picture(device, _ptr(values, keep), _ptr(columns, keep), rows, cols, _ptr(ids, keep), _ptr(vals, keep), nt, _ptr(events, keep), len(events), int(event),
                                 mp.scale, mp.margin, int(half_width), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise EagleError(f"eagle_op_pass_picture failed ({rc}): {L.eagle_last_error(None).decode()}")
    return out
