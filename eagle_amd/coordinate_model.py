"""Drop-in for the hot path of the reference's ``CoordinateModel`` (eagle/models/coordinate_model.py:47-628) in the
stateless configuration: every per-frame number comes from the HIP library through the C ABI.

Same constructor keywords and method names as the reference: ``CoordinateModel(keypoint_conf=0.3, detector_conf=0.35)``,
``get_coordinates(frames, fps, ...)`` -> ``{i: {"Coordinates", "Time", "Keypoints", "Boundaries"}}`` (cm.py:415),
``detect_objects(frame)``, ``detect_keypoints(frame)``.  ``get_coordinates`` covers every key-point / homography cadence of
the reference (optical-flow propagation between detections, first-frame search, on-demand detection, calibration:
cm.py:188-416).  ``tracker=True`` keys Player / Goalkeeper entries by track id like the reference does through boxmot's BotSort
(cm.py:574-596): the library's BoT-SORT association (include/eagle.h, eagle_track_*); ``reid=True`` adds the appearance branch and
``camera_motion="ecc"`` boxmot's default camera-motion compensation (ECC on the 0.15-scale gray frame, eagle_clip_motion_ecc) — together the
configuration the reference constructs at cm.py:66-72; ``camera_motion=True`` / ``"sparse"`` is BoT-SORT's sparse-optical-flow alternative on a
fixed grid (eagle_clip_motion).  ``tracker=False`` (default) is the reference's detection-index fallback (cm.py:598-627), the
stateless configuration of SURVEY §8a."""
import numpy as np

from . import clip, lib, records, weights
from .pitch import INTERSECTION_TO_PITCH_POINTS


class CoordinateModel:
    def __init__(self, keypoint_conf: float = 0.3, detector_conf: float = 0.35, *, frame_hw=(720, 1280),
                 detector="n", det_imgsz=640, batch=8, precision="f32s", device=0, hrnet_state_dict=None,
                 detector_state_dict=None, seed=0, use_graph=None, multi_stream=None, tracker=False, camera_motion=False, detector_precision=None,
                 reid=False, reid_state_dict=None, allow_saturation=False, letterbox="rect"):
        # letterbox: "rect" = ultralytics LetterBox(auto=True), what the reference's .pt detectors run with (cm.py:56-57); "square" = auto=False, the static
        # det_imgsz x det_imgsz input of its exported ONNX detector (the CPU default, cm.py:54-55)
        self.keypoint_conf, self.detector_conf = keypoint_conf, detector_conf
        self.tracker = tracker
        if camera_motion not in (False, True, None, "sparse", "ecc"):
            raise ValueError("camera_motion must be False, True / 'sparse' or 'ecc'")
        self.camera_motion = "sparse" if camera_motion is True else (camera_motion or False)
        self.reid = bool(reid) and tracker      # appearance matching inside the tracker (the reference's BotSort has it on: cm.py:66-72)
        self._tracker_open = False           # the reference builds ONE BotSort in __init__ (cm.py:66-72): ids keep counting across get_coordinates calls
        self.batch = batch
        # detector_precision=None: the library's default — with precision="f32s" the detector runs in the exact fp32 family (boxes, confidences,
        # classes, NMS order and hence every detection-index id equal the fp32 reference arithmetic bit for bit), otherwise in `precision`
        # "mixed": split-family trunk, exact last C2f per level + Detect (EAGLE_DET_PREC_MIXED: measured, does not keep the exact family's ids; never a default)
        dp = {} if detector_precision is None else {"det_precision": lib.DET_PREC_MIXED if detector_precision == "mixed" else lib.PRECISIONS[detector_precision] + 1}
        self.handle = lib.Handle(device=device, frame_h=frame_hw[0], frame_w=frame_hw[1], det_variant=detector,
                                 det_imgsz=det_imgsz, batch=batch, letterbox=letterbox,
                                 precision=lib.PRECISIONS[precision],
                                 keypoint_conf=keypoint_conf, detector_conf=detector_conf,
                                 detector_floor=min(detector_conf, 0.15),
                                 use_graph=self._graph_mode(use_graph),         # None: the library's small-batch rule (include/eagle.h EAGLE_SMALL_BATCH); 0 / 1 / 2 pass through
                                 multi_stream=lib.AUTO if multi_stream is None else int(bool(multi_stream)),
                                 allow_saturation=int(allow_saturation), **dp)
        # the reference reads eagle/models/weights/*.pt|.pth (cm.py:55-59); none exist here -> seeded synthetic
        hs = hrnet_state_dict if hrnet_state_dict is not None else weights.make_hrnet_state_dict(seed)
        ys = detector_state_dict if detector_state_dict is not None else weights.make_yolo_state_dict(detector, seed)
        sds = [hs, ys]
        if self.reid:                           # the reference downloads osnet_x0_25_msmt17.pt at run time (cm.py:69); none here -> seeded synthetic
            from . import osnet
            sds.append(reid_state_dict if reid_state_dict is not None else osnet.make_osnet_state_dict(seed))
        weights.load_into(self.handle, sds)

    @staticmethod
    def _graph_mode(use_graph):
        """EagleConfig::use_graph: None -> EAGLE_AUTO; False / True -> 0 / 1; the integers 0, 1, 2 as they are (2 = replay only inside calls of at least three
        steps).  Round 5 mapped everything through bool(): mode 2 silently became per-step replay."""
        if use_graph is None:
            return lib.AUTO
        if isinstance(use_graph, (bool, np.bool_)):
            return int(use_graph)
        m = int(use_graph)
        if m not in (0, 1, 2):
            raise ValueError(f"use_graph must be None, a bool, or 0 / 1 / 2 (got {use_graph!r})")
        return m

    # ---- raw records ---------------------------------------------------------------------------------
    def process_records(self, frames, pixel_format="bgr"):
        """frames: uint8 BGR [n, h, w, 3] (pixel_format "bgr"), or 4:2:0 decoder output [n, 3h/2, w] ("nv12" / "i420": the records of the BGR
        frames cv2.cvtColor(..., COLOR_YUV2BGR_NV12 / _I420) gives)."""
        if pixel_format == "bgr":
            return self.handle.process(np.asarray(frames))
        return self.handle.process_yuv(frames, pixel_format)

    def _upload(self, frames, pixel_format):
        """a dense BGR device clip of the frames (the entries that read resident frames take BGR): 4:2:0 frames are uploaded as they are and converted on the GPU"""
        return self.handle.upload_bgr(frames, pixel_format)

    # ---- reference-shaped API ------------------------------------------------------------------------
    def get_coordinates(self, frames, fps: int, num_homography: int = 1, num_keypoint_detection: int = 1,
                        verbose: bool = True, calibration: bool = False, pixel_format: str = "bgr") -> dict:
        """pixel_format: "bgr" (uint8 [n, h, w, 3]) or a decoder's 4:2:0 output "nv12" / "i420" (uint8 [n, 3h/2, w]): the same output as for the BGR
        frames cv2.cvtColor(..., COLOR_YUV2BGR_NV12 / _I420) gives."""
        homography_interval = max(1, int(fps / max(1, num_homography)))
        keypoint_interval = max(1, int(fps / max(1, num_keypoint_detection)))
        self._last_fps = fps
        if self.tracker:
            # before ANY motion estimate: eagle_track_open forgets the ECC estimator's carried template, so opening the tracker lazily after the
            # clip's camera motion (as until round 3) threw away the template this clip had just stored and mis-aligned the next clip's frame 0
            self._ensure_tracker_open()
        if calibration or keypoint_interval != 1:
            motion = [] if (self.tracker and self.camera_motion) else None
            recs = self.flow_records(frames, keypoint_interval, homography_interval, calibration, motion=motion, pixel_format=pixel_format)
            if self.tracker:
                self._track(recs, motion[0] if motion else None, frames, pixel_format)
            return self._remember({i: records.to_reference_dict(r, i, fps, own_h=bool(r["pad"][0])) for i, r in enumerate(recs)}, recs,
                                  np.array([bool(r["pad"][0]) for r in recs], bool))
        recs = self.process_records(frames, pixel_format)
        if self.tracker:
            self._track(recs, self._clip_motion(frames, pixel_format) if self.camera_motion else None, frames, pixel_format)
        own = np.ones(len(recs), bool)
        if homography_interval > 1:
            # cm.py:333-367: H is solved on scheduled frames or while the retry flag is set, and carried otherwise.  Every
            # frame's own H is already in its record; decide in clip order whose H each frame uses, then let the GPU
            # re-project the frames that use a carried one.
            Hs = np.zeros((len(recs), 9)); flags = np.zeros(len(recs), np.uint8)
            cur, retry = None, False
            for i, r in enumerate(recs):
                attempt = i % homography_interval == 0 or retry
                if attempt and r["H_valid"]:
                    cur, retry = r["H"].copy(), False
                elif attempt:
                    retry = True
                own[i] = attempt and bool(r["H_valid"])
                if not own[i]:
                    flags[i] = 1 if cur is not None else 2
                    if cur is not None:
                        Hs[i] = cur
            if flags.any():
                recs = self.handle.reproject(np.ascontiguousarray(recs), Hs, flags)
        return self._remember({i: records.to_reference_dict(r, i, fps, own_h=bool(own[i])) for i, r in enumerate(recs)}, recs, own)

    # ---- annotated output ----------------------------------------------------------------------------
    _last = None
    _last_fps = 25

    def _remember(self, coords, recs, own):
        """the records behind the last get_coordinates output (and which frames solved their own homography): annotate() draws from them, the dict is
        never parsed back"""
        self._last = (coords, recs, np.asarray(own, bool))
        return coords

    def _records_of(self, coords_or_records, carried_as_plain=False):
        """raw records, or the records behind the dict the LAST get_coordinates call of this model returned.  carried_as_plain: frames that use a
        carried homography get H_valid = 0, so that their picture lists every key-point, as the dict does (cm.py:330,415)."""
        if isinstance(coords_or_records, dict):
            if self._last is None or coords_or_records is not self._last[0]:
                raise ValueError("raw records, or the dict returned by this model's last get_coordinates call, expected")
            _, recs, own = self._last
            recs = np.array(recs, lib.RESULT_DTYPE, copy=True)
            if carried_as_plain:
                recs["H_valid"][~own] = 0
            return recs
        return np.ascontiguousarray(coords_or_records, lib.RESULT_DTYPE).reshape(-1)

    def shots(self, frames, fps, pixel_format="bgr", **overrides):
        """Where the clip is cut and which of its shots look at the pitch (eagle_amd/shots.py find_shots): run it in front of get_coordinates,
        which assumes one continuous shot.  Nothing consumes the result unless the caller does."""
        from . import shots as sh
        return sh.find_shots(self.handle, frames, fps, pixel_format, **overrides)

    def topview(self, frames, coords_or_records, carry=False, out_format="bgr", **kw):
        """The frames warped onto the pitch plane with the homography of their records (eagle_amd/topview.py topview): uint8 [n, Hc, W, 3], or
        [n, 3 Hc / 2, W] for "nv12" / "i420".  ``coords_or_records`` as annotate takes them; a frame that did not solve its own homography has none
        unless ``carry`` hands it the latest earlier one."""
        from . import topview as tv
        return tv.topview(self.handle, frames, self._records_of(coords_or_records, carried_as_plain=True), carry, out_format, **kw)

    def mosaic(self, frames, coords_or_records, carry=False, **kw):
        """The mean of the warped frames, its count map and every frame's distance from it (eagle_amd/topview.py mosaic)."""
        from . import topview as tv
        return tv.mosaic(self.handle, frames, self._records_of(coords_or_records, carried_as_plain=True), carry, **kw)

    def refine_lines(self, frames, coords_or_records, fps=None, **params):
        """Line registration (eagle_amd/linefit.py, include/eagle.h eagle_linefit_frames): the homography each frame's pitch coordinates were projected
        with, its own or the carried one (the cadence writes the carried matrix into the record when it re-projects), is refined on the frame's painted
        lines; a frame that was projected with none has no map and stays as it is; the detections of the records hide the players.  The accepted
        frames are re-projected by the library (Handle.reproject), so foot points, pitch cells, in_bounds and boundaries follow, and their records hold
        the refined matrix; every other frame keeps its record byte for byte.  ``frames`` uint8 BGR [n, h, w, 3]; ``coords_or_records`` as annotate
        takes them; ``fps`` for the rebuilt dict's Time (default: the last get_coordinates call's).  The new dict takes the place of the old one for
        annotate, topview, ground and Processor.process_data -> (coordinates, report: linefit.Result)."""
        from . import linefit as lf, topview as tv
        of_dict = isinstance(coords_or_records, dict)
        recs = np.ascontiguousarray(self._records_of(coords_or_records)).copy()
        own = self._last[2].copy() if of_dict else np.ones(len(recs), bool)
        if len(recs) != len(frames):
            raise ValueError(f"{len(frames)} frames but {len(recs)} records")
        Hs, valid, _ = tv.homographies(recs)                # the record's H is the matrix the frame was projected with, also where it was carried
        report = lf.refine(self.handle, np.asarray(frames), Hs, valid, recs, **params)
        recs = lf.apply(self.handle, recs, report)
        fps = self._last_fps if fps is None else fps
        return self._remember({i: records.to_reference_dict(r, i, fps, own_h=bool(own[i])) for i, r in enumerate(recs)}, recs, own), report

    def ground(self, frames, coords_or_records, shapes, off, carry=True, out_format="bgr", params=None):
        """The frames with shapes of the pitch plane blended into their grass (eagle_amd/ground.py, include/eagle.h eagle_ground_frames): shapes
        lib.GROUND_SHAPE_DTYPE [off[n]] and off [n + 1], one list per frame, in 1 / 1024 m on the pitch; the homography of a frame is its record's,
        with ``carry`` the latest earlier one where it has none -> (pictures uint8 [n, h, w, 3] or [n, 3h / 2, w], covered uint32 [n])."""
        from . import topview as tv
        Hs, valid, _ = tv.homographies(self._records_of(coords_or_records, carried_as_plain=True), carry)
        return self.handle.ground(frames, Hs, valid, shapes, off, params, out_format)

    def annotate(self, frames, coords_or_records, team_mapping=None, pixel_format="bgr", out_format="bgr", table=None):
        """The frames with their records drawn on them (the reference's annotated video, main.py:43-81; include/eagle.h eagle_annotate_frames):
        uint8 [n, h, w, 3] for out_format "bgr", [n, 3h/2, w] for "nv12" / "i420".  ``frames`` as get_coordinates takes them (pixel_format "bgr",
        "nv12" or "i420"); ``coords_or_records``: raw records (process_records / flow_records), or the dict the LAST get_coordinates call of this
        model returned; team_mapping: Processor.get_team_mapping's {player id: 0 | 1}, or None for a neutral player colour.
        ``table`` (postprocess.process_data): draw the processed table instead, as main.py does — one output frame per kept row, with the
        interpolated ball, the folded goalkeeper ids and the table's team mapping; key-points still come from the frame's record."""
        recs = self._records_of(coords_or_records, carried_as_plain=True)
        if len(recs) != len(frames):
            raise ValueError(f"{len(frames)} frames but {len(recs)} records")
        if table is not None:
            frames = np.asarray(frames)[np.asarray(table.rows, np.int64)]
        n = len(frames)
        if n == 0:
            h, w = self.handle.cfg.frame_h, self.handle.cfg.frame_w
            return np.zeros((0, h, w, 3) if out_format == "bgr" else (0, h * 3 // 2, w), np.uint8)
        d = self._upload(frames, pixel_format)
        try:
            if table is None:
                return self.handle.annotate(d, n, recs, team_mapping, out_format)
            lists = [table.overlay(r, recs[int(f)]) for r, f in enumerate(table.rows)]
            offsets = np.concatenate([[0], np.cumsum([len(p) for p in lists])]).astype(np.int32)
            return self.handle.annotate_prims(d, n, np.concatenate(lists), offsets, out_format)
        finally:
            self.handle.free(d)

    def reset_tracker(self):
        """Forget every track: the next clip starts with a fresh tracker (frame counter 0, ids from 1), which is what a new
        ``CoordinateModel`` gives in the reference."""
        self._tracker_open = False
        if self.tracker:
            self._ensure_tracker_open()      # at once: the reset also drops the camera-motion estimator's template (boxmot's ECC object dies with its tracker)

    def _ensure_tracker_open(self):
        if not self._tracker_open:
            self.handle.track_open()
            self._tracker_open = True

    def reid_inputs(self, recs, high=0.5):
        """boxmot extracts appearance features for the high-confidence detections (conf > track_high_thresh) from ``frame[y1:y2, x1:x2]`` of
        the integer-truncated, frame-clipped box -> (crops [k,5], detection index per crop, crops per record)."""
        fh, fw = self.handle.cfg.frame_h, self.handle.cfg.frame_w
        crops, det, count = [], [], []
        for i, r in enumerate(recs):
            k = 0
            for j in range(int(r["n_det"])):
                d = r["det"][j]
                if not float(d["conf"]) > high:
                    continue
                x1, y1 = max(0, int(d["x1"])), max(0, int(d["y1"]))
                x2, y2 = min(fw - 1, int(d["x2"])), min(fh - 1, int(d["y2"]))
                if x2 > x1 and y2 > y1:
                    crops.append((i, x1, y1, x2, y2)); det.append(j); k += 1
            count.append(k)
        return np.asarray(crops, np.int32).reshape(-1, 5), np.asarray(det, np.int32), np.asarray(count, np.int32)

    def _track(self, recs, warps=None, frames=None, pixel_format="bgr"):
        """One clip: track ids + smoothed boxes into the records (frame order), pitch coordinates re-projected on the GPU.  Like the
        reference's single BotSort instance (cm.py:66-72, 577) the tracker state lives as long as the model: ids keep increasing over
        successive clips and only the very first frame ever seen activates its tracks at once; ``reset_tracker()`` starts over."""
        self._ensure_tracker_open()
        if self.reid and frames is not None:
            crops, det, count = self.reid_inputs(recs)
            d = self._upload(frames, pixel_format)
            try:
                feats = self.handle.reid_features(d, len(frames), crops)
            finally:
                self.handle.free(d)
            self.handle.track_frames_reid(recs, feats, det, count, warps)
        else:
            self.handle.track_frames(recs, warps)
        return recs

    def _session_motion(self, n):
        """camera motions of the open clip session, by the configured estimator"""
        if self.camera_motion == "ecc":
            return self.handle.clip_motion_ecc(0, n, carry=True)
        return self.handle.clip_motion(0, n)

    def _clip_motion(self, frames, pixel_format="bgr"):
        """[n, 6] camera motions of a clip that is not in a clip session yet: gray pyramids + sparse LK on the GPU (eagle_clip_open / _motion)."""
        d = self._upload(frames, pixel_format)
        try:
            self.handle.clip_open(d, len(frames))
            try:
                return self._session_motion(len(frames))
            finally:
                self.handle.clip_close()
        finally:
            self.handle.free(d)

    def flow_records(self, frames, keypoint_interval, homography_interval, calibration=False, stats=None, keypoint_source=None, motion=None,
                     pixel_format="bgr"):
        """Records of the reference loop in a stateful cadence (cm.py:188-416); see eagle_amd/clip.py."""
        if len(frames) == 0:
            return np.zeros(0, lib.RESULT_DTYPE)
        d = self._upload(frames, pixel_format)
        try:
            return clip.run_clip(self.handle, d, len(frames), keypoint_interval, homography_interval, calibration, stats, keypoint_source, motion,
                                 motion_fn=self._session_motion)
        finally:
            self.handle.free(d)

    def detect_objects(self, frame):
        rec = self.process_records(frame[None])[0]
        res = {"Player": {}, "Goalkeeper": {}}
        for cname, objs in records._objects(rec).items():
            for oid, d in objs.items():
                res.setdefault(cname, {})[oid] = {"BBox": [int(d["bx1"]), int(d["by1"]), int(d["bx2"]), int(d["by2"])],
                                                  "Confidence": float(d["conf"]),
                                                  "Bottom_center": [int(d["foot_x"]), int(d["foot_y"])]}
        if any(int(d["cls"]) == 2 for d in rec["det"][: int(rec["n_det"])]):
            res.setdefault("Ball", {})
        return res

    def detect_keypoints(self, frame):
        rec = self.process_records(frame[None])[0]
        return {INTERSECTION_TO_PITCH_POINTS[int(k["label"])]: (int(k["x"]), int(k["y"]))
                for k in rec["kp"][: int(rec["n_kp"])] if not k["synthesized"]}
