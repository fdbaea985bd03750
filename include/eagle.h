/*
 * eagle.h — C ABI of the MI355X-native per-frame inference path for nreHieW/Eagle.
 *
 * The reference has no plugin / FFI interface: the path is reached through three Python call
 * sites of eagle/models/coordinate_model.py, which are the seams this library replaces:
 *   (1) detector      self.detector_model(frame, verbose=False, conf=low_conf)[0].boxes   cm.py:568-572
 *   (2) keypoints     self.keypoint_model.get_keypoints(batch)                            cm.py:226,253,492
 *                                                                                         kh.py:575-595
 *   (3) homography    cv2.findHomography / cv2.perspectiveTransform                       cm.py:355,383,400-403
 * and the per-frame loop body that strings them together (cm.py:277-415) in the stateless configuration
 * (keypoint_interval = homography_interval = 1, tracker off: IDs = detection index, cm.py:598-627).
 *
 * Conventions: every function returns 0 on success or a negative EAGLE_E_* code and never throws; the caller
 * owns the `bgr` and `out` host buffers; the library owns all device memory and streams; one handle per
 * (process, GPU); a handle is not thread-safe; different handles are independent.
 * Plain pointers and sizes only — no torch / numpy types cross this boundary.
 */
#ifndef EAGLE_H
#define EAGLE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EAGLE_OK 0
#define EAGLE_E_INVALID (-1)   /* bad argument */
#define EAGLE_E_HIP (-2)       /* HIP runtime error (see eagle_last_error) */
#define EAGLE_E_STATE (-3)     /* call order: weights not finalized, etc. */
#define EAGLE_E_MISSING (-4)   /* a required weight tensor was never loaded */
#define EAGLE_E_NOKERNEL (-5)  /* no kernel instance for a layer shape */
#define EAGLE_E_COMM (-6)      /* RCCL error */
#define EAGLE_E_RANGE (-8)     /* EAGLE_PREC_F32S: activations left the tensor format's range (|v| > 4094) and were clipped.  The records ARE written
                                  (EagleFrameResult.pad[1] = 1 marks the frames) but are not fp32-grade; see EagleConfig.allow_saturation */

#define EAGLE_MAX_DET 300      /* ultralytics max_det */
#define EAGLE_N_LANDMARKS 57   /* eagle/utils/pitch.py:1-60 */
#define EAGLE_MAX_KP 87        /* 57 detected + at most 30 synthesised (cm.py:140) */

#define EAGLE_PREC_F16 0       /* fp16 tensors, fp32 accumulate on v_mfma_f32_16x16x32_f16 (fast path) */
#define EAGLE_PREC_F32 1       /* fp32 tensors on v_mfma_f32_16x16x4_f32: bit-exact vs the oracle's fmaf chain */
#define EAGLE_PREC_F32S 2      /* fp32-grade: every tensor value as a (hi, lo) pair of binary16 numbers (4 bytes, 22+ significant bits), products as
                                  three v_mfma_f32_16x16x32_f16 (hi*hi + hi*lo + lo*hi) into an fp32 accumulator: the error of an fp32 summation in
                                  another order, at 3/16 of the fp32 MFMA's cost per product */

#define EAGLE_AUTO (-1)          /* EagleConfig::use_graph / multi_stream: chosen from `batch` by eagle_create (eagle_resolve_config) */
#define EAGLE_SMALL_BATCH 32     /* steps of at most this many frames replay their network phase as a hipGraph unless the caller says otherwise (8 until the middle of round 6:
                                    with the branch streams' schedule the replay now pays in one-step calls up to 50 frames, +11 % at 8, +5 % at 16, +3 % at 25, +2 % at 32) */
/* (EAGLE_MULTI_STREAM_BATCH, rounds 5 - 6a: branch streams only up to 16 frames per step.  Since the fuse outputs run on parallel streams they pay at every batch: "auto" = on) */
#define EAGLE_DET_PREC_AUTO (-1) /* EagleConfig::det_precision: chosen from `precision` by eagle_create */
#define EAGLE_DET_PREC_MIXED 4   /* EagleConfig::det_precision: the detector's trunk in EAGLE_PREC_F32S; the last C2f of every level (model.15 / 18 / 21), model.16 / 19 and
                                    Detect in EAGLE_PREC_F32.  Measured and NOT the default: it does not keep the exact family's detection ids */

#define EAGLE_LETTERBOX_RECT 0
#define EAGLE_LETTERBOX_SQUARE 1

#define EAGLE_DET_N 0
#define EAGLE_DET_S 1
#define EAGLE_DET_M 2
#define EAGLE_DET_L 3
#define EAGLE_DET_X 4

typedef struct EagleHandle EagleHandle;

/* Replaces the constructor arguments of CoordinateModel (cm.py:49-74) and the constants of cm.py:18-20,567. */
typedef struct EagleConfig {
    int32_t device;            /* HIP device ordinal */
    int32_t frame_h, frame_w;  /* e.g. 720, 1280 */
    int32_t det_variant;       /* EAGLE_DET_* */
    int32_t det_imgsz;         /* 640 (detector_medium/large) or 960 (detector_large_hd), README.md:107-111 */
    int32_t batch;             /* frames processed per device step (>= 1) */
    int32_t precision;         /* EAGLE_PREC_* */
    double keypoint_conf;      /* 0.3   cm.py:49  (double: the reference compares Python floats) */
    double detector_conf;      /* 0.35  cm.py:49 */
    double ransac_thresh;      /* 5.0   cm.py:355 */
    float detector_floor;      /* 0.15  cm.py:567 (compared in fp32 by ultralytics) */
    float nms_iou;             /* 0.7   ultralytics default */
    int32_t ransac_max_iters;  /* 2000  cv2 default */
    int32_t lm_iters;          /* 10    cv2 default */
    int32_t use_graph;         /* 1: capture the per-batch step into a hipGraph and replay it; 0: plain launches; 2: replay only inside calls of at least three
                                  steps (the graph launch of a step then hides behind the previous step on the GPU; a one-step call of a large batch would pay it
                                  up front; a capture costs ~80 ms per (slot, frame count), once); EAGLE_AUTO (default): 1 when batch <= EAGLE_SMALL_BATCH (the per-frame
                                  use of the reference's loop, cm.py:277), else 0 */
    int32_t det_precision;     /* 0: the detector runs in `precision`; EAGLE_PREC_* + 1: that family for the detector alone; EAGLE_DET_PREC_AUTO (what
                                  eagle_default_config sets; resolved by eagle_create): EAGLE_PREC_F32 + 1 when `precision` is EAGLE_PREC_F32S — key-points
                                  in the split family, the detector (1.4 % of the FLOP with yolov8n) in the exact fp32 family, so that boxes, confidences,
                                  classes, NMS order and detection-index ids are the fp32 oracle's bit for bit — and 0 for any other `precision` (a caller
                                  that takes the defaults and only sets precision = EAGLE_PREC_F16 gets BOTH networks in the fast family) */
    int32_t allow_saturation;  /* EAGLE_PREC_F32S: 0 (default): a call in which an activation store was clipped at +-4094 returns EAGLE_E_RANGE;
                                  1: it returns EAGLE_OK and only flags the frames (EagleFrameResult.pad[1]) and counts them (EagleTimings) */
    int32_t multi_stream;      /* 1: HRNet's branches — and, behind their join, the outputs of its fuse layers — on their own HIP streams inside a step;
                                  0: one stream per network; EAGLE_AUTO (default): 1 (every batch since round 6: +13 % at 12 - 16 frames per step, +1.6 %
                                  at 50; EAGLE_MULTI_STREAM=0 in the environment resolves "auto" to 0) */
    int32_t letterbox;         /* detector input geometry (ultralytics LetterBox): EAGLE_LETTERBOX_RECT (0, default) = auto=True, what the .pt predictor
                                  of cm.py:56-57 does — pad only to the next multiple of 32 (1280x720 @640 -> 384 x 640, 5040 anchors);
                                  EAGLE_LETTERBOX_SQUARE (1) = auto=False, what the exported ONNX detector of the reference's CPU default runs with (cm.py:54-55,
                                  detector_medium.onnx: a static det_imgsz x det_imgsz input — 1280x720 @640 -> 640 x 640, rows 140 / 140 of grey padding, 8400 anchors) */
    int32_t reserved[3];
} EagleConfig;

typedef struct EagleDet {      /* one row of boxes.xyxy/.conf/.cls after NMS (cm.py:569-572) + cm.py:598-627 */
    float x1, y1, x2, y2;      /* float boxes in frame pixels, descending-confidence order */
    float conf;
    int32_t cls;               /* 0 Player 1 Goalkeeper 2 Ball 3 Referee 4 Staff (cm.py:61) */
    int32_t id;                /* Player/Goalkeeper: detection index; Ball: enumerate index; -1 otherwise */
    int32_t bx1, by1, bx2, by2;/* "BBox" ints (truncated, clipped for persons) */
    int32_t foot_x, foot_y;    /* "Bottom_center" */
    float pitch_xf, pitch_yf;  /* perspectiveTransform output before .astype(int) */
    int32_t pitch_x, pitch_y;  /* "Transformed_Coordinates" (valid iff in_bounds) */
    uint8_t reported;          /* 1: appears in the reference dict (class kept and conf >= detector_conf) */
    uint8_t in_bounds;         /* 1: H valid and 0<=X<=105, 0<=Y<=68 */
    uint8_t pad[2];
} EagleDet;

typedef struct EagleKeypoint {
    int32_t label;             /* heat-map index 0..56 (label string via eagle/utils/pitch.py:1-60) */
    int32_t x, y;              /* image pixels */
    float score;               /* sigmoid maximum; 0 for synthesised points */
    uint8_t synthesized;       /* 1: added by the line-intersection synthesis (cm.py:140-186) */
    uint8_t on_plane;          /* 1: handed to findHomography (cm.py:338-347) */
    uint8_t inlier;            /* 1: RANSAC inlier (cm.py:359-362); "Keypoints" = inliers when H_valid */
    uint8_t pad;
} EagleKeypoint;

/* Fixed-size per-frame record == res[i] of cm.py:415 (schema docs/data.md:20-41). */
typedef struct EagleFrameResult {
    int32_t n_det;
    int32_t n_kp;
    int32_t n_candidates;      /* boxes above detector_floor before NMS */
    uint8_t H_valid;
    uint8_t bounds_valid;
    uint8_t pad[2];            /* pad[0]: clip sessions, see eagle_clip_fetch; pad[1] = 1: EAGLE_PREC_F32S clipped an activation of this frame (EAGLE_E_RANGE) */
    double H[9];               /* row-major, h33 = 1 */
    double bounds[4];          /* x of [bottom_left(y=0), top_left(68), top_right(68), bottom_right(0)] */
    int32_t hm_idx[EAGLE_N_LANDMARKS];   /* first-maximum flat index per heat-map (kh.py:588) */
    float hm_score[EAGLE_N_LANDMARKS];   /* kh.py:589 */
    EagleKeypoint kp[EAGLE_MAX_KP];
    EagleDet det[EAGLE_MAX_DET];
} EagleFrameResult;

/* sizeof(EagleConfig), sizeof(EagleFrameResult), sizeof(EagleDet), sizeof(EagleKeypoint): binding self-check */
int eagle_abi_sizes(int32_t* out4);
int eagle_default_config(EagleConfig* cfg);
int eagle_create(const EagleConfig* cfg, EagleHandle** out);
void eagle_destroy(EagleHandle* h);
const char* eagle_last_error(EagleHandle* h);   /* h may be NULL: last error of eagle_create */
int eagle_resolve_config(EagleConfig* cfg);     /* in place, no GPU needed: what eagle_create will make of the "auto" fields (det_precision).  EAGLE_E_INVALID
                                                   (as eagle_create; message: eagle_last_error(NULL)) for a detector geometry with more anchors per frame than the
                                                   NMS kernel sorts (16384: e.g. letterbox square with det_imgsz 960 has 18900) */
int eagle_get_config(EagleHandle* h, EagleConfig* cfg);   /* the handle's configuration as eagle_create resolved it (det_precision no longer "auto") */

/* Weights: state-dict tensors by their reference names, fp32, PyTorch layouts
 *   HRNet + head: "unnormalized_model.0.<...>", "unnormalized_model.1.{weight,bias}" (kh.py:559-562)
 *   detector:     ultralytics "model.<N>.<...>"                                       (cm.py:54-57)
 * eagle_finalize_weights folds BatchNorm, re-tiles for MFMA and builds the per-batch launch schedule. */
int eagle_load_weights(EagleHandle* h, const char* name, const float* data, const int64_t* shape, int ndim);
int eagle_finalize_weights(EagleHandle* h);

/* The hot path: n BGR uint8 HWC frames (host memory) -> n records.  frame_stride / row_stride in bytes, 0 = dense ([n, h, w, 3] contiguous); a
 * row_stride below 3 * frame_w, a frame_stride below (frame_h - 1) * row_stride + 3 * frame_w or a negative stride is EAGLE_E_INVALID.  This is the call that replaces the reference's
 * per-frame loop over host frames (cm.py:277; frames come from eagle/utils/io.py::read_video).  The upload of batch k+1 overlaps the
 * networks of batch k.  Frames in pinned memory (eagle_host_alloc) are DMA'd in place; frames in pageable memory are first copied into a
 * pinned ring by a few worker threads of the handle (EAGLE_COPY_THREADS, default 8).  A video decoder writes 4:2:0, not BGR: its frames go to
 * eagle_process_frames_yuv below, and pinned memory is what the decoder should write into there too. */
int eagle_process_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t frame_stride, int64_t row_stride,
                         EagleFrameResult* out);
int eagle_host_alloc(EagleHandle* h, int64_t bytes, void** ptr);   /* pinned host memory for frames */
int eagle_host_free(EagleHandle* h, void* ptr);

/* Same, inputs already resident in HBM (device pointer, dense [n,h,w,3]); records still land on the host.
 * bench.py reports this entry as `resident`; its `value` is eagle_process_frames from pageable host memory. */
int eagle_process_device_frames(EagleHandle* h, const void* d_bgr, int n, EagleFrameResult* out);
int eagle_device_alloc(EagleHandle* h, int64_t bytes, void** dptr);
int eagle_device_free(EagleHandle* h, void* dptr);
int eagle_device_upload(EagleHandle* h, void* dptr, const void* src, int64_t bytes);

/* ---- decoder-native input: 4:2:0 frames as video decoders emit them ------------------------------------------------------------------
 * EAGLE_PIX_NV12: a Y plane, then one plane of interleaved U V at half resolution (hardware decoders: VCN through VA-API, FFmpeg's hwaccel paths).
 * EAGLE_PIX_I420: a Y plane, then a U plane, then a V plane at half resolution (libavcodec yuv420p, PyAV's to_ndarray()).
 * Each frame is converted on the GPU (yuv.hip) to exactly the BGR bytes of cv2.cvtColor(yuv, COLOR_YUV2BGR_NV12 / _I420) — OpenCV's integer
 * BT.601 limited-range path, one chroma sample per 2x2 block — so every record equals that of eagle_process_frames on those BGR frames.
 * frame_h and frame_w must be even.  A layout field of 0 takes the dense default: y_pitch = w, c_offset = y_pitch * h, c_pitch = w (NV12) or w / 2
 * (I420), v_offset = c_offset + c_pitch * h / 2, frame_stride = the end of the last plane.  A negative field, a pitch below its plane's row, planes
 * that overlap within a frame or a frame_stride below the frame's extent is EAGLE_E_INVALID (eagle_last_error says which). */
#define EAGLE_PIX_NV12 1
#define EAGLE_PIX_I420 2
typedef struct EagleYuvLayout {      /* bytes; 0 = the dense default for that field */
    int64_t frame_stride;            /* frame k starts at src + k * frame_stride */
    int64_t y_pitch;                 /* Y rows (h rows of w bytes) */
    int64_t c_offset;                /* first chroma plane (NV12: UV; I420: U) from the frame start */
    int64_t c_pitch;                 /* chroma rows (h/2 rows of w bytes for NV12, w/2 for I420) */
    int64_t v_offset;                /* I420 only: V plane from the frame start, same c_pitch */
} EagleYuvLayout;
/* n frames in host memory -> n records, as eagle_process_frames.  Pinned source (eagle_host_alloc: a decoder's output surface): the planes are
 * DMA'd from it; pageable source: worker threads first pack them into a pinned ring.  The conversion writes the step's BGR staging buffer, so a
 * YUV call of n frames replays the hipGraph a BGR call of n frames captured.  layout NULL: dense. */
int eagle_process_frames_yuv(EagleHandle* h, int format, const uint8_t* src, int n, const EagleYuvLayout* layout, EagleFrameResult* out);
/* Same, the frames already in HBM (a hardware decoder's device surface, read in place with its layout). */
int eagle_process_device_frames_yuv(EagleHandle* h, int format, const void* d_src, int n, const EagleYuvLayout* layout, EagleFrameResult* out);
/* Device to device: n frames of the handle's size -> d_bgr, a dense [n, h, w, 3] buffer of the caller (eagle_device_alloc).  For the entries that
 * take a BGR clip resident in HBM: eagle_clip_open, eagle_reid_features, eagle_team_colors.  Returns when the conversion is done. */
int eagle_yuv_to_bgr(EagleHandle* h, int format, const void* d_src, int n, const EagleYuvLayout* layout, void* d_bgr);
/* Operator entry (host buffers in / out, parity tests): n frames of h x w -> bgr [n, h, w, 3]. */
int eagle_op_yuv_to_bgr(int device, int format, const uint8_t* src, int n, int h, int w, const EagleYuvLayout* layout, uint8_t* bgr);

/* ---- annotated output: the frames with the records drawn on them, in the layout a video encoder takes ---------------------------------------
 * What the reference's main.py:43-81 draws into annotated.mp4, its one validation aid: a foot ellipse with a gap and the id per player in the
 * team colour, a triangle above the ball, a disc per pitch key-point.  One kernel launch (annotate.hip) reads the clip resident in HBM (it stays
 * untouched), draws and writes BGR, NV12 or I420; the 4:2:0 outputs are converted from the drawn pixels in registers.  The rasterisation is this
 * library's own (tests/annot_ref.py defines every pixel: integer ellipse outline, 5 x 7 bitmap digits; NOT cv2.ellipse / cv2.putText pixels);
 * BGR -> 4:2:0 is OpenCV's integer BT.601 limited-range path of COLOR_BGR2YUV_I420, chroma taken from the even-row even-column pixel of each 2 x 2 block.
 * An overlay is an ordered list of primitives; a pixel takes the colour of the LAST primitive covering it; primitives are clipped to the frame.
 *   EAGLE_PRIM_ARC    a = {cx, cy}                    outline of the ellipse of half-axes 35 x 18, open at the top (parametric angles 235 .. 315 degrees)
 *   EAGLE_PRIM_LABEL  a = {x, y, id}                  decimal digits of id (0 .. 99999, else nothing), 10 x 14 glyphs, bottom-left pixel at (x - 3, y)
 *   EAGLE_PRIM_DISC   a = {cx, cy, r}                 filled, 0 <= r <= 16384
 *   EAGLE_PRIM_TRI    a = {x0, y0, x1, y1, x2, y2}    filled, edges inclusive
 * Coordinates are frame pixels, |coordinate| <= 2^20.  Output layout: EagleYuvLayout with the rules above (0 = dense, EAGLE_E_INVALID for negative
 * fields, short pitches, overlapping planes, odd frame sizes for 4:2:0); EAGLE_PIX_BGR is an output format only: dense or pitched [h][w][3],
 * layout->y_pitch = row pitch, layout->frame_stride, the other fields unused.  Bytes between rows, planes and frames are left untouched. */
#define EAGLE_PIX_BGR 0
#define EAGLE_PRIM_ARC 0
#define EAGLE_PRIM_LABEL 1
#define EAGLE_PRIM_DISC 2
#define EAGLE_PRIM_TRI 3
#define EAGLE_MAX_PRIMS (2 * EAGLE_MAX_DET + EAGLE_MAX_KP + 1)     /* per frame: two per detection, the key-points, one ball */
typedef struct EaglePrim { int32_t kind; int32_t a[6]; uint8_t b, g, r, pad; } EaglePrim;
/* n frames of a BGR clip resident in HBM (dense [n, h, w, 3] of the handle's size) + their records -> n annotated frames in HBM (a buffer of the
 * caller: eagle_device_alloc, or an encoder's input surface with its layout).  team_ids / team_vals: Processor.get_team_mapping as two arrays of
 * n_team entries (team 0 red, any other blue; goalkeepers green; players without an entry are not drawn, main.py:64-65); team_ids NULL: every
 * player white.  Runs on the handle's main stream behind whatever is enqueued and returns when the output is complete; the step's graphs and
 * staging buffers are not involved. */
int eagle_annotate_device_frames(EagleHandle* h, const void* d_bgr, int n, const EagleFrameResult* recs, const int32_t* team_ids,
                                 const int32_t* team_vals, int n_team, int out_format, const EagleYuvLayout* out_layout, void* d_out);
/* Same, the result copied to host memory (pinned: DMA'd; pageable: through a pinned ring of the handle). */
int eagle_annotate_frames(EagleHandle* h, const void* d_bgr, int n, const EagleFrameResult* recs, const int32_t* team_ids,
                          const int32_t* team_vals, int n_team, int out_format, const EagleYuvLayout* out_layout, uint8_t* out);
/* What a record's overlay is (no GPU involved), for callers that draw themselves and for the tests: persons in detection order (ARC + LABEL at
 * the foot point), the marker of the first reported ball, a black disc of radius 6 per key-point of the reference dict (the RANSAC inliers when
 * H_valid, else all).  cap >= EAGLE_MAX_PRIMS always suffices; a smaller cap that does not is EAGLE_E_INVALID. */
int eagle_overlay_from_record(const EagleFrameResult* rec, const int32_t* team_ids, const int32_t* team_vals, int n_team, EaglePrim* out,
                              int cap, int* n_out);
/* Operator entry (host buffers in / out, no handle): arbitrary primitive lists, frame k owns prims[prim_offsets[k] .. prim_offsets[k + 1]) (at most
 * EAGLE_MAX_PRIMS); every list empty = the plain conversion.  `out` is read first, so bytes the layout does not cover come back as they were. */
int eagle_op_annotate(int device, const uint8_t* bgr, int n, int h, int w, const EaglePrim* prims, const int32_t* prim_offsets /* n + 1 */,
                      int out_format, const EagleYuvLayout* out_layout, uint8_t* out);

/* As eagle_annotate_frames with the primitive lists given by the caller (eagle_op_annotate's convention: frame k owns prims[prim_offsets[k] ..
 * prim_offsets[k + 1]), at most EAGLE_MAX_PRIMS) instead of derived from records: how a processed table's rows are drawn (eagle_overlay_from_table). */
int eagle_annotate_frames_prims(EagleHandle* h, const void* d_bgr, int n, const EaglePrim* prims, const int32_t* prim_offsets /* n + 1 */, int out_format,
                                const EagleYuvLayout* out_layout, uint8_t* out);

/* ---- the clip post-processor: Processor.process_data / format_data of eagle/processor.py:30-403, what main.py:34-41 writes as raw_data.json and
 * processed_data.json and draws the annotated video from ------------------------------------------------------------------------------------
 * eagle_postprocess takes the n records of a finished clip (record i = frame i) and builds the reference's table on the GPU: one row per frame with
 * at least one Player / Goalkeeper, one column per boundary corner, per {Player, Goalkeeper} id and its video point, and Ball / Ball_video, in the
 * reference's column order; ids seen in fewer than 1 % of the rows dropped; the ball chosen per frame by parse_ball_detections_with_kalman(filter =
 * False) and filled linearly to both ends; Player_k folded into Goalkeeper_k (combine_first); every column interpolated linearly over row POSITIONS
 * inside its valid span; with `smooth` every other row, from the first, replaced by the interpolation of its neighbours.  The arithmetic is pandas'
 * (np.interp in float64: slope * (x - x0) + y0, no contraction), pinned bit for bit by tests/golden/post_golden.json through tests/post_ref.py.  The
 * reference's pairwise id merge (proc.py:218-319) never merges as written (its overlap test holds for any two non-empty columns) and is reproduced
 * as that by default: nothing.  merge_ids = 1 runs the merge it was meant to be, as a rule of this library's own (contract: tests/stitch_ref.py), at
 * the reference's place: after the 1 % filter, the ball fill and the goalkeeper fold, before interpolation and smoothing.  A track is a person video
 * column after the fold, first / last its first and last present row.  A link a -> b is admissible when both are of one kind, last(a) < first(b), the
 * gap in FRAME numbers g = frame[first(b)] - frame[last(a)] is at most (int)(fps * 1.1), the video points p_last(a) and p_first(b) lie at most 10 g
 * pixels apart (sqrt(dx*dx + dy*dy) in float64, no contraction) and the two ids do not have different teams in the mapping.  The admissible links
 * are walked ascending by (distance, g, column of a, column of b); one is accepted when a has no successor, b no predecessor and the teams known
 * for the two chains do not differ.  A chain becomes one pitch and one video column under the id, kind and position of its head (the member without
 * predecessor; a pitch column exists when a member has one); a cell holds the value of the member present in that row; the other members' columns
 * leave the table; interpolation fills the gaps between fragments linearly.  A head without a team entry inherits the team known for its chain
 * (the table's mapping grows: eagle_overlay_from_table, the minimap and pitch control colour the whole track; an entry below 0 counts as none and is replaced).
 * eagle_post_merges lists the accepted links.  Host C++ discovers columns and walks the ball; two launches (post.hip) on the handle's main stream build the table, which stays
 * resident in HBM until eagle_post_free.  The handle's records, staging buffers and graphs are not involved.
 * Where the reference raises or returns garbage, the library is defined instead:
 *   - fewer than two ball sightings (the reference hands its candidate lists on and fails later): Ball / Ball_video are all NaN, EAGLE_POST_NO_BALL is set;
 *   - the boundary columns and Ball / Ball_video are always kept (the reference's 1 % filter can drop them; its format_data then raises KeyError);
 *   - the goalkeeper fold of an id needs all four of its columns (the reference raises KeyError when Goalkeeper_<id> was dropped by the filter);
 *   - a clip without a kept frame gives a table of 0 rows and 0 columns (the reference: an empty frame; it raises on a clip of no frames);
 *   - non-finite boundary values count as missing;
 *   - filter_ball != 0 (filter_ball_detections=True) is refused with EAGLE_E_INVALID: it needs cv2's SVD-based Kalman gain, which nothing here pins.
 * Unpinned: with several ball candidates the nearest to cv2.KalmanFilter.predict() wins; predict is taken to compute statePre = F * statePost from a
 * zero statePost (the reference sets statePre only), so without correct() the prediction stays at the origin (tests/post_ref.py::kalman_predict).
 * More than 2^20 kept frames, or a table beyond the memory budget (max_bytes; 0: nine tenths of the device's free memory), is EAGLE_E_INVALID with
 * the sizes in the message, before anything is launched. */
#define EAGLE_POST_PLAYER 0
#define EAGLE_POST_GOALKEEPER 1
#define EAGLE_POST_BALL 2
#define EAGLE_POST_BOUNDARY 3      /* id 0 .. 3: Bottom_Left, Top_Left, Top_Right, Bottom_Right */
#define EAGLE_POST_NO_BALL 1       /* flag: fewer than two ball sightings, the ball columns are all NaN */
typedef struct EaglePostTable EaglePostTable;
typedef struct EaglePostParams {
    int32_t fps;                   /* > 0 (the id merge's temporal threshold is (int)(fps * 1.1) frames) */
    int32_t frame_w;               /* > 0 (the refused ball filter's threshold, 0.1 * width) */
    int32_t smooth;                /* process_data(smooth=...) */
    int32_t filter_ball;           /* must be 0 */
    const int32_t* team_ids;       /* Processor.get_team_mapping as two arrays of n_team entries: kept with the table for eagle_overlay_from_table; */
    const int32_t* team_vals;      /* team_ids NULL: no mapping (players drawn white) */
    int32_t n_team;
    int32_t merge_ids;             /* 0: the reference as written (no id ever merges); 1: stitch fragmented ids (rule above); else EAGLE_E_INVALID */
    int64_t max_bytes;             /* device-memory budget of the call, 0 = nine tenths of what is free */
} EaglePostParams;
typedef struct EaglePostColumn { int32_t kind /* EAGLE_POST_* */, id, video /* 1: the "_video" column */, reserved; } EaglePostColumn;
int eagle_postprocess(EagleHandle* h, const EagleFrameResult* recs, int n, const EaglePostParams* p, EaglePostTable** out);
void eagle_post_free(EaglePostTable* t);
int eagle_post_shape(const EaglePostTable* t, int32_t* rows, int32_t* cols, int32_t* flags);                 /* any pointer may be NULL */
int eagle_post_layout(const EaglePostTable* t, int32_t* frames /* rows: kept frame numbers */, EaglePostColumn* columns /* cols, table order */);
int eagle_post_values(EaglePostTable* t, double* values /* [cols][rows][2] = x, y; NaN = missing */);        /* copies the table to the host */
int eagle_post_device_values(const EaglePostTable* t, const double** d_values);                              /* the same layout, in HBM */
/* The links the id merge accepted, in acceptance order: ids from_id -> to_id of `kind` were joined over gap_frames frames and dist pixels; head_id and
 * team (-1: unknown) are those of the finished chain.  *n = their number (0 for a table built with merge_ids = 0); at most cap are written. */
typedef struct EaglePostMerge { int32_t kind /* EAGLE_POST_PLAYER | _GOALKEEPER */, from_id, to_id, head_id, gap_frames, team; double dist; } EaglePostMerge;
int eagle_post_merges(const EaglePostTable* t, EaglePostMerge* out, int cap, int* n);
/* The overlay main.py:44-77 draws for processed row `row` (no launch; the table is copied to the host once): per video column in table order the
 * foot arc and id at (int(x), int(y)) — goalkeepers green, team 0 red, other teams blue, players without a team skipped (white without a mapping) —
 * the marker above the interpolated ball, then, with rec != NULL, that record's key-point discs (the three sources of eagle_overlay_from_record). */
int eagle_overlay_from_table(EaglePostTable* t, int row, const EagleFrameResult* rec, EaglePrim* out, int cap, int* n_out);

/* ---- the minimap: rows of a processed table as top-down pictures of the pitch (the reference's examples/minimap.py and examples/voronoi.py) ------------
 * Per row: a black canvas of w = 105 scale + 2 margin by h = 68 scale + 2 margin pixels (pitch y up, so the canvas flips it); with `voronoi` the pitch
 * rectangle tinted by the team colour of the nearest Player column (goalkeepers are not sites; exact integer distances, ties to the earlier column); with
 * `footprint` the camera's view (the triangles Bottom_Left, Top_Left, Top_Right and Bottom_Left, Top_Right, Bottom_Right of the boundary columns)
 * blended with white; the pitch markings; a disc per Player / Goalkeeper pitch column in table order in the colours of the annotated video (goalkeepers
 * green, team 0 red, any other team blue, players without a mapping entry not drawn, white without a mapping); the ball as a white ring, last.
 * Positions are quantised once to 1/16 pixel in float64; cells that are NaN, infinite or further than 1024 m from the origin are absent, any absent
 * corner drops the footprint of that row.  The rasterisation is this library's own: tests/minimap_ref.py defines every output byte, the 4:2:0
 * conversion and the output layouts are those of the annotated output above.  Two launches (minimap.hip) on the handle's main stream read the table
 * where eagle_postprocess left it; the handle's records, staging buffers and graphs are not involved.
 * EAGLE_E_INVALID with a message, before any launch: NULL pointers, scale odd or outside 2 .. 32, margin odd or outside 0 .. 64, a radius negative or
 * above 4 scale, voronoi with a table that has no team mapping, control together with voronoi or without what it needs (below), n < 0, a row window outside the table (a table of 0 rows with n > 0), and every layout
 * error eagle_annotate_* refuses.  n == 0 is success and writes nothing. */
typedef struct EagleMinimapParams {
    int32_t scale;                 /* pixels per metre: even, 2 .. 32 */
    int32_t margin;                /* pixels around the pitch: even, 0 .. 64 */
    int32_t voronoi, footprint;    /* != 0: draw that layer */
    int32_t player_radius;         /* pixels, 0 .. 4 scale; 0 = max(2, scale) */
    int32_t ball_radius;           /* outer radius of the ring, pixels, 0 .. 4 scale; 0 = max(3, scale / 2 + 1); the ring is max(1, radius / 3) thick */
    int32_t control;               /* != 0: draw the pitch-control layer in Voronoi's slot (below: eagle_minimap_set_control); refused together with voronoi */
    int32_t layers;                /* bit mask of EAGLE_MM_* (below: eagle_minimap_set_trails, eagle_minimap_set_hulls); 0: none of them, the minimap as it is without them */
} EagleMinimapParams;
int eagle_minimap_size(const EagleMinimapParams* p, int* w, int* h);
/* rows row0 .. row0 + n - 1 -> n pictures in HBM (a buffer of the caller: eagle_device_alloc, or an encoder's input surface with its layout); returns when
 * the output is complete */
int eagle_minimap_device_frames(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleMinimapParams* p, int out_format, const EagleYuvLayout* out_layout,
                                void* d_out);
/* Same, the result copied to host memory (pinned: DMA'd; pageable: through a pinned ring of the handle). */
int eagle_minimap_frames(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleMinimapParams* p, int out_format, const EagleYuvLayout* out_layout,
                         uint8_t* out);
/* Operator entry (host buffers in / out, no handle) for constructed tables: values [cols][rows][2], columns as eagle_post_layout gives them, the team
 * mapping as two arrays (team_ids NULL: no mapping).  `out` is read first, so bytes the layout does not cover come back as they were. */
int eagle_op_minimap(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals,
                     int n_team, const EagleMinimapParams* p, int row0, int n, int out_format, const EagleYuvLayout* out_layout, uint8_t* out);

/* ---- kinematics and pitch control: what a processed table says about movement (own specification: tests/control_ref.py defines every output bit) -------
 * VELOCITIES, float64 without contraction, for every column of the table in its layout [cols][rows][2] (video columns in px/s).  A cell is present
 * when x and y are finite; the neighbour row r - 1 (r + 1) is usable when it is present and at most max_gap frames away; both usable: the central
 * difference (p[r + 1] - p[r - 1]) / ((f[r + 1] - f[r - 1]) / fps); one: the one-sided difference; none: (0, 0); an absent cell: (NaN, NaN); a speed
 * above speed_cap is scaled back to it.  One launch (post.hip); the result is kept with the table until eagle_post_free and replaces an earlier one.
 * CONTROL GRID, float32 without contraction: per row cells_per_metre (1, 2 or 4) cells per metre, gw = 105 R by gh = 68 R bytes, grid row 0 at pitch
 * y = 0.  The sites are the minimap's Voronoi sites (Player pitch columns with a team entry, present, within 1024 m; a mapping is required).  A site
 * reacts for t_react seconds at its velocity (q = p + v t_react in fp32, a non-finite velocity component counts as 0, q clamped to +-2^20) and then
 * runs at v_max: t_i = t_react + |cell - q| / v_max.  A cell's byte is floor(255 num / den + 0.5) with w_i = exp(-beta (t_i - min t)), num the sum of w_i
 * over team 0 and den over all sites in table order; 128 everywhere for a row without sites.  d_share[i] is the exact sum of row i's bytes (the team-0
 * area share is that over 255 gw gh).  Two launches (control.hip) on the handle's main stream.  The constants are conventional choices (0.7 s, 5 m/s,
 * 4 / s, a 12 m/s cap), not fitted to data.
 * EAGLE_E_INVALID with a message, before any launch: NULL pointers, fps, max_gap or speed_cap not positive (or speed_cap not finite), cells_per_metre
 * outside {1, 2, 4}, t_react outside 0 .. 1000, v_max outside 0.001 .. 1e6, beta outside (0, 1e6], a table without a team mapping, a table without
 * velocities, a row window outside the table, frames of an operator entry that do not ascend.  n == 0 is success and writes nothing. */
typedef struct EagleKinematicsParams {
    int32_t fps;                   /* > 0: frames per second of the frame numbers */
    int32_t max_gap;               /* > 0: a neighbour row further than this many frames away is not differenced (a usual choice: fps) */
    double speed_cap;              /* > 0, finite: m/s (px/s for video columns) */
    int64_t reserved;
} EagleKinematicsParams;
typedef struct EagleControlParams {
    int32_t cells_per_metre;       /* 1, 2 or 4 */
    float t_react, v_max, beta;    /* seconds, m/s, 1/s */
    int32_t reserved[4];
} EagleControlParams;
int eagle_post_velocities(EagleHandle* h, EaglePostTable* t, const EagleKinematicsParams* p);
int eagle_post_velocity_values(EaglePostTable* t, double* values /* [cols][rows][2] */);                     /* copies the velocities to the host */
int eagle_post_device_velocity_values(const EaglePostTable* t, const double** d_values);                     /* NULL before eagle_post_velocities */
int eagle_control_size(const EagleControlParams* p, int* gw, int* gh);
/* rows row0 .. row0 + n - 1 -> n grids [n][gh][gw] and, with d_share != NULL, n sums in HBM; returns when they are complete */
int eagle_control_device_grids(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleControlParams* p, uint8_t* d_out, int64_t* d_share);
/* Same, to host memory, in passes of what 32 MB of device staging hold. */
int eagle_control_grids(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleControlParams* p, uint8_t* out, int64_t* share);
/* The parameters the minimap's `control` layer is computed with (kept with the table; p NULL: forget them).  The layer needs them, the table's
 * velocities and a team mapping; the grids of a call's rows are computed on its stream in front of the draw launch.  A pixel of the pitch rectangle
 * takes its cell's byte c and, with a = c + (c >> 7), the colour (red a + blue (256 - a) + 128) >> 8, tinted like a Voronoi area. */
int eagle_minimap_set_control(EaglePostTable* t, const EagleControlParams* p);
/* Operator entries (host buffers in / out, no handle) for constructed tables. */
int eagle_op_velocities(int device, const double* values, const int32_t* frames, int rows, int cols, const EagleKinematicsParams* p, double* out);
int eagle_op_control(int device, const double* values, const double* velocities, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                     const int32_t* team_vals, int n_team, const EagleControlParams* p, int row0, int n, uint8_t* out_grid, int64_t* out_share /* may be NULL */);
int eagle_op_minimap_control(int device, const double* values, const double* velocities, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                             const int32_t* team_vals, int n_team, const EagleMinimapParams* p, const EagleControlParams* cp, int row0, int n, int out_format,
                             const EagleYuvLayout* out_layout, uint8_t* out);

/* ---- ball possession and pass events: what a processed table says about the ball (own specification: tests/possession_ref.py defines every output bit) ----
 * float64 without contraction.  The ball is the one Ball pitch column (video == 0), the candidates are the Player and Goalkeeper pitch columns; a cell is
 * present when x and y are finite (the velocity rule).  Per row r:
 *   CANDIDATE  ball[r]: the ball cell is present.  Of the present candidate cells the one with the smallest d2 = dx dx + dy dy (a tie: the earlier
 *              column); cand[r] = its column when the ball is present and d2 <= radius radius (formed once, inclusive), else -1; dist[r] = sqrt(min d2),
 *              NaN without a ball or without a present candidate.
 *   RUNS       seg[r] = r == 0 || frames[r] - frames[r - 1] > max_gap || !ball[r];  head[r] = seg[r] || cand[r] < 0 || cand[r] != cand[r - 1];
 *              headrow[r] = the greatest head row <= r;  run[r] = r - headrow[r] + 1 when cand[r] >= 0, else 0;  conf[r] = cand[r] >= 0 && run[r] >=
 *              min_hold;  lastconf[r] = the greatest confirmed row <= r or -1;  lastseg[r] = the greatest segment start <= r.
 *   OWNER      owner[r] = cand[lastconf[r]] when ball[r] && lastconf[r] >= 0 && lastconf[r] >= lastseg[r], else -1: a person owns the ball from the row
 *              that confirms them (nearest and inside the radius for min_hold consecutive rows), keeps it while it flies or rolls until someone else is
 *              confirmed; a hole in the frame numbers or a row without a ball forgets the owner.
 *   EVENT      at r >= 1 when !seg[r], owner[r] >= 0, owner[r - 1] >= 0 and owner[r] != owner[r - 1]; events are reported in ascending row order.
 * cand, owner, from_col and to_col are COLUMN indices of the table.  A column's team is the first entry of the mapping with its id (an entry below 0 or
 * none: unknown, -1); without a mapping every event is EAGLE_EVENT_UNKNOWN.  A table without a ball column or flagged EAGLE_POST_NO_BALL gives -1 / NaN
 * everywhere and no event.  Three launches (possession.hip) on the handle's main stream read the table where eagle_postprocess left it; the handle's
 * records, staging buffers and graphs are not involved.  radius 2 m, min_hold 2 rows and max_gap = fps are conventional choices, not fitted to data.
 * EAGLE_E_INVALID with a message, before any launch: NULL pointers, fps, max_gap or min_hold not positive, radius not finite, not positive or above
 * 1024, more than one Ball pitch column, a column of unknown kind, frames of the operator entry that do not ascend strictly.  rows == 0 is success and
 * writes nothing. */
#define EAGLE_EVENT_PASS 0         /* both teams known and equal */
#define EAGLE_EVENT_TURNOVER 1     /* both teams known and different */
#define EAGLE_EVENT_UNKNOWN 2      /* a team is unknown */
typedef struct EaglePossessionParams {
    int32_t fps;                   /* > 0: frames per second of the frame numbers (event durations) */
    int32_t min_hold;              /* >= 1: kept rows a candidate must stay nearest and inside the radius to be confirmed */
    int32_t max_gap;               /* > 0: a step of more frames than this starts a new segment (a usual choice: fps) */
    int32_t reserved0;
    double radius;                 /* metres: > 0, finite, at most 1024 */
    int64_t reserved;
} EaglePossessionParams;
typedef struct EaglePossessionEvent {
    int32_t row;                   /* the row whose owner differs from the row before */
    int32_t from_col, to_col;      /* owner[row - 1], owner[row] */
    int32_t release_row;           /* lastconf[row - 1]: the old owner's last confirmed touch */
    int32_t receive_row;           /* headrow[row]: the first row of the new owner's run (= row - min_hold + 1, > release_row) */
    int32_t kind;                  /* EAGLE_EVENT_* */
    int32_t reserved[2];
    double x0, y0, x1, y1;         /* the ball cell at release_row and at receive_row */
    double length;                 /* sqrt(dx dx + dy dy) of the two */
    double duration;               /* (double)(frames[receive_row] - frames[release_row]) / (double)fps, seconds */
} EaglePossessionEvent;            /* 80 bytes */
/* The result is kept with the table until eagle_post_free and replaces an earlier one. */
int eagle_post_possession(EagleHandle* h, EaglePostTable* t, const EaglePossessionParams* p);
int eagle_post_possession_values(EaglePostTable* t, int32_t* cand, int32_t* owner, double* dist);            /* copies [rows] each to the host; any pointer may be NULL */
int eagle_post_device_possession(const EaglePostTable* t, const int32_t** d_owner);                          /* owner[rows] in HBM; NULL before eagle_post_possession */
/* *n = the number of events of the last eagle_post_possession (0 before it); at most cap are written, in row order. */
int eagle_post_events(const EaglePostTable* t, EaglePossessionEvent* out, int cap, int* n);
/* Operator entry (host buffers in / out, no handle) for constructed tables: values [cols][rows][2], frames [rows] strictly ascending, columns as
 * eagle_post_layout gives them, the team mapping as two arrays (team_ids NULL: no mapping).  cand, owner, dist ([rows] each) may be NULL; *n_events = the
 * number of events, of which at most cap are written. */
int eagle_op_possession(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                        const int32_t* team_vals, int n_team, const EaglePossessionParams* p, int32_t* cand, int32_t* owner, double* dist,
                        EaglePossessionEvent* events, int cap, int* n_events);

/* ---- trails, pass arrows and the ball owner in the minimap; the trajectory and the pass still (the reference's examples/trajectory.py and pass.py) ----
 * Own specification: tests/trails_ref.py defines every output byte.  Three more layers of the minimap video, chosen by EagleMinimapParams::layers, drawn
 * between the markings and the discs:
 *   TRAILS  of the selected columns over the last `window` kept rows: on the picture of row r column c draws the segments (j - 1, j), max(1, r - window + 1)
 *           <= j <= r, whose two cells are present (the minimap's rule) and whose frame step is at most max_gap; selection order, the oldest segment first;
 *           a segment of age a = r - j is opaque in (colour * f) >> 8, f = 256 - (a (256 - dim_floor)) / window; the colour is the column's disc colour (a
 *           player without a mapping entry has no trail).  A segment covers the pixels whose squared distance to it is at most (16 half_width)^2 in 1/16
 *           pixel, decided exactly in integers.
 *   PASSES  an arrow per event of eagle_post_possession on the rows release_row <= r < receive_row + pass_hold: white (pass), yellow (turnover) or grey
 *           (unknown), a shaft of the trails' width between the two quantised ball cells and a head 4 half_width long and 2 x 2 half_width wide; either cell
 *           absent: no arrow.
 *   OWNER   a white ring max(1, radius / 3) pixels thick round the disc of eagle_post_possession's owner of the row.
 * The layers need eagle_minimap_set_trails, PASSES and OWNER also eagle_post_possession.  With layers == 0 the output and the two launches are what they
 * are without this section; otherwise the draw is a second instantiation of the kernel behind up to two preparing launches (trails.hip).
 * STILLS, BGR [h][w][3] on the minimap's canvas: the trajectory of a selection over rows row0 .. row0 + n - 1 (markings, the segments undimmed, per column
 * a ring at its first and a disc at its last present cell), and one event at its release row (markings, the arrow, the discs with everyone but passer and
 * receiver blended at a quarter, the ball).
 * EAGLE_E_INVALID with a message, before any launch: a layer bit without eagle_minimap_set_trails, PASSES or OWNER without a possession result, TRAILS with
 * an empty selection, window < 1, half_width outside 1 .. 8, dim_floor outside 0 .. 256, pass_hold < 1, max_gap < 1, a selection member that is out of
 * range, a video or boundary column or repeated, an event outside the event count, a row window outside the table (a still: n < 1), unknown bits in layers,
 * and what the minimap refuses. */
#define EAGLE_MM_TRAILS 1
#define EAGLE_MM_PASSES 2
#define EAGLE_MM_OWNER 4
typedef struct EagleTrailParams {
    int32_t window;                /* >= 1: kept rows a trail looks back */
    int32_t max_gap;               /* >= 1: a step of more frames than this breaks a trail (a usual choice: fps) */
    int32_t half_width;            /* 1 .. 8 pixels: of trails and arrow shafts */
    int32_t pass_hold;             /* >= 1: rows an arrow stays after the receive row */
    int32_t dim_floor;             /* 0 .. 256: the brightness (of 256) the oldest segment fades towards */
    int32_t reserved[3];
} EagleTrailParams;
/* The parameters and the selection are kept with the table (p NULL: forget them); ncols == 0 with p set: passes and owner only. */
int eagle_minimap_set_trails(EaglePostTable* t, const EagleTrailParams* p, const int32_t* cols, int ncols);
int eagle_trajectory_picture(EagleHandle* h, EaglePostTable* t, const int32_t* cols, int ncols, int row0, int n, int scale, int margin, int half_width, int max_gap,
                             uint8_t* out);
int eagle_pass_picture(EagleHandle* h, EaglePostTable* t, int event, int scale, int margin, int half_width, uint8_t* out);
/* Operator entries (host buffers in / out, no handle) for constructed tables, as eagle_op_minimap: frames [rows] strictly ascending, sel [nsel] the selection,
 * owner [rows] or NULL, events [n_events] (ascending release_row and receive_row) or NULL; tp may be NULL when p->layers == 0.  The control layer is not
 * available here. */
int eagle_op_minimap_trails(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                            const int32_t* team_vals, int n_team, const EagleMinimapParams* p, const EagleTrailParams* tp, const int32_t* sel, int nsel,
                            const int32_t* owner, const EaglePossessionEvent* events, int n_events, int row0, int n, int out_format, const EagleYuvLayout* out_layout,
                            uint8_t* out);
int eagle_op_trajectory_picture(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                                const int32_t* team_vals, int n_team, const int32_t* sel, int nsel, int row0, int n, int scale, int margin, int half_width, int max_gap,
                                uint8_t* out);
int eagle_op_pass_picture(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals,
                          int n_team, const EaglePossessionEvent* events, int n_events, int event, int scale, int margin, int half_width, uint8_t* out);

/* ---- team shape per row: members, sums, extrema and the exact convex hull of each team; the minimap's hull layer (own specification: tests/shape_ref.py
 * defines every output bit and byte) ----
 * GROUPS   0 = team value 0, 1 = any other non-negative team value (the minimap's red / blue).  The members of a group are the Player pitch columns
 *          (video == 0) with a mapping entry of that group; a column's team is the first mapping entry with its id (the possession rule).  Goalkeepers,
 *          balls, boundary columns and players without an entry (or with a negative one) are no members.  A mapping is required.  A member is PRESENT on a
 *          row when x and y are finite and |x|, |y| <= 1024 m (the minimap's rule: every hull vertex can be drawn).
 *   QUANTISE qx = (int) floor(x * 1024.0 + 0.5), qy likewise (float64, no contraction; the multiply is exact).  |q| <= 2^20, every product below stays
 *            under 2^45 and is exact in int64; all sums are integers, so no order of accumulation matters.
 *   RECORD   one EagleTeamShape per row and group: n present members, the sums of q and q^2, the extrema and the EARLIEST table column attaining each (0
 *            and -1 when n == 0), hull_n = the true number of hull vertices, area2 = twice the hull's area in q^2 (over all vertices, >= 0).
 *   HULL     int32 [rows][2][EAGLE_SHAPE_HULL_CAP] table columns, counter-clockwise with pitch y up, -1 padded; EAGLE_SHAPE_CUT in flags when hull_n
 *            exceeds the cap.  The start is the present member with the smallest (qy, qx, column).  From the current vertex c the candidates are the
 *            present members whose q differs from q_c; p beats the best so far b when o = (bx - cx)(py - cy) - (by - cy)(px - cx) < 0, or o == 0 and
 *            |p - c|^2 > |b - c|^2, or both are equal and p's column is smaller.  The march ends when the winner is the start, without a candidate, and after
 *            at most n steps.  A point strictly inside an edge is no vertex, coincident points are one (the earliest column); all coincident: hull_n 1;
 *            all collinear: hull_n 2, area2 0.
 *   LAYER    EAGLE_MM_HULLS in EagleMinimapParams::layers: per group (0 first) the stored vertices joined by capsules (the trails' exact rule) of
 *            EagleHullParams::half_width pixels, drawn after the markings and before the trails, opaque, in the group's disc colour scaled (c * 160) >> 8.
 *            hull_n >= 3: the closed polygon, without its closing edge when the list is cut; hull_n == 2: one segment; below: nothing.  It needs
 *            eagle_post_team_shape and eagle_minimap_set_hulls.  eagle_op_minimap_trails cannot carry a shape result and refuses the bit.
 * Two launches (shape.hip) on the handle's main stream read the table where eagle_postprocess left it, a third prepares the layer's edges; the handle's
 * records, staging buffers and graphs are not involved.
 * EAGLE_E_INVALID with a message, before any launch: NULL pointers, a table without a mapping, more than EAGLE_SHAPE_MAX_MEMBERS members over both
 * groups, half_width outside 1 .. 8, the hull bit without a team-shape result or without eagle_minimap_set_hulls, a column of unknown kind, frames of an
 * operator entry that do not ascend strictly, and what the minimap and its other layers refuse.  rows == 0 is success and writes nothing. */
#define EAGLE_MM_HULLS 8
#define EAGLE_SHAPE_HULL_CAP 32
#define EAGLE_SHAPE_MAX_MEMBERS 4096
#define EAGLE_SHAPE_CUT 1          /* EagleTeamShape::flags: the hull has more than EAGLE_SHAPE_HULL_CAP vertices, the stored list holds the first of them */
typedef struct EagleTeamShape {
    int64_t sum_x, sum_y;          /* over the present members, of q */
    int64_t sum_xx, sum_yy;        /* ... of q^2 */
    int64_t area2;                 /* twice the hull's area, q^2 */
    int32_t n;                     /* present members */
    int32_t hull_n;                /* hull vertices (all of them) */
    int32_t flags;                 /* EAGLE_SHAPE_CUT */
    int32_t reserved0;
    int32_t min_x, max_x, min_y, max_y;                      /* q; 0 when n == 0 */
    int32_t col_min_x, col_max_x, col_min_y, col_max_y;      /* the earliest table column attaining each; -1 when n == 0 */
    int32_t reserved[2];
} EagleTeamShape;                  /* 96 bytes */
typedef struct EagleHullParams {
    int32_t half_width;            /* 1 .. 8 pixels */
    int32_t reserved[3];
} EagleHullParams;
/* The result is kept with the table until eagle_post_free and replaces an earlier one. */
int eagle_post_team_shape(EagleHandle* h, EaglePostTable* t);
int eagle_post_team_shape_values(EaglePostTable* t, EagleTeamShape* shapes /* [rows][2] */, int32_t* hull /* [rows][2][EAGLE_SHAPE_HULL_CAP] */);   /* to the host; either may be NULL */
int eagle_post_device_team_shape(const EaglePostTable* t, const EagleTeamShape** d_shapes, const int32_t** d_hull);      /* in HBM; both NULL before eagle_post_team_shape */
/* The hull layer's parameters are kept with the table (p NULL: forget them). */
int eagle_minimap_set_hulls(EaglePostTable* t, const EagleHullParams* p);
/* Operator entries (host buffers in / out, no handle) for constructed tables, as eagle_op_possession and eagle_op_minimap_trails: shapes and hull may be
 * NULL.  eagle_op_minimap_hulls computes the shape itself and draws any combination of the four layer bits: hp is needed with EAGLE_MM_HULLS, tp with any
 * of the other three (sel, owner, events as in eagle_op_minimap_trails), frames with EAGLE_MM_TRAILS. */
int eagle_op_team_shape(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals,
                        int n_team, EagleTeamShape* shapes, int32_t* hull);
int eagle_op_minimap_hulls(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                           const int32_t* team_vals, int n_team, const EagleMinimapParams* p, const EagleHullParams* hp, const EagleTrailParams* tp, const int32_t* sel,
                           int nsel, const int32_t* owner, const EaglePossessionEvent* events, int n_events, int row0, int n, int out_format,
                           const EagleYuvLayout* out_layout, uint8_t* out);

/* ---- physical report per person: speed zones, efforts (high-speed runs, sprints, accelerations, decelerations) and totals (own specification:
 * tests/physical_ref.py defines every output bit) ----
 * float64 without contraction, sqrt and division correctly rounded.  The inputs are the table's velocities (eagle_post_velocities) and frame numbers f.
 * The PERSONS are the Player and Goalkeeper pitch columns (video == 0) in table order; every other column is ignored.  Per person column c and row r,
 * with v = vel[c][r]:
 *   ROW      pres[r]: vx and vy are finite (the velocity rule makes that "the cell is present").  s[r] = sqrt(vx vx + vy vy), NaN when absent.  link[r] =
 *            r >= 1 && pres[r] && pres[r - 1] && f[r] - f[r - 1] <= max_gap.  a[r] = the speed differenced by the velocity kernel's neighbour rule: row
 *            r - 1 is usable when link[r], row r + 1 when r + 1 < rows && link[r + 1]; both: (s[r + 1] - s[r - 1]) / ((double)(f[r + 1] - f[r - 1]) /
 *            (double) fps); one: the one-sided form; none: 0; absent: NaN.  zone[r] = the number of k in 0 .. 3 with s[r] >= zone_edges[k], 255 when absent.
 *   STEP     at every r with link[r]: df = f[r] - f[r - 1], m = 0.5 (s[r - 1] + s[r]), d = m ((double) df / (double) fps) clamped to at most 2^20,
 *            q[r] = (int64) floor(d 1048576.0 + 0.5), zs[r] = the number of k with m >= zone_edges[k].
 *   TOTALS   zone_frames[z] = the sum of df and zone_dist_q[z] = the sum of q over the steps with zs == z; rows_present; top_speed = the greatest s of a
 *            present row (0.0 with none); efforts[kind] = the number of efforts.  Integers and a maximum: no order of accumulation can show.  Metres are
 *            q / 2^20, seconds frames / fps.
 *   EFFORT   kinds: 0 high-speed run (s >= effort_speed[0]), 1 sprint (s >= effort_speed[1]), 2 acceleration (a >= accel), 3 deceleration (a <=
 *            -accel); hot_k[r] = pres[r] and the kind's condition.  head_k[r] = hot_k[r] && (!link[r] || !hot_k[r - 1]); tail_k[r] = hot_k[r] &&
 *            (r == rows - 1 || !link[r + 1] || !hot_k[r + 1]); start_k[r] = the greatest head row <= r.  An effort exists at every tail row r with
 *            f[r] - f[start_k[r]] >= min_frames[kind < 2 ? 0 : 1]: first_row = start_k[r], last_row = r, frames = f[r] - f[first_row], distance_q = the
 *            sum of q over rows first_row + 1 .. r, peak_speed and peak_accel = the greatest s and |a| of rows first_row .. r (from 0.0, a value counts
 *            when it is greater than the peak so far).  Efforts are reported in ascending (person order, kind, first_row).
 * Three launches (physical.hip) on the handle's main stream read the velocities where eagle_post_velocities left them; the handle's records, staging
 * buffers and graphs are not involved.  The result is kept with the table and answers to its max_bytes budget: the per-row arrays and the call's scratch
 * are checked before any launch, the effort records (48 bytes each) against what is left once their number is known, in front of the third launch.  Edges at 2 / 4 / 5.5 / 7 m/s, efforts from
 * 5.5 and 7 m/s, 2 m/s^2 and half a second are conventional choices, not fitted to data.
 * EAGLE_E_INVALID with a message, before any launch: NULL pointers, fps, max_gap or a min_frames not positive, edges not finite, not positive or not
 * strictly ascending, effort_speed or accel not finite or not positive, a table without velocities, a table of another handle, a column of unknown kind,
 * frames of the operator entry that do not ascend strictly, a result beyond the budget.  rows == 0 or no person column is success with nothing written. */
#define EAGLE_LOAD_HSR 0
#define EAGLE_LOAD_SPRINT 1
#define EAGLE_LOAD_ACCEL 2
#define EAGLE_LOAD_DECEL 3
#define EAGLE_LOAD_ABSENT 255      /* zone of an absent row */
typedef struct EagleLoadParams {
    int32_t fps;                   /* > 0: frames per second of the frame numbers */
    int32_t max_gap;               /* > 0: a step of more frames than this links nothing (a usual choice: fps) */
    int32_t min_frames[2];         /* > 0: the shortest effort in frames, [0] for the speed kinds, [1] for accelerations and decelerations */
    double zone_edges[4];          /* m/s: finite, positive, strictly ascending */
    double effort_speed[2];        /* m/s: finite, positive: high-speed run, sprint */
    double accel;                  /* m/s^2: finite, positive */
    int64_t reserved[2];
} EagleLoadParams;                 /* 88 bytes */
typedef struct EagleLoadTotals {
    int64_t zone_frames[5];        /* frames of the steps whose mean speed lies in the zone */
    int64_t zone_dist_q[5];        /* their distance in 2^-20 m */
    double top_speed;              /* m/s; 0.0 without a present row */
    int32_t col;                   /* the person's table column */
    int32_t rows_present;
    int32_t efforts[4];            /* per EAGLE_LOAD_* kind */
    int32_t reserved[4];
} EagleLoadTotals;                 /* 128 bytes */
typedef struct EagleLoadEffort {
    int32_t col, kind;             /* table column, EAGLE_LOAD_* */
    int32_t first_row, last_row;
    int32_t frames;                /* f[last_row] - f[first_row] */
    int32_t reserved0;
    int64_t distance_q;            /* 2^-20 m */
    double peak_speed, peak_accel; /* m/s, m/s^2 (the magnitude) */
} EagleLoadEffort;                 /* 48 bytes */
/* The result is kept with the table until eagle_post_free and replaces an earlier one; it needs eagle_post_velocities.  A call that fails after its
 * argument checks leaves the table without a result (the earlier one's arrays are rewritten in place). */
int eagle_post_physical(EagleHandle* h, EaglePostTable* t, const EagleLoadParams* p);
/* copies [persons][rows] each to the host; any pointer may be NULL */
int eagle_post_physical_values(EaglePostTable* t, double* speed, double* accel, uint8_t* zone);
/* *n = the number of persons / efforts of the last eagle_post_physical (0 before it); at most cap are written, in the order above. */
int eagle_post_physical_totals(const EaglePostTable* t, EagleLoadTotals* out, int cap, int* n);
int eagle_post_physical_efforts(const EaglePostTable* t, EagleLoadEffort* out, int cap, int* n);
int eagle_post_device_physical(const EaglePostTable* t, const double** d_speed, const uint8_t** d_zone);     /* [persons][rows] in HBM; NULL before eagle_post_physical */
/* Operator entry (host buffers in / out, no handle) for constructed tables: velocities [cols][rows][2], frames [rows] strictly ascending, columns as
 * eagle_post_layout gives them.  speed, accel, zone ([persons][rows] each) may be NULL; at most totals_cap totals and efforts_cap efforts are written,
 * *n_persons and *n_efforts are what there is. */
int eagle_op_physical(int device, const double* velocities, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const EagleLoadParams* p,
                      double* speed, double* accel, uint8_t* zone, EagleLoadTotals* totals, int totals_cap, int* n_persons, EagleLoadEffort* efforts,
                      int efforts_cap, int* n_efforts);

/* ---- track smoothing: windowed least-squares fits of the pitch positions (own specification: tests/smooth_ref.py defines every output bit) ------------
 * Opt-in; a table never smoothed is byte for byte what eagle_postprocess built.  Integers wherever a sum is formed, float64 with single operations in
 * the order written everywhere else (no contraction).
 * COLUMNS.  The Player and Goalkeeper pitch columns (video == 0) are smoothed with half-width W = window; the Ball pitch column with W = ball_window
 * when that is > 0.  Every other column (video columns, boundaries, the ball by default) keeps its bytes, gets post_velocity_kernel's velocity for
 * (fps, max_gap, speed_cap) bit for bit, acceleration (NaN, NaN), and 0 in flags, count and residual_q.
 * PRESENCE.  A cell of a smoothed column is present when x and y are finite and |x|, |y| <= 1024 (the minimap's rule); q = rint(x * 1024) as int64, ties
 * to even, once.  An absent cell is absent in every output: NaN value, velocity and acceleration, 0 in flags, count and residual_q.
 * WINDOW of row r: the used rows r' of the column with |f[r'] - f[r]| <= W (frames ascend strictly: within W rows), t = f[r'] - f[r].
 * SUMS, exact int64: S_k = sum t^k (k = 0 .. 4); per axis B_k = sum t^k q (k = 0 .. 2).  n = S_0.
 * DEGREE used: n >= 4: degree; n == 3: min(degree, 1); n == 2: 1; n == 1: 0; n == 0 (the refit only): the cell keeps its raw value, velocity and
 * acceleration (0, 0), flags bit 4, count 0, residual_q 0.
 * SOLVE, Cramer's rule on the sums converted to double.  Degree 2: C00 = S2 S4 - S3 S3, C01 = S2 S3 - S1 S4, C02 = S1 S3 - S2 S2, C11 = S0 S4 - S2 S2,
 * C12 = S1 S2 - S0 S3, C22 = S0 S2 - S1 S1, det = (S0 C00 + S1 C01) + S2 C02, a_i = ((C0i B0 + C1i B1) + C2i B2) / det (C10 = C01, C20 = C02, C21 = C12).
 * Degree 1: det = S0 S2 - S1 S1, a0 = (S2 B0 - S1 B1) / det, a1 = (S0 B1 - S1 B0) / det, a2 = 0.  Degree 0: a0 = B0 / S0, a1 = a2 = 0.
 * PASS 1: used = present; e[r] = max(|q_x - a0_x|, |q_y - a0_y|).
 * PASS 2: med[r] = the element of rank (n - 1) // 2 of the window's e ordered by (value, row); the sample is an outlier when outlier_k > 0 and
 * e[r] > max(outlier_floor * 1024, outlier_k * med[r]).
 * PASS 3: used = present and not an outlier (a cell's own sample included).  Position a0 / 1024; velocity (a1 * fps) / 1024, a speed above speed_cap scaled
 * back as post_velocity_kernel does; acceleration (((2 a2) * fps) * fps) / 1024.
 * PER CELL: flags bit 0 fitted, bit 1 outlier, bits 2-3 the degree used, bit 4 kept raw; count = the refit's n; residual_q = rint(min(16 e', 2^24)) with
 * e' the raw sample's residual against the final fit.  PER COLUMN: EagleSmoothTotals (all zero for a column not smoothed).  PER ROW: suspect = 1 when at
 * least 4 smoothed person cells (Player, Goalkeeper) are present and at least half of them are outliers: the frame's homography probably jumped.
 * Four launches (csrc/smooth.hip): fit, flag, refit, totals.
 * EAGLE_E_INVALID with a message, before any launch and leaving every output and the table alone: NULL pointers, fps, max_gap or speed_cap not positive
 * (speed_cap not finite), window outside 1 .. 64, degree outside {1, 2}, outlier_k negative or not finite, outlier_floor negative or not finite,
 * ball_window outside 0 .. 64, a column of unknown kind, frames of the operator entry that do not ascend; through a handle also a table that already
 * carries a result derived from its positions (velocities, possession, occupancy, shape, physical, roles, space, offside, control parameters) and a
 * second call.
 * The constants (0.4 s, degree 2, k = 4, 0.25 m) are conventional choices, not fitted to data; gap-filled cells count as samples; a homography jump is
 * detected and trimmed per person; correcting it as a common motion is eagle_post_stabilise's part (below), which runs before this stage; one trimming
 * round. */
typedef struct EagleSmoothParams {
    int32_t fps;                   /* > 0 */
    int32_t window;                /* 1 .. 64: half-width W in frames (a usual choice: max(2, round(0.4 fps))) */
    int32_t degree;                /* 1 or 2 */
    int32_t ball_window;           /* 0 .. 64: the ball's half-width; 0 leaves the ball alone */
    int32_t max_gap;               /* > 0: the velocity rule of the columns not smoothed, as EagleKinematicsParams */
    int32_t reserved0;
    double outlier_k;              /* 0: no trimming, else finite and positive: multiple of the window's median residual */
    double outlier_floor;          /* metres, finite, >= 0: no sample closer to its fit than this is rejected */
    double speed_cap;              /* > 0, finite: m/s */
    int64_t reserved;
} EagleSmoothParams;               /* 56 bytes */
typedef struct EagleSmoothTotals {
    int64_t sum_sq;                /* sum of residual_q^2 over the column's cells */
    int32_t present, outliers;
    int32_t low_degree;            /* present cells fitted with a degree below `degree` (kept-raw cells included) */
    int32_t max_residual_q;
    int32_t window;                /* the half-width the column was smoothed with; 0: not smoothed */
    int32_t reserved;
} EagleSmoothTotals;               /* 32 bytes */
/* Replaces the smoothed columns of the table in HBM, sets the table's velocities (as eagle_post_velocities with fps, max_gap, speed_cap; a later
 * eagle_post_velocities replaces them) and keeps acceleration, flags, count, residual_q, suspect and totals with the table until eagle_post_free.
 * It comes before every result derived from the table and once. */
int eagle_post_smooth_tracks(EagleHandle* h, EaglePostTable* t, const EagleSmoothParams* p);
/* copies to the host; any pointer may be NULL: acc [cols][rows][2], flags, count, residual_q [cols][rows], suspect [rows], totals [cols] */
int eagle_post_smooth_values(EaglePostTable* t, double* acc, uint8_t* flags, uint8_t* count, int32_t* residual_q, uint8_t* suspect, EagleSmoothTotals* totals);
int eagle_post_device_smooth(const EaglePostTable* t, const double** d_acc, const uint8_t** d_flags, const uint8_t** d_suspect);  /* NULL before the call */
int eagle_post_raw_values(EaglePostTable* t, double* values /* [cols][rows][2] */);   /* the positions from before eagle_post_smooth_tracks (the table's, without one) */
/* Operator entry (host buffers in / out, no handle): values [cols][rows][2], frames [rows] strictly ascending; every output may be NULL. */
int eagle_op_smooth_tracks(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const EagleSmoothParams* p,
                           double* out_values, double* out_vel, double* out_acc, uint8_t* flags, uint8_t* count, int32_t* residual_q, uint8_t* suspect,
                           EagleSmoothTotals* totals);

/* ---- stabilisation: each frame's common motion is estimated and removed (own specification: tests/stab_ref.py defines every output bit) ----------------
 * Opt-in; directly after eagle_postprocess, before eagle_post_smooth_tracks and every derived result.  A homography that is a little off moves every
 * player and the ball of that frame together by a small translation, stretch and shear of the pitch plane; the persons' own paths over a window of
 * frames predict where each of them should be, and the common part of what they miss is an affine map that is estimated robustly and subtracted.
 * Integers wherever a sum is formed, float64 with single operations in the order written everywhere else (no contraction).
 * COLUMNS.  Voters: the Player and Goalkeeper pitch columns (video == 0).  Moved: the voters and the Ball pitch column.  Every other column (video
 * columns, boundaries) keeps its bytes.
 * PRESENCE of a cell of a moved column and q = rint(x * 1024): eagle_post_smooth_tracks' rule.  C, the corrected integers, start as q.
 * ROUNDS.  `iterations` rounds; each is computed from C of the round before for the neighbours and from q for the row itself; a row's map is estimated
 * afresh each round, never composed.
 * PREDICT, per present voter cell (c, r): the window is the present rows r' != r of the column with |f[r'] - f[r]| <= window; the cell can vote when
 * the window has a row before r, a row after r and n >= 2 rows.  eagle_post_smooth_tracks' SUMS over C[r'] with t = f[r'] - f[r], its DEGREE rule
 * (n >= 4: degree; else 1) and its SOLVE give a0 per axis.  The cell votes when |a0| <= 2^40 on both axes and, with p = llrint(a0) (ties to even),
 * d = q - p has |d| <= 2^24 on both axes (a vote fits its int32 and every sum below its int64).
 * ESTIMATE, per row.  The voters in column order, at most the first 64 (more: flag bit 0).  Fewer than min_voters: no estimate (model 0), the row keeps
 * its bytes.  b = per-axis lower median of d (the element of rank (n - 1) / 2); dev_i = max(|d_x - b_x|, |d_y - b_y|); m = lower median of dev; a voter
 * is an inlier when trim_k == 0 or (double)dev_i <= max(floor * 1024, trim_k * (double)m).  Over the n_in inliers, floor division throughout:
 * translation s = floor((2 sum d + n_in) / (2 n_in)) per axis; centre c = floor(sum q / n_in) per axis; u = q_x - c_x, v = q_y - c_y; exact int64 sums
 * n, Su, Sv, Suu, Suv, Svv and per axis D0 = sum d, Du = sum u d, Dv = sum v d; Cuu = n Suu - Su Su, Cvv = n Svv - Sv Sv, Cuv = n Suv - Su Sv.
 * With model 1 the affine map is used when n_in >= 6 (else flag bit 1), (double)Cuu and (double)Cvv >= (double)(n n) * (smin * smin) with
 * smin = min_spread * 1024 (else bit 2), and (double)Cuv * (double)Cuv <= 0.75 * ((double)Cuu * (double)Cvv) (else bit 3), tested in this order.
 * Its solve on the sums converted to double: C00 = Suu Svv - Suv Suv, C01 = Suv Sv - Su Svv, C02 = Su Suv - Suu Sv, C11 = n Svv - Sv Sv,
 * C12 = Su Sv - n Suv, C22 = n Suu - Su Su, det = (n C00 + Su C01) + Sv C02, coefficient j = ((C0j D0 + C1j Du) + C2j Dv) / det, giving
 * (b0, g_u, g_v) per axis.  A gain above max_gain in magnitude (or |b0| > 2^40) falls back to the translation too (bit 4).
 * T(q) per axis = llrint((b0 + g_u u) + g_v v); for the translation T(q) = s and offset = (double)s.  shift_q = T(c); bit 5 (jump) when |shift_q|
 * exceeds jump * 1024 on either axis: reported only.
 * APPLY.  Every present cell of a moved column in a row with an estimate: C = q - T(q); in a row without: C = q.  After the last round the table's
 * value of such a cell is (double)C / 1024.0; rows without an estimate, absent cells and all other columns keep their input bytes.
 * Launches (csrc/stab.hip): quantise; per round predict, estimate, apply; totals.
 * EAGLE_E_INVALID with a message, before any launch and leaving every output and the table alone: NULL pointers, fps <= 0, window outside 1 .. 64,
 * degree outside {1, 2}, model outside {0, 1}, min_voters outside 3 .. 64, iterations outside 1 .. 4, trim_k neither 0
 * nor in 1 .. 1000, floor outside 0 .. 1024, min_spread outside (0, 1024], max_gain outside (0, 1], jump not positive, anything not finite, a column of
 * unknown kind, frames of the operator entry that do not ascend; through a handle also another handle's table, a second call, and a table that already
 * carries a result derived from its positions, eagle_post_smooth_tracks' included: stabilising comes first.
 * LIMITS.  What differs from the window's trend is removed: an error that lasts (a homography wrong for a second, the drift between two key-point
 * frames) is a path like any other and stays.  Gap-filled cells cannot be told from seen ones: they lie on a line, vote for "no motion" and bias a
 * row in which many cells are filled.  A real common jerk (the whole team stopping in one frame) is taken for camera error.  The affine map is a
 * first-order stand-in for a projective error, valid where the players stand: boundaries are not moved.  The ball is moved although it may be in the
 * air.  At most 64 voters per row.  The constants are conventional choices, not fitted to data; nothing was validated on real footage. */
typedef struct EagleStabParams {
    int32_t fps;                   /* > 0 */
    int32_t window;                /* 1 .. 64: half-width W in frames (a usual choice: min(64, max(2, round(1.0 fps)))) */
    int32_t degree;                /* 1 or 2 */
    int32_t model;                 /* 0 translation, 1 affine (with the translation as its fall-back) */
    int32_t min_voters;            /* 3 .. 64 */
    int32_t iterations;            /* 1 .. 4 */
    int32_t reserved0[2];
    double trim_k;                 /* 0: no trimming, else 1 .. 1000: multiple of the median deviation */
    double floor;                  /* metres, 0 .. 1024: no voter closer to the median than this is trimmed */
    double min_spread;             /* metres, (0, 1024]: the least standard deviation of the inliers along x and y for the affine map */
    double max_gain;               /* (0, 1]: the largest |gain| of the affine map */
    double jump;                   /* metres, > 0: |shift| above it sets the jump flag */
    int64_t reserved;
} EagleStabParams;                 /* 80 bytes */
#define EAGLE_STAB_OVER_CAP 1      /* EagleStabRow.flags: more than 64 voters, the first 64 were used */
#define EAGLE_STAB_FEW 2           /*   fall-back to the translation: fewer than 6 inliers */
#define EAGLE_STAB_SPREAD 4        /*   ... the inliers' spread is below min_spread */
#define EAGLE_STAB_CORR 8          /*   ... the inliers lie too close to a line */
#define EAGLE_STAB_GAIN 16         /*   ... a gain above max_gain */
#define EAGLE_STAB_JUMP 32         /*   |shift_q| above jump */
typedef struct EagleStabRow {
    int32_t voters, inliers;
    int32_t model;                 /* 0 none (the row kept its bytes), 1 translation, 2 affine */
    int32_t flags;
    int32_t shift_q[2];            /* T(centre), 1/1024 m */
    int32_t centre_q[2];
    double offset[2];              /* b0 per axis (the translation as a double for model 1) */
    double gain[4];                /* x by u, x by v, y by u, y by v */
    int64_t ss_before;             /* sum over the inliers of |d|^2 */
    int64_t ss_after;              /* sum over the inliers of |d - T(q)|^2 */
    int32_t moved;                 /* cells of the row that were moved */
    int32_t reserved;
} EagleStabRow;                    /* 104 bytes */
typedef struct EagleStabTotals {
    int64_t ss_before, ss_after;   /* summed over the rows (modulo 2^64) */
    int64_t inliers, moved;
    int32_t rows;
    int32_t none, translation, affine;                          /* rows per model */
    int32_t few_inliers, low_spread, correlated, high_gain;     /* fall-backs by cause */
    int32_t jumps, over_cap;
    int32_t iterations, window;
} EagleStabTotals;                 /* 80 bytes */
/* Replaces the moved cells of the table in HBM and keeps the row records, the last round's votes, the totals and the positions from before with the
 * table until eagle_post_free.  Called once and before everything else; eagle_post_smooth_tracks accepts a stabilised table, and
 * eagle_post_raw_values then gives the stabilised positions. */
int eagle_post_stabilise(EagleHandle* h, EaglePostTable* t, const EagleStabParams* p);
/* copies to the host; any pointer may be NULL: rows [rows], totals, votes [cols][rows][2] ((0, 0) where a cell did not vote); EAGLE_E_INVALID before the stage ran */
int eagle_post_stabilise_values(EaglePostTable* t, EagleStabRow* rows, EagleStabTotals* totals, int32_t* votes);
int eagle_post_original_values(EaglePostTable* t, double* values /* [cols][rows][2] */);   /* the positions from before eagle_post_stabilise (the table's own, without one) */
int eagle_post_device_stabilise(const EaglePostTable* t, const EagleStabRow** d_rows);     /* the row records in HBM; NULL before the call */
/* Operator entry (host buffers in / out, no handle): values [cols][rows][2], frames [rows] strictly ascending; every output may be NULL. */
int eagle_op_stabilise(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const EagleStabParams* p,
                       double* out_values, EagleStabRow* rows_out, int32_t* votes, EagleStabTotals* totals);

/* ---- pass options: where the ball owner can play, per row (own specification: tests/options_ref.py defines every output bit) ----------------------------
 * float32 without contraction, correctly rounded sqrtf and division, the library's own expf (csrc/dmath.h).  Cell centres, the reaction point
 * q = p + v t_react with its clamp to +-2^20, the fp32 rounding of positions and velocities and the non-finite-velocity rule are the control grid's.
 * SITE COLUMNS  the Player pitch columns (video == 0) whose FIRST mapping entry with the column's id is >= 0 (a negative entry is "unknown": no site;
 *               goalkeepers are never sites); their group is 0 for team value 0, else 1.  n_sites counts them, in table order (eagle_pass_options_layout).
 *               A column's site of a row: its cell when it is present with |x|, |y| <= 1024.  The ball is the one Ball pitch column.
 * ROW STATUS    the first that applies: EAGLE_PASS_NO_OWNER owner[r] < 0; _IN_FLIGHT cand[r] != owner[r] (the owner of record is not at the ball);
 *               _NO_TEAM the owner's column is not a site column; _OFF_DOMAIN the ball cell is not within |x|, |y| <= 1024 (absent, or no ball column);
 *               _ACTIVE otherwise.  A row that is not active has a grid of zeros, options all -1, best_col = best_byte = -1 and zero counts.
 * ACTIVE ROW    b = the ball cell in fp32; attackers = the sites of the owner's group except the owner's own column, defenders = the sites of the other
 *               group.  For a target c: dx = cx - bx, dy = cy - by, L = sqrtf(dx dx + dy dy); for k = 1 .. K (K = samples) f_k = (float)k / (float)K, the
 *               sample s_k = (bx + dx f_k, by + dy f_k), the ball time T_k = (L f_k) / v_ball; t_D(s) = t_react + sqrtf(min over defenders of ex ex + ey ey)
 *               / v_max with ex = sx - qx, ey = sy - qy, t_A(s) the same over attackers, every min from FLT_MAX.  Lane safety: m = min over k < K of
 *               t_D(s_k) - T_k, safety = 1 / (1 + expf(-(beta m))), 1 when K == 1.  Reception at s_K as computed: reach = 1 / (1 + expf(-(beta (t_D(s_K) -
 *               t_A(s_K))))).  Without defenders safety = reach = 1.  byte = (int)floorf(safety reach 255 + 0.5); 0 without attackers.
 * OUTPUTS       grid u8 [gh][gw] (gw = 105 R, gh = 68 R, grid row 0 at pitch y = 0): the byte at every cell centre.  options int16 [n_sites]: for a present
 *               attacker the byte at its own reaction point q_i, everything else -1.  The row record: best_col / best_byte = the largest option (a tie:
 *               the earlier column), sum = the exact sum of the row's grid bytes (0 when no grid was asked for), group = the owner's group when its
 *               column is a site column (whatever the status), else -1.
 * Four launches (options.hip) on the handle's main stream: sites, grid (only with a grid), options, best.  The constants (16 samples, 0.7 s, 5 m/s, 4 / s,
 * a 15 m/s ball) are conventional choices, not fitted to data.
 * EAGLE_E_INVALID with a message, before any launch: NULL pointers, cells_per_metre outside {1, 2, 4}, samples outside 1 .. 64, t_react, v_max, beta
 * outside control's ranges, v_ball outside 0.001 .. 1e6, a table without a team mapping, without velocities, without a possession result (handle
 * entries), the table of another handle, a row window outside the table, more than EAGLE_PASS_MAX_SITES site columns, more than one Ball pitch column,
 * a column of unknown kind, cand / owner entries that are neither -1 nor a column index (operator entry), a device-memory need beyond the table's
 * budget.  n == 0 is success and writes nothing. */
#define EAGLE_PASS_ACTIVE 0
#define EAGLE_PASS_NO_OWNER 1
#define EAGLE_PASS_IN_FLIGHT 2
#define EAGLE_PASS_NO_TEAM 3
#define EAGLE_PASS_OFF_DOMAIN 4
#define EAGLE_PASS_MAX_SITES 1024  /* a row's two lists then fit in LDS together (8 bytes per entry) */
typedef struct EaglePassOptionParams {
    int32_t cells_per_metre;       /* 1, 2 or 4 */
    int32_t samples;               /* K: 1 .. 64 lane samples (a usual choice: 16) */
    float t_react, v_max, beta;    /* seconds, m/s, 1/s: control's ranges */
    float v_ball;                  /* m/s: 0.001 .. 1e6 (a usual choice: 15) */
    int32_t reserved[2];
} EaglePassOptionParams;           /* 32 bytes */
typedef struct EaglePassOptionRow {
    int32_t status;                /* EAGLE_PASS_* */
    int32_t owner_col;             /* owner[r] */
    int32_t group;                 /* the owner's group, -1 when its column is not a site column */
    int32_t n_mates, n_defenders;  /* attackers and defenders present on the row (0 unless active) */
    int32_t best_col, best_byte;   /* the largest option and its table column; -1 without an option */
    int32_t reserved;
    int64_t sum;                   /* the sum of the row's grid bytes */
} EaglePassOptionRow;              /* 40 bytes */
int eagle_pass_options_size(const EaglePassOptionParams* p, int* gw, int* gh);                               /* = eagle_control_size's */
/* *n_sites = the number of site columns of the table; at most cap of their table columns are written, in table order. */
int eagle_pass_options_layout(const EaglePostTable* t, int32_t* site_cols, int cap, int* n_sites);
/* rows row0 .. row0 + n - 1 of a table with velocities and possession -> grids [n][gh][gw], records [n], options [n][n_sites] in HBM; d_grid may be
 * NULL (the grid kernel is then not launched, sum = 0) and d_options too; returns when they are complete */
int eagle_pass_options_device(EagleHandle* h, EaglePostTable* t, int row0, int n, const EaglePassOptionParams* p, uint8_t* d_grid, EaglePassOptionRow* d_rows,
                              int16_t* d_options);
/* Same, to host memory, in passes of what 32 MB of device staging hold. */
int eagle_pass_options(EagleHandle* h, EaglePostTable* t, int row0, int n, const EaglePassOptionParams* p, uint8_t* grid, EaglePassOptionRow* rows_out, int16_t* options);
/* Operator entry (host buffers in / out, no handle) for constructed tables; cand and owner [rows] as eagle_op_possession gives them; options
 * [n][n_sites] with n_sites as the columns and the mapping give it; grid and options may be NULL. */
int eagle_op_pass_options(int device, const double* values, const double* velocities, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                          const int32_t* team_vals, int n_team, const int32_t* cand, const int32_t* owner, const EaglePassOptionParams* p, int row0, int n,
                          uint8_t* grid, EaglePassOptionRow* rows_out, int16_t* options);

/* ---- player roles: per row the exact least-cost assignment of a team's present players to R role positions, re-estimated from the assignment (own
 * specification: tests/roles_ref.py defines every output bit) ----
 * MEMBERS, GROUPS, PRESENT and the quantisation q are the team shape's (above).  A role is not a tracker id: a fragment that ends and the one that
 * replaces it land in the same role, and two players who exchange places leave the roles where they are.
 *   ROW      n = present members; status EMPTY (n == 0), TOO_FEW (n < min_present), TOO_MANY (n > roles), else ACTIVE.  Centre cx = floor((2 sum qx + n) /
 *            (2 n)) (0 when n == 0), cy likewise; a present member's centred position is u = q - c, |u| <= 2^21.  The players of a row are its present
 *            members in table-column order.
 *   SEEDS    per member column cnt = the ACTIVE rows on which it is present and S = the sums of u over them; the columns of a group ranked by (cnt
 *            descending, column ascending), the first `roles` with cnt > 0 seed roles 0, 1, ... at floor((2 S + cnt) / (2 cnt)) per axis.  Fewer such
 *            columns: the group's model status is NO_SEEDS, its rows report role -1 and cost 0, the group has no means, counts or sums.
 *   ROUND    for every ACTIVE row of a seeded group c[i][j] = |u_i - M_j|^2 (int64; a row's total < 2^49); sigma = the injective map players -> roles of
 *            least total cost and, among those, the lexicographically smallest sequence (sigma(0), sigma(1), ...).  Then M_j = floor((2 S_j + cnt_j) /
 *            (2 cnt_j)) over the (row, player) pairs given role j; a role nobody played keeps its position.  changed[k] = the (row, group) pairs whose
 *            sigma differs from round k-1's, over both groups (round 0: all of them).
 *   RESULT   after `iterations` rounds: the assignment of the last round, its costs, and the positions it was computed AGAINST (mean); count, sum, sum2:
 *            cnt_j and the sums of u and u^2 per axis over that assignment.  Entries at and beyond `roles` are 0.  Once changed[k] == 0 no later round
 *            changes anything; the launches stop there and the entries of changed behind k are 0.
 * The defaults (10 roles, 8 present, 8 rounds) are conventional choices, not fitted to data.
 * Launches (roles.hip) on the handle's main stream read the table where eagle_postprocess left it; what the call allocates is held against the table's
 * max_bytes before the first launch.  The handle's records, staging buffers and graphs are not involved.
 * EAGLE_E_INVALID with a message, before any launch and leaving every output alone: NULL table or parameters, a table without a mapping, parameters
 * outside their ranges or non-zero reserved words, more than EAGLE_SHAPE_MAX_MEMBERS members, a column of unknown kind.  A refused call leaves an
 * earlier result of the table in place.  rows == 0 is success and writes nothing. */
#define EAGLE_ROLE_CAP 10
#define EAGLE_ROLE_EMPTY 0         /* EagleRoleRow::status */
#define EAGLE_ROLE_TOO_FEW 1
#define EAGLE_ROLE_ACTIVE 2
#define EAGLE_ROLE_TOO_MANY 3
#define EAGLE_ROLE_MODEL_OK 0      /* EagleRoleGroup::status */
#define EAGLE_ROLE_NO_SEEDS 1
typedef struct EagleRoleParams {
    int32_t roles;                 /* R: 2 .. EAGLE_ROLE_CAP (10) */
    int32_t min_present;           /* 2 .. roles (8) */
    int32_t iterations;            /* T: 1 .. 32 (8) */
    int32_t reserved[5];           /* 0 */
} EagleRoleParams;                 /* 32 bytes */
typedef struct EagleRoleRow {
    int64_t cost;                  /* the assignment's total cost, q^2; 0 unless ACTIVE in a seeded group */
    int32_t n;                     /* present members */
    int32_t status;                /* EAGLE_ROLE_EMPTY .. EAGLE_ROLE_TOO_MANY */
    int32_t cx, cy;                /* the centre, q */
    int32_t col[EAGLE_ROLE_CAP];   /* the table column playing role j, or -1 */
} EagleRoleRow;                    /* 64 bytes */
typedef struct EagleRoleGroup {
    int64_t sum[EAGLE_ROLE_CAP][2];        /* of u per role and axis over the final assignment */
    int64_t sum2[EAGLE_ROLE_CAP][2];       /* ... of u^2 */
    int32_t mean[EAGLE_ROLE_CAP][2];       /* the role positions the final assignment was computed against, q round the row's centre */
    int32_t count[EAGLE_ROLE_CAP];         /* (row, player) pairs per role */
    int32_t status;                        /* EAGLE_ROLE_MODEL_OK / EAGLE_ROLE_NO_SEEDS */
    int32_t active_rows;
} EagleRoleGroup;                  /* 448 bytes */
typedef struct EagleRoleModel {
    EagleRoleGroup group[2];
    int32_t changed[32];
} EagleRoleModel;                  /* 1024 bytes */
/* The result is kept with the table until eagle_post_free and replaces an earlier one. */
int eagle_post_roles(EagleHandle* h, EaglePostTable* t, const EagleRoleParams* p);
/* To the host; any pointer may be NULL.  member_roles: int8 [members][rows], members in group order (group 0's columns, then group 1's): the member's role
 * on the row, or -1 (absent, the row not ACTIVE, the group without seeds). */
int eagle_post_roles_values(EaglePostTable* t, EagleRoleRow* rows_out /* [rows][2] */, int8_t* member_roles, EagleRoleModel* model);
/* In HBM; all NULL (and 0 members) before eagle_post_roles.  n_members may be NULL. */
int eagle_post_device_roles(const EaglePostTable* t, const EagleRoleRow** d_rows, const int8_t** d_member_roles, const EagleRoleModel** d_model, int* n_members);
/* Operator entry (host buffers in / out, no handle) for constructed tables, as eagle_op_team_shape; each output may be NULL. */
int eagle_op_roles(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals, int n_team,
                   const EagleRoleParams* p, EagleRoleRow* rows_out, int8_t* member_roles, EagleRoleModel* model);

/* ---- space per player: the exact dominant region of every present member on the pitch grid, the nearest opponent and the opponents within a radius
 * (own specification: tests/space_ref.py defines every output bit) ----
 * GROUPS, MEMBERS, PRESENT and the quantisation q are the team shape's (above): groups 0 and 1 hold the Player pitch columns with a mapping entry (the
 * first entry for an id counts), a member is present when x and y are finite and |x|, |y| <= 1024 m, q = floor(v * 1024 + 0.5); a mapping is required.
 *   GOALKEEPERS  goalkeepers != 0 (the default): the Goalkeeper pitch columns, mapped or not, are the members of group 2, "neither team".  They own
 *            cells; they are nobody's opponent and have no opponent.  goalkeepers == 0: they are no members, as in shape and roles.
 *   SITES    of a row: its present members in table-column order, S of them.  status EMPTY (S == 0), TOO_MANY (S > EAGLE_SPACE_SITE_CAP), else ACTIVE.
 *            The row record always holds status, n_sites = S and n[g], the present members per group.  A row that is not ACTIVE has no site
 *            records, no cells and an owner map of 255.  Unused site slots: col = near_col = -1, near_d2 = -1, zeros.
 *   GRID     cells_per_metre R in {1, 2, 4}, gw = 105 R, gh = 68 R, grid row 0 is pitch y = 0 (eagle_control_size's geometry).  The centre of cell (i, j)
 *            in q is X = (2 i + 1) (512 / R), Y = (2 j + 1) (512 / R), integers for all three R.  d2 = (X - qx)^2 + (Y - qy)^2 in int64: |X - qx| <
 *            2^21, so d2 < 2^43.  The cell's owner is the site of least d2, of equal d2 the earlier table column: coincident sites leave everything
 *            to the earlier one; a site off the pitch is a site like any other.
 *   THIRDS   cell (i, j) lies in third 0 when i < 35 R, in third 1 when i < 70 R, else in third 2.  A site's cells[t]: the cells it owns in third t; the
 *            row's cells[g][t]: their sum over the sites of group g.  On an ACTIVE row all cells add up to gw gh exactly.
 *   MARKING  of a site of group 0 or 1 over the row's sites of the other of those two groups: near_d2 = the least squared distance in q^2 (int64, <=
 *            2^43), near_col = that site's column, the earlier column on a tie; -1, -1 without such a site.  within = the number of those sites with
 *            d2 <= rq^2, inclusive, rq = floor(radius * 1024 + 0.5); radius is finite, > 0 and <= 1024.  A site of group 2 reports -1, -1, 0.
 *   TOTALS   per member, in group order 0, 1, 2 and by column inside a group, over the ACTIVE rows on which it is present: rows, the sums of cells[3],
 *            min and max of its cell total (0 when rows == 0), the rows with an opponent (near_col >= 0), the rows with within > 0, the sum of
 *            within.  Rows are counted, not weighted by the frame step to the next row.
 *   OWNER MAP  of a row window (row0, n): u8 [n][gh][gw], the owner's index into the row's site list; 255 on a row that is not ACTIVE.
 * The default radius of 3 m is a conventional choice, not fitted to data.  The nearest-site rule ignores velocity (that is the control surface's job).
 * Launches (space.hip) on the handle's main stream read the table where eagle_postprocess left it; what the call allocates is held against the table's
 * max_bytes before the first launch.  The handle's records, staging buffers and graphs are not involved.
 * EAGLE_E_INVALID with a message, before any launch and leaving every output alone: NULL table or parameters, a table without a mapping, cells_per_metre
 * outside {1, 2, 4}, a radius that is not finite or outside (0, 1024], non-zero reserved words, more than EAGLE_SHAPE_MAX_MEMBERS members over the
 * three groups, a column of unknown kind, a row window outside the table, a device-memory need beyond the budget.  A refused call leaves an earlier
 * result of the table in place.  rows == 0 (n == 0 for a window) is success and writes nothing. */
#define EAGLE_SPACE_SITE_CAP 32
#define EAGLE_SPACE_EMPTY 0        /* EagleSpaceRow::status */
#define EAGLE_SPACE_ACTIVE 1
#define EAGLE_SPACE_TOO_MANY 2
#define EAGLE_SPACE_NO_OWNER 255   /* the owner map of a row that is not ACTIVE */
typedef struct EagleSpaceParams {
    int32_t cells_per_metre;       /* 1, 2 or 4 */
    int32_t goalkeepers;           /* != 0: the goalkeepers are group 2 (1) */
    double radius;                 /* metres: finite, > 0, <= 1024 (3) */
    int32_t reserved[4];           /* 0 */
} EagleSpaceParams;                /* 32 bytes */
typedef struct EagleSpaceRow {
    int32_t status;                /* EAGLE_SPACE_EMPTY .. EAGLE_SPACE_TOO_MANY */
    int32_t n_sites;               /* S, also beyond the cap */
    int32_t n[3];                  /* present members per group */
    int32_t cells[3][3];           /* [group][third]; 0 unless ACTIVE */
    int32_t reserved[2];           /* 0 */
} EagleSpaceRow;                   /* 64 bytes */
typedef struct EagleSpaceSite {
    int64_t near_d2;               /* the nearest opponent's squared distance, q^2; -1 without one */
    int32_t col;                   /* the site's table column; -1: an unused slot */
    int32_t group;                 /* 0, 1 or 2 */
    int32_t near_col;              /* the nearest opponent's table column, or -1 */
    int32_t within;                /* opponents with d2 <= rq^2 */
    int32_t cells[3];              /* the cells it owns, per third */
    int32_t qx, qy;                /* its position, q */
    int32_t reserved;              /* 0 */
} EagleSpaceSite;                  /* 48 bytes */
typedef struct EagleSpaceTotals {
    int64_t cells[3];              /* the sums of the member's cells per third */
    int64_t within_sum;
    int32_t col, group;            /* the member's table column and group */
    int32_t rows;                  /* ACTIVE rows on which it is present */
    int32_t min, max;              /* of its cell total over those rows; 0 when rows == 0 */
    int32_t opp_rows;              /* ... with near_col >= 0 */
    int32_t within_rows;           /* ... with within > 0 */
    int32_t reserved;              /* 0 */
} EagleSpaceTotals;                /* 64 bytes */
/* The result is kept with the table until eagle_post_free and replaces an earlier one.  The members depend on the parameters, so a call computes into a
 * buffer of its own and frees the earlier result only when the new one is complete: a refused call and a call that fails later both leave the earlier
 * result in place.  What is held against max_bytes is what the call allocates (the new result and its member lists); until the swap the earlier result
 * stands beside it, so for the length of a call the table may hold up to one earlier result more than the budget names. */
int eagle_post_space(EagleHandle* h, EaglePostTable* t, const EagleSpaceParams* p);
/* To the host: rows_out [rows], sites_out [rows][EAGLE_SPACE_SITE_CAP], totals_out [members]; any pointer may be NULL. */
int eagle_post_space_values(EaglePostTable* t, EagleSpaceRow* rows_out, EagleSpaceSite* sites_out, EagleSpaceTotals* totals_out);
/* In HBM; all NULL (and 0 members) before eagle_post_space.  n_members may be NULL. */
int eagle_post_device_space(const EaglePostTable* t, const EagleSpaceRow** d_rows, const EagleSpaceSite** d_sites, const EagleSpaceTotals** d_totals, int* n_members);
/* The owner maps of rows row0 .. row0 + n - 1 -> u8 [n][gh][gw] in HBM; returns when they are complete.  The call computes the sites of the window itself:
 * it neither needs nor touches the table's kept result. */
int eagle_space_device_grids(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleSpaceParams* p, uint8_t* d_grid);
/* Same, to host memory, in passes of what 32 MB of device staging hold. */
int eagle_space_grids(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleSpaceParams* p, uint8_t* grid);
/* Operator entry (host buffers in / out, no handle) for constructed tables, as eagle_op_team_shape: rows_out, sites_out and totals_out cover the whole
 * table, grid the window (row0, n); each output may be NULL. */
int eagle_op_space(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals, int n_team,
                   const EagleSpaceParams* p, int row0, int n, EagleSpaceRow* rows_out, EagleSpaceSite* sites_out, EagleSpaceTotals* totals_out, uint8_t* grid);

/* ---- offside: per row and attacking team the offside line and every attacker's margin beyond it, per pass event a verdict about the receiver (own
 * specification: tests/offside_ref.py defines every output bit) ----
 * GROUPS, MEMBERS, PRESENT and the quantisation q are the team shape's (above): groups 0 and 1 hold the Player pitch columns with a non-negative mapping
 * entry (the first entry for an id counts), a member is present when x and y are finite and |x|, |y| <= 1024 m, q = floor(v * 1024 + 0.5) in float64; a
 * mapping is required.  Integers only behind that one step.
 *   KEEPERS    the Goalkeeper pitch columns, mapped or not.
 *   BALL       the one Ball pitch column; absent when the table has none or carries EAGLE_POST_NO_BALL, else present on a row by the members' rule.
 *   DIRECTION  EagleOffsideParams::direction: RIGHT, group 0 attacks towards x = 105; LEFT, towards x = 0; AUTO, a vote over the rows on which both
 *            groups have a present member: s_r = sign(sum_x0 n1 - sum_x1 n0) (int64, the products stay below 2^45), neg = #{s_r < 0}, pos = #{s_r > 0},
 *            zero = #{s_r == 0}; neg > pos: group 0 defends the left and attacks RIGHT; pos > neg: LEFT; else unresolved: every row has status
 *            NO_DIRECTION and nothing else is computed (rows, margins, totals and events are as on any row that is not OK).  The votes are counted
 *            for a forced direction too.  The clip record holds the resolved direction (0: unresolved), the requested one and the counts.
 *   DEPTH      for the attacking group a with the defenders d = 1 - a: u = qx when a attacks right, else u = 107520 - qx (105 * 1024).  Greater u is
 *            nearer the defenders' goal line; U_HALF = 53760.
 *   DEFENDERS  of a row: the present members of d and every present keeper with u > U_HALF (a keeper "seen"; one exactly on the halfway line is
 *            nobody's), K of them (n_def).
 *   SECOND     a keeper was seen or assume_keeper == 0: the second-largest of the K depths as a multiset (two level defenders: second == largest);
 *            K < 2 gives status TOO_FEW.  No keeper seen and assume_keeper != 0 (the default): the keeper is taken to stand on the goal line behind
 *            everyone, second = the largest depth, K < 1 gives TOO_FEW, flag KEEPER_ASSUMED.  second_col = the earliest table column among the
 *            defenders at depth second.
 *   LINE       line = max(second, U_HALF, u_ball), the ball's term only when the ball is present on the row (else flag NO_BALL).  One of the flags
 *            BY_DEFENDER, BY_BALL, BY_HALF names the term that set it, on a tie in that order.  line_qx is the line as a pitch coordinate: u mapped
 *            back to qx.
 *   MARGINS    every present member of a: m = u - line (int32; |u| < 2^22), in an offside position iff m > 0, level is onside.  An absent member and
 *            every member on a row that is not OK: EAGLE_OFFSIDE_NONE.  The row record holds n_att (the present members of a), n_def, n_off = #{m >
 *            0}, max_margin = the greatest margin and max_col = the earliest column attaining it (NONE and -1 without an attacker).  A row that is
 *            TOO_FEW still holds n_att, n_def and keepers_seen; everything else of a row that is not OK is 0 / -1 / NONE.
 *   TOTALS     per member, in group order 0, 1 and by column inside a group, over the OK rows (of its group's record) on which it is present: rows,
 *            off_rows = #{m > 0}, max_margin (NONE when rows == 0).
 *   EVENTS     one record per event handed in (the table's possession events; none without a possession result), in their order.  status NOT_PASS:
 *            kind != EAGLE_EVENT_PASS; NO_RECEIVER: to_col is no member of group 0 or 1; NO_LINE: the record of the receiver's group at release_row
 *            is not OK, or the receiver is absent there; else OK: group = the receiver's, margin = its margin at release_row, line_qx and n_off
 *            that record's, verdict with tq = floor(tolerance * 1024 + 0.5): OFFSIDE when m > tq, else CLOSE when m > -tq, else ONSIDE (tolerance 0:
 *            never CLOSE); bypassed = the members of d present at release_row and at receive_row with u(release) > u_ball(release) and u(receive)
 *            <= u_ball(receive), -1 when the ball is absent at either row.  A record that is not OK: verdict 0, margin NONE, line_qx 0, n_off 0,
 *            bypassed -1, group = the receiver's for NO_LINE and -1 otherwise.
 * The default tolerance of 0.5 m is a conventional choice, not fitted to data.  Four launches (offside.hip: vote, rows, totals, events) on the handle's
 * main stream read the table where eagle_postprocess left it; what the call allocates is held against the table's max_bytes before the first launch.
 * EAGLE_E_INVALID with a message, before any launch and leaving every output and an earlier result alone: NULL table or parameters, a table without a
 * mapping, an unknown direction, a tolerance that is not finite or outside [0, 1024], non-zero reserved words, more than EAGLE_SHAPE_MAX_MEMBERS members
 * and keepers, more than one Ball pitch column, a column of unknown kind, a pass event whose release_row or receive_row lies outside the table, a
 * device-memory need beyond the budget.  rows == 0 is success and writes nothing. */
#define EAGLE_OFFSIDE_DIR_AUTO 0   /* EagleOffsideParams::direction, EagleOffsideClip::direction (there 0: unresolved) */
#define EAGLE_OFFSIDE_DIR_RIGHT 1  /* group 0 attacks towards x = 105 */
#define EAGLE_OFFSIDE_DIR_LEFT 2   /* group 0 attacks towards x = 0 */
#define EAGLE_OFFSIDE_OK 0         /* EagleOffsideRow::status */
#define EAGLE_OFFSIDE_NO_DIRECTION 1
#define EAGLE_OFFSIDE_TOO_FEW 2
#define EAGLE_OFFSIDE_KEEPER_ASSUMED 1     /* EagleOffsideRow::flags */
#define EAGLE_OFFSIDE_BY_DEFENDER 2
#define EAGLE_OFFSIDE_BY_BALL 4
#define EAGLE_OFFSIDE_BY_HALF 8
#define EAGLE_OFFSIDE_NO_BALL 16
#define EAGLE_OFFSIDE_EV_OK 0      /* EagleOffsideEvent::status */
#define EAGLE_OFFSIDE_EV_NOT_PASS 1
#define EAGLE_OFFSIDE_EV_NO_RECEIVER 2
#define EAGLE_OFFSIDE_EV_NO_LINE 3
#define EAGLE_OFFSIDE_ONSIDE 1     /* EagleOffsideEvent::verdict; 0: none */
#define EAGLE_OFFSIDE_CLOSE 2
#define EAGLE_OFFSIDE_OFFSIDE 3
#define EAGLE_OFFSIDE_NONE (-2147483647 - 1)       /* no margin: INT32_MIN */
#define EAGLE_OFFSIDE_U_MAX 107520 /* 105 * 1024 */
#define EAGLE_OFFSIDE_U_HALF 53760
typedef struct EagleOffsideParams {
    int32_t direction;             /* EAGLE_OFFSIDE_DIR_* (AUTO) */
    int32_t assume_keeper;         /* != 0: an unseen keeper stands on the goal line (1) */
    double tolerance;              /* metres: finite, >= 0, <= 1024 (0.5) */
    int32_t reserved[4];           /* 0 */
} EagleOffsideParams;              /* 32 bytes */
typedef struct EagleOffsideRow {
    int32_t status;                /* EAGLE_OFFSIDE_OK .. EAGLE_OFFSIDE_TOO_FEW */
    int32_t flags;                 /* EAGLE_OFFSIDE_KEEPER_ASSUMED .. EAGLE_OFFSIDE_NO_BALL; 0 unless OK */
    int32_t line_qx;               /* the line as a pitch coordinate, q; 0 unless OK */
    int32_t second_col;            /* the second-last opponent's table column; -1 unless OK */
    int32_t n_att, n_def;          /* present attackers; defenders K, seen keepers included; 0 on NO_DIRECTION */
    int32_t keepers_seen;
    int32_t n_off;                 /* attackers with m > 0 */
    int32_t max_margin;            /* EAGLE_OFFSIDE_NONE without an attacker or unless OK */
    int32_t max_col;               /* the earliest column attaining it, or -1 */
    int32_t reserved[2];           /* 0 */
} EagleOffsideRow;                 /* 48 bytes */
typedef struct EagleOffsideTotals {
    int32_t col, group;            /* the member's table column and group */
    int32_t rows;                  /* OK rows on which it is present */
    int32_t off_rows;              /* ... with m > 0 */
    int32_t max_margin;            /* EAGLE_OFFSIDE_NONE when rows == 0 */
    int32_t reserved[3];           /* 0 */
} EagleOffsideTotals;              /* 32 bytes */
typedef struct EagleOffsideEvent {
    int32_t status;                /* EAGLE_OFFSIDE_EV_* */
    int32_t verdict;               /* EAGLE_OFFSIDE_ONSIDE .. EAGLE_OFFSIDE_OFFSIDE; 0 unless OK */
    int32_t margin;                /* the receiver's at release_row, q; EAGLE_OFFSIDE_NONE unless OK */
    int32_t line_qx;               /* the line at release_row */
    int32_t n_off;                 /* the receiver's team in an offside position at release_row */
    int32_t bypassed;              /* opponents the pass takes out of the game; -1: no ball at either row, or not OK */
    int32_t group;                 /* the receiver's group; -1 for NOT_PASS and NO_RECEIVER */
    int32_t reserved;              /* 0 */
} EagleOffsideEvent;               /* 32 bytes */
typedef struct EagleOffsideClip {
    int32_t direction;             /* resolved: EAGLE_OFFSIDE_DIR_RIGHT or _LEFT; 0: unresolved */
    int32_t requested;             /* EagleOffsideParams::direction */
    int32_t neg, pos, zero;        /* the vote */
    int32_t n_members[2];          /* members of groups 0 and 1 */
    int32_t n_keepers;
} EagleOffsideClip;                /* 32 bytes */
/* The result is kept with the table until eagle_post_free.  A call computes into a buffer of its own and frees the earlier result only when the new one
 * is complete, as eagle_post_space does: a refused call and a call that fails later both leave the earlier result in place.  The events are those of the
 * table's possession result at the time of the call. */
int eagle_post_offside(EagleHandle* h, EaglePostTable* t, const EagleOffsideParams* p);
/* To the host: rows_out [rows][2] (the attacking group is the second index), margins int32 [members][rows] in group order, totals_out [members], one
 * clip record; any pointer may be NULL. */
int eagle_post_offside_values(EaglePostTable* t, EagleOffsideRow* rows_out, int32_t* margins, EagleOffsideTotals* totals_out, EagleOffsideClip* clip_out);
/* *n = the number of event records of the last eagle_post_offside (0 before it); at most cap are written, in event order. */
int eagle_post_offside_events(const EaglePostTable* t, EagleOffsideEvent* out, int cap, int* n);
/* In HBM; all NULL (and 0 members, 0 events) before eagle_post_offside.  n_members and n_events may be NULL. */
int eagle_post_device_offside(const EaglePostTable* t, const EagleOffsideRow** d_rows, const int32_t** d_margins, const EagleOffsideTotals** d_totals,
                              const EagleOffsideClip** d_clip, const EagleOffsideEvent** d_events, int* n_members, int* n_events);
/* Operator entry (host buffers in / out, no handle) for constructed tables, as eagle_op_space; frames [rows] is carried for symmetry with
 * eagle_op_possession and not read (it may be NULL); events [n_events] as eagle_op_possession gives them (NULL with n_events == 0); every output may be
 * NULL. */
int eagle_op_offside(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                     const int32_t* team_vals, int n_team, const EagleOffsideParams* p, const EaglePossessionEvent* events, int n_events,
                     EagleOffsideRow* rows_out, int32_t* margins, EagleOffsideTotals* totals_out, EagleOffsideClip* clip_out, EagleOffsideEvent* events_out);

/* ---- ball track: which ball detection of every frame lies on the best physically possible path through the clip (own specification:
 * tests/balltrack_ref.py defines every output bit) ----
 * eagle_postprocess takes a frame's only ball detection whatever it is and, of several, the one nearest the image origin (above: the reference's
 * parse_ball_detections_with_kalman(filter=False)).  This stage is the library's own, opt-in answer: over the whole clip it takes the sequence of
 * candidates that forms the best path; isolated false positives drop out (the table then interpolates over them), a frame with several candidates is
 * decided by the frames around it, a camera cut (eagle_shots_frames) breaks the path.  Integers only: no order of accumulation exists.
 *   NODES      frame i of the n records: its reported ball detections (cls == 2, reported) in eagle_postprocess's order (one per id, the later record of
 *              an id in the earlier one's place, then stably by descending conf).  The first EAGLE_BALL_MAX_CAND are nodes (i, 0 ..); the others are
 *              ignored and the frame is flagged.  Position in half pixels, exact: qx = (bx1 & 0xFFFF) + (bx2 & 0xFFFF), qy = 2 (by2 & 0xFFFF), the image
 *              point of eagle_postprocess.  cq = floor(conf * 1024); conf must be finite and within [0, 1].
 *   PARAMETERS resolved to integers, pixels as floor(2 v + 0.5) half pixels; 0 stands for the default: V half pixels per frame (speed; 0.1 frame_w
 *              pixels, the reference filter's threshold), G frames (gap, 1 .. 64; min(64, fps)), R0 (reward; V) and B (brk; (5 R0) >> 1).  Conventional
 *              choices, not fitted to data: a sighting of confidence 1 pays for any admissible one-frame step, and a track needs about three sightings
 *              to pay for itself.
 *   SCORE      R(i, a) = (cq R0) >> 10.  A link (i, a) -> (j, b) is admissible when i < j <= i + G, both frames lie in one shot (cuts: the sorted
 *              frames that start a new shot) and d2 = dx dx + dy dy <= (V (j - i))^2 (int64); it costs isqrt(d2), the exact floor.  Per shot, with
 *              P(-1) = 0:  f(j, b) = R(j, b) + max(P(j - 1) - B, max over admissible links of f(i, a) - cost),  P(j) = max(P(j - 1), max_b f(j, b)).
 *   TIES       a link is taken when it is at least as good as the break; among links the larger i wins, then the smaller a; P's arg-max moves only on a
 *              strictly greater f, within a frame to the lowest b; a break's predecessor is that arg-max when P(j - 1) > 0, otherwise it has none.
 *   CHOSEN     per shot with P(end) > 0 the predecessors back from the arg-max.  A tracklet is a maximal run of chosen nodes joined by links, numbered
 *              from 0 in frame order; its gain is its rewards minus its links' costs minus B, and the gains add up to the clip's score, the sum of the
 *              shots' P(end).
 * Launches (balltrack.hip): the recurrence with one wave per piece of the timeline (a shot, cut further at its runs of at least G frames without a
 * candidate, which no link crosses), the pieces chained per shot, the chosen nodes marked by pointer doubling, then rows, a prefix sum of the tracklet
 * starts, the tracklets and the totals.  Host C++ stages the candidates.
 * EAGLE_E_INVALID with a message, before any launch and leaving every output and an earlier result alone: NULL pointers (parameters, the result; recs,
 * counts, positions with n > 0; cuts with n_cuts > 0; neither cq nor conf), n < 0 or n > 2^20, an n_det outside 0 .. EAGLE_MAX_DET (a count outside
 * it), cuts that are unsorted, repeated or outside 1 .. n - 1, fps or frame_w not positive, gap outside 0 .. 64, a speed, reward or brk that is not
 * finite, is negative or exceeds 65535 / 65535 / 2^20 pixels, a frame_w whose default speed exceeds 65535 pixels, non-zero reserved words, a conf
 * outside [0, 1] or not finite, a position outside 0 .. 131070, a cq outside 0 .. 1024, a device-memory need beyond the budget (max_bytes; 0: nine tenths of what is
 * free).  n == 0 succeeds and writes nothing. */
#define EAGLE_BALL_MAX_CAND 8
#define EAGLE_BALL_TOO_MANY 1          /* EagleBallFrame::flags: the frame had more candidates than EAGLE_BALL_MAX_CAND */
#define EAGLE_BALL_SHOT_START 2        /* frame 0 and every cut */
#define EAGLE_BALL_TRACKLET_START 4    /* the chosen node was reached by a break, or by nothing */
#define EAGLE_BALL_RECOVER_DEFAULT 0   /* eagle_op_ball_track's `recover`: how the chosen nodes are found; the default is the faster at 30 000 frames */
#define EAGLE_BALL_RECOVER_DOUBLING 1  /* jump tables by pointer doubling, marking from the end nodes with the powers high to low */
#define EAGLE_BALL_RECOVER_CHASE 2     /* one lane per shot follows the predecessors */
typedef struct EagleBallTrack EagleBallTrack;
typedef struct EagleBallTrackParams {
    int32_t fps, frame_w;          /* > 0 */
    int32_t gap;                   /* G in frames, 1 .. 64; 0: min(64, fps) */
    int32_t reserved[5];           /* 0 */
    double speed, reward, brk;     /* pixels (per frame); 0: the default */
    int64_t max_bytes;             /* device-memory budget of the call, 0 = nine tenths of what is free */
} EagleBallTrackParams;            /* 64 bytes */
typedef struct EagleBallFrame {
    int32_t cand;                  /* the chosen node's index among the frame's candidates, -1: none */
    int32_t det;                   /* the index in EagleFrameResult::det it came from (eagle_op_ball_track: what `det` holds, -1 without), -1: none */
    int32_t tracklet;              /* -1: none */
    int32_t flags;                 /* EAGLE_BALL_TOO_MANY | _SHOT_START | _TRACKLET_START */
    int32_t qx, qy;                /* half pixels; 0 without a chosen node */
    int64_t f;                     /* the recurrence's value at the chosen node; 0 without */
} EagleBallFrame;                  /* 32 bytes */
typedef struct EagleBallTracklet {
    int32_t first, last;           /* frames */
    int32_t shot, sightings;
    int64_t sum_cq;
    int64_t length;                /* the links' costs, half pixels */
    int64_t gain;                  /* rewards - length - B */
    int32_t reserved[2];
} EagleBallTracklet;               /* 48 bytes */
typedef struct EagleBallClip {
    int32_t frames_with;           /* frames with at least one candidate */
    int32_t frames_chosen;
    int32_t rejected;              /* nodes that were not chosen */
    int32_t frames_multi;          /* frames with several candidates */
    int32_t tracklets, shots;
    int32_t ignored;               /* candidates beyond EAGLE_BALL_MAX_CAND of their frame */
    int32_t reserved;
    int64_t score;
    int32_t V, G, R0, B;           /* the resolved parameters */
    int32_t reserved2[2];
} EagleBallClip;                   /* 64 bytes */
/* The result is kept on the host with *out until eagle_ball_track_free; the launches run on the handle's main stream.  cuts may be NULL with n_cuts == 0. */
int eagle_ball_track(EagleHandle* h, const EagleFrameResult* recs, int n, const int32_t* cuts, int n_cuts, const EagleBallTrackParams* p, EagleBallTrack** out);
int eagle_ball_track_values(const EagleBallTrack* t, EagleBallFrame* frames_out /* [n] */, EagleBallClip* clip_out);        /* either may be NULL */
int eagle_ball_track_tracklets(const EagleBallTrack* t, EagleBallTracklet* out, int cap, int* n);                           /* *n = their number; at most cap are written */
void eagle_ball_track_free(EagleBallTrack* t);
/* Operator entry (host buffers in / out, no handle): counts [n] candidates per frame (0 .. EAGLE_MAX_DET), positions [sum of counts][2] half pixels and
 * cq [sum] (or, with cq NULL, conf [sum] float32) frame after frame in descending confidence, det [sum] or NULL.  Every output may be NULL; at most cap
 * tracklets are written (EagleBallClip::tracklets is their number).  times_ms (may be NULL): device events around the recurrence with its chaining, the
 * recovery of the chosen nodes, the row / prefix-sum / tracklet launches, and all of them. */
int eagle_op_ball_track(int device, const int32_t* counts, int n, const int32_t* positions, const int32_t* cq, const float* conf, const int32_t* det,
                        const int32_t* cuts, int n_cuts, const EagleBallTrackParams* p, int recover, EagleBallFrame* frames_out, EagleBallTracklet* tracklets_out,
                        int cap, EagleBallClip* clip_out, float* times_ms /* [4] */);
/* eagle_postprocess with the ball of frame i given: ball_det[i] is -1 (no ball) or the index of a reported ball detection of record i (EagleBallFrame::det).
 * The table is the one eagle_postprocess builds from records in which every other reported ball detection is dropped, so fewer than two sightings still
 * give EAGLE_POST_NO_BALL, and Ball and Ball_video of a row come from the same detection.  ball_det == NULL is eagle_postprocess exactly.  A ball_det
 * entry that is not a reported ball detection of its record is EAGLE_E_INVALID, before anything is built. */
int eagle_postprocess_ball(EagleHandle* h, const EagleFrameResult* recs, int n, const EaglePostParams* p, const int32_t* ball_det, EaglePostTable** out);

/* ---- shots: the camera cuts, gradual transitions and photo flashes of a clip, and which of its shots look at the pitch (own specification:
 * tests/shots_ref.py defines every output bit) ----
 * The stage in front of the networks: every other stage assumes one continuous shot of the main camera.  Input: n dense BGR frames [h][w][3], P = h w.
 *   SIGNATURE  of a frame, EAGLE_SHOT_SIGNATURE = 1537 u32: hist [512], the pixels per bin (b >> 5) 64 + (g >> 5) 8 + (r >> 5); tile [16][64], a 4 x 4 grid
 *            of tiles of th = h / 4 rows and tw = w / 4 columns over the top-left 4 th x 4 tw pixels, tile 4 ty + tx counting the bins (b >> 6) 16 +
 *            (g >> 6) 4 + (r >> 6) (the up to 3 remaining rows and columns count in hist and grass only; A = th tw); grass, the pixels with g >= 48 and
 *            g - max(r, b) >= 16.
 *   SCORE    of a frame pair in 1 / 65536, integers throughout: sg = 65536 sum |hist_a - hist_b| / (2 P); st = 65536 u / (16 A), u the sum of the 8
 *            smallest of the 16 tile distances sum_64 |tile_a - tile_b| (the 8 largest are dropped: captions, local motion); S = max(sg, st).
 *   FRAMES   per frame i: d1 = S(i-1, i), d2 = S(i-2, i), dW = S(i-W, i), 0 where the earlier frame does not exist; sg and st of the d1 pair; grass.
 *   FLASH    f >= 1, d1[f] >= cut, f + 1 < n and d2[f+1] < low: the picture returns to what it was.  A flash in the last frame is a cut.
 *   HARD CUT i >= 1, d1[i] >= cut, neither i nor i - 1 a flash.
 *   GRADUAL  i is eligible when i >= W, dW[i] >= cut, no hard cut lies in [i-W+1, i] and neither i nor i - W is a flash; it ends a transition when
 *            dW[i] is greater than dW of every eligible frame of [i-W+1, i-1] and at least dW of every eligible frame of [i+1, i+W-1] (the first
 *            maximum).  The frames [i-W+1, i-1] are then IN_TRANSITION and form a shot of kind TRANSITION; a new shot starts at i.  Two ends lie at
 *            least W frames apart.
 *   SHOTS    the runs between boundaries (frame 0, a hard cut, a transition's first frame, a gradual end), in frame order.  kind: TRANSITION, else
 *            AFTER_TRANSITION at a gradual end, else AFTER_CUT, else START.  grass_sum: the sum of grass over its frames.  PITCH: kind != TRANSITION
 *            and grass_sum 65536 >= grass_thr P count; SHORT: count < min_len; USABLE: PITCH and not SHORT.
 * The defaults (eagle_amd/shots.py: cut 0.30, low 0.10, grass_thr 0.35, W = max(2, round(0.4 fps)), min_len = fps) are conventional choices; nothing
 * here is fitted to or validated on broadcast footage.  The stage finds boundaries: beyond "looks at grass" it does not classify camera angles, and a
 * wipe longer than W frames shows only through the grass share of what follows it.
 * Launches (shots.hip) on the handle's main stream; the signatures (6148 bytes per frame) are allocated per call and freed.  The handle's records,
 * staging buffers and graphs are not involved.
 * EAGLE_E_INVALID with a message that names the value, before any launch and leaving every output alone: NULL pointers (frames with n > 0, parameters,
 * n_shots; frames_out with n > 0), n < 0, cap < 0, window < 2, min_len < 1, a threshold outside 0 .. 65536, low > cut, non-zero reserved words; in the
 * operator entry h < 4, w < 4 or h w > 2^30; in the host entry strides below a dense frame's.  More shots than cap (or shots_out NULL with shots to report):
 * EAGLE_E_INVALID, *n_shots holds the count, the other outputs are left alone.  n == 0 is success with *n_shots = 0. */
#define EAGLE_SHOT_SIGNATURE 1537
#define EAGLE_SHOT_START 0             /* EagleShot::kind */
#define EAGLE_SHOT_AFTER_CUT 1
#define EAGLE_SHOT_AFTER_TRANSITION 2
#define EAGLE_SHOT_TRANSITION 3
#define EAGLE_SHOT_FRAME_FLASH 1       /* EagleShotFrame::flags */
#define EAGLE_SHOT_FRAME_HARD 2
#define EAGLE_SHOT_FRAME_GRADUAL_END 4
#define EAGLE_SHOT_FRAME_IN_TRANSITION 8
#define EAGLE_SHOT_PITCH 1             /* EagleShot::flags */
#define EAGLE_SHOT_SHORT 2
#define EAGLE_SHOT_USABLE 4
typedef struct EagleShotParams {
    int32_t cut;                   /* 1 / 65536: 0 .. 65536 */
    int32_t low;                   /* 1 / 65536: 0 .. cut */
    int32_t grass_thr;             /* 1 / 65536: 0 .. 65536 */
    int32_t window;                /* W >= 2 frames */
    int32_t min_len;               /* >= 1 frames */
    int32_t reserved[3];           /* 0 */
} EagleShotParams;                 /* 32 bytes */
typedef struct EagleShotFrame {
    int32_t d1, d2, dW;            /* S against the frame 1, 2 and W earlier */
    int32_t sg, st;                /* of the d1 pair */
    uint32_t grass;
    int32_t flags;                 /* EAGLE_SHOT_FRAME_* */
    int32_t reserved;              /* 0 */
} EagleShotFrame;                  /* 32 bytes */
typedef struct EagleShot {
    int32_t first, count;
    int32_t kind;                  /* EAGLE_SHOT_START .. EAGLE_SHOT_TRANSITION */
    int32_t flags;                 /* EAGLE_SHOT_PITCH | _SHORT | _USABLE */
    int64_t grass_sum;
    int32_t reserved[2];           /* 0 */
} EagleShot;                       /* 32 bytes */
/* n frames of the handle's size, dense, resident in HBM -> frames_out [n], shots_out [*n_shots <= cap]; returns when they are complete. */
int eagle_shots_device_frames(EagleHandle* h, const uint8_t* d_bgr, int n, const EagleShotParams* p, EagleShotFrame* frames_out, EagleShot* shots_out, int cap, int* n_shots);
/* Same for frames in host memory (pageable or pinned; row_stride >= 3 w, frame_stride >= (h - 1) row_stride + 3 w, 0 = dense), uploaded in passes of what
 * max_staging_bytes (0: 64 MB; always at least one frame) of device staging hold.  The signatures of all n frames stay resident over the passes and the
 * scores are formed behind the last one, so the result does not depend on the size of a pass. */
int eagle_shots_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t row_stride, int64_t frame_stride, int64_t max_staging_bytes, const EagleShotParams* p,
                       EagleShotFrame* frames_out, EagleShot* shots_out, int cap, int* n_shots);
/* Operator entry (host buffers in / out, no handle): dense frames of any h, w >= 4; signatures_out (may be NULL): [n][EAGLE_SHOT_SIGNATURE] u32. */
int eagle_op_shots(int device, const uint8_t* bgr, int n, int h, int w, const EagleShotParams* p, EagleShotFrame* frames_out, EagleShot* shots_out, int cap, int* n_shots,
                   uint32_t* signatures_out);

/* ---- top view: the frames warped onto the pitch plane, their mean (a mosaic of the pitch without the players) and per frame the distance of its
 * warp from that mean (own specification: tests/topview_ref.py defines every output byte) ----
 * What shows whether a frame's homography H (row-major, image -> pitch) puts the painted lines where the pitch model has them, and which frames of a
 * clip have an H that jumped.  Input: n dense BGR frames [h][w][3], Hs [n][9], valid [n].
 *   CANVAS   the minimap's: scale S even in 2 .. 32, margin M even in 0 .. 64, W = 105 S + 2 M, Hc = 68 S + 2 M.  Pixel (X, Y) stands for the pitch
 *            point x = (X - M) / S, y = 68 - (Y - M) / S (float64, one operation each), so the minimap's marking mask fits without a shift.
 *   MAP      per frame on the host, float64, every product and sum a single operation: A = adj(H), the cofactors A0 = h4 h8 - h5 h7, A1 = h2 h7 - h1 h8,
 *            A2 = h1 h5 - h2 h4, A3 = h5 h6 - h3 h8, A4 = h0 h8 - h2 h6, A5 = h2 h3 - h0 h5, A6 = h3 h7 - h4 h6, A7 = h1 h6 - h0 h7, A8 = h0 h4 - h1 h3;
 *            det = (h0 A0 + h1 A3) + h2 A6; sb = (h6 (w - 1) / 2 + h7 (h - 1)) + h8, the projective weight of the frame's bottom-centre pixel.  The
 *            frame has NO MAP when valid is 0, when any of H, A, det, sb is not finite, when det == 0 or sb == 0.  Else G = A when det and sb have
 *            the same sign, G = -A otherwise: exactly the pitch points on the same side of the horizon as the bottom of the picture are kept, and H
 *            and c H (c != 0) give the same bytes.
 *   SAMPLE   u' = ((G0 x) + (G1 y)) + G2, v' and w' likewise from rows 1 and 2; u = u' / w', v = v' / w'; tu = u 256 + 0.5, tv = v 256 + 0.5.  The
 *            pixel is COVERED iff w' > 0, 0 <= tu < 256 (w - 1) + 1 and 0 <= tv < 256 (h - 1) + 1 (NaN fails).  Then U = floor(tu), x0 = U >> 8,
 *            fx = U & 255, x1 = min(x0 + 1, w - 1), likewise in y, and each channel is ((256 - fx)(256 - fy) p00 + fx (256 - fy) p10 +
 *            (256 - fx) fy p01 + fx fy p11 + 32768) >> 16.  Pixel centres lie at integers; no parity with cv2.warpPerspective is claimed.
 *   VIDEO    covered pixels get the sample, the others `background`; with `markings` the minimap's marking mask of (S, M) is painted on top in
 *            `marking_colour`.  BGR, NV12 or I420 in the caller's layout, as eagle_annotate_* (same conversion, same layout rules).
 *   MOSAIC   over the frames first, first + step, ...: u32 sums sumB, sumG, sumR and cnt per canvas pixel (the accumulator, u32 [Hc][W][4]).  A frame adds
 *            its sample iff the pixel is covered and, with mask_boxes, (u, v) lies in no box det[0 .. n_det) of the frame's record (any class):
 *            x1 - box_pad <= u <= x2 + box_pad and y1 - box_pad <= v <= y2 + box_pad in float64, the float boxes widened exactly.  The picture:
 *            channel = (2 sum + cnt) / (2 cnt) (integer division) where cnt >= min_count, `background` elsewhere, markings on request; dense BGR
 *            [Hc][W][3], and cnt as u32 [Hc][W].  At most EAGLE_TOPVIEW_MAX_FRAMES frames, below which the sums cannot overflow.
 *   RESIDUAL for every frame f of the clip (first and step do not matter here): over the pixels f would add to the mosaic (covered, not masked)
 *            where the accumulator has cnt >= min_count, res_sum[f] = the sum of |sample - mosaic channel| over B, G, R and res_cnt[f] their number;
 *            covered[f] = the covered pixels with M <= X < M + 105 S and M <= Y < M + 68 S.  The frame's own sample is part of the mosaic.
 * All accumulation is in integers: no result depends on how the kernels split the work, two runs give the same bytes.  Limits: bilinear only, no
 * anti-aliasing where the view is minified, no lens distortion; a plain mean, not a median, so a player who stands still through the clip and is not
 * box-masked leaves a ghost; nothing is validated on real footage.  Launches (topview.hip) on the handle's main stream; device memory is allocated
 * per call and freed (the marking mask is the handle's, shared with the minimap); records, staging buffers and graphs of the handle are not involved.
 * EAGLE_E_INVALID with a message, before any launch: NULL pointers (parameters, outputs; frames, Hs, valid with n > 0), scale or margin outside the
 * ranges above, step < 1, first < 0, min_count < 1, box_pad negative or not finite, a colour above 0xffffff, non-zero reserved words, n < 0, n above
 * EAGLE_TOPVIEW_MAX_FRAMES for a mosaic, mask_boxes without records (or with an n_det outside 0 .. EAGLE_MAX_DET), every layout error eagle_annotate_*
 * refuses, a negative max_staging_bytes; in the operator entry a frame side outside 1 .. 16384 or an unknown mode.  n == 0 succeeds and writes nothing;
 * a mosaic of 0 frames is all background with cnt = 0. */
#define EAGLE_TOPVIEW_MAX_FRAMES (1 << 23)
#define EAGLE_TOPVIEW_VIDEO 1          /* eagle_op_topview: mode bits */
#define EAGLE_TOPVIEW_MOSAIC 2
#define EAGLE_TOPVIEW_RESIDUAL 4
typedef struct EagleTopviewParams {
    int32_t scale, margin;         /* S, M */
    uint32_t background;           /* B | G << 8 | R << 16 (conventionally black) */
    int32_t markings;              /* != 0: paint the marking mask */
    uint32_t marking_colour;       /* B | G << 8 | R << 16 (conventionally red, 0xff0000) */
    int32_t mask_boxes;            /* != 0: mosaic and residual leave out the samples inside the frame's detection boxes */
    double box_pad;                /* pixels, >= 0 */
    int32_t first, step;           /* the mosaic's frames: first, first + step, ... */
    int32_t min_count;             /* >= 1 (conventionally 1) */
    int32_t reserved[3];           /* 0 */
} EagleTopviewParams;              /* 56 bytes */
int eagle_topview_size(const EagleTopviewParams* p, int* w, int* h);
/* n frames of the handle's size, dense, resident in HBM -> n pictures at d_out (device) in out_format / out_layout; returns when they are complete.
 * Hs [n][9] and valid [n] are host memory. */
int eagle_topview_device_frames(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleTopviewParams* p, int out_format,
                                const EagleYuvLayout* out_layout, void* d_out);
/* Same, dense frames in host memory -> pictures in host memory, in passes of what 64 MB of device staging hold (pinned or pageable destination, as
 * eagle_minimap_frames). */
int eagle_topview_frames(EagleHandle* h, const uint8_t* bgr, int n, const double* Hs, const uint8_t* valid, const EagleTopviewParams* p, int out_format,
                         const EagleYuvLayout* out_layout, uint8_t* out);
/* The frames first, first + step, ... of a clip resident in HBM are added to the accumulator d_acc (device, u32 [Hc][W][4], eagle_device_alloc; reset != 0:
 * zeroed first, so that several clips or calls can share one).  recs (host, [n]): NULL unless mask_boxes.  Returns when the sums are complete. */
int eagle_topview_mosaic_device(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                const EagleTopviewParams* p, uint32_t* d_acc, int reset);
/* The accumulator -> the mosaic picture bgr_out [Hc][W][3] and cnt_out u32 [Hc][W] (host). */
int eagle_topview_mosaic_finish(EagleHandle* h, const uint32_t* d_acc, const EagleTopviewParams* p, uint8_t* bgr_out, uint32_t* cnt_out);
/* The residual triples of all n frames against the finished accumulator -> res_sum, res_cnt, covered (host, [n]). */
int eagle_topview_residual_device(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                  const EagleTopviewParams* p, const uint32_t* d_acc, uint64_t* res_sum, uint32_t* res_cnt, uint32_t* covered);
/* The last two steps for a clip in host memory (dense [n][h][w][3]): the frames a step needs are uploaded in passes of what max_staging_bytes (0: 64 MB;
 * always at least one frame) of device staging hold; the accumulator stays resident across the passes, the clip is read once per step, and the result
 * does not depend on the size of a pass. */
int eagle_topview_mosaic_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t max_staging_bytes, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                const EagleTopviewParams* p, uint32_t* d_acc, int reset);
int eagle_topview_residual_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t max_staging_bytes, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                  const EagleTopviewParams* p, const uint32_t* d_acc, uint64_t* res_sum, uint32_t* res_cnt, uint32_t* covered);
/* Operator entry (host buffers in / out, no handle): dense frames of any h x w within 1 .. 16384 per side.  boxes [box_off[n]][4] = x1, y1, x2, y2 and
 * box_off [n + 1] (ascending from 0, at most EAGLE_MAX_DET per frame) stand for the records; NULL unless mask_boxes.  mode: EAGLE_TOPVIEW_VIDEO (out, in
 * out_format / out_layout) | _MOSAIC (mosaic_out [Hc][W][3], cnt_out [Hc][W]) | _RESIDUAL (res_sum, res_cnt, covered [n], against the mosaic of this
 * call's frames); outputs of modes not asked for may be NULL. */
int eagle_op_topview(int device, const uint8_t* bgr, int n, int h, int w, const double* Hs, const uint8_t* valid, const float* boxes, const int32_t* box_off,
                     const EagleTopviewParams* p, int mode, int out_format, const EagleYuvLayout* out_layout, uint8_t* out, uint8_t* mosaic_out, uint32_t* cnt_out,
                     uint64_t* res_sum, uint32_t* res_cnt, uint32_t* covered);

/* ---- ground layer: shapes that lie on the pitch plane, blended into the grass of the camera picture under the players (own specification:
 * tests/ground_ref.py defines every output byte) ----
 * What puts an offside line, its zone and a ring under a player's feet into the frame itself, as a broadcaster shows them.  Input: n dense BGR frames
 * [h][w][3], Hs [n][9] (row-major, image -> pitch, as in the records), valid [n], and per frame the shapes shapes[off[f] .. off[f + 1]) (off [n + 1]
 * ascends from 0), at most EAGLE_GROUND_MAX_SHAPES per frame.
 *   MAP      per frame; pixel centres lie at integers, as in the top view.  sb = (h6 (w - 1) / 2 + h7 (h - 1)) + h8 in float64, every operation single:
 *            the projective weight of the frame's bottom-centre pixel.  The frame has NO MAP when valid is 0, when any h_i or sb is not finite, or
 *            when sb == 0; it is then passed through: its source pixels in the output format, covered = 0.
 *   SAMPLES  four per pixel (X, Y), a rotated grid with the offsets (dx, dy) = (-0.375, -0.125), (0.125, -0.375), (0.375, 0.125), (-0.125, 0.375):
 *            u = X + dx, v = Y + dy; x' = ((h0 u) + (h1 v)) + h2, y' and w' likewise from rows 1 and 2.  A sub-sample is ON THE GROUND iff w' and sb
 *            have the same strict sign (the same side of the horizon as the bottom of the picture, so H and c H, c != 0, give the same bytes) and
 *            px = x' / w', py = y' / w' are finite with |px|, |py| <= 1024.  Then qx = floor(px 1024 + 0.5), qy likewise, as int32: the quantisation
 *            q of the team-shape, space and offside stages.  Everything behind it is integers.
 *   SHAPES   EAGLE_GROUND_BAND, a = x0, x1, y0, y1: inside iff x0 <= qx < x1 and y0 <= qy < y1 (half-open).  EAGLE_GROUND_RING, a = cx, cy, r0, r1
 *            with 0 <= r0 < r1 <= 2^20: inside iff r0^2 <= (qx - cx)^2 + (qy - cy)^2 < r1^2 in int64.  Flag EAGLE_GROUND_KEYED: the shape is drawn
 *            only where the SOURCE pixel is grass, g >= key_min and g - max(r, b) >= key_lead (the shots stage's rule with its 48 and 16, which are
 *            conventional choices, not fitted to footage).
 *   BLEND    per pixel over the frame's shapes in list order, starting from the source pixel: c = the number of its four sub-samples that are on the
 *            ground and inside the shape; the shape is skipped when c == 0, when alpha == 0, or when it is KEYED and the source pixel is not grass;
 *            else A = alpha c (at most 1024) and every channel becomes (channel (1024 - A) + colour A + 512) >> 10.  covered[f] = the pixels of
 *            frame f that at least one shape blended into: an integer sum, independent of how the work is split, the same in two runs.
 *   OUTPUT   BGR, NV12 or I420 in the caller's layout, as eagle_annotate_* (same conversion, same layout rules).
 * Limits: the key is a colour rule per pixel of the source frame, no matting and no smoothing over time, so green kits and shadows key wrongly; a shape
 * is only as well placed as the frame's homography; no lens distortion; four sub-samples, so a band narrower than a far-side pixel thins out; bands are
 * axis-aligned on the pitch; nothing is validated on real footage.  One launch per 65535 frames (ground.hip) on the handle's main stream; the table of
 * maps, the shapes and the counts are allocated per call and freed; records, staging buffers and graphs of the handle are not involved.  no_cull = 1
 * switches off the kernel's per-tile rejection of shapes for measurements; the bytes are the same either way.
 * EAGLE_E_INVALID with a message, before any launch and leaving every output alone: NULL pointers (parameters, off; frames, Hs, valid, the output with
 * n > 0; shapes with off[n] > 0), n < 0, off not ascending from 0 or more than EAGLE_GROUND_MAX_SHAPES shapes in a frame, an unknown kind or flag,
 * alpha outside 0 .. 256, a colour above 0xffffff, a band with x0 >= x1 or y0 >= y1 or an argument beyond +-2^21, a ring with a centre coordinate
 * beyond +-2^21 or radii outside 0 <= r0 < r1 <= 2^20, non-zero reserved words (a[4], a[5] and reserved of a shape, reserved of the parameters), key_min
 * or key_lead outside 0 .. 255, no_cull other than 0 or 1, every layout error eagle_annotate_* refuses (odd h or w with a 4:2:0 format among them), a
 * negative max_staging_bytes; d_out equal to d_bgr; in the operator entry a frame side outside 1 .. 16384.  n == 0 succeeds and writes nothing.  covered may
 * be NULL. */
#define EAGLE_GROUND_MAX_SHAPES 16
#define EAGLE_GROUND_BAND 0            /* EagleGroundShape::kind */
#define EAGLE_GROUND_RING 1
#define EAGLE_GROUND_KEYED 1           /* EagleGroundShape::flags */
typedef struct EagleGroundShape {
    int32_t kind;                  /* EAGLE_GROUND_BAND, EAGLE_GROUND_RING */
    int32_t a[6];                  /* band: x0, x1, y0, y1; ring: cx, cy, r0, r1 (1 / 1024 m); a[4] = a[5] = 0 */
    uint32_t colour;               /* B | G << 8 | R << 16 */
    int32_t alpha;                 /* 0 .. 256 per sub-sample */
    int32_t flags;                 /* EAGLE_GROUND_KEYED */
    int32_t reserved[2];           /* 0 */
} EagleGroundShape;                /* 48 bytes */
typedef struct EagleGroundParams {
    int32_t key_min, key_lead;     /* 0 .. 255 (conventionally 48 and 16) */
    int32_t no_cull;               /* 0; 1: measure without the per-tile rejection */
    int32_t reserved;              /* 0 */
} EagleGroundParams;               /* 16 bytes */
/* n frames of the handle's size, dense, resident in HBM -> n pictures at d_out (device, another buffer than d_bgr) in out_format / out_layout, and
 * covered [n] (host); returns when they are complete.  Hs, valid, shapes and off are host memory. */
int eagle_ground_device_frames(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleGroundShape* shapes, const int32_t* off,
                               const EagleGroundParams* p, int out_format, const EagleYuvLayout* out_layout, void* d_out, uint32_t* covered);
/* Same, dense frames in host memory -> pictures in host memory (pinned or pageable, as eagle_minimap_frames), in passes of what max_staging_bytes (0:
 * 64 MB; always at least one frame) of device staging hold.  The result does not depend on the size of a pass. */
int eagle_ground_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t max_staging_bytes, const double* Hs, const uint8_t* valid, const EagleGroundShape* shapes,
                        const int32_t* off, const EagleGroundParams* p, int out_format, const EagleYuvLayout* out_layout, uint8_t* out, uint32_t* covered);
/* Operator entry (host buffers in / out, no handle) for constructed inputs: dense frames of any h x w within 1 .. 16384 per side. */
int eagle_op_ground(int device, const uint8_t* bgr, int n, int h, int w, const double* Hs, const uint8_t* valid, const EagleGroundShape* shapes, const int32_t* off,
                    const EagleGroundParams* p, int out_format, const EagleYuvLayout* out_layout, uint8_t* out, uint32_t* covered);

/* ---- line registration: each frame's homography moved until the frame's painted-line pixels lie on the pitch model's lines (own specification:
 * tests/linefit_ref.py defines every bit of the masks, the matrices and the records) ----
 * The one stage that measures a homography against something absolute, before anything is projected with it.  Input: n dense BGR frames [h][w][3],
 * Hs [n][9] (row-major, image -> pitch), valid [n], optionally the detection boxes of each frame.  Lengths held in integers are in Q = 1 / 1024 m.
 *   LINE PIXELS  Y = b + 2 g + r; grass: g >= 48 and g - max(r, b) >= 16.  A pixel (x, y) with k <= x <= w - 1 - k and k <= y <= h - 1 - k is a line
 *            pixel iff for the horizontal or the vertical direction d both p - k d and p + k d are grass and Y(p) - max(Y(p - k d), Y(p + k d)) >= tau,
 *            and it lies in no detection box widened by box_pad (x1 - box_pad <= x <= x2 + box_pad, likewise y, float64, inclusive).  The mask of a
 *            frame is u32 [h][(w + 31) / 32], pixel x in bit x & 31 of word x >> 5: the set does not depend on how the work is split.
 *   TARGETS  the centre lines of the minimap's markings: 17 axis-aligned segments, the centre circle and the two penalty arcs (beyond the penalty area's
 *            front line), positions and the radius rounded once to Q; the marks are no targets.
 *   MAP      sb = (h6 ((w - 1) / 2) + h7 (h - 1)) + h8; NO MAP when valid is 0, an h_i or sb is not finite, or sb == 0; G = H when sb > 0, else -H.
 *   ROUND    every line pixel is mapped with the frame's current matrix (float64, single operations, w' > 0, |X|, |Y| <= 1024, then floor(X 1024 + 0.5)),
 *            matched to the candidate primitive of least e^2 (segments: the signed distance along the normal, only inside the span; arcs:
 *            floor((|P - c|^2 - R^2 + R) / (2 R)); ties to the earlier primitive) and is an inlier iff e^2 <= rq^2, rq falling from `radius` by
 *            `radius_factor` per round to `radius_min`.  Its row is the gradient (1 / 128) times the derivative of the correction
 *            dx = a0 + a1 x + a2 y - (a6 x + a7 y) x, dy = a3 + a4 x + a5 y - (a6 x + a7 y) y about the centre spot (x, y in 1 / 512 of 64 m), all
 *            integers below 2^17; the normal matrix, the right-hand side, the inlier count, the sum of e^2 and the inliers per primitive are exact
 *            64-bit integer sums, which cannot overflow for a frame of at most 2^28 pixels.  The ladder projective (8) -> affine (6) -> translation
 *            (2) -> none is decided from the number of primitives of each orientation that hold min_per_line inliers, a pivot test (1e-9 of the largest
 *            diagonal entry) and the cap max_step on every |64 a_i|; Gaussian elimination in float64 with partial pivoting; the new matrix is
 *            T (D (T^-1 M)).
 *   DECIDE   the refined matrix is ACCEPTED iff a round changed it, it has min_points inliers at radius_min, its mean e^2 there is below the
 *            original's, and none of nine image points (corners, edge centres, centre) that the original maps to within 10 m of the pitch moved by
 *            more than max_shift.  Otherwise the frame keeps its nine doubles bit for bit and the status says why.  Frames are independent.
 * The constants are conventional choices, not fitted to data, and nothing is validated on real footage.  Limits: straight centre lines and three arcs
 * only; no lens distortion; a line pixel is a colour-and-contrast rule, so white boots outside a box and advertising on grass-coloured ground are
 * candidates until the radius shuts them out; a view with fewer than two line directions can only be shifted; a wrong but self-consistent match (the
 * goal-area line taken for the penalty-area line) is possible and bounded only by radius and max_shift.  Launches (linefit.hip) on the handle's main
 * stream, chained without host synchronisation between the rounds; device memory is allocated per call and freed; records, staging buffers and graphs
 * of the handle are not involved.  EAGLE_E_INVALID with a message, before any launch: NULL pointers (parameters, Hs_out, frames_out; frames, Hs, valid
 * with n > 0), k outside 1 .. 64, tau outside 1 .. 1020, rounds outside 0 .. 16, model outside 1 .. 3, min_points or min_per_line < 1, box_pad negative
 * or not finite, not 0 < radius_min <= radius <= 8 (radius_min at least 1 / 2048 m), radius_factor outside (0, 1], max_shift outside 0 .. 1024, max_step
 * outside (0, 64], non-zero reserved words, box offsets not ascending from 0 or more than EAGLE_MAX_DET boxes in a frame (an n_det outside that range),
 * a negative max_staging_bytes, n < 0; in the operator entry a frame side outside 1 .. 16384.  n == 0 succeeds and writes
 * nothing.  masks_out may be NULL. */
#define EAGLE_LINEFIT_NO_MAP 0         /* EagleLineFitFrame::status */
#define EAGLE_LINEFIT_ACCEPTED 1
#define EAGLE_LINEFIT_UNCHANGED 2      /* no round could move the matrix (or rounds == 0) */
#define EAGLE_LINEFIT_FEW_POINTS 3
#define EAGLE_LINEFIT_NO_GAIN 4
#define EAGLE_LINEFIT_SHIFT 5
#define EAGLE_LINEFIT_NONE 0           /* EagleLineFitFrame::model, EagleLineFitParams::model (1 .. 3) */
#define EAGLE_LINEFIT_TRANSLATION 1
#define EAGLE_LINEFIT_AFFINE 2
#define EAGLE_LINEFIT_PROJECTIVE 3
#define EAGLE_LINEFIT_FALL_LINES 0     /* EagleLineFitFrame::fall: bit 3 (rung - 1) + cause */
#define EAGLE_LINEFIT_FALL_PIVOT 1
#define EAGLE_LINEFIT_FALL_CAP 2
typedef struct EagleLineFitParams {
    int32_t k, tau;                /* the line-pixel rule (conventionally 4 and 200, i.e. 50 grey levels) */
    int32_t rounds;                /* conventionally 5 */
    int32_t model;                 /* the ladder's top rung (conventionally EAGLE_LINEFIT_PROJECTIVE) */
    int32_t min_points;            /* inliers at radius_min a refined matrix needs (conventionally 200) */
    int32_t min_per_line;          /* inliers that make a primitive count for the ladder (conventionally 20) */
    double box_pad;                /* pixels (conventionally 3) */
    double radius, radius_min;     /* metres (conventionally 2.5 and 0.5) */
    double radius_factor;          /* per round (conventionally 0.6) */
    double max_shift;              /* metres (conventionally 3) */
    double max_step;               /* metres at 64 m from the centre spot, per unknown and round (conventionally 4) */
    int32_t reserved[4];           /* 0 */
} EagleLineFitParams;              /* 88 bytes */
typedef struct EagleLineFitFrame {
    int32_t status;                /* EAGLE_LINEFIT_NO_MAP .. _SHIFT */
    int32_t model;                 /* the last round's rung */
    int32_t rounds;
    int32_t n_line;                /* line pixels of the frame */
    int32_t n_before, n_after;     /* inliers at radius_min under the original and under the last matrix */
    int32_t fall;                  /* every rung that fell in any round, and why */
    int32_t reserved;
    int64_t e2_before, e2_after;   /* their sums of e^2 (Q^2) */
    int64_t shift2;                /* the largest squared shift of the nine image points (Q^2); -1: a point left the map */
} EagleLineFitFrame;               /* 56 bytes */
int eagle_linefit_params_default(EagleLineFitParams* p);
/* n frames of the handle's size, dense, resident in HBM.  Hs, valid, recs (NULL: no boxes; else the detections of each record are the boxes) are host
 * memory; Hs_out [n][9], frames_out [n] and masks_out (NULL or u32 [n][h][(w + 31) / 32]) are host memory; returns when they are complete. */
int eagle_linefit_device_frames(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                const EagleLineFitParams* p, double* Hs_out, EagleLineFitFrame* frames_out, uint32_t* masks_out);
/* Same for a clip in host memory, uploaded in passes of what max_staging_bytes (0: 64 MB; always at least one frame) of device staging hold.  The
 * result does not depend on the size of a pass. */
int eagle_linefit_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t max_staging_bytes, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                         const EagleLineFitParams* p, double* Hs_out, EagleLineFitFrame* frames_out, uint32_t* masks_out);
/* Operator entry (host buffers in / out, no handle): dense frames of any h x w within 1 .. 16384 per side.  boxes [box_off[n]][4] =
 * x1, y1, x2, y2 and box_off [n + 1] stand for the records; both NULL: no boxes. */
int eagle_op_linefit(int device, const uint8_t* bgr, int n, int h, int w, const double* Hs, const uint8_t* valid, const float* boxes, const int32_t* box_off,
                     const EagleLineFitParams* p, double* Hs_out, EagleLineFitFrame* frames_out, uint32_t* masks_out);

/* ---- occupancy heat maps: where a player, a team and the ball spent their time (own specification: tests/occupancy_ref.py defines every output bit) ----
 * A call computes n_sel maps.  Selection s is the list sel_cols[sel_off[s] .. sel_off[s + 1] - 1] of table column indices (sel_off[n_sel + 1] ascends from
 * 0).  Members must be pitch columns (video == 0) of kind Player, Goalkeeper or Ball; a column may appear in several selections, not twice in one; an
 * empty selection gives zeros.
 *   WEIGHT   w[r] = frames[r + 1] - frames[r] when r + 1 < rows and that step is <= max_gap, else 1 (the last row, the row in front of a hole).
 *   COUNTS   cells_per_metre R in {1, 2, 4}, gw = 105 R, gh = 68 R, grid row 0 is pitch y = 0 (eagle_control_size's geometry).  A cell of the table is
 *            present when x and y are finite.  A present cell with 0 <= x < 105 and 0 <= y < 68 (float64) adds w[r] to count[s][(int) floor(y R)][(int)
 *            floor(x R)], any other present cell adds it to outside[s], an absent cell adds nothing; total[s] = what went inside.  -0.0 is inside, 105.0
 *            and 68.0 are outside.  Integers: no accumulation order matters.  The library accumulates in 32 bits and refuses a call in which
 *            rows x max_gap x (the largest selection) reaches 2^31.
 *   GRIDS    float32 without contraction: s = (float) sigma * (float) R, rad = (int) ceilf(3.0f * s), inv = 1.0f / (2.0f * s * s), t[0] = 1.0f,
 *            t[k] = d_expf(-((float) (k * k)) * inv) (csrc/dmath.h); sigma == 0: rad = 0.  hz[j][i] = the sum over k = -rad .. rad, ascending, from
 *            0.0f, of t[|k|] * (float) count[j][i + k], terms outside the grid skipped, multiply and add rounded separately; v[j][i] = the same sum
 *            over hz[j + k][i].  Truncated at 3 sigma, zero outside the grid, not renormalised at the borders.  The unit is frames; seconds = v / fps.
 *   BYTES    m = the largest v of the selection; byte = m > 0 ? (int) floorf(v / m * 255.0f + 0.5f) : 0.
 *   PICTURE  a BGR canvas of eagle_minimap_size's size for (scale, margin), black; a pixel (X, Y) of the pitch rectangle reads the byte c of cell
 *            i = ((X - margin) R) / scale, j = gh - 1 - ((Y - margin) R) / scale and takes per channel (colour * a + 128) >> 8 with a = c + (c >> 7);
 *            the minimap's pitch markings on top in white; no players, no ball, no footprint.  bgr_colour = B | G << 8 | R << 16.
 * Five launches (occupancy.hip) on the handle's main stream read the table where eagle_postprocess left it; the handle's records, staging buffers and
 * graphs are not involved.  sigma 2 m is a conventional choice, not fitted to data.  The maps follow a person only when the ids do (merge_ids).
 * EAGLE_E_INVALID with a message, before any launch: NULL pointers, fps or max_gap not positive, cells_per_metre outside {1, 2, 4}, sigma not finite or
 * outside [0, 10], n_sel < 0, offsets that do not ascend from 0, a member that is out of range, a video column, a boundary column or listed twice in its
 * selection, the 2^31 bound, frames of the operator entry that do not ascend strictly, a result beyond the table's memory budget
 * (EaglePostParams::max_bytes; the operator entry: nine tenths of what is free), a bad scale or margin of the picture (the minimap's rules), a sel
 * outside the last result.  rows == 0 gives zeros; n_sel == 0 writes nothing. */
typedef struct EagleOccupancyParams {
    int32_t fps;                   /* > 0: frames per second of the frame numbers (the host divides by it; the kernels count frames) */
    int32_t max_gap;               /* > 0: a row in front of a step of more frames than this counts one frame (a usual choice: fps) */
    int32_t cells_per_metre;       /* 1, 2 or 4 */
    int32_t reserved0;
    double sigma;                  /* metres: 0 .. 10; 0 = no smoothing */
    int64_t reserved;
} EagleOccupancyParams;
int eagle_occupancy_size(const EagleOccupancyParams* p, int* gw, int* gh);                                   /* = eagle_control_size's */
/* The result is kept with the table until eagle_post_free and replaces an earlier one. */
int eagle_post_occupancy(EagleHandle* h, EaglePostTable* t, const EagleOccupancyParams* p, const int32_t* sel_off, const int32_t* sel_cols, int n_sel);
/* copies to the host: grids, bytes and counts [n_sel][gh][gw], total and outside [n_sel]; any pointer may be NULL */
int eagle_post_occupancy_values(EaglePostTable* t, float* grids, uint8_t* bytes, int64_t* total, int64_t* outside, int32_t* counts);
int eagle_post_device_occupancy(const EaglePostTable* t, const float** d_grids, const uint8_t** d_bytes);    /* in HBM; both NULL before eagle_post_occupancy */
/* selection sel of the last result as a picture; out: host memory, [h][w][3] */
int eagle_occupancy_picture(EagleHandle* h, EaglePostTable* t, int sel, int scale, int margin, uint32_t bgr_colour, uint8_t* out);
/* Operator entries (host buffers in / out, no handle) for constructed tables: values [cols][rows][2], frames [rows] strictly ascending, columns as
 * eagle_post_layout gives them; every output may be NULL.  The picture entry takes one selection's bytes [gh][gw]. */
int eagle_op_occupancy(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const EagleOccupancyParams* p,
                       const int32_t* sel_off, const int32_t* sel_cols, int n_sel, float* grids, uint8_t* bytes, int64_t* total, int64_t* outside, int32_t* counts);
int eagle_op_occupancy_picture(int device, const uint8_t* bytes_grid, int cells_per_metre, int scale, int margin, uint32_t bgr_colour, uint8_t* out);

/* Reference cadence with homography_interval > 1 (main.py:27 at --fps 5; cm.py:333-415): the caller decides, frame by frame in
 * clip order, which frame's homography each frame uses (scheduled / retry / carried) and hands the records back:
 * flags[i] = 0 keep the record, 1 re-project foot points and boundaries with Hs[9*i..], 2 no homography available yet. */
int eagle_reproject(EagleHandle* h, EagleFrameResult* recs, int n, const double* Hs, const uint8_t* flags);

/* ---- optical-flow key-point cadence: get_coordinates with keypoint_interval > 1, cm.py:188-416 ----------
 * The reference detects key-points with HRNet only every keypoint_interval-th frame and propagates them with
 * cv2.calcOpticalFlowPyrLK in between (cm.py:313-322, 419-478); that makes the loop sequential over a clip.  A clip session
 * keeps the clip, its gray pyramids, every frame's detections and the loop-carried state in HBM:
 *   eagle_clip_open             gray pyramids of all frames                                                      (cm.py:280)
 *   eagle_clip_detect_objects   detector / NMS / object rules on frames [first, first+count), asynchronous      (cm.py:331)
 *   eagle_clip_detect_keypoints HRNet + decode on frames first, first+stride, ... -> their mem[] entries, asynchronous (cm.py:217-276, 285, 317)
 *   eagle_clip_get/set_keypoints read / replace mem[frame]  (the first-frame search of cm.py:289-311 is sequenced by the caller)
 *   eagle_clip_flow             calculate_optical_flow(frames[hue_frame], gray[src], kps, gray[dst]) as an operator (cm.py:419-478)
 *   eagle_clip_run              the loop body for frames [first, last), in order, on the GPU without host round trips, on its own
 *                               stream behind every pass enqueued so far (so the passes of later frames overlap it); it stops itself
 *                               at a frame that needs a model detection it does not have.  wait = 1: block and report that frame
 *                               (*stalled_at, else -1); first > 0 continues with the loop state of the previous call, and with wait = 1 it
 *                               is the resume after an on-demand detection (clears the stall mark first)
 *   eagle_clip_fetch            the n records.  EagleFrameResult.pad[0] = 1 when the frame solved its own homography
 *                               ("Keypoints" = its inliers, cm.py:359-362); kp[].pad bit 0: the value came from the flow, bit 1: moved by the calibration
 *                               (both are numpy integers in the reference's dict, which json.dump(default=float) writes as floats). */
typedef struct EagleFlowKp { int32_t label; int32_t x, y; float score; } EagleFlowKp;
int eagle_clip_open(EagleHandle* h, const void* d_bgr, int n);
int eagle_clip_detect_objects(EagleHandle* h, int first, int count);
int eagle_clip_detect_keypoints(EagleHandle* h, int first, int stride, int count);
int eagle_clip_get_keypoints(EagleHandle* h, int frame, EagleFlowKp* out /* EAGLE_N_LANDMARKS */, int* n /* -1: no entry */);
int eagle_clip_set_keypoints(EagleHandle* h, int frame, const EagleFlowKp* in, int n);
int eagle_clip_flow(EagleHandle* h, int src_frame, int dst_frame, int hue_frame, const EagleFlowKp* in, int n_in,
                    EagleFlowKp* out /* EAGLE_N_LANDMARKS */, int* n_out, float* next_pts /* 2*n_in or NULL */, uint8_t* status /* n_in or NULL */);
int eagle_clip_run(EagleHandle* h, int first, int last, int keypoint_interval, int homography_interval, int calibration, int wait,
                   int* stalled_at);
int eagle_clip_fetch(EagleHandle* h, EagleFrameResult* out);
int eagle_clip_close(EagleHandle* h);
#define EAGLE_E_REFERENCE_RAISES (-7) /* the reference raises IndexError here (calibration grid at the image border, cm.py:545) */

/* ---- track identities: self.tracker.update(dets, frame) of cm.py:66-72, 574-596 -----------------------------------
 * BoT-SORT's motion / IoU association (constant-velocity Kalman filter, high / low confidence sets, three assignments, life cycle);
 * appearance and camera-motion compensation are separate entry points below (eagle_reid_features, eagle_clip_motion_ecc / eagle_clip_motion).  eagle_track_frames walks n records of ONE
 * clip in frame order (call it chunk after chunk; eagle_track_open starts a new clip): Player / Goalkeeper entries become keyed by
 * track id with the filter's boxes and feet (cm.py:577-596; frames on which the tracker reports no player keep the detection-index
 * fallback of cm.py:598-616), then the pitch coordinates of the moved foot points are recomputed on the GPU with each record's H. */
typedef struct EagleCrop { int32_t frame, x1, y1, x2, y2; } EagleCrop;      /* frame[y1:y2, x1:x2] of a clip resident in HBM */
typedef struct EagleTrackParams {
    float track_high_thresh, track_low_thresh, new_track_thresh, match_thresh;   /* 0.5, 0.1, 0.6, 0.8 (boxmot defaults) */
    int32_t track_buffer, frame_rate;                                             /* 30, 30 */
} EagleTrackParams;
int eagle_track_open(EagleHandle* h, const EagleTrackParams* params /* NULL: defaults */);
int eagle_track_frames(EagleHandle* h, EagleFrameResult* recs, int n);
/* Camera-motion compensation (BoT-SORT's gmc step; boxmot's default estimates the warp with ECC, here: a similarity transform from an 8 x 6 grid
 * of points tracked by the key-point cadence's pyramidal LK kernel, RANSAC over point pairs + least squares on the consensus set — stated deviation).
 * eagle_clip_motion: needs an open clip session (eagle_clip_open); warps[6 * i .. +5] = row-major 2 x 3 warp of frame first+i-1 -> first+i
 * (identity for clip frame 0).  eagle_track_frames_cmc: as eagle_track_frames, applying warps[6 * i] to all track states before frame i is associated. */
int eagle_clip_motion(EagleHandle* h, int first, int count, double* warps);
/* boxmot's default estimator (cmc_method "ecc", what the reference's BotSort(...) of cm.py:66-72 runs on the frame passed at cm.py:577):
 * gray -> cv2.resize(fx = fy = 0.15) -> cv2.findTransformECC(prev, cur, MOTION_EUCLIDEAN, 100 iterations / 1e-5), translation rescaled by 1 / 0.15;
 * a failed alignment (cv2 raises: lambda_d <= 0 or NaN correlation) yields the identity and keeps the OLD template, as boxmot does.  Same warps
 * layout as eagle_clip_motion; ok[i] (may be NULL) = 0 where the alignment of frame first+i failed.  carry != 0: the estimator's template
 * survives the clip like boxmot's ECC object survives inside the tracker — clip frame 0 is aligned to the last template of the previous call
 * (eagle_track_open forgets it).  Restated from the published algorithm (oracle/ecc.py); cv2 / boxmot absent: parity unpinned. */
int eagle_clip_motion_ecc(EagleHandle* h, int first, int count, int carry, double* warps, int* ok);
int eagle_track_frames_cmc(EagleHandle* h, EagleFrameResult* recs, int n, const double* warps /* NULL: none */);
/* Appearance (BoT-SORT with_reid, the reference's configuration: cm.py:66-72 builds BotSort with osnet_x0_25 ReID weights and passes the frame at
 * cm.py:577).  eagle_reid_features: OSNet-x0.25 embeddings (EAGLE_REID_DIM floats each) of crops frame[y1:y2, x1:x2] of a clip resident in HBM,
 * prepared as boxmot does (resize to 128 x 256, RGB, ImageNet normalisation); needs the "reid.*" tensors (torchreid's parameter names) loaded
 * before eagle_finalize_weights, EAGLE_E_STATE otherwise.  eagle_track_frames_reid: as eagle_track_frames_cmc with the embeddings of each
 * record's high-confidence detections: record i owns feat_count[i] consecutive rows of `feats`, feat_det lists their detection indices.  The
 * association then is BoT-SORT's: cost = min(IoU distance, embedding distance / 2) with embedding distances above appearance_thresh 0.25 or IoU
 * distances above proximity_thresh 0.5 set to 1; track features are exponential moving averages (alpha 0.9) of the normalised embeddings.
 * Contract: `feats` holds sum(feat_count) rows of EAGLE_REID_DIM floats and `feat_det` as many entries; 0 <= feat_count[i] <= EAGLE_MAX_DET and
 * 0 <= feat_det[.] < recs[i].n_det are checked (EAGLE_E_INVALID) before anything is read. */
#define EAGLE_REID_DIM 512
int eagle_reid_features(EagleHandle* h, const void* d_bgr, int n_frames, const EagleCrop* crops, int n_crops, float* feats);
int eagle_track_frames_reid(EagleHandle* h, EagleFrameResult* recs, int n, const double* warps /* NULL: none */, const float* feats,
                            const int32_t* feat_det, const int32_t* feat_count);

/* ---- team colours: Processor.detect_color, eagle/processor.py:466-503, for player crops of a clip resident in HBM -----
 * counts[12 * i + k]: pixels of crop i's player cluster inside colour range k of proc.py:10-23, k = red (red2 merged), orange, yellow,
 * green, cyan, blue, purple, magenta, white, gray, black; slot 11 = pixels of the player cluster.  Crops are frame[y1:y2, x1:x2]; a crop that is
 * empty or leaves the clip gives twelve zeros.  The 2-means equals scikit-learn's KMeans(n_clusters=2, random_state=0) for crops with no exact
 * distance tie on the Lloyd path.  On a tie (a pixel exactly equidistant from both centres) the library assigns to cluster 0; scikit-learn's
 * result there depends on the rounding of its centred data and is not reproduced (of 400 seeded few-level crops, 117 tie and 16 of those differ). */
int eagle_team_colors(EagleHandle* h, const void* d_bgr, int n_frames, const EagleCrop* crops, int n_crops, int32_t* counts);

/* ---- team clustering: the two teams as the two clusters of the ids' kit colours over the clip (own specification: tests/kits_ref.py defines every
 * output bit) ----
 * eagle_team_colors above feeds the reference's rule: named colour ranges and the two most common names, which cannot separate two kits inside one
 * named range (navy and sky blue are both "blue").  This stage is the library's own, opt-in answer.  Crop i belongs to the id of slot slots[i]
 * (0 .. n_ids - 1).  With w = x2 - x1, h = y2 - y1 its shirt window is rows [y1 + h/5, y1 + h/2) and columns [x1 + w/4, x2 - w/4) (integer
 * divisions).  A pixel with g >= 48 and g - max(r, b) >= 16 is grass and does not count; every other pixel gets cv2's 8-bit HSV; with s >= 64 and
 * v >= 48 it puts 12 units into the two nearest of 15 circular hue bins of width 12 (t = (h + 174) % 180: 12 - t % 12 units to bin t / 12, t % 12
 * units to the next), in the lower 15 bins for v < 144, in the upper 15 otherwise; any other pixel puts 12 units into bin 30 + v / 64.  A crop of n
 * counted pixels gives q[b] = units[b] * 4096 / (12 n); per id sum[b] adds the q[b] of its used crops and p[b] = sum[b] * 65536 / T with T the sum of
 * sum[b].  D(i, j) = sum_b |p_i[b] - p_j[b]|.  The voters are the ids with at least min_crops used crops, of weight w_i = used.  For every pair of
 * voters a < b, cost(a, b) = sum over the voters of w_i min(D(i, a), D(i, b)); the least cost wins, ties go to the earlier pair.  Every id with a used
 * crop goes to the nearer medoid (equal distances: a); it is "neither" (team -1) when outlier > 0 and d_near * 1024 > outlier * D(a, b).  Team 0 is
 * the cluster with the larger sum of w over its voters that are not neither (a tie: the cluster of a).  With fewer than two voters every id with
 * crops is team 0.  Integers throughout: the result does not depend on any order of accumulation, and two runs give identical bytes.  The constants
 * are conventional choices, not fitted to data. */
#define EAGLE_KIT_BINS 34
#define EAGLE_KIT_MAX_IDS 1024
#define EAGLE_KIT_CROP_OUTSIDE 1   /* the crop leaves the frame or names a frame outside the clip: zeros */
#define EAGLE_KIT_CROP_EMPTY 2     /* the crop or its shirt window is empty: zeros */
#define EAGLE_KIT_CROP_FEW 4       /* fewer than min_pixels counted pixels: units and n are reported, the crop is not used */
#define EAGLE_KIT_ID_WEAK 1        /* fewer than min_crops used crops: assigned, but no voter */
#define EAGLE_KIT_ID_NEITHER 2     /* farther from the nearer medoid than outlier / 1024 of the distance between the medoids: team -1 */
#define EAGLE_KIT_ID_SINGLE 4      /* fewer than two voters: team 0 */
#define EAGLE_KIT_MODEL_SINGLE 1
#define EAGLE_KIT_MODEL_SWAPPED 2  /* team 0 is the cluster of b */
typedef struct {
    int32_t min_pixels;            /* 1 .. 2^20: the least counted pixels of a used crop (default 32) */
    int32_t min_crops;             /* 1 .. 2^16: the least used crops of a voter (default 3) */
    int32_t outlier;               /* 0 .. 2^20, in 1/1024 of D(a, b); 0: nobody is neither (default 512, half the distance between the medoids) */
    int32_t reserved[5];           /* 0 */
} EagleKitParams;                  /* 32 bytes */
typedef struct {
    uint32_t units[EAGLE_KIT_BINS];
    int32_t n, flags;              /* counted pixels; EAGLE_KIT_CROP_* */
} EagleKitCrop;                    /* 144 bytes */
typedef struct {
    int32_t used, skipped;         /* crops of the id that count / that were skipped */
    int32_t team;                  /* 0, 1, or -1: no used crop, or neither */
    int32_t flags;                 /* EAGLE_KIT_ID_* */
    uint32_t d[2];                 /* D to the medoid of team 0 and of team 1 (0 without medoids) */
    uint32_t p[EAGLE_KIT_BINS];    /* the signature (0 without a used crop) */
} EagleKitId;                      /* 160 bytes */
typedef struct {
    int32_t a, b;                  /* the medoids' slots, a < b; -1 with fewer than two voters */
    uint32_t dab;                  /* D(a, b) */
    int32_t voters;
    int64_t cost;                  /* cost(a, b) */
    int64_t w[2];                  /* sum of w over the voters of team 0 and of team 1 that are not neither */
    int32_t neither;               /* ids that are neither */
    int32_t flags;                 /* EAGLE_KIT_MODEL_* */
    int32_t team_of_a;             /* 0 or 1 */
    int32_t reserved[3];
} EagleKitModel;                   /* 64 bytes */
int eagle_kit_params_default(EagleKitParams* p);
/* On a clip of n_frames BGR frames of the handle's size resident at d_bgr (as eagle_team_colors).  Each output may be NULL: crops_out [n_crops],
 * ids_out [n_ids], model_out [1].  EAGLE_E_INVALID, with a message naming the count and the limit and before anything is read or written: more than
 * 1024 ids, more than 2^22 crops, a slot outside 0 .. n_ids - 1, a parameter outside its range.  n_ids == 0 writes the model of no voters only. */
int eagle_team_cluster(EagleHandle* h, const void* d_bgr, int n_frames, const EagleCrop* crops, const int32_t* slots, int n_crops, int n_ids, const EagleKitParams* p,
                       EagleKitCrop* crops_out, EagleKitId* ids_out, EagleKitModel* model_out);
/* Operator entries (host buffers in / out, no handle: parity tests and tools).  The same from n host frames [n, h, w, 3]; times_ms NULL or two device
 * times in milliseconds, from events recorded directly around kit_hist_kernel's launch (0 without crops) and around the four clustering launches;
 * allocations and copies lie outside both. */
int eagle_op_team_cluster(int device, const uint8_t* bgr, int n, int h, int w, const EagleCrop* crops, const int32_t* slots, int n_crops, int n_ids, const EagleKitParams* p,
                          EagleKitCrop* crops_out, EagleKitId* ids_out, EagleKitModel* model_out, float* times_ms);
/* The clustering alone from given sums [n_ids][34] (each 0 .. 2^34) and used [n_ids] (0 .. 2^22 each and in all; an id with used > 0 needs a sum above 0): ties and
 * degenerate distances that pixels cannot reach.  "skipped" of the records is 0. */
int eagle_op_team_cluster_ids(int device, const int64_t* sums, const int32_t* used, int n_ids, const EagleKitParams* p, EagleKitId* ids_out, EagleKitModel* model_out,
                              float* times_ms);

/* Frame-sharded multi-GPU: rank r owns a contiguous chunk; one RCCL all-gather of records.
 * eagle_comm_id fills a 128-byte ncclUniqueId on rank 0; the caller broadcasts it (any channel). */
int eagle_comm_id(void* id128);
int eagle_comm_init(EagleHandle* h, int rank, int world, const void* id128);
int eagle_gather(EagleHandle* h, const EagleFrameResult* local, int n_local, EagleFrameResult* all /* world*n_local */);

/* Timing of the last eagle_process_* call, measured with HIP events on the library's compute stream. */
typedef struct EagleTimings {
    float total_ms;            /* first kernel -> records copied */
    float conv_ms;             /* sum over convolution launches (only when profiling is enabled) */
    int32_t n_launches;
    int32_t n_conv_launches;
    double conv_flop;          /* algorithmic FLOP of the convolutions of the last call (2*MAC) */
    int32_t sat_events;        /* EAGLE_PREC_F32S: lane-level activation stores of the last eagle_process_* / eagle_clip_fetch call that were clipped at +-4094 */
    int32_t sat_frames;        /* ... and the number of frames they occurred in (0 / 0 in every healthy run) */
    int32_t graph_captures;    /* hipGraph captures this handle has made since eagle_create (cumulative: one per pipeline slot and frame count, ~80 ms each; a caller that
                                  sees this number grow call after call is paying for re-captures) */
    int32_t graph_skipped;     /* ... and capture attempts given up because another call of the process held the capture lock (the step then ran as plain launches) */
    int32_t reserved[4];
} EagleTimings;
int eagle_set_profiling(EagleHandle* h, int per_kernel_events);
int eagle_get_timings(EagleHandle* h, EagleTimings* t);
/* Profiling mode also times every non-convolution launch (HIP events on its launch stream) and accumulates, per kernel name, the
 * elapsed time and the ALGORITHMIC HBM bytes of the launches (inputs read once + outputs written once): the HBM-roofline
 * rows of bench.py.  The table is cleared by eagle_set_profiling(h, 1). */
typedef struct EagleKernelTime { char name[40]; float ms; int32_t launches; double bytes; double flop; } EagleKernelTime;   /* convolutions: one row per layer shape, flop = 2*MAC */
int eagle_get_kernel_times(EagleHandle* h, EagleKernelTime* out, int cap, int* n);

/* Operator-level entry points (host buffers in/out) used by the parity tests: each runs ONE kernel of the path.
 * Tensors are dense NHWC fp32 on the host; `precision` selects the fp16 or fp32 kernel family. */
int eagle_op_conv2d(int device, int precision, const float* x, int n, int h, int w, int cin, const float* w_hwio,
                    const float* bias, int cout, int ks, int stride, int pre_act, const float* r1, const float* r2,
                    int post_act, float* y);
/* One fused Bottleneck of HRNet's layer 1 in the split family (bneck.hip; kh.py:101-137): y = relu(conv3(relu(conv2(relu(conv1(x))))) + res), conv1 1x1 Cin->64,
 * conv2 3x3 64->64, conv3 1x1 64->256, BatchNorm already folded into (w, b); weights HWIO ([1][1][Cin][64], [3][3][64][64], [1][1][64][256]); res = NULL: the
 * identity shortcut (Cin = 256).  reps > 0: *ms = average duration of `reps` further launches (HIP events). */
int eagle_op_bottleneck(int device, const float* x, int n, int h, int w, int cin, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, const float* res, float* y, int reps, float* ms,
                        const float* wd /* NULL, or the 1x1 downsample branch [1][1][64][256] computed inside the launch (Cin = 64, res = NULL) */, const float* bd);
/* The fused input path of HRNet in the split family (stem.hip): y = relu(conv1 3x3/2 3->64 (normalise(resize(bgr, dh x dw)))), BatchNorm already folded into
 * (w1 HWIO [3][3][3][64], b1); bgr: n dense u8 frames [h][w][3]; y: [n][(dh-1)/2+1][(dw-1)/2+1][64]; sat (or NULL): per frame, the lanes that stored a value
 * beyond the split format's range (what EagleFrameResult's saturation flag is made of). */
int eagle_op_stem(int device, const uint8_t* bgr, int n, int h, int w, int dh, int dw, const float* w1, const float* b1, float* y, uint32_t* sat);
int eagle_op_fuse_sum(int device, int precision, const float* base, int n, int H, int W, int c, int n_up,
                      const float* const* ups, const int* up_h, const int* up_w, int relu, float* y);
int eagle_op_preprocess(int device, int precision, const uint8_t* bgr, int n, int h, int w, int det_imgsz,
                        float* kp_out /* n*540*960*3 */, float* det_out /* n*dh*dw*3 */, int* det_hw /* 2 */);
int eagle_op_preprocess_lb(int device, int precision, const uint8_t* bgr, int n, int h, int w, int det_imgsz, int letterbox /* EAGLE_LETTERBOX_* */,
                           float* kp_out, float* det_out, int* det_hw);
int eagle_op_find_homography(int device, const float* img_pts, const float* world_pts, int n, double thresh,
                             int max_iters, int lm_iters, double* H9, uint8_t* mask, int* ok);

/* ---- the tail behind the two networks, on chosen inputs (tests/test_gpu_tail.py).  Test surface only: the launches are the data path's own. ----
 * One heat-map partial: the first maximum of sigmoid(logit) of one channel over one pixel range or output tile (score -1, idx 0x7fffffff: empty range). */
typedef struct EagleArgmaxPart { float score; int32_t idx; } EagleArgmaxPart;
/* Detect tail: DFL decode + class sigmoid + confidence floor (yolo_decode_kernel), then sort, class-offset NMS, the 300-box cap, scale_boxes and the
 * detection -> object rules (nms_kernel).  n_lv (1..3) pyramid levels of gh[l] x gw[l] cells and stride[l]; box[l]: fp32 logits [n][gh][gw][64], cls[l]:
 * [n][gh][gw][nc] (nc <= 16); anchors are numbered level by level, row-major.  out: n records, of which n_det, n_candidates and det[0..n_det) are written.
 * boxes [n][A][4] / conf [n][A] / cls_out [n][A] (each may be NULL): what the decode left for every anchor.  More anchors than the NMS workgroup sorts: EAGLE_E_INVALID. */
int eagle_op_detect_tail(int device, int n_lv, const int* gh, const int* gw, const float* stride, const float* const* box, const float* const* cls, int n, int nc,
                         float conf_floor, float nms_iou, double detector_conf, int frame_h, int frame_w, int in_h, int in_w,
                         EagleFrameResult* out, float* boxes, float* conf, int32_t* cls_out);
/* Key-point tail (post_kernel): reduction of the heat-map partials, decode / threshold / dedup, synthesis, homography, bounds and the projection of the foot
 * points.  Either logits (fp32 [n][hm_h][hm_w][64]: heat_argmax_kernel makes `chunks` partials per channel first) or parts ([n][chunks][64], e.g. those of
 * eagle_op_conv2d_argmax with 64 padded channels) is given, the other NULL.  recs: n records, read (n_det and det[k].foot_x / foot_y) and completed in place.
 * parts_out (or NULL): the partials that were reduced, [n][chunks][64]. */
int eagle_op_post(int device, int n, int hm_h, int hm_w, int chunks, const float* logits, const EagleArgmaxPart* parts, EagleArgmaxPart* parts_out,
                  EagleFrameResult* recs, int frame_h, int frame_w, double keypoint_conf, double ransac_thresh, int ransac_max_iters, int lm_iters);
/* The head convolution with its fused arg-max epilogue: ONE ConvLaunch (families EAGLE_PREC_F16 and EAGLE_PREC_F32S, cout <= 64, the configuration the network
 * builder picks for an fp32-output layer) run twice, once storing the fp32 logits [n][ho][wo][cout], once reducing sigmoid(logit) per output tile into
 * parts [n][tiles][cout rounded up to 16].  tiles / tile_h / tile_w: partials per frame and channel and the tile rectangle (tiles are numbered row-major,
 * ceil(wo / tile_w) per row).  logits == NULL: only tiles / tile_h / tile_w are written (no GPU work). */
int eagle_op_conv2d_argmax(int device, int precision, const float* x, int n, int h, int w, int cin, const float* w_hwio, const float* bias, int cout, int ks, int stride,
                           float* logits, EagleArgmaxPart* parts, int* tiles, int* tile_h, int* tile_w);

/* ---- which convolution form a call runs, and the tables the choice is made from (tests/test_conv_forms_cpu.py, tests/test_gpu_conv_forms.py).  Test surface
 * only, host only: no GPU is touched.
 * eagle_op_conv_config: the configuration eagle_op_conv2d (and the network builder) runs for a layer of REAL channel counts cin / cout on an output map wo
 * columns wide, after the entry's own channel padding, with EAGLE_CONV_FORCE / EAGLE_F32_FORCE read as on every call.  plain_epilogue: no activation before
 * the residual adds, none / ReLU after them, 2-byte / split output; second_residual: two residual operands.
 * out = {kc, nt, wx, variant, tile_h, tile_w, lds_bytes, supported}; supported = 1: the instance exists and its LDS fits the 160 KiB a workgroup can have. */
int eagle_op_conv_config(int precision, int ks, int stride, int cin, int cout, int wo, int plain_epilogue, int second_residual, int32_t out[8]);
/* eagle_op_conv_table: rows of `which`, at most cap / width of them written to rows (rows == NULL: none); returns the table's row count, or a negative
 * EAGLE_E_* code.  INSTANCES: every compiled generic / weight-stationary instance, 6 ints (precision, ks, stride, kc, nt, variant).  ADIRECT: the A-direct
 * forms, 8 ints (precision, variant, stride, kc, nt, tile_h, tile_w, lds_bytes).  TUNED_*: the tuned tables verbatim, 9 ints (ks, stride, cin, cout, wo,
 * kc, nt, wx, variant), in the order the choice walks them. */
#define EAGLE_CONV_TABLE_INSTANCES 0
#define EAGLE_CONV_TABLE_ADIRECT 1
#define EAGLE_CONV_TABLE_TUNED_F16 2
#define EAGLE_CONV_TABLE_TUNED_F32 3
#define EAGLE_CONV_TABLE_TUNED_SPLIT 4
int eagle_op_conv_table(int which, int32_t* rows, int cap);

/* ---- the OSNet (ReID) kernels one launch at a time (reid.hip; tests/test_gpu_reid_ops.py).  Test surface only: each entry calls the network's own launch
 * function.  Every activation operand is a slice view: its `c` channels start at channel `off` of a buffer with `cs` floats per pixel (c, cs, off multiples
 * of 4, off + c <= cs).  Inputs are given dense ([n][h][w][c]) and placed into such a buffer by the entry; everything outside a slice holds the quiet NaN
 * EAGLE_OP_SENTINEL_BITS when the kernel starts.  Output buffers come back WHOLE ([n][ho][wo][cs], sentinel included). */
#define EAGLE_OP_SENTINEL_BITS 0x7fc5e171u
/* crop + resize to oh x ow + RGB + ImageNet normalisation of crops[i] (EagleCrop) of nf dense BGR frames; 4 floats per pixel, the 4th 0; a rejected rectangle gives zeros */
int eagle_op_reid_crop(int device, const uint8_t* bgr, int nf, int fh, int fw, const EagleCrop* crops, int n, int oh, int ow, int y_cs, int y_off, float* y);
/* 7 x 7 / 2, pad 3, 3 -> 16 channels + bias + ReLU; x [n][h][w][4] (4th channel unused), wt [7][7][3][16] (BatchNorm folded), y [n][(h-1)/2+1][(w-1)/2+1][y_cs] */
int eagle_op_reid_conv7(int device, const float* x, int n, int h, int w, int x_cs, int x_off, const float* wt, const float* b, int y_cs, int y_off, float* y);
/* MaxPool2d(3, 2, 1): y [n][(h-1)/2+1][(w-1)/2+1][y_cs];  AvgPool2d(2, 2): y [n][h/2][w/2][y_cs], h, w >= 2 */
int eagle_op_reid_maxpool3s2(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int y_cs, int y_off, float* y);
int eagle_op_reid_avgpool2(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int y_cs, int y_off, float* y);
/* depthwise 3 x 3, pad 1, + bias + ReLU; wt [9][c] (BatchNorm folded), b [c] */
int eagle_op_reid_dw3(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, const float* wt, const float* b, int y_cs, int y_off, float* y);
/* ChannelGate shared by four streams and their gated sum: streams[k] [n][h][w][c] (all in slices of the same cs / off), w1 [r][c_real], b1 [r], w2 [c_real][r],
 * b2 [c_real]; g [n][4][c] (the gates; channels >= c_real are 0), y [n][h][w][y_cs] = sum_k streams[k] * g[., k, .] */
int eagle_op_reid_gate(int device, const float* const* streams, int n, int h, int w, int c, int x_cs, int x_off, const float* w1, const float* b1,
                       const float* w2, const float* b2, int c_real, int r, int y_cs, int y_off, float* g, float* y);
/* global average -> Linear(c, dim) + bias -> ReLU; wt [dim][c] (BatchNorm1d folded), feats [n][dim] */
int eagle_op_reid_head(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, const float* wt, const float* b, int dim, float* feats);

/* ---- the detector's concat-by-slice path one launch at a time (nets.hip build_yolo / YoloBuilder::c2f; tests/test_gpu_slices.py).  Test surface only: each
 * entry calls the network's own launch function on TView::slice views.  The caller passes WHOLE buffers as fp32 host arrays [n][h][w][cs] and owns every
 * value outside the slices (the tests put a NaN there); the entry converts whole buffers to the family's storage format (fp32 / binary16 / split pairs,
 * precision = EAGLE_PREC_*), launches, and returns the whole output buffer converted back.  In binary16 and split storage a NaN comes back as a NaN, not
 * with its payload.  c, cs and off are multiples of the family's vector width (4 fp32, 8 otherwise; 16 for a convolution's channel counts) and
 * off + c <= cs; slices of one buffer that a launch reads and writes must not overlap.  A violation is EAGLE_E_INVALID and nothing is launched. */
#define EAGLE_OP_RES_OWN 0      /* the residual is a slice of a buffer of its own [n][ho][wo][cs] */
#define EAGLE_OP_RES_IN_Y 1     /* ... of the OUTPUT buffer (C2f: m.k.cv2 adds slice (1 + k) c of `cat` and writes slice (2 + k) c); the pointer is not read */
#define EAGLE_OP_RES_IN_X 2     /* ... of the INPUT buffer (stride 1 only: same map size); the pointer is not read */
/* eagle_op_conv2d on slice views: x [n][h][w][x_cs] of which channels x_off .. x_off + cin are convolved; y [n][ho][wo][y_cs] is IN/OUT (its contents are
 * uploaded first, channels y_off .. y_off + cout are written); r1 / r2: NULL with where = EAGLE_OP_RES_OWN for none, else cout channels at r_off of the
 * buffer `where` names.  The configuration is conv_choose's for the slice's channel counts, as the network builder's; EAGLE_CONV_FORCE / EAGLE_F32_FORCE apply. */
int eagle_op_conv2d_sliced(int device, int precision, const float* x, int n, int h, int w, int cin, int x_cs, int x_off, const float* w_hwio, const float* bias,
                           int cout, int ks, int stride, int pre_act, const float* r1, int r1_cs, int r1_off, int r1_where,
                           const float* r2, int r2_cs, int r2_off, int r2_where, int post_act, int y_cs, int y_off, float* y);
/* MaxPool2d(5, 1, 2) (SPPF) of c channels.  same_buffer = 0: y [n][h][w][y_cs] is in/out.  same_buffer != 0: input and output are slices of ONE buffer (y_cs
 * = x_cs): x is uploaded, slice y_off is written into it and the whole buffer comes back in y, so that SPPF's chain is three calls feeding y back as x. */
int eagle_op_maxpool5(int device, int precision, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int same_buffer, int y_cs, int y_off, float* y);
/* nearest x2 of c channels into y [n][yh][yw][y_cs] (in/out), yh in {2h - 1, 2h}, yw in {2w - 1, 2w}: y[i][j] = x[i / 2][j / 2].  same_buffer as above (yh = h, yw = w: 1 x 1 maps) */
int eagle_op_upsample2(int device, int precision, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int same_buffer, int yh, int yw, int y_cs, int y_off, float* y);
/* the mixed detector's seam: a split-format slice to an fp32 slice, exactly (hi + lo) / 16.  x is stored as split pairs, y [n][h][w][y_cs] (in/out) as fp32, bit for bit */
int eagle_op_split_to_f32(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int y_cs, int y_off, float* y);

/* The optical-flow kernels (flow.hip K11 / K12, the filter stage of geom.hip) on n dense BGR frames [h][w][3], without a handle or weights: what
 * eagle_clip_open and eagle_clip_flow run, with the same pyramid-level rule.  EAGLE_E_INVALID for h < 32, w < 32 (the limits of EagleConfig) or n < 1.
 * eagle_op_gray_pyramid: gray [n][h][w] and the two pyrDown levels [n][(h+1)/2][(w+1)/2], [n][((h+1)/2+1)/2][((w+1)/2+1)/2] of every frame (all three are always
 * computed); *levels_out = the highest level the tracker uses (cv2 maxLevel 2; a level must exceed the 15 x 15 window).
 * eagle_op_flow: calculate_optical_flow(frames[hue_frame], gray[src_frame], kps, gray[dst_frame]) as eagle_clip_flow; 0 <= n_in <= EAGLE_N_LANDMARKS. */
int eagle_op_gray_pyramid(int device, const uint8_t* bgr, int n, int h, int w, uint8_t* g0, uint8_t* g1, uint8_t* g2, int* levels_out);
int eagle_op_flow(int device, const uint8_t* bgr, int n, int h, int w, int src_frame, int dst_frame, int hue_frame, const EagleFlowKp* in, int n_in,
                  EagleFlowKp* out /* EAGLE_N_LANDMARKS */, int* n_out, float* next_pts /* 2*n_in or NULL */, uint8_t* status /* n_in or NULL */);

/* The ECC camera-motion kernels (ecc.hip, K17) without a handle: the two launches of eagle_clip_motion_ecc, each alone.
 * eagle_op_ecc_small: n gray frames [h][w] (the clip session's gray level 0) -> the scale-sized images [n][dh][dw] that cv2.resize((0, 0), fx = fy = scale)
 * gives, dh = lrint(h * scale), dw = lrint(w * scale), the taps taken from 1 / scale.  *dh_out, *dw_out are always written; small_out = NULL only asks for
 * them.  EAGLE_E_INVALID for dh < 4 or dw < 4, as eagle_clip_motion_ecc, and for a scale outside (0, 1].
 * eagle_op_ecc: findTransformECC(template, image, eye(2, 3), MOTION_EUCLIDEAN, (EPS | COUNT, max_iter, eps)) of n_pairs (template, image) index pairs into
 * small [n][h][w], all in ONE launch; the template index -1 is the image `carry` [h][w].  out[k] is the kernel's raw result: ok = 0 where cv2 raises (no pixel
 * inside the mask, a NaN correlation, lambda_d <= 0) and then iters counts the iteration that failed and rho, M are not meaningful; otherwise iters is the
 * number of iterations run, rho the last correlation (-1 with max_iter = 0) and M the 2 x 3 warp in the pixels of `small` (the translation NOT divided by
 * the scale).  EAGLE_E_INVALID for h < 4, w < 4, n < 1, an index outside [0, n), -1 without carry, max_iter outside [0, 100] and n_pairs outside [0, 4096];
 * n_pairs = 0 returns at once. */
typedef struct EagleEccResult { int32_t ok, iters; double rho; float M[6]; } EagleEccResult;
int eagle_op_ecc_small(int device, const uint8_t* gray, int n, int h, int w, double scale, uint8_t* small_out /* n*dh*dw or NULL */, int* dh_out, int* dw_out);
int eagle_op_ecc(int device, const uint8_t* small, int n, int h, int w, const uint8_t* carry /* h*w or NULL */, const int32_t* pairs /* 2*n_pairs */, int n_pairs,
                 int max_iter, double eps, EagleEccResult* out /* n_pairs */);

/* ---- ball flights: the ball's path cut into straight lines of constant speed (own specification: tests/flights_ref.py defines every output bit) -----
 * Opt-in; a table never asked is byte for byte what it was.  Between two touches a ball moves in a straight line at nearly constant speed on the pitch
 * plane, and a touch is where that line breaks: the stage finds those lines (flights) and breaks (knots; a knot with a large change of velocity is a
 * kick).  Integers wherever a sum is formed, float64 with single operations in the order written and no contraction, sqrt and division only.
 * INPUT.  The table's one Ball pitch column (video == 0), the kept frame numbers f[r], the Player and Goalkeeper pitch columns, and `cuts`: sorted
 * frame numbers at which a new shot starts (eagle_ball_track's).  A table without a ball column or flagged EAGLE_POST_NO_BALL gives no flight and no
 * kick: seg -1, flags 0, NaN everywhere.  rows == 0 is success.
 * PRESENCE.  eagle_post_smooth_tracks' rule: x and y finite and |x|, |y| <= 1024; q = rint(x * 1024) as int64, formed once.
 * RUNS.  Row r starts a run when r == 0, the ball is absent at r or at r - 1, f[r] - f[r-1] > max_gap, or f[r] is a cut.  A run with fewer than two
 * present rows has no segment.
 * SPIKES.  An interior row r of a run (p = r - 1 and n = r + 1 in the same run) has D[r] = f[n] - f[p] and A[r] = the maximum over the two axes of
 * |(q[r] - q[p]) D[r] - (q[n] - q[p]) (f[r] - f[p])|; A = 0 and D = 1 at a run's first and last row.  Row r is a spike when A[r] > T D[r] with T =
 * rint(spike * 1024), A[r] D[r-1] > A[r-1] D[r] and A[r] D[r+1] >= A[r+1] D[r]: two adjacent rows are never both spikes, a tie goes to the earlier
 * row, a run's ends are never spikes.  A spike is not "used": it enters no sum and is no knot; it receives the fitted values of the segment over it.
 * SEGMENT [i, j], used rows of one run with j - i <= L = max_rows.  Over the used rows r' of [i, j]: t = f[r'] - f[i], per axis d = q[r'] - q[i];
 * S0 = sum 1, S1 = sum t, S2 = sum t t, per axis B0 = sum d, B1 = sum t d, Q = sum d d (int64: t < 2^17, |d| <= 2^21, at most 129 terms, so
 * S2 < 2^42, |B1| < 2^46, Q < 2^50 and S0 S2, S1 S1 < 2^50).  det = (double)(S0 S2 - S1 S1), a0 = ((double)S2 (double)B0 - (double)S1 (double)B1) /
 * det, a1 = ((double)S0 (double)B1 - (double)S1 (double)B0) / det, sse = max(0, (double)Q - (a0 (double)B0 + a1 (double)B1)); cost = sse_x + sse_y,
 * c(i, j) = (int64) rint(min(cost, 2^40)).
 * DYNAMIC PROGRAM, per run: lam = rint(penalty ((noise 1024) (noise 1024))) <= 2^40; best[first] = 0, best[j] = min over used i < j with j - i <= L
 * of best[i] + c(i, j) + lam, a tie to the smaller i; the path is read back from the run's last row.  Segments are numbered in row order over all
 * runs; a knot is a row two consecutive segments of one run share.
 * PER SEGMENT EagleBallFlight: fitted ends (((double)q[i] + a0) + a1 t) / 1024; vx = (a1x fps) / 1024, speed = sqrt(vx vx + vy vy); rms =
 * sqrt((double)c / (double)used) / 1024; near = the used rows whose ball cell has a finite person cell within `radius` (eagle_post_possession's
 * candidate arithmetic); kind STILL when speed < still_speed, else CARRIED when 2 near > used, else FREE.  SHOT, for a FREE flight with speed >=
 * shot_speed and vx != 0: X = 105 for vx > 0, else 0; s = (X - x0) / vx, y_cross = y0 + vy s, reach = speed s; with 0 <= reach <= shot_range shot = 2
 * when |y_cross - 34| <= 3.66, 1 when <= 3.66 + shot_margin, else 0; y_cross is NaN when not evaluated.
 * PER KNOT: dv = sqrt(dvx dvx + dvy dvy) of the two flights' velocities; a kick when dv >= kick_dv.  EagleBallKick in row order: col = the nearest
 * finite person cell within `radius` at the row (a tie to the earlier column), -1: a bounce, a post or an unseen player; cos_turn = (vin . vout) /
 * (speed_in speed_out), NaN when a speed is 0.
 * PER ROW: seg (the segment that starts at a knot owns the knot row; -1 when absent or in a run without a segment), flags, the fitted position and the
 * segment's velocity (NaN where seg < 0).  Launches (csrc/flights.hip): prepare, cost, walk, path, fit, events. */
#define EAGLE_FLIGHT_STILL 0
#define EAGLE_FLIGHT_CARRIED 1
#define EAGLE_FLIGHT_FREE 2
#define EAGLE_FLIGHT_ROW_PRESENT 1     /* per-row flags */
#define EAGLE_FLIGHT_ROW_USED 2
#define EAGLE_FLIGHT_ROW_SPIKE 4
#define EAGLE_FLIGHT_ROW_KNOT 8
#define EAGLE_FLIGHT_ROW_KICK 16
#define EAGLE_FLIGHT_CAPPED 1          /* EagleBallFlight.flags: row1 - row0 == max_rows */
#define EAGLE_FLIGHT_CONTINUES 2       /* the knot at row1 is not a kick */
#define EAGLE_FLIGHT_LAYOUT_DEFAULT 0  /* how c(i, j) lies in HBM: the measured choice, or one of the two (tools/flights_rate.py, docs/experiments.md) */
#define EAGLE_FLIGHT_LAYOUT_END_MAJOR 1
#define EAGLE_FLIGHT_LAYOUT_K_MAJOR 2
#define EAGLE_FLIGHT_TIMES 7           /* times_ms: prepare, cost, walk, path, fit, events, the whole call */
typedef struct EagleFlightParams {     /* 96 bytes; eagle_flight_params_default fills the conventional choices (not fitted to data) */
    double fps;                    /* > 0, finite */
    int32_t max_gap;               /* 1 .. 1024 frames */
    int32_t max_rows;              /* L: 2 .. 128 (64) */
    double noise;                  /* metres, 0 .. 1024 (0.25) */
    double penalty;                /* >= 0 (16); penalty (noise 1024)^2 <= 2^40 */
    double spike;                  /* metres, 0 .. 1024 (1.0) */
    double kick_dv;                /* m/s, >= 0 (3) */
    double radius;                 /* metres, (0, 1024] (2) */
    double still_speed;            /* m/s, >= 0 (0.5) */
    double shot_speed;             /* m/s, >= 0 (10) */
    double shot_range;             /* metres, >= 0 (40) */
    double shot_margin;            /* metres, >= 0 (2) */
    int32_t layout;                /* EAGLE_FLIGHT_LAYOUT_* */
    int32_t reserved;              /* 0 */
} EagleFlightParams;
typedef struct EagleBallFlight {       /* 112 bytes */
    int32_t row0, row1, used, spikes;
    int32_t near, kind, shot, flags;
    double x0, y0, x1, y1, vx, vy, speed, rms, y_cross;
    int64_t c;
} EagleBallFlight;
typedef struct EagleBallKick {         /* 48 bytes */
    int32_t row, seg_in, seg_out, col;
    double speed_in, speed_out, dv, cos_turn;
} EagleBallKick;
typedef struct EagleFlightTotals {     /* 64 bytes */
    int32_t runs;                  /* runs with a present row */
    int32_t flights, kinds[3], spikes, knots, kicks;
    int32_t shots[3];              /* evaluated flights per shot value */
    int32_t capped;
    int64_t sum_c, reserved;
} EagleFlightTotals;
int eagle_flight_params_default(EagleFlightParams* p, double fps, int32_t max_gap);
/* EAGLE_E_INVALID with a message, before any launch and leaving every output alone, for NULL pointers, values outside the ranges above or not finite,
 * more than one Ball pitch column, a column of unknown kind, more than 2^20 rows, cuts that do not ascend, another handle's table.  The result is kept
 * with the table until eagle_post_free; a later call replaces it.  It reads whatever ball column the table has (raw, ball-tracked, smoothed); being a
 * derived result, eagle_post_stabilise and eagle_post_smooth_tracks refuse a table that carries it. */
int eagle_post_ball_flights(EagleHandle* h, EaglePostTable* t, const EagleFlightParams* p, const int32_t* cuts, int n_cuts);
/* Any pointer may be NULL.  seg int32 [rows], flags uint8 [rows], fitted and velocity float64 [rows][2].  EAGLE_E_INVALID before the call. */
int eagle_post_ball_flight_values(EaglePostTable* t, int32_t* seg, uint8_t* flags, double* fitted, double* velocity, EagleFlightTotals* totals);
int eagle_post_ball_flight_records(const EaglePostTable* t, EagleBallFlight* flights, int cap, int* n);
int eagle_post_ball_kicks(const EaglePostTable* t, EagleBallKick* kicks, int cap, int* n);
int eagle_post_device_ball_flights(const EaglePostTable* t, const int32_t** d_seg, const uint8_t** d_flags, const double** d_fitted,
                                   const double** d_velocity);                    /* NULLs before the call */
/* The launches on a constructed table in host memory (frames must ascend strictly); every output may be NULL; *n_flights and *n_kicks are the numbers
 * found, of which at most cap_flights / cap_kicks are written; times_ms: EAGLE_FLIGHT_TIMES milliseconds from device events, or NULL. */
int eagle_op_ball_flights(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* cuts,
                          int n_cuts, const EagleFlightParams* p, int32_t* seg, uint8_t* flags, double* fitted, double* velocity, EagleBallFlight* flights,
                          int cap_flights, int* n_flights, EagleBallKick* kicks, int cap_kicks, int* n_kicks, EagleFlightTotals* totals, float* times_ms);

/* ---- goal view: how much of the goal mouth every attacker, the ball and every cell of the pitch sees past the other team (K41; own specification:
 * tests/goalview_ref.py defines every output bit) ----
 * Opt-in, after the table is built; nothing in the table changes.  ARITHMETIC: float64, one operation at a time and in the order written here, no
 * contraction, correctly rounded division and sqrt; only + - * / sqrt, comparisons, floor/rint.  Sums are integers.
 *   POSITIONS  K33's: groups 0 and 1 (the Player pitch columns with a mapping entry), the keepers (the Goalkeeper pitch columns), the ball (the one Ball
 *              pitch column), present when x and y are finite and |x|, |y| <= 1024 m, q = floor(v * 1024 + 0.5); a position in metres is q / 1024, exact.
 *   GOALS      the lines x_g = 0 and x_g = 105; the mouth y = 30.34 .. 37.66 cut into 64 slices of DY = 7.32 / 64, slice k with centre
 *              yc_k = 30.34 + (k + 0.5) * DY.  direction: EAGLE_OFFSIDE_DIR_RIGHT (group 0 attacks x_g = 105, group 1 x_g = 0) or _LEFT; 0: the direction
 *              the table's offside result settled (refused without one, or when it settled none, and by the operator entry).
 *   BLOCKERS   of the attacking group g on a row: the present members of 1 - g with rho = radius and, with rho = keeper_radius, every present keeper that
 *              K33 counts among g's defenders (depth u > U_HALF); in table order.  More than EAGLE_GOALVIEW_BLOCKERS: the row's record of g has status
 *              TOO_MANY and nothing of g is evaluated on it.  n_blockers counts them all.
 *   POINT      P with s = x_g - P.x: absent -> ABSENT; a TOO_MANY row -> ROW; |s| < min_depth -> NEAR_LINE; ex = x_g - P.x, ey = 34 - P.y,
 *              ex ex + ey ey > max_range max_range -> FAR (open 0, mask 0); else OK.  Every other status: open -1, mask 0.
 *   SHADOW     a blocker D counts when its centre lies between the point and the line: wx = D.x - P.x, gx = x_g - D.x; s > 0: wx > 0 and gx >= 0;
 *              s < 0: wx < 0 and gx <= 0.  wy = D.y - P.y, d2 = wx wx + wy wy, r2 = rho rho.  d2 <= r2: all 64 slices.  Else l = sqrt(d2 - r2), the
 *              tangents t+ = (l wx - rho wy, l wy + rho wx), t- = (l wx + rho wy, l wy - rho wx); a tangent t reaches the line at
 *              y = P.y + (t.y s) / t.x when t.x has the sign of s, else at copysign(inf, t.y); lo and hi the smaller and the larger of the two; slice k
 *              is blocked iff lo <= yc_k <= hi.  mask: bit k set = slice k blocked by any blocker.
 *   ANGLE      w_k = rint(2^24 ((DY |s|) / (s s + (yc_k - P.y)^2))), int32 in units of 2^-24 rad (the midpoint rule of d theta / dy);
 *              full = sum of all w_k, open = sum over the slices not blocked.  |s| >= min_depth >= 1 keeps full below 2^27.
 *   RECORDS    [rows][2], the attacking group second: status (OK, TOO_MANY), n_blockers; the ball as a point (ball_status, ball_mask, ball_open,
 *              ball_full; full is 0 unless OK); best_col / best_open: the OK member of g with the largest open, of equal ones the smaller column (-1, -1
 *              without one); with an owner array whose entry of the row is a member of g: owner_col, owner_mask, owner_open (that member's), else -1, 0, -1.
 *   MEMBERS    in group order (0, then 1; by column inside): open int32, mask uint64, status uint8, [members][rows] each.
 *   TOTALS     per member over its OK rows: rows, sum_open, max_open and the earliest row attaining it (-1, -1 without a row), chance_rows =
 *              #{open >= rint(2^24 chance)}.
 *   GRID       optional (grid_rows > 0): uint8 [grid_rows][68 R][105 R] for table rows grid_row0 .., R = cells_per_metre; row 0 is y = 0, cell (j, i)'s
 *              point is ((i + 0.5) / R, (j + 0.5) / R); group 0 or 1, or -1: the group of which the row's owner is a member (no such group: zeros).  The
 *              byte is min(255, open >> 16) of an OK cell and 0 otherwise: one radian is 256.
 * Players are discs at their foot point; height, the ball's loft, shot speed and a keeper's dive are not modelled; the radii and every constant are
 * conventional choices, not fitted to data.  form chooses how the grid kernel gets a cell's weights: 64 divisions on the fly, or a prefix table
 * int32 [2][68 R][105 R][65] built once per call; the results are equal integers (docs/experiments.md, "Goal view (K41)").
 * EAGLE_E_INVALID with a message, before any launch and leaving every output and an earlier result alone: NULL pointers, values that are not finite,
 * radii outside [0, 16], min_depth < 1, max_range <= min_depth or > 1024, chance outside [0, 4], cells_per_metre outside {1, 2, 4}, an unknown
 * direction, group or form, direction 0 without a settled offside result, group -1 (with a grid) without a possession result / owner array, a table
 * without a mapping, grid rows outside the table, non-zero reserved words, a device-memory need beyond the budget. */
#define EAGLE_GOALVIEW_BLOCKERS 32
#define EAGLE_GOALVIEW_SLICES 64
#define EAGLE_GOALVIEW_OK 0        /* EagleGoalViewRow::status */
#define EAGLE_GOALVIEW_TOO_MANY 1
#define EAGLE_GOALVIEW_PT_OK 0     /* a point's status */
#define EAGLE_GOALVIEW_PT_ABSENT 1
#define EAGLE_GOALVIEW_PT_ROW 2    /* the row is TOO_MANY */
#define EAGLE_GOALVIEW_PT_NEAR_LINE 3
#define EAGLE_GOALVIEW_PT_FAR 4
#define EAGLE_GOALVIEW_FORM_DEFAULT 0
#define EAGLE_GOALVIEW_FORM_DIRECT 1
#define EAGLE_GOALVIEW_FORM_TABLE 2
#define EAGLE_GOALVIEW_TIMES 6     /* times_ms of eagle_op_goal_view: prepare, points, rows + totals, table, grid, total */
typedef struct EagleGoalViewParams {
    int32_t direction;             /* EAGLE_OFFSIDE_DIR_RIGHT, _LEFT; 0: the offside result's */
    int32_t group;                 /* the grid's attacking group: 0, 1, -1 (the owner's) */
    int32_t cells_per_metre;       /* 1, 2, 4 */
    int32_t form;                  /* EAGLE_GOALVIEW_FORM_* */
    int32_t grid_row0, grid_rows;  /* the grid's table rows; grid_rows == 0: no grid */
    double radius, keeper_radius;  /* metres, [0, 16] (0.4, 1.0) */
    double min_depth, max_range;   /* metres (1.0, 40.0) */
    double chance;                 /* radians (0.3) */
    int32_t reserved[2];           /* 0 */
} EagleGoalViewParams;             /* 72 bytes */
typedef struct EagleGoalViewRow {
    int32_t status, n_blockers;
    int32_t ball_status, ball_open, ball_full;
    int32_t best_col, best_open;
    int32_t owner_col, owner_open;
    int32_t reserved;              /* 0 */
    uint64_t ball_mask, owner_mask;
} EagleGoalViewRow;                /* 56 bytes */
typedef struct EagleGoalViewTotals {
    int32_t col, group;
    int32_t rows, max_open, max_row, chance_rows;
    int64_t sum_open;
} EagleGoalViewTotals;             /* 32 bytes */
int eagle_goal_view_params_default(EagleGoalViewParams* p);
/* The result is kept with the table until eagle_post_free; a call computes into a buffer of its own and replaces the earlier result when it is complete.
 * The owner array is the table's possession result at the time of the call (none: no owner anywhere).  Being a derived result, eagle_post_stabilise
 * and eagle_post_smooth_tracks refuse a table that carries it. */
int eagle_post_goal_view(EagleHandle* h, EaglePostTable* t, const EagleGoalViewParams* p);
/* To the host; any pointer may be NULL: rows_out [rows][2], open int32, mask uint64, status uint8 [members][rows], totals [members], grid uint8
 * [grid_rows][68 R][105 R].  EAGLE_E_INVALID before the call. */
int eagle_post_goal_view_values(EaglePostTable* t, EagleGoalViewRow* rows_out, int32_t* open, uint64_t* mask, uint8_t* status, EagleGoalViewTotals* totals,
                                uint8_t* grid);
/* In HBM; NULLs and zeros before the call (d_grid NULL without a grid).  The last four may be NULL. */
int eagle_post_device_goal_view(const EaglePostTable* t, const EagleGoalViewRow** d_rows, const int32_t** d_open, const uint64_t** d_mask, const uint8_t** d_status,
                                const EagleGoalViewTotals** d_totals, const uint8_t** d_grid, int* n_members, int* grid_row0, int* grid_rows, int* cells_per_metre);
/* Operator entry (host buffers in / out, no handle) for constructed tables, as eagle_op_offside; owner int32 [rows] (a column or -1) or NULL; every
 * output may be NULL; *n_members (may be NULL) is the number of members, written before anything else so that a caller can size its buffers with a
 * first call that passes no output; times_ms: EAGLE_GOALVIEW_TIMES milliseconds from device events, or NULL. */
int eagle_op_goal_view(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals,
                       int n_team, const int32_t* owner, const EagleGoalViewParams* p, EagleGoalViewRow* rows_out, int32_t* open, uint64_t* mask, uint8_t* status,
                       EagleGoalViewTotals* totals, uint8_t* grid, int* n_members, float* times_ms);

/* Developer diagnostics (process-wide switches and read-backs used by tools/probe_lk_concurrency.py; not part of the data path).
 * Inert (EAGLE_E_STATE) unless the process environment has EAGLE_ENABLE_DEBUG=1: a production caller cannot flip them by accident.
 * Keys: "lk_threads" (64 | 256), "lk_dbg" (1 trace, 2 LDS guard words, 4 end-of-level verification, 8 L1-bypassing loads), "lk_excl_lds" (bytes), "lk_trace", "lk_counters". */
int eagle_debug(const char* key, int64_t value, void* out, int64_t out_bytes);

#ifdef __cplusplus
}
#endif
#endif
