"""Annotated output on the GPU (include/eagle.h, eagle_annotate_* / eagle_op_annotate; csrc/annotate.hip): every output byte equals the numpy
contract of tests/annot_ref.py — drawing, painter's order, clipping, BGR / NV12 / I420 in dense and padded layouts; the library's overlay of
a record equals the contract's; the handle entries agree with the operator, with each other (pinned / pageable, NV12-fed / BGR-fed clips) and
leave the handle's records, graphs and the source clip alone; bad output layouts come back as EagleError; Processor.annotate and the CLI."""
import json
import os

import numpy as np
import pytest

import annot_ref as A
import yuv_ref as Y
from eagle_amd import lib, synth, weights

pytestmark = pytest.mark.gpu
FMTS = ["bgr", "nv12", "i420"]


def _prim_array(prims):
    a = np.zeros(len(prims), lib.PRIM_DTYPE)
    for i, p in enumerate(prims):
        a[i]["kind"], a[i]["a"] = p[0], p[1:7]
        a[i]["b"], a[i]["g"], a[i]["r"] = p[7]
    return a


def _pack(prim_lists):
    offs = np.cumsum([0] + [len(p) for p in prim_lists]).astype(np.int32)
    return _prim_array([p for lst in prim_lists for p in lst]), offs


def _random_prims(r, h, w, count):
    out = []
    for i in range(count):
        color = tuple(int(v) for v in r.integers(0, 256, 3))
        x, y = int(r.integers(-40, w + 40)), int(r.integers(-40, h + 40))
        kind = i % 4
        if kind == A.ARC:
            out.append(A.arc(x, y, color))
        elif kind == A.LABEL:
            out.append(A.label(x, y, int(r.choice([r.integers(0, 10), r.integers(0, 100000), -3, 100000, 7, 10, 99999])), color))
        elif kind == A.DISC:
            out.append(A.disc(x, y, int(r.integers(0, 13)), color))
        else:
            v = r.integers(-30, 31, 6)
            out.append(A.tri(x + v[0], y + v[1], x + v[2], y + v[3], x + v[4], y + v[5], color))
    return out


def _padded_layout(fmt, h, w):
    """an encoder surface: pitch padded, chroma after h + 16 rows, chroma pitch padded too; BGR: row pitch padded, frames apart"""
    if fmt == "bgr":
        return {"y_pitch": 3 * w + 40, "frame_stride": (3 * w + 40) * (h + 3)}
    yp = w + 64
    return {"y_pitch": yp, "c_offset": yp * (h + 16), "c_pitch": yp if fmt == "nv12" else w // 2 + 32}


def _op_case(fmt, case):
    r = np.random.default_rng(23)
    lay, n_prims = None, 512
    if case in ("random720", "empty"):
        n, h, w = 2, 720, 1280
        frames = r.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        if case == "empty":
            n_prims = 0
    elif case == "extremes":
        lv = [0, 1, 127, 128, 254, 255]
        cols = np.array([[b, g, rr] for b in lv for g in lv for rr in lv], np.uint8)              # 216 colours
        n, h, w = 2, 24, 36
        frames = np.stack([cols.reshape(12, 18, 3).repeat(2, 0).repeat(2, 1), np.roll(cols, 1, 0).reshape(24, 9, 3).repeat(4, 1)])
    elif case == "oddwidth":
        n, h, w = 2, 37, 45                                                                      # BGR only: odd rows and columns, a 5-pixel tail strip
        frames = r.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    elif case == "tail":
        n, h, w = 3, 18, 34                                                                      # 34 = 4 strips of 8 + a 2-pixel tail; rows not 8-byte aligned
        frames = r.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    else:
        n, h, w = 2, 64, 200                                                                     # padded layout; 200 = 25 strips
        frames = r.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        lay = _padded_layout(fmt, h, w)
    lists = [[] for _ in range(n)]
    lists[0] = _random_prims(r, h, w, n_prims)                                                   # 512 on one frame, none on its neighbours
    return frames, lists, lay


OP_CASES = [(f, c) for f in FMTS for c in ("random720", "extremes", "oddwidth", "tail", "padded", "empty") if c != "oddwidth" or f == "bgr"]


@pytest.mark.parametrize("fmt,case", OP_CASES)
def test_op_annotate_equals_oracle(fmt, case):
    frames, lists, lay = _op_case(fmt, case)
    n, h, w, _ = frames.shape
    src = frames.copy()
    prims, offs = _pack(lists)
    exp = A.annotate(frames, lists, fmt, lay, fill=201)
    out = np.full(exp.size, 201, np.uint8) if lay is not None else None
    got = lib.op_annotate(frames, prims, offs, fmt, lay, out=out)
    assert np.array_equal(frames, src)                                       # the source is read only
    assert np.array_equal(got.reshape(-1), exp)                              # pad bytes (201) included
    if case != "empty":
        assert not np.array_equal(exp, A.annotate(frames, [[] for _ in lists], fmt, lay, fill=201))      # the overlay is in the picture
    if fmt != "bgr" and lay is None:                                         # NV12 and I420 carry the same samples
        other = "i420" if fmt == "nv12" else "nv12"
        assert all(np.array_equal(a, b) for a, b in zip(Y.split(fmt, got), Y.split(other, lib.op_annotate(frames, prims, offs, other))))


def test_op_annotate_rejects_bad_primitives():
    f = np.zeros((1, 8, 8, 3), np.uint8)
    for bad, what in ((A.disc(0, 0, -1, A.BLACK), "radius"), (A.disc(1 << 21, 0, 1, A.BLACK), "coordinate"), ((7, 0, 0, 0, 0, 0, 0, A.BLACK), "kind")):
        with pytest.raises(lib.EagleError, match=what):
            lib.op_annotate(f, *_pack([[bad]]))
    with pytest.raises(lib.EagleError, match="EAGLE_MAX_PRIMS"):
        lib.op_annotate(f, *_pack([[A.disc(0, 0, 1, A.BLACK)] * (lib.MAX_PRIMS + 1)]))
    assert lib.op_annotate(f, *_pack([[A.disc(0, 0, 1, A.BLACK)] * lib.MAX_PRIMS])).shape == (1, 8, 8, 3)


# ---- the handle ---------------------------------------------------------------------------------------------------------------
def _handle(state_dicts, batch, h=720, w=1280):
    hd = lib.Handle(batch=batch, frame_h=h, frame_w=w)
    weights.load_into(hd, list(state_dicts))
    return hd


def _as_tuples(prims):
    return [(int(p["kind"]), *map(int, p["a"]), (int(p["b"]), int(p["g"]), int(p["r"]))) for p in prims]


def _dressed(recs):
    """the handle's own records + copies in which a few detections are made reported persons / balls and a homography is claimed, so that every
    branch of the overlay is exercised whatever the seeded random networks report"""
    out = np.concatenate([recs, recs.copy()])
    for r in out[len(recs):]:
        n = int(r["n_det"]) if int(r["n_det"]) >= 6 else 6
        r["n_det"] = n
        for j in range(n):
            d = r["det"][j]
            d["reported"], d["cls"], d["id"] = j % 5 != 4, (0, 1, 2, 0, 3, 2)[j % 6], j
            if not (0 <= int(d["foot_x"]) < 1280 and 0 <= int(d["foot_y"]) < 720):
                d["foot_x"], d["foot_y"] = 100 + 150 * j % 1100, 80 + 90 * j % 600
        r["H_valid"] = 1
        for k in range(int(r["n_kp"])):
            r["kp"][k]["on_plane"], r["kp"][k]["inlier"] = 1, k % 2
    return out


def _mapping(recs):
    ids = sorted({int(d["id"]) for r in recs for d in r["det"][: int(r["n_det"])] if int(d["cls"]) == 0})
    return {i: k % 2 for k, i in enumerate(ids) if k % 3 != 2}                # every third player has no team


def test_overlay_from_record_equals_oracle(state_dicts):
    frames = synth.clip(3, 4)
    hd = _handle(state_dicts, 4)
    try:
        recs = _dressed(hd.process(frames))
    finally:
        hd.close()
    mapping = _mapping(recs)
    n_prims = 0
    for r in recs:
        for m in (None, mapping, {}):
            exp = A.overlay_from_record(r, m)
            assert _as_tuples(lib.overlay_from_record(r, m)) == exp
            n_prims += len(exp)
    assert n_prims > 0


def test_handle_annotate_equals_oracle_and_has_no_side_effect(state_dicts):
    """batch 4 (graph replay), 6 frames: the annotated output of the handle's own records equals the contract in all three formats, pinned and pageable
    destinations agree, a padded BGR surface in HBM is written in place, an NV12-fed clip gives the BGR-fed clip's output; processing the clip again
    afterwards gives byte-identical records (also those of a handle that never annotated) without a new graph capture, and the clip is unchanged."""
    n = 6
    yuv = synth.bgr_to_nv12(synth.clip(5, n))
    frames = Y.to_bgr("nv12", yuv)
    fresh = _handle(state_dicts, 4)
    try:
        never = fresh.process(frames)
    finally:
        fresh.close()
    hd = _handle(state_dicts, 4)
    try:
        recs0 = hd.process(frames)
        assert recs0.tobytes() == never.tobytes()
        caps = hd.timings().graph_captures
        assert caps > 0
        recs = _dressed(recs0)[n:]                                              # same frames, records with every branch of the overlay
        mapping = _mapping(recs)
        d = hd.upload(frames)
        d_yuv = hd.upload(yuv)
        d_from_yuv = hd.yuv_to_bgr_device(d_yuv, n, "nv12")
        try:
            for use, mp in ((recs0, None), (recs, mapping)):
                lists = [A.overlay_from_record(r, mp) for r in use]
                for fmt in FMTS:
                    exp = A.annotate_dense(frames, lists, fmt)
                    got = hd.annotate(d, n, use, mp, fmt)
                    assert got.shape == exp.shape and np.array_equal(got, exp), fmt
                    assert np.array_equal(hd.annotate(d_from_yuv, n, use, mp, fmt), exp), fmt       # NV12-fed clip == BGR-fed clip
                    pinned = hd.host_buffer(exp.nbytes)
                    try:
                        pinned[:] = 0
                        assert np.array_equal(hd.annotate(d, n, use, mp, fmt, out=pinned)[: exp.nbytes], exp.reshape(-1)), fmt
                    finally:
                        hd.host_free(pinned)
            assert sum(len(A.overlay_from_record(r, mapping)) for r in recs) > 0
            # pitched output: host (pageable and pinned) and device (an encoder's surface)
            lists = [A.overlay_from_record(r, mapping) for r in recs]
            for fmt in FMTS:
                lay = _padded_layout(fmt, 720, 1280)
                exp = A.annotate(frames, lists, fmt, lay, fill=9)
                assert np.array_equal(hd.annotate(d, n, recs, mapping, fmt, lay, out=np.full(exp.size, 9, np.uint8)), exp), fmt
                pinned = hd.host_buffer(exp.size)
                try:
                    pinned[:] = 9
                    assert np.array_equal(hd.annotate(d, n, recs, mapping, fmt, lay, out=pinned), exp), fmt
                finally:
                    hd.host_free(pinned)
                d_out = hd.upload(np.full(exp.size, 9, np.uint8))
                try:
                    hd.annotate_device(d, n, recs, d_out, mapping, fmt, lay)
                    # a 4:2:0 surface is read back through the library's own conversion (pitched BGR stores are compared byte for byte in the operator test)
                    if fmt != "bgr":
                        back = hd.yuv_to_bgr_device(d_out, n, fmt, lay)
                        try:
                            again = hd.annotate(back, n, np.zeros(n, lib.RESULT_DTYPE), None, "bgr")
                        finally:
                            hd.free(back)
                        assert np.array_equal(again, Y.to_bgr(fmt, exp, lay, 720, 1280, n)), fmt
                finally:
                    hd.free(d_out)
            # no side effect: the clip, the records, the graphs
            assert np.array_equal(hd.annotate(d, n, np.zeros(n, lib.RESULT_DTYPE), None, "bgr"), frames)      # an empty overlay copies: the clip is as uploaded
            assert hd.process_device(d, n).tobytes() == recs0.tobytes()
        finally:
            hd.free(d); hd.free(d_yuv); hd.free(d_from_yuv)
        assert hd.process(frames).tobytes() == recs0.tobytes()
        assert hd.timings().graph_captures == caps
    finally:
        hd.close()


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_bad_output_layouts_raise_and_leave_the_handle_usable(state_dicts, fmt):
    n, h, w = 2, 720, 1280
    frames = synth.clip(8, n)
    hd = _handle(state_dicts, 2)
    try:
        exp = hd.process(frames)
        d = hd.upload(frames)
        try:
            flat = np.zeros(8 << 20, np.uint8)
            one = np.zeros((1, 8, 7, 3), np.uint8)
            with pytest.raises(lib.EagleError, match="even"):
                lib.op_annotate(one, *_pack([[]]), fmt)
            assert lib.op_annotate(one, *_pack([[]]), "bgr").shape == one.shape                   # BGR output takes odd sizes
            with pytest.raises(lib.EagleError, match="unknown pixel format"):
                hd.annotate(d, n, exp, None, 3, out=flat)
            with pytest.raises(lib.EagleError, match="y_pitch"):
                hd.annotate(d, n, exp, None, fmt, {"y_pitch": w - 2}, out=flat)
            with pytest.raises(lib.EagleError, match="y_pitch"):
                hd.annotate(d, n, exp, None, "bgr", {"y_pitch": 3 * w - 1}, out=flat)
            with pytest.raises(lib.EagleError, match="negative"):
                hd.annotate(d, n, exp, None, fmt, {"c_pitch": -8}, out=flat)
            with pytest.raises(lib.EagleError, match="overlaps"):
                hd.annotate(d, n, exp, None, fmt, {"c_offset": w * (h - 1)}, out=flat)
            with pytest.raises(lib.EagleError, match="frame_stride"):
                hd.annotate(d, n, exp, None, fmt, {"frame_stride": w * h}, out=flat)
            d_out = hd.upload(flat)
            try:
                with pytest.raises(lib.EagleError, match="frame_stride"):
                    hd.annotate_device(d, n, exp, d_out, None, fmt, {"frame_stride": w * h})
                hd.annotate_device(d, n, exp, d_out, None, fmt)
            finally:
                hd.free(d_out)
            lists = [A.overlay_from_record(r, None) for r in exp]
            assert np.array_equal(hd.annotate(d, n, exp, None, fmt), A.annotate_dense(frames, lists, fmt))
            assert hd.process_device(d, n).tobytes() == exp.tobytes()
        finally:
            hd.free(d)
    finally:
        hd.close()


# ---- the Python API above the handle, and the command line -----------------------------------------------------------------------
def _read_y4m(path):
    blob = open(path, "rb").read()
    header, rest = blob.split(b"\n", 1)
    tok = header.decode().split()
    assert tok[0] == "YUV4MPEG2" and "C420jpeg" in tok
    w, h = int(next(t for t in tok if t[0] == "W")[1:]), int(next(t for t in tok if t[0] == "H")[1:])
    fsz = 3 * h * w // 2
    assert len(rest) % (6 + fsz) == 0
    frames = []
    for k in range(len(rest) // (6 + fsz)):
        chunk = rest[k * (6 + fsz): (k + 1) * (6 + fsz)]
        assert chunk[:6] == b"FRAME\n"
        frames.append(np.frombuffer(chunk[6:], np.uint8).reshape(h * 3 // 2, w))
    return tok, np.stack(frames)


def test_processor_annotate_and_cli(state_dicts, tmp_path):
    from eagle_amd import cli
    from eagle_amd.annotate import annotate, overlay
    from eagle_amd.processor import Processor
    n, fps = 5, 5
    frames = synth.clip(0, n)
    # the command line: with the flag three files, without it the two it always wrote
    out_a, out_b = str(tmp_path / "with"), str(tmp_path / "without")
    common = ["--frames", str(n), "--fps", str(fps), "--seed", "0", "--synthetic-weights", "--batch", "4"]
    assert cli.main(common + ["--out", out_a, "--annotated"]) == 0
    assert cli.main(common + ["--out", out_b]) == 0
    assert sorted(os.listdir(out_a)) == ["annotated.y4m", "metadata.json", "raw_coordinates.json"]
    assert sorted(os.listdir(out_b)) == ["metadata.json", "raw_coordinates.json"]
    assert open(os.path.join(out_a, "raw_coordinates.json")).read() == open(os.path.join(out_b, "raw_coordinates.json")).read()
    meta_a, meta_b = json.load(open(os.path.join(out_a, "metadata.json"))), json.load(open(os.path.join(out_b, "metadata.json")))
    assert isinstance(meta_a["team_mapping"], dict) and "note" not in meta_a
    assert sorted(meta_b) == ["fps", "frames", "note", "seconds"] and "team_mapping" not in meta_b
    tok, video = _read_y4m(os.path.join(out_a, "annotated.y4m"))
    assert f"W{frames.shape[2]}" in tok and f"H{frames.shape[1]}" in tok and f"F{fps}:1" in tok and len(video) == n
    # the same through the library: Processor.annotate on the dict of the last get_coordinates call, in the CLI's cadence
    p = Processor(batch=4, hrnet_state_dict=state_dicts[0], detector_state_dict=state_dicts[1])
    try:
        coords = p.model.get_coordinates(frames, fps, num_homography=1, num_keypoint_detection=3, verbose=False)
        mapping = p.get_team_mapping(frames, coords)
        assert {str(k): v for k, v in mapping.items()} == meta_a["team_mapping"]
        got = p.annotate(frames, coords, mapping, out_format="i420")
        assert np.array_equal(got, video)
        # ... which is the contract applied to the records behind that dict: every frame's dict key-points are drawn
        _, recs, own = p.model._last
        shown = recs.copy(); shown["H_valid"][~own] = 0
        lists = [A.overlay_from_record(r, mapping) for r in shown]
        assert np.array_equal(got, A.annotate_dense(frames, lists, "i420"))
        for i, lst in enumerate(lists):
            assert [(q[1], q[2]) for q in lst if q[0] == A.DISC] == [(int(v[0]), int(v[1])) for v in coords[i]["Keypoints"].values()]
            assert overlay(shown[i], mapping) == lst
        # raw records, 4:2:0 input, BGR output; and the module-level function on a resident clip
        raw = p.model.process_records(frames)
        exp = A.annotate_dense(frames, [A.overlay_from_record(r, None) for r in raw], "bgr")
        assert np.array_equal(p.annotate(frames, raw), exp)
        nv = synth.bgr_to_nv12(frames)
        bgr_of_nv = Y.to_bgr("nv12", nv)
        raw_nv = p.model.process_records(nv, "nv12")
        assert np.array_equal(p.annotate(nv, raw_nv, None, "nv12", "nv12"), A.annotate_dense(bgr_of_nv, [A.overlay_from_record(r, None) for r in raw_nv], "nv12"))
        d = p.model.handle.upload(frames)
        try:
            assert np.array_equal(annotate(p.model.handle, d, raw), exp)
        finally:
            p.model.handle.free(d)
        with pytest.raises(ValueError):
            p.annotate(frames, dict(coords))                                 # not the dict of the last get_coordinates call
    finally:
        p.model.handle.close()
