"""-m gpu: the fused input launch of HRNet in the split family (csrc/stem.hip: BGR u8 frame -> cv2.resize + A.Normalize + conv1 3x3/2 3->64 + BatchNorm + ReLU, no
key-point input tensor) through the C ABI's operator entry, against (a) the fp32 oracle on the oracle's own preprocess output and (b) the launches it replaces."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32S_TOL = 4e-6          # one split-family convolution against the fp32 oracle (tests/test_gpu_ops.py)
STEM_TOL = 2 * F32S_TOL   # two chained convolutions, the intermediate rounded to the split format (22+ bits) where the oracle keeps fp32 (as BNECK_TOL)


def _rand(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def _frames(n, h, w, seed):
    """noise on a smooth ramp: neighbouring source pixels differ, so a wrong tap or a wrong weight shows"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = ((yy * 3 + xx * 2) % 200)[None, :, :, None]
    return np.clip(ramp + rng.integers(0, 56, (n, h, w, 3)), 0, 255).astype(np.uint8)


def _weights(seed):
    w1 = _rand((3, 3, 3, 64), seed, (2.0 / 27) ** 0.5); b1 = _rand((64,), seed + 1, 0.1)
    w2 = _rand((3, 3, 64, 64), seed + 2, (2.0 / 576) ** 0.5); b2 = _rand((64,), seed + 3, 0.1)
    return w1, b1, w2, b2


def _oracle_input(frames, dh, dw):
    from oracle import host
    return np.concatenate([host.preprocess_keypoints(f, dh, dw) for f in frames])


def _relerr(ref, got):
    return float(np.abs(ref - got).max() / max(np.abs(ref).max(), 1e-6))


# (frames, source h, w, resized h, w): ragged maps with partial tiles in both directions (tile = 8 x 32 output pixels), a source smaller than one tile, the identity
# and exact-2x branches of the resize, an enlarging resize, odd and even map sizes, one and several frames
SHAPES = [(1, 9, 13, 9, 13), (2, 90, 160, 67, 131), (1, 20, 30, 10, 15), (3, 48, 64, 37, 70), (1, 33, 130, 33, 130), (5, 36, 100, 17, 66), (2, 64, 128, 32, 64),
          (1, 7, 5, 1, 1), (2, 100, 140, 50, 70)]


@pytest.mark.parametrize("shape", SHAPES)
def test_stem_against_the_oracle(shape):
    """conv1 of the fused launch below F32S_TOL, and the chain the pipeline runs (fused launch -> conv2 3x3/2 64->64) below 2 * F32S_TOL, both against the oracle's
    convolutions of the oracle's own preprocess output."""
    from eagle_amd import lib
    from oracle import prims as P
    n, sh, sw, dh, dw = shape
    frames = _frames(n, sh, sw, 11)
    w1, b1, w2, b2 = _weights(12)
    pre = _oracle_input(frames, dh, dw)
    ref1 = P.conv2d(pre, w1, b1, stride=2, post=1)
    got1, sat = lib.op_stem(frames, w1, b1, out_hw=(dh, dw))
    assert got1.shape == ref1.shape
    e1 = _relerr(ref1, got1)
    print(f"stem {shape}: conv1 error {e1:.3e}")
    assert e1 < F32S_TOL, f"fused stem error {e1}"
    assert not sat.any()
    ref2 = P.conv2d(ref1, w2, b2, stride=2, post=1)
    got2 = lib.op_conv2d(got1, w2, b2, 2, 0, None, None, 1, lib.PREC_F32S)
    e2 = _relerr(ref2, got2)
    print(f"stem {shape}: conv1 -> conv2 error {e2:.3e}")
    assert e2 < STEM_TOL, f"fused stem -> conv2 error {e2}"


@pytest.mark.parametrize("size", [(1, 720, 1280), (2, 1080, 1920)])
def test_stem_full_frames_against_the_oracle(size):
    """The pipeline's map (540 x 960 -> 270 x 480: 34 x 15 tiles, the last tile row 6 of 8 rows) from 720p (general resize) and 1080p (exact 2x decimation) sources."""
    from eagle_amd import lib
    from oracle import prims as P
    n, sh, sw = size
    frames = _frames(n, sh, sw, 21)
    w1, b1, w2, b2 = _weights(22)
    ref1 = P.conv2d(_oracle_input(frames, 540, 960), w1, b1, stride=2, post=1)
    got1, sat = lib.op_stem(frames, w1, b1)
    e1 = _relerr(ref1, got1)
    print(f"stem {size}: conv1 error {e1:.3e}")
    assert e1 < F32S_TOL and not sat.any()
    ref2 = P.conv2d(ref1, w2, b2, stride=2, post=1)
    e2 = _relerr(ref2, lib.op_conv2d(got1, w2, b2, 2, 0, None, None, 1, lib.PREC_F32S))
    print(f"stem {size}: conv1 -> conv2 error {e2:.3e}")
    assert e2 < STEM_TOL


def test_stem_against_the_launches_it_replaces():
    """One full 720 x 1280 frame: op_preprocess -> op_conv2d (the split family's K1 and generic conv1) against the fused launch.  The resized, normalised, split pixels are
    the same bits (one definition of the arithmetic, resize.h), so the outputs differ only by the order of the 27 products inside an accumulator; the same holds after
    conv2.  Measured on MI355X: 3.6e-7 (conv1), 5.6e-7 (after conv2), relative to the largest magnitude."""
    from eagle_amd import lib
    frames = _frames(1, 720, 1280, 31)
    w1, b1, w2, b2 = _weights(32)
    kp, _ = lib.op_preprocess(frames, precision=lib.PREC_F32S)
    unf1 = lib.op_conv2d(kp, w1, b1, 2, 0, None, None, 1, lib.PREC_F32S)
    got1, _ = lib.op_stem(frames, w1, b1)
    d1 = _relerr(unf1, got1)
    print(f"stem against preprocess -> conv1: {d1:.3e}")
    assert d1 < STEM_TOL
    unf2 = lib.op_conv2d(unf1, w2, b2, 2, 0, None, None, 1, lib.PREC_F32S)
    got2 = lib.op_conv2d(got1, w2, b2, 2, 0, None, None, 1, lib.PREC_F32S)
    d2 = _relerr(unf2, got2)
    print(f"stem -> conv2 against preprocess -> conv1 -> conv2: {d2:.3e}")
    assert d2 < STEM_TOL


def test_stem_zero_padding_of_the_resized_map():
    """conv1 pads the RESIZED map with zeros: a black frame normalises to about -2, so a kernel that resized beyond the map's border (or padded before normalising) would
    differ on every border pixel."""
    from eagle_amd import lib
    from oracle import prims as P
    frames = np.zeros((1, 40, 72, 3), np.uint8)
    w1, b1, _, _ = _weights(42)
    w1 = -np.abs(w1)                                           # negative inputs x negative weights: every output is large and positive, nothing hides behind the ReLU
    ref = P.conv2d(_oracle_input(frames, 30, 54), w1, b1, stride=2, post=1)
    got, _ = lib.op_stem(frames, w1, b1, out_hw=(30, 54))
    assert _relerr(ref, got) < F32S_TOL


def test_stem_counts_clipped_stores_per_frame():
    """Weights scaled so that conv1's outputs of a white frame exceed the split format's range (+-4094) while those of a mid-grey frame (normalised values near zero) stay
    inside: the call flags exactly the frames the unfused path clips, the clipped values are the format's maximum, and a frame's count is bounded by one per lane and
    tile (a lane reports once per workgroup; there is no recomputed halo in this launch that could count twice)."""
    from eagle_amd import lib
    frames = np.stack([np.full((90, 160, 3), 255, np.uint8), np.full((90, 160, 3), 114, np.uint8), np.full((90, 160, 3), 255, np.uint8)])
    w1 = np.abs(_rand((3, 3, 3, 64), 52, 0.27)) * 1000.0
    b1 = _rand((64,), 53, 0.1)
    got, sat = lib.op_stem(frames, w1, b1, out_hw=(90, 160))
    kp, _ = lib.op_preprocess(frames, precision=lib.PREC_F32S)          # (540 x 960: another map, the same per-frame verdict)
    unf = lib.op_conv2d(kp, w1, b1, 2, 0, None, None, 1, lib.PREC_F32S)
    clipped_unfused = [bool((unf[i] >= 4094.0).any()) for i in range(3)]
    assert clipped_unfused == [True, False, True]
    assert [bool(s) for s in sat] == clipped_unfused, f"saturated frames {sat}"
    assert float(got[0].max()) == 4094.0 and float(got[1].max()) < 4094.0 and np.isfinite(got).all()
    tiles = -(-45 // 8) * -(-80 // 32)
    assert 0 < int(sat[0]) <= tiles * 256 and int(sat[0]) == int(sat[2])


def test_default_handle_runs_the_fused_stem_and_reports_it():
    """The split-family handle's schedule starts with the fused launch (a `conv stem` row in the per-kernel table, no conv1 row of the generic kernel), and frames beyond
    n_active of a short last step do not disturb the records of the active ones (the launch covers n_active frames only)."""
    from eagle_amd import lib, synth, weights
    from eagle_amd.coordinate_model import CoordinateModel
    hs, ys = weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)
    frames = np.stack([synth.frame(0, 3 * t) for t in range(3)])
    cm = CoordinateModel(precision="f32s", batch=2, hrnet_state_dict=hs, detector_state_dict=ys)
    full = cm.process_records(frames)                          # steps of 2 + 1 frames
    cm.handle.set_profiling(True)
    cm.process_records(frames[:2])
    names = [row[0] for row in cm.handle.kernel_times()]
    cm.handle.close()
    assert any(nm.startswith("conv stem 3x3/2 3->64 @270x480") for nm in names), names
    assert not any(nm.startswith("conv 3x3/2 3->64") for nm in names), names
    cm1 = CoordinateModel(precision="f32s", batch=1, hrnet_state_dict=hs, detector_state_dict=ys)
    one = cm1.process_records(frames)
    cm1.handle.close()
    for a, b in zip(full, one):
        assert np.array_equal(a["hm_idx"], b["hm_idx"]) and np.array_equal(a["hm_score"], b["hm_score"])
