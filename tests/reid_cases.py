"""Cases and references for the OSNet (ReID) kernels of csrc/reid.hip, one operator at a time (no GPU; tests/test_gpu_reid_ops.py runs them
on the GPU, tests/test_reid_cases_cpu.py checks the references themselves).

Per operator there are two statements of the same arithmetic over the float32 arrays the kernel gets:
  *_ref   plain float64 numpy (explicit padding and tap loops), with the forward-error bound of the kernel's chain next to it:
          |got - ref| <= gamma_k * S, u = 2^-24, gamma_k = k u / (1 - k u), k the rounded operations on the longest path of one output and S the
          float64 sum of the absolute values of its terms, bias included (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1);
  *_f32   the kernel's own order in float32, every fmaf through oracle.prims.fmaf (C fmaf, one rounding): what the kernel must give bit for bit
          (the library is built with -ffp-contract=off and spells its fmaf's out).
The rounded operations per output:
  conv7   147 fmaf + the bias add                                      k = 148
  dw3     9 fmaf + the bias add                                        k = 10
  means   (gate, head) HW pixels over step = 256 / C lanes: ceil(HW / step) - 1 adds per lane (the first adds to 0), step - 1 adds across
          lanes, one division                                          k1 = ceil(HW / step) + step - 1
  fc      a bias followed by m fmaf                                    k = m   (gate fc1: c_real, fc2: r; head: C)
A two-stage bound propagates the first stage's bound through the absolute weights of the second; ReLU is 1-Lipschitz, the sigmoid 1/4-Lipschitz."""
import math

import numpy as np

U = 2.0 ** -24
K_CONV7, K_DW3 = 148, 10
SENTINEL = 0x7FC5E171
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def gamma(k):
    return k * U / (1.0 - k * U)


def k_mean(hw, c):
    step = 256 // c
    return -(-hw // step) + step - 1


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------------
def tensor(seed, shape, neg_channel=None, zeros=0.2):
    """normal values, a fifth of them exact zeros (so ReLU and max matter); channel ``neg_channel`` strictly negative everywhere"""
    r = np.random.default_rng(seed)
    x = r.standard_normal(shape).astype(np.float32)
    x[r.random(shape) < zeros] = 0.0
    if neg_channel is not None:
        x[..., neg_channel] = -(0.5 + r.random(shape[:-1])).astype(np.float32)
    return x


def weights(seed, shape, scale=0.5):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


# ---- float64 references ---------------------------------------------------------------------------------------------------------------------
def _taps(x, ks, stride, pad, ho, wo, fill, skip_last_col=False):
    """yield ((ky, kx), window [n, ho, wo, c]) of the padded float64 input; skip_last_col: the seeded mistake ``ix >= w - 1`` (the last input
    column counts as padding, i.e. every border tap that reads it is dropped)"""
    n, h, w, c = x.shape
    x = x.astype(np.float64)
    if skip_last_col:
        x = x.copy(); x[:, :, w - 1, :] = fill
    xp = np.full((n, (ho - 1) * stride + ks, (wo - 1) * stride + ks, c), fill, np.float64)
    hh, ww = min(h, xp.shape[1] - pad), min(w, xp.shape[2] - pad)
    xp[:, pad:pad + hh, pad:pad + ww] = x[:, :hh, :ww]
    for ky in range(ks):
        for kx in range(ks):
            yield (ky, kx), xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]


def conv7_ref(x, w, b, skip_last_col=False):
    """x [n, h, w, 4] (4th channel unused), w [7, 7, 3, 16], b [16] -> (relu(conv + b) float64 [n, ho, wo, 16], bound)"""
    n, h, wd, _ = x.shape
    ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    acc = np.zeros((n, ho, wo, 16)); s = np.zeros_like(acc)
    w = w.astype(np.float64)
    for (ky, kx), win in _taps(x[..., :3], 7, 2, 3, ho, wo, 0.0, skip_last_col):
        for c in range(3):
            t = win[..., c:c + 1] * w[ky, kx, c]
            acc += t; s += np.abs(t)
    b = b.astype(np.float64)
    return np.maximum(acc + b, 0.0), gamma(K_CONV7) * (s + np.abs(b))


def dw3_ref(x, w, b, skip_last_col=False):
    """x [n, h, w, C], w [9, C], b [C] -> (relu(depthwise + b) float64, bound)"""
    n, h, wd, c = x.shape
    acc = np.zeros(x.shape); s = np.zeros(x.shape)
    w = w.astype(np.float64)
    for (ky, kx), win in _taps(x, 3, 1, 1, h, wd, 0.0, skip_last_col):
        t = win * w[ky * 3 + kx]
        acc += t; s += np.abs(t)
    b = b.astype(np.float64)
    return np.maximum(acc + b, 0.0), gamma(K_DW3) * (s + np.abs(b))


def maxpool3s2_ref(x):
    """MaxPool2d(3, 2, 1): padding never wins (-inf).  Exact in any precision: returns float32"""
    return _maxpool64(x).astype(np.float32)


def avgpool2_ref(x):
    """AvgPool2d(2, 2) as the kernel spells it, ((a + b) + (d + e)) * 0.25 in float32; an odd last row / column is not read"""
    n, h, wd, c = x.shape
    ho, wo = h // 2, wd // 2
    v = x[:, :2 * ho, :2 * wo].reshape(n, ho, 2, wo, 2, c)
    return ((v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + (v[:, :, 1, :, 0] + v[:, :, 1, :, 1])) * np.float32(0.25)


def _mean_ref(x, divisor_plus=0):
    """channel means over the map in float64 and their bound gamma_k1 * mean|x|"""
    n, h, wd, c = x.shape
    hw = h * wd
    x = x.reshape(n, hw, c).astype(np.float64)
    return x.sum(1) / (hw + divisor_plus), gamma(k_mean(hw, c)) * np.abs(x).sum(1) / hw


def _fc_ref(v, ev, w, b):
    """t = v @ w.T + b with v known to +-ev, computed as a bias and m fmaf's: -> (t, bound)"""
    w = w.astype(np.float64); b = b.astype(np.float64)
    m = w.shape[1]
    return v @ w.T + b, gamma(m) * ((np.abs(v) + ev) @ np.abs(w).T + np.abs(b)) + ev @ np.abs(w).T


def gate_ref(streams, w1, b1, w2, b2, divisor_plus=0):
    """streams 4 x [n, h, w, C], w1 [r, c_real], w2 [c_real, r] -> (t [n, 4, c_real] the float64 pre-activation of the sigmoid, its bound,
    g = 1 / (1 + exp(-t)) padded with zeros to [n, 4, C]).  divisor_plus: the seeded mistake HW -> HW + 1"""
    c = streams[0].shape[-1]
    c_real = w1.shape[1]
    ts, es = [], []
    for s in streams:
        m, em = _mean_ref(s, divisor_plus)
        hid, eh = _fc_ref(m[:, :c_real], em[:, :c_real], w1, b1)
        t, et = _fc_ref(np.maximum(hid, 0.0), eh, w2, b2)
        ts.append(t); es.append(et)
    t, et = np.stack(ts, 1), np.stack(es, 1)
    g = np.zeros(t.shape[:2] + (c,))
    g[..., :c_real] = 1.0 / (1.0 + np.exp(-t))
    return t, et, g


def gate_g_bound(et, g):
    """|g_kernel - g| <= bound(t) / 4 (the sigmoid's Lipschitz constant) + 2 ulp of g, padded like g (padding gates are exactly 0)"""
    c_real = et.shape[-1]
    out = np.zeros(g.shape)
    out[..., :c_real] = et / 4.0 + 2.0 * np.spacing(g[..., :c_real].astype(np.float32)).astype(np.float64)
    return out


def gated_sum_f32(streams, g):
    """((v0 g0 + v1 g1) + v2 g2) + v3 g3 in float32 with the gates g [n, 4, C] given"""
    p = [streams[k] * g[:, k, None, None, :] for k in range(4)]
    return ((p[0] + p[1]) + p[2]) + p[3]


def head_ref(x, w, b):
    """x [n, h, w, C], w [dim, C], b [dim] -> (relu(mean(x) @ w.T + b) float64 [n, dim], bound)"""
    m, em = _mean_ref(x)
    t, et = _fc_ref(m, em, w, b)
    return np.maximum(t, 0.0), et


# ---- the kernels' own order in float32 (bit-exact restatements) -----------------------------------------------------------------------------
def _taps_f32(x, ks, stride, pad, ho, wo):
    n, h, w, c = x.shape
    xp = np.zeros((n, (ho - 1) * stride + ks, (wo - 1) * stride + ks, c), np.float32)
    hh, ww = min(h, xp.shape[1] - pad), min(w, xp.shape[2] - pad)
    xp[:, pad:pad + hh, pad:pad + ww] = x[:, :hh, :ww]
    for ky in range(ks):
        for kx in range(ks):
            yield (ky, kx), xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]


def conv7_f32(x, w, b):
    """taps row-major, channels x, y, z inside a tap, one fmaf each; a zero-padded tap leaves the accumulator as it is (fmaf(0, w, acc) = acc),
    which is what the kernel's ``continue`` does"""
    from oracle import prims as P
    n, h, wd, _ = x.shape
    ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    acc = np.zeros((n, ho, wo, 16), np.float32)
    for (ky, kx), win in _taps_f32(x[..., :3], 7, 2, 3, ho, wo):
        for c in range(3):
            acc = P.fmaf(win[..., c:c + 1], w[ky, kx, c], acc)
    return np.maximum(acc + b, np.float32(0))


def dw3_f32(x, w, b):
    from oracle import prims as P
    n, h, wd, c = x.shape
    acc = np.zeros(x.shape, np.float32)
    for (ky, kx), win in _taps_f32(x, 3, 1, 1, h, wd):
        acc = P.fmaf(win, w[ky * 3 + kx], acc)
    return np.maximum(acc + b, np.float32(0))


def _mean_f32(x, divisor_plus=0):
    """thread (lane, ch) sums pixels lane, lane + step, ... in order; lanes are then added in order; one division"""
    n, h, wd, c = x.shape
    hw, step = h * wd, 256 // c
    x = x.reshape(n, hw, c)
    part = np.zeros((n, step, c), np.float32)
    for p0 in range(0, hw, step):
        blk = x[:, p0:p0 + step]
        part[:, :blk.shape[1]] = part[:, :blk.shape[1]] + blk
    t = np.zeros((n, c), np.float32)
    for lane in range(step):
        t = t + part[:, lane]
    return t / np.float32(hw + divisor_plus)


def _fc_f32(v, w, b):
    from oracle import prims as P
    t = np.broadcast_to(b, (v.shape[0], len(b))).astype(np.float32)
    for c in range(w.shape[1]):
        t = P.fmaf(w[:, c], v[:, c:c + 1], t)
    return t


def gate_g_f32(streams, w1, b1, w2, b2, divisor_plus=0):
    """the gates [n, 4, C] as the kernel computes them: means, fc1 + ReLU, fc2, oracle.prims.sigmoid (the C restatement of d_sigmoidf)"""
    from oracle import prims as P
    c, c_real = streams[0].shape[-1], w1.shape[1]
    g = np.zeros((streams[0].shape[0], 4, c), np.float32)
    for k, s in enumerate(streams):
        hid = np.maximum(_fc_f32(_mean_f32(s, divisor_plus)[:, :c_real], w1, b1), np.float32(0))
        g[:, k, :c_real] = P.sigmoid(_fc_f32(hid, w2, b2))
    return g


def head_f32(x, w, b):
    return np.maximum(_fc_f32(_mean_f32(x), w, b), np.float32(0))


def crop_f32(frame_bgr, rect, oh, ow):
    """frame[y1:y2, x1:x2] -> cv2.resize(INTER_LINEAR) -> RGB -> / 255 -> (v - mean) / std, the three float32 operations of oracle.reid.prepare_crop"""
    from oracle import prims as P
    x1, y1, x2, y2 = rect
    c = P.resize_linear_u8c3(np.ascontiguousarray(frame_bgr[y1:y2, x1:x2]), oh, ow)[:, :, ::-1].astype(np.float32)
    return ((c / np.float32(255.0) - MEAN) / STD).astype(np.float32)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def frames(fh, fw, nf=2):
    return np.random.default_rng(fh * 10007 + fw).integers(0, 256, (nf, fh, fw, 3), dtype=np.uint8)


def crop_cases(fh, fw, oh, ow, nf=2):
    """-> (accepted [(name, (frame, x1, y1, x2, y2))], rejected [...]) for an fh x fw clip of nf frames and an oh x ow output"""
    ok = [("full frame", (0, 0, 0, fw, fh)), ("one pixel wide", (1, fw // 2, 3, fw // 2 + 1, fh - 2)), ("one pixel high", (0, 2, fh // 2, fw - 3, fh // 2 + 1)),
          ("touches left", (1, 0, 5, 9, 30)), ("touches top", (0, 7, 0, 20, 11)), ("touches bottom", (1, 4, fh - 13, 17, fh)),
          ("touches right, x2 == fw", (0, fw - 11, 6, fw, 40)), ("interior", (1, 10, 20, 47, 90))]
    if 2 * ow <= fw - 3 and 2 * oh <= fh - 5:
        ok.append(("exact 2x of the output", (1, 3, 5, 3 + 2 * ow, 5 + 2 * oh)))
    bad = [("frame -1", (-1, 0, 0, 10, 10)), ("frame == nf", (nf, 0, 0, 10, 10)), ("x1 < 0", (0, -1, 0, 10, 10)), ("y2 > fh", (0, 0, 0, 10, fh + 1)),
           ("empty", (0, 5, 5, 5, 20)), ("inverted", (1, 20, 5, 10, 30))]
    return ok, bad


CONV7_SIZES = [(1, 1), (2, 3), (8, 5), (9, 6), (256, 128)]
MAPS = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 7), (64, 32)]
CHANNELS = {16: 16, 32: 24, 128: 100}              # padded -> real channel count (padding channels carry zero weights / bias)
NS = (1, 3)
GATE_CFGS = [(16, 16, 1), (32, 24, 1), (32, 32, 2), (64, 50, 4), (128, 100, 8)]          # (C, c_real, r)
GATE_MAPS = [(1, 1), (1, 5), (16, 8), (64, 32)]
HEAD_CS, HEAD_MAPS, HEAD_DIMS = (16, 128), [(1, 1), (3, 5), (16, 8)], (512, 300, 1)
SLICE_IN, SLICE_OUT = (16, 8), (4, 4)              # (cs - c, off) of the slice cases' inputs / outputs


def _seed(*k):
    return [int(v) for v in k]


def conv7_case(n, h, w, ones=False):
    if ones:
        return np.ones((n, h, w, 4), np.float32), np.ones((7, 7, 3, 16), np.float32), np.zeros(16, np.float32)
    x = tensor(_seed(7, n, h, w), (n, h, w, 4))
    return x, weights(_seed(70, n, h, w), (7, 7, 3, 16), 0.2), weights(_seed(71, n, h, w), (16,), 0.3)


def tap_counts(h, w, ks, stride, pad):
    """[ho, wo] number of in-bounds taps of a ks x ks window"""
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    cy = np.array([sum(0 <= o * stride - pad + k < h for k in range(ks)) for o in range(ho)])
    cx = np.array([sum(0 <= o * stride - pad + k < w for k in range(ks)) for o in range(wo)])
    return cy[:, None] * cx[None, :]


def pool_case(n, h, w, c):
    """input with channel 1 strictly negative everywhere: a pool that pads with 0 instead of -inf / 'skip' is wrong there"""
    return tensor(_seed(3, n, h, w, c), (n, h, w, c), neg_channel=1)


def dw3_case(n, h, w, c, ones=False):
    if ones:
        return np.ones((n, h, w, c), np.float32), np.ones((9, c), np.float32), np.zeros(c, np.float32)
    x = tensor(_seed(9, n, h, w, c), (n, h, w, c))
    wt, b = weights(_seed(90, n, h, w, c), (9, c)), weights(_seed(91, n, h, w, c), (c,), 0.3)
    wt[:, CHANNELS[c]:] = 0.0; b[CHANNELS[c]:] = 0.0
    return x, wt, b


def gate_case(n, h, w, c, c_real, r, pad_value=0.0):
    """four distinct streams (post-ReLU like the network's: non-negative with exact zeros, different scales), padding channels = pad_value"""
    streams = []
    for k in range(4):
        s = np.maximum(tensor(_seed(5, n, h, w, c, c_real, r, k), (n, h, w, c)) + np.float32(0.3 * k), np.float32(0)) * np.float32(1.0 + 0.5 * k)
        s[..., c_real:] = pad_value
        streams.append(s)
    sd = _seed(50, c, c_real, r)
    w1 = weights(sd + [1], (r, c_real), math.sqrt(2.0 / c_real))
    w1[0] = np.abs(w1[0])                              # hidden unit 0 is active for every stream (the means are positive): the gates depend on the means
    return (streams, w1, weights(sd + [2], (r,), 0.1),
            weights(sd + [3], (c_real, r), math.sqrt(2.0 / r)), weights(sd + [4], (c_real,), 0.5))


def head_case(n, h, w, c, dim):
    x = np.maximum(tensor(_seed(11, n, h, w, c), (n, h, w, c)), np.float32(0))
    return x, weights(_seed(110, c, dim), (dim, c), math.sqrt(2.0 / c)), weights(_seed(111, c, dim), (dim,), 0.1)


def unslice(whole, c, off):
    """the slice [.., off:off + c] of a buffer returned whole; asserts the sentinel everywhere else and no NaN inside"""
    bits = np.ascontiguousarray(whole).view(np.uint32)
    outside = np.ones(whole.shape[-1], bool)
    outside[off:off + c] = False
    assert (bits[..., outside] == SENTINEL).all(), "a sentinel outside the output slice was overwritten"
    y = whole[..., off:off + c]
    assert not np.isnan(y).any(), "NaN inside the output slice: the kernel read outside an input slice, or left an element unwritten"
    return y


# ---- the composed float64 network (ties the per-operator references to oracle.reid.embed) ---------------------------------------------------
def _fold(sd, bn, c):
    g, b, m, v = (np.asarray(sd["reid." + bn + k], np.float64) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    sc = g / np.sqrt(v + 1e-5)
    return sc[:c], (b - m * sc)[:c]


def _conv1x1_64(sd, x, name, bn, relu):
    w = np.asarray(sd["reid." + name + ".weight"], np.float64)[:, :, 0, 0]
    y = x @ w.T
    if bn:
        sc, sh = _fold(sd, bn, w.shape[0])
        y = y * sc + sh
    return np.maximum(y, 0.0) if relu else y


def _light64(sd, x, lc):
    t = _conv1x1_64(sd, x, lc + ".conv1", None, False)
    mid = t.shape[-1]
    sc, sh = _fold(sd, lc + ".bn", mid)
    w = (np.asarray(sd["reid." + lc + ".conv2.weight"], np.float64).reshape(mid, 9) * sc[:, None]).T          # [9, mid], BatchNorm folded
    return dw3_ref(t, w, sh)[0]


def embed64(sd, crops):
    """OSNet-x0.25 per eagle_amd/osnet.py's table through the float64 references of this module: crops [n, 256, 128, 3] -> [n, 512]"""
    from eagle_amd import osnet
    n = len(crops)
    x = np.concatenate([np.asarray(crops, np.float64), np.zeros((n, 256, 128, 1))], -1)
    sc, sh = _fold(sd, "conv1.bn", 16)
    w = np.asarray(sd["reid.conv1.conv.weight"], np.float64).transpose(2, 3, 1, 0) * sc            # [16, 3, 7, 7] -> [7, 7, 3, 16]
    x = _maxpool64(conv7_ref(x, w, sh)[0])
    for i, (name, cin, cout) in enumerate(osnet.blocks()):
        x1 = _conv1x1_64(sd, x, name + ".conv1.conv", name + ".conv1.bn", True)
        streams = [_light64(sd, x1, name + ".conv2a")]
        for s, depth in (("b", 2), ("c", 3), ("d", 4)):
            y = x1
            for k in range(depth):
                y = _light64(sd, y, f"{name}.conv2{s}.{k}")
            streams.append(y)
        gw = [np.asarray(sd[f"reid.{name}.gate.{k}"], np.float64) for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")]
        _, _, g = gate_ref(streams, gw[0][:, :, 0, 0], gw[1], gw[2][:, :, 0, 0], gw[3])
        x2 = sum(streams[k] * g[:, k, None, None, :] for k in range(4))
        x3 = _conv1x1_64(sd, x2, name + ".conv3.conv", name + ".conv3.bn", False)
        ident = _conv1x1_64(sd, x, name + ".downsample.conv", name + ".downsample.bn", False) if cin != cout else x
        x = np.maximum(x3 + ident, 0.0)
        if i in (1, 3):
            t = _conv1x1_64(sd, x, name[:5] + ".2.0.conv", name[:5] + ".2.0.bn", True)
            m, h, wd, c = t.shape
            v = t.reshape(m, h // 2, 2, wd // 2, 2, c)
            x = ((v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + (v[:, :, 1, :, 0] + v[:, :, 1, :, 1])) * 0.25
    x = _conv1x1_64(sd, x, "conv5.conv", "conv5.bn", True)
    sc, sh = _fold(sd, "fc.1", 512)
    fw, fb = np.asarray(sd["reid.fc.0.weight"], np.float64), np.asarray(sd["reid.fc.0.bias"], np.float64)
    return head_ref(x, fw * sc[:, None], fb * sc + sh)[0]


def _maxpool64(x):
    n, h, wd, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    m = np.full((n, ho, wo, c), -np.inf)
    for _, win in _taps(x, 3, 2, 1, ho, wo, -np.inf):
        m = np.maximum(m, win)
    return m
