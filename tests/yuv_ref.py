"""numpy restatement of the library's 4:2:0 -> BGR contract: cv2.cvtColor(yuv, COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420) of OpenCV 4.x.

The arithmetic is OpenCV's integer path, modules/imgproc/src/color_yuv.simd.hpp (ITUR_BT_601_* constants): BT.601 limited range in 20-bit fixed
point, one chroma sample per 2x2 pixel block (no interpolation):
    uu = U - 128, vv = V - 128
    ruv = 2^19 + 1673527 vv,  guv = 2^19 - 852492 vv - 409993 uu,  buv = 2^19 + 2116026 uu
    y = max(0, Y - 16) * 1220542
    R = sat_u8((y + ruv) >> 20), G = sat_u8((y + guv) >> 20), B = sat_u8((y + buv) >> 20)
cv2 cannot be imported where this was written: the constants are taken from the OpenCV source, not from a run of cv2.  Two anchors hold
whatever the constants are: (Y, U, V) = (16, 128, 128) -> (0, 0, 0) and (235, 128, 128) -> (255, 255, 255) (tests/test_yuv_cpu.py).

This is the oracle of tests/test_gpu_yuv.py; it reads any layout of include/eagle.h's EagleYuvLayout (byte offsets and pitches)."""
import numpy as np

SHIFT, CY, CUB, CUG, CVG, CVR = 20, 1220542, 2116026, -409993, -852492, 1673527
NV12, I420 = "nv12", "i420"


def dense_layout(fmt, h, w):
    """The dense defaults of include/eagle.h for h x w frames: dict of frame_stride, y_pitch, c_offset, c_pitch, v_offset (v_offset: I420 only, 0 for NV12)."""
    c_pitch = w if fmt == NV12 else w // 2
    c_offset = w * h
    v_offset = 0 if fmt == NV12 else c_offset + c_pitch * (h // 2)
    frame_stride = c_offset + c_pitch * (h // 2) if fmt == NV12 else v_offset + c_pitch * (h // 2)
    return {"frame_stride": frame_stride, "y_pitch": w, "c_offset": c_offset, "c_pitch": c_pitch, "v_offset": v_offset}


def resolve(fmt, h, w, layout=None):
    """layout with zero / missing fields replaced by the dense defaults (frame_stride = the end of the last plane)."""
    lay = dict(layout or {})
    c_row = w if fmt == NV12 else w // 2
    y_pitch = lay.get("y_pitch") or w
    c_offset = lay.get("c_offset") or y_pitch * h
    c_pitch = lay.get("c_pitch") or c_row
    v_offset = 0 if fmt == NV12 else (lay.get("v_offset") or c_offset + c_pitch * (h // 2))
    ends = [y_pitch * h, c_offset + c_pitch * (h // 2)] + ([] if fmt == NV12 else [v_offset + c_pitch * (h // 2)])
    return {"frame_stride": lay.get("frame_stride") or max(ends), "y_pitch": y_pitch, "c_offset": c_offset, "c_pitch": c_pitch, "v_offset": v_offset}


def planes(fmt, buf, n, h, w, layout=None):
    """-> Y [n, h, w], U [n, h/2, w/2], V [n, h/2, w/2] (int32) read from a flat uint8 buffer with the given layout."""
    L = resolve(fmt, h, w, layout)
    buf = np.ascontiguousarray(buf, np.uint8).reshape(-1)
    Y = np.empty((n, h, w), np.int32)
    U = np.empty((n, h // 2, w // 2), np.int32)
    V = np.empty_like(U)
    for k in range(n):
        f = k * L["frame_stride"]
        for r in range(h):
            Y[k, r] = buf[f + r * L["y_pitch"]: f + r * L["y_pitch"] + w]
        for r in range(h // 2):
            c = f + L["c_offset"] + r * L["c_pitch"]
            if fmt == NV12:
                row = buf[c: c + w]
                U[k, r], V[k, r] = row[0::2], row[1::2]
            else:
                v = f + L["v_offset"] + r * L["c_pitch"]
                U[k, r], V[k, r] = buf[c: c + w // 2], buf[v: v + w // 2]
    return Y, U, V


def planes_to_bgr(Y, U, V):
    """Y [n, h, w], U / V [n, h/2, w/2] -> BGR uint8 [n, h, w, 3] by OpenCV's integer formula."""
    Y, U, V = (np.asarray(a, np.int64) for a in (Y, U, V))
    uu = np.repeat(np.repeat(U - 128, 2, -1), 2, -2)
    vv = np.repeat(np.repeat(V - 128, 2, -1), 2, -2)
    half = 1 << (SHIFT - 1)
    ruv, guv, buv = half + CVR * vv, half + CVG * vv + CUG * uu, half + CUB * uu
    y = np.maximum(Y - 16, 0) * CY
    sat = lambda a: np.clip(a >> SHIFT, 0, 255).astype(np.uint8)
    return np.stack([sat(y + buv), sat(y + guv), sat(y + ruv)], -1)


def to_bgr(fmt, frames, layout=None, h=None, w=None, n=None):
    """cv2's conversion of uint8 [n, 3h/2, w] / [3h/2, w] frames, or of a flat buffer with layout, h, w and n -> BGR [n, h, w, 3]."""
    a = np.asarray(frames, np.uint8)
    if a.ndim in (2, 3):
        if a.ndim == 2:
            a = a[None]
        n, h, w = a.shape[0], a.shape[1] * 2 // 3, a.shape[2]
    return planes_to_bgr(*planes(fmt, a, n, h, w, layout))


def nv12_to_bgr(frames, layout=None, h=None, w=None, n=None):
    return to_bgr(NV12, frames, layout, h, w, n)


def i420_to_bgr(frames, layout=None, h=None, w=None, n=None):
    return to_bgr(I420, frames, layout, h, w, n)


def pack(fmt, Y, U, V, layout=None, fill=0):
    """Y [n, h, w], U / V [n, h/2, w/2] -> a flat uint8 buffer in the given layout (padding bytes = fill): synthetic decoder surfaces."""
    n, h, w = Y.shape
    L = resolve(fmt, h, w, layout)
    ends = [L["y_pitch"] * (h - 1) + w, L["c_offset"] + L["c_pitch"] * (h // 2 - 1) + (w if fmt == NV12 else w // 2)]
    if fmt == I420:
        ends.append(L["v_offset"] + L["c_pitch"] * (h // 2 - 1) + w // 2)
    buf = np.full((n - 1) * L["frame_stride"] + max(ends), fill, np.uint8)
    for k in range(n):
        f = k * L["frame_stride"]
        for r in range(h):
            buf[f + r * L["y_pitch"]: f + r * L["y_pitch"] + w] = Y[k, r]
        for r in range(h // 2):
            c = f + L["c_offset"] + r * L["c_pitch"]
            if fmt == NV12:
                buf[c: c + w: 2], buf[c + 1: c + w: 2] = U[k, r], V[k, r]
            else:
                v = f + L["v_offset"] + r * L["c_pitch"]
                buf[c: c + w // 2], buf[v: v + w // 2] = U[k, r], V[k, r]
    return buf


def split(fmt, frames):
    """uint8 [n, 3h/2, w] (cv2 convention) -> Y, U, V planes (int32)."""
    a = np.asarray(frames, np.uint8)
    if a.ndim == 2:
        a = a[None]
    n, h, w = a.shape[0], a.shape[1] * 2 // 3, a.shape[2]
    return planes(fmt, a, n, h, w)
