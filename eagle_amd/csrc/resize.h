// cv2.resize(u8, INTER_LINEAR) restated for device code: half-pixel centres, 11-bit fixed-point taps, the exact 2x
// decimation handled as cv2 does (2 x 2 area average).  The ONE definition of that arithmetic: K1 (elementwise.hip), the player crops
// (reid.hip: explicit row stride, a sub-rectangle of a frame is the source) and HRNet's fused input kernel (stem.hip) all call it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace eagle {

struct ResizeTap { int s0, s1; int a0, a1; };

// scale = source pixels per destination pixel: ssize / dsize for cv2.resize(dsize), 1 / fx for cv2.resize((0, 0), fx, fy)
__device__ __forceinline__ ResizeTap resize_tap_scaled(int d, double scale, int ssize)
{
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= ssize - 1) { s = ssize - 1; f = 0.f; }
    ResizeTap r;
    r.s0 = s; r.s1 = (s + 1 < ssize) ? s + 1 : s;
    r.a0 = (int)(short)lrintf((1.f - f) * 2048.f);
    r.a1 = (int)(short)lrintf(f * 2048.f);
    return r;
}
__device__ __forceinline__ ResizeTap resize_tap(int d, int dsize, int ssize) { return resize_tap_scaled(d, (double)ssize / (double)dsize, ssize); }

// the general (two-tap) branch below applies; otherwise the resize is the identity or the exact 2x decimation and needs no taps
__device__ __forceinline__ bool resize_uses_taps(int sh, int sw, int dh, int dw) { return !(sh == dh && sw == dw) && !(sh == 2 * dh && sw == 2 * dw); }

// general branch with the taps of the pixel's column (ax) and row (ay) given: a kernel that resizes a tile computes each tap once per tile
__device__ __forceinline__ void resize_px_taps(const uint8_t* src, size_t rs, const ResizeTap& ax, const ResizeTap& ay, int rgb[3])
{
    const uint8_t* r0 = src + ay.s0 * rs; const uint8_t* r1 = src + ay.s1 * rs;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int t0 = r0[ax.s0 * 3 + c] * ax.a0 + r0[ax.s1 * 3 + c] * ax.a1;
        const int t1 = r1[ax.s0 * 3 + c] * ax.a0 + r1[ax.s1 * 3 + c] * ax.a1;
        rgb[2 - c] = (((ay.a0 * (t0 >> 4)) >> 16) + ((ay.a1 * (t1 >> 4)) >> 16) + 2) >> 2;
    }
}

// resized RGB u8 pixel (dy, dx) of an (sh, sw) -> (dh, dw) resize; src is BGR with `rs` bytes per row
__device__ __forceinline__ void resize_px_strided(const uint8_t* src, size_t rs, int sh, int sw, int dh, int dw, int dy, int dx, int rgb[3])
{
    if (sh == dh && sw == dw) {
        const uint8_t* p = src + dy * rs + dx * 3;
        rgb[0] = p[2]; rgb[1] = p[1]; rgb[2] = p[0];
    } else if (sh == 2 * dh && sw == 2 * dw) {
        const uint8_t* p = src + (size_t)(2 * dy) * rs + (size_t)(2 * dx) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[2 - c] = (p[c] + p[3 + c] + p[rs + c] + p[rs + 3 + c] + 2) >> 2;
    } else {
        resize_px_taps(src, rs, resize_tap(dx, dw, sw), resize_tap(dy, dh, sh), rgb);
    }
}

// A.Normalize of the key-point network's input (ImageNet mean / std on the 0..255 scale, coordinate_model.py:62-64) of one resized RGB u8 pixel
__device__ __forceinline__ void kp_normalize(const int rgb[3], float v[3])
{
    const float m0 = 0x1.eeb334p+6f, m1 = 0x1.d11eb8p+6f, m2 = 0x1.9e1eb8p+6f;      // f32(mean)*255
    const float s0 = 0x1.18926cp-6f, s1 = 0x1.1ed5bp-6f, s2 = 0x1.1d8f56p-6f;       // 1/(f32(std)*255)
    v[0] = ((float)rgb[0] - m0) * s0; v[1] = ((float)rgb[1] - m1) * s1; v[2] = ((float)rgb[2] - m2) * s2;
}

}  // namespace eagle
