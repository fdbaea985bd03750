// The output writer of the kernels that produce pictures (annotate.hip K19, minimap.hip K21): a thread's 2-row strip of AN_STRIP pixels, held in
// registers as B | G << 8 | R << 16, -> BGR, NV12 or I420 in the caller's layout.  Three 8-byte BGR stores per row, or 8-byte stores of Y per row + 8
// bytes of UV (NV12) or 4 + 4 bytes of U and V (I420); tail strips and addresses without the alignment go byte by byte.  BGR -> 4:2:0 is OpenCV's
// integer BT.601 limited-range path of COLOR_BGR2YUV_I420 (tests/annot_ref.py), chroma from the even-row even-column pixel of each 2 x 2 block.
#pragma once
#include "common.h"

namespace eagle {

static constexpr int AN_STRIP = 8, AN_TW = 256, AN_TH = 16;
static constexpr int AN_SX = AN_TW / AN_STRIP, AN_THREADS = AN_SX * (AN_TH / 2);      // 32 strips x 8 row pairs = 256 threads
// OpenCV's BGR -> YUV 4:2:0 coefficients (color_yuv.simd.hpp), 20-bit fixed point
static constexpr int AN_SHIFT = 20, AN_RY = 269484, AN_GY = 528482, AN_BY = 102760, AN_RU = -155188, AN_GU = -305135, AN_BU = 460324,
                     AN_RV = 460324, AN_GV = -385875, AN_BV = -74448;


__device__ __forceinline__ void pack8(const uint32_t* px, uint32_t* w)
{
    #pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t* p = px + 4 * q;
        w[3 * q] = p[0] | p[1] << 24; w[3 * q + 1] = p[1] >> 8 | p[2] << 16; w[3 * q + 2] = p[2] >> 16 | p[3] << 8;
    }
}
__device__ __forceinline__ uint32_t luma(uint32_t p)
{
    const int b = p & 255, g = (p >> 8) & 255, r = (p >> 16) & 255;
    return (uint32_t)((AN_RY * r + AN_GY * g + AN_BY * b + (16 << AN_SHIFT) + (1 << (AN_SHIFT - 1))) >> AN_SHIFT);
}
__device__ __forceinline__ void chroma(uint32_t p, uint32_t& u, uint32_t& v)
{
    const int b = p & 255, g = (p >> 8) & 255, r = (p >> 16) & 255;
    u = (uint32_t)((AN_RU * r + AN_GU * g + AN_BU * b + (128 << AN_SHIFT) + (1 << (AN_SHIFT - 1))) >> AN_SHIFT);
    v = (uint32_t)((AN_RV * r + AN_GV * g + AN_BV * b + (128 << AN_SHIFT) + (1 << (AN_SHIFT - 1))) >> AN_SHIFT);
}

// the strip at (x0, y0) of output frame f: cnt valid pixels per row (4:2:0: even), rows valid rows (4:2:0: 2)
__device__ __forceinline__ void write_strip(const AnnotArgs& a, int f, int x0, int y0, int cnt, int rows, const uint32_t (&px)[2][AN_STRIP])
{
    uint8_t* fr = a.dst + (int64_t)f * a.frame_stride;
    if (a.fmt == EAGLE_PIX_BGR) {
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= rows) continue;
            uint8_t* d = fr + (int64_t)(y0 + r) * a.y_pitch + (int64_t)x0 * 3;
            const uintptr_t da = (uintptr_t)d;
            if (cnt == AN_STRIP && (da & 3) == 0) {
                uint32_t w[6];
                pack8(px[r], w);
                if ((da & 7) == 0) {
                    uint2* o = (uint2*)d;
                    o[0] = make_uint2(w[0], w[1]); o[1] = make_uint2(w[2], w[3]); o[2] = make_uint2(w[4], w[5]);
                } else {
                    #pragma unroll
                    for (int k = 0; k < 6; ++k) ((uint32_t*)d)[k] = w[k];
                }
            } else {
                #pragma unroll
                for (int k = 0; k < AN_STRIP; ++k)
                    if (k < cnt) { d[3 * k] = (uint8_t)px[r][k]; d[3 * k + 1] = (uint8_t)(px[r][k] >> 8); d[3 * k + 2] = (uint8_t)(px[r][k] >> 16); }
            }
        }
        return;
    }
    uint32_t u[AN_STRIP / 2], v[AN_STRIP / 2];
    #pragma unroll
    for (int k = 0; k < AN_STRIP / 2; ++k) chroma(px[0][2 * k], u[k], v[k]);        // the even-row, even-column pixel of each 2 x 2 block
    const int64_t crow = (int64_t)(y0 >> 1) * a.c_pitch + (int64_t)(x0 >> 1) * a.c_step;
    uint8_t* up = fr + a.c_offset + crow;
    uint8_t* vp = fr + a.v_offset + crow;
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint8_t* d = fr + (int64_t)(y0 + r) * a.y_pitch + x0;
        uint32_t y[AN_STRIP];
        #pragma unroll
        for (int k = 0; k < AN_STRIP; ++k) y[k] = luma(px[r][k]);
        if (cnt == AN_STRIP && a.vec) {
            *(uint2*)d = make_uint2(y[0] | y[1] << 8 | y[2] << 16 | y[3] << 24, y[4] | y[5] << 8 | y[6] << 16 | y[7] << 24);
        } else {
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k) if (k < cnt) d[k] = (uint8_t)y[k];
        }
    }
    if (cnt == AN_STRIP && a.vec) {
        if (a.c_step == 2) {
            *(uint2*)up = make_uint2(u[0] | v[0] << 8 | u[1] << 16 | v[1] << 24, u[2] | v[2] << 8 | u[3] << 16 | v[3] << 24);
        } else {
            *(uint32_t*)up = u[0] | u[1] << 8 | u[2] << 16 | u[3] << 24;
            *(uint32_t*)vp = v[0] | v[1] << 8 | v[2] << 16 | v[3] << 24;
        }
    } else {
        #pragma unroll
        for (int k = 0; k < AN_STRIP / 2; ++k)
            if (2 * k < cnt) { up[k * a.c_step] = (uint8_t)u[k]; vp[k * a.c_step] = (uint8_t)v[k]; }
    }
}

}  // namespace eagle
