// K18 — decoder-native input: 4:2:0 frames (NV12 from hardware decoders, I420 from software decoders) -> dense BGR [n, h, w, 3], the layout
// every other kernel of the library reads.  The conversion is OpenCV 4.x's integer path (modules/imgproc/src/color_yuv.simd.hpp,
// cv::COLOR_YUV2BGR_NV12 / _I420): BT.601 limited range in 20-bit fixed point, one chroma sample per 2x2 pixel block, no chroma interpolation.
// Every output byte equals what cv2.cvtColor produces, so every record computed from the converted frame equals the BGR call's.
//
// One thread owns a 2-row strip of YUV_STRIP pixels: its YUV_STRIP / 2 chroma samples are loaded once and serve both rows.  Neighbouring
// lanes own neighbouring strips of the same row pair, so each load and store instruction of a wave covers one contiguous span.  Interior
// strips use 8-byte Y / NV12-chroma loads, 4-byte I420-chroma loads and three 8-byte stores per row whenever the addresses allow it (the
// host reports the source's alignment; the destination row is checked per thread); the tail strip of a row whose width is not a multiple
// of YUV_STRIP, and sources of odd alignment, go byte by byte.  Integer arithmetic only.
#include "common.h"

namespace eagle {

static constexpr int YUV_STRIP = 8;       // pixels per thread and row

// OpenCV's ITUR_BT_601_* constants (color_yuv.simd.hpp)
static constexpr int YUV_SHIFT = 20, YUV_CY = 1220542, YUV_CUB = 2116026, YUV_CUG = -409993, YUV_CVG = -852492, YUV_CVR = 1673527;

__device__ __forceinline__ uint32_t sat_u8(int v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

struct ChromaTerms { int r, g, b; };
__device__ __forceinline__ ChromaTerms chroma_terms(int u, int v)
{
    const int uu = u - 128, vv = v - 128, half = 1 << (YUV_SHIFT - 1);
    return {half + YUV_CVR * vv, half + YUV_CVG * vv + YUV_CUG * uu, half + YUV_CUB * uu};
}
// B | G << 8 | R << 16 of one pixel
__device__ __forceinline__ uint32_t yuv_px(int y, const ChromaTerms& c)
{
    const int yy = max(0, y - 16) * YUV_CY;
    return sat_u8((yy + c.b) >> YUV_SHIFT) | sat_u8((yy + c.g) >> YUV_SHIFT) << 8 | sat_u8((yy + c.r) >> YUV_SHIFT) << 16;
}

__global__ __launch_bounds__(256) void yuv_to_bgr_kernel(YuvArgs a)
{
    const int strips = (a.w + YUV_STRIP - 1) / YUV_STRIP;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= strips * (a.h >> 1)) return;
    const int f = blockIdx.y, rp = t / strips, x0 = (t - rp * strips) * YUV_STRIP;
    const int cnt = min(YUV_STRIP, a.w - x0);       // even: w is even
    const uint8_t* fr = a.src + (int64_t)f * a.frame_stride;
    const uint8_t* yr[2] = {fr + (int64_t)(2 * rp) * a.y_pitch + x0, fr + (int64_t)(2 * rp + 1) * a.y_pitch + x0};
    const int64_t crow = (int64_t)rp * a.c_pitch;
    const uint8_t* up = fr + a.c_offset + crow + (int64_t)(x0 >> 1) * a.c_step;     // NV12: U V U V ...; I420: U U ... and V V ...
    const uint8_t* vp = fr + a.v_offset + crow + (int64_t)(x0 >> 1) * a.c_step;     // (NV12: v_offset = c_offset + 1)
    uint8_t* out[2] = {a.dst + (((int64_t)f * a.h + 2 * rp) * a.w + x0) * 3, a.dst + (((int64_t)f * a.h + 2 * rp + 1) * a.w + x0) * 3};

    if (cnt == YUV_STRIP && a.vec) {
        ChromaTerms c[YUV_STRIP / 2];
        if (a.c_step == 2) {
            const uint2 uv = *(const uint2*)up;
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t wd = k < 2 ? uv.x : uv.y, s = (k & 1) * 16;
                c[k] = chroma_terms((wd >> s) & 255, (wd >> (s + 8)) & 255);
            }
        } else {
            const uint32_t u4 = *(const uint32_t*)up, v4 = *(const uint32_t*)vp;
            #pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = chroma_terms((u4 >> (8 * k)) & 255, (v4 >> (8 * k)) & 255);
        }
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint2 y8 = *(const uint2*)yr[r];
            uint32_t px[YUV_STRIP];
            #pragma unroll
            for (int k = 0; k < YUV_STRIP; ++k) px[k] = yuv_px(((k < 4 ? y8.x : y8.y) >> (8 * (k & 3))) & 255, c[k >> 1]);
            // 8 pixels = 24 bytes = 6 little-endian words
            const uint32_t w0 = px[0] | px[1] << 24, w1 = px[1] >> 8 | px[2] << 16, w2 = px[2] >> 16 | px[3] << 8;
            const uint32_t w3 = px[4] | px[5] << 24, w4 = px[5] >> 8 | px[6] << 16, w5 = px[6] >> 16 | px[7] << 8;
            const uintptr_t o = (uintptr_t)out[r];
            if ((o & 7) == 0) {
                uint2* d = (uint2*)out[r];
                d[0] = make_uint2(w0, w1); d[1] = make_uint2(w2, w3); d[2] = make_uint2(w4, w5);
            } else if ((o & 3) == 0) {
                uint32_t* d = (uint32_t*)out[r];
                d[0] = w0; d[1] = w1; d[2] = w2; d[3] = w3; d[4] = w4; d[5] = w5;
            } else {
                const uint32_t ws[6] = {w0, w1, w2, w3, w4, w5};
                if ((o & 1) == 0) {                     // w is even: every row starts on an even byte when dst does
                    uint16_t* d = (uint16_t*)out[r];
                    #pragma unroll
                    for (int k = 0; k < 6; ++k) { d[2 * k] = (uint16_t)ws[k]; d[2 * k + 1] = (uint16_t)(ws[k] >> 16); }
                } else {
                    #pragma unroll
                    for (int k = 0; k < 24; ++k) out[r][k] = (uint8_t)(ws[k >> 2] >> (8 * (k & 3)));
                }
            }
        }
        return;
    }
    // tail strip (cnt < YUV_STRIP) or a source without the alignment of the vector path
    for (int k = 0; k < cnt; k += 2) {
        const ChromaTerms c = chroma_terms(up[(k >> 1) * a.c_step], vp[(k >> 1) * a.c_step]);
        #pragma unroll
        for (int r = 0; r < 2; ++r)
            #pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t p = yuv_px(yr[r][k + j], c);
                uint8_t* d = out[r] + 3 * (k + j);
                d[0] = (uint8_t)p; d[1] = (uint8_t)(p >> 8); d[2] = (uint8_t)(p >> 16);
            }
    }
}

void yuv_to_bgr_launch(const YuvArgs& args, int n, hipStream_t s)
{
    if (n <= 0) return;
    YuvArgs a = args;
    const int per_frame = (a.w + YUV_STRIP - 1) / YUV_STRIP * (a.h >> 1);
    const int64_t fb = (int64_t)a.h * a.w * 3;
    for (int f0 = 0; f0 < n; f0 += 65535) {          // gridDim.y limit
        const int nf = std::min(n - f0, 65535);
        hipLaunchKernelGGL(yuv_to_bgr_kernel, dim3((per_frame + 255) / 256, nf), dim3(256), 0, s, a);
        HIP_CHECK(hipGetLastError());
        a.src += (int64_t)nf * a.frame_stride;
        a.dst += (int64_t)nf * fb;
    }
}

}  // namespace eagle
