// Fused input path of HRNet for the split-precision family (EAGLE_PREC_F32S): BGR u8 frame -> conv1 output, no key-point input tensor.
//
// Replaces the key-point half of K1 (cv2.resize to 540 x 960 + A.Normalize, written as 8-lane split pixels of which 5 lanes are zeros) and the
// generic launch of conv1 (3 x 3 / 2, 3 -> 64, BatchNorm folded, ReLU; eagle/models/keypoint_hrnet.py:315-321) by ONE kernel that reads the
// frame and writes conv1's output.  Unfused, at B = 50, the 540 x 960 x 8-lane tensor is 0.83 GB written and 0.83 GB read again, and conv1
// spends three K = 32 MFMA steps per product on 27 real values; here the resized pixels never leave the CU and K is the 27 (tap, channel)
// values padded to 32.
//
// Workgroup = 4 waves, tile = 8 rows x 32 columns of conv1 output pixels of one frame.
//   phase 0  the resize taps of the tile's 17 input rows and 65 input columns, once each (resize.h: the arithmetic of K1, one definition)
//   phase 1  the 17 x 65 input window: resized, normalised, split -> LDS records of 16 bytes [hi c0 c1 c2 0][lo c0 c1 c2 0]; ZEROS outside the
//            540 x 960 map (conv1's padding).  Even and odd window columns lie in separate planes, so that the 32 pixels of a stride-2 B fragment are
//            32 consecutive records (conflict-free ds_read_b128)
//   phase 2  wave w owns output rows 2 w and 2 w + 1 (one 32-pixel block each, all 64 channels): per block two K steps of v_mfma_f32_32x32x16_f16,
//            three products each (Whi Xhi + Whi Xlo + Wlo Xhi).  A lane's 8 K slots of a step are two taps' records (c0 c1 c2 + one spare slot each);
//            taps 0 .. 7 fill the four (step, k-group) fragments, the three values of tap 8 ride in spare slots (stem_tile_weights places the weights to match)
//   barrier  the strips of the epilogue take the window's place (36 KB of LDS per workgroup: four workgroups per CU)
//   epilogue relu(acc * descale + bias), the family's saturating split (counted per frame like every other launch), transposed through a wave-private
//            LDS strip: 16 bytes per lane, the 32 pixels of a block are 8 KiB of contiguous memory; non-temporal like the other split-family stores
// Numerics: the three-product split scheme, power-of-two weight scaling and fp32 accumulation of the family's other kernels; against the generic
// launches only the order of the 27 products inside an accumulator differs.  Same kernel and tile order at every batch size.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "dmath.h"
#include "conv_internal.h"
#include "resize.h"

namespace eagle {

#include "conv_kernels.inc"

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int ST_TH = 8, ST_TW = 32;                                  // tile of output pixels
constexpr int ST_WH = 2 * ST_TH + 1, ST_WW = 2 * ST_TW + 1;           // input window 17 x 65
constexpr int ST_HC = ST_TW + 1;                                      // records per column plane of a window row (even columns: 33, odd: 32 used)
constexpr int ST_WIN = ST_WH * 2 * ST_HC * 16;                        // window bytes
constexpr int ST_TPS = 272, ST_STRIP = 32 * ST_TPS;                   // epilogue strip: 256-byte pixel records + 16 (pixel stride = 4 banks mod 64)
constexpr int ST_TAPS = (ST_WH + ST_WW) * (int)sizeof(ResizeTap);
constexpr int ST_REG = ST_WIN > 4 * ST_STRIP ? ST_WIN : 4 * ST_STRIP;   // the window, then (behind a barrier) the four strips
constexpr int ST_LDS = ST_REG + ST_TAPS;                              // 36 KB: four workgroups per CU
constexpr int ST_PI = (ST_WH * ST_WW + 255) / 256;                    // window pixels per thread
static_assert(sizeof(ResizeTap) == 16 && ST_LDS <= 64 * 1024, "stem geometry");

struct StemArgs {
    const uint8_t* bgr; int n, sh, sw;        // dense BGR u8 frames [n, sh, sw, 3]
    int dh, dw;                               // the resized map conv1 reads (540 x 960 in the pipeline)
    const void* w; const float* bias; float descale;
    void* y; int ycs, yoff; unsigned ybytes;  // conv1 output [n, ho, wo, 64] split; channel stride / offset in fp16 elements; bytes of the whole buffer
    int ho, wo, tiles_x, tiles_y;
    unsigned* sat;
};

__device__ __forceinline__ void stem_split4(float v0, float v1, float v2, float v3, half4& hi, half4& lo)
{
    const float s0 = __builtin_amdgcn_fmed3f(v0 * SPLIT_SX, -65504.0f, 65504.0f), s1 = __builtin_amdgcn_fmed3f(v1 * SPLIT_SX, -65504.0f, 65504.0f),
                s2 = __builtin_amdgcn_fmed3f(v2 * SPLIT_SX, -65504.0f, 65504.0f), s3 = __builtin_amdgcn_fmed3f(v3 * SPLIT_SX, -65504.0f, 65504.0f);
    hi = half4{(_Float16)s0, (_Float16)s1, (_Float16)s2, (_Float16)s3};
    lo = half4{(_Float16)(s0 - (float)hi[0]), (_Float16)(s1 - (float)hi[1]), (_Float16)(s2 - (float)hi[2]), (_Float16)(s3 - (float)hi[3])};
}

// byte offset of window pixel (wy, wx) inside the window
__device__ __forceinline__ int stem_rec(int wy, int wx) { return ((wy * 2 + (wx & 1)) * ST_HC + (wx >> 1)) * 16; }

__global__ __launch_bounds__(256, 4) void stem_split_kernel(StemArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const win = smem;
    ResizeTap* const taps = (ResizeTap*)(smem + ST_REG);      // [0, ST_WH): rows, [ST_WH, ST_WH + ST_WW): columns
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = lane >> 5, lx = lane & 31;
    char* const strip = smem + wave * ST_STRIP;
    int t = blockIdx.x;
    const int tx = t % a.tiles_x; t /= a.tiles_x;
    const int ty = t % a.tiles_y, n = t / a.tiles_y;
    const int oy0 = ty * ST_TH, ox0 = tx * ST_TW;
    const int iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - 1;                    // input pixel of window (0, 0)

    // weight image [K step][hi | lo][channel block][lane][8] and the lane's biases: requested first, they travel under phases 0 / 1
    u32x4 A[2][2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int pt = 0; pt < 2; ++pt)
#pragma unroll
            for (int m = 0; m < 2; ++m) A[s][pt][m] = *(const u32x4*)((const char*)a.w + (((s * 2 + pt) * 2 + m) * 64 + lane) * 16);

    // ---- phase 0: taps of the window's rows and columns (general resize only) ----
    const bool use_taps = resize_uses_taps(a.sh, a.sw, a.dh, a.dw);
    if (use_taps && tid < ST_WH + ST_WW) {
        const bool row = tid < ST_WH;
        const int d = row ? iy0 + tid : ix0 + (tid - ST_WH), ds = row ? a.dh : a.dw, ss = row ? a.sh : a.sw;
        if (d >= 0 && d < ds) taps[tid] = resize_tap(d, ds, ss);
    }
    __syncthreads();
    // ---- phase 1: the input window ----
    // A thread's ST_PI pixels in two straight-line passes: every source byte of all of them is requested before the first is used (one memory round trip per tile
    // instead of one per pixel), so a pixel outside the map is resized at clamped coordinates and zeroed afterwards instead of being branched around
    {
        const size_t rs = (size_t)a.sw * 3;
        const uint8_t* const src = a.bgr + (size_t)n * a.sh * rs;
        int rgb[ST_PI][3];
        if (use_taps) {
            ResizeTap tx[ST_PI], ty[ST_PI];
#pragma unroll
            for (int i = 0; i < ST_PI; ++i) {
                const int p = min(tid + i * 256, ST_WH * ST_WW - 1), wy = p / ST_WW, wx = p - wy * ST_WW;
                const int cy = min(max(iy0 + wy, 0), a.dh - 1) - iy0, cx = min(max(ix0 + wx, 0), a.dw - 1) - ix0;      // (a clamped pixel of a window that meets the map lies in the window)
                ty[i] = taps[min(max(cy, 0), ST_WH - 1)]; tx[i] = taps[ST_WH + min(max(cx, 0), ST_WW - 1)];
            }
#pragma unroll
            for (int i = 0; i < ST_PI; ++i) resize_px_taps(src, rs, tx[i], ty[i], rgb[i]);
        } else {
#pragma unroll
            for (int i = 0; i < ST_PI; ++i) {
                const int p = min(tid + i * 256, ST_WH * ST_WW - 1), wy = p / ST_WW, wx = p - wy * ST_WW;
                resize_px_strided(src, rs, a.sh, a.sw, a.dh, a.dw, min(max(iy0 + wy, 0), a.dh - 1), min(max(ix0 + wx, 0), a.dw - 1), rgb[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < ST_PI; ++i) {
            const int p = tid + i * 256, wy = p / ST_WW, wx = p - wy * ST_WW;
            const int iy = iy0 + wy, ix = ix0 + wx;
            float v[3];
            kp_normalize(rgb[i], v);
            half4 hi, lo;
            stem_split4(v[0], v[1], v[2], 0.0f, hi, lo);
            const u32x2 h2 = __builtin_bit_cast(u32x2, hi), l2 = __builtin_bit_cast(u32x2, lo);
            const bool in_map = iy >= 0 && iy < a.dh && ix >= 0 && ix < a.dw;
            const u32x4 rec = in_map ? u32x4{h2[0], h2[1], l2[0], l2[1]} : u32x4{0u, 0u, 0u, 0u};
            if (p < ST_WH * ST_WW) *(u32x4*)(win + stem_rec(wy, wx)) = rec;
        }
    }
    __syncthreads();
    // ---- phase 2: conv1 ----
    // K slot j of fragment g = 2 * step + k-group: j < 3: channel j of tap 2 g; 4 <= j < 7: channel j - 4 of tap 2 g + 1; the spare slots 3 / 7 carry tap 8:
    // (g 0, slot 3) channel 0, (g 0, slot 7) channel 1, (g 1, slot 3) channel 2; every other spare slot is zero on both sides
    int roff[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int tap = 2 * (2 * s + kh) + i, ky = tap / 3, kx = tap - ky * 3;
            roff[s][i] = stem_rec(ky, kx);
        }
    const rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, (int)a.ybytes, 0x00020000);
    const float ds = a.descale;
    float vmax = 0.0f;
    f32x16 accs[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = wave * 2 + j;
        const char* const rb = win + stem_rec(2 * r, 2 * lx);
        f32x16 (&acc)[2] = accs[j];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[m][k] = 0.0f;
        const u32x4 r8 = *(const u32x4*)(rb + stem_rec(2, 2));
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const u32x4 r0 = *(const u32x4*)(rb + roff[s][0]), r1 = *(const u32x4*)(rb + roff[s][1]);
            const int g = 2 * s + kh;
            const unsigned xh0 = g == 0 ? r8[0] << 16 : g == 1 ? r8[1] << 16 : 0u, xh1 = g == 0 ? r8[0] & 0xFFFF0000u : 0u;
            const unsigned xl0 = g == 0 ? r8[2] << 16 : g == 1 ? r8[3] << 16 : 0u, xl1 = g == 0 ? r8[2] & 0xFFFF0000u : 0u;
            const u32x4 bh = {r0[0], r0[1] | xh0, r1[0], r1[1] | xh1}, bl = {r0[2], r0[3] | xl0, r1[2], r1[3] | xl1};
            const half8 Bh = __builtin_bit_cast(half8, bh), Bl = __builtin_bit_cast(half8, bl);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, A[s][0][m]), Bh, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, A[s][0][m]), Bl, acc[m], 0, 0, 0);
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, A[s][1][m]), Bh, acc[m], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                                  // every wave has read the window: the strips take its place
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        // ---- epilogue: the accumulator holds channels m * 32 + jj * 8 + kh * 4 + (0 .. 3) of pixel lx ----
        const int r = wave * 2 + j;
        f32x16 (&acc)[2] = accs[j];
        const int oy = oy0 + r;
        const bool inside = oy < a.ho && ox0 + lx < a.wo;
        char* const rec = strip + lx * ST_TPS + kh * 8;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float4 bv = *(const float4*)(a.bias + m * 32 + jj * 8 + kh * 4);
                float v0 = acc[m][jj * 4 + 0] * ds + bv.x, v1 = acc[m][jj * 4 + 1] * ds + bv.y, v2 = acc[m][jj * 4 + 2] * ds + bv.z, v3 = acc[m][jj * 4 + 3] * ds + bv.w;
                v0 = v0 > 0.f ? v0 : 0.f; v1 = v1 > 0.f ? v1 : 0.f; v2 = v2 > 0.f ? v2 : 0.f; v3 = v3 > 0.f ? v3 : 0.f;
                half4 hi, lo; stem_split4(v0, v1, v2, v3, hi, lo);
                const float mm = split_absmax4(vmax, v0, v1, v2, v3);
                vmax = inside ? mm : vmax;
                char* const d = rec + (m * 4 + jj) * 32;             // 8-channel group m * 4 + jj: [hi x 8][lo x 8]
                *(half4*)d = hi; *(half4*)(d + 16) = lo;
            }
        // the block's 32 pixel records (256 bytes each) out as 16-byte pieces: piece e = i * 64 + lane is unit e % 16 of pixel e / 16
        u32x4 sd[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { const int e = i * 64 + lane; sd[i] = *(const u32x4*)(strip + (e >> 4) * ST_TPS + (e & 15) * 16); }
        __builtin_amdgcn_sched_barrier(0);                            // all data registers read before the first store issues
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = i * 64 + lane, ox = ox0 + (e >> 4);
            const unsigned off = (oy < a.ho && ox < a.wo) ? (unsigned)((((n * a.ho + oy) * a.wo + ox) * a.ycs + a.yoff) * 2 + (e & 15) * 16) : OOB_OFF;
            __builtin_amdgcn_raw_buffer_store_b128(sd[i], yrs, off, 0, EAGLE_STORE_NT * 2);
        }
        // (wide stores read their data registers a few cycles after they issue: bneck.hip, HAZARD; the wait states are fenced on both sides)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 2" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    split_report(a.sat, n, vmax);
}

// ------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------
// folded fp32 weights [9 taps][3][64] -> [K step][hi | lo][2 channel blocks][lane 0..63][8]: lane l of a block's A fragment holds output channel (l & 31) of
// the block and the K slots of fragment g = 2 * step + (l >> 5) in the order the kernel builds its B fragments.  Scale and *descale as bneck_tile_weights.
void stem_tile_weights(const float* w, std::vector<_Float16>& out, float* descale)
{
    float amax = 0.f;
    for (int k = 0; k < 27 * 64; ++k) amax = std::max(amax, std::fabs(w[k]));
    int e = 0;
    if (amax > 0.f) (void)std::frexp(amax, &e);
    const int sw = 15 - e;
    const float scale = std::ldexp(1.0f, sw);
    *descale = std::ldexp(1.0f, -(sw + 4));
    out.resize((size_t)2 * 2 * 2 * 64 * 8);
    _Float16* d = out.data();
    for (int s = 0; s < 2; ++s)
        for (int part = 0; part < 2; ++part)
            for (int mb = 0; mb < 2; ++mb)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int g = 2 * s + (l >> 5);
                        int tap = -1, c = 0;
                        if (j < 3) { tap = 2 * g; c = j; }
                        else if (j >= 4 && j < 7) { tap = 2 * g + 1; c = j - 4; }
                        else if (g == 0) { tap = 8; c = j == 3 ? 0 : 1; }
                        else if (g == 1 && j == 3) { tap = 8; c = 2; }
                        const float v = tap < 0 ? 0.f : w[(size_t)(tap * 3 + c) * 64 + mb * 32 + (l & 31)] * scale;
                        const _Float16 hi = (_Float16)v;
                        *d++ = part == 0 ? hi : (_Float16)(v - (float)hi);
                    }
}

bool stem_supported(int precision, int ks, int stride, int cin, int cout)
{
    return precision == EAGLE_PREC_F32S && ks == 3 && stride == 2 && cin == 3 && cout == 64;
}

void stem_launch(const StemLaunch& L, hipStream_t s)
{
    const TView& y = L.y;
    const int ho = (L.dh - 1) / 2 + 1, wo = (L.dw - 1) / 2 + 1;
    if (y.f32 != 2 || y.c != 64 || y.h != ho || y.w != wo || L.n < 0 || L.n > y.n || L.sh < 1 || L.sw < 1 || L.dh < 1 || L.dw < 1 || !L.bgr)
        fail(EAGLE_E_INVALID, "fused stem: a %d x %d x 64-channel split-format output of at least %d frames required", ho, wo, L.n);
    const size_t ybytes = (size_t)y.n * y.h * y.w * y.cs * 4;
    if (ybytes >= ((size_t)1 << 31)) fail(EAGLE_E_INVALID, "fused stem: the output of %d frames reaches 2 GiB (32-bit tensor offsets); use a smaller device batch", y.n);
    if (L.n == 0) return;
    StemArgs a;
    a.bgr = L.bgr; a.n = L.n; a.sh = L.sh; a.sw = L.sw; a.dh = L.dh; a.dw = L.dw;
    a.w = L.w; a.bias = L.bias; a.descale = L.descale;
    a.y = y.p; a.ycs = y.cs * 2; a.yoff = y.off * 2; a.ybytes = (unsigned)ybytes; a.ho = ho; a.wo = wo;
    a.tiles_x = (wo + ST_TW - 1) / ST_TW; a.tiles_y = (ho + ST_TH - 1) / ST_TH;
    a.sat = L.sat_slot ? *L.sat_slot : nullptr;
    ensure_max_dynamic_lds((const void*)stem_split_kernel, ST_LDS);
    hipLaunchKernelGGL(stem_split_kernel, dim3((unsigned)(a.tiles_x * a.tiles_y * L.n)), dim3(256), ST_LDS, s, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace eagle
