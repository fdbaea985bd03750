// K39: the per-round accumulation of line registration (tests/linefit_ref.py POINT, MATCH, ROW, SUMS), shared by csrc/linefit.hip and tools/linefit_rate.py.
// The library instantiates linefit_accumulate_kernel<false> only: per-lane partial sums, a wave butterfly, one u64 atomic per wave and sum.  <true>, one
// atomic per inlier and sum, is the rate tool's comparison.  Needs <hip/hip_runtime.h>, <cstdint> and include/eagle.h in front of it.
#pragma once

namespace eagle {

static constexpr int LF_NSEG = 17, LF_NARC = 3, LF_NPRIM = 20;
static constexpr int LF_NSUM = 66;                         // 36 N (i <= j, row-major), 8 b, cnt, se2, 20 inliers per primitive
static constexpr int LF_REG = 46;                          // the sums a lane holds in registers
static constexpr int LF_CX = 53760, LF_CY = 34816, LF_R = 9370;
typedef unsigned long long lf_u64;

struct LfSeg { int32_t orient, c, a0, a1; };
struct LfArc { int32_t cx, cy, side, lim; };
// tests/linefit_ref.py SEGMENTS / ARCS (it asserts these literals against the minimap's constants)
__constant__ LfSeg c_seg[LF_NSEG] = {{1, 0, 0, 107520}, {1, 69632, 0, 107520}, {0, 0, 0, 69632}, {0, 107520, 0, 69632}, {0, 53760, 0, 69632},
                                     {0, 16896, 14172, 55460}, {1, 14172, 0, 16896}, {1, 55460, 0, 16896}, {0, 90624, 14172, 55460},
                                     {1, 14172, 90624, 107520}, {1, 55460, 90624, 107520}, {0, 5632, 25436, 44196}, {1, 25436, 0, 5632},
                                     {1, 44196, 0, 5632}, {0, 101888, 25436, 44196}, {1, 25436, 101888, 107520}, {1, 44196, 101888, 107520}};
__constant__ LfArc c_arc[LF_NARC] = {{53760, 34816, 0, 0}, {11264, 34816, 1, 16896}, {96256, 34816, -1, 90624}};

struct LfFrame { double g[9]; int32_t ok, flipped; };      // MAP of a frame, from the host
struct LfState { double m[9]; int32_t changed, fall, rung, pad; };   // the current matrix and what the rounds did

struct LfArgs {
    const uint8_t* bgr;          // chunk frame 0 (device, dense [h][w][3])
    int64_t fstride;
    const LfFrame* tab;          // [n]
    LfState* st;                 // [n]
    const int32_t* boff;         // [n + 1] into boxes, or nullptr
    const float4* boxes;
    int n, h, w, wpr;            // frames of the chunk; frame size; mask words per row
    int k, tau;
    double pad;
    uint32_t* mask;              // [n][h][wpr]
    uint32_t* nline;             // [n]
    lf_u64* sums;                // [slots][n][LF_NSUM]
    int slot, use_orig;          // accumulate: where to, and under G (1) or the state's matrix (0)
    int64_t rq2;                 // accumulate: the inlier bound
    int model, min_points, min_per_line;
    double max_step;
    int rounds;
    int64_t ms2;                 // decide: floor(max_shift 1024 + 0.5)^2
    int slot_before, slot_after;
    double* hout;                // [n][9]
    EagleLineFitFrame* rec;      // [n]
};

// POINT: (x, y) under m -> (qx, qy)
__device__ __forceinline__ bool lf_point(const double (&m)[9], double x, double y, int& qx, int& qy)
{
    const double up = ((m[0] * x) + (m[1] * y)) + m[2];
    const double vp = ((m[3] * x) + (m[4] * y)) + m[5];
    const double wp = ((m[6] * x) + (m[7] * y)) + m[8];
    const double X = up / wp, Y = vp / wp;
    if (!(wp > 0.0 && fabs(X) <= 1024.0 && fabs(Y) <= 1024.0)) return false;                  // (NaN fails)
    qx = (int)floor(X * 1024.0 + 0.5); qy = (int)floor(Y * 1024.0 + 0.5);
    return true;
}

// MATCH: -> the primitive (or -1) and e
__device__ __forceinline__ int lf_match(int qx, int qy, int64_t& e_out)
{
    int best = -1;
    int64_t be = 0, be2 = 0;
    #pragma unroll
    for (int i = 0; i < LF_NSEG; ++i) {
        const LfSeg s = c_seg[i];
        const int along = s.orient == 0 ? qy : qx, across = s.orient == 0 ? qx : qy;
        const int64_t e = (int64_t)across - s.c;
        if (along >= s.a0 && along <= s.a1 && (best < 0 || e * e < be2)) { best = i; be = e; be2 = e * e; }
    }
    #pragma unroll
    for (int j = 0; j < LF_NARC; ++j) {
        const LfArc c = c_arc[j];
        const bool cand = c.side == 0 || (c.side > 0 ? qx > c.lim : qx < c.lim);
        const int64_t dx = (int64_t)qx - c.cx, dy = (int64_t)qy - c.cy;
        // floor((d2 - R^2 + R) / (2 R)): the numerator is moved up by 2 R * R, which keeps it positive
        const int64_t e = (dx * dx + dy * dy + (int64_t)LF_R * LF_R + LF_R) / (2 * LF_R) - LF_R;
        if (cand && (best < 0 || e * e < be2)) { best = LF_NSEG + j; be = e; be2 = e * e; }
    }
    e_out = be;
    return best;
}

// ROW of an inlier matched to `prim`
__device__ __forceinline__ void lf_row(int qx, int qy, int prim, int (&J)[8])
{
    int gx, gy;
    if (prim < LF_NSEG) {
        const bool v = c_seg[prim].orient == 0;
        gx = v ? 128 : 0; gy = v ? 0 : 128;
    } else {
        const LfArc c = c_arc[prim - LF_NSEG];
        // floor((256 d + R) / (2 R)), moved up by 2 R * 65536 (|256 d| < 2^30)
        gx = (int)((256 * ((int64_t)qx - c.cx) + LF_R + (int64_t)2 * LF_R * 65536) / (2 * LF_R) - 65536);
        gy = (int)((256 * ((int64_t)qy - c.cy) + LF_R + (int64_t)2 * LF_R * 65536) / (2 * LF_R) - 65536);
    }
    const int xs = (qx - LF_CX) >> 7, ys = (qy - LF_CY) >> 7;
    const int64_t t = (int64_t)gx * xs + (int64_t)gy * ys;
    J[0] = 512 * gx; J[1] = gx * xs; J[2] = gx * ys; J[3] = 512 * gy; J[4] = gy * xs; J[5] = gy * ys;
    J[6] = (int)-((t * xs) >> 9); J[7] = (int)-((t * ys) >> 9);
}

__device__ __forceinline__ int64_t lf_wave_sum(int64_t v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int lo = __shfl_xor((int)(uint32_t)(lf_u64)v, d, 64), hi = __shfl_xor((int)(uint32_t)((lf_u64)v >> 32), d, 64);
        v += (int64_t)(((lf_u64)(uint32_t)hi << 32) | (uint32_t)lo);
    }
    return v;
}

template <bool PER_INLIER>
__global__ __launch_bounds__(256) void linefit_accumulate_kernel(LfArgs a)
{
    __shared__ uint32_t s_cnt[LF_NPRIM];
    const int f = blockIdx.y;
    const LfFrame& F = a.tab[f];
    if (!F.ok) return;                                      // (uniform)
    if (threadIdx.x < LF_NPRIM) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    double m[9];
    #pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = a.use_orig ? F.g[i] : a.st[f].m[i];
    lf_u64* out = a.sums + ((size_t)a.slot * a.n + f) * LF_NSUM;
    const int idx = blockIdx.x * 256 + threadIdx.x, nw = a.h * a.wpr;
    uint32_t bits = idx < nw ? a.mask[(size_t)f * nw + idx] : 0u;
    const int y = idx / a.wpr, xb = (idx - y * a.wpr) * 32;
    int64_t acc[LF_REG];
    #pragma unroll
    for (int i = 0; i < LF_REG; ++i) acc[i] = 0;
    bool any = false;
    while (bits) {
        const int b = __ffs(bits) - 1;
        bits &= bits - 1;
        int qx, qy;
        if (!lf_point(m, (double)(xb + b), (double)y, qx, qy)) continue;
        int64_t e;
        const int prim = lf_match(qx, qy, e);
        if (prim < 0 || e * e > a.rq2) continue;
        int J[8];
        lf_row(qx, qy, prim, J);
        atomicAdd(&s_cnt[prim], 1u);
        if (PER_INLIER) {
            int s = 0;
            #pragma unroll
            for (int i = 0; i < 8; ++i)
                #pragma unroll
                for (int j = i; j < 8; ++j) atomicAdd(out + s++, (lf_u64)((int64_t)J[i] * J[j]));
            #pragma unroll
            for (int i = 0; i < 8; ++i) atomicAdd(out + 36 + i, (lf_u64)((int64_t)J[i] * e));
            atomicAdd(out + 44, (lf_u64)1);
            atomicAdd(out + 45, (lf_u64)(e * e));
        } else {
            int s = 0;
            #pragma unroll
            for (int i = 0; i < 8; ++i)
                #pragma unroll
                for (int j = i; j < 8; ++j) acc[s++] += (int64_t)J[i] * J[j];
            #pragma unroll
            for (int i = 0; i < 8; ++i) acc[36 + i] += (int64_t)J[i] * e;
            acc[44] += 1;
            acc[45] += e * e;
            any = true;
        }
    }
    if (!PER_INLIER && __ballot(any)) {                     // (uniform per wave)
        #pragma unroll
        for (int i = 0; i < LF_REG; ++i) {
            const int64_t v = lf_wave_sum(acc[i]);
            if ((threadIdx.x & 63) == 0 && v) atomicAdd(out + i, (lf_u64)v);
        }
    }
    __syncthreads();
    if (threadIdx.x < LF_NPRIM && s_cnt[threadIdx.x]) atomicAdd(out + 46 + threadIdx.x, (lf_u64)s_cnt[threadIdx.x]);
}

}  // namespace eagle
