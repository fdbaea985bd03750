// K32 — top view: dense BGR frames resident in HBM + the homography of each -> the frames warped onto the pitch plane (the minimap's canvas), their mean
// (the mosaic: the pitch without the players), and per frame the distance of its warp from that mean (include/eagle.h, eagle_topview_*;
// tests/topview_ref.py is the written definition of every byte).  The projective map is float64 with every product, sum and quotient a single IEEE
// operation (the file is built with -ffp-contract=off, the division is the compiler's); everything behind floor() is integers, and all accumulation is
// integer atomics or one thread's registers, so no result depends on an order.
//
//   topview_frames_kernel      a workgroup of 256 threads takes pix_out.h's 256 x 16 tile of frame blockIdx.z.  The frame's G comes from a per-frame
//                              table (uniform per workgroup).  Thread t samples column t of the tile row after row (x formed once per thread, the 16
//                              y once per workgroup; every pixel evaluates the rule's expressions as written, no stepping of u' along x), so a wave's
//                              12 byte loads per pixel fall on neighbouring source pixels; the tile crosses 16 KB of LDS into pix_out.h's unit, a
//                              thread's 2-row strip of 8 pixels, and leaves through its writer.
//   topview_accumulate_kernel  a thread owns a canvas pixel and walks a chunk of the job's frames (blockIdx.y) with the four sums in registers, then adds
//                              them to the accumulator with u32 atomics; one chunk when the canvas alone fills the chip.  The frame's boxes go through
//                              LDS once per workgroup and frame.
//   topview_residual_kernel    a workgroup takes four runs of 256 pixels of one frame against the mosaic's packed means (4 bytes per pixel, written once
//                              per call by the finish kernel: no division per frame); wave butterfly, the four waves through LDS, then one u64 and two
//                              u32 atomics per workgroup into the frame's triple.
//   topview_finish_kernel      accumulator -> the mosaic picture (dense BGR) and the cnt map, or the packed means the residual reads.
#include "runtime.h"
#include "pix_out.h"

namespace eagle {

static constexpr int64_t TV_STAGING = 64 << 20;
static constexpr int TV_PASS = 65535;                      // gridDim.y / .z limit
static constexpr int TV_MAX_DIM = 16384;                   // per frame side: U = floor(tu) < 2^22 + 1
static constexpr int TV_TARGET_WGS = 2048;                 // accumulate: frame chunks until the grid has about this many workgroups
static constexpr int TV_RES_RUNS = 4;                      // residual: runs of 256 pixels per workgroup (a quarter of the atomics on a frame's triple)
typedef unsigned long long tv_u64;
static_assert(sizeof(EagleTopviewParams) == 56, "include/eagle.h states this size");

struct TvFrame { double g[9]; int32_t ok, pad; };          // G of a frame (ok = 0: no map)

struct TvArgs {
    const uint8_t* bgr;          // job frame 0 (device, dense [h][w][3])
    int64_t fstride;             // bytes from a job frame to the next
    const TvFrame* tab;          // [n]
    const int32_t* boff;         // [n + 1] into boxes, or nullptr: no masking
    const float4* boxes;
    int n, h, w;                 // job frames of this launch; the frame size
    int S, M, W, Hc;
    double tu_hi, tv_hi, pad;    // 256 (w - 1) + 1, 256 (h - 1) + 1; box_pad
    uint32_t background, marking_colour, min_count;
    const uint8_t* mask;         // the marking bit mask, or nullptr
    int mask_pitch;
    int chunk;                   // accumulate: frames per blockIdx.y
    uint32_t* acc;               // [Hc][W][4]
    tv_u64* res_sum;             // [n]
    uint32_t* res_cnt;           // [n]
    uint32_t* covered;           // [n]
    uint8_t* pic;                // finish: [Hc][W][3]
    uint32_t* cnt;               // finish: [Hc][W]
    uint32_t* means;             // [Hc][W] B | G << 8 | R << 16 | (cnt >= min_count) << 24: finish writes it in place of pic and cnt, residual reads it
};

// the rule's SAMPLE: (x, y) on the pitch -> covered, the bilinear sample as B | G << 8 | R << 16, and the sample point (u, v)
__device__ __forceinline__ bool tv_sample(const double (&g)[9], double x, double y, const uint8_t* fr, int w, int h, double tu_hi, double tv_hi, uint32_t& out,
                                          double& u, double& v)
{
    const double up = ((g[0] * x) + (g[1] * y)) + g[2];
    const double vp = ((g[3] * x) + (g[4] * y)) + g[5];
    const double wp = ((g[6] * x) + (g[7] * y)) + g[8];
    u = up / wp; v = vp / wp;
    const double tu = u * 256.0 + 0.5, tv = v * 256.0 + 0.5;
    if (!(wp > 0.0 && tu >= 0.0 && tu < tu_hi && tv >= 0.0 && tv < tv_hi)) return false;       // (NaN fails)
    const int U = (int)floor(tu), V = (int)floor(tv);       // 0 <= U <= 256 (w - 1), likewise V
    const int x0 = U >> 8, y0 = V >> 8, x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const uint32_t fx = U & 255, fy = V & 255;
    const uint32_t w00 = (256u - fx) * (256u - fy), w10 = fx * (256u - fy), w01 = (256u - fx) * fy, w11 = fx * fy;
    const uint8_t* r0 = fr + (size_t)y0 * w * 3;
    const uint8_t* r1 = fr + (size_t)y1 * w * 3;
    const uint8_t* p00 = r0 + 3 * x0;
    const uint8_t* p10 = r0 + 3 * x1;
    const uint8_t* p01 = r1 + 3 * x0;
    const uint8_t* p11 = r1 + 3 * x1;
    out = 0;
    #pragma unroll
    for (int c = 0; c < 3; ++c) out |= ((w00 * p00[c] + w10 * p10[c] + w01 * p01[c] + w11 * p11[c] + 32768u) >> 16) << (8 * c);
    return true;
}

__device__ __forceinline__ void tv_load_g(const TvFrame& F, double (&g)[9])
{
    #pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = F.g[k];
}

__device__ __forceinline__ bool tv_in_boxes(const float4* s_box, int nb, double u, double v, double pad)
{
    bool hit = false;
    for (int k = 0; k < nb; ++k) {
        const float4 b = s_box[k];
        hit = hit || ((double)b.x - pad <= u && u <= (double)b.z + pad && (double)b.y - pad <= v && v <= (double)b.w + pad);
    }
    return hit;
}

// the workgroup stages job frame j's boxes (at most EAGLE_MAX_DET, checked on the host) -> their number; barriers inside
__device__ __forceinline__ int tv_stage_boxes(const TvArgs& a, int j, float4* s_box)
{
    const int b0 = a.boff[j], nb = a.boff[j + 1] - b0;
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += 256) s_box[i] = a.boxes[b0 + i];
    __syncthreads();
    return nb;
}

__device__ __forceinline__ uint32_t tv_wave_sum(uint32_t v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(AN_THREADS) void topview_frames_kernel(TvArgs a, AnnotArgs o)
{
    // Sampling and writing use two thread maps.  Sampling: thread t takes column t of the tile, row after row, so that the lanes of a wave gather
    // neighbouring source pixels (as strips, lanes 8 pixels apart touched 8 times the cache lines per load: 1.14 ms against this form's figure in
    // docs/experiments.md).  The tile crosses LDS, and each thread then owns its strip for pix_out.h's writer.
    __shared__ __align__(16) uint32_t s_px[AN_TH][AN_TW];
    __shared__ double s_y[AN_TH];
    const int f = blockIdx.z, tid = threadIdx.x;
    const int tx0 = blockIdx.x * AN_TW, ty0 = blockIdx.y * AN_TH;
    const TvFrame& F = a.tab[f];
    const uint8_t* fr = a.bgr + (int64_t)f * a.fstride;
    if (F.ok) {                                             // (uniform)
        static_assert(AN_THREADS == AN_TW, "a thread per tile column");
        if (tid < AN_TH) s_y[tid] = 68.0 - (double)(ty0 + tid - a.M) / (double)a.S;
        __syncthreads();
        double g[9];
        tv_load_g(F, g);
        const int X = tx0 + tid;
        const double x = (double)(X - a.M) / (double)a.S;
        #pragma unroll 2
        for (int r = 0; r < AN_TH; ++r) {
            uint32_t s = a.background;
            double u, v;
            if (X < a.W && ty0 + r < a.Hc) {
                uint32_t t;
                if (tv_sample(g, x, s_y[r], fr, a.w, a.h, a.tu_hi, a.tv_hi, t, u, v)) s = t;
            }
            s_px[r][tid] = s;
        }
        __syncthreads();
    }
    const int sx = tid % AN_SX, sy = tid / AN_SX;
    const int x0 = tx0 + sx * AN_STRIP, y0 = ty0 + 2 * sy;
    if (x0 >= a.W || y0 >= a.Hc) return;                    // (behind the last barrier)
    const int cnt = min(AN_STRIP, a.W - x0), rows = min(2, a.Hc - y0);
    uint32_t px[2][AN_STRIP];
    #pragma unroll
    for (int r = 0; r < 2; ++r)
        #pragma unroll
        for (int k = 0; k < AN_STRIP; ++k) px[r][k] = F.ok ? s_px[2 * sy + r][sx * AN_STRIP + k] : a.background;
    if (a.mask) {
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= rows) continue;
            const uint32_t b = a.mask[(size_t)(y0 + r) * a.mask_pitch + (x0 >> 3)];
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k)
                if (b >> k & 1) px[r][k] = a.marking_colour;
        }
    }
    write_strip(o, f, x0, y0, cnt, rows, px);
}

__global__ __launch_bounds__(256) void topview_accumulate_kernel(TvArgs a)
{
    __shared__ float4 s_box[EAGLE_MAX_DET];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x, NP = (int64_t)a.W * a.Hc;
    const bool live = p < NP;
    const int Y = (int)(p / a.W), X = (int)(p - (int64_t)Y * a.W);
    const double x = (double)(X - a.M) / (double)a.S, y = 68.0 - (double)(Y - a.M) / (double)a.S;
    const int j0 = blockIdx.y * a.chunk, j1 = min(j0 + a.chunk, a.n);
    uint32_t sb = 0, sg = 0, sr = 0, sc = 0;                // a chunk has at most 2^23 frames: 255 x 2^23 < 2^32
    for (int j = j0; j < j1; ++j) {
        const TvFrame& F = a.tab[j];
        if (!F.ok) continue;                                // (uniform: the barriers below are met by all or none)
        const int nb = a.boff ? tv_stage_boxes(a, j, s_box) : 0;
        if (!live) continue;
        double g[9], u, v;
        uint32_t s;
        tv_load_g(F, g);
        if (!tv_sample(g, x, y, a.bgr + (int64_t)j * a.fstride, a.w, a.h, a.tu_hi, a.tv_hi, s, u, v)) continue;
        if (nb && tv_in_boxes(s_box, nb, u, v, a.pad)) continue;
        sb += s & 255u; sg += (s >> 8) & 255u; sr += (s >> 16) & 255u; sc += 1;
    }
    if (live && sc) {
        uint32_t* A = a.acc + p * 4;
        atomicAdd(A, sb); atomicAdd(A + 1, sg); atomicAdd(A + 2, sr); atomicAdd(A + 3, sc);
    }
}

// the unpainted mean of an accumulator cell with cnt >= 1
__device__ __forceinline__ uint32_t tv_mean(uint32_t sum, uint32_t cnt) { return (uint32_t)((2ull * sum + cnt) / (2ull * cnt)); }

__global__ __launch_bounds__(256) void topview_residual_kernel(TvArgs a)
{
    __shared__ float4 s_box[EAGLE_MAX_DET];
    __shared__ uint32_t s_part[4][4];
    const int j = blockIdx.y, tid = threadIdx.x;
    const TvFrame& F = a.tab[j];
    if (!F.ok) return;                                      // (uniform)
    const int64_t NP = (int64_t)a.W * a.Hc;
    const int nb = a.boff ? tv_stage_boxes(a, j, s_box) : 0;
    double g[9];
    tv_load_g(F, g);
    uint32_t rs = 0, rc = 0, cv = 0;                        // per thread: at most TV_RES_RUNS x (765, 1, 1)
    #pragma unroll 1
    for (int i = 0; i < TV_RES_RUNS; ++i) {
        const int64_t p = ((int64_t)blockIdx.x * TV_RES_RUNS + i) * 256 + tid;
        if (p >= NP) break;
        const int Y = (int)(p / a.W), X = (int)(p - (int64_t)Y * a.W);
        const double x = (double)(X - a.M) / (double)a.S, y = 68.0 - (double)(Y - a.M) / (double)a.S;
        double u, v;
        uint32_t s;
        if (!tv_sample(g, x, y, a.bgr + (int64_t)j * a.fstride, a.w, a.h, a.tu_hi, a.tv_hi, s, u, v)) continue;
        cv += X >= a.M && X < a.M + 105 * a.S && Y >= a.M && Y < a.M + 68 * a.S;
        const uint32_t m = a.means[p];                      // the mosaic's unpainted means, bit 24: cnt >= min_count
        if (!(m >> 24) || (nb && tv_in_boxes(s_box, nb, u, v, a.pad))) continue;
        const int db = (int)(s & 255u) - (int)(m & 255u), dg = (int)((s >> 8) & 255u) - (int)((m >> 8) & 255u), dr = (int)((s >> 16) & 255u) - (int)((m >> 16) & 255u);
        rs += (uint32_t)(abs(db) + abs(dg) + abs(dr)); rc += 1;
    }
    rs = tv_wave_sum(rs); rc = tv_wave_sum(rc); cv = tv_wave_sum(cv);
    if ((tid & 63) == 0) { s_part[tid >> 6][0] = rs; s_part[tid >> 6][1] = rc; s_part[tid >> 6][2] = cv; }
    __syncthreads();
    if (tid == 0) {
        const uint32_t ts = s_part[0][0] + s_part[1][0] + s_part[2][0] + s_part[3][0], tc = s_part[0][1] + s_part[1][1] + s_part[2][1] + s_part[3][1],
                       tv = s_part[0][2] + s_part[1][2] + s_part[2][2] + s_part[3][2];
        if (ts) atomicAdd(&a.res_sum[j], (tv_u64)ts);
        if (tc) atomicAdd(&a.res_cnt[j], tc);
        if (tv) atomicAdd(&a.covered[j], tv);
    }
}

__global__ __launch_bounds__(256) void topview_finish_kernel(TvArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)a.W * a.Hc) return;
    const int Y = (int)(p / a.W), X = (int)(p - (int64_t)Y * a.W);
    const uint4 c = *(const uint4*)(a.acc + p * 4);
    uint32_t px = a.background;
    if (c.w >= a.min_count) px = tv_mean(c.x, c.w) | tv_mean(c.y, c.w) << 8 | tv_mean(c.z, c.w) << 16;      // (min_count >= 1)
    if (a.means) {                                          // the residual's view of the mosaic: no background, no markings
        a.means[p] = c.w >= a.min_count ? px | 1u << 24 : 0u;
        return;
    }
    if (a.mask && (a.mask[(size_t)Y * a.mask_pitch + (X >> 3)] >> (X & 7) & 1)) px = a.marking_colour;
    a.pic[p * 3] = (uint8_t)px; a.pic[p * 3 + 1] = (uint8_t)(px >> 8); a.pic[p * 3 + 2] = (uint8_t)(px >> 16);
    a.cnt[p] = c.w;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static MmPlan tv_plan(const char* who, const EagleTopviewParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the top-view parameters are NULL", who);
    if (p->scale < 2 || p->scale > 32 || (p->scale & 1)) fail(EAGLE_E_INVALID, "%s: scale %d must be even and within 2 .. 32 pixels per metre", who, p->scale);
    if (p->margin < 0 || p->margin > 64 || (p->margin & 1)) fail(EAGLE_E_INVALID, "%s: margin %d must be even and within 0 .. 64 pixels", who, p->margin);
    if (p->background > 0xffffffu) fail(EAGLE_E_INVALID, "%s: background 0x%x is no B | G << 8 | R << 16", who, p->background);
    if (p->marking_colour > 0xffffffu) fail(EAGLE_E_INVALID, "%s: marking_colour 0x%x is no B | G << 8 | R << 16", who, p->marking_colour);
    if (p->step < 1) fail(EAGLE_E_INVALID, "%s: step %d must be at least 1", who, p->step);
    if (p->first < 0) fail(EAGLE_E_INVALID, "%s: first %d is negative", who, p->first);
    if (p->min_count < 1) fail(EAGLE_E_INVALID, "%s: min_count %d must be at least 1", who, p->min_count);
    if (!(p->box_pad >= 0.0) || !std::isfinite(p->box_pad)) fail(EAGLE_E_INVALID, "%s: box_pad %g must be finite and not negative", who, p->box_pad);
    for (int k = 0; k < 3; ++k)
        if (p->reserved[k]) fail(EAGLE_E_INVALID, "%s: reserved word %d of the top-view parameters is %d, not 0", who, k, p->reserved[k]);
    MmPlan pl{};
    pl.S = p->scale; pl.M = p->margin;
    pl.w = 105 * pl.S + 2 * pl.M; pl.h = 68 * pl.S + 2 * pl.M;
    return pl;
}

static void tv_check_clip(const char* who, const void* frames, int n, int h, int w, const double* Hs, const uint8_t* valid, bool mosaic)
{
    if (n < 0) fail(EAGLE_E_INVALID, "%s: n %d is negative", who, n);
    if (mosaic && n > EAGLE_TOPVIEW_MAX_FRAMES) fail(EAGLE_E_INVALID, "%s: n %d is above the %d frames a mosaic's u32 sums hold", who, n, EAGLE_TOPVIEW_MAX_FRAMES);
    if (h < 1 || w < 1 || h > TV_MAX_DIM || w > TV_MAX_DIM) fail(EAGLE_E_INVALID, "%s: frames of %d x %d lie outside 1 .. %d per side", who, h, w, TV_MAX_DIM);
    if (n > 0 && !frames) fail(EAGLE_E_INVALID, "%s: the frames are NULL", who);
    if (n > 0 && !Hs) fail(EAGLE_E_INVALID, "%s: the homographies are NULL", who);
    if (n > 0 && !valid) fail(EAGLE_E_INVALID, "%s: the valid flags are NULL", who);
}

// the rule's MAP (tests/topview_ref.py frame_map): every product and sum single (-ffp-contract=off holds for the host code of this file too)
static TvFrame tv_frame_map(const double* H, int valid, int h, int w)
{
    static const int cof[9][4] = {{4, 8, 5, 7}, {2, 7, 1, 8}, {1, 5, 2, 4}, {5, 6, 3, 8}, {0, 8, 2, 6}, {2, 3, 0, 5}, {3, 7, 4, 6}, {1, 6, 0, 7}, {0, 4, 1, 3}};
    TvFrame F{};
    if (!valid) return F;
    double A[9];
    bool fin = true;
    for (int k = 0; k < 9; ++k) {
        const double pa = H[cof[k][0]] * H[cof[k][1]], pb = H[cof[k][2]] * H[cof[k][3]];
        A[k] = pa - pb;
        fin = fin && std::isfinite(H[k]) && std::isfinite(A[k]);
    }
    const double d0 = H[0] * A[0], d1 = H[1] * A[3], d2 = H[2] * A[6];
    const double det = (d0 + d1) + d2;
    const double s0 = H[6] * ((double)(w - 1) / 2.0), s1 = H[7] * (double)(h - 1);
    const double sb = (s0 + s1) + H[8];
    if (!fin || !std::isfinite(det) || !std::isfinite(sb) || det == 0.0 || sb == 0.0) return F;
    const bool same = (det > 0.0) == (sb > 0.0);
    for (int k = 0; k < 9; ++k) F.g[k] = same ? A[k] : -A[k];
    F.ok = 1;
    return F;
}

// the device memory of a call, freed with it
struct TvMem {
    std::vector<void*> owned;
    ~TvMem() { for (void* p : owned) (void)hipFree(p); }
    void* get(size_t b)
    {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, std::max<size_t>(b, 16)));
        owned.push_back(p);
        return p;
    }
    void* upload(const void* src, size_t b, hipStream_t s)
    {
        void* p = get(b);
        if (b) HIP_CHECK(hipMemcpyAsync(p, src, b, hipMemcpyHostToDevice, s));
        return p;
    }
};

// A job: the frames idx[0 .. m) of the clip, their maps and (masking) their boxes, in HBM
struct TvJob {
    std::vector<int> idx;
    std::vector<TvFrame> tab;
    std::vector<int32_t> boff;
    std::vector<float> boxes;
    const TvFrame* d_tab = nullptr; const int32_t* d_boff = nullptr; const float4* d_boxes = nullptr;
};

// boxes of frame i: from the records, or from the operator's (boxes, box_off)
static void tv_job(const char* who, TvJob& job, int n, int first, int step, int h, int w, const double* Hs, const uint8_t* valid, const EagleTopviewParams* p,
                   const EagleFrameResult* recs, const float* op_boxes, const int32_t* op_off)
{
    const bool masked = p->mask_boxes != 0;
    if (masked && !recs && !(op_boxes && op_off)) fail(EAGLE_E_INVALID, "%s: mask_boxes needs the records (their boxes are the mask)", who);
    if (masked && op_off) {
        if (op_off[0] != 0) fail(EAGLE_E_INVALID, "%s: box_off[0] is %d, not 0", who, op_off[0]);
        for (int i = 0; i < n; ++i)
            if (op_off[i + 1] < op_off[i] || op_off[i + 1] - op_off[i] > EAGLE_MAX_DET)
                fail(EAGLE_E_INVALID, "%s: frame %d has %d boxes (0 .. %d)", who, i, op_off[i + 1] - op_off[i], EAGLE_MAX_DET);
    }
    if (masked && recs)
        for (int i = 0; i < n; ++i)
            if (recs[i].n_det < 0 || recs[i].n_det > EAGLE_MAX_DET) fail(EAGLE_E_INVALID, "%s: record %d has n_det %d (0 .. %d)", who, i, recs[i].n_det, EAGLE_MAX_DET);
    if (masked) job.boff.push_back(0);
    for (int64_t i = first; i < n; i += step) {
        job.idx.push_back((int)i);
        job.tab.push_back(tv_frame_map(Hs + 9 * i, valid[i], h, w));
        if (!masked) continue;
        if (recs) {
            for (int k = 0; k < recs[i].n_det; ++k) {
                const EagleDet& d = recs[i].det[k];
                job.boxes.insert(job.boxes.end(), {d.x1, d.y1, d.x2, d.y2});
            }
        } else {
            job.boxes.insert(job.boxes.end(), op_boxes + 4 * (size_t)op_off[i], op_boxes + 4 * (size_t)op_off[i + 1]);
        }
        job.boff.push_back((int32_t)(job.boxes.size() / 4));
    }
}

static void tv_job_upload(TvJob& job, TvMem& mem, hipStream_t s)
{
    job.d_tab = (const TvFrame*)mem.upload(job.tab.data(), job.tab.size() * sizeof(TvFrame), s);
    if (!job.boff.empty()) {
        job.d_boff = (const int32_t*)mem.upload(job.boff.data(), job.boff.size() * 4, s);
        job.d_boxes = (const float4*)mem.upload(job.boxes.data(), job.boxes.size() * 4, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));                      // (pageable sources: they have left the vectors)
}

static TvArgs tv_args(const MmPlan& pl, const EagleTopviewParams* p, int h, int w, const uint8_t* d_mask)
{
    TvArgs a{};
    a.h = h; a.w = w; a.S = pl.S; a.M = pl.M; a.W = pl.w; a.Hc = pl.h;
    a.tu_hi = (double)(256 * (w - 1) + 1); a.tv_hi = (double)(256 * (h - 1) + 1); a.pad = p->box_pad;
    a.background = p->background; a.marking_colour = p->marking_colour; a.min_count = (uint32_t)p->min_count;
    a.mask = p->markings ? d_mask : nullptr; a.mask_pitch = (pl.w + 7) / 8;
    return a;
}

// job frames j0 .. j0 + m of `job`, which lie at d_bgr + k * fstride -> their pictures at o.dst; enqueued, not awaited
static void tv_video(EagleHandle* hd, TvArgs a, const TvJob& job, int j0, int m, const uint8_t* d_bgr, int64_t fstride, const AnnotArgs& out, hipStream_t s)
{
    const dim3 tiles((a.W + AN_TW - 1) / AN_TW, (a.Hc + AN_TH - 1) / AN_TH);
    auto fn = [&] {
        for (int f0 = 0; f0 < m; f0 += TV_PASS) {
            TvArgs b = a;
            AnnotArgs o = out;
            b.n = std::min(TV_PASS, m - f0); b.tab = job.d_tab + j0 + f0; b.bgr = d_bgr + (int64_t)f0 * fstride; b.fstride = fstride;
            o.dst = out.dst + (int64_t)f0 * out.frame_stride;
            hipLaunchKernelGGL(topview_frames_kernel, dim3(tiles.x, tiles.y, (unsigned)b.n), dim3(AN_THREADS), 0, s, b, o);
            HIP_CHECK(hipGetLastError());
        }
    };
    const double bytes = (double)m * ((double)a.h * a.w * 3.0 + (double)a.W * a.Hc * (out.fmt == EAGLE_PIX_BGR ? 3.0 : 1.5));
    if (hd) timed_launch(hd, "topview_frames", bytes, s, fn); else fn();
}

static TvArgs tv_slice(const TvArgs& a, const TvJob& job, int j0, int m, const uint8_t* d_bgr, int64_t fstride)
{
    TvArgs b = a;
    b.n = m; b.tab = job.d_tab + j0; b.bgr = d_bgr; b.fstride = fstride;
    if (job.d_boff) { b.boff = job.d_boff + j0; b.boxes = job.d_boxes; }
    return b;
}

static void tv_accumulate(EagleHandle* hd, const TvArgs& a, const TvJob& job, int j0, int m, const uint8_t* d_bgr, int64_t fstride, uint32_t* d_acc, hipStream_t s)
{
    if (m <= 0) return;
    TvArgs b = tv_slice(a, job, j0, m, d_bgr, fstride);
    b.acc = d_acc;
    const int64_t blocks = ((int64_t)a.W * a.Hc + 255) / 256;
    const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(m, TV_PASS), (TV_TARGET_WGS + blocks - 1) / blocks));
    b.chunk = (m + chunks - 1) / chunks;
    auto fn = [&] {
        hipLaunchKernelGGL(topview_accumulate_kernel, dim3((unsigned)blocks, (unsigned)((m + b.chunk - 1) / b.chunk)), dim3(256), 0, s, b);
        HIP_CHECK(hipGetLastError());
    };
    if (hd) timed_launch(hd, "topview_accumulate", (double)m * a.h * a.w * 3.0 + (double)a.W * a.Hc * 32.0, s, fn); else fn();
}

// the accumulator -> the packed means the residual reads (one division per channel and canvas pixel, not per frame); enqueued, not awaited
static uint32_t* tv_means(EagleHandle* hd, const TvArgs& a, const uint32_t* d_acc, TvMem& mem, hipStream_t s)
{
    const size_t NP = (size_t)a.W * a.Hc;
    TvArgs b = a;
    b.acc = const_cast<uint32_t*>(d_acc); b.means = (uint32_t*)mem.get(NP * 4);
    auto fn = [&] {
        hipLaunchKernelGGL(topview_finish_kernel, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, s, b);
        HIP_CHECK(hipGetLastError());
    };
    if (hd) timed_launch(hd, "topview_finish", (double)NP * 20.0, s, fn); else fn();
    return b.means;
}

// the triples of job frames j0 .. j0 + m at res_* + j0 (zeroed by the caller) against tv_means' map; enqueued, not awaited
static void tv_residual(EagleHandle* hd, const TvArgs& a, const TvJob& job, int j0, int m, const uint8_t* d_bgr, int64_t fstride, uint32_t* d_means, tv_u64* d_sum,
                        uint32_t* d_cnt, uint32_t* d_cov, hipStream_t s)
{
    const int64_t blocks = ((int64_t)a.W * a.Hc + 256 * TV_RES_RUNS - 1) / (256 * TV_RES_RUNS);
    auto fn = [&] {
        for (int f0 = 0; f0 < m; f0 += TV_PASS) {
            TvArgs b = tv_slice(a, job, j0 + f0, std::min(TV_PASS, m - f0), d_bgr + (int64_t)f0 * fstride, fstride);
            b.means = d_means; b.res_sum = d_sum + j0 + f0; b.res_cnt = d_cnt + j0 + f0; b.covered = d_cov + j0 + f0;
            hipLaunchKernelGGL(topview_residual_kernel, dim3((unsigned)blocks, (unsigned)b.n), dim3(256), 0, s, b);
            HIP_CHECK(hipGetLastError());
        }
    };
    if (hd) timed_launch(hd, "topview_residual", (double)m * ((double)a.h * a.w * 3.0 + (double)a.W * a.Hc * 16.0), s, fn); else fn();
}

// accumulator -> bgr_out [Hc][W][3], cnt_out [Hc][W] (host); returns when they are complete
static void tv_finish(EagleHandle* hd, const TvArgs& a, const uint32_t* d_acc, uint8_t* bgr_out, uint32_t* cnt_out, hipStream_t s)
{
    const size_t NP = (size_t)a.W * a.Hc;
    TvMem mem;
    TvArgs b = a;
    b.acc = const_cast<uint32_t*>(d_acc); b.pic = (uint8_t*)mem.get(NP * 3); b.cnt = (uint32_t*)mem.get(NP * 4);
    auto fn = [&] {
        hipLaunchKernelGGL(topview_finish_kernel, dim3((unsigned)((NP + 255) / 256)), dim3(256), 0, s, b);
        HIP_CHECK(hipGetLastError());
    };
    if (hd) timed_launch(hd, "topview_finish", (double)NP * 23.0, s, fn); else fn();
    HIP_CHECK(hipMemcpyAsync(bgr_out, b.pic, NP * 3, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(cnt_out, b.cnt, NP * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (hd && hd->prof) collect_spans(hd);
}

// the residual triples of a call in HBM, zeroed, and their way back
struct TvTriples {
    tv_u64* sum; uint32_t* cnt; uint32_t* cov; int n;
    TvTriples(TvMem& mem, int n_, hipStream_t s) : n(n_)
    {
        sum = (tv_u64*)mem.get((size_t)n * 16);
        cnt = (uint32_t*)(sum + n); cov = cnt + n;
        HIP_CHECK(hipMemsetAsync(sum, 0, (size_t)n * 16, s));
    }
    void fetch(uint64_t* res_sum, uint32_t* res_cnt, uint32_t* covered, hipStream_t s)
    {
        HIP_CHECK(hipMemcpyAsync(res_sum, sum, (size_t)n * 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(res_cnt, cnt, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(covered, cov, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
};

static void tv_sync(EagleHandle* h)
{
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    if (h->prof) collect_spans(h);
}

// the passes of a host-fed entry: job frames j0 .. j0 + k uploaded densely into `stage`, then run(j0, k)
static void tv_host_passes(EagleHandle* h, const char* who, const uint8_t* bgr, const TvJob& job, int64_t max_staging_bytes, TvMem& mem,
                           const std::function<void(int, int, const uint8_t*)>& run)
{
    const int64_t fb = (int64_t)h->cfg.frame_h * h->cfg.frame_w * 3;
    if (max_staging_bytes < 0) fail(EAGLE_E_INVALID, "%s: max_staging_bytes %lld is negative", who, (long long)max_staging_bytes);
    const int m = (int)job.idx.size();
    if (m == 0) return;
    const int pass = (int)std::max<int64_t>(1, std::min<int64_t>(m, (max_staging_bytes ? max_staging_bytes : TV_STAGING) / fb));
    uint8_t* stage = (uint8_t*)mem.get((size_t)pass * fb);
    try {
        for (int j0 = 0; j0 < m; j0 += pass) {
            const int k = std::min(pass, m - j0);
            for (int j = 0; j < k; ++j)
                HIP_CHECK(hipMemcpyAsync(stage + (int64_t)j * fb, bgr + (int64_t)job.idx[j0 + j] * fb, (size_t)fb, hipMemcpyHostToDevice, h->s_main));
            run(j0, k, stage);
            tv_sync(h);                                     // (the next pass reuses the staging)
        }
    } catch (...) {
        (void)hipStreamSynchronize(h->s_main);
        throw;
    }
}

}  // namespace eagle

extern "C" {

int eagle_topview_size(const EagleTopviewParams* p, int* w, int* h)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!w || !h) fail(EAGLE_E_INVALID, "eagle_topview_size: w or h is NULL");
    const MmPlan pl = tv_plan("eagle_topview_size", p);
    *w = pl.w; *h = pl.h;
    API_END(hh)
}

int eagle_topview_device_frames(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleTopviewParams* p, int out_format,
                                const EagleYuvLayout* out_layout, void* d_out)
{
    API_BEGIN_H(h)
    const char* who = "eagle_topview_device_frames";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    const MmPlan pl = tv_plan(who, p);
    tv_check_clip(who, d_bgr, n, fh, fw, Hs, valid, false);
    if (!d_out) fail(EAGLE_E_INVALID, "%s: d_out is NULL", who);
    const YuvGeom g = yuv_geometry(out_format, pl.h, pl.w, out_layout, true);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    TvJob job;
    EagleTopviewParams q = *p;
    q.mask_boxes = 0;
    tv_job(who, job, n, 0, 1, fh, fw, Hs, valid, &q, nullptr, nullptr, nullptr);
    TvMem mem;
    tv_job_upload(job, mem, h->s_main);
    const TvArgs a = tv_args(pl, p, fh, fw, p->markings ? minimap_mask(h, pl) : nullptr);
    tv_video(h, a, job, 0, n, d_bgr, (int64_t)fh * fw * 3, annot_args(g, nullptr, (uint8_t*)d_out, nullptr, nullptr), h->s_main);
    tv_sync(h);
    API_END(h)
}

int eagle_topview_frames(EagleHandle* h, const uint8_t* bgr, int n, const double* Hs, const uint8_t* valid, const EagleTopviewParams* p, int out_format,
                         const EagleYuvLayout* out_layout, uint8_t* out)
{
    API_BEGIN_H(h)
    const char* who = "eagle_topview_frames";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    const MmPlan pl = tv_plan(who, p);
    tv_check_clip(who, bgr, n, fh, fw, Hs, valid, false);
    if (!out) fail(EAGLE_E_INVALID, "%s: out is NULL", who);
    const YuvGeom g = yuv_geometry(out_format, pl.h, pl.w, out_layout, true);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    TvJob job;
    EagleTopviewParams q = *p;
    q.mask_boxes = 0;
    tv_job(who, job, n, 0, 1, fh, fw, Hs, valid, &q, nullptr, nullptr, nullptr);
    TvMem mem;
    tv_job_upload(job, mem, h->s_main);
    const TvArgs a = tv_args(pl, p, fh, fw, p->markings ? minimap_mask(h, pl) : nullptr);
    const int64_t fb = (int64_t)fh * fw * 3;
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(n, TV_STAGING / std::max<int64_t>(fb, g.dense_bytes)));
    uint8_t* stage = (uint8_t*)mem.get((size_t)batch * fb);
    frames_to_host(h, n, pl.h, pl.w, batch, out_format, out_layout, out, [&](int i, int na, const YuvGeom& dg, uint8_t* d_dst) {
        HIP_CHECK(hipMemcpyAsync(stage, bgr + (int64_t)i * fb, (size_t)na * fb, hipMemcpyHostToDevice, h->s_main));
        tv_video(h, a, job, i, na, stage, fb, annot_args(dg, nullptr, d_dst, nullptr, nullptr), h->s_main);
        tv_sync(h);
    });
    API_END(h)
}

int eagle_topview_mosaic_device(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                const EagleTopviewParams* p, uint32_t* d_acc, int reset)
{
    API_BEGIN_H(h)
    const char* who = "eagle_topview_mosaic_device";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    const MmPlan pl = tv_plan(who, p);
    tv_check_clip(who, d_bgr, n, fh, fw, Hs, valid, true);
    if (!d_acc) fail(EAGLE_E_INVALID, "%s: d_acc is NULL", who);
    TvJob job;
    tv_job(who, job, n, p->first, p->step, fh, fw, Hs, valid, p, recs, nullptr, nullptr);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    if (reset) HIP_CHECK(hipMemsetAsync(d_acc, 0, (size_t)pl.w * pl.h * 16, h->s_main));
    TvMem mem;
    if (!job.idx.empty()) {
        tv_job_upload(job, mem, h->s_main);
        const int64_t fb = (int64_t)fh * fw * 3;
        tv_accumulate(h, tv_args(pl, p, fh, fw, nullptr), job, 0, (int)job.idx.size(), d_bgr + (int64_t)p->first * fb, fb * p->step, d_acc, h->s_main);
    }
    tv_sync(h);
    API_END(h)
}

int eagle_topview_mosaic_finish(EagleHandle* h, const uint32_t* d_acc, const EagleTopviewParams* p, uint8_t* bgr_out, uint32_t* cnt_out)
{
    API_BEGIN_H(h)
    const char* who = "eagle_topview_mosaic_finish";
    const MmPlan pl = tv_plan(who, p);
    if (!d_acc || !bgr_out || !cnt_out) fail(EAGLE_E_INVALID, "%s: d_acc, bgr_out or cnt_out is NULL", who);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    tv_finish(h, tv_args(pl, p, 1, 1, p->markings ? minimap_mask(h, pl) : nullptr), d_acc, bgr_out, cnt_out, h->s_main);
    API_END(h)
}

int eagle_topview_residual_device(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                  const EagleTopviewParams* p, const uint32_t* d_acc, uint64_t* res_sum, uint32_t* res_cnt, uint32_t* covered)
{
    API_BEGIN_H(h)
    const char* who = "eagle_topview_residual_device";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    const MmPlan pl = tv_plan(who, p);
    tv_check_clip(who, d_bgr, n, fh, fw, Hs, valid, false);
    if (!d_acc) fail(EAGLE_E_INVALID, "%s: d_acc is NULL", who);
    if (n > 0 && (!res_sum || !res_cnt || !covered)) fail(EAGLE_E_INVALID, "%s: res_sum, res_cnt or covered is NULL", who);
    TvJob job;
    tv_job(who, job, n, 0, 1, fh, fw, Hs, valid, p, recs, nullptr, nullptr);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    TvMem mem;
    tv_job_upload(job, mem, h->s_main);
    TvTriples t(mem, n, h->s_main);
    const TvArgs a = tv_args(pl, p, fh, fw, nullptr);
    tv_residual(h, a, job, 0, n, d_bgr, (int64_t)fh * fw * 3, tv_means(h, a, d_acc, mem, h->s_main), t.sum, t.cnt, t.cov, h->s_main);
    tv_sync(h);
    t.fetch(res_sum, res_cnt, covered, h->s_main);
    API_END(h)
}

int eagle_topview_mosaic_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t max_staging_bytes, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                const EagleTopviewParams* p, uint32_t* d_acc, int reset)
{
    API_BEGIN_H(h)
    const char* who = "eagle_topview_mosaic_frames";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    const MmPlan pl = tv_plan(who, p);
    tv_check_clip(who, bgr, n, fh, fw, Hs, valid, true);
    if (!d_acc) fail(EAGLE_E_INVALID, "%s: d_acc is NULL", who);
    if (max_staging_bytes < 0) fail(EAGLE_E_INVALID, "%s: max_staging_bytes %lld is negative", who, (long long)max_staging_bytes);
    TvJob job;
    tv_job(who, job, n, p->first, p->step, fh, fw, Hs, valid, p, recs, nullptr, nullptr);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    if (reset) HIP_CHECK(hipMemsetAsync(d_acc, 0, (size_t)pl.w * pl.h * 16, h->s_main));
    TvMem mem;
    if (!job.idx.empty()) tv_job_upload(job, mem, h->s_main);
    const TvArgs a = tv_args(pl, p, fh, fw, nullptr);
    const int64_t fb = (int64_t)fh * fw * 3;
    tv_host_passes(h, who, bgr, job, max_staging_bytes, mem, [&](int j0, int k, const uint8_t* stage) { tv_accumulate(h, a, job, j0, k, stage, fb, d_acc, h->s_main); });
    tv_sync(h);
    API_END(h)
}

int eagle_topview_residual_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t max_staging_bytes, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                  const EagleTopviewParams* p, const uint32_t* d_acc, uint64_t* res_sum, uint32_t* res_cnt, uint32_t* covered)
{
    API_BEGIN_H(h)
    const char* who = "eagle_topview_residual_frames";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    const MmPlan pl = tv_plan(who, p);
    tv_check_clip(who, bgr, n, fh, fw, Hs, valid, false);
    if (!d_acc) fail(EAGLE_E_INVALID, "%s: d_acc is NULL", who);
    if (n > 0 && (!res_sum || !res_cnt || !covered)) fail(EAGLE_E_INVALID, "%s: res_sum, res_cnt or covered is NULL", who);
    if (max_staging_bytes < 0) fail(EAGLE_E_INVALID, "%s: max_staging_bytes %lld is negative", who, (long long)max_staging_bytes);
    TvJob job;
    tv_job(who, job, n, 0, 1, fh, fw, Hs, valid, p, recs, nullptr, nullptr);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    TvMem mem;
    tv_job_upload(job, mem, h->s_main);
    TvTriples t(mem, n, h->s_main);
    const TvArgs a = tv_args(pl, p, fh, fw, nullptr);
    const int64_t fb = (int64_t)fh * fw * 3;
    uint32_t* d_means = tv_means(h, a, d_acc, mem, h->s_main);
    tv_host_passes(h, who, bgr, job, max_staging_bytes, mem,
                   [&](int j0, int k, const uint8_t* stage) { tv_residual(h, a, job, j0, k, stage, fb, d_means, t.sum, t.cnt, t.cov, h->s_main); });
    t.fetch(res_sum, res_cnt, covered, h->s_main);
    API_END(h)
}

int eagle_op_topview(int device, const uint8_t* bgr, int n, int h, int w, const double* Hs, const uint8_t* valid, const float* boxes, const int32_t* box_off,
                     const EagleTopviewParams* p, int mode, int out_format, const EagleYuvLayout* out_layout, uint8_t* out, uint8_t* mosaic_out, uint32_t* cnt_out,
                     uint64_t* res_sum, uint32_t* res_cnt, uint32_t* covered)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_topview";
    const MmPlan pl = tv_plan(who, p);
    if (mode < 1 || (mode & ~(EAGLE_TOPVIEW_VIDEO | EAGLE_TOPVIEW_MOSAIC | EAGLE_TOPVIEW_RESIDUAL))) fail(EAGLE_E_INVALID, "%s: mode 0x%x names no known output", who, (unsigned)mode);
    const bool video = mode & EAGLE_TOPVIEW_VIDEO, mosaic = mode & EAGLE_TOPVIEW_MOSAIC, resid = mode & EAGLE_TOPVIEW_RESIDUAL;
    tv_check_clip(who, bgr, n, h, w, Hs, valid, mosaic || resid);
    if (video && !out) fail(EAGLE_E_INVALID, "%s: out is NULL", who);
    if (mosaic && (!mosaic_out || !cnt_out)) fail(EAGLE_E_INVALID, "%s: mosaic_out or cnt_out is NULL", who);
    if (resid && n > 0 && (!res_sum || !res_cnt || !covered)) fail(EAGLE_E_INVALID, "%s: res_sum, res_cnt or covered is NULL", who);
    YuvGeom g{};
    if (video) g = yuv_geometry(out_format, pl.h, pl.w, out_layout, true);
    TvJob all, sel;
    if (video || resid) tv_job(who, all, n, 0, 1, h, w, Hs, valid, p, nullptr, boxes, box_off);
    if (mosaic || resid) tv_job(who, sel, n, p->first, p->step, h, w, Hs, valid, p, nullptr, boxes, box_off);
    if (n == 0 && !mosaic) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    TvMem mem;
    int mp = 0;
    const uint8_t* d_mask = nullptr;
    if (p->markings) {
        const std::vector<uint8_t> bits = markings_mask(pl, &mp);
        d_mask = (const uint8_t*)mem.upload(bits.data(), bits.size(), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
    }
    const TvArgs a = tv_args(pl, p, h, w, d_mask);
    const int64_t fb = (int64_t)h * w * 3;
    const uint8_t* d_bgr = n ? (const uint8_t*)mem.upload(bgr, (size_t)n * fb, nullptr) : nullptr;
    if (!all.idx.empty()) tv_job_upload(all, mem, nullptr);
    if (!sel.idx.empty()) tv_job_upload(sel, mem, nullptr);
    if (video && n) {
        const size_t span = (size_t)((n - 1) * g.frame_stride + g.extent);
        uint8_t* d_out = (uint8_t*)mem.upload(out, span, nullptr);              // bytes the layout does not cover come back as they were
        tv_video(nullptr, a, all, 0, n, d_bgr, fb, annot_args(g, nullptr, d_out, nullptr, nullptr), nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, d_out, span, hipMemcpyDeviceToHost));
    }
    if (mosaic || resid) {
        uint32_t* d_acc = (uint32_t*)mem.get((size_t)pl.w * pl.h * 16);
        HIP_CHECK(hipMemsetAsync(d_acc, 0, (size_t)pl.w * pl.h * 16, nullptr));
        if (!sel.idx.empty()) tv_accumulate(nullptr, a, sel, 0, (int)sel.idx.size(), d_bgr + (int64_t)p->first * fb, fb * p->step, d_acc, nullptr);
        if (mosaic) tv_finish(nullptr, a, d_acc, mosaic_out, cnt_out, nullptr);
        if (resid && n) {
            TvTriples t(mem, n, nullptr);
            tv_residual(nullptr, a, all, 0, n, d_bgr, fb, tv_means(nullptr, a, d_acc, mem, nullptr), t.sum, t.cnt, t.cov, nullptr);
            t.fetch(res_sum, res_cnt, covered, nullptr);
        }
    }
    API_END(hh)
}

}  // extern "C"
