// K34 — ground layer: dense BGR frames resident in HBM + the homography of each + a list of shapes on the pitch plane per frame -> the frames with the
// shapes blended into the grass, as BGR, NV12 or I420 (include/eagle.h, eagle_ground_*; tests/ground_ref.py is the written definition of every byte).
// Every pixel maps four sub-samples to the pitch: float64, every product, sum and quotient a single IEEE operation (the file is built with
// -ffp-contract=off, the division is the compiler's); everything behind floor() is integers, and covered[] is an integer sum, so no result depends on
// how the work is split.
//
//   ground_frames_kernel   a workgroup of 256 threads takes pix_out.h's 256 x 16 tile of frame blockIdx.z.  The frame's H comes from a per-frame table
//                          (uniform per workgroup: scalar loads).  Wave 0 stages the frame's shapes in LDS once per workgroup, leaving out those
//                          with alpha 0 and, with the cull, those the tile cannot touch: the tile's four outer sub-sample corners are mapped, and when
//                          all four are on the ground the pitch bounding box of the tile is theirs (a projective map keeps a rectangle on one side
//                          of the horizon convex), widened by one q unit against rounding.  A tile without shapes (and a frame without a map) never
//                          maps a pixel: its strips are copied.  Otherwise thread t takes column t of the tile row after row (8 divisions per
//                          pixel; the shapes are read from LDS at one address per wave, a broadcast), the tile crosses 16 KB of LDS into
//                          pix_out.h's unit, a thread's 2-row strip of 8 pixels, and leaves through its writer.  covered: a wave butterfly and one
//                          u32 atomic per wave.
#include "runtime.h"
#include "pix_out.h"

namespace eagle {

static constexpr int64_t GR_STAGING = 64 << 20;
static constexpr int GR_PASS = 65535;                      // gridDim.z limit
static constexpr int GR_MAX_DIM = 16384;                   // per frame side
static constexpr int GR_ARG_MAX = 1 << 21, GR_R_MAX = 1 << 20;
static_assert(sizeof(EagleGroundShape) == 48 && sizeof(EagleGroundParams) == 16, "include/eagle.h states these sizes");

struct GrFrame { double h[9]; double sb; int32_t ok, s0, ns, pad; };      // a frame's H, the sign giver, its shapes shapes[s0 .. s0 + ns) (ok = 0: no map)

struct GrArgs {
    const uint8_t* bgr;          // job frame 0 (device, dense [h][w][3])
    int64_t fstride;             // bytes from a job frame to the next
    const GrFrame* tab;          // [n]
    const EagleGroundShape* shapes;
    uint32_t* covered;           // [n], zeroed in front of the launch
    int h, w;
    int key_min, key_lead;
    int cull;
};

// the rule's SUB-SAMPLE at (u, v): on the ground -> (qx, qy)
__device__ __forceinline__ bool gr_sample(const double (&hm)[9], bool pos, double u, double v, int& qx, int& qy)
{
    const double xp = ((hm[0] * u) + (hm[1] * v)) + hm[2];
    const double yp = ((hm[3] * u) + (hm[4] * v)) + hm[5];
    const double wp = ((hm[6] * u) + (hm[7] * v)) + hm[8];
    const double px = xp / wp, py = yp / wp;
    qx = 0; qy = 0;
    if (!((pos ? wp > 0.0 : wp < 0.0) && fabs(px) <= 1024.0 && fabs(py) <= 1024.0)) return false;       // (NaN and inf fail)
    qx = (int)floor(px * 1024.0 + 0.5); qy = (int)floor(py * 1024.0 + 0.5);
    return true;
}

__device__ __forceinline__ bool gr_inside(const EagleGroundShape& S, int qx, int qy)
{
    if (S.kind == EAGLE_GROUND_BAND) return S.a[0] <= qx && qx < S.a[1] && S.a[2] <= qy && qy < S.a[3];
    const int dx = qx - S.a[0], dy = qy - S.a[1];            // (|q| <= 2^20 + 1, |c| <= 2^21)
    if (abs(dx) >= S.a[3] || abs(dy) >= S.a[3]) return false;  // (outside the ring's box: most sub-samples, without a 64-bit product)
    const int64_t d2 = (int64_t)dx * dx + (int64_t)dy * dy;
    return (int64_t)S.a[2] * S.a[2] <= d2 && d2 < (int64_t)S.a[3] * S.a[3];
}

// 24 bytes = 6 little-endian words -> 8 pixels B | G << 8 | R << 16
__device__ __forceinline__ void gr_unpack8(const uint32_t* w, uint32_t* px)
{
    #pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t w0 = w[3 * q], w1 = w[3 * q + 1], w2 = w[3 * q + 2];
        px[4 * q] = w0 & 0xffffffu; px[4 * q + 1] = (w0 >> 24) | (w1 & 0xffffu) << 8; px[4 * q + 2] = (w1 >> 16) | (w2 & 0xffu) << 16; px[4 * q + 3] = w2 >> 8;
    }
}

__global__ __launch_bounds__(AN_THREADS) void ground_frames_kernel(GrArgs a, AnnotArgs o)
{
    __shared__ __align__(16) uint32_t s_px[AN_TH][AN_TW];
    __shared__ EagleGroundShape s_shape[EAGLE_GROUND_MAX_SHAPES];
    __shared__ int s_corner[4][3];                          // on, qx, qy
    __shared__ int s_n;
    const int f = blockIdx.z, tid = threadIdx.x;
    const int tx0 = blockIdx.x * AN_TW, ty0 = blockIdx.y * AN_TH;
    const GrFrame& F = a.tab[f];
    const uint8_t* fr = a.bgr + (int64_t)f * a.fstride;
    int ns = F.ok ? F.ns : 0;                               // (uniform, as everything that depends on it)
    if (ns) {
        double hm[9];
        #pragma unroll
        for (int k = 0; k < 9; ++k) hm[k] = F.h[k];
        const bool pos = F.sb > 0.0;
        // ---- the frame's shapes -> LDS in list order, without those this tile cannot show ----
        if (tid < 4) {
            const int X = (tid & 1) ? min(tx0 + AN_TW, a.w) - 1 : tx0, Y = (tid & 2) ? min(ty0 + AN_TH, a.h) - 1 : ty0;
            int qx, qy;
            s_corner[tid][0] = gr_sample(hm, pos, (double)X + ((tid & 1) ? 0.375 : -0.375), (double)Y + ((tid & 2) ? 0.375 : -0.375), qx, qy);
            s_corner[tid][1] = qx; s_corner[tid][2] = qy;
        }
        __syncthreads();
        if (tid < 64) {                                     // (wave 0; ns <= 16)
            const EagleGroundShape* gs = a.shapes + F.s0 + tid;
            bool keep = false;
            if (tid < ns) {
                const int kind = gs->kind, a0 = gs->a[0], a1 = gs->a[1], a2 = gs->a[2], a3 = gs->a[3];
                keep = gs->alpha != 0;
                if (keep && a.cull && s_corner[0][0] && s_corner[1][0] && s_corner[2][0] && s_corner[3][0]) {
                    const int x_lo = min(min(s_corner[0][1], s_corner[1][1]), min(s_corner[2][1], s_corner[3][1])) - 1;
                    const int x_hi = max(max(s_corner[0][1], s_corner[1][1]), max(s_corner[2][1], s_corner[3][1])) + 1;
                    const int y_lo = min(min(s_corner[0][2], s_corner[1][2]), min(s_corner[2][2], s_corner[3][2])) - 1;
                    const int y_hi = max(max(s_corner[0][2], s_corner[1][2]), max(s_corner[2][2], s_corner[3][2])) + 1;
                    if (kind == EAGLE_GROUND_BAND) keep = x_hi >= a0 && x_lo < a1 && y_hi >= a2 && y_lo < a3;
                    else keep = x_hi > a0 - a3 && x_lo < a0 + a3 && y_hi > a1 - a3 && y_lo < a1 + a3;       // (|c| + r1 < 2^31)
                }
            }
            const unsigned long long m = __ballot(keep);
            if (keep) s_shape[__popcll(m & ((1ull << tid) - 1ull))] = *gs;
            if (tid == 0) s_n = __popcll(m);
        }
        __syncthreads();
        ns = s_n;
        if (ns) {
            static_assert(AN_THREADS == AN_TW, "a thread per tile column");
            const int X = tx0 + tid;
            uint32_t cov = 0;
            #pragma unroll 1
            for (int r = 0; r < AN_TH; ++r) {
                const int Y = ty0 + r;
                uint32_t s = 0;
                if (X < a.w && Y < a.h) {
                    const uint8_t* p = fr + ((int64_t)Y * a.w + X) * 3;
                    int cb = p[0], cg = p[1], cr = p[2];
                    const bool grass = cg >= a.key_min && cg - max(cr, cb) >= a.key_lead;
                    int qx0, qy0, qx1, qy1, qx2, qy2, qx3, qy3;                 // the rotated grid
                    const bool on0 = gr_sample(hm, pos, (double)X + -0.375, (double)Y + -0.125, qx0, qy0);
                    const bool on1 = gr_sample(hm, pos, (double)X + 0.125, (double)Y + -0.375, qx1, qy1);
                    const bool on2 = gr_sample(hm, pos, (double)X + 0.375, (double)Y + 0.125, qx2, qy2);
                    const bool on3 = gr_sample(hm, pos, (double)X + -0.125, (double)Y + 0.375, qx3, qy3);
                    bool hit = false;
                    if (on0 || on1 || on2 || on3) {
                        for (int i = 0; i < ns; ++i) {
                            const EagleGroundShape& S = s_shape[i];
                            if ((S.flags & EAGLE_GROUND_KEYED) && !grass) continue;
                            const int c = (on0 && gr_inside(S, qx0, qy0)) + (on1 && gr_inside(S, qx1, qy1)) + (on2 && gr_inside(S, qx2, qy2)) + (on3 && gr_inside(S, qx3, qy3));
                            if (!c) continue;
                            const int A = S.alpha * c, B = 1024 - A;
                            cb = (cb * B + (int)(S.colour & 255u) * A + 512) >> 10;
                            cg = (cg * B + (int)((S.colour >> 8) & 255u) * A + 512) >> 10;
                            cr = (cr * B + (int)((S.colour >> 16) & 255u) * A + 512) >> 10;
                            hit = true;
                        }
                    }
                    cov += hit;
                    s = (uint32_t)cb | (uint32_t)cg << 8 | (uint32_t)cr << 16;
                }
                s_px[r][tid] = s;
            }
            #pragma unroll
            for (int d = 32; d >= 1; d >>= 1) cov += __shfl_xor(cov, d, 64);
            if ((tid & 63) == 0 && cov) atomicAdd(&a.covered[f], cov);
            __syncthreads();
        }
    }
    const int sx = tid % AN_SX, sy = tid / AN_SX;
    const int x0 = tx0 + sx * AN_STRIP, y0 = ty0 + 2 * sy;
    if (x0 >= a.w || y0 >= a.h) return;                     // (behind the last barrier)
    const int cnt = min(AN_STRIP, a.w - x0), rows = min(2, a.h - y0);        // 4:2:0: cnt even, rows = 2
    uint32_t px[2][AN_STRIP];
    if (ns) {
        #pragma unroll
        for (int r = 0; r < 2; ++r)
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k) px[r][k] = s_px[2 * sy + r][sx * AN_STRIP + k];
    } else {                                                // pass-through: the strip's source pixels
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k) px[r][k] = 0;
            if (r >= rows) continue;
            const uint8_t* s = fr + ((int64_t)(y0 + r) * a.w + x0) * 3;
            const uintptr_t sa = (uintptr_t)s;
            if (cnt == AN_STRIP && (sa & 3) == 0) {
                uint32_t w[6];
                #pragma unroll
                for (int k = 0; k < 6; ++k) w[k] = ((const uint32_t*)s)[k];
                gr_unpack8(w, px[r]);
            } else {
                #pragma unroll
                for (int k = 0; k < AN_STRIP; ++k)
                    if (k < cnt) px[r][k] = (uint32_t)s[3 * k] | (uint32_t)s[3 * k + 1] << 8 | (uint32_t)s[3 * k + 2] << 16;
            }
        }
    }
    write_strip(o, f, x0, y0, cnt, rows, px);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void gr_check(const char* who, const void* frames, int n, int h, int w, const double* Hs, const uint8_t* valid, const EagleGroundShape* shapes, const int32_t* off,
                     const EagleGroundParams* p, const void* out)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the ground parameters are NULL", who);
    if (p->key_min < 0 || p->key_min > 255) fail(EAGLE_E_INVALID, "%s: key_min %d lies outside 0 .. 255", who, p->key_min);
    if (p->key_lead < 0 || p->key_lead > 255) fail(EAGLE_E_INVALID, "%s: key_lead %d lies outside 0 .. 255", who, p->key_lead);
    if (p->no_cull != 0 && p->no_cull != 1) fail(EAGLE_E_INVALID, "%s: no_cull %d is neither 0 nor 1", who, p->no_cull);
    if (p->reserved) fail(EAGLE_E_INVALID, "%s: the reserved word of the ground parameters is %d, not 0", who, p->reserved);
    if (n < 0) fail(EAGLE_E_INVALID, "%s: n %d is negative", who, n);
    if (h < 1 || w < 1 || h > GR_MAX_DIM || w > GR_MAX_DIM) fail(EAGLE_E_INVALID, "%s: frames of %d x %d lie outside 1 .. %d per side", who, h, w, GR_MAX_DIM);
    if (n > 0 && !frames) fail(EAGLE_E_INVALID, "%s: the frames are NULL", who);
    if (n > 0 && !Hs) fail(EAGLE_E_INVALID, "%s: the homographies are NULL", who);
    if (n > 0 && !valid) fail(EAGLE_E_INVALID, "%s: the valid flags are NULL", who);
    if (n > 0 && !out) fail(EAGLE_E_INVALID, "%s: the output is NULL", who);
    if (!off) fail(EAGLE_E_INVALID, "%s: off is NULL", who);
    if (off[0] != 0) fail(EAGLE_E_INVALID, "%s: off[0] is %d, not 0", who, off[0]);
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > EAGLE_GROUND_MAX_SHAPES)
            fail(EAGLE_E_INVALID, "%s: frame %d has %d shapes (0 .. %d)", who, i, off[i + 1] - off[i], EAGLE_GROUND_MAX_SHAPES);
    const int ns = off[n];
    if (ns > 0 && !shapes) fail(EAGLE_E_INVALID, "%s: the shapes are NULL", who);
    for (int i = 0; i < ns; ++i) {
        const EagleGroundShape& s = shapes[i];
        if (s.kind != EAGLE_GROUND_BAND && s.kind != EAGLE_GROUND_RING) fail(EAGLE_E_INVALID, "%s: shape %d has the unknown kind %d", who, i, s.kind);
        if (s.flags & ~EAGLE_GROUND_KEYED) fail(EAGLE_E_INVALID, "%s: shape %d has the unknown flags 0x%x", who, i, (unsigned)s.flags);
        if (s.alpha < 0 || s.alpha > 256) fail(EAGLE_E_INVALID, "%s: shape %d has alpha %d (0 .. 256)", who, i, s.alpha);
        if (s.colour > 0xffffffu) fail(EAGLE_E_INVALID, "%s: shape %d has colour 0x%x, no B | G << 8 | R << 16", who, i, s.colour);
        if (s.a[4] || s.a[5] || s.reserved[0] || s.reserved[1]) fail(EAGLE_E_INVALID, "%s: shape %d has a non-zero reserved word", who, i);
        if (s.kind == EAGLE_GROUND_BAND) {
            for (int k = 0; k < 4; ++k)
                if (s.a[k] < -GR_ARG_MAX || s.a[k] > GR_ARG_MAX) fail(EAGLE_E_INVALID, "%s: band %d has the argument %d beyond +-%d", who, i, s.a[k], GR_ARG_MAX);
            if (s.a[0] >= s.a[1] || s.a[2] >= s.a[3]) fail(EAGLE_E_INVALID, "%s: band %d is empty: x %d .. %d, y %d .. %d", who, i, s.a[0], s.a[1], s.a[2], s.a[3]);
        } else {
            if (s.a[0] < -GR_ARG_MAX || s.a[0] > GR_ARG_MAX || s.a[1] < -GR_ARG_MAX || s.a[1] > GR_ARG_MAX)
                fail(EAGLE_E_INVALID, "%s: ring %d has its centre (%d, %d) beyond +-%d", who, i, s.a[0], s.a[1], GR_ARG_MAX);
            if (s.a[2] < 0 || s.a[2] >= s.a[3] || s.a[3] > GR_R_MAX) fail(EAGLE_E_INVALID, "%s: ring %d has the radii %d, %d (0 <= r0 < r1 <= %d)", who, i, s.a[2], s.a[3], GR_R_MAX);
        }
    }
}

// the rule's MAP: every product and sum single (-ffp-contract=off holds for the host code of this file too)
static GrFrame gr_frame_map(const double* H, int valid, int h, int w, int s0, int ns)
{
    GrFrame F{};
    F.s0 = s0; F.ns = ns;
    if (!valid) return F;
    bool fin = true;
    for (int k = 0; k < 9; ++k) { F.h[k] = H[k]; fin = fin && std::isfinite(H[k]); }
    const double s0_ = H[6] * ((double)(w - 1) / 2.0), s1 = H[7] * (double)(h - 1);
    F.sb = (s0_ + s1) + H[8];
    F.ok = fin && std::isfinite(F.sb) && F.sb != 0.0;
    return F;
}

// the device memory of a call, freed with it
struct GrMem {
    std::vector<void*> owned;
    ~GrMem() { for (void* p : owned) (void)hipFree(p); }
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

// the table, the shapes and the zeroed covered counts of a call in HBM
struct GrJob {
    std::vector<GrFrame> tab;
    GrArgs a{};
    GrJob(int n, int h, int w, const double* Hs, const uint8_t* valid, const EagleGroundShape* shapes, const int32_t* off, const EagleGroundParams* p, GrMem& mem, hipStream_t s)
    {
        for (int i = 0; i < n; ++i) tab.push_back(gr_frame_map(Hs + 9 * (size_t)i, valid[i], h, w, off[i], off[i + 1] - off[i]));
        a.tab = (const GrFrame*)mem.upload(tab.data(), tab.size() * sizeof(GrFrame), s);
        a.shapes = (const EagleGroundShape*)mem.upload(shapes, (size_t)off[n] * sizeof(EagleGroundShape), s);
        a.covered = (uint32_t*)mem.get((size_t)n * 4);
        HIP_CHECK(hipMemsetAsync(a.covered, 0, (size_t)n * 4, s));
        HIP_CHECK(hipStreamSynchronize(s));                  // (pageable sources: they have left the caller's memory and the vector)
        a.h = h; a.w = w; a.key_min = p->key_min; a.key_lead = p->key_lead; a.cull = !p->no_cull;
    }
    void fetch(int n, uint32_t* covered, hipStream_t s) const
    {
        if (!covered) return;
        HIP_CHECK(hipMemcpyAsync(covered, a.covered, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    }
};

// job frames j0 .. j0 + m, which lie at d_bgr + k * fstride -> their pictures at out.dst; enqueued, not awaited
static void gr_launch(EagleHandle* hd, const GrJob& job, int j0, int m, const uint8_t* d_bgr, int64_t fstride, const AnnotArgs& out, hipStream_t s)
{
    const GrArgs& a = job.a;
    const dim3 tiles((a.w + AN_TW - 1) / AN_TW, (a.h + AN_TH - 1) / AN_TH);
    auto fn = [&] {
        for (int f0 = 0; f0 < m; f0 += GR_PASS) {
            GrArgs b = a;
            AnnotArgs o = out;
            b.tab = a.tab + j0 + f0; b.covered = a.covered + j0 + f0; b.bgr = d_bgr + (int64_t)f0 * fstride; b.fstride = fstride;
            o.dst = out.dst + (int64_t)f0 * out.frame_stride;
            hipLaunchKernelGGL(ground_frames_kernel, dim3(tiles.x, tiles.y, (unsigned)std::min(GR_PASS, m - f0)), dim3(AN_THREADS), 0, s, b, o);
            HIP_CHECK(hipGetLastError());
        }
    };
    const double bytes = (double)m * (double)a.h * a.w * (3.0 + (out.fmt == EAGLE_PIX_BGR ? 3.0 : 1.5));
    if (hd) timed_launch(hd, "ground_frames", bytes, s, fn); else fn();
}

static void gr_sync(EagleHandle* h)
{
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    if (h->prof) collect_spans(h);
}

}  // namespace eagle

extern "C" {

int eagle_ground_device_frames(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleGroundShape* shapes, const int32_t* off,
                               const EagleGroundParams* p, int out_format, const EagleYuvLayout* out_layout, void* d_out, uint32_t* covered)
{
    API_BEGIN_H(h)
    const char* who = "eagle_ground_device_frames";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    gr_check(who, d_bgr, n, fh, fw, Hs, valid, shapes, off, p, d_out);
    if (n > 0 && (const void*)d_bgr == d_out) fail(EAGLE_E_INVALID, "%s: d_out is the clip itself; the pictures need a buffer of their own", who);
    const YuvGeom g = yuv_geometry(out_format, fh, fw, out_layout, true);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    GrMem mem;
    const GrJob job(n, fh, fw, Hs, valid, shapes, off, p, mem, h->s_main);
    gr_launch(h, job, 0, n, d_bgr, (int64_t)fh * fw * 3, annot_args(g, nullptr, (uint8_t*)d_out, nullptr, nullptr), h->s_main);
    gr_sync(h);
    job.fetch(n, covered, h->s_main);
    API_END(h)
}

int eagle_ground_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t max_staging_bytes, const double* Hs, const uint8_t* valid, const EagleGroundShape* shapes,
                        const int32_t* off, const EagleGroundParams* p, int out_format, const EagleYuvLayout* out_layout, uint8_t* out, uint32_t* covered)
{
    API_BEGIN_H(h)
    const char* who = "eagle_ground_frames";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    gr_check(who, bgr, n, fh, fw, Hs, valid, shapes, off, p, out);
    if (max_staging_bytes < 0) fail(EAGLE_E_INVALID, "%s: max_staging_bytes %lld is negative", who, (long long)max_staging_bytes);
    (void)yuv_geometry(out_format, fh, fw, out_layout, true);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    GrMem mem;
    const GrJob job(n, fh, fw, Hs, valid, shapes, off, p, mem, h->s_main);
    const int64_t fb = (int64_t)fh * fw * 3;
    const int pass = (int)std::max<int64_t>(1, std::min<int64_t>(n, (max_staging_bytes ? max_staging_bytes : GR_STAGING) / fb));
    uint8_t* stage = (uint8_t*)mem.get((size_t)pass * fb);
    frames_to_host(h, n, fh, fw, pass, out_format, out_layout, out, [&](int i, int na, const YuvGeom& dg, uint8_t* d_dst) {
        HIP_CHECK(hipMemcpyAsync(stage, bgr + (int64_t)i * fb, (size_t)na * fb, hipMemcpyHostToDevice, h->s_main));
        gr_launch(h, job, i, na, stage, fb, annot_args(dg, nullptr, d_dst, nullptr, nullptr), h->s_main);
        gr_sync(h);                                         // (the next pass reuses the staging)
    });
    job.fetch(n, covered, h->s_main);
    API_END(h)
}

int eagle_op_ground(int device, const uint8_t* bgr, int n, int h, int w, const double* Hs, const uint8_t* valid, const EagleGroundShape* shapes, const int32_t* off,
                    const EagleGroundParams* p, int out_format, const EagleYuvLayout* out_layout, uint8_t* out, uint32_t* covered)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_ground";
    gr_check(who, bgr, n, h, w, Hs, valid, shapes, off, p, out);
    const YuvGeom g = yuv_geometry(out_format, h, w, out_layout, true);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    GrMem mem;
    const GrJob job(n, h, w, Hs, valid, shapes, off, p, mem, nullptr);
    const int64_t fb = (int64_t)h * w * 3;
    const uint8_t* d_bgr = (const uint8_t*)mem.upload(bgr, (size_t)n * fb, nullptr);
    const size_t span = (size_t)((n - 1) * g.frame_stride + g.extent);
    uint8_t* d_out = (uint8_t*)mem.upload(out, span, nullptr);                  // bytes the layout does not cover come back as they were
    gr_launch(nullptr, job, 0, n, d_bgr, fb, annot_args(g, nullptr, d_out, nullptr, nullptr), nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, d_out, span, hipMemcpyDeviceToHost));
    job.fetch(n, covered, nullptr);
    API_END(hh)
}

}  // extern "C"
