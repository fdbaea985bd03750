// K19 — annotated output: the frames of a clip resident in HBM with their records drawn on them (what the reference's main.py:43-81 draws into
// annotated.mp4), written as BGR, NV12 or I420 in the layout a video encoder takes.  tests/annot_ref.py is the written definition of every
// output byte (own rasterisation, integer arithmetic only; NOT cv2.ellipse / cv2.putText pixels); BGR -> 4:2:0 is OpenCV's integer BT.601
// limited-range path of COLOR_BGR2YUV_I420, the inverse of yuv.hip.
//
// One launch for all frames.  A workgroup owns an AN_TH x AN_TW pixel tile of one frame (even sizes: a 2 x 2 chroma block never straddles
// workgroups): it first culls the frame's primitive list against the tile by bounding box into LDS, in list order (painter's order is list
// order).  Most tiles keep nothing and are a plain copy / conversion.  A thread then owns a 2-row strip of AN_STRIP pixels, the mirror of
// yuv_to_bgr_kernel: 8-byte loads of the 24 BGR bytes per row, the culled primitives applied to the 16 pixels in registers, 8-byte stores of Y per
// row + 8 bytes of UV (NV12) or 4 + 4 bytes of U and V (I420), or three 8-byte BGR stores per row.  A wave covers 32 strips = 768 contiguous bytes
// of a source row.  Tail strips and addresses without the alignment go byte by byte.  The source is never written; no annotated BGR
// intermediate goes through HBM unless BGR is the requested output.
//
// The "out" part is pix_out.h's write_strip, shared with minimap.hip (K21).
//
// The host side of the same file: overlay_from_record (the ONE place that decides what a record's picture is), the argument checks and the
// eagle_annotate_* / eagle_op_annotate entries.
#include "runtime.h"
#include "annot_font.h"
#include "pix_out.h"

namespace eagle {

static constexpr int ARC_A = 35, ARC_B = 18, GLYPH_W = 10, GLYPH_H = 14, GLYPH_ADV = 12;
static constexpr int COORD_MAX = 1 << 20, RADIUS_MAX = 1 << 14, LABEL_MAX_ID = 99999, AN_MAX_DIM = 32767;     // (tile-clamped boxes are packed as 16-bit pairs)
__constant__ uint8_t c_font[10][ANNOT_FONT_ROWS] = {ANNOT_FONT_TABLE};

// a primitive as the tile keeps it: LABEL carries its digits (a[3] = count, a[4] = 4 bits per digit, first digit lowest), every kind its bounding box
// clamped to the tile
struct TilePrim { int a[6]; uint32_t kc; uint32_t bx, by; };      // kc = B | G << 8 | R << 16 | kind << 24; bx = x_lo | x_hi << 16, by likewise

struct Box { int x0, y0, x1, y1; };
// inclusive bounding box of a primitive; false: it covers nothing.  Fills the LABEL digits.
__device__ __forceinline__ bool prim_box(const EaglePrim& p, Box& b, int& nd, int& digits)
{
    nd = 0; digits = 0;
    switch (p.kind) {
    case EAGLE_PRIM_ARC: b = {p.a[0] - ARC_A, p.a[1] - ARC_B, p.a[0] + ARC_A, p.a[1] + ARC_B}; return true;
    case EAGLE_PRIM_DISC: b = {p.a[0] - p.a[2], p.a[1] - p.a[2], p.a[0] + p.a[2], p.a[1] + p.a[2]}; return true;
    case EAGLE_PRIM_TRI:
        b = {min(p.a[0], min(p.a[2], p.a[4])), min(p.a[1], min(p.a[3], p.a[5])), max(p.a[0], max(p.a[2], p.a[4])), max(p.a[1], max(p.a[3], p.a[5]))};
        return true;
    case EAGLE_PRIM_LABEL: {
        int id = p.a[2];
        if (id < 0 || id > LABEL_MAX_ID) return false;
        int rev[5];
        do { rev[nd++] = id % 10; id /= 10; } while (id);
        for (int k = 0; k < nd; ++k) digits |= rev[nd - 1 - k] << (4 * k);
        b = {p.a[0] - 3, p.a[1] - (GLYPH_H - 1), p.a[0] - 3 + GLYPH_ADV * nd - 3, p.a[1]};
        return true;
    }
    }
    return false;
}

__device__ __forceinline__ bool covers(const TilePrim& p, int kind, int px, int py)
{
    if (kind == EAGLE_PRIM_ARC) {
        const int dx = px - p.a[0], dy = py - p.a[1], ax = abs(dx), ay = abs(dy);
        if (ax > ARC_A || ay > ARC_B) return false;
        const int bb = ARC_B * ARC_B, aa = ARC_A * ARC_A, f = bb * dx * dx + aa * dy * dy - aa * bb;
        if (f > 0) return false;
        // F grows with |dx| and with |dy|: an edge neighbour is outside iff the one further from the centre is
        if (bb * (ax + 1) * (ax + 1) + aa * dy * dy - aa * bb <= 0 && bb * dx * dx + aa * (ay + 1) * (ay + 1) - aa * bb <= 0) return false;
        // the gap: cross(d1, p) > 0 and cross(p, d2) > 0 with p = (b dx, a dy), d1 = (-7, -10), d2 = (1, -1)
        return !(10 * ARC_B * dx - 7 * ARC_A * dy > 0 && -ARC_B * dx - ARC_A * dy > 0);
    }
    if (kind == EAGLE_PRIM_DISC) {
        const int dx = px - p.a[0], dy = py - p.a[1];
        if (abs(dx) > p.a[2] || abs(dy) > p.a[2]) return false;
        return dx * dx + dy * dy <= p.a[2] * p.a[2];
    }
    if (kind == EAGLE_PRIM_LABEL) {
        const int ux = px - (p.a[0] - 3), uy = py - (p.a[1] - (GLYPH_H - 1));
        if (ux < 0 || uy < 0 || uy >= GLYPH_H || ux >= GLYPH_ADV * p.a[3]) return false;
        const int k = ux / GLYPH_ADV, gx = ux - k * GLYPH_ADV;
        if (gx >= GLYPH_W) return false;
        return (c_font[(p.a[4] >> (4 * k)) & 15][uy >> 1] >> (4 - (gx >> 1))) & 1;
    }
    // EAGLE_PRIM_TRI: the caller has checked the bounding box.  |coordinate| <= 2^20: the edge functions need 64 bits
    const long long x0 = p.a[0], y0 = p.a[1], x1 = p.a[2], y1 = p.a[3], x2 = p.a[4], y2 = p.a[5], X = px, Y = py;
    const bool neg = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) < 0;
    long long e0 = (x1 - x0) * (Y - y0) - (y1 - y0) * (X - x0), e1 = (x2 - x1) * (Y - y1) - (y2 - y1) * (X - x1), e2 = (x0 - x2) * (Y - y2) - (y0 - y2) * (X - x2);
    if (neg) { e0 = -e0; e1 = -e1; e2 = -e2; }
    return e0 >= 0 && e1 >= 0 && e2 >= 0;
}

// 24 bytes = 6 little-endian words <-> 8 pixels B | G << 8 | R << 16
__device__ __forceinline__ void unpack8(const uint32_t* w, uint32_t* px)
{
    #pragma unroll
    for (int q = 0; q < 2; ++q) {
        const uint32_t w0 = w[3 * q], w1 = w[3 * q + 1], w2 = w[3 * q + 2];
        px[4 * q] = w0 & 0xffffffu; px[4 * q + 1] = (w0 >> 24) | (w1 & 0xffffu) << 8; px[4 * q + 2] = (w1 >> 16) | (w2 & 0xffu) << 16; px[4 * q + 3] = w2 >> 8;
    }
}
__global__ __launch_bounds__(AN_THREADS) void annotate_kernel(AnnotArgs a)
{
    __shared__ TilePrim s_list[EAGLE_MAX_PRIMS];
    __shared__ int s_wcnt[AN_THREADS / 64];
    const int tiles_x = (a.w + AN_TW - 1) / AN_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, f = blockIdx.y;
    const int tx0 = tx * AN_TW, ty0 = ty * AN_TH, tx1 = min(tx0 + AN_TW, a.w) - 1, ty1 = min(ty0 + AN_TH, a.h) - 1;

    // ---- cull the frame's list against the tile, keeping list order ----
    const int p0 = a.offs[f], p1 = a.offs[f + 1];
    int n_list = 0;
    for (int base = p0; base < p1; base += AN_THREADS) {          // (uniform: every thread of the workgroup takes every trip)
        const int i = base + (int)threadIdx.x;
        bool keep = false;
        TilePrim tp;
        if (i < p1) {
            const EaglePrim p = a.prims[i];
            Box b; int nd, digits;
            if (prim_box(p, b, nd, digits)) {
                b.x0 = max(b.x0, tx0); b.y0 = max(b.y0, ty0); b.x1 = min(b.x1, tx1); b.y1 = min(b.y1, ty1);
                if (b.x0 <= b.x1 && b.y0 <= b.y1) {
                    keep = true;
                    #pragma unroll
                    for (int k = 0; k < 6; ++k) tp.a[k] = p.a[k];
                    if (p.kind == EAGLE_PRIM_LABEL) { tp.a[3] = nd; tp.a[4] = digits; }
                    tp.kc = (uint32_t)p.b | (uint32_t)p.g << 8 | (uint32_t)p.r << 16 | (uint32_t)p.kind << 24;
                    tp.bx = (uint32_t)b.x0 | (uint32_t)b.x1 << 16; tp.by = (uint32_t)b.y0 | (uint32_t)b.y1 << 16;
                }
            }
        }
        const unsigned long long m = __ballot(keep);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (lane == 0) s_wcnt[wv] = __popcll(m);
        __syncthreads();
        int off = n_list, tot = 0;
        #pragma unroll
        for (int k = 0; k < AN_THREADS / 64; ++k) { const int c = s_wcnt[k]; tot += c; if (k < wv) off += c; }
        if (keep) s_list[off + __popcll(m & ((1ull << lane) - 1ull))] = tp;
        n_list += tot;
        __syncthreads();
    }

    const int sx = threadIdx.x % AN_SX, sy = threadIdx.x / AN_SX;
    const int x0 = tx0 + sx * AN_STRIP, y0 = ty0 + 2 * sy;
    if (x0 >= a.w || y0 >= a.h) return;
    const int cnt = min(AN_STRIP, a.w - x0), rows = min(2, a.h - y0);        // 4:2:0: cnt even, rows = 2

    // ---- the strip's pixels ----
    uint32_t px[2][AN_STRIP];
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
        #pragma unroll
        for (int k = 0; k < AN_STRIP; ++k) px[r][k] = 0;
        if (r >= rows) continue;
        const uint8_t* s = a.src + (((int64_t)f * a.h + y0 + r) * a.w + x0) * 3;
        const uintptr_t sa = (uintptr_t)s;
        if (cnt == AN_STRIP && (sa & 3) == 0) {
            uint32_t w[6];
            if ((sa & 7) == 0) {
                const uint2* v = (const uint2*)s;
                const uint2 v0 = v[0], v1 = v[1], v2 = v[2];
                w[0] = v0.x; w[1] = v0.y; w[2] = v1.x; w[3] = v1.y; w[4] = v2.x; w[5] = v2.y;
            } else {
                #pragma unroll
                for (int k = 0; k < 6; ++k) w[k] = ((const uint32_t*)s)[k];
            }
            unpack8(w, px[r]);
        } else {
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k)
                if (k < cnt) px[r][k] = (uint32_t)s[3 * k] | (uint32_t)s[3 * k + 1] << 8 | (uint32_t)s[3 * k + 2] << 16;
        }
    }

    // ---- the culled primitives, in list order (an empty list: no loop at all) ----
    for (int i = 0; i < n_list; ++i) {
        const TilePrim& p = s_list[i];
        const int bx0 = p.bx & 0xffff, bx1 = p.bx >> 16, by0 = p.by & 0xffff, by1 = p.by >> 16;
        if (bx1 < x0 || bx0 >= x0 + AN_STRIP || by1 < y0 || by0 > y0 + 1) continue;
        const int kind = p.kc >> 24;
        const uint32_t color = p.kc & 0xffffffu;
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (y0 + r < by0 || y0 + r > by1) continue;
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k)
                if (x0 + k >= bx0 && x0 + k <= bx1 && covers(p, kind, x0 + k, y0 + r)) px[r][k] = color;
        }
    }

    write_strip(a, f, x0, y0, cnt, rows, px);
}

void annotate_launch(const AnnotArgs& args, int n, hipStream_t s)
{
    if (n <= 0) return;
    AnnotArgs a = args;
    const int tiles = (a.w + AN_TW - 1) / AN_TW * ((a.h + AN_TH - 1) / AN_TH);
    for (int f0 = 0; f0 < n; f0 += 65535) {          // gridDim.y limit
        const int nf = std::min(n - f0, 65535);
        hipLaunchKernelGGL(annotate_kernel, dim3(tiles, nf), dim3(AN_THREADS), 0, s, a);
        HIP_CHECK(hipGetLastError());
        a.src += (int64_t)nf * a.h * a.w * 3;
        a.dst += (int64_t)nf * a.frame_stride;
        a.offs += nf;
    }
}

// ---- host: what a record's picture is ----------------------------------------------------------------------------------------------
static EaglePrim make_prim(int kind, int a0, int a1, int a2, int a3, int a4, int a5, const uint8_t* bgr)
{
    EaglePrim p{};
    p.kind = kind;
    p.a[0] = a0; p.a[1] = a1; p.a[2] = a2; p.a[3] = a3; p.a[4] = a4; p.a[5] = a5;
    p.b = bgr[0]; p.g = bgr[1]; p.r = bgr[2];
    return p;
}
static bool in_domain(int x, int y) { return std::abs((long long)x) <= COORD_MAX - 64 && std::abs((long long)y) <= COORD_MAX - 64; }

int overlay_from_record(const EagleFrameResult& rec, const int32_t* team_ids, const int32_t* team_vals, int n_team, EaglePrim* out)
{
    static const uint8_t green[3] = {0, 255, 0}, red[3] = {0, 0, 255}, blue[3] = {255, 0, 0}, white[3] = {255, 255, 255}, black[3] = {0, 0, 0};
    int n = 0;
    const int nd = std::max(0, std::min(rec.n_det, EAGLE_MAX_DET)), nk = std::max(0, std::min(rec.n_kp, EAGLE_MAX_KP));
    // 1. persons, in detection order (main.py:59-73): green goalkeepers, team 0 red, any other team blue, players the mapping does not know skipped
    for (int i = 0; i < nd; ++i) {
        const EagleDet& d = rec.det[i];
        if (!d.reported || (d.cls != 0 && d.cls != 1)) continue;
        const uint8_t* color = green;
        if (d.cls == 0) {
            if (!team_ids) color = white;
            else {
                int k = 0;
                while (k < n_team && team_ids[k] != d.id) ++k;
                if (k == n_team) continue;
                color = team_vals[k] == 0 ? red : blue;
            }
        }
        if (!in_domain(d.foot_x, d.foot_y)) continue;
        out[n++] = make_prim(EAGLE_PRIM_ARC, d.foot_x, d.foot_y, 0, 0, 0, 0, color);
        out[n++] = make_prim(EAGLE_PRIM_LABEL, d.foot_x, d.foot_y, d.id, 0, 0, 0, color);
    }
    // 2. the first reported ball (NMS order: the most confident), main.py:52-58
    for (int i = 0; i < nd; ++i) {
        const EagleDet& d = rec.det[i];
        if (!d.reported || d.cls != 2) continue;
        if (in_domain(d.foot_x, d.foot_y))
            out[n++] = make_prim(EAGLE_PRIM_TRI, d.foot_x, d.foot_y - 20, d.foot_x - 5, d.foot_y - 30, d.foot_x + 5, d.foot_y - 30, green);
        break;
    }
    // 3. the key-points of the reference dict (records.py: the RANSAC inliers when H_valid, else all; one per label, the last entry of a label holding its
    //    value at the label's first position), main.py:75-77
    int first[EAGLE_MAX_KP], last[EAGLE_MAX_KP], nl = 0;
    for (int i = 0; i < nk; ++i) {
        const EagleKeypoint& k = rec.kp[i];
        if (rec.H_valid && !(k.on_plane && k.inlier)) continue;
        int j = 0;
        while (j < nl && rec.kp[first[j]].label != k.label) ++j;
        if (j == nl) first[nl++] = i;
        last[j] = i;
    }
    for (int j = 0; j < nl; ++j) {
        const EagleKeypoint& k = rec.kp[last[j]];
        if (in_domain(k.x, k.y)) out[n++] = make_prim(EAGLE_PRIM_DISC, k.x, k.y, 6, 0, 0, 0, black);
    }
    return n;
}

void check_prims(const EaglePrim* prims, const int32_t* offs, int n)
{
    if (offs[0] < 0) fail(EAGLE_E_INVALID, "prim_offsets[0] = %d is negative", offs[0]);
    for (int f = 0; f < n; ++f) {
        if (offs[f + 1] < offs[f]) fail(EAGLE_E_INVALID, "prim_offsets decrease at frame %d", f);
        if (offs[f + 1] - offs[f] > EAGLE_MAX_PRIMS) fail(EAGLE_E_INVALID, "frame %d has %d primitives (at most EAGLE_MAX_PRIMS = %d)", f, offs[f + 1] - offs[f], EAGLE_MAX_PRIMS);
    }
    for (int i = offs[0]; i < offs[n]; ++i) {
        const EaglePrim& p = prims[i];
        if (p.kind < EAGLE_PRIM_ARC || p.kind > EAGLE_PRIM_TRI) fail(EAGLE_E_INVALID, "primitive %d: unknown kind %d", i, p.kind);
        const int nc = p.kind == EAGLE_PRIM_TRI ? 6 : 2;
        for (int k = 0; k < nc; ++k)
            if (p.a[k] < -COORD_MAX || p.a[k] > COORD_MAX) fail(EAGLE_E_INVALID, "primitive %d: coordinate %d is outside +-2^20", i, p.a[k]);
        if (p.kind == EAGLE_PRIM_DISC && (p.a[2] < 0 || p.a[2] > RADIUS_MAX)) fail(EAGLE_E_INVALID, "primitive %d: radius %d is outside 0 .. %d", i, p.a[2], RADIUS_MAX);
    }
}

// the kernel's view of an output layout the one check (yuv_geometry) has resolved
AnnotArgs annot_args(const YuvGeom& g, const uint8_t* src, uint8_t* dst, const EaglePrim* prims, const int32_t* offs)
{
    if (g.h > AN_MAX_DIM || g.w > AN_MAX_DIM) fail(EAGLE_E_INVALID, "frames of %d x %d are beyond the %d pixels per side annotated output handles", g.w, g.h, AN_MAX_DIM);
    AnnotArgs a{};
    const bool nv12 = g.fmt == EAGLE_PIX_NV12;
    a.src = src; a.dst = dst; a.prims = prims; a.offs = offs; a.h = g.h; a.w = g.w; a.fmt = g.fmt;
    a.frame_stride = g.frame_stride; a.y_pitch = g.y_pitch; a.c_offset = g.c_offset; a.c_pitch = g.c_pitch;
    a.v_offset = nv12 ? g.c_offset + 1 : g.v_offset;
    a.c_step = nv12 ? 2 : 1;
    if (g.fmt != EAGLE_PIX_BGR) {
        const uint64_t al = (uint64_t)(uintptr_t)dst | (uint64_t)g.frame_stride | (uint64_t)g.y_pitch;                // 8-byte Y stores
        const uint64_t ac = nv12 ? ((uint64_t)g.c_offset | (uint64_t)g.c_pitch) & 7                                   // 8-byte UV stores
                                 : ((uint64_t)g.c_offset | (uint64_t)g.c_pitch | (uint64_t)g.v_offset) & 3;           // 4-byte U and V stores
        a.vec = (al & 7) == 0 && ac == 0;
    }
    return a;
}

// algorithmic bytes per pixel: the BGR frame read once + the output written once
static double annot_bytes_per_px(int fmt) { return 3.0 + (fmt == EAGLE_PIX_BGR ? 3.0 : 1.5); }

static void upload_prims(EagleHandle* h, const std::vector<EaglePrim>& prims, const std::vector<int32_t>& offs, const EaglePrim** d_prims, const int32_t** d_offs);
// the primitive lists of n records -> the handle's device buffer: [EaglePrim x total][int32 x (n + 1)], on s_main
static void upload_overlays(EagleHandle* h, const EagleFrameResult* recs, int n, const int32_t* team_ids, const int32_t* team_vals, int n_team,
                            const EaglePrim** d_prims, const int32_t** d_offs)
{
    std::vector<EaglePrim> prims;
    std::vector<int32_t> offs(n + 1, 0);
    EaglePrim one[EAGLE_MAX_PRIMS];
    for (int i = 0; i < n; ++i) {
        const int k = overlay_from_record(recs[i], team_ids, team_vals, n_team, one);
        prims.insert(prims.end(), one, one + k);
        offs[i + 1] = (int32_t)prims.size();
    }
    upload_prims(h, prims, offs, d_prims, d_offs);
}
// ... and any primitive lists (frame k owns prims[offs[k] .. offs[k + 1]))
static void upload_prims(EagleHandle* h, const std::vector<EaglePrim>& prims, const std::vector<int32_t>& offs, const EaglePrim** d_prims, const int32_t** d_offs)
{
    const size_t pb = prims.size() * sizeof(EaglePrim), need = pb + offs.size() * sizeof(int32_t);
    if (need > h->annot_prims_cap) {
        if (h->annot_prims) HIP_CHECK(hipFree(h->annot_prims));
        h->annot_prims = nullptr; h->annot_prims_cap = 0;
        HIP_CHECK(hipMalloc(&h->annot_prims, need * 2));
        h->annot_prims_cap = need * 2;
    }
    // (pageable sources: each copy has left the host vector when the call returns)
    if (pb) HIP_CHECK(hipMemcpyAsync(h->annot_prims, prims.data(), pb, hipMemcpyHostToDevice, h->s_main));
    HIP_CHECK(hipMemcpyAsync((char*)h->annot_prims + pb, offs.data(), offs.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->s_main));
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    *d_prims = (const EaglePrim*)h->annot_prims;
    *d_offs = (const int32_t*)((const char*)h->annot_prims + pb);
}

static void annotate_begin(EagleHandle* h, const void* d_bgr, int n, const EagleFrameResult* recs, const int32_t* team_ids, const int32_t* team_vals,
                           int n_team, const void* out)
{
    if (!d_bgr || !out || n < 0 || (n > 0 && !recs) || n_team < 0 || (team_ids && n_team > 0 && !team_vals)) fail(EAGLE_E_INVALID, "bad argument");
    HIP_CHECK(hipSetDevice(h->cfg.device));
}

// frames [0, n) of d_bgr -> d_out (layout g), one launch on s_main; returns when it is done
static void annotate_device(EagleHandle* h, const uint8_t* d_bgr, int n, const EaglePrim* d_prims, const int32_t* d_offs, const YuvGeom& g, uint8_t* d_out)
{
    timed_launch(h, "annotate", (double)n * g.h * g.w * annot_bytes_per_px(g.fmt), h->s_main,
                 [&] { annotate_launch(annot_args(g, d_bgr, d_out, d_prims, d_offs), n, h->s_main); });
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    if (h->prof) collect_spans(h);
}

void frames_to_host(EagleHandle* h, int n, int fh, int fw, int batch, int out_format, const EagleYuvLayout* out_layout, uint8_t* out,
                    const std::function<void(int, int, const YuvGeom&, uint8_t*)>& draw)
{
    const YuvGeom g = yuv_geometry(out_format, fh, fw, out_layout, true);          // the caller's layout
    const YuvGeom dg = yuv_geometry(out_format, fh, fw, nullptr, true);            // what the kernel writes: dense frames in the handle's staging
    const bool pinned = host_pinned(h, out);
    const int B = std::max(1, batch);
    const size_t fsz = (size_t)dg.dense_bytes, need = fsz * B;
    if (need > h->annot_out_cap) {
        if (h->annot_out) HIP_CHECK(hipFree(h->annot_out));
        h->annot_out = nullptr; h->annot_out_cap = 0;
        HIP_CHECK(hipMalloc((void**)&h->annot_out, need));
        h->annot_out_cap = need;
    }
    if (!pinned && need > h->annot_ring_cap) {
        if (h->annot_ring) HIP_CHECK(hipHostFree(h->annot_ring));
        h->annot_ring = nullptr; h->annot_ring_cap = 0;
        HIP_CHECK(hipHostMalloc((void**)&h->annot_ring, need, hipHostMallocDefault));
        h->annot_ring_cap = need;
    }
    for (int i = 0; i < n; i += B) {
        const int na = std::min(B, n - i);
        draw(i, na, dg, h->annot_out);
        uint8_t* dst = out + (size_t)i * g.frame_stride;
        if (pinned && g.dense) {
            HIP_CHECK(hipMemcpyAsync(dst, h->annot_out, fsz * na, hipMemcpyDeviceToHost, h->s_main));
        } else if (pinned) {
            for (int k = 0; k < na; ++k)
                for (int q = 0; q < g.nplanes; ++q)
                    HIP_CHECK(hipMemcpy2DAsync(dst + (size_t)k * g.frame_stride + g.pl[q].off, (size_t)g.pl[q].pitch, h->annot_out + (size_t)k * fsz + g.pl[q].dense_off,
                                               (size_t)g.pl[q].row_bytes, (size_t)g.pl[q].row_bytes, (size_t)g.pl[q].rows, hipMemcpyDeviceToHost, h->s_main));
        } else {
            HIP_CHECK(hipMemcpyAsync(h->annot_ring, h->annot_out, fsz * na, hipMemcpyDeviceToHost, h->s_main));
        }
        HIP_CHECK(hipStreamSynchronize(h->s_main));
        if (!pinned)
            h->pool->run(na * g.nplanes, [&](int t) {
                const int k = t / g.nplanes;
                const HostPlane& p = g.pl[t % g.nplanes];
                const uint8_t* s0 = h->annot_ring + (size_t)k * fsz + p.dense_off;
                uint8_t* d0 = dst + (size_t)k * g.frame_stride + p.off;
                if (p.pitch == p.row_bytes) memcpy(d0, s0, (size_t)(p.rows * p.row_bytes));
                else for (int64_t r = 0; r < p.rows; ++r) memcpy(d0 + r * p.pitch, s0 + r * p.row_bytes, (size_t)p.row_bytes);
            });
    }
}

}  // namespace eagle

extern "C" {

int eagle_overlay_from_record(const EagleFrameResult* rec, const int32_t* team_ids, const int32_t* team_vals, int n_team, EaglePrim* out, int cap, int* n_out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!rec || !out || !n_out || cap < 0 || n_team < 0 || (team_ids && n_team > 0 && !team_vals)) fail(EAGLE_E_INVALID, "bad argument");
    EaglePrim one[EAGLE_MAX_PRIMS];
    const int n = overlay_from_record(*rec, team_ids, team_vals, n_team, one);
    if (n > cap) fail(EAGLE_E_INVALID, "the record's overlay has %d primitives, cap is %d (EAGLE_MAX_PRIMS = %d always suffices)", n, cap, EAGLE_MAX_PRIMS);
    memcpy(out, one, (size_t)n * sizeof(EaglePrim));
    *n_out = n;
    API_END(hh)
}

int eagle_annotate_device_frames(EagleHandle* h, const void* d_bgr, int n, const EagleFrameResult* recs, const int32_t* team_ids, const int32_t* team_vals,
                                 int n_team, int out_format, const EagleYuvLayout* out_layout, void* d_out)
{
    API_BEGIN_H(h)
    annotate_begin(h, d_bgr, n, recs, team_ids, team_vals, n_team, d_out);
    const YuvGeom g = yuv_geometry(out_format, h->cfg.frame_h, h->cfg.frame_w, out_layout, true);
    if (n == 0) return EAGLE_OK;
    const EaglePrim* dp; const int32_t* dof;
    upload_overlays(h, recs, n, team_ids, team_vals, n_team, &dp, &dof);
    annotate_device(h, (const uint8_t*)d_bgr, n, dp, dof, g, (uint8_t*)d_out);
    API_END(h)
}

// n frames drawn with the uploaded primitive lists -> host memory in the caller's layout
static void annotate_to_host(EagleHandle* h, const void* d_bgr, int n, const EaglePrim* dp, const int32_t* dof, int out_format, const EagleYuvLayout* out_layout, uint8_t* out)
{
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    frames_to_host(h, n, fh, fw, h->cfg.batch, out_format, out_layout, out, [&](int i, int na, const YuvGeom& dg, uint8_t* d_dst) {
        annotate_device(h, (const uint8_t*)d_bgr + (size_t)i * fh * fw * 3, na, dp, dof + i, dg, d_dst);
    });
}

int eagle_annotate_frames(EagleHandle* h, const void* d_bgr, int n, const EagleFrameResult* recs, const int32_t* team_ids, const int32_t* team_vals, int n_team,
                          int out_format, const EagleYuvLayout* out_layout, uint8_t* out)
{
    API_BEGIN_H(h)
    annotate_begin(h, d_bgr, n, recs, team_ids, team_vals, n_team, out);
    (void)yuv_geometry(out_format, h->cfg.frame_h, h->cfg.frame_w, out_layout, true);
    if (n == 0) return EAGLE_OK;
    const EaglePrim* dp; const int32_t* dof;
    upload_overlays(h, recs, n, team_ids, team_vals, n_team, &dp, &dof);
    annotate_to_host(h, d_bgr, n, dp, dof, out_format, out_layout, out);
    API_END(h)
}

int eagle_annotate_frames_prims(EagleHandle* h, const void* d_bgr, int n, const EaglePrim* prims, const int32_t* prim_offsets, int out_format,
                                const EagleYuvLayout* out_layout, uint8_t* out)
{
    API_BEGIN_H(h)
    if (!d_bgr || !out || n < 0 || !prim_offsets || (n > 0 && prim_offsets[n] > prim_offsets[0] && !prims)) fail(EAGLE_E_INVALID, "bad argument");
    HIP_CHECK(hipSetDevice(h->cfg.device));
    (void)yuv_geometry(out_format, h->cfg.frame_h, h->cfg.frame_w, out_layout, true);
    check_prims(prims, prim_offsets, n);
    if (n == 0) return EAGLE_OK;
    std::vector<int32_t> offs(prim_offsets, prim_offsets + n + 1);
    for (int32_t& v : offs) v -= prim_offsets[0];
    const std::vector<EaglePrim> list(prims ? prims + prim_offsets[0] : nullptr, prims ? prims + prim_offsets[n] : nullptr);
    const EaglePrim* dp; const int32_t* dof;
    upload_prims(h, list, offs, &dp, &dof);
    annotate_to_host(h, d_bgr, n, dp, dof, out_format, out_layout, out);
    API_END(h)
}

int eagle_op_annotate(int device, const uint8_t* bgr, int n, int h, int w, const EaglePrim* prims, const int32_t* prim_offsets, int out_format,
                      const EagleYuvLayout* out_layout, uint8_t* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!bgr || !out || n < 0 || !prim_offsets || (n > 0 && prim_offsets[n] > 0 && !prims)) fail(EAGLE_E_INVALID, "bad argument");
    const YuvGeom g = yuv_geometry(out_format, h, w, out_layout, true);
    check_prims(prims, prim_offsets, n);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const size_t span = (size_t)((n - 1) * g.frame_stride + g.extent);      // exactly the bytes the output frames span
    const uint8_t* d = (const uint8_t*)net.upload(bgr, (size_t)n * h * w * 3);
    uint8_t* o = (uint8_t*)net.upload(out, span);                           // bytes the layout does not cover come back as they were
    const int32_t base = prim_offsets[0];
    std::vector<int32_t> offs(prim_offsets, prim_offsets + n + 1);
    for (int32_t& v : offs) v -= base;
    const EaglePrim* dp = (const EaglePrim*)net.upload(prims ? prims + base : (const EaglePrim*)offs.data(), (size_t)offs[n] * sizeof(EaglePrim));
    const int32_t* dof = (const int32_t*)net.upload(offs.data(), offs.size() * sizeof(int32_t));
    annotate_launch(annot_args(g, d, o, dp, dof), n, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, o, span, hipMemcpyDeviceToHost));
    API_END(hh)
}

}  // extern "C"
