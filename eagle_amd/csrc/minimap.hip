// K21 — the minimap: rows of a processed table resident in HBM (post.hip) -> top-down pictures of the pitch, written as BGR, NV12 or I420 in the layout a
// video encoder takes: the camera's footprint, the players in team colours, the ball and, on request, the Voronoi areas of the players (what the
// reference's examples/minimap.py and examples/voronoi.py plot through matplotlib).  tests/minimap_ref.py is the written definition of every output byte
// (own rasterisation; one float64 quantisation to 1/16 pixel, integer arithmetic after it).
//
// Two launches per call, no host round trip for the data:
//   minimap_sites_kernel  one thread per table row walks the drawable pitch columns (the host decides per COLUMN what is drawn and in which colour: the
//                         team lookup does not depend on the row) and writes the row's compacted draw list in drawing order (discs in column order, then the
//                         balls): quantised position + colour / kind / is-a-Voronoi-site, 16 bytes per entry, behind a header of the entry count and the four
//                         quantised footprint corners.  The table is [column][row][2]: a wave's loads are contiguous along rows.  Its stores are not:
//                         each thread writes its own row's list, `stride` x 16 bytes from its neighbour's (16 B per lane and instruction, uncoalesced).  Against
//                         the draw pass this is nothing at tens of columns; a table of thousands of columns would want the list transposed.
//   minimap_kernel        annotate_kernel's shape: a workgroup owns an AN_TH x AN_TW tile of one picture, a thread a 2-row strip of AN_STRIP pixels in
//                         registers; the row's list goes through LDS in chunks of MM_CHUNK entries (any length is exact), once for the Voronoi labelling
//                         (every site counts for every pixel) and once for the discs and rings (culled against the tile by bounding box, list order kept);
//                         the markings are a bit mask built once per (scale, margin) by markings_mask below; the strip leaves through pix_out.h's writer.
// Voronoi without 64-bit multiplies per pixel: (16X - qx)^2 + (16Y - qy)^2 = 256 (X^2 + Y^2) + [qx^2 + qy^2 - 32 X qx - 32 Y qy]; the first term is the
// same for every site, so the sites are compared by the bracket: its constant is formed once per staged entry, the Y term once per strip row, and along a
// row it changes by the 32-bit amount 32 qx per pixel.  Exact: |q| < 2^20 and 32 X < 2^17 keep everything below 2^42.
#include "trails.h"
#include "pix_out.h"

namespace eagle {

static constexpr int MM_CHUNK = AN_THREADS;            // list entries staged per trip: one per thread
static constexpr int MM_TINT_A = 51, MM_FOOT_A = 77, MM_DIM_A = 64;
static constexpr double MM_CIRCLE_R = 9.15;

struct MinimapArgs {
    AnnotArgs out;               // (src, prims, offs unused)
    const double2* values;       // the table, [column][row]
    const MmCol* cols;           // drawable columns in drawing order
    int4* lists;                 // [n][stride]
    const uint8_t* mask;         // markings: bit (x & 7) of byte y * mask_pitch + (x >> 3)
    int rows, row0, n, ncols, stride, mask_pitch;
    int corner[4];               // table columns of Bottom_Left, Top_Left, Top_Right, Bottom_Right (-1: none)
    int scale, margin, voronoi, footprint;
    int r16, rb16, rbi16;        // 16 x the disc radius, the ring's outer and inner radius
    const uint8_t* grid;         // control layer: [n][gh][gw] bytes of control.hip for the rows of this launch (nullptr: layer off)
    int ctl_R, ctl_gw, ctl_gh;   // cells per metre and the grid's size
};

// LAYERS: the instantiation the K25 layers run (la: owner and dim bits of the entries); the plain one is the code it was before them
template <bool LAYERS>
__device__ __forceinline__ void mm_sites(const MinimapArgs& m, const MmLayerArgs* la)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m.n) return;
    const size_t row = (size_t)(m.row0 + i);
    const double K = (double)(16 * m.scale);
    const int ox = 16 * m.margin, oy = 16 * m.margin + 16 * 68 * m.scale;
    int4* L = m.lists + (size_t)i * m.stride;
    int cnt = 0;
    for (int c = 0; c < m.ncols; ++c) {
        const MmCol d = m.cols[c];
        int qx, qy;
        if (!mm_quantise(m.values[(size_t)d.col * m.rows + row], K, ox, oy, qx, qy)) continue;
        uint32_t kc = d.kc;
        if constexpr (LAYERS) {
            const bool person = (kc >> MM_KIND_SHIFT & 15) != EAGLE_POST_BALL;
            if (person && la->owner && la->owner[row] == d.col) kc |= MM_OWNER_BIT;
            if (person && la->dim && d.col != la->pass_from && d.col != la->pass_to) kc |= MM_DIM_BIT;
        }
        L[MM_HEAD + cnt++] = make_int4(qx, qy, (int)kc, 0);
    }
    int q[8];
    bool ok = true;
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
        q[2 * k] = q[2 * k + 1] = 0;
        ok = ok && m.corner[k] >= 0 && mm_quantise(m.values[(size_t)max(m.corner[k], 0) * m.rows + row], K, ox, oy, q[2 * k], q[2 * k + 1]);
    }
    L[0] = make_int4(cnt, ok ? 1 : 0, 0, 0);
    L[1] = make_int4(q[0], q[1], q[2], q[3]);
    L[2] = make_int4(q[4], q[5], q[6], q[7]);
}

__global__ __launch_bounds__(256) void minimap_sites_kernel(MinimapArgs m) { mm_sites<false>(m, nullptr); }
__global__ __launch_bounds__(256) void minimap_sites_layers_kernel(MinimapArgs m, MmLayerArgs la) { mm_sites<true>(m, &la); }

__device__ __forceinline__ uint32_t mm_blend(uint32_t bg, uint32_t c, int a)
{
    uint32_t o = 0;
    #pragma unroll
    for (int s = 0; s < 24; s += 8) o |= ((((c >> s) & 255u) * a + ((bg >> s) & 255u) * (256 - a) + 128u) >> 8) << s;
    return o;
}

// the pixels of the strip at (x0, y0) a triangle covers (bit r * AN_STRIP + k): annot_ref's inclusive TRI rule on 1/16 px vertices at the pixel centres.
// The edge functions are affine: evaluated once in 64 bits at the strip's origin, stepped by additions
__device__ __forceinline__ uint32_t mm_tri_strip(int ax, int ay, int bx, int by, int cx, int cy, int x0, int y0)
{
    const int lx = min(ax, min(bx, cx)), hx = max(ax, max(bx, cx)), ly = min(ay, min(by, cy)), hy = max(ay, max(by, cy));
    const int X = 16 * x0, Y = 16 * y0;
    if (X + 16 * (AN_STRIP - 1) < lx || X > hx || Y + 16 < ly || Y > hy) return 0;
    const long long sg = (long long)(bx - ax) * (cy - ay) - (long long)(by - ay) * (cx - ax) < 0 ? -1 : 1;
    const int vx[3] = {ax, bx, cx}, vy[3] = {ay, by, cy};
    long long e[3], sx[3], sy[3];
    #pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ux = vx[(k + 1) % 3] - vx[k], uy = vy[(k + 1) % 3] - vy[k];
        e[k] = sg * ((long long)ux * (Y - vy[k]) - (long long)uy * (X - vx[k]));
        sx[k] = -sg * 16 * (long long)uy;
        sy[k] = sg * 16 * (long long)ux;
    }
    uint32_t bits = 0;
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (Y + 16 * r < ly || Y + 16 * r > hy) continue;
        #pragma unroll
        for (int k = 0; k < AN_STRIP; ++k) {
            const int px = X + 16 * k;
            if (px >= lx && px <= hx && e[0] + r * sy[0] + k * sx[0] >= 0 && e[1] + r * sy[1] + k * sx[1] >= 0 && e[2] + r * sy[2] + k * sx[2] >= 0)
                bits |= 1u << (r * AN_STRIP + k);
        }
    }
    return bits;
}

// the pixels of the strip at (x0, y0) a capsule covers (tests/trails_ref.py, CAPSULE): squared distance to the segment A B <= hw^2, exactly.  t = (P - A).d and
// cross = (P - A) x d are affine in the pixel: evaluated once in 64 bits at the strip's origin and stepped by additions (|q| < 2^20: both stay below 2^42).
// Between the end points a pixel is first rejected in 64 bits by |cross| > hw (|dx| + |dy|) (sufficient: |d| <= |dx| + |dy|), and only then cross^2 is
// formed as a 128-bit product (high and low half) and compared with hw^2 L2 < 2^57.  (After that reject |cross| < 2^29, so the high half is 0 here; the
// full form is kept so that the comparison stays exact if the reject is ever loosened.)  The end caps are discs: 32-bit once |P - end| <= hw per axis
__device__ __forceinline__ uint32_t mm_capsule_strip(int ax, int ay, int bx, int by, int hw, int x0, int y0)
{
    const int X = 16 * x0, Y = 16 * y0;
    if (X + 16 * (AN_STRIP - 1) < min(ax, bx) - hw || X > max(ax, bx) + hw || Y + 16 < min(ay, by) - hw || Y > max(ay, by) + hw) return 0;
    const int dxi = bx - ax, dyi = by - ay, hw2 = hw * hw;
    const long long dx = dxi, dy = dyi, L2 = dx * dx + dy * dy;
    const long long lim = (long long)hw * (llabs(dx) + llabs(dy));
    const unsigned long long rhs = (unsigned long long)hw2 * (unsigned long long)L2;
    long long t_row = (long long)(X - ax) * dx + (long long)(Y - ay) * dy, c_row = (long long)(X - ax) * dy - (long long)(Y - ay) * dx;
    uint32_t bits = 0;
    #pragma unroll
    for (int r = 0; r < 2; ++r) {
        long long t = t_row, c = c_row;
        const int py = Y + 16 * r - ay;
        #pragma unroll
        for (int k = 0; k < AN_STRIP; ++k) {
            const int px = X + 16 * k - ax;
            bool cov;
            if (t <= 0) cov = abs(px) <= hw && abs(py) <= hw && px * px + py * py <= hw2;
            else if (t >= L2) {
                const int qx = px - dxi, qy = py - dyi;
                cov = abs(qx) <= hw && abs(qy) <= hw && qx * qx + qy * qy <= hw2;
            } else {
                const unsigned long long ac = (unsigned long long)llabs(c);
                cov = (long long)ac <= lim && __umul64hi(ac, ac) == 0 && ac * ac <= rhs;
            }
            if (cov) bits |= 1u << (r * AN_STRIP + k);
            t += 16 * dx; c += 16 * dy;
        }
        t_row += 16 * dy; c_row -= 16 * dx;
    }
    return bits;
}

__device__ __forceinline__ void mm_paint(uint32_t (&px)[2][AN_STRIP], uint32_t bits, uint32_t color)
{
    if (!bits) return;
    #pragma unroll
    for (int r = 0; r < 2; ++r)
        #pragma unroll
        for (int k = 0; k < AN_STRIP; ++k)
            if (bits >> (r * AN_STRIP + k) & 1) px[r][k] = color;
}

// LAYERS: the instantiation with the K25 sections (trails, pass arrows, owner ring, dimmed discs) compiled in, launched only when one of them is on; the
// plain instantiation is the kernel as it was before them
template <bool LAYERS>
__device__ __forceinline__ void mm_draw(const MinimapArgs& m, const MmLayerArgs* la)
{
    __shared__ int4 s_e[MM_CHUNK];
    __shared__ long long s_n[MM_CHUNK];
    __shared__ int4 s_f[LAYERS ? MM_CHUNK : 1], s_g[LAYERS ? MM_CHUNK : 1];
    const AnnotArgs& a = m.out;
    const int tiles_x = (a.w + AN_TW - 1) / AN_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, f = blockIdx.y;
    const int tx0 = tx * AN_TW, ty0 = ty * AN_TH, tx1 = min(tx0 + AN_TW, a.w) - 1, ty1 = min(ty0 + AN_TH, a.h) - 1;
    const int4* L = m.lists + (size_t)f * m.stride;
    const int4 head = L[0];
    const int count = head.x, tid = threadIdx.x;
    const int sx = tid % AN_SX, sy = tid / AN_SX;
    const int x0 = tx0 + sx * AN_STRIP, y0 = ty0 + 2 * sy;
    const bool live = x0 < a.w && y0 < a.h;            // (no early return: the workgroup meets at the barriers of the staging loops)
    const int cnt = min(AN_STRIP, a.w - x0), rows = min(2, a.h - y0);
    uint32_t px[2][AN_STRIP];
    #pragma unroll
    for (int r = 0; r < 2; ++r)
        #pragma unroll
        for (int k = 0; k < AN_STRIP; ++k) px[r][k] = 0;

    // ---- 2. Voronoi tint: every site of the row against every pixel of the pitch rectangle ----
    const int px_lo = m.margin, px_hi = m.margin + 105 * m.scale, py_lo = m.margin, py_hi = m.margin + 68 * m.scale;      // [lo, hi)
    if (m.voronoi && tx0 < px_hi && tx1 >= px_lo && ty0 < py_hi && ty1 >= py_lo) {      // (uniform)
        long long best[2][AN_STRIP];
        uint32_t who[2][AN_STRIP];
        #pragma unroll
        for (int r = 0; r < 2; ++r)
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k) { best[r][k] = 0x7fffffffffffffffLL; who[r][k] = MM_NONE; }
        for (int base = 0; base < count; base += MM_CHUNK) {
            const int nc = min(MM_CHUNK, count - base);
            __syncthreads();                           // the previous chunk has been consumed
            if (tid < nc) {
                const int4 e = L[MM_HEAD + base + tid];
                s_e[tid] = e;
                s_n[tid] = (long long)e.x * e.x + (long long)e.y * e.y;
            }
            __syncthreads();
            if (!live) continue;
            for (int j = 0; j < nc; ++j) {
                const int4 e = s_e[j];                 // (one address for the whole wave: an LDS broadcast)
                if (!(e.z & MM_SITE_BIT)) continue;
                const long long kx = s_n[j] - (long long)(32 * x0) * e.x;
                const int step = 32 * e.x;
                #pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const long long kr = kx - (long long)(32 * (y0 + r)) * e.y;
                    #pragma unroll
                    for (int k = 0; k < AN_STRIP; ++k) {
                        const long long key = kr - (long long)(k * step);
                        if (key < best[r][k]) { best[r][k] = key; who[r][k] = (uint32_t)e.z & MM_WHITE; }       // (strict: a tie stays with the earlier column)
                    }
                }
            }
        }
        #pragma unroll
        for (int r = 0; r < 2; ++r)
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k)
                if (who[r][k] != MM_NONE && x0 + k >= px_lo && x0 + k < px_hi && y0 + r >= py_lo && y0 + r < py_hi) px[r][k] = mm_blend(px[r][k], who[r][k], MM_TINT_A);
    }

    // ---- 2'. the pitch-control tint (in Voronoi's slot; never both): the byte of the pixel's cell, read from HBM (neighbouring pixels share cells and lines) ----
    if (m.grid && live && tx0 < px_hi && tx1 >= px_lo && ty0 < py_hi && ty1 >= py_lo) {
        const uint8_t* G = m.grid + (size_t)f * m.ctl_gw * m.ctl_gh;
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int Y = y0 + r;
            if (Y < py_lo || Y >= py_hi) continue;
            const uint8_t* Gr = G + (size_t)(m.ctl_gh - 1 - (Y - m.margin) * m.ctl_R / m.scale) * m.ctl_gw;
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k) {
                const int X = x0 + k;
                if (X < px_lo || X >= px_hi) continue;
                const uint32_t c = Gr[(X - m.margin) * m.ctl_R / m.scale], al = c + (c >> 7);
                // red a + blue (256 - a): B = (255 (256 - a) + 128) >> 8, G = 128 >> 8 = 0, R = (255 a + 128) >> 8
                const uint32_t color = ((255u * (256u - al) + 128u) >> 8) | ((255u * al + 128u) >> 8) << 16;
                px[r][k] = mm_blend(px[r][k], color, MM_TINT_A);
            }
        }
    }

    // ---- 3. the camera's footprint ----
    if (m.footprint && head.y && live) {
        const int4 c0 = L[1], c1 = L[2];               // BL, TL | TR, BR
        const uint32_t bits = mm_tri_strip(c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, x0, y0) | mm_tri_strip(c0.x, c0.y, c1.x, c1.y, c1.z, c1.w, x0, y0);
        if (bits) {
            #pragma unroll
            for (int r = 0; r < 2; ++r)
                #pragma unroll
                for (int k = 0; k < AN_STRIP; ++k)
                    if (bits >> (r * AN_STRIP + k) & 1) px[r][k] = mm_blend(px[r][k], MM_WHITE, MM_FOOT_A);
        }
    }

    // ---- 4. the markings ----
    if (live) {
        #pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= rows) continue;
            const uint32_t b = m.mask[(size_t)(y0 + r) * m.mask_pitch + (x0 >> 3)];
            #pragma unroll
            for (int k = 0; k < AN_STRIP; ++k)
                if (b >> k & 1) px[r][k] = MM_WHITE;
        }
    }

    if constexpr (LAYERS) {
        const int row = m.row0 + f, hw = la->hw16;
        // ---- 4.0 hulls (K26): the 2 x 32 edge slots of the picture in one staging trip, group 0 first; the trails' capsule in the layer's own width ----
        if (la->hull_edges) {                          // (uniform)
            static_assert(2 * EAGLE_SHAPE_HULL_CAP <= MM_CHUNK, "a picture's hull edges are staged in one trip");
            const int hh = la->hull_hw16;
            __syncthreads();
            if (tid < 2 * EAGLE_SHAPE_HULL_CAP) {
                const int4 e = la->hull_edges[(size_t)(row - la->range_row0) * (2 * EAGLE_SHAPE_HULL_CAP) + tid];
                const bool vis = e.x != MM_ABSENT && min(e.x, e.z) - hh <= 16 * tx1 && max(e.x, e.z) + hh >= 16 * tx0 && min(e.y, e.w) - hh <= 16 * ty1 &&
                                 max(e.y, e.w) + hh >= 16 * ty0;
                s_e[tid] = e;
                s_f[tid] = make_int4(tid < EAGLE_SHAPE_HULL_CAP ? 0x9f0000 : 0x00009f, vis, 0, 0);       // (255 * 160) >> 8 = 159 of red | blue
            }
            __syncthreads();
            if (live) {
                for (int j = 0; j < 2 * EAGLE_SHAPE_HULL_CAP; ++j) {
                    const int4 g = s_f[j];
                    if (!g.y) continue;                // (uniform)
                    const int4 e = s_e[j];
                    mm_paint(px, mm_capsule_strip(e.x, e.y, e.z, e.w, hh, x0, y0), (uint32_t)g.x);
                }
            }
        }
        // ---- 4a. trails: entry e of the picture is segment (j - 1, j) of selected column e / per, j = jlo + e % per, the oldest first ----
        if (la->nsel) {                                // (uniform)
            const int jlo = la->jlo >= 0 ? la->jlo : max(1, row - la->window + 1), per = max(0, row - jlo + 1), total = la->nsel * per;
            for (int base = 0; base < total; base += MM_CHUNK) {
                const int nc = min(MM_CHUNK, total - base);
                __syncthreads();
                if (tid < nc) {
                    const int e = base + tid, ci = e / per, j = jlo + (e - ci * per);
                    const int2* P = la->pts + (size_t)ci * la->prows + (j - la->prow0);
                    const int2 A = P[-1], B = P[0];
                    const bool vis = A.x != MM_ABSENT && B.x != MM_ABSENT && la->link[j - la->prow0] && min(A.x, B.x) - hw <= 16 * tx1 && max(A.x, B.x) + hw >= 16 * tx0 &&
                                     min(A.y, B.y) - hw <= 16 * ty1 && max(A.y, B.y) + hw >= 16 * ty0;
                    const uint32_t c = la->sel[ci].kc, fd = 256u - (uint32_t)(((long long)(row - j) * (256 - la->dim_floor)) / la->window);
                    const uint32_t color = ((c & 255u) * fd >> 8) | ((c >> 8 & 255u) * fd >> 8) << 8 | ((c >> 16 & 255u) * fd >> 8) << 16;
                    s_e[tid] = make_int4(A.x, A.y, B.x, B.y);
                    s_f[tid] = make_int4((int)color, vis, 0, 0);
                }
                __syncthreads();
                if (!live) continue;
                for (int j = 0; j < nc; ++j) {
                    const int4 g = s_f[j];
                    if (!g.y) continue;                // (uniform)
                    const int4 e = s_e[j];
                    mm_paint(px, mm_capsule_strip(e.x, e.y, e.z, e.w, hw, x0, y0), (uint32_t)g.x);
                }
            }
        }
        // ---- 4b. pass arrows: the events [first, last) that can show on this picture, in event order; the shaft, then the head ----
        if (la->ev) {                                  // (uniform)
            const int2 rg = la->ev_range[row - la->range_row0];
            for (int base = rg.x; base < rg.y; base += MM_CHUNK) {
                const int nc = min(MM_CHUNK, rg.y - base);
                __syncthreads();
                if (tid < nc) {
                    const int4* E = la->ev + 3 * (size_t)(base + tid);
                    const int4 sh = E[0], hd = E[1], k = E[2];
                    bool vis = (k.x & MM_EV_OK) && (la->only || (k.y <= row && (long long)row < (long long)k.z + la->pass_hold));
                    int lx = min(sh.x, sh.z) - hw, hx = max(sh.x, sh.z) + hw, ly = min(sh.y, sh.w) - hw, hy = max(sh.y, sh.w) + hw;
                    if (k.x & MM_EV_HEAD) {
                        lx = min(lx, min(hd.x, hd.z)); hx = max(hx, max(hd.x, hd.z)); ly = min(ly, min(hd.y, hd.w)); hy = max(hy, max(hd.y, hd.w));
                    }
                    vis = vis && lx <= 16 * tx1 && hx >= 16 * tx0 && ly <= 16 * ty1 && hy >= 16 * ty0;
                    s_e[tid] = sh; s_f[tid] = hd;
                    s_g[tid] = make_int4(k.x & (int)MM_WHITE, vis, k.x & MM_EV_HEAD, 0);
                }
                __syncthreads();
                if (!live) continue;
                for (int j = 0; j < nc; ++j) {
                    const int4 g = s_g[j];
                    if (!g.y) continue;                // (uniform)
                    const int4 e = s_e[j];
                    uint32_t bits = mm_capsule_strip(e.x, e.y, e.z, e.w, hw, x0, y0);
                    if (g.z) {
                        const int4 hd = s_f[j];
                        bits |= mm_tri_strip(e.z, e.w, hd.x, hd.y, hd.z, hd.w, x0, y0);
                    }
                    mm_paint(px, bits, (uint32_t)g.x);
                }
            }
        }
    }

    // ---- 5. + 6. discs and ball rings in list order, culled against the tile ----
    for (int base = 0; base < count; base += MM_CHUNK) {
        const int nc = min(MM_CHUNK, count - base);
        __syncthreads();
        if (tid < nc) {
            int4 e = L[MM_HEAD + base + tid];
            int rr = ((uint32_t)e.z >> MM_KIND_SHIFT & 15) == EAGLE_POST_BALL ? m.rb16 : m.r16;
            if constexpr (LAYERS) {
                if (e.z & MM_OWNER_BIT) rr = la->r16o;
            }
            // pixels with |16 X - qx| <= rr: ceil((qx - rr) / 16) .. floor((qx + rr) / 16)
            e.w = ((e.x - rr + 15) >> 4) <= tx1 && ((e.x + rr) >> 4) >= tx0 && ((e.y - rr + 15) >> 4) <= ty1 && ((e.y + rr) >> 4) >= ty0;
            if constexpr (LAYERS) {
                if (((uint32_t)e.z >> MM_KIND_SHIFT & 15) == MM_KIND_SKIP) e.w = 0;
            }
            s_e[tid] = e;
        }
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < nc; ++j) {
            const int4 e = s_e[j];
            if (!e.w) continue;                        // (uniform)
            const bool ball = ((uint32_t)e.z >> MM_KIND_SHIFT & 15) == EAGLE_POST_BALL;
            const int rr = ball ? m.rb16 : m.r16;
            const int dx0 = 16 * x0 - e.x, dy0 = 16 * y0 - e.y;
            if constexpr (LAYERS) {                    // the owner's ring after its disc; a dimmed disc; a still's ring in its column's colour
                const int ro = (e.z & MM_OWNER_BIT) ? la->r16o : rr;
                if (dx0 > ro || dx0 + 16 * (AN_STRIP - 1) < -ro || dy0 > ro || dy0 + 16 < -ro) continue;
                const int hi = rr * rr, lo = ball ? m.rbi16 * m.rbi16 : -1, ho = ro * ro;
                const uint32_t color = (uint32_t)e.z & MM_WHITE;
                #pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int dy = dy0 + 16 * r;
                    #pragma unroll
                    for (int k = 0; k < AN_STRIP; ++k) {
                        const int dx = dx0 + 16 * k, d2 = dx * dx + dy * dy;      // (|dx|, |dy| <= ro + 112 <= 2832 here: 32 bits hold it)
                        if (d2 <= hi && d2 > lo) px[r][k] = (e.z & MM_DIM_BIT) ? mm_blend(px[r][k], color, MM_DIM_A) : color;
                        else if (d2 > hi && d2 <= ho) px[r][k] = MM_WHITE;
                    }
                }
                continue;
            }
            if (dx0 > rr || dx0 + 16 * (AN_STRIP - 1) < -rr || dy0 > rr || dy0 + 16 < -rr) continue;
            const int hi = rr * rr, lo = ball ? m.rbi16 * m.rbi16 : -1;
            const uint32_t color = ball ? MM_WHITE : (uint32_t)e.z & MM_WHITE;
            #pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int dy = dy0 + 16 * r;
                #pragma unroll
                for (int k = 0; k < AN_STRIP; ++k) {
                    const int dx = dx0 + 16 * k, d2 = dx * dx + dy * dy;      // (|dx|, |dy| <= rr + 112 here: 32 bits hold it)
                    if (d2 <= hi && d2 > lo) px[r][k] = color;
                }
            }
        }
    }

    if (live) write_strip(a, f, x0, y0, cnt, rows, px);
}

__global__ __launch_bounds__(AN_THREADS) void minimap_kernel(MinimapArgs m) { mm_draw<false>(m, nullptr); }
__global__ __launch_bounds__(AN_THREADS) void minimap_layers_kernel(MinimapArgs m, MmLayerArgs la) { mm_draw<true>(m, &la); }

// rows row0 .. row0 + n - 1 -> n pictures; the lists buffer holds min(n, MM_PASS) rows and is reused pass by pass (same stream: ordered)
static constexpr int MM_PASS = 65535;                  // gridDim.y limit
static constexpr int64_t MM_STAGING = (int64_t)32 << 20;      // eagle_minimap_frames: device + pinned staging per pass (21 BGR pictures at 8 px per metre; a pass
                                                              // of that size moves for a millisecond or more, against which its two launches and one wait vanish)
// la: the K25 layers (nullptr: the plain pair of launches); still: the trajectory still, whose one list trail_marks_kernel writes
static void minimap_launch(const MinimapArgs& args, hipStream_t s, const MmLayerArgs* la = nullptr, bool still = false)
{
    MinimapArgs m = args;
    const int tiles = (m.out.w + AN_TW - 1) / AN_TW * ((m.out.h + AN_TH - 1) / AN_TH);
    for (int f0 = 0; f0 < args.n; f0 += MM_PASS) {
        m.n = std::min(args.n - f0, MM_PASS);
        m.row0 = args.row0 + f0;
        m.out.dst = args.out.dst + (int64_t)f0 * args.out.frame_stride;
        if (args.grid) m.grid = args.grid + (size_t)f0 * args.ctl_gw * args.ctl_gh;
        if (la) {
            if (still) trail_marks_launch(la->pts, la->sel, la->nsel, la->prows, m.lists, s);
            else hipLaunchKernelGGL(minimap_sites_layers_kernel, dim3((m.n + 255) / 256), dim3(256), 0, s, m, *la);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(minimap_layers_kernel, dim3(tiles, m.n), dim3(AN_THREADS), 0, s, m, *la);
            HIP_CHECK(hipGetLastError());
            continue;
        }
        hipLaunchKernelGGL(minimap_sites_kernel, dim3((m.n + 255) / 256), dim3(256), 0, s, m);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(minimap_kernel, dim3(tiles, m.n), dim3(AN_THREADS), 0, s, m);
        HIP_CHECK(hipGetLastError());
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
MmPlan minimap_plan(const EagleMinimapParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "minimap: params is NULL");
    if (p->scale < 2 || p->scale > 32 || (p->scale & 1)) fail(EAGLE_E_INVALID, "minimap: scale %d must be even and within 2 .. 32 pixels per metre", p->scale);
    if (p->margin < 0 || p->margin > 64 || (p->margin & 1)) fail(EAGLE_E_INVALID, "minimap: margin %d must be even and within 0 .. 64 pixels", p->margin);
    if (p->player_radius < 0 || p->player_radius > 4 * p->scale || p->ball_radius < 0 || p->ball_radius > 4 * p->scale)
        fail(EAGLE_E_INVALID, "minimap: radii %d / %d must lie within 0 .. 4 x scale = %d (0: the default)", p->player_radius, p->ball_radius, 4 * p->scale);
    if (p->control && p->voronoi) fail(EAGLE_E_INVALID, "minimap: control and voronoi draw in the same slot: choose one");
    if (p->layers & ~(EAGLE_MM_TRAILS | EAGLE_MM_PASSES | EAGLE_MM_OWNER | EAGLE_MM_HULLS)) fail(EAGLE_E_INVALID, "minimap: layers 0x%x has unknown bits", (unsigned)p->layers);
    MmPlan pl;
    pl.S = p->scale; pl.M = p->margin;
    pl.w = 105 * pl.S + 2 * pl.M; pl.h = 68 * pl.S + 2 * pl.M;
    pl.r = p->player_radius ? p->player_radius : std::max(2, pl.S);
    pl.rb = p->ball_radius ? p->ball_radius : std::max(3, pl.S / 2 + 1);
    pl.t = std::max(1, pl.rb / 3);
    return pl;
}

// the white pitch markings of a (scale, margin) as a bit mask, rows of (w + 7) / 8 bytes: tests/minimap_ref.py::markings, dimension by dimension
std::vector<uint8_t> markings_mask(const MmPlan& pl, int* pitch)
{
    const int S = pl.S, M = pl.M, w = pl.w, h = pl.h, hw = std::max(1, S / 4), mp = (w + 7) / 8;
    std::vector<uint8_t> bits((size_t)mp * h, 0);
    const double K = (double)(16 * S);
    auto u = [&](double d) { return (int)std::floor(d * K + 0.5); };
    auto qx = [&](double x) { return 16 * M + u(x); };
    auto qy = [&](double y) { return 16 * M + 16 * 68 * S - u(y); };
    auto P = [](int q) { return (q + 8) >> 4; };
    auto set = [&](int x, int y) { bits[(size_t)y * mp + (x >> 3)] |= (uint8_t)(1u << (x & 7)); };
    auto rect = [&](int xa, int xb, int ya, int yb) {
        const int x0 = std::max(std::min(xa, xb) - hw, 0), x1 = std::min(std::max(xa, xb) + hw, w - 1), y0 = std::max(std::min(ya, yb) - hw, 0), y1 = std::min(std::max(ya, yb) + hw, h - 1);
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) set(x, y);
    };
    auto vline = [&](double x, double ya, double yb) { rect(P(qx(x)), P(qx(x)), P(qy(ya)), P(qy(yb))); };
    auto hline = [&](double y, double xa, double xb) { rect(P(qx(xa)), P(qx(xb)), P(qy(y)), P(qy(y))); };
    const double PW = 105.0, PH = 68.0, MIDX = 52.5, MIDY = 34.0, PMX = 11.0;
    const double box[2][3] = {{16.5, 13.84, 54.16}, {5.5, 24.84, 43.16}};          // pitch.py: penalty area, goal area (depth, y0, y1)
    vline(0.0, 0.0, PH); vline(MIDX, 0.0, PH); vline(PW, 0.0, PH);
    hline(0.0, 0.0, PW); hline(PH, 0.0, PW);
    for (const auto& b : box) {
        vline(b[0], b[1], b[2]); vline(PW - b[0], b[1], b[2]);
        for (int k = 1; k <= 2; ++k) { hline(b[k], 0.0, b[0]); hline(b[k], PW - b[0], PW); }
    }
    const long long R = u(MM_CIRCLE_R), t = 16 * hw;
    // side: 0 whole ring, +1 only 16 X > lim, -1 only 16 X < lim; r_out < 0: the disc of radius -r_out
    auto round_shape = [&](double cxm, double cym, long long r_in, long long r_out, int side, int lim) {
        const long long cx = qx(cxm), cy = qy(cym);
        const int x0 = std::max((int)((cx - r_out) >> 4) - 1, 0), x1 = std::min((int)((cx + r_out) >> 4) + 1, w - 1);
        const int y0 = std::max((int)((cy - r_out) >> 4) - 1, 0), y1 = std::min((int)((cy + r_out) >> 4) + 1, h - 1);
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) {
                const long long dx = 16LL * x - cx, dy = 16LL * y - cy, d = dx * dx + dy * dy;
                if (d > r_out * r_out || (r_in >= 0 && d < r_in * r_in)) continue;
                if ((side > 0 && !(16 * x > lim)) || (side < 0 && !(16 * x < lim))) continue;
                set(x, y);
            }
    };
    round_shape(MIDX, MIDY, R - t, R + t, 0, 0);
    round_shape(PMX, MIDY, R - t, R + t, 1, qx(box[0][0]));
    round_shape(PW - PMX, MIDY, R - t, R + t, -1, qx(PW - box[0][0]));
    for (double cx : {MIDX, PMX, PW - PMX}) round_shape(cx, MIDY, -1, 2 * t, 0, 0);
    *pitch = mp;
    return bits;
}

// which table columns are drawn, in drawing order, and the four corner columns: eagle_overlay_from_table's walk on the pitch columns
static void minimap_columns(const EaglePostColumn* columns, int ncols, bool has_team, const int32_t* team_ids, const int32_t* team_vals, size_t n_team,
                            std::vector<MmCol>& out, int corner[4])
{
    const uint32_t green = 0x00ff00u, red = 0xff0000u, blue = 0x0000ffu;      // B | G << 8 | R << 16
    for (int k = 0; k < 4; ++k) corner[k] = -1;
    std::vector<MmCol> balls;
    for (int c = 0; c < ncols; ++c) {
        const EaglePostColumn& col = columns[c];
        if (col.video) continue;
        if (col.kind == EAGLE_POST_BOUNDARY) {
            if (col.id >= 0 && col.id < 4 && corner[col.id] < 0) corner[col.id] = c;
            continue;
        }
        if (col.kind == EAGLE_POST_BALL) { balls.push_back(MmCol{c, MM_WHITE | (uint32_t)EAGLE_POST_BALL << MM_KIND_SHIFT}); continue; }
        if (col.kind != EAGLE_POST_PLAYER && col.kind != EAGLE_POST_GOALKEEPER) fail(EAGLE_E_INVALID, "minimap: column %d has unknown kind %d", c, col.kind);
        uint32_t color = green, site = 0;
        if (col.kind == EAGLE_POST_PLAYER) {
            site = MM_SITE_BIT;
            if (!has_team) color = MM_WHITE;
            else {
                size_t k = 0;
                while (k < n_team && team_ids[k] != col.id) ++k;
                if (k == n_team) continue;
                color = team_vals[k] == 0 ? red : blue;
            }
        }
        out.push_back(MmCol{c, color | (uint32_t)col.kind << MM_KIND_SHIFT | site});
    }
    out.insert(out.end(), balls.begin(), balls.end());
}

static void minimap_window(int rows, int row0, int n)
{
    if (n < 0) fail(EAGLE_E_INVALID, "minimap: n = %d is negative", n);
    if (n > 0 && rows == 0) fail(EAGLE_E_INVALID, "minimap: the table has no rows");
    if (row0 < 0 || row0 > rows || n > rows - row0) fail(EAGLE_E_INVALID, "minimap: rows %d .. %d lie outside the table's %d rows", row0, row0 + n - 1, rows);
}

// everything of a call's kernel arguments that does not depend on the output buffer
static MinimapArgs minimap_args(const MmPlan& pl, const EagleMinimapParams* p)
{
    MinimapArgs m{};
    m.scale = pl.S; m.margin = pl.M; m.voronoi = p->voronoi != 0; m.footprint = p->footprint != 0;
    m.r16 = 16 * pl.r; m.rb16 = 16 * pl.rb; m.rbi16 = 16 * (pl.rb - pl.t);
    m.mask_pitch = (pl.w + 7) / 8;
    return m;
}

static void grow(void** buf, size_t* cap, size_t need)
{
    if (need <= *cap) return;
    if (*buf) HIP_CHECK(hipFree(*buf));
    *buf = nullptr; *cap = 0;
    HIP_CHECK(hipMalloc(buf, need));
    *cap = need;
}

// the marking mask of this (scale, margin) in the handle, rebuilt when either changed (also the occupancy picture's)
const uint8_t* minimap_mask(EagleHandle* h, const MmPlan& pl)
{
    if (h->mm_mask_scale != pl.S || h->mm_mask_margin != pl.M) {
        int mp = 0;
        const std::vector<uint8_t> bits = markings_mask(pl, &mp);
        grow((void**)&h->mm_mask, &h->mm_mask_cap, bits.size());
        h->mm_mask_scale = 0;
        HIP_CHECK(hipMemcpyAsync(h->mm_mask, bits.data(), bits.size(), hipMemcpyHostToDevice, h->s_main));
        HIP_CHECK(hipStreamSynchronize(h->s_main));        // (a pageable source: it has left the vector before the vector goes)
        h->mm_mask_scale = pl.S; h->mm_mask_margin = pl.M;
    }
    return h->mm_mask;
}

// bytes a call writes (the pictures) and reads (the pitch cells of its rows)
static double minimap_bytes(const MinimapArgs& m, const YuvGeom& g) { return (double)m.n * ((double)g.dense_bytes + 16.0 * (m.ncols + 4)); }

// Once per call of a handle entry: which columns are drawn (uploaded), the corner columns, the marking mask of this (scale, margin), and list space for
// passes of up to max_pass rows.  The result lacks only the rows and the output of a pass (minimap_pass)
static MinimapArgs minimap_prepare(EagleHandle* h, EaglePostTable* t, const MmPlan& pl, const EagleMinimapParams* p, int max_pass)
{
    std::vector<MmCol> cols;
    MinimapArgs m = minimap_args(pl, p);
    minimap_columns(t->columns.data(), t->cols, t->has_team, t->team_ids.data(), t->team_vals.data(), t->team_ids.size(), cols, m.corner);
    m.values = (const double2*)t->d_values; m.rows = t->rows; m.ncols = (int)cols.size(); m.stride = MM_HEAD + m.ncols;
    grow(&h->mm_list, &h->mm_list_cap, (size_t)std::min(max_pass, MM_PASS) * m.stride * sizeof(int4));
    grow(&h->mm_cols, &h->mm_cols_cap, std::max<size_t>(cols.size() * sizeof(MmCol), 16));
    minimap_mask(h, pl);
    if (!cols.empty()) HIP_CHECK(hipMemcpyAsync(h->mm_cols, cols.data(), cols.size() * sizeof(MmCol), hipMemcpyHostToDevice, h->s_main));
    HIP_CHECK(hipStreamSynchronize(h->s_main));            // (pageable sources: they have left the vectors)
    m.lists = (int4*)h->mm_list; m.cols = (const MmCol*)h->mm_cols; m.mask = h->mm_mask;
    return m;
}

// rows row0 .. row0 + n - 1 -> n pictures at d_out (layout g) on s_main; returns when they are complete
static void minimap_pass(EagleHandle* h, const MinimapArgs& prepared, int row0, int n, const YuvGeom& g, uint8_t* d_out, const ControlArgs* ctl = nullptr,
                         const MmLayerArgs* la = nullptr, bool still = false)
{
    MinimapArgs m = prepared;
    m.out = annot_args(g, nullptr, d_out, nullptr, nullptr);
    m.row0 = row0; m.n = n;
    if (ctl) control_rows(h, *ctl, row0, n, (uint8_t*)h->ct_grid, nullptr);      // the grids of these rows, on the same stream in front of the draw
    timed_launch(h, la ? "minimap_layers" : "minimap", minimap_bytes(m, g), h->s_main, [&] { minimap_launch(m, h->s_main, la, still); });
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    if (h->prof) collect_spans(h);
}

static MmPlan minimap_begin(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleMinimapParams* p, const void* out)
{
    if (!t || !out) fail(EAGLE_E_INVALID, "minimap: bad argument (table %p, out %p)", (const void*)t, out);
    if (t->h != h) fail(EAGLE_E_INVALID, "minimap: the table belongs to another handle");
    const MmPlan pl = minimap_plan(p);
    if (p->voronoi && !t->has_team) fail(EAGLE_E_INVALID, "minimap: voronoi needs a table with a team mapping (the areas are coloured by team)");
    if (p->control) {
        if (!t->has_team) fail(EAGLE_E_INVALID, "minimap: control needs a table with a team mapping (team 0 is counted against the others)");
        if (!t->d_vel) fail(EAGLE_E_INVALID, "minimap: control needs the table's velocities (eagle_post_velocities comes first)");
        if (!t->has_control) fail(EAGLE_E_INVALID, "minimap: control needs its parameters (eagle_minimap_set_control comes first)");
    }
    if (p->layers & EAGLE_MM_HULLS) {
        if (!t->has_shape) fail(EAGLE_E_INVALID, "minimap: the hull layer needs a team-shape result (eagle_post_team_shape comes first)");
        if (!t->has_hulls) fail(EAGLE_E_INVALID, "minimap: the hull layer needs its parameters (eagle_minimap_set_hulls comes first)");
    }
    if (p->layers & (EAGLE_MM_TRAILS | EAGLE_MM_PASSES | EAGLE_MM_OWNER)) {
        if (!t->has_trails) fail(EAGLE_E_INVALID, "minimap: layers need their parameters (eagle_minimap_set_trails comes first)");
        if ((p->layers & (EAGLE_MM_PASSES | EAGLE_MM_OWNER)) && !t->has_poss)
            fail(EAGLE_E_INVALID, "minimap: the pass and owner layers need a possession result (eagle_post_possession comes first)");
        if ((p->layers & EAGLE_MM_TRAILS) && t->trail_cols.empty()) fail(EAGLE_E_INVALID, "minimap: the trail layer needs a selection (eagle_minimap_set_trails was given none)");
    }
    minimap_window(t->rows, row0, n);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    return pl;
}

// ---- the K25 layers: host side ---------------------------------------------------------------------------------------------------------
void trail_check(const char* who, const EagleTrailParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the trail parameters are NULL", who);
    if (p->window < 1) fail(EAGLE_E_INVALID, "%s: window %d must be at least 1 row", who, p->window);
    if (p->max_gap < 1) fail(EAGLE_E_INVALID, "%s: max_gap %d must be at least 1 frame", who, p->max_gap);
    if (p->half_width < 1 || p->half_width > 8) fail(EAGLE_E_INVALID, "%s: half_width %d must lie within 1 .. 8 pixels", who, p->half_width);
    if (p->pass_hold < 1) fail(EAGLE_E_INVALID, "%s: pass_hold %d must be at least 1 row", who, p->pass_hold);
    if (p->dim_floor < 0 || p->dim_floor > 256) fail(EAGLE_E_INVALID, "%s: dim_floor %d must lie within 0 .. 256", who, p->dim_floor);
}

void trail_selection_check(const char* who, const EaglePostColumn* columns, int ncols, const int32_t* sel, int nsel)
{
    if (nsel < 0 || (nsel > 0 && !sel)) fail(EAGLE_E_INVALID, "%s: bad selection (%p, %d members)", who, (const void*)sel, nsel);
    if (nsel > 65535) fail(EAGLE_E_INVALID, "%s: a selection of %d columns is beyond 65535", who, nsel);
    std::vector<uint8_t> seen((size_t)std::max(ncols, 1), 0);
    for (int k = 0; k < nsel; ++k) {
        const int c = sel[k];
        if (c < 0 || c >= ncols) fail(EAGLE_E_INVALID, "%s: selection member %d (column %d) lies outside the table's %d columns", who, k, c, ncols);
        if (columns[c].video || (columns[c].kind != EAGLE_POST_PLAYER && columns[c].kind != EAGLE_POST_GOALKEEPER && columns[c].kind != EAGLE_POST_BALL))
            fail(EAGLE_E_INVALID, "%s: selection member %d (column %d) is not a Player, Goalkeeper or Ball pitch column", who, k, c);
        if (seen[c]) fail(EAGLE_E_INVALID, "%s: column %d is selected twice", who, c);
        seen[c] = 1;
    }
}

// the selected columns that have a colour (their disc's), in selection order
static std::vector<MmCol> trail_selection(const EaglePostColumn* columns, int ncols, bool has_team, const int32_t* team_ids, const int32_t* team_vals, size_t n_team,
                                          const int32_t* sel, int nsel)
{
    std::vector<MmCol> drawn, out;
    int corner[4];
    minimap_columns(columns, ncols, has_team, team_ids, team_vals, n_team, drawn, corner);
    for (int k = 0; k < nsel; ++k)
        for (const MmCol& d : drawn)
            if (d.col == sel[k]) { out.push_back(d); break; }
    return out;
}

// device memory of the layers of one call.  With a handle the buffers are the handle's (mm_tr, grown on demand like the draw lists: no allocation and
// no device-wide synchronisation per call); an operator entry owns them for the call and frees them when it ends (after the device has been synchronised)
enum { TR_SEL, TR_FRAMES, TR_PTS, TR_LINK, TR_EVSRC, TR_EV, TR_RANGE, TR_OUT, TR_HULL };
struct DevTmp {
    EagleHandle* h = nullptr;
    int slot = 0;                                          // the next slot of h->mm_tr (layers_setup asks in a fixed order)
    std::vector<void*> own;
    explicit DevTmp(EagleHandle* hh = nullptr) : h(hh) {}
    ~DevTmp() { for (void* q : own) (void)hipFree(q); }
    void* get(size_t b, int k)
    {
        if (h) { grow(&h->mm_tr[k], &h->mm_tr_cap[k], std::max<size_t>(b, 16)); return h->mm_tr[k]; }
        void* q = nullptr; HIP_CHECK(hipMalloc(&q, std::max<size_t>(b, 16))); own.push_back(q); return q;
    }
    void* upload(const void* src, size_t b, hipStream_t s, int k)
    {
        void* q = get(b, k);
        if (b) HIP_CHECK(hipMemcpyAsync(q, src, b, hipMemcpyHostToDevice, s));
        return q;
    }
};

struct LayerJob {
    int layers = 0;
    EagleTrailParams tp{};
    std::vector<MmCol> sel;              // (trails or the trajectory still)
    const int32_t* d_owner = nullptr;    // [rows] in HBM
    const EaglePossessionEvent* events = nullptr;
    int nev = 0;
    int only_event = -1;                 // >= 0: the pass still
    bool trajectory = false;             // the trajectory still of rows row0 .. row0 + n - 1
    const EagleTeamShape* d_shapes = nullptr;      // K26 hulls: the shape result in HBM ([rows][2]; [rows][2][32]) and the layer's half width
    const int32_t* d_hull = nullptr;
    int hull_hw = 0;
};

// everything the layered launches of rows row0 .. row0 + n - 1 read, prepared on stream s (which is synchronised before the host vectors go)
static MmLayerArgs layers_setup(DevTmp& tmp, hipStream_t s, const double2* d_values, int rows, const int32_t* frames, const MmPlan& pl, const LayerJob& job, int row0, int n)
{
    MmLayerArgs la{};
    const EagleTrailParams& tp = job.tp;
    la.window = tp.window; la.dim_floor = tp.dim_floor; la.hw16 = 16 * tp.half_width; la.pass_hold = tp.pass_hold;
    la.jlo = -1; la.range_row0 = row0; la.pass_from = la.pass_to = -1;
    la.r16o = 16 * (pl.r + std::max(1, pl.r / 3));
    std::vector<int2> range;
    if (((job.layers & EAGLE_MM_TRAILS) || job.trajectory) && !job.sel.empty()) {
        la.nsel = (int)job.sel.size();
        la.prow0 = job.trajectory || tp.window > row0 ? (job.trajectory ? row0 : 0) : row0 - tp.window;
        la.prows = row0 + n - la.prow0;
        if ((int64_t)la.nsel * la.prows > 0x7fffffff) fail(EAGLE_E_INVALID, "minimap: %d selected columns x %d rows of trail is beyond 2^31 segments", la.nsel, la.prows);
        if (job.trajectory) { la.jlo = row0 + 1; la.dim_floor = 256; la.window = std::max(1, n - 1); }
        la.sel = (const MmCol*)tmp.upload(job.sel.data(), job.sel.size() * sizeof(MmCol), s, TR_SEL);
        const int32_t* d_frames = (const int32_t*)tmp.upload(frames + la.prow0, (size_t)la.prows * 4, s, TR_FRAMES);
        int2* pts = (int2*)tmp.get((size_t)la.nsel * la.prows * sizeof(int2), TR_PTS);
        uint8_t* link = (uint8_t*)tmp.get((size_t)la.prows, TR_LINK);
        trail_points_launch(d_values, rows, la.sel, la.nsel, d_frames, la.prow0, la.prows, tp.max_gap, pl.S, pl.M, pts, link, s);
        la.pts = pts; la.link = link;
    }
    if (((job.layers & EAGLE_MM_PASSES) || job.only_event >= 0) && job.nev > 0) {
        const EaglePossessionEvent* d_ev = (const EaglePossessionEvent*)tmp.upload(job.events, (size_t)job.nev * sizeof(EaglePossessionEvent), s, TR_EVSRC);
        int4* out = (int4*)tmp.get((size_t)job.nev * 3 * sizeof(int4), TR_EV);
        trail_events_launch(d_ev, job.nev, pl.S, pl.M, tp.half_width, out, s);
        la.ev = out;
        range.resize((size_t)n);
        if (job.only_event >= 0) {
            la.only = 1;
            range[0] = make_int2(job.only_event, job.only_event + 1);
        } else {
            // release_row and receive_row ascend with the events: those with release_row <= r are a prefix, those with r < receive_row + hold a suffix
            int lo = 0, hi = 0;
            for (int i = 0; i < n; ++i) {
                const int r = row0 + i;
                while (hi < job.nev && job.events[hi].release_row <= r) ++hi;
                while (lo < job.nev && (int64_t)job.events[lo].receive_row + tp.pass_hold <= r) ++lo;
                range[i] = make_int2(std::min(lo, hi), hi);
            }
        }
        la.ev_range = (const int2*)tmp.upload(range.data(), range.size() * sizeof(int2), s, TR_RANGE);
    }
    if (job.only_event >= 0 && job.nev > 0) {
        la.dim = 1; la.pass_from = job.events[job.only_event].from_col; la.pass_to = job.events[job.only_event].to_col;
    }
    if (job.layers & EAGLE_MM_OWNER) la.owner = job.d_owner;
    if ((job.layers & EAGLE_MM_HULLS) && job.d_shapes && n > 0) {
        int4* edges = (int4*)tmp.get((size_t)n * 2 * EAGLE_SHAPE_HULL_CAP * sizeof(int4), TR_HULL);
        shape_edges_launch(d_values, rows, job.d_shapes, job.d_hull, row0, n, pl.S, pl.M, edges, s);
        la.hull_edges = edges; la.hull_hw16 = 16 * job.hull_hw;
    }
    HIP_CHECK(hipStreamSynchronize(s));                    // (pageable sources: they have left the vectors)
    return la;
}

static LayerJob table_job(EaglePostTable* t, int layers)
{
    LayerJob job;
    job.layers = layers; job.tp = t->trails;
    if (layers & EAGLE_MM_TRAILS)
        job.sel = trail_selection(t->columns.data(), t->cols, t->has_team, t->team_ids.data(), t->team_vals.data(), t->team_ids.size(), t->trail_cols.data(), (int)t->trail_cols.size());
    if (t->has_poss) {
        job.d_owner = t->rows ? (const int32_t*)((const double*)t->d_poss + t->rows) + t->rows : nullptr;
        job.events = t->events.data(); job.nev = (int)t->events.size();
    }
    if (!job.d_owner) job.layers &= ~EAGLE_MM_OWNER;
    if ((layers & EAGLE_MM_HULLS) && t->has_shape && t->rows) {
        job.d_shapes = (const EagleTeamShape*)t->d_shape; job.d_hull = (const int32_t*)(job.d_shapes + (size_t)t->rows * 2);
        job.hull_hw = t->hulls.half_width;
    }
    return job;
}

static void events_check(const char* who, const EaglePossessionEvent* ev, int nev, int rows)
{
    if (nev < 0 || (nev > 0 && !ev)) fail(EAGLE_E_INVALID, "%s: bad events (%p, %d)", who, (const void*)ev, nev);
    for (int k = 0; k < nev; ++k) {
        if (ev[k].release_row < 0 || ev[k].release_row >= rows || ev[k].receive_row < 0 || ev[k].receive_row >= rows || ev[k].kind < 0 || ev[k].kind > EAGLE_EVENT_UNKNOWN)
            fail(EAGLE_E_INVALID, "%s: event %d has rows %d, %d outside the table's %d rows or kind %d", who, k, ev[k].release_row, ev[k].receive_row, rows, ev[k].kind);
        if (k && (ev[k].release_row < ev[k - 1].release_row || ev[k].receive_row < ev[k - 1].receive_row))
            fail(EAGLE_E_INVALID, "%s: the rows of event %d do not ascend", who, k);
    }
}

// a still of a handle's table: one picture of row `row0` (pass) or of the window (trajectory) -> host memory, BGR
static void handle_still(EagleHandle* h, EaglePostTable* t, const MmPlan& pl, const EagleMinimapParams* p, const LayerJob& job, int row0, int n, uint8_t* out)
{
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const YuvGeom g = yuv_geometry(EAGLE_PIX_BGR, pl.h, pl.w, nullptr, true);
    DevTmp tmp(h);
    try {
        MinimapArgs m = minimap_prepare(h, t, pl, p, 1);
        if (job.trajectory) {                              // its list has two entries per selected column, written by trail_marks_kernel
            m.ncols = 2 * (int)job.sel.size(); m.stride = MM_HEAD + m.ncols;
            grow(&h->mm_list, &h->mm_list_cap, (size_t)m.stride * sizeof(int4));
            m.lists = (int4*)h->mm_list;
        }
        const MmLayerArgs la = layers_setup(tmp, h->s_main, (const double2*)t->d_values, t->rows, t->frames.data(), pl, job, row0, n);
        uint8_t* d_out = (uint8_t*)tmp.get((size_t)g.dense_bytes, TR_OUT);
        minimap_pass(h, m, job.trajectory ? row0 + n - 1 : row0, 1, g, d_out, nullptr, &la, job.trajectory);
        HIP_CHECK(hipMemcpy(out, d_out, (size_t)g.dense_bytes, hipMemcpyDeviceToHost));
    } catch (...) {
        (void)hipStreamSynchronize(h->s_main);
        throw;
    }
}

// the control layer of a handle call: grid space for passes of up to max_pass rows in the handle, the prepared site columns; m learns where the grids are
static ControlArgs minimap_control(EagleHandle* h, EaglePostTable* t, MinimapArgs& m, int max_pass)
{
    const ControlArgs c = control_prepare(h, t, &t->control, max_pass);
    grow(&h->ct_grid, &h->ct_grid_cap, (size_t)max_pass * c.gw * c.gh);
    m.grid = (const uint8_t*)h->ct_grid; m.ctl_R = c.R; m.ctl_gw = c.gw; m.ctl_gh = c.gh;
    return c;
}

}  // namespace eagle

extern "C" {

int eagle_minimap_size(const EagleMinimapParams* p, int* w, int* h)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!w || !h) fail(EAGLE_E_INVALID, "eagle_minimap_size: w or h is NULL");
    const MmPlan pl = minimap_plan(p);
    *w = pl.w; *h = pl.h;
    API_END(hh)
}

int eagle_minimap_device_frames(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleMinimapParams* p, int out_format, const EagleYuvLayout* out_layout, void* d_out)
{
    API_BEGIN_H(h)
    const MmPlan pl = minimap_begin(h, t, row0, n, p, d_out);
    const YuvGeom g = yuv_geometry(out_format, pl.h, pl.w, out_layout, true);
    if (n == 0) return EAGLE_OK;
    DevTmp tmp(h);
    MmLayerArgs la{};
    const MmLayerArgs* lap = nullptr;
    if (p->layers) {
        la = layers_setup(tmp, h->s_main, (const double2*)t->d_values, t->rows, t->frames.data(), pl, table_job(t, p->layers), row0, n);
        lap = &la;
    }
    if (!p->control) {
        minimap_pass(h, minimap_prepare(h, t, pl, p, n), row0, n, g, (uint8_t*)d_out, nullptr, lap);
        return EAGLE_OK;
    }
    // with the control layer the rows go in passes of what MM_STAGING bytes of grids hold (grids, then their draw), so the handle keeps one pass of grids
    const int64_t cells = (int64_t)7140 * t->control.cells_per_metre * t->control.cells_per_metre;
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(n, MM_STAGING / cells));
    MinimapArgs m = minimap_prepare(h, t, pl, p, batch);
    const ControlArgs ctl = minimap_control(h, t, m, batch);
    for (int i = 0; i < n; i += batch)
        minimap_pass(h, m, row0 + i, std::min(batch, n - i), g, (uint8_t*)d_out + (int64_t)i * g.frame_stride, &ctl, lap);
    API_END(h)
}

int eagle_minimap_frames(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleMinimapParams* p, int out_format, const EagleYuvLayout* out_layout, uint8_t* out)
{
    API_BEGIN_H(h)
    const MmPlan pl = minimap_begin(h, t, row0, n, p, out);
    const YuvGeom g = yuv_geometry(out_format, pl.h, pl.w, out_layout, true);
    if (n == 0) return EAGLE_OK;
    // pictures per pass: what MM_STAGING bytes of staging hold (the handle's batch is about 720p frames through two networks, not about these pictures)
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(n, MM_STAGING / g.dense_bytes));
    MinimapArgs m = minimap_prepare(h, t, pl, p, batch);
    ControlArgs ctl{};
    if (p->control) ctl = minimap_control(h, t, m, batch);
    DevTmp tmp(h);
    MmLayerArgs la{};
    const MmLayerArgs* lap = nullptr;
    if (p->layers) {
        la = layers_setup(tmp, h->s_main, (const double2*)t->d_values, t->rows, t->frames.data(), pl, table_job(t, p->layers), row0, n);
        lap = &la;
    }
    frames_to_host(h, n, pl.h, pl.w, batch, out_format, out_layout, out,
                   [&](int i, int na, const YuvGeom& dg, uint8_t* d_dst) { minimap_pass(h, m, row0 + i, na, dg, d_dst, p->control ? &ctl : nullptr, lap); });
    API_END(h)
}

struct OpLayers {                                          // what eagle_op_minimap_trails and the still entries add to op_minimap
    const int32_t* frames = nullptr;
    const int32_t* owner = nullptr;                        // host, [rows]
    const int32_t* sel = nullptr;
    int nsel = 0;
    LayerJob job;
    bool on = false;
    const EagleHullParams* hp = nullptr;                   // eagle_op_minimap_hulls: the entry computes the shape itself
    bool hulls = false;
};

static void op_minimap(const char* who, int device, const double* values, const double* velocities, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                       const int32_t* team_vals, int n_team, const EagleMinimapParams* p, const EagleControlParams* cp, int row0, int n, int out_format,
                       const EagleYuvLayout* out_layout, uint8_t* out, OpLayers* ol = nullptr)
{
    if (!values || !columns || !out || rows < 0 || cols < 0 || n_team < 0 || (team_ids && n_team > 0 && !team_vals))
        fail(EAGLE_E_INVALID, "%s: bad argument (values %p, columns %p, out %p, %d rows, %d columns, %d teams)", who, (const void*)values, (const void*)columns,
             (const void*)out, rows, cols, n_team);
    const MmPlan pl = minimap_plan(p);
    if (p->voronoi && !team_ids) fail(EAGLE_E_INVALID, "minimap: voronoi needs a table with a team mapping (the areas are coloured by team)");
    if (p->control) {
        if (!team_ids) fail(EAGLE_E_INVALID, "minimap: control needs a table with a team mapping (team 0 is counted against the others)");
        if (!velocities) fail(EAGLE_E_INVALID, "minimap: control needs velocities (eagle_op_minimap_control takes them)");
        control_check(cp);
    }
    if (p->layers && !(ol && ol->on)) fail(EAGLE_E_INVALID, "%s: layers need their parameters (eagle_op_minimap_trails takes them)", who);
    minimap_window(rows, row0, n);
    const bool trajectory = ol && ol->job.trajectory;
    if (trajectory && n < 1) fail(EAGLE_E_INVALID, "%s: a window of %d rows", who, n);
    const int pics = trajectory ? 1 : n;
    const YuvGeom g = yuv_geometry(out_format, pl.h, pl.w, out_layout, true);
    std::vector<MmCol> dc;
    MinimapArgs m = minimap_args(pl, p);
    minimap_columns(columns, cols, team_ids != nullptr, team_ids, team_vals, (size_t)n_team, dc, m.corner);
    m.ncols = (int)dc.size();
    if (ol && ol->on) {
        LayerJob& job = ol->job;
        if ((job.layers & EAGLE_MM_TRAILS) || trajectory) {
            if (!ol->frames) fail(EAGLE_E_INVALID, "%s: trails need the frame numbers", who);
            for (int r = 1; r < rows; ++r)
                if (ol->frames[r] <= ol->frames[r - 1]) fail(EAGLE_E_INVALID, "%s: frame numbers must ascend (row %d: %d after %d)", who, r, ol->frames[r], ol->frames[r - 1]);
            trail_selection_check(who, columns, cols, ol->sel, ol->nsel);
            if ((job.layers & EAGLE_MM_TRAILS) && ol->nsel == 0) fail(EAGLE_E_INVALID, "%s: the trail layer needs a selection", who);
            job.sel = trail_selection(columns, cols, team_ids != nullptr, team_ids, team_vals, (size_t)n_team, ol->sel, ol->nsel);
        }
        if ((job.layers & EAGLE_MM_OWNER) && !ol->owner) fail(EAGLE_E_INVALID, "%s: the owner layer needs owner[rows] (a possession result)", who);
        if ((job.layers & EAGLE_MM_PASSES) && !job.events) fail(EAGLE_E_INVALID, "%s: the pass layer needs events (a possession result)", who);
        if ((job.layers & EAGLE_MM_PASSES) || job.only_event >= 0) events_check(who, job.events, job.nev, rows);
        if (trajectory) { m.ncols = 2 * (int)job.sel.size(); }
    }
    ShapeCols shc;
    if (ol && ol->hulls) {
        hull_check(who, ol->hp);
        shc = shape_columns(who, columns, cols, team_ids, team_vals, (size_t)n_team);
    }
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const size_t span = (size_t)((pics - 1) * g.frame_stride + g.extent);
    int mp = 0;
    const std::vector<uint8_t> bits = markings_mask(pl, &mp);
    uint8_t* d_out = (uint8_t*)net.upload(out, span);                        // bytes the layout does not cover come back as they were
    m.out = annot_args(g, nullptr, d_out, nullptr, nullptr);                 // (alignment is judged on the pointer that is written)
    m.values = (const double2*)net.upload(values, (size_t)cols * rows * 2 * sizeof(double));
    dc.resize(std::max<size_t>(dc.size(), 2), MmCol{0, 0});                  // (a table without a drawable column still uploads 16 bytes; ncols says how many count)
    m.cols = (const MmCol*)net.upload(dc.data(), dc.size() * sizeof(MmCol));
    m.mask = (const uint8_t*)net.upload(bits.data(), bits.size());
    m.rows = rows; m.row0 = trajectory ? row0 + n - 1 : row0; m.n = pics; m.stride = MM_HEAD + m.ncols;
    m.lists = (int4*)net.get((size_t)std::min(pics, MM_PASS) * m.stride * sizeof(int4));
    if (p->control) {                                                        // the grids of the window, in front of the draw on the same (null) stream
        std::vector<CtCol> sc;
        control_columns(columns, cols, team_ids, team_vals, (size_t)n_team, sc);
        ControlArgs c{};
        c.R = cp->cells_per_metre; c.gw = 105 * c.R; c.gh = 68 * c.R; c.t_react = cp->t_react; c.v_max = cp->v_max; c.beta = cp->beta;
        c.ncols = (int)sc.size(); c.stride = 1 + c.ncols; c.rows = rows; c.values = m.values;
        c.vel = (const double2*)net.upload(velocities, (size_t)cols * rows * 2 * sizeof(double));
        sc.resize(std::max<size_t>(sc.size(), 2), CtCol{0, 0});
        c.cols = (const CtCol*)net.upload(sc.data(), sc.size() * sizeof(CtCol));
        c.lists = (float4*)net.get((size_t)std::min(n, CT_PASS) * c.stride * sizeof(float4));
        const size_t cells = (size_t)c.gw * c.gh;
        uint8_t* d_g = (uint8_t*)net.get((size_t)n * cells);
        for (int f0 = 0; f0 < n; f0 += CT_PASS) {
            ControlArgs b = c;
            b.n = std::min(n - f0, CT_PASS); b.row0 = row0 + f0; b.out = d_g + (size_t)f0 * cells;
            control_launch(b, nullptr);
        }
        m.grid = d_g; m.ctl_R = c.R; m.ctl_gw = c.gw; m.ctl_gh = c.gh;
    }
    if (ol && ol->on) {
        HIP_CHECK(hipDeviceSynchronize());                 // (Net::get clears its buffers on the null stream)
        DevTmp tmp;
        if (ol->job.layers & EAGLE_MM_OWNER) ol->job.d_owner = (const int32_t*)tmp.upload(ol->owner, (size_t)rows * 4, nullptr, TR_OUT);
        if (ol->hulls) {                                   // the shape of the whole table, as eagle_op_team_shape computes it
            EagleTeamShape* d_s = (EagleTeamShape*)tmp.get((size_t)rows * 2 * (sizeof(EagleTeamShape) + 4 * EAGLE_SHAPE_HULL_CAP), TR_HULL + 1);
            shape_run(nullptr, shc, m.values, rows, d_s, (int32_t*)(d_s + (size_t)rows * 2), nullptr);
            ol->job.d_shapes = d_s; ol->job.d_hull = (const int32_t*)(d_s + (size_t)rows * 2); ol->job.hull_hw = ol->hp->half_width;
        }
        const MmLayerArgs la = layers_setup(tmp, nullptr, m.values, rows, ol->frames, pl, ol->job, row0, n);
        minimap_launch(m, nullptr, &la, trajectory);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, d_out, span, hipMemcpyDeviceToHost));
        return;
    }
    minimap_launch(m, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, d_out, span, hipMemcpyDeviceToHost));
}

int eagle_op_minimap(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals, int n_team,
                     const EagleMinimapParams* p, int row0, int n, int out_format, const EagleYuvLayout* out_layout, uint8_t* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    op_minimap("eagle_op_minimap", device, values, nullptr, columns, rows, cols, team_ids, team_vals, n_team, p, nullptr, row0, n, out_format, out_layout, out);
    API_END(hh)
}

int eagle_op_minimap_control(int device, const double* values, const double* velocities, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                             const int32_t* team_vals, int n_team, const EagleMinimapParams* p, const EagleControlParams* cp, int row0, int n, int out_format,
                             const EagleYuvLayout* out_layout, uint8_t* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    op_minimap("eagle_op_minimap_control", device, values, velocities, columns, rows, cols, team_ids, team_vals, n_team, p, cp, row0, n, out_format, out_layout, out);
    API_END(hh)
}

int eagle_minimap_set_trails(EaglePostTable* t, const EagleTrailParams* p, const int32_t* cols, int ncols)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (p) {
        trail_check("eagle_minimap_set_trails", p);
        trail_selection_check("eagle_minimap_set_trails", t->columns.data(), t->cols, cols, ncols);
        t->trails = *p;
        t->trail_cols.assign(cols, cols + ncols);
    } else t->trail_cols.clear();
    t->has_trails = p != nullptr;
    API_END(h)
}

int eagle_trajectory_picture(EagleHandle* h, EaglePostTable* t, const int32_t* cols, int ncols, int row0, int n, int scale, int margin, int half_width, int max_gap,
                             uint8_t* out)
{
    API_BEGIN_H(h)
    if (!t || !out) fail(EAGLE_E_INVALID, "eagle_trajectory_picture: bad argument (table %p, out %p)", (const void*)t, (const void*)out);
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_trajectory_picture: the table belongs to another handle");
    EagleMinimapParams p{};
    p.scale = scale; p.margin = margin;
    const MmPlan pl = minimap_plan(&p);
    LayerJob job;
    job.tp.window = 1; job.tp.max_gap = max_gap; job.tp.half_width = half_width; job.tp.pass_hold = 1; job.tp.dim_floor = 256;
    trail_check("eagle_trajectory_picture", &job.tp);
    trail_selection_check("eagle_trajectory_picture", t->columns.data(), t->cols, cols, ncols);
    minimap_window(t->rows, row0, n);
    if (n < 1) fail(EAGLE_E_INVALID, "eagle_trajectory_picture: a window of %d rows", n);
    job.trajectory = true;
    job.sel = trail_selection(t->columns.data(), t->cols, t->has_team, t->team_ids.data(), t->team_vals.data(), t->team_ids.size(), cols, ncols);
    handle_still(h, t, pl, &p, job, row0, n, out);
    API_END(h)
}

int eagle_pass_picture(EagleHandle* h, EaglePostTable* t, int event, int scale, int margin, int half_width, uint8_t* out)
{
    API_BEGIN_H(h)
    if (!t || !out) fail(EAGLE_E_INVALID, "eagle_pass_picture: bad argument (table %p, out %p)", (const void*)t, (const void*)out);
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_pass_picture: the table belongs to another handle");
    EagleMinimapParams p{};
    p.scale = scale; p.margin = margin;
    const MmPlan pl = minimap_plan(&p);
    LayerJob job;
    job.tp.window = 1; job.tp.max_gap = 1; job.tp.half_width = half_width; job.tp.pass_hold = 1; job.tp.dim_floor = 256;
    trail_check("eagle_pass_picture", &job.tp);
    if (!t->has_poss) fail(EAGLE_E_INVALID, "eagle_pass_picture: the table has no possession result (eagle_post_possession comes first)");
    if (event < 0 || event >= (int)t->events.size()) fail(EAGLE_E_INVALID, "eagle_pass_picture: event %d lies outside the table's %d events", event, (int)t->events.size());
    job.events = t->events.data(); job.nev = (int)t->events.size(); job.only_event = event;
    handle_still(h, t, pl, &p, job, t->events[event].release_row, 1, out);
    API_END(h)
}

int eagle_op_minimap_trails(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                            const int32_t* team_vals, int n_team, const EagleMinimapParams* p, const EagleTrailParams* tp, const int32_t* sel, int nsel,
                            const int32_t* owner, const EaglePossessionEvent* events, int n_events, int row0, int n, int out_format, const EagleYuvLayout* out_layout,
                            uint8_t* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_minimap_trails";
    if (!p) fail(EAGLE_E_INVALID, "minimap: params is NULL");
    if (p->control) fail(EAGLE_E_INVALID, "%s: the control layer is not available here (it needs velocities)", who);
    if (p->layers & EAGLE_MM_HULLS) fail(EAGLE_E_INVALID, "%s: the hull layer needs a team-shape result, which this entry cannot carry (eagle_op_minimap_hulls computes one)", who);
    OpLayers ol;
    if (p->layers) {
        if (!tp) fail(EAGLE_E_INVALID, "%s: a layer without trail parameters", who);
        trail_check(who, tp);
        ol.on = true; ol.frames = frames; ol.owner = owner; ol.sel = sel; ol.nsel = nsel;
        ol.job.layers = p->layers; ol.job.tp = *tp; ol.job.events = events; ol.job.nev = n_events;
    }
    op_minimap(who, device, values, nullptr, columns, rows, cols, team_ids, team_vals, n_team, p, nullptr, row0, n, out_format, out_layout, out, &ol);
    API_END(hh)
}

int eagle_op_minimap_hulls(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                           const int32_t* team_vals, int n_team, const EagleMinimapParams* p, const EagleHullParams* hp, const EagleTrailParams* tp, const int32_t* sel,
                           int nsel, const int32_t* owner, const EaglePossessionEvent* events, int n_events, int row0, int n, int out_format,
                           const EagleYuvLayout* out_layout, uint8_t* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_minimap_hulls";
    if (!p) fail(EAGLE_E_INVALID, "minimap: params is NULL");
    if (p->control) fail(EAGLE_E_INVALID, "%s: the control layer is not available here (it needs velocities)", who);
    if (frames)
        for (int r = 1; r < rows; ++r)
            if (frames[r] <= frames[r - 1]) fail(EAGLE_E_INVALID, "%s: frame numbers must ascend (row %d: %d after %d)", who, r, frames[r], frames[r - 1]);
    OpLayers ol;
    if (p->layers) {
        ol.on = true; ol.frames = frames; ol.owner = owner; ol.sel = sel; ol.nsel = nsel;
        ol.job.layers = p->layers; ol.job.events = events; ol.job.nev = n_events;
        if (p->layers & (EAGLE_MM_TRAILS | EAGLE_MM_PASSES | EAGLE_MM_OWNER)) {
            if (!tp) fail(EAGLE_E_INVALID, "%s: a layer without trail parameters", who);
            trail_check(who, tp);
            ol.job.tp = *tp;
        }
        if (p->layers & EAGLE_MM_HULLS) { ol.hulls = true; ol.hp = hp; }
    }
    op_minimap(who, device, values, nullptr, columns, rows, cols, team_ids, team_vals, n_team, p, nullptr, row0, n, out_format, out_layout, out, &ol);
    API_END(hh)
}

int eagle_op_trajectory_picture(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                                const int32_t* team_vals, int n_team, const int32_t* sel, int nsel, int row0, int n, int scale, int margin, int half_width, int max_gap,
                                uint8_t* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_trajectory_picture";
    EagleMinimapParams p{};
    p.scale = scale; p.margin = margin;
    OpLayers ol;
    ol.on = true; ol.frames = frames; ol.sel = sel; ol.nsel = nsel;
    ol.job.trajectory = true;
    ol.job.tp.window = 1; ol.job.tp.max_gap = max_gap; ol.job.tp.half_width = half_width; ol.job.tp.pass_hold = 1; ol.job.tp.dim_floor = 256;
    trail_check(who, &ol.job.tp);
    op_minimap(who, device, values, nullptr, columns, rows, cols, team_ids, team_vals, n_team, &p, nullptr, row0, n, EAGLE_PIX_BGR, nullptr, out, &ol);
    API_END(hh)
}

int eagle_op_pass_picture(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals,
                          int n_team, const EaglePossessionEvent* events, int n_events, int event, int scale, int margin, int half_width, uint8_t* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_pass_picture";
    EagleMinimapParams p{};
    p.scale = scale; p.margin = margin;
    OpLayers ol;
    ol.on = true;
    ol.job.tp.window = 1; ol.job.tp.max_gap = 1; ol.job.tp.half_width = half_width; ol.job.tp.pass_hold = 1; ol.job.tp.dim_floor = 256;
    trail_check(who, &ol.job.tp);
    if (!events || n_events < 0) fail(EAGLE_E_INVALID, "%s: bad events (%p, %d)", who, (const void*)events, n_events);
    if (event < 0 || event >= n_events) fail(EAGLE_E_INVALID, "%s: event %d lies outside the %d events", who, event, n_events);
    events_check(who, events, n_events, rows);
    ol.job.events = events; ol.job.nev = n_events; ol.job.only_event = event;
    op_minimap(who, device, values, nullptr, columns, rows, cols, team_ids, team_vals, n_team, &p, nullptr, events[event].release_row, 1, EAGLE_PIX_BGR, nullptr, out, &ol);
    API_END(hh)
}

}  // extern "C"
