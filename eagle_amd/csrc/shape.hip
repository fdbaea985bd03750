// K26 — team shape: a processed table resident in HBM (post.hip) -> per row and group (team 0 / every other team) the number of present members, the
// integer sums and extrema of their quantised positions and their exact convex hull (include/eagle.h, eagle_post_team_shape / eagle_op_team_shape;
// tests/shape_ref.py is the written definition of every bit).  One float64 step, q = floor(x * 1024 + 0.5); integers after it: |q| <= 2^20, differences
// <= 2^21, every product <= 2^43 and formed in 64 bits.
//
// Two launches per call on one stream, a third for the minimap's hull layer:
//   shape_stats_kernel   one thread per row walks the member columns, group 0's and then group 1's (the host decides per COLUMN who is a member, as
//                        possession_columns does).  The table is [column][row][2]: a wave's load is one run of 1024 bytes.  Its stores are a record
//                        of 96 bytes per thread and group, uncoalesced; against the loads of tens of columns per row they are a few per cent.
//   shape_hull_kernel    one wave per (row, group); a workgroup owns `tile` consecutive rows of one group and first stages their quantised cells into
//                        LDS as int2 [member][row in tile] (the global loads run along rows; an absent cell is the sentinel SH_ABSENT).  Then a gift
//                        wrapping march per wave: every lane takes the members lane, lane + 64, ... and keeps its best under the contract's BEATS
//                        rule, a butterfly of __shfl_xor picks the wave's winner (BEATS is a strict total order of the candidates, so every order of
//                        comparisons returns the same maximum: tests/shape_ref.py), lane k keeps vertex k in a register.  No atomics, no compaction,
//                        no cap on the member count.
//   shape_edges_kernel   one thread per (picture, group, stored vertex): the two end points of the hull edge leaving that vertex in the minimap's
//                        quantisation (mm_quantise), or MM_ABSENT for no edge; minimap.hip draws them.
// LDS: the row stride of the staged cells is tile + 1 (tile > 1), so that the 32 lanes of a ds_read_b64 group, 8 (tile + 1) bytes apart, fall into 32
// different bank pairs (2 (tile + 1) words is twice an odd number: 32 distinct even banks of 64).
#include "trails.h"

namespace eagle {

static constexpr int SH_THREADS = 256;                 // statistics kernel
static constexpr int SH_ABSENT = (int)0x80000000;
static constexpr int SH_TILE_MAX = 16;                 // rows (= waves) per workgroup of the hull kernel: 1024 threads
// Bytes of staged cells per workgroup.  A CU has 160 KB of LDS and room for 32 waves, two workgroups of 16: with 32 KB each the staging of five
// workgroups fits, so LDS never decides how many are resident, and it stays inside the 64 KB a kernel may take without asking for more.  One row per
// workgroup is the least there is, 8 bytes per member: 32 KB / 8 B = 4096 members, the cap of the contract (EAGLE_SHAPE_MAX_MEMBERS).
static constexpr int SH_LDS_BUDGET = 32768;
static_assert(EAGLE_SHAPE_MAX_MEMBERS * 8 == SH_LDS_BUDGET, "the member cap is what one row per workgroup stages");

struct ShapeArgs {
    const double2* values;       // [column][row]
    const int32_t* gcols;        // group 0's columns in table order, then group 1's
    int rows, n0, n1;
    EagleTeamShape* shapes;      // [rows][2]
    int32_t* hull;               // [rows][2][EAGLE_SHAPE_HULL_CAP]
    int tile, tile_shift, stride;        // hull kernel: rows per workgroup (a power of two), its log2, int2 per member in LDS
};

__device__ __forceinline__ bool sh_quantise(double2 v, int& qx, int& qy)
{
    if (!(fabs(v.x) <= MM_DOMAIN) || !(fabs(v.y) <= MM_DOMAIN)) return false;          // NaN, +-inf and the far field: the minimap's rule
    qx = (int)floor(v.x * 1024.0 + 0.5);
    qy = (int)floor(v.y * 1024.0 + 0.5);
    return true;
}

__global__ __launch_bounds__(SH_THREADS) void shape_stats_kernel(ShapeArgs a)
{
    const int r = blockIdx.x * SH_THREADS + threadIdx.x;
    if (r >= a.rows) return;
    #pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int32_t* C = a.gcols + (g ? a.n0 : 0);
        const int ng = g ? a.n1 : a.n0;
        long long sx = 0, sy = 0, sxx = 0, syy = 0;
        int n = 0, lx = 0, hx = 0, ly = 0, hy = 0, clx = -1, chx = -1, cly = -1, chy = -1;
        for (int k = 0; k < ng; ++k) {
            const int c = C[k];                                          // (uniform)
            int qx, qy;
            if (!sh_quantise(a.values[(size_t)c * a.rows + r], qx, qy)) continue;
            sx += qx; sy += qy; sxx += (long long)qx * qx; syy += (long long)qy * qy;
            if (n == 0 || qx < lx) { lx = qx; clx = c; }                 // strict: a tie keeps the earlier column
            if (n == 0 || qx > hx) { hx = qx; chx = c; }
            if (n == 0 || qy < ly) { ly = qy; cly = c; }
            if (n == 0 || qy > hy) { hy = qy; chy = c; }
            ++n;
        }
        EagleTeamShape o{};                                              // (hull_n, area2, flags: the hull kernel, behind this one on the stream)
        o.sum_x = sx; o.sum_y = sy; o.sum_xx = sxx; o.sum_yy = syy; o.n = n;
        o.min_x = lx; o.max_x = hx; o.min_y = ly; o.max_y = hy;
        o.col_min_x = clx; o.col_max_x = chx; o.col_min_y = cly; o.col_max_y = chy;
        a.shapes[(size_t)r * 2 + g] = o;
    }
}

// the contract's BEATS: p beats b as the next vertex after c; m = member index (the members are listed in column order)
__device__ __forceinline__ bool sh_beats(int cx, int cy, int px, int py, int pm, int bx, int by, int bm)
{
    const long long o = (long long)(bx - cx) * (py - cy) - (long long)(by - cy) * (px - cx);
    if (o) return o < 0;
    const long long dp = (long long)(px - cx) * (px - cx) + (long long)(py - cy) * (py - cy), db = (long long)(bx - cx) * (bx - cx) + (long long)(by - cy) * (by - cy);
    if (dp != db) return dp > db;
    return pm < bm;
}

__global__ __launch_bounds__(64 * SH_TILE_MAX) void shape_hull_kernel(ShapeArgs a)
{
    extern __shared__ int2 s_q[];                                        // [members of the group][stride]
    const int g = blockIdx.y, ng = g ? a.n1 : a.n0;
    const int32_t* C = a.gcols + (g ? a.n0 : 0);
    const int row0 = blockIdx.x * a.tile;
    for (int i = threadIdx.x; i < ng * a.tile; i += blockDim.x) {        // (ng * tile <= 4096 * 16)
        const int m = i >> a.tile_shift, rit = i & (a.tile - 1), r = row0 + rit;
        int2 q = make_int2(SH_ABSENT, 0);
        int qx, qy;
        if (r < a.rows && sh_quantise(a.values[(size_t)C[m] * a.rows + r], qx, qy)) q = make_int2(qx, qy);
        s_q[m * a.stride + rit] = q;
    }
    __syncthreads();                                                     // (the only barrier: a wave may leave behind it)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = row0 + wave;
    if (r >= a.rows) return;
    const int2* S = s_q + wave;
    // ---- the start: the smallest (qy, qx, member), and the number of present members ----
    int bm = -1, bx = 0, by = 0, cnt = 0;
    for (int m = lane; m < ng; m += 64) {
        const int2 q = S[m * a.stride];
        if (q.x == SH_ABSENT) continue;
        ++cnt;
        if (bm < 0 || q.y < by || (q.y == by && q.x < bx)) { bm = m; bx = q.x; by = q.y; }      // (m ascends: a tie stays)
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int om = __shfl_xor(bm, d, 64), ox = __shfl_xor(bx, d, 64), oy = __shfl_xor(by, d, 64);
        cnt += __shfl_xor(cnt, d, 64);
        if (om >= 0 && (bm < 0 || oy < by || (oy == by && (ox < bx || (ox == bx && om < bm))))) { bm = om; bx = ox; by = oy; }
    }
    int hv = -1, k = 0;                                                  // lane j holds stored vertex j
    long long area2 = 0;
    if (bm >= 0) {
        const int sm = bm, sx = bx, sy = by;
        if (lane == 0) hv = C[sm];
        k = 1;
        int cx = sx, cy = sy;
        for (int step = 0; step < cnt; ++step) {
            int pm = -1, px = 0, py = 0;
            for (int m = lane; m < ng; m += 64) {
                const int2 q = S[m * a.stride];
                if (q.x == SH_ABSENT || (q.x == cx && q.y == cy)) continue;
                if (pm < 0 || sh_beats(cx, cy, q.x, q.y, m, px, py, pm)) { pm = m; px = q.x; py = q.y; }
            }
            #pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const int om = __shfl_xor(pm, d, 64), ox = __shfl_xor(px, d, 64), oy = __shfl_xor(py, d, 64);
                if (om >= 0 && (pm < 0 || sh_beats(cx, cy, ox, oy, om, px, py, pm))) { pm = om; px = ox; py = oy; }
            }
            if (pm < 0 || pm == sm) break;                               // (uniform: every lane holds the same winner)
            area2 += (long long)(cx - sx) * (py - sy) - (long long)(cy - sy) * (px - sx);
            if (lane == k) hv = C[pm];                                   // (k >= 64: nobody; lanes 32 .. 63 are not stored)
            ++k; cx = px; cy = py;
        }
    }
    if (lane < EAGLE_SHAPE_HULL_CAP) a.hull[((size_t)r * 2 + g) * EAGLE_SHAPE_HULL_CAP + lane] = hv;
    if (lane == 0) {
        EagleTeamShape* o = a.shapes + (size_t)r * 2 + g;
        o->hull_n = k; o->area2 = area2; o->flags = k > EAGLE_SHAPE_HULL_CAP ? EAGLE_SHAPE_CUT : 0;
    }
}

__global__ __launch_bounds__(256) void shape_edges_kernel(const double2* values, int rows, const EagleTeamShape* shapes, const int32_t* hull, int row0, int n, int scale,
                                                          int margin, int4* edges)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 2 * EAGLE_SHAPE_HULL_CAP) return;
    const int f = i / (2 * EAGLE_SHAPE_HULL_CAP), g = i / EAGLE_SHAPE_HULL_CAP & 1, e = i % EAGLE_SHAPE_HULL_CAP;
    const size_t rg = (size_t)(row0 + f) * 2 + g;
    const int hn = shapes[rg].hull_n, k = min(hn, EAGLE_SHAPE_HULL_CAP);
    const int ne = hn < 2 ? 0 : hn == 2 ? 1 : (shapes[rg].flags & EAGLE_SHAPE_CUT) ? k - 1 : k;
    int4 o = make_int4(MM_ABSENT, 0, 0, 0);
    if (e < ne) {
        const int32_t* H = hull + rg * EAGLE_SHAPE_HULL_CAP;
        const int ca = H[e], cb = H[e + 1 == k ? 0 : e + 1];
        const double K = (double)(16 * scale);
        const int ox = 16 * margin, oy = 16 * margin + 16 * 68 * scale;
        int ax, ay, bx, by;
        if (mm_quantise(values[(size_t)ca * rows + (size_t)(row0 + f)], K, ox, oy, ax, ay) && mm_quantise(values[(size_t)cb * rows + (size_t)(row0 + f)], K, ox, oy, bx, by))
            o = make_int4(ax, ay, bx, by);                               // (a vertex is present under the same rule: always)
    }
    edges[i] = o;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
ShapeCols shape_columns(const char* who, const EaglePostColumn* columns, int ncols, const int32_t* team_ids, const int32_t* team_vals, size_t n_team)
{
    if (!team_ids) fail(EAGLE_E_INVALID, "%s: team shape needs a table with a team mapping (team 0 is set against the others)", who);
    std::vector<int32_t> g[2];
    for (int c = 0; c < ncols; ++c) {
        const EaglePostColumn& col = columns[c];
        if (col.kind != EAGLE_POST_PLAYER && col.kind != EAGLE_POST_GOALKEEPER && col.kind != EAGLE_POST_BALL && col.kind != EAGLE_POST_BOUNDARY)
            fail(EAGLE_E_INVALID, "%s: column %d is of unknown kind %d", who, c, col.kind);
        if (col.video || col.kind != EAGLE_POST_PLAYER) continue;
        size_t k = 0;
        while (k < n_team && team_ids[k] != col.id) ++k;                 // the first entry counts, as in possession_columns
        if (k == n_team || team_vals[k] < 0) continue;
        g[team_vals[k] == 0 ? 0 : 1].push_back(c);
    }
    if (g[0].size() + g[1].size() > (size_t)EAGLE_SHAPE_MAX_MEMBERS)
        fail(EAGLE_E_INVALID, "%s: %zu team members are beyond %d", who, g[0].size() + g[1].size(), EAGLE_SHAPE_MAX_MEMBERS);
    ShapeCols sc;
    sc.n0 = (int)g[0].size(); sc.n1 = (int)g[1].size();
    sc.gcols = g[0];
    sc.gcols.insert(sc.gcols.end(), g[1].begin(), g[1].end());
    return sc;
}

void hull_check(const char* who, const EagleHullParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the hull parameters are NULL", who);
    if (p->half_width < 1 || p->half_width > 8) fail(EAGLE_E_INVALID, "%s: half_width %d must lie within 1 .. 8 pixels", who, p->half_width);
}

void shape_run(EagleHandle* h, const ShapeCols& sc, const double2* d_values, int rows, EagleTeamShape* d_shapes, int32_t* d_hull, hipStream_t s)
{
    if (rows <= 0) return;
    const int nmem = sc.n0 + sc.n1;
    int32_t* d_cols = nullptr;
    HIP_CHECK(hipMalloc((void**)&d_cols, std::max<size_t>((size_t)nmem * 4, 16)));
    try {
        if (nmem) HIP_CHECK(hipMemcpyAsync(d_cols, sc.gcols.data(), (size_t)nmem * 4, hipMemcpyHostToDevice, s));
        ShapeArgs a{};
        a.values = d_values; a.gcols = d_cols; a.rows = rows; a.n0 = sc.n0; a.n1 = sc.n1; a.shapes = d_shapes; a.hull = d_hull;
        // rows per workgroup: the largest power of two whose staged cells (all members, whichever group they are in: the bound the cap rests on) fit the budget
        a.tile = SH_TILE_MAX;
        while (a.tile > 1 && (size_t)nmem * (a.tile + 1) * sizeof(int2) > (size_t)SH_LDS_BUDGET) a.tile >>= 1;
        a.stride = a.tile > 1 ? a.tile + 1 : 1;
        for (a.tile_shift = 0; (1 << a.tile_shift) < a.tile; ++a.tile_shift) {}
        const size_t lds = (size_t)std::max(std::max(sc.n0, sc.n1), 1) * a.stride * sizeof(int2);
        auto stats = [&] {
            hipLaunchKernelGGL(shape_stats_kernel, dim3((rows + SH_THREADS - 1) / SH_THREADS), dim3(SH_THREADS), 0, s, a);
            HIP_CHECK(hipGetLastError());
        };
        auto hulls = [&] {
            hipLaunchKernelGGL(shape_hull_kernel, dim3((rows + a.tile - 1) / a.tile, 2), dim3(64 * a.tile), lds, s, a);
            HIP_CHECK(hipGetLastError());
        };
        // bytes: every member cell read once by each kernel; 192 bytes of records per row written, 40 of them again, 256 of vertices
        const double cells = 16.0 * (double)nmem * (double)rows;
        if (h) {
            timed_launch(h, "shape_stats", cells + 192.0 * rows, s, stats);
            timed_launch(h, "shape_hull", cells + 296.0 * rows, s, hulls);
        } else { stats(); hulls(); }
        HIP_CHECK(hipStreamSynchronize(s));
        if (h && h->prof) collect_spans(h);
    } catch (...) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(d_cols);
        throw;
    }
    HIP_CHECK(hipFree(d_cols));
}

void shape_edges_launch(const double2* values, int rows, const EagleTeamShape* shapes, const int32_t* hull, int row0, int n, int scale, int margin, int4* edges, hipStream_t s)
{
    if (n <= 0) return;
    const int total = n * 2 * EAGLE_SHAPE_HULL_CAP;
    hipLaunchKernelGGL(shape_edges_kernel, dim3((total + 255) / 256), dim3(256), 0, s, values, rows, shapes, hull, row0, n, scale, margin, edges);
    HIP_CHECK(hipGetLastError());
}

}  // namespace eagle

extern "C" {

int eagle_post_team_shape(EagleHandle* h, EaglePostTable* t)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_team_shape: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_team_shape: the table belongs to another handle");
    const int32_t none = 0;                                              // (a mapping of no entries is a mapping: nobody is a member)
    const ShapeCols sc = shape_columns("eagle_post_team_shape", t->columns.data(), t->cols, !t->has_team ? nullptr : t->team_ids.empty() ? &none : t->team_ids.data(),
                                       t->team_vals.data(), t->has_team ? t->team_ids.size() : 0);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)t->rows;
    if (!t->d_shape) HIP_CHECK(hipMalloc((void**)&t->d_shape, std::max<size_t>(rows * 2 * (sizeof(EagleTeamShape) + 4 * EAGLE_SHAPE_HULL_CAP), 16)));
    t->has_shape = true;
    shape_run(h, sc, (const double2*)t->d_values, t->rows, (EagleTeamShape*)t->d_shape, (int32_t*)((EagleTeamShape*)t->d_shape + rows * 2), h->s_main);
    API_END(h)
}

int eagle_post_team_shape_values(EaglePostTable* t, EagleTeamShape* shapes, int32_t* hull)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->has_shape) fail(EAGLE_E_INVALID, "eagle_post_team_shape_values: the table has no team shape (eagle_post_team_shape)");
    const size_t rows = (size_t)t->rows;
    if (rows) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        const EagleTeamShape* d = (const EagleTeamShape*)t->d_shape;
        if (shapes) HIP_CHECK(hipMemcpy(shapes, d, rows * 2 * sizeof(EagleTeamShape), hipMemcpyDeviceToHost));
        if (hull) HIP_CHECK(hipMemcpy(hull, d + rows * 2, rows * 2 * 4 * EAGLE_SHAPE_HULL_CAP, hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_post_device_team_shape(const EaglePostTable* t, const EagleTeamShape** d_shapes, const int32_t** d_hull)
{
    if (!t || !d_shapes || !d_hull) return EAGLE_E_INVALID;
    const EagleTeamShape* d = t->has_shape ? (const EagleTeamShape*)t->d_shape : nullptr;
    *d_shapes = d;
    *d_hull = d ? (const int32_t*)(d + (size_t)t->rows * 2) : nullptr;
    return EAGLE_OK;
}

int eagle_minimap_set_hulls(EaglePostTable* t, const EagleHullParams* p)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (p) {
        hull_check("eagle_minimap_set_hulls", p);
        t->hulls = *p;
    }
    t->has_hulls = p != nullptr;
    API_END(h)
}

int eagle_op_team_shape(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals, int n_team,
                        EagleTeamShape* shapes, int32_t* hull)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !columns || rows < 0 || cols < 0 || n_team < 0 || (team_ids && n_team > 0 && !team_vals))
        fail(EAGLE_E_INVALID, "eagle_op_team_shape: bad argument (values %p, columns %p, %d rows, %d columns, %d teams)", (const void*)values, (const void*)columns, rows,
             cols, n_team);
    const ShapeCols sc = shape_columns("eagle_op_team_shape", columns, cols, team_ids, team_vals, (size_t)n_team);
    if (rows == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const size_t n = (size_t)rows;
    const double2* d_v = (const double2*)net.upload(values, std::max<size_t>((size_t)cols * n * sizeof(double2), 16));
    EagleTeamShape* d_s = (EagleTeamShape*)net.get(n * 2 * (sizeof(EagleTeamShape) + 4 * EAGLE_SHAPE_HULL_CAP));
    int32_t* d_h = (int32_t*)(d_s + n * 2);
    shape_run(nullptr, sc, d_v, rows, d_s, d_h, nullptr);
    if (shapes) HIP_CHECK(hipMemcpy(shapes, d_s, n * 2 * sizeof(EagleTeamShape), hipMemcpyDeviceToHost));
    if (hull) HIP_CHECK(hipMemcpy(hull, d_h, n * 2 * 4 * EAGLE_SHAPE_HULL_CAP, hipMemcpyDeviceToHost));
    API_END(hh)
}

}  // extern "C"
