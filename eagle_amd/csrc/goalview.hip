// K41 — goal view: a processed table resident in HBM (post.hip) -> per row, attacking group and point (every member, the ball, optionally every cell of
// the pitch) the 64-bit mask of the goal-mouth slices that the other team's discs hide, and the open angle as an exact integer sum of slice weights
// (include/eagle.h, eagle_post_goal_view / eagle_op_goal_view; tests/goalview_ref.py is the written definition of every bit: float64 one operation at a
// time, no contraction, correctly rounded sqrt and division, integer sums).  Groups, keepers and the quantisation are K33's (offside_columns).
//
// Ranges: |q| <= 2^20, a position is q / 1024 or (i + 0.5) / R, so every difference of coordinates and every square of one is exact in float64; a
// weight is at most 2^24 DY / min_depth < 2^21 and a sum of 64 below 2^27.
//
//   goalview_prepare_kernel one thread per (attacking group, row), rows along the wave: walks K33's list and writes the row's blockers (q, the keeper bit)
//                           column-wise, [group][slot][row], and their number (all of them, the first 32 are kept).
//   goalview_points_kernel  one lane per (point, row), the points being the members and the ball once per group: status, the shadow loop, the weights of
//                           the open slices on the fly (the ball: all 64, for `full`).
//   goalview_rows_kernel    one thread per (group, row): the record from the ball's result, the best member and the owner.
//   goalview_totals_kernel  one workgroup per member: integer sums and a (open, earliest row) maximum as one 64-bit key.
//   goalview_table_kernel   form TABLE: per goal and cell the 65 prefix sums of its weights, once per call.
//   goalview_grid_kernel    the hot path: a workgroup takes one row and a tile of 16 x 16 cells, a wave an 8 x 8 block of it, so that a block beyond
//                           max_range leaves as a whole wave; the row's blockers are staged once in LDS as doubles, the barrier behind the staging also
//                           votes whether any cell of the tile is evaluated.  A lane takes one cell: at most 32 shadows, then the open runs of the mask by
//                           count-trailing-zero steps: a division per open slice (DIRECT) or two table reads per run (TABLE).
// A shadow's slices are found from an estimate of the two bounds that is then moved until it satisfies the definition (the centres ascend strictly), so
// the 64 comparisons of the definition are never made and their result is kept.
#include "trails.h"

static_assert(sizeof(EagleGoalViewParams) == 72 && sizeof(EagleGoalViewRow) == 56 && sizeof(EagleGoalViewTotals) == 32, "include/eagle.h states these sizes");

namespace eagle {

static constexpr int GV_B = EAGLE_GOALVIEW_BLOCKERS, GV_S = EAGLE_GOALVIEW_SLICES, GV_TILE = 16, GV_MAX_ROWS = 1 << 20;
static constexpr double GV_Y0 = 30.34, GV_DY = 7.32 / 64.0, GV_TWO24 = 16777216.0;
static_assert(GV_B == 32 && GV_S == 64, "a row's keeper bits are one word, a mask is one 64-bit word");
typedef unsigned long long gv_u64;

struct GvArgs {
    const double2* values;       // [column][row]
    const int4* list;            // K33's: {column, group (2: keeper), member index, 0} in table order
    const int32_t* gcols;        // member index -> column
    const int32_t* member_of;    // [table columns] -> member index or -1
    const int32_t* owner;        // [rows] or nullptr
    int rows, nl, n0, n1, ball, ncols, dir;
    double rad, krad, min_depth, range2;
    int chance_q;
    // scratch
    int2* bq;                    // [2][GV_B][rows]
    uint32_t* kbits;             // [2][rows]: slot k is a keeper
    int32_t* cnt;                // [2][rows]
    int4* ballres;               // [2][rows]: {status, open, full, 0}
    gv_u64* ballmask;            // [2][rows]
    // kept
    EagleGoalViewRow* rec;       // [rows][2]
    int32_t* open; gv_u64* mask; uint8_t* status;    // [members][rows]
    EagleGoalViewTotals* totals; // preset (col, group)
    // grid
    int R, gw, gh, grid_row0, grid_rows, group, table;
    int32_t* W;                  // [2][gh][gw][65]
    uint8_t* grid;               // [grid_rows][gh][gw]
};

__device__ __forceinline__ bool gv_quantise(double2 v, int& qx, int& qy)
{
    if (!(fabs(v.x) <= MM_DOMAIN) || !(fabs(v.y) <= MM_DOMAIN)) return false;          // K33's rule
    qx = (int)floor(v.x * 1024.0 + 0.5); qy = (int)floor(v.y * 1024.0 + 0.5);
    return true;
}

__device__ __forceinline__ bool gv_right(int dir, int g) { return (dir == EAGLE_OFFSIDE_DIR_RIGHT) == (g == 0); }
__device__ __forceinline__ double gv_yc(int k) { return GV_Y0 + ((double)k + 0.5) * GV_DY; }

// #{k : yc_k < v} (or <= v): an estimate, moved until it is the count; the centres ascend strictly, so the count is the one g with yc_(g-1) below and yc_g not
template <bool INCLUSIVE>
__device__ __forceinline__ int gv_count(double v)
{
    const double e = fmin(fmax((v - GV_Y0) / GV_DY, 0.0), 64.0);
    int g = (int)e;
    while (g > 0 && !(INCLUSIVE ? gv_yc(g - 1) <= v : gv_yc(g - 1) < v)) --g;
    while (g < GV_S && (INCLUSIVE ? gv_yc(g) <= v : gv_yc(g) < v)) ++g;
    return g;
}

__device__ __forceinline__ double gv_reach(double py, double s, double tx, double ty)
{
    if (s > 0.0 ? tx > 0.0 : tx < 0.0) return py + (ty * s) / tx;
    return copysign(__longlong_as_double(0x7ff0000000000000LL), ty);
}

// the slices that the disc (bx, by, rho; r2 = rho rho) hides from P
__device__ __forceinline__ gv_u64 gv_shadow(double px, double py, double s, double xg, double bx, double by, double rho, double r2)
{
    const double wx = bx - px, gx = xg - bx;
    if (!(s > 0.0 ? (wx > 0.0 && gx >= 0.0) : (wx < 0.0 && gx <= 0.0))) return 0;
    const double wy = by - py;
    const double d2 = wx * wx + wy * wy;
    if (d2 <= r2) return ~0ull;
    const double l = sqrt(d2 - r2);
    const double lx = l * wx, ly = l * wy, rx = rho * wx, ry = rho * wy;
    const double y1 = gv_reach(py, s, lx - ry, ly + rx), y2 = gv_reach(py, s, lx + ry, ly - rx);
    const double lo = y1 <= y2 ? y1 : y2, hi = y1 <= y2 ? y2 : y1;
    const int a = gv_count<false>(lo), b = gv_count<true>(hi);       // blocked: a <= k < b
    if (b <= a) return 0;
    const int n = b - a;
    return (n >= 64 ? ~0ull : (1ull << n) - 1ull) << a;
}

__device__ __forceinline__ int gv_weight(double num, double ss, double py, int k)
{
    const double e = gv_yc(k) - py;
    return (int)rint(GV_TWO24 * (num / (ss + e * e)));
}

// the status of an evaluated row's point, s and x_g
__device__ __forceinline__ int gv_point(const GvArgs& a, bool right, double px, double py, double& s, double& xg)
{
    xg = right ? 105.0 : 0.0;
    s = xg - px;
    if (fabs(s) < a.min_depth) return EAGLE_GOALVIEW_PT_NEAR_LINE;
    const double ey = 34.0 - py;
    if (s * s + ey * ey > a.range2) return EAGLE_GOALVIEW_PT_FAR;
    return EAGLE_GOALVIEW_PT_OK;
}

__global__ __launch_bounds__(64) void goalview_prepare_kernel(GvArgs a)
{
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= 2ll * a.rows) return;
    const int g = (int)(idx / a.rows), r = (int)(idx % a.rows);
    const bool right = gv_right(a.dir, g);
    int n = 0;
    uint32_t kb = 0;
    for (int k = 0; k < a.nl; ++k) {
        const int4 m = a.list[k];
        if (m.y == g) continue;
        int qx, qy;
        if (!gv_quantise(a.values[(size_t)m.x * a.rows + r], qx, qy)) continue;
        if (m.y == 2 && (right ? qx : EAGLE_OFFSIDE_U_MAX - qx) <= EAGLE_OFFSIDE_U_HALF) continue;      // K33: a keeper outside g's attacking half is nobody's
        if (n < GV_B) {
            a.bq[((size_t)g * GV_B + n) * a.rows + r] = make_int2(qx, qy);
            if (m.y == 2) kb |= 1u << n;
        }
        ++n;
    }
    a.cnt[idx] = n; a.kbits[idx] = kb;
}

__global__ __launch_bounds__(256) void goalview_points_kernel(GvArgs a)
{
    const int nm = a.n0 + a.n1;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)(nm + 2) * a.rows) return;
    const int p = (int)(idx / a.rows), r = (int)(idx % a.rows);
    const bool isball = p >= nm;
    const int g = isball ? p - nm : p < a.n0 ? 0 : 1;
    const int col = isball ? a.ball : a.gcols[p];
    const int n = a.cnt[(size_t)g * a.rows + r];
    int st = EAGLE_GOALVIEW_PT_ABSENT, open = -1, full = 0, qx = 0, qy = 0;
    gv_u64 mask = 0;
    if (col >= 0 && gv_quantise(a.values[(size_t)col * a.rows + r], qx, qy)) {
        if (n > GV_B) {
            st = EAGLE_GOALVIEW_PT_ROW;
        } else {
            const double px = (double)qx / 1024.0, py = (double)qy / 1024.0;
            double s, xg;
            st = gv_point(a, gv_right(a.dir, g), px, py, s, xg);
            if (st == EAGLE_GOALVIEW_PT_FAR) open = 0;
            if (st == EAGLE_GOALVIEW_PT_OK) {
                const uint32_t kb = a.kbits[(size_t)g * a.rows + r];
                for (int k = 0; k < n; ++k) {
                    const int2 b = a.bq[((size_t)g * GV_B + k) * a.rows + r];
                    const double rho = (kb >> k) & 1 ? a.krad : a.rad;
                    mask |= gv_shadow(px, py, s, xg, (double)b.x / 1024.0, (double)b.y / 1024.0, rho, rho * rho);
                }
                const double num = GV_DY * fabs(s), ss = s * s;
                open = 0;
                if (isball) {
                    for (int k = 0; k < GV_S; ++k) {
                        const int w = gv_weight(num, ss, py, k);
                        full += w;
                        open += (mask >> k) & 1 ? 0 : w;
                    }
                } else {
                    for (gv_u64 um = ~mask; um; um &= um - 1) open += gv_weight(num, ss, py, __builtin_ctzll(um));
                }
            }
        }
    }
    if (isball) {
        a.ballres[(size_t)g * a.rows + r] = make_int4(st, open, full, 0);
        a.ballmask[(size_t)g * a.rows + r] = mask;
    } else {
        a.open[idx] = open; a.mask[idx] = mask; a.status[idx] = (uint8_t)st;
    }
}

__global__ __launch_bounds__(64) void goalview_rows_kernel(GvArgs a)
{
    const long long idx = (long long)blockIdx.x * 64 + threadIdx.x;
    if (idx >= 2ll * a.rows) return;
    const int g = (int)(idx / a.rows), r = (int)(idx % a.rows);
    const int n = a.cnt[idx];
    const int4 b = a.ballres[idx];
    EagleGoalViewRow o{};
    o.status = n > GV_B ? EAGLE_GOALVIEW_TOO_MANY : EAGLE_GOALVIEW_OK; o.n_blockers = n;
    o.ball_status = b.x; o.ball_open = b.y; o.ball_full = b.z; o.ball_mask = a.ballmask[idx];
    o.best_col = -1; o.best_open = -1; o.owner_col = -1; o.owner_open = -1;
    for (int k = g ? a.n0 : 0; k < (g ? a.n0 + a.n1 : a.n0); ++k) {
        if (a.status[(size_t)k * a.rows + r] != EAGLE_GOALVIEW_PT_OK) continue;
        const int v = a.open[(size_t)k * a.rows + r];
        if (v > o.best_open) { o.best_open = v; o.best_col = a.gcols[k]; }            // the columns of a group ascend: a tie keeps the smaller
    }
    if (a.owner) {
        const int oc = a.owner[r];
        const int m = oc >= 0 && oc < a.ncols ? a.member_of[oc] : -1;
        if (m >= 0 && (m < a.n0 ? 0 : 1) == g) {
            o.owner_col = oc; o.owner_open = a.open[(size_t)m * a.rows + r]; o.owner_mask = a.mask[(size_t)m * a.rows + r];
        }
    }
    a.rec[(size_t)r * 2 + g] = o;
}

__global__ __launch_bounds__(256) void goalview_totals_kernel(GvArgs a)
{
    __shared__ long long part[4][4];
    const int m = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long n = 0, ch = 0, sum = 0, key = -1;                           // key: open << 32 | (2^31 - 1 - row): the largest open, of equal ones the earliest row
    for (int r = threadIdx.x; r < a.rows; r += 256) {
        if (a.status[(size_t)m * a.rows + r] != EAGLE_GOALVIEW_PT_OK) continue;
        const long long v = a.open[(size_t)m * a.rows + r];
        ++n; sum += v; ch += v >= a.chance_q ? 1 : 0;
        key = max(key, (v << 32) | (long long)(0x7fffffff - r));
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n += __shfl_xor(n, d, 64); ch += __shfl_xor(ch, d, 64); sum += __shfl_xor(sum, d, 64); key = max(key, __shfl_xor(key, d, 64));
    }
    if (lane == 0) { part[wave][0] = n; part[wave][1] = ch; part[wave][2] = sum; part[wave][3] = key; }
    __syncthreads();
    if (threadIdx.x == 0) {
        EagleGoalViewTotals* T = a.totals + m;
        const long long k = max(max(part[0][3], part[1][3]), max(part[2][3], part[3][3]));
        T->rows = (int)(part[0][0] + part[1][0] + part[2][0] + part[3][0]);
        T->chance_rows = (int)(part[0][1] + part[1][1] + part[2][1] + part[3][1]);
        T->sum_open = part[0][2] + part[1][2] + part[2][2] + part[3][2];
        T->max_open = k < 0 ? -1 : (int)(k >> 32);
        T->max_row = k < 0 ? -1 : 0x7fffffff - (int)(k & 0x7fffffff);
    }
}

// W[goal][cell][0 .. 64]: the prefix sums of the cell's weights towards goal 0 (x = 0) and 1 (x = 105); a cell that is not evaluated is never read
__global__ __launch_bounds__(256) void goalview_table_kernel(GvArgs a)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int cells = a.gw * a.gh;
    if (idx >= 2ll * cells) return;
    const int goal = (int)(idx / cells), c = (int)(idx % cells);
    const double px = ((double)(c % a.gw) + 0.5) / (double)a.R, py = ((double)(c / a.gw) + 0.5) / (double)a.R;
    double s, xg;
    if (gv_point(a, goal == 1, px, py, s, xg) != EAGLE_GOALVIEW_PT_OK) return;
    const double num = GV_DY * fabs(s), ss = s * s;
    int32_t* W = a.W + (size_t)idx * (GV_S + 1);
    int acc = 0;
    W[0] = 0;
    for (int k = 0; k < GV_S; ++k) { acc += gv_weight(num, ss, py, k); W[k + 1] = acc; }
}

__global__ __launch_bounds__(256) void goalview_grid_kernel(GvArgs a, int tiles_x, int ntiles)
{
    __shared__ double s_bx[GV_B], s_by[GV_B], s_rho[GV_B], s_r2[GV_B];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int gr = (int)(blockIdx.x / (unsigned)ntiles), tile = (int)(blockIdx.x % (unsigned)ntiles);      // gr < grid_rows: the launch has grid_rows * ntiles workgroups
    const int r = a.grid_row0 + gr;
    const int i = (tile % tiles_x) * GV_TILE + (wave & 1) * 8 + (lane & 7), j = (tile / tiles_x) * GV_TILE + (wave >> 1) * 8 + (lane >> 3);
    const bool inside = i < a.gw && j < a.gh;
    uint8_t* out = a.grid + ((size_t)gr * a.gh + (inside ? j : 0)) * a.gw + (inside ? i : 0);
    int g = a.group;
    if (g < 0) {                                                          // the owner's group (uniform over the workgroup, as n below)
        const int oc = a.owner[r];
        const int m = oc >= 0 && oc < a.ncols ? a.member_of[oc] : -1;
        g = m < 0 ? -1 : m < a.n0 ? 0 : 1;
    }
    const int n = g < 0 ? GV_B + 1 : a.cnt[(size_t)g * a.rows + r];
    if (n > GV_B) {                                                       // nobody's row, or TOO_MANY: zeros
        if (inside) *out = 0;
        return;
    }
    const bool right = gv_right(a.dir, g);
    if (tid < n) {
        const int2 b = a.bq[((size_t)g * GV_B + tid) * a.rows + r];
        const double rho = (a.kbits[(size_t)g * a.rows + r] >> tid) & 1 ? a.krad : a.rad;
        s_bx[tid] = (double)b.x / 1024.0; s_by[tid] = (double)b.y / 1024.0; s_rho[tid] = rho; s_r2[tid] = rho * rho;
    }
    const double px = ((double)i + 0.5) / (double)a.R, py = ((double)j + 0.5) / (double)a.R;
    double s, xg;
    const bool ok = inside && gv_point(a, right, px, py, s, xg) == EAGLE_GOALVIEW_PT_OK;
    const int any = __syncthreads_or(ok ? 1 : 0);                         // the barrier behind the staging; a tile without an evaluated cell leaves whole
    (void)any;
    if (!ok) {
        if (inside) *out = 0;
        return;
    }
    gv_u64 mask = 0;
    for (int k = 0; k < n; ++k) mask |= gv_shadow(px, py, s, xg, s_bx[k], s_by[k], s_rho[k], s_r2[k]);
    int open = 0;
    if (a.table) {
        const int32_t* W = a.W + ((size_t)(right ? 1 : 0) * a.gw * a.gh + (size_t)j * a.gw + i) * (GV_S + 1);
        for (gv_u64 um = ~mask; um;) {
            const int k0 = __builtin_ctzll(um);
            const gv_u64 t = ~(um >> k0);                                 // the run's length: the zeros above shift in as ones of t
            const int len = t ? __builtin_ctzll(t) : GV_S - k0;
            open += W[k0 + len] - W[k0];
            um &= ~((len >= 64 ? ~0ull : (1ull << len) - 1ull) << k0);
        }
    } else {
        const double num = GV_DY * fabs(s), ss = s * s;
        for (gv_u64 um = ~mask; um; um &= um - 1) open += gv_weight(num, ss, py, __builtin_ctzll(um));
    }
    *out = (uint8_t)min(255, open >> 16);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void goalview_check(const char* who, const EagleGoalViewParams* p, int rows, bool has_owner)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the goal-view parameters are NULL", who);
    const double v[5] = {p->radius, p->keeper_radius, p->min_depth, p->max_range, p->chance};
    static const char* const names[5] = {"radius", "keeper_radius", "min_depth", "max_range", "chance"};
    for (int k = 0; k < 5; ++k)
        if (!std::isfinite(v[k])) fail(EAGLE_E_INVALID, "%s: %s %g is not finite", who, names[k], v[k]);
    for (int k = 0; k < 2; ++k)
        if (!(v[k] >= 0.0 && v[k] <= 16.0)) fail(EAGLE_E_INVALID, "%s: %s %g is outside [0, 16] m", who, names[k], v[k]);
    if (!(p->min_depth >= 1.0)) fail(EAGLE_E_INVALID, "%s: min_depth %g is below 1 m", who, p->min_depth);
    if (!(p->max_range > p->min_depth && p->max_range <= 1024.0)) fail(EAGLE_E_INVALID, "%s: max_range %g must lie above min_depth %g and within 1024 m", who, p->max_range, p->min_depth);
    if (!(p->chance >= 0.0 && p->chance <= 4.0)) fail(EAGLE_E_INVALID, "%s: chance %g is outside [0, 4] rad", who, p->chance);
    if (p->cells_per_metre != 1 && p->cells_per_metre != 2 && p->cells_per_metre != 4)
        fail(EAGLE_E_INVALID, "%s: cells_per_metre %d is none of 1, 2, 4", who, p->cells_per_metre);
    if (p->direction != EAGLE_OFFSIDE_DIR_AUTO && p->direction != EAGLE_OFFSIDE_DIR_RIGHT && p->direction != EAGLE_OFFSIDE_DIR_LEFT)
        fail(EAGLE_E_INVALID, "%s: direction %d is none of 0, EAGLE_OFFSIDE_DIR_RIGHT, _LEFT", who, p->direction);
    if (p->group < -1 || p->group > 1) fail(EAGLE_E_INVALID, "%s: group %d is none of -1, 0, 1", who, p->group);
    if (p->form < EAGLE_GOALVIEW_FORM_DEFAULT || p->form > EAGLE_GOALVIEW_FORM_TABLE) fail(EAGLE_E_INVALID, "%s: form %d is no EAGLE_GOALVIEW_FORM_*", who, p->form);
    if (p->reserved[0] || p->reserved[1]) fail(EAGLE_E_INVALID, "%s: a reserved word of the parameters is not 0", who);
    if (p->grid_rows < 0 || p->grid_row0 < 0 || (p->grid_rows > 0 && (long long)p->grid_row0 + p->grid_rows > rows))
        fail(EAGLE_E_INVALID, "%s: the grid's rows %d .. %lld lie outside the table's %d rows", who, p->grid_row0, (long long)p->grid_row0 + p->grid_rows - 1, rows);
    if (p->grid_rows > 0 && p->group < 0 && !has_owner) fail(EAGLE_E_INVALID, "%s: group -1 (the owner's group) needs a possession result", who);
    if (rows > GV_MAX_ROWS) fail(EAGLE_E_INVALID, "%s: %d rows, at most %d", who, rows, GV_MAX_ROWS);
}

static size_t gv_up(size_t b) { return (std::max<size_t>(b, 16) + 255) & ~(size_t)255; }

// What a call keeps: records | open | mask | status | totals | grid, each from a 256-byte boundary
struct GvKept { size_t rec, open, mask, status, totals, grid, total; };

static GvKept goalview_kept(size_t rows, size_t nm, size_t grid_rows, int R)
{
    GvKept o{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += gv_up(b); return was; };
    o.rec = take(rows * 2 * sizeof(EagleGoalViewRow)); o.open = take(nm * rows * 4); o.mask = take(nm * rows * 8); o.status = take(nm * rows);
    o.totals = take(nm * sizeof(EagleGoalViewTotals)); o.grid = take(grid_rows * (size_t)(68 * R) * (size_t)(105 * R));
    o.total = at;
    return o;
}

// the scratch of a call
struct GvScratch { size_t list, gcols, member_of, bq, kbits, cnt, ballres, ballmask, W, total; };

static GvScratch goalview_scratch(const OfCols& oc, size_t rows, bool table, int R)
{
    GvScratch o{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += gv_up(b); return was; };
    o.list = take(oc.list.size() * sizeof(int4)); o.gcols = take(oc.gcols.size() * 4); o.member_of = take(oc.member_of.size() * 4);
    o.bq = take(2 * (size_t)GV_B * rows * sizeof(int2)); o.kbits = take(2 * rows * 4); o.cnt = take(2 * rows * 4); o.ballres = take(2 * rows * sizeof(int4));
    o.ballmask = take(2 * rows * 8); o.W = take(table ? 2 * (size_t)(68 * R) * (size_t)(105 * R) * (GV_S + 1) * 4 : 0);
    o.total = at;
    return o;
}

static bool goalview_uses_table(const EagleGoalViewParams* p)
{
    // the default is the table: table plus grid is 2.8 to 3.1 times faster than the divisions at R = 1, 2 and 4 (docs/experiments.md, "Goal view (K41)")
    return p->grid_rows > 0 && p->form != EAGLE_GOALVIEW_FORM_DIRECT;
}

static void goalview_budget(const char* who, size_t need, int64_t max_bytes)
{
    double budget = (double)max_bytes;
    if (max_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = 0.9 * (double)free_b;
    }
    if ((double)need > budget) fail(EAGLE_E_INVALID, "%s: the call needs %.0f bytes of device memory, the budget is %.0f", who, (double)need, budget);
}

// The whole table (rows > 0) -> a result at d (goalview_kept bytes); scratch: goalview_scratch bytes.  dir: resolved.  Returns when it is complete.
static void goalview_table(EagleHandle* h, const char* who, const OfCols& oc, const double2* d_values, int rows, int ncols, const int32_t* d_owner, const EagleGoalViewParams* p,
                           int dir, uint8_t* d, uint8_t* scratch, hipStream_t s, float* times_ms)
{
    const size_t nm = oc.gcols.size();
    const bool table = goalview_uses_table(p);
    const int R = p->cells_per_metre;
    const GvKept K = goalview_kept((size_t)rows, nm, (size_t)p->grid_rows, R);
    const GvScratch S = goalview_scratch(oc, (size_t)rows, table, R);
    GvArgs a{};
    a.values = d_values; a.owner = d_owner; a.rows = rows; a.nl = (int)oc.list.size(); a.n0 = oc.n0; a.n1 = oc.n1; a.ball = oc.ball; a.ncols = ncols; a.dir = dir;
    a.rad = p->radius; a.krad = p->keeper_radius; a.min_depth = p->min_depth; a.range2 = p->max_range * p->max_range;
    a.chance_q = (int)std::rint(GV_TWO24 * p->chance);
    a.list = (const int4*)(scratch + S.list); a.gcols = (const int32_t*)(scratch + S.gcols); a.member_of = (const int32_t*)(scratch + S.member_of);
    a.bq = (int2*)(scratch + S.bq); a.kbits = (uint32_t*)(scratch + S.kbits); a.cnt = (int32_t*)(scratch + S.cnt); a.ballres = (int4*)(scratch + S.ballres);
    a.ballmask = (gv_u64*)(scratch + S.ballmask); a.W = (int32_t*)(scratch + S.W);
    a.rec = (EagleGoalViewRow*)(d + K.rec); a.open = (int32_t*)(d + K.open); a.mask = (gv_u64*)(d + K.mask); a.status = d + K.status;
    a.totals = (EagleGoalViewTotals*)(d + K.totals); a.grid = d + K.grid;
    a.R = R; a.gw = 105 * R; a.gh = 68 * R; a.grid_row0 = p->grid_row0; a.grid_rows = p->grid_rows; a.group = p->group; a.table = table ? 1 : 0;
    std::vector<EagleGoalViewTotals> init(nm);
    for (size_t k = 0; k < nm; ++k) { init[k] = EagleGoalViewTotals{}; init[k].col = oc.gcols[k]; init[k].group = (int)k < oc.n0 ? 0 : 1; init[k].max_open = -1; init[k].max_row = -1; }
    auto up = [&](const void* dst, const void* src, size_t b) {
        if (b) HIP_CHECK(hipMemcpyAsync((void*)dst, src, b, hipMemcpyHostToDevice, s));
    };
    up(a.list, oc.list.data(), oc.list.size() * sizeof(int4));
    up(a.gcols, oc.gcols.data(), oc.gcols.size() * 4);
    up(a.member_of, oc.member_of.data(), oc.member_of.size() * 4);
    up(a.totals, init.data(), nm * sizeof(EagleGoalViewTotals));
    hipEvent_t ev[6] = {};
    try {
        if (times_ms)
            for (hipEvent_t& e : ev) HIP_CHECK(hipEventCreate(&e));
        auto stamp = [&](int k) { if (times_ms) HIP_CHECK(hipEventRecord(ev[k], s)); };
        auto run = [&](const char* name, double bytes, const std::function<void()>& fn) {
            if (h) timed_launch(h, name, bytes, s, fn); else fn();
            HIP_CHECK(hipGetLastError());
        };
        const double n = (double)rows;
        const unsigned g2 = (unsigned)((2 * (size_t)rows + 63) / 64);       // (waves of 64 rows: a column's load is one run of 1024 bytes)
        stamp(0);
        run("goalview_prepare", n * 2.0 * (16.0 * a.nl + 8.0 * GV_B + 8.0), [&] { hipLaunchKernelGGL(goalview_prepare_kernel, dim3(g2), dim3(64), 0, s, a); });
        stamp(1);
        run("goalview_points", n * (double)(nm + 2) * (16.0 + 8.0 * GV_B + 13.0),
            [&] { hipLaunchKernelGGL(goalview_points_kernel, dim3((unsigned)(((nm + 2) * (size_t)rows + 255) / 256)), dim3(256), 0, s, a); });
        stamp(2);
        run("goalview_rows", n * (2.0 * 80.0 + 5.0 * (double)nm + 13.0 * (double)nm), [&] {
            hipLaunchKernelGGL(goalview_rows_kernel, dim3(g2), dim3(64), 0, s, a);
            if (nm) hipLaunchKernelGGL(goalview_totals_kernel, dim3((unsigned)nm), dim3(256), 0, s, a);
        });
        stamp(3);
        if (p->grid_rows > 0) {
            const int tiles_x = (a.gw + GV_TILE - 1) / GV_TILE, ntiles = tiles_x * ((a.gh + GV_TILE - 1) / GV_TILE);
            const double cells = (double)a.gw * a.gh;
            if ((double)p->grid_rows * ntiles > 2147483647.0) fail(EAGLE_E_INVALID, "%s: %d grid rows of %d tiles are more workgroups than a launch takes", who, p->grid_rows, ntiles);
            if (table)
                run("goalview_table", 2.0 * cells * 260.0, [&] { hipLaunchKernelGGL(goalview_table_kernel, dim3((unsigned)((2 * (size_t)a.gw * a.gh + 255) / 256)), dim3(256), 0, s, a); });
            stamp(4);
            run("goalview_grid", (double)p->grid_rows * (cells + 8.0 * GV_B + 12.0),
                [&] { hipLaunchKernelGGL(goalview_grid_kernel, dim3((unsigned)((size_t)p->grid_rows * ntiles)), dim3(256), 0, s, a, tiles_x, ntiles); });
        } else {
            stamp(4);
        }
        stamp(5);
        HIP_CHECK(hipStreamSynchronize(s));
        if (h && h->prof) collect_spans(h);
        if (times_ms) {
            for (int k = 0; k < 5; ++k) HIP_CHECK(hipEventElapsedTime(&times_ms[k], ev[k], ev[k + 1]));
            HIP_CHECK(hipEventElapsedTime(&times_ms[5], ev[0], ev[5]));
            if (!(p->grid_rows > 0 && table)) times_ms[3] = 0.0f;         // no table launch: what lies between the two stamps is not a time of anything
            if (!(p->grid_rows > 0)) times_ms[4] = 0.0f;
        }
    } catch (...) {
        (void)hipStreamSynchronize(s);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        throw;
    }
    for (hipEvent_t e : ev) if (e) HIP_CHECK(hipEventDestroy(e));
}

static OfCols goalview_columns(const char* who, const EaglePostColumn* columns, int ncols, bool no_ball, const int32_t* team_ids, const int32_t* team_vals, size_t n_team)
{
    EagleOffsideParams op{};                                             // (offside_columns only copies the direction into its clip record)
    return offside_columns(who, columns, ncols, no_ball, team_ids, team_vals, n_team, &op);
}

}  // namespace eagle

extern "C" {

int eagle_goal_view_params_default(EagleGoalViewParams* p)
{
    if (!p) return EAGLE_E_INVALID;
    *p = EagleGoalViewParams{};
    p->direction = EAGLE_OFFSIDE_DIR_AUTO; p->group = 0; p->cells_per_metre = 1; p->form = EAGLE_GOALVIEW_FORM_DEFAULT;
    p->radius = 0.4; p->keeper_radius = 1.0; p->min_depth = 1.0; p->max_range = 40.0; p->chance = 0.3;
    return EAGLE_OK;
}

int eagle_post_goal_view(EagleHandle* h, EaglePostTable* t, const EagleGoalViewParams* p)
{
    API_BEGIN_H(h)
    const char* who = "eagle_post_goal_view";
    if (!t) fail(EAGLE_E_INVALID, "%s: table is NULL", who);
    if (t->h != h) fail(EAGLE_E_INVALID, "%s: the table belongs to another handle", who);
    goalview_check(who, p, t->rows, t->has_poss);
    const int32_t none = 0;
    const OfCols oc = goalview_columns(who, t->columns.data(), t->cols, (t->flags & EAGLE_POST_NO_BALL) != 0,
                                       !t->has_team ? nullptr : t->team_ids.empty() ? &none : t->team_ids.data(), t->team_vals.data(), t->has_team ? t->team_ids.size() : 0);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    int dir = p->direction;
    if (dir == EAGLE_OFFSIDE_DIR_AUTO) {
        if (!t->d_offside) fail(EAGLE_E_INVALID, "%s: direction 0 takes the offside result's direction and the table has none (eagle_post_offside)", who);
        const EagleOffsideRow* d_rows; const int32_t* d_margins; const EagleOffsideTotals* d_totals; const EagleOffsideClip* d_clip; const EagleOffsideEvent* d_events;
        if (eagle_post_device_offside(t, &d_rows, &d_margins, &d_totals, &d_clip, &d_events, nullptr, nullptr) != EAGLE_OK || !d_clip)
            fail(EAGLE_E_INVALID, "%s: the table's offside result cannot be read", who);
        EagleOffsideClip clip{};
        if (t->rows) HIP_CHECK(hipMemcpy(&clip, d_clip, sizeof(clip), hipMemcpyDeviceToHost));
        dir = clip.direction;
        if (dir != EAGLE_OFFSIDE_DIR_RIGHT && dir != EAGLE_OFFSIDE_DIR_LEFT) fail(EAGLE_E_INVALID, "%s: the table's offside result settled no direction", who);
    }
    const size_t rows = (size_t)t->rows, nm = oc.gcols.size();
    const GvKept K = goalview_kept(rows, nm, (size_t)p->grid_rows, p->cells_per_metre);
    const GvScratch S = goalview_scratch(oc, rows, goalview_uses_table(p), p->cells_per_metre);
    goalview_budget(who, K.total + S.total, t->max_bytes);
    uint8_t *d = nullptr, *scratch = nullptr;
    try {
        HIP_CHECK(hipMalloc((void**)&d, K.total));
        if (rows) {
            HIP_CHECK(hipMalloc((void**)&scratch, S.total));
            const int32_t* d_owner = t->has_poss ? (const int32_t*)((const double*)t->d_poss + t->rows) + t->rows : nullptr;
            goalview_table(h, who, oc, (const double2*)t->d_values, t->rows, t->cols, d_owner, p, dir, d, scratch, h->s_main, nullptr);
        } else {
            HIP_CHECK(hipMemset(d, 0, K.total));
        }
    } catch (...) {
        (void)hipStreamSynchronize(h->s_main);
        if (scratch) (void)hipFree(scratch);
        if (d) (void)hipFree(d);
        throw;
    }
    if (scratch) HIP_CHECK(hipFree(scratch));
    if (t->d_goalview) (void)hipFree(t->d_goalview);                     // a later call replaces the result
    t->d_goalview = d;
    t->goalview_members = (int)nm; t->goalview_grid_row0 = p->grid_row0; t->goalview_grid_rows = p->grid_rows; t->goalview_R = p->cells_per_metre;
    API_END(h)
}

int eagle_post_goal_view_values(EaglePostTable* t, EagleGoalViewRow* rows_out, int32_t* open, uint64_t* mask, uint8_t* status, EagleGoalViewTotals* totals, uint8_t* grid)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->d_goalview) fail(EAGLE_E_INVALID, "eagle_post_goal_view_values: the table has no goal view (eagle_post_goal_view)");
    const size_t rows = (size_t)t->rows, nm = (size_t)t->goalview_members, gr = (size_t)t->goalview_grid_rows;
    if (rows) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        const uint8_t* d = (const uint8_t*)t->d_goalview;
        const GvKept K = goalview_kept(rows, nm, gr, t->goalview_R);
        if (rows_out) HIP_CHECK(hipMemcpy(rows_out, d + K.rec, rows * 2 * sizeof(EagleGoalViewRow), hipMemcpyDeviceToHost));
        if (open && nm) HIP_CHECK(hipMemcpy(open, d + K.open, nm * rows * 4, hipMemcpyDeviceToHost));
        if (mask && nm) HIP_CHECK(hipMemcpy(mask, d + K.mask, nm * rows * 8, hipMemcpyDeviceToHost));
        if (status && nm) HIP_CHECK(hipMemcpy(status, d + K.status, nm * rows, hipMemcpyDeviceToHost));
        if (totals && nm) HIP_CHECK(hipMemcpy(totals, d + K.totals, nm * sizeof(EagleGoalViewTotals), hipMemcpyDeviceToHost));
        if (grid && gr) HIP_CHECK(hipMemcpy(grid, d + K.grid, gr * (size_t)(68 * t->goalview_R) * (size_t)(105 * t->goalview_R), hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_post_device_goal_view(const EaglePostTable* t, const EagleGoalViewRow** d_rows, const int32_t** d_open, const uint64_t** d_mask, const uint8_t** d_status,
                                const EagleGoalViewTotals** d_totals, const uint8_t** d_grid, int* n_members, int* grid_row0, int* grid_rows, int* cells_per_metre)
{
    if (!t || !d_rows || !d_open || !d_mask || !d_status || !d_totals || !d_grid) return EAGLE_E_INVALID;
    const uint8_t* d = (const uint8_t*)t->d_goalview;
    const eagle::GvKept K = eagle::goalview_kept((size_t)t->rows, (size_t)t->goalview_members, (size_t)t->goalview_grid_rows, t->goalview_R);
    *d_rows = d ? (const EagleGoalViewRow*)(d + K.rec) : nullptr;
    *d_open = d ? (const int32_t*)(d + K.open) : nullptr;
    *d_mask = d ? (const uint64_t*)(d + K.mask) : nullptr;
    *d_status = d ? d + K.status : nullptr;
    *d_totals = d ? (const EagleGoalViewTotals*)(d + K.totals) : nullptr;
    *d_grid = d && t->goalview_grid_rows ? d + K.grid : nullptr;
    if (n_members) *n_members = d ? t->goalview_members : 0;
    if (grid_row0) *grid_row0 = d ? t->goalview_grid_row0 : 0;
    if (grid_rows) *grid_rows = d ? t->goalview_grid_rows : 0;
    if (cells_per_metre) *cells_per_metre = d ? t->goalview_R : 0;
    return EAGLE_OK;
}

int eagle_op_goal_view(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals, int n_team,
                       const int32_t* owner, const EagleGoalViewParams* p, EagleGoalViewRow* rows_out, int32_t* open, uint64_t* mask, uint8_t* status,
                       EagleGoalViewTotals* totals, uint8_t* grid, int* n_members, float* times_ms)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_goal_view";
    if (!values || !columns || rows < 0 || cols < 0 || n_team < 0 || (team_ids && n_team > 0 && !team_vals))
        fail(EAGLE_E_INVALID, "%s: bad argument (values %p, columns %p, %d rows, %d columns, %d teams)", who, (const void*)values, (const void*)columns, rows, cols, n_team);
    goalview_check(who, p, rows, owner != nullptr);
    if (p->direction == EAGLE_OFFSIDE_DIR_AUTO) fail(EAGLE_E_INVALID, "%s: direction 0 takes a table's offside result; the operator entry has none", who);
    const OfCols oc = goalview_columns(who, columns, cols, false, team_ids, team_vals, (size_t)n_team);
    const size_t nr = (size_t)rows, nm = oc.gcols.size();
    if (n_members) *n_members = (int)nm;
    if (rows == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    const GvKept K = goalview_kept(nr, nm, (size_t)p->grid_rows, p->cells_per_metre);
    const GvScratch S = goalview_scratch(oc, nr, goalview_uses_table(p), p->cells_per_metre);
    goalview_budget(who, (size_t)cols * nr * sizeof(double2) + K.total + S.total, 0);
    float times[EAGLE_GOALVIEW_TIMES] = {};
    Net net;
    const double2* d_v = (const double2*)net.upload(values, std::max<size_t>((size_t)cols * nr * sizeof(double2), 16));
    const int32_t* d_owner = owner ? (const int32_t*)net.upload(owner, nr * 4) : nullptr;
    uint8_t* d = (uint8_t*)net.get(K.total);
    goalview_table(nullptr, who, oc, d_v, rows, cols, d_owner, p, p->direction, d, (uint8_t*)net.get(S.total), nullptr, times_ms ? times : nullptr);
    if (rows_out) HIP_CHECK(hipMemcpy(rows_out, d + K.rec, nr * 2 * sizeof(EagleGoalViewRow), hipMemcpyDeviceToHost));
    if (open && nm) HIP_CHECK(hipMemcpy(open, d + K.open, nm * nr * 4, hipMemcpyDeviceToHost));
    if (mask && nm) HIP_CHECK(hipMemcpy(mask, d + K.mask, nm * nr * 8, hipMemcpyDeviceToHost));
    if (status && nm) HIP_CHECK(hipMemcpy(status, d + K.status, nm * nr, hipMemcpyDeviceToHost));
    if (totals && nm) HIP_CHECK(hipMemcpy(totals, d + K.totals, nm * sizeof(EagleGoalViewTotals), hipMemcpyDeviceToHost));
    if (grid && p->grid_rows) HIP_CHECK(hipMemcpy(grid, d + K.grid, (size_t)p->grid_rows * (size_t)(68 * p->cells_per_metre) * (size_t)(105 * p->cells_per_metre), hipMemcpyDeviceToHost));
    if (times_ms) std::copy(times, times + EAGLE_GOALVIEW_TIMES, times_ms);
    API_END(hh)
}

}  // extern "C"
