// K30 — space per player: a processed table resident in HBM (post.hip) -> per row the exact dominant region of every present member on the pitch grid (the
// cells nearer to it than to anybody else, per third), the nearest opponent and the opponents within a radius, and per member the totals over the clip
// (include/eagle.h, eagle_post_space / eagle_op_space / eagle_space_grids; tests/space_ref.py is the written definition of every bit).  Members of groups
// 0 and 1 and the quantisation are K26's (shape_columns; q = floor(x * 1024 + 0.5)); the goalkeepers are group 2.  Integers after that: a difference
// between a cell centre and a site is below 2^21, between two sites at most 2^21, a squared distance at most 2^43; counts are added with integer atomics,
// so no result depends on an order.  No floating point behind the quantisation.
//
//   space_sites_kernel     one wave per row.  The lanes take the member columns 64 at a time in table order; a ballot's prefix count compacts the
//                          present ones into the row's site list (LDS, 512 bytes per wave).  Lane s then marks site s against all S <= 32 sites (a
//                          broadcast read per site, ascending with a strict <: the earlier column wins a tie) and writes its record; the lanes up to
//                          32 write the unused slots, lane 0 the row record.  Every byte of both arrays is written here, the cell counts as zeros.
//   space_cells_kernel     the hot one: <R, MAP>, a workgroup of four waves per (band of SP_BAND cell rows, row).  The row's sites are staged once
//                          in LDS; a lane takes a cell and scans the sites in ascending order with a strict <, the distance as two 32 x 32 -> 64 bit
//                          multiply-adds.  A wave's 64 cells lie side by side and regions are coherent, so the wave counts with a first-lane / ballot
//                          loop over the distinct (owner, third) keys of its cells and lane 0 adds each popcount to the wave's OWN counters in LDS (no
//                          LDS atomic at all).  Behind a barrier the workgroup sums its four counter sets and issues one global atomic per non-zero
//                          (site, third) and one per non-zero (group, third) of the row record.  MAP: the owner's site index is also stored per
//                          cell (255 on a row that is not ACTIVE); compiled out otherwise.
//   space_totals_kernel    a wave per (64 consecutive rows, site slot): a slot mostly holds the same member from row to row, so the wave reduces the
//                          lanes that agree with a butterfly and lane 0 issues one set of atomics per distinct member.  space_totals_close_kernel
//                          then sets min to 0 for a member without rows.
//
// The cells kernel's launch: R = 4 has 68 bands of 1680 cells per row, so a one-row call is 68 workgroups of four waves; 30 000 rows are 2 040 000.
#include "trails.h"

namespace eagle {

static constexpr int SP_CAP = EAGLE_SPACE_SITE_CAP;
static constexpr int SP_BAND = 4;                      // cell rows per workgroup of the cells kernel (68 R is a multiple of it)
static constexpr int SP_KEYS = SP_CAP * 3;             // (owner, third)
static constexpr int SP_PASS = 65535;                  // gridDim.y limit
static constexpr int64_t SP_STAGING = 32 << 20;
typedef unsigned long long sp_u64;
static_assert(sizeof(EagleSpaceParams) == 32 && sizeof(EagleSpaceRow) == 64 && sizeof(EagleSpaceSite) == 48 && sizeof(EagleSpaceTotals) == 64,
              "include/eagle.h states these sizes");
static_assert(SP_CAP == 32 && 68 % SP_BAND == 0, "a site index is a lane of half a wave; a band never crosses the grid's end");

struct SpArgs {
    const double2* values;       // [column][row]
    const int2* mcols;           // the member columns in table order: {column, group}
    const int32_t* member_of;    // [table columns]: the member's index in group order, or -1
    int rows, row0, n, nm;       // the table's rows; the window; the members
    long long rq2;               // the marking radius squared, q^2
    EagleSpaceRow* rows_out;     // [n]
    EagleSpaceSite* sites;       // [n][SP_CAP]
    EagleSpaceTotals* totals;    // [nm], preset (col, group, min = INT32_MAX), or nullptr
    uint8_t* grid;               // [n][gh][gw], or nullptr
    int cbase;                   // cells kernel: blockIdx.y counts the window's rows from here
};

__device__ __forceinline__ bool sp_quantise(double2 v, int& qx, int& qy)
{
    if (!(fabs(v.x) <= MM_DOMAIN) || !(fabs(v.y) <= MM_DOMAIN)) return false;          // NaN, +-inf and the far field: K26's rule
    qx = (int)floor(v.x * 1024.0 + 0.5);
    qy = (int)floor(v.y * 1024.0 + 0.5);
    return true;
}

// the steps of one wave follow each other through LDS: its operations there complete in order, the fence keeps the compiler from moving them
__device__ __forceinline__ void sp_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void space_sites_kernel(SpArgs a)
{
    __shared__ int4 slot[4][SP_CAP];                                      // {qx, qy, column, group}
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= a.n) return;                                                // (uniform over the wave; the kernel has no workgroup barrier)
    int S = 0, ng[3] = {0, 0, 0};
    for (int base = 0; base < a.nm; base += 64) {
        const int k = base + lane;
        int2 m = make_int2(-1, -1);
        int qx = 0, qy = 0;
        bool ok = false;
        if (k < a.nm) {
            m = a.mcols[k];
            ok = sp_quantise(a.values[(size_t)m.x * a.rows + (size_t)(a.row0 + r)], qx, qy);
        }
        const sp_u64 b = __ballot(ok);
        const int at = S + __popcll(b & (((sp_u64)1 << lane) - 1));
        if (ok && at < SP_CAP) slot[wave][at] = make_int4(qx, qy, m.x, m.y);
        S += __popcll(b);
        #pragma unroll
        for (int g = 0; g < 3; ++g) ng[g] += __popcll(__ballot(ok && m.y == g));
    }
    sp_wave_sync();
    const int status = S == 0 ? EAGLE_SPACE_EMPTY : S > SP_CAP ? EAGLE_SPACE_TOO_MANY : EAGLE_SPACE_ACTIVE;
    if (lane < SP_CAP) {
        EagleSpaceSite o{};
        o.near_d2 = -1; o.col = -1; o.near_col = -1;
        if (status == EAGLE_SPACE_ACTIVE && lane < S) {
            const int4 me = slot[wave][lane];
            o.col = me.z; o.group = me.w; o.qx = me.x; o.qy = me.y;
            for (int s = 0; s < S; ++s) {                                // ascending, strict <: of equal distances the earlier column
                const int4 ot = slot[wave][s];
                const long long dx = ot.x - me.x, dy = ot.y - me.y;
                const long long d2 = dx * dx + dy * dy;                  // <= 2^43
                if (me.w < 2 && ot.w == 1 - me.w) {
                    if (o.near_col < 0 || d2 < o.near_d2) { o.near_d2 = d2; o.near_col = ot.z; }
                    o.within += d2 <= a.rq2 ? 1 : 0;
                }
            }
        }
        a.sites[(size_t)r * SP_CAP + lane] = o;
    }
    if (lane == 0) {
        EagleSpaceRow o{};
        o.status = status; o.n_sites = S; o.n[0] = ng[0]; o.n[1] = ng[1]; o.n[2] = ng[2];
        a.rows_out[r] = o;
    }
}

template <int R, bool MAP>
__global__ __launch_bounds__(256) void space_cells_kernel(SpArgs a)
{
    constexpr int GW = 105 * R, GH = 68 * R, HALF = 512 / R, NCELL = SP_BAND * GW;
    __shared__ int2 sq[SP_CAP];
    __shared__ int32_t sgrp[SP_CAP];
    __shared__ uint32_t cnt[4][SP_KEYS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = a.cbase + blockIdx.y, j0 = blockIdx.x * SP_BAND;       // (r < n and j0 + SP_BAND <= GH by the launch)
    EagleSpaceRow* ro = a.rows_out + r;
    const int S = __builtin_amdgcn_readfirstlane(ro->status == EAGLE_SPACE_ACTIVE ? ro->n_sites : 0);
    uint8_t* G = MAP ? a.grid + ((size_t)r * GH + j0) * GW : nullptr;
    if (S == 0) {                                                        // (uniform over the workgroup)
        if (MAP)
            for (int i = tid; i < NCELL; i += 256) G[i] = 255;
        return;
    }
    EagleSpaceSite* st = a.sites + (size_t)r * SP_CAP;
    if (tid < S) { sq[tid] = make_int2(st[tid].qx, st[tid].qy); sgrp[tid] = st[tid].group; }
    for (int i = tid; i < 4 * SP_KEYS; i += 256) (&cnt[0][0])[i] = 0;
    __syncthreads();
    uint32_t* C = cnt[wave];
    for (int c0 = wave * 64; c0 < NCELL; c0 += 256) {                    // (uniform over the wave)
        const int idx = c0 + lane;
        const bool live = idx < NCELL;
        const int jj = idx / GW, i = idx - jj * GW;
        const int X = (2 * i + 1) * HALF, Y = (2 * (j0 + jj) + 1) * HALF;
        long long best = 0x7fffffffffffffffLL;
        int own = 0;
        for (int s = 0; s < S; ++s) {
            const int2 q = sq[s];
            const int dx = X - q.x, dy = Y - q.y;                        // |d| < 2^21
            const long long d2 = (long long)dx * dx + (long long)dy * dy;
            own = d2 < best ? s : own;
            best = d2 < best ? d2 : best;
        }
        if (MAP && live) G[idx] = (uint8_t)own;
        const int key = live ? own * 3 + (i < 35 * R ? 0 : i < 70 * R ? 1 : 2) : -1;
        sp_u64 todo = __ballot(live);
        while (todo) {                                                   // the distinct keys of the wave's cells, a few
            const int k = __shfl(key, __ffsll((long long)todo) - 1, 64);
            const sp_u64 m = __ballot(key == k);
            if (lane == 0) C[k] += (uint32_t)__popcll(m);
            todo &= ~m;
        }
    }
    __syncthreads();
    if (tid < SP_KEYS) {
        const uint32_t v = cnt[0][tid] + cnt[1][tid] + cnt[2][tid] + cnt[3][tid];
        cnt[0][tid] = v;
        if (v) atomicAdd(&st[tid / 3].cells[tid % 3], (int32_t)v);
    }
    __syncthreads();
    if (tid < 9) {
        const int g = tid / 3, t = tid % 3;
        uint32_t v = 0;
        for (int s = 0; s < S; ++s) v += sgrp[s] == g ? cnt[0][s * 3 + t] : 0;
        if (v) atomicAdd(&ro->cells[g][t], (int32_t)v);
    }
}

__global__ __launch_bounds__(256) void space_totals_kernel(SpArgs a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slot = blockIdx.y * 4 + wave, r = blockIdx.x * 64 + lane;
    int m = -1, c0 = 0, c1 = 0, c2 = 0, opp = 0, within = 0;
    if (r < a.n && a.rows_out[r].status == EAGLE_SPACE_ACTIVE && slot < a.rows_out[r].n_sites) {
        const EagleSpaceSite* s = a.sites + (size_t)r * SP_CAP + slot;
        m = a.member_of[s->col];
        c0 = s->cells[0]; c1 = s->cells[1]; c2 = s->cells[2];
        opp = s->near_col >= 0 ? 1 : 0; within = s->within;
    }
    sp_u64 todo = __ballot(m >= 0);
    while (todo) {                                                       // (uniform: every lane stays in the loop)
        const int k = __shfl(m, __ffsll((long long)todo) - 1, 64);
        const bool mine = m == k;
        const sp_u64 mask = __ballot(mine);
        const int tot = c0 + c1 + c2;
        int v[6] = {mine ? c0 : 0, mine ? c1 : 0, mine ? c2 : 0, mine ? opp : 0, mine && within > 0 ? 1 : 0, mine ? within : 0};       // 64 x 114 240 fits
        int mn = mine ? tot : 0x7fffffff, mx = mine ? tot : 0;
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            #pragma unroll
            for (int x = 0; x < 6; ++x) v[x] += __shfl_xor(v[x], d, 64);
            mn = min(mn, __shfl_xor(mn, d, 64));
            mx = max(mx, __shfl_xor(mx, d, 64));
        }
        if (lane == 0) {
            EagleSpaceTotals* T = a.totals + k;
            atomicAdd(&T->rows, __popcll(mask));
            #pragma unroll
            for (int x = 0; x < 3; ++x)
                if (v[x]) atomicAdd((sp_u64*)&T->cells[x], (sp_u64)v[x]);
            atomicMin(&T->min, mn);
            atomicMax(&T->max, mx);
            if (v[3]) atomicAdd(&T->opp_rows, v[3]);
            if (v[4]) atomicAdd(&T->within_rows, v[4]);
            if (v[5]) atomicAdd((sp_u64*)&T->within_sum, (sp_u64)v[5]);
        }
        todo &= ~mask;
    }
}

__global__ __launch_bounds__(256) void space_totals_close_kernel(SpArgs a)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m < a.nm && a.totals[m].rows == 0) a.totals[m].min = 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void space_check(const char* who, const EagleSpaceParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the space parameters are NULL", who);
    if (p->cells_per_metre != 1 && p->cells_per_metre != 2 && p->cells_per_metre != 4)
        fail(EAGLE_E_INVALID, "%s: cells_per_metre %d must be 1, 2 or 4", who, p->cells_per_metre);
    if (!(std::isfinite(p->radius) && p->radius > 0.0 && p->radius <= 1024.0)) fail(EAGLE_E_INVALID, "%s: radius %g must be finite and within (0, 1024] metres", who, p->radius);
    for (int k = 0; k < 4; ++k)
        if (p->reserved[k]) fail(EAGLE_E_INVALID, "%s: reserved word %d of the space parameters is %d, not 0", who, k, p->reserved[k]);
}

static void space_window(const char* who, int rows, int row0, int n)
{
    if (n < 0 || row0 < 0 || row0 > rows || n > rows - row0) fail(EAGLE_E_INVALID, "%s: rows %d .. %d lie outside the table's %d rows", who, row0, row0 + n - 1, rows);
}

struct SpCols { std::vector<int2> mcols; std::vector<int32_t> member_of; std::vector<EagleSpaceTotals> init; };

// groups 0 and 1 are the team shape's (and its refusals); group 2: the Goalkeeper pitch columns
static SpCols space_columns(const char* who, const EaglePostColumn* columns, int ncols, const int32_t* team_ids, const int32_t* team_vals, size_t n_team, int goalkeepers)
{
    const ShapeCols sc = shape_columns(who, columns, ncols, team_ids, team_vals, n_team);
    std::vector<int32_t> group((size_t)std::max(ncols, 1), -1);
    for (int k = 0; k < sc.n0 + sc.n1; ++k) group[sc.gcols[k]] = k < sc.n0 ? 0 : 1;
    if (goalkeepers)
        for (int c = 0; c < ncols; ++c)
            if (columns[c].kind == EAGLE_POST_GOALKEEPER && !columns[c].video) group[c] = 2;
    SpCols o;
    o.member_of.assign((size_t)std::max(ncols, 1), -1);
    for (int g = 0; g < 3; ++g)
        for (int c = 0; c < ncols; ++c)
            if (group[c] == g) {
                o.member_of[c] = (int32_t)o.init.size();
                EagleSpaceTotals t{};
                t.col = c; t.group = g; t.min = 0x7fffffff;
                o.init.push_back(t);
            }
    for (int c = 0; c < ncols; ++c)
        if (group[c] >= 0) o.mcols.push_back(make_int2(c, group[c]));
    if (o.mcols.size() > (size_t)EAGLE_SHAPE_MAX_MEMBERS) fail(EAGLE_E_INVALID, "%s: %zu members are beyond %d", who, o.mcols.size(), EAGLE_SHAPE_MAX_MEMBERS);
    return o;
}

static size_t sp_up(size_t b) { return (std::max<size_t>(b, 16) + 255) & ~(size_t)255; }

// a result: records | sites | totals, each from a 256-byte boundary
static size_t space_kept(size_t rows, size_t nm) { return sp_up(rows * sizeof(EagleSpaceRow)) + sp_up(rows * SP_CAP * sizeof(EagleSpaceSite)) + sp_up(nm * sizeof(EagleSpaceTotals)); }
static size_t space_lists(const SpCols& sc) { return sp_up(sc.mcols.size() * sizeof(int2)) + sp_up(sc.member_of.size() * 4); }

static void space_budget(const char* who, size_t need, int64_t max_bytes)
{
    double budget = (double)max_bytes;
    if (max_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = 0.9 * (double)free_b;
    }
    if ((double)need > budget) fail(EAGLE_E_INVALID, "%s: the call needs %.0f bytes of device memory, the budget is %.0f", who, (double)need, budget);
}

// the member lists at `lists` (space_lists bytes); pageable sources: they have left the vectors when this returns
static void space_upload(SpArgs& a, const SpCols& sc, uint8_t* lists, hipStream_t s)
{
    a.nm = (int)sc.mcols.size();
    a.mcols = (const int2*)lists;
    a.member_of = (const int32_t*)(lists + sp_up(sc.mcols.size() * sizeof(int2)));
    if (a.nm) HIP_CHECK(hipMemcpyAsync(lists, sc.mcols.data(), sc.mcols.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync((void*)a.member_of, sc.member_of.data(), sc.member_of.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

template <int R>
static void space_cells_launch(const SpArgs& a, int n, hipStream_t s)
{
    if (a.grid) hipLaunchKernelGGL((space_cells_kernel<R, true>), dim3(68 * R / SP_BAND, n), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((space_cells_kernel<R, false>), dim3(68 * R / SP_BAND, n), dim3(256), 0, s, a);
}

// The launches of rows a.row0 .. a.row0 + a.n - 1 (a.n > 0) on s (h: timed under its profiling mode, or nullptr); enqueued, not awaited.  totals_init: the
// preset totals (a.totals then takes the sums), or nullptr
static void space_launch(EagleHandle* h, SpArgs a, int R, const EagleSpaceTotals* totals_init, hipStream_t s)
{
    auto run = [&](const char* name, double bytes, const std::function<void()>& fn) {
        if (h) timed_launch(h, name, bytes, s, fn); else fn();
    };
    const double n = (double)a.n, cells = 7140.0 * R * R;
    // bytes: the cells of the members read, the records written; the sites read, the maps written; the site records read
    run("space_sites", n * (16.0 * a.nm + 64.0 + 48.0 * SP_CAP), [&] {
        hipLaunchKernelGGL(space_sites_kernel, dim3((a.n + 3) / 4), dim3(256), 0, s, a);
        HIP_CHECK(hipGetLastError());
    });
    run("space_cells", n * (68.0 * R / SP_BAND) * 16.0 * SP_CAP + (a.grid ? n * cells : 0.0), [&] {
        for (int i = 0; i < a.n; i += SP_PASS) {
            SpArgs b = a;
            b.cbase = i;
            const int k = std::min(SP_PASS, a.n - i);
            if (R == 1) space_cells_launch<1>(b, k, s); else if (R == 2) space_cells_launch<2>(b, k, s); else space_cells_launch<4>(b, k, s);
            HIP_CHECK(hipGetLastError());
        }
    });
    if (a.totals && a.nm) {
        HIP_CHECK(hipMemcpyAsync(a.totals, totals_init, (size_t)a.nm * sizeof(EagleSpaceTotals), hipMemcpyHostToDevice, s));
        run("space_totals", n * (64.0 + 48.0 * SP_CAP), [&] {
            hipLaunchKernelGGL(space_totals_kernel, dim3((a.n + 63) / 64, SP_CAP / 4), dim3(256), 0, s, a);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(space_totals_close_kernel, dim3((a.nm + 255) / 256), dim3(256), 0, s, a);
            HIP_CHECK(hipGetLastError());
        });
    }
}

static SpArgs space_args(const double2* d_values, int rows, const EagleSpaceParams* p)
{
    SpArgs a{};
    a.values = d_values; a.rows = rows;
    const long long rq = (long long)floor(p->radius * 1024.0 + 0.5);
    a.rq2 = rq * rq;
    return a;
}

// The whole table -> a result at d (space_kept bytes); lists: space_lists bytes.  Returns when it is complete.  rows > 0.
static void space_table(EagleHandle* h, const SpCols& sc, const double2* d_values, int rows, const EagleSpaceParams* p, uint8_t* d, uint8_t* lists, hipStream_t s)
{
    SpArgs a = space_args(d_values, rows, p);
    space_upload(a, sc, lists, s);
    a.row0 = 0; a.n = rows;
    a.rows_out = (EagleSpaceRow*)d;
    a.sites = (EagleSpaceSite*)(d + sp_up((size_t)rows * sizeof(EagleSpaceRow)));
    a.totals = (EagleSpaceTotals*)((uint8_t*)a.sites + sp_up((size_t)rows * SP_CAP * sizeof(EagleSpaceSite)));
    space_launch(h, a, p->cells_per_metre, sc.init.data(), s);
    HIP_CHECK(hipStreamSynchronize(s));
    if (h && h->prof) collect_spans(h);
}

// the scratch of an owner-map call: the lists, and per row of a pass the records, the sites and (host destination) the map
struct SpPlan { int pass; size_t lists, rows, sites, grid, total; };

static SpPlan space_plan(const SpCols& sc, int n, size_t cells, bool own_grid)
{
    const size_t per_row = sizeof(EagleSpaceRow) + SP_CAP * sizeof(EagleSpaceSite) + (own_grid ? cells : 0);
    SpPlan o{};
    o.pass = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(n, SP_PASS), SP_STAGING / (int64_t)per_row));
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += sp_up(b); return was; };
    o.lists = take(space_lists(sc)); o.rows = take((size_t)o.pass * sizeof(EagleSpaceRow)); o.sites = take((size_t)o.pass * SP_CAP * sizeof(EagleSpaceSite));
    o.grid = take(own_grid ? (size_t)o.pass * cells : 0);
    o.total = at;
    return o;
}

// The owner maps of rows row0 .. row0 + n - 1 (n > 0) in passes, to device memory (device) or through staging to host memory; base: pl.total bytes
static void space_maps(EagleHandle* h, const SpCols& sc, const double2* d_values, int rows, int row0, int n, const EagleSpaceParams* p, uint8_t* grid, bool device,
                       uint8_t* base, const SpPlan& pl, hipStream_t s)
{
    const size_t cells = (size_t)7140 * p->cells_per_metre * p->cells_per_metre;
    SpArgs a = space_args(d_values, rows, p);
    space_upload(a, sc, base + pl.lists, s);
    a.rows_out = (EagleSpaceRow*)(base + pl.rows); a.sites = (EagleSpaceSite*)(base + pl.sites);
    for (int i = 0; i < n; i += pl.pass) {
        a.row0 = row0 + i; a.n = std::min(pl.pass, n - i);
        a.grid = device ? grid + (size_t)i * cells : base + pl.grid;
        space_launch(h, a, p->cells_per_metre, nullptr, s);
        if (!device) HIP_CHECK(hipMemcpyAsync(grid + (size_t)i * cells, a.grid, (size_t)a.n * cells, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));                              // (the next pass reuses the records)
        if (h && h->prof) collect_spans(h);
    }
}

static SpCols space_table_columns(const char* who, const EaglePostTable* t, const EagleSpaceParams* p)
{
    const int32_t none = 0;                                              // (a mapping of no entries is a mapping: nobody is a member of groups 0 and 1)
    return space_columns(who, t->columns.data(), t->cols, !t->has_team ? nullptr : t->team_ids.empty() ? &none : t->team_ids.data(), t->team_vals.data(),
                         t->has_team ? t->team_ids.size() : 0, p->goalkeepers);
}

static void space_grids_entry(const char* who, EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleSpaceParams* p, uint8_t* grid, bool device)
{
    if (!t) fail(EAGLE_E_INVALID, "%s: table is NULL", who);
    if (t->h != h) fail(EAGLE_E_INVALID, "%s: the table belongs to another handle", who);
    space_check(who, p);
    const SpCols sc = space_table_columns(who, t, p);
    space_window(who, t->rows, row0, n);
    if (n == 0) return;
    if (!grid) fail(EAGLE_E_INVALID, "%s: grid is NULL", who);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const SpPlan pl = space_plan(sc, n, (size_t)7140 * p->cells_per_metre * p->cells_per_metre, !device);
    space_budget(who, pl.total, t->max_bytes);
    uint8_t* base = nullptr;
    HIP_CHECK(hipMalloc((void**)&base, pl.total));
    try {
        space_maps(h, sc, (const double2*)t->d_values, t->rows, row0, n, p, grid, device, base, pl, h->s_main);
    } catch (...) {
        (void)hipStreamSynchronize(h->s_main);
        (void)hipFree(base);
        throw;
    }
    HIP_CHECK(hipFree(base));
}

}  // namespace eagle

extern "C" {

int eagle_post_space(EagleHandle* h, EaglePostTable* t, const EagleSpaceParams* p)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_space: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_space: the table belongs to another handle");
    space_check("eagle_post_space", p);
    const SpCols sc = space_table_columns("eagle_post_space", t, p);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)t->rows, nm = sc.mcols.size();
    // the budget: the new result and the lists.  The members depend on the parameters, so a result is a buffer of its own: the earlier one stays until
    // the new one is complete, and in place when the call fails
    space_budget("eagle_post_space", space_kept(rows, nm) + space_lists(sc), t->max_bytes);
    uint8_t* d = nullptr;
    uint8_t* lists = nullptr;
    try {
        HIP_CHECK(hipMalloc((void**)&d, space_kept(rows, nm)));
        if (rows) {
            HIP_CHECK(hipMalloc((void**)&lists, space_lists(sc)));
            space_table(h, sc, (const double2*)t->d_values, t->rows, p, d, lists, h->s_main);
        } else {
            HIP_CHECK(hipMemset(d, 0, space_kept(rows, nm)));            // (no launch writes a table without rows)
        }
    } catch (...) {
        (void)hipStreamSynchronize(h->s_main);
        if (lists) (void)hipFree(lists);
        if (d) (void)hipFree(d);
        throw;
    }
    if (lists) HIP_CHECK(hipFree(lists));
    if (t->d_space) (void)hipFree(t->d_space);
    t->d_space = d;
    t->space_members = (int)nm;
    API_END(h)
}

int eagle_post_space_values(EaglePostTable* t, EagleSpaceRow* rows_out, EagleSpaceSite* sites_out, EagleSpaceTotals* totals_out)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->d_space) fail(EAGLE_E_INVALID, "eagle_post_space_values: the table has no space result (eagle_post_space)");
    const size_t rows = (size_t)t->rows, nm = (size_t)t->space_members;
    if (rows) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        const uint8_t* d = (const uint8_t*)t->d_space;
        const size_t rb = sp_up(rows * sizeof(EagleSpaceRow)), sb = sp_up(rows * SP_CAP * sizeof(EagleSpaceSite));
        if (rows_out) HIP_CHECK(hipMemcpy(rows_out, d, rows * sizeof(EagleSpaceRow), hipMemcpyDeviceToHost));
        if (sites_out) HIP_CHECK(hipMemcpy(sites_out, d + rb, rows * SP_CAP * sizeof(EagleSpaceSite), hipMemcpyDeviceToHost));
        if (totals_out && nm) HIP_CHECK(hipMemcpy(totals_out, d + rb + sb, nm * sizeof(EagleSpaceTotals), hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_post_device_space(const EaglePostTable* t, const EagleSpaceRow** d_rows, const EagleSpaceSite** d_sites, const EagleSpaceTotals** d_totals, int* n_members)
{
    if (!t || !d_rows || !d_sites || !d_totals) return EAGLE_E_INVALID;
    const uint8_t* d = (const uint8_t*)t->d_space;
    const size_t rb = eagle::sp_up((size_t)t->rows * sizeof(EagleSpaceRow)), sb = eagle::sp_up((size_t)t->rows * eagle::SP_CAP * sizeof(EagleSpaceSite));
    *d_rows = (const EagleSpaceRow*)d;
    *d_sites = d ? (const EagleSpaceSite*)(d + rb) : nullptr;
    *d_totals = d ? (const EagleSpaceTotals*)(d + rb + sb) : nullptr;
    if (n_members) *n_members = d ? t->space_members : 0;
    return EAGLE_OK;
}

int eagle_space_device_grids(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleSpaceParams* p, uint8_t* d_grid)
{
    API_BEGIN_H(h)
    space_grids_entry("eagle_space_device_grids", h, t, row0, n, p, d_grid, true);
    API_END(h)
}

int eagle_space_grids(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleSpaceParams* p, uint8_t* grid)
{
    API_BEGIN_H(h)
    space_grids_entry("eagle_space_grids", h, t, row0, n, p, grid, false);
    API_END(h)
}

int eagle_op_space(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals, int n_team,
                   const EagleSpaceParams* p, int row0, int n, EagleSpaceRow* rows_out, EagleSpaceSite* sites_out, EagleSpaceTotals* totals_out, uint8_t* grid)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !columns || rows < 0 || cols < 0 || n_team < 0 || (team_ids && n_team > 0 && !team_vals))
        fail(EAGLE_E_INVALID, "eagle_op_space: bad argument (values %p, columns %p, %d rows, %d columns, %d teams)", (const void*)values, (const void*)columns, rows, cols,
             n_team);
    space_check("eagle_op_space", p);
    const SpCols sc = space_columns("eagle_op_space", columns, cols, team_ids, team_vals, (size_t)n_team, p->goalkeepers);
    space_window("eagle_op_space", rows, row0, n);
    if (rows == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    const size_t nr = (size_t)rows, nm = sc.mcols.size(), cells = (size_t)7140 * p->cells_per_metre * p->cells_per_metre;
    const bool maps = grid && n > 0;
    const SpPlan pl = space_plan(sc, std::max(n, 1), cells, true);
    space_budget("eagle_op_space", (size_t)cols * nr * sizeof(double2) + space_kept(nr, nm) + space_lists(sc) + (maps ? pl.total : 0), 0);
    Net net;
    const double2* d_v = (const double2*)net.upload(values, std::max<size_t>((size_t)cols * nr * sizeof(double2), 16));
    if (rows_out || sites_out || totals_out) {
        uint8_t* d = (uint8_t*)net.get(space_kept(nr, nm));
        space_table(nullptr, sc, d_v, rows, p, d, (uint8_t*)net.get(space_lists(sc)), nullptr);
        const size_t rb = sp_up(nr * sizeof(EagleSpaceRow)), sb = sp_up(nr * SP_CAP * sizeof(EagleSpaceSite));
        if (rows_out) HIP_CHECK(hipMemcpy(rows_out, d, nr * sizeof(EagleSpaceRow), hipMemcpyDeviceToHost));
        if (sites_out) HIP_CHECK(hipMemcpy(sites_out, d + rb, nr * SP_CAP * sizeof(EagleSpaceSite), hipMemcpyDeviceToHost));
        if (totals_out && nm) HIP_CHECK(hipMemcpy(totals_out, d + rb + sb, nm * sizeof(EagleSpaceTotals), hipMemcpyDeviceToHost));
    }
    if (maps) space_maps(nullptr, sc, d_v, rows, row0, n, p, grid, false, (uint8_t*)net.get(pl.total), pl, nullptr);
    API_END(hh)
}

}  // extern "C"
