// K28 — pass options: rows of a processed table resident in HBM (post.hip), their velocities and the possession result -> per row a grid of how well a
// pass from the ball to each pitch cell would do, the same figure for every teammate's own reaction point, and the best of those (include/eagle.h,
// eagle_pass_options_*; tests/options_ref.py is the written definition of every byte: fp32, no contraction, correctly rounded sqrt and division, d_expf of
// dmath.h).  Only minima cross sites, so no order of accumulation exists.
//
// Four launches per pass, no host round trip for the data:
//   options_sites_kernel    one thread per row (control_sites_kernel's shape): the row's status, the ball in fp32, the compacted reaction points of the
//                           attackers and, behind them, of the defenders (8 bytes per entry), the site index of every attacker, the counts, and the row
//                           record with best = -1 and sum = 0.
//   options_grid_kernel     control_kernel's shape: a workgroup owns PO_THREADS x PO_CELLS consecutive cells of one row's grid, a thread PO_CELLS of them in
//                           registers.  Both lists are staged in LDS once (at most EAGLE_PASS_MAX_SITES entries = 8 KB, so no chunking) and every lane reads
//                           the same entry (an LDS broadcast): one 8-byte read feeds PO_CELLS cells.  The loop order is SAMPLES OUTER: the K
//                           samples are a run-time count, so defenders-outer would keep PO_CELLS x (K - 1) running minima in registers for a K known at
//                           compile time only; samples-outer keeps PO_CELLS and re-reads the defender list K times from LDS, one 16-byte read per 44 VALU
//                           instructions.  A row that is not active (uniform per workgroup) writes zeros and leaves in front of the only barrier.
//   options_targets_kernel  one thread per (row, attacker) evaluates the same device function at the attacker's own reaction point, lists in HBM.
//   options_best_kernel     one thread per row: the largest option, a tie to the earlier column.
#include "runtime.h"
#include "dmath.h"

namespace eagle {

static constexpr int PO_THREADS = 256, PO_CELLS = 4;
static constexpr int PO_PASS = 65535;                         // gridDim.y limit
static constexpr float PO_QLIM = 1048576.0f, PO_FLT_MAX = 3.402823466e+38f;
static constexpr double PO_DOMAIN = 1024.0;
static constexpr int64_t PO_STAGING = (int64_t)32 << 20;      // device staging per pass
static_assert(sizeof(EaglePassOptionRow) == 40 && sizeof(EaglePassOptionParams) == 32, "include/eagle.h states these sizes");

struct PoCol { int32_t col, group; };                          // a site column of the table, in table order
struct PoHdr { int32_t status; float bx, by; int32_t nA, nD, pad[3]; };     // 32 bytes per row of a pass
struct PoArgs {
    const double2* values;       // the table and its velocities, [column][row]
    const double2* vel;
    const int32_t* cand;         // [rows] of the table
    const int32_t* owner;
    const PoCol* cols;           // [nsites]
    const int32_t* colsite;      // [tcols]: a table column's site index, -1: not a site column
    PoHdr* hdr;                  // [n]
    float2* lists;               // [n][stride]: the attackers' reaction points, then the defenders'
    int32_t* att;                // [n][stride]: the site index of every attacker
    uint8_t* grid;               // [n][gh][gw] or nullptr
    EaglePassOptionRow* rows_out;    // [n]
    int16_t* options;            // [n][nsites] (-1 in front of the launches)
    int rows, row0, n, nsites, stride, tcols, ball, R, gw, gh, K;
    float t_react, v_max, beta, v_ball;
};

__device__ __forceinline__ bool in_domain(double2 p) { return fabs(p.x) <= PO_DOMAIN && fabs(p.y) <= PO_DOMAIN; }       // false for NaN and +-inf

__device__ __forceinline__ float2 reaction_point(double2 p, double2 vd, float t_react)       // control_sites_kernel's q
{
    float vx = (float)vd.x, vy = (float)vd.y;
    if (!(fabsf(vx) <= PO_FLT_MAX)) vx = 0.0f;                                               // NaN, or beyond fp32
    if (!(fabsf(vy) <= PO_FLT_MAX)) vy = 0.0f;
    float qx = (float)p.x + vx * t_react, qy = (float)p.y + vy * t_react;
    qx = fminf(fmaxf(qx, -PO_QLIM), PO_QLIM);
    qy = fminf(fmaxf(qy, -PO_QLIM), PO_QLIM);
    return make_float2(qx, qy);
}

__global__ __launch_bounds__(256) void options_sites_kernel(PoArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const size_t row = (size_t)(a.row0 + i);
    const int o = a.owner[row], cd = a.cand[row];
    const int osite = (o >= 0 && o < a.tcols) ? a.colsite[o] : -1;
    const int g = osite >= 0 ? a.cols[osite].group : -1;
    double2 b = make_double2(0.0, 0.0);
    bool ball = false;
    if (a.ball >= 0) { b = a.values[(size_t)a.ball * a.rows + row]; ball = in_domain(b); }
    const int status = o < 0 ? EAGLE_PASS_NO_OWNER : cd != o ? EAGLE_PASS_IN_FLIGHT : osite < 0 ? EAGLE_PASS_NO_TEAM : !ball ? EAGLE_PASS_OFF_DOMAIN : EAGLE_PASS_ACTIVE;
    int nA = 0, nD = 0;
    if (status == EAGLE_PASS_ACTIVE) {
        float2* L = a.lists + (size_t)i * a.stride;
        int32_t* S = a.att + (size_t)i * a.stride;
        for (int side = 0; side < 2; ++side)                       // the attackers, then the defenders behind them
            for (int c = 0; c < a.nsites; ++c) {
                const PoCol d = a.cols[c];                          // (uniform)
                if ((d.group == g) != (side == 0) || d.col == o) continue;
                const double2 p = a.values[(size_t)d.col * a.rows + row];
                if (!in_domain(p)) continue;
                const float2 q = reaction_point(p, a.vel[(size_t)d.col * a.rows + row], a.t_react);
                L[nA + nD] = q;                                     // nA + nD <= nsites - 1 < stride
                if (side == 0) S[nA++] = c; else ++nD;
            }
    }
    PoHdr h{};
    h.status = status; h.bx = (float)b.x; h.by = (float)b.y; h.nA = nA; h.nD = nD;
    a.hdr[i] = h;
    EaglePassOptionRow r{};
    r.status = status; r.owner_col = o; r.group = g; r.n_mates = nA; r.n_defenders = nD; r.best_col = -1; r.best_byte = -1;
    a.rows_out[i] = r;
}

struct PoModel { int K; float fK, t_react, v_max, beta, v_ball; };

// With one target per thread the x and y halves of the arithmetic below are two independent scalar chains, which the compiler would pair into packed
// fp32 instructions (v_pk_add_f32, v_pk_mul_f32); the library holds none (Makefile, -fno-slp-vectorize; tests/test_isa_guard.py).  An empty statement
// the optimiser cannot look through keeps the x half on its own; with PO_CELLS targets nothing pairs, and nothing is added.
template <int C>
__device__ __forceinline__ float solo(float v)
{
    if constexpr (C == 1) asm volatile("" : "+v"(v));
    return v;
}

// The bytes of C targets of one row with at least one attacker: the one statement of the model, for the grid (C = PO_CELLS, lists in LDS) and for the
// attackers' own reaction points (C = 1, lists in HBM)
template <int C, typename P>
__device__ __forceinline__ void pass_bytes(const PoModel& m, float bx, float by, P A, int nA, P D, int nD, const float (&cx)[C], const float (&cy)[C], uint32_t (&out)[C])
{
    if (nD == 0) {                                                 // safety = reach = 1: floorf(255.5)
        #pragma unroll
        for (int c = 0; c < C; ++c) out[c] = 255u;
        return;
    }
    float dx[C], dy[C], len[C], lane[C];
    #pragma unroll
    for (int c = 0; c < C; ++c) {
        dx[c] = solo<C>(cx[c] - bx); dy[c] = cy[c] - by;
        len[c] = sqrtf(solo<C>(dx[c] * dx[c]) + dy[c] * dy[c]);
        lane[c] = PO_FLT_MAX;
    }
    for (int k = 1; k <= m.K; ++k) {
        const float f = (float)k / m.fK;
        float sx[C], sy[C], best[C];
        #pragma unroll
        for (int c = 0; c < C; ++c) { sx[c] = solo<C>(bx + solo<C>(dx[c] * f)); sy[c] = by + dy[c] * f; best[c] = PO_FLT_MAX; }
        for (int s = 0; s < nD; ++s) {
            const float2 e = D[s];                                 // (the grid: one address for the whole wave, an LDS broadcast)
            #pragma unroll
            for (int c = 0; c < C; ++c) {
                const float ex = solo<C>(sx[c] - e.x), ey = sy[c] - e.y;
                best[c] = fminf(best[c], solo<C>(ex * ex) + ey * ey);
            }
        }
        if (k < m.K) {
            #pragma unroll
            for (int c = 0; c < C; ++c) lane[c] = fminf(lane[c], (m.t_react + sqrtf(best[c]) / m.v_max) - (len[c] * f) / m.v_ball);
        } else {                                                   // the reception, at s_K as computed
            float mate[C];
            #pragma unroll
            for (int c = 0; c < C; ++c) mate[c] = PO_FLT_MAX;
            for (int s = 0; s < nA; ++s) {
                const float2 e = A[s];
                #pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float ex = solo<C>(sx[c] - e.x), ey = sy[c] - e.y;
                    mate[c] = fminf(mate[c], solo<C>(ex * ex) + ey * ey);
                }
            }
            #pragma unroll
            for (int c = 0; c < C; ++c) {
                const float tD = m.t_react + sqrtf(best[c]) / m.v_max, tA = m.t_react + sqrtf(mate[c]) / m.v_max;
                const float reach = 1.0f / (1.0f + d_expf(-(m.beta * (tD - tA))));
                const float safety = m.K == 1 ? 1.0f : 1.0f / (1.0f + d_expf(-(m.beta * lane[c])));
                out[c] = (uint32_t)(int)floorf(safety * reach * 255.0f + 0.5f);
            }
        }
    }
}

__device__ __forceinline__ PoModel model_of(const PoArgs& a) { return PoModel{a.K, (float)a.K, a.t_react, a.v_max, a.beta, a.v_ball}; }

__global__ __launch_bounds__(PO_THREADS) void options_grid_kernel(PoArgs a)
{
    __shared__ float2 s_q[EAGLE_PASS_MAX_SITES];
    const int f = blockIdx.y, tid = threadIdx.x;
    const int cells = a.gw * a.gh;                     // (a multiple of PO_CELLS: 7140 R^2)
    const int k0 = (blockIdx.x * PO_THREADS + tid) * PO_CELLS;
    const bool live = k0 < cells;
    const PoHdr h = a.hdr[f];                          // (uniform per workgroup)
    uint8_t* dst = a.grid + (size_t)f * cells + k0;
    if (h.status != EAGLE_PASS_ACTIVE || h.nA == 0) {  // zeros; the whole workgroup leaves here, in front of the barrier
        if (live) {
            if (((uintptr_t)dst & 3) == 0) *(uint32_t*)dst = 0u;
            else {
                #pragma unroll
                for (int c = 0; c < PO_CELLS; ++c) dst[c] = 0;
            }
        }
        return;
    }
    const int count = min(h.nA + h.nD, EAGLE_PASS_MAX_SITES);      // (the sites kernel writes at most nsites - 1 <= 1023)
    const float2* L = a.lists + (size_t)f * a.stride;
    for (int s = tid; s < count; s += PO_THREADS) s_q[s] = L[s];
    __syncthreads();
    const float fR = (float)a.R;
    float cx[PO_CELLS], cy[PO_CELLS];
    #pragma unroll
    for (int c = 0; c < PO_CELLS; ++c) {
        const int k = live ? k0 + c : 0, j = k / a.gw, i = k - j * a.gw;      // (an idle lane of the last workgroup works on cell 0 and stores nothing)
        cx[c] = ((float)i + 0.5f) / fR;                // (exact: R is 1, 2 or 4)
        cy[c] = ((float)j + 0.5f) / fR;
    }
    uint32_t b[PO_CELLS];
    pass_bytes<PO_CELLS>(model_of(a), h.bx, h.by, (const float2*)s_q, h.nA, (const float2*)s_q + h.nA, h.nD, cx, cy, b);
    uint32_t word = 0, sum = 0;
    #pragma unroll
    for (int c = 0; c < PO_CELLS; ++c) { word |= b[c] << (8 * c); sum += b[c]; }
    if (live) {
        if (((uintptr_t)dst & 3) == 0) *(uint32_t*)dst = word;
        else {
            #pragma unroll
            for (int c = 0; c < PO_CELLS; ++c) dst[c] = (uint8_t)(word >> (8 * c));
        }
    } else sum = 0;
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((tid & 63) == 0 && sum) atomicAdd((unsigned long long*)&a.rows_out[f].sum, (unsigned long long)sum);
}

__global__ __launch_bounds__(256) void options_targets_kernel(PoArgs a)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)a.n * a.stride) return;
    const int f = (int)(t / a.stride), j = (int)(t - (long long)f * a.stride);
    const PoHdr h = a.hdr[f];
    if (h.status != EAGLE_PASS_ACTIVE || j >= h.nA) return;
    const float2* L = a.lists + (size_t)f * a.stride;
    const float2 q = L[j];
    const float cx[1] = {q.x}, cy[1] = {q.y};
    uint32_t b[1];
    pass_bytes<1>(model_of(a), h.bx, h.by, L, h.nA, L + h.nA, h.nD, cx, cy, b);
    a.options[(size_t)f * a.nsites + a.att[(size_t)f * a.stride + j]] = (int16_t)b[0];
}

__global__ __launch_bounds__(256) void options_best_kernel(PoArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int16_t* o = a.options + (size_t)i * a.nsites;
    int best = -1, at = -1;
    for (int s = 0; s < a.nsites; ++s) {
        const int v = o[s];
        if (v > best) { best = v; at = s; }                         // a tie keeps the earlier column
    }
    if (at >= 0) { a.rows_out[i].best_col = a.cols[at].col; a.rows_out[i].best_byte = best; }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------
static void options_check(const EaglePassOptionParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "pass options: params is NULL");
    if (p->samples < 1 || p->samples > 64) fail(EAGLE_E_INVALID, "pass options: samples %d must lie within 1 .. 64", p->samples);
    if (!(p->v_ball >= 1e-3f && p->v_ball <= 1e6f)) fail(EAGLE_E_INVALID, "pass options: v_ball %g must be positive (0.001 .. 1e6 m/s)", (double)p->v_ball);
    EagleControlParams c{};
    c.cells_per_metre = p->cells_per_metre; c.t_react = p->t_react; c.v_max = p->v_max; c.beta = p->beta;
    control_check(&c);                                             // (the shared fields answer to control's one check)
}

struct PoCols { std::vector<PoCol> sites; std::vector<int32_t> colsite; int ball = -1; };

static PoCols options_columns(const EaglePostColumn* columns, int ncols, bool no_ball, const int32_t* team_ids, const int32_t* team_vals, size_t n_team)
{
    PoCols pc;
    pc.colsite.assign(std::max(ncols, 1), -1);
    for (int c = 0; c < ncols; ++c) {
        const EaglePostColumn& col = columns[c];
        if (col.kind != EAGLE_POST_PLAYER && col.kind != EAGLE_POST_GOALKEEPER && col.kind != EAGLE_POST_BALL && col.kind != EAGLE_POST_BOUNDARY)
            fail(EAGLE_E_INVALID, "pass options: column %d is of unknown kind %d", c, col.kind);
        if (col.video) continue;
        if (col.kind == EAGLE_POST_BALL) {
            if (pc.ball >= 0) fail(EAGLE_E_INVALID, "pass options: columns %d and %d are both the ball", pc.ball, c);
            pc.ball = c;
        } else if (col.kind == EAGLE_POST_PLAYER) {
            size_t k = 0;
            while (k < n_team && team_ids[k] != col.id) ++k;       // the first entry counts, as in possession and shape
            if (k == n_team || team_vals[k] < 0) continue;
            pc.colsite[c] = (int32_t)pc.sites.size();
            pc.sites.push_back(PoCol{c, team_vals[k] == 0 ? 0 : 1});
        }
    }
    if (pc.sites.size() > (size_t)EAGLE_PASS_MAX_SITES)
        fail(EAGLE_E_INVALID, "pass options: %zu site columns, at most %d are supported", pc.sites.size(), EAGLE_PASS_MAX_SITES);
    if (no_ball) pc.ball = -1;
    return pc;
}

static void options_window(int rows, int row0, int n)
{
    if (n < 0) fail(EAGLE_E_INVALID, "pass options: n = %d is negative", n);
    if (n > 0 && rows == 0) fail(EAGLE_E_INVALID, "pass options: the table has no rows");
    if (row0 < 0 || row0 > rows || n > rows - row0) fail(EAGLE_E_INVALID, "pass options: rows %d .. %d lie outside the table's %d rows", row0, row0 + n - 1, rows);
}

static size_t up256(size_t b) { return (std::max<size_t>(b, 16) + 255) & ~(size_t)255; }

// The device memory of one call behind a single base: the site columns, the per-row lists of a pass and, where the caller's memory is not on the device
// or absent, the outputs of a pass
struct PoPlan { int pass; size_t cols, colsite, hdr, lists, att, options, rows, grid, total; };

static PoPlan options_plan(const PoCols& pc, int tcols, int n, size_t cells, bool own_options, bool own_rows, bool own_grid)
{
    const size_t ns = pc.sites.size(), stride = std::max<size_t>(ns, 1);
    const size_t per_row = sizeof(PoHdr) + stride * 12 + (own_options ? ns * 2 : 0) + (own_rows ? sizeof(EaglePassOptionRow) : 0) + (own_grid ? cells : 0);
    PoPlan o{};
    o.pass = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(n, PO_PASS), PO_STAGING / (int64_t)per_row));
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += up256(b); return was; };
    o.cols = take(ns * sizeof(PoCol)); o.colsite = take((size_t)std::max(tcols, 1) * 4);
    o.hdr = take((size_t)o.pass * sizeof(PoHdr)); o.lists = take((size_t)o.pass * stride * 8); o.att = take((size_t)o.pass * stride * 4);
    o.options = take(own_options ? (size_t)o.pass * ns * 2 : 0); o.rows = take(own_rows ? (size_t)o.pass * sizeof(EaglePassOptionRow) : 0);
    o.grid = take(own_grid ? (size_t)o.pass * cells : 0);
    o.total = at;
    return o;
}

static PoArgs options_args(const EaglePassOptionParams* p, const PoCols& pc, int rows, int tcols, uint8_t* base, const PoPlan& pl, hipStream_t s)
{
    PoArgs a{};
    a.R = p->cells_per_metre; a.gw = 105 * a.R; a.gh = 68 * a.R; a.K = p->samples;
    a.t_react = p->t_react; a.v_max = p->v_max; a.beta = p->beta; a.v_ball = p->v_ball;
    a.rows = rows; a.tcols = tcols; a.ball = pc.ball; a.nsites = (int)pc.sites.size(); a.stride = std::max(a.nsites, 1);
    if (!pc.sites.empty()) HIP_CHECK(hipMemcpyAsync(base + pl.cols, pc.sites.data(), pc.sites.size() * sizeof(PoCol), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(base + pl.colsite, pc.colsite.data(), pc.colsite.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));                            // (pageable sources: they have left the vectors)
    a.cols = (const PoCol*)(base + pl.cols); a.colsite = (const int32_t*)(base + pl.colsite);
    a.hdr = (PoHdr*)(base + pl.hdr); a.lists = (float2*)(base + pl.lists); a.att = (int32_t*)(base + pl.att);
    return a;
}

// The launches of a.n <= PO_PASS rows on s (h: timed under its profiling mode, or nullptr); enqueued, not awaited
static void options_launch(EagleHandle* h, const PoArgs& a, hipStream_t s)
{
    const int cells = a.gw * a.gh, per = PO_THREADS * PO_CELLS;
    auto run = [&](const char* name, double bytes, const std::function<void()>& fn) {
        if (h) timed_launch(h, name, bytes, s, fn); else fn();
    };
    // bytes: the cells of the sites read (twice: the two sides), the lists and records written; the grids written; the lists read, the options written
    run("options_sites", (double)a.n * (64.0 * a.nsites + 12.0 * a.stride + 72.0 + 16.0), [&] {
        if (a.nsites) HIP_CHECK(hipMemsetAsync(a.options, 0xff, (size_t)a.n * a.nsites * 2, s));
        hipLaunchKernelGGL(options_sites_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
        HIP_CHECK(hipGetLastError());
    });
    if (a.grid) run("options_grid", (double)a.n * ((double)cells + 8.0 * a.stride), [&] {
        hipLaunchKernelGGL(options_grid_kernel, dim3((cells + per - 1) / per, a.n), dim3(PO_THREADS), 0, s, a);
        HIP_CHECK(hipGetLastError());
    });
    run("options_targets", (double)a.n * (12.0 * a.stride + 2.0 * a.nsites + 40.0), [&] {
        const long long threads = (long long)a.n * a.stride;
        hipLaunchKernelGGL(options_targets_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(options_best_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
        HIP_CHECK(hipGetLastError());
    });
}

static void options_budget(const PoPlan& pl, int64_t max_bytes)
{
    double budget = (double)max_bytes;
    if (max_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = 0.9 * (double)free_b;
    }
    if ((double)pl.total > budget)
        fail(EAGLE_E_INVALID, "pass options: a pass of %d rows needs %.0f bytes of device memory, the budget is %.0f", pl.pass, (double)pl.total, budget);
}

// A handle entry: rows row0 .. row0 + n - 1 in passes; device: the three outputs are device memory (grid and options may be nullptr), else host memory
static void options_rows(EagleHandle* h, EaglePostTable* t, int row0, int n, const EaglePassOptionParams* p, uint8_t* grid, EaglePassOptionRow* rows_out, int16_t* options,
                         bool device)
{
    if (!t || !rows_out) fail(EAGLE_E_INVALID, "pass options: bad argument (table %p, rows %p)", (const void*)t, (const void*)rows_out);
    if (t->h != h) fail(EAGLE_E_INVALID, "pass options: the table belongs to another handle");
    options_check(p);
    if (!t->has_team) fail(EAGLE_E_INVALID, "pass options: the table has no team mapping (attackers and defenders are told apart by it)");
    if (!t->d_vel) fail(EAGLE_E_INVALID, "pass options: the table has no velocities (eagle_post_velocities comes first)");
    if (!t->has_poss) fail(EAGLE_E_INVALID, "pass options: the table has no possession result (eagle_post_possession comes first)");
    options_window(t->rows, row0, n);
    const PoCols pc = options_columns(t->columns.data(), t->cols, (t->flags & EAGLE_POST_NO_BALL) != 0, t->team_ids.data(), t->team_vals.data(), t->team_ids.size());
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t cells = (size_t)7140 * p->cells_per_metre * p->cells_per_metre, ns = pc.sites.size();
    const PoPlan pl = options_plan(pc, t->cols, n, cells, !device || !options, !device, !device && grid);
    options_budget(pl, t->max_bytes);
    const hipStream_t s = h->s_main;
    uint8_t* base = nullptr;
    HIP_CHECK(hipMalloc((void**)&base, pl.total));
    try {
        PoArgs a = options_args(p, pc, t->rows, t->cols, base, pl, s);
        a.values = (const double2*)t->d_values; a.vel = (const double2*)t->d_vel;
        a.cand = (const int32_t*)((const double*)t->d_poss + t->rows); a.owner = a.cand + t->rows;
        for (int i = 0; i < n; i += pl.pass) {
            a.n = std::min(pl.pass, n - i); a.row0 = row0 + i;
            if (device) {
                a.grid = grid ? grid + (size_t)i * cells : nullptr; a.rows_out = rows_out + i;
                a.options = options ? options + (size_t)i * ns : (int16_t*)(base + pl.options);
            } else {
                a.grid = grid ? base + pl.grid : nullptr; a.rows_out = (EaglePassOptionRow*)(base + pl.rows); a.options = (int16_t*)(base + pl.options);
            }
            options_launch(h, a, s);
            if (!device) {
                if (grid) HIP_CHECK(hipMemcpyAsync(grid + (size_t)i * cells, a.grid, (size_t)a.n * cells, hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipMemcpyAsync(rows_out + i, a.rows_out, (size_t)a.n * sizeof(EaglePassOptionRow), hipMemcpyDeviceToHost, s));
                if (options && ns) HIP_CHECK(hipMemcpyAsync(options + (size_t)i * ns, a.options, (size_t)a.n * ns * 2, hipMemcpyDeviceToHost, s));
            }
            HIP_CHECK(hipStreamSynchronize(s));                    // (the next pass reuses the lists)
            if (h->prof) collect_spans(h);
        }
    } catch (...) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(base);
        throw;
    }
    HIP_CHECK(hipFree(base));
}

}  // namespace eagle

extern "C" {

int eagle_pass_options_size(const EaglePassOptionParams* p, int* gw, int* gh)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!gw || !gh) fail(EAGLE_E_INVALID, "eagle_pass_options_size: gw or gh is NULL");
    options_check(p);
    *gw = 105 * p->cells_per_metre; *gh = 68 * p->cells_per_metre;
    API_END(hh)
}

int eagle_pass_options_layout(const EaglePostTable* t, int32_t* site_cols, int cap, int* n_sites)
{
    if (!t || !n_sites || cap < 0 || (cap > 0 && !site_cols)) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->has_team) fail(EAGLE_E_INVALID, "pass options: the table has no team mapping (attackers and defenders are told apart by it)");
    const PoCols pc = options_columns(t->columns.data(), t->cols, false, t->team_ids.data(), t->team_vals.data(), t->team_ids.size());
    *n_sites = (int)pc.sites.size();
    for (size_t i = 0; i < std::min<size_t>(cap, pc.sites.size()); ++i) site_cols[i] = pc.sites[i].col;
    API_END(h)
}

int eagle_pass_options_device(EagleHandle* h, EaglePostTable* t, int row0, int n, const EaglePassOptionParams* p, uint8_t* d_grid, EaglePassOptionRow* d_rows,
                              int16_t* d_options)
{
    API_BEGIN_H(h)
    options_rows(h, t, row0, n, p, d_grid, d_rows, d_options, true);
    API_END(h)
}

int eagle_pass_options(EagleHandle* h, EaglePostTable* t, int row0, int n, const EaglePassOptionParams* p, uint8_t* grid, EaglePassOptionRow* rows_out, int16_t* options)
{
    API_BEGIN_H(h)
    options_rows(h, t, row0, n, p, grid, rows_out, options, false);
    API_END(h)
}

int eagle_op_pass_options(int device, const double* values, const double* velocities, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                          const int32_t* team_vals, int n_team, const int32_t* cand, const int32_t* owner, const EaglePassOptionParams* p, int row0, int n,
                          uint8_t* grid, EaglePassOptionRow* rows_out, int16_t* options)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !columns || !cand || !owner || !rows_out || rows < 0 || cols < 0 || n_team < 0 || (team_ids && n_team > 0 && !team_vals))
        fail(EAGLE_E_INVALID, "eagle_op_pass_options: bad argument (values %p, columns %p, cand %p, owner %p, rows_out %p, %d rows, %d columns, %d teams)",
             (const void*)values, (const void*)columns, (const void*)cand, (const void*)owner, (const void*)rows_out, rows, cols, n_team);
    options_check(p);
    if (!team_ids) fail(EAGLE_E_INVALID, "pass options: the table has no team mapping (attackers and defenders are told apart by it)");
    if (!velocities) fail(EAGLE_E_INVALID, "pass options: the table has no velocities (eagle_op_velocities comes first)");
    options_window(rows, row0, n);
    const PoCols pc = options_columns(columns, cols, false, team_ids, team_vals, (size_t)n_team);
    for (int r = 0; r < rows; ++r)
        if (cand[r] < -1 || cand[r] >= cols || owner[r] < -1 || owner[r] >= cols)
            fail(EAGLE_E_INVALID, "eagle_op_pass_options: row %d: cand %d and owner %d must be -1 or a column index below %d", r, cand[r], owner[r], cols);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    const size_t cells = (size_t)7140 * p->cells_per_metre * p->cells_per_metre, ns = pc.sites.size(), tb = (size_t)cols * rows * sizeof(double2);
    const PoPlan pl = options_plan(pc, cols, n, cells, true, true, grid != nullptr);
    options_budget(pl, 0);
    Net net;
    uint8_t* base = (uint8_t*)net.get(pl.total);
    PoArgs a = options_args(p, pc, rows, cols, base, pl, nullptr);
    a.values = (const double2*)net.upload(values, tb);
    a.vel = (const double2*)net.upload(velocities, tb);
    a.cand = (const int32_t*)net.upload(cand, (size_t)rows * 4);
    a.owner = (const int32_t*)net.upload(owner, (size_t)rows * 4);
    a.grid = grid ? base + pl.grid : nullptr; a.rows_out = (EaglePassOptionRow*)(base + pl.rows); a.options = (int16_t*)(base + pl.options);
    for (int i = 0; i < n; i += pl.pass) {
        a.n = std::min(pl.pass, n - i); a.row0 = row0 + i;
        options_launch(nullptr, a, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        if (grid) HIP_CHECK(hipMemcpy(grid + (size_t)i * cells, a.grid, (size_t)a.n * cells, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(rows_out + i, a.rows_out, (size_t)a.n * sizeof(EaglePassOptionRow), hipMemcpyDeviceToHost));
        if (options && ns) HIP_CHECK(hipMemcpy(options + (size_t)i * ns, a.options, (size_t)a.n * ns * 2, hipMemcpyDeviceToHost));
    }
    API_END(hh)
}

}  // extern "C"
