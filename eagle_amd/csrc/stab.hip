// K38 — stabilisation: the common motion of a frame, the small translation, stretch and shear of the pitch plane that a slightly wrong homography gives
// every player and the ball at once, is estimated per row of a processed table from what the persons' own paths predict, and removed (include/eagle.h,
// eagle_post_stabilise / eagle_op_stabilise; tests/stab_ref.py is the written definition of every bit: integer sums and decisions, float64 without
// contraction, correctly rounded division, llrint to even).
//
// One launch in front, three per round, one behind, on one stream:
//   stab_quantise_kernel  every cell of a moved column once: presence byte, q = rint(x * 1024) as int32 pairs, C = q.  (q is read again by the estimate and
//                         the apply kernel of every round; the predict kernel's tile is filled from C, which IS q in the first round.)
//   stab_predict_kernel   smooth_fit_kernel's tile: 256 rows of one voter column per workgroup plus a halo of W rows each side in LDS (C, the frame number, a
//                         presence byte).  One thread owns one row, walks its window from LDS leaving out its own sample, forms the eleven int64 sums,
//                         solves by Cramer's rule in float64 (K37's solve, restated here: smooth.hip stays as it is) and writes the vote d = q - llrint(a0)
//                         and a vote byte.
//   stab_estimate_kernel  (stab_estimate.inc) one wave per row.  The row's voters are compacted in column order into the wave's LDS slots (ballot + prefix
//                         count); a lane owns a voter; the two medians and the deviation median are found by rank counting (#{< v} <= rank < #{<= v});
//                         the integer sums by a butterfly; every lane solves, lane 0 writes the row record.  A lane reads the cell of its column, so the
//                         wave's reads are strided by the row count; the form that transposes a block of rows through LDS first measured 8 % slower
//                         (docs/experiments.md, "Stabilisation (K38)") and lives in tools/stab_rate.py only.
//   stab_apply_kernel     per cell of the moved columns: C = q - T(q) (C = q in a row without an estimate); in the last round the table's value C / 1024.
//   stab_totals_kernel    the clip totals over the row records: a butterfly per wave, integer atomics per wave: no order of arrival can show.
#include "runtime.h"

static_assert(sizeof(EagleStabParams) == 80 && sizeof(EagleStabRow) == 104 && sizeof(EagleStabTotals) == 80, "include/eagle.h states these sizes");

namespace eagle {

static constexpr int ST_TILE = 256;            // rows of a column per workgroup of the predict kernel, one thread each
static constexpr int ST_WMAX = 64;             // the largest half-width
static constexpr int ST_LDS = ST_TILE + 2 * ST_WMAX;
static constexpr double ST_Q = 1024.0, ST_LIMIT = 1024.0;
static constexpr long long ST_VOTE_CAP = 1 << 24;

#include "stab_estimate.inc"                   // StabArgs, the estimate of a row by a wave, stab_estimate_kernel

__device__ __forceinline__ bool st_present(double2 v) { return fabs(v.x) <= ST_LIMIT && fabs(v.y) <= ST_LIMIT; }     // false for NaN and +-inf

__global__ __launch_bounds__(ST_TILE) void stab_quantise_kernel(StabArgs a)
{
    const int r = blockIdx.x * ST_TILE + threadIdx.x;
    if (r >= a.rows) return;
    for (int c = blockIdx.y; c < a.cols; c += gridDim.y) {
        if (!a.kind[c]) continue;
        const size_t at = (size_t)c * a.rows + r;
        const double2 v = a.values[at];
        int2 q = make_int2(0, 0);
        const bool ok = st_present(v);
        if (ok) q = make_int2((int)rint(v.x * ST_Q), (int)rint(v.y * ST_Q));
        a.q[at] = q; a.C[at] = q; a.present[at] = ok;
    }
}

// K37's solve (csrc/smooth.hip sm_solve), a0 only
__device__ __forceinline__ double st_a0(const double* S, const double* B, int deg)
{
    if (deg == 2) {
        const double C00 = S[2] * S[4] - S[3] * S[3];
        const double C01 = S[2] * S[3] - S[1] * S[4];
        const double C02 = S[1] * S[3] - S[2] * S[2];
        const double det = (S[0] * C00 + S[1] * C01) + S[2] * C02;
        return ((C00 * B[0] + C01 * B[1]) + C02 * B[2]) / det;
    }
    const double det = S[0] * S[2] - S[1] * S[1];
    return (S[2] * B[0] - S[1] * B[1]) / det;
}

struct StTile {
    int cx[ST_LDS], cy[ST_LDS], f[ST_LDS];
    uint8_t used[ST_LDS];
};

__global__ __launch_bounds__(ST_TILE) void stab_predict_kernel(StabArgs a)
{
    __shared__ StTile t;
    const int r0 = blockIdx.x * ST_TILE, r = r0 + threadIdx.x, W = a.W;
    for (int c = blockIdx.y; c < a.cols; c += gridDim.y) {
        if (a.kind[c] != 3) continue;                           // uniform over the workgroup
        for (int i = threadIdx.x; i < ST_TILE + 2 * W; i += ST_TILE) {          // rows r0 - W .. r0 + ST_TILE + W - 1 -> slot 0 ..; a row outside the table is not used
            const int rr = r0 - W + i;
            int2 v = make_int2(0, 0);
            int f = 0;
            uint8_t u = 0;
            if (rr >= 0 && rr < a.rows) {
                const size_t at = (size_t)c * a.rows + rr;
                u = a.present[at];
                if (u) v = a.C[at];
                f = a.frames[rr];
            }
            t.cx[i] = v.x; t.cy[i] = v.y; t.f[i] = f; t.used[i] = u;
        }
        __syncthreads();
        const int me = threadIdx.x + W;
        if (r < a.rows) {
            const size_t at = (size_t)c * a.rows + r;
            int2 d = make_int2(0, 0);
            uint8_t vote = 0;
            if (t.used[me]) {
                long long S0 = 0, S1 = 0, S2 = 0, S3 = 0, S4 = 0, X0 = 0, X1 = 0, X2 = 0, Y0 = 0, Y1 = 0, Y2 = 0;
                const int fr = t.f[me];
                bool before = false, after = false;
                for (int j = me - W; j <= me + W; ++j) {
                    if (j == me || !t.used[j]) continue;
                    const long long dt = (long long)t.f[j] - fr;
                    if (dt < -W || dt > W) continue;
                    before |= j < me; after |= j > me;
                    const long long d2 = dt * dt, x = t.cx[j], y = t.cy[j];
                    S0 += 1; S1 += dt; S2 += d2; S3 += d2 * dt; S4 += d2 * d2;
                    X0 += x; X1 += dt * x; X2 += d2 * x;
                    Y0 += y; Y1 += dt * y; Y2 += d2 * y;
                }
                if (before && after && S0 >= 2) {
                    const int deg = S0 >= 4 ? a.degree : 1;     // n == 3: min(degree, 1); n == 2: 1
                    const double S[5] = {(double)S0, (double)S1, (double)S2, (double)S3, (double)S4};
                    const double X[3] = {(double)X0, (double)X1, (double)X2}, Y[3] = {(double)Y0, (double)Y1, (double)Y2};
                    const double ax = st_a0(S, X, deg), ay = st_a0(S, Y, deg);
                    if (fabs(ax) <= ST_A0_CAP && fabs(ay) <= ST_A0_CAP) {
                        const int2 q = a.q[at];
                        const long long dx = (long long)q.x - llrint(ax), dy = (long long)q.y - llrint(ay);
                        if (dx >= -ST_VOTE_CAP && dx <= ST_VOTE_CAP && dy >= -ST_VOTE_CAP && dy <= ST_VOTE_CAP) { d = make_int2((int)dx, (int)dy); vote = 1; }
                    }
                }
            }
            a.votes[at] = d; a.voteb[at] = vote;
        }
        __syncthreads();                                        // the tile is rewritten for the next column
    }
}

__global__ __launch_bounds__(ST_TILE) void stab_apply_kernel(StabArgs a)
{
    const int r = blockIdx.x * ST_TILE + threadIdx.x;
    if (r >= a.rows) return;
    const EagleStabRow* e = a.rec + r;
    const int model = e->model;
    const int sx = e->shift_q[0], sy = e->shift_q[1], cx = e->centre_q[0], cy = e->centre_q[1];
    const double ox = e->offset[0], oy = e->offset[1], gain[4] = {e->gain[0], e->gain[1], e->gain[2], e->gain[3]};
    for (int c = blockIdx.y; c < a.cols; c += gridDim.y) {
        if (!a.kind[c]) continue;
        const size_t at = (size_t)c * a.rows + r;
        if (!a.present[at]) continue;
        int2 q = a.q[at];
        if (model) {
            const int2 t = st_map(model, sx, sy, cx, cy, ox, oy, gain, q);
            q.x -= t.x; q.y -= t.y;
            if (a.last) a.out[at] = make_double2((double)q.x / ST_Q, (double)q.y / ST_Q);
        }
        a.C[at] = q;
    }
}

__global__ __launch_bounds__(ST_TILE) void stab_totals_kernel(StabArgs a)
{
    const int r = blockIdx.x * ST_TILE + threadIdx.x;
    const bool in = r < a.rows;
    EagleStabRow e{};
    if (in) e = a.rec[r];
    const int fl = e.flags;
    const long long ssb = st_wave_sum(e.ss_before), ssa = st_wave_sum(e.ss_after), inl = st_wave_sum(e.inliers), moved = st_wave_sum(e.moved);
    const int none = (int)st_wave_sum(in && e.model == 0), tr = (int)st_wave_sum(e.model == 1), af = (int)st_wave_sum(e.model == 2);
    const int few = (int)st_wave_sum((fl >> 1) & 1), spread = (int)st_wave_sum((fl >> 2) & 1), corr = (int)st_wave_sum((fl >> 3) & 1), gain = (int)st_wave_sum((fl >> 4) & 1);
    const int jumps = (int)st_wave_sum((fl >> 5) & 1), over = (int)st_wave_sum(fl & 1);
    if ((threadIdx.x & 63) == 0) {
        EagleStabTotals* T = a.totals;
        if (ssb) atomicAdd((unsigned long long*)&T->ss_before, (unsigned long long)ssb);
        if (ssa) atomicAdd((unsigned long long*)&T->ss_after, (unsigned long long)ssa);
        if (inl) atomicAdd((unsigned long long*)&T->inliers, (unsigned long long)inl);
        if (moved) atomicAdd((unsigned long long*)&T->moved, (unsigned long long)moved);
        if (none) atomicAdd(&T->none, none);
        if (tr) atomicAdd(&T->translation, tr);
        if (af) atomicAdd(&T->affine, af);
        if (few) atomicAdd(&T->few_inliers, few);
        if (spread) atomicAdd(&T->low_spread, spread);
        if (corr) atomicAdd(&T->correlated, corr);
        if (gain) atomicAdd(&T->high_gain, gain);
        if (jumps) atomicAdd(&T->jumps, jumps);
        if (over) atomicAdd(&T->over_cap, over);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void stab_check(const char* who, const EagleStabParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: params is NULL", who);
    auto fin = [](double v) { return std::isfinite(v); };
    if (p->fps <= 0) fail(EAGLE_E_INVALID, "%s: fps %d must be positive", who, p->fps);
    if (p->window < 1 || p->window > ST_WMAX) fail(EAGLE_E_INVALID, "%s: window %d is outside 1 .. %d", who, p->window, ST_WMAX);
    if (p->degree != 1 && p->degree != 2) fail(EAGLE_E_INVALID, "%s: degree %d is neither 1 nor 2", who, p->degree);
    if (p->model != 0 && p->model != 1) fail(EAGLE_E_INVALID, "%s: model %d is neither 0 (translation) nor 1 (affine)", who, p->model);
    if (p->min_voters < 3 || p->min_voters > ST_VOTERS) fail(EAGLE_E_INVALID, "%s: min_voters %d is outside 3 .. %d", who, p->min_voters, ST_VOTERS);
    if (p->iterations < 1 || p->iterations > 4) fail(EAGLE_E_INVALID, "%s: iterations %d is outside 1 .. 4", who, p->iterations);
    if (!fin(p->trim_k) || !(p->trim_k == 0.0 || (p->trim_k >= 1.0 && p->trim_k <= 1000.0)))
        fail(EAGLE_E_INVALID, "%s: trim_k %g must be 0 (no trimming) or lie in 1 .. 1000", who, p->trim_k);
    if (!fin(p->floor) || p->floor < 0.0 || p->floor > 1024.0) fail(EAGLE_E_INVALID, "%s: floor %g must lie in 0 .. 1024", who, p->floor);
    if (!fin(p->min_spread) || !(p->min_spread > 0.0) || p->min_spread > 1024.0) fail(EAGLE_E_INVALID, "%s: min_spread %g must be positive and at most 1024", who, p->min_spread);
    if (!fin(p->max_gain) || !(p->max_gain > 0.0) || p->max_gain > 1.0) fail(EAGLE_E_INVALID, "%s: max_gain %g must be positive and at most 1", who, p->max_gain);
    if (!fin(p->jump) || !(p->jump > 0.0)) fail(EAGLE_E_INVALID, "%s: jump %g must be positive and finite", who, p->jump);
}

static void stab_columns(const char* who, const EaglePostColumn* columns, int ncols, std::vector<uint8_t>& kind)
{
    kind.assign((size_t)ncols, 0);
    for (int c = 0; c < ncols; ++c) {
        const EaglePostColumn& col = columns[c];
        if (col.kind != EAGLE_POST_PLAYER && col.kind != EAGLE_POST_GOALKEEPER && col.kind != EAGLE_POST_BALL && col.kind != EAGLE_POST_BOUNDARY)
            fail(EAGLE_E_INVALID, "%s: column %d is of unknown kind %d", who, c, col.kind);
        if (col.video) continue;
        if (col.kind == EAGLE_POST_PLAYER || col.kind == EAGLE_POST_GOALKEEPER) kind[c] = 3;
        else if (col.kind == EAGLE_POST_BALL) kind[c] = 1;
    }
}

static size_t st_up(size_t b) { return (std::max<size_t>(b, 16) + 255) & ~(size_t)255; }

// What a call keeps: EagleStabRow [rows] | votes i32 [cols][rows][2] | EagleStabTotals, each from a 256-byte boundary
struct StabKept { size_t rec, votes, totals, total; };

static StabKept stab_kept(size_t rows, size_t cols)
{
    StabKept o{};
    o.rec = 0;
    o.votes = st_up(rows * sizeof(EagleStabRow));
    o.totals = o.votes + st_up(rows * cols * 8);
    o.total = o.totals + st_up(sizeof(EagleStabTotals));
    return o;
}

static size_t stab_scratch(size_t rows, size_t cols) { return 2 * st_up(rows * cols * 8) + 2 * st_up(rows * cols) + st_up(cols); }

// d_values: the table as it was; d_out: a copy of it (the moved cells are overwritten); kept: stab_kept's block.  Returns when everything is complete.
static void stab_run(EagleHandle* h, const double2* d_values, const int32_t* d_frames, const std::vector<uint8_t>& kind, int rows, int cols, const EagleStabParams* p,
                     double2* d_out, uint8_t* kept, EagleStabTotals& totals_out, hipStream_t s)
{
    totals_out = EagleStabTotals{};
    totals_out.rows = rows; totals_out.iterations = p->iterations; totals_out.window = p->window;
    if (rows <= 0 || cols <= 0) { totals_out.none = std::max(rows, 0); return; }       // rows without a column have no estimate
    const StabKept L = stab_kept((size_t)rows, (size_t)cols);
    const size_t cells = (size_t)rows * cols;
    uint8_t* base = nullptr;
    HIP_CHECK(hipMalloc((void**)&base, stab_scratch((size_t)rows, (size_t)cols)));
    try {
        StabArgs a{};
        a.values = d_values; a.frames = d_frames; a.rows = rows; a.cols = cols; a.W = p->window; a.degree = p->degree; a.model = p->model; a.min_voters = p->min_voters;
        a.trim_k = p->trim_k; a.floor_q = p->floor * ST_Q; a.max_gain = p->max_gain; a.jump_q = p->jump * ST_Q;
        const double smin = p->min_spread * ST_Q;
        a.lim_s = smin * smin;
        a.q = (int2*)base; a.C = (int2*)(base + st_up(cells * 8));
        a.present = base + 2 * st_up(cells * 8); a.voteb = a.present + st_up(cells);
        uint8_t* d_kind = a.voteb + st_up(cells);
        a.kind = d_kind;
        a.rec = (EagleStabRow*)(kept + L.rec); a.votes = (int2*)(kept + L.votes); a.totals = (EagleStabTotals*)(kept + L.totals);
        a.out = d_out;
        HIP_CHECK(hipMemcpyAsync(d_kind, kind.data(), (size_t)cols, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(kept, 0, L.total, s));
        HIP_CHECK(hipMemsetAsync(a.present, 0, 2 * st_up(cells), s));                 // present and vote bytes of the columns no kernel writes
        const dim3 grid((unsigned)((rows + ST_TILE - 1) / ST_TILE), (unsigned)std::min(cols, 65535));
        const dim3 grid_rows((unsigned)((rows + ST_TILE - 1) / ST_TILE));
        size_t nm = 0, nv = 0;
        for (int c = 0; c < cols; ++c) { nm += kind[c] != 0; nv += kind[c] == 3; }
        const double mc = (double)nm * rows, vc = (double)nv * rows;
        auto run = [&](const char* name, double bytes, const std::function<void()>& fn) {
            if (h) timed_launch(h, name, bytes, s, fn); else fn();
        };
        run("stab_quantise", 33.0 * mc, [&] { hipLaunchKernelGGL(stab_quantise_kernel, grid, dim3(ST_TILE), 0, s, a); HIP_CHECK(hipGetLastError()); });
        for (int it = 0; it < p->iterations; ++it) {
            a.last = it + 1 == p->iterations;
            run("stab_predict", 26.0 * vc, [&] { hipLaunchKernelGGL(stab_predict_kernel, grid, dim3(ST_TILE), 0, s, a); HIP_CHECK(hipGetLastError()); });
            run("stab_estimate", 10.0 * vc + 104.0 * rows, [&] {
                hipLaunchKernelGGL(stab_estimate_kernel, dim3((unsigned)((rows + ST_WAVES - 1) / ST_WAVES)), dim3(ST_WAVES * 64), 0, s, a);
                HIP_CHECK(hipGetLastError());
            });
            run("stab_apply", (a.last ? 33.0 : 17.0) * mc, [&] { hipLaunchKernelGGL(stab_apply_kernel, grid, dim3(ST_TILE), 0, s, a); HIP_CHECK(hipGetLastError()); });
        }
        run("stab_totals", 104.0 * rows, [&] { hipLaunchKernelGGL(stab_totals_kernel, grid_rows, dim3(ST_TILE), 0, s, a); HIP_CHECK(hipGetLastError()); });
        EagleStabTotals got{};
        HIP_CHECK(hipMemcpyAsync(&got, a.totals, sizeof got, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h && h->prof) collect_spans(h);
        got.rows = rows; got.iterations = p->iterations; got.window = p->window;
        totals_out = got;
    } catch (...) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(base);
        throw;
    }
    HIP_CHECK(hipFree(base));
}

}  // namespace eagle

extern "C" {

int eagle_post_stabilise(EagleHandle* h, EaglePostTable* t, const EagleStabParams* p)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_stabilise: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_stabilise: the table belongs to another handle");
    stab_check("eagle_post_stabilise", p);
    if (t->has_stab) fail(EAGLE_E_INVALID, "eagle_post_stabilise: the table has been stabilised already (a second call is refused)");
    const char* derived = t->has_smooth ? "smoothed positions" : t->d_vel ? "velocities" : t->has_poss ? "a possession result" : t->has_occ ? "occupancy maps" :
                          t->has_shape ? "team shapes" : t->has_phys ? "a physical report" : t->has_roles ? "roles" : t->d_space ? "a space result" :
                          t->d_offside ? "an offside result" : t->has_control ? "control parameters" : t->has_flights ? "ball flights" : t->d_goalview ? "a goal view" : nullptr;
    if (derived) fail(EAGLE_E_INVALID, "eagle_post_stabilise: the table already carries %s derived from its positions; stabilising comes first", derived);
    std::vector<uint8_t> kind;
    stab_columns("eagle_post_stabilise", t->columns.data(), t->cols, kind);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)t->rows, cols = (size_t)t->cols, cells = rows * cols;
    const StabKept L = stab_kept(rows, cols);
    {
        double budget = (double)t->max_bytes;
        if (t->max_bytes <= 0) {
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            budget = 0.9 * (double)free_b;
        }
        const double need = (double)L.total + 16.0 * (double)cells + (double)stab_scratch(rows, cols) + (double)rows * 4.0;      // kept, the old positions, scratch, frames
        if (need > budget)
            fail(EAGLE_E_INVALID, "eagle_post_stabilise: %zu columns over %zu rows need %.0f bytes of device memory, the budget is %.0f", cols, rows, need, budget);
    }
    double* d_orig = nullptr;
    uint8_t* kept = nullptr;
    int32_t* d_frames = nullptr;
    const hipStream_t s = h->s_main;
    EagleStabTotals totals{};
    bool copied = false;
    try {
        HIP_CHECK(hipMalloc((void**)&d_orig, std::max<size_t>(cells * 16, 16)));
        HIP_CHECK(hipMalloc((void**)&kept, L.total));
        HIP_CHECK(hipMalloc((void**)&d_frames, std::max<size_t>(rows * 4, 16)));
        if (cells) {
            HIP_CHECK(hipMemcpyAsync(d_frames, t->frames.data(), rows * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(d_orig, t->d_values, cells * 16, hipMemcpyDeviceToDevice, s));
            copied = true;
        }
        stab_run(h, (const double2*)d_orig, d_frames, kind, t->rows, t->cols, p, (double2*)t->d_values, kept, totals, s);
    } catch (...) {
        (void)hipStreamSynchronize(s);
        if (copied) (void)hipMemcpy(t->d_values, d_orig, cells * 16, hipMemcpyDeviceToDevice);      // the table as it was
        if (d_orig) (void)hipFree(d_orig);
        if (kept) (void)hipFree(kept);
        if (d_frames) (void)hipFree(d_frames);
        throw;
    }
    HIP_CHECK(hipFree(d_frames));
    t->d_orig = d_orig; t->d_stab = kept;
    t->host_ok = false;
    t->stab_totals = totals;
    t->has_stab = true;
    API_END(h)
}

int eagle_post_stabilise_values(EaglePostTable* t, EagleStabRow* rows_out, EagleStabTotals* totals, int32_t* votes)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->has_stab) fail(EAGLE_E_INVALID, "eagle_post_stabilise_values: the table has not been stabilised (eagle_post_stabilise)");
    const size_t rows = (size_t)t->rows, cols = (size_t)t->cols, cells = rows * cols;
    const StabKept L = stab_kept(rows, cols);
    const uint8_t* d = (const uint8_t*)t->d_stab;
    if (cells) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        if (rows_out) HIP_CHECK(hipMemcpy(rows_out, d + L.rec, rows * sizeof(EagleStabRow), hipMemcpyDeviceToHost));
        if (votes) HIP_CHECK(hipMemcpy(votes, d + L.votes, cells * 8, hipMemcpyDeviceToHost));
    } else if (rows_out && rows) std::fill(rows_out, rows_out + rows, EagleStabRow{});
    if (totals) *totals = t->stab_totals;
    API_END(h)
}

int eagle_post_device_stabilise(const EaglePostTable* t, const EagleStabRow** d_rows)
{
    if (!t || !d_rows) return EAGLE_E_INVALID;
    *d_rows = t->has_stab && t->rows > 0 && t->cols > 0 ? (const EagleStabRow*)t->d_stab : nullptr;
    return EAGLE_OK;
}

int eagle_post_original_values(EaglePostTable* t, double* values)
{
    if (!t || !values) return EAGLE_E_INVALID;
    if (!t->has_stab) return eagle_post_values(t, values);
    EagleHandle* h = t->h;
    API_BEGIN
    const size_t cells = (size_t)t->rows * (size_t)t->cols;
    if (cells) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        HIP_CHECK(hipMemcpy(values, t->d_orig, cells * 16, hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_op_stabilise(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const EagleStabParams* p,
                       double* out_values, EagleStabRow* rows_out, int32_t* votes, EagleStabTotals* totals)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !frames || !columns || rows < 0 || cols < 0)
        fail(EAGLE_E_INVALID, "eagle_op_stabilise: bad argument (values %p, frames %p, columns %p, %d rows, %d columns)", (const void*)values, (const void*)frames,
             (const void*)columns, rows, cols);
    stab_check("eagle_op_stabilise", p);
    std::vector<uint8_t> kind;
    stab_columns("eagle_op_stabilise", columns, cols, kind);
    for (int r = 1; r < rows; ++r)
        if (frames[r] <= frames[r - 1]) fail(EAGLE_E_INVALID, "eagle_op_stabilise: frame numbers must ascend (row %d: %d after %d)", r, frames[r], frames[r - 1]);
    EagleStabTotals tv{};
    tv.rows = rows; tv.iterations = p->iterations; tv.window = p->window;
    const size_t cells = (size_t)rows * cols;
    if (cells) {
        HIP_CHECK(hipSetDevice(device));
        Net net;
        const StabKept L = stab_kept((size_t)rows, (size_t)cols);
        const double2* d_v = (const double2*)net.upload(values, cells * 16);
        double2* d_o = (double2*)net.upload(values, cells * 16);
        const int32_t* d_f = (const int32_t*)net.upload(frames, (size_t)rows * 4);
        uint8_t* kept = (uint8_t*)net.get(L.total);
        stab_run(nullptr, d_v, d_f, kind, rows, cols, p, d_o, kept, tv, nullptr);
        if (out_values) HIP_CHECK(hipMemcpy(out_values, d_o, cells * 16, hipMemcpyDeviceToHost));
        if (rows_out) HIP_CHECK(hipMemcpy(rows_out, kept + L.rec, (size_t)rows * sizeof(EagleStabRow), hipMemcpyDeviceToHost));
        if (votes) HIP_CHECK(hipMemcpy(votes, kept + L.votes, cells * 8, hipMemcpyDeviceToHost));
    } else if (rows_out && rows > 0) std::fill(rows_out, rows_out + rows, EagleStabRow{});
    if (totals) *totals = tv;
    API_END(hh)
}

}  // extern "C"
