// K37 — track smoothing: the pitch positions of the person columns (and, on request, the ball) of a processed table are replaced by the value at the row
// of a least-squares polynomial over a window of frames around it; samples are fitted once, trimmed against a robust threshold and refitted; the fit's
// derivatives become the table's velocities and an acceleration array (include/eagle.h, eagle_post_smooth_tracks / eagle_op_smooth_tracks;
// tests/smooth_ref.py is the written definition of every bit: integer sums, float64 without contraction, correctly rounded sqrt and division).
//
// Four launches per call on one stream, after post_velocity_kernel has written the velocities of the whole table (the columns not smoothed keep them):
//   smooth_fit_kernel     a workgroup takes SM_TILE rows of one column (blockIdx.y the column; columns that are not smoothed leave at once) plus a halo of
//                         W rows each side and quantises them ONCE into LDS: int32 x, int32 y, the frame number, a used byte (13 bytes a row, 5 KB at
//                         256 + 128 rows).  A thread walks its window from LDS (consecutive threads read consecutive words: no bank conflict), forms the
//                         eleven integer sums in int64 and solves by Cramer's rule in float64; the residual e of its own sample goes to HBM.
//   smooth_flag_kernel    the same tile shape over e (its bit pattern: a non-negative double orders as an unsigned integer).  The median of a window is
//                         the value v with #{< v} <= rank < #{<= v} (the element of that rank by (value, row), however ties are ordered): a thread counts
//                         both per candidate over the one run of slots within W frames, one LDS word per comparison, and stops at the hit: n^2 / 2 on
//                         average for n <= 129.  It writes one outlier byte.
//   smooth_refit_kernel   the fit again with used = present and not outlier; writes position, velocity (with the cap rule), acceleration, flags, count and
//                         residual_q of the smoothed columns, and the NaN acceleration of the others.
//   smooth_totals_kernel  per column the integer totals (a butterfly per wave, integer atomics per wave: no order of arrival can show) and, in the
//                         workgroups of the first column, the suspect byte of the tile's rows.
#include "runtime.h"

static_assert(sizeof(EagleSmoothParams) == 56 && sizeof(EagleSmoothTotals) == 32, "include/eagle.h states these sizes");

namespace eagle {

static constexpr int SM_TILE = 256;            // rows of a column per workgroup, one thread each
static constexpr int SM_WMAX = 64;             // the largest half-width
static constexpr int SM_LDS = SM_TILE + 2 * SM_WMAX;
static constexpr double SM_Q = 1024.0, SM_LIMIT = 1024.0, SM_RES_CAP = 16777216.0;

struct SmoothArgs {
    const double2* values;       // the raw table, [column][row]
    const int32_t* frames;       // [rows]
    const int32_t* colw;         // [cols]: the half-width of a column, 0: not smoothed
    const uint8_t* person;       // [cols]: 1 for a smoothed Player / Goalkeeper column
    int rows, cols, degree;
    double fps, k, floor_q, cap;
    double* e;                   // [column][row] pass 1's residual (scratch)
    uint8_t* outl;               // [column][row] pass 2's decision (scratch)
    double2 *out, *vel, *acc;    // [column][row]; out starts as a copy of values, vel as post_velocity_kernel's result
    uint8_t *flags, *count;      // [column][row], zeroed in front of the launches
    int32_t* resid;
    uint8_t* suspect;            // [rows]
    EagleSmoothTotals* totals;   // [cols], zeroed in front of the launches
};

__device__ __forceinline__ double sm_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool sm_present(double2 v) { return fabs(v.x) <= SM_LIMIT && fabs(v.y) <= SM_LIMIT; }     // false for NaN and +-inf
__device__ __forceinline__ bool sm_near(int fa, int fb, int W) { const long long d = (long long)fa - fb; return d >= -W && d <= W; }

struct SmTile {
    int qx[SM_LDS], qy[SM_LDS], f[SM_LDS];
    uint8_t used[SM_LDS];        // bit 0: a sample of this pass, bit 1: present
};

// rows r0 - W .. r0 + SM_TILE + W - 1 of column c -> LDS slot 0 ..; a row outside the table is not used
template <bool REFIT>
__device__ __forceinline__ void sm_load(const SmoothArgs& a, int c, int r0, int W, SmTile& t)
{
    for (int i = threadIdx.x; i < SM_TILE + 2 * W; i += SM_TILE) {
        const int r = r0 - W + i;
        int qx = 0, qy = 0, f = 0;
        uint8_t u = 0;
        if (r >= 0 && r < a.rows) {
            const double2 v = a.values[(size_t)c * a.rows + r];
            f = a.frames[r];
            if (sm_present(v)) {
                qx = (int)rint(v.x * SM_Q);
                qy = (int)rint(v.y * SM_Q);
                u = 3;
                if (REFIT && a.outl[(size_t)c * a.rows + r]) u = 2;
            }
        }
        t.qx[i] = qx; t.qy[i] = qy; t.f[i] = f; t.used[i] = u;
    }
    __syncthreads();
}

struct SmFit { int n, deg; double ax[3], ay[3]; };

__device__ __forceinline__ void sm_solve(const double* S, const double* B, int deg, double* a)
{
    if (deg == 2) {
        const double C00 = S[2] * S[4] - S[3] * S[3];
        const double C01 = S[2] * S[3] - S[1] * S[4];
        const double C02 = S[1] * S[3] - S[2] * S[2];
        const double C11 = S[0] * S[4] - S[2] * S[2];
        const double C12 = S[1] * S[2] - S[0] * S[3];
        const double C22 = S[0] * S[2] - S[1] * S[1];
        const double det = (S[0] * C00 + S[1] * C01) + S[2] * C02;
        a[0] = ((C00 * B[0] + C01 * B[1]) + C02 * B[2]) / det;
        a[1] = ((C01 * B[0] + C11 * B[1]) + C12 * B[2]) / det;
        a[2] = ((C02 * B[0] + C12 * B[1]) + C22 * B[2]) / det;
    } else if (deg == 1) {
        const double det = S[0] * S[2] - S[1] * S[1];
        a[0] = (S[2] * B[0] - S[1] * B[1]) / det;
        a[1] = (S[0] * B[1] - S[1] * B[0]) / det;
        a[2] = 0.0;
    } else {
        a[0] = B[0] / S[0];
        a[1] = 0.0;
        a[2] = 0.0;
    }
}

// the fit of LDS slot `me` over the used slots within W frames of it (they lie within W slots)
__device__ __forceinline__ SmFit sm_fit(const SmTile& t, int me, int W, int degree)
{
    long long S0 = 0, S1 = 0, S2 = 0, S3 = 0, S4 = 0, X0 = 0, X1 = 0, X2 = 0, Y0 = 0, Y1 = 0, Y2 = 0;
    const int fr = t.f[me];
    for (int j = me - W; j <= me + W; ++j) {
        if (!(t.used[j] & 1)) continue;
        const long long d = (long long)t.f[j] - fr;
        if (d < -W || d > W) continue;
        const long long d2 = d * d, x = t.qx[j], y = t.qy[j];
        S0 += 1; S1 += d; S2 += d2; S3 += d2 * d; S4 += d2 * d2;
        X0 += x; X1 += d * x; X2 += d2 * x;
        Y0 += y; Y1 += d * y; Y2 += d2 * y;
    }
    SmFit o;
    o.n = (int)S0;
    o.deg = S0 >= 4 ? degree : S0 == 3 ? min(degree, 1) : S0 == 2 ? 1 : 0;
    if (S0 > 0) {
        const double S[5] = {(double)S0, (double)S1, (double)S2, (double)S3, (double)S4};
        const double X[3] = {(double)X0, (double)X1, (double)X2}, Y[3] = {(double)Y0, (double)Y1, (double)Y2};
        sm_solve(S, X, o.deg, o.ax);
        sm_solve(S, Y, o.deg, o.ay);
    }
    return o;
}

__device__ __forceinline__ double sm_resid(const SmTile& t, int me, const SmFit& ft)
{
    return fmax(fabs((double)t.qx[me] - ft.ax[0]), fabs((double)t.qy[me] - ft.ay[0]));
}

__global__ __launch_bounds__(SM_TILE) void smooth_fit_kernel(SmoothArgs a)
{
    __shared__ SmTile t;
    const int r0 = blockIdx.x * SM_TILE, r = r0 + threadIdx.x;
    for (int c = blockIdx.y; c < a.cols; c += gridDim.y) {
        const int W = a.colw[c];
        if (W == 0) continue;                                   // uniform over the workgroup
        sm_load<false>(a, c, r0, W, t);
        const int me = threadIdx.x + W;
        if (r < a.rows) {
            double e = -1.0;
            if (t.used[me]) e = sm_resid(t, me, sm_fit(t, me, W, a.degree));
            a.e[(size_t)c * a.rows + r] = e;
        }
        __syncthreads();                                        // the tile is rewritten for the next column
    }
}

__global__ __launch_bounds__(SM_TILE) void smooth_flag_kernel(SmoothArgs a)
{
    __shared__ unsigned long long s_key[SM_LDS];                // the bit pattern of e; SM_UNUSED for a slot that is no sample
    __shared__ int s_f[SM_LDS];
    constexpr unsigned long long SM_UNUSED = ~0ull;             // no finite double
    const int r0 = blockIdx.x * SM_TILE, r = r0 + threadIdx.x;
    for (int c = blockIdx.y; c < a.cols; c += gridDim.y) {
        const int W = a.colw[c];
        if (W == 0) continue;
        for (int i = threadIdx.x; i < SM_TILE + 2 * W; i += SM_TILE) {
            const int rr = r0 - W + i;
            double e = -1.0;
            int f = 0;
            if (rr >= 0 && rr < a.rows) { e = a.e[(size_t)c * a.rows + rr]; f = a.frames[rr]; }
            s_key[i] = e >= 0.0 ? (unsigned long long)__double_as_longlong(e) : SM_UNUSED;
            s_f[i] = f;
        }
        __syncthreads();
        const int me = threadIdx.x + W;
        if (r < a.rows) {
            uint8_t o = 0;
            const unsigned long long km = s_key[me];
            if (km != SM_UNUSED && a.k > 0.0) {
                // frames ascend, so the slots within W frames are one run [lo, hi] around `me`; slots outside the table lie at its ends and are unused
                const int fr = s_f[me];
                int lo = me, hi = me, n = 0;
                for (int j = me - W; j <= me + W; ++j)
                    if (s_key[j] != SM_UNUSED && sm_near(s_f[j], fr, W)) { lo = min(lo, j); hi = max(hi, j); ++n; }
                const int rank = (n - 1) / 2;
                // the element of rank `rank` by (value, row) has the value v with #{< v} <= rank < #{<= v}, whichever way ties are ordered
                unsigned long long med = km;
                for (int i = lo; i <= hi; ++i) {
                    const unsigned long long ki = s_key[i];
                    if (ki == SM_UNUSED) continue;
                    int less = 0, leq = 0;
                    for (int j = lo; j <= hi; ++j) { const unsigned long long kj = s_key[j]; less += kj < ki; leq += kj <= ki; }
                    if (less <= rank && rank < leq) { med = ki; break; }
                }
                o = __longlong_as_double((long long)km) > fmax(a.floor_q, a.k * __longlong_as_double((long long)med));
            }
            a.outl[(size_t)c * a.rows + r] = o;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(SM_TILE) void smooth_refit_kernel(SmoothArgs a)
{
    __shared__ SmTile t;
    const int r0 = blockIdx.x * SM_TILE, r = r0 + threadIdx.x;
    const double2 nn = make_double2(sm_nan(), sm_nan());
    for (int c = blockIdx.y; c < a.cols; c += gridDim.y) {
        const int W = a.colw[c];
        const size_t at = (size_t)c * a.rows + r;
        if (W == 0) {
            if (r < a.rows) a.acc[at] = nn;
            continue;
        }
        sm_load<true>(a, c, r0, W, t);
        const int me = threadIdx.x + W;
        if (r < a.rows) {
            double2 p = nn, v = nn, ac = nn;
            uint8_t fl = 0, cnt = 0;
            int rq = 0;
            const uint8_t u = t.used[me];
            if (u) {
                const SmFit ft = sm_fit(t, me, W, a.degree);
                const uint8_t ob = (u & 1) ? 0 : 2;
                if (ft.n == 0) {
                    p = a.values[at];
                    v = make_double2(0.0, 0.0);
                    ac = v;
                    fl = 16 | ob;
                } else {
                    p = make_double2(ft.ax[0] / SM_Q, ft.ay[0] / SM_Q);
                    v = make_double2((ft.ax[1] * a.fps) / SM_Q, (ft.ay[1] * a.fps) / SM_Q);
                    const double s = sqrt(v.x * v.x + v.y * v.y);
                    if (s > a.cap) { const double k = a.cap / s; v.x = v.x * k; v.y = v.y * k; }
                    ac = make_double2((((2.0 * ft.ax[2]) * a.fps) * a.fps) / SM_Q, (((2.0 * ft.ay[2]) * a.fps) * a.fps) / SM_Q);
                    fl = 1 | ob | (uint8_t)(ft.deg << 2);
                    cnt = (uint8_t)ft.n;
                    rq = (int)rint(fmin(16.0 * sm_resid(t, me, ft), SM_RES_CAP));
                }
            }
            a.out[at] = p; a.vel[at] = v; a.acc[at] = ac;
            a.flags[at] = fl; a.count[at] = cnt; a.resid[at] = rq;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ long long sm_wave_sum(long long v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(SM_TILE) void smooth_totals_kernel(SmoothArgs a)
{
    const int r = blockIdx.x * SM_TILE + threadIdx.x;
    const bool in = r < a.rows;
    for (int c = blockIdx.y; c < a.cols; c += gridDim.y) {
        if (a.colw[c] == 0) continue;
        const size_t at = (size_t)c * a.rows + r;
        const int fl = in ? a.flags[at] : 0;
        const long long rq = in ? a.resid[at] : 0;
        const long long present = sm_wave_sum(fl != 0), outl = sm_wave_sum((fl >> 1) & 1), low = sm_wave_sum(fl != 0 && ((fl >> 2) & 3) < a.degree);
        const long long sq = sm_wave_sum(rq * rq);
        int mx = (int)rq;
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
        if ((threadIdx.x & 63) == 0 && present) {
            EagleSmoothTotals* T = a.totals + c;
            atomicAdd(&T->present, (int)present);
            if (outl) atomicAdd(&T->outliers, (int)outl);
            if (low) atomicAdd(&T->low_degree, (int)low);
            if (sq) atomicAdd((unsigned long long*)&T->sum_sq, (unsigned long long)sq);
            if (mx) atomicMax(&T->max_residual_q, mx);
        }
    }
    if (blockIdx.y == 0 && in) {                                // the suspect byte of this tile's rows
        int present = 0, outl = 0;
        for (int c = 0; c < a.cols; ++c) {
            if (!a.person[c]) continue;
            const int fl = a.flags[(size_t)c * a.rows + r];
            present += fl != 0;
            outl += (fl >> 1) & 1;
        }
        a.suspect[r] = present >= 4 && 2 * outl >= present;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void smooth_check(const char* who, const EagleSmoothParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: params is NULL", who);
    if (p->fps <= 0 || p->max_gap <= 0 || !(p->speed_cap > 0) || !std::isfinite(p->speed_cap))
        fail(EAGLE_E_INVALID, "%s: fps %d, max_gap %d and speed_cap %g must be positive (and finite)", who, p->fps, p->max_gap, p->speed_cap);
    if (p->window < 1 || p->window > SM_WMAX) fail(EAGLE_E_INVALID, "%s: window %d is outside 1 .. %d", who, p->window, SM_WMAX);
    if (p->degree != 1 && p->degree != 2) fail(EAGLE_E_INVALID, "%s: degree %d is neither 1 nor 2", who, p->degree);
    if (p->ball_window < 0 || p->ball_window > SM_WMAX) fail(EAGLE_E_INVALID, "%s: ball_window %d is outside 0 .. %d", who, p->ball_window, SM_WMAX);
    if (!std::isfinite(p->outlier_k) || p->outlier_k < 0.0) fail(EAGLE_E_INVALID, "%s: outlier_k %g must be 0 (no trimming) or finite and positive", who, p->outlier_k);
    if (!std::isfinite(p->outlier_floor) || p->outlier_floor < 0.0) fail(EAGLE_E_INVALID, "%s: outlier_floor %g must be finite and not negative", who, p->outlier_floor);
}

// the half-width of every column (0: not smoothed) and which of them are smoothed persons
static void smooth_columns(const char* who, const EaglePostColumn* columns, int ncols, const EagleSmoothParams* p, std::vector<int32_t>& colw, std::vector<uint8_t>& person)
{
    colw.assign((size_t)ncols, 0); person.assign((size_t)ncols, 0);
    for (int c = 0; c < ncols; ++c) {
        const EaglePostColumn& col = columns[c];
        if (col.kind != EAGLE_POST_PLAYER && col.kind != EAGLE_POST_GOALKEEPER && col.kind != EAGLE_POST_BALL && col.kind != EAGLE_POST_BOUNDARY)
            fail(EAGLE_E_INVALID, "%s: column %d is of unknown kind %d", who, c, col.kind);
        if (col.video) continue;
        if (col.kind == EAGLE_POST_PLAYER || col.kind == EAGLE_POST_GOALKEEPER) { colw[c] = p->window; person[c] = 1; }
        else if (col.kind == EAGLE_POST_BALL) colw[c] = p->ball_window;
    }
}

static size_t sm_up(size_t b) { return (std::max<size_t>(b, 16) + 255) & ~(size_t)255; }

// What a call keeps: acc f64 [cols][rows][2] | residual_q i32 [cols][rows] | flags u8 [cols][rows] | count u8 [cols][rows] | suspect u8 [rows] |
// totals [cols], each from a 256-byte boundary
struct SmoothKept { size_t acc, resid, flags, count, suspect, totals, total; };

static SmoothKept smooth_kept(size_t rows, size_t cols)
{
    SmoothKept o{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += sm_up(b); return was; };
    const size_t cells = rows * cols;
    o.acc = take(cells * 16); o.resid = take(cells * 4); o.flags = take(cells); o.count = take(cells); o.suspect = take(rows); o.totals = take(cols * sizeof(EagleSmoothTotals));
    o.total = at;
    return o;
}

static size_t smooth_scratch(size_t rows, size_t cols) { return sm_up(rows * cols * 8) + sm_up(rows * cols) + sm_up(cols * 4) + sm_up(cols); }

// d_values: the raw table; d_out: a copy of it (the smoothed columns are overwritten); d_vel: [cols][rows][2]; kept: smooth_kept's block.  Returns when
// everything is complete; totals_out has the window of every column filled in.
static void smooth_run(EagleHandle* h, const double2* d_values, const int32_t* d_frames, const EaglePostColumn* columns, int rows, int cols, const EagleSmoothParams* p,
                       double2* d_out, double2* d_vel, uint8_t* kept, std::vector<EagleSmoothTotals>& totals_out, hipStream_t s)
{
    std::vector<int32_t> colw;
    std::vector<uint8_t> person;
    smooth_columns("smooth", columns, cols, p, colw, person);
    totals_out.assign((size_t)cols, EagleSmoothTotals{});
    for (int c = 0; c < cols; ++c) totals_out[c].window = colw[c];
    if (rows <= 0 || cols <= 0) return;
    const SmoothKept L = smooth_kept((size_t)rows, (size_t)cols);
    const size_t cells = (size_t)rows * cols;
    uint8_t* base = nullptr;
    HIP_CHECK(hipMalloc((void**)&base, smooth_scratch((size_t)rows, (size_t)cols)));
    try {
        SmoothArgs a{};
        a.values = d_values; a.frames = d_frames; a.rows = rows; a.cols = cols; a.degree = p->degree;
        a.fps = (double)p->fps; a.k = p->outlier_k; a.floor_q = p->outlier_floor * SM_Q; a.cap = p->speed_cap;
        a.e = (double*)base; a.outl = base + sm_up(cells * 8);
        uint8_t* d_colw = a.outl + sm_up(cells);
        uint8_t* d_person = d_colw + sm_up((size_t)cols * 4);
        a.colw = (const int32_t*)d_colw; a.person = d_person;
        a.out = d_out; a.vel = d_vel; a.acc = (double2*)(kept + L.acc);
        a.resid = (int32_t*)(kept + L.resid); a.flags = kept + L.flags; a.count = kept + L.count; a.suspect = kept + L.suspect;
        a.totals = (EagleSmoothTotals*)(kept + L.totals);
        HIP_CHECK(hipMemcpyAsync(d_colw, colw.data(), (size_t)cols * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(d_person, person.data(), (size_t)cols, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(kept + L.resid, 0, L.total - L.resid, s));           // residual_q, flags, count, suspect, totals
        EagleKinematicsParams kp{};
        kp.fps = p->fps; kp.max_gap = p->max_gap; kp.speed_cap = p->speed_cap;
        const dim3 grid((unsigned)((rows + SM_TILE - 1) / SM_TILE), (unsigned)std::min(cols, 65535));
        auto vel_k = [&] { velocity_launch(d_values, d_frames, d_vel, rows, cols, &kp, s); };
        auto fit_k = [&] { hipLaunchKernelGGL(smooth_fit_kernel, grid, dim3(SM_TILE), 0, s, a); HIP_CHECK(hipGetLastError()); };
        auto flag_k = [&] { hipLaunchKernelGGL(smooth_flag_kernel, grid, dim3(SM_TILE), 0, s, a); HIP_CHECK(hipGetLastError()); };
        auto refit_k = [&] { hipLaunchKernelGGL(smooth_refit_kernel, grid, dim3(SM_TILE), 0, s, a); HIP_CHECK(hipGetLastError()); };
        auto totals_k = [&] { hipLaunchKernelGGL(smooth_totals_kernel, grid, dim3(SM_TILE), 0, s, a); HIP_CHECK(hipGetLastError()); };
        size_t ns = 0;
        for (int c = 0; c < cols; ++c) ns += colw[c] != 0;
        const double sc = (double)ns * (double)rows;          // smoothed cells: 16 bytes read and 8 written by the fit, 8 + 1 by the flag kernel, 17 + 54 by the refit
        if (h) {
            timed_launch(h, "post_velocity", 32.0 * (double)cells, s, vel_k);
            timed_launch(h, "smooth_fit", 24.0 * sc, s, fit_k);
            timed_launch(h, "smooth_flag", 9.0 * sc, s, flag_k);
            timed_launch(h, "smooth_refit", 71.0 * sc + 16.0 * ((double)cells - sc), s, refit_k);
            timed_launch(h, "smooth_totals", 6.0 * sc, s, totals_k);
        } else { vel_k(); fit_k(); flag_k(); refit_k(); totals_k(); }
        HIP_CHECK(hipMemcpyAsync(totals_out.data(), a.totals, (size_t)cols * sizeof(EagleSmoothTotals), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h && h->prof) collect_spans(h);
        for (int c = 0; c < cols; ++c) totals_out[c].window = colw[c];
    } catch (...) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(base);
        throw;
    }
    HIP_CHECK(hipFree(base));
}

}  // namespace eagle

extern "C" {

int eagle_post_smooth_tracks(EagleHandle* h, EaglePostTable* t, const EagleSmoothParams* p)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_smooth_tracks: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_smooth_tracks: the table belongs to another handle");
    smooth_check("eagle_post_smooth_tracks", p);
    if (t->has_smooth) fail(EAGLE_E_INVALID, "eagle_post_smooth_tracks: the table has been smoothed already (a second call is refused)");
    const char* derived = t->d_vel ? "velocities" : t->has_poss ? "a possession result" : t->has_occ ? "occupancy maps" : t->has_shape ? "team shapes" :
                          t->has_phys ? "a physical report" : t->has_roles ? "roles" : t->d_space ? "a space result" : t->d_offside ? "an offside result" :
                          t->has_control ? "control parameters" : t->has_flights ? "ball flights" : t->d_goalview ? "a goal view" : nullptr;
    if (derived) fail(EAGLE_E_INVALID, "eagle_post_smooth_tracks: the table already carries %s derived from its positions; smoothing comes first", derived);
    std::vector<int32_t> colw;
    std::vector<uint8_t> person;
    smooth_columns("eagle_post_smooth_tracks", t->columns.data(), t->cols, p, colw, person);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)t->rows, cols = (size_t)t->cols, cells = rows * cols;
    const SmoothKept L = smooth_kept(rows, cols);
    {
        double budget = (double)t->max_bytes;
        if (t->max_bytes <= 0) {
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            budget = 0.9 * (double)free_b;
        }
        const double need = (double)L.total + 32.0 * (double)cells + (double)smooth_scratch(rows, cols) + (double)rows * 4.0;      // kept, raw + velocities, scratch, frames
        if (need > budget)
            fail(EAGLE_E_INVALID, "eagle_post_smooth_tracks: %zu columns over %zu rows need %.0f bytes of device memory, the budget is %.0f", cols, rows, need, budget);
    }
    double *d_raw = nullptr, *d_vel = nullptr;
    uint8_t* kept = nullptr;
    int32_t* d_frames = nullptr;
    const hipStream_t s = h->s_main;
    std::vector<EagleSmoothTotals> totals;
    bool copied = false;
    try {
        HIP_CHECK(hipMalloc((void**)&d_raw, std::max<size_t>(cells * 16, 16)));
        HIP_CHECK(hipMalloc((void**)&d_vel, std::max<size_t>(cells * 16, 16)));
        HIP_CHECK(hipMalloc((void**)&kept, L.total));
        HIP_CHECK(hipMalloc((void**)&d_frames, std::max<size_t>(rows * 4, 16)));
        if (cells) {
            HIP_CHECK(hipMemcpyAsync(d_frames, t->frames.data(), rows * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(d_raw, t->d_values, cells * 16, hipMemcpyDeviceToDevice, s));
            copied = true;
        }
        smooth_run(h, (const double2*)d_raw, d_frames, t->columns.data(), t->rows, t->cols, p, (double2*)t->d_values, (double2*)d_vel, kept, totals, s);
    } catch (...) {
        (void)hipStreamSynchronize(s);
        if (copied) (void)hipMemcpy(t->d_values, d_raw, cells * 16, hipMemcpyDeviceToDevice);      // the table as it was
        if (d_raw) (void)hipFree(d_raw);
        if (d_vel) (void)hipFree(d_vel);
        if (kept) (void)hipFree(kept);
        if (d_frames) (void)hipFree(d_frames);
        throw;
    }
    HIP_CHECK(hipFree(d_frames));
    t->d_raw = d_raw; t->d_vel = d_vel; t->d_smooth = kept;
    t->kin = EagleKinematicsParams{};
    t->kin.fps = p->fps; t->kin.max_gap = p->max_gap; t->kin.speed_cap = p->speed_cap;
    t->host_ok = false; t->host_vel_ok = false;
    t->smooth_totals.swap(totals);
    t->has_smooth = true;
    API_END(h)
}

int eagle_post_smooth_values(EaglePostTable* t, double* acc, uint8_t* flags, uint8_t* count, int32_t* residual_q, uint8_t* suspect, EagleSmoothTotals* totals)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->has_smooth) fail(EAGLE_E_INVALID, "eagle_post_smooth_values: the table has not been smoothed (eagle_post_smooth_tracks)");
    const size_t rows = (size_t)t->rows, cols = (size_t)t->cols, cells = rows * cols;
    const SmoothKept L = smooth_kept(rows, cols);
    const uint8_t* d = (const uint8_t*)t->d_smooth;
    if (cells) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        if (acc) HIP_CHECK(hipMemcpy(acc, d + L.acc, cells * 16, hipMemcpyDeviceToHost));
        if (flags) HIP_CHECK(hipMemcpy(flags, d + L.flags, cells, hipMemcpyDeviceToHost));
        if (count) HIP_CHECK(hipMemcpy(count, d + L.count, cells, hipMemcpyDeviceToHost));
        if (residual_q) HIP_CHECK(hipMemcpy(residual_q, d + L.resid, cells * 4, hipMemcpyDeviceToHost));
        if (suspect) HIP_CHECK(hipMemcpy(suspect, d + L.suspect, rows, hipMemcpyDeviceToHost));
    }
    if (totals) std::copy(t->smooth_totals.begin(), t->smooth_totals.end(), totals);
    API_END(h)
}

int eagle_post_device_smooth(const EaglePostTable* t, const double** d_acc, const uint8_t** d_flags, const uint8_t** d_suspect)
{
    if (!t || !d_acc || !d_flags || !d_suspect) return EAGLE_E_INVALID;
    const uint8_t* d = t->has_smooth ? (const uint8_t*)t->d_smooth : nullptr;
    const SmoothKept L = smooth_kept((size_t)t->rows, (size_t)t->cols);
    *d_acc = d ? (const double*)(d + L.acc) : nullptr;
    *d_flags = d ? d + L.flags : nullptr;
    *d_suspect = d ? d + L.suspect : nullptr;
    return EAGLE_OK;
}

int eagle_post_raw_values(EaglePostTable* t, double* values)
{
    if (!t || !values) return EAGLE_E_INVALID;
    if (!t->has_smooth) return eagle_post_values(t, values);
    EagleHandle* h = t->h;
    API_BEGIN
    const size_t cells = (size_t)t->rows * (size_t)t->cols;
    if (cells) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        HIP_CHECK(hipMemcpy(values, t->d_raw, cells * 16, hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_op_smooth_tracks(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const EagleSmoothParams* p,
                           double* out_values, double* out_vel, double* out_acc, uint8_t* flags, uint8_t* count, int32_t* residual_q, uint8_t* suspect,
                           EagleSmoothTotals* totals)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !frames || !columns || rows < 0 || cols < 0)
        fail(EAGLE_E_INVALID, "eagle_op_smooth_tracks: bad argument (values %p, frames %p, columns %p, %d rows, %d columns)", (const void*)values, (const void*)frames,
             (const void*)columns, rows, cols);
    smooth_check("eagle_op_smooth_tracks", p);
    std::vector<int32_t> colw;
    std::vector<uint8_t> person;
    smooth_columns("eagle_op_smooth_tracks", columns, cols, p, colw, person);
    for (int r = 1; r < rows; ++r)
        if (frames[r] <= frames[r - 1]) fail(EAGLE_E_INVALID, "eagle_op_smooth_tracks: frame numbers must ascend (row %d: %d after %d)", r, frames[r], frames[r - 1]);
    std::vector<EagleSmoothTotals> tv((size_t)cols, EagleSmoothTotals{});
    for (int c = 0; c < cols; ++c) tv[c].window = colw[c];
    const size_t cells = (size_t)rows * cols;
    if (cells) {
        HIP_CHECK(hipSetDevice(device));
        Net net;
        const SmoothKept L = smooth_kept((size_t)rows, (size_t)cols);
        const double2* d_v = (const double2*)net.upload(values, cells * 16);
        double2* d_o = (double2*)net.upload(values, cells * 16);
        const int32_t* d_f = (const int32_t*)net.upload(frames, (size_t)rows * 4);
        double2* d_vel = (double2*)net.get(cells * 16);
        uint8_t* kept = (uint8_t*)net.get(L.total);
        smooth_run(nullptr, d_v, d_f, columns, rows, cols, p, d_o, d_vel, kept, tv, nullptr);
        if (out_values) HIP_CHECK(hipMemcpy(out_values, d_o, cells * 16, hipMemcpyDeviceToHost));
        if (out_vel) HIP_CHECK(hipMemcpy(out_vel, d_vel, cells * 16, hipMemcpyDeviceToHost));
        if (out_acc) HIP_CHECK(hipMemcpy(out_acc, kept + L.acc, cells * 16, hipMemcpyDeviceToHost));
        if (flags) HIP_CHECK(hipMemcpy(flags, kept + L.flags, cells, hipMemcpyDeviceToHost));
        if (count) HIP_CHECK(hipMemcpy(count, kept + L.count, cells, hipMemcpyDeviceToHost));
        if (residual_q) HIP_CHECK(hipMemcpy(residual_q, kept + L.resid, cells * 4, hipMemcpyDeviceToHost));
        if (suspect) HIP_CHECK(hipMemcpy(suspect, kept + L.suspect, (size_t)rows, hipMemcpyDeviceToHost));
    }
    if (totals) std::copy(tv.begin(), tv.end(), totals);
    API_END(hh)
}

}  // extern "C"
