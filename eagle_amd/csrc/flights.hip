// K40 — ball flights: the ball's pitch column of a processed table is cut into straight lines of constant speed (flights) by a segmented least-squares
// fit, solved exactly by a dynamic program over the kept rows; where two lines meet is a knot, a knot with a large change of velocity a kick
// (include/eagle.h, eagle_post_ball_flights / eagle_op_ball_flights; tests/flights_ref.py is the written definition of every bit: integer sums,
// float64 without contraction, correctly rounded sqrt and division).
//
// No sum can overflow: validation bounds max_gap <= 1024 and L <= 128, so over the at most 129 rows of a segment t = f[r'] - f[i] < 2^17 and
// |d| = |q[r'] - q[i]| <= 2^21; S0 < 2^8, S1 < 2^25, S2 < 2^42, |B0| < 2^29, |B1| < 2^46, Q < 2^50, S0 S2 and S1 S1 < 2^50: all exact in int64 AND in
// float64.  The spike test: |q differences| <= 2^21 times D <= 2^11 -> A < 2^34, A D < 2^45, T D <= 2^31.  best <= rows (2^40 + 2^40) <= 2^61 for
// rows <= 2^20; FL_INF = 2^62 is never reached.
//
//   flights_prepare_kernel  a workgroup takes FL_TILE rows plus a halo of two each side into LDS (a spike needs A of its neighbours, A needs q of its
//                           neighbours): presence and q, run heads (the cuts by binary search), A and D, the spike decision; and per present row the
//                           nearest person (possession's candidate arithmetic).
//   flights_scan_kernel     one workgroup: inclusive prefix sum of a flag array, the flagged indices compacted in order, the total.  Used for the runs
//                           that have a segment, the segment numbers and the kicks.
//   flights_cost_kernel     the hot path: one lane per start row i walks its L ends from an LDS tile of FL_TILE + L rows of (q, f, used, head), the nine
//                           sums kept incrementally in registers, a Cramer solve per used end, c(i, j) to HBM.  The layout of c is a parameter: end-major
//                           c[j][k] (the walk's loads are one run of 8 L bytes, this kernel's stores are strided) or k-major c[k][j] (the reverse,
//                           and the default: cost plus walk is about 1 % less in every measured case, docs/experiments.md has both).
//   flights_walk_kernel     one wave per run, rows in order.  Lane l holds the offsets k = l + 1 and l + 65; the last 256 values of best live in LDS;
//                           c of the NEXT row is loaded while this row's minimum is taken (a (value, k) butterfly over the wave, the larger k on a
//                           tie = the smaller i).  Latency-bound by construction.
//   flights_double / mark   the path by pointer doubling, balltrack.hip's scheme: a marked row marks its 2^k-th predecessor, k from high to low.
//   flights_segend_kernel   the rows that end a segment; their prefix sum numbers the segments in row order.
//   flights_fit_kernel      one thread per segment: the sums once more, the record, the fit for the rows kernel.
//   flights_rows_kernel     one thread per row: seg, flags, fitted position, velocity; at a knot the kick decision and the `continues` flag.
//   flights_kicks_kernel    one thread per kick; flights_totals_kernel the integer totals (a butterfly per wave, integer atomics: no order can show).
#include "runtime.h"

static_assert(sizeof(EagleFlightParams) == 96 && sizeof(EagleBallFlight) == 112 && sizeof(EagleBallKick) == 48 && sizeof(EagleFlightTotals) == 64,
              "include/eagle.h states these sizes");

namespace eagle {

static constexpr int FL_TILE = 256, FL_LMAX = 128, FL_MAX_ROWS = 1 << 20, FL_RING = 256;
static constexpr long long FL_INF = 1ll << 62;
static constexpr double FL_Q = 1024.0, FL_LIMIT = 1024.0, FL_CAP = 1099511627776.0;
static constexpr int FL_HEAD = 0x80;                   // the walk's own bit beside the row flags

struct FlArgs {
    const double2* values;       // the table, [column][row]
    const int32_t* frames;       // [rows]
    const int32_t* persons;      // person columns in table order
    const int32_t* cuts;         // [n_cuts] ascending frame numbers
    int rows, npersons, ball, n_cuts, L, max_gap, kmajor;
    long long T, lam;
    double r2, fps, kick_dv, still_speed, shot_speed, shot_range, shot_margin;
    // scratch, per row
    int32_t *qx, *qy, *cand, *pred, *mark, *jump, *runflag, *runlist, *segnum, *kickflag, *kicklist;
    uint8_t *head, *rf;
    long long* c;                // [rows][L] or [L][rows]
    int32_t* counts;             // runs with a segment, segments, kicks
    // per segment
    EagleBallFlight* flights; double4* segfit; EagleBallKick* kicks; int nseg, nkick;
    // kept
    int32_t* seg; uint8_t* flags; double2 *fitted, *velocity; EagleFlightTotals* totals;
};

__device__ __forceinline__ double fl_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool fl_finite(double2 p) { return fabs(p.x) <= 1.7976931348623157e308 && fabs(p.y) <= 1.7976931348623157e308; }

__device__ __forceinline__ bool fl_is_cut(const FlArgs& a, int f)
{
    int lo = 0, hi = a.n_cuts;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.cuts[mid] < f) lo = mid + 1; else hi = mid;
    }
    return lo < a.n_cuts && a.cuts[lo] == f;
}

__global__ __launch_bounds__(FL_TILE) void flights_prepare_kernel(FlArgs a)
{
    constexpr int N = FL_TILE + 4;                     // slot s is row r0 - 2 + s
    __shared__ int s_qx[N], s_qy[N], s_f[N], s_D[N];
    __shared__ long long s_A[N];
    __shared__ uint8_t s_p[N], s_h[N];
    const int r0 = blockIdx.x * FL_TILE, tid = threadIdx.x;
    for (int s = tid; s < N; s += FL_TILE) {
        const int r = r0 - 2 + s;
        int qx = 0, qy = 0, f = 0;
        uint8_t p = 0;
        if (r >= 0 && r < a.rows) {
            f = a.frames[r];
            if (a.ball >= 0) {
                const double2 v = a.values[(size_t)a.ball * a.rows + r];
                if (fabs(v.x) <= FL_LIMIT && fabs(v.y) <= FL_LIMIT) { p = 1; qx = (int)rint(v.x * FL_Q); qy = (int)rint(v.y * FL_Q); }
            }
        }
        s_qx[s] = qx; s_qy[s] = qy; s_f[s] = f; s_p[s] = p;
    }
    __syncthreads();
    for (int s = tid; s < N; s += FL_TILE) {
        const int r = r0 - 2 + s;
        uint8_t h = 1;                                 // a row outside the table is the head of nothing's run
        if (r >= 0 && r < a.rows && s >= 1)
            h = r == 0 || !s_p[s] || !s_p[s - 1] || (long long)s_f[s] - s_f[s - 1] > a.max_gap || fl_is_cut(a, s_f[s]);
        s_h[s] = h;
    }
    __syncthreads();
    for (int s = tid; s < N; s += FL_TILE) {
        long long A = 0;
        int D = 1;
        if (s >= 1 && s + 1 < N && s_p[s] && !s_h[s] && !s_h[s + 1]) {
            D = s_f[s + 1] - s_f[s - 1];
            const long long tr = s_f[s] - s_f[s - 1];
            const long long ax = ((long long)s_qx[s] - s_qx[s - 1]) * D - ((long long)s_qx[s + 1] - s_qx[s - 1]) * tr;
            const long long ay = ((long long)s_qy[s] - s_qy[s - 1]) * D - ((long long)s_qy[s + 1] - s_qy[s - 1]) * tr;
            A = max(ax < 0 ? -ax : ax, ay < 0 ? -ay : ay);
        }
        s_A[s] = A; s_D[s] = D;
    }
    __syncthreads();
    const int r = r0 + tid, s = tid + 2;
    if (r >= a.rows) return;
    const long long A = s_A[s], D = s_D[s];
    const bool spike = A > a.T * D && A * s_D[s - 1] > s_A[s - 1] * D && A * s_D[s + 1] >= s_A[s + 1] * D;
    const bool p = s_p[s] != 0;
    a.qx[r] = s_qx[s]; a.qy[r] = s_qy[s];
    a.head[r] = s_h[s];
    a.rf[r] = (uint8_t)((p ? EAGLE_FLIGHT_ROW_PRESENT : 0) | (p && !spike ? EAGLE_FLIGHT_ROW_USED : 0) | (spike ? EAGLE_FLIGHT_ROW_SPIKE : 0));
    a.runflag[r] = p && s_h[s] && !s_h[s + 1];
    int bc = -1;
    if (p) {
        const double2 b = a.values[(size_t)a.ball * a.rows + r];
        double best = 0.0;
        for (int k = 0; k < a.npersons; ++k) {
            const int c = a.persons[k];
            const double2 q = a.values[(size_t)c * a.rows + r];
            if (!fl_finite(q)) continue;
            const double dx = q.x - b.x, dy = q.y - b.y;
            const double d2 = dx * dx + dy * dy;
            if (bc < 0 || d2 < best) { best = d2; bc = c; }          // a tie keeps the earlier column
        }
        if (!(bc >= 0 && best <= a.r2)) bc = -1;
    }
    a.cand[r] = bc;
}

// v: flags -> their inclusive prefix sum; list (or nullptr): the flagged indices in order; total[0]: their number
__global__ __launch_bounds__(1024) void flights_scan_kernel(int32_t* v, int n, int32_t* list, int32_t* total)
{
    __shared__ int part[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        const int flag = i < n ? v[i] : 0;
        int x = flag;
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(x, d, 64);
            if (lane >= d) x += o;
        }
        if (lane == 63) part[wave] = x;
        __syncthreads();
        int before = 0, sum = 0;
        #pragma unroll
        for (int w = 0; w < 16; ++w) { before += w < wave ? part[w] : 0; sum += part[w]; }
        if (i < n) {
            const int pos = carry + before + x;
            v[i] = pos;
            if (flag && list) list[pos - 1] = i;       // pos - 1 < n: at most one per index
        }
        carry += sum;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = carry;
}

struct FlSums { long long S0, S1, S2, B0x, B1x, Qx, B0y, B1y, Qy; };

__device__ __forceinline__ void fl_add(FlSums& s, long long t, long long dx, long long dy)
{
    s.S0 += 1; s.S1 += t; s.S2 += t * t;
    s.B0x += dx; s.B1x += t * dx; s.Qx += dx * dx;
    s.B0y += dy; s.B1y += t * dy; s.Qy += dy * dy;
}

// c of the sums and the fit (a0x, a1x, a0y, a1y)
__device__ __forceinline__ long long fl_solve(const FlSums& s, double4& fit)
{
    const double det = (double)(s.S0 * s.S2 - s.S1 * s.S1);
    const double S0 = (double)s.S0, S1 = (double)s.S1, S2 = (double)s.S2;
    const double B0x = (double)s.B0x, B1x = (double)s.B1x, B0y = (double)s.B0y, B1y = (double)s.B1y;
    fit.x = (S2 * B0x - S1 * B1x) / det;
    fit.y = (S0 * B1x - S1 * B0x) / det;
    fit.z = (S2 * B0y - S1 * B1y) / det;
    fit.w = (S0 * B1y - S1 * B0y) / det;
    const double ex = fmax(0.0, (double)s.Qx - (fit.x * B0x + fit.y * B1x));
    const double ey = fmax(0.0, (double)s.Qy - (fit.z * B0y + fit.w * B1y));
    return (long long)rint(fmin(ex + ey, FL_CAP));
}

__device__ __forceinline__ size_t fl_at(const FlArgs& a, int j, int k)      // c(j - k, j), 1 <= k <= L
{
    return a.kmajor ? (size_t)(k - 1) * a.rows + j : (size_t)j * a.L + (k - 1);
}

__global__ __launch_bounds__(FL_TILE) void flights_cost_kernel(FlArgs a)
{
    constexpr int N = FL_TILE + FL_LMAX;               // slot s is row r0 + s
    __shared__ int s_qx[N], s_qy[N], s_f[N];
    __shared__ uint8_t s_u[N];                         // the row flags, FL_HEAD for a run's first row and for a row outside the table
    const int r0 = blockIdx.x * FL_TILE, tid = threadIdx.x;
    for (int s = tid; s < FL_TILE + a.L; s += FL_TILE) {
        const int r = r0 + s;
        int qx = 0, qy = 0, f = 0;
        uint8_t u = FL_HEAD;
        if (r < a.rows) { qx = a.qx[r]; qy = a.qy[r]; f = a.frames[r]; u = (uint8_t)(a.rf[r] | (a.head[r] ? FL_HEAD : 0)); }
        s_qx[s] = qx; s_qy[s] = qy; s_f[s] = f; s_u[s] = u;
    }
    __syncthreads();
    const int i = r0 + tid;
    if (i >= a.rows || !(s_u[tid] & EAGLE_FLIGHT_ROW_USED)) return;
    FlSums sm{1, 0, 0, 0, 0, 0, 0, 0, 0};
    const int fi = s_f[tid], xi = s_qx[tid], yi = s_qy[tid];
    for (int k = 1; k <= a.L; ++k) {
        const int s = tid + k;
        const uint8_t u = s_u[s];
        if (u & FL_HEAD) break;                        // the run has ended (or the table)
        if (!(u & EAGLE_FLIGHT_ROW_USED)) continue;
        fl_add(sm, (long long)s_f[s] - fi, (long long)s_qx[s] - xi, (long long)s_qy[s] - yi);
        double4 fit;
        a.c[fl_at(a, i + k, k)] = fl_solve(sm, fit);   // i + k < rows: the slot is inside the table
    }
}

__global__ __launch_bounds__(64) void flights_walk_kernel(FlArgs a, int nruns)
{
    __shared__ long long ring[FL_RING];                // best of row r at r & 255; FL_INF: not a used row
    const int lane = threadIdx.x;
    const int k1 = lane + 1, k2 = lane + 65;
    const bool has1 = k1 <= a.L, has2 = k2 <= a.L;
    for (int run = blockIdx.x; run < nruns; run += gridDim.x) {
        const int first = a.runlist[run];
        __syncthreads();
        for (int s = lane; s < FL_RING; s += 64) ring[s] = FL_INF;
        __syncthreads();
        if (lane == 0) ring[first & (FL_RING - 1)] = 0;
        __syncthreads();
        int last = first;
        long long n1 = 0, n2 = 0;                      // c of the row about to be walked
        if (first + 1 < a.rows) {
            if (has1) n1 = a.c[fl_at(a, first + 1, k1)];
            if (has2) n2 = a.c[fl_at(a, first + 1, k2)];
        }
        bool done = false;
        for (int j0 = first + 1; !done; j0 += 64) {
            const int rr = j0 + lane;
            const int mine = rr < a.rows ? (a.rf[rr] | (a.head[rr] ? FL_HEAD : 0)) : FL_HEAD;
            for (int jj = 0; jj < 64; ++jj) {
                const int fl = __shfl(mine, jj, 64);
                if (fl & FL_HEAD) { done = true; break; }          // (uniform)
                const int j = j0 + jj;
                last = j;
                const long long c1 = n1, c2 = n2;
                if (j + 1 < a.rows) {                  // the next row's, in flight during this row's minimum; what it reads may be unwritten and is then unused
                    if (has1) n1 = a.c[fl_at(a, j + 1, k1)];
                    if (has2) n2 = a.c[fl_at(a, j + 1, k2)];
                }
                if (!(fl & EAGLE_FLIGHT_ROW_USED)) {
                    if (lane == 0) ring[j & (FL_RING - 1)] = FL_INF;
                    __syncthreads();
                    continue;
                }
                long long v = FL_INF;
                int k = 0;
                if (has1 && j - k1 >= first) {
                    const long long b = ring[(j - k1) & (FL_RING - 1)];
                    if (b < FL_INF) { v = b + c1 + a.lam; k = k1; }
                }
                if (has2 && j - k2 >= first) {
                    const long long b = ring[(j - k2) & (FL_RING - 1)];
                    if (b < FL_INF && b + c2 + a.lam <= v) { v = b + c2 + a.lam; k = k2; }      // a tie: the larger k is the smaller i
                }
                #pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    const long long ov = __shfl_xor(v, d, 64);
                    const int ok = __shfl_xor(k, d, 64);
                    if (ov < v || (ov == v && ok > k)) { v = ov; k = ok; }
                }
                if (lane == 0) { ring[j & (FL_RING - 1)] = v; a.pred[j] = j - k; }
                __syncthreads();
            }
        }
        if (lane == 0) a.mark[last] = 1;
    }
}

__global__ __launch_bounds__(256) void flights_double_kernel(const int32_t* from, int32_t* to, int n)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const int t = from[v];
    to[v] = t >= 0 ? from[t] : -1;
}

__global__ __launch_bounds__(256) void flights_mark_kernel(const int32_t* jump, int32_t* mark, int n)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n || !mark[v]) return;
    const int t = jump[v];
    if (t >= 0) mark[t] = 1;
}

__global__ __launch_bounds__(256) void flights_segend_kernel(FlArgs a)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < a.rows) a.segnum[r] = a.mark[r] && a.pred[r] >= 0;
}

__global__ __launch_bounds__(256) void flights_fit_kernel(FlArgs a)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.rows || !a.mark[j]) return;
    const int i = a.pred[j];
    if (i < 0) return;
    const int idx = a.segnum[j] - 1;
    if (idx < 0 || idx >= a.nseg || i > j) return;    // (cannot be: the buffers are sized by the scan's total)
    FlSums sm{0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long long fi = a.frames[i], xi = a.qx[i], yi = a.qy[i];
    int near = 0;
    for (int r = i; r <= j; ++r) {
        if (!(a.rf[r] & EAGLE_FLIGHT_ROW_USED)) continue;
        fl_add(sm, a.frames[r] - fi, a.qx[r] - xi, a.qy[r] - yi);
        near += a.cand[r] >= 0;
    }
    double4 fit;
    const long long c = fl_solve(sm, fit);
    const double t1 = (double)(a.frames[j] - fi);
    EagleBallFlight o{};
    o.row0 = i; o.row1 = j; o.used = (int)sm.S0; o.spikes = (j - i + 1) - (int)sm.S0; o.near = near;
    o.x0 = (((double)xi + fit.x) + fit.y * 0.0) / FL_Q; o.y0 = (((double)yi + fit.z) + fit.w * 0.0) / FL_Q;
    o.x1 = (((double)xi + fit.x) + fit.y * t1) / FL_Q; o.y1 = (((double)yi + fit.z) + fit.w * t1) / FL_Q;
    o.vx = (fit.y * a.fps) / FL_Q; o.vy = (fit.w * a.fps) / FL_Q;
    o.speed = sqrt(o.vx * o.vx + o.vy * o.vy);
    o.rms = sqrt((double)c / (double)sm.S0) / FL_Q;
    o.c = c;
    o.kind = o.speed < a.still_speed ? EAGLE_FLIGHT_STILL : 2 * near > o.used ? EAGLE_FLIGHT_CARRIED : EAGLE_FLIGHT_FREE;
    o.flags = j - i == a.L ? EAGLE_FLIGHT_CAPPED : 0;
    o.shot = -1;                                       // not evaluated (the totals kernel counts the others and makes it 0)
    o.y_cross = fl_nan();
    if (o.kind == EAGLE_FLIGHT_FREE && o.speed >= a.shot_speed && o.vx != 0.0) {
        const double X = o.vx > 0.0 ? 105.0 : 0.0;
        const double s = (X - o.x0) / o.vx;
        o.y_cross = o.y0 + o.vy * s;
        const double reach = o.speed * s;
        o.shot = 0;
        if (reach >= 0.0 && reach <= a.shot_range) {
            const double off = fabs(o.y_cross - 34.0);
            o.shot = off <= 3.66 ? 2 : off <= 3.66 + a.shot_margin ? 1 : 0;
        }
    }
    a.flights[idx] = o;
    a.segfit[idx] = fit;
}

__device__ __forceinline__ int fl_wave_sum(int v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// nseg == 0: every row is without a segment
__global__ __launch_bounds__(256) void flights_rows_kernel(FlArgs a)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    const int rf = a.rf[r];
    const bool islast = r + 1 >= a.rows || a.head[r + 1];
    const bool hasseg = (rf & EAGLE_FLIGHT_ROW_PRESENT) && (!a.head[r] || !islast);
    int seg = -1, fl = rf;
    double2 p = make_double2(fl_nan(), fl_nan()), v = p;
    if (hasseg && a.nseg > 0) {
        seg = a.segnum[r] - (islast ? 1 : 0);
        if (seg < 0 || seg >= a.nseg) seg = 0;         // (cannot be: a row of a run with a segment lies in one)
        const EagleBallFlight* F = a.flights + seg;
        const double4 fit = a.segfit[seg];
        const int i = F->row0;
        const double t = (double)((long long)a.frames[r] - a.frames[i]);
        p = make_double2((((double)a.qx[i] + fit.x) + fit.y * t) / FL_Q, (((double)a.qy[i] + fit.z) + fit.w * t) / FL_Q);
        v = make_double2(F->vx, F->vy);
        if (a.mark[r] && a.pred[r] >= 0 && !islast && seg >= 1) {  // a knot: segments seg - 1 and seg meet here
            const EagleBallFlight* I = a.flights + (seg - 1);
            const double dvx = F->vx - I->vx, dvy = F->vy - I->vy;
            const double dv = sqrt(dvx * dvx + dvy * dvy);
            fl |= EAGLE_FLIGHT_ROW_KNOT;
            if (dv >= a.kick_dv) { fl |= EAGLE_FLIGHT_ROW_KICK; a.kickflag[r] = 1; }
            else a.flights[seg - 1].flags |= EAGLE_FLIGHT_CONTINUES;       // this thread alone writes the word after the fit kernel
        }
    }
    a.seg[r] = seg; a.flags[r] = (uint8_t)fl; a.fitted[r] = p; a.velocity[r] = v;
}

__global__ __launch_bounds__(256) void flights_kicks_kernel(FlArgs a)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.nkick) return;
    const int r = a.kicklist[e], seg = a.seg[r];
    if (seg < 1 || seg >= a.nseg) return;
    const EagleBallFlight *I = a.flights + (seg - 1), *F = a.flights + seg;
    EagleBallKick o{};
    o.row = r; o.seg_in = seg - 1; o.seg_out = seg; o.col = a.cand[r];
    o.speed_in = I->speed; o.speed_out = F->speed;
    const double dvx = F->vx - I->vx, dvy = F->vy - I->vy;
    o.dv = sqrt(dvx * dvx + dvy * dvy);
    o.cos_turn = (o.speed_in == 0.0 || o.speed_out == 0.0) ? fl_nan() : (I->vx * F->vx + I->vy * F->vy) / (o.speed_in * o.speed_out);
    a.kicks[e] = o;
}

// one thread per row and, with the same index, per segment
__global__ __launch_bounds__(256) void flights_totals_kernel(FlArgs a)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int fl = r < a.rows ? a.flags[r] : 0;
    const int runs = fl_wave_sum(r < a.rows && (fl & EAGLE_FLIGHT_ROW_PRESENT) && a.head[r]);
    const int spikes = fl_wave_sum((fl & EAGLE_FLIGHT_ROW_SPIKE) != 0), knots = fl_wave_sum((fl & EAGLE_FLIGHT_ROW_KNOT) != 0);
    EagleFlightTotals* T = a.totals;
    if ((threadIdx.x & 63) == 0) {
        if (runs) atomicAdd(&T->runs, runs);
        if (spikes) atomicAdd(&T->spikes, spikes);
        if (knots) atomicAdd(&T->knots, knots);
    }
    if (r < a.nseg) {
        EagleBallFlight* F = a.flights + r;
        atomicAdd(&T->kinds[F->kind], 1);
        if (F->shot >= 0) atomicAdd(&T->shots[F->shot], 1); else F->shot = 0;
        if (F->flags & EAGLE_FLIGHT_CAPPED) atomicAdd(&T->capped, 1);
        if (F->c) atomicAdd((unsigned long long*)&T->sum_c, (unsigned long long)F->c);
    }
    if (r == 0) { T->flights = a.nseg; T->kicks = a.nkick; }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct FlResolved { long long T, lam; };

static FlResolved flights_check(const char* who, const EagleFlightParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: params is NULL", who);
    if (!(std::isfinite(p->fps) && p->fps > 0.0)) fail(EAGLE_E_INVALID, "%s: fps %g must be finite and positive", who, p->fps);
    if (p->max_gap < 1 || p->max_gap > 1024) fail(EAGLE_E_INVALID, "%s: max_gap %d is outside 1 .. 1024", who, p->max_gap);
    if (p->max_rows < 2 || p->max_rows > FL_LMAX) fail(EAGLE_E_INVALID, "%s: max_rows %d is outside 2 .. %d", who, p->max_rows, FL_LMAX);
    const double lim[2] = {p->noise, p->spike};
    static const char* const lim_names[2] = {"noise", "spike"};
    for (int k = 0; k < 2; ++k)
        if (!(std::isfinite(lim[k]) && lim[k] >= 0.0 && lim[k] <= 1024.0)) fail(EAGLE_E_INVALID, "%s: %s %g must be finite and within [0, 1024] m", who, lim_names[k], lim[k]);
    const double pos[6] = {p->penalty, p->kick_dv, p->still_speed, p->shot_speed, p->shot_range, p->shot_margin};
    static const char* const pos_names[6] = {"penalty", "kick_dv", "still_speed", "shot_speed", "shot_range", "shot_margin"};
    for (int k = 0; k < 6; ++k)
        if (!(std::isfinite(pos[k]) && pos[k] >= 0.0)) fail(EAGLE_E_INVALID, "%s: %s %g must be finite and not negative", who, pos_names[k], pos[k]);
    if (!(p->radius > 0.0 && p->radius <= 1024.0)) fail(EAGLE_E_INVALID, "%s: radius %g must be positive and at most 1024 m", who, p->radius);
    if (p->layout < EAGLE_FLIGHT_LAYOUT_DEFAULT || p->layout > EAGLE_FLIGHT_LAYOUT_K_MAJOR) fail(EAGLE_E_INVALID, "%s: layout %d is no EAGLE_FLIGHT_LAYOUT_*", who, p->layout);
    if (p->reserved) fail(EAGLE_E_INVALID, "%s: the reserved word of the parameters is %d, not 0", who, p->reserved);
    const double nq = p->noise * FL_Q;
    const double lam = p->penalty * (nq * nq);
    if (!(lam <= FL_CAP)) fail(EAGLE_E_INVALID, "%s: penalty %g times (noise %g * 1024)^2 exceeds 2^40", who, p->penalty, p->noise);
    FlResolved r;
    r.T = (long long)std::rint(p->spike * FL_Q);
    r.lam = (long long)std::rint(lam);
    return r;
}

struct FlCols { std::vector<int32_t> persons; int ball = -1; };

static FlCols flights_columns(const char* who, const EaglePostColumn* columns, int ncols, bool no_ball)
{
    FlCols fc;
    for (int c = 0; c < ncols; ++c) {
        const EaglePostColumn& col = columns[c];
        if (col.kind != EAGLE_POST_PLAYER && col.kind != EAGLE_POST_GOALKEEPER && col.kind != EAGLE_POST_BALL && col.kind != EAGLE_POST_BOUNDARY)
            fail(EAGLE_E_INVALID, "%s: column %d is of unknown kind %d", who, c, col.kind);
        if (col.video) continue;
        if (col.kind == EAGLE_POST_BALL) {
            if (fc.ball >= 0) fail(EAGLE_E_INVALID, "%s: columns %d and %d are both the ball", who, fc.ball, c);
            fc.ball = c;
        } else if (col.kind == EAGLE_POST_PLAYER || col.kind == EAGLE_POST_GOALKEEPER) fc.persons.push_back(c);
    }
    if (no_ball) fc.ball = -1;
    return fc;
}

static void flights_cuts_check(const char* who, const int32_t* cuts, int n_cuts)
{
    if (n_cuts < 0 || (n_cuts > 0 && !cuts)) fail(EAGLE_E_INVALID, "%s: %d cuts at %p", who, n_cuts, (const void*)cuts);
    for (int k = 1; k < n_cuts; ++k)
        if (cuts[k] <= cuts[k - 1]) fail(EAGLE_E_INVALID, "%s: cut %d (frame %d) does not lie behind cut %d (frame %d)", who, k, cuts[k], k - 1, cuts[k - 1]);
}

static size_t fl_up(size_t b) { return (std::max<size_t>(b, 16) + 255) & ~(size_t)255; }

// What a call keeps: seg i32 [rows] | flags u8 [rows] | fitted f64 [rows][2] | velocity f64 [rows][2], each from a 256-byte boundary
struct FlKept { size_t seg, flags, fitted, velocity, total; };

static FlKept flights_kept(size_t rows)
{
    FlKept o{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += fl_up(b); return was; };
    o.seg = take(rows * 4); o.flags = take(rows); o.fitted = take(rows * 16); o.velocity = take(rows * 16);
    o.total = at;
    return o;
}

static int fl_rounds(int rows)                         // tables 0 .. K - 1 reach 2^K - 1 >= any path's length
{
    int K = 1;
    while ((1ll << K) < (long long)rows) ++K;
    return K;
}

struct FlResult { std::vector<EagleBallFlight> flights; std::vector<EagleBallKick> kicks; EagleFlightTotals totals{}; };

// rows > 0.  d_values: the table; kept: flights_kept's block (written whole).  Returns when everything is complete.
static void flights_run(EagleHandle* h, const char* who, const FlCols& fc, const double2* d_values, const int32_t* d_frames, int rows, const int32_t* cuts, int n_cuts,
                        const EagleFlightParams* p, const FlResolved& rs, int64_t max_bytes, uint8_t* kept, FlResult& res, hipStream_t s, float* times_ms)
{
    const size_t n = (size_t)rows, L = (size_t)p->max_rows;
    const int K = fl_rounds(rows);
    const FlKept KP = flights_kept(n);
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += fl_up(b); return was; };
    const size_t o_persons = take(fc.persons.size() * 4), o_cuts = take((size_t)n_cuts * 4), o_qx = take(n * 4), o_qy = take(n * 4), o_cand = take(n * 4),
                 o_head = take(n), o_rf = take(n), o_runflag = take(n * 4), o_runlist = take(n * 4), o_segnum = take(n * 4), o_kicklist = take(n * 4),
                 o_jump = take((size_t)(K - 1) * n * 4), o_c = take(n * L * 8), o_pred = take(n * 4), o_zero = at;
    const size_t o_mark = take(n * 4), o_kickflag = take(n * 4), o_counts = take(16), o_totals = take(sizeof(EagleFlightTotals)), total = at;
    // per segment: at most rows - 1 of them
    const size_t seg_bytes = fl_up(n * sizeof(EagleBallFlight)) + fl_up(n * sizeof(double4)) + fl_up(n * sizeof(EagleBallKick));
    double budget = (double)max_bytes;
    if (max_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = 0.9 * (double)free_b;
    }
    if ((double)total + (double)seg_bytes > budget)
        fail(EAGLE_E_INVALID, "%s: %d rows with max_rows %d need %.0f bytes of device memory, the budget is %.0f", who, rows, p->max_rows, (double)total + (double)seg_bytes, budget);
    uint8_t *d = nullptr, *d2 = nullptr;
    hipEvent_t ev[12] = {};
    try {
        HIP_CHECK(hipMalloc((void**)&d, total));
        FlArgs a{};
        a.values = d_values; a.frames = d_frames; a.persons = (const int32_t*)(d + o_persons); a.cuts = (const int32_t*)(d + o_cuts);
        a.rows = rows; a.npersons = (int)fc.persons.size(); a.ball = fc.ball; a.n_cuts = n_cuts; a.L = p->max_rows; a.max_gap = p->max_gap;
        a.kmajor = p->layout != EAGLE_FLIGHT_LAYOUT_END_MAJOR;        // the default is k-major: docs/experiments.md, "Ball flights (K40)"
        a.T = rs.T; a.lam = rs.lam;
        a.r2 = p->radius * p->radius; a.fps = p->fps; a.kick_dv = p->kick_dv; a.still_speed = p->still_speed; a.shot_speed = p->shot_speed;
        a.shot_range = p->shot_range; a.shot_margin = p->shot_margin;
        a.qx = (int32_t*)(d + o_qx); a.qy = (int32_t*)(d + o_qy); a.cand = (int32_t*)(d + o_cand); a.pred = (int32_t*)(d + o_pred); a.mark = (int32_t*)(d + o_mark);
        a.jump = (int32_t*)(d + o_jump); a.runflag = (int32_t*)(d + o_runflag); a.runlist = (int32_t*)(d + o_runlist); a.segnum = (int32_t*)(d + o_segnum);
        a.kickflag = (int32_t*)(d + o_kickflag); a.kicklist = (int32_t*)(d + o_kicklist); a.head = d + o_head; a.rf = d + o_rf; a.c = (long long*)(d + o_c);
        a.counts = (int32_t*)(d + o_counts); a.totals = (EagleFlightTotals*)(d + o_totals);
        a.seg = (int32_t*)(kept + KP.seg); a.flags = kept + KP.flags; a.fitted = (double2*)(kept + KP.fitted); a.velocity = (double2*)(kept + KP.velocity);
        if (!fc.persons.empty()) HIP_CHECK(hipMemcpyAsync(d + o_persons, fc.persons.data(), fc.persons.size() * 4, hipMemcpyHostToDevice, s));
        if (n_cuts) HIP_CHECK(hipMemcpyAsync(d + o_cuts, cuts, (size_t)n_cuts * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(d + o_pred, 0xff, fl_up(n * 4), s));                  // pred = -1: no predecessor
        HIP_CHECK(hipMemsetAsync(d + o_zero, 0, total - o_zero, s));
        if (times_ms)
            for (hipEvent_t& e : ev) HIP_CHECK(hipEventCreate(&e));
        auto stamp = [&](int k) { if (times_ms) HIP_CHECK(hipEventRecord(ev[k], s)); };
        auto run = [&](const char* name, double bytes, const std::function<void()>& fn) {
            if (h) timed_launch(h, name, bytes, s, fn); else fn();
            HIP_CHECK(hipGetLastError());
        };
        const unsigned gt = (unsigned)((rows + FL_TILE - 1) / FL_TILE), gr = (unsigned)((rows + 255) / 256);
        const double dn = (double)rows;
        int32_t counts[3] = {0, 0, 0};
        stamp(0);
        run("flights_prepare", dn * (20.0 + (fc.ball >= 0 ? 16.0 * (1.0 + (double)fc.persons.size()) : 0.0) + 18.0),
            [&] { hipLaunchKernelGGL(flights_prepare_kernel, dim3(gt), dim3(FL_TILE), 0, s, a); });
        run("flights_scan", 12.0 * dn, [&] { hipLaunchKernelGGL(flights_scan_kernel, dim3(1), dim3(1024), 0, s, a.runflag, rows, a.runlist, a.counts); });
        stamp(1);
        HIP_CHECK(hipMemcpyAsync(&counts[0], a.counts, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const int nruns = counts[0];
        if (nruns < 0 || nruns > rows) fail(EAGLE_E_HIP, "%s: %d runs from %d rows", who, nruns, rows);
        if (nruns) {
            stamp(2);
            run("flights_cost", dn * (14.0 + 8.0 * (double)L), [&] { hipLaunchKernelGGL(flights_cost_kernel, dim3(gt), dim3(FL_TILE), 0, s, a); });
            stamp(3);
            stamp(4);
            run("flights_walk", dn * (6.0 + 8.0 * (double)L), [&] { hipLaunchKernelGGL(flights_walk_kernel, dim3((unsigned)std::min(nruns, 4096)), dim3(64), 0, s, a, nruns); });
            stamp(5);
            stamp(6);
            run("flights_path", dn * (12.0 * (K - 1) + 8.0 * K + 24.0), [&] {
                for (int k = 1; k < K; ++k)
                    hipLaunchKernelGGL(flights_double_kernel, dim3(gr), dim3(256), 0, s, k == 1 ? a.pred : a.jump + (size_t)(k - 2) * n, a.jump + (size_t)(k - 1) * n, rows);
                for (int k = K - 1; k >= 0; --k)
                    hipLaunchKernelGGL(flights_mark_kernel, dim3(gr), dim3(256), 0, s, k == 0 ? a.pred : a.jump + (size_t)(k - 1) * n, a.mark, rows);
                hipLaunchKernelGGL(flights_segend_kernel, dim3(gr), dim3(256), 0, s, a);
                hipLaunchKernelGGL(flights_scan_kernel, dim3(1), dim3(1024), 0, s, a.segnum, rows, (int32_t*)nullptr, a.counts + 1);
            });
            stamp(7);
            HIP_CHECK(hipMemcpyAsync(&counts[1], a.counts + 1, 4, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
        const int nseg = counts[1];
        if (nseg < 0 || nseg >= std::max(rows, 1)) fail(EAGLE_E_HIP, "%s: %d segments from %d rows", who, nseg, rows);
        if (nseg) {
            const size_t b_fl = fl_up((size_t)nseg * sizeof(EagleBallFlight)), b_fit = fl_up((size_t)nseg * sizeof(double4));
            HIP_CHECK(hipMalloc((void**)&d2, b_fl + b_fit + fl_up((size_t)nseg * sizeof(EagleBallKick))));
            a.flights = (EagleBallFlight*)d2; a.segfit = (double4*)(d2 + b_fl); a.kicks = (EagleBallKick*)(d2 + b_fl + b_fit);
            a.nseg = nseg;
            stamp(8);
            run("flights_fit", 25.0 * dn + 144.0 * nseg, [&] { hipLaunchKernelGGL(flights_fit_kernel, dim3(gr), dim3(256), 0, s, a); });
            stamp(9);
        }
        stamp(10);
        run("flights_rows", 60.0 * dn, [&] {
            hipLaunchKernelGGL(flights_rows_kernel, dim3(gr), dim3(256), 0, s, a);
            hipLaunchKernelGGL(flights_scan_kernel, dim3(1), dim3(1024), 0, s, a.kickflag, rows, a.kicklist, a.counts + 2);
        });
        HIP_CHECK(hipMemcpyAsync(&counts[2], a.counts + 2, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const int nkick = counts[2];
        if (nkick < 0 || nkick > std::max(nseg - 1, 0)) fail(EAGLE_E_HIP, "%s: %d kicks from %d segments", who, nkick, nseg);
        a.nkick = nkick;
        run("flights_events", 2.0 * dn + 48.0 * nkick + 112.0 * nseg, [&] {
            if (nkick) hipLaunchKernelGGL(flights_kicks_kernel, dim3((unsigned)((nkick + 255) / 256)), dim3(256), 0, s, a);
            hipLaunchKernelGGL(flights_totals_kernel, dim3(gr), dim3(256), 0, s, a);
        });
        stamp(11);
        res.flights.assign((size_t)nseg, EagleBallFlight{});
        res.kicks.assign((size_t)nkick, EagleBallKick{});
        if (nseg) HIP_CHECK(hipMemcpyAsync(res.flights.data(), a.flights, (size_t)nseg * sizeof(EagleBallFlight), hipMemcpyDeviceToHost, s));
        if (nkick) HIP_CHECK(hipMemcpyAsync(res.kicks.data(), a.kicks, (size_t)nkick * sizeof(EagleBallKick), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(&res.totals, a.totals, sizeof(EagleFlightTotals), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h && h->prof) collect_spans(h);
        if (times_ms) {
            std::fill(times_ms, times_ms + EAGLE_FLIGHT_TIMES, 0.0f);
            HIP_CHECK(hipEventElapsedTime(&times_ms[0], ev[0], ev[1]));
            if (nruns)
                for (int k = 1; k <= 3; ++k) HIP_CHECK(hipEventElapsedTime(&times_ms[k], ev[2 * k], ev[2 * k + 1]));
            if (nseg) HIP_CHECK(hipEventElapsedTime(&times_ms[4], ev[8], ev[9]));
            HIP_CHECK(hipEventElapsedTime(&times_ms[5], ev[10], ev[11]));
            HIP_CHECK(hipEventElapsedTime(&times_ms[6], ev[0], ev[11]));
        }
    } catch (...) {
        (void)hipStreamSynchronize(s);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (d2) (void)hipFree(d2);
        if (d) (void)hipFree(d);
        throw;
    }
    for (hipEvent_t e : ev) if (e) HIP_CHECK(hipEventDestroy(e));
    if (d2) HIP_CHECK(hipFree(d2));
    HIP_CHECK(hipFree(d));
}

}  // namespace eagle

extern "C" {

int eagle_flight_params_default(EagleFlightParams* p, double fps, int32_t max_gap)
{
    if (!p) return EAGLE_E_INVALID;
    *p = EagleFlightParams{};
    p->fps = fps; p->max_gap = max_gap; p->max_rows = 64;
    p->noise = 0.25; p->penalty = 16.0; p->spike = 1.0; p->kick_dv = 3.0; p->radius = 2.0; p->still_speed = 0.5;
    p->shot_speed = 10.0; p->shot_range = 40.0; p->shot_margin = 2.0;
    return EAGLE_OK;
}

int eagle_post_ball_flights(EagleHandle* h, EaglePostTable* t, const EagleFlightParams* p, const int32_t* cuts, int n_cuts)
{
    API_BEGIN_H(h)
    const char* who = "eagle_post_ball_flights";
    if (!t) fail(EAGLE_E_INVALID, "%s: table is NULL", who);
    if (t->h != h) fail(EAGLE_E_INVALID, "%s: the table belongs to another handle", who);
    const FlResolved rs = flights_check(who, p);
    flights_cuts_check(who, cuts, n_cuts);
    const FlCols fc = flights_columns(who, t->columns.data(), t->cols, (t->flags & EAGLE_POST_NO_BALL) != 0);
    if (t->rows > FL_MAX_ROWS) fail(EAGLE_E_INVALID, "%s: %d rows, at most %d", who, t->rows, FL_MAX_ROWS);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)t->rows;
    FlResult res;
    if (rows) {
        const hipStream_t s = h->s_main;
        int32_t* d_frames = nullptr;
        uint8_t* kept = nullptr;
        try {
            HIP_CHECK(hipMalloc((void**)&d_frames, rows * 4));
            HIP_CHECK(hipMalloc((void**)&kept, flights_kept(rows).total));
            HIP_CHECK(hipMemcpyAsync(d_frames, t->frames.data(), rows * 4, hipMemcpyHostToDevice, s));
            flights_run(h, who, fc, (const double2*)t->d_values, d_frames, t->rows, cuts, n_cuts, p, rs, t->max_bytes, kept, res, s, nullptr);
        } catch (...) {
            (void)hipStreamSynchronize(s);
            if (d_frames) (void)hipFree(d_frames);
            if (kept) (void)hipFree(kept);
            throw;
        }
        HIP_CHECK(hipFree(d_frames));
        if (t->d_flights) HIP_CHECK(hipFree(t->d_flights));         // a later call replaces the result
        t->d_flights = kept;
    }
    t->flights.swap(res.flights); t->kicks.swap(res.kicks); t->flight_totals = res.totals;
    t->has_flights = true;
    API_END(h)
}

int eagle_post_ball_flight_values(EaglePostTable* t, int32_t* seg, uint8_t* flags, double* fitted, double* velocity, EagleFlightTotals* totals)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->has_flights) fail(EAGLE_E_INVALID, "eagle_post_ball_flight_values: the table has no ball flights (eagle_post_ball_flights)");
    const size_t rows = (size_t)t->rows;
    if (rows) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        const FlKept L = flights_kept(rows);
        const uint8_t* d = (const uint8_t*)t->d_flights;
        if (seg) HIP_CHECK(hipMemcpy(seg, d + L.seg, rows * 4, hipMemcpyDeviceToHost));
        if (flags) HIP_CHECK(hipMemcpy(flags, d + L.flags, rows, hipMemcpyDeviceToHost));
        if (fitted) HIP_CHECK(hipMemcpy(fitted, d + L.fitted, rows * 16, hipMemcpyDeviceToHost));
        if (velocity) HIP_CHECK(hipMemcpy(velocity, d + L.velocity, rows * 16, hipMemcpyDeviceToHost));
    }
    if (totals) *totals = t->flight_totals;
    API_END(h)
}

int eagle_post_ball_flight_records(const EaglePostTable* t, EagleBallFlight* flights, int cap, int* n)
{
    if (!t || !n || cap < 0 || (cap > 0 && !flights) || !t->has_flights) return EAGLE_E_INVALID;
    *n = (int)t->flights.size();
    std::copy(t->flights.begin(), t->flights.begin() + std::min<size_t>(cap, t->flights.size()), flights);
    return EAGLE_OK;
}

int eagle_post_ball_kicks(const EaglePostTable* t, EagleBallKick* kicks, int cap, int* n)
{
    if (!t || !n || cap < 0 || (cap > 0 && !kicks) || !t->has_flights) return EAGLE_E_INVALID;
    *n = (int)t->kicks.size();
    std::copy(t->kicks.begin(), t->kicks.begin() + std::min<size_t>(cap, t->kicks.size()), kicks);
    return EAGLE_OK;
}

int eagle_post_device_ball_flights(const EaglePostTable* t, const int32_t** d_seg, const uint8_t** d_flags, const double** d_fitted, const double** d_velocity)
{
    if (!t || !d_seg || !d_flags || !d_fitted || !d_velocity) return EAGLE_E_INVALID;
    const uint8_t* d = t->has_flights && t->rows > 0 ? (const uint8_t*)t->d_flights : nullptr;
    const FlKept L = flights_kept((size_t)t->rows);
    *d_seg = d ? (const int32_t*)(d + L.seg) : nullptr;
    *d_flags = d ? d + L.flags : nullptr;
    *d_fitted = d ? (const double*)(d + L.fitted) : nullptr;
    *d_velocity = d ? (const double*)(d + L.velocity) : nullptr;
    return EAGLE_OK;
}

int eagle_op_ball_flights(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* cuts,
                          int n_cuts, const EagleFlightParams* p, int32_t* seg, uint8_t* flags, double* fitted, double* velocity, EagleBallFlight* flights,
                          int cap_flights, int* n_flights, EagleBallKick* kicks, int cap_kicks, int* n_kicks, EagleFlightTotals* totals, float* times_ms)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_ball_flights";
    if (rows < 0 || cols < 0 || rows > FL_MAX_ROWS || (rows > 0 && !frames) || (cols > 0 && !columns) || (rows > 0 && cols > 0 && !values) || cap_flights < 0 || cap_kicks < 0 ||
        (cap_flights > 0 && !flights) || (cap_kicks > 0 && !kicks))
        fail(EAGLE_E_INVALID, "%s: bad argument (values %p, frames %p, columns %p, %d rows of at most %d, %d columns, flights %p cap %d, kicks %p cap %d)", who, (const void*)values,
             (const void*)frames, (const void*)columns, rows, FL_MAX_ROWS, cols, (const void*)flights, cap_flights, (const void*)kicks, cap_kicks);
    const FlResolved rs = flights_check(who, p);
    flights_cuts_check(who, cuts, n_cuts);
    const FlCols fc = flights_columns(who, columns, cols, false);
    for (int r = 1; r < rows; ++r)
        if (frames[r] <= frames[r - 1]) fail(EAGLE_E_INVALID, "%s: frame numbers must ascend (row %d: %d after %d)", who, r, frames[r], frames[r - 1]);
    FlResult res;
    float times[EAGLE_FLIGHT_TIMES] = {};
    if (rows) {
        HIP_CHECK(hipSetDevice(device));
        Net net;
        const size_t n = (size_t)rows;
        const FlKept L = flights_kept(n);
        const double2* d_v = (const double2*)net.upload(values ? (const void*)values : (const void*)frames, values ? (size_t)cols * n * 16 : 0);
        const int32_t* d_f = (const int32_t*)net.upload(frames, n * 4);
        uint8_t* kept = (uint8_t*)net.get(L.total);
        flights_run(nullptr, who, fc, d_v, d_f, rows, cuts, n_cuts, p, rs, 0, kept, res, nullptr, times_ms ? times : nullptr);
        if (seg) HIP_CHECK(hipMemcpy(seg, kept + L.seg, n * 4, hipMemcpyDeviceToHost));
        if (flags) HIP_CHECK(hipMemcpy(flags, kept + L.flags, n, hipMemcpyDeviceToHost));
        if (fitted) HIP_CHECK(hipMemcpy(fitted, kept + L.fitted, n * 16, hipMemcpyDeviceToHost));
        if (velocity) HIP_CHECK(hipMemcpy(velocity, kept + L.velocity, n * 16, hipMemcpyDeviceToHost));
    }
    if (flights) std::copy(res.flights.begin(), res.flights.begin() + std::min<size_t>(cap_flights, res.flights.size()), flights);
    if (kicks) std::copy(res.kicks.begin(), res.kicks.begin() + std::min<size_t>(cap_kicks, res.kicks.size()), kicks);
    if (n_flights) *n_flights = (int)res.flights.size();
    if (n_kicks) *n_kicks = (int)res.kicks.size();
    if (totals) *totals = res.totals;
    if (times_ms) std::copy(times, times + EAGLE_FLIGHT_TIMES, times_ms);
    API_END(hh)
}

}  // extern "C"
