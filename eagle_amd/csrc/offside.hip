// K33 — offside: a processed table resident in HBM (post.hip) -> per row and attacking group the offside line (the second-last opponent, the halfway
// line or the ball, whichever is deepest) and every attacker's margin beyond it, per member the totals over the clip, per pass event a verdict about the
// receiver at the moment of release (include/eagle.h, eagle_post_offside / eagle_op_offside; tests/offside_ref.py is the written definition of every
// bit).  Members of groups 0 and 1 and the quantisation are K26's (shape_columns; q = floor(x * 1024 + 0.5)); the goalkeepers are listed as group 2.
// Integers after that: |qx| <= 2^20, a depth u = qx or 107520 - qx lies within +-2^21, a margin within +-2^22; a row's vote is the sign of sum_x0 n1 -
// sum_x1 n0 with sums <= 2^32 and counts <= 2^12.  Counts are added with integer atomics, extrema are taken under strict total orders, so no result depends
// on an order.  No floating point behind the quantisation.
//
//   offside_vote_kernel    one thread per row walks the member columns of both groups (a wave's load of a column is one run of 1024 bytes) and forms
//                          the row's sign; a wave counts its signs with three ballots and lane 0 adds the popcounts to the clip record.
//   offside_rows_kernel    one wave per (row, attacking group a).  Every wave resolves the direction from the clip record's counts (the launch is behind
//                          the vote on the stream); the wave of row 0, group 0 stores it.  The lanes stride over the listed columns 64 at a time: a
//                          defender (a present member of 1 - a, or a present keeper beyond the halfway line) enters the lane's top two (u, column) under
//                          DEEPER (greater u, of equal u the earlier column: a strict total order, the columns being distinct), a butterfly of
//                          __shfl_xor merges the lanes' pairs into the multiset's top two (the partners' sets are disjoint at every step).  Then the
//                          line, and a second walk writes the margins of a's members and takes n_off and the greatest margin (earliest column) the same
//                          way.  Every int32 of the margins is written by exactly one wave, NONE where there is no margin.
//   offside_totals_kernel  one workgroup per member: the threads stride along the member's margins (coalesced), a butterfly and four LDS slots reduce.
//   offside_events_kernel  one thread per event: the receiver's margin and its group's record at the release row, the verdict, and a walk over the
//                          opponents for the ones the pass takes out of the game.
#include "trails.h"

namespace eagle {

static constexpr int OF_NONE = EAGLE_OFFSIDE_NONE, OF_UMAX = EAGLE_OFFSIDE_U_MAX, OF_UHALF = EAGLE_OFFSIDE_U_HALF;
static constexpr int OF_NOCOL = 0x7fffffff;            // the column of an empty top-two slot: loses every comparison together with u = OF_NONE
typedef unsigned long long of_u64;
static_assert(sizeof(EagleOffsideParams) == 32 && sizeof(EagleOffsideRow) == 48 && sizeof(EagleOffsideTotals) == 32 && sizeof(EagleOffsideEvent) == 32 &&
              sizeof(EagleOffsideClip) == 32 && sizeof(EaglePossessionEvent) == 80, "include/eagle.h states these sizes");
static_assert(OF_UMAX == 105 * 1024 && OF_UHALF * 2 == OF_UMAX, "the pitch is 105 m long");

struct OfArgs {
    const double2* values;       // [column][row]
    const int4* list;            // the members and keepers in table order: {column, group (2: keeper), member index in group order (keeper: -1), 0}
    const int32_t* gcols;        // group 0's columns in table order, then group 1's: member index -> column
    const int32_t* member_of;    // [table columns]: the member's index in group order, or -1
    int rows, nl, n0, n1, ball;  // the table's rows; list entries; members per group; the ball's column or -1
    int requested, assume, tq;   // EagleOffsideParams
    EagleOffsideRow* rows_out;   // [rows][2]
    int32_t* margins;            // [n0 + n1][rows]
    EagleOffsideTotals* totals;  // [n0 + n1], preset (col, group)
    EagleOffsideClip* clip;      // preset (requested, n_members, n_keepers), counts zero
    const EaglePossessionEvent* events;
    EagleOffsideEvent* events_out;
    int n_events;
};

__device__ __forceinline__ bool of_quantise(double2 v, int& qx)
{
    if (!(fabs(v.x) <= MM_DOMAIN) || !(fabs(v.y) <= MM_DOMAIN)) return false;          // NaN, +-inf and the far field: K26's rule
    qx = (int)floor(v.x * 1024.0 + 0.5);
    return true;
}

// the contract's vote: neg > pos, group 0 stands on the left and attacks right
__device__ __forceinline__ int of_direction(int requested, const EagleOffsideClip* c)
{
    if (requested != EAGLE_OFFSIDE_DIR_AUTO) return requested;
    const int neg = c->neg, pos = c->pos;
    return neg > pos ? EAGLE_OFFSIDE_DIR_RIGHT : pos > neg ? EAGLE_OFFSIDE_DIR_LEFT : 0;
}

// group a attacks towards x = 105
__device__ __forceinline__ bool of_right(int dir, int a) { return (dir == EAGLE_OFFSIDE_DIR_RIGHT) == (a == 0); }

// DEEPER: (u, c) stands in front of (v, d) in the order of depths
__device__ __forceinline__ bool of_deeper(int u, int c, int v, int d) { return u > v || (u == v && c < d); }

__device__ __forceinline__ void of_push(int u, int c, int& u1, int& c1, int& u2, int& c2)
{
    const bool first = of_deeper(u, c, u1, c1), second = of_deeper(u, c, u2, c2);      // (selects: the pairs stay in registers)
    u2 = first ? u1 : second ? u : u2; c2 = first ? c1 : second ? c : c2;
    u1 = first ? u : u1; c1 = first ? c : c1;
}

__global__ __launch_bounds__(256) void offside_vote_kernel(OfArgs a)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    int s = 2;                                                           // 2: the row has no vote
    if (r < a.rows) {
        long long sx[2] = {0, 0};
        int n[2] = {0, 0};
        for (int k = 0; k < a.n0 + a.n1; ++k) {
            int qx;
            if (!of_quantise(a.values[(size_t)a.gcols[k] * a.rows + r], qx)) continue;       // (gcols[k]: uniform)
            const int g = k < a.n0 ? 0 : 1;
            sx[g] += qx; ++n[g];
        }
        if (n[0] && n[1]) {
            const long long v = sx[0] * n[1] - sx[1] * n[0];                                 // < 2^45
            s = v < 0 ? -1 : v > 0 ? 1 : 0;
        }
    }
    const of_u64 bn = __ballot(s == -1), bp = __ballot(s == 1), bz = __ballot(s == 0);
    if ((threadIdx.x & 63) == 0) {
        if (bn) atomicAdd(&a.clip->neg, __popcll(bn));
        if (bp) atomicAdd(&a.clip->pos, __popcll(bp));
        if (bz) atomicAdd(&a.clip->zero, __popcll(bz));
    }
}

__global__ __launch_bounds__(256) void offside_rows_kernel(OfArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r = (int)(w >> 1), g = (int)(w & 1);                      // g: the attacking group
    if (r >= a.rows) return;                                             // (uniform over the wave; the kernel has no workgroup barrier)
    const int dir = of_direction(a.requested, a.clip);
    if (w == 0 && lane == 0) a.clip->direction = dir;
    const bool right = of_right(dir, g);
    int status = dir ? EAGLE_OFFSIDE_OK : EAGLE_OFFSIDE_NO_DIRECTION, flags = 0, line = 0, line_qx = 0, second_col = -1, natt = 0, ndef = 0, seen = 0;
    if (dir) {
        int u1 = OF_NONE, c1 = OF_NOCOL, u2 = OF_NONE, c2 = OF_NOCOL;
        for (int k = lane; k < a.nl; k += 64) {
            const int4 m = a.list[k];
            int qx;
            if (!of_quantise(a.values[(size_t)m.x * a.rows + r], qx)) continue;
            const int u = right ? qx : OF_UMAX - qx;
            if (m.y == g) { ++natt; continue; }
            if (m.y == 2) {
                if (u <= OF_UHALF) continue;                             // a keeper in the attackers' half or on the halfway line is nobody's
                ++seen;
            }
            ++ndef;
            of_push(u, m.x, u1, c1, u2, c2);
        }
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int v1 = __shfl_xor(u1, d, 64), d1 = __shfl_xor(c1, d, 64), v2 = __shfl_xor(u2, d, 64), d2 = __shfl_xor(c2, d, 64);
            of_push(v1, d1, u1, c1, u2, c2);
            of_push(v2, d2, u1, c1, u2, c2);
            natt += __shfl_xor(natt, d, 64); ndef += __shfl_xor(ndef, d, 64); seen += __shfl_xor(seen, d, 64);
        }
        const bool assumed = seen == 0 && a.assume != 0;
        if (ndef < (assumed ? 1 : 2)) {
            status = EAGLE_OFFSIDE_TOO_FEW;
        } else {
            const int second = assumed ? u1 : u2;
            second_col = assumed || u1 == u2 ? c1 : c2;                 // the earliest column at that depth
            int ub = 0;
            bool ball = false;
            if (a.ball >= 0) {
                int bq;
                ball = of_quantise(a.values[(size_t)a.ball * a.rows + r], bq);
                ub = right ? bq : OF_UMAX - bq;
            }
            line = second;
            int by = EAGLE_OFFSIDE_BY_DEFENDER;
            if (ball && ub > line) { line = ub; by = EAGLE_OFFSIDE_BY_BALL; }
            if (OF_UHALF > line) { line = OF_UHALF; by = EAGLE_OFFSIDE_BY_HALF; }
            flags = by | (assumed ? EAGLE_OFFSIDE_KEEPER_ASSUMED : 0) | (ball ? 0 : EAGLE_OFFSIDE_NO_BALL);
            line_qx = right ? line : OF_UMAX - line;
        }
    }
    const bool ok = status == EAGLE_OFFSIDE_OK;
    int mm = OF_NONE, mc = OF_NOCOL, noff = 0;
    for (int k = lane; k < a.nl; k += 64) {
        const int4 m = a.list[k];
        if (m.y != g) continue;
        int qx, mg = OF_NONE;
        if (ok && of_quantise(a.values[(size_t)m.x * a.rows + r], qx)) {
            mg = (right ? qx : OF_UMAX - qx) - line;
            noff += mg > 0 ? 1 : 0;
            if (of_deeper(mg, m.x, mm, mc)) { mm = mg; mc = m.x; }
        }
        a.margins[(size_t)m.z * a.rows + r] = mg;
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int vm = __shfl_xor(mm, d, 64), vc = __shfl_xor(mc, d, 64);
        if (of_deeper(vm, vc, mm, mc)) { mm = vm; mc = vc; }
        noff += __shfl_xor(noff, d, 64);
    }
    if (lane == 0) {
        EagleOffsideRow o{};
        o.status = status; o.flags = flags; o.line_qx = line_qx; o.second_col = second_col; o.n_att = natt; o.n_def = ndef; o.keepers_seen = seen; o.n_off = noff;
        o.max_margin = mc != OF_NOCOL ? mm : OF_NONE; o.max_col = mc != OF_NOCOL ? mc : -1;
        a.rows_out[(size_t)r * 2 + g] = o;
    }
}

__global__ __launch_bounds__(256) void offside_totals_kernel(OfArgs a)
{
    __shared__ int part[4][3];
    const int m = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t* M = a.margins + (size_t)m * a.rows;
    int n = 0, off = 0, mx = OF_NONE;
    for (int r = threadIdx.x; r < a.rows; r += 256) {
        const int v = M[r];
        if (v == OF_NONE) continue;
        ++n; off += v > 0 ? 1 : 0; mx = max(mx, v);
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        n += __shfl_xor(n, d, 64); off += __shfl_xor(off, d, 64); mx = max(mx, __shfl_xor(mx, d, 64));
    }
    if (lane == 0) { part[wave][0] = n; part[wave][1] = off; part[wave][2] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        EagleOffsideTotals* T = a.totals + m;
        T->rows = part[0][0] + part[1][0] + part[2][0] + part[3][0];
        T->off_rows = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        T->max_margin = max(max(part[0][2], part[1][2]), max(part[2][2], part[3][2]));
    }
}

__global__ __launch_bounds__(256) void offside_events_kernel(OfArgs a)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n_events) return;
    const EaglePossessionEvent ev = a.events[e];
    EagleOffsideEvent o{};
    o.margin = OF_NONE; o.bypassed = -1; o.group = -1;
    const int m = ev.kind == EAGLE_EVENT_PASS ? a.member_of[ev.to_col] : -1;            // (a pass event's columns and rows lie inside the table: the host's check)
    if (ev.kind != EAGLE_EVENT_PASS) {
        o.status = EAGLE_OFFSIDE_EV_NOT_PASS;
    } else if (m < 0) {
        o.status = EAGLE_OFFSIDE_EV_NO_RECEIVER;
    } else {
        const int g = m < a.n0 ? 0 : 1, r0 = ev.release_row, r1 = ev.receive_row;
        const EagleOffsideRow rec = a.rows_out[(size_t)r0 * 2 + g];
        const int mg = a.margins[(size_t)m * a.rows + r0];
        o.group = g;
        if (rec.status != EAGLE_OFFSIDE_OK || mg == OF_NONE) {
            o.status = EAGLE_OFFSIDE_EV_NO_LINE;
        } else {
            o.status = EAGLE_OFFSIDE_EV_OK;
            o.margin = mg; o.line_qx = rec.line_qx; o.n_off = rec.n_off;
            o.verdict = mg > a.tq ? EAGLE_OFFSIDE_OFFSIDE : mg > -a.tq ? EAGLE_OFFSIDE_CLOSE : EAGLE_OFFSIDE_ONSIDE;
            const bool right = of_right(a.clip->direction, g);                             // (resolved: the record is OK)
            int b0, b1;
            if (a.ball >= 0 && of_quantise(a.values[(size_t)a.ball * a.rows + r0], b0) && of_quantise(a.values[(size_t)a.ball * a.rows + r1], b1)) {
                int n = 0;
                for (int k = g ? 0 : a.n0; k < (g ? a.n0 : a.n0 + a.n1); ++k) {            // the members of 1 - g
                    const size_t c = (size_t)a.gcols[k] * a.rows;
                    int q0, q1;
                    if (!of_quantise(a.values[c + r0], q0) || !of_quantise(a.values[c + r1], q1)) continue;
                    n += right ? (q0 > b0 && q1 <= b1) : (q0 < b0 && q1 >= b1);           // u = qx, or 107520 - qx on both sides
                }
                o.bypassed = n;
            }
        }
    }
    a.events_out[e] = o;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static int offside_check(const char* who, const EagleOffsideParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the offside parameters are NULL", who);
    if (p->direction != EAGLE_OFFSIDE_DIR_AUTO && p->direction != EAGLE_OFFSIDE_DIR_RIGHT && p->direction != EAGLE_OFFSIDE_DIR_LEFT)
        fail(EAGLE_E_INVALID, "%s: direction %d is none of EAGLE_OFFSIDE_DIR_AUTO, _RIGHT, _LEFT", who, p->direction);
    if (!(std::isfinite(p->tolerance) && p->tolerance >= 0.0 && p->tolerance <= 1024.0))
        fail(EAGLE_E_INVALID, "%s: tolerance %g must be finite and within [0, 1024] metres", who, p->tolerance);
    for (int k = 0; k < 4; ++k)
        if (p->reserved[k]) fail(EAGLE_E_INVALID, "%s: reserved word %d of the offside parameters is %d, not 0", who, k, p->reserved[k]);
    return (int)floor(p->tolerance * 1024.0 + 0.5);
}

// (OfCols: runtime.h)  groups 0 and 1 are the team shape's (and its refusals); the keepers: the Goalkeeper pitch columns; the ball: the one Ball pitch column
OfCols offside_columns(const char* who, const EaglePostColumn* columns, int ncols, bool no_ball, const int32_t* team_ids, const int32_t* team_vals, size_t n_team,
                              const EagleOffsideParams* p)
{
    const ShapeCols sc = shape_columns(who, columns, ncols, team_ids, team_vals, n_team);
    OfCols o;
    o.n0 = sc.n0; o.n1 = sc.n1; o.gcols = sc.gcols;
    o.member_of.assign((size_t)std::max(ncols, 1), -1);
    for (int k = 0; k < sc.n0 + sc.n1; ++k) {
        o.member_of[sc.gcols[k]] = k;
        EagleOffsideTotals t{};
        t.col = sc.gcols[k]; t.group = k < sc.n0 ? 0 : 1; t.max_margin = OF_NONE;
        o.init.push_back(t);
    }
    int keepers = 0;
    for (int c = 0; c < ncols; ++c) {
        if (columns[c].video) continue;
        if (o.member_of[c] >= 0) o.list.push_back(make_int4(c, o.member_of[c] < sc.n0 ? 0 : 1, o.member_of[c], 0));
        else if (columns[c].kind == EAGLE_POST_GOALKEEPER) { o.list.push_back(make_int4(c, 2, -1, 0)); ++keepers; }
        else if (columns[c].kind == EAGLE_POST_BALL) {
            if (o.ball >= 0) fail(EAGLE_E_INVALID, "%s: columns %d and %d are both the ball", who, o.ball, c);
            o.ball = c;
        }
    }
    if (no_ball) o.ball = -1;
    if (o.list.size() > (size_t)EAGLE_SHAPE_MAX_MEMBERS) fail(EAGLE_E_INVALID, "%s: %zu members and keepers are beyond %d", who, o.list.size(), EAGLE_SHAPE_MAX_MEMBERS);
    o.clip.requested = p->direction; o.clip.n_members[0] = sc.n0; o.clip.n_members[1] = sc.n1; o.clip.n_keepers = keepers;
    return o;
}

// a pass event is read at its two rows and its receiver's column
static void offside_events_check(const char* who, const EaglePossessionEvent* ev, size_t n, int rows, int cols)
{
    for (size_t e = 0; e < n; ++e)
        if (ev[e].kind == EAGLE_EVENT_PASS &&
            (ev[e].release_row < 0 || ev[e].release_row >= rows || ev[e].receive_row < 0 || ev[e].receive_row >= rows || ev[e].to_col < 0 || ev[e].to_col >= cols))
            fail(EAGLE_E_INVALID, "%s: pass event %zu (rows %d and %d, receiver column %d) lies outside the table's %d rows and %d columns", who, e, ev[e].release_row,
                 ev[e].receive_row, ev[e].to_col, rows, cols);
}

static size_t of_up(size_t b) { return (std::max<size_t>(b, 16) + 255) & ~(size_t)255; }

// a result: records | margins | totals | clip | events, each from a 256-byte boundary
struct OfKept { size_t rows, margins, totals, clip, events, total; };

static OfKept offside_kept(size_t rows, size_t nm, size_t ne)
{
    OfKept o{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += of_up(b); return was; };
    o.rows = take(rows * 2 * sizeof(EagleOffsideRow)); o.margins = take(nm * rows * 4); o.totals = take(nm * sizeof(EagleOffsideTotals));
    o.clip = take(sizeof(EagleOffsideClip)); o.events = take(ne * sizeof(EagleOffsideEvent));
    o.total = at;
    return o;
}

// the scratch of a call: list | gcols | member_of | the possession events
struct OfLists { size_t list, gcols, member_of, events, total; };

static OfLists offside_lists(const OfCols& oc, size_t ne)
{
    OfLists o{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += of_up(b); return was; };
    o.list = take(oc.list.size() * sizeof(int4)); o.gcols = take(oc.gcols.size() * 4); o.member_of = take(oc.member_of.size() * 4);
    o.events = take(ne * sizeof(EaglePossessionEvent));
    o.total = at;
    return o;
}

static void offside_budget(const char* who, size_t need, int64_t max_bytes)
{
    double budget = (double)max_bytes;
    if (max_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = 0.9 * (double)free_b;
    }
    if ((double)need > budget) fail(EAGLE_E_INVALID, "%s: the call needs %.0f bytes of device memory, the budget is %.0f", who, (double)need, budget);
}

// The whole table (rows > 0) -> a result at d (offside_kept bytes); lists: offside_lists bytes.  Returns when it is complete.  Pageable sources: they
// have left the vectors when this returns
static void offside_table(EagleHandle* h, const OfCols& oc, const double2* d_values, int rows, const EagleOffsideParams* p, int tq, const EaglePossessionEvent* events,
                          size_t ne, uint8_t* d, uint8_t* lists, hipStream_t s)
{
    const size_t nm = oc.init.size();
    const OfKept K = offside_kept((size_t)rows, nm, ne);
    const OfLists L = offside_lists(oc, ne);
    OfArgs a{};
    a.values = d_values; a.rows = rows; a.nl = (int)oc.list.size(); a.n0 = oc.n0; a.n1 = oc.n1; a.ball = oc.ball;
    a.requested = p->direction; a.assume = p->assume_keeper; a.tq = tq;
    a.list = (const int4*)(lists + L.list); a.gcols = (const int32_t*)(lists + L.gcols); a.member_of = (const int32_t*)(lists + L.member_of);
    a.events = (const EaglePossessionEvent*)(lists + L.events); a.n_events = (int)ne;
    a.rows_out = (EagleOffsideRow*)(d + K.rows); a.margins = (int32_t*)(d + K.margins); a.totals = (EagleOffsideTotals*)(d + K.totals);
    a.clip = (EagleOffsideClip*)(d + K.clip); a.events_out = (EagleOffsideEvent*)(d + K.events);
    auto up = [&](const void* dst, const void* src, size_t b) {
        if (b) HIP_CHECK(hipMemcpyAsync((void*)dst, src, b, hipMemcpyHostToDevice, s));
    };
    up(a.list, oc.list.data(), oc.list.size() * sizeof(int4));
    up(a.gcols, oc.gcols.data(), oc.gcols.size() * 4);
    up(a.member_of, oc.member_of.data(), oc.member_of.size() * 4);
    up(a.events, events, ne * sizeof(EaglePossessionEvent));
    up(a.totals, oc.init.data(), nm * sizeof(EagleOffsideTotals));
    up(a.clip, &oc.clip, sizeof(EagleOffsideClip));
    auto run = [&](const char* name, double bytes, const std::function<void()>& fn) {
        if (h) timed_launch(h, name, bytes, s, fn); else fn();
    };
    // bytes: the member cells read; the listed cells read twice, the records and margins written; the margins read; per event a record, a margin, the cells
    const double n = (double)rows;
    run("offside_vote", n * 16.0 * (double)nm, [&] {
        hipLaunchKernelGGL(offside_vote_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, a);
        HIP_CHECK(hipGetLastError());
    });
    run("offside_rows", n * 2.0 * (32.0 * a.nl + 16.0 + 48.0) + n * 4.0 * (double)nm, [&] {
        hipLaunchKernelGGL(offside_rows_kernel, dim3((unsigned)(((size_t)rows * 2 + 3) / 4)), dim3(256), 0, s, a);
        HIP_CHECK(hipGetLastError());
    });
    if (nm)
        run("offside_totals", n * 4.0 * (double)nm, [&] {
            hipLaunchKernelGGL(offside_totals_kernel, dim3((unsigned)nm), dim3(256), 0, s, a);
            HIP_CHECK(hipGetLastError());
        });
    if (ne)
        run("offside_events", (double)ne * (80.0 + 48.0 + 4.0 + 32.0 + 32.0 * (double)(nm + 1)), [&] {
            hipLaunchKernelGGL(offside_events_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, a);
            HIP_CHECK(hipGetLastError());
        });
    HIP_CHECK(hipStreamSynchronize(s));
    if (h && h->prof) collect_spans(h);
}

}  // namespace eagle

extern "C" {

int eagle_post_offside(EagleHandle* h, EaglePostTable* t, const EagleOffsideParams* p)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_offside: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_offside: the table belongs to another handle");
    const int tq = offside_check("eagle_post_offside", p);
    const int32_t none = 0;                                              // (a mapping of no entries is a mapping: nobody is a member)
    const OfCols oc = offside_columns("eagle_post_offside", t->columns.data(), t->cols, (t->flags & EAGLE_POST_NO_BALL) != 0,
                                      !t->has_team ? nullptr : t->team_ids.empty() ? &none : t->team_ids.data(), t->team_vals.data(), t->has_team ? t->team_ids.size() : 0, p);
    const size_t rows = (size_t)t->rows, nm = oc.init.size(), ne = t->has_poss ? t->events.size() : 0;
    offside_events_check("eagle_post_offside", t->events.data(), ne, t->rows, t->cols);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    // the budget: the new result and the lists.  The result is a buffer of its own: the earlier one stays until the new one is complete, and in place
    // when the call fails
    const OfKept K = offside_kept(rows, nm, ne);
    const OfLists L = offside_lists(oc, ne);
    offside_budget("eagle_post_offside", K.total + L.total, t->max_bytes);
    uint8_t* d = nullptr;
    uint8_t* lists = nullptr;
    try {
        HIP_CHECK(hipMalloc((void**)&d, K.total));
        if (rows) {
            HIP_CHECK(hipMalloc((void**)&lists, L.total));
            offside_table(h, oc, (const double2*)t->d_values, t->rows, p, tq, t->events.data(), ne, d, lists, h->s_main);
        } else {
            HIP_CHECK(hipMemset(d, 0, K.total));                         // (no launch writes a table without rows)
        }
    } catch (...) {
        (void)hipStreamSynchronize(h->s_main);
        if (lists) (void)hipFree(lists);
        if (d) (void)hipFree(d);
        throw;
    }
    if (lists) HIP_CHECK(hipFree(lists));
    if (t->d_offside) (void)hipFree(t->d_offside);
    t->d_offside = d;
    t->offside_members = (int)nm;
    t->offside_events = rows ? (int)ne : 0;
    API_END(h)
}

int eagle_post_offside_values(EaglePostTable* t, EagleOffsideRow* rows_out, int32_t* margins, EagleOffsideTotals* totals_out, EagleOffsideClip* clip_out)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->d_offside) fail(EAGLE_E_INVALID, "eagle_post_offside_values: the table has no offside result (eagle_post_offside)");
    const size_t rows = (size_t)t->rows, nm = (size_t)t->offside_members;
    if (rows) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        const uint8_t* d = (const uint8_t*)t->d_offside;
        const OfKept K = offside_kept(rows, nm, (size_t)t->offside_events);
        if (rows_out) HIP_CHECK(hipMemcpy(rows_out, d + K.rows, rows * 2 * sizeof(EagleOffsideRow), hipMemcpyDeviceToHost));
        if (margins && nm) HIP_CHECK(hipMemcpy(margins, d + K.margins, nm * rows * 4, hipMemcpyDeviceToHost));
        if (totals_out && nm) HIP_CHECK(hipMemcpy(totals_out, d + K.totals, nm * sizeof(EagleOffsideTotals), hipMemcpyDeviceToHost));
        if (clip_out) HIP_CHECK(hipMemcpy(clip_out, d + K.clip, sizeof(EagleOffsideClip), hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_post_offside_events(const EaglePostTable* t, EagleOffsideEvent* out, int cap, int* n)
{
    if (!t || !n || cap < 0 || (cap > 0 && !out)) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    const int ne = t->d_offside ? t->offside_events : 0;
    *n = ne;
    const size_t k = (size_t)std::min(cap, ne);
    if (k) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        const OfKept K = offside_kept((size_t)t->rows, (size_t)t->offside_members, (size_t)ne);
        HIP_CHECK(hipMemcpy(out, (const uint8_t*)t->d_offside + K.events, k * sizeof(EagleOffsideEvent), hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_post_device_offside(const EaglePostTable* t, const EagleOffsideRow** d_rows, const int32_t** d_margins, const EagleOffsideTotals** d_totals,
                              const EagleOffsideClip** d_clip, const EagleOffsideEvent** d_events, int* n_members, int* n_events)
{
    if (!t || !d_rows || !d_margins || !d_totals || !d_clip || !d_events) return EAGLE_E_INVALID;
    const uint8_t* d = (const uint8_t*)t->d_offside;
    const eagle::OfKept K = eagle::offside_kept((size_t)t->rows, (size_t)t->offside_members, (size_t)t->offside_events);
    *d_rows = d ? (const EagleOffsideRow*)(d + K.rows) : nullptr;
    *d_margins = d ? (const int32_t*)(d + K.margins) : nullptr;
    *d_totals = d ? (const EagleOffsideTotals*)(d + K.totals) : nullptr;
    *d_clip = d ? (const EagleOffsideClip*)(d + K.clip) : nullptr;
    *d_events = d ? (const EagleOffsideEvent*)(d + K.events) : nullptr;
    if (n_members) *n_members = d ? t->offside_members : 0;
    if (n_events) *n_events = d ? t->offside_events : 0;
    return EAGLE_OK;
}

int eagle_op_offside(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                     const int32_t* team_vals, int n_team, const EagleOffsideParams* p, const EaglePossessionEvent* events, int n_events,
                     EagleOffsideRow* rows_out, int32_t* margins, EagleOffsideTotals* totals_out, EagleOffsideClip* clip_out, EagleOffsideEvent* events_out)
{
    EagleHandle* hh = nullptr;
    (void)frames;
    API_BEGIN
    if (!values || !columns || rows < 0 || cols < 0 || n_team < 0 || (team_ids && n_team > 0 && !team_vals) || n_events < 0 || (n_events > 0 && !events))
        fail(EAGLE_E_INVALID, "eagle_op_offside: bad argument (values %p, columns %p, %d rows, %d columns, %d teams, events %p, %d events)", (const void*)values,
             (const void*)columns, rows, cols, n_team, (const void*)events, n_events);
    const int tq = offside_check("eagle_op_offside", p);
    const OfCols oc = offside_columns("eagle_op_offside", columns, cols, false, team_ids, team_vals, (size_t)n_team, p);
    if (rows == 0) return EAGLE_OK;
    const size_t nr = (size_t)rows, nm = oc.init.size(), ne = (size_t)n_events;
    offside_events_check("eagle_op_offside", events, ne, rows, cols);
    HIP_CHECK(hipSetDevice(device));
    const OfKept K = offside_kept(nr, nm, ne);
    const OfLists L = offside_lists(oc, ne);
    offside_budget("eagle_op_offside", (size_t)cols * nr * sizeof(double2) + K.total + L.total, 0);
    Net net;
    const double2* d_v = (const double2*)net.upload(values, std::max<size_t>((size_t)cols * nr * sizeof(double2), 16));
    uint8_t* d = (uint8_t*)net.get(K.total);
    offside_table(nullptr, oc, d_v, rows, p, tq, events, ne, d, (uint8_t*)net.get(L.total), nullptr);
    if (rows_out) HIP_CHECK(hipMemcpy(rows_out, d + K.rows, nr * 2 * sizeof(EagleOffsideRow), hipMemcpyDeviceToHost));
    if (margins && nm) HIP_CHECK(hipMemcpy(margins, d + K.margins, nm * nr * 4, hipMemcpyDeviceToHost));
    if (totals_out && nm) HIP_CHECK(hipMemcpy(totals_out, d + K.totals, nm * sizeof(EagleOffsideTotals), hipMemcpyDeviceToHost));
    if (clip_out) HIP_CHECK(hipMemcpy(clip_out, d + K.clip, sizeof(EagleOffsideClip), hipMemcpyDeviceToHost));
    if (events_out && ne) HIP_CHECK(hipMemcpy(events_out, d + K.events, ne * sizeof(EagleOffsideEvent), hipMemcpyDeviceToHost));
    API_END(hh)
}

}  // extern "C"
