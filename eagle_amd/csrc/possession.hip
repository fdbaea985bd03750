// K23 — ball possession and pass events: a processed table resident in HBM (post.hip) -> per row the nearest person to the ball, the owner of the ball,
// and the rows at which the ball changes feet (include/eagle.h, eagle_post_possession / eagle_op_possession; tests/possession_ref.py is the written
// definition of every bit: float64, no contraction, correctly rounded sqrt and division).
//
// Three launches per call on one stream, no host round trip for the rows:
//   possession_cand_kernel    one thread per row walks the person columns (the host decides per COLUMN what is a person, as control_columns does).
//                             In the [cols][rows][2] layout consecutive rows are consecutive 16-byte cells, so a wave's load is one run of 1024 bytes:
//                             the velocity kernel's access pattern.  It reads the pitch half of the table once and is the bandwidth-bound part.
//   possession_scan_kernel    ONE workgroup of PS_SCAN threads walks the rows in chunks of PS_SCAN.  Every rule of the specification is an inclusive
//                             max-scan of row indices: run start (greatest head row), last confirmation, last segment start.  Per chunk: a wave scan
//                             (__shfl_up), the 16 wave totals through LDS, the carry of the chunks before in registers; the confirmation scan needs
//                             the run start, so it is a second round; the owner is a gather of cand[] at the last confirmation (a thread forms
//                             the owner of row r - 1 too, from the scans without its own term, so owners are not exchanged); the event flags go
//                             through an add-scan of the same shape and the event rows are stored compacted, in row order.  Three barriers per chunk.
//   possession_event_kernel   one thread per event fills its record from the per-row arrays (after the host has read the count: the buffer is sized by
//                             it, not by the row count).
#include "runtime.h"

namespace eagle {

static constexpr int PC_THREADS = 256;         // candidate kernel
static constexpr int PS_SCAN = 1024;           // scan kernel: one workgroup, 16 waves
static constexpr int PS_WAVES = PS_SCAN / 64;

struct PossArgs {
    const double2* values;       // [column][row]
    const int32_t* frames;       // [rows]
    const int32_t* persons;      // candidate columns in table order
    const int32_t* team;         // [cols] resolved team, -1 unknown
    int rows, npersons, ball;    // ball: the ball's column, -1 = none
    double r2, fps;
    int min_hold, max_gap;
    // per row
    double* dist; int32_t* cand; int32_t* owner;
    uint8_t* has_ball; int32_t* headrow; int32_t* lastconf; int32_t* evrow;
    int32_t* count;              // [1] events
    EaglePossessionEvent* events; int n_events;
};

__device__ __forceinline__ bool present(double2 p) { return fabs(p.x) <= 1.7976931348623157e308 && fabs(p.y) <= 1.7976931348623157e308; }

__global__ __launch_bounds__(PC_THREADS) void possession_cand_kernel(PossArgs a)
{
    const int r = blockIdx.x * PC_THREADS + threadIdx.x;
    if (r >= a.rows) return;
    double2 b = make_double2(0.0, 0.0);
    bool ball = false;
    if (a.ball >= 0) { b = a.values[(size_t)a.ball * a.rows + r]; ball = present(b); }
    double best = 0.0;
    int bc = -1;
    if (ball) {
        #pragma unroll 4
        for (int k = 0; k < a.npersons; ++k) {
            const int c = a.persons[k];                                  // (uniform)
            const double2 p = a.values[(size_t)c * a.rows + r];
            if (!present(p)) continue;
            const double dx = p.x - b.x, dy = p.y - b.y;
            const double d2 = dx * dx + dy * dy;
            if (bc < 0 || d2 < best) { best = d2; bc = c; }              // a tie keeps the earlier column
        }
    }
    a.has_ball[r] = ball ? 1 : 0;
    a.dist[r] = bc >= 0 ? sqrt(best) : __longlong_as_double(0x7ff8000000000000ll);
    a.cand[r] = (bc >= 0 && best <= a.r2) ? bc : -1;
}

__device__ __forceinline__ int wave_max_scan(int v, int lane)
{
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d, 64); if (lane >= d) v = max(v, o); }
    return v;
}

__device__ __forceinline__ int wave_add_scan(int v, int lane)
{
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d, 64); if (lane >= d) v += o; }
    return v;
}

__global__ __launch_bounds__(PS_SCAN) void possession_scan_kernel(PossArgs a)
{
    __shared__ int s_head[PS_WAVES], s_seg[PS_WAVES], s_conf[PS_WAVES], s_cnt[PS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int c_head = -1, c_seg = -1, c_conf = -1, c_cnt = 0;                 // the chunks before this one (registers, the same in every thread)
    for (int base = 0; base < a.rows; base += PS_SCAN) {                 // (uniform: every thread meets every barrier)
        const int r = base + tid;
        const bool live = r < a.rows;
        int cand = -1;
        bool ball = false, ball_prev = false, seg = false, head = false;
        if (live) {
            cand = a.cand[r];
            ball = a.has_ball[r] != 0;
            seg = r == 0 || !ball || (long long)a.frames[r] - (long long)a.frames[r - 1] > (long long)a.max_gap;
            head = seg || cand < 0 || cand != a.cand[r - 1];             // (seg covers r == 0)
            ball_prev = r >= 1 && a.has_ball[r - 1] != 0;
        }
        // ---- round 1: run start and last segment start (and the latter for row r - 1: the scan without the row's own term) ----
        const int w_head = wave_max_scan(head ? r : -1, lane), w_seg = wave_max_scan(seg ? r : -1, lane);
        int x_seg = __shfl_up(w_seg, 1, 64);
        if (lane == 0) x_seg = -1;
        if (lane == 63) { s_head[wave] = w_head; s_seg[wave] = w_seg; }
        __syncthreads();
        int before_head = c_head, before_seg = c_seg;                    // everything in front of this wave
        #pragma unroll
        for (int w = 0; w < PS_WAVES; ++w) {
            const int th = s_head[w], ts = s_seg[w];                     // (one address per wave: an LDS broadcast)
            if (w < wave) { before_head = max(before_head, th); before_seg = max(before_seg, ts); }
            c_head = max(c_head, th); c_seg = max(c_seg, ts);
        }
        const int headrow = max(before_head, w_head), lastseg = max(before_seg, w_seg), lastseg_prev = max(before_seg, x_seg);
        // ---- round 2: the last confirmation, for row r and for row r - 1 ----
        const int run = cand >= 0 ? r - headrow + 1 : 0;
        const bool conf = cand >= 0 && run >= a.min_hold;
        const int w_conf = wave_max_scan(conf ? r : -1, lane);
        int x_conf = __shfl_up(w_conf, 1, 64);
        if (lane == 0) x_conf = -1;
        if (lane == 63) s_conf[wave] = w_conf;
        __syncthreads();
        int before_conf = c_conf;
        #pragma unroll
        for (int w = 0; w < PS_WAVES; ++w) {
            const int tc = s_conf[w];
            if (w < wave) before_conf = max(before_conf, tc);
            c_conf = max(c_conf, tc);
        }
        const int lastconf = max(before_conf, w_conf), lastconf_prev = max(before_conf, x_conf);
        // ---- owner of row r and of row r - 1 (the same rule, so no exchange), event flag, compaction ----
        int owner = -1, prev = -1;
        if (live && ball && lastconf >= 0 && lastconf >= lastseg) owner = a.cand[lastconf];
        if (live && ball_prev && lastconf_prev >= 0 && lastconf_prev >= lastseg_prev) prev = a.cand[lastconf_prev];
        const bool ev = live && r >= 1 && !seg && owner >= 0 && prev >= 0 && owner != prev;
        const int w_cnt = wave_add_scan(ev ? 1 : 0, lane);
        if (lane == 63) s_cnt[wave] = w_cnt;
        __syncthreads();
        int off = c_cnt + w_cnt - (ev ? 1 : 0);
        #pragma unroll
        for (int w = 0; w < PS_WAVES; ++w) {
            const int tn = s_cnt[w];
            if (w < wave) off += tn;
            c_cnt += tn;
        }
        if (live) {
            a.owner[r] = owner; a.headrow[r] = headrow; a.lastconf[r] = lastconf;
            if (ev) a.evrow[off] = r;                                    // off < rows: at most one event per row
        }
        // no barrier here: an array is written again only behind a later barrier than the one its readers have passed (s_head and s_seg: read in
        // front of the second barrier, written behind the third; s_conf: read in front of the third, written behind the next chunk's first; s_cnt:
        // read in front of the next chunk's first, written behind its second)
    }
    if (tid == 0) a.count[0] = c_cnt;
}

__global__ __launch_bounds__(256) void possession_event_kernel(PossArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_events) return;
    const int r = a.evrow[i];
    EaglePossessionEvent e{};
    e.row = r; e.from_col = a.owner[r - 1]; e.to_col = a.owner[r];
    e.release_row = a.lastconf[r - 1]; e.receive_row = a.headrow[r];
    const int tf = a.team[e.from_col], tt = a.team[e.to_col];
    e.kind = (tf < 0 || tt < 0) ? EAGLE_EVENT_UNKNOWN : (tf == tt ? EAGLE_EVENT_PASS : EAGLE_EVENT_TURNOVER);
    const double2 p0 = a.values[(size_t)a.ball * a.rows + e.release_row], p1 = a.values[(size_t)a.ball * a.rows + e.receive_row];
    e.x0 = p0.x; e.y0 = p0.y; e.x1 = p1.x; e.y1 = p1.y;
    const double dx = p1.x - p0.x, dy = p1.y - p0.y;
    e.length = sqrt(dx * dx + dy * dy);
    e.duration = (double)((long long)a.frames[e.receive_row] - (long long)a.frames[e.release_row]) / a.fps;
    a.events[i] = e;
}

static void possession_check(const char* who, const EaglePossessionParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: params is NULL", who);
    if (p->fps <= 0 || p->max_gap <= 0 || p->min_hold <= 0)
        fail(EAGLE_E_INVALID, "%s: fps %d, max_gap %d and min_hold %d must be positive", who, p->fps, p->max_gap, p->min_hold);
    if (!(p->radius > 0.0 && p->radius <= 1024.0)) fail(EAGLE_E_INVALID, "%s: radius %g must be positive and at most 1024 m", who, p->radius);
}

// What the kernels need to know of the columns: the persons in table order, the ball's column (-1: none) and every column's team (-1: unknown)
struct PossCols { std::vector<int32_t> persons, team; int ball = -1; };

static PossCols possession_columns(const char* who, const EaglePostColumn* columns, int ncols, bool no_ball, const int32_t* team_ids, const int32_t* team_vals, size_t n_team)
{
    PossCols pc;
    pc.team.assign(std::max(ncols, 1), -1);
    for (int c = 0; c < ncols; ++c) {
        const EaglePostColumn& col = columns[c];
        if (col.kind != EAGLE_POST_PLAYER && col.kind != EAGLE_POST_GOALKEEPER && col.kind != EAGLE_POST_BALL && col.kind != EAGLE_POST_BOUNDARY)
            fail(EAGLE_E_INVALID, "%s: column %d is of unknown kind %d", who, c, col.kind);
        if (col.video) continue;
        if (col.kind == EAGLE_POST_BALL) {
            if (pc.ball >= 0) fail(EAGLE_E_INVALID, "%s: columns %d and %d are both the ball", who, pc.ball, c);
            pc.ball = c;
        } else if (col.kind == EAGLE_POST_PLAYER || col.kind == EAGLE_POST_GOALKEEPER) {
            pc.persons.push_back(c);
            size_t k = 0;
            while (k < n_team && team_ids[k] != col.id) ++k;             // the first entry counts, as in control_columns
            if (k < n_team && team_vals[k] >= 0) pc.team[c] = team_vals[k];
        }
    }
    if (no_ball) pc.ball = -1;
    return pc;
}

static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// The scratch of one call in a single allocation behind `base`; the three launches on s.  events_out receives the events (the count is read in between).
struct PossScratch { size_t persons, team, has_ball, headrow, lastconf, evrow, count, total; };

static PossScratch possession_scratch(int rows, int ncols, size_t npersons)
{
    PossScratch o{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += up16(std::max<size_t>(b, 16)); return was; };
    o.persons = take(npersons * 4); o.team = take((size_t)std::max(ncols, 1) * 4); o.has_ball = take(rows);
    o.headrow = take((size_t)rows * 4); o.lastconf = take((size_t)rows * 4); o.evrow = take((size_t)rows * 4); o.count = take(4);
    o.total = at;
    return o;
}

static void possession_run(EagleHandle* h, const PossCols& pc, const double2* d_values, const int32_t* d_frames, int rows, int ncols, const EaglePossessionParams* p,
                           double* d_dist, int32_t* d_cand, int32_t* d_owner, std::vector<EaglePossessionEvent>& events_out, hipStream_t s)
{
    const PossScratch L = possession_scratch(rows, ncols, pc.persons.size());
    uint8_t* base = nullptr;
    EaglePossessionEvent* d_ev = nullptr;
    HIP_CHECK(hipMalloc((void**)&base, L.total));
    try {
        if (!pc.persons.empty()) HIP_CHECK(hipMemcpyAsync(base + L.persons, pc.persons.data(), pc.persons.size() * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(base + L.team, pc.team.data(), pc.team.size() * 4, hipMemcpyHostToDevice, s));
        PossArgs a{};
        a.values = d_values; a.frames = d_frames; a.persons = (const int32_t*)(base + L.persons); a.team = (const int32_t*)(base + L.team);
        a.rows = rows; a.npersons = (int)pc.persons.size(); a.ball = pc.ball;
        a.r2 = p->radius * p->radius; a.fps = (double)p->fps; a.min_hold = p->min_hold; a.max_gap = p->max_gap;
        a.dist = d_dist; a.cand = d_cand; a.owner = d_owner;
        a.has_ball = base + L.has_ball; a.headrow = (int32_t*)(base + L.headrow); a.lastconf = (int32_t*)(base + L.lastconf);
        a.evrow = (int32_t*)(base + L.evrow); a.count = (int32_t*)(base + L.count);
        auto cand = [&] {
            hipLaunchKernelGGL(possession_cand_kernel, dim3((rows + PC_THREADS - 1) / PC_THREADS), dim3(PC_THREADS), 0, s, a);
            HIP_CHECK(hipGetLastError());
        };
        auto scan = [&] {
            hipLaunchKernelGGL(possession_scan_kernel, dim3(1), dim3(PS_SCAN), 0, s, a);
            HIP_CHECK(hipGetLastError());
        };
        // bytes: the ball's and the persons' cells read (when there is a ball), 13 per row written; the scan reads 13 + 8 and writes 12 per row
        const double cand_b = (double)rows * ((pc.ball >= 0 ? 16.0 * (1.0 + (double)pc.persons.size()) : 0.0) + 13.0);
        if (h) {
            timed_launch(h, "possession_cand", cand_b, s, cand);
            timed_launch(h, "possession_scan", 33.0 * (double)rows, s, scan);
        } else { cand(); scan(); }
        int32_t n = 0;
        HIP_CHECK(hipMemcpyAsync(&n, a.count, 4, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (n < 0 || n >= std::max(rows, 1)) fail(EAGLE_E_STATE, "possession: %d events from %d rows", n, rows);
        events_out.assign((size_t)n, EaglePossessionEvent{});
        if (n) {
            HIP_CHECK(hipMalloc((void**)&d_ev, (size_t)n * sizeof(EaglePossessionEvent)));
            a.events = d_ev; a.n_events = n;
            hipLaunchKernelGGL(possession_event_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(events_out.data(), d_ev, (size_t)n * sizeof(EaglePossessionEvent), hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
        if (h && h->prof) collect_spans(h);
    } catch (...) {
        (void)hipStreamSynchronize(s);
        if (d_ev) (void)hipFree(d_ev);
        (void)hipFree(base);
        throw;
    }
    if (d_ev) HIP_CHECK(hipFree(d_ev));
    HIP_CHECK(hipFree(base));
}

}  // namespace eagle

extern "C" {

int eagle_post_possession(EagleHandle* h, EaglePostTable* t, const EaglePossessionParams* p)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_possession: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_possession: the table belongs to another handle");
    possession_check("eagle_post_possession", p);
    const PossCols pc = possession_columns("eagle_post_possession", t->columns.data(), t->cols, (t->flags & EAGLE_POST_NO_BALL) != 0,
                                           t->has_team ? t->team_ids.data() : nullptr, t->has_team ? t->team_vals.data() : nullptr, t->has_team ? t->team_ids.size() : 0);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)t->rows;
    if (!t->d_poss) HIP_CHECK(hipMalloc((void**)&t->d_poss, std::max<size_t>(rows * 16, 16)));       // dist [rows] f64 | cand [rows] i32 | owner [rows] i32
    t->events.clear();
    t->has_poss = true;
    if (rows) {
        double* d_dist = (double*)t->d_poss;
        int32_t* d_cand = (int32_t*)(d_dist + rows);
        int32_t* d_owner = d_cand + rows;
        const hipStream_t s = h->s_main;
        int32_t* d_frames = nullptr;
        HIP_CHECK(hipMalloc((void**)&d_frames, rows * 4));
        try {
            HIP_CHECK(hipMemcpyAsync(d_frames, t->frames.data(), rows * 4, hipMemcpyHostToDevice, s));
            possession_run(h, pc, (const double2*)t->d_values, d_frames, t->rows, t->cols, p, d_dist, d_cand, d_owner, t->events, s);
        } catch (...) {
            (void)hipStreamSynchronize(s);
            (void)hipFree(d_frames);
            throw;
        }
        HIP_CHECK(hipFree(d_frames));
    }
    API_END(h)
}

int eagle_post_possession_values(EaglePostTable* t, int32_t* cand, int32_t* owner, double* dist)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->has_poss) fail(EAGLE_E_INVALID, "eagle_post_possession_values: the table has no possession (eagle_post_possession)");
    const size_t rows = (size_t)t->rows;
    if (rows) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        const double* d_dist = (const double*)t->d_poss;
        const int32_t* d_cand = (const int32_t*)(d_dist + rows);
        if (dist) HIP_CHECK(hipMemcpy(dist, d_dist, rows * 8, hipMemcpyDeviceToHost));
        if (cand) HIP_CHECK(hipMemcpy(cand, d_cand, rows * 4, hipMemcpyDeviceToHost));
        if (owner) HIP_CHECK(hipMemcpy(owner, d_cand + rows, rows * 4, hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_post_device_possession(const EaglePostTable* t, const int32_t** d_owner)
{
    if (!t || !d_owner) return EAGLE_E_INVALID;
    *d_owner = t->has_poss ? (const int32_t*)((const double*)t->d_poss + t->rows) + t->rows : nullptr;
    return EAGLE_OK;
}

int eagle_post_events(const EaglePostTable* t, EaglePossessionEvent* out, int cap, int* n)
{
    if (!t || !n || cap < 0 || (cap > 0 && !out)) return EAGLE_E_INVALID;
    *n = (int)t->events.size();
    std::copy(t->events.begin(), t->events.begin() + std::min<size_t>(cap, t->events.size()), out);
    return EAGLE_OK;
}

int eagle_op_possession(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                        const int32_t* team_vals, int n_team, const EaglePossessionParams* p, int32_t* cand, int32_t* owner, double* dist,
                        EaglePossessionEvent* events, int cap, int* n_events)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !frames || !columns || !n_events || rows < 0 || cols < 0 || n_team < 0 || cap < 0 || (cap > 0 && !events) || (team_ids && n_team > 0 && !team_vals))
        fail(EAGLE_E_INVALID, "eagle_op_possession: bad argument (values %p, frames %p, columns %p, n_events %p, %d rows, %d columns, %d teams, events %p, cap %d)",
             (const void*)values, (const void*)frames, (const void*)columns, (const void*)n_events, rows, cols, n_team, (const void*)events, cap);
    possession_check("eagle_op_possession", p);
    const PossCols pc = possession_columns("eagle_op_possession", columns, cols, false, team_ids, team_vals, team_ids ? (size_t)n_team : 0);
    for (int r = 1; r < rows; ++r)
        if (frames[r] <= frames[r - 1]) fail(EAGLE_E_INVALID, "eagle_op_possession: frame numbers must ascend (row %d: %d after %d)", r, frames[r], frames[r - 1]);
    *n_events = 0;
    if (rows == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const size_t n = (size_t)rows;
    const double2* d_v = (const double2*)net.upload(values, (size_t)cols * n * sizeof(double2));
    const int32_t* d_f = (const int32_t*)net.upload(frames, n * 4);
    double* d_dist = (double*)net.get(n * 16);
    int32_t* d_cand = (int32_t*)(d_dist + n);
    std::vector<EaglePossessionEvent> ev;
    possession_run(nullptr, pc, d_v, d_f, rows, cols, p, d_dist, d_cand, d_cand + n, ev, nullptr);
    if (dist) HIP_CHECK(hipMemcpy(dist, d_dist, n * 8, hipMemcpyDeviceToHost));
    if (cand) HIP_CHECK(hipMemcpy(cand, d_cand, n * 4, hipMemcpyDeviceToHost));
    if (owner) HIP_CHECK(hipMemcpy(owner, d_cand + n, n * 4, hipMemcpyDeviceToHost));
    *n_events = (int)ev.size();
    std::copy(ev.begin(), ev.begin() + std::min<size_t>(cap, ev.size()), events);
    API_END(hh)
}

}  // extern "C"
