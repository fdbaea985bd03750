// K27 — physical report per person: the velocities of a processed table resident in HBM (post.hip, eagle_post_velocities) -> per person and row the speed,
// its derivative and the speed zone; per person the frames and the distance per zone, the top speed and the efforts: high-speed runs, sprints, accelerations
// and decelerations (include/eagle.h, eagle_post_physical / eagle_op_physical; tests/physical_ref.py is the written definition of every bit: float64, no
// contraction, correctly rounded sqrt and division).
//
// Three launches per call on one stream, no host round trip for the rows:
//   physical_rows_kernel     one thread per (person, row), blockIdx.y the person.  In the [cols][rows][2] layout consecutive rows are consecutive 16-byte
//                            cells, so a wave's load is one run of 1024 bytes: the velocity kernel's access pattern.  The neighbour cells come from the same
//                            cache lines and their speeds are formed again (two more sqrt per thread) instead of being exchanged.  It
//                            writes s, a, the zone, one mask byte (bits 0 .. 3: hot per kind, bit 4: link) and the step's quantised distance q.  The totals
//                            are integers (a distance is quantised ONCE per step, shape.hip's rule) and one maximum over the bit pattern of a non-negative
//                            double, which orders as an integer: a butterfly per wave and one integer atomic per wave, zone and total, only for the zones
//                            the wave has met.  No floating-point atomic anywhere, so no order of arrival can show.
//   physical_scan_kernel     ONE workgroup of PH_SCAN threads per person walks the rows in chunks of PH_SCAN, as possession_scan_kernel does.  Per kind an
//                            inclusive max-scan of head rows (a wave scan by __shfl_up, the 16 wave totals through LDS, the carry of the chunks before in
//                            registers; a wave folds the 16 totals by a scan of its own, one LDS read per thread) gives the start of the run a row stands
//                            in; the tail rows whose run is long enough go through an add-scan of the same shape and store (first_row, last_row)
//                            compacted, in row order.  Two barriers per chunk.
//   physical_effort_kernel   one thread per effort (after the host has read the counts: the buffer is sized by them, not by the row count) finds its
//                            (person, kind) in the prefix sums of the counts and walks the effort's rows once for the peaks; the walk visits every q of
//                            the effort, so it sums them itself (integers) instead of reading a prefix sum the scan kernel would have had to write per row.
#include "runtime.h"

static_assert(sizeof(EagleLoadParams) == 88 && sizeof(EagleLoadTotals) == 128 && sizeof(EagleLoadEffort) == 48, "include/eagle.h states these sizes");

namespace eagle {

static constexpr int PH_THREADS = 256;         // rows kernel
static constexpr int PH_SCAN = 1024;           // scan kernel: one workgroup per person, 16 waves
static constexpr int PH_WAVES = PH_SCAN / 64;
static constexpr int PH_LINK = 16;             // mask bit 4
static constexpr double PH_CLAMP = 1048576.0;  // metres per step, and the quantum's reciprocal

struct PhysArgs {
    const double2* vel;          // [column][row]
    const int32_t* frames;       // [rows]
    const int32_t* persons;      // person columns in table order
    int rows, npersons;
    double fps;
    int max_gap, minf[2];
    double edges[4], espeed[2], accel;
    double* speed; double* acc; uint8_t* zone;      // [person][row], the result
    uint8_t* mask; long long* q;                    // [person][row], scratch
    int2* pairs; int cap;                           // [person][kind][cap] (first_row, last_row)
    EagleLoadTotals* totals;                        // [person], zeroed in front of the launches
    const int32_t* prefix;                          // [4 persons + 1] efforts in front of each (person, kind)
    EagleLoadEffort* efforts; int n_efforts;
};

__device__ __forceinline__ bool vel_finite(double2 v) { return fabs(v.x) <= 1.7976931348623157e308 && fabs(v.y) <= 1.7976931348623157e308; }
__device__ __forceinline__ double vel_speed(double2 v) { return sqrt(v.x * v.x + v.y * v.y); }

__device__ __forceinline__ long long wave_sum(long long v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(PH_THREADS) void physical_rows_kernel(PhysArgs a)
{
    const int r = blockIdx.x * PH_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = r < a.rows;
    long long fr = 0, fa = 0, fb = 0;
    bool near_a = false, near_b = false;
    if (live) {
        fr = a.frames[r];
        if (r > 0) { fa = a.frames[r - 1]; near_a = fr - fa <= a.max_gap; }
        if (r + 1 < a.rows) { fb = a.frames[r + 1]; near_b = fb - fr <= a.max_gap; }
    }
    for (int p = blockIdx.y; p < a.npersons; p += gridDim.y) {           // (uniform: every lane meets every shuffle)
        const double2* V = a.vel + (size_t)a.persons[p] * a.rows;
        bool pres = false, link = false;
        long long df = 0, q = 0;
        int zs = 0;
        double s = 0.0;
        if (live) {
            const double2 v = V[r];
            pres = vel_finite(v);
            double acc = __longlong_as_double(0x7ff8000000000000ll);
            unsigned zone = EAGLE_LOAD_ABSENT, mask = 0;
            if (pres) {
                s = vel_speed(v);
                double lo = s, hi = s;
                long long flo = fr, fhi = fr;
                if (near_a) { const double2 w = V[r - 1]; if (vel_finite(w)) { link = true; lo = vel_speed(w); flo = fa; } }
                if (near_b) { const double2 w = V[r + 1]; if (vel_finite(w)) { hi = vel_speed(w); fhi = fb; } }
                acc = 0.0;
                if (fhi != flo) acc = (hi - lo) / ((double)(fhi - flo) / a.fps);
                zone = 0;
                #pragma unroll
                for (int k = 0; k < 4; ++k) zone += s >= a.edges[k] ? 1 : 0;
                if (link) {
                    df = fr - fa;
                    const double m = 0.5 * (lo + s);
                    double d = m * ((double)df / a.fps);
                    if (d > PH_CLAMP) d = PH_CLAMP;
                    q = (long long)floor(d * PH_CLAMP + 0.5);
                    #pragma unroll
                    for (int k = 0; k < 4; ++k) zs += m >= a.edges[k] ? 1 : 0;
                    mask = PH_LINK;
                }
                mask |= (s >= a.espeed[0] ? 1 : 0) | (s >= a.espeed[1] ? 2 : 0) | (acc >= a.accel ? 4 : 0) | (acc <= -a.accel ? 8 : 0);
            }
            const size_t o = (size_t)p * a.rows + r;
            a.speed[o] = pres ? s : __longlong_as_double(0x7ff8000000000000ll);
            a.acc[o] = acc; a.zone[o] = (uint8_t)zone; a.mask[o] = (uint8_t)mask; a.q[o] = q;
        }
        // ---- the totals: per wave a butterfly and one integer atomic, for the zones it has met ----
        EagleLoadTotals* T = a.totals + p;
        #pragma unroll
        for (int z = 0; z < 5; ++z) {
            const bool mine = link && zs == z;
            if (__ballot(mine) == 0) continue;                           // (uniform)
            const long long sf = wave_sum(mine ? df : 0), sq = wave_sum(mine ? q : 0);
            if (lane == 0) {
                atomicAdd((unsigned long long*)&T->zone_frames[z], (unsigned long long)sf);
                atomicAdd((unsigned long long*)&T->zone_dist_q[z], (unsigned long long)sq);
            }
        }
        const unsigned long long here = __ballot(pres);
        if (here) {                                                      // (uniform)
            long long top = pres ? __double_as_longlong(s) : 0;          // s >= 0 (or +inf): the bit patterns order as the values do
            #pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { const long long o = __shfl_xor(top, d, 64); top = o > top ? o : top; }
            if (lane == 0) {
                atomicAdd(&T->rows_present, (int)__popcll(here));
                atomicMax((unsigned long long*)&T->top_speed, (unsigned long long)top);
            }
        }
    }
}

__device__ __forceinline__ int ph_max_scan(int v, int lane)
{
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d, 64); if (lane >= d) v = max(v, o); }
    return v;
}

__device__ __forceinline__ int ph_add_scan(int v, int lane)
{
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d, 64); if (lane >= d) v += o; }
    return v;
}

// The 16 wave totals of a chunk (LDS, complete behind a barrier) -> what stands in front of this wave, the chunks before included; `carry` takes the chunk
// in.  Every wave scans the 16 totals in its first 16 lanes and hands out two of them by shuffle: one LDS read per thread instead of sixteen.
template <bool MAX>
__device__ __forceinline__ int ph_fold(const int* tot, int lane, int wave, int& carry)
{
    int v = lane < PH_WAVES ? tot[lane] : (MAX ? -1 : 0);
    #pragma unroll
    for (int d = 1; d < PH_WAVES; d <<= 1) { const int o = __shfl_up(v, d, 64); if (lane >= d) v = MAX ? max(v, o) : v + o; }
    const int all = __shfl(v, PH_WAVES - 1, 64), prev = __shfl(v, wave > 0 ? wave - 1 : 0, 64);      // (wave is uniform)
    const int before = wave == 0 ? carry : (MAX ? max(carry, prev) : carry + prev);
    carry = MAX ? max(carry, all) : carry + all;
    return before;
}

__global__ __launch_bounds__(PH_SCAN) void physical_scan_kernel(PhysArgs a)
{
    __shared__ int s_head[4][PH_WAVES], s_cnt[4][PH_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint8_t* M = a.mask + (size_t)p * a.rows;
    int c_head[4] = {-1, -1, -1, -1}, c_cnt[4] = {0, 0, 0, 0};           // the chunks before this one (registers, the same in every thread)
    for (int base = 0; base < a.rows; base += PH_SCAN) {                 // (uniform: every thread meets every barrier)
        const int r = base + tid;
        const bool live = r < a.rows;
        unsigned m = 0, mp = 0, mn = 0;                                  // the row's mask, the row before's, the next one's (0 beyond the table)
        if (live) {
            m = M[r];
            if (r > 0) mp = M[r - 1];
            if (r + 1 < a.rows) mn = M[r + 1];
        }
        const bool link = (m & PH_LINK) != 0, link_n = (mn & PH_LINK) != 0;
        int w_head[4];
        bool tail[4];
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool hot = (m >> k & 1) != 0;
            const bool head = hot && (!link || !(mp >> k & 1));
            tail[k] = hot && (!link_n || !(mn >> k & 1));                // (the last row: mn == 0)
            w_head[k] = ph_max_scan(head ? r : -1, lane);
            if (lane == 63) s_head[k][wave] = w_head[k];
        }
        __syncthreads();
        int w_cnt[4], start[4];
        bool ev[4];
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int before = ph_fold<true>(s_head[k], lane, wave, c_head[k]);                    // everything in front of this wave
            start[k] = max(before, w_head[k]);
            ev[k] = tail[k] && start[k] >= 0 && (long long)a.frames[r] - (long long)a.frames[start[k]] >= (long long)a.minf[k < 2 ? 0 : 1];
            w_cnt[k] = ph_add_scan(ev[k] ? 1 : 0, lane);
            if (lane == 63) s_cnt[k][wave] = w_cnt[k];
        }
        __syncthreads();
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int off = ph_fold<false>(s_cnt[k], lane, wave, c_cnt[k]) + w_cnt[k] - (ev[k] ? 1 : 0);
            // an effort spans two rows at least and the efforts of a kind are disjoint: off < rows / 2 <= cap (the test keeps a broken mask inside the buffer)
            if (ev[k] && off < a.cap) a.pairs[((size_t)p * 4 + k) * a.cap + off] = make_int2(start[k], r);
        }
        // no barrier here: s_head is read in front of the second barrier and written behind it (the next chunk); s_cnt is read in front of the next
        // chunk's first barrier and written behind it
    }
    #pragma unroll
    for (int k = 0; k < 4; ++k)
        if (tid == k) a.totals[p].efforts[k] = c_cnt[k];
    if (tid == 0) a.totals[p].col = a.persons[p];
}

__global__ __launch_bounds__(256) void physical_effort_kernel(PhysArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_efforts) return;
    int lo = 0, hi = a.npersons * 4;                                     // the (person, kind) with prefix[pk] <= i < prefix[pk + 1]: prefix[0] = 0 <= i < prefix[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (a.prefix[mid] <= i) lo = mid; else hi = mid;
    }
    const int p = lo >> 2, k = lo & 3;
    const int2 pr = a.pairs[(size_t)lo * a.cap + (i - a.prefix[lo])];
    const size_t o = (size_t)p * a.rows;
    double ps = 0.0, pa = 0.0;
    long long dq = 0;
    for (int j = pr.x; j <= pr.y; ++j) {
        const double sj = a.speed[o + j], aj = fabs(a.acc[o + j]);
        if (sj > ps) ps = sj;
        if (aj > pa) pa = aj;
        if (j > pr.x) dq += a.q[o + j];
    }
    EagleLoadEffort e{};
    e.col = a.persons[p]; e.kind = k; e.first_row = pr.x; e.last_row = pr.y;
    e.frames = (int32_t)((long long)a.frames[pr.y] - (long long)a.frames[pr.x]);
    e.distance_q = dq; e.peak_speed = ps; e.peak_accel = pa;
    a.efforts[i] = e;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void physical_check(const char* who, const EagleLoadParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: params is NULL", who);
    if (p->fps <= 0 || p->max_gap <= 0 || p->min_frames[0] <= 0 || p->min_frames[1] <= 0)
        fail(EAGLE_E_INVALID, "%s: fps %d, max_gap %d and min_frames %d, %d must be positive", who, p->fps, p->max_gap, p->min_frames[0], p->min_frames[1]);
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(p->zone_edges[k]) || !(p->zone_edges[k] > 0.0) || (k && !(p->zone_edges[k] > p->zone_edges[k - 1])))
            fail(EAGLE_E_INVALID, "%s: zone_edges %g, %g, %g, %g must be finite, positive and strictly ascending", who, p->zone_edges[0], p->zone_edges[1],
                 p->zone_edges[2], p->zone_edges[3]);
    if (!std::isfinite(p->effort_speed[0]) || !(p->effort_speed[0] > 0.0) || !std::isfinite(p->effort_speed[1]) || !(p->effort_speed[1] > 0.0) ||
        !std::isfinite(p->accel) || !(p->accel > 0.0))
        fail(EAGLE_E_INVALID, "%s: effort_speed %g, %g and accel %g must be finite and positive", who, p->effort_speed[0], p->effort_speed[1], p->accel);
}

// the persons: the Player and Goalkeeper pitch columns in table order
static std::vector<int32_t> physical_columns(const char* who, const EaglePostColumn* columns, int ncols)
{
    std::vector<int32_t> persons;
    for (int c = 0; c < ncols; ++c) {
        const EaglePostColumn& col = columns[c];
        if (col.kind != EAGLE_POST_PLAYER && col.kind != EAGLE_POST_GOALKEEPER && col.kind != EAGLE_POST_BALL && col.kind != EAGLE_POST_BOUNDARY)
            fail(EAGLE_E_INVALID, "%s: column %d is of unknown kind %d", who, c, col.kind);
        if (!col.video && (col.kind == EAGLE_POST_PLAYER || col.kind == EAGLE_POST_GOALKEEPER)) persons.push_back(c);
    }
    return persons;
}

static size_t ph_up(size_t b) { return (std::max<size_t>(b, 16) + 15) & ~(size_t)15; }

// The scratch of one call in a single allocation
struct PhysScratch { size_t persons, mask, q, pairs, totals, prefix, total; int cap; };

static PhysScratch physical_scratch(size_t rows, size_t P)
{
    PhysScratch o{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += ph_up(b); return was; };
    o.cap = (int)std::max<size_t>(rows / 2, 1);
    o.persons = take(P * 4); o.mask = take(P * rows); o.q = take(P * rows * 8); o.pairs = take(P * 4 * (size_t)o.cap * sizeof(int2));
    o.totals = take(P * sizeof(EagleLoadTotals)); o.prefix = take((P * 4 + 1) * 4);
    o.total = at;
    return o;
}

static size_t physical_kept(size_t rows, size_t P) { return std::max<size_t>(P * rows * 17, 16); }      // speed f64 | accel f64 | zone u8

// The three launches on s; the per-row results go to d_speed / d_acc / d_zone ([persons][rows]), totals and efforts to the host.  budget_left: the
// bytes the effort records may take on the device (what the caller's budget leaves beside the result and the scratch); negative: not checked.
static void physical_run(EagleHandle* h, const std::vector<int32_t>& persons, const double2* d_vel, const int32_t* d_frames, int rows, const EagleLoadParams* p,
                         double* d_speed, double* d_acc, uint8_t* d_zone, std::vector<EagleLoadTotals>& totals_out, std::vector<EagleLoadEffort>& efforts_out, hipStream_t s,
                         double budget_left = -1.0)
{
    const size_t P = persons.size();
    totals_out.clear(); efforts_out.clear();
    if (P == 0 || rows <= 0) return;
    const PhysScratch L = physical_scratch((size_t)rows, P);
    uint8_t* base = nullptr;
    EagleLoadEffort* d_ev = nullptr;
    HIP_CHECK(hipMalloc((void**)&base, L.total));
    try {
        HIP_CHECK(hipMemcpyAsync(base + L.persons, persons.data(), P * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(base + L.totals, 0, P * sizeof(EagleLoadTotals), s));
        PhysArgs a{};
        a.vel = d_vel; a.frames = d_frames; a.persons = (const int32_t*)(base + L.persons);
        a.rows = rows; a.npersons = (int)P; a.fps = (double)p->fps; a.max_gap = p->max_gap; a.minf[0] = p->min_frames[0]; a.minf[1] = p->min_frames[1];
        for (int k = 0; k < 4; ++k) a.edges[k] = p->zone_edges[k];
        a.espeed[0] = p->effort_speed[0]; a.espeed[1] = p->effort_speed[1]; a.accel = p->accel;
        a.speed = d_speed; a.acc = d_acc; a.zone = d_zone;
        a.mask = base + L.mask; a.q = (long long*)(base + L.q); a.pairs = (int2*)(base + L.pairs); a.cap = L.cap;
        a.totals = (EagleLoadTotals*)(base + L.totals); a.prefix = (const int32_t*)(base + L.prefix);
        auto rows_k = [&] {
            hipLaunchKernelGGL(physical_rows_kernel, dim3((rows + PH_THREADS - 1) / PH_THREADS, (unsigned)std::min<size_t>(P, 65535)), dim3(PH_THREADS), 0, s, a);
            HIP_CHECK(hipGetLastError());
        };
        auto scan_k = [&] {
            hipLaunchKernelGGL(physical_scan_kernel, dim3((unsigned)P), dim3(PH_SCAN), 0, s, a);
            HIP_CHECK(hipGetLastError());
        };
        // bytes per (person, row): the cell read (its neighbours come from the same lines), 26 written; the scan reads the mask byte and the frame number
        const double cells = (double)P * (double)rows;
        if (h) {
            timed_launch(h, "physical_rows", 42.0 * cells, s, rows_k);
            timed_launch(h, "physical_scan", 5.0 * cells, s, scan_k);
        } else { rows_k(); scan_k(); }
        totals_out.assign(P, EagleLoadTotals{});
        HIP_CHECK(hipMemcpyAsync(totals_out.data(), a.totals, P * sizeof(EagleLoadTotals), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        std::vector<int32_t> prefix(P * 4 + 1, 0);
        long long n = 0;
        for (size_t i = 0; i < P * 4; ++i) {
            const int32_t c = totals_out[i >> 2].efforts[i & 3];
            if (c < 0 || c > L.cap) fail(EAGLE_E_STATE, "physical: %d efforts of one kind from %d rows", c, rows);
            n += c;
            if (n > 0x7fffffffll) fail(EAGLE_E_STATE, "physical: %lld efforts are beyond what one call reports", n);
            prefix[i + 1] = (int32_t)n;
        }
        if (budget_left >= 0.0 && (double)n * sizeof(EagleLoadEffort) > budget_left)
            fail(EAGLE_E_INVALID, "physical: the records of %lld efforts need %.0f bytes of device memory, the budget leaves %.0f", n, (double)n * sizeof(EagleLoadEffort),
                 budget_left);
        efforts_out.assign((size_t)n, EagleLoadEffort{});
        if (n) {
            HIP_CHECK(hipMemcpyAsync(base + L.prefix, prefix.data(), prefix.size() * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMalloc((void**)&d_ev, (size_t)n * sizeof(EagleLoadEffort)));
            a.efforts = d_ev; a.n_efforts = (int)n;
            auto effort_k = [&] {
                hipLaunchKernelGGL(physical_effort_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
                HIP_CHECK(hipGetLastError());
            };
            if (h) timed_launch(h, "physical_effort", 48.0 * (double)n, s, effort_k);
            else effort_k();
            HIP_CHECK(hipMemcpyAsync(efforts_out.data(), d_ev, (size_t)n * sizeof(EagleLoadEffort), hipMemcpyDeviceToHost, s));
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

int eagle_post_physical(EagleHandle* h, EaglePostTable* t, const EagleLoadParams* p)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_physical: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_physical: the table belongs to another handle");
    physical_check("eagle_post_physical", p);
    if (!t->d_vel) fail(EAGLE_E_INVALID, "eagle_post_physical: the table has no velocities (eagle_post_velocities comes first)");
    const std::vector<int32_t> persons = physical_columns("eagle_post_physical", t->columns.data(), t->cols);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)t->rows, P = persons.size();
    double left = 0.0;
    {   // the budget: what this call allocates, the result (once: the columns of a table never change) and the scratch; what it leaves is for the effort
        // records, whose number is known behind the second launch
        double budget = (double)t->max_bytes;
        if (t->max_bytes <= 0) {
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            budget = 0.9 * (double)free_b;
        }
        const double need = (t->d_phys ? 0.0 : (double)physical_kept(rows, P)) + (double)physical_scratch(rows, P).total + (double)rows * 4.0;
        if (need > budget)
            fail(EAGLE_E_INVALID, "eagle_post_physical: %zu persons over %zu rows need %.0f bytes of device memory, the budget is %.0f", P, rows, need, budget);
        left = budget - need;
    }
    if (!t->d_phys) HIP_CHECK(hipMalloc((void**)&t->d_phys, physical_kept(rows, P)));
    t->has_phys = false;                                                 // the per-row arrays are rewritten in place: a call that fails leaves no result
    t->phys_totals.clear(); t->phys_efforts.clear(); t->phys_persons = 0;
    std::vector<EagleLoadTotals> totals;
    std::vector<EagleLoadEffort> efforts;
    if (rows && P) {
        double* d_speed = (double*)t->d_phys;
        const hipStream_t s = h->s_main;
        int32_t* d_frames = nullptr;
        HIP_CHECK(hipMalloc((void**)&d_frames, rows * 4));
        try {
            HIP_CHECK(hipMemcpyAsync(d_frames, t->frames.data(), rows * 4, hipMemcpyHostToDevice, s));
            physical_run(h, persons, (const double2*)t->d_vel, d_frames, t->rows, p, d_speed, d_speed + P * rows, (uint8_t*)(d_speed + 2 * P * rows), totals, efforts, s,
                         left);
        } catch (...) {
            (void)hipStreamSynchronize(s);
            (void)hipFree(d_frames);
            throw;
        }
        HIP_CHECK(hipFree(d_frames));
    }
    t->phys_totals.swap(totals); t->phys_efforts.swap(efforts);
    t->phys_persons = (int)P;
    t->has_phys = true;
    API_END(h)
}

int eagle_post_physical_values(EaglePostTable* t, double* speed, double* accel, uint8_t* zone)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->has_phys) fail(EAGLE_E_INVALID, "eagle_post_physical_values: the table has no physical report (eagle_post_physical)");
    const size_t n = (size_t)t->rows * (size_t)t->phys_persons;
    if (n) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        const double* d = (const double*)t->d_phys;
        if (speed) HIP_CHECK(hipMemcpy(speed, d, n * 8, hipMemcpyDeviceToHost));
        if (accel) HIP_CHECK(hipMemcpy(accel, d + n, n * 8, hipMemcpyDeviceToHost));
        if (zone) HIP_CHECK(hipMemcpy(zone, d + 2 * n, n, hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_post_physical_totals(const EaglePostTable* t, EagleLoadTotals* out, int cap, int* n)
{
    if (!t || !n || cap < 0 || (cap > 0 && !out)) return EAGLE_E_INVALID;
    *n = (int)t->phys_totals.size();
    std::copy(t->phys_totals.begin(), t->phys_totals.begin() + std::min<size_t>(cap, t->phys_totals.size()), out);
    return EAGLE_OK;
}

int eagle_post_physical_efforts(const EaglePostTable* t, EagleLoadEffort* out, int cap, int* n)
{
    if (!t || !n || cap < 0 || (cap > 0 && !out)) return EAGLE_E_INVALID;
    *n = (int)t->phys_efforts.size();
    std::copy(t->phys_efforts.begin(), t->phys_efforts.begin() + std::min<size_t>(cap, t->phys_efforts.size()), out);
    return EAGLE_OK;
}

int eagle_post_device_physical(const EaglePostTable* t, const double** d_speed, const uint8_t** d_zone)
{
    if (!t || !d_speed || !d_zone) return EAGLE_E_INVALID;
    const double* d = t->has_phys ? (const double*)t->d_phys : nullptr;
    *d_speed = d;
    *d_zone = d ? (const uint8_t*)(d + 2 * (size_t)t->rows * (size_t)t->phys_persons) : nullptr;
    return EAGLE_OK;
}

int eagle_op_physical(int device, const double* velocities, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const EagleLoadParams* p,
                      double* speed, double* accel, uint8_t* zone, EagleLoadTotals* totals, int totals_cap, int* n_persons, EagleLoadEffort* efforts,
                      int efforts_cap, int* n_efforts)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!velocities || !frames || !columns || !n_persons || !n_efforts || rows < 0 || cols < 0 || totals_cap < 0 || efforts_cap < 0 || (totals_cap > 0 && !totals) ||
        (efforts_cap > 0 && !efforts))
        fail(EAGLE_E_INVALID, "eagle_op_physical: bad argument (velocities %p, frames %p, columns %p, n_persons %p, n_efforts %p, %d rows, %d columns, totals %p, cap %d, "
             "efforts %p, cap %d)", (const void*)velocities, (const void*)frames, (const void*)columns, (const void*)n_persons, (const void*)n_efforts, rows, cols,
             (const void*)totals, totals_cap, (const void*)efforts, efforts_cap);
    physical_check("eagle_op_physical", p);
    const std::vector<int32_t> persons = physical_columns("eagle_op_physical", columns, cols);
    for (int r = 1; r < rows; ++r)
        if (frames[r] <= frames[r - 1]) fail(EAGLE_E_INVALID, "eagle_op_physical: frame numbers must ascend (row %d: %d after %d)", r, frames[r], frames[r - 1]);
    *n_persons = 0; *n_efforts = 0;
    if (rows == 0 || persons.empty()) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const size_t n = (size_t)rows * persons.size();
    const double2* d_v = (const double2*)net.upload(velocities, (size_t)cols * rows * sizeof(double2));
    const int32_t* d_f = (const int32_t*)net.upload(frames, (size_t)rows * 4);
    double* d_speed = (double*)net.get(physical_kept((size_t)rows, persons.size()));
    std::vector<EagleLoadTotals> tv;
    std::vector<EagleLoadEffort> ev;
    physical_run(nullptr, persons, d_v, d_f, rows, p, d_speed, d_speed + n, (uint8_t*)(d_speed + 2 * n), tv, ev, nullptr);
    if (speed) HIP_CHECK(hipMemcpy(speed, d_speed, n * 8, hipMemcpyDeviceToHost));
    if (accel) HIP_CHECK(hipMemcpy(accel, d_speed + n, n * 8, hipMemcpyDeviceToHost));
    if (zone) HIP_CHECK(hipMemcpy(zone, d_speed + 2 * n, n, hipMemcpyDeviceToHost));
    *n_persons = (int)tv.size(); *n_efforts = (int)ev.size();
    std::copy(tv.begin(), tv.begin() + std::min<size_t>(totals_cap, tv.size()), totals);
    std::copy(ev.begin(), ev.begin() + std::min<size_t>(efforts_cap, ev.size()), efforts);
    API_END(hh)
}

}  // extern "C"
