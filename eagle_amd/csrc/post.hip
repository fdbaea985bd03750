// K20 — the clip post-processor: the records of a finished clip -> the table the reference's Processor.process_data builds with pandas
// (eagle/processor.py:30-403 with filter_ball_detections=False; contract: tests/post_ref.py, pinned by tests/golden/post_golden.json).
//
// Host part (sequential and tiny, like tracker.hip's): column discovery in first-appearance order, the kept frames, the two ball walks, the list
// of (row, column, x, y) entries, the 1 % filter and the goalkeeper fold's pairing.  Device part, two launches on the handle's main stream:
//   post_scatter_kernel  the raw [column][row] table: NaN, then the entries (grouped by column; a workgroup fills and then scatters its own chunk)
//   post_series_kernel   one workgroup per raw column, rows in blocks of 256: statistics, the fold of the column's chain (goalkeeper fold and, with
//                        merge_ids, the stitched fragments of one track), previous / next valid row by wave scans carried between blocks through
//                        LDS, np.interp's gap fill in double, the every-other-row smoothing; 16-byte stores.
// An output column is an ordered chain of members, each a raw column plus the Player column folded in front of it, with the rows the member spans;
// spans ascend and do not overlap, so a row belongs to at most one member and costs at most two raw cells, whatever the chain's length.
// Arithmetic: pandas' method="linear" is np.interp over row positions, slope * (x - x0) + y0 in float64 without contraction (the library is
// built with -ffp-contract=off).  x and y of a cell are interpolated as two series that share their rows.
#include "runtime.h"
#include <climits>

namespace eagle {

static constexpr int PS_THREADS = 256, PS_WAVES = PS_THREADS / 64, SC_ROWS = 1024;
static constexpr int PS_MAX_BLOCKS = 4096;        // dynamic LDS of the series kernel: 8 bytes per 256-row block -> at most 2^20 rows (11 hours at 25 frames/s)

static constexpr int PS_MAX_CHAIN = 100;          // members of a chain: each holds >= 1 % of the rows and their spans are disjoint
struct PostCol { int32_t out, mem0, nmem, fill; };          // per raw column: output column (-1: dropped, folded or stitched away), its chain = members[mem0 .. mem0 + nmem), ball rule
struct PostMember { int32_t first, last, col, pair; };      // rows the member spans, its raw column, the Player column folded in first (-1: none)
struct PostStat { int32_t count, first, last, keep; };      // per raw column, before the fold: valid cells, first / last valid row, count >= 0.01 * rows

__device__ __forceinline__ double post_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool is_nan(double v) { return v != v; }
__device__ __forceinline__ bool cell_present(double2 v) { return !(is_nan(v.x) && is_nan(v.y)); }

__global__ __launch_bounds__(PS_THREADS) void post_scatter_kernel(double2* raw, const int32_t* col_off, const int32_t* ent_row, const double2* ent_xy, int rows, int chunks)
{
    const int c = blockIdx.x / chunks, r0 = (blockIdx.x % chunks) * SC_ROWS, r1 = min(rows, r0 + SC_ROWS);
    double2* A = raw + (size_t)c * rows;
    const double2 nn = make_double2(post_nan(), post_nan());
    for (int r = r0 + threadIdx.x; r < r1; r += PS_THREADS) A[r] = nn;
    __syncthreads();                                  // the chunk's NaN stores are ordered before its entries (same workgroup, same addresses)
    int lo = col_off[c], hi = col_off[c + 1];
    const int e1 = hi;
    while (lo < hi) {                                 // first entry of this column at or behind row r0 (entries of a column ascend by row)
        const int mid = (lo + hi) >> 1;
        if (ent_row[mid] < r0) lo = mid + 1; else hi = mid;
    }
    for (int e = lo + threadIdx.x; e < e1; e += PS_THREADS) {
        const int r = ent_row[e];
        if (r >= r1) break;
        A[r] = ent_xy[e];
    }
}

__device__ __forceinline__ int wave_min(int v) { for (int d = 32; d; d >>= 1) v = min(v, __shfl_xor(v, d, 64)); return v; }
__device__ __forceinline__ int wave_max(int v) { for (int d = 32; d; d >>= 1) v = max(v, __shfl_xor(v, d, 64)); return v; }
__device__ __forceinline__ int wave_sum(int v) { for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
// inclusive scans across the wave's 64 rows: the latest valid row at or before each lane, the earliest at or behind it
__device__ __forceinline__ int wave_scan_max(int v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(v, d, 64); if (lane >= d) v = max(v, o); }
    return v;
}
__device__ __forceinline__ int wave_scan_min_rev(int v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_down(v, d, 64); if (lane + d < 64) v = min(v, o); }
    return v;
}

// the chain of an output column: its members (in LDS), and the only member's two raw columns when there is just one
struct Chain { const double2* raw; const PostMember* mem; const double2* A; const double2* P; int rows, n; };

// the cell of row r after the fold: inside a member Player.combine_first(Goalkeeper); across members the one whose span covers the row
__device__ __forceinline__ double2 folded(const Chain& ch, int r)
{
    const double2* A = ch.A;
    const double2* P = ch.P;
    if (ch.n > 1) {                                    // (uniform) the last member that starts at or before row r
        int lo = 0, hi = ch.n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ch.mem[mid].first <= r) lo = mid + 1; else hi = mid;
        }
        if (lo == 0) return make_double2(post_nan(), post_nan());
        const PostMember m = ch.mem[lo - 1];
        if (r > m.last) return make_double2(post_nan(), post_nan());
        A = ch.raw + (size_t)m.col * ch.rows;
        P = m.pair >= 0 ? ch.raw + (size_t)m.pair * ch.rows : nullptr;
    }
    double2 v = A[r];
    if (P) { const double2 p = P[r]; if (cell_present(p)) v = p; }
    return v;
}
__device__ __forceinline__ double comp(double2 v, int k) { return k ? v.y : v.x; }

// np.interp's expression (numpy compiled_base.c): slope * (x - x0) + y0, with its two fall-backs for a NaN result
__device__ __forceinline__ double lerp_np(double y0, double y1, double x0, double x1, double x)
{
    const double slope = (y1 - y0) / (x1 - x0);
    double v = slope * (x - x0) + y0;
    if (is_nan(v)) {
        v = slope * (x - x1) + y1;
        if (is_nan(v) && y0 == y1) v = y0;
    }
    return v;
}

// component k of row r after the gap fill: p = latest valid row <= r (-1: none), n = earliest valid row >= r (INT_MAX: none)
__device__ __forceinline__ double filled(const Chain& ch, int k, int r, int p, int n, bool fill)
{
    if (p == r) return comp(folded(ch, r), k);
    if (p < 0 || n == INT_MAX) {                       // outside the valid span: the ball's bfill / ffill, or left missing (limit_area="inside")
        if (!fill || (p < 0 && n == INT_MAX)) return post_nan();
        return comp(folded(ch, p < 0 ? n : p), k);
    }
    return lerp_np(comp(folded(ch, p), k), comp(folded(ch, n), k), (double)p, (double)n, (double)r);
}

__global__ __launch_bounds__(PS_THREADS) void post_series_kernel(const double2* raw, double2* out, const PostCol* cols, const PostMember* members, PostStat* stats, int rows, int nblk,
                                                                 int smooth)
{
    extern __shared__ int blk_first[];                 // [nblk][2]: first valid row of the block per component; then the earliest valid row at or behind the block's start
    __shared__ int s_red[3][PS_WAVES];
    __shared__ int s_scan[2][2][PS_WAVES];
    __shared__ double s_f[2][PS_THREADS + 2];
    __shared__ PostMember s_mem[PS_MAX_CHAIN];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const PostCol d = cols[c];
    const double2* A = raw + (size_t)c * rows;
    const int nmem = d.out >= 0 ? min(d.nmem, PS_MAX_CHAIN) : 0;      // (the host refuses longer chains)
    if (tid < nmem) s_mem[tid] = members[d.mem0 + tid];
    for (int i = tid; i < 2 * nblk; i += PS_THREADS) blk_first[i] = INT_MAX;
    __syncthreads();
    Chain ch{raw, s_mem, A, nullptr, rows, nmem};
    if (nmem == 1) {
        const PostMember m = s_mem[0];
        ch.A = raw + (size_t)m.col * rows;
        ch.P = m.pair >= 0 ? raw + (size_t)m.pair * rows : nullptr;
    }
    const bool own = nmem == 1 && ch.A == A;           // (uniform) the chain is this raw column alone: its cell is read once for both uses
    // (a) statistics of the raw column, and per block the first valid row of the folded series
    int cnt = 0, first = INT_MAX, last = -1;
    for (int b = 0; b < nblk; ++b) {
        const int r = b * PS_THREADS + tid;
        int fx = INT_MAX, fy = INT_MAX;
        if (r < rows) {
            double2 v = A[r];
            if (cell_present(v)) { ++cnt; first = min(first, r); last = r; }
            if (own) { if (ch.P) { const double2 p = ch.P[r]; if (cell_present(p)) v = p; } }
            else if (nmem) v = folded(ch, r);
            if (!is_nan(v.x)) fx = r;
            if (!is_nan(v.y)) fy = r;
        }
        fx = wave_min(fx); fy = wave_min(fy);
        if (lane == 0) {
            if (fx != INT_MAX) atomicMin(&blk_first[2 * b], fx);
            if (fy != INT_MAX) atomicMin(&blk_first[2 * b + 1], fy);
        }
    }
    cnt = wave_sum(cnt); first = wave_min(first); last = wave_max(last);
    if (lane == 0) { s_red[0][wave] = cnt; s_red[1][wave] = first; s_red[2][wave] = last; }
    __syncthreads();
    if (tid == 0) {
        PostStat st{0, INT_MAX, -1, 0};
        for (int w = 0; w < PS_WAVES; ++w) { st.count += s_red[0][w]; st.first = min(st.first, s_red[1][w]); st.last = max(st.last, s_red[2][w]); }
        if (st.count == 0) st.first = -1;
        st.keep = (double)st.count >= 0.01 * (double)rows;       // df.notna().sum() >= 0.01 * len(df), proc.py:202
        stats[c] = st;
    }
    if (d.out < 0) return;                              // (uniform) a dropped column, or a Player column folded into its Goalkeeper column
    if (tid < 2) {                                      // suffix minimum over the blocks: the carry of the backward scan
        int run = INT_MAX;
        for (int b = nblk - 1; b >= 0; --b) { run = min(run, blk_first[2 * b + tid]); blk_first[2 * b + tid] = run; }
    }
    __syncthreads();
    double2* O = out + (size_t)d.out * rows;
    const bool fill = d.fill != 0;
    int carry[2] = {-1, -1};                            // latest valid row in front of this block, per component (uniform)
    for (int b = 0; b < nblk; ++b) {
        const int r0 = b * PS_THREADS, r = r0 + tid;
        const bool in = r < rows;
        double2 v = make_double2(post_nan(), post_nan());
        if (in) v = folded(ch, r);                      // (b) the fold
        int p[2], n[2];
        for (int k = 0; k < 2; ++k) {                   // (c) neighbours: forward max-scan, backward min-scan
            const bool ok = in && !is_nan(comp(v, k));
            p[k] = wave_scan_max(ok ? r : -1, lane);
            n[k] = wave_scan_min_rev(ok ? r : INT_MAX, lane);
            if (lane == 63) s_scan[0][k][wave] = p[k];
            if (lane == 0) s_scan[1][k][wave] = n[k];
        }
        __syncthreads();
        double f[2];
        for (int k = 0; k < 2; ++k) {
            const int carry_in = carry[k], next_in = b + 1 < nblk ? blk_first[2 * (b + 1) + k] : INT_MAX;
            int pk = max(p[k], carry_in), nk = min(n[k], next_in), tot = carry_in;
            for (int w = 0; w < PS_WAVES; ++w) {
                if (w < wave) pk = max(pk, s_scan[0][k][w]);
                if (w > wave) nk = min(nk, s_scan[1][k][w]);
                tot = max(tot, s_scan[0][k][w]);
            }
            carry[k] = tot;
            f[k] = in ? filled(ch, k, r, pk, nk, fill) : post_nan();      // (d) gap fill
            if (smooth) {                               // (e) the filled series of this block and of the row on either side of it
                s_f[k][tid + 1] = f[k];
                if (tid == 0) s_f[k][0] = b > 0 ? filled(ch, k, r0 - 1, carry_in, carry_in == r0 - 1 ? r0 - 1 : nk, fill) : post_nan();
                if (tid == PS_THREADS - 1) {
                    const int rn = r0 + PS_THREADS;
                    s_f[k][PS_THREADS + 1] = rn < rows ? filled(ch, k, rn, next_in == rn ? rn : pk, next_in, fill) : post_nan();
                }
            }
        }
        if (smooth) {
            // smooth_df: rows 0, 2, 4, ... are forgotten and interpolated back "inside" from the odd rows.  The filled series is valid on one span of
            // rows (or nowhere), so the nearest valid odd rows around an even row are r - 1 and r + 1, or the row lies outside their span and stays missing
            __syncthreads();
            if (in && !(r & 1)) {
                for (int k = 0; k < 2; ++k) {
                    const double a = s_f[k][tid], z = s_f[k][tid + 2];
                    f[k] = (is_nan(a) || is_nan(z)) ? post_nan() : lerp_np(a, z, (double)(r - 1), (double)(r + 1), (double)r);
                }
            }
        }
        if (in) O[r] = make_double2(f[0], f[1]);
        __syncthreads();                                // s_scan / s_f are rewritten by the next block
    }
}

// K22a — velocities of every cell of a table: one thread per (column, row), the differences of tests/control_ref.py in float64, each operation single and in
// the order written there.  Memory-bound: 16 bytes per cell in (neighbours come from the same cache lines), 16 out.
__device__ __forceinline__ bool cell_finite(double2 v) { return fabs(v.x) <= 1.7976931348623157e308 && fabs(v.y) <= 1.7976931348623157e308; }

__global__ __launch_bounds__(PS_THREADS) void post_velocity_kernel(const double2* values, const int32_t* frames, double2* out, int rows, int cols, double fps, int max_gap,
                                                                   double cap)
{
    const int r = blockIdx.x * PS_THREADS + threadIdx.x;
    if (r >= rows) return;
    const long long fr = frames[r];
    const long long fa = r > 0 ? frames[r - 1] : 0, fb = r + 1 < rows ? frames[r + 1] : 0;
    const bool near_a = r > 0 && fr - fa <= max_gap, near_b = r + 1 < rows && fb - fr <= max_gap;
    for (int c = blockIdx.y; c < cols; c += gridDim.y) {
        const double2* A = values + (size_t)c * rows;
        const double2 p = A[r];
        double2 v = make_double2(post_nan(), post_nan());
        if (cell_finite(p)) {
            double2 lo = p, hi = p;
            long long flo = fr, fhi = fr;
            if (near_a) { const double2 q = A[r - 1]; if (cell_finite(q)) { lo = q; flo = fa; } }
            if (near_b) { const double2 q = A[r + 1]; if (cell_finite(q)) { hi = q; fhi = fb; } }
            v = make_double2(0.0, 0.0);
            if (fhi != flo) {
                const double dt = (double)(fhi - flo) / fps;
                v.x = (hi.x - lo.x) / dt;
                v.y = (hi.y - lo.y) / dt;
            }
            const double s = sqrt(v.x * v.x + v.y * v.y);
            if (s > cap) { const double k = cap / s; v.x = v.x * k; v.y = v.y * k; }
        }
        out[(size_t)c * rows + r] = v;
    }
}

void velocity_check(const EagleKinematicsParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "velocities: params is NULL");
    if (p->fps <= 0 || p->max_gap <= 0 || !(p->speed_cap > 0) || !std::isfinite(p->speed_cap))
        fail(EAGLE_E_INVALID, "velocities: fps %d, max_gap %d and speed_cap %g must be positive (and finite)", p->fps, p->max_gap, p->speed_cap);
}

void velocity_launch(const double2* values, const int32_t* frames, double2* out, int rows, int cols, const EagleKinematicsParams* p, hipStream_t s)
{
    const dim3 grid((unsigned)((rows + PS_THREADS - 1) / PS_THREADS), (unsigned)std::min(cols, 65535));
    hipLaunchKernelGGL(post_velocity_kernel, grid, dim3(PS_THREADS), 0, s, values, frames, out, rows, cols, (double)p->fps, p->max_gap, p->speed_cap);
    HIP_CHECK(hipGetLastError());
}

// ---- host: the sequential part ------------------------------------------------------------------------------------------------------
struct BallCand { double ix, iy, rx, ry, conf; };

// cv2.KalmanFilter.predict() for the reference's 4-state constant-velocity filter (proc.py:506-517), the one step of OpenCV this file leans on.
// ASSUMPTION (unpinned, as tests/post_ref.py::kalman_predict): statePre = transitionMatrix * statePost in float32, then statePost = statePre; statePost
// starts as zeros and the reference only writes statePre, which this overwrites.  Without correct() (filter_ball = 0) the prediction stays at the origin.
static void kalman_predict(float post[4], float pre[4])
{
    pre[0] = post[0] + post[2]; pre[1] = post[1] + post[3]; pre[2] = post[2]; pre[3] = post[3];
    for (int i = 0; i < 4; ++i) post[i] = pre[i];
}

// parse_ball_detections_with_kalman(filter=False), proc.py:321-403, for the image points (real = false) or the pitch points of the candidate lists;
// pos[2 * i]: the chosen candidate of frame i as float32 values, NaN = none.  false: fewer than two sightings (nothing chosen)
static bool ball_walk(const std::vector<std::vector<BallCand>>& cand, bool real, std::vector<double>& pos)
{
    const size_t n = cand.size();
    pos.assign(2 * n, NAN);
    size_t sightings = 0;
    for (const auto& c : cand) sightings += !c.empty();
    if (sightings < 2) return false;                   // the initialisation window (>= 5 entries, >= 2 sightings) runs to the clip's end looking for them
    float post[4] = {0, 0, 0, 0}, pre[4];
    for (size_t i = 0; i < n; ++i) {
        const auto& c = cand[i];
        if (c.empty()) continue;
        size_t best = 0;
        if (c.size() > 1) {
            kalman_predict(post, pre);
            double bd = 0;
            for (size_t k = 0; k < c.size(); ++k) {
                const double dx = (real ? c[k].rx : c[k].ix) - (double)pre[0], dy = (real ? c[k].ry : c[k].iy) - (double)pre[1];
                const double dist = std::sqrt(dx * dx + dy * dy);
                if (k == 0 || dist < bd) { bd = dist; best = k; }      // np.argmin: the first minimum
            }
        }
        pos[2 * i] = (double)(float)(real ? c[best].rx : c[best].ix);
        pos[2 * i + 1] = (double)(float)(real ? c[best].ry : c[best].iy);
    }
    return true;
}

struct PostEntry { int32_t row, col; double x, y; };

static double finite_or_nan(double v) { return std::isfinite(v) ? v : NAN; }

template <typename T> static T* dev_upload(std::vector<void*>& owned, const std::vector<T>& v, hipStream_t s)
{
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, std::max<size_t>(v.size() * sizeof(T), 16)));
    owned.push_back(p);
    if (!v.empty()) HIP_CHECK(hipMemcpyAsync(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return (T*)p;
}

static int team_of(const EaglePostTable* t, int id)
{
    if (t->has_team)
        for (size_t k = 0; k < t->team_ids.size(); ++k)
            if (t->team_ids[k] == id) return t->team_vals[k];
    return -1;
}

// merge_ids = 1: the fragments of one person under several tracker ids become one chain (rule and contract: tests/stitch_ref.py).  A track is a
// person video column after the goalkeeper fold.  A link a -> b needs the same kind, last(a) < first(b), a frame gap g <= int(fps * 1.1), the end
// points at most 10 g pixels apart and no two different known teams; the admissible links, ascending by (distance, gap, column of a, column of b),
// are accepted while a has no successor, b no predecessor and the two chains' teams agree.
struct PostTrack { int col, pair, kind, id, first, last; double fx, fy, lx, ly; int succ, pred, root, team; };
struct PostLink { double d; int g, a, b; };

static void stitch_tracks(std::vector<PostTrack>& tr, const std::vector<int32_t>& frames, int fps, EaglePostTable* t)
{
    const int nt = (int)tr.size(), limit = (int)((double)fps * 1.1);
    std::vector<int> by_first(nt);
    for (int i = 0; i < nt; ++i) by_first[i] = i;
    std::stable_sort(by_first.begin(), by_first.end(), [&](int x, int y) { return tr[x].first < tr[y].first; });
    std::vector<PostLink> links;
    for (int a = 0; a < nt; ++a) {                      // the window of tracks that start behind last(a), within the temporal threshold
        const PostTrack& A = tr[a];
        auto it = std::upper_bound(by_first.begin(), by_first.end(), A.last, [&](int row, int x) { return row < tr[x].first; });
        for (; it != by_first.end(); ++it) {
            const PostTrack& B = tr[*it];
            const int g = frames[B.first] - frames[A.last];
            if (g > limit) break;
            if (B.kind != A.kind) continue;
            const double dx = B.fx - A.lx, dy = B.fy - A.ly;
            const double xx = dx * dx, yy = dy * dy, d = std::sqrt(xx + yy);
            if (d > 10.0 * (double)g) continue;
            if (A.team >= 0 && B.team >= 0 && A.team != B.team) continue;
            links.push_back(PostLink{d, g, a, *it});
        }
    }
    std::sort(links.begin(), links.end(), [&](const PostLink& x, const PostLink& y) {
        if (x.d != y.d) return x.d < y.d;
        if (x.g != y.g) return x.g < y.g;
        if (tr[x.a].col != tr[y.a].col) return tr[x.a].col < tr[y.a].col;
        return tr[x.b].col < tr[y.b].col;
    });
    auto find = [&](int x) { while (tr[x].root != x) x = tr[x].root = tr[tr[x].root].root; return x; };
    for (const PostLink& l : links) {
        if (tr[l.a].succ >= 0 || tr[l.b].pred >= 0) continue;
        const int ra = find(l.a);                       // (b has no predecessor: it heads its chain)
        if (tr[ra].team >= 0 && tr[l.b].team >= 0 && tr[ra].team != tr[l.b].team) continue;
        tr[l.a].succ = l.b; tr[l.b].pred = l.a; tr[l.b].root = ra;
        if (tr[ra].team < 0) tr[ra].team = tr[l.b].team;
        t->merges.push_back(EaglePostMerge{tr[l.a].kind, tr[l.a].id, tr[l.b].id, ra, l.g, -1, l.d});
    }
    for (EaglePostMerge& m : t->merges) {               // head and team of the finished chain
        const PostTrack& H = tr[find(m.head_id)];
        m.head_id = H.id; m.team = H.team;
    }
}

// ball_det (may be NULL): the one reported ball detection of every frame that counts, -1: none (eagle_postprocess_ball)
static void postprocess(EagleHandle* h, const EagleFrameResult* recs, int n, const EaglePostParams* p, EaglePostTable* t, const int32_t* ball_det)
{
    t->h = h;
    if (p->team_ids && p->n_team >= 0) {
        t->has_team = true;
        t->team_ids.assign(p->team_ids, p->team_ids + p->n_team);
        t->team_vals.assign(p->team_vals, p->team_vals + p->n_team);
    }
    // 1. create_dataframe (proc.py:127-203): persons per frame (Player entries, then Goalkeeper entries, keyed by id: a repeated id keeps its first
    //    position and its last value, like the dict it comes from), ball candidates in descending confidence (stable), kept frames, columns
    struct Person { int cls, id; double vx, vy, rx, ry; };
    std::vector<std::vector<Person>> persons(n);
    std::vector<std::vector<BallCand>> balls(n);
    std::map<std::pair<int, int>, int> col_of;          // (class, id) -> raw column of the pitch point; + 1: the video point
    std::vector<EaglePostColumn> raw_cols;
    std::vector<int32_t> kept;
    for (int i = 0; i < n; ++i) {
        const EagleFrameResult& rec = recs[i];
        const int nd = std::max(0, std::min(rec.n_det, EAGLE_MAX_DET));
        std::vector<int> ball_ids;
        for (int want = 0; want < 3; ++want)
            for (int k = 0; k < nd; ++k) {
                const EagleDet& d = rec.det[k];
                if (d.cls != want || !d.reported) continue;
                if (want == 2 && ball_det && ball_det[i] != k) continue;
                const double cx = (double)((d.bx1 & 0xFFFF) + (d.bx2 & 0xFFFF)) / 2.0, cy = (double)(d.by2 & 0xFFFF);      // ((x1 + x2) / 2, y2) of the uint16 "BBox"
                const bool on_pitch = rec.H_valid && d.in_bounds;
                if (want < 2) {
                    Person q{want, d.id, cx, cy, on_pitch ? (double)d.pitch_x : NAN, on_pitch ? (double)d.pitch_y : NAN};
                    auto it = std::find_if(persons[i].begin(), persons[i].end(), [&](const Person& o) { return o.cls == want && o.id == d.id; });
                    if (it != persons[i].end()) *it = q; else persons[i].push_back(q);
                } else {
                    // (a ball without Transformed_Coordinates falls back to its image point: the reference's behaviour, proc.py:169-170)
                    BallCand b{cx, cy, on_pitch ? (double)d.pitch_x : cx, on_pitch ? (double)d.pitch_y : cy, (double)d.conf};
                    auto it = std::find(ball_ids.begin(), ball_ids.end(), d.id);
                    if (it != ball_ids.end()) balls[i][it - ball_ids.begin()] = b; else { ball_ids.push_back(d.id); balls[i].push_back(b); }
                }
            }
        std::stable_sort(balls[i].begin(), balls[i].end(), [](const BallCand& a, const BallCand& b) { return a.conf > b.conf; });
        if (persons[i].empty()) continue;
        if (kept.empty())
            for (int k = 0; k < 4; ++k) raw_cols.push_back(EaglePostColumn{EAGLE_POST_BOUNDARY, k, 0, 0});
        kept.push_back(i);
        for (const Person& q : persons[i])
            if (col_of.emplace(std::make_pair(q.cls, q.id), (int)raw_cols.size()).second) {
                raw_cols.push_back(EaglePostColumn{q.cls == 0 ? EAGLE_POST_PLAYER : EAGLE_POST_GOALKEEPER, q.id, 0, 0});
                raw_cols.push_back(EaglePostColumn{q.cls == 0 ? EAGLE_POST_PLAYER : EAGLE_POST_GOALKEEPER, q.id, 1, 0});
            }
    }
    const int rows = (int)kept.size();
    t->rows = rows; t->frames = kept;
    std::vector<double> ball_img, ball_real;            // (the ball is chosen on the full timeline, kept frames or not)
    const bool enough = ball_walk(balls, false, ball_img);
    ball_walk(balls, true, ball_real);                  // (masked by the image ball, proc.py:192: the same frames by construction)
    if (!enough) t->flags |= EAGLE_POST_NO_BALL;
    if (rows == 0) return;                              // df.empty: the reference returns the empty frame (proc.py:75-76)
    const int c_ball = (int)raw_cols.size();
    raw_cols.push_back(EaglePostColumn{EAGLE_POST_BALL, 0, 0, 0});
    raw_cols.push_back(EaglePostColumn{EAGLE_POST_BALL, 0, 1, 0});
    const int nraw = (int)raw_cols.size();
    const int nblk = (rows + PS_THREADS - 1) / PS_THREADS;
    if (nblk > PS_MAX_BLOCKS) fail(EAGLE_E_INVALID, "%d kept frames: the post-processor handles at most %d per call", rows, PS_MAX_BLOCKS * PS_THREADS);
    // 2. the entries, row by row
    std::vector<PostEntry> ent;
    static const double by[4] = {0, 68, 68, 0};
    for (int r = 0; r < rows; ++r) {
        const int i = kept[r];
        const EagleFrameResult& rec = recs[i];
        if (rec.bounds_valid)
            for (int k = 0; k < 4; ++k) {
                const double x = finite_or_nan(rec.bounds[k]);
                ent.push_back(PostEntry{r, k, x, by[k]});
            }
        for (const Person& q : persons[i]) {
            const int c = col_of[std::make_pair(q.cls, q.id)];
            if (!std::isnan(q.rx)) ent.push_back(PostEntry{r, c, q.rx, q.ry});
            ent.push_back(PostEntry{r, c + 1, q.vx, q.vy});
        }
        if (enough && !std::isnan(ball_img[2 * i])) {
            ent.push_back(PostEntry{r, c_ball, ball_real[2 * i], ball_real[2 * i + 1]});
            ent.push_back(PostEntry{r, c_ball + 1, ball_img[2 * i], ball_img[2 * i + 1]});
        }
    }
    if (ent.size() > (size_t)INT_MAX) fail(EAGLE_E_INVALID, "%zu table entries are beyond the 2^31 - 1 the post-processor indexes", ent.size());
    // 3. the 1 % filter (proc.py:202; boundary and ball columns are always kept) and the goalkeeper fold's pairing (proc.py:206-216)
    std::vector<int32_t> count(nraw, 0), col_off(nraw + 1, 0);
    for (const PostEntry& e : ent) ++count[e.col];
    std::vector<PostCol> desc(nraw);
    std::vector<char> keep(nraw);
    std::vector<int> pair(nraw, -1);
    std::vector<std::vector<PostMember>> chain(nraw);   // per raw column that is an output column: its members
    for (int c = 0; c < nraw; ++c) {
        keep[c] = raw_cols[c].kind >= EAGLE_POST_BALL || (double)count[c] >= 0.01 * (double)rows;
        desc[c] = PostCol{keep[c] ? 0 : -1, 0, 0, raw_cols[c].kind == EAGLE_POST_BALL ? 1 : 0};
        col_off[c + 1] = col_off[c] + count[c];
    }
    for (int c = 0; c < nraw; ++c) {
        if (raw_cols[c].kind != EAGLE_POST_GOALKEEPER || !raw_cols[c].video || !keep[c] || !keep[c - 1]) continue;
        auto it = col_of.find(std::make_pair(0, raw_cols[c].id));
        if (it == col_of.end() || !keep[it->second] || !keep[it->second + 1]) continue;
        pair[c - 1] = it->second; pair[c] = it->second + 1;
        desc[it->second].out = desc[it->second + 1].out = -1;
    }
    // entries grouped by column (stable: rows ascend inside a column)
    std::vector<int32_t> ent_row(ent.size()), fill_at(col_off.begin(), col_off.end() - 1);
    std::vector<double2> ent_xy(ent.size());
    for (const PostEntry& e : ent) { const int k = fill_at[e.col]++; ent_row[k] = e.row; ent_xy[k] = make_double2(e.x, e.y); }
    for (int c = 0; c < nraw; ++c)
        if (desc[c].out >= 0) chain[c].push_back(PostMember{0, rows - 1, c, pair[c]});
    if (p->merge_ids) {
        // 3b. the id merge: tracks = the person video columns after the fold, their spans and end points from the grouped entries
        std::vector<PostTrack> tr;
        for (int c = 0; c < nraw; ++c) {
            if (raw_cols[c].kind >= EAGLE_POST_BALL || !raw_cols[c].video || desc[c].out < 0) continue;
            PostTrack k{c, pair[c], raw_cols[c].kind, raw_cols[c].id, 0, 0, 0, 0, 0, 0, -1, -1, (int)tr.size(), team_of(t, raw_cols[c].id)};
            int ef = col_off[c], el = col_off[c + 1] - 1;          // (a kept column holds at least one entry)
            if (k.pair >= 0) {                                      // Player.combine_first(Goalkeeper): the Player cell wins a shared row
                const int pf = col_off[k.pair], pl = col_off[k.pair + 1] - 1;
                if (ent_row[pf] <= ent_row[ef]) ef = pf;
                if (ent_row[pl] >= ent_row[el]) el = pl;
            }
            k.first = ent_row[ef]; k.fx = ent_xy[ef].x; k.fy = ent_xy[ef].y;
            k.last = ent_row[el]; k.lx = ent_xy[el].x; k.ly = ent_xy[el].y;
            tr.push_back(k);
        }
        stitch_tracks(tr, kept, p->fps, t);
        for (size_t i = 0; i < tr.size(); ++i) {
            if (tr[i].pred >= 0) continue;                          // a head: its chain in time order, for the video and the pitch column
            const int hc = tr[i].col;
            std::vector<PostMember> vid, pit;
            for (int m = (int)i; m >= 0; m = tr[m].succ) {
                const PostTrack& M = tr[m];
                vid.push_back(PostMember{M.first, M.last, M.col, M.pair});
                if (keep[M.col - 1]) pit.push_back(PostMember{M.first, M.last, M.col - 1, M.pair >= 0 ? M.pair - 1 : -1});
                desc[M.col].out = desc[M.col - 1].out = -1;
            }
            if (vid.size() > (size_t)PS_MAX_CHAIN)
                fail(EAGLE_E_STATE, "post-processor: a chain of %zu tracks (each holds 1 %% of the rows and their spans are disjoint: at most %d)", vid.size(), PS_MAX_CHAIN);
            desc[hc].out = 0; chain[hc] = vid;
            chain[hc - 1] = pit;
            if (!pit.empty()) desc[hc - 1].out = 0;
            if (vid.size() > 1 && t->has_team && tr[i].team >= 0 && team_of(t, tr[i].id) < 0) {      // the head inherits the chain's team
                size_t k = 0;                                       // (an entry below 0 is no team: replaced)
                while (k < t->team_ids.size() && t->team_ids[k] != tr[i].id) ++k;
                if (k < t->team_ids.size()) t->team_vals[k] = tr[i].team;
                else { t->team_ids.push_back(tr[i].id); t->team_vals.push_back(tr[i].team); }
            }
        }
    }
    int ncols = 0;
    std::vector<PostMember> members;
    for (int c = 0; c < nraw; ++c)
        if (desc[c].out >= 0) {
            desc[c].out = ncols++; t->columns.push_back(raw_cols[c]);
            desc[c].mem0 = (int32_t)members.size(); desc[c].nmem = (int32_t)chain[c].size();
            members.insert(members.end(), chain[c].begin(), chain[c].end());
        }
    t->cols = ncols;
    // 4. the memory the call needs, against the budget: refused here, never inside a launch
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const double cell = 16.0, need = ((double)nraw + (double)ncols) * (double)rows * cell + (double)ent.size() * 20.0 + (double)nraw * 40.0 + (double)members.size() * 16.0;
    double budget = (double)p->max_bytes;
    if (p->max_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = 0.9 * (double)free_b;
    }
    if (need > budget)
        fail(EAGLE_E_INVALID, "the table of %d rows x %d raw columns (%d kept) needs %.0f bytes of device memory, the budget is %.0f", rows, nraw, ncols, need, budget);
    std::vector<void*> owned;
    const hipStream_t s = h->s_main;
    try {
        double2* d_raw = nullptr;
        HIP_CHECK(hipMalloc((void**)&d_raw, (size_t)nraw * rows * sizeof(double2)));
        owned.push_back(d_raw);
        HIP_CHECK(hipMalloc((void**)&t->d_values, (size_t)ncols * rows * sizeof(double2)));
        const int32_t* d_off = dev_upload(owned, col_off, s);
        const int32_t* d_row = dev_upload(owned, ent_row, s);
        const double2* d_xy = dev_upload(owned, ent_xy, s);
        const PostCol* d_desc = dev_upload(owned, desc, s);
        const PostMember* d_mem = dev_upload(owned, members, s);
        std::vector<PostStat> stats(nraw);
        PostStat* d_stats = dev_upload(owned, stats, s);
        const int chunks = (rows + SC_ROWS - 1) / SC_ROWS;
        const double table_b = (double)nraw * rows * cell, out_b = (double)ncols * rows * cell;
        timed_launch(h, "post_scatter", table_b + (double)ent.size() * 20.0, s, [&] {
            hipLaunchKernelGGL(post_scatter_kernel, dim3((unsigned)(nraw * chunks)), dim3(PS_THREADS), 0, s, d_raw, d_off, d_row, d_xy, rows, chunks);
            HIP_CHECK(hipGetLastError());
        });
        timed_launch(h, "post_series", 2.0 * table_b + out_b, s, [&] {
            hipLaunchKernelGGL(post_series_kernel, dim3((unsigned)nraw), dim3(PS_THREADS), (size_t)nblk * 2 * sizeof(int), s, d_raw, (double2*)t->d_values, d_desc, d_mem,
                               d_stats, rows, nblk, p->smooth ? 1 : 0);
            HIP_CHECK(hipGetLastError());
        });
        HIP_CHECK(hipMemcpyAsync(stats.data(), d_stats, stats.size() * sizeof(PostStat), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h->prof) collect_spans(h);
        for (int c = 0; c < nraw; ++c)                  // the kernel's statistics against the host's bookkeeping that laid the table out
            if (stats[c].count != count[c] || (raw_cols[c].kind < EAGLE_POST_BALL && (stats[c].keep != 0) != (keep[c] != 0)))
                fail(EAGLE_E_STATE, "post-processor: column %d has %d valid cells on the device, %d entries on the host", c, stats[c].count, count[c]);
    } catch (...) {
        for (void* q : owned) (void)hipFree(q);
        throw;
    }
    for (void* q : owned) HIP_CHECK(hipFree(q));
}

static void fetch_host(EaglePostTable* t)
{
    if (t->host_ok) return;
    t->host.resize((size_t)t->cols * t->rows * 2);
    if (!t->host.empty()) {
        HIP_CHECK(hipSetDevice(t->h->cfg.device));
        HIP_CHECK(hipMemcpy(t->host.data(), t->d_values, t->host.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    t->host_ok = true;
}

static EaglePrim post_prim(int kind, int a0, int a1, int a2, int a3, int a4, int a5, const uint8_t* bgr)
{
    EaglePrim p{};
    p.kind = kind;
    p.a[0] = a0; p.a[1] = a1; p.a[2] = a2; p.a[3] = a3; p.a[4] = a4; p.a[5] = a5;
    p.b = bgr[0]; p.g = bgr[1]; p.r = bgr[2];
    return p;
}

}  // namespace eagle

extern "C" {

int eagle_postprocess(EagleHandle* h, const EagleFrameResult* recs, int n, const EaglePostParams* p, EaglePostTable** out)
{
    return eagle_postprocess_ball(h, recs, n, p, nullptr, out);
}

int eagle_postprocess_ball(EagleHandle* h, const EagleFrameResult* recs, int n, const EaglePostParams* p, const int32_t* ball_det, EaglePostTable** out)
{
    API_BEGIN_H(h)
    if (!out) fail(EAGLE_E_INVALID, "eagle_postprocess: out is NULL");
    *out = nullptr;
    if (!p || n < 0 || (n > 0 && !recs)) fail(EAGLE_E_INVALID, "eagle_postprocess: bad argument (params %p, %d records at %p)", (const void*)p, n, (const void*)recs);
    if (p->filter_ball != 0)
        fail(EAGLE_E_INVALID, "eagle_postprocess: filter_ball = %d is refused: the reference's filter_ball_detections=True needs cv2's Kalman gain, which is not restated", p->filter_ball);
    if (p->merge_ids != 0 && p->merge_ids != 1)
        fail(EAGLE_E_INVALID, "eagle_postprocess: merge_ids = %d is refused: 0 keeps the reference's table (its id merge never merges), 1 stitches fragmented ids", p->merge_ids);
    if (p->fps <= 0 || p->frame_w <= 0) fail(EAGLE_E_INVALID, "eagle_postprocess: fps %d and frame_w %d must be positive", p->fps, p->frame_w);
    if (p->n_team < 0 || (p->n_team > 0 && p->team_ids && !p->team_vals)) fail(EAGLE_E_INVALID, "eagle_postprocess: bad team map (%d entries)", p->n_team);
    if (p->max_bytes < 0) fail(EAGLE_E_INVALID, "eagle_postprocess: max_bytes %lld is negative", (long long)p->max_bytes);
    for (int i = 0; ball_det && i < n; ++i) {
        const int k = ball_det[i];
        if (k == -1) continue;
        if (k < 0 || k >= std::min(recs[i].n_det, EAGLE_MAX_DET) || recs[i].det[k].cls != 2 || !recs[i].det[k].reported)
            fail(EAGLE_E_INVALID, "eagle_postprocess_ball: ball_det[%d] = %d is not a reported ball detection of its record (%d detections)", i, k, recs[i].n_det);
    }
    std::unique_ptr<EaglePostTable> t(new EaglePostTable);
    t->max_bytes = p->max_bytes;
    try {
        postprocess(h, recs, n, p, t.get(), ball_det);
    } catch (...) {
        if (t->d_values) (void)hipFree(t->d_values);
        throw;
    }
    *out = t.release();
    API_END(h)
}

void eagle_post_free(EaglePostTable* t)
{
    if (!t) return;
    if (t->d_values || t->d_vel || t->d_poss || t->d_occ || t->d_shape || t->d_phys || t->d_roles || t->d_space || t->d_offside) (void)hipSetDevice(t->h->cfg.device);
    if (t->d_values) (void)hipFree(t->d_values);
    if (t->d_vel) (void)hipFree(t->d_vel);
    if (t->d_raw) (void)hipFree(t->d_raw);
    if (t->d_smooth) (void)hipFree(t->d_smooth);
    if (t->d_flights) (void)hipFree(t->d_flights);
    if (t->d_goalview) (void)hipFree(t->d_goalview);
    if (t->d_orig) (void)hipFree(t->d_orig);
    if (t->d_stab) (void)hipFree(t->d_stab);
    if (t->d_poss) (void)hipFree(t->d_poss);
    if (t->d_occ) (void)hipFree(t->d_occ);
    if (t->d_shape) (void)hipFree(t->d_shape);
    if (t->d_phys) (void)hipFree(t->d_phys);
    if (t->d_roles) (void)hipFree(t->d_roles);
    if (t->d_space) (void)hipFree(t->d_space);
    if (t->d_offside) (void)hipFree(t->d_offside);
    delete t;
}

int eagle_post_velocities(EagleHandle* h, EaglePostTable* t, const EagleKinematicsParams* p)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_velocities: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_velocities: the table belongs to another handle");
    velocity_check(p);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t cells = (size_t)t->cols * t->rows;
    t->host_vel_ok = false;
    if (!t->d_vel) HIP_CHECK(hipMalloc((void**)&t->d_vel, std::max<size_t>(cells * sizeof(double2), 16)));
    t->kin = *p;
    if (cells) {
        std::vector<void*> owned;
        const hipStream_t s = h->s_main;
        try {
            const int32_t* d_frames = dev_upload(owned, t->frames, s);
            timed_launch(h, "post_velocity", 32.0 * (double)cells, s, [&] { velocity_launch((const double2*)t->d_values, d_frames, (double2*)t->d_vel, t->rows, t->cols, p, s); });
            HIP_CHECK(hipStreamSynchronize(s));
            if (h->prof) collect_spans(h);
        } catch (...) {
            for (void* q : owned) (void)hipFree(q);
            throw;
        }
        for (void* q : owned) HIP_CHECK(hipFree(q));
    }
    API_END(h)
}

int eagle_post_velocity_values(EaglePostTable* t, double* values)
{
    if (!t || !values) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->d_vel) fail(EAGLE_E_INVALID, "eagle_post_velocity_values: the table has no velocities (eagle_post_velocities)");
    if (!t->host_vel_ok) {
        t->host_vel.resize((size_t)t->cols * t->rows * 2);
        if (!t->host_vel.empty()) {
            HIP_CHECK(hipSetDevice(h->cfg.device));
            HIP_CHECK(hipMemcpy(t->host_vel.data(), t->d_vel, t->host_vel.size() * sizeof(double), hipMemcpyDeviceToHost));
        }
        t->host_vel_ok = true;
    }
    std::copy(t->host_vel.begin(), t->host_vel.end(), values);
    API_END(h)
}

int eagle_post_device_velocity_values(const EaglePostTable* t, const double** d_values)
{
    if (!t || !d_values) return EAGLE_E_INVALID;
    *d_values = t->d_vel;
    return EAGLE_OK;
}

int eagle_op_velocities(int device, const double* values, const int32_t* frames, int rows, int cols, const EagleKinematicsParams* p, double* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !frames || !out || rows < 0 || cols < 0)
        fail(EAGLE_E_INVALID, "eagle_op_velocities: bad argument (values %p, frames %p, out %p, %d rows, %d columns)", (const void*)values, (const void*)frames, (const void*)out, rows, cols);
    velocity_check(p);
    for (int r = 1; r < rows; ++r)
        if (frames[r] <= frames[r - 1]) fail(EAGLE_E_INVALID, "eagle_op_velocities: frame numbers must ascend (row %d: %d after %d)", r, frames[r], frames[r - 1]);
    const size_t cells = (size_t)rows * cols;
    if (cells == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const double2* d_v = (const double2*)net.upload(values, cells * sizeof(double2));
    const int32_t* d_f = (const int32_t*)net.upload(frames, (size_t)rows * sizeof(int32_t));
    double2* d_o = (double2*)net.get(cells * sizeof(double2));
    velocity_launch(d_v, d_f, d_o, rows, cols, p, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, d_o, cells * sizeof(double2), hipMemcpyDeviceToHost));
    API_END(hh)
}

int eagle_post_shape(const EaglePostTable* t, int32_t* rows, int32_t* cols, int32_t* flags)
{
    if (!t) return EAGLE_E_INVALID;
    if (rows) *rows = t->rows;
    if (cols) *cols = t->cols;
    if (flags) *flags = t->flags;
    return EAGLE_OK;
}

int eagle_post_layout(const EaglePostTable* t, int32_t* frames, EaglePostColumn* columns)
{
    if (!t) return EAGLE_E_INVALID;
    if (frames) std::copy(t->frames.begin(), t->frames.end(), frames);
    if (columns) std::copy(t->columns.begin(), t->columns.end(), columns);
    return EAGLE_OK;
}

int eagle_post_values(EaglePostTable* t, double* values)
{
    if (!t || !values) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    fetch_host(t);
    std::copy(t->host.begin(), t->host.end(), values);
    API_END(h)
}

int eagle_post_merges(const EaglePostTable* t, EaglePostMerge* out, int cap, int* n)
{
    if (!t || !n || cap < 0 || (cap > 0 && !out)) return EAGLE_E_INVALID;
    *n = (int)t->merges.size();
    std::copy(t->merges.begin(), t->merges.begin() + std::min<size_t>(cap, t->merges.size()), out);
    return EAGLE_OK;
}

int eagle_post_device_values(const EaglePostTable* t, const double** d_values)
{
    if (!t || !d_values) return EAGLE_E_INVALID;
    *d_values = t->d_values;
    return EAGLE_OK;
}

int eagle_overlay_from_table(EaglePostTable* t, int row, const EagleFrameResult* rec, EaglePrim* out, int cap, int* n_out)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    static const uint8_t green[3] = {0, 255, 0}, red[3] = {0, 0, 255}, blue[3] = {255, 0, 0}, white[3] = {255, 255, 255};
    if (!out || !n_out || cap < 0 || row < 0 || row >= t->rows) fail(EAGLE_E_INVALID, "eagle_overlay_from_table: bad argument (row %d of %d)", row, t->rows);
    fetch_host(t);
    std::vector<EaglePrim> prims;
    const int lim = (1 << 20) - 64;                     // the annotate kernel's coordinate domain (eagle_overlay_from_record skips what lies outside, too)
    for (int c = 0; c < t->cols; ++c) {                 // main.py:44-73: the video columns in table order
        const EaglePostColumn& col = t->columns[c];
        if (!col.video || col.kind == EAGLE_POST_BOUNDARY) continue;
        const double xd = t->host[((size_t)c * t->rows + row) * 2], yd = t->host[((size_t)c * t->rows + row) * 2 + 1];
        if (std::isnan(xd) || std::isnan(yd) || std::fabs(xd) > lim || std::fabs(yd) > lim) continue;
        const int x = (int)xd, y = (int)yd;             // int(x), int(y)
        if (col.kind == EAGLE_POST_BALL) { prims.push_back(post_prim(EAGLE_PRIM_TRI, x, y - 20, x - 5, y - 30, x + 5, y - 30, green)); continue; }
        const uint8_t* color = green;
        if (col.kind == EAGLE_POST_PLAYER) {
            if (!t->has_team) color = white;
            else {
                size_t k = 0;
                while (k < t->team_ids.size() && t->team_ids[k] != col.id) ++k;
                if (k == t->team_ids.size()) continue;
                color = t->team_vals[k] == 0 ? red : blue;
            }
        }
        prims.push_back(post_prim(EAGLE_PRIM_ARC, x, y, 0, 0, 0, 0, color));
        prims.push_back(post_prim(EAGLE_PRIM_LABEL, x, y, col.id, 0, 0, 0, color));
    }
    if (rec) {                                          // the key-points: the record's own, from the same three sources as eagle_overlay_from_record
        EaglePrim one[EAGLE_MAX_PRIMS]; int k = 0;
        const int rc = eagle_overlay_from_record(rec, nullptr, nullptr, 0, one, EAGLE_MAX_PRIMS, &k);
        if (rc) fail(rc, "eagle_overlay_from_table: the record's overlay failed");
        for (int i = 0; i < k; ++i) if (one[i].kind == EAGLE_PRIM_DISC) prims.push_back(one[i]);
    }
    if ((int)prims.size() > cap) fail(EAGLE_E_INVALID, "the row's overlay has %zu primitives, cap is %d", prims.size(), cap);
    std::copy(prims.begin(), prims.end(), out);
    *n_out = (int)prims.size();
    API_END(h)
}

}  // extern "C"
