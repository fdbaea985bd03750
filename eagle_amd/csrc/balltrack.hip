// K35 — ball track: the ball candidates of a clip -> per frame the candidate on the best physically possible path, the tracklets and the clip's totals
// (include/eagle.h, eagle_ball_track / eagle_op_ball_track; tests/balltrack_ref.py is the written definition of every bit).  Integers only: positions in
// half pixels (<= 131070), cq <= 1024, R <= R0 <= 131070, a link's cost = isqrt(d2) <= 185361, B <= 2^21; f lies within [-2^21, 2^37] for n <= 2^20.
//
// A piece is a maximal run of frames of one shot in which two consecutive frames with candidates lie at most G apart: no link leaves it.  With P the shot's
// maximum before the piece, every f inside is f of the piece run from P = 0 plus P, comparisons and ties included (both sides of every comparison shift by
// P), and a break that found no predecessor inside goes back to the arg-max before the piece when P > 0.
//
//   balltrack_forward_kernel   one wave per piece, frames in order.  Lane l keeps in registers the nodes (position, f) of the last frame whose offset in
//                              the piece is l mod 64: the 64 lanes are the window of G <= 64 frames, no LDS and no barrier.  Each lane loads its own
//                              frame of the next 64 at once (coalesced); a target node is broadcast from its lane, every lane forms the best link from its
//                              frame's nodes as one 64-bit key (biased value, then 64 - (j - i), then 7 - a: the tie rules are the key's order) and
//                              bt_wave_max takes the maximum (DPP rotations inside the rows of 16, v_readlane across them).  Broadcasts are
//                              v_readlane_b32 with a uniform lane.  Lane 0 stores f and the predecessor.
//   balltrack_chain_kernel     one thread per shot walks its pieces: P before each piece and the arg-max a break goes back to; the shot's end node; the score.
//   balltrack_next_kernel      one thread per node: f + P before its piece, and the predecessor as an index (jump table 0).
//   balltrack_double_kernel    jump table k from k - 1.   balltrack_mark_kernel  marked nodes mark their 2^k-th predecessor, k from high to low: every
//                              marked node is a predecessor of an end node, so the set does not depend on the order inside a launch.
//   balltrack_chase_kernel     the other recovery: one lane per shot follows table 0 (kept for comparison: docs/experiments.md).
//   balltrack_rows_kernel      one thread per frame: the record, the tracklet-start flag, the counts (ballots, integer atomics).
//   balltrack_scan_kernel      one workgroup: the inclusive prefix sum of the start flags = tracklet number + 1.
//   balltrack_tracklets_kernel one thread per frame: the tracklet number, and the chosen node's share of its tracklet (integer atomics).
#include "runtime.h"

namespace eagle {

static_assert(sizeof(EagleBallTrackParams) == 64 && sizeof(EagleBallFrame) == 32 && sizeof(EagleBallTracklet) == 48 && sizeof(EagleBallClip) == 64,
              "include/eagle.h states these sizes");
static constexpr int BT_MAXC = EAGLE_BALL_MAX_CAND, BT_MAX_N = 1 << 20, BT_MAX_Q = 2 * 65535;
static constexpr long long BT_BIAS = 1ll << 23;        // f - cost >= -2^21 - 2^18: the biased value of a link is positive, 0 is "no link"
typedef unsigned long long bt_u64;

struct BtArgs {
    // staged by the host
    const int32_t* counts;       // [n] candidates of the frame, ignored ones included
    const int32_t* nstart;       // [n + 1] first node of the frame
    const int2* pos;             // [N]
    const int32_t* cq;           // [N]
    const int32_t* det;          // [N]
    const int32_t* piece_of;     // [N]
    const int2* pieces;          // [S] first and last frame
    const int32_t* shot_piece;   // [shots + 1] first piece of the shot
    const int32_t* cuts;         // [shots - 1]
    int n, N, S, shots, V, G, R0, B;
    // the launches' own
    long long* f;                // [N]
    int32_t* pred;               // [N] >= 0: a link from that node; -1: none; -2 - k: a break from node k
    long long* pieceP;           // [S]
    int32_t* pieceArg;           // [S]
    long long* pieceBefore;      // [S] P of the shot before the piece
    int32_t* pieceCarry;         // [S] its arg-max
    int32_t* shotEnd;            // [shots] the node the path ends in, -1: P(end) = 0
    int32_t* jump;               // [K][N]
    int32_t* mark;               // [N]
    int32_t* starts;             // [n] flag, then its inclusive prefix sum
    EagleBallFrame* frames;      // [n]
    EagleBallTracklet* tracklets;
    EagleBallClip* clip;
};

// floor(sqrt(d2)), d2 < 2^36: the float estimate is off by at most 1 (2^-24 of d2 in the conversion, half an ulp in the root: 0.02 at the largest), the
// integer comparisons decide; nothing depends on how sqrtf rounds
__device__ __forceinline__ long long bt_isqrt(long long d2)
{
    long long r = (long long)__builtin_amdgcn_sqrtf((float)d2);            // (v_sqrt_f32, 1 ulp: still within one of the floor)
    #pragma unroll
    for (int k = 0; k < 2; ++k) r -= r * r > d2 ? 1 : 0;
    #pragma unroll
    for (int k = 0; k < 2; ++k) r += (r + 1) * (r + 1) <= d2 ? 1 : 0;
    return r;
}

__device__ __forceinline__ long long bt_cost(int2 a, int2 b)
{
    const long long dx = a.x - b.x, dy = a.y - b.y;
    return bt_isqrt(dx * dx + dy * dy);
}

// lane `from` of x, `from` uniform over the wave: one v_readlane_b32 instead of a trip through the LDS crossbar
__device__ __forceinline__ int bt_lane(int x, int from) { return __builtin_amdgcn_readlane(x, from); }

// The wave's maximum of a 64-bit key, uniform.  Inside each row of 16 lanes four rotations (DPP row_ror 8, 4, 2, 1: every lane reads a lane of its own
// row, none is invalid) leave the row's maximum in every lane; the four rows are read with v_readlane_b32 and compared as scalars.
__device__ __forceinline__ bt_u64 bt_wave_max(bt_u64 key)
{
    #define BT_ROR_STEP(N)                                                                                        \
        {                                                                                                         \
            const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)key, 0x120 + (N), 0xf, 0xf, false);      \
            const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(key >> 32), 0x120 + (N), 0xf, 0xf, false); \
            const bt_u64 o = ((bt_u64)hi << 32) | lo;                                                             \
            key = o > key ? o : key;                                                                              \
        }
    BT_ROR_STEP(8) BT_ROR_STEP(4) BT_ROR_STEP(2) BT_ROR_STEP(1)
    #undef BT_ROR_STEP
    bt_u64 best = 0;
    #pragma unroll
    for (int row = 0; row < 4; ++row) {
        const bt_u64 o = ((bt_u64)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(key >> 32), 16 * row) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(unsigned)key, 16 * row);
        best = o > best ? o : best;
    }
    return best;
}

__global__ __launch_bounds__(64) void balltrack_forward_kernel(BtArgs a)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const int s0 = a.pieces[s].x, s1 = a.pieces[s].y;
    long long P = 0;
    int parg = -1;
    int cm = 0, cbase = 0, cx[BT_MAXC], cy[BT_MAXC];   // the window frame this lane holds: its nodes, the first one's index
    long long cf[BT_MAXC];
    int nm = 0, nbase = 0, nx[BT_MAXC], ny[BT_MAXC], nr[BT_MAXC];      // the frame of the current 64 this lane loaded
    #pragma unroll
    for (int c = 0; c < BT_MAXC; ++c) { cx[c] = cy[c] = nx[c] = ny[c] = nr[c] = 0; cf[c] = 0; }
    for (int j = s0; j <= s1; ++j) {
        const int lj = (j - s0) & 63;
        if (lj == 0) {
            const int fr = j + lane;
            nm = 0;
            if (fr <= s1) {
                nbase = a.nstart[fr];
                nm = a.nstart[fr + 1] - nbase;
                #pragma unroll
                for (int c = 0; c < BT_MAXC; ++c)
                    if (c < nm) {
                        const int2 q = a.pos[nbase + c];
                        nx[c] = q.x; ny[c] = q.y; nr[c] = (a.cq[nbase + c] * a.R0) >> 10;
                    }
            }
        }
        const int m = bt_lane(nm, lj);
        if (m == 0) {                                  // (uniform)
            if (lane == lj) cm = 0;
            continue;
        }
        const int base = bt_lane(nbase, lj);
        const int delta = lane < lj ? lj - lane : lj - lane + 64;          // this lane's frame is j - delta
        const bool live = delta <= a.G && j - delta >= s0 && cm > 0;
        const long long lim = (long long)a.V * delta, lim2 = lim * lim;
        const long long brk = P - a.B;
        long long fb[BT_MAXC];
        #pragma unroll
        for (int b = 0; b < BT_MAXC; ++b) {
            fb[b] = 0;
            if (b < m) {                               // (uniform)
                const int tx = bt_lane(nx[b], lj), ty = bt_lane(ny[b], lj), R = bt_lane(nr[b], lj);
                bt_u64 key = 0;
                if (live) {
                    #pragma unroll
                    for (int c = 0; c < BT_MAXC; ++c)
                        if (c < cm) {
                            const long long dx = tx - cx[c], dy = ty - cy[c], d2 = dx * dx + dy * dy;
                            if (d2 <= lim2) {
                                const bt_u64 k = ((bt_u64)(cf[c] - bt_isqrt(d2) + BT_BIAS) << 10) | (bt_u64)(((64 - delta) << 3) | (7 - c));
                                key = k > key ? k : key;
                            }
                        }
                }
                key = bt_wave_max(key);
                const long long link = (long long)(key >> 10) - BT_BIAS;
                const int from = bt_lane(cbase, (lj + (int)((key >> 3) & 63)) & 63);           // the winner's lane: lj - (j - i) = lj + (64 - (j - i)) mod 64
                long long val = brk;
                int pr = P > 0 ? -2 - parg : -1;
                if (key != 0 && link >= brk) {
                    val = link;
                    pr = from + (7 - (int)(key & 7));
                }
                fb[b] = R + val;
                if (lane == 0) { a.f[base + b] = fb[b]; a.pred[base + b] = pr; }
            }
        }
        #pragma unroll
        for (int b = 0; b < BT_MAXC; ++b)
            if (b < m && fb[b] > P) { P = fb[b]; parg = base + b; }
        if (lane == lj) {
            cm = m; cbase = base;
            #pragma unroll
            for (int b = 0; b < BT_MAXC; ++b) { cx[b] = nx[b]; cy[b] = ny[b]; cf[b] = fb[b]; }
        }
    }
    if (lane == 0) { a.pieceP[s] = P; a.pieceArg[s] = parg; }
}

__global__ __launch_bounds__(64) void balltrack_chain_kernel(BtArgs a)
{
    const int sh = blockIdx.x * 64 + threadIdx.x;
    if (sh >= a.shots) return;
    long long P = 0;
    int arg = -1;
    for (int s = a.shot_piece[sh]; s < a.shot_piece[sh + 1]; ++s) {
        a.pieceBefore[s] = P; a.pieceCarry[s] = arg;
        const long long p = a.pieceP[s];
        if (p > 0) { P += p; arg = a.pieceArg[s]; }
    }
    a.shotEnd[sh] = P > 0 ? arg : -1;
    if (P > 0) {
        atomicAdd((bt_u64*)&a.clip->score, (bt_u64)P);
        a.mark[arg] = 1;
    }
}

__global__ __launch_bounds__(256) void balltrack_next_kernel(BtArgs a)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= a.N) return;
    const int s = a.piece_of[v], p = a.pred[v];
    const long long before = a.pieceBefore[s];
    a.f[v] += before;
    a.jump[v] = p >= 0 ? p : p <= -2 ? -2 - p : before > 0 ? a.pieceCarry[s] : -1;
}

__global__ __launch_bounds__(256) void balltrack_double_kernel(const int32_t* from, int32_t* to, int N)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N) return;
    const int t = from[v];
    to[v] = t >= 0 ? from[t] : -1;
}

__global__ __launch_bounds__(256) void balltrack_mark_kernel(const int32_t* jump, int32_t* mark, int N)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= N || !mark[v]) return;
    const int t = jump[v];
    if (t >= 0) mark[t] = 1;
}

__global__ __launch_bounds__(64) void balltrack_chase_kernel(BtArgs a)
{
    const int sh = blockIdx.x * 64 + threadIdx.x;
    if (sh >= a.shots) return;
    for (int v = a.shotEnd[sh]; v >= 0; v = a.jump[v]) a.mark[v] = 1;
}

__device__ __forceinline__ int bt_shot_of(const BtArgs& a, int j)      // the cuts at or before j
{
    int lo = 0, hi = a.shots - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.cuts[mid] <= j) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void balltrack_rows_kernel(BtArgs a)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    int with = 0, multi = 0, chosen = 0, nodes = 0, ignored = 0, start = 0;
    if (j < a.n) {
        const int cnt = a.counts[j], base = a.nstart[j], m = a.nstart[j + 1] - base;
        EagleBallFrame o{};
        o.cand = o.det = o.tracklet = -1;
        const int sh = bt_shot_of(a, j);
        o.flags = (cnt > BT_MAXC ? EAGLE_BALL_TOO_MANY : 0) | (j == 0 || (sh > 0 && a.cuts[sh - 1] == j) ? EAGLE_BALL_SHOT_START : 0);
        for (int b = 0; b < m; ++b)
            if (a.mark[base + b]) {                    // (at most one: the path passes a frame once)
                const int2 q = a.pos[base + b];
                o.cand = b; o.det = a.det[base + b]; o.qx = q.x; o.qy = q.y; o.f = a.f[base + b];
                start = a.pred[base + b] < 0 ? 1 : 0;
                chosen = 1;
            }
        if (start) o.flags |= EAGLE_BALL_TRACKLET_START;
        a.frames[j] = o;
        a.starts[j] = start;
        with = cnt > 0; multi = cnt > 1; nodes = m; ignored = cnt - m;
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        with += __shfl_xor(with, d, 64); multi += __shfl_xor(multi, d, 64); chosen += __shfl_xor(chosen, d, 64);
        nodes += __shfl_xor(nodes, d, 64); ignored += __shfl_xor(ignored, d, 64); start += __shfl_xor(start, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (with) atomicAdd(&a.clip->frames_with, with);
        if (multi) atomicAdd(&a.clip->frames_multi, multi);
        if (chosen) atomicAdd(&a.clip->frames_chosen, chosen);
        if (nodes - chosen) atomicAdd(&a.clip->rejected, nodes - chosen);
        if (ignored) atomicAdd(&a.clip->ignored, ignored);
        if (start) atomicAdd(&a.clip->tracklets, start);
    }
}

__global__ __launch_bounds__(1024) void balltrack_scan_kernel(int32_t* v, int n)
{
    __shared__ int part[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + threadIdx.x;
        int x = i < n ? v[i] : 0;
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(x, d, 64);
            if (lane >= d) x += o;
        }
        if (lane == 63) part[wave] = x;
        __syncthreads();
        int before = 0, total = 0;
        #pragma unroll
        for (int w = 0; w < 16; ++w) { before += w < wave ? part[w] : 0; total += part[w]; }
        if (i < n) v[i] = carry + before + x;
        carry += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void balltrack_tracklets_kernel(BtArgs a)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.n) return;
    const int b = a.frames[j].cand;
    if (b < 0) return;
    const int t = a.starts[j] - 1, v = a.nstart[j] + b, p = a.pred[v];
    a.frames[j].tracklet = t;
    EagleBallTracklet* T = a.tracklets + t;
    const int cq = a.cq[v];
    long long gain = (cq * a.R0) >> 10;
    if (p >= 0) {
        const long long c = bt_cost(a.pos[v], a.pos[p]);
        gain -= c;
        if (c) atomicAdd((bt_u64*)&T->length, (bt_u64)c);
    } else {
        gain -= a.B;
        T->first = j; T->shot = bt_shot_of(a, j);
    }
    atomicMax(&T->last, j);
    atomicAdd(&T->sightings, 1);
    atomicAdd((bt_u64*)&T->sum_cq, (bt_u64)cq);
    atomicAdd((bt_u64*)&T->gain, (bt_u64)gain);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct BtResolved { int V, G, R0, B; };

static int bt_quantise(double v) { return (int)std::floor(2.0 * v + 0.5); }

static BtResolved balltrack_check(const char* who, const EagleBallTrackParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the ball-track parameters are NULL", who);
    if (p->fps <= 0 || p->frame_w <= 0) fail(EAGLE_E_INVALID, "%s: fps %d and frame_w %d must be positive", who, p->fps, p->frame_w);
    if (p->gap < 0 || p->gap > 64) fail(EAGLE_E_INVALID, "%s: gap %d lies outside 1 .. 64 (0: the default)", who, p->gap);
    const double lim[3] = {65535.0, 65535.0, 1048576.0}, val[3] = {p->speed, p->reward, p->brk};
    static const char* const names[3] = {"speed", "reward", "brk"};
    for (int k = 0; k < 3; ++k)
        if (!(std::isfinite(val[k]) && val[k] >= 0.0 && val[k] <= lim[k]))
            fail(EAGLE_E_INVALID, "%s: %s %g must be finite and within [0, %.0f] pixels", who, names[k], val[k], lim[k]);
    for (int k = 0; k < 5; ++k)
        if (p->reserved[k]) fail(EAGLE_E_INVALID, "%s: reserved word %d of the ball-track parameters is %d, not 0", who, k, p->reserved[k]);
    if (p->max_bytes < 0) fail(EAGLE_E_INVALID, "%s: max_bytes %lld is negative", who, (long long)p->max_bytes);
    if (p->speed == 0.0 && 0.1 * (double)p->frame_w > 65535.0) fail(EAGLE_E_INVALID, "%s: frame_w %d: the default speed exceeds 65535 pixels", who, p->frame_w);
    BtResolved r;
    r.V = p->speed != 0.0 ? bt_quantise(p->speed) : bt_quantise(0.1 * (double)p->frame_w);
    r.G = p->gap ? p->gap : std::min(64, p->fps);
    r.R0 = p->reward != 0.0 ? bt_quantise(p->reward) : r.V;
    r.B = p->brk != 0.0 ? bt_quantise(p->brk) : (5 * r.R0) >> 1;
    return r;
}

static void balltrack_cuts_check(const char* who, int n, const int32_t* cuts, int n_cuts)
{
    if (n_cuts < 0 || (n_cuts > 0 && !cuts)) fail(EAGLE_E_INVALID, "%s: %d cuts at %p", who, n_cuts, (const void*)cuts);
    for (int k = 0; k < n_cuts; ++k) {
        if (cuts[k] < 1 || cuts[k] > n - 1) fail(EAGLE_E_INVALID, "%s: cut %d (frame %d) lies outside 1 .. %d", who, k, cuts[k], n - 1);
        if (k && cuts[k] <= cuts[k - 1]) fail(EAGLE_E_INVALID, "%s: cut %d (frame %d) does not lie behind cut %d (frame %d)", who, k, cuts[k], k - 1, cuts[k - 1]);
    }
}

// the candidates as the launches read them: the nodes only
struct BtStaged {
    std::vector<int32_t> counts, nstart, cq, det, piece_of, shot_piece;
    std::vector<int2> pos, pieces;
    int n = 0, frames_with = 0;
};

// counts / nstart / pos / cq / det are filled; the pieces of every shot from them
static void balltrack_pieces(BtStaged& st, const int32_t* cuts, int n_cuts, int G)
{
    const int n = st.n;
    st.piece_of.assign(st.pos.size(), 0);
    st.shot_piece.assign(1, 0);
    int cut = 0, last = -1;                            // the last frame with nodes of the current shot
    for (int j = 0; j < n; ++j) {
        if (cut < n_cuts && cuts[cut] == j) { ++cut; last = -1; st.shot_piece.push_back((int)st.pieces.size()); }
        const int m = st.nstart[j + 1] - st.nstart[j];
        if (st.counts[j] > 0) ++st.frames_with;
        if (!m) continue;
        if (last >= 0 && j - last <= G) st.pieces.back().y = j; else st.pieces.push_back(make_int2(j, j));
        last = j;
        for (int k = st.nstart[j]; k < st.nstart[j + 1]; ++k) st.piece_of[k] = (int)st.pieces.size() - 1;
    }
    st.shot_piece.push_back((int)st.pieces.size());
}

static size_t bt_up(size_t b) { return (std::max<size_t>(b, 16) + 255) & ~(size_t)255; }

static int bt_rounds(int frames_with)                  // tables 0 .. K - 1 reach 2^K - 1 > any path's length - 1
{
    int K = 1;
    while ((1ll << K) < (long long)frames_with) ++K;
    return K;
}

struct BtResult { std::vector<EagleBallFrame> frames; std::vector<EagleBallTracklet> tracklets; EagleBallClip clip{}; };

// The whole stage (n > 0): stage st -> res on the host.  Everything is checked; the budget is held before the first allocation.
static void balltrack_run(EagleHandle* h, const char* who, const BtStaged& st, int shots, const int32_t* cuts, const BtResolved& r, int recover, int64_t max_bytes,
                          hipStream_t s, BtResult& res, float* times_ms)
{
    const int n = st.n, N = (int)st.pos.size(), S = (int)st.pieces.size();
    const int K = recover == EAGLE_BALL_RECOVER_CHASE ? 1 : bt_rounds(st.frames_with);
    const size_t cap = (size_t)std::min(n, std::max(st.frames_with, 1));
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += bt_up(b); return was; };
    const size_t o_counts = take((size_t)n * 4), o_nstart = take(((size_t)n + 1) * 4), o_pos = take((size_t)N * 8), o_cq = take((size_t)N * 4), o_det = take((size_t)N * 4),
                 o_piece_of = take((size_t)N * 4), o_pieces = take((size_t)S * 8), o_shot_piece = take(((size_t)shots + 1) * 4), o_cuts = take((size_t)shots * 4),
                 o_f = take((size_t)N * 8), o_pred = take((size_t)N * 4), o_pP = take((size_t)S * 8), o_pArg = take((size_t)S * 4), o_pBefore = take((size_t)S * 8),
                 o_pCarry = take((size_t)S * 4), o_shotEnd = take((size_t)shots * 4), o_jump = take((size_t)K * (size_t)N * 4), o_zero = at;
    // behind o_zero: what starts as zeros
    const size_t o_mark = take((size_t)N * 4), o_starts = take((size_t)n * 4), o_frames = take((size_t)n * sizeof(EagleBallFrame)), o_tracklets = take(cap * sizeof(EagleBallTracklet)),
                 o_clip = take(sizeof(EagleBallClip)), total = at;
    double budget = (double)max_bytes;
    if (max_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = 0.9 * (double)free_b;
    }
    if ((double)total > budget) fail(EAGLE_E_INVALID, "%s: the call needs %.0f bytes of device memory, the budget is %.0f", who, (double)total, budget);
    uint8_t* d = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    try {
        HIP_CHECK(hipMalloc((void**)&d, total));
        BtArgs a{};
        a.counts = (const int32_t*)(d + o_counts); a.nstart = (const int32_t*)(d + o_nstart); a.pos = (const int2*)(d + o_pos); a.cq = (const int32_t*)(d + o_cq);
        a.det = (const int32_t*)(d + o_det); a.piece_of = (const int32_t*)(d + o_piece_of); a.pieces = (const int2*)(d + o_pieces);
        a.shot_piece = (const int32_t*)(d + o_shot_piece); a.cuts = (const int32_t*)(d + o_cuts);
        a.n = n; a.N = N; a.S = S; a.shots = shots; a.V = r.V; a.G = r.G; a.R0 = r.R0; a.B = r.B;
        a.f = (long long*)(d + o_f); a.pred = (int32_t*)(d + o_pred); a.pieceP = (long long*)(d + o_pP); a.pieceArg = (int32_t*)(d + o_pArg);
        a.pieceBefore = (long long*)(d + o_pBefore); a.pieceCarry = (int32_t*)(d + o_pCarry); a.shotEnd = (int32_t*)(d + o_shotEnd); a.jump = (int32_t*)(d + o_jump);
        a.mark = (int32_t*)(d + o_mark); a.starts = (int32_t*)(d + o_starts); a.frames = (EagleBallFrame*)(d + o_frames);
        a.tracklets = (EagleBallTracklet*)(d + o_tracklets); a.clip = (EagleBallClip*)(d + o_clip);
        auto up = [&](const void* dst, const void* src, size_t b) {
            if (b) HIP_CHECK(hipMemcpyAsync((void*)dst, src, b, hipMemcpyHostToDevice, s));
        };
        up(a.counts, st.counts.data(), (size_t)n * 4); up(a.nstart, st.nstart.data(), ((size_t)n + 1) * 4); up(a.pos, st.pos.data(), (size_t)N * 8);
        up(a.cq, st.cq.data(), (size_t)N * 4); up(a.det, st.det.data(), (size_t)N * 4); up(a.piece_of, st.piece_of.data(), (size_t)N * 4);
        up(a.pieces, st.pieces.data(), (size_t)S * 8); up(a.shot_piece, st.shot_piece.data(), ((size_t)shots + 1) * 4); up(a.cuts, cuts, ((size_t)shots - 1) * 4);
        HIP_CHECK(hipMemsetAsync(d + o_zero, 0, total - o_zero, s));
        EagleBallClip clip0{};
        clip0.shots = shots; clip0.V = r.V; clip0.G = r.G; clip0.R0 = r.R0; clip0.B = r.B;
        up(a.clip, &clip0, sizeof(clip0));
        if (times_ms)
            for (int k = 0; k < 4; ++k) HIP_CHECK(hipEventCreate(&ev[k]));
        auto stamp = [&](int k) { if (times_ms) HIP_CHECK(hipEventRecord(ev[k], s)); };
        auto run = [&](const char* name, double bytes, const std::function<void()>& fn) {
            if (h) timed_launch(h, name, bytes, s, fn); else fn();
            HIP_CHECK(hipGetLastError());
        };
        const unsigned gN = (unsigned)((N + 255) / 256), gn = (unsigned)((n + 255) / 256), gs = (unsigned)((shots + 63) / 64);
        stamp(0);
        if (S) run("balltrack_forward", 28.0 * N + 8.0 * n, [&] { hipLaunchKernelGGL(balltrack_forward_kernel, dim3((unsigned)S), dim3(64), 0, s, a); });
        run("balltrack_chain", 32.0 * S + 8.0 * shots, [&] { hipLaunchKernelGGL(balltrack_chain_kernel, dim3(gs), dim3(64), 0, s, a); });
        if (N) run("balltrack_next", 32.0 * N, [&] { hipLaunchKernelGGL(balltrack_next_kernel, dim3(gN), dim3(256), 0, s, a); });
        stamp(1);
        if (N && recover == EAGLE_BALL_RECOVER_CHASE) {
            run("balltrack_chase", 8.0 * st.frames_with, [&] { hipLaunchKernelGGL(balltrack_chase_kernel, dim3(gs), dim3(64), 0, s, a); });
        } else if (N) {
            run("balltrack_double", 12.0 * N * (K - 1), [&] {
                for (int k = 1; k < K; ++k) hipLaunchKernelGGL(balltrack_double_kernel, dim3(gN), dim3(256), 0, s, a.jump + (size_t)(k - 1) * N, a.jump + (size_t)k * N, N);
            });
            run("balltrack_mark", 8.0 * N * K, [&] {
                for (int k = K - 1; k >= 0; --k) hipLaunchKernelGGL(balltrack_mark_kernel, dim3(gN), dim3(256), 0, s, a.jump + (size_t)k * N, a.mark, N);
            });
        }
        stamp(2);
        run("balltrack_rows", 44.0 * n + 4.0 * N, [&] { hipLaunchKernelGGL(balltrack_rows_kernel, dim3(gn), dim3(256), 0, s, a); });
        run("balltrack_scan", 8.0 * n, [&] { hipLaunchKernelGGL(balltrack_scan_kernel, dim3(1), dim3(1024), 0, s, a.starts, n); });
        run("balltrack_tracklets", 12.0 * n + 64.0 * st.frames_with, [&] { hipLaunchKernelGGL(balltrack_tracklets_kernel, dim3(gn), dim3(256), 0, s, a); });
        stamp(3);
        HIP_CHECK(hipStreamSynchronize(s));
        if (h && h->prof) collect_spans(h);
        if (times_ms) {
            for (int k = 0; k < 3; ++k) HIP_CHECK(hipEventElapsedTime(&times_ms[k], ev[k], ev[k + 1]));
            HIP_CHECK(hipEventElapsedTime(&times_ms[3], ev[0], ev[3]));
        }
        res.frames.resize((size_t)n);
        HIP_CHECK(hipMemcpy(res.frames.data(), a.frames, (size_t)n * sizeof(EagleBallFrame), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&res.clip, a.clip, sizeof(EagleBallClip), hipMemcpyDeviceToHost));
        if (res.clip.tracklets < 0 || (size_t)res.clip.tracklets > cap) fail(EAGLE_E_HIP, "%s: %d tracklets from %d frames with candidates", who, res.clip.tracklets, st.frames_with);
        res.tracklets.resize((size_t)res.clip.tracklets);
        if (res.clip.tracklets) HIP_CHECK(hipMemcpy(res.tracklets.data(), a.tracklets, res.tracklets.size() * sizeof(EagleBallTracklet), hipMemcpyDeviceToHost));
    } catch (...) {
        (void)hipStreamSynchronize(s);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (d) (void)hipFree(d);
        throw;
    }
    for (hipEvent_t e : ev) if (e) HIP_CHECK(hipEventDestroy(e));
    HIP_CHECK(hipFree(d));
}

// the reported ball detections of a record in eagle_postprocess's order (post.hip, create_dataframe): one per id, a later record of an id in the earlier
// one's place, then stably by descending confidence -> indices into rec.det
static void balltrack_candidates(const EagleFrameResult& rec, std::vector<int>& out)
{
    out.clear();
    const int nd = rec.n_det;
    std::vector<int> ids;
    for (int k = 0; k < nd; ++k) {
        const EagleDet& d = rec.det[k];
        if (d.cls != 2 || !d.reported) continue;
        auto it = std::find(ids.begin(), ids.end(), d.id);
        if (it != ids.end()) out[it - ids.begin()] = k; else { ids.push_back(d.id); out.push_back(k); }
    }
    std::stable_sort(out.begin(), out.end(), [&](int x, int y) { return (double)rec.det[x].conf > (double)rec.det[y].conf; });
}

static int bt_cq(const char* who, float conf, int frame, int k)
{
    if (!(std::isfinite(conf) && conf >= 0.0f && conf <= 1.0f)) fail(EAGLE_E_INVALID, "%s: frame %d, candidate %d: conf %g is not finite or lies outside [0, 1]", who, frame, k, (double)conf);
    return (int)std::floor((double)conf * 1024.0);
}

}  // namespace eagle

struct EagleBallTrack { eagle::BtResult res; };

extern "C" {

int eagle_ball_track(EagleHandle* h, const EagleFrameResult* recs, int n, const int32_t* cuts, int n_cuts, const EagleBallTrackParams* p, EagleBallTrack** out)
{
    API_BEGIN_H(h)
    const char* who = "eagle_ball_track";
    if (!out) fail(EAGLE_E_INVALID, "%s: out is NULL", who);
    if (n < 0 || n > BT_MAX_N || (n > 0 && !recs)) fail(EAGLE_E_INVALID, "%s: %d records at %p (at most %d)", who, n, (const void*)recs, BT_MAX_N);
    const BtResolved r = balltrack_check(who, p);
    balltrack_cuts_check(who, n, cuts, n_cuts);
    BtStaged st;
    st.n = n;
    st.counts.resize((size_t)n); st.nstart.assign((size_t)n + 1, 0);
    std::vector<int> cand;
    for (int i = 0; i < n; ++i) {
        const EagleFrameResult& rec = recs[i];
        if (rec.n_det < 0 || rec.n_det > EAGLE_MAX_DET) fail(EAGLE_E_INVALID, "%s: record %d: n_det %d lies outside 0 .. %d", who, i, rec.n_det, EAGLE_MAX_DET);
        balltrack_candidates(rec, cand);
        st.counts[i] = (int)cand.size();
        const int m = std::min((int)cand.size(), BT_MAXC);
        for (int k = 0; k < (int)cand.size(); ++k) {
            const EagleDet& d = rec.det[cand[k]];
            const int cq = bt_cq(who, d.conf, i, k);
            if (k >= m) continue;
            st.pos.push_back(make_int2((d.bx1 & 0xFFFF) + (d.bx2 & 0xFFFF), 2 * (d.by2 & 0xFFFF)));
            st.cq.push_back(cq); st.det.push_back(cand[k]);
        }
        st.nstart[i + 1] = st.nstart[i] + m;
    }
    std::unique_ptr<EagleBallTrack> t(new EagleBallTrack);
    if (n) {
        balltrack_pieces(st, cuts, n_cuts, r.G);
        HIP_CHECK(hipSetDevice(h->cfg.device));
        balltrack_run(h, who, st, n_cuts + 1, cuts, r, EAGLE_BALL_RECOVER_DEFAULT, p->max_bytes, h->s_main, t->res, nullptr);
    }
    *out = t.release();
    API_END(h)
}

int eagle_ball_track_values(const EagleBallTrack* t, EagleBallFrame* frames_out, EagleBallClip* clip_out)
{
    if (!t) return EAGLE_E_INVALID;
    if (frames_out) std::copy(t->res.frames.begin(), t->res.frames.end(), frames_out);
    if (clip_out) *clip_out = t->res.clip;
    return EAGLE_OK;
}

int eagle_ball_track_tracklets(const EagleBallTrack* t, EagleBallTracklet* out, int cap, int* n)
{
    if (!t || !n || cap < 0 || (cap > 0 && !out)) return EAGLE_E_INVALID;
    *n = (int)t->res.tracklets.size();
    std::copy(t->res.tracklets.begin(), t->res.tracklets.begin() + std::min(cap, *n), out);
    return EAGLE_OK;
}

void eagle_ball_track_free(EagleBallTrack* t) { delete t; }

int eagle_op_ball_track(int device, const int32_t* counts, int n, const int32_t* positions, const int32_t* cq, const float* conf, const int32_t* det,
                        const int32_t* cuts, int n_cuts, const EagleBallTrackParams* p, int recover, EagleBallFrame* frames_out, EagleBallTracklet* tracklets_out,
                        int cap, EagleBallClip* clip_out, float* times_ms)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_ball_track";
    if (n < 0 || n > BT_MAX_N || (n > 0 && (!counts || !positions || (!cq && !conf))) || cap < 0)
        fail(EAGLE_E_INVALID, "%s: bad argument (%d frames of at most %d, counts %p, positions %p, cq %p, conf %p, cap %d)", who, n, BT_MAX_N, (const void*)counts,
             (const void*)positions, (const void*)cq, (const void*)conf, cap);
    if (recover != EAGLE_BALL_RECOVER_DEFAULT && recover != EAGLE_BALL_RECOVER_DOUBLING && recover != EAGLE_BALL_RECOVER_CHASE)
        fail(EAGLE_E_INVALID, "%s: recover %d is none of EAGLE_BALL_RECOVER_DEFAULT, _DOUBLING, _CHASE", who, recover);
    const BtResolved r = balltrack_check(who, p);
    balltrack_cuts_check(who, n, cuts, n_cuts);
    BtStaged st;
    st.n = n;
    st.counts.assign(counts, counts + n); st.nstart.assign((size_t)n + 1, 0);
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        if (counts[i] < 0 || counts[i] > EAGLE_MAX_DET) fail(EAGLE_E_INVALID, "%s: frame %d: %d candidates lie outside 0 .. %d", who, i, counts[i], EAGLE_MAX_DET);
        const int m = std::min(counts[i], BT_MAXC);
        for (int k = 0; k < counts[i]; ++k, ++at) {
            const int qx = positions[2 * at], qy = positions[2 * at + 1];
            if (qx < 0 || qx > BT_MAX_Q || qy < 0 || qy > BT_MAX_Q) fail(EAGLE_E_INVALID, "%s: frame %d, candidate %d: position (%d, %d) lies outside 0 .. %d half pixels", who, i, k, qx, qy, BT_MAX_Q);
            const int c = cq ? cq[at] : bt_cq(who, conf[at], i, k);
            if (c < 0 || c > 1024) fail(EAGLE_E_INVALID, "%s: frame %d, candidate %d: cq %d lies outside 0 .. 1024", who, i, k, c);
            if (k >= m) continue;
            st.pos.push_back(make_int2(qx, qy)); st.cq.push_back(c); st.det.push_back(det ? det[at] : -1);
        }
        st.nstart[i + 1] = st.nstart[i] + m;
    }
    if (n == 0) return EAGLE_OK;
    balltrack_pieces(st, cuts, n_cuts, r.G);
    HIP_CHECK(hipSetDevice(device));
    BtResult res;
    float times[4] = {0, 0, 0, 0};
    balltrack_run(nullptr, who, st, n_cuts + 1, cuts, r, recover, p->max_bytes, nullptr, res, times_ms ? times : nullptr);
    if (frames_out) std::copy(res.frames.begin(), res.frames.end(), frames_out);
    if (tracklets_out) std::copy(res.tracklets.begin(), res.tracklets.begin() + std::min((size_t)cap, res.tracklets.size()), tracklets_out);
    if (clip_out) *clip_out = res.clip;
    if (times_ms) std::copy(times, times + 4, times_ms);
    API_END(hh)
}

}  // extern "C"
