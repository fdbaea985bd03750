// K38: the estimate of one row's common motion by one wave, and stab_estimate_kernel, the form of it that the library runs (csrc/stab.hip includes this
// inside namespace eagle; include/eagle.h states the rule, tests/stab_ref.py defines every bit).  It is a file of its own because tools/stab_rate.py
// compiles it a second time, next to the comparison form it measures against (a block of rows transposed through LDS, which lives in the tool only).
// Needs EagleStabRow (include/eagle.h) and the HIP runtime, nothing else.

static constexpr int ST_VOTERS = 64;           // voters of a row: one lane each
static constexpr int ST_WAVES = 4;             // waves (rows in flight) of an estimate workgroup
static constexpr double ST_A0_CAP = 1099511627776.0;      // 2^40

struct StabArgs {
    const double2* values;       // the table before the stage, [column][row]
    const int32_t* frames;       // [rows]
    const uint8_t* kind;         // [cols]: 0 untouched, 1 moved only (the ball), 3 voter and moved
    int rows, cols, W, degree, model, min_voters, last;
    double trim_k, floor_q, lim_s, max_gain, jump_q;
    int2* q;                     // [column][row] scratch: the original integers
    int2* C;                     //                        the corrected integers of the round before
    uint8_t* present;            //                        1: a present cell of a moved column
    uint8_t* voteb;              //                        1: the cell votes in this round
    int2* votes;                 // [column][row], zeroed in front of the launches
    EagleStabRow* rec;           // [rows]
    double2* out;                // the table: the moved cells of rows with an estimate are overwritten in the last round
    EagleStabTotals* totals;     // zeroed in front of the launches
};

__device__ __forceinline__ long long st_wave_sum(long long v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ long long st_floor_div(long long a, long long b)     // b > 0
{
    long long q = a / b;
    if (a % b < 0) --q;
    return q;
}

struct StSlots { int dx[ST_VOTERS], dy[ST_VOTERS], col[ST_VOTERS]; };

// the lower median of the n values the lanes hold (lane < n): the value v with #{< v} <= rank < #{<= v}
__device__ __forceinline__ int st_wave_median(int v, int n, int lane)
{
    const int rank = (n - 1) / 2;
    int less = 0, leq = 0;
    for (int j = 0; j < n; ++j) { const int w = __shfl(v, j, 64); less += w < v; leq += w <= v; }
    const unsigned long long hit = __ballot(lane < n && less <= rank && rank < leq);
    return __shfl(v, __ffsll((long long)hit) - 1, 64);
}

__device__ __forceinline__ void st_affine(double n, double Su, double Sv, double Suu, double Suv, double Svv, double D0, double Du, double Dv, double* g)
{
    const double C00 = Suu * Svv - Suv * Suv;
    const double C01 = Suv * Sv - Su * Svv;
    const double C02 = Su * Suv - Suu * Sv;
    const double C11 = n * Svv - Sv * Sv;
    const double C12 = Su * Sv - n * Suv;
    const double C22 = n * Suu - Su * Su;
    const double det = (n * C00 + Su * C01) + Sv * C02;
    g[0] = ((C00 * D0 + C01 * Du) + C02 * Dv) / det;
    g[1] = ((C01 * D0 + C11 * Du) + C12 * Dv) / det;
    g[2] = ((C02 * D0 + C12 * Du) + C22 * Dv) / det;
}

// The map of a row record at q -> T(q)
__device__ __forceinline__ int2 st_map(int model, int sx, int sy, int cx, int cy, double ox, double oy, const double* gain, int2 q)
{
    if (model != 2) return make_int2(sx, sy);
    const double u = (double)(q.x - cx), v = (double)(q.y - cy);
    return make_int2((int)llrint((ox + gain[0] * u) + gain[1] * v), (int)llrint((oy + gain[2] * u) + gain[3] * v));
}

// One wave, one row: the first min(found, 64) voters lie in the wave's slots (and are visible); `moved` present cells of moved columns
__device__ __forceinline__ void st_row_estimate(const StabArgs& a, int r, int found, int moved, const StSlots& w, int lane)
{
    const int n = min(found, ST_VOTERS);
    EagleStabRow rec{};
    rec.voters = n;
    rec.flags = found > ST_VOTERS ? 1 : 0;
    if (n < a.min_voters) {                                     // uniform over the wave
        if (lane == 0) a.rec[r] = rec;
        return;
    }
    const bool act = lane < n;
    const int dx = act ? w.dx[lane] : 0, dy = act ? w.dy[lane] : 0;
    int2 q = make_int2(0, 0);
    if (act) q = a.q[(size_t)w.col[lane] * a.rows + r];
    const int bx = st_wave_median(dx, n, lane), by = st_wave_median(dy, n, lane);
    const int dev = max(abs(dx - bx), abs(dy - by));
    const int m = st_wave_median(dev, n, lane);
    const bool in = act && (a.trim_k == 0.0 || (double)dev <= fmax(a.floor_q, a.trim_k * (double)m));
    const long long ni = st_wave_sum(in);
    const long long ldx = in ? dx : 0, ldy = in ? dy : 0;
    const long long sdx = st_wave_sum(ldx), sdy = st_wave_sum(ldy);
    const long long sqx = st_wave_sum(in ? q.x : 0), sqy = st_wave_sum(in ? q.y : 0);
    const long long ssb = st_wave_sum(ldx * ldx + ldy * ldy);
    const int sx = (int)st_floor_div(2 * sdx + ni, 2 * ni), sy = (int)st_floor_div(2 * sdy + ni, 2 * ni);
    const int cx = (int)st_floor_div(sqx, ni), cy = (int)st_floor_div(sqy, ni);
    int model = 1, flags = rec.flags;
    double ox = (double)sx, oy = (double)sy, gain[4] = {0.0, 0.0, 0.0, 0.0};
    if (a.model == 1) {
        const long long u = in ? q.x - cx : 0, v = in ? q.y - cy : 0;
        const long long Su = st_wave_sum(u), Sv = st_wave_sum(v), Suu = st_wave_sum(u * u), Suv = st_wave_sum(u * v), Svv = st_wave_sum(v * v);
        const long long Dux = st_wave_sum(u * ldx), Dvx = st_wave_sum(v * ldx), Duy = st_wave_sum(u * ldy), Dvy = st_wave_sum(v * ldy);
        const long long Cuu = ni * Suu - Su * Su, Cvv = ni * Svv - Sv * Sv, Cuv = ni * Suv - Su * Sv;
        const double lim = (double)(ni * ni) * a.lim_s;
        if (ni < 6) flags |= 2;
        else if (!((double)Cuu >= lim && (double)Cvv >= lim)) flags |= 4;
        else if (!((double)Cuv * (double)Cuv <= 0.75 * ((double)Cuu * (double)Cvv))) flags |= 8;
        else {
            double gx[3], gy[3];
            st_affine((double)ni, (double)Su, (double)Sv, (double)Suu, (double)Suv, (double)Svv, (double)sdx, (double)Dux, (double)Dvx, gx);
            st_affine((double)ni, (double)Su, (double)Sv, (double)Suu, (double)Suv, (double)Svv, (double)sdy, (double)Duy, (double)Dvy, gy);
            if (fabs(gx[1]) <= a.max_gain && fabs(gx[2]) <= a.max_gain && fabs(gy[1]) <= a.max_gain && fabs(gy[2]) <= a.max_gain && fabs(gx[0]) <= ST_A0_CAP &&
                fabs(gy[0]) <= ST_A0_CAP) {
                model = 2; ox = gx[0]; oy = gy[0];
                gain[0] = gx[1]; gain[1] = gx[2]; gain[2] = gy[1]; gain[3] = gy[2];
            } else flags |= 16;
        }
    }
    const int2 shift = st_map(model, sx, sy, cx, cy, ox, oy, gain, make_int2(cx, cy));
    if ((double)abs(shift.x) > a.jump_q || (double)abs(shift.y) > a.jump_q) flags |= 32;
    const int2 tq = st_map(model, sx, sy, cx, cy, ox, oy, gain, q);
    const long long ex = in ? ldx - tq.x : 0, ey = in ? ldy - tq.y : 0;
    const long long ssa = st_wave_sum(ex * ex + ey * ey);
    if (lane == 0) {
        rec.inliers = (int)ni; rec.model = model; rec.flags = flags;
        rec.shift_q[0] = shift.x; rec.shift_q[1] = shift.y; rec.centre_q[0] = cx; rec.centre_q[1] = cy;
        rec.offset[0] = ox; rec.offset[1] = oy;
        for (int i = 0; i < 4; ++i) rec.gain[i] = gain[i];
        rec.ss_before = ssb; rec.ss_after = ssa; rec.moved = moved;
        a.rec[r] = rec;
    }
}

// the bits of the cell (column c, row r): 1 present in a moved column, 2 votes; its vote -> d
__device__ __forceinline__ int st_cell(const StabArgs& a, int c, int r, int2& d)
{
    d = make_int2(0, 0);
    if (c >= a.cols || r >= a.rows) return 0;
    const int k = a.kind[c];
    const size_t at = (size_t)c * a.rows + r;
    if (!k || !a.present[at]) return 0;
    if (k != 3 || !a.voteb[at]) return 1;
    d = a.votes[at];
    return 3;
}

// one chunk of 64 columns of one row: the lane's cell has the bits `st` and the vote d
__device__ __forceinline__ void st_compact(int st, int2 d, int col, int lane, int& found, int& moved, StSlots& w)
{
    const unsigned long long vm = __ballot(st & 2), pm = __ballot(st & 1);
    if (st & 2) {
        const int pos = found + __popcll(vm & ((1ull << lane) - 1ull));
        if (pos < ST_VOTERS) { w.dx[pos] = d.x; w.dy[pos] = d.y; w.col[pos] = col; }
    }
    found += __popcll(vm);
    moved += __popcll(pm);
}

// One wave per row; a lane reads the cell of its column, so a wave's reads are strided by the row count (the plain gather)
__global__ __launch_bounds__(ST_WAVES * 64) void stab_estimate_kernel(StabArgs a)
{
    __shared__ StSlots slots[ST_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * ST_WAVES + wave;
    const bool live = r < a.rows;                               // uniform over the wave; every wave passes the barrier
    int found = 0, moved = 0;
    if (live)
        for (int c0 = 0; c0 < a.cols; c0 += 64) {
            int2 d;
            const int st = st_cell(a, c0 + lane, r, d);
            st_compact(st, d, c0 + lane, lane, found, moved, slots[wave]);
        }
    __syncthreads();
    if (live) st_row_estimate(a, r, found, moved, slots[wave], lane);
}
