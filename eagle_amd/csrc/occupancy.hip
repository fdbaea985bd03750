// K24 — occupancy heat maps: a processed table resident in HBM (post.hip) -> per SELECTION of its columns where those columns spent their time: integer
// frame counts per pitch cell, a Gaussian-smoothed float32 surface, its byte form and a still picture of the pitch (include/eagle.h,
// eagle_post_occupancy / eagle_occupancy_picture / eagle_op_occupancy; tests/occupancy_ref.py is the written definition of every bit: integer counts,
// fp32 without contraction, d_expf of dmath.h for the taps, correctly rounded division).
//
// Five launches per call on one stream, no host round trip for the data:
//   occupancy_hist_kernel     one thread per (row, member column).  In the [cols][rows][2] layout a wave reads one run of 64 consecutive 16-byte cells of
//                             ONE column (the velocity and possession candidate kernels' pattern) and the frame numbers next to it.  INTEGERS ONLY: the
//                             row's weight in frames goes to the cell's int32 by a global integer atomic, after a wave-level merge: consecutive rows of
//                             a column mostly hit the same cell (a player moves a fraction of a cell per frame), so a segmented scan over the lanes
//                             (__shfl_up, runs of equal cell) leaves one atomic per RUN, issued by the run's last lane.  What falls outside the pitch
//                             and the inside total are wave sums (__shfl_xor) and one atomic per wave each.  No float atomics anywhere: their sums
//                             depend on arrival order and the contract is bit-exact.
//   occupancy_blur_kernel     twice: <false, int32> along x from the counts, <true, float> along y from the first pass.  A workgroup owns an OB_AX x
//                             OB_CR tile of one selection's grid (64 cells along the filter's axis, 16 across) and stages it with a `rad`-wide halo on
//                             both sides of the axis through LDS, zeros beyond the grid (a skipped term and an added t * 0.0f = +0.0f give the same
//                             bits: every term is >= +0); the staging loop walks the staged region whatever its size, so a rad beyond the tile or the
//                             grid is the same code.  The taps are formed once per workgroup into LDS.  A thread sums 4 outputs, each in the
//                             contract's order (k = -rad .. rad, multiply and add rounded separately).  LDS rows run along memory's x in both passes,
//                             so a wave's reads are 64 consecutive words: no bank conflict.  The second pass also folds its outputs into the
//                             selection's maximum (wave max, one integer atomicMax per wave on the float's bits: v >= 0, so the order of the bits is
//                             the order of the values, and a maximum does not depend on arrival order).
//   occupancy_norm_kernel     the byte form from the grid and that maximum, 4 cells per thread, one packed store.
//   occupancy_picture_kernel  (its own entry) one thread per pixel: the byte of the pixel's cell scaled into the caller's colour, the markings on top from
//                             minimap.hip's bit mask (shared through runtime.h, not copied).
#include "runtime.h"
#include "dmath.h"

namespace eagle {

static constexpr int OH_THREADS = 256;
static constexpr int OB_THREADS = 256, OB_AX = 64, OB_CR = 16, OB_OUT = OB_AX * OB_CR / OB_THREADS;      // 4 outputs per thread
static constexpr int OC_RAD_MAX = 120;                                                                   // ceil(3 x 10 m x 4 cells per metre)
static constexpr int OB_STAGE = (OB_AX + 2 * OC_RAD_MAX) * OB_CR;                                        // floats: 19 KB
static constexpr int OC_PASS = 65535;                                                                    // gridDim.y limit
static constexpr double OC_SIGMA_MAX = 10.0;

struct OccMember { int32_t col, sel; };

struct OccArgs {
    const double2* values;       // [column][row]
    const int32_t* frames;       // [rows]
    const OccMember* members;    // the selections' members, selection by selection
    int rows, max_gap, m0, R, gw, gh;
    int32_t* counts;             // [n_sel][gh][gw]
    uint32_t* total;             // [n_sel] each
    uint32_t* outside;
    uint32_t* maxbits;
    // smoothing
    float* hz; float* grids; uint8_t* bytes;
    int rad, sel0;
    float inv;
};

__global__ __launch_bounds__(OH_THREADS) void occupancy_hist_kernel(OccArgs a)
{
    const int r = blockIdx.x * OH_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const OccMember m = a.members[a.m0 + blockIdx.y];                    // (uniform)
    int key = -2, w = 0;                                                // key: the cell, -1 outside the pitch, -2 nothing (absent, or no such row)
    if (r < a.rows) {
        const double2 p = a.values[(size_t)m.col * a.rows + r];
        if (fabs(p.x) <= 1.7976931348623157e308 && fabs(p.y) <= 1.7976931348623157e308) {
            w = 1;
            if (r + 1 < a.rows) {
                const long long d = (long long)a.frames[r + 1] - (long long)a.frames[r];
                if (d <= (long long)a.max_gap) w = (int)d;
            }
            key = -1;
            if (p.x >= 0.0 && p.x < 105.0 && p.y >= 0.0 && p.y < 68.0) {
                const double fR = (double)a.R;
                key = (int)floor(p.y * fR) * a.gw + (int)floor(p.x * fR);
            }
        }
    }
    // (no early return: every lane takes part in the shuffles)
    int in_sum = key >= 0 ? w : 0, out_sum = key == -1 ? w : 0;
    #pragma unroll
    for (int d = 32; d; d >>= 1) { in_sum += __shfl_xor(in_sum, d, 64); out_sum += __shfl_xor(out_sum, d, 64); }
    // runs of equal cell along the wave's rows: a segmented inclusive add-scan; `head` = a run's first lane lies within what v already covers
    const int prev = __shfl_up(key, 1, 64), next = __shfl_down(key, 1, 64);
    int head = lane == 0 || prev != key;
    int v = w;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int ov = __shfl_up(v, d, 64), oh = __shfl_up(head, d, 64);
        if (lane >= d && !head) { v += ov; head = oh; }
    }
    int32_t* C = a.counts + (size_t)m.sel * a.gw * a.gh;
    if (key >= 0 && (lane == 63 || next != key)) atomicAdd(C + key, v);  // (key < gw gh: 0 <= x < 105 and 0 <= y < 68 were checked in double)
    if (lane == 0) {
        if (in_sum) atomicAdd(a.total + m.sel, (uint32_t)in_sum);
        if (out_sum) atomicAdd(a.outside + m.sel, (uint32_t)out_sum);
    }
}

// One separable pass.  VERT: the axis is y.  Memory's x stays the LDS row in both passes.
template <bool VERT, typename Tin>
__global__ __launch_bounds__(OB_THREADS) void occupancy_blur_kernel(OccArgs a, const Tin* in, float* out)
{
    __shared__ float s_in[OB_STAGE];
    __shared__ float s_t[OC_RAD_MAX + 1];
    constexpr int TX = VERT ? OB_CR : OB_AX, TY = VERT ? OB_AX : OB_CR;          // the tile in memory's terms
    const int tid = threadIdx.x, rad = a.rad, gw = a.gw, gh = a.gh;
    const int tiles_x = (gw + TX - 1) / TX;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int x0 = tx * TX, y0 = ty * TY;
    const int SX = VERT ? TX : TX + 2 * rad, SY = VERT ? TY + 2 * rad : TY;      // the staged region; SX * SY <= OB_STAGE since rad <= OC_RAD_MAX (host)
    const int sx0 = VERT ? x0 : x0 - rad, sy0 = VERT ? y0 - rad : y0;
    const size_t plane = (size_t)(a.sel0 + blockIdx.y) * gw * gh;
    const Tin* I = in + plane;
    static_assert(OC_RAD_MAX < OB_THREADS, "one tap per thread");
    if (tid <= rad) s_t[tid] = tid == 0 ? 1.0f : d_expf(-((float)(tid * tid)) * a.inv);      // (no loop: a loop here is vectorised into packed fp32 arithmetic)
    for (int e = tid; e < SX * SY; e += OB_THREADS) {
        const int sy = e / SX, sx = e - sy * SX, gx = sx0 + sx, gy = sy0 + sy;
        s_in[e] = (gx >= 0 && gx < gw && gy >= 0 && gy < gh) ? (float)I[(size_t)gy * gw + gx] : 0.0f;
    }
    __syncthreads();
    // a thread's outputs: one x, OB_OUT values of y (VERT: 16 x 64 tile, y = ly + 16 q; else 64 x 16 tile, y = ly + 4 q)
    const int lx = tid % TX, ly = tid / TX;
    constexpr int YS = OB_THREADS / TX;
    float acc[OB_OUT];
    #pragma unroll
    for (int q = 0; q < OB_OUT; ++q) acc[q] = 0.0f;
    const int step = VERT ? SX : 1;                                              // one cell along the axis, in LDS words
    const float* base = s_in + (VERT ? (ly + rad) * SX + lx : ly * SX + lx + rad);
    for (int k = -rad; k <= rad; ++k) {
        const float t = s_t[k < 0 ? -k : k];                                     // (one address for the whole wave: an LDS broadcast)
        #pragma unroll
        for (int q = 0; q < OB_OUT; ++q) acc[q] = acc[q] + t * base[q * YS * SX + k * step];
    }
    float best = 0.0f;
    #pragma unroll
    for (int q = 0; q < OB_OUT; ++q) {
        const int gx = x0 + lx, gy = y0 + ly + q * YS;
        if (gx < gw && gy < gh) { out[plane + (size_t)gy * gw + gx] = acc[q]; best = fmaxf(best, acc[q]); }
    }
    if (VERT) {
        #pragma unroll
        for (int d = 32; d; d >>= 1) best = fmaxf(best, __shfl_xor(best, d, 64));
        if ((tid & 63) == 0 && best > 0.0f) atomicMax(a.maxbits + a.sel0 + blockIdx.y, __float_as_uint(best));
    }
}

__global__ __launch_bounds__(256) void occupancy_norm_kernel(OccArgs a)
{
    const int cells = a.gw * a.gh;                                               // (a multiple of 4: 7140 R^2)
    const int k0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (k0 >= cells) return;
    const size_t plane = (size_t)(a.sel0 + blockIdx.y) * cells;
    const float m = __uint_as_float(a.maxbits[a.sel0 + blockIdx.y]);
    const float4 v = *(const float4*)(a.grids + plane + k0);                     // (plane and k0 are multiples of 4 floats; the buffer is 256-byte aligned)
    const float f[4] = {v.x, v.y, v.z, v.w};
    uint32_t word = 0;
    #pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t b = m > 0.0f ? (uint32_t)(int)floorf(f[c] / m * 255.0f + 0.5f) : 0u;
        word |= b << (8 * c);
    }
    *(uint32_t*)(a.bytes + plane + k0) = word;
}

struct OccPicArgs {
    const uint8_t* grid;         // [gh][gw] bytes of one selection
    const uint8_t* mask;         // markings: bit (x & 7) of byte y * mask_pitch + (x >> 3)
    uint8_t* out;                // [h][w][3]
    int w, h, S, M, R, gw, gh, mask_pitch;
    uint32_t colour;             // B | G << 8 | R << 16
};

__global__ __launch_bounds__(256) void occupancy_picture_kernel(OccPicArgs p)
{
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y;
    if (X >= p.w) return;
    uint32_t px = 0;
    if (p.mask[(size_t)Y * p.mask_pitch + (X >> 3)] >> (X & 7) & 1) px = 0xffffffu;
    else if (X >= p.M && X < p.M + 105 * p.S && Y >= p.M && Y < p.M + 68 * p.S) {
        const uint32_t c = p.grid[(size_t)(p.gh - 1 - (Y - p.M) * p.R / p.S) * p.gw + (X - p.M) * p.R / p.S], al = c + (c >> 7);
        #pragma unroll
        for (int s = 0; s < 24; s += 8) px |= ((((p.colour >> s) & 255u) * al + 128u) >> 8) << s;
    }
    uint8_t* d = p.out + ((size_t)Y * p.w + X) * 3;
    d[0] = (uint8_t)px; d[1] = (uint8_t)(px >> 8); d[2] = (uint8_t)(px >> 16);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void occupancy_check(const char* who, const EagleOccupancyParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: params is NULL", who);
    if (p->fps <= 0 || p->max_gap <= 0) fail(EAGLE_E_INVALID, "%s: fps %d and max_gap %d must be positive", who, p->fps, p->max_gap);
    if (p->cells_per_metre != 1 && p->cells_per_metre != 2 && p->cells_per_metre != 4)
        fail(EAGLE_E_INVALID, "%s: cells_per_metre %d must be 1, 2 or 4", who, p->cells_per_metre);
    if (!(p->sigma >= 0.0 && p->sigma <= OC_SIGMA_MAX)) fail(EAGLE_E_INVALID, "%s: sigma %g must lie within 0 .. 10 m", who, p->sigma);
}

// The selections against the table's columns -> their members, selection by selection.  Everything a launch relies on is settled here.
static std::vector<OccMember> occupancy_members(const char* who, const EaglePostColumn* columns, int ncols, int rows, const EagleOccupancyParams* p, const int32_t* sel_off,
                                                const int32_t* sel_cols, int n_sel)
{
    std::vector<OccMember> mem;
    if (n_sel < 0) fail(EAGLE_E_INVALID, "%s: n_sel = %d is negative", who, n_sel);
    if (n_sel == 0) return mem;
    if (!sel_off) fail(EAGLE_E_INVALID, "%s: sel_off is NULL", who);
    if (sel_off[0] != 0) fail(EAGLE_E_INVALID, "%s: sel_off[0] = %d must be 0", who, sel_off[0]);
    for (int s = 0; s < n_sel; ++s)
        if (sel_off[s + 1] < sel_off[s]) fail(EAGLE_E_INVALID, "%s: sel_off must ascend (selection %d: %d after %d)", who, s, sel_off[s + 1], sel_off[s]);
    if (sel_off[n_sel] > 0 && !sel_cols) fail(EAGLE_E_INVALID, "%s: sel_cols is NULL", who);
    std::vector<int> seen(std::max(ncols, 1), -1);
    int largest = 0;
    for (int s = 0; s < n_sel; ++s) {
        largest = std::max(largest, sel_off[s + 1] - sel_off[s]);
        for (int k = sel_off[s]; k < sel_off[s + 1]; ++k) {
            const int c = sel_cols[k];
            if (c < 0 || c >= ncols) fail(EAGLE_E_INVALID, "%s: selection %d names column %d of %d", who, s, c, ncols);
            const EaglePostColumn& col = columns[c];
            if (col.video) fail(EAGLE_E_INVALID, "%s: selection %d names column %d, a video column (pitch columns only)", who, s, c);
            if (col.kind != EAGLE_POST_PLAYER && col.kind != EAGLE_POST_GOALKEEPER && col.kind != EAGLE_POST_BALL)
                fail(EAGLE_E_INVALID, "%s: selection %d names column %d of kind %d (players, goalkeepers and the ball only)", who, s, c, col.kind);
            if (seen[c] == s) fail(EAGLE_E_INVALID, "%s: selection %d lists column %d twice", who, s, c);
            seen[c] = s;
            mem.push_back(OccMember{c, s});
        }
    }
    // 32-bit accumulators: a cell, a total or an outside count is at most rows x max_gap x (members of the selection)
    if ((double)rows * (double)p->max_gap * (double)largest >= 2147483648.0)
        fail(EAGLE_E_INVALID, "%s: %d rows x max_gap %d x %d members of the largest selection reaches 2^31 (32-bit counts)", who, rows, p->max_gap, largest);
    return mem;
}

struct OccLayout { size_t grids, counts, bytes, total, outside, maxbits, end; };

static OccLayout occupancy_layout(int n_sel, int R)
{
    const size_t cells = (size_t)7140 * R * R, n = (size_t)n_sel;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    OccLayout L{};
    L.grids = 0; L.counts = up(n * cells * 4); L.bytes = L.counts + up(n * cells * 4);
    L.total = L.bytes + up(n * cells); L.outside = L.total + up(n * 4); L.maxbits = L.outside + up(n * 4); L.end = L.maxbits + up(n * 4);
    return L;
}

// bytes a call needs on the device: the result and the first pass's plane
static double occupancy_need(int n_sel, int R) { return (double)occupancy_layout(n_sel, R).end + (double)n_sel * 7140.0 * R * R * 4.0; }

static void occupancy_budget(const char* who, int n_sel, int R, int64_t max_bytes)
{
    double budget = (double)max_bytes;
    if (max_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = 0.9 * (double)free_b;
    }
    const double need = occupancy_need(n_sel, R);
    if (need > budget) fail(EAGLE_E_INVALID, "%s: %d maps at %d cells per metre need %.0f bytes of device memory, the budget is %.0f", who, n_sel, R, need, budget);
}

static float occupancy_taps(const EagleOccupancyParams* p, int* rad)
{
    if (p->sigma == 0.0) { *rad = 0; return 0.0f; }
    const float s = (float)p->sigma * (float)p->cells_per_metre;
    *rad = (int)ceilf(3.0f * s);
    return 1.0f / (2.0f * s * s);
}

// The launches of one call on s; `res` is the result block (occupancy_layout), zeroed here; d_hz the first pass's plane.
static void occupancy_run(EagleHandle* h, const std::vector<OccMember>& mem, const OccMember* d_mem, const double2* d_values, const int32_t* d_frames, int rows,
                          const EagleOccupancyParams* p, int n_sel, uint8_t* res, float* d_hz, hipStream_t s)
{
    const int R = p->cells_per_metre;
    const OccLayout L = occupancy_layout(n_sel, R);
    OccArgs a{};
    a.values = d_values; a.frames = d_frames; a.members = d_mem; a.rows = rows; a.max_gap = p->max_gap;
    a.R = R; a.gw = 105 * R; a.gh = 68 * R;
    a.grids = (float*)(res + L.grids); a.counts = (int32_t*)(res + L.counts); a.bytes = res + L.bytes;
    a.total = (uint32_t*)(res + L.total); a.outside = (uint32_t*)(res + L.outside); a.maxbits = (uint32_t*)(res + L.maxbits);
    a.hz = d_hz;
    a.inv = occupancy_taps(p, &a.rad);
    if (a.rad < 0 || a.rad > OC_RAD_MAX) fail(EAGLE_E_STATE, "occupancy: radius %d outside 0 .. %d", a.rad, OC_RAD_MAX);
    const int cells = a.gw * a.gh, nmem = (int)mem.size();
    HIP_CHECK(hipMemsetAsync(res + L.counts, 0, L.end - L.counts, s));            // counts, bytes, total, outside, maxbits
    auto hist = [&] {
        OccArgs b = a;
        for (int m0 = 0; m0 < nmem && rows > 0; m0 += OC_PASS) {
            b.m0 = m0;
            hipLaunchKernelGGL(occupancy_hist_kernel, dim3((rows + OH_THREADS - 1) / OH_THREADS, std::min(nmem - m0, OC_PASS)), dim3(OH_THREADS), 0, s, b);
            HIP_CHECK(hipGetLastError());
        }
    };
    auto blur = [&](bool vert) {
        OccArgs b = a;
        const int tiles = vert ? ((a.gw + OB_CR - 1) / OB_CR) * ((a.gh + OB_AX - 1) / OB_AX) : ((a.gw + OB_AX - 1) / OB_AX) * ((a.gh + OB_CR - 1) / OB_CR);
        for (int s0 = 0; s0 < n_sel; s0 += OC_PASS) {
            b.sel0 = s0;
            const dim3 g(tiles, std::min(n_sel - s0, OC_PASS));
            if (vert) hipLaunchKernelGGL((occupancy_blur_kernel<true, float>), g, dim3(OB_THREADS), 0, s, b, (const float*)a.hz, a.grids);
            else hipLaunchKernelGGL((occupancy_blur_kernel<false, int32_t>), g, dim3(OB_THREADS), 0, s, b, (const int32_t*)a.counts, a.hz);
            HIP_CHECK(hipGetLastError());
        }
    };
    auto norm = [&] {
        OccArgs b = a;
        for (int s0 = 0; s0 < n_sel; s0 += OC_PASS) {
            b.sel0 = s0;
            hipLaunchKernelGGL(occupancy_norm_kernel, dim3((cells / 4 + 255) / 256, std::min(n_sel - s0, OC_PASS)), dim3(256), 0, s, b);
            HIP_CHECK(hipGetLastError());
        }
    };
    // bytes: a member's cells and frame numbers read; per pass a plane read and a plane written; the grid read and the bytes written
    const double plane = (double)n_sel * cells;
    if (h) {
        timed_launch(h, "occupancy_hist", (double)nmem * rows * 20.0, s, hist);
        timed_launch(h, "occupancy_blur_x", plane * 8.0, s, [&] { blur(false); });
        timed_launch(h, "occupancy_blur_y", plane * 8.0, s, [&] { blur(true); });
        timed_launch(h, "occupancy_norm", plane * 5.0, s, norm);
    } else { hist(); blur(false); blur(true); norm(); }
}

static void occupancy_fetch(const uint8_t* res, int n_sel, int R, float* grids, uint8_t* bytes, int64_t* total, int64_t* outside, int32_t* counts)
{
    const OccLayout L = occupancy_layout(n_sel, R);
    const size_t n = (size_t)n_sel * 7140 * R * R;
    if (grids) HIP_CHECK(hipMemcpy(grids, res + L.grids, n * 4, hipMemcpyDeviceToHost));
    if (counts) HIP_CHECK(hipMemcpy(counts, res + L.counts, n * 4, hipMemcpyDeviceToHost));
    if (bytes) HIP_CHECK(hipMemcpy(bytes, res + L.bytes, n, hipMemcpyDeviceToHost));
    if (total || outside) {
        std::vector<uint32_t> acc(2 * (size_t)n_sel);
        HIP_CHECK(hipMemcpy(acc.data(), res + L.total, (size_t)n_sel * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(acc.data() + n_sel, res + L.outside, (size_t)n_sel * 4, hipMemcpyDeviceToHost));
        for (int s = 0; s < n_sel; ++s) {
            if (total) total[s] = (int64_t)acc[s];
            if (outside) outside[s] = (int64_t)acc[n_sel + s];
        }
    }
}

static OccPicArgs occupancy_picture_args(const MmPlan& pl, int R, uint32_t colour)
{
    OccPicArgs a{};
    a.w = pl.w; a.h = pl.h; a.S = pl.S; a.M = pl.M; a.R = R; a.gw = 105 * R; a.gh = 68 * R; a.mask_pitch = (pl.w + 7) / 8;
    a.colour = colour & 0xffffffu;
    return a;
}

static MmPlan occupancy_picture_plan(int scale, int margin)
{
    EagleMinimapParams mp{};
    mp.scale = scale; mp.margin = margin;
    return minimap_plan(&mp);                                                    // the minimap's rules for scale and margin
}

static void occupancy_picture_launch(const OccPicArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(occupancy_picture_kernel, dim3((a.w + 255) / 256, a.h), dim3(256), 0, s, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace eagle

extern "C" {

int eagle_occupancy_size(const EagleOccupancyParams* p, int* gw, int* gh)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!gw || !gh) fail(EAGLE_E_INVALID, "eagle_occupancy_size: gw or gh is NULL");
    occupancy_check("eagle_occupancy_size", p);
    *gw = 105 * p->cells_per_metre; *gh = 68 * p->cells_per_metre;
    API_END(hh)
}

int eagle_post_occupancy(EagleHandle* h, EaglePostTable* t, const EagleOccupancyParams* p, const int32_t* sel_off, const int32_t* sel_cols, int n_sel)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_occupancy: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_occupancy: the table belongs to another handle");
    occupancy_check("eagle_post_occupancy", p);
    const std::vector<OccMember> mem = occupancy_members("eagle_post_occupancy", t->columns.data(), t->cols, t->rows, p, sel_off, sel_cols, n_sel);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const int R = p->cells_per_metre;
    if (n_sel) occupancy_budget("eagle_post_occupancy", n_sel, R, t->max_bytes);
    if (t->d_occ) { HIP_CHECK(hipFree(t->d_occ)); t->d_occ = nullptr; }          // a call replaces the result of the one before
    t->has_occ = true; t->occ_nsel = n_sel; t->occ_R = R;
    if (n_sel == 0) return EAGLE_OK;
    const hipStream_t s = h->s_main;
    const size_t rows = (size_t)t->rows, cells = (size_t)7140 * R * R;
    void *d_frames = nullptr, *d_mem = nullptr, *d_hz = nullptr;
    try {
        HIP_CHECK(hipMalloc(&t->d_occ, occupancy_layout(n_sel, R).end));
        HIP_CHECK(hipMalloc(&d_hz, (size_t)n_sel * cells * 4));
        HIP_CHECK(hipMalloc(&d_frames, std::max<size_t>(rows * 4, 16)));
        HIP_CHECK(hipMalloc(&d_mem, std::max<size_t>(mem.size() * sizeof(OccMember), 16)));
        if (rows) HIP_CHECK(hipMemcpyAsync(d_frames, t->frames.data(), rows * 4, hipMemcpyHostToDevice, s));
        if (!mem.empty()) HIP_CHECK(hipMemcpyAsync(d_mem, mem.data(), mem.size() * sizeof(OccMember), hipMemcpyHostToDevice, s));
        occupancy_run(h, mem, (const OccMember*)d_mem, (const double2*)t->d_values, (const int32_t*)d_frames, t->rows, p, n_sel, (uint8_t*)t->d_occ, (float*)d_hz, s);
        HIP_CHECK(hipStreamSynchronize(s));
        if (h->prof) collect_spans(h);
    } catch (...) {
        (void)hipStreamSynchronize(s);
        for (void* q : {d_frames, d_mem, d_hz}) if (q) (void)hipFree(q);
        if (t->d_occ) { (void)hipFree(t->d_occ); t->d_occ = nullptr; }
        t->has_occ = false; t->occ_nsel = 0;
        throw;
    }
    for (void* q : {d_frames, d_mem, d_hz}) HIP_CHECK(hipFree(q));
    API_END(h)
}

int eagle_post_occupancy_values(EaglePostTable* t, float* grids, uint8_t* bytes, int64_t* total, int64_t* outside, int32_t* counts)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->has_occ) fail(EAGLE_E_INVALID, "eagle_post_occupancy_values: the table has no occupancy (eagle_post_occupancy)");
    if (t->occ_nsel) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        occupancy_fetch((const uint8_t*)t->d_occ, t->occ_nsel, t->occ_R, grids, bytes, total, outside, counts);
    }
    API_END(h)
}

int eagle_post_device_occupancy(const EaglePostTable* t, const float** d_grids, const uint8_t** d_bytes)
{
    if (!t || !d_grids || !d_bytes) return EAGLE_E_INVALID;
    *d_grids = nullptr; *d_bytes = nullptr;
    if (t->has_occ && t->d_occ) {
        *d_grids = (const float*)t->d_occ;
        *d_bytes = (const uint8_t*)t->d_occ + occupancy_layout(t->occ_nsel, t->occ_R).bytes;
    }
    return EAGLE_OK;
}

int eagle_occupancy_picture(EagleHandle* h, EaglePostTable* t, int sel, int scale, int margin, uint32_t bgr_colour, uint8_t* out)
{
    API_BEGIN_H(h)
    if (!t || !out) fail(EAGLE_E_INVALID, "eagle_occupancy_picture: bad argument (table %p, out %p)", (const void*)t, (const void*)out);
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_occupancy_picture: the table belongs to another handle");
    const MmPlan pl = occupancy_picture_plan(scale, margin);
    if (!t->has_occ) fail(EAGLE_E_INVALID, "eagle_occupancy_picture: the table has no occupancy (eagle_post_occupancy comes first)");
    if (sel < 0 || sel >= t->occ_nsel) fail(EAGLE_E_INVALID, "eagle_occupancy_picture: selection %d lies outside the last result's %d", sel, t->occ_nsel);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    OccPicArgs a = occupancy_picture_args(pl, t->occ_R, bgr_colour);
    a.grid = (const uint8_t*)t->d_occ + occupancy_layout(t->occ_nsel, t->occ_R).bytes + (size_t)sel * a.gw * a.gh;
    a.mask = minimap_mask(h, pl);
    const size_t nb = (size_t)pl.w * pl.h * 3;
    void* d_out = nullptr;
    HIP_CHECK(hipMalloc(&d_out, nb));
    a.out = (uint8_t*)d_out;
    try {
        timed_launch(h, "occupancy_picture", (double)nb, h->s_main, [&] { occupancy_picture_launch(a, h->s_main); });
        HIP_CHECK(hipMemcpyAsync(out, d_out, nb, hipMemcpyDeviceToHost, h->s_main));
        HIP_CHECK(hipStreamSynchronize(h->s_main));
        if (h->prof) collect_spans(h);
    } catch (...) {
        (void)hipStreamSynchronize(h->s_main);
        (void)hipFree(d_out);
        throw;
    }
    HIP_CHECK(hipFree(d_out));
    API_END(h)
}

int eagle_op_occupancy(int device, const double* values, const int32_t* frames, const EaglePostColumn* columns, int rows, int cols, const EagleOccupancyParams* p,
                       const int32_t* sel_off, const int32_t* sel_cols, int n_sel, float* grids, uint8_t* bytes, int64_t* total, int64_t* outside, int32_t* counts)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !frames || !columns || rows < 0 || cols < 0)
        fail(EAGLE_E_INVALID, "eagle_op_occupancy: bad argument (values %p, frames %p, columns %p, %d rows, %d columns)", (const void*)values, (const void*)frames,
             (const void*)columns, rows, cols);
    occupancy_check("eagle_op_occupancy", p);
    const std::vector<OccMember> mem = occupancy_members("eagle_op_occupancy", columns, cols, rows, p, sel_off, sel_cols, n_sel);
    for (int r = 1; r < rows; ++r)
        if (frames[r] <= frames[r - 1]) fail(EAGLE_E_INVALID, "eagle_op_occupancy: frame numbers must ascend (row %d: %d after %d)", r, frames[r], frames[r - 1]);
    if (n_sel == 0) return EAGLE_OK;
    const int R = p->cells_per_metre;
    HIP_CHECK(hipSetDevice(device));
    occupancy_budget("eagle_op_occupancy", n_sel, R, 0);
    Net net;
    const size_t n = (size_t)rows;
    const double2* d_v = rows && cols ? (const double2*)net.upload(values, (size_t)cols * n * sizeof(double2)) : nullptr;
    const int32_t* d_f = rows ? (const int32_t*)net.upload(frames, n * 4) : nullptr;
    const OccMember* d_m = mem.empty() ? nullptr : (const OccMember*)net.upload(mem.data(), mem.size() * sizeof(OccMember));
    uint8_t* res = (uint8_t*)net.get(occupancy_layout(n_sel, R).end);
    float* d_hz = (float*)net.get((size_t)n_sel * 7140 * R * R * 4);
    occupancy_run(nullptr, mem, d_m, d_v, d_f, rows, p, n_sel, res, d_hz, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    occupancy_fetch(res, n_sel, R, grids, bytes, total, outside, counts);
    API_END(hh)
}

int eagle_op_occupancy_picture(int device, const uint8_t* bytes_grid, int cells_per_metre, int scale, int margin, uint32_t bgr_colour, uint8_t* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!bytes_grid || !out) fail(EAGLE_E_INVALID, "eagle_op_occupancy_picture: bad argument (bytes %p, out %p)", (const void*)bytes_grid, (const void*)out);
    if (cells_per_metre != 1 && cells_per_metre != 2 && cells_per_metre != 4)
        fail(EAGLE_E_INVALID, "eagle_op_occupancy_picture: cells_per_metre %d must be 1, 2 or 4", cells_per_metre);
    const MmPlan pl = occupancy_picture_plan(scale, margin);
    HIP_CHECK(hipSetDevice(device));
    Net net;
    int mp = 0;
    const std::vector<uint8_t> bits = markings_mask(pl, &mp);
    OccPicArgs a = occupancy_picture_args(pl, cells_per_metre, bgr_colour);
    a.grid = (const uint8_t*)net.upload(bytes_grid, (size_t)a.gw * a.gh);
    a.mask = (const uint8_t*)net.upload(bits.data(), bits.size());
    const size_t nb = (size_t)pl.w * pl.h * 3;
    a.out = (uint8_t*)net.get(nb);
    occupancy_picture_launch(a, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, a.out, nb, hipMemcpyDeviceToHost));
    API_END(hh)
}

}  // extern "C"
