// K22 — pitch control: rows of a processed table resident in HBM (post.hip) and their velocities -> per row a grid of the share of each pitch cell team 0
// reaches first (include/eagle.h, eagle_control_*; tests/control_ref.py is the written definition of every byte: fp32, no contraction, correctly
// rounded sqrt and division, d_expf of dmath.h).
//
// Two launches per call, no host round trip for the data:
//   control_sites_kernel  one thread per table row walks the site columns (the host decides per COLUMN what is a site and of which team, as
//                         minimap_columns does) and writes the row's compacted list: the reaction point q = p + v t_react in fp32 and the team bit,
//                         16 bytes per entry behind a header with the count.  Loads are contiguous along rows, stores are not (minimap_sites_kernel's
//                         trade, for the same reason).
//   control_kernel        a workgroup owns CT_THREADS x CT_CELLS consecutive cells of one row's grid (the grid taken as one run of gw gh bytes, a
//                         multiple of 4 for every R), a thread CT_CELLS of them in registers; the row's sites go through LDS in chunks of CT_CHUNK
//                         (any count is exact) and every lane reads the same entry at once (an LDS broadcast), so one 16-byte read feeds
//                         CT_CELLS cells.  Pass 1 keeps the smallest squared distance per cell: sqrtf, the division by v_max and the addition of
//                         t_react are monotone, so t_min = t(min d^2), formed once.  Pass 2 RECOMPUTES t_i per site (the site
//                         count is a run-time value, so keeping t_i would mean scratch or LDS of CT_CELLS x count floats per thread) and sums the
//                         weights in table order.  The bytes leave as one packed 32-bit store per thread; their sum goes to the row's int64 by a wave
//                         reduction and one integer atomic per wave (order-free).
#include "runtime.h"
#include "dmath.h"

namespace eagle {

static constexpr int CT_THREADS = 256, CT_CELLS = 4, CT_CHUNK = 256;
static constexpr float CT_QLIM = 1048576.0f;
static constexpr double CT_DOMAIN = 1024.0;
static constexpr int64_t CT_STAGING = (int64_t)32 << 20;      // eagle_control_grids: device staging per pass

__global__ __launch_bounds__(256) void control_sites_kernel(ControlArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const size_t row = (size_t)(a.row0 + i);
    float4* L = a.lists + (size_t)i * a.stride;
    int cnt = 0;
    for (int c = 0; c < a.ncols; ++c) {
        const CtCol d = a.cols[c];
        const double2 p = a.values[(size_t)d.col * a.rows + row];
        if (!(fabs(p.x) <= CT_DOMAIN) || !(fabs(p.y) <= CT_DOMAIN)) continue;           // NaN, +-inf and the far field
        const double2 vd = a.vel[(size_t)d.col * a.rows + row];
        float vx = (float)vd.x, vy = (float)vd.y;
        if (!(fabsf(vx) <= 3.402823466e+38f)) vx = 0.0f;                                // NaN, or beyond fp32
        if (!(fabsf(vy) <= 3.402823466e+38f)) vy = 0.0f;
        float qx = (float)p.x + vx * a.t_react, qy = (float)p.y + vy * a.t_react;
        qx = fminf(fmaxf(qx, -CT_QLIM), CT_QLIM);
        qy = fminf(fmaxf(qy, -CT_QLIM), CT_QLIM);
        L[1 + cnt++] = make_float4(qx, qy, d.team0 ? 1.0f : 0.0f, 0.0f);
    }
    L[0] = make_float4(__int_as_float(cnt), 0.0f, 0.0f, 0.0f);
}

__global__ __launch_bounds__(CT_THREADS) void control_kernel(ControlArgs a)
{
    __shared__ float4 s_e[CT_CHUNK];
    const int f = blockIdx.y, tid = threadIdx.x;
    const int cells = a.gw * a.gh;                     // (a multiple of CT_CELLS: 7140 R^2)
    const int k0 = (blockIdx.x * CT_THREADS + tid) * CT_CELLS;
    const bool live = k0 < cells;                      // (no early return: the workgroup meets at the barriers of the staging loops)
    const float4* L = a.lists + (size_t)f * a.stride;
    const int count = __float_as_int(L[0].x);
    const float fR = (float)a.R;
    float cx[CT_CELLS], cy[CT_CELLS], best[CT_CELLS], num[CT_CELLS], den[CT_CELLS];
    #pragma unroll
    for (int c = 0; c < CT_CELLS; ++c) {
        const int k = live ? k0 + c : 0, j = k / a.gw, i = k - j * a.gw;
        cx[c] = ((float)i + 0.5f) / fR;                // (exact: R is 1, 2 or 4)
        cy[c] = ((float)j + 0.5f) / fR;
        best[c] = 3.402823466e+38f; num[c] = 0.0f; den[c] = 0.0f;
    }
    // ---- pass 1: the smallest squared distance to a reaction point ----
    for (int base = 0; base < count; base += CT_CHUNK) {
        const int nc = min(CT_CHUNK, count - base);
        __syncthreads();                               // the previous chunk has been consumed
        if (tid < nc) s_e[tid] = L[1 + base + tid];
        __syncthreads();
        if (!live) continue;
        for (int s = 0; s < nc; ++s) {
            const float4 e = s_e[s];                   // (one address for the whole wave: an LDS broadcast)
            #pragma unroll
            for (int c = 0; c < CT_CELLS; ++c) {
                const float dx = cx[c] - e.x, dy = cy[c] - e.y;
                best[c] = fminf(best[c], dx * dx + dy * dy);
            }
        }
    }
    float t_min[CT_CELLS];
    #pragma unroll
    for (int c = 0; c < CT_CELLS; ++c) t_min[c] = a.t_react + sqrtf(best[c]) / a.v_max;
    // ---- pass 2: the weights, summed in table order ----
    const float nbeta = -a.beta;
    for (int base = 0; base < count; base += CT_CHUNK) {
        const int nc = min(CT_CHUNK, count - base);
        if (count > CT_CHUNK) {                        // (uniform; a single chunk is still staged)
            __syncthreads();
            if (tid < nc) s_e[tid] = L[1 + base + tid];
            __syncthreads();
        }
        if (!live) continue;
        for (int s = 0; s < nc; ++s) {
            const float4 e = s_e[s];
            const bool team0 = e.z != 0.0f;            // (uniform)
            #pragma unroll
            for (int c = 0; c < CT_CELLS; ++c) {
                const float dx = cx[c] - e.x, dy = cy[c] - e.y;
                const float t = a.t_react + sqrtf(dx * dx + dy * dy) / a.v_max;
                const float w = d_expf(nbeta * (t - t_min[c]));
                den[c] = den[c] + w;
                if (team0) num[c] = num[c] + w;
            }
        }
    }
    uint32_t word = 0, sum = 0;
    #pragma unroll
    for (int c = 0; c < CT_CELLS; ++c) {
        const uint32_t b = count > 0 ? (uint32_t)(int)floorf(num[c] / den[c] * 255.0f + 0.5f) : 128u;
        word |= b << (8 * c);
        sum += b;
    }
    if (live) {
        uint8_t* d = a.out + (size_t)f * cells + k0;
        if (((uintptr_t)d & 3) == 0) *(uint32_t*)d = word;
        else {
            #pragma unroll
            for (int c = 0; c < CT_CELLS; ++c) d[c] = (uint8_t)(word >> (8 * c));
        }
    } else sum = 0;
    if (a.share) {
        for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if ((tid & 63) == 0 && sum) atomicAdd(a.share + f, (unsigned long long)sum);
    }
}

void control_launch(const ControlArgs& a, hipStream_t s)
{
    const int cells = a.gw * a.gh, per = CT_THREADS * CT_CELLS;
    if (a.share) HIP_CHECK(hipMemsetAsync(a.share, 0, (size_t)a.n * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(control_sites_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(control_kernel, dim3((cells + per - 1) / per, a.n), dim3(CT_THREADS), 0, s, a);
    HIP_CHECK(hipGetLastError());
}

void control_check(const EagleControlParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "control: params is NULL");
    if (p->cells_per_metre != 1 && p->cells_per_metre != 2 && p->cells_per_metre != 4)
        fail(EAGLE_E_INVALID, "control: cells_per_metre %d must be 1, 2 or 4", p->cells_per_metre);
    if (!(p->t_react >= 0.0f && p->t_react <= 1000.0f)) fail(EAGLE_E_INVALID, "control: t_react %g must lie within 0 .. 1000 s", (double)p->t_react);
    if (!(p->v_max >= 1e-3f && p->v_max <= 1e6f)) fail(EAGLE_E_INVALID, "control: v_max %g must be positive (0.001 .. 1e6 m/s)", (double)p->v_max);
    if (!(p->beta > 0.0f && p->beta <= 1e6f)) fail(EAGLE_E_INVALID, "control: beta %g must be positive (at most 1e6 / s)", (double)p->beta);
}

// which table columns are sites, in table order: minimap_columns' Voronoi sites
void control_columns(const EaglePostColumn* columns, int ncols, const int32_t* team_ids, const int32_t* team_vals, size_t n_team, std::vector<CtCol>& out)
{
    for (int c = 0; c < ncols; ++c) {
        const EaglePostColumn& col = columns[c];
        if (col.video || col.kind != EAGLE_POST_PLAYER) continue;
        size_t k = 0;
        while (k < n_team && team_ids[k] != col.id) ++k;
        if (k == n_team) continue;
        out.push_back(CtCol{c, team_vals[k] == 0 ? 1 : 0});
    }
}

static void control_window(int rows, int row0, int n)
{
    if (n < 0) fail(EAGLE_E_INVALID, "control: n = %d is negative", n);
    if (n > 0 && rows == 0) fail(EAGLE_E_INVALID, "control: the table has no rows");
    if (row0 < 0 || row0 > rows || n > rows - row0) fail(EAGLE_E_INVALID, "control: rows %d .. %d lie outside the table's %d rows", row0, row0 + n - 1, rows);
}

static ControlArgs control_args(const EagleControlParams* p)
{
    ControlArgs a{};
    a.R = p->cells_per_metre; a.gw = 105 * a.R; a.gh = 68 * a.R;
    a.t_react = p->t_react; a.v_max = p->v_max; a.beta = p->beta;
    return a;
}

static void grow(void** buf, size_t* cap, size_t need)
{
    if (need <= *cap) return;
    if (*buf) HIP_CHECK(hipFree(*buf));
    *buf = nullptr; *cap = 0;
    HIP_CHECK(hipMalloc(buf, need));
    *cap = need;
}

static void control_begin(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleControlParams* p, const void* out)
{
    if (!t || !out) fail(EAGLE_E_INVALID, "control: bad argument (table %p, out %p)", (const void*)t, out);
    if (t->h != h) fail(EAGLE_E_INVALID, "control: the table belongs to another handle");
    control_check(p);
    if (!t->has_team) fail(EAGLE_E_INVALID, "control: the table has no team mapping (team 0 is counted against the others)");
    if (!t->d_vel) fail(EAGLE_E_INVALID, "control: the table has no velocities (eagle_post_velocities comes first)");
    control_window(t->rows, row0, n);
    HIP_CHECK(hipSetDevice(h->cfg.device));
}

}  // namespace eagle

namespace eagle {
// Once per call of a handle entry: the site columns (uploaded) and list space for passes of up to max_pass rows (also minimap.hip's control layer)
ControlArgs control_prepare(EagleHandle* h, EaglePostTable* t, const EagleControlParams* p, int max_pass)
{
    std::vector<CtCol> cols;
    ControlArgs a = control_args(p);
    control_columns(t->columns.data(), t->cols, t->team_ids.data(), t->team_vals.data(), t->team_ids.size(), cols);
    a.values = (const double2*)t->d_values; a.vel = (const double2*)t->d_vel; a.rows = t->rows;
    a.ncols = (int)cols.size(); a.stride = 1 + a.ncols;
    grow(&h->ct_list, &h->ct_list_cap, (size_t)std::min(max_pass, CT_PASS) * a.stride * sizeof(float4));
    grow(&h->ct_cols, &h->ct_cols_cap, std::max<size_t>(cols.size() * sizeof(CtCol), 16));
    if (!cols.empty()) HIP_CHECK(hipMemcpyAsync(h->ct_cols, cols.data(), cols.size() * sizeof(CtCol), hipMemcpyHostToDevice, h->s_main));
    HIP_CHECK(hipStreamSynchronize(h->s_main));            // (a pageable source: it has left the vector)
    a.lists = (float4*)h->ct_list; a.cols = (const CtCol*)h->ct_cols;
    return a;
}

// rows row0 .. row0 + n - 1 -> grids at d_out (and sums at d_share) on s_main, in launches of at most CT_PASS rows; enqueued, not awaited
void control_rows(EagleHandle* h, const ControlArgs& prepared, int row0, int n, uint8_t* d_out, int64_t* d_share)
{
    ControlArgs a = prepared;
    const size_t cells = (size_t)a.gw * a.gh;
    for (int f0 = 0; f0 < n; f0 += CT_PASS) {
        a.n = std::min(n - f0, CT_PASS);
        a.row0 = row0 + f0;
        a.out = d_out + (size_t)f0 * cells;
        a.share = d_share ? (unsigned long long*)d_share + f0 : nullptr;
        // bytes: the grids written, the positions and velocities of the sites read
        timed_launch(h, "control", (double)a.n * ((double)cells + 32.0 * a.ncols), h->s_main, [&] { control_launch(a, h->s_main); });
    }
}
}  // namespace eagle

extern "C" {

int eagle_control_size(const EagleControlParams* p, int* gw, int* gh)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!gw || !gh) fail(EAGLE_E_INVALID, "eagle_control_size: gw or gh is NULL");
    control_check(p);
    *gw = 105 * p->cells_per_metre; *gh = 68 * p->cells_per_metre;
    API_END(hh)
}

int eagle_control_device_grids(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleControlParams* p, uint8_t* d_out, int64_t* d_share)
{
    API_BEGIN_H(h)
    control_begin(h, t, row0, n, p, d_out);
    if (n == 0) return EAGLE_OK;
    control_rows(h, control_prepare(h, t, p, n), row0, n, d_out, d_share);
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    if (h->prof) collect_spans(h);
    API_END(h)
}

int eagle_control_grids(EagleHandle* h, EaglePostTable* t, int row0, int n, const EagleControlParams* p, uint8_t* out, int64_t* share)
{
    API_BEGIN_H(h)
    control_begin(h, t, row0, n, p, out);
    if (n == 0) return EAGLE_OK;
    const size_t cells = (size_t)7140 * p->cells_per_metre * p->cells_per_metre;
    // grids per pass: what CT_STAGING bytes of staging hold, the sums behind them
    const int batch = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(n, CT_PASS), CT_STAGING / (int64_t)(cells + 8)));
    const size_t share_off = ((size_t)batch * cells + 7) & ~(size_t)7;
    grow(&h->ct_grid, &h->ct_grid_cap, share_off + (size_t)batch * 8);
    const ControlArgs a = control_prepare(h, t, p, batch);
    uint8_t* d_g = (uint8_t*)h->ct_grid;
    int64_t* d_s = (int64_t*)(d_g + share_off);
    for (int i = 0; i < n; i += batch) {
        const int na = std::min(batch, n - i);
        control_rows(h, a, row0 + i, na, d_g, share ? d_s : nullptr);
        HIP_CHECK(hipMemcpyAsync(out + (size_t)i * cells, d_g, (size_t)na * cells, hipMemcpyDeviceToHost, h->s_main));
        if (share) HIP_CHECK(hipMemcpyAsync(share + i, d_s, (size_t)na * 8, hipMemcpyDeviceToHost, h->s_main));
        HIP_CHECK(hipStreamSynchronize(h->s_main));
        if (h->prof) collect_spans(h);
    }
    API_END(h)
}

int eagle_minimap_set_control(EaglePostTable* t, const EagleControlParams* p)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (p) { control_check(p); t->control = *p; }
    t->has_control = p != nullptr;
    API_END(h)
}

int eagle_op_control(int device, const double* values, const double* velocities, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids,
                     const int32_t* team_vals, int n_team, const EagleControlParams* p, int row0, int n, uint8_t* out_grid, int64_t* out_share)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !columns || !out_grid || rows < 0 || cols < 0 || n_team < 0 || (team_ids && n_team > 0 && !team_vals))
        fail(EAGLE_E_INVALID, "eagle_op_control: bad argument (values %p, columns %p, out %p, %d rows, %d columns, %d teams)", (const void*)values, (const void*)columns,
             (const void*)out_grid, rows, cols, n_team);
    control_check(p);
    if (!team_ids) fail(EAGLE_E_INVALID, "control: the table has no team mapping (team 0 is counted against the others)");
    if (!velocities) fail(EAGLE_E_INVALID, "control: the table has no velocities (eagle_op_velocities comes first)");
    control_window(rows, row0, n);
    if (n == 0) return EAGLE_OK;
    std::vector<CtCol> sc;
    control_columns(columns, cols, team_ids, team_vals, (size_t)n_team, sc);
    ControlArgs a = control_args(p);
    a.ncols = (int)sc.size(); a.stride = 1 + a.ncols; a.rows = rows;
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const size_t cells = (size_t)a.gw * a.gh, tb = (size_t)cols * rows * sizeof(double2);
    a.values = (const double2*)net.upload(values, tb);
    a.vel = (const double2*)net.upload(velocities, tb);
    sc.resize(std::max<size_t>(sc.size(), 2), CtCol{0, 0});                    // (a table without a site still uploads 16 bytes; ncols says how many count)
    a.cols = (const CtCol*)net.upload(sc.data(), sc.size() * sizeof(CtCol));
    a.lists = (float4*)net.get((size_t)std::min(n, CT_PASS) * a.stride * sizeof(float4));
    uint8_t* d_g = (uint8_t*)net.get((size_t)n * cells);
    unsigned long long* d_s = out_share ? (unsigned long long*)net.get((size_t)n * 8) : nullptr;
    for (int f0 = 0; f0 < n; f0 += CT_PASS) {
        ControlArgs b = a;
        b.n = std::min(n - f0, CT_PASS); b.row0 = row0 + f0; b.out = d_g + (size_t)f0 * cells; b.share = d_s ? d_s + f0 : nullptr;
        control_launch(b, nullptr);
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out_grid, d_g, (size_t)n * cells, hipMemcpyDeviceToHost));
    if (out_share) HIP_CHECK(hipMemcpy(out_share, d_s, (size_t)n * 8, hipMemcpyDeviceToHost));
    API_END(hh)
}

}  // extern "C"
