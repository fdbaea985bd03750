// K29 — player roles: a processed table resident in HBM (post.hip) -> per row and group the exact least-cost assignment of the present members to R
// role positions, re-estimated from the assignment over T rounds (include/eagle.h, eagle_post_roles / eagle_op_roles; tests/roles_ref.py is the written
// definition of every bit).  Members and quantisation are K26's (shape_columns; q = floor(x * 1024 + 0.5)); integers after that: |u| <= 2^21, a cost
// <= 2^45, a row's total < 2^49, every sum in 64 bits.  All accumulation is integer addition, so no result depends on an order.
//
//   roles_prepare_kernel   once.  One thread per row walks the member columns of group 0, then of group 1, twice: n, the sums and the centre first, then
//                          the centred positions.  It writes the row record (status, n, centre; cost 0, no columns), compacts the players of an ACTIVE
//                          row as int4 {ux, uy, member, column} [row][group][EAGLE_ROLE_CAP] and adds the seed statistics per member column: the walk is
//                          uniform over the wave, so the wave sums its 64 rows with a butterfly (64 x 2^21 fits 32 bits) and lane 0 issues one 64-bit
//                          atomic per figure.  The host reads the per-column figures back once and ranks the seeds.
//   roles_assign_kernel    the hot one, once per round.  A workgroup of RL_WAVES waves owns RL_ITEMS consecutive (row, group) pairs, a wave one pair
//                          at a time.  Staged once per workgroup: the role positions of both groups, the subsets of R roles ordered by popcount and the
//                          layer offsets.  Per pair: lane i forms row i of the cost matrix in LDS; the subset recurrence runs layer by layer, popcount
//                          descending, the lanes sharing the subsets of a layer (h in LDS, 8 KB per wave, indexed by the subset itself); the backtrack is n
//                          steps in which lane j tests role j and a ballot's lowest bit is the smallest j.  Lane j compares and stores col[j]; lane i adds
//                          player i to the workgroup's sums in LDS.  Behind a barrier the workgroup adds its non-zero sums to the NEXT model buffer with
//                          one atomic each: 100 per RL_ITEMS pairs, not 50 per pair.
//   roles_means_kernel     the next buffer's sums -> its positions (a role nobody played keeps the current one).  Two buffers ping-pong, so the assign
//                          kernel never reads what it adds to.
// The host reads changed[k] (4 bytes) behind every round and stops launching once it is 0: from there on nothing moves (tests/roles_ref.py).
//
// LDS of the assign kernel: RL_WAVES x (8192 h + 800 costs) + 800 sums + 160 positions + 2048 subsets + 48 offsets = 39 024 bytes.  A CU has 160 KB: four
// workgroups, 16 waves, 4 per SIMD; LDS, not registers, bounds the residency.  Waves of one workgroup never wait for each other inside the loop: the only
// barriers are behind the staging and in front of the flush; inside a wave LDS operations complete in order, so a wave-scope fence orders the layers.
#include "trails.h"

namespace eagle {

static constexpr int RL_CAP = EAGLE_ROLE_CAP;
static constexpr int RL_PREP_THREADS = 64;             // one wave per workgroup: 30 000 rows are 469 workgroups
static constexpr int RL_WAVES = 4;
static constexpr int RL_ITEMS = 32;                    // (row, group) pairs per workgroup of the assign kernel
static constexpr int RL_ACC = 5;                       // per role: count, sum ux, sum uy, sum ux^2, sum uy^2
typedef unsigned long long rl_u64;
static_assert(sizeof(EagleRoleParams) == 32 && sizeof(EagleRoleRow) == 64 && sizeof(EagleRoleGroup) == 448 && sizeof(EagleRoleModel) == 1024,
              "include/eagle.h states these sizes");

struct RlBuf { int32_t mean[2][RL_CAP][2]; rl_u64 acc[2][RL_CAP][RL_ACC]; };          // 160 + 800 bytes
struct RlTable { int32_t off[RL_CAP + 2]; uint16_t order[1 << RL_CAP]; };             // the subsets of R roles by popcount; off[k] .. off[k + 1]: popcount k

struct RlArgs {
    const double2* values;       // [column][row]
    const int32_t* gcols;        // group 0's columns in table order, then group 1's
    int rows, n0, n1, R, min_present;
    EagleRoleRow* rows_out;      // [rows][2]
    int8_t* mroles;              // [members][rows], preset to -1
    int4* players;               // [rows][2][RL_CAP] = {ux, uy, member, column} of an ACTIVE row
    rl_u64* seeds;               // [members][3] = count, sum ux, sum uy over the ACTIVE rows (zeroed in front of the launch)
    int32_t* active;             // [2] ACTIVE rows per group (zeroed)
    const RlBuf* cur;            // assign, means: the positions of this round
    RlBuf* nxt;                  // ... the sums of this round (zeroed), the positions of the next
    int32_t* changed;            // this round's counter (zeroed)
    const RlTable* table;
    int first, seeded;           // round 0: every pair counts as changed; bit g: group g has seeds
};

__device__ __forceinline__ bool rl_quantise(double2 v, int& qx, int& qy)
{
    if (!(fabs(v.x) <= MM_DOMAIN) || !(fabs(v.y) <= MM_DOMAIN)) return false;          // NaN, +-inf and the far field: K26's rule
    qx = (int)floor(v.x * 1024.0 + 0.5);
    qy = (int)floor(v.y * 1024.0 + 0.5);
    return true;
}

// floor((2 S + cnt) / (2 cnt)), cnt > 0
__host__ __device__ inline long long rl_rounded_mean(long long S, long long cnt)
{
    const long long a = 2 * S + cnt, b = 2 * cnt;
    long long q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}

__global__ __launch_bounds__(RL_PREP_THREADS) void roles_prepare_kernel(RlArgs a)
{
    const int r = blockIdx.x * RL_PREP_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = r < a.rows;
    const int rr = live ? r : a.rows - 1;                                // (a dead lane reads the last row and contributes nothing)
    #pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int base = g ? a.n0 : 0, ng = g ? a.n1 : a.n0;
        const int32_t* C = a.gcols + base;
        long long sx = 0, sy = 0;
        int n = 0;
        for (int k = 0; k < ng; ++k) {
            int qx, qy;
            if (!rl_quantise(a.values[(size_t)C[k] * a.rows + rr], qx, qy)) continue;
            sx += qx; sy += qy; ++n;
        }
        const int cx = n ? (int)rl_rounded_mean(sx, n) : 0, cy = n ? (int)rl_rounded_mean(sy, n) : 0;
        const int status = n == 0 ? EAGLE_ROLE_EMPTY : n < a.min_present ? EAGLE_ROLE_TOO_FEW : n > a.R ? EAGLE_ROLE_TOO_MANY : EAGLE_ROLE_ACTIVE;
        const bool act = live && status == EAGLE_ROLE_ACTIVE;
        if (live) {
            EagleRoleRow o;
            o.cost = 0; o.n = n; o.status = status; o.cx = cx; o.cy = cy;
            #pragma unroll
            for (int j = 0; j < RL_CAP; ++j) o.col[j] = -1;
            a.rows_out[(size_t)r * 2 + g] = o;
        }
        int4* P = a.players + ((size_t)rr * 2 + g) * RL_CAP;
        int i = 0;
        for (int k = 0; k < ng; ++k) {                                   // (uniform: every lane of the wave walks the same column)
            const int c = C[k];
            int qx = 0, qy = 0;
            const bool one = rl_quantise(a.values[(size_t)c * a.rows + rr], qx, qy) && act;
            int cnt = one ? 1 : 0, ux = one ? qx - cx : 0, uy = one ? qy - cy : 0;
            if (one) P[i++] = make_int4(ux, uy, base + k, c);            // (i < n <= R <= RL_CAP on an ACTIVE row)
            #pragma unroll
            for (int d = 32; d >= 1; d >>= 1) { cnt += __shfl_xor(cnt, d, 64); ux += __shfl_xor(ux, d, 64); uy += __shfl_xor(uy, d, 64); }
            if (lane == 0 && cnt) {
                rl_u64* S = a.seeds + (size_t)(base + k) * 3;
                atomicAdd(S, (rl_u64)cnt); atomicAdd(S + 1, (rl_u64)(long long)ux); atomicAdd(S + 2, (rl_u64)(long long)uy);
            }
        }
        const int na = __popcll(__ballot(act));
        if (lane == 0 && na) atomicAdd(a.active + g, na);
    }
}

struct RlShared {
    rl_u64 h[RL_WAVES][1 << RL_CAP];
    rl_u64 c[RL_WAVES][RL_CAP * RL_CAP];
    rl_u64 acc[2][RL_CAP][RL_ACC];
    int32_t mean[2][RL_CAP][2];
    int32_t off[RL_CAP + 2];
    uint16_t order[1 << RL_CAP];
};

// the layers of one wave follow each other through LDS: its operations there complete in order, the fence keeps the compiler from moving them
__device__ __forceinline__ void rl_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(64 * RL_WAVES) void roles_assign_kernel(RlArgs a)
{
    __shared__ RlShared S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, R = a.R;
    for (int i = tid; i < (1 << R); i += 64 * RL_WAVES) S.order[i] = a.table->order[i];
    if (tid < RL_CAP + 2) S.off[tid] = a.table->off[tid];
    if (tid < 2 * RL_CAP * 2) (&S.mean[0][0][0])[tid] = (&a.cur->mean[0][0][0])[tid];
    for (int i = tid; i < 2 * RL_CAP * RL_ACC; i += 64 * RL_WAVES) (&S.acc[0][0][0])[i] = 0;
    __syncthreads();
    rl_u64* H = S.h[wave];
    rl_u64* Cw = S.c[wave];
    const long long item0 = (long long)blockIdx.x * RL_ITEMS, items = 2LL * a.rows;
    int moved = 0;
    for (int it = wave; it < RL_ITEMS; it += RL_WAVES) {
        const long long item = item0 + it;
        if (item >= items) break;                                        // (uniform over the wave, as everything that steers it below)
        const int r = (int)(item >> 1), g = (int)(item & 1);
        if (!((a.seeded >> g) & 1)) continue;
        EagleRoleRow* o = a.rows_out + item;
        if (__builtin_amdgcn_readfirstlane(o->status) != EAGLE_ROLE_ACTIVE) continue;
        const int n = __builtin_amdgcn_readfirstlane(o->n);              // min_present <= n <= R
        const int4 p = lane < n ? a.players[item * RL_CAP + lane] : make_int4(0, 0, -1, -1);
        if (lane < n)
            for (int j = 0; j < R; ++j) {
                const long long dx = p.x - S.mean[g][j][0], dy = p.y - S.mean[g][j][1];
                Cw[lane * RL_CAP + j] = (rl_u64)(dx * dx + dy * dy);
            }
        for (int e = S.off[n] + lane; e < S.off[n + 1]; e += 64) H[S.order[e]] = 0;
        rl_wave_sync();
        for (int k = n - 1; k >= 0; --k) {
            const rl_u64* ck = Cw + k * RL_CAP;
            for (int e = S.off[k] + lane; e < S.off[k + 1]; e += 64) {
                const int m = S.order[e];
                rl_u64 best = ~(rl_u64)0;
                for (int j = 0; j < R; ++j) {
                    const rl_u64 t = ck[j] + H[m | (1 << j)];            // (j in m: this layer's own slot, whatever it holds; not taken)
                    best = (!((m >> j) & 1) && t < best) ? t : best;
                }
                H[m] = best;
            }
            rl_wave_sync();
        }
        int mask = 0, myrole = -1, mycol = -1;
        for (int k = 0; k < n; ++k) {
            const int jl = lane < R ? lane : 0;
            const bool hit = lane < R && !((mask >> jl) & 1) && Cw[k * RL_CAP + jl] + H[mask | (1 << jl)] == H[mask];
            const rl_u64 b = __ballot(hit);
            if (!b) break;                                               // (never: the minimum is attained)
            const int j = __ffsll((long long)b) - 1;
            const int col = __shfl(p.w, k, 64);
            if (lane == k) myrole = j;
            if (lane == j) mycol = col;
            mask |= 1 << j;
        }
        bool diff = false;
        if (lane < RL_CAP) {
            diff = a.first || o->col[lane] != mycol;
            o->col[lane] = mycol;
        }
        if (__ballot(diff)) ++moved;
        if (lane == 0) o->cost = (long long)H[0];
        if (lane < n && myrole >= 0) {
            a.mroles[(size_t)p.z * a.rows + r] = (int8_t)myrole;
            rl_u64* A = S.acc[g][myrole];
            atomicAdd(A, (rl_u64)1); atomicAdd(A + 1, (rl_u64)(long long)p.x); atomicAdd(A + 2, (rl_u64)(long long)p.y);
            atomicAdd(A + 3, (rl_u64)((long long)p.x * p.x)); atomicAdd(A + 4, (rl_u64)((long long)p.y * p.y));
        }
        rl_wave_sync();                                                  // (the next pair overwrites h and the costs)
    }
    if (lane == 0 && moved) atomicAdd(a.changed, moved);
    __syncthreads();
    for (int i = tid; i < 2 * RL_CAP * RL_ACC; i += 64 * RL_WAVES) {
        const rl_u64 v = (&S.acc[0][0][0])[i];
        if (v) atomicAdd(&a.nxt->acc[0][0][0] + i, v);
    }
}

__global__ __launch_bounds__(64) void roles_means_kernel(RlArgs a)
{
    const int t = threadIdx.x;
    if (t >= 2 * RL_CAP) return;
    const int g = t / RL_CAP, j = t % RL_CAP;
    const long long cnt = (long long)a.nxt->acc[g][j][0];
    #pragma unroll
    for (int x = 0; x < 2; ++x)
        a.nxt->mean[g][j][x] = cnt ? (int32_t)rl_rounded_mean((long long)a.nxt->acc[g][j][1 + x], cnt) : a.cur->mean[g][j][x];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void roles_check(const char* who, const EagleRoleParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the role parameters are NULL", who);
    if (p->roles < 2 || p->roles > EAGLE_ROLE_CAP) fail(EAGLE_E_INVALID, "%s: roles %d must lie within 2 .. %d", who, p->roles, EAGLE_ROLE_CAP);
    if (p->min_present < 2 || p->min_present > p->roles) fail(EAGLE_E_INVALID, "%s: min_present %d must lie within 2 .. roles (%d)", who, p->min_present, p->roles);
    if (p->iterations < 1 || p->iterations > 32) fail(EAGLE_E_INVALID, "%s: iterations %d must lie within 1 .. 32", who, p->iterations);
    for (int k = 0; k < 5; ++k)
        if (p->reserved[k]) fail(EAGLE_E_INVALID, "%s: reserved word %d of the role parameters is %d, not 0", who, k, p->reserved[k]);
}

static size_t rl_up(size_t b) { return (std::max<size_t>(b, 16) + 255) & ~(size_t)255; }

// what a call keeps: records | model | member roles
static size_t roles_kept(size_t rows, size_t nmem) { return rl_up(rows * 2 * sizeof(EagleRoleRow)) + rl_up(sizeof(EagleRoleModel)) + rl_up(nmem * rows); }

struct RlPlan { size_t cols, players, seeds, active, buf, changed, table, total; };

static RlPlan roles_plan(size_t rows, size_t nmem)
{
    RlPlan o{};
    size_t at = 0;
    auto take = [&](size_t b) { const size_t was = at; at += rl_up(b); return was; };
    o.cols = take(nmem * 4); o.players = take(rows * 2 * RL_CAP * sizeof(int4)); o.seeds = take(nmem * 3 * 8); o.active = take(8);
    o.buf = take(2 * rl_up(sizeof(RlBuf))); o.changed = take(32 * 4); o.table = take(sizeof(RlTable));
    o.total = at;
    return o;
}

static void roles_budget(const char* who, size_t need, int64_t max_bytes)
{
    double budget = (double)max_bytes;
    if (max_bytes <= 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = 0.9 * (double)free_b;
    }
    if ((double)need > budget) fail(EAGLE_E_INVALID, "%s: the roles need %.0f bytes of device memory, the budget is %.0f", who, (double)need, budget);
}

// The launches on stream s (h: timed under its profiling mode, or nullptr); returns when d_rows, d_mroles and d_model are complete.  rows > 0.
static void roles_run(EagleHandle* h, const ShapeCols& sc, const double2* d_values, int rows, const EagleRoleParams* p, EagleRoleRow* d_rows, int8_t* d_mroles,
                      EagleRoleModel* d_model, hipStream_t s)
{
    const size_t nmem = (size_t)sc.n0 + sc.n1, n = (size_t)rows;
    const int R = p->roles;
    const RlPlan pl = roles_plan(n, nmem);
    RlTable tab{};
    {
        int at = 0;
        for (int k = 0; k <= R; ++k) {
            tab.off[k] = at;
            for (int m = 0; m < (1 << R); ++m)
                if (__builtin_popcount(m) == k) tab.order[at++] = (uint16_t)m;
        }
        for (int k = R + 1; k < RL_CAP + 2; ++k) tab.off[k] = at;
    }
    uint8_t* base = nullptr;
    HIP_CHECK(hipMalloc((void**)&base, pl.total));
    try {
        RlArgs a{};
        a.values = d_values; a.gcols = (const int32_t*)(base + pl.cols); a.rows = rows; a.n0 = sc.n0; a.n1 = sc.n1; a.R = R; a.min_present = p->min_present;
        a.rows_out = d_rows; a.mroles = d_mroles; a.players = (int4*)(base + pl.players); a.seeds = (rl_u64*)(base + pl.seeds); a.active = (int32_t*)(base + pl.active);
        a.table = (const RlTable*)(base + pl.table);
        RlBuf* bufs[2] = {(RlBuf*)(base + pl.buf), (RlBuf*)(base + pl.buf + rl_up(sizeof(RlBuf)))};
        int32_t* d_changed = (int32_t*)(base + pl.changed);
        if (nmem) HIP_CHECK(hipMemcpyAsync(base + pl.cols, sc.gcols.data(), nmem * 4, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemcpyAsync(base + pl.table, &tab, sizeof tab, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipMemsetAsync(base + pl.seeds, 0, pl.table - pl.seeds, s));         // seeds, active, both buffers, changed
        HIP_CHECK(hipMemsetAsync(d_mroles, 0xff, std::max<size_t>(nmem * n, 1), s));
        auto run = [&](const char* name, double bytes, const std::function<void()>& fn) {
            if (h) timed_launch(h, name, bytes, s, fn); else fn();
        };
        // bytes: every member cell read twice, a record and the players of a row written
        run("roles_prepare", 32.0 * (double)nmem * (double)n + (double)n * 2.0 * (64.0 + 160.0), [&] {
            hipLaunchKernelGGL(roles_prepare_kernel, dim3((rows + RL_PREP_THREADS - 1) / RL_PREP_THREADS), dim3(RL_PREP_THREADS), 0, s, a);
            HIP_CHECK(hipGetLastError());
        });
        std::vector<rl_u64> seeds(std::max<size_t>(nmem * 3, 1));
        int32_t active[2] = {0, 0};
        if (nmem) HIP_CHECK(hipMemcpyAsync(seeds.data(), a.seeds, nmem * 24, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(active, a.active, 8, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        // the seeds: the columns of a group by (count descending, column ascending: the members are listed in column order), the first R with a count
        RlBuf first{};
        for (int g = 0; g < 2; ++g) {
            const int b0 = g ? sc.n0 : 0, ng = g ? sc.n1 : sc.n0;
            std::vector<int> order;
            for (int m = 0; m < ng; ++m)
                if (seeds[(size_t)(b0 + m) * 3]) order.push_back(m);
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return seeds[(size_t)(b0 + x) * 3] > seeds[(size_t)(b0 + y) * 3]; });
            if ((int)order.size() < R) continue;
            a.seeded |= 1 << g;
            for (int j = 0; j < R; ++j) {
                const rl_u64* S = &seeds[(size_t)(b0 + order[j]) * 3];
                first.mean[g][j][0] = (int32_t)rl_rounded_mean((long long)S[1], (long long)S[0]);
                first.mean[g][j][1] = (int32_t)rl_rounded_mean((long long)S[2], (long long)S[0]);
            }
        }
        EagleRoleModel model{};
        RlBuf used = first, sums{};
        if (a.seeded) {
            HIP_CHECK(hipMemcpyAsync(bufs[0], &first, sizeof first, hipMemcpyHostToDevice, s));
            const int blocks = (int)((2 * (long long)rows + RL_ITEMS - 1) / RL_ITEMS);
            int last = 0;
            for (int k = 0; k < p->iterations; ++k) {
                a.cur = bufs[k & 1]; a.nxt = bufs[(k & 1) ^ 1]; a.changed = d_changed + k; a.first = k == 0;
                HIP_CHECK(hipMemsetAsync(&a.nxt->acc[0][0][0], 0, sizeof(a.nxt->acc), s));
                // bytes: the players and the record of every pair read, the columns, the cost and the members' roles written
                run("roles_assign", (double)n * 2.0 * (160.0 + 64.0 + 48.0 + 10.0), [&] {
                    hipLaunchKernelGGL(roles_assign_kernel, dim3(blocks), dim3(64 * RL_WAVES), 0, s, a);
                    HIP_CHECK(hipGetLastError());
                });
                run("roles_means", 2.0 * sizeof(RlBuf), [&] {
                    hipLaunchKernelGGL(roles_means_kernel, dim3(1), dim3(64), 0, s, a);
                    HIP_CHECK(hipGetLastError());
                });
                HIP_CHECK(hipMemcpyAsync(&model.changed[k], a.changed, 4, hipMemcpyDeviceToHost, s));
                HIP_CHECK(hipStreamSynchronize(s));
                last = k;
                if (model.changed[k] == 0) break;                        // nothing moves any more: the rounds left would repeat this one
            }
            HIP_CHECK(hipMemcpyAsync(&used, bufs[last & 1], sizeof used, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipMemcpyAsync(&sums, bufs[(last & 1) ^ 1], sizeof sums, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
        }
        for (int g = 0; g < 2; ++g) {
            EagleRoleGroup& o = model.group[g];
            o.active_rows = active[g];
            o.status = (a.seeded >> g) & 1 ? EAGLE_ROLE_MODEL_OK : EAGLE_ROLE_NO_SEEDS;
            if (o.status != EAGLE_ROLE_MODEL_OK) continue;
            for (int j = 0; j < R; ++j) {
                o.count[j] = (int32_t)sums.acc[g][j][0];
                for (int x = 0; x < 2; ++x) {
                    o.mean[j][x] = used.mean[g][j][x];
                    o.sum[j][x] = (int64_t)sums.acc[g][j][1 + x];
                    o.sum2[j][x] = (int64_t)sums.acc[g][j][3 + x];
                }
            }
        }
        HIP_CHECK(hipMemcpyAsync(d_model, &model, sizeof model, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (h && h->prof) collect_spans(h);
    } catch (...) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(base);
        throw;
    }
    HIP_CHECK(hipFree(base));
}

}  // namespace eagle

extern "C" {

int eagle_post_roles(EagleHandle* h, EaglePostTable* t, const EagleRoleParams* p)
{
    API_BEGIN_H(h)
    if (!t) fail(EAGLE_E_INVALID, "eagle_post_roles: table is NULL");
    if (t->h != h) fail(EAGLE_E_INVALID, "eagle_post_roles: the table belongs to another handle");
    roles_check("eagle_post_roles", p);
    const int32_t none = 0;                                              // (a mapping of no entries is a mapping: nobody is a member)
    const ShapeCols sc = shape_columns("eagle_post_roles", t->columns.data(), t->cols, !t->has_team ? nullptr : t->team_ids.empty() ? &none : t->team_ids.data(),
                                       t->team_vals.data(), t->has_team ? t->team_ids.size() : 0);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const size_t rows = (size_t)t->rows, nmem = (size_t)sc.n0 + sc.n1;
    // the budget: what this call allocates, the result (once: the columns of a table never change) and the scratch
    roles_budget("eagle_post_roles", (t->d_roles ? 0 : roles_kept(rows, nmem)) + (rows ? roles_plan(rows, nmem).total : 0), t->max_bytes);
    if (!t->d_roles) HIP_CHECK(hipMalloc((void**)&t->d_roles, roles_kept(rows, nmem)));
    t->has_roles = false;                                                // the arrays are rewritten in place: a call that fails here leaves no result
    t->roles_members = (int)nmem;
    if (rows) {
        uint8_t* d = (uint8_t*)t->d_roles;
        roles_run(h, sc, (const double2*)t->d_values, t->rows, p, (EagleRoleRow*)d, (int8_t*)(d + rl_up(rows * 2 * sizeof(EagleRoleRow)) + rl_up(sizeof(EagleRoleModel))),
                  (EagleRoleModel*)(d + rl_up(rows * 2 * sizeof(EagleRoleRow))), h->s_main);
    }
    t->has_roles = true;
    API_END(h)
}

int eagle_post_roles_values(EaglePostTable* t, EagleRoleRow* rows_out, int8_t* member_roles, EagleRoleModel* model)
{
    if (!t) return EAGLE_E_INVALID;
    EagleHandle* h = t->h;
    API_BEGIN
    if (!t->has_roles) fail(EAGLE_E_INVALID, "eagle_post_roles_values: the table has no roles (eagle_post_roles)");
    const size_t rows = (size_t)t->rows, nmem = (size_t)t->roles_members;
    if (rows) {
        HIP_CHECK(hipSetDevice(h->cfg.device));
        const uint8_t* d = (const uint8_t*)t->d_roles;
        if (rows_out) HIP_CHECK(hipMemcpy(rows_out, d, rows * 2 * sizeof(EagleRoleRow), hipMemcpyDeviceToHost));
        if (model) HIP_CHECK(hipMemcpy(model, d + rl_up(rows * 2 * sizeof(EagleRoleRow)), sizeof(EagleRoleModel), hipMemcpyDeviceToHost));
        if (member_roles && nmem)
            HIP_CHECK(hipMemcpy(member_roles, d + rl_up(rows * 2 * sizeof(EagleRoleRow)) + rl_up(sizeof(EagleRoleModel)), nmem * rows, hipMemcpyDeviceToHost));
    }
    API_END(h)
}

int eagle_post_device_roles(const EaglePostTable* t, const EagleRoleRow** d_rows, const int8_t** d_member_roles, const EagleRoleModel** d_model, int* n_members)
{
    if (!t || !d_rows || !d_member_roles || !d_model) return EAGLE_E_INVALID;
    const uint8_t* d = t->has_roles ? (const uint8_t*)t->d_roles : nullptr;
    const size_t rb = eagle::rl_up((size_t)t->rows * 2 * sizeof(EagleRoleRow));
    *d_rows = (const EagleRoleRow*)d;
    *d_model = d ? (const EagleRoleModel*)(d + rb) : nullptr;
    *d_member_roles = d ? (const int8_t*)(d + rb + eagle::rl_up(sizeof(EagleRoleModel))) : nullptr;
    if (n_members) *n_members = d ? t->roles_members : 0;
    return EAGLE_OK;
}

int eagle_op_roles(int device, const double* values, const EaglePostColumn* columns, int rows, int cols, const int32_t* team_ids, const int32_t* team_vals, int n_team,
                   const EagleRoleParams* p, EagleRoleRow* rows_out, int8_t* member_roles, EagleRoleModel* model)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!values || !columns || rows < 0 || cols < 0 || n_team < 0 || (team_ids && n_team > 0 && !team_vals))
        fail(EAGLE_E_INVALID, "eagle_op_roles: bad argument (values %p, columns %p, %d rows, %d columns, %d teams)", (const void*)values, (const void*)columns, rows, cols,
             n_team);
    roles_check("eagle_op_roles", p);
    const ShapeCols sc = shape_columns("eagle_op_roles", columns, cols, team_ids, team_vals, (size_t)n_team);
    if (rows == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    const size_t n = (size_t)rows, nmem = (size_t)sc.n0 + sc.n1, rb = rl_up(n * 2 * sizeof(EagleRoleRow)), mb = rl_up(sizeof(EagleRoleModel));
    roles_budget("eagle_op_roles", (size_t)cols * n * sizeof(double2) + roles_kept(n, nmem) + roles_plan(n, nmem).total, 0);
    Net net;
    const double2* d_v = (const double2*)net.upload(values, std::max<size_t>((size_t)cols * n * sizeof(double2), 16));
    uint8_t* d = (uint8_t*)net.get(roles_kept(n, nmem));
    roles_run(nullptr, sc, d_v, rows, p, (EagleRoleRow*)d, (int8_t*)(d + rb + mb), (EagleRoleModel*)(d + rb), nullptr);
    if (rows_out) HIP_CHECK(hipMemcpy(rows_out, d, n * 2 * sizeof(EagleRoleRow), hipMemcpyDeviceToHost));
    if (model) HIP_CHECK(hipMemcpy(model, d + rb, sizeof(EagleRoleModel), hipMemcpyDeviceToHost));
    if (member_roles && nmem) HIP_CHECK(hipMemcpy(member_roles, d + rb + mb, nmem * n, hipMemcpyDeviceToHost));
    API_END(hh)
}

}  // extern "C"
