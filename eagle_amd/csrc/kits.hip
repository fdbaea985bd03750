// K36 — team assignment by clustering kit colours over the clip (include/eagle.h, eagle_team_cluster; own specification: tests/kits_ref.py defines
// every output bit, twice).  The reference's rule (teams.hip + eagle_amd/teams.py) counts pixels into eleven named HSV ranges and takes the two most
// common names: two kits inside one named range (navy and sky blue) end in one team.  This stage describes the shirt window of every player crop by an
// integer histogram of 34 colour bins, sums the normalised histograms per tracker id and splits the ids by an exact weighted 2-medoid clustering:
// every pair of voters is tried as the two centres.  No seeding, no iteration, no floating point: integer sums do not depend on the order in which
// they arrive, so two runs give identical bytes.
//   kit_hist_kernel    one wave per crop, four crops per workgroup: the lanes walk the shirt window row-major, the histogram is built per wave in LDS
//                      with integer LDS atomics, lanes 0 .. 33 normalise (q = units * 4096 / (12 n)), write the crop's record and add q into the id's
//                      row with 64-bit integer global atomics (4096 per crop, up to 2^22 crops: 34 bits)
//   kit_prep_kernel    one thread per id: the signature p = sum * 65536 / T, and the voters (used >= min_crops) compacted in slot order by a scan
//   kit_dist_kernel    the matrix D of L1 distances between the voters' signatures (uint32, at most 1024 x 1024)
//   kit_pair_kernel    workgroup x takes the pairs (x, y > x): row x of D and the weights wait in LDS, each wave sums w_t min(D[x][t], D[y][t]) over the
//                      voters t with row y read coalesced, the waves' best keys meet in LDS and one 64-bit atomicMin per workgroup goes to the packed
//                      key cost << 20 | pair rank: exact, free of any order, and the tie rule (the earlier pair) is the key itself
//   kit_assign_kernel  one thread per id: distances to the two medoids, weak, neither, the clusters' weights, the swap for team 0, the records
#include "runtime.h"

namespace eagle {

static_assert(sizeof(EagleKitParams) == 32 && sizeof(EagleKitCrop) == 144 && sizeof(EagleKitId) == 160 && sizeof(EagleKitModel) == 64, "include/eagle.h states these sizes");

constexpr int KIT_BINS = EAGLE_KIT_BINS;
constexpr int KIT_MAX_IDS = EAGLE_KIT_MAX_IDS;
constexpr int KIT_MAX_CROPS = 1 << 22;
constexpr long long KIT_MAX_SUM = 1ll << 34;
constexpr unsigned long long KIT_NO_KEY = ~0ull;

// cv2's 8-bit BGR2HSV in fixed point, as bgr2hsv_px of teams.hip
__device__ __forceinline__ void kit_hsv(int b, int g, int r, int* ho, int* so, int* vo)
{
    int v = b, vmin = b;
    if (g > v) v = g;
    if (r > v) v = r;
    if (g < vmin) vmin = g;
    if (r < vmin) vmin = r;
    const int diff = v - vmin;
    const int sdiv = v ? (int)rint((double)(255 << 12) / (double)v) : 0;
    const int hdiv = diff ? (int)rint((double)(180 << 12) / (6. * (double)diff)) : 0;
    const int s = (diff * sdiv + (1 << 11)) >> 12;
    int hh = v == r ? g - b : v == g ? b - r + 2 * diff : r - g + 4 * diff;
    hh = (hh * hdiv + (1 << 11)) >> 12;
    hh += hh < 0 ? 180 : 0;
    *ho = hh & 255; *so = s & 255; *vo = v;
}

struct KitHistArgs {
    const uint8_t* bgr; int n_frames, fh, fw;
    const EagleCrop* crops; const int32_t* slots; int n_crops, min_pixels;
    EagleKitCrop* recs;                      // [n_crops]
    unsigned long long* sums;                // [n_ids][34]
    int32_t* used; int32_t* skipped;         // [n_ids]
};

__global__ __launch_bounds__(256) void kit_hist_kernel(KitHistArgs a)
{
    __shared__ unsigned s_hist[4][KIT_BINS + 2];                               // per wave: the bins and the counted pixels
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ci = blockIdx.x * 4 + wave;
    const bool live = ci < a.n_crops;                                          // (wave-uniform; nobody leaves before the barriers)
    if (lane < KIT_BINS + 2) s_hist[wave][lane] = 0;
    int flag = 0, wx0 = 0, wy0 = 0, ww = 0, wh = 0, frame = 0;
    if (live) {
        const EagleCrop c = a.crops[ci];
        const long long w = (long long)c.x2 - c.x1, h = (long long)c.y2 - c.y1;
        if (w <= 0 || h <= 0) flag = EAGLE_KIT_CROP_EMPTY;
        else if (c.frame < 0 || c.frame >= a.n_frames || c.x1 < 0 || c.y1 < 0 || c.x2 > a.fw || c.y2 > a.fh) flag = EAGLE_KIT_CROP_OUTSIDE;
        else {
            frame = c.frame;
            wx0 = c.x1 + (int)(w / 4); ww = c.x2 - (int)(w / 4) - wx0;
            wy0 = c.y1 + (int)(h / 5); wh = c.y1 + (int)(h / 2) - wy0;
            if (ww <= 0 || wh <= 0) flag = EAGLE_KIT_CROP_EMPTY;
        }
    }
    __syncthreads();
    if (live && !flag) {
        const uint8_t* base = a.bgr + ((size_t)frame * a.fh + wy0) * a.fw * 3 + (size_t)wx0 * 3;
        const int total = ww * wh;
        unsigned* hist = s_hist[wave];
        unsigned counted = 0;                                                  // per lane; one LDS atomic per lane behind the loop
        for (int i = lane; i < total; i += 64) {
            const int yy = i / ww, xx = i - yy * ww;
            const uint8_t* p = base + ((size_t)yy * a.fw + xx) * 3;
            const int b = p[0], g = p[1], r = p[2];
            if (g >= 48 && g - max(r, b) >= 16) continue;                      // grass (the shots stage's key)
            int hh, ss, vv;
            kit_hsv(b, g, r, &hh, &ss, &vv);
            if (ss >= 64 && vv >= 48) {
                const int t = (hh + 174) % 180, k = t / 12, f = t - 12 * k, up = vv < 144 ? 0 : 15;
                atomicAdd(&hist[up + k], (unsigned)(12 - f));
                if (f) atomicAdd(&hist[up + (k + 1) % 15], (unsigned)f);
            } else {
                atomicAdd(&hist[30 + (vv >> 6)], 12u);
            }
            ++counted;
        }
        if (counted) atomicAdd(&hist[KIT_BINS], counted);
    }
    __syncthreads();
    if (!live) return;
    const int n = (int)s_hist[wave][KIT_BINS];
    if (!flag && n < a.min_pixels) flag = EAGLE_KIT_CROP_FEW;
    const int slot = a.slots[ci];                                              // (checked on the host: 0 .. n_ids - 1)
    if (lane < KIT_BINS) {
        const unsigned u = s_hist[wave][lane];
        if (a.recs) a.recs[ci].units[lane] = u;
        if (!flag) {
            const unsigned long long q = ((unsigned long long)u * 4096ull) / (12ull * (unsigned long long)n);
            if (q) atomicAdd(&a.sums[(size_t)slot * KIT_BINS + lane], q);
        }
    }
    if (lane == 0) {
        if (a.recs) { a.recs[ci].n = n; a.recs[ci].flags = flag; }
        atomicAdd(flag ? &a.skipped[slot] : &a.used[slot], 1);
    }
}

struct KitArgs {
    const unsigned long long* sums;          // [n_ids][34]
    const int32_t* used; const int32_t* skipped;
    int n_ids, min_crops, outlier;
    uint32_t* p;                             // [n_ids][34]
    int32_t* vlist;                          // [n_ids] the voters' slots, ascending
    int32_t* nv;                             // [1]
    uint32_t* D;                             // [nv][nv]
    unsigned long long* key;                 // [1]
    EagleKitId* ids; EagleKitModel* model;
};

__global__ __launch_bounds__(1024) void kit_prep_kernel(KitArgs a)
{
    __shared__ int s_scan[1024];
    const int i = threadIdx.x;
    int voter = 0;
    if (i < a.n_ids) {
        const int used = a.used[i];
        unsigned long long T = 0;
        for (int b = 0; b < KIT_BINS; ++b) T += a.sums[(size_t)i * KIT_BINS + b];
        for (int b = 0; b < KIT_BINS; ++b) a.p[(size_t)i * KIT_BINS + b] = used > 0 && T ? (uint32_t)((a.sums[(size_t)i * KIT_BINS + b] * 65536ull) / T) : 0u;
        voter = used >= a.min_crops ? 1 : 0;
    }
    s_scan[i] = voter;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                                 // inclusive scan
        const int v = i >= off ? s_scan[i - off] : 0;
        __syncthreads();
        s_scan[i] += v;
        __syncthreads();
    }
    if (voter) a.vlist[s_scan[i] - 1] = i;
    if (i == 1023) { *a.nv = s_scan[1023]; *a.key = KIT_NO_KEY; }
}

__device__ __forceinline__ unsigned kit_l1(const uint32_t* x, const uint32_t* y)
{
    unsigned d = 0;
    for (int b = 0; b < KIT_BINS; ++b) { const unsigned u = x[b], v = y[b]; d += u > v ? u - v : v - u; }
    return d;
}

__global__ __launch_bounds__(256) void kit_dist_kernel(KitArgs a)
{
    const int nv = *a.nv;
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= nv || y >= nv) return;
    a.D[(size_t)y * nv + x] = kit_l1(a.p + (size_t)a.vlist[x] * KIT_BINS, a.p + (size_t)a.vlist[y] * KIT_BINS);
}

__global__ __launch_bounds__(256) void kit_pair_kernel(KitArgs a)
{
    __shared__ uint32_t s_row[KIT_MAX_IDS];
    __shared__ uint32_t s_w[KIT_MAX_IDS];
    __shared__ unsigned long long s_key[4];
    const int nv = *a.nv, x = blockIdx.x;
    if (x >= nv - 1) return;                                                   // (uniform over the workgroup)
    for (int t = threadIdx.x; t < nv; t += 256) { s_row[t] = a.D[(size_t)x * nv + t]; s_w[t] = (uint32_t)a.used[a.vlist[t]]; }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long rank0 = (unsigned long long)x * (unsigned long long)nv - (unsigned long long)x * (unsigned long long)(x + 1) / 2ull;
    unsigned long long best = KIT_NO_KEY;
    for (int y = x + 1 + wave; y < nv; y += 4) {
        const uint32_t* row = a.D + (size_t)y * nv;
        unsigned long long cost = 0;
        for (int t = lane; t < nv; t += 64) cost += (unsigned long long)s_w[t] * (unsigned long long)min(s_row[t], row[t]);
        for (int off = 32; off; off >>= 1) cost += __shfl_xor(cost, off, 64);
        const unsigned long long key = cost << 20 | (rank0 + (unsigned long long)(y - x - 1));
        best = key < best ? key : best;
    }
    if (lane == 0) s_key[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) best = s_key[k] < best ? s_key[k] : best;
        if (best != KIT_NO_KEY) atomicMin(a.key, best);
    }
}

__global__ __launch_bounds__(1024) void kit_assign_kernel(KitArgs a)
{
    __shared__ int s_ab[2];
    __shared__ unsigned long long s_wsum[2];
    __shared__ int s_neither;
    const int i = threadIdx.x, nv = *a.nv;
    const bool have = i < a.n_ids && a.used[i] > 0;
    const int used = i < a.n_ids ? a.used[i] : 0;
    const bool voter = i < a.n_ids && used >= a.min_crops;
    if (i < 2) { s_wsum[i] = 0; s_ab[i] = -1; }
    if (i == 0) s_neither = 0;
    __syncthreads();
    EagleKitId rec{};
    if (i < a.n_ids) {
        rec.used = used; rec.skipped = a.skipped[i]; rec.team = -1;
        for (int b = 0; b < KIT_BINS; ++b) rec.p[b] = a.p[(size_t)i * KIT_BINS + b];
    }
    if (nv < 2) {                                                              // fewer than two voters: one team
        if (have) { rec.team = 0; rec.flags = EAGLE_KIT_ID_SINGLE | (voter ? 0 : EAGLE_KIT_ID_WEAK); }
        if (voter) atomicAdd(&s_wsum[0], (unsigned long long)used);
        __syncthreads();
        if (i < a.n_ids && a.ids) a.ids[i] = rec;
        if (i == 0 && a.model) {
            EagleKitModel m{};
            m.a = m.b = -1; m.voters = nv; m.flags = EAGLE_KIT_MODEL_SINGLE; m.w[0] = (int64_t)s_wsum[0];
            *a.model = m;
        }
        return;
    }
    const unsigned long long key = *a.key;
    const long long rank = (long long)(key & ((1ull << 20) - 1));
    if (i < nv - 1) {                                                          // the pair of that rank: row i holds the ranks start .. start + nv - 2 - i
        const long long start = (long long)i * nv - (long long)i * (i + 1) / 2;
        if (rank >= start && rank < start + (nv - 1 - i)) { s_ab[0] = a.vlist[i]; s_ab[1] = a.vlist[i + 1 + (int)(rank - start)]; }
    }
    __syncthreads();
    const int ma = s_ab[0], mb = s_ab[1];
    if (ma < 0 || mb < 0) return;                                              // (cannot happen: every rank lies in one row)
    const unsigned dab = kit_l1(a.p + (size_t)ma * KIT_BINS, a.p + (size_t)mb * KIT_BINS);
    unsigned da = 0, db = 0;
    int cluster = 0;
    bool neither = false;
    if (have) {
        da = kit_l1(rec.p, a.p + (size_t)ma * KIT_BINS);
        db = kit_l1(rec.p, a.p + (size_t)mb * KIT_BINS);
        cluster = db < da ? 1 : 0;
        const unsigned long long dn = cluster ? db : da;
        neither = a.outlier > 0 && dn * 1024ull > (unsigned long long)a.outlier * (unsigned long long)dab;
        if (voter && !neither) atomicAdd(&s_wsum[cluster], (unsigned long long)used);
        if (neither) atomicAdd(&s_neither, 1);
    }
    __syncthreads();
    const int swap = s_wsum[1] > s_wsum[0] ? 1 : 0;
    if (have) {
        rec.team = neither ? -1 : (cluster ^ swap);
        rec.flags = (voter ? 0 : EAGLE_KIT_ID_WEAK) | (neither ? EAGLE_KIT_ID_NEITHER : 0);
        rec.d[swap] = da; rec.d[1 - swap] = db;                                // d[k]: to the medoid of team k
    }
    if (i < a.n_ids && a.ids) a.ids[i] = rec;
    if (i == 0 && a.model) {
        EagleKitModel m{};
        m.a = ma; m.b = mb; m.dab = dab; m.voters = nv; m.cost = (int64_t)(key >> 20);
        m.w[0] = (int64_t)s_wsum[swap]; m.w[1] = (int64_t)s_wsum[1 - swap];
        m.neither = s_neither; m.flags = swap ? EAGLE_KIT_MODEL_SWAPPED : 0; m.team_of_a = swap;
        *a.model = m;
    }
}

static void kit_params_check(const char* who, const EagleKitParams* p)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the parameters are NULL", who);
    if (p->min_pixels < 1 || p->min_pixels > (1 << 20)) fail(EAGLE_E_INVALID, "%s: min_pixels %d lies outside 1 .. %d", who, p->min_pixels, 1 << 20);
    if (p->min_crops < 1 || p->min_crops > (1 << 16)) fail(EAGLE_E_INVALID, "%s: min_crops %d lies outside 1 .. %d", who, p->min_crops, 1 << 16);
    if (p->outlier < 0 || p->outlier > (1 << 20)) fail(EAGLE_E_INVALID, "%s: outlier %d lies outside 0 .. %d (in 1/1024 of the distance between the medoids; 0: off)", who, p->outlier, 1 << 20);
    for (int k = 0; k < 5; ++k)
        if (p->reserved[k]) fail(EAGLE_E_INVALID, "%s: reserved word %d of the parameters is %d, not 0", who, k, p->reserved[k]);
}

static void kit_ids_check(const char* who, int n_ids)
{
    if (n_ids < 0 || n_ids > KIT_MAX_IDS) fail(EAGLE_E_INVALID, "%s: %d ids, the limit is %d", who, n_ids, KIT_MAX_IDS);
}

static void kit_empty_model(EagleKitModel* model_out)
{
    if (!model_out) return;
    EagleKitModel m{};
    m.a = m.b = -1; m.flags = EAGLE_KIT_MODEL_SINGLE;
    *model_out = m;
}

// the device memory of a call, n_ids > 0
struct KitBuf {
    Net net;
    unsigned long long* sums; int32_t* used; int32_t* skipped;
    KitArgs a{};
    KitBuf(int n_ids, const EagleKitParams* p, hipStream_t s)
    {
        const size_t n = (size_t)n_ids;
        sums = (unsigned long long*)net.get(n * KIT_BINS * 8);
        used = (int32_t*)net.get(n * 4); skipped = (int32_t*)net.get(n * 4);
        a.sums = sums; a.used = used; a.skipped = skipped; a.n_ids = n_ids; a.min_crops = p->min_crops; a.outlier = p->outlier;
        a.p = (uint32_t*)net.get(n * KIT_BINS * 4); a.vlist = (int32_t*)net.get(n * 4); a.nv = (int32_t*)net.get(4);
        a.D = (uint32_t*)net.get(n * n * 4); a.key = (unsigned long long*)net.get(8);
        a.ids = (EagleKitId*)net.get(n * sizeof(EagleKitId)); a.model = (EagleKitModel*)net.get(sizeof(EagleKitModel));
        HIP_CHECK(hipMemsetAsync(sums, 0, n * KIT_BINS * 8, s));
        HIP_CHECK(hipMemsetAsync(used, 0, n * 4, s));
        HIP_CHECK(hipMemsetAsync(skipped, 0, n * 4, s));
    }
};

// steps 5 to 11 on the sums in m -> the outputs (each may be NULL); the stream is synchronised on return.  ev: NULL, or four events of which ev[2] and
// ev[3] are recorded directly before the first and behind the last of the four launches
static void kit_cluster(EagleHandle* h, KitBuf& m, EagleKitId* ids_out, EagleKitModel* model_out, hipStream_t s, hipEvent_t* ev)
{
    const int n = m.a.n_ids;
    const unsigned g16 = (unsigned)((n + 15) / 16);
    auto run = [&](const char* name, double bytes, const std::function<void()>& fn) {
        if (h) timed_launch(h, name, bytes, s, fn); else fn();
        HIP_CHECK(hipGetLastError());
    };
    KitArgs a = m.a;
    try {
        if (ev) HIP_CHECK(hipEventRecord(ev[2], s));
        run("kit_prep", 420.0 * n, [&] { hipLaunchKernelGGL(kit_prep_kernel, dim3(1), dim3(1024), 0, s, a); });
        run("kit_dist", 4.0 * n * n + 136.0 * n, [&] { hipLaunchKernelGGL(kit_dist_kernel, dim3(g16, g16), dim3(256), 0, s, a); });
        if (n > 1) run("kit_pair", 4.0 * n * n, [&] { hipLaunchKernelGGL(kit_pair_kernel, dim3((unsigned)(n - 1)), dim3(256), 0, s, a); });
        run("kit_assign", 300.0 * n, [&] { hipLaunchKernelGGL(kit_assign_kernel, dim3(1), dim3(1024), 0, s, a); });
        if (ev) HIP_CHECK(hipEventRecord(ev[3], s));
        if (ids_out) HIP_CHECK(hipMemcpyAsync(ids_out, a.ids, (size_t)n * sizeof(EagleKitId), hipMemcpyDeviceToHost, s));
        if (model_out) HIP_CHECK(hipMemcpyAsync(model_out, a.model, sizeof(EagleKitModel), hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
    } catch (...) {
        (void)hipStreamSynchronize(s);
        throw;
    }
    if (h && h->prof) collect_spans(h);
}

static void kit_check(const char* who, const void* bgr, int n_frames, int fh, int fw, const EagleCrop* crops, const int32_t* slots, int n_crops, int n_ids, const EagleKitParams* p)
{
    kit_ids_check(who, n_ids);
    if (n_crops < 0 || n_crops > KIT_MAX_CROPS) fail(EAGLE_E_INVALID, "%s: %d crops, the limit is %d", who, n_crops, KIT_MAX_CROPS);
    kit_params_check(who, p);
    if (n_frames < 0 || fh <= 0 || fw <= 0 || (n_frames > 0 && !bgr)) fail(EAGLE_E_INVALID, "%s: %d frames of %d x %d at %p", who, n_frames, fh, fw, bgr);
    if (n_crops > 0 && (!crops || !slots)) fail(EAGLE_E_INVALID, "%s: %d crops at %p with slots at %p", who, n_crops, (const void*)crops, (const void*)slots);
    for (int i = 0; i < n_crops; ++i)
        if (slots[i] < 0 || slots[i] >= n_ids) fail(EAGLE_E_INVALID, "%s: crop %d: slot %d lies outside 0 .. %d", who, i, slots[i], n_ids - 1);
}

// the whole stage on a clip resident at d_bgr; n_ids > 0
static void kit_device(EagleHandle* h, const uint8_t* d_bgr, int n_frames, int fh, int fw, const EagleCrop* crops, const int32_t* slots, int n_crops, int n_ids,
                       const EagleKitParams* p, EagleKitCrop* crops_out, EagleKitId* ids_out, EagleKitModel* model_out, hipStream_t s, float* times_ms)
{
    KitBuf m(n_ids, p, s);
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    try {
        if (times_ms)
            for (hipEvent_t& e : ev) HIP_CHECK(hipEventCreate(&e));
        if (n_crops > 0) {
            KitHistArgs a{};
            EagleCrop* d_c = (EagleCrop*)m.net.get(sizeof(EagleCrop) * (size_t)n_crops);
            int32_t* d_s = (int32_t*)m.net.get(4 * (size_t)n_crops);
            HIP_CHECK(hipMemcpyAsync(d_c, crops, sizeof(EagleCrop) * (size_t)n_crops, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(d_s, slots, 4 * (size_t)n_crops, hipMemcpyHostToDevice, s));
            a.bgr = d_bgr; a.n_frames = n_frames; a.fh = fh; a.fw = fw; a.crops = d_c; a.slots = d_s; a.n_crops = n_crops; a.min_pixels = p->min_pixels;
            a.recs = crops_out ? (EagleKitCrop*)m.net.get(sizeof(EagleKitCrop) * (size_t)n_crops) : nullptr;
            a.sums = m.sums; a.used = m.used; a.skipped = m.skipped;
            auto fn = [&] { hipLaunchKernelGGL(kit_hist_kernel, dim3((unsigned)((n_crops + 3) / 4)), dim3(256), 0, s, a); };
            if (times_ms) HIP_CHECK(hipEventRecord(ev[0], s));                 // (the scratch is allocated and the crop list enqueued before; the records leave behind ev[1])
            if (h) timed_launch(h, "kit_hist", 1200.0 * n_crops, s, fn); else fn();
            HIP_CHECK(hipGetLastError());
            if (times_ms) HIP_CHECK(hipEventRecord(ev[1], s));
            if (crops_out) HIP_CHECK(hipMemcpyAsync(crops_out, a.recs, sizeof(EagleKitCrop) * (size_t)n_crops, hipMemcpyDeviceToHost, s));
        }
        kit_cluster(h, m, ids_out, model_out, s, times_ms ? ev : nullptr);
        if (times_ms) {
            times_ms[0] = 0.0f;
            if (n_crops > 0) HIP_CHECK(hipEventElapsedTime(&times_ms[0], ev[0], ev[1]));
            HIP_CHECK(hipEventElapsedTime(&times_ms[1], ev[2], ev[3]));
        }
    } catch (...) {
        (void)hipStreamSynchronize(s);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        throw;
    }
    for (hipEvent_t e : ev) if (e) HIP_CHECK(hipEventDestroy(e));
}

}  // namespace eagle

extern "C" {

int eagle_kit_params_default(EagleKitParams* p)
{
    if (!p) return EAGLE_E_INVALID;
    *p = EagleKitParams{};
    p->min_pixels = 32; p->min_crops = 3; p->outlier = 512;
    return EAGLE_OK;
}

int eagle_team_cluster(EagleHandle* h, const void* d_bgr, int n_frames, const EagleCrop* crops, const int32_t* slots, int n_crops, int n_ids, const EagleKitParams* p,
                       EagleKitCrop* crops_out, EagleKitId* ids_out, EagleKitModel* model_out)
{
    API_BEGIN_H(h)
    kit_check("eagle_team_cluster", d_bgr, n_frames, h->cfg.frame_h, h->cfg.frame_w, crops, slots, n_crops, n_ids, p);
    if (n_ids == 0) { kit_empty_model(model_out); return EAGLE_OK; }
    HIP_CHECK(hipSetDevice(h->cfg.device));
    kit_device(h, (const uint8_t*)d_bgr, n_frames, h->cfg.frame_h, h->cfg.frame_w, crops, slots, n_crops, n_ids, p, crops_out, ids_out, model_out, h->s_main, nullptr);
    API_END(h)
}

int eagle_op_team_cluster(int device, const uint8_t* bgr, int n, int h, int w, const EagleCrop* crops, const int32_t* slots, int n_crops, int n_ids, const EagleKitParams* p,
                          EagleKitCrop* crops_out, EagleKitId* ids_out, EagleKitModel* model_out, float* times_ms)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    kit_check("eagle_op_team_cluster", bgr, n, h, w, crops, slots, n_crops, n_ids, p);
    if (n_ids == 0) { kit_empty_model(model_out); return EAGLE_OK; }
    HIP_CHECK(hipSetDevice(device));
    Net clip;
    const uint8_t* d = n > 0 ? (const uint8_t*)clip.upload(bgr, (size_t)n * h * w * 3) : nullptr;
    kit_device(nullptr, d, n, h, w, crops, slots, n_crops, n_ids, p, crops_out, ids_out, model_out, nullptr, times_ms);
    API_END(hh)
}

int eagle_op_team_cluster_ids(int device, const int64_t* sums, const int32_t* used, int n_ids, const EagleKitParams* p, EagleKitId* ids_out, EagleKitModel* model_out,
                              float* times_ms)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_team_cluster_ids";
    kit_ids_check(who, n_ids);
    kit_params_check(who, p);
    if (n_ids > 0 && (!sums || !used)) fail(EAGLE_E_INVALID, "%s: %d ids with sums at %p and used at %p", who, n_ids, (const void*)sums, (const void*)used);
    long long crops = 0;
    for (int i = 0; i < n_ids; ++i) {
        if (used[i] < 0 || used[i] > KIT_MAX_CROPS) fail(EAGLE_E_INVALID, "%s: id %d: used %d lies outside 0 .. %d", who, i, used[i], KIT_MAX_CROPS);
        long long T = 0;
        for (int b = 0; b < KIT_BINS; ++b) {
            const long long v = sums[(size_t)i * KIT_BINS + b];
            if (v < 0 || v > KIT_MAX_SUM) fail(EAGLE_E_INVALID, "%s: id %d, bin %d: sum %lld lies outside 0 .. %lld", who, i, b, v, KIT_MAX_SUM);
            T += v;
        }
        if (used[i] > 0 && T == 0) fail(EAGLE_E_INVALID, "%s: id %d has %d crops and no colour: its sums are all 0", who, i, used[i]);
        crops += used[i];
    }
    if (crops > KIT_MAX_CROPS) fail(EAGLE_E_INVALID, "%s: the ids have %lld crops in all, the limit is %d (the key cost << 20 | rank holds 64 bits up to there)", who, crops, KIT_MAX_CROPS);
    if (n_ids == 0) { kit_empty_model(model_out); return EAGLE_OK; }
    HIP_CHECK(hipSetDevice(device));
    KitBuf m(n_ids, p, nullptr);
    HIP_CHECK(hipMemcpyAsync(m.sums, sums, (size_t)n_ids * KIT_BINS * 8, hipMemcpyHostToDevice, nullptr));
    HIP_CHECK(hipMemcpyAsync(m.used, used, (size_t)n_ids * 4, hipMemcpyHostToDevice, nullptr));
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    try {
        if (times_ms)
            for (int k = 2; k < 4; ++k) HIP_CHECK(hipEventCreate(&ev[k]));
        kit_cluster(nullptr, m, ids_out, model_out, nullptr, times_ms ? ev : nullptr);
        if (times_ms) { times_ms[0] = 0.0f; HIP_CHECK(hipEventElapsedTime(&times_ms[1], ev[2], ev[3])); }
    } catch (...) {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        throw;
    }
    for (hipEvent_t e : ev) if (e) HIP_CHECK(hipEventDestroy(e));
    API_END(hh)
}

}  // extern "C"
