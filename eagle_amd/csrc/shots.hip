// K31 — shots: a clip of dense BGR frames resident in HBM -> per frame a colour signature of integer histograms, per frame and lag a score, and from the
// scores the flashes, hard cuts, gradual transitions and the list of shots (include/eagle.h, eagle_shots_device_frames / eagle_shots_frames /
// eagle_op_shots; tests/shots_ref.py is the written definition of every bit).  Integers behind the pixel read: counts are added with integer atomics and
// the two divisions are in 64 bits, so no result depends on an order.
//
//   shot_signature_kernel  the hot one, one read of the clip.  A workgroup of four waves takes a band of up to SH_ROWS rows of one frame that lies inside
//                          one tile row (the up to 3 rows below the tiles are a band of their own), so it touches 512 + 4 x 64 counters.  The band is one
//                          run of bytes: up to 15 head pixels bring it to a 16-byte boundary, then every lane takes groups of 16 pixels as three 16-byte
//                          loads, and up to 15 tail pixels follow; head and tail are read byte by byte.  On a pitch picture most pixels fall into one
//                          bin, and 64 lanes adding to one LDS address serialise.  So a lane folds its pixel stream by run length in registers, the colour
//                          bin and the (tile column, tile bin) key apart: it issues an LDS atomic only when a key changes, which on one colour is once per
//                          tile column it enters instead of twice per pixel.  Each wave adds into its OWN counters in LDS; behind a barrier the workgroup
//                          sums its four sets and issues one global u32 atomic per non-zero counter (the signatures are zeroed in front of the launch).
//   shot_distance_kernel   one wave per frame and lag (1, 2, W): the 512-bin and the 16 x 64-bin absolute differences by wave reduction; lane t < 16 keeps
//                          tile t's distance and ranks it among the 16 (only the values matter, so ties are harmless); the 8 smallest are summed.
//
// The decisions and the shot list work on n x 7 integers and run on the host (shot_decide), as post.hip's column discovery does.
#include "runtime.h"

namespace eagle {

static constexpr int SH_SIG = EAGLE_SHOT_SIGNATURE;
static constexpr int SH_ROWS = 16;                     // rows per band
static constexpr int SH_CNT = 512 + 4 * 64;            // a band's counters: the colour bins and the four tiles of its tile row
static constexpr int64_t SH_STAGING = 64 << 20;
static constexpr int SH_MAX_BLOCKS = 1 << 30;
typedef unsigned long long sh_u64;
static_assert(sizeof(EagleShotParams) == 32 && sizeof(EagleShotFrame) == 32 && sizeof(EagleShot) == 32, "include/eagle.h states these sizes");
static_assert(SH_SIG == 512 + 16 * 64 + 1, "hist, tiles, grass");

struct ShArgs {
    const uint8_t* bgr;          // [n][h][w][3]
    uint32_t* sig;               // [n][SH_SIG], zeroed
    int h, w, th, tw;
    int bpt, nbands;             // bands per tile row; bands per frame (4 bpt, + 1 with rows below the tiles)
    int f0;                      // blockIdx.x counts the bands from frame f0
};

__device__ __forceinline__ uint32_t sh_wave_sum(uint32_t v)
{
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// one lane's folded pixel stream: the run of the colour bin and the run of the tile key, flushed into the wave's counters when the key changes
struct ShRun {
    int hk = 0, tk = 512;
    uint32_t hn = 0, tn = 0, grass = 0;
    __device__ __forceinline__ void pixel(uint32_t* C, uint32_t b, uint32_t g, uint32_t r, int x, bool tiled, int tw)
    {
        const int k5 = (int)(((b >> 5) << 6) | ((g >> 5) << 3) | (r >> 5));
        if (k5 != hk) {
            if (hn) atomicAdd(&C[hk], hn);
            hk = k5; hn = 0;
        }
        ++hn;
        if (tiled && x < 4 * tw) {
            const int tx = (x >= tw ? 1 : 0) + (x >= 2 * tw ? 1 : 0) + (x >= 3 * tw ? 1 : 0);
            const int k6 = 512 + tx * 64 + (int)(((b >> 6) << 4) | ((g >> 6) << 2) | (r >> 6));
            if (k6 != tk) {
                if (tn) atomicAdd(&C[tk], tn);
                tk = k6; tn = 0;
            }
            ++tn;
        }
        grass += (g >= 48 && (int)g - (int)max(r, b) >= 16) ? 1u : 0u;
    }
    __device__ __forceinline__ void flush(uint32_t* C)
    {
        if (hn) atomicAdd(&C[hk], hn);
        if (tn) atomicAdd(&C[tk], tn);
    }
};

__global__ __launch_bounds__(256) void shot_signature_kernel(ShArgs a)
{
    __shared__ uint32_t cnt[4][SH_CNT];
    __shared__ uint32_t gr[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int f = a.f0 + (int)(blockIdx.x / (unsigned)a.nbands), band = (int)(blockIdx.x % (unsigned)a.nbands);
    const int ty = band / a.bpt;                                        // 4: the rows below the tiles
    const bool tiled = ty < 4;
    const int r0 = tiled ? ty * a.th + (band - ty * a.bpt) * SH_ROWS : 4 * a.th;
    const int r1 = tiled ? min(r0 + SH_ROWS, (ty + 1) * a.th) : a.h;      // (r0 < r1 <= h by the launch: bpt = ceil(th / SH_ROWS))
    const int NP = (r1 - r0) * a.w;                                     // the band's pixels, one run of 3 NP bytes
    const uint8_t* base = a.bgr + ((size_t)f * a.h + r0) * (size_t)a.w * 3;
    const int head = min(NP, (int)(((16 - ((uintptr_t)base & 15)) * 11) & 15));       // 3 * 11 = 1 (mod 16): base + 3 head is a 16-byte boundary
    const int G = (NP - head) >> 4, tail0 = head + (G << 4);
    for (int i = tid; i < 4 * SH_CNT; i += 256) (&cnt[0][0])[i] = 0;
    __syncthreads();
    uint32_t* C = cnt[wave];
    ShRun run;
    if (tid < head) {
        const uint8_t* p = base + 3 * tid;
        run.pixel(C, p[0], p[1], p[2], tid % a.w, tiled, a.tw);
    }
    const uint4* body = (const uint4*)(base + 3 * head);
    for (int g = tid; g < G; g += 256) {
        const uint4 q0 = body[3 * g], q1 = body[3 * g + 1], q2 = body[3 * g + 2];
        const uint32_t v[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        int x = (head + (g << 4)) % a.w;
        #pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t b = (v[(3 * j) >> 2] >> (((3 * j) & 3) * 8)) & 255u;
            const uint32_t gg = (v[(3 * j + 1) >> 2] >> (((3 * j + 1) & 3) * 8)) & 255u;
            const uint32_t r = (v[(3 * j + 2) >> 2] >> (((3 * j + 2) & 3) * 8)) & 255u;
            run.pixel(C, b, gg, r, x, tiled, a.tw);
            x = x + 1 == a.w ? 0 : x + 1;
        }
    }
    if (tail0 + tid < NP) {
        const uint8_t* p = base + 3 * (size_t)(tail0 + tid);
        run.pixel(C, p[0], p[1], p[2], (tail0 + tid) % a.w, tiled, a.tw);
    }
    run.flush(C);
    const uint32_t wg = sh_wave_sum(run.grass);
    if (lane == 0) gr[wave] = wg;
    __syncthreads();
    uint32_t* S = a.sig + (size_t)f * SH_SIG;
    for (int i = tid; i < SH_CNT; i += 256) {
        const uint32_t v = cnt[0][i] + cnt[1][i] + cnt[2][i] + cnt[3][i];
        if (v && (i < 512 || tiled)) atomicAdd(&S[i < 512 ? i : 512 + ty * 256 + (i - 512)], v);      // (a band below the tiles has no tile counts)
    }
    if (tid == 0) {
        const uint32_t v = gr[0] + gr[1] + gr[2] + gr[3];
        if (v) atomicAdd(&S[1536], v);
    }
}

// out [n][8]: {sg, st} of the lags 1, 2, W, then grass, 0
__global__ __launch_bounds__(256) void shot_distance_kernel(const uint32_t* sig, int n, int W, sh_u64 P2, sh_u64 A16, uint32_t* out)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long idx = (long long)blockIdx.x * 4 + wave;
    if (idx >= 3ll * n) return;                                         // (uniform over the wave; the kernel has no workgroup barrier)
    const int f = (int)(idx / 3), k = (int)(idx % 3);
    const int lag = k == 0 ? 1 : k == 1 ? 2 : W;
    uint32_t* o = out + (size_t)f * 8;
    const uint32_t* b = sig + (size_t)f * SH_SIG;
    if (k == 0 && lane == 0) { o[6] = b[1536]; o[7] = 0; }
    if (f < lag) {
        if (lane == 0) { o[2 * k] = 0; o[2 * k + 1] = 0; }
        return;
    }
    const uint32_t* a = sig + (size_t)(f - lag) * SH_SIG;
    uint32_t s = 0;
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t x = a[j * 64 + lane], y = b[j * 64 + lane];
        s += x > y ? x - y : y - x;
    }
    s = sh_wave_sum(s);                                                 // <= 2 P <= 2^31
    uint32_t mine = 0;
    #pragma unroll
    for (int t = 0; t < 16; ++t) {
        const uint32_t x = a[512 + t * 64 + lane], y = b[512 + t * 64 + lane];
        const uint32_t v = sh_wave_sum(x > y ? x - y : y - x);
        mine = lane == t ? v : mine;
    }
    int rank = 0;
    #pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t ot = __shfl(mine, j, 64);
        rank += (ot < mine || (ot == mine && j < lane)) ? 1 : 0;
    }
    const uint32_t u = sh_wave_sum(lane < 16 && rank < 8 ? mine : 0u);      // <= 16 A
    if (lane == 0) {
        o[2 * k] = (uint32_t)((65536ull * s) / P2);
        o[2 * k + 1] = (uint32_t)((65536ull * u) / A16);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
static void shot_check(const char* who, const void* frames, int n, int h, int w, const EagleShotParams* p, const EagleShotFrame* frames_out, int cap, const int* n_shots)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the shot parameters are NULL", who);
    if (!n_shots) fail(EAGLE_E_INVALID, "%s: n_shots is NULL", who);
    if (n < 0) fail(EAGLE_E_INVALID, "%s: n %d is negative", who, n);
    if (cap < 0) fail(EAGLE_E_INVALID, "%s: cap %d is negative", who, cap);
    if (h < 4 || w < 4) fail(EAGLE_E_INVALID, "%s: frames of %d x %d are below 4 x 4", who, h, w);
    if ((int64_t)h * w > (1 << 30)) fail(EAGLE_E_INVALID, "%s: frames of %d x %d have more than 2^30 pixels", who, h, w);
    if (p->cut < 0 || p->cut > 65536) fail(EAGLE_E_INVALID, "%s: cut %d lies outside 0 .. 65536", who, p->cut);
    if (p->low < 0 || p->low > 65536) fail(EAGLE_E_INVALID, "%s: low %d lies outside 0 .. 65536", who, p->low);
    if (p->grass_thr < 0 || p->grass_thr > 65536) fail(EAGLE_E_INVALID, "%s: grass_thr %d lies outside 0 .. 65536", who, p->grass_thr);
    if (p->low > p->cut) fail(EAGLE_E_INVALID, "%s: low %d is above cut %d", who, p->low, p->cut);
    if (p->window < 2) fail(EAGLE_E_INVALID, "%s: window %d must be at least 2", who, p->window);
    if (p->min_len < 1) fail(EAGLE_E_INVALID, "%s: min_len %d must be at least 1", who, p->min_len);
    for (int k = 0; k < 3; ++k)
        if (p->reserved[k]) fail(EAGLE_E_INVALID, "%s: reserved word %d of the shot parameters is %d, not 0", who, k, p->reserved[k]);
    if (n > 0 && !frames) fail(EAGLE_E_INVALID, "%s: the frames are NULL", who);
    if (n > 0 && !frames_out) fail(EAGLE_E_INVALID, "%s: frames_out is NULL", who);
}

static ShArgs shot_args(int h, int w)
{
    ShArgs a{};
    a.h = h; a.w = w; a.th = h / 4; a.tw = w / 4;
    a.bpt = (a.th + SH_ROWS - 1) / SH_ROWS;
    a.nbands = 4 * a.bpt + (h > 4 * a.th ? 1 : 0);
    return a;
}

// The signatures of `count` frames at d_bgr into sig (zeroed by the caller) on s; enqueued, not awaited
static void shot_signatures(EagleHandle* hd, const uint8_t* d_bgr, int count, int h, int w, uint32_t* sig, hipStream_t s)
{
    ShArgs a = shot_args(h, w);
    a.bgr = d_bgr; a.sig = sig;
    const int per = std::max(1, SH_MAX_BLOCKS / a.nbands);
    auto fn = [&] {
        for (int f0 = 0; f0 < count; f0 += per) {
            ShArgs b = a;
            b.f0 = f0;
            hipLaunchKernelGGL(shot_signature_kernel, dim3((unsigned)(std::min(per, count - f0) * a.nbands)), dim3(256), 0, s, b);
            HIP_CHECK(hipGetLastError());
        }
    };
    if (hd) timed_launch(hd, "shot_signature", (double)count * h * w * 3.0, s, fn); else fn();
}

// sig [n][SH_SIG] -> dist [n][8] on s; enqueued, not awaited
static void shot_distances(EagleHandle* hd, const uint32_t* sig, int n, int h, int w, int W, uint32_t* dist, hipStream_t s)
{
    const sh_u64 P2 = 2ull * (sh_u64)h * (sh_u64)w, A16 = 16ull * (sh_u64)(h / 4) * (sh_u64)(w / 4);
    auto fn = [&] {
        hipLaunchKernelGGL(shot_distance_kernel, dim3((unsigned)((3ll * n + 3) / 4)), dim3(256), 0, s, sig, n, W, P2, A16, dist);
        HIP_CHECK(hipGetLastError());
    };
    if (hd) timed_launch(hd, "shot_distance", (double)n * (3.0 * 2.0 * SH_SIG * 4.0 + 32.0), s, fn); else fn();
}

// the decisions: pure functions of the n x 7 integers (tests/shots_ref.py, decide)
static void shot_decide(const uint32_t* dist, int n, sh_u64 P, const EagleShotParams& p, std::vector<EagleShotFrame>& fr, std::vector<EagleShot>& shots)
{
    fr.assign((size_t)n, EagleShotFrame{});
    shots.clear();
    if (n == 0) return;
    const long long W = p.window;
    for (int i = 0; i < n; ++i) {
        const uint32_t* d = dist + (size_t)i * 8;
        EagleShotFrame& o = fr[i];
        o.sg = (int32_t)d[0]; o.st = (int32_t)d[1];
        o.d1 = (int32_t)std::max(d[0], d[1]); o.d2 = (int32_t)std::max(d[2], d[3]); o.dW = (int32_t)std::max(d[4], d[5]);
        o.grass = d[6];
    }
    std::vector<char> flash((size_t)n, 0), hard((size_t)n, 0), elig((size_t)n, 0), gend((size_t)n, 0), tstart((size_t)n, 0);
    std::vector<int> hsum((size_t)n + 1, 0);                               // hard cuts in front of frame i
    for (int i = 1; i < n; ++i) flash[i] = fr[i].d1 >= p.cut && i + 1 < n && fr[i + 1].d2 < p.low;
    for (int i = 1; i < n; ++i) hard[i] = fr[i].d1 >= p.cut && !flash[i] && !flash[i - 1];
    for (int i = 0; i < n; ++i) hsum[i + 1] = hsum[i] + hard[i];
    for (long long i = W; i < n; ++i)
        elig[i] = fr[i].dW >= p.cut && hsum[i + 1] - hsum[i - W + 1] == 0 && !flash[i] && !flash[i - W];
    for (long long i = W; i < n; ++i) {
        if (!elig[i]) continue;
        bool first_max = true;
        for (long long j = i - W + 1; j < i && first_max; ++j) first_max = !(elig[j] && fr[j].dW >= fr[i].dW);
        for (long long j = i + 1; j < std::min<long long>(i + W, n) && first_max; ++j) first_max = !(elig[j] && fr[j].dW > fr[i].dW);
        if (!first_max) continue;
        gend[i] = 1; tstart[i - W + 1] = 1;
        for (long long j = i - W + 1; j < i; ++j) fr[j].flags |= EAGLE_SHOT_FRAME_IN_TRANSITION;
    }
    for (int i = 0; i < n; ++i) {
        fr[i].flags |= (flash[i] ? EAGLE_SHOT_FRAME_FLASH : 0) | (hard[i] ? EAGLE_SHOT_FRAME_HARD : 0) | (gend[i] ? EAGLE_SHOT_FRAME_GRADUAL_END : 0);
        if (i == 0 || hard[i] || gend[i] || tstart[i]) {
            EagleShot s{};
            s.first = i;
            s.kind = tstart[i] ? EAGLE_SHOT_TRANSITION : gend[i] ? EAGLE_SHOT_AFTER_TRANSITION : hard[i] ? EAGLE_SHOT_AFTER_CUT : EAGLE_SHOT_START;
            shots.push_back(s);
        }
        EagleShot& s = shots.back();
        s.count += 1; s.grass_sum += fr[i].grass;
    }
    for (EagleShot& s : shots) {
        const bool pitch = s.kind != EAGLE_SHOT_TRANSITION && (unsigned __int128)s.grass_sum * 65536u >= (unsigned __int128)((sh_u64)p.grass_thr * P) * (sh_u64)s.count;
        const bool shrt = s.count < p.min_len;
        s.flags = (pitch ? EAGLE_SHOT_PITCH : 0) | (shrt ? EAGLE_SHOT_SHORT : 0) | (pitch && !shrt ? EAGLE_SHOT_USABLE : 0);
    }
}

// dist (device, complete) -> the caller's outputs; the refusal of a list beyond cap leaves them alone but for the count
static void shot_finish(const char* who, const uint32_t* d_dist, int n, int h, int w, const EagleShotParams* p, EagleShotFrame* frames_out, EagleShot* shots_out, int cap,
                        int* n_shots)
{
    std::vector<uint32_t> dist((size_t)n * 8);
    HIP_CHECK(hipMemcpy(dist.data(), d_dist, dist.size() * 4, hipMemcpyDeviceToHost));
    std::vector<EagleShotFrame> fr;
    std::vector<EagleShot> shots;
    shot_decide(dist.data(), n, (sh_u64)h * (sh_u64)w, *p, fr, shots);
    if (shots.size() > (size_t)cap || (!shots_out && !shots.empty())) {
        *n_shots = (int)shots.size();
        fail(EAGLE_E_INVALID, "%s: the clip has %zu shots, the list takes %d", who, shots.size(), shots_out ? cap : 0);
    }
    memcpy(frames_out, fr.data(), fr.size() * sizeof(EagleShotFrame));
    if (!shots.empty()) memcpy(shots_out, shots.data(), shots.size() * sizeof(EagleShot));
    *n_shots = (int)shots.size();
}

struct ShBuf {                  // the device memory of a call
    uint32_t* sig = nullptr; uint32_t* dist = nullptr; uint8_t* stage = nullptr;
    ~ShBuf() { if (sig) (void)hipFree(sig); if (dist) (void)hipFree(dist); if (stage) (void)hipFree(stage); }
    void alloc(int n)
    {
        HIP_CHECK(hipMalloc((void**)&sig, (size_t)n * SH_SIG * 4));
        HIP_CHECK(hipMalloc((void**)&dist, (size_t)n * 8 * 4));
    }
};

// n > 0 frames resident at d_bgr -> outputs
static void shot_device(const char* who, EagleHandle* hd, const uint8_t* d_bgr, int n, int h, int w, const EagleShotParams* p, EagleShotFrame* frames_out,
                        EagleShot* shots_out, int cap, int* n_shots, uint32_t* signatures_out, hipStream_t s)
{
    ShBuf m;
    m.alloc(n);
    try {
        HIP_CHECK(hipMemsetAsync(m.sig, 0, (size_t)n * SH_SIG * 4, s));
        shot_signatures(hd, d_bgr, n, h, w, m.sig, s);
        shot_distances(hd, m.sig, n, h, w, p->window, m.dist, s);
        HIP_CHECK(hipStreamSynchronize(s));
    } catch (...) {
        (void)hipStreamSynchronize(s);
        throw;
    }
    if (hd && hd->prof) collect_spans(hd);
    shot_finish(who, m.dist, n, h, w, p, frames_out, shots_out, cap, n_shots);
    if (signatures_out) HIP_CHECK(hipMemcpy(signatures_out, m.sig, (size_t)n * SH_SIG * 4, hipMemcpyDeviceToHost));
}

}  // namespace eagle

extern "C" {

int eagle_shots_device_frames(EagleHandle* h, const uint8_t* d_bgr, int n, const EagleShotParams* p, EagleShotFrame* frames_out, EagleShot* shots_out, int cap, int* n_shots)
{
    API_BEGIN_H(h)
    shot_check("eagle_shots_device_frames", d_bgr, n, h->cfg.frame_h, h->cfg.frame_w, p, frames_out, cap, n_shots);
    if (n == 0) { *n_shots = 0; return EAGLE_OK; }
    HIP_CHECK(hipSetDevice(h->cfg.device));
    shot_device("eagle_shots_device_frames", h, d_bgr, n, h->cfg.frame_h, h->cfg.frame_w, p, frames_out, shots_out, cap, n_shots, nullptr, h->s_main);
    API_END(h)
}

int eagle_shots_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t row_stride, int64_t frame_stride, int64_t max_staging_bytes, const EagleShotParams* p,
                       EagleShotFrame* frames_out, EagleShot* shots_out, int cap, int* n_shots)
{
    API_BEGIN_H(h)
    const char* who = "eagle_shots_frames";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    shot_check(who, bgr, n, fh, fw, p, frames_out, cap, n_shots);
    const int64_t fb = (int64_t)fh * fw * 3;
    if (row_stride == 0) row_stride = 3 * (int64_t)fw;
    if (frame_stride == 0) frame_stride = (int64_t)fh * row_stride;
    if (row_stride < 3 * (int64_t)fw) fail(EAGLE_E_INVALID, "%s: row_stride %lld is below a row's %lld bytes", who, (long long)row_stride, 3ll * fw);
    if (frame_stride < (fh - 1) * row_stride + 3 * (int64_t)fw)
        fail(EAGLE_E_INVALID, "%s: frame_stride %lld is below a frame's extent of %lld bytes", who, (long long)frame_stride, (long long)((fh - 1) * row_stride + 3ll * fw));
    if (max_staging_bytes < 0) fail(EAGLE_E_INVALID, "%s: max_staging_bytes %lld is negative", who, (long long)max_staging_bytes);
    if (n == 0) { *n_shots = 0; return EAGLE_OK; }
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const int pass = (int)std::max<int64_t>(1, std::min<int64_t>(n, (max_staging_bytes ? max_staging_bytes : SH_STAGING) / fb));
    hipStream_t s = h->s_main;
    ShBuf m;
    m.alloc(n);
    HIP_CHECK(hipMalloc((void**)&m.stage, (size_t)pass * fb));
    try {
        HIP_CHECK(hipMemsetAsync(m.sig, 0, (size_t)n * SH_SIG * 4, s));
        for (int i = 0; i < n; i += pass) {
            const int k = std::min(pass, n - i);
            const uint8_t* src = bgr + (int64_t)i * frame_stride;
            if (row_stride == 3 * (int64_t)fw && frame_stride == fb) {
                HIP_CHECK(hipMemcpyAsync(m.stage, src, (size_t)k * fb, hipMemcpyHostToDevice, s));
            } else {
                for (int j = 0; j < k; ++j)
                    HIP_CHECK(hipMemcpy2DAsync(m.stage + (int64_t)j * fb, 3 * (size_t)fw, src + (int64_t)j * frame_stride, (size_t)row_stride, 3 * (size_t)fw, (size_t)fh,
                                               hipMemcpyHostToDevice, s));
            }
            shot_signatures(h, m.stage, k, fh, fw, m.sig + (size_t)i * SH_SIG, s);
            HIP_CHECK(hipStreamSynchronize(s));                          // (the next pass reuses the staging)
            if (h->prof) collect_spans(h);
        }
        shot_distances(h, m.sig, n, fh, fw, p->window, m.dist, s);
        HIP_CHECK(hipStreamSynchronize(s));
        if (h->prof) collect_spans(h);
    } catch (...) {
        (void)hipStreamSynchronize(s);
        throw;
    }
    shot_finish(who, m.dist, n, fh, fw, p, frames_out, shots_out, cap, n_shots);
    API_END(h)
}

int eagle_op_shots(int device, const uint8_t* bgr, int n, int h, int w, const EagleShotParams* p, EagleShotFrame* frames_out, EagleShot* shots_out, int cap, int* n_shots,
                   uint32_t* signatures_out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    shot_check("eagle_op_shots", bgr, n, h, w, p, frames_out, cap, n_shots);
    if (n == 0) { *n_shots = 0; return EAGLE_OK; }
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const uint8_t* d = (const uint8_t*)net.upload(bgr, (size_t)n * h * w * 3);
    shot_device("eagle_op_shots", nullptr, d, n, h, w, p, frames_out, shots_out, cap, n_shots, signatures_out, nullptr);
    API_END(hh)
}

}  // extern "C"
