// K39 — line registration: dense BGR frames resident in HBM + the homography of each -> the homographies moved until the frames' painted-line pixels lie
// on the pitch model's centre lines (include/eagle.h, eagle_linefit_* / eagle_op_linefit; tests/linefit_ref.py is the written definition of every bit).
// The projective map and the solve are float64 with every product, sum and quotient a single IEEE operation (the file is built with -ffp-contract=off,
// the division is the compiler's); everything between floor() and the solve is integers, and all accumulation across pixels is integer atomics, so no
// result depends on an order and two runs give the same bytes.
//
//   linefit_mask_kernel        a thread per pixel, 256 neighbours of a row per workgroup: the rule's five reads per pixel fall on cached neighbours, a
//                              wave's ballot is two words of the frame's bit mask, its popcount one u32 atomic on the frame's n_line.  The frame's boxes go
//                              through LDS once per workgroup (only with boxes).
//   linefit_accumulate_kernel  a thread per mask word walks its set bits: POINT, MATCH against the 20 primitives (constant memory), ROW, and the 46 sums
//                              of N, b, cnt, se2 in its registers; a wave's lanes are summed by a butterfly and one lane adds them with 46 u64 atomics
//                              (csrc/linefit_accumulate.inc, shared with the rate tool, which also builds the form with an atomic per inlier and sum).  The inliers per primitive are LDS
//                              atomics flushed once per workgroup.
//   linefit_solve_kernel       a thread per frame: the round's ladder, Gaussian elimination, T (D (T^-1 M)) into the frame's state.
//   linefit_decide_kernel      a thread per frame: SHIFT, the status, the record and the accepted matrix.
// A call enqueues mask, then (accumulate, solve) per round, two accumulates at radius_min (before / after) and decide on one stream, with no host
// synchronisation in between.
#include "runtime.h"
#include "linefit_accumulate.inc"

namespace eagle {

static constexpr int64_t LF_STAGING = 64 << 20;
static constexpr int LF_PASS = 65535;                      // gridDim.y / .z limit: frames per chunk
static constexpr int LF_MAX_DIM = 16384;
static constexpr int64_t LF_MAX_PIXELS = 1 << 28;
static constexpr int LF_MAX_ROUNDS = 16;
static_assert(sizeof(EagleLineFitParams) == 88 && sizeof(EagleLineFitFrame) == 56, "include/eagle.h states these sizes");
// |J| < 2^17, |e| <= 2^13 (radius <= 8 m), at most 2^28 pixels: every sum stays below 2^62
static_assert(LF_MAX_PIXELS * ((int64_t)1 << 34) == (int64_t)1 << 62 && (int64_t)LF_MAX_DIM * LF_MAX_DIM <= LF_MAX_PIXELS, "the sums fit 63 bits");

__device__ __forceinline__ bool lf_grass(const uint8_t* p) { return p[1] >= 48 && (int)p[1] - max((int)p[2], (int)p[0]) >= 16; }
__device__ __forceinline__ int lf_luma(const uint8_t* p) { return (int)p[0] + 2 * (int)p[1] + (int)p[2]; }

__global__ __launch_bounds__(256) void linefit_mask_kernel(LfArgs a)
{
    __shared__ float4 s_box[EAGLE_MAX_DET];
    const int f = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    const uint8_t* fr = a.bgr + (int64_t)f * a.fstride;
    int nb = 0;
    if (a.boff) {                                           // (uniform)
        const int b0 = a.boff[f];
        nb = a.boff[f + 1] - b0;                            // at most EAGLE_MAX_DET, checked on the host
        for (int i = threadIdx.x; i < nb; i += 256) s_box[i] = a.boxes[b0 + i];
        __syncthreads();
    }
    bool hit = false;
    const int k = a.k;
    if (x >= k && x <= a.w - 1 - k && y >= k && y <= a.h - 1 - k) {
        const uint8_t* p = fr + ((size_t)y * a.w + x) * 3;
        const int Y = lf_luma(p);
        const uint8_t* l = p - 3 * k;
        const uint8_t* r = p + 3 * k;
        const uint8_t* u = p - (size_t)3 * k * a.w;
        const uint8_t* d = p + (size_t)3 * k * a.w;
        hit = (lf_grass(l) && lf_grass(r) && Y - max(lf_luma(l), lf_luma(r)) >= a.tau) || (lf_grass(u) && lf_grass(d) && Y - max(lf_luma(u), lf_luma(d)) >= a.tau);
        if (hit && nb) {
            const double px = (double)x, py = (double)y;
            for (int i = 0; i < nb; ++i) {
                const float4 b = s_box[i];
                if ((double)b.x - a.pad <= px && px <= (double)b.z + a.pad && (double)b.y - a.pad <= py && py <= (double)b.w + a.pad) hit = false;
            }
        }
    }
    const lf_u64 bal = __ballot(hit);
    const int lane = threadIdx.x & 63, x0 = blockIdx.x * 256 + (threadIdx.x & ~63);
    uint32_t* row = a.mask + ((size_t)f * a.h + y) * a.wpr;
    const int wd = (x0 >> 5) + (lane >> 5);
    if ((lane & 31) == 0 && wd < a.wpr) row[wd] = (uint32_t)(bal >> (lane & 32));
    if (lane == 0 && bal) atomicAdd(a.nline + f, (uint32_t)__popcll(bal));
}

// 3 x 3 product, every entry ((r0 c0) + (r1 c1)) + (r2 c2)
__host__ __device__ inline void lf_matmul3(const double* A, const double* B, double* C)
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[3 * r + c] = ((A[3 * r] * B[c]) + (A[3 * r + 1] * B[3 + c])) + (A[3 * r + 2] * B[6 + c]);
}

// SOLVE over the unknowns idx[0 .. m): false on a failed pivot
__device__ static bool lf_solve(const lf_u64* S, const int* idx, int m, double* x)
{
    double A[8][8], rhs[8];
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < m; ++j) {
            const int lo = min(idx[i], idx[j]), hi = max(idx[i], idx[j]);
            A[i][j] = (double)(int64_t)S[lo * 8 - lo * (lo - 1) / 2 + (hi - lo)];
        }
        rhs[i] = -(double)(int64_t)S[36 + idx[i]];
    }
    double dmax = A[0][0];
    for (int i = 1; i < m; ++i) dmax = A[i][i] > dmax ? A[i][i] : dmax;
    for (int c = 0; c < m; ++c) {
        int piv = c;
        for (int r = c + 1; r < m; ++r)
            if (fabs(A[r][c]) > fabs(A[piv][c])) piv = r;
        if (!(fabs(A[piv][c]) >= 1e-9 * dmax) || A[piv][c] == 0.0) return false;
        for (int j = 0; j < m; ++j) { const double t = A[c][j]; A[c][j] = A[piv][j]; A[piv][j] = t; }
        { const double t = rhs[c]; rhs[c] = rhs[piv]; rhs[piv] = t; }
        for (int r = c + 1; r < m; ++r) {
            const double fct = A[r][c] / A[c][c];
            for (int j = c + 1; j < m; ++j) A[r][j] = A[r][j] - fct * A[c][j];
            rhs[r] = rhs[r] - fct * rhs[c];
        }
    }
    for (int c = m - 1; c >= 0; --c) {
        double s = rhs[c];
        for (int j = c + 1; j < m; ++j) s = s - A[c][j] * x[j];
        x[c] = s / A[c][c];
    }
    return true;
}

__global__ __launch_bounds__(64) void linefit_solve_kernel(LfArgs a)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= a.n || !a.tab[f].ok) return;
    const lf_u64* S = a.sums + ((size_t)a.slot * a.n + f) * LF_NSUM;
    LfState& st = a.st[f];
    int nV = 0, nH = 0, nA = 0;
    for (int i = 0; i < LF_NSEG; ++i)
        if (S[46 + i] >= (lf_u64)a.min_per_line) { if (c_seg[i].orient == 0) ++nV; else ++nH; }
    for (int j = 0; j < LF_NARC; ++j)
        if (S[46 + LF_NSEG + j] >= (lf_u64)a.min_per_line) ++nA;
    const int nT = nV + nH + nA, cX = nV + nA, cY = nH + nA;
    const double T[9] = {64.0, 0.0, 52.5, 0.0, 64.0, 34.0, 0.0, 0.0, 1.0};
    const double TI[9] = {0.015625, 0.0, -0.8203125, 0.0, 0.015625, -0.53125, 0.0, 0.0, 1.0};
    int fall = st.fall, rung = a.model;
    while (rung > 0) {
        const int bit = 3 * (rung - 1);
        int idx[8], m = 0;
        bool ok;
        if (rung == 3) { ok = nT >= 4 && cX >= 2 && cY >= 2; m = 8; for (int i = 0; i < 8; ++i) idx[i] = i; }
        else if (rung == 2) { ok = nT >= 3 && cX >= 1 && cY >= 1; m = 6; for (int i = 0; i < 6; ++i) idx[i] = i; }
        else { ok = nT >= 1; if (cX >= 1) idx[m++] = 0; if (cY >= 1) idx[m++] = 3; }
        if (!ok) { fall |= 1 << (bit + EAGLE_LINEFIT_FALL_LINES); --rung; continue; }
        double x[8];
        if (!lf_solve(S, idx, m, x)) { fall |= 1 << (bit + EAGLE_LINEFIT_FALL_PIVOT); --rung; continue; }
        double p[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = 0; i < m; ++i) p[idx[i]] = x[i];
        const double D[9] = {1.0 + p[1], p[2], p[0], p[4], 1.0 + p[5], p[3], p[6], p[7], 1.0};
        double M1[9], M2[9], M3[9];
        lf_matmul3(TI, st.m, M1);
        lf_matmul3(D, M1, M2);
        lf_matmul3(T, M2, M3);
        bool good = true;
        for (int i = 0; i < 8; ++i) good = good && fabs(p[i] * 64.0) <= a.max_step;
        for (int i = 0; i < 9; ++i) good = good && isfinite(M3[i]);
        if (!good) { fall |= 1 << (bit + EAGLE_LINEFIT_FALL_CAP); --rung; continue; }
        for (int i = 0; i < 9; ++i) st.m[i] = M3[i];
        break;
    }
    st.fall = fall; st.rung = rung;
    if (rung > 0) st.changed = 1;
}

__global__ __launch_bounds__(64) void linefit_decide_kernel(LfArgs a)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= a.n) return;
    EagleLineFitFrame r{};
    r.n_line = (int32_t)a.nline[f];
    const LfFrame& F = a.tab[f];
    if (!F.ok) { a.rec[f] = r; return; }                    // status NO_MAP; the host keeps the frame's matrix
    const LfState& st = a.st[f];
    const lf_u64* B = a.sums + ((size_t)a.slot_before * a.n + f) * LF_NSUM;
    const lf_u64* A = a.sums + ((size_t)a.slot_after * a.n + f) * LF_NSUM;
    double g[9], m[9];
    for (int i = 0; i < 9; ++i) { g[i] = F.g[i]; m[i] = st.m[i]; }
    int64_t sh = 0;
    const double xs[3] = {0.0, (double)(a.w - 1) / 2.0, (double)(a.w - 1)}, ys[3] = {0.0, (double)(a.h - 1) / 2.0, (double)(a.h - 1)};
    for (int j = 0; j < 3 && sh >= 0; ++j)
        for (int i = 0; i < 3; ++i) {
            int ax, ay, bx, by;
            if (!lf_point(g, xs[i], ys[j], ax, ay) || ax < -10240 || ax > 117760 || ay < -10240 || ay > 79872) continue;
            if (!lf_point(m, xs[i], ys[j], bx, by)) { sh = -1; break; }
            const int64_t dx = (int64_t)ax - bx, dy = (int64_t)ay - by;
            sh = max(sh, dx * dx + dy * dy);
        }
    r.model = st.rung; r.rounds = a.rounds; r.fall = st.fall;
    r.n_before = (int32_t)B[44]; r.e2_before = (int64_t)B[45]; r.n_after = (int32_t)A[44]; r.e2_after = (int64_t)A[45]; r.shift2 = sh;
    int status;
    if (!st.changed) status = EAGLE_LINEFIT_UNCHANGED;
    else if ((int64_t)A[44] < a.min_points) status = EAGLE_LINEFIT_FEW_POINTS;
    else if (!(B[44] == 0 || (double)(int64_t)A[45] / (double)(int64_t)A[44] < (double)(int64_t)B[45] / (double)(int64_t)B[44])) status = EAGLE_LINEFIT_NO_GAIN;
    else if (sh < 0 || sh > a.ms2) status = EAGLE_LINEFIT_SHIFT;
    else status = EAGLE_LINEFIT_ACCEPTED;
    r.status = status;
    a.rec[f] = r;
    if (status == EAGLE_LINEFIT_ACCEPTED)
        for (int i = 0; i < 9; ++i) a.hout[9 * (size_t)f + i] = F.flipped ? -m[i] : m[i];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static int64_t lf_q(double v) { return (int64_t)std::floor(v * 1024.0 + 0.5); }

static void lf_check(const char* who, const void* bgr, int n, int h, int w, const double* Hs, const uint8_t* valid, const EagleLineFitParams* p, const double* Hs_out,
                     const EagleLineFitFrame* frames_out)
{
    if (!p) fail(EAGLE_E_INVALID, "%s: the parameters are NULL", who);
    if (p->k < 1 || p->k > 64) fail(EAGLE_E_INVALID, "%s: k %d is outside 1 .. 64", who, p->k);
    if (p->tau < 1 || p->tau > 1020) fail(EAGLE_E_INVALID, "%s: tau %d is outside 1 .. 1020", who, p->tau);
    if (p->rounds < 0 || p->rounds > LF_MAX_ROUNDS) fail(EAGLE_E_INVALID, "%s: rounds %d is outside 0 .. %d", who, p->rounds, LF_MAX_ROUNDS);
    if (p->model < 1 || p->model > 3) fail(EAGLE_E_INVALID, "%s: model %d is outside 1 .. 3", who, p->model);
    if (p->min_points < 1) fail(EAGLE_E_INVALID, "%s: min_points %d is below 1", who, p->min_points);
    if (p->min_per_line < 1) fail(EAGLE_E_INVALID, "%s: min_per_line %d is below 1", who, p->min_per_line);
    if (!(p->box_pad >= 0.0) || !std::isfinite(p->box_pad)) fail(EAGLE_E_INVALID, "%s: box_pad %g is negative or not finite", who, p->box_pad);
    if (!(p->radius_min > 0.0 && p->radius_min <= p->radius && p->radius <= 8.0) || lf_q(p->radius_min) < 1)
        fail(EAGLE_E_INVALID, "%s: radius %g and radius_min %g must have 1 / 2048 <= radius_min <= radius <= 8", who, p->radius, p->radius_min);
    if (!(p->radius_factor > 0.0 && p->radius_factor <= 1.0)) fail(EAGLE_E_INVALID, "%s: radius_factor %g is outside (0, 1]", who, p->radius_factor);
    if (!(p->max_shift >= 0.0 && p->max_shift <= 1024.0)) fail(EAGLE_E_INVALID, "%s: max_shift %g is outside 0 .. 1024", who, p->max_shift);
    if (!(p->max_step > 0.0 && p->max_step <= 64.0)) fail(EAGLE_E_INVALID, "%s: max_step %g is outside (0, 64]", who, p->max_step);
    for (int i = 0; i < 4; ++i)
        if (p->reserved[i]) fail(EAGLE_E_INVALID, "%s: reserved[%d] is %d, not 0", who, i, p->reserved[i]);
    if (n < 0) fail(EAGLE_E_INVALID, "%s: n is %d", who, n);
    if (h < 1 || h > LF_MAX_DIM || w < 1 || w > LF_MAX_DIM) fail(EAGLE_E_INVALID, "%s: a frame of %d x %d is outside 1 .. %d per side", who, h, w, LF_MAX_DIM);
    if (!Hs_out || !frames_out) fail(EAGLE_E_INVALID, "%s: Hs_out or frames_out is NULL", who);
    if (n > 0 && !bgr) fail(EAGLE_E_INVALID, "%s: the frames are NULL", who);
    if (n > 0 && !Hs) fail(EAGLE_E_INVALID, "%s: the homographies are NULL", who);
    if (n > 0 && !valid) fail(EAGLE_E_INVALID, "%s: the valid flags are NULL", who);
}

static LfFrame lf_frame_map(const double* H, int valid, int h, int w)
{
    LfFrame F{};
    if (!valid) return F;
    bool fin = true;
    for (int k = 0; k < 9; ++k) fin = fin && std::isfinite(H[k]);
    const double s0 = H[6] * ((double)(w - 1) / 2.0), s1 = H[7] * (double)(h - 1);
    const double sb = (s0 + s1) + H[8];
    if (!fin || !std::isfinite(sb) || sb == 0.0) return F;
    F.ok = 1; F.flipped = sb < 0.0;
    for (int k = 0; k < 9; ++k) F.g[k] = F.flipped ? -H[k] : H[k];
    return F;
}

struct LfMem {
    std::vector<void*> owned;
    ~LfMem() { for (void* p : owned) (void)hipFree(p); }
    void* get(size_t b)
    {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, std::max<size_t>(b, 16)));
        owned.push_back(p);
        return p;
    }
    void* upload(const void* src, size_t b, hipStream_t s)
    {
        void* p = get(b);
        if (b) HIP_CHECK(hipMemcpyAsync(p, src, b, hipMemcpyHostToDevice, s));
        return p;
    }
};

// the boxes of all n frames of a call: from the records, or the operator's (boxes, box_off); empty boff: no boxes
struct LfBoxes { std::vector<int32_t> boff; std::vector<float> boxes; };
static LfBoxes lf_boxes(const char* who, int n, const EagleFrameResult* recs, const float* op_boxes, const int32_t* op_off)
{
    LfBoxes b;
    if ((op_boxes != nullptr) != (op_off != nullptr)) fail(EAGLE_E_INVALID, "%s: boxes and box_off come together (boxes %p, box_off %p)", who, (const void*)op_boxes, (const void*)op_off);
    if (!recs && !op_off) return b;
    if (op_off && op_off[0] != 0) fail(EAGLE_E_INVALID, "%s: box_off[0] is %d, not 0", who, op_off[0]);
    b.boff.push_back(0);
    for (int i = 0; i < n; ++i) {
        if (recs) {
            if (recs[i].n_det < 0 || recs[i].n_det > EAGLE_MAX_DET) fail(EAGLE_E_INVALID, "%s: record %d has n_det %d (0 .. %d)", who, i, recs[i].n_det, EAGLE_MAX_DET);
            for (int k = 0; k < recs[i].n_det; ++k) {
                const EagleDet& d = recs[i].det[k];
                b.boxes.insert(b.boxes.end(), {d.x1, d.y1, d.x2, d.y2});
            }
        } else {
            if (op_off[i + 1] < op_off[i] || op_off[i + 1] - op_off[i] > EAGLE_MAX_DET)
                fail(EAGLE_E_INVALID, "%s: frame %d has %d boxes (0 .. %d)", who, i, op_off[i + 1] - op_off[i], EAGLE_MAX_DET);
            b.boxes.insert(b.boxes.end(), op_boxes + 4 * (size_t)op_off[i], op_boxes + 4 * (size_t)op_off[i + 1]);
        }
        b.boff.push_back((int32_t)(b.boxes.size() / 4));
    }
    return b;
}

// Frames i0 .. i0 + m of the call (m <= LF_PASS), dense at d_bgr: every launch of the stage on stream s, then the results to the host.  Returns when
// they are complete.
static void lf_run(EagleHandle* hd, hipStream_t s, const uint8_t* d_bgr, int i0, int m, int h, int w, const double* Hs, const uint8_t* valid, const LfBoxes& bx,
                   const EagleLineFitParams* p, double* Hs_out, EagleLineFitFrame* frames_out, uint32_t* masks_out)
{
    LfMem mem;
    std::vector<LfFrame> tab(m);
    std::vector<LfState> st(m);
    for (int i = 0; i < m; ++i) {
        tab[i] = lf_frame_map(Hs + 9 * (size_t)(i0 + i), valid[i0 + i], h, w);
        st[i] = LfState{};
        for (int k = 0; k < 9; ++k) st[i].m[k] = tab[i].g[k];
    }
    LfArgs a{};
    a.bgr = d_bgr; a.fstride = (int64_t)h * w * 3; a.n = m; a.h = h; a.w = w; a.wpr = (w + 31) / 32;
    a.k = p->k; a.tau = p->tau; a.pad = p->box_pad;
    a.model = p->model; a.min_points = p->min_points; a.min_per_line = p->min_per_line; a.max_step = p->max_step; a.rounds = p->rounds;
    const int64_t ms = lf_q(p->max_shift);
    a.ms2 = ms * ms;
    a.tab = (const LfFrame*)mem.upload(tab.data(), (size_t)m * sizeof(LfFrame), s);
    a.st = (LfState*)mem.upload(st.data(), (size_t)m * sizeof(LfState), s);
    std::vector<int32_t> boff;
    if (!bx.boff.empty()) {
        const int32_t b0 = bx.boff[i0];
        for (int i = 0; i <= m; ++i) boff.push_back(bx.boff[i0 + i] - b0);
        a.boff = (const int32_t*)mem.upload(boff.data(), boff.size() * 4, s);
        a.boxes = (const float4*)mem.upload(bx.boxes.data() + 4 * (size_t)b0, (size_t)boff[m] * 16, s);
    }
    const int slots = p->rounds + 2;
    const size_t mask_words = (size_t)m * h * a.wpr, sum_bytes = (size_t)slots * m * LF_NSUM * 8;
    a.mask = (uint32_t*)mem.get(mask_words * 4);
    a.nline = (uint32_t*)mem.get((size_t)m * 4);
    a.sums = (lf_u64*)mem.get(sum_bytes);
    a.hout = (double*)mem.get((size_t)m * 72);
    a.rec = (EagleLineFitFrame*)mem.get((size_t)m * sizeof(EagleLineFitFrame));
    HIP_CHECK(hipMemsetAsync(a.nline, 0, (size_t)m * 4, s));
    HIP_CHECK(hipMemsetAsync(a.sums, 0, sum_bytes, s));
    HIP_CHECK(hipMemsetAsync(a.hout, 0, (size_t)m * 72, s));
    auto timed = [&](const char* name, double bytes, const std::function<void()>& fn) { if (hd) timed_launch(hd, name, bytes, s, fn); else fn(); };
    timed("linefit_mask", (double)m * h * w * 3.0, [&] {
        hipLaunchKernelGGL(linefit_mask_kernel, dim3((unsigned)((w + 255) / 256), (unsigned)h, (unsigned)m), dim3(256), 0, s, a);
        HIP_CHECK(hipGetLastError());
    });
    const dim3 agrid((unsigned)(((int64_t)h * a.wpr + 255) / 256), (unsigned)m);
    auto accumulate = [&](int slot, int use_orig, int64_t rq) {
        LfArgs b = a;
        b.slot = slot; b.use_orig = use_orig; b.rq2 = rq * rq;
        timed("linefit_accumulate", (double)mask_words * 4.0, [&] {
            hipLaunchKernelGGL(linefit_accumulate_kernel<false>, agrid, dim3(256), 0, s, b);
            HIP_CHECK(hipGetLastError());
        });
    };
    const dim3 fgrid((unsigned)((m + 63) / 64));
    double r = p->radius;
    for (int t = 0; t < p->rounds; ++t) {
        accumulate(t, 0, lf_q(r));
        LfArgs b = a;
        b.slot = t;
        timed("linefit_solve", (double)m * LF_NSUM * 8.0, [&] {
            hipLaunchKernelGGL(linefit_solve_kernel, fgrid, dim3(64), 0, s, b);
            HIP_CHECK(hipGetLastError());
        });
        r = r * p->radius_factor;
        if (r < p->radius_min) r = p->radius_min;
    }
    accumulate(p->rounds, 1, lf_q(p->radius_min));
    accumulate(p->rounds + 1, 0, lf_q(p->radius_min));
    {
        LfArgs b = a;
        b.slot_before = p->rounds; b.slot_after = p->rounds + 1;
        timed("linefit_decide", (double)m * 128.0, [&] {
            hipLaunchKernelGGL(linefit_decide_kernel, fgrid, dim3(64), 0, s, b);
            HIP_CHECK(hipGetLastError());
        });
    }
    std::vector<double> hout((size_t)m * 9);
    HIP_CHECK(hipMemcpyAsync(hout.data(), a.hout, (size_t)m * 72, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(frames_out + i0, a.rec, (size_t)m * sizeof(EagleLineFitFrame), hipMemcpyDeviceToHost, s));
    if (masks_out) HIP_CHECK(hipMemcpyAsync(masks_out + (size_t)i0 * h * a.wpr, a.mask, mask_words * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (hd && hd->prof) collect_spans(hd);
    for (int i = 0; i < m; ++i) {
        const bool acc = frames_out[i0 + i].status == EAGLE_LINEFIT_ACCEPTED;
        std::memcpy(Hs_out + 9 * (size_t)(i0 + i), acc ? hout.data() + 9 * (size_t)i : Hs + 9 * (size_t)(i0 + i), 72);
    }
}

}  // namespace eagle

extern "C" {

int eagle_linefit_params_default(EagleLineFitParams* p)
{
    if (!p) return EAGLE_E_INVALID;
    *p = EagleLineFitParams{};
    p->k = 4; p->tau = 200; p->rounds = 5; p->model = EAGLE_LINEFIT_PROJECTIVE; p->min_points = 200; p->min_per_line = 20;
    p->box_pad = 3.0; p->radius = 2.5; p->radius_min = 0.5; p->radius_factor = 0.6; p->max_shift = 3.0; p->max_step = 4.0;
    return EAGLE_OK;
}

int eagle_linefit_device_frames(EagleHandle* h, const uint8_t* d_bgr, int n, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                                const EagleLineFitParams* p, double* Hs_out, EagleLineFitFrame* frames_out, uint32_t* masks_out)
{
    API_BEGIN_H(h)
    const char* who = "eagle_linefit_device_frames";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    lf_check(who, d_bgr, n, fh, fw, Hs, valid, p, Hs_out, frames_out);
    const LfBoxes bx = lf_boxes(who, n, recs, nullptr, nullptr);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const int64_t fb = (int64_t)fh * fw * 3;
    for (int i0 = 0; i0 < n; i0 += LF_PASS)
        lf_run(h, h->s_main, d_bgr + (int64_t)i0 * fb, i0, std::min(LF_PASS, n - i0), fh, fw, Hs, valid, bx, p, Hs_out, frames_out, masks_out);
    API_END(h)
}

int eagle_linefit_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t max_staging_bytes, const double* Hs, const uint8_t* valid, const EagleFrameResult* recs,
                         const EagleLineFitParams* p, double* Hs_out, EagleLineFitFrame* frames_out, uint32_t* masks_out)
{
    API_BEGIN_H(h)
    const char* who = "eagle_linefit_frames";
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    lf_check(who, bgr, n, fh, fw, Hs, valid, p, Hs_out, frames_out);
    if (max_staging_bytes < 0) fail(EAGLE_E_INVALID, "%s: max_staging_bytes %lld is negative", who, (long long)max_staging_bytes);
    const LfBoxes bx = lf_boxes(who, n, recs, nullptr, nullptr);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    const int64_t fb = (int64_t)fh * fw * 3;
    const int pass = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(n, LF_PASS), (max_staging_bytes ? max_staging_bytes : LF_STAGING) / fb));
    LfMem mem;
    uint8_t* stage = (uint8_t*)mem.get((size_t)pass * fb);
    for (int i0 = 0; i0 < n; i0 += pass) {
        const int m = std::min(pass, n - i0);
        HIP_CHECK(hipMemcpyAsync(stage, bgr + (int64_t)i0 * fb, (size_t)m * fb, hipMemcpyHostToDevice, h->s_main));
        lf_run(h, h->s_main, stage, i0, m, fh, fw, Hs, valid, bx, p, Hs_out, frames_out, masks_out);      // (returns after the stream has drained: the next pass reuses the staging)
    }
    API_END(h)
}

int eagle_op_linefit(int device, const uint8_t* bgr, int n, int h, int w, const double* Hs, const uint8_t* valid, const float* boxes, const int32_t* box_off,
                     const EagleLineFitParams* p, double* Hs_out, EagleLineFitFrame* frames_out, uint32_t* masks_out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    const char* who = "eagle_op_linefit";
    lf_check(who, bgr, n, h, w, Hs, valid, p, Hs_out, frames_out);
    const LfBoxes bx = lf_boxes(who, n, nullptr, boxes, box_off);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    const int64_t fb = (int64_t)h * w * 3;
    LfMem mem;
    for (int i0 = 0; i0 < n; i0 += LF_PASS) {
        const int m = std::min(LF_PASS, n - i0);
        const uint8_t* d_bgr = (const uint8_t*)mem.upload(bgr + (int64_t)i0 * fb, (size_t)m * fb, nullptr);
        lf_run(nullptr, nullptr, d_bgr, i0, m, h, w, Hs, valid, bx, p, Hs_out, frames_out, masks_out);
    }
    API_END(hh)
}

}  // extern "C"
