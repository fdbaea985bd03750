#ifndef EAGLE_CONV_AD_SPLIT32_INC
#define EAGLE_CONV_AD_SPLIT32_INC
// -DEAGLE_ABL_M32=n (developer ablation builds only, tools/convbench/ablate_split.sh; 0 = the product): 1 the MFMAs replaced by one v_xor3 each, 2 no weight-fragment
// loads after the item's first RING - 1 steps, 3 no halo requests (LDS-DMA) after the workgroup's first, 4 no LDS fragment reads after a chunk's first tap, 5 no
// output stores / residual loads, 6 all of them, 7 only the memory traffic removed (2 + 3 + 5), 8 every halo request after the workgroup's first re-reads channel chunk 0 of
// its pixels (cache-hot, NON-ZERO data: separates what the halo's bytes cost from what multiplying by zeros saves in power under 3; weights and stores as in the product —
// the first build of this ablation tested ">= 6" and silently dropped them too, which produced a "27 %" that was ablation 7's: profiles/r05n).  Results are garbage by
// construction; only the time is of interest.
#ifndef EAGLE_ABL_M32
#define EAGLE_ABL_M32 0
#endif
// (Measured in round 5 and taken out again, each negative: cache-policy bits on the halo requests (sc0 / sc1: nothing; nt: -2 ... -5 %), the slab requests spread over the
//  chunk's taps, three halo slots with the requests of two chunks issued together (variant 25), two chunks per request as whole 128-byte lines in 144-byte records (variant 26):
//  DESIGN.md 10.9, profiles/r05f_*, r05h_*, r05ijk_*; the code is in the history at commit "Variant 26 (whole-line halo requests) ...".)
// -DEAGLE_M32_SAUX=n (developer measurement): cache-policy bits of the output stores (bits 0..1; 2 = nt: streaming through the L2 instead of displacing the halo lines
// and the weight image); bit 2: the residual loads non-temporal as well (read-once data)
#ifndef EAGLE_M32_RES_NT
#define EAGLE_M32_RES_NT 1
#endif
#ifndef EAGLE_M32_SAUX
#define EAGLE_M32_SAUX (EAGLE_STORE_NT * 2 + EAGLE_M32_RES_NT * 4)
#endif
// ------------------------------------------------------------------------------------------------------------
// Split-precision family (EAGLE_PREC_F32S), variants 21 / 22 (round 5): the A-direct 3x3 stride-1 kernel on v_mfma_f32_32x32x16_f16.
//
// Same skeleton as conv_ad_split.inc — four waves, weight fragments straight from global memory / L2 into registers through a small ring, activations by
// LDS-DMA into a two-deep halo ring that runs on across the workgroup's XCD-contiguous items, one s_barrier per 16-channel chunk, two workgroups per CU,
// wave-private epilogue through an LDS strip — but the wave tile is 96 output channels x 2 rows x 32 pixels = 3 x 2 accumulator blocks of 32 x 32
// (the same 96 accumulator registers as the 48-channel x 128-pixel tile of the 16x16 form), and K = 16 per instruction = the two 8-channel groups of
// the chunk:
//   * a B fragment is 32 pixels x (g0 | g1): lanes 0..31 read record slot s of pixels x .. x + 31, lanes 32..63 slot s + 1.  The (hi g0, hi g1) fragment
//     and the (lo g0, lo g1) fragment of a tap are TWO ds_read_b128 per row and serve all three products: Whi x Xhi, Whi x Xlo, Wlo x Xhi — nothing is
//     read twice (the 16x16x32 form reads 8 fragments per K-step and 14 K-steps per chunk because its K = 32 has to be filled with four distinct
//     8-channel slots: 112 fragment reads per chunk and wave against 36 here);
//   * an A fragment is 32 output channels x (g0 | g1) of one tap, hi or lo: 2 x 3 loads per tap and wave, no duplicated half as in the 16x16 form's
//     (Whi g0, Whi g1, Whi g0, Whi g1) K-steps: 54 KB per chunk and wave for 96 channels against 42 KB for 48 channels;
//   * 18 MFMAs of 32x32x16 per tap = 162 per chunk, every one of them useful (the 16x16 form: 336 of which 324 are);
//   * per tap two "steps": (Whi: 12 MFMAs against the hi and lo fragments), (Wlo: 6 MFMAs against the hi fragments); the weight ring holds RING steps,
//     18 steps per chunk is a multiple of RING = 3 (and 6): no ring-phase bookkeeping, hence ANY number of 16-channel chunks (the 16x16 form: Cin = 48 k);
//   * LDS record = [hi g0][hi g1][lo g0][lo g1] + ONE pad slot = 80 bytes: pixel stride 20 banks, so the 16 pixels of every ds_read_b128 lane group
//     ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, MI355X_MICROARCH.md) fall on 16 distinct 4-bank columns — conflict-free with one
//     address register and immediates;
//   * C / D layout of the 32x32 block: lane holds pixel (lane & 31) and the channels 8 j + 4 (lane >> 5) + r (j, r = 0..3): four runs of 4 consecutive
//     channels -> the same 8-byte (hi) + 8-byte (lo) strip stores as the 16x16 form; a pass of the epilogue is one row (32 pixels) x one 32-channel block.
// Workgroup forms: <CQ, PG> = <2, 2>: BN = 192, tile 4 rows x 32 (variant 21; geometry of variant 8); <1, 4>: BN = 96, tile 8 rows x 32 (variant 22;
// geometry of variant 9; all four waves stream the same weight fragments).
// NRH = 2 (variants 23 / 24): the wave's two 32-pixel blocks lie SIDE BY SIDE in one row instead of in two rows — wave tile 96 channels x 1 row x 64 pixels,
// workgroup tile PG rows x 64 columns.  HRNet's maps are 34 x 60 and 68 x 120: 2- and 4-row tiles divide 34 and 68 exactly where the 4- and 8-row tiles compute
// 36 and 72 rows, the column remainder (60 -> 64, 120 -> 128) is the same: 6.7 % of the MFMAs on padding instead of 12.9 %.  Halo (PG + 2) rows x 66 records.
// The epilogue strips are 128-byte records with the 16-byte unit XOR-swizzled by the pixel (unit ^ (pixel & 7)): no padding (the 4 x 64 tile of variant 24 then
// fits two workgroups per CU to the byte: 2 x 32 KB halo ring + 4 x 4 KB strips = 80 KB), 2-way conflicts at most on the 8-byte strip writes, none on the 16-byte reads.
// MAPW = 30 (variant 27; BN = 192 only): LINEAR tiling.  An item owns the 128 consecutive pixels L0 = 128 t .. L0 + 127 of the frame's row-major sequence
// L = y W + x instead of a rectangle: wave pg the 32-pixel blocks 2 pg and 2 pg + 1, lane lx of block b pixel L0 + 32 b + lx.  17 x 30 = 510 pixels are 4 items
// per frame where 4 x 32 tiles need 5 (25.5 % of their MFMAs on padding).  The halo holds WHOLE map rows of MAPW + 2 records (x = -1 .. W): rows y_first - 1 ..
// y_first + LROWS, y_first = L0 / W, LROWS = 126 / W + 2 = 6 = the rows 128 consecutive pixels can touch -> 8 x 32 records = 20 slabs per slot, 56 KB of LDS with
// the strips; 256 records x 400 items = the 204 x 500 of the 4 x 32 tiles: the halo traffic is unchanged.  Same slab decomposition and (iy, ix) bounds test; each
// block has its own per-lane fragment base ((y - y_first) * HW_ + x) * PS, computed once per item, the tap offsets stay immediates.  Lanes past the frame's last
// pixel read that pixel and store out of range.  The epilogue's pixel index is n H W + L.  Same chunk, tap and product order into the same accumulators as
// variant 21: bit-identical results.  384->384 @17x30, B = 50: 222 -> 177 us isolated, +1.2 % frames/s in the pipeline (docs/experiments.md 10.11).
// (MAPW = 60 for the 34 x 60 maps — 16 items per frame instead of 18, halo 6 x 62 records = 32 slabs, 80 KB — was built with it, bit-identical too, and taken
//  out again: 372 x 800 halo records per launch against 204 x 900 cost more than 11 % fewer MFMAs gave, 180 -> 188 us isolated, a mixed +0.5 % in the pipeline.)
// The 96-channel class stays on variant 24: a full-width halo at W = 120 (its 256 pixels: 6 x 122 records x 2 slots = 120 KB) leaves one workgroup per CU, and
// its padding is 6.7 % only.
// Weight image (conv_tile_weights): [Cout block][chunk][tap 0..8][hi | lo][BN / 32 blocks][lane 0..63][8].
// ------------------------------------------------------------------------------------------------------------
using f32x16 = __attribute__((ext_vector_type(16))) float;
#if EAGLE_ABL_M32 == 1 || EAGLE_ABL_M32 == 6
__device__ __forceinline__ f32x16 abl_m32_xor(const half8& a_, const half8& b_, f32x16 c_)
{
    const u32x4 ua = __builtin_bit_cast(u32x4, a_), ub = __builtin_bit_cast(u32x4, b_);
    c_[0] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, c_[0]) ^ ua[0] ^ ub[3]);
    return c_;
}
#define EAGLE_MFMA_M32(A_, B_, C_) abl_m32_xor(A_, B_, C_)
#else
#define EAGLE_MFMA_M32(A_, B_, C_) __builtin_amdgcn_mfma_f32_32x32x16_f16(A_, B_, C_, 0, 0, 0)
#endif
// split_store4 with the lo half at its own address (swizzled strips)
__device__ __forceinline__ void split_store4x(char* dhi, char* dlo, float v0, float v1, float v2, float v3)
{
    const float s0 = __builtin_amdgcn_fmed3f(v0 * SPLIT_SX, -65504.0f, 65504.0f), s1 = __builtin_amdgcn_fmed3f(v1 * SPLIT_SX, -65504.0f, 65504.0f),
                s2 = __builtin_amdgcn_fmed3f(v2 * SPLIT_SX, -65504.0f, 65504.0f), s3 = __builtin_amdgcn_fmed3f(v3 * SPLIT_SX, -65504.0f, 65504.0f);
    const half4 hi = {(_Float16)s0, (_Float16)s1, (_Float16)s2, (_Float16)s3};
    const half4 lo = {(_Float16)(s0 - (float)hi[0]), (_Float16)(s1 - (float)hi[1]), (_Float16)(s2 - (float)hi[2]), (_Float16)(s3 - (float)hi[3])};
    *(half4*)dhi = hi; *(half4*)dlo = lo;
}
template <int CQ, int PG, int RES, int RING = 3, int NRH = 1, int MAPW = 0>
__global__ __launch_bounds__(256, 2) void conv_split_ad32_kernel(ConvArgs a)
{
    static_assert(CQ * PG == 4, "four waves per workgroup");
    constexpr bool LIN = MAPW != 0;                       // the item owns 128 consecutive pixels of the frame's row-major sequence (map width MAPW, a.W == a.Wo == MAPW)
    static_assert(!LIN || (CQ == 2 && PG == 2 && NRH == 1 && MAPW == 30), "linear tiling: the BN = 192 form on the 30-column map");
    static_assert(NRH == 1 || NRH == 2, "the wave's two pixel blocks: one above the other (1) or side by side (2)");
    static_assert(18 % RING == 0 && RING >= 3, "the weight ring holds a divisor of the 18 steps of a chunk");
    using rsrc_t = __amdgpu_buffer_rsrc_t;
    constexpr unsigned OOB = 0x80000000u;
    constexpr int MB = 3, NR = 2, NRV = NR / NRH, NW = 4, BN = CQ * 96, TH = NRV * PG, TW = 32 * NRH;      // wave tile: MB blocks of 32 channels x NRV rows x NRH blocks of 32 pixels
    constexpr int KSTEP = (BN / 32) * 1024;              // bytes of one step of the weight image (one tap, hi or lo, the whole Cout block)
    // halo record: [hi g0][hi g1][lo g0][lo g1] + ONE pad slot = 80 bytes: 20 banks per pixel put the 16 pixels of a ds_read_b128 lane group on 16 distinct 4-bank columns
    constexpr int PS = 80, SPC = 18, AHEAD = RING - 1;
    constexpr int LROWS = LIN ? (128 - 2) / (LIN ? MAPW : 1) + 2 : 0;      // map rows that 128 consecutive pixels touch at most: 6 at 30 columns
    constexpr int HW_ = LIN ? MAPW + 2 : TW + 2, HPIX = (LIN ? LROWS + 2 : TH + 2) * HW_;      // linear: whole map rows y_first - 1 .. y_first + LROWS, columns -1 .. MAPW
    constexpr int HSLABS = ((HPIX * PS + 1023) / 1024 + NW - 1) / NW * NW, HB = HSLABS * 1024, HK = HSLABS / NW;
    constexpr int RS = 32 * 4, STRIP = 32 * RS;          // one pass: 32 pixels x 32 channels x 4 bytes, 16-byte units XOR-swizzled by the pixel
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Hb = smem;                                // 2 x HB
    char* const strip = smem + 2 * HB + (threadIdx.x >> 6) * STRIP;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cq = wave % CQ, pg = wave / CQ, kh = lane >> 5, lx = lane & 31;
    const int gy = a.gy, nitems = a.tiles_x * a.tiles_y * a.N * gy, nwg = gridDim.x;
    int item0, item_end;
    {
        const int b = blockIdx.x, xcd = b & 7, k = b >> 3;
        const int wgs_here = (nwg + 7 - xcd) >> 3;
        const int qn = nitems >> 3, rn = nitems & 7;
        const int x0 = xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn;
        const int xc = qn + (xcd < rn ? 1 : 0);
        item0 = x0 + (int)((long)xc * k / wgs_here);
        item_end = x0 + (int)((long)xc * (k + 1) / wgs_here);
    }
    if (item0 >= item_end) return;
    const int nloc = item_end - item0, nch = a.nchunks, GC = nloc * nch;
    const rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, 0x7FFFFFFF, 0x00020000);
    const rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, 0, 0x7FFFFFFF, 0x00020000);
    const rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.r1, 0, 0x7FFFFFFF, 0x00020000);
    const rsrc_t rrs2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.r2, 0, 0x7FFFFFFF, 0x00020000);
    const rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.y, 0, 0x7FFFFFFF, 0x00020000);
    // slab k of this wave covers LDS 16-byte slots e = (wave + NW k) * 64 + lane: halo pixel e / 5, record slot e % 5 (slot 4 = padding).
    // record slot (hi g0, hi g1, lo g0, lo g1) <- the tensor's unit (hi g0, lo g0, hi g1, lo g1)
    constexpr bool RECOMP = HK > 6;                       // (as in conv_ad_split.inc: the 8-row tile recomputes the decomposition at every request instead of holding it)
    const int e0 = wave * 64 + lane;
    int hpk[RECOMP ? 1 : HK];                             // per slab: halo row | column << 8 | source 16-byte unit << 16, or -1 (padding)
    if constexpr (!RECOMP) {
#pragma unroll
        for (int k = 0; k < HK; ++k) {
            const int e = e0 + NW * 64 * k;
            const int pix = e / 5, slot = e - pix * 5;
            const int hy = pix / HW_, hx = pix - hy * HW_;
            hpk[k] = (pix < HPIX && slot < 4) ? (hy | (hx << 8) | (((slot & 1) * 2 + (slot >> 1)) << 16)) : -1;
        }
    }
    const int bbase = ((pg * NRV) * HW_ + lx) * PS + kh * 16;      // B fragments: lanes 0..31 slot s (g0), lanes 32..63 slot s + 1 (g1); hi: s = 0, lo: s = 2
    const unsigned wlane = (unsigned)((cq * MB * 64 + lane) * 16);

    auto decode = [&](int item, int& n, int& ty, int& tx, int& nb) {
        int t = item / gy; nb = item - t * gy;
        tx = t % a.tiles_x; t /= a.tiles_x;
        ty = t % a.tiles_y; n = t / a.tiles_y;
    };
    // ---- halo ring: global chunk index = local item * nch + chunk; slot = index & 1 -------------------------------------------
    int h_g = 0, h_ch = 0, h_item = item0;
    int h_iy0, h_ix0, h_gb;                                // geometry of the item the next request belongs to (scalars)
    auto halo_origin = [&](int item) {
        int n, ty, tx, nb; decode(item, n, ty, tx, nb);
        if constexpr (LIN) { h_iy0 = (tx * 128) / MAPW - 1; h_ix0 = -1; }      // tx: the item's index in the frame (tiles_y = 1); the row of its first pixel
        else { h_iy0 = ty * TH - 1; h_ix0 = tx * TW - 1; }
        h_gb = (((n * a.H + h_iy0) * a.W + h_ix0) * a.xcs + a.xoff) * 2;       // xcs / xoff: fp16 elements (two per logical channel)
    };
    halo_origin(h_item);
    auto issue_h_slab = [&](int k) {                       // slab k of the next chunk's halo (k is a compile-time constant at every call site)
        char* dst = Hb + (h_g & 1) * HB;                  // (past the last chunk: the same requests again, harmlessly, so that the count stays static)
        const unsigned so = (EAGLE_ABL_M32 == 8) ? 0u : (unsigned)(h_ch * 32) * 2u;   // 16 logical channels = 32 fp16 elements per chunk
        int hy, hx, unit; bool live;
        if constexpr (RECOMP) {
            int e = e0 + NW * 64 * k;
            asm volatile("" : "+v"(e));                 // keep the decomposition below from being hoisted out of the item loop into registers
            const int pix = (int)(((unsigned)e * 52429u) >> 18), slot = e - pix * 5;              // e / 5 for e < 2^16
            hy = HW_ == 34 ? (int)(((unsigned)pix * 1928u) >> 16) : (int)(((unsigned)pix * 993u) >> 16); hx = pix - hy * HW_;      // pix / 34, pix / 66 for pix < 2^11
            unit = (slot & 1) * 2 + (slot >> 1);
            live = pix < HPIX && slot < 4;
        } else {
            hy = hpk[k] & 0xFF; hx = (hpk[k] >> 8) & 0xFF; unit = (hpk[k] >> 16) & 7; live = hpk[k] >= 0;
        }
        const int iy = h_iy0 + hy, ix = h_ix0 + hx;
        const unsigned off = !(live && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) ? OOB
                             : (unsigned)(h_gb + ((hy * a.W + hx) * a.xcs + unit * 8) * 2);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(dst + (wave + NW * k) * 1024), 16,
                                                 ((EAGLE_ABL_M32 == 3 || EAGLE_ABL_M32 == 6 || EAGLE_ABL_M32 == 7) && h_g > 0) ? OOB : off, so, 0, 0);
    };
    auto advance_h = [&]() {
        if (h_g + 1 >= GC) return;
        ++h_g;
        if (++h_ch == nch) { h_ch = 0; ++h_item; halo_origin(h_item); }
    };
    auto issue_h = [&]() {
#pragma unroll
        for (int k = 0; k < HK; ++k) issue_h_slab(k);
        advance_h();
    };
    issue_h();
    int gc = 0;
    for (int item = item0; item < item_end; ++item) {
        int n, ty, tx, nb; decode(item, n, ty, tx, nb);
        const int oy0 = ty * TH, ox0 = tx * TW;
        // linear tiling: lane lx of the wave's block p holds pixel L0 + 32 (2 pg + p) + lx of the frame; the lanes past the frame's last pixel read that pixel
        // (their stores go out of range).  One B-fragment base per block: halo row y - y_first (+ ky), record x (+ kx).
        const int L0 = tx * 128, npix = a.H * a.W;
        int bbl[LIN ? NR : 1];
        if constexpr (LIN) {
            const int yf = L0 / MAPW;
#pragma unroll
            for (int p = 0; p < NR; ++p) {
                const int L = min(L0 + (pg * NR + p) * 32 + lx, npix - 1), y = L / MAPW, x = L - y * MAPW;
                bbl[p] = ((y - yf) * HW_ + x) * PS + kh * 16;
            }
        }
        f32x16 acc[MB][NR];
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int p = 0; p < NR; ++p)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][p][r] = 0.f;
        // A ring: the fragments of steps s .. s + RING - 1 of the item's step sequence (slot = sequence index % RING; 18 steps per chunk keep the slots static)
        u32x4 A[RING][MB];
        unsigned wsrc = (unsigned)(nb * nch * SPC) * (unsigned)KSTEP;      // step 0 of this item
        const unsigned wend = wsrc + (unsigned)(nch * SPC) * (unsigned)KSTEP;
        bool abl_a_done = false;
        auto load_a = [&](int slot) {                      // requests the next step of the item (the last AHEAD requests of an item repeat its last step)
            const unsigned so = wsrc < wend ? wsrc : wend - KSTEP;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
                if (!((EAGLE_ABL_M32 == 2 || EAGLE_ABL_M32 == 6 || EAGLE_ABL_M32 == 7) && abl_a_done)) A[slot][mb] = __builtin_amdgcn_raw_buffer_load_b128(wrs, wlane + mb * 1024, so, 0);
            wsrc += KSTEP;
        };
#pragma unroll
        for (int s = 0; s < AHEAD; ++s) load_a(s);
        abl_a_done = true;
        for (int ch = 0; ch < nch; ++ch, ++gc) {
            // chunk gc has landed (requested one chunk ago); every wave is done with the other slot
            if constexpr (AHEAD * MB == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");        // everything older than the AHEAD steps of A in flight
            else asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
            static_assert(AHEAD * MB == 6 || AHEAD * MB == 15, "vmcnt literal");
            __builtin_amdgcn_s_barrier();
            issue_h();                                              // chunk gc + 1 into the slot chunk gc - 1 used
            const char* hb = Hb + (gc & 1) * HB + bbase;
            const char* hbl[LIN ? NR : 1];
            if constexpr (LIN) {
#pragma unroll
                for (int p = 0; p < NR; ++p) hbl[p] = Hb + (gc & 1) * HB + bbl[p];
            }
            half8 Bh[2][NR], Bl[2][NR];
            auto read_b = [&](int slot, int tap) {
                const int ky = tap / 3, kx = tap - ky * 3;
#pragma unroll
                for (int p = 0; p < NR; ++p) {      // block p: row p / NRH of the wave, 32-pixel column group p % NRH
                    if constexpr (LIN) {
                        Bh[slot][p] = *(const half8*)(hbl[p] + (ky * HW_ + kx) * PS);
                        Bl[slot][p] = *(const half8*)(hbl[p] + (ky * HW_ + kx) * PS + 32);
                    } else {
                        Bh[slot][p] = *(const half8*)(hb + ((p / NRH + ky) * HW_ + (p % NRH) * 32 + kx) * PS);
                        Bl[slot][p] = *(const half8*)(hb + ((p / NRH + ky) * HW_ + (p % NRH) * 32 + kx) * PS + 32);
                    }
                }
            };
            read_b(0, 0);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int bs = (EAGLE_ABL_M32 == 4 || EAGLE_ABL_M32 == 6) ? 0 : (t & 1);
                // step 2 t: Whi of tap t against the hi and the lo fragments
                load_a((2 * t + AHEAD) % RING);
                if (t + 1 < 9 && !(EAGLE_ABL_M32 == 4 || EAGLE_ABL_M32 == 6)) read_b((t + 1) & 1, t + 1);
#pragma unroll
                for (int p = 0; p < NR; ++p)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) acc[mb][p] = EAGLE_MFMA_M32((half8)A[(2 * t) % RING][mb], Bh[bs][p], acc[mb][p]);
#pragma unroll
                for (int p = 0; p < NR; ++p)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) acc[mb][p] = EAGLE_MFMA_M32((half8)A[(2 * t) % RING][mb], Bl[bs][p], acc[mb][p]);
                __builtin_amdgcn_sched_barrier(0);
                // step 2 t + 1: Wlo of tap t against the hi fragments
                load_a((2 * t + 1 + AHEAD) % RING);
#pragma unroll
                for (int p = 0; p < NR; ++p)
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) acc[mb][p] = EAGLE_MFMA_M32((half8)A[(2 * t + 1) % RING][mb], Bh[bs][p], acc[mb][p]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        const int co0 = nb * BN + cq * 96;
        __builtin_amdgcn_sched_barrier(0);
        const float ds = a.descale;
        // piece e = i * 64 + lane of a pass (one row of 32 pixels x one 32-channel block): pixel e / 8, 16-byte unit e % 8 (4 channel groups x (hi, lo), tensor order)
        int pstrip[4], ppx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = i * 64 + lane, px = e >> 3, u = e & 7;
            pstrip[i] = px * RS + ((u ^ (px & 7)) * 16);
            ppx[i] = px | (u << 8);
        }
        auto piece_off = [&](int pass, int i, int cs, int off) -> unsigned {      // pass = pixel block * MB + channel block; cs / off in fp16 elements
            const int row = pass / MB, mb = pass - row * MB;
            if constexpr (LIN) {                            // NHWC pixel n H W + L; the tail of the frame's last block goes out of range
                const int L = L0 + (pg * NR + row) * 32 + (ppx[i] & 0xFF), u = ppx[i] >> 8;
                return L < npix ? (unsigned)(((n * npix + L) * cs + off + (co0 + mb * 32) * 2 + u * 8) * 2) : OOB;
            }
            const int oy = oy0 + pg * NRV + row / NRH, ox2 = ox0 + (row % NRH) * 32 + (ppx[i] & 0xFF), u = ppx[i] >> 8;
            return (oy < a.Ho && ox2 < a.Wo) ? (unsigned)((((n * a.Ho + oy) * a.Wo + ox2) * cs + off + (co0 + mb * 32) * 2 + u * 8) * 2) : OOB;
        };
        float vmax = 0.0f;                                  // largest |v| this lane stores (saturation report, split_report)
        constexpr int NPASS = NR * MB, PB = (RES == 2 && NRH == 2) ? 2 : (RES == 2 || (RES == 1 && NRH == 2)) ? 3 : 6;   // passes whose residual pieces are in flight together (registers; the side-by-side form
                                                                                        // carries a few more address registers: six passes in flight spilled two VGPRs)
        u32x4 rres[RES >= 1 ? PB : 1][4], rres2[RES >= 2 ? PB : 1][4];
        char* const sp = strip + lx * RS + kh * 8;           // the lane's 4-channel run j of a pass: hi in unit 2 j, lo in unit 2 j + 1, units swizzled by the pixel
        const int sw = (lx & 7) * 16;
        auto run_hi = [&](int j) -> char* { return sp + ((j * 32) ^ sw); };
        auto run_lo = [&](int j) -> char* { return sp + ((j * 32 + 16) ^ sw); };
#pragma unroll
        for (int pb0 = 0; pb0 < NPASS; pb0 += PB) {
            if (RES >= 1) {
#pragma unroll
                for (int h2 = 0; h2 < PB; ++h2)
#pragma unroll
                    for (int i = 0; i < 4; ++i) rres[h2][i] = __builtin_amdgcn_raw_buffer_load_b128(rrs, piece_off(pb0 + h2, i, a.r1cs, a.r1off), 0, (EAGLE_M32_SAUX & 4) ? 2 : 0);
            }
            if (RES >= 2) {
#pragma unroll
                for (int h2 = 0; h2 < PB; ++h2)
#pragma unroll
                    for (int i = 0; i < 4; ++i) rres2[h2][i] = __builtin_amdgcn_raw_buffer_load_b128(rrs2, piece_off(pb0 + h2, i, a.r2cs, a.r2off), 0, (EAGLE_M32_SAUX & 4) ? 2 : 0);
            }
#pragma unroll
            for (int h2 = 0; h2 < PB; ++h2) {
                const int pass = pb0 + h2, row = pass / MB, mb = pass - row * MB;
                if (RES >= 1) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) *(u32x4*)(strip + pstrip[i]) = rres[h2][i];
                }
                float v[4][4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float4 bv = *(const float4*)(a.bias + co0 + mb * 32 + j * 8 + kh * 4);
                    v[j][0] = acc[mb][row][j * 4 + 0] * ds + bv.x; v[j][1] = acc[mb][row][j * 4 + 1] * ds + bv.y;
                    v[j][2] = acc[mb][row][j * 4 + 2] * ds + bv.z; v[j][3] = acc[mb][row][j * 4 + 3] * ds + bv.w;
                    if (RES >= 1) {
                        const half4 rh = *(const half4*)run_hi(j), rl = *(const half4*)run_lo(j);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[j][r] = ((float)rh[r] + (float)rl[r]) * SPLIT_RX + v[j][r];
                    }
                }
                if (RES >= 2) {                             // second residual through the same strip (LDS operations of a wave execute in order)
#pragma unroll
                    for (int i = 0; i < 4; ++i) *(u32x4*)(strip + pstrip[i]) = rres2[h2][i];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const half4 rh = *(const half4*)run_hi(j), rl = *(const half4*)run_lo(j);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[j][r] = v[j][r] + ((float)rh[r] + (float)rl[r]) * SPLIT_RX;
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (a.post_act == 1) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[j][r] = v[j][r] > 0.f ? v[j][r] : 0.f;
                    }
                    split_store4x(run_hi(j), run_lo(j), v[j][0], v[j][1], v[j][2], v[j][3]);
                    vmax = split_absmax4(vmax, v[j][0], v[j][1], v[j][2], v[j][3]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    __builtin_amdgcn_raw_buffer_store_b128(*(const u32x4*)(strip + pstrip[i]), yrs, (EAGLE_ABL_M32 >= 5 && EAGLE_ABL_M32 <= 7) ? OOB : piece_off(pass, i, a.ycs, a.yoff), 0, EAGLE_M32_SAUX & 3);
            }
        }
        split_report(a.sat, n, vmax);
    }
}

#endif
