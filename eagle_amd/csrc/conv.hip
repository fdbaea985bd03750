// Implicit-GEMM convolution for gfx950 (CDNA4), NHWC, BatchNorm pre-folded, fused epilogue.
//
// Replaces nn.Conv2d + BatchNorm2d + ReLU (+ residual) of the reference's HRNet (eagle/models/keypoint_hrnet.py:65-137,
// 215-278, 353-391, 553-558) and ultralytics' Conv/Bottleneck.
//
// GEMM view:  D[Cout x pixels] = W[Cout x K] * X[K x pixels],  K = ks*ks*Cin.
//   * weights are the MFMA "A" operand, activations the "B" operand, so each lane ends up holding 4 CONSECUTIVE
//     output channels of one pixel -> 8-byte (fp16) / 16-byte (fp32) NHWC stores and residual loads.
//   * a workgroup (4 waves) owns a (16/wx) x (16*wx) output-pixel tile and BN = 16*NT output channels; each wave
//     owns 4 sub-tiles of 16 consecutive pixels.  The input halo tile and the weight slice of one Cin-chunk (KC
//     channels) are staged in LDS; pixel stride in LDS is padded so ds_read_b128 over 16 pixels is conflict-free.
//   * fp16 family: v_mfma_f32_16x16x32_f16, K flattened over (tap, 8-channel group); fp32 accumulate.
//   * fp32 family: v_mfma_f32_16x16x4_f32 in the canonical K order (16-channel chunk, tap, channel): gfx950
//     accumulates these as a k-ordered fmaf chain, so outputs are bit-identical to oracle/eo_prims.c.
// Epilogue: v = acc + bias; v = pre(v); v = r1 + v; v = v + r2; v = post(v); store (fp16 RNE / fp32).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>

#include "common.h"
#include "dmath.h"
#include "conv_internal.h"

namespace eagle {

// ------------------------------------------------------------------------------------------------------------
// host side: form table, geometry, choice, weight tiling
// ------------------------------------------------------------------------------------------------------------
static int f16_ps(int kc) { const int g = kc / 8; return kc * 2 + ((g % 2 == 0) ? 16 : 0); }
static int f16_ni(int ks, int kc) { return (ks * ks * (kc / 8) + 3) / 4; }

// Every kernel form the library instantiates, keyed by (family, ConvConfig::variant): the ids are those of the tuned tables, tools/autotune_*.py and the
// parity tests' EAGLE_CONV_FORCE strings.  Generic and weight-stationary forms have one instance per (ks, stride, kc, nt) in conv_inst_*.hip; an A-direct
// form is one kernel (per residual count and ring depth) for 3x3 layers of the row's stride, kc and nt.
enum FormKind { GENERIC, WSTAT, ADIRECT };                  // implicit GEMM; weight-stationary persistent; A-direct (weights straight into MFMA registers)
enum StrideForm { S1, S2D, S2T, S1L };                      // A-direct: stride 1; stride 2 over the space-to-depth image; TRUE stride 2 on a column-plane halo;
                                                            // stride 1 tiled over the linear pixel sequence of a map exactly `cols` wide (rows + 2 = the halo's map rows)
enum WeightImage { W_F32, W_F16, W_F16_S2D, W_SPLIT, W_SPLIT_AD, W_SPLIT_S2D, W_SPLIT_M32 };    // layout written by conv_tile_weights
struct Form {
    int prec, variant, kind;
    int pw;                  // generic / weight-stationary: 16-pixel sub-tiles per wave (tile = 4 pw / wx rows x 16 wx columns)
    int sform, rows, cols;   // A-direct: stride handling and output tile
    int kc, nt, halo_bufs;   // A-direct: the instance's chunk and Cout tiles (BN = 16 nt); halo buffers in LDS
    int wimage;
    int grid_cap;            // A-direct: at most this many workgroups per launch (0: one per item)
    ConvKernelGetter get;    // A-direct
};
static constexpr Form gen(int prec, int variant, int pw, int wimage, int kind = GENERIC) { return {prec, variant, kind, pw, S1, 0, 0, 0, 0, 0, wimage, 0, nullptr}; }
static constexpr Form ad(int prec, int variant, int sform, int rows, int cols, int nt, int halo_bufs, int wimage, ConvKernelGetter get, int grid_cap = 0)
{
    return {prec, variant, ADIRECT, 0, sform, rows, cols, prec == EAGLE_PREC_F16 ? 32 : 16, nt, halo_bufs, wimage, grid_cap, get};
}
static constexpr int F16 = EAGLE_PREC_F16, F32 = EAGLE_PREC_F32, F32S = EAGLE_PREC_F32S;
static constexpr Form g_forms[] = {
    // exact fp32 family: full (0), half (3) and quarter (4) tiles
    gen(F32, 0, 4, W_F32), gen(F32, 3, 2, W_F32), gen(F32, 4, 1, W_F32),
    // fp16: register-staged full tiles (0), chunk-pipelined staging (2), half (3) and quarter (4) tiles; weight-stationary 3x3 kernels, kc = Cin (6: 4 sub-tiles per wave, 7: 2)
    gen(F16, 0, 4, W_F16), gen(F16, 2, 4, W_F16), gen(F16, 3, 2, W_F16), gen(F16, 4, 1, W_F16), gen(F16, 6, 4, W_F16, WSTAT), gen(F16, 7, 2, W_F16, WSTAT),
    // fp16 A-direct (conv_ad_kernel.inc), kc = 32: BN 192, tile 4 x 32 (8) / BN 96, tile 8 x 32 (9); the same for stride 2 (10 / 11)
    ad(F16, 8, S1, 4, 32, 12, 2, W_F16, conv_ad_kernel_s1_bn192), ad(F16, 9, S1, 8, 32, 6, 2, W_F16, conv_ad_kernel_s1_bn96),
    ad(F16, 10, S2D, 4, 32, 12, 2, W_F16_S2D, conv_ad_kernel_s2_bn192), ad(F16, 11, S2D, 8, 32, 6, 2, W_F16_S2D, conv_ad_kernel_s2_bn96),
    // split family, generic kernel: full (0) and half (3) tiles, 8 x 48 tiles (18: six sub-tiles per wave, wx = 3)
    gen(F32S, 0, 4, W_SPLIT), gen(F32S, 3, 2, W_SPLIT), gen(F32S, 18, 6, W_SPLIT),
    // split family, A-direct on 16x16x32 MFMA (conv_ad_split.inc), chunks of 16 logical channels: stride 1 (8 / 9), space-to-depth stride 2 (10 / 11)
    ad(F32S, 8, S1, 4, 32, 12, 2, W_SPLIT_AD, conv_ad_split_kernel_bn192), ad(F32S, 9, S1, 8, 32, 6, 2, W_SPLIT_AD, conv_ad_split_kernel_bn96),
    ad(F32S, 10, S2D, 4, 32, 12, 2, W_SPLIT_S2D, conv_ad_split_kernel_s2_bn192), ad(F32S, 11, S2D, 8, 32, 6, 2, W_SPLIT_S2D, conv_ad_split_kernel_s2_bn96),
    // ... Cout = 48: tile 8 x 32 with the K dimension split over wave pairs (12); 16 x 32 with one halo buffer (13); 16 x 32 with the two-deep halo ring, whose
    // 130 KB of LDS leave one workgroup per CU: persistent, so that the ring's prefetch runs on from item to item (19)
    ad(F32S, 12, S1, 8, 32, 3, 2, W_SPLIT_AD, conv_ad_split_kernel48), ad(F32S, 13, S1, 16, 32, 3, 1, W_SPLIT_AD, conv_ad_split_kernel48sb),
    ad(F32S, 19, S1, 16, 32, 3, 2, W_SPLIT_AD, conv_ad_split_kernel48ring, 256),
    // ... TRUE stride 2 on an even / odd column-plane halo with the stride-1 weight image, one halo buffer: BN 192 (14); BN 96, K split over wave pairs (15)
    ad(F32S, 14, S2T, 4, 32, 12, 1, W_SPLIT_AD, conv_ad_split_kernel_s2t_bn192), ad(F32S, 15, S2T, 4, 32, 6, 1, W_SPLIT_AD, conv_ad_split_kernel_s2t_bn96),
    // split family, A-direct on 32x32x16 MFMA (conv_ad_split32.inc): tiles 4 x 32 (21) / 8 x 32 (22); the wave's two pixel blocks side by side (23 / 24)
    ad(F32S, 21, S1, 4, 32, 12, 2, W_SPLIT_M32, conv_ad_split32_kernel_bn192), ad(F32S, 22, S1, 8, 32, 6, 2, W_SPLIT_M32, conv_ad_split32_kernel_bn96),
    ad(F32S, 23, S1, 2, 64, 12, 2, W_SPLIT_M32, conv_ad_split32_kernel_w64_bn192), ad(F32S, 24, S1, 4, 64, 6, 2, W_SPLIT_M32, conv_ad_split32_kernel_w64_bn96),
    // ... BN 192 with items of 128 consecutive pixels of the row-major sequence, for maps exactly 30 columns wide: halo of 8 map rows x 32 records (27)
    ad(F32S, 27, S1L, 6, 30, 12, 2, W_SPLIT_M32, conv_ad_split32_kernel_lin30)};
static constexpr int LIN_PIXELS = 128;                      // pixels per item of the S1L forms

static const Form* find_form(int precision, int variant)
{
    for (const Form& f : g_forms)
        if (f.prec == precision && f.variant == variant) return &f;
    return nullptr;
}
static const Form& form_of(int precision, const ConvConfig& c)
{
    const Form* f = find_form(precision, c.variant);
    if (!f) fail(EAGLE_E_NOKERNEL, "no conv kernel form: prec=%d variant=%d", precision, c.variant);
    return *f;
}
static int kind_of(int precision, const ConvConfig& c) { const Form* f = find_form(precision, c.variant); return f ? f->kind : -1; }

static size_t lds_bytes(int precision, const ConvConfig& c)
{
    const Form& f = form_of(precision, c);
    if (f.kind == ADIRECT) {                                // halo buffers of 1-KiB slabs (a multiple of four) + the output strips
        int hpix, rec, strips;
        if (precision == EAGLE_PREC_F16) { hpix = f.sform == S2D ? (f.rows + 1) * 33 : (f.rows + 2) * 34; rec = 96; strips = 4 * 32 * 112; }
        else if (f.wimage == W_SPLIT_M32) { hpix = (f.rows + 2) * (f.cols + 2); rec = 80; strips = 4 * 32 * 128; }      // 80-byte halo records; strips of 32 pixels x 32 channels x 4 bytes, 128-byte records swizzled by the pixel
        else { hpix = f.sform == S2T ? (2 * f.rows + 1) * 66 : (f.rows + 2) * 34; rec = 96; strips = 4 * 16 * 208; }   // 16 logical channels = the 96-byte record (S2T: 2 rows + 1 x (33 even + 33 odd columns)); strips of 16 pixels x 48 channels x 4 bytes
        const int slabs = ((hpix * rec + 1023) / 1024 + 3) / 4 * 4;
        return (size_t)f.halo_bufs * slabs * 1024 + strips;
    }
    const int th = 4 * f.pw / c.wx, tw = 16 * c.wx;
    const int hw = (tw - 1) * c.stride + c.ks, hh = (th - 1) * c.stride + c.ks;
    const int bn = c.nt * 16;
    if (precision == EAGLE_PREC_F16) {
        const size_t operands = (size_t)f16_ni(c.ks, c.kc) * 4 * bn * 16 + (size_t)hh * hw * f16_ps(c.kc);
        const size_t strips = (size_t)4 * f.pw * 16 * (bn * 2 + 16);        // output transpose, one strip per wave
        return f.kind == WSTAT ? operands + strips + 16 : std::max(operands + 16, strips);
    }
    if (precision == EAGLE_PREC_F32S) {                    // hi and lo fragment blocks per K-step; 2 * kc fp16 values per staged pixel; 4-byte outputs
        const size_t operands = (size_t)f16_ni(c.ks, c.kc) * 2 * 4 * bn * 16 + (size_t)hh * hw * f16_ps(2 * c.kc);
        const size_t strips = (size_t)4 * f.pw * 16 * (bn * 4 + 16);
        return std::max(operands + 16, strips);
    }
    return (size_t)c.ks * c.ks * (c.kc / 4) * 4 * bn * 4 + (size_t)hh * hw * (c.kc + 1) * 4;
}

size_t conv_lds_bytes(int precision, const ConvConfig& c) { return lds_bytes(precision, c); }
void conv_tile_shape(int precision, const ConvConfig& c, int* th, int* tw)
{
    const Form& f = form_of(precision, c);
    *th = f.kind == ADIRECT ? f.rows : 4 * f.pw / c.wx; *tw = f.kind == ADIRECT ? f.cols : 16 * c.wx;
}

int conv_tiles_per_frame(int precision, const ConvConfig& c, int ho, int wo)
{
    int th, tw;
    conv_tile_shape(precision, c, &th, &tw);
    if (form_of(precision, c).sform == S1L) return (ho * wo + LIN_PIXELS - 1) / LIN_PIXELS;
    return ((wo + tw - 1) / tw) * ((ho + th - 1) / th);
}

// The generic instances live in conv_inst_0..3.hip / conv_inst_s0..2.hip so that a clean build compiles them in parallel; the A-direct kernels in
// conv_ad_s1.hip / conv_ad_s2.hip / conv_ad_split.hip / conv_ad_split32.hip.
static const Inst* generic_inst(int precision, const ConvConfig& c)
{
    for (auto part : {conv_inst_part0, conv_inst_part1, conv_inst_part2, conv_inst_part3, conv_inst_split0, conv_inst_split1, conv_inst_split2}) {
        int n = 0;
        const Inst* t = part(&n);
        for (int k = 0; k < n; ++k)
            if (t[k].prec == precision && t[k].ks == c.ks && t[k].s == c.stride && t[k].kc == c.kc && t[k].nt == c.nt && t[k].variant == c.variant) return &t[k];
    }
    return nullptr;
}
bool conv_supported(int precision, const ConvConfig& c)
{
    const Form* f = find_form(precision, c.variant);
    if (f && f->kind == ADIRECT) return c.ks == 3 && c.stride == (f->sform == S1 || f->sform == S1L ? 1 : 2) && c.kc == f->kc && c.nt == f->nt;
    return f && generic_inst(precision, c);
}

struct Tuned { int ks, s, cin, cout, wo, kc, nt, wx, variant; };
static const Tuned g_tuned[] = {
#include "conv_tuned.inc"
    {0, 0, 0, 0, 0, 0, 0, 0, 0}};
static const Tuned g_tuned_f32[] = {         // EAGLE_PREC_F32: tile shape only (nt, wx); the summation order, hence every bit, is the same for all rows
#include "conv_tuned_f32.inc"
    {0, 0, 0, 0, 0, 0, 0, 0, 0}};
static const Tuned g_tuned_split[] = {       // EAGLE_PREC_F32S (tools/autotune_split.py); rows of one shape are ordered best first
#include "conv_tuned_split.inc"
    {0, 0, 0, 0, 0, 0, 0, 0, 0}};
static bool tuned_match(const Tuned& t, const ConvConfig& c, int wo, ConvConfig* q)
{
    if (t.ks != c.ks || t.s != c.stride || t.cin != c.cin || t.cout != c.cout_pad || t.wo != wo) return false;
    *q = c; q->kc = t.kc; q->nt = t.nt; q->wx = t.wx; q->variant = t.variant;
    return true;
}

// The developer switches, read on every call (the parity tests set them between calls):
//   EAGLE_CONV_FORCE="kc,nt,variant" (fp16 and split families) / EAGLE_F32_FORCE="nt,wx,variant" (exact family): this form for every layer it is valid for;
//   EAGLE_CONV_M32=0: the split family's 3x3 stride-1 layers with Cout = 96 k on the 16x16x32 A-direct forms instead of the 32x32x16 ones;
//   EAGLE_F32_STACK=0: no row stacking in the exact family (conv_launch).
static bool env_force(const char* name, int* a, int* b, int* c) { const char* f = getenv(name); return f && sscanf(f, "%d,%d,%d", a, b, c) == 3; }
static bool env_off(const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; }

static const int g_nts[] = {6, 4, 3, 2, 1};
static ConvConfig with_ad(ConvConfig c, int kc, int v192, int v96)      // an A-direct form: BN = 192 where Cout allows it, else BN = 96
{
    c.kc = kc;
    if (c.cout_pad % 192 == 0) { c.nt = 12; c.variant = v192; } else { c.nt = 6; c.variant = v96; }
    return c;
}

static ConvConfig choose_f32(ConvConfig c, int wo)
{
    ConvConfig q = c; q.kc = (c.cin < 16) ? 4 : 16;          // parity tests of the tilings (every tiling gives the same bits)
    if (env_force("EAGLE_F32_FORCE", &q.nt, &q.wx, &q.variant) && (q.wx == 1 || q.wx == 2) && q.nt >= 1 && c.cout_pad % (16 * q.nt) == 0 &&
        conv_supported(EAGLE_PREC_F32, q) && lds_bytes(EAGLE_PREC_F32, q) <= 160 * 1024)
        return q;
    for (const Tuned& t : g_tuned_f32)                       // variant: 0 full, 3 half, 4 quarter tiles
        if (tuned_match(t, c, wo, &q) && conv_supported(EAGLE_PREC_F32, q)) return q;
    c.nt = 1;
    for (int nt : g_nts)
        if (c.cout_pad % (16 * nt) == 0) { c.nt = nt; break; }
    c.kc = (c.cin < 16) ? 4 : 16;
    if (c.stride == 2 && c.ks == 3) {                       // the halo of a stride-2 tile is four times the tile: half tiles keep two workgroups on a CU
        q = c; q.variant = 3;
        if (conv_supported(EAGLE_PREC_F32, q)) return q;
    }
    return c;
}

static ConvConfig choose_split(ConvConfig c, int wo, bool plain_epilogue)
{
    const int prec = EAGLE_PREC_F32S, cin = c.cin, cout = c.cout_pad;
    ConvConfig q = c;
    if (env_force("EAGLE_CONV_FORCE", &q.kc, &q.nt, &q.variant) && cin % q.kc == 0 && cout % (16 * q.nt) == 0 && conv_supported(prec, q) &&
        (form_of(prec, q).sform != S1L || (plain_epilogue && wo == form_of(prec, q).cols))) {      // a linear form is compiled for one map width
        if (form_of(prec, q).pw == 6) q.wx = 3;              // six sub-tiles per wave: the 8 x 48 tile
        if (lds_bytes(prec, q) <= 160 * 1024) return q;
    }
    // 3x3 stride 2 with Cin = 48 k, Cout = 96 k (HRNet's transition / fuse down-sampling chains): the TRUE stride-2 A-direct forms.  Same box, all
    // instances per layer (tools/convbench/split_tune, B = 50, best other form -> this one): 96->192 145 -> 108 us, 48->192 80 -> 62, 192->384
    // 139 -> 102, 96->384 76 -> 55, 48->384 45 -> 33 (variant 14); 48->96 203 -> 175, 96->96 88 -> 70 (variant 15).
    if (plain_epilogue && c.ks == 3 && c.stride == 2 && cin % 48 == 0 && cout % 96 == 0) return with_ad(c, 16, 14, 15);
    // 3x3 stride 1 with Cout = 96 k, any Cin = 16 k: the 32x32x16 A-direct forms (round 5), 4 x 32 tiles for BN = 192 (2 x 64 measured 1.5 % slower on 34 x 60),
    // 4 x 64 tiles for BN = 96 on maps wider than 32 columns, else 8 x 32 — same box, three alternating pairs through the whole pipeline against the 16x16x32
    // forms: 750.0 / 751.0 / 753.4 -> 761.3 / 761.5 / 761.8 frames/s (+1.4 %), 96->96 @68x120 208.5 -> 193.5 us.
    // BN = 192 on maps exactly 30 columns wide (HRNet's 17 x 30 branch): items of 128 consecutive pixels of the row-major sequence (variant 27) instead of
    // 4 x 32 rectangles, 16 instead of 20 32-pixel blocks per frame at the same halo traffic — same box, four alternating runs through the whole pipeline:
    // 828.7 ... 834.3 -> 839.4 ... 845.2 frames/s (+1.2 %), 384->384 @17x30 222 -> 177 us isolated (docs/experiments.md 10.11).  The same form at 60 columns
    // (34 x 60: 72 -> 64 blocks, but a halo of 372 records per item instead of 204) ran 5 % SLOWER per launch and gave a mixed +0.5 % in the pipeline: measured
    // and taken out again, 34 x 60 stays on variant 21.  The 96-channel class stays on the 4 x 64 tile: a full-width halo for its 256 pixels at W = 120
    // (120 KB) leaves one workgroup per CU, and its padding is 6.7 % only.
    if (!env_off("EAGLE_CONV_M32") && plain_epilogue && c.ks == 3 && c.stride == 1 && cin % 16 == 0 && cout % 96 == 0) {
        q = with_ad(c, 16, 21, wo > 32 ? 24 : 22);
        if (q.variant == 21 && wo == 30) q.variant = 27;
        return q;
    }
    for (const Tuned& t : g_tuned_split)
        if (tuned_match(t, c, wo, &q)) {
            const Form* f = find_form(prec, q.variant);      // the A-direct kernels: ReLU / none after at most two residual adds, three chunks per loop body
            if (kind_of(prec, q) == ADIRECT && !(plain_epilogue && cin % (f->sform == S2D ? 16 : 48) == 0)) continue;
            if (conv_supported(prec, q) && lds_bytes(prec, q) <= 160 * 1024) return q;
        }
    if (plain_epilogue && c.ks == 3 && c.stride == 1 && cin % 48 == 0 && cout % 96 == 0) return with_ad(c, 16, 8, 9);      // A-direct, split form (three 16-channel chunks per loop body)
    // generic kernel, full (variant 0) or half (variant 3) tiles: the (NT, KC) pair with the most MFMA work per staged byte whose LDS footprint lets two
    // workgroups share a CU
    static const int skcs[] = {32, 16, 8};
    long best = -1;
    c.nt = 1; c.kc = 8; c.variant = 0;
    for (int variant : {0, 3})
        for (int nt : g_nts) {
            if (cout % (16 * nt)) continue;
            for (int kc : skcs) {
                if (cin % kc) continue;
                ConvConfig t = c; t.nt = nt; t.kc = kc; t.variant = variant;
                if (!conv_supported(prec, t)) continue;
                if (lds_bytes(prec, t) > 80 * 1024) continue;
                const int pw = form_of(prec, t).pw;
                if (nt * pw > 12) continue;                        // registers: 4 accumulator VGPRs per (NT, PW) pair next to twice the fragments of the fp16 kernel
                const long score = (long)nt * pw * 1000 + kc * 10 + (variant == 0 ? 1 : 0);
                if (score > best) { best = score; c.nt = nt; c.kc = kc; c.variant = variant; }
            }
        }
    return c;
}

static ConvConfig choose_f16(ConvConfig c, int wo, bool plain_epilogue, bool plain_one)
{
    const int prec = EAGLE_PREC_F16, cin = c.cin, cout = c.cout_pad;
    ConvConfig q = c;
    if (env_force("EAGLE_CONV_FORCE", &q.kc, &q.nt, &q.variant) && cin % q.kc == 0 && cout % (16 * q.nt) == 0 && conv_supported(prec, q) &&
        lds_bytes(prec, q) <= 160 * 1024 && (kind_of(prec, q) == WSTAT ? plain_one : kind_of(prec, q) == ADIRECT ? plain_epilogue : true))
        return q;
    // 3x3 stride-1 layers whose Cout is a multiple of 96 (HRNet's 96 / 192 / 384-channel branches): the A-direct kernel
    if (plain_epilogue && c.ks == 3 && c.stride == 1 && cin % 32 == 0 && cout % 96 == 0) return with_ad(c, 32, 8, 9);
    // 3x3 stride-2 layers with the same Cout: the A-direct kernel over the space-to-depth image
    if (plain_epilogue && c.ks == 3 && c.stride == 2 && cin % 8 == 0 && cin >= 32 && cout % 96 == 0) return with_ad(c, 32, 10, 11);
    // per-layer table measured on MI355X (tools/autotune_conv.py); shapes not in the table use the heuristic below
    for (const Tuned& t : g_tuned)
        if (tuned_match(t, c, wo, &q)) {
            if (kind_of(prec, q) == WSTAT && !plain_one) continue;   // the weight-stationary kernel has no SiLU / second-residual / fp32-output epilogue
            if (conv_supported(prec, q) && lds_bytes(prec, q) <= 160 * 1024) return q;
        }
    // heuristic: the (NT, KC) pair with the most work per staged item whose LDS footprint still lets two workgroups share a CU
    static const int kcs[] = {64, 48, 32, 16, 8};
    long best = -1;
    c.nt = 1; c.kc = 8;
    for (int nt : g_nts) {
        if (cout % (16 * nt)) continue;
        for (int kc : kcs) {
            if (cin % kc) continue;
            ConvConfig t = c; t.nt = nt; t.kc = kc;
            if (!conv_supported(prec, t)) continue;
            if (lds_bytes(prec, t) > 80 * 1024) continue;
            const long score = (long)kc * nt * 1000 + kc;
            if (score > best) { best = score; c.nt = nt; c.kc = kc; }
        }
    }
    return c;
}

ConvConfig conv_choose(int precision, int ks, int stride, int cin_pad, int cout_pad, int wo, bool plain_epilogue, bool second_residual)
{
    // plain_epilogue: no activation before the residual adds, none / ReLU after them, fp16 output.  The weight-stationary kernels also need
    // at most one residual; the A-direct kernels take two.
    ConvConfig c;
    c.ks = ks; c.stride = stride; c.cin = cin_pad; c.cout_pad = cout_pad;
    c.wx = (wo > 16) ? 2 : 1;
    if (precision == EAGLE_PREC_F32) return choose_f32(c, wo);
    if (precision == EAGLE_PREC_F32S) return choose_split(c, wo, plain_epilogue);
    return choose_f16(c, wo, plain_epilogue, plain_epilogue && !second_residual);
}

// The tables the choice above is made from, for the tests (eagle_op_conv_table; host only).  Rows beyond `cap` ints are counted, not written.
int conv_table(int which, int32_t* rows, int cap)
{
    int n = 0, used = 0;
    auto put = [&](std::initializer_list<int> r) {
        if (rows && used + (int)r.size() <= cap)
            for (int v : r) rows[used++] = v;
        ++n;
    };
    if (which == EAGLE_CONV_TABLE_INSTANCES) {
        for (auto part : {conv_inst_part0, conv_inst_part1, conv_inst_part2, conv_inst_part3, conv_inst_split0, conv_inst_split1, conv_inst_split2}) {
            int k = 0;
            const Inst* t = part(&k);
            for (int i = 0; i < k; ++i) put({t[i].prec, t[i].ks, t[i].s, t[i].kc, t[i].nt, t[i].variant});
        }
        return n;
    }
    if (which == EAGLE_CONV_TABLE_ADIRECT) {
        for (const Form& f : g_forms)
            if (f.kind == ADIRECT) {
                ConvConfig c;
                c.ks = 3; c.stride = (f.sform == S1 || f.sform == S1L) ? 1 : 2; c.kc = f.kc; c.nt = f.nt; c.variant = f.variant;
                put({f.prec, f.variant, c.stride, f.kc, f.nt, f.rows, f.cols, (int)lds_bytes(f.prec, c)});
            }
        return n;
    }
    const Tuned* t = which == EAGLE_CONV_TABLE_TUNED_F16 ? g_tuned : which == EAGLE_CONV_TABLE_TUNED_F32 ? g_tuned_f32 : which == EAGLE_CONV_TABLE_TUNED_SPLIT ? g_tuned_split : nullptr;
    if (!t) fail(EAGLE_E_INVALID, "conv_table: no table %d", which);
    for (; t->ks; ++t) put({t->ks, t->s, t->cin, t->cout, t->wo, t->kc, t->nt, t->wx, t->variant});      // (the terminator row is all zeros)
    return n;
}

size_t conv_weight_elems(int precision, const ConvConfig& c)
{
    const int bn = c.nt * 16, nblk = c.cout_pad / bn, nch = c.cin / c.kc;
    switch (form_of(precision, c).wimage) {
    case W_F16_S2D: return (size_t)nblk * (4 * c.cin / 32) * 16 * bn * 8;
    case W_F16: return (size_t)nblk * nch * f16_ni(c.ks, c.kc) * 4 * bn * 8;
    case W_SPLIT_S2D: return (size_t)nblk * (4 * c.cin / 16) * 6 * 4 * bn * 8;      // 6 K-steps per 16-channel chunk of the space-to-depth image
    case W_SPLIT_M32: return (size_t)nblk * (c.cin / 16) * 18 * (bn / 32) * 512;    // 18 steps (tap, hi | lo) per 16-channel chunk, one 1-KiB fragment per 32 output channels
    case W_SPLIT_AD: return (size_t)nblk * (c.cin / 16) * 14 * 4 * bn * 8;          // 14 K-steps per 16-channel chunk
    case W_SPLIT: return (size_t)nblk * nch * f16_ni(c.ks, c.kc) * 2 * 4 * bn * 8;  // fp16 elements: a hi and a lo block per K-step
    default: return (size_t)nblk * nch * c.ks * c.ks * (c.kc / 4) * 4 * bn;
    }
}

void conv_tile_weights(int precision, const ConvConfig& c, const float* w, int cin_real, int cout_real, void* dst, float* descale)
{
    const int bn = c.nt * 16, nblk = c.cout_pad / bn, nch = c.cin / c.kc, taps = c.ks * c.ks, wimage = form_of(precision, c).wimage;
    auto W = [&](int tap, int ci, int co) -> float {
        return (ci < cin_real && co < cout_real) ? w[((size_t)tap * cin_real + ci) * cout_real + co] : 0.0f;
    };
    if (descale) *descale = 1.0f;
    if (precision == EAGLE_PREC_F32S) {
        // [Cout block][Cin chunk][K-step][hi | lo][q][BN][8]; K-step i, lane group q: (tap, channel group) pair 4 i + q in (tap-major) order
        float amax = 0.f;
        for (size_t k = 0; k < (size_t)taps * cin_real * cout_real; ++k) amax = std::max(amax, std::fabs(w[k]));
        int e = 0;
        if (amax > 0.f) (void)std::frexp(amax, &e);                        // amax in [2^(e-1), 2^e)
        const int sw = 15 - e;                                             // scaled maximum in [2^14, 2^15)
        const float scale = std::ldexp(1.0f, sw);
        if (descale) *descale = std::ldexp(1.0f, -(sw + 4));
        _Float16* d = (_Float16*)dst;
        if (wimage == W_SPLIT_S2D) {
            // stride 2: [Cout block][s2d chunk][K-step 0..5][q][BN][8].  s2d chunk -> (phase (ry, rx), 16 real channels); K-steps 0..3 = the taps' (tyy, txx)
            // of the 2x2 kernel over the space-to-depth image, lane groups (hi g0, hi g1, hi g0, hi g1); K-steps 4, 5 = the tap' pairs (0|1), (2|3), lane
            // groups (lo g0, lo g1 | lo g0, lo g1).  tap' row 0 is the s2d row above: only its odd phase contributes (ky = 0); row 1: ky = 1 (even phase), 2 (odd).
            const int per_phase = c.cin / 16;
            for (int b = 0; b < nblk; ++b)
                for (int ch = 0; ch < 4 * per_phase; ++ch)
                    for (int k = 0; k < 6; ++k)
                        for (int qq = 0; qq < 4; ++qq)
                            for (int nn = 0; nn < bn; ++nn)
                                for (int j = 0; j < 8; ++j) {
                                    const int ph = ch / per_phase, c0 = (ch - ph * per_phase) * 16, ry = ph >> 1, rx = ph & 1;
                                    const int tp = k < 4 ? k : 2 * (k - 4) + (qq >> 1), tyy = tp >> 1, txx = tp & 1;
                                    const int ky = tyy == 0 ? (ry == 1 ? 0 : -1) : (ry == 0 ? 1 : 2), kx = txx == 0 ? (rx == 1 ? 0 : -1) : (rx == 0 ? 1 : 2);
                                    float v = 0.f;
                                    if (ky >= 0 && kx >= 0) v = W(ky * 3 + kx, c0 + (qq & 1) * 8 + j, b * bn + nn) * scale;
                                    const _Float16 hi = (_Float16)v;
                                    *d++ = k < 4 ? hi : (_Float16)(v - (float)hi);
                                }
            return;
        }
        if (wimage == W_SPLIT_M32) {
            // 32x32x16 form: [Cout block][16-channel chunk][tap 0..8][hi | lo][BN / 32 blocks][lane 0..63][8]: lane l of a block's A fragment holds output
            // channel (l & 31) of the block and the chunk's 8-channel group (l >> 5)
            for (int b = 0; b < nblk; ++b)
                for (int ch = 0; ch < c.cin / 16; ++ch)
                    for (int tap = 0; tap < 9; ++tap)
                        for (int part = 0; part < 2; ++part)
                            for (int mb = 0; mb < bn / 32; ++mb)
                                for (int l = 0; l < 64; ++l)
                                    for (int j = 0; j < 8; ++j) {
                                        const float v = W(tap, ch * 16 + (l >> 5) * 8 + j, b * bn + mb * 32 + (l & 31)) * scale;
                                        const _Float16 hi = (_Float16)v;
                                        *d++ = part == 0 ? hi : (_Float16)(v - (float)hi);
                                    }
            return;
        }
        if (wimage == W_SPLIT_AD) {
            // A-direct form: [Cout block][16-channel chunk][K-step 0..13][q][BN][8].  K-steps 0..8 = taps, lane groups (hi g0, hi g1, hi g0, hi g1):
            // against the record slots (hi g0, hi g1, lo g0, lo g1) that is hi*hi + hi*lo.  K-steps 9..13 = tap pairs (0|1, 2|3, 4|5, 6|7, 8|-),
            // lane groups (lo g0, lo g1 at the first tap | lo g0, lo g1 at the second): lo*hi.
            for (int b = 0; b < nblk; ++b)
                for (int ch = 0; ch < c.cin / 16; ++ch)
                    for (int k = 0; k < 14; ++k)
                        for (int qq = 0; qq < 4; ++qq)
                            for (int nn = 0; nn < bn; ++nn)
                                for (int j = 0; j < 8; ++j) {
                                    const int tap = k < 9 ? k : 2 * (k - 9) + (qq >> 1);
                                    float v = 0.f;
                                    if (tap < 9) v = W(tap, ch * 16 + (qq & 1) * 8 + j, b * bn + nn) * scale;
                                    const _Float16 hi = (_Float16)v;
                                    *d++ = k < 9 ? hi : (_Float16)(v - (float)hi);
                                }
            return;
        }
        const int G = c.kc / 8, NGR = taps * G, NI = f16_ni(c.ks, c.kc);
        for (int b = 0; b < nblk; ++b)
            for (int ch = 0; ch < nch; ++ch)
                for (int i = 0; i < NI; ++i)
                    for (int part = 0; part < 2; ++part)
                        for (int qq = 0; qq < 4; ++qq)
                            for (int nn = 0; nn < bn; ++nn)
                                for (int j = 0; j < 8; ++j) {
                                    const int g = 4 * i + qq;
                                    float v = 0.f;
                                    if (g < NGR) { const int tap = g / G, cg = g % G; v = W(tap, ch * c.kc + cg * 8 + j, b * bn + nn) * scale; }
                                    const _Float16 hi = (_Float16)v;
                                    *d++ = part == 0 ? hi : (_Float16)(v - (float)hi);
                                }
        return;
    }
    if (wimage == W_F16_S2D) {
        // space-to-depth form: [Cout block][chunk of 32 s2d channels][tap' (2x2) * 4 + channel group][BN][8]; s2d channel = phase * Cin + channel,
        // phase = 2 * ry + rx; tap' row 0 is the s2d row above (only its odd phase contributes: ky = 0), tap' row 1 the same row (ky = 1, 2)
        _Float16* d = (_Float16*)dst;
        const int nch2 = 4 * c.cin / 32;
        for (int b = 0; b < nblk; ++b)
            for (int ch = 0; ch < nch2; ++ch)
                for (int g = 0; g < 16; ++g)
                    for (int nn = 0; nn < bn; ++nn)
                        for (int j = 0; j < 8; ++j) {
                            const int tp = g / 4, cg = g % 4, tyy = tp >> 1, txx = tp & 1;
                            const int sc = ch * 32 + cg * 8 + j, ph = sc / c.cin, ci = sc - ph * c.cin, ry = ph >> 1, rx = ph & 1;
                            const int ky = tyy == 0 ? (ry == 1 ? 0 : -1) : (ry == 0 ? 1 : 2), kx = txx == 0 ? (rx == 1 ? 0 : -1) : (rx == 0 ? 1 : 2);
                            *d++ = (_Float16)((ky < 0 || kx < 0) ? 0.f : W(ky * 3 + kx, ci, b * bn + nn));
                        }
        return;
    }
    if (precision == EAGLE_PREC_F16) {
        const int G = c.kc / 8, NGR = taps * G, NI = f16_ni(c.ks, c.kc);
        _Float16* d = (_Float16*)dst;
        for (int b = 0; b < nblk; ++b)
            for (int ch = 0; ch < nch; ++ch)
                for (int g = 0; g < NI * 4; ++g)
                    for (int nn = 0; nn < bn; ++nn)
                        for (int j = 0; j < 8; ++j) {
                            float v = 0.f;
                            if (g < NGR) {
                                const int tap = g / G, cg = g % G;
                                v = W(tap, ch * c.kc + cg * 8 + j, b * bn + nn);
                            }
                            *d++ = (_Float16)v;
                        }
    } else {
        const int CSTEPS = c.kc / 4;
        float* d = (float*)dst;
        for (int b = 0; b < nblk; ++b)
            for (int ch = 0; ch < nch; ++ch)
                for (int tap = 0; tap < taps; ++tap)
                    for (int cs = 0; cs < CSTEPS; ++cs)
                        for (int qq = 0; qq < 4; ++qq)
                            for (int nn = 0; nn < bn; ++nn) *d++ = W(tap, ch * c.kc + cs * 4 + qq, b * bn + nn);
    }
}

static std::mutex g_page_mutex;
static const void* conv_zero_page()
{
    static void* z[64] = {};
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(g_page_mutex);
    if (!z[dev]) { HIP_CHECK(hipMalloc(&z[dev], 256)); HIP_CHECK(hipMemset(z[dev], 0, 256)); HIP_CHECK(hipStreamSynchronize(nullptr)); }     // (read on non-blocking streams)
    return z[dev];
}
static void* conv_trash_page()
{
    static void* z[64] = {};
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(g_page_mutex);
    if (!z[dev]) HIP_CHECK(hipMalloc(&z[dev], 8192));
    return z[dev];
}

void conv_launch(int precision, const ConvLaunch& L, hipStream_t s)
{
    const ConvConfig& c = L.cfg;
    if (!conv_supported(precision, c)) fail(EAGLE_E_NOKERNEL, "no conv kernel instance: prec=%d ks=%d s=%d kc=%d nt=%d", precision, c.ks, c.stride, c.kc, c.nt);
    const Form& f = form_of(precision, c);
    ConvArgs a;
    a.x = L.x.p; a.xcs = L.x.cs; a.xoff = L.x.off; a.N = L.x.n; a.H = L.x.h; a.W = L.x.w;
    a.w = L.w; a.bias = L.bias;
    a.y = L.y.p; a.ycs = L.y.cs; a.yoff = L.y.off; a.Ho = L.y.h; a.Wo = L.y.w;
    a.r1 = L.r1.p; a.r1cs = L.r1.cs; a.r1off = L.r1.off;
    a.r2 = L.r2.p; a.r2cs = L.r2.cs; a.r2off = L.r2.off;
    a.descale = L.descale;
    if (precision == EAGLE_PREC_F32S) {                     // the kernels address split tensors in fp16 elements: two per logical channel
        if (L.x.f32 != 2 || (L.r1.p && L.r1.f32 != 2) || (L.r2.p && L.r2.f32 != 2) || L.y.f32 != (L.out_f32 ? 1 : 2))
            fail(EAGLE_E_INVALID, "split conv: operand tensor formats do not match the family");
        a.xcs *= 2; a.xoff *= 2; a.r1cs *= 2; a.r1off *= 2; a.r2cs *= 2; a.r2off *= 2;
        if (!L.out_f32) { a.ycs *= 2; a.yoff *= 2; }
    }
    if (!a.r1 && a.r2) { a.r1 = a.r2; a.r1cs = a.r2cs; a.r1off = a.r2off; a.r2 = nullptr; }       // a single residual is always operand 1 (IEEE addition is commutative: same bits)
    a.pre_act = L.pre_act; a.post_act = L.post_act; a.out_f32 = L.out_f32 || precision == EAGLE_PREC_F32;
    a.wx = c.wx;
    a.nchunks = c.cin / c.kc;
    a.zeros = conv_zero_page(); a.trash = conv_trash_page(); a.xcd = 0; a.gy = 1; a.stack = 0;
    a.am = L.am_slot ? *L.am_slot : nullptr; a.am_cs = c.cout_pad;
    a.sat = (L.sat_slot && precision == EAGLE_PREC_F32S) ? *L.sat_slot : nullptr;
    if (f.kind == ADIRECT) {
        // the split forms with 14 K-steps per chunk take three chunks per loop body
        if (a.out_f32 || a.pre_act != 0 || a.post_act > 1 || L.am_slot || (precision == EAGLE_PREC_F32S && c.cin % (f.wimage == W_SPLIT_AD ? 48 : 16)))
            fail(EAGLE_E_NOKERNEL, "A-direct conv needs 2-byte / split output, pre_act none, post_act in {none, ReLU} and, in the split family, Cin = 16 k (48 k for variants 8, 9 and 12 - 15)");
        if (f.sform == S2D) a.nchunks = 4 * c.cin / c.kc;  // chunks of the space-to-depth image
        a.tiles_x = (a.Wo + f.cols - 1) / f.cols; a.tiles_y = (a.Ho + f.rows - 1) / f.rows;
        if (f.sform == S1L) {                               // items of LIN_PIXELS consecutive pixels: tiles_x = items per frame
            if (a.Wo != f.cols || a.W != a.Wo || a.H != a.Ho) fail(EAGLE_E_NOKERNEL, "linear A-direct conv (variant %d) needs a map %d columns wide, got %d x %d", c.variant, f.cols, a.Ho, a.Wo);
            a.tiles_x = (a.Ho * a.Wo + LIN_PIXELS - 1) / LIN_PIXELS; a.tiles_y = 1;
        }
        a.gy = c.cout_pad / (c.nt * 16);
        const size_t lim = (size_t)1 << 31;
        if ((size_t)a.N * a.H * a.W * a.xcs * 2 >= lim || (size_t)a.N * a.Ho * a.Wo * std::max(std::max(a.ycs, a.r1 ? a.r1cs : 0), a.r2 ? a.r2cs : 0) * 2 >= lim)
            fail(EAGLE_E_INVALID, "fp16 conv: a tensor of %d frames reaches 2 GiB; use a smaller device batch", a.N);
        const int nres = (a.r1 ? 1 : 0) + (a.r2 ? 1 : 0);
        const int items = a.tiles_x * a.tiles_y * a.N * a.gy;
        const bool deep = items <= 256;                     // at most one workgroup per CU: the deep weight ring (conv_ad_split32.hip)
        // the attributes of both ring depths: a graph captured at a new frame count may switch depth, and a capture sets no function attribute
        for (bool d : {false, true}) ensure_max_dynamic_lds((const void*)f.get(nres, d), 160 * 1024);
        // workgroups per launch: one per item (the hardware hands a queued workgroup to whichever CU frees a slot: dynamic balance) rather than 512
        // resident ones walking static item ranges — same box, alternating: 774.4 / 774.5 -> 779.0 / 780.7 frames/s, 96->96 209.9 -> 204.4 us,
        // 192->192 180.3 -> 177.2 (768 workgroups: 707 frames/s — 1.5 rounds of uneven ranges).  grid_cap: persistent forms (variant 19).
        hipLaunchKernelGGL(f.get(nres, deep), dim3(f.grid_cap ? std::min(items, f.grid_cap) : items), dim3(256), lds_bytes(precision, c), s, a);
        HIP_CHECK(hipGetLastError());
        return;
    }
    const int th = 4 * f.pw / c.wx, tw = 16 * c.wx;
    a.tiles_x = (a.Wo + tw - 1) / tw; a.tiles_y = (a.Ho + th - 1) / th;
    if (precision == EAGLE_PREC_F32) {
        // row stacking (conv_f32_kernel): stride-1 layers of a batch are tiled as one image of N (Ho + 1) rows
        if (!env_off("EAGLE_F32_STACK") && c.stride == 1 && a.N > 1 && a.Ho == a.H) { a.stack = 1; a.tiles_y = (a.N * (a.Ho + 1) + th - 1) / th; }
        // raw buffer descriptors with 32-bit byte offsets for the activation loads
        if ((size_t)a.N * a.H * a.W * a.xcs * 4 >= ((size_t)1 << 31)) fail(EAGLE_E_INVALID, "fp32 conv: the input tensor of %d frames reaches 2 GiB; use a smaller device batch", a.N);
    }
    const bool ws = f.kind == WSTAT;
    if (a.am && (!prec_is_f16_kernels(precision) || ws))
        fail(EAGLE_E_NOKERNEL, "fused heat-map maxima need the generic fp16 kernel");
    if (prec_is_f16_kernels(precision)) {                   // the fp16 kernels address tensors through raw buffer descriptors with 32-bit byte offsets
        const size_t lim = (size_t)1 << 31;
        const size_t cs_out = std::max(std::max(a.out_f32 ? 2 * a.ycs : a.ycs, a.r1 ? a.r1cs : 0), a.r2 ? a.r2cs : 0);
        if ((size_t)a.N * a.H * a.W * a.xcs * 2 >= lim || (size_t)a.N * a.Ho * a.Wo * cs_out * 2 >= lim)
            fail(EAGLE_E_INVALID, "fp16 conv: a tensor of %d frames reaches 2 GiB; use a smaller device batch", a.N);
    }
    const ConvKernel fn = generic_inst(precision, c)->fn;
    const size_t lds = lds_bytes(precision, c);
    ensure_max_dynamic_lds((const void*)fn, 160 * 1024);
    const int gy = c.cout_pad / (c.nt * 16);
    int gx = a.stack ? a.tiles_x * a.tiles_y : a.tiles_x * a.tiles_y * a.N;
    if (ws) {                                               // persistent, weight-stationary: 8*gy | grid, up to two workgroups per CU
        if (c.kc != c.cin || a.out_f32 || a.r2 || a.pre_act != 0 || a.post_act > 1 || (size_t)a.N * a.H * a.W * a.xcs * 2 >= (1ull << 31) || (size_t)a.N * a.Ho * a.Wo * std::max(a.ycs, a.r1 ? a.r1cs : 0) * 2 >= (1ull << 31))
            fail(EAGLE_E_NOKERNEL, "weight-stationary conv needs kc == cin, fp16 output, at most one residual, pre_act none, post_act in {none, ReLU} and tensors below 2 GiB (kc=%d cin=%d)", c.kc, c.cin);
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / lds));
        const int unit = 8 * gy;
        gx = std::max(unit, std::min((gx * gy + unit - 1) / unit * unit, 256 * per_cu / unit * unit));
    }
    a.gy = gy;
    // 1x1 layers with several Cout blocks re-read their input tile once per block: in tile-major / block-minor order on one XCD the
    // re-reads hit that XCD's L2 instead of HBM
    a.xcd = (prec_is_f16_kernels(precision) && !ws && (c.ks == 3 || (c.ks == 1 && gy > 1))) ? 1 : 0;
    dim3 grid(gx, gy);
    if (a.xcd) grid = dim3(gx * gy, 1);
    if (ws) grid = dim3(gx, 1);
    hipLaunchKernelGGL(fn, grid, dim3(256), lds, s, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace eagle
