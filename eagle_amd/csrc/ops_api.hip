// Operator-level entry points (eagle_op_*): one kernel family each, host tensors in and out, for the parity tests.
#include "runtime.h"

extern "C" {

// ---- operator-level entry points for the parity tests ---------------------------------------------------------------
static void to_dev(Net& net, int prec, const float* src, int n, int h, int w, int c, int cpad, TView& v)
{
    v.n = n; v.h = h; v.w = w; v.c = cpad; v.cs = cpad; v.off = 0; v.f32 = prec_tensor_fmt(prec);
    const size_t px = (size_t)n * h * w;
    if (v.f32 == 2) {                                       // [hi x 8][lo x 8] per 8 channels, hi = rn(16 v), lo = rn(16 v - hi)
        std::vector<_Float16> t(px * cpad * 2, (_Float16)0.f);
        for (size_t p = 0; p < px; ++p)
            for (int k = 0; k < c; ++k) {
                const float sv = src[p * c + k] * 16.0f;
                const _Float16 hi = (_Float16)sv;
                t[p * cpad * 2 + (k / 8) * 16 + (k % 8)] = hi;
                t[p * cpad * 2 + (k / 8) * 16 + 8 + (k % 8)] = (_Float16)(sv - (float)hi);
            }
        v.p = net.upload(t.data(), t.size() * 2);
    } else if (v.f32) {
        std::vector<float> t(px * cpad, 0.f);
        for (size_t p = 0; p < px; ++p) for (int k = 0; k < c; ++k) t[p * cpad + k] = src[p * c + k];
        v.p = net.upload(t.data(), t.size() * 4);
    } else {
        std::vector<_Float16> t(px * cpad, (_Float16)0.f);
        for (size_t p = 0; p < px; ++p) for (int k = 0; k < c; ++k) t[p * cpad + k] = (_Float16)src[p * c + k];
        v.p = net.upload(t.data(), t.size() * 2);
    }
}
static void from_dev(const TView& v, int c, float* dst)
{
    const size_t px = (size_t)v.n * v.h * v.w;
    if (v.f32 == 2) {
        std::vector<_Float16> t(px * v.cs * 2);
        HIP_CHECK(hipMemcpy(t.data(), v.p, t.size() * 2, hipMemcpyDeviceToHost));
        for (size_t p = 0; p < px; ++p)
            for (int k = 0; k < c; ++k) {
                const size_t e = p * v.cs * 2 + (size_t)((v.off + k) / 8) * 16 + (v.off + k) % 8;
                dst[p * c + k] = ((float)t[e] + (float)t[e + 8]) * 0.0625f;
            }
    } else if (v.f32) {
        std::vector<float> t(px * v.cs);
        HIP_CHECK(hipMemcpy(t.data(), v.p, t.size() * 4, hipMemcpyDeviceToHost));
        for (size_t p = 0; p < px; ++p) for (int k = 0; k < c; ++k) dst[p * c + k] = t[p * v.cs + v.off + k];
    } else {
        std::vector<_Float16> t(px * v.cs);
        HIP_CHECK(hipMemcpy(t.data(), v.p, t.size() * 2, hipMemcpyDeviceToHost));
        for (size_t p = 0; p < px; ++p) for (int k = 0; k < c; ++k) dst[p * c + k] = (float)t[p * v.cs + v.off + k];
    }
}

// The channel padding of eagle_op_conv2d and conv_choose's pick for the padded layer: shared with eagle_op_conv_config, which reports what the former runs.
static ConvConfig op_conv_choose(int precision, int ks, int stride, int cin, int cout, int wo, bool plain_epilogue, bool second_residual, int* cin_pad, int* cout_pad)
{
    const int g = precision == EAGLE_PREC_F32 ? 4 : 8;
    *cin_pad = cin <= g ? g : (cin + 15) / 16 * 16; *cout_pad = (cout + 15) / 16 * 16;
    return conv_choose(precision, ks, stride, *cin_pad, *cout_pad, wo, plain_epilogue, second_residual);
}

int eagle_op_conv_config(int precision, int ks, int stride, int cin, int cout, int wo, int plain_epilogue, int second_residual, int32_t out[8])
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (precision < EAGLE_PREC_F16 || precision > EAGLE_PREC_F32S || (ks != 1 && ks != 3) || stride < 1 || cin < 1 || cout < 1 || wo < 1 || !out)
        fail(EAGLE_E_INVALID, "eagle_op_conv_config: bad argument (ks 1 or 3)");
    int cin_pad, cout_pad;
    const ConvConfig c = op_conv_choose(precision, ks, stride, cin, cout, wo, plain_epilogue != 0, second_residual != 0, &cin_pad, &cout_pad);
    int th = 0, tw = 0;
    size_t lds = 0;
    const bool inst = conv_supported(precision, c);
    if (inst) { conv_tile_shape(precision, c, &th, &tw); lds = conv_lds_bytes(precision, c); }
    const int r[8] = {c.kc, c.nt, c.wx, c.variant, th, tw, (int)lds, inst && lds <= 160 * 1024 ? 1 : 0};
    for (int k = 0; k < 8; ++k) out[k] = r[k];
    API_END(hh)
}

int eagle_op_conv_table(int which, int32_t* rows, int cap)
{
    try { return conv_table(which, rows, rows ? cap : 0); }
    catch (const eagle::Err& e) { eagle::g_create_error = e.msg; return e.code; }
}

int eagle_op_conv2d(int device, int precision, const float* x, int n, int h, int w, int cin, const float* w_hwio,
                    const float* bias, int cout, int ks, int stride, int pre_act, const float* r1, const float* r2,
                    int post_act, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const int ho = (h + 2 * (ks / 2) - ks) / stride + 1, wo = (w + 2 * (ks / 2) - ks) / stride + 1;
    ConvLaunch L;
    int cin_pad, cout_pad;
    L.cfg = op_conv_choose(precision, ks, stride, cin, cout, wo, pre_act == ACT_NONE && post_act <= ACT_RELU, r1 && r2, &cin_pad, &cout_pad);
    to_dev(net, precision, x, n, h, w, cin, cin_pad, L.x);
    if (!conv_supported(precision, L.cfg)) fail(EAGLE_E_NOKERNEL, "no kernel instance ks=%d s=%d kc=%d nt=%d", ks, stride, L.cfg.kc, L.cfg.nt);
    std::vector<char> tiled(conv_weight_elems(precision, L.cfg) * (precision == EAGLE_PREC_F32 ? 4 : 2));
    conv_tile_weights(precision, L.cfg, w_hwio, cin, cout, tiled.data(), &L.descale);
    L.w = net.upload(tiled.data(), tiled.size());
    std::vector<float> b(cout_pad, 0.f);
    for (int i = 0; i < cout; ++i) b[i] = bias[i];
    L.bias = (const float*)net.upload(b.data(), b.size() * 4);
    L.y.n = n; L.y.h = ho; L.y.w = wo; L.y.c = cout_pad; L.y.cs = cout_pad; L.y.f32 = prec_tensor_fmt(precision);
    L.y.p = net.get((size_t)n * ho * wo * cout_pad * L.y.esize());
    if (r1) to_dev(net, precision, r1, n, ho, wo, cout, cout_pad, L.r1);
    if (r2) to_dev(net, precision, r2, n, ho, wo, cout, cout_pad, L.r2);
    L.pre_act = pre_act; L.post_act = post_act;
    conv_launch(precision, L, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    from_dev(L.y, cout, y);
    API_END(hh)
}

int eagle_op_bottleneck(int device, const float* x, int n, int h, int w, int cin, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, const float* res, float* y, int reps, float* ms, const float* wd, const float* bd)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    if (!x || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !y || n < 1 || h < 1 || w < 1 || cin % 16 || cin < 16) fail(EAGLE_E_INVALID, "eagle_op_bottleneck: bad argument (Cin must be a multiple of 16)");
    if ((wd != nullptr) != (bd != nullptr) || (wd && (res || cin != 64))) fail(EAGLE_E_INVALID, "eagle_op_bottleneck: the in-kernel downsample branch takes (wd, bd) together, Cin = 64 and no residual tensor");
    if (!res && !wd && cin != 256) fail(EAGLE_E_INVALID, "eagle_op_bottleneck: an identity shortcut needs Cin = 256");
    Net net;
    BneckLaunch L;
    to_dev(net, EAGLE_PREC_F32S, x, n, h, w, cin, cin, L.x);
    if (res) to_dev(net, EAGLE_PREC_F32S, res, n, h, w, 256, 256, L.res); else L.res = L.x;
    L.y = L.x; L.y.c = L.y.cs = 256; L.y.off = 0; L.y.p = net.get((size_t)n * h * w * 256 * 4);
    if (wd) L.res = L.y;                                    // (not read)
    std::vector<_Float16> img;
    bneck_tile_weights(w1, 1, cin, 64, img, &L.ds1); L.w1 = net.upload(img.data(), img.size() * 2);
    bneck_tile_weights(w2, 9, 64, 64, img, &L.ds2); L.w2 = net.upload(img.data(), img.size() * 2);
    std::vector<float> w3x(w3, w3 + 64 * 256), sb3(b3, b3 + 256);
    if (wd) {                                               // K = 128: [W3 | Wd], bias b3 + bd
        w3x.insert(w3x.end(), wd, wd + 64 * 256);
        for (int o = 0; o < 256; ++o) sb3[o] = sb3[o] + bd[o];
        L.ds_fused = true;
    }
    bneck_tile_weights(w3x.data(), 1, wd ? 128 : 64, 256, img, &L.ds3); L.w3 = net.upload(img.data(), img.size() * 2);
    std::vector<float> sb1(b1, b1 + 64), sb2(b2, b2 + 64);
    bneck_scale_bias(sb1, L.ds1); bneck_scale_bias(sb2, L.ds2); bneck_scale_bias(sb3, L.ds3);
    L.b1 = (const float*)net.upload(sb1.data(), 64 * 4); L.b2 = (const float*)net.upload(sb2.data(), 64 * 4); L.b3 = (const float*)net.upload(sb3.data(), 256 * 4);
    if (getenv("EAGLE_BNECK_TIMING")) L.dbg = (unsigned long long*)net.get(8192 * 8 * 8);      // (developer timing builds: -DEAGLE_BNECK_TIMING)
    unsigned* op_sat = nullptr; unsigned* const* op_sat_slot = &op_sat;
    if (getenv("EAGLE_BNECK_OPSAT")) { op_sat = (unsigned*)net.get(sizeof(unsigned) * (size_t)n); L.sat_slot = op_sat_slot; }      // developer: the per-frame saturation counters the pipeline passes
    bneck_launch(L, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    if (L.dbg) {
        std::vector<unsigned long long> t(8192 * 8);
        HIP_CHECK(hipMemcpy(t.data(), L.dbg, t.size() * 8, hipMemcpyDeviceToHost));
        double sum[8] = {0}; int nw = 0;
        for (int b = 0; b < 8192; ++b) { bool any = false; for (int k = 0; k < 8; ++k) { sum[k] += (double)t[b * 8 + k]; any |= t[b * 8 + k] != 0; } nw += any; }
        if (nw) fprintf(stderr, "[bneck timing] %d workgroups, mean us per workgroup: phase1 %.1f  wait %.1f  epi1 %.1f  phase2 %.1f  epi2 %.1f  phase3 %.1f\n", nw,
                        sum[0] / nw / 100, sum[1] / nw / 100, sum[2] / nw / 100, sum[3] / nw / 100, sum[4] / nw / 100, sum[5] / nw / 100);
    }
    if (reps > 0 && ms) {                                   // developer timing: the launch alone, HIP events on the launch stream
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, nullptr));
        for (int i = 0; i < reps; ++i) bneck_launch(L, nullptr);
        HIP_CHECK(hipEventRecord(e1, nullptr));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(ms, e0, e1));
        *ms /= (float)reps;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    from_dev(L.y, 256, y);
    API_END(hh)
}

int eagle_op_stem(int device, const uint8_t* bgr, int n, int h, int w, int dh, int dw, const float* w1, const float* b1, float* y, uint32_t* sat)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    if (!bgr || !w1 || !b1 || !y || n < 1 || h < 1 || w < 1 || dh < 1 || dw < 1) fail(EAGLE_E_INVALID, "eagle_op_stem: bad argument");
    if (!stem_supported(EAGLE_PREC_F32S, 3, 2, 3, 64)) fail(EAGLE_E_NOKERNEL, "eagle_op_stem: no kernel");
    Net net;
    StemLaunch L;
    L.bgr = (const uint8_t*)net.upload(bgr, (size_t)n * h * w * 3);
    L.n = n; L.sh = h; L.sw = w; L.dh = dh; L.dw = dw;
    std::vector<_Float16> img;
    stem_tile_weights(w1, img, &L.descale);
    L.w = net.upload(img.data(), img.size() * 2);
    L.bias = (const float*)net.upload(b1, 64 * 4);
    L.y.n = n; L.y.h = (dh - 1) / 2 + 1; L.y.w = (dw - 1) / 2 + 1; L.y.c = L.y.cs = 64; L.y.f32 = 2;
    L.y.p = net.get((size_t)n * L.y.h * L.y.w * 64 * 4);
    unsigned* d_sat = (unsigned*)net.get(sizeof(unsigned) * (size_t)n);      // (Net::get returns zeroed memory)
    unsigned* const* slot = &d_sat;
    L.sat_slot = slot;
    stem_launch(L, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    from_dev(L.y, 64, y);
    if (sat) HIP_CHECK(hipMemcpy(sat, d_sat, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost));
    API_END(hh)
}

int eagle_op_fuse_sum(int device, int precision, const float* base, int n, int H, int W, int c, int n_up,
                      const float* const* ups, const int* up_h, const int* up_w, int relu, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    if (n_up > 3 || c % 8) fail(EAGLE_E_INVALID, "fuse_sum: n_up <= 3 and c %% 8 == 0 required");
    Net net;
    TView b, o;
    to_dev(net, precision, base, n, H, W, c, c, b);
    FuseUp u[3];
    for (int i = 0; i < n_up; ++i) to_dev(net, precision, ups[i], n, up_h[i], up_w[i], c, c, u[i].z);
    o = b; o.p = net.get((size_t)n * H * W * c * b.esize());
    fuse_sum_launch(b, u, n_up, relu, o, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    from_dev(o, c, y);
    API_END(hh)
}

int eagle_op_preprocess(int device, int precision, const uint8_t* bgr, int n, int h, int w, int det_imgsz,
                        float* kp_out, float* det_out, int* det_hw)
{
    return eagle_op_preprocess_lb(device, precision, bgr, n, h, w, det_imgsz, EAGLE_LETTERBOX_RECT, kp_out, det_out, det_hw);
}

int eagle_op_preprocess_lb(int device, int precision, const uint8_t* bgr, int n, int h, int w, int det_imgsz, int letterbox,
                           float* kp_out, float* det_out, int* det_hw)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const int cp = precision == EAGLE_PREC_F32 ? 4 : 8;
    const LetterBox lb = letterbox_geometry(h, w, det_imgsz, letterbox);
    det_hw[0] = lb.out_h; det_hw[1] = lb.out_w;
    if (!kp_out || !det_out) return EAGLE_OK;
    uint8_t* d = (uint8_t*)net.upload(bgr, (size_t)n * h * w * 3);
    TView kp, det;
    kp.n = n; kp.h = 540; kp.w = 960; kp.c = kp.cs = cp; kp.f32 = prec_tensor_fmt(precision);
    det = kp; det.h = lb.out_h; det.w = lb.out_w;
    kp.p = net.get((size_t)n * 540 * 960 * cp * kp.esize());
    det.p = net.get((size_t)n * lb.out_h * lb.out_w * cp * det.esize());
    preprocess_launch(precision, d, n, h, w, kp, det, lb, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    from_dev(kp, 3, kp_out);
    from_dev(det, 3, det_out);
    API_END(hh)
}

int eagle_op_find_homography(int device, const float* img_pts, const float* world_pts, int n, double thresh,
                             int max_iters, int lm_iters, double* H9, uint8_t* mask, int* ok)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    if (n < 0 || n > EAGLE_MAX_KP) fail(EAGLE_E_INVALID, "0 <= n <= %d required", EAGLE_MAX_KP);
    Net net;
    float* di = (float*)net.upload(img_pts, sizeof(float) * 2 * std::max(n, 1));
    float* dw = (float*)net.upload(world_pts, sizeof(float) * 2 * std::max(n, 1));
    double* dH = (double*)net.get(72);
    uint8_t* dm = (uint8_t*)net.get(256);
    int* dok = (int*)net.get(16);
    homography_only_launch(di, dw, n, thresh, max_iters, lm_iters, dH, dm, dok, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(H9, dH, 72, hipMemcpyDeviceToHost));
    if (n > 0) HIP_CHECK(hipMemcpy(mask, dm, n, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(ok, dok, sizeof(int), hipMemcpyDeviceToHost));
    API_END(hh)
}

// ---- the tail behind the networks on chosen inputs (tests/test_gpu_tail.py) -----------------------------------------------------
int eagle_op_detect_tail(int device, int n_lv, const int* gh, const int* gw, const float* stride, const float* const* box, const float* const* cls, int n, int nc,
                         float conf_floor, float nms_iou, double detector_conf, int frame_h, int frame_w, int in_h, int in_w,
                         EagleFrameResult* out, float* boxes, float* conf, int32_t* cls_out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (n_lv < 1 || n_lv > 3 || !gh || !gw || !stride || !box || !cls || !out || n < 1 || nc < 1 || nc > 16 || frame_h < 1 || frame_w < 1 || in_h < 1 || in_w < 1)
        fail(EAGLE_E_INVALID, "eagle_op_detect_tail: bad argument (1 - 3 levels, 1 - 16 classes)");
    int A = 0;
    for (int l = 0; l < n_lv; ++l) {
        if (gh[l] < 1 || gw[l] < 1 || !box[l] || !cls[l]) fail(EAGLE_E_INVALID, "eagle_op_detect_tail: bad level %d", l);
        A += gh[l] * gw[l];
    }
    if (A > nms_anchor_limit()) fail(EAGLE_E_INVALID, "eagle_op_detect_tail: %d anchors, the NMS kernel sorts at most %d", A, nms_anchor_limit());
    HIP_CHECK(hipSetDevice(device));
    Net net;
    DetLevel lv[3];
    int a0 = 0;
    for (int l = 0; l < n_lv; ++l) {
        to_dev(net, EAGLE_PREC_F32, box[l], n, gh[l], gw[l], 64, 64, lv[l].box);
        to_dev(net, EAGLE_PREC_F32, cls[l], n, gh[l], gw[l], nc, (nc + 3) / 4 * 4, lv[l].cls);
        lv[l].gh = gh[l]; lv[l].gw = gw[l]; lv[l].stride = stride[l]; lv[l].a0 = a0;
        a0 += gh[l] * gw[l];
    }
    DetScratch sc;
    sc.A = A;
    sc.boxes = (float*)net.get(sizeof(float) * 4 * (size_t)n * A);
    sc.conf = (float*)net.get(sizeof(float) * (size_t)n * A);
    sc.cls = (int*)net.get(sizeof(int) * (size_t)n * A);
    sc.keys = (unsigned long long*)net.get(sizeof(unsigned long long) * (size_t)n * A);
    sc.count = (int*)net.get(sizeof(int) * (size_t)n);
    EagleFrameResult* d_out = (EagleFrameResult*)net.get(sizeof(EagleFrameResult) * (size_t)n);
    PostParams pp{};
    pp.frame_h = frame_h; pp.frame_w = frame_w; pp.in_h = in_h; pp.in_w = in_w; pp.nms_iou = nms_iou; pp.detector_conf = detector_conf;
    yolo_decode_launch(lv, n_lv, n, nc, conf_floor, sc, nullptr);
    nms_launch(sc, n, pp, d_out, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, d_out, sizeof(EagleFrameResult) * (size_t)n, hipMemcpyDeviceToHost));
    if (boxes) HIP_CHECK(hipMemcpy(boxes, sc.boxes, sizeof(float) * 4 * (size_t)n * A, hipMemcpyDeviceToHost));
    if (conf) HIP_CHECK(hipMemcpy(conf, sc.conf, sizeof(float) * (size_t)n * A, hipMemcpyDeviceToHost));
    if (cls_out) HIP_CHECK(hipMemcpy(cls_out, sc.cls, sizeof(int) * (size_t)n * A, hipMemcpyDeviceToHost));
    API_END(hh)
}

int eagle_op_post(int device, int n, int hm_h, int hm_w, int chunks, const float* logits, const EagleArgmaxPart* parts, EagleArgmaxPart* parts_out,
                  EagleFrameResult* recs, int frame_h, int frame_w, double keypoint_conf, double ransac_thresh, int ransac_max_iters, int lm_iters)
{
    static_assert(sizeof(EagleArgmaxPart) == sizeof(ArgmaxPart), "the public partial is the kernels' ArgmaxPart");
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (n < 1 || hm_h < 1 || hm_w < 1 || chunks < 1 || !recs || (logits != nullptr) == (parts != nullptr) || frame_h < 1 || frame_w < 1)
        fail(EAGLE_E_INVALID, "eagle_op_post: bad argument (exactly one of logits / parts)");
    for (int f = 0; f < n; ++f)
        if (recs[f].n_det < 0 || recs[f].n_det > EAGLE_MAX_DET) fail(EAGLE_E_INVALID, "eagle_op_post: record %d has n_det %d", f, recs[f].n_det);
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const size_t np = (size_t)n * chunks * 64;
    ArgmaxPart* d_parts;
    if (logits) {
        TView lg;
        to_dev(net, EAGLE_PREC_F32, logits, n, hm_h, hm_w, 64, 64, lg);
        d_parts = (ArgmaxPart*)net.get(sizeof(ArgmaxPart) * np);
        heat_argmax_launch(lg, d_parts, chunks, nullptr);
    } else {
        d_parts = (ArgmaxPart*)net.upload(parts, sizeof(ArgmaxPart) * np);
    }
    EagleFrameResult* d_recs = (EagleFrameResult*)net.upload(recs, sizeof(EagleFrameResult) * (size_t)n);
    PostParams pp{};
    pp.frame_h = frame_h; pp.frame_w = frame_w; pp.hm_h = hm_h; pp.hm_w = hm_w; pp.hm_chunks = chunks;
    pp.keypoint_conf = keypoint_conf; pp.ransac_thresh = ransac_thresh; pp.ransac_max_iters = ransac_max_iters; pp.lm_iters = lm_iters;
    post_launch(d_parts, n, pp, d_recs, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(recs, d_recs, sizeof(EagleFrameResult) * (size_t)n, hipMemcpyDeviceToHost));
    if (parts_out) HIP_CHECK(hipMemcpy(parts_out, d_parts, sizeof(ArgmaxPart) * np, hipMemcpyDeviceToHost));
    API_END(hh)
}

int eagle_op_conv2d_argmax(int device, int precision, const float* x, int n, int h, int w, int cin, const float* w_hwio, const float* bias, int cout, int ks, int stride,
                           float* logits, EagleArgmaxPart* parts, int* tiles, int* tile_h, int* tile_w)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!prec_is_f16_kernels(precision) || cout < 1 || cout > 64 || n < 1 || h < 1 || w < 1 || cin < 1 || (ks != 1 && ks != 3) || stride < 1 || !tiles || !tile_h || !tile_w)
        fail(EAGLE_E_INVALID, "eagle_op_conv2d_argmax: the fp16 and split families, cout <= 64, ks 1 or 3");
    const int cin_pad = cin <= 8 ? 8 : (cin + 15) / 16 * 16, cout_pad = (cout + 15) / 16 * 16;
    const int ho = (h + 2 * (ks / 2) - ks) / stride + 1, wo = (w + 2 * (ks / 2) - ks) / stride + 1;
    ConvLaunch L;
    L.cfg = conv_choose(precision, ks, stride, cin_pad, cout_pad, wo, false, false);      // as Builder::conv for an fp32-output layer
    if (!conv_supported(precision, L.cfg)) fail(EAGLE_E_NOKERNEL, "no kernel instance ks=%d s=%d kc=%d nt=%d", ks, stride, L.cfg.kc, L.cfg.nt);
    conv_tile_shape(precision, L.cfg, tile_h, tile_w);
    *tiles = conv_tiles_per_frame(precision, L.cfg, ho, wo);
    if (!logits) return EAGLE_OK;
    if (!x || !w_hwio || !bias || !parts) fail(EAGLE_E_INVALID, "eagle_op_conv2d_argmax: null argument");
    HIP_CHECK(hipSetDevice(device));
    Net net;
    to_dev(net, precision, x, n, h, w, cin, cin_pad, L.x);
    std::vector<char> tiled(conv_weight_elems(precision, L.cfg) * 2);
    conv_tile_weights(precision, L.cfg, w_hwio, cin, cout, tiled.data(), &L.descale);
    L.w = net.upload(tiled.data(), tiled.size());
    std::vector<float> b(cout_pad, 0.f);
    for (int i = 0; i < cout; ++i) b[i] = bias[i];
    L.bias = (const float*)net.upload(b.data(), b.size() * 4);
    L.y.n = n; L.y.h = ho; L.y.w = wo; L.y.c = cout_pad; L.y.cs = cout_pad; L.y.f32 = 1;
    L.y.p = net.get((size_t)n * ho * wo * cout_pad * 4);
    L.out_f32 = 1;
    conv_launch(precision, L, nullptr);                     // the logits
    const size_t np = (size_t)n * *tiles * cout_pad;
    ArgmaxPart* d_parts = (ArgmaxPart*)net.get(sizeof(ArgmaxPart) * np);
    ArgmaxPart* const* slot = &d_parts;
    L.am_slot = slot;
    conv_launch(precision, L, nullptr);                     // the same launch with the fused arg-max epilogue
    HIP_CHECK(hipDeviceSynchronize());
    from_dev(L.y, cout, logits);
    HIP_CHECK(hipMemcpy(parts, d_parts, sizeof(ArgmaxPart) * np, hipMemcpyDeviceToHost));
    API_END(hh)
}

// ---- the optical-flow kernels without a handle or weights (tests/test_gpu_lk.py) ------------------------------------------------------------
// n dense BGR frames -> a ClipView as eagle_clip_open makes it (same level rule, same K11 launch), its buffers owned by `net`
static void flow_op_view(Net& net, const char* what, const uint8_t* bgr, int n, int h, int w, ClipView& cv, uint8_t* g[3])
{
    if (!bgr || n < 1 || h < 32 || w < 32) fail(EAGLE_E_INVALID, "%s: n >= 1 frames of at least 32 x 32 pixels required (n %d, %d x %d)", what, n, h, w);
    cv.bgr = (const uint8_t*)net.upload(bgr, (size_t)n * h * w * 3);
    cv.n = n; cv.h = h; cv.w = w;
    clip_view_levels(cv);
    for (int l = 0; l < 3; ++l) {
        g[l] = (uint8_t*)net.get(std::max<size_t>((size_t)n * cv.lh[l] * cv.lw[l], 16));
        cv.g[l] = g[l];
    }
    gray_pyramid_launch(cv.bgr, n, h, w, g[0], g[1], g[2], nullptr);
}

int eagle_op_gray_pyramid(int device, const uint8_t* bgr, int n, int h, int w, uint8_t* g0, uint8_t* g1, uint8_t* g2, int* levels_out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!g0 || !g1 || !g2 || !levels_out) fail(EAGLE_E_INVALID, "eagle_op_gray_pyramid: null argument");
    HIP_CHECK(hipSetDevice(device));
    Net net;
    ClipView cv; uint8_t* g[3];
    flow_op_view(net, "eagle_op_gray_pyramid", bgr, n, h, w, cv, g);
    HIP_CHECK(hipDeviceSynchronize());
    uint8_t* out[3] = {g0, g1, g2};
    for (int l = 0; l < 3; ++l) HIP_CHECK(hipMemcpy(out[l], g[l], (size_t)n * cv.lh[l] * cv.lw[l], hipMemcpyDeviceToHost));
    *levels_out = cv.levels;
    API_END(hh)
}

int eagle_op_flow(int device, const uint8_t* bgr, int n, int h, int w, int src_frame, int dst_frame, int hue_frame, const EagleFlowKp* in, int n_in,
                  EagleFlowKp* out, int* n_out, float* next_pts, uint8_t* status)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (src_frame < 0 || src_frame >= n || dst_frame < 0 || dst_frame >= n || hue_frame < 0 || hue_frame >= n || n_in < 0 || n_in > EAGLE_N_LANDMARKS ||
        (!in && n_in > 0) || !out || !n_out)
        fail(EAGLE_E_INVALID, "eagle_op_flow: frames inside the clip and 0 <= n_in <= %d required", EAGLE_N_LANDMARKS);
    HIP_CHECK(hipSetDevice(device));
    Net net;
    ClipView cv; uint8_t* g[3];
    flow_op_view(net, "eagle_op_flow", bgr, n, h, w, cv, g);
    *n_out = 0;
    if (n_in == 0) { HIP_CHECK(hipDeviceSynchronize()); return EAGLE_OK; }      // cm.py:429: empty dict in -> empty dict out
    std::vector<ChainState> zs(1);                        // exactly eagle_clip_flow's step on a scratch state
    ChainState& z = zs[0];
    memset(&z, 0, sizeof(z));
    z.stalled = -1; z.n_prev = n_in;
    for (int k = 0; k < n_in; ++k) z.prev[k] = in[k];
    ChainState* st = (ChainState*)net.upload(&z, sizeof(z));
    lk_launch(cv, src_frame, dst_frame, st, nullptr, 1, nullptr);
    flow_filter_launch(cv, st, hue_frame, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(&z, st, sizeof(z), hipMemcpyDeviceToHost));
    *n_out = z.flow_n;
    for (int k = 0; k < z.flow_n; ++k) out[k] = z.flow[k];
    if (next_pts) memcpy(next_pts, z.lk_next, sizeof(float) * 2 * n_in);
    if (status) memcpy(status, z.lk_status, n_in);
    API_END(hh)
}

// ---- the ECC camera-motion kernels (ecc.hip, K17) without a handle (tests/test_gpu_ecc_ops.py) ---------------------------------------------
int eagle_op_ecc_small(int device, const uint8_t* gray, int n, int h, int w, double scale, uint8_t* small_out, int* dh_out, int* dw_out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!gray || !dh_out || !dw_out || n < 1 || h < 1 || w < 1 || !(scale > 0.0) || !(scale <= 1.0))
        fail(EAGLE_E_INVALID, "eagle_op_ecc_small: n >= 1 gray frames and 0 < scale <= 1 required (n %d, %d x %d, scale %g)", n, h, w, scale);
    const int dh = (int)lrint(h * scale), dw = (int)lrint(w * scale);      // as eagle_clip_motion_ecc
    if (dh < 4 || dw < 4) fail(EAGLE_E_INVALID, "eagle_op_ecc_small: frame too small for the %g-scale alignment (%d x %d -> %d x %d)", scale, h, w, dh, dw);
    *dh_out = dh; *dw_out = dw;
    if (!small_out) return EAGLE_OK;                      // the size query
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const uint8_t* d = (const uint8_t*)net.upload(gray, (size_t)n * h * w);
    uint8_t* s = (uint8_t*)net.get((size_t)n * dh * dw);
    ecc_small_launch(d, s, n, h, w, dh, dw, 1.0 / scale, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(small_out, s, (size_t)n * dh * dw, hipMemcpyDeviceToHost));
    API_END(hh)
}

int eagle_op_ecc(int device, const uint8_t* small, int n, int h, int w, const uint8_t* carry, const int32_t* pairs, int n_pairs, int max_iter, double eps,
                 EagleEccResult* out)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    static_assert(sizeof(EagleEccResult) == sizeof(EccResult) && offsetof(EagleEccResult, rho) == offsetof(EccResult, rho) &&
                  offsetof(EagleEccResult, M) == offsetof(EccResult, M), "EagleEccResult mirrors EccResult");
    if (!small || n < 1 || h < 4 || w < 4) fail(EAGLE_E_INVALID, "eagle_op_ecc: n >= 1 images of at least 4 x 4 pixels required (n %d, %d x %d)", n, h, w);
    if (max_iter < 0 || max_iter > 100 || n_pairs < 0 || n_pairs > 4096 || !(eps == eps))
        fail(EAGLE_E_INVALID, "eagle_op_ecc: 0 <= max_iter <= 100 and 0 <= n_pairs <= 4096 required (max_iter %d, n_pairs %d)", max_iter, n_pairs);
    if (n_pairs == 0) return EAGLE_OK;
    if (!pairs || !out) fail(EAGLE_E_INVALID, "eagle_op_ecc: null argument");
    for (int k = 0; k < n_pairs; ++k) {
        const int t = pairs[2 * k], i = pairs[2 * k + 1];
        if (i < 0 || i >= n || t < -1 || t >= n || (t == -1 && !carry))
            fail(EAGLE_E_INVALID, "eagle_op_ecc: pair %d = (%d, %d): images inside [0, %d), the template -1 only with a carried image", k, t, i, n);
    }
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const size_t npx = (size_t)h * w;
    const uint8_t* d = (const uint8_t*)net.upload(small, (size_t)n * npx);
    const uint8_t* dc = carry ? (const uint8_t*)net.upload(carry, npx) : nullptr;
    const int2* dp = (const int2*)net.upload(pairs, sizeof(int2) * (size_t)n_pairs);
    EccResult* dr = (EccResult*)net.get(sizeof(EccResult) * (size_t)n_pairs);
    ecc_launch(d, dc, dp, n_pairs, dr, h, w, max_iter, eps, nullptr);     // one launch for all pairs
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, dr, sizeof(EccResult) * (size_t)n_pairs, hipMemcpyDeviceToHost));
    API_END(hh)
}

// ---- the OSNet (ReID) kernels of reid.hip one launch at a time (tests/test_gpu_reid_ops.py) ------------------------------------------------
// Every activation operand is a slice view: `c` channels at channel `off` of a buffer with `cs` floats per pixel.  Whatever lies outside the
// slice holds EAGLE_OP_SENTINEL_BITS (a quiet NaN) when the kernel starts, and output buffers come back whole: a read outside an input slice
// shows as a NaN in the result, a write outside an output slice as an overwritten sentinel.
static void reid_fill_sentinel(std::vector<float>& t)
{
    const uint32_t bits = EAGLE_OP_SENTINEL_BITS;
    float s; memcpy(&s, &bits, 4);
    std::fill(t.begin(), t.end(), s);
}
static TView reid_view(Net& net, const char* what, const float* src, int n, int h, int w, int c, int cs, int off)
{
    if (n < 1 || h < 1 || w < 1 || c < 4 || c % 4 || cs % 4 || off % 4 || off < 0 || cs < off + c)
        fail(EAGLE_E_INVALID, "%s: [%d, %d, %d, %d] at channel %d of %d: sizes >= 1; c, cs, off multiples of 4; off + c <= cs", what, n, h, w, c, off, cs);
    TView v; v.n = n; v.h = h; v.w = w; v.c = c; v.cs = cs; v.off = off; v.f32 = 1;
    const size_t px = (size_t)n * h * w;
    std::vector<float> t(px * cs);
    reid_fill_sentinel(t);
    if (src) for (size_t p = 0; p < px; ++p) for (int k = 0; k < c; ++k) t[p * cs + off + k] = src[p * c + k];
    v.p = net.upload(t.data(), t.size() * 4);
    return v;
}
static float* reid_flat(Net& net, size_t count)
{
    std::vector<float> t(count);
    reid_fill_sentinel(t);
    return (float*)net.upload(t.data(), t.size() * 4);
}
static void reid_whole(const TView& v, float* dst) { HIP_CHECK(hipMemcpy(dst, v.p, (size_t)v.n * v.h * v.w * v.cs * 4, hipMemcpyDeviceToHost)); }

int eagle_op_reid_crop(int device, const uint8_t* bgr, int nf, int fh, int fw, const EagleCrop* crops, int n, int oh, int ow, int y_cs, int y_off, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!bgr || !crops || !y || nf < 1 || fh < 1 || fw < 1) fail(EAGLE_E_INVALID, "eagle_op_reid_crop: bad argument");
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const uint8_t* d = (const uint8_t*)net.upload(bgr, (size_t)nf * fh * fw * 3);
    const EagleCrop* dc = (const EagleCrop*)net.upload(crops, sizeof(EagleCrop) * (size_t)std::max(n, 1));
    const TView o = reid_view(net, "eagle_op_reid_crop: y", nullptr, n, oh, ow, 4, y_cs, y_off);
    reid_crop_launch(d, nf, fh, fw, dc, n, o, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    reid_whole(o, y);
    API_END(hh)
}

int eagle_op_reid_conv7(int device, const float* x, int n, int h, int w, int x_cs, int x_off, const float* wt, const float* b, int y_cs, int y_off, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!x || !wt || !b || !y) fail(EAGLE_E_INVALID, "eagle_op_reid_conv7: null argument");
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const TView xv = reid_view(net, "eagle_op_reid_conv7: x", x, n, h, w, 4, x_cs, x_off);
    const TView yv = reid_view(net, "eagle_op_reid_conv7: y", nullptr, n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, 16, y_cs, y_off);
    const float* dw = (const float*)net.upload(wt, 7 * 7 * 3 * 16 * 4);
    const float* db = (const float*)net.upload(b, 16 * 4);
    reid_conv7_launch(xv, dw, db, yv, n, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    reid_whole(yv, y);
    API_END(hh)
}

int eagle_op_reid_maxpool3s2(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int y_cs, int y_off, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!x || !y) fail(EAGLE_E_INVALID, "eagle_op_reid_maxpool3s2: null argument");
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const TView xv = reid_view(net, "eagle_op_reid_maxpool3s2: x", x, n, h, w, c, x_cs, x_off);
    const TView yv = reid_view(net, "eagle_op_reid_maxpool3s2: y", nullptr, n, (h - 1) / 2 + 1, (w - 1) / 2 + 1, c, y_cs, y_off);
    reid_maxpool3s2_launch(xv, yv, n, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    reid_whole(yv, y);
    API_END(hh)
}

int eagle_op_reid_avgpool2(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int y_cs, int y_off, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!x || !y) fail(EAGLE_E_INVALID, "eagle_op_reid_avgpool2: null argument");
    if (h < 2 || w < 2) fail(EAGLE_E_INVALID, "eagle_op_reid_avgpool2: a %d x %d map has no 2 x 2 window", h, w);
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const TView xv = reid_view(net, "eagle_op_reid_avgpool2: x", x, n, h, w, c, x_cs, x_off);
    const TView yv = reid_view(net, "eagle_op_reid_avgpool2: y", nullptr, n, h / 2, w / 2, c, y_cs, y_off);
    reid_avgpool2_launch(xv, yv, n, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    reid_whole(yv, y);
    API_END(hh)
}

int eagle_op_reid_dw3(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, const float* wt, const float* b, int y_cs, int y_off, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!x || !wt || !b || !y) fail(EAGLE_E_INVALID, "eagle_op_reid_dw3: null argument");
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const TView xv = reid_view(net, "eagle_op_reid_dw3: x", x, n, h, w, c, x_cs, x_off);
    const TView yv = reid_view(net, "eagle_op_reid_dw3: y", nullptr, n, h, w, c, y_cs, y_off);
    const float* dw = (const float*)net.upload(wt, (size_t)9 * c * 4);
    const float* db = (const float*)net.upload(b, (size_t)c * 4);
    reid_dw3_launch(xv, dw, db, yv, n, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    reid_whole(yv, y);
    API_END(hh)
}

int eagle_op_reid_gate(int device, const float* const* streams, int n, int h, int w, int c, int x_cs, int x_off, const float* w1, const float* b1,
                       const float* w2, const float* b2, int c_real, int r, int y_cs, int y_off, float* g, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!streams || !streams[0] || !streams[1] || !streams[2] || !streams[3] || !w1 || !b1 || !w2 || !b2 || !g || !y) fail(EAGLE_E_INVALID, "eagle_op_reid_gate: null argument");
    if (c < 16 || c > 128 || 256 % c || c_real < 1 || c_real > c || r < 1 || r > 8)
        fail(EAGLE_E_INVALID, "eagle_op_reid_gate: c in {16, 32, 64, 128}, 1 <= c_real <= c and 1 <= r <= 8 required (c %d, c_real %d, r %d)", c, c_real, r);
    HIP_CHECK(hipSetDevice(device));
    Net net;
    TView sv[4];
    for (int k = 0; k < 4; ++k) sv[k] = reid_view(net, "eagle_op_reid_gate: stream", streams[k], n, h, w, c, x_cs, x_off);
    const TView yv = reid_view(net, "eagle_op_reid_gate: y", nullptr, n, h, w, c, y_cs, y_off);
    const float* d1 = (const float*)net.upload(w1, (size_t)r * c_real * 4);
    const float* e1 = (const float*)net.upload(b1, (size_t)r * 4);
    const float* d2 = (const float*)net.upload(w2, (size_t)c_real * r * 4);
    const float* e2 = (const float*)net.upload(b2, (size_t)c_real * 4);
    float* dg = reid_flat(net, (size_t)n * 4 * c);
    reid_gate_launch(sv, d1, e1, d2, e2, c_real, r, dg, yv, n, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(g, dg, (size_t)n * 4 * c * 4, hipMemcpyDeviceToHost));
    reid_whole(yv, y);
    API_END(hh)
}

int eagle_op_reid_head(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, const float* wt, const float* b, int dim, float* feats)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!x || !wt || !b || !feats || dim < 1) fail(EAGLE_E_INVALID, "eagle_op_reid_head: bad argument");
    if (c < 16 || c > 128 || 256 % c) fail(EAGLE_E_INVALID, "eagle_op_reid_head: c in {16, 32, 64, 128} required (c %d)", c);
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const TView xv = reid_view(net, "eagle_op_reid_head: x", x, n, h, w, c, x_cs, x_off);
    const float* dw = (const float*)net.upload(wt, (size_t)dim * c * 4);
    const float* db = (const float*)net.upload(b, (size_t)dim * 4);
    float* df = reid_flat(net, (size_t)n * dim);
    reid_head_launch(xv, dw, db, df, dim, n, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(feats, df, (size_t)n * dim * 4, hipMemcpyDeviceToHost));
    API_END(hh)
}

// ---- the detector's concat-by-slice path one launch at a time (tests/test_gpu_slices.py) -----------------------------------------------------
// The caller's whole buffers go through to_dev / from_dev (all three storage formats) and the launches get TView::slice views of them, as
// build_yolo / YoloBuilder::c2f make them: what lies outside a slice is the caller's (the tests' NaN) and comes back with the output buffer.
static void slice_check(const char* what, int prec, int n, int h, int w, int c, int cs, int off, int gran = 0)
{
    const int vn = prec == EAGLE_PREC_F32 ? 4 : 8;
    if (gran == 0) gran = vn;
    if (n < 1 || h < 1 || w < 1 || c < gran || c % gran || cs % vn || off % vn || off < 0 || cs < off + c)
        fail(EAGLE_E_INVALID, "%s: [%d, %d, %d, %d] at channel %d of %d: sizes >= 1; c a multiple of %d; cs, off multiples of %d; off + c <= cs", what, n, h, w, c, off, cs, gran, vn);
}
static void slice_disjoint(const char* what, int off_a, int c_a, int off_b, int c_b)
{
    if (off_a < off_b + c_b && off_b < off_a + c_a) fail(EAGLE_E_INVALID, "%s: channels %d..%d and %d..%d of one buffer overlap", what, off_a, off_a + c_a, off_b, off_b + c_b);
}
static TView whole_to_dev(Net& net, int prec, const float* src, int n, int h, int w, int cs)
{
    TView v;
    to_dev(net, prec, src, n, h, w, cs, cs, v);
    return v;
}
static void whole_from_dev(TView v, float* dst) { v.off = 0; v.c = v.cs; from_dev(v, v.cs, dst); }

int eagle_op_conv2d_sliced(int device, int precision, const float* x, int n, int h, int w, int cin, int x_cs, int x_off, const float* w_hwio, const float* bias,
                           int cout, int ks, int stride, int pre_act, const float* r1, int r1_cs, int r1_off, int r1_where,
                           const float* r2, int r2_cs, int r2_off, int r2_where, int post_act, int y_cs, int y_off, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!x || !w_hwio || !bias || !y || (ks != 1 && ks != 3) || stride < 1 || stride > 2 || precision < EAGLE_PREC_F16 || precision > EAGLE_PREC_F32S)
        fail(EAGLE_E_INVALID, "eagle_op_conv2d_sliced: bad argument (ks 1 or 3, stride 1 or 2)");
    const int ho = (h + 2 * (ks / 2) - ks) / stride + 1, wo = (w + 2 * (ks / 2) - ks) / stride + 1;
    slice_check("eagle_op_conv2d_sliced: x", precision, n, h, w, cin, x_cs, x_off, 16);
    slice_check("eagle_op_conv2d_sliced: y", precision, n, ho, wo, cout, y_cs, y_off, 16);
    const float* rp[2] = {r1, r2};
    int rcs[2] = {r1_cs, r2_cs};
    const int roff[2] = {r1_off, r2_off}, rwhere[2] = {r1_where, r2_where};
    bool has[2];
    for (int k = 0; k < 2; ++k) {
        has[k] = rp[k] || rwhere[k] != EAGLE_OP_RES_OWN;
        if (!has[k]) continue;
        if (rwhere[k] == EAGLE_OP_RES_IN_Y) rcs[k] = y_cs;
        else if (rwhere[k] == EAGLE_OP_RES_IN_X) {
            if (ho != h || wo != w) fail(EAGLE_E_INVALID, "eagle_op_conv2d_sliced: a residual inside the input buffer needs an output of the input's size");
            rcs[k] = x_cs;
        } else if (rwhere[k] != EAGLE_OP_RES_OWN) fail(EAGLE_E_INVALID, "eagle_op_conv2d_sliced: residual placement %d", rwhere[k]);
        slice_check("eagle_op_conv2d_sliced: residual", precision, n, ho, wo, cout, rcs[k], roff[k], 16);
        if (rwhere[k] == EAGLE_OP_RES_IN_Y) slice_disjoint("eagle_op_conv2d_sliced: residual and output", roff[k], cout, y_off, cout);
    }
    HIP_CHECK(hipSetDevice(device));
    Net net;
    ConvLaunch L;
    const TView xb = whole_to_dev(net, precision, x, n, h, w, x_cs);
    const TView yb = whole_to_dev(net, precision, y, n, ho, wo, y_cs);
    L.x = xb.slice(x_off, cin);
    L.y = yb.slice(y_off, cout);
    TView* rv[2] = {&L.r1, &L.r2};
    for (int k = 0; k < 2; ++k) {
        if (!has[k]) continue;
        const TView base = rwhere[k] == EAGLE_OP_RES_IN_Y ? yb : rwhere[k] == EAGLE_OP_RES_IN_X ? xb : whole_to_dev(net, precision, rp[k], n, ho, wo, rcs[k]);
        *rv[k] = base.slice(roff[k], cout);
    }
    L.cfg = conv_choose(precision, ks, stride, cin, cout, wo, pre_act == ACT_NONE && post_act <= ACT_RELU, has[0] && has[1]);      // as Builder::conv: the slice's channel counts
    if (!conv_supported(precision, L.cfg)) fail(EAGLE_E_NOKERNEL, "no kernel instance ks=%d s=%d kc=%d nt=%d", ks, stride, L.cfg.kc, L.cfg.nt);
    std::vector<char> tiled(conv_weight_elems(precision, L.cfg) * (precision == EAGLE_PREC_F32 ? 4 : 2));
    conv_tile_weights(precision, L.cfg, w_hwio, cin, cout, tiled.data(), &L.descale);
    L.w = net.upload(tiled.data(), tiled.size());
    L.bias = (const float*)net.upload(bias, (size_t)cout * 4);
    L.pre_act = pre_act; L.post_act = post_act;
    conv_launch(precision, L, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    whole_from_dev(yb, y);
    API_END(hh)
}

// x -> y of one element-wise launch: y is the caller's in/out buffer, or (same_buffer) the input buffer itself
static void slice_pair(Net& net, const char* what, int prec_x, int prec_y, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int same_buffer,
                       int yh, int yw, int y_cs, int y_off, const float* y, TView& xv, TView& yv)
{
    if (!x || !y) fail(EAGLE_E_INVALID, "%s: null argument", what);
    if (same_buffer && (y_cs != x_cs || yh != h || yw != w || prec_x != prec_y)) fail(EAGLE_E_INVALID, "%s: slices of one buffer share its size, stride and format", what);
    slice_check(what, prec_x, n, h, w, c, x_cs, x_off);
    slice_check(what, prec_y, n, yh, yw, c, y_cs, y_off, prec_x == EAGLE_PREC_F32 ? 4 : 8);
    if (same_buffer) slice_disjoint(what, x_off, c, y_off, c);
    const TView xb = whole_to_dev(net, prec_x, x, n, h, w, x_cs);
    const TView yb = same_buffer ? xb : whole_to_dev(net, prec_y, y, n, yh, yw, y_cs);
    xv = xb.slice(x_off, c); yv = yb.slice(y_off, c);
}

int eagle_op_maxpool5(int device, int precision, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int same_buffer, int y_cs, int y_off, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (precision < EAGLE_PREC_F16 || precision > EAGLE_PREC_F32S) fail(EAGLE_E_INVALID, "eagle_op_maxpool5: precision %d", precision);
    HIP_CHECK(hipSetDevice(device));
    Net net;
    TView xv, yv;
    slice_pair(net, "eagle_op_maxpool5", precision, precision, x, n, h, w, c, x_cs, x_off, same_buffer, h, w, y_cs, y_off, y, xv, yv);
    maxpool5_launch(xv, yv, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    whole_from_dev(yv, y);
    API_END(hh)
}

int eagle_op_upsample2(int device, int precision, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int same_buffer, int yh, int yw, int y_cs, int y_off, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (precision < EAGLE_PREC_F16 || precision > EAGLE_PREC_F32S) fail(EAGLE_E_INVALID, "eagle_op_upsample2: precision %d", precision);
    if (h < 1 || w < 1 || (yh != 2 * h - 1 && yh != 2 * h) || (yw != 2 * w - 1 && yw != 2 * w))
        fail(EAGLE_E_INVALID, "eagle_op_upsample2: a %d x %d map goes to {%d, %d} x {%d, %d}, not %d x %d", h, w, 2 * h - 1, 2 * h, 2 * w - 1, 2 * w, yh, yw);
    HIP_CHECK(hipSetDevice(device));
    Net net;
    TView xv, yv;
    slice_pair(net, "eagle_op_upsample2", precision, precision, x, n, h, w, c, x_cs, x_off, same_buffer, yh, yw, y_cs, y_off, y, xv, yv);
    yv.h = yh; yv.w = yw;
    upsample2_launch(xv, yv, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    whole_from_dev(yv, y);
    API_END(hh)
}

int eagle_op_split_to_f32(int device, const float* x, int n, int h, int w, int c, int x_cs, int x_off, int y_cs, int y_off, float* y)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    HIP_CHECK(hipSetDevice(device));
    Net net;
    TView xv, yv;
    slice_pair(net, "eagle_op_split_to_f32", EAGLE_PREC_F32S, EAGLE_PREC_F32, x, n, h, w, c, x_cs, x_off, 0, h, w, y_cs, y_off, y, xv, yv);
    split_to_f32_launch(xv, yv, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    whole_from_dev(yv, y);
    API_END(hh)
}

}  // extern "C"
