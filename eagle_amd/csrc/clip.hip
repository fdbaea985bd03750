// The clip session of the optical-flow cadence (eagle_clip_*), the tracker entries (eagle_track_*) and the per-clip operators next to them
// (re-projection, team colours, appearance embeddings).
#include "runtime.h"

namespace eagle {

// ---- clip session (optical-flow cadence) ----------------------------------------------------------------------------------
// Three streams: s_det runs the detector pass, s_main the HRNet pass (+ gray pyramids, operator calls), s_post the sequential
// loop body (K12 + K13 per frame).  The passes of later frames overlap the loop of earlier ones; events order them.
// h->prof off for a scope (the passes of a clip session and the appearance network run unprofiled): restored on every exit path, a fail() included
struct ProfOff { EagleHandle* h; bool was; explicit ProfOff(EagleHandle* h_) : h(h_), was(h_->prof) { h->prof = false; } ~ProfOff() { h->prof = was; } };

static void clip_sync(EagleHandle* h)
{
    HIP_CHECK(hipStreamSynchronize(h->s_det));
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    HIP_CHECK(hipStreamSynchronize(h->s_post));
}

void clip_close(EagleHandle* h)
{
    EagleHandle::Clip& c = h->clip;
    if (c.open) { (void)hipStreamSynchronize(h->s_det); (void)hipStreamSynchronize(h->s_main); (void)hipStreamSynchronize(h->s_post); }
    for (auto& p : c.g) { if (p) (void)hipFree(p); p = nullptr; }
    if (c.recs) (void)hipFree(c.recs);
    if (c.mem) (void)hipFree(c.mem);
    if (c.st) (void)hipFree(c.st);
    if (c.st_op) (void)hipFree(c.st_op);
    if (c.h_st) (void)hipHostFree(c.h_st);
    if (c.h_zero) (void)hipHostFree(c.h_zero);
    if (c.h_tail) (void)hipHostFree(c.h_tail);
    if (c.h_mem) (void)hipHostFree(c.h_mem);
    if (c.ecc_small) (void)hipFree(c.ecc_small);
    if (c.ecc_pairs) (void)hipFree(c.ecc_pairs);
    if (c.ecc_out) (void)hipFree(c.ecc_out);
    for (hipEvent_t e : {c.ev_gray, c.ev_det, c.ev_kp, c.ev_loop}) if (e) (void)hipEventDestroy(e);
    c = EagleHandle::Clip();
}

static void clip_open(EagleHandle* h, const uint8_t* d_bgr, int n)
{
    clip_close(h);
    const EagleConfig& cf = h->cfg;
    EagleHandle::Clip& c = h->clip;
    c.cv.bgr = d_bgr; c.cv.n = n; c.cv.h = cf.frame_h; c.cv.w = cf.frame_w;
    clip_view_levels(c.cv);
    c.open = true;
    for (int l = 0; l < 3; ++l) {
        HIP_CHECK(hipMalloc((void**)&c.g[l], std::max<size_t>((size_t)n * c.cv.lh[l] * c.cv.lw[l], 16)));
        c.cv.g[l] = c.g[l];
    }
    const size_t nn = (size_t)std::max(n, 1);
    HIP_CHECK(hipMalloc((void**)&c.recs, sizeof(EagleFrameResult) * nn));
    HIP_CHECK(hipMalloc((void**)&c.mem, sizeof(MemList) * nn));
    HIP_CHECK(hipMalloc((void**)&c.st, sizeof(ChainState)));
    HIP_CHECK(hipMalloc((void**)&c.st_op, sizeof(ChainState)));
    HIP_CHECK(hipHostMalloc((void**)&c.h_st, sizeof(ChainState), hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void**)&c.h_zero, sizeof(ChainState), hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void**)&c.h_tail, sizeof(int) * 4, hipHostMallocDefault));
    HIP_CHECK(hipHostMalloc((void**)&c.h_mem, sizeof(MemList), hipHostMallocDefault));
    memset(c.h_zero, 0, sizeof(ChainState));
    c.h_zero->stalled = -1;
    c.h_tail[0] = -1; c.h_tail[1] = 0; c.h_tail[2] = -1;
    for (hipEvent_t* e : {&c.ev_gray, &c.ev_det, &c.ev_kp, &c.ev_loop}) HIP_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    HIP_CHECK(hipMemsetAsync(c.mem, 0xFF, sizeof(MemList) * nn, h->s_main));                  // n = -1 everywhere
    HIP_CHECK(hipMemsetAsync(c.recs, 0, sizeof(EagleFrameResult) * nn, h->s_main));
    HIP_CHECK(hipMemsetAsync(h->clip_sat, 0, sat_pad_bytes(cf.batch), h->s_main));
    HIP_CHECK(hipMemcpyAsync(c.st, c.h_zero, sizeof(ChainState), hipMemcpyHostToDevice, h->s_main));
    if (n > 0) gray_pyramid_launch(d_bgr, n, c.cv.h, c.cv.w, c.g[0], c.g[1], c.g[2], h->s_main);
    HIP_CHECK(hipEventRecord(c.ev_gray, h->s_main));
    HIP_CHECK(hipStreamWaitEvent(h->s_det, c.ev_gray, 0));       // the record memset precedes the first detector write
    HIP_CHECK(hipEventRecord(c.ev_det, h->s_det));
    HIP_CHECK(hipEventRecord(c.ev_kp, h->s_main));
    HIP_CHECK(hipEventRecord(c.ev_loop, h->s_post));
}

// detector + decode + NMS + object rules of frames [first, first+count) (cm.py:331 detect_objects), records kept in HBM; asynchronous
static void clip_detect_objects(EagleHandle* h, int first, int count)
{
    const EagleConfig& cf = h->cfg;
    EagleHandle::Clip& c = h->clip;
    const int B = cf.batch;
    const size_t fb = (size_t)cf.frame_h * cf.frame_w * 3;
    size_t ev_i = 0;
    EagleHandle::StepBuf& sb = h->sb[0];
    ProfOff prof_off(h);
    h->cur_sat = h->clip_sat;
    // The passes of later chunks run under the sequential loop of earlier frames (three streams).  Round 1 had to serialise them
    // behind the loop because K12 was not reproducible next to the convolution kernels; the cause was the packed-fp32 code hipcc's
    // SLP vectoriser generated for K12 (Makefile), not the overlap.
    for (int i = first; i < first + count; i += B) {
        const int na = std::min(B, first + count - i);
        HIP_CHECK(hipMemsetAsync(sb.d_out, 0, sizeof(EagleFrameResult) * B, h->s_det));
        preprocess_launch(h->det_prec, c.cv.bgr + (size_t)i * fb, na, cf.frame_h, cf.frame_w, h->kp_in, h->det_in, h->lb, h->s_det, 2);
        run_net(h, h->yo.get(), h->s_det, ev_i);
        yolo_decode_launch(h->levels, 3, B, 5, cf.detector_floor, h->ds, h->s_det);
        nms_launch(h->ds, B, h->pp, sb.d_out, h->s_det);
        HIP_CHECK(hipMemcpyAsync(c.recs + i, sb.d_out, sizeof(EagleFrameResult) * na, hipMemcpyDeviceToDevice, h->s_det));
    }
    HIP_CHECK(hipEventRecord(c.ev_det, h->s_det));
}

// HRNet + heat-map maxima + decode of frames first, first+stride, ... -> mem[]; asynchronous
static void clip_detect_keypoints(EagleHandle* h, int first, int stride, int count)
{
    const EagleConfig& cf = h->cfg;
    EagleHandle::Clip& c = h->clip;
    const int B = cf.batch;
    const size_t fb = (size_t)cf.frame_h * cf.frame_w * 3;
    size_t ev_i = 0;
    EagleHandle::StepBuf& sb = h->sb[0];
    ProfOff prof_off(h);
    h->cur_sat = h->clip_sat;
    for (int k0 = 0; k0 < count; k0 += B) {
        const int na = std::min(B, count - k0);
        const uint8_t* src;
        if (stride == 1) src = c.cv.bgr + (size_t)(first + k0) * fb;
        else {
            for (int k = 0; k < na; ++k)
                HIP_CHECK(hipMemcpyAsync(sb.d_frames + (size_t)k * fb, c.cv.bgr + (size_t)(first + (k0 + k) * stride) * fb, fb, hipMemcpyDeviceToDevice, h->s_main));
            src = sb.d_frames;
        }
        h->cur_src = src; h->cur_n = na;
        if (!h->stem_on) preprocess_launch(h->prec, src, na, cf.frame_h, cf.frame_w, h->kp_in, h->det_in, h->lb, h->s_main, 1);      // (the fused stem reads the frames itself)
        h->cur_parts = sb.parts;
        run_net(h, h->hr.get(), h->s_main, ev_i);
        if (!h->fused_argmax) heat_argmax_launch(h->logits, sb.parts, h->hm_chunks, h->s_main);
        decode_mem_launch(sb.parts, na, h->pp, c.mem, first + k0 * stride, stride, h->s_main);
    }
    HIP_CHECK(hipEventRecord(c.ev_kp, h->s_main));
}

}  // namespace eagle

extern "C" {

int eagle_reproject(EagleHandle* h, EagleFrameResult* recs, int n, const double* Hs, const uint8_t* flags)
{
    API_BEGIN_H(h)
    if (!recs || !Hs || !flags || n < 0) fail(EAGLE_E_INVALID, "bad argument");
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    Net scratch;                                          // owns the three device buffers: freed on every exit path
    EagleFrameResult* d_r = (EagleFrameResult*)scratch.get(sizeof(EagleFrameResult) * (size_t)n);
    double* d_H = (double*)scratch.get(sizeof(double) * 9 * (size_t)n);
    unsigned char* d_f = (unsigned char*)scratch.get((size_t)n);
    HIP_CHECK(hipMemcpyAsync(d_r, recs, sizeof(EagleFrameResult) * (size_t)n, hipMemcpyHostToDevice, h->s_main));
    HIP_CHECK(hipMemcpyAsync(d_H, Hs, sizeof(double) * 9 * (size_t)n, hipMemcpyHostToDevice, h->s_main));
    HIP_CHECK(hipMemcpyAsync(d_f, flags, (size_t)n, hipMemcpyHostToDevice, h->s_main));
    reproject_launch(d_r, d_H, d_f, n, h->cfg.frame_h, h->cfg.frame_w, h->s_main);
    HIP_CHECK(hipMemcpyAsync(recs, d_r, sizeof(EagleFrameResult) * (size_t)n, hipMemcpyDeviceToHost, h->s_main));
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    API_END(h)
}

int eagle_team_colors(EagleHandle* h, const void* d_bgr, int n_frames, const EagleCrop* crops, int n_crops, int32_t* counts)
{
    API_BEGIN_H(h)
    if (!d_bgr || n_frames < 0 || n_crops < 0 || (n_crops > 0 && (!crops || !counts))) fail(EAGLE_E_INVALID, "bad argument");
    if (n_crops == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    Net scratch;
    EagleCrop* d_c = (EagleCrop*)scratch.get(sizeof(EagleCrop) * (size_t)n_crops);
    int* d_n = (int*)scratch.get(sizeof(int) * 12 * (size_t)n_crops);
    HIP_CHECK(hipMemcpyAsync(d_c, crops, sizeof(EagleCrop) * (size_t)n_crops, hipMemcpyHostToDevice, h->s_main));
    eagle::team_colors_launch((const uint8_t*)d_bgr, n_frames, h->cfg.frame_h, h->cfg.frame_w, d_c, n_crops, d_n, h->s_main);
    HIP_CHECK(hipMemcpyAsync(counts, d_n, sizeof(int) * 12 * (size_t)n_crops, hipMemcpyDeviceToHost, h->s_main));
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    API_END(h)
}

int eagle_reid_features(EagleHandle* h, const void* d_bgr, int n_frames, const EagleCrop* crops, int n_crops, float* feats)
{
    API_BEGIN_H(h)
    if (!h->finalized || !h->reid) fail(EAGLE_E_STATE, "no appearance network: load the reid.* tensors (OSNet-x0.25, torchreid names) before eagle_finalize_weights");
    if (n_frames < 0 || n_crops < 0 || (n_crops > 0 && (!d_bgr || !crops || !feats))) fail(EAGLE_E_INVALID, "bad argument");
    if (n_crops == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(h->cfg.device));
    eagle::ProfOff prof_off(h);
    for (int i0 = 0; i0 < n_crops; i0 += eagle::REID_NB) {
        const int nb = std::min(eagle::REID_NB, n_crops - i0);
        for (int k = 0; k < eagle::REID_NB; ++k) {
            EagleCrop c = {-1, 0, 0, 0, 0};
            if (k < nb) c = crops[i0 + k];
            h->reid_crops_h[k] = c;
        }
        HIP_CHECK(hipMemcpyAsync(h->reid_crops, h->reid_crops_h, sizeof(EagleCrop) * eagle::REID_NB, hipMemcpyHostToDevice, h->s_main));
        eagle::reid_crop_launch((const uint8_t*)d_bgr, n_frames, h->cfg.frame_h, h->cfg.frame_w, h->reid_crops, eagle::REID_NB, h->reid_in, h->s_main);
        size_t ev_i = 0;
        eagle::run_net(h, h->reid.get(), h->s_main, ev_i);
        HIP_CHECK(hipMemcpyAsync(h->reid_feats_h, h->reid_feats, sizeof(float) * EAGLE_REID_DIM * (size_t)nb, hipMemcpyDeviceToHost, h->s_main));
        HIP_CHECK(hipStreamSynchronize(h->s_main));
        memcpy(feats + (size_t)i0 * EAGLE_REID_DIM, h->reid_feats_h, sizeof(float) * EAGLE_REID_DIM * (size_t)nb);
    }
    API_END(h)
}

int eagle_track_open(EagleHandle* h, const EagleTrackParams* params)
{
    API_BEGIN_H(h)
    if (h->tracker) eagle::tracker_destroy(h->tracker);
    h->tracker = eagle::tracker_create(params);
    h->ecc_has_prev = false;                              // a new BotSort builds a new ECC estimator
    API_END(h)
}

int eagle_track_frames(EagleHandle* h, EagleFrameResult* recs, int n) { return eagle_track_frames_cmc(h, recs, n, nullptr); }

int eagle_track_frames_cmc(EagleHandle* h, EagleFrameResult* recs, int n, const double* warps) { return eagle_track_frames_reid(h, recs, n, warps, nullptr, nullptr, nullptr); }

int eagle_track_frames_reid(EagleHandle* h, EagleFrameResult* recs, int n, const double* warps, const float* feats, const int32_t* feat_det, const int32_t* feat_count)
{
    API_BEGIN_H(h)
    if (!recs || n < 0 || (feats && (!feat_det || !feat_count))) fail(EAGLE_E_INVALID, "bad argument");
    if (!h->tracker) fail(EAGLE_E_STATE, "eagle_track_open has not been called");
    if (n == 0) return EAGLE_OK;
    if (feats)                                               // the caller's index arrays are untrusted: validate before anything is dereferenced
        for (int i = 0; i < n; ++i) {
            if (feat_count[i] < 0 || feat_count[i] > EAGLE_MAX_DET) fail(EAGLE_E_INVALID, "eagle_track_frames_reid: feat_count[%d] = %d", i, feat_count[i]);
            if (recs[i].n_det < 0 || recs[i].n_det > EAGLE_MAX_DET) fail(EAGLE_E_INVALID, "eagle_track_frames_reid: record %d has n_det = %d", i, recs[i].n_det);
        }
    if (feats) {
        size_t o = 0;
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < feat_count[i]; ++k, ++o)
                if (feat_det[o] < 0 || feat_det[o] >= recs[i].n_det)
                    fail(EAGLE_E_INVALID, "eagle_track_frames_reid: feat_det[%zu] = %d is not a detection of record %d (n_det %d)", o, feat_det[o], i, recs[i].n_det);
    }
    std::vector<double> Hs((size_t)n * 9, 0.0);
    std::vector<uint8_t> flags((size_t)n, 0);
    bool any = false;
    size_t fo = 0;                                           // running offset into feats / feat_det
    for (int i = 0; i < n; ++i) {
        const int nf = feats ? feat_count[i] : 0;
        const bool applied = eagle::tracker_apply(h->tracker, recs + i, h->cfg.frame_h, h->cfg.frame_w, h->cfg.detector_conf, warps ? warps + (size_t)i * 6 : nullptr,
                                                  feats ? feats + fo * EAGLE_REID_DIM : nullptr, feats ? feat_det + fo : nullptr, nf);
        fo += (size_t)nf;
        if (!applied) continue;
        any = true;
        flags[i] = recs[i].H_valid ? 1 : 2;                  // re-project the moved foot points with the frame's own homography
        memcpy(&Hs[(size_t)i * 9], recs[i].H, sizeof(double) * 9);
    }
    if (any) {
        const int rc = eagle_reproject(h, recs, n, Hs.data(), flags.data());
        if (rc) return rc;
    }
    API_END(h)
}

#define CLIP_CHECK(h, cond, msg) if (!(h) || !(h)->finalized) return EAGLE_E_STATE; if (!(cond)) { (h)->err = msg; return EAGLE_E_INVALID; }
int eagle_clip_open(EagleHandle* h, const void* d_bgr, int n)
{
    CLIP_CHECK(h, n >= 0 && (d_bgr || n == 0), "eagle_clip_open: bad arguments")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    eagle::clip_open(h, (const uint8_t*)d_bgr, n);
    API_END(h)
}

int eagle_clip_close(EagleHandle* h)
{
    API_BEGIN_H(h)
    HIP_CHECK(hipSetDevice(h->cfg.device));
    eagle::clip_close(h);
    API_END(h)
}

int eagle_clip_detect_objects(EagleHandle* h, int first, int count)
{
    CLIP_CHECK(h, h->clip.open && first >= 0 && count >= 0 && first + (int64_t)count <= h->clip.cv.n, "eagle_clip_detect_objects: no open clip or frames out of range")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    eagle::clip_detect_objects(h, first, count);
    API_END(h)
}

int eagle_clip_detect_keypoints(EagleHandle* h, int first, int stride, int count)
{
    CLIP_CHECK(h, h->clip.open && first >= 0 && stride >= 1 && count >= 0 && (count == 0 || first + (int64_t)(count - 1) * stride < h->clip.cv.n),
               "eagle_clip_detect_keypoints: no open clip or frames out of range")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    eagle::clip_detect_keypoints(h, first, stride, count);
    API_END(h)
}

int eagle_clip_get_keypoints(EagleHandle* h, int frame, EagleFlowKp* out, int* n)
{
    CLIP_CHECK(h, h->clip.open && frame >= 0 && frame < h->clip.cv.n && out && n, "eagle_clip_get_keypoints: bad arguments")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    MemList& m = *h->clip.h_mem;                          // mem[] is written on s_main (key-point passes, eagle_clip_set_keypoints)
    HIP_CHECK(hipMemcpyAsync(&m, h->clip.mem + frame, sizeof(m), hipMemcpyDeviceToHost, h->s_main));
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    *n = m.n;
    for (int k = 0; k < m.n && k < EAGLE_N_LANDMARKS; ++k) out[k] = m.kp[k];
    API_END(h)
}

int eagle_clip_set_keypoints(EagleHandle* h, int frame, const EagleFlowKp* in, int n)
{
    CLIP_CHECK(h, h->clip.open && frame >= 0 && frame < h->clip.cv.n && n >= -1 && n <= EAGLE_N_LANDMARKS && (in || n <= 0),
               "eagle_clip_set_keypoints: bad arguments")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    HIP_CHECK(hipStreamSynchronize(h->s_main));           // the staging buffer is free again
    HIP_CHECK(hipStreamSynchronize(h->s_post));           // no loop launch still reads the old entry
    MemList& m = *h->clip.h_mem;
    memset(&m, 0, sizeof(m));
    m.n = n;
    for (int k = 0; k < n; ++k) m.kp[k] = in[k];
    HIP_CHECK(hipMemcpyAsync(h->clip.mem + frame, &m, sizeof(m), hipMemcpyHostToDevice, h->s_main));
    HIP_CHECK(hipEventRecord(h->clip.ev_kp, h->s_main));      // eagle_clip_run orders the loop behind this write
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    API_END(h)
}

int eagle_clip_flow(EagleHandle* h, int src_frame, int dst_frame, int hue_frame, const EagleFlowKp* in, int n_in,
                    EagleFlowKp* out, int* n_out, float* next_pts, uint8_t* status)
{
    CLIP_CHECK(h, h->clip.open && src_frame >= 0 && src_frame < h->clip.cv.n && dst_frame >= 0 && dst_frame < h->clip.cv.n && hue_frame >= 0 &&
               hue_frame < h->clip.cv.n && n_in >= 0 && n_in <= EAGLE_N_LANDMARKS && (in || n_in == 0) && out && n_out,
               "eagle_clip_flow: bad arguments")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    EagleHandle::Clip& c = h->clip;
    *n_out = 0;
    if (n_in == 0) return EAGLE_OK;                       // cm.py:429: empty dict in -> empty dict out
    ChainState& z = *c.h_st;                              // (stream-ordered on s_main behind the gray pyramids; independent of the loop's state)
    memset(&z, 0, sizeof(z));
    z.stalled = -1; z.n_prev = n_in;
    for (int k = 0; k < n_in; ++k) z.prev[k] = in[k];
    HIP_CHECK(hipMemcpyAsync(c.st_op, &z, sizeof(z), hipMemcpyHostToDevice, h->s_main));
    lk_launch(c.cv, src_frame, dst_frame, c.st_op, nullptr, 1, h->s_main);
    flow_filter_launch(c.cv, c.st_op, hue_frame, h->s_main);
    HIP_CHECK(hipMemcpyAsync(&z, c.st_op, sizeof(z), hipMemcpyDeviceToHost, h->s_main));
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    *n_out = z.flow_n;
    for (int k = 0; k < z.flow_n; ++k) out[k] = z.flow[k];
    if (next_pts) memcpy(next_pts, z.lk_next, sizeof(float) * 2 * n_in);
    if (status) memcpy(status, z.lk_status, n_in);
    API_END(h)
}

int eagle_clip_motion(EagleHandle* h, int first, int count, double* warps)
{
    CLIP_CHECK(h, h->clip.open && first >= 0 && count >= 0 && first + count <= h->clip.cv.n && (warps || count == 0), "eagle_clip_motion: bad arguments")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    EagleHandle::Clip& c = h->clip;
    constexpr int GW = 8, GH = 6, NP = GW * GH;              // 48 grid points: one launch of the key-point LK kernel (<= EAGLE_N_LANDMARKS)
    ChainState& z = *c.h_st;
    for (int i = 0; i < count; ++i) {
        double* W = warps + (size_t)i * 6;
        W[0] = 1; W[1] = 0; W[2] = 0; W[3] = 0; W[4] = 1; W[5] = 0;
        const int f = first + i;
        if (f == 0) continue;
        memset(&z, 0, sizeof(z));
        z.stalled = -1; z.n_prev = NP;
        for (int gy = 0; gy < GH; ++gy)
            for (int gx = 0; gx < GW; ++gx) {
                EagleFlowKp& k = z.prev[gy * GW + gx];
                k.label = gy * GW + gx; k.score = 1.f;
                k.x = (int)floor((gx + 0.5) * h->cfg.frame_w / GW); k.y = (int)floor((gy + 0.5) * h->cfg.frame_h / GH);
            }
        HIP_CHECK(hipMemcpyAsync(c.st_op, &z, sizeof(z), hipMemcpyHostToDevice, h->s_main));
        lk_launch(c.cv, f - 1, f, c.st_op, nullptr, 1, h->s_main);
        HIP_CHECK(hipMemcpyAsync(&z, c.st_op, sizeof(z), hipMemcpyDeviceToHost, h->s_main));
        HIP_CHECK(hipStreamSynchronize(h->s_main));
        double p0[2 * NP], p1[2 * NP]; int m = 0;
        for (int k = 0; k < NP; ++k)
            if (z.lk_status[k] == 1) { p0[2 * m] = z.prev[k].x; p0[2 * m + 1] = z.prev[k].y; p1[2 * m] = z.lk_next[2 * k]; p1[2 * m + 1] = z.lk_next[2 * k + 1]; ++m; }
        eagle::similarity_ransac(p0, p1, m, W);
    }
    API_END(h)
}

int eagle_clip_motion_ecc(EagleHandle* h, int first, int count, int carry, double* warps, int* ok_out)
{
    CLIP_CHECK(h, h->clip.open && first >= 0 && count >= 0 && first + count <= h->clip.cv.n && (warps || count == 0), "eagle_clip_motion_ecc: bad arguments")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    EagleHandle::Clip& c = h->clip;
    constexpr double SCALE = 0.15, EPS = 1e-5; constexpr int MAX_ITER = 100;      // boxmot ECC(): scale 0.15, (EPS | COUNT, 100, 1e-5)
    const int dh = (int)lrint(c.cv.h * SCALE), dw = (int)lrint(c.cv.w * SCALE), n = c.cv.n;
    if (dh < 4 || dw < 4) fail(EAGLE_E_INVALID, "eagle_clip_motion_ecc: frame too small for the 0.15-scale alignment");
    hipStream_t sm = h->s_main;
    if (c.ecc_h == 0 && n > 0) {                          // first call of the session (ecc_h is set last: a failed allocation is retried, not half-used)
        if (!c.ecc_small) HIP_CHECK(hipMalloc(&c.ecc_small, (size_t)n * dh * dw));
        if (!c.ecc_pairs) HIP_CHECK(hipMalloc(&c.ecc_pairs, sizeof(int2) * n));
        if (!c.ecc_out) HIP_CHECK(hipMalloc(&c.ecc_out, sizeof(eagle::EccResult) * n));
        HIP_CHECK(hipStreamWaitEvent(sm, c.ev_gray, 0));
        eagle::ecc_small_launch(c.g[0], c.ecc_small, n, c.cv.h, c.cv.w, dh, dw, 1.0 / SCALE, sm);
        c.ecc_h = dh; c.ecc_w = dw;
    }
    const bool use_carry = carry && h->ecc_has_prev && h->ecc_prev_h == dh && h->ecc_prev_w == dw;
    // every adjacent pair at once; pairs behind a failed alignment (boxmot keeps the old template) are re-run one by one below
    std::vector<int2> pairs; std::vector<int> slot(count, -1);
    for (int i = 0; i < count; ++i) {
        const int f = first + i;
        if (f > 0) { slot[i] = (int)pairs.size(); pairs.push_back(make_int2(f - 1, f)); }
        else if (use_carry) { slot[i] = (int)pairs.size(); pairs.push_back(make_int2(-1, f)); }
    }
    std::vector<eagle::EccResult> res(pairs.size());
    if (!pairs.empty()) {
        HIP_CHECK(hipMemcpyAsync(c.ecc_pairs, pairs.data(), sizeof(int2) * pairs.size(), hipMemcpyHostToDevice, sm));
        eagle::ecc_launch(c.ecc_small, h->ecc_prev, c.ecc_pairs, (int)pairs.size(), c.ecc_out, dh, dw, MAX_ITER, EPS, sm);
        HIP_CHECK(hipMemcpyAsync(res.data(), c.ecc_out, sizeof(eagle::EccResult) * pairs.size(), hipMemcpyDeviceToHost, sm));
        HIP_CHECK(hipStreamSynchronize(sm));
    }
    constexpr int NONE = -2;
    int prev = first > 0 ? first - 1 : (use_carry ? -1 : NONE);
    if (first > 0 && c.ecc_next == first && c.ecc_tmpl != NONE && (c.ecc_tmpl >= 0 || use_carry)) prev = c.ecc_tmpl;   // the previous range ended behind a failed alignment
    for (int i = 0; i < count; ++i) {
        const int f = first + i;
        double* W = warps + (size_t)i * 6;
        W[0] = 1; W[1] = 0; W[2] = 0; W[3] = 0; W[4] = 1; W[5] = 0;
        if (ok_out) ok_out[i] = 1;
        if (prev == NONE) { prev = f; continue; }        // the estimator's first frame: identity, becomes the template
        eagle::EccResult r;
        if (slot[i] >= 0 && pairs[slot[i]].x == prev) r = res[slot[i]];
        else {
            const int2 one = make_int2(prev, f);
            HIP_CHECK(hipMemcpyAsync(c.ecc_pairs, &one, sizeof(one), hipMemcpyHostToDevice, sm));
            eagle::ecc_launch(c.ecc_small, h->ecc_prev, c.ecc_pairs, 1, c.ecc_out, dh, dw, MAX_ITER, EPS, sm);
            HIP_CHECK(hipMemcpyAsync(&r, c.ecc_out, sizeof(r), hipMemcpyDeviceToHost, sm));
            HIP_CHECK(hipStreamSynchronize(sm));
        }
        if (!r.ok) { if (ok_out) ok_out[i] = 0; continue; }     // cv2 raised: identity, template unchanged
        for (int k = 0; k < 6; ++k) W[k] = (double)r.M[k];
        W[2] = (double)(float)((double)r.M[2] / SCALE); W[5] = (double)(float)((double)r.M[5] / SCALE);   // warp_matrix[i, 2] /= self.scale
        prev = f;
    }
    if (count > 0) { c.ecc_next = first + count; c.ecc_tmpl = prev; }
    if (carry && prev != NONE && prev != -1) {
        if (!h->ecc_prev || h->ecc_prev_h != dh || h->ecc_prev_w != dw) {
            if (h->ecc_prev) HIP_CHECK(hipFree(h->ecc_prev));
            h->ecc_prev = nullptr;
            HIP_CHECK(hipMalloc(&h->ecc_prev, (size_t)dh * dw));
            h->ecc_prev_h = dh; h->ecc_prev_w = dw;
        }
        HIP_CHECK(hipMemcpyAsync(h->ecc_prev, c.ecc_small + (size_t)prev * dh * dw, (size_t)dh * dw, hipMemcpyDeviceToDevice, sm));
        HIP_CHECK(hipStreamSynchronize(sm));
        h->ecc_has_prev = true;
    }
    API_END(h)
}

int eagle_clip_run(EagleHandle* h, int first, int last, int keypoint_interval, int homography_interval, int calibration, int wait, int* stalled_at)
{
    CLIP_CHECK(h, h->clip.open && first >= 0 && first <= last && last <= h->clip.cv.n && keypoint_interval >= 1 && homography_interval >= 1,
               "eagle_clip_run: bad arguments")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    EagleHandle::Clip& c = h->clip;
    hipStream_t sp = h->s_post;
    HIP_CHECK(hipStreamWaitEvent(sp, c.ev_gray, 0));
    HIP_CHECK(hipStreamWaitEvent(sp, c.ev_det, 0));       // every detector / HRNet pass enqueued so far
    HIP_CHECK(hipStreamWaitEvent(sp, c.ev_kp, 0));
    if (first < last) {
        if (first == 0) HIP_CHECK(hipMemcpyAsync(c.st, c.h_zero, sizeof(ChainState), hipMemcpyHostToDevice, sp));
        else if (wait) HIP_CHECK(hipMemcpyAsync((char*)c.st + offsetof(ChainState, stalled), &c.h_tail[2], sizeof(int), hipMemcpyHostToDevice, sp));   // resume
        // (an asynchronous call for a later chunk must NOT clear the flag: if an earlier chunk stalled, its launches have to fall through too)
    }
    for (int i = first; i < last; ++i) {
        lk_launch(c.cv, i > 0 ? i - 1 : 0, i, c.st, c.mem, keypoint_interval, sp);
        chain_launch(c.cv, c.st, c.mem, c.recs, h->pp, i, keypoint_interval, homography_interval, calibration, sp);
    }
    HIP_CHECK(hipEventRecord(c.ev_loop, sp));
    if (stalled_at) *stalled_at = -1;
    if (wait) {
        HIP_CHECK(hipMemcpyAsync(c.h_tail, (char*)c.st + offsetof(ChainState, stalled), sizeof(int) * 2, hipMemcpyDeviceToHost, sp));
        HIP_CHECK(hipStreamSynchronize(sp));
        if (stalled_at) *stalled_at = c.h_tail[0];
        if (c.h_tail[1]) { h->err = "the reference raises IndexError in calibrate_keypoints at frame " + std::to_string(c.h_tail[1] - 1); return EAGLE_E_REFERENCE_RAISES; }
    }
    API_END(h)
}

int eagle_clip_fetch(EagleHandle* h, EagleFrameResult* out)
{
    CLIP_CHECK(h, h->clip.open && (out || h->clip.cv.n == 0), "eagle_clip_fetch: bad arguments")
    API_BEGIN
    HIP_CHECK(hipSetDevice(h->cfg.device));
    eagle::clip_sync(h);
    if (h->clip.cv.n > 0) HIP_CHECK(hipMemcpy(out, h->clip.recs, sizeof(EagleFrameResult) * (size_t)h->clip.cv.n, hipMemcpyDeviceToHost));
    // saturated f32s stores of the session's detector / key-point passes (counted per slot of the device batch, not per clip frame)
    HIP_CHECK(hipMemcpy(h->clip_sat_h, h->clip_sat, eagle::sat_pad_bytes(h->cfg.batch), hipMemcpyDeviceToHost));
    h->sat_events = 0; h->sat_frames = 0;
    for (int i = 0; i < h->cfg.batch; ++i) if (h->clip_sat_h[i]) { h->sat_events += h->clip_sat_h[i]; ++h->sat_frames; }
    h->timings.sat_events = (int32_t)std::min<long long>(h->sat_events, 0x7fffffff); h->timings.sat_frames = h->sat_frames;
    eagle::check_saturation(h, "eagle_clip_fetch");
    API_END(h)
}

}  // extern "C"
