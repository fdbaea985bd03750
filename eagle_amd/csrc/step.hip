// Per-batch execution: the launch schedule of one step on the handle's streams (optionally replayed as a hipGraph), the two-deep pipeline over the
// steps of a call, staging of caller frames (BGR or 4:2:0, host or device) and the eagle_process_* entries.
#include "runtime.h"

namespace eagle {

// ------------------------------------------------------------------------------------------------------------
// step execution
// ------------------------------------------------------------------------------------------------------------
// profiling mode only: HIP events around one non-convolution launch on stream st (the stream the kernel is launched on)
static int ktab_index(EagleHandle* h, const char* name)
{
    for (size_t i = 0; i < h->ktab.size(); ++i) if (!strcmp(h->ktab[i].name, name)) return (int)i;
    EagleKernelTime e; memset(&e, 0, sizeof(e)); strncpy(e.name, name, sizeof(e.name) - 1);
    h->ktab.push_back(e);
    return (int)h->ktab.size() - 1;
}
template <class F>
static void timed(EagleHandle* h, const char* name, double bytes, hipStream_t st, F&& fn)
{
    if (!h->prof) { fn(); return; }
    while (h->span_pool.size() < h->span_used + 2) { hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); h->span_pool.push_back(e); }
    EagleHandle::Span sp{ktab_index(h, name), bytes, h->span_pool[h->span_used], h->span_pool[h->span_used + 1]};
    h->span_used += 2;
    HIP_CHECK(hipEventRecord(sp.a, st));
    fn();
    HIP_CHECK(hipEventRecord(sp.b, st));
    h->spans.push_back(sp);
}

void timed_launch(EagleHandle* h, const char* name, double bytes, hipStream_t st, const std::function<void()>& fn) { timed(h, name, bytes, st, fn); }

size_t sat_pad_bytes(int B) { return ((size_t)B * sizeof(unsigned) + 255) & ~(size_t)255; }

void run_net(EagleHandle* h, Net* net, hipStream_t s, size_t& ev_i)
{
    const bool multi = h->multi_stream && !h->prof;
    for (Op& op : net->ops) {
        if (op.kind == Op::FORK) {
            if (multi) {
                HIP_CHECK(hipEventRecord(h->ev_fork, s));
                for (int k = 0; k < op.nbranch; ++k) HIP_CHECK(hipStreamWaitEvent(h->s_br[k], h->ev_fork, 0));
            }
            continue;
        }
        if (op.kind == Op::JOIN) {
            if (multi)
                for (int k = 0; k < op.nbranch; ++k) {
                    HIP_CHECK(hipEventRecord(h->ev_join[k], h->s_br[k]));
                    HIP_CHECK(hipStreamWaitEvent(s, h->ev_join[k], 0));
                }
            continue;
        }
        hipStream_t st = (multi && op.stream > 0) ? h->s_br[op.stream - 1] : s;
        if ((g_dbg_skip & 64) && op.kind == Op::OTHER) continue;
        if ((g_dbg_skip & 128) && op.kind == Op::CONV) continue;
        if (h->prof && op.kind == Op::CONV) {
            HIP_CHECK(hipEventRecord(h->conv_ev[ev_i++], st));
            op.run(st);
            HIP_CHECK(hipEventRecord(h->conv_ev[ev_i++], st));
            h->conv_ops.push_back(&op);
        } else {
            timed(h, op.tag, op.bytes, st, [&] { op.run(st); });
        }
    }
}

// networks + decode/NMS + heat-map maxima of one batch (buffers of parity p), reading frames from d_src (device)
static void enqueue_compute(EagleHandle* h, int p, const uint8_t* d_src, int n_active)
{
    const EagleConfig& c = h->cfg;
    const int B = c.batch;
    EagleHandle::StepBuf& sb = h->sb[p];
    size_t ev_i = 0;
    HIP_CHECK(hipMemsetAsync(sb.d_sat, 0, sat_pad_bytes(B) + sizeof(EagleFrameResult) * B, h->s_main));      // saturation words + records
    h->cur_sat = sb.d_sat;
    h->cur_src = d_src; h->cur_n = n_active;
    const double esz = h->prec == EAGLE_PREC_F16 ? 2 : 4, det_esz = h->det_prec == EAGLE_PREC_F16 ? 2 : 4;
    if (!(g_dbg_skip & 16))
        timed(h, "preprocess", (double)n_active * ((double)c.frame_h * c.frame_w * 3 + (h->stem_on ? 0.0 : 540.0 * 960 * h->kp_in.c * esz) + (double)h->lb.out_h * h->lb.out_w * h->det_in.c * det_esz), h->s_main,
              [&] {
                  // one launch, each tensor in its network's format; with the fused stem (stem.hip) only the detector's: HRNet reads the frames itself
                  preprocess_launch(h->prec, d_src, n_active, c.frame_h, c.frame_w, h->kp_in, h->det_in, h->lb, h->s_main, h->stem_on ? 2 : 3, h->det_prec);
              });
    const bool two = !h->prof;
    hipStream_t sd = two ? h->s_det : h->s_main;
    if (two) {
        HIP_CHECK(hipEventRecord(h->ev_pre, h->s_main));
        HIP_CHECK(hipStreamWaitEvent(sd, h->ev_pre, 0));
    }
    if (!(g_dbg_skip & 2)) run_net(h, h->yo.get(), sd, ev_i);            // detector branch
    if (!(g_dbg_skip & 4)) {
        // (64 box logits + 16-padded class logits) fp32 in, 4 box floats + confidence + class + sort key out, per anchor
        timed(h, "yolo_decode", (double)B * h->ds.A * ((64 + 16) * 4.0 + 4 * 4 + 4 + 4 + 8), sd, [&] { yolo_decode_launch(h->levels, 3, B, 5, c.detector_floor, h->ds, sd); });
        timed(h, "nms", (double)B * h->ds.A * 8.0, sd, [&] { nms_launch(h->ds, B, h->pp, sb.d_out, sd); });      // the key array, read once
    }
    if (two) HIP_CHECK(hipEventRecord(h->ev_det, sd));
    h->cur_parts = sb.parts;
    if (!(g_dbg_skip & 1)) run_net(h, h->hr.get(), h->s_main, ev_i);     // keypoint branch
    if (!(g_dbg_skip & 32) && !h->fused_argmax)
        timed(h, "heat_argmax", (double)h->logits.n * h->logits.h * h->logits.w * h->logits.cs * 4.0, h->s_main, [&] { heat_argmax_launch(h->logits, sb.parts, h->hm_chunks, h->s_main); });
    if (two) HIP_CHECK(hipStreamWaitEvent(h->s_main, h->ev_det, 0));     // join
}

// use_graph: 1 = every step is replayed; 2 = only inside calls of at least three steps — there the graph launch of step i + 1 hides behind step i on the GPU and saves the host
// the 383 launches, while a ONE-step call of a large batch pays the graph launch in full before anything runs (B = 25 per call: 658 -> 455 frames/s,
// profiles/r05c_latency_modes.txt).  Measured at batch 50, 20 steps: nothing on /opt/rocm's runtime (765.3 against 766.1 frames/s), +1.6 % on the PyTorch wheel's ROCm 7.0.2 runtime,
// whose launch path is slower (739 -> 751): bench.py asks for 2 in its multi-rank path; "auto" stays at plain launches for batch > EAGLE_SMALL_BATCH (a capture costs ~80 ms per
// (slot, frame count), which a short first call would pay inside its own latency)
static bool graph_on(const EagleHandle* h) { return !h->graph_broken && (h->cfg.use_graph == 1 || (h->cfg.use_graph == 2 && h->call_steps >= 3)); }

static void launch_step(EagleHandle* h, int p, const uint8_t* d_src, int n_active)
{
    const EagleConfig& c = h->cfg;
    EagleHandle::StepBuf& sb = h->sb[p];
    bool replayed = false;
    if (graph_on(h) && !h->prof) {
        if (!h->warmed) {   // first call eager: lets every launcher set its function attributes outside a capture
            enqueue_compute(h, p, d_src, n_active);
            HIP_CHECK(hipStreamSynchronize(h->s_main));
            h->warmed = true;
        }
        if (d_src != sb.d_frames) fail(EAGLE_E_STATE, "graph replay needs the slot's staging buffer as the source");
        auto it = sb.graphs.find(n_active);
        if (it == sb.graphs.end() && sb.capture_skip > 0) --sb.capture_skip;
        else if (it == sb.graphs.end()) {
            CaptureExclusive only_this_thread_talks_to_hip;
            if (only_this_thread_talks_to_hip.ok) {
                // thread-local capture mode: only THIS thread is held to capture-safe calls while the capture is open (it makes none: the warm-up step above has
                // set the function attributes of every kernel a step may launch at any frame count — conv_launch sets those of both weight-ring depths, which
                // depend on the number of work items — and allocated the zero / trash pages).  The global mode made every hipMalloc / hipFree / synchronise of ANY other
                // thread fail with "operation not permitted when stream is capturing" — a second handle on another host thread, which is how the concurrency
                // tests and a multi-handle server run — and left this stream in a broken capture (round 5: six tests of the suite, once small batches captured by default)
                struct CaptureScope {                       // a throw between Begin and End must not leave s_main capturing: end it, drop the graph, stop replaying
                    EagleHandle* h; bool open = false; hipGraph_t g = nullptr;
                    ~CaptureScope()
                    {
                        if (open) { (void)hipStreamEndCapture(h->s_main, &g); (void)hipGetLastError(); h->graph_broken = true; }
                        if (g) (void)hipGraphDestroy(g);
                    }
                } cs{h};
                HIP_CHECK(hipStreamBeginCapture(h->s_main, hipStreamCaptureModeThreadLocal));
                cs.open = true;
                enqueue_compute(h, p, d_src, n_active);
                cs.open = false;
                HIP_CHECK(hipStreamEndCapture(h->s_main, &cs.g));
                hipGraphExec_t ge = nullptr;
                if (hipGraphInstantiate(&ge, cs.g, nullptr, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); h->graph_broken = true; fail(EAGLE_E_HIP, "hipGraphInstantiate failed"); }
                if (sb.graphs.size() >= 16) { (void)hipGraphExecDestroy(sb.graphs.begin()->second); sb.graphs.erase(sb.graphs.begin()); }      // (frame counts 1 .. batch: bounded)
                it = sb.graphs.emplace(n_active, ge).first;
                sb.capture_backoff = 0;
                ++h->graph_captures;
            } else {
                sb.capture_backoff = std::min(64, std::max(1, sb.capture_backoff * 2));
                sb.capture_skip = sb.capture_backoff;
                ++h->graph_skipped;
            }
        }
        if (it != sb.graphs.end()) { HIP_CHECK(hipGraphLaunch(it->second, h->s_main)); replayed = true; }
    }
    if (!replayed) enqueue_compute(h, p, d_src, n_active);
    hipStream_t sp = h->prof ? h->s_main : h->s_post;
    if (!h->prof) {
        HIP_CHECK(hipEventRecord(sb.ev_compute, h->s_main));
        HIP_CHECK(hipStreamWaitEvent(sp, sb.ev_compute, 0));
    }
    if (!(g_dbg_skip & 8)) timed(h, "post (geometry)", 0, sp, [&] { post_launch(sb.parts, c.batch, h->pp, sb.d_out, sp); });
    HIP_CHECK(hipMemcpyAsync(sb.h_sat, sb.d_sat, sat_pad_bytes(c.batch) + sizeof(EagleFrameResult) * n_active, hipMemcpyDeviceToHost, sp));
    HIP_CHECK(hipEventRecord(sb.ev_done, sp));
}

void collect_spans(EagleHandle* h)
{
    for (const EagleHandle::Span& sp : h->spans) {
        float t = 0.f;
        HIP_CHECK(hipEventElapsedTime(&t, sp.a, sp.b));
        EagleKernelTime& e = h->ktab[sp.k];
        e.ms += t; e.launches += 1; e.bytes += sp.bytes;
    }
    h->spans.clear(); h->span_used = 0;
}

static void collect_step(EagleHandle* h, int p, int n_active, EagleFrameResult* out)
{
    HIP_CHECK(hipEventSynchronize(h->sb[p].ev_done));
    memcpy(out, h->sb[p].h_out, sizeof(EagleFrameResult) * n_active);
    for (int i = 0; i < n_active; ++i)                      // f32s: frames in which an activation left the split format's range (|v| > 4094) are flagged
        if (h->sb[p].h_sat[i]) { out[i].pad[1] = 1; h->sat_events += h->sb[p].h_sat[i]; ++h->sat_frames; }
    h->timings.n_launches += h->n_launch;
    h->timings.n_conv_launches += h->n_conv;
    h->timings.conv_flop += h->conv_flop_step;
    if (h->prof) {
        for (size_t i = 0; i + 1 < h->conv_ev.size(); i += 2) {
            float t = 0.f;
            HIP_CHECK(hipEventElapsedTime(&t, h->conv_ev[i], h->conv_ev[i + 1]));
            h->timings.conv_ms += t;
            if (i / 2 < h->conv_ops.size()) {
                const Op* op = h->conv_ops[i / 2];
                EagleKernelTime& e = h->ktab[ktab_index(h, op->tag)];
                e.ms += t; e.launches += 1; e.bytes += op->bytes; e.flop += op->flop;
            }
        }
        h->conv_ops.clear();
        collect_spans(h);
    }
}

// all batches of one call of entry `what`; stage(p, i, na) yields the device pointer of the na frames from frame i on (after any staging copy into slot p)
template <class Stage>
static void run_pipeline(EagleHandle* h, const char* what, int n, EagleFrameResult* out, Stage stage)
{
    const int B = h->cfg.batch;
    memset(&h->timings, 0, sizeof(h->timings));
    h->sat_events = 0; h->sat_frames = 0;
    if (n == 0) return;
    h->call_steps = (n + B - 1) / B;
    HIP_CHECK(hipEventRecord(h->ev_t0, h->s_main));
    int prev_n = 0, prev_i = 0, k = 0;
    for (int i = 0; i < n; i += B, ++k) {
        const int p = k & 1, na = std::min(B, n - i);
        const uint8_t* src = stage(p, i, na);
        launch_step(h, p, src, na);
        if (k > 0) collect_step(h, p ^ 1, prev_n, out + prev_i);
        prev_n = na; prev_i = i;
        if (h->prof) { collect_step(h, p, na, out + i); prev_n = 0; }     // profiling mode: strictly serial
    }
    if (prev_n > 0) collect_step(h, (k - 1) & 1, prev_n, out + prev_i);
    hipStream_t sp = h->prof ? h->s_main : h->s_post;
    HIP_CHECK(hipEventRecord(h->ev_t1, sp));
    HIP_CHECK(hipEventSynchronize(h->ev_t1));
    HIP_CHECK(hipEventSynchronize(h->ev_t0));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, h->ev_t0, h->ev_t1));
    h->timings.total_ms = ms;
    h->timings.sat_events = (int32_t)std::min<long long>(h->sat_events, 0x7fffffff);
    h->timings.sat_frames = h->sat_frames;
    check_saturation(h, what);
}

// EAGLE_PREC_F32S stores clip at +-4094 instead of overflowing; a call in which that happened must not look like a success
void check_saturation(EagleHandle* h, const char* what)
{
    if (h->sat_events > 0 && !h->cfg.allow_saturation)
        fail(EAGLE_E_RANGE, "%s: %lld activation stores in %d frame(s) left the range of the f32s tensor format (|v| > 4094) and were clipped; the records are "
             "written (EagleFrameResult.pad[1] marks the frames) but are not fp32-grade.  Use EAGLE_PREC_F32 for these weights, or set EagleConfig.allow_saturation",
             what, h->sat_events, h->sat_frames);
}

// ---- decoder-native input (eagle_*_yuv): layout of the caller's 4:2:0 frames ---------------------------------------------------------------
// The one argument check of every entry that takes an EagleYuvLayout (declared in runtime.h; eagle_annotate_* check their output layout with it)
YuvGeom yuv_geometry(int fmt, int h, int w, const EagleYuvLayout* L, bool output)
{
    const bool bgr = output && fmt == EAGLE_PIX_BGR;       // pitched BGR exists as an OUTPUT layout only: one plane, y_pitch = row pitch
    if (!bgr && fmt != EAGLE_PIX_NV12 && fmt != EAGLE_PIX_I420)
        fail(EAGLE_E_INVALID, output ? "unknown pixel format %d (EAGLE_PIX_BGR = 0, EAGLE_PIX_NV12 = 1, EAGLE_PIX_I420 = 2)" : "unknown pixel format %d (EAGLE_PIX_NV12 = 1, EAGLE_PIX_I420 = 2)", fmt);
    if (bgr ? (h < 1 || w < 1) : (h < 2 || w < 2 || (h & 1) || (w & 1))) fail(EAGLE_E_INVALID, "4:2:0 frames need an even height and width (got %d x %d)", h, w);
    EagleYuvLayout l{};
    if (L) l = *L;
    const int64_t lim = (int64_t)1 << 40;
    const int64_t* f = &l.frame_stride;
    static const char* names[5] = {"frame_stride", "y_pitch", "c_offset", "c_pitch", "v_offset"};
    for (int k = 0; k < 5; ++k)
        if (f[k] < 0 || f[k] > lim) fail(EAGLE_E_INVALID, "layout.%s = %lld is negative or out of range", names[k], (long long)f[k]);
    YuvGeom g{};
    g.fmt = fmt; g.h = h; g.w = w;
    if (bgr) {
        const int64_t row = (int64_t)w * 3;
        g.y_pitch = l.y_pitch ? l.y_pitch : row;
        if (g.y_pitch < row) fail(EAGLE_E_INVALID, "layout.y_pitch %lld is smaller than a row of %d BGR pixels (%lld bytes)", (long long)g.y_pitch, w, (long long)row);
        g.nplanes = 1;
        g.pl[0] = {0, g.y_pitch, h, row, 0};
        g.extent = g.y_pitch * (h - 1) + row;
        g.frame_stride = l.frame_stride ? l.frame_stride : g.y_pitch * h;
        if (g.frame_stride < g.extent) fail(EAGLE_E_INVALID, "layout.frame_stride %lld is smaller than a frame's extent (%lld bytes)", (long long)g.frame_stride, (long long)g.extent);
        g.dense_bytes = row * h;
        g.dense = g.y_pitch == row && g.frame_stride == g.dense_bytes;
        return g;
    }
    const bool nv12 = fmt == EAGLE_PIX_NV12;
    const int64_t c_row = nv12 ? w : w / 2, c_rows = h / 2;
    g.y_pitch = l.y_pitch ? l.y_pitch : w;
    g.c_offset = l.c_offset ? l.c_offset : g.y_pitch * h;
    g.c_pitch = l.c_pitch ? l.c_pitch : c_row;
    g.v_offset = nv12 ? 0 : l.v_offset ? l.v_offset : g.c_offset + g.c_pitch * c_rows;
    if (g.y_pitch < w) fail(EAGLE_E_INVALID, "layout.y_pitch %lld is smaller than a Y row (%d bytes)", (long long)g.y_pitch, w);
    if (g.c_pitch < c_row) fail(EAGLE_E_INVALID, "layout.c_pitch %lld is smaller than a chroma row (%lld bytes)", (long long)g.c_pitch, (long long)c_row);
    g.nplanes = nv12 ? 2 : 3;
    g.pl[0] = {0, g.y_pitch, h, w, 0};
    g.pl[1] = {g.c_offset, g.c_pitch, c_rows, c_row, (int64_t)h * w};
    g.pl[2] = {g.v_offset, g.c_pitch, c_rows, c_row, (int64_t)h * w + c_row * c_rows};
    static const char* pn[2][3] = {{"Y", "UV", ""}, {"Y", "U", "V"}};
    int64_t end = 0;
    g.extent = 0;
    for (int a = 0; a < g.nplanes; ++a) {
        const HostPlane& p = g.pl[a];
        const int64_t a1 = p.off + p.pitch * (p.rows - 1) + p.row_bytes;
        g.extent = std::max(g.extent, a1);
        end = std::max(end, p.off + p.pitch * p.rows);
        for (int b = 0; b < a; ++b) {
            const HostPlane& q = g.pl[b];
            const int64_t b1 = q.off + q.pitch * (q.rows - 1) + q.row_bytes;
            if (p.off < b1 && q.off < a1)
                fail(EAGLE_E_INVALID, "the %s plane [%lld, %lld) overlaps the %s plane [%lld, %lld) of the frame", pn[!nv12][a], (long long)p.off, (long long)a1,
                     pn[!nv12][b], (long long)q.off, (long long)b1);
        }
    }
    g.frame_stride = l.frame_stride ? l.frame_stride : end;
    if (g.frame_stride < g.extent) fail(EAGLE_E_INVALID, "layout.frame_stride %lld is smaller than a frame's extent (%lld bytes)", (long long)g.frame_stride, (long long)g.extent);
    g.dense_bytes = (int64_t)h * w * 3 / 2;
    g.dense = g.y_pitch == w && g.c_offset == (int64_t)h * w && g.c_pitch == c_row && (nv12 || g.v_offset == g.pl[2].dense_off) && g.frame_stride == g.dense_bytes;
    return g;
}

static YuvArgs yuv_args(const YuvGeom& g, const uint8_t* src, uint8_t* dst)
{
    YuvArgs a{};
    const bool nv12 = g.fmt == EAGLE_PIX_NV12;
    a.src = src; a.dst = dst; a.h = g.h; a.w = g.w;
    a.frame_stride = g.frame_stride; a.y_pitch = g.y_pitch; a.c_offset = g.c_offset; a.c_pitch = g.c_pitch;
    a.v_offset = nv12 ? g.c_offset + 1 : g.v_offset;
    a.c_step = nv12 ? 2 : 1;
    const uint64_t al = (uint64_t)(uintptr_t)src | (uint64_t)g.frame_stride | (uint64_t)g.y_pitch;                 // 8-byte Y loads
    const uint64_t ac = nv12 ? ((uint64_t)g.c_offset | (uint64_t)g.c_pitch) & 7                                    // 8-byte UV loads
                             : ((uint64_t)g.c_offset | (uint64_t)g.c_pitch | (uint64_t)g.v_offset) & 3;            // 4-byte U and V loads
    a.vec = (al & 7) == 0 && ac == 0;
    return a;
}

// n frames of layout g at src (device) -> dense BGR at dst, on stream s (timed as "yuv_to_bgr": 4:2:0 read once + BGR written once)
static void yuv_convert(EagleHandle* h, const YuvGeom& g, const uint8_t* src, int n, uint8_t* dst, hipStream_t s)
{
    timed(h, "yuv_to_bgr", (double)n * g.h * g.w * (1.5 + 3.0), s, [&] { yuv_to_bgr_launch(yuv_args(g, src, dst), n, s); });
}

// ---- caller frames in host memory -> the slot's dense device buffer --------------------------------------------------------------------
// the shared preamble of the eagle_process_* entries
static void process_begin(EagleHandle* h, const void* src, const void* out, int n)
{
    if (!h->finalized) fail(EAGLE_E_STATE, "eagle_finalize_weights has not been called");
    if (!src || !out || n < 0) fail(EAGLE_E_INVALID, "bad argument");
    HIP_CHECK(hipSetDevice(h->cfg.device));
}

// is the caller's memory pinned (eagle_host_alloc, hipHostMalloc, hipHostRegister)?  Pageable memory needs the copy workers: started here
bool host_pinned(EagleHandle* h, const void* p)
{
    hipPointerAttribute_t pa;
    const bool pinned = hipPointerGetAttributes(&pa, p) == hipSuccess && pa.type == hipMemoryTypeHost;
    (void)hipGetLastError();                               // an unregistered pointer is reported as an error: not one of ours
    if (!pinned && !h->pool) {
        int nt = getenv("EAGLE_COPY_THREADS") ? atoi(getenv("EAGLE_COPY_THREADS")) : 8;
        nt = std::max(1, std::min(nt, (int)std::max(1u, std::thread::hardware_concurrency())));
        h->pool.reset(new CopyPool(nt));
    }
    return pinned;
}

// na frames of `npl` planes each (frame k at src + k * frame_stride; `dense`: the batch already has the destination's layout) -> dense frames of fsz bytes at
// d_dst.  H2D on its own stream: the upload of batch k+1 overlaps the networks of batch k (the device buffer of parity p was last read by batch k-2, whose
// records the host has already collected); profiling mode: on s_main, no event.  Pinned caller memory is DMA-ed in place.  Pageable memory is first copied
// into the pinned ring slot `ring` (allocated on first use) by the workers, `parts` row ranges per plane so that every worker is busy on small batches: an
// asynchronous copy out of pageable memory is staged by the runtime on the calling thread and cost 16 % of the frame rate in round 1.
static void stage_host_frames(EagleHandle* h, EagleHandle::StepBuf& sb, const uint8_t* src, int na, const HostPlane* pl, int npl, int64_t frame_stride, size_t fsz,
                              bool dense, bool pinned, uint8_t*& ring, uint8_t* d_dst, int parts)
{
    hipStream_t sc = h->prof ? h->s_main : h->s_copy;
    if (!pinned) {
        if (!ring) HIP_CHECK(hipHostMalloc((void**)&ring, (size_t)h->cfg.batch * fsz, hipHostMallocDefault));
        if (sb.copy_pending) HIP_CHECK(hipEventSynchronize(sb.ev_copy));      // the DMA of batch k-2 has left this slot
        h->pool->run(na * npl * parts, [&](int t) {
            const int k = t / (npl * parts), q = t % (npl * parts);
            const HostPlane& p = pl[q / parts];
            const int64_t r0 = p.rows * (q % parts) / parts, r1 = p.rows * (q % parts + 1) / parts;
            const uint8_t* s0 = src + (size_t)k * frame_stride + p.off;
            uint8_t* d0 = ring + (size_t)k * fsz + p.dense_off;
            if (p.pitch == p.row_bytes) memcpy(d0 + r0 * p.row_bytes, s0 + r0 * p.pitch, (size_t)((r1 - r0) * p.row_bytes));
            else for (int64_t r = r0; r < r1; ++r) memcpy(d0 + r * p.row_bytes, s0 + r * p.pitch, (size_t)p.row_bytes);
        });
        src = ring; dense = true;
    }
    if (dense) {
        HIP_CHECK(hipMemcpyAsync(d_dst, src, (size_t)na * fsz, hipMemcpyHostToDevice, sc));
    } else {
        for (int k = 0; k < na; ++k)
            for (int q = 0; q < npl; ++q)
                HIP_CHECK(hipMemcpy2DAsync(d_dst + (size_t)k * fsz + pl[q].dense_off, (size_t)pl[q].row_bytes, src + (size_t)k * frame_stride + pl[q].off,
                                           (size_t)pl[q].pitch, (size_t)pl[q].row_bytes, (size_t)pl[q].rows, hipMemcpyHostToDevice, sc));
    }
    if (!h->prof) {
        HIP_CHECK(hipEventRecord(sb.ev_copy, sc));
        sb.copy_pending = true;
        HIP_CHECK(hipStreamWaitEvent(h->s_main, sb.ev_copy, 0));
    }
}

}  // namespace eagle

extern "C" {

int eagle_process_device_frames(EagleHandle* h, const void* d_bgr, int n, EagleFrameResult* out)
{
    API_BEGIN_H(h)
    process_begin(h, d_bgr, out, n);
    const size_t fsz = (size_t)h->cfg.frame_h * h->cfg.frame_w * 3;
    h->call_steps = (n + h->cfg.batch - 1) / h->cfg.batch;
    const bool direct = !graph_on(h);                             // under graph replay every step goes through the stable staging pointer of its parity (a
    run_pipeline(h, "eagle_process_device_frames", n, out, [&](int p, int i, int na) -> const uint8_t* {   // 2.76-MB-per-frame device copy; the instances are keyed by frame count alone)
        const uint8_t* src = (const uint8_t*)d_bgr + (size_t)i * fsz;
        if (direct) return src;
        HIP_CHECK(hipMemcpyAsync(h->sb[p].d_frames, src, fsz * na, hipMemcpyDeviceToDevice, h->s_main));
        return h->sb[p].d_frames;
    });
    API_END(h)
}

int eagle_process_frames(EagleHandle* h, const uint8_t* bgr, int n, int64_t frame_stride, int64_t row_stride, EagleFrameResult* out)
{
    API_BEGIN_H(h)
    process_begin(h, bgr, out, n);
    const int fh = h->cfg.frame_h, fw = h->cfg.frame_w;
    const size_t fsz = (size_t)fh * fw * 3;
    if (row_stride == 0) row_stride = (int64_t)fw * 3;
    if (frame_stride == 0) frame_stride = row_stride * fh;
    // strides in bytes; a row must hold fw BGR pixels and the frames of one call must not overlap (the caller's view may be a crop of a wider
    // surface or a decoder's padded plane: cm.py:568 hands over whatever view it holds).  Negative strides (flipped views) are not supported.
    if (row_stride < (int64_t)fw * 3) fail(EAGLE_E_INVALID, "row_stride %lld is smaller than a row of %d BGR pixels (%d bytes)", (long long)row_stride, fw, fw * 3);
    if (frame_stride < row_stride * (fh - 1) + (int64_t)fw * 3) fail(EAGLE_E_INVALID, "frame_stride %lld is smaller than a frame (%d rows of stride %lld)", (long long)frame_stride, fh, (long long)row_stride);
    const HostPlane plane = {0, row_stride, fh, (int64_t)fw * 3, 0};      // a BGR frame: one plane
    const bool dense = row_stride == (int64_t)fw * 3 && frame_stride == (int64_t)fsz;
    const bool pinned = host_pinned(h, bgr);
    run_pipeline(h, "eagle_process_frames", n, out, [&](int p, int i, int na) -> const uint8_t* {
        EagleHandle::StepBuf& sb = h->sb[p];
        stage_host_frames(h, sb, bgr + (size_t)i * frame_stride, na, &plane, 1, frame_stride, fsz, dense, pinned, sb.h_frames, sb.d_frames, 4);
        return sb.d_frames;
    });
    API_END(h)
}

int eagle_process_frames_yuv(EagleHandle* h, int format, const uint8_t* src, int n, const EagleYuvLayout* layout, EagleFrameResult* out)
{
    API_BEGIN_H(h)
    process_begin(h, src, out, n);
    const YuvGeom g = yuv_geometry(format, h->cfg.frame_h, h->cfg.frame_w, layout);
    const YuvGeom dg = yuv_geometry(format, h->cfg.frame_h, h->cfg.frame_w, nullptr);      // what the staging buffer holds
    const bool pinned = host_pinned(h, src);
    const size_t fsz = (size_t)g.dense_bytes;
    if (!h->sb[0].d_yuv) {                                 // first 4:2:0 call of the handle: both slots' staging, before anything of this call is enqueued
        for (auto& sb : h->sb) sb.d_yuv = (uint8_t*)h->misc->get((size_t)h->cfg.batch * fsz);
        HIP_CHECK(hipDeviceSynchronize());                 // Net::get zeroes on the null stream, which the handle's non-blocking streams do not wait for
    }
    // As in eagle_process_frames the planes of batch k go up on s_copy while batch k-1 computes, into the slot's own d_yuv[p].  Its previous
    // reader is batch k-2's conversion on s_main, and run_pipeline has collected batch k-2's records (ev_done, behind that conversion on s_main)
    // before it stages batch k: the upload cannot overwrite planes that are still to be read.  The conversion then writes the slot's BGR staging
    // buffer on s_main, in stream order behind batch k-2's network phase that read it.
    run_pipeline(h, "eagle_process_frames_yuv", n, out, [&](int p, int i, int na) -> const uint8_t* {
        EagleHandle::StepBuf& sb = h->sb[p];
        stage_host_frames(h, sb, src + (size_t)i * g.frame_stride, na, g.pl, g.nplanes, g.frame_stride, fsz, g.dense, pinned, sb.h_yuv, sb.d_yuv, 2);
        yuv_convert(h, dg, sb.d_yuv, na, sb.d_frames, h->s_main);
        return sb.d_frames;
    });
    API_END(h)
}

int eagle_process_device_frames_yuv(EagleHandle* h, int format, const void* d_src, int n, const EagleYuvLayout* layout, EagleFrameResult* out)
{
    API_BEGIN_H(h)
    process_begin(h, d_src, out, n);
    const YuvGeom g = yuv_geometry(format, h->cfg.frame_h, h->cfg.frame_w, layout);
    // the caller's frames are read in place, with their layout; the conversion writes the slot's staging buffer (stream order on s_main behind
    // batch k-2's network phase, the last reader), which is also the source graph replay needs: no device-to-device copy
    run_pipeline(h, "eagle_process_device_frames_yuv", n, out, [&](int p, int i, int na) -> const uint8_t* {
        yuv_convert(h, g, (const uint8_t*)d_src + (size_t)i * g.frame_stride, na, h->sb[p].d_frames, h->s_main);
        return h->sb[p].d_frames;
    });
    API_END(h)
}

int eagle_yuv_to_bgr(EagleHandle* h, int format, const void* d_src, int n, const EagleYuvLayout* layout, void* d_bgr)
{
    API_BEGIN_H(h)
    if (!d_src || !d_bgr || n < 0) fail(EAGLE_E_INVALID, "bad argument");
    const YuvGeom g = yuv_geometry(format, h->cfg.frame_h, h->cfg.frame_w, layout);
    HIP_CHECK(hipSetDevice(h->cfg.device));
    yuv_to_bgr_launch(yuv_args(g, (const uint8_t*)d_src, (uint8_t*)d_bgr), n, h->s_main);
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    API_END(h)
}

int eagle_op_yuv_to_bgr(int device, int format, const uint8_t* src, int n, int h, int w, const EagleYuvLayout* layout, uint8_t* bgr)
{
    EagleHandle* hh = nullptr;
    API_BEGIN
    if (!src || !bgr || n < 0) fail(EAGLE_E_INVALID, "bad argument");
    const YuvGeom g = yuv_geometry(format, h, w, layout);
    if (n == 0) return EAGLE_OK;
    HIP_CHECK(hipSetDevice(device));
    Net net;
    const uint8_t* d = (const uint8_t*)net.upload(src, (size_t)((n - 1) * g.frame_stride + g.extent));      // exactly the bytes the frames span
    uint8_t* o = (uint8_t*)net.get((size_t)n * h * w * 3);
    yuv_to_bgr_launch(yuv_args(g, d, o), n, nullptr);
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(bgr, o, (size_t)n * h * w * 3, hipMemcpyDeviceToHost));
    API_END(hh)
}

}  // extern "C"
