// Host runtime behind the C ABI (include/eagle.h): error plumbing, the state of the process-wide capture lock, handle creation and destruction, the weight store,
// allocation, profiling read-back, eagle_debug and the RCCL gather.  The launch schedules are built in nets.hip and executed in step.hip (per batch) and clip.hip
// (clip session); ops_api.hip holds the operator-level test entries.  No torch, no MIOpen/hipBLASLt: every kernel the runtime launches is one of this library's own.
#include <dlfcn.h>

#include "runtime.h"

namespace eagle {

void fail(int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    throw Err{code, buf};
}

void ensure_max_dynamic_lds(const void* fn, int bytes)
{
    static std::mutex m;
    static std::map<std::pair<const void*, int>, int> done;      // (kernel, device) -> bytes already granted
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(m);
    auto it = done.find({fn, dev});
    if (it != done.end() && it->second >= bytes) return;
    HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done[{fn, dev}] = bytes;
}

thread_local std::string g_create_error;
// the capture lock (runtime.h): one instance per process
std::shared_timed_mutex g_capture_mutex;
std::mutex g_gate_m;
std::condition_variable g_gate_cv;
int g_capture_waiting = 0;                  // threads queued for the exclusive hold: new API calls let them pass first (glibc's rwlock prefers readers; with
                                                   // several handles making overlapping calls a capture would otherwise never get its turn), for a bounded time
thread_local std::shared_lock<std::shared_timed_mutex>* t_api_lock = nullptr;
int g_dbg_skip = 0;      // developer bisection (eagle_debug "skip"): 1 HRNet, 2 detector, 4 decode + NMS, 8 geometry kernel, 16 preprocess, 32 heat-map maxima, 64 fuse_sum / pool / upsample ops, 128 convolutions

}  // namespace eagle

extern "C" {

int eagle_abi_sizes(int32_t* o)
{
    if (!o) return EAGLE_E_INVALID;
    o[0] = (int32_t)sizeof(EagleConfig); o[1] = (int32_t)sizeof(EagleFrameResult); o[2] = (int32_t)sizeof(EagleDet); o[3] = (int32_t)sizeof(EagleKeypoint);
    return EAGLE_OK;
}

int eagle_default_config(EagleConfig* cfg)
{
    if (!cfg) return EAGLE_E_INVALID;
    memset(cfg, 0, sizeof(*cfg));
    cfg->device = 0; cfg->frame_h = 720; cfg->frame_w = 1280;
    cfg->det_variant = EAGLE_DET_N; cfg->det_imgsz = 640; cfg->batch = 8; cfg->precision = EAGLE_PREC_F32S;      // fp32-grade results by default (the reference computes in fp32)
    cfg->keypoint_conf = 0.3; cfg->detector_conf = 0.35; cfg->ransac_thresh = 5.0;
    cfg->detector_floor = 0.15f; cfg->nms_iou = 0.7f;
    cfg->ransac_max_iters = 2000; cfg->lm_iters = 10;
    cfg->use_graph = EAGLE_AUTO; cfg->multi_stream = EAGLE_AUTO;      // small-batch mode (batch <= EAGLE_SMALL_BATCH): hipGraph replay + HRNet's branches on their own streams
    // "auto" (resolved by eagle_create from the `precision` the caller ends up with): next to split-family key-points the detector (1.4 % of the
    // FLOP with yolov8n) runs in the exact fp32 family — boxes, confidences, classes, the NMS order and therefore every detection-index id
    // (cm.py:598-627) equal the fp32 oracle's bit for bit; next to any other `precision` it runs in that same family
    cfg->det_precision = EAGLE_DET_PREC_AUTO;
    return EAGLE_OK;
}

int eagle_resolve_config(EagleConfig* cfg)
{
    if (!cfg) return EAGLE_E_INVALID;
    if (cfg->det_precision == EAGLE_DET_PREC_AUTO) cfg->det_precision = cfg->precision == EAGLE_PREC_F32S ? EAGLE_PREC_F32 + 1 : 0;
    // Small-batch mode (round 5; the reference's caller hands over ONE frame per iteration, cm.py:277).  A step of <= EAGLE_SMALL_BATCH frames leaves most
    // of the chip idle inside every launch (48->48 @135x240 is 116 workgroups per frame for 512 slots) and its 383 launches cost as much as its kernels:
    // the network phase is replayed as ONE hipGraph and HRNet's branches (and the detector) run on their own streams so that the small launches of
    // different branches fill the CUs together.  Measured on MI355X (default handle, per call incl. H2D and records back, bench.py `latency`): B = 1
    // 13.9 -> 9.6 ms, B = 4 252 -> 344 frames/s, B = 8 395 -> 505 frames/s; at B = 50 the same switches measure nothing (DESIGN.md §4b xii), so larger
    // batches keep plain launches (no graph replay).
    // Sweep on one box (profiles/r05c_latency_modes.txt; frames/s plain -> small-batch mode): B = 1 72 -> 105, 4 252 -> 344, 8 395 -> 505, 12 506 -> 571,
    // 16 530 -> 599 (the branch streams alone; the graph adds nothing beyond B = 8), 25 658 -> 674 (graph replay of a 25-frame step: 455, it loses), 50 0.
    if (cfg->use_graph == EAGLE_AUTO) cfg->use_graph = (cfg->batch >= 1 && cfg->batch <= EAGLE_SMALL_BATCH) ? 1 : 0;      // (2 = replay only inside calls of >= 3 steps: on request)
    // Branch streams: on for EVERY batch since round 6.  Until then they paid up to 16 frames per step and measured nothing at 50; with the fuse outputs on parallel
    // streams and the branches' blocks interleaved (hr_stage) the small launches of a module's fuse phase and the tails of its branch launches overlap at any
    // batch: B = 50, same box, three alternating pairs 810.2 / 806.4 / 805.7 -> 823.1 / 820.2 / 818.0 frames/s (profiles/r06aj_*).  EAGLE_MULTI_STREAM=0 in the
    // environment resolves "auto" to one stream per network (developer A/B).
    if (cfg->multi_stream == EAGLE_AUTO) cfg->multi_stream = (getenv("EAGLE_MULTI_STREAM") && atoi(getenv("EAGLE_MULTI_STREAM")) == 0) ? 0 : 1;
    // A geometry with more anchors than the NMS workgroup sorts is refused here, not by the first step's enqueue (eagle_last_error(NULL) names count and limit).
    // Fields eagle_create rejects on their own are left to it.
    if (cfg->frame_h >= 32 && cfg->frame_w >= 32 && cfg->det_imgsz >= 32 && cfg->det_imgsz % 32 == 0 &&
        (cfg->letterbox == EAGLE_LETTERBOX_RECT || cfg->letterbox == EAGLE_LETTERBOX_SQUARE)) {
        try { eagle::check_anchor_limit(*cfg); }
        catch (const eagle::Err& e) { eagle::g_create_error = e.msg; return e.code; }
    }
    return EAGLE_OK;
}

int eagle_create(const EagleConfig* cfg, EagleHandle** out)
{
    EagleHandle* h = nullptr;
    API_BEGIN
    if (!cfg || !out) fail(EAGLE_E_INVALID, "null argument");
    if (cfg->batch < 1 || cfg->frame_h < 32 || cfg->frame_w < 32) fail(EAGLE_E_INVALID, "bad batch/frame size");
    if (cfg->precision != EAGLE_PREC_F16 && cfg->precision != EAGLE_PREC_F32 && cfg->precision != EAGLE_PREC_F32S) fail(EAGLE_E_INVALID, "bad precision");
    if (cfg->det_variant < 0 || cfg->det_variant > 4) fail(EAGLE_E_INVALID, "bad detector variant");
    if (cfg->letterbox != EAGLE_LETTERBOX_RECT && cfg->letterbox != EAGLE_LETTERBOX_SQUARE) fail(EAGLE_E_INVALID, "letterbox: 0 (rect, auto=True) or 1 (square, auto=False)");
    if (cfg->det_imgsz < 32 || cfg->det_imgsz % 32) fail(EAGLE_E_INVALID, "det_imgsz must be a positive multiple of 32 (the detector's largest stride)");
    if (cfg->det_precision < EAGLE_DET_PREC_AUTO || cfg->det_precision > EAGLE_DET_PREC_MIXED) fail(EAGLE_E_INVALID, "bad detector precision");
    if (cfg->use_graph < EAGLE_AUTO || cfg->use_graph > 2 || cfg->multi_stream < EAGLE_AUTO || cfg->multi_stream > 1) fail(EAGLE_E_INVALID, "use_graph: -1 (auto), 0, 1 or 2; multi_stream: -1 (auto), 0 or 1");
    check_anchor_limit(*cfg);                              // before anything is built
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) fail(EAGLE_E_HIP, "device %d not present (%d visible)", cfg->device, ndev);
    HIP_CHECK(hipSetDevice(cfg->device));
    EagleHandle* nh = new EagleHandle;
    nh->cfg = *cfg;
    (void)eagle_resolve_config(&nh->cfg);                  // det_precision "auto" -> a family, from the precision the caller actually asked for
    HIP_CHECK(hipStreamCreateWithFlags(&nh->s_main, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&nh->s_det, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&nh->s_post, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&nh->s_copy, hipStreamNonBlocking));
    for (auto& st : nh->s_br) HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreateWithFlags(&nh->ev_fork, hipEventDisableTiming));
    for (auto& e : nh->ev_join) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    nh->multi_stream = nh->cfg.multi_stream != 0;         // concurrent HRNet branches: pays for small batches only (eagle_resolve_config)
    HIP_CHECK(hipEventCreateWithFlags(&nh->ev_pre, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&nh->ev_det, hipEventDisableTiming));
    HIP_CHECK(hipEventCreate(&nh->ev_t0));
    HIP_CHECK(hipEventCreate(&nh->ev_t1));
    *out = nh;
    API_END(h)
}

void eagle_destroy(EagleHandle* h)
{
    eagle::ApiGuard not_during_a_capture;                  // hipDeviceSynchronize / hipFree below would invalidate a capture that another handle's thread has open
    if (h && h->clip.open) { (void)hipSetDevice(h->cfg.device); eagle::clip_close(h); }
    if (!h) return;
    if (h->tracker) eagle::tracker_destroy(h->tracker);
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    if (h->comm && h->rccl) {                               // the communicator of eagle_comm_init: released with the handle, before its streams go
        typedef int (*fn_comm_destroy)(void*);
        if (fn_comm_destroy cd = (fn_comm_destroy)dlsym(h->rccl, "ncclCommDestroy")) (void)cd(h->comm);
        h->comm = nullptr;
    }
    for (auto& sb : h->sb) {
        for (auto& kv : sb.graphs) (void)hipGraphExecDestroy(kv.second);
        if (sb.h_sat) (void)hipHostFree(sb.h_sat);       // (h_out lies inside it)
        if (sb.h_frames) (void)hipHostFree(sb.h_frames);
        if (sb.h_yuv) (void)hipHostFree(sb.h_yuv);           // (d_yuv belongs to the misc Net)
        if (sb.ev_compute) (void)hipEventDestroy(sb.ev_compute);
        if (sb.ev_done) (void)hipEventDestroy(sb.ev_done);
        if (sb.ev_copy) (void)hipEventDestroy(sb.ev_copy);
    }
    for (auto& e : h->conv_ev) (void)hipEventDestroy(e);
    for (auto& e : h->span_pool) (void)hipEventDestroy(e);
    h->hr.reset(); h->yo.reset(); h->misc.reset(); h->reid.reset();
    if (h->ecc_prev) (void)hipFree(h->ecc_prev);
    if (h->gather_buf) (void)hipFree(h->gather_buf);
    if (h->annot_prims) (void)hipFree(h->annot_prims);
    if (h->annot_out) (void)hipFree(h->annot_out);
    if (h->annot_ring) (void)hipHostFree(h->annot_ring);
    if (h->mm_list) (void)hipFree(h->mm_list);
    if (h->mm_cols) (void)hipFree(h->mm_cols);
    for (void* q : h->mm_tr) if (q) (void)hipFree(q);
    if (h->mm_mask) (void)hipFree(h->mm_mask);
    if (h->ct_list) (void)hipFree(h->ct_list);
    if (h->ct_cols) (void)hipFree(h->ct_cols);
    if (h->ct_grid) (void)hipFree(h->ct_grid);
    if (h->reid_crops_h) (void)hipHostFree(h->reid_crops_h);
    if (h->reid_feats_h) (void)hipHostFree(h->reid_feats_h);
    if (h->clip_sat_h) (void)hipHostFree(h->clip_sat_h);
    if (h->s_main) (void)hipStreamDestroy(h->s_main);
    if (h->s_det) (void)hipStreamDestroy(h->s_det);
    if (h->s_post) (void)hipStreamDestroy(h->s_post);
    if (h->s_copy) (void)hipStreamDestroy(h->s_copy);
    for (auto st : h->s_br) if (st) (void)hipStreamDestroy(st);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (auto e : h->ev_join) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {h->ev_pre, h->ev_det, h->ev_t0, h->ev_t1}) if (e) (void)hipEventDestroy(e);
    delete h;
}

int eagle_get_config(EagleHandle* h, EagleConfig* cfg)
{
    if (!h || !cfg) return EAGLE_E_INVALID;
    *cfg = h->cfg;
    return EAGLE_OK;
}

const char* eagle_last_error(EagleHandle* h) { return h ? h->err.c_str() : eagle::g_create_error.c_str(); }

int eagle_load_weights(EagleHandle* h, const char* name, const float* data, const int64_t* shape, int ndim)
{
    API_BEGIN_H(h)
    if (!name || !data || ndim < 0 || ndim > 8) fail(EAGLE_E_INVALID, "bad weight tensor");
    if (h->finalized) fail(EAGLE_E_STATE, "weights already finalized");
    HostTensor t;
    size_t n = 1;
    if (ndim > 0 && !shape) fail(EAGLE_E_INVALID, "bad weight tensor");
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] <= 0 || shape[i] > (1ll << 31) || n * (size_t)shape[i] > ((size_t)1 << 33)) fail(EAGLE_E_INVALID, "%s: bad dimension %lld", name, (long long)shape[i]);
        t.shape.push_back(shape[i]); n *= (size_t)shape[i];
    }
    t.data.assign(data, data + n);
    h->weights[name] = std::move(t);
    API_END(h)
}

int eagle_finalize_weights(EagleHandle* h)
{
    API_BEGIN_H(h)
    if (h->finalized) fail(EAGLE_E_STATE, "already finalized");
    HIP_CHECK(hipSetDevice(h->cfg.device));
    finalize(h);
    API_END(h)
}

int eagle_device_alloc(EagleHandle* h, int64_t bytes, void** dptr)
{
    API_BEGIN_H(h)
    HIP_CHECK(hipSetDevice(h->cfg.device));
    HIP_CHECK(hipMalloc(dptr, (size_t)bytes));
    API_END(h)
}
int eagle_device_free(EagleHandle* h, void* dptr)
{
    API_BEGIN_H(h)
    HIP_CHECK(hipFree(dptr));
    API_END(h)
}
int eagle_device_upload(EagleHandle* h, void* dptr, const void* src, int64_t bytes)
{
    API_BEGIN_H(h)
    HIP_CHECK(hipMemcpy(dptr, src, (size_t)bytes, hipMemcpyHostToDevice));
    API_END(h)
}

int eagle_host_alloc(EagleHandle* h, int64_t bytes, void** ptr)
{
    API_BEGIN_H(h)
    if (!ptr || bytes < 0) fail(EAGLE_E_INVALID, "bad argument");
    HIP_CHECK(hipSetDevice(h->cfg.device));
    HIP_CHECK(hipHostMalloc(ptr, (size_t)std::max<int64_t>(bytes, 16), hipHostMallocDefault));
    API_END(h)
}
int eagle_host_free(EagleHandle* h, void* ptr)
{
    API_BEGIN_H(h)
    HIP_CHECK(hipHostFree(ptr));
    API_END(h)
}

int eagle_set_profiling(EagleHandle* h, int on)
{
    if (!h) return EAGLE_E_INVALID;
    h->prof = on != 0;
    if (h->prof) h->ktab.clear();
    return EAGLE_OK;
}
int eagle_get_kernel_times(EagleHandle* h, EagleKernelTime* out, int cap, int* n)
{
    if (!h || !n || (cap > 0 && !out)) return EAGLE_E_INVALID;
    *n = (int)h->ktab.size();
    for (int i = 0; i < *n && i < cap; ++i) out[i] = h->ktab[i];
    return EAGLE_OK;
}
int eagle_get_timings(EagleHandle* h, EagleTimings* t)
{
    if (!h || !t) return EAGLE_E_INVALID;
    *t = h->timings;
    t->graph_captures = h->graph_captures; t->graph_skipped = h->graph_skipped;
    return EAGLE_OK;
}

int eagle_debug(const char* key, int64_t value, void* out, int64_t out_bytes)
{
    EagleHandle* h = nullptr;
    int rc = 0;
    API_BEGIN
    // The switches are process-wide and change what every handle computes ("skip" drops whole kernels): they only exist for the developer
    // probes under tools/ and stay inert unless the process opts in.
    static const bool enabled = getenv("EAGLE_ENABLE_DEBUG") && atoi(getenv("EAGLE_ENABLE_DEBUG")) != 0;
    if (!enabled) fail(EAGLE_E_STATE, "eagle_debug is disabled: set EAGLE_ENABLE_DEBUG=1 in the environment of a developer probe to use it");
    if (key && !strcmp(key, "skip")) { eagle::g_dbg_skip = (int)value; return EAGLE_OK; }
    rc = eagle::lk_debug(key, value, out, out_bytes);
    if (rc) return EAGLE_E_INVALID;
    API_END(h)
}

// ---- RCCL gather (resolved lazily with dlopen so the library loads on hosts without RCCL) ------------------------
typedef struct { char internal[128]; } nccl_uid;
typedef int (*fn_uid)(nccl_uid*);
typedef int (*fn_init)(void**, int, nccl_uid, int);
typedef int (*fn_allgather)(const void*, void*, size_t, int, void*, hipStream_t);
typedef int (*fn_destroy)(void*);
typedef const char* (*fn_errstr)(int);

// A process must hold ONE copy of the ROCm runtime stack.  PyTorch-ROCm wheels bundle their own (torch/lib/libamdhip64.so, libhsa-runtime64.so,
// librccl.so — SONAMEs libamdhip64.so.7 / librccl.so.1, the same as /opt/rocm's), so in a process that has imported torch the RCCL to use is the
// one that is already mapped: RTLD_NOLOAD by SONAME finds it (round 3 opened "librccl.so.1" RTLD_GLOBAL from the search path, which next to an
// already-imported torch could map a second RCCL against a second HIP runtime — DESIGN.md §8).  Only a torch-free process loads /opt/rocm's copy,
// and never RTLD_GLOBAL: nothing else resolves symbols through it.
static void* rccl_lib()
{
    static void* lib = nullptr;
    if (!lib) {
        for (const char* n : {"librccl.so.1", "librccl.so"}) {
            lib = dlopen(n, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
            if (lib) return lib;
        }
        for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
    }
    return lib;
}

int eagle_comm_id(void* id128)
{
    EagleHandle* h = nullptr;
    API_BEGIN
    void* lib = rccl_lib();
    if (!lib) fail(EAGLE_E_COMM, "librccl not found: %s", dlerror());
    fn_uid f = (fn_uid)dlsym(lib, "ncclGetUniqueId");
    if (!f) fail(EAGLE_E_COMM, "ncclGetUniqueId missing");
    nccl_uid id;
    const int rc = f(&id);
    if (rc) fail(EAGLE_E_COMM, "ncclGetUniqueId failed: %d", rc);
    memcpy(id128, &id, 128);
    API_END(h)
}

int eagle_comm_init(EagleHandle* h, int rank, int world, const void* id128)
{
    API_BEGIN_H(h)
    void* lib = rccl_lib();
    if (!lib) fail(EAGLE_E_COMM, "librccl not found");
    fn_init f = (fn_init)dlsym(lib, "ncclCommInitRank");
    if (!f) fail(EAGLE_E_COMM, "ncclCommInitRank missing");
    HIP_CHECK(hipSetDevice(h->cfg.device));
    nccl_uid id;
    memcpy(&id, id128, 128);
    const int rc = f(&h->comm, world, id, rank);
    if (rc) fail(EAGLE_E_COMM, "ncclCommInitRank failed: %d", rc);
    h->rank = rank; h->world = world; h->rccl = lib;
    API_END(h)
}

int eagle_gather(EagleHandle* h, const EagleFrameResult* local, int n_local, EagleFrameResult* all)
{
    API_BEGIN_H(h)
    if (!local || !all || n_local < 0) fail(EAGLE_E_INVALID, "bad argument");
    const size_t bytes = sizeof(EagleFrameResult) * (size_t)n_local;
    if (h->world == 1 && !h->comm) { memcpy(all, local, bytes); return EAGLE_OK; }
    if (!h->comm) fail(EAGLE_E_STATE, "eagle_comm_init has not been called");
    HIP_CHECK(hipSetDevice(h->cfg.device));
    fn_allgather ag = (fn_allgather)dlsym(h->rccl, "ncclAllGather");
    if (!ag) fail(EAGLE_E_COMM, "ncclAllGather missing");
    // device staging of the collective: kept with the handle and only ever grown (a hipMalloc / hipFree pair per call sat inside the bench's timed region)
    const size_t need = std::max<size_t>(bytes * (size_t)(h->world + 1), 256);
    if (h->gather_cap < need) {
        if (h->gather_buf) { (void)hipFree(h->gather_buf); h->gather_buf = nullptr; h->gather_cap = 0; }
        HIP_CHECK(hipMalloc(&h->gather_buf, need));
        h->gather_cap = need;
    }
    void *d_send = h->gather_buf, *d_recv = (char*)h->gather_buf + bytes;
    HIP_CHECK(hipMemcpyAsync(d_send, local, bytes, hipMemcpyHostToDevice, h->s_main));
    const int rc = ag(d_send, d_recv, bytes, /*ncclChar*/ 0, h->comm, h->s_main);
    if (rc) fail(EAGLE_E_COMM, "ncclAllGather failed: %d", rc);
    HIP_CHECK(hipMemcpyAsync(all, d_recv, bytes * h->world, hipMemcpyDeviceToHost, h->s_main));
    HIP_CHECK(hipStreamSynchronize(h->s_main));
    API_END(h)
}

}  // extern "C"
