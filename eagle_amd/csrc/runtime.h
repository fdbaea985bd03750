// Internal header of the host runtime behind the C ABI (runtime.hip, nets.hip, step.hip, clip.hip, ops_api.hip): the handle, the launch schedule it owns, the
// process-wide capture lock and the few functions that cross those files.  The kernel launchers include common.h only: none of them sees EagleHandle.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <cstdarg>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include <cstddef>
#include "common.h"

namespace eagle {

extern thread_local std::string g_create_error;
// hipGraph capture against the rest of the process.  While ANY stream of the process is being captured, HIP refuses every operation that touches the legacy stream
// (hipMemcpy, hipMemset, a null-stream launch: hipErrorStreamCaptureImplicit) in every thread — also with a thread-local capture of non-blocking streams.  Small
// batches capture by default since round 5, and a second handle on another host thread (the concurrency tests; a multi-handle server) uploads weights or runs an
// operator on the null stream whenever it likes.  So a capture is made exclusive: every C-ABI entry holds this mutex shared for its duration (outermost call only),
// the capturing thread trades its shared hold for the exclusive one around Begin ... EndCapture + instantiate.
// Round 6: the exclusive hold is only ever TRIED, for a bounded time (CAPTURE_TRY_MS).  Another handle's call may hold the mutex shared for seconds (a clip
// call) or be blocked in a collective that waits for THIS thread's own gather (one thread per GPU in one process): waiting for it without a bound was a deadlock.
// A capture that cannot get its turn is skipped — the step runs as plain launches, the same kernels in the same order — and tried again a few steps later.
// (defined once, in runtime.hip: every translation unit of the library takes the same lock)
extern std::shared_timed_mutex g_capture_mutex;
extern std::mutex g_gate_m;
extern std::condition_variable g_gate_cv;
extern int g_capture_waiting;
constexpr int CAPTURE_TRY_MS = 10, GATE_WAIT_MS = 20;
extern thread_local std::shared_lock<std::shared_timed_mutex>* t_api_lock;
struct ApiGuard {
    std::shared_lock<std::shared_timed_mutex> lk;
    bool outer;
    ApiGuard() : lk(g_capture_mutex, std::defer_lock), outer(t_api_lock == nullptr)
    {
        if (!outer) return;
        {
            std::unique_lock<std::mutex> g(g_gate_m);      // (a condition variable, not a spin: ADVICE r5)
            g_gate_cv.wait_for(g, std::chrono::milliseconds(GATE_WAIT_MS), [] { return g_capture_waiting == 0; });
        }
        lk.lock(); t_api_lock = &lk;
    }
    ~ApiGuard() { if (outer) t_api_lock = nullptr; }
};
struct CaptureExclusive {       // inside an API call: shared -> (try) exclusive -> shared again.  ok == false: no capture this time
    std::shared_lock<std::shared_timed_mutex>* al;
    std::unique_lock<std::shared_timed_mutex> ex;
    bool ok = false;
    CaptureExclusive() : al(t_api_lock), ex(g_capture_mutex, std::defer_lock)
    {
        if (al && al->owns_lock()) al->unlock();
        { std::lock_guard<std::mutex> g(g_gate_m); ++g_capture_waiting; }
        ok = ex.try_lock_for(std::chrono::milliseconds(CAPTURE_TRY_MS));
        { std::lock_guard<std::mutex> g(g_gate_m); --g_capture_waiting; }
        g_gate_cv.notify_all();
        if (!ok && al) al->lock();
    }
    ~CaptureExclusive() { if (ok) { ex.unlock(); if (al) al->lock(); } }
};
extern int g_dbg_skip;

struct HostTensor { std::vector<int64_t> shape; std::vector<float> data; };

// A few host threads that copy caller frames (pageable memory) into the pinned staging ring in parallel: one memcpy thread moves
// 5-8 GB/s, the per-frame path needs 2.76 MB x ~1800 frames/s = 5 GB/s on top of the PCIe transfer itself.
class CopyPool {
public:
    explicit CopyPool(int n) { for (int i = 0; i < n; ++i) th_.emplace_back([this] { work(); }); }
    ~CopyPool()
    {
        { std::lock_guard<std::mutex> g(m_); quit_ = true; }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    // fn(k) for k in [0, n), spread over the workers; returns when all are done
    void run(int n, const std::function<void(int)>& fn)
    {
        if (n <= 0) return;
        std::unique_lock<std::mutex> g(m_);
        fn_ = &fn; next_ = 0; n_ = n; left_ = n;
        cv_.notify_all();
        done_.wait(g, [this] { return left_ == 0; });
        fn_ = nullptr;
    }
private:
    void work()
    {
        std::unique_lock<std::mutex> g(m_);
        for (;;) {
            cv_.wait(g, [this] { return quit_ || (fn_ && next_ < n_); });
            if (quit_) return;
            const int k = next_++;
            const std::function<void(int)>* f = fn_;
            g.unlock();
            (*f)(k);
            g.lock();
            if (--left_ == 0) done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    int next_ = 0, n_ = 0, left_ = 0;
    bool quit_ = false;
};

// ------------------------------------------------------------------------------------------------------------
struct Op {
    enum Kind { CONV, OTHER, FORK, JOIN } kind = OTHER;
    std::function<void(hipStream_t)> run;
    double flop = 0;
    double bytes = 0;        // OTHER ops: algorithmic HBM bytes of one launch (inputs read once + outputs written once)
    const char* tag = "";
    int stream = 0;          // 0: the network's own stream; 1..3: HRNet branch streams (concurrent branches between fuses)
    int nbranch = 0;         // FORK/JOIN: number of side streams involved
};

struct Net {                      // one launch schedule + the device memory it owns
    std::vector<Op> ops;
    std::vector<std::unique_ptr<std::string>> names;   // layer-shape labels of the convolutions (Op::tag points into them)
    std::vector<void*> owned;
    std::multimap<size_t, void*> free_list[4];   // one pool per stream: a buffer is recycled only by work ordered after its last use
    int pool = 0;                                // pool of the stream the builder is currently emitting for
    std::map<void*, size_t> sizes;
    size_t bytes = 0;
    ~Net() { for (void* p : owned) (void)hipFree(p); }
    void* get(size_t b)
    {
        b = (b + 255) & ~(size_t)255;
        auto it = free_list[pool].find(b);
        if (it != free_list[pool].end()) { void* p = it->second; free_list[pool].erase(it); return p; }
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, b));
        HIP_CHECK(hipMemset(p, 0, b));
        // the fill runs on the null stream and need not have finished when hipMemset returns; the handle's streams are non-blocking and do not wait
        // for it, so a copy or a kernel that writes the buffer right away could be overwritten by the late zeros: wait here, once per new buffer
        HIP_CHECK(hipStreamSynchronize(nullptr));
        owned.push_back(p); sizes[p] = b; bytes += b;
        return p;
    }
    void put(void* p) { if (p) free_list[pool].insert({sizes.at(p), p}); }
    void* upload(const void* src, size_t b)
    {
        void* p = nullptr;
        HIP_CHECK(hipMalloc(&p, std::max<size_t>(b, 16)));
        HIP_CHECK(hipMemcpy(p, src, b, hipMemcpyHostToDevice));
        owned.push_back(p); bytes += b;
        return p;
    }
};

}  // namespace eagle

using namespace eagle;

struct EagleHandle {
    EagleConfig cfg;
    std::string err;
    std::map<std::string, HostTensor> weights;
    bool finalized = false;
    int prec = 0, det_prec = 0;              // precision family of the key-point network / of the detector (EagleConfig::det_precision)
    hipStream_t s_main = nullptr, s_det = nullptr, s_post = nullptr, s_copy = nullptr;
    hipStream_t s_br[3] = {nullptr, nullptr, nullptr};          // HRNet branches 1..3 (branch 0 stays on s_main)
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    bool multi_stream = true;
    hipEvent_t ev_pre = nullptr, ev_det = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
    // two-deep software pipeline: geometry + record D2H of batch i overlap the networks of batch i+1
    struct StepBuf {
        ArgmaxPart* parts = nullptr;
        EagleFrameResult* d_out = nullptr;
        EagleFrameResult* h_out = nullptr;   // pinned
        unsigned* d_sat = nullptr;           // [batch] saturated stores per frame (EAGLE_PREC_F32S; ConvArgs::sat).  Lies SAT_PAD bytes in front of d_out
        unsigned* h_sat = nullptr;           // (and of h_out): one memset and one device-to-host copy serve both
        uint8_t* d_frames = nullptr;         // staging copy of the batch (stable pointer for the captured graph)
        uint8_t* h_frames = nullptr;         // pinned ring slot for caller frames that live in pageable memory (allocated on first use)
        uint8_t* d_yuv = nullptr;            // dense 4:2:0 frames of a host-fed eagle_process_frames_yuv step (allocated on the first such call)
        uint8_t* h_yuv = nullptr;            // pinned ring slot for 4:2:0 frames that live in pageable memory (allocated on first use)
        bool copy_pending = false;           // ev_copy has been recorded for this slot
        hipEvent_t ev_compute = nullptr, ev_done = nullptr, ev_copy = nullptr;
        // hipGraph instances of this slot's network phase, one per frame count (the source is always d_frames when graphs are on: a device-fed call is staged
        // into it).  Round 5 kept ONE instance keyed on (source pointer, frame count): a call whose last step is ragged, or a caller walking a resident clip,
        // re-captured (~80 ms, process-exclusive) on every call
        std::map<int, hipGraphExec_t> graphs;
        int capture_backoff = 0, capture_skip = 0;       // steps to run eagerly before the next capture attempt after one that could not get its turn
    } sb[2];
    bool graph_broken = false;                           // a capture failed half-way: this handle runs plain launches from now on
    int graph_captures = 0, graph_skipped = 0;           // EagleTimings::graph_captures / graph_skipped
    std::unique_ptr<Net> hr, yo, misc, reid;
    // K16 appearance embeddings (OSNet-x0.25; built when the "reid.*" tensors were loaded): REID_NB crops per pass
    TView reid_in; float* reid_feats = nullptr; EagleCrop* reid_crops = nullptr; EagleCrop* reid_crops_h = nullptr; float* reid_feats_h = nullptr;
    eagle::Tracker* tracker = nullptr;       // K14 state of the clip being tracked (eagle_track_*)
    std::unique_ptr<CopyPool> pool;          // host-side copy workers (eagle_process_frames from pageable memory)
    // step buffers
    TView kp_in, det_in, logits;             // kp_in.p == nullptr: the fused stem reads the frames itself (stem_on)
    bool stem_on = false;                    // HRNet's first launch is stem.hip: no key-point half of K1, no kp_in tensor
    const uint8_t* cur_src = nullptr;        // frames of the step being enqueued (device) and their number: what the stem launch reads
    int cur_n = 0;
    LetterBox lb;
    int hm_chunks = 64;                      // heat-map partials per channel and frame (fused: output tiles of the head convolution)
    ArgmaxPart* cur_parts = nullptr;         // where the head convolution of the step being enqueued writes its partials (fused K5)
    unsigned* cur_sat = nullptr;             // where the f32s kernels of the step being enqueued count saturated stores per frame
    unsigned* clip_sat = nullptr;            // the same for the passes of a clip session (read by eagle_clip_fetch), pinned host copy behind it
    unsigned* clip_sat_h = nullptr;
    long long sat_events = 0; int sat_frames = 0;      // of the last eagle_process_* / eagle_clip_fetch call
    bool fused_argmax = false;
    DetScratch ds;
    DetLevel levels[3];
    PostParams pp;
    bool warmed = false;
    int call_steps = 0;                      // steps of the eagle_process_* call being executed (graph_on)
    // profiling
    bool prof = false;
    std::vector<hipEvent_t> conv_ev;
    struct Span { int k; double bytes; hipEvent_t a, b; };
    std::vector<hipEvent_t> span_pool; size_t span_used = 0;
    std::vector<Span> spans;                     // non-convolution launches of the step being profiled
    std::vector<EagleKernelTime> ktab;           // accumulated per kernel name since eagle_set_profiling(1)
    std::vector<const Op*> conv_ops;             // the convolution behind each conv_ev pair of the step being profiled
    EagleTimings timings{};
    double conv_flop_step = 0; int n_conv = 0, n_launch = 0;
    // clip session of the optical-flow cadence (eagle_clip_*)
    struct Clip {
        bool open = false;
        ClipView cv;
        uint8_t* g[3] = {nullptr, nullptr, nullptr};
        EagleFrameResult* recs = nullptr;
        MemList* mem = nullptr;
        ChainState* st = nullptr;          // loop state
        ChainState* st_op = nullptr;       // scratch state of eagle_clip_flow
        ChainState* h_st = nullptr;        // pinned staging of eagle_clip_flow
        ChainState* h_zero = nullptr;      // pinned: the initial loop state
        int* h_tail = nullptr;             // pinned: {stalled, error} read-back, [2] = the constant -1
        MemList* h_mem = nullptr;          // pinned staging of eagle_clip_get/set_keypoints
        hipEvent_t ev_gray = nullptr, ev_det = nullptr, ev_kp = nullptr, ev_loop = nullptr;
        uint8_t* ecc_small = nullptr;      // K17: [n, ecc_h, ecc_w] 0.15-scale gray images (built on the first eagle_clip_motion_ecc call)
        int ecc_h = 0, ecc_w = 0;
        int2* ecc_pairs = nullptr; eagle::EccResult* ecc_out = nullptr;   // device, n entries
        int ecc_next = -1, ecc_tmpl = -2;  // eagle_clip_motion_ecc called range after range: the frame the last call stopped in front of, and the template it left
                                           // (a clip frame, or -1 = the carried template); a failed alignment keeps the OLD template across calls too
    } clip;
    // boxmot's ECC object lives as long as the tracker: the last template survives the clip (carried by eagle_clip_motion_ecc, reset by eagle_track_open)
    uint8_t* ecc_prev = nullptr; int ecc_prev_h = 0, ecc_prev_w = 0; bool ecc_has_prev = false;
    // comm
    void* rccl = nullptr; void* comm = nullptr; int rank = 0, world = 1;
    void* gather_buf = nullptr; size_t gather_cap = 0;      // device staging of eagle_gather (send | receive), grown on demand
    // annotated output (annotate.hip): the primitive lists of the call being run (device), and the device / pinned staging of eagle_annotate_frames.
    // Grown on demand, the handle's own: an annotate call touches neither the step's staging buffers nor its graphs
    void* annot_prims = nullptr; size_t annot_prims_cap = 0;
    uint8_t* annot_out = nullptr; size_t annot_out_cap = 0;
    uint8_t* annot_ring = nullptr; size_t annot_ring_cap = 0;
    // minimap (minimap.hip): the draw lists of the call being run, the drawable columns and the marking mask of the last (scale, margin); grown on demand
    void* mm_list = nullptr; size_t mm_list_cap = 0;
    void* mm_cols = nullptr; size_t mm_cols_cap = 0;
    // the K25 layers of the call being run (minimap.hip layers_setup): selection, frame numbers, points, links, events, prepared events, event ranges, still picture, hull edges (K26)
    void* mm_tr[9] = {}; size_t mm_tr_cap[9] = {};
    uint8_t* mm_mask = nullptr; size_t mm_mask_cap = 0; int mm_mask_scale = 0, mm_mask_margin = -1;
    // pitch control (control.hip): the site lists and site columns of the call being run, and the grids the minimap's control layer reads; grown on demand
    void* ct_list = nullptr; size_t ct_list_cap = 0;
    void* ct_cols = nullptr; size_t ct_cols_cap = 0;
    void* ct_grid = nullptr; size_t ct_grid_cap = 0;
};

// A processed clip table (post.hip builds it; minimap.hip draws it)
struct EaglePostTable {
    EagleHandle* h = nullptr;
    int rows = 0, cols = 0, flags = 0;
    std::vector<int32_t> frames;
    std::vector<EaglePostColumn> columns;
    std::vector<int32_t> team_ids, team_vals;
    bool has_team = false;
    std::vector<EaglePostMerge> merges;  // merge_ids = 1: the accepted links, in acceptance order
    double* d_values = nullptr;          // [cols][rows][2], resident until eagle_post_free
    std::vector<double> host;            // the same on the host, fetched on first use (getters, overlays)
    bool host_ok = false;
    double* d_vel = nullptr;             // velocities, same layout (eagle_post_velocities), resident until eagle_post_free
    EagleKinematicsParams kin{};
    std::vector<double> host_vel;
    bool host_vel_ok = false;
    bool has_control = false;            // eagle_minimap_set_control
    EagleControlParams control{};
    void* d_poss = nullptr;              // possession (eagle_post_possession): dist [rows] f64 | cand [rows] i32 | owner [rows] i32, resident until eagle_post_free
    bool has_poss = false;
    std::vector<EaglePossessionEvent> events;
    int64_t max_bytes = 0;               // eagle_postprocess's memory budget (0: nine tenths of what is free): later results kept with the table answer to it too
    void* d_occ = nullptr;               // occupancy (eagle_post_occupancy): grids f32 | counts i32 | bytes u8, [occ_nsel][gh][gw] each, then total | outside | max
    int occ_nsel = 0, occ_R = 0;         // u32 [occ_nsel] each; resident until eagle_post_free
    bool has_occ = false;
    bool has_trails = false;             // eagle_minimap_set_trails
    EagleTrailParams trails{};
    std::vector<int32_t> trail_cols;
    void* d_shape = nullptr;             // team shape (eagle_post_team_shape): EagleTeamShape [rows][2] | hull i32 [rows][2][32], resident until eagle_post_free
    bool has_shape = false;
    bool has_hulls = false;              // eagle_minimap_set_hulls
    EagleHullParams hulls{};
    void* d_phys = nullptr;              // physical report (eagle_post_physical): speed f64 | accel f64 | zone u8, [phys_persons][rows] each, resident until eagle_post_free
    int phys_persons = 0;
    bool has_phys = false;
    std::vector<EagleLoadTotals> phys_totals;
    std::vector<EagleLoadEffort> phys_efforts;
    void* d_roles = nullptr;             // roles (eagle_post_roles): EagleRoleRow [rows][2] | EagleRoleModel | role i8 [roles_members][rows], each from a 256-byte
    int roles_members = 0;               // boundary; resident until eagle_post_free
    bool has_roles = false;
    void* d_space = nullptr;             // space (eagle_post_space): EagleSpaceRow [rows] | EagleSpaceSite [rows][32] | EagleSpaceTotals [space_members], each from a
    int space_members = 0;               // 256-byte boundary; nullptr before the first call, resident until eagle_post_free
    void* d_offside = nullptr;           // offside (eagle_post_offside): EagleOffsideRow [rows][2] | margins i32 [offside_members][rows] | EagleOffsideTotals
    int offside_members = 0;             // [offside_members] | EagleOffsideClip | EagleOffsideEvent [offside_events], each from a 256-byte boundary; nullptr
    int offside_events = 0;              // before the first call, resident until eagle_post_free
    double* d_raw = nullptr;             // track smoothing (eagle_post_smooth_tracks): the positions from before it, the layout of d_values
    void* d_smooth = nullptr;            // acc f64 [cols][rows][2] | residual_q i32 | flags u8 | count u8 [cols][rows] | suspect u8 [rows] | EagleSmoothTotals [cols],
    bool has_smooth = false;             // each from a 256-byte boundary; both nullptr before the call, resident until eagle_post_free
    std::vector<EagleSmoothTotals> smooth_totals;
    double* d_orig = nullptr;            // stabilisation (eagle_post_stabilise): the positions from before it, the layout of d_values
    void* d_stab = nullptr;              // EagleStabRow [rows] | votes i32 [cols][rows][2] | EagleStabTotals, each from a 256-byte boundary; both nullptr before
    bool has_stab = false;               // the call, resident until eagle_post_free
    EagleStabTotals stab_totals{};
    void* d_flights = nullptr;           // ball flights (eagle_post_ball_flights): seg i32 [rows] | flags u8 [rows] | fitted f64 [rows][2] | velocity f64 [rows][2], each
    bool has_flights = false;            // from a 256-byte boundary; nullptr before the first call (and with no rows), resident until eagle_post_free
    std::vector<EagleBallFlight> flights;
    std::vector<EagleBallKick> kicks;
    EagleFlightTotals flight_totals{};
    void* d_goalview = nullptr;          // goal view (eagle_post_goal_view): EagleGoalViewRow [rows][2] | open i32 | mask u64 | status u8 [goalview_members][rows] |
    int goalview_members = 0;            // EagleGoalViewTotals [goalview_members] | grid u8 [goalview_grid_rows][68 R][105 R], each from a 256-byte boundary;
    int goalview_grid_row0 = 0, goalview_grid_rows = 0, goalview_R = 0;   // nullptr before the first call, resident until eagle_post_free
};

namespace eagle {
constexpr int REID_NB = 64;                    // crops per pass of the appearance network
void finalize(EagleHandle* h);                                                  // nets.hip
size_t sat_pad_bytes(int B);                                                    // step.hip
void run_net(EagleHandle* h, Net* net, hipStream_t s, size_t& ev_i);
void check_saturation(EagleHandle* h, const char* what);
// profiling mode: HIP events around fn()'s launches on stream st, accumulated under `name` with their algorithmic bytes by collect_spans; otherwise just fn()
void timed_launch(EagleHandle* h, const char* name, double bytes, hipStream_t st, const std::function<void()>& fn);
void collect_spans(EagleHandle* h);                                             // after the stream has been synchronised
// one plane of a frame in caller memory: `rows` rows of `row_bytes` bytes at off + r * pitch; at dense_off + r * row_bytes in the dense frame
struct HostPlane { int64_t off, pitch, rows, row_bytes, dense_off; };
// layout of a caller's frames: 4:2:0 (eagle_*_yuv, and the output of eagle_annotate_*) or, for annotated output only, pitched BGR (one plane)
struct YuvGeom {
    int fmt, h, w, nplanes;
    int64_t frame_stride, y_pitch, c_offset, c_pitch, v_offset;
    int64_t extent;          // bytes of one frame from its start to the end of its last row
    int64_t dense_bytes;     // h * w * 3 / 2 (BGR: h * w * 3)
    bool dense;              // the layout is the dense default
    HostPlane pl[3];          // Y, then UV (NV12) or U, V (I420); BGR: the frame
};
// The one argument check of every entry that takes an EagleYuvLayout: fills the dense defaults and rejects what a kernel cannot read or write safely.
YuvGeom yuv_geometry(int fmt, int h, int w, const EagleYuvLayout* L, bool output = false);      // output: EAGLE_PIX_BGR is a format too
bool host_pinned(EagleHandle* h, const void* p);
// annotate.hip: the kernel's view of an output layout the one check (yuv_geometry) has resolved
AnnotArgs annot_args(const YuvGeom& g, const uint8_t* src, uint8_t* dst, const EaglePrim* prims, const int32_t* offs);
// n pictures of fh x fw -> host memory in the caller's layout: draw(first, count, dense geometry, d_dst) renders `count` (<= batch) of them into the handle's
// device staging and returns when they are complete; a pinned destination is DMA'd, a pageable one goes through the handle's pinned ring
void frames_to_host(EagleHandle* h, int n, int fh, int fw, int batch, int out_format, const EagleYuvLayout* out_layout, uint8_t* out,
                    const std::function<void(int, int, const YuvGeom&, uint8_t*)>& draw);
void clip_close(EagleHandle* h);                                                // clip.hip
// post.hip: post_velocity_kernel over a whole table on stream s (smooth.hip keeps its result for the columns it does not smooth)
void velocity_check(const EagleKinematicsParams* p);
void velocity_launch(const double2* values, const int32_t* frames, double2* out, int rows, int cols, const EagleKinematicsParams* p, hipStream_t s);
// control.hip: what the minimap's control layer needs from it
struct CtCol { int32_t col; int32_t team0; };              // a site column of the table: a mapped Player pitch column, and whether its team is 0
struct ControlArgs {
    const double2* values;       // the table and its velocities, [column][row]
    const double2* vel;
    const CtCol* cols;           // site columns in table order
    float4* lists;               // [n][stride]: {count}, then per site {qx, qy, team 0 ? 1 : 0}
    uint8_t* out;                // [n][gh][gw]
    unsigned long long* share;   // [n] sums of the bytes (zeroed in front of the launch), or nullptr
    int rows, row0, n, ncols, stride, R, gw, gh;
    float t_react, v_max, beta;
};
static constexpr int CT_PASS = 65535;                      // gridDim.y limit
void control_check(const EagleControlParams* p);                                // EAGLE_E_INVALID unless the parameters are in range
void control_columns(const EaglePostColumn* columns, int ncols, const int32_t* team_ids, const int32_t* team_vals, size_t n_team, std::vector<CtCol>& out);
void control_launch(const ControlArgs& a, hipStream_t s);                       // n <= CT_PASS rows: (share memset,) sites, grids
ControlArgs control_prepare(EagleHandle* h, EaglePostTable* t, const EagleControlParams* p, int max_pass);      // site columns uploaded, list space for max_pass rows
void control_rows(EagleHandle* h, const ControlArgs& prepared, int row0, int n, uint8_t* d_out, int64_t* d_share);   // enqueued on s_main, not awaited
// minimap.hip: what the occupancy picture (occupancy.hip) shares with it
struct MmPlan { int S, M, w, h, r, rb, t; };
MmPlan minimap_plan(const EagleMinimapParams* p);                               // EAGLE_E_INVALID unless the parameters are in range; canvas size and radii
std::vector<uint8_t> markings_mask(const MmPlan& pl, int* pitch);               // the white markings of a (scale, margin) as a bit mask, rows of (w + 7) / 8 bytes
const uint8_t* minimap_mask(EagleHandle* h, const MmPlan& pl);                  // the same in HBM, kept in the handle for the last (scale, margin); synchronises s_main
// shape.hip (K26): what the minimap's hull layer and eagle_op_minimap_hulls need from it
struct ShapeCols { std::vector<int32_t> gcols; int n0 = 0, n1 = 0; };   // the member columns in table order, group 0's and then group 1's
// EAGLE_E_INVALID without a mapping, for a column of unknown kind and beyond EAGLE_SHAPE_MAX_MEMBERS members
ShapeCols shape_columns(const char* who, const EaglePostColumn* columns, int ncols, const int32_t* team_ids, const int32_t* team_vals, size_t n_team);
void hull_check(const char* who, const EagleHullParams* p);
// the two launches on stream s (h: timed under its profiling mode, or nullptr); returns when the records and vertices are complete
void shape_run(EagleHandle* h, const ShapeCols& sc, const double2* d_values, int rows, EagleTeamShape* d_shapes, int32_t* d_hull, hipStream_t s);
// rows row0 .. row0 + n - 1 -> edges [n][2][EAGLE_SHAPE_HULL_CAP] = {A, B} in the minimap's quantisation (x == MM_ABSENT: no edge); no synchronisation
// offside.hip (K33): the members of groups 0 and 1, the keepers and the ball of a table; goalview.hip (K41) takes its groups from here too
struct OfCols { std::vector<int4> list; std::vector<int32_t> gcols, member_of; std::vector<EagleOffsideTotals> init; EagleOffsideClip clip{}; int n0 = 0, n1 = 0, ball = -1; };
OfCols offside_columns(const char* who, const EaglePostColumn* columns, int ncols, bool no_ball, const int32_t* team_ids, const int32_t* team_vals, size_t n_team,
                       const EagleOffsideParams* p);
void shape_edges_launch(const double2* values, int rows, const EagleTeamShape* shapes, const int32_t* hull, int row0, int n, int scale, int margin, int4* edges, hipStream_t s);
}  // namespace eagle

// ---- C ABI: the body of every entry runs between API_BEGIN and API_END ---------------------------------------
#define API_BEGIN try { eagle::ApiGuard api_guard_;
#define API_BEGIN_H(h) if (!(h)) return EAGLE_E_INVALID; API_BEGIN      // an entry that needs a handle
#define API_END(h)                                                       \
    }                                                                    \
    catch (const eagle::Err& e) { if (h) (h)->err = e.msg; else eagle::g_create_error = e.msg; return e.code; } \
    catch (const std::exception& e) { if (h) (h)->err = e.what(); else eagle::g_create_error = e.what(); return EAGLE_E_INVALID; } \
    return EAGLE_OK;
