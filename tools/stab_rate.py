#!/usr/bin/env python3
"""Cost of the stabilisation kernels (include/eagle.h, eagle_post_stabilise; csrc/stab.hip): one JSON line.

    python tools/stab_rate.py [--rows 30000] [--players 22] [--reps 3] [--windows 10,25,64] [--iterations 2]

A processed table of --rows rows is built by eagle_postprocess from constructed records (--players players, 2 goalkeepers and the ball on a random walk:
tools/control_rate.py's table; 24 person columns at the defaults), and per half-width W eagle_post_stabilise is called on --reps fresh tables (a table is
stabilised once) after a warm-up.  Every launch is timed separately (HIP events of the profiling mode): the median over the repetitions of the time PER
LAUNCH (a round's kernels run --iterations times a call), the sum of all launches of a call, and the wall time of a call.  Next to them, on the same
table and at the same half-width, the yardstick: K37's four launches (eagle_post_smooth_tracks: fit, flag, refit, totals) summed.

The two forms of the estimate kernel.  The library's stab_estimate_kernel is the plain gather (a wave's reads of its row are strided by the row count).
The COMPARISON FORM, a workgroup of four waves that stages 64 columns x 16 rows through LDS with the rows of a column contiguous and then gives each wave
four rows, lives in this tool only: it is compiled with hipcc when the tool runs, together with a second copy of the gather, both from
csrc/stab_estimate.inc (the estimate of a row by a wave), so the two differ in their reads alone.  Both run on the votes and integers of the same table
(the table's own positions quantised, its rows' common error drawn at random: the estimate does not depend on W), are timed with HIP events of the
tool's own, and their row records are compared byte for byte with each other."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from eagle_amd import lib, weights  # noqa: E402
from control_rate import records  # noqa: E402

NAMES = ("stab_quantise", "stab_predict", "stab_estimate", "stab_apply", "stab_totals")
SMOOTH = ("smooth_fit", "smooth_flag", "smooth_refit", "smooth_totals")

BOTH_FORMS = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <vector>
#include "eagle.h"
namespace eagle {
#include "stab_estimate.inc"
static constexpr int ST_TROWS = 16;            // rows of a transposed block: four per wave
// the comparison form: 64 columns x 16 rows staged through LDS, the rows of a column contiguous (thread -> column threadIdx.x / 16 + 16 k, row threadIdx.x % 16)
__global__ __launch_bounds__(ST_WAVES * 64) void stab_estimate_transposed_kernel(StabArgs a)
{
    __shared__ StSlots slots[ST_TROWS];
    __shared__ int2 t_d[64][ST_TROWS + 1];
    __shared__ uint8_t t_s[64][ST_TROWS + 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rb = blockIdx.x * ST_TROWS;
    int found[ST_TROWS / ST_WAVES] = {}, moved[ST_TROWS / ST_WAVES] = {};
    for (int c0 = 0; c0 < a.cols; c0 += 64) {
        for (int k = 0; k < 64; k += ST_WAVES * 64 / ST_TROWS) {
            const int cl = k + threadIdx.x / ST_TROWS, rl = threadIdx.x % ST_TROWS;
            int2 d;
            t_s[cl][rl] = (uint8_t)st_cell(a, c0 + cl, rb + rl, d);
            t_d[cl][rl] = d;
        }
        __syncthreads();
        #pragma unroll
        for (int i = 0; i < ST_TROWS / ST_WAVES; ++i) {
            const int rl = wave * (ST_TROWS / ST_WAVES) + i;
            st_compact(t_s[lane][rl], t_d[lane][rl], c0 + lane, lane, found[i], moved[i], slots[rl]);
        }
        __syncthreads();                                    // the block is rewritten for the next 64 columns
    }
    #pragma unroll
    for (int i = 0; i < ST_TROWS / ST_WAVES; ++i) {
        const int rl = wave * (ST_TROWS / ST_WAVES) + i;
        if (rb + rl < a.rows) st_row_estimate(a, rb + rl, found[i], moved[i], slots[rl], lane);
    }
}
}  // namespace eagle
// host arrays [cols][rows] (kind [cols]); reps timed launches of each form after one warm-up -> ms_gather[reps], ms_transposed[reps]; the records of
// the gather -> rec_out [rows]; *equal: the two forms' records are the same bytes
extern "C" int time_estimate(const uint8_t* kind, const uint8_t* present, const uint8_t* voteb, const int32_t* votes, const int32_t* q, int rows, int cols, int model,
                             int min_voters, double trim_k, double floor_q, double lim_s, double max_gain, double jump_q, int reps, float* ms_gather, float* ms_transposed,
                             EagleStabRow* rec_out, int* equal)
{
    using namespace eagle;
    const size_t cells = (size_t)rows * cols;
    uint8_t *d_kind = nullptr, *d_present = nullptr, *d_voteb = nullptr;
    int2 *d_votes = nullptr, *d_q = nullptr;
    EagleStabRow* d_rec[2] = {nullptr, nullptr};
    hipEvent_t e0, e1;
    if (hipMalloc((void**)&d_kind, cols) || hipMalloc((void**)&d_present, cells) || hipMalloc((void**)&d_voteb, cells) || hipMalloc((void**)&d_votes, cells * 8) ||
        hipMalloc((void**)&d_q, cells * 8) || hipMalloc((void**)&d_rec[0], (size_t)rows * sizeof(EagleStabRow)) || hipMalloc((void**)&d_rec[1], (size_t)rows * sizeof(EagleStabRow)))
        return 1;
    if (hipMemcpy(d_kind, kind, cols, hipMemcpyHostToDevice) || hipMemcpy(d_present, present, cells, hipMemcpyHostToDevice) || hipMemcpy(d_voteb, voteb, cells, hipMemcpyHostToDevice) ||
        hipMemcpy(d_votes, votes, cells * 8, hipMemcpyHostToDevice) || hipMemcpy(d_q, q, cells * 8, hipMemcpyHostToDevice) || hipEventCreate(&e0) || hipEventCreate(&e1))
        return 2;
    StabArgs a{};
    a.kind = d_kind; a.present = d_present; a.voteb = d_voteb; a.votes = d_votes; a.q = d_q; a.rows = rows; a.cols = cols; a.model = model; a.min_voters = min_voters;
    a.trim_k = trim_k; a.floor_q = floor_q; a.lim_s = lim_s; a.max_gain = max_gain; a.jump_q = jump_q;
    for (int form = 0; form < 2; ++form) {
        a.rec = d_rec[form];
        if (hipMemset(a.rec, 0xff, (size_t)rows * sizeof(EagleStabRow))) return 3;
        for (int i = -1; i < reps; ++i) {
            hipEventRecord(e0, nullptr);
            if (form == 0) hipLaunchKernelGGL(stab_estimate_kernel, dim3((rows + ST_WAVES - 1) / ST_WAVES), dim3(ST_WAVES * 64), 0, nullptr, a);
            else hipLaunchKernelGGL(stab_estimate_transposed_kernel, dim3((rows + ST_TROWS - 1) / ST_TROWS), dim3(ST_WAVES * 64), 0, nullptr, a);
            hipEventRecord(e1, nullptr);
            if (hipEventSynchronize(e1) || hipGetLastError()) return 4;
            if (i >= 0) hipEventElapsedTime((form == 0 ? ms_gather : ms_transposed) + i, e0, e1);
        }
    }
    std::vector<EagleStabRow> other((size_t)rows);
    int rc = 0;
    if (hipMemcpy(rec_out, d_rec[0], (size_t)rows * sizeof(EagleStabRow), hipMemcpyDeviceToHost) || hipMemcpy(other.data(), d_rec[1], (size_t)rows * sizeof(EagleStabRow), hipMemcpyDeviceToHost))
        rc = 5;
    *equal = rc == 0 && std::memcmp(rec_out, other.data(), (size_t)rows * sizeof(EagleStabRow)) == 0;
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(d_kind); hipFree(d_present); hipFree(d_voteb); hipFree(d_votes); hipFree(d_q); hipFree(d_rec[0]); hipFree(d_rec[1]);
    return rc;
}
"""


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms[0]), 4), "ms_max": round(float(ms[-1]), 4)}


def build_both_forms(tmp):
    src, so = os.path.join(tmp, "stab_forms.hip"), os.path.join(tmp, "stab_forms.so")
    with open(src, "w") as f:
        f.write(BOTH_FORMS)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-std=c++17", "-Wno-unused-result",
                           "-Wno-unused-value", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "eagle_amd", "csrc"), "-shared", "-fPIC", src, "-o", so])
    L = C.CDLL(so)
    vp, i32, f64 = C.c_void_p, C.c_int, C.c_double
    L.time_estimate.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, f64, f64, f64, f64, f64, i32, vp, vp, vp, vp]
    return L


def estimate_input(values, columns, seed=0):
    """the table's positions and columns -> kind [cols], present, voteb uint8 [cols][rows], votes, q int32 [cols][rows][2]: every present person cell of
    the inner rows votes its row's common error (a random shift of up to 0.4 m and gains of up to 0.6 %) plus 0.08 m of noise"""
    rng = np.random.default_rng(seed)
    cols, rows = values.shape[:2]
    kind = np.array([0 if k["video"] else 3 if int(k["kind"]) in (lib.POST_PLAYER, lib.POST_GOALKEEPER) else 1 if int(k["kind"]) == lib.POST_BALL else 0 for k in columns], np.uint8)
    with np.errstate(invalid="ignore"):
        present = ((np.abs(values) <= 1024.0).all(2) & (kind != 0)[:, None]).astype(np.uint8)
    q = np.where(present[:, :, None] != 0, np.rint(np.nan_to_num(values) * 1024.0), 0).astype(np.int32)
    e = np.concatenate([rng.uniform(-0.4, 0.4, (rows, 2)), rng.uniform(-0.006, 0.006, (rows, 4))], 1)
    x, y = q[:, :, 0] / 1024.0, q[:, :, 1] / 1024.0
    d = np.stack([e[:, 0] + e[:, 2] * x + e[:, 3] * y, e[:, 1] + e[:, 4] * x + e[:, 5] * y], 2) + rng.normal(0.0, 0.08, q.shape)
    voteb = present & (kind == 3)[:, None]
    voteb[:, 0] = voteb[:, -1] = 0
    votes = np.where(voteb[:, :, None] != 0, np.rint(d * 1024.0), 0).astype(np.int32)
    return kind, np.ascontiguousarray(present), np.ascontiguousarray(voteb), np.ascontiguousarray(votes), np.ascontiguousarray(q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--players", type=int, default=22)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", default="10,25,64")
    ap.add_argument("--iterations", type=int, default=2)
    a = ap.parse_args()
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    tm = {i + 1: i % 2 for i in range(a.players)}
    recs = records(a.rows, a.players, 2)
    res = {"reps": a.reps, "iterations": a.iterations}

    def profiled(call, names):
        """call(table) on --reps fresh tables after a warm-up -> per name the (total ms, launches) of every repetition, and the wall times"""
        spans, wall = {k: [] for k in names}, []
        for rep in range(-1, a.reps):
            t = h.postprocess(recs, 25, 1280, tm)
            try:
                h.set_profiling(1)
                t0 = time.perf_counter()
                call(t)
                dt = time.perf_counter() - t0
                times = h.kernel_times()
                h.set_profiling(0)
                if rep >= 0:
                    wall.append(dt * 1e3)
                    for k in names:
                        spans[k].append((sum(x[1] for x in times if x[0] == k), sum(x[2] for x in times if x[0] == k)))
            finally:
                t.close()
        return spans, wall

    try:
        # the two forms of the estimate kernel on one input
        t = h.postprocess(recs, 25, 1280, tm)
        try:
            values, columns = t.values.copy(), t.columns.copy()
        finally:
            t.close()
        cols, rows = values.shape[:2]
        res.update(rows=rows, columns=cols)
        kind, present, voteb, votes, q = estimate_input(values, columns)
        res.update(voting_columns=int((kind == 3).sum()), moved_columns=int((kind != 0).sum()))
        p = lib.stab_params(25)
        with tempfile.TemporaryDirectory() as tmp:
            G = build_both_forms(tmp)
            ms_g, ms_t = np.zeros(a.reps, np.float32), np.zeros(a.reps, np.float32)
            rec, equal = np.zeros(rows, lib.STAB_ROW_DTYPE), C.c_int(0)
            ptr = lambda x: x.ctypes.data_as(C.c_void_p)
            smin = p.min_spread * 1024.0
            rc = G.time_estimate(ptr(kind), ptr(present), ptr(voteb), ptr(votes), ptr(q), rows, cols, p.model, p.min_voters, p.trim_k, p.floor * 1024.0, smin * smin, p.max_gain,
                                 p.jump * 1024.0, a.reps, ptr(ms_g), ptr(ms_t), ptr(rec), C.byref(equal))
            assert rc == 0, rc
        res["estimate_forms"] = {"gather": stats(ms_g), "transposed_through_lds": stats(ms_t), "records_equal": bool(equal.value),
                                 "rows_per_model_none_translation_affine": [int((rec["model"] == m).sum()) for m in (0, 1, 2)]}
        for W in (int(w) for w in a.windows.split(",")):
            p = lib.stab_params(25, window=W, iterations=a.iterations)
            spans, wall = profiled(lambda t: h._check(h.L.eagle_post_stabilise(h._h, t._t, C.byref(p)), "post_stabilise"), NAMES)
            out = {k: {**stats([ms / max(n, 1) for ms, n in spans[k]]), "launches_per_call": spans[k][0][1]} for k in NAMES}
            out["all_launches_ms"] = stats([sum(spans[k][i][0] for k in NAMES) for i in range(a.reps)])
            out["wall_ms_per_call_profiled"] = stats(wall)
            sp = lib.smooth_params(25, window=W)
            spans, wall = profiled(lambda t: h._check(h.L.eagle_post_smooth_tracks(h._h, t._t, C.byref(sp)), "post_smooth_tracks"), SMOOTH)
            out["k37_four_launches_ms"] = stats([sum(spans[k][i][0] for k in SMOOTH) for i in range(a.reps)])
            res[f"window_{W}"] = out
    finally:
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
