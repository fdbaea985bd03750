#!/usr/bin/env python3
"""Cost of the track-smoothing kernels (include/eagle.h, eagle_post_smooth_tracks; csrc/smooth.hip): one JSON line.

    python tools/smooth_rate.py [--rows 30000] [--players 20] [--reps 5] [--windows 10,64]

A processed table of --rows rows is built by eagle_postprocess from constructed records (--players players, 2 goalkeepers and the ball on a random walk:
tools/control_rate.py's table; 24 person columns at the defaults), and per half-width W eagle_post_smooth_tracks is called on --reps fresh tables (a table
is smoothed once) after a warm-up.  Each of the four launches is timed separately (HIP events of the profiling mode): median, minimum and maximum, and in
GB/s against the bytes it moves per smoothed cell (fit 24, flag 9, refit 71, totals 6).  Next to them: eagle_post_velocities on the same table (32 bytes
a cell: the bandwidth yardstick), the wall time of a whole call, and the COMPARISON FORM of the fit: the same sums and solve with every window sample read
and quantised from global memory instead of the LDS tile.  That kernel lives in this tool only (compiled with hipcc when the tool runs, timed with HIP
events of its own, its residuals compared bit for bit with tests/smooth_ref.py on the first rows of one column)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from eagle_amd import lib, weights  # noqa: E402
from control_rate import records  # noqa: E402

NAMES = ("smooth_fit", "smooth_flag", "smooth_refit", "smooth_totals")
BYTES = {"smooth_fit": 24.0, "smooth_flag": 9.0, "smooth_refit": 71.0, "smooth_totals": 6.0}

GLOBAL_FORM = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
// the fit of csrc/smooth.hip, pass 1, without the LDS tile: one thread per (column, row), every sample of its window read and quantised from HBM / cache
__global__ __launch_bounds__(256) void fit_global(const double2* values, const int32_t* frames, const int32_t* clist, int rows, int W, int degree, double* e_out)
{
    const int r = blockIdx.x * 256 + threadIdx.x, c = clist[blockIdx.y];
    if (r >= rows) return;
    const double2* A = values + (size_t)c * rows;
    const double2 me = A[r];
    double e = -1.0;
    if (fabs(me.x) <= 1024.0 && fabs(me.y) <= 1024.0) {
        long long S0 = 0, S1 = 0, S2 = 0, S3 = 0, S4 = 0, X0 = 0, X1 = 0, X2 = 0, Y0 = 0, Y1 = 0, Y2 = 0;
        const int fr = frames[r];
        const int lo = r - W < 0 ? 0 : r - W, hi = r + W >= rows ? rows - 1 : r + W;
        for (int j = lo; j <= hi; ++j) {
            const double2 v = A[j];
            if (!(fabs(v.x) <= 1024.0 && fabs(v.y) <= 1024.0)) continue;
            const long long d = (long long)frames[j] - fr;
            if (d < -W || d > W) continue;
            const long long d2 = d * d, x = (long long)rint(v.x * 1024.0), y = (long long)rint(v.y * 1024.0);
            S0 += 1; S1 += d; S2 += d2; S3 += d2 * d; S4 += d2 * d2;
            X0 += x; X1 += d * x; X2 += d2 * x;
            Y0 += y; Y1 += d * y; Y2 += d2 * y;
        }
        const int deg = S0 >= 4 ? degree : S0 == 3 ? (degree < 1 ? degree : 1) : S0 == 2 ? 1 : 0;
        const double s0 = (double)S0, s1 = (double)S1, s2 = (double)S2, s3 = (double)S3, s4 = (double)S4;
        double ax, ay;
        if (deg == 2) {
            const double C00 = s2 * s4 - s3 * s3, C01 = s2 * s3 - s1 * s4, C02 = s1 * s3 - s2 * s2;
            const double det = (s0 * C00 + s1 * C01) + s2 * C02;
            ax = ((C00 * (double)X0 + C01 * (double)X1) + C02 * (double)X2) / det;
            ay = ((C00 * (double)Y0 + C01 * (double)Y1) + C02 * (double)Y2) / det;
        } else if (deg == 1) {
            const double det = s0 * s2 - s1 * s1;
            ax = (s2 * (double)X0 - s1 * (double)X1) / det;
            ay = (s2 * (double)Y0 - s1 * (double)Y1) / det;
        } else { ax = (double)X0 / s0; ay = (double)Y0 / s0; }
        e = fmax(fabs(rint(me.x * 1024.0) - ax), fabs(rint(me.y * 1024.0) - ay));
    }
    e_out[(size_t)blockIdx.y * rows + r] = e;
}
// the ncols columns clist of the device table; reps timed launches after one warm-up -> ms[reps]; the residuals of the last launch -> e_host [ncols][rows]
extern "C" int time_fit_global(const double* d_values, const int32_t* frames, int rows, const int32_t* clist, int ncols, int W, int degree, int reps, float* ms, double* e_host)
{
    int32_t *d_f = nullptr, *d_c = nullptr; double* d_e = nullptr;
    hipEvent_t a, b;
    if (hipMalloc((void**)&d_f, (size_t)rows * 4) || hipMalloc((void**)&d_c, (size_t)ncols * 4) || hipMalloc((void**)&d_e, (size_t)rows * ncols * 8)) return 1;
    if (hipMemcpy(d_f, frames, (size_t)rows * 4, hipMemcpyHostToDevice) || hipMemcpy(d_c, clist, (size_t)ncols * 4, hipMemcpyHostToDevice) || hipEventCreate(&a) || hipEventCreate(&b))
        return 2;
    const double2* v = (const double2*)d_values;
    const dim3 grid((rows + 255) / 256, ncols);
    for (int i = -1; i < reps; ++i) {
        hipEventRecord(a, nullptr);
        hipLaunchKernelGGL(fit_global, grid, dim3(256), 0, nullptr, v, d_f, d_c, rows, W, degree, d_e);
        hipEventRecord(b, nullptr);
        if (hipEventSynchronize(b) || hipGetLastError()) return 3;
        if (i >= 0) hipEventElapsedTime(ms + i, a, b);
    }
    const int rc = hipMemcpy(e_host, d_e, (size_t)rows * ncols * 8, hipMemcpyDeviceToHost) ? 4 : 0;
    hipEventDestroy(a); hipEventDestroy(b); hipFree(d_f); hipFree(d_c); hipFree(d_e);
    return rc;
}
"""


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms[0]), 4), "ms_max": round(float(ms[-1]), 4)}


def build_global_form(tmp):
    src, so = os.path.join(tmp, "fit_global.hip"), os.path.join(tmp, "fit_global.so")
    with open(src, "w") as f:
        f.write(GLOBAL_FORM)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-Wno-unused-result", "-Wno-unused-value", "-shared", "-fPIC", src, "-o", so])
    L = C.CDLL(so)
    L.time_fit_global.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=30000)
    ap.add_argument("--players", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", default="10,64")
    a = ap.parse_args()
    h = lib.Handle(batch=10)
    weights.load_into(h, [weights.make_hrnet_state_dict(0), weights.make_yolo_state_dict("n", 0)])
    tm = {i + 1: i % 2 for i in range(a.players)}
    recs = records(a.rows, a.players, 2)
    res = {"reps": a.reps}
    try:
        with tempfile.TemporaryDirectory() as tmp:
            G = build_global_form(tmp)
            for W in (int(w) for w in a.windows.split(",")):
                p = lib.smooth_params(25, window=W)
                spans = {k: [] for k in NAMES}
                wall, out = [], {}
                for rep in range(-1, a.reps):
                    t = h.postprocess(recs, 25, 1280, tm)
                    try:
                        if rep == -1:                                                             # on the first table: the yardstick and the comparison form
                            n, cols = len(t.rows), len(t.columns)
                            persons = [c for c, k in enumerate(t.columns) if not k["video"] and int(k["kind"]) in (lib.POST_PLAYER, lib.POST_GOALKEEPER)]
                            clist = np.ascontiguousarray(persons, np.int32)
                            ms = np.zeros(a.reps, np.float32)
                            e = np.zeros((len(persons), n), np.float64)
                            frames = np.ascontiguousarray(t.rows, np.int32)
                            rc = G.time_fit_global(t.device_values, frames.ctypes.data_as(C.c_void_p), n, clist.ctypes.data_as(C.c_void_p), len(persons), W, 2, a.reps, ms.ctypes.data_as(C.c_void_p),
                                                   e.ctypes.data_as(C.c_void_p))
                            assert rc == 0, rc
                            out["fit_global_memory"] = stats(ms)
                            import smooth_ref as SR
                            k = min(n, 3 * W + 40)
                            ref = SR.smooth(t.values[persons[0]:persons[0] + 1, :k + W], frames[:k + W], [(0, 1, 0)], 25, window=W)["e"][0][:k]
                            out["fit_global_memory"]["equal_to_contract"] = bool(np.array(ref).tobytes() == e[0, :k].tobytes())
                            res.update(rows=n, columns=cols, smoothed_columns=len(persons))
                        h.set_profiling(1)
                        t0 = time.perf_counter()
                        h._check(h.L.eagle_post_smooth_tracks(h._h, t._t, C.byref(p)), "post_smooth_tracks")
                        dt = time.perf_counter() - t0
                        times = h.kernel_times()
                        h.set_profiling(0)
                        if rep >= 0:
                            wall.append(dt * 1e3)
                            for k in NAMES:
                                spans[k].append(sum(x[1] for x in times if x[0] == k))
                    finally:
                        t.close()
                cells = res["smoothed_columns"] * res["rows"]
                for k in NAMES:
                    out[k] = stats(spans[k])
                    out[k]["GB_per_s"] = round(BYTES[k] * cells / (out[k]["ms_median"] * 1e-3) / 1e9, 1) if out[k]["ms_median"] > 0 else None
                out["wall_ms_per_call_profiled"] = stats(wall)
                res[f"window_{W}"] = out
            # the bandwidth yardstick on the same table
            t = h.postprocess(recs, 25, 1280, tm)
            try:
                kp = lib.kinematics_params(25)
                ms = []
                for rep in range(-1, a.reps):
                    h.set_profiling(1)
                    h._check(h.L.eagle_post_velocities(h._h, t._t, C.byref(kp)), "post_velocities")
                    times = h.kernel_times()
                    h.set_profiling(0)
                    if rep >= 0:
                        ms.append(sum(x[1] for x in times if x[0] == "post_velocity"))
                res["post_velocity"] = stats(ms)
                res["post_velocity"]["GB_per_s"] = round(32.0 * res["columns"] * res["rows"] / (res["post_velocity"]["ms_median"] * 1e-3) / 1e9, 1)
            finally:
                t.close()
    finally:
        h.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
