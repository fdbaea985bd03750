#!/usr/bin/env python3
"""Cost of the line-registration kernels (include/eagle.h, eagle_linefit_device_frames; csrc/linefit.hip): one JSON line.

    python tools/linefit_rate.py [--frames 200] [--distinct 10] [--reps 5]

A clip of 720 x 1280 synthetic frames resident in HBM (--distinct generated frames, repeated), each under its true homography disturbed by about 2 m
and with its players' boxes, is put through eagle_linefit_device_frames with the default parameters.  The kernels are timed by the HIP events of the
profiling mode directly around their launches: --reps calls after a warm-up call, reported as the median with the minimum and the maximum; the
accumulate kernel runs rounds + 2 times per call and is reported per launch.  The mask kernel's yardstick is a device-to-device copy of the clip's bytes
(hipMemcpyAsync, HIP events, the same run): `times_the_copy`.  `whole_call` is the host's wall time of the call, uploads of the tables and the copy
back of the results included.

One structural A/B: the library's accumulate form (per-lane partial sums, a wave butterfly, one u64 atomic per wave and sum) against one atomic per
inlier and sum.  The second form lives in this tool only: both are compiled with hipcc when the tool runs, from csrc/linefit_accumulate.inc, so they
differ in the reduction alone, and run interleaved on the masks and matrices of the same clip between HIP events; their sums must be the same bytes."""
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

from eagle_amd import lib, synth  # noqa: E402

FH, FW = 720, 1280
DISTURB = np.array([[1.012, .006, .9], [-.004, .99, -.6], [1e-4, -2e-4, 1]])
NAMES = ("linefit_mask", "linefit_accumulate", "linefit_solve", "linefit_decide")

BOTH_FORMS = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <vector>
#include "eagle.h"
#include "linefit_accumulate.inc"
// masks u32 [n][h][wpr] and G [n][9] (host); reps timed launches of each form, interleaved, after one warm-up each -> ms_wave[reps], ms_inlier[reps];
// *inliers: the inlier count over the clip; *equal: the two forms' sums are the same bytes
extern "C" int time_accumulate(const uint32_t* masks, const double* G, int n, int h, int w, long long rq, int reps, float* ms_wave, float* ms_inlier, long long* inliers, int* equal)
{
    using namespace eagle;
    const int wpr = (w + 31) / 32;
    const size_t words = (size_t)n * h * wpr, sum_bytes = (size_t)n * LF_NSUM * 8;
    std::vector<LfFrame> tab(n);
    for (int i = 0; i < n; ++i) { std::memcpy(tab[i].g, G + 9 * (size_t)i, 72); tab[i].ok = 1; tab[i].flipped = 0; }
    uint32_t* d_mask = nullptr;
    LfFrame* d_tab = nullptr;
    lf_u64* d_sums[2] = {nullptr, nullptr};
    hipEvent_t e0, e1;
    if (hipMalloc((void**)&d_mask, words * 4) || hipMalloc((void**)&d_tab, n * sizeof(LfFrame)) || hipMalloc((void**)&d_sums[0], sum_bytes) || hipMalloc((void**)&d_sums[1], sum_bytes)) return 1;
    if (hipMemcpy(d_mask, masks, words * 4, hipMemcpyHostToDevice) || hipMemcpy(d_tab, tab.data(), n * sizeof(LfFrame), hipMemcpyHostToDevice) || hipEventCreate(&e0) || hipEventCreate(&e1)) return 2;
    LfArgs a{};
    a.tab = d_tab; a.mask = d_mask; a.n = n; a.h = h; a.w = w; a.wpr = wpr; a.slot = 0; a.use_orig = 1; a.rq2 = rq * rq;
    const dim3 grid((unsigned)(((size_t)h * wpr + 255) / 256), (unsigned)n);
    for (int i = -1; i < reps; ++i)
        for (int form = 0; form < 2; ++form) {
            a.sums = d_sums[form];
            if (hipMemset(a.sums, 0, sum_bytes)) return 3;
            hipEventRecord(e0, nullptr);
            if (form == 0) hipLaunchKernelGGL(linefit_accumulate_kernel<false>, grid, dim3(256), 0, nullptr, a);
            else hipLaunchKernelGGL(linefit_accumulate_kernel<true>, grid, dim3(256), 0, nullptr, a);
            hipEventRecord(e1, nullptr);
            if (hipEventSynchronize(e1) || hipGetLastError()) return 4;
            if (i >= 0) hipEventElapsedTime((form == 0 ? ms_wave : ms_inlier) + i, e0, e1);
        }
    std::vector<lf_u64> s0((size_t)n * LF_NSUM), s1((size_t)n * LF_NSUM);
    int rc = 0;
    if (hipMemcpy(s0.data(), d_sums[0], sum_bytes, hipMemcpyDeviceToHost) || hipMemcpy(s1.data(), d_sums[1], sum_bytes, hipMemcpyDeviceToHost)) rc = 5;
    *equal = rc == 0 && std::memcmp(s0.data(), s1.data(), sum_bytes) == 0;
    *inliers = 0;
    for (int i = 0; i < n; ++i) *inliers += (long long)s0[(size_t)i * LF_NSUM + 44];
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(d_mask); hipFree(d_tab); hipFree(d_sums[0]); hipFree(d_sums[1]);
    return rc;
}
"""


def stats(ms):
    ms = np.sort(np.asarray(ms, np.float64))
    return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms[0]), 4), "ms_max": round(float(ms[-1]), 4)}


def build_both_forms(tmp):
    src, so = os.path.join(tmp, "linefit_forms.hip"), os.path.join(tmp, "linefit_forms.so")
    with open(src, "w") as f:
        f.write(BOTH_FORMS)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-slp-vectorize", "-std=c++17", "-Wno-unused-result",
                           "-Wno-unused-value", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "eagle_amd", "csrc"), "-shared", "-fPIC", src, "-o", so])
    L = C.CDLL(so)
    vp, i32 = C.c_void_p, C.c_int
    L.time_accumulate.argtypes = [vp, vp, i32, i32, i32, C.c_longlong, i32, vp, vp, vp, vp]
    return L


def copy_ms(dst, src, nbytes, reps):
    """a device-to-device copy of nbytes on the null stream between HIP events"""
    hip = C.CDLL("libamdhip64.so")
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    ms = []
    for k in range(reps + 1):
        t = C.c_float(0)
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemcpyAsync(dst, src, C.c_size_t(nbytes), 3, None) == 0          # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
        if k:
            ms.append(t.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return stats(ms)


def clip(n, distinct):
    d = min(distinct, n)
    views = [(3, 20 * t) for t in range(d)]
    frames = np.stack([synth.frame(s, t) for s, t in views])
    Hs = np.stack([(DISTURB @ np.linalg.inv(synth.camera(s, t))).reshape(9) for s, t in views])
    recs = np.zeros(d, lib.RESULT_DTYPE)
    for i, (s, t) in enumerate(views):
        bx = np.array([b[1:] for b in synth.player_boxes(s, t)], np.float32)
        recs[i]["n_det"] = len(bx)
        for k, name in enumerate(("x1", "y1", "x2", "y2")):
            recs[i]["det"][name][:len(bx)] = bx[:, k]
    idx = np.arange(n) % d
    return frames[idx], Hs[idx], recs[idx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--distinct", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = a.frames
    frames, Hs, recs = clip(n, a.distinct)
    valid = np.ones(n, np.uint8)
    p = lib.linefit_params()
    launches = {"linefit_mask": 1, "linefit_accumulate": p.rounds + 2, "linefit_solve": p.rounds, "linefit_decide": 1}
    h = lib.Handle(batch=1, frame_h=FH, frame_w=FW)
    clip_bytes = n * FH * FW * 3
    res = {"frames": n, "size": [FW, FH], "reps": a.reps, "clip_bytes": clip_bytes, "rounds": int(p.rounds)}
    d = h.upload(frames)
    d_out = h.device_alloc(clip_bytes)
    try:
        res["copy"] = copy_ms(d_out, d, clip_bytes, a.reps)
        out, fr, masks = h.linefit_device(d, n, Hs, valid, recs, p, masks=True)          # (warm-up; its masks feed the A/B)
        res["line_pixels_per_frame"] = round(float(fr["n_line"].mean()), 1)
        res["status"] = {name: int((fr["status"] == i).sum()) for i, name in enumerate(lib.LINEFIT_STATUS)}
        per, wall = {k: [] for k in NAMES}, []
        for _ in range(a.reps):
            h.set_profiling(1)
            t0 = time.perf_counter()
            h.linefit_device(d, n, Hs, valid, recs, p)
            wall.append((time.perf_counter() - t0) * 1e3)
            rows = h.kernel_times()
            h.set_profiling(0)
            for k in NAMES:
                per[k].append(sum(x[1] for x in rows if x[0] == k) / launches[k])
        for k in NAMES:
            res[k] = dict(stats(per[k]), launches_per_call=launches[k])
        res["linefit_mask"]["times_the_copy"] = round(res["linefit_mask"]["ms_median"] / res["copy"]["ms_median"], 3)
        res["kernels_per_call_ms"] = round(sum(res[k]["ms_median"] * launches[k] for k in NAMES), 4)
        res["whole_call"] = stats(wall)
        res["whole_call"]["us_per_frame"] = round(res["whole_call"]["ms_median"] * 1e3 / n, 2)
    finally:
        h.free(d)
        h.free(d_out)
        h.close()
    with tempfile.TemporaryDirectory() as tmp:
        G = build_both_forms(tmp)
        sb = (Hs[:, 6] * ((FW - 1) / 2) + Hs[:, 7] * (FH - 1)) + Hs[:, 8]
        Gs = np.ascontiguousarray(Hs * np.where(sb > 0, 1.0, -1.0)[:, None])
        ms_w, ms_i = np.zeros(a.reps, np.float32), np.zeros(a.reps, np.float32)
        inl, eq = C.c_longlong(0), C.c_int(0)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)
        rc = G.time_accumulate(ptr(np.ascontiguousarray(masks)), ptr(Gs), n, FH, FW, 2560, a.reps, ptr(ms_w), ptr(ms_i), C.byref(inl), C.byref(eq))
        if rc:
            raise SystemExit(f"time_accumulate failed ({rc})")
        res["accumulate_ab"] = {"radius_q": 2560, "inliers_per_frame": round(inl.value / n, 1), "sums_equal": bool(eq.value), "per_wave": stats(ms_w), "per_inlier": stats(ms_i),
                                "per_inlier_over_per_wave": round(float(np.median(ms_i) / np.median(ms_w)), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
