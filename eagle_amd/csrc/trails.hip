// K25 — what the minimap's trail, pass-arrow and owner layers need in front of the draw kernel (minimap.hip draws them; tests/trails_ref.py is the written
// definition of every output byte).  Three small launches, none per pixel:
//   trail_points_kernel  one thread per (selected column, row) of the call's row span: the cell is quantised ONCE (the draw kernel would otherwise redo it
//                        for every picture the cell shows on, window times) to an int2 in [column][row] order, MM_ABSENT for an absent cell: the table is
//                        [column][row] too, so a wave's loads and stores are contiguous along rows.  link[row] = the frame step into the row is at
//                        most max_gap.  No per-picture segment list exists: consecutive pictures share all but one of their segments, the draw kernel
//                        indexes this array by (column, row - age).
//   trail_events_kernel  one thread per possession event: the two ball cells quantised, the three vertices of the arrow head (the float64 sqrt and
//                        divisions happen here, once per event, never per pixel), colour by kind: 3 x int4 per event.
//   trail_marks_kernel   the trajectory still's draw list: one thread per selected column walks the window's points for the first and the last present
//                        one (a still: the walk is n loads, once).
#include "trails.h"

namespace eagle {

__global__ __launch_bounds__(256) void trail_points_kernel(const double2* values, int rows, const MmCol* sel, const int32_t* frames, int prow0, int prows, int max_gap,
                                                           int scale, int margin, int2* pts, uint8_t* link)
{
    const int i = blockIdx.x * 256 + threadIdx.x, ci = blockIdx.y;
    if (i >= prows) return;
    const double K = (double)(16 * scale);
    const int ox = 16 * margin, oy = 16 * margin + 16 * 68 * scale;
    int qx = 0, qy = 0;
    const bool ok = mm_quantise(values[(size_t)sel[ci].col * rows + (size_t)(prow0 + i)], K, ox, oy, qx, qy);
    pts[(size_t)ci * prows + i] = ok ? make_int2(qx, qy) : make_int2(MM_ABSENT, 0);
    if (ci == 0) link[i] = i > 0 && (long long)frames[i] - (long long)frames[i - 1] <= (long long)max_gap;
}

__global__ __launch_bounds__(256) void trail_events_kernel(const EaglePossessionEvent* events, int nev, int scale, int margin, int half_width, int4* out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nev) return;
    const EaglePossessionEvent ev = events[e];
    const double K = (double)(16 * scale);
    const int ox = 16 * margin, oy = 16 * margin + 16 * 68 * scale;
    int ax = 0, ay = 0, bx = 0, by = 0, h1x = 0, h1y = 0, h2x = 0, h2y = 0;
    const bool oka = mm_quantise(make_double2(ev.x0, ev.y0), K, ox, oy, ax, ay), okb = mm_quantise(make_double2(ev.x1, ev.y1), K, ox, oy, bx, by);
    const bool ok = oka && okb;
    uint32_t flags = ev.kind == EAGLE_EVENT_PASS ? 0xffffffu : ev.kind == EAGLE_EVENT_TURNOVER ? 0xffff00u : 0xa0a0a0u;      // B | G << 8 | R << 16
    if (ok) {
        flags |= MM_EV_OK;
        const long long dx = bx - ax, dy = by - ay, L2 = dx * dx + dy * dy;
        if (L2) {
            flags |= MM_EV_HEAD;
            const double s = sqrt((double)L2), ux = (double)dx / s, uy = (double)dy / s;
            const double hl = (double)(64 * half_width), hh = (double)(32 * half_width);
            const double cx = (double)bx - hl * ux, cy = (double)by - hl * uy;
            h1x = (int)floor((cx - hh * uy) + 0.5); h1y = (int)floor((cy + hh * ux) + 0.5);
            h2x = (int)floor((cx + hh * uy) + 0.5); h2y = (int)floor((cy - hh * ux) + 0.5);
        }
    }
    out[3 * (size_t)e] = make_int4(ax, ay, bx, by);
    out[3 * (size_t)e + 1] = make_int4(h1x, h1y, h2x, h2y);
    out[3 * (size_t)e + 2] = make_int4((int)flags, ev.release_row, ev.receive_row, 0);
}

__global__ __launch_bounds__(256) void trail_marks_kernel(const int2* pts, const MmCol* sel, int nsel, int prows, int4* list)
{
    const int ci = blockIdx.x * 256 + threadIdx.x;
    if (ci == 0) {
        list[0] = make_int4(2 * nsel, 0, 0, 0);        // (no footprint)
        list[1] = list[2] = make_int4(0, 0, 0, 0);
    }
    if (ci >= nsel) return;
    const int2* P = pts + (size_t)ci * prows;
    int first = -1, last = -1;
    for (int i = 0; i < prows; ++i)
        if (P[i].x != MM_ABSENT) { if (first < 0) first = i; last = i; }
    const uint32_t color = sel[ci].kc & MM_WHITE;
    const int2 a = first >= 0 ? P[first] : make_int2(0, 0), b = first >= 0 ? P[last] : make_int2(0, 0);
    const uint32_t ring = first >= 0 ? (uint32_t)EAGLE_POST_BALL : (uint32_t)MM_KIND_SKIP, disc = first >= 0 ? (uint32_t)EAGLE_POST_PLAYER : (uint32_t)MM_KIND_SKIP;
    list[MM_HEAD + 2 * ci] = make_int4(a.x, a.y, (int)(color | ring << MM_KIND_SHIFT), 0);
    list[MM_HEAD + 2 * ci + 1] = make_int4(b.x, b.y, (int)(color | disc << MM_KIND_SHIFT), 0);
}

void trail_points_launch(const double2* values, int rows, const MmCol* sel, int nsel, const int32_t* frames, int prow0, int prows, int max_gap, int scale, int margin,
                         int2* pts, uint8_t* link, hipStream_t s)
{
    if (nsel <= 0 || prows <= 0) return;
    hipLaunchKernelGGL(trail_points_kernel, dim3((prows + 255) / 256, nsel), dim3(256), 0, s, values, rows, sel, frames, prow0, prows, max_gap, scale, margin, pts, link);
    HIP_CHECK(hipGetLastError());
}

void trail_events_launch(const EaglePossessionEvent* events, int nev, int scale, int margin, int half_width, int4* out, hipStream_t s)
{
    if (nev <= 0) return;
    hipLaunchKernelGGL(trail_events_kernel, dim3((nev + 255) / 256), dim3(256), 0, s, events, nev, scale, margin, half_width, out);
    HIP_CHECK(hipGetLastError());
}

void trail_marks_launch(const int2* pts, const MmCol* sel, int nsel, int prows, int4* list, hipStream_t s)
{
    hipLaunchKernelGGL(trail_marks_kernel, dim3(std::max(1, (nsel + 255) / 256)), dim3(256), 0, s, pts, sel, nsel, prows, list);
    HIP_CHECK(hipGetLastError());
}

}  // namespace eagle
