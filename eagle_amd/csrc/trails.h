// What the minimap's draw kernel (minimap.hip) and the kernels that prepare its trail, pass-arrow and owner layers (trails.hip, K25) share.
#pragma once
#include "runtime.h"

namespace eagle {

static constexpr double MM_DOMAIN = 1024.0;
static constexpr int MM_HEAD = 3;                      // header slots of a row's list: {count, footprint ok}, {BL, TL}, {TR, BR}
static constexpr int MM_KIND_SHIFT = 24, MM_SITE_BIT = 1 << 28, MM_OWNER_BIT = 1 << 29, MM_DIM_BIT = 1 << 30;
static constexpr int MM_KIND_SKIP = 15;                // a list entry that draws nothing (a still's column without a present cell)
static constexpr int MM_ABSENT = (int)0x80000000;      // trail points: x of an absent cell
static constexpr int MM_EV_OK = 1 << 24, MM_EV_HEAD = 1 << 25;
static constexpr uint32_t MM_WHITE = 0xffffffu, MM_NONE = 0xffffffffu;

struct MmCol { int32_t col; uint32_t kc; };            // a drawable table column: B | G << 8 | R << 16 | kind << 24 | site << 28

// the layers of K25, handed to the layered instantiation of the draw kernel beside MinimapArgs (the plain instantiation never sees it)
struct MmLayerArgs {
    const int2* pts;             // trails: [nsel][prows] quantised cells of the selected columns over rows prow0 .. prow0 + prows - 1 (x == MM_ABSENT: absent)
    const uint8_t* link;         // [prows]: frames[row] - frames[row - 1] <= max_gap
    const MmCol* sel;            // [nsel] the selected columns that have a colour, in selection order
    const int4* ev;              // pass arrows: [nev][3] = {A, B}, {H1, H2}, {colour | MM_EV_*, release_row, receive_row, 0} (nullptr: layer off)
    const int2* ev_range;        // [pictures of the call]: the events [first, last) that can show on picture (row - range_row0)
    const int32_t* owner;        // [rows] of the table (nullptr: layer off)
    int nsel, prow0, prows;      // nsel == 0: no trail layer
    int window, dim_floor, hw16, pass_hold;
    int jlo;                     // >= 0: the trajectory still (segments from this j on, whatever the window); -1: the video's rule
    int range_row0, only;        // only != 0: the pass still (the one event of the range shows whatever its rows are)
    int dim, pass_from, pass_to; // dim != 0: person discs of other columns than these two are blended at a = 64
    int r16o;                    // 16 x the owner ring's outer radius
    const int4* hull_edges;      // K26 hulls: [pictures of the call][2][EAGLE_SHAPE_HULL_CAP] = {A, B} (x == MM_ABSENT: no edge); nullptr: layer off (shape.hip)
    int hull_hw16;               // 16 x the hull layer's half width
};

__device__ __forceinline__ bool mm_quantise(double2 v, double K, int ox, int oy, int& qx, int& qy)
{
    if (!(fabs(v.x) <= MM_DOMAIN) || !(fabs(v.y) <= MM_DOMAIN)) return false;          // NaN, +-inf and the far field
    qx = ox + (int)floor(v.x * K + 0.5);
    qy = oy - (int)floor(v.y * K + 0.5);
    return true;
}

// trails.hip: launches on stream s, no synchronisation
// rows prow0 .. prow0 + prows - 1 of the selected columns -> pts, link (frames: the frame numbers of those rows, in HBM)
void trail_points_launch(const double2* values, int rows, const MmCol* sel, int nsel, const int32_t* frames, int prow0, int prows, int max_gap, int scale, int margin,
                         int2* pts, uint8_t* link, hipStream_t s);
// events (in HBM) -> 3 x int4 per event
void trail_events_launch(const EaglePossessionEvent* events, int nev, int scale, int margin, int half_width, int4* out, hipStream_t s);
// the one draw list of a trajectory still: per selected column a ring entry at its first present point and a disc entry at its last
void trail_marks_launch(const int2* pts, const MmCol* sel, int nsel, int prows, int4* list, hipStream_t s);

}  // namespace eagle
