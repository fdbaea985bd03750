"""The minimap: a processed clip table as a top-down video of the pitch — per kept frame the camera's footprint, the players in team colours and
the ball, and on request the Voronoi picture of the areas each team controls (what the reference's ``examples/minimap.py`` and
``examples/voronoi.py`` plot through matplotlib, frame by frame).

The pictures are drawn on the GPU from the table where the post-processor left it in HBM (include/eagle.h, eagle_minimap_*; csrc/minimap.hip); this
module only passes arrays through.  The rasterisation is the library's own (tests/minimap_ref.py defines every pixel; parity with matplotlib or
mplsoccer is not claimed).  ``annotate.write_y4m`` writes the I420 result as a video."""
from . import lib


def minimap(handle, table, scale=8, margin=None, voronoi=False, footprint=True, pixel_format="bgr", rows=None, player_radius=0, ball_radius=0, control=None,
            trails=None, passes=False, owner=False, trail_params=None, hulls=None):
    """A lib.PostTable of ``handle`` -> its minimap pictures on the host: uint8 [n, h, w, 3] ("bgr") or [n, 3h/2, w] ("nv12" / "i420"), one per table
    row, with w = 105 scale + 2 margin and h = 68 scale + 2 margin (margin None: two metres' worth of pixels).  ``rows``: (first row, count) to draw
    a window of the table.  voronoi needs a table with a team mapping.  ``control``: a lib.control_params(...) draws the pitch-control layer in
    Voronoi's place (not both); the table needs velocities (Handle.velocities) and a team mapping.  ``trails``: table columns whose paths over the last
    rows are drawn; ``passes`` / ``owner``: an arrow per possession event and a ring round the ball's owner (Handle.possession comes first);
    ``trail_params``: a lib.trail_params(...) for the three (None: its defaults).  ``hulls``: half the line width in pixels (1 .. 8) of the two teams'
    convex hulls, drawn under the trails (Handle.team_shape comes first; None: no hulls)."""
    layers = (lib.MM_TRAILS if trails is not None and len(trails) else 0) | (lib.MM_PASSES if passes else 0) | (lib.MM_OWNER if owner else 0)
    params = lib.minimap_params(scale, margin, voronoi, footprint, player_radius, ball_radius, control is not None, layers | (lib.MM_HULLS if hulls is not None else 0))
    if hulls is not None:
        handle.set_hulls(table, hulls)
    if layers:
        handle.minimap_set_trails(table, trail_params or lib.trail_params(), () if trails is None else trails)
    if control is not None:
        handle.minimap_set_control(table, control)
    row0, n = (0, len(table.rows)) if rows is None else (int(rows[0]), int(rows[1]))
    return handle.minimap(table, params, row0, n, pixel_format)


def size(scale=8, margin=None):
    """(w, h) of the pictures minimap() gives for these parameters"""
    return lib.minimap_size(lib.minimap_params(scale, margin))


def trajectory_picture(handle, table, cols, rows=None, scale=8, margin=None, half_width=1, max_gap=25, path=None):
    """The paths of table columns ``cols`` over ``rows`` = (first row, count) (None: the whole table) as a still picture, BGR uint8 [h, w, 3] (what the
    reference's ``examples/trajectory.py`` plots); ``path``: also written there as a PPM."""
    row0, n = (0, len(table.rows)) if rows is None else (int(rows[0]), int(rows[1]))
    pic = handle.trajectory_picture(table, cols, row0, n, scale, margin, half_width, max_gap)
    if path is not None:
        from .occupancy import write_ppm
        write_ppm(path, pic)
    return pic


def pass_picture(handle, table, event, scale=8, margin=None, half_width=1, path=None):
    """Event ``event`` of the table's possession result at its release row (what the reference's ``examples/pass.py`` plots): BGR uint8 [h, w, 3]."""
    pic = handle.pass_picture(table, event, scale, margin, half_width)
    if path is not None:
        from .occupancy import write_ppm
        write_ppm(path, pic)
    return pic
