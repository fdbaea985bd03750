"""The minimap: a processed clip table as a top-down video of the pitch — per kept frame the camera's footprint, the players in team colours and
the ball, and on request the Voronoi picture of the areas each team controls (what the reference's ``examples/minimap.py`` and
``examples/voronoi.py`` plot through matplotlib, frame by frame).

The pictures are drawn on the GPU from the table where the post-processor left it in HBM (include/eagle.h, eagle_minimap_*; csrc/minimap.hip); this
module only passes arrays through.  The rasterisation is the library's own (tests/minimap_ref.py defines every pixel; parity with matplotlib or
mplsoccer is not claimed).  ``annotate.write_y4m`` writes the I420 result as a video."""
from . import lib


def minimap(handle, table, scale=8, margin=None, voronoi=False, footprint=True, pixel_format="bgr", rows=None, player_radius=0, ball_radius=0, control=None):
    """A lib.PostTable of ``handle`` -> its minimap pictures on the host: uint8 [n, h, w, 3] ("bgr") or [n, 3h/2, w] ("nv12" / "i420"), one per table
    row, with w = 105 scale + 2 margin and h = 68 scale + 2 margin (margin None: two metres' worth of pixels).  ``rows``: (first row, count) to draw
    a window of the table.  voronoi needs a table with a team mapping.  ``control``: a lib.control_params(...) draws the pitch-control layer in
    Voronoi's place (not both); the table needs velocities (Handle.velocities) and a team mapping."""
    params = lib.minimap_params(scale, margin, voronoi, footprint, player_radius, ball_radius, control is not None)
    if control is not None:
        handle.minimap_set_control(table, control)
    row0, n = (0, len(table.rows)) if rows is None else (int(rows[0]), int(rows[1]))
    return handle.minimap(table, params, row0, n, pixel_format)


def size(scale=8, margin=None):
    """(w, h) of the pictures minimap() gives for these parameters"""
    return lib.minimap_size(lib.minimap_params(scale, margin))
