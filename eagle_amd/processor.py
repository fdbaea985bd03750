"""``Processor.process(frame) -> {players, ball, H}`` — the per-frame API BASELINE.json's north_star names.

The reference's ``eagle/processor.py`` is a whole-clip pandas post-processor and has no ``process(frame)``
(SURVEY §0); semantically this method is one iteration of the loop body of
``CoordinateModel.get_coordinates`` (eagle/models/coordinate_model.py:277-415) in the stateless configuration, with
``players`` == Coordinates["Player"] ∪ ["Goalkeeper"], ``ball`` == Coordinates["Ball"] (cm.py:369-392) and ``H`` the
3x3 homography of cm.py:355,363."""
import numpy as np

from . import lib, records
from .coordinate_model import CoordinateModel


class Processor:
    def __init__(self, model: CoordinateModel = None, **model_kwargs):
        self.model = model or CoordinateModel(**model_kwargs)
        self.team_report = None                                   # the report of the last get_team_mapping(method="cluster")

    def process(self, frame, pixel_format="bgr"):
        """frame: uint8 HWC BGR, or a decoder's 4:2:0 frame [3h/2, w] with pixel_format "nv12" / "i420".
        -> {"players": {id: {...}}, "ball": {k: {...}}, "H": 3x3 float64 | None, ...}"""
        rec = self.model.process_records(np.asarray(frame)[None], pixel_format)[0]
        return records.to_process_dict(rec)

    def process_clip(self, frames, pixel_format="bgr"):
        return [records.to_process_dict(r) for r in self.model.process_records(frames, pixel_format)]

    def get_team_mapping(self, frames, coords, pixel_format="bgr", method="colours", **params):
        """The reference post-processor's ``get_team_mapping`` (eagle/processor.py:405-464; its "pretty slow" step) for a clip and the
        ``get_coordinates`` output of that clip: colour segmentation and counting of every player crop on the GPU (eagle_amd/teams.py).
        -> {player_id: 0 | 1}.  Player ids are track ids when the model was built with ``tracker=True``.
        method="cluster": the project's own rule instead, the two clusters of the ids' kit colours over the clip (eagle_amd/kits.py; params
        min_pixels, min_crops, outlier); an id in neither team has no entry, and the report is kept as ``self.team_report``."""
        if method not in ("colours", "cluster"):
            raise ValueError(f"get_team_mapping: method {method!r} is neither 'colours' nor 'cluster'")
        if method == "colours" and params:
            raise ValueError(f"get_team_mapping: {sorted(params)} belong to method='cluster'")
        from . import kits, teams
        d = self.model._upload(frames, pixel_format)
        try:
            if method == "cluster":
                mapping, self.team_report = kits.cluster_team_mapping(self.model.handle, d, coords, n_frames=len(frames), **params)
                return mapping
            return teams.get_team_mapping(self.model.handle, d, coords, n_frames=len(frames))
        finally:
            self.model.handle.free(d)

    def ball_track(self, records, fps, cuts=None, speed=None, gap=None, reward=None, brk=None):
        """Which ball detection of every frame lies on the best physically possible path through the clip (cuts: the frames that start a new shot)
        -> (frame records, tracklets, clip totals): see eagle_amd/balltrack.py."""
        from . import balltrack as bt
        return bt.track(self.model.handle, self.model._records_of(records), fps, self.model.handle.cfg.frame_w, cuts, speed, gap, reward, brk)

    def process_data(self, frames, coords_or_records, fps, smooth=False, pixel_format="bgr", merge_ids=False, ball_track=False, cuts=None, team_method="colours",
                     team_params=None, smooth_tracks=False, smooth_params=None, stabilise=False, stabilise_params=None):
        """The reference post-processor's ``process_data`` (eagle/processor.py:73-87) for a clip and its ``get_coordinates`` output (or raw
        records): the team mapping (get_team_mapping above), then the interpolated, goalkeeper-folded, optionally smoothed table, built on the GPU
        (eagle_amd/postprocess.py).  -> (table, team_mapping); postprocess.raw_data_rows / format_data turn the table into main.py's two JSON files.
        merge_ids: stitch fragmented tracker ids (postprocess.process_data); the returned mapping then includes the teams the merged ids inherit.
        ball_track: True, or a dict of ball_track's settings (speed, gap, reward, brk): the table's ball is the tracked one (ball_track above, with
        ``cuts``) instead of the reference's choice; the track is kept as ``table.ball_track``.
        team_method: "colours" (the reference's rule) or "cluster" (get_team_mapping above, with the dict ``team_params``); the cluster report is kept
        as ``table.team_report`` (None otherwise).
        smooth_tracks: replace the pitch positions of the person columns by windowed least-squares fits right after the table is built (smooth_tracks
        below, with the dict ``smooth_params``); the report is kept as ``table.smooth_report`` (None otherwise).
        stabilise: estimate and remove each kept frame's common motion from the Player, Goalkeeper and Ball pitch positions directly after the table is
        built, before smooth_tracks (stabilise below, with the dict ``stabilise_params``); the report is kept as ``table.stabilise_report`` (None
        otherwise)."""
        from . import postprocess
        if stabilise_params and not stabilise:
            raise ValueError("process_data: stabilise_params without stabilise")
        coords = coords_or_records
        if not isinstance(coords, dict):
            coords = {i: records.to_reference_dict(r, i, fps) for i, r in enumerate(np.ascontiguousarray(coords_or_records, lib.RESULT_DTYPE).reshape(-1))}
        recs = self.model._records_of(coords_or_records)
        if team_method not in ("colours", "cluster") or (team_method == "colours" and team_params):
            raise ValueError(f"process_data: team_method {team_method!r} with team_params {team_params!r}")
        self.team_report = None
        if team_method == "cluster":
            team_mapping = self.get_team_mapping(frames, coords, pixel_format, method="cluster", **(team_params or {})) if len(recs) else {}
        else:
            team_mapping = self.get_team_mapping(frames, coords, pixel_format) if len(recs) else {}
        track = self.ball_track(recs, fps, cuts, **(ball_track if isinstance(ball_track, dict) else {})) if ball_track else None
        table = postprocess.process_data(self.model.handle, recs, fps, self.model.handle.cfg.frame_w, team_mapping, smooth=smooth, merge_ids=merge_ids,
                                         ball_det=None if track is None else track[0]["det"])
        table.ball_track = track
        table.team_report = self.team_report
        table.stabilise_report = self.stabilise(table, fps, **(stabilise_params or {})) if stabilise else None
        if smooth_params and not smooth_tracks:
            raise ValueError("process_data: smooth_params without smooth_tracks")
        table.smooth_report = self.smooth_tracks(table, fps, **(smooth_params or {})) if smooth_tracks else None
        return table, table.team_mapping if merge_ids else team_mapping

    def shots(self, frames, fps, pixel_format="bgr", **overrides):
        """The cuts, transitions, flashes and shots of a clip, and which shots look at the pitch: see eagle_amd/shots.py."""
        from . import shots as sh
        return sh.find_shots(self.model.handle, frames, fps, pixel_format, **overrides)

    def topview(self, frames, coords_or_records, carry=False, out_format="bgr", **kw):
        """The frames warped onto the pitch plane with their homographies: see CoordinateModel.topview and eagle_amd/topview.py."""
        return self.model.topview(frames, coords_or_records, carry, out_format, **kw)

    def refine_lines(self, frames, coords_or_records, fps=None, **params):
        """Each frame's homography refined on its painted lines, the accepted frames re-projected -> (coordinates, report): see
        CoordinateModel.refine_lines and eagle_amd/linefit.py.  Run it directly after get_coordinates; process_data takes the new dict."""
        return self.model.refine_lines(frames, coords_or_records, fps, **params)

    def annotate(self, frames, coords_or_records, team_mapping=None, pixel_format="bgr", out_format="bgr", table=None):
        """The annotated frames of a clip (the reference's annotated video, main.py:43-81), drawn on the GPU: see CoordinateModel.annotate.
        ``table``: draw the processed table (process_data above) instead of the raw records."""
        return self.model.annotate(frames, coords_or_records, team_mapping, pixel_format, out_format, table=table)

    def minimap(self, table, scale=8, margin=None, voronoi=False, footprint=True, pixel_format="bgr", rows=None, control=None, trails=None, passes=False, owner=False,
                trail_params=None, hulls=None):
        """The minimap pictures of a processed table (process_data above), drawn on the GPU: see eagle_amd/minimap.py.  trails (table columns), passes and
        owner add the paths, the pass arrows and the owner's ring (the last two after possession below); hulls (a half width in pixels) the two teams'
        convex hulls (after shape below)."""
        from . import minimap as mm
        return mm.minimap(self.model.handle, table, scale, margin, voronoi, footprint, pixel_format, rows, control=control, trails=trails, passes=passes, owner=owner,
                          trail_params=trail_params, hulls=hulls)

    def trajectory(self, table, cols, rows=None, scale=8, margin=None, half_width=1, max_gap=25):
        """The paths of table columns over a row window as one still picture of the pitch (BGR): see eagle_amd/minimap.py trajectory_picture."""
        from . import minimap as mm
        return mm.trajectory_picture(self.model.handle, table, cols, rows, scale, margin, half_width, max_gap)

    def pass_pictures(self, table, scale=8, margin=None, half_width=1, kinds=(0,)):
        """One still picture (BGR) per possession event of the given kinds (default: passes) at its release row, after possession below
        -> [(event index, picture)]."""
        from . import minimap as mm
        events = self.model.handle.events(table)
        return [(k, mm.pass_picture(self.model.handle, table, k, scale, margin, half_width)) for k, e in enumerate(events) if int(e["kind"]) in kinds]

    def stabilise(self, table, fps, **kw):
        """Estimate and remove each kept frame's common motion (the error of its homography) from a processed table that carries no derived result yet
        (window, degree, model, min_voters, iterations, trim_k, floor, min_spread, max_gain, jump): see eagle_amd/stabilise.py."""
        from . import stabilise as st
        return st.stabilise(self.model.handle, table, fps, **kw)

    def smooth_tracks(self, table, fps, **kw):
        """Smooth the player paths of a processed table that carries no derived result yet (window, degree, outlier_k, outlier_floor, ball_window,
        max_gap, speed_cap): positions, velocities and accelerations from windowed fits, rejected samples and suspect rows: see eagle_amd/smooth.py."""
        from . import smooth as sm
        return sm.smooth_tracks(self.model.handle, table, fps, **kw)

    def ball_flights(self, table, fps, cuts=None, **params):
        """The ball's path of a processed table cut into straight flights of constant speed, the knots between them, the kicks among the knots and the
        flights that would cross a goal line between the posts (max_gap, max_rows, noise, penalty, spike, kick_dv, radius, still_speed, shot_speed,
        shot_range, shot_margin; cuts: the frames that start a new shot).  The table's positions are not changed: see eagle_amd/flights.py."""
        from . import flights as fl
        return fl.ball_flights(self.model.handle, table, fps, cuts, **params)

    def goal_view(self, table, grid=False, **params):
        """How much of the goal mouth every attacker, the ball and (grid=True) every cell of the pitch sees past the other team on a processed table
        (direction, group, cells_per_metre, radius, keeper_radius, min_depth, max_range, chance).  Nothing in the table changes: see eagle_amd/goalview.py."""
        from . import goalview as gv
        return gv.goal_view(self.model.handle, table, grid, **params)

    def kinematics(self, table, fps, max_gap=None, speed_cap=12.0, keep=False):
        """Velocities of a processed table (computed on the GPU, kept with the table; keep=True: the ones it carries, as after smooth_tracks) plus per
        id distance covered and top speed: see eagle_amd/control.py."""
        from . import control as ct
        return ct.kinematics(self.model.handle, table, fps, max_gap, speed_cap, keep)

    def control(self, table, cells_per_metre=1, t_react=0.7, v_max=5.0, beta=4.0, rows=None):
        """The pitch-control grids of a processed table with velocities (kinematics above) and team 0's area share per row: see eagle_amd/control.py."""
        from . import control as ct
        return ct.control(self.model.handle, table, cells_per_metre, t_react, v_max, beta, rows)

    def possession(self, table, fps, radius=2.0, min_hold=2, max_gap=None):
        """Who has the ball in each kept frame of a processed table, the passes and turnovers, and what they add up to: see eagle_amd/possession.py."""
        from . import possession as po
        return po.possession(self.model.handle, table, fps, radius, min_hold, max_gap)

    def occupancy(self, table, fps, cells_per_metre=1, sigma=2.0, max_gap=None):
        """Where every player, every team and the ball of a processed table spent their time, as smoothed seconds per pitch cell: see eagle_amd/occupancy.py."""
        from . import occupancy as oc
        return oc.occupancy(self.model.handle, table, fps, cells_per_metre, sigma, max_gap)

    def physical(self, table, fps, max_gap=None, zone_edges=(2.0, 4.0, 5.5, 7.0), effort_speed=(5.5, 7.0), accel=2.0, min_frames=None):
        """The physical report of a processed table with velocities (kinematics above): per id the distance and the seconds per speed zone, the top speed,
        and the high-speed runs, sprints, accelerations and decelerations: see eagle_amd/physical.py."""
        from . import physical as ph
        return ph.physical(self.model.handle, table, fps, max_gap, zone_edges, effort_speed, accel, min_frames)

    def pass_options(self, table, cells_per_metre=1, samples=16, t_react=0.7, v_max=5.0, beta=4.0, v_ball=15.0, rows=None, grids=True):
        """Where the owner of the ball could play in each kept frame of a processed table with velocities (kinematics above) and possession: a grid per
        row, a figure per teammate, the best of them, and how every pass that was played compares: see eagle_amd/options.py."""
        from . import options as op
        return op.pass_options(self.model.handle, table, cells_per_metre, samples, t_react, v_max, beta, v_ball, rows, grids)

    def shape(self, table):
        """Each team as a body in every kept frame of a processed table (centroid, length, width, hull area, stretch, lines, hull) and what that adds up
        to over the clip: see eagle_amd/shape.py."""
        from . import shape as sh
        return sh.shape(self.model.handle, table)

    def roles(self, table, roles=10, min_present=8, iterations=8, lines=3, per_row=False):
        """What the players of a processed table DO, whatever ids the tracker gave them: each team's mean formation from an exact per-frame assignment of
        its players to roles, its lines and label (4-4-2), the rows per id and role, every change of role and the stints per role: see eagle_amd/roles.py."""
        from . import roles as ro
        return ro.roles(self.model.handle, table, roles, min_present, iterations, lines, per_row)

    def space(self, table, cells_per_metre=1, goalkeepers=True, radius=3.0, per_row=False):
        """How much room every player of a processed table has: the exact area of the pitch nearer to him than to anybody else (by thirds), his nearest
        opponent, the opponents within ``radius`` metres and his usual marker, per id and per team; with a possession result on the table also per owner
        and pass: see eagle_amd/space.py."""
        from . import space as sp
        return sp.space(self.model.handle, table, cells_per_metre, goalkeepers, radius, per_row)

    def offside(self, table, direction="auto", tolerance=0.5, assume_keeper=True, per_row=False):
        """Where the offside line stood for each team in every kept frame of a processed table, who was beyond it and by how much, how often per id; with
        a possession result on the table also, per pass, whether the receiver was onside, close or offside when the ball was played: see
        eagle_amd/offside.py."""
        from . import offside as of
        return of.offside(self.model.handle, table, direction, tolerance, assume_keeper, per_row)

    def offside_view(self, frames, coords_or_records, table, team="possession", width=0.25, zone=True, rings=True, keyed=True, pixel_format="bgr", out_format="bgr"):
        """The annotated video of a processed table with the offside line lying on the grass under the players, after offside above (and possession for
        team="possession") -> (pictures, the dict offside_view.json holds): see eagle_amd/ground.py."""
        from . import ground as gr
        return gr.offside_view(self.model, frames, coords_or_records, table, team, width, zone, rings, keyed, pixel_format, out_format)

    def offside_stills(self, frames, coords_or_records, table, width=0.25, zone=True, keyed=True, pixel_format="bgr"):
        """One picture per pass with an offside verdict, after possession and offside above: the frame in which the ball was played with the receiver's
        team's line and a ring under the receiver in the colour of the verdict -> [(event index, picture, dict)]: see eagle_amd/ground.py."""
        from . import ground as gr
        return gr.offside_stills(self.model, frames, coords_or_records, table, width, zone, keyed, pixel_format)
