"""Minimal command line for the plumbing configuration (BASELINE.json configs[0]; SURVEY §2 row 16): run a clip through
the GPU path and write ``raw_coordinates.json`` exactly the way the reference's ``main.py:26-30`` does
(``json.dump(coordinates, f, default=float)`` of ``CoordinateModel.get_coordinates``; schema ``docs/data.md:20-41``).

    python -m eagle_amd.cli --frames 10 --fps 5 --out output/synthetic          # synthetic clip (no video decode here)
    python -m eagle_amd.cli --clip frames.npy --fps 25 --out output/myclip       # uint8 [n,h,w,3] BGR frames

    python -m eagle_amd.cli --frames 10 --fps 5 --out output/synthetic --annotated      # + annotated.y4m and the team mapping
    python -m eagle_amd.cli --frames 30 --fps 5 --out output/synthetic --processed      # + raw_data.json, processed_data.json and the team mapping
    python -m eagle_amd.cli --frames 30 --fps 5 --out output/synthetic --processed --minimap --minimap-voronoi      # + minimap.y4m

``--annotated`` writes the annotated video of ``main.py:43-81`` as ``annotated.y4m`` (YUV4MPEG2: uncompressed I420, which common players open
without a codec), drawn on the GPU from the raw records, and ``metadata.json`` then carries the ``team_mapping`` like the reference's
(``main.py:37-38``).  ``--processed`` runs the reference's post-processor (``main.py:34-41``: ``Processor.process_data`` and ``format_data``) on
the GPU (eagle_amd/postprocess.py) and writes ``raw_data.json`` (the table, one record per kept frame), ``processed_data.json`` and the
``team_mapping`` into ``metadata.json``; together with ``--annotated`` the video is then drawn from the processed table (kept frames only,
interpolated ball, folded goalkeeper ids), as ``main.py:43-81`` does.  ``--merge-ids`` (with ``--processed``) stitches the fragments of one person
under several tracker ids into one id first and lists the joins as ``merges`` in ``metadata.json``.  ``--minimap`` (with ``--processed``) writes ``minimap.y4m``: the processed table as
a top-down video of the pitch at the clip's fps (eagle_amd/minimap.py; ``--minimap-voronoi`` tints the areas each team controls, ``--minimap-scale``
sets the pixels per metre).  ``--possession`` (with ``--processed``) writes ``possession.json``: per kept frame who has the ball, the passes and
turnovers, and what they add up to per id, per team and per pair of ids (eagle_amd/possession.py).  ``--occupancy`` (with ``--processed``) writes
``occupancy.npy`` and ``occupancy.json``: where every player, every team and the ball spent their time, as seconds per pitch cell
(eagle_amd/occupancy.py; ``--occupancy-grid`` cells per metre, ``--occupancy-sigma`` metres of Gaussian smoothing, ``--occupancy-pictures`` one PPM per
team and one for the ball); the maps follow a person only with ``--merge-ids``.  ``--shape`` (with ``--processed``) writes ``shape.json``: per kept
frame each team's centroid, length, width, hull area, stretch, lines and convex hull, and the clip's means (eagle_amd/shape.py); ``--minimap-hulls [W]``
draws the two hulls into the minimap.  ``--physical`` (with ``--processed``) writes ``physical.json``: per id the distance and the seconds per speed
zone, the total distance, the top speed, the high-speed runs, sprints, accelerations and decelerations, and the list of those efforts
(eagle_amd/physical.py; ``--physical-edges a,b,c,d`` sets the zone edges in m/s, ``--physical-rows`` adds the per-frame speed, acceleration and zone); the figures follow a person only with ``--merge-ids``.  ``--stabilise`` (with ``--processed``) estimates, per kept frame, the motion that every player and the ball share (the small translation, stretch and shear of the pitch plane that a slightly wrong homography gives them at once) from what the players' own paths predict, removes it directly after the table is built and before ``--smooth-tracks``, and writes ``stabilise.json`` (eagle_amd/stabilise.py; ``--stabilise-window``, ``--stabilise-degree``, ``--stabilise-model``, ``--stabilise-min-voters``, ``--stabilise-iterations``, ``--stabilise-trim`` and ``--stabilise-floor`` set the rule, conventional choices that are not fitted to data, ``--stabilise-rows`` adds a record per kept frame); ``metadata.json`` then says ``"stabilised": true``.  ``--smooth-tracks`` (with ``--processed``) replaces the pitch positions of every Player and Goalkeeper by windowed least-squares fits directly after the table is built, trims jumps, hands the fits' velocities to ``kinematics.json``, the physical report, pass options and the control grid, and writes ``smooth.json`` (eagle_amd/smooth.py; ``--smooth-window``, ``--smooth-degree``, ``--smooth-outlier``, ``--smooth-floor`` and ``--smooth-ball`` set the rule, conventional choices that are not fitted to data, ``--smooth-rows`` adds the per-cell records); ``metadata.json`` then says ``"positions": "smoothed"``.  ``--ball-track`` (with ``--processed``) makes the table's ball the detection of every frame that lies on the best physically possible path through the clip, not the reference's choice, and writes ``ball_track.json`` (eagle_amd/balltrack.py; ``--ball-track-speed``, ``-gap``, ``-reward``, ``-break`` set the rule, ``--ball-track-rows`` adds a record per frame).  ``--team-method cluster`` (with ``--processed`` or ``--annotated``) finds the team mapping as the two clusters of the ids' kit colours over the clip instead of by the reference's named colour ranges, and writes ``teams.json`` (eagle_amd/kits.py; ``--team-min-pixels``, ``--team-min-crops``, ``--team-outlier`` set the rule).  ``--pass-options`` (with ``--processed``) writes ``pass_options.json``: per kept frame where the ball's owner could play and per pass event how the pass played ranks among the open ones (eagle_amd/options.py; ``--pass-options-grid R`` adds ``pass_options.npy``, ``--pass-options-pictures`` one PPM per pass event).  ``--roles`` (with ``--processed``) writes ``roles.json``: each team's mean formation, its lines and a label such as 4-4-2, the rows every id played in each role, every change of role and who held each role when (eagle_amd/roles.py; ``--roles-count R``, ``--roles-min-present M``, ``--roles-iterations T`` and ``--roles-lines L`` set the parameters, ``--roles-rows`` adds the ids per role and kept frame); a role follows what a player does, whatever ids the tracker gave.  ``--space`` (with ``--processed``) writes ``space.json``: per id the area of the pitch nearer to him than to anybody else (mean, smallest, largest, by thirds), the mean distance to the nearest opponent, how often an opponent stands within ``--space-radius`` metres and who usually marks him; per team its share of the pitch; with ``--possession`` the owner's room per frame and per pass (eagle_amd/space.py; ``--space-grid R`` cells per metre, ``--space-rows`` adds the per-frame records, ``--space-map`` writes the owner maps as ``space.npy``); an area follows a person only with ``--merge-ids``.  ``--offside`` (with ``--processed``) writes ``offside.json``: per team the offside line of every kept frame (the deepest of the second-last opponent, the halfway line and the ball), per id how often he stood beyond it and by how much at most, and with ``--possession`` per pass whether the receiver was onside, close or offside when the ball was played (eagle_amd/offside.py; ``--offside-direction auto|right|left``, ``--offside-tolerance M``, ``--offside-no-assumed-keeper``, ``--offside-rows`` adds the per-frame lines and margins); only foot points are known and a defender the camera does not see is not counted.  ``--offside-view`` (with ``--processed --offside``) writes ``offside_view.y4m``, the annotated video with that line lying on the grass under the players, and ``offside_view.json``; ``--offside-stills`` (with ``--possession`` too) writes ``offside_<k>.ppm`` per pass with a verdict (eagle_amd/ground.py; the line is only as good as the frame's homography).  ``--shots`` writes ``shots.json``: the camera cuts, gradual transitions and photo flashes of the clip, its shots and which of them look at the pitch (eagle_amd/shots.py; ``--shots-cut``, ``--shots-low``, ``--shots-grass``, ``--shots-window`` and ``--shots-min-len`` set the parameters, conventional choices that are not fitted to footage); ``--trim-to-shot auto`` (or a shot's index) keeps only that shot's frames for everything that follows, the trimming the reference's README asks its users to do by hand.  ``--topview`` writes ``topview.y4m``: every frame warped onto the pitch plane with its homography, the check of the one input every analysis stage trusts (eagle_amd/topview.py; ``--topview-scale``, ``--topview-margin``, ``--topview-markings``, ``--topview-carry``); ``--topview-mosaic`` adds ``topview_mosaic.ppm``, ``topview_count.npy`` and ``topview.json``, per frame its coverage and its distance from the mosaic (``--topview-mask-boxes``, ``--topview-step``, ``--topview-min-count``, ``--topview-suspect``; the suspect ratio 2.0 is a conventional choice, not fitted to footage).  Video decode and compressed encode are out of scope (SURVEY §8f rows 3-4).  The cadence is main.py:27's by default (homography once per second, key-point model three times per
second, optical flow in between); ``--every-frame`` selects the stateless configuration (both on every frame).  ``--ball-flights`` (with
``--processed``) writes ``ball_flights.json``: the ball's path cut into straight flights of constant speed, the kicks between them, the shots and, with
``--possession``, per pass its kick, kicker and speed (eagle_amd/flights.py; ``--ball-flights-rows``, ``-noise``, ``-penalty``, ``-spike``, ``-kick``,
``-shot`` set the rule, ``--ball-flights-cells`` adds the per-row arrays).  ``--goal-view`` (with ``--processed``) writes ``goal_view.json``: how much of
the goal mouth every attacker sees past the other team, per id the totals, with ``--ball-flights`` per shot the ball's view and whether its lane was open,
with ``--possession`` per pass the threat it added (eagle_amd/goalview.py; ``--goal-view-direction``, ``--goal-view-cells``); ``--goal-view-map`` also writes
``goal_view.npy``, the value of every cell of the pitch per kept frame (``--goal-view-grid``, ``--goal-view-team``)."""
import argparse
import json
import os
import time

import numpy as np


def load_state_dict(path):
    """A checkpoint file -> {name: float32 ndarray}.  torch is used only here, to read the file (weight loading is the one place the
    north star allows it)."""
    import torch
    try:                                    # plain state-dict files (.pth) need no unpickling of arbitrary objects
        obj = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:                  # ultralytics .pt checkpoints pickle their model classes: full unpickling executes code from the file
        import warnings
        warnings.warn(f"{path}: not loadable with weights_only=True ({type(e).__name__}); falling back to full unpickling — only do this with "
                      "checkpoints you trust", stacklevel=2)
        obj = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(obj, dict) and "model" in obj and hasattr(obj["model"], "state_dict"):      # ultralytics checkpoint
        obj = obj["model"].float().state_dict()
    elif hasattr(obj, "state_dict"):
        obj = obj.state_dict()
    elif isinstance(obj, dict) and "state_dict" in obj:
        obj = obj["state_dict"]
    return {k: v.detach().float().cpu().numpy() for k, v in obj.items() if hasattr(v, "detach") and v.ndim >= 0 and not k.endswith("num_batches_tracked")}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clip", help=".npy file with uint8 [n,h,w,3] BGR frames (default: synthetic clip)")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--fps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="output/synthetic")
    ap.add_argument("--detector", default="n")
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--precision", default="f32s", choices=["f16", "f32", "f32s"],
                    help="f32s (default): fp32-grade results on fp16 MFMAs (what the reference's .float() path computes); f16: fastest; f32: bit-exact fp32 MFMA")
    ap.add_argument("--detector-precision", default=None, choices=["f16", "f32", "f32s"],
                    help="family of the detector alone (default: the library's — exact fp32 next to f32s key-points, so that boxes / confidences / ids are the fp32 arithmetic's bit for bit)")
    ap.add_argument("--allow-saturation", action="store_true",
                    help="f32s stores activations with a range of +-4094; by default a run in which one was clipped fails (EAGLE_E_RANGE). With this flag it only warns "
                         "(for a checkpoint with larger activations prefer --precision f32)")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--num-homography", type=int, default=1, help="homography solves per second (main.py:27: 1)")
    ap.add_argument("--num-keypoint-detection", type=int, default=3, help="key-point model runs per second (main.py:27: 3)")
    ap.add_argument("--every-frame", action="store_true", help="key-points and homography on every frame (stateless configuration)")
    ap.add_argument("--letterbox", default="rect", choices=["rect", "square"],
                    help="detector input geometry: 'rect' = ultralytics LetterBox(auto=True), what the reference's .pt detectors run with (cm.py:56-57); 'square' = auto=False, the "
                         "static imgsz x imgsz input of its exported ONNX detector (the CPU default, cm.py:54-55)")
    ap.add_argument("--calibration", action="store_true")
    ap.add_argument("--tracker", action="store_true", help="key players by track id (BoT-SORT association) instead of the detection index")
    ap.add_argument("--reid", action="store_true", help="with --tracker: appearance matching with OSNet-x0.25 embeddings, as the reference configures BotSort (cm.py:66-72)")
    ap.add_argument("--reid-weights", help="with --reid: torchreid osnet_x0_25 state-dict (.pth; keys conv1.* ... fc.*, the 'reid.' prefix is added here)")
    ap.add_argument("--camera-motion", nargs="?", const="ecc", default=None, choices=["ecc", "sparse"],
                    help="with --tracker: compensate camera motion; 'ecc' (default when the flag is given) is boxmot's default estimator, i.e. the reference's "
                         "configuration; 'sparse' = BoT-SORT's sparse-optical-flow alternative on a fixed grid")
    ap.add_argument("--keypoint-weights", help="HRNet state-dict (.pth as the reference loads at cm.py:58-59: keys unnormalized_model.0.* / unnormalized_model.1.*)")
    ap.add_argument("--detector-weights", help="detector checkpoint: a torch state-dict (.pth) with ultralytics key names model.N.*, or an ultralytics .pt whose 'model' entry has .state_dict()")
    ap.add_argument("--synthetic-weights", action="store_true", help="run with seeded RANDOM networks (plumbing / benchmarking only: the coordinates are meaningless)")
    ap.add_argument("--native-fps", type=float, default=None, help="frame rate of --clip: sample it down to --fps the way read_video does (io.py:17-25)")
    ap.add_argument("--annotated", action="store_true",
                    help="also write <out>/annotated.y4m (the reference's annotated video, main.py:43-81, as uncompressed YUV4MPEG2) and put the team mapping into metadata.json")
    ap.add_argument("--processed", action="store_true",
                    help="also run the post-processor of main.py:34-41 on the GPU: write <out>/raw_data.json and <out>/processed_data.json, put the team mapping into "
                         "metadata.json, and draw --annotated from the processed table")
    ap.add_argument("--smooth", action="store_true", help="with --processed: process_data(smooth=True)")
    ap.add_argument("--merge-ids", action="store_true",
                    help="with --processed: stitch the fragments of one person under several tracker ids into one id (off: the reference as written, which never "
                         "merges); metadata.json then lists the joins as \"merges\" and its team_mapping holds the teams the merged ids inherit")
    ap.add_argument("--stabilise", action="store_true",
                    help="with --processed: estimate each kept frame's common motion (the small translation, stretch and shear a slightly wrong homography gives "
                         "every player and the ball at once) from what the players' own paths predict, and remove it, directly after the table is built and before "
                         "--smooth-tracks; writes <out>/stabilise.json (the constants are conventional choices, not fitted to data)")
    ap.add_argument("--stabilise-window", type=int, default=None, metavar="F", help="with --stabilise: the half-width in frames, 1 .. 64 (default min(64, max(2, round(fps))))")
    ap.add_argument("--stabilise-degree", type=int, default=None, choices=[1, 2], metavar="D", help="with --stabilise: the degree of the predicting polynomial (default 2)")
    ap.add_argument("--stabilise-model", default=None, choices=["translation", "affine"], help="with --stabilise: the common motion's model (default affine)")
    ap.add_argument("--stabilise-min-voters", type=int, default=None, metavar="N", help="with --stabilise: rows with fewer voting players keep their positions, 3 .. 64 (default 6)")
    ap.add_argument("--stabilise-iterations", type=int, default=None, metavar="T", help="with --stabilise: rounds, 1 .. 4 (default 2)")
    ap.add_argument("--stabilise-trim", type=float, default=None, metavar="K", help="with --stabilise: trim a voter beyond K medians of the row's deviations; 0: none (default 3)")
    ap.add_argument("--stabilise-floor", type=float, default=None, metavar="M", help="with --stabilise: never trim a voter closer than M metres to the median (default 0.1)")
    ap.add_argument("--stabilise-rows", action="store_true", help="with --stabilise: also write a record per kept frame into stabilise.json")
    ap.add_argument("--smooth-tracks", action="store_true",
                    help="with --processed: replace the pitch positions of every Player and Goalkeeper by windowed least-squares fits right after the table is built, "
                         "trim jumps, and hand the fits' velocities to every later stage; writes <out>/smooth.json (the half-width, degree, threshold and floor are "
                         "conventional choices, not fitted to data)")
    ap.add_argument("--smooth-window", type=int, default=None, metavar="F", help="with --smooth-tracks: the half-width in frames, 1 .. 64 (default max(2, round(0.4 fps)))")
    ap.add_argument("--smooth-degree", type=int, default=None, choices=[1, 2], metavar="D", help="with --smooth-tracks: the polynomial degree (default 2)")
    ap.add_argument("--smooth-outlier", type=float, default=None, metavar="K", help="with --smooth-tracks: reject a sample beyond K medians of its window's residuals; 0: none (default 4)")
    ap.add_argument("--smooth-floor", type=float, default=None, metavar="M", help="with --smooth-tracks: never reject a sample closer than M metres to its fit (default 0.25)")
    ap.add_argument("--smooth-ball", type=int, default=None, metavar="F", help="with --smooth-tracks: smooth the ball too, with this half-width in frames (default: the ball stays)")
    ap.add_argument("--smooth-rows", action="store_true", help="with --smooth-tracks: also write the per-cell records into smooth.json")
    ap.add_argument("--minimap", action="store_true", help="with --processed: also write <out>/minimap.y4m, the processed table as a top-down video of the pitch")
    ap.add_argument("--minimap-voronoi", action="store_true", help="with --minimap: tint the pitch by the team whose player is nearest")
    ap.add_argument("--minimap-scale", type=int, default=8, help="with --minimap: pixels per metre (even, 2 .. 32)")
    ap.add_argument("--kinematics", action="store_true", help="with --processed: also write <out>/kinematics.json, per id the distance covered (m) and the top speed (m/s)")
    ap.add_argument("--minimap-control", action="store_true", help="with --processed: write <out>/minimap.y4m with the pitch-control layer (not together with --minimap-voronoi)")
    ap.add_argument("--control-grid", type=int, default=None, choices=[1, 2, 4], metavar="R",
                    help="with --processed: also write <out>/control.npy (uint8 [rows, 68 R, 105 R]) and <out>/control_share.json, team 0's share of the pitch per row")
    ap.add_argument("--minimap-trails", nargs="?", const="fps", default=None, metavar="W",
                    help="with --minimap: draw the paths of every person and the ball over the last W kept rows (default: --fps rows)")
    ap.add_argument("--minimap-passes", action="store_true",
                    help="with --minimap: draw an arrow per pass or turnover and a ring round the ball's owner (runs the possession step with its defaults)")
    ap.add_argument("--trajectory", default=None, metavar="IDS",
                    help="with --processed: also write <out>/trajectory.ppm, the paths of the comma-separated ids (or `ball`) over the clip, at --minimap-scale")
    ap.add_argument("--pass-pictures", action="store_true",
                    help="with --processed: also write <out>/pass_<k>.ppm, one still per pass event at its release row (runs the possession step with its defaults)")
    ap.add_argument("--possession", action="store_true",
                    help="with --processed: also write <out>/possession.json, per kept frame who has the ball, the passes and turnovers, and per id / team what they add up "
                         "to (most useful with --merge-ids)")
    ap.add_argument("--occupancy", action="store_true",
                    help="with --processed: also write <out>/occupancy.npy (float64 seconds [maps, 68 R, 105 R]) and <out>/occupancy.json, where every player, every "
                         "team and the ball spent their time (the maps follow a person only with --merge-ids)")
    ap.add_argument("--occupancy-grid", type=int, default=1, choices=[1, 2, 4], metavar="R", help="with --occupancy: cells per metre")
    ap.add_argument("--occupancy-sigma", type=float, default=2.0, metavar="S", help="with --occupancy: the Gaussian's sigma in metres, 0 .. 10 (0: the raw counts)")
    ap.add_argument("--occupancy-pictures", action="store_true",
                    help="with --occupancy: also write one binary PPM per team (<out>/occupancy_team<t>.ppm) and one for the ball (<out>/occupancy_ball.ppm) at "
                         "--minimap-scale pixels per metre")
    ap.add_argument("--shape", action="store_true",
                    help="with --processed: also write <out>/shape.json, per kept frame each team's centroid, length, width, hull area, stretch index, lines and "
                         "convex hull, and their means over the clip")
    ap.add_argument("--minimap-hulls", nargs="?", const="1", default=None, metavar="W",
                    help="with --minimap: draw the convex hull of each team, W pixels either side of the line (1 .. 8, default 1); computes the team shape if "
                         "--shape did not")
    ap.add_argument("--physical", action="store_true",
                    help="with --processed: also write <out>/physical.json, per id the distance and the seconds per speed zone, the total distance, the top speed and "
                         "the high-speed runs, sprints, accelerations and decelerations (computes the velocities with the --kinematics defaults if they are absent; the "
                         "figures follow a person only with --merge-ids)")
    ap.add_argument("--physical-rows", action="store_true",
                    help="with --physical: also write the speed (m/s), its derivative (m/s^2) and the zone per id and kept frame into physical.json")
    ap.add_argument("--physical-edges", default=None, metavar="a,b,c,d",
                    help="with --physical: the four zone edges in m/s, strictly ascending (default 2,4,5.5,7: conventional choices, not fitted to data)")
    ap.add_argument("--pass-options", action="store_true",
                    help="with --processed: also write <out>/pass_options.json, per kept frame where the ball's owner could play (status, owner, best option, the "
                         "option per teammate id) and per pass event how the pass played ranks among them (computes velocities and possession with their "
                         "defaults if they are absent; 16 samples, 0.7 s, 5 m/s, 4 / s and a 15 m/s ball are conventional choices, not fitted to data)")
    ap.add_argument("--pass-options-grid", type=int, default=None, choices=[1, 2, 4], metavar="R",
                    help="with --pass-options: also write <out>/pass_options.npy (uint8 [rows, 68 R, 105 R]), the option surface per kept frame at R cells per metre")
    ap.add_argument("--pass-options-pictures", action="store_true",
                    help="with --pass-options: also write <out>/pass_options_<k>.ppm, the option surface at the release row of pass event k in the owner's team "
                         "colour, at --minimap-scale pixels per metre")
    ap.add_argument("--roles", action="store_true",
                    help="with --processed: also write <out>/roles.json, each team's mean formation from an exact per-frame assignment of its players to roles: the "
                         "role positions, lines and label (4-4-2), the rows per id and role, every change of role and the stints per role (10 roles, 8 present, 8 "
                         "rounds and 3 lines are conventional choices, not fitted to data)")
    ap.add_argument("--roles-count", type=int, default=None, metavar="R", help="with --roles: the number of roles per team, 2 .. 10 (default 10)")
    ap.add_argument("--roles-min-present", type=int, default=None, metavar="M",
                    help="with --roles: the fewest players of a team a frame must show to be assigned, 2 .. R (default 8, or R below that)")
    ap.add_argument("--roles-iterations", type=int, default=None, metavar="T", help="with --roles: the rounds of assignment and re-estimation, 1 .. 32 (default 8)")
    ap.add_argument("--roles-lines", type=int, default=None, metavar="L", help="with --roles: the lines a team is split into, 2 .. 4 (default 3)")
    ap.add_argument("--roles-rows", action="store_true", help="with --roles: also write the id playing each role per kept frame and team into roles.json")
    ap.add_argument("--space", action="store_true",
                    help="with --processed: also write <out>/space.json, the room every player has: the exact area of the pitch nearer to him than to anybody "
                         "else, by thirds, his nearest opponent and the opponents within a radius, per id, per team and (with --possession) per owner and pass")
    ap.add_argument("--space-grid", type=int, default=None, choices=[1, 2, 4], metavar="R", help="with --space: the cells per metre of the grid, 1, 2 or 4 (default 1)")
    ap.add_argument("--space-radius", type=float, default=None, metavar="M",
                    help="with --space: the marking radius in metres, > 0 and <= 1024 (default 3, a conventional choice, not fitted to data)")
    ap.add_argument("--space-rows", action="store_true", help="with --space: also write the sites of every kept frame into space.json")
    ap.add_argument("--offside", action="store_true",
                    help="with --processed: also write <out>/offside.json, the offside line of each team in every kept frame (the deepest of the second-last opponent, "
                         "the halfway line and the ball), who was beyond it and by how much, per id how often; with --possession also a verdict per pass: was the "
                         "receiver onside, close or offside when the ball was played (eagle_amd/offside.py)")
    ap.add_argument("--offside-direction", choices=["auto", "right", "left"], default=None,
                    help="with --offside: the way the team with value 0 attacks, towards x = 105 (right) or x = 0 (left); auto (the default) votes over the frames")
    ap.add_argument("--offside-tolerance", type=float, default=None, metavar="M",
                    help="with --offside: a receiver within M metres of the line is `close`; >= 0 and <= 1024 (default 0.5, a conventional choice, not fitted to data)")
    ap.add_argument("--offside-no-assumed-keeper", action="store_true",
                    help="with --offside: do not take a goalkeeper the camera does not see to stand on his goal line (the line is then the second-last opponent seen)")
    ap.add_argument("--offside-rows", action="store_true", help="with --offside: also write the line and the margins of every kept frame into offside.json")
    ap.add_argument("--offside-view", action="store_true",
                    help="with --processed --offside: also write <out>/offside_view.y4m, the annotated video of the table with the offside line lying on the grass under "
                         "the players (a zone behind it, a ring under the second-last opponent and under every attacker beyond the line), and offside_view.json "
                         "(eagle_amd/ground.py; the line is only as good as the frame's homography, which --topview shows)")
    ap.add_argument("--offside-view-team", choices=["possession", "0", "1", "both"], default=None, metavar="T",
                    help="with --offside-view: whose attack is shown: the team in possession on each frame (needs --possession, and is the default with it), "
                         "team 0, 1 or both (the default without --possession)")
    ap.add_argument("--offside-view-width", type=float, default=None, metavar="M",
                    help="with --offside-view or --offside-stills: the width of the line in metres, > 0 and <= 10 (default 0.25, a conventional choice)")
    ap.add_argument("--offside-view-no-zone", action="store_true", help="with --offside-view or --offside-stills: do not tint the zone between the line and the goal line")
    ap.add_argument("--offside-view-no-key", action="store_true",
                    help="with --offside-view or --offside-stills: draw over everything, players included, instead of only where the frame's pixel is grass")
    ap.add_argument("--offside-stills", action="store_true",
                    help="with --processed --offside --possession: write <out>/offside_<k>.ppm for every pass k with a verdict: the frame in which the ball was played with "
                         "the receiver's team's line and a ring under the receiver, green (onside), yellow (close) or red (offside)")
    ap.add_argument("--space-map", action="store_true",
                    help="with --space: also write <out>/space.npy (uint8 [rows, 68 R, 105 R]), per cell the index of its owner among the frame's sites, 255 on a skipped frame")
    ap.add_argument("--ball-track", action="store_true",
                    help="with --processed: the table's ball is the detection of every frame that lies on the best physically possible path through the clip "
                         "instead of the reference's choice (a frame's only detection whatever it is, of several the nearest to the image origin); also write "
                         "<out>/ball_track.json.  With --shots or --trim-to-shot the cuts break the path (eagle_amd/balltrack.py)")
    ap.add_argument("--ball-track-speed", type=float, default=None, metavar="PX",
                    help="with --ball-track: the ball's greatest speed in pixels per frame, > 0 and <= 65535 (default a tenth of the frame's width, a conventional choice)")
    ap.add_argument("--ball-track-gap", type=int, default=None, metavar="G", help="with --ball-track: the most frames a link may span, 1 .. 64 (default min(64, --fps))")
    ap.add_argument("--ball-track-reward", type=float, default=None, metavar="PX",
                    help="with --ball-track: what a sighting of confidence 1 is worth, in pixels of path, > 0 and <= 65535 (default the speed)")
    ap.add_argument("--ball-track-break", type=float, default=None, metavar="PX",
                    help="with --ball-track: what it costs to break the path off and start again, in pixels, > 0 and <= 1048576 (default two and a half rewards)")
    ap.add_argument("--ball-track-rows", action="store_true", help="with --ball-track: also write the record of every frame into ball_track.json")
    ap.add_argument("--team-method", choices=("colours", "cluster"), default="colours",
                    help="with --processed or --annotated: how the team mapping is found.  colours (the default): the reference's rule, named colour ranges and the two "
                         "most common names.  cluster: the two clusters of the ids' kit colours over the clip, which separates two kits of one colour name and leaves "
                         "a referee in neither team; also write <out>/teams.json (eagle_amd/kits.py)")
    ap.add_argument("--team-min-pixels", type=int, default=None, metavar="N", help="with --team-method cluster: the least counted pixels of a crop's shirt window, 1 .. 1048576 (default 32)")
    ap.add_argument("--team-min-crops", type=int, default=None, metavar="N", help="with --team-method cluster: the least used crops of an id that votes, 1 .. 65536 (default 3)")
    ap.add_argument("--team-outlier", type=float, default=None, metavar="R",
                    help="with --team-method cluster: an id farther from its team's medoid than R times the distance between the medoids is in neither team, "
                         "0 .. 1024, 0 = off (default 0.5)")
    ap.add_argument("--ball-flights", action="store_true",
                    help="with --processed: cut the ball's path into straight flights of constant speed and write <out>/ball_flights.json: the flights (still, carried, "
                         "free), the kicks between them, the shots and, with --possession, per pass its kick, kicker and speed.  With --shots or --trim-to-shot the "
                         "shots' first frames break the path (eagle_amd/flights.py; the constants are conventional choices, not fitted to data)")
    ap.add_argument("--ball-flights-rows", type=int, default=None, metavar="L", help="with --ball-flights: the longest flight in rows, 2 .. 128 (default 64)")
    ap.add_argument("--ball-flights-noise", type=float, default=None, metavar="M", help="with --ball-flights: the noise of a ball sample in metres (default 0.25)")
    ap.add_argument("--ball-flights-penalty", type=float, default=None, metavar="P", help="with --ball-flights: the price of a flight in noise variances (default 16)")
    ap.add_argument("--ball-flights-spike", type=float, default=None, metavar="M", help="with --ball-flights: a sample this far off its neighbours' line is set aside (default 1.0)")
    ap.add_argument("--ball-flights-kick", type=float, default=None, metavar="V", help="with --ball-flights: the change of velocity of a kick in m/s (default 3)")
    ap.add_argument("--ball-flights-shot", type=float, default=None, metavar="V", help="with --ball-flights: the least speed of a shot in m/s (default 10)")
    ap.add_argument("--ball-flights-cells", action="store_true", help="with --ball-flights: also write the per-row arrays into ball_flights.json")
    ap.add_argument("--goal-view", action="store_true",
                    help="with --processed: write <out>/goal_view.json: the open angle of the goal mouth that every attacker sees past the other team's players (discs of "
                         "0.4 m) and keeper (1.0 m) in every kept frame, per id the totals, with --ball-flights per shot the ball's view and whether its lane was open, with "
                         "--possession per pass the angle gained (eagle_amd/goalview.py; the constants are conventional choices, not fitted to data)")
    ap.add_argument("--goal-view-direction", choices=["offside", "right", "left"], default=None,
                    help="with --goal-view: the way the team with value 0 attacks, towards x = 105 (right) or x = 0 (left); offside (the default) takes what --offside settled")
    ap.add_argument("--goal-view-cells", action="store_true", help="with --goal-view: also write the per-frame records into goal_view.json")
    ap.add_argument("--goal-view-map", action="store_true",
                    help="with --goal-view: also write <out>/goal_view.npy, uint8 [kept frames][68 R][105 R]: the open angle from every cell of the pitch, 256 per radian")
    ap.add_argument("--goal-view-grid", type=int, choices=[1, 2, 4], default=None, metavar="R", help="with --goal-view-map: cells per metre, 1, 2 or 4 (default 1)")
    ap.add_argument("--goal-view-team", choices=["0", "1", "possession"], default=None,
                    help="with --goal-view-map: the attacking team of the map; possession (the default with --possession): per frame the team that owns the ball")
    ap.add_argument("--shots", action="store_true",
                    help="also write <out>/shots.json: the camera cuts, gradual transitions and photo flashes of the clip, its shots and which of them look at "
                         "the pitch, and put the shot count into metadata.json (the thresholds are conventional choices, not fitted to footage)")
    ap.add_argument("--shots-cut", type=float, default=None, metavar="C", help="with --shots or --trim-to-shot: the score of a cut, 0 .. 1 (default 0.30)")
    ap.add_argument("--shots-low", type=float, default=None, metavar="L",
                    help="with --shots or --trim-to-shot: the score below which the picture has returned behind a flash, 0 .. C (default 0.10)")
    ap.add_argument("--shots-grass", type=float, default=None, metavar="G",
                    help="with --shots or --trim-to-shot: the mean share of grass pixels from which a shot looks at the pitch, 0 .. 1 (default 0.35)")
    ap.add_argument("--shots-window", type=int, default=None, metavar="W",
                    help="with --shots or --trim-to-shot: the longest gradual transition in frames, at least 2 (default max(2, round(0.4 fps)))")
    ap.add_argument("--shots-min-len", type=int, default=None, metavar="N",
                    help="with --shots or --trim-to-shot: the fewest frames of a usable shot, at least 1 (default --fps)")
    ap.add_argument("--trim-to-shot", default=None, metavar="{auto,K}",
                    help="keep only the frames of shot K of the clip (auto: the longest usable shot, the earliest on a tie) for everything that follows, the "
                         "trimming the reference asks its users to do by hand; metadata.json records the shot's first frame and count")
    ap.add_argument("--refine-lines", action="store_true",
                    help="refine each frame's homography on the frame's painted lines directly after the coordinates are computed (and after --trim-to-shot): "
                         "raw_coordinates.json and everything behind it carry the refined result; writes <out>/lines.json (eagle_amd/linefit.py; the constants are "
                         "conventional choices, not fitted to data)")
    ap.add_argument("--refine-lines-rounds", type=int, default=None, metavar="T", help="with --refine-lines: rounds, 0 .. 16 (default 5)")
    ap.add_argument("--refine-lines-radius", type=float, default=None, metavar="M", help="with --refine-lines: the first round's inlier radius in metres, at most 8 (default 2.5)")
    ap.add_argument("--refine-lines-min-radius", type=float, default=None, metavar="M", help="with --refine-lines: the last and the deciding inlier radius in metres (default 0.5)")
    ap.add_argument("--refine-lines-max-shift", type=float, default=None, metavar="M",
                    help="with --refine-lines: a refined homography that moves the view by more than M metres is not taken (default 3)")
    ap.add_argument("--refine-lines-contrast", type=int, default=None, metavar="TAU",
                    help="with --refine-lines: a line pixel's b + 2 g + r exceeds both neighbours' by TAU, 1 .. 1020 (default 200, i.e. 50 grey levels)")
    ap.add_argument("--refine-lines-model", default=None, choices=["projective", "affine", "translation"], help="with --refine-lines: the largest correction (default projective)")
    ap.add_argument("--refine-lines-rows", action="store_true", help="with --refine-lines: also write a record per frame into lines.json")
    ap.add_argument("--topview", action="store_true",
                    help="also write <out>/topview.y4m: every frame warped onto the pitch plane with its homography (the picture that shows whether the homography "
                         "puts the painted lines where the pitch model has them); needs neither --processed nor a tracker")
    ap.add_argument("--topview-scale", type=int, default=None, metavar="S", help="with --topview: pixels per metre, even, 2 .. 32 (default 8)")
    ap.add_argument("--topview-margin", type=int, default=None, metavar="M", help="with --topview: pixels round the pitch, even, 0 .. 64 (default two metres' worth, at most 64)")
    ap.add_argument("--topview-markings", action="store_true", help="with --topview: draw the pitch model's markings over the pictures, in red")
    ap.add_argument("--topview-carry", action="store_true",
                    help="with --topview: a frame without a homography of its own uses the latest earlier one, which is what the reference projects with")
    ap.add_argument("--topview-mosaic", action="store_true",
                    help="with --topview: also write <out>/topview_mosaic.ppm (the mean of the warped frames: the pitch without the players), <out>/topview_count.npy "
                         "(how many frames each pixel has) and <out>/topview.json (per frame its coverage and its distance from the mosaic, the clip's median and the "
                         "suspect frames)")
    ap.add_argument("--topview-mask-boxes", type=float, default=None, metavar="PAD",
                    help="with --topview-mosaic: leave the inside of every detection box, widened by PAD pixels, out of the mosaic")
    ap.add_argument("--topview-step", type=int, default=None, metavar="K", help="with --topview-mosaic: build the mosaic from every K-th frame (default 1)")
    ap.add_argument("--topview-min-count", type=int, default=None, metavar="C", help="with --topview-mosaic: a mosaic pixel needs C frames (default 1)")
    ap.add_argument("--topview-suspect", type=float, default=None, metavar="R",
                    help="with --topview-mosaic: list the frames whose residual exceeds R times the clip's median (default 2.0, a conventional choice, not fitted to footage)")
    a = ap.parse_args(argv)
    if not a.topview and (a.topview_markings or a.topview_carry or a.topview_mosaic or
                          any(v is not None for v in (a.topview_scale, a.topview_margin, a.topview_mask_boxes, a.topview_step, a.topview_min_count, a.topview_suspect))):
        ap.error("--topview-scale, --topview-margin, --topview-markings, --topview-carry, --topview-mosaic, --topview-mask-boxes, --topview-step, --topview-min-count and "
                 "--topview-suspect set up the top view: they need --topview")
    if a.topview:
        if not a.topview_mosaic and any(v is not None for v in (a.topview_mask_boxes, a.topview_step, a.topview_min_count, a.topview_suspect)):
            ap.error("--topview-mask-boxes, --topview-step, --topview-min-count and --topview-suspect set up the mosaic: they need --topview-mosaic")
        S = 8 if a.topview_scale is None else a.topview_scale
        if not (2 <= S <= 32 and S % 2 == 0):
            ap.error("--topview-scale takes an even number of pixels per metre within 2 .. 32")
        M = min(64, 2 * S) if a.topview_margin is None else a.topview_margin
        if not (0 <= M <= 64 and M % 2 == 0):
            ap.error("--topview-margin takes an even number of pixels within 0 .. 64")
        if a.topview_step is not None and a.topview_step < 1:
            ap.error("--topview-step takes at least 1")
        if a.topview_min_count is not None and a.topview_min_count < 1:
            ap.error("--topview-min-count takes at least 1")
        if a.topview_mask_boxes is not None and not 0.0 <= a.topview_mask_boxes < float("inf"):      # (nan fails both comparisons)
            ap.error("--topview-mask-boxes takes a finite padding of 0 pixels or more")
        if a.topview_suspect is not None and not 0.0 < a.topview_suspect < float("inf"):
            ap.error("--topview-suspect takes a finite ratio above 0")
        a.topview_set = dict(scale=S, margin=M, markings=a.topview_markings)
        a.mosaic_set = dict(a.topview_set, mask_boxes=a.topview_mask_boxes is not None, box_pad=a.topview_mask_boxes or 0.0, step=a.topview_step or 1,
                            min_count=a.topview_min_count or 1)
    shot_set = {"cut": a.shots_cut, "low": a.shots_low, "grass_thr": a.shots_grass, "window": a.shots_window, "min_len": a.shots_min_len}
    if not (a.shots or a.trim_to_shot is not None) and any(v is not None for v in shot_set.values()):
        ap.error("--shots-cut, --shots-low, --shots-grass, --shots-window and --shots-min-len set up the shots: they need --shots or --trim-to-shot")
    if a.shots or a.trim_to_shot is not None:
        if a.fps < 1:
            ap.error("--shots and --trim-to-shot need --fps of at least 1")
        for k in ("cut", "low", "grass_thr"):
            if shot_set[k] is not None:
                if not 0.0 <= shot_set[k] <= 1.0:                       # (nan fails both comparisons)
                    ap.error("--shots-cut, --shots-low and --shots-grass take a share of 0 .. 1")
                shot_set[k] = int(shot_set[k] * 65536 + 0.5)
        from . import shots as _shots
        resolved = dict(_shots.default_params(a.fps), **{k: v for k, v in shot_set.items() if v is not None})
        if resolved["low"] > resolved["cut"]:
            ap.error("--shots-low must not be above --shots-cut")
        if resolved["window"] < 2:
            ap.error("--shots-window takes at least 2 frames")
        if resolved["min_len"] < 1:
            ap.error("--shots-min-len takes at least 1 frame")
        if a.trim_to_shot is not None and a.trim_to_shot != "auto":
            try:
                a.trim_to_shot = int(a.trim_to_shot)
            except ValueError:
                a.trim_to_shot = -1
            if a.trim_to_shot < 0:
                ap.error("--trim-to-shot takes `auto` or the index of a shot, 0 or above")
    if a.space and not a.processed:
        ap.error("--space works on the processed table: it needs --processed")
    if not a.space and (a.space_rows or a.space_map or a.space_grid is not None or a.space_radius is not None):
        ap.error("--space-grid, --space-radius, --space-rows and --space-map set up the space report: they need --space")
    if a.space:
        a.space_set = (1 if a.space_grid is None else a.space_grid, 3.0 if a.space_radius is None else a.space_radius)
        if not (a.space_set[1] == a.space_set[1] and 0.0 < a.space_set[1] <= 1024.0):
            ap.error("--space-radius: M must be > 0 and <= 1024 metres")
    if a.ball_track and not a.processed:
        ap.error("--ball-track chooses the ball of the processed table: it needs --processed")
    bt_set = {"speed": a.ball_track_speed, "gap": a.ball_track_gap, "reward": a.ball_track_reward, "brk": a.ball_track_break}
    if not a.ball_track and (a.ball_track_rows or any(v is not None for v in bt_set.values())):
        ap.error("--ball-track-speed, --ball-track-gap, --ball-track-reward, --ball-track-break and --ball-track-rows set up the ball track: they need --ball-track")
    if a.ball_track:
        if a.fps < 1:
            ap.error("--ball-track needs --fps of at least 1")
        if a.ball_track_gap is not None and not 1 <= a.ball_track_gap <= 64:
            ap.error("--ball-track-gap takes 1 .. 64 frames")
        for v, top, flag in ((a.ball_track_speed, 65535.0, "speed"), (a.ball_track_reward, 65535.0, "reward"), (a.ball_track_break, 1048576.0, "break")):
            if v is not None and not 0.0 < v <= top:                      # (NaN fails too)
                ap.error(f"--ball-track-{flag}: PX must be > 0 and <= {top:.0f} pixels")
        a.ball_track_set = {k: v for k, v in bt_set.items() if v is not None}
    team_set = {"min_pixels": a.team_min_pixels, "min_crops": a.team_min_crops, "outlier": a.team_outlier}
    if a.team_method != "cluster" and any(v is not None for v in team_set.values()):
        ap.error("--team-min-pixels, --team-min-crops and --team-outlier set up the team clustering: they need --team-method cluster")
    a.team_set = {}
    if a.team_method == "cluster":
        if not (a.processed or a.annotated):
            ap.error("--team-method cluster chooses how the team mapping is found: it needs --processed or --annotated")
        if a.team_min_pixels is not None and not 1 <= a.team_min_pixels <= 1048576:
            ap.error("--team-min-pixels takes 1 .. 1048576 pixels")
        if a.team_min_crops is not None and not 1 <= a.team_min_crops <= 65536:
            ap.error("--team-min-crops takes 1 .. 65536 crops")
        if a.team_outlier is not None and not 0.0 <= a.team_outlier <= 1024.0:                      # (NaN fails too)
            ap.error("--team-outlier: R must be >= 0 and <= 1024 (--team-method cluster)")
        a.team_set = {k: v for k, v in team_set.items() if v is not None}
    if a.offside and not a.processed:
        ap.error("--offside works on the processed table: it needs --processed")
    if not a.offside and (a.offside_rows or a.offside_no_assumed_keeper or a.offside_direction is not None or a.offside_tolerance is not None):
        ap.error("--offside-direction, --offside-tolerance, --offside-no-assumed-keeper and --offside-rows set up the offside report: they need --offside")
    if (a.offside_view or a.offside_stills) and not (a.processed and a.offside):
        ap.error("--offside-view and --offside-stills draw the offside result of the processed table: they need --processed --offside")
    if a.offside_stills and not a.possession:
        ap.error("--offside-stills shows the passes: it needs --possession")
    if not a.offside_view and a.offside_view_team is not None:
        ap.error("--offside-view-team sets up the offside view: it needs --offside-view")
    if not (a.offside_view or a.offside_stills) and (a.offside_view_width is not None or a.offside_view_no_zone or a.offside_view_no_key):
        ap.error("--offside-view-width, --offside-view-no-zone and --offside-view-no-key set up the offside pictures: they need --offside-view or --offside-stills")
    if a.offside_view_team == "possession" and not a.possession:
        ap.error("--offside-view-team possession follows the owner of the ball: it needs --possession")
    if a.offside_view or a.offside_stills:
        team = a.offside_view_team or ("possession" if a.possession else "both")
        a.offside_view_set = dict(team=int(team) if team in ("0", "1") else team, width=0.25 if a.offside_view_width is None else a.offside_view_width,
                                  zone=not a.offside_view_no_zone, keyed=not a.offside_view_no_key)
        if not 0.0 < a.offside_view_set["width"] <= 10.0:
            ap.error("--offside-view-width: M must be > 0 and <= 10 metres")
    if a.offside:
        a.offside_set = (a.offside_direction or "auto", 0.5 if a.offside_tolerance is None else a.offside_tolerance)
        if not 0.0 <= a.offside_set[1] <= 1024.0:
            ap.error("--offside-tolerance: M must be >= 0 and <= 1024 metres")
    if a.roles and not a.processed:
        ap.error("--roles works on the processed table: it needs --processed")
    if not a.roles and (a.roles_rows or any(v is not None for v in (a.roles_count, a.roles_min_present, a.roles_iterations, a.roles_lines))):
        ap.error("--roles-count, --roles-min-present, --roles-iterations, --roles-lines and --roles-rows set up the roles: they need --roles")
    if a.roles:
        R = 10 if a.roles_count is None else a.roles_count
        a.roles_set = (R, min(8, R) if a.roles_min_present is None else a.roles_min_present, 8 if a.roles_iterations is None else a.roles_iterations,
                       3 if a.roles_lines is None else a.roles_lines)
        if not (2 <= R <= 10 and 2 <= a.roles_set[1] <= R and 1 <= a.roles_set[2] <= 32 and 2 <= a.roles_set[3] <= min(4, R)):
            ap.error("--roles: R within 2 .. 10, M within 2 .. R, T within 1 .. 32 and L within 2 .. min(4, R)")
    if a.pass_options and not a.processed:
        ap.error("--pass-options works on the processed table: it needs --processed")
    if (a.pass_options_grid is not None or a.pass_options_pictures) and not a.pass_options:
        ap.error("--pass-options-grid and --pass-options-pictures add to the pass options: they need --pass-options")
    if a.physical and not a.processed:
        ap.error("--physical works on the processed table: it needs --processed")
    if a.physical_rows and not a.physical:
        ap.error("--physical-rows adds to the physical report: it needs --physical")
    if a.physical_edges is not None:
        if not a.physical:
            ap.error("--physical-edges sets the zones of the physical report: it needs --physical")
        try:
            a.physical_edges = [float(tok) for tok in a.physical_edges.split(",")]
        except ValueError:
            a.physical_edges = []
        if len(a.physical_edges) != 4 or not all(0.0 < x < float("inf") for x in a.physical_edges) or any(x >= y for x, y in zip(a.physical_edges, a.physical_edges[1:])):
            ap.error("--physical-edges takes four positive speeds in m/s, strictly ascending")
    if a.shape and not a.processed:
        ap.error("--shape works on the processed table: it needs --processed")
    if a.minimap_hulls is not None:
        if not (a.minimap or a.minimap_control):
            ap.error("--minimap-hulls draws into the minimap: it needs --minimap")
        try:
            a.minimap_hulls = int(a.minimap_hulls)
        except ValueError:
            a.minimap_hulls = 0
        if not 1 <= a.minimap_hulls <= 8:
            ap.error("--minimap-hulls takes a half width of 1 .. 8 pixels")
    if a.occupancy and not a.processed:
        ap.error("--occupancy works on the processed table: it needs --processed")
    if a.occupancy_pictures and not a.occupancy:
        ap.error("--occupancy-pictures draws the occupancy maps: it needs --occupancy")
    if (a.minimap_trails is not None or a.minimap_passes) and not (a.minimap or a.minimap_control):
        ap.error("--minimap-trails and --minimap-passes draw into the minimap: they need --minimap")
    if a.minimap_trails is not None:
        try:
            a.minimap_trails = a.fps if a.minimap_trails == "fps" else int(a.minimap_trails)
        except ValueError:
            a.minimap_trails = 0
        if a.minimap_trails < 1:
            ap.error("--minimap-trails takes a number of rows of at least 1")
    if (a.trajectory is not None or a.pass_pictures) and not a.processed:
        ap.error("--trajectory and --pass-pictures work on the processed table: they need --processed")
    if a.trajectory is not None:
        try:
            a.trajectory = [tok if tok == "ball" else int(tok) for tok in a.trajectory.split(",")]
        except ValueError:
            ap.error("--trajectory takes a comma list of ids or `ball`")
    if a.possession and not a.processed:
        ap.error("--possession works on the processed table: it needs --processed")
    if a.minimap and not a.processed:
        ap.error("--minimap draws the processed table: it needs --processed")
    if (a.kinematics or a.minimap_control or a.control_grid) and not a.processed:
        ap.error("--kinematics, --minimap-control and --control-grid work on the processed table: they need --processed")
    a.smooth_set = {k: v for k, v in (("window", a.smooth_window), ("degree", a.smooth_degree), ("outlier_k", a.smooth_outlier), ("outlier_floor", a.smooth_floor),
                                      ("ball_window", a.smooth_ball)) if v is not None}
    a.stabilise_set = {k: v for k, v in (("window", a.stabilise_window), ("degree", a.stabilise_degree), ("model", a.stabilise_model), ("min_voters", a.stabilise_min_voters),
                                         ("iterations", a.stabilise_iterations), ("trim_k", a.stabilise_trim), ("floor", a.stabilise_floor)) if v is not None}
    if a.stabilise and not a.processed:
        ap.error("--stabilise works on the processed table: it needs --processed")
    if (a.stabilise_set or a.stabilise_rows) and not a.stabilise:
        ap.error("--stabilise-window, --stabilise-degree, --stabilise-model, --stabilise-min-voters, --stabilise-iterations, --stabilise-trim, --stabilise-floor and "
                 "--stabilise-rows set the stabilisation: they need --stabilise")
    if a.stabilise:
        from . import stabilise as stb
        try:
            stb.resolve(a.fps, **a.stabilise_set)
        except ValueError as e:
            ap.error(str(e))
    a.lines_set = {k: v for k, v in (("rounds", a.refine_lines_rounds), ("radius", a.refine_lines_radius), ("radius_min", a.refine_lines_min_radius),
                                     ("max_shift", a.refine_lines_max_shift), ("tau", a.refine_lines_contrast), ("model", a.refine_lines_model)) if v is not None}
    if (a.lines_set or a.refine_lines_rows) and not a.refine_lines:
        ap.error("--refine-lines-rounds, --refine-lines-radius, --refine-lines-min-radius, --refine-lines-max-shift, --refine-lines-contrast, --refine-lines-model and "
                 "--refine-lines-rows set the line registration: they need --refine-lines")
    if a.refine_lines:
        r0, r1 = a.lines_set.get("radius", 2.5), a.lines_set.get("radius_min", 0.5)
        if not 0 <= a.lines_set.get("rounds", 5) <= 16:
            ap.error("--refine-lines-rounds takes 0 .. 16")
        if not (1.0 / 2048 <= r1 <= r0 <= 8.0):
            ap.error("--refine-lines-radius and --refine-lines-min-radius take metres with 1 / 2048 <= min radius <= radius <= 8")
        if not 0.0 <= a.lines_set.get("max_shift", 3.0) <= 1024.0:
            ap.error("--refine-lines-max-shift takes 0 .. 1024 metres")
        if not 1 <= a.lines_set.get("tau", 200) <= 1020:
            ap.error("--refine-lines-contrast takes 1 .. 1020")
    a.ball_flights_set = {k: v for k, v in (("max_rows", a.ball_flights_rows), ("noise", a.ball_flights_noise), ("penalty", a.ball_flights_penalty),
                                            ("spike", a.ball_flights_spike), ("kick_dv", a.ball_flights_kick), ("shot_speed", a.ball_flights_shot)) if v is not None}
    if a.ball_flights and not a.processed:
        ap.error("--ball-flights works on the processed table: it needs --processed")
    if (a.ball_flights_set or a.ball_flights_cells) and not a.ball_flights:
        ap.error("--ball-flights-rows, --ball-flights-noise, --ball-flights-penalty, --ball-flights-spike, --ball-flights-kick, --ball-flights-shot and "
                 "--ball-flights-cells set the ball flights: they need --ball-flights")
    if a.ball_flights:
        from . import flights as _flights
        try:
            _flights.resolve(a.fps, **a.ball_flights_set)
        except ValueError as e:
            ap.error(str(e))
    if a.goal_view and not a.processed:
        ap.error("--goal-view works on the processed table: it needs --processed")
    if (a.goal_view_direction or a.goal_view_cells or a.goal_view_map) and not a.goal_view:
        ap.error("--goal-view-direction, --goal-view-cells and --goal-view-map set the goal view: they need --goal-view")
    if (a.goal_view_grid is not None or a.goal_view_team is not None) and not a.goal_view_map:
        ap.error("--goal-view-grid and --goal-view-team set the map: they need --goal-view-map")
    if a.goal_view:
        a.goal_view_direction = a.goal_view_direction or "offside"
        if a.goal_view_direction == "offside" and not a.offside:
            ap.error("--goal-view takes the attacking direction from the offside result: it needs --offside, or --goal-view-direction right / left")
        a.goal_view_team = a.goal_view_team or ("possession" if a.possession else "0")
        if a.goal_view_map and a.goal_view_team == "possession" and not a.possession:
            ap.error("--goal-view-team possession needs --possession")
    if a.smooth_tracks and not a.processed:
        ap.error("--smooth-tracks works on the processed table: it needs --processed")
    if (a.smooth_set or a.smooth_rows) and not a.smooth_tracks:
        ap.error("--smooth-window, --smooth-degree, --smooth-outlier, --smooth-floor, --smooth-ball and --smooth-rows set the track smoothing: they need --smooth-tracks")
    if a.smooth_tracks:
        from . import smooth as sm
        try:
            sm.resolve(a.fps, **a.smooth_set)
        except ValueError as e:
            ap.error(str(e))
    if a.merge_ids and not a.processed:
        ap.error("--merge-ids works on the processed table: it needs --processed")
    if a.minimap_control and a.minimap_voronoi:
        ap.error("--minimap-control and --minimap-voronoi draw in the same slot: choose one")

    from . import synth
    from .coordinate_model import CoordinateModel
    frames = np.load(a.clip) if a.clip else synth.clip(a.seed, a.frames)
    if a.native_fps is not None:
        from . import io as eio
        frames, _ = eio.read_clip(frames, a.native_fps, a.fps)
    n, h, w, _ = frames.shape
    hs = ys = None
    if a.keypoint_weights:
        hs = load_state_dict(a.keypoint_weights)
    if a.detector_weights:
        ys = load_state_dict(a.detector_weights)
    if (hs is None or ys is None) and not a.synthetic_weights:
        raise SystemExit("no checkpoints given: pass --keypoint-weights and --detector-weights (the reference's keypoints_main.pth / detector_*.pt, cm.py:54-59), "
                         "or --synthetic-weights to run seeded random networks on purpose")
    if hs is None or ys is None:
        print("WARNING: running with seeded RANDOM network weights: the output has the reference's schema but no meaning", flush=True)
    model = CoordinateModel(frame_hw=(h, w), detector=a.detector, det_imgsz=a.imgsz, letterbox=a.letterbox, batch=min(a.batch, max(n, 1)),
                            precision=a.precision, detector_precision=a.detector_precision, allow_saturation=a.allow_saturation, device=a.device, seed=a.seed,
                            hrnet_state_dict=hs, detector_state_dict=ys, tracker=a.tracker, camera_motion=a.camera_motion or False,
                            reid=a.reid, reid_state_dict=({("reid." + k): v for k, v in load_state_dict(a.reid_weights).items()} if a.reid_weights else None))
    shot_meta, found_shots, first_frame = {}, None, 0
    if a.shots or a.trim_to_shot is not None:
        from . import shots as _shots
        found = model.shots(frames, a.fps, **shot_set)
        found_shots = found.shots
        shot_meta["shots"] = len(found.shots)
        if a.shots:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, "shots.json"), "w") as f:
                json.dump(_shots.to_json(found), f)
        if a.trim_to_shot is not None:
            k = _shots.longest_usable(found) if a.trim_to_shot == "auto" else a.trim_to_shot
            if k is None:
                raise SystemExit(f"error: --trim-to-shot auto: none of the clip's {len(found.shots)} shots looks at the pitch for at least {found.params['min_len']} frames")
            if k >= len(found.shots):
                raise SystemExit(f"error: --trim-to-shot {k}: the clip has {len(found.shots)} shots")
            first, count = int(found.shots[k]["first"]), int(found.shots[k]["count"])
            shot_meta["trim"] = {"shot": int(k), "first": first, "count": count}
            frames = frames[first:first + count]
            n, first_frame = count, first
    t0 = time.perf_counter()
    nh, nk = (a.fps, a.fps) if a.every_frame else (a.num_homography, a.num_keypoint_detection)
    from . import lib
    try:
        coordinates = model.get_coordinates(frames, a.fps, num_homography=nh, num_keypoint_detection=nk, verbose=False, calibration=a.calibration)
    except lib.EagleRangeError as e:
        raise SystemExit(f"error: {e}\n(re-run with --precision f32, or with --allow-saturation to accept clipped activations)")
    if a.refine_lines:
        coordinates, lines = model.refine_lines(frames, coordinates, **a.lines_set)
    dt = time.perf_counter() - t0
    sat = model.handle.timings()
    if sat.sat_events:
        print(f"WARNING: {sat.sat_events} activation stores in {sat.sat_frames} frame(s) were clipped at +-4094 (f32s range); the affected frames are not fp32-grade", flush=True)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "raw_coordinates.json"), "w") as f:
        json.dump(coordinates, f, default=float)
    if a.refine_lines:
        from . import linefit
        with open(os.path.join(a.out, "lines.json"), "w") as f:
            json.dump(linefit.to_json(lines, rows=a.refine_lines_rows), f)
    meta = {"fps": a.fps, "frames": n, "seconds": dt, "note": "team_mapping needs the post-processor (out of scope)"}
    if a.processed:
        from . import postprocess
        from .annotate import write_y4m
        from .processor import Processor
        team_kw = dict(team_method="cluster", team_params=a.team_set) if a.team_method == "cluster" else {}
        if a.stabilise:                                                    # directly after the table is built, before --smooth-tracks and every other stage
            team_kw.update(stabilise=True, stabilise_params=a.stabilise_set)
        if a.smooth_tracks:                                                # directly after the table is built, before every other stage
            team_kw.update(smooth_tracks=True, smooth_params=a.smooth_set)
        if a.ball_track:
            from . import balltrack as bt
            cuts = bt.cuts_of_shots(found_shots, first_frame, n) if found_shots is not None else None
            table, team_mapping = Processor(model).process_data(frames, coordinates, a.fps, smooth=a.smooth, merge_ids=a.merge_ids, ball_track=a.ball_track_set or True, cuts=cuts,
                                                                **team_kw)
            with open(os.path.join(a.out, "ball_track.json"), "w") as f:
                json.dump(bt.to_json(*table.ball_track, rows=a.ball_track_rows), f)
        else:
            table, team_mapping = Processor(model).process_data(frames, coordinates, a.fps, smooth=a.smooth, merge_ids=a.merge_ids, **team_kw)
        team_report = table.team_report                                    # None: the colours' rule, or a clip without records (no teams.json then)
        if team_report is not None:
            from . import kits
            with open(os.path.join(a.out, "teams.json"), "w") as f:
                json.dump(kits.to_json(team_report), f)
        merges = table.merges
        if a.stabilise:
            from . import stabilise as stb
            with open(os.path.join(a.out, "stabilise.json"), "w") as f:
                json.dump(stb.to_json(table.stabilise_report, rows=a.stabilise_rows), f)
        if a.smooth_tracks:
            from . import smooth as sm
            with open(os.path.join(a.out, "smooth.json"), "w") as f:
                json.dump(sm.to_json(table.smooth_report, rows=a.smooth_rows), f)
        with open(os.path.join(a.out, "raw_data.json"), "w") as f:
            json.dump(postprocess.json_rows(postprocess.raw_data_rows(table)), f)
        with open(os.path.join(a.out, "processed_data.json"), "w") as f:
            json.dump(postprocess.json_rows(postprocess.format_data(table)), f)
        if a.annotated:
            write_y4m(os.path.join(a.out, "annotated.y4m"), model.annotate(frames, coordinates, team_mapping, out_format="i420", table=table), a.fps)
        if a.kinematics or a.minimap_control or a.control_grid:
            from . import control as ct
            kin = ct.kinematics(model.handle, table, a.fps, keep=a.smooth_tracks)      # after --smooth-tracks: the fits' velocities
            if a.kinematics:
                with open(os.path.join(a.out, "kinematics.json"), "w") as f:
                    json.dump({"fps": a.fps, "players": kin["players"]}, f)
            if a.control_grid:
                grids, share = ct.control(model.handle, table, a.control_grid)
                np.save(os.path.join(a.out, "control.npy"), grids)
                with open(os.path.join(a.out, "control_share.json"), "w") as f:
                    json.dump({"cells_per_metre": a.control_grid, "frames": [int(r) for r in table.rows], "team0_share": [float(v) for v in share]}, f)
        have_vel = bool(a.kinematics or a.minimap_control or a.control_grid or a.smooth_tracks)
        if (a.physical or a.pass_options) and not have_vel:
            model.handle.velocities(table, a.fps)
        if a.physical:
            from . import physical as ph
            d = ph.physical(model.handle, table, a.fps, **({} if a.physical_edges is None else {"zone_edges": a.physical_edges}))
            with open(os.path.join(a.out, "physical.json"), "w") as f:
                json.dump(ph.to_json(d, rows=a.physical_rows), f)
        if a.possession:
            from . import possession as po
            with open(os.path.join(a.out, "possession.json"), "w") as f:
                json.dump(po.to_json(po.possession(model.handle, table, a.fps)), f)
        if a.ball_flights:                                                 # reads the table's ball column as it is; changes nothing in the table
            from . import balltrack as bt, flights as fls
            cuts = bt.cuts_of_shots(found_shots, first_frame, n) if found_shots is not None else None
            res = fls.ball_flights(model.handle, table, a.fps, cuts, **a.ball_flights_set)
            with open(os.path.join(a.out, "ball_flights.json"), "w") as f:
                json.dump(fls.to_json(res, events=model.handle.events(table) if a.possession else None, cells=a.ball_flights_cells), f)
        if a.occupancy:
            from . import occupancy as oc
            occ = oc.occupancy(model.handle, table, a.fps, a.occupancy_grid, a.occupancy_sigma)
            np.save(os.path.join(a.out, "occupancy.npy"), occ["grids"])
            with open(os.path.join(a.out, "occupancy.json"), "w") as f:
                json.dump(oc.to_json(occ), f)
            if a.occupancy_pictures:
                for name, img in oc.pictures(model.handle, table, occ, a.minimap_scale):
                    oc.write_ppm(os.path.join(a.out, "occupancy_%s.ppm" % name), img)
        if a.shape:
            from . import shape as sh
            with open(os.path.join(a.out, "shape.json"), "w") as f:
                json.dump(sh.to_json(sh.shape(model.handle, table)), f)
        elif a.minimap_hulls is not None:
            model.handle.team_shape(table)
        if a.roles:
            from . import roles as ro
            with open(os.path.join(a.out, "roles.json"), "w") as f:
                json.dump(ro.to_json(ro.roles(model.handle, table, *a.roles_set, per_row=a.roles_rows)), f)
        if (a.minimap_passes or a.pass_pictures or a.pass_options) and not a.possession:
            model.handle.possession(table, lib.possession_params(a.fps))
        if a.pass_options:
            from . import occupancy as oc, options as op
            want_grid = a.pass_options_grid is not None or a.pass_options_pictures
            res = op.pass_options(model.handle, table, a.pass_options_grid or 1, grids=want_grid)
            with open(os.path.join(a.out, "pass_options.json"), "w") as f:
                json.dump(op.to_json(res, table), f)
            if a.pass_options_grid is not None:
                np.save(os.path.join(a.out, "pass_options.npy"), res["grids"])
            if a.pass_options_pictures:
                for k, img in op.pictures(model.handle, table, res, a.minimap_scale):
                    oc.write_ppm(os.path.join(a.out, "pass_options_%d.ppm" % k), img)
        if a.space:
            from . import space as spc
            with open(os.path.join(a.out, "space.json"), "w") as f:
                json.dump(spc.to_json(spc.space(model.handle, table, a.space_set[0], True, a.space_set[1], per_row=a.space_rows)), f)
            if a.space_map:
                np.save(os.path.join(a.out, "space.npy"), model.handle.space_grids(table, lib.space_params(a.space_set[0], 1, a.space_set[1])))
        if a.offside:
            from . import offside as ofs
            with open(os.path.join(a.out, "offside.json"), "w") as f:
                json.dump(ofs.to_json(ofs.offside(model.handle, table, a.offside_set[0], a.offside_set[1], not a.offside_no_assumed_keeper, per_row=a.offside_rows)), f)
        if a.goal_view:                                                    # after the offside, possession and flight results it joins; changes nothing in the table
            from . import goalview as gv
            try:
                res = gv.goal_view(model.handle, table, grid=a.goal_view_map, direction={"offside": 0, "right": 1, "left": 2}[a.goal_view_direction],
                                   group={"0": 0, "1": 1, "possession": -1}[a.goal_view_team], cells_per_metre=a.goal_view_grid or 1)
                out = gv.to_json(res, flights=model.handle.ball_flight_values(table)["flights"] if a.ball_flights else None,
                                 events=model.handle.events(table) if a.possession else None, cells=a.goal_view_cells)
            except ValueError as e:                                        # the offside vote settled no direction, or the table has no team mapping
                res, out = None, {"error": str(e)}
            with open(os.path.join(a.out, "goal_view.json"), "w") as f:
                json.dump(out, f)
            if a.goal_view_map and res is not None:
                np.save(os.path.join(a.out, "goal_view.npy"), res["grid"])
        if a.offside_view:
            from . import ground as gr
            pics, info = gr.offside_view(model, frames, coordinates, table, out_format="i420", **a.offside_view_set)
            write_y4m(os.path.join(a.out, "offside_view.y4m"), pics, a.fps)
            with open(os.path.join(a.out, "offside_view.json"), "w") as f:
                json.dump(info, f)
        if a.offside_stills:
            from . import ground as gr, occupancy as oc
            st = {k: v for k, v in a.offside_view_set.items() if k != "team"}
            for k, img, _ in gr.offside_stills(model, frames, coordinates, table, **st):
                oc.write_ppm(os.path.join(a.out, "offside_%d.ppm" % k), img)
        entities = [c for c, k in enumerate(table.columns) if not k["video"] and int(k["kind"]) in (lib.POST_PLAYER, lib.POST_GOALKEEPER, lib.POST_BALL)]
        if a.trajectory is not None:
            from . import minimap as mm
            want = a.trajectory
            cols = [c for c in entities if (("ball" in want) if int(table.columns[c]["kind"]) == lib.POST_BALL else int(table.columns[c]["id"]) in want)]
            mm.trajectory_picture(model.handle, table, cols, None, a.minimap_scale, max_gap=a.fps, path=os.path.join(a.out, "trajectory.ppm"))
        if a.pass_pictures:
            from . import minimap as mm
            for k, e in enumerate(model.handle.events(table)):
                if int(e["kind"]) == lib.EVENT_PASS:
                    mm.pass_picture(model.handle, table, k, a.minimap_scale, path=os.path.join(a.out, "pass_%d.ppm" % k))
        if a.minimap or a.minimap_control:
            from .minimap import minimap
            tp = lib.trail_params(window=a.minimap_trails or a.fps, max_gap=a.fps, pass_hold=a.fps)      # (None: no trails, the window is not used)
            write_y4m(os.path.join(a.out, "minimap.y4m"), minimap(model.handle, table, a.minimap_scale, voronoi=a.minimap_voronoi, pixel_format="i420",
                                                                   control=lib.control_params(min(4, a.minimap_scale)) if a.minimap_control else None,
                                                                   trails=entities if a.minimap_trails is not None else None, passes=a.minimap_passes,
                                                                   owner=a.minimap_passes, trail_params=tp, hulls=a.minimap_hulls), a.fps)
        table.close()
        meta = {"fps": a.fps, "frames": n, "seconds": dt, "team_mapping": team_mapping}
        if a.merge_ids:
            meta["merges"] = merges
        if a.stabilise:
            meta["stabilised"] = True                                      # each kept frame's common motion was removed (stabilise.json)
        if a.smooth_tracks:
            meta["positions"] = "smoothed"                                 # the table's pitch positions are the fits' (smooth.json)
        if a.ball_flights:
            meta["ball_flights"] = True                                    # ball_flights.json
        if a.goal_view:
            meta["goal_view"] = True                                       # goal_view.json
        if a.ball_track:
            meta["ball"] = "ball_track"                                    # the table's ball is the tracked one (ball_track.json)
        if team_report is not None:
            meta["teams"] = "cluster"                                      # the mapping is the clustering's (teams.json)
    elif a.annotated:
        from .annotate import write_y4m
        from .processor import Processor
        if a.team_method == "cluster":
            from . import kits
            pr = Processor(model)
            team_mapping = pr.get_team_mapping(frames, coordinates, method="cluster", **a.team_set)
            with open(os.path.join(a.out, "teams.json"), "w") as f:
                json.dump(kits.to_json(pr.team_report), f)
        else:
            team_mapping = Processor(model).get_team_mapping(frames, coordinates)
        write_y4m(os.path.join(a.out, "annotated.y4m"), model.annotate(frames, coordinates, team_mapping, out_format="i420"), a.fps)
        meta = {"fps": a.fps, "frames": n, "seconds": dt, "team_mapping": team_mapping}
        if a.team_method == "cluster":
            meta["teams"] = "cluster"
    if a.topview:
        from . import topview as tv
        from .annotate import write_y4m
        write_y4m(os.path.join(a.out, "topview.y4m"), model.topview(frames, coordinates, carry=a.topview_carry, out_format="i420", **a.topview_set), a.fps)
        if a.topview_mosaic:
            res = model.mosaic(frames, coordinates, carry=a.topview_carry, **a.mosaic_set)
            tv.write_ppm(os.path.join(a.out, "topview_mosaic.ppm"), res.mosaic)
            np.save(os.path.join(a.out, "topview_count.npy"), res.cnt)
            with open(os.path.join(a.out, "topview.json"), "w") as f:
                json.dump(tv.to_json(res, carry=a.topview_carry, suspect=tv.SUSPECT if a.topview_suspect is None else a.topview_suspect), f)
    meta.update(shot_meta)
    if a.refine_lines:
        meta["homography"] = "refined"                                     # the accepted frames were projected with the refined matrix (lines.json)
    with open(os.path.join(a.out, "metadata.json"), "w") as f:
        json.dump(meta, f, default=str)
    print(f"{n} frames in {dt:.3f} s -> {os.path.join(a.out, 'raw_coordinates.json')}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
