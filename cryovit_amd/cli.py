"""``cryovit`` command line for the script-level flows (mirror of
``/root/reference/src/cryovit/cli/{cli,dino_cli,train_cli,infer_cli,eval_cli}.py``): same command names, arguments, options and defaults.

    python -m cryovit_amd.cli preprocess <tomograms> <result-folder> <normalisation>
    python -m cryovit_amd.cli features <tomograms> <result-folder> [--batch-size 64] [--visualize] [--normalize <normalisation>]
    python -m cryovit_amd.cli train <train-data> <train-labels> <label-key> --labels A [--labels B ...] [--val-data ..] [--val-labels ..]
                                    [--name ..] [--result-folder ..] [--ckpt x.model|x.pt] [--num-epochs 50]
    python -m cryovit_amd.cli infer <tomograms> --model x.model [--result-folder DIR] [--threshold 0.5]
                                    [--instances <measurements>]
    python -m cryovit_amd.cli evaluate <test-data> <test-labels> x.model --labels A [--labels B ...] [--result-folder DIR] [-v]
                                       [--boundary [--boundary-mode slices|3d] [--boundary-tolerance T ...]]
                                       [--instance-metrics [--instance-mode slices|3d] [--instance-connectivity 6|26]
                                                           [--instance-min-size N] [--instance-iou T ...]]
    python -m cryovit_amd.cli instances <predictions> --label NAME [--result-folder DIR] <measurements>
                                        [--distance-to NAME] [--contacts-with NAME] [--distance-to-folder DIR] [--contact-radius R]

    <normalisation>: [--bin K] [--bin-z KZ] [--clip sigma|percentile|minmax|range] [--sigma S] [--percentile LO HI] [--range LO HI]
                     [--per-slice] [--invert]
    <measurements>: [--close-radius R] [--fill-holes 3d|slices] [--open-radius R]
                    [--min-size N] [--connectivity 6|26] [--split-radius R [--split-min-core N]] [--morphology] [--shape]
                    [--skeleton [--skeleton-end-radius R]] [--thickness] [--mesh [--mesh-smooth N] [--mesh-format ply|stl]]
                    [--curvature [--curvature-radius R]]
                    [--pick [--pick-spacing S] [--pick-radius R] [--pick-offset V] [--pick-scale F] [--pick-seed N]]
                    [--trace [--trace-spacing S] [--trace-window H] [--trace-min-length L] [--trace-scale F] [--trace-angpix A]]
                    [--extract picks|filaments [--extract-box B] [--extract-orient aligned|none] [--extract-profile-radius R]
                     [--extract-align N [--align-angles T] [--align-shift S] [--align-radius R] [--align-height Z] [--align-reference F.mrc]]]

``preprocess`` (build extension) turns raw reconstructions (int8 / uint8 / int16 / uint16 / float MRC, TIFF or HDF5, as IMOD or AreTomo
write them) into the uint8 tomograms every other command expects, on the GPU: bin, clip, rescale to [0, 255]
(``run.preprocess.PreprocessOptions``); ``features --normalize`` does the same on the fly and feeds the encoder from the device.
``train`` fits the CryoVIT head on the GPU (HIP backward, fused AdamW; ``run/train_model.py``) and writes the ``.model`` file that
``infer`` and ``evaluate`` load; UNet3D and SAM2 training are not built.  Extra options, marked "build extension",
replace the network fetch of the encoder weights or add what the reference leaves to the user: ``instances`` (and
``infer --instances``) labels the connected instances of a predicted mask on the GPU, tabulates their size and position and
measures them.  The measurement options are declared once, below, for both commands; each is a field of
``analysis.instances.InstanceOptions``, which says what it computes and writes.  ``--close-radius``, ``--fill-holes`` and
``--open-radius`` clean the mask on the GPU before it is labelled, in that order (``analysis.cleanup.CleanupOptions``): the file gains
``<label>_cleaned`` and the CSV ``added_voxels``.  ``--curvature`` maps the mean curvature of the membrane at the scale
``--curvature-radius`` (``analysis.curvature.CurvatureOptions``).  ``--pick`` places positions for subtomogram averaging on every
instance's membrane, no two of one instance closer than ``--pick-spacing`` voxels, each with the membrane normal, and writes them as
``picks/<tomo>_<label>.csv`` and a RELION ``.star`` (``analysis.picks.PickOptions``).  ``--trace`` follows every instance's skeleton
(it implies ``--skeleton`` and uses ``--skeleton-end-radius``) and splits it into branches between ends and junctions, and rings: how many
filaments there are, how long and how straight each is, which meet where, and positions every ``--trace-spacing`` voxels along them with
the tangent, as ``filaments/<tomo>_<label>_branches.csv``, ``.csv`` and a helical RELION ``.star`` (``analysis.filaments.TraceOptions``).
``--extract picks`` (it implies ``--pick``) and ``--extract filaments`` (it implies ``--trace``) cut a box of ``--extract-box`` voxels out
of the uint8 tomogram around every such position, rotated so that its z axis is the membrane normal or the filament tangent, and write
``subtomograms/<tomo>_<label>.mrcs``, their average, a RELION ``.star`` and the density profile along that axis per instance
(``analysis.subtomograms.ExtractOptions``).  ``--extract-align N`` then refines every box about that axis, the in-plane angle and the
shift along it, and writes the aligned stack, its average, a STAR file and the alignment tables (``analysis.alignment.AlignOptions``).
``--distance-to NAME`` adds the gap to another
label's mask and the voxels in contact with it; ``--contacts-with NAME`` says which instance touches which: every instance gains
``partners_<NAME>``, and ``contacts/<tomo>_<label>_<NAME>.csv`` lists per pair (instance, nearest instance of NAME within
``--contact-radius``) the voxels in contact, the narrowest gap and where it is.
"""

from __future__ import annotations

import logging
import math
from pathlib import Path
from typing import Annotated, Optional

import typer
from typer import Argument, Option

cli = typer.Typer(add_completion=False, no_args_is_help=True, pretty_exceptions_show_locals=False)


@cli.callback()
def callback():
    """CryoViT's command line interface (MI355X build): feature extraction, training, inference and evaluation."""


def _load_encoder(encoder: Optional[str], checkpoint: Optional[str], synthetic_seed: Optional[int]):
    """The encoder of the "build extension" options, or None when none of them is given."""
    ov = _encoder_overrides(encoder, checkpoint, synthetic_seed)
    if not ov:
        return None
    from cryovit_amd.config import compose
    from cryovit_amd.models.encoder import load_encoder

    cfg = compose("dino_features", [])
    return load_encoder(ov.get("name", "dinov2_vitg14_reg"), model_dir=cfg.model_dir, checkpoint=ov.get("checkpoint"),
                        synthetic_seed=ov.get("synthetic_seed"))


def _checked(ok, message: str):
    """A typer callback that turns a value down with ``message`` unless ``ok(value)``: a usage error while the arguments are parsed,
    before anything that labels or infers is imported."""
    def check(value):
        if value is not None and not ok(value):
            raise typer.BadParameter(message)
        return value

    return check


def _non_negative(what: str):
    return _checked(lambda v: v >= 0, f"{what} must be >= 0 (voxels)")


def _each(check):
    """``check`` on every value of a repeatable option."""
    def check_all(values):
        for v in values or ():
            check(v)
        return values

    return check_all


# The measurement options `infer` and `instances` share, each declared once; analysis.instances.InstanceOptions has the full account.
_MIN_SIZE_HELP = "drop instances of fewer voxels (with infer: with --instances)"
_CONNECTIVITY_HELP = "6 (faces) or 26 (faces, edges and corners) (with infer: with --instances)"
_MORPHOLOGY_HELP = ("add surface voxels, inscribed radius and deepest voxel per instance (exact distance map on the GPU; voxels; with "
                    "infer: needs --instances)")
_SPLIT_RADIUS_HELP = ("split instances that touch over a neck: cores deeper than this many voxels are grown back inside their "
                      "instance; the CSV gains the column component (voxels, >= 0; with infer: needs --instances)")
_SPLIT_MIN_CORE_HELP = "with --split-radius, ignore cores of fewer voxels"
_SHAPE_HELP = ("add surface area (Crofton estimate over 13 directions), sphericity, Euler number (under --connectivity), principal-axis "
               "lengths, elongation and major-axis direction per instance as the last CSV columns (voxels; with infer: needs --instances)")
_SKELETON_HELP = ("thin every instance to its centreline on the GPU: write it as <label>_skeleton and add skeleton_voxels, "
                  "skeleton_length, skeleton_ends, skeleton_branches and skeleton_rms_radius after the shape columns (voxels; with "
                  "infer: needs --instances)")
_SKELETON_END_RADIUS_HELP = ("with --skeleton, keep a line's end once it lies this deep inside the instance: 1 keeps a spur per "
                             "surface bump, larger values drop them; structures thinner than this shrink to a point or a ring (voxels, >= 0)")
_THICKNESS_HELP = ("map the local thickness on the GPU (at every voxel the diameter of the largest ball inside the structure that "
                   "contains it, as Fiji's Local Thickness): write it as <label>_thickness and add thickness_mean, thickness_std, "
                   "thickness_min and thickness_max as the last CSV columns.  The values are diameters between voxel centres of the "
                   "background, so a slab of n voxels reads about n + 1 (the discrete bias of Fiji's Local Thickness); for an instance "
                   "that touches no other, thickness_max equals 2 * inscribed_radius; touching pieces after --split-radius are "
                   "measured as their union (voxels; with infer: needs --instances)")

_MESH_HELP = ("write the surface of the labelled mask as a triangle mesh, built on the GPU (marching tetrahedra, one watertight, "
              "consistently oriented mesh with shared vertices): <result>/meshes/<tomo>_<label>.ply, and add mesh_triangles, mesh_area "
              "and mesh_volume as the last CSV columns.  Midpoint vertices: the raw staircase mesh over-reads the area of slanted "
              "surfaces, quote the smoothed one (--mesh-smooth).  14-connectivity: parts that meet only across another diagonal show "
              "as two shells.  Touching pieces after --split-radius are meshed as their union, and mesh_volume is not for them.  The "
              "volume's border is treated as background, so every surface closes (voxels; with infer: needs --instances)")
_MESH_SMOOTH_HELP = ("with --mesh, relax the mesh by N pairs of integer Taubin steps (lambda 0.5, mu -0.53) before it is measured and "
                     "written; 0 keeps the raw mesh, about 10 gives a surface to quote beside surface_area of --shape")
_MESH_FORMAT_HELP = ("with --mesh, the file format: ply (binary, shared vertices, an instance id per face) or stl (binary, the id in "
                     "the attribute word, saturated at 65535)")
_CLOSE_RADIUS_HELP = ("before labelling, close the mask by a ball of this radius on the GPU (seals pinholes and one-voxel cracks; "
                      "applied first; writes <label>_cleaned and the CSV column added_voxels; voxels, >= 0; with infer: needs --instances)")
_FILL_HOLES_HELP = ("before labelling, fill the background that is not connected to the border, on the GPU: 3d = enclosed cavities "
                    "of the volume, slices = every z-slice on its own, as Fiji's Fill Holes (for structures the missing wedge leaves "
                    "open along z); applied after --close-radius (with infer: needs --instances)")
_OPEN_RADIUS_HELP = ("before labelling, open the mask by a ball of this radius on the GPU (removes spurs and specks; applied last; "
                     "voxels, >= 0; with infer: needs --instances)")
_BOUNDARY_HELP = ("score the predicted boundary against the annotated one on the GPU: after the model's metrics every CSV row gains hd95 "
                  "(95th-percentile Hausdorff distance), hd, assd (average symmetric surface distance), nsd_<t> (surface Dice at each "
                  "--boundary-tolerance) and the surface / unmatched voxel counts (voxels; exact distance maps)")
_BOUNDARY_MODE_HELP = ("with --boundary: slices = every fully annotated z-slice scored as an image of its own (sparse CryoVIT labels), "
                       "3d = the whole volume, which must hold no ignored (-1) voxel")
_BOUNDARY_TOLERANCE_HELP = "with --boundary: a tolerance of the surface Dice, column nsd_<T>; repeatable (voxels, >= 0)"
_INSTANCE_METRICS_HELP = ("score the prediction object by object on the GPU: the connected instances of the predicted mask against those "
                          "of the annotation.  After the model's metrics (and the boundary columns) every CSV row gains inst_f1_<T> "
                          "(detection F1, a pair matched iff IoU > T, per --instance-iou), at IoU > 0.5 inst_tp, inst_precision, "
                          "inst_recall, inst_sq (mean IoU of the matches) and inst_pq (panoptic quality), over the annotated voxels "
                          "inst_ari (adjusted Rand index), inst_vi_split and inst_vi_merge (variation of information, bits), and the "
                          "counts inst_pred, inst_true, inst_merged_true, inst_split_true; results/<name>/instances/<sample>_<tomo>.csv "
                          "lists every annotated instance with its best predicted partner, then the unmatched predicted ones")
_INSTANCE_MODE_HELP = ("with --instance-metrics: slices = every fully annotated z-slice an image of its own, its instances the "
                       "components in the plane (sparse CryoVIT labels), 3d = the components of the whole volume, which must hold no "
                       "ignored (-1) voxel; with --boundary it must agree with --boundary-mode")
_INSTANCE_CONNECTIVITY_HELP = "with --instance-metrics: 6 (faces; 4 in a slice) or 26 (faces, edges and corners; 8 in a slice)"
_INSTANCE_MIN_SIZE_HELP = "with --instance-metrics: instances of fewer voxels are background, predicted and annotated alike"
_INSTANCE_IOU_HELP = "with --instance-metrics: an IoU threshold of the detection F1, column inst_f1_<T>; repeatable (in [0.5, 1))"
_CURVATURE_HELP = ("map the mean curvature of the membrane on the GPU (ball-volume integral invariant: the share of a ball centred "
                   "on the surface that lies inside the object; exact integer arithmetic): write it as <label>_curvature (1/voxel, NaN "
                   "off the surface) and add curvature_mean, curvature_std, curvature_min, curvature_max, convex_fraction, "
                   "curvature_voxels and curvature_unscored as the last CSV columns; with --mesh the PLY gains a curvature per vertex "
                   "(not with --mesh-format stl).  Positive is convex, negative concave (a cavity wall, an invagination); surface "
                   "voxels within the ball radius + 1 of the volume's border are not scored; touching pieces after --split-radius are "
                   "scored as their union (with infer: needs --instances)")
_CURVATURE_RADIUS_HELP = ("with --curvature, the radius of the ball: the scale at which the surface is read.  Larger is quieter (the "
                          "per-voxel noise falls with 1/R^2) and blurs features smaller than R (voxels, an integer in 2..16)")
_PICK_HELP = ("place evenly spaced positions on the membrane of every instance on the GPU, each with the membrane normal: the particle "
              "positions of subtomogram averaging.  Writes <result>/picks/<tomo>_<label>.csv (every pick: instance id, voxel, position, "
              "outward normal, Euler angles, the ball's moment) and .star (a RELION data_particles loop of the oriented picks: "
              "_rlnCoordinateX/Y/Z, _rlnAngleRot/Tilt/Psi with the particle's z axis along the normal) and adds picks and "
              "picks_unoriented as the last CSV columns.  The CSV normals are the authoritative orientation (with infer: needs "
              "--instances)")
_PICK_SPACING_HELP = ("with --pick, the least distance between two picks of one instance, centre to centre; every surface voxel then "
                      "has a pick of its instance closer than this (voxels, an integer in 2..16)")
_PICK_RADIUS_HELP = ("with --pick, the radius of the ball the normal is read from; picks lie at least this far from the volume's "
                     "border (voxels, an integer in 2..16)")
_PICK_OFFSET_HELP = ("with --pick, move every oriented pick this far along its outward normal before it is written; negative moves "
                     "into the object (voxels)")
_PICK_SCALE_HELP = ("with --pick, write coordinates of a volume this many times finer: (q + 0.5) * F - 0.5, which undoes "
                    "preprocess --bin F (> 0)")
_PICK_SEED_HELP = "with --pick, the seed of the pseudo-random order the candidates are taken in (0 .. 2^32 - 1); same seed, same picks"
_TRACE_HELP = ("trace the skeleton of every instance into filaments on the GPU (implies --skeleton; uses --skeleton-end-radius): branches "
               "between ends and junctions, and closed rings, each with its length, chord, tortuosity and radius, and positions along "
               "them with the tangent: where to cut segments for helical averaging.  Writes <result>/filaments/<tomo>_<label>_branches.csv "
               "(every branch), <tomo>_<label>.csv (every position: branch, instance id, arc length, position, tangent, Euler angles, "
               "radius) and .star (a RELION data_particles loop with _rlnHelicalTubeID = the branch and _rlnHelicalTrackLengthAngst, the "
               "particle's z axis along the filament), the dataset <label>_filaments (the branch number of every path voxel, -1 on "
               "ends and junction voxels) and adds filament_branches, filament_rings, filament_junctions, filament_points, "
               "filament_length, filament_longest and filament_tortuosity after the skeleton's CSV columns.  The polarity of a branch "
               "is arbitrary and the CSV tangents are the authoritative orientation (with infer: needs --instances)")
_TRACE_SPACING_HELP = "with --trace, the arc length between two positions of a branch, the first at its start (voxels, >= 1)"
_TRACE_WINDOW_HELP = ("with --trace, the tangent at a position is the direction between the points this far before and after it along "
                      "the branch; larger is smoother and blurs bends shorter than it (voxels, >= 1)")
_TRACE_MIN_LENGTH_HELP = "with --trace, branches shorter than this get no positions; they stay in the branch CSV and the columns (voxels, >= 0)"
_TRACE_SCALE_HELP = ("with --trace, write coordinates of a volume this many times finer: (q + 0.5) * F - 0.5, which undoes "
                     "preprocess --bin F (> 0)")
_TRACE_ANGPIX_HELP = "with --trace, Angstrom per voxel of that finer volume, for _rlnHelicalTrackLengthAngst = arc * F * A (> 0)"
_EXT = "build extension: "

MinSize = Annotated[int, Option(min=0, help=_EXT + _MIN_SIZE_HELP)]
Connectivity = Annotated[int, Option(callback=_checked(lambda v: v in (6, 26), "connectivity must be 6 (faces) or 26 (faces, edges and corners)"),
                                     help=_EXT + _CONNECTIVITY_HELP)]
Morphology = Annotated[bool, Option("--morphology", help=_EXT + _MORPHOLOGY_HELP)]
SplitRadius = Annotated[Optional[float], Option(callback=_non_negative("split radius"), help=_EXT + _SPLIT_RADIUS_HELP)]
SplitMinCore = Annotated[int, Option(min=0, help=_EXT + _SPLIT_MIN_CORE_HELP)]
Shape = Annotated[bool, Option("--shape", help=_EXT + _SHAPE_HELP)]
Skeleton = Annotated[bool, Option("--skeleton", help=_EXT + _SKELETON_HELP)]
SkeletonEndRadius = Annotated[float, Option(callback=_non_negative("skeleton end radius"), help=_EXT + _SKELETON_END_RADIUS_HELP)]
Thickness = Annotated[bool, Option("--thickness", help=_EXT + _THICKNESS_HELP)]
Mesh = Annotated[bool, Option("--mesh", help=_EXT + _MESH_HELP)]
MeshSmooth = Annotated[int, Option("--mesh-smooth", callback=_checked(lambda v: v >= 0, "mesh smoothing iterations must be >= 0"),
                                   help=_EXT + _MESH_SMOOTH_HELP)]
MeshFormat = Annotated[str, Option("--mesh-format", callback=_checked(lambda v: v in ("ply", "stl"), "mesh format must be ply or stl"),
                                   help=_EXT + _MESH_FORMAT_HELP)]
CloseRadius = Annotated[Optional[float], Option(callback=_non_negative("close radius"), help=_EXT + _CLOSE_RADIUS_HELP)]
FillHoles = Annotated[Optional[str], Option(callback=_checked(lambda v: v in ("3d", "slices"), "fill holes must be 3d or slices"),
                                            help=_EXT + _FILL_HOLES_HELP)]
OpenRadius = Annotated[Optional[float], Option(callback=_non_negative("open radius"), help=_EXT + _OPEN_RADIUS_HELP)]
Curvature = Annotated[bool, Option("--curvature", help=_EXT + _CURVATURE_HELP)]
CurvatureRadius = Annotated[int, Option("--curvature-radius", callback=_checked(lambda v: 2 <= v <= 16, "curvature radius must lie in 2..16 (voxels)"),
                                        help=_EXT + _CURVATURE_RADIUS_HELP)]

# The normalisation options `preprocess` and `features --normalize` share; run.preprocess.PreprocessOptions has the full account.
Bin = Annotated[int, Option("--bin", min=1, max=8, help=_EXT + "sum the raw volume over boxes of this size in y and x before anything else (1..8)")]
BinZ = Annotated[Optional[int], Option("--bin-z", min=1, max=8, help=_EXT + "box size in z (1..8)", show_default="--bin")]
Clip = Annotated[str, Option("--clip", callback=_checked(lambda v: v in ("sigma", "percentile", "minmax", "range"),
                                                         "clip must be sigma, percentile, minmax or range"),
                             help=_EXT + "where 0 and 255 lie: mean -+ --sigma standard deviations, the --percentile pair, the extremes, or --range")]
Sigma = Annotated[float, Option("--sigma", callback=_checked(lambda v: v > 0, "sigma must be > 0"), help=_EXT + "with --clip sigma: standard deviations either side of the mean")]
Percentile = Annotated[tuple[float, float], Option("--percentile", help=_EXT + "with --clip percentile: the low and the high percentile (exact, lower nearest rank)")]
Range = Annotated[Optional[tuple[float, float]], Option("--range", help=_EXT + "with --clip range: the raw values that map to 0 and 255", show_default=False)]
PerSlice = Annotated[bool, Option("--per-slice", help=_EXT + "limits per z-slice instead of one pair for the volume")]
Invert = Annotated[bool, Option("--invert", help=_EXT + "store 255 - q")]


def _preprocess_options(bin_, bin_z, clip, sigma, percentile, range_, per_slice, invert):
    """The PreprocessOptions of the shared options; what ``validate`` refuses is a usage error."""
    from cryovit_amd.run.preprocess import PreprocessOptions

    try:
        return PreprocessOptions(bin=bin_, bin_z=bin_z, clip=clip, sigma=sigma, percentiles=tuple(percentile),
                                 range=tuple(range_) if range_ is not None else None, per_slice=per_slice, invert=invert).validate()
    except ValueError as e:
        raise typer.BadParameter(str(e)) from None

Pick = Annotated[bool, Option("--pick", help=_EXT + _PICK_HELP)]
PickSpacing = Annotated[int, Option("--pick-spacing", callback=_checked(lambda v: 2 <= v <= 16, "pick spacing must lie in 2..16 (voxels)"),
                                    help=_EXT + _PICK_SPACING_HELP)]
PickRadius = Annotated[int, Option("--pick-radius", callback=_checked(lambda v: 2 <= v <= 16, "pick radius must lie in 2..16 (voxels)"),
                                   help=_EXT + _PICK_RADIUS_HELP)]
PickOffset = Annotated[float, Option("--pick-offset", callback=_checked(lambda v: math.isfinite(v), "pick offset must be finite (voxels)"),
                                     help=_EXT + _PICK_OFFSET_HELP)]
PickScale = Annotated[float, Option("--pick-scale", callback=_checked(lambda v: math.isfinite(v) and v > 0, "pick scale must be finite and > 0"),
                                    help=_EXT + _PICK_SCALE_HELP)]
PickSeed = Annotated[int, Option("--pick-seed", callback=_checked(lambda v: 0 <= v < 2**32, "pick seed must lie in 0..2^32 - 1"),
                                 help=_EXT + _PICK_SEED_HELP)]



def _trace_checked(name: str, ok, rule: str):
    """As ``_checked``, in the words of ``analysis.filaments.TraceOptions.validate``."""
    def check(value):
        if value is not None and not (math.isfinite(value) and ok(value)):
            raise typer.BadParameter(f"{name} must be a finite number {rule}, got {value!r}")
        return value

    return check


Trace = Annotated[bool, Option("--trace", help=_EXT + _TRACE_HELP)]
TraceSpacing = Annotated[float, Option("--trace-spacing", callback=_trace_checked("trace_spacing", lambda v: v >= 1, ">= 1"),
                                       help=_EXT + _TRACE_SPACING_HELP)]
TraceWindow = Annotated[float, Option("--trace-window", callback=_trace_checked("trace_window", lambda v: v >= 1, ">= 1"),
                                      help=_EXT + _TRACE_WINDOW_HELP)]
TraceMinLength = Annotated[float, Option("--trace-min-length", callback=_trace_checked("trace_min_length", lambda v: v >= 0, ">= 0"),
                                         help=_EXT + _TRACE_MIN_LENGTH_HELP)]
TraceScale = Annotated[float, Option("--trace-scale", callback=_trace_checked("trace_scale", lambda v: v > 0, "> 0"),
                                     help=_EXT + _TRACE_SCALE_HELP)]
TraceAngpix = Annotated[float, Option("--trace-angpix", callback=_trace_checked("trace_angpix", lambda v: v > 0, "> 0"),
                                      help=_EXT + _TRACE_ANGPIX_HELP)]

_EXTRACT_HELP = ("cut oriented subtomograms out of the uint8 tomogram on the GPU, at the picks (picks: implies --pick) or at the "
                 "positions along the filaments (filaments: implies --trace): a box around each, rotated so that its z axis is the membrane "
                 "normal or the filament tangent, trilinear.  Writes <result>/subtomograms/<tomo>_<label>.mrcs (a stack of float32 "
                 "volumes), _average.mrc, .star (the pick or helical columns and _rlnImageName) and _profiles.csv (the mean density "
                 "per box z slab and instance) and adds extracted and extract_skipped as the last CSV columns.  The file's data must be "
                 "the uint8 tomogram that `cryovit preprocess` makes (with infer: needs --instances)")
Extract = Annotated[Optional[str], Option("--extract", callback=_checked(lambda v: v in ("picks", "filaments"), "extract must be picks or filaments"),
                                          help=_EXT + _EXTRACT_HELP)]
ExtractBox = Annotated[int, Option("--extract-box", callback=_checked(lambda v: 8 <= v <= 128 and v % 2 == 0,
                                                                      "extract box must be even and lie in 8..128 (voxels)"),
                                   help=_EXT + "with --extract, the edge of the box (voxels, an even integer in 8..128)")]
ExtractOrient = Annotated[str, Option("--extract-orient", callback=_checked(lambda v: v in ("aligned", "none"), "extract orient must be aligned or none"),
                                      help=_EXT + "with --extract, aligned: box z along the normal / tangent, angles written as 0; none: "
                                                  "axis-parallel boxes, the angles stay priors in the STAR file")]
ExtractProfileRadius = Annotated[Optional[float], Option("--extract-profile-radius",
                                                         callback=_checked(lambda v: math.isfinite(v) and v >= 0,
                                                                           "extract profile radius must be finite and >= 0 (voxels)"),
                                                         help=_EXT + "with --extract, the radius of the disc around the axis that the density "
                                                                     "profile averages over (voxels, >= 0)",
                                                         show_default="a quarter of the box")]
ExtractAlign = Annotated[Optional[int], Option("--extract-align", callback=_checked(lambda v: 1 <= v <= 20, "extract align must lie in 1..20 (iterations)"),
                                               help=_EXT + "with --extract (--extract-orient aligned), refine every box about its axis on the GPU for this "
                                                           "many iterations (1..20): the in-plane angle and the shift along the axis against the "
                                                           "average of the boxes as aligned so far.  Writes _aligned.mrcs (every box cut again "
                                                           "with its refined frame), _aligned_average.mrc, _aligned.star, _alignment.csv (psi, shift, "
                                                           "score, refined centre and angles per particle) and _alignment_log.csv beside the boxes and "
                                                           "adds aligned and align_score as the last CSV columns", show_default="off")]
AlignAngles = Annotated[int, Option("--align-angles", callback=_checked(lambda v: v in (32, 64, 128), "align angles must be 32, 64 or 128"),
                                    help=_EXT + "with --extract-align, the angular samples T (32, 64 or 128); the step is 360/T degrees")]
AlignShift = Annotated[int, Option("--align-shift", callback=_checked(lambda v: 0 <= v <= 8, "align shift must lie in 0..8 (voxels)"),
                                   help=_EXT + "with --extract-align, the search range along the axis (voxels, 0..8)")]
AlignRadius = Annotated[Optional[int], Option("--align-radius", callback=_checked(lambda v: v >= 1, "align radius must be >= 1 (voxels)"),
                                              help=_EXT + "with --extract-align, the rings 1..R around the axis are scored (1 <= R <= B/2 - 1)",
                                              show_default="B/2 - 2")]
AlignHeight = Annotated[Optional[int], Option("--align-height", callback=_checked(lambda v: v >= 0, "align height must be >= 0 (voxels)"),
                                              help=_EXT + "with --extract-align, the slabs B/2 - Z .. B/2 + Z of the reference are scored "
                                                          "(Z >= 0, Z + shift <= B/2 - 1)", show_default="B/2 - 1 - shift")]
AlignReference = Annotated[Optional[str], Option("--align-reference", help=_EXT + "with --extract-align, a float32 MRC volume of B^3 voxels in grey "
                                                                                  "levels to start from", show_default="the best particle against the plain average")]


def _align_options(extract, extract_box, extract_orient, extract_align, align_angles, align_shift, align_radius, align_height, align_reference) -> dict:
    """The keyword arguments of the alignment for ``run_inference`` and ``label_file``: none without --extract-align; a usage error for
    what ``analysis.alignment.AlignOptions`` refuses."""
    if extract_align is None:
        return {}
    from cryovit_amd.analysis.alignment import AlignOptions
    from cryovit_amd.analysis.subtomograms import ExtractOptions

    given = dict(extract_align=extract_align, align_angles=align_angles, align_shift=align_shift, align_radius=align_radius,
                 align_height=align_height, align_reference=align_reference)
    try:
        AlignOptions(**given).validate(ExtractOptions(extract=extract, extract_box=extract_box, extract_orient=extract_orient).validate())
    except ValueError as err:
        raise typer.BadParameter(str(err), param_hint="--extract-align") from err
    return given


# infer measures nothing without --instances: asking for one of these without it is a usage error
_NEEDS_INSTANCES = ("morphology", "shape", "skeleton", "split_radius", "thickness", "mesh", "close_radius", "fill_holes", "open_radius",
                    "curvature", "pick", "trace", "extract")


def _refuse_stl_curvature(curvature: bool, mesh: bool, mesh_format: str) -> None:
    """A usage error for --curvature with an STL mesh: the format has no per-vertex data to hold the values."""
    if curvature and mesh and mesh_format == "stl":
        raise typer.BadParameter("--curvature colours the mesh per vertex, which an STL file cannot hold: use --mesh-format ply",
                                 param_hint="--mesh-format")


def _encoder_overrides(encoder: Optional[str], checkpoint: Optional[str], synthetic_seed: Optional[int]) -> dict:
    out = {}
    if encoder:
        out["name"] = encoder
    if checkpoint:
        out["checkpoint"] = checkpoint
    if synthetic_seed is not None:
        out["synthetic_seed"] = synthetic_seed
    return out


@cli.command(name="features", no_args_is_help=True)
def features(
    tomograms: Annotated[str, Argument(help="Path to the folder or .txt file containing the tomograms to process.")],
    result_folder: Annotated[str, Argument(help="Path to the folder where the DINO features will be saved.")],
    batch_size: Annotated[int, Option(min=1, help="Batch size for DINO feature extraction.")] = 64,
    visualize: Annotated[bool, Option("--visualize", "-v", help="Save PCA visualization of DINO features? This will increase the runtime.")] = False,
    encoder: Annotated[Optional[str], Option(help="build extension: encoder name (default dinov2_vitg14_reg)")] = None,
    checkpoint: Annotated[Optional[str], Option(help="build extension: local DINOv2 state_dict file")] = None,
    synthetic_seed: Annotated[Optional[int], Option(help="build extension: seeded random encoder weights")] = None,
    normalize: Annotated[bool, Option("--normalize", help=_EXT + "the files hold raw intensities: normalise each to uint8 on the GPU first (the options below, as `preprocess`); the result feeds the encoder from the device and is written as the output's data")] = False,
    bin_: Bin = 1,
    bin_z: BinZ = None,
    clip: Clip = "sigma",
    sigma: Sigma = 3.0,
    percentile: Percentile = (0.5, 99.5),
    range_: Range = None,
    per_slice: PerSlice = False,
    invert: Invert = False,
):
    """Compute high-level features using DINOv2 for a set of tomograms."""
    given = dict(bin_=bin_, bin_z=bin_z, clip=clip, sigma=sigma, percentile=percentile, range_=range_, per_slice=per_slice, invert=invert)
    if not normalize and given != dict(bin_=1, bin_z=None, clip="sigma", sigma=3.0, percentile=(0.5, 99.5), range_=None, per_slice=False, invert=False):
        raise typer.BadParameter("the normalisation options need --normalize", param_hint="--normalize")
    options = _preprocess_options(**given) if normalize else None
    from cryovit_amd.run.dino_features import run_dino
    from cryovit_amd.utils import load_files_from_path

    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    tomograms_path, result_path = Path(tomograms), Path(result_folder)
    assert tomograms_path.exists(), "Tomograms path does not exist."
    result_path.mkdir(parents=True, exist_ok=True)
    extra = {"normalize": options} if normalize else {}  # without the flag the call is what it always was
    run_dino(load_files_from_path(tomograms_path), result_path, batch_size=batch_size, visualize=visualize,
             encoder=_encoder_overrides(encoder, checkpoint, synthetic_seed), **extra)


@cli.command(name="preprocess", no_args_is_help=True)
def preprocess(
    tomograms: Annotated[str, Argument(help="Path to the folder or .txt file containing the raw tomograms.")],
    result_folder: Annotated[str, Argument(help="Path to the folder where the uint8 tomograms and preprocess.csv will be saved.")],
    bin_: Bin = 1,
    bin_z: BinZ = None,
    clip: Clip = "sigma",
    sigma: Sigma = 3.0,
    percentile: Percentile = (0.5, 99.5),
    range_: Range = None,
    per_slice: PerSlice = False,
    invert: Invert = False,
):
    """Bin, clip and 8-bit-normalise raw tomograms on the GPU (build extension)."""
    options = _preprocess_options(bin_, bin_z, clip, sigma, percentile, range_, per_slice, invert)
    tomograms_path, result_path = Path(tomograms), Path(result_folder)
    assert tomograms_path.exists(), "Tomograms path does not exist."
    from cryovit_amd.run.preprocess import run_preprocess
    from cryovit_amd.run.sharding import select_device
    from cryovit_amd.utils import load_files_from_path

    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    try:
        device = select_device()
    except RuntimeError as e:  # no device: say so and write nothing
        typer.echo(f"Error: {e}", err=True)
        raise typer.Exit(1) from None
    result_path.mkdir(parents=True, exist_ok=True)
    for out in run_preprocess(load_files_from_path(tomograms_path), result_path, options, device=device):
        logging.info("Wrote %s", out)


@cli.command(name="train", no_args_is_help=True)
def train(
    train_data: Annotated[str, Argument(help="Path to the folder or .txt file containing the training tomograms.")],
    train_labels: Annotated[str, Argument(help="Path to the folder or .txt file containing the training labels.")],
    labels: Annotated[list[str], Option(help="List of available label names in ascending-value order.")],
    label_key: Annotated[str, Argument(help="Label key to train on. Must be one of the provided labels.")],
    validation_data: Annotated[Optional[str], Option("--validation-data", "--val-data", show_default=False,
                                                     help="Path to the folder or .txt file containing the validation tomograms.")] = None,
    validation_labels: Annotated[Optional[str], Option("--validation-labels", "--val-labels", show_default=False,
                                                       help="Path to the folder or .txt file containing the validation labels.")] = None,
    name: Annotated[Optional[str], Option(show_default=False, help="Name to identify the model. If not provided, a random name will be generated.")] = None,
    model: Annotated[str, Option(help="The type of model to train (this build trains cryovit only).")] = "cryovit",
    result_folder: Annotated[Optional[str], Option(help="Path to the folder where the trained model will be saved.",
                                                   show_default="the current working directory")] = None,
    ckpt: Annotated[Optional[str], Option(help="Path to a pre-trained .model file, or .pt weights (a state_dict) to fine-tune a model from.")] = None,
    num_epochs: Annotated[int, Option(min=1, help="Number of training epochs.")] = 50,
    encoder: Annotated[Optional[str], Option(help="build extension: encode files without dino_features on the fly with this encoder")] = None,
    checkpoint: Annotated[Optional[str], Option(help="build extension: local DINOv2 state_dict file")] = None,
    synthetic_seed: Annotated[Optional[int], Option(help="build extension: seeded random encoder weights")] = None,
):
    """Train a segmentation model on given training data and labels."""
    import random
    import string

    if model.lower() != "cryovit":
        raise typer.BadParameter(f"only cryovit can be trained here: this command does not train a {model} model (unet3d trains through "
                                 "run.train_model.run_training(model_type=ModelType.UNET3D); sam2 is inference-only).", param_hint="--model")
    train_path, label_path = Path(train_data), Path(train_labels)
    ckpt_path = Path(ckpt) if ckpt is not None else None
    val_path = Path(validation_data) if validation_data else None
    val_label_path = Path(validation_labels) if validation_labels else None
    result_path = Path(result_folder) if result_folder else Path.cwd()
    model_name = name or "cryovit_" + "".join(random.choices(string.ascii_uppercase + string.digits, k=6))  # (utils.id_generator of the reference)
    assert train_path.exists(), "Training data path does not exist."
    assert label_path.exists(), "Training labels path does not exist."
    if val_path is not None:
        assert val_path.exists(), "Validation data path does not exist."
        assert val_label_path is not None and val_label_path.exists(), "Validation data provided but validation labels path does not exist."
    if ckpt_path is not None:
        assert ckpt_path.exists(), "Checkpoint path does not exist."
    assert label_key in labels, f"The label key {label_key} is not in the provided labels."
    from cryovit_amd.run.train_model import run_training
    from cryovit_amd.types import ModelType
    from cryovit_amd.utils import load_files_from_path

    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    train_files, train_label_files = load_files_from_path(train_path), load_files_from_path(label_path)
    val_files = load_files_from_path(val_path) if val_path is not None else None
    val_label_files = load_files_from_path(val_label_path) if val_label_path is not None else None
    result_path.mkdir(parents=True, exist_ok=True)
    run_training(train_files, train_label_files, labels, ModelType.CRYOVIT, model_name, label_key, result_path, val_files, val_label_files,
                 num_epochs=num_epochs, ckpt_path=ckpt_path, encoder=_load_encoder(encoder, checkpoint, synthetic_seed))


@cli.command(name="infer", no_args_is_help=True)
def infer(
    tomograms: Annotated[str, Argument(help="Path to the folder or .txt file containing the tomograms to process.")],
    model: Annotated[str, Option(help="Path to the .model file containing the pre-trained model.")],
    result_folder: Annotated[Optional[str], Option(help="Path to the folder where the inference results will be saved.")] = None,
    threshold: Annotated[float, Option(min=0.0, max=1.0, help="Threshold for binary segmentation.")] = 0.5,
    encoder: Annotated[Optional[str], Option(help="build extension: encode files without dino_features on the fly with this encoder")] = None,
    checkpoint: Annotated[Optional[str], Option(help="build extension: local DINOv2 state_dict file")] = None,
    synthetic_seed: Annotated[Optional[int], Option(help="build extension: seeded random encoder weights")] = None,
    instances: Annotated[bool, Option("--instances", help="build extension: also label the connected instances of each mask on the GPU (<label>_instances dataset and instances/<tomogram>_<label>.csv)")] = False,
    min_size: MinSize = 0,
    connectivity: Connectivity = 26,
    morphology: Morphology = False,
    split_radius: SplitRadius = None,
    split_min_core: SplitMinCore = 0,
    shape: Shape = False,
    skeleton: Skeleton = False,
    skeleton_end_radius: SkeletonEndRadius = 2.0,
    thickness: Thickness = False,
    mesh: Mesh = False,
    mesh_smooth: MeshSmooth = 0,
    mesh_format: MeshFormat = "ply",
    close_radius: CloseRadius = None,
    fill_holes: FillHoles = None,
    open_radius: OpenRadius = None,
    curvature: Curvature = False,
    curvature_radius: CurvatureRadius = 5,
    pick: Pick = False,
    pick_spacing: PickSpacing = 8,
    pick_radius: PickRadius = 5,
    pick_offset: PickOffset = 0.0,
    pick_scale: PickScale = 1.0,
    pick_seed: PickSeed = 0,
    trace: Trace = False,
    trace_spacing: TraceSpacing = 8.0,
    trace_window: TraceWindow = 4.0,
    trace_min_length: TraceMinLength = 0.0,
    trace_scale: TraceScale = 1.0,
    trace_angpix: TraceAngpix = 1.0,
    extract: Extract = None,
    extract_box: ExtractBox = 32,
    extract_orient: ExtractOrient = "aligned",
    extract_profile_radius: ExtractProfileRadius = None,
    extract_align: ExtractAlign = None,
    align_angles: AlignAngles = 64,
    align_shift: AlignShift = 2,
    align_radius: AlignRadius = None,
    align_height: AlignHeight = None,
    align_reference: AlignReference = None,
):
    """Segment tomograms using a pre-trained model."""
    measurements = dict(min_size=min_size, connectivity=connectivity, morphology=morphology, split_radius=split_radius,
                        split_min_core=split_min_core, shape=shape, skeleton=skeleton, skeleton_end_radius=skeleton_end_radius,
                        thickness=thickness, mesh=mesh, mesh_smooth=mesh_smooth, mesh_format=mesh_format,
                        close_radius=close_radius, fill_holes=fill_holes, open_radius=open_radius,
                        curvature=curvature, curvature_radius=curvature_radius,
                        pick=pick, pick_spacing=pick_spacing, pick_radius=pick_radius, pick_offset=pick_offset, pick_scale=pick_scale,
                        pick_seed=pick_seed, trace=trace, trace_spacing=trace_spacing, trace_window=trace_window,
                        trace_min_length=trace_min_length, trace_scale=trace_scale, trace_angpix=trace_angpix,
                        extract=extract, extract_box=extract_box, extract_orient=extract_orient,
                        extract_profile_radius=extract_profile_radius)
    _refuse_stl_curvature(curvature, mesh, mesh_format)
    measurements |= _align_options(extract, extract_box, extract_orient, extract_align, align_angles, align_shift, align_radius, align_height,
                                   align_reference)
    for name in _NEEDS_INSTANCES:
        value = measurements[name]  # a flag that is off is False, a radius that is not given None; a radius of 0 is given
        if not instances and value is not False and value is not None:
            flag = "--" + name.replace("_", "-")
            raise typer.BadParameter(f"{flag} needs --instances", param_hint=flag)
    from cryovit_amd.run.infer_model import run_inference
    from cryovit_amd.utils import load_files_from_path

    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    tomograms_path, model_path = Path(tomograms), Path(model)
    result_path = Path(result_folder) if result_folder else Path.cwd() / "predictions"
    assert tomograms_path.exists(), "Tomograms path does not exist."
    assert model_path.exists() and model_path.suffix == ".model", "Model path does not exist or is not a .model file."
    result_path.mkdir(parents=True, exist_ok=True)
    run_inference(load_files_from_path(tomograms_path), model_path, result_path, threshold=threshold,
                  encoder=_load_encoder(encoder, checkpoint, synthetic_seed), instances=instances, **measurements)


@cli.command(name="instances", no_args_is_help=True)
def instances_cmd(
    predictions: Annotated[str, Argument(help="Path to the folder or .txt file containing prediction files written by `infer`.")],
    label: Annotated[str, Option(help="build extension: label name; the <label>_preds dataset of every file is labelled.")],
    min_size: MinSize = 0,
    connectivity: Connectivity = 26,
    result_folder: Annotated[Optional[str], Option(help="build extension: folder for the labelled files and instances/*.csv.",
                                                   show_default="the folder of the predictions (files are updated in place)")] = None,
    morphology: Morphology = False,
    distance_to: Annotated[Optional[str], Option(help="build extension: another label NAME; add the gap to <NAME>_preds and the voxels in contact with it (voxels)")] = None,
    distance_to_folder: Annotated[Optional[str], Option(help="build extension: folder whose <same stem>.hdf holds <NAME>_preds (for --contacts-with also <NAME>_instances) when the prediction file itself does not; serves --distance-to and --contacts-with")] = None,
    contact_radius: Annotated[float, Option(callback=_non_negative("contact radius"), help="build extension: with --distance-to or --contacts-with, voxels within this distance of the other label count as contact (voxels, >= 0)")] = 1.0,
    contacts_with: Annotated[Optional[str], Option(help="build extension: another label NAME; write contacts/<tomo>_<label>_<NAME>.csv, one row per pair of an instance and the instance of NAME nearest to some of its voxels within --contact-radius (voxels in contact, gap, where), and add partners_<NAME> per instance")] = None,
    split_radius: SplitRadius = None,
    split_min_core: SplitMinCore = 0,
    shape: Shape = False,
    skeleton: Skeleton = False,
    skeleton_end_radius: SkeletonEndRadius = 2.0,
    thickness: Thickness = False,
    mesh: Mesh = False,
    mesh_smooth: MeshSmooth = 0,
    mesh_format: MeshFormat = "ply",
    close_radius: CloseRadius = None,
    fill_holes: FillHoles = None,
    open_radius: OpenRadius = None,
    curvature: Curvature = False,
    curvature_radius: CurvatureRadius = 5,
    pick: Pick = False,
    pick_spacing: PickSpacing = 8,
    pick_radius: PickRadius = 5,
    pick_offset: PickOffset = 0.0,
    pick_scale: PickScale = 1.0,
    pick_seed: PickSeed = 0,
    trace: Trace = False,
    trace_spacing: TraceSpacing = 8.0,
    trace_window: TraceWindow = 4.0,
    trace_min_length: TraceMinLength = 0.0,
    trace_scale: TraceScale = 1.0,
    trace_angpix: TraceAngpix = 1.0,
    extract: Extract = None,
    extract_box: ExtractBox = 32,
    extract_orient: ExtractOrient = "aligned",
    extract_profile_radius: ExtractProfileRadius = None,
    extract_align: ExtractAlign = None,
    align_angles: AlignAngles = 64,
    align_shift: AlignShift = 2,
    align_radius: AlignRadius = None,
    align_height: AlignHeight = None,
    align_reference: AlignReference = None,
):
    """Label and measure the connected instances of existing predictions (build extension)."""
    _refuse_stl_curvature(curvature, mesh, mesh_format)
    aligning = _align_options(extract, extract_box, extract_orient, extract_align, align_angles, align_shift, align_radius, align_height,
                              align_reference)
    from cryovit_amd.analysis.instances import label_file
    from cryovit_amd.utils import load_files_from_path

    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    predictions_path = Path(predictions)
    assert predictions_path.exists(), "Predictions path does not exist."
    for f in load_files_from_path(predictions_path):
        out = label_file(f, label, connectivity=connectivity, min_size=min_size, result_dir=result_folder, morphology=morphology,
                         distance_to=distance_to, distance_to_dir=distance_to_folder, contact_radius=contact_radius,
                         split_radius=split_radius, split_min_core=split_min_core, contacts_with=contacts_with, shape=shape,
                         skeleton=skeleton, skeleton_end_radius=skeleton_end_radius, thickness=thickness,
                         mesh=mesh, mesh_smooth=mesh_smooth, mesh_format=mesh_format,
                         close_radius=close_radius, fill_holes=fill_holes, open_radius=open_radius,
                         curvature=curvature, curvature_radius=curvature_radius,
                         pick=pick, pick_spacing=pick_spacing, pick_radius=pick_radius, pick_offset=pick_offset, pick_scale=pick_scale,
                         pick_seed=pick_seed, trace=trace, trace_spacing=trace_spacing, trace_window=trace_window,
                         trace_min_length=trace_min_length, trace_scale=trace_scale, trace_angpix=trace_angpix,
                         extract=extract, extract_box=extract_box, extract_orient=extract_orient,
                         extract_profile_radius=extract_profile_radius, **aligning)
        logging.info("Labelled %s", out)


@cli.command(name="evaluate", no_args_is_help=True)
def evaluate(
    test_data: Annotated[str, Argument(help="Path to the folder or .txt file containing the test tomograms.")],
    test_labels: Annotated[str, Argument(help="Path to the folder or .txt file containing the test labels.")],
    labels: Annotated[list[str], Option(help="List of available label names in ascending-value order.")],
    model: Annotated[str, Argument(help="Path to the .model file containing the pre-trained model.")],
    result_folder: Annotated[Optional[str], Option(help="Path to the directory to save the evaluation results. Evaluation metrics will be saved to a .csv file in a folder named 'results' inside the result folder.",
                                                   show_default="the current working directory")] = None,
    visualize: Annotated[bool, Option("--visualize", "-v", help="Save visualizations of model predictions?. This will slightly increase the runtime. Results will be saved in a folder named `predictions` inside the result folder.")] = False,
    encoder: Annotated[Optional[str], Option(help="build extension: encode files without dino_features on the fly with this encoder")] = None,
    checkpoint: Annotated[Optional[str], Option(help="build extension: local DINOv2 state_dict file")] = None,
    synthetic_seed: Annotated[Optional[int], Option(help="build extension: seeded random encoder weights")] = None,
    boundary: Annotated[bool, Option("--boundary", help=_EXT + _BOUNDARY_HELP)] = False,
    boundary_mode: Annotated[str, Option("--boundary-mode", callback=_checked(lambda v: v in ("slices", "3d"), "boundary mode must be slices or 3d"),
                                         help=_EXT + _BOUNDARY_MODE_HELP)] = "slices",
    boundary_tolerance: Annotated[Optional[list[float]], Option("--boundary-tolerance", callback=_each(_non_negative("boundary tolerance")),
                                                                help=_EXT + _BOUNDARY_TOLERANCE_HELP,
                                                                show_default="1 and 2")] = None,
    instance_metrics: Annotated[bool, Option("--instance-metrics", help=_EXT + _INSTANCE_METRICS_HELP)] = False,
    instance_mode: Annotated[Optional[str], Option("--instance-mode", callback=_checked(lambda v: v in ("slices", "3d"), "instance mode must be slices or 3d"),
                                                   help=_EXT + _INSTANCE_MODE_HELP, show_default="slices; with --boundary, --boundary-mode")] = None,
    instance_connectivity: Annotated[int, Option("--instance-connectivity", callback=_checked(lambda v: v in (6, 26), "instance connectivity must be 6 or 26"),
                                                 help=_EXT + _INSTANCE_CONNECTIVITY_HELP)] = 26,
    instance_min_size: Annotated[int, Option("--instance-min-size", callback=_checked(lambda v: v >= 0, "instance min size must be >= 0"),
                                             help=_EXT + _INSTANCE_MIN_SIZE_HELP)] = 0,
    instance_iou: Annotated[Optional[list[float]], Option("--instance-iou", callback=_each(_checked(lambda v: 0.5 <= v < 1.0, "an instance IoU threshold must lie in [0.5, 1)")),
                                                          help=_EXT + _INSTANCE_IOU_HELP, show_default="0.5 and 0.75")] = None,
):
    """Evaluate a pre-trained model on a test dataset."""
    instance_iou = tuple(instance_iou) if instance_iou else (0.5, 0.75)
    if len({f"{t:g}" for t in instance_iou}) != len(instance_iou):
        raise typer.BadParameter(f"the thresholds {list(instance_iou)} give the same column twice", param_hint="--instance-iou")
    if instance_metrics and boundary and instance_mode is not None and instance_mode != boundary_mode:
        raise typer.BadParameter(f"--instance-mode {instance_mode} and --boundary-mode {boundary_mode} would score different regions: give one, or "
                                 "the same value to both", param_hint="--instance-mode")

    from cryovit_amd.run.eval_model import run_evaluation
    from cryovit_amd.utils import load_files_from_path, load_model

    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    test_path, label_path, model_path = Path(test_data), Path(test_labels), Path(model)
    result_path = Path(result_folder) if result_folder else Path.cwd()
    assert test_path.exists(), "Test data path does not exist."
    assert label_path.exists(), "Test labels path does not exist."
    assert model_path.exists() and model_path.suffix == ".model", "Model path does not exist, or is not a .model file."
    _, _, _, label_key = load_model(model_path, load_model=False)
    assert label_key in labels, f"The label key {label_key} used to train the model is not in the provided labels."
    result_path.mkdir(parents=True, exist_ok=True)
    run_evaluation(load_files_from_path(test_path), load_files_from_path(label_path), labels, model_path, result_path,
                   visualize=visualize, encoder=_load_encoder(encoder, checkpoint, synthetic_seed), boundary=boundary,
                   boundary_mode=boundary_mode, boundary_tolerances=tuple(boundary_tolerance) if boundary_tolerance else (1.0, 2.0),
                   instance_metrics=instance_metrics, instance_mode=instance_mode, instance_connectivity=instance_connectivity,
                   instance_min_size=instance_min_size, instance_iou=instance_iou)


if __name__ == "__main__":
    cli()
