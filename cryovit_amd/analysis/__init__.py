"""Quantification of predictions after the model has run: connected instances of a predicted mask, what
its distance maps say about them, the split of instances that touch over a neck, which instance of one label touches
which of another, the shape of each instance (surface area, Euler number, principal axes), its centreline (length, ends, branches)
its local thickness (mean, spread, min, max), the surface mesh of the mask (PLY / STL; triangles, area, volume) and the mean
curvature of its membrane (ball-volume integral invariant; mean, spread, min, max, convex share); evenly spaced positions on
that membrane with its normal, the particle picks of subtomogram averaging (RELION STAR / CSV); the centreline traced into
filaments (branches, junctions, rings; positions with tangents along them as helical STAR / CSV); oriented subtomograms cut out
of the tomogram at either kind of position (MRC stack, average, density profile along the axis) and their alignment about that
axis (in-plane angle and shift against the running average); the
clean-up of the mask before all of that (close, fill holes, open); and, against annotated labels, how far the predicted boundary
lies from the true one (HD95, surface distance, surface Dice) and how well the annotated objects are recovered one by one (detection
F1, panoptic quality, Rand index, split / merge variation of information)."""

from cryovit_amd.analysis.instances import (  # noqa: F401
    INSTANCE_COLUMNS, InstanceOptions, instance_rows, label_and_split, label_file, label_volume, measure, split_volume)
from cryovit_amd.analysis.cleanup import CleanupOptions, clean_mask  # noqa: F401
from cryovit_amd.analysis.distances import (  # noqa: F401
    PAIR_COLUMNS, edt_squared, instance_contacts, instance_morphology, instance_pair_contacts, pair_rows, partner_rows)
from cryovit_amd.analysis.shape import SHAPE_COLUMNS, instance_shape, shape_rows  # noqa: F401
from cryovit_amd.analysis.skeleton import SKELETON_COLUMNS, instance_skeleton, skeleton_rows, skeleton_volume  # noqa: F401
from cryovit_amd.analysis.thickness import THICKNESS_COLUMNS, instance_thickness, thickness_rows, thickness_volume  # noqa: F401
from cryovit_amd.analysis.mesh import MESH_COLUMNS, instance_mesh, mesh_arrays, mesh_rows, write_mesh, write_ply, write_stl  # noqa: F401
from cryovit_amd.analysis.curvature import (  # noqa: F401
    CURVATURE_COLUMNS, CurvatureOptions, curvature_map, curvature_rows, curvature_volume, vertex_curvature)
from cryovit_amd.analysis.picks import (  # noqa: F401
    PICK_COLUMNS, PICK_CSV_COLUMNS, PickOptions, pick_records, pick_rows, pick_table, write_picks_csv, write_star)
from cryovit_amd.analysis.filaments import (  # noqa: F401
    BRANCH_CSV_COLUMNS, FILAMENT_COLUMNS, POINT_CSV_COLUMNS, TraceOptions, branch_records, filament_rows, filament_volume, junction_nodes,
    sample_points, trace_tables, write_branches_csv, write_helical_star, write_points_csv)
from cryovit_amd.analysis.subtomograms import (  # noqa: F401
    EXTRACT_COLUMNS, ExtractOptions, extract_rows, extract_to_files, filament_particles, instance_profiles, particle_frames, particle_table,
    pick_particles, write_particle_star, write_profiles_csv)
from cryovit_amd.analysis.alignment import (  # noqa: F401
    ALIGN_COLUMNS, ALIGNMENT_CSV_COLUMNS, ALIGNMENT_LOG_COLUMNS, AlignOptions, align_particles, align_to_files)
from cryovit_amd.analysis.boundary import (  # noqa: F401
    BOUNDARY_COUNT_COLUMNS, BOUNDARY_DISTANCE_COLUMNS, BOUNDARY_MODES, boundary_columns, boundary_histograms, boundary_scores, check_scored,
    nsd_column)
# (the function instance_scores stays in its module: here the name is the module analysis.instance_scores)
from cryovit_amd.analysis.instance_scores import (  # noqa: F401
    INSTANCE_LIST_COLUMNS, INSTANCE_MODES, OverlapTables, check_instance_options, f1_column, instance_columns, instance_list_rows,
    instance_overlap_tables)
