"""ctypes binding of libshoulder_hip.so (include/shoulder_hip.h).  Fails loudly when the HIP
library is missing -- there is no CPU fallback on the product path."""
import ctypes
import os

import numpy as np

from . import build as _build

GROOVE_ROWS = 330
ANP_MAX_PTS = 4096

STAGE_OBB, STAGE_FULL, STAGE_NECK, STAGE_CANAL, STAGE_PROXIMAL = 1, 2, 4, 8, 16
STAGE_GROOVE, STAGE_ANP, STAGE_DISTAL, STAGE_TE, STAGE_CSYS = 32, 64, 128, 256, 512
STAGE_APPLY = 1024
STAGE_ALL = 0x7FF
UNET_F32, UNET_BF16, UNET_F16, UNET_F32X = 0, 1, 2, 3
BONE_HUMERUS, BONE_PROXIMAL = 0, 1
OPEN_ERROR, OPEN_BRIDGE = 0, 1
OPEN_GAP_DEFAULT = 12.0      # mm, SH_OPEN_GAP_DEFAULT


class Landmarks(ctypes.Structure):
    _fields_ = [
        ("obb_transform", ctypes.c_double * 16),
        ("z_length", ctypes.c_double),
        ("neck_z", ctypes.c_double),
        ("canal_axis", ctypes.c_double * 6),
        ("te_axis", ctypes.c_double * 6),
        ("groove_axis", ctypes.c_double * 6),
        ("bg_theta", ctypes.c_double),
        ("anp_plane_point", ctypes.c_double * 3),
        ("anp_plane_normal", ctypes.c_double * 3),
        ("anp_axis_normal", ctypes.c_double * 6),
        ("anp_axis_central", ctypes.c_double * 6),
        ("csys", ctypes.c_double * 16),
        ("csys_articular", ctypes.c_double * 16),
        ("neckshaft", ctypes.c_double),
        ("retroversion", ctypes.c_double),
        ("radius_curvature", ctypes.c_double),
        ("canal_cutoff", ctypes.c_double * 2),
        ("groove_points", ctypes.c_double * (GROOVE_ROWS * 3)),
        ("anp_points", ctypes.c_double * (ANP_MAX_PTS * 3)),
        ("n_anp", ctypes.c_int32),
        ("n_articular", ctypes.c_int32),
        ("neck_index", ctypes.c_int32),
        ("flipped", ctypes.c_int32),
        ("status", ctypes.c_int32),
        ("side", ctypes.c_int32),
    ]


LANDMARKS_DTYPE = np.dtype([
    ("obb_transform", "<f8", (4, 4)), ("z_length", "<f8"), ("neck_z", "<f8"), ("canal_axis", "<f8", (2, 3)),
    ("te_axis", "<f8", (2, 3)), ("groove_axis", "<f8", (2, 3)), ("bg_theta", "<f8"), ("anp_plane_point", "<f8", (3,)),
    ("anp_plane_normal", "<f8", (3,)), ("anp_axis_normal", "<f8", (2, 3)), ("anp_axis_central", "<f8", (2, 3)),
    ("csys", "<f8", (4, 4)), ("csys_articular", "<f8", (4, 4)), ("neckshaft", "<f8"), ("retroversion", "<f8"), ("radius_curvature", "<f8"), ("canal_cutoff", "<f8", (2,)), ("groove_points", "<f8", (GROOVE_ROWS, 3)), ("anp_points", "<f8", (ANP_MAX_PTS, 3)),
    ("n_anp", "<i4"), ("n_articular", "<i4"), ("neck_index", "<i4"), ("flipped", "<i4"), ("status", "<i4"), ("side", "<i4")])
assert LANDMARKS_DTYPE.itemsize == ctypes.sizeof(Landmarks)


def record_dtype(anp_rows=0):
    """NumPy dtype of the records a run hands out: the full sh_landmarks (anp_rows = 0) or the packed wire format of
    sh_set_record_rows(anp_rows): the fields in front of anp_points, the six trailing int32 fields, then anp_rows point rows."""
    if anp_rows <= 0:
        return LANDMARKS_DTYPE
    names = list(LANDMARKS_DTYPE.names)
    k = names.index("anp_points")
    fields = [(n, LANDMARKS_DTYPE.fields[n][0]) for n in names[:k] + names[k + 1:]] + [("anp_points", "<f8", (int(anp_rows), 3))]
    return np.dtype(fields)


class CutOffset(ctypes.Structure):
    """sh_cut_offset: one planned cut relative to the native anatomic-neck plane (arthroplasty.py:90-175)."""
    _fields_ = [(n, ctypes.c_double) for n in ("retroversion_deg", "neckshaft_deg", "depth_canal_mm", "depth_anp_mm",
                                               "depth_resection_mm", "anterior_mm", "medial_mm")]


CUT_OFFSET_DTYPE = np.dtype([(n, "<f8") for n, _ in CutOffset._fields_])
assert CUT_OFFSET_DTYPE.itemsize == ctypes.sizeof(CutOffset)


class Resection(ctypes.Structure):
    """sh_resection: the measurements of one (humerus, plane) cut."""
    _fields_ = [("plane_point", ctypes.c_double * 3), ("plane_normal", ctypes.c_double * 3), ("head_volume", ctypes.c_double),
                ("head_area", ctypes.c_double), ("head_height", ctypes.c_double), ("cut_area", ctypes.c_double),
                ("cut_perimeter", ctypes.c_double), ("cut_centroid", ctypes.c_double * 3), ("cap_area", ctypes.c_double),
                ("n_loops", ctypes.c_int32), ("n_ring", ctypes.c_int32), ("n_cut_faces", ctypes.c_int32), ("status", ctypes.c_int32)]


RESECTION_DTYPE = np.dtype([
    ("plane_point", "<f8", (3,)), ("plane_normal", "<f8", (3,)), ("head_volume", "<f8"), ("head_area", "<f8"), ("head_height", "<f8"),
    ("cut_area", "<f8"), ("cut_perimeter", "<f8"), ("cut_centroid", "<f8", (3,)), ("cap_area", "<f8"),
    ("n_loops", "<i4"), ("n_ring", "<i4"), ("n_cut_faces", "<i4"), ("status", "<i4")])
assert RESECTION_DTYPE.itemsize == ctypes.sizeof(Resection)


class HeadFit(ctypes.Structure):
    """sh_head_fit: the sphere of the resected head piece and the ellipse of the cut, one (humerus, plane)."""
    _fields_ = [("sphere_center", ctypes.c_double * 3), ("sphere_radius", ctypes.c_double), ("sphere_rms", ctypes.c_double),
                ("cap_height", ctypes.c_double), ("fit_area", ctypes.c_double), ("center_articular", ctypes.c_double * 3),
                ("cut_semi_major", ctypes.c_double), ("cut_semi_minor", ctypes.c_double), ("cut_major_dir", ctypes.c_double * 3),
                ("sphere_status", ctypes.c_int32), ("ring_status", ctypes.c_int32)]


HEAD_FIT_DTYPE = np.dtype([
    ("sphere_center", "<f8", (3,)), ("sphere_radius", "<f8"), ("sphere_rms", "<f8"), ("cap_height", "<f8"), ("fit_area", "<f8"),
    ("center_articular", "<f8", (3,)), ("cut_semi_major", "<f8"), ("cut_semi_minor", "<f8"), ("cut_major_dir", "<f8", (3,)),
    ("sphere_status", "<i4"), ("ring_status", "<i4")])
assert HEAD_FIT_DTYPE.itemsize == ctypes.sizeof(HeadFit)


class ImplantHead(ctypes.Structure):
    """sh_implant_head: radius of curvature and thickness of one catalogue head."""
    _fields_ = [("radius", ctypes.c_double), ("thickness", ctypes.c_double)]


IMPLANT_HEAD_DTYPE = np.dtype([("radius", "<f8"), ("thickness", "<f8")])
SEAT_CUT_CENTROID, SEAT_SPHERE_AXIS, SEAT_MAX_HEADS = 0, 1, 64


class Seat(ctypes.Structure):
    """sh_seat: how one implant head sits on one (humerus, plane) cut."""
    _fields_ = [("base_radius", ctypes.c_double), ("seat_center", ctypes.c_double * 3), ("covered_area", ctypes.c_double),
                ("coverage", ctypes.c_double), ("overhang_area", ctypes.c_double), ("uncovered_area", ctypes.c_double),
                ("rim_min", ctypes.c_double), ("rim_max", ctypes.c_double), ("max_overhang", ctypes.c_double),
                ("max_uncovered", ctypes.c_double), ("overhang_dir", ctypes.c_double * 3), ("uncovered_dir", ctypes.c_double * 3),
                ("implant_center", ctypes.c_double * 3), ("cor_shift", ctypes.c_double * 3), ("cor_shift_articular", ctypes.c_double * 3),
                ("surface_rms", ctypes.c_double), ("center_inside", ctypes.c_int32), ("status", ctypes.c_int32)]


SEAT_DTYPE = np.dtype([
    ("base_radius", "<f8"), ("seat_center", "<f8", (3,)), ("covered_area", "<f8"), ("coverage", "<f8"), ("overhang_area", "<f8"),
    ("uncovered_area", "<f8"), ("rim_min", "<f8"), ("rim_max", "<f8"), ("max_overhang", "<f8"), ("max_uncovered", "<f8"),
    ("overhang_dir", "<f8", (3,)), ("uncovered_dir", "<f8", (3,)), ("implant_center", "<f8", (3,)), ("cor_shift", "<f8", (3,)),
    ("cor_shift_articular", "<f8", (3,)), ("surface_rms", "<f8"), ("center_inside", "<i4"), ("status", "<i4")])
assert SEAT_DTYPE.itemsize == ctypes.sizeof(Seat) and IMPLANT_HEAD_DTYPE.itemsize == ctypes.sizeof(ImplantHead)


class CanalGrid(ctypes.Structure):
    """sh_canal_grid: levels z_l = z0 - l dz (l < L) and A rays per level in a humerus' canal frame."""
    _fields_ = [("z0", ctypes.c_double), ("dz", ctypes.c_double), ("L", ctypes.c_int32), ("A", ctypes.c_int32)]


class CanalLevel(ctypes.Structure):
    """sh_canal_level: the polar profile of one (humerus, level) about the canal axis."""
    _fields_ = [("r_min", ctypes.c_double), ("r_max", ctypes.c_double), ("r_mean", ctypes.c_double), ("area", ctypes.c_double),
                ("centroid", ctypes.c_double * 2), ("extent_x", ctypes.c_double * 2), ("extent_y", ctypes.c_double * 2),
                ("wall_min", ctypes.c_double), ("a_min", ctypes.c_int32), ("a_max", ctypes.c_int32), ("n_hit", ctypes.c_int32),
                ("status", ctypes.c_int32)]


CANAL_LEVEL_DTYPE = np.dtype([
    ("r_min", "<f8"), ("r_max", "<f8"), ("r_mean", "<f8"), ("area", "<f8"), ("centroid", "<f8", (2,)), ("extent_x", "<f8", (2,)),
    ("extent_y", "<f8", (2,)), ("wall_min", "<f8"), ("a_min", "<i4"), ("a_max", "<i4"), ("n_hit", "<i4"), ("status", "<i4")])
assert CANAL_LEVEL_DTYPE.itemsize == ctypes.sizeof(CanalLevel)
STEM_MAX = 64


class Stem(ctypes.Structure):
    """sh_stem: a frustum about the canal axis, r(d) = r_prox + (r_tip - r_prox) d / length."""
    _fields_ = [("length", ctypes.c_double), ("r_prox", ctypes.c_double), ("r_tip", ctypes.c_double)]


STEM_DTYPE = np.dtype([("length", "<f8"), ("r_prox", "<f8"), ("r_tip", "<f8")])


class StemFit(ctypes.Structure):
    """sh_stem_fit: how one stem of a catalogue sits in the canal below one (humerus, plane) cut."""
    _fields_ = [("entry", ctypes.c_double * 3), ("z_entry", ctypes.c_double), ("min_clearance", ctypes.c_double), ("depth", ctypes.c_double),
                ("direction", ctypes.c_double * 3), ("scale_max", ctypes.c_double), ("fill_mean", ctypes.c_double), ("fill_max", ctypes.c_double),
                ("fill_max_depth", ctypes.c_double), ("angle_index", ctypes.c_int32), ("n_samples", ctypes.c_int32), ("n_breach", ctypes.c_int32),
                ("n_open", ctypes.c_int32), ("fits", ctypes.c_int32), ("status", ctypes.c_int32)]


STEM_FIT_DTYPE = np.dtype([
    ("entry", "<f8", (3,)), ("z_entry", "<f8"), ("min_clearance", "<f8"), ("depth", "<f8"), ("direction", "<f8", (3,)), ("scale_max", "<f8"),
    ("fill_mean", "<f8"), ("fill_max", "<f8"), ("fill_max_depth", "<f8"), ("angle_index", "<i4"), ("n_samples", "<i4"), ("n_breach", "<i4"),
    ("n_open", "<i4"), ("fits", "<i4"), ("status", "<i4")])
assert STEM_FIT_DTYPE.itemsize == ctypes.sizeof(StemFit) and STEM_DTYPE.itemsize == ctypes.sizeof(Stem)


PLAN_MAX = 64
_PLAN_RULE_FIELDS = ("max_overhang", "min_coverage", "min_clearance", "max_eccentricity", "fill_target", "margin",
                     "w_uncovered", "w_overhang", "w_cor", "w_height", "w_eccentricity", "w_fill")


class PlanRule(ctypes.Structure):
    """sh_plan_rule: the limits, the two constants and the weights one ranking of (cut, head, stem) triples runs under."""
    _fields_ = [(n, ctypes.c_double) for n in _PLAN_RULE_FIELDS]


PLAN_RULE_DTYPE = np.dtype([(n, "<f8") for n in _PLAN_RULE_FIELDS])


class PlanRef(ctypes.Structure):
    """sh_plan_ref: the height reference of one humerus -- native head apex and tuberosity top in its canal frame."""
    _fields_ = [("tuberosity_top", ctypes.c_double * 3), ("tuberosity_z", ctypes.c_double), ("head_apex", ctypes.c_double * 3),
                ("head_apex_z", ctypes.c_double), ("head_height", ctypes.c_double), ("n_feasible", ctypes.c_int64),
                ("tuberosity_vid", ctypes.c_int32), ("head_apex_vid", ctypes.c_int32), ("status", ctypes.c_int32), ("pad", ctypes.c_int32)]


PLAN_REF_DTYPE = np.dtype([
    ("tuberosity_top", "<f8", (3,)), ("tuberosity_z", "<f8"), ("head_apex", "<f8", (3,)), ("head_apex_z", "<f8"), ("head_height", "<f8"),
    ("n_feasible", "<i8"), ("tuberosity_vid", "<i4"), ("head_apex_vid", "<i4"), ("status", "<i4"), ("pad", "<i4")])


class Plan(ctypes.Structure):
    """sh_plan: one ranked (cut, head, stem) triple of one humerus, its cost and the six unweighted terms of it."""
    _fields_ = [("cost", ctypes.c_double), ("uncovered", ctypes.c_double), ("overhang", ctypes.c_double), ("cor", ctypes.c_double),
                ("height", ctypes.c_double), ("eccentricity", ctypes.c_double), ("fill", ctypes.c_double), ("apex", ctypes.c_double * 3),
                ("apex_z", ctypes.c_double), ("head_height", ctypes.c_double), ("cut", ctypes.c_int32), ("head", ctypes.c_int32),
                ("stem", ctypes.c_int32), ("status", ctypes.c_int32)]


PLAN_DTYPE = np.dtype([
    ("cost", "<f8"), ("uncovered", "<f8"), ("overhang", "<f8"), ("cor", "<f8"), ("height", "<f8"), ("eccentricity", "<f8"), ("fill", "<f8"),
    ("apex", "<f8", (3,)), ("apex_z", "<f8"), ("head_height", "<f8"), ("cut", "<i4"), ("head", "<i4"), ("stem", "<i4"), ("status", "<i4")])
PLAN_TERM_DTYPE = np.dtype([("cost", "<f8"), ("feasible", "<i4"), ("pad", "<i4")])      # the elements of "plan.cut_terms" / "head_terms" / "stem_terms"
assert PLAN_RULE_DTYPE.itemsize == ctypes.sizeof(PlanRule) and PLAN_REF_DTYPE.itemsize == ctypes.sizeof(PlanRef) and PLAN_DTYPE.itemsize == ctypes.sizeof(Plan)


RAY_MAX, RAY_MAX_HITS = 65536, 1024


class Ray(ctypes.Structure):
    """sh_ray: origin and direction (CT; t counts in units of |dir|)."""
    _fields_ = [("origin", ctypes.c_double * 3), ("dir", ctypes.c_double * 3)]


class RayHit(ctypes.Structure):
    """sh_ray_hit: one hit of one ray -- t, the point, the humerus-local face and +1 where the ray runs against the face's normal."""
    _fields_ = [("t", ctypes.c_double), ("point", ctypes.c_double * 3), ("face", ctypes.c_int32), ("side", ctypes.c_int32)]


RAY_DTYPE = np.dtype([("origin", "<f8", (3,)), ("dir", "<f8", (3,))])
RAY_HIT_DTYPE = np.dtype([("t", "<f8"), ("point", "<f8", (3,)), ("face", "<i4"), ("side", "<i4")])
assert RAY_DTYPE.itemsize == ctypes.sizeof(Ray) and RAY_HIT_DTYPE.itemsize == ctypes.sizeof(RayHit) == 40


CLOSEST_MAX = 1048576


class Closest(ctypes.Structure):
    """sh_closest: the closest surface point of one humerus to one query point -- distance, point (CT), the humerus-local face, the
    region of that face (0 interior, 1 / 2 / 3 edge AB / BC / CA, 4 / 5 / 6 vertex A / B / C), +1 on the side the face's normal points to."""
    _fields_ = [("dist", ctypes.c_double), ("point", ctypes.c_double * 3), ("face", ctypes.c_int32), ("region", ctypes.c_int32),
                ("side", ctypes.c_int32), ("status", ctypes.c_int32)]


CLOSEST_DTYPE = np.dtype([("dist", "<f8"), ("point", "<f8", (3,)), ("face", "<i4"), ("region", "<i4"), ("side", "<i4"), ("status", "<i4")])
assert CLOSEST_DTYPE.itemsize == ctypes.sizeof(Closest) == 48


WINDING_MAX = 1048576
WIND_BLOCK = 2048


class Winding(ctypes.Structure):
    """sh_winding: the generalized winding number of one humerus about one query point, inside = 1 when |winding| >= 0.5 (undefined on
    the surface itself, where winding is about 0.5), status 0 or SH_ERR_GEOMETRY with zeros when the sum was not finite."""
    _fields_ = [("winding", ctypes.c_double), ("inside", ctypes.c_int32), ("status", ctypes.c_int32)]


WINDING_DTYPE = np.dtype([("winding", "<f8"), ("inside", "<i4"), ("status", "<i4")])
assert WINDING_DTYPE.itemsize == ctypes.sizeof(Winding) == 16


ICP_POINT, ICP_PLANE, ICP_BLOCK, ICP_MAX_ITER = 0, 1, 256, 64


class IcpOptions(ctypes.Structure):
    """sh_icp_options: the metric (ICP_POINT / ICP_PLANE), max_iter in 1..64, the rejection distance in mm (inf: none) and the rms
    change at or below which a humerus has converged (0: every iteration runs)."""
    _fields_ = [("metric", ctypes.c_int32), ("max_iter", ctypes.c_int32), ("reject", ctypes.c_double), ("tol", ctypes.c_double)]


class Registration(ctypes.Structure):
    """sh_registration: the rigid CT -> CT transform of one humerus' point set onto its mesh, the rms and the accepted pairs at that
    transform, the rms at the start, the smallest Cholesky pivot ratio of the last solve (1.0 under the point metric), the updates
    applied, whether the rms settled within tol, and the status."""
    _fields_ = [("T", ctypes.c_double * 16), ("rms", ctypes.c_double), ("rms_first", ctypes.c_double), ("min_pivot", ctypes.c_double),
                ("pairs", ctypes.c_int32), ("iterations", ctypes.c_int32), ("converged", ctypes.c_int32), ("status", ctypes.c_int32)]


REGISTRATION_DTYPE = np.dtype([("T", "<f8", (4, 4)), ("rms", "<f8"), ("rms_first", "<f8"), ("min_pivot", "<f8"), ("pairs", "<i4"),
                               ("iterations", "<i4"), ("converged", "<i4"), ("status", "<i4")])
assert REGISTRATION_DTYPE.itemsize == ctypes.sizeof(Registration) == 168 and ctypes.sizeof(IcpOptions) == 24


MASS_BLOCK, MS_MAX_STARTS = 256, 64


class Mass(ctypes.Structure):
    """sh_mass: the surface and volume integrals of one resident humerus -- area, signed volume, closure (|sum of face normals| / (2 area):
    0 on a closed mesh); the shell's centroid (CT), covariance (00, 01, 02, 11, 12, 22), its eigenvalues descending and their axes as
    rows, long axis first; the centre of mass (CT), the inertia tensor at density 1 about it, its principal moments ascending and their
    axes as rows; faces, the faces of zero area, status (shell) and vstatus (volume)."""
    _fields_ = [("area", ctypes.c_double), ("volume", ctypes.c_double), ("closure", ctypes.c_double), ("shell_centroid", ctypes.c_double * 3),
                ("shell_cov", ctypes.c_double * 6), ("shell_eig", ctypes.c_double * 3), ("shell_axes", ctypes.c_double * 9),
                ("center_mass", ctypes.c_double * 3), ("inertia", ctypes.c_double * 9), ("principal", ctypes.c_double * 3),
                ("principal_axes", ctypes.c_double * 9), ("faces", ctypes.c_int32), ("degenerate", ctypes.c_int32), ("status", ctypes.c_int32),
                ("vstatus", ctypes.c_int32)]


MASS_DTYPE = np.dtype([("area", "<f8"), ("volume", "<f8"), ("closure", "<f8"), ("shell_centroid", "<f8", (3,)), ("shell_cov", "<f8", (6,)),
                       ("shell_eig", "<f8", (3,)), ("shell_axes", "<f8", (3, 3)), ("center_mass", "<f8", (3,)), ("inertia", "<f8", (3, 3)),
                       ("principal", "<f8", (3,)), ("principal_axes", "<f8", (3, 3)), ("faces", "<i4"), ("degenerate", "<i4"), ("status", "<i4"),
                       ("vstatus", "<i4")])
assert MASS_DTYPE.itemsize == ctypes.sizeof(Mass) == 400


SAMPLE_MAX, SAMPLE_THIN_MAX, SAMPLE_BLOCK, THIN_MAX_ROUNDS = 1048576, 65536, 256, 32


class SampleOptions(ctypes.Structure):
    """sh_sample_options: the minimum spacing of the thinning in mm (0: no thinning) and the rounds it may take (1..32)."""
    _fields_ = [("radius", ctypes.c_double), ("max_rounds", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Sample(ctypes.Structure):
    """sh_sample: one surface sample of a resident humerus -- the point (CT), the barycentric weights u, v of corners B and C of its
    face (humerus-local), and keep: 1 kept, 0 removed by the thinning, -1 undecided when max_rounds ran out."""
    _fields_ = [("point", ctypes.c_double * 3), ("u", ctypes.c_double), ("v", ctypes.c_double), ("face", ctypes.c_int32), ("keep", ctypes.c_int32)]


class SampleInfo(ctypes.Structure):
    """sh_sample_info: the humerus' area, its samples with keep == 1, the rounds the thinning took, and the status."""
    _fields_ = [("area", ctypes.c_double), ("kept", ctypes.c_int32), ("rounds", ctypes.c_int32), ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


SAMPLE_DTYPE = np.dtype([("point", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"), ("face", "<i4"), ("keep", "<i4")])
SAMPLE_INFO_DTYPE = np.dtype([("area", "<f8"), ("kept", "<i4"), ("rounds", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
assert SAMPLE_DTYPE.itemsize == ctypes.sizeof(Sample) == 48 and SAMPLE_INFO_DTYPE.itemsize == ctypes.sizeof(SampleInfo) == 24
assert ctypes.sizeof(SampleOptions) == 16


ADJ_BORDER, ADJ_NONMANIFOLD, ADJ_DEGENERATE = -1, -2, -3
TOPO_MAX_SHELLS, TOPO_MAX_ROUNDS, TOPO_WATERTIGHT, TOPO_CONSISTENT = 65536, 32, 1, 2
_TOPOLOGY_FIELDS = ("status", "rounds", "faces_degenerate", "vertices_used", "edges", "border_edges", "nonmanifold_edges", "inconsistent_edges",
                    "euler", "max_valence", "n_shells", "shells_written", "largest_shell", "largest_faces", "flags", "reserved")
_SHELL_COUNTS = ("first_face", "faces", "border_slots", "nonmanifold_slots", "manifold_edges", "inconsistent_edges")


class TopologyOptions(ctypes.Structure):
    """sh_topology_options: the shell records kept per mesh (1..65536) and the rounds the labelling may take (1..32)."""
    _fields_ = [("max_shells", ctypes.c_int32), ("max_rounds", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Topology(ctypes.Structure):
    """sh_topology: the counts of one resident mesh (include/shoulder_hip.h); flags bit 0 watertight, bit 1 winding-consistent."""
    _fields_ = [(n, ctypes.c_int32) for n in _TOPOLOGY_FIELDS]


class Shell(ctypes.Structure):
    """sh_shell: one connected component over manifold edges -- its first face, its faces, its slot counts and its float32 box."""
    _fields_ = [(n, ctypes.c_int32) for n in _SHELL_COUNTS] + [("lo", ctypes.c_float * 3), ("hi", ctypes.c_float * 3)]


TOPOLOGY_OPTIONS = TopologyOptions
TOPOLOGY_DTYPE = np.dtype([(n, "<i4") for n in _TOPOLOGY_FIELDS])
SHELL_DTYPE = np.dtype([(n, "<i4") for n in _SHELL_COUNTS] + [("lo", "<f4", (3,)), ("hi", "<f4", (3,))])
assert TOPOLOGY_DTYPE.itemsize == ctypes.sizeof(Topology) == 64 and SHELL_DTYPE.itemsize == ctypes.sizeof(Shell) == 48
assert ctypes.sizeof(TopologyOptions) == 12


class Params(ctypes.Structure):
    _fields_ = [("canal_cutoff", ctypes.c_double * 2), ("groove_cutoff", ctypes.c_double * 2),
                ("groove_deg_window", ctypes.c_double), ("unet_dtype", ctypes.c_int32), ("bone_kind", ctypes.c_int32)]


EXPORTS = ["sh_ctx_create", "sh_ctx_destroy", "sh_last_error", "sh_default_params", "sh_set_params", "sh_load_rfc",
           "sh_load_unet", "sh_param_block", "sh_upload_meshes", "sh_synth_batch", "sh_batch_size", "sh_run",
           "sh_landmarks_device", "sh_affine_apply", "sh_mesh_transformed", "sh_transform_points", "sh_section_plane", "sh_buffer_info", "sh_fetch", "sh_store",
           "sh_kernel_time_ms", "sh_enable_timing", "sh_set_overlap", "sh_discard_prepared", "sh_unet_infer", "sh_host_alloc", "sh_host_free", "sh_upload_stl", "sh_submit", "sh_collect",
           "sh_stage_meshes", "sh_stage_stl", "sh_commit_staged", "sh_staged", "sh_set_record_rows", "sh_record_bytes", "sh_anp_points",
           "sh_comm_init_all", "sh_bcast_weights", "sh_gather_landmarks", "sh_set_keep_products",
           "sh_slice_mesh_planes", "sh_set_unet_turns", "sh_get_params", "sh_buffer_device", "sh_param_block_commit", "sh_set_hull_mode", "sh_get_hull_mode", "sh_auto_hull_mode", "sh_ring",
           "sh_set_open_contours", "sh_get_open_contours", "sh_open_contour_stats", "sh_mesh_open_edges",
           "sh_resect_planes", "sh_resect_offsets", "sh_resect_ring", "sh_resect_planes_fit", "sh_resect_offsets_fit",
           "sh_resect_planes_seat", "sh_resect_offsets_seat", "sh_canal_profile", "sh_resect_stems", "sh_resect_plan",
           "sh_ray_cast", "sh_anp_axis_hits", "sh_closest_points", "sh_winding_numbers", "sh_register_points",
           "sh_mass_properties", "sh_register_multistart", "sh_sample_surface", "sh_mesh_topology"]

_lib = None


def lib_path():
    return _build.LIB


def load(build_if_missing=True):
    """Load (building in-tree first if the .so is absent or stale and hipcc is present)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    alt = os.environ.get("SHOULDER_LIB")      # experiments: an alternative build of the same sources (A/B runs on one GPU box)
    if alt:
        if not os.path.exists(alt):
            raise RuntimeError(f"SHOULDER_LIB={alt} does not exist")
        path, build_if_missing = alt, False
    if build_if_missing and _build.is_stale():
        try:
            _build.build_lib(verbose=False)
        except Exception as e:  # no hipcc: use a prebuilt .so if there is one
            if not os.path.exists(path):
                raise RuntimeError(f"libshoulder_hip.so is not built and cannot be built here: {e}") from e
    if not os.path.exists(path):
        raise RuntimeError(f"{path} missing: run `python -m shoulder_amd.build` (needs hipcc / ROCm)")
    L = ctypes.CDLL(path)
    vp, cp = ctypes.c_void_p, ctypes.c_char_p
    L.sh_ctx_create.argtypes = [ctypes.c_int, vp, ctypes.POINTER(vp)]
    L.sh_ctx_destroy.argtypes = [vp]
    L.sh_ctx_destroy.restype = None
    L.sh_last_error.argtypes = [vp]
    L.sh_last_error.restype = cp
    L.sh_default_params.argtypes = [ctypes.POINTER(Params)]
    L.sh_set_params.argtypes = [vp, ctypes.POINTER(Params)]
    L.sh_get_params.argtypes = [vp, ctypes.POINTER(Params)]
    L.sh_buffer_device.argtypes = [vp, cp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    L.sh_param_block_commit.argtypes = [vp]
    L.sh_set_hull_mode.argtypes = [vp, cp]
    L.sh_get_hull_mode.argtypes = [vp]
    L.sh_auto_hull_mode.argtypes = []
    L.sh_load_rfc.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_int, vp, ctypes.c_int]
    L.sh_load_unet.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_size_t]
    L.sh_param_block.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    L.sh_upload_meshes.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int]
    L.sh_synth_batch.argtypes = [vp, vp, ctypes.c_int]
    L.sh_batch_size.argtypes = [vp]
    L.sh_run.argtypes = [vp, ctypes.c_uint32, vp]
    L.sh_submit.argtypes = [vp, ctypes.c_uint32, vp]
    L.sh_collect.argtypes = [vp]
    L.sh_landmarks_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    L.sh_affine_apply.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int]
    L.sh_mesh_transformed.argtypes = [vp, ctypes.c_int, vp, vp]
    L.sh_transform_points.argtypes = [vp, vp, vp, ctypes.c_int, vp]
    L.sh_ring.argtypes = [vp, cp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.sh_section_plane.argtypes = [vp, ctypes.c_int, vp, vp, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.sh_slice_mesh_planes.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, vp, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, vp]
    L.sh_buffer_info.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
    L.sh_fetch.argtypes = [vp, cp, vp, ctypes.c_size_t]
    L.sh_store.argtypes = [vp, cp, vp, ctypes.c_size_t]
    L.sh_kernel_time_ms.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    L.sh_enable_timing.argtypes = [vp, ctypes.c_int]
    L.sh_set_overlap.argtypes = [vp, ctypes.c_int]
    L.sh_set_unet_turns.argtypes = [vp, ctypes.c_int]
    L.sh_discard_prepared.argtypes = [vp]
    L.sh_host_alloc.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(vp)]
    L.sh_host_free.argtypes = [vp, vp]
    L.sh_upload_stl.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, vp, vp]
    L.sh_stage_meshes.argtypes = [vp, vp, vp, vp, vp, ctypes.c_int]
    L.sh_stage_stl.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ctypes.c_int]
    L.sh_commit_staged.argtypes = [vp, vp, vp]
    L.sh_staged.argtypes = [vp]
    L.sh_set_record_rows.argtypes = [vp, ctypes.c_int]
    L.sh_record_bytes.argtypes = [ctypes.c_int]
    L.sh_record_bytes.restype = ctypes.c_size_t
    L.sh_anp_points.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.sh_set_keep_products.argtypes = [vp, ctypes.c_int]
    L.sh_comm_init_all.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    L.sh_bcast_weights.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int]
    L.sh_gather_landmarks.argtypes = [ctypes.POINTER(vp), ctypes.c_int, vp]
    L.sh_unet_infer.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
    L.sh_set_open_contours.argtypes = [vp, ctypes.c_int, ctypes.c_double]
    L.sh_get_open_contours.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
    L.sh_open_contour_stats.argtypes = [vp, vp, vp]
    L.sh_mesh_open_edges.argtypes = [vp, vp]
    if not alt or hasattr(L, "sh_resect_planes"):      # (an A/B arm may be an older build: tools/time_resect.py parent)
        L.sh_resect_planes.argtypes = [vp, vp, ctypes.c_int, vp]
        L.sh_resect_offsets.argtypes = [vp, vp, ctypes.c_int, vp]
        L.sh_resect_ring.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    if not alt or hasattr(L, "sh_resect_planes_fit"):      # (tools/time_head_fit.py parent)
        L.sh_resect_planes_fit.argtypes = [vp, vp, ctypes.c_int, vp, vp]
        L.sh_resect_offsets_fit.argtypes = [vp, vp, ctypes.c_int, vp, vp]
    if not alt or hasattr(L, "sh_resect_planes_seat"):      # (tools/time_seat.py parent)
        L.sh_resect_planes_seat.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
        L.sh_resect_offsets_seat.argtypes = [vp, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    if not alt or hasattr(L, "sh_canal_profile"):      # (tools/time_stem.py parent)
        L.sh_canal_profile.argtypes = [vp, ctypes.POINTER(CanalGrid), vp, vp, vp, vp]
        L.sh_resect_stems.argtypes = [vp, vp, ctypes.c_int, vp]
    if not alt or hasattr(L, "sh_resect_plan"):      # (tools/time_plan.py and the benchmark's parent arm)
        L.sh_resect_plan.argtypes = [vp, ctypes.POINTER(PlanRule), vp, vp, ctypes.c_int, vp, vp]
    if not alt or hasattr(L, "sh_ray_cast"):      # (tools/time_rays.py and the benchmark's parent arm)
        L.sh_ray_cast.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
        L.sh_anp_axis_hits.argtypes = [vp, ctypes.c_int, vp, vp, vp]
    if not alt or hasattr(L, "sh_closest_points"):      # (tools/time_closest.py and the benchmark's parent arm)
        L.sh_closest_points.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp]
    if not alt or hasattr(L, "sh_winding_numbers"):      # (tools/time_winding.py and the benchmark's parent arm)
        L.sh_winding_numbers.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp]
    if not alt or hasattr(L, "sh_register_points"):      # (the benchmark's parent arm has no registration)
        L.sh_register_points.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    if not alt or hasattr(L, "sh_mass_properties"):      # (tools/time_register_global.py and the benchmark's parent arm)
        L.sh_mass_properties.argtypes = [vp, vp]
        L.sh_register_multistart.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    if not alt or hasattr(L, "sh_sample_surface"):      # (tools/time_sample.py and the benchmark's parent arm)
        L.sh_sample_surface.argtypes = [vp, ctypes.c_int, vp, ctypes.POINTER(SampleOptions), vp, vp]
    if not alt or hasattr(L, "sh_mesh_topology"):      # (tools/time_topology.py and the benchmark's parent arm)
        L.sh_mesh_topology.argtypes = [vp, ctypes.POINTER(TopologyOptions), vp, vp]
    _lib = L
    return L
