"""ctypes binding of libshoulder_hip.so (include/shoulder_hip.h).  Fails loudly when the HIP
library is missing -- there is no CPU fallback on the product path.

Every record of the header is stated once, as a row of RECORDS (_record below); every entry point once, as a row of SIGNATURES.
tests/test_abi_exports.py holds both tables, and the constants, to a C compile of the header."""
import ctypes
import os

import numpy as np

from . import build as _build

# ---- the header's SH_* values, without the prefix ---------------------------------------------------------------------------------------
STAGE_OBB, STAGE_FULL, STAGE_NECK, STAGE_CANAL, STAGE_PROXIMAL = 1, 2, 4, 8, 16
STAGE_GROOVE, STAGE_ANP, STAGE_DISTAL, STAGE_TE, STAGE_CSYS = 32, 64, 128, 256, 512
STAGE_APPLY = 1024
STAGE_ALL = 0x7FF
UNET_F32, UNET_BF16, UNET_F16, UNET_F32X = 0, 1, 2, 3
BONE_HUMERUS, BONE_PROXIMAL = 0, 1
OPEN_ERROR, OPEN_BRIDGE = 0, 1
OPEN_GAP_DEFAULT = 12.0      # mm
GROOVE_ROWS = 330
ANP_MAX_PTS = 4096
SEAT_CUT_CENTROID, SEAT_SPHERE_AXIS, SEAT_MAX_HEADS = 0, 1, 64
STEM_MAX = 64
PLAN_MAX = 64
RAY_MAX, RAY_MAX_HITS = 65536, 1024
CLOSEST_MAX = 1048576
WINDING_MAX = 1048576
WIND_BLOCK = 2048
ICP_POINT, ICP_PLANE, ICP_BLOCK, ICP_MAX_ITER = 0, 1, 256, 64
MASS_BLOCK, MS_MAX_STARTS = 256, 64
SAMPLE_MAX, SAMPLE_THIN_MAX, SAMPLE_BLOCK, THIN_MAX_ROUNDS = 1048576, 65536, 256, 32
ADJ_BORDER, ADJ_NONMANIFOLD, ADJ_DEGENERATE = -1, -2, -3
TOPO_MAX_SHELLS, TOPO_MAX_ROUNDS, TOPO_WATERTIGHT, TOPO_CONSISTENT = 65536, 32, 1, 2
VERT_WEIGHT_AREA, VERT_WEIGHT_ANGLE, VERT_MAX_SMOOTH, VERT_FIELDS = 0, 1, 64, 8
VERT_USED, VERT_BORDER, VERT_NONMANIFOLD, VERT_FLAT = 1, 2, 4, 8
GEO_EDGES, GEO_UNFOLD, GEO_MAX_SETS, GEO_LDS_VERTICES, GEO_CHUNK, GEO_INFO_BYTES = 0, 1, 16, 20000, 32, 32
GEO_ROOT, GEO_NO_PRED, GEO_UNREACHED = -1, -2, -3
SMOOTH_LAPLACIAN, SMOOTH_TAUBIN, SMOOTH_HC, SMOOTH_UNIFORM, SMOOTH_INVLEN = 0, 1, 2, 0, 1
SMOOTH_PIN_BORDER, SMOOTH_KEEP_VOLUME, SMOOTH_MAX_ITER, SMOOTH_INFO_BYTES = 1, 2, 256, 64
REPAIR_NONE, REPAIR_WINDING, REPAIR_OUTWARD, REPAIR_NESTED, REPAIR_FILL_NONE, REPAIR_FAN, REPAIR_CENTROID = 0, 1, 2, 3, 0, 1, 2
REPAIR_NONORIENTABLE, REPAIR_AMBIGUOUS, REPAIR_CHANGED, REPAIR_SHELLS_LEFT = 1, 2, 1, 2
REPAIR_HOLE_FILLED, REPAIR_HOLE_TOO_LONG, REPAIR_HOLE_SHELL, REPAIR_HOLE_OPEN, REPAIR_HOLE_TOO_SHORT = 0, 1, 2, 3, 4
REPAIR_MAX_HOLES, REPAIR_MAX_ROUNDS, REPAIR_LDS_FACES = 65536, 1048576, 131072
SIMPLIFY_MEAN, SIMPLIFY_QUADRIC, SIMPLIFY_MAX_CELLS, SIMPLIFY_MAX_CLUSTERS = 0, 1, 1048576, 2097152
ACCEL_OFF, ACCEL_BVH, BVH_INFO_BYTES = 0, 1, 48

# ---- the records ------------------------------------------------------------------------------------------------------------------------
RECORDS = {}      # C name -> (ctypes.Structure, NumPy dtype), in the order of the header
_CTYPES = {"<f8": ctypes.c_double, "<f4": ctypes.c_float, "<i4": ctypes.c_int32, "<i8": ctypes.c_int64}


def _record(cname, pyname, doc, fields, size=None):
    """One record of the header: `fields` is a NumPy field list (name, base type[, shape]) in the header's order.  -> (the
    ctypes.Structure called pyname, its arrays flat, and the dtype), entered into RECORDS."""
    dtype = np.dtype(fields)
    members = []
    for name in dtype.names:
        base, shape = dtype.fields[name][0].subdtype or (dtype.fields[name][0], ())
        members.append((name, _CTYPES[base.str] * int(np.prod(shape)) if shape else _CTYPES[base.str]))
    cls = type(pyname, (ctypes.Structure,), {"__doc__": doc, "__module__": __name__, "_fields_": members})
    assert ctypes.sizeof(cls) == dtype.itemsize == (size or dtype.itemsize), cname
    RECORDS[cname] = (cls, dtype)
    return cls, dtype


Landmarks, LANDMARKS_DTYPE = _record("sh_landmarks", "Landmarks", None, [
    ("obb_transform", "<f8", (4, 4)), ("z_length", "<f8"), ("neck_z", "<f8"), ("canal_axis", "<f8", (2, 3)),
    ("te_axis", "<f8", (2, 3)), ("groove_axis", "<f8", (2, 3)), ("bg_theta", "<f8"), ("anp_plane_point", "<f8", (3,)),
    ("anp_plane_normal", "<f8", (3,)), ("anp_axis_normal", "<f8", (2, 3)), ("anp_axis_central", "<f8", (2, 3)),
    ("csys", "<f8", (4, 4)), ("csys_articular", "<f8", (4, 4)), ("neckshaft", "<f8"), ("retroversion", "<f8"), ("radius_curvature", "<f8"), ("canal_cutoff", "<f8", (2,)), ("groove_points", "<f8", (GROOVE_ROWS, 3)), ("anp_points", "<f8", (ANP_MAX_PTS, 3)),
    ("n_anp", "<i4"), ("n_articular", "<i4"), ("neck_index", "<i4"), ("flipped", "<i4"), ("status", "<i4"), ("side", "<i4")])


def record_dtype(anp_rows=0):
    """NumPy dtype of the records a run hands out: the full sh_landmarks (anp_rows = 0) or the packed wire format of
    sh_set_record_rows(anp_rows): the fields in front of anp_points, the six trailing int32 fields, then anp_rows point rows."""
    if anp_rows <= 0:
        return LANDMARKS_DTYPE
    names = list(LANDMARKS_DTYPE.names)
    k = names.index("anp_points")
    fields = [(n, LANDMARKS_DTYPE.fields[n][0]) for n in names[:k] + names[k + 1:]] + [("anp_points", "<f8", (int(anp_rows), 3))]
    return np.dtype(fields)


Params, _ = _record("sh_params", "Params", None, [
    ("canal_cutoff", "<f8", (2,)), ("groove_cutoff", "<f8", (2,)), ("groove_deg_window", "<f8"), ("unet_dtype", "<i4"), ("bone_kind", "<i4")])

CutOffset, CUT_OFFSET_DTYPE = _record(
    "sh_cut_offset", "CutOffset", """sh_cut_offset: one planned cut relative to the native anatomic-neck plane (arthroplasty.py:90-175).""",
    [(n, "<f8") for n in ("retroversion_deg", "neckshaft_deg", "depth_canal_mm", "depth_anp_mm", "depth_resection_mm", "anterior_mm", "medial_mm")])

Resection, RESECTION_DTYPE = _record("sh_resection", "Resection", """sh_resection: the measurements of one (humerus, plane) cut.""", [
    ("plane_point", "<f8", (3,)), ("plane_normal", "<f8", (3,)), ("head_volume", "<f8"), ("head_area", "<f8"), ("head_height", "<f8"),
    ("cut_area", "<f8"), ("cut_perimeter", "<f8"), ("cut_centroid", "<f8", (3,)), ("cap_area", "<f8"),
    ("n_loops", "<i4"), ("n_ring", "<i4"), ("n_cut_faces", "<i4"), ("status", "<i4")])

HeadFit, HEAD_FIT_DTYPE = _record(
    "sh_head_fit", "HeadFit", """sh_head_fit: the sphere of the resected head piece and the ellipse of the cut, one (humerus, plane).""", [
        ("sphere_center", "<f8", (3,)), ("sphere_radius", "<f8"), ("sphere_rms", "<f8"), ("cap_height", "<f8"), ("fit_area", "<f8"),
        ("center_articular", "<f8", (3,)), ("cut_semi_major", "<f8"), ("cut_semi_minor", "<f8"), ("cut_major_dir", "<f8", (3,)),
        ("sphere_status", "<i4"), ("ring_status", "<i4")])

ImplantHead, IMPLANT_HEAD_DTYPE = _record(
    "sh_implant_head", "ImplantHead", """sh_implant_head: radius of curvature and thickness of one catalogue head.""",
    [("radius", "<f8"), ("thickness", "<f8")])

Seat, SEAT_DTYPE = _record("sh_seat", "Seat", """sh_seat: how one implant head sits on one (humerus, plane) cut.""", [
    ("base_radius", "<f8"), ("seat_center", "<f8", (3,)), ("covered_area", "<f8"), ("coverage", "<f8"), ("overhang_area", "<f8"),
    ("uncovered_area", "<f8"), ("rim_min", "<f8"), ("rim_max", "<f8"), ("max_overhang", "<f8"), ("max_uncovered", "<f8"),
    ("overhang_dir", "<f8", (3,)), ("uncovered_dir", "<f8", (3,)), ("implant_center", "<f8", (3,)), ("cor_shift", "<f8", (3,)),
    ("cor_shift_articular", "<f8", (3,)), ("surface_rms", "<f8"), ("center_inside", "<i4"), ("status", "<i4")])

CanalGrid, _ = _record(
    "sh_canal_grid", "CanalGrid", """sh_canal_grid: levels z_l = z0 - l dz (l < L) and A rays per level in a humerus' canal frame.""",
    [("z0", "<f8"), ("dz", "<f8"), ("L", "<i4"), ("A", "<i4")])

CanalLevel, CANAL_LEVEL_DTYPE = _record(
    "sh_canal_level", "CanalLevel", """sh_canal_level: the polar profile of one (humerus, level) about the canal axis.""", [
        ("r_min", "<f8"), ("r_max", "<f8"), ("r_mean", "<f8"), ("area", "<f8"), ("centroid", "<f8", (2,)), ("extent_x", "<f8", (2,)),
        ("extent_y", "<f8", (2,)), ("wall_min", "<f8"), ("a_min", "<i4"), ("a_max", "<i4"), ("n_hit", "<i4"), ("status", "<i4")])

Stem, STEM_DTYPE = _record(
    "sh_stem", "Stem", """sh_stem: a frustum about the canal axis, r(d) = r_prox + (r_tip - r_prox) d / length.""",
    [("length", "<f8"), ("r_prox", "<f8"), ("r_tip", "<f8")])

StemFit, STEM_FIT_DTYPE = _record(
    "sh_stem_fit", "StemFit", """sh_stem_fit: how one stem of a catalogue sits in the canal below one (humerus, plane) cut.""", [
        ("entry", "<f8", (3,)), ("z_entry", "<f8"), ("min_clearance", "<f8"), ("depth", "<f8"), ("direction", "<f8", (3,)), ("scale_max", "<f8"),
        ("fill_mean", "<f8"), ("fill_max", "<f8"), ("fill_max_depth", "<f8"), ("angle_index", "<i4"), ("n_samples", "<i4"), ("n_breach", "<i4"),
        ("n_open", "<i4"), ("fits", "<i4"), ("status", "<i4")])

PlanRule, PLAN_RULE_DTYPE = _record(
    "sh_plan_rule", "PlanRule", """sh_plan_rule: the limits, the two constants and the weights one ranking of (cut, head, stem) triples runs under.""",
    [(n, "<f8") for n in ("max_overhang", "min_coverage", "min_clearance", "max_eccentricity", "fill_target", "margin",
                          "w_uncovered", "w_overhang", "w_cor", "w_height", "w_eccentricity", "w_fill")])

PlanRef, PLAN_REF_DTYPE = _record(
    "sh_plan_ref", "PlanRef", """sh_plan_ref: the height reference of one humerus -- native head apex and tuberosity top in its canal frame.""", [
        ("tuberosity_top", "<f8", (3,)), ("tuberosity_z", "<f8"), ("head_apex", "<f8", (3,)), ("head_apex_z", "<f8"), ("head_height", "<f8"),
        ("n_feasible", "<i8"), ("tuberosity_vid", "<i4"), ("head_apex_vid", "<i4"), ("status", "<i4"), ("pad", "<i4")])

Plan, PLAN_DTYPE = _record(
    "sh_plan", "Plan", """sh_plan: one ranked (cut, head, stem) triple of one humerus, its cost and the six unweighted terms of it.""", [
        ("cost", "<f8"), ("uncovered", "<f8"), ("overhang", "<f8"), ("cor", "<f8"), ("height", "<f8"), ("eccentricity", "<f8"), ("fill", "<f8"),
        ("apex", "<f8", (3,)), ("apex_z", "<f8"), ("head_height", "<f8"), ("cut", "<i4"), ("head", "<i4"), ("stem", "<i4"), ("status", "<i4")])
PLAN_TERM_DTYPE = np.dtype([("cost", "<f8"), ("feasible", "<i4"), ("pad", "<i4")])      # the elements of "plan.cut_terms" / "head_terms" / "stem_terms"

Ray, RAY_DTYPE = _record("sh_ray", "Ray", """sh_ray: origin and direction (CT; t counts in units of |dir|).""",
                         [("origin", "<f8", (3,)), ("dir", "<f8", (3,))])

RayHit, RAY_HIT_DTYPE = _record(
    "sh_ray_hit", "RayHit", """sh_ray_hit: one hit of one ray -- t, the point, the humerus-local face and +1 where the ray runs against the face's normal.""",
    [("t", "<f8"), ("point", "<f8", (3,)), ("face", "<i4"), ("side", "<i4")], size=40)

Closest, CLOSEST_DTYPE = _record(
    "sh_closest", "Closest",
    """sh_closest: the closest surface point of one humerus to one query point -- distance, point (CT), the humerus-local face, the
    region of that face (0 interior, 1 / 2 / 3 edge AB / BC / CA, 4 / 5 / 6 vertex A / B / C), +1 on the side the face's normal points to.""",
    [("dist", "<f8"), ("point", "<f8", (3,)), ("face", "<i4"), ("region", "<i4"), ("side", "<i4"), ("status", "<i4")], size=48)

Winding, WINDING_DTYPE = _record(
    "sh_winding", "Winding",
    """sh_winding: the generalized winding number of one humerus about one query point, inside = 1 when |winding| >= 0.5 (undefined on
    the surface itself, where winding is about 0.5), status 0 or SH_ERR_GEOMETRY with zeros when the sum was not finite.""",
    [("winding", "<f8"), ("inside", "<i4"), ("status", "<i4")], size=16)

IcpOptions, _ = _record(
    "sh_icp_options", "IcpOptions",
    """sh_icp_options: the metric (ICP_POINT / ICP_PLANE), max_iter in 1..64, the rejection distance in mm (inf: none) and the rms
    change at or below which a humerus has converged (0: every iteration runs).""",
    [("metric", "<i4"), ("max_iter", "<i4"), ("reject", "<f8"), ("tol", "<f8")], size=24)

Registration, REGISTRATION_DTYPE = _record(
    "sh_registration", "Registration",
    """sh_registration: the rigid CT -> CT transform of one humerus' point set onto its mesh, the rms and the accepted pairs at that
    transform, the rms at the start, the smallest Cholesky pivot ratio of the last solve (1.0 under the point metric), the updates
    applied, whether the rms settled within tol, and the status.""",
    [("T", "<f8", (4, 4)), ("rms", "<f8"), ("rms_first", "<f8"), ("min_pivot", "<f8"), ("pairs", "<i4"),
     ("iterations", "<i4"), ("converged", "<i4"), ("status", "<i4")], size=168)

Mass, MASS_DTYPE = _record(
    "sh_mass", "Mass",
    """sh_mass: the surface and volume integrals of one resident humerus -- area, signed volume, closure (|sum of face normals| / (2 area):
    0 on a closed mesh); the shell's centroid (CT), covariance (00, 01, 02, 11, 12, 22), its eigenvalues descending and their axes as
    rows, long axis first; the centre of mass (CT), the inertia tensor at density 1 about it, its principal moments ascending and their
    axes as rows; faces, the faces of zero area, status (shell) and vstatus (volume).""",
    [("area", "<f8"), ("volume", "<f8"), ("closure", "<f8"), ("shell_centroid", "<f8", (3,)), ("shell_cov", "<f8", (6,)),
     ("shell_eig", "<f8", (3,)), ("shell_axes", "<f8", (3, 3)), ("center_mass", "<f8", (3,)), ("inertia", "<f8", (3, 3)),
     ("principal", "<f8", (3,)), ("principal_axes", "<f8", (3, 3)), ("faces", "<i4"), ("degenerate", "<i4"), ("status", "<i4"),
     ("vstatus", "<i4")], size=400)

SampleOptions, _ = _record(
    "sh_sample_options", "SampleOptions",
    """sh_sample_options: the minimum spacing of the thinning in mm (0: no thinning) and the rounds it may take (1..32).""",
    [("radius", "<f8"), ("max_rounds", "<i4"), ("reserved", "<i4")], size=16)

Sample, SAMPLE_DTYPE = _record(
    "sh_sample", "Sample",
    """sh_sample: one surface sample of a resident humerus -- the point (CT), the barycentric weights u, v of corners B and C of its
    face (humerus-local), and keep: 1 kept, 0 removed by the thinning, -1 undecided when max_rounds ran out.""",
    [("point", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"), ("face", "<i4"), ("keep", "<i4")], size=48)

SampleInfo, SAMPLE_INFO_DTYPE = _record(
    "sh_sample_info", "SampleInfo", """sh_sample_info: the humerus' area, its samples with keep == 1, the rounds the thinning took, and the status.""",
    [("area", "<f8"), ("kept", "<i4"), ("rounds", "<i4"), ("status", "<i4"), ("reserved", "<i4")], size=24)

TopologyOptions, _ = _record(
    "sh_topology_options", "TopologyOptions",
    """sh_topology_options: the shell records kept per mesh (1..65536) and the rounds the labelling may take (1..32).""",
    [("max_shells", "<i4"), ("max_rounds", "<i4"), ("reserved", "<i4")], size=12)
TOPOLOGY_OPTIONS = TopologyOptions

Topology, TOPOLOGY_DTYPE = _record(
    "sh_topology", "Topology", """sh_topology: the counts of one resident mesh (include/shoulder_hip.h); flags bit 0 watertight, bit 1 winding-consistent.""",
    [(n, "<i4") for n in ("status", "rounds", "faces_degenerate", "vertices_used", "edges", "border_edges", "nonmanifold_edges", "inconsistent_edges",
                          "euler", "max_valence", "n_shells", "shells_written", "largest_shell", "largest_faces", "flags", "reserved")], size=64)

Shell, SHELL_DTYPE = _record(
    "sh_shell", "Shell", """sh_shell: one connected component over manifold edges -- its first face, its faces, its slot counts and its float32 box.""",
    [(n, "<i4") for n in ("first_face", "faces", "border_slots", "nonmanifold_slots", "manifold_edges", "inconsistent_edges")]
    + [("lo", "<f4", (3,)), ("hi", "<f4", (3,))], size=48)

# the info record of sh_geodesic per (mesh, set): the header states its 32 bytes in words, not as a typedef
GEO_INFO_DTYPE = np.dtype([("far_dist", "<f8"), ("reached", "<i4"), ("roots", "<i4"), ("no_pred", "<i4"), ("farthest", "<i4"), ("sweeps", "<i4"), ("status", "<i4")])
assert GEO_INFO_DTYPE.itemsize == GEO_INFO_BYTES
# the info record of sh_smooth_vertices per mesh: stated in the header's text, as sh_geodesic's
SMOOTH_INFO_DTYPE = np.dtype([(n, "<f8") for n in ("volume_before", "volume_after", "scale", "max_disp", "sum_sq_disp")]
                             + [("pinned", "<i4"), ("isolated", "<i4"), ("status", "<i4"), ("pad", "<i4", (3,))])
assert SMOOTH_INFO_DTYPE.itemsize == SMOOTH_INFO_BYTES
# the records of sh_mesh_repair: the header declares each struct and its typedef in two statements, as sh_bvh_info; stated here once.
# tests/hostcheck/repair_check.cpp holds the sizes and offsets against a C compile of the header (rc_sizes)
REPAIR_OPTIONS_DTYPE = np.dtype([(n, "<i4") for n in ("orient", "fill", "max_hole_edges", "max_holes", "max_rounds", "reserved")])
REPAIR_INFO_DTYPE = np.dtype([(n, "<i4") for n in ("status", "shells_nonorientable", "shells_inverted", "faces_flipped", "holes", "holes_written", "holes_filled",
                                                   "largest_hole", "blocked_edges", "faces_added", "verts_added", "faces_out", "verts_out", "flags", "shell_records",
                                                   "reserved")])
REPAIR_SHELL_DTYPE = np.dtype([(n, "<i4") for n in ("status", "parity_flips", "inverted", "depth", "holes", "holes_filled")] + [("V6", "<f8"), ("W", "<f8")])
REPAIR_HOLE_DTYPE = np.dtype([(n, "<i4") for n in ("shell", "start_face", "start_slot", "edges", "status", "first_face", "faces_added", "vertex")])
assert (REPAIR_OPTIONS_DTYPE.itemsize, REPAIR_INFO_DTYPE.itemsize, REPAIR_SHELL_DTYPE.itemsize, REPAIR_HOLE_DTYPE.itemsize) == (24, 64, 40, 32)
# the records of sh_mesh_simplify (two statements each in the header, as the repair's); tests/hostcheck/simplify_check.cpp holds the sizes
# and offsets against a C compile of the header (sc_sizes)
SIMPLIFY_OPTIONS_DTYPE = np.dtype([("place", "<i4"), ("reserved", "<i4"), ("reg", "<f8"), ("clamp", "<f8")])
SIMPLIFY_INFO_DTYPE = np.dtype([(n, "<i4") for n in ("status", "verts_used", "clusters", "verts_out", "faces_out", "faces_collapsed", "faces_duplicate", "fallbacks",
                                                     "largest_cluster", "reserved")] + [("cell", "<f8"), ("max_move", "<f8"), ("pad", "<i4", (2,))])
assert (SIMPLIFY_OPTIONS_DTYPE.itemsize, SIMPLIFY_INFO_DTYPE.itemsize) == (24, 64)
# sh_bvh_info per mesh (sh_mesh_bvh): the header declares the struct and its typedef in two statements; stated here once, beside its bytes
BVH_INFO_DTYPE = np.dtype([(n, "<i4") for n in ("tight", "loose", "leaves", "levels", "nodes", "reserved")] + [("lo", "<f4", (3,)), ("hi", "<f4", (3,))])
assert BVH_INFO_DTYPE.itemsize == BVH_INFO_BYTES

# ---- the entry points -------------------------------------------------------------------------------------------------------------------
_P, _vp, _cp, _i, _d, _sz = ctypes.POINTER, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_double, ctypes.c_size_t


def _f(*argtypes, restype=_i, optional=False):
    """One entry point.  optional: with SHOULDER_LIB set the symbol may be absent (an A/B arm may be an older build: the benchmark's
    parent arm and tools/time_*.py); without it every symbol must be there."""
    return list(argtypes), restype, optional


SIGNATURES = {      # name -> (argtypes, restype, optional)
    "sh_ctx_create": _f(_i, _vp, _P(_vp)),
    "sh_ctx_destroy": _f(_vp, restype=None),
    "sh_last_error": _f(_vp, restype=_cp),
    "sh_default_params": _f(_P(Params)),
    "sh_set_params": _f(_vp, _P(Params)),
    "sh_load_rfc": _f(_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i),
    "sh_load_unet": _f(_vp, _i, _i, _vp, _sz),
    "sh_param_block": _f(_vp, _P(_vp), _P(_sz)),
    "sh_upload_meshes": _f(_vp, _vp, _vp, _vp, _vp, _i),
    "sh_synth_batch": _f(_vp, _vp, _i),
    "sh_batch_size": _f(_vp),
    "sh_run": _f(_vp, ctypes.c_uint32, _vp),
    "sh_landmarks_device": _f(_vp, _P(_vp), _P(_sz)),
    "sh_affine_apply": _f(_vp, _vp, _vp, _vp, _vp, _i),
    "sh_mesh_transformed": _f(_vp, _i, _vp, _vp),
    "sh_transform_points": _f(_vp, _vp, _vp, _i, _vp),
    "sh_section_plane": _f(_vp, _i, _vp, _vp, _vp, _i, _P(_i)),
    "sh_buffer_info": _f(_vp, _cp, _P(_sz), _P(_i)),
    "sh_fetch": _f(_vp, _cp, _vp, _sz),
    "sh_store": _f(_vp, _cp, _vp, _sz),
    "sh_kernel_time_ms": _f(_vp, _cp, _P(_d), _P(_i)),
    "sh_enable_timing": _f(_vp, _i),
    "sh_set_overlap": _f(_vp, _i),
    "sh_discard_prepared": _f(_vp),
    "sh_unet_infer": _f(_vp, _vp, _i, _i, _i, _vp),
    "sh_host_alloc": _f(_vp, _sz, _P(_vp)),
    "sh_host_free": _f(_vp, _vp),
    "sh_upload_stl": _f(_vp, _P(_vp), _P(_sz), _i, _vp, _vp),
    "sh_submit": _f(_vp, ctypes.c_uint32, _vp),
    "sh_collect": _f(_vp),
    "sh_stage_meshes": _f(_vp, _vp, _vp, _vp, _vp, _i),
    "sh_stage_stl": _f(_vp, _P(_vp), _P(_sz), _i),
    "sh_commit_staged": _f(_vp, _vp, _vp),
    "sh_staged": _f(_vp),
    "sh_set_record_rows": _f(_vp, _i),
    "sh_record_bytes": _f(_i, restype=_sz),
    "sh_anp_points": _f(_vp, _i, _vp, _i, _P(_i)),
    "sh_comm_init_all": _f(_P(_vp), _i),
    "sh_bcast_weights": _f(_P(_vp), _i, _i),
    "sh_gather_landmarks": _f(_P(_vp), _i, _vp),
    "sh_set_keep_products": _f(_vp, _i),
    "sh_slice_mesh_planes": _f(_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp),
    "sh_set_unet_turns": _f(_vp, _i),
    "sh_get_params": _f(_vp, _P(Params)),
    "sh_buffer_device": _f(_vp, _cp, _P(_vp), _P(_sz)),
    "sh_param_block_commit": _f(_vp),
    "sh_set_hull_mode": _f(_vp, _cp),
    "sh_get_hull_mode": _f(_vp),
    "sh_auto_hull_mode": _f(),
    "sh_ring": _f(_vp, _cp, _i, _i, _vp, _i, _P(_i)),
    "sh_set_open_contours": _f(_vp, _i, _d),
    "sh_get_open_contours": _f(_vp, _P(_i), _P(_d)),
    "sh_open_contour_stats": _f(_vp, _vp, _vp),
    "sh_mesh_open_edges": _f(_vp, _vp),
    "sh_resect_planes": _f(_vp, _vp, _i, _vp, optional=True),
    "sh_resect_offsets": _f(_vp, _vp, _i, _vp, optional=True),
    "sh_resect_ring": _f(_vp, _i, _i, _vp, _i, _P(_i), optional=True),
    "sh_resect_planes_fit": _f(_vp, _vp, _i, _vp, _vp, optional=True),
    "sh_resect_offsets_fit": _f(_vp, _vp, _i, _vp, _vp, optional=True),
    "sh_resect_planes_seat": _f(_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, optional=True),
    "sh_resect_offsets_seat": _f(_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, optional=True),
    "sh_canal_profile": _f(_vp, _P(CanalGrid), _vp, _vp, _vp, _vp, optional=True),
    "sh_resect_stems": _f(_vp, _vp, _i, _vp, optional=True),
    "sh_resect_plan": _f(_vp, _P(PlanRule), _vp, _vp, _i, _vp, _vp, optional=True),
    "sh_ray_cast": _f(_vp, _vp, _i, _i, _i, _vp, _vp, optional=True),
    "sh_anp_axis_hits": _f(_vp, _i, _vp, _vp, _vp, optional=True),
    "sh_ray_nearest": _f(_vp, _vp, _i, _i, _vp, optional=True),
    "sh_closest_points": _f(_vp, _vp, _i, _i, _vp, optional=True),
    "sh_winding_numbers": _f(_vp, _vp, _i, _i, _vp, optional=True),
    "sh_register_points": _f(_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, optional=True),
    "sh_mass_properties": _f(_vp, _vp, optional=True),
    "sh_register_multistart": _f(_vp, _vp, _i, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, optional=True),
    "sh_sample_surface": _f(_vp, _i, _vp, _P(SampleOptions), _vp, _vp, optional=True),
    "sh_mesh_topology": _f(_vp, _P(TopologyOptions), _vp, _vp, optional=True),
    "sh_vertex_fields": _f(_vp, _i, _i, _vp, _vp, _vp, _vp, optional=True),
    "sh_geodesic": _f(_vp, _i, _i, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp, optional=True),
    "sh_smooth_vertices": _f(_vp, _i, _i, _i, _i, _d, _d, _vp, _vp, _vp, optional=True),
    "sh_mesh_repair": _f(_vp, _vp, _vp, _vp, _vp, _vp, optional=True),
    "sh_mesh_simplify": _f(_vp, _vp, _vp, _vp, _vp, _vp, _vp, optional=True),
    "sh_mesh_bvh": _f(_vp, _vp, optional=True),
    "sh_set_query_accel": _f(_vp, _i, optional=True),
    "sh_get_query_accel": _f(_vp, optional=True),
}
EXPORTS = list(SIGNATURES)

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
    for name, (argtypes, restype, optional) in SIGNATURES.items():
        if optional and alt and not hasattr(L, name):
            continue
        fn = getattr(L, name)      # (raises where a symbol that must be there is missing)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = L
    return L
