"""CPU-only ABI checks: libshoulder_hip.so loads without a GPU, exports every entry point that
include/shoulder_hip.h declares, and the record layout agrees between the C header and the ctypes /
NumPy mirrors.  No compute call is made."""
import ctypes
import os
import re

import pytest

import abi_probe
from conftest import ROOT
from shoulder_amd import _lib


def _declared():
    src = open(os.path.join(ROOT, "include", "shoulder_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sh_[a-z_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported():
    names = _declared()
    assert len(names) >= 20
    L = ctypes.CDLL(_lib.lib_path()) if os.path.exists(_lib.lib_path()) else _lib.load()
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert set(_lib.EXPORTS) == set(names)


# What the layout tests of the features asserted as literals, kept as literals: the check that does not hang on _lib's own table.
# size: sizeof;  names: every field in order;  offsets: the offsetof of every field in order;  at: the offsetof of some fields.
EXPECTED_RECORDS = {
    "sh_cut_offset": dict(size=56),
    "sh_resection": dict(size=136),
    "sh_head_fit": dict(size=128),
    "sh_implant_head": dict(size=16, at={"thickness": 8}),
    "sh_seat": dict(size=232, at={"base_radius": 0},
                    names=["base_radius", "seat_center", "covered_area", "coverage", "overhang_area", "uncovered_area", "rim_min", "rim_max", "max_overhang",
                           "max_uncovered", "overhang_dir", "uncovered_dir", "implant_center", "cor_shift", "cor_shift_articular", "surface_rms", "center_inside",
                           "status"]),
    "sh_canal_grid": dict(size=24, at={"L": 16, "A": 20}),
    "sh_canal_level": dict(size=104, names=["r_min", "r_max", "r_mean", "area", "centroid", "extent_x", "extent_y", "wall_min", "a_min", "a_max", "n_hit",
                                            "status"]),
    "sh_stem": dict(size=24, at={"r_tip": 16}),
    "sh_stem_fit": dict(size=128, names=["entry", "z_entry", "min_clearance", "depth", "direction", "scale_max", "fill_mean", "fill_max", "fill_max_depth",
                                         "angle_index", "n_samples", "n_breach", "n_open", "fits", "status"]),
    "sh_plan_rule": dict(size=96),
    "sh_plan_ref": dict(size=96),
    "sh_plan": dict(size=112),      # twelve doubles and four int32
    "sh_ray": dict(size=48),
    "sh_ray_hit": dict(size=40, offsets=[0, 8, 32, 36]),
    "sh_closest": dict(size=48, names=["dist", "point", "face", "region", "side", "status"], offsets=[0, 8, 32, 36, 40, 44]),
    "sh_winding": dict(size=16, names=["winding", "inside", "status"], offsets=[0, 8, 12]),
    "sh_icp_options": dict(size=24, names=["metric", "max_iter", "reject", "tol"], offsets=[0, 4, 8, 16]),
    "sh_registration": dict(size=168, names=["T", "rms", "rms_first", "min_pivot", "pairs", "iterations", "converged", "status"],
                            offsets=[0, 128, 136, 144, 152, 156, 160, 164]),
    "sh_mass": dict(size=400),
    "sh_sample_options": dict(size=16),
    "sh_sample": dict(size=48),
    "sh_sample_info": dict(size=24),
    "sh_topology_options": dict(size=12),
    "sh_topology": dict(size=64),
    "sh_shell": dict(size=48),
}
EXPECTED_CONSTANTS = dict(
    STEM_MAX=64, PLAN_MAX=64, RAY_MAX=65536, RAY_MAX_HITS=1024, CLOSEST_MAX=1048576, WINDING_MAX=1048576, WIND_BLOCK=2048,
    ICP_POINT=0, ICP_PLANE=1, ICP_BLOCK=256, ICP_MAX_ITER=64, MASS_BLOCK=256, MS_MAX_STARTS=64,
    SAMPLE_MAX=1048576, SAMPLE_THIN_MAX=65536, SAMPLE_BLOCK=256, THIN_MAX_ROUNDS=32,
    ADJ_BORDER=-1, ADJ_NONMANIFOLD=-2, ADJ_DEGENERATE=-3, TOPO_MAX_SHELLS=65536, TOPO_MAX_ROUNDS=32, TOPO_WATERTIGHT=1, TOPO_CONSISTENT=2)


@pytest.mark.parametrize("cname", list(abi_probe.header()[0]))
def test_record_layout_matches_header(cname):
    """Every record of the header, every field of it: sizeof and offsetof of a C compile of the header equal those of the
    ctypes.Structure and of the NumPy dtype, and the three name the fields in the same order."""
    sizes, offsets, _ = abi_probe.probe()
    cls, dtype = _lib.RECORDS[cname]
    names = abi_probe.header()[0][cname]
    assert names == [n for n, _ in cls._fields_] == list(dtype.names) == list(offsets[cname])
    assert sizes[cname] == ctypes.sizeof(cls) == dtype.itemsize
    for n in names:
        assert offsets[cname][n] == getattr(cls, n).offset == dtype.fields[n][1], n
    want = EXPECTED_RECORDS.get(cname, {})
    assert sizes[cname] == want.get("size", sizes[cname])
    assert names == want.get("names", names)
    assert [offsets[cname][n] for n in names] == want.get("offsets", [offsets[cname][n] for n in names])
    for n, off in want.get("at", {}).items():
        assert offsets[cname][n] == off, n


def test_header_and_binding_name_the_same_records_and_constants():
    """A record, a #define or a mirrored enum member that only one of include/shoulder_hip.h and _lib knows fails here; the values
    are those of the C compile."""
    records, defines, enums = abi_probe.header()
    values = abi_probe.probe()[2]
    assert set(records) == set(_lib.RECORDS) == set(abi_probe.probe()[0]) and len(records) == 27 and "sh_status" not in records
    assert set(EXPECTED_RECORDS) <= set(records)
    mirrored = {k: v for k, v in vars(_lib).items() if re.fullmatch(r"[A-Z][A-Z0-9_]*", k) and type(v) in (int, float)}
    assert set(defines) == {"SH_" + k for k in mirrored if "SH_" + k not in enums}
    for k, v in mirrored.items():
        assert values["SH_" + k] == v, k
    for n in enums:                                                                     # (the members of sh_status are not mirrored)
        assert hasattr(_lib, n[3:]) == n.startswith(("SH_STAGE_", "SH_UNET_", "SH_BONE_", "SH_OPEN_")), n
    assert {k: mirrored[k] for k in EXPECTED_CONSTANTS} == EXPECTED_CONSTANTS


def test_ctx_create_fails_loudly_without_gpu():
    """No HIP device here (or a bad index): the call reports an error instead of falling back."""
    L = _lib.load()
    h = ctypes.c_void_p()
    rc = L.sh_ctx_create(9999, None, ctypes.byref(h))
    assert rc != 0 and not h.value


def test_collective_entry_points_check_their_arguments_without_a_gpu():
    """sh_comm_init_all / sh_bcast_weights / sh_gather_landmarks: exported, and an empty group is an argument error
    (RCCL itself is only loaded once a group of real contexts asks for it)."""
    L = _lib.load()
    assert L.sh_comm_init_all(None, 0) == -1 and L.sh_bcast_weights(None, 0, 0) == -1 and L.sh_gather_landmarks(None, 0, None) == -1
    import subprocess
    deps = subprocess.run(["ldd", _lib.lib_path()], capture_output=True, text=True).stdout
    assert "rccl" not in deps


def test_packed_record_layout():
    """sh_set_record_rows(R): the NumPy mirror of the packed wire record has the library's size and keeps the field order of the
    full record around the point list (head | six trailing int32 | R rows)."""
    L = ctypes.CDLL(_lib.lib_path()) if os.path.exists(_lib.lib_path()) else _lib.load()
    L.sh_record_bytes.restype = ctypes.c_size_t
    L.sh_record_bytes.argtypes = [ctypes.c_int]
    full = _lib.LANDMARKS_DTYPE
    assert L.sh_record_bytes(0) == full.itemsize
    for R in (1, 1024, 1536, 4096):
        dt = _lib.record_dtype(R)
        assert dt.itemsize == L.sh_record_bytes(R) == 8680 + 24 * R
        for name in full.names:
            if name == "anp_points":
                continue
            off = full.fields[name][1]
            assert dt.fields[name][1] == (off if off < full.fields["anp_points"][1] else off - 4096 * 24), name
        assert dt.fields["anp_points"][1] == 8680 and dt["anp_points"].shape == (R, 3)
