"""The named-buffer lists of shoulder_amd/csrc/sh_arthro.h and sh_query.h, walked through the structs SH_BUF_LIST declares for them
(tests/hostcheck/buflist_check.cpp, a stand-alone program; no GPU): field, name and element size of every buffer, in list order, against
the table written out here.  The names and element sizes are what sh_fetch and sh_buffer_info see."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "hostcheck", "buflist_check.cpp")

# list: (field, name, elem) in list order
TABLE = {
    "chain": [
        ("planes", "resect.planes", 8), ("status", "resect.status", 4), ("slab", "resect.slab", 8), ("segcnt", "resect.segcnt", 4),
        ("segs", "resect.segs", 4), ("out", "resect.out", 8), ("one", "resect.one", 8), ("ring", "resect.ring", 8), ("offs", "resect.offs", 8),
        ("fit_slab", "resect.fit_slab", 8), ("fit_moments", "resect.fit_moments", 8), ("fit_ring", "resect.fit_ring", 8),
        ("fit_out", "resect.fit_out", 8), ("seat_ring", "resect.seat_ring", 8), ("seat_heads", "resect.seat_heads", 8),
        ("seat_out", "resect.seat_out", 8),
        ("canal_near", "canal.near", 8), ("canal_far", "canal.far", 8), ("canal_levels", "canal.levels", 8), ("canal_frames", "canal.frames", 8),
        ("canal_status", "canal.status", 4), ("canal_dirs", "canal.dirs", 8),
        ("stem_catalogue", "stem.catalogue", 8), ("stem_out", "stem.out", 8),
        ("plan_ref_planes", "plan.ref_planes", 8), ("plan_compat", "plan.compat", 8), ("plan_ref_slab", "plan.ref_slab", 8), ("plan_ref", "plan.ref", 8),
        ("plan_cut_terms", "plan.cut_terms", 8), ("plan_head_terms", "plan.head_terms", 8), ("plan_stem_terms", "plan.stem_terms", 8),
        ("plan_cut_vals", "plan.cut_vals", 8), ("plan_head_vals", "plan.head_vals", 8), ("plan_stem_vals", "plan.stem_vals", 8), ("plan_out", "plan.out", 8)],
    "ray": [
        ("ray_rays", "ray.rays", 8), ("ray_status", "ray.status", 4), ("ray_counts", "ray.counts", 4), ("ray_offs", "ray.offs", 8),
        ("ray_cursor", "ray.cursor", 4), ("ray_pool", "ray.pool", 8), ("ray_hits", "ray.hits", 8), ("ray_blockhit", "ray.blockhit", 4)],
    "closest": [("cp_points", "cp.points", 8), ("cp_part", "cp.part", 8), ("cp_out", "cp.out", 8)],
    "winding": [("wn_points", "wn.points", 8), ("wn_part", "wn.part", 8), ("wn_out", "wn.out", 8)],
    "registration": [
        ("icp_points", "icp.points", 8), ("icp_moved", "icp.moved", 8), ("icp_cp_part", "icp.cp_part", 8), ("icp_near", "icp.near", 8),
        ("icp_part", "icp.part", 8), ("icp_T", "icp.T", 8), ("icp_hist", "icp.hist", 8), ("icp_flags", "icp.flags", 4), ("icp_out", "icp.out", 8)],
    "mass": [("mass_part", "mass.part", 8), ("mass_out", "mass.out", 8)],
    "multistart": [("ms_T0s", "ms.T0s", 8), ("ms_points", "ms.points", 8), ("ms_coarse", "ms.coarse", 8), ("ms_best", "ms.best", 8), ("ms_winner", "ms.winner", 4)],
}


def test_every_list_walks_its_buffers_in_order(tmp_path):
    assert [len(TABLE[k]) for k in ("chain", "ray", "closest", "winding", "registration", "mass", "multistart")] == [35, 8, 3, 3, 9, 2, 5]
    exe = tmp_path / "buflist_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe), SRC])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.stdout[-300:], run.stderr[-2000:])
    want = [f"{title} {field} {name} {elem}" for title, rows in TABLE.items() for field, name, elem in rows]
    assert run.stdout.splitlines() == want
