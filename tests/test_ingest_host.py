"""The host decisions of mesh ingest (shoulder_amd/csrc/sh_ingest.h: what sh_upload_meshes / sh_stage_meshes check of the arrays,
what sh_upload_stl / sh_stage_stl plan from the STL headers and conclude from the device's counts), without a GPU.  The expected
values are the rules the five entry points applied so far, written out here: which error comes FIRST, its text behind the entry
point's name, and the offsets / sizes / table size of an accepted input."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "shoulder_amd", "csrc")
ERR_ARG = -1
BIG = 0x7FFFFFFF // 3
E_START = "offsets must start at 0"
E_SMALL = "a mesh has fewer than 4 vertices/faces"
E_LARGE = "a mesh is too large"
E_INDEX = "face index out of range"
E_NAN = "NaN / infinite vertex coordinate"
E_SHORT = "a file is too short for a binary STL"
E_SIZE = "not a binary STL (size does not match the triangle count)"
E_TRIS = "a mesh has fewer than 4 (or too many) triangles"
E_FILE_NAN = "a file holds NaN / infinite coordinates"
E_MERGED = "a mesh has fewer than 4 vertices/faces after merging"


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("ingest_check") / "libingest_check.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(so),
                           os.path.join(ROOT, "tests", "hostcheck", "ingest_check.cpp")])
    L = ctypes.CDLL(str(so))
    vp, txt = ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p)
    L.ic_arrays.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, txt]
    L.ic_plan.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, txt]
    L.ic_counted.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp, txt]
    L.ic_table_size.argtypes = [ctypes.c_longlong]
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _text(t):
    return t.value.decode() if t.value else None


def test_header_builds_with_gxx_alone(tmp_path):
    """compile-only: sh_ingest.h needs no HIP header and no hipcc"""
    src = tmp_path / "probe.cpp"
    src.write_text('#include "sh_ingest.h"\nint main() { sh::StlPlan p; sh::MeshSizes s; return (int)p.maxc + (int)s.sumV; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)])


# ---- arrays ----------------------------------------------------------------------------------------------------------
def arrays(L, voff, foff, faces, verts, elements=True):
    voff, foff = np.asarray(voff, np.int64), np.asarray(foff, np.int64)
    faces, verts = np.ascontiguousarray(faces, np.int32), np.ascontiguousarray(verts, np.float32)
    sizes, t = np.zeros(4, np.int64), ctypes.c_char_p()
    rc = L.ic_arrays(_p(voff), _p(foff), len(voff) - 1, _p(faces) if elements else None, _p(verts) if elements else None, _p(sizes), ctypes.byref(t))
    return rc, _text(t), (tuple(int(x) for x in sizes) if rc == 0 else None)


def parent_arrays(voff, foff, faces, verts, elements=True):
    """sh_upload_meshes at the parent commit (elements=False: sh_stage_meshes, whose elements the device checks)"""
    B = len(voff) - 1
    faces = np.asarray(faces).reshape(-1)
    if voff[0] != 0 or foff[0] != 0:
        return ERR_ARG, E_START, None
    maxV = maxF = 0
    for b in range(B):
        nv, nf = voff[b + 1] - voff[b], foff[b + 1] - foff[b]
        if nv < 4 or nf < 4:
            return ERR_ARG, E_SMALL, None
        if nv > BIG or nf > BIG:
            return ERR_ARG, E_LARGE, None
        maxV, maxF = max(maxV, nv), max(maxF, nf)
        if elements:
            f = faces[3 * foff[b]:3 * foff[b + 1]]
            if ((f < 0) | (f >= nv)).any():
                return ERR_ARG, E_INDEX, None
    if elements and not np.isfinite(np.asarray(verts, np.float32).reshape(-1)[:3 * voff[B]]).all():
        return ERR_ARG, E_NAN, None
    return 0, None, (int(voff[B]), int(foff[B]), int(maxV), int(maxF))


def _two_meshes():
    """mesh 0: 5 vertices, 4 faces; mesh 1: 4 vertices, 6 faces (indices local to each mesh)"""
    verts = np.arange(27, dtype=np.float32).reshape(9, 3)
    faces = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4], [4, 0, 1], [0, 1, 2], [1, 2, 3], [3, 0, 1], [2, 3, 0], [0, 2, 1], [3, 1, 0]], np.int32)
    return [0, 5, 9], [0, 4, 10], faces, verts


def _with(base, **kw):
    voff, foff, faces, verts = base
    d = dict(voff=list(voff), foff=list(foff), faces=faces.copy(), verts=verts.copy())
    for k, fn in kw.items():
        fn(d[k])
    return d["voff"], d["foff"], d["faces"], d["verts"]


def _set(i, v):
    def fn(a):
        a.reshape(-1)[i] = v
    return fn


ARRAY_CASES = {
    "good": (lambda b: b, 0, None),
    "start_v": (lambda b: _with(b, voff=lambda a: a.__setitem__(0, 1)), ERR_ARG, E_START),
    "start_f": (lambda b: _with(b, foff=lambda a: a.__setitem__(0, 2)), ERR_ARG, E_START),
    "three_vertices": (lambda b: ([0, 3, 7], b[1], b[2], b[3]), ERR_ARG, E_SMALL),
    "three_faces": (lambda b: (b[0], [0, 3, 9], b[2], b[3]), ERR_ARG, E_SMALL),
    # mesh 0 too large: refused before any element is read (the arrays are far shorter than the offsets claim)
    "too_large": (lambda b: ([0, BIG + 1, BIG + 5], b[1], b[2], b[3]), ERR_ARG, E_LARGE),
    "too_many_faces": (lambda b: (b[0], [0, BIG + 1, BIG + 7], b[2], b[3]), ERR_ARG, E_LARGE),
    "index_minus_one": (lambda b: _with(b, faces=_set(3 * 7 + 1, -1)), ERR_ARG, E_INDEX),
    "index_equals_nv": (lambda b: _with(b, faces=_set(3 * 5, 4)), ERR_ARG, E_INDEX),       # mesh 1 has 4 vertices
    "index_nv_of_mesh0_is_fine_there": (lambda b: _with(b, faces=_set(0, 4)), 0, None),    # mesh 0 has 5
    "nan": (lambda b: _with(b, verts=_set(13, np.nan)), ERR_ARG, E_NAN),
    "inf": (lambda b: _with(b, verts=_set(26, -np.inf)), ERR_ARG, E_NAN),
    # precedence: mesh by mesh (sizes, then that mesh's indices), the coordinates behind all meshes
    "bad_index_in_0_beats_small_1": (lambda b: _with(([0, 5, 8], b[1], b[2], b[3]), faces=_set(2, 5)), ERR_ARG, E_INDEX),
    "small_0_beats_bad_index_in_1": (lambda b: _with(([0, 3, 9], b[1], b[2], b[3]), faces=_set(3 * 5, -1)), ERR_ARG, E_SMALL),
    "bad_index_beats_nan": (lambda b: _with(b, faces=_set(3 * 9, 7), verts=_set(0, np.nan)), ERR_ARG, E_INDEX),
    "small_1_beats_nan": (lambda b: _with((b[0], [0, 7, 10], b[2], b[3]), verts=_set(0, np.nan)), ERR_ARG, E_SMALL),
}


@pytest.mark.parametrize("name", sorted(ARRAY_CASES))
def test_arrays(shim, name):
    make, code, text = ARRAY_CASES[name]
    voff, foff, faces, verts = make(_two_meshes())
    want = parent_arrays(voff, foff, faces, verts)
    assert want[:2] == (code, text)      # (the table and the written-out rules agree)
    assert arrays(shim, voff, foff, faces, verts) == want
    if name == "good":
        assert want[2] == (9, 10, 5, 6)


@pytest.mark.parametrize("name", sorted(ARRAY_CASES))
def test_arrays_offsets_only(shim, name):
    """the staged call: the same offset rules, no element is looked at"""
    voff, foff, faces, verts = ARRAY_CASES[name][0](_two_meshes())
    want = parent_arrays(voff, foff, faces, verts, elements=False)
    assert want[1] in (None, E_START, E_SMALL, E_LARGE)
    assert arrays(shim, voff, foff, faces, verts, elements=False) == want


# ---- STL headers -----------------------------------------------------------------------------------------------------
def _stl(nt, nbytes=None):
    """(image, size handed over): a header that claims nt triangles; the image is as long as the size says, up to 84 + 50 nt"""
    n = 84 + 50 * nt if nbytes is None else nbytes
    img = (b"h" * 80 + struct.pack("<I", nt) + b"\0" * max(0, min(n, 84 + 50 * nt) - 84))
    return img, n


def plan(L, files):
    """files: list of (bytes or None, nbytes)"""
    B = len(files)
    keep = [f for f, _ in files]
    ptrs = (ctypes.c_void_p * B)(*[ctypes.cast(ctypes.c_char_p(k), ctypes.c_void_p) if k is not None else None for k in keep])
    sizes = (ctypes.c_size_t * B)(*[n for _, n in files])
    fo, co, pl, t = np.zeros(B + 1, np.int64), np.zeros(B + 1, np.int64), np.zeros(3, np.int64), ctypes.c_char_p()
    rc = L.ic_plan(ptrs, sizes, B, _p(fo), _p(co), _p(pl), ctypes.byref(t))
    return rc, _text(t), (dict(file_off=fo.tolist(), coff=co.tolist(), maxc=int(pl[0]), sumC=int(pl[1]), tsize=int(pl[2])) if rc == 0 else None)


def parent_table_size(maxc):
    t = 1024
    while t < 2 * maxc:
        t <<= 1
    return t


def parent_plan(files):
    """the header scan of sh_upload_stl / sh_stage_stl at the parent commit"""
    fo, co, maxc = [0], [0], 0
    for img, n in files:
        if img is None or n < 84:
            return ERR_ARG, E_SHORT, None
        nt = struct.unpack_from("<I", img, 80)[0]
        if n != 84 + 50 * nt:
            return ERR_ARG, E_SIZE, None
        if nt < 4 or nt > 0x7FFFFFFF // 3:
            return ERR_ARG, E_TRIS, None
        fo.append(fo[-1] + ((n + 3) & ~3))
        co.append(co[-1] + 3 * nt)
        maxc = max(maxc, 3 * nt)
    return 0, None, dict(file_off=fo, coff=co, maxc=maxc, sumC=co[-1], tsize=parent_table_size(maxc))


STL_CASES = {
    "83_bytes": ([(b"x" * 83, 83)], E_SHORT),
    "null_file": ([_stl(7), (None, 434)], E_SHORT),
    "one_byte_short": ([_stl(7, 433)], E_SIZE),
    "one_byte_long": ([_stl(7), _stl(5, 335)], E_SIZE),
    "three_triangles": ([_stl(3)], E_TRIS),
    # an 84-byte header and a size to match its claim: only bytes 80..83 are read
    "too_many_triangles": ([_stl(BIG + 1, 84)[:1] + (84 + 50 * (BIG + 1),)], E_TRIS),
    "first_error_wins": ([_stl(3), (None, 0)], E_TRIS),
}


@pytest.mark.parametrize("name", sorted(STL_CASES))
def test_stl_headers(shim, name):
    files, text = STL_CASES[name]
    want = parent_plan(files)
    assert want[:2] == (ERR_ARG, text)
    assert plan(shim, files) == want


def test_three_file_plan(shim):
    files = [_stl(7), _stl(4), _stl(342)]
    rc, text, p = plan(shim, files)
    assert (rc, text) == (0, None)
    assert p["file_off"] == [0, 436, 720, 17904]      # 7 * 50 + 84 = 434 pads to 436
    assert p["coff"] == [0, 21, 33, 1059]
    assert p["maxc"] == 1026 and p["sumC"] == 1059 and p["tsize"] == 4096
    assert (rc, text, p) == parent_plan(files)


def test_table_size(shim):
    assert shim.ic_table_size(512) == 1024 and shim.ic_table_size(513) == 2048
    for maxc in (0, 12, 511, 512, 513, 1024, 1025, 1026, 3 * 50000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 29):
        assert shim.ic_table_size(maxc) == parent_table_size(maxc), maxc


# ---- what the device counted -----------------------------------------------------------------------------------------
def counted(L, counts, nonfin):
    B = len(nonfin)
    c, n = np.asarray(counts, np.int32).reshape(-1), np.asarray(nonfin, np.int32)
    vo, fo, sizes, t = np.zeros(B + 1, np.int64), np.zeros(B + 1, np.int64), np.zeros(4, np.int64), ctypes.c_char_p()
    rc = L.ic_counted(_p(c), _p(n), B, _p(vo), _p(fo), _p(sizes), ctypes.byref(t))
    return rc, _text(t), ((vo.tolist(), fo.tolist(), tuple(int(x) for x in sizes)) if rc == 0 else None)


def parent_counted(counts, nonfin):
    vo, fo = [0], [0]
    for (nv, nf), bad in zip(counts, nonfin):
        if bad:
            return ERR_ARG, E_FILE_NAN, None
        if nv < 4 or nf < 4:
            return ERR_ARG, E_MERGED, None
        vo.append(vo[-1] + nv)
        fo.append(fo[-1] + nf)
    return 0, None, (vo, fo, (vo[-1], fo[-1], max(c[0] for c in counts), max(c[1] for c in counts)))


GOOD = [(5, 6), (2502, 5000), (4, 4)]
COUNTED_CASES = {
    "good": (GOOD, [0, 0, 0], None),
    "nonfinite_file_1_of_3": (GOOD, [0, 1, 0], E_FILE_NAN),
    "three_vertices": ([(5, 6), (3, 9), (4, 4)], [0, 0, 0], E_MERGED),
    "three_faces": ([(9, 3)], [0], E_MERGED),
    "small_0_beats_nonfinite_1": ([(3, 9), (5, 6)], [0, 1], E_MERGED),
    "nonfinite_beats_its_own_counts": ([(5, 6), (3, 3)], [0, 2], E_FILE_NAN),
}


@pytest.mark.parametrize("name", sorted(COUNTED_CASES))
def test_counted(shim, name):
    counts, nonfin, text = COUNTED_CASES[name]
    want = parent_counted(counts, nonfin)
    assert want[:2] == ((ERR_ARG, text) if text else (0, None))
    assert counted(shim, counts, nonfin) == want
    if name == "good":
        assert want[2] == ([0, 5, 2507, 2511], [0, 6, 5006, 5010], (2511, 5010, 2502, 5000))
