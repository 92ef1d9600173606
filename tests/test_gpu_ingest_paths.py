"""The ways a batch becomes resident (sh_upload_stl, sh_stage_stl + commit, sh_upload_meshes, sh_stage_meshes + commit) share one
STL plan, one parse chain and one commit: the same two meshes handed over each way give the same device bytes, from pageable and from
page-locked caller memory; the parse kernels are timed once per synchronous upload and never by the staged thread; a rejected
hand-over leaves the resident batch as it was.  No stage runs, so no forest and no network are loaded."""
import contextlib
import ctypes
import os
import struct

import numpy as np
import pytest

from conftest import BONES
from shoulder_amd.engine import Engine, ShoulderHipError
from shoulder_amd.stl import load_stl

pytestmark = pytest.mark.gpu
STL_BUFFERS = ["stl.raw", "stl.file_off", "stl.coff", "stl.corners", "stl.table", "stl.slot", "stl.vid", "stl.fpos", "stl.counts", "stl.bsum", "stl.nonfinite"]
PARSE_KERNELS = ["k_stl_corners", "k_stl_table_init", "k_stl_hash", "k_stl_emit"]


def _stl_bytes(tris):
    tris = np.asarray(tris, dtype=np.float32)
    out = bytearray(b"x" * 80) + struct.pack("<I", len(tris))
    for t in tris:
        out += struct.pack("<12fH", 0, 0, 0, *t.reshape(-1), 0)
    return bytes(out)


def _blob_tris():
    """the 7 triangles of test_gpu_stl.test_merge_edge_cases: +-0.0, a degenerate triangle, an odd count (the next file starts padded)"""
    a, b, c, d, e = [0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]
    nz = [-0.0, 0.0, -0.0]
    return [[a, b, c], [nz, c, d], [b, b, e], [a, d, b], [c, b, e], [e, d, c], [d, e, b]]


@contextlib.contextmanager
def _engine():
    e = Engine(0)
    try:
        yield e
    finally:
        e.close()


def _resident(e):
    B = e.B
    voff = e.fetch("voff", np.int64, (B + 1,)).copy()
    foff = e.fetch("foff", np.int64, (B + 1,)).copy()
    return dict(B=B, voff=voff.tobytes(), foff=foff.tobytes(),
                verts=e.fetch("verts", np.uint32, (int(voff[-1]), 3)).tobytes(), faces=e.fetch("faces", np.int32, (int(foff[-1]), 3)).tobytes())


def _stl_info(e):
    out = {}
    for name in STL_BUFFERS:
        n, el = ctypes.c_size_t(), ctypes.c_int()
        e._chk(e.L.sh_buffer_info(e.h, name.encode(), ctypes.byref(n), ctypes.byref(el)))
        out[name] = (n.value, el.value)
    return out


@pytest.fixture(scope="module")
def batch(tmp_path_factory):
    """the two files, as images and as host-merged meshes"""
    blob = _stl_bytes(_blob_tris())
    p = tmp_path_factory.mktemp("ingest") / "blob.stl"
    p.write_bytes(blob)
    cut = os.path.join(BONES, "proximal_left_cut.stl")
    files = [blob, open(cut, "rb").read()]
    assert len(files[0]) % 4 == 2      # (the second file starts on a padded offset)
    return dict(files=files, meshes=[load_stl(str(p)), load_stl(cut)])


@pytest.fixture(scope="module")
def reference(batch):
    """four fresh engines, one per way in: the resident bytes of each (and the stl.* buffers of the two STL ways)"""
    got, info = {}, {}
    with _engine() as e:
        e.upload_stl(batch["files"])
        got["upload_stl"], info["upload_stl"] = _resident(e), _stl_info(e)
    with _engine() as e:
        e.stage_stl(batch["files"]); e.commit_staged()
        got["stage_stl"], info["stage_stl"] = _resident(e), _stl_info(e)
    with _engine() as e:
        e.upload(batch["meshes"])
        got["upload"] = _resident(e)
    with _engine() as e:
        e.stage(batch["meshes"]); e.commit_staged()
        got["stage"] = _resident(e)
    return got, info


def test_four_ways_in_one_result(reference, batch):
    got, info = reference
    hv = np.concatenate([v for v, _ in batch["meshes"]])
    assert got["upload"]["B"] == 2 and got["upload"]["verts"] == hv.view(np.uint32).tobytes()
    for way in ("upload_stl", "stage_stl", "stage"):
        for key in ("B", "voff", "foff", "verts", "faces"):
            assert got[way][key] == got["upload"][key], (way, key)
    assert info["upload_stl"] == info["stage_stl"]
    assert all(n > 0 for n, _ in info["upload_stl"].values())


@contextlib.contextmanager
def _page_locked(e, nbytes):
    p = ctypes.c_void_p()
    e._chk(e.L.sh_host_alloc(e.h, nbytes, ctypes.byref(p)))
    try:
        yield p.value
    finally:
        e.L.sh_host_free(e.h, p)


def _locked_copy(stack, e, a):
    """a copy of array `a` in page-locked memory of the library"""
    addr = stack.enter_context(_page_locked(e, a.nbytes))
    out = np.ctypeslib.as_array((ctypes.c_ubyte * a.nbytes).from_address(addr)).view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


@pytest.mark.parametrize("vpin,fpin", [(True, True), (True, False), (False, True)])
def test_page_locked_arrays(reference, batch, vpin, fpin):
    verts, faces, voff, foff = Engine.pack_meshes(batch["meshes"])
    with _engine() as e, contextlib.ExitStack() as stack:
        if vpin:
            verts = _locked_copy(stack, e, verts)
        if fpin:
            faces = _locked_copy(stack, e, faces)
        e.stage((verts, faces, voff, foff)); e.commit_staged()
        assert _resident(e) == reference[0]["upload"]


@pytest.mark.parametrize("pinned", [(True, True), (True, False), (False, True)])
def test_page_locked_files(reference, batch, pinned):
    with _engine() as e, contextlib.ExitStack() as stack:
        imgs = [np.frombuffer(f, np.uint8) for f in batch["files"]]
        imgs = [_locked_copy(stack, e, a) if pin else a for a, pin in zip(imgs, pinned)]
        ptrs = (ctypes.c_void_p * 2)(*[a.ctypes.data for a in imgs])
        sizes = (ctypes.c_size_t * 2)(*[a.nbytes for a in imgs])
        e._chk(e.L.sh_stage_stl(e.h, ptrs, sizes, 2))
        e.commit_staged()      # (the images stay alive until here: the library reads them until the commit returns)
        assert _resident(e) == reference[0]["upload"]
        assert _stl_info(e) == reference[1]["upload_stl"]


def test_parse_kernels_are_timed_once_per_upload(batch):
    with _engine() as e:
        e.enable_timing(1)
        e.reset_timers()
        e.upload_stl(batch["files"])
        assert [e.kernel_time_ms(k)[1] for k in PARSE_KERNELS] == [1, 1, 1, 1]
        e.stage_stl(batch["files"]); e.commit_staged()
        assert [e.kernel_time_ms(k)[1] for k in PARSE_KERNELS] == [1, 1, 1, 1]      # the staged thread records none
        e.upload_stl(batch["files"])
        assert [e.kernel_time_ms(k)[1] for k in PARSE_KERNELS] == [2, 2, 2, 2]


def test_rejections_leave_the_resident_batch(reference, batch):
    tris = np.array(_blob_tris(), np.float32)
    nan_tris = tris.copy(); nan_tris[4, 1, 2] = np.nan
    nan_file, three = _stl_bytes(nan_tris), _stl_bytes(tris[:3])
    (v0, f0), m1 = batch["meshes"]
    bad_faces = f0.copy(); bad_faces[2, 1] = len(v0)

    def staged_nan(e):
        e.stage_stl([batch["files"][1], nan_file])      # accepted by the call: the device finds the NaN, the commit reports it
        e.commit_staged()

    attempts = [(lambda e: e.upload_stl([batch["files"][1], nan_file]), "sh_upload_stl: a file holds NaN / infinite coordinates"),
                (staged_nan, "sh_stage_stl: a file holds NaN / infinite coordinates"),
                (lambda e: e.upload([(v0, bad_faces), m1]), "sh_upload_meshes: face index out of range"),
                (lambda e: e.upload_stl([three]), "sh_upload_stl: a mesh has fewer than 4 (or too many) triangles")]
    with _engine() as e:
        e.upload(batch["meshes"])
        before = _resident(e)
        assert before == reference[0]["upload"]
        for attempt, text in attempts:
            with pytest.raises(ShoulderHipError) as err:
                attempt(e)
            assert err.value.code == -1 and str(err.value) == f"libshoulder_hip error -1: {text}"
            assert not e.staged
            assert _resident(e) == before, text
