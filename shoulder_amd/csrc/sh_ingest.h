// sh_ingest.h -- what mesh ingest decides on the host before a batch becomes resident: are the arrays / STL headers / merged sizes
// acceptable, and which offsets and table size follow from them.  No kernels, no HIP types: shoulder_hip.hip includes it, and so does a
// plain g++ (tests/hostcheck/ingest_check.cpp).  An error is a code plus the text BEHIND the entry point's name: the caller puts
// "sh_upload_stl: " (or the name it was called under) in front.
#pragma once
#include "../../include/shoulder_hip.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace sh {

struct IngestError { int code; const char* text; };      // code SH_OK: accepted (text null)
struct MeshSizes { long long sumV = 0, sumF = 0, maxV = 0, maxF = 0; };

// The arrays of sh_upload_meshes / sh_stage_meshes: offsets start at 0; mesh by mesh at least 4 vertices and faces, at most
// 0x7fffffff / 3 of each, then (faces != null) that mesh's face indices inside it; behind all meshes (verts != null) every coordinate
// finite.  The staged call passes null for both: its elements are checked on the device (k_validate_meshes).
inline IngestError check_mesh_arrays(const int64_t* v_off, const int64_t* f_off, int B, const int32_t* faces, const float* verts, MeshSizes* out) {
  if (v_off[0] != 0 || f_off[0] != 0) return {SH_ERR_ARG, "offsets must start at 0"};
  MeshSizes s;
  for (int b = 0; b < B; ++b) {
    const long long nv = v_off[b + 1] - v_off[b], nf = f_off[b + 1] - f_off[b];
    if (nv < 4 || nf < 4) return {SH_ERR_ARG, "a mesh has fewer than 4 vertices/faces"};
    if (nv > 0x7fffffffLL / 3 || nf > 0x7fffffffLL / 3) return {SH_ERR_ARG, "a mesh is too large"};
    s.maxV = nv > s.maxV ? nv : s.maxV; s.maxF = nf > s.maxF ? nf : s.maxF;
    if (faces)
      for (long long i = 3 * f_off[b]; i < 3 * f_off[b + 1]; ++i)
        if (faces[i] < 0 || faces[i] >= nv) return {SH_ERR_ARG, "face index out of range"};
  }
  s.sumV = v_off[B]; s.sumF = f_off[B];
  if (verts)
    for (long long i = 0; i < 3 * s.sumV; ++i)
      if (!std::isfinite(verts[i])) return {SH_ERR_ARG, "NaN / infinite vertex coordinate"};
  *out = s;
  return {SH_OK, nullptr};
}

// Where B binary STL files go in one image (file starts padded to 4 bytes) and in the corner list (3 per triangle), the largest corner
// count and the size of a mesh's hash table: the smallest power of two >= 2 maxc, at least 1024.
struct StlPlan { std::vector<long long> file_off, coff; long long maxc = 0, sumC = 0; int tsize = 0; };

inline int stl_table_size(long long maxc) { int t = 1024; while (t < 2 * maxc) t <<= 1; return t; }

// reads bytes 80..83 of each file (the triangle count) and nbytes[b], nothing else
inline IngestError stl_plan(const void* const* files, const size_t* nbytes, int B, StlPlan* out) {
  StlPlan p;
  p.file_off.assign(B + 1, 0); p.coff.assign(B + 1, 0);
  for (int b = 0; b < B; ++b) {
    if (!files[b] || nbytes[b] < 84) return {SH_ERR_ARG, "a file is too short for a binary STL"};
    uint32_t nt;
    memcpy(&nt, (const char*)files[b] + 80, 4);
    if (nbytes[b] != 84 + 50ull * nt) return {SH_ERR_ARG, "not a binary STL (size does not match the triangle count)"};
    if (nt < 4 || nt > 0x7fffffffu / 3) return {SH_ERR_ARG, "a mesh has fewer than 4 (or too many) triangles"};
    p.file_off[b + 1] = p.file_off[b] + (long long)((nbytes[b] + 3) & ~(size_t)3);
    p.coff[b + 1] = p.coff[b] + 3ll * nt;
    p.maxc = 3ll * nt > p.maxc ? 3ll * nt : p.maxc;
  }
  p.tsize = stl_table_size(p.maxc);
  p.sumC = p.coff[B];
  *out = std::move(p);
  return {SH_OK, nullptr};
}

// What the device counted (counts[2 b], counts[2 b + 1]: merged vertices, kept faces of file b; nonfinite[b]: it holds a NaN / inf)
// -> the offsets and sizes of the merged batch, or why it is refused.
inline IngestError stl_counted(const int* counts, const int* nonfinite, int B, std::vector<long long>* voff, std::vector<long long>* foff, MeshSizes* out) {
  voff->assign(B + 1, 0); foff->assign(B + 1, 0);
  MeshSizes s;
  for (int b = 0; b < B; ++b) {
    const long long nv = counts[2 * b], nf = counts[2 * b + 1];
    if (nonfinite[b]) return {SH_ERR_ARG, "a file holds NaN / infinite coordinates"};
    if (nv < 4 || nf < 4) return {SH_ERR_ARG, "a mesh has fewer than 4 vertices/faces after merging"};
    (*voff)[b + 1] = (*voff)[b] + nv;
    (*foff)[b + 1] = (*foff)[b] + nf;
    s.maxV = nv > s.maxV ? nv : s.maxV; s.maxF = nf > s.maxF ? nf : s.maxF;
  }
  s.sumV = (*voff)[B]; s.sumF = (*foff)[B];
  *out = s;
  return {SH_OK, nullptr};
}

}  // namespace sh
