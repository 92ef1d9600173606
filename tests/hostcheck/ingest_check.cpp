// Test shim (NOT product): the host decisions of mesh ingest (shoulder_amd/csrc/sh_ingest.h) for tests/test_ingest_host.py.
// Every call returns the error code and *text (the text behind the entry point's name, null when accepted).
// sizes: sumV, sumF, maxV, maxF.  plan: maxc, sumC, tsize.
#include "../../shoulder_amd/csrc/sh_ingest.h"
#include <algorithm>
extern "C" {
int ic_arrays(const int64_t* v_off, const int64_t* f_off, int B, const int32_t* faces, const float* verts, long long* sizes, const char** text) {
  sh::MeshSizes s;
  const sh::IngestError e = sh::check_mesh_arrays(v_off, f_off, B, faces, verts, &s);
  *text = e.text;
  if (e.code == SH_OK) { sizes[0] = s.sumV; sizes[1] = s.sumF; sizes[2] = s.maxV; sizes[3] = s.maxF; }
  return e.code;
}
int ic_plan(const void* const* files, const size_t* nbytes, int B, long long* file_off, long long* coff, long long* plan, const char** text) {
  sh::StlPlan p;
  const sh::IngestError e = sh::stl_plan(files, nbytes, B, &p);
  *text = e.text;
  if (e.code == SH_OK) {
    std::copy(p.file_off.begin(), p.file_off.end(), file_off); std::copy(p.coff.begin(), p.coff.end(), coff);
    plan[0] = p.maxc; plan[1] = p.sumC; plan[2] = p.tsize;
  }
  return e.code;
}
int ic_table_size(long long maxc) { return sh::stl_table_size(maxc); }
int ic_counted(const int* counts, const int* nonfinite, int B, long long* voff, long long* foff, long long* sizes, const char** text) {
  std::vector<long long> v, f;
  sh::MeshSizes s;
  const sh::IngestError e = sh::stl_counted(counts, nonfinite, B, &v, &f, &s);
  *text = e.text;
  if (e.code == SH_OK) {
    std::copy(v.begin(), v.end(), voff); std::copy(f.begin(), f.end(), foff);
    sizes[0] = s.sumV; sizes[1] = s.sumF; sizes[2] = s.maxV; sizes[3] = s.maxF;
  }
  return e.code;
}
}
