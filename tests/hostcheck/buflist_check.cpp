// Test program (NOT product): every named-buffer list of shoulder_amd/csrc/sh_arthro.h and sh_query.h, walked through the structs that
// SH_BUF_LIST declares for it, for tests/test_buflist_host.py.  Prints one line per buffer, `list field name elem`, from the walk of the
// list's Bytes struct; the walk of its View must give the mesh's five pointers and then the same fields in the same order (exit 1).
#include "../../shoulder_amd/csrc/sh_query.h"
#include <cstdio>
#include <string>
#include <vector>
using namespace sh;

template <typename Bytes, typename View>
static bool list(const char* title, size_t mesh_fields = 5) {
  std::vector<std::string> sized, viewed;
  Bytes z;
  z.each([&](size_t bytes, const char* field, const char* name, int elem) {
    printf("%s %s %s %d\n", title, field, name, elem);
    sized.push_back(std::string(field) + " " + name + (bytes ? " not zero" : ""));
  });
  View v;
  v.each([&](auto* p, const char* field, const char* name, auto...) { viewed.push_back(std::string(field) + " " + name + (p ? " not null" : "")); });
  const std::vector<std::string> mesh = {"verts verts", "faces faces", "voff voff", "foff foff", "lm landmarks"};
  if (viewed.size() != mesh_fields + sized.size() || !std::equal(mesh.begin(), mesh.begin() + mesh_fields, viewed.begin()) ||
      !std::equal(sized.begin(), sized.end(), viewed.begin() + mesh_fields)) {
    printf("buflist_check: the view of %s does not walk the mesh and then the list\n", title);
    return false;
  }
  return true;
}

int main() {
  const bool ok = list<ArthroBytes, ArthroView>("chain") && list<RayBytes, RayView>("ray") && list<CpBytes, CpView>("closest") && list<WnBytes, WnView>("winding") &&
                  list<IcpBytes, IcpView>("registration") && list<MassBytes, MassView>("mass") && list<MsBytes, MsBufs>("multistart", 0);
  return ok ? 0 : 1;
}
