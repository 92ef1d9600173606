// sh_params.h -- the host rules of the parameters: the layout of the device parameter block "params" (the UNet's floats, then the
// forest's tables), the check that those tables describe a forest, the range checks and defaults of sh_set_params, and ParamState,
// the one record of what is loaded and which packed copies of the block are current.  No kernels, no HIP types: shoulder_hip.hip,
// unet.hip and comm.hip act on it, a plain g++ compiles it (tests/hostcheck/params_check.cpp).
#pragma once
#include "../../include/shoulder_hip.h"
#include "sh_common.h"

#include <vector>

namespace sh {

// ---- the sections of the block: the one statement of its layout -----------------------------------------------------------------------
// X(field, element type, count) in the order the sections lie in the block, nothing between them; count is a field of ParamShape.
// The byte offsets, the host mirrors, the copy in either direction (ParamMirror::each) and the forest's device view come from this list.
#define SH_PARAM_FOREST_SECTIONS(X) X(feat, int32_t, nodes) X(thr, float, nodes) X(ti, int32_t, nodes) X(fi, int32_t, nodes) X(lw, float, nodes) X(roots, int32_t, trees)
#define SH_PARAM_SECTIONS(X) X(unet, float, unet_floats) SH_PARAM_FOREST_SECTIONS(X)

struct ParamShape {
  int base = 0, depth = 0;                          // of the loaded network (0: none)
  size_t unet_floats = 0, nodes = 0, trees = 0;     // elements of the sections
  bool operator==(const ParamShape& o) const { return base == o.base && depth == o.depth && unet_floats == o.unet_floats && nodes == o.nodes && trees == o.trees; }
};
struct ParamLayout {      // the byte offset of every section and the bytes of the block
#define X(field, T, count) size_t field;
  SH_PARAM_SECTIONS(X) size_t total = 0;
#undef X
#define X(field, T, count) field = total; total += s.count * sizeof(T);
  explicit ParamLayout(const ParamShape& s) { SH_PARAM_SECTIONS(X) }
#undef X
};
struct ParamMirror {      // the host copy of every section: what a load re-uploads the whole block from
#define X(field, T, count) std::vector<T> field;
  SH_PARAM_SECTIONS(X)
#undef X
#define X(field, T, count) field.resize(s.count);
  void resize(const ParamShape& s) { SH_PARAM_SECTIONS(X) }
#undef X
#define X(field, T, count) fn((void*)field.data(), L.field, field.size() * sizeof(T));
  template <typename F> void each(const ParamLayout& L, F&& fn) { SH_PARAM_SECTIONS(X) }      // fn(host pointer, byte offset, bytes) per section
#undef X
};
struct ForestView {       // the forest's sections of the block at `block`, typed
#define X(field, T, count) const T* field;
  SH_PARAM_FOREST_SECTIONS(X)
#undef X
#define X(field, T, count) field = (const T*)((const char*)block + L.field);
  ForestView(const void* block, const ParamLayout& L) { SH_PARAM_FOREST_SECTIONS(X) }
#undef X
};

struct ParamError { int code; const char* text; };      // code SH_OK: accepted

// ---- the forest check -----------------------------------------------------------------------------------------------------------------
#define SH_RFC_FEATURES 9      // columns of a peak's feature row (k_groove.h, groove.xraw): what a node's feature id indexes
// The walk on the device (k_groove_rfc) indexes a feature row by a node's feature id and follows child indices until it meets a leaf
// (both children negative): every id and index must be in range and every node reached once at most (no cycle, no shared subtree).
// All nodes first, then all roots, then reachability; `text` is a fragment the caller completes.
inline ParamError forest_check(const int32_t* feat, const int32_t* ti, const int32_t* fi, int n_nodes, const int32_t* roots, int n_trees) {
  for (int i = 0; i < n_nodes; ++i) {
    if (feat[i] < 0 || feat[i] >= SH_RFC_FEATURES) return {SH_ERR_ARG, "feature id out of range"};
    if ((ti[i] < 0) != (fi[i] < 0) || ti[i] >= n_nodes || fi[i] >= n_nodes) return {SH_ERR_ARG, "bad child index"};
  }
  for (int t = 0; t < n_trees; ++t)
    if (roots[t] < 0 || roots[t] >= n_nodes) return {SH_ERR_ARG, "bad root"};
  std::vector<char> seen(n_nodes > 0 ? n_nodes : 0, 0);
  std::vector<int> stack;
  for (int t = 0; t < n_trees; ++t) {
    stack.push_back(roots[t]);
    while (!stack.empty()) {
      const int i = stack.back(); stack.pop_back();
      if (seen[i]) return {SH_ERR_ARG, "the node tables do not describe a forest (a node is reachable twice)"};
      seen[i] = 1;
      if (ti[i] >= 0) { stack.push_back(ti[i]); stack.push_back(fi[i]); }
    }
  }
  return {SH_OK, ""};
}

// ---- the run parameters: sh_default_params, and what sh_set_params refuses (values the kernels and the reference cannot index with) ------
inline sh_params default_run_params() { return sh_params{{0.35, 0.75}, {0.2, 0.75}, 7.0, SH_UNET_F32, SH_BONE_HUMERUS}; }
inline ParamError run_params_check(const sh_params& p) {
  for (double x : {p.groove_cutoff[0], p.groove_cutoff[1], p.canal_cutoff[0], p.canal_cutoff[1]})
    if (!(x >= 0.0 && x <= 1.0)) return {SH_ERR_ARG, "cut-off fractions must lie in [0, 1]"};
  int a, b;
  cutoff_range(SH_NPROX, p.groove_cutoff[0], p.groove_cutoff[1], &a, &b);
  if (b - a != SH_GROOVE_NROWS) return {SH_ERR_ARG, "groove_cutoff must select 330 proximal rows"};
  cutoff_range(SH_NFULL, p.canal_cutoff[0], p.canal_cutoff[1], &a, &b);
  if (b - a < 2 || a < 0 || b > SH_NFULL) return {SH_ERR_ARG, "canal_cutoff selects fewer than 2 slices"};
  // the search window of the groove's local minimum is +-round(deg_window / (360 / 512)) samples of a 512-sample row
  // (bicipital_groove.py:190-229); beyond half a turn the reference's negative indices run off the row (IndexError there)
  if (!(p.groove_deg_window >= 0.0 && p.groove_deg_window <= 180.0)) return {SH_ERR_ARG, "groove_deg_window must lie in [0, 180] degrees"};
  if (p.unet_dtype != SH_UNET_F32 && p.unet_dtype != SH_UNET_BF16 && p.unet_dtype != SH_UNET_F16 && p.unet_dtype != SH_UNET_F32X)
    return {SH_ERR_ARG, "unet_dtype must be SH_UNET_F32, SH_UNET_F32X, SH_UNET_BF16 or SH_UNET_F16"};
  if (p.bone_kind != SH_BONE_HUMERUS && p.bone_kind != SH_BONE_PROXIMAL) return {SH_ERR_ARG, "bone_kind must be SH_BONE_HUMERUS or SH_BONE_PROXIMAL"};
  return {SH_OK, ""};
}

// ---- what is loaded, and which packed copies of the block are current ------------------------------------------------------------------
// One member of sh_ctx.  Not every kernel reads the block as it lies: the 16-bit and split-f16 UNet paths read packed weights
// ("params_bf16", "params_x3h/l", by the layer table "unet16.packtab"), the groove stage packed nodes ("rfc.nodes").  Each copy is made
// once and is stale as soon as the block can have changed.
class ParamState {
 public:
  // events, one per place that learns something.  A load fires its event in front of its upload
  void unet_loaded(int base, int depth, size_t n_floats) { shape_.base = base; shape_.depth = depth; shape_.unet_floats = n_floats; unet_ = true; packtab_ = false; }
  void rfc_loaded(size_t nodes, size_t trees) { shape_.nodes = nodes; shape_.trees = trees; rfc_ = true; forest_ = false; }
  // the block can change: every upload, sh_param_block / sh_buffer_device("params") handing the pointer out (the caller may write
  // it), sh_store("params"), sh_param_block_commit
  void block_exposed() { kind16_ = -1; x3_ = false; forest_ = false; }
  void block_lost() { *this = ParamState(); }      // an upload failed and the block is gone: neither half counts as loaded
  void packed16(int kind) { kind16_ = kind; }      // unet.hip pack_weights: "params_bf16" holds the block's weights as `kind` (0 bf16, 1 f16)
  void packed_x3() { x3_ = true; }                 // ... "params_x3h/l" its split weights
  void packtab_uploaded() { packtab_ = true; }     // ... "unet16.packtab" the layer table of the loaded network
  void forest_packed() { forest_ = true; }         // stage_groove: "rfc.nodes" holds the block's forest
  // queries
  bool has_unet() const { return unet_; }
  bool has_rfc() const { return rfc_; }
  const ParamShape& shape() const { return shape_; }
  bool same_shape(const ParamState& o) const { return shape_ == o.shape_; }      // sh_bcast_weights: one block fits the other
  bool need_pack16(int kind) const { return kind16_ != kind; }
  bool need_pack_x3() const { return !x3_; }
  bool need_packtab() const { return !packtab_; }
  bool need_forest_pack() const { return !forest_; }

 private:
  ParamShape shape_;
  bool unet_ = false, rfc_ = false, packtab_ = false, x3_ = false, forest_ = false;
  int kind16_ = -1;      // the kind "params_bf16" holds; -1: stale
};

}  // namespace sh
