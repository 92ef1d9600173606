// sh_query.h -- what the queries of the resident batch decide on the host: the rays (sh_ray_cast / sh_anp_axis_hits), the closest surface
// points (sh_closest_points), the generalized winding numbers (sh_winding_numbers), the registration of point sets (sh_register_points,
// sh_register_multistart), the mass properties (sh_mass_properties), the surface samples (sh_sample_surface), the mesh topology (sh_mesh_topology), the vertex fields (sh_vertex_fields), the geodesics (sh_geodesic), the smoothing of the vertices (sh_smooth_vertices), the repair (sh_mesh_repair), the simplification (sh_mesh_simplify) and the face hierarchy (sh_mesh_bvh, sh_set_query_accel).  A query reads the mesh and changes no state of the
// arthroplasty chain; it is no link of it.  Per query: the buffer list, the plan with the bytes of every buffer, and one ordered
// precheck.  No kernels, no HIP types: sh_ctx.h includes it, and so does a plain g++ (tests/hostcheck/{ray,closest,winding,icp,mass,sample,topo,vert,geo,bvh,smooth,repair,simplify}_check.cpp).
// The entry points are sh_query_host.h.  From sh_arthro.h: SH_BUF_LIST, ArthroError and the refusal texts, ArthroFacts (the anatomic-neck
// rays ask the chain's state for the last run), `resident`, tiles_of.
#pragma once
#include "sh_arthro.h"
#include "sh_scalar.h"      // the level rule of the face hierarchy (bvh_levels_of, bvh_nodes_of)

#include <vector>

namespace sh {

// ---- the named buffers of the queries, one statement each: X(field, "name", element type, elem), and one line for their structs ----
struct RayKey; struct CpPart; struct GeoInfo;
#define RAY_BUFS(X)                                                                                                                \
  X(ray_rays, "ray.rays", double, 8) X(ray_status, "ray.status", int, 4) X(ray_counts, "ray.counts", int, 4)                       \
  X(ray_offs, "ray.offs", unsigned long long, 8) X(ray_cursor, "ray.cursor", int, 4) X(ray_pool, "ray.pool", RayKey, 8)            \
  X(ray_hits, "ray.hits", sh_ray_hit, 8) X(ray_blockhit, "ray.blockhit", int, 4)
#define CP_BUFS(X) X(cp_points, "cp.points", double, 8) X(cp_part, "cp.part", CpPart, 8) X(cp_out, "cp.out", sh_closest, 8)
#define WN_BUFS(X) X(wn_points, "wn.points", double, 8) X(wn_part, "wn.part", double, 8) X(wn_out, "wn.out", sh_winding, 8)
// the walk of a registration runs on buffers of its own ("icp.cp_part", "icp.near")
#define ICP_BUFS(X)                                                                                                                \
  X(icp_points, "icp.points", double, 8) X(icp_moved, "icp.moved", double, 8) X(icp_cp_part, "icp.cp_part", CpPart, 8)             \
  X(icp_near, "icp.near", sh_closest, 8) X(icp_part, "icp.part", double, 8) X(icp_T, "icp.T", double, 8)                           \
  X(icp_hist, "icp.hist", double, 8) X(icp_flags, "icp.flags", int, 4) X(icp_out, "icp.out", sh_registration, 8)
// the block rows and the records
#define MASS_BUFS(X) X(mass_part, "mass.part", double, 8) X(mass_out, "mass.out", sh_mass, 8)
// the multi-start registration runs the chain of sh_register_points on the "icp.*" buffers; these are its own
#define MS_BUFS(X)                                                                                                                 \
  X(ms_T0s, "ms.T0s", double, 8) X(ms_points, "ms.points", double, 8) X(ms_coarse, "ms.coarse", sh_registration, 8)                \
  X(ms_best, "ms.best", double, 8) X(ms_winner, "ms.winner", int, 4)
// the cumulative areas and the block bases, the records, and the states of the thinning (per humerus AR_SAMP_HEAD counters, then 2 x N)
#define SAMP_BUFS(X)                                                                                                               \
  X(samp_cdf, "samp.cdf", double, 8) X(samp_base, "samp.base", double, 8) X(samp_out, "samp.out", sh_sample, 8)                    \
  X(samp_info, "samp.info", sh_sample_info, 8) X(samp_state, "samp.state", int, 4)
// the incidence (row starts, rows), the adjacency, the labels and the records; scratch: the heads (AR_TOPO_HEAD int32 per mesh), the rows'
// cursors, the unordered rows / shell indices / shell sizes, and the two arrays of the rounds
#define TOPO_BUFS(X)                                                                                                               \
  X(topo_vrow, "topo.vrow", int, 4) X(topo_vface, "topo.vface", int, 4) X(topo_adj, "topo.adj", int, 4) X(topo_label, "topo.label", int, 4) \
  X(topo_info, "topo.info", sh_topology, 4) X(topo_shells, "topo.shells", sh_shell, 4) X(topo_state, "topo.state", int, 4)         \
  X(topo_cursor, "topo.cursor", int, 4) X(topo_tmp, "topo.tmp", int, 4) X(topo_p, "topo.p", int, 4)
// the face records, the unit normals, the fields, the flags and the status per mesh; scratch: A2 per face, the four planes of the
// smoothing (two arrays of gauss and mean), one int32 per mesh (a face that is not flat)
#define VERT_BUFS(X)                                                                                                               \
  X(vert_face, "vert.face", double, 8) X(vert_normal, "vert.normal", double, 8) X(vert_fields, "vert.fields", double, 8)           \
  X(vert_flags, "vert.flags", int, 4) X(vert_status, "vert.status", int, 4) X(vert_a2, "vert.a2", double, 8)                       \
  X(vert_plane, "vert.plane", double, 8) X(vert_state, "vert.state", int, 4)
// the face records, the K planes of distances, predecessors and sources per mesh, the info records; scratch: the vertex across each slot,
// the second plane of the general path, the pointer jumping, the lists of the call (offsets and vertices; d0) and SH_GEO_STATE int32 per
// (mesh, set) pair and once more for the call
#define GEO_BUFS(X)                                                                                                                \
  X(geo_face, "geo.face", double, 8) X(geo_dist, "geo.dist", double, 8) X(geo_pred, "geo.pred", int, 4) X(geo_source, "geo.source", int, 4) \
  X(geo_info, "geo.info", GeoInfo, 8) X(geo_opp, "geo.opp", int, 4) X(geo_plane, "geo.plane", double, 8) X(geo_jump, "geo.jump", int, 4)    \
  X(geo_src, "geo.src", int, 4) X(geo_d0, "geo.d0", double, 8) X(geo_state, "geo.state", int, 4)
// the order, the loose list, the offsets, the boxes, the sorted corners and the records; scratch: SH_BVH_HEAD words per mesh (the box as
// topo_enc words, the tight faces), each mesh's first node and first key (B + 1 each), the keys before and behind the sort
#define BVH_BUFS(X)                                                                                                                \
  X(bvh_order, "bvh.order", int, 4) X(bvh_loose, "bvh.loose", int, 4) X(bvh_off, "bvh.off", int, 4) X(bvh_box, "bvh.box", float, 4)  \
  X(bvh_tri, "bvh.tri", float, 4) X(bvh_info, "bvh.info", sh_bvh_info, 4) X(bvh_state, "bvh.state", unsigned, 4)                   \
  X(bvh_base, "bvh.base", int, 4) X(bvh_seg, "bvh.seg", unsigned, 4) X(bvh_key, "bvh.key", unsigned long long, 8)                  \
  X(bvh_sorted, "bvh.sorted", unsigned long long, 8)
// the vertex -> vertex rows (row starts, neighbours, the stored weights beside them), the result and the info records; scratch: three planes
// of 3 sumV doubles (two for the iteration, one for b of the HC filter), the pins, the host's mask, the block rows and heads of the sums
#define SMOOTH_BUFS(X)                                                                                                             \
  X(smooth_nbr, "smooth.nbr", int, 4) X(smooth_w, "smooth.w", double, 8) X(smooth_pos, "smooth.pos", double, 8)                    \
  X(smooth_info, "smooth.info", SmoothInfo, 8) X(smooth_plane, "smooth.plane", double, 8) X(smooth_pin, "smooth.pin", int, 4)      \
  X(smooth_mask, "smooth.mask", unsigned char, 1) X(smooth_part, "smooth.part", double, 8) X(smooth_nrow, "smooth.nrow", int, 4)
// the final flips, the repaired meshes (regions sized from "topo.info"), the records and the regions' starts; scratch: the outward
// orientation, the int32 work of the walk and the lists (first, bad, two queues, lists: 5 sumF, and AR_REPAIR_HEAD per mesh), the
// AR_REPAIR_EDGE_ARRAYS arrays of the border half-edges, the terms and block sums of V6
#define REPAIR_BUFS(X)                                                                                                             \
  X(repair_flip, "repair.flip", unsigned char, 1) X(repair_faces, "repair.faces", int, 4) X(repair_verts, "repair.verts", float, 4) \
  X(repair_info, "repair.info", sh_repair_info, 4) X(repair_shells, "repair.shells", sh_repair_shell, 8)                           \
  X(repair_holes, "repair.holes", sh_repair_hole, 4) X(repair_off, "repair.off", long long, 8) X(repair_par, "repair.par", unsigned char, 1) \
  X(repair_work, "repair.work", int, 4) X(repair_edge, "repair.edge", int, 4) X(repair_term, "repair.term", double, 8)
// the simplified meshes (mesh b at voff[b] / foff[b]), the map and the records; scratch: AR_SIMP_HEAD words per mesh (the box as topo_enc
// words, the counts, the largest move), the segments of the sorts (B + 1), the cells, the keys before and behind a sort, the key and the
// first sorted place of every cluster, the cluster of every vertex, the marks (heads, then named clusters) and their scan, the vertex
// quadrics, the cluster positions, the kept faces and their scan.  ("simp.tmp", the sorts' storage, is sized by rocPRIM beside the list.)
#define SIMPLIFY_BUFS(X)                                                                                                           \
  X(simp_verts, "simp.verts", float, 4) X(simp_faces, "simp.faces", int, 4) X(simp_map, "simp.map", int, 4)                        \
  X(simp_info, "simp.info", sh_simplify_info, 8) X(simp_state, "simp.state", unsigned, 4) X(simp_seg, "simp.seg", unsigned, 4)     \
  X(simp_cell, "simp.cell", double, 8) X(simp_key, "simp.key", unsigned long long, 8) X(simp_sorted, "simp.sorted", unsigned long long, 8) \
  X(simp_ukey, "simp.ukey", unsigned long long, 8) X(simp_start, "simp.start", int, 4) X(simp_cid, "simp.cid", int, 4)             \
  X(simp_mark, "simp.mark", int, 4) X(simp_rank, "simp.rank", int, 4) X(simp_quad, "simp.quad", double, 8)                         \
  X(simp_pos, "simp.pos", float, 4) X(simp_keep, "simp.keep", int, 4) X(simp_frank, "simp.frank", int, 4)
// (RayBytes, RayBufs and RayView, the mesh's pointers and the list's: what a query hands to its kernels)
#define SH_QUERY_LIST(Name, LIST) SH_BUF_LIST(Name, LIST) using Name##View = BufJoin<MeshBufs, Name##Bufs>;
SH_QUERY_LIST(Ray, RAY_BUFS)
SH_QUERY_LIST(Cp, CP_BUFS)
SH_QUERY_LIST(Wn, WN_BUFS)
SH_QUERY_LIST(Icp, ICP_BUFS)
SH_QUERY_LIST(Mass, MASS_BUFS)
SH_BUF_LIST(Ms, MS_BUFS)      // (beside an IcpView: no mesh of its own)
SH_QUERY_LIST(Samp, SAMP_BUFS)
SH_QUERY_LIST(Topo, TOPO_BUFS)
SH_BUF_LIST(Vert, VERT_BUFS)
using VertView = BufJoin<MeshBufs, TopoBufs, VertBufs>;      // (the mesh, the incidence and adjacency it reads, and its own)
SH_BUF_LIST(Geo, GEO_BUFS)
using GeoView = BufJoin<MeshBufs, TopoBufs, GeoBufs>;
SH_QUERY_LIST(Bvh, BVH_BUFS)
SH_BUF_LIST(Smooth, SMOOTH_BUFS)
using SmoothView = BufJoin<MeshBufs, TopoBufs, SmoothBufs>;
SH_BUF_LIST(Repair, REPAIR_BUFS)
using RepairView = BufJoin<MeshBufs, TopoBufs, RepairBufs>;
SH_BUF_LIST(Simplify, SIMPLIFY_BUFS)
using SimplifyView = BufJoin<MeshBufs, TopoBufs, SimplifyBufs>;

// what the kernel headers fix, restated (shoulder_hip.hip holds each against its header with a static_assert)
constexpr int AR_RAY_TILE = 256, AR_RAY_CHUNK = 256, AR_RAY_KEY_BYTES = 16;       // SH_RAY_TILE, SH_RAY_CHUNK, sizeof(RayKey)
constexpr int AR_CP_TILE = 256, AR_CP_CHUNK = 256, AR_CP_PART_BYTES = 16;         // SH_CP_TILE, SH_CP_CHUNK, sizeof(CpPart)
constexpr int AR_CP_FILL = 1024;      // workgroups of k_cp_walk that fill the chip: four of 256 lanes on each of 256 compute units
constexpr int AR_WN_TILE = 256, AR_WN_CHUNK = 256, AR_WN_BLOCK = 2048;            // SH_WN_TILE, SH_WN_CHUNK, SH_WIND_BLOCK
constexpr int AR_WN_FILL = 1024;      // workgroups of k_wn_walk that fill the chip, as AR_CP_FILL
constexpr int AR_ICP_TERMS = 32, AR_ICP_TSTRIDE = 20;                             // SH_ICP_TERMS, SH_ICP_TSTRIDE
constexpr int AR_MASS_TERMS = 24;                                                 // SH_MASS_TERMS
constexpr int AR_SAMP_CHUNK = 256, AR_SAMP_HEAD = 64;                             // SH_SAMP_CHUNK, SH_SAMP_HEAD
constexpr int AR_TOPO_BLOCK = 256, AR_TOPO_HEAD = 64;                             // SH_TOPO_BLOCK, SH_TOPO_HEAD
constexpr int AR_VERT_BLOCK = 256, AR_VERT_FACE = 10;                             // SH_VERT_BLOCK, SH_VTX_FACE
constexpr int AR_GEO_BLOCK = 256, AR_GEO_FACE = 6, AR_GEO_STATE = 8;              // SH_GEO_BLOCK, SH_GEOD_FACE, SH_GEO_STATE
constexpr int AR_BVH_BLOCK = 256, AR_BVH_HEAD = 8, AR_BVH_CHUNK = 64;             // SH_BVH_BLOCK, SH_BVH_HEAD, SH_BVH_CHUNK
constexpr int AR_SMOOTH_BLOCK = 256;                                              // SH_SMOOTH_BLOCK
constexpr int AR_REPAIR_BLOCK = 256, AR_REPAIR_HEAD = 16, AR_REPAIR_EDGE_ARRAYS = 18;      // SH_REPAIR_BLOCK, SH_REPAIR_HEAD, SH_REPAIR_EDGE_ARRAYS
constexpr int AR_SIMP_BLOCK = 256, AR_SIMP_HEAD = 20, AR_SIMP_Q = 10;                      // SH_SIMP_BLOCK, SH_SIMP_HEAD, SH_SIMP_Q

// ---- the checks, each once --------------------------------------------------------------------------------------------------------
// n rays: the index of the first one that is not six finite doubles with a non-zero direction, or -1
inline long long first_bad_ray(const sh_ray* rays, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const sh_ray& r = rays[i];
    bool fin = true;
    for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(r.origin[k]) && std::isfinite(r.dir[k]);
    if (!fin || (r.dir[0] == 0.0 && r.dir[1] == 0.0 && r.dir[2] == 0.0)) return (long long)i;
  }
  return -1;
}

// n points: the index of the first one with a coordinate that is not finite, or -1 (one scan loop for all callers, not inlined into each)
__attribute__((noinline)) inline long long first_bad_point(const double* pts, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(pts[3 * i]) || !std::isfinite(pts[3 * i + 1]) || !std::isfinite(pts[3 * i + 2])) return (long long)i;
  return -1;
}

// a rigid CT -> CT start of a registration: finite, last row exactly 0 0 0 1, |R^T R - I| <= 1e-9 in every entry (the columns: a shear
// of 1e-6 fails), determinant positive (a reflection fails)
inline bool rigid_start_ok(const double* T) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(T[i])) return false;
  if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const double d = (T[i] * T[j] + T[4 + i] * T[4 + j]) + T[8 + i] * T[8 + j];
      if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-9)) return false;
    }
  return det3_of4(T) > 0.0;
}
inline bool icp_options_ok(const sh_icp_options* o) {
  return (o->metric == SH_ICP_POINT || o->metric == SH_ICP_PLANE) && o->max_iter >= 1 && o->max_iter <= SH_ICP_MAX_ITER && o->reject > 0.0 &&
         o->tol >= 0.0 && std::isfinite(o->tol);
}

// A set of Q query points, shared or per humerus, in the order every call that takes one refuses it: Q in 1..Qmax; `args`, the call's
// verdict on its other arguments, which ranks here; the state (`resident`); the first point that is not finite.  (Always inlined: a
// precheck stays the one function it was, in the library's symbol table too.)
__attribute__((always_inline)) inline ArthroError point_set(const double* points, int Q, int Qmax, int per_humerus, const ArthroFacts& f, const ArthroError& args = arthro_ok()) {
  if (!f.ctx || !points || Q < 1 || Q > Qmax) return {SH_ERR_ARG, "bad argument (Q in 1.." + std::to_string(Qmax) + ")"};
  if (args.code) return args;
  if (const ArthroError e = resident(f); e.code) return e;
  const long long i = first_bad_point(points, per_humerus ? (size_t)f.B * Q : (size_t)Q);
  if (i >= 0) return {SH_ERR_ARG, "point " + std::to_string(i) + " has a coordinate that is not finite"};
  return arthro_ok();
}

// ---- the plans and the bytes of every buffer ----------------------------------------------------------------------------------------
// a cast of R rays per humerus with room for cap hits each: everything but the pool, which the counts size ("ray.pool", ray_pool_bytes)
// tree: the walk descends the face hierarchy (k_raytree.h) -- chunks of AR_BVH_CHUNK rays, one per lane, and no "ray.blockhit".
// near: the call is sh_ray_nearest -- the bytes of "ray.near" (B x R sh_ray_hit; a buffer of its own beside the list, which stays the
// chain's) and the chain's buffers at cap = 1, or with `tree` "ray.rays" and "ray.near" alone.
struct RayPlan { int tmax, chunks; size_t rays; RayBytes bytes; size_t near; };      // face tiles per humerus, ray chunks, B x R, ..., bytes of "ray.near"
inline RayPlan ray_plan(int B, int R, bool per_humerus, int cap, long long maxF, bool with_status, bool tree = false, bool near = false) {
  const size_t n = (size_t)B * R, near_bytes = near ? n * sizeof(sh_ray_hit) : 0;
  RayBytes z;
  z.ray_rays = (per_humerus ? n : (size_t)R) * sizeof(sh_ray);
  const long long tmax = tiles_of(maxF, AR_RAY_TILE);
  if (tree && near) return {(int)tmax, (R + AR_BVH_CHUNK - 1) / AR_BVH_CHUNK, n, z, near_bytes};
  z.ray_counts = n * 4; z.ray_offs = (n + 1) * 8; z.ray_cursor = n * 4;
  z.ray_hits = n * cap * sizeof(sh_ray_hit);
  if (with_status) z.ray_status = (size_t)B * 4;
  const int chunks = tree ? (R + AR_BVH_CHUNK - 1) / AR_BVH_CHUNK : (R + AR_RAY_CHUNK - 1) / AR_RAY_CHUNK;
  if (!tree) z.ray_blockhit = (size_t)tmax * B * chunks * 4;      // one word per workgroup of the walk
  return {(int)tmax, chunks, n, z, near_bytes};
}
inline size_t ray_pool_bytes(unsigned long long total) { return (size_t)(total > 0 ? total : 1) * AR_RAY_KEY_BYTES; }

// The splits of a walk over the units (face tiles, face blocks) of the largest humerus.  S is the host's choice and no knob: as many
// splits as bring a grid of `groups` (B x point chunks) workgroups to `fill` when it is small, never more than the units, at least one.
inline int fill_splits(long long groups, long long units, int fill) {
  const long long g = groups > 1 ? groups : 1, want = (fill + g - 1) / g;
  const long long s = want < units ? want : units;
  return (int)(s > 1 ? s : 1);
}

// Closest points, Q per humerus.  The grid of k_cp_walk is (chunks of 256 points, B, S face splits): split s of a humerus with T tiles
// walks the tiles cp_split_range(T, S, s) (sh_scalar.h).  A minimum under a total order does not depend on how its candidates are
// grouped, so S changes no result.
inline int cp_splits(long long groups /* B x chunks */, long long tiles /* of the largest humerus */) { return fill_splits(groups, tiles, AR_CP_FILL); }
struct CpPlan { int tmax, chunks, S; size_t points; CpBytes bytes; };      // face tiles of the largest humerus, point chunks, face splits, B x Q
inline CpPlan cp_plan(int B, int Q, bool per_humerus, long long maxF) {
  const size_t n = (size_t)B * Q;
  const long long tmax = tiles_of(maxF, AR_CP_TILE);
  const int chunks = (Q + AR_CP_CHUNK - 1) / AR_CP_CHUNK;
  const int S = cp_splits((long long)B * chunks, tmax);
  CpBytes z;
  z.cp_points = (per_humerus ? n : (size_t)Q) * 24; z.cp_part = n * S * AR_CP_PART_BYTES; z.cp_out = n * sizeof(sh_closest);
  return {(int)tmax, chunks, S, n, z};
}

// Winding numbers, Q per humerus.  The grid of k_wn_walk is (chunks of 256 points, B, S splits): split s of a humerus with K blocks of
// AR_WN_BLOCK faces walks the blocks cp_split_range(K, S, s) (sh_scalar.h) -- whole blocks, a split never cuts one, because the block
// sums are the fixed inner level of the summation tree.  With S == 1 a workgroup owns all blocks of its humerus and adds the block sums
// itself, in block order ("wn.part" holds one total per point); with S > 1 "wn.part" holds the block sums (kmax per point) and
// k_wn_join adds them in the same order.  S changes no byte.
inline int wn_splits(long long groups /* B x chunks */, long long blocks /* of the largest humerus */) { return fill_splits(groups, blocks, AR_WN_FILL); }
struct WnPlan { int kmax, chunks, S, stride; size_t points; WnBytes bytes; };      // blocks of the largest humerus, point chunks, splits, doubles of "wn.part" per point, B x Q
inline WnPlan wn_plan(int B, int Q, bool per_humerus, long long maxF) {
  const size_t n = (size_t)B * Q;
  const long long kmax = tiles_of(maxF, AR_WN_BLOCK);
  const int chunks = (Q + AR_WN_CHUNK - 1) / AR_WN_CHUNK;
  const int S = wn_splits((long long)B * chunks, kmax);
  const int stride = S == 1 ? 1 : (int)kmax;
  WnBytes z;
  z.wn_points = (per_humerus ? n : (size_t)Q) * 24; z.wn_part = n * stride * sizeof(double); z.wn_out = n * sizeof(sh_winding);
  return {(int)kmax, chunks, S, stride, n, z};
}

// Registration, Q points per humerus.  The walk of an evaluation is the closest-point walk on the moved points, always per humerus:
// its chunks and its split S are cp_plan's, unchanged.  The sums take the points in blocks of SH_ICP_BLOCK = the walk's chunk, one
// row of AR_ICP_TERMS doubles per (humerus, block) in "icp.part"; "icp.T" holds the transform and the mean of the input points.
struct IcpPlan { int chunks, S; size_t points; IcpBytes bytes; };      // point chunks = blocks of the sums, face splits of the walk, B x Q
inline IcpPlan icp_plan(int B, int Q, bool per_humerus, long long maxF, int max_iter) {
  const CpPlan cp = cp_plan(B, Q, true, maxF);
  IcpBytes z;
  z.icp_points = (per_humerus ? cp.points : (size_t)Q) * 24; z.icp_moved = cp.points * 24; z.icp_cp_part = cp.bytes.cp_part; z.icp_near = cp.bytes.cp_out;
  z.icp_part = (size_t)B * cp.chunks * AR_ICP_TERMS * 8; z.icp_T = (size_t)B * AR_ICP_TSTRIDE * 8; z.icp_hist = (size_t)B * (max_iter + 1) * 16;
  z.icp_flags = (size_t)B * 4; z.icp_out = (size_t)B * sizeof(sh_registration);
  return {cp.chunks, cp.S, cp.points, z};
}

// Mass properties: one row of AR_MASS_TERMS doubles per (humerus, block of SH_MASS_BLOCK faces) in "mass.part", the blocks of the largest
// humerus for every humerus
struct MassPlan { int blocks; MassBytes bytes; };
inline MassPlan mass_plan(int B, long long maxF) {
  const long long blocks = tiles_of(maxF, SH_MASS_BLOCK);
  MassBytes z;
  z.mass_part = (size_t)B * blocks * AR_MASS_TERMS * 8; z.mass_out = (size_t)B * sizeof(sh_mass);
  return {(int)blocks, z};
}

// Surface samples, N per humerus.  "samp.cdf" follows the faces (humerus b at foff[b]); "samp.base" has one double per block of
// SH_SAMPLE_BLOCK faces of the largest humerus for every humerus; "samp.state" per humerus AR_SAMP_HEAD int32 (word r: the undecided at
// the start of round r) and, with a radius, the two state arrays of N int32 that the rounds alternate between.
struct SampPlan { int blocks, chunks, thin, stride; SampBytes bytes; };      // face blocks of the largest humerus, sample chunks, radius > 0, int32 of "samp.state" per humerus
inline SampPlan samp_plan(int B, int N, bool thin, long long maxF, long long sumF) {
  static_assert(AR_SAMP_HEAD > SH_THIN_MAX_ROUNDS, "samp.state: a counter per round and one behind the last");
  const long long blocks = tiles_of(maxF, SH_SAMPLE_BLOCK);
  const int chunks = (N + AR_SAMP_CHUNK - 1) / AR_SAMP_CHUNK;
  const int stride = AR_SAMP_HEAD + (thin ? 2 * N : 0);
  SampBytes z;
  z.samp_cdf = (size_t)(sumF > 0 ? sumF : 1) * 8; z.samp_base = (size_t)B * blocks * 8; z.samp_out = (size_t)B * N * sizeof(sh_sample);
  z.samp_info = (size_t)B * sizeof(sh_sample_info); z.samp_state = (size_t)B * stride * 4;
  return {(int)blocks, chunks, thin ? 1 : 0, stride, z};
}

// Mesh topology.  "topo.vrow" and "topo.cursor" have V_b + 1 int32 per mesh (mesh b at voff[b] + b); "topo.vface", "topo.adj" and
// "topo.tmp" three per face (mesh b at 3 foff[b]), "topo.label" one, "topo.p" two (the arrays of the rounds, mesh b at 2 foff[b]);
// "topo.state" AR_TOPO_HEAD int32 per mesh: word r says whether round r - 1 changed something, the counts behind the rounds.
struct TopoPlan { int blocks; TopoBytes bytes; };      // face blocks of the largest mesh
inline TopoPlan topo_plan(int B, int max_shells, long long maxF, long long sumV, long long sumF) {
  static_assert(AR_TOPO_HEAD > SH_TOPO_MAX_ROUNDS + 1, "topo.state: a word per round and one behind the last");
  const size_t f = (size_t)(sumF > 0 ? sumF : 1), rows = ((size_t)sumV + B) * 4;
  TopoBytes z;
  z.topo_vrow = rows; z.topo_vface = 3 * f * 4; z.topo_adj = 3 * f * 4; z.topo_label = f * 4;
  z.topo_info = (size_t)B * sizeof(sh_topology); z.topo_shells = (size_t)B * max_shells * sizeof(sh_shell);
  z.topo_state = (size_t)B * AR_TOPO_HEAD * 4; z.topo_cursor = rows; z.topo_tmp = 3 * f * 4; z.topo_p = 2 * f * 4;
  return {(int)tiles_of(maxF, AR_TOPO_BLOCK), z};
}

// Vertex fields.  "vert.face" has AR_VERT_FACE doubles per face (mesh b at 10 foff[b]) and "vert.a2" one; "vert.normal" three doubles per
// vertex (mesh b at 3 voff[b]), "vert.fields" SH_VERT_FIELDS, "vert.flags" one int32; "vert.plane" four planes of sumV doubles: the two
// arrays of the smoothing, gauss and mean each; "vert.status" and "vert.state" one int32 per mesh.
struct VertPlan { int fblocks, vblocks; VertBytes bytes; };      // face and vertex blocks of the largest mesh
inline VertPlan vert_plan(int B, long long maxV, long long maxF, long long sumV, long long sumF) {
  const size_t f = (size_t)(sumF > 0 ? sumF : 1), v = (size_t)(sumV > 0 ? sumV : 1);
  VertBytes z;
  z.vert_face = f * AR_VERT_FACE * 8; z.vert_normal = v * 24; z.vert_fields = v * SH_VERT_FIELDS * 8; z.vert_flags = v * 4;
  z.vert_status = (size_t)B * 4; z.vert_a2 = f * 8; z.vert_plane = 4 * v * 8; z.vert_state = (size_t)B * 4;
  return {(int)tiles_of(maxF, AR_VERT_BLOCK), (int)tiles_of(maxV, AR_VERT_BLOCK), z};
}

// Geodesics.  "geo.face" has AR_GEO_FACE doubles per face and "geo.opp" three int32; "geo.dist", "geo.plane" (only with a mesh of the
// general path), "geo.pred", "geo.source" and "geo.jump" K words per vertex (mesh b at K voff[b]); "geo.info" 32 bytes per pair; "geo.src"
// the B K + 1 offsets and behind them the S vertices of the call, "geo.d0" its S offsets; "geo.state" AR_GEO_STATE int32 per pair and
// once more for the call.  general: the largest mesh has more than lds_vertices vertices; rounds_max = that mesh's vertices + 1.
struct GeoPlan { int fblocks, vblocks, jumps; bool general; long long rounds_max; GeoBytes bytes; };
inline GeoPlan geo_plan(int B, int K, long long S, int lds_vertices, long long maxV, long long maxF, long long sumV, long long sumF) {
  const size_t f = (size_t)(sumF > 0 ? sumF : 1), v = (size_t)(sumV > 0 ? sumV : 1) * (size_t)K, pairs = (size_t)B * (size_t)K;
  const bool general = maxV > lds_vertices;
  GeoBytes z;
  z.geo_face = f * AR_GEO_FACE * 8; z.geo_dist = v * 8; z.geo_pred = v * 4; z.geo_source = v * 4; z.geo_info = pairs * SH_GEO_INFO_BYTES; z.geo_opp = f * 12;
  z.geo_plane = general ? v * 8 : 0; z.geo_jump = v * 4; z.geo_src = (pairs + 1 + (size_t)S) * 4; z.geo_d0 = (size_t)(S > 0 ? S : 1) * 8;
  z.geo_state = (pairs + 1) * AR_GEO_STATE * 4;
  int jumps = 0;
  while ((1ll << jumps) < maxV) ++jumps;      // a round of the pointer jumping at least halves what is left of a chain of at most maxV - 1 hops
  return {(int)tiles_of(maxF, AR_GEO_BLOCK), (int)tiles_of(maxV, AR_GEO_BLOCK), jumps, general, general ? maxV + 1 : 0, z};
}

// Smoothing of the vertices.  "smooth.nrow" has V_b + 1 int32 per mesh (mesh b at voff[b] + b); "smooth.nbr" and "smooth.w" room for two
// neighbours per corner of a face (mesh b at 6 foff[b]; a mesh uses the first nrow[V_b] of its 6 F_b places); "smooth.pos" three doubles
// per vertex and "smooth.plane" three such planes; "smooth.pin" one int32 and "smooth.mask" one byte per vertex; "smooth.part" the block
// rows of the two volume sums (SH_SMO_TERMS doubles per face block of the largest mesh, for every mesh: at vol0 and vol1), the rows of
// the displacement (two doubles per vertex block: at disp) and the heads (SH_SMO_HEAD doubles per mesh: at head).  Every size follows
// from the batch alone, so a second call allocates nothing.  steps: the launches of k_smooth_round; last: the plane they leave P in.
struct SmoothPlan { int fblocks, vblocks, steps, last; size_t plane, vol0, vol1, disp, head; SmoothBytes bytes; };      // (plane .. head: in doubles)
inline SmoothPlan smooth_plan(int B, int filter, int iterations, long long maxV, long long maxF, long long sumV, long long sumF) {
  const size_t f = (size_t)(sumF > 0 ? sumF : 1), v = (size_t)(sumV > 0 ? sumV : 1);
  SmoothPlan p{};
  p.fblocks = (int)tiles_of(maxF, AR_SMOOTH_BLOCK); p.vblocks = (int)tiles_of(maxV, AR_SMOOTH_BLOCK);
  p.steps = filter == SH_SMOOTH_LAPLACIAN ? iterations : 2 * iterations;
  p.last = filter == SH_SMOOTH_HC ? 0 : (p.steps & 1);      // (an HC iteration reads plane 0 and leaves P there)
  p.plane = 3 * v;
  p.vol0 = 0; p.vol1 = (size_t)B * p.fblocks * SH_SMO_TERMS; p.disp = 2 * p.vol1; p.head = p.disp + (size_t)B * p.vblocks * 2;
  SmoothBytes& z = p.bytes;
  z.smooth_nrow = ((size_t)sumV + B) * 4; z.smooth_nbr = 6 * f * 4; z.smooth_w = 6 * f * 8; z.smooth_pos = p.plane * 8;
  z.smooth_info = (size_t)B * SH_SMOOTH_INFO_BYTES; z.smooth_plane = 3 * p.plane * 8; z.smooth_pin = v * 4; z.smooth_mask = (v + 3) / 4 * 4;
  z.smooth_part = (p.head + (size_t)B * SH_SMO_HEAD) * 8;
  return p;
}

// The repair.  The regions of the repaired meshes follow from "topo.info", which the host reads before the first launch: mesh b has room
// for F_b + border_edges faces and V_b + border_edges / 3 vertices (a hole of L edges adds at most L faces and one vertex, and has at
// least three edges) and border_edges places in each array of "repair.edge".  off: the 3 (B + 1) starts of "repair.off".
struct RepairPlan { int blocks; std::vector<long long> off; RepairBytes bytes; };      // blocks: of 256 faces or vertices of the largest mesh
inline RepairPlan repair_plan(int B, int shell_records, int max_holes, long long maxV, long long maxF, long long sumF, const long long* voff, const long long* foff,
                              const sh_topology* info) {
  RepairPlan p;
  p.blocks = (int)tiles_of(maxF > maxV ? maxF : maxV, AR_REPAIR_BLOCK);
  p.off.assign(3 * ((size_t)B + 1), 0);
  long long *rf = p.off.data(), *rv = rf + B + 1, *re = rv + B + 1;
  for (int b = 0; b < B; ++b) {
    const long long e = info[b].border_edges > 0 ? info[b].border_edges : 0;
    rf[b + 1] = rf[b] + (foff[b + 1] - foff[b]) + e;
    rv[b + 1] = rv[b] + (voff[b + 1] - voff[b]) + e / 3;
    re[b + 1] = re[b] + e;
  }
  const size_t f = (size_t)(sumF > 0 ? sumF : 1);
  RepairBytes& z = p.bytes;
  z.repair_flip = (f + 3) / 4 * 4; z.repair_par = z.repair_flip;
  z.repair_faces = (size_t)(rf[B] > 0 ? rf[B] : 1) * 12; z.repair_verts = (size_t)(rv[B] > 0 ? rv[B] : 1) * 12;
  z.repair_info = (size_t)B * sizeof(sh_repair_info); z.repair_shells = (size_t)B * shell_records * sizeof(sh_repair_shell);
  z.repair_holes = (size_t)B * max_holes * sizeof(sh_repair_hole); z.repair_off = p.off.size() * 8;
  z.repair_work = (5 * f + (size_t)B * AR_REPAIR_HEAD) * 4; z.repair_edge = (size_t)AR_REPAIR_EDGE_ARRAYS * (size_t)(re[B] > 0 ? re[B] : 1) * 4;
  z.repair_term = 2 * f * 8;
  return p;
}

// The simplification.  Every array follows the vertices (mesh b at voff[b]; "simp.verts" and "simp.pos" three float32 and "simp.quad"
// AR_SIMP_Q doubles per vertex) or the faces (mesh b at foff[b]; "simp.faces" three int32 per face): an output is never larger than its
// input, so every size follows from the batch alone and a second call allocates nothing.  seg: the first vertex of every mesh, the
// segments of both sorts; state0: an empty box (lo above, hi below everything) and zero counts.
struct SimplifyPlan { int blocks = 0, vblocks = 0, fblocks = 0; std::vector<unsigned> seg, state0; SimplifyBytes bytes; };
inline ArthroError simplify_plan(int B, long long maxV, long long maxF, const long long* voff /* B + 1 */, long long sumF, SimplifyPlan* out) {
  SimplifyPlan p;
  if (voff[B] > 0x7fffffffLL) return {SH_ERR_NOMEM, "the batch has more than 2^31 - 1 vertices: its keys do not sort in one call"};
  p.vblocks = (int)tiles_of(maxV, AR_SIMP_BLOCK); p.fblocks = (int)tiles_of(maxF, AR_SIMP_BLOCK);
  p.blocks = p.vblocks > p.fblocks ? p.vblocks : p.fblocks;
  p.seg.resize((size_t)B + 1); p.state0.assign((size_t)B * AR_SIMP_HEAD, 0u);
  for (int b = 0; b <= B; ++b) p.seg[b] = (unsigned)voff[b];
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < 3; ++k) p.state0[(size_t)b * AR_SIMP_HEAD + k] = 0xffffffffu;
  const size_t v = (size_t)(voff[B] > 0 ? voff[B] : 1), f = (size_t)(sumF > 0 ? sumF : 1);
  SimplifyBytes& z = p.bytes;
  z.simp_verts = v * 12; z.simp_faces = f * 12; z.simp_map = v * 4; z.simp_info = (size_t)B * sizeof(sh_simplify_info);
  z.simp_state = (size_t)B * AR_SIMP_HEAD * 4; z.simp_seg = ((size_t)B + 1) * 4; z.simp_cell = (size_t)B * 8;
  z.simp_key = v * 8; z.simp_sorted = v * 8; z.simp_ukey = v * 8; z.simp_start = v * 4; z.simp_cid = v * 4; z.simp_mark = v * 4; z.simp_rank = v * 4;
  z.simp_quad = v * AR_SIMP_Q * 8; z.simp_pos = v * 12; z.simp_keep = f * 4; z.simp_frank = f * 4;
  *out = std::move(p);
  return arthro_ok();
}

// The face hierarchy (sh_scalar.h bvh_*).  "bvh.order", "bvh.loose", "bvh.key" and "bvh.sorted" follow the faces (mesh b at foff[b]) and
// "bvh.tri" nine float32 per face; "bvh.box" has six float32 per node, mesh b from base[b] = the sum of bvh_nodes_of(F_a) over the meshes
// before it -- room for a mesh without a loose face, known before the device has counted them; "bvh.off" SH_BVH_OFF_WORDS int32 and
// "bvh.state" AR_BVH_HEAD words per mesh.  levels: those of the largest mesh were all its faces tight -- the launches of k_bvh_level are
// levels - 1; leaf_blocks / node_blocks[k]: the workgroups per mesh that cover the leaves and level k of such a mesh.
// Refused: a batch whose faces or nodes are no int32 (the sort and "bvh.off" count in 32 bits).
struct BvhPlan {
  int fblocks = 0, levels = 0, leaf_blocks = 0, node_blocks[SH_BVH_MAX_LEVELS] = {};
  std::vector<int> base;            // B + 1: the first node of every mesh, the nodes of the batch behind the last
  std::vector<unsigned> seg;        // B + 1: the first key of every mesh
  std::vector<unsigned> state0;     // B x AR_BVH_HEAD: an empty box (lo above, hi below everything), no tight face
  BvhBytes bytes;
};
inline ArthroError bvh_plan(int B, const long long* foff /* B + 1 */, BvhPlan* out) {
  BvhPlan p;
  long long nodes = 0, maxF = 0;
  p.base.resize((size_t)B + 1); p.seg.resize((size_t)B + 1); p.state0.assign((size_t)B * AR_BVH_HEAD, 0u);
  if (foff[B] > 0x7fffffffLL) return {SH_ERR_NOMEM, "the batch has more than 2^31 - 1 faces: its keys do not sort in one call"};
  for (int b = 0; b < B; ++b) {
    const long long nf = foff[b + 1] - foff[b];
    if (nf < 0 || nf > SH_BVH_MAX_FACES) return {SH_ERR_ARG, "a mesh has more faces than an upload admits"};
    maxF = nf > maxF ? nf : maxF;
    p.base[b] = (int)nodes; p.seg[b] = (unsigned)foff[b];
    nodes += bvh_nodes_of(nf);
    if (nodes > 0x7fffffffLL) return {SH_ERR_NOMEM, "the batch has more than 2^31 - 1 nodes"};
    for (int k = 0; k < 3; ++k) p.state0[(size_t)b * AR_BVH_HEAD + k] = 0xffffffffu;
  }
  p.base[B] = (int)nodes; p.seg[B] = (unsigned)foff[B];
  p.fblocks = (int)tiles_of(maxF, AR_BVH_BLOCK);
  p.levels = bvh_levels_of(maxF);
  long long n = (maxF + SH_BVH_LEAF - 1) / SH_BVH_LEAF;
  p.leaf_blocks = (int)tiles_of(n, AR_BVH_BLOCK);
  for (int k = 0; k < p.levels; ++k) { p.node_blocks[k] = (int)tiles_of(n, AR_BVH_BLOCK); n = (n + SH_BVH_WIDTH - 1) / SH_BVH_WIDTH; }
  const size_t f = (size_t)(foff[B] > 0 ? foff[B] : 1);
  BvhBytes& z = p.bytes;
  z.bvh_order = f * 4; z.bvh_loose = f * 4; z.bvh_off = (size_t)B * SH_BVH_OFF_WORDS * 4; z.bvh_box = (size_t)(nodes > 0 ? nodes : 1) * 24; z.bvh_tri = f * 36;
  z.bvh_info = (size_t)B * sizeof(sh_bvh_info); z.bvh_state = (size_t)B * AR_BVH_HEAD * 4; z.bvh_base = ((size_t)B + 1) * 4; z.bvh_seg = ((size_t)B + 1) * 4;
  z.bvh_key = f * 8; z.bvh_sorted = f * 8;
  *out = std::move(p);
  return arthro_ok();
}
// the grid of k_cp_tree over Q points per mesh: chunks of one wave
inline int bvh_chunks(int Q) { return (Q + AR_BVH_CHUNK - 1) / AR_BVH_CHUNK; }

// Multi-start registration: the coarse stage is sh_register_points on Qc points, the fine stage on all Q, both on the "icp.*" buffers,
// which take the larger of the two sizes field by field (the split of the walk, and so "icp.cp_part", may be larger for the fewer points).
inline int ms_coarse_count(int Q, int coarse_points) { return coarse_points == 0 || coarse_points > Q ? Q : coarse_points; }
inline long long ms_coarse_index(long long j, int Q, int Qc) { return j * Q / Qc; }      // point j of the coarse set
struct MsPlan { int Qc; IcpPlan coarse, fine; IcpBytes icp; MsBytes bytes; };
inline MsPlan ms_plan(int B, int Q, bool per_humerus, long long maxF, int K, int coarse_points, int coarse_iter, int fine_iter) {
  const int Qc = ms_coarse_count(Q, coarse_points);
  MsPlan p{Qc, icp_plan(B, Qc, per_humerus, maxF, coarse_iter), icp_plan(B, Q, per_humerus, maxF, fine_iter), IcpBytes(), MsBytes()};
#define X(f, name, T, elem) p.icp.f = std::max(p.coarse.bytes.f, p.fine.bytes.f);
  ICP_BUFS(X)
#undef X
  p.bytes.ms_T0s = (size_t)B * K * 128; p.bytes.ms_points = (per_humerus ? (size_t)B * Qc : (size_t)Qc) * 24;
  p.bytes.ms_coarse = (size_t)B * K * sizeof(sh_registration); p.bytes.ms_best = (size_t)B * 8; p.bytes.ms_winner = (size_t)B * 4;
  return p;
}

// The pick rule: does candidate k (its status, pairs and rms) replace the best so far (winner < 0: none yet)?  The candidates come in
// ascending k, so "strictly smaller rms" is the order (rms, k).  A candidate with a status, too few pairs or a NaN rms never wins.
SH_HD bool ms_candidate_wins(int status, int pairs, double rms, int min_pairs, int winner, double best_rms) {
  if (status != 0 || pairs < min_pairs || !(rms == rms)) return false;
  return winner < 0 || rms < best_rms;
}

// ---- one ordered precheck per entry point: the first refusal, or SH_OK ------------------------------------------------------------------
inline ArthroError precheck_ray_cast(const sh_ray* rays, int R, int per_humerus, int cap, const ArthroFacts& f) {
  if (!f.ctx || !rays || R < 1 || R > SH_RAY_MAX || cap < 1 || cap > SH_RAY_MAX_HITS) return {SH_ERR_ARG, "bad argument (R in 1..65536, cap in 1..1024)"};
  if (const ArthroError e = resident(f); e.code) return e;
  const long long i = first_bad_ray(rays, per_humerus ? (size_t)f.B * R : (size_t)R);
  if (i >= 0) return {SH_ERR_ARG, "ray " + std::to_string(i) + " has a non-finite number or a zero direction"};
  return arthro_ok();
}

// (the order and the codes of precheck_ray_cast with cap = 1)
inline ArthroError precheck_ray_nearest(const sh_ray* rays, int R, int per_humerus, const ArthroFacts& f) {
  if (!f.ctx || !rays || R < 1 || R > SH_RAY_MAX) return {SH_ERR_ARG, "bad argument (R in 1..65536)"};
  return precheck_ray_cast(rays, R, per_humerus, 1, f);
}

inline ArthroError precheck_anp_hits(int cap, const int32_t* status, const ArthroFacts& f) {
  if (!f.ctx || !status || cap < 1 || cap > SH_RAY_MAX_HITS) return {SH_ERR_ARG, "bad argument (cap in 1..1024)"};
  if (const ArthroError e = resident(f); e.code) return e;
  if (!f.st->has_anp(f.batch_gen) || !f.landmarks) return {SH_ERR_STATE, "needs a collected run of the resident batch with SH_STAGE_ANP"};
  return arthro_ok();
}

inline ArthroError precheck_closest(const double* points, int Q, int per_humerus, const ArthroFacts& f) { return point_set(points, Q, SH_CLOSEST_MAX, per_humerus, f); }
inline ArthroError precheck_winding(const double* points, int Q, int per_humerus, const ArthroFacts& f) { return point_set(points, Q, SH_WINDING_MAX, per_humerus, f); }

inline ArthroError precheck_mass(const ArthroFacts& f) {
  if (!f.ctx) return {SH_ERR_ARG, "bad argument (no context)"};
  return resident(f);
}

inline bool sample_options_ok(const sh_sample_options* o) {
  return std::isfinite(o->radius) && o->radius >= 0.0 && o->max_rounds >= 1 && o->max_rounds <= SH_THIN_MAX_ROUNDS && o->reserved == 0;
}
inline ArthroError precheck_sample(int N, const uint64_t* seeds, const sh_sample_options* opt, const ArthroFacts& f) {
  if (!f.ctx || !seeds || !opt) return {SH_ERR_ARG, "bad argument (context, seeds and options must be given)"};
  if (N < 1 || N > SH_SAMPLE_MAX) return {SH_ERR_ARG, "bad argument (N in 1..1048576)"};
  if (!sample_options_ok(opt)) return {SH_ERR_ARG, "bad options (radius finite and >= 0, max_rounds in 1..32, reserved 0)"};
  if (opt->radius > 0.0 && N > SH_SAMPLE_THIN_MAX) return {SH_ERR_ARG, "bad argument (N in 1..65536 with a radius: the thinning looks at all pairs)"};
  return resident(f);
}

inline ArthroError precheck_topology(const sh_topology_options* opt, const ArthroFacts& f) {
  if (!f.ctx || !opt) return {SH_ERR_ARG, "bad argument (context and options must be given)"};
  if (opt->max_shells < 1 || opt->max_shells > SH_TOPO_MAX_SHELLS || opt->max_rounds < 1 || opt->max_rounds > SH_TOPO_MAX_ROUNDS || opt->reserved != 0)
    return {SH_ERR_ARG, "bad options (max_shells in 1..65536, max_rounds in 1..32, reserved 0)"};
  return resident(f);
}

// (the order and the codes of precheck_topology without its options)
inline ArthroError precheck_bvh(const ArthroFacts& f) {
  if (!f.ctx) return {SH_ERR_ARG, "bad argument (no context)"};
  return resident(f);
}
inline ArthroError precheck_query_accel(bool ctx, int mode) {
  if (!ctx || (mode != SH_ACCEL_OFF && mode != SH_ACCEL_BVH)) return {SH_ERR_ARG, "bad argument (mode SH_ACCEL_OFF or SH_ACCEL_BVH)"};
  return arthro_ok();
}

// incidence: "topo.vrow", "topo.vface" and "topo.adj" of the resident batch are there (a new batch removes them)
inline ArthroError precheck_vertex_fields(int weight, int smooth_rounds, bool incidence, const ArthroFacts& f) {
  if (!f.ctx) return {SH_ERR_ARG, "bad argument (no context)"};
  if ((weight != SH_VERT_WEIGHT_AREA && weight != SH_VERT_WEIGHT_ANGLE) || smooth_rounds < 0 || smooth_rounds > SH_VERT_MAX_SMOOTH)
    return {SH_ERR_ARG, "bad argument (weight 0 or 1, smooth_rounds in 0..64)"};
  if (const ArthroError e = resident(f); e.code) return e;
  if (!incidence) return {SH_ERR_STATE, "no incidence of the resident batch: call sh_mesh_topology first"};
  return arthro_ok();
}

// The lists of sh_geodesic against the resident batch (voff: its B + 1 vertex offsets on the host): the offsets ascend from 0, every
// source index lies in [0, V_b), every d0 is finite and >= 0.  -> the text of the first offence with its mesh, set and position, or "".
inline std::string geo_first_bad(int B, int K, const long long* voff, const int32_t* src_off, const int32_t* src, const double* d0) {
  if (src_off[0] != 0) return "src_off[0] is not 0";
  for (int p = 0; p < B * K; ++p) {
    const std::string where = "mesh " + std::to_string(p / K) + ", set " + std::to_string(p % K);
    if (src_off[p + 1] < src_off[p]) return where + ": src_off does not ascend";
    const long long nv = voff[p / K + 1] - voff[p / K];
    for (int i = src_off[p]; i < src_off[p + 1]; ++i) {
      const std::string at = where + ", position " + std::to_string(i - src_off[p]);
      if (!src || src[i] < 0 || src[i] >= nv) return at + ": source vertex " + (src ? std::to_string(src[i]) : std::string("(null)")) + " is not in [0, " + std::to_string(nv) + ")";
      if (d0 && !(std::isfinite(d0[i]) && d0[i] >= 0.0)) return at + ": d0 is not finite and >= 0";
    }
  }
  return "";
}

// incidence as in precheck_vertex_fields; voff: the host's vertex offsets of the resident batch (unused without one)
inline ArthroError precheck_geodesic(int mode, int K, double max_dist, const int32_t* src_off, const int32_t* src, const double* d0, const long long* voff, bool incidence,
                                     const ArthroFacts& f) {
  if (!f.ctx) return {SH_ERR_ARG, "bad argument (no context)"};
  if ((mode != SH_GEO_EDGES && mode != SH_GEO_UNFOLD) || K < 1 || K > SH_GEO_MAX_SETS || !(max_dist > 0.0) || !src_off)
    return {SH_ERR_ARG, "bad argument (mode 0 or 1, K in 1..16, max_dist +inf or > 0, src_off)"};
  if (f.B >= 1 && voff)
    if (const std::string bad = geo_first_bad(f.B, K, voff, src_off, src, d0); !bad.empty()) return {SH_ERR_ARG, "bad argument (" + bad + ")"};
  if (const ArthroError e = resident(f); e.code) return e;
  if (!incidence) return {SH_ERR_STATE, "no incidence of the resident batch: call sh_mesh_topology first"};
  return arthro_ok();
}

// incidence as in precheck_vertex_fields; has_pin: the call brings a mask; maxF: the faces of the largest resident mesh (its rows count in 32 bits)
inline ArthroError precheck_smooth(int filter, int weight, int iterations, int flags, double p0, double p1, bool has_pin, bool incidence, long long maxF, const ArthroFacts& f) {
  if (!f.ctx) return {SH_ERR_ARG, "bad argument (no context)"};
  if (filter < SH_SMOOTH_LAPLACIAN || filter > SH_SMOOTH_HC || (weight != SH_SMOOTH_UNIFORM && weight != SH_SMOOTH_INVLEN) || iterations < 0 || iterations > SH_SMOOTH_MAX_ITER ||
      (flags & ~(SH_SMOOTH_PIN_BORDER | SH_SMOOTH_KEEP_VOLUME)) != 0)
    return {SH_ERR_ARG, "bad argument (filter 0, 1 or 2, weight 0 or 1, iterations in 0..256, flags 0..3)"};
  const bool hc = filter == SH_SMOOTH_HC;
  if (!std::isfinite(p0) || !(p0 >= 0.0 && p0 <= 1.0)) return {SH_ERR_ARG, std::string("bad argument (") + (hc ? "alpha" : "lambda") + " in 0..1)"};
  if (!std::isfinite(p1)) return {SH_ERR_ARG, std::string("bad argument (") + (hc ? "beta" : "mu") + " is not finite)"};
  if (hc && !(p1 >= 0.0 && p1 <= 1.0)) return {SH_ERR_ARG, "bad argument (beta in 0..1)"};
  if (filter == SH_SMOOTH_TAUBIN && !(p1 >= -1.0 && p1 <= 0.0)) return {SH_ERR_ARG, "bad argument (mu in -1..0)"};
  if ((flags & SH_SMOOTH_KEEP_VOLUME) && (has_pin || (flags & SH_SMOOTH_PIN_BORDER)))
    return {SH_ERR_ARG, "bad argument (SH_SMOOTH_KEEP_VOLUME with a pin: the scaling would move pinned vertices)"};
  if (const ArthroError e = resident(f); e.code) return e;
  if (!incidence) return {SH_ERR_STATE, "no incidence of the resident batch: call sh_mesh_topology first"};
  if (6 * maxF > 0x7fffffffLL) return {SH_ERR_NOMEM, "a mesh has more than 2^31 - 1 places for neighbours"};
  return arthro_ok();
}

// topology: "topo.adj", "topo.label", "topo.info" and "topo.shells" of the resident batch are there (a new batch removes them)
inline ArthroError precheck_repair(const sh_repair_options* opt, bool topology, const ArthroFacts& f) {
  if (!f.ctx || !opt) return {SH_ERR_ARG, "bad argument (context and options must be given)"};
  if (opt->orient < SH_REPAIR_NONE || opt->orient > SH_REPAIR_NESTED || opt->fill < SH_REPAIR_FILL_NONE || opt->fill > SH_REPAIR_CENTROID || opt->max_hole_edges < 3 ||
      opt->max_holes < 1 || opt->max_holes > SH_REPAIR_MAX_HOLES || opt->max_rounds < 1 || opt->max_rounds > SH_REPAIR_MAX_ROUNDS || opt->reserved != 0)
    return {SH_ERR_ARG, "bad options (orient in 0..3, fill in 0..2, max_hole_edges >= 3, max_holes in 1..65536, max_rounds in 1..1048576, reserved 0)"};
  if (const ArthroError e = resident(f); e.code) return e;
  if (!topology) return {SH_ERR_STATE, "no topology of the resident batch: call sh_mesh_topology first"};
  return arthro_ok();
}

// incidence: "topo.vrow" and "topo.vface" of the resident batch are there (a new batch removes them); cell: f.B entries
inline ArthroError precheck_simplify(const sh_simplify_options* opt, const double* cell, bool incidence, const ArthroFacts& f) {
  if (!f.ctx || !opt) return {SH_ERR_ARG, "bad argument (context and options must be given)"};
  if ((opt->place != SH_SIMPLIFY_MEAN && opt->place != SH_SIMPLIFY_QUADRIC) || opt->reserved != 0 || !std::isfinite(opt->reg) || !(opt->reg >= 0.0 && opt->reg <= 1.0) ||
      !std::isfinite(opt->clamp) || !(opt->clamp > 0.0))
    return {SH_ERR_ARG, "bad options (place 0 or 1, reserved 0, reg finite in 0..1, clamp finite and > 0)"};
  if (!cell) return {SH_ERR_ARG, "bad argument (cell must be given: one per resident mesh)"};
  for (int b = 0; b < f.B; ++b)
    if (!std::isfinite(cell[b]) || !(cell[b] > 0.0)) return {SH_ERR_ARG, "bad argument (cell[" + std::to_string(b) + "] is not finite and > 0)"};
  if (const ArthroError e = resident(f); e.code) return e;
  if (!incidence) return {SH_ERR_STATE, "no incidence of the resident batch: call sh_mesh_topology first"};
  return arthro_ok();
}

static const char* const AR_ICP_OPTIONS = "options (metric 0 or 1, max_iter in 1..64, reject > 0, tol >= 0 and finite)";
static const char* const AR_NOT_RIGID = " is not a rigid matrix (last row 0 0 0 1, |R^T R - I| <= 1e-9, det > 0)";

inline ArthroError precheck_register(const double* points, int Q, int per_humerus, const double* T0, const sh_icp_options* opt, const ArthroFacts& f) {
  if (!f.ctx || !points || !opt) return {SH_ERR_ARG, "bad argument (context, points and options must be given)"};
  const ArthroError args = icp_options_ok(opt) ? arthro_ok() : ArthroError{SH_ERR_ARG, std::string("bad ") + AR_ICP_OPTIONS};
  if (const ArthroError e = point_set(points, Q, SH_CLOSEST_MAX, per_humerus, f, args); e.code) return e;
  if (T0)
    for (int b = 0; b < f.B; ++b)
      if (!rigid_start_ok(T0 + 16 * (size_t)b)) return {SH_ERR_ARG, "T0 of humerus " + std::to_string(b) + AR_NOT_RIGID};
  return arthro_ok();
}

inline ArthroError precheck_multistart(const double* points, int Q, int per_humerus, const double* T0s, int K, const sh_icp_options* coarse,
                                       int coarse_points, int min_pairs, const sh_icp_options* fine, const ArthroFacts& f) {
  if (!f.ctx || !points || !T0s || !coarse || !fine) return {SH_ERR_ARG, "bad argument (context, points, T0s and both options must be given)"};
  const bool sizes = K >= 1 && K <= SH_MS_MAX_STARTS && coarse_points >= 0 && min_pairs >= 6;
  const ArthroError args = !sizes                   ? ArthroError{SH_ERR_ARG, "bad argument (K in 1..64, coarse_points >= 0, min_pairs >= 6)"}
                           : !icp_options_ok(coarse) ? ArthroError{SH_ERR_ARG, std::string("bad coarse ") + AR_ICP_OPTIONS}
                           : !icp_options_ok(fine)   ? ArthroError{SH_ERR_ARG, std::string("bad fine ") + AR_ICP_OPTIONS}
                                                     : arthro_ok();
  if (const ArthroError e = point_set(points, Q, SH_CLOSEST_MAX, per_humerus, f, args); e.code) return e;
  for (int b = 0; b < f.B; ++b)
    for (int k = 0; k < K; ++k)
      if (!rigid_start_ok(T0s + 16 * ((size_t)b * K + k))) return {SH_ERR_ARG, "start " + std::to_string(k) + " of humerus " + std::to_string(b) + AR_NOT_RIGID};
  return arthro_ok();
}

}  // namespace sh
