// sh_query_host.h -- the entry points of the queries of the resident batch: the rays, sh_ray_cast / sh_anp_axis_hits (k_rays.h), the
// closest surface points, sh_closest_points (k_closest.h), the winding numbers, sh_winding_numbers (k_winding.h), the registration of
// point sets, sh_register_points (k_icp.h) and sh_register_multistart (k_ms.h), the mass properties, sh_mass_properties (k_mass.h), the surface samples, sh_sample_surface
// (k_sample.h), the mesh topology, sh_mesh_topology (k_topo.h), the vertex fields, sh_vertex_fields (k_vert.h), the geodesics, sh_geodesic (k_geo.h), the smoothing of the vertices, sh_smooth_vertices (k_smooth.h), the repair, sh_mesh_repair (k_repair.h), the simplification, sh_mesh_simplify (k_simplify.h), and the face hierarchy, sh_mesh_bvh / sh_set_query_accel (k_bvh.h).
// Every one reads the mesh and changes no state of the arthroplasty chain.  Host code of shoulder_hip.hip, included there EXACTLY
// ONCE, right behind sh_arthro_host.h (arthro_facts, arthro_refuse) and for its reason: a header, not a unit.
// What a query DECIDES is sh_query.h (checks, first refusal, plan, buffer sizes).  Every entry point here reads:
// precheck -> ensure_bytes -> view_of -> enqueue -> copies back -> synchronise.
#pragma once

static_assert(AR_RAY_TILE == SH_RAY_TILE && AR_RAY_CHUNK == SH_RAY_CHUNK && AR_RAY_KEY_BYTES == sizeof(RayKey), "sh_query.h: ray tile, ray chunk, RayKey");
static_assert(AR_CP_TILE == SH_CP_TILE && AR_CP_CHUNK == SH_CP_CHUNK && AR_CP_PART_BYTES == sizeof(CpPart), "sh_query.h: closest-point tile, chunk, CpPart");
static_assert(AR_WN_TILE == SH_WN_TILE && AR_WN_CHUNK == SH_WN_CHUNK && AR_WN_BLOCK == SH_WIND_BLOCK, "sh_query.h: winding tile, chunk, block");
static_assert(AR_ICP_TERMS == SH_ICP_TERMS && AR_ICP_TSTRIDE == SH_ICP_TSTRIDE, "sh_query.h: registration terms, stride of icp.T");
static_assert(AR_MASS_TERMS == SH_MASS_TERMS, "sh_query.h: mass terms");
static_assert(AR_SAMP_CHUNK == SH_SAMP_CHUNK && AR_SAMP_HEAD == SH_SAMP_HEAD, "sh_query.h: sample chunk, head of samp.state");
static_assert(AR_TOPO_BLOCK == SH_TOPO_BLOCK && AR_TOPO_HEAD == SH_TOPO_HEAD, "sh_query.h: topology block, head of topo.state");
static_assert(AR_VERT_BLOCK == SH_VERT_BLOCK && AR_VERT_FACE == SH_VTX_FACE, "sh_query.h: vertex block, doubles of a face record");

// ---- rays, every hit (k_rays.h, k_raytree.h); the anatomic-neck rays also read the last run ----
static int bvh_build(sh_ctx* c, const char* fn);

// THE ONE PLACE the switch of sh_set_query_accel is read for rays, as cp_walk_join is for points: do the rays of this call descend the
// hierarchy?  Not the box-frame rays of sh_anp_axis_hits (T_obb): their corners are the vertices under "obb_transform", which the index
// does not hold.  The plan of a call and its run ask here, so they agree.
static bool ray_tree_mode(const sh_ctx* c, bool box) { return !box && c->query_accel == SH_ACCEL_BVH; }
// the index, built when "bvh.order" is not resident (a new batch removed it)
static int ray_tree_index(sh_ctx* c, const char* fn) { return c->at("bvh.order") ? SH_OK : bvh_build(c, fn); }

// count -> scan -> the total to the host -> "ray.pool" -> fill -> sort -> copies back.  "ray.rays" (and "ray.status" with `box`) are filled
// by the caller on the stream; T_obb / hstatus: the box transforms and the humeri to leave out (sh_anp_axis_hits), or null.  In tree mode
// count and fill are k_ray_tree (one ray per lane: plain stores, nothing to clear); scan, pool and sort are the same launches.
static int ray_run(sh_ctx* c, const RayPlan& plan, int R, int per_humerus, int cap, const double* T_obb, const int* hstatus, sh_ray_hit* hits, int32_t* counts) {
  int rc;
  const int B = c->B;
  const size_t n = plan.rays;
  const bool box = T_obb != nullptr;
  if (ray_tree_mode(c, box)) {
    if ((rc = ray_tree_index(c, "the ray walk")) != SH_OK) return rc;
    RayView v = view_of<RayView>(c);
    BvhBufs t = view_of<BvhBufs>(c);
    const dim3 grid((unsigned)plan.chunks, (unsigned)B), block(SH_BVH_CHUNK);
    LAUNCH(c, "k_ray_tree", k_ray_tree<false>, grid, block, v.verts, v.faces, v.voff, v.foff, (const int*)t.bvh_order, (const int*)t.bvh_loose, (const int*)t.bvh_off,
           (const float*)t.bvh_box, (const float*)t.bvh_tri, (const double*)v.ray_rays, R, per_humerus, v.ray_counts, (const unsigned long long*)nullptr, (int*)nullptr,
           (RayKey*)nullptr);
    LAUNCH(c, "k_ray_scan", k_ray_scan, dim3(1), dim3(1024), (const int*)v.ray_counts, (long long)n, v.ray_offs);
    unsigned long long total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, v.ray_offs + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ENS_SHARED("ray.pool", ray_pool_bytes(total), 8);
    v = view_of<RayView>(c);
    t = view_of<BvhBufs>(c);
    LAUNCH(c, "k_ray_tree", k_ray_tree<true>, grid, block, v.verts, v.faces, v.voff, v.foff, (const int*)t.bvh_order, (const int*)t.bvh_loose, (const int*)t.bvh_off,
           (const float*)t.bvh_box, (const float*)t.bvh_tri, (const double*)v.ray_rays, R, per_humerus, v.ray_counts, (const unsigned long long*)v.ray_offs, v.ray_cursor,
           v.ray_pool);
    LAUNCH(c, "k_ray_sort", k_ray_sort<false>, dim3((unsigned)n), dim3(64), (const double*)v.ray_rays, R, per_humerus, (const unsigned long long*)v.ray_offs,
           (const int*)v.ray_cursor, (const RayKey*)v.ray_pool, T_obb, cap, v.ray_hits);
    if (hits) HIPCHK(c, hipMemcpyAsync(hits, v.ray_hits, n * cap * sizeof(sh_ray_hit), hipMemcpyDeviceToHost, c->stream));
    if (counts) HIPCHK(c, hipMemcpyAsync(counts, v.ray_counts, n * 4, hipMemcpyDeviceToHost, c->stream));
    return SH_OK;
  }
  RayView v = view_of<RayView>(c);
  HIPCHK(c, hipMemsetAsync(v.ray_counts, 0, n * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(v.ray_cursor, 0, n * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(v.ray_blockhit, 0, plan.bytes.ray_blockhit, c->stream));
  const dim3 grid((unsigned)plan.tmax, (unsigned)B, (unsigned)plan.chunks), block(SH_RAY_TILE);
  LAUNCH(c, "k_ray_count", box ? k_ray_count<true> : k_ray_count<false>, grid, block, v.verts, v.faces, v.voff, v.foff, T_obb, hstatus, (const double*)v.ray_rays, R,
         per_humerus, v.ray_counts, v.ray_blockhit);
  LAUNCH(c, "k_ray_scan", k_ray_scan, dim3(1), dim3(1024), (const int*)v.ray_counts, (long long)n, v.ray_offs);
  unsigned long long total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, v.ray_offs + n, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ENS_SHARED("ray.pool", ray_pool_bytes(total), 8);
  v = view_of<RayView>(c);
  LAUNCH(c, "k_ray_fill", box ? k_ray_fill<true> : k_ray_fill<false>, grid, block, v.verts, v.faces, v.voff, v.foff, T_obb, hstatus, (const double*)v.ray_rays, R,
         per_humerus, (const unsigned long long*)v.ray_offs, v.ray_cursor, v.ray_pool, v.ray_blockhit);
  LAUNCH(c, "k_ray_sort", box ? k_ray_sort<true> : k_ray_sort<false>, dim3((unsigned)n), dim3(64), (const double*)v.ray_rays, R, per_humerus,
         (const unsigned long long*)v.ray_offs, (const int*)v.ray_cursor, (const RayKey*)v.ray_pool, T_obb, cap, v.ray_hits);
  if (hits) HIPCHK(c, hipMemcpyAsync(hits, v.ray_hits, n * cap * sizeof(sh_ray_hit), hipMemcpyDeviceToHost, c->stream));
  if (counts) HIPCHK(c, hipMemcpyAsync(counts, v.ray_counts, n * 4, hipMemcpyDeviceToHost, c->stream));
  return SH_OK;
}

int sh_ray_cast(sh_ctx* c, const sh_ray* rays, int R, int per_humerus, int cap, sh_ray_hit* hits, int32_t* counts) {
  if (const ArthroError e = precheck_ray_cast(rays, R, per_humerus, cap, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_ray_cast", e);
  HIPCHK(c, hipSetDevice(c->device));
  const RayPlan plan = ray_plan(c->B, R, per_humerus != 0, cap, c->maxF, false, ray_tree_mode(c, false));
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const RayView v = view_of<RayView>(c);
  HIPCHK(c, hipMemcpyAsync(v.ray_rays, rays, plan.bytes.ray_rays, hipMemcpyHostToDevice, c->stream));
  if (int rc = ray_run(c, plan, R, per_humerus != 0, cap, nullptr, nullptr, hits, counts)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// The nearest hit of every ray: row 0 of sh_ray_cast's answer, resident as "ray.near".  SH_ACCEL_OFF: the chain above with cap = 1 and a
// copy of its B x R x 1 records; SH_ACCEL_BVH: k_ray_near alone, and the host looks at nothing before the result.
int sh_ray_nearest(sh_ctx* c, const sh_ray* rays, int R, int per_humerus, sh_ray_hit* hit) {
  if (const ArthroError e = precheck_ray_nearest(rays, R, per_humerus, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_ray_nearest", e);
  HIPCHK(c, hipSetDevice(c->device));
  const bool tree = ray_tree_mode(c, false);
  const RayPlan plan = ray_plan(c->B, R, per_humerus != 0, 1, c->maxF, false, tree, true);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  if (int rc = ensure_shared(c, "ray.near", plan.near, 8)) return rc;
  if (tree) {
    if (int rc = ray_tree_index(c, "sh_ray_nearest")) return rc;
    const RayView v = view_of<RayView>(c);
    const BvhBufs t = view_of<BvhBufs>(c);
    HIPCHK(c, hipMemcpyAsync(v.ray_rays, rays, plan.bytes.ray_rays, hipMemcpyHostToDevice, c->stream));
    LAUNCH(c, "k_ray_near", k_ray_near, dim3((unsigned)plan.chunks, (unsigned)c->B), dim3(SH_BVH_CHUNK), v.verts, v.faces, v.voff, v.foff, (const int*)t.bvh_order,
           (const int*)t.bvh_loose, (const int*)t.bvh_off, (const float*)t.bvh_box, (const float*)t.bvh_tri, (const double*)v.ray_rays, R, per_humerus != 0 ? 1 : 0,
           (sh_ray_hit*)c->at("ray.near"));
  } else {
    const RayView v = view_of<RayView>(c);
    HIPCHK(c, hipMemcpyAsync(v.ray_rays, rays, plan.bytes.ray_rays, hipMemcpyHostToDevice, c->stream));
    if (int rc = ray_run(c, plan, R, per_humerus != 0, 1, nullptr, nullptr, nullptr, nullptr)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->at("ray.near"), c->at("ray.hits"), plan.near, hipMemcpyDeviceToDevice, c->stream));      // (cap = 1: row 0 is all of it)
  }
  if (hit) HIPCHK(c, hipMemcpyAsync(hit, c->at("ray.near"), plan.near, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

int sh_anp_axis_hits(sh_ctx* c, int cap, sh_ray_hit* hits, int32_t* counts, int32_t* status) {
  if (const ArthroError e = precheck_anp_hits(cap, status, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_anp_axis_hits", e);
  const double* plane = (const double*)c->at("anp.plane");
  const double* T_obb = (const double*)c->at("obb_transform");
  const sh_landmarks* lm = (const sh_landmarks*)c->at("landmarks");
  if (!plane || !T_obb || !lm) return fail(c, SH_ERR_STATE, "sh_anp_axis_hits: the buffers of the anatomic-neck stage are not there");
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B;
  const RayPlan plan = ray_plan(B, 4, true, cap, c->maxF, true);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const RayView v = view_of<RayView>(c);
  LAUNCH(c, "k_ray_anp_rays", k_ray_anp_rays, dim3((unsigned)((B + 63) / 64)), dim3(64), lm, plane, B, v.ray_rays, v.ray_status);
  if (int rc = ray_run(c, plan, 4, 1, cap, T_obb, (const int*)v.ray_status, hits, counts)) return rc;
  HIPCHK(c, hipMemcpyAsync(status, v.ray_status, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- the face hierarchy (k_bvh.h) ----
static_assert(AR_BVH_BLOCK == SH_BVH_BLOCK && AR_BVH_HEAD == SH_BVH_HEAD && AR_BVH_CHUNK == SH_BVH_CHUNK, "sh_query.h: hierarchy block, head of bvh.state, chunk of the walk");

// The build, enqueued on the context's stream: the offsets and the empty boxes to the device -> class -> key -> sort -> emit -> leaves ->
// a launch per level above them; the host looks at nothing in between (the temporary storage of the sort is sized on the host).
static int bvh_enqueue(sh_ctx* c, const char* fn) {
  BvhPlan plan;
  if (const ArthroError e = bvh_plan(c->B, c->h_foff.data(), &plan); e.code) return arthro_refuse(c, fn, e);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  BvhView v = view_of<BvhView>(c);
  const int B = c->B;
  const unsigned nkeys = (unsigned)c->sumF;
  size_t tmp_bytes = 0;
  HIPCHK(c, rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, (const unsigned long long*)v.bvh_key, v.bvh_sorted, nkeys, (unsigned)B, (const unsigned*)v.bvh_seg,
                                               (const unsigned*)v.bvh_seg + 1, 0u, 63u, c->stream));
  if (int rc = ensure_shared(c, "bvh.tmp", tmp_bytes ? tmp_bytes : 16, 1)) return rc;
  v = view_of<BvhView>(c);
  void* tmp = c->at("bvh.tmp");
  HIPCHK(c, hipMemcpyAsync(v.bvh_base, plan.base.data(), plan.bytes.bvh_base, hipMemcpyHostToDevice, c->stream));      // (pageable: staged before the call returns)
  HIPCHK(c, hipMemcpyAsync(v.bvh_seg, plan.seg.data(), plan.bytes.bvh_seg, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(v.bvh_state, plan.state0.data(), plan.bytes.bvh_state, hipMemcpyHostToDevice, c->stream));
  const dim3 fblocks((unsigned)plan.fblocks, (unsigned)B), lanes(SH_BVH_BLOCK);
  LAUNCH(c, "k_bvh_class", k_bvh_class, fblocks, lanes, v.verts, v.faces, v.voff, v.foff, v.bvh_state);
  LAUNCH(c, "k_bvh_key", k_bvh_key, fblocks, lanes, v.verts, v.faces, v.voff, v.foff, (const unsigned*)v.bvh_state, v.bvh_key);
  HIPCHK(c, rocprim::segmented_radix_sort_keys(tmp, tmp_bytes, (const unsigned long long*)v.bvh_key, v.bvh_sorted, nkeys, (unsigned)B, (const unsigned*)v.bvh_seg,
                                               (const unsigned*)v.bvh_seg + 1, 0u, 63u, c->stream));
  LAUNCH(c, "k_bvh_emit", k_bvh_emit, fblocks, lanes, v.verts, v.faces, v.voff, v.foff, (const unsigned long long*)v.bvh_sorted, (const unsigned*)v.bvh_state,
         (const int*)v.bvh_base, v.bvh_order, v.bvh_loose, v.bvh_tri, v.bvh_off, v.bvh_info);
  LAUNCH(c, "k_bvh_leaves", k_bvh_leaves, dim3((unsigned)plan.leaf_blocks, (unsigned)B), lanes, v.foff, (const float*)v.bvh_tri, (const int*)v.bvh_off, v.bvh_box);
  for (int k = 1; k < plan.levels; ++k)
    LAUNCH(c, "k_bvh_level", k_bvh_level, dim3((unsigned)plan.node_blocks[k], (unsigned)B), lanes, (const int*)v.bvh_off, v.bvh_box, k);
  return SH_OK;
}

// ... and a build that did not get through leaves no "bvh.order" behind: that name is what says "the index of this batch is resident"
static int bvh_build(sh_ctx* c, const char* fn) {      // (declared above the rays, which build it too)
  const int rc = bvh_enqueue(c, fn);
  if (rc != SH_OK)
    if (auto it = c->bufs.find("bvh.order"); it != c->bufs.end()) {
      if (it->second.p) (void)hipFree(it->second.p);
      c->bufs.erase(it);
    }
  return rc;
}

int sh_mesh_bvh(sh_ctx* c, sh_bvh_info* out) {
  if (const ArthroError e = precheck_bvh(arthro_facts(c)); e.code) return arthro_refuse(c, "sh_mesh_bvh", e);
  HIPCHK(c, hipSetDevice(c->device));
  if (int rc = bvh_build(c, "sh_mesh_bvh")) return rc;
  if (out) HIPCHK(c, hipMemcpyAsync(out, c->at("bvh.info"), (size_t)c->B * sizeof(sh_bvh_info), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

int sh_set_query_accel(sh_ctx* c, int mode) {
  if (const ArthroError e = precheck_query_accel(c != nullptr, mode); e.code) return arthro_refuse(c, "sh_set_query_accel", e);
  c->query_accel = mode;
  return SH_OK;
}
int sh_get_query_accel(const sh_ctx* c) { return c ? c->query_accel : SH_ACCEL_OFF; }

// ---- closest surface points (k_closest.h) ----
// The walk and its join for B x Q device points `pts` (per != 0: Q of its own for every humerus) over S face splits, from `part` into `out`.
// THE ONE PLACE sh_closest_points and the evaluations of a registration go through: with SH_ACCEL_BVH the walk is k_cp_tree over the
// hierarchy (built here when "bvh.order" is not resident: a new batch removed it), one partial per point, and the same join with S = 1.
// (The rays read the switch in ray_tree_mode.)
static int cp_walk_join(sh_ctx* c, const MeshBufs& m, const double* pts, int Q, int per, int chunks, int S, size_t points, CpPart* part, sh_closest* out) {
  if (c->query_accel == SH_ACCEL_BVH) {
    if (!c->at("bvh.order"))
      if (int rc = bvh_build(c, "the closest-point step")) return rc;
    const BvhBufs t = view_of<BvhBufs>(c);
    LAUNCH(c, "k_cp_tree", k_cp_tree, dim3((unsigned)bvh_chunks(Q), (unsigned)c->B), dim3(SH_BVH_CHUNK), m.verts, m.faces, m.voff, m.foff, (const int*)t.bvh_order,
           (const int*)t.bvh_loose, (const int*)t.bvh_off, (const float*)t.bvh_box, (const float*)t.bvh_tri, pts, Q, per, part);
    LAUNCH(c, "k_cp_join", k_cp_join, dim3((unsigned)((points + 255) / 256)), dim3(256), m.verts, m.faces, m.voff, m.foff, pts, Q, per, 1, (const CpPart*)part,
           (long long)points, out);
    return SH_OK;
  }
  LAUNCH(c, "k_cp_walk", k_cp_walk, dim3((unsigned)chunks, (unsigned)c->B, (unsigned)S), dim3(SH_CP_CHUNK), m.verts, m.faces, m.voff, m.foff, pts, Q, per, S, part);
  LAUNCH(c, "k_cp_join", k_cp_join, dim3((unsigned)((points + 255) / 256)), dim3(256), m.verts, m.faces, m.voff, m.foff, pts, Q, per, S, (const CpPart*)part,
         (long long)points, out);
  return SH_OK;
}

int sh_closest_points(sh_ctx* c, const double* points, int Q, int per_humerus, sh_closest* out) {
  if (const ArthroError e = precheck_closest(points, Q, per_humerus, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_closest_points", e);
  HIPCHK(c, hipSetDevice(c->device));
  const CpPlan plan = cp_plan(c->B, Q, per_humerus != 0, c->maxF);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const CpView v = view_of<CpView>(c);
  HIPCHK(c, hipMemcpyAsync(v.cp_points, points, plan.bytes.cp_points, hipMemcpyHostToDevice, c->stream));
  if (int rc = cp_walk_join(c, v, v.cp_points, Q, per_humerus != 0 ? 1 : 0, plan.chunks, plan.S, plan.points, v.cp_part, v.cp_out)) return rc;
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.cp_out, plan.bytes.cp_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- generalized winding numbers (k_winding.h) ----
int sh_winding_numbers(sh_ctx* c, const double* points, int Q, int per_humerus, sh_winding* out) {
  if (const ArthroError e = precheck_winding(points, Q, per_humerus, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_winding_numbers", e);
  HIPCHK(c, hipSetDevice(c->device));
  const WnPlan plan = wn_plan(c->B, Q, per_humerus != 0, c->maxF);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const WnView v = view_of<WnView>(c);
  HIPCHK(c, hipMemcpyAsync(v.wn_points, points, plan.bytes.wn_points, hipMemcpyHostToDevice, c->stream));
  LAUNCH(c, "k_wn_walk", k_wn_walk, dim3((unsigned)plan.chunks, (unsigned)c->B, (unsigned)plan.S), dim3(SH_WN_CHUNK), v.verts, v.faces, v.voff, v.foff,
         (const double*)v.wn_points, Q, per_humerus != 0 ? 1 : 0, plan.S, plan.stride, v.wn_part);
  LAUNCH(c, "k_wn_join", k_wn_join, dim3((unsigned)((plan.points + 255) / 256)), dim3(256), v.foff, Q, plan.S, plan.stride, (const double*)v.wn_part,
         (long long)plan.points, v.wn_out);
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.wn_out, plan.bytes.wn_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- rigid registration of point sets (k_icp.h) ----
// The chain of one registration, enqueued on the context's stream: the mean of the input points (phase 0), then max_iter + 1 evaluations
// of move -> walk -> join -> sums -> step.  `pts` are the device points (Q, shared or per humerus); "icp.T", "icp.flags", "icp.out" and
// "icp.hist" are in place.  Both entry points below run exactly this.
static int icp_chain(sh_ctx* c, const IcpView& v, const double* pts, int Q, int per, const IcpPlan& plan, const sh_icp_options* opt) {
  const int B = c->B, K = opt->max_iter;
  const dim3 blocks((unsigned)plan.chunks, (unsigned)B), lanes(SH_ICP_BLOCK);
  // one pass over the blocks: phase 0 the mean of the input points, phase 1 evaluation k
  // (LAUNCH ends in HIPCHK(hipGetLastError()): a launch that fails returns SH_ERR_HIP from the lambda, which the callers pass on)
  auto sum_step = [&](int phase, int k) -> int {
    LAUNCH(c, "k_icp_sum", k_icp_sum, blocks, lanes, v.verts, v.faces, v.voff, v.foff, pts, (const double*)v.icp_moved,
           (const sh_closest*)v.icp_near, Q, per, phase, (int)opt->metric, opt->reject, (const double*)v.icp_T, (const int*)v.icp_flags, v.icp_part);
    LAUNCH(c, "k_icp_step", k_icp_step, dim3((unsigned)B), dim3(64), (const double*)v.icp_part, plan.chunks, Q, phase, (int)opt->metric, k, K, opt->tol,
           v.icp_T, v.icp_flags, v.icp_hist, v.icp_out);
    return SH_OK;
  };
  if (int rc = sum_step(0, 0)) return rc;
  for (int k = 0; k <= K; ++k) {
    LAUNCH(c, "k_icp_move", k_icp_move, blocks, lanes, pts, Q, per, (const double*)v.icp_T, (const int*)v.icp_flags, v.icp_moved);
    if (int rc = cp_walk_join(c, v, v.icp_moved, Q, 1, plan.chunks, plan.S, plan.points, v.icp_cp_part, v.icp_near)) return rc;
    if (int rc = sum_step(1, k)) return rc;
  }
  return SH_OK;
}

int sh_register_points(sh_ctx* c, const double* points, int Q, int per_humerus, const double* T0, const sh_icp_options* opt, sh_registration* out,
                       double* history) {
  if (const ArthroError e = precheck_register(points, Q, per_humerus, T0, opt, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_register_points", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, per = per_humerus != 0 ? 1 : 0, K = opt->max_iter;
  const IcpPlan plan = icp_plan(B, Q, per != 0, c->maxF, K);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const IcpView v = view_of<IcpView>(c);
  std::vector<double> start((size_t)B * SH_ICP_TSTRIDE, 0.0);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 16; ++i) start[(size_t)b * SH_ICP_TSTRIDE + i] = T0 ? T0[16 * (size_t)b + i] : (i % 5 == 0 ? 1.0 : 0.0);
  HIPCHK(c, hipMemcpyAsync(v.icp_T, start.data(), plan.bytes.icp_T, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(v.icp_points, points, plan.bytes.icp_points, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(v.icp_flags, 0, plan.bytes.icp_flags, c->stream));
  HIPCHK(c, hipMemsetAsync(v.icp_hist, 0, plan.bytes.icp_hist, c->stream));
  HIPCHK(c, hipMemsetAsync(v.icp_out, 0, plan.bytes.icp_out, c->stream));
  if (int rc = icp_chain(c, v, (const double*)v.icp_points, Q, per, plan, opt)) return rc;
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.icp_out, plan.bytes.icp_out, hipMemcpyDeviceToHost, c->stream));
  if (history) HIPCHK(c, hipMemcpyAsync(history, v.icp_hist, plan.bytes.icp_hist, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- multi-start registration (k_ms.h around the chain above) ----
int sh_register_multistart(sh_ctx* c, const double* points, int Q, int per_humerus, const double* T0s, int K, const sh_icp_options* coarse,
                           int coarse_points, int min_pairs, const sh_icp_options* fine, sh_registration* out, sh_registration* coarse_out,
                           int32_t* winner) {
  if (const ArthroError e = precheck_multistart(points, Q, per_humerus, T0s, K, coarse, coarse_points, min_pairs, fine, arthro_facts(c)); e.code)
    return arthro_refuse(c, "sh_register_multistart", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, per = per_humerus != 0 ? 1 : 0;
  const MsPlan plan = ms_plan(B, Q, per != 0, c->maxF, K, coarse_points, coarse->max_iter, fine->max_iter);
  const int Qc = plan.Qc;
  if (int rc = ensure_bytes(c, plan.icp)) return rc;      // (the field-wise maximum of the coarse and the fine sizes: no stage re-allocates)
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const IcpView v = view_of<IcpView>(c);
  const MsBufs m = view_of<MsBufs>(c);
  const size_t sets = per ? (size_t)B : 1;
  std::vector<double> cpts(sets * Qc * 3);      // (pageable: the copy is staged before the call returns)
  for (size_t s = 0; s < sets; ++s)
    for (int j = 0; j < Qc; ++j) {
      const double* p = points + 3 * (s * Q + (size_t)ms_coarse_index(j, Q, Qc));
      double* q = &cpts[3 * (s * Qc + j)];
      q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    }
  HIPCHK(c, hipMemcpyAsync(m.ms_points, cpts.data(), plan.bytes.ms_points, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(m.ms_T0s, T0s, plan.bytes.ms_T0s, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(v.icp_points, points, plan.fine.bytes.icp_points, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(v.icp_moved, 0, plan.icp.icp_moved, c->stream));      // (a humerus without a winner is walked, never moved, in the fine stage)
  HIPCHK(c, hipMemsetAsync(v.icp_hist, 0, plan.icp.icp_hist, c->stream));
  const dim3 per_b((unsigned)((B + 63) / 64)), wave(64);
  for (int k = 0; k < K; ++k) {
    LAUNCH(c, "k_ms_seed", k_ms_seed, per_b, wave, (const double*)m.ms_T0s, B, K, k, (const sh_registration*)m.ms_coarse, (const int*)m.ms_winner, v.icp_T,
           v.icp_flags, v.icp_out);
    if (int rc = icp_chain(c, v, (const double*)m.ms_points, Qc, per, plan.coarse, coarse)) return rc;
    LAUNCH(c, "k_ms_pick", k_ms_pick, per_b, wave, (const sh_registration*)v.icp_out, B, K, k, min_pairs, m.ms_coarse, m.ms_best, m.ms_winner);
  }
  HIPCHK(c, hipMemsetAsync(v.icp_hist, 0, plan.icp.icp_hist, c->stream));
  LAUNCH(c, "k_ms_seed", k_ms_seed, per_b, wave, (const double*)m.ms_T0s, B, K, -1, (const sh_registration*)m.ms_coarse, (const int*)m.ms_winner, v.icp_T,
         v.icp_flags, v.icp_out);
  if (int rc = icp_chain(c, v, (const double*)v.icp_points, Q, per, plan.fine, fine)) return rc;
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.icp_out, plan.fine.bytes.icp_out, hipMemcpyDeviceToHost, c->stream));
  if (coarse_out) HIPCHK(c, hipMemcpyAsync(coarse_out, m.ms_coarse, plan.bytes.ms_coarse, hipMemcpyDeviceToHost, c->stream));
  if (winner) HIPCHK(c, hipMemcpyAsync(winner, m.ms_winner, plan.bytes.ms_winner, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- mass properties (k_mass.h) ----
int sh_mass_properties(sh_ctx* c, sh_mass* out) {
  if (const ArthroError e = precheck_mass(arthro_facts(c)); e.code) return arthro_refuse(c, "sh_mass_properties", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B;
  const MassPlan plan = mass_plan(B, c->maxF);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const MassView v = view_of<MassView>(c);
  HIPCHK(c, hipMemsetAsync(v.mass_part, 0, plan.bytes.mass_part, c->stream));
  LAUNCH(c, "k_mass_sum", k_mass_sum, dim3((unsigned)plan.blocks, (unsigned)B), dim3(SH_MASS_BLOCK), v.verts, v.faces, v.voff, v.foff, v.mass_part);
  LAUNCH(c, "k_mass_join", k_mass_join, dim3((unsigned)B), dim3(64), v.verts, v.voff, v.foff, (const double*)v.mass_part, plan.blocks, v.mass_out);
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.mass_out, plan.bytes.mass_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- surface samples (k_sample.h) ----
// heads (the seeds, every counter 0) -> scan -> base -> draw -> max_rounds x thin -> finish; the host looks at nothing in between
int sh_sample_surface(sh_ctx* c, int N, const uint64_t* seeds, const sh_sample_options* opt, sh_sample* out, sh_sample_info* info) {
  if (const ArthroError e = precheck_sample(N, seeds, opt, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_sample_surface", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, thin = opt->radius > 0.0 ? 1 : 0;
  const SampPlan plan = samp_plan(B, N, thin != 0, c->maxF, c->sumF);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const SampView v = view_of<SampView>(c);
  std::vector<int32_t> heads((size_t)B * SH_SAMP_HEAD, 0);      // (pageable: the call synchronises before it returns)
  for (int b = 0; b < B; ++b) memcpy(&heads[(size_t)b * SH_SAMP_HEAD + SH_SAMP_SEED_WORD], seeds + b, 8);
  HIPCHK(c, hipMemcpy2DAsync(v.samp_state, (size_t)plan.stride * 4, heads.data(), SH_SAMP_HEAD * 4, SH_SAMP_HEAD * 4, (size_t)B, hipMemcpyHostToDevice, c->stream));
  const dim3 chunks((unsigned)plan.chunks, (unsigned)B), lanes(SH_SAMP_CHUNK);
  LAUNCH(c, "k_samp_scan", k_samp_scan, dim3((unsigned)plan.blocks, (unsigned)B), dim3(SH_SAMPLE_BLOCK), v.verts, v.faces, v.voff, v.foff, v.samp_cdf, v.samp_base);
  LAUNCH(c, "k_samp_base", k_samp_base, dim3((unsigned)B), dim3(256), v.foff, plan.blocks, N, thin, v.samp_base, v.samp_cdf, v.samp_info, v.samp_state, plan.stride);
  LAUNCH(c, "k_samp_draw", k_samp_draw, chunks, lanes, v.verts, v.faces, v.voff, v.foff, (const double*)v.samp_cdf, (const sh_sample_info*)v.samp_info, N, thin,
         v.samp_out, v.samp_state, plan.stride);
  if (thin) {
    const double r2 = opt->radius * opt->radius;
    for (int r = 0; r < opt->max_rounds; ++r)
      LAUNCH(c, "k_samp_thin", k_samp_thin, chunks, lanes, (const sh_sample*)v.samp_out, N, r2, r, v.samp_state, plan.stride);
    LAUNCH(c, "k_samp_finish", k_samp_finish, dim3((unsigned)B), dim3(256), N, (int)opt->max_rounds, (const int*)v.samp_state, plan.stride, v.samp_out, v.samp_info);
  }
  if (out) HIPCHK(c, hipMemcpyAsync(out, v.samp_out, plan.bytes.samp_out, hipMemcpyDeviceToHost, c->stream));
  if (info) HIPCHK(c, hipMemcpyAsync(info, v.samp_info, plan.bytes.samp_info, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- mesh topology (k_topo.h) ----
// zeroed heads and counts, rows of -1 -> count -> scan -> fill -> rows -> adj -> max_rounds x round -> rank -> label -> finish; the host
// looks at nothing in between
int sh_mesh_topology(sh_ctx* c, const sh_topology_options* opt, sh_topology* info, sh_shell* shells) {
  if (const ArthroError e = precheck_topology(opt, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_mesh_topology", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, max_shells = opt->max_shells;
  const TopoPlan plan = topo_plan(B, max_shells, c->maxF, c->sumV, c->sumF);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  c->topo_shell_records = max_shells;
  const TopoView v = view_of<TopoView>(c);
  HIPCHK(c, hipMemsetAsync(v.topo_state, 0, plan.bytes.topo_state, c->stream));
  HIPCHK(c, hipMemsetAsync(v.topo_cursor, 0, plan.bytes.topo_cursor, c->stream));
  HIPCHK(c, hipMemsetAsync(v.topo_vface, 0xff, plan.bytes.topo_vface, c->stream));
  const dim3 blocks((unsigned)plan.blocks, (unsigned)B), lanes(SH_TOPO_BLOCK), meshes((unsigned)B);
  LAUNCH(c, "k_topo_count", k_topo_count, blocks, lanes, v.faces, v.voff, v.foff, v.topo_cursor, v.topo_p, v.topo_state);
  LAUNCH(c, "k_topo_scan", k_topo_scan, meshes, dim3(256), v.voff, v.topo_cursor, v.topo_vrow, v.topo_state);
  LAUNCH(c, "k_topo_fill", k_topo_fill, blocks, lanes, v.faces, v.voff, v.foff, v.topo_cursor, v.topo_tmp);
  LAUNCH(c, "k_topo_rows", k_topo_rows, blocks, lanes, v.faces, v.voff, v.foff, (const int*)v.topo_vrow, (const int*)v.topo_tmp, v.topo_vface);
  LAUNCH(c, "k_topo_adj", k_topo_adj, blocks, lanes, v.faces, v.voff, v.foff, (const int*)v.topo_vrow, (const int*)v.topo_vface, v.topo_adj, v.topo_state);
  for (int r = 0; r < opt->max_rounds; ++r)
    LAUNCH(c, "k_topo_round", k_topo_round, blocks, lanes, v.foff, (const int*)v.topo_adj, v.topo_p, v.topo_state, r);
  LAUNCH(c, "k_topo_rank", k_topo_rank, meshes, dim3(256), v.foff, (const int*)v.topo_adj, (const int*)v.topo_p, v.topo_state, v.topo_tmp, (int*)v.topo_shells,
         max_shells, (int)opt->max_rounds);
  LAUNCH(c, "k_topo_label", k_topo_label, blocks, lanes, v.verts, v.faces, v.voff, v.foff, (const int*)v.topo_adj, (const int*)v.topo_p, (const int*)v.topo_state,
         v.topo_tmp, v.topo_label, (int*)v.topo_shells, max_shells);
  LAUNCH(c, "k_topo_finish", k_topo_finish, meshes, dim3(256), v.foff, (const int*)v.topo_state, (const int*)v.topo_tmp, (int*)v.topo_shells, max_shells, v.topo_info);
  if (info) HIPCHK(c, hipMemcpyAsync(info, v.topo_info, plan.bytes.topo_info, hipMemcpyDeviceToHost, c->stream));
  if (shells) HIPCHK(c, hipMemcpyAsync(shells, v.topo_shells, plan.bytes.topo_shells, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- vertex normals and discrete curvatures (k_vert.h) ----
// a zeroed word per mesh -> face -> gather -> smooth_rounds x smooth -> pack; the host looks at nothing in between
int sh_vertex_fields(sh_ctx* c, int weight, int smooth_rounds, double* normals, double* fields, int32_t* flags, int32_t* status) {
  const bool incidence = c && c->at("topo.vrow") && c->at("topo.vface") && c->at("topo.adj");
  if (const ArthroError e = precheck_vertex_fields(weight, smooth_rounds, incidence, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_vertex_fields", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B;
  const VertPlan plan = vert_plan(B, c->maxV, c->maxF, c->sumV, c->sumF);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const VertView v = view_of<VertView>(c);
  HIPCHK(c, hipMemsetAsync(v.vert_state, 0, plan.bytes.vert_state, c->stream));
  const dim3 fblocks((unsigned)plan.fblocks, (unsigned)B), vblocks((unsigned)plan.vblocks, (unsigned)B), lanes(SH_VERT_BLOCK);
  const long long sumV = c->sumV;
  LAUNCH(c, "k_vert_face", k_vert_face, fblocks, lanes, v.verts, v.faces, v.voff, v.foff, v.vert_face, v.vert_a2, v.vert_state);
  LAUNCH(c, "k_vert_gather", k_vert_gather, vblocks, lanes, v.verts, v.faces, v.voff, v.foff, (const int*)v.topo_vrow, (const int*)v.topo_vface, (const int*)v.topo_adj,
         (const double*)v.vert_face, weight, sumV, v.vert_normal, v.vert_fields, v.vert_flags, v.vert_plane);
  for (int r = 0; r < smooth_rounds; ++r)
    LAUNCH(c, "k_vert_smooth", k_vert_smooth, vblocks, lanes, v.faces, v.voff, v.foff, (const int*)v.topo_vrow, (const int*)v.topo_vface, (const double*)v.vert_a2, sumV, r,
           v.vert_plane);
  LAUNCH(c, "k_vert_pack", k_vert_pack, vblocks, lanes, v.voff, (const double*)v.vert_plane, sumV, smooth_rounds, (const int*)v.vert_state, v.vert_fields, v.vert_status);
  if (normals) HIPCHK(c, hipMemcpyAsync(normals, v.vert_normal, (size_t)sumV * 24, hipMemcpyDeviceToHost, c->stream));
  if (fields) HIPCHK(c, hipMemcpyAsync(fields, v.vert_fields, (size_t)sumV * SH_VERT_FIELDS * 8, hipMemcpyDeviceToHost, c->stream));
  if (flags) HIPCHK(c, hipMemcpyAsync(flags, v.vert_flags, (size_t)sumV * 4, hipMemcpyDeviceToHost, c->stream));
  if (status) HIPCHK(c, hipMemcpyAsync(status, v.vert_status, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- smoothing of the vertices (k_smooth.h) ----
// [count -> scan -> fill, when the rows of this batch are not resident] -> init -> one round per M(.) evaluation -> the volume of P0 and
// of P -> scale -> apply -> info; the host looks at nothing in between.  "smooth.nrow" is what says "the rows of this batch are resident":
// it is the last buffer of its list, so it exists only when every other one does, and a build that did not get through removes it.
static_assert(AR_SMOOTH_BLOCK == SH_SMOOTH_BLOCK, "sh_query.h: smoothing block");

static int smooth_rows(sh_ctx* c, const SmoothPlan& plan, const SmoothView& v) {
  const dim3 vblocks((unsigned)plan.vblocks, (unsigned)c->B), lanes(SH_SMOOTH_BLOCK);
  LAUNCH(c, "k_smooth_count", k_smooth_count, vblocks, lanes, v.faces, v.voff, v.foff, (const int*)v.topo_vrow, (const int*)v.topo_vface, v.smooth_nrow);
  LAUNCH(c, "k_smooth_scan", k_smooth_scan, dim3((unsigned)c->B), lanes, v.voff, v.smooth_nrow);
  LAUNCH(c, "k_smooth_fill", k_smooth_fill, vblocks, lanes, v.verts, v.faces, v.voff, v.foff, (const int*)v.topo_vrow, (const int*)v.topo_vface, (const int*)v.smooth_nrow,
         v.smooth_nbr, v.smooth_w);
  return SH_OK;
}

static int smooth_enqueue(sh_ctx* c, const SmoothPlan& plan, bool rows, int filter, int weight, int iterations, int flags, double p0, double p1, const unsigned char* pin) {
  const SmoothView v = view_of<SmoothView>(c);
  const int B = c->B;
  if (!rows)
    if (int rc = smooth_rows(c, plan, v)) return rc;
  if (pin) HIPCHK(c, hipMemcpyAsync(v.smooth_mask, pin, (size_t)c->sumV, hipMemcpyHostToDevice, c->stream));      // (pageable: staged before the call returns)
  const dim3 fblocks((unsigned)plan.fblocks, (unsigned)B), vblocks((unsigned)plan.vblocks, (unsigned)B), lanes(SH_SMOOTH_BLOCK), meshes((unsigned)B);
  double* pl[3] = {v.smooth_plane, v.smooth_plane + plan.plane, v.smooth_plane + 2 * plan.plane};
  const int *nrow = v.smooth_nrow, *nbr = v.smooth_nbr, *pins = v.smooth_pin;
  const double* w = v.smooth_w;
  LAUNCH(c, "k_smooth_init", k_smooth_init, vblocks, lanes, v.verts, v.faces, v.voff, v.foff, (const int*)v.topo_vrow, (const int*)v.topo_vface, (const int*)v.topo_adj,
         pin ? (const unsigned char*)v.smooth_mask : (const unsigned char*)nullptr, flags & SH_SMOOTH_PIN_BORDER, pl[0], v.smooth_pin);
  for (int it = 0; it < iterations; ++it) {
    if (filter == SH_SMOOTH_HC) {
      LAUNCH(c, "k_smooth_hc_b", k_smooth_round<1>, vblocks, lanes, v.verts, v.voff, v.foff, nrow, nbr, w, pins, weight, p0, (const double*)pl[0], (const double*)nullptr, pl[1], pl[2]);
      LAUNCH(c, "k_smooth_hc_p", k_smooth_round<2>, vblocks, lanes, v.verts, v.voff, v.foff, nrow, nbr, w, pins, weight, p1, (const double*)pl[2], (const double*)pl[1], pl[0],
             (double*)nullptr);
      continue;
    }
    const int per = filter == SH_SMOOTH_TAUBIN ? 2 : 1;
    for (int k = 0; k < per; ++k) {
      const int s = it * per + k;
      LAUNCH(c, "k_smooth_step", k_smooth_round<0>, vblocks, lanes, v.verts, v.voff, v.foff, nrow, nbr, w, pins, weight, k == 0 ? p0 : p1, (const double*)pl[s & 1],
             (const double*)nullptr, pl[(s + 1) & 1], (double*)nullptr);
    }
  }
  const double* fin = pl[plan.last];
  double* part = v.smooth_part;
  LAUNCH(c, "k_smooth_vol", k_smooth_vol<true>, fblocks, lanes, v.verts, v.faces, v.voff, v.foff, (const double*)nullptr, part + plan.vol0);
  LAUNCH(c, "k_smooth_vol", k_smooth_vol<false>, fblocks, lanes, v.verts, v.faces, v.voff, v.foff, fin, part + plan.vol1);
  LAUNCH(c, "k_smooth_scale", k_smooth_scale, meshes, dim3(64), v.verts, v.voff, v.foff, (const double*)(part + plan.vol0), (const double*)(part + plan.vol1), plan.fblocks,
         flags & SH_SMOOTH_KEEP_VOLUME, part + plan.head, v.smooth_info);
  LAUNCH(c, "k_smooth_apply", k_smooth_apply, vblocks, lanes, v.verts, v.voff, fin, (const double*)(part + plan.head), v.smooth_pos, part + plan.disp);
  LAUNCH(c, "k_smooth_info", k_smooth_info, meshes, lanes, v.voff, nrow, pins, (const double*)(part + plan.disp), plan.vblocks, v.smooth_info);
  return SH_OK;
}

int sh_smooth_vertices(sh_ctx* c, int filter, int weight, int iterations, int flags, double p0, double p1, const unsigned char* pin, double* out, void* info) {
  const bool incidence = c && c->at("topo.vrow") && c->at("topo.vface") && c->at("topo.adj");
  if (const ArthroError e = precheck_smooth(filter, weight, iterations, flags, p0, p1, pin != nullptr, incidence, c ? c->maxF : 0, arthro_facts(c)); e.code)
    return arthro_refuse(c, "sh_smooth_vertices", e);
  HIPCHK(c, hipSetDevice(c->device));
  const SmoothPlan plan = smooth_plan(c->B, filter, iterations, c->maxV, c->maxF, c->sumV, c->sumF);
  const bool rows = c->at("smooth.nrow") != nullptr;
  int rc = ensure_bytes(c, plan.bytes);
  if (rc == SH_OK) rc = smooth_enqueue(c, plan, rows, filter, weight, iterations, flags, p0, p1, pin);
  if (rc != SH_OK) {
    if (auto it = c->bufs.find("smooth.nrow"); !rows && it != c->bufs.end()) {
      if (it->second.p) (void)hipFree(it->second.p);
      c->bufs.erase(it);
    }
    return rc;
  }
  if (out) HIPCHK(c, hipMemcpyAsync(out, c->at("smooth.pos"), (size_t)c->sumV * 24, hipMemcpyDeviceToHost, c->stream));
  if (info) HIPCHK(c, hipMemcpyAsync(info, c->at("smooth.info"), (size_t)c->B * SH_SMOOTH_INFO_BYTES, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- repair: one winding, outward shells, filled holes (k_repair.h) ----
// "topo.info" to the host (the one look, before the first launch: it sizes the regions) -> the starts to the device, first = above every
// face, bad = 0, zeroed shell and hole records -> seed -> parity -> shell -> [nest] -> emit -> holes; the host looks at nothing in between
static_assert(AR_REPAIR_BLOCK == SH_REPAIR_BLOCK && AR_REPAIR_HEAD == SH_REPAIR_HEAD && AR_REPAIR_EDGE_ARRAYS == SH_REPAIR_EDGE_ARRAYS, "sh_query.h: repair block, head, border arrays");

int sh_mesh_repair(sh_ctx* c, const sh_repair_options* opt, sh_repair_info* info, sh_repair_shell* shells, sh_repair_hole* holes, unsigned char* flip) {
  const bool topology = c && c->at("topo.adj") && c->at("topo.label") && c->at("topo.vrow") && c->at("topo.vface") && c->at("topo.info") && c->at("topo.shells") && c->topo_shell_records > 0;
  if (const ArthroError e = precheck_repair(opt, topology, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_mesh_repair", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, S = c->topo_shell_records;
  std::vector<sh_topology> tinfo((size_t)B);
  HIPCHK(c, hipMemcpyAsync(tinfo.data(), c->at("topo.info"), (size_t)B * sizeof(sh_topology), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const RepairPlan plan = repair_plan(B, S, opt->max_holes, c->maxV, c->maxF, c->sumF, c->h_voff.data(), c->h_foff.data(), tinfo.data());
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const RepairView v = view_of<RepairView>(c);
  const long long sumF = c->sumF;
  const size_t f = (size_t)(sumF > 0 ? sumF : 1);
  HIPCHK(c, hipMemcpyAsync(v.repair_off, plan.off.data(), plan.bytes.repair_off, hipMemcpyHostToDevice, c->stream));      // (pageable: staged before the call returns)
  HIPCHK(c, hipMemsetAsync(v.repair_work, 0x7f, f * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(v.repair_work + f, 0, f * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(v.repair_shells, 0, plan.bytes.repair_shells, c->stream));
  HIPCHK(c, hipMemsetAsync(v.repair_holes, 0, plan.bytes.repair_holes, c->stream));
  const dim3 blocks((unsigned)plan.blocks, (unsigned)B), lanes(SH_REPAIR_BLOCK), meshes((unsigned)B), per_shell((unsigned)S, (unsigned)B);
  const sh_topology* ti = v.topo_info;
  const sh_shell* ts = v.topo_shells;
  LAUNCH(c, "k_repair_seed", k_repair_seed, blocks, lanes, v.foff, (const int*)v.topo_label, ti, ts, S, sumF, v.repair_work);
  LAUNCH(c, "k_repair_parity", k_repair_parity, meshes, dim3(SH_REPAIR_WALK), v.faces, v.foff, (const int*)v.topo_adj, (const int*)v.topo_label, ti, sumF, (int)opt->orient,
         (int)opt->max_rounds, v.repair_work, v.repair_flip, v.repair_par);
  LAUNCH(c, "k_repair_shell", k_repair_shell, per_shell, lanes, v.verts, v.faces, v.voff, v.foff, (const int*)v.topo_label, ti, ts, S, sumF, (int)opt->orient, v.repair_work,
         v.repair_term, v.repair_flip, v.repair_par, v.repair_shells);
  if (opt->orient == SH_REPAIR_NESTED)
    LAUNCH(c, "k_repair_nest", k_repair_nest, per_shell, lanes, v.verts, v.faces, v.voff, v.foff, (const int*)v.topo_label, ti, ts, S, sumF, v.repair_work,
           (const unsigned char*)v.repair_par, v.repair_flip, v.repair_shells);
  LAUNCH(c, "k_repair_emit", k_repair_emit, blocks, lanes, v.verts, v.faces, v.voff, v.foff, (const unsigned char*)v.repair_flip, (const long long*)v.repair_off, B,
         v.repair_faces, v.repair_verts);
  LAUNCH(c, "k_repair_holes", k_repair_holes, meshes, lanes, v.verts, v.faces, v.voff, v.foff, (const int*)v.topo_adj, (const int*)v.topo_label, (const int*)v.topo_vrow,
         (const int*)v.topo_vface, ti, (const unsigned char*)v.repair_flip, (const long long*)v.repair_off, B, S, sumF, (int)opt->orient, (int)opt->fill, (int)opt->max_hole_edges, (int)opt->max_holes,
         v.repair_work, v.repair_edge, v.repair_faces, v.repair_verts, v.repair_info, v.repair_shells, v.repair_holes);
  if (info) HIPCHK(c, hipMemcpyAsync(info, v.repair_info, plan.bytes.repair_info, hipMemcpyDeviceToHost, c->stream));
  if (shells) HIPCHK(c, hipMemcpyAsync(shells, v.repair_shells, plan.bytes.repair_shells, hipMemcpyDeviceToHost, c->stream));
  if (holes) HIPCHK(c, hipMemcpyAsync(holes, v.repair_holes, plan.bytes.repair_holes, hipMemcpyDeviceToHost, c->stream));
  if (flip) HIPCHK(c, hipMemcpyAsync(flip, v.repair_flip, (size_t)sumF, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- simplification: vertex clustering with quadric placement (k_simplify.h) ----
// the segments, the empty boxes and the cells to the device, zeroed outputs -> box -> key -> sort -> heads -> scan -> ukey -> assign ->
// quadric -> sort -> cluster -> faces -> scan, scan -> emit -> info; the host looks at nothing in between (the temporary storage of the
// sorts is sized on the host)
static_assert(AR_SIMP_BLOCK == SH_SIMP_BLOCK && AR_SIMP_HEAD == SH_SIMP_HEAD && AR_SIMP_Q == SH_SIMP_Q, "sh_query.h: simplification block, head of simp.state, sums of a quadric");

int sh_mesh_simplify(sh_ctx* c, const sh_simplify_options* opt, const double* cell, sh_simplify_info* info, float* verts, int32_t* faces, int32_t* map) {
  const bool incidence = c && c->at("topo.vrow") && c->at("topo.vface");
  if (const ArthroError e = precheck_simplify(opt, cell, incidence, arthro_facts(c)); e.code) return arthro_refuse(c, "sh_mesh_simplify", e);
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B;
  SimplifyPlan plan;
  if (const ArthroError e = simplify_plan(B, c->maxV, c->maxF, c->h_voff.data(), c->sumF, &plan); e.code) return arthro_refuse(c, "sh_mesh_simplify", e);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  SimplifyView v = view_of<SimplifyView>(c);
  const unsigned nkeys = (unsigned)c->sumV;
  size_t tmp_bytes = 0;
  HIPCHK(c, rocprim::segmented_radix_sort_keys(nullptr, tmp_bytes, (const unsigned long long*)v.simp_key, v.simp_sorted, nkeys, (unsigned)B, (const unsigned*)v.simp_seg,
                                               (const unsigned*)v.simp_seg + 1, 0u, 64u, c->stream));
  if (int rc = ensure_shared(c, "simp.tmp", tmp_bytes ? tmp_bytes : 16, 1)) return rc;
  v = view_of<SimplifyView>(c);
  void* tmp = c->at("simp.tmp");
  HIPCHK(c, hipMemcpyAsync(v.simp_seg, plan.seg.data(), plan.bytes.simp_seg, hipMemcpyHostToDevice, c->stream));      // (pageable: staged before the call returns)
  HIPCHK(c, hipMemcpyAsync(v.simp_state, plan.state0.data(), plan.bytes.simp_state, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(v.simp_cell, cell, plan.bytes.simp_cell, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(v.simp_verts, 0, plan.bytes.simp_verts, c->stream));
  HIPCHK(c, hipMemsetAsync(v.simp_faces, 0, plan.bytes.simp_faces, c->stream));
  const dim3 vblocks((unsigned)plan.vblocks, (unsigned)B), fblocks((unsigned)plan.fblocks, (unsigned)B), blocks((unsigned)plan.blocks, (unsigned)B), lanes(SH_SIMP_BLOCK),
      meshes((unsigned)B), scan(SH_SIMP_SCAN);
  const int* vrow = v.topo_vrow;
  const int* vface = v.topo_vface;
  const double* cells = v.simp_cell;
  LAUNCH(c, "k_simp_box", k_simp_box, vblocks, lanes, v.verts, v.voff, vrow, v.simp_state);
  LAUNCH(c, "k_simp_key", k_simp_key, vblocks, lanes, v.verts, v.voff, vrow, cells, v.simp_state, v.simp_key);
  HIPCHK(c, rocprim::segmented_radix_sort_keys(tmp, tmp_bytes, (const unsigned long long*)v.simp_key, v.simp_sorted, nkeys, (unsigned)B, (const unsigned*)v.simp_seg,
                                               (const unsigned*)v.simp_seg + 1, 0u, 64u, c->stream));
  LAUNCH(c, "k_simp_heads", k_simp_heads, vblocks, lanes, (const unsigned long long*)v.simp_sorted, v.voff, v.simp_mark);
  LAUNCH(c, "k_simp_scan", k_simp_scan, meshes, scan, (const int*)v.simp_mark, v.voff, SH_SIMP_W_CLUSTERS, v.simp_rank, v.simp_state);
  LAUNCH(c, "k_simp_ukey", k_simp_ukey, vblocks, lanes, (const unsigned long long*)v.simp_sorted, (const int*)v.simp_mark, (const int*)v.simp_rank, v.voff, v.simp_ukey,
         v.simp_start);
  LAUNCH(c, "k_simp_assign", k_simp_assign, vblocks, lanes, (const unsigned long long*)v.simp_ukey, v.voff, (const unsigned*)v.simp_state, v.simp_cid, v.simp_key);
  LAUNCH(c, "k_simp_quadric", k_simp_quadric, vblocks, lanes, v.verts, v.faces, v.voff, v.foff, vrow, vface, cells, (const unsigned*)v.simp_state, (const int*)v.simp_cid,
         v.simp_quad);
  HIPCHK(c, rocprim::segmented_radix_sort_keys(tmp, tmp_bytes, (const unsigned long long*)v.simp_key, v.simp_sorted, nkeys, (unsigned)B, (const unsigned*)v.simp_seg,
                                               (const unsigned*)v.simp_seg + 1, 0u, 64u, c->stream));
  LAUNCH(c, "k_simp_cluster", k_simp_cluster, vblocks, lanes, v.verts, v.voff, cells, v.simp_state, (const unsigned long long*)v.simp_sorted,
         (const unsigned long long*)v.simp_ukey, (const int*)v.simp_start, (const double*)v.simp_quad, (int)opt->place, opt->reg, opt->clamp, v.simp_pos);
  HIPCHK(c, hipMemsetAsync(v.simp_mark, 0, plan.bytes.simp_mark, c->stream));      // (the heads are spent: the marks of the named clusters)
  LAUNCH(c, "k_simp_faces", k_simp_faces, fblocks, lanes, v.faces, v.voff, v.foff, vrow, vface, v.simp_state, (const int*)v.simp_cid, (const unsigned long long*)v.simp_sorted,
         (const int*)v.simp_start, v.simp_keep, v.simp_mark);
  LAUNCH(c, "k_simp_scan", k_simp_scan, meshes, scan, (const int*)v.simp_keep, v.foff, SH_SIMP_W_FACES, v.simp_frank, v.simp_state);
  LAUNCH(c, "k_simp_scan", k_simp_scan, meshes, scan, (const int*)v.simp_mark, v.voff, SH_SIMP_W_VERTS, v.simp_rank, v.simp_state);
  LAUNCH(c, "k_simp_emit", k_simp_emit, blocks, lanes, v.verts, v.faces, v.voff, v.foff, v.simp_state, (const int*)v.simp_cid, (const float*)v.simp_pos, (const int*)v.simp_keep,
         (const int*)v.simp_frank, (const int*)v.simp_mark, (const int*)v.simp_rank, v.simp_verts, v.simp_faces, v.simp_map);
  LAUNCH(c, "k_simp_info", k_simp_info, dim3((unsigned)((B + SH_SIMP_BLOCK - 1) / SH_SIMP_BLOCK)), lanes, (const unsigned*)v.simp_state, cells, B, v.simp_info);
  if (info) HIPCHK(c, hipMemcpyAsync(info, v.simp_info, plan.bytes.simp_info, hipMemcpyDeviceToHost, c->stream));
  if (verts) HIPCHK(c, hipMemcpyAsync(verts, v.simp_verts, (size_t)c->sumV * 12, hipMemcpyDeviceToHost, c->stream));
  if (faces) HIPCHK(c, hipMemcpyAsync(faces, v.simp_faces, (size_t)c->sumF * 12, hipMemcpyDeviceToHost, c->stream));
  if (map) HIPCHK(c, hipMemcpyAsync(map, v.simp_map, (size_t)c->sumV * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

// ---- geodesic distances and shortest paths (k_geo.h) ----
// the lists to the device -> face -> init -> seed -> lds (the pairs whose plane fits one workgroup's LDS) -> for a larger mesh chunks of
// SH_GEO_CHUNK rounds, the host reading ONE word of "geo.state" after each (the only look: the number of rounds is not known beforehand)
// -> root -> pred -> jumps x jump -> info.  lds_vertices: SH_GEO_LDS_VERTICES, or less from the lab entry point below.
static_assert(AR_GEO_BLOCK == SH_GEO_BLOCK && AR_GEO_FACE == SH_GEOD_FACE && AR_GEO_STATE == SH_GEO_STATE, "sh_query.h: geodesic block, doubles of a face record, words of a pair");

static int geodesic_run(sh_ctx* c, const char* fn, int lds_vertices, int mode, int K, double max_dist, const int32_t* src_off, const int32_t* src, const double* d0,
                        double* dist, int32_t* pred, int32_t* source, void* info) {
  const bool incidence = c && c->at("topo.vrow") && c->at("topo.vface") && c->at("topo.adj");
  const bool lists = c && c->B >= 1 && (int)c->h_voff.size() == c->B + 1;
  if (const ArthroError e = precheck_geodesic(mode, K, max_dist, src_off, src, d0, lists ? c->h_voff.data() : nullptr, incidence, arthro_facts(c)); e.code)
    return arthro_refuse(c, fn, e);
  if (lds_vertices < 0 || lds_vertices > SH_GEO_LDS_VERTICES) return fail(c, SH_ERR_ARG, std::string(fn) + ": bad argument (lds_vertices in 0..SH_GEO_LDS_VERTICES)");
  HIPCHK(c, hipSetDevice(c->device));
  const int B = c->B, pairs = B * K;
  const long long S = src_off[pairs], sumV = c->sumV;
  const GeoPlan plan = geo_plan(B, K, S, lds_vertices, c->maxV, c->maxF, sumV, c->sumF);
  if (int rc = ensure_bytes(c, plan.bytes)) return rc;
  const GeoView v = view_of<GeoView>(c);
  HIPCHK(c, hipMemcpyAsync(v.geo_src, src_off, (size_t)(pairs + 1) * 4, hipMemcpyHostToDevice, c->stream));
  if (S > 0) {
    HIPCHK(c, hipMemcpyAsync(v.geo_src + pairs + 1, src, (size_t)S * 4, hipMemcpyHostToDevice, c->stream));
    if (d0) HIPCHK(c, hipMemcpyAsync(v.geo_d0, d0, (size_t)S * 8, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(v.geo_d0, 0, (size_t)S * 8, c->stream));
  }
  HIPCHK(c, hipMemsetAsync(v.geo_state, 0, plan.bytes.geo_state, c->stream));
  const dim3 fblocks((unsigned)plan.fblocks, (unsigned)B), vblocks((unsigned)plan.vblocks, (unsigned)K, (unsigned)B), lanes(SH_GEO_BLOCK), each((unsigned)pairs);
  const int *d_off = v.geo_src, *d_src = v.geo_src + pairs + 1;
  const int *vrow = v.topo_vrow, *vface = v.topo_vface, *opp = v.geo_opp;
  const double* frec = v.geo_face;
  LAUNCH(c, "k_geo_face", k_geo_face, fblocks, lanes, v.verts, v.faces, v.voff, v.foff, (const int*)v.topo_adj, v.geo_face, v.geo_opp);
  LAUNCH(c, "k_geo_init", k_geo_init, vblocks, lanes, v.voff, K, lds_vertices, v.geo_dist, v.geo_source, v.geo_state);
  LAUNCH(c, "k_geo_seed", k_geo_seed, each, lanes, v.voff, K, d_off, d_src, (const double*)v.geo_d0, max_dist, v.geo_dist);
  if (lds_vertices > 0)
    LAUNCH(c, "k_geo_lds", k_geo_lds, dim3((unsigned)K, (unsigned)B), dim3(SH_GEO_LDS_BLOCK), v.faces, v.voff, v.foff, vrow, vface, frec, opp, K, mode, max_dist, lds_vertices,
           v.geo_dist, v.geo_state);
  if (plan.general) {
    const int* call = v.geo_state + (size_t)pairs * SH_GEO_STATE;
    long long r = 0;
    for (int more = 1; more;) {
      if (r >= plan.rounds_max) return fail(c, SH_ERR_INTERNAL, std::string(fn) + ": the relaxation did not settle within max V_b + 1 rounds");
      for (int i = 0; i < SH_GEO_CHUNK && r < plan.rounds_max; ++i, ++r)
        LAUNCH(c, "k_geo_round", k_geo_round, vblocks, lanes, v.faces, v.voff, v.foff, vrow, vface, frec, opp, K, mode, max_dist, lds_vertices, (int)r, v.geo_dist, v.geo_plane,
               v.geo_state);
      HIPCHK(c, hipMemcpyAsync(&more, call + r % 3, 4, hipMemcpyDeviceToHost, c->stream));      // round r - 1 changed something
      HIPCHK(c, hipStreamSynchronize(c->stream));
    }
  }
  LAUNCH(c, "k_geo_root", k_geo_root, each, lanes, v.voff, K, d_off, d_src, (const double*)v.geo_d0, (const double*)v.geo_dist, v.geo_source);
  LAUNCH(c, "k_geo_pred", k_geo_pred, vblocks, lanes, v.faces, v.voff, v.foff, vrow, vface, frec, opp, K, mode, (const double*)v.geo_dist, v.geo_pred, v.geo_source, v.geo_jump);
  for (int j = 0; j < plan.jumps; ++j) LAUNCH(c, "k_geo_jump", k_geo_jump, vblocks, lanes, v.voff, K, v.geo_jump);
  LAUNCH(c, "k_geo_info", k_geo_info, dim3((unsigned)K, (unsigned)B), lanes, v.voff, K, (const double*)v.geo_dist, (const int*)v.geo_pred, (const int*)v.geo_jump,
         (const int*)v.geo_state, v.geo_source, v.geo_info);
  const size_t n = (size_t)sumV * (size_t)K;
  if (dist) HIPCHK(c, hipMemcpyAsync(dist, v.geo_dist, n * 8, hipMemcpyDeviceToHost, c->stream));
  if (pred) HIPCHK(c, hipMemcpyAsync(pred, v.geo_pred, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (source) HIPCHK(c, hipMemcpyAsync(source, v.geo_source, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (info) HIPCHK(c, hipMemcpyAsync(info, v.geo_info, (size_t)pairs * SH_GEO_INFO_BYTES, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SH_OK;
}

int sh_geodesic(sh_ctx* c, int mode, int K, double max_dist, const int32_t* src_off, const int32_t* src, const double* d0, double* dist, int32_t* pred, int32_t* source,
                void* info) {
  return geodesic_run(c, "sh_geodesic", SH_GEO_LDS_VERTICES, mode, K, max_dist, src_off, src, d0, dist, pred, source, info);
}

// Lab entry point (not in the header; tools/time_geodesic.py and the tests of the general path): sh_geodesic with the threshold between
// the two paths lowered to lds_vertices in 0..SH_GEO_LDS_VERTICES, so that a small mesh takes the general path.  The result is the same bytes.
extern "C" int sh_lab_geodesic(sh_ctx* c, int lds_vertices, int mode, int K, double max_dist, const int32_t* src_off, const int32_t* src, const double* d0, double* dist,
                               int32_t* pred, int32_t* source, void* info) {
  return geodesic_run(c, "sh_lab_geodesic", lds_vertices, mode, K, max_dist, src_off, src, d0, dist, pred, source, info);
}
