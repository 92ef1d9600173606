// sh_hullcap.h -- capacities of the hull record, shared by the OBB / hull kernels (k_obb.h, k_hull.h) and the context (sh_ctx.h)
#pragma once

namespace sh {

// hull record capacities (HBM): vertices / faces / edges per humerus.  The fixtures' hulls have 1 368 / 2 732 / 4 098; the hull of
// a 519 k-triangle humerus 4 209 / 8 414 / 12 621; a convex region sampled more densely keeps more of its vertices on the hull.
// These are the capacities a context STARTS with; a batch with a larger hull grows the record (sh_ctx::hcap) and every kernel
// takes the per-humerus strides as an argument.
#define SH_HV 16384
#define SH_HF 32768
#define SH_HE 49152
struct HullCap { int v, f, e; };      // per-humerus strides of hull.hv / hull.normals (+ the per-face obb.* arrays) / hull.edges
// What the kernels of the OBB stage (k_obb.h) and the device hull (k_hull.h) share with the host's launch plan (sh_obb_plan.h)
#define SH_OBB_THREADS 256
#define SH_OBB_TILE 16           // hull faces (candidate directions) per workgroup
#define SH_OBB_TILE_LARGE 8      // ... of the large and the workspace tier of k_obb_candidates (one face per scan)
#define SH_OBB_GROUP 4           // faces whose rectangle scans run together (2 would fit three workgroups per CU: measured slower)
#define SH_OBB_BND_SPLIT 4       // waves of a k_obb_bounds workgroup
#define SH_OBB_BND_DIRS 128      // directions per k_obb_bounds workgroup
#define SH_OBB_BND_THREADS (64 * SH_OBB_BND_SPLIT)
// the LDS tiers of k_obb_candidates: silhouette edges per direction / hull faces the small and the large one hold (above: the workspace tier)
#define SH_OBB_SIL_SMALL 512
#define SH_OBB_NF_SMALL 8192
#define SH_OBB_SIL_LARGE 2048
#define SH_OBB_NF_LARGE 32768
#define HD_SLOTS 3072            // face slots of the device hull (alive + not yet reused); a humerus ends with ~2 700 faces
#define SH_ENDCAP 8192      // crossing points of an end section (mesh.py:91-107) a context starts with; ~330 at the fixture resolution, ~1 300 on a 519 k-triangle mesh.
                            // A run that meets more records how many (overflow counter word 7) and sh_collect grows the buffer and runs the batch again

}  // namespace sh
