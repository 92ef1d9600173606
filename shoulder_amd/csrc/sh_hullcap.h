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
#define SH_ENDCAP 8192      // crossing points of an end section (mesh.py:91-107) a context starts with; ~330 at the fixture resolution, ~1 300 on a 519 k-triangle mesh.
                            // A run that meets more records how many (overflow counter word 7) and sh_collect grows the buffer and runs the batch again

}  // namespace sh
