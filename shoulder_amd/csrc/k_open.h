// k_open.h -- sections of meshes that are not watertight (sh_set_open_contours; DESIGN.md section 3, "Open contours").
//
// The reference warns about such a mesh (humerus/mesh.py:24-27) and resamples `slice.discrete[0]` even when that path is
// open (slice.py:65-80).  This library keeps its default -- an open chain in a section is SH_ERR_GEOMETRY for the humerus --
// and offers one opt-in rule, SH_OPEN_BRIDGE, that closes gaps up to `max_gap` mm:
//   chains   in the successor graph of a plane's crossing segments, a head has no predecessor and a tail no successor;
//   bridges  a (tail t, head h) pair is a candidate if |end(t) - start(h)| <= max_gap (box-frame xy, seg_start_point's
//            crossing formula); the candidate with the smallest (gap, end key of t, start key of h) is bridged first, t and h
//            leave the candidates, and so on.  A bridge is a virtual segment whose start key is t's end key and whose successor
//            is h: it adds one ring vertex, the crossing on t's end edge;
//   loops    the cycles of at least three vertices of the graph with its bridges; every other segment is dropped.
// A single missing triangle leaves a chain whose tail ends on one of the triangle's two cut edges and whose head starts on the
// other: the bridge is the missing triangle's segment, and the ring is the intact mesh's, point for point.
#pragma once
#include "k_slices.h"      // (the rule itself: bridge_open_chains, used by the joins of k_slices.h and k_ovf.h)

namespace sh {

// ---- open-edge count (sh_mesh_open_edges; mesh.py:24 `mesh.is_watertight`) ---------------------------------------------------
// Per mesh an open-addressing table of its undirected edges (keys min vid << 32 | max vid, all ones = empty) with a use count;
// the edges used by a number of faces other than two are counted.  Table of mesh b: [toff[b], toff[b + 1]), a power of two >= 4 F_b.
__global__ void __launch_bounds__(256)
k_edge_insert(const int* __restrict__ faces, const long long* __restrict__ foff, const long long* __restrict__ toff,
              unsigned long long* __restrict__ keys, int* __restrict__ uses) {
  const int b = blockIdx.y;
  const long long f0 = foff[b], nf = foff[b + 1] - f0, t0 = toff[b];
  const unsigned long long mask = (unsigned long long)(toff[b + 1] - t0) - 1ull;
  for (long long fi = blockIdx.x * (long long)blockDim.x + threadIdx.x; fi < nf; fi += (long long)gridDim.x * blockDim.x) {
    const int* f = faces + 3 * (f0 + fi);
    for (int e = 0; e < 3; ++e) {
      const uint32_t a = (uint32_t)f[e], c = (uint32_t)f[(e + 1) % 3];
      const unsigned long long k = a < c ? ((unsigned long long)a << 32) | c : ((unsigned long long)c << 32) | a;
      unsigned long long h = hash_key64(k) & mask;
      for (unsigned long long probe = 0; probe <= mask; ++probe) {      // (>= 4 F slots for <= 3 F distinct edges: a free slot always exists)
        const unsigned long long prev = atomicCAS(&keys[t0 + h], ~0ull, k);
        if (prev == ~0ull || prev == k) { atomicAdd(&uses[t0 + h], 1); break; }
        h = (h + 1) & mask;
      }
    }
  }
}
__global__ void __launch_bounds__(256)
k_edge_count_open(const long long* __restrict__ toff, const unsigned long long* __restrict__ keys, const int* __restrict__ uses,
                  unsigned long long* __restrict__ out /*[B]*/) {
  const int b = blockIdx.y;
  const long long t0 = toff[b], nt = toff[b + 1] - t0;
  unsigned long long cnt = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < nt; i += (long long)gridDim.x * blockDim.x)
    if (keys[t0 + i] != ~0ull && uses[t0 + i] != 2) ++cnt;
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&out[b], cnt);
}

}  // namespace sh
