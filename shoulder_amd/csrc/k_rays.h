// k_rays.h -- rays against the resident batch, every hit, ordered (include/shoulder_hip.h sh_ray_cast / sh_anp_axis_hits).  The
// reference asks `ray.intersects_location` (anatomic_neck.py:184-192, 217-224), which returns every hit; k_rays_hit (k_anp.h) keeps
// the nearest one and k_canal_rays (k_stem.h) the nearest and the farthest.  Brute force over the faces, count -> scan -> fill -> sort:
//   k_ray_count     (tile of 256 faces, humerus, chunk of SH_RAY_CHUNK rays) workgroups, one face per lane as k_resect_faces: the
//                   face is fetched once and kept as (A, e1, e2) in registers; the rays of the chunk are read one after another
//                   at an address that is the same in every lane.  The full test is sh_scalar.h ray_tri_hit (canal_ray_hit's
//                   statement, which restates k_rays_hit).  Hits are sparse: per ray and wave one ballot and a popcount, then at
//                   most one integer atomicAdd on counts[b][r].  A workgroup that saw a hit sets its word of "ray.blockhit".
//   k_ray_scan      one workgroup: the exclusive scan of the B x R counts in 64 bits, offs[B R] is the total (the host reads these
//                   8 bytes once and sizes "ray.pool", the count-then-fill habit of sh_slice_mesh_planes).
//   k_ray_fill      the same walk and the same statement, so the same verdicts -- by the workgroups whose word is set: the others
//                   counted nothing and leave at once (hits are sparse: most of them); a wave takes its slots of the ray's segment with
//                   one integer atomicAdd on the ray's cursor and writes {t, face, side}.  Every write is guarded with
//                   slot < end of the segment: a disagreement between the passes could lose a hit, never write outside the pool.
//   k_ray_sort      one wave per (humerus, ray): a rank sort of the segment on the key (t, face) (sh_scalar.h ray_key_less; total,
//                   a face is hit once) -- a lane counts the keys below its own, for any segment length; the ranks below cap are
//                   stored with their points, the slots behind them are zero with face = -1.
// The integer atomics only choose slots and the sort removes their order; no floating-point atomics, no floating-point sums across
// lanes: a (humerus, ray) result depends on that mesh and that ray alone.
// Two vertex loaders, one body (BOX): the float32 CT vertex widened (sh_ray_cast), or that vertex under "obb_transform" by the
// expression k_transform_verts fills "verts_obb" with (sh_anp_axis_hits: "verts_obb" itself is shared scratch that a later call may
// have rewritten, the transform and the vertices are the batch's).  With BOX the points go to CT as k_tail's pack_one maps the
// record's axis rows: xform_pt of the inverse of the box transform.
#pragma once
#include "k_anp.h"
#include "k_resect.h"

namespace sh {

#define SH_RAY_TILE SH_RS_TILE
#define SH_RAY_CHUNK 256      // rays per workgroup (grid.z chunks)

struct __attribute__((aligned(16))) RayKey { double t; int face, side; };      // one hit in "ray.pool"
static_assert(sizeof(RayKey) == 16, "RayKey must be 16 bytes");
static_assert(sizeof(sh_ray) == 48 && sizeof(sh_ray_hit) == 40, "sh_ray is six doubles, sh_ray_hit four doubles and two int32");

// the four rays of SH_STAGE_ANP per humerus from "anp.plane" (box frame) and the status of its record
__global__ void k_ray_anp_rays(const sh_landmarks* __restrict__ lm, const double* __restrict__ plane /* B x 6 */, int B,
                               double* __restrict__ rays /* B x 4 x 6 */, int* __restrict__ hstatus /* B */) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* pl = plane + 6 * (size_t)b;
  int st = lm[b].status;
  double d[4][3];
  bool ok = true;
  for (int k = 0; k < 6; ++k) ok = ok && isfinite(pl[k]);
  for (int ray = 0; ray < 4; ++ray) {
    ray_dir(pl, ray, d[ray]);
    ok = ok && isfinite(d[ray][0]) && isfinite(d[ray][1]) && isfinite(d[ray][2]) && (d[ray][0] != 0.0 || d[ray][1] != 0.0 || d[ray][2] != 0.0);
  }
  if (st == 0 && !ok) st = SH_ERR_GEOMETRY_DEV;
  for (int ray = 0; ray < 4; ++ray) {
    double* o = rays + ((size_t)b * 4 + ray) * 6;
    for (int k = 0; k < 3; ++k) { o[k] = st == 0 ? pl[k] : 0.0; o[3 + k] = st == 0 ? d[ray][k] : 0.0; }
  }
  hstatus[b] = st;
}

// the walk of both passes: FILL = false counts, FILL = true writes the pool
template <bool BOX, bool FILL>
__device__ __forceinline__ void ray_walk(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff,
                                         const long long* __restrict__ foff, const double* __restrict__ T_obb /* B x 16 (BOX) */,
                                         const int* __restrict__ hstatus /* B or null */, const double* __restrict__ rays, int R, int per_humerus,
                                         int* __restrict__ counts /* B x R */, const unsigned long long* __restrict__ offs /* B x R + 1 */,
                                         int* __restrict__ cursor /* B x R */, RayKey* __restrict__ pool, int* __restrict__ blockhit /* one per workgroup */) {
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  if (hstatus && hstatus[b] != 0) return;      // (uniform) a humerus without rays keeps its zero counts
  const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (FILL && blockhit[wg] == 0) return;       // (uniform) the count pass found nothing here
  bool live; long long fi; double V[9];
  if (!resect_tile_face(verts, faces, voff, foff, b, (int)blockIdx.x, tid, &live, &fi, V)) return;      // (uniform)
  if (BOX) {
    const double* T = T_obb + 16 * (size_t)b;
#pragma unroll
    for (int j = 0; j < 3; ++j) { double q[3]; xform_pt(T, V[3 * j], V[3 * j + 1], V[3 * j + 2], q); V[3 * j] = q[0]; V[3 * j + 1] = q[1]; V[3 * j + 2] = q[2]; }
  }
  const double A[3] = {V[0], V[1], V[2]};
  const double e1[3] = {V[3] - V[0], V[4] - V[1], V[5] - V[2]};
  const double e2[3] = {V[6] - V[0], V[7] - V[1], V[8] - V[2]};
  const int r0 = (int)blockIdx.z * SH_RAY_CHUNK, r1 = min(R, r0 + SH_RAY_CHUNK);
  const double* rb = rays + (per_humerus ? 6 * (size_t)b * R : (size_t)0);
  bool any = false;
  for (int r = r0; r < r1; ++r) {
    const double* rg = rb + 6 * (size_t)r;      // (the same address in every lane)
    const double o[3] = {rg[0], rg[1], rg[2]}, d[3] = {rg[3], rg[4], rg[5]};
    double t = 0.0;
    int side = 0;
    const bool hit = live && ray_tri_hit(o, d, A, e1, e2, &t, &side);
    const unsigned long long m = __ballot(hit);
    if (m == 0ull) continue;      // (uniform in the wave)
    any = true;
    const size_t i = (size_t)b * R + r;
    const int n = __popcll(m);
    if (!FILL) {
      if (lane == 0) atomicAdd(&counts[i], n);
    } else {
      int base = 0;
      if (lane == 0) base = atomicAdd(&cursor[i], n);
      base = __shfl(base, 0);
      if (hit) {
        const unsigned long long slot = offs[i] + (unsigned long long)(unsigned)(base + __popcll(m & ((1ull << lane) - 1ull)));
        if (slot < offs[i + 1]) { RayKey k; k.t = t; k.face = (int)fi; k.side = side; pool[slot] = k; }
      }
    }
  }
  if (!FILL && any && lane == 0) blockhit[wg] = 1;      // (up to four waves store the same word)
}

template <bool BOX>
__global__ void __launch_bounds__(SH_RAY_TILE)
k_ray_count(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
            const double* __restrict__ T_obb, const int* __restrict__ hstatus, const double* __restrict__ rays, int R, int per_humerus,
            int* __restrict__ counts, int* __restrict__ blockhit) {
  ray_walk<BOX, false>(verts, faces, voff, foff, T_obb, hstatus, rays, R, per_humerus, counts, nullptr, nullptr, nullptr, blockhit);
}

template <bool BOX>
__global__ void __launch_bounds__(SH_RAY_TILE)
k_ray_fill(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
           const double* __restrict__ T_obb, const int* __restrict__ hstatus, const double* __restrict__ rays, int R, int per_humerus,
           const unsigned long long* __restrict__ offs, int* __restrict__ cursor, RayKey* __restrict__ pool, int* __restrict__ blockhit) {
  ray_walk<BOX, true>(verts, faces, voff, foff, T_obb, hstatus, rays, R, per_humerus, nullptr, offs, cursor, pool, blockhit);
}

// exclusive scan of n counts into offs[0 .. n], offs[n] the total; integers, one workgroup of sixteen waves
__global__ void __launch_bounds__(1024)
k_ray_scan(const int* __restrict__ counts, long long n, unsigned long long* __restrict__ offs /* n + 1 */) {
  __shared__ unsigned long long s_wave[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long carry = 0ull;
  for (long long base = 0; base < n; base += 1024) {
    const long long i = base + tid;
    const unsigned long long v = i < n ? (unsigned long long)(unsigned)counts[i] : 0ull;
    unsigned long long incl = v;
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned long long pre = 0ull, tot = 0ull;
    for (int w = 0; w < 16; ++w) { const unsigned long long s = s_wave[w]; if (w < wave) pre += s; tot += s; }
    if (i < n) offs[i] = (carry + pre) + (incl - v);
    carry += tot;
    __syncthreads();
  }
  if (tid == 0) offs[n] = carry;
}

template <bool BOX>
__global__ void __launch_bounds__(64)
k_ray_sort(const double* __restrict__ rays, int R, int per_humerus, const unsigned long long* __restrict__ offs /* B x R + 1 */,
           const int* __restrict__ cursor /* B x R */, const RayKey* __restrict__ pool, const double* __restrict__ T_obb /* B x 16 (BOX) */, int cap,
           sh_ray_hit* __restrict__ hits /* B x R x cap */) {
  const size_t i = blockIdx.x;
  const int b = (int)(i / (size_t)R), r = (int)(i - (size_t)b * R), lane = threadIdx.x;
  const unsigned long long base = offs[i], room = offs[i + 1] - base;
  const unsigned long long wrote = (unsigned long long)(unsigned)cursor[i];
  const int n = (int)(wrote < room ? wrote : room);      // what the fill stored: the ray's count
  const RayKey* seg = pool + base;
  const double* rg = rays + 6 * ((per_humerus ? (size_t)b * R : (size_t)0) + r);
  const double o[3] = {rg[0], rg[1], rg[2]}, d[3] = {rg[3], rg[4], rg[5]};
  double Ti[16];
  if (BOX) inv_transform(T_obb + 16 * (size_t)b, Ti);
  sh_ray_hit* out = hits + i * (size_t)cap;
  for (int j = lane; j < n; j += 64) {
    const RayKey kj = seg[j];
    int rank = 0;
    for (int k = 0; k < n; ++k) { const RayKey kk = seg[k]; rank += ray_key_less(kk.t, kk.face, kj.t, kj.face) ? 1 : 0; }
    if (rank >= cap) continue;
    sh_ray_hit* h = out + rank;
    double p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = o[k] + d[k] * kj.t;
    if (BOX) { double q[3]; xform_pt(Ti, p[0], p[1], p[2], q); p[0] = q[0]; p[1] = q[1]; p[2] = q[2]; }
    h->t = kj.t; h->point[0] = p[0]; h->point[1] = p[1]; h->point[2] = p[2]; h->face = kj.face; h->side = kj.side;
  }
  for (int s = (n < cap ? n : cap) + lane; s < cap; s += 64) {      // zero with face = -1
    long long* w = (long long*)(out + s);
    w[0] = 0; w[1] = 0; w[2] = 0; w[3] = 0; w[4] = 0x00000000ffffffffll;
  }
}

}  // namespace sh
