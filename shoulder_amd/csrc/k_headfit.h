// k_headfit.h -- head sizing of the cuts of a batched resection (include/shoulder_hip.h sh_head_fit): the sphere of the resected
// head piece and the ellipse of the cut, per (humerus, plane).  The reference stops in front of this step (arthroplasty.py:178-182,
// a commented-out `HumeralImplantation`); its RadiusCurvature (bone_props.py:114-148) fits the native head only.
//   k_headfit_faces   sibling of k_resect_faces (same tile / plane loop): one workgroup per (humerus, tile of SH_RS_TILE faces), the
//                     faces loaded once into float64 registers, then the humerus' planes (wave-uniform loads).  Per plane every lane
//                     adds the fourteen moment terms of its face's kept triangles (k_resect_faces' re-triangulation); a wave with no
//                     kept face (ballot) skips the arithmetic and the reduction and stores zeros.  The sixteen words (two pads) are
//                     reduced in the wave by a transposing butterfly -- at step 32 a lane keeps eight words and hands the other
//                     eight to its partner, at 16 four, at 8 two, at 4 one, then two plain steps: 17 double shuffles instead of
//                     14 x 6 -- a fixed tree; the four waves are added in order and the slab entry of (humerus, plane, tile) is
//                     STORED.  No floating-point atomics.
//   k_resect_join_fit (k_resect.h) adds a cut's slab in tile order and the largest loop's second-moment shoelace sums in ring order.
//   k_headfit_solve   one lane per cut (of the batch, or of one pass when k_seat.h follows pass by pass): sh_scalar.h
//                     head_sphere_from_moments / ellipse_from_moments (the source the host check instantiates), cap height, the
//                     centre in the humerus' canal / articular frame, the record.
#pragma once
#include "k_resect.h"
#include "sh_scalar.h"

namespace sh {

#define SH_HF_WORDS 16      // moment words per slab entry: S0, S1 (3), S2 (6), S3 (3), S4, two pads

// the fourteen terms of the three corners of triangle (a, b, c), weight (area / 3) each, coordinates about o
__device__ inline void headfit_tri(const double* a, const double* b, const double* c, const double* o, double* m) {
  const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
  const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  const double w = (0.5 * sqrt((nx * nx + ny * ny) + nz * nz)) / 3.0;
  const double* pt[3] = {a, b, c};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double qx = pt[j][0] - o[0], qy = pt[j][1] - o[1], qz = pt[j][2] - o[2];
    const double wx = w * qx, wy = w * qy, wz = w * qz;
    const double r2 = (qx * qx + qy * qy) + qz * qz, wr2 = w * r2;
    m[0] += w; m[1] += wx; m[2] += wy; m[3] += wz;
    m[4] += wx * qx; m[5] += wx * qy; m[6] += wx * qz; m[7] += wy * qy; m[8] += wy * qz; m[9] += wz * qz;
    m[10] += wr2 * qx; m[11] += wr2 * qy; m[12] += wr2 * qz; m[13] += wr2 * r2;
  }
}

// sum over the wave of sixteen words per lane; afterwards every lane holds the total of word headfit_word(lane) (four lanes each)
__device__ inline double headfit_wave_reduce(double* v, int lane) {
#pragma unroll
  for (int half = 8, off = 32; half >= 1; half >>= 1, off >>= 1) {
    const bool up = (lane & off) != 0;
#pragma unroll
    for (int k = 0; k < half; ++k) {
      const double keep = up ? v[k + half] : v[k], give = up ? v[k] : v[k + half];
      v[k] = keep + __shfl_xor(give, off);
    }
  }
  v[0] += __shfl_xor(v[0], 2);
  v[0] += __shfl_xor(v[0], 1);
  return v[0];
}
__device__ inline int headfit_word(int lane) { return ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1); }

__global__ void __launch_bounds__(SH_RS_TILE)
k_headfit_faces(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
                const double* __restrict__ planes /* B x P x 6 */, int P, int p0, int pc /* planes p0 .. p0 + pc of this pass */,
                int b0 /* first humerus of the grid */, int tstride /* tiles per humerus in the slab */,
                double* __restrict__ fslab /* [grid.y][pc][tstride][SH_HF_WORDS] */) {
  __shared__ double s_red[2][SH_RS_TILE / 64][SH_HF_WORDS];
  const int bi = blockIdx.y, b = b0 + bi, t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bool live; long long fi; double V[9];
  if (!resect_tile_face(verts, faces, voff, foff, b, t, tid, &live, &fi, V)) return;      // (uniform)
  const int word = headfit_word(lane);
  for (int q = 0; q < pc; ++q) {
    const double* plg = planes + ((size_t)b * P + (p0 + q)) * 6;
    const double pl[6] = {plg[0], plg[1], plg[2], plg[3], plg[4], plg[5]};      // (the same address in every lane)
    int s[3]; double d[3];
    const int k = live ? resect_class(V, pl, s, d) : 0;
    const int bf = q & 1;
    if (__ballot(k != 0) == 0ull) {      // (wave-uniform) nothing of this wave's faces on the normal's side: + 0.0 in the fixed-order sum
      if (lane < SH_HF_WORDS) s_red[bf][wave][lane] = 0.0;
    } else {
      double m[SH_HF_WORDS];
#pragma unroll
      for (int i = 0; i < SH_HF_WORDS; ++i) m[i] = 0.0;
      if (k == 1) headfit_tri(V, V + 3, V + 6, pl, m);
      else if (k == 2) {      // one vertex cut away: the quad's two triangles (a, b, n0), (n0, n1, a)
        const int qi = s[0] == 1 ? 0 : (s[1] == 1 ? 1 : 2);
        double n0[3], n1[3];
        clip_cross(V, (qi + 2) % 3, pl, n0);
        clip_cross(V, qi, pl, n1);
        const double* a = V + 3 * ((qi + 1) % 3); const double* bb = V + 3 * ((qi + 2) % 3);
        headfit_tri(a, bb, n0, pl, m);
        headfit_tri(n0, n1, a, pl, m);
      } else if (k == 3) {    // one vertex kept: (v, m0, m1)
        const int ti = s[0] == -1 ? 0 : (s[1] == -1 ? 1 : 2);
        double m0[3], m1[3];
        clip_cross(V, ti, pl, m0);
        clip_cross(V, (ti + 2) % 3, pl, m1);
        headfit_tri(V + 3 * ti, m0, m1, pl, m);
      }
      const double tot = headfit_wave_reduce(m, lane);
      if ((lane & 3) == 0) s_red[bf][wave][word] = tot;
    }
    __syncthreads();
    if (tid < SH_HF_WORDS)
      fslab[(((size_t)bi * pc + q) * tstride + t) * SH_HF_WORDS + tid] = ((s_red[bf][0][tid] + s_red[bf][1][tid]) + s_red[bf][2][tid]) + s_red[bf][3][tid];
  }
}

// one lane per cut of planes [p0, p0 + pc) of every humerus (n = B x pc lanes; p0 = 0, pc = P: the batch): the record from the cut's
// moments, its ring sums and its sh_resection
__global__ void k_headfit_solve(const sh_resection* __restrict__ recs /* B x P */, const int* __restrict__ cut_status /* B x P */,
                                const double* __restrict__ moments /* B x P x 16 */, const double* __restrict__ ringm /* B x P x 8 */,
                                const sh_landmarks* __restrict__ lm /* nullable: no run with the anatomic neck and the csys */, int P, int p0, int pc,
                                int n, sh_head_fit* __restrict__ out /* B x P */) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int i = (j / pc) * P + p0 + j % pc;
  sh_head_fit r;
  memset(&r, 0, sizeof r);
  const int st0 = cut_status[i];
  if (st0 != 0) {      // the humerus' record failed: its status in both halves, nothing else
    r.sphere_status = st0; r.ring_status = st0;
    out[i] = r;
    return;
  }
  const sh_resection rec = recs[i];
  const double* pl = rec.plane_point; const double* nn = rec.plane_normal;
  const double nlen = sqrt((nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2]);
  const double un[3] = {nn[0] / nlen, nn[1] / nlen, nn[2] / nlen};
  const double* m = moments + (size_t)i * 16;
  r.fit_area = m[0];
  bool sphere = false;
  if (m[0] != 0.0) {
    double c[3], rad, rms;
    if (head_sphere_from_moments(m, c, &rad, &rms)) {
      sphere = true;
      for (int k = 0; k < 3; ++k) r.sphere_center[k] = pl[k] + c[k];
      r.sphere_radius = rad; r.sphere_rms = rms;
      r.cap_height = rad + ((c[0] * un[0] + c[1] * un[1]) + c[2] * un[2]);
    } else r.sphere_status = SH_ERR_GEOMETRY_DEV;
  }
  const sh_landmarks* L = lm ? lm + i / P : nullptr;
  if (!L || L->status != 0) { const double qnan = __longlong_as_double(0x7ff8000000000000ll); r.center_articular[0] = r.center_articular[1] = r.center_articular[2] = qnan; }
  else if (sphere) xform_pt(L->csys_articular, r.sphere_center[0], r.sphere_center[1], r.sphere_center[2], r.center_articular);
  r.ring_status = rec.status;
  if (rec.status == 0 && rec.n_loops > 0) {
    double dir[2];
    if (ellipse_from_moments(ringm + (size_t)i * 8, &r.cut_semi_major, &r.cut_semi_minor, dir)) {
      double u[3], w[3];
      resect_basis(un, u, w);
      double dd[3];
      for (int k = 0; k < 3; ++k) dd[k] = dir[0] * u[k] + dir[1] * w[k];
      const double lead = dd[0] != 0.0 ? dd[0] : (dd[1] != 0.0 ? dd[1] : dd[2]);
      for (int k = 0; k < 3; ++k) r.cut_major_dir[k] = lead < 0.0 ? -dd[k] : dd[k];
    }      // (a largest loop without area has no ellipse: the ring fields stay zero)
  }
  out[i] = r;
}

}  // namespace sh
