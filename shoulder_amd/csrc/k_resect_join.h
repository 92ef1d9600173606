// k_resect_join.h -- the body of k_resect_join (k_resect.h), included once per mode: SH_RJ_NAME the kernel's name, SH_RJ_FIT 0 / 1,
// SH_RJ_SEAT 0 / 1 (only with SH_RJ_FIT).
// SH_RJ_FIT = 1 (k_resect_join_fit, the head fit of k_headfit.h): the cut's moment slab is added in tile order as well
// ("resect.fit_moments"), and the largest loop's loop carries the three second-moment shoelace sums beside the area's ("resect.fit_ring":
// sum cr, the two centroid sums, then sum cr (x0^2 + x0 x1 + x1^2), the same in y, sum cr (x0 y1 + 2 x0 y0 + 2 x1 y1 + x1 y0)), same tree.
// SH_RJ_SEAT = 1 (k_resect_join_seat, the seats of k_seat.h): the fitted join that also stores the largest loop's in-plane coordinates
// about the plane point -- the (x0, y0) its shoelace terms are made of -- in sh_resect_ring's order to the pass' ring buffer
// ("resect.seat_ring": per cut of the pass SH_MAXSEG u's, then SH_MAXSEG w's; n_ring of the record tells how many).
// SH_RJ_FIT = 0 is k_resect_join as it was: the preprocessor leaves the other modes' statements out.  (No include guard.)
__global__ void __launch_bounds__(SH_RS_JOIN_THREADS)
SH_RJ_NAME(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
              const double* __restrict__ planes, int P, int p0, int pc, int b0, int tstride, const int* __restrict__ cut_status /* B x P */,
              const ResectPart* __restrict__ slab, const int* __restrict__ seg_count, const int* __restrict__ segs,
#if SH_RJ_FIT
              sh_resection* __restrict__ out /* B x P */, const double* __restrict__ fit_slab /* [grid][tstride][16] */,
              double* __restrict__ fit_moments /* B x P x 16 */, double* __restrict__ fit_ring /* B x P x 8 */
#if SH_RJ_SEAT
              , double* __restrict__ ring_uw /* [cuts of the pass][2][SH_MAXSEG] */
#endif
              ) {
  sh_resection* const out_one = nullptr;
  double* const ring_out = nullptr;
#else
              sh_resection* __restrict__ out /* B x P */, sh_resection* __restrict__ out_one /* nullable: the record goes here instead */,
              double* __restrict__ ring_out /* nullable: (SH_MAXSEG + 1) x 3 */) {
#endif
  constexpr int CAP = SH_MAXSEG, HASH = 2048, T = SH_RS_JOIN_THREADS;
  __shared__ unsigned long long skey[CAP];      // start keys; then the ring's z
  __shared__ unsigned long long bufA[CAP];      // end keys, label ping; then the ring's x
  __shared__ unsigned long long bufB[CAP];      // hash table, label pong; then the ring's y
  __shared__ int nxt[CAP], prd[CAP], jmpA[CAP], jmpB[CAP], offA[CAP], offB[CAP], fid[CAP];
  __shared__ unsigned long long l_key[SH_MAXLOOPS];
  __shared__ int l_start[SH_MAXLOOPS], l_len[SH_MAXLOOPS], l_off[SH_MAXLOOPS];
  __shared__ double l_area[SH_MAXLOOPS];
  __shared__ int n_loops, bad;
  __shared__ double s_sum[3];
  __shared__ int s_ncut;
  __shared__ double s_best[4][T / 64];
  int* const table = (int*)bufB;

  const int cut = blockIdx.x, bi = cut / pc, q = cut - bi * pc, b = b0 + bi, p = p0 + q, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  sh_resection* rec = out_one ? out_one : out + (size_t)b * P + p;
  const int st0 = cut_status[(size_t)b * P + p];
  const double* plg = planes + ((size_t)b * P + p) * 6;
  const double pl[6] = {plg[0], plg[1], plg[2], plg[3], plg[4], plg[5]};
  if (st0 != 0) {      // the humerus' record failed: its status, nothing else
    if (tid == 0) {
      sh_resection r;
      memset(&r, 0, sizeof r);
      r.status = st0;
      *rec = r;
    }
    return;
  }
  const long long f0 = foff[b], nf = foff[b + 1] - f0;
  const int ntile = (int)((nf + SH_RS_TILE - 1) / SH_RS_TILE);
  if (tid == 0) { n_loops = 0; bad = 0; }
  // the face sums: tiles lane-strided in order, then the shuffle tree -- a fixed order for a given face count
  if (wave == 0) {
    const ResectPart* sp = slab + (size_t)cut * tstride;
    double vol = 0.0, ar = 0.0, hm = 0.0; int nc = 0;
    for (int t = lane; t < ntile; t += 64) { const ResectPart r = sp[t]; vol += r.vol; ar += r.area; hm = fmax(hm, r.hmax); nc += r.n_cut; }
    for (int off = 32; off > 0; off >>= 1) {
      vol += __shfl_down(vol, off); ar += __shfl_down(ar, off); hm = fmax(hm, __shfl_down(hm, off)); nc += __shfl_down(nc, off);
    }
    if (lane == 0) { s_sum[0] = vol; s_sum[1] = ar; s_sum[2] = hm; s_ncut = nc; }
  }
#if SH_RJ_FIT
  {      // the moment slab: word k = tid & 15 of tiles g, g + 16, ... (g = tid >> 4), the four groups of a wave, the waves in order
    __shared__ double s_fit[T / 64][16];
    const double* fs = fit_slab + (size_t)cut * tstride * 16;
    const int k = tid & 15;
    double s = 0.0;
    for (int t = tid >> 4; t < ntile; t += T / 16) s += fs[(size_t)t * 16 + k];
    s += __shfl_down(s, 32); s += __shfl_down(s, 16);
    if (lane < 16) s_fit[wave][k] = s;
    __syncthreads();
    if (tid < 16) fit_moments[((size_t)b * P + p) * 16 + tid] = ((s_fit[0][tid] + s_fit[1][tid]) + s_fit[2][tid]) + s_fit[3][tid];
  }
#endif
  for (int i = tid; i < HASH; i += T) table[i] = -1;
  const int n = seg_count[cut];
  __syncthreads();
  const double nlen = sqrt((pl[3] * pl[3] + pl[4] * pl[4]) + pl[5] * pl[5]);
  double un[3] = {pl[3] / nlen, pl[4] / nlen, pl[5] / nlen}, u[3], w[3];
  resect_basis(un, u, w);
  int status = 0, nl = 0, best = 0;
  const float* vb = verts + 3 * voff[b];
  const int* fb = faces + 3 * f0;
  if (n > CAP) status = SH_ERR_CAPACITY_DEV;
  else if (n > 0) {
    const int* sg = segs + (size_t)cut * SH_MAXSEG;
    for (int i = tid; i < n; i += T) {
      const int f = sg[i];
      int id[3]; double V[9];
      resect_load_face(vb, fb, f, id, V);
      const ResectEnds e = resect_ends(V, id, pl);
      fid[i] = f; skey[i] = e.skey; bufA[i] = e.ekey; prd[i] = -1;
      if (!e.ok || e.skey == e.ekey) bad = 1;
    }
    __syncthreads();
    for (int i = tid; i < n; i += T) {
      const unsigned long long k = skey[i];
      uint32_t h = hash_key64(k) & (HASH - 1);
      for (;;) {
        const int o = atomicCAS(&table[h], -1, i);
        if (o == -1) break;
        if (skey[o] == k) { bad = 1; break; }      // two segments leave one crossing: no simple loop
        h = (h + 1) & (HASH - 1);
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += T) {
      const unsigned long long k = bufA[i];
      uint32_t h = hash_key64(k) & (HASH - 1);
      int t, found = -1;
      while ((t = table[h]) != -1) {
        if (skey[t] == k) { found = t; break; }
        h = (h + 1) & (HASH - 1);
      }
      if (found < 0) { found = i; bad = 1; }      // an open chain
      else if (atomicExch(&prd[found], i) != -1) bad = 1;      // two segments arrive at one crossing
      nxt[i] = found;
    }
    __syncthreads();
    if (bad) status = SH_ERR_GEOMETRY_DEV;      // (uniform)
    else {
      // nxt is a permutation: every segment lies on one closed loop.  One pointer-jumping pass: the loop's smallest start key and
      // the forward distance to its node (slice_link_plane's scheme).
      unsigned long long* labA = bufA; unsigned long long* labB = bufB;
      int* ja = jmpA; int* jb = jmpB; int* ra = offA; int* rb = offB;
      for (int i = tid; i < n; i += T) { labA[i] = skey[i]; ja[i] = nxt[i]; ra[i] = 0; }
      __syncthreads();
      for (int span = 1; span < n; span <<= 1) {
        for (int i = tid; i < n; i += T) {
          const int j = ja[i];
          const unsigned long long a = labA[i], c = labA[j];
          const bool own = a <= c;
          labB[i] = own ? a : c;
          rb[i] = own ? ra[i] : span + ra[j];
          jb[i] = ja[j];
        }
        __syncthreads();
        unsigned long long* tl = labA; labA = labB; labB = tl;
        int* tj = ja; ja = jb; jb = tj;
        int* tr = ra; ra = rb; rb = tr;
      }
      for (int i = tid; i < n; i += T)
        if (ra[i] == 0) { const int l = atomicAdd(&n_loops, 1); if (l < SH_MAXLOOPS) l_start[l] = i; }
      __syncthreads();
      nl = n_loops;
      if (nl > SH_MAXLOOPS) { status = SH_ERR_CAPACITY_DEV; nl = 0; }      // (uniform)
      else {
        if (tid == 0) {      // canonical loop order: ascending start key
          for (int a = 1; a < nl; ++a) {
            const int v = l_start[a]; int c = a - 1;
            while (c >= 0 && skey[l_start[c]] > skey[v]) { l_start[c + 1] = l_start[c]; --c; }
            l_start[c + 1] = v;
          }
          int off = 0;
          for (int l = 0; l < nl; ++l) {
            const int s = l_start[l], L = ra[nxt[s]] + 1;
            l_len[l] = L; l_off[l] = off; off += L; l_key[l] = skey[s];
          }
        }
        __syncthreads();
        // ring position of every segment's start crossing; its point: of the two faces that compute this crossing the one whose
        // new vertex slice_plane's merge keeps (smallest pre-merge index: quads before triangles, then face order)
        int my_pos[CAP / T]; double my_pt[CAP / T][3];
        {
          int c = 0;
          for (int i = tid; i < n; i += T, ++c) {
            const unsigned long long key = labA[i];
            int l = 0;
            for (int qq = 0; qq < nl; ++qq) if (l_key[qq] == key) { l = qq; break; }
            const int r = ra[i];
            my_pos[c] = l_off[l] + (r == 0 ? 0 : l_len[l] - r);
            int id[3]; double V[9];
            const int f = fid[i];
            resect_load_face(vb, fb, f, id, V);
            const ResectEnds e = resect_ends(V, id, pl);
            const int g = fid[prd[i]];
            int idg[3]; double Vg[9];
            resect_load_face(vb, fb, g, idg, Vg);
            const ResectEnds eg = resect_ends(Vg, idg, pl);
            const bool own = e.is_tri != eg.is_tri ? !e.is_tri : f < g;
            if (own) resect_point(V, id, e.sj, e.skey, pl, my_pt[c]);
            else resect_point(Vg, idg, eg.ej, eg.ekey, pl, my_pt[c]);
          }
        }
        __syncthreads();      // labels, keys and ranks are dead: the ring takes their place
        double* rx = (double*)bufA; double* ry = (double*)bufB; double* rz = (double*)skey;
        {
          int c = 0;
          for (int i = tid; i < n; i += T, ++c) { rx[my_pos[c]] = my_pt[c][0]; ry[my_pos[c]] = my_pt[c][1]; rz[my_pos[c]] = my_pt[c][2]; }
        }
        __syncthreads();
        // shoelace area of every loop about the plane point: one wave per loop, lane-strided terms in ring order, fixed tree
        for (int l = wave; l < nl; l += T / 64) {
          const int o = l_off[l], L = l_len[l];
          double a2 = 0.0;
          for (int k = lane; k < L; k += 64) {
            const int kn = k + 1 == L ? 0 : k + 1;
            const double ax = rx[o + k] - pl[0], ay = ry[o + k] - pl[1], az = rz[o + k] - pl[2];
            const double bx = rx[o + kn] - pl[0], by = ry[o + kn] - pl[1], bz = rz[o + kn] - pl[2];
            const double x0 = (ax * u[0] + ay * u[1]) + az * u[2], y0 = (ax * w[0] + ay * w[1]) + az * w[2];
            const double x1 = (bx * u[0] + by * u[1]) + bz * u[2], y1 = (bx * w[0] + by * w[1]) + bz * w[2];
            a2 += x0 * y1 - x1 * y0;
          }
          for (int off = 32; off > 0; off >>= 1) a2 += __shfl_down(a2, off);
          if (lane == 0) l_area[l] = 0.5 * a2;
        }
        __syncthreads();
        for (int l = 1; l < nl; ++l) if (fabs(l_area[l]) > fabs(l_area[best])) best = l;
      }
    }
  }
  __syncthreads();
  // the largest loop: perimeter and centroid sums (all waves, lane-strided in ring order, fixed tree, waves added in order)
  double per = 0.0, sx = 0.0, sy = 0.0, a2b = 0.0;
#if SH_RJ_FIT
  double qxx = 0.0, qyy = 0.0, qxy = 0.0;
  __shared__ double s_fitb[3][T / 64];
#endif
  if (nl > 0) {
    const double* rx = (const double*)bufA; const double* ry = (const double*)bufB; const double* rz = (const double*)skey;
    const int o = l_off[best], L = l_len[best];
    for (int k = tid; k < L; k += T) {
      const int kn = k + 1 == L ? 0 : k + 1;
      const double dx = rx[o + kn] - rx[o + k], dy = ry[o + kn] - ry[o + k], dz = rz[o + kn] - rz[o + k];
      per += sqrt((dx * dx + dy * dy) + dz * dz);
      const double ax = rx[o + k] - pl[0], ay = ry[o + k] - pl[1], az = rz[o + k] - pl[2];
      const double bx = rx[o + kn] - pl[0], by = ry[o + kn] - pl[1], bz = rz[o + kn] - pl[2];
      const double x0 = (ax * u[0] + ay * u[1]) + az * u[2], y0 = (ax * w[0] + ay * w[1]) + az * w[2];
      const double x1 = (bx * u[0] + by * u[1]) + bz * u[2], y1 = (bx * w[0] + by * w[1]) + bz * w[2];
      const double cr = x0 * y1 - x1 * y0;
      a2b += cr; sx += (x0 + x1) * cr; sy += (y0 + y1) * cr;
#if SH_RJ_FIT
      {
        qxx += cr * ((x0 * x0 + x0 * x1) + x1 * x1); qyy += cr * ((y0 * y0 + y0 * y1) + y1 * y1);
        qxy += cr * (((x0 * y1 + 2.0 * (x0 * y0)) + 2.0 * (x1 * y1)) + x1 * y0);
      }
#endif
    }
    for (int off = 32; off > 0; off >>= 1) {
      per += __shfl_down(per, off); sx += __shfl_down(sx, off); sy += __shfl_down(sy, off); a2b += __shfl_down(a2b, off);
#if SH_RJ_FIT
      qxx += __shfl_down(qxx, off); qyy += __shfl_down(qyy, off); qxy += __shfl_down(qxy, off);
#endif
    }
    if (lane == 0) { s_best[0][wave] = per; s_best[1][wave] = sx; s_best[2][wave] = sy; s_best[3][wave] = a2b; }
#if SH_RJ_FIT
    if (lane == 0) { s_fitb[0][wave] = qxx; s_fitb[1][wave] = qyy; s_fitb[2][wave] = qxy; }
#endif
  }
  __syncthreads();
  if (tid == 0) {
    sh_resection r;
    memset(&r, 0, sizeof r);
    for (int k = 0; k < 3; ++k) { r.plane_point[k] = pl[k]; r.plane_normal[k] = pl[3 + k]; }
    r.head_volume = s_sum[0] / 6.0;
    r.head_area = 0.5 * s_sum[1];
    r.head_height = s_sum[2] / nlen;
    r.n_cut_faces = s_ncut;
    r.status = status;
    if (nl > 0) {
      double v[4];
      for (int k = 0; k < 4; ++k) v[k] = ((s_best[k][0] + s_best[k][1]) + s_best[k][2]) + s_best[k][3];
      r.cut_area = fabs(l_area[best]);
      r.cut_perimeter = v[0];
      const double cx = v[1] / (3.0 * v[3]), cy = v[2] / (3.0 * v[3]);      // polygon centroid: sum (x0 + x1) cr / (6 A), A = sum cr / 2
      for (int k = 0; k < 3; ++k) r.cut_centroid[k] = (pl[k] + cx * u[k]) + cy * w[k];
      double tot = 0.0;
      for (int l = 0; l < nl; ++l) tot += l_area[l];
      r.cap_area = fabs(tot);
      r.n_loops = nl; r.n_ring = l_len[best];
#if SH_RJ_FIT
      {
        double* fr = fit_ring + ((size_t)b * P + p) * 8;
        fr[0] = v[3]; fr[1] = v[1]; fr[2] = v[2];
        for (int k = 0; k < 3; ++k) fr[3 + k] = ((s_fitb[k][0] + s_fitb[k][1]) + s_fitb[k][2]) + s_fitb[k][3];
      }
#endif
    }
    *rec = r;
  }
#if SH_RJ_SEAT
  if (nl > 0) {
    const double* rx = (const double*)bufA; const double* ry = (const double*)bufB; const double* rz = (const double*)skey;
    const int o = l_off[best], L = l_len[best];
    const bool rev = l_area[best] < 0;
    double* dst = ring_uw + (size_t)cut * 2 * SH_MAXSEG;
    for (int k = tid; k < L; k += T) {
      const int src = rev ? (k == 0 ? 0 : L - k) : k;
      const double ax = rx[o + src] - pl[0], ay = ry[o + src] - pl[1], az = rz[o + src] - pl[2];
      dst[k] = (ax * u[0] + ay * u[1]) + az * u[2]; dst[SH_MAXSEG + k] = (ax * w[0] + ay * w[1]) + az * w[2];
    }
  }
#endif
  if (ring_out && nl > 0) {
    const double* rx = (const double*)bufA; const double* ry = (const double*)bufB; const double* rz = (const double*)skey;
    const int o = l_off[best], L = l_len[best];
    const bool rev = l_area[best] < 0;      // clockwise seen from the normal's tip: backwards from the same start
    for (int k = tid; k <= L; k += T) {
      const int kk = k == L ? 0 : k, src = rev ? (kk == 0 ? 0 : L - kk) : kk;
      ring_out[3 * k] = rx[o + src]; ring_out[3 * k + 1] = ry[o + src]; ring_out[3 * k + 2] = rz[o + src];
    }
  }
}
