// Test shim (NOT product): the repair rules of shoulder_amd/csrc/sh_scalar.h (rep_face, rep_slot, rep_same, rep_center, rep_v6_term,
// rep_succ, rep_hole_status, rep_fill_face, rep_centroid, rep_depth -- the source k_repair.h runs on the device) and, of sh_query.h, the
// argument checks of sh_mesh_repair and its buffer plan, on the host, for tests/test_repair_host.py.  rc_repair makes the buffers of one
// mesh as the kernels do, on the topology it is handed: the first face of every label, a walk through a queue, the contradictions, the
// shells' lists, terms, block sums and V6, the nesting sums in blocks of face indices, the oriented copy, the border half-edges
// compacted in ascending order, the successors found by bisection, TWO RUNS OF POINTER DOUBLING on two arrays each, the cut of the cycles
// that pass a vertex twice and the doubling again, the scans over the
// starts and the holes, the fill faces, the new vertices and the records.  Its own main() walks a box stored inside out, an open box
// under both fills, a Moebius strip and the checks, so that the file can be built as a stand-alone program with
// -fsanitize=address,undefined.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../include/shoulder_hip.h"
#include "../../shoulder_amd/csrc/sh_query.h"
#include "../../shoulder_amd/csrc/sh_scalar.h"

static_assert(sizeof(sh_repair_options) == 24 && sizeof(sh_repair_info) == 64 && sizeof(sh_repair_shell) == 40 && sizeof(sh_repair_hole) == 32, "the records of sh_mesh_repair");
static_assert(SH_REPAIR_NESTED == SH_REP_ORIENT_NESTED && SH_REPAIR_CENTROID == SH_REP_FILL_CENTROID && SH_REPAIR_HOLE_TOO_SHORT == SH_REP_HOLE_TOO_SHORT, "the modes of sh_mesh_repair");

extern "C" void rc_repair(const float* verts, int nv, const int* faces, int nf, const int32_t* adj /* 3 nf */, const int32_t* label /* nf */, const sh_topology* tinfo,
                          const sh_shell* tshells /* S */, int S, const sh_repair_options* opt, sh_repair_info* info, sh_repair_shell* shells /* S */,
                          sh_repair_hole* holes /* max_holes */, unsigned char* flip /* nf */, int32_t* rfaces /* 3 (nf + border) */, float* rverts /* 3 (nv + border / 3) */) {
  const int orient = opt->orient, fill = opt->fill, max_holes = opt->max_holes;
  memset(shells, 0, (size_t)S * sizeof(sh_repair_shell));
  memset(holes, 0, (size_t)max_holes * sizeof(sh_repair_hole));
  std::vector<unsigned char> par((size_t)nf + 1, 0);
  for (int f = 0; f < nf; ++f) flip[f] = 0;
  int status = tinfo->status != 0 || nf > SH_REPAIR_LDS_FACES ? SH_ERR_CAPACITY : 0;
  // k_repair_seed, k_repair_parity
  std::vector<int> first((size_t)nf + 1, 0x7f7f7f7f), bad((size_t)nf + 1, 0), queue, next;
  std::vector<unsigned char> seen((size_t)nf + 1, 0), bit((size_t)nf + 1, 0);
  if (!status) {
    for (int f = 0; f < nf; ++f)
      if (label[f] >= 0 && label[f] < nf && f < first[label[f]]) first[label[f]] = f;
    for (int f = 0; f < nf; ++f)
      if (label[f] >= 0 && first[label[f]] == f) { seen[f] = 1; queue.push_back(f); }
    int level = 0;
    while (!queue.empty()) {
      if (level >= opt->max_rounds) { status = SH_ERR_CAPACITY; break; }
      next.clear();
      for (int f : queue)
        for (int e = 0; e < 3; ++e) {
          const int g = adj[3 * (size_t)f + e];
          if (g < 0 || g >= nf || seen[g]) continue;
          seen[g] = 1;
          bit[g] = (unsigned char)(bit[f] ^ sh::rep_same(faces, f, e, g));
          next.push_back(g);
        }
      queue.swap(next);
      ++level;
    }
  }
  if (!status) {
    for (int f = 0; f < nf; ++f) {
      if (label[f] < 0) continue;
      for (int e = 0; e < 3; ++e) {
        const int g = adj[3 * (size_t)f + e];
        if (g <= f || g >= nf) continue;
        if ((bit[f] ^ bit[g]) != sh::rep_same(faces, f, e, g)) bad[label[f]] = 1;
      }
    }
    for (int f = 0; f < nf; ++f) flip[f] = par[f] = orient >= SH_REPAIR_WINDING && label[f] >= 0 && !bad[label[f]] ? bit[f] : 0;
  }
  const int written = tinfo->shells_written < S ? tinfo->shells_written : S;
  // k_repair_shell
  std::vector<std::vector<int>> lists((size_t)(status ? 0 : written));
  if (!status) {
    for (int f = 0; f < nf; ++f)
      if (label[f] >= 0 && label[f] < written) lists[label[f]].push_back(f);
    for (int k = 0; k < written; ++k) {
      const std::vector<int>& list = lists[k];
      const int n = (int)list.size();
      const bool ok = !bad[k];
      double v6 = 0.0;
      int inv = 0;
      if (ok && orient >= SH_REPAIR_OUTWARD) {
        const sh_shell& rec = tshells[k];
        const double o[3] = {sh::rep_center(rec.lo[0], rec.hi[0]), sh::rep_center(rec.lo[1], rec.hi[1]), sh::rep_center(rec.lo[2], rec.hi[2])};
        std::vector<double> term((size_t)n + 1);
        for (int i = 0; i < n; ++i) {
          int c[3];
          sh::rep_face(faces, list[i], flip[list[i]], c);
          term[i] = sh::rep_v6_term(verts, c, o);
        }
        for (int i0 = 0; i0 < n; i0 += SH_REP_V6_BLOCK) {
          double sum = 0.0;
          for (int i = i0; i < n && i < i0 + SH_REP_V6_BLOCK; ++i) sum += term[i];
          v6 += sum;
        }
        inv = v6 < 0.0 ? 1 : 0;
      }
      int flips = 0;
      for (int f : list) { flips += flip[f]; flip[f] = par[f] = (unsigned char)(flip[f] ^ inv); }
      sh_repair_shell r;
      r.status = ok ? 0 : SH_REPAIR_NONORIENTABLE; r.parity_flips = flips; r.inverted = inv; r.depth = -1; r.holes = 0; r.holes_filled = 0; r.V6 = v6; r.W = 0.0;
      shells[k] = r;
    }
  }
  // k_repair_nest
  if (!status && orient == SH_REPAIR_NESTED && tinfo->n_shells <= written)
    for (int k = 0; k < written; ++k) {
      if (bad[k]) { shells[k].depth = 0; shells[k].W = 0.0; continue; }
      const float* pk = verts + 3 * (size_t)faces[3 * (size_t)tshells[k].first_face];
      const double p[3] = {(double)pk[0], (double)pk[1], (double)pk[2]};
      double total = 0.0;
      for (int f0 = 0; f0 < nf; f0 += SH_WIND_BLOCK) {
        double sum = 0.0;
        for (int f = f0; f < nf && f < f0 + SH_WIND_BLOCK; ++f) {
          const int lab = label[f];
          if (lab < 0 || lab == k || lab >= written) continue;
          if (bad[lab] || tshells[lab].border_slots != 0 || tshells[lab].nonmanifold_slots != 0) continue;
          int c[3];
          sh::rep_face(faces, f, par[f], c);
          double P[3][3];
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) P[i][j] = (double)verts[3 * (size_t)c[i] + j];
          sum += sh::solid_angle_tri(p, P[0], P[1], P[2]);
        }
        total += sum;
      }
      int ambiguous;
      shells[k].W = total / (4.0 * M_PI);
      shells[k].depth = sh::rep_depth(shells[k].W, &ambiguous);
      if (ambiguous) shells[k].status = SH_REPAIR_AMBIGUOUS;
      if (shells[k].depth & 1)
        for (int f : lists[k]) flip[f] = (unsigned char)(par[f] ^ 1);
    }
  // k_repair_emit
  for (int f = 0; f < nf; ++f) sh::rep_face(faces, f, flip[f], rfaces + 3 * (size_t)f);
  memcpy(rverts, verts, (size_t)nv * 12);
  // k_repair_holes
  int n = 0, H = 0, faces_added = 0, verts_added = 0, blocked = 0, filled_n = 0, largest = 0;
  if (!status) {
    std::vector<int> half;
    for (int f = 0; f < nf; ++f)
      for (int e = 0; e < 3; ++e)
        if (adj[3 * (size_t)f + sh::rep_slot(e, flip[f])] == SH_ADJ_BORDER) half.push_back(3 * f + e);
    n = (int)half.size();
    std::vector<int> succ((size_t)n + 1), cut((size_t)n + 1), cyc((size_t)n + 1), start((size_t)n + 1), dist((size_t)n + 1), hidx((size_t)n + 1);
    for (int i = 0; i < n; ++i) {
      int sf, se, at = -1;
      if (sh::rep_succ(faces, adj, flip, nf, half[i] / 3, half[i] % 3, &sf, &se)) {
        const int want = 3 * sf + se;
        int lo = 0, hi = n - 1;
        while (lo <= hi) {
          const int mid = (lo + hi) >> 1;
          if (half[mid] == want) { at = mid; break; }
          if (half[mid] < want) lo = mid + 1; else hi = mid - 1;
        }
      }
      succ[i] = at;
    }
    int R = 1;
    while ((1 << (R - 1)) < n) ++R;
    // repair_loops: two runs of pointer doubling, each round from one pair of arrays into the other
    auto loops = [&](const std::vector<int>& to) {
      std::vector<int> p0((size_t)n + 1), p1((size_t)n + 1), m0((size_t)n + 1), m1((size_t)n + 1);
      for (int i = 0; i < n; ++i) { p0[i] = to[i]; m0[i] = i; }
      std::vector<int>*pi = &p0, *po = &p1, *mi = &m0, *mo = &m1;
      for (int r = 0; r < R; ++r) {
        for (int i = 0; i < n; ++i) {
          const int p = (*pi)[i], a = (*mi)[i], b = p >= 0 ? (*mi)[p] : a;
          (*mo)[i] = b < a ? b : a;
          (*po)[i] = p >= 0 ? (*pi)[p] : -1;
        }
        std::swap(pi, po); std::swap(mi, mo);
      }
      for (int i = 0; i < n; ++i) { cyc[i] = (*pi)[i] >= 0; start[i] = cyc[i] ? (*mi)[i] : -1; }
      std::vector<int>*ni = &p0, *no = &p1, *di = &m0, *dq = &m1;
      for (int i = 0; i < n; ++i) { (*ni)[i] = cyc[i] && to[i] != start[i] ? to[i] : -1; (*di)[i] = (*ni)[i] >= 0 ? 1 : 0; }
      for (int r = 0; r < R; ++r) {
        for (int i = 0; i < n; ++i) {
          const int p = (*ni)[i];
          (*dq)[i] = (*di)[i] + (p >= 0 ? (*di)[p] : 0);
          (*no)[i] = p >= 0 ? (*ni)[p] : -1;
        }
        std::swap(ni, no); std::swap(di, dq);
      }
      for (int i = 0; i < n; ++i) dist[i] = (*di)[i];
    };
    loops(succ);
    // a cycle that passes a vertex more than once is cut there: the half-edges of one cycle with one head, in the order of their places
    // (here a plain search over the half-edges; the kernel walks the head's incidence row)
    bool pinched = false;
    for (int i = 0; i < n; ++i) {
      cut[i] = succ[i];
      if (!cyc[i]) continue;
      int c[3];
      sh::rep_face(faces, half[i] / 3, flip[half[i] / 3], c);
      const int w = c[(half[i] % 3 + 1) % 3], top = dist[start[i]], mine = top - dist[i];
      int best = -1, best_at = -1;
      for (int k = 0; k < n; ++k) {
        if (k == i || !cyc[k] || start[k] != start[i]) continue;
        int d[3];
        sh::rep_face(faces, half[k] / 3, flip[half[k] / 3], d);
        if (d[(half[k] % 3 + 1) % 3] != w) continue;
        const int place = top - dist[k], key = place < mine ? place + top + 1 : place;
        if (key > best) { best = key; best_at = k; }
      }
      if (best_at >= 0) { cut[i] = succ[best_at]; pinched = true; }
    }
    if (pinched) loops(cut);
    for (int i = 0; i < n; ++i) blocked += !cyc[i];
    for (int i = 0; i < n; ++i) { hidx[i] = H; H += cyc[i] && start[i] == i; }
    std::vector<int> hst((size_t)H + 1), hL((size_t)H + 1), hsta((size_t)H + 1), hff((size_t)H + 1), hvv((size_t)H + 1), heo((size_t)H + 1), order((size_t)n + 1);
    int ea = 0;
    for (int i = 0; i < n; ++i)
      if (cyc[i] && start[i] == i) {
        const int h = hidx[i], L = dist[i] + 1, lab = label[half[i] / 3];
        const int st = sh::rep_hole_status(L, lab >= 0 && !bad[lab], fill, opt->max_hole_edges);
        hst[h] = i; hL[h] = L; hsta[h] = st; heo[h] = ea; hff[h] = faces_added; hvv[h] = verts_added;
        ea += L;
        if (st == SH_REPAIR_HOLE_FILLED) { faces_added += sh::rep_fill_faces(L, fill); verts_added += sh::rep_fill_verts(fill); }
      }
    for (int i = 0; i < n; ++i) {
      if (!cyc[i]) continue;
      const int si = start[i], h = hidx[si], L = hL[h], j = L - 1 - dist[i];
      int c[3], c0[3], out[3];
      sh::rep_face(faces, half[i] / 3, flip[half[i] / 3], c);
      const int e = half[i] % 3, tail = c[e], head = c[e == 2 ? 0 : e + 1];
      order[heo[h] + j] = tail;
      if (hsta[h] != SH_REPAIR_HOLE_FILLED) continue;
      sh::rep_face(faces, half[si] / 3, flip[half[si] / 3], c0);
      const int k = sh::rep_fill_face(fill, L, j, c0[half[si] % 3], tail, head, nv + hvv[h], out);
      if (k >= 0) memcpy(rfaces + 3 * ((size_t)nf + hff[h] + k), out, 12);
    }
    for (int h = 0; h < H; ++h) {
      const int filled = hsta[h] == SH_REPAIR_HOLE_FILLED, L = hL[h], id = half[hst[h]], lab = label[id / 3];
      if (filled && fill == SH_REPAIR_CENTROID) sh::rep_centroid(verts, order.data() + heo[h], L, rverts + 3 * ((size_t)nv + hvv[h]));
      if (lab >= 0 && lab < written) { shells[lab].holes += 1; shells[lab].holes_filled += filled; }
      filled_n += filled;
      largest = L > largest ? L : largest;
      if (h < max_holes)
        holes[h] = sh_repair_hole{lab, id / 3, id % 3, L, hsta[h], filled ? nf + hff[h] : -1, filled ? sh::rep_fill_faces(L, fill) : 0,
                                  filled && fill == SH_REPAIR_CENTROID ? nv + hvv[h] : -1};
    }
  }
  sh_repair_info r;
  memset(&r, 0, sizeof r);
  const bool left = !status && tinfo->n_shells > tinfo->shells_written;
  r.status = status ? status : (left && orient == SH_REPAIR_NESTED ? SH_ERR_CAPACITY : 0);
  if (!status) {
    for (int k = 0; k < tinfo->n_shells && k < nf; ++k) r.shells_nonorientable += bad[k] != 0;
    for (int k = 0; k < written; ++k) r.shells_inverted += shells[k].inverted;
    for (int f = 0; f < nf; ++f) r.faces_flipped += flip[f];
  }
  r.holes = H; r.holes_written = H < max_holes ? H : max_holes; r.holes_filled = filled_n; r.largest_hole = largest; r.blocked_edges = blocked;
  r.faces_added = faces_added; r.verts_added = verts_added; r.faces_out = nf + faces_added; r.verts_out = nv + verts_added;
  r.flags = (r.faces_flipped > 0 || faces_added > 0 ? SH_REPAIR_CHANGED : 0) | (left && orient >= SH_REPAIR_OUTWARD ? SH_REPAIR_SHELLS_LEFT : 0);
  r.shell_records = S;
  *info = r;
}

// precheck_repair; the refusal's text to `text`
extern "C" int rc_precheck(int ctx, int have_opt, int orient, int fill, int max_hole_edges, int max_holes, int max_rounds, int reserved, int topology, int B, int n_pending,
                           char* text, int cap) {
  const sh::ArthroState st;
  const sh_repair_options opt = {orient, fill, max_hole_edges, max_holes, max_rounds, reserved};
  const sh::ArthroError e = sh::precheck_repair(have_opt ? &opt : nullptr, topology != 0, sh::ArthroFacts{ctx != 0, B, n_pending, 0, false, &st});
  if (text && cap > 0) { strncpy(text, e.text.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
  return e.code;
}

// out: blocks, the 3 (B + 1) starts, then the eleven sizes of REPAIR_BUFS
extern "C" void rc_plan(int B, int shell_records, int max_holes, const long long* voff, const long long* foff, const sh_topology* info, size_t* out) {
  long long maxV = 0, maxF = 0;
  for (int b = 0; b < B; ++b) {
    maxV = voff[b + 1] - voff[b] > maxV ? voff[b + 1] - voff[b] : maxV;
    maxF = foff[b + 1] - foff[b] > maxF ? foff[b + 1] - foff[b] : maxF;
  }
  const sh::RepairPlan p = sh::repair_plan(B, shell_records, max_holes, maxV, maxF, foff[B], voff, foff, info);
  size_t* o = out;
  *o++ = (size_t)p.blocks;
  for (long long x : p.off) *o++ = (size_t)x;
#define X(f, name, T, elem) *o++ = p.bytes.f;
  REPAIR_BUFS(X)
#undef X
}

// the sizes of the four records, then the offsets of every field in the header's order: options (6), info (16), shell (8), hole (8)
extern "C" void rc_sizes(int* out) {
  int* o = out;
  *o++ = (int)sizeof(sh_repair_options); *o++ = (int)sizeof(sh_repair_info); *o++ = (int)sizeof(sh_repair_shell); *o++ = (int)sizeof(sh_repair_hole);
#define OFF(T, f) *o++ = (int)offsetof(T, f);
  OFF(sh_repair_options, orient) OFF(sh_repair_options, fill) OFF(sh_repair_options, max_hole_edges) OFF(sh_repair_options, max_holes) OFF(sh_repair_options, max_rounds)
  OFF(sh_repair_options, reserved)
  OFF(sh_repair_info, status) OFF(sh_repair_info, shells_nonorientable) OFF(sh_repair_info, shells_inverted) OFF(sh_repair_info, faces_flipped) OFF(sh_repair_info, holes)
  OFF(sh_repair_info, holes_written) OFF(sh_repair_info, holes_filled) OFF(sh_repair_info, largest_hole) OFF(sh_repair_info, blocked_edges) OFF(sh_repair_info, faces_added)
  OFF(sh_repair_info, verts_added) OFF(sh_repair_info, faces_out) OFF(sh_repair_info, verts_out) OFF(sh_repair_info, flags) OFF(sh_repair_info, shell_records)
  OFF(sh_repair_info, reserved)
  OFF(sh_repair_shell, status) OFF(sh_repair_shell, parity_flips) OFF(sh_repair_shell, inverted) OFF(sh_repair_shell, depth) OFF(sh_repair_shell, holes)
  OFF(sh_repair_shell, holes_filled) OFF(sh_repair_shell, V6) OFF(sh_repair_shell, W)
  OFF(sh_repair_hole, shell) OFF(sh_repair_hole, start_face) OFF(sh_repair_hole, start_slot) OFF(sh_repair_hole, edges) OFF(sh_repair_hole, status)
  OFF(sh_repair_hole, first_face) OFF(sh_repair_hole, faces_added) OFF(sh_repair_hole, vertex)
#undef OFF
}

// ---- stand-alone run (sanitizer build) ----
struct Result {
  sh_repair_info info;
  std::vector<sh_repair_shell> shells;
  std::vector<sh_repair_hole> holes;
  std::vector<unsigned char> flip;
  std::vector<int32_t> faces;
  std::vector<float> verts;
};
// the adjacency by the topo_* rules, the labels by a flood from every unlabelled face in turn, one shell record each; then rc_repair
static Result run(const std::vector<float>& v, const std::vector<int>& f, int orient, int fill, int max_hole_edges = 4096, int max_holes = 8) {
  const int nv = (int)v.size() / 3, nf = (int)f.size() / 3, S = 4;
  std::vector<int32_t> vrow((size_t)nv + 1, 0), vface(3 * (size_t)nf + 1, -1), adj(3 * (size_t)nf + 1, SH_ADJ_DEGENERATE), label((size_t)nf + 1, -1);
  for (int i = 0; i < nf; ++i)
    if (!sh::topo_degenerate(&f[3 * (size_t)i], nv))
      for (int k = 0; k < 3; ++k) ++vrow[f[3 * (size_t)i + k] + 1];
  for (int i = 0; i < nv; ++i) vrow[i + 1] += vrow[i];
  std::vector<int> cur(vrow.begin(), vrow.end());
  for (int i = 0; i < nf; ++i)
    if (!sh::topo_degenerate(&f[3 * (size_t)i], nv))
      for (int k = 0; k < 3; ++k) vface[cur[f[3 * (size_t)i + k]]++] = i;
  sh_topology t;
  memset(&t, 0, sizeof t);
  for (int i = 0; i < nf; ++i) {
    if (sh::topo_degenerate(&f[3 * (size_t)i], nv)) continue;
    for (int e = 0; e < 3; ++e) {
      const int a = f[3 * (size_t)i + e];
      int owner, same;
      adj[3 * (size_t)i + e] = sh::topo_slot(f.data(), vface.data() + vrow[a], vrow[a + 1] - vrow[a], i, e, &owner, &same);
      if (owner && adj[3 * (size_t)i + e] == SH_ADJ_BORDER) ++t.border_edges;
    }
  }
  std::vector<sh_shell> ts((size_t)S);
  memset(ts.data(), 0, (size_t)S * sizeof(sh_shell));
  for (int i = 0; i < nf; ++i) {
    if (label[i] >= 0 || adj[3 * (size_t)i] == SH_ADJ_DEGENERATE) continue;
    const int k = t.n_shells++;
    std::vector<int> stack = {i};
    label[i] = k;
    while (!stack.empty()) {
      const int u = stack.back();
      stack.pop_back();
      if (k < S) {
        sh_shell& r = ts[k];
        if (r.faces++ == 0) { r.first_face = i; for (int c = 0; c < 3; ++c) r.lo[c] = r.hi[c] = v[3 * (size_t)f[3 * (size_t)u] + c]; }
        for (int j = 0; j < 3; ++j)
          for (int c = 0; c < 3; ++c) {
            const float x = v[3 * (size_t)f[3 * (size_t)u + j] + c];
            r.lo[c] = x < r.lo[c] ? x : r.lo[c]; r.hi[c] = x > r.hi[c] ? x : r.hi[c];
          }
      }
      for (int e = 0; e < 3; ++e) {
        const int g = adj[3 * (size_t)u + e];
        if (k < S) { ts[k].border_slots += g == SH_ADJ_BORDER; ts[k].nonmanifold_slots += g == SH_ADJ_NONMANIFOLD; }
        if (g >= 0 && label[g] < 0) { label[g] = k; stack.push_back(g); }
      }
    }
  }
  t.shells_written = t.n_shells < S ? t.n_shells : S;
  const sh_repair_options opt = {orient, fill, max_hole_edges, max_holes, SH_REPAIR_MAX_ROUNDS, 0};
  Result r;
  r.shells.resize((size_t)S); r.holes.resize((size_t)max_holes); r.flip.resize((size_t)nf + 1); r.faces.resize(3 * ((size_t)nf + t.border_edges) + 3);
  r.verts.resize(3 * ((size_t)nv + t.border_edges / 3) + 3);
  rc_repair(v.data(), nv, f.data(), nf, adj.data(), label.data(), &t, ts.data(), S, &opt, &r.info, r.shells.data(), r.holes.data(), r.flip.data(), r.faces.data(), r.verts.data());
  return r;
}

int main() {
  std::vector<float> bv(24);
  const std::vector<int> bf = {0, 2, 1, 1, 2, 3, 4, 5, 6, 5, 7, 6, 0, 1, 4, 1, 5, 4, 2, 6, 3, 3, 6, 7, 0, 4, 2, 2, 4, 6, 1, 3, 5, 3, 7, 5};
  for (int i = 0; i < 8; ++i) { bv[3 * i] = 120.f + ((i & 1) ? 30.f : 0.f); bv[3 * i + 1] = -85.f + ((i & 2) ? 20.f : 0.f); bv[3 * i + 2] = 410.f + ((i & 4) ? 10.f : 0.f); }
  // the box: nothing to do, V6 = 6 x its volume; stored inside out: inverted, and the stored faces come back reversed
  Result r = run(bv, bf, SH_REPAIR_OUTWARD, SH_REPAIR_CENTROID);
  if (r.info.status || r.info.flags || r.info.faces_flipped || r.info.holes || r.shells[0].V6 != 36000.0 || r.shells[0].inverted || r.info.faces_out != 12 || r.info.verts_out != 8 ||
      memcmp(r.faces.data(), bf.data(), 144) != 0) {
    printf("repair_check: box (V6 %.17g flipped %d)\n", r.shells[0].V6, r.info.faces_flipped); return 1;
  }
  std::vector<int> out = bf, one = bf;
  for (int i = 0; i < 12; ++i) std::swap(out[3 * i + 1], out[3 * i + 2]);
  r = run(bv, out, SH_REPAIR_OUTWARD, SH_REPAIR_CENTROID);
  if (r.info.status || r.shells[0].V6 != -36000.0 || !r.shells[0].inverted || r.info.shells_inverted != 1 || r.info.faces_flipped != 12 || memcmp(r.faces.data(), bf.data(), 144) != 0) {
    printf("repair_check: box inside out (V6 %.17g)\n", r.shells[0].V6); return 1;
  }
  // one face reversed: the winding alone puts it right
  std::swap(one[16], one[17]);
  r = run(bv, one, SH_REPAIR_WINDING, SH_REPAIR_FILL_NONE);
  if (r.info.faces_flipped != 1 || !r.flip[5] || r.shells[0].parity_flips != 1 || r.shells[0].V6 != 0.0 || memcmp(r.faces.data(), bf.data(), 144) != 0) {
    printf("repair_check: one reversed face (%d flipped)\n", r.info.faces_flipped); return 1;
  }
  // without face 0: one hole of three edges; the fan gives the face back up to a rotation, the centroid three faces and a vertex
  const std::vector<int> open(bf.begin() + 3, bf.end());
  r = run(bv, open, SH_REPAIR_OUTWARD, SH_REPAIR_FAN);
  bool back = r.info.holes == 1 && r.info.holes_filled == 1 && r.info.faces_added == 1 && r.info.verts_added == 0 && r.holes[0].edges == 3 && r.holes[0].first_face == 11;
  if (back) {
    const int32_t* g = r.faces.data() + 33;
    back = (g[0] == 0 && g[1] == 2 && g[2] == 1) || (g[0] == 2 && g[1] == 1 && g[2] == 0) || (g[0] == 1 && g[1] == 0 && g[2] == 2);
  }
  if (!back) { printf("repair_check: open box, fan (%d holes, %d faces)\n", r.info.holes, r.info.faces_added); return 1; }
  r = run(bv, open, SH_REPAIR_OUTWARD, SH_REPAIR_CENTROID);
  if (r.info.faces_added != 3 || r.info.verts_added != 1 || r.holes[0].vertex != 8 || r.verts[24] != 130.f || r.shells[0].holes_filled != 1 || r.info.largest_hole != 3) {
    printf("repair_check: open box, centroid (%d faces, x %.9g)\n", r.info.faces_added, r.verts[24]); return 1;
  }
  r = run(bv, open, SH_REPAIR_OUTWARD, SH_REPAIR_CENTROID, 3, 1);
  const Result longer = run(bv, std::vector<int>(bf.begin() + 6, bf.end()), SH_REPAIR_OUTWARD, SH_REPAIR_FAN, 3);
  if (r.info.holes_filled != 1 || longer.info.holes != 1 || longer.holes[0].edges != 4 || longer.holes[0].status != SH_REPAIR_HOLE_TOO_LONG || longer.info.faces_added != 0) {
    printf("repair_check: max_hole_edges (%d edges, status %d)\n", longer.holes[0].edges, longer.holes[0].status); return 1;
  }
  // a Moebius strip of ten faces: not orientable, unchanged, its border one loop that is not filled
  {
    std::vector<float> mv(30, 0.f);
    std::vector<int> mf;
    for (int i = 0; i < 5; ++i) {
      const double t = i * 1.2566370614359172;
      const double w[3] = {cos(t / 2) * cos(t), cos(t / 2) * sin(t), sin(t / 2)};
      for (int c = 0; c < 3; ++c) {
        const double m = c == 0 ? 30 * cos(t) : c == 1 ? 30 * sin(t) : 0.0;
        mv[3 * i + c] = (float)(m - 4 * w[c]); mv[3 * (i + 5) + c] = (float)(m + 4 * w[c]);
      }
      const int a = i, b = i + 5, c = i < 4 ? i + 1 : 5, d = i < 4 ? i + 6 : 0;
      mf.insert(mf.end(), {a, c, b, c, d, b});
    }
    r = run(mv, mf, SH_REPAIR_OUTWARD, SH_REPAIR_CENTROID);
    if (r.info.status || r.info.shells_nonorientable != 1 || r.shells[0].status != SH_REPAIR_NONORIENTABLE || r.info.faces_flipped || r.info.holes_filled || r.info.faces_added ||
        r.info.holes + r.info.blocked_edges == 0 || memcmp(r.faces.data(), mf.data(), 120) != 0) {
      printf("repair_check: Moebius strip (%d not orientable, %d holes, %d blocked)\n", r.info.shells_nonorientable, r.info.holes, r.info.blocked_edges); return 1;
    }
  }
  // the checks of sh_mesh_repair in their order
  char text[256];
  auto pre = [&](int ctx, int opt, int orient, int fill, int edges, int holes, int rounds, int reserved, int topo, int B, int pend) {
    return rc_precheck(ctx, opt, orient, fill, edges, holes, rounds, reserved, topo, B, pend, text, (int)sizeof text);
  };
  if (pre(1, 1, 2, 2, 4096, 64, 1000, 0, 1, 1, 0) != SH_OK || pre(0, 1, 2, 2, 4096, 64, 1000, 0, 1, 1, 0) != SH_ERR_ARG || pre(1, 0, 2, 2, 4096, 64, 1000, 0, 0, 0, 0) != SH_ERR_ARG ||
      pre(1, 1, 4, 2, 4096, 64, 1000, 0, 0, 0, 0) != SH_ERR_ARG || !strstr(text, "options") || pre(1, 1, 2, 3, 4096, 64, 1000, 0, 1, 1, 0) != SH_ERR_ARG ||
      pre(1, 1, 2, 2, 2, 64, 1000, 0, 1, 1, 0) != SH_ERR_ARG || pre(1, 1, 2, 2, 4096, 0, 1000, 0, 1, 1, 0) != SH_ERR_ARG || pre(1, 1, 2, 2, 4096, 64, 0, 0, 1, 1, 0) != SH_ERR_ARG ||
      pre(1, 1, 2, 2, 4096, 64, 1000, 1, 1, 1, 0) != SH_ERR_ARG || pre(1, 1, 2, 2, 4096, 64, 1000, 0, 1, 0, 0) != SH_ERR_STATE || pre(1, 1, 2, 2, 4096, 64, 1000, 0, 1, 1, 1) != SH_ERR_STATE ||
      pre(1, 1, 2, 2, 4096, 64, 1000, 0, 0, 1, 0) != SH_ERR_STATE || !strstr(text, "sh_mesh_topology")) {
    printf("repair_check: precheck_repair (%s)\n", text); return 1;
  }
  printf("repair_check: ok\n");
  return 0;
}
