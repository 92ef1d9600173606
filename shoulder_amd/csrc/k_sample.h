// k_sample.h -- surface samples of the resident batch (include/shoulder_hip.h sh_sample_surface): N area-weighted points on every
// humerus and, with a radius, their greedy thinning to a minimum spacing.
//   k_samp_scan   (block of SH_SAMPLE_BLOCK = 256 faces, humerus), 256 lanes.  Each lane forms A2 of its face (sh_scalar.h samp_area2),
//                 then LANE 0 ALONE adds the block up in index order (samp_scan_block) and the lanes store the block's running sums to
//                 "samp.cdf" and its last one to "samp.base".
//   k_samp_base   (humerus), 256 lanes.  LANE 0 ALONE turns the block sums into the bases base_0 = 0.0, base_(k+1) = base_k + s_k[255],
//                 in block order, and writes the humerus' sh_sample_info and the count of round 0; then the lanes add base_k to the
//                 running sums of block k.
//                 THE TWO SCANS ARE SEQUENTIAL ON PURPOSE: a few hundred dependent additions in one lane per block and one lane per
//                 humerus, once per call and far off the hot path.  The order is the definition (it makes "samp.cdf" non-decreasing in
//                 floating point, which the search of k_samp_draw needs); a tree or a Hillis-Steele scan gives other bytes and no such
//                 guarantee.  Do not "optimise" them.
//   k_samp_draw   (chunk of SH_SAMP_CHUNK = 256 samples, humerus).  A lane makes the three words of its sample, searches "samp.cdf"
//                 (samp_search) and stores the record (samp_point); with a radius also the sample's first state.
//   k_samp_thin   (chunk, humerus), once per round.  THE HOT PATH.  A workgroup whose humerus has nothing undecided at the start of
//                 the round (word `round` of the humerus' head in "samp.state") returns at once, one whose own chunk has nothing
//                 undecided copies its states and returns.  Otherwise the candidates i < j pass through LDS in tiles of 256 x (point,
//                 state); every lane reads the same candidate at a time (one address: an LDS broadcast, no bank conflict), a removed
//                 candidate costs no distance, a lane stops at its first kept neighbour, a wave whose lanes are all decided skips the
//                 tile (its EXEC is empty) and the workgroup leaves the tiles once all its lanes are.  The states read are those of the
//                 start of the round, the states written go to the other array (Jacobi), and the samples still undecided are counted
//                 into word `round + 1` with one integer atomic per workgroup.
//   k_samp_finish (humerus), 256 lanes: the rounds used (the first word of the head that is 0), keep of every record from the final
//                 states, kept, and SH_ERR_CAPACITY when max_rounds did not decide every sample.
// No floating-point atomics; no record depends on B, N, the grid or the humerus' place.
#pragma once
#include "sh_scalar.h"

#include <cstddef>

namespace sh {

#define SH_SAMP_CHUNK 256      // samples of a workgroup of k_samp_draw / k_samp_thin, and candidates of an LDS tile
#define SH_SAMP_HEAD 64        // int32 in front of a humerus' states in "samp.state": word r the undecided at the start of round r
#define SH_SAMP_SEED_WORD 62   // ... and words 62, 63 the humerus' seed

static_assert(SH_SAMPLE_BLOCK == 256 && SH_SAMP_CHUNK == 256, "k_samp_*: one face, one sample, one candidate per lane of a 256-lane workgroup");
static_assert(SH_THIN_MAX_ROUNDS + 1 <= SH_SAMP_SEED_WORD && SH_SAMP_SEED_WORD + 2 == SH_SAMP_HEAD && SH_SAMP_HEAD % 2 == 0, "samp.state: the head of a humerus");
static_assert(sizeof(sh_sample) == 48 && offsetof(sh_sample, u) == 24 && offsetof(sh_sample, face) == 40 && offsetof(sh_sample, keep) == 44, "sh_sample");
static_assert(sizeof(sh_sample_info) == 24 && offsetof(sh_sample_info, kept) == 8 && offsetof(sh_sample_info, status) == 16, "sh_sample_info");
static_assert(sizeof(sh_sample_options) == 16, "sh_sample_options");

// the widened corners of face fi of the humerus whose vertices start at vb and whose faces start at fb
__device__ inline void samp_corners(const float* vb, const int* fb, long long fi, double* A, double* B, double* C) {
  const int* f = fb + 3 * fi;
  const float *v0 = vb + 3 * (size_t)f[0], *v1 = vb + 3 * (size_t)f[1], *v2 = vb + 3 * (size_t)f[2];
  for (int k = 0; k < 3; ++k) { A[k] = (double)v0[k]; B[k] = (double)v1[k]; C[k] = (double)v2[k]; }
}

__global__ void __launch_bounds__(SH_SAMPLE_BLOCK)
k_samp_scan(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
            double* __restrict__ cdf /* faces of the batch */, double* __restrict__ base /* B x gridDim.x */) {
  __shared__ double s[SH_SAMPLE_BLOCK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b], f0 = (long long)blockIdx.x * SH_SAMPLE_BLOCK;
  if (f0 >= nf) return;      // (uniform in the workgroup)
  const long long fi = f0 + tid;
  double a2 = 0.0;
  if (fi < nf) {
    double A[3], B[3], C[3];
    samp_corners(verts + 3 * voff[b], faces + 3 * foff[b], fi, A, B, C);
    a2 = samp_area2(A, B, C);
  }
  s[tid] = a2;
  __syncthreads();
  if (tid == 0) {
    const int n = nf - f0 < SH_SAMPLE_BLOCK ? (int)(nf - f0) : SH_SAMPLE_BLOCK;
    samp_scan_block(s, n);
    base[(size_t)b * gridDim.x + blockIdx.x] = s[n - 1];
  }
  __syncthreads();
  if (fi < nf) cdf[foff[b] + fi] = s[tid];
}

__global__ void __launch_bounds__(256)
k_samp_base(const long long* __restrict__ foff, int blocks /* per humerus in base */, int N, int thin, double* __restrict__ base, double* __restrict__ cdf,
            sh_sample_info* __restrict__ info /* B */, int* __restrict__ state, int stride) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long nf = foff[b + 1] - foff[b];
  double* bs = base + (size_t)b * blocks;
  if (tid == 0) {
    const long long nblk = (nf + SH_SAMPLE_BLOCK - 1) / SH_SAMPLE_BLOCK;
    double run = 0.0;
    for (long long k = 0; k < nblk; ++k) { const double t = bs[k]; bs[k] = run; run = run + t; }      // run ends as cdf[nf - 1]
    const bool ok = nf > 0 && run != 0.0 && icp_finite(run);
    sh_sample_info r;
    r.area = ok ? run / 2.0 : 0.0; r.kept = ok && !thin ? N : 0; r.rounds = 0; r.status = ok ? 0 : SH_ERR_GEOMETRY_DEV; r.reserved = 0;
    info[b] = r;
    state[(size_t)b * stride] = ok && thin ? N : 0;
  }
  __syncthreads();
  double* cd = cdf + foff[b];
  for (long long f = tid; f < nf; f += 256) cd[f] = bs[f / SH_SAMPLE_BLOCK] + cd[f];
}

__global__ void __launch_bounds__(SH_SAMP_CHUNK)
k_samp_draw(const float* __restrict__ verts, const int* __restrict__ faces, const long long* __restrict__ voff, const long long* __restrict__ foff,
            const double* __restrict__ cdf, const sh_sample_info* __restrict__ info, int N, int thin, sh_sample* __restrict__ out /* B x N */,
            int* __restrict__ state, int stride) {
  const int b = blockIdx.y;
  const long long j = (long long)blockIdx.x * SH_SAMP_CHUNK + threadIdx.x;
  if (j >= N) return;
  int* head = state + (size_t)b * stride;
  double rec[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int face = 0, keep = 0;
  if (info[b].status == 0) {
    const unsigned long long seed = *(const unsigned long long*)(head + SH_SAMP_SEED_WORD);
    const long long nf = foff[b + 1] - foff[b];
    const double* cd = cdf + foff[b];
    const double target = samp_unit(samp_word(seed, 3ull * (unsigned long long)j)) * cd[nf - 1];
    const long long fi = samp_search(cd, nf, target);
    double A[3], B[3], C[3];
    samp_corners(verts + 3 * voff[b], faces + 3 * foff[b], fi, A, B, C);
    samp_point(A, B, C, samp_unit(samp_word(seed, 3ull * (unsigned long long)j + 1ull)), samp_unit(samp_word(seed, 3ull * (unsigned long long)j + 2ull)), rec);
    face = (int)fi;
    keep = thin ? SH_SAMP_UNDECIDED : SH_SAMP_KEPT;
  }
  sh_sample r;
  r.point[0] = rec[0]; r.point[1] = rec[1]; r.point[2] = rec[2]; r.u = rec[3]; r.v = rec[4]; r.face = face; r.keep = keep;
  out[(size_t)b * N + j] = r;
  if (thin) head[SH_SAMP_HEAD + j] = keep;      // (round 0 reads the first of the two arrays)
}

__global__ void __launch_bounds__(SH_SAMP_CHUNK)
k_samp_thin(const sh_sample* __restrict__ out /* B x N */, int N, double r2, int round, int* __restrict__ state, int stride) {
  __shared__ double tp[3][SH_SAMP_CHUNK];
  __shared__ int ts[SH_SAMP_CHUNK];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  int* head = state + (size_t)b * stride;
  if (head[round] == 0) return;      // nothing undecided on this humerus (uniform in the workgroup; written by the launch before this one)
  const int* in = head + SH_SAMP_HEAD + (size_t)(round & 1) * N;
  int* nxt = head + SH_SAMP_HEAD + (size_t)((round + 1) & 1) * N;
  const sh_sample* rec = out + (size_t)b * N;
  const int j = c * SH_SAMP_CHUNK + tid;
  const bool valid = j < N;
  const int st = valid ? in[j] : SH_SAMP_REMOVED;
  const bool und = st == SH_SAMP_UNDECIDED;
  if (!__syncthreads_or(und ? 1 : 0)) {      // this chunk is decided: its states go to the other array as they are
    if (valid) nxt[j] = st;
    return;
  }
  double p[3] = {0.0, 0.0, 0.0};
  if (valid) { p[0] = rec[j].point[0]; p[1] = rec[j].point[1]; p[2] = rec[j].point[2]; }
  int flags = 0;
  for (int t = 0; t <= c; ++t) {
    const int i = t * SH_SAMP_CHUNK + tid;      // (i < N for t < c; the last tile is the chunk's own)
    const bool there = i < N;
    tp[0][tid] = there ? rec[i].point[0] : 0.0; tp[1][tid] = there ? rec[i].point[1] : 0.0; tp[2][tid] = there ? rec[i].point[2] : 0.0;
    ts[tid] = there ? in[i] : SH_SAMP_REMOVED;
    __syncthreads();
    if (und && !(flags & 1)) {
      const int lim = j - t * SH_SAMP_CHUNK < SH_SAMP_CHUNK ? j - t * SH_SAMP_CHUNK : SH_SAMP_CHUNK;      // the candidates i < j of this tile
      for (int k = 0; k < lim; ++k) {
        const int sk = ts[k];
        if (sk == SH_SAMP_REMOVED) continue;
        const double q[3] = {tp[0][k], tp[1][k], tp[2][k]};
        flags = samp_thin_see(flags, sk, samp_d2(p, q), r2);
        if (flags & 1) break;
      }
    }
    if (__syncthreads_and(!und || (flags & 1) ? 1 : 0)) break;      // (the barrier in front of the next tile's stores, too)
  }
  const int ns = und ? samp_thin_verdict(flags) : st;
  if (valid) nxt[j] = ns;
  const int left = __syncthreads_count(ns == SH_SAMP_UNDECIDED ? 1 : 0);
  if (tid == 0 && left) atomicAdd(head + round + 1, left);
}

__global__ void __launch_bounds__(256)
k_samp_finish(int N, int max_rounds, const int* __restrict__ state, int stride, sh_sample* __restrict__ out /* B x N */, sh_sample_info* __restrict__ info /* B */) {
  __shared__ int kept;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (info[b].status != 0) return;      // (no area: the records are zero; uniform in the workgroup)
  const int* head = state + (size_t)b * stride;
  int rounds = max_rounds, full = 1;
  for (int r = 0; r <= max_rounds; ++r)
    if (head[r] == 0) { rounds = r; full = 0; break; }
  const int* fin = head + SH_SAMP_HEAD + (size_t)(rounds & 1) * N;      // launch r wrote array (r + 1) & 1; the launches behind `rounds` returned at once
  if (tid == 0) kept = 0;
  __syncthreads();
  int mine = 0;
  for (int j = tid; j < N; j += 256) {
    const int st = fin[j];
    out[(size_t)b * N + j].keep = st;
    mine += st == SH_SAMP_KEPT ? 1 : 0;
  }
  if (mine) atomicAdd(&kept, mine);
  __syncthreads();
  if (tid == 0) { info[b].kept = kept; info[b].rounds = rounds; info[b].status = full ? SH_ERR_CAPACITY_DEV : 0; }
}

}  // namespace sh
