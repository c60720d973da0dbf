// match.hip -- the evaluation matchers on gfx950.
//
// Replaces, for L2-normalised 128-d descriptors:
//   mnn_matcher              losses/preprocess_utils.py:795-803
//                            (= evaluations/hpatches/evaluation.py:28-38)
//   mutual_nn_matcher        evaluations/aachen/matchers.py:5-14
//                            (= evaluations/ETH_local_feature/custom_matcher.py:5-14)
//   ratio_matcher            evaluations/aachen/matchers.py:17-44
//   mutual_nn_ratio_matcher  evaluations/aachen/matchers.py:47-75
//
// All four need, per row of sim = d1 d2^T and per column, the arg-max and the
// top-2 similarities.  sim is never written: match_top2_kernel computes one
// side's statistics (for every row j of B: top-2 over the rows i of A of
// <A_i, B_j>) with fp32 MFMA and keeps them in registers; it runs twice, with
// (A, B) = (d1, d2) for the columns and (d2, d1) for the rows.  The k order of
// the fmaf chain is the same in both runs, so both read identical sim bits.
//
// Layout: each wave holds 32 B rows (its columns) as MFMA B fragments in 64
// VGPRs for the whole launch; A is streamed in 64-row steps through LDS by
// DMA (global_load_lds, XOR-swizzled 16-B slots: conflict-free ds_read_b128),
// two stages.  Per step each wave runs 2 x 64 v_mfma_f32_32x32x2_f32 and folds
// the 32 x 32 accumulators into a running (best value, best index, second
// value) per column lane -- in increasing row order with strict '>' updates,
// so the FIRST index wins an arg-max tie (the stated tie rule; the second
// value is the 2nd largest with multiplicity, as torch.topk(2) returns it).
// A rows are split over blockIdx.y so launches reach >= 512 workgroups; the
// split partials are merged in split order (deterministic).  The match
// kernel applies the reference's mask (mutual, ratio via sqrt(2 - 2 s) in
// fp32, or both) and compacts the matches in ascending first index.
#include <algorithm>
#include <cmath>

#include "match_tile.h"

namespace {

using namespace pfmatch;  // the tile loop, merge and selection shared with matchpairs.hip

__global__ __launch_bounds__(256) void match_top2_kernel(const float* __restrict__ A, int na,
                                                         const float* __restrict__ B, int nb,
                                                         int rows_per_split,
                                                         float* __restrict__ pv1,
                                                         int* __restrict__ pi1,
                                                         float* __restrict__ pv2) {
  __shared__ __attribute__((aligned(16))) float As[2 * MSTEP * MD];  // 2 x 32 KB
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * MCOLS + wave * 32 + (lane & 31);
  const int split = blockIdx.y;
  const int r0 = split * rows_per_split;
  const int r1 = min(na, r0 + rows_per_split);
  const Top2 best = match_tile_top2(A, r0, r1, B, nb, col, As);
  if ((lane >> 5) == 0 && col < nb) {
    const long long p = (long long)split * nb + col;
    pv1[p] = best.v1;
    pi1[p] = best.i1;
    pv2[p] = best.v2;
  }
}

// merge the split partials of each column in split order
__global__ void match_merge_kernel(const float* __restrict__ pv1, const int* __restrict__ pi1,
                                   const float* __restrict__ pv2, int nsplit, int nb,
                                   int* __restrict__ nn, float* __restrict__ v1,
                                   float* __restrict__ v2) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nb) return;
  Top2 t{pv1[c], pi1[c], pv2[c]};
  for (int s = 1; s < nsplit; ++s) {
    const long long p = (long long)s * nb + c;
    t = top2_merge(t, Top2{pv1[p], pi1[p], pv2[p]});
  }
  nn[c] = t.i1;
  v1[c] = t.v1;
  v2[c] = t.v2;
}

// one workgroup: match_select_pair (match_tile.h)
__global__ __launch_bounds__(1024) void match_select_kernel(
    const int* __restrict__ nn12, const float* __restrict__ r1a, const float* __restrict__ r1b,
    const int* __restrict__ nn21, const float* __restrict__ r2a, const float* __restrict__ r2b,
    int n1, int n2, int mode, float ratio, int* __restrict__ matches, int* __restrict__ count) {
  __shared__ int off[1024];
  match_select_pair(nn12, r1a, r1b, nn21, r2a, r2b, n1, n2, mode, ratio, matches, count, off);
}

// A-row split filling whole rounds of the 512 resident workgroups (2 per CU)
int nsplit_for(int na, int nb) {
  const int ncb = (nb + MCOLS - 1) / MCOLS;
  const int smax = std::max(1, std::min(32, (na + MSTEP - 1) / MSTEP));
  int best = 1;
  double best_eff = 0.0;
  for (int s = 1; s <= smax; ++s) {
    const double r = (double)ncb * s / 512.0;
    const double eff = r / std::ceil(r) * (r < 1.0 ? r : 1.0);
    if (eff >= 0.94) return s;  // the fewest splits that keep the tail small
    if (eff > best_eff + 1e-9) {
      best_eff = eff;
      best = s;
    }
  }
  return best;
}

size_t side_ws(int na, int nb) {  // partials (3 per column per split) + merged (3 per column)
  return pf_align((size_t)nsplit_for(na, nb) * nb * 12, 256) + pf_align((size_t)nb * 12, 256);
}

// per row j of B: (arg-max_i, top value, 2nd value) over the rows i of A
int top2_side(const float* A, int na, const float* B, int nb, char* ws, int* nn, float* v1,
              float* v2, hipStream_t st) {
  const int ns = nsplit_for(na, nb);
  const int rps = ((na + ns - 1) / ns + MSTEP - 1) / MSTEP * MSTEP;
  const int ns_eff = (na + rps - 1) / rps;
  float* pv1 = reinterpret_cast<float*>(ws);
  int* pi1 = reinterpret_cast<int*>(ws + (size_t)ns * nb * 4);
  float* pv2 = reinterpret_cast<float*>(ws + (size_t)ns * nb * 8);
  hipLaunchKernelGGL(match_top2_kernel, dim3((nb + MCOLS - 1) / MCOLS, ns_eff), dim3(256), 0, st,
                     A, na, B, nb, rps, pv1, pi1, pv2);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(match_merge_kernel, dim3((nb + 255) / 256), dim3(256), 0, st, pv1, pi1, pv2,
                     ns_eff, nb, nn, v1, v2);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}

}  // namespace

extern "C" size_t posfeat_match_workspace(int n1, int n2) {
  if (n1 <= 0 || n2 <= 0) return 0;
  return side_ws(n2, n1) + side_ws(n1, n2) + 256;
}

extern "C" int posfeat_match(const float* d1, int n1, const float* d2, int n2, int dim, int mode,
                             float ratio, int32_t* matches, int32_t* count, void* ws,
                             size_t ws_bytes, void* stream) {
  if (!d1 || !d2 || !matches || !count || !ws || n1 <= 0 || n2 <= 0) return POSFEAT_E_INVALID;
  if (dim != MD || mode < 0 || mode > 2) return POSFEAT_E_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(d1) & 15) || (reinterpret_cast<uintptr_t>(d2) & 15) ||
      (reinterpret_cast<uintptr_t>(ws) & 255))
    return POSFEAT_E_INVALID;
  if (ws_bytes < posfeat_match_workspace(n1, n2)) return POSFEAT_E_WORKSPACE;
  hipStream_t st = pf_stream(stream);
  char* w = static_cast<char*>(ws);
  // rows of sim: for each d1 row i, top-2 over d2 rows (A = d2, B = d1)
  char* rws = w;
  char* rout = rws + pf_align((size_t)nsplit_for(n2, n1) * n1 * 12, 256);
  int* nn12 = reinterpret_cast<int*>(rout);
  float* r1a = reinterpret_cast<float*>(rout + (size_t)n1 * 4);
  float* r1b = reinterpret_cast<float*>(rout + (size_t)n1 * 8);
  PF_TRY(top2_side(d2, n2, d1, n1, rws, nn12, r1a, r1b, st));
  // columns: for each d2 row j, top-2 over d1 rows (A = d1, B = d2)
  char* cws = w + side_ws(n2, n1);
  char* cout_ = cws + pf_align((size_t)nsplit_for(n1, n2) * n2 * 12, 256);
  int* nn21 = reinterpret_cast<int*>(cout_);
  float* r2a = reinterpret_cast<float*>(cout_ + (size_t)n2 * 4);
  float* r2b = reinterpret_cast<float*>(cout_ + (size_t)n2 * 8);
  PF_TRY(top2_side(d1, n1, d2, n2, cws, nn21, r2a, r2b, st));
  hipLaunchKernelGGL(match_select_kernel, dim3(1), dim3(1024), 0, st, nn12, r1a, r1b, nn21, r2a,
                     r2b, n1, n2, mode, ratio, matches, count);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}
