// match_tile.h -- the device code match.hip (one pair per call) and
// matchpairs.hip (a whole pair list per call) share: one tile of the fused
// fp32-MFMA similarity + top-2 pass, the partial merge and the Lowe ratio.
// Everything here is __forceinline__: both kernels contain the same
// instruction sequence and no device-function call (tools/isa_check.py).
#pragma once
#include <cmath>

#include "common.h"
#include "guided_solve.h"

namespace pfmatch {

constexpr int MD = 128;       // descriptor dimension
constexpr int MCOLS = 128;    // B rows (columns of sim) per block: 4 waves x 32
constexpr int MSTEP = 64;     // A rows per LDS step (2 x 32-row MFMA blocks)

struct Top2 {
  float v1;
  int i1;
  float v2;
};

// merge two partial top-2 sets (value descending, index ascending)
__device__ __forceinline__ Top2 top2_merge(const Top2& a, const Top2& b) {
  const bool a_first = a.v1 > b.v1 || (a.v1 == b.v1 && a.i1 < b.i1);
  const Top2& f = a_first ? a : b;
  const Top2& s = a_first ? b : a;
  return Top2{f.v1, f.i1, fmaxf(f.v2, s.v1)};
}

// One tile, run by a 256-thread workgroup: for B row `col` (this lane's column
// of sim; columns >= nb read row nb - 1 and are dropped by the caller), the
// top-2 of <A_i, B_col> over the A rows i in [r0, r1), indices relative to A.
// As: 2 x MSTEP x MD floats of LDS, 16-B aligned.  The result is valid in the
// lanes with (lane >> 5) == 0.  Each similarity is one K = 128 fmaf chain in a
// fixed k order, so its bits do not depend on [r0, r1).
//
// GUIDE (compile time): GUIDE_NONE is the plain tile.  GUIDE_H / GUIDE_F fold
// only the rows guided_solve.h admits for this column under a homography / a
// fundamental matrix (posfeat_match_pairs_guided): arec[i] is the record of A
// row i, Rs 2 x MSTEP records of LDS beside As, (cx, cy, cw) the column's data
// and t2 the squared threshold.  The records of a step travel with its
// descriptors (one more 1 KB DMA by wave 0); the fold reads a row's record at
// one address per lane half, a broadcast.  An inadmissible entry takes -inf,
// as a row past r1 does; nothing before the fold differs.
struct GuideCol {
  float cx, cy, cw, t2;
};
constexpr int GUIDE_NONE = -1, GUIDE_H = pfguided::HOMOGRAPHY, GUIDE_F = pfguided::FUNDAMENTAL;

template <int GUIDE>
__device__ __forceinline__ Top2 match_tile_top2_g(const float* __restrict__ A, int r0, int r1,
                                                  const float* __restrict__ B, int nb, int col,
                                                  float* As, const f32x4* __restrict__ arec,
                                                  float* Rs, const GuideCol& gc) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5;
  // this wave's B fragments: lane half h supplies k = 8g + 4h + j for MFMA j
  f32x4 breg[MD / 8];
  {
    const float* brow = B + (long long)min(col, nb - 1) * MD;
#pragma unroll
    for (int g = 0; g < MD / 8; ++g) breg[g] = *reinterpret_cast<const f32x4*>(brow + 8 * g + 4 * h);
  }
  const int nsteps = (r1 - r0 + MSTEP - 1) / MSTEP;
  // DMA of step s into stage `buf`: wave-instruction t covers rows 2t, 2t+1
  // of the step (lane L: row 2t + L/32, physical slot L%32 holding logical
  // slot (L%32) ^ (row & 15)); rows past r1 re-read row r1 - 1 (masked later)
  auto issue = [&](int s, int buf) {
#pragma unroll
    for (int t = 0; t < MSTEP / 2 / 4; ++t) {
      const int lr = (wave * (MSTEP / 8) + t) * 2 + h;
      const int row = min(r0 + s * MSTEP + lr, r1 - 1);
      const int slot = (lane & 31) ^ (lr & 15);
      const float* src = A + (long long)row * MD + slot * 4;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)(As + buf * MSTEP * MD +
                                                     (wave * (MSTEP / 8) + t) * 2 * MD),
          16, 0, 0);
    }
    if constexpr (GUIDE != GUIDE_NONE) {
      if (wave == 0) {  // lane L: the record of row L of the step
        const int row = min(r0 + s * MSTEP + lane, r1 - 1);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(arec + row),
            (__attribute__((address_space(3))) void*)(Rs + buf * MSTEP * 4), 16, 0, 0);
      }
    }
  };
  Top2 best{-INFINITY, 0x7fffffff, -INFINITY};
  if (nsteps > 0) issue(0, 0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    const int cur = s & 1;
    if (s + 1 < nsteps) issue(s + 1, cur ^ 1);
    const float* Ab = As + cur * MSTEP * MD;
    // both 32-row blocks at once: two independent accumulation chains
    f32x16 accs[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) accs[0][r] = accs[1][r] = 0.f;
    {
      const int la = lane & 31;  // rows la and 32 + la share the swizzle (la & 15)
      const float* arow0 = Ab + la * MD;
      const float* arow1 = Ab + (32 + la) * MD;
#pragma unroll
      for (int g = 0; g < MD / 8; ++g) {
        const int off = ((2 * g + h) ^ (la & 15)) * 4;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(arow0 + off);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(arow1 + off);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          accs[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], breg[g][j], accs[0], 0, 0, 0);
          accs[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], breg[g][j], accs[1], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const f32x16& acc = accs[mi];
      // acc[r] = sim(A row i, B row col), i = step base + mi*32 + (r&3) + 8(r>>2) + 4h:
      // increasing in r, so strict '>' keeps the first index on ties
      const int ib = r0 + s * MSTEP + mi * 32 + 4 * h;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = ib + (r & 3) + 8 * (r >> 2);
        bool ok = i < r1;
        if constexpr (GUIDE != GUIDE_NONE) {
          const f32x4 ra = *reinterpret_cast<const f32x4*>(
              Rs + (cur * MSTEP + mi * 32 + 4 * h + (r & 3) + 8 * (r >> 2)) * 4);
          ok = ok && pfguided::admissible<GUIDE>(ra[0], ra[1], ra[2], ra[3], gc.cx, gc.cy, gc.cw,
                                                 gc.t2);
        }
        const float v = ok ? acc[r] : -INFINITY;
        if (v > best.v1) {
          best.v2 = best.v1;
          best.v1 = v;
          best.i1 = i;
        } else if (v > best.v2) {
          best.v2 = v;
        }
      }
    }
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
  // the two lane halves of a column hold interleaved row sets: merge
  Top2 o;
  o.v1 = __shfl_xor(best.v1, 32, 64);
  o.i1 = __shfl_xor(best.i1, 32, 64);
  o.v2 = __shfl_xor(best.v2, 32, 64);
  return h == 0 ? top2_merge(best, o) : top2_merge(o, best);
}

__device__ __forceinline__ Top2 match_tile_top2(const float* __restrict__ A, int r0, int r1,
                                                const float* __restrict__ B, int nb, int col,
                                                float* As) {
  return match_tile_top2_g<GUIDE_NONE>(A, r0, r1, B, nb, col, As, nullptr, nullptr,
                                       GuideCol{0.f, 0.f, 0.f, 0.f});
}

// torch: sqrt(2 - 2 s) in fp32; ratio = d1 / (d2 + 1e-8)
__device__ __forceinline__ float lowe_ratio(float s1, float s2) {
  const float d1 = __fsqrt_rn(__fsub_rn(2.f, __fmul_rn(2.f, s1)));
  const float d2 = __fsqrt_rn(__fsub_rn(2.f, __fmul_rn(2.f, s2)));
  return __fdiv_rn(d1, __fadd_rn(d2, 1e-8f));
}

// The selection of one pair, run by a 1024-thread workgroup.  mode: 0 mutual
// NN, 1 symmetric ratio, 2 mutual NN + symmetric ratio.  Each thread owns a
// contiguous range of rows i, counts its matches, an exclusive scan in LDS
// (off: 1024 ints) gives its output offset (matches come out in ascending i,
// as the reference's boolean-mask indexing orders them).  GUARD (the guided
// call): a row whose best value is -inf had no admissible candidate and never
// matches, in any mode (the clamp below would let mode 0 emit it).
template <bool GUARD = false>
__device__ __forceinline__ void match_select_pair(
    const int* __restrict__ nn12, const float* __restrict__ r1a, const float* __restrict__ r1b,
    const int* __restrict__ nn21, const float* __restrict__ r2a, const float* __restrict__ r2b,
    int n1, int n2, int mode, float ratio, int* __restrict__ matches, int* __restrict__ count,
    int* off) {
  const int t = threadIdx.x, per = (n1 + 1023) / 1024;
  const int i0 = min(n1, t * per), i1 = min(n1, i0 + per);
  auto keep = [&](int i) {
    if constexpr (GUARD) {
      if (r1a[i] == -INFINITY) return false;
    }
    // a row of NaN similarities keeps the fold's initial index: stay in bounds
    const int j = min(nn12[i], n2 - 1);
    bool k = true;
    if (mode != 1) k = nn21[j] == i;
    if (mode != 0) {
      const float q12 = lowe_ratio(r1a[i], r1b[i]);
      const float q21 = lowe_ratio(r2a[j], r2b[j]);
      k = k && (q12 <= ratio) && (q21 <= ratio);  // NaN compares false, as in torch
    }
    return k;
  };
  int c = 0;
  for (int i = i0; i < i1; ++i) c += keep(i) ? 1 : 0;
  off[t] = c;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan
    const int v = t >= d ? off[t - d] : 0;
    __syncthreads();
    off[t] += v;
    __syncthreads();
  }
  int o = off[t] - c;
  for (int i = i0; i < i1; ++i)
    if (keep(i)) {
      matches[2 * o] = i;
      matches[2 * o + 1] = nn12[i];
      ++o;
    }
  if (t == 1023) *count = off[1023];
}

}  // namespace pfmatch
