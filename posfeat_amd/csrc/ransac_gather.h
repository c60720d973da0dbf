// ransac_gather.h -- the first launch of posfeat_ransac_homography (ransac.hip)
// and posfeat_ransac_fundamental (fundamental.hip), and the small device
// helpers both files use: the gather of the matched keypoints into compact
// rows with the two normalisations, the fixed-order block reduction, the
// clamped match count.  Include it inside the file's anonymous namespace,
// after common.h and ransac_plan.h; each file gets its own copy of the kernel.

#pragma clang fp contract(off)

struct Norm {
  double cx1, cy1, s1, cx2, cy2, s2;
};

// fixed-order tree over the 256 threads; every thread gets the result
template <class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* red, Op op) {
  const int tid = threadIdx.x;
  __syncthreads();  // red may still be read from the call before
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = RBLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = op(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}
struct OpAdd {
  template <class T>
  __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
  template <class T>
  __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};

__device__ __forceinline__ int pair_count(const int* __restrict__ counts, int p, const Pair& q) {
  return max(0, min(counts[p], q.n1));
}

__global__ __launch_bounds__(256) void ransac_gather_kernel(const float* __restrict__ kp,
                                                            const Pair* __restrict__ tab,
                                                            const int* __restrict__ matches,
                                                            const int* __restrict__ counts,
                                                            float4* __restrict__ pts,
                                                            double* __restrict__ norm) {
  __shared__ double red[RBLOCK];
  __shared__ int ired[RBLOCK];
  const int p = blockIdx.x, tid = threadIdx.x;
  const Pair q = tab[p];
  const int n = pair_count(counts, p, q);
  if (n == 0) return;
  const int* mp = matches + 2 * (long long)q.moff;
  float4* op = pts + q.moff;
  double sx1 = 0, sy1 = 0, sx2 = 0, sy2 = 0;
  int nv = 0;
  for (int i = tid; i < n; i += RBLOCK) {
    const int ia = mp[2 * i], ib = mp[2 * i + 1];
    // a match outside its sets is kept as a NaN row: never sampled into a
    // hypothesis that survives, never an inlier, not part of the normalisation
    float4 m = make_float4(NAN, NAN, NAN, NAN);
    if ((unsigned)ia < (unsigned)q.n1 && (unsigned)ib < (unsigned)q.n2) {
      const float* pa = kp + 2 * ((long long)q.a_off + ia);
      const float* pb = kp + 2 * ((long long)q.b_off + ib);
      m = make_float4(pa[0], pa[1], pb[0], pb[1]);
      sx1 += (double)m.x, sy1 += (double)m.y, sx2 += (double)m.z, sy2 += (double)m.w;
      ++nv;
    }
    op[i] = m;
  }
  const double cnt = (double)block_reduce(nv, ired, OpAdd());
  Norm nm;
  nm.cx1 = block_reduce(sx1, red, OpAdd()) / cnt;
  nm.cy1 = block_reduce(sy1, red, OpAdd()) / cnt;
  nm.cx2 = block_reduce(sx2, red, OpAdd()) / cnt;
  nm.cy2 = block_reduce(sy2, red, OpAdd()) / cnt;
  double d1 = 0, d2 = 0;
  for (int i = tid; i < n; i += RBLOCK) {
    const float4 m = op[i];  // this thread's own rows
    if (m.x != m.x) continue;
    const double ax = (double)m.x - nm.cx1, ay = (double)m.y - nm.cy1;
    const double bx = (double)m.z - nm.cx2, by = (double)m.w - nm.cy2;
    d1 += sqrt(ax * ax + ay * ay);
    d2 += sqrt(bx * bx + by * by);
  }
  nm.s1 = sqrt(2.0) / (block_reduce(d1, red, OpAdd()) / cnt);
  nm.s2 = sqrt(2.0) / (block_reduce(d2, red, OpAdd()) / cnt);
  if (tid == 0) {
    double* o = norm + 8 * (long long)p;
    o[0] = nm.cx1, o[1] = nm.cy1, o[2] = nm.s1, o[3] = nm.cx2, o[4] = nm.cy2, o[5] = nm.s2;
    o[6] = 0.0, o[7] = 0.0;
  }
}

__device__ __forceinline__ Norm load_norm(const double* __restrict__ norm, int p) {
  const double* o = norm + 8 * (long long)p;
  return Norm{o[0], o[1], o[2], o[3], o[4], o[5]};
}
