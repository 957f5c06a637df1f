// Grouped binomial score sketch: the one pass behind the fairness tables.
//
// Reference: hex/ModelMetricsBinomial.java + hex/AUC2.java built once per
// intersection of protected levels on a filtered frame
// (water/rapids/ast/prims/models/AstFairnessMetrics.java).  Here every row is
// read once, wherever its group lies: per (group, class, logit bin) a row
// count, per group the confusion matrix at the labelling threshold and the
// logloss / squared-error sums.  No row is compacted and no per-group frame
// exists.
//
// MI355X design.  The counts are integers (fairness tables count rows, every
// row weighs 1), so the atomics are exact and the result does not depend on
// arrival order; only the two f64 loss sums do.  A big group under an early
// boosting model puts millions of rows on a few (group, class, bin) cells, so
// each wave merges before it adds: the lowest pending lane's key is broadcast,
// the lanes that share it are balloted and one lane adds the popcount (up to
// FS_PEEL rounds, which covers the few-key case completely; lanes still
// pending after that hold rare keys and add 1 on their own).  The per-group
// cells (4 counts + 2 sums) are merged the same way by group and, for up to
// FS_LDS_GROUPS groups, accumulate in LDS and reach HBM once per block.
// The row filter is applied before any key is formed: a row with a NaN
// score, a response code other than 0 / 1 or a group outside the launch's
// range touches no memory.
#include "common.h"

#define FS_LIM 40.0
#define FS_LDS_GROUPS 512
#define FS_PEEL 8

// the binning of metrics.hip's mh_bin (models/metrics.py _logit_bins)
__device__ __forceinline__ int fs_bin(double p, int nb) {
  double x = log(fmax(p, 1e-300)) - log1p(-fmin(p, 1.0 - 1e-16));
  x = fmin(fmax(x, -FS_LIM), FS_LIM);
  long long b = (long long)((x + FS_LIM) * ((double)nb / (2.0 * FS_LIM)));
  return (int)(b < 0 ? 0 : (b > nb - 1 ? nb - 1 : b));
}

template <bool LDS>
__device__ __forceinline__ void fs_add(long long* p, long long v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ void fs_add(double* p, double v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
}

// cnt [Gc, 2, nb]: rows per (group - g0, y', bin of p'); cm [Gc, 4]: tp, fp,
// tn, fn with the favourable class positive; sums [Gc, 2]: sum of logloss,
// sum of squared error.  With flip the favourable class is code 0:
// y' = 1 - y, p' = 1 - p, selected' = !(p >= thr).
template <typename T, bool LDS>
__global__ __launch_bounds__(256) void group_sketch_kernel(const T* __restrict__ p, const int* __restrict__ y,
                                                           const int* __restrict__ g, long long n, int nb, int g0,
                                                           int Gc, double thr, int flip, long long* __restrict__ cnt,
                                                           long long* __restrict__ cm, double* __restrict__ sums) {
  __shared__ long long lcm[LDS ? 4 * FS_LDS_GROUPS : 1];
  __shared__ double lsum[LDS ? 2 * FS_LDS_GROUPS : 1];
  const int lane = lane_id();
  if (LDS) {
    for (int j = threadIdx.x; j < 4 * Gc; j += blockDim.x) lcm[j] = 0;
    for (int j = threadIdx.x; j < 2 * Gc; j += blockDim.x) lsum[j] = 0.0;
    __syncthreads();
  }
  long long* dcm = LDS ? lcm : cm;
  double* dsum = LDS ? lsum : sums;
  const long long stride = (long long)gridDim.x * blockDim.x;
  // the loop bound is uniform over the block, so every lane takes part in
  // the ballots below
  for (long long base = (long long)blockIdx.x * blockDim.x; base < n; base += stride) {
    const long long i = base + threadIdx.x;
    bool v = false;
    long long key = -1;
    int gl = -1, cell = 0;
    double ll = 0.0, se = 0.0;
    if (i < n) {
      const T pr = p[i];
      const int yi = y[i], gi = g[i];
      if (!isnan(pr) && (yi == 0 || yi == 1) && gi >= g0 && gi - g0 < Gc) {
        v = true;
        gl = gi - g0;
        const bool sel = ((double)pr >= thr) != (flip != 0);
        const int yy = flip ? 1 - yi : yi;
        const double pp = flip ? 1.0 - (double)pr : (double)pr;
        const double pc = fmin(fmax(pp, 1e-15), 1.0 - 1e-15);
        ll = -(yy ? log(pc) : log(1.0 - pc));
        se = ((double)yy - pp) * ((double)yy - pp);
        cell = yy ? (sel ? 0 : 3) : (sel ? 1 : 2);
        key = ((long long)gl * 2 + yy) * nb + fs_bin(pp, nb);
      }
    }
    // (group, class, bin) counts
    bool pend = v;
    unsigned long long act = __ballot(pend);
    for (int r = 0; r < FS_PEEL && act; ++r) {
      const int leader = __ffsll((long long)act) - 1;
      const long long lk = __shfl(key, leader, H2O_WAVE);
      const bool m = pend && key == lk;
      const unsigned long long mm = __ballot(m);
      if (lane == leader) fs_add<false>(&cnt[lk], (long long)__popcll(mm));
      if (m) pend = false;
      act &= ~mm;
    }
    if (pend) fs_add<false>(&cnt[key], 1LL);
    // per-group cells
    pend = v;
    act = __ballot(pend);
    for (int r = 0; r < FS_PEEL && act; ++r) {
      const int leader = __ffsll((long long)act) - 1;
      const int lg = __shfl(gl, leader, H2O_WAVE);
      const bool m = pend && gl == lg;
      const unsigned long long mm = __ballot(m);
      const int c0 = __popcll(__ballot(m && cell == 0));
      const int c1 = __popcll(__ballot(m && cell == 1));
      const int c2 = __popcll(__ballot(m && cell == 2));
      const int c3 = __popcll(__ballot(m && cell == 3));
      const double sl = wave_sum(m ? ll : 0.0);
      const double ss = wave_sum(m ? se : 0.0);
      if (lane == leader) {
        if (c0) fs_add<LDS>(&dcm[4 * lg + 0], (long long)c0);
        if (c1) fs_add<LDS>(&dcm[4 * lg + 1], (long long)c1);
        if (c2) fs_add<LDS>(&dcm[4 * lg + 2], (long long)c2);
        if (c3) fs_add<LDS>(&dcm[4 * lg + 3], (long long)c3);
        fs_add<LDS>(&dsum[2 * lg + 0], sl);
        fs_add<LDS>(&dsum[2 * lg + 1], ss);
      }
      if (m) pend = false;
      act &= ~mm;
    }
    if (pend) {
      fs_add<LDS>(&dcm[4 * gl + cell], 1LL);
      fs_add<LDS>(&dsum[2 * gl + 0], ll);
      fs_add<LDS>(&dsum[2 * gl + 1], se);
    }
  }
  if (LDS) {
    __syncthreads();
    for (int j = threadIdx.x; j < 4 * Gc; j += blockDim.x)
      if (lcm[j] != 0) fs_add<false>(&cm[j], lcm[j]);
    for (int j = threadIdx.x; j < 2 * Gc; j += blockDim.x)
      if (lsum[j] != 0.0) fs_add<false>(&sums[j], lsum[j]);
  }
}

template <typename T>
static int fs_launch(const T* p, const int* y, const int* g, long long n, int nb, int g0, int Gc, double thr, int flip,
                     long long* cnt, long long* cm, double* sums, int max_blocks, hipStream_t s) {
  const bool lds = Gc <= FS_LDS_GROUPS;
  long long blocks = (n + 255) / 256;
  // LDS mode flushes up to 6 Gc atomics per block: fewer, fuller blocks
  const long long cap = lds ? 1024 : 4096;
  if (blocks > cap) blocks = cap;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  if (lds)
    hipLaunchKernelGGL((group_sketch_kernel<T, true>), dim3((unsigned)blocks), dim3(256), 0, s, p, y, g, n, nb, g0, Gc,
                       thr, flip, cnt, cm, sums);
  else
    hipLaunchKernelGGL((group_sketch_kernel<T, false>), dim3((unsigned)blocks), dim3(256), 0, s, p, y, g, n, nb, g0,
                       Gc, thr, flip, cnt, cm, sums);
  return (int)hipGetLastError();
}

extern "C" {

int h2o_fairness_lds_groups() { return FS_LDS_GROUPS; }

// p: f32 or f64 [n] (p_f64); y, g: i32 [n]; groups [g0, g0 + Gc) are counted.
// cnt: i64 [Gc, 2, nb], cm: i64 [Gc, 4], sums: f64 [Gc, 2], the slices of
// this range of groups, zeroed by the caller (they accumulate).  max_blocks
// <= 0: the default cap.
int h2o_group_sketch(const void* p, int p_f64, const int* y, const int* g, long long n, int nb, int g0, int Gc,
                     double thr, int flip, long long* cnt, long long* cm, double* sums, int max_blocks,
                     hipStream_t s) {
  if (n <= 0 || Gc <= 0) return 0;
  if (nb <= 0 || g0 < 0) return -1;
  if (p_f64)
    return fs_launch<double>((const double*)p, y, g, n, nb, g0, Gc, thr, flip ? 1 : 0, cnt, cm, sums, max_blocks, s);
  return fs_launch<float>((const float*)p, y, g, n, nb, g0, Gc, thr, flip ? 1 : 0, cnt, cm, sums, max_blocks, s);
}

}  // extern "C"
