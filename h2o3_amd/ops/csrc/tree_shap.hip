// Baseline (interventional) SHAP of a tree ensemble against a background
// frame: predict_contributions(test, background_frame=bg).  Reference:
// hex/tree/SharedTreeModelWithContributions.java (ScoreContributionsWithBackground)
// and Laberge & Pequignot, "Understanding Interventional TreeSHAP".
//
// For a test row x, a background row z and a leaf, the root-to-leaf conditions
// are grouped by feature into m <= 32 path elements.  bit e of mx / mz says
// that x / z satisfies every condition of element e.  The leaf matters for the
// pair only when mx | mz is full; then with A = mx & ~mz (a bits) and
// B = mz & ~mx (b bits) every feature of A gets +v (a-1)! b! / (a+b)! and every
// feature of B gets -v a! (b-1)! / (a+b)!.
//
// Two stages, both recursion-free:
//   shap_mask_kernel  one thread per (row, leaf): evaluates the leaf's
//                     conditions with forest_predict_kernel's decision rule and
//                     stores the uint32 mask (and/or adds the leaf value to the
//                     row's score when every element holds);
//   shap_pair_kernel  lane = test row, wave = leaf slice, loop over background
//                     rows: mask algebra + two popcounts + a weight table.
//                     The background masks of a leaf are wave-uniform loads.
//                     Averaged mode sums each test row's F+1 values in LDS
//                     (f64) and adds the tile to the output once per block.
//
// Without a background frame (path-dependent TreeSHAP, node covers as the
// background distribution) the same masks feed shap_path_kernel, further down.
#include "common.h"

#define SHAP_WDIM 33            // weight table W[a][b], a, b in 0..32
#define SHAP_ROWS 64            // test rows per block of the pair kernel (one per lane)
#define SHAP_WAVES 4

// The decision of forest_predict_kernel (tree_predict.hip) for one node.
__device__ __forceinline__ bool shap_go_left(const int4 n, int nd, float x, const int* __restrict__ cat_off,
                                             const int* __restrict__ cat_len,
                                             const uint8_t* __restrict__ cat_bits) {
  const bool nal = (n.x >> 30) & 1;
  if (n.x < 0) {   // categorical: left-level bitset
    if (x != x) return nal;
    const int c = (int)x;
    return (c < 0 || c >= cat_len[nd]) ? nal : (cat_bits[cat_off[nd] + c] != 0);
  }
  return (x != x) ? nal : (x < __int_as_float(n.y));
}

__device__ __forceinline__ uint32_t shap_full(int k) { return k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u); }

// X: column-major tile, row r of feature f at X[f * ldx + r], r < R.
// mask: [l1 - l0, R] or null.  score: [R] f64 or null (+= vscale * leaf value
// of every leaf of class `cls` whose elements all hold).
__global__ __launch_bounds__(256) void shap_mask_kernel(
    const float* __restrict__ X, long long ldx, int R, const int4* __restrict__ nodes,
    const int* __restrict__ cat_off, const int* __restrict__ cat_len, const uint8_t* __restrict__ cat_bits,
    const int* __restrict__ el_off, const int* __restrict__ el_feat, const int* __restrict__ cond_off,
    const int* __restrict__ cond_node, const uint8_t* __restrict__ cond_left, const double* __restrict__ leaf_val,
    const int* __restrict__ leaf_cls, int cls, int l0, int l1, uint32_t* __restrict__ mask,
    double* __restrict__ score, double vscale) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  for (int l = l0 + (int)blockIdx.y; l < l1; l += (int)gridDim.y) {
    if (leaf_cls[l] != cls) continue;
    const int e0 = el_off[l], e1 = el_off[l + 1];
    uint32_t m = 0;
    for (int e = e0; e < e1; ++e) {
      const float x = X[(size_t)el_feat[e] * (size_t)ldx + r];
      bool ok = true;
      const int c1 = cond_off[e + 1];
      for (int c = cond_off[e]; c < c1; ++c) {
        const int nd = cond_node[c];
        ok &= shap_go_left(nodes[nd], nd, x, cat_off, cat_len, cat_bits) == (cond_left[c] != 0);
      }
      m |= (uint32_t)ok << (e - e0);
    }
    if (mask) mask[(size_t)(l - l0) * R + r] = m;
    if (score && m == shap_full(e1 - e0)) gbl_add(&score[r], vscale * leaf_val[l]);
  }
}

// MX: [l1 - l0, R] test masks, MZ: [l1 - l0, Bt] background masks.
// pscale: optional [R, Bt] per-pair factor.  out: averaged mode [*, F+1] sums
// over the background rows (row out_r0 + r); per-reference mode
// [*, Btot, F+1] (pair (out_r0 + r, b0 + b)).  Feature columns only: the
// bias column is the caller's.
template <bool PER_REF, bool USE_LDS>
__global__ __launch_bounds__(SHAP_ROWS * SHAP_WAVES) void shap_pair_kernel(
    const uint32_t* __restrict__ MX, int R, const uint32_t* __restrict__ MZ, int Bt,
    const int* __restrict__ el_off, const int* __restrict__ el_feat, const double* __restrict__ leaf_val,
    const int* __restrict__ leaf_cls, int cls, int l0, int l1, const double* __restrict__ W,
    const double* __restrict__ pscale, double vscale, double* __restrict__ out, long long out_r0, int b0,
    int Btot, int F) {
  extern __shared__ double shap_smem[];
  double* sW = shap_smem;                               // [33 * 33]
  double* acc = shap_smem + SHAP_WDIM * SHAP_WDIM;      // [64][stride], odd stride: lanes on distinct banks
  const int stride = (F + 1) | 1;
  for (int i = threadIdx.x; i < SHAP_WDIM * SHAP_WDIM; i += blockDim.x) sW[i] = W[i];
  if (USE_LDS && !PER_REF)
    for (int i = threadIdx.x; i < SHAP_ROWS * stride; i += blockDim.x) acc[i] = 0.0;
  __syncthreads();
  const int lane = threadIdx.x & (SHAP_ROWS - 1);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / SHAP_ROWS));
  const int r = blockIdx.x * SHAP_ROWS + lane;
  const bool live = r < R;
  double* dst0 = PER_REF ? nullptr
                         : (USE_LDS ? acc + lane * stride : out + (size_t)(out_r0 + r) * (size_t)(F + 1));
  for (int l = l0 + (int)blockIdx.y * SHAP_WAVES + w; l < l1; l += SHAP_WAVES * (int)gridDim.y) {
    if (leaf_cls[l] != cls) continue;
    const int e0 = el_off[l];
    const int k = el_off[l + 1] - e0;
    if (k == 0) continue;                               // single-leaf tree: constant, no contribution
    const uint32_t full = shap_full(k);
    const double v = leaf_val[l] * vscale;
    const uint32_t mx = live ? MX[(size_t)(l - l0) * R + r] : 0u;
    const uint32_t* __restrict__ mzrow = MZ + (size_t)(l - l0) * Bt;
    const int* __restrict__ feat = el_feat + e0;
    for (int b = 0; b < Bt; ++b) {
      const uint32_t mz = mzrow[b];
      if (!live || (mx | mz) != full) continue;
      uint32_t A = mx & ~mz, Bm = mz & ~mx;
      if (!(A | Bm)) continue;
      const int na = __popc(A), nb = __popc(Bm);
      const double s = pscale ? v * pscale[(size_t)r * Bt + b] : v;
      const double wa = s * sW[na * SHAP_WDIM + nb];
      const double wb = -s * sW[nb * SHAP_WDIM + na];
      double* dst = PER_REF ? out + ((size_t)(out_r0 + r) * (size_t)Btot + (size_t)(b0 + b)) * (size_t)(F + 1)
                            : dst0;
      while (A) {
        const int e = __ffs(A) - 1;
        A &= A - 1;
        if (USE_LDS && !PER_REF) __hip_atomic_fetch_add(dst + feat[e], wa, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_WORKGROUP);
        else gbl_add(dst + feat[e], wa);
      }
      while (Bm) {
        const int e = __ffs(Bm) - 1;
        Bm &= Bm - 1;
        if (USE_LDS && !PER_REF) __hip_atomic_fetch_add(dst + feat[e], wb, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_WORKGROUP);
        else gbl_add(dst + feat[e], wb);
      }
    }
  }
  if (USE_LDS && !PER_REF) {
    __syncthreads();
    const int n = SHAP_ROWS * (F + 1);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int rr = i / (F + 1), f = i - rr * (F + 1);
      const int gr = blockIdx.x * SHAP_ROWS + rr;
      const double a = acc[rr * stride + f];
      if (gr < R && a != 0.0) gbl_add(&out[(size_t)(out_r0 + gr) * (size_t)(F + 1) + f], a);
    }
  }
}

// ---------------------------------------------------------------------------
// Path-dependent TreeSHAP (predict_contributions without a background frame;
// Lundberg et al., Algorithm 2) in leaf-path form.  For a row and a leaf of
// value v with k path elements, element e has a one-fraction o_e in {0, 1}
// (bit e of the row's mask) and a zero-fraction z_e (product of the cover
// ratios of its conditions, el_zero).  The path weights of EXTEND are
//   w[i] = p[i] * i! (k-i)! / (k+1)!,   sum_i p[i] x^i = prod_e (z_e + o_e x),
// so EXTEND is a multiplication by (z + o x) without coefficients, UNWIND of
// element e is the division by (z_e + o_e x), and with
// c_k[i] = i! (k-1-i)! / k! (the table C) UNWOUND-SUM times (o_e - z_e) is
//   o_e = 1:  (1 - z_e) * sum_i c_k[i] q[i],  q = p / (z_e + x), from the top
//             coefficient down: q[i-1] = p[i] - z_e q[i]
//   o_e = 0:  -sum_i c_k[i] p[i]  (q = p / z_e and the factor -z_e cancel; if
//             z_e = 0 then p = 0) -- the same for every such element.
// The k+1 coefficients live in registers: every loop is unrolled to the padded
// width KK in {4, 8, 16, 32}, so no index is a run-time value (ScratchSize 0).
// The outer steps (one per element) sit behind wave-uniform guards (k is a
// property of the leaf, one leaf per wave); the inner ones are straight-line
// code over all KK coefficients, the ones past k being zero.  Guarding them
// too made every step a taken branch out and back: 59 against 46 ms for
// 100k rows x 100 depth-8 trees (profiles/shap_path_mb.txt).
#define SHAP_PMAX 32            // path elements a mask holds
#define SHAP_CDIM 32            // C[k * 32 + i], k in 0..32, i < k

// Element e's zero-fraction from lane e of zl: the leaf's elements are read by
// one vector load per leaf (lane e holds element e) and broadcast from there,
// instead of one scalar load, and its latency, per guarded step (46 -> 37 ms).
__device__ __forceinline__ double shap_lane_f64(double x, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane),
                          __builtin_amdgcn_readlane(__double2loint(x), lane));
}

template <int KK, bool USE_LDS>
__device__ __forceinline__ void shap_path_leaf(uint32_t mx, int k, double zl, int fl,
                                               const double* __restrict__ ck, double v, bool live,
                                               double* __restrict__ dst) {
  double p[KK + 1];
  p[0] = 1.0;
#pragma unroll
  for (int i = 1; i <= KK; ++i) p[i] = 0.0;
#pragma unroll
  for (int d = 1; d <= KK; ++d) {
    if (d <= k) {
      const double z = shap_lane_f64(zl, d - 1);
      const double o = ((mx >> (d - 1)) & 1u) ? 1.0 : 0.0;
#pragma unroll
      for (int i = d - 1; i >= 0; --i) {
        p[i + 1] = fma(o, p[i], p[i + 1]);
        p[i] *= z;
      }
    }
  }
  // p[i] = 0 for i > k and c_k[i] = 0 for i >= k: the sums run to KK unguarded
  double s0 = 0.0;
#pragma unroll
  for (int i = 0; i < KK; ++i) s0 = fma(ck[i], p[i], s0);
  const double c0 = -v * s0;
#pragma unroll
  for (int e = 0; e < KK; ++e) {
    if (e < k) {
      const double z = shap_lane_f64(zl, e);
      const int f = __builtin_amdgcn_readlane(fl, e);
      double q = 0.0, tot = 0.0;
#pragma unroll
      for (int i = KK; i >= 1; --i) {
        q = fma(-z, q, p[i]);
        tot = fma(ck[i - 1], q, tot);
      }
      const double c = ((mx >> e) & 1u) ? (1.0 - z) * v * tot : c0;
      if (live && c != 0.0) {
        if (USE_LDS) __hip_atomic_fetch_add(dst + f, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else gbl_add(dst + f, c);
      }
    }
  }
}

// MX: [l1 - l0, R] masks of shap_mask_kernel.  out: [*, F+1], row out_r0 + r;
// feature columns only, the bias column is the caller's.  lane = row, wave =
// leaf slice: the leaf's table entries are wave-uniform, only the mask
// differs per lane.  Per-row sums as in shap_pair_kernel's averaged mode.
// Four waves per block: with six (two blocks per CU at F = 100 would then fill
// the three waves per SIMD the registers allow) the same run took 48 ms.
template <bool USE_LDS>
__global__ __launch_bounds__(SHAP_ROWS * SHAP_WAVES) void shap_path_kernel(
    const uint32_t* __restrict__ MX, int R, const int* __restrict__ el_off, const int* __restrict__ el_feat,
    const double* __restrict__ el_zero, const double* __restrict__ leaf_val, const int* __restrict__ leaf_cls,
    int cls, int l0, int l1, const double* __restrict__ C, double vscale, double* __restrict__ out,
    long long out_r0, int F) {
  extern __shared__ double shap_smem[];
  double* sC = shap_smem;                                     // [33 * 32]
  double* acc = shap_smem + (SHAP_PMAX + 1) * SHAP_CDIM;      // [64][stride], odd stride
  const int stride = (F + 1) | 1;
  for (int i = threadIdx.x; i < (SHAP_PMAX + 1) * SHAP_CDIM; i += blockDim.x) sC[i] = C[i];
  if (USE_LDS)
    for (int i = threadIdx.x; i < SHAP_ROWS * stride; i += blockDim.x) acc[i] = 0.0;
  __syncthreads();
  const int lane = threadIdx.x & (SHAP_ROWS - 1);
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / SHAP_ROWS));
  const int r = blockIdx.x * SHAP_ROWS + lane;
  const bool live = r < R;
  double* dst = USE_LDS ? acc + lane * stride : out + (size_t)(out_r0 + (live ? r : 0)) * (size_t)(F + 1);
  for (int l = l0 + (int)blockIdx.y * SHAP_WAVES + w; l < l1; l += SHAP_WAVES * (int)gridDim.y) {
    if (leaf_cls[l] != cls) continue;
    const int e0 = el_off[l];
    const int k = el_off[l + 1] - e0;
    if (k <= 0 || k > SHAP_PMAX) continue;                    // single-leaf tree: constant, no contribution
    const double v = leaf_val[l] * vscale;
    const uint32_t mx = live ? MX[(size_t)(l - l0) * R + r] : 0u;
    const int ei = e0 + (lane < k ? lane : k - 1);            // lane e: element e of the leaf
    const double zl = el_zero[ei];
    const int fl = el_feat[ei];
    const double* ck = sC + k * SHAP_CDIM;
    if (k <= 4) shap_path_leaf<4, USE_LDS>(mx, k, zl, fl, ck, v, live, dst);
    else if (k <= 8) shap_path_leaf<8, USE_LDS>(mx, k, zl, fl, ck, v, live, dst);
    else if (k <= 16) shap_path_leaf<16, USE_LDS>(mx, k, zl, fl, ck, v, live, dst);
    else shap_path_leaf<32, USE_LDS>(mx, k, zl, fl, ck, v, live, dst);
  }
  if (USE_LDS) {
    __syncthreads();
    const int n = SHAP_ROWS * (F + 1);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int rr = i / (F + 1), f = i - rr * (F + 1);
      const int gr = blockIdx.x * SHAP_ROWS + rr;
      const double a = acc[rr * stride + f];
      if (gr < R && a != 0.0) gbl_add(&out[(size_t)(out_r0 + gr) * (size_t)(F + 1) + f], a);
    }
  }
}

extern "C" int h2o_shap_masks(const float* X, long long ldx, int R, const int* nodes, const int* cat_off,
                              const int* cat_len, const uint8_t* cat_bits, const int* el_off, const int* el_feat,
                              const int* cond_off, const int* cond_node, const uint8_t* cond_left,
                              const double* leaf_val, const int* leaf_cls, int cls, int l0, int l1, uint32_t* mask,
                              double* score, double vscale, hipStream_t s) {
  if (R <= 0 || l1 <= l0) return 0;
  const int nl = l1 - l0;
  dim3 grid((unsigned)((R + 255) / 256), (unsigned)(nl < 65535 ? nl : 65535));
  hipLaunchKernelGGL(shap_mask_kernel, grid, dim3(256), 0, s, X, ldx, R, (const int4*)nodes, cat_off, cat_len,
                     cat_bits, el_off, el_feat, cond_off, cond_node, cond_left, leaf_val, leaf_cls, cls, l0, l1,
                     mask, score, vscale);
  return (int)hipGetLastError();
}

// LDS bytes the averaged mode needs for F features (weight table + 64 rows).
extern "C" long long h2o_shap_lds_bytes(int F) {
  return (long long)(SHAP_WDIM * SHAP_WDIM + SHAP_ROWS * ((F + 1) | 1)) * (long long)sizeof(double);
}

extern "C" int h2o_shap_pairs(const uint32_t* MX, int R, const uint32_t* MZ, int Bt, const int* el_off,
                              const int* el_feat, const double* leaf_val, const int* leaf_cls, int cls, int l0,
                              int l1, const double* W, const double* pscale, double vscale, double* out,
                              long long out_r0, int b0, int Btot, int F, int per_ref, hipStream_t s) {
  if (R <= 0 || Bt <= 0 || l1 <= l0) return 0;
  const int nl = l1 - l0;
  const int bx = (R + SHAP_ROWS - 1) / SHAP_ROWS;
  // leaf slices per row block: enough blocks to fill the 256 CUs a few times over
  int by = (2048 + bx - 1) / bx;
  const int by_max = (nl + SHAP_WAVES - 1) / SHAP_WAVES;
  if (by > by_max) by = by_max;
  if (by < 1) by = 1;
  if (by > 65535) by = 65535;
  const dim3 grid((unsigned)bx, (unsigned)by), block(SHAP_ROWS * SHAP_WAVES);
  const size_t wbytes = (size_t)SHAP_WDIM * SHAP_WDIM * sizeof(double);
#define SHAP_LAUNCH(PR_, LDS_, BYTES_)                                                                          \
  hipLaunchKernelGGL((shap_pair_kernel<PR_, LDS_>), grid, block, (BYTES_), s, MX, R, MZ, Bt, el_off, el_feat,   \
                     leaf_val, leaf_cls, cls, l0, l1, W, pscale, vscale, out, out_r0, b0, Btot, F)
  if (per_ref) {
    SHAP_LAUNCH(true, false, wbytes);
  } else {
    const size_t lds = (size_t)h2o_shap_lds_bytes(F);
    if (lds <= 64 * 1024) {
      SHAP_LAUNCH(false, true, lds);
    } else if (lds <= 160 * 1024) {
      hipError_t e = hipFuncSetAttribute((const void*)shap_pair_kernel<false, true>,
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
      SHAP_LAUNCH(false, true, lds);
    } else {
      SHAP_LAUNCH(false, false, wbytes);   // too many features for LDS rows: global f64 atomics
    }
  }
#undef SHAP_LAUNCH
  return (int)hipGetLastError();
}

// LDS bytes the path kernel needs for F features (coefficient table + 64 rows).
extern "C" long long h2o_shap_path_lds_bytes(int F) {
  return (long long)((SHAP_PMAX + 1) * SHAP_CDIM + SHAP_ROWS * ((F + 1) | 1)) * (long long)sizeof(double);
}

// Path-dependent TreeSHAP of leaves [l0, l1) for the R rows whose masks are in
// MX; C: [33 * 32] f64, C[k * 32 + i] = i! (k-1-i)! / k!.
extern "C" int h2o_shap_path(const uint32_t* MX, int R, const int* el_off, const int* el_feat,
                             const double* el_zero, const double* leaf_val, const int* leaf_cls, int cls, int l0,
                             int l1, const double* C, double vscale, double* out, long long out_r0, int F,
                             hipStream_t s) {
  if (R <= 0 || l1 <= l0) return 0;
  const int nl = l1 - l0;
  const int bx = (R + SHAP_ROWS - 1) / SHAP_ROWS;
  int by = (2048 + bx - 1) / bx;
  const int by_max = (nl + SHAP_WAVES - 1) / SHAP_WAVES;
  if (by > by_max) by = by_max;
  if (by < 1) by = 1;
  if (by > 65535) by = 65535;
  const dim3 grid((unsigned)bx, (unsigned)by), block(SHAP_ROWS * SHAP_WAVES);
#define SHAP_PATH_LAUNCH(LDS_, BYTES_)                                                                        \
  hipLaunchKernelGGL((shap_path_kernel<LDS_>), grid, block, (BYTES_), s, MX, R, el_off, el_feat, el_zero,     \
                     leaf_val, leaf_cls, cls, l0, l1, C, vscale, out, out_r0, F)
  const size_t lds = (size_t)h2o_shap_path_lds_bytes(F);
  if (lds <= 64 * 1024) {
    SHAP_PATH_LAUNCH(true, lds);
  } else if (lds <= 160 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)shap_path_kernel<true>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    SHAP_PATH_LAUNCH(true, lds);
  } else {
    SHAP_PATH_LAUNCH(false, (size_t)(SHAP_PMAX + 1) * SHAP_CDIM * sizeof(double));
  }
#undef SHAP_PATH_LAUNCH
  return (int)hipGetLastError();
}
