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
