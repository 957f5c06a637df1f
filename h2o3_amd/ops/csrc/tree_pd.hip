// Partial dependence of a packed forest: per-class leaf sums of every row on a
// grid of overridden columns.  Reference: hex/PartialDependence.java (score the
// frame once per grid value with one or two columns held constant).
//
// out[g, r, k] is what forest_predict_kernel (tree_predict.hip) gives for row
// r after X[cols[s], r] = grid[s, g] for every s, bit for bit: the same f32
// leaf values are added in tree order into a zero accumulator.
//
// A launch covers up to 64 grid points as the bits of a uint64_t.
//   pd_node_mask_kernel  one thread per packed node: for a node that splits on
//                        an overridden column, the bits g whose grid value goes
//                        left there (go()'s rule; no row is involved)
//   pd_walk_kernel       one thread per row: every tree is walked depth-first
//                        over (node, mask) from (root, all bits).  A node on
//                        the row's own columns steps as go() does; a node on an
//                        overridden column splits the mask, pushes the right
//                        part when both parts are non-empty, and goes on left.
//                        A leaf adds its value to acc[g] of every bit g.
// Every g reaches one leaf per tree, so acc[g] sums in tree order.  The stack
// holds at most min(tree depth, G - 1) entries: an entry is pushed only when a
// mask really splits, and the entries sit at distinct depths of one path.
// acc and the stack live in LDS, thread-minor (lane l of a wave on bank
// l mod 32 or 64: conflict-free), sized from G and that bound.
#include "common.h"

#define PD_MAX_COLS 4

struct PdCols {
  int c[PD_MAX_COLS];   // overridden feature ids, -1 = unused
};

__device__ __forceinline__ int pd_slot(const PdCols& cols, int f) {
  int s = -1;
#pragma unroll
  for (int i = 0; i < PD_MAX_COLS; ++i) s = (cols.c[i] == f) ? i : s;
  return s;
}

// lmask[nd]: bit g set when grid value (g0 + g) of the node's column goes left.
__global__ __launch_bounds__(256) void pd_node_mask_kernel(
    const int4* __restrict__ nodes, int n_nodes, const int* __restrict__ cat_off, const int* __restrict__ cat_len,
    const uint8_t* __restrict__ cat_bits, PdCols cols, const float* __restrict__ grid, int G, int g0, int gc,
    unsigned long long* __restrict__ lmask) {
  const int nd = blockIdx.x * blockDim.x + threadIdx.x;
  if (nd >= n_nodes) return;
  const int4 n = nodes[nd];
  unsigned long long m = 0ull;
  const int s = n.z >= 0 ? pd_slot(cols, n.x & 0x3FFFFFFF) : -1;
  if (s >= 0) {
    const bool nal = (n.x >> 30) & 1;
    const float* gv = grid + (size_t)s * G + g0;
    for (int g = 0; g < gc; ++g) {
      const float x = gv[g];
      bool go_left;
      if (n.x < 0) {   // categorical: left-level bitset
        if (x != x) go_left = nal;
        else {
          const int c = (int)x;
          go_left = (c < 0 || c >= cat_len[nd]) ? nal : (cat_bits[cat_off[nd] + c] != 0);
        }
      } else {
        go_left = (x != x) ? nal : (x < __int_as_float(n.y));
      }
      m |= (unsigned long long)go_left << g;
    }
  }
  lmask[nd] = m;
}

// LDS of a block of `threads` rows: the mask stack (8 B), acc (4 B), the node
// stack (4 B); depth >= 1.
__host__ __device__ inline size_t pd_lds_bytes(int threads, int gc, int depth) {
  return (size_t)threads * ((size_t)depth * 12 + (size_t)gc * 4);
}

__global__ __launch_bounds__(256) void pd_walk_kernel(
    const float* __restrict__ X, long long ldx, int R, const int4* __restrict__ nodes,
    const int* __restrict__ cat_off, const int* __restrict__ cat_len, const uint8_t* __restrict__ cat_bits,
    const float* __restrict__ value, const int* __restrict__ roots, const int* __restrict__ tclass, int T, int cls,
    PdCols cols, const unsigned long long* __restrict__ lmask, int gc, int depth, float* __restrict__ out,
    long long out_gstride, int K) {
  extern __shared__ __align__(16) unsigned char pd_smem[];
  const int B = blockDim.x;
  const int tid = threadIdx.x;
  unsigned long long* smask = reinterpret_cast<unsigned long long*>(pd_smem);   // [depth][B]
  float* acc = reinterpret_cast<float*>(smask + (size_t)depth * B);              // [gc][B]
  int* snode = reinterpret_cast<int*>(acc + (size_t)gc * B);                     // [depth][B]
  const long long r = (long long)blockIdx.x * B + tid;
  if (r >= R) return;   // no block-wide barrier below: every LDS cell belongs to one thread
  for (int g = 0; g < gc; ++g) acc[g * B + tid] = 0.f;
  const unsigned long long full = gc >= 64 ? ~0ull : ((1ull << gc) - 1ull);
  for (int t = 0; t < T; ++t) {
    if (tclass[t] != cls) continue;
    int nd = roots[t];
    unsigned long long mask = full;
    int sp = 0;
    for (;;) {
      const int4 n = nodes[nd];
      if (n.z < 0) {   // leaf
        const float v = value[nd];
        for (unsigned long long m = mask; m; m &= m - 1) acc[(__ffsll((long long)m) - 1) * B + tid] += v;
        if (sp == 0) break;
        --sp;
        nd = snode[sp * B + tid];
        mask = smask[sp * B + tid];
        continue;
      }
      const int f = n.x & 0x3FFFFFFF;
      if (pd_slot(cols, f) >= 0) {
        const unsigned long long lm = lmask[nd] & mask;
        const unsigned long long rm = mask & ~lm;
        if (lm != 0ull && rm != 0ull) {
          snode[sp * B + tid] = n.w;
          smask[sp * B + tid] = rm;
          ++sp;
          nd = n.z;
          mask = lm;
        } else {
          nd = lm != 0ull ? n.z : n.w;
        }
        continue;
      }
      // the row's own value: forest_predict_kernel's go()
      const float x = X[(size_t)f * ldx + r];
      const bool nal = (n.x >> 30) & 1;
      bool go_left;
      if (n.x < 0) {
        if (x != x) go_left = nal;
        else {
          const int c = (int)x;
          go_left = (c < 0 || c >= cat_len[nd]) ? nal : (cat_bits[cat_off[nd] + c] != 0);
        }
      } else {
        go_left = (x != x) ? nal : (x < __int_as_float(n.y));
      }
      nd = go_left ? n.z : n.w;
    }
  }
  float* o = out + (size_t)r * K + cls;
  for (int g = 0; g < gc; ++g) o[(size_t)g * out_gstride] = acc[g * B + tid];
}

// Threads per block for gc grid points and a stack of `depth` entries: 256,
// halved until the block's LDS fits the 160 KiB of a CU; 0 when 64 do not fit.
extern "C" int h2o_pd_block_threads(int gc, int depth) {
  if (depth < 1) depth = 1;
  int th = 256;
  while (th >= 64 && pd_lds_bytes(th, gc, depth) > 160 * 1024) th >>= 1;
  return th >= 64 ? th : 0;
}

extern "C" long long h2o_pd_lds_bytes(int threads, int gc, int depth) {
  return (long long)pd_lds_bytes(threads, gc, depth < 1 ? 1 : depth);
}

// One chunk of gc <= 64 grid points (grid columns [g0, g0 + gc) of grid [S, G])
// for rows [0, R) of X (leading dimension ldx; X already points at the first
// row of the tile) and the trees of class cls.  out points at element
// [g0, first row, 0] of the [G, N, K] result; out_gstride = N * K.  lmask:
// n_nodes uint64 of scratch, filled when build_masks is set (a later class of
// the same chunk reuses it).  depth: the forest's max depth (splits on a path).
extern "C" int h2o_forest_pd_chunk(const float* X, long long ldx, int R, const int* nodes, int n_nodes,
                                   const int* cat_off, const int* cat_len, const uint8_t* cat_bits,
                                   const float* value, const int* roots, const int* tclass, int T, int cls,
                                   const int* cols, int S, const float* grid, int G, int g0, int gc, int depth,
                                   unsigned long long* lmask, int build_masks, float* out,
                                   long long out_gstride, int K, hipStream_t s) {
  if (S < 1 || S > PD_MAX_COLS || gc < 1 || gc > 64 || g0 < 0 || g0 + gc > G) return (int)hipErrorInvalidValue;
  if (R <= 0 || T <= 0 || n_nodes <= 0) return 0;
  PdCols pc;
  for (int i = 0; i < PD_MAX_COLS; ++i) pc.c[i] = i < S ? cols[i] : -1;
  int sd = depth < gc - 1 ? depth : gc - 1;   // stack bound
  if (sd < 1) sd = 1;
  const int threads = h2o_pd_block_threads(gc, sd);
  if (threads == 0) return (int)hipErrorInvalidValue;
  const size_t lds = pd_lds_bytes(threads, gc, sd);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)pd_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  if (build_masks)
    hipLaunchKernelGGL(pd_node_mask_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s,
                       (const int4*)nodes, n_nodes, cat_off, cat_len, cat_bits, pc, grid, G, g0, gc, lmask);
  hipLaunchKernelGGL(pd_walk_kernel, dim3((unsigned)((R + threads - 1) / threads)), dim3(threads), lds, s, X, ldx,
                     R, (const int4*)nodes, cat_off, cat_len, cat_bits, value, roots, tclass, T, cls, pc, lmask, gc,
                     sd, out, out_gstride, K);
  return (int)hipGetLastError();
}
