// Extended Isolation Forest scoring: walk every hyperplane tree for every row
// and add the leaves' path lengths.  Reference:
// hex/tree/isoforextended/isolationtree/CompressedIsolationTree.java
// (computePathLength: at a node, (row - p) . n <= 0 goes left).
//
// A trained node has extension_level + 1 non-zero normal components, so the
// forest is stored sparse:
//   hdr   int4 per node   inner: left, right, first entry, entry count
//                         leaf:  -1, -1, the f64 path length in the other 8 B
//   col   int32 per entry the column of the entry, ascending within a node
//   np    f64 pair per entry (normal component, point component)
// Node ids are global (trees concatenated); roots[t] is tree t's first node.
//
// The rule, in f64: xj = the f32 input widened, NaN -> 0, +-inf -> +-DBL_MAX;
// proj = sum over the node's entries, in entry order, of n_j * (xj - p_j), each
// product rounded before it is added; left iff proj <= 0, a NaN proj goes right.
// The file is built without FMA contraction (the hipcc-flags line below; the
// project's -ffp-contract=fast overrides a contract(off) pragma), so the torch
// twin and the numpy oracle compute the same bits, and two products that
// overflow to opposite infinities give NaN as the rule says, where
// fma(n, d, +inf) would stay +inf.
//
// One thread per row, X row-major [n, P] f32.  TW trees are walked together
// per thread: TW independent header -> entry -> X -> header load chains in
// flight instead of one (the walk is latency-bound).  TILE stages the 64 rows
// of a wave in LDS as tile[j][lane] (one coalesced read of 64 * P contiguous
// floats), so the walk's per-lane X[r, j] reads hit LDS, conflict-free for any
// per-lane j, instead of 64 different cache lines.
// hipcc-flags: -ffp-contract=off
#include "common.h"
#include <cfloat>

#define EIF_TILE_LDS_MAX (64 * 1024)   // dynamic LDS a block may ask for without opting in

__device__ __forceinline__ double eif_clean(float xf) {
  double x = (double)xf;
  if (x != x) return 0.0;
  return fmin(fmax(x, -DBL_MAX), DBL_MAX);
}

template <int TW, bool TILE>
__global__ __launch_bounds__(TILE ? 64 : 256) void eif_lengths_kernel(
    const float* __restrict__ X, long long n, int P, const int4* __restrict__ hdr, const int* __restrict__ col,
    const double2* __restrict__ np, const int* __restrict__ roots, int t0, int t1, double* __restrict__ tot,
    int* __restrict__ node_out) {
  extern __shared__ float tile[];
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (TILE) {
    // the block is one wave; its rows are 64 * P contiguous floats of X
    const long long r0 = (long long)blockIdx.x * H2O_WAVE;
    const long long left = n - r0;
    const int cnt = (int)(left < H2O_WAVE ? left : H2O_WAVE) * P;
    const float* __restrict__ src = X + r0 * P;
    const int dj = H2O_WAVE % P, dr = H2O_WAVE / P;
    int j = threadIdx.x % P, rr = threadIdx.x / P;
    for (int i = threadIdx.x; i < cnt; i += H2O_WAVE) {
      tile[j * H2O_WAVE + rr] = src[i];
      j += dj;
      rr += dr;
      if (j >= P) {
        j -= P;
        ++rr;
      }
    }
    __syncthreads();
  }
  if (r >= n) return;
  const float* __restrict__ xr = X + r * P;
  const int lane = threadIdx.x;          // TILE blocks are one wave wide
  const int W = t1 - t0;
  double acc = tot[r];
  for (int t = t0; t < t1; t += TW) {
    int nd[TW];
    int4 h[TW];
#pragma unroll
    for (int k = 0; k < TW; ++k) {
      nd[k] = t + k < t1 ? roots[t + k] : -1;
      h[k] = nd[k] >= 0 ? hdr[nd[k]] : int4{-1, -1, 0, 0};
    }
    bool live = true;
    while (live) {
      live = false;
#pragma unroll
      for (int k = 0; k < TW; ++k) {
        if (h[k].x >= 0) {
          double proj = 0.0;
          const int e1 = h[k].z + h[k].w;
          for (int e = h[k].z; e < e1; ++e) {
            const int c = col[e];
            const double2 q = np[e];
            const float xf = TILE ? tile[c * H2O_WAVE + lane] : xr[c];
            const double d = eif_clean(xf) - q.y;
            proj = proj + q.x * d;
          }
          nd[k] = proj <= 0.0 ? h[k].x : h[k].y;
          h[k] = hdr[nd[k]];
          live |= h[k].x >= 0;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < TW; ++k) {
      if (nd[k] < 0) continue;
      acc += __hiloint2double(h[k].w, h[k].z);
      if (node_out) node_out[r * W + (t + k - t0)] = nd[k] - roots[t + k];
    }
  }
  tot[r] = acc;
}

// tot[r] += path lengths of trees t0..t1-1 for every row of X [n, P], in tree
// order; node_out (optional) [n, t1 - t0] gets the tree-local leaf ids.  tw =
// trees walked together per thread (1, 2 or 4); tile != 0 stages rows in LDS
// and needs 256 * P bytes of it per block.
extern "C" int h2o_eif_lengths(const float* X, long long n, int P, const int* hdr, const int* col,
                               const double* np, const int* roots, int t0, int t1, double* tot, int* node_out,
                               int tw, int tile, hipStream_t s) {
  if (n <= 0 || t0 >= t1) return 0;
  if (P <= 0 || t0 < 0 || (tw != 1 && tw != 2 && tw != 4)) return (int)hipErrorInvalidValue;
  const size_t lds = tile ? (size_t)H2O_WAVE * sizeof(float) * (size_t)P : 0;
  if (lds > EIF_TILE_LDS_MAX) return (int)hipErrorInvalidValue;
  const int threads = tile ? H2O_WAVE : 256;
  const long long blocks = (n + threads - 1) / threads;
  if (blocks > 0x7FFFFFFFLL) return (int)hipErrorInvalidValue;
#define EIF_LAUNCH(TW_, TILE_)                                                                              \
  hipLaunchKernelGGL((eif_lengths_kernel<TW_, TILE_>), dim3((unsigned)blocks), dim3(threads), lds, s, X, n, P, \
                     (const int4*)hdr, col, (const double2*)np, roots, t0, t1, tot, node_out)
  if (tile) {
    if (tw == 4) EIF_LAUNCH(4, true);
    else if (tw == 2) EIF_LAUNCH(2, true);
    else EIF_LAUNCH(1, true);
  } else {
    if (tw == 4) EIF_LAUNCH(4, false);
    else if (tw == 2) EIF_LAUNCH(2, false);
    else EIF_LAUNCH(1, false);
  }
#undef EIF_LAUNCH
  return (int)hipGetLastError();
}
