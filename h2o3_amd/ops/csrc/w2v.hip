// Word2Vec hierarchical-softmax mini-batch step (skip-gram and CBOW).
// Reference: hex/word2vec/WordVectorTrainer.java (hierarchicalSoftmaxSG / CBOW),
// batched as in models/word2vec.py; the rule is stated in ops/w2v_ops.py
// (hsm_step_torch), which is also the f64 oracle of tests/test_w2v_kernel.py.
//
// One example = a target word c and up to W input words.  From the tables as
// they stand at the start of the batch:
//   h      = mean of syn0[inputs]
//   dot_l  = syn1[point[c][l]] . h                  for l < len[c]
//   g_l    = ((1 - code[c][l]) - sigmoid(dot_l)) * lr    if |dot_l| < 6, else 0
//   neu1e  = sum_l g_l * syn1[point[c][l]]
//   syn1[node] += sum g * h    / max(1, c1[node] / 8)    c1 = valid (example, l) hits
//   syn0[word] += sum neu1e    / max(1, c0[word] / 8)    c0 = (example, slot) hits
//
// Work split: one wave per example, lane-strided (coalesced) rows, each lane
// holding NR = ceil(d / 64) components of h and neu1e in registers; the dot is a
// wave butterfly.  A workgroup walks a contiguous slab of the batch.  The loop
// over l runs over the word's own code length (ragged len / point / code).
//
// Three kernels per batch on one stream, all reading batch-start state:
//   grad    g[b, l], neu1e[b, :] to scratch; c1 / c0 by integer atomics
//   apply1  syn1 += g * h / c1'     (reads syn0 only, recomputes h)
//   apply0  syn0 += neu1e / c0'     (a launch of its own: no update of syn0
//                                    may begin before every read of it is done)
//
// Hot-node cache: Huffman inner nodes are numbered in creation order, so the
// root is the last node and the most-hit nodes are the highest indices.  Each
// workgroup keeps the top H nodes' accumulators (apply1: H * d floats; grad: H
// counters) in LDS, adds to them with LDS atomics and flushes each touched row
// once with global atomics; the root then takes grid * d global atomics per
// batch instead of B * d.  Nodes below the cache and syn0 rows take global
// atomics directly.
//
// Float atomics commit in arbitrary order, so the result is order-dependent
// in the last bits, as index_add_ is on the torch route.
#include "common.h"

#define W2V_MAX_THREADS 1024
#define W2V_MAX_D 512
#define W2V_LDS_MAX (64 * 1024)   // dynamic LDS a block may ask for without opting in
#define W2V_MAX_EXP 6.0f          // WordVectorTrainer.MAX_EXP

struct W2vTables {        // ragged Huffman tables
  const int* len;         // [V] code length
  const int* point;       // [V, Lmax] inner node per level
  const signed char* code;  // [V, Lmax] 0 / 1
  int V, nodes, Lmax;     // nodes = rows of syn1
};

struct W2vBatch {
  const long long* tgt;       // [B] target word
  const long long* inp;       // [B, W] input words
  const unsigned char* mask;  // [B, W] slot used (null: all)
  int B, W;
  int per;                    // examples per workgroup slab
};

// h = mean of the example's input rows; returns the number of inputs
template <int NR>
__device__ __forceinline__ int w2v_hidden(const float* __restrict__ syn0, int V, int d, const long long* inp,
                                          const unsigned char* mask, int W, int lane, float (&h)[NR]) {
#pragma unroll
  for (int j = 0; j < NR; ++j) h[j] = 0.f;
  int n_in = 0;
  for (int k = 0; k < W; ++k) {
    if (mask && !mask[k]) continue;
    const long long w = inp[k];
    if ((unsigned long long)w >= (unsigned long long)V) continue;
    const float* __restrict__ row = syn0 + (size_t)w * d;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int e = j * H2O_WAVE + lane;
      if (e < d) h[j] += row[e];
    }
    ++n_in;
  }
  if (n_in > 1) {
    const float nf = (float)n_in;
#pragma unroll
    for (int j = 0; j < NR; ++j) h[j] = h[j] / nf;
  }
  return n_in;
}

// code length of the example's target; 0 when the example does nothing
__device__ __forceinline__ int w2v_path(const W2vTables& t, long long c) {
  if ((unsigned long long)c >= (unsigned long long)t.V) return 0;
  const int n = t.len[c];
  return n < t.Lmax ? n : t.Lmax;
}

template <int NR>
__global__ __launch_bounds__(W2V_MAX_THREADS) void w2v_grad_kernel(
    const float* __restrict__ syn0, const float* __restrict__ syn1, int d, W2vTables t, W2vBatch bt, float lr,
    int hot_base, int H, float* __restrict__ g, float* __restrict__ neu1e, int* __restrict__ c1,
    int* __restrict__ c0) {
  extern __shared__ int w2v_cnt[];   // hits of the H cached nodes
  for (int i = threadIdx.x; i < H; i += blockDim.x) w2v_cnt[i] = 0;
  __syncthreads();
  const int lane = lane_id(), nw = blockDim.x / H2O_WAVE;
  const long long b0 = (long long)blockIdx.x * bt.per;
  const long long b1 = b0 + bt.per < bt.B ? b0 + bt.per : bt.B;
  for (long long b = b0 + wave_id(); b < b1; b += nw) {
    const long long c = bt.tgt[b];
    const int n = w2v_path(t, c);
    const long long* inp = bt.inp + b * bt.W;
    const unsigned char* mask = bt.mask ? bt.mask + b * bt.W : nullptr;
    float h[NR], ne[NR];
    if ((unsigned long long)c >= (unsigned long long)t.V) continue;
    const int n_in = w2v_hidden<NR>(syn0, t.V, d, inp, mask, bt.W, lane, h);
    if (n_in == 0) continue;
    for (int k = lane; k < bt.W; k += H2O_WAVE) {
      const long long w = inp[k];
      if ((!mask || mask[k]) && (unsigned long long)w < (unsigned long long)t.V) atomicAdd(&c0[w], 1);
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) ne[j] = 0.f;
    const int* __restrict__ pt = t.point + (size_t)c * t.Lmax;
    const signed char* __restrict__ cd = t.code + (size_t)c * t.Lmax;
    for (int l = 0; l < n; ++l) {
      const int node = pt[l];
      float gv = 0.f;
      if ((unsigned)node < (unsigned)t.nodes) {
        const float* __restrict__ row = syn1 + (size_t)node * d;
        float r[NR], p = 0.f;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const int e = j * H2O_WAVE + lane;
          r[j] = e < d ? row[e] : 0.f;
          p += r[j] * h[j];
        }
        const float dot = wave_sum(p);   // the butterfly leaves the same bits in every lane
        if (fabsf(dot) < W2V_MAX_EXP) {
          gv = ((1.f - (float)cd[l]) - 1.f / (1.f + expf(-dot))) * lr;
#pragma unroll
          for (int j = 0; j < NR; ++j) ne[j] += gv * r[j];
          if (lane == 0) {
            if (node >= hot_base) atomicAdd(&w2v_cnt[node - hot_base], 1);
            else atomicAdd(&c1[node], 1);
          }
        }
      }
      if (lane == 0) g[b * t.Lmax + l] = gv;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int e = j * H2O_WAVE + lane;
      if (e < d) neu1e[b * d + e] = ne[j];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += blockDim.x)
    if (w2v_cnt[i]) atomicAdd(&c1[hot_base + i], w2v_cnt[i]);
}

template <int NR>
__global__ __launch_bounds__(W2V_MAX_THREADS) void w2v_apply1_kernel(
    const float* __restrict__ syn0, float* __restrict__ syn1, int d, W2vTables t, W2vBatch bt, int hot_base, int H,
    const float* __restrict__ g, const int* __restrict__ c1) {
  extern __shared__ float w2v_acc[];   // [H, d] update of the cached nodes, then [H] touched flags
  int* touched = (int*)(w2v_acc + (size_t)H * d);
  for (int i = threadIdx.x; i < H * d + H; i += blockDim.x) w2v_acc[i] = 0.f;   // 0.f and 0 share their bits
  __syncthreads();
  const int lane = lane_id(), nw = blockDim.x / H2O_WAVE;
  const long long b0 = (long long)blockIdx.x * bt.per;
  const long long b1 = b0 + bt.per < bt.B ? b0 + bt.per : bt.B;
  for (long long b = b0 + wave_id(); b < b1; b += nw) {
    const long long c = bt.tgt[b];
    const int n = w2v_path(t, c);
    if (n == 0) continue;
    float h[NR];
    const int n_in = w2v_hidden<NR>(syn0, t.V, d, bt.inp + b * bt.W, bt.mask ? bt.mask + b * bt.W : nullptr, bt.W,
                                    lane, h);
    if (n_in == 0) continue;
    const int* __restrict__ pt = t.point + (size_t)c * t.Lmax;
    for (int l = 0; l < n; ++l) {
      const float gv = g[b * t.Lmax + l];
      const int node = pt[l];
      if (gv == 0.f || (unsigned)node >= (unsigned)t.nodes) continue;   // skipped or out of the tree
      const float cf = fmaxf(1.f, (float)c1[node] * 0.125f);
      if (node >= hot_base) {
        float* a = w2v_acc + (size_t)(node - hot_base) * d;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const int e = j * H2O_WAVE + lane;
          if (e < d) lds_add(a + e, gv * h[j] / cf);
        }
        if (lane == 0) touched[node - hot_base] = 1;
      } else {
        float* a = syn1 + (size_t)node * d;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const int e = j * H2O_WAVE + lane;
          if (e < d) gbl_add(a + e, gv * h[j] / cf);
        }
      }
    }
  }
  __syncthreads();
  for (int r = wave_id(); r < H; r += nw) {
    if (!touched[r]) continue;
    float* a = syn1 + (size_t)(hot_base + r) * d;
    for (int e = lane; e < d; e += H2O_WAVE) {
      const float v = w2v_acc[(size_t)r * d + e];
      if (v != 0.f) gbl_add(a + e, v);
    }
  }
}

template <int NR>
__global__ __launch_bounds__(W2V_MAX_THREADS) void w2v_apply0_kernel(
    float* __restrict__ syn0, int d, W2vTables t, W2vBatch bt, const float* __restrict__ neu1e,
    const int* __restrict__ c0) {
  const int lane = lane_id(), nw = blockDim.x / H2O_WAVE;
  const long long b0 = (long long)blockIdx.x * bt.per;
  const long long b1 = b0 + bt.per < bt.B ? b0 + bt.per : bt.B;
  for (long long b = b0 + wave_id(); b < b1; b += nw) {
    if ((unsigned long long)bt.tgt[b] >= (unsigned long long)t.V) continue;   // grad wrote no neu1e
    const long long* inp = bt.inp + b * bt.W;
    const unsigned char* mask = bt.mask ? bt.mask + b * bt.W : nullptr;
    float ne[NR];
    bool loaded = false;
    for (int k = 0; k < bt.W; ++k) {
      if (mask && !mask[k]) continue;
      const long long w = inp[k];
      if ((unsigned long long)w >= (unsigned long long)t.V) continue;
      if (!loaded) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const int e = j * H2O_WAVE + lane;
          ne[j] = e < d ? neu1e[b * d + e] : 0.f;
        }
        loaded = true;
      }
      const float cf = fmaxf(1.f, (float)c0[w] * 0.125f);
      float* a = syn0 + (size_t)w * d;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int e = j * H2O_WAVE + lane;
        if (e < d && ne[j] != 0.f) gbl_add(a + e, ne[j] / cf);
      }
    }
  }
}

// One mini-batch step on syn0 [V, d] and syn1 [nodes, d] (f32, row-major).
// tgt [B] / inp [B, W] are int64 word ids, mask [B, W] bytes (null: every slot
// is used).  Scratch: g [B, Lmax], neu1e [B, d] f32, counts [nodes + V] int32
// (c1 then c0; zeroed here).  Launch plan: H = nodes cached in LDS (the top H,
// (H * d + H) * 4 <= 64 KiB), threads per workgroup (a multiple of 64), grid
// = workgroups, each walking ceil(B / grid) consecutive examples.
extern "C" int h2o_w2v_hsm_step(float* syn0, float* syn1, int V, int nodes, int d, const int* len, const int* point,
                                const signed char* code, int Lmax, const long long* tgt, const long long* inp,
                                const unsigned char* mask, int B, int W, float lr, float* g, float* neu1e,
                                int* counts, int H, int threads, int grid, hipStream_t s) {
  if (B <= 0) return 0;
  if (V <= 0 || nodes <= 0 || d <= 0 || d > W2V_MAX_D || Lmax <= 0 || W <= 0 || H < 0 || H > nodes || grid <= 0 ||
      threads < H2O_WAVE || threads > W2V_MAX_THREADS || threads % H2O_WAVE != 0)
    return (int)hipErrorInvalidValue;
  const size_t lds1 = ((size_t)H * d + H) * sizeof(float);
  if (lds1 > W2V_LDS_MAX) return (int)hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counts, 0, ((size_t)nodes + V) * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  const W2vTables t{len, point, code, V, nodes, Lmax};
  const W2vBatch bt{tgt, inp, mask, B, W, (B + grid - 1) / grid};
  const int hot_base = nodes - H;
  int* c1 = counts;
  int* c0 = counts + nodes;
#define W2V_STEP(NR)                                                                                             \
  do {                                                                                                           \
    hipLaunchKernelGGL((w2v_grad_kernel<NR>), dim3(grid), dim3(threads), (size_t)H * sizeof(int), s, syn0, syn1, d, \
                       t, bt, lr, hot_base, H, g, neu1e, c1, c0);                                                \
    hipLaunchKernelGGL((w2v_apply1_kernel<NR>), dim3(grid), dim3(threads), lds1, s, syn0, syn1, d, t, bt, hot_base, \
                       H, g, c1);                                                                                \
    hipLaunchKernelGGL((w2v_apply0_kernel<NR>), dim3(grid), dim3(threads), 0, s, syn0, d, t, bt, neu1e, c0);      \
  } while (0)
  if (d <= 64) W2V_STEP(1);
  else if (d <= 128) W2V_STEP(2);
  else if (d <= 256) W2V_STEP(4);
  else W2V_STEP(8);
#undef W2V_STEP
  return (int)hipGetLastError();
}
