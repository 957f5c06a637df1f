// DeepSHAP (rescale rule) pair stage of a dense MLP: contributions of the
// inputs to one linear output unit for every (test row, background row) pair.
//
// The forward pass is not repeated here: the caller hands over the f32
// pre-activations (bias included) of every hidden layer for the test rows and
// for the background rows, as the scoring forward produced them.  For a pair
// (x, z) the multiplier on the last hidden activation is the output weight
// row; going down through hidden layer l
//     g_l = s_l (act(a_l(x)) - act(a_l(z))) / (a_l(x) - a_l(z))
//           (s_l act'((a_l(x) + a_l(z)) / 2) where the two differ by < 1e-6),
//     M_{l-1} = (M_l * g_l) W_l,
// and phi_i = M_0,i (x_i - z_i).
//
// MI355X design (after dl.hip's dl_mlp_fb_kernel): a workgroup owns 16 test
// rows; their input tile and every layer's pre-activation tile stay in LDS for
// its lifetime.  It loops over its slice of DLS_CHUNK background rows; per
// background row the 16 x U tile M * g is formed in an LDS ping-pong buffer
// and (M * g) W_l runs on v_mfma_f32_16x16x4_f32 with the operand orientation
// of the training step's dA = dZ W (weights streamed from L2 through a 4-deep
// register ring), the next layer's g fused into the epilogue.  The grid is
// (row tiles, background slices): one test row against thousands of
// background rows still fills the chip.  A slice's sum lives in LDS (f32);
// the slices are then added in slice order, in f64, by dl_shap_reduce_kernel
// -- no atomics, so two runs agree bit for bit, and because a slice is always
// DLS_CHUNK rows of the background the sum does not depend on how the caller
// tiles rows or background rows either.  per_ref mode writes every pair's
// values instead.
//
// With few test rows a 16-row tile would be mostly padding, so the caller may
// swap the roles (the rule is antisymmetric: phi(x, z) = -phi(z, x)): the tile
// holds 16 background rows, the loop runs over test rows, and a slice's sum is
// the sum over the tile's rows (4 per lane, then across the 4 lane groups by
// two shuffles) -- again one f32 sum per DLS_CHUNK background rows in a fixed
// order.  Which mapping runs is the caller's choice from the total row counts,
// never from the tiling.
#include "common.h"
#include <algorithm>

enum { DLS_LINEAR = 0, DLS_TANH = 1, DLS_RELU = 2, DLS_ELU = 3 };

#define DLS_MAXL 8
#define DLS_ROWS 16
#define DLS_CHUNK 16            // background rows per slice (fixed: see above)
#define DLS_WAVES 8
#define DLS_THREADS (64 * DLS_WAVES)
#define DLS_TPW 2
#define DLS_LDS_BYTES (160 * 1024)
typedef float dls_f32x4 __attribute__((ext_vector_type(4)));

struct DLShapNet {
  int nl;                        // hidden layers
  int N, B, P;                   // tile-side rows, loop-side rows of this launch; inputs
  int per_ref;
  int swap;                      // the tile rows are background rows, the loop runs over test rows
  int ldS;                       // background rows of this launch (row stride of S)
  int width[DLS_MAXL + 1];       // [0] = inputs, [l] = units of hidden layer l (1-based)
  int act[DLS_MAXL + 1];         // activation of hidden layer l
  float scale[DLS_MAXL + 1];     // its test-time scale
  int lds_a[DLS_MAXL + 1];       // LDS offsets (floats): [0] the input tile, [l] pre-activations of layer l
  int stride[DLS_MAXL + 1];
  int lds_acc;                   // slice sum [16, stride[0]]
  int lds_d0, lds_d1, ldsw;      // multiplier ping-pong buffers and their row stride
  const float* W[DLS_MAXL + 1];  // [l]: [width[l], width[l-1]]
  const float* PX[DLS_MAXL + 1]; // [l]: [N, width[l]]   (tile side: the test rows unless swap)
  const float* PZ[DLS_MAXL + 1]; // [l]: [B, width[l]]   (loop side: the background rows unless swap)
  const float* X;                // [N, P]
  const float* Z;                // [B, P]
  const float* out_w;            // [width[nl]]
  const float* S;                // [test rows, background rows] pair factors or null
  float* partial;                // [background slices, test rows, P] (averaged mode)
  double* out;                   // per_ref: [(row_off + r) * Btot + bg_off + b][P + 1]
  long long row_off, bg_off, Btot;
};

__device__ __forceinline__ dls_f32x4 dls_mfma4(float4 a, float4 b, dls_f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
  return c;
}

__device__ __forceinline__ float dls_act(int act, float z) {
  switch (act) {
    case DLS_TANH: return tanhf(z);
    case DLS_RELU: return fmaxf(z, 0.f);
    case DLS_ELU: return z > 0.f ? z : expm1f(z);
    default: return z;
  }
}

__device__ __forceinline__ float dls_dact(int act, float z) {
  switch (act) {
    case DLS_TANH: { const float t = tanhf(z); return 1.f - t * t; }
    case DLS_RELU: return z > 0.f ? 1.f : 0.f;
    case DLS_ELU: return z > 0.f ? 1.f : expf(z);
    default: return 1.f;
  }
}

// rescale-rule gain of one unit between the pre-activations ax and az.  In f32
// act(ax) - act(az) cancels when the two are close, and the division by d
// amplifies it; tanh and the exponential branch have difference forms without
// the cancellation: tanh(a) - tanh(b) = tanh(a - b) (1 - tanh(a) tanh(b)),
// expm1(a) - expm1(b) = exp(b) expm1(a - b).
__device__ __forceinline__ float dls_gain(int act, float ax, float az, float s) {
  const float d = ax - az;
  if (fabsf(d) < 1e-6f) return s * dls_dact(act, 0.5f * (ax + az));
  float num;
  if (act == DLS_TANH)
    num = tanhf(d) * (1.f - tanhf(ax) * tanhf(az));
  else if (act == DLS_ELU && ax <= 0.f && az <= 0.f)
    num = expf(az) * expm1f(d);
  else
    num = dls_act(act, ax) - dls_act(act, az);
  return s * num / d;
}

__global__ __launch_bounds__(DLS_THREADS) void dl_shap_pairs_kernel(const DLShapNet net) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g4 = 4 * (lane >> 4), c16 = lane & 15;
  const int r0 = blockIdx.x * DLS_ROWS;
  const int N = net.N, P = net.P, nl = net.nl;
  const int bs = blockIdx.y * DLS_CHUNK;
  const int be = min(net.B, bs + DLS_CHUNK);
  const int S0 = net.stride[0];
  float* xs = lds + net.lds_a[0];
  float* accl = lds + net.lds_acc;
  // ---- the workgroup's 16 rows: inputs, pre-activations of every layer
  for (int e = tid; e < DLS_ROWS * S0; e += DLS_THREADS) {
    const int r = e / S0, c = e - r * S0;
    xs[e] = (r0 + r < N && c < P) ? net.X[(long long)(r0 + r) * P + c] : 0.f;
    accl[e] = 0.f;
  }
  for (int l = 1; l <= nl; ++l) {
    const int U = net.width[l], Sl = net.stride[l];
    float* al = lds + net.lds_a[l];
    const float* __restrict__ px = net.PX[l];
    for (int e = tid; e < DLS_ROWS * Sl; e += DLS_THREADS) {
      const int r = e / Sl, c = e - r * Sl;
      al[e] = (r0 + r < N && c < U) ? px[(long long)(r0 + r) * U + c] : 0.f;
    }
  }
  __syncthreads();
  float* dcur = lds + net.lds_d0;
  float* dnext = lds + net.lds_d1;
  const int ldsw = net.ldsw;
  for (int b = bs; b < be; ++b) {
    // ---- multiplier on the last hidden layer's pre-activation: out_w * g
    {
      const int U = net.width[nl], Sl = net.stride[nl];
      const float* al = lds + net.lds_a[nl];
      const float* __restrict__ pz = net.PZ[nl] + (long long)b * U;
      const int act = net.act[nl];
      const float sc = net.scale[nl];
      for (int e = tid; e < DLS_ROWS * ldsw; e += DLS_THREADS) {
        const int r = e / ldsw, u = e - r * ldsw;
        float v = 0.f;
        if (u < U) v = net.out_w[u] * dls_gain(act, al[r * Sl + u], pz[u], sc);
        dcur[e] = v;
      }
    }
    __syncthreads();
    // ---- down through the layers: M_{l-1} = (M_l * g_l) W_l
    for (int l = nl; l >= 1; --l) {
      const int U = net.width[l], I = net.width[l - 1];
      const int NT = (I + 15) >> 4, KP = (U + 15) & ~15;
      const float* __restrict__ W = net.W[l];
      const int nk = KP >> 4;
      // W column slice of tile t (inputs t*16 + c16) at k step ks: rows 16 ks + g4 .. +3
      auto wload = [&](int t, int ks) -> float4 {
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        const int i = t * 16 + c16, kk = ks * 16 + g4;
        if (t < NT && i < I) {
          const float* wc = W + (long long)kk * I + i;
          w.x = kk < U ? wc[0] : 0.f;
          w.y = kk + 1 < U ? wc[I] : 0.f;
          w.z = kk + 2 < U ? wc[2 * I] : 0.f;
          w.w = kk + 3 < U ? wc[3 * I] : 0.f;
        }
        return w;
      };
      // what the epilogue multiplies with: the layer below's gain, or x - z
      const float* al = lds + net.lds_a[l - 1];
      const int Sa = net.stride[l - 1];
      const float* __restrict__ zb = (l > 1 ? net.PZ[l - 1] : net.Z) + (long long)b * I;
      const int act = net.act[l - 1];
      const float sc = net.scale[l - 1];
      for (int t0 = wave; t0 < NT; t0 += DLS_WAVES * DLS_TPW) {
        dls_f32x4 acc[DLS_TPW];
#pragma unroll
        for (int j = 0; j < DLS_TPW; ++j) acc[j] = (dls_f32x4){0.f, 0.f, 0.f, 0.f};
        float4 wq[4][DLS_TPW];
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int j = 0; j < DLS_TPW; ++j)
            wq[d][j] = d < nk ? wload(t0 + DLS_WAVES * j, d) : make_float4(0.f, 0.f, 0.f, 0.f);
        for (int kb = 0; kb < nk; kb += 4) {
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            const int ks = kb + d;
            if (ks < nk) {
              const float4 dv = *reinterpret_cast<const float4*>(dcur + c16 * ldsw + ks * 16 + g4);
#pragma unroll
              for (int j = 0; j < DLS_TPW; ++j)
                if (t0 + DLS_WAVES * j < NT) acc[j] = dls_mfma4(dv, wq[d][j], acc[j]);
              if (ks + 4 < nk) {
#pragma unroll
                for (int j = 0; j < DLS_TPW; ++j) wq[d][j] = wload(t0 + DLS_WAVES * j, ks + 4);
              }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < DLS_TPW; ++j) {
          const int t = t0 + DLS_WAVES * j;
          if (t < NT) {
            const int i = t * 16 + c16;
            const float zv = i < I ? zb[i] : 0.f;
            if (l > 1) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = g4 + r;
                dnext[row * ldsw + i] = i < I ? acc[j][r] * dls_gain(act, al[row * Sa + i], zv, sc) : 0.f;
              }
            } else if (!net.swap) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = g4 + r, rg = r0 + row;
                if (i < I && rg < N) {
                  float ph = acc[j][r] * (al[row * Sa + i] - zv);
                  if (net.S) ph *= net.S[(long long)rg * net.ldS + b];
                  if (net.per_ref)
                    net.out[((net.row_off + rg) * net.Btot + net.bg_off + b) * (P + 1) + i] = (double)ph;
                  else
                    accl[row * S0 + i] += ph;
                }
              }
            } else {
              // tile rows are background rows, b is the test row: phi(x, z) = -phi(z, x)
              float v = 0.f;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int row = g4 + r, rg = r0 + row;
                if (i < I && rg < N) {
                  float ph = acc[j][r] * (zv - al[row * Sa + i]);
                  if (net.S) ph *= net.S[(long long)b * net.ldS + rg];
                  if (net.per_ref)
                    net.out[((net.row_off + b) * net.Btot + net.bg_off + rg) * (P + 1) + i] = (double)ph;
                  else
                    v += ph;
                }
              }
              if (!net.per_ref) {
                // the tile's 16 background rows in a fixed order: 4 per lane, then across the 4 lane groups
                v += __shfl_xor(v, 16, H2O_WAVE);
                v += __shfl_xor(v, 32, H2O_WAVE);
                if (lane < 16 && i < I) net.partial[((long long)blockIdx.x * net.B + b) * P + i] = v;
              }
            }
          }
        }
      }
      __syncthreads();
      float* tmp = dcur;
      dcur = dnext;
      dnext = tmp;
    }
  }
  if (!net.per_ref && !net.swap) {
    float* __restrict__ part = net.partial + (long long)blockIdx.y * N * P;
    for (int e = tid; e < DLS_ROWS * P; e += DLS_THREADS) {
      const int r = e / P, c = e - r * P;
      if (r0 + r < N) part[(long long)(r0 + r) * P + c] = accl[r * S0 + c];
    }
  }
}

// out[row_off + r][i] += sum over the slices, in slice order, in f64
__global__ __launch_bounds__(256) void dl_shap_reduce_kernel(const float* __restrict__ partial, int slices, int N,
                                                             int P, double* __restrict__ out, long long row_off) {
  const long long n = (long long)N * P;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const long long r = e / P;
  const int c = (int)(e - r * P);
  double* o = out + (row_off + r) * (P + 1) + c;
  double a = *o;
  for (int s = 0; s < slices; ++s) a += (double)partial[(long long)s * n + e];
  *o = a;
}

static size_t dl_shap_plan(DLShapNet& net, int nl, const int* width) {
  int off = 0, maxw = 0;
  for (int l = 0; l <= nl; ++l) {
    net.width[l] = width[l];
    const int pw = (width[l] + 15) & ~15;
    net.lds_a[l] = off;
    net.stride[l] = pw + 4;
    off += DLS_ROWS * (pw + 4);
    if (l >= 1) maxw = std::max(maxw, pw);
  }
  net.lds_acc = off;
  off += DLS_ROWS * net.stride[0];
  net.ldsw = maxw + 4;
  net.lds_d0 = off;
  off += DLS_ROWS * net.ldsw;
  net.lds_d1 = off;
  off += DLS_ROWS * net.ldsw;
  return (size_t)off * sizeof(float);
}

// LDS bytes of the plan for width[0 .. nl] (inputs, hidden layers), or -1
// when the network does not fit (more than 8 hidden layers, > 160 KiB)
static long long dl_shap_lds(int nl, const int* width) {
  if (nl < 1 || nl > DLS_MAXL) return -1;
  for (int l = 0; l <= nl; ++l)
    if (width[l] < 1 || width[l] > (1 << 20)) return -1;
  DLShapNet net{};
  const size_t bytes = dl_shap_plan(net, nl, width);
  return bytes <= DLS_LDS_BYTES ? (long long)bytes : -1;
}

extern "C" {

// background rows per slice: a launch with B rows writes ceil(B / chunk) slices
int h2o_dl_shap_chunk() { return DLS_CHUNK; }

// Pair stage for N test rows x B background rows.  width[nl + 1], act[nl],
// scale[nl], W / PX / PZ[nl] per hidden layer (bottom up); S [N, B] or null.
// Averaged mode: partial must hold ceil(B / chunk) * N * P floats; the slice
// sums are ADDED to out[(row_off + r) * (P + 1) + i].  per_ref: out rows are
// (row_off + r) * Btot + bg_off + b.  Returns -2 when the network does not fit.
int h2o_dl_shap_pairs(int nl, const int* width, const int* act, const float* scale, const float* const* W,
                      const float* const* PX, const float* const* PZ, const float* X, const float* Z,
                      const float* out_w, const float* S, int N, int B, float* partial, double* out,
                      long long row_off, long long bg_off, long long Btot, int per_ref, int swap, hipStream_t s) {
  if (N <= 0 || B <= 0) return 0;
  if (dl_shap_lds(nl, width) < 0) return -2;
  DLShapNet net{};
  const size_t lds_bytes = dl_shap_plan(net, nl, width);
  net.nl = nl;
  net.N = swap ? B : N;
  net.B = swap ? N : B;
  net.P = width[0];
  net.per_ref = per_ref;
  net.swap = swap;
  net.ldS = B;
  for (int l = 1; l <= nl; ++l) {
    net.act[l] = act[l - 1];
    net.scale[l] = scale[l - 1];
    net.W[l] = W[l - 1];
    net.PX[l] = swap ? PZ[l - 1] : PX[l - 1];
    net.PZ[l] = swap ? PX[l - 1] : PZ[l - 1];
  }
  net.X = swap ? Z : X;
  net.Z = swap ? X : Z;
  net.out_w = out_w;
  net.S = S;
  net.partial = partial;
  net.out = out;
  net.row_off = row_off;
  net.bg_off = bg_off;
  net.Btot = Btot;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)dl_shap_pairs_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              DLS_LDS_BYTES);
    attr_set = true;
  }
  const int tiles = (net.N + DLS_ROWS - 1) / DLS_ROWS, chunks = (net.B + DLS_CHUNK - 1) / DLS_CHUNK;
  if (chunks > 65535) return -3;
  const int slices = (B + DLS_CHUNK - 1) / DLS_CHUNK;   // of the background: tiles when swapped, else chunks
  hipLaunchKernelGGL(dl_shap_pairs_kernel, dim3(tiles, chunks), dim3(DLS_THREADS), lds_bytes, s, net);
  if (!per_ref) {
    const long long n = (long long)N * net.P;
    hipLaunchKernelGGL(dl_shap_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, partial, slices, N,
                       net.P, out, row_off);
  }
  H2O_CHECK_LAUNCH();
}

}  // extern "C"
