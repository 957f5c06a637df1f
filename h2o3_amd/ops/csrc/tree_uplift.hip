// Uplift DRF split search: the best split of every frontier node under the
// KL / chi-squared / Euclidean divergence between the treatment and the control
// response rates (hex/tree/uplift/Divergence.java and its subclasses;
// TreeGrower._find_splits_torch_core is the definition this file follows
// operation by operation).  Built without contraction so that a product and
// the sum it feeds round as they do in the torch expression.
// hipcc-flags: -ffp-contract=off
//
// Input: the level histogram H [Fl, n, Bs, 4] f64, channels wt, wt*y, wc, wc*y,
// bin Bs-1 the NA bin, B = Bs-1 value bins.  Candidates of one (node, feature)
// pair, in the flat order k of the torch path:
//   A  k in [0, B-1)        bins (in order) <= t left, NA right
//   B  k in [B-1, 2(B-1))   the same with NA left      (only if the NA bin has rows)
//   C  k = 2(B-1)           NA against the rest        (only if the NA bin has rows)
// gain = nl/nt * D(L) + nr/nt * D(R) - D(T), valid when both sides hold
// min_rows rows and rows of both groups, kept when above 1e-12.
//
// MI355X design.  The search is latency bound (a few hundred f64 divisions
// and logarithms per pair, thousands of pairs per level), so the unit of work
// is small and there are many of them:
//   uplift_pair_kernel: ONE WAVE per (node, feature) pair, no workgroup
//     barrier anywhere (waves of a workgroup take different paths: masked
//     pairs leave at once, categorical pairs sort).  The pair's B x 4 bins are
//     staged once in LDS as f64 with a row stride of 5 doubles, so the lanes'
//     reads of one channel of consecutive bins spread over the banks.  A
//     categorical pair sorts (key, bin) with a bitonic network in LDS, key =
//     pt - pc (+inf for an empty bin); comparing the pair makes it the stable
//     order.  Each lane owns a run of ceil(B/64) bins in (sorted) order: it
//     sums its run, four independent f64 wave scans over the 64 lane totals
//     give its start, and a second walk over the run forms L / R of options A
//     and B per threshold; lane 0 adds option C.  A wave arg-max on (gain, k),
//     exact ties to the lowest k, leaves one record per pair:
//     gain, k, L[4], T[4].
//     Two instances: four pairs per 256-thread workgroup while B <= 256, one
//     pair per 64-thread workgroup up to B <= 1024.  The stage is dynamic LDS
//     sized by B rounded up to a power of two (50 B per bin and pair, at most
//     51200 B per workgroup), so a 20-bin histogram keeps a CU full of waves.
//   uplift_select_kernel: one workgroup per node.  Arg-max over the node's
//     Fl records (ties to the lowest feature), the node totals from H[0], the
//     fields of the split record and the go-left byte mask.  For a categorical
//     winner the rank of a bin is RECOMPUTED for that one pair by counting the
//     (key, bin) pairs below it (B^2 / 256 compares per thread, only for the
//     node's winner) instead of keeping a rank table per pair from the first
//     kernel: no [n, Fl, B] table is written for pairs that lose.
// No atomics; every sum has a fixed order, so a call returns the same bits.
#include "common.h"

#define UP_STRIDE 5          // doubles per staged bin: 4 channels + 1 pad
#define UP_REC 10            // doubles per pair record
#define UP_NEG_INF (-__builtin_inf())
#define UP_NO_K 0x7fffffff

// LDS traffic of one wave is ordered by the hardware; this keeps the compiler
// from moving accesses across and waits for the outstanding ones.
__device__ __forceinline__ void up_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ double up_rate(double wy, double w) {
  return fmin(fmax(wy / fmax(w, 1e-300), 1e-6), 1.0 - 1e-6);
}

__device__ __forceinline__ double up_div(const double* S, int crit) {
  if (!(S[0] > 0.0 && S[2] > 0.0)) return 0.0;
  const double pt = up_rate(S[1], S[0]), pc = up_rate(S[3], S[2]);
  if (crit == 0) return pt * log(pt / pc) + (1.0 - pt) * log((1.0 - pt) / (1.0 - pc));
  const double a = pt - pc, b = (1.0 - pt) - (1.0 - pc);
  if (crit == 1) return a * a / pc + b * b / (1.0 - pc);
  return a * a + b * b;
}

__device__ __forceinline__ double up_gain(const double* L, const double* R, double sT, double min_rows, int crit) {
  const double nl = L[0] + L[2], nr = R[0] + R[2];
  if (!(nl >= min_rows && nr >= min_rows && L[0] > 0.0 && L[2] > 0.0 && R[0] > 0.0 && R[2] > 0.0)) return UP_NEG_INF;
  const double nt = fmax(nl + nr, 1e-300);
  const double g = (nl / nt) * up_div(L, crit) + (nr / nt) * up_div(R, crit) - sT;
  return g > 1e-12 ? g : UP_NEG_INF;
}

// sort key of a categorical bin: treatment rate - control rate, empty bins last
__device__ __forceinline__ double up_key(double wt, double wty, double wc, double wcy) {
  if (!(wt + wc > 0.0)) return __builtin_inf();
  return wty / fmax(wt, 1e-300) - wcy / fmax(wc, 1e-300);
}

// (ka, ia) before (kb, ib): ascending key, NaN after everything, then ascending bin
__device__ __forceinline__ bool up_less(double ka, int ia, double kb, int ib) {
  const bool na = ka != ka, nb = kb != kb;
  if (na || nb) return na == nb ? ia < ib : nb;
  return ka < kb || (ka == kb && ia < ib);
}

// LDS of one pair, sized by P2 = B rounded up to a power of two (dynamic, so a
// narrow histogram leaves room for more resident waves): bins [P2][5] f64,
// key [P2] f64, perm [P2] u16.
static inline int up_pow2(int B) {
  int p = 4;
  while (p < B) p <<= 1;
  return p;
}
static inline size_t up_stage_doubles(int P2) { return (size_t)P2 * (UP_STRIDE + 1) + P2 / 4; }

template <int WAVES>
__global__ __launch_bounds__(WAVES* H2O_WAVE) void uplift_pair_kernel(
    const double* __restrict__ H, int Fl, int n, int Bs, const uint8_t* __restrict__ ok,
    const uint8_t* __restrict__ is_cat, int f0, int F, double min_rows, int crit, int P2, double* __restrict__ rec) {
  extern __shared__ double up_lds[];
  const long long pair = (long long)blockIdx.x * WAVES + wave_id();
  if (pair >= (long long)n * Fl) return;
  const int node = (int)(pair / Fl), f = (int)(pair % Fl);
  const int lane = lane_id();
  double* r = rec + pair * UP_REC;
  if (f0 + f >= F || !ok[pair]) {
    if (lane < UP_REC) r[lane] = lane == 0 ? UP_NEG_INF : 0.0;
    return;
  }
  double* sm_bins = up_lds + (size_t)wave_id() * ((size_t)P2 * (UP_STRIDE + 1) + P2 / 4);
  double* sm_key = sm_bins + (size_t)P2 * UP_STRIDE;
  unsigned short* sm_perm = (unsigned short*)(sm_key + P2);
  const int B = Bs - 1;
  const double* h = H + ((long long)f * n + node) * Bs * 4;
  for (int i = lane; i < B * 4; i += H2O_WAVE) sm_bins[(i >> 2) * UP_STRIDE + (i & 3)] = h[i];
  double na[4];
#pragma unroll
  for (int c = 0; c < 4; c++) na[c] = h[B * 4 + c];
  const bool cat = is_cat[f] != 0;
  up_wave_sync();

  if (cat) {
    for (int i = lane; i < P2; i += H2O_WAVE) {
      const double* b = sm_bins + i * UP_STRIDE;
      sm_key[i] = i < B ? up_key(b[0], b[1], b[2], b[3]) : __builtin_nan("");
      sm_perm[i] = (unsigned short)i;
    }
    up_wave_sync();
    for (int k = 2; k <= P2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int p = lane; p < (P2 >> 1); p += H2O_WAVE) {
          const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), x = i | j;
          const double ki = sm_key[i], kx = sm_key[x];
          const int pi = sm_perm[i], px = sm_perm[x];
          const bool up = (i & k) == 0;
          if (up ? up_less(kx, px, ki, pi) : up_less(ki, pi, kx, px)) {
            sm_key[i] = kx, sm_key[x] = ki;
            sm_perm[i] = (unsigned short)px, sm_perm[x] = (unsigned short)pi;
          }
        }
        up_wave_sync();
      }
  }

  // lane totals of a contiguous run, then a wave scan per channel
  const int run = (B + H2O_WAVE - 1) / H2O_WAVE;
  const int j0 = min(lane * run, B), j1 = min(j0 + run, B);
  double inc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = j0; j < j1; j++) {
    const double* b = sm_bins + (cat ? (int)sm_perm[j] : j) * UP_STRIDE;
#pragma unroll
    for (int c = 0; c < 4; c++) inc[c] += b[c];
  }
#pragma unroll
  for (int o = 1; o < H2O_WAVE; o <<= 1) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const double v = __shfl_up(inc[c], o, H2O_WAVE);
      if (lane >= o) inc[c] += v;
    }
  }
  double cum[4], totnn[4], T[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const double v = __shfl_up(inc[c], 1, H2O_WAVE);
    cum[c] = lane == 0 ? 0.0 : v;
    totnn[c] = __shfl(inc[c], H2O_WAVE - 1, H2O_WAVE);
    T[c] = totnn[c] + na[c];
  }
  const double sT = up_div(T, crit);
  const bool has_na = na[0] + na[2] > 0.0;

  double bg = UP_NEG_INF, bL[4] = {0.0, 0.0, 0.0, 0.0};
  int bk = UP_NO_K;
  auto consider = [&](double g, int k, const double* L) {
    if (g > bg || (g == bg && k < bk)) {
      bg = g, bk = k;
#pragma unroll
      for (int c = 0; c < 4; c++) bL[c] = L[c];
    }
  };
  for (int j = j0; j < j1; j++) {
    const double* b = sm_bins + (cat ? (int)sm_perm[j] : j) * UP_STRIDE;
#pragma unroll
    for (int c = 0; c < 4; c++) cum[c] += b[c];
    if (j >= B - 1) break;
    double L2[4], R2[4];
#pragma unroll
    for (int c = 0; c < 4; c++) R2[c] = (totnn[c] - cum[c]) + na[c];
    consider(up_gain(cum, R2, sT, min_rows, crit), j, cum);
    if (has_na) {      // without NA rows every B candidate is -inf and loses the tie to k = 0
#pragma unroll
      for (int c = 0; c < 4; c++) L2[c] = cum[c] + na[c], R2[c] = totnn[c] - cum[c];
      consider(up_gain(L2, R2, sT, min_rows, crit), (B - 1) + j, L2);
    }
  }
  if (lane == 0) consider(has_na ? up_gain(totnn, na, sT, min_rows, crit) : UP_NEG_INF, 2 * (B - 1), totnn);

  const int myk = bk;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double og = __shfl_xor(bg, o, H2O_WAVE);
    const int ok_ = __shfl_xor(bk, o, H2O_WAVE);
    if (og > bg || (og == bg && ok_ < bk)) bg = og, bk = ok_;
  }
  if (myk == bk) {     // candidate indices are distinct over the lanes, lane 0 always holds one
    r[0] = bg, r[1] = (double)bk;
#pragma unroll
    for (int c = 0; c < 4; c++) r[2 + c] = bL[c], r[6 + c] = T[c];
  }
}

#define UP_SEL_THREADS 256
#define UP_SEL_BMAX 1024

// fout: gain [n], L [n,4], R [n,4], tot [n,4]; iout: feat [n], t [n], opt [n]
__global__ __launch_bounds__(UP_SEL_THREADS) void uplift_select_kernel(
    const double* __restrict__ rec, const double* __restrict__ H, int Fl, int n, int Bs,
    const uint8_t* __restrict__ is_cat, int f0, double* __restrict__ fout, long long* __restrict__ iout,
    uint8_t* __restrict__ na_left_out, uint8_t* __restrict__ mask) {
  __shared__ double sg[UP_SEL_THREADS];
  __shared__ int sf[UP_SEL_THREADS];
  __shared__ double skey[UP_SEL_BMAX];
  const int node = blockIdx.x, tid = threadIdx.x, B = Bs - 1;

  // node totals: H[0, node] over all bins; a thread's elements share one channel (256 % 4 == 0)
  const double* h0 = H + (long long)node * Bs * 4;
  double part = 0.0;
  for (int i = tid; i < Bs * 4; i += UP_SEL_THREADS) part += h0[i];
  sg[tid] = part;
  __syncthreads();
  for (int s = UP_SEL_THREADS / 2; s >= 4; s >>= 1) {
    if (tid < s) sg[tid] += sg[tid + s];
    __syncthreads();
  }
  const double tot_c = sg[tid & 3];
  __syncthreads();

  // best record, lowest feature on ties
  const double* rn = rec + (long long)node * Fl * UP_REC;
  double g = UP_NEG_INF;
  int fb = UP_NO_K;
  for (int f = tid; f < Fl; f += UP_SEL_THREADS) {
    const double v = rn[(long long)f * UP_REC];
    if (v > g || fb == UP_NO_K) g = v, fb = f;
  }
  sg[tid] = g, sf[tid] = fb;
  __syncthreads();
  for (int s = UP_SEL_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double og = sg[tid + s];
      const int of = sf[tid + s];
      if (of != UP_NO_K && (sf[tid] == UP_NO_K || og > sg[tid] || (og == sg[tid] && of < sf[tid])))
        sg[tid] = og, sf[tid] = of;
    }
    __syncthreads();
  }
  const int fl = sf[0];
  const double* w = rn + (long long)fl * UP_REC;
  const int k = (int)w[1], nt = B - 1;
  const int opt = k < nt ? 0 : (k < 2 * nt ? 1 : 2);
  const int t = opt == 0 ? k : (opt == 1 ? k - nt : 0);
  const bool na_left = opt == 1;

  if (tid == 0) {
    fout[node] = w[0];
    iout[node] = f0 + fl, iout[(long long)n + node] = t, iout[2LL * n + node] = opt;
    na_left_out[node] = na_left;
  }
  if (tid < 4) {
    double* L = fout + n + (long long)node * 4;
    double* R = fout + 5LL * n + (long long)node * 4;
    L[tid] = w[2 + tid], R[tid] = w[6 + tid] - w[2 + tid];
    fout[9LL * n + (long long)node * 4 + tid] = tot_c;
  }

  uint8_t* m = mask + (long long)node * Bs;
  if (tid == 0) m[B] = na_left;
  if (!is_cat[fl]) {
    for (int b = tid; b < B; b += UP_SEL_THREADS) m[b] = opt == 2 || b <= t;
    return;
  }
  // categorical winner: rank of a bin = number of (key, bin) pairs below it
  const double* hw = H + ((long long)fl * n + node) * Bs * 4;
  for (int b = tid; b < B; b += UP_SEL_THREADS) skey[b] = up_key(hw[b * 4], hw[b * 4 + 1], hw[b * 4 + 2], hw[b * 4 + 3]);
  __syncthreads();
  for (int b = tid; b < B; b += UP_SEL_THREADS) {
    const bool empty = !(hw[b * 4] + hw[b * 4 + 2] > 0.0);
    bool left;
    if (empty) left = na_left;
    else if (opt == 2) left = true;
    else {
      const double kb = skey[b];
      int rank = 0;
      for (int o = 0; o < B; o++) rank += up_less(skey[o], o, kb, b) ? 1 : 0;
      left = rank <= t;
    }
    m[b] = left;
  }
}

// One record [gain, k, L[4], T[4]] per (node, local feature) pair into rec [n, Fl, 10].
// ok [n, Fl]: eligible pairs; is_cat [Fl]; crit: 0 KL, 1 chi-squared, 2 Euclidean.
extern "C" int h2o_uplift_pairs(const double* H, int Fl, int n, int Bs, const uint8_t* ok, const uint8_t* is_cat, int f0,
                                int F, double min_rows, int crit, double* rec, hipStream_t s) {
  if (Fl <= 0 || n <= 0) return 0;
  const int B = Bs - 1;
  if (B < 1 || B > 1024 || crit < 0 || crit > 2) return (int)hipErrorInvalidValue;
  const long long pairs = (long long)n * Fl;
  const int P2 = up_pow2(B);
  const size_t lds = up_stage_doubles(P2) * sizeof(double);      // <= 51200 B at P2 = 1024
  if (B <= 256)
    hipLaunchKernelGGL((uplift_pair_kernel<4>), dim3((unsigned)((pairs + 3) / 4)), dim3(256), 4 * lds, s, H, Fl, n, Bs, ok,
                       is_cat, f0, F, min_rows, crit, P2, rec);
  else
    hipLaunchKernelGGL((uplift_pair_kernel<1>), dim3((unsigned)pairs), dim3(64), lds, s, H, Fl, n, Bs, ok, is_cat, f0, F,
                       min_rows, crit, P2, rec);
  H2O_CHECK_LAUNCH();
}

// The split record of every node from the pair records; mask [n, Bs] go-left bytes.
extern "C" int h2o_uplift_select(const double* rec, const double* H, int Fl, int n, int Bs, const uint8_t* is_cat, int f0,
                                 double* fout, long long* iout, uint8_t* na_left, uint8_t* mask, hipStream_t s) {
  if (Fl <= 0 || n <= 0) return 0;
  if (Bs < 2 || Bs - 1 > UP_SEL_BMAX) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(uplift_select_kernel, dim3(n), dim3(UP_SEL_THREADS), 0, s, rec, H, Fl, n, Bs, is_cat, f0, fout, iout,
                     na_left, mask);
  H2O_CHECK_LAUNCH();
}
