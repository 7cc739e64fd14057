// Fusion-head epilogues, the fused MC-head reductions, and small reductions.
//
//  * AdditiveAttention (models/base_models.py:43-52): with q|k|v produced by ONE linear over
//    the concatenated [Wq;Wk;Wv] sample (N = 384), the epilogues are
//       t = tanh(q + k)                        (attn_t)
//       s = Wm t + bm                          (linear, conv_gemm.hip 1x1 path)
//       a = softmax(s, dim=1);  o = v * a      (attn_out; o written into the concat slot)
//  * MC head (train/multimodal.py:121-127, :287-310; inference/predictors.py:65-84):
//       mean over MC of logits + cross-entropy (+ backward), and the sufficient statistics
//       sum_g p, sum_g p^2, sum_g H[p_g] -> mean prob, unbiased variance, aleatoric
//       entropy, predictive entropy, argmax.  Partial sums are shardable across GPUs
//       (MC-sharded inference: one all-reduce of [B,2C+1] doubles).
#include "mauv_common.h"

using namespace mauv;

namespace mauv {

// qkv rows are [q | k | v], each `hid` wide (the reference model: hid = 128, d_model 2048)
__global__ __launch_bounds__(256) void attn_t_kernel(const float* __restrict__ qkv, int rows,
                                                     int hid, float* __restrict__ t) {
  const long long total = (long long)rows * hid;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / hid;
    const int j = (int)(i - r * hid);
    t[i] = tanhf(qkv[r * 3 * hid + j] + qkv[r * 3 * hid + hid + j]);
  }
}

__global__ __launch_bounds__(256) void attn_t_bwd_kernel(const float* __restrict__ dt,
                                                         const float* __restrict__ t, int rows,
                                                         int hid, float* __restrict__ dqkv) {
  const long long total = (long long)rows * hid;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / hid;
    const int j = (int)(i - r * hid);
    const float tv = t[i];
    const float d = dt[i] * (1.0f - tv * tv);
    dqkv[r * 3 * hid + j] = d;
    dqkv[r * 3 * hid + hid + j] = d;
  }
}

// softmax over the hidden dim of one row, one wave per row (lane j covers j, j+64, ...):
// returns the row max and 1 / sum exp(s - max)
__device__ __forceinline__ void row_softmax_norm(const float* __restrict__ s, int hid, int lane,
                                                 float& m, float& inv) {
  m = -INFINITY;
  for (int j = lane; j < hid; j += 64) m = fmaxf(m, s[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float e = 0.f;
  for (int j = lane; j < hid; j += 64) e += expf(s[j] - m);
  inv = 1.0f / wave_sum(e);
}

__global__ __launch_bounds__(256) void attn_out_kernel(const float* __restrict__ qkv,
                                                       const float* __restrict__ s, int rows,
                                                       int hid, float* __restrict__ comb,
                                                       int comb_ld, int comb_off) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* sr = s + (long long)r * hid;
  float m, inv;
  row_softmax_norm(sr, hid, lane, m, inv);
  const float* v = qkv + (long long)r * 3 * hid + 2 * hid;
  float* o = comb + (long long)r * comb_ld + comb_off;
  for (int j = lane; j < hid; j += 64) o[j] = v[j] * (expf(sr[j] - m) * inv);
}

__global__ __launch_bounds__(256) void attn_out_bwd_kernel(const float* __restrict__ dcomb,
                                                           int comb_ld, int comb_off,
                                                           const float* __restrict__ qkv,
                                                           const float* __restrict__ s, int rows,
                                                           int hid, float* __restrict__ dqkv,
                                                           float* __restrict__ ds) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* sr = s + (long long)r * hid;
  float m, inv;
  row_softmax_norm(sr, hid, lane, m, inv);
  const float* v = qkv + (long long)r * 3 * hid + 2 * hid;
  const float* d = dcomb + (long long)r * comb_ld + comb_off;
  float* dv = dqkv + (long long)r * 3 * hid + 2 * hid;
  float dot = 0.f;
  for (int j = lane; j < hid; j += 64) {
    const float a = expf(sr[j] - m) * inv;
    dv[j] = d[j] * a;
    dot += a * d[j] * v[j];
  }
  dot = wave_sum(dot);
  for (int j = lane; j < hid; j += 64) {
    const float a = expf(sr[j] - m) * inv;
    ds[(long long)r * hid + j] = a * (d[j] * v[j] - dot);
  }
}

// out[g][n] (+)= sum_rows dy[g][row][n]
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ dy, int G,
                                                     int rows, int N, float* __restrict__ out,
                                                     int accumulate) {
  const long long total = (long long)G * N;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long g = i / N;
    const int n = (int)(i - g * N);
    const float* src = dy + g * rows * (long long)N + n;
    float acc = 0.f;
    for (int r = 0; r < rows; ++r) acc += src[(long long)r * N];
    out[i] = accumulate ? out[i] + acc : acc;
  }
}

// mean over G of logits [G][B][C] -> [B][C]; optional cross-entropy with int64 labels.
__global__ __launch_bounds__(256) void mc_mean_ce_kernel(const float* __restrict__ logits,
                                                         const long long* __restrict__ labels,
                                                         int G, int B, int C,
                                                         float* __restrict__ mean,
                                                         float* __restrict__ loss,
                                                         long long* __restrict__ pred) {
  __shared__ float red[256];
  float acc = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    float m = -INFINITY;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      float s = 0.f;
      for (int g = 0; g < G; ++g) s += logits[((long long)g * B + b) * C + c];
      s = s / (float)G;
      mean[(long long)b * C + c] = s;
      if (s > m) { m = s; arg = c; }
    }
    if (pred) pred[b] = arg;
    if (labels) {
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(mean[(long long)b * C + c] - m);
      acc += (logf(se) + m) - mean[(long long)b * C + labels[b]];
    }
  }
  if (!labels) return;
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] / (float)B;
}

// dlogits[g][b][c] = (dmean[b][c] or g_loss*(softmax(mean)-onehot)/B) / G
__global__ __launch_bounds__(256) void mc_mean_bwd_kernel(const float* __restrict__ dmean,
                                                          const float* __restrict__ gloss,
                                                          const float* __restrict__ mean,
                                                          const long long* __restrict__ labels,
                                                          int G, int B, int C,
                                                          float* __restrict__ dlogits) {
  for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
    float d[32];
    if (labels) {
      float m = -INFINITY;
      for (int c = 0; c < C; ++c) m = fmaxf(m, mean[(long long)b * C + c]);
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(mean[(long long)b * C + c] - m);
      const float gl = gloss ? gloss[0] : 1.0f;
      for (int c = 0; c < C; ++c) {
        const float p = expf(mean[(long long)b * C + c] - m) / se;
        d[c] = gl * (p - (labels[b] == c ? 1.f : 0.f)) / (float)B;
      }
    } else {
      for (int c = 0; c < C; ++c) d[c] = dmean[(long long)b * C + c];
    }
    for (int g = 0; g < G; ++g)
      for (int c = 0; c < C; ++c) dlogits[((long long)g * B + b) * C + c] = d[c] / (float)G;
  }
}

// sums layout per item b: [sum_p (C)][sum_p2 (C)][sum_H] doubles, stride 2C+1.
__global__ __launch_bounds__(256) void mc_stats_kernel(const float* __restrict__ logits, int G,
                                                       int B, int C, float eps_h,
                                                       double* __restrict__ sums,
                                                       int accumulate) {
  for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
    double sp[32], sp2[32], sh = 0.0;
    for (int c = 0; c < C; ++c) { sp[c] = 0.0; sp2[c] = 0.0; }
    for (int g = 0; g < G; ++g) {
      const float* l = logits + ((long long)g * B + b) * C;
      float m = -INFINITY;
      for (int c = 0; c < C; ++c) m = fmaxf(m, l[c]);
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(l[c] - m);
      float h = 0.f;
      for (int c = 0; c < C; ++c) {
        const float p = expf(l[c] - m) / se;
        sp[c] += p;
        sp2[c] += (double)p * p;
        h -= p * logf(p + eps_h);
      }
      sh += h;
    }
    double* o = sums + (long long)b * (2 * C + 1);
    for (int c = 0; c < C; ++c) {
      o[c] = (accumulate ? o[c] : 0.0) + sp[c];
      o[C + c] = (accumulate ? o[C + c] : 0.0) + sp2[c];
    }
    o[2 * C] = (accumulate ? o[2 * C] : 0.0) + sh;
  }
}

__global__ __launch_bounds__(256) void mc_finalize_kernel(const double* __restrict__ sums, int N,
                                                          int B, int C, float eps_pred,
                                                          float* __restrict__ mean_prob,
                                                          float* __restrict__ var_unc,
                                                          float* __restrict__ alea,
                                                          float* __restrict__ pred_entropy,
                                                          long long* __restrict__ pred) {
  for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
    const double* s = sums + (long long)b * (2 * C + 1);
    double vsum = 0.0, H = 0.0;
    int arg = 0;
    float best = -INFINITY;
    for (int c = 0; c < C; ++c) {
      const double pm = s[c] / N;
      const float pmf = (float)pm;
      if (mean_prob) mean_prob[(long long)b * C + c] = pmf;
      vsum += (s[C + c] - N * pm * pm) / (double)(N - 1);
      H -= (double)pmf * log((double)pmf + (double)eps_pred);
      if (pmf > best) { best = pmf; arg = c; }
    }
    if (var_unc) var_unc[b] = (float)(vsum / C);
    if (alea) alea[b] = (float)(s[2 * C] / N);
    if (pred_entropy) pred_entropy[b] = (float)H;
    if (pred) pred[b] = arg;
  }
}

// ---------------------------------------------------------------------------------------------
// The many-class MC head (kSmallClasses < C <= kMaxClasses).  The kernels above give a thread one
// item and walk its C logits, which fits C = 7; here lanes run along the class axis (coalesced
// loads of logits[g][b][0..C)), a wave or a block owns an item, and the row maximum, the sum of
// exponentials and the argmax are cross-lane reductions in a fixed order.  No float atomics:
// every output is bit-reproducible from run to run.  mauv_mc_mean_ce_ex / _bwd_ex run these
// kernels at every C from 1 (a wave holds a row of C <= 64 as well as one of 33).
constexpr int kSmallClasses = 32;   // up to here: the one-thread-per-item kernels above
constexpr int kMaxClasses = 4096;   // the bound mauv_confusion_update has
// Labels of the many-class head: -100 (torch's ignore_index) leaves the item out of the loss sum
// and of its divisor and zeroes its dlogits rows; any other label outside [0, C) makes the loss
// (and the item's dlogits) NaN.  No label indexes memory unchecked.
constexpr long long kIgnoreLabel = -100;
// The criterion of the many-class cross-entropy (torch's CrossEntropyLoss arguments).  kPlainCe is
// CrossEntropyLoss(): with it every expression below multiplies by exactly 1.0 or is skipped on a
// block-uniform branch, so mauv_mc_mean_ce / _bwd keep their bits.
struct CeCrit {
  const float* weight;   // [C] class weights, null = all ones
  float eps;             // label_smoothing in [0, 1]
  int sum;               // reduction: 0 = mean (divisor: the counted labels' weights), 1 = sum
  long long ignore;      // ignore_index: compared before the range check, so it may be a class
};
constexpr CeCrit kPlainCe = {nullptr, 0.f, 0, kIgnoreLabel};

struct ArgBest {
  float v;
  int i;
};
// first strict maximum: the larger value wins, equal values go to the lower class index; a NaN
// never wins because `>` never takes it into a thread's (v, i) in the first place
__device__ __forceinline__ ArgBest arg_better(ArgBest a, ArgBest b) {
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ ArgBest wave_argmax(ArgBest a) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ArgBest b;
    b.v = __shfl_xor(a.v, o, 64);
    b.i = __shfl_xor(a.i, o, 64);
    a = arg_better(a, b);
  }
  return a;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Block-wide reductions of U independent values over NW waves: butterfly inside the wave, one
// LDS slot per (value, wave), one barrier, then every thread folds the NW slots in slot order,
// so all threads end with the same bits.  A slot array is written once per caller iteration and
// every caller iteration has a later barrier between its reads and the next write.
template <int NW, int U>
__device__ __forceinline__ void block_max_u(float (&v)[U], float (*slot)[NW]) {
#pragma unroll
  for (int u = 0; u < U; ++u) v[u] = wave_max(v[u]);
  if (NW == 1) return;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int u = 0; u < U; ++u) slot[u][threadIdx.x >> 6] = v[u];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    float r = slot[u][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r = fmaxf(r, slot[u][w]);
    v[u] = r;
  }
}
template <int NW, int U, typename T>
__device__ __forceinline__ void block_sum_u(T (&v)[U], T (*slot)[NW]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[u] += __shfl_xor(v[u], o, 64);
  }
  if (NW == 1) return;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int u = 0; u < U; ++u) slot[u][threadIdx.x >> 6] = v[u];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < U; ++u) {
    T r = slot[u][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r += slot[u][w];
    v[u] = r;
  }
}

// mean over G: float64 sum over g = 0..G-1, rounded once; elementwise over [B][C].
__global__ __launch_bounds__(256) void mc_mean_wide_kernel(const float* __restrict__ logits,
                                                           int G, long long BC,
                                                           float* __restrict__ mean) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < BC; i += (long long)gridDim.x * 256) {
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)logits[g * BC + i];
    mean[i] = (float)(s / (double)G);
  }
}

// argmax and cross-entropy of the [B][C] mean: ONE block (the loss is one fixed-order sum), a
// wave per item (items w, w + NW, ...) holding the row in registers (C <= 64 * KT, lane l owns
// classes l + 64 k), per-item terms and their sum in float64, rounded to float once.  With
// lp = log_softmax(row), y the label and w the class weights, a counted item (y != cr.ignore) adds
//   nll = -w[y] lp[y],   smooth = -sum_c w[c] lp[c] (only when eps > 0),   D += w[y]
// and loss = (1 - eps) nll / D + (eps / C) smooth / D with D = 1 for the sum reduction (torch
// divides the two parts separately: no counted weight is 0 / 0 = NaN in both).  A label outside
// [0, C) adds NaN to nll and nothing to D.  The weights are read in the row's lane pattern.
template <int KT, int NT>
__global__ __launch_bounds__(NT) void mc_ce_wide_kernel(const float* __restrict__ mean,
                                                          const long long* __restrict__ labels,
                                                          int B, int C, CeCrit cr,
                                                          float* __restrict__ loss,
                                                          float* __restrict__ denom,
                                                          long long* __restrict__ pred) {
  constexpr int NW = NT / 64;
  __shared__ double sacc[3][NW];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double nll = 0.0, smooth = 0.0, den = 0.0;
  for (int b = w; b < B; b += NW) {   // wave-uniform control flow throughout
    const float* row = mean + (long long)b * C;
    float x[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) x[k] = lane + 64 * k < C ? row[lane + 64 * k] : -INFINITY;
    ArgBest best = {-INFINITY, 0};
#pragma unroll
    for (int k = 0; k < KT; ++k)
      if (x[k] > best.v) { best.v = x[k]; best.i = lane + 64 * k; }
    best = wave_argmax(best);
    if (pred && lane == 0) pred[b] = best.i;
    if (!labels) continue;
    const long long y = labels[b];
    if (y == cr.ignore) continue;
    const float m = best.v;   // the maximum over the non-NaN entries (-inf if there is none)
    double se = 0.0;
#pragma unroll
    for (int k = 0; k < KT; ++k) se += (double)expf(x[k] - m);
    se = wave_sum_d(se);
    const double lse = log(se);
    if (y < 0 || y >= C) {
      nll += (double)NAN;
    } else {
      const double wy = cr.weight ? (double)cr.weight[y] : 1.0;
      nll += wy * (lse - ((double)row[y] - (double)m));
      den += wy;
    }
    if (cr.eps > 0.f) {
      // a rolled loop over the cache-resident row: the registers of x[] end with the loop above
      double s = 0.0;
#pragma unroll 2
      for (int c = lane; c < C; c += 64)
        s += (cr.weight ? (double)cr.weight[c] : 1.0) * (lse - ((double)row[c] - (double)m));
      smooth += wave_sum_d(s);
    }
  }
  if (!labels) return;
  if (lane == 0) { sacc[0][w] = nll; sacc[1][w] = smooth; sacc[2][w] = den; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = sacc[0][0], s = sacc[1][0], d = sacc[2][0];
    for (int i = 1; i < NW; ++i) { a += sacc[0][i]; s += sacc[1][i]; d += sacc[2][i]; }
    if (cr.sum) d = 1.0;
    a /= d;   // mean reduction, no counted weight: 0 / 0 = NaN, as torch
    if (cr.eps > 0.f) a = (1.0 - (double)cr.eps) * a + ((double)cr.eps / (double)C) * (s / d);
    loss[0] = (float)a;
    if (denom) denom[0] = (float)d;
  }
}

// dlogits[g][b][c] = (dmean[b][c] or dloss/dmean[b][c]) / G; block per (item, g), the softmax
// normalisers recomputed per block from the cache-resident mean.  With p = softmax(mean[b]),
// W = sum_c w[c] (one block sum per launch, only when eps > 0) and D the forward's divisor
// (`denom`; null: the number of counted labels, which is D of kPlainCe):
//   dloss/dmean[b][c] = g_loss / D ((1 - eps) w[y] (p[c] - [c == y]) + (eps / C) (p[c] W - w[c]))
// zero for an ignored item, NaN for a label outside [0, C).
__global__ __launch_bounds__(256) void mc_mean_bwd_wide_kernel(const float* __restrict__ dmean,
                                                               const float* __restrict__ gloss,
                                                               const float* __restrict__ mean,
                                                               const long long* __restrict__ labels,
                                                               int G, int B, int C, CeCrit cr,
                                                               const float* __restrict__ denom,
                                                               float* __restrict__ dlogits) {
  __shared__ float smax[1][4], ssum[1][4];
  __shared__ int scnt[1][4];
  __shared__ double swsum[1][4];
  const float fG = (float)G;
  int counted[1] = {0};
  if (labels && !denom) {
    for (int b = threadIdx.x; b < B; b += 256) counted[0] += labels[b] != cr.ignore;
    block_sum_u<4, 1, int>(counted, scnt);
  }
  const bool smoothed = labels && cr.eps > 0.f;
  float W = (float)C;
  if (smoothed && cr.weight) {
    double ws[1] = {0.0};
    for (int c = threadIdx.x; c < C; c += 256) ws[0] += (double)cr.weight[c];
    block_sum_u<4, 1, double>(ws, swsum);
    W = (float)ws[0];
  }
  const float D = !labels ? 1.f : denom ? denom[0] : (float)counted[0];
  const float se_c = cr.eps / (float)C;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {   // block-uniform control flow throughout
    for (int g = blockIdx.y; g < G; g += gridDim.y) {
      float* out = dlogits + ((long long)g * B + b) * C;
      if (!labels) {
        const float* d = dmean + (long long)b * C;
        for (int c = threadIdx.x; c < C; c += 256) out[c] = d[c] / fG;
        continue;
      }
      const long long y = labels[b];
      if (y == cr.ignore) {
        for (int c = threadIdx.x; c < C; c += 256) out[c] = 0.f;
        continue;
      }
      const float* x = mean + (long long)b * C;
      float m[1] = {-INFINITY};
      for (int c = threadIdx.x; c < C; c += 256) m[0] = fmaxf(m[0], x[c]);
      block_max_u<4, 1>(m, smax);
      float se[1] = {0.f};
      for (int c = threadIdx.x; c < C; c += 256) se[0] += expf(x[c] - m[0]);
      block_sum_u<4, 1, float>(se, ssum);
      const bool bad = y < 0 || y >= C;
      const float k = bad ? NAN : (gloss ? gloss[0] : 1.0f) / D;
      const float a = (1.f - cr.eps) * (cr.weight && !bad ? cr.weight[y] : 1.f);
      for (int c = threadIdx.x; c < C; c += 256) {
        const float p = expf(x[c] - m[0]) / se[0];
        float t = a * (p - (y == c ? 1.f : 0.f));
        if (smoothed) t += se_c * (p * W - (cr.weight ? cr.weight[c] : 1.f));
        out[c] = k * t / fG;
      }
    }
  }
}

// sums[b] = {sum_g p (C), sum_g p^2 (C), sum_g H[p_g]}.  A block of NT threads owns an item;
// thread t owns classes t + k * NT (k < KT, C <= NT * KT) and keeps their float64 accumulators in
// registers, starting from the previous contents of `sums` when accumulating and adding the
// samples g = 0..G-1 in order, so a chunked call sequence gives the bits of one call.  Samples
// are taken U at a time (their softmax reductions are independent and share a barrier), and the
// next U rows are loaded while the current ones are reduced.
template <int NT, int KT, int U>
__global__ __launch_bounds__(NT) void mc_stats_wide_kernel(const float* __restrict__ logits,
                                                           int G, int B, int C, float eps_h,
                                                           double* __restrict__ sums,
                                                           int accumulate) {
  constexpr int NW = NT / 64;
  __shared__ float smax[U][NW], ssum[U][NW];
  __shared__ double sent[U][NW];
  const long long BC = (long long)B * C;
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    double* o = sums + (long long)b * (2 * C + 1);
    double sp[KT], sp2[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const int c = threadIdx.x + k * NT;
      const bool live = accumulate && c < C;
      sp[k] = live ? o[c] : 0.0;
      sp2[k] = live ? o[C + c] : 0.0;
    }
    double sh = accumulate ? o[2 * C] : 0.0;
    const float* row = logits + (long long)b * C;
    float nx[U][KT];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < KT; ++k) {
        const int c = threadIdx.x + k * NT;
        nx[u][k] = (u < G && c < C) ? row[u * BC + c] : -INFINITY;
      }
    for (int g0 = 0; g0 < G; g0 += U) {
      float x[U][KT];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int k = 0; k < KT; ++k) x[u][k] = nx[u][k];
      if (g0 + U < G) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int k = 0; k < KT; ++k) {
            const int c = threadIdx.x + k * NT;
            nx[u][k] = (g0 + U + u < G && c < C) ? row[(g0 + U + u) * BC + c] : -INFINITY;
          }
      }
      float m[U], se[U];
      double h[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        m[u] = x[u][0];
#pragma unroll
        for (int k = 1; k < KT; ++k) m[u] = fmaxf(m[u], x[u][k]);
      }
      block_max_u<NW, U>(m, smax);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        se[u] = 0.f;
#pragma unroll
        for (int k = 0; k < KT; ++k) {
          x[u][k] = expf(x[u][k] - m[u]);   // a padding class: exp(-inf) = 0
          se[u] += x[u][k];
        }
      }
      block_sum_u<NW, U, float>(se, ssum);
#pragma unroll
      for (int u = 0; u < U; ++u) {   // ascending g: the per-class order of the float64 sums
        h[u] = 0.0;
        if (g0 + u < G) {
#pragma unroll
          for (int k = 0; k < KT; ++k) {
            const float p = x[u][k] / se[u];
            if (threadIdx.x + k * NT < C) {
              sp[k] += (double)p;
              sp2[k] += (double)p * (double)p;
              h[u] -= (double)(p * logf(p + eps_h));
            }
          }
        }
      }
      block_sum_u<NW, U, double>(h, sent);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (g0 + u < G) sh += h[u];
    }
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      const int c = threadIdx.x + k * NT;
      if (c < C) { o[c] = sp[k]; o[C + c] = sp2[k]; }
    }
    if (threadIdx.x == 0) o[2 * C] = sh;
  }
}

// mc_finalize with lanes along the classes; block per item.
__global__ __launch_bounds__(256) void mc_finalize_wide_kernel(const double* __restrict__ sums,
                                                               int N, int B, int C, float eps_pred,
                                                               float* __restrict__ mean_prob,
                                                               float* __restrict__ var_unc,
                                                               float* __restrict__ alea,
                                                               float* __restrict__ pred_entropy,
                                                               long long* __restrict__ pred) {
  __shared__ double sred[2][4];
  __shared__ float sv[4];
  __shared__ int si[4];
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const double* s = sums + (long long)b * (2 * C + 1);
    double r[2] = {0.0, 0.0};   // variance sum, predictive entropy
    ArgBest best = {-INFINITY, 0};
    for (int c = threadIdx.x; c < C; c += 256) {
      const double pm = s[c] / N;
      const float pmf = (float)pm;
      if (mean_prob) mean_prob[(long long)b * C + c] = pmf;
      r[0] += (s[C + c] - N * pm * pm) / (double)(N - 1);
      r[1] -= (double)pmf * log((double)pmf + (double)eps_pred);
      if (pmf > best.v) { best.v = pmf; best.i = c; }
    }
    best = wave_argmax(best);
    __syncthreads();   // thread 0 has read the previous item's slots
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best.v; si[threadIdx.x >> 6] = best.i; }
    block_sum_u<4, 2, double>(r, sred);   // its barrier also publishes sv / si
    if (threadIdx.x == 0) {
      ArgBest a = {sv[0], si[0]};
      for (int w = 1; w < 4; ++w) a = arg_better(a, ArgBest{sv[w], si[w]});
      if (var_unc) var_unc[b] = (float)(r[0] / C);
      if (alea) alea[b] = (float)(s[2 * C] / N);
      if (pred_entropy) pred_entropy[b] = (float)r[1];
      if (pred) pred[b] = a.i;
    }
  }
}

__global__ __launch_bounds__(256) void nonfinite_kernel(const float* __restrict__ p, long long n,
                                                        int* __restrict__ out) {
  int bad = 0;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    bad |= !isfinite(p[i]);
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0 && bad) atomicAdd(out, 1);
}

static int grid1(long long n, int cap = 4096) {
  long long b = (n + 255) / 256;
  if (b > cap) b = cap;
  return (int)(b < 1 ? 1 : b);
}

}  // namespace mauv

static bool attn_args_ok(int rows, int hid) {
  if (rows < 0 || hid < 1) {
    set_error("attn: rows must be >= 0 and hid >= 1");
    return false;
  }
  return true;
}
MAUV_API int mauv_attn_t(const float* qkv, int rows, int hid, float* t, hipStream_t stream) {
  if (!attn_args_ok(rows, hid)) return -1;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(attn_t_kernel, dim3(grid1((long long)rows * hid)), dim3(256), 0, stream, qkv, rows, hid, t);
  return check_launch("attn_t");
}
MAUV_API int mauv_attn_t_bwd(const float* dt, const float* t, int rows, int hid, float* dqkv,
                             hipStream_t stream) {
  if (!attn_args_ok(rows, hid)) return -1;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(attn_t_bwd_kernel, dim3(grid1((long long)rows * hid)), dim3(256), 0, stream, dt, t, rows, hid, dqkv);
  return check_launch("attn_t_bwd");
}
MAUV_API int mauv_attn_out(const float* qkv, const float* s, int rows, int hid, float* comb,
                           int comb_ld, int comb_off, hipStream_t stream) {
  if (!attn_args_ok(rows, hid)) return -1;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(attn_out_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, qkv, s, rows, hid, comb, comb_ld, comb_off);
  return check_launch("attn_out");
}
MAUV_API int mauv_attn_out_bwd(const float* dcomb, int comb_ld, int comb_off, const float* qkv,
                               const float* s, int rows, int hid, float* dqkv, float* ds,
                               hipStream_t stream) {
  if (!attn_args_ok(rows, hid)) return -1;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(attn_out_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, dcomb, comb_ld, comb_off, qkv, s, rows, hid, dqkv, ds);
  return check_launch("attn_out_bwd");
}
MAUV_API int mauv_colsum(const float* dy, int G, int rows, int N, float* out, int accumulate,
                         hipStream_t stream) {
  hipLaunchKernelGGL(colsum_kernel, dim3(grid1((long long)G * N)), dim3(256), 0, stream, dy, G, rows, N, out, accumulate);
  return check_launch("colsum");
}
// The MC head's class range: 1..kSmallClasses on the one-thread-per-item kernels,
// kSmallClasses+1..kMaxClasses on the wide ones (include/mauv.h).  An empty batch (B or G zero)
// launches nothing.
static bool mc_args_ok(const char* what, int G, int B, int C) {
  if (G < 0 || B < 0 || C < 1 || C > kMaxClasses) {
    set_error(std::string(what) + ": G, B must be >= 0 and 1 <= C <= 4096 classes");
    return false;
  }
  return true;
}
static int item_grid(int B, int cap) { return B < cap ? B : cap; }

template <int KT>
static void launch_mc_ce_wide(const float* mean, const long long* labels, int B, int C,
                              const CeCrit& cr, float* loss, float* denom, long long* pred,
                              hipStream_t stream) {
  // 64 row registers per lane (C > 2048) fit without scratch under the 512-thread budget only
  constexpr int NT = KT > 32 ? 512 : 1024;
  hipLaunchKernelGGL((mc_ce_wide_kernel<KT, NT>), dim3(1), dim3(NT), 0, stream, mean, labels, B, C, cr, loss, denom, pred);
}
// the register tier of the row: 64 * KT classes, down to C = 1 on KT = 1
static void launch_mc_ce(const float* mean, const long long* labels, int B, int C,
                         const CeCrit& cr, float* loss, float* denom, long long* pred,
                         hipStream_t stream) {
  if (C <= 64) launch_mc_ce_wide<1>(mean, labels, B, C, cr, loss, denom, pred, stream);
  else if (C <= 128) launch_mc_ce_wide<2>(mean, labels, B, C, cr, loss, denom, pred, stream);
  else if (C <= 256) launch_mc_ce_wide<4>(mean, labels, B, C, cr, loss, denom, pred, stream);
  else if (C <= 512) launch_mc_ce_wide<8>(mean, labels, B, C, cr, loss, denom, pred, stream);
  else if (C <= 1024) launch_mc_ce_wide<16>(mean, labels, B, C, cr, loss, denom, pred, stream);
  else if (C <= 2048) launch_mc_ce_wide<32>(mean, labels, B, C, cr, loss, denom, pred, stream);
  else launch_mc_ce_wide<64>(mean, labels, B, C, cr, loss, denom, pred, stream);
}
template <int NT, int KT, int U>
static void launch_mc_stats_wide(const float* logits, int G, int B, int C, float eps_h,
                                 double* sums, int accumulate, hipStream_t stream) {
  // one resident block of 1024 threads per CU-sized share; smaller blocks, more of them
  hipLaunchKernelGGL((mc_stats_wide_kernel<NT, KT, U>), dim3(item_grid(B, 256 * (1024 / NT))), dim3(NT), 0, stream, logits, G, B, C, eps_h, sums, accumulate);
}

// mean over MC samples of logits (train/multimodal.py:121), cross-entropy against int64
// labels (:127, nullable) and argmax of the mean (torch.max(output, 1), :151; nullable).
MAUV_API int mauv_mc_mean_ce(const float* logits, const long long* labels, int G, int B, int C,
                             float* mean, float* loss, long long* pred, hipStream_t stream) {
  if (!mc_args_ok("mc_mean_ce", G, B, C)) return kErrArg;
  if (B == 0 || G == 0) return 0;
  if (C <= kSmallClasses) {
    hipLaunchKernelGGL(mc_mean_ce_kernel, dim3(1), dim3(256), 0, stream, logits, labels, G, B, C, mean, loss, pred);
    return check_launch("mc_mean_ce");
  }
  const long long BC = (long long)B * C;
  hipLaunchKernelGGL(mc_mean_wide_kernel, dim3(grid1(BC)), dim3(256), 0, stream, logits, G, BC, mean);
  if (labels || pred) launch_mc_ce(mean, labels, B, C, kPlainCe, loss, nullptr, pred, stream);
  return check_launch("mc_mean_ce");
}
MAUV_API int mauv_mc_mean_bwd(const float* dmean, const float* gloss, const float* mean,
                              const long long* labels, int G, int B, int C, float* dlogits,
                              hipStream_t stream) {
  if (!mc_args_ok("mc_mean_bwd", G, B, C)) return kErrArg;
  if (B == 0 || G == 0) return 0;
  if (C <= kSmallClasses)
    hipLaunchKernelGGL(mc_mean_bwd_kernel, dim3(grid1(B)), dim3(256), 0, stream, dmean, gloss, mean, labels, G, B, C, dlogits);
  else
    hipLaunchKernelGGL(mc_mean_bwd_wide_kernel, dim3(item_grid(B, 256), item_grid(G, 64)), dim3(256), 0, stream, dmean, gloss, mean, labels, G, B, C, kPlainCe, nullptr, dlogits);
  return check_launch("mc_mean_bwd");
}
// The same head under CrossEntropyLoss(weight, ignore_index, reduction, label_smoothing): the
// many-class kernels at every C (no label indexes memory unchecked, C <= 32 included).
static bool ce_crit_ok(const char* what, float eps, int reduction) {
  if (!(eps >= 0.f && eps <= 1.f) || (reduction != 0 && reduction != 1)) {
    set_error(std::string(what) + ": label_smoothing must be in [0, 1] and reduction 0 (mean) or 1 (sum)");
    return false;
  }
  return true;
}
MAUV_API int mauv_mc_mean_ce_ex(const float* logits, const long long* labels,
                                const float* class_weight, float label_smoothing,
                                long long ignore_index, int reduction, int G, int B, int C,
                                float* mean, float* loss, float* denom, long long* pred,
                                hipStream_t stream) {
  if (!mc_args_ok("mc_mean_ce_ex", G, B, C) || !ce_crit_ok("mc_mean_ce_ex", label_smoothing, reduction))
    return kErrArg;
  if (B == 0 || G == 0) return 0;
  const long long BC = (long long)B * C;
  hipLaunchKernelGGL(mc_mean_wide_kernel, dim3(grid1(BC)), dim3(256), 0, stream, logits, G, BC, mean);
  const CeCrit cr = {class_weight, label_smoothing, reduction, ignore_index};
  if (labels || pred) launch_mc_ce(mean, labels, B, C, cr, loss, denom, pred, stream);
  return check_launch("mc_mean_ce_ex");
}
MAUV_API int mauv_mc_mean_bwd_ex(const float* gloss, const float* mean, const long long* labels,
                                 const float* class_weight, float label_smoothing,
                                 long long ignore_index, int reduction, const float* denom,
                                 int G, int B, int C, float* dlogits, hipStream_t stream) {
  if (!mc_args_ok("mc_mean_bwd_ex", G, B, C) || !ce_crit_ok("mc_mean_bwd_ex", label_smoothing, reduction))
    return kErrArg;
  if (B == 0 || G == 0) return 0;
  const CeCrit cr = {class_weight, label_smoothing, reduction, ignore_index};
  hipLaunchKernelGGL(mc_mean_bwd_wide_kernel, dim3(item_grid(B, 256), item_grid(G, 64)), dim3(256), 0, stream, (const float*)nullptr, gloss, mean, labels, G, B, C, cr, denom, dlogits);
  return check_launch("mc_mean_bwd_ex");
}
MAUV_API int mauv_mc_stats(const float* logits, int G, int B, int C, float eps_h, double* sums,
                           int accumulate, hipStream_t stream) {
  if (!mc_args_ok("mc_stats", G, B, C)) return kErrArg;
  if (B == 0 || G == 0) return 0;
  if (C <= kSmallClasses)
    hipLaunchKernelGGL(mc_stats_kernel, dim3(grid1(B)), dim3(256), 0, stream, logits, G, B, C, eps_h, sums, accumulate);
  else if (C <= 64) launch_mc_stats_wide<64, 1, 8>(logits, G, B, C, eps_h, sums, accumulate, stream);
  else if (C <= 256) launch_mc_stats_wide<256, 1, 8>(logits, G, B, C, eps_h, sums, accumulate, stream);
  // few waves with several classes per thread: the cross-lane reductions cost per wave
  else if (C <= 512) launch_mc_stats_wide<256, 2, 4>(logits, G, B, C, eps_h, sums, accumulate, stream);
  else if (C <= 1024) launch_mc_stats_wide<256, 4, 4>(logits, G, B, C, eps_h, sums, accumulate, stream);
  else if (C <= 2048) launch_mc_stats_wide<512, 4, 2>(logits, G, B, C, eps_h, sums, accumulate, stream);
  else launch_mc_stats_wide<1024, 4, 2>(logits, G, B, C, eps_h, sums, accumulate, stream);
  return check_launch("mc_stats");
}
MAUV_API int mauv_mc_finalize(const double* sums, int N, int B, int C, float eps_pred,
                              float* mean_prob, float* var_unc, float* alea,
                              float* pred_entropy, long long* pred, hipStream_t stream) {
  if (!mc_args_ok("mc_finalize", N, B, C)) return kErrArg;
  if (B == 0) return 0;
  if (C <= kSmallClasses)
    hipLaunchKernelGGL(mc_finalize_kernel, dim3(grid1(B)), dim3(256), 0, stream, sums, N, B, C, eps_pred, mean_prob, var_unc, alea, pred_entropy, pred);
  else
    hipLaunchKernelGGL(mc_finalize_wide_kernel, dim3(item_grid(B, 256)), dim3(256), 0, stream, sums, N, B, C, eps_pred, mean_prob, var_unc, alea, pred_entropy, pred);
  return check_launch("mc_finalize");
}
MAUV_API int mauv_nonfinite_count(const float* p, long long n, int* out, hipStream_t stream) {
  hipLaunchKernelGGL(nonfinite_kernel, dim3(grid1(n, 2048)), dim3(256), 0, stream, p, n, out);
  return check_launch("nonfinite_count");
}
