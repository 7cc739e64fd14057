// Global gradient norm + non-finite scan in one pass, and the in-place clip.
//
// torch.nn.utils.clip_grad_norm_ over a model's gradients is a norm per tensor, a norm of the
// norms, and a multiply per tensor.  Here the gradients are a device table of spans (the flat
// gradient arena is ONE span; a plain parameter list is one span per tensor):
//   grad_norm_kernel     every block reduces its share of one span to a double partial (sum of
//                        squares, or max |x|) and a "saw a non-finite element" flag, and writes
//                        both into its own workspace slot
//   grad_norm_finalize   one block adds the partials in a fixed order, takes the root, rounds
//                        once to fp32; a non-finite element makes the norm NaN and adds 1 to the
//                        caller's counter (the contract of mauv_nonfinite_count)
//   grad_clip_kernel     g *= min(1, max_norm / (norm + 1e-6)), the coefficient formed on the
//                        device from the norm word
// No floating-point atomics: the same data gives the same bits on every run and on every rank.
// The gated Adam step never runs grad_clip_kernel: step_gate_kernel forms the same coefficient
// and the Adam kernels multiply as they load g (adam.hip).
#include "mauv_common.h"

using namespace mauv;

namespace mauv {

constexpr int kNormBlocks = 2048;   // blocks of the single-span (arena) launch: 8 per CU

// blocks per span: the whole budget for one span, a share of it for a table of many
static int norm_gx(int n_spans) {
  const int g = kNormBlocks / n_spans;
  return g < 1 ? 1 : g;
}

// A span as a scalar head up to the first 16-byte boundary, a body of 16-byte quads, and a
// scalar tail (block 0 of the span takes head and tail).
struct SpanSplit {
  long long numel, head, n4;
  float* body;
};
__device__ __forceinline__ SpanSplit split_span(const MauvSpan& t) {
  SpanSplit s;
  const uintptr_t a = reinterpret_cast<uintptr_t>(t.p);
  s.numel = t.numel > 0 ? t.numel : 0;
  s.head = (a & 3) ? s.numel : (long long)(((16 - (a & 15)) & 15) >> 2);
  if (s.head > s.numel) s.head = s.numel;
  s.n4 = (s.numel - s.head) / 4;
  s.body = const_cast<float*>(t.p) + s.head;
  return s;
}
// a block past the span's last quad (most blocks of a small tensor) has nothing to do
__device__ __forceinline__ bool span_block_idle(const SpanSplit& s) {
  return blockIdx.x != 0 && blockIdx.x * 256LL >= s.n4;
}

template <int KIND>
__device__ __forceinline__ void norm_acc(double& acc, int& bad, float x) {
  bad |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
  const double d = (double)x;   // exact; d * d is exact too, and the sum cannot overflow
  if (KIND == 0) acc = fma(d, d, acc);
  else acc = fmax(acc, fabs(d));
}
template <int KIND>
__device__ __forceinline__ double norm_join(double a, double b) {
  return KIND == 0 ? a + b : fmax(a, b);
}

// width-64 shuffles, then the four waves through LDS in wave order; thread 0 holds the result
template <int KIND>
__device__ __forceinline__ void block_norm_reduce(double& acc, int& bad) {
  __shared__ double sacc[4];
  __shared__ int sbad[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc = norm_join<KIND>(acc, __shfl_xor(acc, o, 64));
    bad |= __shfl_xor(bad, o, 64);
  }
  if ((threadIdx.x & 63) == 0) { sacc[threadIdx.x >> 6] = acc; sbad[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc = sacc[0]; bad = sbad[0];
    for (int w = 1; w < 4; ++w) { acc = norm_join<KIND>(acc, sacc[w]); bad |= sbad[w]; }
  }
}

// grid = (blocks per span, spans)
template <int KIND>
__global__ __launch_bounds__(256) void grad_norm_kernel(const MauvSpan* __restrict__ tab,
                                                        double* __restrict__ part,
                                                        int* __restrict__ flag) {
  const int bid = blockIdx.y * gridDim.x + blockIdx.x;
  const SpanSplit s = split_span(tab[blockIdx.y]);
  if (span_block_idle(s)) {
    if (threadIdx.x == 0) { part[bid] = 0.0; flag[bid] = 0; }
    return;
  }
  double acc = 0.0;
  int bad = 0;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < s.n4; i += (long long)gridDim.x * 256) {
    const floatx4 v = ((const floatx4*)s.body)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) norm_acc<KIND>(acc, bad, v[e]);
  }
  if (blockIdx.x == 0) {
    const float* p = s.body - s.head;
    for (long long i = threadIdx.x; i < s.head; i += 256) norm_acc<KIND>(acc, bad, p[i]);
    for (long long i = s.head + s.n4 * 4 + threadIdx.x; i < s.numel; i += 256)
      norm_acc<KIND>(acc, bad, p[i]);
  }
  block_norm_reduce<KIND>(acc, bad);
  if (threadIdx.x == 0) { part[bid] = acc; flag[bid] = bad; }
}

// one block: thread t joins partials t, t + 256, ... in that order, then the block reduce
template <int KIND>
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double* __restrict__ part,
                                                                 const int* __restrict__ flag,
                                                                 int nb, float* norm_out,
                                                                 int* nonfinite) {
  double acc = 0.0;
  int bad = 0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    acc = norm_join<KIND>(acc, part[i]);
    bad |= flag[i];
  }
  block_norm_reduce<KIND>(acc, bad);
  if (threadIdx.x == 0) {
    if (bad) {
      if (nonfinite) atomicAdd(nonfinite, 1);
      *norm_out = __uint_as_float(0x7fc00000u);
    } else {
      *norm_out = (float)(KIND == 0 ? sqrt(acc) : acc);
    }
  }
}

__global__ __launch_bounds__(256) void grad_clip_kernel(const MauvSpan* __restrict__ tab,
                                                        const float* __restrict__ norm,
                                                        float max_norm) {
  const float coef = clip_coef(max_norm, *norm);
  if (coef == 1.0f) return;   // g * 1 is g: nothing to write
  const SpanSplit s = split_span(tab[blockIdx.y]);
  if (span_block_idle(s)) return;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < s.n4; i += (long long)gridDim.x * 256) {
    floatx4 v = ((const floatx4*)s.body)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = __fmul_rn(v[e], coef);
    ((floatx4*)s.body)[i] = v;
  }
  if (blockIdx.x == 0) {
    float* p = s.body - s.head;
    for (long long i = threadIdx.x; i < s.head; i += 256) p[i] = __fmul_rn(p[i], coef);
    for (long long i = s.head + s.n4 * 4 + threadIdx.x; i < s.numel; i += 256)
      p[i] = __fmul_rn(p[i], coef);
  }
}

}  // namespace mauv

static bool spans_ok(const char* who, const void* spans, int n_spans) {
  if (n_spans < 1 || n_spans > 65535 || !spans) {
    set_error(std::string(who) + ": 1..65535 spans in a device table");
    return false;
  }
  return true;
}

MAUV_API long long mauv_grad_norm_workspace_bytes(int n_spans) {
  if (n_spans < 1 || n_spans > 65535) {
    set_error("grad_norm_workspace_bytes: 1..65535 spans");
    return kErrArg;
  }
  return (long long)norm_gx(n_spans) * n_spans * 16;   // a double and a flag word (padded) each
}

MAUV_API int mauv_grad_norm(const MauvSpan* spans, int n_spans, int kind, void* workspace,
                            float* norm_out, int* nonfinite, hipStream_t stream) {
  if (!spans_ok("grad_norm", spans, n_spans)) return kErrArg;
  if (kind != 0 && kind != 1) { set_error("grad_norm: kind is 0 (L2) or 1 (max-abs)"); return kErrArg; }
  if (!workspace || !norm_out) { set_error("grad_norm: null workspace / norm_out"); return kErrArg; }
  const int gx = norm_gx(n_spans), nb = gx * n_spans;
  double* part = (double*)workspace;
  int* flag = (int*)(part + nb);
  if (kind == 0) {
    hipLaunchKernelGGL(grad_norm_kernel<0>, dim3(gx, n_spans), dim3(256), 0, stream, spans, part, flag);
    hipLaunchKernelGGL(grad_norm_finalize_kernel<0>, dim3(1), dim3(256), 0, stream,
                       (const double*)part, (const int*)flag, nb, norm_out, nonfinite);
  } else {
    hipLaunchKernelGGL(grad_norm_kernel<1>, dim3(gx, n_spans), dim3(256), 0, stream, spans, part, flag);
    hipLaunchKernelGGL(grad_norm_finalize_kernel<1>, dim3(1), dim3(256), 0, stream,
                       (const double*)part, (const int*)flag, nb, norm_out, nonfinite);
  }
  return check_launch("grad_norm");
}

MAUV_API int mauv_grad_clip(const MauvSpan* spans, int n_spans, const float* norm, float max_norm,
                            hipStream_t stream) {
  if (!spans_ok("grad_clip", spans, n_spans)) return kErrArg;
  if (!norm) { set_error("grad_clip: null norm"); return kErrArg; }
  if (!(max_norm > 0.f) || !std::isfinite(max_norm)) {
    set_error("grad_clip: max_norm must be finite and > 0");
    return kErrArg;
  }
  hipLaunchKernelGGL(grad_clip_kernel, dim3(norm_gx(n_spans), n_spans), dim3(256), 0, stream,
                     spans, norm, max_norm);
  return check_launch("grad_clip");
}
