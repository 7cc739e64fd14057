// Input staging on the device.
//
//  * data/datasets.py:239-250 (CustomImageDataset.__getitem__, :343-352): every tile is
//    decoded by PIL and turned into fp32 on CPU workers — ToTensor (x / 255, HWC -> CHW) and,
//    for the optical tile, Normalize((x - mean) / std) — and train/multimodal.py:87-94 copies
//    the fp32 tensors (and every patch size) to the GPU.  mauv_stage_u8 takes the decoded
//    uint8 HWC tiles instead (4x fewer bytes over PCIe) and does ToTensor + Normalize on the
//    device, with the same fp32 operations in the same order (bit-exact).
//  * Example training with image noise.py:55-93 (simulate_underwater_degradation, applied to
//    the normalised optical batch at :237-262): the underwater image formation model
//        t = exp(-beta_c * turbidity * d * depth);  I = clamp(J * t + B_inf,c * (1 - t), 0, 1)
//    with beta = (0.8, 0.5, 0.3), B_inf = (0.1, 0.3, 0.5) and d a [B][1][H][W] distance map
//    (the script passes a map of ones).  mauv_uifm applies it to fp32 NCHW tiles;
//    mauv_stage_u8 can apply it in the same pass as the normalisation (one read of the uint8
//    tile, one fp32 write).
// Both kernels are HBM-bound element-wise passes: 4 consecutive pixels of one (b, c, h) row
// per thread, 16-byte output stores.
#include "mauv_common.h"

using namespace mauv;

namespace mauv {

struct StageArgs {
  const unsigned char* x;  // uint8 [B][H][W][C] (mauv_stage_u8) or null
  const float* xf;         // fp32 [B][C][H][W] (mauv_uifm) or null
  int B, C, H, W;
  const float* mean;       // [C] or null
  const float* stdv;       // [C] or null
  const float* bt;         // [C]: beta_c * turbidity (fp32, as the reference computes it) or null
  const float* binf;       // [C]
  const float* dist;       // [B][1][H][W] or null (uniform distance 1)
  float depth;
  float* out;              // fp32 [B][C][H][W]
  // the augmented entries (mauv_*_aug); all null / 0 in the plain ones
  const unsigned char* ops;  // [B] move codes or null (no move)
  const float* turb;         // [B] per-item turbidity or null (bt holds beta_c * turbidity)
  int tr;                    // allow_transpose: bit2 of a code is read (H == W checked on the host)
};

// The dihedral move of item b (include/mauv.h): bit0 flips W, bit1 flips H, bit2 transposes
// (last).  As a gather: output (h, w) takes the value computed at source (hs, ws).
__device__ __forceinline__ unsigned move_code(const StageArgs& a, int b) {
  return a.ops ? (unsigned)a.ops[b] & (a.tr ? 7u : 3u) : 0u;
}
__device__ __forceinline__ void move_src(unsigned op, int H, int W, int h, int w, int& hs,
                                         int& ws) {
  const int p = (op & 4u) ? w : h, q = (op & 4u) ? h : w;
  hs = (op & 2u) ? H - 1 - p : p;
  ws = (op & 1u) ? W - 1 - q : q;
}
// beta_c * turbidity: the host's fp32 product (bt), or formed here per item as one fp32 product
template <bool AUG>
__device__ __forceinline__ float uifm_bt(const StageArgs& a, int b, int c) {
  if (AUG && a.turb) return __fmul_rn(a.bt[c], a.turb[b]);
  return a.bt[c];
}

__device__ __forceinline__ float uifm1(float j, float bt, float binf, float d, float depth) {
  // reference order: d = map * depth; t = exp(-beta * d); J * t + B_inf * (1 - t); clamp
  // separate roundings as the reference's tensor ops (no fma contraction)
  const float t = expf(__fmul_rn(-bt, __fmul_rn(d, depth)));
  const float v = __fadd_rn(__fmul_rn(j, t), __fmul_rn(binf, __fadd_rn(1.0f, -t)));
  return fminf(fmaxf(v, 0.0f), 1.0f);
}

// ToTensor (+ Normalize) (+ UIFM) of one uint8 sample of channel c at (b, h, w)
template <bool AUG = false>
__device__ __forceinline__ float stage_u8_val(const StageArgs& a, unsigned v, int b, int c, int h,
                                              int w) {
  // ToTensor: img.float().div(255) (torchvision functional.to_tensor)
  float x = (float)v / 255.0f;
  // Normalize: tensor.sub_(mean).div_(std)
  if (a.mean) x = (x - a.mean[c]) / a.stdv[c];
  if (a.bt) {
    const float d = a.dist ? a.dist[((long long)b * a.H + h) * a.W + w] : 1.0f;
    x = uifm1(x, uifm_bt<AUG>(a, b, c), a.binf[c], d, a.depth);
  }
  return x;
}

// AUG: every sample is evaluated at the moved source pixel (distance map included) and stored
// at the thread's own output position, so the 16-byte output stores stay as they are
template <bool AUG>
__global__ __launch_bounds__(256) void stage_kernel(const StageArgs a) {
  const int W4 = (a.W + 3) >> 2;
  const long long total = (long long)a.B * a.C * a.H * W4;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int w4 = (int)(i % W4);
    long long r = i / W4;
    const int h = (int)(r % a.H);
    r /= a.H;
    const int c = (int)(r % a.C);
    const int b = (int)(r / a.C);
    const int w0 = 4 * w4;
    const int nw = min(4, a.W - w0);
    const unsigned op = AUG ? move_code(a, b) : 0u;
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int hs = h, ws = w0 + (e < nw ? e : 0);
      if (AUG) move_src(op, a.H, a.W, h, ws, hs, ws);
      float x;
      if (a.x) {
        x = stage_u8_val<AUG>(a, a.x[(((long long)b * a.H + hs) * a.W + ws) * a.C + c], b, c, hs,
                              ws);
      } else {
        x = a.xf[(((long long)b * a.C + c) * a.H + hs) * a.W + ws];
        if (a.bt) {
          const float d = a.dist ? a.dist[((long long)b * a.H + hs) * a.W + ws] : 1.0f;
          x = uifm1(x, uifm_bt<AUG>(a, b, c), a.binf[c], d, a.depth);
        }
      }
      v[e] = x;
    }
    float* o = a.out + (((long long)b * a.C + c) * a.H + h) * a.W + w0;
    if (nw == 4 && (a.W & 3) == 0) {
      *(floatx4*)o = floatx4{v[0], v[1], v[2], v[3]};
    } else {
      for (int e = 0; e < nw; ++e) o[e] = v[e];
    }
  }
}

static int stage_grid(long long n) {
  long long b = (n + 255) / 256;
  if (b > 8192) b = 8192;
  return (int)(b < 1 ? 1 : b);
}

static int stage_launch(const StageArgs& a, hipStream_t stream, const char* what) {
  if (a.B < 0 || a.C < 1 || a.H < 0 || a.W < 0) {
    set_error(std::string(what) + ": bad shape or null output");
    return kErrArg;
  }
  if ((a.mean == nullptr) != (a.stdv == nullptr) || (a.bt && !a.binf)) {
    set_error(std::string(what) + ": mean/std and bt/binf come in pairs");
    return kErrArg;
  }
  const long long n = (long long)a.B * a.C * a.H * ((a.W + 3) / 4);
  if (n == 0) return 0;
  if ((!a.x && !a.xf) || !a.out) { set_error(std::string(what) + ": null input / output"); return kErrArg; }
  if (a.ops || a.turb)
    hipLaunchKernelGGL(stage_kernel<true>, dim3(stage_grid(n)), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(stage_kernel<false>, dim3(stage_grid(n)), dim3(256), 0, stream, a);
  return check_launch(what);
}

// ---------------------------------------------------------------------------------- Resize
// data/datasets.py:240-246: transforms.Resize((256, 256)) of every PIL tile before ToTensor /
// Normalize = PIL's Image.resize(size, BILINEAR) (PIL always antialiases).  Pillow's 8-bit
// separable resampler (libImaging/Resample.c; the reference pins pillow 11.0.0), restated:
//  * coefficients per output position o of a pass (in -> out): scale = in / out, filterscale =
//    max(scale, 1), support = filterscale (triangle filter of radius 1, widened when
//    downscaling), center = (o + 0.5) * scale, taps xmin = max((int)(center - support + 0.5), 0)
//    .. min((int)(center + support + 0.5), in) - 1, w_x = tri((x - center + 0.5) / filterscale)
//    normalised by their double sum, then (int)(0.5 + w * 2^22) — all in double, no FMA
//    contraction (PIL's x86-64 build issues separate multiplies and adds);
//  * a pass: acc = 2^21 + sum_x v_x * k_x (int32), out = clamp(acc >> 22, 0, 255) — the
//    horizontal pass into an 8-bit intermediate [B][H][Wo][C], then the vertical pass (each
//    only when its size changes, as ImagingResample does).
// The vertical pass optionally ends in the staging maths above (ToTensor, Normalize, UIFM):
// one fp32 NCHW write instead of an 8-bit image and a second pass.
constexpr int kResizeBits = 22;

__device__ __forceinline__ double tri_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// one thread per output position: bounds[o] = (xmin, n), kk[o][0..ksize) fixed point
__global__ __launch_bounds__(256) void resize_coeffs_kernel(int in, int out, int ksize,
                                                            int* bounds, int* kk) {
#pragma clang fp contract(off)
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= out) return;
  const double scale = (double)in / (double)out;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale, ss = 1.0 / filterscale;
  const double center = 0.0 + ((double)o + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += tri_filter(((double)(x + xmin) - center + 0.5) * ss);
  for (int x = 0; x < ksize; ++x) {
    int k = 0;
    if (x < xmax) {
      double w = tri_filter(((double)(x + xmin) - center + 0.5) * ss);
      if (ww != 0.0) w /= ww;
      k = w < 0.0 ? (int)(-0.5 + w * (double)(1 << kResizeBits))
                  : (int)(0.5 + w * (double)(1 << kResizeBits));
    }
    kk[(long long)o * ksize + x] = k;
  }
  bounds[2 * o] = xmin;
  bounds[2 * o + 1] = xmax;
}

__device__ __forceinline__ unsigned clip8_acc(int acc) {
  const int v = acc >> kResizeBits;
  return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v);
}

struct ResizeArgs {
  const unsigned char* x;  // [B][H][W][C]
  int B, H, W, C, Ho, Wo;
  const int *hb, *hk, *vb, *vk;  // horizontal / vertical bounds + coefficients (null: no pass)
  int hks, vks;
  unsigned char* tmp;      // [B][H][Wo][C] (both passes) or null
  unsigned char* out8;     // [B][Ho][Wo][C] or null
  StageArgs st;            // out8 null: fused staging into st.out [B][C][Ho][Wo]
};

// horizontal pass: one thread per (b, h, output column), all C channels
__global__ __launch_bounds__(256) void resize_h_kernel(const ResizeArgs a) {
  const long long n = (long long)a.B * a.H * a.Wo;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int xo = (int)(i % a.Wo);
    const long long bh = i / a.Wo;
    const int xmin = a.hb[2 * xo], nx = a.hb[2 * xo + 1];
    const int* k = a.hk + (long long)xo * a.hks;
    const unsigned char* src = a.x + (bh * a.W + xmin) * a.C;
    int acc[4] = {1 << (kResizeBits - 1), 1 << (kResizeBits - 1), 1 << (kResizeBits - 1),
                  1 << (kResizeBits - 1)};
    for (int t = 0; t < nx; ++t) {
      const int kt = k[t];
      for (int c = 0; c < a.C; ++c) acc[c] += (int)src[t * a.C + c] * kt;
    }
    unsigned char* dst = a.tmp + (bh * a.Wo + xo) * a.C;
    for (int c = 0; c < a.C; ++c) dst[c] = (unsigned char)clip8_acc(acc[c]);
  }
}

// vertical pass (or the only pass): one thread per (b, output row, output column); the source
// is tmp [B][H][Wo][C] after a horizontal pass, else x (W == Wo).  AUG: the thread of output
// (yo, xo) resamples and stages the moved source position (ys, xs) of the resized tile
template <bool AUG>
__global__ __launch_bounds__(256) void resize_v_kernel(const ResizeArgs a) {
  const long long n = (long long)a.B * a.Ho * a.Wo;
  const unsigned char* src = a.tmp ? a.tmp : a.x;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int xo = (int)(i % a.Wo);
    const long long r = i / a.Wo;
    const int yo = (int)(r % a.Ho), b = (int)(r / a.Ho);
    int ys = yo, xs = xo;
    if (AUG) move_src(move_code(a.st, b), a.Ho, a.Wo, yo, xo, ys, xs);
    unsigned v[4];
    if (a.vb) {
      const int ymin = a.vb[2 * ys], ny = a.vb[2 * ys + 1];
      const int* k = a.vk + (long long)ys * a.vks;
      int acc[4] = {1 << (kResizeBits - 1), 1 << (kResizeBits - 1), 1 << (kResizeBits - 1),
                    1 << (kResizeBits - 1)};
      for (int t = 0; t < ny; ++t) {
        const unsigned char* p = src + (((long long)b * a.H + ymin + t) * a.Wo + xs) * a.C;
        const int kt = k[t];
        for (int c = 0; c < a.C; ++c) acc[c] += (int)p[c] * kt;
      }
      for (int c = 0; c < a.C; ++c) v[c] = clip8_acc(acc[c]);
    } else {  // height unchanged: the horizontal result (or the input) as it is
      const unsigned char* p = src + (((long long)b * a.H + ys) * a.Wo + xs) * a.C;
      for (int c = 0; c < a.C; ++c) v[c] = p[c];
    }
    if (a.out8) {
      unsigned char* d = a.out8 + (((long long)b * a.Ho + yo) * a.Wo + xo) * a.C;
      for (int c = 0; c < a.C; ++c) d[c] = (unsigned char)v[c];
    } else {
      for (int c = 0; c < a.C; ++c)
        a.st.out[(((long long)b * a.C + c) * a.Ho + yo) * a.Wo + xo] =
            stage_u8_val<AUG>(a.st, v[c], b, c, ys, xs);
    }
  }
}

static int resize_ksize(int in, int out) {
  const double scale = (double)in / (double)out;
  const double support = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(support) * 2 + 1;
}

// workspace layout: hb [2 Wo] | hk [Wo * hks] | vb [2 Ho] | vk [Ho * vks] (int32), then the
// 8-bit horizontal result [B][H][Wo][C] (16-byte aligned; when the width changes)
static long long resize_ws(int B, int H, int W, int C, int Ho, int Wo, long long* tmp_off) {
  long long ints = 0;
  if (Wo != W) ints += 2LL * Wo + (long long)Wo * resize_ksize(W, Wo);
  if (Ho != H) ints += 2LL * Ho + (long long)Ho * resize_ksize(H, Ho);
  const long long off = (ints * 4 + 15) / 16 * 16;
  if (tmp_off) *tmp_off = off;
  return off + (Wo != W ? (long long)B * H * Wo * C : 0);
}

// ------------------------------------------------------------------- augmentation
// One thread per item i = item0 + b: r = philox4x32_10(ctr = (i, step lo, kAugLayer, step hi),
// key = seed), the counter layout of normal4.  code = r.x >> 30 (flips) or >> 29 (dihedral);
// turbidity = lo + (hi - lo) * u, u = ((float)r.y + 0.5f) * 2^-32, every step rounded in fp32.
constexpr uint32_t kAugLayer = 0x41554721u;

__global__ __launch_bounds__(256) void augment_draw_kernel(uint64_t seed, uint64_t step,
                                                           uint32_t item0, int B, int mode,
                                                           float lo, float hi, unsigned char* ops,
                                                           float* turb) {
#pragma clang fp contract(off)  // lo + span * u in two roundings, as the numpy oracle forms it
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const uint4 r = philox4x32_10(
      make_uint4(item0 + (uint32_t)b, (uint32_t)step, kAugLayer, (uint32_t)(step >> 32)),
      make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  ops[b] = (unsigned char)(mode == 0 ? 0u : mode == 1 ? r.x >> 30 : r.x >> 29);
  if (turb) {
    // plain operators: the pragma above does not reach into the inlined _rn intrinsics
    const float u = ((float)r.y + 0.5f) * 2.3283064365386963e-10f;
    const float span = hi - lo;
    const float part = span * u;
    turb[b] = lo + part;
  }
}

static int refuse(const char* what, const std::string& why) {
  set_error(std::string(what) + ": " + why);
  return kErrArg;
}

// a move is a gather: a thread reads pixels that another thread's store may have replaced, so
// the input and the output of a moving call share no byte
static bool overlap(const void* a, unsigned long long na, const void* b, unsigned long long nb) {
  const unsigned long long pa = (uintptr_t)a, pb = (uintptr_t)b;   // byte ranges [p, p + n)
  return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

// what the augmented staging entries share: the extents by name, the square tile a transposing
// code needs, and an element count every long long index of the kernels holds
static int aug_check(const char* what, int B, int C, int cmax, int H, int W, const char* hn,
                     const char* wn, int allow_transpose) {
  if (B < 0) return refuse(what, "B must be >= 0");
  if (C < 1 || C > cmax) return refuse(what, "C must be in 1.." + std::to_string(cmax));
  if (H < 1) return refuse(what, std::string(hn) + " must be >= 1");
  if (W < 1) return refuse(what, std::string(wn) + " must be >= 1");
  if (allow_transpose && H != W)
    return refuse(what, std::string("allow_transpose needs a square tile, ") + hn + " must equal " +
                            wn + " (got " + std::to_string(H) + " x " + std::to_string(W) + ")");
  if ((__int128)B * C * H * W >= ((__int128)1 << 62))
    return refuse(what, std::string("elements B * C * ") + hn + " * " + wn +
                            " must stay below 2^62 (the kernels index with long long)");
  return 0;
}

static int resize_run(const char* what, const unsigned char* x, int B, int H, int W, int C, int Ho,
                      int Wo, void* workspace, unsigned char* out_u8, const float* mean,
                      const float* stdv, const float* uifm_bt, const float* uifm_binf,
                      const float* dist, float depth, const unsigned char* ops, const float* turb,
                      int tr, float* out_f32, hipStream_t stream) {
  const std::string w(what);
  if ((out_u8 == nullptr) == (out_f32 == nullptr)) {
    set_error(w + ": exactly one of out_u8 / out_f32");
    return kErrArg;
  }
  if ((mean == nullptr) != (stdv == nullptr) || (uifm_bt && !uifm_binf)) {
    set_error(w + ": mean/std and bt/binf come in pairs");
    return kErrArg;
  }
  if (B == 0) return 0;
  if (!x) { set_error(w + ": null input"); return kErrArg; }
  long long tmp_off = 0;
  resize_ws(B, H, W, C, Ho, Wo, &tmp_off);
  if ((Wo != W || Ho != H) && !workspace) { set_error(w + ": null workspace"); return kErrArg; }
  int* ws = (int*)workspace;
  ResizeArgs a{};
  a.x = x; a.B = B; a.H = H; a.W = W; a.C = C; a.Ho = Ho; a.Wo = Wo;
  a.out8 = out_u8;
  a.st = StageArgs{nullptr, nullptr, B, C, Ho, Wo, mean, stdv, uifm_bt, uifm_binf, dist, depth,
                   out_f32, ops, turb, tr};
  const bool aug = ops || turb;
  int* p = ws;
  if (Wo != W) {
    a.hks = resize_ksize(W, Wo);
    a.hb = p; a.hk = p + 2 * Wo; p += 2 * Wo + (long long)Wo * a.hks;
    hipLaunchKernelGGL(resize_coeffs_kernel, dim3(ceil_div(Wo, 256)), dim3(256), 0, stream, W, Wo,
                       a.hks, (int*)a.hb, (int*)a.hk);
  }
  if (Ho != H) {
    a.vks = resize_ksize(H, Ho);
    a.vb = p; a.vk = p + 2 * Ho;
    hipLaunchKernelGGL(resize_coeffs_kernel, dim3(ceil_div(Ho, 256)), dim3(256), 0, stream, H, Ho,
                       a.vks, (int*)a.vb, (int*)a.vk);
  }
  if (Wo != W) {
    // the intermediate: the vertical pass's source; with the height unchanged the horizontal
    // pass writes straight into the 8-bit output, or into the workspace before the staging (or
    // before the move: the last pass is the one that stores at the moved position)
    const bool direct = Ho == H && out_u8 && !aug;
    a.tmp = direct ? out_u8 : (unsigned char*)workspace + tmp_off;
    const long long n = (long long)B * H * Wo;
    hipLaunchKernelGGL(resize_h_kernel, dim3(stage_grid(n)), dim3(256), 0, stream, a);
    if (direct) return check_launch(what);
  }
  const long long n = (long long)B * Ho * Wo;
  if (aug)
    hipLaunchKernelGGL(resize_v_kernel<true>, dim3(stage_grid(n)), dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(resize_v_kernel<false>, dim3(stage_grid(n)), dim3(256), 0, stream, a);
  return check_launch(what);
}

}  // namespace mauv

MAUV_API long long mauv_resize_workspace_bytes(int B, int H, int W, int C, int Ho, int Wo) {
  if (B < 0 || H < 1 || W < 1 || C < 1 || C > 4 || Ho < 1 || Wo < 1) return -1;
  return resize_ws(B, H, W, C, Ho, Wo, nullptr);
}

MAUV_API int mauv_resize_u8(const unsigned char* x, int B, int H, int W, int C, int Ho, int Wo,
                            void* workspace, unsigned char* out_u8, const float* mean,
                            const float* stdv, const float* uifm_bt, const float* uifm_binf,
                            const float* dist, float depth, float* out_f32, hipStream_t stream) {
  if (B < 0 || H < 1 || W < 1 || C < 1 || C > 4 || Ho < 1 || Wo < 1) {
    set_error("resize_u8: bad shape (1 <= C <= 4)");
    return kErrArg;
  }
  return resize_run("resize_u8", x, B, H, W, C, Ho, Wo, workspace, out_u8, mean, stdv, uifm_bt,
                    uifm_binf, dist, depth, nullptr, nullptr, 0, out_f32, stream);
}

MAUV_API int mauv_resize_u8_aug(const unsigned char* x, int B, int H, int W, int C, int Ho, int Wo,
                                void* workspace, unsigned char* out_u8, const float* mean,
                                const float* stdv, const float* uifm_bt, const float* uifm_binf,
                                const float* dist, float depth, const unsigned char* ops,
                                const float* turb, int allow_transpose, float* out_f32,
                                hipStream_t stream) {
  const char* what = "resize_u8_aug";
  if (int rc = aug_check(what, B, C, 4, Ho, Wo, "Ho", "Wo", allow_transpose)) return rc;
  if (H < 1) return refuse(what, "H must be >= 1");
  if (W < 1) return refuse(what, "W must be >= 1");
  // the input and the 8-bit horizontal result [B][H][Wo][C], and the coefficient tables'
  // int indices 2 * o + 1
  if ((__int128)B * C * H * (W > Wo ? W : Wo) >= ((__int128)1 << 62))
    return refuse(what, "elements B * C * H * max(W, Wo) must stay below 2^62");
  if (Ho > (1 << 30)) return refuse(what, "Ho must be <= 2^30");
  if (Wo > (1 << 30)) return refuse(what, "Wo must be <= 2^30");
  const long long nin = (long long)B * H * W * C, nout = (long long)B * Ho * Wo * C;
  if (ops && (overlap(x, nin, out_u8, nout) || overlap(x, nin, out_f32, 4ULL * nout)))
    return refuse(what, "x must not overlap out_u8 / out_f32 when ops are given (the move is a "
                        "gather)");
  if (turb && !out_f32) return refuse(what, "turb goes with the fp32 output only (out_f32 is null)");
  if (turb && !uifm_bt) return refuse(what, "turb needs uifm_bt (the plain beta[c])");
  return resize_run(what, x, B, H, W, C, Ho, Wo, workspace, out_u8, mean, stdv, uifm_bt,
                    uifm_binf, dist, depth, ops, turb, allow_transpose != 0, out_f32, stream);
}

MAUV_API int mauv_stage_u8(const unsigned char* x, int B, int H, int W, int C, const float* mean,
                           const float* stdv, const float* uifm_bt, const float* uifm_binf,
                           const float* dist, float depth, float* out, hipStream_t stream) {
  StageArgs a{x, nullptr, B, C, H, W, mean, stdv, uifm_bt, uifm_binf, dist, depth, out};
  return stage_launch(a, stream, "stage_u8");
}

MAUV_API int mauv_stage_u8_aug(const unsigned char* x, int B, int H, int W, int C,
                               const float* mean, const float* stdv, const float* uifm_bt,
                               const float* uifm_binf, const float* dist, float depth,
                               const unsigned char* ops, const float* turb, int allow_transpose,
                               float* out, hipStream_t stream) {
  const char* what = "stage_u8_aug";
  if (int rc = aug_check(what, B, C, INT32_MAX, H, W, "H", "W", allow_transpose)) return rc;
  if (turb && !uifm_bt) return refuse(what, "turb needs uifm_bt (the plain beta[c])");
  const long long n = (long long)B * C * H * W;
  if (ops && overlap(x, n, out, 4ULL * n))
    return refuse(what, "x must not overlap out when ops are given (the move is a gather)");
  StageArgs a{x, nullptr, B, C, H, W, mean, stdv, uifm_bt, uifm_binf, dist, depth, out,
              ops, turb, allow_transpose != 0};
  return stage_launch(a, stream, what);
}

MAUV_API int mauv_stage_f32_aug(const float* x, int B, int C, int H, int W, const float* beta,
                                const float* binf, const float* dist, float depth,
                                const unsigned char* ops, const float* turb, int allow_transpose,
                                float* out, hipStream_t stream) {
  const char* what = "stage_f32_aug";
  if (int rc = aug_check(what, B, C, INT32_MAX, H, W, "H", "W", allow_transpose)) return rc;
  if (turb && !beta) return refuse(what, "turb needs beta");
  const long long n = (long long)B * C * H * W;
  if (overlap(x, 4ULL * n, out, 4ULL * n))
    return refuse(what, "x must not overlap out (the kernel is a gather)");
  StageArgs a{nullptr, x, B, C, H, W, nullptr, nullptr, beta, binf, dist, depth, out,
              ops, turb, allow_transpose != 0};
  return stage_launch(a, stream, what);  // ops and turb null: the plain kernel (a copy / mauv_uifm)
}

MAUV_API int mauv_augment_draw(unsigned long long seed, unsigned long long step, long long item0,
                               int B, int mode, float turb_lo, float turb_hi,
                               unsigned char* ops_out, float* turb_out, hipStream_t stream) {
  const char* what = "augment_draw";
  if (mode < 0 || mode > 2) return refuse(what, "mode must be 0 (none), 1 (flips) or 2 (dihedral)");
  if (!(turb_hi >= turb_lo)) return refuse(what, "turb_hi must be >= turb_lo");
  if (B < 0) return refuse(what, "B must be >= 0");
  if (item0 < 0 || item0 + (long long)B > (1LL << 32))
    return refuse(what, "item0 must be >= 0 and item0 + B <= 2^32 (the item index is a 32-bit "
                        "counter word)");
  if (B == 0) return 0;
  if (!ops_out) return refuse(what, "null ops_out");
  hipLaunchKernelGGL(augment_draw_kernel, dim3(ceil_div(B, 256)), dim3(256), 0, stream,
                     (uint64_t)seed, (uint64_t)step, (uint32_t)item0, B, mode, turb_lo, turb_hi,
                     ops_out, turb_out);
  return check_launch(what);
}

MAUV_API int mauv_uifm(const float* x, int B, int C, int H, int W, const float* bt,
                       const float* binf, const float* dist, float depth, float* out,
                       hipStream_t stream) {
  StageArgs a{nullptr, x, B, C, H, W, nullptr, nullptr, bt, binf, dist, depth, out};
  if (!bt) { set_error("uifm: null bt"); return kErrArg; }
  return stage_launch(a, stream, "uifm");
}
