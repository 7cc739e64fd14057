// Implicit-GEMM convolution on CDNA4 16-bit MFMA (bf16 / f16 operands, fp32 accumulation): the
// C entry points of the 16-bit convs and the register-staged kernel conv_gemm_h16, which runs
// every shape outside the pipelined kernels (conv_pipe16.hip and the families it routes to):
// forwards with Cin % 64 != 0, data gradients with Cout % 64 != 0, weight gradients over rows or
// columns of more than 4096 output pixels, tensors beyond 31-bit byte offsets (it addresses by
// 64-bit pointers).  It takes the pipelined kernels' argument block (ConvArgs) and their shared
// pieces — conv_block_tile, acc_shift16 / acc_start16, bn_relu8, epilogue16 (conv_epi16.h) and
// the weight gradient's conv_epilogue (conv_common.h) — so its outputs and statistics partials
// are the pipelined kernel's bits on the same operands zero-padded to its channel multiples.
//
// The reduced-precision counterpart of conv_gemm.hip for BASELINE configs[2] (bf16 training)
// and the reference predictor's autocast inference (inference/predictors.py:55): the same three
// GEMM views of every Bayesian conv of the three trunks (models/base_models.py:15-18,
// models/model_utils.py:57-61), one launch for all G MC samples (blockIdx.y = sample).
//
//   FWD   y [B*Ho*Wo][Cout]  = im2col(x)[.][R*S*Cin] . W_g^T            (16-bit out, fp32 BN
//                                                                        statistics partials)
//   DGRAD dx[B*H*W][Cin]     = gather(dy)[.][R*S*Cout] . W_g[(r,s,n)][c]  (per output-parity
//                                                                        class, as conv_gemm.hip)
//   WGRAD dW[Cout][R*S*Cin]  = dy^T[Cout][pixels] . im2col(x)[pixels][.]  (fp32 split-K slabs)
//
// MFMA v_mfma_f32_32x32x16_{bf16,f16}: lane l holds A[row l&31][k = 8(l>>5) + j] and
// B[k = 8(l>>5) + j][col l&31], j = 0..7.  Operands are staged global -> registers -> LDS in
// 16-byte chunks (8 channels; every conv of the path has Cin, Cout % 8 == 0 — the stems' 1/3
// input channels are zero-padded to 8 by the caller), double buffered, BK = 32 per stage, in
// one of two LDS images:
//   row image [rows][BK+8]   k-contiguous (80-B rows): an operand fragment is ONE
//                            ds_read_b128, conflict-free (FWD A and B, DGRAD A);
//   col image [BK][rows+32]  rows-contiguous, i.e. the natural layout of a k-strided operand
//                            (DGRAD B = KRSC weights along Cin, WGRAD A = dy, WGRAD B = x):
//                            an operand fragment is two ds_read_b64_tr_b16 hardware-transposed
//                            reads; the 64-B pad makes a 32-lane half's 4 rows x 64 B cover
//                            the 64 banks once (conflict-free).
// 256 threads = 4 waves (2x2), wave tile (BM/2)x(BN/2) = 1 or 2 MFMA tiles of 32x32 each way.
#include <stdlib.h>

#include "conv_common.h"
#include "conv_epi16.h"

namespace mauv {

constexpr int HBK = 32;
constexpr int RLD = HBK + 8;
__host__ __device__ constexpr int cld(int rows) { return rows + 32; }

template <int MODE, int DT, int BM, int BN, bool TAPU>
__global__ __launch_bounds__(256) void conv_gemm_h16(const ConvArgs a) {
  constexpr bool A_COL = (MODE == WGRAD);
  constexpr bool B_COL = (MODE != FWD);
  constexpr int A_SZ = A_COL ? HBK * cld(BM) : BM * RLD;
  constexpr int B_SZ = B_COL ? HBK * cld(BN) : BN * RLD;
  constexpr int STG = A_SZ + B_SZ;
  constexpr int WM = BM / 2, WN = BN / 2, MI = WM / 32, NI = WN / 32;
  constexpr int NA = BM / 64, NB = BN / 64;  // 16-B chunks per thread per stage
  static_assert(2 * STG >= 2 * WM * (BN + 4) && 2 * STG >= 16 * BN, "epilogue scratch");
  __shared__ __attribute__((aligned(16))) u16 smem[2 * STG];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  int m0, n0, by;
  conv_block_tile<BM, BN>(a, m0, n0, by);  // xcd_grid = 0: XCD-aware order over blockIdx.x
  int g, sp = 0;
  if constexpr (MODE == WGRAD) { g = by / a.splits; sp = by % a.splits; }
  else g = by;
  int kbeg = 0, kend = a.K;
  if constexpr (MODE == WGRAD) { kbeg = sp * a.kchunk; kend = min(a.K, kbeg + a.kchunk); }

  const u16* xg = (const u16*)a.x + (long long)g * a.xs_g;
  const u16* wg = (const u16*)a.w + (long long)g * a.ws_g;
  const u16* dyg = (const u16*)a.dy + (long long)g * ((long long)a.B * a.Ho * a.Wo * a.Cout);

  // ---------------- per-thread loader state ----------------
  long long a_base[NA];
  int a_p0[NA], a_p1[NA];
  bool a_ok[NA];
  int b_r[NB], b_s[NB], b_c[NB];
  bool b_ok[NB];
  int px_b[NB], px_h[NB], px_w[NB];  // WGRAD B: pixel of this thread's chunk row
  const int kc = tid & 3;           // row images: chunk within the 32-deep k slice
  // A
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    if constexpr (MODE == FWD || MODE == DGRAD) {
      const int m = m0 + (tid >> 2) + 64 * j;
      a_ok[j] = m < a.M;
      const int mm = a_ok[j] ? m : 0;
      const int HW = (MODE == FWD) ? a.Ho * a.Wo : a.Hc * a.Wc;
      const int WW = (MODE == FWD) ? a.Wo : a.Wc;
      const int b = mm / HW, rem = mm - b * HW, oh = rem / WW, ow = rem - oh * WW;
      if constexpr (MODE == FWD) {
        a_base[j] = (long long)b * a.xs_b;
        a_p0[j] = oh * a.stride - a.pad;
        a_p1[j] = ow * a.stride - a.pad;
      } else {
        a_base[j] = (long long)b * a.Ho * a.Wo * a.Cout;
        a_p0[j] = oh * a.stride + a.ph + a.pad;
        a_p1[j] = ow * a.stride + a.pw + a.pad;
      }
    } else {  // WGRAD A (col image [pixel][cout])
      const int idx = tid + 256 * j;
      a_p0[j] = idx / (BM / 8);        // k row
      a_p1[j] = m0 + 8 * (idx % (BM / 8));  // cout
      a_ok[j] = a_p1[j] < a.M;
      a_base[j] = 0;
    }
  }
  // B
  floatx8 bsc[NB], bsh[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int idx = tid + 256 * j;
    if constexpr (MODE == FWD) {
      const int n = n0 + (tid >> 2) + 64 * j;
      b_ok[j] = n < a.N;
      b_r[j] = b_ok[j] ? n : 0;
    } else if constexpr (MODE == DGRAD) {
      b_r[j] = idx / (BN / 8);              // k row within the stage
      b_c[j] = n0 + 8 * (idx % (BN / 8));   // cin
      b_ok[j] = b_c[j] < a.N;
    } else {  // WGRAD B: fixed column chunk (r,s,c..c+7), moving pixel row
      const int col = n0 + 8 * (idx % (BN / 8));
      b_ok[j] = col < a.N;
      const int cc = b_ok[j] ? col : 0;
      const int rs = cc / a.Cin;
      b_c[j] = cc - rs * a.Cin;
      b_r[j] = rs / a.S;
      b_s[j] = rs - b_r[j] * a.S;
      const int p = kbeg + idx / (BN / 8);
      const int HW = a.Ho * a.Wo;
      px_b[j] = p / HW;
      const int rem = p - px_b[j] * HW;
      px_h[j] = rem / a.Wo;
      px_w[j] = rem - px_h[j] * a.Wo;
      if (a.xsc && b_ok[j]) {
        bsc[j] = ldf8(a.xsc + g * a.Cin + b_c[j]);
        bsh[j] = ldf8(a.xsh + g * a.Cin + b_c[j]);
      }
    }
  }

  // tile-uniform tap counters (FWD with Cin % 32 == 0; DGRAD: Cout % 32 == 0 always)
  int t_r = 0, t_s = 0, t_c = 0;  // FWD: (r, s, c0)   DGRAD: (tr, ts, n0)

  u32x4 ra[NA], rb[NB];
  const u32x4 zero = {0u, 0u, 0u, 0u};
  const unsigned rfloor = a.xrelu ? 0u : 0x80008000u;  // bn_relu8's ReLU floor

  auto load = [&](int k0) {
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      u32x4 v = zero;
      if constexpr (MODE == FWD) {
        int r, s, c;
        bool kok = true;
        if constexpr (TAPU) {
          r = t_r; s = t_s; c = t_c + 8 * kc;
        } else {
          const int k = k0 + 8 * kc;
          kok = k < kend;
          const int tap = k / a.Cin;
          c = k - tap * a.Cin;
          r = tap / a.S;
          s = tap - r * a.S;
        }
        const int ih = a_p0[j] + r, iw = a_p1[j] + s;
        if (a_ok[j] && kok && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
          v = *(const u32x4*)(xg + a_base[j] + (long long)ih * a.xs_h + (long long)iw * a.xs_w + c);
          if (a.xsc)
            v = bn_relu8<DT>(v, ldf8(a.xsc + g * a.Cin + c), ldf8(a.xsh + g * a.Cin + c), rfloor, true);
        }
      } else if constexpr (MODE == DGRAD) {
        const int ohn = a_p0[j] - a.r0 - a.stride * t_r, own = a_p1[j] - a.s0 - a.stride * t_s;
        if (a_ok[j] && ohn >= 0 && own >= 0) {
          const int oh = a.stride == 1 ? ohn : ohn / a.stride;
          const int ow = a.stride == 1 ? own : own / a.stride;
          if (oh < a.Ho && ow < a.Wo)
            v = *(const u32x4*)(dyg + a_base[j] + ((long long)oh * a.Wo + ow) * a.Cout + t_c + 8 * kc);
        }
      } else {  // WGRAD A
        const int p = k0 + a_p0[j];
        if (a_ok[j] && p < kend) v = *(const u32x4*)(dyg + (long long)p * a.Cout + a_p1[j]);
      }
      ra[j] = v;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      u32x4 v = zero;
      if constexpr (MODE == FWD) {
        const int k = k0 + 8 * kc;
        if (b_ok[j] && k < kend) v = *(const u32x4*)(wg + (long long)b_r[j] * a.K + k);
      } else if constexpr (MODE == DGRAD) {
        const int n = t_c + b_r[j];
        const int r = a.r0 + a.stride * t_r, s = a.s0 + a.stride * t_s;
        if (b_ok[j]) v = *(const u32x4*)(wg + (((long long)n * a.R + r) * a.S + s) * a.Cin + b_c[j]);
      } else {  // WGRAD B
        const int p = k0 + (tid + 256 * j) / (BN / 8);
        if (b_ok[j] && p < kend) {
          const int ih = px_h[j] * a.stride - a.pad + b_r[j];
          const int iw = px_w[j] * a.stride - a.pad + b_s[j];
          if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
            v = *(const u32x4*)(xg + (long long)px_b[j] * a.xs_b + (long long)ih * a.xs_h +
                                (long long)iw * a.xs_w + b_c[j]);
            if (a.xsc) v = bn_relu8<DT>(v, bsc[j], bsh[j], rfloor, true);
          }
        }
        // advance this chunk's pixel by one stage
        px_w[j] += HBK;
        while (px_w[j] >= a.Wo) { px_w[j] -= a.Wo; ++px_h[j]; }
        while (px_h[j] >= a.Ho) { px_h[j] -= a.Ho; ++px_b[j]; }
      }
      rb[j] = v;
    }
    // advance the tile-uniform tap counters by one stage
    if constexpr ((MODE == FWD && TAPU)) {
      t_c += HBK;
      if (t_c >= a.Cin) { t_c = 0; if (++t_s == a.S) { t_s = 0; ++t_r; } }
    } else if constexpr (MODE == DGRAD) {
      t_c += HBK;
      if (t_c >= a.Cout) { t_c = 0; if (++t_s == a.ns) { t_s = 0; ++t_r; } }
    }
  };

  auto store = [&](int buf) {
    u16* A = smem + buf * STG;
    u16* Bm = A + A_SZ;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      if constexpr (A_COL) {
        const int idx = tid + 256 * j;
        *(u32x4*)(A + (idx / (BM / 8)) * cld(BM) + 8 * (idx % (BM / 8))) = ra[j];
      } else {
        *(u32x4*)(A + ((tid >> 2) + 64 * j) * RLD + 8 * kc) = ra[j];
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if constexpr (B_COL) {
        const int idx = tid + 256 * j;
        *(u32x4*)(Bm + (idx / (BN / 8)) * cld(BN) + 8 * (idx % (BN / 8))) = rb[j];
      } else {
        *(u32x4*)(Bm + ((tid >> 2) + 64 * j) * RLD + 8 * kc) = rb[j];
      }
    }
  };

  floatx16 acc[MI][NI];
  float cs[NI];  // the accumulators' start (conv_epi16.h): loaded here, filled behind the loads
  acc_shift16(cs, a, n0 + wn * WN, MODE == FWD);

  const int ntiles = (kend - kbeg + HBK - 1) / HBK;
  if (ntiles > 0) load(kbeg);
  acc_start16(acc, cs);
  if (ntiles > 0) store(0);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < ntiles; ++t) {
    const bool more = t + 1 < ntiles;
    if (more) load(kbeg + (t + 1) * HBK);
    const u16* A = smem + cur * STG;
    const u16* Bm = A + A_SZ;
#pragma unroll
    for (int s = 0; s < HBK / 16; ++s) {
      u32x4 af[MI], bfr[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
        af[mi] = A_COL ? col_frag(A, cld(BM), wm * WM + mi * 32, s, lane)
                       : row_frag_ld<RLD>(A, wm * WM + mi * 32, s, li, lh);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
        bfr[ni] = B_COL ? col_frag(Bm, cld(BN), wn * WN + ni * 32, s, lane)
                        : row_frag_ld<RLD>(Bm, wn * WN + ni * 32, s, li, lh);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = H16<DT>::mfma(af[mi], bfr[ni], acc[mi][ni]);
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // ---------------- epilogue (shared with the pipelined kernels) ----------------
  if constexpr (MODE == WGRAD)
    conv_epilogue<WGRAD, BM, BN, MI, NI, 2, 2>(a, acc, (float*)smem, tid, m0, n0, g, sp);
  else
    epilogue16<MODE, DT, BM, BN, MI, NI, 2, 2, sizeof(smem)>(a, acc, smem, m0, n0, g);
}

template <int MODE, int DT, int BM, int BN, bool TAPU>
static void launch16(const ConvArgs& a, hipStream_t st) {
  dim3 grid(ceil_div(a.M, BM) * ceil_div(a.N, BN), MODE == WGRAD ? a.G * a.splits : a.G);
  hipLaunchKernelGGL((conv_gemm_h16<MODE, DT, BM, BN, TAPU>), grid, dim3(256), 0, st, a);
}

template <int MODE, int DT, bool TAPU>
static void tiles16(const ConvArgs& a, hipStream_t st) {
  const int bm = conv_tile_rows(a.M), bn = conv_tile_rows(a.N);
  if (bm == 64 && bn == 64) launch16<MODE, DT, 64, 64, TAPU>(a, st);
  else if (bm == 64) launch16<MODE, DT, 64, 128, TAPU>(a, st);
  else if (bn == 64) launch16<MODE, DT, 128, 64, TAPU>(a, st);
  else launch16<MODE, DT, 128, 128, TAPU>(a, st);
}

template <int MODE, bool TAPU>
static void dispatch16(int dt, const ConvArgs& a, hipStream_t st) {
  if (dt == DT_BF16) tiles16<MODE, DT_BF16, TAPU>(a, st);
  else tiles16<MODE, DT_F16, TAPU>(a, st);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int check_shape16(const char* what, int dt, int G, int B, int Cin, int Cout,
                         const long long* xs) {
  if (dt != DT_BF16 && dt != DT_F16) { set_error(std::string(what) + ": dtype must be 0 (bf16) or 1 (f16)"); return kErrArg; }
  if (G <= 0 || B <= 0 || Cin <= 0 || Cout <= 0) { set_error(std::string(what) + ": bad shape"); return kErrArg; }
  if (Cin % 8 || Cout % 8) { set_error(std::string(what) + ": 16-bit path needs Cin, Cout % 8 == 0 (pad the stem input)"); return kErrArg; }
  if (xs && (xs[4] != 1 || xs[0] % 8 || xs[1] % 8 || xs[2] % 8 || xs[3] % 8)) {
    set_error(std::string(what) + ": x strides must be channel-contiguous multiples of 8");
    return kErrArg;
  }
  return 0;
}

}  // namespace mauv

using namespace mauv;

MAUV_API int mauv_conv2d_fwd_h16(int dtype, const void* x, const long long* x_strides,
                                 const float* x_scale, const float* x_shift, int x_relu,
                                 const void* w, void* y, int G, int B, int H, int W, int Cin,
                                 int Cout, int R, int S, int stride, int pad, float* st_mean,
                                 float* st_m2, float* st_cnt, const float* y_shift,
                                 hipStream_t stream) {
  if (int e = conv_check_geometry("conv2d_fwd_h16", G, B, H, W, Cin, Cout, R, S, stride, pad)) return e;
  if (int e = check_shape16("conv2d_fwd_h16", dtype, G, B, Cin, Cout, x_strides)) return e;
  if (!aligned16(x) || !aligned16(w)) { set_error("conv2d_fwd_h16: x, w must be 16-B aligned"); return kErrArg; }
  ConvArgs a = make_args(G, B, H, W, Cin, Cout, R, S, stride, pad, x_strides);
  a.x = (const float*)x; a.w = (const float*)w; a.out = (float*)y;
  a.xsc = x_scale; a.xsh = x_shift; a.xrelu = x_relu;
  a.M = B * a.Ho * a.Wo; a.N = Cout; a.K = R * S * Cin;
  a.out_sg = (long long)a.M * a.N;
  a.st_mean = st_mean; a.st_m2 = st_m2; a.st_cnt = st_cnt;
  a.st_nblk = stat_blocks(a.M);
  a.ysh = y_shift;
  if (conv_pipe16_launch(FWD, dtype, a, stream)) {}
  else if (Cin % HBK == 0) dispatch16<FWD, true>(dtype, a, stream);
  else dispatch16<FWD, false>(dtype, a, stream);
  return check_launch("conv2d_fwd_h16");
}

// A bottleneck's conv1 (1x1, stride 1) whose input is the previous block's output, formed while
// its tiles are loaded: out = relu(y*scale + shift + r), r = res or res*res_scale + res_shift
// (conv_big16.hip's fold; bn_apply's arithmetic), written through once (with out_mask non-null
// also its ReLU-mask bits, mauv_bn_apply_mask's) and fed to the GEMM.
// 0: launched; 1: shape outside the kernel (nothing launched: the caller runs mauv_bn_apply,
// then mauv_conv2d_fwd_h16 on its output); < 0: argument error.
MAUV_API int mauv_conv2d_fwd_fold_h16(int dtype, const void* y, const float* scale,
                                      const float* shift, const void* res, const float* res_scale,
                                      const float* res_shift, void* out, unsigned char* out_mask,
                                      const void* w, void* y1, int G, int B, int H, int W,
                                      int Cin, int Cout,
                                      float* st_mean, float* st_m2, float* st_cnt,
                                      const float* y1_shift, hipStream_t stream) {
  if (int e = check_shape16("conv2d_fwd_fold_h16", dtype, G, B, Cin, Cout, nullptr)) return e;
  if (!y || !scale || !shift || !res || !out || !w || !y1 || !res_scale != !res_shift) {
    set_error("conv2d_fwd_fold_h16: y, scale, shift, res, out, w, y1 required; res_scale and "
              "res_shift together");
    return kErrArg;
  }
  if (!aligned16(y) || !aligned16(res) || !aligned16(out) || !aligned16(w)) {
    set_error("conv2d_fwd_fold_h16: y, res, out, w must be 16-B aligned");
    return kErrArg;
  }
  ConvArgs a = make_args(G, B, H, W, Cin, Cout, 1, 1, 1, 0, nullptr);
  a.x = (const float*)y; a.w = (const float*)w; a.out = (float*)y1;
  a.xsc = scale; a.xsh = shift; a.xrelu = 1;
  a.M = B * H * W; a.N = Cout; a.K = Cin;
  a.out_sg = (long long)a.M * a.N;
  a.st_mean = st_mean; a.st_m2 = st_m2; a.st_cnt = st_cnt;
  a.st_nblk = stat_blocks(a.M);
  a.ysh = y1_shift;
  a.rs = res; a.rs_sc = res_scale; a.rs_sh = res_shift; a.fout = out; a.fmask = out_mask;
  if (!conv_big16_fold_launch(dtype, a, stream)) return 1;
  return check_launch("conv2d_fwd_fold_h16");
}

// 16-bit counterpart of mauv_stem_fwd_f32 (conv_gemm.hip): the pipelined kernel over the
// shared im2col rows with the G weight sets stacked along N; Kp % 64 == 0.
MAUV_API int mauv_stem_fwd_h16(int dtype, const void* cols, const void* w, void* y, int G,
                               int M, int Kp, int Cout, float* st_mean, float* st_m2,
                               float* st_cnt, const float* y_shift, hipStream_t stream) {
  if (int e = check_shape16("stem_fwd_h16", dtype, G, 1, Kp, Cout, nullptr)) return e;
  if (M <= 0 || Kp % 64) { set_error("stem_fwd_h16: needs M > 0 and Kp % 64 == 0"); return kErrArg; }
  if (!aligned16(cols) || !aligned16(w)) { set_error("stem_fwd_h16: cols, w must be 16-B aligned"); return kErrArg; }
  // cols as one 1 x M image of Kp channels
  ConvArgs a = make_args(1, 1, 1, M, Kp, G * Cout, 1, 1, 1, 0, nullptr);
  a.x = (const float*)cols; a.w = (const float*)w; a.out = (float*)y;
  a.M = M; a.N = G * Cout; a.K = Kp;
  a.out_sg = (long long)M * Cout;
  a.st_mean = st_mean; a.st_m2 = st_m2; a.st_cnt = st_cnt;
  a.st_nblk = stat_blocks(M);
  a.ysh = y_shift;
  a.cpg = Cout;
  // the pipelined kernel reads cols by a buffer descriptor: in row chunks (conv_stem_row_chunks)
  const long long rows = conv_stem_row_chunks(a, 2, [&](const ConvArgs& c) {
    return conv_pipe16_launch(FWD, dtype, c, stream);
  });
  if (rows != M) { set_error("stem_fwd_h16: shape outside the pipelined kernel"); return kErrArg; }
  return check_launch("stem_fwd_h16");
}

MAUV_API int mauv_conv2d_bwd_data_h16(int dtype, const void* dy, const void* w, void* dx,
                                      const void* addend, int accumulate, int G, int B, int H,
                                      int W, int Cin, int Cout, int R, int S, int stride, int pad,
                                      hipStream_t stream) {
  if (int e = conv_check_geometry("conv2d_bwd_data_h16", G, B, H, W, Cin, Cout, R, S, stride, pad)) return e;
  return mauv_conv2d_bwd_data_bn_h16(dtype, dy, w, dx, addend, accumulate, G, B, H, W, Cin, Cout,
                                     R, S, stride, pad, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                                     stream);
}

// The data gradient with the BN-backward partial sums of the BatchNorm whose output gradient dx
// is (bn_bwd_partial's sum dz, sum dz*xhat per [G][nblk][Cin], nblk =
// mauv_conv2d_bwd_data_stat_blocks) written by the epilogue (conv_epi16.h).  ReLU mask source:
// bn_mask bits (mauv_bn_apply_mask), else bn_out > 0, else bn_y*bn_scale + bn_shift > 0.  The
// partials need the pipelined kernel (Cout % 64 == 0) and every dx row written by this call
// (accumulate without addend over a tapless parity class is refused).  addend_mask (nullable):
// the addend counts only where these ReLU-mask bits ([G][B*H*W][Cin] / 8, mauv_bn_apply_mask)
// are set — the residual gradient of a block output's BN without a dres tensor.
MAUV_API int mauv_conv2d_bwd_data_bn_h16(int dtype, const void* dy, const void* w, void* dx,
                                         const void* addend, int accumulate, int G, int B, int H,
                                         int W, int Cin, int Cout, int R, int S, int stride,
                                         int pad, const unsigned char* addend_mask,
                                         const void* bn_y, const void* bn_out,
                                         const unsigned char* bn_mask, const float* bn_scale,
                                         const float* bn_shift, const float* bn_mean,
                                         const float* bn_invstd, int bn_relu, float* bn_p1,
                                         float* bn_p2, hipStream_t stream) {
  if (int e = conv_check_geometry("conv2d_bwd_data_bn_h16", G, B, H, W, Cin, Cout, R, S, stride, pad)) return e;
  if (int e = check_shape16("conv2d_bwd_data_h16", dtype, G, B, Cin, Cout, nullptr)) return e;
  if (Cout % HBK) { set_error("conv2d_bwd_data_h16: needs Cout % 32 == 0"); return kErrArg; }
  const bool bst = bn_p1 != nullptr;
  if (addend_mask && (!addend || Cout % 64)) { set_error("conv2d_bwd_data_bn_h16: addend_mask needs an addend and Cout % 64 == 0"); return kErrArg; }
  if (bst) {
    if (!bn_p2 || !bn_y || !bn_mean || !bn_invstd || Cout % 64) { set_error("conv2d_bwd_data_bn_h16: partials need p1, p2, y, mean, invstd and Cout % 64 == 0"); return kErrArg; }
    if (bn_relu && !bn_mask && !bn_out && (!bn_scale || !bn_shift)) { set_error("conv2d_bwd_data_bn_h16: relu mask needs mask, out or scale/shift"); return kErrArg; }
    if (!aligned16(bn_y) || !aligned16(bn_out)) { set_error("conv2d_bwd_data_bn_h16: y, out must be 16-B aligned"); return kErrArg; }
  }
  ConvArgs a = make_args(G, B, H, W, Cin, Cout, R, S, stride, pad, nullptr);
  a.dy = (const float*)dy; a.w = (const float*)w; a.out = (float*)dx;
  a.addend = (const float*)addend; a.accumulate = accumulate;
  a.add_mask = addend_mask;
  a.N = Cin;
  a.out_sg = (long long)B * H * W * Cin;
  if (bst) {
    a.bp_y = (const float*)bn_y; a.bp_out = (const float*)bn_out; a.bp_mask = bn_mask;
    a.bp_sc = bn_scale; a.bp_sh = bn_shift; a.bp_mean = bn_mean; a.bp_invstd = bn_invstd;
    a.bp_relu = bn_relu; a.bp_p1 = bn_p1; a.bp_p2 = bn_p2;
    a.bp_nblk = mauv_conv2d_bwd_data_stat_blocks(G, B, H, W, Cin, Cout, R, S, stride, pad);
  }
  // one launch per output-parity class (stride^2 of them; 1 for stride 1)
  for (int ph = 0; ph < stride; ++ph)
    for (int pw = 0; pw < stride; ++pw) {
      conv_parity_class(a, ph, pw);
      if (a.M <= 0) continue;
      // a tapless class accumulating into dx adds nothing (stride-2 1x1 downsample: 3 of 4)
      if (a.K == 0 && accumulate && !addend) {
        if (bst) { set_error("conv2d_bwd_data_bn_h16: partials over a tapless accumulate class"); return kErrArg; }
        continue;
      }
      if (!conv_pipe16_launch(DGRAD, dtype, a, stream)) {
        // the register-staged kernel writes no partials and reads no addend mask
        if (bst) { set_error("conv2d_bwd_data_bn_h16: shape outside the pipelined kernel"); return kErrArg; }
        if (addend_mask) { set_error("conv2d_bwd_data_bn_h16: addend_mask outside the pipelined kernel"); return kErrArg; }
        dispatch16<DGRAD, true>(dtype, a, stream);
      }
      a.bp_base += stat_blocks(a.M);
    }
  return check_launch("conv2d_bwd_data_h16");
}

MAUV_API int mauv_conv2d_bwd_weight_h16(int dtype, const void* x, const long long* x_strides,
                                        const float* x_scale, const float* x_shift, int x_relu,
                                        const void* dy, float* ws, int splits, int G, int B,
                                        int H, int W, int Cin, int Cout, int R, int S, int stride,
                                        int pad, hipStream_t stream) {
  if (int e = conv_check_geometry("conv2d_bwd_weight_h16", G, B, H, W, Cin, Cout, R, S, stride, pad, splits)) return e;
  if (int e = check_shape16("conv2d_bwd_weight_h16", dtype, G, B, Cin, Cout, x_strides)) return e;
  ConvArgs a = make_args(G, B, H, W, Cin, Cout, R, S, stride, pad, x_strides);
  a.x = (const float*)x; a.dy = (const float*)dy; a.out = ws;
  a.xsc = x_scale; a.xsh = x_shift; a.xrelu = x_relu;
  a.M = Cout; a.N = R * S * Cin; a.K = B * a.Ho * a.Wo;
  a.splits = splits;
  // whole tile depths per split-K slice: the pipelined kernel's 64, else HBK
  a.kchunk = ((a.K + splits - 1) / splits + 63) / 64 * 64;
  if (!conv_pipe16_launch(WGRAD, dtype, a, stream)) {
    a.kchunk = ((a.K + splits - 1) / splits + HBK - 1) / HBK * HBK;
    dispatch16<WGRAD, false>(dtype, a, stream);
  }
  return check_launch("conv2d_bwd_weight_h16");
}

