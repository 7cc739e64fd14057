// The stems' data gradient: d loss / d images through conv1 of each trunk, summed over the G MC
// samples (they all convolve the SAME images, stem.hip), in two deterministic stages:
//
//   drows[m][k] = sum_g sum_co dy[g][m][co] * w[g][co][k]      one GEMM  M x Kp x (G*Cout)
//   dx[b][c][ih][iw] = sum over the taps (r, s) that reach the pixel of
//                      drows[(b, oh, ow)][c*R*S + r*S + s]      col2im, the mirror of im2col
//
// The GEMM's K loop runs over (g, co): the sum over the samples happens in the fp32 accumulators
// (no per-sample intermediate, no read-modify-write, no 16-bit rounding between samples).  drows
// is always fp32; col2im gathers (one thread per dx element, taps in a fixed order): no atomics,
// so both stages give the same bits on every run.  The padded columns k >= C*R*S of drows come
// out 0 (w's padding is 0) and col2im never reads them.
//
// GEMM tiles: 256 threads = 4 waves (2x2), block tile 128 x BN (BN = 64 or 128 columns of Kp),
// double-buffered LDS, operands staged global -> registers -> LDS.
//   16-bit  v_mfma_f32_32x32x16_{bf16,f16}: dy rows are k-contiguous -> row image [128][32+8]
//           (one ds_read_b128 per fragment); w rows are n-contiguous, k-strided -> col image
//           [32][BN+32] read with the hardware-transposed col_frag (h16.h).
//   fp32    v_mfma_f32_32x32x2_f32 (exact products, fmaf-chain accumulation): both operands
//           k-major, [16][128+2] (dy, transposed while stored) and [16][BN+32] (w), one
//           ds_read_b32 per lane and k.
#include "h16.h"

using namespace mauv;

namespace mauv {

constexpr int kRowsBM = 128;        // rows of drows per block
constexpr int kMaxStemKp = 2048;    // as im2col's (stem.hip)

// DT: -1 fp32, DT_BF16, DT_F16.  Kt = G * Cout, the GEMM's K; a 16-byte chunk of dy (8 16-bit
// or 4 fp32 values along co) never straddles two samples because Cout % 8 == 0.
template <int DT, int BN>
__global__ __launch_bounds__(256) void stem_bwd_rows_kernel(const void* __restrict__ dy_,
                                                            const void* __restrict__ w_,
                                                            float* __restrict__ drows, int G,
                                                            int M, int Kp, int Cout, int ntn) {
  constexpr bool F32 = DT < 0;
  constexpr int BM = kRowsBM, BK = F32 ? 16 : 32;
  constexpr int WM = BM / 2, WN = BN / 2, MI = WM / 32, NI = WN / 32;
  // LDS images, in elements of the operand type
  // fp32: [BK][BM+2]; 16-bit: [BM][BK+8].  BM + 2: the transposed store below writes k rows
  // 4 a_kc + e for 8 consecutive rows per 32-lane half, and 4 * 130 = 8 (mod 32 banks, the
  // ds_write modulus) puts the four a_kc on banks 0-7, 8-15, 16-23, 24-31: conflict-free
  constexpr int LDA = F32 ? BM + 2 : BK + 8;
  constexpr int LDB = BN + 32;                   // [BK][BN+32] in both
  constexpr int A_SZ = F32 ? BK * LDA : BM * LDA;
  constexpr int B_SZ = BK * LDB;
  constexpr int ESZ = F32 ? 4 : 2;
  constexpr int STG = A_SZ + B_SZ;
  constexpr int NA = 2;            // 16-byte chunks of dy per thread and stage (512 per stage)
  constexpr int NB = BN / 64;      // 16-byte chunks of w per thread and stage
  constexpr int EPC = 16 / ESZ;    // elements per 16-byte chunk
  __shared__ __attribute__((aligned(16))) unsigned char smem_raw[2 * STG * ESZ];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int nt = (int)(blockIdx.x % (unsigned)ntn), mt = (int)(blockIdx.x / (unsigned)ntn);
  const int m0 = mt * BM, n0 = nt * BN;
  const int Kt = G * Cout;

  // per-thread loader state: A chunk j = (row a_row[j], k chunk a_kc), B chunk j = (k row, cols)
  const int a_kc = tid & 3;
  int a_row[NA];
  bool a_ok[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    a_row[j] = (tid >> 2) + 64 * j;
    a_ok[j] = m0 + a_row[j] < M;
  }
  int b_kr[NB], b_cc[NB];
  bool b_ok[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int idx = tid + 256 * j;
    b_kr[j] = idx / (BN / EPC);
    b_cc[j] = EPC * (idx % (BN / EPC));
    b_ok[j] = n0 + b_cc[j] < Kp;
  }
  // (BK * BN / EPC chunks of w per stage: 16 * BN / 4 fp32, 32 * BN / 8 16-bit = 256 NB in both)
  static_assert(BK * BN / EPC == 256 * NB && BM * BK / EPC == 256 * NA, "loader coverage");

  u32x4 ra[NA], rb[NB];
  const u32x4 zero = {0u, 0u, 0u, 0u};

  auto load = [&](int k0) {
    const int kk = k0 + EPC * a_kc;
    const int g = kk / Cout, co = kk - g * Cout;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      u32x4 v = zero;
      if (a_ok[j] && kk < Kt) {
        const long long o = ((long long)g * M + (m0 + a_row[j])) * Cout + co;
        v = *(const u32x4*)((const unsigned char*)dy_ + o * ESZ);
      }
      ra[j] = v;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      u32x4 v = zero;
      const int kr = k0 + b_kr[j];
      if (b_ok[j] && kr < Kt) {
        const long long o = (long long)kr * Kp + n0 + b_cc[j];
        v = *(const u32x4*)((const unsigned char*)w_ + o * ESZ);
      }
      rb[j] = v;
    }
  };

  auto store = [&](int buf) {
    if constexpr (F32) {
      float* A = (float*)smem_raw + buf * STG;
      float* Bm = A + A_SZ;
#pragma unroll
      for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          A[(4 * a_kc + e) * LDA + a_row[j]] = __uint_as_float(ra[j][e]);
#pragma unroll
      for (int j = 0; j < NB; ++j) *(u32x4*)(Bm + b_kr[j] * LDB + b_cc[j]) = rb[j];
    } else {
      u16* A = (u16*)smem_raw + buf * STG;
      u16* Bm = A + A_SZ;
#pragma unroll
      for (int j = 0; j < NA; ++j) *(u32x4*)(A + a_row[j] * LDA + 8 * a_kc) = ra[j];
#pragma unroll
      for (int j = 0; j < NB; ++j) *(u32x4*)(Bm + b_kr[j] * LDB + b_cc[j]) = rb[j];
    }
  };

  floatx16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

  const int ntiles = (Kt + BK - 1) / BK;
  load(0);
  store(0);
  __syncthreads();
  int cur = 0;
  for (int t = 0; t < ntiles; ++t) {
    const bool more = t + 1 < ntiles;
    if (more) load((t + 1) * BK);
    if constexpr (F32) {
      const float* A = (const float*)smem_raw + cur * STG;
      const float* Bm = A + A_SZ;
#pragma unroll
      for (int k2 = 0; k2 < BK / 2; ++k2) {
        float av[MI], bv[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) av[mi] = A[(2 * k2 + lh) * LDA + wm * WM + mi * 32 + li];
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) bv[ni] = Bm[(2 * k2 + lh) * LDB + wn * WN + ni * 32 + li];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
      }
    } else {
      const u16* A = (const u16*)smem_raw + cur * STG;
      const u16* Bm = A + A_SZ;
#pragma unroll
      for (int s = 0; s < BK / 16; ++s) {
        u32x4 af[MI], bq[NI];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) af[mi] = row_frag_ld<LDA>(A, wm * WM + mi * 32, s, li, lh);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) bq[ni] = col_frag(Bm, LDB, wn * WN + ni * 32, s, lane);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NI; ++ni)
            acc[mi][ni] = H16<F32 ? 0 : DT>::mfma(af[mi], bq[ni], acc[mi][ni]);
      }
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // C/D layout of the 32x32 MFMAs: lane l = column l&31, register r = row (r&3) + 8(r>>2) + 4(l>>5)
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int col = n0 + wn * WN + ni * 32 + li;
      if (col >= Kp) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * WM + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row < M) drows[(long long)row * Kp + col] = acc[mi][ni][r];
      }
    }
}

// one thread per element of the fp32 NCHW gradient: the pixel (ih, iw) is tap (r, s) of the
// output pixels oh = (ih + pad - r) / stride, ow = (iw + pad - s) / stride where those divide —
// at most ceil(R/stride) * ceil(S/stride) of them — walked with oh, then ow ascending.  The
// element index is split with 32-bit arithmetic (host-checked B*C*H*W and M * Kp/8 < 2^31).
__global__ __launch_bounds__(256) void stem_col2im_kernel(const float* __restrict__ drows, int C,
                                                          int H, int W, int R, int S, int stride,
                                                          int pad, int Ho, int Wo, int Kp,
                                                          unsigned total,
                                                          float* __restrict__ dx) {
  const int RS = R * S;
  const unsigned HW = (unsigned)(H * W);
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const unsigned bc = i / HW, rem = i - bc * HW;
    const int ih = (int)(rem / (unsigned)W), iw = (int)rem - ih * W;
    const unsigned b = bc / (unsigned)C;
    const int c = (int)(bc - b * (unsigned)C);
    const int ph = ih + pad, pw = iw + pad;
    const int oh0 = ph >= R ? (ph - R) / stride + 1 : 0, oh1 = min(Ho - 1, ph / stride);
    const int ow0 = pw >= S ? (pw - S) / stride + 1 : 0, ow1 = min(Wo - 1, pw / stride);
    float acc = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh) {
      const int r = ph - oh * stride;
      const unsigned mrow = (b * (unsigned)Ho + (unsigned)oh) * (unsigned)Wo;
      const int kr = c * RS + r * S;
      for (int ow = ow0; ow <= ow1; ++ow) {
        const int s = pw - ow * stride;
        acc += drows[(long long)(mrow + (unsigned)ow) * Kp + kr + s];
      }
    }
    dx[i] = acc;
  }
}

static int refuse(const char* what, const std::string& msg) {
  set_error(std::string(what) + ": " + msg);
  return kErrArg;
}

static int positive(const char* what, const char* name, int v, int lo = 1) {
  if (v >= lo) return 0;
  return refuse(what, std::string(name) + " must be >= " + std::to_string(lo) + ", got " +
                          std::to_string(v));
}

static int check_kp(const char* what, int Kp) {
  if (Kp % 8) return refuse(what, "Kp must be a multiple of 8, got " + std::to_string(Kp));
  if (Kp > kMaxStemKp)
    return refuse(what, "Kp must be <= 2048, got " + std::to_string(Kp));
  return 0;
}

static int check_chunks(const char* what, long long M, int Kp) {
  if (M * (Kp / 8) >= (1LL << 31))
    return refuse(what, "M * Kp / 8 must be below 2^31 (row chunks), got " +
                            std::to_string(M * (Kp / 8)));
  return 0;
}

static int rows_check(const char* what, const void* dy, const void* w, const float* drows, int G,
                      int M, int Kp, int Cout) {
  if (int e = positive(what, "G", G)) return e;
  if (int e = positive(what, "M", M)) return e;
  if (int e = positive(what, "Kp", Kp)) return e;
  if (int e = positive(what, "Cout", Cout)) return e;
  if (int e = check_kp(what, Kp)) return e;
  if (Cout % 8) return refuse(what, "Cout must be a multiple of 8, got " + std::to_string(Cout));
  if (int e = check_chunks(what, M, Kp)) return e;
  if ((long long)G * Cout >= (1LL << 31))
    return refuse(what, "G * Cout must be below 2^31, got " + std::to_string((long long)G * Cout));
  if (!dy || !w || !drows) return refuse(what, "dy, w and drows must be non-null");
  if (((uintptr_t)dy | (uintptr_t)w | (uintptr_t)drows) & 15)
    return refuse(what, "dy, w and drows must be 16-byte aligned");
  return 0;
}

// 64-column tiles where they waste fewer columns of the last tile than 128-column ones
static bool rows_bn64(int Kp) { return (Kp + 63) / 64 * 64 < (Kp + 127) / 128 * 128; }

template <int DT>
static void rows_launch(const void* dy, const void* w, float* drows, int G, int M, int Kp,
                        int Cout, hipStream_t stream) {
  const long long mt = ((long long)M + kRowsBM - 1) / kRowsBM;
  if (rows_bn64(Kp)) {
    const int ntn = (Kp + 63) / 64;
    hipLaunchKernelGGL((stem_bwd_rows_kernel<DT, 64>), dim3((unsigned)(mt * ntn)), dim3(256), 0,
                       stream, dy, w, drows, G, M, Kp, Cout, ntn);
  } else {
    const int ntn = (Kp + 127) / 128;
    hipLaunchKernelGGL((stem_bwd_rows_kernel<DT, 128>), dim3((unsigned)(mt * ntn)), dim3(256), 0,
                       stream, dy, w, drows, G, M, Kp, Cout, ntn);
  }
}

}  // namespace mauv

// drows[M][Kp] (fp32) = sum_g dy[g][M][Cout] . w[g][Cout][Kp]; Kp % 8 == 0, Kp <= 2048,
// Cout % 8 == 0.
MAUV_API int mauv_stem_bwd_rows_f32(const float* dy, const float* w, float* drows, int G, int M,
                                    int Kp, int Cout, hipStream_t stream) {
  if (int e = rows_check("stem_bwd_rows_f32", dy, w, drows, G, M, Kp, Cout)) return e;
  rows_launch<-1>(dy, w, drows, G, M, Kp, Cout, stream);
  return check_launch("stem_bwd_rows_f32");
}

// dtype 0 = bf16, 1 = f16 operands dy and w; drows stays fp32.
MAUV_API int mauv_stem_bwd_rows_h16(int dtype, const void* dy, const void* w, float* drows, int G,
                                    int M, int Kp, int Cout, hipStream_t stream) {
  if (dtype != DT_BF16 && dtype != DT_F16) {
    set_error("stem_bwd_rows_h16: dtype must be 0 (bf16) or 1 (f16)");
    return kErrArg;
  }
  if (int e = rows_check("stem_bwd_rows_h16", dy, w, drows, G, M, Kp, Cout)) return e;
  if (dtype == DT_BF16) rows_launch<DT_BF16>(dy, w, drows, G, M, Kp, Cout, stream);
  else rows_launch<DT_F16>(dy, w, drows, G, M, Kp, Cout, stream);
  return check_launch("stem_bwd_rows_h16");
}

// dx[B][C][H][W] (fp32 NCHW) from drows[B*Ho*Wo][Kp]: the adjoint of mauv_stem_im2col's fp32 rows.
MAUV_API int mauv_stem_col2im(const float* drows, int B, int C, int H, int W, int R, int S,
                              int stride, int pad, int Kp, float* dx, hipStream_t stream) {
  const char* what = "stem_col2im";
  if (int e = positive(what, "B", B)) return e;
  if (int e = positive(what, "C", C)) return e;
  if (int e = positive(what, "H", H)) return e;
  if (int e = positive(what, "W", W)) return e;
  if (int e = positive(what, "R", R)) return e;
  if (int e = positive(what, "S", S)) return e;
  if (int e = positive(what, "stride", stride)) return e;
  if (int e = positive(what, "pad", pad, 0)) return e;
  if (int e = positive(what, "Kp", Kp)) return e;
  // the padded extents stay 32-bit (the kernel forms ih + pad), so Ho, Wo < 2^31 below
  if ((long long)H + 2LL * pad >= (1LL << 31) || (long long)W + 2LL * pad >= (1LL << 31))
    return refuse(what, "pad must keep H + 2 pad and W + 2 pad below 2^31, got " + std::to_string(pad));
  const long long nh = (long long)H + 2LL * pad - R, nw = (long long)W + 2LL * pad - S;
  const long long Ho = nh < 0 ? 0 : nh / stride + 1, Wo = nw < 0 ? 0 : nw / stride + 1;
  if (Ho < 1) return refuse(what, "Ho must be >= 1, got 0 (the filter is taller than the padded image)");
  if (Wo < 1) return refuse(what, "Wo must be >= 1, got 0 (the filter is wider than the padded image)");
  if (int e = check_kp(what, Kp)) return e;
  // (64-bit products formed in steps that cannot wrap: R * S first, then times C)
  const long long RS = (long long)R * S;
  if (RS > kMaxStemKp || RS * C > Kp)
    return refuse(what, "Kp must be >= C*R*S, got Kp = " + std::to_string(Kp) + " for C = " +
                            std::to_string(C) + ", R = " + std::to_string(R) + ", S = " + std::to_string(S));
  const long long HW = (long long)H * W, BC = (long long)B * C;
  if (HW >= (1LL << 31) || BC >= (1LL << 31) || BC * HW >= (1LL << 31))
    return refuse(what, "B * C * H * W must be below 2^31");
  const long long n = BC * HW;
  // Ho * Wo < 2^62 cannot wrap; times B only once it is known to be below 2^31
  if (Ho * Wo >= (1LL << 31))
    return refuse(what, "M * Kp / 8 must be below 2^31 (row chunks): Ho * Wo = " +
                            std::to_string(Ho * Wo) + " alone is not");
  if (int e = check_chunks(what, (long long)B * Ho * Wo, Kp)) return e;
  if (!drows || !dx) return refuse(what, "drows and dx must be non-null");
  long long nb = (n + 255) / 256;
  if (nb > 65536) nb = 65536;
  hipLaunchKernelGGL(stem_col2im_kernel, dim3((unsigned)nb), dim3(256), 0, stream, drows, C, H, W,
                     R, S, stride, pad, (int)Ho, (int)Wo, Kp, (unsigned)n, dx);
  return check_launch(what);
}
