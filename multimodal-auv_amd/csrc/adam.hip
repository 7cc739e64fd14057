// Fused multi-tensor Adam for the Bayesian parameter set.
//
// The reference builds torch.optim.Adam over the model's ~700 parameter tensors
// (train/loop_utils.py:45-61; lr 5e-5, weight_decay 1e-5 when retraining) and steps it after
// every batch (train/multimodal.py:141-143).  This is the same update — torch's Adam with
// amsgrad=False, maximize=False, L2 weight decay folded into the gradient — for every tensor of
// a table in ONE launch (grid.y = table entry), one read and one write of p, m, v and one read
// of g per element:
//   g' = g + wd * p;  m = m + (1 - b1) * (g' - m);  v = b2 * v + (1 - b2) * g'^2
//   p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// mauv_adam_step_ex is the same launch with torch's other options (amsgrad, maximize, decoupled
// weight decay) and up to 8 parameter groups, each row naming its group.
// The gated forms run ONE single-thread decision kernel first, then the Adam launch, which
// multiplies g as it loads it by 1 / scale (dynamic loss scaling, §2.37), 1 / micro (gradient
// accumulation, §2.39; mauv_accum_note counts the window's other micro-batches) and the clip
// coefficient (global-norm clipping, §2.36), each 1 when off, and moves each row's shadow towards
// the new p (weight EMA, §2.42).  The four gated all-groups entries differ only in which of the
// optional state pointers they take.  mauv_ema_update / mauv_ema_swap are the
// EMA's element update at a host-given weight and the in-place exchange of parameters and shadows.
#include "mauv_common.h"

using namespace mauv;

namespace mauv {

// One element of torch's Adam update (m, v, p updated in place).  The weight-decay term is
// stated as the single rounding fl(wd * p + g): left as g + wd * p the compiler fused it in the
// vector loops and the ungated kernels but rounded wd * p first in the gated kernels' scalar
// loops, so one element's bits depended on its row's alignment and on the entry point.
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float omb1,
                                          float beta2, float omb2, float eps, float wd,
                                          float step_size, float bc2_sqrt) {
  const float ge = wd != 0.f ? __builtin_fmaf(wd, p, g) : g;
  m = m + omb1 * (ge - m);
  v = v * beta2 + omb2 * ge * ge;
  p = p - step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
}

// MODE 1: Adam update; MODE 3: Adam update, then the gradient is zeroed (the reference's
// optimizer.zero_grad() after a successful step, multimodal.py:141-143); MODE 2: zero the
// gradient only.  The gated launch reads the mode and constants from the device gate.
template <bool GATED>
__global__ __launch_bounds__(256) void adam_kernel(const MauvAdamEntry* __restrict__ tab,
                                                   float lr, float beta1, float beta2, float eps,
                                                   float wd, float step_size, float bc2_sqrt,
                                                   const MauvStepGate* __restrict__ gate) {
  int mode = 1;
  float clip = 1.0f;   // the gate's clip coefficient (1 when clipping is off: g * 1 is g)
  if (GATED) {
    mode = gate->mode;
    if (mode == 0) return;
    step_size = gate->step_size;
    bc2_sqrt = gate->bc2_sqrt;
    clip = gate->clip_coef;
  }
  const MauvAdamEntry t = tab[blockIdx.y];
  float* grad = const_cast<float*>(t.grad);
  const bool upd = mode & 1, zero = mode & 2;
  // 16-byte vector path only when all four tensors are 16-byte aligned (a parameter may be
  // a view at any offset); otherwise every element takes the scalar loop below
  const bool aligned = ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) |
                         reinterpret_cast<uintptr_t>(t.exp_avg) |
                         reinterpret_cast<uintptr_t>(t.exp_avg_sq)) & 15) == 0;
  const long long n4 = aligned ? t.numel / 4 : 0;
  const float omb1 = 1.0f - beta1, omb2 = 1.0f - beta2;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    if (upd) {
      floatx4 p = ((const floatx4*)t.param)[i];
      floatx4 g = ((const floatx4*)t.grad)[i];
      floatx4 m = ((const floatx4*)t.exp_avg)[i];
      floatx4 v = ((const floatx4*)t.exp_avg_sq)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        // the clipped gradient is rounded on its own (never contracted into g + wd * p), as
        // if it had been clipped in place before the step
        adam_elem(pe, GATED ? __fmul_rn(g[e], clip) : g[e], me, ve, omb1, beta2, omb2, eps, wd,
                  step_size, bc2_sqrt);
        p[e] = pe; m[e] = me; v[e] = ve;
      }
      ((floatx4*)t.param)[i] = p;
      ((floatx4*)t.exp_avg)[i] = m;
      ((floatx4*)t.exp_avg_sq)[i] = v;
    }
    if (zero) ((floatx4*)grad)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  // scalar tail
  const long long base = n4 * 4;
  for (long long i = base + blockIdx.x * 256LL + threadIdx.x; i < t.numel;
       i += (long long)gridDim.x * 256) {
    if (upd) {
      float p = t.param[i], m = t.exp_avg[i], v = t.exp_avg_sq[i];
      adam_elem(p, GATED ? __fmul_rn(t.grad[i], clip) : t.grad[i], m, v, omb1, beta2, omb2, eps,
                wd, step_size, bc2_sqrt);
      t.param[i] = p;
      t.exp_avg[i] = m;
      t.exp_avg_sq[i] = v;
    }
    if (zero) grad[i] = 0.f;
  }
}

// The "otherwise" branch of both decisions below: the bias-correction constants at the next
// step count, Adam + zero_grad.
__device__ __forceinline__ void gate_take_step(MauvStepGate* g, float lr, float beta1,
                                               float beta2) {
  const int t = g->step + 1;
  const double bc1 = 1.0 - pow((double)beta1, (double)t);
  const double bc2 = 1.0 - pow((double)beta2, (double)t);
  g->step = t;
  g->step_size = (float)((double)lr / bc1);
  g->bc2_sqrt = (float)sqrt(bc2);
  g->mode = 3;
  g->poisoned = 0;
  g->stepped = 1;
}

// The step decision of train/multimodal.py:133-145 taken on the device (one thread):
//   loss non-finite  -> no step; the batch's gradients are taken back out of the arena
//                       (mode 2 zeroes it when it was clean before; a poisoned arena stays)
//   grads non-finite -> no step, no zero_grad: the arena keeps them ("poisoned")
//   otherwise        -> Adam at step count t+1, then zero_grad (mode 3)
// With a loss scaler `s` beside the gate the arena holds the gradients of
// loss * scale, and:
//   loss non-finite  -> as above; the scaler is not touched (a NaN input is no overflow)
//   grads non-finite -> an overflow of the scaled gradients: no step, the arena is zeroed
//                       (mode 2; never "poisoned": the next batch starts clean, as GradScaler
//                       followed by zero_grad), scale *= backoff_factor, growth_tracker = 0
//   otherwise        -> Adam + zero_grad as above; growth_tracker += 1, and when it reaches
//                       growth_interval: scale *= growth_factor if that is finite (torch's
//                       _amp_update_scale_), growth_tracker = 0
// growth_interval == 0 is a static scale: only the counters move.  unscale = 1 / scale is formed
// from the scale the backward ran with, before it changes.
// Then the non-finite counter is reset for the next scan, and every decision writes the clip
// coefficient the Adam kernels multiply the gradient by: torch's clip_grad_norm_ formula over
// the scan's grad_norm when max_norm > 0, else 1 (unused when the step is skipped).  The scanned
// norm is that of the scaled, summed gradients, so grad_norm is first rewritten as the true norm.
// `ok_loss`: the loss was finite (a window of micro-batches: every one of them); `loss_skips`:
// what a bad loss adds to skipped_loss (1, or 0 when mauv_accum_note counted it already); `avg`:
// 1, or 1 / micro of a closing window.
__device__ __forceinline__ void gate_decide(MauvStepGate* g, MauvLossScale* s, int ok_loss,
                                            int loss_skips, float avg, float lr, float beta1,
                                            float beta2) {
  const int ok_grad = g->nonfinite == 0;
  float unscale = 1.0f;
  if (!s) {
    if (ok_loss && ok_grad) {
      gate_take_step(g, lr, beta1, beta2);
    } else {
      g->stepped = 0;
      if (!ok_loss) {
        g->mode = g->poisoned ? 0 : 2;
        g->skipped_loss += loss_skips;
      } else {
        g->mode = 0;
        g->poisoned = 1;
        g->skipped_grad += 1;
      }
    }
  } else {
    const float scale = s->scale;
    const bool dynamic = s->growth_interval != 0;
    unscale = (float)(1.0 / (double)scale);
    s->unscale = unscale;
    if (!ok_loss) {
      g->stepped = 0;
      g->mode = g->poisoned ? 0 : 2;
      g->skipped_loss += loss_skips;
    } else if (!ok_grad) {
      g->stepped = 0;
      g->mode = 2;
      g->poisoned = 0;
      g->skipped_grad += 1;
      s->overflows += 1;
      if (dynamic) {
        s->scale = (float)((double)scale * (double)s->backoff_factor);   // torch's rounding
        s->growth_tracker = 0;
      }
    } else {
      gate_take_step(g, lr, beta1, beta2);
      if (dynamic) {
        const int ok_steps = s->growth_tracker + 1;
        if (ok_steps == s->growth_interval) {
          const float grown = (float)((double)scale * (double)s->growth_factor);
          if (isfinite(grown)) s->scale = grown;
          s->growth_tracker = 0;
          s->growths += 1;
        } else {
          s->growth_tracker = ok_steps;
        }
      }
    }
  }
  g->nonfinite = 0;
  if (g->max_norm > 0.f) {
    if (s) g->grad_norm = __fmul_rn(g->grad_norm, unscale);   // (a NaN stays NaN)
    if (avg != 1.0f) g->grad_norm = __fmul_rn(g->grad_norm, avg);
    g->clip_coef = clip_coef(g->max_norm, g->grad_norm);
  } else {
    g->clip_coef = 1.0f;
  }
}

// ---- gradient accumulation -------------------------------------------------
// A micro-batch that does not close its window (one thread): it is counted, a non-finite loss
// is remembered, and the gate reports "no step" (no Adam launch follows).
__global__ void accum_note_kernel(MauvStepGate* g, MauvAccum* a) {
  a->micro += 1;
  if (g->ok_loss == 0) {
    a->bad_loss += 1;
    g->skipped_loss += 1;
  }
  g->stepped = 0;
  g->mode = 0;
}

// The decision kernel of every gated entry (one thread); `s`, `a` and `e` may each be NULL.
// With a window `a` this is its closing micro-batch: folded in as above, then one decision for
// the window, "loss ok" being "no micro-batch of it had a non-finite loss".  With a weight EMA `e`
// (DESIGN.md §2.42), and only when the decision is "Adam step" (mode bit 1), the weight of this
// update: 1 for the first one (torch's AveragedModel copies), else 1 - decay, the decay capped at
// (1 + n) / (10 + n) under timm's warm-up.  Every other decision leaves the MauvEma as it is.
__global__ void step_gate_kernel(MauvStepGate* g, MauvLossScale* s, MauvAccum* a, MauvEma* e,
                                 float lr, float beta1, float beta2) {
  if (a) {
    const int bad_now = g->ok_loss == 0;
    const int micro = a->micro + 1, bad = a->bad_loss + bad_now;
    const float avg = (float)(1.0 / (double)micro);
    a->avg = avg;
    gate_decide(g, s, bad == 0, bad_now, avg, lr, beta1, beta2);
    a->windows += 1;
    a->dropped += bad != 0;
    a->micro = 0;
    a->bad_loss = 0;
  } else {
    gate_decide(g, s, g->ok_loss != 0, 1, 1.0f, lr, beta1, beta2);
  }
  if (e && (g->mode & 1)) {
    const int n = e->updates;
    float w = 1.0f;
    if (n != 0) {
      double d = (double)e->decay;
      if (e->warmup) d = fmin(d, (1.0 + (double)n) / (10.0 + (double)n));
      w = (float)(1.0 - d);
    }
    e->weight = w;
    e->updates = n + 1;
  }
}

// ---- weight EMA: the element code ------------------------------------------------------------
// The new p as the average reads it: the value the Adam update has settled on, opaque to the
// compiler, so that the update's own arithmetic (which products it fuses) is compiled exactly as
// in the instantiations without an average and p keeps their bits.
__device__ __forceinline__ float settled(float p) {
  asm volatile("" : "+v"(p));
  return p;
}

// One element of the average: torch's lerp for weights below 0.5, e + w (p - e) with the product
// and the sum in one rounding; w == 1 copies (exact also where p - e would overflow).
__device__ __forceinline__ float ema_elem(float e, float p, float w) {
  return w == 1.0f ? p : __builtin_fmaf(w, p - e, e);
}

// ---- every option, several parameter groups (mauv_adam_step_ex) ------------------------------
// The groups travel by value in the kernel arguments (a StepLR-changed lr needs no device copy);
// step_size / bc2_sqrt are the host's for the ungated step, formed per block from the gate's
// count for the gated one.
struct AdamGroupsArg {
  MauvAdamGroup g[MAUV_ADAM_MAX_GROUPS];
  float step_size[MAUV_ADAM_MAX_GROUPS];
  float bc2_sqrt[MAUV_ADAM_MAX_GROUPS];
};

struct AdamConsts {
  float omb1, beta2, omb2, eps, wd, decay, step_size, bc2_sqrt, clip, unscale, avg;
};

// The gradient a gated step loads: unscaled, averaged over an accumulation window's
// micro-batches, clipped; every factor is 1 when off (g * 1 is g).  Contraction is off for this
// statement (__fmul_rn is a plain product here and could be fused): the three products are
// rounded one by one and none of them is fused into the arithmetic that follows, so the element
// equals the step on gradients multiplied in place, one factor at a time.
__device__ __forceinline__ float loaded_grad(float g, float unscale, float avg, float clip) {
#pragma clang fp contract(off)
  return ((g * unscale) * avg) * clip;
}

// One element of torch's single-tensor Adam with the row's options; all off is adam_elem.
template <bool AMS, bool MAXI, bool DEC>
__device__ __forceinline__ void adam_elem_ex(float& p, float g, float& m, float& v, float& vmax,
                                             const AdamConsts& k) {
  // first, where torch's GradScaler.unscale_ and then clip_grad_norm_ work: on .grad before
  // step(), with the 1 / micro of an accumulation window in between (the mean of the unscaled
  // micro-batch gradients is what gets clipped)
  g = loaded_grad(g, k.unscale, k.avg, k.clip);
  if (!AMS && !MAXI && !DEC) {
    adam_elem(p, g, m, v, k.omb1, k.beta2, k.omb2, k.eps, k.wd, k.step_size, k.bc2_sqrt);
    return;
  }
  if (MAXI) g = -g;
  float ge = g;
  if (k.wd != 0.f) {
    if (DEC) p = p * k.decay;
    else ge = __builtin_fmaf(k.wd, p, g);   // one rounding, as adam_elem
  }
  m = m + k.omb1 * (ge - m);
  v = v * k.beta2 + k.omb2 * ge * ge;
  float d = v;
  if (AMS) {
    vmax = (v > vmax || v != v) ? v : vmax;   // torch.maximum: a NaN on either side stays
    d = vmax;
  }
  p = p - k.step_size * (m / (sqrtf(d) / k.bc2_sqrt + k.eps));
}

// The loops of adam_kernel for one row, with a fifth tensor when AMS.  EMA: the row's shadow
// tensor `sh` moves towards the new p at weight w, read and written beside p (only on an
// updating step: a shadow is never touched otherwise).  sh16: the shadow is 16-byte aligned;
// one that is not is read and written float by float inside the vector loop, because the two
// loops of the Adam update do not round alike (the compiler fuses their products differently):
// a row must not change loops, and with them the bits of p, m and v, over its shadow's address.
template <bool AMS, bool MAXI, bool DEC, bool EMA>
__device__ __forceinline__ void adam_row(const MauvAdamEntryEx& t, long long n4, bool upd,
                                         bool zero, const AdamConsts& k, float* sh = nullptr,
                                         float w = 1.0f, bool sh16 = true) {
  float* grad = const_cast<float*>(t.grad);
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    if (upd) {
      floatx4 p = ((const floatx4*)t.param)[i];
      floatx4 g = ((const floatx4*)t.grad)[i];
      floatx4 m = ((const floatx4*)t.exp_avg)[i];
      floatx4 v = ((const floatx4*)t.exp_avg_sq)[i];
      floatx4 x = floatx4{0.f, 0.f, 0.f, 0.f};
      if (AMS) x = ((const floatx4*)t.max_exp_avg_sq)[i];
      floatx4 s = floatx4{0.f, 0.f, 0.f, 0.f};
      if (EMA) {
        if (sh16) s = ((const floatx4*)sh)[i];
        else s = floatx4{sh[4 * i], sh[4 * i + 1], sh[4 * i + 2], sh[4 * i + 3]};
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e], xe = x[e];
        adam_elem_ex<AMS, MAXI, DEC>(pe, g[e], me, ve, xe, k);
        p[e] = pe; m[e] = me; v[e] = ve; x[e] = xe;
        if (EMA) s[e] = ema_elem(s[e], settled(pe), w);
      }
      ((floatx4*)t.param)[i] = p;
      ((floatx4*)t.exp_avg)[i] = m;
      ((floatx4*)t.exp_avg_sq)[i] = v;
      if (AMS) ((floatx4*)t.max_exp_avg_sq)[i] = x;
      if (EMA) {
        if (sh16) {
          ((floatx4*)sh)[i] = s;
        } else {
          sh[4 * i] = s[0]; sh[4 * i + 1] = s[1]; sh[4 * i + 2] = s[2]; sh[4 * i + 3] = s[3];
        }
      }
    }
    if (zero) ((floatx4*)grad)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
  // scalar tail
  const long long base = n4 * 4;
  for (long long i = base + blockIdx.x * 256LL + threadIdx.x; i < t.numel;
       i += (long long)gridDim.x * 256) {
    if (upd) {
      float p = t.param[i], m = t.exp_avg[i], v = t.exp_avg_sq[i], x = 0.f;
      if (AMS) x = t.max_exp_avg_sq[i];
      adam_elem_ex<AMS, MAXI, DEC>(p, t.grad[i], m, v, x, k);
      t.param[i] = p;
      t.exp_avg[i] = m;
      t.exp_avg_sq[i] = v;
      if (AMS) t.max_exp_avg_sq[i] = x;
      if (EMA) sh[i] = ema_elem(sh[i], settled(p), w);
    }
    if (zero) grad[i] = 0.f;
  }
}

// The row's loops for its group's option flags (uniform over the block).
template <bool EMA>
__device__ __forceinline__ void adam_row_flags(unsigned flags, const MauvAdamEntryEx& t,
                                               long long n4, bool upd, bool zero,
                                               const AdamConsts& k, float* sh = nullptr,
                                               float w = 1.0f, bool sh16 = true) {
  switch (flags) {
    case 0: adam_row<false, false, false, EMA>(t, n4, upd, zero, k, sh, w, sh16); break;
    case 1: adam_row<true, false, false, EMA>(t, n4, upd, zero, k, sh, w, sh16); break;
    case 2: adam_row<false, true, false, EMA>(t, n4, upd, zero, k, sh, w, sh16); break;
    case 3: adam_row<true, true, false, EMA>(t, n4, upd, zero, k, sh, w, sh16); break;
    case 4: adam_row<false, false, true, EMA>(t, n4, upd, zero, k, sh, w, sh16); break;
    case 5: adam_row<true, false, true, EMA>(t, n4, upd, zero, k, sh, w, sh16); break;
    case 6: adam_row<false, true, true, EMA>(t, n4, upd, zero, k, sh, w, sh16); break;
    default: adam_row<true, true, true, EMA>(t, n4, upd, zero, k, sh, w, sh16); break;
  }
}

// grid.y = table row, as adam_kernel; the row's group gives the constants and the options,
// which are uniform over the block: one branch per block, outside the element loops.  EMA (gated
// only): ema_rows[row] is the row's shadow tensor or NULL, ema->weight this update's weight; the
// EMA-off instantiations never look at either.
template <bool GATED, bool EMA>
__global__ __launch_bounds__(256) void adam_ex_kernel(const MauvAdamEntryEx* __restrict__ tab,
                                                      AdamGroupsArg ga, int n_groups,
                                                      const MauvStepGate* __restrict__ gate,
                                                      const MauvLossScale* __restrict__ ls,
                                                      const MauvAccum* __restrict__ acc,
                                                      float* const* __restrict__ ema_rows,
                                                      const MauvEma* __restrict__ ema) {
  int mode = 1;
  if (GATED) {
    mode = gate->mode;
    if (mode == 0) return;
  }
  const MauvAdamEntryEx t = tab[blockIdx.y];
  if (t.group < 0 || t.group >= n_groups) return;
  const int gi = (int)t.group;
  const unsigned flags = ga.g[gi].flags & 7u;
  if ((flags & MAUV_ADAM_AMSGRAD) && !t.max_exp_avg_sq) return;
  // a shadow is touched by an updating step only
  float* sh = (EMA && (mode & 1)) ? ema_rows[blockIdx.y] : nullptr;
  // 16-byte vector path only when all (up to five) tensors are 16-byte aligned
  const bool aligned = ((reinterpret_cast<uintptr_t>(t.param) | reinterpret_cast<uintptr_t>(t.grad) |
                         reinterpret_cast<uintptr_t>(t.exp_avg) |
                         reinterpret_cast<uintptr_t>(t.exp_avg_sq) |
                         reinterpret_cast<uintptr_t>(t.max_exp_avg_sq)) & 15) == 0;
  const long long n4 = aligned ? t.numel / 4 : 0;
  // a block past the row's end (most blocks of a small tensor) has nothing to do
  const long long first = blockIdx.x * 256LL;
  if (first >= n4 && n4 * 4 + first >= t.numel) return;
  const float lr = ga.g[gi].lr, beta1 = ga.g[gi].beta1, wd = ga.g[gi].weight_decay;
  AdamConsts k;
  k.beta2 = ga.g[gi].beta2;
  k.omb1 = 1.0f - beta1;
  k.omb2 = 1.0f - k.beta2;
  k.eps = ga.g[gi].eps;
  k.wd = wd;
  k.decay = (float)(1.0 - (double)lr * (double)wd);
  k.step_size = ga.step_size[gi];
  k.bc2_sqrt = ga.bc2_sqrt[gi];
  k.clip = GATED ? gate->clip_coef : 1.0f;
  k.unscale = (GATED && ls) ? ls->unscale : 1.0f;   // written by step_gate_scaled_kernel
  k.avg = (GATED && acc) ? acc->avg : 1.0f;         // written by step_gate_accum_kernel
  if (GATED && (mode & 1)) {   // as step_gate_kernel forms them, at the gate's count
    const int st = gate->step;
    const double bc1 = 1.0 - pow((double)beta1, (double)st);
    const double bc2 = 1.0 - pow((double)k.beta2, (double)st);
    k.step_size = (float)((double)lr / bc1);
    k.bc2_sqrt = (float)sqrt(bc2);
  }
  const bool upd = mode & 1, zero = mode & 2;
  if (EMA && sh)
    adam_row_flags<true>(flags, t, n4, upd, zero, k, sh, ema->weight,
                         (reinterpret_cast<uintptr_t>(sh) & 15) == 0);
  else adam_row_flags<false>(flags, t, n4, upd, zero, k);
}

// ---- the average at a host-given weight, and the exchange (mauv_ema_update / mauv_ema_swap) ---
// grid.y = row, the loops of adam_row: 16-byte vectors when both tensors are 16-byte aligned.
template <bool SWAP>
__global__ __launch_bounds__(256) void ema_rows_kernel(const MauvEmaRow* __restrict__ rows,
                                                       float w) {
  const MauvEmaRow t = rows[blockIdx.y];
  if (!t.ema || !t.param) return;
  float* par = const_cast<float*>(t.param);
  const bool aligned = ((reinterpret_cast<uintptr_t>(t.ema) |
                         reinterpret_cast<uintptr_t>(t.param)) & 15) == 0;
  const long long n4 = aligned ? t.numel / 4 : 0;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const floatx4 p = ((const floatx4*)t.param)[i];
    floatx4 s = ((const floatx4*)t.ema)[i];
    if (SWAP) {
      ((floatx4*)par)[i] = s;
      s = p;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = ema_elem(s[e], p[e], w);
    }
    ((floatx4*)t.ema)[i] = s;
  }
  // scalar tail
  const long long base = n4 * 4;
  for (long long i = base + blockIdx.x * 256LL + threadIdx.x; i < t.numel;
       i += (long long)gridDim.x * 256) {
    const float p = t.param[i], s = t.ema[i];
    if (SWAP) {
      par[i] = s;
      t.ema[i] = p;
    } else {
      t.ema[i] = ema_elem(s, p, w);
    }
  }
}

}  // namespace mauv

// One Adam step (bias-correction step index `step` >= 1, shared by the table) for n tensors.
// Entries whose pointers are all 16-byte aligned take 16-byte vector loads, others scalar ones.
MAUV_API int mauv_adam_step(const MauvAdamEntry* table, int n, float lr, float beta1,
                            float beta2, float eps, float weight_decay, long long step,
                            hipStream_t stream) {
  if (n <= 0 || n > 65535 || step < 1) { set_error("adam_step: bad table size / step"); return kErrArg; }
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(adam_kernel<false>, dim3(64, n), dim3(256), 0, stream, table, lr, beta1,
                     beta2, eps, weight_decay, (float)(lr / bc1), (float)sqrt(bc2), nullptr);
  return check_launch("adam_step");
}

// The same step gated on the device (no host round trip): the caller has written
// gate->ok_loss before the backward and counted the arena's non-finite elements into
// gate->nonfinite after it (mauv_nonfinite_count); the step count lives in gate->step.
MAUV_API int mauv_adam_step_gated(const MauvAdamEntry* table, int n, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, MauvStepGate* gate,
                                  hipStream_t stream) {
  if (n <= 0 || n > 65535 || !gate) { set_error("adam_step_gated: bad table size / gate"); return kErrArg; }
  hipLaunchKernelGGL(step_gate_kernel, dim3(1), dim3(1), 0, stream, gate, nullptr, nullptr,
                     nullptr, lr, beta1, beta2);
  hipLaunchKernelGGL(adam_kernel<true>, dim3(64, n), dim3(256), 0, stream, table, lr, beta1,
                     beta2, eps, weight_decay, 0.f, 1.f, (const MauvStepGate*)gate);
  return check_launch("adam_step_gated");
}

// The table and group checks of every all-groups entry, `name` being the entry's own.
static bool ex_args_ok(const char* name, const MauvAdamEntryEx* table, int n,
                       const MauvAdamGroup* groups, int n_groups) {
  if (n <= 0 || n > 65535 || !table) {
    set_error(std::string(name) + ": bad table size");
    return false;
  }
  if (n_groups < 1 || n_groups > MAUV_ADAM_MAX_GROUPS || !groups) {
    set_error(std::string(name) + ": 1..8 parameter groups");
    return false;
  }
  return true;
}

// The groups by value; step == 0: gated, the constants come from the gate.
static void fill_groups(AdamGroupsArg& ga, const MauvAdamGroup* groups, int n_groups,
                        long long step) {
  for (int i = 0; i < n_groups; ++i) {
    ga.g[i] = groups[i];
    ga.step_size[i] = 0.f;
    ga.bc2_sqrt[i] = 1.f;
    if (step) {
      const double bc1 = 1.0 - pow((double)groups[i].beta1, (double)step);
      const double bc2 = 1.0 - pow((double)groups[i].beta2, (double)step);
      ga.step_size[i] = (float)(groups[i].lr / bc1);
      ga.bc2_sqrt[i] = (float)sqrt(bc2);
    }
  }
}

// Every gated all-groups entry: the decision (scaler, acc and ema may each be NULL), then the
// Adam launch reading 1 / scale, 1 / micro and the clip coefficient, and moving the rows' shadows
// when both ema and ema_rows are given.
static int launch_gated_ex(const char* name, const MauvAdamEntryEx* table, int n,
                           const MauvAdamGroup* groups, int n_groups, MauvStepGate* gate,
                           MauvLossScale* scaler, MauvAccum* acc, float* const* ema_rows,
                           MauvEma* ema, hipStream_t stream) {
  if (!ex_args_ok(name, table, n, groups, n_groups)) return kErrArg;
  if (!gate) { set_error(std::string(name) + ": no gate"); return kErrArg; }
  if (!ema || !ema_rows) ema = nullptr, ema_rows = nullptr;
  AdamGroupsArg ga = {};
  fill_groups(ga, groups, n_groups, 0);
  hipLaunchKernelGGL(step_gate_kernel, dim3(1), dim3(1), 0, stream, gate, scaler, acc, ema,
                     groups[0].lr, groups[0].beta1, groups[0].beta2);
  auto kernel = ema ? adam_ex_kernel<true, true> : adam_ex_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3(64, n), dim3(256), 0, stream, table, ga, n_groups,
                     (const MauvStepGate*)gate, (const MauvLossScale*)scaler,
                     (const MauvAccum*)acc, ema_rows, (const MauvEma*)ema);
  return check_launch(name);
}

// Every Adam option and up to MAUV_ADAM_MAX_GROUPS parameter groups in one launch (mauv.h).
// gate == NULL: the ungated step at `step`; otherwise the gate's decision runs first, as in
// mauv_adam_step_gated, and every group steps at the gate's count.
MAUV_API int mauv_adam_step_ex(const MauvAdamEntryEx* table, int n, const MauvAdamGroup* groups,
                               int n_groups, long long step, MauvStepGate* gate,
                               hipStream_t stream) {
  if (gate)
    return launch_gated_ex("adam_step_ex", table, n, groups, n_groups, gate, nullptr, nullptr,
                           nullptr, nullptr, stream);
  if (!ex_args_ok("adam_step_ex", table, n, groups, n_groups)) return kErrArg;
  if (step < 1) { set_error("adam_step_ex: ungated step < 1"); return kErrArg; }
  AdamGroupsArg ga = {};
  fill_groups(ga, groups, n_groups, step);
  hipLaunchKernelGGL((adam_ex_kernel<false, false>), dim3(64, n), dim3(256), 0, stream, table, ga,
                     n_groups, nullptr, nullptr, nullptr, nullptr, nullptr);
  return check_launch("adam_step_ex");
}

// The gated mauv_adam_step_ex with a loss scaler (mauv.h).  scaler == NULL is exactly
// mauv_adam_step_ex(table, n, groups, n_groups, 0, gate, stream).
MAUV_API int mauv_adam_step_ex_scaled(const MauvAdamEntryEx* table, int n,
                                      const MauvAdamGroup* groups, int n_groups,
                                      MauvStepGate* gate, MauvLossScale* scaler,
                                      hipStream_t stream) {
  return launch_gated_ex("adam_step_ex_scaled", table, n, groups, n_groups, gate, scaler, nullptr,
                         nullptr, nullptr, stream);
}

// A micro-batch inside an accumulation window (mauv.h): one single-thread launch, no scan and
// no Adam launch.
MAUV_API int mauv_accum_note(MauvStepGate* gate, MauvAccum* acc, hipStream_t stream) {
  if (!gate || !acc) { set_error("accum_note: no gate / window state"); return kErrArg; }
  hipLaunchKernelGGL(accum_note_kernel, dim3(1), dim3(1), 0, stream, gate, acc);
  return check_launch("accum_note");
}

// The closing micro-batch of an accumulation window (mauv.h).  acc == NULL is exactly
// mauv_adam_step_ex_scaled(table, n, groups, n_groups, gate, scaler, stream).
MAUV_API int mauv_adam_step_ex_accum(const MauvAdamEntryEx* table, int n,
                                     const MauvAdamGroup* groups, int n_groups,
                                     MauvStepGate* gate, MauvLossScale* scaler, MauvAccum* acc,
                                     hipStream_t stream) {
  return launch_gated_ex("adam_step_ex_accum", table, n, groups, n_groups, gate, scaler, acc,
                         nullptr, nullptr, stream);
}

// The gated step with a weight EMA (mauv.h); scaler and acc may each be NULL.  ema == NULL or
// ema_rows == NULL is exactly mauv_adam_step_ex_accum(table, n, groups, n_groups, gate, scaler,
// acc, stream).
MAUV_API int mauv_adam_step_ex_ema(const MauvAdamEntryEx* table, int n,
                                   const MauvAdamGroup* groups, int n_groups, MauvStepGate* gate,
                                   MauvLossScale* scaler, MauvAccum* acc, float* const* ema_rows,
                                   MauvEma* ema, hipStream_t stream) {
  return launch_gated_ex("adam_step_ex_ema", table, n, groups, n_groups, gate, scaler, acc,
                         ema_rows, ema, stream);
}

// The average's element update at a host-given weight over a device table of (shadow, parameter,
// numel) rows (mauv.h): for steps the host decided.  w == 1 copies.
MAUV_API int mauv_ema_update(const MauvEmaRow* rows, int n, float w, hipStream_t stream) {
  if (n <= 0 || n > 65535 || !rows) { set_error("ema_update: bad table size"); return kErrArg; }
  if (!(w > 0.f && w <= 1.f)) { set_error("ema_update: weight outside (0, 1]"); return kErrArg; }
  hipLaunchKernelGGL(ema_rows_kernel<false>, dim3(64, n), dim3(256), 0, stream, rows, w);
  return check_launch("ema_update");
}

// Parameters and shadows exchanged element-wise, in place (mauv.h): no pointer changes.
MAUV_API int mauv_ema_swap(const MauvEmaRow* rows, int n, hipStream_t stream) {
  if (n <= 0 || n > 65535 || !rows) { set_error("ema_swap: bad table size"); return kErrArg; }
  hipLaunchKernelGGL(ema_rows_kernel<true>, dim3(64, n), dim3(256), 0, stream, rows, 1.0f);
  return check_launch("ema_swap");
}
