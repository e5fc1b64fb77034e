// Per-element arithmetic of the optimiser step, shared by the per-tensor kernels (ofx_misc.hip: adamw_kernel,
// ema_kernel) and the multi-tensor kernel (ofx_train.hip) so that both give the same bits.
//
// Every operation here is rounded on its own: contraction is switched off for these bodies and the one fused
// multiply-add of the update is written out.  Left to the compiler, which products of `a * b + c * d` become an FMA
// depends on the code around the expression (hipcc's default is -ffp-contract=fast, and the SLP vectoriser packs
// multiplies before FMAs are formed), so two kernels inlining the same source line could round differently.  The
// operations below are the ones hipcc chose for the per-tensor kernels before the helpers existed.
#pragma once
#include <hip/hip_runtime.h>

// Wave-uniform factors of one AdamW step (torch.optim.AdamW: decoupled weight decay, bias-corrected moments).
struct OfxAdamW {
  float b1, b2, one_m_b1, one_m_b2, eps;
  float decay;         // 1 - lr * wd, one FMA
  float step_size;     // lr / bc1
  float sqrt_bc2;
};

// Computed on the device, per thread, as the per-tensor kernel always did (division and square root are the correctly
// rounded ones there).
__device__ __forceinline__ OfxAdamW ofx_adamw_setup(float lr, float b1, float b2, float eps, float wd, float bc1,
                                                    float bc2) {
#pragma clang fp contract(off)
  OfxAdamW a;
  a.b1 = b1;
  a.b2 = b2;
  a.one_m_b1 = 1.f - b1;
  a.one_m_b2 = 1.f - b2;
  a.eps = eps;
  a.decay = __builtin_fmaf(-lr, wd, 1.f);
  a.step_size = lr / bc1;
  a.sqrt_bc2 = sqrtf(bc2);
  return a;
}

// One element: returns the new parameter, updates the moments in place.
__device__ __forceinline__ float ofx_adamw_elem(const OfxAdamW& a, float p, float g, float& m, float& v) {
#pragma clang fp contract(off)
  float pi = p * a.decay;
  const float mi = a.b1 * m + a.one_m_b1 * g;
  const float vi = a.b2 * v + a.one_m_b2 * g * g;
  m = mi;
  v = vi;
  const float denom = sqrtf(vi) / a.sqrt_bc2 + a.eps;
  pi -= a.step_size * (mi / denom);
  return pi;
}

// ldm_diffusion_util.py:38-54: old * beta + (1 - beta) * new.
__device__ __forceinline__ float ofx_ema_elem(float e, float p, float beta) {
#pragma clang fp contract(off)
  return e * beta + (1.f - beta) * p;
}
