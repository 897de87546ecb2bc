// dalle_pytorch_amd gfx950 (CDNA4) kernel library: shared device helpers.
//
// First-party HIP kernels for the hot ops of the DALL-E stack
// (decode), one translation unit per family:
//   attention.hip  flash attention forward + backward (dQ, dKdV, Dv) with
//                  online softmax and tile-skipping sparsity (MFMA bf16
//                  16x16x32, LDS-tiled K/V with transposed-V store and
//                  swizzled rows for bank-conflict-free ds_read_b128)
//   train_ops.hip  fused rope+QKV split, GEGLU, token-shift, LayerNorm,
//                  residual scale, reversible replay, fp8 quantize
//   decode.hip     the single-token decode family (key-split attention +
//                  ring-buffer shift, the sk2 decode GEMM, sampler)
//   wgrad.hip      split-K weight gradient: chunk GEMMs through ATen + the
//                  fixed-order fp32 reduce of the partials (a dispatcher op)
//   module.hip     the Python module definition
// Written for wave64 / 8-XCD MI355X per the CDNA4 HIP guide — NOT a port of
// any CUDA kernel.
//
// bf16 values are carried as raw `short` bit patterns end to end; float
// math goes through explicit bit casts (bf2f/f2bf) so no accidental
// numeric conversion happens on the storage path.
//
// Numerics contract (matches the eager oracle in ops/attention.py):
//   S = scale * (Q K^T); masked entries -> -inf; P = softmax(S) with online
//   max subtraction (identical to the reference's stable_softmax,
//   attention.py:27-30); O = P V; lse = rowmax + log(rowsum).

#pragma once

#include <hip/hip_runtime.h>

#define DEVFN __device__ __forceinline__

using bf16x8 = __attribute__((ext_vector_type(8))) short;   // MFMA A/B frag
using bf16x4 = __attribute__((ext_vector_type(4))) short;    // packed P stores
using f32x4 = __attribute__((ext_vector_type(4))) float;    // MFMA C/D frag
using int4v = __attribute__((ext_vector_type(4))) int;      // 16B copies

constexpr float NEG_INF = -INFINITY;

constexpr int FA_D = 64;        // head dim (attention, rope split)

DEVFN float bf2f(short u) {
  union { unsigned int i; float f; } c;
  c.i = (unsigned int)(unsigned short)u << 16;
  return c.f;
}
DEVFN short f2bf(float f) {
  union { unsigned int i; float f; } c;
  c.f = f;
  unsigned int r = c.i + 0x7fff + ((c.i >> 16) & 1);  // round-nearest-even
  return (short)(r >> 16);
}

// raw v_exp_f32 (base-2): libm exp2f lowers to a guarded cmp/cndmask/
// v_exp/v_ldexp sequence (ISA-checked) that costs MORE than __expf's
// mul+exp; the amdgcn builtin is the single instruction. Softmax args are
// <= 0 and > -20000, far from the guard range.
DEVFN float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// exact erf gelu (transformer.py:106-109): the GEGLU kernels and the decode
// GEMM's fused GEGLU epilogue
DEVFN float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678f)); }
DEVFN float gelu_grad_f(float x) {
  const float cdf = 0.5f * (1.f + erff(x * 0.70710678f));
  const float pdf = 0.3989422804f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}

// Training token shift as a gather (the token_shift kernel and the
// LayerNorm shift variants): where channel offset `off` of position `pos`
// comes from, or that it is zero-filled. backward=1 is the transpose.
DEVFN void token_shift_src(int pos, int off, int n, int text_len, int S,
                           int half, int quarter, int backward,
                           int* srcpos, bool* zero) {
  *srcpos = pos;
  *zero = false;
  if (!backward) {
    if (pos < text_len) {
      if (off < half) { *srcpos = pos - 1; *zero = pos == 0; }
    } else {
      const int g = pos - text_len;
      const int gr = g / S, gc = g - gr * S;
      if (off < quarter) { *srcpos = pos - S; *zero = gr == 0; }
      else if (off < half) { *srcpos = pos - 1; *zero = gc == 0; }
    }
  } else {
    if (pos < text_len) {
      if (off < half) { *srcpos = pos + 1; *zero = pos + 1 >= text_len; }
    } else {
      const int g = pos - text_len;
      const int gr = g / S, gc = g - gr * S;
      if (off < quarter) { *srcpos = pos + S; *zero = gr + 1 >= S || pos + S >= n; }
      else if (off < half) { *srcpos = pos + 1; *zero = gc + 1 >= S || pos + 1 >= n; }
    }
  }
}
