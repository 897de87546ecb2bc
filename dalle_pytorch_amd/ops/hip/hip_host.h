// Host-side helpers shared by the kernel units, and the wrappers that
// module.hip binds.

#pragma once

#include <torch/types.h>
#include <ATen/hip/HIPContext.h>

#include "hip_common.h"

#define CHK(x) TORCH_CHECK(x, #x)

inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

// bf16 tensors travel as raw 16-bit patterns (see hip_common.h)
inline short* bf16_ptr(const torch::Tensor& t) {
  return reinterpret_cast<short*>(t.data_ptr());
}
inline const short* bf16_cptr(const torch::Tensor& t) {
  return reinterpret_cast<const short*>(t.data_ptr());
}

// optional rotary tables ([positions, rot] fp32 each) -> raw pointers; all
// null / rot = 0 when rotary is off
struct RopeTables {
  const float* cos = nullptr;
  const float* sin = nullptr;
  int rot = 0;
};
inline RopeTables rope_tables(const std::optional<torch::Tensor>& cosv,
                              const std::optional<torch::Tensor>& sinv) {
  RopeTables t;
  if (cosv.has_value()) {
    t.rot = cosv->size(1);
    t.cos = cosv->data_ptr<float>();
    t.sin = sinv->data_ptr<float>();
  }
  return t;
}

using TensorList = std::vector<torch::Tensor>;
using OptTensor = std::optional<torch::Tensor>;

// attention.hip
TensorList fa_fwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                  double scale, bool causal, OptTensor key_mask,
                  OptTensor static_mask, OptTensor tile_map, bool out_bnhd,
                  int64_t ax_t, int64_t ax_S, int64_t ax_axis);
TensorList fa_bwd(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                  torch::Tensor out, torch::Tensor lse, torch::Tensor dout,
                  double scale, bool causal, OptTensor key_mask,
                  OptTensor static_mask, OptTensor tile_map,
                  OptTensor tile_map_t, bool out_bnhd, OptTensor grad_lse,
                  int64_t ax_t, int64_t ax_S, int64_t ax_axis);
TensorList permlane_probe(torch::Tensor a, torch::Tensor b_);
torch::Tensor mfma_probe(torch::Tensor A, torch::Tensor B);

// train_ops.hip
TensorList rope_split_fwd(torch::Tensor qkv, int64_t heads, OptTensor cosv,
                          OptTensor sinv);
torch::Tensor rope_split_bwd(torch::Tensor dq, torch::Tensor dk,
                             torch::Tensor dv, OptTensor cosv, OptTensor sinv);
torch::Tensor geglu_fwd(torch::Tensor x);
torch::Tensor geglu_bwd(torch::Tensor x, torch::Tensor dout);
TensorList geglu_bwd_colsum(torch::Tensor x, torch::Tensor dout);
torch::Tensor token_shift(torch::Tensor x, int64_t text_len,
                          int64_t image_size, bool backward);
TensorList ln_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                  double eps);
TensorList ln_bwd(torch::Tensor x, torch::Tensor dy, torch::Tensor w,
                  torch::Tensor mean, torch::Tensor rstd);
TensorList ln_shift_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b,
                        double eps, int64_t text_len, int64_t image_size);
TensorList ln_shift_bwd(torch::Tensor x, torch::Tensor dy, torch::Tensor w,
                        torch::Tensor mean, torch::Tensor rstd, OptTensor dres,
                        int64_t text_len, int64_t image_size);
torch::Tensor amax_bf16(torch::Tensor x);
torch::Tensor quant_fp8(torch::Tensor x, torch::Tensor amax);
torch::Tensor resls_fwd(torch::Tensor x, torch::Tensor y, torch::Tensor gamma);
TensorList resls_bwd(torch::Tensor dout, torch::Tensor y, torch::Tensor gamma);
TensorList rev_replay(torch::Tensor o, torch::Tensor gamma, torch::Tensor y,
                      torch::Tensor d);

// decode.hip
torch::Tensor fa_decode(torch::Tensor qkv, torch::Tensor kc, torch::Tensor vc,
                        OptTensor cosv, OptTensor sinv, torch::Tensor offset,
                        OptTensor pattern, double scale, OptTensor live,
                        OptTensor live_cnt);
torch::Tensor shift_decode(torch::Tensor x, torch::Tensor offset,
                           torch::Tensor ring, int64_t text_len);
TensorList dec_prelude(torch::Tensor x, OptTensor y, OptTensor scale,
                       torch::Tensor w, torch::Tensor b, OptTensor ring,
                       torch::Tensor offset, double eps, int64_t S,
                       int64_t text_len);
torch::Tensor sample_topk_gumbel(torch::Tensor logits, torch::Tensor noise,
                                 int64_t k, double temperature,
                                 OptTensor out_tok, OptTensor seq,
                                 OptTensor seq_ptr);
torch::Tensor sk2(torch::Tensor x, torch::Tensor wp, OptTensor bias, long N,
                  long K, long mode, double wscale);
