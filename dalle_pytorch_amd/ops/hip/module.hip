// Python module definition: every binding of the extension, nothing else.
// No device code, so the device pass sees an empty file and skips the torch
// headers (they cost more to parse than any kernel unit costs to compile).

#ifndef __HIP_DEVICE_COMPILE__

#include <torch/extension.h>

#include "hip_host.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("resls_fwd", &resls_fwd, "fused residual + per-channel scale fwd");
  m.def("resls_bwd", &resls_bwd, "fused residual + per-channel scale bwd");
  m.def("quant_fp8", &quant_fp8, "bf16 -> e4m3 one-pass quantize");
  m.def("sample_topk_gumbel", &sample_topk_gumbel,
        py::arg("logits"), py::arg("noise"), py::arg("k"),
        py::arg("temperature"), py::arg("out_tok") = std::nullopt,
        py::arg("seq") = std::nullopt, py::arg("seq_ptr") = std::nullopt,
        "fused top-k threshold + gumbel argmax sampling");
  m.def("amax_bf16", &amax_bf16, "abs-max of a bf16 tensor (one pass)");
  m.def("sk2", &sk2,
        py::arg("x"), py::arg("wp"), py::arg("bias"), py::arg("N"),
        py::arg("K"), py::arg("mode"), py::arg("wscale") = 1.0,
        "decode skinny GEMM on packed bf16/e4m3 weights "
        "(fused bias/geglu/fp32 head)");
  m.def("dec_prelude", &dec_prelude,
        "fused decode residual + LayerNorm + token-shift");
  m.def("permlane_probe", &permlane_probe,
        "v_permlane32_swap_b32 semantics probe");
  m.def("fa_fwd", &fa_fwd, "flash attention forward (gfx950, d=64)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("causal"), py::arg("key_mask"), py::arg("static_mask"),
        py::arg("tile_map"), py::arg("out_bnhd"),
        py::arg("ax_t") = 0, py::arg("ax_S") = 0, py::arg("ax_axis") = -1);
  m.def("fa_bwd", &fa_bwd, "flash attention backward (gfx950, d=64)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"),
        py::arg("lse"), py::arg("dout"), py::arg("scale"), py::arg("causal"),
        py::arg("key_mask"), py::arg("static_mask"), py::arg("tile_map"),
        py::arg("tile_map_t"), py::arg("out_bnhd"),
        py::arg("grad_lse") = std::nullopt,
        py::arg("ax_t") = 0, py::arg("ax_S") = 0, py::arg("ax_axis") = -1);
  m.def("rope_split_fwd", &rope_split_fwd,
        "fused qkv split + rotary (q,k,v all rotated)");
  m.def("rope_split_bwd", &rope_split_bwd, "rope_split backward");
  m.def("token_shift", &token_shift, "fused token shift (fwd/transpose)");
  m.def("fa_decode", &fa_decode, "fused single-token decode attention");
  m.def("shift_decode", &shift_decode, "fused single-token token shift");
  m.def("ln_fwd", &ln_fwd, "fused LayerNorm forward (bf16 rows)");
  m.def("ln_bwd", &ln_bwd, "fused LayerNorm backward");
  m.def("geglu_fwd", &geglu_fwd, "fused GEGLU forward");
  m.def("geglu_bwd", &geglu_bwd, "fused GEGLU backward");
  m.def("geglu_bwd_colsum", &geglu_bwd_colsum,
        "fused GEGLU backward + fp32 column sums of dx");
  m.def("ln_shift_fwd", &ln_shift_fwd, "LayerNorm + token shift forward");
  m.def("ln_shift_bwd", &ln_shift_bwd,
        "LayerNorm backward with shifted dy and/or residual gradient",
        py::arg("x"), py::arg("dy"), py::arg("w"), py::arg("mean"),
        py::arg("rstd"), py::arg("dres") = py::none(),
        py::arg("text_len") = 0, py::arg("image_size") = 0);
  m.def("rev_replay", &rev_replay,
        "reversible replay tail: x_rec, d_o, dgamma in one pass");
  m.def("mfma_probe", &mfma_probe, "MFMA 16x16x32 bf16 layout probe");
}

#endif  // !__HIP_DEVICE_COMPILE__
