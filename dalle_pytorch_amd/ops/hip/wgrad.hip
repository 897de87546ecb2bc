// Split-K weight gradient: dW[n, k] = do2[M, n]^T · x2[M, k] with the long
// row dimension M cut into S chunks. A weight gradient has a small output
// (32-128 macro-tiles at the flagship shapes, on 256 CUs) and a very long
// reduction, so one GEMM leaves most of the chip idle; S chunk GEMMs run as
// ONE strided-batched GEMM into a [S, n, k] workspace and fill it, and
// wgrad_reduce_kernel below sums the S partials into dW. The GEMM is ATen's
// (at::bmm_out on views, no operand copy); only the reduce is ours.
//
// Registered through the dispatcher (torch.ops.dalle_amd.*), not pybind:
// loading the shared object is enough.

#include <torch/library.h>

#include "hip_host.h"

// ---------------------------------------------------------------------------
// out[i] = sum_{s=0..S-1} part[s, i], accumulated in fp32 in that fixed order
// (no atomics: bitwise reproducible), one rounding at the store. Each thread
// owns 16-byte chunks (4 fp32 values) of a partial slab and issues all S
// loads of a chunk before the first add, so S independent 16-byte
// requests are in flight per lane (the compiler keeps them all in registers
// up to S = 8 and starts adding earlier at 16 and 32: 62 VGPRs, no scratch).
// Pure bandwidth: reads S slabs, writes one. Measured 4.4-5.9 TB/s where it
// moves 30 MB or more (profiles/probe_wgrad.txt; rev_replay runs at 5.6);
// below that the 5 us launch floor shows.
// ---------------------------------------------------------------------------

template <int S, bool OUT_BF16>
__global__ __launch_bounds__(256)
void wgrad_reduce_kernel(const f32x4* __restrict__ part,  // [S, nvec]
                         void* __restrict__ out,          // [nvec * 4]
                         long nvec) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec;
       i += (long)gridDim.x * 256) {
    f32x4 v[S];
    #pragma unroll
    for (int s = 0; s < S; ++s) v[s] = part[(long)s * nvec + i];
    f32x4 acc = v[0];
    #pragma unroll
    for (int s = 1; s < S; ++s) acc += v[s];
    if (OUT_BF16) {
      bf16x4 o;
      #pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = f2bf(acc[e]);
      reinterpret_cast<bf16x4*>(out)[i] = o;
    } else {
      reinterpret_cast<f32x4*>(out)[i] = acc;
    }
  }
}

constexpr int WGRAD_MAX_SPLITS = 32;

static bool wgrad_dtype_ok(at::ScalarType t) {
  return t == at::kFloat || t == at::kBFloat16;
}

template <int S>
static void launch_reduce(const torch::Tensor& part, torch::Tensor& out) {
  const long nvec = out.numel() / 4;
  const long nb = std::max<long>(std::min<long>((nvec + 255) / 256, 2048), 1);
  auto* p = reinterpret_cast<const f32x4*>(part.data_ptr<float>());
  if (out.scalar_type() == at::kBFloat16)
    hipLaunchKernelGGL((wgrad_reduce_kernel<S, true>), dim3(nb), dim3(256), 0,
                       cur_stream(), p, out.data_ptr(), nvec);
  else
    hipLaunchKernelGGL((wgrad_reduce_kernel<S, false>), dim3(nb), dim3(256),
                       0, cur_stream(), p, out.data_ptr(), nvec);
}

// part [S, n, k] fp32 -> [n, k] in out_dtype
torch::Tensor wgrad_reduce(const torch::Tensor& part,
                           at::ScalarType out_dtype) {
  TORCH_CHECK(part.is_cuda() && part.dim() == 3 && part.is_contiguous(),
              "wgrad_reduce: partials must be a contiguous [S, n, k] GPU "
              "tensor");
  TORCH_CHECK(part.scalar_type() == at::kFloat && wgrad_dtype_ok(out_dtype),
              "wgrad_reduce: partials must be float32, the output float32 or "
              "bfloat16");
  const long S = part.size(0), n = part.size(1), k = part.size(2);
  TORCH_CHECK(n * k > 0 && (n * k) % 4 == 0,
              "wgrad_reduce: n * k must be a positive multiple of 4, got ", n,
              " x ", k);
  auto out = at::empty({n, k}, part.options().dtype(out_dtype));
  switch (S) {
    case 1: launch_reduce<1>(part, out); break;
    case 2: launch_reduce<2>(part, out); break;
    case 4: launch_reduce<4>(part, out); break;
    case 8: launch_reduce<8>(part, out); break;
    case 16: launch_reduce<16>(part, out); break;
    case 32: launch_reduce<32>(part, out); break;
    default:
      TORCH_CHECK(false, "wgrad_reduce: S must be a power of two <= ",
                  WGRAD_MAX_SPLITS, ", got ", S);
  }
  return out;
}

// do2 [M, n] bf16, x2 [M, k] bf16 -> dW [n, k] = do2^T x2 in out_dtype, the
// M rows reduced as `splits` chunk GEMMs with fp32 partials + the fixed-
// order reduce. splits = 1 with fp32 output is the GEMM alone, written
// straight into dW.
torch::Tensor wgrad_splitk(const torch::Tensor& do2, const torch::Tensor& x2,
                           int64_t splits, at::ScalarType out_dtype) {
  TORCH_CHECK(do2.scalar_type() == at::kBFloat16 &&
                  x2.scalar_type() == at::kBFloat16,
              "wgrad_splitk: inputs must be bfloat16, got ",
              do2.scalar_type(), " and ", x2.scalar_type());
  TORCH_CHECK(do2.dim() == 2 && x2.dim() == 2,
              "wgrad_splitk: inputs must be 2-D [rows, n] and [rows, k]");
  TORCH_CHECK(do2.is_contiguous() && x2.is_contiguous(),
              "wgrad_splitk: inputs must be contiguous");
  TORCH_CHECK(do2.size(0) == x2.size(0),
              "wgrad_splitk: row counts differ: ", do2.size(0), " vs ",
              x2.size(0));
  TORCH_CHECK(wgrad_dtype_ok(out_dtype),
              "wgrad_splitk: out_dtype must be float32 or bfloat16");
  const long M = do2.size(0), n = do2.size(1), k = x2.size(1);
  const long S = splits;
  TORCH_CHECK(S >= 1 && S <= WGRAD_MAX_SPLITS && (S & (S - 1)) == 0,
              "wgrad_splitk: splits must be a power of two <= ",
              WGRAD_MAX_SPLITS, ", got ", S);
  TORCH_CHECK(M > 0 && M % S == 0, "wgrad_splitk: splits = ", S,
              " does not divide the ", M, " rows");
  TORCH_CHECK(n * k > 0 && (n * k) % 4 == 0,
              "wgrad_splitk: n * k must be a positive multiple of 4, got ", n,
              " x ", k);
  TORCH_CHECK(do2.is_cuda() && x2.is_cuda() &&
                  do2.device() == x2.device(),
              "wgrad_splitk: inputs must be GPU tensors on one device");
  // chunk s is rows [s*M/S, (s+1)*M/S): views only, the GEMM reads in place
  auto a = do2.view({S, M / S, n}).transpose(1, 2);
  auto b = x2.view({S, M / S, k});
  // caching allocator, current stream
  auto part = at::empty({S, n, k}, do2.options().dtype(at::kFloat));
  at::bmm_out(part, a, b, at::kFloat);
  if (S == 1 && out_dtype == at::kFloat) return part.view({n, k});
  return wgrad_reduce(part, out_dtype);
}

#ifndef __HIP_DEVICE_COMPILE__
TORCH_LIBRARY(dalle_amd, m) {
  m.def("wgrad_splitk(Tensor do2, Tensor x2, int splits, "
        "ScalarType out_dtype) -> Tensor", &wgrad_splitk);
  m.def("wgrad_reduce(Tensor part, ScalarType out_dtype) -> Tensor",
        &wgrad_reduce);
}
#endif
