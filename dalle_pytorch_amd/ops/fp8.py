"""fp8 (e4m3) forward path for the projection GEMMs.

gfx950 runs e4m3 MFMA at 2x the bf16 rate; measured on MI355X the raw
ff1-shaped GEMM goes 1297 -> 2134 TF/s (scripts/probe_fp8.py). Master
weights stay bf16/fp32 — fp8 exists only on the wire into the GEMM:

* activations: one torch amax reduce + the one-pass quant_fp8 HIP kernel
  (the eager cast chain costs more than the fp8 GEMM saves);
* weights: quantized once per optimizer step (cached on the parameter's
  version counter, so the reversible recompute pass reuses it);
* backward: bf16 dgrad/wgrad (transposed-weight dgrad, split-K wgrad on the
  long-reduction shapes) — fp8 is forward-only, which under reversible
  execution still covers 2 of the 4 GEMM passes per step.

Enable with DALLE_AMD_FP8=1 (or ``set_fp8_enabled(True)``; bench.py
exposes ``--fp8``). Default OFF: the headline BASELINE numbers are bf16.
"""

import weakref

import torch
import torch.nn.functional as F

from dalle_pytorch_amd.ops.dispatch import (env_flag, hip_module,
                                            using_eager_fallback)
from dalle_pytorch_amd.ops.fused import (fusion_enabled, geglu_bwd_colsum,
                                         geglu_colsum_tiles)

_FORCED = None
FP8_MAX = 448.0


def set_fp8_enabled(flag):
    global _FORCED
    _FORCED = bool(flag) if flag is not None else None


def fp8_enabled():
    if _FORCED is not None:
        return _FORCED
    return env_flag('FP8', False)


_generation = 0


def fp8_mark_step():
    """Invalidate the per-step weight caches. Call after optimizer steps —
    parameter version counters are not reliably bumped by every
    fused/foreach CUDA optimizer path."""
    global _generation
    _generation += 1


class _StepCache:
    """Per-step cache of one tensor derived from a weight by ``make(w)``:
    the reversible recompute re-runs every forward with unchanged weights,
    so derive once per (parameter, version, step).

    Keyed by storage + shape, so fresh VIEWS of the same slice (the
    split-vocab head re-slices its weight every step) hit too. Each entry
    also holds a weak reference to the tensor that owns the storage — the
    base parameter for a view, else ``w`` itself — so an entry left by a
    freed parameter is never served to a new one that the allocator placed
    at the same address with the same shape and version. Always key on the
    MASTER parameter (stable storage), never on cast temporaries. At most
    ``BOUND`` entries: a full cache empties itself."""

    BOUND = 512

    def __init__(self, make):
        self.make = make
        self.entries = {}

    def __call__(self, w):
        key = (w.data_ptr(), tuple(w.shape))
        stamp = (w._version, _generation)
        owner = w._base if w._base is not None else w
        hit = self.entries.get(key)
        if hit is not None and hit[0] == stamp and hit[2]() is owner:
            return hit[1]
        val = self.make(w)
        if len(self.entries) >= self.BOUND:
            self.entries.clear()
        self.entries[key] = (stamp, val, weakref.ref(owner))
        return val


def _bf16(w):
    w = w.detach()
    return w if w.dtype == torch.bfloat16 else w.to(torch.bfloat16)


def _quant(t, ext):
    t = t.detach().contiguous()
    scale = ext.amax_bf16(t)   # outputs amax/448 directly (one pass)
    return ext.quant_fp8(t, scale), scale.squeeze()


# (e4m3 weight, scale)
_quant_weight = _StepCache(lambda w: _quant(_bf16(w), hip_module()))
# bf16 copy of a master weight (what autocast's per-region weight cache
# would provide)
_bf16_weight = _StepCache(_bf16)
# contiguous bf16 W^T: hipBLASLt runs dgrad ~15% faster fed a transposed-
# view B operand (scripts/probe_dgrad.py: ff1-dgrad 1261 -> 1460 TF/s)
_transposed_weight = _StepCache(lambda w: _bf16(w).t().contiguous())


def _fp8_ok(x, weight):
    if not fp8_enabled() or using_eager_fallback(x):
        return False
    if x.dtype != torch.bfloat16:
        return False
    rows = x.numel() // x.shape[-1]
    k, n = weight.shape[1], weight.shape[0]
    if rows % 16 or k % 16 or n % 16 or rows < 256:
        return False
    if rows * k < (32 << 20):
        # quantization passes don't amortize on small inputs (configs B/D
        # measured net-negative: 421k -> 379k and 8.3k -> 7.4k)
        return False
    # profitability gate, measured per-shape on MI355X (probe_fp8b + end-to-
    # end A/B): ff1 (N=8192,K=1024) +375 us/call and qkv (N=3072) +123 win;
    # ff2 (K=4096) and the square out-proj are net NEUTRAL in isolation and
    # LOSE ~1%% end-to-end (launch-gap overhead of the extra quant kernels),
    # so only clearly-profitable shapes pass
    return n * 2 >= k * 3


def _fast_dgrad_ok(x, w):
    if using_eager_fallback(x) or x.dtype != torch.bfloat16:
        return False
    rows = x.numel() // x.shape[-1]
    return (rows >= 1024 and rows % 16 == 0 and w.shape[0] % 16 == 0
            and w.shape[1] % 16 == 0 and torch.is_grad_enabled())


def _gemm_forward(x, weight, bias):
    """x @ weight^T + bias in bf16 -> (x as [rows, k], output [rows, n]):
    the fp8 GEMM where ``_fp8_ok``, else F.linear on the cached bf16 weight.
    ``weight`` is the MASTER parameter, ``bias`` None or already bf16."""
    x2 = x.reshape(-1, x.shape[-1])
    if _fp8_ok(x, weight):
        xq, xs = _quant(x2, hip_module())
        wq, ws = _quant_weight(weight)
        out = torch._scaled_mm(xq, wq.t(), scale_a=xs, scale_b=ws,
                               bias=bias, out_dtype=torch.bfloat16)
    else:
        wb = weight if weight.dtype == torch.bfloat16 else _bf16_weight(weight)
        out = F.linear(x, wb, bias).reshape(-1, weight.shape[0])
    return x2, out


# Split-K weight gradient (ops/hip/wgrad.hip). dW = do2^T x2 has a small
# output and a very long reduction: the flagship shapes give 16-128 macro-
# tiles of 256 x 256 on 256 CUs, so a single GEMM leaves half the chip idle.
# Constants from profiles/probe_wgrad.txt (scripts/probe_wgrad.py; 81920 rows
# unless stated, fp32 output, "today" = bf16 GEMM + the cast to fp32):
#   dW              today    best S        rule
#   8192 x 1024    1252 us    2: 1204 us     2   ff1 (2-4% in every run)
#   1024 x 4096     702 us    4:  627 us     4   ff2
#   3072 x 1024     686 us    4:  474 us     4   qkv (S = 8: 493 us)
#   1024 x 1024     419 us   16:  182 us    16   out-proj (S = 32: 195 us)
#   10256 x 1024    525 us    2:  376 us     2   text CE head, 16448 rows
#                                                (S = 4, 4112-row chunks: 462)
# i.e. split until S x tiles reaches 192; a target of 256 would pick S = 8
# for qkv. The fp32-output GEMM alone (S = 1) ties with today's GEMM + cast,
# so a shape that is not split keeps today's expression.
WGRAD_TILE = 256          # macro-tile edge the tile count is taken in
WGRAD_TILE_TARGET = 192   # split until S x tiles reaches this many
# rows: nothing under 16448 rows was probed (config B runs 10240); chunks of
# 5120 rows still gained over the next-lower S, chunks of 4112 rows lost
WGRAD_ROW_FLOOR = 16384   # fewer rows than this: never split
WGRAD_CHUNK_FLOOR = 5120  # rows per chunk, at least
WGRAD_MAX_SPLITS = 32     # the reduce kernel's widest instantiation


def wgrad_splits(rows, n, k):
    """How many row chunks the weight gradient dW[n, k] of ``rows`` rows is
    split into: the smallest power of two S for which S x (macro-tiles of dW)
    fills the chip, among those that divide ``rows`` and leave chunks of at
    least WGRAD_CHUNK_FLOOR rows. 1 (no split) below WGRAD_ROW_FLOOR rows and
    where n or k is no multiple of 16. Shapes only: a pure function."""
    if rows < WGRAD_ROW_FLOOR or n <= 0 or k <= 0 or n % 16 or k % 16:
        return 1
    tiles = -(-n // WGRAD_TILE) * -(-k // WGRAD_TILE)
    s = 1
    while (s * tiles < WGRAD_TILE_TARGET and s < WGRAD_MAX_SPLITS
           and rows % (2 * s) == 0 and rows // (2 * s) >= WGRAD_CHUNK_FLOOR):
        s *= 2
    return s


def wgrad_plan(do2, x2, out_dtype):
    """Splits for torch.ops.dalle_amd.wgrad_splitk on these operands, or 0
    for the plain ``do2.t() @ x2``: off the kernel path (CPU, eager
    fallback, non-bf16 or non-contiguous operands, a weight dtype the reduce
    does not store), with DALLE_AMD_WGRAD_SPLITK=0, and where the rule does
    not split."""
    # the shape rule first: small layers leave here at the cost of a compare
    s = wgrad_splits(do2.shape[0], do2.shape[-1], x2.shape[-1])
    if s <= 1:
        return 0
    if not fusion_enabled('WGRAD_SPLITK') or using_eager_fallback(do2):
        return 0
    if not (do2.dtype == x2.dtype == torch.bfloat16 and do2.dim() == 2
            and x2.dim() == 2 and do2.is_contiguous() and x2.is_contiguous()
            and out_dtype in (torch.float32, torch.bfloat16)):
        return 0
    return s


def _wgrad_op(do2, x2, splits, out_dtype):
    # registered by the extension's shared object (dispatcher op, not a
    # pybind export); wgrad_plan has loaded it
    return torch.ops.dalle_amd.wgrad_splitk(do2, x2, splits, out_dtype)


def _gemm_backward(do2, x2, weight, lead):
    """(dx [*lead, k], dW) from the output gradient do2 [rows, n]:
    transposed-weight dgrad; split-K wgrad, stored once in the weight's
    dtype, where ``wgrad_plan`` splits, else the standard wgrad."""
    wt = _transposed_weight(weight)
    dx = (do2 @ wt.t()).reshape(*lead, weight.shape[1])
    x2 = x2.to(do2.dtype)
    splits = wgrad_plan(do2, x2, weight.dtype)
    if splits:
        dw = _wgrad_op(do2, x2, splits, weight.dtype)
    else:
        dw = (do2.t() @ x2).to(weight.dtype)
    return dx, dw


def _bf16_bias(bias):
    if bias is None or bias.dtype == torch.bfloat16:
        return bias
    return bias.to(torch.bfloat16)


class _LinearFn(torch.autograd.Function):
    """bf16 linear (fp8 forward GEMM where profitable) with the
    transposed-dgrad backward. Receives MASTER weights (any float dtype)
    and casts inside, so the per-step caches key on stable parameter
    storage."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x2, out = _gemm_forward(x, weight, _bf16_bias(bias))
        ctx.save_for_backward(x2, weight)
        ctx.has_bias = bias is not None
        return out.reshape(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dout):
        x2, weight = ctx.saved_tensors
        do2 = dout.reshape(-1, dout.shape[-1]).contiguous()
        dx, dw = _gemm_backward(do2, x2, weight, dout.shape[:-1])
        return dx, dw, do2.sum(0) if ctx.has_bias else None


def fp8_linear_raw(x, weight, bias, module=None):
    """F.linear(x, weight, bias) through the fp8 forward path when
    profitable, else in bf16 with the transposed-dgrad backward (raw-tensor
    form for weight slices, e.g. the split-vocab CE head); else plain
    F.linear — or ``module(x)`` when the tensors are a module's own."""
    if (_fp8_ok(x, weight) or _fast_dgrad_ok(x, weight)) \
            and weight.is_contiguous():
        return _LinearFn.apply(x.contiguous(), weight, bias)
    return F.linear(x, weight, bias) if module is None else module(x)


def fp8_linear(linear_module, x):
    """Drop-in for ``linear_module(x)`` on the fp8_linear_raw ladder; its
    last resort is the module itself, so module hooks still fire."""
    return fp8_linear_raw(x, linear_module.weight, linear_module.bias,
                          linear_module)


class _LinearGegluFn(torch.autograd.Function):
    """geglu(linear(x)) as one autograd node, so the backward can take the
    linear's bias gradient from geglu_bwd's column partials instead of a
    separate reduce over the [rows, 2H] gradient it has just written. The
    GEMMs and weight caches are _LinearFn's."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x2, h = _gemm_forward(x, weight, _bf16_bias(bias))
        out = hip_module().geglu_fwd(h)
        ctx.save_for_backward(x2, weight, h)
        ctx.bias_dtype = bias.dtype
        return out.reshape(*x.shape[:-1], weight.shape[0] // 2)

    @staticmethod
    def backward(ctx, dout):
        x2, weight, h = ctx.saved_tensors
        do2 = dout.reshape(-1, dout.shape[-1]).contiguous()
        dh, db = geglu_bwd_colsum(h, do2)
        dx, dw = _gemm_backward(dh, x2, weight, dout.shape[:-1])
        return dx, dw, db.to(ctx.bias_dtype)


def linear_geglu_ok(linear_module, x):
    """The fused linear -> GEGLU node applies where the linear would take
    one of the custom-backward paths anyway and the GEGLU kernels apply."""
    w = linear_module.weight
    return (fusion_enabled('FF1_BIAS') and linear_module.bias is not None
            and (_fp8_ok(x, w) or _fast_dgrad_ok(x, w))
            and geglu_colsum_tiles(w.shape[0]))


def linear_geglu(linear_module, x):
    """geglu(linear_module(x)); callers check linear_geglu_ok first."""
    return _LinearGegluFn.apply(x.contiguous(), linear_module.weight,
                                linear_module.bias)
