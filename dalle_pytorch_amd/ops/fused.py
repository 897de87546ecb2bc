"""Fused elementwise ops (memory-bound; reference kernel rows K6/K7).

On gfx950 these are single HBM-bound passes (vectorized bf16x8 loads per the
CDNA4 guide); on CPU the eager equivalents run.
"""

import torch
import torch.nn.functional as F

from dalle_pytorch_amd.ops.dispatch import (env_flag, hip_module,
                                            using_eager_fallback)


class _GegluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ext = hip_module()
        x = x.contiguous()
        out = ext.geglu_fwd(x)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, dout):
        ext = hip_module()
        (x,) = ctx.saved_tensors
        return ext.geglu_bwd(x, dout.contiguous())


def geglu(x: torch.Tensor) -> torch.Tensor:
    """GEGLU gate: split the last dim in half, return value * gelu(gate).

    Matches reference transformer.py:106-109 (erf-based exact gelu).
    """
    if using_eager_fallback(x) or x.shape[-1] % 16:
        a, b = x.chunk(2, dim=-1)
        return a * F.gelu(b)
    return _GegluFn.apply(x)


class _TokenShiftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, text_len, image_size):
        ext = hip_module()
        ctx.text_len, ctx.image_size = text_len, image_size
        return ext.token_shift(x.contiguous(), text_len, image_size, False)

    @staticmethod
    def backward(ctx, dout):
        ext = hip_module()
        dx = ext.token_shift(dout.contiguous(), ctx.text_len, ctx.image_size, True)
        return dx, None, None


def token_shift(x, text_len, image_size):
    """Fused training-path token shift (reference transformer.py:165-186):
    text halves shift one token; image quarters shift from the grid row
    above / left neighbor. One gather kernel each way."""
    return _TokenShiftFn.apply(x, text_len, image_size)


def token_shift_supported(x):
    return (not using_eager_fallback(x)
            and x.shape[-1] * x.element_size() % 64 == 0)


def token_shift_eager(x, text_len, image_size):
    """Eager training-shape token shift, whole sequence at once (same
    contract as token_shift)."""
    b, n, c = x.shape
    t, S, q = text_len, image_size, c // 4
    prev = x[:, :t - 1, :c // 2]
    text = torch.cat((
        torch.cat((x.new_zeros(b, 1, c // 2), prev), dim=1),
        x[:, :t, c // 2:]), dim=-1)
    img = x[:, t:]
    ni = img.shape[1]
    if ni == 0:
        return text
    g = F.pad(img, (0, 0, 0, S * S - ni)).view(b, S, S, c)
    top = torch.cat((g.new_zeros(b, 1, S, q), g[:, :-1, :, :q]), dim=1)
    left = torch.cat((g.new_zeros(b, S, 1, q), g[:, :, :-1, q:2 * q]), dim=2)
    img = torch.cat((top, left, g[..., 2 * q:]), dim=-1)
    return torch.cat((text, img.view(b, S * S, c)[:, :ni]), dim=1)


def _rows_of_8(*tensors):
    """The resls_* / rev_replay kernels' rule: bf16 rows on the kernel path,
    8 channels per thread, and the dim/8 threads of a row tile a 256-thread
    block."""
    x = tensors[0]
    c8, rest = divmod(x.shape[-1], 8)
    return (x.is_cuda and all(t.dtype == torch.bfloat16 for t in tensors)
            and not using_eager_fallback(x) and rest == 0
            and 0 < c8 <= 256 and 256 % c8 == 0)


class _AddScaledFn(torch.autograd.Function):
    """out = x + gamma * y with per-channel gamma — the residual + LayerScale
    fusion (reference transformer.py:74-88 + reversible.py:138-140 adds).
    Backward: dx aliases dout (no kernel), dy/dgamma in one fused pass."""

    @staticmethod
    def forward(ctx, x, y, gamma):
        ext = hip_module()
        y = y.contiguous()
        gf = gamma.detach().reshape(-1).float().contiguous()
        out = ext.resls_fwd(x.contiguous(), y, gf)
        ctx.save_for_backward(y, gf)
        ctx.gamma_meta = (gamma.shape, gamma.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        ext = hip_module()
        y, gf = ctx.saved_tensors
        dout = dout.contiguous()
        dy, dgamma = ext.resls_bwd(dout, y, gf)
        shape, dtype = ctx.gamma_meta
        return dout, dy, dgamma.reshape(shape).to(dtype)


def add_scaled(x, y, gamma):
    """x + gamma * y (gamma broadcast over the last dim)."""
    if _rows_of_8(x, y):
        return _AddScaledFn.apply(x, y, gamma)
    return x + y * gamma.to(y.dtype)


def fusion_enabled(name):
    """Off switches for the fused training-tail paths, for A/B runs and
    tests: DALLE_AMD_LN_SHIFT, DALLE_AMD_REV_REPLAY, DALLE_AMD_FF1_BIAS,
    and DALLE_AMD_WGRAD_SPLITK for the split-K weight gradient (each
    default '1'; '0' restores the earlier path)."""
    return env_flag(name, True)


class _LayerNormFn(torch.autograd.Function):
    """``dres`` (optional, no gradient) is a residual-stream gradient that
    the backward folds into dx: dx = dres + (LN gradient), one pass."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, dres=None):
        ext = hip_module()
        x = x.contiguous()
        y, mean, rstd = ext.ln_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.dres = dres
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = hip_module()
        x, weight, mean, rstd = ctx.saved_tensors
        dres, ctx.dres = ctx.dres, None
        if dres is None:
            dx, dgamma, dbeta = ext.ln_bwd(x, dy.contiguous(), weight, mean,
                                           rstd)
        else:
            dx, dgamma, dbeta = ext.ln_shift_bwd(
                x, dy.contiguous(), weight, mean, rstd, dres.contiguous())
        return dx, dgamma.to(weight.dtype), dbeta.to(weight.dtype), None, None


class _LnShiftFn(torch.autograd.Function):
    """token_shift(layer_norm(x)) without the intermediate tensor: the LN
    kernel stores each channel group at the row the shift moves it to, and
    the backward reads dy through the transposed gather."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, text_len, image_size, dres=None):
        ext = hip_module()
        x = x.contiguous()
        y, mean, rstd = ext.ln_shift_fwd(x, weight, bias, eps, text_len,
                                         image_size)
        ctx.save_for_backward(x, weight, mean, rstd)
        ctx.shift = (text_len, image_size)
        ctx.dres = dres
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = hip_module()
        x, weight, mean, rstd = ctx.saved_tensors
        dres, ctx.dres = ctx.dres, None
        dx, dgamma, dbeta = ext.ln_shift_bwd(
            x, dy.contiguous(), weight, mean, rstd,
            None if dres is None else dres.contiguous(), *ctx.shift)
        return (dx, dgamma.to(weight.dtype), dbeta.to(weight.dtype),
                None, None, None, None)


_LN_DIMS = (512, 1024, 1536, 2048)


def layer_norm_fused(x):
    """True when layer_norm(x) takes the HIP kernel (which can also fold a
    residual-stream gradient into its backward)."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] in _LN_DIMS
            and not using_eager_fallback(x))


def layer_norm(x, weight, bias, eps=1e-5, dres=None):
    """LayerNorm over the last dim; fused bf16 kernel on GPU for the
    transformer widths, F.layer_norm elsewhere. Matches autocast semantics
    (fp32 statistics and affine) with a single bf16 rounding at the output.

    ``dres`` is only accepted where ``layer_norm_fused(x)`` holds: the
    backward then returns dres + dx (see _LayerNormFn).
    """
    if layer_norm_fused(x):
        return _LayerNormFn.apply(x, weight, bias, eps, dres)
    assert dres is None, 'dres needs the fused LayerNorm path'
    if weight is not None and weight.dtype != x.dtype and x.dtype != torch.float32:
        weight = weight.to(x.dtype)
        bias = bias.to(x.dtype) if bias is not None else None
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def ln_shift_supported(x):
    return (fusion_enabled('LN_SHIFT') and x.dim() == 3 and layer_norm_fused(x)
            and token_shift_supported(x))


def ln_shift(x, weight, bias, eps, text_len, image_size, dres=None):
    """token_shift(layer_norm(x), text_len, image_size) in one pass over x
    ([b, n, dim], n >= text_len). Bitwise the composition of the two
    kernels; elsewhere (CPU, other widths) the composition itself runs."""
    if ln_shift_supported(x):
        return _LnShiftFn.apply(x, weight, bias, eps, text_len, image_size,
                                dres)
    y = layer_norm(x, weight, bias, eps, dres)
    if token_shift_supported(y):
        return token_shift(y, text_len, image_size)
    return token_shift_eager(y, text_len, image_size)


def rev_replay_supported(o, y, d):
    return o.shape == y.shape == d.shape and _rows_of_8(o, y, d)


def rev_replay(o, gamma, y, d):
    """Reversible replay tail for a LayerScale'd branch, one pass:

        x_rec  = y - gamma * o          (input of the block, reconstructed)
        d_o    = gamma * d              (gradient w.r.t. the raw output o)
        dgamma = sum_rows(d * o)        (gradient w.r.t. gamma, its shape)

    gamma stays fp32 and x_rec is rounded once, mirroring add_scaled's
    forward. No autograd: the executor feeds d_o / dgamma to backward()."""
    o, y, d = o.detach(), y.detach(), d.detach()
    if rev_replay_supported(o, y, d):
        ext = hip_module()
        gf = gamma.detach().reshape(-1).float().contiguous()
        x_rec, d_o, dg = ext.rev_replay(o.contiguous(), gf, y.contiguous(),
                                        d.contiguous())
        return x_rec, d_o, dg.reshape(gamma.shape).to(gamma.dtype)
    g = gamma.detach()
    x_rec = (y - g * o).to(y.dtype)
    d_o = (g * d).to(o.dtype)
    dg = (d.float() * o.float()).reshape(-1, o.shape[-1]).sum(0)
    return x_rec, d_o, dg.reshape(gamma.shape).to(gamma.dtype)


def geglu_colsum_tiles(width):
    """geglu_bwd_colsum's tiling rule for a GEGLU input of ``width`` = 2H
    channels: the H/8 column groups of a half row are a multiple or a
    divisor of the 256-thread block."""
    h8, rest = divmod(width, 16)
    return rest == 0 and h8 > 0 and (h8 % 256 == 0 or 256 % h8 == 0)


def geglu_bwd_colsum_supported(x):
    return (x.is_cuda and x.dtype == torch.bfloat16
            and geglu_colsum_tiles(x.shape[-1]) and not using_eager_fallback(x))


def geglu_bwd_colsum(x, dout):
    """(dx, column sums of dx over all rows, fp32 [2H]) for out = geglu(x):
    the kernel emits the bias gradient of the linear that produced x while
    writing dx. Eager equivalent elsewhere."""
    if geglu_bwd_colsum_supported(x) and dout.dtype == torch.bfloat16:
        ext = hip_module()
        dx, cs = ext.geglu_bwd_colsum(x.contiguous(), dout.contiguous())
        return dx, cs
    if not using_eager_fallback(x):
        dx = hip_module().geglu_bwd(x.contiguous(), dout.contiguous())
    else:
        with torch.enable_grad():
            xl = x.detach().requires_grad_(True)
            a, b = xl.chunk(2, dim=-1)
            out = a * F.gelu(b)
        dx, = torch.autograd.grad(out, xl, dout)
    return dx, dx.reshape(-1, dx.shape[-1]).float().sum(0)
