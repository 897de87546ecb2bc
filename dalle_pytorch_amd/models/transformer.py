"""Transformer assembly: wrapper chain, feed-forward, token shift, rotary.

Parity target: reference transformer.py (layer cycling :204-328, wrappers
:38-102, GEGLU/FF :106-122, PreShiftToken :126-200, static axial masks
:333-350). The module *nesting and attribute names* deliberately reproduce
the reference checkpoint key schema so state dicts are
interchangeable; the compute inside routes through the fused CDNA4 ops.
"""

from collections import deque
from collections.abc import Iterable
from functools import partial
from itertools import islice, cycle

import torch
from torch import nn

from dalle_pytorch_amd.models.reversible import ReversibleSequence, SequentialSequence
from dalle_pytorch_amd.models.attention import (
    Attention, SparseAttention, SparseConvCausalAttention,
    SparseAxialCausalAttention, axial_mask, grid_text_len)
from dalle_pytorch_amd.models.positional import build_dalle_rotary_table
from dalle_pytorch_amd.ops import geglu
from dalle_pytorch_amd.ops.fp8 import fp8_linear, linear_geglu, linear_geglu_ok
from dalle_pytorch_amd.ops.fused import (token_shift, token_shift_eager,
                                          token_shift_supported,
                                          layer_norm, layer_norm_fused,
                                          ln_shift, ln_shift_supported,
                                          add_scaled)


_AXIAL_AXIS = {'axial_row': 0, 'axial_col': 1}


def _as_tuple(val, depth=1):
    return val if isinstance(val, Iterable) else (val,) * depth


class DivideMax(nn.Module):
    """x / max(x) with a detached max (reference transformer.py:29-36)."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        maxes = x.amax(dim=self.dim, keepdim=True).detach()
        return x / maxes


class NonCached(nn.Module):
    """Rebuilds the full sequence for layers without native cache support,
    then returns only the suffix (reference transformer.py:38-58).

    When no cache_key is supplied (the PreShiftToken wrapper does not thread
    one through, reference transformer.py:153,200 — under which the
    reference's sparse layers would all share ``cache[None]`` and corrupt
    each other during cached decode) a per-instance key is used instead.
    """

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x, *, cache=None, cache_key=None, **kwargs):
        n = x.shape[-2]
        if cache is not None:
            if cache_key is None:
                cache_key = ('noncached', id(self))
            if cache_key in cache:
                x = torch.cat([cache[cache_key], x], dim=-2)
            cache[cache_key] = x
        return self.fn(x, **kwargs)[:, -n:]


class CachedAs(nn.Module):
    """Names the cache slot for the wrapped layer (reference transformer.py:60-71)."""

    def __init__(self, cache_key, fn):
        super().__init__()
        self.cache_key = cache_key
        self.fn = fn

    def forward(self, x, *, cache=None, **kwargs):
        return self.fn(x, cache=cache, cache_key=self.cache_key, **kwargs)


class LayerScale(nn.Module):
    """Per-channel learned residual scale, depth-tiered init
    (https://arxiv.org/abs/2103.17239; reference transformer.py:74-88).

    When the caller passes ``residual=``, the residual add is fused with the
    scale into one HBM pass (ops.fused.add_scaled) — the executors use this,
    replacing the eager scale-cast + mul + add chain (5 tensor passes -> 3).
    """

    INIT_BY_DEPTH = ((18, 0.1), (24, 1e-5), (float('inf'), 1e-6))
    supports_residual = True   # executors may pass residual= for the fused add

    def __init__(self, dim, depth, fn):
        super().__init__()
        init_eps = next(eps for bound, eps in self.INIT_BY_DEPTH
                        if depth <= bound)
        self.scale = nn.Parameter(torch.full((1, 1, dim), init_eps))
        self.fn = fn

    def forward(self, x, residual=None, **kwargs):
        out = self.fn(x, **kwargs)
        if residual is not None:
            return add_scaled(residual, out, self.scale)
        # multiply in the stream dtype: a fp32 scale would silently promote
        # the bf16 residual stream (2x elementwise traffic downstream)
        return out * self.scale.to(out.dtype)


class PreNorm(nn.Module):
    """Pre-LN (optionally sandwich) around a layer (reference
    transformer.py:92-102); the norm runs through the fused bf16 kernel on
    GPU (ops/fused.py)."""

    def __init__(self, dim, fn, sandwich=False):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.norm_out = nn.LayerNorm(dim) if sandwich else nn.Identity()
        self.fn = fn

    def fuses_dres(self, x):
        """Whether forward(x, dres=...) can fold a residual-stream gradient
        into the input norm's backward (the reversible executor asks)."""
        return layer_norm_fused(x)

    def _shift_child(self, x, kwargs):
        """The PreShiftToken under this norm when LN + shift can run as one
        kernel for this call (training-shape, uncached), else None."""
        wrap = self.fn
        shift = wrap.fn if isinstance(wrap, CachedAs) else None
        if (isinstance(shift, PreShiftToken) and kwargs.get('cache') is None
                and x.dim() == 3 and x.shape[1] >= shift.text_len
                and ln_shift_supported(x)):
            return shift
        return None

    def forward(self, x, dres=None, **kwargs):
        """``dres`` (reversible replay only, see fuses_dres): gradient of
        the residual stream at x; x.grad then comes back as dres + the
        branch's own gradient, saving the executor's eager add."""
        shift = self._shift_child(x, kwargs)
        if shift is not None:
            # LN + token shift in one pass; PreShiftToken's inner fn takes
            # the shifted rows directly (it gets no cache / cache_key, as on
            # PreShiftToken's own uncached path)
            y = ln_shift(x, self.norm.weight, self.norm.bias, self.norm.eps,
                         shift.text_len, shift.image_size, dres)
            inner = {k: v for k, v in kwargs.items() if k != 'cache'}
            y = shift.fn(y, **inner)
        else:
            y = layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps,
                           dres)
            y = self.fn(y, **kwargs)
        if isinstance(self.norm_out, nn.LayerNorm):
            y = layer_norm(y, self.norm_out.weight, self.norm_out.bias,
                           self.norm_out.eps)
        return y


class GEGLU(nn.Module):
    def forward(self, x):
        return geglu(x)


class FeedForward(nn.Module):
    """Linear -> GEGLU -> Dropout -> Linear (reference transformer.py:111-122).
    The two projections route through the optional fp8 forward path
    (ops/fp8.py, DALLE_AMD_FP8=1) — e4m3 MFMA runs at 2x the bf16 rate."""

    def __init__(self, dim, dropout=0., mult=4.):
        super().__init__()
        self.net = nn.Sequential(
            nn.Linear(dim, int(dim * mult * 2)),
            GEGLU(),
            nn.Dropout(dropout),
            nn.Linear(int(dim * mult), dim),
        )

    def forward(self, x, cache=None, cache_key=None):
        if linear_geglu_ok(self.net[0], x):
            # one autograd node: the ff1 bias gradient comes out of geglu_bwd
            x = linear_geglu(self.net[0], x)
        else:
            x = self.net[1](fp8_linear(self.net[0], x))
        x = self.net[2](x)
        return fp8_linear(self.net[3], x)


class PreShiftToken(nn.Module):
    """Token-shift preprocessor (same contract as reference
    transformer.py:126-200, re-expressed).

    Channel layout: for text positions the FIRST HALF of the channels reads
    from the previous token; for image positions the first quarter reads
    from the grid row above and the second quarter from the left neighbor
    (zeros where no such neighbor exists). The cached decode path keeps a
    ring of the last ``image_size`` positions' RAW (top, left) quarters so a
    single-token step reproduces the training-time shift.

    Deviations from the reference: (a) the training path on GPU is one fused
    gather kernel; (b) the ring is seeded from the raw inputs — the
    reference seeds it from already-shifted values (transformer.py:193-198),
    so its first ``image_size`` primed-generation steps read neighbors one
    step too far back and cached priming diverges from uncached (pinned by
    tests/test_dalle.py::test_primed_cached_generation_matches_uncached).
    """

    def __init__(self, fn, image_size, seq_len):
        super().__init__()
        self.fn = fn
        self.image_size = image_size
        self.seq_len = seq_len
        self.img_seq_len = image_size ** 2
        self.text_len = grid_text_len(seq_len, image_size)

    def _shift_full(self, x):
        """Training-shape shift, whole sequence at once (eager path)."""
        return token_shift_eager(x, self.text_len, self.image_size)

    def _seed_ring(self, x):
        """Ring of the last S image positions' raw (top, left) quarters,
        front-padded with zeros when fewer than S image tokens exist yet."""
        b, _, c = x.shape
        S, q = self.image_size, x.shape[-1] // 4
        tail = x[:, self.text_len:][:, -S:]
        zero = x.new_zeros(b, q)
        ring = deque((zero, zero) for _ in range(S - tail.shape[1]))
        ring.extend((tail[:, i, :q], tail[:, i, q:2 * q])
                    for i in range(tail.shape[1]))
        return ring

    def _shift_one(self, x, ring, cache, kwargs):
        t, S = self.text_len, self.image_size
        offset = cache['offset']
        assert offset >= t, 'cached decode starts after the text prefix'
        assert len(ring) == S
        cur = x[:, -1]
        q = cur.shape[-1] // 4
        ring.append((cur[:, :q], cur[:, q:2 * q]))
        top = ring.popleft()[0]
        at_row_start = (offset - t) % S == 0
        left = torch.zeros_like(top) if at_row_start else ring[-2][1]
        shifted = torch.cat((top, left, cur[:, 2 * q:]), dim=-1)
        return self.fn(shifted[:, None], cache=cache, **kwargs)

    def forward(self, x, cache=None, cache_key=None, **kwargs):
        ring = cache.get(cache_key) if cache is not None else None
        if ring is not None:
            return self._shift_one(x, ring, cache, kwargs)
        if x.shape[1] < self.text_len:
            return self.fn(x, **kwargs)
        if cache is None and token_shift_supported(x):
            # fused gather kernel (no pad/cat/fill chain) — training hot path
            return self.fn(token_shift(x, self.text_len, self.image_size),
                           **kwargs)
        shifted = self._shift_full(x)
        if cache is not None:
            cache[cache_key] = self._seed_ring(x)
        return self.fn(shifted, cache=cache, **kwargs)


class Transformer(nn.Module):
    """depth x (attn, ff) stack with attention-type cycling, layer sharing,
    LayerScale, optional sandwich norm, token shifting, reversibility, and a
    host-precomputed rotary table (reference transformer.py:204-331)."""

    def __init__(
        self,
        *,
        dim,
        depth,
        seq_len,
        reversible=False,
        causal=True,
        heads=8,
        dim_head=64,
        ff_mult=4,
        attn_dropout=0.,
        ff_dropout=0.,
        attn_types=None,
        image_fmap_size=None,
        sparse_attn=False,
        stable=False,
        sandwich_norm=False,
        shift_tokens=False,
        rotary_emb=True,
        shared_attn_ids=None,
        shared_ff_ids=None,
        optimize_for_inference=False,
    ):
        super().__init__()
        self.seq_len = seq_len
        self.image_fmap_size = image_fmap_size
        del sparse_attn  # accepted for flag parity; per-layer value is unused
        # (the reference shadows and ignores it too, transformer.py:245-246)

        attn_kwargs = dict(causal=causal, seq_len=seq_len, heads=heads,
                           dim_head=dim_head, dropout=attn_dropout)
        self._attn_common = (attn_kwargs, stable, optimize_for_inference)

        attn_types = _as_tuple(attn_types if attn_types is not None else ('full',))
        plan = zip(islice(cycle(attn_types), depth),
                   cycle(shared_attn_ids if shared_attn_ids is not None else range(depth)),
                   cycle(shared_ff_ids if shared_ff_ids is not None else range(depth)))

        built_attn, built_ff = {}, {}
        layers = nn.ModuleList([])
        for ind, (attn_type, attn_id, ff_id) in enumerate(plan):
            if attn_id in built_attn:
                leaf, built_type = built_attn[attn_id]
                if built_type != attn_type:
                    raise ValueError(
                        f'attn_types do not match shared_attn_ids (ind={ind}, '
                        f'attn_type="{attn_type}", reused="{built_type}")')
            else:
                leaf = self._leaf_attention(attn_type, dim)
                built_attn[attn_id] = (leaf, attn_type)

            if ff_id not in built_ff:
                built_ff[ff_id] = FeedForward(dim, mult=ff_mult, dropout=ff_dropout)
            ff = built_ff[ff_id]

            # wrapper chain (outer to inner), identical key schema to the
            # reference: [CachedAs -> PreShiftToken ->]
            # CachedAs|NonCached -> leaf
            attn = (CachedAs(f'attn_{ind}', leaf) if isinstance(leaf, Attention)
                    else NonCached(leaf))
            if shift_tokens:
                wrap = partial(PreShiftToken, image_size=image_fmap_size,
                               seq_len=seq_len)
                attn = CachedAs(f'preshift_attn_{ind}', wrap(attn))
                ff = CachedAs(f'preshift_ff_{ind}', wrap(ff))

            layers.append(nn.ModuleList([
                LayerScale(dim, ind + 1, PreNorm(dim, attn, sandwich=sandwich_norm)),
                LayerScale(dim, ind + 1, PreNorm(dim, ff, sandwich=sandwich_norm)),
            ]))

        executor = ReversibleSequence if reversible else SequentialSequence
        to_attn_only = ((True, False),) * depth
        self.layers = executor(layers, args_route={
            'mask': to_attn_only,
            'rotary_pos_emb': to_attn_only,
            'cache': ((True, True),) * depth,
        })

        pos_emb = None
        if rotary_emb:
            pos_emb = build_dalle_rotary_table(
                dim_head, grid_text_len(seq_len, image_fmap_size),
                image_fmap_size)
        self.register_buffer('pos_emb', pos_emb)

    def forward(self, x, **kwargs):
        return self.layers(x, rotary_pos_emb=self.pos_emb, **kwargs)

    def _leaf_attention(self, attn_type, dim):
        """Construct the leaf attention module for one layer."""
        common, stable, opt_inference = self._attn_common
        S = self.image_fmap_size
        if attn_type == 'full':
            return Attention(dim, stable=stable, **common)
        if attn_type == 'sparse':
            return SparseAttention(dim, **common)
        if attn_type in _AXIAL_AXIS:
            if opt_inference:   # cache-friendly static-mask simulation
                return Attention(dim, stable=stable,
                                 static_mask=self._get_attention_mask(attn_type),
                                 **common)
            return SparseAxialCausalAttention(
                dim, axis=_AXIAL_AXIS[attn_type],
                image_size=S, stable=stable, **common)
        if attn_type == 'conv_like':
            return SparseConvCausalAttention(dim, image_size=S, stable=stable,
                                             **common)
        raise ValueError(f'attention type "{attn_type}" is not valid')

    def _get_attention_mask(self, attn_type):
        """Dense bool mask reproducing axial attention (reference
        transformer.py:333-350): text keys always visible; image keys only
        within the same grid row (axial_row) or column (axial_col)."""
        if attn_type not in _AXIAL_AXIS:
            raise ValueError(f'attention type "{attn_type}" cannot be simulated '
                             'with a static mask')
        S = self.image_fmap_size
        return axial_mask(self.seq_len, grid_text_len(self.seq_len, S), S,
                          _AXIAL_AXIS[attn_type])
