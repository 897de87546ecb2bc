"""Which path each training op takes: HIP kernel node or eager torch.

The route is observed from outside — the class name of the output's
``grad_fn`` (a custom autograd node is named ``<Function>Backward``), or
the public ``*_supported`` / ``*_ok`` predicate where the op has no node of
its own — so a change to an eligibility rule cannot move a boundary
unnoticed. On CPU every op is eager; on the GPU each boundary is pinned from
both sides.
"""

import warnings

import pytest
import torch
from torch import nn

from dalle_pytorch_amd.ops import attention_core, geglu
from dalle_pytorch_amd.ops.fp8 import fp8_linear, linear_geglu_ok
from dalle_pytorch_amd.ops.fused import (
    add_scaled, geglu_bwd_colsum_supported, layer_norm, ln_shift,
    ln_shift_supported, rev_replay_supported, token_shift_supported)
from dalle_pytorch_amd.ops.rope import rope_split_supported

# what every custom autograd.Function's node derives from; a torch node
# (AddBackward0, NativeLayerNormBackward0, ...) does not
CUSTOM_NODE = torch.autograd.function.BackwardCFunction
_SWITCHES = ('DALLE_AMD_LN_SHIFT', 'DALLE_AMD_REV_REPLAY',
             'DALLE_AMD_FF1_BIAS', 'DALLE_AMD_FP8', 'DALLE_AMD_ALLOW_EAGER')
TEXT_LEN, S = 4, 2     # [2, 8, dim]: 4 text rows + the full 2x2 grid


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _node(out):
    assert out.grad_fn is not None
    name = type(out.grad_fn).__name__
    return name if isinstance(out.grad_fn, CUSTOM_NODE) else 'eager:' + name


def _rand(*shape, dtype=torch.bfloat16, device='cpu', grad=True):
    return torch.randn(*shape, device=device).to(dtype).requires_grad_(grad)


def _add_scaled_node(dim, dtype, device, y_dtype=None):
    x = _rand(2, 8, dim, dtype=dtype, device=device)
    y = _rand(2, 8, dim, dtype=y_dtype or dtype, device=device)
    gamma = torch.full((1, 1, dim), 0.1, device=device, requires_grad=True)
    return _node(add_scaled(x, y, gamma))


def _rev_replay_ok(dim, dtype, device, y_dtype=None):
    o, d = (_rand(2, 8, dim, dtype=dtype, device=device, grad=False)
            for _ in range(2))
    y = _rand(2, 8, dim, dtype=y_dtype or dtype, device=device, grad=False)
    return rev_replay_supported(o, y, d)


def _ln_args(dim, dtype, device, lead=(2, 8)):
    x = _rand(*lead, dim, dtype=dtype, device=device)
    return (x, torch.ones(dim, device=device, requires_grad=True),
            torch.zeros(dim, device=device, requires_grad=True))


def _layer_norm_node(dim, dtype, device):
    return _node(layer_norm(*_ln_args(dim, dtype, device)))


def _ln_shift_node(dim, dtype, device):
    x, w, b = _ln_args(dim, dtype, device)
    return _node(ln_shift(x, w, b, 1e-5, TEXT_LEN, S))


def _geglu_node(last, dtype, device):
    return _node(geglu(_rand(2, 8, last, dtype=dtype, device=device)))


def _attention_node(nq, d, dtype, device):
    q, k, v = (_rand(2, 2, nq, d, dtype=dtype, device=device)
               for _ in range(3))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return _node(attention_core(q, k, v, d ** -0.5))


def _linear_geglu_ok(rows, device, bias=True, n_out=1024):
    lin = nn.Linear(512, n_out, bias=bias).to(device)
    return linear_geglu_ok(lin, _rand(1, rows, 512, device=device))


def _fp8_linear_node(rows, dtype, device):
    lin = nn.Linear(64, 64).to(device)
    with torch.autocast(device_type=torch.device(device).type,
                        dtype=torch.bfloat16):
        return _node(fp8_linear(lin, _rand(1, rows, 64, dtype=dtype,
                                           device=device)))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
def test_cpu_every_op_is_eager(dtype):
    for node in (_add_scaled_node(512, dtype, 'cpu'),
                 _layer_norm_node(512, dtype, 'cpu'),
                 _ln_shift_node(512, dtype, 'cpu'),
                 _geglu_node(32, dtype, 'cpu'),
                 _attention_node(32, 64, dtype, 'cpu'),
                 _fp8_linear_node(1024, dtype, 'cpu')):
        assert node.startswith('eager:'), node
    assert not _rev_replay_ok(512, dtype, 'cpu')
    assert not ln_shift_supported(_rand(2, 8, 512, dtype=dtype))
    assert not token_shift_supported(_rand(2, 8, 32, dtype=dtype))
    assert not geglu_bwd_colsum_supported(_rand(2, 8, 4096, dtype=dtype))
    assert not rope_split_supported(_rand(2, 8, 3 * 2 * 64, dtype=dtype), 64)
    lin = nn.Linear(512, 1024)
    assert not linear_geglu_ok(lin, _rand(1, 1024, 512, dtype=dtype))


gpu = pytest.mark.gpu
BF16, FP32 = torch.bfloat16, torch.float32


@gpu
@pytest.mark.parametrize('dim,dtype,y_dtype,kernel', [
    (512, BF16, None, True), (1024, BF16, None, True),
    (2048, BF16, None, True),
    (520, BF16, None, False),      # 8 | dim, but dim/8 = 65 does not divide 256
    (4096, BF16, None, False),     # dim/8 = 512 > 256
    (512, FP32, None, False), (512, BF16, FP32, False)])
def test_add_scaled_and_rev_replay_routes(dim, dtype, y_dtype, kernel):
    node = _add_scaled_node(dim, dtype, 'cuda', y_dtype)
    assert (node == '_AddScaledFnBackward') == kernel, node
    assert _rev_replay_ok(dim, dtype, 'cuda', y_dtype) == kernel


@gpu
@pytest.mark.parametrize('dim,dtype,kernel', [
    (512, BF16, True), (1024, BF16, True), (1536, BF16, True),
    (2048, BF16, True), (768, BF16, False), (512, FP32, False)])
def test_layer_norm_routes(dim, dtype, kernel):
    node = _layer_norm_node(dim, dtype, 'cuda')
    assert (node == '_LayerNormFnBackward') == kernel, node


@gpu
@pytest.mark.parametrize('switch,kernel', [(None, True), ('1', True),
                                           ('0', False)])
def test_ln_shift_routes(monkeypatch, switch, kernel):
    if switch is not None:
        monkeypatch.setenv('DALLE_AMD_LN_SHIFT', switch)
    node = _ln_shift_node(512, BF16, 'cuda')
    # switched off, the two separate kernels run: the shift's node is last
    want = '_LnShiftFnBackward' if kernel else '_TokenShiftFnBackward'
    assert node == want, node
    assert ln_shift_supported(_rand(2, 8, 512, device='cuda')) == kernel
    # 3-D input only
    assert not ln_shift_supported(_rand(16, 512, device='cuda'))
    assert not ln_shift_supported(_rand(2, 2, 8, 512, device='cuda'))
    # and only where both halves have a kernel
    assert not ln_shift_supported(_rand(2, 8, 768, device='cuda'))
    assert not ln_shift_supported(_rand(2, 8, 512, dtype=FP32, device='cuda'))


@gpu
@pytest.mark.parametrize('last,kernel', [(32, True), (24, False)])
def test_geglu_routes(last, kernel):
    node = _geglu_node(last, BF16, 'cuda')
    assert (node == '_GegluFnBackward') == kernel, node


@gpu
@pytest.mark.parametrize('h8,ok', [(1, True), (3, False), (256, True),
                                   (384, False), (512, True), (768, True)])
def test_geglu_bwd_colsum_supported(h8, ok):
    """h8 = H/8 column groups per half row: a divisor or a multiple of 256
    (768 = 3 x 256 is one; 384 is neither)."""
    x = _rand(2, 8, 16 * h8, device='cuda', grad=False)
    assert geglu_bwd_colsum_supported(x) == ok
    assert not geglu_bwd_colsum_supported(x.float())


@gpu
def test_linear_geglu_ok_routes(monkeypatch):
    assert _linear_geglu_ok(1024, 'cuda')
    assert not _linear_geglu_ok(1008, 'cuda')       # below the 1024-row floor
    assert not _linear_geglu_ok(1024, 'cuda', bias=False)
    # 2H = 48: 3 column groups of 8 per half do not tile a 256-thread block
    assert not _linear_geglu_ok(1024, 'cuda', n_out=48)
    with torch.no_grad():       # neither custom-backward linear path applies
        assert not _linear_geglu_ok(1024, 'cuda')
    monkeypatch.setenv('DALLE_AMD_FF1_BIAS', '0')
    assert not _linear_geglu_ok(1024, 'cuda')


@gpu
@pytest.mark.parametrize('rows,dtype,kernel', [
    (1024, BF16, True), (1008, BF16, False), (1024, FP32, False)])
def test_fp8_linear_routes(rows, dtype, kernel):
    node = _fp8_linear_node(rows, dtype, 'cuda')
    # the custom-backward linear node, whatever its name
    assert node.startswith('eager:') != kernel, node


@gpu
@pytest.mark.parametrize('nq,d,dtype,kernel', [
    (32, 64, BF16, True), (31, 64, BF16, False), (32, 32, BF16, False),
    (32, 64, torch.float16, False)])
def test_attention_core_routes(nq, d, dtype, kernel):
    node = _attention_node(nq, d, dtype, 'cuda')
    assert (node == '_FlashAttentionBackward') == kernel, node


@gpu
def test_rope_split_and_token_shift_supported():
    qkv = _rand(2, 8, 3 * 2 * 64, device='cuda', grad=False)
    assert rope_split_supported(qkv, 64)
    assert not rope_split_supported(qkv, 32)
    assert not rope_split_supported(qkv.float(), 64)
    # row bytes a multiple of 64 or not
    assert token_shift_supported(_rand(2, 8, 32, device='cuda', grad=False))
    assert not token_shift_supported(_rand(2, 8, 24, device='cuda',
                                           grad=False))
