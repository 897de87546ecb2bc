"""Split-K weight gradient: torch.ops.dalle_amd.wgrad_splitk (ATen batched
GEMM over row chunks + wgrad_reduce_kernel), the wgrad_splits rule and the
_gemm_backward call site.

Error bound against the fp64 oracle, elementwise and derived (not tuned):

    |got - ref| <= 2^-8 * sum_s |partial_s|  +  2^-20 * sum |terms|

The first term covers one bf16 rounding (relative 2^-8 at most) per chunk
partial; with fp32 partials it is slack for the single output rounding. The
second covers fp32 accumulation of the products. Partials and absolute term
sums are the oracle's own."""

import pytest
import torch

import dalle_pytorch_amd.ops.fp8 as fp8
from dalle_pytorch_amd.ops.dispatch import hip_module

gpu = pytest.mark.gpu
BF16, FP32 = torch.bfloat16, torch.float32
BLOCKS = 8      # finest chunking any case uses: one input offset per block

# the six flagship weight gradients (rows, n, k): ff1, ff2, qkv, out-proj,
# text and image slices of the CE head
FLAGSHIP = [(81920, 8192, 1024), (81920, 1024, 4096), (81920, 3072, 1024),
            (81920, 1024, 1024), (16448, 10256, 1024), (65472, 8192, 1024)]
SMALL = [(64, 64, 64), (1024, 1024, 1024), (4096, 1024, 512),
         (8192, 1024, 1024), (8200, 512, 512), (12288, 256, 256),
         (16384, 1000, 1024), (16384, 1024, 1032), (1 << 20, 64, 64),
         (24576, 4096, 4096), (81920, 16, 16), (3 * 8192, 512, 2048)]


@pytest.fixture(scope='module')
def ops():
    if hip_module() is None:
        pytest.skip('extension not built')
    return torch.ops.dalle_amd


def _poison_allocator(mb=64):
    """Leave NaNs in the caching allocator's free blocks so an output
    element that is never written reads back as NaN."""
    t = torch.full((mb << 18,), float('nan'), device='cuda')
    del t
    torch.cuda.synchronize()


_CASES = {}


def _case(M, n, k):
    """bf16 operands with a per-block offset (a chunk read twice or skipped
    moves the answer well outside the bound) and the fp64 oracle, computed
    once per shape: per-block partials [BLOCKS, n, k] and sum |terms|."""
    if (M, n, k) not in _CASES:
        g = torch.Generator(device='cuda').manual_seed(M + n + k)
        step = torch.arange(1, BLOCKS + 1, device='cuda').repeat_interleave(
            M // BLOCKS)[:, None]
        do2 = (torch.randn(M, n, device='cuda', generator=g)
               + 0.1 * step).bfloat16()
        x2 = (torch.randn(M, k, device='cuda', generator=g)
              + 0.05 * step).bfloat16()
        dd = do2.double().view(BLOCKS, M // BLOCKS, n)
        xd = x2.double().view(BLOCKS, M // BLOCKS, k)
        parts = torch.bmm(dd.transpose(1, 2), xd)
        terms = torch.bmm(dd.abs().transpose(1, 2), xd.abs()).sum(0)
        _CASES[M, n, k] = (do2, x2, parts, terms)
    return _CASES[M, n, k]


def _bound(parts, terms, S):
    """The module docstring's bound for S chunks, from [B, n, k] oracle
    partials of equal row blocks (S divides B)."""
    chunk = parts.view(S, parts.shape[0] // S, *parts.shape[1:]).sum(1)
    return 2.0 ** -8 * chunk.abs().sum(0) + 2.0 ** -20 * terms


def _check(got, parts, terms, S, what):
    ref = parts.sum(0)
    err = (got.double() - ref).abs()
    bound = _bound(parts, terms, S)
    print(f'{what}: max err {err.max().item():.3e}, '
          f'max err/bound {(err / bound).max().item():.3e}')
    assert (err <= bound).all()
    return err.max().item()


@gpu
@pytest.mark.parametrize('M,n,k,S', [
    (2560, 256, 512, 1), (2560, 256, 512, 2), (2560, 256, 512, 4),
    (2560, 256, 512, 8), (1280, 1024, 64, 1), (1280, 1024, 64, 4)])
def test_numerics_vs_fp64(ops, M, n, k, S):
    do2, x2, parts, terms = _case(M, n, k)
    err = {}
    for dt in (FP32, BF16):
        got = ops.wgrad_splitk(do2, x2, S, dt)
        assert got.shape == (n, k) and got.dtype == dt
        err[dt] = _check(got, parts, terms, S, f'S={S} -> {dt}')
    # fp32 partials: no worse than today's expression against the oracle
    today = ((do2.t() @ x2).double() - parts.sum(0)).abs().max().item()
    print(f'today max err {today:.3e}')
    assert err[FP32] <= today
    # with one bf16 rounding at the store the two differ only where fp32
    # accumulation noise moves a value across a rounding boundary
    assert err[BF16] <= today + 2.0 ** -20 * terms.max().item()


@gpu
@pytest.mark.parametrize('dt', [FP32, BF16])
@pytest.mark.parametrize('S', [1, 4])
def test_output_fully_written(ops, S, dt):
    do2, x2, _, _ = _case(2560, 256, 512)
    _poison_allocator()
    got = ops.wgrad_splitk(do2, x2, S, dt)
    assert not torch.isnan(got).any()


@gpu
@pytest.mark.parametrize('S', [1, 8])
def test_reproducible(ops, S):
    do2, x2, _, _ = _case(2560, 256, 512)
    for dt in (FP32, BF16):
        a = ops.wgrad_splitk(do2, x2, S, dt)
        _poison_allocator(8)
        assert torch.equal(a, ops.wgrad_splitk(do2, x2, S, dt))


@gpu
@pytest.mark.parametrize('wdtype', [FP32, BF16])
def test_linear_backward_split_vs_switch_off(ops, monkeypatch, wdtype):
    """nn.Linear(512, 1024) at 4096 rows through fp8_linear, the rule forced
    to S = 4, against DALLE_AMD_WGRAD_SPLITK=0: everything but dW bitwise
    equal, dW within the bound, gradient dtypes unchanged."""
    torch.manual_seed(5)
    rows, S = 4096, 4
    lin = torch.nn.Linear(512, 1024).cuda().to(wdtype)
    x0 = torch.randn(rows, 512, device='cuda').bfloat16()
    dout = torch.randn(rows, 1024, device='cuda').bfloat16()
    monkeypatch.setattr(fp8, 'wgrad_splits', lambda r, n, k: S)
    calls = []
    real = fp8._wgrad_op
    monkeypatch.setattr(fp8, '_wgrad_op',
                        lambda *a: calls.append(a[2]) or real(*a))
    res = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('DALLE_AMD_WGRAD_SPLITK', flag)
        x = x0.clone().requires_grad_()
        lin.zero_grad(set_to_none=True)
        with torch.autocast(device_type='cuda', dtype=BF16):
            out = fp8.fp8_linear(lin, x)
        assert type(out.grad_fn).__name__ == '_LinearFnBackward'
        out.backward(dout)
        res[flag] = (out.detach(), x.grad, lin.bias.grad, lin.weight.grad)
    assert calls == [S]                     # once, with the switch on only
    on, off = res['1'], res['0']
    for a, b in zip(on[:3], off[:3]):
        assert torch.equal(a, b)
    assert on[3].dtype == off[3].dtype == wdtype
    assert on[2].dtype == wdtype
    dd = dout.double().view(S, rows // S, 1024)
    xd = x0.double().view(S, rows // S, 512)
    parts = torch.bmm(dd.transpose(1, 2), xd)
    terms = torch.bmm(dd.abs().transpose(1, 2), xd.abs()).sum(0)
    _check(on[3], parts, terms, S, f'linear dW, {wdtype} weights')


def _pow2(s):
    return s >= 1 and s & (s - 1) == 0


@pytest.mark.parametrize('rows,n,k', FLAGSHIP + SMALL)
def test_rule_properties(rows, n, k):
    s = fp8.wgrad_splits(rows, n, k)
    assert _pow2(s) and s <= fp8.WGRAD_MAX_SPLITS
    assert rows % s == 0
    if s > 1:
        assert rows // s >= fp8.WGRAD_CHUNK_FLOOR
        assert rows >= fp8.WGRAD_ROW_FLOOR
        assert n % 16 == 0 and k % 16 == 0
    if rows < fp8.WGRAD_ROW_FLOOR:
        assert s == 1


def test_rule_is_pure_and_monotone_in_tiles():
    assert fp8.wgrad_splits(81920, 1024, 1024) == \
        fp8.wgrad_splits(81920, 1024, 1024)
    # a smaller output never gets fewer splits at the same row count
    prev = fp8.WGRAD_MAX_SPLITS
    for n in (256, 1024, 4096, 16384):
        s = fp8.wgrad_splits(81920, n, 1024)
        assert s <= prev
        prev = s


def test_plan_off_the_kernel_path(monkeypatch):
    monkeypatch.setattr(fp8, 'wgrad_splits', lambda r, n, k: 4)
    do2 = torch.randn(16384, 64).bfloat16()
    x2 = torch.randn(16384, 32).bfloat16()
    assert fp8.wgrad_plan(do2, x2, FP32) == 0            # CPU tensors
    monkeypatch.setenv('DALLE_AMD_WGRAD_SPLITK', '0')
    assert fp8.wgrad_plan(do2, x2, FP32) == 0


@gpu
def test_plan_on_the_kernel_path(ops, monkeypatch):
    monkeypatch.delenv('DALLE_AMD_WGRAD_SPLITK', raising=False)
    monkeypatch.setattr(fp8, 'wgrad_splits', lambda r, n, k: 4)
    do2 = torch.zeros(4096, 64, device='cuda', dtype=BF16)
    x2 = torch.zeros(4096, 32, device='cuda', dtype=BF16)
    assert fp8.wgrad_plan(do2, x2, FP32) == 4
    assert fp8.wgrad_plan(do2, x2, BF16) == 4
    assert fp8.wgrad_plan(do2, x2, torch.float16) == 0   # unsupported store
    assert fp8.wgrad_plan(do2.float(), x2.float(), FP32) == 0
    assert fp8.wgrad_plan(do2[:, ::2], x2, FP32) == 0    # non-contiguous
    monkeypatch.setenv('DALLE_AMD_WGRAD_SPLITK', '0')
    assert fp8.wgrad_plan(do2, x2, FP32) == 0
    monkeypatch.setenv('DALLE_AMD_ALLOW_EAGER', '1')
    monkeypatch.delenv('DALLE_AMD_WGRAD_SPLITK')
    import dalle_pytorch_amd.ops.dispatch as dispatch
    monkeypatch.setattr(dispatch, '_HIP', None)
    assert fp8.wgrad_plan(do2, x2, FP32) == 0            # eager fallback


def test_op_registered(ops):
    assert hasattr(ops, 'wgrad_splitk') and hasattr(ops, 'wgrad_reduce')
    assert not hasattr(hip_module(), 'wgrad_splitk')


# every argument check runs before anything touches the device, so the same
# messages come back for CPU tensors
@pytest.mark.parametrize('device', ['cpu', pytest.param('cuda', marks=gpu)])
def test_op_rejects_bad_arguments(ops, device):
    do2 = torch.zeros(80, 32, device=device, dtype=BF16)
    x2 = torch.zeros(80, 16, device=device, dtype=BF16)
    bad = [
        ((do2.float(), x2, 2, FP32), 'must be bfloat16'),
        ((do2, x2.half(), 2, FP32), 'must be bfloat16'),
        ((do2.t().contiguous().t(), x2, 2, FP32), 'must be contiguous'),
        ((do2, torch.zeros(80, 32, device=device, dtype=BF16)[:, ::2], 2,
          FP32), 'must be contiguous'),
        ((do2, x2[:64], 2, FP32), 'row counts differ'),
        ((do2, x2, 32, FP32), 'does not divide'),
        ((do2, x2, 3, FP32), 'power of two'),
        ((do2, x2, 0, FP32), 'power of two'),
        ((do2, x2, 2, torch.float16), 'out_dtype'),
    ]
    for args, msg in bad:
        with pytest.raises(RuntimeError, match='wgrad_splitk: .*' + msg):
            ops.wgrad_splitk(*args)
    if device == 'cpu':
        with pytest.raises(RuntimeError, match='must be GPU tensors'):
            ops.wgrad_splitk(do2, x2, 2, FP32)
