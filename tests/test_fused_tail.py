"""GPU numerics of the fused training-tail kernels: LayerNorm + token shift
(ln_shift), the reversible replay tail (rev_replay), geglu_bwd with column
sums, and one end-to-end reversible training step with the fusions on/off."""

import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TEXT_LEN, S = 5, 4


@pytest.fixture(scope='module')
def ext():
    import dalle_pytorch_amd._hip as m
    return m


def _poison_allocator(mb=64):
    """Leave NaNs in the caching allocator's free blocks so a kernel output
    element that is never written reads back as NaN."""
    t = torch.full((mb << 18,), float('nan'), device='cuda')
    del t
    torch.cuda.synchronize()


def _rel(got, want):
    return ((got.float() - want.float()).abs().max()
            / want.float().abs().max().clamp(min=1e-6)).item()


# (b, n): full grid, grid minus one, partial last grid row (22 rows: the
# two-rows-per-wave tail), text only, odd total row count
SHIFT_SHAPES = [(2, TEXT_LEN + 16), (2, TEXT_LEN + 15), (2, TEXT_LEN + 6),
                (2, TEXT_LEN), (1, TEXT_LEN + 8)]
SHIFT_CASES = [(dim, b, n) for dim in (512, 1024) for b, n in SHIFT_SHAPES]


def _ln_inputs(dim, b, n, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = (torch.randn(b, n, dim, device='cuda', generator=g) * 2 + 0.5).bfloat16()
    w = torch.randn(dim, device='cuda', generator=g)
    bias = torch.randn(dim, device='cuda', generator=g)
    dy = torch.randn(b, n, dim, device='cuda', generator=g).bfloat16()
    dres = torch.randn(b, n, dim, device='cuda', generator=g).bfloat16()
    return x, w, bias, dy, dres


@pytest.mark.parametrize('dim,b,n', SHIFT_CASES)
def test_ln_shift_fwd_bitwise(ext, dim, b, n):
    x, w, bias, _, _ = _ln_inputs(dim, b, n, 21)
    y0, mean0, rstd0 = ext.ln_fwd(x, w, bias, 1e-5)
    want = ext.token_shift(y0, TEXT_LEN, S, False)
    _poison_allocator()
    got, mean, rstd = ext.ln_shift_fwd(x, w, bias, 1e-5, TEXT_LEN, S)
    assert not torch.isnan(got.float()).any(), 'unwritten output element'
    assert torch.equal(got, want)
    assert torch.equal(mean, mean0) and torch.equal(rstd, rstd0)


def _shift_full(x, t, s):
    from dalle_pytorch_amd.models.transformer import PreShiftToken
    n_full = t - 1 + s * s
    return PreShiftToken(lambda v: v, image_size=s, seq_len=n_full)._shift_full(x)


@pytest.mark.parametrize('with_dres', [False, True])
@pytest.mark.parametrize('dim,b,n', SHIFT_CASES)
def test_ln_shift_bwd_vs_oracle(ext, dim, b, n, with_dres):
    x, w, bias, dy, dres = _ln_inputs(dim, b, n, 22)
    _, mean, rstd = ext.ln_fwd(x, w, bias, 1e-5)
    _poison_allocator()
    dx, dgamma, dbeta = ext.ln_shift_bwd(x, dy, w, mean, rstd,
                                         dres if with_dres else None,
                                         TEXT_LEN, S)

    xr = x.float().requires_grad_()
    wr = w.clone().requires_grad_()
    br = bias.clone().requires_grad_()
    yr = _shift_full(F.layer_norm(xr, (dim,), wr, br), TEXT_LEN, S)
    yr.backward(dy.float())
    want_dx = xr.grad + (dres.float() if with_dres else 0)
    figs = (_rel(dx, want_dx), _rel(dgamma, wr.grad), _rel(dbeta, br.grad))
    print('ln_shift_bwd rel dx/dgamma/dbeta', dim, b, n, with_dres, figs)
    assert all(f < 2e-2 for f in figs), figs

    if not with_dres:
        # the per-row arithmetic is ln_bwd's: bitwise the two-kernel result
        dy_t = ext.token_shift(dy, TEXT_LEN, S, True)
        dx2, dgamma2, dbeta2 = ext.ln_bwd(x, dy_t, w, mean, rstd)
        assert torch.equal(dx, dx2)
        assert torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2)


def test_ln_shift_many_rows(ext):
    """3120 rows on a 32x32 grid: more rows than one pass of the backward's
    512 blocks x 4 waves, so its row loop and the partial sums over several
    rows per slot run. Both directions bitwise against the two kernels."""
    t, s, b = 17, 32, 3
    n = t + s * s - 1
    x, w, bias, dy, _ = _ln_inputs(1024, b, n, 24)
    y0, mean, rstd = ext.ln_fwd(x, w, bias, 1e-5)
    _poison_allocator()
    got, mean1, _ = ext.ln_shift_fwd(x, w, bias, 1e-5, t, s)
    assert torch.equal(got, ext.token_shift(y0, t, s, False))
    assert torch.equal(mean, mean1)
    dx, dgamma, dbeta = ext.ln_shift_bwd(x, dy, w, mean, rstd, None, t, s)
    dx2, dgamma2, dbeta2 = ext.ln_bwd(x, ext.token_shift(dy, t, s, True), w,
                                      mean, rstd)
    assert torch.equal(dx, dx2)
    assert torch.equal(dgamma, dgamma2) and torch.equal(dbeta, dbeta2)


def test_ln_dres_without_shift(ext):
    """dres on the plain (unshifted) LN backward: the shift_tokens=False /
    DALLE_AMD_LN_SHIFT=0 route of the reversible replay."""
    x, w, bias, dy, dres = _ln_inputs(1024, 3, 7, 23)
    _, mean, rstd = ext.ln_fwd(x, w, bias, 1e-5)
    dx0, dg0, db0 = ext.ln_bwd(x, dy, w, mean, rstd)
    _poison_allocator()
    dx, dg, db = ext.ln_shift_bwd(x, dy, w, mean, rstd, dres)
    xr = x.float().requires_grad_()
    F.layer_norm(xr, (1024,), w, bias).backward(dy.float())
    assert _rel(dx, xr.grad + dres.float()) < 2e-2
    assert torch.equal(dg, dg0) and torch.equal(db, db0)


# the last shape has more rows than 1024 blocks x 2 rows per pass: the
# kernel's row loop and multi-row dgamma accumulation run
@pytest.mark.parametrize('shape', [(3, 40, 512), (3, 40, 1024), (3, 40, 2048),
                                   (3, 41, 1024), (1, 2101, 1024)])
def test_rev_replay_vs_oracle(ext, shape):
    from dalle_pytorch_amd.ops.fused import rev_replay, rev_replay_supported
    torch.manual_seed(12)
    dim = shape[-1]
    o0, y0, d0 = (torch.randn(*shape, device='cuda') for _ in range(3))
    g0 = torch.randn(1, 1, dim, device='cuda') * 0.1
    o, y, d = o0.bfloat16(), y0.bfloat16(), d0.bfloat16()
    assert rev_replay_supported(o, y, d)
    _poison_allocator()
    x_rec, d_o, dg = rev_replay(o, g0, y, d)
    assert dg.shape == g0.shape and dg.dtype == g0.dtype

    of, yf, df = o.float(), y.float(), d.float()
    want_x = yf - g0 * of
    want_do = g0 * df
    want_dg = (df * of).reshape(-1, dim).sum(0)
    err_x = (x_rec.float() - want_x).abs().max().item()
    figs = (_rel(d_o, want_do), _rel(dg.reshape(-1), want_dg))
    print('rev_replay abs x_rec / rel d_o, dgamma', shape, err_x, figs)
    assert err_x < 0.05
    assert all(f < 5e-2 for f in figs), figs


# 1100 rows at h=4096: more rows than row slots in the grid (at most 1024
# there), so the kernel's row loop runs more than once
@pytest.mark.parametrize('rows,h', [(37, 512), (256, 512), (37, 4096),
                                    (256, 4096), (1100, 4096)])
def test_geglu_bwd_colsum(ext, rows, h):
    torch.manual_seed(13)
    x = torch.randn(rows, 2 * h, device='cuda').bfloat16()
    dout = torch.randn(rows, h, device='cuda').bfloat16()
    want = ext.geglu_bwd(x, dout)
    _poison_allocator()
    dx, cs = ext.geglu_bwd_colsum(x, dout)
    assert torch.equal(dx, want)
    assert cs.shape == (2 * h,) and cs.dtype == torch.float32
    rel = _rel(cs, dx.float().sum(0))
    print('geglu_bwd_colsum rel', rows, h, rel)
    assert rel < 2e-2


def test_linear_geglu_matches_unfused():
    """FeedForward with the fused linear -> GEGLU node vs the two separate
    nodes: same forward, same dx / dW (the GEMM inputs are bitwise equal),
    bias gradient within the column-sum bound."""
    from dalle_pytorch_amd.models.transformer import FeedForward
    from dalle_pytorch_amd.ops.fp8 import linear_geglu_ok
    torch.manual_seed(14)
    ff = FeedForward(512, mult=2).cuda()
    x0 = torch.randn(4, 256, 512, device='cuda').bfloat16()
    dout = torch.randn(4, 256, 512, device='cuda').bfloat16()
    res = {}
    for flag in ('1', '0'):
        os.environ['DALLE_AMD_FF1_BIAS'] = flag
        try:
            x = x0.clone().requires_grad_()
            assert linear_geglu_ok(ff.net[0], x) == (flag == '1')
            ff.zero_grad(set_to_none=True)
            with torch.autocast(device_type='cuda', dtype=torch.bfloat16):
                out = ff(x)
            out.backward(dout)
            res[flag] = (out.detach(), x.grad, ff.net[0].weight.grad.clone(),
                         ff.net[0].bias.grad.clone())
        finally:
            del os.environ['DALLE_AMD_FF1_BIAS']
    for a, b in list(zip(res['1'], res['0']))[:3]:
        assert torch.equal(a, b)
    rel = _rel(res['1'][3], res['0'][3])
    print('linear_geglu bias grad rel', rel)
    assert rel < 2e-2


_SWITCHES = ('DALLE_AMD_LN_SHIFT', 'DALLE_AMD_REV_REPLAY', 'DALLE_AMD_FF1_BIAS')


def _step(dalle, text, codes, autocast=True):
    dalle.zero_grad(set_to_none=True)
    with torch.autocast(device_type='cuda', dtype=torch.bfloat16,
                        enabled=autocast):
        loss = dalle(text, codes, return_loss=True)
    loss.backward()
    torch.cuda.synchronize()
    grads = torch.cat([p.grad.detach().float().flatten()
                       for p in dalle.parameters() if p.grad is not None])
    return loss.detach().clone(), grads


def test_reversible_step_fusions_on_off_vs_oracle(monkeypatch):
    """One bf16 training step of a small reversible, token-shifted, axial
    DALLE: fusions on vs off (same forward loss, bit for bit) and both
    against the eager fp32 oracle of the same weights."""
    from dalle_pytorch_amd import DALLE, DiscreteVAE
    import dalle_pytorch_amd.ops.dispatch as dispatch
    torch.manual_seed(0)
    vae = DiscreteVAE(image_size=64, num_layers=3, num_tokens=64,
                      codebook_dim=32, hidden_dim=8)
    dalle = DALLE(dim=512, vae=vae, num_text_tokens=100, text_seq_len=16,
                  depth=2, heads=8, dim_head=64, reversible=True,
                  attn_types=('axial_row', 'axial_col'), shift_tokens=True,
                  rotary_emb=True).cuda()
    text = torch.randint(1, 100, (2, 16), device='cuda')
    images = torch.rand(2, 3, 64, 64, device='cuda')
    with torch.no_grad():
        codes = dalle.vae.get_codebook_indices(images)

    for k in _SWITCHES:
        monkeypatch.setenv(k, '1')
    loss_on, g_on = _step(dalle, text, codes)
    for k in _SWITCHES:
        monkeypatch.setenv(k, '0')
    loss_off, g_off = _step(dalle, text, codes)
    for k in _SWITCHES:
        monkeypatch.delenv(k)

    # eager fp32 oracle of the same weights (as __graft_entry__.smoke())
    monkeypatch.setenv('DALLE_AMD_ALLOW_EAGER', '1')
    hip_saved = dispatch._HIP
    dispatch._HIP = None
    try:
        loss_ref, g_ref = _step(dalle, text, codes, autocast=False)
    finally:
        dispatch._HIP = hip_saved

    cos_on = F.cosine_similarity(g_on, g_ref, dim=0).item()
    cos_off = F.cosine_similarity(g_off, g_ref, dim=0).item()
    print(f'loss on/off/oracle {loss_on.item():.6f} {loss_off.item():.6f} '
          f'{loss_ref.item():.6f}  grad cos on/off {cos_on:.6f} {cos_off:.6f}')
    assert torch.equal(loss_on, loss_off)
    assert cos_on > 0.99
    assert cos_on >= cos_off - 1e-3
