"""Reversible executor, fused replay path (LayerScale'd branches): gradient
parity with plain autograd, hook firing and gradient accumulation. Runs on
CPU in fp32, where ops.fused.rev_replay computes the same math in torch."""

import torch
import torch.nn as nn

from dalle_pytorch_amd.models.reversible import ReversibleSequence
from dalle_pytorch_amd.models.transformer import LayerScale, PreNorm

DIM, DEPTH = 16, 3


class _Kw(nn.Module):
    """Swallow routed kwargs like the transformer wrappers do."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x, **kwargs):
        return self.net(x)


def make_blocks(seed=0):
    torch.manual_seed(seed)
    layers = nn.ModuleList()
    for ind in range(DEPTH):
        f = nn.Sequential(nn.Linear(DIM, DIM), nn.GELU(), nn.Linear(DIM, DIM))
        g = nn.Sequential(nn.Linear(DIM, DIM), nn.Tanh())
        layers.append(nn.ModuleList([
            LayerScale(DIM, ind + 1, PreNorm(DIM, _Kw(f))),
            LayerScale(DIM, ind + 1, PreNorm(DIM, _Kw(g)))]))
    # distinct per-channel scales: a uniform init would hide a mix-up of
    # channels or of the two branches' scales
    with torch.no_grad():
        for p in layers.parameters():
            if p.shape == (1, 1, DIM):
                p.copy_(torch.rand(1, 1, DIM) * 0.5 + 0.1)
    return layers


def reference(layers, x0):
    """Plain autograd over the same computation."""
    x1, x2 = x0.clone(), x0.clone()
    for (f, g) in layers:
        y1 = x1 + f(x2)
        y2 = x2 + g(y1)
        x1, x2 = y1, y2
    loss = ((x1 + x2) / 2).square().mean()
    loss.backward()
    return loss.detach(), [p.grad.clone() for p in layers.parameters()]


def rev_loss(layers, x):
    # the executor is one autograd node over the stream: its input has to
    # require grad for the backward to reach it
    x = x.detach().requires_grad_()
    return ReversibleSequence(layers)(x).square().mean()


def test_fused_replay_is_taken():
    """The branches here must exercise the fused executor path, not
    _replay_grad (guards the other tests against testing the old path)."""
    from dalle_pytorch_amd.models import reversible as R
    layers = make_blocks()
    calls = []
    orig = R.ReversibleBlock._replay_fused

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    R.ReversibleBlock._replay_fused = staticmethod(spy)
    try:
        rev_loss(layers, torch.randn(2, 5, DIM)).backward()
    finally:
        R.ReversibleBlock._replay_fused = staticmethod(orig)
    assert len(calls) == 2 * DEPTH


def test_fused_replay_matches_autograd():
    torch.manual_seed(1)
    x = torch.randn(2, 5, DIM).requires_grad_()
    layers = make_blocks()
    loss = ReversibleSequence(layers)(x).square().mean()
    loss.backward()
    dx = x.grad.clone()
    x.grad = None

    layers2 = make_blocks()   # same seed -> same weights
    loss_ref, ref_grads = reference(layers2, x)

    assert torch.allclose(loss, loss_ref, atol=1e-6)
    names = [n for n, _ in layers.named_parameters()]
    assert any(n.endswith('scale') for n in names)
    for n, p, want in zip(names, layers.parameters(), ref_grads):
        assert p.grad is not None, n
        assert torch.allclose(p.grad, want, atol=1e-5), (n, (p.grad - want).abs().max())
    assert torch.allclose(dx, x.grad, atol=1e-5)


def test_fused_replay_off_switch_matches(monkeypatch):
    torch.manual_seed(2)
    x = torch.randn(2, 5, DIM)
    layers = make_blocks()
    rev_loss(layers, x).backward()
    monkeypatch.setenv('DALLE_AMD_REV_REPLAY', '0')
    layers2 = make_blocks()
    rev_loss(layers2, x).backward()
    for a, b in zip(layers.parameters(), layers2.parameters()):
        assert torch.allclose(a.grad, b.grad, atol=1e-5)


def test_fused_replay_fires_accumulate_hooks_once():
    torch.manual_seed(3)
    layers = make_blocks()
    fired = {}
    for n, p in layers.named_parameters():
        fired[n] = 0

        def hook(param, n=n):
            fired[n] += 1
        p.register_post_accumulate_grad_hook(hook)
    rev_loss(layers, torch.randn(2, 5, DIM)).backward()
    assert all(v == 1 for v in fired.values()), fired
    rev_loss(layers, torch.randn(2, 5, DIM)).backward()
    assert all(v == 2 for v in fired.values()), fired


def test_fused_replay_accumulates_over_backwards():
    torch.manual_seed(4)
    x = torch.randn(2, 5, DIM)
    layers = make_blocks()
    rev_loss(layers, x).backward()
    once = [p.grad.clone() for p in layers.parameters()]
    rev_loss(layers, x).backward()   # no zeroing in between
    for p, g in zip(layers.parameters(), once):
        assert torch.allclose(p.grad, 2 * g, atol=1e-5)
