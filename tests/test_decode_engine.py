"""FastDecoder parity: engine generation must equal the model's dict-cache
generation (which is itself pinned bitwise-equal to uncached recompute)."""

import pytest
import torch

from dalle_pytorch_amd import DALLE, DiscreteVAE
from dalle_pytorch_amd.engine import FastDecoder

torch.manual_seed(0)


def tiny_dalle(**kw):
    vae = DiscreteVAE(image_size=64, num_layers=3, num_tokens=64,
                      codebook_dim=32, hidden_dim=8)
    args = dict(dim=32, num_text_tokens=50, text_seq_len=8, depth=2, heads=2,
                dim_head=16, attn_types=('full',), shift_tokens=True)
    args.update(kw)
    return DALLE(vae=vae, **args)


@pytest.mark.parametrize('kw', [
    dict(attn_types=('full',)),
    dict(attn_types=('full',), shift_tokens=False),
    dict(attn_types=('axial_row', 'axial_col')),
    dict(attn_types=('conv_like',)),
    dict(attn_types=('sparse',)),
    dict(attn_types=('full',), stable=True),
    dict(attn_types=('full', 'axial_row'), reversible=True),
    dict(attn_types=('full',), rotary_emb=False),
])
def test_engine_matches_model_generation(kw):
    torch.manual_seed(3)
    d = tiny_dalle(**kw).eval()
    text = torch.randint(1, 50, (2, 8))

    torch.manual_seed(11)
    ref = d.generate_images(text, use_cache=True, temperature=1e-8,
                            filter_thres=0.99)
    dec = FastDecoder(d, batch_size=2)
    torch.manual_seed(11)
    got = dec.generate(text, temperature=1e-8, filter_thres=0.99)
    assert torch.allclose(got, ref, atol=1e-4), \
        (got - ref).abs().max().item()


def test_engine_guided_matches_model_guided():
    """cond_scale != 1 on the fast path: the doubled-batch (cond + null)
    stream must reproduce the model's guided generation (which is itself
    pinned cached == uncached by test_dalle.py)."""
    torch.manual_seed(6)
    d = tiny_dalle(attn_types=('full', 'axial_row')).eval()
    text = torch.randint(1, 50, (2, 8))

    torch.manual_seed(23)
    ref = d.generate_images(text, use_cache=True, temperature=1e-8,
                            filter_thres=0.99, cond_scale=2.0)
    dec = FastDecoder(d, batch_size=4)   # 2*b for the guided stream pair
    torch.manual_seed(23)
    got = dec.generate(text, temperature=1e-8, filter_thres=0.99,
                       cond_scale=2.0)
    assert got.shape == ref.shape
    assert torch.allclose(got, ref, atol=1e-4), \
        (got - ref).abs().max().item()


def test_engine_step_logits_match_model_cache():
    """Per-step logits comparison (tighter than end-to-end argmax parity)."""
    torch.manual_seed(4)
    d = tiny_dalle(attn_types=('axial_row', 'axial_col')).eval()
    text = torch.randint(1, 50, (1, 8))

    cache = {}
    with torch.no_grad():
        ref_logits = d(text, None, cache=cache)[:, -1]
    dec = FastDecoder(d, batch_size=1)
    with torch.no_grad():
        got_logits = dec.prefill(text)
    valid = ref_logits > -1e30
    assert torch.allclose(got_logits[valid], ref_logits[valid], atol=1e-4)

    token = torch.tensor([5])
    with torch.no_grad():
        step_ref = d(text, token.unsqueeze(0), cache=cache)[:, -1]
        step_got = dec.step(token)
    valid = step_ref > -1e30
    assert torch.allclose(step_got[valid], step_ref[valid], atol=1e-4), \
        (step_got[valid] - step_ref[valid]).abs().max().item()


@pytest.mark.gpu
def test_engine_gpu_graph_mode():
    torch.manual_seed(5)
    d = tiny_dalle(attn_types=('axial_row', 'axial_col'), depth=2).cuda().eval()
    text = torch.randint(1, 50, (2, 8), device='cuda')
    torch.manual_seed(7)
    ref = d.generate_images(text, use_cache=True, temperature=1e-8,
                            filter_thres=0.99)
    dec = FastDecoder(d, batch_size=2, dtype=torch.float32, use_graph=True)
    torch.manual_seed(7)
    got = dec.generate(text, temperature=1e-8, filter_thres=0.99)
    assert torch.allclose(got, ref, atol=1e-3), (got - ref).abs().max().item()


@pytest.mark.gpu
def test_fused_decode_kernels_match_torch_path():
    """bf16 fused fa_decode/shift_decode vs the torch-op decode path."""
    torch.manual_seed(6)
    d = tiny_dalle(attn_types=('axial_row', 'full'), depth=2, dim=256,
                   heads=4, dim_head=64).cuda().eval()
    text = torch.randint(1, 50, (2, 8), device='cuda')
    token = torch.randint(0, 64, (2,), device='cuda')

    dec_f = FastDecoder(d, batch_size=2, dtype=torch.bfloat16)
    assert dec_f._fused_decode
    dec_t = FastDecoder(d, batch_size=2, dtype=torch.bfloat16, fused=False)
    assert not dec_t._fused_decode

    with torch.no_grad():
        a = dec_f.prefill(text)
        b = dec_t.prefill(text)
        for _ in range(5):
            a = dec_f.step(token)
            b = dec_t.step(token)
    valid = b > -1e30
    rel = (a[valid].float() - b[valid].float()).abs().max() / \
        b[valid].float().abs().max()
    assert rel < 5e-2, rel.item()


def test_sk2_pack_layout():
    """The sk2 packed-weight layout must match the kernel's index math:
    element (lane, e) of chunk (nt, kc) is w[nt*16 + (lane&15),
    kc*32 + (lane>>4)*8 + e] (decode.hip sk2_kernel). Pure-CPU check of
    the reshape/permute formula used by FastDecoder._sk2_pack."""
    N, K = 64, 1024
    w = torch.arange(N * K, dtype=torch.float32).reshape(N, K)
    pk = (w.reshape(N // 16, 16, K // 32, 4, 8)
           .permute(0, 2, 3, 1, 4).contiguous())    # [nt][kc][kg][col][e]
    flat = pk.reshape(N // 16, K // 32, 64, 8)      # lane = kg*16 + col
    for nt, kc, lane, e in [(0, 0, 0, 0), (1, 3, 17, 5), (3, 31, 63, 7),
                            (2, 10, 48, 2)]:
        col, kg = lane & 15, lane >> 4
        assert flat[nt, kc, lane, e] == w[nt * 16 + col, kc * 32 + kg * 8 + e]


def test_sk2_pack_gates():
    """_sk2_pack returns None for shapes the kernel contract rejects
    (K % 1024, N % 32) and for non-bf16/non-cuda tensors (CPU here)."""
    from dalle_pytorch_amd.engine.decode import FastDecoder
    assert FastDecoder._sk2_pack(torch.zeros(64, 512)) is None     # K % 1024
    assert FastDecoder._sk2_pack(torch.zeros(48, 1024)) is None    # N % 32
    assert FastDecoder._sk2_pack(torch.zeros(64, 1024)) is None    # cpu/fp32


@pytest.mark.gpu
def test_sk2_decode_path_matches_unpacked():
    """In-situ sk2 coverage: at batch 16 and dim 1024 every sk2 call site
    engages (qkv/out mode 0, geglu-fused ff1 mode 1, fp32 head mode 2).
    Parity against the same engine with sk2 disabled."""
    torch.manual_seed(9)
    d = tiny_dalle(attn_types=('axial_row', 'axial_col'), depth=2, dim=1024,
                   heads=16, dim_head=64).cuda().eval()
    text = torch.randint(1, 50, (16, 8), device='cuda')
    token = torch.randint(0, 64, (16,), device='cuda')

    dec_s = FastDecoder(d, batch_size=16, dtype=torch.bfloat16)
    assert dec_s._fused_decode and dec_s._sk2_on
    assert dec_s.states[0].qkv.pk is not None
    assert dec_s.head_img.pk is not None
    dec_u = FastDecoder(d, batch_size=16, dtype=torch.bfloat16, sk2=False)
    assert not dec_u._sk2_on

    with torch.no_grad():
        a = dec_s.prefill(text)
        b = dec_u.prefill(text)
        for _ in range(4):
            a = dec_s.step(token)
            b = dec_u.step(token)
    valid = b > -1e30
    rel = (a[valid].float() - b[valid].float()).abs().max() / \
        b[valid].float().abs().max()
    assert rel < 5e-2, rel.item()


def _linears(dec):
    """Every _DecodeLinear of a decoder, as (name, instance)."""
    out = [(f'{i}.{name}', getattr(st, name))
           for i, st in enumerate(dec.states)
           for name in (('qkv', 'out') if st.is_attn else ('ff1', 'ff2'))]
    return out + [('head_img', dec.head_img)]


def test_cpu_decoder_routes_are_plain():
    """Without the fused path every projection decodes through F.linear and
    holds nothing but the plain weight: no transposed copy, no pack."""
    dec = FastDecoder(tiny_dalle(), batch_size=2)
    assert not dec._fused_decode and not dec._sk2_on
    assert len(_linears(dec)) == 2 * 4 + 1
    for name, lin in _linears(dec):
        assert lin.route == 'linear', (name, lin.route)
        assert lin.wT is None and lin.pk is None and lin.pk8 is None, name
        assert lin.b32 is None, name


@pytest.fixture(scope='module')
def sk2_dalle():
    """Smallest model whose projections pass the sk2 pack gates
    (K % 1024 == 0, dim_head 64)."""
    torch.manual_seed(9)
    return tiny_dalle(attn_types=('axial_row', 'axial_col'), depth=2, dim=1024,
                      heads=16, dim_head=64).cuda().eval()


@pytest.mark.gpu
def test_decode_routes_fixed_at_construction(sk2_dalle, monkeypatch):
    """The GEMM route of each projection is chosen in the constructor from
    batch rows, weight shape and the switches, and only the tensors that
    route reads are built."""
    monkeypatch.delenv('DALLE_AMD_SK2', raising=False)
    monkeypatch.delenv('DALLE_AMD_SK2_MAXK', raising=False)
    monkeypatch.delenv('DALLE_AMD_FP8_DECODE', raising=False)

    dec = FastDecoder(sk2_dalle, batch_size=16)
    assert dec._fused_decode and dec._sk2_on and dec._fused_prelude
    for st in dec.states:
        if st.is_attn:
            for lin in (st.qkv, st.out):
                assert lin.route == 'sk2' and lin.mode == 0
                assert lin.pk is not None and lin.wT is None
        else:
            assert st.ff1.route == 'sk2' and st.ff1.mode == 1
            assert st.ff1.pk is not None
            assert st.ff2.w.shape[1] == 4096      # K above the 2048 default
            assert st.ff2.route == 'linear'
            assert st.ff2.pk is None and st.ff2.wT is None
    assert dec.head_img.route == 'sk2' and dec.head_img.mode == 2
    assert dec.head_img.pk is not None
    assert all(lin.pk8 is None for _, lin in _linears(dec))

    dec = FastDecoder(sk2_dalle, batch_size=16, sk2=False)
    assert dec._fused_decode and not dec._sk2_on
    for st in dec.states:
        if st.is_attn:
            for lin in (st.qkv, st.out):
                assert lin.route == 'transposed'
                assert lin.wT is not None and lin.pk is None
    assert all(lin.pk is None and lin.pk8 is None for _, lin in _linears(dec))

    # the stale-flag case: sk2 may not outlive the fused path it depends on
    dec = FastDecoder(sk2_dalle, batch_size=16, fused=False)
    assert not dec._fused_decode and not dec._sk2_on
    assert not dec._fused_prelude
    for name, lin in _linears(dec):
        assert not lin.route.startswith('sk2'), (name, lin.route)
        assert lin.pk is None and lin.pk8 is None, name

    monkeypatch.setenv('DALLE_AMD_SK2_MAXK', '4096')
    dec = FastDecoder(sk2_dalle, batch_size=16)
    for st in dec.states:
        if not st.is_attn:
            assert st.ff2.route == 'sk2' and st.ff2.pk is not None


@pytest.mark.gpu
def test_step_graph_and_token_graph_do_not_share(sk2_dalle):
    """_graph_step (logits out) and _graph_token_step (sampling included)
    each own their graph and static tensors: either order of use replays
    the right one. Eager counterparts come from a second decoder."""
    d = sk2_dalle
    torch.manual_seed(13)
    text = torch.randint(1, 50, (16, 8), device='cuda')
    token = torch.randint(0, 64, (16,), device='cuda')
    dec_g = FastDecoder(d, batch_size=16, dtype=torch.float32, use_graph=True)
    dec_e = FastDecoder(d, batch_size=16, dtype=torch.float32)

    def step_logits():
        with torch.no_grad():
            dec_g.prefill(text)
            dec_e.prefill(text)
            snap = dec_g._snapshot()
            got = dec_g._graph_step(token).clone()
            dec_g._restore(snap)
            return got, dec_e.step(token)

    def images():
        torch.manual_seed(7)
        got = dec_g.generate(text, temperature=1e-8, filter_thres=0.99)
        torch.manual_seed(7)
        return got, dec_e.generate(text, temperature=1e-8, filter_thres=0.99)

    # step graph first, then the token graph through generate() ...
    got, want = step_logits()
    assert torch.allclose(got, want, atol=1e-3), (got - want).abs().max().item()
    got, want = images()
    assert torch.allclose(got, want, atol=1e-3), (got - want).abs().max().item()
    # ... then the other way round, with the token graph still alive
    got, want = step_logits()
    assert torch.allclose(got, want, atol=1e-3), (got - want).abs().max().item()
    assert dec_g._step_graph is not None and dec_g._token_graph is not None
    assert dec_g._step_graph[0] is not dec_g._token_graph[0]
    got, want = images()
    assert torch.allclose(got, want, atol=1e-3), (got - want).abs().max().item()
