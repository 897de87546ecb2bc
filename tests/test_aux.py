"""Auxiliary subsystems: tar streaming, conversion mapping, flops profiler,
rainbow convergence, bench distributed launch and output dump."""

import io
import json
import os
import subprocess
import sys
import tarfile
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))


def _make_shard(path, n, size=32):
    from dalle_pytorch_amd.utils.vision import tensor_to_pil
    with tarfile.open(path, 'w') as tf:
        for i in range(n):
            img = tensor_to_pil(torch.rand(3, size, size))
            buf = io.BytesIO()
            img.save(buf, format='PNG')
            data = buf.getvalue()
            info = tarfile.TarInfo(f'{i:06d}.png')
            info.size = len(data)
            tf.addfile(info, io.BytesIO(data))
            cap = f'sample number {i}'.encode()
            info = tarfile.TarInfo(f'{i:06d}.txt')
            info.size = len(cap)
            tf.addfile(info, io.BytesIO(cap))


def test_tar_streaming_dataset(tmp_path):
    from dalle_pytorch_amd.utils.wds import TarImageTextDataset, expand_shards
    from dalle_pytorch_amd.utils.tokenizer import SimpleTokenizer
    for s in range(2):
        _make_shard(tmp_path / f'shard-{s:03d}.tar', 5)

    assert len(expand_shards(str(tmp_path / 'shard-{000..001}.tar'))) == 2
    assert len(expand_shards(str(tmp_path / '*.tar'))) == 2

    ds = TarImageTextDataset(str(tmp_path / '*.tar'),
                             tokenizer=SimpleTokenizer(), text_len=16,
                             image_size=32)
    samples = list(ds)
    assert len(samples) == 10
    tokens, image = samples[0]
    assert tokens.shape == (16,) and image.shape == (3, 32, 32)

    from torch.utils.data import DataLoader
    dl = DataLoader(ds, batch_size=4, drop_last=True)
    batch = next(iter(dl))
    assert batch[0].shape == (4, 16) and batch[1].shape == (4, 3, 32, 32)


def test_tar_dataset_repeats_shards_when_fewer_than_ranks(tmp_path, monkeypatch):
    """1 shard, 2 ranks: rank 1 must still yield data (a zero-batch rank
    stalls the other ranks' gradient all-reduce forever)."""
    from dalle_pytorch_amd.utils import wds as wds_mod
    from dalle_pytorch_amd.utils.tokenizer import SimpleTokenizer
    _make_shard(tmp_path / 'shard-000.tar', 3)
    ds = wds_mod.TarImageTextDataset(str(tmp_path / '*.tar'),
                                     tokenizer=SimpleTokenizer(), text_len=16,
                                     image_size=32)
    import dalle_pytorch_amd.parallel as par
    monkeypatch.setattr(par, 'get_world_size', lambda: 2)
    for rank in (0, 1):
        monkeypatch.setattr(par, 'get_rank', lambda r=rank: r)
        with pytest.warns(RuntimeWarning, match='repeating shards'):
            assert len(ds._my_shards()) >= 1
        assert len(list(ds)) == 3


def test_vqgan_downsample_matches_taming_asymmetric_pad():
    """taming pads (0,1,0,1) with a padding=0 stride-2 conv; a symmetric
    padding=1 conv is spatially shifted and decodes real ckpts wrong."""
    import torch.nn.functional as F
    from dalle_pytorch_amd.models.vae_adapters import _VqDownsample
    ds = _VqDownsample(4)
    x = torch.randn(2, 4, 16, 16)
    want = F.conv2d(F.pad(x, (0, 1, 0, 1)), ds.conv.weight, ds.conv.bias, stride=2)
    assert torch.allclose(ds(x), want)
    # and it must differ from the symmetric-pad variant on generic input
    sym = F.conv2d(x, ds.conv.weight, ds.conv.bias, stride=2, padding=1)
    assert ds(x).shape == sym.shape and not torch.allclose(ds(x), sym)


def test_vqgan_gumbel_proj_consumed_and_rejects_mismatch(tmp_path):
    from dalle_pytorch_amd import VQGanVAE
    g = VQGanVAE(image_size=32, num_tokens=128, embed_dim=16, ch=16,
                 ch_mult=(1, 2), num_res_blocks=1, gumbel=True)
    sd = g.state_dict()
    assert 'quantize.proj.weight' in sd  # taming GumbelQuantize layout
    ck = tmp_path / 'g.ckpt'
    torch.save({'state_dict': sd}, ck)
    # round-trips into a fresh gumbel module
    g2 = VQGanVAE(vqgan_model_path=str(ck), image_size=32, num_tokens=128,
                  embed_dim=16, ch=16, ch_mult=(1, 2), num_res_blocks=1,
                  gumbel=True)
    img = torch.rand(1, 3, 32, 32)
    assert torch.equal(g.get_codebook_indices(img), g2.get_codebook_indices(img))
    # a gumbel checkpoint must NOT silently load into a non-gumbel module
    with pytest.raises(RuntimeError):
        VQGanVAE(vqgan_model_path=str(ck), image_size=32, num_tokens=128,
                 embed_dim=16, ch=16, ch_mult=(1, 2), num_res_blocks=1,
                 gumbel=False)


def test_openai_dvae_conversion_mapping():
    """Synthesize a dall_e-layout state dict with matching shapes; the
    converter must cover every parameter of our module."""
    sys.path.insert(0, str(REPO / 'scripts'))
    import convert_openai_dvae as conv
    from dalle_pytorch_amd import OpenAIDiscreteVAE

    vae = OpenAIDiscreteVAE(n_hid=32, vocab_size=64)

    def fake_block_state(prefix, block, out):
        import torch.nn as nn
        if isinstance(block.id_path, nn.Conv2d):
            out[f'{prefix}id_path.w'] = torch.randn_like(block.id_path.weight)
            out[f'{prefix}id_path.b'] = torch.randn_like(block.id_path.bias)
        convs = [m for m in block.res_path if isinstance(m, nn.Conv2d)]
        for i, c in enumerate(convs, start=1):
            out[f'{prefix}res_path.conv_{i}.w'] = torch.randn_like(c.weight)
            out[f'{prefix}res_path.conv_{i}.b'] = torch.randn(1, c.out_channels, 1, 1)

    enc, dec = {}, {}
    enc['blocks.input.w'] = torch.randn_like(vae.encoder.input.weight)
    enc['blocks.input.b'] = torch.randn(1, 32, 1, 1)
    for g in range(1, 5):
        for j in range(1, 3):
            fake_block_state(f'blocks.group_{g}.block_{j}.',
                             getattr(vae.encoder, f'group_{g}')[j - 1], enc)
    enc['blocks.output.conv.w'] = torch.randn_like(vae.encoder.output[1].weight)
    enc['blocks.output.conv.b'] = torch.randn(1, 64, 1, 1)

    dec['blocks.input.w'] = torch.randn(16, 64, 1, 1)  # [n_init, vocab, 1, 1]
    for g in range(1, 5):
        for j in range(1, 3):
            fake_block_state(f'blocks.group_{g}.block_{j}.',
                             getattr(vae.decoder, f'group_{g}')[j - 1], dec)
    dec['blocks.output.conv.w'] = torch.randn_like(vae.decoder.output[1].weight)
    dec['blocks.output.conv.b'] = torch.randn(1, 3 * 2, 1, 1)

    state = conv.convert(enc, dec)
    missing, unexpected = vae.load_state_dict(state, strict=False)
    assert not unexpected, unexpected[:5]
    assert not missing, missing[:5]
    # codebook is the transposed decoder input conv
    assert torch.equal(state['codebook.weight'],
                       dec['blocks.input.w'][:, :, 0, 0].t())


def test_flops_profiler_table(capsys):
    from dalle_pytorch_amd import DALLE, DiscreteVAE
    from dalle_pytorch_amd.utils.flops import profile_step
    vae = DiscreteVAE(image_size=64, num_layers=3, num_tokens=64,
                      codebook_dim=32, hidden_dim=8)
    d = DALLE(dim=64, vae=vae, num_text_tokens=100, text_seq_len=8, depth=2,
              heads=2, dim_head=32, attn_types=('full', 'axial_row'),
              shift_tokens=True)
    fl = profile_step(d, batch_size=2, step_time_s=0.1)
    out = capsys.readouterr().out
    assert 'achieved' in out and 'layer0.attn' in out
    assert fl > 0


def test_vqgan_yaml_config(tmp_path):
    import yaml
    from dalle_pytorch_amd import VQGanVAE
    cfg = {'model': {'target': 'taming.models.vqgan.VQModel',
                     'params': {'n_embed': 128, 'embed_dim': 32,
                                'ddconfig': {'ch': 16, 'ch_mult': [1, 2],
                                             'num_res_blocks': 1,
                                             'resolution': 32}}}}
    p = tmp_path / 'cfg.yaml'
    p.write_text(yaml.safe_dump(cfg))
    vae = VQGanVAE(vqgan_config_path=str(p))
    assert vae.num_tokens == 128 and vae.num_layers == 1
    codes = vae.get_codebook_indices(torch.rand(1, 3, 32, 32))
    assert codes.max() < 128


@pytest.mark.slow
def test_rainbow_overfits_cpu():
    """Tiny end-to-end: loss must clearly fall on the compositional data
    (the reference notebook's correctness signal, bounded for CI time)."""
    sys.path.insert(0, str(REPO / 'examples'))
    import train_rainbow
    first, last, acc = train_rainbow.main([
        '--samples', '32', '--vae_steps', '30', '--dalle_steps', '60',
        '--dim', '64', '--depth', '1', '--batch_size', '8'])
    assert last < first * 0.7, (first, last)


def test_bench_distributed_launch_cpu():
    """bench.py tiny config under torch.distributed.run, 2 ranks on CPU
    (gloo): the exact launch shape the driver uses for multi-GPU."""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29701', str(REPO / 'bench.py'),
           '--config', 'tiny', '--steps', '2', '--warmup', '1']
    # hide any GPUs: this is the CPU/gloo launch, and a 1-GPU machine has no
    # device for local rank 1
    env = dict(os.environ, CUDA_VISIBLE_DEVICES='', HIP_VISIBLE_DEVICES='')
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                         cwd=str(REPO), env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [l for l in res.stdout.splitlines() if l.startswith('{')][-1]
    rec = json.loads(line)
    assert rec['n_gpus'] == 2
    assert rec['config']['parallelism'] == 'dp2'
    assert rec['value'] > 0


def test_bench_dump_outputs_cpu(tmp_path):
    """bench.py --dump-outputs: the last timed step's loss lands in
    DIR/loss.npy as float32, identical across two runs with the same
    arguments (seeded weights and data); --steps sets the timed step count
    and the result line carries ms_per_step. --full is accepted."""
    import numpy as np
    env = dict(os.environ, CUDA_VISIBLE_DEVICES='', HIP_VISIBLE_DEVICES='')
    losses = []
    for name, extra in (('a', []), ('b', ['--full'])):
        out = tmp_path / name
        cmd = [sys.executable, str(REPO / 'bench.py'), '--gpus', '1',
               '--config', 'tiny', '--steps', '3', '--warmup', '1',
               '--dump-outputs', str(out), *extra]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                             cwd=str(REPO), env=env)
        assert res.returncode == 0, res.stderr[-2000:]
        rec = json.loads(
            [l for l in res.stdout.splitlines() if l.startswith('{')][-1])
        assert rec['steps'] == 3 and rec['ms_per_step'] > 0
        assert [p.name for p in out.iterdir()] == ['loss.npy']
        loss = np.load(out / 'loss.npy')
        assert loss.dtype == np.float32 and np.isfinite(loss).all()
        losses.append(loss)
    assert np.array_equal(losses[0], losses[1])


def test_weight_caches_reject_recycled_storage():
    """The per-step weight caches (one class, three users: fp8 quant, bf16
    cast, bf16 W^T) key on (data_ptr, shape). A new parameter that lands on
    a freed one's address with the same shape and version must not be served
    the old entry; the same parameter and fresh slices of it must still hit.
    An entry lasts until the parameter's version or the step changes, and a
    full cache empties itself."""
    from dalle_pytorch_amd.ops import fp8
    users = (fp8._quant_weight, fp8._bf16_weight, fp8._transposed_weight)
    assert all(type(u) is fp8._StepCache for u in users)
    assert len({id(u.entries) for u in users}) == 3

    made = []

    def make(w):
        made.append(w)
        return w.detach().to(torch.bfloat16).t().contiguous()

    cache = fp8._StepCache(make)
    p = torch.nn.Parameter(torch.randn(32, 16))
    assert cache(p) is cache(p)
    assert cache(p[:16]) is cache(p[:16])
    assert len(made) == 2
    # what address reuse produces: q's key maps to the entry p left behind
    q = torch.nn.Parameter(torch.randn(32, 16))
    cache.entries[(q.data_ptr(), tuple(q.shape))] = \
        cache.entries[(p.data_ptr(), tuple(p.shape))]
    qb = q.detach().to(torch.bfloat16)
    assert torch.equal(cache(q), qb.t())
    assert len(made) == 3 and cache(q) is cache(q)

    # a version bump misses, and so does the step mark
    hit = cache(p)
    with torch.no_grad():
        p.add_(1)
    bumped = cache(p)
    assert bumped is not hit
    assert torch.equal(bumped, p.detach().to(torch.bfloat16).t())
    fp8.fp8_mark_step()
    assert cache(p) is not bumped and cache(p) is cache(p)

    # the bound: 512 entries stay, the 513th insert clears the rest
    cache = fp8._StepCache(lambda w: w.detach().clone())
    params = [torch.nn.Parameter(torch.zeros(1)) for _ in range(513)]
    for w in params[:512]:
        cache(w)
    assert len(cache.entries) == 512
    cache(params[512])
    assert len(cache.entries) == 1 and cache(params[512]) is cache(params[512])


def test_gpu_tensor_without_extension_is_loud(monkeypatch):
    """Dispatch policy: a GPU tensor with the extension missing raises from
    every eligibility predicate instead of quietly choosing the eager route;
    DALLE_AMD_ALLOW_EAGER=1 turns that into a plain 'not supported'."""
    from types import SimpleNamespace
    from dalle_pytorch_amd.ops import dispatch
    from dalle_pytorch_amd.ops.fused import (layer_norm_fused,
                                              token_shift_supported)
    from dalle_pytorch_amd.ops.rope import rope_split_supported
    monkeypatch.setattr(dispatch, '_TRIED', True)
    monkeypatch.setattr(dispatch, '_HIP', None)
    x = SimpleNamespace(is_cuda=True, dtype=torch.bfloat16, shape=(2, 8, 512),
                        element_size=lambda: 2)
    checks = (lambda: token_shift_supported(x),
              lambda: rope_split_supported(x, 64),
              lambda: layer_norm_fused(x))
    monkeypatch.delenv('DALLE_AMD_ALLOW_EAGER', raising=False)
    for check in checks:
        with pytest.raises(RuntimeError, match='is not built'):
            check()
    monkeypatch.setenv('DALLE_AMD_ALLOW_EAGER', '1')
    assert not any(check() for check in checks)


def test_clip_train_and_rerank(tmp_path):
    """CLIP example trains (loss falls) and the saved checkpoint loads for
    re-ranking."""
    sys.path.insert(0, str(REPO / 'examples'))
    import train_clip
    out = tmp_path / 'clip.pt'
    first, last = train_clip.main(['--steps', '40', '--dim', '64',
                                   '--depth', '1', '--batch_size', '16',
                                   '--out', str(out)])
    assert last < first
    from dalle_pytorch_amd.utils.checkpoint import load_clip_checkpoint
    clip, _ = load_clip_checkpoint(out)
    text = torch.randint(0, 100, (4, 16))
    imgs = torch.rand(4, 3, 32, 32)
    scores = clip(text, imgs)
    assert scores.shape == (4,)
