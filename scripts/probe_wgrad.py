"""Weight-gradient GEMM probe: today's `do2.t() @ x2` (+ the fp32 cast)
against the split-K op at S in {1..32}, and the partial-sum reduce alone, at
the flagship shapes (M = 81920 rows, bf16). Every tensor comes from a pool
larger than the 256 MB MALL and the pool rotates per call, so no variant is
flattered by replaying one cached buffer. Device-event timing.

The constants of ops/fp8.py:wgrad_splits come from this script's output
(profiles/probe_wgrad.txt)."""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import torch
from dalle_pytorch_amd.ops.dispatch import hip_module

assert hip_module() is not None, 'extension not built'
OPS = torch.ops.dalle_amd
MALL = 256 << 20
ROWS = 81920
SPLITS = (1, 2, 4, 8, 16, 32)
SHAPES = (('ff1', ROWS, 8192, 1024), ('ff2', ROWS, 1024, 4096),
          ('qkv', ROWS, 3072, 1024), ('out', ROWS, 1024, 1024),
          ('head-text', ROWS, 10256, 1024), ('head-img', ROWS, 8192, 1024),
          # the CE-head slices at the row counts config C gives them
          ('head-text (its rows)', 64 * 257, 10256, 1024),
          ('head-img (its rows)', 64 * 1023, 8192, 1024))


def timeit(fn, pool, iters=30, warm=6):
    """fn(i) on pool entry i, rotating -> us per call (device events)."""
    for i in range(warm):
        fn(i % pool)
    beg, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    torch.cuda.synchronize()
    beg.record()
    for i in range(iters):
        fn(i % pool)
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters * 1e3


def pool_size(nbytes):
    return max(3, -(-(MALL * 5 // 4) // nbytes))


def try_time(fn, pool):
    try:
        return timeit(fn, pool)
    except RuntimeError as e:
        # a host-side rejection (e.g. bmm.dtype unsupported) is a result;
        # a device error ends the probe
        if 'HIP error' in str(e) or 'illegal' in str(e):
            raise
        return str(e).split('\n')[0][:60]


def fmt(us, flops):
    if isinstance(us, str):
        return f'REJECTED ({us})'
    return f'{us:7.0f}us {flops / us / 1e6:5.0f}TF'


print(f'device {torch.cuda.get_device_name(0)}, torch {torch.__version__}, '
      f'M = {ROWS} unless stated, bf16, pool > {MALL >> 20} MB, '
      f'30 iters after 6 warm-up')
for tag, M, n, k in SHAPES:
    P = pool_size(M * (n + k) * 2)
    do = [torch.randn(M, n, device='cuda').bfloat16() for _ in range(P)]
    x = [torch.randn(M, k, device='cuda').bfloat16() for _ in range(P)]
    flops = 2 * M * n * k
    print(f'\n{tag}: dW [{n} x {k}] over {M} rows, operand pool of {P}')
    a0 = timeit(lambda i: do[i].t() @ x[i], P)
    a1 = timeit(lambda i: (do[i].t() @ x[i]).to(torch.float32), P)
    print(f'  (a) do2.t() @ x2            {fmt(a0, flops)}   '
          f'+ .to(float32) {fmt(a1, flops)}')
    for S in SPLITS:
        f32 = try_time(lambda i: OPS.wgrad_splitk(do[i], x[i], S,
                                                  torch.float32), P)
        b16 = try_time(lambda i: OPS.wgrad_splitk(do[i], x[i], S,
                                                  torch.bfloat16), P)
        gain = '' if isinstance(f32, str) else f'  vs (a)+cast {a1 / f32:4.2f}x'
        print(f'  (b) S={S:2d} fp32 partials -> fp32 {fmt(f32, flops)}   '
              f'-> bf16 {fmt(b16, flops)}{gain}')
    del do, x
    if M != ROWS:       # the reduce does not depend on the row count
        continue
    for S in SPLITS[1:]:
        W = pool_size(S * n * k * 4)
        ws = [torch.randn(S, n, k, device='cuda') for _ in range(W)]
        for dt in (torch.float32, torch.bfloat16):
            us = timeit(lambda i: OPS.wgrad_reduce(ws[i], dt), W)
            moved = n * k * (4 * S + ws[0].new_empty(0, dtype=dt).element_size())
            print(f'  (c) reduce alone S={S:2d} -> {str(dt)[6:]:8s} '
                  f'{us:6.1f}us  {moved / us / 1e6:4.2f} TB/s '
                  f'({moved >> 20} MB, pool of {W})')
        del ws
