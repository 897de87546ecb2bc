"""In-tree hipcc build for the gfx950 extension.

Drives hipcc directly (no torch hipify pass — the sources are native HIP)
and drops ``dalle_pytorch_amd/_hip.so`` next to the package so the built
artifact travels with repo snapshots to GPU boxes. Cross-compiles fine on
machines without a GPU.

One object per kernel family, compiled concurrently; a unit is recompiled
when it is older than its source or than any header in this directory.
"""

import os
import subprocess
import sys
import sysconfig
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parents[2]   # dalle_pytorch_amd/
SRC_DIR = Path(__file__).resolve().parent
SOURCES = [SRC_DIR / name for name in (
    'attention.hip', 'decode.hip', 'train_ops.hip', 'wgrad.hip',
    'module.hip')]
OBJ_DIR = SRC_DIR / 'build'                     # ignored by git
OUTPUT = PKG_DIR / '_hip.so'
MAX_JOBS = 16


def _mtime(path):
    return path.stat().st_mtime if path.exists() else 0.0


def toolchain():
    """-> (hipcc path, per-unit compile flags, library search flags)."""
    import torch
    from torch.utils import cpp_extension as ce

    hipcc = str(Path(ce.ROCM_HOME or '/opt/rocm') / 'bin' / 'hipcc')
    abi = '1' if torch._C._GLIBCXX_USE_CXX11_ABI else '0'
    inc = [f'-I{p}' for p in ce.include_paths()]
    inc.append(f"-I{sysconfig.get_paths()['include']}")
    flags = [
        '-O3', '-std=c++17', '--offload-arch=gfx950',
        '-fPIC',
        '-DTORCH_EXTENSION_NAME=_hip',
        '-DTORCH_API_INCLUDE_EXTENSION_H',
        f'-D_GLIBCXX_USE_CXX11_ABI={abi}',
        *ce.COMMON_HIP_FLAGS, *ce.COMMON_HIPCC_FLAGS,
        '-DTORCH_HIP_VERSION=' + torch.version.hip.split('.')[0],
        '-Wno-deprecated-declarations', '-Wno-unused-result',
        *inc,
    ]
    return hipcc, flags, [f'-L{p}' for p in ce.library_paths()]


def build(verbose=True, force=False):
    newest_hdr = max((_mtime(h) for h in SRC_DIR.glob('*.h')), default=0.0)
    newest_src = max(newest_hdr, *(_mtime(s) for s in SOURCES))
    # a snapshot may carry the .so without its objects: the .so alone decides
    if not force and _mtime(OUTPUT) > newest_src:
        if verbose:
            print(f'[build] {OUTPUT.name} up to date')
        return str(OUTPUT)
    objs = [OBJ_DIR / (s.stem + '.o') for s in SOURCES]
    stale = [(s, o) for s, o in zip(SOURCES, objs)
             if force or _mtime(o) <= max(_mtime(s), newest_hdr)]

    hipcc, flags, libdirs = toolchain()

    def compile_unit(pair):
        src, obj = pair
        tmp = obj.with_suffix('.tmp.o')     # a killed hipcc leaves no fresh .o
        cmd = [hipcc, *flags, '-c', str(src), '-o', str(tmp)]
        if verbose:
            print('[build]', ' '.join(cmd), flush=True)
        t0 = time.time()
        res = subprocess.run(cmd, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True)
        if res.returncode == 0:
            tmp.replace(obj)
        return src.name, res, time.time() - t0

    if stale:
        OBJ_DIR.mkdir(exist_ok=True)
        jobs = min(len(stale), MAX_JOBS, os.cpu_count() or 1)
        with ThreadPoolExecutor(max_workers=jobs) as pool:
            results = list(pool.map(compile_unit, stale))
        for name, res, secs in results:
            if verbose or res.returncode != 0:
                print(f'[build] {name}: exit {res.returncode}, {secs:.0f} s\n'
                      f'{res.stdout}', end='', flush=True)
        failed = [name for name, res, _ in results if res.returncode != 0]
        if failed:
            raise RuntimeError('hipcc failed for ' + ', '.join(failed))

    cmd = [
        hipcc, '--offload-arch=gfx950', '-fPIC', '-shared',
        *[str(o) for o in objs], *libdirs,
        '-ltorch', '-ltorch_cpu', '-ltorch_hip', '-lc10', '-lc10_hip',
        '-ltorch_python', '-lamdhip64',
        '-o', str(OUTPUT),
    ]
    if verbose:
        print('[build]', ' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return str(OUTPUT)


if __name__ == '__main__':
    build(force='--force' in sys.argv)
