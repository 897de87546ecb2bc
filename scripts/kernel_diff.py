#!/usr/bin/env python
"""Compare the compiled gfx950 kernels of two versions of the HIP sources.

    python scripts/kernel_diff.py --a OLD_TREE --b NEW_TREE
    python scripts/kernel_diff.py --a old.s --b attention.s decode.s ...

Each side is a source tree (a checkout of this repository; every *.hip under
dalle_pytorch_amd/ops/hip is compiled to device assembly with build.py's
flags plus --cuda-device-only -S) or a list of device-assembly files. Whole
units are compiled, host code included, because template kernels are only
instantiated by their host launches. Both trees are compiled with the flags
of THIS checkout's build.py (an older tree may have no toolchain() to ask),
so a change of flags between the two trees goes unseen here.

Per kernel symbol the tool reports whether the instruction text and the
kernel descriptor block (.amdhsa_* : registers, LDS, scratch, occupancy
hints) are equal, and lists kernels present on one side only. Only what a
move between files changes is normalised away: comments and the function
number in local basic-block labels (.LBB<n>_<m>). Exit status 1 on any
difference, so a refactor can be gated on it.
"""

import argparse
import importlib.util
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HIP_DIR = Path('dalle_pytorch_amd') / 'ops' / 'hip'
REPO = Path(__file__).resolve().parents[1]


def toolchain():
    spec = importlib.util.spec_from_file_location(
        '_hip_build', REPO / HIP_DIR / 'build.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hipcc, flags, _ = mod.toolchain()
    return hipcc, flags


def emit_asm(tree, outdir, jobs):
    srcs = sorted((tree / HIP_DIR).glob('*.hip'))
    if not srcs:
        sys.exit(f'no *.hip under {tree / HIP_DIR}')
    hipcc, flags = toolchain()

    def one(src):
        out = outdir / (src.stem + '.s')
        subprocess.run([hipcc, *flags, '--cuda-device-only', '-S',
                        str(src), '-o', str(out)], check=True)
        return out

    with ThreadPoolExecutor(max_workers=min(jobs, len(srcs))) as pool:
        return list(pool.map(one, srcs))


def norm(line):
    line = line.split(';', 1)[0].strip()
    return re.sub(r'\.LBB\d+_', '.LBB_', line)


def kernels(asm_files):
    """-> {symbol: (instruction lines, descriptor lines)}"""
    bodies, descs = {}, {}
    for path in asm_files:
        lines = Path(path).read_text().split('\n')
        i = 0
        while i < len(lines):
            m = re.match(r'\s*\.type\s+(\S+),@function', lines[i])
            if m:
                name, body = m.group(1), []
                i += 1
                while i < len(lines) and not re.match(
                        r'\.Lfunc_end\d+:|\s*\.section\b', lines[i]):
                    text = norm(lines[i])
                    if text and text != name + ':':
                        body.append(text)
                    i += 1
                bodies[name] = body
                continue
            m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', lines[i])
            if m:
                name, desc = m.group(1), []
                i += 1
                while not lines[i].strip().startswith('.end_amdhsa_kernel'):
                    desc.append(norm(lines[i]))
                    i += 1
                descs[name] = desc
            i += 1
    empty = [k for k in descs if not bodies.get(k)]
    if empty:       # two unparsed bodies would otherwise compare as equal
        sys.exit('no instruction text found for: ' + ', '.join(empty))
    return {k: (bodies[k], d) for k, d in descs.items()}


def side(paths, tmp, tag, jobs):
    if len(paths) == 1 and Path(paths[0]).is_dir():
        out = Path(tmp) / tag
        out.mkdir(exist_ok=True)
        paths = emit_asm(Path(paths[0]).resolve(), out, jobs)
    return kernels(paths)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--a', nargs='+', required=True,
                    help='source tree, or device-assembly files')
    ap.add_argument('--b', nargs='+', required=True)
    ap.add_argument('--jobs', type=int, default=8)
    ap.add_argument('--keep', metavar='DIR',
                    help='keep the emitted assembly under DIR/a and DIR/b')
    ap.add_argument('--quiet', action='store_true',
                    help='print only differences and the summary')
    args = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        if args.keep:
            tmp = args.keep
            Path(tmp).mkdir(parents=True, exist_ok=True)
        a = side(args.a, tmp, 'a', args.jobs)
        b = side(args.b, tmp, 'b', args.jobs)

    both = sorted(a.keys() & b.keys())
    differ = 0
    for name in both:
        text_eq, desc_eq = a[name][0] == b[name][0], a[name][1] == b[name][1]
        differ += not (text_eq and desc_eq)
        if not args.quiet or not (text_eq and desc_eq):
            print(f'{"equal" if text_eq else "DIFFER":7s} text  '
                  f'{"equal" if desc_eq else "DIFFER":7s} descriptor  {name}')
    only_a, only_b = sorted(a.keys() - b.keys()), sorted(b.keys() - a.keys())
    for name in only_a:
        print(f'only in A: {name}')
    for name in only_b:
        print(f'only in B: {name}')
    print(f'{len(a)} kernels in A, {len(b)} in B: {len(both) - differ} equal, '
          f'{differ} differ, {len(only_a)} only in A, {len(only_b)} only in B')
    return 1 if differ or only_a or only_b else 0


if __name__ == '__main__':
    sys.exit(main())
