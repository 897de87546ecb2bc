"""Source layout of the HIP extension and the Python surface it exports.

CPU-only: the build list must match the directory, and the bindings (names
and the keyword defaults callers rely on) are read from the docstring
signatures pybind generates, which needs the built extension but no GPU.
"""

import importlib
import re

import pytest

from dalle_pytorch_amd.ops.hip import build as hip_build

EXPORTS = {
    'resls_fwd', 'resls_bwd', 'quant_fp8', 'sample_topk_gumbel', 'amax_bf16',
    'sk2', 'dec_prelude', 'permlane_probe', 'fa_fwd', 'fa_bwd',
    'rope_split_fwd', 'rope_split_bwd', 'token_shift', 'fa_decode',
    'shift_decode', 'ln_fwd', 'ln_bwd', 'geglu_fwd', 'geglu_bwd',
    'geglu_bwd_colsum', 'ln_shift_fwd', 'ln_shift_bwd', 'rev_replay',
    'mfma_probe',
}

# binding -> {keyword: default as pybind prints it}
DEFAULTS = {
    'fa_fwd': {'ax_t': '0', 'ax_S': '0', 'ax_axis': '-1'},
    'fa_bwd': {'grad_lse': 'None', 'ax_t': '0', 'ax_S': '0', 'ax_axis': '-1'},
    'sk2': {'wscale': '1.0'},
    'ln_shift_bwd': {'dres': 'None', 'text_len': '0', 'image_size': '0'},
    'sample_topk_gumbel': {'out_tok': 'None', 'seq': 'None',
                           'seq_ptr': 'None'},
}


@pytest.fixture(scope='module')
def ext():
    try:
        return importlib.import_module('dalle_pytorch_amd._hip')
    except ImportError as e:
        pytest.skip(f'extension not built: {e}')


def test_sources_match_directory():
    on_disk = sorted(hip_build.SRC_DIR.glob('*.hip'))
    assert on_disk, 'no HIP sources found'
    assert set(on_disk) <= set(hip_build.SOURCES)
    for src in hip_build.SOURCES:
        assert src.exists(), src


def test_monolith_is_gone():
    assert not (hip_build.SRC_DIR / 'hip_ops.hip').exists()


def test_exports(ext):
    assert {n for n in dir(ext) if not n.startswith('_')} == EXPORTS


@pytest.mark.parametrize('name', sorted(DEFAULTS))
def test_keyword_defaults(ext, name):
    sig = getattr(ext, name).__doc__.split('\n')[0]
    assert sig.startswith(name + '(')
    for kw, default in DEFAULTS[name].items():
        assert re.search(rf'\b{kw}: [^,)]* = {re.escape(default)}[,)]', sig), \
            f'{name}: {kw} = {default} not in "{sig}"'
