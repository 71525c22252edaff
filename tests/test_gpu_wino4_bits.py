"""The output bits of the fused F(4x4, 3x3) kernels (k_wino4f, k_wino4h, k_wino4c) against tests/golden/wino4_bits.json, which
tests/golden/make_wino4_bits.py recorded with the library of the commit the file names.  test_wino4c_gives_the_bits_of_wino4h compares two
kernels of one build; this file compares every kernel with its own earlier self, so a rework that moves them together is seen too."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
with open(os.path.join(GOLDEN, 'wino4_bits.json')) as _f:
    PINNED = json.load(_f)
_got = {}


def _recorded(lib_option):
    """every launch of the recorder, run once for the whole file"""
    if not _got:
        spec = importlib.util.spec_from_file_location('make_wino4_bits', os.path.join(GOLDEN, 'make_wino4_bits.py'))
        rec = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(rec)
        _got.update(rec.record(lib_option))
    return _got


def test_the_recorder_runs_the_launches_the_file_pins(lib_option):
    assert sorted(_recorded(lib_option)) == sorted(PINNED['sha256'])
    # 6 cases x ReLU off / on x (k_wino4f, k_wino4h, k_wino4c with wino4c_nw 4 and 8) + the channel-window launch of each
    assert len(PINNED['sha256']) == 6 * 2 * 4 + 4


@pytest.mark.parametrize('key', sorted(PINNED['sha256']))
def test_fused_f4_output_bits_are_those_of_the_recorded_commit(key, lib_option):
    assert _recorded(lib_option)[key] == PINNED['sha256'][key], 'bits differ from commit %s' % PINNED['recorded_at_commit']
