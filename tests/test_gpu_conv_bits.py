"""The output bits of the direct, F(2x2), through-memory F(4x4), bf16x3 and bf16 convolutions, the pointwise families, both weight-gradient
families and the fused point head against tests/golden/conv_bits.json, which tests/golden/make_conv_bits.py recorded with the library of
the commit the file names.  The tolerance tests of these kernels compare with a reference; this file compares every kernel with its own
earlier self, and the recorder runs every launch twice and demands the same bits of both runs."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
with open(os.path.join(GOLDEN, 'conv_bits.json')) as _f:
    PINNED = json.load(_f)
_got = {}


def _recorded(lib_option):
    """every launch of the recorder, run once for the whole file"""
    if not _got:
        spec = importlib.util.spec_from_file_location('make_conv_bits', os.path.join(GOLDEN, 'make_conv_bits.py'))
        rec = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(rec)
        _got.update(rec.record(lib_option))
    return _got


def test_the_recorder_runs_the_launches_the_file_pins(lib_option):
    assert sorted(_recorded(lib_option)) == sorted(PINNED['sha256'])
    # per map: 3 + 3 direct, 3 pointwise, 3 F(2x2), 1 F(4x4), 4 bf16 | 2 + 2 + 3 of the bf16 training family; 2 point heads;
    # (3 + 1) x 2 fp32 and (2 + 1) x 2 bf16 pointwise weight gradients; 4 fp32 3x3 weight gradients
    assert len(PINNED['sha256']) == 2 * (17 + 7) + 2 + 8 + 6 + 4


@pytest.mark.parametrize('key', sorted(PINNED['sha256']))
def test_conv_output_bits_are_those_of_the_recorded_commit(key, lib_option):
    assert _recorded(lib_option)[key] == PINNED['sha256'][key], 'bits differ from commit %s' % PINNED['recorded_at_commit']
