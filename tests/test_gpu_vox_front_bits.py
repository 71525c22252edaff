"""The output bits of the three point-cloud front ends -- pcp_voxelize (+ pcp_voxelize_sort_pillar_rows), pcp_pillarise_rows +
pcp_pillar_index_export, pcp_hard_voxelize (+ gather) and pcp_mean_vfe (+ features), which share csrc/vox_front.h -- against
tests/golden/vox_front_bits.json, which tests/golden/make_vox_front_bits.py recorded with the library of the commit the file names.  The
other tests of these entry points compare each with a CPU reference; this file compares every pinned output buffer with its own earlier
self, and the recorder runs every launch twice and demands the same bits of both runs."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
with open(os.path.join(GOLDEN, 'vox_front_bits.json')) as _f:
    PINNED = json.load(_f)
_got = {}


def _recorder():
    spec = importlib.util.spec_from_file_location('make_vox_front_bits', os.path.join(GOLDEN, 'make_vox_front_bits.py'))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec


def _recorded():
    """every launch of the recorder, run once for the whole file"""
    if not _got:
        _got.update(_recorder().record())
    return _got


def test_the_generator_meets_the_conditions_it_asserts():
    """no GPU: the seeded cloud holds every condition the pinned cases rest on (cloud() asserts them)"""
    rec = _recorder()
    pts = rec.cloud()
    assert pts.shape[1] == 1 + rec.NUM_RAW and pts.shape[0] % 1024 != 0 and pts.dtype.name == 'float32'


@pytest.mark.gpu
def test_the_recorder_runs_the_launches_the_file_pins():
    assert sorted(_recorded()) == sorted(PINNED['sha256'])
    # voxelize: coords, unq_inv, unq_cnt, counters, sorted bucket order | rows + export: 3 | hard voxels: 4 | mean VFE: 3
    assert len(PINNED['sha256']) == 5 + 3 + 4 + 3


@pytest.mark.gpu
@pytest.mark.parametrize('key', sorted(PINNED['sha256']))
def test_vox_front_output_bits_are_those_of_the_recorded_commit(key):
    assert _recorded()[key] == PINNED['sha256'][key], 'bits differ from commit %s' % PINNED['recorded_at_commit']
