"""The output bits of the CenterHead training kernels -- pcp_centerhead_targets / _loss and pcp_centerhead_targets_ext / _loss_ext, which
share one statement of their arithmetic in csrc/loss.hip -- against tests/golden/centerhead_train_bits.json, which
tests/golden/make_centerhead_train_bits.py recorded with the library of the commit the file names.  The tolerance tests of these kernels
(test_gpu_loss.py, test_gpu_train_ops.py, test_gpu_nusc_head_train.py) compare each family with a reference; this file compares every
output buffer with its own earlier self, and the recorder runs every launch twice and demands the same bits of both runs."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
with open(os.path.join(GOLDEN, 'centerhead_train_bits.json')) as _f:
    PINNED = json.load(_f)
_got = {}


def _recorder():
    spec = importlib.util.spec_from_file_location('make_centerhead_train_bits', os.path.join(GOLDEN, 'make_centerhead_train_bits.py'))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return rec


def _recorded():
    """every launch of the recorder, run once for the whole file"""
    if not _got:
        _got.update(_recorder().record())
    return _got


def test_the_generators_meet_the_conditions_they_assert():
    """no GPU: the seeded inputs hold every condition the pinned cases rest on (the generators assert them)"""
    rec = _recorder()
    assert rec.targets_case().shape == (2, 300, 10)
    _shape, heads = rec.loss_ext_case()
    assert [len(h['reg_ch']) for h in heads] == [8, 11]
    assert sorted(rec.loss_one_cases()) == ['many blocks', 'one block', 'one block nan']


@pytest.mark.gpu
def test_the_recorder_runs_the_launches_the_file_pins():
    assert sorted(_recorded()) == sorted(PINNED['sha256'])
    # targets: 4 buffers of the one head, 2 x 2 heads x 4 of the ext forms | ext loss: losses, total (+ 2 dhead) | one-head loss: 3 x (losses, dhead)
    assert len(PINNED['sha256']) == 4 + 16 + (4 + 2) + 6


@pytest.mark.gpu
@pytest.mark.parametrize('key', sorted(PINNED['sha256']))
def test_centerhead_train_output_bits_are_those_of_the_recorded_commit(key):
    assert _recorded()[key] == PINNED['sha256'][key], 'bits differ from commit %s' % PINNED['recorded_at_commit']
