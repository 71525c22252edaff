"""The host side of the SECOND ops against the call table recorded before their two count forms were given one body each
(tests/golden/make_second_ops_calls.py -> second_ops_calls.json): every C call with its scalars and the place of every pointer, every returned
shape, every DevBuffers size, every host read and every exception text, row by row.  No GPU: the library is a fake for the duration."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _recorder():
    spec = importlib.util.spec_from_file_location('make_second_ops_calls', os.path.join(GOLDEN, 'make_second_ops_calls.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def tables():
    with open(os.path.join(GOLDEN, 'second_ops_calls.json')) as f:
        want = json.load(f)['rows']
    return want, _recorder().record()


def test_every_row_of_the_call_table(tables):
    want, got = tables
    assert sorted(got) == sorted(want)
    wrong = [key for key in sorted(want) if got[key] != want[key]]
    for key in wrong[:5]:
        print('%s\n  recorded: %s\n  now:      %s' % (key, json.dumps(want[key]), json.dumps(got[key])))
    assert not wrong, '%d of %d rows differ, the first: %s' % (len(wrong), len(want), wrong[:5])


def test_the_table_holds_what_it_is_for(tables):
    """the recording itself: both forms of the five pairs, the refusals, and the reads of each form"""
    want, _ = tables
    for op in ('mean_vfe', 'spconv_table', 'spconv_build_subm', 'spconv_build_strided', 'spconv3d'):
        for form in (op, op + '_dev'):
            mine = [row for key, row in want.items() if key.split(' ')[0] == form]
            assert len(mine) >= 6 and any('raises' not in row for row in mine), form
            if form != 'spconv_build_subm' and form != 'spconv_build_subm_dev':
                assert any('raises' in row for row in mine), form
            if form.endswith('_dev'):
                assert all(row['reads'] == 0 for row in mine), form
    assert want['mean_vfe n=17']['reads'] == 1 and want['spconv_build_strided s2 n=17']['reads'] == 1
    assert want['spconv_table n=17 check_input=True']['reads'] == 1 and want['spconv_table bad flag, check_input=False']['reads'] == 0
    assert want['layers n=17 host counts trusted_indices=False']['reads'] == 2 and want['layers n=17 host counts trusted_indices=True']['reads'] == 1
    first, second = (want['layers n=17 device counts row_capacity None forward %d' % i] for i in (1, 2))
    assert first['bufs'] == second['bufs'] and first['reads'] == second['reads'] == 0
    assert any('status+16' in call for call in first['calls'])


def test_the_fakes_are_gone_afterwards(tables):
    import torch
    from pcp_amd import lib, ops
    assert ops._need_cuda.__module__ == 'pcp_amd.ops' and lib.load.__module__ == 'pcp_amd.lib' and ops._stream.__module__ == 'pcp_amd.ops'
    assert torch.Tensor.tolist.__name__ == 'tolist' and torch.Tensor.item.__name__ == 'item'
