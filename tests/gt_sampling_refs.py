"""Shared by tests/test_gt_sampler_cpu.py and tests/test_gpu_gt_sampling.py: the fixture tests/golden/g27_gt_sampling.npz (the reference's
own DataBaseSampler, made by tests/golden/make_golden_gt_sampling.py), loaded once and left unchanged."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = 'g27_gt_sampling.npz'


def load_fixture():
    z = np.load(os.path.join(GOLDEN, FIXTURE), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    meta = json.loads(str(d.pop('meta_json')))
    return d, meta


def case_arrays(d, name):
    pre = name + '/'
    return {k[len(pre):]: v for k, v in d.items() if k.startswith(pre)}


def database_of(c, info, device):
    from pcp_amd.gt_sampler import DeviceGtDatabase
    return DeviceGtDatabase(info['db_names'], c['db_boxes'], c['db_counts'], c['db_velo'], c['db_instance_tf'], c['db_points'], device=device)


def sampler_of(c, info, device, cfg=None):
    from pcp_amd.gt_sampler import DeviceGtSampler
    return DeviceGtSampler(cfg or info['sampler_cfg'], info['classes'], database_of(c, info, device))


def drawn_of(sampler, info, key='candidates'):
    """the fixture's recorded candidates in the form DeviceGtSampler.draw() returns them"""
    return [{'n_own': n, 'groups': [np.asarray(cands.get(g['name'], []), dtype=np.int64) for g in sampler.groups]}
            for n, cands in zip(info['n_own'], info[key])]
