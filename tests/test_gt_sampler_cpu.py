"""Host side of the device gt_sampling (pcp_amd/gt_sampler.py), no GPU: draw() reproduces the candidates the reference's
sample_with_fixed_number returned (tests/golden/g27_gt_sampling.npz: pointer / permutation state machine, short slices included), the
config is parsed and refused like the issue says, and DeviceWorldAugmentor(gt_sampler=...) interleaves the sampler's draws with the
world draws the way the reference's DataAugmentor.forward consumes numpy's generator."""
import logging

import numpy as np
import pytest

import gt_sampling_refs as gr
from pcp_amd import lib
from pcp_amd.augment import DeviceWorldAugmentor
from pcp_amd.gt_sampler import DeviceGtSampler

D, META = gr.load_fixture()
CASES = list(META['cases'])


def _classes(c, info):
    W = info['W']
    return [c['gt_boxes'][b, :n, W - 1].astype(np.int64) for b, n in enumerate(info['n_own'])]


@pytest.mark.parametrize('name', CASES)
def test_draw_reproduces_the_candidates_the_reference_drew(name):
    info = META['cases'][name]
    c = gr.case_arrays(D, name)
    s = gr.sampler_of(c, info, None)
    rng = np.random.RandomState(info['seed'])
    want = gr.drawn_of(s, info)
    short = 0
    for b, cls in enumerate(_classes(c, info)):
        got = s.draw(cls, rng)
        assert got['n_own'] == info['n_own'][b]
        for g, a, w in zip(s.groups, got['groups'], want[b]['groups']):
            assert a.tolist() == w.tolist(), (name, b, g['name'])
            asked = g['num'] - int((cls == g['class_id']).sum())
            short += 0 < a.size < asked
            assert (g['name'] in info['candidates'][b]) == (asked > 0)
    if name == 's7':
        assert short >= 1 and info['events']['short'] >= 1 and max(info['events']['permutations'].values()) >= 2


def test_fixture_holds_the_listed_events():
    e = META['cases']['s12']['events']
    assert e['vs_original'] >= 1 and e['vs_earlier_class'] >= 1 and e['mutual'] >= 2 and min(e['accepted_per_frame']) >= 1
    s7 = META['cases']['s7']
    assert 0 in s7['n_own'] and 0 in s7['own_rows'] and s7['events']['limit_skips'] >= 1
    big = META['cases']['big']
    first = big['own_rows'][0] + big['added_rows'][0]
    assert big['own_rows'] == [511, 513] and max(big['added_rows']) > 1100 and first % lib.AUG_TILE_ROWS not in (0, 1, lib.AUG_TILE_ROWS - 1)
    assert META['conditioning']['margin'] == 1e-2 and META['tile_rows'] == lib.AUG_TILE_ROWS


def test_config_parsing_prepare_and_refusals(caplog):
    info = META['cases']['s7']
    c = gr.case_arrays(D, 's7')
    db = gr.database_of(c, info, None)
    cfg = dict(info['sampler_cfg'])
    s = DeviceGtSampler(cfg, info['classes'], db)
    assert [g['name'] for g in s.groups] == ['car', 'truck', 'pedestrian'] and s.class_sizes() == {'car': 5, 'truck': 7, 'pedestrian': 3}
    assert [g['pointer'] for g in s.groups] == [5, 7, 3]                   # pointer starts at len(db): the first call permutes
    assert s.inst_col == 1 + 5 + 1 and s.limit_whole_scene
    # classes the model does not have are dropped, the class id is the model's
    s2 = DeviceGtSampler(cfg, ['pedestrian', 'car'], db)
    assert [(g['name'], g['class_id']) for g in s2.groups] == [('car', 2), ('pedestrian', 1)]
    # PREPARE.filter_by_min_points drops records and changes what is drawn
    prep = META['cases']['prep']
    with caplog.at_level(logging.INFO):
        sp = DeviceGtSampler(prep['sampler_cfg'], prep['classes'], db)
    kept = {g['name']: g['members'].tolist() for g in sp.groups}
    assert kept['car'] == [i for i in range(5) if db.counts[i] >= 20] and 0 < len(kept['car']) < 5 and len(kept['pedestrian']) == 3
    assert sum('filter by min points' in r.getMessage() for r in caplog.records) == 2
    # filter_by_difficulty
    db.difficulty = np.asarray([0, 1, 0, 2, 0] + [0] * 10)
    sd = DeviceGtSampler(dict(cfg, PREPARE={'filter_by_difficulty': [1, 2]}), info['classes'], db)
    assert sd.groups[0]['members'].tolist() == [0, 2, 4]
    db.difficulty = None
    # the refusals name their key
    for key, val in (('IMG_AUG_TYPE', 'kitti'), ('USE_ROAD_PLANE', True), ('DATABASE_WITH_FAKELIDAR', True)):
        with pytest.raises(ValueError, match=key):
            DeviceGtSampler(dict(cfg, **{key: val}), info['classes'], db)
    DeviceGtSampler(dict(cfg, USE_ROAD_PLANE=False, IMG_AUG_TYPE=None), info['classes'], db)
    with pytest.raises(ValueError, match='SAMPLE_GROUPS.*car'):
        DeviceGtSampler(dict(cfg, PREPARE={'filter_by_min_points': ['car:1000']}), info['classes'], db)
    with pytest.raises(ValueError, match=str(lib.GTS_MAX_CAND)):
        DeviceGtSampler(dict(cfg, SAMPLE_GROUPS=['car:65']), info['classes'], db)
    many = ['c%d' % i for i in range(17)]
    big_db = gr.database_of(c, dict(info, db_names=(many * 15)[:15]), None)
    with pytest.raises(ValueError, match='17 sample groups.*%d' % lib.GTS_MAX_GROUPS):
        DeviceGtSampler(dict(cfg, SAMPLE_GROUPS=['%s:1' % n for n in many[:15]] + ['c0:1', 'c1:1']), many, big_db)   # 15 stocked classes, 17 entries
    with pytest.raises(ValueError, match='NUM_POINT_FEATURES'):
        DeviceGtSampler(dict(cfg, NUM_POINT_FEATURES=10), info['classes'], db)
    # the per-frame limits of the candidate table, with their numbers
    with pytest.raises(ValueError, match=str(lib.GTS_MAX_BOXES)):
        s.candidate_table([{'n_own': 510, 'groups': [np.arange(3), np.zeros(0, np.int64), np.zeros(0, np.int64)]}], 8, None)
    with pytest.raises(ValueError, match=str(lib.AUG_MAX_BATCH)):
        s.candidate_table([{'n_own': 0, 'groups': [np.zeros(0, np.int64)] * 3}] * (lib.AUG_MAX_BATCH + 1), 8, None)
    with pytest.raises(ValueError, match='tf_target_from_glob'):
        gr.sampler_of(gr.case_arrays(D, 's12'), META['cases']['s12'], None).candidate_table(
            [{'n_own': 0, 'groups': [np.arange(1)] + [np.zeros(0, np.int64)] * 9}], 10, [{}])


def test_candidate_table_maps_the_velocity_like_the_reference():
    info = META['cases']['s12']
    c = gr.case_arrays(D, 's12')
    s = gr.sampler_of(c, info, None)
    meta = [{'tf_target_from_glob': c['tf_target_from_glob'][b]} for b in range(3)]
    ft, cand_db, cand_box, rows = s.candidate_table(gr.drawn_of(s, info), 10, meta)
    assert ft.shape == (3, 12) and ft[:, 0].tolist() == info['n_own'] and ft[-1, -1] == cand_db.size == cand_box.shape[0]
    assert rows == int(c['db_counts'][cand_db].sum())
    b = 1
    for t in range(ft[b, 1], ft[b, 11]):
        want = (c['tf_target_from_glob'][b][:3, :3] @ c['db_velo'][cand_db[t]].reshape(3, 1))[:2, 0].astype(np.float32)
        assert np.array_equal(cand_box[t, 7:9], want) and np.array_equal(cand_box[t, :7], c['db_boxes'][cand_db[t], :7])
        assert cand_box[t, 9] == info['classes'].index(info['db_names'][cand_db[t]]) + 1


def test_augmentor_interleaves_the_sampler_draws_with_the_world_draws():
    """RandomState(s) reproduces DataAugmentor.forward after np.random.seed(s): per frame the sampler's permutations first, then flip x,
    flip y, rotation, scaling -- checked against the reference's record and against a numpy restatement of the call order"""
    info = META['cases']['s12']
    c = gr.case_arrays(D, 's12')
    s = gr.sampler_of(c, info, None)
    aug = DeviceWorldAugmentor(info['aug_cfg'], META['pc_range'], layout='nusc_map', gt_sampler=s)
    assert [n for n, _ in aug.queue] == ['gt_sampling', 'random_world_flip', 'random_world_rotation', 'random_world_scaling'] and aug.skipped == []
    assert aug.stages == [lib.AUG_FLIP_X, lib.AUG_FLIP_Y, lib.AUG_ROTATE, lib.AUG_SCALE]
    classes = _classes(c, info)
    p = aug.draw(3, np.random.RandomState(info['aug_seed']), classes)
    want = gr.drawn_of(s, info, 'aug_candidates')
    for b in range(3):
        assert [a.tolist() for a in p['gt_sampled'][b]['groups']] == [w.tolist() for w in want[b]['groups']]
    assert np.array_equal(p['flip_x'], c['aug_flip_x'].astype(bool)) and np.array_equal(p['flip_y'], c['aug_flip_y'].astype(bool))
    assert np.array_equal(p['noise_rot'], c['aug_noise_rot']) and np.array_equal(p['noise_scale'], c['aug_noise_scale'])
    # the restatement: one generator, frame after frame
    rng = np.random.RandomState(info['aug_seed'])
    s2 = gr.sampler_of(c, info, None)
    for b in range(3):
        for g in s2.groups:
            num = g['num'] - int((classes[b] == g['class_id']).sum())
            if num <= 0:
                continue
            if g['pointer'] >= g['members'].size:
                g['indices'], g['pointer'] = rng.permutation(g['members'].size), 0
            assert g['members'][g['indices'][g['pointer']:g['pointer'] + num]].tolist() == info['aug_candidates'][b][g['name']]
            g['pointer'] += num
        fx = rng.choice([False, True], replace=False, p=[0.5, 0.5])
        fy = rng.choice([False, True], replace=False, p=[0.5, 0.5])
        rot, scl = rng.uniform(-0.3925, 0.3925), rng.uniform(0.95, 1.05)
        assert (fx, fy, rot, scl) == (p['flip_x'][b], p['flip_y'][b], p['noise_rot'][b], p['noise_scale'][b])
    with pytest.raises(ValueError, match='gt_classes'):
        aug.draw(3, np.random.RandomState(0))


def test_without_a_sampler_gt_sampling_is_skipped_as_before(caplog):
    info = META['cases']['s12']
    with caplog.at_level(logging.INFO):
        aug = DeviceWorldAugmentor(info['aug_cfg'], META['pc_range'], layout='nusc_map')
    assert aug.skipped == ['gt_sampling'] and aug.gt_sampler is None and [n for n, _ in aug.queue][0] == 'random_world_flip'
    assert sum('gt_sampling' in r.getMessage() for r in caplog.records) == 1
    p = aug.draw(2, np.random.RandomState(1))
    assert 'gt_sampled' not in p
    # a sampler with the entry disabled stays out of the queue too
    s = gr.sampler_of(gr.case_arrays(D, 's12'), info, None)
    off = DeviceWorldAugmentor(dict(info['aug_cfg'], DISABLE_AUG_LIST=['gt_sampling']), META['pc_range'], layout='nusc_map', gt_sampler=s)
    assert off.gt_sampler is None and off.skipped == []


def test_symbols_and_host_side_argument_checks():
    import ctypes
    for name in ('pcp_gt_sample_select', 'pcp_gt_sample_paste_points', 'pcp_gt_sample_paste_boxes'):
        assert name in lib.SYMBOLS
    L = lib.load()
    p = ctypes.c_void_p(256)
    assert L.pcp_gt_sample_select(p, 65, 4, 8, p, 3, p, p, 1, p, 1, p, 1, p, None) != 0          # batch
    assert L.pcp_gt_sample_select(p, 2, 4, 8, p, 17, p, p, 1, p, 1, p, 1, p, None) != 0          # groups
    assert L.pcp_gt_sample_select(p, 2, 4, 9, p, 3, p, p, 1, p, 1, p, 1, p, None) != 0           # box width
    assert L.pcp_gt_sample_paste_points(p, 10, 3, 2, p, 3, p, 1, p, p, p, p, 2, 0, p, p, None) != 0    # row stride
    assert L.pcp_gt_sample_paste_points(p, 10, 8, 2, p, 3, p, 1, p, p, p, p, 8, 0, p, p, None) != 0    # instance column outside the row
    assert L.pcp_gt_sample_paste_boxes(p, 2, 4, 8, p, 3, 5, p, 3, p, 1, p, p, p, p, p, 4, None) != 0   # tf rows


def test_from_infos_reads_path_records_like_the_reference(tmp_path):
    """records with a `path`: float32 files, the float64 fallback when the row count disagrees, and the refusal of a wrong row count"""
    from pcp_amd.gt_sampler import DeviceGtDatabase
    info = META['cases']['s7']
    c = gr.case_arrays(D, 's7')
    off = np.concatenate([[0], np.cumsum(c['db_counts'])])
    infos = {}
    for i, name in enumerate(info['db_names']):
        rows = c['db_points'][off[i]:off[i + 1]]
        rows.astype(np.float64 if i % 3 == 1 else np.float32).tofile(str(tmp_path / ('%d.bin' % i)))     # every third file holds doubles
        infos.setdefault(name, []).append({'name': name, 'path': '%d.bin' % i, 'box3d_lidar': c['db_boxes'][i], 'num_points_in_gt': int(c['db_counts'][i]),
                                           'instance_tf': c['db_instance_tf'][i], 'velo': c['db_velo'][i]})
    with pytest.raises(ValueError, match='root_path and columns'):
        DeviceGtDatabase.from_infos(infos, device=None)
    db = DeviceGtDatabase.from_infos(infos, root_path=tmp_path, columns=7, device=None)
    want = gr.database_of(c, info, None)
    assert db.names == want.names and np.array_equal(db.boxes, want.boxes) and np.array_equal(db.counts, want.counts)
    assert np.array_equal(db.velo, want.velo) and np.array_equal(db.instance_tf, want.instance_tf) and db.columns == 7 and db.points_dev is None
    assert np.array_equal(db.offsets, off[:-1])
    # global_data_offset records into one flat array give the same database, rows included
    flat = {n: [dict(r, global_data_offset=(int(off[info['db_names'].index(n) + k]), int(off[info['db_names'].index(n) + k + 1]))) for k, r in enumerate(v)]
            for n, v in infos.items()}
    db2 = DeviceGtDatabase.from_infos(flat, points=c['db_points'], device=None)
    assert np.array_equal(db2.counts, want.counts) and db2.names == want.names
    infos[info['db_names'][0]][0]['num_points_in_gt'] += 1
    with pytest.raises(ValueError, match='num_points_in_gt'):
        DeviceGtDatabase.from_infos(infos, root_path=tmp_path, columns=7, device=None)


def test_paste_form_option_is_declared():
    assert lib.OPTIONS['gts_paste_form'] == 8
    assert lib.set_option('gts_paste_form', 1) is None and lib.set_option('gts_paste_form', None) == 1
