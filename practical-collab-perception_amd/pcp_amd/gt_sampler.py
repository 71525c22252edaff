"""gt_sampling of a collated training batch on the device (csrc/gt_sample.hip).

The reference pastes ground-truth objects from a database into every sample in its DataLoader workers (pcdet/datasets/augmentor/
database_sampler.py: DataBaseSampler.__call__, add_sampled_boxes_to_scene).  Here

  * DeviceGtDatabase holds the database where the paste runs: the flat float32 point array (rows of NUM_POINT_FEATURES + 2 columns, xyz
    relative to the box centre), per-object offsets / counts, boxes, global velocities and instance matrices on the device, and host
    copies of everything but the points;
  * DeviceGtSampler.draw() reproduces the reference's per-class pointer / permutation state machine on a numpy RandomState (the only
    random part), apply() ships a candidate table and runs three kernels: the collision test and selection per frame, the ragged paste
    into the point rows, the new gt_boxes / instances_tf.  The scene's own points inside a pasted box stay, as in the reference fork
    (it has no remove_points_in_boxes3d).

Host reads per call: the class column of gt_boxes (rule: sample_num = configured - objects of that class already there) and one read of
2 B + 1 ints (accepted objects and added rows per frame, the error word).  There is no CPU path.
"""
import logging

import numpy as np
import torch

from . import lib as _lib
from .aug_common import _get
from .lib import check
from .ops import _need_cuda, _p, _stream

REFUSED_KEYS = ('IMG_AUG_TYPE', 'USE_ROAD_PLANE', 'DATABASE_WITH_FAKELIDAR')


class DeviceGtDatabase:
    """names: one class name per object; boxes (N, 7 | 9) float32 [x y z dx dy dz heading (vx vy)]; counts (N,) points per object; velo
    (N, 3) float64, the velocity in the global frame; instance_tf (N, S, 4, 4) float32; points: flat (sum counts, columns) float32 in
    object order.  `difficulty` (N,) or None is only read by PREPARE.filter_by_difficulty."""

    def __init__(self, names, boxes, counts, velo, instance_tf, points, difficulty=None, device='cuda'):
        self.names = [str(n) for n in names]
        n = len(self.names)
        self.boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.float32).reshape(n, -1))
        assert self.boxes.shape[1] in (7, 9), self.boxes.shape
        self.counts = np.asarray(counts, dtype=np.int64).reshape(n)
        self.offsets = np.concatenate([[0], np.cumsum(self.counts)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
        self.velo = np.asarray(velo, dtype=np.float64).reshape(n, 3)
        self.instance_tf = np.ascontiguousarray(np.asarray(instance_tf, dtype=np.float32))
        assert self.instance_tf.ndim == 4 and self.instance_tf.shape[0] == n and self.instance_tf.shape[2:] == (4, 4), self.instance_tf.shape
        self.difficulty = None if difficulty is None else np.asarray(difficulty)
        points = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
        assert points.ndim == 2 and points.shape[0] == int(self.counts.sum()), (points.shape, int(self.counts.sum()))
        if points.shape[0] >= 2 ** 31:
            raise ValueError('%d database rows: the kernels index them with int32' % points.shape[0])
        self.columns = int(points.shape[1])
        self.n_sweeps = int(self.instance_tf.shape[1])
        self.device = None                 # device=None: host copies only (drawing, inspection); apply() needs the device arrays
        self.points_dev = None
        if device is None:
            return
        dev = torch.device(device)
        if dev.type != 'cuda':
            raise _lib.PcpError('the ground-truth database lives in device memory (got %s); no CPU fallback exists' % dev)
        self.device = dev
        self.points_dev = torch.from_numpy(points).to(dev)
        self.counts_dev = torch.from_numpy(self.counts.astype(np.int32)).to(dev)
        self.offsets_dev = torch.from_numpy(self.offsets.astype(np.int32)).to(dev)
        self.boxes_dev = torch.from_numpy(self.boxes).to(dev)
        self.velo_dev = torch.from_numpy(self.velo.astype(np.float32)).to(dev)
        self.instance_tf_dev = torch.from_numpy(self.instance_tf).to(dev)

    def __len__(self):
        return len(self.names)

    def class_sizes(self):
        out = {}
        for n in self.names:
            out[n] = out.get(n, 0) + 1
        return out

    @classmethod
    def from_infos(cls, db_infos, points=None, root_path=None, columns=None, device='cuda'):
        """db_infos: the reference's dict class name -> list of records (name, box3d_lidar, num_points_in_gt, instance_tf, velo and either
        global_data_offset into `points` or a `path` below root_path; `columns` = NUM_POINT_FEATURES + 2 for the files, read as float32 and,
        when the row count disagrees, as float64, as the reference reads them)."""
        import os
        names, boxes, counts, velo, tfs, rows, diff = [], [], [], [], [], [], []
        for infos in db_infos.values():
            for info in infos:
                if 'global_data_offset' in info and points is not None:
                    lo, hi = info['global_data_offset']
                    obj = np.asarray(points[lo:hi], dtype=np.float32)
                else:
                    if root_path is None or columns is None:
                        raise ValueError("a record with a 'path' needs root_path and columns")
                    path = os.path.join(str(root_path), str(info['path']))
                    obj = np.fromfile(path, dtype=np.float32).reshape(-1, columns)
                    if obj.shape[0] != info['num_points_in_gt']:
                        obj = np.fromfile(path, dtype=np.float64).reshape(-1, columns).astype(np.float32)
                if obj.shape[0] != info['num_points_in_gt']:
                    raise ValueError('database record %s holds %d rows, num_points_in_gt says %d' % (info.get('path', info.get('global_data_offset')),
                                                                                                 obj.shape[0], info['num_points_in_gt']))
                names.append(info['name'])
                boxes.append(np.asarray(info['box3d_lidar'], dtype=np.float32))
                counts.append(int(info['num_points_in_gt']))
                velo.append(np.asarray(info.get('velo', np.zeros(3)), dtype=np.float64).reshape(3))
                tfs.append(np.asarray(info['instance_tf'], dtype=np.float32))
                rows.append(obj)
                diff.append(info.get('difficulty', 0))
        if not names:
            raise ValueError('the ground-truth database is empty')
        return cls(names, np.stack(boxes), counts, np.stack(velo), np.stack(tfs), np.concatenate(rows, axis=0), difficulty=diff, device=device)

    @classmethod
    def build_from_dataset(cls, dataset, frames, min_points=1, device='cuda'):
        """cuts the objects out of the first `frames` training items of `dataset` (the synthetic one included): pcp_points_in_boxes assigns
        rows to boxes, the rows are stored minus the box centre (float32), instance_tf comes from the item, and with
        metadata['tf_target_from_glob'] the box velocity is taken back to the global frame.  -> (database, db_infos dict)"""
        from . import ops
        class_names = list(dataset.class_names)
        db_infos = {n: [] for n in class_names}
        flat, n_rows = [], 0
        for index in range(int(frames)):
            item = dataset[index]
            gt = np.asarray(item['gt_boxes'], dtype=np.float32)
            pts = np.ascontiguousarray(np.asarray(item['points'], dtype=np.float32))
            if gt.shape[0] == 0 or pts.shape[0] == 0:
                continue
            W = gt.shape[1]
            assign = ops.points_in_boxes(torch.from_numpy(pts[None, :, :3].copy()).to(device), torch.from_numpy(gt[None, :, :7].copy()).to(device))
            assign = assign[0].cpu().numpy()
            tf_item = item.get('instances_tf', None)
            glob = item.get('metadata', {}).get('tf_target_from_glob', None) if isinstance(item.get('metadata', None), dict) else None
            for j in range(gt.shape[0]):
                rows = np.nonzero(assign == j)[0]
                cls_id = int(gt[j, W - 1])
                if rows.size < max(int(min_points), 1) or cls_id <= 0:
                    continue
                obj = pts[rows].copy()
                obj[:, :3] -= gt[j, :3]
                v = np.zeros(3)
                if W == 10:
                    v[:2] = gt[j, 7:9]
                    if glob is not None:
                        v = np.linalg.inv(np.asarray(glob, dtype=np.float64)[:3, :3]) @ v
                tf = np.asarray(tf_item[j], dtype=np.float32) if tf_item is not None else np.eye(4, dtype=np.float32)[None]
                if tf.shape[-2] == 3:
                    tf = np.concatenate([tf, np.broadcast_to(np.asarray([0, 0, 0, 1], np.float32), tf.shape[:-2] + (1, 4))], axis=-2)
                name = class_names[cls_id - 1]
                db_infos[name].append({'name': name, 'box3d_lidar': gt[j, :W - 1].copy(), 'num_points_in_gt': int(rows.size), 'instance_tf': tf,
                                       'velo': v, 'global_data_offset': (n_rows, n_rows + int(rows.size)), 'frame': index, 'gt_idx': j,
                                       'difficulty': 0})
                flat.append(obj)
                n_rows += int(rows.size)
        if not flat:
            raise ValueError('no object of the first %d training items holds %d points' % (frames, min_points))
        points = np.concatenate(flat, axis=0)
        return cls.from_infos(db_infos, points=points, device=device), db_infos


class DeviceGtSampler:
    """sampler_cfg: the gt_sampling entry of AUG_CONFIG_LIST (PREPARE, SAMPLE_GROUPS, LIMIT_WHOLE_SCENE, NUM_POINT_FEATURES,
    POINT_FEAT_INDEX_OFFSET_FROM_RAW_FEAT); class_names: the model's classes (a class id of gt_boxes is 1 + its index)."""

    def __init__(self, sampler_cfg, class_names, database, logger=None):
        self.logger = logger or logging.getLogger(__name__)
        self.class_names = list(class_names)
        self.db = database
        self._logged = False
        for key in REFUSED_KEYS:
            v = _get(sampler_cfg, key, None)
            if v is not None and v is not False:
                raise ValueError('gt_sampling: %s = %r is not supported on the device path' % (key, v))
        members = {n: [i for i, nm in enumerate(database.names) if nm == n] for n in self.class_names}
        prepare = _get(sampler_cfg, 'PREPARE', None) or {}
        for func, val in (prepare.items() if hasattr(prepare, 'items') else []):
            if func == 'filter_by_min_points':
                for name_num in val:
                    name, num = name_num.split(':')
                    if int(num) > 0 and name in members:
                        kept = [i for i in members[name] if database.counts[i] >= int(num)]
                        self.logger.info('Database filter by min points %s: %d => %d' % (name, len(members[name]), len(kept)))
                        members[name] = kept
            elif func == 'filter_by_difficulty':
                for name in members:
                    kept = [i for i in members[name] if database.difficulty is None or database.difficulty[i] not in val]
                    self.logger.info('Database filter by difficulty %s: %d => %d' % (name, len(members[name]), len(kept)))
                    members[name] = kept
            else:
                raise ValueError('gt_sampling: PREPARE.%s is not supported on the device path' % func)
        self.limit_whole_scene = bool(_get(sampler_cfg, 'LIMIT_WHOLE_SCENE', False))
        self.groups = []                                    # dicts: name, class id, configured number, db members, pointer, indices
        for x in _get(sampler_cfg, 'SAMPLE_GROUPS'):
            name, num = x.split(':')
            if name not in self.class_names:
                continue
            if not members[name]:
                raise ValueError('gt_sampling: SAMPLE_GROUPS names %s, whose database is empty after PREPARE' % name)
            self.groups.append({'name': name, 'class_id': self.class_names.index(name) + 1, 'num': int(num),
                                'members': np.asarray(members[name], dtype=np.int64), 'pointer': len(members[name]),
                                'indices': np.arange(len(members[name]))})
        if not self.groups:
            raise ValueError('gt_sampling: SAMPLE_GROUPS names no class of %s' % self.class_names)
        if len(self.groups) > _lib.GTS_MAX_GROUPS:
            raise ValueError('gt_sampling: %d sample groups, the kernels take %d' % (len(self.groups), _lib.GTS_MAX_GROUPS))
        for g in self.groups:
            if g['num'] > _lib.GTS_MAX_CAND:
                raise ValueError('gt_sampling: %s samples %d candidates per frame, the kernels take %d' % (g['name'], g['num'], _lib.GTS_MAX_CAND))
        self.num_point_features = int(_get(sampler_cfg, 'NUM_POINT_FEATURES'))
        off = _get(sampler_cfg, 'POINT_FEAT_INDEX_OFFSET_FROM_RAW_FEAT')
        self.inst_col = 1 + self.num_point_features + int(_get(off, 'INSTANCE_INDEX'))      # in a collated row: column 0 is the frame index
        if database.columns != self.num_point_features + 2:
            raise ValueError('gt_sampling: database rows have %d columns, NUM_POINT_FEATURES + 2 = %d' % (database.columns, self.num_point_features + 2))

    def class_sizes(self):
        return {g['name']: int(g['members'].size) for g in self.groups}

    # ---- the random part: the reference's sample_with_fixed_number, class after class --------------------------------------------------
    def draw(self, frame_gt_classes, rng):
        """frame_gt_classes: the class ids (> 0) of the frame's ORIGINAL boxes; rng: numpy.random.RandomState.  -> {'n_own', 'groups': per
        sample group the drawn database indices (int64, possibly fewer than asked at the end of a pass, empty when nothing is drawn)}"""
        cls = np.asarray(frame_gt_classes).reshape(-1)
        out = []
        for g in self.groups:
            num = g['num'] - int((cls == g['class_id']).sum()) if self.limit_whole_scene else g['num']
            if num <= 0:
                out.append(np.zeros(0, dtype=np.int64))
                continue
            n = int(g['members'].size)
            if g['pointer'] >= n:
                g['indices'] = rng.permutation(n)
                g['pointer'] = 0
            out.append(g['members'][g['indices'][g['pointer']:g['pointer'] + num]])
            g['pointer'] += num                              # by the number asked for, not by the slice length: no wrap
        return {'n_own': int(cls.size), 'groups': out}

    @staticmethod
    def frame_gt_classes(gt_boxes):
        """the one host read of the class column: per frame the class ids of its real rows, which must be rows 0 .. n - 1"""
        cls = gt_boxes[..., -1].detach().cpu().numpy()
        out = []
        for b in range(cls.shape[0]):
            n = int((cls[b] > 0).sum())
            if not (cls[b, :n] > 0).all():
                raise ValueError('gt_boxes of frame %d: the rows of class > 0 are not contiguous from row 0' % b)
            out.append(cls[b, :n].astype(np.int64))
        return out

    # ---- the device part ---------------------------------------------------------------------------------------------------------------
    def candidate_table(self, drawn, box_width, metadata):
        """-> (frame_table (B, G + 2) int32, cand_db (T,) int32, cand_box (T, GTS_CAND_STRIDE) float32, rows the candidates hold)"""
        B, G = len(drawn), len(self.groups)
        if not 0 < B <= _lib.AUG_MAX_BATCH:
            raise ValueError('batch of %d frames: the gt_sampling kernels take 1 to %d' % (B, _lib.AUG_MAX_BATCH))
        ft = np.zeros((B, G + 2), dtype=np.int32)
        dbs, boxes = [], []
        t = 0
        for b, d in enumerate(drawn):
            assert len(d['groups']) == G
            ft[b, 0] = d['n_own']
            total = 0
            R = None
            for g, (grp, idx) in enumerate(zip(self.groups, d['groups'])):
                idx = np.asarray(idx, dtype=np.int64)
                if idx.size > _lib.GTS_MAX_CAND:
                    raise ValueError('gt_sampling: %d candidates of %s in frame %d, the kernels take %d' % (idx.size, grp['name'], b, _lib.GTS_MAX_CAND))
                ft[b, 1 + g] = t
                if idx.size:
                    row = np.zeros((idx.size, _lib.GTS_CAND_STRIDE), dtype=np.float32)
                    row[:, :7] = self.db.boxes[idx, :7]
                    if box_width == 10:
                        if R is None:
                            m = metadata[b] if metadata is not None else None
                            if not isinstance(m, dict) or 'tf_target_from_glob' not in m:
                                raise ValueError("gt_sampling with velocity boxes needs metadata[%d]['tf_target_from_glob']" % b)
                            R = np.asarray(m['tf_target_from_glob'])[:3, :3]
                        for k, i in enumerate(idx):                     # tf_target_from_glob[:3, :3] @ velo, float64, rounded once
                            row[k, 7:9] = (R @ self.db.velo[i].reshape(3, 1))[:2, 0]
                    row[:, 9] = grp['class_id']
                    dbs.append(idx.astype(np.int32))
                    boxes.append(row)
                t += idx.size
                total += idx.size
            ft[b, 1 + G] = t
            if d['n_own'] + total > _lib.GTS_MAX_BOXES:
                raise ValueError('gt_sampling: frame %d holds %d boxes and %d candidates, the kernels take %d existing + candidate boxes (every candidate may be accepted)'
                                 % (b, d['n_own'], total, _lib.GTS_MAX_BOXES))
        cand_db = np.concatenate(dbs) if dbs else np.zeros(0, dtype=np.int32)
        cand_box = np.concatenate(boxes, axis=0) if boxes else np.zeros((0, _lib.GTS_CAND_STRIDE), dtype=np.float32)
        return ft, cand_db, cand_box, int(self.db.counts[cand_db].sum()) if cand_db.size else 0

    def apply(self, batch_dict, drawn):
        """pastes into batch_dict (new tensors under the same keys): points, gt_boxes, instances_tf; metadata[b]['num_added_instances'];
        gt_sampled_db_index: per frame the database indices of the pasted objects in order (device int32 views, nothing read back)"""
        B = int(batch_dict['batch_size'])
        assert len(drawn) == B, (len(drawn), B)
        points, gt, tf = batch_dict['points'], batch_dict['gt_boxes'], batch_dict.get('instances_tf', None)
        _need_cuda(points, gt, tf)
        if self.db.points_dev is None:
            raise _lib.PcpError('the ground-truth database was built with device=None; the paste needs it in device memory')
        if gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] not in (8, 10):
            raise ValueError('gt_boxes of shape %s: gt_sampling takes (B, M, 8 | 10)' % (tuple(gt.shape),))
        if points.dim() != 2 or points.dtype != torch.float32 or not _lib.AUG_MIN_ROW_STRIDE <= points.shape[1] <= _lib.AUG_MAX_ROW_STRIDE:
            raise ValueError('points of shape %s (%s): gt_sampling takes float32 (N, 1 + C) rows of %d up to %d columns'
                             % (tuple(points.shape), points.dtype, _lib.AUG_MIN_ROW_STRIDE, _lib.AUG_MAX_ROW_STRIDE))
        if points.shape[1] != 1 + self.db.columns:
            raise ValueError('points have 1 + %d columns, the database rows %d' % (points.shape[1] - 1, self.db.columns))
        if (gt.shape[2] == 10) != (self.db.boxes.shape[1] == 9):
            raise ValueError('gt_boxes are %d wide, the database boxes %d' % (gt.shape[2], self.db.boxes.shape[1]))
        _, M, W = (int(v) for v in gt.shape)
        n_sweeps = tf_rows = 0
        if tf is not None:
            if tf.dim() != 5 or tuple(tf.shape[:2]) != (B, M) or tf.shape[3] not in (3, 4) or tf.shape[4] != 4 or tf.shape[2] != self.db.n_sweeps:
                raise ValueError('instances_tf of shape %s: gt_sampling takes (%d, %d, %d, 3 | 4, 4), the sweeps of the database' % (tuple(tf.shape), B, M, self.db.n_sweeps))
            n_sweeps, tf_rows = int(tf.shape[2]), int(tf.shape[3])
            tf = tf.float().contiguous()
        meta = batch_dict.get('metadata', None)
        ft, cand_db, cand_box, max_added = self.candidate_table(drawn, W, meta)
        G, T = len(self.groups), int(cand_db.size)
        dev = points.device
        # one upload: frame table | database indices | candidate boxes (as bits), each part starting on a multiple of 4 words
        a0 = (ft.size + 3) // 4 * 4
        a1 = a0 + (max(T, 1) + 3) // 4 * 4
        host = np.zeros(a1 + max(T, 1) * _lib.GTS_CAND_STRIDE, dtype=np.int32)
        host[:ft.size] = ft.reshape(-1)
        host[a0:a0 + T] = cand_db
        host[a1:a1 + T * _lib.GTS_CAND_STRIDE] = cand_box.reshape(-1).view(np.int32)
        table = torch.from_numpy(host).to(dev)
        ft_d, db_d, box_d = table[:a0], table[a0:a1], table[a1:].view(torch.float32)
        cap = max(int((ft[:, 1 + G] - ft[:, 1]).max()), 1)
        acc = torch.empty((B, cap, _lib.GTS_ACC_STRIDE), dtype=torch.int32, device=dev)
        counts = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)
        seg = torch.empty(B + 1, dtype=torch.int32, device=dev)
        gt = gt.float().contiguous()
        points = points.contiguous()
        if points.data_ptr() % 16:
            points = points.clone()
        n, S = int(points.shape[0]), int(points.shape[1])
        out = torch.empty((n + max_added, S), dtype=torch.float32, device=dev)
        L = _lib.load()
        check(L.pcp_gt_sample_select(_p(gt), B, M, W, _p(ft_d), G, _p(db_d), _p(box_d), T, _p(self.db.counts_dev), len(self.db), _p(acc), cap,
                                     _p(counts), _stream()), 'pcp_gt_sample_select')
        check(L.pcp_gt_sample_paste_points(_p(points), n, S, B, _p(ft_d), G, _p(acc), cap, _p(counts), _p(box_d), _p(self.db.points_dev),
                                           _p(self.db.offsets_dev), self.inst_col, max_added, _p(out), _p(seg), _stream()),
              'pcp_gt_sample_paste_points')
        c = counts.cpu().numpy()                              # the one read: accepted, added rows, error word
        if c[2 * B] != 0:
            raise ValueError('gt_sampling: the point rows are not grouped by ascending frame index in [0, %d) (error word %d)' % (B, int(c[2 * B])))
        n_acc, added = c[:B], c[B:2 * B]
        n_own = ft[:, 0]
        m_out = int((n_own + n_acc).max())
        gt_out = torch.empty((B, m_out, W), dtype=torch.float32, device=dev)
        tf_out = torch.empty((B, m_out, n_sweeps, tf_rows, 4), dtype=torch.float32, device=dev) if tf is not None else None
        check(L.pcp_gt_sample_paste_boxes(_p(gt), B, M, W, _p(tf), n_sweeps, tf_rows, _p(ft_d), G, _p(acc), cap, _p(counts), _p(box_d),
                                          _p(self.db.instance_tf_dev), _p(gt_out), _p(tf_out), m_out, _stream()), 'pcp_gt_sample_paste_boxes')
        batch_dict['points'] = out[:n + int(added.sum())]
        batch_dict['gt_boxes'] = gt_out
        if tf_out is not None:
            batch_dict['instances_tf'] = tf_out
        if meta is not None:
            batch_dict['metadata'] = [dict(m, num_added_instances=int(n_acc[b])) if isinstance(m, dict) else m for b, m in enumerate(meta)]
        batch_dict['gt_sampled_db_index'] = [acc[b, :int(n_acc[b]), 1] for b in range(B)]
        batch_dict['gt_sampled_rows'] = added.astype(np.int64)
        if not self._logged:                                 # once: what the first batch got
            self._logged = True
            self.logger.info('device gt_sampling: first batch pasted %d instances, %d rows' % (int(n_acc.sum()), int(added.sum())))
        return batch_dict

    def __call__(self, batch_dict, rng):
        classes = self.frame_gt_classes(batch_dict['gt_boxes'])
        return self.apply(batch_dict, [self.draw(c, rng) for c in classes])
