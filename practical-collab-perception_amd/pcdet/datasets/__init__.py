"""Dataset side of the plugin surface.  The reference's V2X-Sim datasets need the V2X-Sim data and nuscenes-devkit 1.1.9
(pcdet/datasets/v2x_sim/, README.md:77), neither available offline, and are numpy-only code outside the hot path
(SURVEY.md section 2).  What the hot path needs from a dataset is (a) the six attributes Detector3DTemplate reads and
(b) the collate layout: a frame-index column prepended to every point row (pcdet/datasets/dataset.py:224-229).
SyntheticV2XDataset provides both with the counter-based clouds of pcp_amd.synth; build_dataloader keeps the reference's
signature (pcdet/datasets/__init__.py:54-82) and DistributedSampler semantics."""
import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data import DistributedSampler as _DistributedSampler

from pcp_amd import synth

from ..models import DatasetInfo
from ..utils import common_utils

LAYOUT_OF = {'V2XSimDataset_CAR': 'car', 'V2XSimDataset_RSU': 'car', 'V2XSimDataset_EGO': 'lately', 'V2XSimDataset_EGO_LATE': 'lately',
             'V2XSimDataset_EGO_EARLY': 'early', 'V2XSimDataset_EGO_DISCO': 'disco'}
AGENTS_OF = {'car': 1, 'lately': 1, 'early': 6, 'disco': 6, 'nusc_map': 1}


class SyntheticV2XDataset(DatasetInfo, Dataset):
    def __init__(self, dataset_cfg, class_names, training=False, root_path=None, logger=None):
        vs = [p.VOXEL_SIZE for p in dataset_cfg.DATA_PROCESSOR if 'VOXEL_SIZE' in p][0]
        enc = dataset_cfg.POINT_FEATURE_ENCODING
        DatasetInfo.__init__(self, class_names, dataset_cfg.POINT_CLOUD_RANGE, vs, len(enc.used_feature_list), dataset_cfg.DATA_PROCESSOR)
        self.dataset_cfg = dataset_cfg
        self.training = training
        self.logger = logger
        self.layout = LAYOUT_OF.get(dataset_cfg.DATASET, 'car')
        syn = dataset_cfg.get('SYNTHETIC', {})
        self.points_per_agent = int(syn.get('POINTS_PER_AGENT', 60000))
        self.num_frames = int(syn.get('NUM_FRAMES', 16))
        self.distribution = syn.get('DISTRIBUTION', 'uniform')
        if dataset_cfg.DATASET == 'NuScenesDataset' and len(enc.used_feature_list) == 12:
            self.layout = 'nusc_map'       # the five HD-map layers behind the timestamp (synth.nusc_cloud with_map)
            self.points_per_agent = int(syn.get('POINTS_PER_FRAME', self.points_per_agent))   # the nuScenes configs size the frame
        self.xy_half = float(syn.get('XY_HALF', 52.0))
        self.gt_boxes_max = int(syn.get('GT_BOXES', 40))      # boxes of a training frame before the index-dependent cut
        self.eval_gt = bool(syn.get('EVAL_GT', False))        # evaluation items carry gt_boxes too (pcp_amd/det_eval.py scores against them)

    @property
    def mode(self):
        return 'train' if self.training else 'test'

    def __len__(self):
        return self.num_frames

    def __getitem__(self, index):
        parts = []
        n_agents = AGENTS_OF[self.layout]
        for a in range(n_agents):
            if self.layout == 'nusc_map':
                c = synth.nusc_cloud(index, self.points_per_agent, xy_half=self.xy_half, with_map=True, dist=self.distribution)
            else:
                c = synth.agent_cloud(agent=100 * index + a, n_points=self.points_per_agent, layout=self.layout, dist=self.distribution)
            if self.layout == 'disco':
                c[:, -1] = float(a)
            parts.append(c)
        meta = {'sample_token': 'synthetic_%06d' % index, 'lidar_id': 1,
                'se3_from_ego': {a: synth.agent_pose(a) for a in range(n_agents) if a != 1}}
        if self.training and self.dataset_cfg.DATASET == 'NuScenesDataset':
            # the pose gt_sampling maps a database object's global velocity with (database_sampler.py reads metadata['tf_target_from_glob'])
            r = np.random.RandomState(77000 + int(index))
            yaw = r.uniform(-np.pi, np.pi)
            T = np.eye(4)
            T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
            T[:3, 3] = [r.uniform(-200.0, 200.0), r.uniform(-200.0, 200.0), r.uniform(-1.0, 1.0)]
            meta['tf_target_from_glob'] = T
        if self.dataset_cfg.DATASET == 'V2XSimDataset_EGO_LATE':
            # box-level fusion reads every agent's detections from the exchange database (v2x_sim_dataset_ego_late.py): synthetic stand-in
            # = 40 boxes per agent, neighbouring agents reporting overlapping boxes so that the NMS has something to merge
            meta['exchange_boxes'] = {a: self.synthetic_exchange_boxes(index, a) for a in range(6)}
        item = {'points': np.concatenate(parts, 0), 'frame_id': index, 'metadata': meta}
        if self.training and self.layout == 'nusc_map':
            # the HD-map models train on 10-column boxes; the corrector model reads the foreground rows and instances_tf, withmap ignores them
            item['gt_boxes'] = self.synthetic_gt_boxes_velocity(index)
            sweeps = int(self.dataset_cfg.get('MAX_SWEEPS', 10))
            fg, item['instances_tf'] = synth.nusc_instance_foreground(index, item['gt_boxes'], n_sweeps=sweeps)
            item['points'] = np.concatenate([item['points'], fg], 0)
        elif self.training:
            item['gt_boxes'] = self.synthetic_gt_boxes(index)
            if self.layout == 'car' and self.dataset_cfg.DATASET in ('V2XSimDataset_CAR', 'V2XSimDataset_RSU'):
                # configs 1 / 2 train HunterJr: foreground points carry (sweep, instance) and every instance its per-sweep motion
                fg, item['instances_tf'] = self.synthetic_foreground(index, item['gt_boxes'])
                item['points'] = np.concatenate([item['points'], fg], 0)
        elif self.eval_gt:
            # the boxes a training item of this index carries; without EVAL_GT an evaluation item keeps its keys (and its batch its bytes)
            item['gt_boxes'] = self.synthetic_gt_boxes_velocity(index) if self.layout == 'nusc_map' else self.synthetic_gt_boxes(index)
        return item

    def synthetic_foreground(self, index, gt, n_sweeps=11, per_local=12):
        """the fields V2XSimDataset_CAR adds for HunterJr (pcdet/datasets/v2x_sim/v2x_sim_dataset_car.py): see synth.instance_foreground"""
        return synth.instance_foreground(index, gt, n_sweeps, per_local)

    def synthetic_exchange_boxes(self, index, agent, n=40):
        """(n, 9) [box7, score, label]: the boxes of synthetic_gt_boxes jittered per agent (same objects seen by several agents)"""
        gt = self.synthetic_gt_boxes(index, n_max=n)
        s = synth.SEED_BASE + 7000 + 10 * index + agent
        out = np.zeros((gt.shape[0], 9), dtype=np.float32)
        out[:, :7] = gt[:, :7]
        out[:, 0:2] += synth.uniform(s, 1, gt.shape[0] * 2, -0.3, 0.3).reshape(-1, 2)
        out[:, 7] = synth.uniform(s, 2, gt.shape[0], 0.05, 0.95)
        out[:, 8] = gt[:, 7]
        return out[agent::2].copy()                       # every agent sees a different subset

    def synthetic_gt_boxes(self, index, n_max=None):
        """(n, 8) [x, y, z, dx, dy, dz, heading, class] car-sized boxes inside the range, n varies with the frame"""
        n_max = self.gt_boxes_max if n_max is None else n_max
        n = n_max - (index % 7)
        s = synth.SEED_BASE + 5000 + index
        r = self.point_cloud_range
        gt = np.zeros((n, 8), dtype=np.float32)
        gt[:, 0] = synth.uniform(s, 1, n, float(r[0]) + 1.0, float(r[3]) - 1.0)
        gt[:, 1] = synth.uniform(s, 2, n, float(r[1]) + 1.0, float(r[4]) - 1.0)
        gt[:, 2] = synth.uniform(s, 3, n, -3.0, -1.0)
        gt[:, 3] = synth.uniform(s, 4, n, 3.0, 5.5)
        gt[:, 4] = synth.uniform(s, 5, n, 1.5, 2.5)
        gt[:, 5] = synth.uniform(s, 6, n, 1.4, 2.0)
        gt[:, 6] = synth.uniform(s, 7, n, -3.14159, 3.14159)
        gt[:, 7] = np.floor(synth.uniform(s, 8, n, 1.0, len(self.class_names) + 0.999))
        return gt

    def synthetic_gt_boxes_velocity(self, index, n_max=None):
        """(n, 10) [x, y, z, dx, dy, dz, heading, vx, vy, class]: the boxes of synthetic_gt_boxes with the velocity the foreground of
        synth.nusc_instance_foreground moves at (odd rows drive along their heading, even rows stand still); the centre of the LAST row is
        put outside the range, so that the corrector's box filter has a row to drop"""
        g8 = self.synthetic_gt_boxes(index, n_max)
        n = g8.shape[0]
        gt = np.zeros((n, 10), dtype=np.float32)
        gt[:, :7], gt[:, 9] = g8[:, :7], g8[:, 7]
        speed = np.where(np.arange(n) % 2 == 1, 3.0 + 0.5 * np.arange(n), 0.0)
        gt[:, 7] = (speed * np.cos(g8[:, 6].astype(np.float64))).astype(np.float32)
        gt[:, 8] = (speed * np.sin(g8[:, 6].astype(np.float64))).astype(np.float32)
        gt[n - 1, 0] = float(self.point_cloud_range[3]) + 2.0
        return gt

    @staticmethod
    def collate_batch(batch_list, _unused=False):
        """reference layout: `points` gets the frame index as column 0; metadata / frame_id stay python lists."""
        ret = {'batch_size': len(batch_list)}
        ret['points'] = synth.collate([b['points'] for b in batch_list])
        ret['frame_id'] = np.array([b['frame_id'] for b in batch_list])
        ret['metadata'] = [b['metadata'] for b in batch_list]
        if 'gt_boxes' in batch_list[0]:
            # zero-padded to the longest frame (pcdet/datasets/dataset.py:260-266)
            m = max(b['gt_boxes'].shape[0] for b in batch_list)
            gt = np.zeros((len(batch_list), m, batch_list[0]['gt_boxes'].shape[1]), dtype=np.float32)
            for i, b in enumerate(batch_list):
                gt[i, :b['gt_boxes'].shape[0]] = b['gt_boxes']
            ret['gt_boxes'] = gt
            ret['num_gt_boxes'] = [int(b['gt_boxes'].shape[0]) for b in batch_list]   # the host's numbers: the device augmentor draws per box
            if 'instances_tf' in batch_list[0]:
                tf = np.zeros((len(batch_list), m) + batch_list[0]['instances_tf'].shape[1:], dtype=np.float32)
                tf[..., :3, :3] = np.eye(3, dtype=np.float32)
                for i, b in enumerate(batch_list):
                    tf[i, :b['instances_tf'].shape[0]] = b['instances_tf']
                ret['instances_tf'] = tf
        return ret

    def generate_prediction_dicts(self, batch_dict, pred_dicts, class_names, output_path=None):
        out = []
        for i, pd in enumerate(pred_dicts):
            labels = pd['pred_labels'].cpu().numpy()
            out.append({'frame_id': batch_dict['frame_id'][i], 'boxes_lidar': pd['pred_boxes'].cpu().numpy(),
                        'score': pd['pred_scores'].cpu().numpy(), 'pred_labels': labels,
                        'name': np.array(class_names)[labels - 1] if labels.size else np.zeros(0, dtype='<U8')})
        return out

    def evaluation(self, det_annos, class_names, **kwargs):
        n = sum(len(a['score']) for a in det_annos)
        if kwargs.get('device_eval', None) is not None:
            # (metrics, text) of pcp_amd.det_eval.DeviceDetectionEval.result(): the nuScenes-protocol report against the synthetic boxes
            metrics, text = kwargs['device_eval']
            out = {'num_detections': n, 'mAP': metrics['mean_ap']}
            out.update(metrics['tp_errors'])
            if 'nd_score' in metrics:
                out['NDS'] = metrics['nd_score']
            out['metrics'] = metrics
            return text + 'mAP line: mean_ap %.6f over %d detections, %d frames\n' % (metrics['mean_ap'], n, len(det_annos)), out
        return 'synthetic data: %d detections over %d frames (no ground truth, no mAP)\n' % (n, len(det_annos)), {'num_detections': n}


__all__ = {name: SyntheticV2XDataset for name in LAYOUT_OF}
__all__['SyntheticV2XDataset'] = SyntheticV2XDataset


class DistributedSampler(_DistributedSampler):
    """round-robin shard without shuffling in eval (reference: pcdet/datasets/__init__.py:31-51)"""

    def __init__(self, dataset, num_replicas=None, rank=None, shuffle=True):
        super().__init__(dataset, num_replicas=num_replicas, rank=rank, shuffle=shuffle)


def build_dataloader(dataset_cfg, class_names, batch_size, dist, root_path=None, workers=0, seed=None, logger=None, training=True,
                     merge_all_iters_to_one_epoch=False, total_epochs=0):
    dataset = __all__.get(dataset_cfg.DATASET, SyntheticV2XDataset)(dataset_cfg=dataset_cfg, class_names=class_names,
                                                                   root_path=root_path, training=training, logger=logger)
    sampler = None
    if dist:
        rank, world = common_utils.get_dist_info()
        sampler = DistributedSampler(dataset, world, rank, shuffle=training)
    loader = DataLoader(dataset, batch_size=batch_size, pin_memory=True, num_workers=workers, shuffle=(sampler is None) and training,
                        collate_fn=dataset.collate_batch, drop_last=False, sampler=sampler, timeout=0)
    return dataset, loader, sampler
