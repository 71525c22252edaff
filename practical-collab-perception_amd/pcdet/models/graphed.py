"""hipGraph capture of a detector's forward (MI355X pipeline mode, not in the reference).

At small batch the path is launch bound (~70 launches per frame through Python/ctypes); every C-ABI entry point is
capturable by construction (no allocation, no sync, explicit stream), so the whole module chain -- point copy-in, pillariser,
PFN, convolutions, HunterJr, decode, NMS -- becomes one graph replay per batch; only the final "how many boxes" host read
stays outside.  Shapes are frozen at capture time (N points, batch size); feed a batch of another size eagerly.
DiscoNet (round 5): the BEV makers' agent discovery -- torch.unique(...).cpu() in the reference (bev_maker.py:156), a histogram read-back in
the eager path -- is replaced by device-side flags under capture: the makers run for every agent the metadata lists with the whole cloud as
the row capacity, and pcp_zero_maps_unless zeroes the maps the reference would not have produced (`_pcp_static_agents`).  The agents'
poses travel as kernel arguments: they are frozen at capture time like the shapes (a new pose set needs a new capture).
"""
import torch


class GraphedDetector:
    def __init__(self, model, points, batch_size, metadata, warmup=3):
        assert points.is_cuda and not model.training
        if any(type(m).__name__ == 'PillarVFE' for m in model.modules()):
            raise NotImplementedError('GraphedDetector: PillarVFE reads the voxel count back to size its tensors and cannot be captured; '
                                      'run the model batch by batch')
        if any(type(m).__name__ == 'VoxelResBackBone8x' for m in model.modules()):
            raise NotImplementedError('GraphedDetector: VoxelResBackBone8x reads the row count of every strided sparse conv back and cannot be '
                                      'captured; run the model batch by batch')
        self.model = model
        self.batch_size = batch_size
        self.metadata = metadata
        self.static_points = points.clone()
        self._pristine_shape = tuple(points.shape)
        for m in model.modules():
            if hasattr(m, 'materialize_pillars'):
                m.materialize_pillars = False          # exact-shape per-pillar tensors need a host sync
                m.reuse_buffers = True
        self.head = model.dense_head
        self.head.defer_finalize = True
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(warmup):
                    self.static_points.copy_(points)
                    self._pending = self._run_modules()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph), torch.no_grad():
                self._pending = self._run_modules()
        finally:
            self.head.defer_finalize = False

    def _run_modules(self):
        bd = {'points': self.static_points, 'batch_size': self.batch_size, 'metadata': self.metadata}
        if any(type(m).__name__ == 'BEVMaker' for m in self.model.module_list):
            bd['_pcp_static_agents'] = True                  # no host read inside the capture (see the module docstring)
        if hasattr(self.model, '_run_modules'):
            # the detector's own runner: the frozen BEV-maker passes on their own streams (forked from / joined to the capturing stream by
            # events, so they become parallel branches of the graph) and one pillar list for the two VFEs that see the same cloud
            bd = self.model._run_modules(bd)
        else:
            for m in self.model.module_list:
                bd = m(bd)
        self._last = bd
        return bd['_pcp_pending_head']

    def __call__(self, points):
        assert tuple(points.shape) == self._pristine_shape, 'graph was captured for a different point count'
        self.static_points.copy_(points, non_blocking=True)
        self.graph.replay()
        return self.head.finalize(self._pending, self.batch_size)

    @property
    def batch_dict(self):
        """static tensors of the captured forward (overwritten by every replay)"""
        return self._last
