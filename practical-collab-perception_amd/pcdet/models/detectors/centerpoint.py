"""CenterPoint detector: the module chain of the reference (pcdet/models/detectors/centerpoint.py:4-78) --
forward = for m in module_list: batch_dict = m(batch_dict); eval returns (pred_dicts, recall_dict)."""
import torch

from .detector3d_template import Detector3DTemplate


class _HipBackward(torch.autograd.Function):
    """One-node autograd graph behind the training loss: loss.backward() runs the hand-written backward closures the train-mode
    modules recorded (reverse order), which deposit the gradients in param.grad."""

    @staticmethod
    def forward(ctx, anchor, value, tape, hook=None):
        ctx.tape = tape
        ctx.hook = hook
        return value.detach().clone()

    @staticmethod
    def backward(ctx, grad_out):
        scale = float(grad_out)
        if scale != 1.0:
            raise NotImplementedError('scale the loss through the optimizer (grad_scale), not through loss.backward(gradient=...)')
        run_tape(ctx.tape, ctx.hook)
        return None, None, None, None


class Tape(list):
    """the backward closures a training forward recorded; `done` once they ran"""
    done = False


# `hook`: set on the MODEL by its data-parallel optimizer (tools/train_utils/optimization: FlatAdamOneCycle.attach_overlap, attribute
# `_pcp_grad_ready_hook`) and carried by the loss node of every forward of THAT model: called with the name of each module whose backward
# closure has just been queued, so the gradient all-reduce of the modules that finish FIRST in the backward pass (head, fusion) runs under
# the backward of the rest (backbone, VFE) -- what DistributedDataParallel's buckets do at the reference's train.py:161.  (Round 4 kept the
# hook in a process global: a second optimizer in the process replaced it, and another model's backward fired this one's reduction.)
def run_tape(tape, hook=None):
    g = None
    for name, fn in reversed(tape):
        g = fn(g)
        if hook is not None:
            hook(name)
    if isinstance(tape, Tape):
        tape.done = True


def hip_loss(value, tape, hook=None):
    anchor = torch.zeros((), dtype=torch.float32, device=value.device, requires_grad=True)
    return _HipBackward.apply(anchor, value, tape, hook)


class CenterPoint(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    # MI355X knob (off by default = the reference's sequential module chain): the frozen BEVMaker passes of a DiscoNet forward are
    # independent of each other and of the ego trunk until V2XMidFusionDisco reads their maps, so each runs on its own HIP stream and
    # the streams are joined in front of the fusion module.  Same kernels, same inputs, same launch order per stream: outputs are
    # bit-identical (tests/test_gpu_e2e.py::test_overlapped_makers_*); small launches of one pass fill the CUs another pass leaves idle.
    # Works in train() mode too: the makers are frozen teachers evaluated under no_grad, the tape only holds the ego branch.
    overlap_makers = False
    # MI355X knob (off by default, never part of a headline number): skip BEV-maker passes whose output no later module reads -- reference
    # quirk F3 (bev_maker.py:157,212-230): every rsu / car maker REPLACES batch_dict['bev_img'], so an rsu maker followed by a car maker
    # is overwritten (the car maker re-encodes agent 0 with its own weights), and 'bev_img_early' feeds only the training distillation
    # loss (v2x_fusion_disco.py:119).  pred_dicts are bit-identical (tests/test_gpu_e2e.py::test_eliding_dead_makers_*); bench.py
    # --elide-dead-makers reports what the quirk costs.
    elide_dead_makers = False

    def _dead_makers(self, makers):
        dead = set()
        if not self.elide_dead_makers:
            return dead
        for i, m in enumerate(makers):
            if m.maker_type == 'early' and not self.training:
                dead.add(id(m))
            if m.maker_type == 'rsu' and any(n.maker_type in ('rsu', 'car') for n in makers[i + 1:]):
                dead.add(id(m))
        return dead

    # MI355X knob (pipeline mode only: needs the VFEs' persistent buffers): the early-fusion BEV maker and the ego branch pillarise the same
    # cloud on the same grid -- share the pillar list (DynamicPillarVFE._voxelize).  Off when a corrector moves the points in place.
    share_voxelization = True

    def _run_modules(self, batch_dict):
        from ..bev_layers.bev_maker import BEVMaker
        makers = [m for m in self.module_list if isinstance(m, BEVMaker)]
        dead = self._dead_makers(makers)
        if (self.share_voxelization and getattr(self, 'corrector', None) is None and batch_dict['points'].is_cuda
                and any(m.maker_type == 'early' and id(m) not in dead for m in makers) and getattr(self, 'vfe', None) is not None):
            batch_dict['_pcp_vox_share'] = {}
        # a module in front of the fusion that corrects the points IN PLACE (HunterJr's k_apply_flow) would race with makers still
        # reading them on their own streams: such models run the sequential chain
        if not self.overlap_makers or not makers or not batch_dict['points'].is_cuda or getattr(self, 'corrector', None) is not None:
            for cur_module in self.module_list:
                if id(cur_module) in dead:
                    continue
                batch_dict = cur_module(batch_dict)
            return batch_dict
        main = torch.cuda.current_stream()
        if getattr(self, '_maker_streams', None) is None or len(self._maker_streams) != len(makers):
            self._maker_streams = [torch.cuda.Stream() for _ in makers]
        # the makers read only the batch's points: in the pipelined mode (pcdet/models/pipelined.py) those were written on a side stream whose
        # event is handed in, so the maker streams of batch i+1 need not wait for the main stream to finish batch i's head / decode / NMS
        ready = batch_dict.get('_pcp_points_ready', None) or main.record_event()
        joins = []

        def join_all():
            for ev in joins:
                main.wait_event(ev)
            for t in list(batch_dict.get('bev_img', {}).values()) + [batch_dict.get('bev_img_early', None)]:
                if t is not None:
                    t.record_stream(main)               # allocated on a side stream, consumed on the main one
            del joins[:]
        mi = 0
        for cur_module in self.module_list:
            if isinstance(cur_module, BEVMaker):
                s = self._maker_streams[mi]
                mi += 1
                if id(cur_module) in dead:
                    continue
                s.wait_event(ready)
                batch_dict['points'].record_stream(s)             # main-stream allocation read on the side stream
                with torch.cuda.stream(s):
                    batch_dict = cur_module(batch_dict)            # dict updates happen in program order (car replaces rsu)
                    joins.append(s.record_event())
                continue
            if joins and cur_module is self.v2x_mid_fusion:
                join_all()
            batch_dict = cur_module(batch_dict)
        if joins:                                                  # no fusion module consumed the maps: still leave with everything joined
            join_all()
        return batch_dict

    def pose_arrays(self, metadata, batch_size):
        """name -> host array: every pose-derived launch parameter of a static (graph-mode) forward, from the metadata alone -- the BEV makers'
        pose / presence tables and the fusion module's warp affines, under the names the modules use with the pose table"""
        from ..bev_layers.bev_maker import BEVMaker
        out = {}
        makers = [m for m in self.module_list if isinstance(m, BEVMaker)]
        dead = self._dead_makers(makers)
        last = None
        for m in makers:
            if id(m) in dead:
                continue
            out.update(m.pose_arrays(metadata, batch_size))
            if m.maker_type in ('rsu', 'car'):
                last = m                                     # every rsu / car maker REPLACES batch_dict['bev_img']
        fusion = getattr(self, 'v2x_mid_fusion', None)
        if fusion is not None and last is not None and getattr(fusion, '_last_map_hw', None) is not None:
            order = last.static_agent_order(metadata, batch_size)
            th = fusion.theta_array(metadata, order, *fusion._last_map_hw)
            if th.shape[0]:
                out['fusion.thetas'] = th
        return out

    def forward(self, batch_dict):
        if (self.training and getattr(self, 'corrector', None) is not None and type(self.backbone_2d).__name__.startswith('SCConvBackbone')
                and not batch_dict['points'].is_cuda):
            # before any module runs (the VFE would pillarise a host batch on the CPU path first)
            raise NotImplementedError('training HunterJr behind an SC backbone (the nuScenes corrector, pointpillar_jr_corr_withmap) runs on '
                                      'the HIP training path only and the points of this batch are on %s: off the GPU this model is inference only'
                                      % batch_dict['points'].device)
        batch_dict = self._run_modules(batch_dict)
        if self.training:
            tape = batch_dict.get('_pcp_tape', [])
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': hip_loss(loss, tape, getattr(self, '_pcp_grad_ready_hook', None))}, tb_dict, disp_dict
        pred_dicts, recall_dicts = self.post_processing(batch_dict)
        if self.model_cfg.get('RETURN_BATCH_DICT', False):
            return pred_dicts, batch_dict
        return pred_dicts, recall_dicts

    def get_training_loss(self):
        disp_dict = {}
        rd = lambda t: t.item()
        loss_rpn, tb_dict = self.dense_head.get_loss()
        tb_dict = {'loss_rpn': rd(loss_rpn), **tb_dict}
        loss = loss_rpn
        if self.corrector is not None:
            loss_corrector, tb_dict = self.corrector.get_training_loss(tb_dict)
            tb_dict['loss_corrector'] = rd(loss_corrector)
            loss = loss + loss_corrector
        if self.v2x_mid_fusion is not None:
            distill = self.v2x_mid_fusion.loss_dict['loss_distill']
            loss = loss + distill
            tb_dict['loss_mid_fusion_distill'] = rd(distill) if hasattr(distill, 'item') else 0.0
        tb_dict['loss_total'] = rd(loss)
        return loss, tb_dict, disp_dict

    def post_processing(self, batch_dict):
        post_process_cfg = self.model_cfg.POST_PROCESSING
        final_pred_dict = batch_dict['final_box_dicts']
        recall_dict = {}
        for index in range(batch_dict['batch_size']):
            recall_dict = self.generate_recall_record(
                box_preds=final_pred_dict[index]['pred_boxes'], recall_dict=recall_dict, batch_index=index,
                data_dict=batch_dict, thresh_list=post_process_cfg.RECALL_THRESH_LIST)
        return final_pred_dict, recall_dict
