/*
 * pcp_hip_train.h -- C ABI of libpcp_hip.so, training half (SURVEY.md 8 row a15 + appendix C: config 5, DiscoNet).
 *
 * Same conventions as pcp_hip.h (device pointers, caller-owned workspaces, explicit stream, int status, no allocation, no
 * synchronisation).  The reference trains through torch.autograd + cuDNN; there is no native training ABI to mirror, so each
 * entry point names the autograd node(s) of the reference module it stands for.  Forward convolutions of a training step are
 * the inference entry points of pcp_hip.h called with identity folding (raw weights, zero bias, relu = 0); data gradients of
 * convolutions are the same entry points called with transposed / flipped weights.
 */
#ifndef PCP_HIP_TRAIN_H
#define PCP_HIP_TRAIN_H

#include "pcp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------------------------
 * BatchNorm in train() mode + ReLU on (rows, c) row-major / NHWC float32 (rows = B*H*W or N' points), c % 4 == 0, c <= 1024.
 * Replaces nn.BatchNorm2d / nn.BatchNorm1d (+ nn.ReLU) forward and backward as used by
 *   pcdet/models/backbones_2d/base_bev_backbone.py:37-44,56,67 (eps 1e-3, momentum 0.01),
 *   pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:29,40-43, pcdet/models/dense_heads/center_head.py:26,80,
 *   pcdet/models/bev_layers/v2x_fusion_disco.py:13-16,53,60 (eps 1e-5, momentum 0.1).
 * pcp_bn_train_stats: batch mean / biased variance (float64 accumulation) -> scale = gamma * invstd, shift = beta - mean * scale,
 *   saved mean / invstd, running stats updated in place with the unbiased variance (NULL, NULL: not tracked).
 * pcp_scale_shift_act: out = act(x * scale + shift) (one fma per element -- the same expression the backward mask recomputes).
 * pcp_bn_act_backward: given dout = dL/d relu(bn(x)): dgamma, dbeta (written or accumulated) and
 *   dx = scale * (dz - mean(dz) - xhat * mean(dz * xhat)), dz = dout * [bn(x) > 0]; dx may alias dout.
 * workspace: pcp_bn_workspace_bytes(c) bytes.
 * ------------------------------------------------------------------------------------------------------------------ */
size_t pcp_bn_workspace_bytes(int32_t c);
int pcp_bn_train_stats(const float *x, int64_t rows, int32_t c, int32_t ld, const float *gamma, const float *beta, float eps,
                       float momentum, float *running_mean, float *running_var, void *workspace, float *scale, float *shift,
                       float *mean, float *invstd, void *stream);
int pcp_scale_shift_act(const float *x, int64_t rows, int32_t c, int32_t ld_x, const float *scale, const float *shift, int32_t relu,
                        float *out, int32_t ld_out, void *stream);
int pcp_bn_act_backward(const float *dout, int32_t ld_dout, const float *x, int32_t ld_x, int64_t rows, int32_t c, const float *scale,
                        const float *shift, const float *mean, const float *invstd, int32_t relu, void *workspace, float *dgamma,
                        float *dbeta, int32_t accumulate, float *dx, int32_t ld_dx, void *stream);
/* Cross-rank BatchNorm (nn.SyncBatchNorm: reference tools/train.py:37,128-129 `--sync_bn`): the two calls above split where the ranks
 * exchange.  sums = 2 * c float64 on the device ([sum x | sum x^2] forward, [sum dz | sum dz * xhat] backward); the host all-reduces them
 * (and the row count) over the ranks between the two halves.  Forward statistics then come from the global sums; backward dgamma / dbeta
 * from the LOCAL sums (the gradient all-reduce combines them, as DDP does) and the mean terms of dx from the global ones. */
int pcp_bn_train_sums(const float *x, int64_t rows, int32_t c, int32_t ld, void *workspace, double *sums, void *stream);
int pcp_bn_train_stats_from_sums(const double *sums, int64_t total_rows, int32_t c, const float *gamma, const float *beta, float eps,
                                 float momentum, float *running_mean, float *running_var, float *scale, float *shift, float *mean,
                                 float *invstd, void *stream);
int pcp_bn_bwd_sums(const float *dout, int32_t ld_dout, const float *x, int32_t ld_x, int64_t rows, int32_t c, const float *scale,
                    const float *shift, const float *mean, const float *invstd, int32_t relu, void *workspace, double *sums, void *stream);
int pcp_bn_bwd_apply_from_sums(const float *dout, int32_t ld_dout, const float *x, int32_t ld_x, int64_t rows, int32_t c, const float *scale,
                               const float *shift, const float *mean, const float *invstd, int32_t relu, const double *local_sums,
                               const double *global_sums, int64_t total_rows, void *workspace, float *dgamma, float *dbeta,
                               int32_t accumulate, float *dx, int32_t ld_dx, void *stream);
/* out[c] (+)= sum over rows (bias gradients); workspace as above */
int pcp_colsum(const float *x, int64_t rows, int32_t c, int32_t ld, void *workspace, float *out, int32_t accumulate, void *stream);
/* dst[r, :c] += alpha * src[r, :c] (gradient fan-in) */
int pcp_accumulate(float *dst, int32_t ld_dst, const float *src, int32_t ld_src, int64_t rows, int32_t c, float alpha, void *stream);
/* out (B, 2h, 2w, c): in at the even pixels, zero elsewhere.  The data gradient of a stride-2 3x3 conv (ZeroPad2d(1) + Conv2d s2,
 * base_bev_backbone.py:33-36) is the stride-1 conv of this map with the flipped, transposed weights. */
int pcp_dilate2x(const float *in, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t ld_in, float *out, int32_t ld_out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Weight gradients (cuDNN backward-filter of nn.Conv2d / nn.ConvTranspose2d), fp32 MFMA with the pixel as contraction index;
 * split-K partials in the workspace are reduced in a fixed order (deterministic).
 * pcp_conv3x3_wgrad: desc as for pcp_conv3x3 (ld_in = pixel stride of x, ld_out = pixel stride of dy; cout_pad / relu ignored);
 *   dw is PyTorch's (cout, cin, 3, 3) float32, written or accumulated.  cin % 4 == 0, cout % 4 == 0.
 * pcp_pointwise_wgrad: out[n][k] (+)= sum_r a[map_a(r)][n] * b[map_b(r)][k] with n < a.channels, k < b.channels; a row map is the
 *   identity (lattice = 0) or sends r = (b, y, x) on a (grid_h, grid_w) grid to pixel (b, 2y + ky, 2x + kx) of the (2 grid_h,
 *   2 grid_w) map (the taps of Conv2d k2 s2 / ConvTranspose2d k2 s2, base_bev_backbone.py:48-69).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  const float *ptr;
  int32_t ld, channels;
  int32_t lattice, grid_h, grid_w, ky, kx;
} pcp_rowmap_t;

size_t pcp_conv3x3_wgrad_workspace_bytes(const pcp_conv3x3_t *desc);
int pcp_conv3x3_wgrad(const pcp_conv3x3_t *desc, const float *x, const float *dy, void *workspace, size_t workspace_bytes, float *dw,
                      int32_t accumulate, void *stream);
size_t pcp_pointwise_wgrad_workspace_bytes(int64_t rows, int32_t n, int32_t k);
int pcp_pointwise_wgrad(const pcp_rowmap_t *a, const pcp_rowmap_t *b, int64_t rows, void *workspace, size_t workspace_bytes,
                        float *out, int32_t ld_out, int32_t accumulate, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * a15  CenterHead training: target assignment, focal + L1 losses and their gradients, DiscoNet distillation loss.
 * Replaces: pcdet/models/dense_heads/center_head.py:104-164,166-268 (assign_targets: per-frame .cpu() + python loop over
 *           boxes), pcdet/models/model_utils/centernet_utils.py:8-68 (gaussian_radius, gaussian2D, draw_gaussian_to_heatmap),
 *           center_head.py:270-300 (get_loss), pcdet/utils/loss_utils.py:264-375 (neg_loss_cornernet, _reg_loss,
 *           RegLossCenterNet) and pcdet/models/bev_layers/v2x_fusion_disco.py:119-123 (loss_distill), plus their autograd.
 * One head (all five configs); classes of gt_boxes[..., 7] in 1..num_class, 0 = padding row (dataset.py collate_batch).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t batch, h, w;            /* feature map */
  int32_t num_class;
  int32_t k;                      /* NUM_MAX_OBJS */
  float stride;                   /* FEATURE_MAP_STRIDE */
  float voxel_x, voxel_y, min_x, min_y;
  float gaussian_overlap;         /* GAUSSIAN_OVERLAP */
  int32_t min_radius;             /* MIN_RADIUS */
} pcp_target_t;

/* gt_boxes (B, max_boxes, 8) [x,y,z,dx,dy,dz,heading,class] (max_boxes <= 1024).  Outputs: heatmap (B, H, W, num_class) NHWC,
 * target_boxes (B, k, 8) = [dx, dy, z, log dims(3), cos, sin], inds (B, k) int32 flat y*W+x, mask (B, k) int32. */
int pcp_centerhead_targets(const pcp_target_t *desc, const float *gt_boxes, int32_t max_boxes, float *heatmap, float *target_boxes,
                           int32_t *inds, int32_t *mask, void *stream);

typedef struct {
  int32_t batch, h, w;
  int32_t ld;                     /* pixel stride of the head-map buffer */
  int32_t ld_d;                   /* pixel stride of the gradient buffer (channel numbering identical to the head buffer) */
  int32_t num_class, ch_hm;       /* heat-map logits at channels [ch_hm, ch_hm + num_class) */
  int32_t reg_ch[8];              /* channel of each regression code in HEAD_ORDER: center(2), center_z, dim(3), rot(2) */
  int32_t k;
  float cls_weight, loc_weight, code_weights[8];
} pcp_headloss_t;

size_t pcp_loss_workspace_bytes(void);
/* losses (4,) float32 device: [hm_loss * cls_weight, loc_loss * loc_weight, their sum, num_pos].  dhead (B, H, W, ld_d) or NULL:
 * every channel written (zero where no loss term reads the map), scaled by grad_scale. */
int pcp_centerhead_loss(const pcp_headloss_t *desc, const float *head, const float *heatmap, const float *target_boxes,
                        const int32_t *inds, const int32_t *mask, float grad_scale, void *workspace, float *losses, float *dhead,
                        void *stream);
/* ------------------------------------------------------------------------------------------------------------------
 * a15x  CenterHead training for several heads, velocity codes and the IoU branch (the nuScenes PointPillar-Jr head).
 * Replaces: center_head.py:168-268 (assign_targets: per head and frame a class-name filter in python, .cpu(), the per-box loop),
 *           :213-242 with dense_heads/box_utils.py:6-67 (the IoU target: decode the prediction at each ground-truth centre,
 *           axis-aligned IoU), :105-166 with 9- and 10-column rows (velocity targets, the IoU column), :274-300 (get_loss over
 *           every head) and their autograd.  The one-head, 8-code entry points above keep serving the five V2X-Sim configs.
 * ------------------------------------------------------------------------------------------------------------------ */
#define PCP_TGT_MAX_CLASSES 32
#define PCP_HEADLOSS_MAX_CODES 16

typedef struct {
  int32_t num_class;                              /* classes of this head = channels of its heat map */
  int32_t class_to_local[PCP_TGT_MAX_CLASSES];    /* indexed by the class column of gt_boxes (0 = padding row): 0 = not in this head,
                                                   * else the 1-based index inside the head */
  float *heatmap;                                 /* (B, H, W, num_class) NHWC */
  float *target_boxes;                            /* (B, k, T) */
  int32_t *inds, *mask;                           /* (B, k) */
  const float *head;                              /* raw head maps (B, H, W, ld) for the IoU target; read only when with_iou */
  int32_t ld, ch_center, ch_z, ch_dim, ch_rot;         /* ch_z is validated but not read: the IoU is that of the BEV rectangles */
} pcp_target_head_t;

/* ONE launch for every (frame, head); desc->num_class is not read (each head brings its own).
 * gt_boxes (B, max_boxes, box_width), box_width 8 = [x,y,z,dx,dy,dz,heading,class] or 10 = [.., heading, vx, vy, class]; max_boxes <= 1024;
 * gt_boxes is only read (the reference rewrites the class column in place, center_head.py:203-204: the caller checks that this is inert).
 * A row's slot is its rank among the rows of its head in row order; ranks >= k are dropped.
 * target_boxes columns, T = 8 (+2 if box_width = 10) (+1 if with_iou): [dx, dy, z, log dims(3), cos, sin, (vx, vy), (iou)],
 * iou = 2 * axis_aligned_iou(box decoded from head at the clamped, truncated centre, gt box) - 1, a constant of the step (no gradient).
 * Rows are finite by contract: a NaN velocity is copied as it is and makes the loss NaN. */
int pcp_centerhead_targets_ext(const pcp_target_t *desc, const pcp_target_head_t *heads, int32_t n_heads, const float *gt_boxes,
                               int32_t max_boxes, int32_t box_width, int32_t with_iou, void *stream);

typedef struct {
  const float *head;              /* raw head maps (B, H, W, ld) */
  float *dhead;                   /* gradient (B, H, W, ld_d), same channel numbering; NULL for every head or for none */
  const float *heatmap, *target_boxes;
  const int32_t *inds, *mask;
  int32_t ld, ld_d, ch_hm, num_class;
  int32_t n_codes;                /* <= PCP_HEADLOSS_MAX_CODES */
  int32_t reg_ch[PCP_HEADLOSS_MAX_CODES];   /* channel of each regression code, in HEAD_ORDER concatenation order */
  int32_t tb_width;               /* row width of target_boxes; must equal n_codes (column j pairs with code j, center_head.py:286-292) */
} pcp_headloss_head_t;

typedef struct {
  int32_t batch, h, w, k;
  float cls_weight, loc_weight, code_weights[PCP_HEADLOSS_MAX_CODES];
} pcp_headloss_ext_t;

size_t pcp_centerhead_loss_ext_workspace_bytes(int32_t n_heads);
/* All heads in four launches, whatever n_heads (<= PCP_DET_MAX_HEADS).  losses (n_heads, 4) = per head [hm_loss * cls_weight,
 * loc_loss * loc_weight, their sum, num_pos]; total (1,) = the sum of the third column, added in head order.  The arithmetic per head
 * is pcp_centerhead_loss's; block partials are float64 and added in a fixed order, and the gradient of boxes that share a cell is added
 * in slot order, so the result is the same bits on every run.  dhead of every head is written completely (zero where no term reads the
 * map), scaled by grad_scale.  Targets are finite by contract: NaN targets (the reference's isnotnan mask) are out of scope. */
int pcp_centerhead_loss_ext(const pcp_headloss_ext_t *desc, const pcp_headloss_head_t *heads, int32_t n_heads, float grad_scale,
                            void *workspace, size_t workspace_bytes, float *losses, float *total, void *stream);

/* loss (1,) = weight * mean smooth_l1(softmax_c(fused) - softmax_c(early)); dfused (pixels, ld_d) written or accumulated (NULL: none);
 * c <= 512.  Shares the workspace of pcp_centerhead_loss. */
int pcp_distill_loss(const float *fused, int32_t ld_f, const float *early, int32_t ld_e, int64_t pixels, int32_t c, float weight,
                     float grad_scale, void *workspace, float *loss, float *dfused, int32_t ld_d, int32_t accumulate, void *stream);
/* HunterJr teacher-BEV term (hunter_jr.py:352-365): loss (1,) = mean over the pixels with ||teacher[p, :]||_2 > thresh of
 * sum_c smooth_l1(fused[p, c] - teacher[p, c]) (nan when no pixel qualifies, as torch's mean of an empty selection).  Value only: the
 * reference keeps it in forward_return_dict['loss_dtl_bev_img'] and never adds it to the training loss (hunter_jr.py:490-494).
 * workspace: pcp_loss_workspace_bytes() bytes. */
int pcp_masked_smooth_l1_rows(const float *fused, int32_t ld_f, const float *teacher, int32_t ld_t, int64_t pixels, int32_t c, float thresh,
                              void *workspace, float *loss, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training-mode PillarFeatureNet (BatchNorm1d with batch statistics splits the fused inference kernel at its two global
 * reductions).  Per-point tensors are in BUCKET ORDER (the counting sort pcp_voxelize leaves in its workspace; slot s, 0 <= s < N');
 * the Linear layers run on pcp_pointwise, their gradients on pcp_pointwise / pcp_pointwise_wgrad, BatchNorm on pcp_bn_*.
 * Replaces dynamic_pillar_vfe.py:110-126 (features), :35-46 (scatter_max + concat) and their autograd (scatter_max backward
 * routes to one arg-max row per (pillar, channel); ties -> first row in bucket order), pointpillar_scatter.py:14-37.
 *   features      fbuf (N', FW) = [raw(num_raw), f_cluster(3), f_center(3), 0...], FW = 16 if num_raw + 6 <= 16 else 32;
 *                 slot_pillar (N',) int32 pillar rank of each slot.  Widths 3, 4, 5 and 11 have a kernel of their own; every other
 *                 width runs pcp_pfn_train_features_w
 *   features_w    the same rows (the same bits) for ANY raw width PCP_PFN_TRAIN_MIN_RAW <= num_raw <= PCP_PFN_TRAIN_MAX_RAW, the width a
 *                 run-time argument: row_stride >= 1 + num_raw floats (the cloud may carry columns the PFN does not read), fw = 16 or 32
 *                 with num_raw + 6 <= fw; anything else is PCP_ERR_ARG and nothing is launched
 *   mid           in1 (N', 64) = [relu(x0 * scale0 + shift0), per-pillar max of it]; arg0 (P, 32) int32 arg-max slot
 *   out           pillar_features (P, 64) (may be NULL), arg1 (P, 64), canvas (B, ny, nx, 64) rows (may be NULL)
 *   route_out     dz1 (kept_rows, 64) = 0 except dz1[arg1[p, c], c] = dcanvas[cell(p), c]  (or dpillar[p, c]; exactly one non-NULL)
 *   route_mid     da0 (N', 32) = din1[:, :32] + [slot == arg0] * sum over the pillar of din1[:, 32:]
 * ------------------------------------------------------------------------------------------------------------------ */
#define PCP_PFN_TRAIN_MIN_RAW 3
#define PCP_PFN_TRAIN_MAX_RAW 26 /* 26 + 6 = the 32 floats of the wider feature row */
int pcp_pfn_train_features(const float *points, int64_t n, int32_t row_stride, int32_t num_raw, const pcp_grid_t *grid,
                           const void *vox_workspace, float *fbuf, int32_t *slot_pillar, void *stream);
int pcp_pfn_train_features_w(const float *points, int64_t n, int32_t row_stride, int32_t num_raw, int32_t fw, const pcp_grid_t *grid,
                             const void *vox_workspace, float *fbuf, int32_t *slot_pillar, void *stream);
int pcp_pfn_train_mid(const pcp_grid_t *grid, const void *vox_workspace, int64_t n, const float *x0, const float *scale0,
                      const float *shift0, float *in1, int32_t *arg0, void *stream);
int pcp_pfn_train_out(const pcp_grid_t *grid, const void *vox_workspace, int64_t n, const float *x1, const float *scale1,
                      const float *shift1, float *pillar_features, int32_t *arg1, float *canvas, void *stream);
int pcp_pfn_train_route_out_grad(const pcp_grid_t *grid, const void *vox_workspace, int64_t n, int64_t kept_rows, const float *dcanvas,
                                 const float *dpillar, const int32_t *arg1, float *dz1, void *stream);
int pcp_pfn_train_route_mid_grad(const pcp_grid_t *grid, const void *vox_workspace, int64_t n, const float *din1, const int32_t *arg0,
                                 float *da0, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * DiscoNet mid fusion, training: last weightor stage and the backward of softmax-over-agents + weighted sum.
 * Replaces the autograd graph of pcdet/models/bev_layers/v2x_fusion_disco.py:22-24 and :109-115.  Agent maps are constants
 * (transform_bev_img is @torch.no_grad, :29): only map 0 (ego) receives a gradient.  n_agents <= 8, c <= 256.
 * pcp_disco_weight_logits: logits[p, a] = relu(<h2_a[p, 0:16], w4> + b4).
 * pcp_disco_fuse_backward: dmap0 = softmax_a(logits)[0] * dfused;  dh2_a[p, :] = dlogit_a * [logit_a > 0] * w4;
 *   dw4 (16), db4 (1) written or accumulated.  *_host arrays are HOST arrays of device pointers.
 * ------------------------------------------------------------------------------------------------------------------ */
int pcp_disco_weight_logits(const float *const *h2_host, int32_t n_agents, int32_t ld_h, const float *w4, const float *b4,
                            int64_t pixels, float *logits, int32_t ld_w, void *stream);
size_t pcp_disco_fuse_backward_workspace_bytes(void);
int pcp_disco_fuse_backward(const float *const *maps_host, int32_t n_agents, int32_t ld_map, int32_t c, const float *logits, int32_t ld_w,
                            const float *dfused, int32_t ld_df, const float *const *h2_host, int32_t ld_h, const float *w4,
                            int64_t pixels, float *dmap0, int32_t ld_dm, float *const *dh2_host, void *workspace, float *dw4, float *db4,
                            int32_t accumulate, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * a16  AnchorHeadSingle training (MODEL.NAME PointPillar): target assignment, the three losses and dL/d(head maps).
 * Replaces: pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:37-210 (assign_targets: python loop over frames x
 *           anchor classes, an anchors x boxes IoU matrix and .nonzero() host syncs per pair), pcdet/utils/box_utils.py:291-340
 *           (boxes3d_nearest_bev_iou), pcdet/utils/box_coder_utils.py:13-44 (ResidualCoder.encode_torch),
 *           pcdet/models/dense_heads/anchor_head_template.py:99-216 (get_cls_layer_loss, add_sin_difference, get_direction_target,
 *           get_box_reg_layer_loss, get_loss), pcdet/utils/loss_utils.py:9-148,180-208 (SigmoidFocalClassificationLoss,
 *           WeightedSmoothL1Loss, WeightedCrossEntropyLoss) and their autograd.
 * Covers POS_FRACTION < 0, MATCH_HEIGHT False, NORM_BY_NUM_EXAMPLES False, ResidualCoder without sin/cos (every anchor YAML of the
 * reference).  Anchors are flat in the order of torch.cat(anchors, dim=-3).view(-1, 7): index = (y * W + x) * A + slot.
 * ------------------------------------------------------------------------------------------------------------------ */
#define PCP_ANCHOR_MAX_SLOTS 32
#define PCP_ANCHOR_MAX_GROUPS 8
typedef struct {
  int32_t batch, h, w;                          /* feature map */
  int32_t anchors_per_loc;                      /* A */
  int32_t num_class;                            /* len(CLASS_NAMES); box class c names CLASS_NAMES[c - 1] (0 wraps to the last, like numpy) */
  int32_t num_groups;                           /* ANCHOR_GENERATOR_CONFIG entries (anchor classes) */
  int32_t slot_group[PCP_ANCHOR_MAX_SLOTS];     /* anchor class of each per-location slot */
  int32_t group_class[PCP_ANCHOR_MAX_GROUPS];   /* 0-based index of the anchor class's class_name in CLASS_NAMES (-1: not a detected class) */
  float matched[PCP_ANCHOR_MAX_GROUPS], unmatched[PCP_ANCHOR_MAX_GROUPS];
} pcp_anchor_assign_t;

size_t pcp_anchor_assign_workspace_bytes(const pcp_anchor_assign_t *desc, int32_t max_boxes);
/* anchors (H*W*A, 7); gt_boxes (B, max_boxes, 8) [x,y,z,dx,dy,dz,heading,class], max_boxes <= 1024 (0: no boxes at all).
 * Outputs: labels (B, N) int32 (-1 ignored, 0 background, > 0 class), reg_targets (B, N, 7), reg_weights (B, N). */
int pcp_anchor_assign_targets(const pcp_anchor_assign_t *desc, const float *anchors, const float *gt_boxes, int32_t max_boxes,
                              void *workspace, size_t workspace_bytes, int32_t *labels, float *reg_targets, float *reg_weights,
                              void *stream);

typedef struct {
  int32_t batch, h, w;
  int32_t ld, ld_d;                             /* pixel stride of the head buffer / of the gradient buffer (same channel numbering) */
  int32_t anchors_per_loc, num_class, num_dir_bins;     /* num_dir_bins 0: no direction classifier */
  int32_t ch_cls, ch_box, ch_dir;               /* first channel of conv_cls / conv_box / conv_dir_cls outputs */
  float dir_offset, dir_period;                 /* DIR_OFFSET, 2 pi / NUM_DIR_BINS */
  float cls_weight, loc_weight, dir_weight, code_weights[7];
} pcp_anchor_loss_t;

size_t pcp_anchor_loss_workspace_bytes(int32_t batch);
/* losses (5,) float32 device: [rpn_loss_cls, rpn_loss_loc, rpn_loss_dir, rpn_loss, positives].  dhead (B, H, W, ld_d) or NULL: every
 * channel written (padding channels zero), scaled by grad_scale. */
int pcp_anchor_loss(const pcp_anchor_loss_t *desc, const float *head, const float *anchors, const int32_t *labels,
                    const float *reg_targets, float grad_scale, void *workspace, size_t workspace_bytes, float *losses, float *dhead,
                    void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * a17  HunterJr training branch (configs 1 / 2).
 * Replaces: pcdet/models/bev_layers/hunter_jr.py:165-196 (_build_meta: two torch.unique + scatter_max / scatter_min), :42-76
 *           (HunterObjectHead: scatter_mean, three scatter_max, cat), :198-260 (assign_target), :106-113 (get_loss_distill), :401-495
 *           (get_training_loss), pcdet/models/loss_fnc/pcaccum_ce_lovasz_loss.py:20-71, lovasz_softmax.py:56-95,
 *           hunter_toolbox.py:42-62 (quat2mat), :161-184 (remove_gt_boxes_outside_range), :187-219 (hard_mining_regression_loss), and the
 *           autograd of hunter_toolbox.py:8-39 (bilinear sampling incl. its position gradient), :65-91 (bev_scatter), hunter_jr.py:281-285.
 * Rows of `points` are [frame, x, y, z, ..., sweep, instance]; foreground = instance > -1 (hunter_jr.py:323).
 * ------------------------------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t batch, max_inst, num_sweeps;          /* key = (frame * max_inst + instance) * num_sweeps + sweep; max_inst = gt_boxes.shape[1] */
  int32_t sweep_col, inst_col;                  /* columns of the point rows */
} pcp_hunter_meta_t;

size_t pcp_hunter_meta_workspace_bytes(const pcp_hunter_meta_t *desc, int64_t n);
/* fg_idx / fg_local (n): rows of the foreground points in ascending order and their local index (locals2fg);
 * local_key / local_inst (batch*max_inst*num_sweeps): locals_bis / inst2locals; inst_key / inst_first / inst_last (batch*max_inst):
 * instance_bi / indices_locals_min_sweep / indices_locals_max_sweep; counts (4) int32 = [n_fg, n_local, n_inst, rows with a key outside
 * the table (treated as background)]. */
int pcp_hunter_meta(const pcp_hunter_meta_t *desc, const float *points, int64_t n, int32_t row_stride, void *workspace, size_t workspace_bytes,
                    int32_t *fg_idx, int32_t *fg_local, int32_t *local_key, int32_t *local_inst, int32_t *inst_key, int32_t *inst_first,
                    int32_t *inst_last, int32_t *counts, void *stream);

/* torch_scatter.scatter_max(src[row_index], seg): out (n_seg, c) and the arg-max row (first maximal row) per (segment, channel);
 * backward: dsrc[row_index[arg[s, ch]], ch] += dout[s, ch]. */
int pcp_segment_max(const float *src, int32_t ld_src, const int32_t *row_index, int64_t rows, const int32_t *seg, int64_t n_seg, int32_t c,
                    float *out, int32_t ld_out, int32_t *arg, void *stream);
int pcp_segment_max_backward(const float *dout, int32_t ld_dout, const int32_t *arg, int64_t n_seg, int32_t c, const int32_t *row_index,
                             float *dsrc, int32_t ld_dsrc, void *stream);
/* dst[row_index[r], :c] += src[r, :c]  (row_index injective) */
int pcp_rows_scatter_add(const float *src, int32_t ld_src, const int32_t *row_index, int64_t rows, int32_t c, float *dst, int32_t ld_dst,
                         void *stream);
/* centroid (n_local, 3) = scatter_mean(fg xyz); centered (n_fg, ld) = [xyz - centroid[local], 0 ...]; workspace >= 32 * n_local bytes */
int pcp_hunter_local_centroids(const float *points, int32_t row_stride, const int32_t *fg_idx, const int32_t *fg_local, int32_t n_fg,
                               int32_t n_local, void *workspace, size_t workspace_bytes, float *centroid, float *centered, int32_t ld_centered,
                               void *stream);
/* out (n_local, ld) = [lf0 | gf[inst] | centroid | centroid[last local of inst] | 0 ...]   (hunter_jr.py:64-69) and its backward */
int pcp_hunter_object_cat(const float *lf0, const float *gf, const float *centroid, const int32_t *local_inst, const int32_t *inst_last,
                          int32_t n_local, int32_t c, float *out, int32_t ld_out, void *stream);
int pcp_hunter_object_cat_backward(const float *dcat, int32_t ld, const int32_t *inst_first, const int32_t *inst_last, int32_t n_local,
                                   int32_t n_inst, int32_t c, float *dlf0, float *dgf, void *stream);

typedef struct {
  int64_t n;
  int32_t stride, n_fg, n_local, n_inst, c;
  int32_t batch, max_inst, num_sweeps;
  const float *points;                          /* rows BEFORE the in-place correction */
  const float *gt_boxes;                        /* (batch, max_inst, gt_stride): the centre x, y in columns 0, 1 */
  const float *instances_tf;                    /* (batch, max_inst, num_sweeps, 3, 4) */
  const int32_t *fg_idx, *fg_local, *local_key, *local_inst, *inst_key;
  const float *head;                            /* (n, ld_head): [cls(3) | flow(3) | embedding(2)] */
  int32_t ld_head;
  const float *local_feat;                      /* (n, ld): point head's local feature */
  int32_t ld_local_feat;
  const float *locals_feat;                     /* (n_local, ld): object head's local feature */
  int32_t ld_locals_feat;
  const float *locals_tf;                       /* (n_local, ld): [t(3) | quaternion xyzw(4)] */
  int32_t ld_locals_tf;
  float coef_fg, coef_locals;                   /* LOSS_HARD_MINING_STATIC_FG_COEF / _LOCALS_COEF */
  float grad_scale;
  float *dhead;                                 /* (n, ld_dhead), every channel written */
  int32_t ld_dhead;
  float *dlocal_feat_fg;                        /* (n_fg, c): gradient of local_feat at the foreground rows */
  float *dlocals_feat;                          /* (n_local, c) */
  float *dlocals_tf;                            /* (n_local, ld_dlocals_tf), every channel written */
  int32_t ld_dlocals_tf;
  float *losses;                                /* (8): l_points_cls, l_points_embed, l_fg_offset, l_locals_transl, l_locals_rot, l_recon,
                                                   l_dtl_locals_feat, their sum */
  int32_t *labels;                              /* (n): point class targets 0 background / 1 static / 2 moving foreground */
  float *tgt_embedding, *tgt_offset;            /* optional (n_fg, 2) / (n_fg, 3) */
  int32_t gt_stride;                            /* floats per gt_boxes row, PCP_GT_BOX_MIN_WIDTH .. PCP_GT_BOX_MAX_WIDTH (10 with velocity);
                                                   0 = 8, the rows of the V2X-Sim models */
} pcp_hunter_loss_t;

size_t pcp_hunter_loss_workspace_bytes(int64_t n, int32_t n_fg, int32_t n_local, int32_t c);
int pcp_hunter_losses(const pcp_hunter_loss_t *desc, void *workspace, size_t workspace_bytes, void *stream);

/* fused = map0 * w0 + map1 * w1, (w0, w1) = softmax(logits[:, 0:2]); cat rows hold [map0 (c) | map1 (c)].  dcat (pixels, ld_dcat) and
 * dlogits (pixels, ld_dlogits; channels >= 2 zeroed) are overwritten. */
int pcp_softmax_fuse2_backward(const float *dfused, int32_t ld_df, const float *cat, int32_t ld_cat, const float *logits, int32_t ld_logits,
                               int64_t pixels, int32_t c, float *dcat, int32_t ld_dcat, float *dlogits, int32_t ld_dlogits, void *stream);
/* backward of pcp_bev_scatter_mean through the workspace its forward left: rows with dyn_mask go to dfeat_dyn (overwritten), the others are
 * ADDED to dfeat_acc */
int pcp_bev_scatter_mean_backward(const void *scatter_workspace, int32_t batch, int32_t h, int32_t w, int64_t n, const float *dmap,
                                  int32_t ld_dmap, int32_t c, const uint8_t *dyn_mask, float *dfeat_acc, int32_t ld_acc, float *dfeat_dyn,
                                  int32_t ld_dyn, void *stream);
/* backward of pcp_bev_sample_bilinear: dbev += (atomic); with bev != NULL also dxyz[i, 0..1] += d loss / d (x, y) of point i */
int pcp_bev_sample_bilinear_backward(const float *dfeat, int32_t ld_dfeat, const uint8_t *row_mask, const float *points, int64_t n,
                                     int32_t row_stride, const float *bev, int32_t ld_bev, int32_t batch, int32_t h, int32_t w, int32_t c,
                                     float min_x, float min_y, float pix_x, float pix_y, float *dbev, int32_t ld_dbev, float *dxyz,
                                     int32_t ld_dxyz, void *stream);
/* remove_gt_boxes_outside_range: rows whose centre lies in [range[0:3], range[3:6]) keep their order, the rest of (batch, max_boxes, width)
 * is zero (the reference additionally shrinks max_boxes to the largest kept count; zero rows are padding to every consumer).  Rows are
 * [x, y, z, ..., class]: 8 floats in the V2X-Sim models, 10 with velocity (nuScenes), at most the 16 codes the head kernels take; any other
 * width is PCP_ERR_UNSUPPORTED before a launch.  pcp_filter_gt_boxes is the width-8 form. */
#define PCP_GT_BOX_MIN_WIDTH 8
#define PCP_GT_BOX_MAX_WIDTH 16
int pcp_filter_gt_boxes_w(const float *gt_boxes, int32_t batch, int32_t max_boxes, int32_t width, const float *range6_host, float *out,
                          void *stream);
int pcp_filter_gt_boxes(const float *gt_boxes, int32_t batch, int32_t max_boxes, const float *range6_host, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Optimizer step on flat buffers: global-norm clipping + Adam with decoupled weight decay.
 * Replaces tools/train_utils/train_utils.py:57-58 (clip_grad_norm_ + optimizer.step()) and
 *          tools/train_utils/optimization/fastai_optim.py:104-122 (p.mul_(1 - wd * lr); torch.optim.Adam.step, betas (mom, 0.99)).
 * pcp_grad_sqnorm: *sqnorm (double, device) (+)= sum g^2.
 * pcp_adam_step (torch.optim.Adam arithmetic, amsgrad off, bias-corrected):
 *   g = grad * grad_scale * min(1, max_norm / (sqrt(*sqnorm) * |grad_scale| + 1e-6))   (sqnorm NULL: no clipping)
 *   p *= 1 - weight_decay * lr;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr / (1-b1^step) * m / (sqrt(v) / sqrt(1-b2^step) + eps)
 * ------------------------------------------------------------------------------------------------------------------ */
int pcp_grad_sqnorm(const float *grad, int64_t n, double *sqnorm, int32_t accumulate, void *stream);
int pcp_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int64_t step, float max_norm, const double *sqnorm, float grad_scale, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-step weight repacking of a 3x3 conv (the optimizer rewrites the weights every iteration): w is PyTorch's (cout, cin, 3, 3);
 * transpose = 0 packs the forward conv, transpose = 1 the conv that computes its DATA gradient (channel roles swapped, taps
 * flipped: the autograd "conv_transpose" of nn.Conv2d).  direct: [I/16][9][O_pad][16]; winograd: U = G g G^T as [I/8][16][O_pad][8]
 * (layouts of pcp_conv3x3 / pcp_conv3x3_winograd); split_bf16: the hi / lo bf16 layout of pcp_conv3x3_bf16x3 (opt-in arithmetic).
 * Any of the three may be NULL.  (I, O) = (cin, cout) or swapped.
 * ------------------------------------------------------------------------------------------------------------------ */
int pcp_pack_conv3x3(const float *w, int32_t cout, int32_t cin, int32_t transpose, float *direct, int32_t direct_cout_pad,
                     float *winograd, int32_t winograd_cout_pad, void *split_bf16, int32_t split_cout_pad, void *stream);

/* The same per-step repacking into the weight forms of the two fused Winograd F(4x4,3x3) kernels: U = G g G^T (float64, one rounding --
 * the arithmetic of pcp_amd/pack.py::pack_conv3x3_winograd4f) as u4f [I/8][36][cout_pad][8] (pcp_conv3x3_winograd4f) and / or u4h
 * [I/8][36][cout_pad/64][64][8] (pcp_conv3x3_winograd4h); either may be NULL.  I % 8 == 0, cout_pad % 64 == 0, cout_pad >= O. */
int pcp_pack_conv3x3_winograd4(const float *w, int32_t cout, int32_t cin, int32_t transpose, float *u4f, float *u4h, int32_t cout_pad,
                               void *stream);

/* All 3x3 layers of a training step repacked by ONE launch.  A job is one (layer, direction): the arguments of pcp_pack_conv3x3 (without the
 * split-bf16 form) and of pcp_pack_conv3x3_winograd4; any destination may be NULL.  block_start = first block of the job in the grouped
 * launch (jobs in ascending order: job i covers blocks [block_start_i, block_start_i + pcp_pack_conv3x3_group_blocks(job_i))), total_blocks
 * their sum.  `jobs_device` is the table in DEVICE memory (it holds device pointers; the caller keeps it and the buffers alive).
 * _group_blocks: blocks of 256 threads the job needs, -1 for an invalid job (host-side helper, no launch). */
typedef struct pcp_pack_job {
  const float *w;              /* (cout, cin, 3, 3) */
  int32_t cout, cin, transpose;
  int32_t direct_cout_pad;
  float *direct;
  float *winograd;
  int32_t winograd_cout_pad;
  int32_t f4_cout_pad;
  float *u4f;
  float *u4h;
  int32_t block_start;
  int32_t reserved;
} pcp_pack_job_t;
int pcp_pack_conv3x3_group_blocks(const pcp_pack_job_t *job);
int pcp_pack_conv3x3_group(const pcp_pack_job_t *jobs_device, int32_t n_jobs, int32_t total_blocks, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * SC backbone, training half (workspace/sc_conv.py:14-44,91-119 under autograd): what the conv / BatchNorm entry points above do
 * not cover of an SCBottleneck.  Conventions of pcp_avgpool_nhwc / pcp_sc_gate (pcp_hip.h): NHWC float32 channel windows, c / ld
 * multiples of 4, 16-byte aligned pointers.  No atomics: every output element is written by one thread, sums run in a fixed order.
 * ------------------------------------------------------------------------------------------------------------------ */
/* backward of nn.AvgPool2d(r, r): dx[b, y, x] (+)= dpooled[b, y / r, x / r] / (r * r) for y < (h / r) * r and x < (w / r) * r; the
 * remainder rows / columns the pool dropped get 0 (accumulate: are left as they are).  dpooled (B, h / r, w / r), dx (B, h, w). */
int pcp_avgpool_nhwc_backward(const float *dpooled, int32_t ld_dpooled, int32_t batch, int32_t h, int32_t w, int32_t c, int32_t r, float *dx,
                              int32_t ld_dx, int32_t accumulate, void *stream);

/* backward of pcp_sc_gate's out = t * g, g = sigmoid(x + up(s)):
 *   dt = dout * g;  dz = dout * t * (1 - g) * g;  dx (+)= dz (dx NULL: skipped, dz IS the gradient of x);
 *   ds[b, sy, sx] = sum of dz over exactly the pixels the forward's nearest rule sends to (sy, sx), rows then columns ascending.
 * Two launches: one thread per pixel, then one thread per s element walking its own pixel range (the inverse of the nearest index,
 * found with the same float32 scale product).  dt may alias dout; dz (B, h, w, ld_dz) is a buffer of its own. */
int pcp_sc_gate_backward(const float *dout, int32_t ld_dout, const float *t, int32_t ld_t, const float *x, int32_t ld_x, const float *s,
                         int32_t ld_s, int32_t sh, int32_t sw, float *dt, int32_t ld_dt, float *dz, int32_t ld_dz, float *dx, int32_t ld_dx,
                         int32_t accumulate_dx, float *ds, int32_t ld_ds, int32_t batch, int32_t h, int32_t w, int32_t c, void *stream);

/* the bottleneck's residual in front of its last ReLU: out = relu(z + res) (out may alias z), and its backward
 * dz = dout * [out > 0] (dz may alias dout), also copied to dz2 when that is not NULL (the residual branch and the in-place
 * BatchNorm backward of the conv branch each need their own). */
int pcp_add_relu(const float *z, int32_t ld_z, const float *res, int32_t ld_res, float *out, int32_t ld_out, int64_t rows, int32_t c,
                 void *stream);
int pcp_add_relu_backward(const float *dout, int32_t ld_dout, const float *out, int32_t ld_out, float *dz, int32_t ld_dz, float *dz2,
                          int32_t ld_dz2, int64_t rows, int32_t c, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * World augmentation of a collated training batch (the reference's DataAugmentor random_world_flip / _rotation / _scaling /
 * _translation and the DataProcessor's mask_points_and_boxes_outside_range, which it runs per sample on the host before collation;
 * csrc/augment.hip).  Every row / box / matrix is transformed with the parameters of ITS frame, stage by stage in the order of
 * `stage[]`, each stage with the reference's own float32 operations (nothing is composed into one matrix).
 *
 * table (device, batch x PCP_AUG_TABLE_STRIDE float32, written by the host), per frame:
 *   [0] flip_x (0 / 1: y -> -y)  [1] flip_y (0 / 1: x -> -x)  [2] cos  [3] sin  [4] rot  [5] scale  [6..8] tx ty tz  [9..11] unused
 * cos / sin are the float32 values the host computed for the rotation matrix; the kernels evaluate no sine or cosine for it.
 * ------------------------------------------------------------------------------------------------------------------ */
#define PCP_AUG_FLIP_X 1
#define PCP_AUG_FLIP_Y 2
#define PCP_AUG_ROTATE 3
#define PCP_AUG_SCALE 4
#define PCP_AUG_TRANSLATE 5
#define PCP_AUG_MAX_STAGES 8
#define PCP_AUG_MAX_BATCH 64
#define PCP_AUG_TABLE_STRIDE 12
#define PCP_AUG_MIN_ROW_STRIDE 4  /* frame index + xyz */
#define PCP_AUG_MAX_ROW_STRIDE 15 /* frame index + 14 feature columns */
#define PCP_AUG_TILE_ROWS 512     /* rows one workgroup stages through LDS */
typedef struct pcp_world_aug {
  int32_t n_stages;
  int32_t stage[PCP_AUG_MAX_STAGES]; /* PCP_AUG_* in the order they are applied */
  int32_t batch;
  int32_t hd_map;   /* rows are [b, x y z i t, 4 map masks, lane_dir, sweep, instance] (row_stride 13): lane_dir follows the flips / rotation */
  int32_t filter;   /* keep only rows with range[0..2] <= xyz < range[3..5] after the transform, compacted in input order */
  float range[6];
  int32_t raw_heading; /* pcp_world_augment_boxes: 1 = leave the heading as the stages made it (object stages follow and the reference applies
                          limit_period once, behind its whole list); 0 = end with limit_period */
} pcp_world_aug_t;

/* points (n, row_stride) float32, column 0 the frame index, 16-byte aligned like `out`.  xyz always; hd_map: column 10 (lane_dir);
 * row_stride >= 14: column 9 (MoDAR heading) on the rows whose column row_stride - 3 is > 0; every other column keeps its bits.  Rows of
 * a frame outside [0, batch) are not transformed and, with the filter on, dropped.
 *   filter off: out[i] = transformed points[i] (out may be points itself); frame_count and the workspace are not used.
 *   filter on : the kept rows in input order at the front of `out` (n rows of capacity, NOT points itself; the rows behind them are
 *               left as they are) and frame_count[b] (device, batch int32) = rows kept of frame b.
 * Two launches with the filter on (count per tile, place), one without; no atomics on the placement path: a call repeats bit for bit. */
size_t pcp_world_augment_points_workspace_bytes(int64_t n);
int pcp_world_augment_points(const pcp_world_aug_t *aug, const float *table, const float *points, int64_t n, int32_t row_stride, float *out,
                             int32_t *frame_count, void *workspace, size_t workspace_bytes, void *stream);

/* gt_boxes (batch, max_boxes, box_width) in place, box_width 8 [x y z dx dy dz heading class] or 10 [.. heading vx vy class]; rows of class 0
 * (padding) keep their bits; the heading ends with limit_period(h, 0.5, 2 pi) unless aug->raw_heading.  instances_tf (nullable; batch, max_boxes, n_sweeps, tf_rows,
 * 4) with tf_rows 3 or 4: every matrix of a box of class != 0 becomes T A T^-1 for each stage in order, evaluated as an affine map in
 * float32 (a fourth row keeps its bits).  `range` / `filter` / `hd_map` of aug are not read.  One launch. */
int pcp_world_augment_boxes(const pcp_world_aug_t *aug, const float *table, float *gt_boxes, int32_t max_boxes, int32_t box_width,
                            float *instances_tf, int32_t n_sweeps, int32_t tf_rows, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * gt_sampling on a collated training batch (the reference's DataBaseSampler.__call__ / add_sampled_boxes_to_scene, which it runs per
 * sample on the host; csrc/gt_sample.hip).  The host draws the candidates (the numpy pointer / permutation state machine) and writes
 *   frame_table (device, batch x (n_groups + 2) int32), per frame: [0] n_own = its real gt boxes (class column > 0, rows 0 .. n_own - 1),
 *               [1 + g] .. [2 + g] = the candidate slots of sample group g, in class order;
 *   cand_db     (device, n_cand int32) the database index of every candidate slot;
 *   cand_box    (device, n_cand x PCP_GTS_CAND_STRIDE float32) [x y z dx dy dz heading, vx vy mapped into the frame, 1-based class id].
 * The device decides which candidates collide and pastes the others.  accepted (device, batch x acc_cap x PCP_GTS_ACC_STRIDE int32), per
 * frame and accepted object in order: [slot, database index, exclusive prefix of the point counts, point count];
 * counts (device, 2 batch + 1 int32): [b] accepted objects, [batch + b] rows added, [2 batch] the error word of the paste.
 * ------------------------------------------------------------------------------------------------------------------ */
#define PCP_GTS_MAX_GROUPS 16  /* sample groups (classes) */
#define PCP_GTS_MAX_CAND 64    /* candidates per class per frame */
#define PCP_GTS_MAX_BOXES 512  /* existing + accepted boxes per frame; the host wrapper refuses existing + CANDIDATE boxes above it, since every candidate may be accepted */
#define PCP_GTS_CAND_STRIDE 10
#define PCP_GTS_ACC_STRIDE 4

/* One workgroup per frame walks the groups in order: a candidate is accepted iff its rotated BEV IoU (the arithmetic of pcp_nms_rotated /
 * pcp_boxes_bev_pairwise) with every existing box and with every OTHER candidate of its group is 0; the accepted boxes join the existing
 * ones before the next group.  gt_boxes (batch, max_boxes, box_width 8 | 10); db_count (n_db int32) the points of every database object.
 * Also clears the error word. */
int pcp_gt_sample_select(const float *gt_boxes, int32_t batch, int32_t max_boxes, int32_t box_width, const int32_t *frame_table,
                         int32_t n_groups, const int32_t *cand_db, const float *cand_box, int32_t n_cand, const int32_t *db_count, int32_t n_db,
                         int32_t *accepted, int32_t acc_cap, int32_t *counts, void *stream);

/* out (capacity n + max_added rows of row_stride floats, 16-byte aligned like points): every frame's own rows in their input order followed
 * by its accepted objects' stored rows (db_points rows of row_stride - 1 floats starting at row db_offset[db]) in order, column 0 = the
 * frame index, xyz + the candidate's float32 box centre (a float32 add), column inst_col = n_own + the object's position in the frame's
 * accepted list, every other column bit for bit.  The input rows must be grouped by ascending frame index; the first row of every frame is
 * found on the device (segments: batch + 1 int32 of scratch).  A descending neighbour pair (error word 1) or a frame index outside
 * [0, batch) (2) sets counts[2 batch] and nothing is written.  max_added: an upper bound of the rows added (the grid is sized by it).
 * Two launches, no atomics: a call repeats bit for bit. */
int pcp_gt_sample_paste_points(const float *points, int64_t n, int32_t row_stride, int32_t batch, const int32_t *frame_table, int32_t n_groups,
                               const int32_t *accepted, int32_t acc_cap, const int32_t *counts, const float *cand_box, const float *db_points,
                               const int32_t *db_offset, int32_t inst_col, int64_t max_added, float *out, int32_t *segments, void *stream);

/* gt_out (batch, max_boxes_out, box_width) and tf_out (nullable; batch, max_boxes_out, n_sweeps, tf_rows 3 | 4, 4): own rows bit for bit,
 * then the accepted objects (box7, vx vy of cand_box when box_width is 10, the class id; the first tf_rows rows of db_tf (n_db, n_sweeps,
 * 4, 4)), then padding as the collation writes it (zero boxes, identity 3 x 3).  One launch. */
int pcp_gt_sample_paste_boxes(const float *gt_boxes, int32_t batch, int32_t max_boxes, int32_t box_width, const float *instances_tf,
                              int32_t n_sweeps, int32_t tf_rows, const int32_t *frame_table, int32_t n_groups, const int32_t *accepted,
                              int32_t acc_cap, const int32_t *counts, const float *cand_box, const float *db_tf, float *gt_out, float *tf_out,
                              int32_t max_boxes_out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-object augmentation of a collated training batch (the reference's random_local_translation / _rotation / _scaling,
 * random_local_frustum_dropout and random_world_frustum_dropout, augmentor_utils.py; csrc/object_augment.hip).  The reference walks the
 * boxes of a sample in order; box i masks the points inside it as it is BEFORE its own change (get_points_in_box), changes them, then
 * changes itself, and later boxes see the moved points.  A box never depends on another box, so pcp_object_augment_boxes runs every box
 * through the sub-stages and records its state in front of each; a point walks sub-stages x boxes against those states.
 *
 * params (device, batch x n_stages x max_boxes x PCP_OBJ_PARAM_STRIDE float32, written by the host), per sub-stage and box:
 *   [0] the drawn value as float32 (offset / scale / angle / intensity)  [1] cos  [2] sin of the angle (ROTATE only, host float32)  [3] unused
 * box_states (device, batch x n_stages x max_boxes x PCP_OBJ_STATE_STRIDE float32, written by pcp_object_augment_boxes):
 *   [0..2] centre  [3] dx/2 + 0.1  [4] dy/2 + 0.1  [5] dz/2 (-1 on padding rows: nothing is inside)  [6] cos(-heading)  [7] sin(-heading)
 *   [8] offset | scale | cos | dropout threshold  [9] sin  [10..11] unused
 * ------------------------------------------------------------------------------------------------------------------ */
#define PCP_OBJ_TRANSLATE_X 1
#define PCP_OBJ_TRANSLATE_Y 2
#define PCP_OBJ_TRANSLATE_Z 3
#define PCP_OBJ_SCALE 4
#define PCP_OBJ_ROTATE 5
#define PCP_OBJ_DROP_TOP 6          /* local frustum dropouts: inside box i and z >= (z + dz/2) - intensity dz, ... */
#define PCP_OBJ_DROP_BOTTOM 7
#define PCP_OBJ_DROP_LEFT 8
#define PCP_OBJ_DROP_RIGHT 9
#define PCP_OBJ_WORLD_DROP_TOP 10   /* world frustum dropouts: a row filter against frame_thr; only as the single stage of a points call */
#define PCP_OBJ_WORLD_DROP_BOTTOM 11
#define PCP_OBJ_WORLD_DROP_LEFT 12
#define PCP_OBJ_WORLD_DROP_RIGHT 13
#define PCP_OBJ_MAX_STAGES 16       /* sub-stages of one call (a translation over x y z is three) */
#define PCP_OBJ_MAX_BOXES 512       /* box rows per frame (max_boxes) */
#define PCP_OBJ_LDS_BOXES 64        /* box states staged in LDS at a time, next to the two row tiles */
#define PCP_OBJ_STATE_STRIDE 12
#define PCP_OBJ_PARAM_STRIDE 4
typedef struct pcp_object_aug {
  int32_t n_stages;
  int32_t stage[PCP_OBJ_MAX_STAGES]; /* PCP_OBJ_* in the order they are applied */
  int32_t batch;
  int32_t limit_heading; /* pcp_object_augment_boxes ends with limit_period(h, 0.5, 2 pi): set when no world stage follows */
} pcp_object_aug_t;

/* gt_boxes (batch, max_boxes <= PCP_OBJ_MAX_BOXES, box_width 8 | 10) in place: translation adds to its coordinate only (the velocity
 * stays), scaling multiplies dx dy dz, rotation adds to the heading (the centre goes through the reference's subtract, rotate, add-back of
 * its own value and keeps its bits; box_width 10 is refused with PCP_ERR_UNSUPPORTED as the reference's velocity branch raises),
 * dropouts leave the box.  Rows of class 0 keep their bits.  n_boxes[b] (device, batch int32) = 1 + the last row of class != 0.
 * Stages PCP_OBJ_TRANSLATE_X .. PCP_OBJ_DROP_RIGHT only.  One launch. */
int pcp_object_augment_boxes(const pcp_object_aug_t *aug, const float *params, float *gt_boxes, int32_t max_boxes, int32_t box_width,
                             float *box_states, int32_t *n_boxes, void *stream);

/* points (n, row_stride) float32 like pcp_world_augment_points (column 0 the frame index, 16-byte aligned like `out`); the frames a tile
 * holds are read from its rows, a tile that straddles frames walks each of them.  Only xyz change; every other column keeps its bits.
 * Rows of a frame outside [0, batch) pass untouched.  Without a dropout stage: one launch, out[i] = points[i] moved (out may be points).
 * With one: the surviving rows in input order at the front of `out` (n rows of capacity, not points itself), frame_count (device,
 * batch + 1 int32): [b] = rows kept of frame b, [batch] = rows of a frame outside [0, batch), all kept, so the sum is the rows written;
 * two launches (count per tile, place), no atomics on the placement path: a call repeats bit for bit.
 * A single PCP_OBJ_WORLD_DROP_* stage reads frame_thr (device, batch float32) instead of box states: TOP keeps z < thr, BOTTOM z > thr,
 * LEFT y < thr, RIGHT y > thr. */
size_t pcp_object_augment_points_workspace_bytes(int64_t n);
int pcp_object_augment_points(const pcp_object_aug_t *aug, const float *box_states, const int32_t *n_boxes, int32_t max_boxes,
                              const float *frame_thr, const float *points, int64_t n, int32_t row_stride, float *out, int32_t *frame_count,
                              void *workspace, size_t workspace_bytes, void *stream);

/* extent[2 b], extent[2 b + 1] (device float32) = min, max of column `col` (2 = y, 3 = z) over the rows of frame b; +inf, -inf for a frame
 * without rows.  Two launches (per tile, per frame), no float atomics: deterministic. */
size_t pcp_frame_extent_workspace_bytes(int64_t n, int32_t batch);
int pcp_frame_extent(const float *points, int64_t n, int32_t row_stride, int32_t batch, int32_t col, float *extent, void *workspace,
                     size_t workspace_bytes, void *stream);

/* The box half of a world frustum dropout and its threshold.  direction PCP_OBJ_WORLD_DROP_*; intensity (device, batch float32).
 * frame_thr[b] = max - intensity (max - min) (TOP, LEFT) or min + intensity (max - min) (BOTTOM, RIGHT) in float32; a frame without
 * extent gets the threshold every row and box passes (+-inf) and its boxes are copied as they are.  gt_out / tf_out (not the inputs):
 * the boxes of class != 0 whose z (TOP, BOTTOM) or y (LEFT, RIGHT) passes the strict test, in order, their instances_tf rows (nullable;
 * batch, max_boxes, n_sweeps, tf_rows 3 | 4, 4) with them, then zero boxes and the collation's identity padding.  n_boxes_out[b] = survivors.
 * One launch. */
int pcp_object_augment_drop_boxes(const float *gt_boxes, int32_t batch, int32_t max_boxes, int32_t box_width, const float *instances_tf,
                                  int32_t n_sweeps, int32_t tf_rows, const float *extent, const float *intensity, int32_t direction,
                                  float *frame_thr, float *gt_out, float *tf_out, int32_t *n_boxes_out, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training half of the sparse 3D convolution (csrc/spconv3d_train.hip; the forward and its tables: include/pcp_hip.h).  fp32, no float
 * atomics: every call repeats bit for bit.
 *
 * Data gradient: pcp_spconv3d itself.  Submanifold layer: dx = pcp_spconv3d(dy, nbr, W') with the forward's own table (it is symmetric
 * under mirroring the offset: nbr[k][j] == i exactly when nbr[26 - k][i] == j) and W'[k] = W[26 - k]^T packed [K][Cin][Cout].  Strided
 * layer: dx = pcp_spconv3d(dy, inv, W'), W'[k] = W[k]^T, with the inverse table below.  No bias, residual or ReLU.
 * ------------------------------------------------------------------------------------------------------------------ */

/* inv (num_offsets, n_in) int32: inv[k][i] = j where nbr[k][j] == i, else -1.  nbr (num_offsets, n_out).  A fill and one launch; each
 * (k, i) has at most one j, so the stores do not race.  Entries of nbr outside [0, n_in) are passed over. */
int pcp_spconv_invert_nbr(const int32_t *nbr, int32_t num_offsets, int64_t n_out, int64_t n_in, int32_t *inv, void *stream);

/* dw (cout, num_offsets, cin) -- the parameter's (Cout, kz, ky, kx, Cin) -- (+)= sum over rows j with nbr[k][j] in [0, n_in) of
 * dy[j][co] * x[nbr[k][j]][ci].  x (n_in, ld_in) with cin columns, dy (n_out, cout) contiguous and 16-byte aligned; the channel pairs
 * and the alignment rules of x are pcp_spconv3d's forward ones (PCP_ERR_UNSUPPORTED for another pair).  Two launches: workgroups over
 * (offset, row chunk) write partial blocks to the workspace, a second kernel adds the partials of an offset in ascending chunk order.
 * chunk_rows: rows per chunk, a multiple of 16; 0 = the library's rule (at most 32 chunks, none shorter than 1024 rows), which bounds
 * the workspace by 27 x 32 x cout x cin_pad floats.  The workspace size depends on chunk_rows: ask with the same value.
 * n_out == 0 or n_in == 0: dw is zero-filled (left alone when accumulating), no kernel runs. */
size_t pcp_spconv3d_wgrad_workspace_bytes(int64_t n_out, int32_t num_offsets, int32_t cin, int32_t cout, int32_t chunk_rows);
int pcp_spconv3d_wgrad(const float *x, int64_t n_in, int32_t cin, int32_t ld_in, const float *dy, const int32_t *nbr, int32_t num_offsets,
                       int64_t n_out, int32_t cout, int32_t chunk_rows, void *workspace, size_t workspace_bytes, float *dw, int32_t accumulate,
                       void *stream);

/* gradient of pcp_spconv_dense: dfeat[r][c] = dcanvas[(b, y, x)][c * d + z] for row r at coords[r] = [b, z, y, x] (int32, 16-byte
 * aligned); dcanvas (batch, h, w, channels * d) NHWC.  Every element of dfeat (n, channels) is written (zero for a row outside the grid). */
int pcp_spconv_dense_backward(const float *dcanvas, const int32_t *coords, int64_t n, int32_t channels, int32_t batch, int32_t d, int32_t h,
                              int32_t w, float *dfeat, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PCP_HIP_TRAIN_H */
