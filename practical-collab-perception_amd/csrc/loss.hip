// a15 -- CenterHead target assignment and training losses on the device, plus the DiscoNet distillation loss.
//
// Replaces (all host-side python / numpy loops or chains of small ATen ops in the reference):
//   CenterHead.assign_targets / assign_target_of_single_head   pcdet/models/dense_heads/center_head.py:104-164,166-268
//     (.cpu() -> per-box python loop -> .to(device), one host round trip per iteration)
//   gaussian_radius / gaussian2D / draw_gaussian_to_heatmap    pcdet/models/model_utils/centernet_utils.py:8-68
//   CenterHead.get_loss, sigmoid clamp                          center_head.py:270-300
//   neg_loss_cornernet, _reg_loss, RegLossCenterNet             pcdet/utils/loss_utils.py:264-375
//   loss_distill = 10 * smooth_l1(softmax_c(fused), softmax_c(bev_img_early))   bev_layers/v2x_fusion_disco.py:119-123
// and the autograd nodes behind them: the loss kernels also emit dL/d(head maps) and dL/d(fused map).
//
// Latency-bound integer/float work (<= 500 boxes, 16 384 cells): one workgroup per frame for the targets, flat streaming
// kernels for the losses; every reduction is float64 (atomics per block), so the scalar losses are order independent.
#include "pcp_common.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace {

constexpr int TGT_THREADS = 256;
constexpr int TGT_MAX_BOXES = 1024;

// centernet_utils.py:8-35 in float32 (tensor arithmetic of the reference); python scalars enter as float32 constants
__device__ float gaussian_radius_f32(float height, float width, float min_overlap) {
  const float b1 = height + width;
  const float c1 = width * height * ((1.f - min_overlap) / (1.f + min_overlap));
  const float sq1 = sqrtf(b1 * b1 - 4.f * c1);
  const float r1 = (b1 + sq1) / 2.f;
  const float b2 = 2.f * (height + width);
  const float c2 = (1.f - min_overlap) * width * height;
  const float sq2 = sqrtf(b2 * b2 - 16.f * c2);
  const float r2 = (b2 + sq2) / 2.f;
  const float a3 = 4.f * min_overlap;
  const float b3 = -2.f * min_overlap * (height + width);
  const float c3 = (min_overlap - 1.f) * width * height;
  const float sq3 = sqrtf(b3 * b3 - 4.f * a3 * c3);
  const float r3 = (b3 + sq3) / 2.f;
  return fminf(fminf(r1, r2), r3);
}

struct BoxT { int valid, x, y, r, cls; };

// One head as targets_frame sees it.  pcp_centerhead_targets leaves the optional parts absent; everything the two entry points do
// differently on purpose is a field here.
struct TgtHead {
  int bw, tw;                        // row width of gt_boxes (class in the last column; 10: vx, vy before it) and of target_boxes
  int num_class;                     // channels of the heat map
  float *heat, *tbox;                // the four outputs, all frames
  int *inds, *mask;
  const int *class_to_local;         // the head's class table; nullptr: the head owns classes 1 .. num_class
  const pcp_target_head_t *iou;      // raw head maps and channels the IoU column decodes; nullptr: no IoU column
  bool zero_heat;                    // the block zeroes its heat-map slab, so the assignment is one launch; false: the host zeroed it
  bool guard_boxes;                  // also test i < TGT_MAX_BOXES around boxes[].  Both entry points refuse max_boxes > TGT_MAX_BOXES on
                                     // the host, so either form is safe; the flag only keeps each kernel's code as it was
};

// head-local class of a row, 1-based (0: not this head's), from its class column
__device__ __forceinline__ int local_class(const TgtHead &f, float c) {
  if (!f.class_to_local) return (c >= 1.f && c <= (float)f.num_class) ? (int)c : 0;
  const int gc = (c >= 1.f && c < (float)PCP_TGT_MAX_CLASSES) ? (int)c : 0;
  return f.class_to_local[gc];
}

// box_utils.py:6-25 as it stands: the (3, 4) sign table is reshaped with .view(4, 3), NOT transposed, so the four "corners" are
// (+,+), (-,-), (+,-), (+,+) -- three distinct points.  The rectangle is the axis-aligned hull of those, rotated (common_utils.py:39-61:
// x' = x cos - y sin, y' = x sin + y cos) and shifted to the centre.
__device__ void aa_rect(float x, float y, float dx, float dy, float angle, float *r) {
  const float c = cosf(angle), s = sinf(angle);
  const float hx = 0.5f * dx, hy = 0.5f * dy;
  const float sx[4] = {1.f, -1.f, 1.f, 1.f}, sy[4] = {1.f, -1.f, -1.f, 1.f};
  float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lx = hx * sx[i], ly = hy * sy[i];
    const float wx = lx * c + ly * (-s) + x;
    const float wy = lx * s + ly * c + y;
    x0 = fminf(x0, wx); x1 = fmaxf(x1, wx);
    y0 = fminf(y0, wy); y1 = fmaxf(y1, wy);
  }
  r[0] = x0; r[1] = y0; r[2] = x1; r[3] = y1;
}

// box_utils.py:39-67
__device__ float aa_iou(const float *a, const float *b) {
  const float ix1 = fminf(a[2], b[2]), iy1 = fminf(a[3], b[3]);
  const float ix0 = fmaxf(a[0], b[0]), iy0 = fmaxf(a[1], b[1]);
  const float inter = fmaxf(ix1 - ix0, 0.f) * fmaxf(iy1 - iy0, 0.f);
  const float a1 = fmaxf(a[2] - a[0], 0.f) * fmaxf(a[3] - a[1], 0.f);
  const float a2 = fmaxf(b[2] - b[0], 0.f) * fmaxf(b[3] - b[1], 0.f);
  const float uni = a1 + a2 - inter;
  return uni > 0.f ? inter / uni : 0.f;
}

// CenterHead target assignment (center_head.py:166-268): frame b of one head per workgroup of TGT_THREADS, gt_boxes (batch, m, bw).
// pcp_centerhead_targets (a15) and pcp_centerhead_targets_ext (a15x: several heads, velocity codes, the IoU column) both run this body.
__device__ __forceinline__ void targets_frame(const pcp_target_t &d, const TgtHead &f, const float *gt, int m, int b) {
  __shared__ BoxT boxes[TGT_MAX_BOXES];
  __shared__ int rank_of[TGT_MAX_BOXES];
  __shared__ int wave_tot[TGT_THREADS / 64];
  __shared__ int base;
  const int tid = threadIdx.x;
  const int bw = f.bw, tw = f.tw, ncls = f.num_class;
  const float *g = gt + (long long)b * m * bw;
  float *heat = f.heat + (long long)b * d.h * d.w * ncls, *tbox = f.tbox + (long long)b * d.k * tw;
  int *inds = f.inds + (long long)b * d.k, *mask = f.mask + (long long)b * d.k;
  if (tid == 0) base = 0;
  // zero this frame's sparse outputs
  for (int i = tid; i < d.k * tw; i += TGT_THREADS) tbox[i] = 0.f;
  for (int i = tid; i < d.k; i += TGT_THREADS) { inds[i] = 0; mask[i] = 0; }
  if (f.zero_heat)
    for (int i = tid; i < d.h * d.w * ncls; i += TGT_THREADS) heat[i] = 0.f;
  __syncthreads();
  // rank of each foreground row among the rows of this head, in row order (class filter of center_head.py:192-210)
  for (int start = 0; start < m; start += TGT_THREADS) {
    const int i = start + tid;
    const int local = i < m ? local_class(f, g[i * bw + bw - 1]) : 0;
    const int fg = local > 0 ? 1 : 0;
    const unsigned long long bal = __ballot(fg);
    const int lane = tid & 63, wv = tid >> 6;
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wv] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wv; ++w) off += wave_tot[w];
    if (i < m) {
      rank_of[i] = fg ? off + before : -1;
      if (f.class_to_local) boxes[i].cls = local - 1;          // the table lookup is kept for the box loop
    }
    __syncthreads();
    if (tid == 0) { int t = 0; for (int w = 0; w < TGT_THREADS / 64; ++w) t += wave_tot[w]; base += t; }
    __syncthreads();
  }
  for (int i = tid; i < m; i += TGT_THREADS) {
    BoxT bx{0, 0, 0, 0, f.class_to_local ? boxes[i].cls : 0};
    const int k = rank_of[i];
    if (k >= 0 && k < d.k) {
      const float *r = g + i * bw;
      float cx = (r[0] - d.min_x) / d.voxel_x / d.stride;
      float cy = (r[1] - d.min_y) / d.voxel_y / d.stride;
      cx = fminf(fmaxf(cx, 0.f), (float)d.w - 0.5f);
      cy = fminf(fmaxf(cy, 0.f), (float)d.h - 0.5f);
      const int ix = (int)cx, iy = (int)cy;
      const float dx = r[3] / d.voxel_x / d.stride;
      const float dy = r[4] / d.voxel_y / d.stride;
      if (dx > 0.f && dy > 0.f) {
        float rad = gaussian_radius_f32(dx, dy, d.gaussian_overlap);
        int ri = (rad == rad) ? (int)rad : 0;
        if (ri < d.min_radius) ri = d.min_radius;
        bx.valid = 1; bx.x = ix; bx.y = iy; bx.r = ri;
        // no table: a row that has a slot passed the range test, so its class converts directly.  Open-coded: the trip through LDS,
        // or a second range test, costs k_targets 1 % of a targets + loss call (profiles/centerhead_train_twins.txt)
        if (!f.class_to_local) bx.cls = (int)r[bw - 1] - 1;
        inds[k] = iy * d.w + ix;
        mask[k] = 1;
        float *t = tbox + (long long)k * tw;
        t[0] = cx - (float)ix;
        t[1] = cy - (float)iy;
        t[2] = r[2];
        t[3] = logf(r[3]);
        t[4] = logf(r[4]);
        t[5] = logf(r[5]);
        t[6] = cosf(r[6]);
        t[7] = sinf(r[6]);
        if (bw == 10) { t[8] = r[7]; t[9] = r[8]; }
        if (f.iou) {
          // center_head.py:213-242: the prediction at the ground-truth centre's cell, decoded, against the ground-truth box
          const pcp_target_head_t &hd = *f.iou;
          const float *px = hd.head + (((long long)b * d.h + iy) * d.w + ix) * hd.ld;
          const float pxw = ((float)ix + px[hd.ch_center]) * d.stride * d.voxel_x + d.min_x;
          const float pyw = ((float)iy + px[hd.ch_center + 1]) * d.stride * d.voxel_y + d.min_y;
          const float ang = atan2f(px[hd.ch_rot + 1], px[hd.ch_rot]);
          float ra[4], rb[4];
          aa_rect(pxw, pyw, expf(px[hd.ch_dim]), expf(px[hd.ch_dim + 1]), ang, ra);
          aa_rect(r[0], r[1], r[3], r[4], r[6], rb);
          t[tw - 1] = 2.0f * aa_iou(ra, rb) - 1.f;
        }
      }
    }
    if (!f.guard_boxes || i < TGT_MAX_BOXES) boxes[i] = bx;
  }
  __syncthreads();
  // gaussian splat with max blending (order independent); float64 exp then one rounding, like numpy float64 -> .float()
  int *hm = reinterpret_cast<int *>(heat);
  for (int i = 0; i < m && (!f.guard_boxes || i < TGT_MAX_BOXES); ++i) {
    const BoxT bx = boxes[i];
    if (!bx.valid) continue;
    const int r = bx.r;
    const int left = min(bx.x, r), right = min(d.w - bx.x, r + 1);
    const int top = min(bx.y, r), bottom = min(d.h - bx.y, r + 1);
    const int ww = left + right, hh = top + bottom;
    if (ww <= 0 || hh <= 0) continue;
    const double sigma = (double)(2 * r + 1) / 6.0;
    const double inv = 1.0 / (2.0 * sigma * sigma);
    for (int p = tid; p < ww * hh; p += TGT_THREADS) {
      const int py = p / ww - top, px = p % ww - left;
      const float v = (float)exp(-(double)(px * px + py * py) * inv);
      atomicMax(hm + ((long long)(bx.y + py) * d.w + (bx.x + px)) * ncls + bx.cls, __float_as_int(v));
    }
  }
}

// grid = frames.  The one-head form: classes 1 .. num_class, 8-column rows, no IoU column; the host zeroed the heat map before the launch.
__global__ __launch_bounds__(TGT_THREADS) void k_targets(pcp_target_t d, const float *__restrict__ gt, int m, float *__restrict__ heat,
                                                        float *__restrict__ tbox, int *__restrict__ inds, int *__restrict__ mask) {
  const TgtHead f = {8, 8, d.num_class, heat, tbox, inds, mask, nullptr, nullptr, /*zero_heat*/ false, /*guard_boxes*/ true};
  targets_frame(d, f, gt, m, blockIdx.x);
}

struct TgtExtParams {
  pcp_target_t d;
  pcp_target_head_t heads[PCP_DET_MAX_HEADS];
  int bw, with_iou, tw;            // row width of gt_boxes, IoU column requested, row width of target_boxes
};

// grid = heads x frames: block (h * batch + b).  The head's class table, 8- or 10-column rows and the IoU column; the block zeroes its
// own heat-map slab, so the whole assignment is this one launch.
__global__ __launch_bounds__(TGT_THREADS) void k_targets_ext(TgtExtParams p, const float *__restrict__ gt, int m) {
  const pcp_target_head_t &hd = p.heads[blockIdx.x / p.d.batch];
  const TgtHead f = {p.bw, p.tw, hd.num_class, hd.heatmap, hd.target_boxes, hd.inds, hd.mask, hd.class_to_local,
                     p.with_iou ? &hd : nullptr, /*zero_heat*/ true, /*guard_boxes*/ false};
  targets_frame(p.d, f, gt, m, blockIdx.x % p.d.batch);
}

// ---- losses ---------------------------------------------------------------------------------------------------------------
// acc (double): [0] pos_loss  [1] neg_loss  [2] num_pos  [3] num (mask sum)  [4..11] per-code L1 sums  [12] distill sum
constexpr int ACC_N = 16;

__device__ __forceinline__ float clamped_sigmoid(float x, int *inside) {
  const float s = 1.f / (1.f + expf(-x));
  *inside = (s >= 1e-4f && s <= 1.f - 1e-4f) ? 1 : 0;
  return fminf(fmaxf(s, 1e-4f), 1.f - 1e-4f);
}

// neg_loss_cornernet (loss_utils.py:264-290): a thread's sums, and what one heat-map element adds to them (x the raw logit, gtv the
// target).  By value: accumulators passed by reference end up in scratch.
struct FocalSums { double pos, neg, npos; };

__device__ __forceinline__ FocalSums focal_add(FocalSums a, float x, float gtv) {
  int inside;
  const float p = clamped_sigmoid(x, &inside);
  if (gtv == 1.f) {
    a.pos += (double)(logf(p) * (1.f - p) * (1.f - p));
    a.npos += 1.0;
  } else if (gtv < 1.f) {
    const float w = (1.f - gtv) * (1.f - gtv);
    a.neg += (double)(logf(1.f - p) * p * p * (w * w));
  }
  return a;
}

// ... and its derivative by the logit, weighted: zero where the sigmoid clamp is active; npos is the head's count of gtv == 1 elements
__device__ __forceinline__ float focal_grad(float x, float gtv, double npos, float cls_weight, float grad_scale) {
  const float coef = -cls_weight * grad_scale / (float)(npos == 0.0 ? 1.0 : npos);
  int inside;
  const float p = clamped_sigmoid(x, &inside);
  float dldp = 0.f;
  if (gtv == 1.f) {
    if (npos != 0.0) dldp = (1.f - p) * (1.f - p) / p - 2.f * (1.f - p) * logf(p);
  } else if (gtv < 1.f) {
    const float w = (1.f - gtv) * (1.f - gtv);
    dldp = (w * w) * (-(p * p) / (1.f - p) + 2.f * p * logf(1.f - p));
  }
  return inside ? coef * dldp * p * (1.f - p) : 0.f;
}

// the mask sum as the L1 terms divide by it: torch.clamp_min(num, 1.0) of _reg_loss
__device__ __forceinline__ double clamped_num(double mask_sum) { return mask_sum < 1.0 ? 1.0 : mask_sum; }

// one head's losses from its sums (center_head.py:274-295): out = [hm_loss (weighted), loc_loss (weighted), hm + loc, num_pos]; returns
// out[2].  sums[j] is the L1 sum of code j; its mean is rounded to float32 before the code weight, as the reference's float32 tensor is.
__device__ __forceinline__ float head_losses(double pos, double neg, double npos, double mask_sum, const double *sums, int n_codes,
                                             const float *code_weights, float cls_weight, float loc_weight, float *out) {
  const double hm = (npos == 0.0 ? -neg : -(pos + neg) / npos) * (double)cls_weight;
  const double num = clamped_num(mask_sum);
  double loc = 0;
  for (int j = 0; j < n_codes; ++j) loc += (double)(float)(sums[j] / num) * (double)code_weights[j];
  loc *= (double)loc_weight;
  out[0] = (float)hm;
  out[1] = (float)loc;
  out[2] = (float)(hm + loc);
  out[3] = (float)npos;
  return (float)(hm + loc);
}

// the L1 term of one code: its sign (0 where prediction and target are equal: nothing is added), and what one slot adds to dL/d(pred)
__device__ __forceinline__ float l1_sign(float diff) { return diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float l1_grad_term(float sg, float loc_weight, float code_weight, float grad_scale, double num) {
  return sg * loc_weight * code_weight * grad_scale / (float)num;
}

__global__ __launch_bounds__(256) void k_focal_reduce(pcp_headloss_t d, const float *__restrict__ head, const float *__restrict__ heat,
                                                     double *acc) {
  __shared__ double sh[4];
  const long long total = (long long)d.batch * d.h * d.w * d.num_class;
  FocalSums a = {0, 0, 0};
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(t % d.num_class);
    const long long pix = t / d.num_class;
    a = focal_add(a, head[pix * d.ld + d.ch_hm + c], heat[t]);
  }
  double s = block_sum_lane0(a.pos, sh);
  if (threadIdx.x == 0) atomicAdd(acc + 0, s);
  s = block_sum_lane0(a.neg, sh);
  if (threadIdx.x == 0) atomicAdd(acc + 1, s);
  s = block_sum_lane0(a.npos, sh);
  if (threadIdx.x == 0) atomicAdd(acc + 2, s);
}

__global__ __launch_bounds__(256) void k_reg_reduce(pcp_headloss_t d, const float *__restrict__ head, const float *__restrict__ tbox,
                                                   const int *__restrict__ inds, const int *__restrict__ mask, double *acc) {
  __shared__ double sh[4];
  const int total = d.batch * d.k;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0}, num = 0;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    if (!mask[t]) continue;
    num += 1.0;
    const int b = t / d.k;
    const float *px = head + ((long long)b * d.h * d.w + inds[t]) * d.ld;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float tv = tbox[(long long)t * 8 + j];
      if (tv != tv) continue;                               // isnotnan mask of _reg_loss
      s[j] += (double)fabsf(px[d.reg_ch[j]] - tv);
    }
  }
  double r = block_sum_lane0(num, sh);
  if (threadIdx.x == 0) atomicAdd(acc + 3, r);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    r = block_sum_lane0(s[j], sh);
    if (threadIdx.x == 0) atomicAdd(acc + 4 + j, r);
  }
}

__global__ void k_headloss_finalize(pcp_headloss_t d, const double *acc, float *losses_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  head_losses(acc[0], acc[1], acc[2], acc[3], acc + 4, 8, d.code_weights, d.cls_weight, d.loc_weight, losses_out);
}

// dense part of dL/d(head): heat-map channels get the focal gradient, every other channel of the ld_d-wide row is zeroed
__global__ __launch_bounds__(256) void k_focal_grad(pcp_headloss_t d, const float *__restrict__ head, const float *__restrict__ heat,
                                                   const double *acc, float grad_scale, float *__restrict__ dhead) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)d.batch * d.h * d.w * d.ld_d;
  if (t >= total) return;
  const int ch = (int)(t % d.ld_d);
  const long long pix = t / d.ld_d;
  float gval = 0.f;
  const int c = ch - d.ch_hm;
  if (c >= 0 && c < d.num_class) gval = focal_grad(head[pix * d.ld + ch], heat[pix * d.num_class + c], acc[2], d.cls_weight, grad_scale);
  dhead[t] = gval;
}

__global__ __launch_bounds__(256) void k_reg_grad(pcp_headloss_t d, const float *__restrict__ head, const float *__restrict__ tbox,
                                                 const int *__restrict__ inds, const int *__restrict__ mask, const double *acc,
                                                 float grad_scale, float *__restrict__ dhead) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= d.batch * d.k || !mask[t]) return;
  const double num = clamped_num(acc[3]);
  const int b = t / d.k;
  const long long pix = (long long)b * d.h * d.w + inds[t];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float tv = tbox[(long long)t * 8 + j];
    if (tv != tv) continue;
    const float sg = l1_sign(head[pix * d.ld + d.reg_ch[j]] - tv);
    if (sg != 0.f) atomicAdd(dhead + pix * d.ld_d + d.reg_ch[j], l1_grad_term(sg, d.loc_weight, d.code_weights[j], grad_scale, num));
  }
}

// ---- distillation: one wavefront per pixel, c <= 512 -----------------------------------------------------------------------
constexpr int DIST_MAXV = 8;

__global__ __launch_bounds__(256) void k_distill(const float *__restrict__ fused, int ld_f, const float *__restrict__ early, int ld_e,
                                                long long pixels, int c, float weight, float grad_scale, double *acc,
                                                float *__restrict__ dfused, int ld_d, int accumulate) {
  __shared__ double sh[4];
  const int lane = threadIdx.x & 63;
  const long long wave0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
  const double inv_n = 1.0 / ((double)pixels * (double)c);
  double loss = 0;
  for (long long pix = wave0; pix < pixels; pix += nw) {
    float f[DIST_MAXV], e[DIST_MAXV];
    float mf = -INFINITY, me = -INFINITY;
#pragma unroll
    for (int i = 0; i < DIST_MAXV; ++i) {
      const int ch = lane + 64 * i;
      f[i] = ch < c ? fused[pix * ld_f + ch] : -INFINITY;
      e[i] = ch < c ? early[pix * ld_e + ch] : -INFINITY;
      mf = fmaxf(mf, f[i]);
      me = fmaxf(me, e[i]);
    }
    for (int o = 32; o > 0; o >>= 1) { mf = fmaxf(mf, __shfl_xor(mf, o)); me = fmaxf(me, __shfl_xor(me, o)); }    float sf = 0.f, se = 0.f;
#pragma unroll
    for (int i = 0; i < DIST_MAXV; ++i) {
      f[i] = expf(f[i] - mf);
      e[i] = expf(e[i] - me);
      sf += f[i];
      se += e[i];
    }
    for (int o = 32; o > 0; o >>= 1) { sf += __shfl_xor(sf, o); se += __shfl_xor(se, o); }     // a pair in one loop: two wave_sum calls change the schedule
    float dot = 0.f;
    float gs[DIST_MAXV];
#pragma unroll
    for (int i = 0; i < DIST_MAXV; ++i) {
      f[i] = f[i] / sf;
      const float diff = f[i] - e[i] / se;
      const float ad = fabsf(diff);
      const int ch = lane + 64 * i;
      if (ch < c) loss += (double)(ad < 1.f ? 0.5f * diff * diff : ad - 0.5f);
      gs[i] = ad < 1.f ? diff : (diff > 0.f ? 1.f : -1.f);
      dot += ch < c ? gs[i] * f[i] : 0.f;
    }
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);     // open-coded: the wave_ops.h call changes this kernel's schedule
    if (dfused) {
      const float k = weight * grad_scale * (float)inv_n;
#pragma unroll
      for (int i = 0; i < DIST_MAXV; ++i) {
        const int ch = lane + 64 * i;
        if (ch < c) {
          const float gv = k * f[i] * (gs[i] - dot);
          float *o = dfused + pix * ld_d + ch;
          *o = accumulate ? *o + gv : gv;
        }
      }
    }
  }
  const double s = block_sum_lane0(loss, sh);
  if (threadIdx.x == 0) atomicAdd(acc + 12, s);
}

__global__ void k_distill_finalize(const double *acc, long long pixels, int c, float weight, float *loss_out) {
  if (threadIdx.x == 0 && blockIdx.x == 0) loss_out[0] = (float)(acc[12] / ((double)pixels * (double)c) * (double)weight);
}

}  // namespace

namespace {
constexpr int MSL_BLOCKS = 1024;

__global__ __launch_bounds__(256) void k_masked_sl1(const float *__restrict__ fused, int ld_f, const float *__restrict__ teacher, int ld_t,
                                                   long long pixels, int c, float thresh, double *__restrict__ acc) {
  __shared__ double red[4][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long wave0 = (long long)blockIdx.x * 4 + wv, nw = (long long)gridDim.x * 4;
  double sum = 0.0, cnt = 0.0;
  for (long long pix = wave0; pix < pixels; pix += nw) {
    float n2 = 0.f, l = 0.f;
    for (int ch = lane; ch < c; ch += 64) {
      const float t = teacher[pix * ld_t + ch], d = fused[pix * ld_f + ch] - t, a = fabsf(d);
      n2 = fmaf(t, t, n2);
      l += a < 1.0f ? 0.5f * d * d : a - 0.5f;
    }
    n2 = wave_sum(n2);
    l = wave_sum(l);
    if (sqrtf(n2) > thresh) {
      sum += (double)l;
      cnt += 1.0;
    }
  }
  if (lane == 0) { red[wv][0] = sum; red[wv][1] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc[2 * blockIdx.x] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    acc[2 * blockIdx.x + 1] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
  }
}

__global__ void k_masked_sl1_finalize(const double *__restrict__ acc, int nb, float *__restrict__ loss) {
  double s = 0.0, n = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) { s += acc[2 * i]; n += acc[2 * i + 1]; }
  for (int o = 32; o > 0; o >>= 1) {                                     // a pair in one loop, as in k_distill
    s += __shfl_xor(s, o);
    n += __shfl_xor(n, o);
  }
  if (threadIdx.x == 0) loss[0] = n > 0.0 ? (float)(s / n) : __builtin_nanf("");      // torch: the mean of an empty selection is nan
}
}  // namespace

// ---- a15x: the losses of several heads, with velocity and IoU codes (center_head.py:270-300 for the nuScenes head) ---------------
// Per element and per head these are the a15 functions above (focal_add, focal_grad, head_losses, l1_grad_term); the kernels differ
// on purpose: block partials added in a fixed order and ordered stores where a15 has float64 / float atomics, and no NaN-target mask.
namespace {

// workspace (double) per head: [LX_BLOCKS][3] focal partials (pos, neg, num_pos) | [1 + 16] mask sum and per-code L1 sums | [2] num_pos, num
constexpr int LX_BLOCKS = 64;
constexpr int LX_PER_HEAD = LX_BLOCKS * 3 + 1 + PCP_HEADLOSS_MAX_CODES + 2;

struct LossExtParams {
  pcp_headloss_ext_t d;
  pcp_headloss_head_t heads[PCP_DET_MAX_HEADS];
  int n_heads;
  float grad_scale;
};

// grid (LX_BLOCKS + 1, heads): blocks 0 .. LX_BLOCKS-1 reduce the focal terms of their head, block LX_BLOCKS its L1 sums; every block
// writes its own partial (no atomics), the finalize kernel adds them in block order
__global__ __launch_bounds__(256) void k_lossx_reduce(LossExtParams p, double *__restrict__ ws) {
  __shared__ double sh[4];
  const pcp_headloss_ext_t &d = p.d;
  const pcp_headloss_head_t &hd = p.heads[blockIdx.y];
  double *w = ws + (long long)blockIdx.y * LX_PER_HEAD;
  if (blockIdx.x < LX_BLOCKS) {
    const long long total = (long long)d.batch * d.h * d.w * hd.num_class;
    FocalSums a = {0, 0, 0};
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)LX_BLOCKS * blockDim.x) {
      const int c = (int)(t % hd.num_class);
      const long long pix = t / hd.num_class;
      a = focal_add(a, hd.head[pix * hd.ld + hd.ch_hm + c], hd.heatmap[t]);
    }
    double s = block_sum_lane0(a.pos, sh);
    if (threadIdx.x == 0) w[blockIdx.x * 3 + 0] = s;
    s = block_sum_lane0(a.neg, sh);
    if (threadIdx.x == 0) w[blockIdx.x * 3 + 1] = s;
    s = block_sum_lane0(a.npos, sh);
    if (threadIdx.x == 0) w[blockIdx.x * 3 + 2] = s;
    return;
  }
  double *wr = w + LX_BLOCKS * 3;
  const int total = d.batch * d.k;
  double s[PCP_HEADLOSS_MAX_CODES], num = 0;
#pragma unroll
  for (int j = 0; j < PCP_HEADLOSS_MAX_CODES; ++j) s[j] = 0;
  for (int t = threadIdx.x; t < total; t += blockDim.x) {
    if (!hd.mask[t]) continue;
    num += 1.0;
    const int b = t / d.k;
    const float *px = hd.head + ((long long)b * d.h * d.w + hd.inds[t]) * hd.ld;
    const float *tv = hd.target_boxes + (long long)t * hd.tb_width;
#pragma unroll
    for (int j = 0; j < PCP_HEADLOSS_MAX_CODES; ++j)
      if (j < hd.n_codes) s[j] += (double)fabsf(px[hd.reg_ch[j]] - tv[j]);
  }
  double r = block_sum_lane0(num, sh);
  if (threadIdx.x == 0) wr[0] = r;
#pragma unroll
  for (int j = 0; j < PCP_HEADLOSS_MAX_CODES; ++j) {
    r = block_sum_lane0(s[j], sh);
    if (threadIdx.x == 0) wr[1 + j] = r;
  }
}

// one thread per head, then thread 0 adds the heads in order
__global__ void k_lossx_finalize(LossExtParams p, double *__restrict__ ws, float *__restrict__ losses, float *__restrict__ total) {
  __shared__ double sums[PCP_DET_MAX_HEADS];
  const int h = threadIdx.x;
  if (h < p.n_heads) {
    const pcp_headloss_ext_t &d = p.d;
    double *w = ws + (long long)h * LX_PER_HEAD;
    double pos = 0, neg = 0, npos = 0;
    for (int i = 0; i < LX_BLOCKS; ++i) { pos += w[i * 3]; neg += w[i * 3 + 1]; npos += w[i * 3 + 2]; }
    const double *wr = w + LX_BLOCKS * 3;
    sums[h] = (double)head_losses(pos, neg, npos, wr[0], wr + 1, p.heads[h].n_codes, d.code_weights, d.cls_weight, d.loc_weight,
                                  losses + h * 4);
    w[LX_PER_HEAD - 2] = npos;
    w[LX_PER_HEAD - 1] = wr[0];
  }
  __syncthreads();
  if (h == 0) {
    float t = 0.f;                                            // the reference adds the float32 per-head losses in head order (:295)
    for (int i = 0; i < p.n_heads; ++i) t += (float)sums[i];
    total[0] = t;
  }
}

// grid (blocks, heads): k_focal_grad per head
__global__ __launch_bounds__(256) void k_lossx_focal_grad(LossExtParams p, const double *__restrict__ ws) {
  const pcp_headloss_ext_t &d = p.d;
  const pcp_headloss_head_t &hd = p.heads[blockIdx.y];
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long total = (long long)d.batch * d.h * d.w * hd.ld_d;
  if (t >= total) return;
  const int ch = (int)(t % hd.ld_d);
  const long long pix = t / hd.ld_d;
  float gval = 0.f;
  const int c = ch - hd.ch_hm;
  if (c >= 0 && c < hd.num_class)
    gval = focal_grad(hd.head[pix * hd.ld + ch], hd.heatmap[pix * hd.num_class + c], ws[(long long)blockIdx.y * LX_PER_HEAD + LX_PER_HEAD - 2],
                      d.cls_weight, p.grad_scale);
  hd.dhead[t] = gval;
}

// grid (blocks, heads), after k_lossx_focal_grad (the regression channels are zero).  Slots of one frame that share a cell: the first of
// them adds all their terms in slot order and stores once -- no atomics, one fixed order.
__global__ __launch_bounds__(256) void k_lossx_reg_grad(LossExtParams p, const double *__restrict__ ws) {
  const pcp_headloss_ext_t &d = p.d;
  const pcp_headloss_head_t &hd = p.heads[blockIdx.y];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= d.batch * d.k || !hd.mask[t]) return;
  const int b = t / d.k, k0 = t - b * d.k;
  const int *inds = hd.inds + b * d.k, *mask = hd.mask + b * d.k;
  const int cell = inds[k0];
  for (int k = 0; k < k0; ++k)
    if (mask[k] && inds[k] == cell) return;
  const double num = clamped_num(ws[(long long)blockIdx.y * LX_PER_HEAD + LX_PER_HEAD - 1]);
  const long long pix = (long long)b * d.h * d.w + cell;
  float acc[PCP_HEADLOSS_MAX_CODES];
#pragma unroll
  for (int j = 0; j < PCP_HEADLOSS_MAX_CODES; ++j) acc[j] = 0.f;
  for (int k = k0; k < d.k; ++k) {
    if (!mask[k] || inds[k] != cell) continue;
    const float *tv = hd.target_boxes + ((long long)b * d.k + k) * hd.tb_width;
#pragma unroll
    for (int j = 0; j < PCP_HEADLOSS_MAX_CODES; ++j) {
      if (j >= hd.n_codes) continue;
      const float sg = l1_sign(hd.head[pix * hd.ld + hd.reg_ch[j]] - tv[j]);
      if (sg != 0.f) acc[j] += l1_grad_term(sg, d.loc_weight, d.code_weights[j], p.grad_scale, num);
    }
  }
  // two codes never share a channel (checked on the host), so these are plain stores
#pragma unroll
  for (int j = 0; j < PCP_HEADLOSS_MAX_CODES; ++j)
    if (j < hd.n_codes) hd.dhead[pix * hd.ld_d + hd.reg_ch[j]] = acc[j];
}

}  // namespace

extern "C" {

int pcp_centerhead_targets_ext(const pcp_target_t *d, const pcp_target_head_t *heads, int32_t n_heads, const float *gt_boxes,
                               int32_t max_boxes, int32_t box_width, int32_t with_iou, void *stream) {
  if (!d || !heads || !gt_boxes || n_heads <= 0 || n_heads > PCP_DET_MAX_HEADS) return PCP_ERR_ARG;
  if (d->batch <= 0 || d->h <= 0 || d->w <= 0 || d->k <= 0 || max_boxes < 0) return PCP_ERR_ARG;
  if (box_width != 8 && box_width != 10) return PCP_ERR_ARG;
  if (max_boxes > TGT_MAX_BOXES) return PCP_ERR_UNSUPPORTED;
  TgtExtParams p;
  p.d = *d;
  p.bw = box_width;
  p.with_iou = with_iou ? 1 : 0;
  p.tw = 8 + (box_width == 10 ? 2 : 0) + p.with_iou;
  for (int i = 0; i < n_heads; ++i) {
    const pcp_target_head_t &h = heads[i];
    if (!h.heatmap || !h.target_boxes || !h.inds || !h.mask || h.num_class <= 0) return PCP_ERR_ARG;
    if (h.class_to_local[0] != 0) return PCP_ERR_ARG;
    for (int c = 0; c < PCP_TGT_MAX_CLASSES; ++c)
      if (h.class_to_local[c] < 0 || h.class_to_local[c] > h.num_class) return PCP_ERR_ARG;
    if (p.with_iou) {
      if (!h.head || h.ld <= 0 || h.ch_center < 0 || h.ch_z < 0 || h.ch_dim < 0 || h.ch_rot < 0) return PCP_ERR_ARG;
      if (h.ch_center + 2 > h.ld || h.ch_z >= h.ld || h.ch_dim + 3 > h.ld || h.ch_rot + 2 > h.ld) return PCP_ERR_ARG;
    }
    p.heads[i] = h;
  }
  hipLaunchKernelGGL(k_targets_ext, dim3(n_heads * d->batch), dim3(TGT_THREADS), 0, (hipStream_t)stream, p, gt_boxes, max_boxes);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

size_t pcp_centerhead_loss_ext_workspace_bytes(int32_t n_heads) {
  return (size_t)(n_heads > 0 ? n_heads : 0) * LX_PER_HEAD * sizeof(double);
}

int pcp_centerhead_loss_ext(const pcp_headloss_ext_t *d, const pcp_headloss_head_t *heads, int32_t n_heads, float grad_scale,
                            void *workspace, size_t workspace_bytes, float *losses, float *total, void *stream) {
  if (!d || !heads || !workspace || !losses || !total || n_heads <= 0 || n_heads > PCP_DET_MAX_HEADS) return PCP_ERR_ARG;
  if (d->batch <= 0 || d->h <= 0 || d->w <= 0 || d->k <= 0) return PCP_ERR_ARG;
  if (workspace_bytes < pcp_centerhead_loss_ext_workspace_bytes(n_heads)) return PCP_ERR_WORKSPACE;
  LossExtParams p;
  p.d = *d;
  p.n_heads = n_heads;
  p.grad_scale = grad_scale;
  const bool with_grad = heads[0].dhead != nullptr;
  long long max_total = 0;
  for (int i = 0; i < n_heads; ++i) {
    const pcp_headloss_head_t &h = heads[i];
    if (!h.head || !h.heatmap || !h.target_boxes || !h.inds || !h.mask) return PCP_ERR_ARG;
    if ((h.dhead != nullptr) != with_grad) return PCP_ERR_ARG;
    if (h.ld <= 0 || h.num_class <= 0 || h.ch_hm < 0 || h.ch_hm + h.num_class > h.ld) return PCP_ERR_ARG;
    if (h.n_codes <= 0 || h.n_codes > PCP_HEADLOSS_MAX_CODES || h.tb_width != h.n_codes) return PCP_ERR_ARG;
    if (with_grad && (h.ld_d <= 0 || h.ch_hm + h.num_class > h.ld_d)) return PCP_ERR_ARG;
    for (int j = 0; j < h.n_codes; ++j) {
      if (h.reg_ch[j] < 0 || h.reg_ch[j] >= h.ld || (with_grad && h.reg_ch[j] >= h.ld_d)) return PCP_ERR_ARG;
      if (h.reg_ch[j] >= h.ch_hm && h.reg_ch[j] < h.ch_hm + h.num_class) return PCP_ERR_ARG;
      for (int i2 = 0; i2 < j; ++i2)
        if (h.reg_ch[i2] == h.reg_ch[j]) return PCP_ERR_ARG;
    }
    if (with_grad) {
      const long long t = (long long)d->batch * d->h * d->w * h.ld_d;
      if (t > max_total) max_total = t;
    }
    p.heads[i] = h;
  }
  hipStream_t s = (hipStream_t)stream;
  double *ws = (double *)workspace;
  hipLaunchKernelGGL(k_lossx_reduce, dim3(LX_BLOCKS + 1, n_heads), dim3(256), 0, s, p, ws);
  hipLaunchKernelGGL(k_lossx_finalize, dim3(1), dim3(64), 0, s, p, ws, losses, total);
  if (with_grad) {
    const int nk = d->batch * d->k;
    hipLaunchKernelGGL(k_lossx_focal_grad, dim3((unsigned)((max_total + 255) / 256), n_heads), dim3(256), 0, s, p, ws);
    hipLaunchKernelGGL(k_lossx_reg_grad, dim3((nk + 255) / 256, n_heads), dim3(256), 0, s, p, ws);
  }
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

int pcp_centerhead_targets(const pcp_target_t *d, const float *gt_boxes, int32_t max_boxes, float *heatmap, float *target_boxes,
                           int32_t *inds, int32_t *mask, void *stream) {
  if (!d || !gt_boxes || !heatmap || !target_boxes || !inds || !mask) return PCP_ERR_ARG;
  if (d->batch <= 0 || d->h <= 0 || d->w <= 0 || d->num_class <= 0 || d->k <= 0 || max_boxes < 0) return PCP_ERR_ARG;
  if (max_boxes > TGT_MAX_BOXES) return PCP_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (pcp_zero_async(heatmap, (size_t)d->batch * d->h * d->w * d->num_class * sizeof(float), s) != PCP_OK) return PCP_ERR_LAUNCH;
  hipLaunchKernelGGL(k_targets, dim3(d->batch), dim3(TGT_THREADS), 0, s, *d, gt_boxes, max_boxes, heatmap, target_boxes, inds, mask);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

size_t pcp_loss_workspace_bytes(void) { return (size_t)(ACC_N > 2 * MSL_BLOCKS ? ACC_N : 2 * MSL_BLOCKS) * sizeof(double); }

int pcp_centerhead_loss(const pcp_headloss_t *d, const float *head, const float *heatmap, const float *target_boxes,
                        const int32_t *inds, const int32_t *mask, float grad_scale, void *workspace, float *losses, float *dhead,
                        void *stream) {
  if (!d || !head || !heatmap || !target_boxes || !inds || !mask || !workspace || !losses) return PCP_ERR_ARG;
  if (d->batch <= 0 || d->h <= 0 || d->w <= 0 || d->num_class <= 0 || d->k <= 0 || d->ld <= 0) return PCP_ERR_ARG;
  if (dhead && d->ld_d <= 0) return PCP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  double *acc = (double *)workspace;
  if (pcp_zero_async(acc, 12 * sizeof(double), s) != PCP_OK) return PCP_ERR_LAUNCH;     // [12] belongs to the distillation loss
  const long long cells = (long long)d->batch * d->h * d->w * d->num_class;
  int blocks = (int)((cells + 255) / 256);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(k_focal_reduce, dim3(blocks), dim3(256), 0, s, *d, head, heatmap, acc);
  const int nk = d->batch * d->k;
  hipLaunchKernelGGL(k_reg_reduce, dim3((nk + 255) / 256 > 64 ? 64 : (nk + 255) / 256), dim3(256), 0, s, *d, head, target_boxes, inds,
                     mask, acc);
  hipLaunchKernelGGL(k_headloss_finalize, dim3(1), dim3(64), 0, s, *d, acc, losses);
  if (dhead) {
    const long long total = (long long)d->batch * d->h * d->w * d->ld_d;
    hipLaunchKernelGGL(k_focal_grad, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, *d, head, heatmap, acc, grad_scale, dhead);
    hipLaunchKernelGGL(k_reg_grad, dim3((nk + 255) / 256), dim3(256), 0, s, *d, head, target_boxes, inds, mask, acc, grad_scale, dhead);
  }
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

// HunterJr's teacher-BEV term (hunter_jr.py:352-365): mean over the pixels whose teacher row has an L2 norm > thresh of the per-pixel SUM
// of smooth_l1(fused - teacher) (beta = 1).  The reference stores the value in forward_return_dict['loss_dtl_bev_img'] and never adds it
// to the training loss (hunter_jr.py:490-494), so no gradient is formed.  One wavefront per pixel, block partials in float64 reduced in a
// fixed order by one wave (deterministic).
int pcp_masked_smooth_l1_rows(const float *fused, int32_t ld_f, const float *teacher, int32_t ld_t, int64_t pixels, int32_t c, float thresh,
                              void *workspace, float *loss, void *stream) {
  if (!fused || !teacher || !workspace || !loss || pixels <= 0 || c <= 0) return PCP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  double *acc = (double *)workspace;                         // [MSL_BLOCKS][2]: sum, count
  long long blocks = (pixels + 3) / 4;
  if (blocks > MSL_BLOCKS) blocks = MSL_BLOCKS;
  hipLaunchKernelGGL(k_masked_sl1, dim3((unsigned)blocks), dim3(256), 0, s, fused, ld_f, teacher, ld_t, (long long)pixels, c, thresh, acc);
  hipLaunchKernelGGL(k_masked_sl1_finalize, dim3(1), dim3(64), 0, s, acc, (int)blocks, loss);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

int pcp_distill_loss(const float *fused, int32_t ld_f, const float *early, int32_t ld_e, int64_t pixels, int32_t c, float weight,
                     float grad_scale, void *workspace, float *loss, float *dfused, int32_t ld_d, int32_t accumulate, void *stream) {
  if (!fused || !early || !workspace || !loss || pixels <= 0 || c <= 0 || c > 64 * DIST_MAXV) return PCP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  double *acc = (double *)workspace;
  if (pcp_zero_async(acc + 12, 4 * sizeof(double), s) != PCP_OK) return PCP_ERR_LAUNCH;
  long long blocks = (pixels + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_distill, dim3((unsigned)blocks), dim3(256), 0, s, fused, ld_f, early, ld_e, (long long)pixels, c, weight,
                     grad_scale, acc, dfused, ld_d, accumulate);
  hipLaunchKernelGGL(k_distill_finalize, dim3(1), dim3(64), 0, s, acc, (long long)pixels, c, weight, loss);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

}  // extern "C"
