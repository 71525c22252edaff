// gt_sampling on the device: the ground-truth database paste of the reference's DataBaseSampler (pcdet/datasets/augmentor/
// database_sampler.py) on a collated training batch (include/pcp_hip_train.h: pcp_gt_sample_select / _paste_points / _paste_boxes).
//
// The reference draws candidates per class on the host, rejects every candidate whose BEV IoU with an existing box or with another
// candidate of its class is positive, and appends the survivors' stored points and boxes to the sample.  Here the host only draws (the
// numpy state machine) and ships a candidate table; the collision test, the selection and the paste run on the batch where it lies:
//   k_gts_select  one workgroup per frame: classes in order, candidate x existing and candidate x candidate pairs over the lanes with the
//                 overlap arithmetic of nms.hip (bev_geom.h, contraction off), the accepted boxes join the existing list in LDS.
//   k_gts_bounds  the first row of every frame in the (ascending) collated rows; a descending neighbour pair sets the error word.
//   k_gts_paste   one workgroup per tile of PCP_AUG_TILE_ROWS OUTPUT rows.  A tile is a sequence of pieces (a run of a frame's own rows,
//                 or a run of one accepted object's rows); every piece is copied into LDS at its place in the tile, own rows with 16-byte
//                 loads from the 16-byte aligned part of their source, and the tile leaves with 16-byte stores (the tile starts 16-byte
//                 aligned for every stride, as in augment.hip).  Positions come from prefix sums only: no atomics, a call repeats bit for bit.
//                 Measured against k_gts_paste_rows, the plain thread-per-row form of the same paste (profiles/gt_sampling_bench.txt,
//                 tools/bench_augment.py --gt-sampling): 25 against 27 us at 260 000 rows x 13 floats, 42 against 91 us at four such
//                 frames, so the tiles are the default and the row form stays behind PCP_OPT_GTS_PASTE_FORM = 1 for that comparison.
//   k_gts_boxes   one thread per output box row / instance matrix.
#include "pcp_common.h"

#pragma clang fp contract(off)

namespace {

#include "aug_tile.h"
#include "bev_geom.h"

constexpr int GTS_THREADS = 256;
constexpr int CS = PCP_GTS_CAND_STRIDE;
constexpr int AS = PCP_GTS_ACC_STRIDE;
static_assert((PCP_AUG_TILE_ROWS * PCP_AUG_MAX_ROW_STRIDE + 4) * 4 <= 65536, "a tile fits the LDS of one workgroup");

__global__ __launch_bounds__(GTS_THREADS) void k_gts_select(const float *__restrict__ gt, int max_boxes, int W, const int *__restrict__ frame_table,
                                                            int G, const int *__restrict__ cand_db, const float *__restrict__ cand_box,
                                                            int n_cand, const int *__restrict__ db_count, int n_db, int *__restrict__ acc,
                                                            int acc_cap, int *__restrict__ counts, int batch) {
  __shared__ float ex[PCP_GTS_MAX_BOXES * 5];                        // existing + accepted: x y dx dy heading
  __shared__ float cb[PCP_GTS_MAX_CAND * 5];
  __shared__ int hit[PCP_GTS_MAX_CAND];
  __shared__ int s_state[3];                                         // boxes in ex, accepted, rows added
  const int b = blockIdx.x, t = threadIdx.x;
  const int *ft = frame_table + (size_t)b * (G + 2);
  int n_ex = min(max(ft[0], 0), min(max_boxes, PCP_GTS_MAX_BOXES));
  for (int i = t; i < n_ex; i += GTS_THREADS) {
    const float *p = gt + ((size_t)b * max_boxes + i) * W;
    ex[i * 5 + 0] = p[0];
    ex[i * 5 + 1] = p[1];
    ex[i * 5 + 2] = p[3];
    ex[i * 5 + 3] = p[4];
    ex[i * 5 + 4] = p[6];
  }
  int n_acc = 0, rows = 0;
  __syncthreads();
  for (int g = 0; g < G; g++) {
    const int s = ft[1 + g];
    const int nc = min(min(ft[2 + g], n_cand) - s, PCP_GTS_MAX_CAND);
    if (s < 0 || nc <= 0) continue;                                   // uniform over the workgroup
    if (t < nc) {
      const float *p = cand_box + (size_t)(s + t) * CS;
      cb[t * 5 + 0] = p[0];
      cb[t * 5 + 1] = p[1];
      cb[t * 5 + 2] = p[3];
      cb[t * 5 + 3] = p[4];
      cb[t * 5 + 4] = p[6];
      hit[t] = 0;
    }
    __syncthreads();
    const int tot = n_ex + nc;
    for (int p = t; p < nc * tot; p += GTS_THREADS) {
      const int i = p / tot, j = p - i * tot;
      const float *o = j < n_ex ? ex + j * 5 : cb + (j - n_ex) * 5;
      if (j - n_ex == i) continue;                                    // iou2's zeroed diagonal
      Box A, B;
      A.x = cb[i * 5]; A.y = cb[i * 5 + 1]; A.dx = cb[i * 5 + 2]; A.dy = cb[i * 5 + 3]; A.ang = cb[i * 5 + 4];
      B.x = o[0]; B.y = o[1]; B.dx = o[2]; B.dy = o[3]; B.ang = o[4];
      if (iou_of(A, B) > 0.f) hit[i] = 1;                             // iou1.max + iou2.max == 0 <=> no positive IoU at all
    }
    __syncthreads();
    if (t == 0) {                                                     // the accepted candidates in slot order join the existing boxes
      for (int i = 0; i < nc; i++) {
        if (hit[i]) continue;
        const int db = cand_db[s + i];
        if (db < 0 || db >= n_db || n_ex >= PCP_GTS_MAX_BOXES || n_acc >= acc_cap) continue;   // the host refuses these before the launch
        const int cnt = max(db_count[db], 0);
        int *a = acc + ((size_t)b * acc_cap + n_acc) * AS;
        a[0] = s + i;
        a[1] = db;
        a[2] = rows;
        a[3] = cnt;
#pragma unroll
        for (int c = 0; c < 5; c++) ex[n_ex * 5 + c] = cb[i * 5 + c];
        n_ex++;
        n_acc++;
        rows += cnt;
      }
      s_state[0] = n_ex;
      s_state[1] = n_acc;
      s_state[2] = rows;
    }
    __syncthreads();
    n_ex = s_state[0];
    n_acc = s_state[1];
    rows = s_state[2];
    __syncthreads();                                                  // s_state, cb and hit are rewritten by the next class
  }
  if (t == 0) {
    counts[b] = n_acc;
    counts[batch + b] = rows;
    if (b == 0) counts[2 * batch] = 0;                                // the error word of the paste that follows
  }
}

// seg[k] = first row of frame k (k = batch: n), from the neighbour pairs of the ascending frame column
__global__ __launch_bounds__(256) void k_gts_bounds(const float *__restrict__ points, long long n, int S, int batch, int *__restrict__ seg,
                                                    int *__restrict__ err) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n == 0) {
    if (i <= batch) seg[i] = 0;
    return;
  }
  if (i >= n) return;
  const float fv = points[i * S];
  if (!(fv >= 0.f && fv < (float)batch)) {
    *err = 2;
    return;
  }
  const int f = (int)fv;
  int prev = -1;
  if (i > 0) {
    const float pv = points[(i - 1) * S];
    if (!(pv >= 0.f && pv < (float)batch)) return;                    // that row's own thread reports it
    prev = (int)pv;
  }
  if (f < prev) {
    *err = 1;
    return;
  }
  for (int k = prev + 1; k <= f; k++) seg[k] = (int)i;
  if (i == n - 1)
    for (int k = f + 1; k <= batch; k++) seg[k] = (int)n;
}

// `count` floats src[s0 ..) -> lds[d0 ..): 16-byte loads over the 16-byte aligned middle of the source (src itself is 16-byte aligned)
__device__ __forceinline__ void gts_copy_own(float *lds, int d0, const float *__restrict__ src, long long s0, int count) {
  int h = (int)((4 - (s0 & 3)) & 3);
  if (h > count) h = count;
  for (int i = threadIdx.x; i < h; i += GTS_THREADS) lds[d0 + i] = src[s0 + i];
  const int n4 = (count - h) >> 2;
  const f32x4 *s4 = reinterpret_cast<const f32x4 *>(src + s0 + h);
  for (int i = threadIdx.x; i < n4; i += GTS_THREADS) {
    const f32x4 v = s4[i];
    float *d = lds + d0 + h + 4 * i;
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }
  for (int i = h + 4 * n4 + threadIdx.x; i < count; i += GTS_THREADS) lds[d0 + i] = src[s0 + i];
}

__global__ __launch_bounds__(GTS_THREADS) void k_gts_paste(const float *__restrict__ points, int S, int batch, const int *__restrict__ seg,
                                                           const int *__restrict__ counts, const int *__restrict__ acc, int acc_cap,
                                                           const int *__restrict__ frame_table, int G, const float *__restrict__ cand_box,
                                                           const float *__restrict__ db_points, const int *__restrict__ db_off, int inst_col,
                                                           float *__restrict__ out) {
  extern __shared__ f32x4 gts_lds4[];
  float *tile = reinterpret_cast<float *>(gts_lds4);
  if (counts[2 * batch] != 0) return;                                 // rows not grouped by ascending frame: nothing is written
  const long long o0 = (long long)blockIdx.x * PCP_AUG_TILE_ROWS;
  // the frame the tile starts in: fs = first output row of frame b.  Every thread walks the same few values (uniform loads).
  int b = 0;
  long long fs = 0;
  for (; b < batch; b++) {
    const long long tot = (long long)(seg[b + 1] - seg[b]) + counts[batch + b];
    if (o0 < fs + tot) break;
    fs += tot;
  }
  if (b == batch) return;                                             // a tile behind the last output row
  const int C = S - 1;
  long long r = o0;
  const long long end = o0 + PCP_AUG_TILE_ROWS;
  while (r < end && b < batch) {
    const int own = seg[b + 1] - seg[b], add = counts[batch + b];
    const long long q = r - fs;
    if (q >= (long long)own + add) {
      fs += (long long)own + add;
      b++;
      continue;
    }
    const int d0 = (int)(r - o0) * S;
    int len;
    if (q < own) {
      len = (int)min((long long)own - q, end - r);
      gts_copy_own(tile, d0, points, ((long long)seg[b] + q) * S, len * S);
    } else {
      const int qq = (int)(q - own), n_acc = counts[b];
      const int *ab = acc + (size_t)b * acc_cap * AS;
      int lo = 0, hi = n_acc - 1;                                     // the last object whose exclusive prefix is <= qq
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ab[mid * AS + 2] <= qq) lo = mid;
        else hi = mid - 1;
      }
      const int slot = ab[lo * AS], db = ab[lo * AS + 1], inner = qq - ab[lo * AS + 2];
      len = (int)min((long long)(ab[lo * AS + 3] - inner), end - r);
      const float *ctr = cand_box + (size_t)slot * CS;
      const float cx = ctr[0], cy = ctr[1], cz = ctr[2];
      const float inst = (float)(frame_table[(size_t)b * (G + 2)] + lo);   // num_original_instances + idx
      const float *src = db_points + ((long long)db_off[db] + inner) * C;
      for (int f = threadIdx.x; f < len * S; f += GTS_THREADS) {
        const int row = f / S, col = f - row * S;
        float v;
        if (col == 0) v = (float)b;
        else {
          v = src[row * C + col - 1];
          if (col == 1) v = __fadd_rn(v, cx);                          // obj_points[:, :3] += box3d_lidar[:3].astype(float32)
          else if (col == 2) v = __fadd_rn(v, cy);
          else if (col == 3) v = __fadd_rn(v, cz);
          else if (col == inst_col) v = inst;
        }
        tile[d0 + f] = v;
      }
    }
    if (len <= 0) break;                                              // an accepted list that does not cover its row count: stop, never spin
    r += len;
  }
  __syncthreads();
  // r <= total output rows: the stores stay inside them; out + o0 * S is 16-byte aligned (PCP_AUG_TILE_ROWS * 4 * S bytes per tile)
  aug_stage_out<GTS_THREADS>(out + o0 * S, tile, 0, (int)(r - o0) * S);
}

// The plain form of the same paste (option PCP_OPT_GTS_PASTE_FORM = 1; tools/bench_augment.py --gt-sampling times both): one thread per
// output row, dword loads and stores, no LDS.
__global__ __launch_bounds__(256) void k_gts_paste_rows(const float *__restrict__ points, int S, int batch, const int *__restrict__ seg,
                                                        const int *__restrict__ counts, const int *__restrict__ acc, int acc_cap,
                                                        const int *__restrict__ frame_table, int G, const float *__restrict__ cand_box,
                                                        const float *__restrict__ db_points, const int *__restrict__ db_off, int inst_col,
                                                        float *__restrict__ out) {
  if (counts[2 * batch] != 0) return;
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  int b = 0;
  long long fs = 0;
  for (; b < batch; b++) {
    const long long tot = (long long)(seg[b + 1] - seg[b]) + counts[batch + b];
    if (r < fs + tot) break;
    fs += tot;
  }
  if (b == batch) return;                                             // behind the last output row
  const int own = seg[b + 1] - seg[b];
  const long long q = r - fs;
  float *dst = out + r * S;
  if (q < own) {
    const float *src = points + ((long long)seg[b] + q) * S;
    for (int c = 0; c < S; c++) dst[c] = src[c];
    return;
  }
  const int qq = (int)(q - own), n_acc = counts[b];
  const int *ab = acc + (size_t)b * acc_cap * AS;
  int lo = 0, hi = n_acc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (ab[mid * AS + 2] <= qq) lo = mid;
    else hi = mid - 1;
  }
  const int inner = qq - ab[lo * AS + 2];
  if (inner >= ab[lo * AS + 3]) return;
  const float *ctr = cand_box + (size_t)ab[lo * AS] * CS;
  const float *src = db_points + ((long long)db_off[ab[lo * AS + 1]] + inner) * (S - 1);
  dst[0] = (float)b;
  dst[1] = __fadd_rn(src[0], ctr[0]);
  dst[2] = __fadd_rn(src[1], ctr[1]);
  dst[3] = __fadd_rn(src[2], ctr[2]);
  for (int c = 4; c < S; c++) dst[c] = c == inst_col ? (float)(frame_table[(size_t)b * (G + 2)] + lo) : src[c - 1];
}

// one thread per output box row (k == 0) or instance matrix (k >= 1) of (b, m), m < m_out
__global__ __launch_bounds__(256) void k_gts_boxes(const float *__restrict__ gt_in, int M, int W, const float *__restrict__ tf_in, int n_sweeps,
                                                   int R, int batch, const int *__restrict__ frame_table, int G, const int *__restrict__ counts,
                                                   const int *__restrict__ acc, int acc_cap, const float *__restrict__ cand_box,
                                                   const float *__restrict__ db_tf, float *__restrict__ gt_out, float *__restrict__ tf_out,
                                                   int m_out) {
  const int per = 1 + (tf_out ? n_sweeps : 0);
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)batch * m_out * per) return;
  const int k = (int)(idx % per);
  const long long obj = idx / per;
  const int b = (int)(obj / m_out), m = (int)(obj % m_out);
  const int n_own = min(max(frame_table[(size_t)b * (G + 2)], 0), M), n_acc = counts[b];
  const int kind = m < n_own ? 0 : (m < n_own + n_acc ? 1 : 2);       // own row, accepted object, padding
  const int *a = acc + ((size_t)b * acc_cap + (kind == 1 ? m - n_own : 0)) * AS;
  if (k == 0) {
    float *o = gt_out + obj * W;
    if (kind == 0) {
      const float *s = gt_in + ((size_t)b * M + m) * W;
      for (int c = 0; c < W; c++) o[c] = s[c];
    } else if (kind == 1) {
      const float *s = cand_box + (size_t)a[0] * CS;
      for (int c = 0; c < 7; c++) o[c] = s[c];
      if (W == 10) {
        o[7] = s[7];
        o[8] = s[8];
      }
      o[W - 1] = s[9];
    } else {
      for (int c = 0; c < W; c++) o[c] = 0.f;
    }
    return;
  }
  float *o = tf_out + (obj * n_sweeps + (k - 1)) * (long long)(R * 4);
  if (kind == 0) {
    const float *s = tf_in + (((size_t)b * M + m) * n_sweeps + (k - 1)) * (size_t)(R * 4);
    for (int c = 0; c < R * 4; c++) o[c] = s[c];
  } else if (kind == 1) {
    const float *s = db_tf + ((size_t)a[1] * n_sweeps + (k - 1)) * 16;   // the first R rows of the stored 4 x 4
    for (int c = 0; c < R * 4; c++) o[c] = s[c];
  } else {
    for (int c = 0; c < R * 4; c++) o[c] = aug_identity_pad(c);
  }
}

}  // namespace

extern "C" int pcp_gt_sample_select(const float *gt_boxes, int32_t batch, int32_t max_boxes, int32_t box_width, const int32_t *frame_table,
                                    int32_t n_groups, const int32_t *cand_db, const float *cand_box, int32_t n_cand, const int32_t *db_count,
                                    int32_t n_db, int32_t *accepted, int32_t acc_cap, int32_t *counts, void *stream) {
  if (batch <= 0 || batch > PCP_AUG_MAX_BATCH || n_groups <= 0 || n_groups > PCP_GTS_MAX_GROUPS || max_boxes < 0 || n_cand < 0 || n_db < 0 ||
      acc_cap < 0 || (box_width != 8 && box_width != 10))
    return PCP_ERR_ARG;
  if (!frame_table || !counts || (max_boxes > 0 && !gt_boxes) || (n_cand > 0 && (!cand_db || !cand_box || !db_count)) || (acc_cap > 0 && !accepted))
    return PCP_ERR_ARG;
  hipLaunchKernelGGL(k_gts_select, dim3(batch), dim3(GTS_THREADS), 0, (hipStream_t)stream, gt_boxes, (int)max_boxes, (int)box_width, frame_table,
                     (int)n_groups, cand_db, cand_box, (int)n_cand, db_count, (int)n_db, accepted, (int)acc_cap, counts, (int)batch);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_gt_sample_paste_points(const float *points, int64_t n, int32_t row_stride, int32_t batch, const int32_t *frame_table,
                                          int32_t n_groups, const int32_t *accepted, int32_t acc_cap, const int32_t *counts,
                                          const float *cand_box, const float *db_points, const int32_t *db_offset, int32_t inst_col,
                                          int64_t max_added, float *out, int32_t *segments, void *stream_) {
  if (batch <= 0 || batch > PCP_AUG_MAX_BATCH || n_groups <= 0 || n_groups > PCP_GTS_MAX_GROUPS || n < 0 || max_added < 0 || acc_cap < 0 ||
      row_stride < PCP_AUG_MIN_ROW_STRIDE || row_stride > PCP_AUG_MAX_ROW_STRIDE || inst_col < 4 || inst_col >= row_stride)
    return PCP_ERR_ARG;
  if (!frame_table || !counts || !segments || (n > 0 && !points) || (max_added > 0 && (!accepted || !cand_box || !db_points || !db_offset)))
    return PCP_ERR_ARG;
  if ((n + max_added) * row_stride >= (1LL << 31)) return PCP_ERR_UNSUPPORTED;   // LDS and tile indices are ints
  if ((((uintptr_t)points) | ((uintptr_t)out)) & 15) return PCP_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const long long nb = n > 0 ? (n + 255) / 256 : 1;
  hipLaunchKernelGGL(k_gts_bounds, dim3((unsigned)nb), dim3(256), 0, stream, points, (long long)n, (int)row_stride, (int)batch, (int *)segments,
                     (int *)counts + 2 * batch);
  PCP_CHECK_LAUNCH();
  if (n + max_added == 0) return PCP_OK;
  if (!out) return PCP_ERR_ARG;
  if (pcp_option(PCP_OPT_GTS_PASTE_FORM, 0) == 1) {
    hipLaunchKernelGGL(k_gts_paste_rows, dim3((unsigned)((n + max_added + 255) / 256)), dim3(256), 0, stream, points, (int)row_stride, (int)batch,
                       (const int *)segments, (const int *)counts, (const int *)accepted, (int)acc_cap, (const int *)frame_table, (int)n_groups,
                       cand_box, db_points, (const int *)db_offset, (int)inst_col, out);
    PCP_CHECK_LAUNCH();
    return PCP_OK;
  }
  const int tiles = (int)((n + max_added + PCP_AUG_TILE_ROWS - 1) / PCP_AUG_TILE_ROWS);
  hipLaunchKernelGGL(k_gts_paste, dim3(tiles), dim3(GTS_THREADS), (size_t)PCP_AUG_TILE_ROWS * row_stride * 4, stream, points, (int)row_stride,
                     (int)batch, (const int *)segments, (const int *)counts, (const int *)accepted, (int)acc_cap, (const int *)frame_table,
                     (int)n_groups, cand_box, db_points, (const int *)db_offset, (int)inst_col, out);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_gt_sample_paste_boxes(const float *gt_boxes, int32_t batch, int32_t max_boxes, int32_t box_width, const float *instances_tf,
                                         int32_t n_sweeps, int32_t tf_rows, const int32_t *frame_table, int32_t n_groups,
                                         const int32_t *accepted, int32_t acc_cap, const int32_t *counts, const float *cand_box,
                                         const float *db_tf, float *gt_out, float *tf_out, int32_t max_boxes_out, void *stream) {
  if (batch <= 0 || batch > PCP_AUG_MAX_BATCH || n_groups <= 0 || n_groups > PCP_GTS_MAX_GROUPS || max_boxes < 0 || max_boxes_out < 0 ||
      acc_cap < 0 || (box_width != 8 && box_width != 10))
    return PCP_ERR_ARG;
  if (tf_out && (!db_tf || n_sweeps <= 0 || (tf_rows != 3 && tf_rows != 4) || (max_boxes > 0 && !instances_tf))) return PCP_ERR_ARG;
  if (max_boxes_out == 0) return PCP_OK;
  if (!frame_table || !counts || !gt_out || (max_boxes > 0 && !gt_boxes) || (acc_cap > 0 && (!accepted || !cand_box))) return PCP_ERR_ARG;
  const long long total = (long long)batch * max_boxes_out * (1 + (tf_out ? n_sweeps : 0));
  if (total >= (1LL << 31)) return PCP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_gts_boxes, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gt_boxes, (int)max_boxes,
                     (int)box_width, instances_tf, (int)n_sweeps, (int)tf_rows, (int)batch, frame_table, (int)n_groups, counts, accepted,
                     (int)acc_cap, cand_box, db_tf, gt_out, tf_out, (int)max_boxes_out);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}
