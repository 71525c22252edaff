// World augmentation of a collated training batch on the device (include/pcp_hip_train.h: pcp_world_augment_points / _boxes).
//
// The reference augments every sample on the host before collation (data_augmentor.py, augmentor_utils.py: numpy float32 arrays, the
// rotation through torch-CPU).  Here the batch is already collated and on the device, so the same per-frame operations run as one
// pass over the rows: stage after stage in the configured order, each with the reference's own float32 operations, spelled with
// explicit roundings (__fmul_rn / __fmaf_rn / __fadd_rn) so that no contraction setting can change which rows the range filter keeps
// between the count pass and the place pass.
//
// Memory access: a row is 7 to 15 floats (28 to 60 bytes), never a multiple of 16 bytes that is also aligned, so a thread per row with
// dword accesses would touch every 64-byte sector several times from different instructions.  A workgroup instead copies a tile of
// PCP_AUG_TILE_ROWS whole rows into LDS with 16-byte loads (a tile starts 16-byte aligned: 512 rows x 4 bytes x stride), the lanes
// work on their rows out of LDS, the kept rows are compacted into a second LDS buffer placed at the same offset modulo 16 bytes as
// their destination, and that buffer leaves with 16-byte stores.
#include "pcp_common.h"

namespace {

#include "aug_tile.h"

constexpr int AUG_THREADS = 256;
constexpr int AUG_ITEMS = PCP_AUG_TILE_ROWS / AUG_THREADS;       // rows per thread
constexpr int AUG_WAVES = AUG_THREADS / PCP_WAVE;
constexpr int TS = PCP_AUG_TABLE_STRIDE;
static_assert(PCP_AUG_TILE_ROWS % AUG_THREADS == 0 && (PCP_AUG_TILE_ROWS * 4) % 16 == 0, "a tile starts 16-byte aligned for every stride");
static_assert(2 * (PCP_AUG_TILE_ROWS * PCP_AUG_MAX_ROW_STRIDE + 4) * 4 <= 65536, "both tile buffers fit the LDS of one workgroup");

// atan2(sin v, cos v): how the reference brings lane_dir and the MoDAR heading back into [-pi, pi]
__device__ __forceinline__ float aug_wrap(float v) { return atan2f(sinf(v), cosf(v)); }

// rotate_points_along_z with the host's float32 cos / sin: x' = x c + y (-s), y' = x s + y c
__device__ __forceinline__ void aug_rot(float &x, float &y, float c, float s) {
  const float nx = __fmaf_rn(y, -s, __fmul_rn(x, c));
  const float ny = __fmaf_rn(y, c, __fmul_rn(x, s));
  x = nx;
  y = ny;
}

struct AugRow {
  float x, y, z, lane, head;
};

// one row through every stage.  -> the row lies inside the range (true when the filter is off); rows of a foreign frame: untouched, outside
__device__ __forceinline__ bool aug_row(const float *row, int S, const pcp_world_aug_t &a, const float *__restrict__ table, AugRow &r,
                                        bool &modar) {
  r.x = row[1];
  r.y = row[2];
  r.z = row[3];
  r.lane = a.hd_map ? row[10] : 0.f;
  modar = S >= 14 && row[S - 3] > 0.f;
  r.head = S >= 14 ? row[9] : 0.f;
  const float fb = row[0];
  if (!(fb >= 0.f && fb < (float)a.batch)) return !a.filter;
  const float *t = table + (int)fb * TS;
  for (int k = 0; k < a.n_stages; k++) {
    switch (a.stage[k]) {
      case PCP_AUG_FLIP_X:
        if (t[0] != 0.f) {
          r.y = -r.y;
          r.lane = -r.lane;
          r.head = -r.head;
        }
        break;
      case PCP_AUG_FLIP_Y:
        if (t[1] != 0.f) {
          r.x = -r.x;
          if (a.hd_map) r.lane = aug_wrap(-__fadd_rn(r.lane, AUG_PI));
          if (modar) r.head = aug_wrap(-__fadd_rn(r.head, AUG_PI));
        }
        break;
      case PCP_AUG_ROTATE:
        aug_rot(r.x, r.y, t[2], t[3]);
        if (a.hd_map) r.lane = aug_wrap(__fadd_rn(r.lane, t[4]));
        if (modar) r.head = aug_wrap(__fadd_rn(r.head, t[4]));
        break;
      case PCP_AUG_SCALE:
        r.x = __fmul_rn(r.x, t[5]);
        r.y = __fmul_rn(r.y, t[5]);
        r.z = __fmul_rn(r.z, t[5]);
        break;
      case PCP_AUG_TRANSLATE:
        r.x = __fadd_rn(r.x, t[6]);
        r.y = __fadd_rn(r.y, t[7]);
        r.z = __fadd_rn(r.z, t[8]);
        break;
      default:
        break;
    }
  }
  if (!a.filter) return true;
  return r.x >= a.range[0] && r.x < a.range[3] && r.y >= a.range[1] && r.y < a.range[4] && r.z >= a.range[2] && r.z < a.range[5];
}

// rows of this tile inside the range -> tile_cnt[tile]; per frame -> frame_count (integer adds: the order does not reach the result)
__global__ __launch_bounds__(AUG_THREADS) void k_aug_count(const float *__restrict__ points, long long n, int S, pcp_world_aug_t a,
                                                           const float *__restrict__ table, int *__restrict__ tile_cnt,
                                                           int *__restrict__ frame_count) {
  extern __shared__ f32x4 aug_lds4[];
  float *in = reinterpret_cast<float *>(aug_lds4);
  __shared__ int s_frame[PCP_AUG_MAX_BATCH];
  __shared__ int s_wave[AUG_ITEMS][AUG_WAVES];
  const long long base = (long long)blockIdx.x * PCP_AUG_TILE_ROWS;
  const int rows = (int)((n - base) < PCP_AUG_TILE_ROWS ? (n - base) : PCP_AUG_TILE_ROWS);
  if (threadIdx.x < PCP_AUG_MAX_BATCH) s_frame[threadIdx.x] = 0;
  aug_stage_in<AUG_THREADS>(in, points + base * S, rows * S);
  __syncthreads();
#pragma unroll
  for (int it = 0; it < AUG_ITEMS; it++) {
    const int r = it * AUG_THREADS + threadIdx.x;
    bool keep = false;
    if (r < rows) {
      AugRow v;
      bool modar;
      keep = aug_row(in + r * S, S, a, table, v, modar);
      if (keep && a.filter) atomicAdd(&s_frame[(int)in[r * S]], 1);  // kept with the filter on: the frame index is inside [0, batch)
    }
    aug_tile_rank<AUG_THREADS>(keep, it, s_wave);
  }
  aug_tile_count_finish<AUG_THREADS>(s_wave, s_frame, a.batch, tile_cnt, frame_count);
}

__global__ __launch_bounds__(AUG_THREADS) void k_aug_place(const float *__restrict__ points, long long n, int S, pcp_world_aug_t a,
                                                           const float *__restrict__ table, const int *__restrict__ tile_cnt,
                                                           float *__restrict__ out) {
  extern __shared__ f32x4 aug_lds4[];
  float *in = reinterpret_cast<float *>(aug_lds4);
  float *ob = in + PCP_AUG_TILE_ROWS * S;                            // second buffer (filter on): 4 floats longer than a tile
  __shared__ int s_wave[AUG_ITEMS][AUG_WAVES];
  __shared__ long long s_before[AUG_WAVES];
  const long long base = (long long)blockIdx.x * PCP_AUG_TILE_ROWS;
  const int rows = (int)((n - base) < PCP_AUG_TILE_ROWS ? (n - base) : PCP_AUG_TILE_ROWS);
  aug_stage_in<AUG_THREADS>(in, points + base * S, rows * S);
  const long long before = a.filter ? aug_tile_before<AUG_THREADS>(tile_cnt) : 0;
  __syncthreads();
  bool keep[AUG_ITEMS];
  int rank[AUG_ITEMS];
#pragma unroll
  for (int it = 0; it < AUG_ITEMS; it++) {
    const int r = it * AUG_THREADS + threadIdx.x;
    keep[it] = false;
    if (r < rows) {
      float *row = in + r * S;
      AugRow v;
      bool modar;
      keep[it] = aug_row(row, S, a, table, v, modar);
      row[1] = v.x;
      row[2] = v.y;
      row[3] = v.z;
      if (a.hd_map) row[10] = v.lane;
      if (modar) row[9] = v.head;
    }
    rank[it] = aug_tile_rank<AUG_THREADS>(keep[it], it, s_wave);
  }
  if (!a.filter) {                                                    // same place, same alignment: the tile goes back as it came
    __syncthreads();
    aug_stage_out<AUG_THREADS>(out + base * S, in, 0, rows * S);
    return;
  }
  aug_tile_compact<AUG_THREADS>(before, keep, rank, in, ob, S, s_wave, s_before, out);
}

// one thread per box (k == 0) or per instance matrix (k >= 1) of object (b, m)
__global__ __launch_bounds__(256) void k_aug_boxes(pcp_world_aug_t a, const float *__restrict__ table, float *__restrict__ gt, int max_boxes,
                                                   int W, float *__restrict__ tf, int n_sweeps, int tf_rows) {
  const int per = 1 + (tf ? n_sweeps : 0);
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)a.batch * max_boxes * per) return;
  const int k = (int)(idx % per);
  const long long obj = idx / per;
  const int b = (int)(obj / max_boxes);
  float *box = gt + obj * W;
  if (box[W - 1] == 0.f) return;                                      // padding: the box and its matrices keep their bits
  const float *t = table + b * TS;
  if (k == 0) {
    float x = box[0], y = box[1], z = box[2], dx = box[3], dy = box[4], dz = box[5], h = box[6];
    float vx = W == 10 ? box[7] : 0.f, vy = W == 10 ? box[8] : 0.f;
    for (int s = 0; s < a.n_stages; s++) {
      switch (a.stage[s]) {
        case PCP_AUG_FLIP_X:
          if (t[0] != 0.f) {
            y = -y;
            h = -h;
            vy = -vy;
          }
          break;
        case PCP_AUG_FLIP_Y:
          if (t[1] != 0.f) {
            x = -x;
            h = -__fadd_rn(h, AUG_PI);
            vx = -vx;
          }
          break;
        case PCP_AUG_ROTATE:
          aug_rot(x, y, t[2], t[3]);
          h = __fadd_rn(h, t[4]);
          aug_rot(vx, vy, t[2], t[3]);
          break;
        case PCP_AUG_SCALE:
          x = __fmul_rn(x, t[5]);
          y = __fmul_rn(y, t[5]);
          z = __fmul_rn(z, t[5]);
          dx = __fmul_rn(dx, t[5]);
          dy = __fmul_rn(dy, t[5]);
          dz = __fmul_rn(dz, t[5]);
          vx = __fmul_rn(vx, t[5]);
          vy = __fmul_rn(vy, t[5]);
          break;
        case PCP_AUG_TRANSLATE:
          x = __fadd_rn(x, t[6]);
          y = __fadd_rn(y, t[7]);
          z = __fadd_rn(z, t[8]);
          break;
        default:
          break;
      }
    }
    if (!a.raw_heading) h = aug_limit_period(h);
    box[0] = x;
    box[1] = y;
    box[2] = z;
    box[3] = dx;
    box[4] = dy;
    box[5] = dz;
    box[6] = h;
    if (W == 10) {
      box[7] = vx;
      box[8] = vy;
    }
    return;
  }
  // A = [R | p] -> T A T^-1, stage by stage
  float *m = tf + (obj * n_sweeps + (k - 1)) * (long long)(tf_rows * 4);
  float R[3][3], p[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) R[i][j] = m[i * 4 + j];
    p[i] = m[i * 4 + 3];
  }
  for (int s = 0; s < a.n_stages; s++) {
    const int st = a.stage[s];
    if ((st == PCP_AUG_FLIP_X && t[0] != 0.f) || (st == PCP_AUG_FLIP_Y && t[1] != 0.f)) {
      const int ax = st == PCP_AUG_FLIP_X ? 1 : 0;                     // D A D with D = diag(.., -1 at ax, ..): sign changes only
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
          if ((i == ax) != (j == ax)) R[i][j] = -R[i][j];
#pragma unroll
      for (int i = 0; i < 3; i++)
        if (i == ax) p[i] = -p[i];
    } else if (st == PCP_AUG_ROTATE) {                                 // Rz R Rz^T | Rz p
      const float c = t[2], sn = t[3];
#pragma unroll
      for (int j = 0; j < 3; j++) aug_rot(R[0][j], R[1][j], c, sn);    // rows 0, 1 of Rz R
#pragma unroll
      for (int i = 0; i < 3; i++) aug_rot(R[i][0], R[i][1], c, sn);    // (M Rz^T)[i][0] = M[i][0] c - M[i][1] s, [i][1] = M[i][0] s + M[i][1] c
      aug_rot(p[0], p[1], c, sn);
    } else if (st == PCP_AUG_SCALE) {                                  // s R (1 / s) = R | s p
#pragma unroll
      for (int i = 0; i < 3; i++) p[i] = __fmul_rn(p[i], t[5]);
    } else if (st == PCP_AUG_TRANSLATE) {                              // x -> R (x - d) + p + d: p + d - R d
      const float d[3] = {t[6], t[7], t[8]};
#pragma unroll
      for (int i = 0; i < 3; i++) {
        const float rd = __fmaf_rn(R[i][2], d[2], __fmaf_rn(R[i][1], d[1], __fmul_rn(R[i][0], d[0])));
        p[i] = __fadd_rn(p[i], __fsub_rn(d[i], rd));
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) m[i * 4 + j] = R[i][j];
    m[i * 4 + 3] = p[i];
  }
}

bool aug_ok(const pcp_world_aug_t *a) {
  if (!a || a->n_stages < 0 || a->n_stages > PCP_AUG_MAX_STAGES || a->batch <= 0 || a->batch > PCP_AUG_MAX_BATCH) return false;
  for (int k = 0; k < a->n_stages; k++)
    if (a->stage[k] < PCP_AUG_FLIP_X || a->stage[k] > PCP_AUG_TRANSLATE) return false;
  return true;
}

}  // namespace

extern "C" size_t pcp_world_augment_points_workspace_bytes(int64_t n) {
  return aug_points_workspace_bytes(n);
}

extern "C" int pcp_world_augment_points(const pcp_world_aug_t *aug, const float *table, const float *points, int64_t n, int32_t row_stride,
                                        float *out, int32_t *frame_count, void *workspace, size_t workspace_bytes, void *stream_) {
  if (!aug_ok(aug) || !table || (aug->hd_map && row_stride != 13)) return PCP_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  int st = aug_points_shape(n, row_stride);
  if (st == PCP_OK) st = aug_points_buffers(points, n, out, aug->filter != 0, aug->batch, frame_count, workspace, workspace_bytes, stream);
  if (st != PCP_OK || n == 0) return st;
  const int tiles = (int)((n + PCP_AUG_TILE_ROWS - 1) / PCP_AUG_TILE_ROWS);
  const size_t tile_bytes = (size_t)PCP_AUG_TILE_ROWS * row_stride * 4;
  if (aug->filter) {
    hipLaunchKernelGGL(k_aug_count, dim3(tiles), dim3(AUG_THREADS), tile_bytes, stream, points, (long long)n, (int)row_stride, *aug, table,
                       (int *)workspace, (int *)frame_count);
    PCP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_aug_place, dim3(tiles), dim3(AUG_THREADS), aug->filter ? 2 * tile_bytes + 16 : tile_bytes, stream, points, (long long)n,
                     (int)row_stride, *aug, table, (const int *)workspace, out);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_world_augment_boxes(const pcp_world_aug_t *aug, const float *table, float *gt_boxes, int32_t max_boxes, int32_t box_width,
                                       float *instances_tf, int32_t n_sweeps, int32_t tf_rows, void *stream_) {
  if (!aug_ok(aug) || !table || max_boxes < 0 || (box_width != 8 && box_width != 10)) return PCP_ERR_ARG;
  if (instances_tf && (n_sweeps <= 0 || (tf_rows != 3 && tf_rows != 4))) return PCP_ERR_ARG;
  if (max_boxes == 0) return PCP_OK;
  if (!gt_boxes) return PCP_ERR_ARG;
  const long long total = (long long)aug->batch * max_boxes * (1 + (instances_tf ? n_sweeps : 0));
  if (total >= (1LL << 31)) return PCP_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_aug_boxes, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, *aug, table, gt_boxes,
                     (int)max_boxes, (int)box_width, instances_tf, (int)n_sweeps, (int)tf_rows);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}
