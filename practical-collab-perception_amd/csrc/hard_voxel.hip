// Hard voxelisation (spconv's CPU point-to-voxel generator, pillar case nz == 1) and the one-layer PillarVFE of the classic PointPillar front end.
//
// Reference behaviour: pcdet/datasets/processor/data_processor.py:116-144 (transform_points_to_voxels: VoxelGeneratorWrapper over spconv's
// CPU generator, MAX_POINTS_PER_VOXEL = T, MAX_NUMBER_OF_VOXELS = max_voxels) and pcdet/models/backbones_3d/vfe/pillar_vfe.py.  Per frame, for
// the points in input order:
//     c = floor((p - range_min) / voxel)   (float32 subtract, IEEE divide), skipped unless 0 <= c < grid on x, y AND z
//     a cell not seen before becomes voxel nvox++ unless nvox == max_voxels (then the point is skipped, later points go on)
//     the point takes the next slot of its voxel unless the voxel already holds T points
// so voxels are numbered by FIRST APPEARANCE and slots by input order.  No step here depends on the arrival order of an atomic:
//   k_cells_z      (csrc/vox_front.h, shared with the mean VFE) cell id per row (z range too), integer histogram, frame column validated        (the only atomics: integer adds)
//   pcp_voxelize_cells_ready + pcp_voxelize_sort_pillar_rows (csrc/voxelize.hip, called, not changed; the sort itself is csrc/vox_front.h's):
//                  rows grouped by cell, every cell's rows in ascending row index -- the first entry of a run is the cell's first point,
//                  entry j its slot-j point; a cell of thousands of rows is ranked by a whole workgroup there
//   k_hv_flags     flag "first point of its cell" per row; flags per 1024-row tile and per frame
//   k_hv_number    exclusive prefix of the flags in row order = first-appearance rank; minus the frame's start = rank inside the frame;
//                  kept if < max_voxels; voxel number = kept voxels of the frames in front + rank.  Writes coords, num_points, counters
//                  (both on csrc/vox_front.h's tile-sum and tile-prefix helpers and its 1024-row tile)
//   k_hv_gather    (after the host read M) one thread per (voxel, slot): the row of slot j < min(count, T), zeros behind
#include "vox_front.h"

namespace {

constexpr int HV_MAX_B = PCP_HARD_VOXEL_MAX_BATCH;   // 64: one wave scans the per-frame counts

// counters (int32, PCP_HARD_VOXEL_COUNTERS of them): [0] M, [1] error word, [4 .. 4 + 64) voxels kept per frame, [68 .. 68 + 64) cells hit per frame
constexpr int HV_CNT_M = 0, HV_CNT_ERR = 1, HV_CNT_FRAME = 4, HV_CNT_FIRST = 4 + HV_MAX_B;

struct HvLayout {
  VoxLayout v;             // the pillariser's workspace in front, laid out as pcp_voxelize lays it out
  size_t tile_sums;        // int32 [n_tiles + 1]
  size_t vox_pillar;       // int32 [n]       voxel number -> pillar rank of the pillariser (cell order)
  size_t dense_coords;     // int32 [n][4]    pcp_voxelize_cells_ready insists on writing its own coordinates
  size_t total;
};
inline HvLayout hv_layout(int64_t cells, int64_t n) {
  HvLayout L;
  PcpCarver ws = pcp_behind_vox_layout(cells, n, &L.v);
  L.tile_sums = ws.take((size_t)((n + SCAN_TILE - 1) / SCAN_TILE + 1) * 4);
  L.vox_pillar = ws.take((size_t)n * 4);
  L.dense_coords = ws.take((size_t)n * 16);
  L.total = ws.total();
  return L;
}

// is row r the first point of its cell?  The cell's run in the sorted bucket order starts with its smallest row index.
__device__ __forceinline__ bool hv_is_first(long long r, long long n, const int *__restrict__ point_cell, const int2 *__restrict__ cell_rs,
                                            const int *__restrict__ bucket_order, int *cell_out) {
  *cell_out = -1;
  if (r >= n) return false;
  const int c = point_cell[r];
  if (c < 0) return false;
  *cell_out = c;
  return bucket_order[cell_rs[c].y] == (int)r;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_hv_flags(long long n, int plane, const int *__restrict__ point_cell,
                                                         const int2 *__restrict__ cell_rs, const int *__restrict__ bucket_order,
                                                         int *__restrict__ tile_sums, int *__restrict__ counters) {
  __shared__ int s_frame[HV_MAX_B];
  __shared__ int wave_tot[SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < HV_MAX_B) s_frame[threadIdx.x] = 0;
  __syncthreads();
  const long long base = (long long)blockIdx.x * SCAN_TILE;
  int total = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    int c;
    const bool first = hv_is_first(base + i * SCAN_THREADS + threadIdx.x, n, point_cell, cell_rs, bucket_order, &c);
    const int b = first ? c / plane : -1;
    // frames are grouped, so a wave's flagged rows share one or two frames: one LDS add per (wave, frame)
    unsigned long long todo = __ballot(first);
    total += __popcll(todo);
    while (todo) {
      const int lead = __ffsll((long long)todo) - 1;
      const int bl = __shfl(b, lead, 64);
      const unsigned long long same = __ballot(b == bl);
      if (lane == lead) atomicAdd(&s_frame[bl], __popcll(same));
      todo &= ~same;
    }
  }
  tile_sum_store(total, wave_tot, tile_sums);         // `total` is already the wave's count (ballots)
  if (threadIdx.x < HV_MAX_B && s_frame[threadIdx.x]) atomicAdd(&counters[HV_CNT_FIRST + threadIdx.x], s_frame[threadIdx.x]);
}

__global__ __launch_bounds__(SCAN_THREADS) void k_hv_number(long long n, pcp_grid_t g, int T, int max_voxels, int n_tiles,
                                                          const int *__restrict__ point_cell, const int2 *__restrict__ cell_rs,
                                                          const int *__restrict__ bucket_order, const int *__restrict__ cell_count,
                                                          const int *__restrict__ tile_sums, int *__restrict__ counters,
                                                          int *__restrict__ vox_pillar, int *__restrict__ voxel_coords,
                                                          int *__restrict__ voxel_num_points) {
  __shared__ int s_first0[HV_MAX_B], s_vox0[HV_MAX_B];      // per frame: first-appearance rank of its first cell, number of its first voxel
  __shared__ int red[SCAN_THREADS / 64], lds_wave[SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile = blockIdx.x;
  if (wave == 0) {
    const int hit = lane < g.batch_size ? counters[HV_CNT_FIRST + lane] : 0;
    const int kept = min(hit, max_voxels);
    int ih = hit, ik = kept;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                                   // a pair in one loop: two wave_incl_scan calls change the schedule
      const int uh = __shfl_up(ih, d, 64), uk = __shfl_up(ik, d, 64);
      if (lane >= d) {
        ih += uh;
        ik += uk;
      }
    }
    s_first0[lane] = ih - hit;
    s_vox0[lane] = ik - kept;
    if (tile == 0) {
      counters[HV_CNT_FRAME + lane] = kept;
      if (lane == 63) counters[HV_CNT_M] = ik;
    }
  }
  tiles_in_front(tile_sums, min(tile, n_tiles), red);
  // exclusive scan of this tile's flags; a thread's items are CONSECUTIVE rows
  const long long base = (long long)tile * SCAN_TILE + (long long)threadIdx.x * SCAN_ITEMS;
  int cell[SCAN_ITEMS], excl[SCAN_ITEMS], local = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    const bool first = hv_is_first(base + i, n, point_cell, cell_rs, bucket_order, &cell[i]);
    if (!first) cell[i] = -1;
    excl[i] = local;
    local += first ? 1 : 0;
  }
  const int before = tile_prefix_before<true>(local, red, lds_wave);
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; i++) {
    const int c = cell[i];
    if (c < 0) continue;
    const CellCoords at = cell_coords(c, g);
    const int in_frame = before + excl[i] - s_first0[at.b];
    if (in_frame >= max_voxels) continue;                        // the frame is full: this cell never becomes a voxel
    const int v = s_vox0[at.b] + in_frame;
    vox_pillar[v] = cell_rs[c].x;
    *reinterpret_cast<int4 *>(voxel_coords + 4LL * v) = make_int4(at.b, 0, at.cy, at.cx);       // [b, z, y, x]
    voxel_num_points[v] = min(cell_count[c], T);
  }
}

// one thread per (voxel, slot): C floats
template <bool VEC4>
__global__ __launch_bounds__(SCAN_THREADS) void k_hv_gather(const float *__restrict__ points, int stride, int C, int T, long long slots,
                                                          const int *__restrict__ vox_pillar, const int *__restrict__ pillar_start,
                                                          const int *__restrict__ bucket_order, const int *__restrict__ voxel_num_points,
                                                          float *__restrict__ voxels) {
  const long long s = (long long)blockIdx.x * SCAN_THREADS + threadIdx.x;
  if (s >= slots) return;
  const long long v = s / T;
  const int j = (int)(s - v * T);
  float *dst = voxels + s * C;
  const float *src = nullptr;
  if (j < voxel_num_points[v]) src = points + (long long)bucket_order[pillar_start[vox_pillar[v]] + j] * stride + 1;
  if (VEC4) {
    for (int c = 0; c < C; c += 4)
      *reinterpret_cast<f32x4 *>(dst + c) = src ? f32x4{src[c], src[c + 1], src[c + 2], src[c + 3]} : f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    for (int c = 0; c < C; c++) dst[c] = src ? src[c] : 0.f;
  }
}

// the checks behind pcp_front_args' PCP_ERR_ARG ones
inline bool hv_args_ok(const pcp_grid_t *grid, int64_t n, int32_t row_stride, int32_t nz, int32_t T, int64_t max_voxels) {
  if (row_stride < 4) return false;
  if (nz != 1 || T < 1 || T > PCP_HARD_VOXEL_MAX_T || max_voxels < 1 || grid->batch_size > HV_MAX_B) return false;
  return true;
}

}  // namespace

extern "C" size_t pcp_hard_voxelize_workspace_bytes(const pcp_grid_t *grid, int64_t max_points) {
  if (!grid || max_points < 0 || grid->nx <= 0 || grid->ny <= 0 || grid->batch_size <= 0) return 0;
  return hv_layout((int64_t)grid->batch_size * grid->nx * grid->ny, max_points > 0 ? max_points : 1).total;
}

extern "C" int pcp_hard_voxelize(const float *points, int64_t n, int32_t row_stride, const pcp_grid_t *grid, int32_t nz, int32_t max_points,
                                 int64_t max_voxels, void *workspace, size_t workspace_bytes, int32_t *voxel_coords,
                                 int32_t *voxel_num_points, int32_t *counters, void *stream_) {
  int64_t cells;
  const int front = pcp_front_args(grid, n, &cells);
  if (front == PCP_ERR_ARG || !hv_args_ok(grid, n, row_stride, nz, max_points, max_voxels)) return PCP_ERR_ARG;
  if (!workspace || !voxel_coords || !voxel_num_points || !counters || (n > 0 && !points)) return PCP_ERR_ARG;
  if ((((uintptr_t)voxel_coords) & 15) || (((uintptr_t)counters) & 15)) return PCP_ERR_ARG;
  if (front != PCP_OK) return front;
  const int64_t n_alloc = n > 0 ? n : 1;
  const HvLayout L = hv_layout(cells, n_alloc);
  if (workspace_bytes < L.total) return PCP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char *ws = (char *)workspace;
  int *cell_count = (int *)(ws + L.v.cell_count);
  int *point_cell = (int *)(ws + L.v.point_cell);
  int *point_rank = (int *)(ws + L.v.point_rank);
  const int *bucket_order = (const int *)(ws + L.v.bucket_order);
  const int2 *cell_rs = (const int2 *)(ws + L.v.cell_rs);
  int *tile_sums = (int *)(ws + L.tile_sums);
  const int n_tiles = (int)((n + SCAN_TILE - 1) / SCAN_TILE);
  const int mv = (int)(max_voxels > 0x7fffffffLL ? 0x7fffffffLL : max_voxels);

  if (pcp_zero_async(cell_count, (size_t)cells * 4, stream) != PCP_OK) return PCP_ERR_LAUNCH;
  if (pcp_zero_async(counters, (size_t)PCP_HARD_VOXEL_COUNTERS * 4, stream) != PCP_OK) return PCP_ERR_LAUNCH;
  if (n_tiles > 0) {
    hipLaunchKernelGGL(k_cells_z<false>, dim3(n_tiles), dim3(SCAN_THREADS), 0, stream, points, (long long)n, (int)row_stride, *grid, (int)nz, cell_count,
                       point_cell, point_rank, (int *)nullptr, counters + HV_CNT_ERR);
    PCP_CHECK_LAUNCH();
  }
  // cells -> pillars in cell order, rows grouped by pillar; then every pillar's rows in ascending row index
  int st = pcp_voxelize_cells_ready(points, n, row_stride, grid, workspace, L.v.total, (int32_t *)(ws + L.dense_coords), nullptr, nullptr, stream_);
  if (st != PCP_OK) return st;
  st = pcp_voxelize_sort_pillar_rows(grid, workspace, n, stream_);
  if (st != PCP_OK) return st;
  if (n_tiles > 0) {
    hipLaunchKernelGGL(k_hv_flags, dim3(n_tiles), dim3(SCAN_THREADS), 0, stream, (long long)n, grid->nx * grid->ny, point_cell, cell_rs, bucket_order,
                       tile_sums, counters);
    PCP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_hv_number, dim3(n_tiles > 0 ? n_tiles : 1), dim3(SCAN_THREADS), 0, stream, (long long)n, *grid, (int)max_points, mv, n_tiles,
                     point_cell, cell_rs, bucket_order, cell_count, tile_sums, counters, (int *)(ws + L.vox_pillar), voxel_coords,
                     voxel_num_points);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_hard_voxelize_gather(const float *points, int64_t n, int32_t row_stride, int32_t num_features, const pcp_grid_t *grid,
                                        int32_t max_points, const void *workspace, size_t workspace_bytes, int64_t num_voxels,
                                        const int32_t *voxel_num_points, float *voxels, void *stream_) {
  int64_t cells;
  const int front = pcp_front_args(grid, n, &cells);
  if (front == PCP_ERR_ARG || !hv_args_ok(grid, n, row_stride, 1, max_points, 1)) return PCP_ERR_ARG;
  if (num_features < PCP_HARD_VOXEL_MIN_FEATURES || num_features > PCP_HARD_VOXEL_MAX_FEATURES || row_stride < 1 + num_features) return PCP_ERR_ARG;
  if (num_voxels < 0 || num_voxels > n) return PCP_ERR_ARG;
  if (num_voxels == 0) return PCP_OK;
  if (!points || !workspace || !voxel_num_points || !voxels) return PCP_ERR_ARG;
  if (front != PCP_OK) return front;
  const HvLayout L = hv_layout(cells, n);
  if (workspace_bytes < L.total) return PCP_ERR_WORKSPACE;
  const char *ws = (const char *)workspace;
  const long long slots = (long long)num_voxels * max_points;
  const long long blocks = (slots + SCAN_THREADS - 1) / SCAN_THREADS;
  if (blocks >= (1LL << 31)) return PCP_ERR_UNSUPPORTED;
  const bool vec4 = (num_features % 4 == 0) && ((((uintptr_t)voxels) & 15) == 0);
#define PCP_HV_GATHER(V_)                                                                                                                     \
  hipLaunchKernelGGL(k_hv_gather<V_>, dim3((unsigned)blocks), dim3(SCAN_THREADS), 0, (hipStream_t)stream_, points, (int)row_stride,             \
                     (int)num_features, (int)max_points, slots, (const int *)(ws + L.vox_pillar), (const int *)(ws + L.v.pillar_start),      \
                     (const int *)(ws + L.v.bucket_order), voxel_num_points, voxels)
  if (vec4) PCP_HV_GATHER(true); else PCP_HV_GATHER(false);
#undef PCP_HV_GATHER
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

// ---- PillarVFE, one PFN layer (pillar_vfe.py:94-123) -------------------------------------------------------------------------------------------
// Per pillar: mean of xyz = sum over slots / n; feature row = [raw (all, or columns 3.. without USE_ABSLOTE_XYZ), xyz - mean, xyz - centre,
// |xyz| with WITH_DISTANCE], masked rows are zero; Linear (+ folded BatchNorm) + ReLU; max over ALL T slots.  A masked row contributes
// ReLU(bias) whatever the pillar holds, so the kernel walks the n real rows only and adds that one candidate when n < T.
// Mapping: a wave per pillar (a workgroup of four waves takes four pillars per step, grid-stride).  Lane r builds the feature row of slot r
// into the wave's LDS rows; then lane c keeps output channel c (and c + 64) with its K <= 24 weights in registers and walks the rows,
// every row read as 16-byte LDS broadcasts.
namespace {

struct VfeGeom { float voxel_x, voxel_y, voxel_z, off_x, off_y, off_z; };

template <int KP4, int NCH>
__global__ __launch_bounds__(256) void k_pillar_vfe(const float *__restrict__ voxels, const int *__restrict__ num_points,
                                                    const int *__restrict__ coords, long long M, int T, int C, int K, unsigned flags,
                                                    VfeGeom g, const float *__restrict__ w, const float *__restrict__ bias, int out,
                                                    float *__restrict__ pillar_features) {
  extern __shared__ f32x4 s_feat[];                         // [4 waves][T][KP4]
  constexpr int KP = KP4 * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float *feat = reinterpret_cast<float *>(s_feat + (size_t)wave * T * KP4);
  float wr[NCH][KP], br[NCH];
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    const int ch = lane + 64 * h;
#pragma unroll
    for (int k = 0; k < KP; k++) wr[h][k] = (ch < out && k < K) ? w[(long long)ch * K + k] : 0.f;
    br[h] = ch < out ? bias[ch] : 0.f;
  }
  const bool with_distance = (flags & PCP_PFN_WITH_DISTANCE) != 0;
  const int raw0 = (flags & PCP_PFN_ABSOLUTE_XYZ) ? 0 : 3;
  for (long long m0 = (long long)blockIdx.x * 4; m0 < M; m0 += (long long)gridDim.x * 4) {
    const long long m = m0 + wave;
    const bool live = m < M;
    const int n = live ? min(max(num_points[m], 0), T) : 0;
    const float *vrow = voxels + (live ? m : 0) * (long long)T * C;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int r = lane; r < n; r += 64) {
      sx += vrow[r * C];
      sy += vrow[r * C + 1];
      sz += vrow[r * C + 2];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {                                  // a triple in one loop: three wave_sum calls change the schedule
      sx += __shfl_xor(sx, d, 64);
      sy += __shfl_xor(sy, d, 64);
      sz += __shfl_xor(sz, d, 64);
    }
    const float fn = (float)n;
    const float mx = __fdiv_rn(sx, fn), my = __fdiv_rn(sy, fn), mz = __fdiv_rn(sz, fn);
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (live) {
      const int4 cd = *reinterpret_cast<const int4 *>(coords + 4 * m);              // [b, z, y, x]
      // coords * voxel + offset with both roundings, as the reference's two tensor ops
      ox = __fadd_rn(__fmul_rn((float)cd.w, g.voxel_x), g.off_x);
      oy = __fadd_rn(__fmul_rn((float)cd.z, g.voxel_y), g.off_y);
      oz = __fadd_rn(__fmul_rn((float)cd.y, g.voxel_z), g.off_z);
    }
    for (int r = lane; r < n; r += 64) {
      const float *p = vrow + r * C;
      float *f = feat + r * KP;
      const float x = p[0], y = p[1], z = p[2];
      int k = 0;
      for (int c = raw0; c < C; c++) f[k++] = p[c];
      f[k++] = __fsub_rn(x, mx);
      f[k++] = __fsub_rn(y, my);
      f[k++] = __fsub_rn(z, mz);
      f[k++] = __fsub_rn(x, ox);
      f[k++] = __fsub_rn(y, oy);
      f[k++] = __fsub_rn(z, oz);
      if (with_distance) f[k++] = sqrtf(x * x + y * y + z * z);
      for (; k < KP; k++) f[k] = 0.f;
    }
    __syncthreads();
    float acc[NCH];
#pragma unroll
    for (int h = 0; h < NCH; h++) acc[h] = (n < T) ? br[h] : -INFINITY;       // the zero rows of a pillar that is not full
    const f32x4 *rows = reinterpret_cast<const f32x4 *>(feat);
    for (int r = 0; r < n; r++) {
      float y[NCH];
#pragma unroll
      for (int h = 0; h < NCH; h++) y[h] = br[h];
#pragma unroll
      for (int q = 0; q < KP4; q++) {
        const f32x4 f = rows[r * KP4 + q];
#pragma unroll
        for (int h = 0; h < NCH; h++) {
          y[h] = fmaf(wr[h][4 * q], f.x, y[h]);
          y[h] = fmaf(wr[h][4 * q + 1], f.y, y[h]);
          y[h] = fmaf(wr[h][4 * q + 2], f.z, y[h]);
          y[h] = fmaf(wr[h][4 * q + 3], f.w, y[h]);
        }
      }
#pragma unroll
      for (int h = 0; h < NCH; h++) acc[h] = fmaxf(acc[h], y[h]);
    }
#pragma unroll
    for (int h = 0; h < NCH; h++) {
      const int ch = lane + 64 * h;
      if (live && ch < out) pillar_features[m * out + ch] = fmaxf(acc[h], 0.f);
    }
    __syncthreads();
  }
}

template <int KP4>
int vfe_launch(int nch, dim3 grid, size_t lds, hipStream_t stream, const float *voxels, const int *num_points, const int *coords, long long M, int T,
               int C, int K, unsigned flags, VfeGeom g, const float *w, const float *bias, int out, float *pf) {
  if (nch == 1)
    hipLaunchKernelGGL((k_pillar_vfe<KP4, 1>), grid, dim3(256), lds, stream, voxels, num_points, coords, M, T, C, K, flags, g, w, bias, out, pf);
  else
    hipLaunchKernelGGL((k_pillar_vfe<KP4, 2>), grid, dim3(256), lds, stream, voxels, num_points, coords, M, T, C, K, flags, g, w, bias, out, pf);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

}  // namespace

extern "C" int pcp_pillar_vfe(const float *voxels, const int32_t *voxel_num_points, const int32_t *voxel_coords, int64_t num_voxels,
                              int32_t max_points, int32_t num_features, uint32_t flags, const float *voxel_size3, const float *offset3,
                              const float *w, const float *b, int32_t out_channels, float *pillar_features, void *stream_) {
  if (num_voxels < 0 || max_points < 1 || max_points > PCP_HARD_VOXEL_MAX_T || num_features < PCP_HARD_VOXEL_MIN_FEATURES ||
      num_features > PCP_HARD_VOXEL_MAX_FEATURES || (flags & ~(PCP_PFN_ABSOLUTE_XYZ | PCP_PFN_WITH_DISTANCE)) || !voxel_size3 || !offset3)
    return PCP_ERR_ARG;
  if (out_channels < 16 || out_channels > PCP_PILLAR_VFE_MAX_OUT || out_channels % 16) return PCP_ERR_UNSUPPORTED;
  if (num_voxels == 0) return PCP_OK;
  if (!voxels || !voxel_num_points || !voxel_coords || !w || !b || !pillar_features || (((uintptr_t)voxel_coords) & 15)) return PCP_ERR_ARG;
  const int K = ((flags & PCP_PFN_ABSOLUTE_XYZ) ? num_features : num_features - 3) + 6 + ((flags & PCP_PFN_WITH_DISTANCE) ? 1 : 0);
  const int kp4 = (K + 3) / 4;                                    // K in 6 .. 23: 2 .. 6 quads
  const int nch = out_channels > 64 ? 2 : 1;
  long long blocks = (num_voxels + 3) / 4;
  const long long cap = (long long)pcp_current_device_cus() * 8;
  if (blocks > cap) blocks = cap;
  const size_t lds = (size_t)4 * max_points * kp4 * 16;            // at most 4 * 128 * 6 * 16 = 48 KiB
  const VfeGeom g{voxel_size3[0], voxel_size3[1], voxel_size3[2], offset3[0], offset3[1], offset3[2]};
#define PCP_VFE(Q_)                                                                                                                            \
  case Q_:                                                                                                                                     \
    return vfe_launch<Q_>(nch, dim3((unsigned)blocks), lds, (hipStream_t)stream_, voxels, voxel_num_points, voxel_coords, (long long)num_voxels, \
                          (int)max_points, (int)num_features, K, flags, g, w, b, (int)out_channels, pillar_features)
  switch (kp4) {
    PCP_VFE(2);
    PCP_VFE(3);
    PCP_VFE(4);
    PCP_VFE(5);
    PCP_VFE(6);
  }
#undef PCP_VFE
  return PCP_ERR_UNSUPPORTED;
}
