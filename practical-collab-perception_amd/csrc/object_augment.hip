// Per-object augmentation of a collated training batch on the device (include/pcp_hip_train.h: pcp_object_augment_* / pcp_frame_extent).
//
// The reference (augmentor_utils.py random_local_translation_along_* / local_scaling / local_rotation / local_frustum_dropout_* /
// global_frustum_dropout_*) walks the boxes of a sample in order: box i masks the points inside it as it is before its own change, moves
// or removes them, then changes itself; later boxes see the moved points.  A box never reads another box, so k_obj_boxes runs every box
// through the sub-stages on its own and records what the point side needs in front of each sub-stage.  A point then walks sub-stages x
// boxes against those records; points do not depend on each other.  Every operation is the reference's float32 operation with an explicit
// rounding, so the count pass and the place pass agree on which rows a dropout removes.
//
// Memory access is that of augment.hip: tiles of PCP_AUG_TILE_ROWS whole rows through LDS with 16-byte loads and stores, survivors
// compacted into a second LDS buffer at the destination's offset modulo 16 bytes.  The box records of one (frame, sub-stage) are staged in
// LDS PCP_OBJ_LDS_BOXES at a time next to the two tiles: 2 x (512 x 15 + 4) x 4 + 64 x 48 + 332 bytes stay under 64 KB at the widest row.
//
// Cost (tools/bench_augment.py --object, MI355X): the box tests, not the memory traffic: 260 000 rows x 5 sub-stages x 40 boxes take 154 us
// (81 GB/s of row traffic); a list with a dropout walks twice (count, place).
#include "pcp_common.h"

namespace {

#include "aug_tile.h"

constexpr int OBJ_THREADS = 256;
constexpr int OBJ_ITEMS = PCP_AUG_TILE_ROWS / OBJ_THREADS;
constexpr int OBJ_WAVES = OBJ_THREADS / PCP_WAVE;
constexpr int SS = PCP_OBJ_STATE_STRIDE;
constexpr int PS = PCP_OBJ_PARAM_STRIDE;
static_assert(PCP_AUG_TILE_ROWS % OBJ_THREADS == 0, "whole items per thread");
// what k_obj_points declares next to the two dynamic tile buffers: the staged box records, s_mask, s_frame, s_wave, s_before
constexpr int OBJ_STATIC_LDS = PCP_OBJ_LDS_BOXES * SS * 4 + 8 + (PCP_AUG_MAX_BATCH + 1) * 4 + OBJ_ITEMS * OBJ_WAVES * 4 + OBJ_WAVES * 8;
static_assert(2 * (PCP_AUG_TILE_ROWS * PCP_AUG_MAX_ROW_STRIDE + 4) * 4 + OBJ_STATIC_LDS + 16 <= 65536,
              "both tile buffers, the staged box records and the small arrays (16 bytes of alignment slack) fit the LDS of one workgroup");
static_assert(SS % 4 == 0, "a box record is whole 16-byte words");
static_assert(PCP_AUG_MAX_BATCH <= 64, "the frames of a tile are one 64-bit mask");

constexpr float OBJ_MARGIN = 0.1f;                               // get_points_in_box MARGIN, as float32

__device__ __forceinline__ bool obj_is_drop(int st) { return st >= PCP_OBJ_DROP_TOP; }
__device__ __forceinline__ bool obj_is_world(int st) { return st >= PCP_OBJ_WORLD_DROP_TOP; }

struct ObjRow {
  float x, y, z;
  int frame;                                                     // -1: no row, or a frame outside [0, batch)
  bool dead;
};

// one box record against one row: get_points_in_box, then the sub-stage's change
__device__ __forceinline__ void obj_apply(int st, const float *s, ObjRow &r) {
  const float sx = __fsub_rn(r.x, s[0]), sy = __fsub_rn(r.y, s[1]), sz = __fsub_rn(r.z, s[2]);
  const float lx = __fadd_rn(__fmul_rn(sx, s[6]), __fmul_rn(sy, -s[7]));
  const float ly = __fadd_rn(__fmul_rn(sx, s[7]), __fmul_rn(sy, s[6]));
  if (!(fabsf(sz) <= s[5] && fabsf(lx) <= s[3] && fabsf(ly) <= s[4])) return;
  switch (st) {
    case PCP_OBJ_TRANSLATE_X: r.x = __fadd_rn(r.x, s[8]); break;
    case PCP_OBJ_TRANSLATE_Y: r.y = __fadd_rn(r.y, s[8]); break;
    case PCP_OBJ_TRANSLATE_Z: r.z = __fadd_rn(r.z, s[8]); break;
    case PCP_OBJ_SCALE:
      r.x = __fadd_rn(__fmul_rn(sx, s[8]), s[0]);
      r.y = __fadd_rn(__fmul_rn(sy, s[8]), s[1]);
      r.z = __fadd_rn(__fmul_rn(sz, s[8]), s[2]);
      break;
    case PCP_OBJ_ROTATE:                                         // rotate_points_along_z: x' = x c + y (-s), y' = x s + y c, z' = z
      r.x = __fadd_rn(__fmaf_rn(sy, -s[9], __fmul_rn(sx, s[8])), s[0]);
      r.y = __fadd_rn(__fmaf_rn(sy, s[8], __fmul_rn(sx, s[9])), s[1]);
      r.z = __fadd_rn(sz, s[2]);
      break;
    case PCP_OBJ_DROP_TOP: r.dead = r.z >= s[8]; break;
    case PCP_OBJ_DROP_BOTTOM: r.dead = r.z <= s[8]; break;
    case PCP_OBJ_DROP_LEFT: r.dead = r.y >= s[8]; break;
    case PCP_OBJ_DROP_RIGHT: r.dead = r.y <= s[8]; break;
    default: break;
  }
}

// the rows of this thread through every sub-stage.  Every loop bound is the same for the whole workgroup (the frame mask, the stage list,
// the box count of a frame), so the barriers inside are reached by all threads.
__device__ __forceinline__ void obj_walk(const float *in, int rows, int S, const pcp_object_aug_t &a, const float *__restrict__ states,
                                         const int *__restrict__ n_boxes, int M, const float *__restrict__ frame_thr, float *sbox,
                                         unsigned long long *s_mask, ObjRow (&r)[OBJ_ITEMS]) {
  if (threadIdx.x == 0) *s_mask = 0ULL;
  __syncthreads();
#pragma unroll
  for (int it = 0; it < OBJ_ITEMS; it++) {
    const int i = it * OBJ_THREADS + threadIdx.x;
    r[it].frame = -1;
    r[it].dead = false;
    r[it].x = r[it].y = r[it].z = 0.f;
    if (i < rows) {
      const float *row = in + i * S;
      const float fb = row[0];
      r[it].x = row[1];
      r[it].y = row[2];
      r[it].z = row[3];
      if (fb >= 0.f && fb < (float)a.batch) {
        r[it].frame = (int)fb;
        atomicOr(s_mask, 1ULL << r[it].frame);                   // an integer or: the order does not reach the result
      }
    }
  }
  __syncthreads();
  unsigned long long mask = *s_mask;
  while (mask) {
    const int f = __ffsll((long long)mask) - 1;
    mask &= mask - 1;
    const int nb = min(max(n_boxes ? n_boxes[f] : 0, 0), M);
    for (int k = 0; k < a.n_stages; k++) {
      const int st = a.stage[k];
      if (obj_is_world(st)) {
        const float t = frame_thr[f];
#pragma unroll
        for (int it = 0; it < OBJ_ITEMS; it++)
          if (r[it].frame == f && !r[it].dead) {
            const float v = (st == PCP_OBJ_WORLD_DROP_TOP || st == PCP_OBJ_WORLD_DROP_BOTTOM) ? r[it].z : r[it].y;
            const bool keep = (st == PCP_OBJ_WORLD_DROP_TOP || st == PCP_OBJ_WORLD_DROP_LEFT) ? v < t : v > t;
            r[it].dead = !keep;
          }
        continue;
      }
      const float *src = states + ((size_t)f * a.n_stages + k) * (size_t)M * SS;
      for (int c0 = 0; c0 < nb; c0 += PCP_OBJ_LDS_BOXES) {
        const int cnt = min(PCP_OBJ_LDS_BOXES, nb - c0);
        __syncthreads();                                         // the previous chunk has been read by every thread
        aug_stage_in<OBJ_THREADS>(sbox, src + (size_t)c0 * SS, cnt * SS);
        __syncthreads();
#pragma unroll
        for (int it = 0; it < OBJ_ITEMS; it++)
          if (r[it].frame == f)
            for (int j = 0; j < cnt && !r[it].dead; j++) obj_apply(st, sbox + j * SS, r[it]);
      }
    }
  }
}

// PLACE false: rows of this tile that survive -> tile_cnt[tile], per frame -> frame_count.  PLACE true: the moved rows, compacted when
// `compact`, to `out`.
template <bool PLACE>
__global__ __launch_bounds__(OBJ_THREADS) void k_obj_points(const float *__restrict__ points, long long n, int S, pcp_object_aug_t a,
                                                            const float *__restrict__ states, const int *__restrict__ n_boxes, int M,
                                                            const float *__restrict__ frame_thr, int compact, int *__restrict__ tile_cnt,
                                                            int *__restrict__ frame_count, float *__restrict__ out) {
  extern __shared__ f32x4 obj_lds4[];
  float *in = reinterpret_cast<float *>(obj_lds4);
  __shared__ f32x4 s_box4[PCP_OBJ_LDS_BOXES * SS / 4];
  __shared__ unsigned long long s_mask;
  __shared__ int s_frame[PCP_AUG_MAX_BATCH + 1];                 // [batch]: kept rows of a frame outside [0, batch)
  __shared__ int s_wave[OBJ_ITEMS][OBJ_WAVES];
  __shared__ long long s_before[OBJ_WAVES];
  float *sbox = reinterpret_cast<float *>(s_box4);
  const long long base = (long long)blockIdx.x * PCP_AUG_TILE_ROWS;
  const int rows = (int)((n - base) < PCP_AUG_TILE_ROWS ? (n - base) : PCP_AUG_TILE_ROWS);
  if (!PLACE && threadIdx.x <= PCP_AUG_MAX_BATCH) s_frame[threadIdx.x] = 0;
  aug_stage_in<OBJ_THREADS>(in, points + base * S, rows * S);
  const long long before = PLACE && compact ? aug_tile_before<OBJ_THREADS>(tile_cnt) : 0;
  __syncthreads();
  ObjRow r[OBJ_ITEMS];
  obj_walk(in, rows, S, a, states, n_boxes, M, frame_thr, sbox, &s_mask, r);
  bool keep[OBJ_ITEMS];
  int rank[OBJ_ITEMS];
#pragma unroll
  for (int it = 0; it < OBJ_ITEMS; it++) {
    const int i = it * OBJ_THREADS + threadIdx.x;
    keep[it] = i < rows && !r[it].dead;
    if (PLACE && keep[it] && r[it].frame >= 0) {                 // this thread's own row: no other thread touches it
      float *row = in + i * S;
      row[1] = r[it].x;
      row[2] = r[it].y;
      row[3] = r[it].z;
    }
    if (!PLACE && keep[it]) atomicAdd(&s_frame[r[it].frame >= 0 ? r[it].frame : a.batch], 1);
    rank[it] = aug_tile_rank<OBJ_THREADS>(keep[it], it, s_wave);
  }
  if (!PLACE) {
    aug_tile_count_finish<OBJ_THREADS>(s_wave, s_frame, a.batch + 1, tile_cnt, frame_count);
    return;
  }
  if (!compact) {                                                // same place, same alignment: the tile goes back as it came
    __syncthreads();
    aug_stage_out<OBJ_THREADS>(out + base * S, in, 0, rows * S);
    return;
  }
  float *ob = in + PCP_AUG_TILE_ROWS * S;                        // second buffer: 4 floats longer than a tile
  aug_tile_compact<OBJ_THREADS>(before, keep, rank, in, ob, S, s_wave, s_before, out);
}

// one workgroup per frame, a thread per box row: the box through every sub-stage, its record written in front of each
__global__ __launch_bounds__(256) void k_obj_boxes(pcp_object_aug_t a, const float *__restrict__ params, float *__restrict__ gt, int M, int W,
                                                   float *__restrict__ states, int *__restrict__ n_boxes) {
  __shared__ int s_last;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) s_last = 0;
  __syncthreads();
  for (int m = threadIdx.x; m < M; m += 256) {
    float *box = gt + ((size_t)b * M + m) * W;
    const bool real = box[W - 1] != 0.f;
    if (real) atomicMax(&s_last, m + 1);
    float c[3] = {box[0], box[1], box[2]}, d[3] = {box[3], box[4], box[5]}, h = box[6];
    for (int k = 0; k < a.n_stages; k++) {
      const int st = a.stage[k];
      const float *p = params + (((size_t)b * a.n_stages + k) * M + m) * PS;
      f32x4 *rec = reinterpret_cast<f32x4 *>(states + (((size_t)b * a.n_stages + k) * M + m) * SS);
      // math.cos(-rz), math.sin(-rz): float64 of the float32 heading, rounded to float32 where numpy multiplies a float32 array by them
      const double nh = -(double)h;
      float p0 = p[0], p1 = 0.f;
      const float half_z = __fmul_rn(d[2], 0.5f);
      if (st == PCP_OBJ_ROTATE) {
        p0 = p[1];
        p1 = p[2];
      } else if (st == PCP_OBJ_DROP_TOP) {
        p0 = __fsub_rn(__fadd_rn(c[2], half_z), __fmul_rn(p[0], d[2]));
      } else if (st == PCP_OBJ_DROP_BOTTOM) {
        p0 = __fadd_rn(__fsub_rn(c[2], half_z), __fmul_rn(p[0], d[2]));
      } else if (st == PCP_OBJ_DROP_LEFT) {
        p0 = __fsub_rn(__fadd_rn(c[1], __fmul_rn(d[1], 0.5f)), __fmul_rn(p[0], d[1]));
      } else if (st == PCP_OBJ_DROP_RIGHT) {
        p0 = __fadd_rn(__fsub_rn(c[1], __fmul_rn(d[1], 0.5f)), __fmul_rn(p[0], d[1]));
      }
      f32x4 v0 = {c[0], c[1], c[2], __fadd_rn(__fmul_rn(d[0], 0.5f), OBJ_MARGIN)};
      f32x4 v1 = {__fadd_rn(__fmul_rn(d[1], 0.5f), OBJ_MARGIN), real ? half_z : -1.f, (float)cos(nh), (float)sin(nh)};
      f32x4 v2 = {p0, p1, 0.f, 0.f};
      rec[0] = v0;
      rec[1] = v1;
      rec[2] = v2;
      if (!real) continue;
      if (st >= PCP_OBJ_TRANSLATE_X && st <= PCP_OBJ_TRANSLATE_Z) c[st - PCP_OBJ_TRANSLATE_X] = __fadd_rn(c[st - PCP_OBJ_TRANSLATE_X], p[0]);
      else if (st == PCP_OBJ_SCALE)
        for (int i = 0; i < 3; i++) d[i] = __fmul_rn(d[i], p[0]);
      else if (st == PCP_OBJ_ROTATE) h = __fadd_rn(h, p[0]);
    }
    if (!real) continue;
    if (a.limit_heading) h = aug_limit_period(h);
    for (int i = 0; i < 3; i++) {
      box[i] = c[i];
      box[3 + i] = d[i];
    }
    box[6] = h;
  }
  __syncthreads();
  if (threadIdx.x == 0) n_boxes[b] = s_last;
}

// floats in an order-preserving integer form: min / max of the keys is min / max of the floats, whatever the order of the updates
__device__ __forceinline__ int obj_key(float v) {
  const int i = __float_as_int(v);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float obj_unkey(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }
constexpr int OBJ_KEY_PINF = 0x7f800000;                         // +inf
constexpr int OBJ_KEY_NINF = (int)0xff800000 ^ 0x7fffffff;       // -inf

// pass 1: part[tile][b] = (min key, max key) of the tile's rows of frame b
__global__ __launch_bounds__(OBJ_THREADS) void k_obj_extent_tiles(const float *__restrict__ points, long long n, int S, int batch, int col,
                                                                  int *__restrict__ part) {
  __shared__ int s_min[PCP_AUG_MAX_BATCH], s_max[PCP_AUG_MAX_BATCH];
  if (threadIdx.x < PCP_AUG_MAX_BATCH) {
    s_min[threadIdx.x] = OBJ_KEY_PINF;
    s_max[threadIdx.x] = OBJ_KEY_NINF;
  }
  __syncthreads();
  const long long base = (long long)blockIdx.x * PCP_AUG_TILE_ROWS;
#pragma unroll
  for (int it = 0; it < OBJ_ITEMS; it++) {
    const long long i = base + it * OBJ_THREADS + threadIdx.x;
    if (i < n) {
      const float fb = points[i * S];
      if (fb >= 0.f && fb < (float)batch) {
        const int key = obj_key(points[i * S + col]);
        atomicMin(&s_min[(int)fb], key);                         // integer min / max in LDS
        atomicMax(&s_max[(int)fb], key);
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < batch) {
    part[((size_t)blockIdx.x * batch + threadIdx.x) * 2] = s_min[threadIdx.x];
    part[((size_t)blockIdx.x * batch + threadIdx.x) * 2 + 1] = s_max[threadIdx.x];
  }
}

// pass 2: one workgroup per frame over the tiles
__global__ __launch_bounds__(256) void k_obj_extent_frames(const int *__restrict__ part, int tiles, int batch, float *__restrict__ extent) {
  __shared__ int s_min[4], s_max[4];
  const int b = blockIdx.x;
  int lo = OBJ_KEY_PINF, hi = OBJ_KEY_NINF;
  for (int t = threadIdx.x; t < tiles; t += 256) {
    lo = min(lo, part[((size_t)t * batch + b) * 2]);
    hi = max(hi, part[((size_t)t * batch + b) * 2 + 1]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    lo = min(lo, __shfl_xor(lo, d, 64));
    hi = max(hi, __shfl_xor(hi, d, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    s_min[threadIdx.x >> 6] = lo;
    s_max[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; w++) {
      lo = min(lo, s_min[w]);
      hi = max(hi, s_max[w]);
    }
    extent[2 * b] = obj_unkey(lo);
    extent[2 * b + 1] = obj_unkey(hi);
  }
}

// one workgroup per frame: the threshold, which boxes stay, and the copy
__global__ __launch_bounds__(256) void k_obj_drop_boxes(const float *__restrict__ gt, int M, int W, const float *__restrict__ tf, int n_sweeps,
                                                        int R, const float *__restrict__ extent, const float *__restrict__ intensity, int dir,
                                                        float *__restrict__ frame_thr, float *__restrict__ gt_out, float *__restrict__ tf_out,
                                                        int *__restrict__ n_out) {
  __shared__ short s_dst[PCP_OBJ_MAX_BOXES];
  __shared__ int s_kept;
  const int b = blockIdx.x;
  const float lo = extent[2 * b], hi = extent[2 * b + 1];
  const bool upper = dir == PCP_OBJ_WORLD_DROP_TOP || dir == PCP_OBJ_WORLD_DROP_LEFT;   // keeps col < thr
  const bool empty = !(lo <= hi);                                // a frame without rows has no extent: everything passes
  float thr;
  if (empty) thr = upper ? __int_as_float(0x7f800000) : __int_as_float((int)0xff800000);
  else {
    const float span = __fmul_rn(intensity[b], __fsub_rn(hi, lo));
    thr = upper ? __fsub_rn(hi, span) : __fadd_rn(lo, span);
  }
  const int col = (dir == PCP_OBJ_WORLD_DROP_TOP || dir == PCP_OBJ_WORLD_DROP_BOTTOM) ? 2 : 1;
  const float *g = gt + (size_t)b * M * W;
  if (threadIdx.x == 0) {
    frame_thr[b] = thr;
    int run = 0;
    for (int m = 0; m < M; m++) {
      const float v = g[m * W + col];
      const bool keep = empty ? true : (g[m * W + W - 1] != 0.f && (upper ? v < thr : v > thr));
      s_dst[m] = keep ? (short)run++ : (short)-1;
    }
    s_kept = run;
    int real = 0;
    for (int m = 0; m < M; m++) real += (s_dst[m] >= 0 && g[m * W + W - 1] != 0.f) ? 1 : 0;
    n_out[b] = real;
  }
  __syncthreads();
  const int kept = s_kept;
  float *go = gt_out + (size_t)b * M * W;
  for (int i = threadIdx.x; i < M * W; i += 256) {
    const int m = i / W, d = s_dst[m];
    if (d >= 0) go[d * W + (i - m * W)] = g[i];
    if (m >= kept) go[i] = 0.f;
  }
  if (!tf_out) return;
  const int per = n_sweeps * R * 4;
  const float *t = tf + (size_t)b * M * per;
  float *to = tf_out + (size_t)b * M * per;
  for (int i = threadIdx.x; i < M * per; i += 256) {
    const int m = i / per, d = s_dst[m], c = (i - m * per) % (R * 4);
    if (d >= 0) to[d * per + (i - m * per)] = t[i];
    if (m >= kept) to[i] = aug_identity_pad(c);
  }
}

bool obj_ok(const pcp_object_aug_t *a, bool points) {
  if (!a || a->n_stages < 0 || a->n_stages > PCP_OBJ_MAX_STAGES || a->batch <= 0 || a->batch > PCP_AUG_MAX_BATCH) return false;
  for (int k = 0; k < a->n_stages; k++) {
    if (a->stage[k] < PCP_OBJ_TRANSLATE_X || a->stage[k] > PCP_OBJ_WORLD_DROP_RIGHT) return false;
    if (a->stage[k] >= PCP_OBJ_WORLD_DROP_TOP && (!points || a->n_stages != 1)) return false;
  }
  return true;
}

}  // namespace

extern "C" int pcp_object_augment_boxes(const pcp_object_aug_t *aug, const float *params, float *gt_boxes, int32_t max_boxes, int32_t box_width,
                                        float *box_states, int32_t *n_boxes, void *stream) {
  if (!obj_ok(aug, false) || max_boxes < 0 || (box_width != 8 && box_width != 10) || !n_boxes) return PCP_ERR_ARG;
  if (max_boxes > PCP_OBJ_MAX_BOXES) return PCP_ERR_UNSUPPORTED;
  if (max_boxes > 0 && (!gt_boxes || (aug->n_stages > 0 && (!params || !box_states)))) return PCP_ERR_ARG;
  if ((((uintptr_t)box_states) & 15) || (((uintptr_t)params) & 3)) return PCP_ERR_ARG;
  for (int k = 0; k < aug->n_stages; k++)
    if (aug->stage[k] == PCP_OBJ_ROTATE && box_width == 10) return PCP_ERR_UNSUPPORTED;   // the reference's velocity branch raises
  hipLaunchKernelGGL(k_obj_boxes, dim3(aug->batch), dim3(256), 0, (hipStream_t)stream, *aug, params, gt_boxes, (int)max_boxes, (int)box_width,
                     box_states, (int *)n_boxes);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" size_t pcp_object_augment_points_workspace_bytes(int64_t n) {
  return aug_points_workspace_bytes(n);
}

extern "C" int pcp_object_augment_points(const pcp_object_aug_t *aug, const float *box_states, const int32_t *n_boxes, int32_t max_boxes,
                                         const float *frame_thr, const float *points, int64_t n, int32_t row_stride, float *out,
                                         int32_t *frame_count, void *workspace, size_t workspace_bytes, void *stream_) {
  if (!obj_ok(aug, true) || max_boxes < 0) return PCP_ERR_ARG;
  int st = aug_points_shape(n, row_stride);
  if (st != PCP_OK) return st;
  if (max_boxes > PCP_OBJ_MAX_BOXES) return PCP_ERR_UNSUPPORTED;
  bool drop = false, world = false, local = false;
  for (int k = 0; k < aug->n_stages; k++) {
    drop |= aug->stage[k] >= PCP_OBJ_DROP_TOP;
    world |= aug->stage[k] >= PCP_OBJ_WORLD_DROP_TOP;
    local |= aug->stage[k] < PCP_OBJ_WORLD_DROP_TOP;
  }
  if (world && !frame_thr) return PCP_ERR_ARG;
  if (local && max_boxes > 0 && (!box_states || !n_boxes)) return PCP_ERR_ARG;
  if (((uintptr_t)box_states) & 15) return PCP_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  st = aug_points_buffers(points, n, out, drop, aug->batch + 1, frame_count, workspace, workspace_bytes, stream);
  if (st != PCP_OK || n == 0) return st;
  const int M = local ? (int)max_boxes : 0;                            // no box is read by a world dropout
  const int tiles = (int)((n + PCP_AUG_TILE_ROWS - 1) / PCP_AUG_TILE_ROWS);
  const size_t tile_bytes = (size_t)PCP_AUG_TILE_ROWS * row_stride * 4;
  if (drop) {
    hipLaunchKernelGGL(k_obj_points<false>, dim3(tiles), dim3(OBJ_THREADS), tile_bytes, stream, points, (long long)n, (int)row_stride, *aug,
                       box_states, (const int *)n_boxes, M, frame_thr, 1, (int *)workspace, (int *)frame_count, (float *)nullptr);
    PCP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_obj_points<true>, dim3(tiles), dim3(OBJ_THREADS), drop ? 2 * tile_bytes + 16 : tile_bytes, stream, points, (long long)n,
                     (int)row_stride, *aug, box_states, (const int *)n_boxes, M, frame_thr, drop ? 1 : 0, (int *)workspace, (int *)nullptr, out);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" size_t pcp_frame_extent_workspace_bytes(int64_t n, int32_t batch) {
  if (n < 0 || batch <= 0) return 0;
  const int64_t tiles = (n + PCP_AUG_TILE_ROWS - 1) / PCP_AUG_TILE_ROWS;
  return pcp_align_up((size_t)(tiles > 0 ? tiles : 1) * (size_t)batch * 8, 256);
}

extern "C" int pcp_frame_extent(const float *points, int64_t n, int32_t row_stride, int32_t batch, int32_t col, float *extent, void *workspace,
                                size_t workspace_bytes, void *stream_) {
  if (n < 0 || batch <= 0 || batch > PCP_AUG_MAX_BATCH || row_stride < PCP_AUG_MIN_ROW_STRIDE || row_stride > PCP_AUG_MAX_ROW_STRIDE ||
      col < 1 || col >= row_stride || !extent || !workspace || (n > 0 && !points))
    return PCP_ERR_ARG;
  if (n * row_stride >= (1LL << 31)) return PCP_ERR_UNSUPPORTED;
  if (workspace_bytes < pcp_frame_extent_workspace_bytes(n, batch)) return PCP_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int tiles = (int)((n + PCP_AUG_TILE_ROWS - 1) / PCP_AUG_TILE_ROWS);
  if (tiles > 0) {
    hipLaunchKernelGGL(k_obj_extent_tiles, dim3(tiles), dim3(OBJ_THREADS), 0, stream, points, (long long)n, (int)row_stride, (int)batch, (int)col,
                       (int *)workspace);
    PCP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_obj_extent_frames, dim3(batch), dim3(256), 0, stream, (const int *)workspace, tiles, (int)batch, extent);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

extern "C" int pcp_object_augment_drop_boxes(const float *gt_boxes, int32_t batch, int32_t max_boxes, int32_t box_width, const float *instances_tf,
                                             int32_t n_sweeps, int32_t tf_rows, const float *extent, const float *intensity, int32_t direction,
                                             float *frame_thr, float *gt_out, float *tf_out, int32_t *n_boxes_out, void *stream) {
  if (batch <= 0 || batch > PCP_AUG_MAX_BATCH || max_boxes < 0 || (box_width != 8 && box_width != 10) || !extent || !intensity || !frame_thr ||
      !n_boxes_out || direction < PCP_OBJ_WORLD_DROP_TOP || direction > PCP_OBJ_WORLD_DROP_RIGHT)
    return PCP_ERR_ARG;
  if (max_boxes > PCP_OBJ_MAX_BOXES) return PCP_ERR_UNSUPPORTED;
  if (max_boxes > 0 && (!gt_boxes || !gt_out || gt_boxes == gt_out)) return PCP_ERR_ARG;
  if (tf_out && (!instances_tf || instances_tf == tf_out || n_sweeps <= 0 || (tf_rows != 3 && tf_rows != 4))) return PCP_ERR_ARG;
  hipLaunchKernelGGL(k_obj_drop_boxes, dim3(batch), dim3(256), 0, (hipStream_t)stream, gt_boxes, (int)max_boxes, (int)box_width, instances_tf,
                     (int)n_sweeps, (int)tf_rows, extent, intensity, (int)direction, frame_thr, gt_out, max_boxes > 0 ? tf_out : (float *)nullptr,
                     (int *)n_boxes_out);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}
