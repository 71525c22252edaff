// Detection evaluation by the nuScenes protocol on the device (include/pcp_hip.h: pcp_det_eval_match / pcp_det_eval_curves; host side
// pcp_amd/det_eval.py).  The reference hands its detections to nuscenes-devkit on the host (pcdet/datasets/v2x_sim/v2x_sim_eval_utils.py,
// pcdet/datasets/nuscenes/nuscenes_eval_utils.py); the protocol itself is small:
//   k_eval_match   one workgroup per (frame, class), one wave per distance threshold.  The frame's predictions of the class are compacted
//                  into LDS in slot order and sorted by (score descending, slot ascending) with a bitonic network over 64-bit keys; the
//                  ground-truth rows of the class are compacted in row order.  Each wave then walks the predictions in that order: its
//                  lanes stride over the rows not yet taken (lane l owns rows l, l + 64, ...: the taken bits are eight bits of a register),
//                  a shuffle min-reduce over (distance bits, row) picks the nearest with ties to the lower row, and a distance under the
//                  wave's threshold takes the row.  The wave of the TP threshold also leaves the four errors.  Every prediction's record
//                  goes to its own slot: no compaction across workgroups, no atomics, so a call repeats bit for bit.
//   k_eval_curves  one workgroup per (class, threshold) over the epoch's records, sorted by the host.  A running scan in float64 leaves the
//                  TP count behind every record and, at the TP threshold, the list of matches with the NaN-aware running means of their
//                  errors; 101 threads then evaluate the precision / confidence / error curves the way numpy.interp does (largest sample
//                  not above x, the sample itself on equality, one slope product otherwise).
// Neither kernel is near a roofline: the point is that the boxes never leave the device and an epoch ends with one read.
#include "pcp_common.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_MAX = PCP_EVAL_MAX_BOXES;
constexpr int EV_T = PCP_EVAL_THRESHOLDS;
constexpr int EV_RW = PCP_EVAL_RECORD_WORDS;
constexpr int EV_PTS = PCP_EVAL_POINTS;
constexpr int EV_STRIDE = 3 * EV_T * EV_PTS + 8;           // doubles per class of the curve output
static_assert(EV_THREADS == 64 * EV_T, "one wave per threshold");
static_assert(EV_MAX == 2 * EV_THREADS && EV_MAX <= 64 * 32, "the sort pairs and the per-lane taken bits");
static_assert(EV_RW == 8, "a record is two 16-byte stores");

struct EvThresholds {
  float v[EV_T];
};

typedef unsigned long long u64;

// ascending key order = descending score (-0 counts as +0)
__device__ __forceinline__ unsigned ev_score_key(float s) {
  unsigned u = __float_as_uint(s + 0.0f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

// positions of the set flags of a workgroup-wide pass in thread order: -> this thread's position (valid where f), `base` moves on
__device__ __forceinline__ int ev_compact(bool f, int &base, int *s_wave) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 bal = __ballot(f);
  const int within = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) s_wave[w] = __popcll(bal);
  __syncthreads();
  int off = base, tot = 0;
#pragma unroll
  for (int q = 0; q < EV_T; q++) {
    if (q < w) off += s_wave[q];
    tot += s_wave[q];
  }
  base += tot;
  __syncthreads();
  return off + within;
}

__device__ __forceinline__ float ev_orient_err(float yaw_gt, float yaw_pred, float period) {
  const float half = period * 0.5f;
  const float a = yaw_gt - yaw_pred + half;
  float r = a - floorf(a / period) * period;                // (x - y + p / 2) mod p, the sign of p
  if (r < 0.f) r += period;
  if (r >= period) r -= period;
  r -= half;
  if (r > 3.14159265358979f) r -= 6.28318530717959f;
  return fabsf(r);
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_match(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                           const long long *__restrict__ labels, const int *__restrict__ count, int K, int BW,
                                                           const float *__restrict__ gt, int M, int GW, int C, EvThresholds ths, int tp_index,
                                                           const float *__restrict__ period, const int *__restrict__ flags,
                                                           long long frame_base, uint4 *__restrict__ records, int *__restrict__ gt_count) {
  __shared__ u64 s_key[EV_MAX];
  __shared__ float s_px[EV_MAX], s_py[EV_MAX], s_gx[EV_MAX], s_gy[EV_MAX];
  __shared__ int s_gm[EV_MAX], s_match[EV_MAX];
  __shared__ float s_err[4][EV_MAX];
  __shared__ unsigned char s_tp[EV_T][EV_MAX];
  __shared__ int s_wave[EV_T];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int c = blockIdx.x + 1, b = blockIdx.y;
  const long long frame = frame_base + b;
  const int cnt = min(max(count[b], 0), K);
  const float *fb = boxes + (size_t)b * K * BW;
  const float *fs = scores + (size_t)b * K;
  const long long *fl = labels + (size_t)b * K;
  uint4 *rec = records + (size_t)frame * K * 2;

  // the slots without a prediction of any class: written once per frame, by the workgroup of the first class
  if (c == 1) {
    for (int k = t; k < K; k += EV_THREADS) {
      const long long l = k < cnt ? fl[k] : 0;
      if (l < 1 || l > C) {
        rec[2 * k] = make_uint4(0u, 0u, 0u, 0xffffffffu);
        rec[2 * k + 1] = make_uint4(0u, 0u, 0u, 0u);
      }
    }
  }

  // predictions of the class, in slot order
  for (int i = t; i < EV_MAX; i += EV_THREADS) s_key[i] = ~0ull;
  __syncthreads();
  int n_pred = 0;
  for (int k0 = 0; k0 < cnt; k0 += EV_THREADS) {
    const int k = k0 + t;
    const bool f = k < cnt && fl[k] == (long long)c;
    const int pos = ev_compact(f, n_pred, s_wave);
    if (f && pos < EV_MAX) s_key[pos] = ((u64)ev_score_key(fs[k]) << 32) | (unsigned)k;
  }
  n_pred = min(n_pred, EV_MAX);
  // ground-truth rows of the class, in row order
  int n_gt = 0;
  for (int j0 = 0; j0 < M; j0 += EV_THREADS) {
    const int j = j0 + t;
    const float *g = gt + ((size_t)b * M + min(j, M - 1)) * GW;
    const bool f = j < M && g[GW - 1] == (float)c;
    const int pos = ev_compact(f, n_gt, s_wave);
    if (f && pos < EV_MAX) {
      s_gx[pos] = g[0];
      s_gy[pos] = g[1];
      s_gm[pos] = j;
    }
  }
  if (t == 0) gt_count[frame * C + (c - 1)] = n_gt;
  n_gt = min(n_gt, EV_MAX);
  if (n_pred == 0) return;                                            // uniform: nothing of this class to record

  // bitonic network over the EV_MAX keys (the empty ones sort behind every prediction): score descending, slot ascending
  for (int size = 2; size <= EV_MAX; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      const int pos = 2 * t - (t & (stride - 1));
      const u64 a = s_key[pos], o = s_key[pos + stride];
      if ((a > o) == ((pos & size) == 0)) {
        s_key[pos] = o;
        s_key[pos + stride] = a;
      }
    }
  }
  __syncthreads();
  for (int p = t; p < n_pred; p += EV_THREADS) {
    const float *pb = fb + (size_t)(unsigned)(s_key[p] & 0xffffffffull) * BW;
    s_px[p] = pb[0];
    s_py[p] = pb[1];
  }
  __syncthreads();

  // one wave per threshold
  const float th = ths.v[w];
  const bool tp_wave = w == tp_index;
  const float per = period[c - 1];
  const int fl_c = flags[c - 1];
  unsigned taken = 0u;
  const int rounds = (n_gt + 63) >> 6;
  for (int p = 0; p < n_pred; p++) {
    const float x = s_px[p], y = s_py[p];
    u64 best = ~0ull;
    for (int i = 0; i < rounds; i++) {
      const int j = lane + 64 * i;
      if (j < n_gt && !((taken >> i) & 1u)) {
        const float dx = s_gx[j] - x, dy = s_gy[j] - y;
        const float d = sqrtf(dx * dx + dy * dy);
        const u64 kk = ((u64)__float_as_uint(d) << 32) | (unsigned)j;
        best = kk < best ? kk : best;
      }
    }
    best = wave_min_u64(best);
    const float d = __uint_as_float((unsigned)(best >> 32));
    const int j = (int)(best & 0xffffffffull);
    const bool tp = best != ~0ull && d < th;                          // a NaN distance never matches
    if (tp && (j & 63) == lane) taken |= 1u << (j >> 6);
    if (lane == 0) {
      s_tp[w][p] = tp ? 1 : 0;
      if (tp_wave) {
        float e_scale = 0.f, e_orient = 0.f, e_vel = 0.f;
        if (tp) {
          const float *pb = fb + (size_t)(unsigned)(s_key[p] & 0xffffffffull) * BW;
          const float *g = gt + ((size_t)b * M + s_gm[j]) * GW;
          const float inter = fminf(pb[3], g[3]) * fminf(pb[4], g[4]) * fminf(pb[5], g[5]);
          const float va = g[3] * g[4] * g[5], vb = pb[3] * pb[4] * pb[5];
          e_scale = 1.f - inter / (va + vb - inter);
          e_orient = (fl_c & PCP_EVAL_NAN_ORIENT) ? __uint_as_float(0x7fc00000u) : ev_orient_err(g[6], pb[6], per);
          if (fl_c & PCP_EVAL_NAN_VEL) e_vel = __uint_as_float(0x7fc00000u);
          else if (BW == 9 && GW == 10) {
            const float vx = g[7] - pb[7], vy = g[8] - pb[8];
            e_vel = sqrtf(vx * vx + vy * vy);
          }
        }
        s_match[p] = tp ? s_gm[j] : -1;
        s_err[0][p] = tp ? d : 0.f;
        s_err[1][p] = e_scale;
        s_err[2][p] = e_orient;
        s_err[3][p] = e_vel;
      }
    }
  }
  __syncthreads();
  for (int p = t; p < n_pred; p += EV_THREADS) {
    const unsigned k = (unsigned)(s_key[p] & 0xffffffffull);
    unsigned mask = 0u;
#pragma unroll
    for (int q = 0; q < EV_T; q++) mask |= (unsigned)s_tp[q][p] << q;
    rec[2 * k] = make_uint4(__float_as_uint(fs[k]), (unsigned)c, mask, (unsigned)s_match[p]);
    rec[2 * k + 1] = make_uint4(__float_as_uint(s_err[0][p]), __float_as_uint(s_err[1][p]), __float_as_uint(s_err[2][p]),
                                __float_as_uint(s_err[3][p]));
  }
}

// numpy.interp on samples xp[j] = tpc[j] / npos (non-decreasing), right = 0
template <typename F>
__device__ __forceinline__ double ev_interp_recall(double x, const int *__restrict__ tpc, int n, double npos, F fp) {
  if (x > (double)tpc[n - 1] / npos) return 0.0;
  if (x < (double)tpc[0] / npos) return fp(0);
  int lo = 0, hi = n;                                                 // -> the largest j with xp[j] <= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((double)tpc[mid] / npos <= x) lo = mid + 1;
    else hi = mid;
  }
  const int j = lo - 1;
  const double xj = (double)tpc[j] / npos;
  if (j == n - 1 || xj == x) return fp(j);
  const double slope = (fp(j + 1) - fp(j)) / ((double)tpc[j + 1] / npos - xj);
  return slope * (x - xj) + fp(j);
}

// numpy.interp(x, tc[::-1], cm[::-1]) for a non-increasing tc of n > 0 samples (default ends: the outer samples)
__device__ __forceinline__ double ev_interp_conf(double x, const double *__restrict__ tc, const double *__restrict__ cm, int n) {
  if (x > tc[0]) return cm[0];
  int lo = 0, hi = n;                                                 // -> the first o with tc[o] <= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tc[mid] <= x) hi = mid;
    else lo = mid + 1;
  }
  if (lo == n) return cm[n - 1];
  if (lo == 0 || tc[lo] == x) return cm[lo];
  const double slope = (cm[lo - 1] - cm[lo]) / (tc[lo - 1] - tc[lo]);
  double r = slope * (x - tc[lo]) + cm[lo];
  if (r != r) {                                                       // numpy: a NaN from one side, try the other
    r = slope * (x - tc[lo - 1]) + cm[lo - 1];
    if (r != r && cm[lo] == cm[lo - 1]) r = cm[lo];
  }
  return r;
}

__global__ __launch_bounds__(EV_THREADS) void k_eval_curves(const unsigned *__restrict__ sorted, long long n, const int *__restrict__ class_start,
                                                            const int *__restrict__ npos_all, int tp_index, const double *__restrict__ rec_interp,
                                                            double *__restrict__ ws_list, int *__restrict__ ws_tpc, double *__restrict__ out) {
  __shared__ int s_itot[EV_T][5];
  __shared__ double s_dtot[EV_T][4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int tt = blockIdx.x, c = blockIdx.y + 1;
  const bool errs = tt == tp_index;
  const int s0 = class_start[c], N = class_start[c + 1] - s0, npos_i = npos_all[c - 1];
  double *o = out + (size_t)(c - 1) * EV_STRIDE;
  double *o_prec = o + tt * EV_PTS, *o_conf = o + (EV_T + tt) * EV_PTS, *o_err = o + 2 * EV_T * EV_PTS;
  if (t == 0) {
    if (tt == 0) {
      o[3 * EV_T * EV_PTS] = (double)npos_i;
      o[3 * EV_T * EV_PTS + 1 + EV_T] = (double)N;
      o[3 * EV_T * EV_PTS + 2 + EV_T] = 0.0;
      o[3 * EV_T * EV_PTS + 3 + EV_T] = 0.0;
    }
  }
  if (npos_i <= 0 || N <= 0) {                                        // the "no predictions" data
    if (t < EV_PTS) {
      o_prec[t] = 0.0;
      o_conf[t] = 0.0;
      if (errs)
        for (int m = 0; m < 4; m++) o_err[m * EV_PTS + t] = 1.0;
    }
    if (t == 0) o[3 * EV_T * EV_PTS + 1 + tt] = 0.0;
    return;
  }
  const unsigned *rec = sorted + (size_t)s0 * EV_RW;
  int *tpc = ws_tpc + (size_t)tt * n + s0;
  double *l_conf = ws_list + s0;                                      // the match list of the class: confidence, then four running means
  int c_tp = 0, c_cnt[4] = {0, 0, 0, 0};
  double c_sum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i0 = 0; i0 < N; i0 += EV_THREADS) {
    const int i = i0 + t;
    const bool valid = i < N;
    const unsigned *r = rec + (size_t)min(i, N - 1) * EV_RW;
    const int f = valid && ((r[2] >> tt) & 1u);
    const int tp_w = wave_incl_scan<int>(f, lane);
    int cnt_w[4] = {0, 0, 0, 0};
    double sum_w[4] = {0.0, 0.0, 0.0, 0.0};
    if (errs) {
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const float e = __uint_as_float(r[4 + m]);
        const bool ok = f && e == e;
        cnt_w[m] = wave_incl_scan<int>(ok ? 1 : 0, lane);
        sum_w[m] = wave_incl_scan<double>(ok ? (double)e : 0.0, lane);
      }
    }
    if (lane == 63) {
      s_itot[w][0] = tp_w;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        s_itot[w][1 + m] = cnt_w[m];
        s_dtot[w][m] = sum_w[m];
      }
    }
    __syncthreads();
    int tp_i = c_tp + tp_w, cnt_i[4];
    double sum_i[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      cnt_i[m] = c_cnt[m] + cnt_w[m];
      sum_i[m] = c_sum[m];
    }
#pragma unroll
    for (int q = 0; q < EV_T; q++) {
      if (q < w) {
        tp_i += s_itot[q][0];
#pragma unroll
        for (int m = 0; m < 4; m++) {
          cnt_i[m] += s_itot[q][1 + m];
          sum_i[m] += s_dtot[q][m];
        }
      }
      c_tp += s_itot[q][0];
#pragma unroll
      for (int m = 0; m < 4; m++) {
        c_cnt[m] += s_itot[q][1 + m];
        c_sum[m] += s_dtot[q][m];
      }
    }
    if (valid) tpc[i] = tp_i;
    if (errs && f) {
      l_conf[tp_i - 1] = (double)__uint_as_float(r[0]);
#pragma unroll
      for (int m = 0; m < 4; m++) l_conf[(size_t)(1 + m) * n + tp_i - 1] = cnt_i[m] > 0 ? (sum_i[m] + sum_w[m]) / (double)cnt_i[m] : 0.0;
    }
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();                                                    // the list and the counts are read back by other threads of this workgroup
  if (t == 0) o[3 * EV_T * EV_PTS + 1 + tt] = (double)c_tp;
  if (t >= EV_PTS) return;
  const double x = rec_interp[t], npos = (double)npos_i;
  const double prec = ev_interp_recall(x, tpc, N, npos, [&](int j) { return (double)tpc[j] / (double)(j + 1); });
  const double conf = ev_interp_recall(x, tpc, N, npos, [&](int j) { return (double)__uint_as_float(rec[(size_t)j * EV_RW]); });
  o_prec[t] = prec;
  o_conf[t] = conf;
  if (!errs) return;
#pragma unroll
  for (int m = 0; m < 4; m++)                                          // no match, or only NaN errors: ones
    o_err[m * EV_PTS + t] = (c_tp == 0 || c_cnt[m] == 0) ? 1.0 : ev_interp_conf(conf, l_conf, l_conf + (size_t)(1 + m) * n, c_tp);
}

}  // namespace

extern "C" int pcp_det_eval_match(const float *boxes, const float *scores, const int64_t *labels, const int32_t *count, int32_t batch, int32_t k,
                                  int32_t box_width, const float *gt_boxes, int32_t m, int32_t gt_width, int32_t n_classes,
                                  const float *dist_ths_host, int32_t tp_index, const float *orient_period, const int32_t *class_flags,
                                  int64_t frame_base, void *records, int32_t *gt_count, void *stream) {
  if (batch <= 0 || batch > 65535 || k <= 0 || m < 0 || n_classes <= 0 || frame_base < 0 || (box_width != 7 && box_width != 9) ||
      (gt_width != 8 && gt_width != 10) || tp_index < 0 || tp_index >= EV_T)
    return PCP_ERR_ARG;
  if (!boxes || !scores || !labels || !count || !dist_ths_host || !orient_period || !class_flags || !records || !gt_count || (m > 0 && !gt_boxes))
    return PCP_ERR_ARG;
  if (((uintptr_t)records) & 15) return PCP_ERR_ARG;
  if ((long long)batch * k >= (1LL << 31) || (long long)batch * m >= (1LL << 31)) return PCP_ERR_UNSUPPORTED;
  EvThresholds ths;
  for (int i = 0; i < EV_T; i++) ths.v[i] = dist_ths_host[i];
  hipLaunchKernelGGL(k_eval_match, dim3(n_classes, batch), dim3(EV_THREADS), 0, (hipStream_t)stream, boxes, scores, (const long long *)labels,
                     (const int *)count, (int)k, (int)box_width, gt_boxes, (int)m, (int)gt_width, (int)n_classes, ths, (int)tp_index, orient_period,
                     (const int *)class_flags, (long long)frame_base, (uint4 *)records, (int *)gt_count);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}

// [five float64 lists of n | four int32 lists of n]
extern "C" size_t pcp_det_eval_curves_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return pcp_align_up((size_t)n * (5 * sizeof(double) + EV_T * sizeof(int)), 256) + 256;
}

extern "C" int32_t pcp_det_eval_curves_stride(void) { return EV_STRIDE; }

extern "C" int pcp_det_eval_curves(const void *sorted, int64_t n, const int32_t *class_start, const int32_t *npos, int32_t n_classes,
                                   int32_t tp_index, const double *rec_interp, void *workspace, size_t workspace_bytes, double *out, void *stream) {
  if (n < 0 || n >= (1LL << 31) / EV_RW || n_classes <= 0 || n_classes > 65535 || tp_index < 0 || tp_index >= EV_T) return PCP_ERR_ARG;
  if (!class_start || !npos || !rec_interp || !out || !workspace || (n > 0 && !sorted)) return PCP_ERR_ARG;
  if (((uintptr_t)workspace) & 7) return PCP_ERR_ARG;
  if (workspace_bytes < pcp_det_eval_curves_workspace_bytes(n)) return PCP_ERR_WORKSPACE;
  double *ws_list = (double *)workspace;
  int *ws_tpc = (int *)(ws_list + 5 * (size_t)n);
  hipLaunchKernelGGL(k_eval_curves, dim3(EV_T, n_classes), dim3(EV_THREADS), 0, (hipStream_t)stream, (const unsigned *)sorted, (long long)n,
                     (const int *)class_start, (const int *)npos, (int)tp_index, rec_interp, ws_list, ws_tpc, out);
  PCP_CHECK_LAUNCH();
  return PCP_OK;
}
