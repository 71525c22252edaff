// Rotated BEV overlap and IoU of two boxes on the device: the geometry of csrc/nms.hip, shared with csrc/gt_sample.hip.
//
// The geometry follows the reference arithmetic (pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu, iou3d_cpu.cpp) operation for operation
// (fp32, one rounding per operation) so that a keep set or an "overlaps at all" decision matches away from the threshold.  The
// including file states `#pragma clang fp contract(off)` at file scope first and includes this inside its anonymous namespace.
#pragma once

constexpr float NMS_EPS = 1e-8f;
constexpr float NMS_MARGIN = 1e-2f;

struct P2 { float x, y; };

__device__ __forceinline__ float cross3(P2 a, P2 b, P2 o) { return (a.x - o.x) * (b.y - o.y) - (b.x - o.x) * (a.y - o.y); }

__device__ __forceinline__ bool rects_touch(P2 p1, P2 p2, P2 q1, P2 q2) {
  return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
         fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

__device__ __forceinline__ bool seg_hit(P2 p1, P2 p0, P2 q1, P2 q0, P2 &out) {
  if (!rects_touch(p0, p1, q0, q1)) return false;
  float s1 = cross3(q0, p1, p0);
  float s2 = cross3(p1, q1, p0);
  float s3 = cross3(p0, q1, q0);
  float s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > NMS_EPS) {
    out.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    out.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    float D = a0 * b1 - a1 * b0;
    out.x = (b0 * c1 - b1 * c0) / D;
    out.y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

struct Box {
  float x, y, dx, dy, ang;
};

__device__ __forceinline__ bool corner_in(const Box &b, P2 p) {
  float c = cosf(-b.ang), s = sinf(-b.ang);
  float rx = (p.x - b.x) * c + (p.y - b.y) * (-s);
  float ry = (p.x - b.x) * s + (p.y - b.y) * c;
  return fabsf(rx) < b.dx / 2 + NMS_MARGIN && fabsf(ry) < b.dy / 2 + NMS_MARGIN;
}

__device__ __forceinline__ void corners_of(const Box &b, P2 (&c)[5]) {
  float hx = b.dx / 2, hy = b.dy / 2;
  float x1 = b.x - hx, y1 = b.y - hy, x2 = b.x + hx, y2 = b.y + hy;
  float ca = cosf(b.ang), sa = sinf(b.ang);
  float rx[4] = {x1, x2, x2, x1}, ry[4] = {y1, y1, y2, y2};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    float ddx = rx[k] - b.x, ddy = ry[k] - b.y;
    c[k].x = ddx * ca + ddy * (-sa) + b.x;
    c[k].y = ddx * sa + ddy * ca + b.y;
  }
  c[4] = c[0];
}

__device__ float overlap_area(const Box &a, const Box &b) {
  P2 ca[5], cb[5], poly[16], ctr;
  ctr.x = 0.f;
  ctr.y = 0.f;
  int cnt = 0;
  corners_of(a, ca);
  corners_of(b, cb);
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      P2 hit;
      if (seg_hit(ca[i + 1], ca[i], cb[j + 1], cb[j], hit)) {
        poly[cnt] = hit;
        ctr.x = ctr.x + hit.x;
        ctr.y = ctr.y + hit.y;
        cnt++;
      }
    }
  for (int k = 0; k < 4; k++) {
    if (corner_in(a, cb[k])) { ctr.x = ctr.x + cb[k].x; ctr.y = ctr.y + cb[k].y; poly[cnt++] = cb[k]; }
    if (corner_in(b, ca[k])) { ctr.x = ctr.x + ca[k].x; ctr.y = ctr.y + ca[k].y; poly[cnt++] = ca[k]; }
  }
  if (cnt < 3) return 0.f;          // reference: loops below do not run / a degenerate fan has zero area
  ctr.x /= cnt;
  ctr.y /= cnt;
  for (int j = 0; j < cnt - 1; j++)
    for (int i = 0; i < cnt - j - 1; i++) {
      float ai = atan2f(poly[i].y - ctr.y, poly[i].x - ctr.x);
      float an = atan2f(poly[i + 1].y - ctr.y, poly[i + 1].x - ctr.x);
      if (ai > an) { P2 t = poly[i]; poly[i] = poly[i + 1]; poly[i + 1] = t; }
    }
  float area = 0.f;
  for (int k = 0; k < cnt - 1; k++) {
    float ux = poly[k].x - poly[0].x, uy = poly[k].y - poly[0].y;
    float vx = poly[k + 1].x - poly[0].x, vy = poly[k + 1].y - poly[0].y;
    area += ux * vy - uy * vx;
  }
  return fabsf(area) / 2.0f;
}

__device__ __forceinline__ bool far_apart(const Box &a, const Box &b) {
  // conservative: circumscribed circles (+ margin) do not meet -> no crossing, no corner within the 1e-2 margin
  float ra = 0.5f * sqrtf(a.dx * a.dx + a.dy * a.dy), rb = 0.5f * sqrtf(b.dx * b.dx + b.dy * b.dy);
  float ddx = a.x - b.x, ddy = a.y - b.y, R = ra + rb + 0.1f;
  return ddx * ddx + ddy * ddy > R * R * 1.0001f;
}

__device__ __forceinline__ float iou_of(const Box &a, const Box &b) {
  float sa = a.dx * a.dy, sb = b.dx * b.dy;
  float ov = overlap_area(a, b);
  return ov / fmaxf(sa + sb - ov, NMS_EPS);
}

// axis-aligned IoU of nms_normal_gpu (iou3d_nms_kernel.cu:314-325: the heading is ignored), operation for operation
__device__ __forceinline__ float iou_normal_of(const Box &a, const Box &b) {
  float left = fmaxf(a.x - a.dx / 2, b.x - b.dx / 2), right = fminf(a.x + a.dx / 2, b.x + b.dx / 2);
  float top = fmaxf(a.y - a.dy / 2, b.y - b.dy / 2), bottom = fminf(a.y + a.dy / 2, b.y + b.dy / 2);
  float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
  float inter = width * height;
  float sa = a.dx * a.dy, sb = b.dx * b.dy;
  return inter / fmaxf(sa + sb - inter, NMS_EPS);
}

__device__ __forceinline__ Box load_box(const float *p) {
  Box b;
  b.x = p[0]; b.y = p[1]; b.dx = p[3]; b.dy = p[4]; b.ang = p[6];
  return b;
}
