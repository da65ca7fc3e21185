// dsr_frame.hpp — frame ingest (dsr_frame_inputs*, dsr_batch_refill_frame): one
// depth image + one instance-label image + a list of detections -> each detection's surface
// points, foreground / background rays and observed depths, laid out as dsr_object_in wants them.
// Replaces FrameWithLiDAR.get_detections / pixels_sampler (reconstruct/kitti_sequence.py:70-92,
// :139-146, :200-210), Frame.pixels_sampler (reconstruct/mono_sequence.py:51-73) and get_rays
// (reconstruct/loss_utils.py:23-37).
//
// The second half (dsr_frame_poses*, dsr_batch_refill_frame_poses) gives a detection
// without a pose the reference's mono / RGB-D start: MapObject::RemoveOutliersSimple and
// ComputeCuboidPCA_onlyformono (src/MapObject.cc:249-283, :330-443) on the ingested rows, which are
// then compacted to the kept points (LocalMapping_util.cc:284-410).
//
// The rule is stated once for both sides (frame_sel, frame_ray, frame_finish are __host__
// __device__); the host function walks it forwards (output row i -> its pixel), the kernels
// backwards (every pixel finds out whether an output row wants it), so the two check each other.
//
// Device buffers of one call (H x W image, n_det detections):
//   rows  [n_det][H]  int4   per image row: mask pixels, valid pixels, first / last mask column
//   voff  [n_det][H]  int    exclusive scan of the rows' valid pixels
//   bgoff [n_det][H]  int    per grid row: background candidates, then their exclusive scan
//   aux   [n_det]     int    N_bg (candidates before the max_bg cap)
//   recs  [n_det]     dsr_frame_det_out
// and, for the start poses of §3.5c (dsr_frame_poses, dsr_batch_refill_frame_poses), after them
//   keep  [n_det][max_pts] uchar  per surface point: near after pass 1, kept after pass 2
//   precs [n_det]     dsr_frame_pose_out
#pragma once
#include "../../include/dsr.h"
#include "dsr_dev.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace dsr {

constexpr int FRAME_WG = 256;                 // threads per workgroup of the frame kernels
constexpr int FRAME_WAVES = FRAME_WG / 64;    // image (or grid) rows per workgroup

struct FrameCam {
  float fx, fy, cx, cy;
  int W, H;
};

struct FrameDet {          // what the kernels need of a dsr_frame_det
  int label;
  int bbox[4];
  int mode;                // DSR_FRAME_POSE_* (§3.5c; 0 = given for the plain frame calls)
};

// sel(i, n, N): index i of n evenly spread over [0, N-1] — np.linspace(0, N-1, n).astype(int32)
// made exact (64-bit integers; i < n <= N < 2^31)
__host__ __device__ __forceinline__ long long frame_sel(long long i, long long n, long long N) {
  return n >= 2 ? (i * (N - 1)) / (n - 1) : 0;
}
// ... applied only when N > n
__host__ __device__ __forceinline__ long long frame_pick(long long i, long long n, long long N) {
  return N > n ? frame_sel(i, n, N) : i;
}
// the inverse, for element p of N: the output row that picks it, or -1 if none does
__host__ __device__ __forceinline__ long long frame_row_of(long long p, long long n, long long N) {
  if (N <= n) return p;
  if (n < 2) return p == 0 && n == 1 ? 0 : -1;
  const long long i = (p * (n - 1) + (N - 2)) / (N - 1);      // ceil(p (n-1) / (N-1))
  return frame_sel(i, n, N) == p ? i : -1;
}

// pixel (u, v) -> ray ((u - cx) / fx, (v - cy) / fy, 1): single correctly rounded fp32 operations
__host__ __device__ __forceinline__ void frame_ray(const FrameCam& C, int u, int v, float* rx, float* ry) {
  *rx = ((float)u - C.cx) / C.fx;
  *ry = ((float)v - C.cy) / C.fy;
}

__host__ __device__ __forceinline__ bool frame_valid(float z, float near, float far) { return z == z && z > near && z < far; }

// status, counts, expanded box and grid of one detection from its mask statistics (tight box
// tl, tt, tr, tb of the mask pixels; meaningless when n_mask == 0).  n_bg is left 0.
__host__ __device__ __forceinline__ void frame_finish(const FrameCam& C, const dsr_frame_params& P, const int* bbox,
                                             int n_mask, int n_valid, int tl, int tt, int tr, int tb,
                                             dsr_frame_det_out* o) {
  o->n_mask = n_mask;
  o->n_valid = n_valid;
  o->status = n_mask == 0 ? DSR_FRAME_NO_MASK
                          : n_mask <= P.min_mask_area ? DSR_FRAME_SMALL_MASK
                                                      : n_valid == 0 ? DSR_FRAME_NO_DEPTH : DSR_FRAME_OK;
  o->n_pts = o->status == DSR_FRAME_OK ? (n_valid < P.max_pts ? n_valid : P.max_pts) : 0;
  o->n_bg = 0;
  int l, t, r, b;
  bool have;
  if (bbox[2] >= bbox[0]) {                  // a given box, clamped to the image
    l = bbox[0] > 0 ? bbox[0] : 0;
    t = bbox[1] > 0 ? bbox[1] : 0;
    r = bbox[2] < C.W - 1 ? bbox[2] : C.W - 1;
    b = bbox[3] < C.H - 1 ? bbox[3] : C.H - 1;
    have = l <= r && t <= b;
  } else {                                   // the tight box of the mask
    l = tl; t = tt; r = tr; b = tb;
    have = n_mask > 0;
  }
  if (!have) {
    o->box[0] = o->box[1] = 0;
    o->box[2] = o->box[3] = -1;
    o->grid_h = o->grid_w = 0;
    return;
  }
  const int e = P.expand;
  l = l > e ? l - e : 0;
  t = t > e ? t - e : 0;
  r = r < C.W - 1 - e ? r + e : C.W - 1;
  b = b < C.H - 1 - e ? b + e : C.H - 1;
  o->box[0] = l; o->box[1] = t; o->box[2] = r; o->box[3] = b;
  o->grid_h = (b - t + 1) / P.downsample;
  o->grid_w = (r - l + 1) / P.downsample;
}

// ---------------------------------------------------------------------------------------------
// host: the rule in plain C++ (dsr_frame_inputs_host)
inline void frame_inputs_host_impl(const FrameCam& C, const dsr_frame_params& P, const float* depth,
                                   const int* inst, int n_det, const dsr_frame_det* dets, float* pts, float* rays,
                                   float* dobs, dsr_frame_det_out* out) {
  std::vector<int> valid, cand;
  for (int d = 0; d < n_det; ++d) {
    const int label = dets[d].label;
    valid.clear();
    cand.clear();
    int n_mask = 0, tl = C.W, tt = C.H, tr = -1, tb = -1;
    for (int v = 0; v < C.H; ++v)
      for (int u = 0; u < C.W; ++u) {
        const size_t px = (size_t)v * C.W + u;
        if (inst[px] != label) continue;
        ++n_mask;
        tl = u < tl ? u : tl; tr = u > tr ? u : tr;
        tt = v < tt ? v : tt; tb = v > tb ? v : tb;
        if (frame_valid(depth[px], P.near, P.far)) valid.push_back((int)px);
      }
    dsr_frame_det_out o{};
    frame_finish(C, P, dets[d].bbox, n_mask, (int)valid.size(), tl, tt, tr, tb, &o);
    if (o.status == DSR_FRAME_OK) {
      float* p = pts ? pts + (size_t)d * P.max_pts * 3 : nullptr;
      float* r = rays ? rays + (size_t)d * ((size_t)P.max_pts + P.max_bg) * 3 : nullptr;
      float* z = dobs ? dobs + (size_t)d * P.max_pts : nullptr;
      const long long N = (long long)valid.size(), n = o.n_pts;
      for (long long i = 0; i < n; ++i) {
        const int px = valid[(size_t)frame_pick(i, n, N)];
        float rx, ry;
        frame_ray(C, px % C.W, px / C.W, &rx, &ry);
        const float zz = depth[px];
        if (r) { r[i * 3] = rx; r[i * 3 + 1] = ry; r[i * 3 + 2] = 1.f; }
        if (p) { p[i * 3] = rx * zz; p[i * 3 + 1] = ry * zz; p[i * 3 + 2] = zz; }
        if (z) z[i] = zz;
      }
      const int bh = o.box[3] - o.box[1] + 1, bw = o.box[2] - o.box[0] + 1;
      for (int j = 0; j < o.grid_h; ++j)
        for (int k = 0; k < o.grid_w; ++k) {
          const int v = o.box[1] + (int)frame_pick(j, o.grid_h, bh), u = o.box[0] + (int)frame_pick(k, o.grid_w, bw);
          const size_t px = (size_t)v * C.W + u;
          if (inst[px] != label) cand.push_back((int)px);
        }
      const long long NB = (long long)cand.size(), nb = NB < P.max_bg ? NB : P.max_bg;
      o.n_bg = (int)nb;
      for (long long i = 0; i < nb; ++i) {
        const int px = cand[(size_t)frame_pick(i, nb, NB)];
        float rx, ry;
        frame_ray(C, px % C.W, px / C.W, &rx, &ry);
        if (r) { r[(n + i) * 3] = rx; r[(n + i) * 3 + 1] = ry; r[(n + i) * 3 + 2] = 1.f; }
      }
    }
    if (out) out[d] = o;
  }
}

// ---------------------------------------------------------------------------------------------
// device

// Pass 1: per (image row, detection) the mask / valid counts and the row's first / last mask
// column.  grid = (ceil(H / FRAME_WAVES), n_det), one wave per row, lanes over 64-pixel chunks.
__global__ __launch_bounds__(FRAME_WG) void k_frame_rows(FrameCam C, dsr_frame_params P,
                                                         const float* __restrict__ depth,
                                                         const int* __restrict__ inst,
                                                         const FrameDet* __restrict__ dets, int4* __restrict__ rows) {
  const int lane = threadIdx.x & 63, v = blockIdx.x * FRAME_WAVES + (threadIdx.x >> 6), d = blockIdx.y;
  if (v >= C.H) return;
  const int label = dets[d].label;
  int nm = 0, nv = 0, umin = C.W, umax = -1;
  for (int c = 0; c < C.W; c += 64) {
    const int u = c + lane;
    bool m = false, ok = false;
    if (u < C.W) {
      const size_t px = (size_t)v * C.W + u;
      m = inst[px] == label;
      ok = m && frame_valid(depth[px], P.near, P.far);
    }
    const unsigned long long mb = __ballot(m), vb = __ballot(ok);
    nm += __popcll(mb);
    nv += __popcll(vb);
    if (mb) {
      const int first = c + (__ffsll((long long)mb) - 1), last = c + 63 - __clzll((long long)mb);
      umin = first < umin ? first : umin;
      umax = last > umax ? last : umax;
    }
  }
  if (lane == 0) rows[(size_t)d * C.H + v] = make_int4(nm, nv, umin, umax);
}

// exclusive scan of a[0 .. n) in place by one workgroup (thread t owns a contiguous run of
// elements); returns the total to every thread.  sh: FRAME_WG ints
__device__ inline int frame_block_scan(int* __restrict__ a, int n, int* sh) {
  const int t = threadIdx.x, per = (n + FRAME_WG - 1) / FRAME_WG;
  const int i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
  int s = 0;
  for (int i = i0; i < i1; ++i) s += a[i];
  __syncthreads();                       // sh may still be read from an earlier use
  sh[t] = s;
  __syncthreads();
  int base = 0, total = 0;
  for (int k = 0; k < FRAME_WG; ++k) {   // 256 LDS broadcasts: this kernel is one workgroup per detection
    const int x = sh[k];
    base += k < t ? x : 0;
    total += x;
  }
  for (int i = i0; i < i1; ++i) {
    const int x = a[i];
    a[i] = base;
    base += x;
  }
  return total;
}

// Pass 2: one workgroup per detection — the row scan (voff), the mask totals and tight box, the
// status / expanded box / grid (frame_finish), the background candidates per grid row and their
// scan (bgoff), the record, and (desc != null) the slot's ObjDesc counts.
__global__ __launch_bounds__(FRAME_WG) void k_frame_scan(FrameCam C, dsr_frame_params P,
                                                         const int* __restrict__ inst,
                                                         const FrameDet* __restrict__ dets,
                                                         const int4* __restrict__ rows, int* __restrict__ voff,
                                                         int* __restrict__ bgoff, int* __restrict__ aux,
                                                         dsr_frame_det_out* __restrict__ recs,
                                                         ObjDesc* __restrict__ desc) {
  __shared__ int sh[FRAME_WG];
  __shared__ int red[5][FRAME_WG];
  __shared__ dsr_frame_det_out rec;
  const int d = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int4* row = rows + (size_t)d * C.H;
  int* vo = voff + (size_t)d * C.H;
  int* bo = bgoff + (size_t)d * C.H;
  int nm = 0, tl = C.W, tt = C.H, tr = -1, tb = -1;
  for (int v = t; v < C.H; v += FRAME_WG) {
    const int4 r = row[v];
    vo[v] = r.y;
    nm += r.x;
    if (r.x > 0) {
      tl = r.z < tl ? r.z : tl;
      tr = r.w > tr ? r.w : tr;
      tt = v < tt ? v : tt;
      tb = v > tb ? v : tb;
    }
  }
  red[0][t] = nm; red[1][t] = tl; red[2][t] = tt; red[3][t] = tr; red[4][t] = tb;
  __syncthreads();                       // vo[] and red[] written
  const int n_valid = frame_block_scan(vo, C.H, sh);
  if (t == 0) {
    for (int k = 1; k < FRAME_WG; ++k) {
      nm += red[0][k];
      tl = red[1][k] < tl ? red[1][k] : tl;
      tt = red[2][k] < tt ? red[2][k] : tt;
      tr = red[3][k] > tr ? red[3][k] : tr;
      tb = red[4][k] > tb ? red[4][k] : tb;
    }
    dsr_frame_det_out o;
    frame_finish(C, P, dets[d].bbox, nm, n_valid, tl, tt, tr, tb, &o);
    rec = o;
  }
  __syncthreads();
  const int gh = rec.status == DSR_FRAME_OK && P.max_bg > 0 ? rec.grid_h : 0, gw = rec.grid_w;
  const int bl = rec.box[0], bt = rec.box[1], bw = rec.box[2] - rec.box[0] + 1, bh = rec.box[3] - rec.box[1] + 1;
  const int label = dets[d].label;
  for (int j = wave; j < gh; j += FRAME_WAVES) {            // gh <= H: bo[] holds it
    const int v = bt + (int)frame_pick(j, gh, bh);
    int n = 0;
    for (int c = 0; c < gw; c += 64) {
      const int k = c + lane;
      bool cand = false;
      if (k < gw) cand = inst[(size_t)v * C.W + bl + (int)frame_pick(k, gw, bw)] != label;
      n += __popcll(__ballot(cand));
    }
    if (lane == 0) bo[j] = n;
  }
  __syncthreads();
  const int NB = frame_block_scan(bo, gh, sh);
  if (t == 0) {
    dsr_frame_det_out o = rec;
    o.n_bg = NB < P.max_bg ? NB : P.max_bg;
    recs[d] = o;
    aux[d] = NB;
    if (desc) {
      desc[d].n_pts = o.n_pts;
      desc[d].n_rays = o.n_pts + o.n_bg;
      desc[d].n_fg = o.n_pts;
    }
  }
}

// Pass 3: every valid pixel (blockIdx.z == 0) and every background candidate (== 1) finds the
// output row that picks it (frame_row_of) and writes it: no search, no atomics.  grid =
// (ceil(H / FRAME_WAVES), n_det, 2), one wave per image / grid row.  Outputs go to the slots of
// desc (a capacity batch) or, desc == null, to fixed strides per detection (max_pts x 3,
// (max_pts + max_bg) x 3, max_pts); only a batch's dobs has rows for the background rays (0).
// RAYS = false (the tracker, dsr_track.hpp): the surface points alone, through desc's pts_off —
// launched without the background z-slice; rays, dobs, bgoff and aux are not read.
template <bool RAYS>
__global__ __launch_bounds__(FRAME_WG) DSR_NO_PK_F32 void k_frame_emit(FrameCam C, dsr_frame_params P,
                                                         const float* __restrict__ depth,
                                                         const int* __restrict__ inst,
                                                         const FrameDet* __restrict__ dets,
                                                         const int4* __restrict__ rows,
                                                         const int* __restrict__ voff, const int* __restrict__ bgoff,
                                                         const int* __restrict__ aux,
                                                         const dsr_frame_det_out* __restrict__ recs,
                                                         const ObjDesc* __restrict__ desc, float* __restrict__ pts,
                                                         float* __restrict__ rays, float* __restrict__ dobs) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * FRAME_WAVES + (threadIdx.x >> 6), d = blockIdx.y;
  const dsr_frame_det_out& rec = recs[d];
  if (rec.status != DSR_FRAME_OK) return;
  float *op, *orr = nullptr, *oz = nullptr;
  if (desc) {
    op = pts + (size_t)desc[d].pts_off * 3;
    if constexpr (RAYS) {
      orr = rays + (size_t)desc[d].ray_off * 3;
      oz = dobs + desc[d].ray_off;
    }
  } else {
    op = pts + (size_t)d * P.max_pts * 3;
    if constexpr (RAYS) {
      orr = rays + (size_t)d * ((size_t)P.max_pts + P.max_bg) * 3;
      oz = dobs + (size_t)d * P.max_pts;
    }
  }
  const int label = dets[d].label;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  if (blockIdx.z == 0) {
    const int v = j;
    if (v >= C.H) return;
    if (rows[(size_t)d * C.H + v].y == 0) return;
    const long long N = rec.n_valid, n = rec.n_pts;
    long long base = voff[(size_t)d * C.H + v];
    for (int c = 0; c < C.W; c += 64) {
      const int u = c + lane;
      bool ok = false;
      float z = 0.f;
      if (u < C.W) {
        const size_t px = (size_t)v * C.W + u;
        z = depth[px];
        ok = inst[px] == label && frame_valid(z, P.near, P.far);
      }
      const unsigned long long vb = __ballot(ok);
      if (ok) {
        const long long i = frame_row_of(base + __popcll(vb & below), n, N);
        if (i >= 0 && i < n) {
          float rx, ry;
          frame_ray(C, u, v, &rx, &ry);
          if constexpr (RAYS) {
            orr[i * 3] = rx; orr[i * 3 + 1] = ry; orr[i * 3 + 2] = 1.f;
          }
          op[i * 3] = rx * z; op[i * 3 + 1] = ry * z; op[i * 3 + 2] = z;
          if constexpr (RAYS) oz[i] = z;
        }
      }
      base += __popcll(vb);
    }
  } else if constexpr (RAYS) {
    const int gh = P.max_bg > 0 ? rec.grid_h : 0, gw = rec.grid_w;
    if (j >= gh) return;
    const int bl = rec.box[0], bt = rec.box[1], bw = rec.box[2] - rec.box[0] + 1, bh = rec.box[3] - rec.box[1] + 1;
    const long long N = aux[d], n = rec.n_bg, n_fg = rec.n_pts;
    const int v = bt + (int)frame_pick(j, gh, bh);
    long long base = bgoff[(size_t)d * C.H + j];
    for (int c = 0; c < gw; c += 64) {
      const int k = c + lane;
      bool cand = false;
      int u = 0;
      if (k < gw) {
        u = bl + (int)frame_pick(k, gw, bw);
        cand = inst[(size_t)v * C.W + u] != label;
      }
      const unsigned long long cb = __ballot(cand);
      if (cand) {
        const long long i = frame_row_of(base + __popcll(cb & below), n, N);
        if (i >= 0 && i < n) {
          float rx, ry;
          frame_ray(C, u, v, &rx, &ry);
          const long long r = n_fg + i;
          orr[r * 3] = rx; orr[r * 3 + 1] = ry; orr[r * 3 + 2] = 1.f;
          if (desc) oz[r] = 0.f;
        }
      }
      base += __popcll(cb);
    }
  }
}

// the device buffers of one frame call, carved from one block (256 B aligned parts)
struct FrameDev {
  float* depth;
  int* inst;
  FrameDet* dets;
  int4* rows;
  int *voff, *bgoff, *aux;
  dsr_frame_det_out* recs;
};
inline size_t frame_up256(size_t b) { return (b + 255) & ~(size_t)255; }
// bytes of the uploaded part (depth | inst | dets) and of the whole block
inline size_t frame_upload_bytes(int W, int H, int n_det) {
  return 2 * frame_up256((size_t)W * H * 4) + frame_up256(sizeof(FrameDet) * (size_t)(n_det > 0 ? n_det : 1));
}
inline size_t frame_dev_bytes(int W, int H, int n_det) {
  const size_t nd = (size_t)(n_det > 0 ? n_det : 1);
  return frame_upload_bytes(W, H, n_det) + frame_up256(nd * H * sizeof(int4)) + 2 * frame_up256(nd * H * sizeof(int)) +
         frame_up256(nd * sizeof(int)) + frame_up256(nd * sizeof(dsr_frame_det_out));
}
inline FrameDev frame_carve(void* block, int W, int H, int n_det) {
  const size_t nd = (size_t)(n_det > 0 ? n_det : 1);
  char* p = static_cast<char*>(block);
  FrameDev D;
  D.depth = reinterpret_cast<float*>(p); p += frame_up256((size_t)W * H * 4);
  D.inst = reinterpret_cast<int*>(p);    p += frame_up256((size_t)W * H * 4);
  D.dets = reinterpret_cast<FrameDet*>(p); p += frame_up256(sizeof(FrameDet) * nd);
  D.rows = reinterpret_cast<int4*>(p);   p += frame_up256(nd * H * sizeof(int4));
  D.voff = reinterpret_cast<int*>(p);    p += frame_up256(nd * H * sizeof(int));
  D.bgoff = reinterpret_cast<int*>(p);   p += frame_up256(nd * H * sizeof(int));
  D.aux = reinterpret_cast<int*>(p);     p += frame_up256(nd * sizeof(int));
  D.recs = reinterpret_cast<dsr_frame_det_out*>(p);
  return D;
}

// the three passes on stream s (n_det > 0); D.depth / inst / dets are already enqueued uploads
inline void frame_launch(hipStream_t s, const FrameCam& C, const dsr_frame_params& P, int n_det, const FrameDev& D,
                         ObjDesc* desc, float* pts, float* rays, float* dobs) {
  const unsigned gy = (unsigned)((C.H + FRAME_WAVES - 1) / FRAME_WAVES);
  hipLaunchKernelGGL(k_frame_rows, dim3(gy, n_det), dim3(FRAME_WG), 0, s, C, P, (const float*)D.depth,
                     (const int*)D.inst, (const FrameDet*)D.dets, D.rows);
  hipLaunchKernelGGL(k_frame_scan, dim3(n_det), dim3(FRAME_WG), 0, s, C, P, (const int*)D.inst,
                     (const FrameDet*)D.dets, (const int4*)D.rows, D.voff, D.bgoff, D.aux, D.recs, desc);
  hipLaunchKernelGGL(k_frame_emit<true>, dim3(gy, n_det, 2), dim3(FRAME_WG), 0, s, C, P, (const float*)D.depth,
                     (const int*)D.inst, (const FrameDet*)D.dets, (const int4*)D.rows, (const int*)D.voff,
                     (const int*)D.bgoff, (const int*)D.aux, (const dsr_frame_det_out*)D.recs,
                     (const ObjDesc*)desc, pts, rays, dobs);
}

// ---------------------------------------------------------------------------------------------
// Cuboid start poses and outlier removal (MapObject::RemoveOutliersSimple and
// ComputeCuboidPCA_onlyformono, src/MapObject.cc:249-283, :330-443).  fp64 on the fp32 rows, every
// operation rounded on its own (no contraction: the pragma below, on both sides), sums in one
// fixed shape: partial j < FRAME_WG adds the terms of points j, j + FRAME_WG, ... in that order
// from 0, then the partials are added in index order.  The functions are shared by the host twin
// and the kernels.
#define DSR_FP_STRICT _Pragma("clang fp contract(off)")

struct FramePoseFit {
  double eig[3];     // ascending
  double R[9];       // row-major, columns x (v1), y (v0), z (-v2)
  double dims[3];    // w, h, l
  double co[3];      // centre in the cuboid's axes
  double cc[3];      // centre in the camera frame
};

__host__ __device__ __forceinline__ bool frame_fin(double x) { return x - x == 0.0; }   // false for NaN, +-inf
__host__ __device__ __forceinline__ double frame_abs(double x) { return x < 0.0 ? -x : x; }

// pass 1: |P - m0|^2 <= r2, the sum taken left to right
__host__ __device__ __forceinline__ bool frame_pose_near(const float* p, const double* m0, double r2) {
  DSR_FP_STRICT
  const double dx = (double)p[0] - m0[0], dy = (double)p[1] - m0[1], dz = (double)p[2] - m0[2];
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return xx + yy + zz <= r2;
}

// the six terms of (P - m1)(P - m1)^T: xx, xy, xz, yy, yz, zz
__host__ __device__ __forceinline__ void frame_pose_terms(const float* p, const double* m1, double* t) {
  DSR_FP_STRICT
  const double dx = (double)p[0] - m1[0], dy = (double)p[1] - m1[1], dz = (double)p[2] - m1[2];
  t[0] = dx * dx; t[1] = dx * dy; t[2] = dx * dz; t[3] = dy * dy; t[4] = dy * dz; t[5] = dz * dz;
}

// one Jacobi rotation's update of a pair of values
__host__ __device__ __forceinline__ void frame_rot(double c, double s, double* x, double* y) {
  DSR_FP_STRICT
  const double a = *x, b = *y;
  const double ca = c * a, sb = s * b, sa = s * a, cb = c * b;
  *x = ca - sb;
  *y = sa + cb;
}

// one Jacobi step on the pair (P_, Q_): indices are compile-time so that A and V stay in registers
template <int P_, int Q_>
__host__ __device__ __forceinline__ void frame_jacobi_pair(double (&A)[3][3], double (&V)[3][3]) {
  DSR_FP_STRICT
  const double apq = A[P_][Q_];
  if (apq == 0.0) return;
  const double diff = A[Q_][Q_] - A[P_][P_];
  const double two = 2.0 * apq;
  const double theta = diff / two;
  const double th2 = theta * theta;
  const double rad = sqrt(th2 + 1.0);
  double t = 1.0 / (frame_abs(theta) + rad);
  if (theta < 0.0) t = -t;
  const double t2 = t * t;
  const double c = 1.0 / sqrt(t2 + 1.0);
  const double s = t * c;
  frame_rot(c, s, &A[0][P_], &A[0][Q_]);
  frame_rot(c, s, &A[1][P_], &A[1][Q_]);
  frame_rot(c, s, &A[2][P_], &A[2][Q_]);
  frame_rot(c, s, &A[P_][0], &A[Q_][0]);
  frame_rot(c, s, &A[P_][1], &A[Q_][1]);
  frame_rot(c, s, &A[P_][2], &A[Q_][2]);
  frame_rot(c, s, &V[0][P_], &V[0][Q_]);
  frame_rot(c, s, &V[1][P_], &V[1][Q_]);
  frame_rot(c, s, &V[2][P_], &V[2][Q_]);
}
__host__ __device__ __forceinline__ double frame_pick3(int i, double a, double b, double c) { return i == 0 ? a : i == 1 ? b : c; }

// scatter matrix C (xx, xy, xz, yy, yz, zz) -> ascending eigenvalues and the axes R: 10 cyclic
// Jacobi sweeps, ascending order with ties by index, canonical sign of v2, R = [v1 | v0 | -v2],
// det and up corrections (MapObject.cc:363-385)
__host__ __device__ __forceinline__ void frame_pose_axes(const double* C, const float* up, double* eig, double* R) {
  DSR_FP_STRICT
  double A[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
  double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < 10; ++sweep) {
    frame_jacobi_pair<0, 1>(A, V);
    frame_jacobi_pair<0, 2>(A, V);
    frame_jacobi_pair<1, 2>(A, V);
  }
  const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
  int i0 = 0, i1 = 1, i2 = 2;                // insertion sort, strict >: ascending, ties by index
  if (d0 > d1) { i0 = 1; i1 = 0; }
  if (frame_pick3(i1, d0, d1, d2) > d2) {
    i2 = i1;
    i1 = 2;
    if (frame_pick3(i0, d0, d1, d2) > d2) { i1 = i0; i0 = 2; }
  }
  eig[0] = frame_pick3(i0, d0, d1, d2);
  eig[1] = frame_pick3(i1, d0, d1, d2);
  eig[2] = frame_pick3(i2, d0, d1, d2);
  double v0[3], v1[3], v2[3];                // the eigenvectors
  v0[0] = frame_pick3(i0, V[0][0], V[0][1], V[0][2]); v0[1] = frame_pick3(i0, V[1][0], V[1][1], V[1][2]); v0[2] = frame_pick3(i0, V[2][0], V[2][1], V[2][2]);
  v1[0] = frame_pick3(i1, V[0][0], V[0][1], V[0][2]); v1[1] = frame_pick3(i1, V[1][0], V[1][1], V[1][2]); v1[2] = frame_pick3(i1, V[2][0], V[2][1], V[2][2]);
  v2[0] = frame_pick3(i2, V[0][0], V[0][1], V[0][2]); v2[1] = frame_pick3(i2, V[1][0], V[1][1], V[1][2]); v2[2] = frame_pick3(i2, V[2][0], V[2][1], V[2][2]);
  double lead = v2[0];                       // canonical sign of v2: its component of largest magnitude
  if (frame_abs(v2[1]) > frame_abs(lead)) lead = v2[1];
  if (frame_abs(v2[2]) > frame_abs(lead)) lead = v2[2];
  const bool neg = lead < 0.0;
  R[0] = v1[0]; R[1] = v0[0]; R[2] = neg ? v2[0] : -v2[0];
  R[3] = v1[1]; R[4] = v0[1]; R[5] = neg ? v2[1] : -v2[1];
  R[6] = v1[2]; R[7] = v0[2]; R[8] = neg ? v2[2] : -v2[2];
  const double m0 = R[4] * R[8], m1 = R[5] * R[7], m2 = R[3] * R[8], m3 = R[5] * R[6], m4 = R[3] * R[7],
               m5 = R[4] * R[6];
  const double c0 = R[0] * (m0 - m1), c1 = R[1] * (m2 - m3), c2 = R[2] * (m4 - m5);
  const double det = c0 - c1 + c2;
  if (det < 0.0)
    for (int r = 0; r < 3; ++r) R[r * 3] = -R[r * 3];
  const double u0 = (double)up[0] * R[1], u1 = (double)up[1] * R[4], u2 = (double)up[2] * R[7];
  if (u0 + u1 + u2 < 0.0)
    for (int r = 0; r < 3; ++r) {
      R[r * 3] = -R[r * 3];
      R[r * 3 + 1] = -R[r * 3 + 1];
    }
}

// q = R^T P, each component a left-to-right sum of three products; -0 is taken as +0 so that
// equal values have equal bits
__host__ __device__ __forceinline__ void frame_pose_q(const double* R, const float* p, double* q) {
  DSR_FP_STRICT
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double t0 = R[a] * x, t1 = R[3 + a] * y, t2 = R[6 + a] * z;
    q[a] = (t0 + t1 + t2) + 0.0;
  }
}

// monotone 64-bit keys of doubles (the radix select's order) and back
__host__ __device__ __forceinline__ unsigned long long frame_key(double x) {
  unsigned long long u;
  __builtin_memcpy(&u, &x, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double frame_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}

// extents from the order statistics; false when degenerate (l == 0 or a non-finite value)
__host__ __device__ __forceinline__ bool frame_pose_extents(const double* qlo, const double* qhi, FramePoseFit* f) {
  DSR_FP_STRICT
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    f->dims[a] = qhi[a] - qlo[a];
    f->co[a] = (qhi[a] + qlo[a]) / 2.0;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double t0 = f->R[k * 3] * f->co[0], t1 = f->R[k * 3 + 1] * f->co[1], t2 = f->R[k * 3 + 2] * f->co[2];
    f->cc[k] = t0 + t1 + t2;
  }
  bool ok = !(f->dims[2] == 0.0);
#pragma unroll
  for (int k = 0; k < 3; ++k) ok = ok && frame_fin(f->eig[k]) && frame_fin(f->dims[k]) && frame_fin(f->co[k]) && frame_fin(f->cc[k]);
  for (int k = 0; k < 9; ++k) ok = ok && frame_fin(f->R[k]);
  return ok;
}

// pass 2: |q_a - co_a| > margin dims_a / 2 on some axis (a comparison with NaN is false)
__host__ __device__ __forceinline__ void frame_pose_half(float margin, const double* dims, double* half) {
  DSR_FP_STRICT
#pragma unroll
  for (int a = 0; a < 3; ++a) half[a] = ((double)margin * dims[a]) / 2.0;
}
__host__ __device__ __forceinline__ bool frame_pose_outlier(const double* q, const double* co, const double* half) {
  DSR_FP_STRICT
  bool out = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) out = out || frame_abs(q[a] - co[a]) > half[a];
  return out;
}

// t_cam_obj = [scale_factor l R | cc; 0 0 0 1], each entry rounded once to fp32; flipped: columns
// 0 and 2 of the fp32 matrix negated (flipped_Two, LocalMapping_util.cc:402-404)
__host__ __device__ __forceinline__ void frame_pose_matrix(float scale_factor, const FramePoseFit& f, bool flipped, float* T) {
  DSR_FP_STRICT
  const double sl = (double)scale_factor * f.dims[2];
  for (int k = 0; k < 3; ++k) {
    for (int j = 0; j < 3; ++j) {
      const float x = (float)(sl * f.R[k * 3 + j]);
      T[k * 4 + j] = flipped && j != 1 ? -x : x;
    }
    T[k * 4 + 3] = (float)f.cc[k];
  }
  T[12] = T[13] = T[14] = 0.f;
  T[15] = 1.f;
}
__host__ __device__ __forceinline__ void frame_pose_identity(float* T) {
  for (int i = 0; i < 16; ++i) T[i] = i % 5 == 0 ? 1.f : 0.f;
}
__host__ __device__ __forceinline__ void frame_pose_blank(dsr_frame_pose_out* o, int status, int n_in) {
  o->status = status;
  o->n_in = n_in;
  o->n_near = o->n_kept = 0;
  for (int k = 0; k < 3; ++k) o->dims[k] = o->eig[k] = 0.0;
  frame_pose_identity(o->t_cam_obj);
}
__host__ __device__ __forceinline__ long long frame_pose_rank(long long n, int pct) { return (n * pct) / 100; }

// host: the rule on one detection's ingested rows (p: n_in x 3, z: n_in, r: (n_in + n_bg) x 3),
// compacted in place.  rec->status / n_in / t_cam_obj are set by the caller for the modes that
// do not run it.
inline void frame_pose_host_one(const dsr_frame_pose_params& Q, bool flipped, int n_in, int n_bg, float* p, float* r,
                                float* z, dsr_frame_pose_out* rec) {
  DSR_FP_STRICT
  frame_pose_blank(rec, DSR_FRAME_POSE_FEW_POINTS, n_in);
  double part[6][FRAME_WG];
  auto total = [&](int k) {
    double s = 0.0;
    for (int j = 0; j < FRAME_WG; ++j) s = s + part[k][j];
    return s;
  };
  auto clear = [&](int n) {
    for (int k = 0; k < n; ++k)
      for (int j = 0; j < FRAME_WG; ++j) part[k][j] = 0.0;
  };
  clear(3);
  for (int i = 0; i < n_in; ++i)
    for (int k = 0; k < 3; ++k) part[k][i % FRAME_WG] = part[k][i % FRAME_WG] + (double)p[i * 3 + k];
  double m0[3], m1[3];
  for (int k = 0; k < 3; ++k) m0[k] = total(k) / (double)n_in;
  const double r2 = (double)Q.outlier_radius * (double)Q.outlier_radius;
  std::vector<unsigned char> keep((size_t)n_in);
  int n_near = 0;
  for (int i = 0; i < n_in; ++i) n_near += keep[i] = frame_pose_near(p + i * 3, m0, r2) ? 1 : 0;
  rec->n_near = n_near;
  if (n_in < Q.min_points || n_near < Q.min_points) return;
  clear(3);
  for (int i = 0; i < n_in; ++i)
    if (keep[i])
      for (int k = 0; k < 3; ++k) part[k][i % FRAME_WG] = part[k][i % FRAME_WG] + (double)p[i * 3 + k];
  for (int k = 0; k < 3; ++k) m1[k] = total(k) / (double)n_near;
  clear(6);
  for (int i = 0; i < n_in; ++i)
    if (keep[i]) {
      double t[6];
      frame_pose_terms(p + i * 3, m1, t);
      for (int k = 0; k < 6; ++k) part[k][i % FRAME_WG] = part[k][i % FRAME_WG] + t[k];
    }
  double C[6];
  for (int k = 0; k < 6; ++k) C[k] = total(k);
  FramePoseFit f;
  frame_pose_axes(C, Q.up, f.eig, f.R);
  for (int k = 0; k < 3; ++k) rec->eig[k] = f.eig[k];
  std::vector<double> qa[3];
  for (int i = 0; i < n_in; ++i)
    if (keep[i]) {
      double q[3];
      frame_pose_q(f.R, p + i * 3, q);
      for (int a = 0; a < 3; ++a) qa[a].push_back(q[a]);
    }
  const size_t lo = (size_t)frame_pose_rank(n_near, Q.lo_pct), hi = (size_t)frame_pose_rank(n_near, Q.hi_pct);
  double qlo[3], qhi[3];
  for (int a = 0; a < 3; ++a) {              // order statistics by their keys: exact, NaN included
    std::vector<unsigned long long> key(qa[a].size());
    for (size_t i = 0; i < key.size(); ++i) key[i] = frame_key(qa[a][i]);
    std::nth_element(key.begin(), key.begin() + lo, key.end());
    qlo[a] = frame_unkey(key[lo]);
    std::nth_element(key.begin(), key.begin() + hi, key.end());
    qhi[a] = frame_unkey(key[hi]);
  }
  const bool ok = frame_pose_extents(qlo, qhi, &f);
  for (int k = 0; k < 3; ++k) rec->dims[k] = f.dims[k];
  if (!ok) {
    rec->status = DSR_FRAME_POSE_DEGENERATE;
    return;
  }
  double half[3];
  frame_pose_half(Q.box_margin, f.dims, half);
  int n_kept = 0;
  for (int i = 0; i < n_in; ++i)
    if (keep[i]) {
      double q[3];
      frame_pose_q(f.R, p + i * 3, q);
      n_kept += keep[i] = frame_pose_outlier(q, f.co, half) ? 0 : 1;
    }
  rec->n_kept = n_kept;
  if (n_kept < Q.min_points) return;
  rec->status = DSR_FRAME_POSE_OK;
  frame_pose_matrix(Q.scale_factor, f, flipped, rec->t_cam_obj);
  int w = 0;                                 // ordered compaction in place (w <= i)
  for (int i = 0; i < n_in; ++i)
    if (keep[i]) {
      if (w != i) {
        for (int k = 0; k < 3; ++k) {
          p[w * 3 + k] = p[i * 3 + k];
          r[w * 3 + k] = r[i * 3 + k];
        }
        z[w] = z[i];
      }
      ++w;
    }
  if (n_kept != n_in)
    for (int i = 0; i < n_bg; ++i)
      for (int k = 0; k < 3; ++k) r[((size_t)n_kept + i) * 3 + k] = r[((size_t)n_in + i) * 3 + k];
}

// host: ingest plus the rule (dsr_frame_poses_host)
inline void frame_poses_host_impl(const FrameCam& C, const dsr_frame_params& P, const dsr_frame_pose_params& Q,
                                  const float* depth, const int* inst, int n_det, const dsr_frame_det* dets,
                                  const int* modes, float* pts, float* rays, float* dobs, dsr_frame_det_out* out,
                                  dsr_frame_pose_out* pose_out) {
  frame_inputs_host_impl(C, P, depth, inst, n_det, dets, pts, rays, dobs, out);
  for (int d = 0; d < n_det; ++d) {
    dsr_frame_pose_out* rec = pose_out + d;
    if (modes[d] == DSR_FRAME_POSE_GIVEN) {
      frame_pose_blank(rec, DSR_FRAME_POSE_NOT_ASKED, out[d].n_pts);
      for (int i = 0; i < 16; ++i) rec->t_cam_obj[i] = dets[d].t_cam_obj[i];
    } else if (out[d].status != DSR_FRAME_OK) {
      frame_pose_blank(rec, DSR_FRAME_POSE_NO_INPUT, 0);
    } else {
      frame_pose_host_one(Q, modes[d] == DSR_FRAME_POSE_CUBOID_FLIPPED, out[d].n_pts, out[d].n_bg,
                          pts + (size_t)d * P.max_pts * 3, rays + (size_t)d * ((size_t)P.max_pts + P.max_bg) * 3,
                          dobs + (size_t)d * P.max_pts, rec);
    }
  }
}

// device -----------------------------------------------------------------------------------
// the FRAME_WG partials of up to 6 sums -> their totals, each added in index order by one lane
// (lane k adds sum k); every thread gets all totals.  sh: [6][FRAME_WG], res: [6] (shared)
__device__ __forceinline__ void frame_block_sums(int n, const double* mine, double (*sh)[FRAME_WG], double* res, double* tot) {
  DSR_FP_STRICT
  const int t = threadIdx.x;
  __syncthreads();                           // sh / res may still be read from an earlier use
  for (int k = 0; k < n; ++k) sh[k][t] = mine[k];
  __syncthreads();
  if (t < n) {
    double s = 0.0;
    for (int j = 0; j < FRAME_WG; ++j) s = s + sh[t][j];
    res[t] = s;
  }
  __syncthreads();
  for (int k = 0; k < n; ++k) tot[k] = res[k];
}

// (one thread) the record, the pose row and the slot's counts: an empty object unless the status is OK
__device__ __forceinline__ void frame_pose_finish(const dsr_frame_pose_out& o, dsr_frame_pose_out* po, float* trow,
                                                  ObjDesc* slot, int n_bg) {
  *po = o;
  if (trow)
    for (int i = 0; i < 16; ++i) trow[i] = o.t_cam_obj[i];
  if (slot) {
    const int n = o.status == DSR_FRAME_POSE_OK ? o.n_kept : 0;
    slot->n_pts = n;
    slot->n_fg = n;
    slot->n_rays = o.status == DSR_FRAME_POSE_OK ? n + n_bg : 0;
  }
}

// One workgroup per detection, after k_frame_emit: the rule of §3.5c on the detection's rows —
// the strided sums (lane j is partial j), the pass-1 flags, C, Jacobi and axes on one lane, the
// projections, six order statistics by a radix select over the monotone keys (eight 8-bit passes,
// integer LDS histograms: order-independent), the pass-2 flags, then the record, the pose row
// t_in[d] (tin != null) and the slot's ObjDesc counts (desc != null).  keep[d][i] ends as 1 for a
// kept point.  Points are re-read from memory in every pass, so n_in is bounded by max_pts only.
__global__ __launch_bounds__(FRAME_WG) DSR_NO_PK_F32 void k_frame_pose(dsr_frame_params P, dsr_frame_pose_params Q,
                                                         const FrameDet* __restrict__ dets,
                                                         const dsr_frame_det_out* __restrict__ recs,
                                                         ObjDesc* __restrict__ desc, const float* __restrict__ pts,
                                                         unsigned char* __restrict__ keep_all,
                                                         dsr_frame_pose_out* __restrict__ precs,
                                                         float* __restrict__ tin) {
  DSR_FP_STRICT
  __shared__ double sh[6][FRAME_WG];
  __shared__ double res[6];
  __shared__ int hist[6][256];
  __shared__ unsigned long long pre[6];      // the keys' bits decided so far
  __shared__ int rank[6];                    // the rank still to find within them
  __shared__ int cnt[2];
  __shared__ FramePoseFit fit;
  __shared__ int verdict;                    // after the extents: 1 go on, 0 degenerate
  __shared__ dsr_frame_pose_out o;           // the record, written by thread 0
  const int d = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int mode = dets[d].mode;
  const dsr_frame_det_out& rec = recs[d];
  dsr_frame_pose_out* po = precs + d;
  float* trow = tin ? tin + (size_t)d * 16 : nullptr;
  if (mode == DSR_FRAME_POSE_GIVEN) {        // today's detection: nothing but the record
    if (t == 0) {
      frame_pose_blank(&o, DSR_FRAME_POSE_NOT_ASKED, rec.n_pts);
      if (trow)
        for (int i = 0; i < 16; ++i) o.t_cam_obj[i] = trow[i];
      *po = o;
    }
    return;
  }
  if (rec.status != DSR_FRAME_OK) {
    if (t == 0) {
      frame_pose_blank(&o, DSR_FRAME_POSE_NO_INPUT, 0);
      frame_pose_finish(o, po, trow, desc ? desc + d : nullptr, rec.n_bg);
    }
    return;
  }
  const int n_in = rec.n_pts;
  const float* p = desc ? pts + (size_t)desc[d].pts_off * 3 : pts + (size_t)d * P.max_pts * 3;
  unsigned char* keep = keep_all + (size_t)d * P.max_pts;
  if (t == 0) frame_pose_blank(&o, DSR_FRAME_POSE_FEW_POINTS, n_in);
  double mine[6], tot[6];
  // m0
  for (int k = 0; k < 3; ++k) mine[k] = 0.0;
  for (int i = t; i < n_in; i += FRAME_WG)
    for (int k = 0; k < 3; ++k) mine[k] = mine[k] + (double)p[(size_t)i * 3 + k];
  frame_block_sums(3, mine, sh, res, tot);
  double m0[3], m1[3];
  for (int k = 0; k < 3; ++k) m0[k] = tot[k] / (double)n_in;
  // pass 1
  const double r2 = (double)Q.outlier_radius * (double)Q.outlier_radius;
  if (t < 2) cnt[t] = 0;
  __syncthreads();
  int c = 0;
  for (int k = 0; k < 3; ++k) mine[k] = 0.0;
  for (int i = t; i < n_in; i += FRAME_WG) {
    const bool near = frame_pose_near(p + (size_t)i * 3, m0, r2);
    keep[i] = near ? 1 : 0;
    if (near) {
      ++c;
      for (int k = 0; k < 3; ++k) mine[k] = mine[k] + (double)p[(size_t)i * 3 + k];
    }
  }
  if (c) atomicAdd(&cnt[0], c);
  frame_block_sums(3, mine, sh, res, tot);    // (its barriers also publish cnt[0])
  const int n_near = cnt[0];
  if (n_in < Q.min_points || n_near < Q.min_points) {
    if (t == 0) {
      o.n_near = n_near;
      frame_pose_finish(o, po, trow, desc ? desc + d : nullptr, rec.n_bg);
    }
    return;
  }
  for (int k = 0; k < 3; ++k) m1[k] = tot[k] / (double)n_near;
  // C
  for (int k = 0; k < 6; ++k) mine[k] = 0.0;
  for (int i = t; i < n_in; i += FRAME_WG)
    if (keep[i]) {
      double x[6];
      frame_pose_terms(p + (size_t)i * 3, m1, x);
      for (int k = 0; k < 6; ++k) mine[k] = mine[k] + x[k];
    }
  frame_block_sums(6, mine, sh, res, tot);
  if (t == 0) {
    frame_pose_axes(tot, Q.up, fit.eig, fit.R);
    for (int s = 0; s < 6; ++s) {
      pre[s] = 0ull;
      rank[s] = (int)frame_pose_rank(n_near, (s & 1) ? Q.hi_pct : Q.lo_pct);
    }
  }
  __syncthreads();
  double R[9];
  for (int k = 0; k < 9; ++k) R[k] = fit.R[k];
  // six order statistics: selection s = 2 axis + (0 lo, 1 hi)
  for (int b = 7; b >= 0; --b) {
    for (int k = t; k < 6 * 256; k += FRAME_WG) (&hist[0][0])[k] = 0;
    __syncthreads();
    unsigned long long want[6];
    for (int s = 0; s < 6; ++s) want[s] = pre[s];
    for (int i = t; i < n_in; i += FRAME_WG)
      if (keep[i]) {
        double q[3];
        frame_pose_q(R, p + (size_t)i * 3, q);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const unsigned long long key = frame_key(q[a]);
          const int digit = (int)((key >> (8 * b)) & 255ull);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int s = 2 * a + h;
            if (b == 7 || ((key ^ want[s]) >> (8 * (b + 1))) == 0ull) atomicAdd(&hist[s][digit], 1);
          }
        }
      }
    __syncthreads();
    for (int s = wave; s < 6; s += FRAME_WAVES) {       // one wave per selection: lane l owns bins 4l .. 4l+3
      const int k = rank[s];
      const unsigned long long cur = pre[s];            // read by every lane before the one write below
      const int h0 = hist[s][4 * lane], h1 = hist[s][4 * lane + 1], h2 = hist[s][4 * lane + 2], h3 = hist[s][4 * lane + 3];
      const int sum = h0 + h1 + h2 + h3;
      int inc = sum;
      for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const int up = __shfl_up(inc, dlt, 64);
        if (lane >= dlt) inc += up;
      }
      const int exc = inc - sum;
      if (k >= exc && k < inc) {                        // exactly one lane: the counts sum to more than k
        int rem = k - exc, bin = 0;
        if (rem >= h0) { rem -= h0; bin = 1;
          if (rem >= h1) { rem -= h1; bin = 2;
            if (rem >= h2) { rem -= h2; bin = 3; } } }
        pre[s] = cur | ((unsigned long long)(4 * lane + bin) << (8 * b));
        rank[s] = rem;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    double qlo[3], qhi[3];
    for (int a = 0; a < 3; ++a) {
      qlo[a] = frame_unkey(pre[2 * a]);
      qhi[a] = frame_unkey(pre[2 * a + 1]);
    }
    verdict = frame_pose_extents(qlo, qhi, &fit) ? 1 : 0;
    o.n_near = n_near;
    for (int k = 0; k < 3; ++k) {
      o.eig[k] = fit.eig[k];
      o.dims[k] = fit.dims[k];
    }
  }
  __syncthreads();
  if (!verdict) {
    if (t == 0) {
      o.status = DSR_FRAME_POSE_DEGENERATE;
      frame_pose_finish(o, po, trow, desc ? desc + d : nullptr, rec.n_bg);
    }
    return;
  }
  // pass 2
  double half[3], co[3];
  frame_pose_half(Q.box_margin, fit.dims, half);
  for (int k = 0; k < 3; ++k) co[k] = fit.co[k];
  c = 0;
  for (int i = t; i < n_in; i += FRAME_WG)
    if (keep[i]) {
      double q[3];
      frame_pose_q(R, p + (size_t)i * 3, q);
      const bool out = frame_pose_outlier(q, co, half);
      if (out) keep[i] = 0;
      else ++c;
    }
  if (c) atomicAdd(&cnt[1], c);
  __syncthreads();
  if (t == 0) {
    o.n_kept = cnt[1];
    if (o.n_kept >= Q.min_points) {
      o.status = DSR_FRAME_POSE_OK;
      frame_pose_matrix(Q.scale_factor, fit, mode == DSR_FRAME_POSE_CUBOID_FLIPPED, o.t_cam_obj);
    }
    frame_pose_finish(o, po, trow, desc ? desc + d : nullptr, rec.n_bg);
  }
}

// One workgroup per detection, after k_frame_pose: ordered in-place compaction of the point,
// depth and foreground-ray rows by keep[], in ascending FRAME_WG-row chunks — a chunk is read
// into registers, __syncthreads(), then written; every destination is at or before the chunk's
// own start plus the thread's index, all of which has been read — then the background rays move
// down by n_in - n_kept the same way (a batch's dobs rows under them are 0).
__global__ __launch_bounds__(FRAME_WG) DSR_NO_PK_F32 void k_frame_compact(dsr_frame_params P,
                                                         const FrameDet* __restrict__ dets,
                                                         const dsr_frame_det_out* __restrict__ recs,
                                                         const ObjDesc* __restrict__ desc,
                                                         const unsigned char* __restrict__ keep_all,
                                                         const dsr_frame_pose_out* __restrict__ precs,
                                                         float* __restrict__ pts, float* __restrict__ rays,
                                                         float* __restrict__ dobs) {
  __shared__ int wsum[FRAME_WAVES];
  const int d = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (dets[d].mode == DSR_FRAME_POSE_GIVEN || precs[d].status != DSR_FRAME_POSE_OK) return;
  const int n_in = precs[d].n_in, n_kept = precs[d].n_kept, n_bg = recs[d].n_bg;
  if (n_kept == n_in) return;
  float *op, *orr, *oz;
  if (desc) {
    op = pts + (size_t)desc[d].pts_off * 3;
    orr = rays + (size_t)desc[d].ray_off * 3;
    oz = dobs + desc[d].ray_off;
  } else {
    op = pts + (size_t)d * P.max_pts * 3;
    orr = rays + (size_t)d * ((size_t)P.max_pts + P.max_bg) * 3;
    oz = dobs + (size_t)d * P.max_pts;
  }
  const unsigned char* keep = keep_all + (size_t)d * P.max_pts;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  int base = 0;
  for (int c0 = 0; c0 < n_in; c0 += FRAME_WG) {
    const int i = c0 + t;
    const bool f = i < n_in && keep[i] != 0;
    float px = 0.f, py = 0.f, pz = 0.f, rx = 0.f, ry = 0.f, rz = 0.f, z = 0.f;
    if (f) {
      px = op[(size_t)i * 3]; py = op[(size_t)i * 3 + 1]; pz = op[(size_t)i * 3 + 2];
      rx = orr[(size_t)i * 3]; ry = orr[(size_t)i * 3 + 1]; rz = orr[(size_t)i * 3 + 2];
      z = oz[i];
    }
    const unsigned long long fb = __ballot(f);
    if (lane == 0) wsum[wave] = __popcll(fb);
    __syncthreads();                         // the chunk is in registers, wsum[] written
    int off = base + __popcll(fb & below), all = 0;
    for (int w = 0; w < FRAME_WAVES; ++w) {
      off += w < wave ? wsum[w] : 0;
      all += wsum[w];
    }
    if (f) {                                 // off <= i
      op[(size_t)off * 3] = px; op[(size_t)off * 3 + 1] = py; op[(size_t)off * 3 + 2] = pz;
      orr[(size_t)off * 3] = rx; orr[(size_t)off * 3 + 1] = ry; orr[(size_t)off * 3 + 2] = rz;
      oz[off] = z;
    }
    base += all;
    __syncthreads();                         // wsum[] is rewritten by the next chunk
  }
  for (int c0 = 0; c0 < n_bg; c0 += FRAME_WG) {          // rows n_in + i -> n_kept + i
    const int i = c0 + t;
    float rx = 0.f, ry = 0.f, rz = 0.f;
    if (i < n_bg) {
      const size_t s = ((size_t)n_in + i) * 3;
      rx = orr[s]; ry = orr[s + 1]; rz = orr[s + 2];
    }
    __syncthreads();
    if (i < n_bg) {
      const size_t q = ((size_t)n_kept + i) * 3;
      orr[q] = rx; orr[q + 1] = ry; orr[q + 2] = rz;
      if (desc) oz[n_kept + i] = 0.f;
    }
  }
}

// the pose part of a frame block, after the frame_dev_bytes(W, H, n_det) of the ingest
struct FramePoseDev {
  unsigned char* keep;
  dsr_frame_pose_out* precs;
};
inline size_t frame_pose_dev_bytes(int n_det, int max_pts) {
  const size_t nd = (size_t)(n_det > 0 ? n_det : 1);
  return frame_up256(nd * (size_t)max_pts) + frame_up256(nd * sizeof(dsr_frame_pose_out));
}
inline FramePoseDev frame_pose_carve(void* block, int W, int H, int n_det, int max_pts) {
  const size_t nd = (size_t)(n_det > 0 ? n_det : 1);
  char* p = static_cast<char*>(block) + frame_dev_bytes(W, H, n_det);
  FramePoseDev D;
  D.keep = reinterpret_cast<unsigned char*>(p); p += frame_up256(nd * (size_t)max_pts);
  D.precs = reinterpret_cast<dsr_frame_pose_out*>(p);
  return D;
}

// the two kernels on stream s, after frame_launch (n_det > 0)
inline void frame_pose_launch(hipStream_t s, const dsr_frame_params& P, const dsr_frame_pose_params& Q, int n_det,
                              const FrameDev& D, const FramePoseDev& E, ObjDesc* desc, float* pts, float* rays,
                              float* dobs, float* tin) {
  hipLaunchKernelGGL(k_frame_pose, dim3(n_det), dim3(FRAME_WG), 0, s, P, Q, (const FrameDet*)D.dets,
                     (const dsr_frame_det_out*)D.recs, desc, (const float*)pts, E.keep, E.precs, tin);
  hipLaunchKernelGGL(k_frame_compact, dim3(n_det), dim3(FRAME_WG), 0, s, P, (const FrameDet*)D.dets,
                     (const dsr_frame_det_out*)D.recs, (const ObjDesc*)desc, (const unsigned char*)E.keep,
                     (const dsr_frame_pose_out*)E.precs, pts, rays, dobs);
}

// the parameter errors of the pose entry points (checked before the device is touched)
inline const char* frame_pose_args_error(const dsr_frame_pose_params* Q, int n_det, const int* modes) {
  if (!Q) return "frame poses: null pose parameters";
  if (n_det > 0 && !modes) return "frame poses: null modes";
  if (Q->min_points < 1) return "frame poses: min_points must be >= 1";
  if (!(0 <= Q->lo_pct && Q->lo_pct < Q->hi_pct && Q->hi_pct < 100)) return "frame poses: need 0 <= lo_pct < hi_pct < 100";
  if (!(Q->outlier_radius > 0.f)) return "frame poses: outlier_radius must be positive";
  if (!(Q->box_margin > 0.f)) return "frame poses: box_margin must be positive";
  if (!(Q->scale_factor > 0.f) || std::isinf(Q->scale_factor)) return "frame poses: scale_factor must be positive and finite";
  bool zero = true;
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(Q->up[k])) return "frame poses: up must be finite";
    zero = zero && Q->up[k] == 0.f;
  }
  if (zero) return "frame poses: up must not be zero";
  for (int d = 0; d < n_det; ++d)
    if (modes[d] != DSR_FRAME_POSE_GIVEN && modes[d] != DSR_FRAME_POSE_CUBOID && modes[d] != DSR_FRAME_POSE_CUBOID_FLIPPED)
      return "frame poses: unknown pose mode";
  return nullptr;
}

// the argument errors of the frame entry points (checked before the device is touched)
inline const char* frame_args_error(const dsr_camera* cam, const dsr_frame_params* P, const float* depth,
                                    const int* inst, int n_det, const dsr_frame_det* dets) {
  if (!cam || !P) return "frame: null camera or parameters";
  if (!depth || !inst) return "frame: null depth or instance image";
  if (cam->width <= 0 || cam->height <= 0) return "frame: image size must be positive";
  if ((long long)cam->width * cam->height > 0x7fffffffLL) return "frame: image larger than 2^31 - 1 pixels";
  if (!(cam->fx > 0.f) || !(cam->fy > 0.f)) return "frame: focal lengths must be positive";
  if (P->max_pts < 1) return "frame: max_pts must be >= 1";
  if (P->max_bg < 0) return "frame: max_bg must be >= 0";
  if (P->downsample < 1) return "frame: downsample must be >= 1";
  if (P->expand < 0) return "frame: expand must be >= 0";
  if (n_det < 0 || (n_det > 0 && !dets)) return "frame: n_det < 0 or null detections";
  return nullptr;
}

}  // namespace dsr
