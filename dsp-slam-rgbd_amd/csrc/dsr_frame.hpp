// dsr_frame.hpp — frame ingest (dsr_frame_inputs*, dsr_batch_refill_frame): one
// depth image + one instance-label image + a list of detections -> each detection's surface
// points, foreground / background rays and observed depths, laid out as dsr_object_in wants them.
// Replaces FrameWithLiDAR.get_detections / pixels_sampler (reconstruct/kitti_sequence.py:70-92,
// :139-146, :200-210), Frame.pixels_sampler (reconstruct/mono_sequence.py:51-73) and get_rays
// (reconstruct/loss_utils.py:23-37).
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
#pragma once
#include "../../include/dsr.h"
#include "dsr_dev.hpp"

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
          orr[i * 3] = rx; orr[i * 3 + 1] = ry; orr[i * 3 + 2] = 1.f;
          op[i * 3] = rx * z; op[i * 3 + 1] = ry * z; op[i * 3 + 2] = z;
          oz[i] = z;
        }
      }
      base += __popcll(vb);
    }
  } else {
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
  hipLaunchKernelGGL(k_frame_emit, dim3(gy, n_det, 2), dim3(FRAME_WG), 0, s, C, P, (const float*)D.depth,
                     (const int*)D.inst, (const FrameDet*)D.dets, (const int4*)D.rows, (const int*)D.voff,
                     (const int*)D.bgoff, (const int*)D.aux, (const dsr_frame_det_out*)D.recs,
                     (const ObjDesc*)desc, pts, rays, dobs);
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
