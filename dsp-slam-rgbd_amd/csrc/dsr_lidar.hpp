// dsr_lidar.hpp — LiDAR keyframe ingest (dsr_lidar_inputs*, dsr_batch_refill_lidar):
// one Velodyne sweep + the 3-D detector's boxes + one instance-label image and its mask list ->
// each detection's surface points, foreground / background rays, observed depths and start pose,
// laid out as dsr_object_in wants them.  Replaces FrameWithLiDAR.get_detections
// (reconstruct/kitti_sequence.py:99-216) with pixels_sampler (:70-92) and get_rays
// (reconstruct/loss_utils.py:23-37).
//
// The rule is stated once for both sides (lidar_prep on the host for both; lidar_test, lidar_q,
// lidar_project, lidar_finish and the frame ingest's frame_finish / frame_pick / frame_row_of /
// frame_ray are __host__ __device__); the host function walks it forwards (output row i -> its
// sweep point), the kernels backwards (every sweep point finds the row that picks it), so the two
// check each other.  Integer atomics only: the results do not depend on the order of execution.
//
// Device buffers of one call (n_velo points in n_chunks = ceil(n_velo / 64) chunks, H x W image,
// n_det detections):
//   cnt   [n_det][n_chunks] int   per chunk: near points | in points << 8
//   coff  [n_det][n_chunks] int   exclusive scan of the chunks' in points
//   hits  [n_det][256]      int   projected rows per mask-list entry
//   nproj [n_det]           int   projected rows
//   match [n_det]           LidarMatch  the matched entry's label and box
//   rows  [n_det][H]        int4  per image row: matched-label pixels, -, first / last column
//   bgoff [n_det][H]        int   per grid row: background candidates, then their exclusive scan
//   aux   [n_det]           int   N_bg (candidates before the max_bg cap)
//   recs  [n_det]           dsr_lidar_det_out
#pragma once
#include "dsr_frame.hpp"

namespace dsr {

constexpr int LIDAR_MAX_VELO = 1 << 24;
static_assert(DSR_LIDAR_MAX_MASKS <= FRAME_WG, "one thread per mask-list entry");

struct LidarDet {          // the host preparation of one dsr_lidar_det
  float lo[3], hi[3];      // the cube around trans
  float A[9], t[3];        // velodyne -> box axes
  float e[3];              // half extents (widened w, h, widened l)
  float tco[16];           // t_cam_obj
};
struct LidarXf {           // t_cam_velo, rows 0..2
  float c[12];
};
struct LidarMatch {        // the association's outcome, as the mask passes read it
  int label;
  int bbox[4];
  int mask;                // mask-list index, -1 unmatched
};

// fp64 on the fp32 inputs, every stored value rounded once; each fp64 operation rounded on its own
inline void lidar_prep(const dsr_lidar_params& P, const float* tcv, const dsr_lidar_det& d, LidarDet* L) {
  DSR_FP_STRICT
  const double th = (double)d.theta, c = std::cos(th), s = std::sin(th);
  const double R[3][3] = {{c, 0.0, -s}, {-s, 0.0, -c}, {0.0, 1.0, 0.0}};
  const double hh = (double)d.size[2] / 2.0;
  const double o[3] = {(double)d.trans[0], (double)d.trans[1], (double)d.trans[2] + hh};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) L->A[i * 3 + j] = (float)R[j][i];
  const double cx = c * o[0], sy = s * o[1], sx = s * o[0], cy = c * o[1];
  L->t[0] = (float)(-(cx - sy));
  L->t[1] = (float)(-o[2]);
  L->t[2] = (float)(sx + cy);
  const double m = (double)P.box_margin, r = (double)P.radius;
  for (int k = 0; k < 3; ++k) {
    L->lo[k] = (float)((double)d.trans[k] - r);
    L->hi[k] = (float)((double)d.trans[k] + r);
  }
  const double sigma = (m * (double)d.size[1]) / 2.0;
  L->e[0] = (float)((m * (double)d.size[0]) / 2.0);
  L->e[1] = (float)hh;
  L->e[2] = (float)sigma;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) {
        const double sr = sigma * R[k][j];
        const double term = (double)tcv[i * 4 + k] * sr;
        acc = acc + term;
      }
      L->tco[i * 4 + j] = (float)acc;
    }
    double acc = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double term = (double)tcv[i * 4 + k] * o[k];
      acc = acc + term;
    }
    L->tco[i * 4 + 3] = (float)(acc + (double)tcv[i * 4 + 3]);
  }
  L->tco[12] = L->tco[13] = L->tco[14] = 0.f;
  L->tco[15] = 1.f;
}

// 0: not near; 1: near; 3: near and in (strict inequalities; a NaN coordinate is in nothing)
__host__ __device__ __forceinline__ int lidar_test(const LidarDet& L, float px, float py, float pz) {
  const bool near = L.lo[0] < px && px < L.hi[0] && L.lo[1] < py && py < L.hi[1] && L.lo[2] < pz && pz < L.hi[2];
  if (!near) return 0;
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float x = __builtin_fmaf(L.A[k * 3], px, __builtin_fmaf(L.A[k * 3 + 1], py, __builtin_fmaf(L.A[k * 3 + 2], pz, L.t[k])));
    in = in && -L.e[k] < x && x < L.e[k];
  }
  return in ? 3 : 1;
}

// q = t_cam_velo p
__host__ __device__ __forceinline__ void lidar_q(const LidarXf& X, float px, float py, float pz, float* q) {
#pragma unroll
  for (int k = 0; k < 3; ++k)
    q[k] = __builtin_fmaf(X.c[k * 4], px, __builtin_fmaf(X.c[k * 4 + 1], py, __builtin_fmaf(X.c[k * 4 + 2], pz, X.c[k * 4 + 3])));
}

// the row's pixel, or false: q_z <= 0 (or NaN) or outside the open rectangle (0, W) x (0, H)
__host__ __device__ __forceinline__ bool lidar_project(const FrameCam& C, float qz, float rx, float ry, int* u, int* v) {
  if (!(qz > 0.f)) return false;
  const float uf = __builtin_fmaf(C.fx, rx, C.cx), vf = __builtin_fmaf(C.fy, ry, C.cy);
  if (!(0.f < uf && uf < (float)C.W && 0.f < vf && vf < (float)C.H)) return false;
  *u = (int)uf;
  *v = (int)vf;
  return true;
}

// the first entry with the most hits, -1 without entries
__host__ __device__ __forceinline__ int lidar_best(const int* hits, int n_masks) {
  int best = -1, bh = -1;
  for (int j = 0; j < n_masks; ++j)
    if (hits[j] > bh) {
      bh = hits[j];
      best = j;
    }
  return best;
}
__host__ __device__ __forceinline__ bool lidar_matched(int best_hits, int n_proj) {
  return 2 * (long long)best_hits > (long long)n_proj;
}

__host__ __device__ __forceinline__ dsr_frame_params lidar_frame_params(const dsr_lidar_params& P) {
  dsr_frame_params F;
  F.max_pts = P.max_pts; F.max_bg = P.max_bg; F.downsample = P.downsample; F.expand = P.expand;
  F.min_mask_area = P.min_mask_area; F.near = 0.f; F.far = 0.f;
  return F;
}

// status, mask pixels, expanded box and grid from the record's counts, pose and mask index and the
// matched mask's statistics (frame_finish's box rule; bbox and the statistics are meaningless when
// o->mask < 0).  n_bg is left 0.
__host__ __device__ __forceinline__ void lidar_finish(const FrameCam& C, const dsr_lidar_params& P, const int* bbox,
                                                      int n_mask_px, int tl, int tt, int tr, int tb,
                                                      dsr_lidar_det_out* o) {
  o->n_mask_px = 0;
  o->n_bg = 0;
  o->box[0] = o->box[1] = 0;
  o->box[2] = o->box[3] = -1;
  o->grid_h = o->grid_w = 0;
  if (o->mask >= 0) {
    dsr_frame_det_out f;
    frame_finish(C, lidar_frame_params(P), bbox, n_mask_px, 1, tl, tt, tr, tb, &f);
    o->n_mask_px = n_mask_px;
    for (int k = 0; k < 4; ++k) o->box[k] = f.box[k];
    o->grid_h = f.grid_h;
    o->grid_w = f.grid_w;
  }
  o->status = o->t_cam_obj[11] <= 0.f ? DSR_LIDAR_BEHIND
            : o->n_crop == 0 ? DSR_LIDAR_NO_POINTS
            : o->mask < 0 ? DSR_LIDAR_NO_MATCH
            : n_mask_px <= P.min_mask_area ? DSR_LIDAR_SMALL_MASK : DSR_LIDAR_OK;
}

inline LidarXf lidar_xf(const float* tcv) {
  LidarXf X;
  for (int i = 0; i < 12; ++i) X.c[i] = tcv[i];
  return X;
}

// ---------------------------------------------------------------------------------------------
// host: the rule in plain C++ (dsr_lidar_inputs_host)
inline void lidar_inputs_host_impl(const FrameCam& C, const dsr_lidar_params& P, const float* tcv, const float* velo,
                                   int n_velo, int stride, const int* inst, int n_masks, const dsr_lidar_mask* masks,
                                   int n_det, const dsr_lidar_det* dets, float* pts, float* rays, float* dobs,
                                   dsr_lidar_det_out* out) {
  const LidarXf X = lidar_xf(tcv);
  std::vector<int> crop, cand, hits;
  for (int d = 0; d < n_det; ++d) {
    LidarDet L;
    lidar_prep(P, tcv, dets[d], &L);
    crop.clear();
    cand.clear();
    hits.assign((size_t)n_masks, 0);
    dsr_lidar_det_out o{};
    for (int i = 0; i < 16; ++i) o.t_cam_obj[i] = L.tco[i];
    for (int i = 0; i < n_velo; ++i) {
      const float* p = velo + (size_t)i * stride;
      const int r = lidar_test(L, p[0], p[1], p[2]);
      o.n_near += r & 1;
      if (r == 3) crop.push_back(i);
    }
    o.n_crop = (int)crop.size();
    o.n_pts = o.n_crop < P.max_pts ? o.n_crop : P.max_pts;
    float* op = pts ? pts + (size_t)d * P.max_pts * 3 : nullptr;
    float* orr = rays ? rays + (size_t)d * ((size_t)P.max_pts + P.max_bg) * 3 : nullptr;
    float* oz = dobs ? dobs + (size_t)d * P.max_pts : nullptr;
    const long long N = o.n_crop, n = o.n_pts;
    for (long long i = 0; i < n; ++i) {
      const float* p = velo + (size_t)crop[(size_t)frame_pick(i, n, N)] * stride;
      float q[3];
      lidar_q(X, p[0], p[1], p[2], q);
      const float rx = q[0] / q[2], ry = q[1] / q[2];
      if (op) { op[i * 3] = q[0]; op[i * 3 + 1] = q[1]; op[i * 3 + 2] = q[2]; }
      if (orr) { orr[i * 3] = rx; orr[i * 3 + 1] = ry; orr[i * 3 + 2] = 1.f; }
      if (oz) oz[i] = q[2];
      int u, v;
      if (!lidar_project(C, q[2], rx, ry, &u, &v)) continue;
      ++o.n_proj;
      const int label = inst[(size_t)v * C.W + u];
      for (int j = 0; j < n_masks; ++j)
        if (masks[j].label == label) {
          ++hits[(size_t)j];
          break;
        }
    }
    const int best = lidar_best(hits.data(), n_masks);
    o.n_hits = best >= 0 ? hits[(size_t)best] : 0;
    o.mask = best >= 0 && lidar_matched(o.n_hits, o.n_proj) ? best : -1;
    int n_mask_px = 0, tl = C.W, tt = C.H, tr = -1, tb = -1;
    const int label = o.mask >= 0 ? masks[o.mask].label : 0;
    if (o.mask >= 0)
      for (int v = 0; v < C.H; ++v)
        for (int u = 0; u < C.W; ++u) {
          if (inst[(size_t)v * C.W + u] != label) continue;
          ++n_mask_px;
          tl = u < tl ? u : tl; tr = u > tr ? u : tr;
          tt = v < tt ? v : tt; tb = v > tb ? v : tb;
        }
    lidar_finish(C, P, o.mask >= 0 ? masks[o.mask].bbox : nullptr, n_mask_px, tl, tt, tr, tb, &o);
    if (o.status == DSR_LIDAR_OK) {
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
        if (orr) { orr[(n + i) * 3] = rx; orr[(n + i) * 3 + 1] = ry; orr[(n + i) * 3 + 2] = 1.f; }
      }
    }
    if (out) out[d] = o;
  }
}

// ---------------------------------------------------------------------------------------------
// device

// Pass 1: per (64-point chunk, detection) the near and in counts.  grid = (ceil(n_chunks /
// FRAME_WAVES), n_det), one wave per chunk.
__global__ __launch_bounds__(FRAME_WG) DSR_NO_PK_F32 void k_lidar_count(const float* __restrict__ velo, int n_velo,
                                                         int stride, const LidarDet* __restrict__ dets,
                                                         int n_chunks, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * FRAME_WAVES + (threadIdx.x >> 6), d = blockIdx.y;
  if (c >= n_chunks) return;
  const int i = c * 64 + lane;
  int r = 0;
  if (i < n_velo) {
    const float* p = velo + (size_t)i * stride;
    r = lidar_test(dets[d], p[0], p[1], p[2]);
  }
  const unsigned long long nb = __ballot(r != 0), ib = __ballot(r == 3);
  if (lane == 0) cnt[(size_t)d * n_chunks + c] = __popcll(nb) | (__popcll(ib) << 8);
}

// Pass 2: one workgroup per detection — the near total, the chunk scan (coff), the counts and the
// pose of the record, and the association counters cleared.
__global__ __launch_bounds__(FRAME_WG) void k_lidar_scan(dsr_lidar_params P, const LidarDet* __restrict__ dets,
                                                         int n_chunks, const int* __restrict__ cnt,
                                                         int* __restrict__ coff, int* __restrict__ hits,
                                                         int* __restrict__ nproj,
                                                         dsr_lidar_det_out* __restrict__ recs) {
  __shared__ int sh[FRAME_WG];
  __shared__ int red[FRAME_WG];
  const int d = blockIdx.x, t = threadIdx.x;
  const int* cn = cnt + (size_t)d * n_chunks;
  int* co = coff + (size_t)d * n_chunks;
  int near = 0;
  for (int c = t; c < n_chunks; c += FRAME_WG) {
    const int v = cn[c];
    near += v & 255;
    co[c] = v >> 8;
  }
  red[t] = near;
  hits[(size_t)d * DSR_LIDAR_MAX_MASKS + t] = 0;            // (FRAME_WG >= DSR_LIDAR_MAX_MASKS; the tail is unused)
  __syncthreads();                                          // co[] and red[] written
  const int n_crop = frame_block_scan(co, n_chunks, sh);
  if (t == 0) {
    for (int k = 1; k < FRAME_WG; ++k) near += red[k];
    dsr_lidar_det_out o;
    o.status = 0;
    o.n_near = near;
    o.n_crop = n_crop;
    o.n_pts = n_crop < P.max_pts ? n_crop : P.max_pts;
    o.n_proj = 0; o.mask = -1; o.n_hits = 0; o.n_mask_px = 0; o.n_bg = 0;
    o.box[0] = o.box[1] = 0; o.box[2] = o.box[3] = -1;
    o.grid_h = o.grid_w = 0;
    for (int i = 0; i < 16; ++i) o.t_cam_obj[i] = dets[d].tco[i];
    recs[d] = o;
    nproj[d] = 0;
  }
}

// Pass 3: every in-point finds the output row that picks it (frame_row_of over its rank among the
// in-points) and writes its surface point, foreground ray and depth; a projected row counts for the
// first mask-list entry carrying its pixel's label (integer atomics).  grid as pass 1.  Outputs go
// to the slots of desc (a capacity batch) or, desc == null, to fixed strides per detection.
// IMG = false (the tracker, dsr_track.hpp): the surface points alone — no ray, no depth, no
// projection; C, inst, masks, hits, nproj, rays and dobs are not read.
template <bool IMG>
__global__ __launch_bounds__(FRAME_WG) DSR_NO_PK_F32 void k_lidar_emit(FrameCam C, dsr_lidar_params P, LidarXf X,
                                                         const float* __restrict__ velo, int n_velo, int stride,
                                                         const int* __restrict__ inst,
                                                         const dsr_lidar_mask* __restrict__ masks, int n_masks,
                                                         const LidarDet* __restrict__ dets, int n_chunks,
                                                         const int* __restrict__ cnt, const int* __restrict__ coff,
                                                         const dsr_lidar_det_out* __restrict__ recs,
                                                         int* __restrict__ hits, int* __restrict__ nproj,
                                                         const ObjDesc* __restrict__ desc, float* __restrict__ pts,
                                                         float* __restrict__ rays, float* __restrict__ dobs) {
  __shared__ int mlabel[IMG ? DSR_LIDAR_MAX_MASKS : 1];
  const int lane = threadIdx.x & 63, c = blockIdx.x * FRAME_WAVES + (threadIdx.x >> 6), d = blockIdx.y;
  if constexpr (IMG) {
    if ((int)threadIdx.x < n_masks) mlabel[threadIdx.x] = masks[threadIdx.x].label;
    __syncthreads();
  }
  if (c >= n_chunks) return;
  if ((cnt[(size_t)d * n_chunks + c] >> 8) == 0) return;
  const long long N = recs[d].n_crop, n = recs[d].n_pts;
  const long long base = coff[(size_t)d * n_chunks + c];
  float *op, *orr = nullptr, *oz = nullptr;
  if (desc) {
    op = pts + (size_t)desc[d].pts_off * 3;
    if constexpr (IMG) {
      orr = rays + (size_t)desc[d].ray_off * 3;
      oz = dobs + desc[d].ray_off;
    }
  } else {
    op = pts + (size_t)d * P.max_pts * 3;
    if constexpr (IMG) {
      orr = rays + (size_t)d * ((size_t)P.max_pts + P.max_bg) * 3;
      oz = dobs + (size_t)d * P.max_pts;
    }
  }
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const int i = c * 64 + lane;
  bool in = false;
  [[maybe_unused]] bool proj = false;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (i < n_velo) {
    const float* p = velo + (size_t)i * stride;
    px = p[0]; py = p[1]; pz = p[2];
    in = lidar_test(dets[d], px, py, pz) == 3;
  }
  const unsigned long long ib = __ballot(in);
  if (in) {
    const long long row = frame_row_of(base + __popcll(ib & below), n, N);
    if (row >= 0 && row < n) {
      float q[3];
      lidar_q(X, px, py, pz, q);
      op[row * 3] = q[0]; op[row * 3 + 1] = q[1]; op[row * 3 + 2] = q[2];
      if constexpr (IMG) {
        const float rx = q[0] / q[2], ry = q[1] / q[2];
        orr[row * 3] = rx; orr[row * 3 + 1] = ry; orr[row * 3 + 2] = 1.f;
        oz[row] = q[2];
        int u, v;
        if (lidar_project(C, q[2], rx, ry, &u, &v)) {
          proj = true;
          const int label = inst[(size_t)v * C.W + u];
          for (int j = 0; j < n_masks; ++j)
            if (mlabel[j] == label) {
              atomicAdd(&hits[(size_t)d * DSR_LIDAR_MAX_MASKS + j], 1);
              break;
            }
        }
      }
    }
  }
  if constexpr (IMG) {
    const unsigned long long pb = __ballot(proj);
    if (lane == 0 && pb) atomicAdd(&nproj[d], __popcll(pb));
  }
}

// Pass 4: one workgroup per detection — the first entry with the most hits, the threshold, and
// the {label, bbox} the mask passes read.
__global__ __launch_bounds__(FRAME_WG) void k_lidar_match(const dsr_lidar_mask* __restrict__ masks, int n_masks,
                                                          const int* __restrict__ hits,
                                                          const int* __restrict__ nproj,
                                                          dsr_lidar_det_out* __restrict__ recs,
                                                          LidarMatch* __restrict__ match) {
  __shared__ int sh[FRAME_WG];
  const int d = blockIdx.x, t = threadIdx.x;
  sh[t] = t < n_masks ? hits[(size_t)d * DSR_LIDAR_MAX_MASKS + t] : -1;
  __syncthreads();
  if (t != 0) return;
  const int best = lidar_best(sh, n_masks), np = nproj[d];
  const int bh = best >= 0 ? sh[best] : 0;
  const bool matched = best >= 0 && lidar_matched(bh, np);
  recs[d].n_proj = np;
  recs[d].n_hits = bh;
  recs[d].mask = matched ? best : -1;
  LidarMatch M;
  M.mask = matched ? best : -1;
  M.label = matched ? masks[best].label : 0;
  for (int k = 0; k < 4; ++k) M.bbox[k] = matched ? masks[best].bbox[k] : (k < 2 ? 0 : -1);
  match[d] = M;
}

// Pass 5: per (image row, matched detection) the pixels carrying the matched label and the row's
// first / last such column.  grid = (ceil(H / FRAME_WAVES), n_det), one wave per row.
__global__ __launch_bounds__(FRAME_WG) void k_lidar_rows(FrameCam C, const int* __restrict__ inst,
                                                         const LidarMatch* __restrict__ match,
                                                         int4* __restrict__ rows) {
  const int lane = threadIdx.x & 63, v = blockIdx.x * FRAME_WAVES + (threadIdx.x >> 6), d = blockIdx.y;
  if (v >= C.H) return;
  if (match[d].mask < 0) return;
  const int label = match[d].label;
  int nm = 0, umin = C.W, umax = -1;
  for (int c = 0; c < C.W; c += 64) {
    const int u = c + lane;
    const bool m = u < C.W && inst[(size_t)v * C.W + u] == label;
    const unsigned long long mb = __ballot(m);
    nm += __popcll(mb);
    if (mb) {
      const int first = c + (__ffsll((long long)mb) - 1), last = c + 63 - __clzll((long long)mb);
      umin = first < umin ? first : umin;
      umax = last > umax ? last : umax;
    }
  }
  if (lane == 0) rows[(size_t)d * C.H + v] = make_int4(nm, 0, umin, umax);
}

// Pass 6: one workgroup per detection — the mask totals and tight box, the status / expanded box /
// grid (lidar_finish), the background candidates per grid row and their scan (bgoff), the record,
// and (desc != null) the slot's ObjDesc counts: an empty object unless the status is OK.
__global__ __launch_bounds__(FRAME_WG) void k_lidar_bg_scan(FrameCam C, dsr_lidar_params P,
                                                            const int* __restrict__ inst,
                                                            const LidarMatch* __restrict__ match,
                                                            const int4* __restrict__ rows, int* __restrict__ bgoff,
                                                            int* __restrict__ aux,
                                                            dsr_lidar_det_out* __restrict__ recs,
                                                            ObjDesc* __restrict__ desc) {
  __shared__ int sh[FRAME_WG];
  __shared__ int red[5][FRAME_WG];
  __shared__ dsr_lidar_det_out rec;
  const int d = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool matched = match[d].mask >= 0;                  // the same for the whole workgroup
  const int4* row = rows + (size_t)d * C.H;
  int* bo = bgoff + (size_t)d * C.H;
  int nm = 0, tl = C.W, tt = C.H, tr = -1, tb = -1;
  if (matched)
    for (int v = t; v < C.H; v += FRAME_WG) {
      const int4 r = row[v];
      nm += r.x;
      if (r.x > 0) {
        tl = r.z < tl ? r.z : tl;
        tr = r.w > tr ? r.w : tr;
        tt = v < tt ? v : tt;
        tb = v > tb ? v : tb;
      }
    }
  red[0][t] = nm; red[1][t] = tl; red[2][t] = tt; red[3][t] = tr; red[4][t] = tb;
  __syncthreads();
  if (t == 0) {
    for (int k = 1; k < FRAME_WG; ++k) {
      nm += red[0][k];
      tl = red[1][k] < tl ? red[1][k] : tl;
      tt = red[2][k] < tt ? red[2][k] : tt;
      tr = red[3][k] > tr ? red[3][k] : tr;
      tb = red[4][k] > tb ? red[4][k] : tb;
    }
    dsr_lidar_det_out o = recs[d];
    int bbox[4];
    for (int k = 0; k < 4; ++k) bbox[k] = match[d].bbox[k];
    lidar_finish(C, P, bbox, nm, tl, tt, tr, tb, &o);
    rec = o;
  }
  __syncthreads();
  const int gh = rec.status == DSR_LIDAR_OK && P.max_bg > 0 ? rec.grid_h : 0, gw = rec.grid_w;
  const int bl = rec.box[0], bt = rec.box[1], bw = rec.box[2] - rec.box[0] + 1, bh = rec.box[3] - rec.box[1] + 1;
  const int label = match[d].label;
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
    dsr_lidar_det_out o = rec;
    o.n_bg = NB < P.max_bg ? NB : P.max_bg;
    recs[d] = o;
    aux[d] = NB;
    if (desc) {
      const bool ok = o.status == DSR_LIDAR_OK;
      desc[d].n_pts = ok ? o.n_pts : 0;
      desc[d].n_rays = ok ? o.n_pts + o.n_bg : 0;
      desc[d].n_fg = ok ? o.n_pts : 0;
    }
  }
}

// Pass 7: every background candidate finds the output row that picks it (k_frame_emit's second
// half).  grid = (ceil(H / FRAME_WAVES), n_det), one wave per grid row; only a batch's dobs has
// rows for the background rays (0).
__global__ __launch_bounds__(FRAME_WG) DSR_NO_PK_F32 void k_lidar_bg_emit(FrameCam C, dsr_lidar_params P,
                                                         const int* __restrict__ inst,
                                                         const LidarMatch* __restrict__ match,
                                                         const int* __restrict__ bgoff,
                                                         const int* __restrict__ aux,
                                                         const dsr_lidar_det_out* __restrict__ recs,
                                                         const ObjDesc* __restrict__ desc, float* __restrict__ rays,
                                                         float* __restrict__ dobs) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * FRAME_WAVES + (threadIdx.x >> 6), d = blockIdx.y;
  const dsr_lidar_det_out& rec = recs[d];
  if (rec.status != DSR_LIDAR_OK) return;
  const int gh = P.max_bg > 0 ? rec.grid_h : 0, gw = rec.grid_w;
  if (j >= gh) return;
  float* orr = desc ? rays + (size_t)desc[d].ray_off * 3 : rays + (size_t)d * ((size_t)P.max_pts + P.max_bg) * 3;
  float* oz = desc ? dobs + desc[d].ray_off : nullptr;
  const int label = match[d].label;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
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
        if (oz) oz[r] = 0.f;
      }
    }
    base += __popcll(cb);
  }
}

// the device buffers of one sweep call, carved from one block (256 B aligned parts)
struct LidarDev {
  float* velo;
  int* inst;
  dsr_lidar_mask* masks;
  LidarDet* dets;
  int *cnt, *coff, *hits, *nproj;
  LidarMatch* match;
  int4* rows;
  int *bgoff, *aux;
  dsr_lidar_det_out* recs;
};
struct LidarShape {        // what sizes the block
  int n_velo, stride, W, H, n_det;
};
inline int lidar_chunks(int n_velo) { return (n_velo + 63) / 64; }
// bytes of the uploaded part (velo | inst | masks | dets) and of the whole block
inline size_t lidar_upload_bytes(const LidarShape& S) {
  const size_t nd = (size_t)(S.n_det > 0 ? S.n_det : 1);
  return frame_up256((size_t)S.n_velo * S.stride * 4) + frame_up256((size_t)S.W * S.H * 4) +
         frame_up256(sizeof(dsr_lidar_mask) * DSR_LIDAR_MAX_MASKS) + frame_up256(sizeof(LidarDet) * nd);
}
inline size_t lidar_dev_bytes(const LidarShape& S) {
  const size_t nd = (size_t)(S.n_det > 0 ? S.n_det : 1), nc = (size_t)lidar_chunks(S.n_velo);
  return lidar_upload_bytes(S) + 2 * frame_up256(nd * nc * sizeof(int)) +
         frame_up256(nd * DSR_LIDAR_MAX_MASKS * sizeof(int)) + frame_up256(nd * sizeof(int)) +
         frame_up256(nd * sizeof(LidarMatch)) + frame_up256(nd * S.H * sizeof(int4)) +
         frame_up256(nd * S.H * sizeof(int)) + frame_up256(nd * sizeof(int)) +
         frame_up256(nd * sizeof(dsr_lidar_det_out));
}
inline LidarDev lidar_carve(void* block, const LidarShape& S) {
  const size_t nd = (size_t)(S.n_det > 0 ? S.n_det : 1), nc = (size_t)lidar_chunks(S.n_velo);
  char* p = static_cast<char*>(block);
  LidarDev D;
  D.velo = reinterpret_cast<float*>(p);           p += frame_up256((size_t)S.n_velo * S.stride * 4);
  D.inst = reinterpret_cast<int*>(p);             p += frame_up256((size_t)S.W * S.H * 4);
  D.masks = reinterpret_cast<dsr_lidar_mask*>(p); p += frame_up256(sizeof(dsr_lidar_mask) * DSR_LIDAR_MAX_MASKS);
  D.dets = reinterpret_cast<LidarDet*>(p);        p += frame_up256(sizeof(LidarDet) * nd);
  D.cnt = reinterpret_cast<int*>(p);              p += frame_up256(nd * nc * sizeof(int));
  D.coff = reinterpret_cast<int*>(p);             p += frame_up256(nd * nc * sizeof(int));
  D.hits = reinterpret_cast<int*>(p);             p += frame_up256(nd * DSR_LIDAR_MAX_MASKS * sizeof(int));
  D.nproj = reinterpret_cast<int*>(p);            p += frame_up256(nd * sizeof(int));
  D.match = reinterpret_cast<LidarMatch*>(p);     p += frame_up256(nd * sizeof(LidarMatch));
  D.rows = reinterpret_cast<int4*>(p);            p += frame_up256(nd * S.H * sizeof(int4));
  D.bgoff = reinterpret_cast<int*>(p);            p += frame_up256(nd * S.H * sizeof(int));
  D.aux = reinterpret_cast<int*>(p);              p += frame_up256(nd * sizeof(int));
  D.recs = reinterpret_cast<dsr_lidar_det_out*>(p);
  return D;
}

// the uploaded part of a sweep block, laid out as lidar_carve does; the detections prepared
inline void lidar_pack(void* host, const LidarShape& S, const dsr_lidar_params& P, const float* tcv, const float* velo,
                       const int* inst, int n_masks, const dsr_lidar_mask* masks, const dsr_lidar_det* dets) {
  const LidarDev H = lidar_carve(host, S);
  if (S.n_velo > 0) std::memcpy(H.velo, velo, (size_t)S.n_velo * S.stride * sizeof(float));
  std::memcpy(H.inst, inst, (size_t)S.W * S.H * sizeof(int));
  if (n_masks > 0) std::memcpy(H.masks, masks, sizeof(dsr_lidar_mask) * (size_t)n_masks);
  for (int d = 0; d < S.n_det; ++d) lidar_prep(P, tcv, dets[d], &H.dets[d]);
}

// the seven passes on stream s (n_det > 0); the uploaded part of D is already enqueued
inline void lidar_launch(hipStream_t s, const FrameCam& C, const dsr_lidar_params& P, const LidarXf& X,
                         const LidarShape& S, int n_masks, const LidarDev& D, ObjDesc* desc, float* pts, float* rays,
                         float* dobs) {
  const int nc = lidar_chunks(S.n_velo), nd = S.n_det;
  const unsigned gc = (unsigned)((nc + FRAME_WAVES - 1) / FRAME_WAVES);
  const unsigned gy = (unsigned)((C.H + FRAME_WAVES - 1) / FRAME_WAVES);
  if (nc > 0)
    hipLaunchKernelGGL(k_lidar_count, dim3(gc, nd), dim3(FRAME_WG), 0, s, (const float*)D.velo, S.n_velo, S.stride,
                       (const LidarDet*)D.dets, nc, D.cnt);
  hipLaunchKernelGGL(k_lidar_scan, dim3(nd), dim3(FRAME_WG), 0, s, P, (const LidarDet*)D.dets, nc, (const int*)D.cnt,
                     D.coff, D.hits, D.nproj, D.recs);
  if (nc > 0)
    hipLaunchKernelGGL(k_lidar_emit<true>, dim3(gc, nd), dim3(FRAME_WG), 0, s, C, P, X, (const float*)D.velo, S.n_velo,
                       S.stride, (const int*)D.inst, (const dsr_lidar_mask*)D.masks, n_masks, (const LidarDet*)D.dets,
                       nc, (const int*)D.cnt, (const int*)D.coff, (const dsr_lidar_det_out*)D.recs, D.hits, D.nproj,
                       (const ObjDesc*)desc, pts, rays, dobs);
  hipLaunchKernelGGL(k_lidar_match, dim3(nd), dim3(FRAME_WG), 0, s, (const dsr_lidar_mask*)D.masks, n_masks,
                     (const int*)D.hits, (const int*)D.nproj, D.recs, D.match);
  hipLaunchKernelGGL(k_lidar_rows, dim3(gy, nd), dim3(FRAME_WG), 0, s, C, (const int*)D.inst,
                     (const LidarMatch*)D.match, D.rows);
  hipLaunchKernelGGL(k_lidar_bg_scan, dim3(nd), dim3(FRAME_WG), 0, s, C, P, (const int*)D.inst,
                     (const LidarMatch*)D.match, (const int4*)D.rows, D.bgoff, D.aux, D.recs, desc);
  hipLaunchKernelGGL(k_lidar_bg_emit, dim3(gy, nd), dim3(FRAME_WG), 0, s, C, P, (const int*)D.inst,
                     (const LidarMatch*)D.match, (const int*)D.bgoff, (const int*)D.aux,
                     (const dsr_lidar_det_out*)D.recs, (const ObjDesc*)desc, rays, dobs);
}

// the argument errors of the sweep entry points (checked before the device is touched);
// rigid: the caller's verdict on t_cam_velo (null pointer: not rigid)
inline const char* lidar_args_error(const dsr_camera* cam, const dsr_lidar_params* P, bool rigid, const float* velo,
                                    int n_velo, int stride, const int* inst, int n_masks, const dsr_lidar_mask* masks,
                                    int n_det, const dsr_lidar_det* dets) {
  if (!cam || !P) return "lidar: null camera or parameters";
  if (!inst) return "lidar: null instance image";
  if (cam->width <= 0 || cam->height <= 0) return "lidar: image size must be positive";
  if ((long long)cam->width * cam->height > 0x7fffffffLL) return "lidar: image larger than 2^31 - 1 pixels";
  if (!(cam->fx > 0.f) || !(cam->fy > 0.f)) return "lidar: focal lengths must be positive";
  if (P->max_pts < 1) return "lidar: max_pts must be >= 1";
  if (P->max_bg < 0) return "lidar: max_bg must be >= 0";
  if (P->downsample < 1) return "lidar: downsample must be >= 1";
  if (P->expand < 0) return "lidar: expand must be >= 0";
  if (!(P->radius > 0.f) || std::isinf(P->radius)) return "lidar: radius must be positive and finite";
  if (!(P->box_margin > 0.f) || std::isinf(P->box_margin)) return "lidar: box_margin must be positive and finite";
  if (!rigid) return "lidar: t_cam_velo must be rigid";
  if (stride < 3) return "lidar: stride must be >= 3";
  if (n_velo < 0 || n_velo > LIDAR_MAX_VELO) return "lidar: n_velo must be in 0 .. 2^24";
  if (n_velo > 0 && !velo) return "lidar: null sweep";
  if (n_masks < 0 || n_masks > DSR_LIDAR_MAX_MASKS || (n_masks > 0 && !masks)) return "lidar: n_masks outside 0 .. 256 or null masks";
  if (n_det < 0 || (n_det > 0 && !dets)) return "lidar: n_det < 0 or null detections";
  for (int d = 0; d < n_det; ++d) {
    for (int k = 0; k < 3; ++k) {
      if (!std::isfinite(dets[d].trans[k]) || !std::isfinite(dets[d].size[k])) return "lidar: non-finite detection";
      if (!(dets[d].size[k] > 0.f)) return "lidar: detection sizes must be positive";
    }
    if (!std::isfinite(dets[d].theta)) return "lidar: non-finite detection";
  }
  return nullptr;
}

}  // namespace dsr
