// dsr_track.hpp — the resident object tracker (dsr_tracker_*): pose-only GN of the
// detections that are already in the map (Optimizer.estimate_pose_cam_obj,
// reconstruct/optimizer.py:46-87, called once per associated detection by
// LocalMapping::GetNewObservations_onyforStereo, src/LocalMapping_util.cc:84-154) without a host
// step between the upload and the download.  The GN iteration itself is dsr_pose_only_batch's
// (launch_jac with raw residuals, k_solve_pose, k_inv_out: dsr_kernels.hpp); what is here is what
// that entry point does on the host between its launches: the descriptors, the tile table and the
// iteration-4 inlier filter (optimizer.py:77-79), and the host rule of a sweep call's start pose.
// The points come from host rows, from a sweep (k_lidar_emit<false>, dsr_lidar.hpp) or from a depth
// image and its instance labels (k_frame_emit<false>, dsr_frame.hpp).
//
// Layout of a tracker of max_obj objects x max_pts points, tpo = ceil(max_pts / TILE):
//   pts    [max_obj][max_pts][3]   object o's rows from o * max_pts           (ObjDesc.pts_off)
//   res    [max_obj][max_pts]      the Jacobian kernel's residuals, as pts
//   slots  [max_obj][tpo]          object o's tile partials from o * tpo      (ObjDesc.slot_sdf)
//   tiles  [max_obj * tpo]         {object, 0, start, count}: object order, then tile order
// k_solve_pose adds an object's tiles in tile order from its own base, so the strides change no value.
// Wave64; ordinary vector stores, no atomics, nothing depends on the order of execution.
#pragma once
#include "dsr_lidar.hpp"

namespace dsr {

constexpr float TRACK_INLIER = 0.05f;             // optimizer.py:78
constexpr int TRACK_MAX_PTS = 1 << 20;            // points per object at most
constexpr long long TRACK_MAX_ROWS = 1ll << 22;   // max_obj x max_pts at most (65536 tiles of slots: 0.7 GB)

inline int track_tiles_per_obj(int max_pts) { return (max_pts + TILE - 1) / TILE; }

// The start pose of a sweep call (dsr_lidar_track_prep_host): lidar_prep's quantities and
// arithmetic — fp64 on the fp32 inputs, each operation rounded on its own, each stored value
// rounded to fp32 once — with sigma left out of the rotation block: t_co_se3 = t_cam_velo [R | o],
// det_scale = (float)sigma, sigma = m l / 2.  t_cam_velo is rigid, so this is ObjectDetection's
// decomposition of t_cam_obj (src/ObjectDetection.cc:29-37) without a determinant or a cube root.
inline void lidar_track_prep(const dsr_lidar_params& P, const float* tcv, const dsr_lidar_det& d, float* t_co_se3,
                             float* det_scale) {
  DSR_FP_STRICT
  const double th = (double)d.theta, c = std::cos(th), s = std::sin(th);
  const double R[3][3] = {{c, 0.0, -s}, {-s, 0.0, -c}, {0.0, 1.0, 0.0}};
  const double hh = (double)d.size[2] / 2.0;
  const double o[3] = {(double)d.trans[0], (double)d.trans[1], (double)d.trans[2] + hh};
  const double sigma = ((double)P.box_margin * (double)d.size[1]) / 2.0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      double acc = 0.0;
      for (int k = 0; k < 3; ++k) {
        const double term = (double)tcv[i * 4 + k] * R[k][j];
        acc = acc + term;
      }
      t_co_se3[i * 4 + j] = (float)acc;
    }
    double acc = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double term = (double)tcv[i * 4 + k] * o[k];
      acc = acc + term;
    }
    t_co_se3[i * 4 + 3] = (float)(acc + (double)tcv[i * 4 + 3]);
  }
  t_co_se3[12] = t_co_se3[13] = t_co_se3[14] = 0.f;
  t_co_se3[15] = 1.f;
  *det_scale = (float)sigma;
}

// every object's tiles from its count `n_of(o)` (k_tiles_jac's block scan), the total beside them
template <class NOf>
__device__ __forceinline__ void track_tiles(int n_obj, NOf n_of, Tile* __restrict__ tiles, int* __restrict__ n_tiles) {
  const int total = tile_scan(
      n_obj, 0,
      [&](int o, int& n, int& nt) {
        n = n_of(o);
        nt = (n + TILE - 1) / TILE;
      },
      [&](int idx, int o, int i, int n) {
        Tile t;
        t.obj = o; t.term = 0; t.start = i * TILE;
        t.count = min(TILE, n - i * TILE);
        tiles[idx] = t;
      });
  if (threadIdx.x == 0) *n_tiles = total;
}

// After the fill, one workgroup of TILE_SCAN_THREADS: every object's descriptor at the fixed
// strides and its record, from the staged counts (cnt, host rows) or from where the ingest's scan
// left them — k_lidar_scan (lrecs, a sweep: n_pts, n_near, n_crop) or k_frame_scan (frecs, a depth
// image: n_pts, n_mask, n_valid; 0 points unless the ingest is ok) — no host read in between; then
// the tile table.  At most one of lrecs and frecs is given.
__global__ __launch_bounds__(TILE_SCAN_THREADS) void k_track_begin(int n_obj, int max_pts, int tpo,
                                                                 const int* __restrict__ cnt,
                                                                 const dsr_lidar_det_out* __restrict__ lrecs,
                                                                 const dsr_frame_det_out* __restrict__ frecs,
                                                                 ObjDesc* __restrict__ desc,
                                                                 dsr_track_out* __restrict__ recs,
                                                                 Tile* __restrict__ tiles, int* __restrict__ n_tiles) {
  const auto n_of = [&](int o) { return lrecs ? lrecs[o].n_pts : frecs ? frecs[o].n_pts : cnt[o]; };
  for (int o = threadIdx.x; o < n_obj; o += blockDim.x) {
    const int n = n_of(o);
    ObjDesc d;
    d.pts_off = o * max_pts; d.n_pts = n;
    d.ray_off = 0; d.n_rays = 0; d.n_fg = 0; d.cand_off = 0;
    d.slot_sdf = o * tpo; d.pad = 0;
    desc[o] = d;
    dsr_track_out r;
    r.status = n > 0 ? DSR_TRACK_OK : DSR_TRACK_NO_POINTS;
    r.n_pts = n;
    r.n_inliers = n;
    r.n_near = lrecs ? lrecs[o].n_near : frecs ? frecs[o].n_mask : 0;
    r.n_crop = lrecs ? lrecs[o].n_crop : frecs ? frecs[o].n_valid : 0;
    recs[o] = r;
  }
  track_tiles(n_obj, n_of, tiles, n_tiles);
}

// After the filter: the tile table of the compacted point sets.
__global__ __launch_bounds__(TILE_SCAN_THREADS) void k_track_tiles(int n_obj, const ObjDesc* __restrict__ desc,
                                                                 Tile* __restrict__ tiles, int* __restrict__ n_tiles) {
  track_tiles(n_obj, [&](int o) { return desc[o].n_pts; }, tiles, n_tiles);
}

// The iteration-4 inlier filter (optimizer.py:77-79), one workgroup per object after that
// iteration's solve: a point is kept iff |res| <= 0.05 (a NaN residual drops it).  The object's
// rows are compacted in place, in order, in ascending FRAME_WG-row chunks — a chunk is read into
// registers, __syncthreads(), then written; every destination is at or before its source
// (k_frame_compact's scheme).  The new count goes to the ObjDesc, n_inliers and the status to the
// record.
__global__ __launch_bounds__(FRAME_WG) DSR_NO_PK_F32 void k_track_filter(ObjDesc* __restrict__ desc,
                                                                        const float* __restrict__ res,
                                                                        float* __restrict__ pts,
                                                                        dsr_track_out* __restrict__ recs) {
  __shared__ int wsum[FRAME_WAVES];
  const int o = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n_in = desc[o].n_pts;
  if (n_in <= 0) return;                     // (uniform: the record stays NO_POINTS)
  float* op = pts + (size_t)desc[o].pts_off * 3;
  const float* rs = res + desc[o].pts_off;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  int base = 0;
  for (int c0 = 0; c0 < n_in; c0 += FRAME_WG) {
    const int i = c0 + t;
    const bool f = i < n_in && fabsf(rs[i]) <= TRACK_INLIER;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (f) {
      px = op[(size_t)i * 3]; py = op[(size_t)i * 3 + 1]; pz = op[(size_t)i * 3 + 2];
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
    }
    base += all;
    __syncthreads();                         // wsum[] is rewritten by the next chunk
  }
  if (t == 0) {
    desc[o].n_pts = base;
    recs[o].n_inliers = base;
    if (base == 0) recs[o].status = DSR_TRACK_NO_INLIERS;
  }
}

}  // namespace dsr
