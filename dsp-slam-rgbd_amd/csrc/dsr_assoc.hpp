// dsr_assoc.hpp — a frame's detections against the objects of a map (dsr_scene_associate_*,
// DESIGN.md §3.6d).  Replaces Tracking::AssociateObjectsByProjection_onlyformono
// (src/Tracking_util.cc:210-288), which votes per detection over the object ids of the ORB map
// points under its mask: here the evidence is the depth under the mask and the map's decoders — a
// detection belongs to the map object whose surface its back-projected points lie on.
//
// One call: detection j's camera-frame rows (the frame ingest's, dsr_frame.hpp, or the caller's)
// go to the world and into the scene's point buffer at the fixed stride max_pts (k_assoc_world),
// the scene's value passes (dsr_scene.hpp: bin, scan, emit, the exact decode) run on them
// unchanged, every decoded tile adds its candidates to the int32 tables n_in / n_hit / n_neg
// [detection][object] (k_assoc_vote), and every detection decides (k_assoc_pick).  The decision
// rule is stated once for both sides (assoc_decide is __host__ __device__).
#pragma once
#include "../../include/dsr.h"
#include "dsr_dev.hpp"
#include "dsr_frame.hpp"

#include <cmath>

namespace dsr {

constexpr int ASSOC_WG = 256;     // threads per workgroup of k_assoc_world

struct AssocXf {                  // rows 0..2 of t_world_cam (B | b), row-major; on == 0: the rows are world points
  float M[12];
  int on;
};

// w_k = fmaf(B_k0, q_x, fmaf(B_k1, q_y, fmaf(B_k2, q_z, b_k))): the three operations of sc_point
__host__ __device__ __forceinline__ void assoc_world(const AssocXf& X, const float* q, float* w) {
  const float x = q[0], y = q[1], z = q[2];
  if (!X.on) {
    w[0] = x; w[1] = y; w[2] = z;
    return;
  }
#ifdef __HIP_DEVICE_COMPILE__
  w[0] = fmaf(X.M[0], x, fmaf(X.M[1], y, fmaf(X.M[2], z, X.M[3])));
  w[1] = fmaf(X.M[4], x, fmaf(X.M[5], y, fmaf(X.M[6], z, X.M[7])));
  w[2] = fmaf(X.M[8], x, fmaf(X.M[9], y, fmaf(X.M[10], z, X.M[11])));
#else
  w[0] = std::fmaf(X.M[0], x, std::fmaf(X.M[1], y, std::fmaf(X.M[2], z, X.M[3])));
  w[1] = std::fmaf(X.M[4], x, std::fmaf(X.M[5], y, std::fmaf(X.M[6], z, X.M[7])));
  w[2] = std::fmaf(X.M[8], x, std::fmaf(X.M[9], y, std::fmaf(X.M[10], z, X.M[11])));
#endif
}

inline AssocXf assoc_xf(const float* t_world_cam) {
  AssocXf X{};
  X.on = t_world_cam ? 1 : 0;
  if (t_world_cam)
    for (int i = 0; i < 12; ++i) X.M[i] = t_world_cam[i];
  return X;
}

// a candidate (object a, n_hit ha) goes before (b, hb): more hits, then the lower index
__host__ __device__ __forceinline__ bool assoc_before(int ha, int a, int hb, int b) {
  return ha > hb || (ha == hb && a < b);
}

// The record of one detection from its best object and runner-up (-1: none) and their counts.
// n_hit / n_in / n_neg are the best object's whether or not it is accepted.
__host__ __device__ __forceinline__ void assoc_decide(const dsr_assoc_params& A, int n_pts, int best, int hit, int in,
                                                      int neg, int second, int second_hit, dsr_assoc_out* o) {
  const bool matched = n_pts > 0 && best >= 0 && hit >= A.min_hits &&
                       100ll * (long long)hit > (long long)A.min_pct * (long long)n_pts;
  o->status = n_pts <= 0 ? DSR_ASSOC_NO_POINTS : matched ? DSR_ASSOC_MATCHED : DSR_ASSOC_NEW;
  o->n_pts = n_pts > 0 ? n_pts : 0;
  o->obj = matched ? best : -1;
  o->n_hit = best >= 0 ? hit : 0;
  o->n_in = best >= 0 ? in : 0;
  o->n_neg = best >= 0 ? neg : 0;
  o->second = second;
  o->second_hit = second >= 0 ? second_hit : 0;
  o->ingest_status = 0;
  o->n_mask = 0;
  o->n_valid = 0;
}

// host: the pick over one detection's rows of the tables (tin / thit / tneg: n_obj ints each)
inline void assoc_pick_host_one(const dsr_assoc_params& A, int n_obj, const int* tin, const int* thit,
                                const int* tneg, int n_pts, dsr_assoc_out* o) {
  int b = -1, s = -1;
  for (int i = 0; i < n_obj; ++i) {
    if (b < 0 || assoc_before(thit[i], i, thit[b], b)) {
      s = b;
      b = i;
    } else if (s < 0 || assoc_before(thit[i], i, thit[s], s)) {
      s = i;
    }
  }
  assoc_decide(A, n_pts, b, b >= 0 ? thit[b] : 0, b >= 0 ? tin[b] : 0, b >= 0 ? tneg[b] : 0, s, s >= 0 ? thit[s] : 0, o);
}

inline const char* assoc_params_error(const dsr_assoc_params* A) {
  if (!A) return "associate: null parameters";
  if (!(A->inlier_tol > 0.f) || !std::isfinite(A->inlier_tol)) return "associate: inlier_tol must be positive and finite";
  if (A->min_hits < 1) return "associate: min_hits must be >= 1";
  if (A->min_pct < 0 || A->min_pct > 99) return "associate: min_pct must be in [0, 99]";
  return nullptr;
}

// ---------------------------------------------------------------------------------------------
// device

// World: one thread per slot p = j * max_pts + k of the scene's point buffer — row k of detection
// j to the world, NaN where k >= the detection's count (a NaN point is in no ball).  The count is
// the ingest record's n_pts (recs != null: a frame call) or cnt[j] (host rows).
__global__ __launch_bounds__(ASSOC_WG) DSR_NO_PK_F32 void k_assoc_world(int n_slots, int max_pts, AssocXf X,
                                                                        const float* __restrict__ rows,
                                                                        const int* __restrict__ cnt,
                                                                        const dsr_frame_det_out* __restrict__ recs,
                                                                        float* __restrict__ pts) {
  const int p = blockIdx.x * ASSOC_WG + (int)threadIdx.x;
  if (p >= n_slots) return;
  const int j = p / max_pts, k = p - j * max_pts;
  const int n = recs ? recs[j].n_pts : cnt[j];
  const float nan = __builtin_nanf("");
  float w[3] = {nan, nan, nan};
  if (k < n) assoc_world(X, rows + (size_t)p * 3, w);
  float* o = pts + (size_t)p * 3;
  o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
}

// Vote: one wave per decoded tile (grid-stride over *n_tiles, as k_sc_min).  A tile's candidates
// are in point order, so their detections p / max_pts are non-decreasing across the lanes: the
// lanes whose detection differs from the lane before head a segment, and each head adds the
// popcounts of the live / hit / neg ballots under its segment's lane mask — one integer atomicAdd
// per non-zero (segment, counter), so the tables do not depend on the order of execution.
// table: n_in | n_hit | n_neg, each [n_det][n_obj].
__global__ __launch_bounds__(TILE) void k_assoc_vote(const ObjDesc* __restrict__ desc, const Tile* __restrict__ tiles,
                                                     const int* __restrict__ n_tiles,
                                                     const float4* __restrict__ cand, const float* __restrict__ dense,
                                                     int max_pts, int n_det, int n_obj, float tol,
                                                     int* __restrict__ table) {
  const int nt = *n_tiles;
  const int lane = threadIdx.x;
  const size_t plane = (size_t)n_det * n_obj;
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const Tile tl = tiles[t];
    const bool live = lane < tl.count;
    int d = -1;
    bool hit = false, neg = false;
    if (live) {
      const int off = desc[tl.obj].cand_off;
      const int i = __float_as_int(cand[off + tl.start + lane].w);
      const float y = dense[off + i];
      d = i / max_pts;
      hit = fabsf(y) <= tol;                 // (false for a NaN value: it counts in n_in only)
      neg = y < -tol;
    }
    const int prev = __shfl_up(d, 1, 64);
    const bool head = live && (lane == 0 || prev != d);
    const unsigned long long lb = __ballot(live), hb = __ballot(head), ib = __ballot(hit), nb = __ballot(neg);
    if (head) {
      const unsigned long long later = lane == 63 ? 0ull : (hb >> (lane + 1));       // the heads after this one
      const int end = later ? lane + __ffsll((long long)later) : 64;                 // first lane past the segment
      const unsigned long long upto = end >= 64 ? ~0ull : ((1ull << end) - 1ull);
      const unsigned long long mask = upto & ~((1ull << lane) - 1ull) & lb;
      int* at = table + (size_t)d * n_obj + tl.obj;
      const int n_in = __popcll(mask), n_hit = __popcll(ib & mask), n_neg = __popcll(nb & mask);
      atomicAdd(at, n_in);                                                           // (>= 1: the head itself)
      if (n_hit) atomicAdd(at + plane, n_hit);
      if (n_neg) atomicAdd(at + 2 * plane, n_neg);
    }
  }
}

// the better of two (hit, index) candidates first; index -1 is no candidate
struct AssocTop {
  int b, bh, s, sh;       // best and runner-up: index, n_hit
};
__device__ __forceinline__ void assoc_push(AssocTop& T, int i, int h) {
  if (i < 0) return;
  if (T.b < 0 || assoc_before(h, i, T.bh, T.b)) {
    T.s = T.b; T.sh = T.bh;
    T.b = i; T.bh = h;
  } else if (T.s < 0 || assoc_before(h, i, T.sh, T.s)) {
    T.s = i; T.sh = h;
  }
}

// Pick: one wave per detection, lanes striding over the objects; each lane keeps its two best,
// the wave merges them by a butterfly.  (more hits, then the lower index) is a total order on the
// objects, so the two best of the union are the same whatever the order of the merges.
__global__ __launch_bounds__(64) void k_assoc_pick(dsr_assoc_params A, int n_det, int n_obj,
                                                   const int* __restrict__ table, const int* __restrict__ cnt,
                                                   const dsr_frame_det_out* __restrict__ recs,
                                                   dsr_assoc_out* __restrict__ out) {
  const int j = blockIdx.x, lane = threadIdx.x;
  const size_t plane = (size_t)n_det * n_obj;
  const int* thit = table + plane + (size_t)j * n_obj;
  AssocTop T{-1, 0, -1, 0};
  for (int i = lane; i < n_obj; i += 64) assoc_push(T, i, thit[i]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int ob = __shfl_xor(T.b, m, 64), obh = __shfl_xor(T.bh, m, 64);
    const int os = __shfl_xor(T.s, m, 64), osh = __shfl_xor(T.sh, m, 64);
    assoc_push(T, ob, obh);
    assoc_push(T, os, osh);
  }
  if (lane != 0) return;
  const int n_pts = recs ? recs[j].n_pts : cnt[j];
  dsr_assoc_out o;
  const int in = T.b >= 0 ? table[(size_t)j * n_obj + T.b] : 0;
  const int neg = T.b >= 0 ? table[2 * plane + (size_t)j * n_obj + T.b] : 0;
  assoc_decide(A, n_pts, T.b, T.bh, in, neg, T.s, T.sh, &o);
  if (recs) {
    o.ingest_status = recs[j].status;
    o.n_mask = recs[j].n_mask;
    o.n_valid = recs[j].n_valid;
  }
  out[j] = o;
}

// ---------------------------------------------------------------------------------------------
// the blocks of one call: what goes up through the pinned half (cnt | desc | rows), what the
// device half holds (cnt | table | recs) and what comes back into the pinned half (table | recs)
struct AssocLayout {
  size_t cnt, desc, rows, table, recs, host_bytes;       // offsets into the pinned half
  size_t d_cnt, d_table, d_recs, dev_bytes;              // offsets into the device half
};
inline AssocLayout assoc_layout(int n_det, int n_obj, size_t row_floats) {
  AssocLayout L{};
  const size_t nd = (size_t)(n_det > 0 ? n_det : 1), no = (size_t)(n_obj > 0 ? n_obj : 1);
  const size_t b_cnt = frame_up256(sizeof(int) * nd), b_desc = frame_up256(sizeof(ObjDesc) * no),
               b_rows = frame_up256(sizeof(float) * (row_floats ? row_floats : 1)),
               b_table = frame_up256(sizeof(int) * 3 * nd * no), b_recs = frame_up256(sizeof(dsr_assoc_out) * nd);
  L.cnt = 0;
  L.desc = L.cnt + b_cnt;
  L.rows = L.desc + b_desc;
  L.table = L.rows + b_rows;
  L.recs = L.table + b_table;
  L.host_bytes = L.recs + b_recs;
  L.d_cnt = 0;
  L.d_table = b_cnt;
  L.d_recs = L.d_table + b_table;
  L.dev_bytes = L.d_recs + b_recs;
  return L;
}

}  // namespace dsr
