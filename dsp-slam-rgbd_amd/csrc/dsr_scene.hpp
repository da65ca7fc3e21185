// dsr_scene.hpp — the point-query sibling of the sphere tracer (dsr_scene_query):
// world points against every object of a map at once — MapObject::compute_sdf_loss /
// compute_sdf_loss_of_all_inside_points (src/MapObject_util.cc:9-69) and the planner's per-vertex
// collision check (src/NbvGenerator.cpp:320-327) without the per-object host loop.  Each (point,
// object) pair is transformed and tested against the object's unit ball, the candidates of each
// object are compacted in point order into 64-point decoder tiles, decoded by the exact forward
// kernel (k_mlp_fwd16, unchanged) and composited by a 64-bit atomicMin; the winners go through the
// Jacobian kernel's query tiles for the world-frame gradient.
//
// Layout of one pass (k objects of the query, k * n_pts pairs within the pair buffers):
//   chunk c of the pass = 256 consecutive points of ONE object: slot c / nc, points (c % nc) * 256..
//                         (nc = ceil(n_pts / 256); every object has the same chunks, so there is
//                         no chunk table)
//   ccnt [chunk]        candidates of the chunk;  gpos [chunk] their exclusive scan over the pass
//   cand [pair slot]    float4 (x, y, z, bits(point index)) of the candidates, compacted per object
//                       in point order at slot * n_pts
//   dense[pair slot]    the decoded value of point p of the object at slot * n_pts + p
//   part [tile]         per-tile partial sums (fixed order), reduced per object in tile order
//   keys [point]        (ord(d) << 32) | object index, atomicMin; persists over the passes
#pragma once
#include "dsr_dev.hpp"
#include "dsr_render.hpp"

namespace dsr {

constexpr int SCHUNK = 256;       // points per chunk = threads per workgroup of the pair kernels
constexpr unsigned long long SKEY_EMPTY = ~0ull;

struct SceneObj {
  float T[12];           // rows 0..2 of inverse(t_world_obj) (world -> object), row-major: A | t
  float s;               // det(R)^(1/3)
  int pad[3];
};

struct ScenePart {        // one decoded tile's sums, in the tile's fixed order
  double sum, sum_abs;
  int n_neg, n_nan;
};

struct SceneSums {        // one object's sums over its tiles, in tile order
  double sum, sum_abs;
  int n_neg, n_nan;
};

// x_k = fmaf(A_k0, p_x, fmaf(A_k1, p_y, fmaf(A_k2, p_z, t_k))) — the same three operations as
// dsr_scene_bin_host, so membership and coordinates are bitwise the host's
__device__ __forceinline__ float3 sc_point(const SceneObj& o, const float* __restrict__ p) {
  const float px = p[0], py = p[1], pz = p[2];
  float3 x;
  x.x = fmaf(o.T[0], px, fmaf(o.T[1], py, fmaf(o.T[2], pz, o.T[3])));
  x.y = fmaf(o.T[4], px, fmaf(o.T[5], py, fmaf(o.T[6], pz, o.T[7])));
  x.z = fmaf(o.T[8], px, fmaf(o.T[9], py, fmaf(o.T[10], pz, o.T[11])));
  return x;
}
// the in-ball rule of loss.py:82 on the squared norm (a non-finite point gives inf or NaN: false)
__device__ __forceinline__ int sc_in_ball(const float3& x) {
  const float r2 = fmaf(x.x, x.x, fmaf(x.y, x.y, x.z * x.z));
  return r2 < 1.0f;
}
// the monotone map of float bits to unsigned: flip the sign bit of non-negatives, invert negatives
__device__ __forceinline__ unsigned sc_ord(float d) {
  const unsigned b = __float_as_uint(d);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sc_unord(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ int sc_won(unsigned long long k, int obj) {
  return k != SKEY_EMPTY && (int)(unsigned)(k & 0xffffffffull) == obj;
}

// Bin: chunk = 256 points of one object; transform, test, the chunk's candidate count.
// grid = k * nc, block = SCHUNK
__global__ __launch_bounds__(SCHUNK) DSR_NO_PK_F32 void k_sc_bin(int obj0, int nc, int n_pts,
                                                                  const SceneObj* __restrict__ objs,
                                                                  const float* __restrict__ pts,
                                                                  int* __restrict__ ccnt) {
  const int slot = blockIdx.x / nc, i = (blockIdx.x % nc) * SCHUNK + (int)threadIdx.x;
  int live = 0;
  if (i < n_pts) live = sc_in_ball(sc_point(objs[obj0 + slot], pts + (size_t)i * 3));
  const int n = __syncthreads_count(live);
  if (threadIdx.x == 0) ccnt[blockIdx.x] = n;
}

// Winners: the chunk's points whose nearest object this is (keys); n_win by one atomic per chunk.
__global__ __launch_bounds__(SCHUNK) void k_sc_winners(int obj0, int nc, int n_pts,
                                                        const unsigned long long* __restrict__ keys,
                                                        int* __restrict__ ccnt, int* __restrict__ nwin) {
  const int slot = blockIdx.x / nc, i = (blockIdx.x % nc) * SCHUNK + (int)threadIdx.x;
  const int live = i < n_pts && sc_won(keys[i], obj0 + slot);
  const int n = __syncthreads_count(live);
  if (threadIdx.x == 0) {
    ccnt[blockIdx.x] = n;
    if (n) atomicAdd(nwin + obj0 + slot, n);
  }
}

// Scan (one workgroup): k_rt_scan's two scans without its RenderObj chunk table and march
// statistics — the scene's chunks are uniform (nc per object), so an object's range is slot * nc.
// gpos = exclusive scan of the pass's chunk counts; per object its count and the first of its
// 64-point tiles (tiles never mix objects); the tile count for the decode launch.
__global__ __launch_bounds__(RT_SCAN_THREADS) void k_sc_scan(int n_chunk, int nc, int obj0, int n_obj,
                                                             const int* __restrict__ ccnt, int* __restrict__ gpos,
                                                             int* __restrict__ ocount, int* __restrict__ otile,
                                                             int* __restrict__ n_tiles) {
  __shared__ int ws[17];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int c0 = 0; c0 < n_chunk; c0 += RT_SCAN_THREADS) {
    const int c = c0 + tid;
    const int v = c < n_chunk ? ccnt[c] : 0;
    int tot;
    const int ex = rt_block_scan(v, ws, tid, &tot);
    if (c < n_chunk) gpos[c] = carry + ex;
    carry += tot;
  }
  const int total = carry;
  __syncthreads();                       // gpos of every chunk is written (same workgroup)
  int tcarry = 0;
  for (int o0 = 0; o0 < n_obj; o0 += RT_SCAN_THREADS) {
    const int o = o0 + tid;
    int live = 0;
    if (o < n_obj) {
      const int a = o * nc, e = a + nc;
      live = (e < n_chunk ? gpos[e] : total) - gpos[a];
    }
    const int nt = (live + TILE - 1) / TILE;
    int tot;
    const int ex = rt_block_scan(nt, ws, tid, &tot);
    if (o < n_obj) {
      ocount[obj0 + o] = live;
      otile[obj0 + o] = tcarry + ex;
    }
    tcarry += tot;
  }
  if (tid == 0) *n_tiles = tcarry;
}

// Emit: each object's candidates (winners == 0) or winners (winners == 1), in point order, to
// float4 (x, point index) and the object's tiles.  winners == 0: candidates at slot * n_pts, tiles
// of the forward kernel {object, 0, position, count} (start relative to ObjDesc.cand_off);
// winners == 1: at 64 x the object's first tile, query tiles of the Jacobian kernel (term 2,
// absolute start).
__global__ __launch_bounds__(SCHUNK) DSR_NO_PK_F32 void k_sc_emit(int obj0, int nc, int n_pts,
                                                                   const SceneObj* __restrict__ objs,
                                                                   const float* __restrict__ pts,
                                                                   const unsigned long long* __restrict__ keys,
                                                                   const int* __restrict__ gpos,
                                                                   const int* __restrict__ ocount,
                                                                   const int* __restrict__ otile,
                                                                   float4* __restrict__ cand, Tile* __restrict__ tiles,
                                                                   int winners) {
  __shared__ int wsum[SCHUNK / 64];
  const int slot = blockIdx.x / nc, obj = obj0 + slot;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i = (blockIdx.x % nc) * SCHUNK + tid;
  float3 x = make_float3(0.f, 0.f, 0.f);
  int live = 0;
  if (i < n_pts) {
    x = sc_point(objs[obj], pts + (size_t)i * 3);
    live = winners ? sc_won(keys[i], obj) : sc_in_ball(x);
  }
  const int inc = wave_incl_scan(live, lane);
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  if (!live) return;
  int pos = gpos[blockIdx.x] - gpos[slot * nc] + inc - 1;
  for (int k = 0; k < wv; ++k) pos += wsum[k];
  const int base = winners ? otile[obj] * TILE : slot * n_pts;
  cand[base + pos] = make_float4(x.x, x.y, x.z, __int_as_float(i));
  if (pos % TILE == 0) {
    const int n = ocount[obj];
    tiles[otile[obj] + pos / TILE] =
        Tile{obj, winners ? 2 : 0, winners ? base + pos : pos, n - pos < TILE ? n - pos : TILE};
  }
}

// sum of v over the wave in a fixed order (butterfly: every lane ends with the same value)
__device__ __forceinline__ double sc_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int sc_wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Min: per decoded tile (one wave each) the composite d = s * f into the point keys (NaN values
// are skipped and counted) and the tile's partial sums of f, |f| and the f < 0 count.
__global__ __launch_bounds__(TILE) void k_sc_min(const SceneObj* __restrict__ objs, const ObjDesc* __restrict__ desc,
                                                 const Tile* __restrict__ tiles, const int* __restrict__ n_tiles,
                                                 const float4* __restrict__ cand, const float* __restrict__ dense,
                                                 unsigned long long* __restrict__ keys,
                                                 ScenePart* __restrict__ part) {
  const int nt = *n_tiles;
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const Tile tl = tiles[t];
    const int p = threadIdx.x;
    double f = 0.0;
    int neg = 0, nan = 0;
    if (p < tl.count) {
      const int off = desc[tl.obj].cand_off;
      const int i = __float_as_int(cand[off + tl.start + p].w);
      const float y = dense[off + i];
      if (y != y) {
        nan = 1;
      } else {
        const float d = objs[tl.obj].s * y;
        atomicMin(keys + i, ((unsigned long long)sc_ord(d) << 32) | (unsigned long long)(unsigned)tl.obj);
        f = (double)y;
        neg = y < 0.f;
      }
    }
    const double s = sc_wave_sum(f), sa = sc_wave_sum(fabs(f));
    const int nn = sc_wave_sum(neg), nq = sc_wave_sum(nan);
    if (p == 0) part[t] = ScenePart{s, sa, nn, nq};
  }
}

// Sums: one wave per object of the pass; lane l adds tiles l, l + 64, .. of the object in order,
// then the wave's fixed-order sum — the result depends on the object's tiles only.
__global__ __launch_bounds__(64) void k_sc_sums(int obj0, const int* __restrict__ ocount, const int* __restrict__ otile,
                                                const ScenePart* __restrict__ part, SceneSums* __restrict__ sums) {
  const int obj = obj0 + blockIdx.x;
  const int nt = (ocount[obj] + TILE - 1) / TILE, t0 = otile[obj];
  double s = 0.0, sa = 0.0;
  int nn = 0, nq = 0;
  for (int t = threadIdx.x; t < nt; t += 64) {
    const ScenePart q = part[t0 + t];
    s += q.sum;
    sa += q.sum_abs;
    nn += q.n_neg;
    nq += q.n_nan;
  }
  s = sc_wave_sum(s);
  sa = sc_wave_sum(sa);
  nn = sc_wave_sum(nn);
  nq = sc_wave_sum(nq);
  if (threadIdx.x == 0) sums[obj] = SceneSums{s, sa, nn, nq};
}

// Resolve: the point keys to dist / obj (+inf, -1 where the point is in no ball).
__global__ __launch_bounds__(256) void k_sc_resolve(const unsigned long long* __restrict__ keys, int n_pts,
                                                    float* __restrict__ dist, int* __restrict__ obj) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  const unsigned long long k = keys[p];
  const bool hit = k != SKEY_EMPTY;
  dist[p] = hit ? sc_unord((unsigned)(k >> 32)) : __builtin_inff();
  obj[p] = hit ? (int)(unsigned)(k & 0xffffffffull) : -1;
}

// Grad: the Jacobian kernel's query output (sdf, d/dcode (64), d/dxyz (3) per point) at the
// winners -> grad_k = s * fmaf(A_0k, g_0, fmaf(A_1k, g_1, A_2k * g_2)) at the winner's point.
__global__ __launch_bounds__(TILE) DSR_NO_PK_F32 void k_sc_grad(const SceneObj* __restrict__ objs,
                                                                const Tile* __restrict__ tiles,
                                                                const int* __restrict__ n_tiles,
                                                                const float4* __restrict__ cand,
                                                                const float* __restrict__ raw,
                                                                float* __restrict__ grad) {
  const int nt = *n_tiles;
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const Tile tl = tiles[t];
    const int p = threadIdx.x;
    if (p >= tl.count) continue;
    const SceneObj& o = objs[tl.obj];
    const int i = __float_as_int(cand[tl.start + p].w);
    const float* g = raw + (size_t)(tl.start + p) * (IN + 1) + 1 + CODE;
    const float g0 = g[0], g1 = g[1], g2 = g[2];
    float* out = grad + (size_t)i * 3;
    out[0] = o.s * fmaf(o.T[0], g0, fmaf(o.T[4], g1, o.T[8] * g2));
    out[1] = o.s * fmaf(o.T[1], g0, fmaf(o.T[5], g1, o.T[9] * g2));
    out[2] = o.s * fmaf(o.T[2], g0, fmaf(o.T[6], g1, o.T[10] * g2));
  }
}

}  // namespace dsr
