// dsr_mesh.hpp — batched mesh extraction (dsr_mesher_run_batch): the sign pass
// over the lite volumes, the exact band tiles, and marching cubes for all slots at once.
//
// Marching cubes (dsr_mc.hpp) reads two things from a volume: the predicate v < level at every
// voxel, and the values at both ends of every crossing edge.  So one lite (fp16) decode of the
// grid settles the predicate wherever the lite value is further than a margin m from the level,
// and only the band around the surface needs the exact decoder.  The exact kernels scale every
// 64-point tile from the tile's own maximum, so whole tiles of the per-code mesher's tiling are
// decoded: every exact value is then bit for bit the one dsr_mesher_run computes, and if every
// lite error is below m the meshes are bitwise those of the per-code path.
//
//   k_mesh_mark     band B = {not finite, |y - level| < m, flagged by the lite kernel}; a voxel
//                   needs an exact value if it or a grid neighbour is in B, or a neighbour outside
//                   B lies on the other side of the level.  A tile with such a voxel is needed
//                   (flag 1); a tile with a voxel in the shell m <= |y - level| < 2m, or in a
//                   hashed 2^-7 share of the rest, is audited (flag 2) — decoded too, as evidence.
//   k_mesh_compact  the flagged tiles, in order, into the exact kernel's tile table (the scan is
//                   dsr_mc.hpp's; no atomics, no host round trip)
//   k_mesh_merge    final = exact where the tile was decoded, lite elsewhere; per slot the largest
//                   |lite - exact| and the decoded voxels outside B whose exact side differs
//   k_mesh_redo     slots with a violation or an error above m / 4: all their other tiles, into a
//                   second table the exact kernel runs next (empty when the guard holds)
//   k_mcb_*         dsr_mc.hpp's edge / cell / vertex / face kernels with the slot as grid.y; flags
//                   and counts are concatenated per slot, so one scan each orders all meshes
#pragma once
#include "dsr_mc.hpp"

namespace dsr {

constexpr int MESH_AUDIT_LOG2 = 7;

// per-run counters (ints) of a pass, zeroed by k_mesh_begin
enum { MS_AUDIT_TILES = 0, MS_REDO_TILES, MS_REDO_SLOTS, MS_INTS };

__device__ __forceinline__ bool mesh_in_band(float y, unsigned char r, float level, float m) {
  return r != 0 || !(fabsf(y - level) >= m) || !(fabsf(y) <= 3.0e38f);
}

// one workgroup: the pass's read-back record zeroed and its tile counts (lite tiles, all exact
// tiles) written on the stream, so a run uploads nothing but the codes
__global__ void k_mesh_begin(int* __restrict__ rb, int n_rb, int* __restrict__ cnt, int n_lite, int n_all) {
  for (int i = threadIdx.x; i < n_rb; i += blockDim.x) rb[i] = 0;
  __syncthreads();
  if (threadIdx.x == 0) { cnt[0] = n_lite; cnt[1] = n_all; }
}

// one wave per 64-point tile; grid (ceil(nt / 4), slots), 256 threads
__global__ __launch_bounds__(256) void k_mesh_mark(const float* __restrict__ lite,
                                                   const unsigned char* __restrict__ refine, int d, int n,
                                                   int np, int nt, float level, float m,
                                                   unsigned char* __restrict__ tflag, int* __restrict__ tmark,
                                                   int* __restrict__ stat) {
  const int slot = blockIdx.y, lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const float* v = lite + (size_t)slot * np;
  const unsigned char* rf = refine + (size_t)slot * np;
  bool need = false, shell = false;
  const int p = t * TILE + lane;
  if (t < nt && p < n) {
    const int i = p / (d * d), j = (p / d) % d, k = p % d;
    const float y = v[p];
    const bool b = mesh_in_band(y, rf[p], level, m);
    const bool in = mc_inside(y, level);
    need = b;
    shell = !b && fabsf(y - level) < 2.f * m;
    const int step[3] = {d * d, d, 1};
    const int c[3] = {i, j, k};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int sg = -1; sg <= 1; sg += 2) {
        if (c[a] + sg < 0 || c[a] + sg >= d) continue;
        const int q = p + sg * step[a];
        const float yq = v[q];
        need |= mesh_in_band(yq, rf[q], level, m) || (mc_inside(yq, level) != in);
      }
    }
  }
  const bool any_need = __ballot(need) != 0ull, any_shell = __ballot(shell) != 0ull;
  int audit = 0;
  if (t < nt && lane == 0) {
    const unsigned h = (unsigned)(slot * nt + t) * 2654435761u;
    const bool au = !any_need && (any_shell || (h >> (32 - MESH_AUDIT_LOG2)) == 0u);
    tflag[(size_t)slot * nt + t] = any_need ? 1 : (au ? 2 : 0);
    tmark[(size_t)slot * nt + t] = (any_need || au) ? 1 : 0;
    audit = au ? 1 : 0;
  }
  // the audited-tile count is a statistic only (one add per workgroup)
  __shared__ int sh[4];
  if (lane == 0) sh[threadIdx.x >> 6] = audit;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int a = sh[0] + sh[1] + sh[2] + sh[3];
    if (a) atomicAdd(stat + MS_AUDIT_TILES, a);
  }
}

// flagged tiles, in (slot, tile) order, into the exact kernel's table
__global__ void k_mesh_compact(const int* __restrict__ tmark, const int* __restrict__ tpos, int nt, int n,
                               int total, Tile* __restrict__ tiles) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total || !tmark[i]) return;
  const int slot = i / nt, t = i - slot * nt;
  tiles[tpos[i]] = Tile{slot, 0, t * TILE, min(TILE, n - t * TILE)};
}

// final volume in place of the exact one; grid (ceil(n / 256), slots)
__global__ __launch_bounds__(256) void k_mesh_merge(const float* __restrict__ lite,
                                                    const unsigned char* __restrict__ refine,
                                                    const unsigned char* __restrict__ tflag, int n, int np,
                                                    int nt, float level, float m, float* __restrict__ vol,
                                                    int* __restrict__ slot_err, int* __restrict__ slot_viol) {
  const int slot = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  float err = 0.f;
  int viol = 0;
  if (p < n) {
    const size_t o = (size_t)slot * np + p;
    const float yl = lite[o];
    if (tflag[(size_t)slot * nt + p / TILE]) {
      const float ye = vol[o];
      const float e = fabsf(yl - ye);
      if (e <= 3.0e38f) err = e;               // (a lite value that is not finite is in the band)
      viol = !mesh_in_band(yl, refine[o], level, m) && (mc_inside(yl, level) != mc_inside(ye, level));
    } else {
      vol[o] = yl;
    }
  }
  __shared__ float se[4];
  __shared__ int sv[4];
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    err = fmaxf(err, __shfl_xor(err, w));
    viol += __shfl_xor(viol, w);
  }
  if ((threadIdx.x & 63) == 0) { se[threadIdx.x >> 6] = err; sv[threadIdx.x >> 6] = viol; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float e = fmaxf(fmaxf(se[0], se[1]), fmaxf(se[2], se[3]));
    const int vv = sv[0] + sv[1] + sv[2] + sv[3];
    if (e > 0.f) atomicMax(slot_err + slot, __float_as_int(e));   // non-negative floats order as ints
    if (vv) atomicAdd(slot_viol + slot, vv);
  }
}

// one workgroup: the slots the guard rejects (a violation, or an error above m / 4) get every tile
// the sign pass left out, in order, into the redo table
__global__ __launch_bounds__(MC_SCAN_BLOCK) void k_mesh_redo(const int* __restrict__ slot_err,
                                                             const int* __restrict__ slot_viol, int ns, int nt,
                                                             int n, float m, const unsigned char* __restrict__ tflag,
                                                             Tile* __restrict__ tiles, int* __restrict__ n_tiles,
                                                             int* __restrict__ slot_redo,
                                                             int* __restrict__ stat) {
  __shared__ int sh[MC_SCAN_BLOCK / 64 + 1];
  int base = 0, slots = 0;
  for (int s = 0; s < ns; ++s) {
    const bool bad = slot_viol[s] > 0 || __int_as_float(slot_err[s]) > 0.25f * m;
    if (threadIdx.x == 0) slot_redo[s] = bad ? 1 : 0;
    if (!bad) continue;
    ++slots;
    for (int c0 = 0; c0 < nt; c0 += MC_SCAN_BLOCK) {
      const int t = c0 + threadIdx.x;
      const int mk = (t < nt && tflag[(size_t)s * nt + t] == 0) ? 1 : 0;
      int total;
      const int r = block_excl_scan(mk, sh, total);
      if (mk) tiles[base + r] = Tile{s, 0, t * TILE, min(TILE, n - t * TILE)};
      base += total;
    }
  }
  if (threadIdx.x == 0) {
    *n_tiles = base;
    stat[MS_REDO_TILES] = base;
    stat[MS_REDO_SLOTS] = slots;
  }
}

// ---- marching cubes over `ns` volumes (slot = blockIdx.y; volume pitch np, flags 3n, cells nc)
__global__ void k_mcb_edges(const float* __restrict__ vol, int d, int np, float level, int* __restrict__ flag) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = d * d * d;
  if (p >= n) return;
  const float* v = vol + (size_t)blockIdx.y * np;
  int* f = flag + (size_t)blockIdx.y * 3 * n;
  const int i = p / (d * d), j = (p / d) % d, k = p % d;
  const bool in0 = mc_inside(v[p], level);
  f[p * 3 + 0] = (i + 1 < d) && (in0 != mc_inside(v[p + d * d], level));
  f[p * 3 + 1] = (j + 1 < d) && (in0 != mc_inside(v[p + d], level));
  f[p * 3 + 2] = (k + 1 < d) && (in0 != mc_inside(v[p + 1], level));
}

__global__ void k_mcb_cells(const float* __restrict__ vol, int d, int np, float level, int* __restrict__ ntri) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = d - 1, nc = m * m * m;
  if (c >= nc) return;
  const int i = c / (m * m), j = (c / m) % m, k = c % m;
  ntri[(size_t)blockIdx.y * nc + c] = dsr_mc_ntri_dev[mc_case(vol + (size_t)blockIdx.y * np, d, i, j, k, level)];
}

// vidx / toff are scans over all slots' flags / counts: vertices and faces of all meshes come out
// concatenated in slot order; offs[slot] = the slot's first vertex
__global__ void k_mcb_verts(const float* __restrict__ vol, int d, int np, float level, double spacing,
                            const int* __restrict__ flag, const int* __restrict__ vidx,
                            float* __restrict__ verts, int* __restrict__ offs) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int ne = d * d * d * 3;
  if (e >= ne) return;
  const size_t ge = (size_t)blockIdx.y * ne + e;
  if (e == 0) offs[blockIdx.y] = vidx[ge];
  if (!flag[ge]) return;
  const float* v = vol + (size_t)blockIdx.y * np;
  const int p = e / 3, a = e - 3 * p;
  const int i = p / (d * d), j = (p / d) % d, k = p % d;
  const int q = p + (a == 0 ? d * d : (a == 1 ? d : 1));
  const double v0 = v[p], v1 = v[q];
  const double t = ((double)level - v0) / (v1 - v0);
  double c[3] = {(double)i, (double)j, (double)k};
  c[a] = c[a] + t;
  float* o = verts + (size_t)vidx[ge] * 3;
#pragma unroll
  for (int x = 0; x < 3; ++x) o[x] = (float)(-1.0 + c[x] * spacing);
}

// face indices are local to their mesh (vidx minus the slot's first vertex)
__global__ void k_mcb_faces(const float* __restrict__ vol, int d, int np, float level,
                            const int* __restrict__ vidx, const int* __restrict__ toff,
                            int* __restrict__ faces, int* __restrict__ offs) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = d - 1, nc = m * m * m;
  if (c >= nc) return;
  const float* v = vol + (size_t)blockIdx.y * np;
  const int* vi = vidx + (size_t)blockIdx.y * 3 * d * d * d;
  const size_t gc = (size_t)blockIdx.y * nc + c;
  if (c == 0) offs[blockIdx.y] = toff[gc];
  const int vbase = vi[0];
  const int i = c / (m * m), j = (c / m) % m, k = c % m;
  const int cs = mc_case(v, d, i, j, k, level);
  const int nt = dsr_mc_ntri_dev[cs];
  int* out = faces + (size_t)toff[gc] * 3;
  for (int t = 0; t < 3 * nt; ++t) {
    const int e = dsr_mc_tri_dev[cs][t];
    const int a = e >> 2, b = e & 3;
    const int u = (a + 1) % 3, w = (a + 2) % 3;
    int g[3] = {i, j, k};
    g[u] += b & 1;
    g[w] += (b >> 1) & 1;
    out[t] = vi[((g[0] * d + g[1]) * d + g[2]) * 3 + a] - vbase;
  }
}

}  // namespace dsr
