// dsr_render.hpp — the ray machinery of the sphere tracer (dsr_renderer_render):
// per-pixel rays of each object's image rectangle, their entry into the object's unit ball, the
// stable per-object compaction of the live rays into 64-point decoder tiles between two steps,
// the signed step itself with the nearest-hit composite, and the resolve / normal passes.  The
// decoding is done by the exact forward kernel (k_mlp_fwd16) and, for normals, by the Jacobian
// kernel's query tiles, both unchanged.
//
// Layout of one pass (objects whose rectangle areas fit in the renderer's 2*W*H ray slots):
//   objs  [n_obj]       RenderObj: T_oc, rectangle, first ray slot, first chunk
//   chunks[n_chunk]     RayChunk: 256 consecutive rays of ONE object (row-major in its rectangle)
//   lam, lam0, lam1, state [ray slot]   the ray's depth, its ball interval, RS_*
//   ccnt  [chunk]       live rays of the chunk;  gpos [chunk] their exclusive scan over the pass
//   cand  [ray slot]    float4 (x, y, z, bits(ray index in the object)) of the live rays,
//                       compacted per object in ray order at the object's first ray slot
//   dense [ray slot]    the decoded value of ray i of the object at first ray slot + i
//   keys  [W*H]         (float_bits(depth) << 32) | object index, atomicMin; persists over passes
#pragma once
#include "dsr_dev.hpp"

namespace dsr {

constexpr int RCHUNK = 256;       // rays per chunk = threads per workgroup of the ray kernels
enum { RS_MISS = 0, RS_LIVE = 1, RS_HIT = 2 };
enum { RC_BALL = 0, RC_HIT = 1, RC_UNCONV = 2, RC_VISIBLE = 3, RC_INTS = 4 };   // per-object counters
constexpr unsigned long long RKEY_EMPTY = ~0ull;

struct RenderCam {
  float fx, fy, cx, cy;
  int W, H;
};

struct RenderObj {
  float Toc[12];         // rows 0..2 of inverse(t_cam_obj) (camera -> object), row-major
  int u0, v0, w, h;      // image rectangle (w * h rays, row-major)
  int ray_off;           // first ray slot in the pass's ray arrays
  int chunk0, nchunk;    // its chunks (indices into the call's chunk array)
  int pad;
};

struct RayChunk {
  int obj, start;        // object (index in the call) and first ray of the chunk within it
};

struct RenderMarch {
  float hit_eps, damp;
  int last;              // 1: the last step — rays still live become misses, counted unconverged
};

// per-call march statistics, written by k_rt_scan (one workgroup: plain stores)
struct RenderStepStats {
  long long decoded;     // sum over steps of the live rays
  int steps_run;         // 1 + the last step that had a live ray (max over the passes)
  int max_live_last;     // live rays entering that step
};

// pixel (u, v) -> object-frame direction d = R_oc . ((u - cx) / fx, (v - cy) / fy, 1)
__device__ __forceinline__ float3 rt_dir(const RenderCam& C, const RenderObj& o, int i) {
  const int u = o.u0 + i % o.w, v = o.v0 + i / o.w;
  const float rx = ((float)u - C.cx) / C.fx, ry = ((float)v - C.cy) / C.fy;
  float3 d;
  d.x = (rx * o.Toc[0] + ry * o.Toc[1]) + o.Toc[2];
  d.y = (rx * o.Toc[4] + ry * o.Toc[5]) + o.Toc[6];
  d.z = (rx * o.Toc[8] + ry * o.Toc[9]) + o.Toc[10];
  return d;
}
__device__ __forceinline__ int rt_pixel(const RenderCam& C, const RenderObj& o, int i) {
  return (o.v0 + i / o.w) * C.W + o.u0 + i % o.w;
}
__device__ __forceinline__ float3 rt_point(const RenderObj& o, const float3& d, float lam) {
  return make_float3(o.Toc[3] + lam * d.x, o.Toc[7] + lam * d.y, o.Toc[11] + lam * d.z);
}

// Setup: every ray's interval [lam0, lam1] inside the object's unit ball; lam <- lam0.
// grid = the pass's chunks (chunks already offset to the pass), block = RCHUNK
__global__ __launch_bounds__(RCHUNK) DSR_NO_PK_F32 void k_rt_setup(RenderCam C, const RenderObj* __restrict__ objs,
                                                                   const RayChunk* __restrict__ chunks,
                                                                   float* __restrict__ lam, float* __restrict__ lam0,
                                                                   float* __restrict__ lam1, int* __restrict__ state,
                                                                   int* __restrict__ ccnt) {
  const RayChunk ch = chunks[blockIdx.x];
  const RenderObj o = objs[ch.obj];
  const int i = ch.start + (int)threadIdx.x;
  int live = 0;
  if (i < o.w * o.h) {
    const float3 d = rt_dir(C, o, i);
    const float ox = o.Toc[3], oy = o.Toc[7], oz = o.Toc[11];
    const float a = (d.x * d.x + d.y * d.y) + d.z * d.z;
    const float b = (ox * d.x + oy * d.y) + oz * d.z;
    const float c = ((ox * ox + oy * oy) + oz * oz) - 1.f;
    const float disc = b * b - a * c;
    float l0 = 0.f, l1 = 0.f;
    if (disc > 0.f) {
      const float sq = sqrtf(disc);
      l0 = (-b - sq) / a;
      l1 = (-b + sq) / a;
      live = 1;
    }
    const int s = o.ray_off + i;
    lam[s] = l0;
    lam0[s] = l0;
    lam1[s] = l1;
    state[s] = live ? RS_LIVE : RS_MISS;
  }
  const int n = __syncthreads_count(live);
  if (threadIdx.x == 0) ccnt[blockIdx.x] = n;
}

// Normal pass setup: the live rays are the pixels the object won (keys), at the winning depth.
__global__ __launch_bounds__(RCHUNK) void k_rt_winners(RenderCam C, const RenderObj* __restrict__ objs,
                                                       const RayChunk* __restrict__ chunks,
                                                       const unsigned long long* __restrict__ keys,
                                                       float* __restrict__ lam, int* __restrict__ state,
                                                       int* __restrict__ ccnt) {
  const RayChunk ch = chunks[blockIdx.x];
  const RenderObj o = objs[ch.obj];
  const int i = ch.start + (int)threadIdx.x;
  int live = 0;
  if (i < o.w * o.h) {
    const unsigned long long k = keys[rt_pixel(C, o, i)];
    live = k != RKEY_EMPTY && (int)(unsigned)(k & 0xffffffffull) == ch.obj;
    const int s = o.ray_off + i;
    lam[s] = live ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
    state[s] = live ? RS_LIVE : RS_MISS;
  }
  const int n = __syncthreads_count(live);
  if (threadIdx.x == 0) ccnt[blockIdx.x] = n;
}

// exclusive scan of v over a 1024-thread workgroup; *total = the sum (ws: 17 ints of LDS)
__device__ __forceinline__ int rt_block_scan(int v, int* ws, int tid, int* total) {
  const int lane = tid & 63, wv = tid >> 6;
  const int inc = wave_incl_scan(v, lane);
  __syncthreads();                       // (ws may still be read from the previous call)
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  if (wv == 0) {
    int s = lane < 16 ? ws[lane] : 0;
    s = wave_incl_scan(s, lane);
    if (lane < 16) ws[lane] = s;
  }
  __syncthreads();
  *total = ws[15];
  return (wv ? ws[wv - 1] : 0) + inc - v;
}

// Scan (one workgroup): gpos = exclusive scan of the pass's chunk counts; per object of the pass
// its live count and the first of its 64-point tiles (tiles never mix objects); the tile count
// for the decode launch; step >= 0: the march statistics (step 0: the rays that enter the ball).
constexpr int RT_SCAN_THREADS = 1024;
__global__ __launch_bounds__(RT_SCAN_THREADS) void k_rt_scan(int n_chunk, int chunk_base, int obj0, int n_obj,
                                                             const RenderObj* __restrict__ objs,
                                                             const int* __restrict__ ccnt, int* __restrict__ gpos,
                                                             int* __restrict__ olive, int* __restrict__ otile,
                                                             int* __restrict__ n_tiles, int step,
                                                             RenderStepStats* __restrict__ ss,
                                                             int* __restrict__ counters) {
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
      const RenderObj& ob = objs[obj0 + o];
      if (ob.nchunk > 0) {
        const int a = ob.chunk0 - chunk_base, e = a + ob.nchunk;
        live = (e < n_chunk ? gpos[e] : total) - gpos[a];
      }
    }
    const int nt = (live + TILE - 1) / TILE;
    int tot;
    const int ex = rt_block_scan(nt, ws, tid, &tot);
    if (o < n_obj) {
      olive[obj0 + o] = live;
      otile[obj0 + o] = tcarry + ex;
      if (step == 0) counters[(size_t)(obj0 + o) * RC_INTS + RC_BALL] = live;
    }
    tcarry += tot;
  }
  if (tid == 0) {
    *n_tiles = tcarry;
    if (step >= 0 && total > 0) {
      ss->decoded += total;
      if (step + 1 > ss->steps_run) {
        ss->steps_run = step + 1;
        ss->max_live_last = total;
      } else if (step + 1 == ss->steps_run && total > ss->max_live_last) {
        ss->max_live_last = total;
      }
    }
  }
}

// Emit: the live rays of each object, in ray order, to the object's candidate list and its tiles.
// normals == 0: candidates at the object's ray slots, tiles of the forward kernel (start relative
// to ObjDesc.cand_off); normals == 1: candidates at 64 x the object's first tile, query tiles of
// the Jacobian kernel (term 2, absolute start).
__global__ __launch_bounds__(RCHUNK) DSR_NO_PK_F32 void k_rt_emit(RenderCam C, const RenderObj* __restrict__ objs,
                                                                  const RayChunk* __restrict__ chunks, int chunk_base,
                                                                  const int* __restrict__ gpos,
                                                                  const int* __restrict__ olive,
                                                                  const int* __restrict__ otile,
                                                                  const int* __restrict__ state,
                                                                  const float* __restrict__ lam,
                                                                  float4* __restrict__ cand, Tile* __restrict__ tiles,
                                                                  int normals) {
  __shared__ int wsum[RCHUNK / 64];
  const RayChunk ch = chunks[blockIdx.x];
  const RenderObj o = objs[ch.obj];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int i = ch.start + tid;
  const bool in = i < o.w * o.h;
  const int live = in && state[o.ray_off + i] == RS_LIVE;
  const int inc = wave_incl_scan(live, lane);
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  if (!live) return;
  int pos = gpos[blockIdx.x] - gpos[o.chunk0 - chunk_base] + inc - 1;
  for (int k = 0; k < wv; ++k) pos += wsum[k];
  const float3 d = rt_dir(C, o, i);
  const float3 x = rt_point(o, d, lam[o.ray_off + i]);
  const int base = normals ? otile[ch.obj] * TILE : o.ray_off;
  cand[base + pos] = make_float4(x.x, x.y, x.z, __int_as_float(i));
  if (pos % TILE == 0) {
    const int n = olive[ch.obj];
    tiles[otile[ch.obj] + pos / TILE] =
        Tile{ch.obj, normals ? 2 : 0, normals ? base + pos : pos, n - pos < TILE ? n - pos : TILE};
  }
}

// Advance: a live ray whose decoded |y| < hit_eps is a hit at its depth and competes for its
// pixel; otherwise lam += damp * y / |d| (signed), and a ray that leaves [lam0, lam1] is a miss.
__global__ __launch_bounds__(RCHUNK) DSR_NO_PK_F32 void k_rt_advance(RenderCam C, const RenderObj* __restrict__ objs,
                                                                     const RayChunk* __restrict__ chunks,
                                                                     const float* __restrict__ dense,
                                                                     float* __restrict__ lam,
                                                                     const float* __restrict__ lam0,
                                                                     const float* __restrict__ lam1,
                                                                     int* __restrict__ state,
                                                                     unsigned long long* __restrict__ keys,
                                                                     int* __restrict__ counters, int* __restrict__ ccnt,
                                                                     RenderMarch M) {
  const RayChunk ch = chunks[blockIdx.x];
  const RenderObj o = objs[ch.obj];
  const int i = ch.start + (int)threadIdx.x;
  int live = 0, hit = 0, unc = 0;
  if (i < o.w * o.h) {
    const int s = o.ray_off + i;
    if (state[s] == RS_LIVE) {
      const float y = dense[s];
      const float l = lam[s];
      if (fabsf(y) < M.hit_eps) {
        hit = 1;
        state[s] = RS_HIT;
        atomicMin(keys + rt_pixel(C, o, i),
                  ((unsigned long long)__float_as_uint(l) << 32) | (unsigned long long)(unsigned)ch.obj);
      } else {
        const float3 d = rt_dir(C, o, i);
        const float nd = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
        const float ln = l + (M.damp * y) / nd;
        live = ln >= lam0[s] && ln <= lam1[s];          // (a NaN leaves too)
        if (live && M.last) {
          live = 0;
          unc = 1;
        }
        lam[s] = ln;
        if (!live) state[s] = RS_MISS;
      }
    }
  }
  const int nl = __syncthreads_count(live);
  const int nh = __syncthreads_count(hit);
  const int nu = __syncthreads_count(unc);
  if (threadIdx.x == 0) {
    ccnt[blockIdx.x] = nl;
    if (nh) atomicAdd(counters + (size_t)ch.obj * RC_INTS + RC_HIT, nh);
    if (nu) atomicAdd(counters + (size_t)ch.obj * RC_INTS + RC_UNCONV, nu);
  }
}

// Resolve: the pixel keys to the depth and instance images.
__global__ __launch_bounds__(256) void k_rt_resolve(const unsigned long long* __restrict__ keys, int npix,
                                                    float* __restrict__ depth, int* __restrict__ inst) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  const unsigned long long k = keys[p];
  const bool hit = k != RKEY_EMPTY;
  depth[p] = hit ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
  inst[p] = hit ? (int)(unsigned)(k & 0xffffffffull) : -1;
}

// n_visible: the pixels of each object's rectangle that carry its index (grid = all chunks of the call)
__global__ __launch_bounds__(RCHUNK) void k_rt_visible(RenderCam C, const RenderObj* __restrict__ objs,
                                                       const RayChunk* __restrict__ chunks,
                                                       const int* __restrict__ inst, int* __restrict__ counters) {
  const RayChunk ch = chunks[blockIdx.x];
  const RenderObj o = objs[ch.obj];
  const int i = ch.start + (int)threadIdx.x;
  const int mine = i < o.w * o.h && inst[rt_pixel(C, o, i)] == ch.obj;
  const int n = __syncthreads_count(mine);
  if (threadIdx.x == 0 && n) atomicAdd(counters + (size_t)ch.obj * RC_INTS + RC_VISIBLE, n);
}

// Normals: the Jacobian kernel's query output (sdf, d/dcode (64), d/dxyz (3) per point) at the
// winning hit points -> camera-frame normal normalize(R_oc^T g) at the point's pixel.
__global__ __launch_bounds__(TILE) DSR_NO_PK_F32 void k_rt_normals(RenderCam C, const RenderObj* __restrict__ objs,
                                                                   const Tile* __restrict__ tiles,
                                                                   const int* __restrict__ n_tiles,
                                                                   const float4* __restrict__ cand,
                                                                   const float* __restrict__ raw,
                                                                   float* __restrict__ normals) {
  const int nt = *n_tiles;
  for (int t = blockIdx.x; t < nt; t += gridDim.x) {
    const Tile tl = tiles[t];
    const int p = threadIdx.x;
    if (p >= tl.count) continue;
    const RenderObj& o = objs[tl.obj];
    const int i = __float_as_int(cand[tl.start + p].w);
    const float* g = raw + (size_t)(tl.start + p) * (IN + 1) + 1 + CODE;
    const float gx = g[0], gy = g[1], gz = g[2];
    const float nx = (o.Toc[0] * gx + o.Toc[4] * gy) + o.Toc[8] * gz;
    const float ny = (o.Toc[1] * gx + o.Toc[5] * gy) + o.Toc[9] * gz;
    const float nz = (o.Toc[2] * gx + o.Toc[6] * gy) + o.Toc[10] * gz;
    const float nn = sqrtf((nx * nx + ny * ny) + nz * nz);
    float* out = normals + (size_t)rt_pixel(C, o, i) * 3;
    const float inv = nn > 0.f ? 1.f / nn : 0.f;
    out[0] = nx * inv;
    out[1] = ny * inv;
    out[2] = nz * inv;
  }
}

}  // namespace dsr
