// dsr_mlp_lite.hpp — the one-product ("lite") decoder pass that classifies render samples.
//
// k_render only needs, for a ray sample, its occupancy 0.5 - clamp(sdf, +-th)/(2 th)
// (loss_utils.py:40-48) and whether |sdf| < th (loss.py:101): for sdf >= th the sample is
// exactly empty (o = 0), for sdf <= -th exactly full (o = 1), and only the samples in
// between need their SDF value.  The lite pass decodes every sample with one fp16 MFMA
// product (fp16(W) . fp16(H), fp32 accumulate: 1/3 of the split-fp16 MFMA work, half its
// weight bytes) on 128-point tiles (one fp16 image fits LDS twice as wide as the split
// kernels' two, halving the weight stream per point again), and
//   * writes its value to `dense` (a value outside the band has the class of the exact one),
//   * flags the ray dead when sdf <= -th - margin (certainly full: early termination),
//   * flags the sample for the exact split-fp16 pass when |sdf| < th + margin.
// The margin bounds the lite pass's error and calibrates itself per object (k_solve): th in
// the first GN iteration, then max(floor, safety x the largest |lite - exact| the object's
// own re-decoded samples have shown so far; 0.002 and 4) — the exact pass measures that
// error on every band sample it overwrites; a margin above 0.1 sends every sample to the
// exact pass.  The refined samples carry the exact values, so every occupancy, mask and
// de_do downstream is the split-fp16 one.
//
// One kernel, k_mlp_fwd_lite_st<SWZ, PIN>, in three schedules that give bitwise equal values
// (DSR_LITE_VARIANT, dsr_api.hip: lite_schedule):
//   472   <false, false>  gemm_lite_x, H image unswizzled
//   1496  <true,  false>  gemm_lite_x, H image swizzled (lite_swz_g)
//   3544  <true,  true>   gemm_lite_r (B ring pinned), H image swizzled; the default
// Layout: tile = 128 points, 512 threads; wave w owns rows 64w..64w+63 as 4 x 8 blocks of
// 16x16 accumulators; LDS image H[128][528] fp16; weights: the unscaled fp16 copy D.Wl_raw
// (one 1 KiB wave-load per row block and k step), streamed from L2 through a ring of two k
// steps that is carried across layers and tiles; biases and lin8's row in LDS, the bias
// seeding the accumulators, so an epilogue is a range check, an fp16 convert and a packed
// ReLU, and no vector global load waits behind the next layer's in-flight weight fragments
// (vmcnt counts in order).  Activations are stored unscaled: fp16 keeps 11 significant bits
// over 6e-5..65504, so only the range needs a guard — a tile in which a value reaches 2^15
// sends all its samples to the exact pass.  (The one-barrier-per-layer kernel these schedules
// were derived from, and its scaled-weight variants, are in git history; DESIGN.md appendix A.)
//
// Register discipline.  The accumulators take 128 of the wave's 256 VGPRs, so every other
// value live across a GEMM costs registers the rings need.  Lane-derived values (LDS
// addresses, shuffle indices, bias offsets) are re-derived per layer from an opaque copy of
// the lane id (`opaque`), so the compiler cannot hoist them out of the tile loop and keep ~60
// of them live through every GEMM (which it otherwise does).  Conditions that single out rows
// (lin4's xyz rows) are split into a wave-uniform branch + a per-lane select, never a
// per-element divergent branch.
#pragma once
#include <utility>
#include "dsr_dev.hpp"
#include "dsr_mlp.hpp"
#include "dsr_mlp16.hpp"

namespace dsr {

constexpr int LTILE = 128;

// `hook(t)` of the GEMMs below runs at the start of k step t, before that step's loads (the
// kernel's event waits and signals); the default does nothing.
struct NoHook {
  __device__ __forceinline__ void operator()(int) const {}
};

// acc[4][8] = bias rows + fp16(A rows of this wave) . H over K = 32*T, A = Wl (D.Wl_raw[l]:
// 1 KiB per row block and k step), read with buffer loads (one wave-uniform descriptor per
// matrix, the lane's 16-byte offset in one VGPR, the (row block, k step) offset in an SGPR).
// The A ring is two k steps deep and carried across GEMMs (every T is even, so step t of
// every matrix uses slot t % 2): on entry a[0] holds step 0 of this matrix, and the last step
// loads step 0 of the NEXT matrix (Wn, Tn k steps) into a[0], so that load's L2 latency hides
// behind this layer's last MFMAs and the epilogue instead of stalling the next layer's first
// MFMA.  B ring, 4 deep: the fragment of column block cb+3 (of this step or, past the last
// block, of the next one) is read from LDS as the MFMAs of block cb issue.
// `ci`: this wave's bias rows (4 row blocks x the lane's 4 rows).
// SWZ: H image swizzled — 16-B chunk index bit 0 XOR point bit 2 (lite_swz_g), a per-lane
// base offset here.
template <int T, bool SWZ, class Hook = NoHook>
__device__ __forceinline__ void gemm_lite_x(const _Float16* Wl, const _Float16* Wn, int Tn, int w,
                                            const _Float16* H, floatx4 (&acc)[4][8], half8 (&a)[2][4],
                                            int lane, const floatx4* ci, Hook hook = Hook{}) {
  const _Float16* base = Wl + (size_t)(4 * w) * T * 64 * 8;
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(base), 0, 4 * T * 1024, 0x00020000);
  const int voff = lane * 16;
  const int gsw = SWZ ? ((lane >> 4) ^ (((lane & 15) >> 2) & 1)) : (lane >> 4);
  const _Float16* B = H + (lane & 15) * PH + 8 * gsw;
  auto lda = [&](int q, int t) {
    return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, (q * T + t) * 1024, 0));
  };
  auto ldb = [&](int cb, int k32) { return *reinterpret_cast<const half8*>(B + cb * 16 * PH + k32); };
  half8 b[4];
  // the accumulators start as the bias rows, copied before the first step — holding the 16
  // bias registers live through step 0 instead (as its C operand) made the compiler spill
  // inside the tile loop: per-tile scratch stores whose dirty lines the weight stream then
  // evicts to HBM (+30 MB written per launch)
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      acc[q][cb] = ci[q];
      asm volatile("" : "+v"(acc[q][cb]));   // keep the copy (else folded back into the C operand)
    }
#pragma unroll
  for (int cb = 0; cb < 3; ++cb) b[cb] = ldb(cb, 0);
  auto step = [&](auto J, int t) {
    constexpr int j = decltype(J)::value;
    hook(t);
    if (t + 1 < T) {
#pragma unroll
      for (int q = 0; q < 4; ++q) a[j ^ 1][q] = lda(q, t + 1);
    }
    const int pc = 32 * t, pn = 32 * (t + 1);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      b[(cb + 3) & 3] = (cb + 3 < 8) ? ldb(cb + 3, pc) : ldb(cb - 5, pn);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[q][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[j][q], b[cb & 3], acc[q][cb], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
  };
  step(std::integral_constant<int, 0>{}, 0);
#pragma unroll 1
  for (int t0 = 1; t0 < T - 1; t0 += 2) {
    step(std::integral_constant<int, 1>{}, t0);
    step(std::integral_constant<int, 0>{}, t0 + 1);
  }
  {   // the next matrix's first step, into the slot step T-2 released
    const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<_Float16*>(Wn + (size_t)(4 * w) * Tn * 64 * 8), 0, 4 * Tn * 1024, 0x00020000);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      a[0][q] = __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rn, voff, q * Tn * 1024, 0));
  }
  step(std::integral_constant<int, 1>{}, T - 1);
}

// gemm_lite_x with the B ring pinned.  Left to itself the compiler folds gemm_lite_x's four B
// fragments onto two register tuples and sinks each ds_read next to the MFMAs that use it (a
// read, a wait for it, its four MFMAs, three times per k step), so a wave issuing alone stalls
// for the LDS latency every block.  Here
//   * a sched_barrier after each block's read keeps the read of column block cb+3 ahead of the
//     MFMAs of block cb (12 MFMAs of lead, 4 fragments live, lgkmcnt(3) waits), as gemm16_ring
//     does for the split kernels;
//   * the B addresses are two running element offsets (column blocks 0-3 and 4-7: the 1056-byte
//     pitch puts blocks 4-7 past the 16-bit DS offset of one base), advanced by one k step each;
//   * the last k step reads no B fragment past the image (gemm_lite_x reads three that nothing
//     uses) and the next matrix's first A fragments are requested before it like any k step's;
//   * the accumulators are seeded from the bias rows in LDS inside the GEMM (`bias`: this
//     layer's 512 floats), so the caller holds no bias registers.
// Same MFMAs, same operands, same k order per accumulator: values bitwise those of gemm_lite_x.
template <int T, bool SWZ, class Hook = NoHook>
__device__ __forceinline__ void gemm_lite_r(const _Float16* Wl, const _Float16* Wn, int Tn, int w,
                                            const _Float16* H, floatx4 (&acc)[4][8], half8 (&a)[2][4],
                                            int lane, const float* bias, Hook hook = Hook{}) {
  const _Float16* base = Wl + (size_t)(4 * w) * T * 64 * 8;
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(base), 0, 4 * T * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<_Float16*>(Wn + (size_t)(4 * w) * Tn * 64 * 8), 0, 4 * Tn * 1024, 0x00020000);
  const int voff = lane * 16;
  const int gsw = SWZ ? ((lane >> 4) ^ (((lane & 15) >> 2) & 1)) : (lane >> 4);
  int blo = (lane & 15) * PH + 8 * gsw;      // column blocks 0..3 of the current k step
  int bhi = blo + 64 * PH;                   // column blocks 4..7
  asm volatile("" : "+v"(blo), "+v"(bhi));   // two registers, not one base and an add per read
  auto lda = [&](int q, int t) {
    return __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, (q * T + t) * 1024, 0));
  };
  // block cb of the current k step (NEXT: of the one after it)
  auto ldb = [&](int cb, bool next) {
    return *reinterpret_cast<const half8*>(H + (cb < 4 ? blo : bhi) + (cb & 3) * 16 * PH + (next ? 32 : 0));
  };
  half8 b[4];
  // the accumulators start as the bias rows, one row block at a time, so 4 bias registers are
  // live at once and none into the first step
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const floatx4 bq = *reinterpret_cast<const floatx4*>(bias + 64 * w + 16 * q + 4 * (lane >> 4));
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      acc[q][cb] = bq;
      asm volatile("" : "+v"(acc[q][cb]));   // keep the copy (gemm_lite_x)
    }
  }
#pragma unroll
  for (int cb = 0; cb < 3; ++cb) b[cb] = ldb(cb, false);
  auto step = [&](auto J, auto LAST, int t) {
    constexpr int j = decltype(J)::value;
    constexpr bool last = decltype(LAST)::value;
    hook(t);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      a[j ^ 1][q] = last ? __builtin_bit_cast(half8, __builtin_amdgcn_raw_buffer_load_b128(rn, voff, q * Tn * 1024, 0))
                         : lda(q, t + 1);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      if (cb + 3 < 8) b[(cb + 3) & 3] = ldb(cb + 3, false);
      else if (!last) b[(cb + 3) & 3] = ldb(cb - 5, true);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[q][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[j][q], b[cb & 3], acc[q][cb], 0, 0, 0);
    }
    __builtin_amdgcn_s_setprio(0);
    blo += 32;
    bhi += 32;
  };
  step(std::integral_constant<int, 0>{}, std::false_type{}, 0);
#pragma unroll 1
  for (int t0 = 1; t0 < T - 1; t0 += 2) {
    step(std::integral_constant<int, 1>{}, std::false_type{}, t0);
    step(std::integral_constant<int, 0>{}, std::false_type{}, t0 + 1);
  }
  step(std::integral_constant<int, 1>{}, std::true_type{}, T - 1);
}

// H swizzle (SWZ): element (point p, k) at p * PH + (k ^ (8 * ((p >> 2) & 1))).  The
// 16-lane groups of the epilogue's 8-byte stores (one 4-row slice, 16 points at the 264-dword
// pitch) hit each bank 4 times unswizzled and twice swizzled; the 16-byte B reads stay
// conflict-free (their lane groups mix the two slices).  Only a per-lane offset changes.
__device__ __forceinline__ int lite_swz_g(int g, int c, bool swz) { return swz ? (g ^ (((c >> 2) & 1) << 1)) : g; }

// this wave's 64 rows x 128 points of fp32 values, as fp16, into the image
template <bool SWZ>
__device__ __forceinline__ void lite_write(floatx4 (&acc)[4][8], _Float16* H, int w, int lane) {
  const int c = lane & 15, g = lite_swz_g(lane >> 4, c, SWZ);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n0 = 64 * w + 16 * q + 4 * g;
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
      half4 h;
#pragma unroll
      for (int r = 0; r < 4; ++r) h[r] = (_Float16)accr(acc[q][cb], r);
      *reinterpret_cast<half4*>(H + (16 * cb + c) * PH + n0) = h;
    }
  }
}

// ------------------------------------------------------------------------------------
// Staggered groups.  With one barrier per layer all 8 waves would run their epilogues together
// and the MFMA pipes idle meanwhile.  Here waves 0-3 (group A: rows 0..255 = the next GEMM's k
// steps 0..7) and waves 4-7 (group B: rows 256..511 = k steps 8..15) synchronise through event
// counters in LDS instead, so B can trail A and each SIMD's two waves (w, w+4) overlap one
// wave's epilogue with the other's MFMAs.  The order in which waves run changes no value: every
// accumulator sees the same MFMAs in the same k order.  Events (monotonic; a wave adds 1 per
// event):
//   cH[g]  group g wrote its rows of the current image (or, at lin7, its part of `red`)
//   cRlo   a wave finished reading k steps 0..7 of a GEMM's input (signalled at step 8)
//   cRhi   a wave finished the GEMM (all its reads)
//   cP     an A wave reached k step `lag` of a GEMM (B starts a GEMM only then: the stagger)
//   cT[g]  group g's tile inputs (its xyz copy, its rows of the object's lin0/lin4 biases)
//   cE     a B wave finished a tile (B's xyz copy is read until the last B wave is done)
// Dependencies per GEMM: k steps 0..7 need cH[A], 8..15 cH[B] of the previous image; A may
// overwrite its rows once every wave passed step 8 (cRlo), B once every wave finished (cRhi).
// Every wait is bounded: a wave that waits ~2^16 polls marks the block broken, skips all
// further waits and sends every sample it classifies to the exact pass (results stay exact).
struct LiteStShared {
  _Float16 H[LTILE * PH];
  float xyz[2][LTILE * 4];     // per group
  float red[NWAVE * LTILE];
  float bias[8][HID];
  float w8[HID];
  int ovf[2];                  // per tile parity: (tile iteration + 1) if a value reached 2^15
  int cH[2], cRlo, cRhi, cP, cT[2], cE, broken, pad[7];
  unsigned twait[NWAVE];       // 100 MHz time at which a wave's current wait passed 1024 polls
  int rec[6];                  // the block's first expired wait: counter, target, observed, tile
                               // iteration, wave (-1: none), 100 MHz ticks
};

__device__ __forceinline__ void st_signal(int* c) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (__lane_id() == 0) __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  asm volatile("" ::: "memory");
}

#ifndef DSR_LITE_WAIT_LOG2
#define DSR_LITE_WAIT_LOG2 16
#endif
// The wave whose wait expires first breaks its block and notes in LDS which counter it waited
// on, the target and the value it saw, the tile iteration, itself, the real time its last
// 2^16 - 1024 polls took (a poll is one s_sleep 1 + one LDS load, ~0.1 us: far more time than
// that means the wave was not running).  (A snapshot of all counters here doubled the kernel's
// register spills, so the record holds the waited-on counter only.)
// At its exit the same wave counts the block in diag[STD_BROKEN] and, if it is the run's
// first, copies the note to diag (st_report) — the global writes stay out of the GEMM loop.
__device__ __forceinline__ void st_expire(int* c, int target, int observed, LiteStShared& sm, int it, int w) {
  int prev = 0;
  if (__lane_id() == 0) prev = __hip_atomic_exchange(&sm.broken, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  prev = __builtin_amdgcn_readfirstlane(prev);
  if (prev != 0 || __lane_id() != 0) return;
  sm.rec[0] = (int)(c - &sm.ovf[0]);
  sm.rec[1] = target;
  sm.rec[2] = observed;
  sm.rec[3] = it;
  sm.rec[5] = (int)((unsigned)__builtin_amdgcn_s_memrealtime() - sm.twait[w]);
  sm.rec[4] = w;
}

__device__ __forceinline__ void st_report(const LiteStShared& sm, int* diag, int w) {
  if (diag == nullptr || sm.rec[4] != w || __lane_id() != 0) return;
  atomicAdd(diag + STD_BROKEN, 1);
  if (atomicCAS(diag + STD_CLAIM, 0, 1) != 0) return;
  diag[STD_BLOCK] = (int)blockIdx.x;
  diag[STD_WAVE] = w;
  diag[STD_COUNTER] = sm.rec[0];
  diag[STD_TARGET] = sm.rec[1];
  diag[STD_OBSERVED] = sm.rec[2];
  diag[STD_IT] = sm.rec[3];
  diag[STD_HWID] = (int)__builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_ID: wave / SIMD / CU / SE
  diag[STD_XCC] = (int)__builtin_amdgcn_s_getreg((31 << 11) | 20);     // XCC_ID
  diag[STD_POLLS] = (1 << DSR_LITE_WAIT_LOG2) - 1024;
  diag[STD_REAL] = sm.rec[5];
  __threadfence();
}

__device__ __forceinline__ void st_wait(int* c, int target, LiteStShared& sm, int it, int w) {
  int n = 0;
  int v;
  while ((v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) <
         target) {
    if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(&sm.broken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)))
      break;
    ++n;
    if (n == 1024) sm.twait[w] = (unsigned)__builtin_amdgcn_s_memrealtime();   // a long wait: clock it
    if (n > (1 << DSR_LITE_WAIT_LOG2)) {
      st_expire(c, target, v, sm, it, w);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  asm volatile("" ::: "memory");
}

#ifdef DSR_EXP_STAMP   // diagnostic build (tools: exp_STAMP.so): per-wave cycles by phase, block 0-3
#define LSTAMP(cat)                                                         \
  {                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                      \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();            \
    stamp[cat] += t_ - stamp_last;                                          \
    stamp_last = t_;                                                        \
    __builtin_amdgcn_sched_barrier(0);                                      \
  }
#else
#define LSTAMP(cat)
#endif
// SWZ: the H image is swizzled (lite_swz_g); PIN: the GEMMs run gemm_lite_r, not gemm_lite_x.
template <bool SWZ, bool PIN>
__global__ __launch_bounds__(512) void k_mlp_fwd_lite_st(DevDecoder D, const Tile* __restrict__ tiles,
                                                         const int* __restrict__ n_tiles,
                                                         const ObjDesc* __restrict__ desc,
                                                         const float4* __restrict__ cand,
                                                         const float* __restrict__ bias0f,
                                                         const float* __restrict__ bias4f,
                                                         float* __restrict__ dense, ErtArgs E) {
  __shared__ LiteStShared sm;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = w >> 2;
  const int nt = *n_tiles;
  if ((int)blockIdx.x >= nt) return;     // no tile for this block: skip the prologue (small passes)
  const int lag = E.lag;
  half8 ring[2][4];
  {
    const int tid = opaque(threadIdx.x);
    for (int e = tid; e < 7 * HID; e += 512) {
      const int l = e / HID, n = e - l * HID;        // lin1..3, lin5..7, W8
      if (l < 6) sm.bias[l < 3 ? l + 1 : l + 2][n] = D.bias[l < 3 ? l + 1 : l + 2][n];
      else sm.w8[n] = D.W8[n];
    }
    if (tid < 18) {   // counters and flags; DSR_LITE_BREAK test hook: start broken (and count it)
      int* f = &sm.ovf[0] + tid;
      *f = (f == &sm.broken && E.lag < 0) ? 1 : 0;
      if (f == &sm.broken && E.lag < 0 && E.diag) atomicAdd(E.diag + STD_BROKEN, 1);
    }
    if (tid == 18) sm.rec[4] = -1;
    const int lane = tid & 63;
    const _Float16* A1 = D.Wl_raw[1] + (size_t)(4 * w) * (D.Kf[1] / 32) * 64 * 8;
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<_Float16*>(A1), 0, 4 * (D.Kf[1] / 32) * 1024, 0x00020000);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      ring[0][q] = __builtin_bit_cast(
          half8, __builtin_amdgcn_raw_buffer_load_b128(r1, lane * 16, q * (D.Kf[1] / 32) * 1024, 0));
  }
  __syncthreads();                       // the only block-wide barrier
#ifdef DSR_EXP_STAMP
  unsigned long long stamp[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long stamp_last = __builtin_amdgcn_s_memtime(), stamp_lk = 0;
#endif
  int it = 0;
  auto wait = [&](int* c, int target) { st_wait(c, target, sm, it, w); };
  for (int ti = blockIdx.x; ti < nt; ti += gridDim.x, ++it) {
    const int p = it & 1;
    const Tile tl = tiles[ti];
    const ObjDesc d = desc[tl.obj];
    float* xyz = sm.xyz[grp];
    LSTAMP(7)
    // ---- tile inputs, per group
    {
      const int lane = opaque(threadIdx.x & 63);
      if (grp == 1) wait(&sm.cE, 4 * it);
      const int gt = opaque(threadIdx.x) & 255;
      if (gt < LTILE) {
        const float4 v = (gt < tl.count) ? cand[d.cand_off + tl.start + gt] : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(xyz + gt * 4) = v;
      } else {
        const int e = gt - LTILE, which = e >> 6, n = 256 * grp + 4 * (e & 63);
        const float* src = (which == 0 ? bias0f : bias4f) + tl.obj * HID + n;
        *reinterpret_cast<float4*>(&sm.bias[which == 0 ? 0 : 4][n]) = *reinterpret_cast<const float4*>(src);
      }
      st_signal(&sm.cT[grp]);
      wait(&sm.cT[grp], 4 * (it + 1));
    }
    LSTAMP(0)
    floatx4 acc[4][8];
    // ---- lin0 (3 inputs, fp32 VALU) into the accumulator layout
    {
      const int lane = opaque(threadIdx.x & 63), g = lane >> 4, c = lane & 15;
      const float* bias0 = sm.bias[0];
      float m = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n0 = 64 * w + 16 * q + 4 * g;
        const float4 bb = *reinterpret_cast<const float4*>(bias0 + n0);
        float wx[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) wx[i] = D.W0x[n0 * 3 + i];
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) {
          const float4 pt = *reinterpret_cast<const float4*>(xyz + (16 * cb + c) * 4);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float a = __builtin_fmaf(
                wx[3 * r + 2], pt.z, __builtin_fmaf(wx[3 * r + 1], pt.y, __builtin_fmaf(wx[3 * r], pt.x, fetch4(bb, r))));
            const float h = fmaxf(a, 0.f);
            acc[q][cb][r] = h;
            m = fmaxf(m, h);
          }
        }
      }
      if (!(m < 32768.f)) sm.ovf[p] = it + 1;
      LSTAMP(1)
      wait(grp == 0 ? &sm.cRlo : &sm.cRhi, 8 * 7 * it);   // readers of lin7's input
      LSTAMP(2)
      lite_write<SWZ>(acc, sm.H, w, lane);
      st_signal(&sm.cH[grp]);
      LSTAMP(3)
    }
    // ---- lin1..lin7 (lin7: + relu, lin8 dot product -> red); gemm(l): acc = b_l + W_l . H
    auto gemm = [&](int l) {
      const int ng = 7 * it + l;         // GEMMs so far, this one included
      const int hs = 4 * (8 * it + l);   // cH count once the input image is complete
      wait(&sm.cH[0], hs);
      if (grp == 1) {
        wait(&sm.cH[1], hs);
        if (lag > 0) wait(&sm.cP, 4 * ng);
      }
      LSTAMP(4)
      auto hook = [&](int t) {
#ifdef DSR_EXP_STAMP
        if (t == 7 && grp == 0) {
          __builtin_amdgcn_sched_barrier(0);
          const unsigned long long h0 = __builtin_amdgcn_s_memtime();
          wait(&sm.cH[1], hs);
          stamp[8] += __builtin_amdgcn_s_memtime() - h0;
          __builtin_amdgcn_sched_barrier(0);
        }
#else
        if (t == 7 && grp == 0) wait(&sm.cH[1], hs);
#endif
        if (t == 8) st_signal(&sm.cRlo);
        if (t == lag && grp == 0) st_signal(&sm.cP);
#ifdef DSR_EXP_STAMP   // the last k step of the GEMM (with the next matrix's first loads), stamp[9]
        if (t == D.Kf[l] / 32 - 1) {
          __builtin_amdgcn_sched_barrier(0);
          stamp_lk = __builtin_amdgcn_s_memtime();
          __builtin_amdgcn_sched_barrier(0);
        }
#endif
      };
      // The bias rows start the accumulators: gemm_lite_x takes this wave's in registers (ci),
      // gemm_lite_r reads them from sm.bias[l] itself.  K = 512, or 448 for lin4 (h3 | xyz).
      floatx4 ci[4];
      if constexpr (!PIN) {
        const int g = opaque(threadIdx.x & 63) >> 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) ci[q] = *reinterpret_cast<const floatx4*>(sm.bias[l] + 64 * w + 16 * q + 4 * g);
      }
      const int ln = l < 7 ? l + 1 : 1;  // (after lin7: the next tile's lin1 fragments)
      const _Float16 *Wl = D.Wl_raw[l], *Wn = D.Wl_raw[ln];
      const int T = D.Kf[l] / 32, Tn = D.Kf[ln] / 32;
      const int lane = opaque(threadIdx.x & 63);
      if constexpr (PIN) {
        if (T != 14) gemm_lite_r<16, SWZ>(Wl, Wn, Tn, w, sm.H, acc, ring, lane, sm.bias[l], hook);
        else gemm_lite_r<14, SWZ>(Wl, Wn, Tn, w, sm.H, acc, ring, lane, sm.bias[l], hook);
      } else {
        if (T != 14) gemm_lite_x<16, SWZ>(Wl, Wn, Tn, w, sm.H, acc, ring, lane, ci, hook);
        else gemm_lite_x<14, SWZ>(Wl, Wn, Tn, w, sm.H, acc, ring, lane, ci, hook);
      }
#ifdef DSR_EXP_STAMP
      __builtin_amdgcn_sched_barrier(0);
      stamp[9] += __builtin_amdgcn_s_memtime() - stamp_lk;
      __builtin_amdgcn_sched_barrier(0);
#endif
      st_signal(&sm.cRhi);
      LSTAMP(5)
    };
#pragma unroll 1
    for (int l = 1; l <= 6; ++l) {
      gemm(l);
      const int lane = opaque(threadIdx.x & 63), g = lane >> 4, c = lane & 15;
      // acc = b + W.h already: range max, fp16 convert, packed fp16 ReLU.
      // The range max runs on the bit patterns (signed int order = float order for x >= 0,
      // every negative below 0, NaN above +inf so it trips the guard): v_max3_i32, no NaN
      // canonicalisation of the MFMA results that a float max would insert.
      half4 hv[4][8];
      int mi = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) {
          const floatx4 v = acc[q][cb];
          mi = max(mi, max(__float_as_int(v[0]), __float_as_int(v[1])));
          mi = max(mi, max(__float_as_int(v[2]), __float_as_int(v[3])));
          half4 h;
#pragma unroll
          for (int r = 0; r < 4; ++r) h[r] = (_Float16)v[r];
          hv[q][cb] = __builtin_elementwise_max(h, half4{0, 0, 0, 0});
        }
      if (l == 3 && w == (D.l3 >> 6)) {   // lin4 input = h3 | xyz: rows l3..l3+2 (g 3, r 1..3) <- x, y, z
        const int xq = (D.l3 >> 4) & 3;   // (after the ReLU)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q != xq) continue;
#pragma unroll
          for (int cb = 0; cb < 8; ++cb) {
            const float4 pt = *reinterpret_cast<const float4*>(xyz + (16 * cb + c) * 4);
            const bool on = g == 3;
            hv[q][cb][1] = on ? (_Float16)pt.x : hv[q][cb][1];
            hv[q][cb][2] = on ? (_Float16)pt.y : hv[q][cb][2];
            hv[q][cb][3] = on ? (_Float16)pt.z : hv[q][cb][3];
            mi = max(mi, on ? __float_as_int(fmaxf(fabsf(pt.x), fmaxf(fabsf(pt.y), fabsf(pt.z)))) : 0);
          }
        }
      }
      if (!(__int_as_float(mi) < 32768.f)) sm.ovf[p] = it + 1;
      LSTAMP(6)
      wait(grp == 0 ? &sm.cRlo : &sm.cRhi, 8 * (7 * it + l));
      LSTAMP(2)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int cb = 0; cb < 8; ++cb)
          *reinterpret_cast<half4*>(sm.H + (16 * cb + c) * PH + 64 * w + 16 * q + 4 * lite_swz_g(g, c, SWZ)) =
              hv[q][cb];
      st_signal(&sm.cH[grp]);
      LSTAMP(3)
    }
    {
      gemm(7);
      const int lane = opaque(threadIdx.x & 63), g = lane >> 4, c = lane & 15;
      float part[8];
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) part[cb] = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n0 = 64 * w + 16 * q + 4 * g;
        const float4 w8 = *reinterpret_cast<const float4*>(sm.w8 + n0);
#pragma unroll
        for (int cb = 0; cb < 8; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = __int_as_float(max(__float_as_int(accr(acc[q][cb], r)), 0));   // ReLU on bits
            part[cb] = __builtin_fmaf(fetch4(w8, r), v, part[cb]);
          }
      }
#pragma unroll
      for (int cb = 0; cb < 8; ++cb) {
        float s = part[cb];
        s += xor_lane(s, lane, 16);
        s += xor_lane(s, lane, 32);
        if (g == 0) sm.red[w * LTILE + 16 * cb + c] = s;
      }
      st_signal(&sm.cH[grp]);
    }
    // ---- tanh + classification (B's waves 4, 5), then B's tile-done event
    if (grp == 1) {
      const int lane = opaque(threadIdx.x & 63);
      if (w < 6) {
        wait(&sm.cH[0], 4 * (8 * it + 8));
        wait(&sm.cH[1], 4 * (8 * it + 8));
        const int tid = opaque(threadIdx.x) - 256;
        if (tid < tl.count) {
          float s = sm.red[tid];
          for (int k = 1; k < NWAVE; ++k) s += sm.red[k * LTILE + tid];
          float y = tanhf(s + D.b8);
          const float4 pt = *reinterpret_cast<const float4*>(xyz + tid * 4);
          if (pt.x != pt.x || pt.y != pt.y || pt.z != pt.z || bias0f[tl.obj * HID] != bias0f[tl.obj * HID])
            y = __builtin_nanf("");
          const int idx = __float_as_int(pt.w);
          const ObjState& So = E.st[tl.obj];
          const float margin = So.lite_margin;
          y = lite_perturb(E, y, idx);
          dense[d.cand_off + idx] = y;
          bool full = false;
          const unsigned char fl = (sm.ovf[p] == it + 1 || sm.broken)
                                       ? 1 : lite_flag(E, y, idx, margin, So.iters_done, full);
          if (fl) E.refine[d.cand_off + idx] = fl;               // band / range guard / audit
          if (fl != 1 && full) dead_put(E.dead + d.ray_off + idx / E.M, 1);  // certainly full
#ifdef DSR_EXP_PROV
          prov_lite(So.iters_done, d.cand_off + idx, d.ray_off + idx / E.M, idx % E.M, y, fl != 1 && full);
#endif
        }
      }
      st_signal(&sm.cE);
    }
  }
  st_report(sm, E.diag, w);
#ifdef DSR_EXP_STAMP
  LSTAMP(7)
  if (blockIdx.x < 4 && (threadIdx.x == 0 || threadIdx.x == 256))
    printf("lite_stamp %d %d %d %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (int)blockIdx.x, w, it,
           stamp[0], stamp[1], stamp[2], stamp[3], stamp[4], stamp[5], stamp[6], stamp[7], stamp[8], stamp[9]);
#endif
}
#undef LSTAMP

}  // namespace dsr