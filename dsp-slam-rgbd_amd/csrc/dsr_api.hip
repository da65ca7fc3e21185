// dsr_api.hip — C ABI of libdsr (include/dsr.h): contexts, decoder packing, resident
// batches and the per-iteration launch sequence of the device Gauss-Newton loop.
//
// Build (gfx950 only, in-tree):  make -C dsp-slam-rgbd_amd/csrc   -> libdsr.so
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dsr.h"
#include "dsr_kernels.hpp"
#include "dsr_mc.hpp"
#include "dsr_mesh.hpp"
#include "dsr_render.hpp"
#include "dsr_scene.hpp"
#include "dsr_frame.hpp"
#include "dsr_assoc.hpp"
#include "dsr_lidar.hpp"
#include "dsr_track.hpp"

#ifndef DSR_DEFAULT_FWD_VARIANT
#define DSR_DEFAULT_FWD_VARIANT 12  // split-fp16 (3xFP16) + s_setprio (A/B: tools/fwd_variants.py)
#endif

using namespace dsr;

constexpr int MAX_GROUPS = 4;       // = GPU_MAX_HW_QUEUES on the box

struct dsr_ctx {
  int device = 0;
  int n_cu = 256;
  hipStream_t stream = nullptr;
  hipStream_t gstream[MAX_GROUPS] = {};   // [0] = stream; [1..] object-group streams
  std::string err;
  // Device memory and events of destroyed batches, reused by the next ones: a keyframe
  // stream, or the per-call reconstruct_object API, creates one batch per call, and
  // hipMalloc / hipFree (which synchronises) / hipEventCreate cost more than a small
  // batch's GN run takes.  Capped at POOL_CAP bytes; released by dsr_ctx_destroy.
  std::multimap<size_t, void*> pool;      // free device blocks by size
  size_t pool_bytes = 0;
  std::vector<hipEvent_t> ev_timing, ev_plain;
  // guards pool / ev_*: a context is used from one thread at a time (include/dsr.h), but
  // batches of async handles may be destroyed from another Python thread (finalizers)
  std::mutex mu;
  // serialises the stream work of batch entry points (launch, graph capture, refill, redo) with
  // dsr_batch_destroy: a destroy from a finalizer thread synchronises the context's streams and
  // destroys a graph, which must never happen while the owning thread captures on that stream
  std::recursive_mutex run_mu;
  // LayerNorm decoders: the Jacobian kernel's x^ / rstd workspace per stream (gstream[g]; the
  // context stream's serves sdf_eval and pose-only too), n_cu x LN_WS_WG floats each, allocated
  // on first need outside any capture and kept until dsr_ctx_destroy (graphs hold the pointer)
  float* lnws[MAX_GROUPS] = {};
};
static constexpr size_t POOL_CAP = (size_t)16 << 30;

static float* ln_workspace(dsr_ctx* ctx, int g) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (!ctx->lnws[g] &&
      hipMalloc((void**)&ctx->lnws[g], sizeof(float) * (size_t)LN_WS_WG * ctx->n_cu) != hipSuccess) {
    (void)hipGetLastError();
    ctx->lnws[g] = nullptr;
  }
  return ctx->lnws[g];
}

// Forward-kernel variant (DSR_FWD_VARIANT: bit0 XCD soft sync, bit1 B prefetch, bit2 setprio,
// bit3 split-fp16; 12 = split-fp16 + setprio, the default) and the A-ring depth of the split
// kernels (DSR_SPLIT_RING: 0 = the two-set gemm16_tile, 2..4 = gemm16_ring k steps in flight)
// Kernel-selecting switches (A/B experiments: DSR_FWD_VARIANT, DSR_JAC_VARIANT, DSR_SPLIT_RING,
// DSR_LITE_VARIANT, DSR_LITE_LAG, DSR_REFINE_ALL, DSR_RENDER_PASSES, DSR_ADAPTIVE_WINDOWS,
// DSR_KEEP_MASKS, DSR_SURFACE_EXACT) and the test hooks are read from the environment only under
// DSR_TEST_HOOKS=1, which dsr_stats.test_hooks reports: a stray variable cannot change the kernels
// of a production run (test_gpu_lite_audit.py: test_kernel_switches_ignored_without_the_gate).
// The two production switches, DSR_STREAMS (object groups) and DSR_GRAPH (graph replay), are
// reported in dsr_stats (n_groups, graph_mode); DSR_LITE=0 (every sample decoded exactly) in
// dsr_stats.lite.
static bool test_hooks() {
  const char* e = getenv("DSR_TEST_HOOKS");
  return e && atoi(e) != 0;
}
static const char* hook_env(const char* k) { return test_hooks() ? getenv(k) : nullptr; }

#ifndef DSR_DEFAULT_SPLIT_RING
#define DSR_DEFAULT_SPLIT_RING 2
#endif
static int split_ring() {
  const char* e = hook_env("DSR_SPLIT_RING");
  const int r = e ? atoi(e) : DSR_DEFAULT_SPLIT_RING;
  return (r >= 2 && r <= 4) ? r : 0;
}

static int fwd_variant() {
  const char* e = hook_env("DSR_FWD_VARIANT");
  return e ? atoi(e) : DSR_DEFAULT_FWD_VARIANT;
}
static int jac_variant() {
  const char* e = hook_env("DSR_JAC_VARIANT");
  return e ? atoi(e) : 12;
}
// the forward variant of a one-launch decoder query (dsr_sdf_eval, the mesher): the XCD soft-sync
// variants (bit 0) need the per-batch sync counter these launches have not got, so their bit 0 is
// dropped there (the same kernels otherwise)
static int query_fwd_variant() { return fwd_variant() & ~1; }
using FwdKernel = void (*)(DevDecoder, const Tile*, const int*, const ObjDesc*, const float4*, const float*,
                           const float*, float*, unsigned*, ErtArgs, MaskArgs);
// split-fp16 forward with X's mask bit (512) and the ring depth in bits 10-11
template <int MSK>
static FwdKernel fwd16_kernel() {
  switch (split_ring()) {
    case 2: return k_mlp_fwd16<true, MSK | 1024>;
    case 3: return k_mlp_fwd16<true, MSK | 2048>;
    case 4: return k_mlp_fwd16<true, MSK | 3072>;
  }
  return k_mlp_fwd16<true, MSK>;
}
// What a kernel family runs and what dsr_stats reports of it: the variant number, the kernel, and
// the A-ring depth of the split kernels
struct FwdChoice {
  int number;
  FwdKernel kernel;
  int ring;
};
// the low nibble of v selects: a table row, or 12, the split kernels at fwd16_kernel's ring depth;
// an unknown one runs k_mlp_fwd<0> and reports v without it
static FwdChoice fwd_kernel(int v) {
  static const struct {
    int number;
    FwdKernel kernel;
  } table[] = {{1, k_mlp_fwd<1>}, {2, k_mlp_fwd<2>}, {3, k_mlp_fwd<3>},
               {6, k_mlp_fwd<6>}, {7, k_mlp_fwd<7>}, {8, k_mlp_fwd16<false, 0>}};
  const int ring = split_ring();
  for (const auto& c : table)
    if (c.number == (v & 15)) return {v, c.kernel, ring};
  if ((v & 15) == 12) return {v, fwd16_kernel<0>(), ring};
  return {v & ~15, k_mlp_fwd<0>, ring};
}
using JacKernel = void (*)(DevDecoder, const Tile*, const int*, const ObjDesc*, const ObjState*, const float*,
                           const float4*, const float*, const float*, const float*, GNParams, float*,
                           const float4*, float*, float*, MaskArgs, float*);
struct JacChoice {
  int number;
  JacKernel kernel;
  int ring = -1;            // (a table row's ring -1: the row holds for any depth)
};
// an unknown DSR_JAC_VARIANT runs k_mlp_jac and reports 0
static JacChoice jac_kernel() {
  static const JacChoice table[] = {{8, k_mlp_jac16<false, 0>},
                                    {12, k_mlp_jac16<true, 2>, 2},
                                    {12, k_mlp_jac16<true, 3>, 3},
                                    {12, k_mlp_jac16<true, 4>, 4},
                                    {12, k_mlp_jac16<true, 0>, 0}};
  const int v = jac_variant(), ring = split_ring();
  for (const JacChoice& c : table)
    if (c.number == v && (c.ring < 0 || c.ring == ring)) return {v, c.kernel, ring};
  return {0, k_mlp_jac, ring};
}
struct dsr_decoder {
  dsr_ctx* ctx = nullptr;
  float* dmem = nullptr;
  size_t bytes = 0;
  DevDecoder D{};
  int code_len = 64;
  dsr_decoder_info info{};      // load-time lite qualification (decoder_qualify)
};

// Decoder variants (use_tanh / xyz_in_all / LayerNorm) run their own instantiations of the
// split-fp16 kernels (ring depth 2), so the shipped topology's kernels carry none of their code;
// variant_kernels_ok has already refused the fp32-MFMA A/B variants for them
static bool is_variant(const DevDecoder& D) { return D.xyz_all || D.use_tanh || D.ln_mask; }
// the decoder variants (use_tanh, xyz_in_all) are implemented in the split-fp16 kernels only
// (the fp32-MFMA A/B variants k_mlp_fwd / k_mlp_jac implement the shipped topology)
static bool variant_kernels_ok(const dsr_decoder* dec) {
  return !is_variant(dec->D) || (fwd_variant() == 12 && jac_variant() == 12);
}
static FwdChoice fwd_kernel_for(const DevDecoder& D, int v) {
  return is_variant(D) ? FwdChoice{12, k_mlp_fwd16<true, 1024 | 8192>, 2} : fwd_kernel(v);
}
static JacChoice jac_kernel_for(const DevDecoder& D) {
  return is_variant(D) ? JacChoice{12, k_mlp_jac16<true, 2, true>, 2} : jac_kernel();
}
// Lite-pass schedule (DSR_LITE_VARIANT; dsr_mlp_lite.hpp: k_mlp_fwd_lite_st<SWZ, PIN>).  The
// numbers are names (environment, dsr_stats.lite_variant); all three give bitwise equal values:
//   472   staggered wave groups, unswizzled H image
//   1496  472 + swizzled H image (2-way instead of 4-way epilogue store conflicts); what an
//         unknown number runs
//   3544  1496 + the B-fragment ring pinned 12 MFMAs ahead of its use (gemm_lite_r); the default
using LiteKernel = void (*)(DevDecoder, const Tile*, const int*, const ObjDesc*, const float4*, const float*,
                            const float*, float*, ErtArgs);
#ifndef DSR_DEFAULT_LITE_VARIANT
#define DSR_DEFAULT_LITE_VARIANT 3544
#endif
struct LiteSchedule {
  int number;
  LiteKernel kernel;
};
static const LiteSchedule& lite_schedule() {
  static const LiteSchedule table[] = {{1496, k_mlp_fwd_lite_st<true, false>},   // first: the fallback
                                       {472, k_mlp_fwd_lite_st<false, false>},
                                       {3544, k_mlp_fwd_lite_st<true, true>}};
  const char* e = hook_env("DSR_LITE_VARIANT");
  const int v = e ? atoi(e) : DSR_DEFAULT_LITE_VARIANT;
  for (const LiteSchedule& s : table)
    if (s.number == v) return s;
  return table[0];
}
// DSR_REFINE_ALL=1: the exact pass re-decodes every band sample, also those behind a ray's
// first certainly-full sample (k_refine_scan)
static bool refine_all() {
  const char* e = hook_env("DSR_REFINE_ALL");
  return e && atoi(e) != 0;
}
// Test hooks (DSR_LITE_PERTURB, DSR_LITE_BREAK) change results or cost on purpose; the library
// honours them only when DSR_TEST_HOOKS=1 was set as the batch was created, and reports that
// in dsr_stats.test_hooks, so a stray variable cannot silently change a production run.
// DSR_LITE_LAG (staggered lite kernel): the k step group A reaches before group B starts a GEMM.
// DSR_LITE_BREAK=1 (test hook): every block starts in the "broken" state of a timed-out
// event wait, so every sample goes to the exact pass (lag -1)
static int lite_lag(bool hooks) {
  const char* b = getenv("DSR_LITE_BREAK");
  if (hooks && b && atoi(b) != 0) return -1;
  const char* e = hooks ? getenv("DSR_LITE_LAG") : nullptr;
  const int v = e ? atoi(e) : 4;
  return v < 0 ? 0 : (v > 7 ? 7 : v);
}

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
};

struct dsr_batch {
  dsr_ctx* ctx = nullptr;
  const dsr_decoder* dec = nullptr;
  GNParams P{};
  int n_obj = 0;
  int iters = 0;
  int M = 50;
  std::vector<ObjDesc> hdesc;
  int cand_total = 0, slot_total = 0, fwd_tile_cap = 0, jac_tile_cap = 0;
  std::vector<std::pair<void*, size_t>> allocs;   // (block, its size): back to the context pool
  // device
  ObjDesc* desc = nullptr;
  ObjState* st = nullptr;
  float *zbuf = nullptr, *z_in = nullptr, *t_in = nullptr;
  int* is_oc = nullptr;
  float *pts = nullptr, *rays = nullptr, *dobs = nullptr;
  float4 *cand = nullptr, *kpts = nullptr;
  float4* kst = nullptr;           // k_render_rays staging (per chunk, at its rays' sample range)
  float* rst = nullptr;
  int* sst = nullptr;
  float *dense = nullptr, *kres = nullptr;
  float *bias0f = nullptr, *bias4f = nullptr;
  // Object groups: contiguous object ranges whose GN iterations run on their own streams,
  // so one group's latency-bound kernels and kernel tails overlap the other's decoder
  // kernels (objects never interact; every group owns its tile tables and counters).
  struct Group {
    int o0 = 0, n = 0;
    int c0 = 0, c1 = 0;        // cand range of the group's objects
    Tile *tiles_f = nullptr, *tiles_j = nullptr;
    int *nt_f = nullptr, *nt_j = nullptr;
    unsigned* sync = nullptr;
    RenderChunk* rchunks = nullptr;   // k_render_rays chunks of the group's objects
    int* ccnt = nullptr;              // render points per chunk
    int* scnt = nullptr;              // chunked render passes: samples, in-ball samples per chunk
    int2* och = nullptr;              // per object: first chunk, chunks (the chunked path's tile tables)
    int n_rch = 0;
    int t0 = 0, nt = 0;               // tied batches: the group's tied objects (tie[t0 .. t0 + nt))
  };
  std::vector<Group> groups;
  // Tied batches (dsr_reconstruct_views): the views of one object are consecutive members, the
  // reference view first.  tie[i] = (leader member relative to its group's first member, views)
  // of tied object i; cview[member] = inverse(t_view_ref); fail_view[i] = the view that failed
  // object i or -1.  k_solve_views replaces k_solve, k_views_pose re-derives the members' poses.
  int n_tied = 0;                     // 0: an ordinary batch
  bool tie_multi = false;             // some object has more than one view
  int2* tie = nullptr;
  float* cview = nullptr;
  int* fail_view = nullptr;
  hipEvent_t fork_ev = nullptr;
  hipEvent_t done_ev = nullptr;  // recorded after every run (dsr_batch_query)
  std::vector<hipEvent_t> join_ev;
  float* slots = nullptr;
  float* sred = nullptr;        // [n_obj][2][SLOT_FLOATS] tile-partial sums (k_reduce_slots)
  int* counts = nullptr;
  dsr_object_out* out = nullptr;
  float *tr_H = nullptr, *tr_v = nullptr;
  int* tr_i = nullptr;
  int* dead = nullptr;          // per-ray early-termination flags (k_sample_pass)
  int* rinfo = nullptr;         // per-ray in-ball run (first in-ball sample | count << 8), or -1
  int* rwin = nullptr;          // per-ray window of the current render pass (k_sample_scan / _count)
  unsigned char* refine = nullptr;   // per-sample flags of the lite pass (dsr_mlp_lite.hpp)
  uint64_t *rbits = nullptr, *abits = nullptr;   // per-ray refined / audited sample bits (k_refine_scan)
  MaskArgs ma{nullptr, nullptr, nullptr, nullptr};   // kept masks of the exact re-decode
  int* kslot = nullptr;
  bool lite = true;             // lite classification pass + exact re-decode of the band
  int loop_iters = 0;           // iters + 1 spare iteration for audit redos (lite + audit)
  bool spare_run = false;       // the spare iteration was enqueued for the last run
  // lite-pass settings fixed at creation (the iteration count, event sizing and the spare
  // iteration depend on them, so a run never re-reads the environment)
  ErtArgs lite_cfg{};           // audit, shell, audit_log2, perturb, lag
  bool hooks = false;           // DSR_TEST_HOOKS=1 at creation
  int* diag = nullptr;          // [STD_INTS] broken-block count + first expired wait (dsr_dev.hpp)
  std::vector<int> passes;      // render-pass rank boundaries, last = M
  std::vector<hipEvent_t> ev;   // begin, end, then per (iteration, group): fwd0/fwd1 per pass, jac0, jac1
  bool ran = false;
  int runs = 0;
  bool timed = false;               // last run recorded per-kernel events (eager run)
  bool prescan = false;             // first pass's ray scan over the ray chunks (k_sample_scan)
  // the kernels the last enqueue dispatched (dsr_stats, ABI 11; resolved there, so a later change
  // of the environment cannot misreport them)
  int ran_fwd = 0, ran_jac = 0, ran_lite = 0, ran_ring = 0;
#ifdef DSR_EXP_PROV
  int *prov_alive = nullptr, *prov_set = nullptr, *prov_xcc = nullptr, *prov_j = nullptr;   // (PROV_IT)
  unsigned* prov_t = nullptr;
  unsigned* prov_h = nullptr;
  unsigned* prov_ri = nullptr;
  float* prov_nrm = nullptr;
  float* prov_nrm2 = nullptr;
  float* prov_y = nullptr;
  int prov_R = 0, prov_C = 0;
#endif
  hipGraphExec_t graph = nullptr;   // the whole run, captured on the 2nd dsr_batch_run
  long graph_key = -1;              // kernel variants the graph was captured with
  int captures = 0, replays = 0;    // graph captures / replays over the batch's life
  // Fixed-capacity batches (dsr_batch_create_capacity): n_obj slots of max_pts / max_rays each;
  // dsr_batch_refill uploads a new object set into them (pinned staging, one stream-ordered
  // copy per input buffer) and rewrites the per-slot descriptors, so every kernel argument —
  // and a captured graph — stays valid from one keyframe to the next.
  bool capacity = false;
  bool cap_graph = false;           // DSR_BATCH_GRAPH: every run replays one captured graph
  int max_pts = 0, max_rays = 0;
  size_t pts_floats = 0, ray_slots = 0;   // pts / rays+dobs buffer lengths (group padding included)
  int n_active = 0;                 // objects of the current fill (out-records downloaded)
  struct Stage {                    // pinned host mirrors of the refilled input buffers
    void* host = nullptr;
    void* dev = nullptr;
    size_t bytes = 0;
  };
  std::vector<Stage> stage;
  hipEvent_t up_ev = nullptr;       // recorded after the last refill's uploads
  // Device-filled refills (dsr_batch_refill_frame, _frame_poses, _lidar) share one ingest block: a
  // pinned half (what the fill uploads — depth | instance | detections, or sweep | instance | masks |
  // prepared detections) and a device half (the same, then the kernels' tables and records;
  // dsr_frame.hpp, dsr_lidar.hpp).  A fill is of one kind, so the block is laid out for the last
  // fill only; it grows to the largest fill seen (refill_begin) and is freed with the batch.
  struct IngestBlock {
    void* host = nullptr;
    void* dev = nullptr;
    size_t host_bytes = 0, dev_bytes = 0;
  };
  IngestBlock ingest;
  // The last fill: its kind and what lays its part of the ingest block out.  Written by refill_end
  // alone; the *_info entry points read it.
  struct Fill {
    enum Kind { OBJECTS, FRAME, FRAME_POSES, SWEEP };
    Kind kind = OBJECTS;
    LidarShape shape{0, 3, 0, 0, 0};   // n_det: every kind's objects; W, H: the image kinds; n_velo, stride: a sweep
    int max_pts = 0;                   // FRAME_POSES: sizes the keep flags (§3.5c)
  };
  Fill last;
};

#define DSR_CHECK(ctx, call)                                                        \
  do {                                                                              \
    hipError_t e_ = (call);                                                         \
    if (e_ != hipSuccess) {                                                         \
      if (ctx) (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);      \
      return -1;                                                                    \
    }                                                                               \
  } while (0)

static int fail(dsr_ctx* ctx, const std::string& m) {
  if (ctx) ctx->err = m;
  return -2;
}

#include "dsr_host.hpp"

extern "C" {

int dsr_abi_version(void) { return DSR_ABI_VERSION; }

int dsr_device_count(int* n) {
  if (!n) return -2;
  return hipGetDeviceCount(n) == hipSuccess ? 0 : -1;
}

int dsr_ctx_create(int device, dsr_ctx** out) {
  if (!out) return -2;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -3;
  if (device < 0 || device >= n) return -2;
  if (hipSetDevice(device) != hipSuccess) return -1;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return -1;
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) return -4;
  // k_render_rays' dynamic LDS reaches 66.5 KB at the largest sample count (M = 64)
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_render_rays), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)render_lds_bytes(MAXM)) != hipSuccess)
    return -1;
  auto* c = new dsr_ctx();
  c->device = device;
  c->n_cu = prop.multiProcessorCount;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return -1;
  }
  c->gstream[0] = c->stream;
  for (int g = 1; g < MAX_GROUPS; ++g)
    if (hipStreamCreateWithFlags(&c->gstream[g], hipStreamNonBlocking) != hipSuccess) {
      for (int k = 0; k < g; ++k) hipStreamDestroy(c->gstream[k]);
      delete c;
      return -1;
    }
  *out = c;
  return 0;
}

int dsr_ctx_destroy(dsr_ctx* ctx) {
  if (!ctx) return 0;
  hipSetDevice(ctx->device);
  for (auto& kv : ctx->pool) hipFree(kv.second);
  for (hipEvent_t e : ctx->ev_timing) hipEventDestroy(e);
  for (hipEvent_t e : ctx->ev_plain) hipEventDestroy(e);
  for (int g = 1; g < MAX_GROUPS; ++g)
    if (ctx->gstream[g]) hipStreamDestroy(ctx->gstream[g]);
  if (ctx->stream) hipStreamDestroy(ctx->stream);
  for (float* p : ctx->lnws)
    if (p) hipFree(p);
  delete ctx;
  return 0;
}

const char* dsr_last_error(const dsr_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// ------------------------------------------------------------------------------------
// decoder packing
// ------------------------------------------------------------------------------------
// A-fragment layout of v_mfma_f32_16x16x4_f32 with the permuted-k float4 scheme of
// dsr_mlp.hpp: out[((rb*T + t)*64 + lane)*4 + j] = src(16 rb + (lane&15), 16 t + 4 (lane>>4) + j)
static void pack_frag(std::vector<float>& out, int rows_pad, int cols_pad,
                      const std::function<float(int, int)>& src) {
  const int RB = rows_pad / 16, T = cols_pad / 16;
  out.assign((size_t)RB * T * 256, 0.f);
  for (int rb = 0; rb < RB; ++rb)
    for (int t = 0; t < T; ++t)
      for (int lane = 0; lane < 64; ++lane)
        for (int j = 0; j < 4; ++j)
          out[(((size_t)rb * T + t) * 64 + lane) * 4 + j] =
              src(16 * rb + (lane & 15), 16 * t + 4 * (lane >> 4) + j);
}

// The fp16 neighbour of h on the other side of r (h = fp16(r) != r): one step up or down the fp16
// grid, by the bit pattern (sign-magnitude; +0 / -0 step to the smallest subnormals)
static _Float16 f16_other_side(_Float16 h, double r) {
  uint16_t b;
  std::memcpy(&b, &h, 2);
  const bool up = (double)h < r;                    // r lies above h: the next value up
  const bool neg = (b & 0x8000) != 0, zero = (b & 0x7fff) == 0;
  if (zero) b = up ? 0x0001 : 0x8001;
  else if (up != neg) b = (uint16_t)(b + 1);        // away from zero
  else b = (uint16_t)(b - 1);                       // toward zero
  _Float16 o;
  std::memcpy(&o, &b, 2);
  return o;
}

// Probe inputs of one split GEMM: P points' values of its input columns, in the GEMM's packed k
// order, column-major (x[c * P + p]); empty: the pack's lo pieces round to nearest.
struct ProbeCols {
  std::vector<float> x;
  int P = 0;
  bool empty() const { return x.empty(); }
};

// Split-fp16 A fragments for v_mfma_f32_16x16x32_f16 (dsr_mlp16.hpp):
// out[(((rb*T + t)*2 + piece)*64 + lane)*8 + j] = piece of src(16 rb + (lane&15), 32 t + 8 (lane>>4) + j) * 2^sw
// hi = fp16(W 2^sw) and lo = one of the two fp16 neighbours of the remainder W 2^sw - hi.  hi + lo
// carries 22-23 of an fp32 weight's 24 bits, and the rounded-away tails are a FIXED perturbation
// of the decoder: a smooth function of x that puts nearly the same error on every nearby point's
// sdf and Jacobian, which b = sum_p J_p r_p adds up coherently (-2.3e-8 sdf offset and a 5e-8
// Jacobian bias on the bench decoder with lo to nearest; numpy emulation and tools/bias_probe.py).
// With `probe` (the GEMM's inputs at a fixed probe set, decoder_probe) lo is chosen by greedy error
// feedback along each row: of the two neighbours, the one that keeps the row's error over the
// probe points, sum_p ((hi + lo - W 2^sw) . x_p)^2, smallest — a GPTQ-style rounding against the
// probe inputs' second moments, not only their mean.  Emulated on the bench decoder (/the sphere-
// shell points of tools/bias_probe.py): Jacobian bias 5.0e-8 -> 1.2e-8 (mean-only feedback 2.1e-8),
// random error 2.2e-7 -> 7.5e-8.  Rows are independent: split over a fixed 8 host threads, the
// same packs on every host.
static int pack_frag16(std::vector<_Float16>& out, int rows_pad, int cols_pad,
                       const std::function<float(int, int)>& src, const ProbeCols* probe = nullptr) {
  float mx = 0.f;
  for (int r = 0; r < rows_pad; ++r)
    for (int c = 0; c < cols_pad; ++c) mx = std::max(mx, std::fabs(src(r, c)));
  int e = 0;
  if (mx > 0.f) (void)std::frexp(mx, &e);
  const int sw = 14 - e;                            // max |W| * 2^sw < 2^14
  const int RB = rows_pad / 16, T = cols_pad / 32;
  out.assign((size_t)RB * T * 2 * 64 * 8, (_Float16)0.f);
  const bool fb = probe && !probe->empty() && probe->x.size() == (size_t)cols_pad * probe->P;
  const int P = fb ? probe->P : 0;
  const float* X = fb ? probe->x.data() : nullptr;
  std::vector<double> nrm((size_t)cols_pad, 0.0);   // |x_c|^2 over the probe points
  for (int c = 0; fb && c < cols_pad; ++c)
    for (int p = 0; p < P; ++p) nrm[c] += (double)X[(size_t)c * P + p] * X[(size_t)c * P + p];
  auto rows = [&](int th, int nth) {
    std::vector<_Float16> hi((size_t)cols_pad), lo((size_t)cols_pad);
    std::vector<double> u((size_t)P);               // the row's error at each probe point so far
    for (int r = th; r < rows_pad; r += nth) {
      std::fill(u.begin(), u.end(), 0.0);
      for (int c = 0; c < cols_pad; ++c) {
        const float x = std::ldexp(src(r, c), sw);
        const _Float16 h = (_Float16)x;
        const double rem = (double)x - (double)(float)h;   // exact
        _Float16 l = (_Float16)(float)rem;                 // to nearest (rem is exact in fp32)
        bool upd = false;
        if (fb && nrm[c] > 0.0 && (double)(float)l != rem) {
          const float* xs = X + (size_t)c * P;
          double dot = 0.0;
          for (int p = 0; p < P; ++p) dot += u[p] * xs[p];
          const _Float16 l2 = f16_other_side(l, rem);
          const double d1 = (double)(float)l - rem, d2 = (double)(float)l2 - rem;
          if (2.0 * d2 * dot + d2 * d2 * nrm[c] < 2.0 * d1 * dot + d1 * d1 * nrm[c]) l = l2;
          upd = true;
        }
        if (upd) {
          const double d = (double)(float)l - rem;
          const float* xs = X + (size_t)c * P;
          for (int p = 0; p < P; ++p) u[p] += d * xs[p];
        }
        hi[c] = h;
        lo[c] = l;
      }
      const int rb = r >> 4, lr = r & 15;
      // odd 16-row blocks negated (SPLIT_ROW_SIGNS, dsr_mlp16.hpp: row_sign): exact, both pieces
      const bool neg = SPLIT_ROW_SIGNS && (rb & 1);
      for (int t = 0; t < T; ++t)
        for (int g = 0; g < 4; ++g)
          for (int j = 0; j < 8; ++j) {
            const int c = 32 * t + 8 * g + j, lane = lr + 16 * g;
            out[((((size_t)rb * T + t) * 2 + 0) * 64 + lane) * 8 + j] = neg ? (_Float16)(-hi[c]) : hi[c];
            out[((((size_t)rb * T + t) * 2 + 1) * 64 + lane) * 8 + j] = neg ? (_Float16)(-lo[c]) : lo[c];
          }
    }
  };
  if (!fb) {
    rows(0, 1);
  } else {
    constexpr int nth = 8;
    std::vector<std::thread> ts;
    for (int t = 0; t < nth; ++t) ts.emplace_back(rows, t, nth);
    for (auto& t : ts) t.join();
  }
  return sw;
}

// The split GEMMs' inputs at a fixed probe set — 256 points uniform in the unit ball (fixed LCG),
// code 0 — in the packed column order pack_frag16 uses, for its feedback rounding:
//  fwd[l], l = 1..7: lin l's input h_{l-1} (with xyz at 509..511 under xyz_in_all); lin4's columns
//    are h3 (l3) then xyz (the code is folded into its bias);
//  bwd[l], l = 0..7: d sdf / d(output of lin l), through its ReLU (and LayerNorm, if any) — the
//    input of the backward GEMM W_l^T, over lin l's outputs.
// A host forward + backward pass of deep_sdf_decoder.py:75-110 in fp32 (LayerNorm, use_tanh and
// xyz_in_all included), split over a fixed 8 host threads (not the core count: the same probes,
// hence the same packs, on every host); well under 0.1 s once per load.
struct DecoderProbe {
  ProbeCols fwd[8], bwd[8];
};
static DecoderProbe decoder_probe(const int* od, const int* id, const std::vector<const float*>& W,
                                  const std::vector<const float*>& B, const std::vector<const float*>& LG,
                                  const std::vector<const float*>& LB, int L, int l3, int XA, int K4, int K3b,
                                  int use_tanh, bool with_bwd) {
  constexpr int P = 256;
  std::vector<float> pts((size_t)P * 3);
  uint64_t s = 0xD1B54A32D192ED03ull;
  auto u01 = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
  };
  for (int i = 0; i < P;) {
    const double x = 2 * u01() - 1, y = 2 * u01() - 1, z = 2 * u01() - 1;
    if (x * x + y * y + z * z >= 1.0) continue;
    pts[3 * i] = (float)x; pts[3 * i + 1] = (float)y; pts[3 * i + 2] = (float)z;
    ++i;
  }
  DecoderProbe pr;
  for (int l = 0; l <= 7; ++l) {
    if (l >= 1) {
      pr.fwd[l].P = P;
      pr.fwd[l].x.assign((size_t)(l == 4 ? K4 : 512) * P, 0.f);
    }
    if (with_bwd) {
      pr.bwd[l].P = P;
      pr.bwd[l].x.assign((size_t)(l == 3 ? K3b : 512) * P, 0.f);
    }
  }
  auto work = [&](int th, int nth) {
    std::vector<float> h, in, a;
    std::vector<std::vector<float>> post(9), xh(9);   // pre-ReLU values (after LayerNorm); x^
    std::vector<double> rs(9, 0.0);                    // LayerNorm 1 / sqrt(var + eps)
    for (int p = th; p < P; p += nth) {
      const float* xyz = &pts[3 * p];
      std::vector<float> inp((size_t)L + 3, 0.f);  // [code (0) | xyz]
      inp[L] = xyz[0]; inp[L + 1] = xyz[1]; inp[L + 2] = xyz[2];
      h = inp;
      for (int l = 0; l <= 7; ++l) {
        in = h;
        if (l == 4) in.insert(in.end(), inp.begin(), inp.end());
        else if (l != 0 && XA) in.insert(in.end(), xyz, xyz + 3);
        if (l >= 1) {                                // the GEMM's packed columns
          float* m = pr.fwd[l].x.data();
          if (l == 4) {
            for (int c = 0; c < l3; ++c) m[(size_t)c * P + p] = in[c];
            for (int k = 0; k < 3; ++k) m[(size_t)(l3 + k) * P + p] = xyz[k];
          } else {
            for (int c = 0; c < (int)in.size() && c < 512; ++c) m[(size_t)c * P + p] = in[c];
          }
        }
        a.assign(od[l], 0.f);
        for (int r = 0; r < od[l]; ++r) {    // 8 partial sums: a vectorisable dot product
          const float* wr = W[l] + (size_t)r * id[l];
          float ps[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
          int c = 0;
          for (; c + 8 <= id[l]; c += 8)
            for (int k = 0; k < 8; ++k) ps[k] += wr[c + k] * in[c + k];
          float acc = B[l][r];
          for (; c < id[l]; ++c) acc += wr[c] * in[c];
          a[r] = acc + (((ps[0] + ps[1]) + (ps[2] + ps[3])) + ((ps[4] + ps[5]) + (ps[6] + ps[7])));
        }
        if (LG[l]) {                                 // nn.LayerNorm(out_dim), eps 1e-5, biased variance
          double mu = 0, var = 0;
          for (float v : a) mu += v;
          mu /= od[l];
          for (float v : a) var += (v - mu) * (v - mu);
          var /= od[l];
          rs[l] = 1.0 / std::sqrt(var + 1e-5);
          xh[l].resize(od[l]);
          for (int r = 0; r < od[l]; ++r) {
            xh[l][r] = (float)((a[r] - mu) * rs[l]);
            a[r] = xh[l][r] * LG[l][r] + LB[l][r];
          }
        }
        post[l] = a;
        for (float& v : a) v = v > 0.f ? v : 0.f;
        h = a;
      }
      if (!with_bwd) continue;
      // d sdf / d pre-activation, layer by layer down
      float s8 = B[8][0];
      for (int c = 0; c < id[8]; ++c) {
        const float hv = c < (int)h.size() ? h[c] : xyz[c - (int)h.size()];   // (xyz_in_all: lin8 sees xyz too)
        s8 += W[8][c] * hv;
      }
      float t = std::tanh(s8), y = t;
      float g8 = 1.f - y * y;
      if (use_tanh) { y = std::tanh(t); g8 = (1.f - y * y) * (1.f - t * t); }
      std::vector<float> g(od[7]);
      for (int r = 0; r < od[7]; ++r) g[r] = post[7][r] > 0.f ? g8 * W[8][r] : 0.f;
      for (int l = 7; l >= 0; --l) {
        if (LG[l]) {                                 // through the LayerNorm (dsr_oracle.forward_jac)
          double m1 = 0, m2 = 0;
          for (int r = 0; r < od[l]; ++r) {
            const double gx = (double)g[r] * LG[l][r];
            m1 += gx;
            m2 += gx * xh[l][r];
          }
          m1 /= od[l];
          m2 /= od[l];
          for (int r = 0; r < od[l]; ++r)
            g[r] = (float)(rs[l] * ((double)g[r] * LG[l][r] - m1 - xh[l][r] * m2));
        }
        float* m = pr.bwd[l].x.data();
        for (int r = 0; r < od[l]; ++r) m[(size_t)r * P + p] = g[r];
        if (l == 0) break;
        std::vector<float> gi(od[l - 1], 0.f);     // W_l^T g, the h_{l-1} part, masked
        for (int r = 0; r < od[l]; ++r) {
          if (g[r] == 0.f) continue;
          const float* wr = W[l] + (size_t)r * id[l];
          for (int c = 0; c < od[l - 1]; ++c) gi[c] += wr[c] * g[r];
        }
        for (int c = 0; c < od[l - 1]; ++c) gi[c] = post[l - 1][c] > 0.f ? gi[c] : 0.f;
        g.swap(gi);
      }
    }
  };
  constexpr int nth = 8;
  std::vector<std::thread> ts;
  for (int t = 0; t < nth; ++t) ts.emplace_back(work, t, nth);
  for (auto& t : ts) t.join();
  return pr;
}

// a code's bias folds of lin0 and lin4: bias + W_z z, per code (every decoder query runs on them)
__global__ void k_fold_code(DevDecoder D, const float* __restrict__ z, float* __restrict__ bias0f,
                            float* __restrict__ bias4f) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= HID) return;
  float s0 = 0.f, s4 = 0.f;
  for (int k = 0; k < CODE; ++k) {
    s0 = __builtin_fmaf(D.W0z[k * HID + n], z[k], s0);
    s4 = __builtin_fmaf(D.W4z[k * HID + n], z[k], s4);
  }
  bias0f[n] = D.bias[0][n] + s0;
  bias4f[n] = D.bias[4][n] + s4;
}
// the bias folds of n codes (64 floats each, back to back) into b0 / b4 (HID floats each)
static void fold_codes(hipStream_t s, const DevDecoder& D, const float* codes, int n, float* b0, float* b4) {
  for (int i = 0; i < n; ++i)
    hipLaunchKernelGGL(k_fold_code, dim3(HID / 256), dim3(256), 0, s, D, codes + (size_t)i * CODE, b0 + (size_t)i * HID,
                       b4 + (size_t)i * HID);
}

// ------------------------------------------------------------------------------------
// load-time qualification of the lite pass (include/dsr.h: dsr_decoder_info)
// ------------------------------------------------------------------------------------
// The lite pass classifies ray samples with one fp16 product; the per-object margin and the
// audit guard it at run time, but their evidence is empirical: a decoder with
// larger weights or activations has larger fp16 errors.  So before any batch trusts the lite
// pass with a loaded decoder, the decoder decodes a fixed probe set through both passes — the
// same kernels, tiles and bias fold a batch uses — and the lite error is measured against the
// distance of each exact value to its nearest class boundary (full <= -th < band < th <=
// empty, th = 0.01, loss_utils.py:40-48, loss.py:98-102), floored at the margin floor 0.002, and
// against the floor itself near the surface (|exact| < 0.1, where the band and the audit shell
// lie).  Above half of either anywhere, the decoder is lite-ineligible and every batch decodes
// exactly.
static constexpr int PROBE_POINTS = 65536, PROBE_CODES = 4;
static constexpr float PROBE_TH = 0.01f, PROBE_FLOOR = 0.002f, PROBE_MAX_RATIO = 0.5f;

static int decoder_qualify(dsr_ctx* ctx, dsr_decoder* dec) {
  const auto t0 = std::chrono::steady_clock::now();
  if (dec->D.xyz_all || dec->D.use_tanh || dec->D.ln_mask) {   // the lite kernels: the shipped topology only
    dsr_decoder_info& I = dec->info;
    I.code_len = dec->code_len;
    I.lite_eligible = 0;
    I.lite_probe_ratio = I.lite_probe_max_err = I.lite_probe_max_err_all = NAN;
    I.probe_points = I.probe_codes = 0;
    I.probe_ms = 0.0;
    return 0;
  }
  const int n = PROBE_POINTS, nc = PROBE_CODES, tot = n * nc;
  uint64_t s = 0x9E3779B97F4A7C15ull;           // fixed LCG: the probe set is part of the contract
  auto u01 = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
  };
  std::vector<float4> cand(tot);
  for (int i = 0; i < n;) {                     // uniform in the unit ball (rejection from the cube)
    const double x = 2 * u01() - 1, y = 2 * u01() - 1, z = 2 * u01() - 1;
    if (x * x + y * y + z * z >= 1.0) continue;
    for (int c = 0; c < nc; ++c) {
      int idx = i;
      float fi;
      std::memcpy(&fi, &idx, sizeof(float));
      cand[(size_t)c * n + i] = make_float4((float)x, (float)y, (float)z, fi);
    }
    ++i;
  }
  static const float scale[PROBE_CODES] = {0.0f, 0.1f, 0.3f, 1.0f};
  std::vector<float> hz((size_t)nc * CODE);
  for (int c = 0; c < nc; ++c)
    for (int k = 0; k < CODE; ++k) {               // Box-Muller
      const double r = std::sqrt(-2.0 * std::log(1.0 - u01())), t = 2.0 * M_PI * u01();
      hz[(size_t)c * CODE + k] = (float)(scale[c] * r * std::cos(t));
    }
  std::vector<ObjDesc> hd(nc);
  std::vector<ObjState> hs(nc);
  std::vector<Tile> tl, te;
  for (int c = 0; c < nc; ++c) {
    hd[c] = ObjDesc{};
    hd[c].ray_off = c * n;
    hd[c].n_rays = n;
    hd[c].cand_off = c * n;
    std::memset(&hs[c], 0, sizeof(ObjState));    // lite_margin 0: flags are not used here
    for (int t = 0; t * LTILE < n; ++t) tl.push_back(Tile{c, 0, t * LTILE, std::min(LTILE, n - t * LTILE)});
    for (int t = 0; t * TILE < n; ++t) te.push_back(Tile{c, 0, t * TILE, std::min(TILE, n - t * TILE)});
  }
  const int ntl = (int)tl.size(), nte = (int)te.size();
  DevArena mem;
  float4* dc = nullptr;
  float *dl = nullptr, *de = nullptr, *dz = nullptr, *db0 = nullptr, *db4 = nullptr;
  unsigned char* dref = nullptr;
  int *ddead = nullptr, *dntl = nullptr, *dnte = nullptr;
  ObjDesc* ddesc = nullptr;
  ObjState* dst = nullptr;
  Tile *dtl = nullptr, *dte = nullptr;
  if (!mem.alloc(&dc, tot) || !mem.alloc(&dl, tot) || !mem.alloc(&de, tot) || !mem.alloc(&dz, hz.size()) ||
      !mem.alloc(&db0, HID * nc) || !mem.alloc(&db4, HID * nc) || !mem.alloc(&dref, tot) ||
      !mem.alloc(&ddead, tot) || !mem.alloc(&dntl, 1) || !mem.alloc(&dnte, 1) || !mem.alloc(&ddesc, nc) ||
      !mem.alloc(&dst, nc) || !mem.alloc(&dtl, ntl) || !mem.alloc(&dte, nte))
    return fail(ctx, "hipMalloc failed (lite qualification)");
  hipStream_t st = ctx->stream;
  DSR_CHECK(ctx, hipMemcpyAsync(dc, cand.data(), sizeof(float4) * tot, hipMemcpyHostToDevice, st));
  DSR_CHECK(ctx, hipMemcpyAsync(dz, hz.data(), sizeof(float) * hz.size(), hipMemcpyHostToDevice, st));
  DSR_CHECK(ctx, hipMemcpyAsync(ddesc, hd.data(), sizeof(ObjDesc) * nc, hipMemcpyHostToDevice, st));
  DSR_CHECK(ctx, hipMemcpyAsync(dst, hs.data(), sizeof(ObjState) * nc, hipMemcpyHostToDevice, st));
  DSR_CHECK(ctx, hipMemcpyAsync(dtl, tl.data(), sizeof(Tile) * ntl, hipMemcpyHostToDevice, st));
  DSR_CHECK(ctx, hipMemcpyAsync(dte, te.data(), sizeof(Tile) * nte, hipMemcpyHostToDevice, st));
  DSR_CHECK(ctx, hipMemcpyAsync(dntl, &ntl, sizeof(int), hipMemcpyHostToDevice, st));
  DSR_CHECK(ctx, hipMemcpyAsync(dnte, &nte, sizeof(int), hipMemcpyHostToDevice, st));
  DSR_CHECK(ctx, hipMemsetAsync(dref, 0, tot, st));
  DSR_CHECK(ctx, hipMemsetAsync(ddead, 0, sizeof(int) * tot, st));
  const DevDecoder& D = dec->D;
  fold_codes(st, D, dz, nc, db0, db4);
  ErtArgs E{};
  E.dead = ddead;
  E.M = 1;
  E.nth = -PROBE_TH;
  E.st = dst;
  E.refine = dref;
  E.lag = lite_lag(false);
  E.audit = 0;
  E.shell = 1.0f;
  E.audit_log2 = 7;
  E.perturb = 0.0f;
  E.diag = nullptr;
  launch_lite(st, ctx->n_cu, D, {dtl, dntl, ddesc, dc, db0, db4, dl, E});
  // against the split-fp16 exact pass a lite batch runs (fwd_kernel(12)), whatever a test's
  // DSR_FWD_VARIANT selects: the XCD soft-sync variants (bit 0) need a sync counter this launch
  // has not got, and batches on them never run the lite pass anyway
  FwdQuery exact{dte, dnte, ddesc, dc, db0, db4, de};
  exact.kernel = fwd_kernel(12).kernel;
  launch_fwd(st, ctx->n_cu, D, exact);
  DSR_CHECK(ctx, hipGetLastError());
  std::vector<float> yl(tot), ye(tot);
  DSR_CHECK(ctx, hipMemcpyAsync(yl.data(), dl, sizeof(float) * tot, hipMemcpyDeviceToHost, st));
  DSR_CHECK(ctx, hipMemcpyAsync(ye.data(), de, sizeof(float) * tot, hipMemcpyDeviceToHost, st));
  DSR_CHECK(ctx, hipStreamSynchronize(st));
  double ratio = 0.0, near = 0.0, all = 0.0;
  for (int i = 0; i < tot; ++i) {
    const double e = ye[i], d = std::fabs((double)yl[i] - e);
    if (!std::isfinite(e) || !(d == d)) {          // an overflowing or NaN lite value: not eligible
      ratio = INFINITY;
      all = INFINITY;
      continue;
    }
    all = std::max(all, d);
    if (std::fabs(e) < 0.1) near = std::max(near, d);
    ratio = std::max(ratio, d / std::max((double)PROBE_FLOOR, std::fabs(std::fabs(e) - (double)PROBE_TH)));
  }
  dsr_decoder_info& I = dec->info;
  I.code_len = dec->code_len;
  I.lite_probe_ratio = ratio;
  I.lite_probe_max_err = near;
  I.lite_probe_max_err_all = all;
  I.lite_eligible = (ratio <= PROBE_MAX_RATIO && near <= PROBE_MAX_RATIO * PROBE_FLOOR) ? 1 : 0;
  I.probe_points = n;
  I.probe_codes = nc;
  I.probe_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

int dsr_decoder_load(dsr_ctx* ctx, const dsr_decoder_desc* d, const float* w, size_t n_floats,
                     dsr_decoder** out) {
  if (!ctx || !d || !w || !out) return fail(ctx, "null argument");
  *out = nullptr;
  // The DeepSDF topology DSP-SLAM ships (deep_sdf_decoder.py with dims=[512]*8, latent_in=[4],
  // weight_norm) at CodeLength 64 or 32 (LocalMapping_util.cc:416-422 handles both), plus the
  // module's use_tanh and xyz_in_all switches (:46-47, :65-67, :89-94; round 4).  Anything else
  // — LayerNorm layers among them — is rejected loudly.
  if (d->code_len != 64 && d->code_len != 32) return fail(ctx, "libdsr supports code_len 64 or 32");
  const int XA = d->xyz_in_all ? 1 : 0, H = XA ? HID - 3 : HID;   // xyz_in_all: 509 outputs
  const int L = d->code_len, l3 = HID - (L + 3);           // lin3 out: 445 / 477
  const int od[9] = {H, H, H, l3, H, H, H, H, 1};
  const int id[9] = {L + 3, 512, 512, 512, 512, 512, 512, 512, 512};
  if (d->n_layers != 9) return fail(ctx, "libdsr supports the 9-layer (dims=[512]*8) DeepSDF decoder only");
  for (int i = 0; i < 9; ++i)
    if (d->out_dim[i] != od[i] || d->in_dim[i] != id[i])
      return fail(ctx, "unsupported decoder layer shapes (expected DeepSDF 8x512 with latent_in=[4])");
  if (d->latent_in != 4) return fail(ctx, "latent_in must be [4]");
  if (d->use_tanh != 0 && d->use_tanh != 1) return fail(ctx, "use_tanh must be 0 or 1");
  if (d->xyz_in_all != 0 && d->xyz_in_all != 1) return fail(ctx, "xyz_in_all must be 0 or 1");
  if (d->norm_mask & ~0xFF) return fail(ctx, "norm_mask: LayerNorm may follow lin0..lin7 only");
  if ((XA || d->use_tanh || d->norm_mask) && (fwd_variant() != 12 || jac_variant() != 12))
    return fail(ctx, "use_tanh / xyz_in_all / LayerNorm decoders run on the split-fp16 kernels only "
                     "(DSR_FWD_VARIANT / DSR_JAC_VARIANT 12)");
  size_t need = 0;
  std::vector<const float*> W(9), B(9);
  for (int i = 0; i < 9; ++i) {
    W[i] = w + need;
    need += (size_t)od[i] * id[i];
    B[i] = w + need;
    need += od[i];
  }
  // LayerNorm layers' (gamma, beta) follow the linear layers, in layer order (deep_sdf_decoder.py:58-63)
  std::vector<const float*> LG(8, nullptr), LB(8, nullptr);
  for (int j = 0; j < 8; ++j)
    if ((d->norm_mask >> j) & 1) {
      LG[j] = w + need;
      need += od[j];
      LB[j] = w + need;
      need += od[j];
    }
  if (n_floats != need) return fail(ctx, "weight buffer has the wrong size");
  hipSetDevice(ctx->device);

  // rows beyond a layer's outputs (xyz_in_all: 509..511) are zero weights (and zero bias below)
  auto Wat = [&](int l, int r, int c) { return r < od[l] ? W[l][(size_t)r * id[l] + c] : 0.f; };
  // Everything downstream uses the 64-D layout: a 32-D decoder's code columns 32..63 are zero
  // (its J_code entries there are exactly 0, H's code block there k3 I, its step 0: the 39-
  // parameter system of the reference, solved inside the 71 one).  lin4's input is [h3 (l3) |
  // code (L) | xyz (3)]; the GEMMs see h3 | xyz, K4 deep (448 = 445 + 3; 512 >= 477 + 3), the code
  // is folded into the per-object bias.
  // (the GEMM k loops are unrolled for 14 or 16 k steps: lin4's h3 | xyz depth and lin3^T's depth
  // pad to 448 or 512 — zero weights over the ReLU'd zero rows of lin3's padded outputs)
  const int K4 = l3 + 3 <= 448 ? 448 : 512;
  auto E0 = [&](int r, int c) {            // lin0 in the 64-D layout: [code (64) | xyz (3)]
    return c < CODE ? (c < L ? Wat(0, r, c) : 0.f) : Wat(0, r, L + (c - CODE));
  };
  auto A3 = [&](int r, int c) { return r < l3 ? Wat(3, r, c) : 0.f; };
  auto A4 = [&](int r, int c) { return c < l3 ? Wat(4, r, c) : (c < l3 + 3 ? Wat(4, r, l3 + L + (c - l3)) : 0.f); };
  std::vector<std::vector<float>> blobs;
  std::vector<size_t> offs;
  size_t total = 0;
  auto add = [&](std::vector<float>&& v) {
    offs.push_back(total);
    total += (v.size() + 63) / 64 * 64;     // 256-B alignment
    blobs.push_back(std::move(v));
    return (int)blobs.size() - 1;
  };
  int hf[8] = {-1}, hb[8] = {-1}, hbias[8] = {-1};
  int Kf[8] = {0}, Kb[8] = {0};
  // split-fp16 forward fragments (stored as raw float storage in the same blob)
  int hf16[8] = {-1}, sw16[8] = {0};
  // the packs' lo pieces by error feedback against each GEMM's inputs at a probe set (pack_frag16)
  const int K3b = l3 <= 448 ? 448 : 512;
  const DecoderProbe probe = decoder_probe(od, id, W, B, LG, LB, L, l3, XA, K4, K3b, d->use_tanh, true);
  for (int l = 1; l <= 7; ++l) {
    std::vector<_Float16> v16;
    if (l == 3) {
      sw16[l] = pack_frag16(v16, 512, 512, A3, &probe.fwd[l]);
    } else if (l == 4) {
      sw16[l] = pack_frag16(v16, 512, K4, A4, &probe.fwd[l]);
    } else {
      sw16[l] = pack_frag16(v16, 512, 512, [&](int r, int c) { return Wat(l, r, c); }, &probe.fwd[l]);
    }
    std::vector<float> as_f((v16.size() + 1) / 2);
    std::memcpy(as_f.data(), v16.data(), v16.size() * sizeof(_Float16));
    hf16[l] = add(std::move(as_f));
  }
  // lite-pass fragments: fp16(W) without the 2^sw scale, so the lite epilogue needs no
  // rescale multiply (same lane layout as pack_frag16's hi pieces, packed densely)
  int hl16[8] = {-1};
  for (int l = 1; l <= 7; ++l) {
    const int K = (l == 4) ? K4 : 512, T = K / 32;
    std::vector<_Float16> v16((size_t)32 * T * 64 * 8);
    for (int rb = 0; rb < 32; ++rb)
      for (int t = 0; t < T; ++t)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j) {
            const int r = 16 * rb + (lane & 15), c = 32 * t + 8 * (lane >> 4) + j;
            float x;
            if (l == 3) x = A3(r, c);
            else if (l == 4) x = A4(r, c);
            else x = Wat(l, r, c);
            v16[(((size_t)rb * T + t) * 64 + lane) * 8 + j] = (_Float16)x;
          }
    std::vector<float> as_f((v16.size() + 1) / 2);
    std::memcpy(as_f.data(), v16.data(), v16.size() * sizeof(_Float16));
    hl16[l] = add(std::move(as_f));
  }
  for (int l = 1; l <= 7; ++l) {
    std::vector<float> v;
    if (l == 3) {
      Kf[l] = 512;
      pack_frag(v, 512, 512, A3);
    } else if (l == 4) {
      Kf[l] = K4;
      pack_frag(v, 512, K4, A4);
    } else {
      Kf[l] = 512;
      pack_frag(v, 512, 512, [&](int r, int c) { return Wat(l, r, c); });
    }
    hf[l] = add(std::move(v));
  }
  int hb16[8] = {-1}, swb16[8] = {0};
  for (int l = 0; l <= 7; ++l) {
    std::vector<_Float16> v16;
    if (l == 0) {
      swb16[l] = pack_frag16(v16, 80, 512, [&](int r, int c) { return r < IN ? E0(c, r) : 0.f; }, &probe.bwd[0]);
    } else if (l == 3) {
      swb16[l] = pack_frag16(v16, 512, K3b, [&](int r, int c) { return A3(c, r); }, &probe.bwd[3]);
    } else {
      swb16[l] = pack_frag16(v16, 512, 512, [&](int r, int c) { return Wat(l, c, r); }, &probe.bwd[l]);
    }
    std::vector<float> as_f((v16.size() + 1) / 2);
    std::memcpy(as_f.data(), v16.data(), v16.size() * sizeof(_Float16));
    hb16[l] = add(std::move(as_f));
  }
  for (int l = 1; l <= 7; ++l) {
    std::vector<float> v;
    if (l == 3) {
      Kb[l] = K3b;
      pack_frag(v, 512, K3b, [&](int r, int c) { return A3(c, r); });
    } else {
      Kb[l] = 512;
      pack_frag(v, 512, 512, [&](int r, int c) { return Wat(l, c, r); });
    }
    hb[l] = add(std::move(v));
  }
  {
    std::vector<float> v;
    Kb[0] = 512;
    pack_frag(v, 80, 512, [&](int r, int c) { return r < IN ? E0(c, r) : 0.f; });
    hb[0] = add(std::move(v));
  }
  for (int l = 0; l <= 7; ++l) {
    std::vector<float> v(512, 0.f);
    for (int i = 0; i < od[l]; ++i) v[i] = B[l][i];
    hbias[l] = add(std::move(v));
  }
  std::vector<float> w0x(512 * 3), w0z(512 * 64), w4z(512 * 64), w8(512);
  for (int n = 0; n < 512; ++n) {
    for (int i = 0; i < 3; ++i) w0x[n * 3 + i] = Wat(0, n, L + i);
    for (int k = 0; k < 64; ++k) {
      w0z[k * 512 + n] = k < L ? Wat(0, n, k) : 0.f;          // k-major: the fold's loads coalesce over n
      w4z[k * 512 + n] = k < L ? Wat(4, n, l3 + k) : 0.f;
    }
    w8[n] = Wat(8, 0, n);
  }
  const int h0x = add(std::move(w0x)), h0z = add(std::move(w0z)), h4z = add(std::move(w4z)),
            h8 = add(std::move(w8));
  int hlg[8], hlb[8];
  for (int j = 0; j < 8; ++j) {
    hlg[j] = hlb[j] = -1;
    if (!LG[j]) continue;
    std::vector<float> g(512, 0.f), bb(512, 0.f);     // zero beyond out_dim: padded rows stay 0
    for (int i = 0; i < od[j]; ++i) {
      g[i] = LG[j][i];
      bb[i] = LB[j][i];
    }
    hlg[j] = add(std::move(g));
    hlb[j] = add(std::move(bb));
  }

  auto* dec = new dsr_decoder();
  dec->ctx = ctx;
  dec->code_len = L;
  dec->bytes = total * sizeof(float);
  if (hipMalloc(&dec->dmem, dec->bytes) != hipSuccess) {
    delete dec;
    return fail(ctx, "hipMalloc failed for decoder weights");
  }
  std::vector<float> host(total, 0.f);
  for (size_t i = 0; i < blobs.size(); ++i)
    std::copy(blobs[i].begin(), blobs[i].end(), host.begin() + offs[i]);
  if (hipMemcpy(dec->dmem, host.data(), dec->bytes, hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(dec->dmem);
    delete dec;
    return fail(ctx, "hipMemcpy failed for decoder weights");
  }
  auto P = [&](int h) { return dec->dmem + offs[h]; };
  DevDecoder& D = dec->D;
  for (int l = 0; l < 8; ++l) {
    D.Wf[l] = (l >= 1) ? reinterpret_cast<const float4*>(P(hf[l])) : nullptr;
    D.Kf[l] = Kf[l];
    D.Wb[l] = reinterpret_cast<const float4*>(P(hb[l]));
    D.Kb[l] = Kb[l];
    D.bias[l] = P(hbias[l]);
  }
  D.W0x = P(h0x);
  D.W0z = P(h0z);
  D.W4z = P(h4z);
  D.W8 = P(h8);
  D.b8 = B[8][0];
  D.code_len = L;
  D.l3 = l3;
  D.xyz_all = XA;
  D.use_tanh = d->use_tanh ? 1 : 0;
  D.ln_mask = d->norm_mask & 0xFF;
  for (int j = 0; j < 8; ++j) {
    D.ln_dim[j] = od[j];
    D.ln_g[j] = hlg[j] >= 0 ? P(hlg[j]) : nullptr;
    D.ln_b[j] = hlb[j] >= 0 ? P(hlb[j]) : nullptr;
  }
  for (int l = 0; l < 8; ++l) {
    D.Wh_raw[l] = (l >= 1) ? reinterpret_cast<const _Float16*>(P(hf16[l])) : nullptr;
    D.Wl_raw[l] = (l >= 1) ? reinterpret_cast<const _Float16*>(P(hl16[l])) : nullptr;
    D.sw[l] = sw16[l];
    D.Wbh_raw[l] = reinterpret_cast<const _Float16*>(P(hb16[l]));
    D.swb[l] = swb16[l];
  }
  const int rc = decoder_qualify(ctx, dec);       // may a batch trust the lite pass with it?
  if (rc) {
    hipFree(dec->dmem);
    delete dec;
    return rc;
  }
  *out = dec;
  return 0;
}

int dsr_decoder_free(dsr_ctx* ctx, dsr_decoder* dec) {
  if (!dec) return 0;
  hipSetDevice(dec->ctx->device);
  hipFree(dec->dmem);
  delete dec;
  (void)ctx;
  return 0;
}

int dsr_decoder_info_get(const dsr_decoder* dec, dsr_decoder_info* info) {
  if (!dec || !info) return -2;
  *info = dec->info;
  return 0;
}

// ------------------------------------------------------------------------------------
// batches
// ------------------------------------------------------------------------------------
// Render-pass schedule of the early ray termination (k_sample_pass): in-ball rank
// boundaries, DSR_RENDER_PASSES="8,12,16,20,24,32" style (ascending, each < M); one pass
// [0, M) when empty ("0" disables termination).  Default: fine windows for large batches
// (fewer wasted samples), coarse ones for small batches whose passes are too short to
// fill the chip: each pass costs at least one tile's latency, extra samples are nearly free
// (measured: 64 KITTI objects 186 vs 176 obj/s, 8 Redwood objects 10.6 vs 11.2 ms per
// batch; round 2, same box: 8 KITTI objects 341-346 obj/s with 16,24 vs 337-341 with
// 8,16,24, keyframe batch 4.82 vs 4.98 ms).  Below 100k ray samples (one or two Redwood
// objects: the reference's one-call-per-detection pattern) one pass: its tiles fit one round of
// the chip, so every extra pass is a whole tile latency plus a sample pass (round 3, one box: a
// Redwood object per reconstruct_object call 4.1 -> 3.1 ms; a KITTI object, 112k samples, 9.8 ms
// either way; the 8-hypothesis keyframe batch 4.90 ms with 16,24 vs 5.90 with one pass).
// A batch whose first 16-rank window would spill just past one round of lite tiles (n_cu
// 128-point tiles: one KITTI-sized object per call) runs TWO passes, ranks [0, 20) and the rest:
// one KITTI object per call 8.14 ms with round 4's round-filling first window (14,24), 7.88 with
// 20 (24: 7.91, 16: 8.76, one pass 8.77; r5bb, 40 calls each, same box).
static std::vector<int> render_passes(int M, long samples, long rays, int n_cu) {
  const char* e = hook_env("DSR_RENDER_PASSES");
  std::string spec = e ? e : (samples >= 1000000 ? "8,12,16,20,24,32" : samples >= 100000 ? "16,24" : "0");
  const long round = (long)n_cu * LTILE;
  if (!e && spec == "16,24" && rays > 0 && rays * 16 > round && rays * 12 <= round)
    spec = "20";
  std::vector<int> r{0};
  size_t p = 0;
  while (p < spec.size()) {
    const size_t q = spec.find(',', p);
    const int v = atoi(spec.substr(p, q == std::string::npos ? std::string::npos : q - p).c_str());
    if (v > r.back() && v < M) r.push_back(v);
    if (q == std::string::npos) break;
    p = q + 1;
  }
  r.push_back(M);
  return r;
}
// Per-object render-pass windows (choose_windows, dsr_kernels.hpp): on by default
// for a lite batch on its default multi-pass schedule.  Under DSR_TEST_HOOKS=1
// DSR_ADAPTIVE_WINDOWS=0 keeps the fixed windows; an explicit DSR_RENDER_PASSES keeps its fixed
// windows too unless DSR_ADAPTIVE_WINDOWS=1 is set beside it (the windows then start from that
// schedule).  Returns the pass count the objects re-choose windows for, 0: fixed windows.
static int adaptive_windows(const std::vector<int>& passes, bool lite) {
  const int np = (int)passes.size() - 1;
  if (!lite || np < 2 || np + 1 > WIN_MAX) return 0;
  const char* e = hook_env("DSR_ADAPTIVE_WINDOWS");
  const bool on = e ? atoi(e) != 0 : hook_env("DSR_RENDER_PASSES") == nullptr;
  return on ? np : 0;
}
static WinTable win_table(const std::vector<int>& passes) {
  WinTable w{};
  if ((int)passes.size() > WIN_MAX) return w;    // (a longer explicit schedule: kernel arguments only)
  w.n = (int)passes.size();
  for (int i = 0; i < w.n; ++i) w.b[i] = (unsigned char)passes[i];
  return w;
}
static size_t ev_per_iter(const dsr_batch* b) { return 2 * (b->passes.size() - 1 + (b->lite ? 1 : 0)) + 2; }

// A batch buffer: the smallest pooled block that fits (and wastes at most half of itself
// plus 1 MB), else hipMalloc.
static int batch_alloc(dsr_batch* b, void** p, size_t bytes) {
  dsr_ctx* ctx = b->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  bytes = std::max<size_t>(256, (bytes + 255) & ~(size_t)255);
  auto it = ctx->pool.lower_bound(bytes);
  if (it != ctx->pool.end() && it->first <= 2 * bytes + ((size_t)1 << 20)) {
    *p = it->second;
    b->allocs.emplace_back(it->second, it->first);
    ctx->pool_bytes -= it->first;
    ctx->pool.erase(it);
    return 0;
  }
  if (hipMalloc(p, bytes) != hipSuccess) {
    // pooled blocks that did not fit may be what fills the device: return them and retry once
    (void)hipGetLastError();
    for (auto& kv : ctx->pool) hipFree(kv.second);
    ctx->pool.clear();
    ctx->pool_bytes = 0;
    if (hipMalloc(p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, "hipMalloc failed (" + std::to_string(bytes) + " B)");
    }
  }
  b->allocs.emplace_back(*p, bytes);
  return 0;
}
static hipError_t pool_event(dsr_ctx* ctx, hipEvent_t* e, bool timing) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  auto& v = timing ? ctx->ev_timing : ctx->ev_plain;
  if (!v.empty()) {
    *e = v.back();
    v.pop_back();
    return hipSuccess;
  }
  return timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming);
}

// Lite-pass audit (dsr_dev.hpp: lite_flag): the shipped guard is always on — out-of-band
// samples with |y| < th + (1 + shell)*margin, shell = 1 (`shell` margins beyond the band edge),
// are audited, plus a hashed 2^-7 share of all other decoded samples.  Only under
// DSR_TEST_HOOKS=1 (reported in dsr_stats.test_hooks) does a batch read DSR_LITE_AUDIT (0: off),
// DSR_LITE_SHELL, DSR_LITE_AUDIT_LOG2 (0: every sample — the audit-everything survey,
// tools/lite_audit_all.py) and the DSR_LITE_PERTURB test hook: a stray variable cannot switch
// off or thin out the misclassification guard of a production run.
static float env_hook(bool hooks, const char* k, float d) {
  const char* e = hooks ? getenv(k) : nullptr;
  return e ? (float)atof(e) : d;
}
static ErtArgs lite_settings(bool hooks) {
  ErtArgs E{};
  E.audit = env_hook(hooks, "DSR_LITE_AUDIT", 1.0f) == 0.0f ? 0 : 1;
  E.shell = env_hook(hooks, "DSR_LITE_SHELL", 1.0f);
  E.audit_log2 = std::max(0, std::min(24, (int)env_hook(hooks, "DSR_LITE_AUDIT_LOG2", 7.0f)));
  E.perturb = env_hook(hooks, "DSR_LITE_PERTURB", 0.0f);
  E.lag = lite_lag(hooks);
  return E;
}

static GNParams make_params(const dsr_optim_params* p, bool hooks) {
  GNParams P;
  P.k1 = p->k1; P.k2 = p->k2; P.k3 = p->k3; P.k4 = p->k4;
  P.b1 = p->b1; P.b2 = p->b2; P.lr = p->lr; P.s_damp = p->s_damp;
  P.cut_off = p->cut_off; P.iters = p->num_iterations; P.M = p->num_depth_samples;
  P.raw_residual = 0;
  P.n_win = 0;                                   // (a batch sets it: adaptive_windows)
  // lite-pass margin: th in the first iteration, then max(0.002, 4 x the
  // largest |lite - exact| the object's band and audit samples showed; the audit guards it).
  // DSR_LITE_MARGIN / _FLOOR / _SAFETY only under DSR_TEST_HOOKS=1 (lite_settings)
  P.lite_margin0 = env_hook(hooks, "DSR_LITE_MARGIN", p->cut_off);   // th (0.01 in every reference config)
  P.lite_floor = env_hook(hooks, "DSR_LITE_FLOOR", 0.002f);
  P.lite_safety = env_hook(hooks, "DSR_LITE_SAFETY", 4.0f);
  return P;
}

int dsr_batch_destroy(dsr_batch* b) {
  if (!b) return 0;
  dsr_ctx* ctx = b->ctx;
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  // the blocks go back to the pool: no kernel of this batch may still be using them
  for (size_t g = 0; g < std::max<size_t>(1, b->groups.size()); ++g) hipStreamSynchronize(ctx->gstream[g]);
  if (b->graph) hipGraphExecDestroy(b->graph);
  for (auto& sg : b->stage)
    if (sg.host) hipHostFree(sg.host);
  if (b->ingest.host) hipHostFree(b->ingest.host);
  if (b->ingest.dev) hipFree(b->ingest.dev);
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (b->up_ev) ctx->ev_plain.push_back(b->up_ev);
  for (auto& e : b->ev)
    if (e) ctx->ev_timing.push_back(e);
  for (hipEvent_t e : b->join_ev)
    if (e) ctx->ev_plain.push_back(e);
  if (b->fork_ev) ctx->ev_plain.push_back(b->fork_ev);
  if (b->done_ev) ctx->ev_plain.push_back(b->done_ev);
  for (auto& a : b->allocs) {
    if (ctx->pool_bytes + a.second <= POOL_CAP) {
      ctx->pool.emplace(a.second, a.first);
      ctx->pool_bytes += a.second;
    } else {
      hipFree(a.first);
    }
  }
  delete b;
  return 0;
}

// the one owner of a batch under construction: a failure exit destroys it after fail() has set the
// error (dsr_batch_destroy never writes it); success releases it to the caller
namespace {   // (internal linkage: the library exports no symbol for the owner)
struct BatchDeleter {
  void operator()(dsr_batch* b) const { dsr_batch_destroy(b); }
};
}  // namespace
using BatchOwner = std::unique_ptr<dsr_batch, BatchDeleter>;

static bool graph_enabled() {        // DSR_GRAPH=1: replay re-run batches as hipGraphs
  const char* ge = getenv("DSR_GRAPH");
  return ge && atoi(ge) != 0;
}

static int batch_create_impl(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p,
                             int n_obj, const dsr_object_in* in, bool trace, dsr_batch** out,
                             bool one_group = false, const std::vector<int>* views = nullptr,
                             const float* cview = nullptr) {
  if (!ctx || !dec || !p || !out || (n_obj > 0 && !in)) return fail(ctx, "null argument");
  *out = nullptr;
  if (n_obj <= 0) return fail(ctx, "n_obj must be > 0");
  if (p->code_len != dec->code_len) return fail(ctx, "optimizer code_len != decoder code_len");
  if (p->num_depth_samples < 2 || p->num_depth_samples > MAXM)
    return fail(ctx, "num_depth_samples must be in [2, 64]");
  if (p->num_iterations < 0) return fail(ctx, "num_iterations < 0");
  if (int rc = decoder_ready(ctx, dec)) return rc;
  hipSetDevice(ctx->device);
  BatchOwner owner(new dsr_batch());
  dsr_batch* b = owner.get();
  b->ctx = ctx;
  b->dec = dec;
  b->hooks = test_hooks();
  b->P = make_params(p, b->hooks);
  b->n_obj = n_obj;
  b->n_active = n_obj;
  b->iters = p->num_iterations;
  b->M = p->num_depth_samples;
  const int M = b->M;
  std::vector<float> hpts, hrays, hdobs, hz((size_t)n_obj * CODE, 0.f), ht((size_t)n_obj * 16);
  std::vector<int> hoc(n_obj), ftile_o(n_obj), jtile_o(n_obj);
  long cand_est = 0;                         // ray samples of the batch (group count heuristic)
  for (int o = 0; o < n_obj; ++o) cand_est += (long)std::max(0, in[o].n_rays) * M;
  {
    // object groups on concurrent streams: 2 for large batches (the decoder
    // grids fill the chip; more groups only overlap their launches), 4 for small batches of
    // large objects (a strong-scaled shard of 8-16 KITTI objects is bound by its latency
    // kernels, which the extra groups hide: 8 objects 317 -> 333 obj/s), 2 again for small
    // batches of small objects (8 Redwood keyframe hypotheses: 5.31 -> 5.16 ms)
    // Under DSR_GRAPH=1 the default is ONE group: ROCm 7.2 replays a captured multi-stream
    // fork/join as a graph 1.6x slower than the eager groups (keyframe batch 8.4 vs 5.2 ms,
    // whatever DEBUG_HIP_FORCE_GRAPH_QUEUES / DEBUG_CLR_GRAPH_PACKET_CAPTURE say), while a
    // one-group graph replays 3% faster than a one-group eager run (5.31 vs 5.46 ms; r3k,
    // tools/graph_queues.py).  Results are bitwise the same for any grouping.
    const char* e = getenv("DSR_STREAMS");
    int G = e ? atoi(e) : (graph_enabled() || one_group) ? 1 : ((n_obj <= 16 && cand_est >= 500000) ? 4 : 2);
    G = std::max(1, std::min(std::min(G, MAX_GROUPS), n_obj));
    if (fwd_variant() & 1) G = 1;             // the XCD soft sync assumes one fwd grid at a time
    if (views) {
      // a tied batch: the same split over the tied objects, so that a group boundary is an
      // object boundary and every view of an object runs on one stream (k_solve_views reads all
      // of them in stream order); with one view per object these are the ranges below
      const int nt = (int)views->size();
      std::vector<int> first(nt + 1, 0);
      for (int i = 0; i < nt; ++i) first[i + 1] = first[i] + (*views)[i];
      G = std::min(G, nt);
      for (int g = 0; g < G; ++g) {
        dsr_batch::Group gr;
        gr.t0 = (int)((long)nt * g / G);
        gr.nt = (int)((long)nt * (g + 1) / G) - gr.t0;
        gr.o0 = first[gr.t0];
        gr.n = first[gr.t0 + gr.nt] - gr.o0;
        b->groups.push_back(gr);
      }
    } else {
      for (int g = 0; g < G; ++g) {
        dsr_batch::Group gr;
        gr.o0 = (int)((long)n_obj * g / G);
        gr.n = (int)((long)n_obj * (g + 1) / G) - gr.o0;
        b->groups.push_back(gr);
      }
    }
    if (dec->D.ln_mask)
      for (int g = 0; g < G; ++g)
        if (!ln_workspace(ctx, g)) return fail(ctx, "hipMalloc failed (LayerNorm workspace)");
  }
  // Every group's slices of the per-ray / per-sample / per-point / per-slot buffers start on
  // a fresh 256 B line (zero padding between groups): the groups' kernels run concurrently on
  // their own streams, so no cache line holds both groups' elements (round 5 suspected that for
  // the variable decode counts of DESIGN.md §3.9; the cause was elsewhere, the layout stays).
  // DSR_GROUP_ALIGN=0 (test hook) packs the groups back to back.
  bool galign = true;
  {
    const char* e = hook_env("DSR_GROUP_ALIGN");
    if (e && atoi(e) == 0) galign = false;
  }
  std::vector<char> gfirst(n_obj, 0);
  auto up_to = [](int v, int a) { return (int)std::min<long>(INT_MAX, ((long)v + a - 1) / a * a); };
  for (size_t g = 1; g < b->groups.size(); ++g) gfirst[b->groups[g].o0] = 1;
  int pts_off = 0, ray_off = 0, cand_off = 0, slot_off = 0, ftiles = 0;
  for (int o = 0; o < n_obj; ++o) {
    const dsr_object_in& x = in[o];
    if (galign && gfirst[o]) {
      const int r1 = up_to(ray_off, 64), c1 = up_to(cand_off, 256), p1 = up_to(pts_off, 64);
      hrays.resize((size_t)r1 * 3, 0.f);
      hdobs.resize((size_t)r1, 0.f);
      hpts.resize((size_t)p1 * 3, 0.f);
      ray_off = r1;
      cand_off = c1;
      pts_off = p1;
      slot_off = up_to(slot_off, 8);
    }
    // Empty inputs are the reference's numeric failures, not errors: no surface points make
    // the sdf loss a mean of nothing (NaN, optimizer.py:137), no rays leave < 10 in-ball
    // samples (loss.py:86-88) — is_good = False, loss 0., exactly as there (golden F10)
    if (x.n_pts < 0 || (x.n_pts > 0 && !x.pts)) return fail(ctx, "bad surface points");
    if (x.n_rays < 0 || (x.n_rays > 0 && !x.rays)) return fail(ctx, "bad rays");
    if (x.n_depth < 0 || x.n_depth > x.n_rays || (x.n_depth > 0 && !x.depth))
      return fail(ctx, "depth must hold at most n_rays foreground values");
    // device offsets and tile tables are 32-bit: a batch holds at most 2^31 - 1 ray samples
    // plus surface points (HBM runs out first with kept masks, ~580 B per sample; without
    // them ~70 B per sample would let a batch pass the limit) — split larger jobs
    if ((long long)x.n_rays * M + cand_off + x.n_pts + pts_off > (long long)INT_MAX)
      return fail(ctx, "batch too large: more than 2^31 - 1 ray samples + surface points (split it)");
    ObjDesc d{};
    d.pts_off = pts_off; d.n_pts = x.n_pts;
    d.ray_off = ray_off; d.n_rays = x.n_rays; d.n_fg = x.n_depth;
    d.cand_off = cand_off; d.slot_sdf = slot_off;
    b->hdesc.push_back(d);
    if (x.n_pts > 0) hpts.insert(hpts.end(), x.pts, x.pts + (size_t)x.n_pts * 3);
    if (x.n_rays > 0) hrays.insert(hrays.end(), x.rays, x.rays + (size_t)x.n_rays * 3);
    for (int r = 0; r < x.n_rays; ++r) hdobs.push_back(r < x.n_depth ? x.depth[r] : 0.f);
    if (x.code) std::copy(x.code, x.code + dec->code_len, hz.begin() + (size_t)o * CODE);   // (rest 0)
    std::copy(x.t_cam_obj, x.t_cam_obj + 16, ht.begin() + (size_t)o * 16);
    hoc[o] = x.pose_is_obj_cam ? 1 : 0;
    const int cap = x.n_rays * M;
    pts_off += x.n_pts;
    ray_off += x.n_rays;
    cand_off += cap;
    ftile_o[o] = (cap + TILE - 1) / TILE + (x.n_pts + TILE - 1) / TILE;   // + surface tiles (exact pass)
    jtile_o[o] = (x.n_pts + TILE - 1) / TILE + (cap + TILE - 1) / TILE;
    ftiles += ftile_o[o];
    slot_off += jtile_o[o];
  }
  // (the surface points' mask / sdf slots follow the samples': their groups' slices too)
  if (galign && b->groups.size() > 1) cand_off = up_to(cand_off, 256);
  b->cand_total = cand_off;
  b->slot_total = slot_off;
  b->fwd_tile_cap = ftiles;
  b->jac_tile_cap = slot_off;
  int rc = 0;
#define ALLOC(ptr, bytes) \
  if ((rc = batch_alloc(b, (void**)&(ptr), (bytes))) != 0) return rc;
  ALLOC(b->desc, sizeof(ObjDesc) * n_obj);
  ALLOC(b->st, sizeof(ObjState) * n_obj);
  ALLOC(b->zbuf, sizeof(float) * CODE * n_obj);
  ALLOC(b->z_in, sizeof(float) * CODE * n_obj);
  ALLOC(b->t_in, sizeof(float) * 16 * n_obj);
  ALLOC(b->is_oc, sizeof(int) * n_obj);
  b->pts_floats = hpts.size();
  b->ray_slots = hdobs.size();
  ALLOC(b->pts, sizeof(float) * hpts.size());
  ALLOC(b->rays, sizeof(float) * hrays.size());
  ALLOC(b->dobs, sizeof(float) * hdobs.size());
  ALLOC(b->cand, sizeof(float4) * (size_t)cand_off);
  ALLOC(b->kpts, sizeof(float4) * (size_t)cand_off);
  ALLOC(b->dense, sizeof(float) * (size_t)cand_off);
  ALLOC(b->dead, sizeof(int) * (size_t)std::max(1, ray_off));
  ALLOC(b->rinfo, sizeof(int) * (size_t)std::max(1, ray_off));
  ALLOC(b->rwin, sizeof(int) * (size_t)std::max(1, ray_off));
#ifdef DSR_EXP_PROV
  {
    int* pa = nullptr;
    float* py = nullptr;
    int* ps = nullptr;
    int* px = nullptr;
    const int R = std::max(1, ray_off), C = std::max(1, cand_off);
    int* pj = nullptr;
    unsigned* pt = nullptr;
    ALLOC(pj, sizeof(int) * (size_t)PROV_IT * 64 * R);
    ALLOC(pt, sizeof(unsigned) * (size_t)PROV_IT * 65 * R);
    hipMemset(pj, 0xff, sizeof(int) * (size_t)PROV_IT * 64 * R);
    hipMemset(pt, 0xff, sizeof(unsigned) * (size_t)PROV_IT * 65 * R);
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_j), &pj, sizeof(pj));
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_t), &pt, sizeof(pt));
    b->prov_j = pj;
    b->prov_t = pt;
    float* pn2 = nullptr;
    ALLOC(pn2, sizeof(float) * (size_t)PROV_IT * R * 8);
    hipMemset(pn2, 0, sizeof(float) * (size_t)PROV_IT * R * 8);
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_nrm2), &pn2, sizeof(pn2));
    b->prov_nrm2 = pn2;
    float* pn = nullptr;
    ALLOC(pn, sizeof(float) * (size_t)PROV_IT * R * 12);
    hipMemset(pn, 0, sizeof(float) * (size_t)PROV_IT * R * 12);
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_nrm), &pn, sizeof(pn));
    b->prov_nrm = pn;
    unsigned* pr = nullptr;
    ALLOC(pr, sizeof(unsigned) * 2 * (size_t)PROV_IT * R * 2);
    hipMemset(pr, 0, sizeof(unsigned) * 2 * (size_t)PROV_IT * R * 2);
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_ri), &pr, sizeof(pr));
    b->prov_ri = pr;
    unsigned* ph = nullptr;
    ALLOC(ph, sizeof(unsigned) * 2 * (size_t)PROV_IT * R * 3);
    hipMemset(ph, 0, sizeof(unsigned) * 2 * (size_t)PROV_IT * R * 3);
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_h), &ph, sizeof(ph));
    b->prov_h = ph;
    ALLOC(px, sizeof(int) * (size_t)PROV_IT * R * 2);
    hipMemset(px, 0xff, sizeof(int) * (size_t)PROV_IT * R * 2);
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_xcc), &px, sizeof(px));
    b->prov_xcc = px;
    ALLOC(pa, sizeof(int) * (size_t)PROV_IT * 64 * R);
    ALLOC(py, sizeof(float) * (size_t)PROV_IT * C);
    ALLOC(ps, sizeof(int) * (size_t)PROV_IT * R);
    hipMemset(pa, 0, sizeof(int) * (size_t)PROV_IT * 64 * R);
    hipMemset(py, 0xff, sizeof(float) * (size_t)PROV_IT * C);
    hipMemset(ps, 0x7f, sizeof(int) * (size_t)PROV_IT * R);
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_alive), &pa, sizeof(pa));
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_y), &py, sizeof(py));
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_set), &ps, sizeof(ps));
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_R), &R, sizeof(R));
    hipMemcpyToSymbol(HIP_SYMBOL(g_prov_C), &C, sizeof(C));
    b->prov_alive = pa;
    b->prov_y = py;
    b->prov_set = ps;
    b->prov_R = R;
    b->prov_C = C;
  }
#endif
  {
    // The render passes over the ray chunks (a count kernel — k_sample_scan for the first pass,
    // k_sample_count after — then k_sample_emit) for one-group batches: single calls, graph-mode
    // keyframe slots, where one object's pass otherwise runs on one workgroup (DESIGN.md §3.8:
    // a KITTI call 8.77 -> 8.14 ms with the chunked first-pass scan alone, Appendix A D1; every
    // pass chunked, with the render staging of the same change, 7.50 -> 7.05 ms, r6y).
    // Multi-group batches measured equal either way and keep k_sample_pass.  The
    // scan's round-4/5 timing-dependent decode counts were wrong products of a packed-FP32
    // multiply in its loop's first trip (§3.9); these kernels are built without packed FP32.
    // DSR_PRESCAN=0/1 (test hook) forces one form.
    const char* e = hook_env("DSR_PRESCAN");
    b->prescan = e ? atoi(e) != 0 : b->groups.size() == 1;
  }
  {
    // the lite pass runs only on decoders that passed their load-time qualification
    // (decoder_qualify); DSR_LITE=0 decodes every sample exactly on any decoder
    const char* e = getenv("DSR_LITE");
    b->lite = !(e && atoi(e) == 0) && !(fwd_variant() & 1) && dec->info.lite_eligible;
  }
  if (b->lite) {
    const char* km = hook_env("DSR_KEEP_MASKS");
    if (!(km && atoi(km) == 0)) {     // 512 B of masks per sample of the worst case: HBM is ample
      // slots: the samples' (cand order), then the surface points' (MaskArgs.surf_base)
      ALLOC(b->ma.msk, sizeof(uint16_t) * 256 * ((size_t)cand_off + pts_off));
      ALLOC(b->ma.yv, sizeof(float) * ((size_t)cand_off + pts_off));
      ALLOC(b->ma.slotmap, sizeof(int) * (size_t)std::max(1, cand_off));
      ALLOC(b->kslot, sizeof(int) * (size_t)std::max(1, cand_off));
      b->ma.kslot = b->kslot;
      // the exact pass runs the surface points' forward too (MaskArgs.pts), so the Jacobian
      // kernel chains only backward passes: bitwise the same results; it shortens small
      // batches' chains (8-object Redwood keyframe -7%) and costs 64-object batches ~1%
      // (the forward moves, the MFMA work is equal).  DSR_SURFACE_EXACT=0/1 overrides.
      const char* se = hook_env("DSR_SURFACE_EXACT");
      const bool surf = se ? atoi(se) != 0 : n_obj <= 16;
      if (surf && fwd_variant() == 12) {
        b->ma.pts = b->pts;
        b->ma.surf_base = cand_off;
      }
    }
    ALLOC(b->refine, (size_t)std::max(1, cand_off));
    ALLOC(b->rbits, sizeof(uint64_t) * (size_t)std::max(1, ray_off));
    ALLOC(b->abits, sizeof(uint64_t) * (size_t)std::max(1, ray_off));
    if (hipMemsetAsync(b->refine, 0, (size_t)std::max(1, cand_off), ctx->stream) != hipSuccess)
      return fail(ctx, "hipMemset failed");
  }
  ALLOC(b->kres, sizeof(float) * (size_t)cand_off);
  ALLOC(b->kst, sizeof(float4) * (size_t)cand_off);
  ALLOC(b->rst, sizeof(float) * (size_t)cand_off);
  if (b->kslot) ALLOC(b->sst, sizeof(int) * (size_t)cand_off);
  ALLOC(b->bias0f, sizeof(float) * HID * n_obj);
  ALLOC(b->bias4f, sizeof(float) * HID * n_obj);
  for (auto& gr : b->groups) {
    gr.c0 = b->hdesc[gr.o0].cand_off;
    gr.c1 = b->hdesc[gr.o0 + gr.n - 1].cand_off + b->hdesc[gr.o0 + gr.n - 1].n_rays * M;
    size_t ft = 0, jt = 0;
    for (int o = gr.o0; o < gr.o0 + gr.n; ++o) { ft += ftile_o[o]; jt += jtile_o[o]; }
    ALLOC(gr.tiles_f, sizeof(Tile) * std::max<size_t>(1, ft));
    ALLOC(gr.tiles_j, sizeof(Tile) * std::max<size_t>(1, jt));
    ALLOC(gr.nt_f, sizeof(int));
    ALLOC(gr.nt_j, sizeof(int));
    ALLOC(gr.sync, 8 * 32 * sizeof(unsigned));
    std::vector<RenderChunk> rch;
    std::vector<int2> och;
    for (int o = gr.o0; o < gr.o0 + gr.n; ++o) {
      const int first = (int)rch.size(), nch = (b->hdesc[o].n_rays + RENDER_RAYS - 1) / RENDER_RAYS;
      for (int c = 0; c < nch; ++c) rch.push_back(RenderChunk{o - gr.o0, c * RENDER_RAYS, first, nch});
      och.push_back(make_int2(first, nch));
    }
    gr.n_rch = (int)rch.size();
    ALLOC(gr.rchunks, sizeof(RenderChunk) * rch.size());
    ALLOC(gr.ccnt, sizeof(int) * rch.size());
    ALLOC(gr.scnt, 2 * sizeof(int) * rch.size());
    ALLOC(gr.och, sizeof(int2) * och.size());
    if (!rch.empty() &&
        (hipMemcpy(gr.rchunks, rch.data(), sizeof(RenderChunk) * rch.size(), hipMemcpyHostToDevice) != hipSuccess ||
         hipMemcpy(gr.och, och.data(), sizeof(int2) * och.size(), hipMemcpyHostToDevice) != hipSuccess))
      return fail(ctx, "hipMemcpy (render chunks) failed");
  }
  ALLOC(b->slots, sizeof(float) * SLOT_FLOATS * (size_t)slot_off);
  ALLOC(b->sred, sizeof(float) * SRED_STRIDE * (size_t)n_obj);
  b->lite_cfg = lite_settings(b->hooks);
  b->loop_iters = b->iters + ((b->lite && b->lite_cfg.audit && b->iters > 0) ? 1 : 0);
  ALLOC(b->diag, sizeof(int) * STD_INTS);
  ALLOC(b->counts, sizeof(int) * COUNT_STRIDE * (size_t)std::max(1, b->loop_iters) * n_obj);
  ALLOC(b->out, sizeof(dsr_object_out) * n_obj);
  std::vector<int2> htie;
  if (views) {
    b->n_tied = (int)views->size();
    for (const auto& gr : b->groups)
      for (int i = gr.t0, o = gr.o0; i < gr.t0 + gr.nt; o += (*views)[i], ++i) {
        htie.push_back(make_int2(o - gr.o0, (*views)[i]));
        b->tie_multi = b->tie_multi || (*views)[i] > 1;
      }
    ALLOC(b->tie, sizeof(int2) * htie.size());
    ALLOC(b->cview, sizeof(float) * 16 * n_obj);
    ALLOC(b->fail_view, sizeof(int) * htie.size());
  }
  if (trace) {
    const size_t it = std::max(1, b->iters);
    ALLOC(b->tr_H, sizeof(float) * TRACE_H_STRIDE * it * n_obj);
    ALLOC(b->tr_v, sizeof(float) * TRACE_V_STRIDE * it * n_obj);
    ALLOC(b->tr_i, sizeof(int) * TRACE_I_STRIDE * it * n_obj);
  }
#undef ALLOC
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up(b->desc, b->hdesc.data(), sizeof(ObjDesc) * n_obj) ||
      !up(b->z_in, hz.data(), sizeof(float) * hz.size()) ||
      !up(b->t_in, ht.data(), sizeof(float) * ht.size()) ||
      !up(b->is_oc, hoc.data(), sizeof(int) * n_obj) ||
      !up(b->pts, hpts.data(), sizeof(float) * hpts.size()) ||
      !up(b->rays, hrays.data(), sizeof(float) * hrays.size()) ||
      !up(b->dobs, hdobs.data(), sizeof(float) * hdobs.size()) ||
      (views && (!up(b->tie, htie.data(), sizeof(int2) * htie.size()) ||
                 !up(b->cview, cview, sizeof(float) * 16 * n_obj))))
    return fail(ctx, "hipMemcpy (inputs) failed");
  if (trace) {
    hipMemsetAsync(b->tr_H, 0, sizeof(float) * TRACE_H_STRIDE * std::max(1, b->iters) * n_obj, ctx->stream);
    hipMemsetAsync(b->tr_v, 0, sizeof(float) * TRACE_V_STRIDE * std::max(1, b->iters) * n_obj, ctx->stream);
    hipMemsetAsync(b->tr_i, 0, sizeof(int) * TRACE_I_STRIDE * std::max(1, b->iters) * n_obj, ctx->stream);
  }
  b->passes = render_passes(M, (long)cand_off, (long)ray_off, ctx->n_cu);
  b->P.n_win = adaptive_windows(b->passes, b->lite);
  b->ev.resize((size_t)std::max(1, b->loop_iters) * b->groups.size() * ev_per_iter(b) + 2);
  b->join_ev.resize(b->groups.size());
  for (auto& e : b->ev)
    if (pool_event(ctx, &e, true) != hipSuccess) return fail(ctx, "hipEventCreate failed");
  for (auto& e : b->join_ev)
    if (pool_event(ctx, &e, false) != hipSuccess) return fail(ctx, "hipEventCreate failed");
  if (pool_event(ctx, &b->done_ev, false) != hipSuccess || pool_event(ctx, &b->fork_ev, false) != hipSuccess)
    return fail(ctx, "hipEventCreate failed");
  *out = owner.release();
  return 0;
}

int dsr_batch_create(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, int n_obj,
                     const dsr_object_in* in, dsr_batch** out) {
  return batch_create_impl(ctx, dec, p, n_obj, in, false, out);
}

// A capacity batch is an ordinary batch laid out for max_obj objects of max_pts points and
// max_rays rays each (every buffer, tile table, render-chunk table and object group sized for
// that), whose slots dsr_batch_refill fills; slots without an object hold an empty object (no
// points, no rays: the reference's numeric failure, which every kernel skips after iteration 0).
int dsr_batch_create_capacity(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, int max_obj,
                              int max_pts, int max_rays, int flags, dsr_batch** out) {
  if (!ctx || !dec || !p || !out) return fail(ctx, "null argument");
  *out = nullptr;
  if (max_obj <= 0 || max_pts < 0 || max_rays < 0) return fail(ctx, "capacities must be > 0");
  if (flags & ~DSR_BATCH_GRAPH) return fail(ctx, "unknown batch flags");
  const std::vector<float> zp((size_t)std::max(1, max_pts) * 3, 0.f), zr((size_t)std::max(1, max_rays) * 3, 0.f);
  std::vector<dsr_object_in> in(max_obj);
  for (auto& x : in) {
    x = dsr_object_in{};
    for (int i = 0; i < 16; i += 5) x.t_cam_obj[i] = 1.f;
    x.pts = zp.data();
    x.n_pts = max_pts;
    x.rays = zr.data();
    x.n_rays = max_rays;
    x.depth = nullptr;
    x.n_depth = 0;
  }
  dsr_batch* b = nullptr;
  int rc = batch_create_impl(ctx, dec, p, max_obj, in.data(), false, &b, (flags & DSR_BATCH_GRAPH) != 0);
  if (rc) return rc;
  BatchOwner owner(b);
  b->capacity = true;
  b->cap_graph = (flags & DSR_BATCH_GRAPH) != 0;
  b->max_pts = max_pts;
  b->max_rays = max_rays;
  const std::pair<void*, size_t> bufs[] = {
      {b->desc, sizeof(ObjDesc) * max_obj},          {b->t_in, sizeof(float) * 16 * max_obj},
      {b->z_in, sizeof(float) * CODE * max_obj},     {b->is_oc, sizeof(int) * max_obj},
      {b->pts, sizeof(float) * b->pts_floats},
      {b->rays, sizeof(float) * 3 * b->ray_slots},
      {b->dobs, sizeof(float) * b->ray_slots}};
  for (const auto& kv : bufs) {
    dsr_batch::Stage sg;
    sg.dev = kv.first;
    sg.bytes = std::max<size_t>(kv.second, 4);
    if (hipHostMalloc(&sg.host, sg.bytes, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return fail(ctx, "hipHostMalloc failed (capacity batch staging)");
    }
    std::memset(sg.host, 0, sg.bytes);
    b->stage.push_back(sg);
  }
  if (pool_event(ctx, &b->up_ev, false) != hipSuccess) return fail(ctx, "hipEventCreate failed");
  rc = dsr_batch_refill(b, 0, nullptr);          // every slot empty until the first fill
  if (rc) return rc;
  *out = owner.release();
  return 0;
}

// inverse of a rigid 4x4 (x_view = t_view_ref x_ref) in fp64, rounded once: [R^T | -R^T t].
// False unless the last row is 0 0 0 1 and R^T R = I within 1e-4 with det R > 0.
static bool rigid_inverse(const float* t, float* out) {
  if (t[12] != 0.f || t[13] != 0.f || t[14] != 0.f || t[15] != 1.f) return false;
  double R[3][3], tr[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[i][j] = (double)t[i * 4 + j];
    tr[i] = (double)t[i * 4 + 3];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += R[k][i] * R[k][j];
      if (!(std::fabs(s - (i == j ? 1.0 : 0.0)) <= 1e-4)) return false;       // (NaN fails too)
    }
  const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                     R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
  if (!(det > 0.0)) return false;
  for (int i = 0; i < 3; ++i) {
    if (!std::isfinite(tr[i])) return false;
    for (int j = 0; j < 3; ++j) out[i * 4 + j] = (float)R[j][i];
    out[i * 4 + 3] = (float)(-(R[0][i] * tr[0] + R[1][i] * tr[1] + R[2][i] * tr[2]));
  }
  out[12] = out[13] = out[14] = 0.f;
  out[15] = 1.f;
  return true;
}

// ------------------------------------------------------------------------------------
// ingest: what fills a capacity batch (host arrays, a frame, a frame with start poses, a sweep) and
// the one-call forms of the device ingests (include/dsr.h)
// ------------------------------------------------------------------------------------
// ---- the shared forms
// A refill is: the entry point's refusals; refill_begin; the kind packs its ingest block and says
// what every filled slot stages; refill_upload; the kind's kernels; refill_end.
static int refill_needs_capacity(dsr_batch* b, const char* who) {
  if (b->capacity) return 0;
  return fail(b->ctx, std::string("dsr_batch_") + who + " needs a batch from dsr_batch_create_capacity");
}

// the refusals of a device-filled kind, after its own argument errors
static int refill_fits(dsr_batch* b, const char* who, int n_det, int max_pts, int max_bg) {
  const std::string w(who);
  if (n_det > b->n_obj) return fail(b->ctx, w + ": n_det exceeds the batch's object capacity");
  if (max_pts > b->max_pts) return fail(b->ctx, w + ": max_pts exceeds the batch's max_pts");
  if ((long long)max_pts + max_bg > b->max_rays) return fail(b->ctx, w + ": max_pts + max_bg exceeds the batch's max_rays");
  return 0;
}

namespace {   // (internal linkage, as BatchDeleter: the library exports no symbol for these)
// what one filled slot stages: the counts (zero where the ingest kernels write them), the pose
// (null: the identity, as in an empty slot), the code (null: zeros) and pose_is_obj_cam
struct SlotFill {
  int n_pts = 0, n_rays = 0, n_fg = 0;
  const float* pose = nullptr;
  const float* code = nullptr;
  bool is_oc = false;
};

// The round trip of a one-call ingest (n_det > 0): the packed block and the caller's pts | rays |
// dobs (| t_in) go up, the entry point launches its kernels if upload() says so, the arrays and
// the records come back, and finish() synchronises the stream before the arena frees.  The first
// HIP error is the call's: -1 with its text.
struct IngestCall {
  dsr_ctx* ctx;
  hipStream_t s;
  float *pts, *rays, *dobs;                        // the caller's arrays
  size_t np, nr, nz;                               // their lengths
  DevArena mem;
  char* dev = nullptr;                             // the ingest block
  float* o = nullptr;                              // pts | rays | dobs | t_in on the device
  int rc = 0;
  IngestCall(dsr_ctx* c, int n_det, int max_pts, int max_bg, float* p, float* r, float* d)
      : ctx(c), s(c->stream), pts(p), rays(r), dobs(d), np((size_t)n_det * max_pts * 3),
        nr((size_t)n_det * ((size_t)max_pts + max_bg) * 3), nz((size_t)n_det * max_pts) {}
  float* d_pts() const { return o; }
  float* d_rays() const { return o + np; }
  float* d_dobs() const { return o + np + nr; }
  float* d_tin() const { return o + np + nr + nz; }
  bool chk(hipError_t e, const char* what) {
    if (e != hipSuccess && rc == 0) {
      ctx->err = std::string(what) + ": " + hipGetErrorString(e);
      rc = -1;
    }
    return e == hipSuccess;
  }
  void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    chk(hipMemcpyAsync(dst, src, bytes, kind, s), "hipMemcpyAsync");
  }
  // true: the kernels may run
  bool upload(const char* kind, const std::vector<char>& host, size_t all, const std::vector<float>& tin = {}) {
    if (!mem.alloc(&dev, all) || !mem.alloc(&o, np + nr + nz + tin.size())) {
      ctx->err = std::string("hipMalloc failed (") + kind + ")";
      rc = -1;
      return false;
    }
    // rows beyond a detection's counts come back as the caller had them
    copy(dev, host.data(), host.size(), hipMemcpyHostToDevice);
    copy(d_pts(), pts, sizeof(float) * np, hipMemcpyHostToDevice);
    copy(d_rays(), rays, sizeof(float) * nr, hipMemcpyHostToDevice);
    copy(d_dobs(), dobs, sizeof(float) * nz, hipMemcpyHostToDevice);
    if (!tin.empty()) copy(d_tin(), tin.data(), sizeof(float) * tin.size(), hipMemcpyHostToDevice);
    return rc == 0;
  }
  void download(const char* kernels) {
    chk(hipGetLastError(), kernels);
    copy(pts, d_pts(), sizeof(float) * np, hipMemcpyDeviceToHost);
    copy(rays, d_rays(), sizeof(float) * nr, hipMemcpyDeviceToHost);
    copy(dobs, d_dobs(), sizeof(float) * nz, hipMemcpyDeviceToHost);
  }
  void records(void* out, const void* recs, size_t bytes) { copy(out, recs, bytes, hipMemcpyDeviceToHost); }
  int finish() {
    if (o) chk(hipStreamSynchronize(s), "hipStreamSynchronize");
    return rc;
  }
};
}  // namespace

// Waits until the copies recorded in up_ev have left the owner's staging buffers and the pinned
// half of its ingest block g, then makes the block hold `up` uploaded bytes of `all` (0, 0: a fill
// without one).  Both halves only grow; the device block is replaced only once no kernel can still
// read it.  The owner is a batch (refill_begin) or a tracker (dsr_tracker_track_lidar,
// dsr_tracker_track_frame).
static int ingest_fit(dsr_ctx* ctx, dsr_batch::IngestBlock& g, hipEvent_t up_ev, size_t up, size_t all) {
  DSR_CHECK(ctx, hipEventSynchronize(up_ev));
  if (up > g.host_bytes) {
    if (g.host) hipHostFree(g.host);
    g.host = nullptr;
    g.host_bytes = 0;
    DSR_CHECK(ctx, hipHostMalloc(&g.host, up, hipHostMallocDefault));
    g.host_bytes = up;
  }
  if (all > g.dev_bytes) {
    // the kernels of an earlier ingest refill may still read the old block
    DSR_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (g.dev) hipFree(g.dev);
    g.dev = nullptr;
    g.dev_bytes = 0;
    DSR_CHECK(ctx, hipMalloc(&g.dev, all));
    g.dev_bytes = all;
  }
  return 0;
}

static int refill_begin(dsr_batch* b, size_t up, size_t all) {
  return ingest_fit(b->ctx, b->ingest, b->up_ev, up, all);
}

// Stages every slot (fill[0 .. n) and the empty rest), then uploads the first `stages` staging
// buffers — desc, t_in, z_in, is_oc, and for host arrays pts, rays, dobs — and `up` bytes of the
// ingest block, on the context stream: ordered after the previous run's work.
static int refill_upload(dsr_batch* b, const SlotFill* fill, int n, int stages, size_t up) {
  dsr_ctx* ctx = b->ctx;
  auto* desc = static_cast<ObjDesc*>(b->stage[0].host);
  auto* t_in = static_cast<float*>(b->stage[1].host);
  auto* z_in = static_cast<float*>(b->stage[2].host);
  auto* is_oc = static_cast<int*>(b->stage[3].host);
  for (int o = 0; o < b->n_obj; ++o) {
    const SlotFill x = o < n ? fill[o] : SlotFill{};
    ObjDesc d = b->hdesc[o];                       // the slot's offsets; the fill's counts
    d.n_pts = x.n_pts;
    d.n_rays = x.n_rays;
    d.n_fg = x.n_fg;
    desc[o] = d;
    float* t = t_in + (size_t)o * 16;
    for (int i = 0; i < 16; ++i) t[i] = x.pose ? x.pose[i] : (i % 5 == 0 ? 1.f : 0.f);
    float* z = z_in + (size_t)o * CODE;
    std::memset(z, 0, sizeof(float) * CODE);
    if (x.code) std::memcpy(z, x.code, sizeof(float) * b->dec->code_len);
    is_oc[o] = x.is_oc ? 1 : 0;
  }
  hipStream_t s = ctx->stream;
  for (int k = 0; k < stages; ++k)
    DSR_CHECK(ctx, hipMemcpyAsync(b->stage[k].dev, b->stage[k].host, b->stage[k].bytes, hipMemcpyHostToDevice, s));
  if (up) DSR_CHECK(ctx, hipMemcpyAsync(b->ingest.dev, b->ingest.host, up, hipMemcpyHostToDevice, s));
  return 0;
}

// The tail of every refill, after the kind's kernels: the one place that says what the batch holds.
static int refill_end(dsr_batch* b, const dsr_batch::Fill& fill) {
  dsr_ctx* ctx = b->ctx;
  hipStream_t s = ctx->stream;
  // lite flags of the previous fill's rays beyond the new counts are never read, but start clean
  if (b->refine) DSR_CHECK(ctx, hipMemsetAsync(b->refine, 0, (size_t)std::max(1, b->cand_total), s));
  DSR_CHECK(ctx, hipEventRecord(b->up_ev, s));
  b->n_active = fill.shape.n_det;
  b->last = fill;
  b->ran = false;
  return 0;
}

// The tail of the info entry points: the last fill's records out of the ingest block.
static int info_download(dsr_batch* b, void* out, const void* recs, size_t bytes) {
  dsr_ctx* ctx = b->ctx;
  if (!out) return fail(ctx, "null argument");
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  DSR_CHECK(ctx, hipEventSynchronize(b->up_ev));
  DSR_CHECK(ctx, hipMemcpy(out, recs, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// ---- host arrays
int dsr_batch_refill(dsr_batch* b, int n_obj, const dsr_object_in* in) {
  if (!b) return -2;
  dsr_ctx* ctx = b->ctx;
  if (int rc = refill_needs_capacity(b, "refill")) return rc;
  if (n_obj < 0 || n_obj > b->n_obj || (n_obj > 0 && !in))
    return fail(ctx, "refill: n_obj must be in [0, the batch's object capacity]");
  for (int o = 0; o < n_obj; ++o) {
    const dsr_object_in& x = in[o];
    if (x.n_pts < 0 || x.n_pts > b->max_pts || (x.n_pts > 0 && !x.pts))
      return fail(ctx, "refill: surface points exceed the batch capacity (or are null)");
    if (x.n_rays < 0 || x.n_rays > b->max_rays || (x.n_rays > 0 && !x.rays))
      return fail(ctx, "refill: rays exceed the batch capacity (or are null)");
    if (x.n_depth < 0 || x.n_depth > x.n_rays || (x.n_depth > 0 && !x.depth))
      return fail(ctx, "depth must hold at most n_rays foreground values");
  }
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  if (int rc = refill_begin(b, 0, 0)) return rc;
  auto* pts = static_cast<float*>(b->stage[4].host);
  auto* rays = static_cast<float*>(b->stage[5].host);
  auto* dobs = static_cast<float*>(b->stage[6].host);
  std::vector<SlotFill> fill(n_obj);
  for (int o = 0; o < n_obj; ++o) {
    const dsr_object_in& x = in[o];
    const ObjDesc& d = b->hdesc[o];
    fill[o] = SlotFill{x.n_pts, x.n_rays, x.n_depth, x.t_cam_obj, x.code, x.pose_is_obj_cam != 0};
    if (x.n_pts) std::memcpy(pts + (size_t)d.pts_off * 3, x.pts, sizeof(float) * 3 * x.n_pts);
    if (x.n_rays) std::memcpy(rays + (size_t)d.ray_off * 3, x.rays, sizeof(float) * 3 * x.n_rays);
    for (int r = 0; r < x.n_rays; ++r) dobs[d.ray_off + r] = r < x.n_depth ? x.depth[r] : 0.f;
  }
  if (int rc = refill_upload(b, fill.data(), n_obj, 7, 0)) return rc;
  return refill_end(b, {dsr_batch::Fill::OBJECTS, LidarShape{0, 3, 0, 0, n_obj}, 0});
}

// ---- frame (kernels and the host rule in dsr_frame.hpp)
int dsr_frame_params_default(dsr_frame_params* p) {
  if (!p) return -2;
  p->max_pts = 250;
  p->max_bg = 200;
  p->downsample = 4;
  p->expand = 5;
  p->min_mask_area = 1000;
  p->near = 0.01f;
  p->far = INFINITY;
  return 0;
}

static FrameCam frame_cam(const dsr_camera* cam) {
  return FrameCam{cam->fx, cam->fy, cam->cx, cam->cy, cam->width, cam->height};
}

int dsr_frame_inputs_host(const dsr_camera* cam, const dsr_frame_params* params, const float* depth,
                          const int* instance, int n_det, const dsr_frame_det* dets, float* pts, float* rays,
                          float* dobs, dsr_frame_det_out* out) {
  if (frame_args_error(cam, params, depth, instance, n_det, dets)) return -2;
  frame_inputs_host_impl(frame_cam(cam), *params, depth, instance, n_det, dets, pts, rays, dobs, out);
  return 0;
}

// the uploaded part of a frame block: depth | instance | detections, laid out as frame_carve does
static void frame_pack(void* host, const dsr_camera* cam, const float* depth, const int* inst, int n_det,
                       const dsr_frame_det* dets, const int* modes = nullptr) {
  const FrameDev H = frame_carve(host, cam->width, cam->height, n_det);
  const size_t px = (size_t)cam->width * cam->height;
  std::memcpy(H.depth, depth, px * sizeof(float));
  std::memcpy(H.inst, inst, px * sizeof(int));
  for (int d = 0; d < n_det; ++d) {
    H.dets[d].label = dets[d].label;
    for (int k = 0; k < 4; ++k) H.dets[d].bbox[k] = dets[d].bbox[k];
    H.dets[d].mode = modes ? modes[d] : DSR_FRAME_POSE_GIVEN;
  }
}

// dsr_frame_inputs (pose_params == null) and dsr_frame_poses: the latter adds k_frame_pose /
// k_frame_compact, and the given poses travel in a t_in array
static int frame_call(dsr_ctx* ctx, const dsr_camera* cam, const dsr_frame_params* params,
                      const dsr_frame_pose_params* pose_params, const float* depth, const int* instance, int n_det,
                      const dsr_frame_det* dets, const int* modes, float* pts, float* rays, float* dobs,
                      dsr_frame_det_out* out, dsr_frame_pose_out* pose_out) {
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  const int W = cam->width, H = cam->height;
  const size_t all = frame_dev_bytes(W, H, n_det) + (pose_params ? frame_pose_dev_bytes(n_det, params->max_pts) : 0);
  std::vector<char> host(frame_upload_bytes(W, H, n_det));
  frame_pack(host.data(), cam, depth, instance, n_det, dets, modes);
  std::vector<float> tin;
  if (pose_params)
    for (int d = 0; d < n_det; ++d) tin.insert(tin.end(), dets[d].t_cam_obj, dets[d].t_cam_obj + 16);
  IngestCall c(ctx, n_det, params->max_pts, params->max_bg, pts, rays, dobs);
  if (c.upload("frame", host, all, tin)) {
    const FrameDev D = frame_carve(c.dev, W, H, n_det);
    const FramePoseDev E = pose_params ? frame_pose_carve(c.dev, W, H, n_det, params->max_pts) : FramePoseDev{};
    frame_launch(c.s, frame_cam(cam), *params, n_det, D, nullptr, c.d_pts(), c.d_rays(), c.d_dobs());
    if (pose_params)
      frame_pose_launch(c.s, *params, *pose_params, n_det, D, E, nullptr, c.d_pts(), c.d_rays(), c.d_dobs(), c.d_tin());
    c.download("frame kernels");
    c.records(out, D.recs, sizeof(dsr_frame_det_out) * n_det);
    if (pose_params) c.records(pose_out, E.precs, sizeof(dsr_frame_pose_out) * n_det);
  }
  return c.finish();
}

int dsr_frame_inputs(dsr_ctx* ctx, const dsr_camera* cam, const dsr_frame_params* params, const float* depth,
                     const int* instance, int n_det, const dsr_frame_det* dets, float* pts, float* rays,
                     float* dobs, dsr_frame_det_out* out) {
  if (!ctx) return -2;
  if (const char* m = frame_args_error(cam, params, depth, instance, n_det, dets)) return fail(ctx, m);
  if (n_det > 0 && (!pts || !rays || !dobs || !out)) return fail(ctx, "frame: null output arrays");
  if (n_det == 0) return 0;
  return frame_call(ctx, cam, params, nullptr, depth, instance, n_det, dets, nullptr, pts, rays, dobs, out, nullptr);
}

// dsr_batch_refill_frame (pose_params == null) and dsr_batch_refill_frame_poses
static int batch_refill_frame_impl(dsr_batch* b, const dsr_camera* cam, const dsr_frame_params* params,
                                   const dsr_frame_pose_params* pose_params, const float* depth,
                                   const int* instance, int n_det, const dsr_frame_det* dets, const int* modes) {
  if (!b) return -2;
  dsr_ctx* ctx = b->ctx;
  if (int rc = refill_needs_capacity(b, "refill_frame")) return rc;
  if (const char* m = frame_args_error(cam, params, depth, instance, n_det, dets)) return fail(ctx, m);
  if (pose_params)
    if (const char* m = frame_pose_args_error(pose_params, n_det, modes)) return fail(ctx, m);
  if (int rc = refill_fits(b, "refill_frame", n_det, params->max_pts, params->max_bg)) return rc;
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  const int W = cam->width, H = cam->height;
  const size_t up = frame_upload_bytes(W, H, n_det),
               all = frame_dev_bytes(W, H, n_det) + (pose_params ? frame_pose_dev_bytes(n_det, params->max_pts) : 0);
  if (int rc = refill_begin(b, up, all)) return rc;
  frame_pack(b->ingest.host, cam, depth, instance, n_det, dets, pose_params ? modes : nullptr);
  std::vector<SlotFill> fill(n_det);                // k_frame_scan writes the counts
  for (int o = 0; o < n_det; ++o) {
    // a cuboid detection's pose row is written by k_frame_pose after this upload (t_cam_obj)
    const bool given = !(pose_params && modes[o] != DSR_FRAME_POSE_GIVEN);
    fill[o].pose = given ? dets[o].t_cam_obj : nullptr;
    fill[o].code = dets[o].code;
    fill[o].is_oc = given && dets[o].pose_is_obj_cam;
  }
  if (int rc = refill_upload(b, fill.data(), n_det, 4, up)) return rc;   // (pts / rays / dobs: the kernels)
  if (n_det > 0) {
    const FrameDev D = frame_carve(b->ingest.dev, W, H, n_det);
    frame_launch(ctx->stream, frame_cam(cam), *params, n_det, D, b->desc, b->pts, b->rays, b->dobs);
    if (pose_params)
      frame_pose_launch(ctx->stream, *params, *pose_params, n_det, D,
                        frame_pose_carve(b->ingest.dev, W, H, n_det, params->max_pts), b->desc, b->pts, b->rays,
                        b->dobs, b->t_in);
    DSR_CHECK(ctx, hipGetLastError());
  }
  return refill_end(b, {pose_params ? dsr_batch::Fill::FRAME_POSES : dsr_batch::Fill::FRAME,
                        LidarShape{0, 3, W, H, n_det}, params->max_pts});
}

int dsr_batch_refill_frame(dsr_batch* b, const dsr_camera* cam, const dsr_frame_params* params,
                           const float* depth, const int* instance, int n_det, const dsr_frame_det* dets) {
  return batch_refill_frame_impl(b, cam, params, nullptr, depth, instance, n_det, dets, nullptr);
}

int dsr_batch_frame_info(dsr_batch* b, dsr_frame_det_out* out) {
  if (!b) return -2;
  const dsr_batch::Fill& f = b->last;
  if (f.kind != dsr_batch::Fill::FRAME && f.kind != dsr_batch::Fill::FRAME_POSES)
    return fail(b->ctx, "dsr_batch_frame_info: the batch's last fill was not a frame (dsr_batch_refill_frame)");
  if (f.shape.n_det == 0) return 0;
  const FrameDev D = frame_carve(b->ingest.dev, f.shape.W, f.shape.H, f.shape.n_det);
  return info_download(b, out, D.recs, sizeof(dsr_frame_det_out) * f.shape.n_det);
}

// ---- frame with start poses
int dsr_frame_pose_params_default(dsr_frame_pose_params* p) {
  if (!p) return -2;
  p->outlier_radius = 1.0f;
  p->lo_pct = 5;
  p->hi_pct = 95;
  p->box_margin = 1.2f;
  p->scale_factor = 0.40f;
  p->min_points = 50;
  p->up[0] = 0.f;
  p->up[1] = -1.f;
  p->up[2] = 0.f;
  return 0;
}

int dsr_frame_poses_host(const dsr_camera* cam, const dsr_frame_params* params,
                         const dsr_frame_pose_params* pose_params, const float* depth, const int* instance,
                         int n_det, const dsr_frame_det* dets, const int* modes, float* pts, float* rays,
                         float* dobs, dsr_frame_det_out* out, dsr_frame_pose_out* pose_out) {
  if (frame_args_error(cam, params, depth, instance, n_det, dets)) return -2;
  if (frame_pose_args_error(pose_params, n_det, modes)) return -2;
  if (n_det > 0 && (!pts || !rays || !dobs || !out || !pose_out)) return -2;
  frame_poses_host_impl(frame_cam(cam), *params, *pose_params, depth, instance, n_det, dets, modes, pts, rays, dobs,
                        out, pose_out);
  return 0;
}

int dsr_frame_poses(dsr_ctx* ctx, const dsr_camera* cam, const dsr_frame_params* params,
                    const dsr_frame_pose_params* pose_params, const float* depth, const int* instance,
                    int n_det, const dsr_frame_det* dets, const int* modes, float* pts, float* rays,
                    float* dobs, dsr_frame_det_out* out, dsr_frame_pose_out* pose_out) {
  if (!ctx) return -2;
  if (const char* m = frame_args_error(cam, params, depth, instance, n_det, dets)) return fail(ctx, m);
  if (const char* m = frame_pose_args_error(pose_params, n_det, modes)) return fail(ctx, m);
  if (n_det > 0 && (!pts || !rays || !dobs || !out || !pose_out)) return fail(ctx, "frame: null output arrays");
  if (n_det == 0) return 0;
  return frame_call(ctx, cam, params, pose_params, depth, instance, n_det, dets, modes, pts, rays, dobs, out, pose_out);
}

int dsr_batch_refill_frame_poses(dsr_batch* b, const dsr_camera* cam, const dsr_frame_params* params,
                                 const dsr_frame_pose_params* pose_params, const float* depth,
                                 const int* instance, int n_det, const dsr_frame_det* dets, const int* modes) {
  if (!b) return -2;
  if (!pose_params) return fail(b->ctx, "frame poses: null pose parameters");
  return batch_refill_frame_impl(b, cam, params, pose_params, depth, instance, n_det, dets, modes);
}

int dsr_batch_frame_pose_info(dsr_batch* b, dsr_frame_pose_out* out) {
  if (!b) return -2;
  const dsr_batch::Fill& f = b->last;
  if (f.kind != dsr_batch::Fill::FRAME_POSES)
    return fail(b->ctx, "dsr_batch_frame_pose_info: the batch's last fill was not a frame with poses (dsr_batch_refill_frame_poses)");
  if (f.shape.n_det == 0) return 0;
  const FramePoseDev E = frame_pose_carve(b->ingest.dev, f.shape.W, f.shape.H, f.shape.n_det, f.max_pts);
  return info_download(b, out, E.precs, sizeof(dsr_frame_pose_out) * f.shape.n_det);
}

// ---- LiDAR sweep (kernels and the host rule in dsr_lidar.hpp)
int dsr_lidar_params_default(dsr_lidar_params* p) {
  if (!p) return -2;
  p->max_pts = 250;
  p->max_bg = 200;
  p->downsample = 4;
  p->expand = 5;
  p->min_mask_area = 1000;
  p->radius = 3.0f;
  p->box_margin = 1.1f;
  return 0;
}

// t_cam_velo is validated as dsr_reconstruct_views validates t_view_ref
static bool lidar_rigid(const float* t) {
  float inv[16];
  return t && rigid_inverse(t, inv);
}

static LidarShape lidar_shape(const dsr_camera* cam, int n_velo, int stride, int n_det) {
  return LidarShape{n_velo, stride, cam->width, cam->height, n_det};
}

int dsr_lidar_inputs_host(const dsr_camera* cam, const dsr_lidar_params* params, const float* t_cam_velo,
                          const float* velo, int n_velo, int stride, const int* instance, int n_masks,
                          const dsr_lidar_mask* masks, int n_det, const dsr_lidar_det* dets, float* pts,
                          float* rays, float* dobs, dsr_lidar_det_out* out) {
  if (lidar_args_error(cam, params, lidar_rigid(t_cam_velo), velo, n_velo, stride, instance, n_masks, masks, n_det, dets))
    return -2;
  lidar_inputs_host_impl(frame_cam(cam), *params, t_cam_velo, velo, n_velo, stride, instance, n_masks, masks, n_det,
                         dets, pts, rays, dobs, out);
  return 0;
}

int dsr_lidar_inputs(dsr_ctx* ctx, const dsr_camera* cam, const dsr_lidar_params* params,
                     const float* t_cam_velo, const float* velo, int n_velo, int stride, const int* instance,
                     int n_masks, const dsr_lidar_mask* masks, int n_det, const dsr_lidar_det* dets, float* pts,
                     float* rays, float* dobs, dsr_lidar_det_out* out) {
  if (!ctx) return -2;
  if (const char* m = lidar_args_error(cam, params, lidar_rigid(t_cam_velo), velo, n_velo, stride, instance, n_masks,
                                       masks, n_det, dets))
    return fail(ctx, m);
  if (n_det > 0 && (!pts || !rays || !dobs || !out)) return fail(ctx, "lidar: null output arrays");
  if (n_det == 0) return 0;
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  const LidarShape S = lidar_shape(cam, n_velo, stride, n_det);
  std::vector<char> host(lidar_upload_bytes(S));
  lidar_pack(host.data(), S, *params, t_cam_velo, velo, instance, n_masks, masks, dets);
  IngestCall c(ctx, n_det, params->max_pts, params->max_bg, pts, rays, dobs);
  if (c.upload("lidar", host, lidar_dev_bytes(S))) {
    const LidarDev D = lidar_carve(c.dev, S);
    lidar_launch(c.s, frame_cam(cam), *params, lidar_xf(t_cam_velo), S, n_masks, D, nullptr, c.d_pts(), c.d_rays(),
                 c.d_dobs());
    c.download("lidar kernels");
    c.records(out, D.recs, sizeof(dsr_lidar_det_out) * n_det);
  }
  return c.finish();
}

int dsr_batch_refill_lidar(dsr_batch* b, const dsr_camera* cam, const dsr_lidar_params* params,
                           const float* t_cam_velo, const float* velo, int n_velo, int stride,
                           const int* instance, int n_masks, const dsr_lidar_mask* masks, int n_det,
                           const dsr_lidar_det* dets) {
  if (!b) return -2;
  dsr_ctx* ctx = b->ctx;
  if (int rc = refill_needs_capacity(b, "refill_lidar")) return rc;
  if (const char* m = lidar_args_error(cam, params, lidar_rigid(t_cam_velo), velo, n_velo, stride, instance, n_masks,
                                       masks, n_det, dets))
    return fail(ctx, m);
  if (int rc = refill_fits(b, "refill_lidar", n_det, params->max_pts, params->max_bg)) return rc;
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  const LidarShape S = lidar_shape(cam, n_velo, stride, n_det);
  const size_t up = lidar_upload_bytes(S);
  if (int rc = refill_begin(b, up, lidar_dev_bytes(S))) return rc;
  lidar_pack(b->ingest.host, S, *params, t_cam_velo, velo, instance, n_masks, masks, dets);
  const LidarDev Hd = lidar_carve(b->ingest.host, S);
  std::vector<SlotFill> fill(n_det);                // k_lidar_bg_scan writes the counts
  for (int o = 0; o < n_det; ++o) {
    fill[o].pose = Hd.dets[o].tco;
    fill[o].code = dets[o].code;
  }
  if (int rc = refill_upload(b, fill.data(), n_det, 4, up)) return rc;   // (pts / rays / dobs: the kernels)
  if (n_det > 0) {
    lidar_launch(ctx->stream, frame_cam(cam), *params, lidar_xf(t_cam_velo), S, n_masks, lidar_carve(b->ingest.dev, S),
                 b->desc, b->pts, b->rays, b->dobs);
    DSR_CHECK(ctx, hipGetLastError());
  }
  return refill_end(b, {dsr_batch::Fill::SWEEP, S, 0});
}

int dsr_batch_lidar_info(dsr_batch* b, dsr_lidar_det_out* out) {
  if (!b) return -2;
  const dsr_batch::Fill& f = b->last;
  if (f.kind != dsr_batch::Fill::SWEEP)
    return fail(b->ctx, "dsr_batch_lidar_info: the batch's last fill was not a sweep (dsr_batch_refill_lidar)");
  if (f.shape.n_det == 0) return 0;
  return info_download(b, out, lidar_carve(b->ingest.dev, f.shape).recs, sizeof(dsr_lidar_det_out) * f.shape.n_det);
}

static int batch_enqueue_iters(dsr_batch* b, bool timing, int it0, int it1) {
  dsr_ctx* ctx = b->ctx;
  hipStream_t s0 = ctx->stream;
  const int n = b->n_obj;
  const DevDecoder& D = b->dec->D;
  const GNParams P = b->P;
  const int grid = ctx->n_cu;
  const int cb = (n + 63) / 64;
  const int fv = fwd_variant();
  const FwdChoice fwdc = fwd_kernel_for(D, fv);
  const JacChoice jacc = jac_kernel_for(D);
  const FwdKernel fwdk = fwdc.kernel;
  const JacKernel jack = jacc.kernel;
  const LiteSchedule& lites = lite_schedule();
  const LiteKernel litek = lites.kernel;
  // (the kernels dispatched, as dsr_batch_stats reports them: fwd_kernel / jac_kernel's choice)
  b->ran_fwd = fwdc.number;
  b->ran_jac = jacc.number;
  b->ran_lite = b->lite ? lites.number : 0;
  b->ran_ring = fwdc.ring;
  const int np = (int)b->passes.size() - 1;
  const size_t epi = ev_per_iter(b);
  const int G = (int)b->groups.size();
  DSR_CHECK(ctx, hipEventRecord(b->fork_ev, s0));
  for (int g = 1; g < G; ++g) DSR_CHECK(ctx, hipStreamWaitEvent(ctx->gstream[g], b->fork_ev, 0));
  for (int it = it0; it < it1; ++it) {
    for (int g = 0; g < G; ++g) {             // groups interleaved, one stream each
      const dsr_batch::Group& gr = b->groups[g];
      hipStream_t s = ctx->gstream[g];
      const int ng = gr.n, o0 = gr.o0;
      const ObjDesc* desc = b->desc + o0;
      ObjState* st = b->st + o0;
      float* zbuf = b->zbuf + (size_t)o0 * CODE;
      float* b0 = b->bias0f + (size_t)o0 * HID;
      float* b4 = b->bias4f + (size_t)o0 * HID;
      hipEvent_t* ev = b->ev.data() + 2 + ((size_t)it * G + g) * epi;
      hipLaunchKernelGGL(k_iter_begin, dim3(ng), dim3(512), 0, s, ng, desc, st, zbuf, D, P, b0, b4, b->dobs);
      ErtArgs ert = b->lite_cfg;
      ert.dead = b->dead;
      ert.M = b->M;
      ert.nth = -P.cut_off;
      ert.st = b->lite ? st : nullptr;
      ert.refine = b->refine;
      ert.diag = b->diag;
      const bool chunked = b->prescan && gr.n_rch > 0;
      if (!chunked)                              // (the chunked first pass fills its own rows)
        DSR_CHECK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b->dense + gr.c0), 0x7fc00000,
                                         (size_t)(gr.c1 - gr.c0), s));   // out-of-ball samples: NaN
      for (int pz = 0; pz < np; ++pz) {          // render passes with early ray termination
        const int ra = b->passes[pz], rb = b->passes[pz + 1];
        const int wz = P.n_win ? pz : -1;        // the objects' own windows for this pass, or [ra, rb)
        if (chunked) {                           // count (the first pass: the ray scan), then emit
          if (pz == 0)
            hipLaunchKernelGGL(k_sample_scan, dim3(gr.n_rch), dim3(RENDER_RAYS), 0, s, gr.rchunks, desc, st, b->rays,
                               b->M, rb, wz, b->dead, b->rinfo, b->rwin, gr.scnt, b->dense);
          else
            hipLaunchKernelGGL(k_sample_count, dim3(gr.n_rch), dim3(RENDER_RAYS), 0, s, gr.rchunks, desc, st, b->rays,
                               b->M, ra, rb, wz, b->dead, b->rinfo, b->rwin, gr.scnt);
          // (+1 workgroup: the pass's tile table, from the count kernel's chunk counts)
          hipLaunchKernelGGL(k_sample_emit, dim3(gr.n_rch + 1), dim3(RENDER_RAYS), 0, s, gr.rchunks, desc, st,
                             b->rays, b->M, ra, rb, wz, b->cand, b->rwin, gr.scnt,
                             ChunkTiles{gr.och, gr.tiles_f, gr.nt_f, ng, b->lite ? LTILE : TILE, 0});
        } else {
          hipLaunchKernelGGL(k_sample_pass, dim3(ng), dim3(SAMPLE_THREADS), 0, s, ng, desc, st, b->rays, b->M,
                             ra, rb, wz, b->cand, b->dead, b->rinfo);
          hipLaunchKernelGGL(k_tiles_fwd, dim3(1), dim3(1024), 0, s, ng, desc, st, gr.tiles_f, gr.nt_f,
                             b->lite ? LTILE : TILE, 0);
        }
        if (fv & 1) DSR_CHECK(ctx, hipMemsetAsync(gr.sync, 0, 8 * 32 * sizeof(unsigned), s));
        if (timing) DSR_CHECK(ctx, hipEventRecord(ev[2 * pz], s));
        if (b->lite)
          hipLaunchKernelGGL(litek, dim3(grid), dim3(512), 0, s, D, gr.tiles_f, gr.nt_f, desc,
                             b->cand, b0, b4, b->dense, ert);
        else
          hipLaunchKernelGGL(fwdk, dim3(grid), dim3(512), 0, s, D, gr.tiles_f, gr.nt_f, desc, b->cand,
                             b0, b4, b->dense, gr.sync, ert, MaskArgs{nullptr, nullptr, nullptr, nullptr});
        if (timing) DSR_CHECK(ctx, hipEventRecord(ev[2 * pz + 1], s));
      }
      const bool rays = gr.n_rch > 0;            // (a group of ray-less objects: all failed, loss.py:86-88)
      if (b->lite) {                             // exact split-fp16 decode of the band samples
        if (rays) {
          hipLaunchKernelGGL(k_refine_scan, dim3(gr.n_rch), dim3(REFINE_SCAN_THREADS), 0, s, gr.rchunks, desc, st, b->M,
                             b->refine, b->dense, refine_all() ? 1 : 0, -P.cut_off, b->rbits, b->abits, gr.ccnt,
                             b->ma.slotmap, P.n_win);
          const int wp = (b->ma.pts && fv == 12) ? 1 : 0;   // (chunked: +1 workgroup, the exact pass's tiles)
          hipLaunchKernelGGL(k_refine_emit, dim3(gr.n_rch + (chunked ? 1 : 0)), dim3(RENDER_RAYS), 0, s, gr.rchunks,
                             desc, st, b->rays, b->M, b->cand, b->ma.slotmap, b->rbits, b->abits, gr.ccnt,
                             chunked ? ChunkTiles{gr.och, gr.tiles_f, gr.nt_f, ng, TILE, wp} : ChunkTiles{});
        }
        if (!chunked)
          hipLaunchKernelGGL(k_tiles_fwd, dim3(1), dim3(1024), 0, s, ng, desc, st, gr.tiles_f, gr.nt_f, TILE,
                             (b->ma.pts && fv == 12) ? 1 : 0);
        if (timing) DSR_CHECK(ctx, hipEventRecord(ev[2 * np], s));
        const ErtArgs ex{nullptr, b->M, -P.cut_off, st, nullptr};
        if (b->ma.msk && fv == 12)               // keep masks + sdf for the Jacobian's render points
          hipLaunchKernelGGL(fwd16_kernel<512>(), dim3(grid), dim3(512), 0, s, D, gr.tiles_f, gr.nt_f, desc,
                             b->cand, b0, b4, b->dense, gr.sync, ex, b->ma);
        else
          hipLaunchKernelGGL(fwdk, dim3(grid), dim3(512), 0, s, D, gr.tiles_f, gr.nt_f, desc, b->cand,
                             b0, b4, b->dense, gr.sync, ex, MaskArgs{nullptr, nullptr, nullptr, nullptr});
        if (timing) DSR_CHECK(ctx, hipEventRecord(ev[2 * np + 1], s));
      }
      const bool keep = b->lite && b->ma.msk && fv == 12;
      const int je = 2 * (np + (b->lite ? 1 : 0));
      if (rays) {
        hipLaunchKernelGGL(k_render_rays, dim3(gr.n_rch), dim3(RENDER_RAYS), render_lds_bytes(b->M), s,
                           gr.rchunks, desc, st, b->rays, b->dobs, P, b->dense, b->kst, b->rst,
                           keep ? b->sst : nullptr, (const int*)b->ma.slotmap, gr.ccnt);
        // (chunked: +1 workgroup, the Jacobian's tiles from the render chunks' counts)
        hipLaunchKernelGGL(k_render_gather, dim3(gr.n_rch + (chunked ? 1 : 0)), dim3(256), 0, s, gr.rchunks, desc,
                           st, gr.ccnt, b->M, b->kst, b->rst, b->sst, b->kpts, b->kres, keep ? b->kslot : nullptr,
                           chunked ? ChunkTiles{gr.och, gr.tiles_j, gr.nt_j, ng, TILE, 0} : ChunkTiles{});
      }
      if (!chunked)
        hipLaunchKernelGGL(k_tiles_jac, dim3(1), dim3(1024), 0, s, ng, desc, st, gr.tiles_j, gr.nt_j);
      if (timing) DSR_CHECK(ctx, hipEventRecord(ev[je], s));
      hipLaunchKernelGGL(jack, dim3(grid), dim3(512), 0, s, D, gr.tiles_j, gr.nt_j, desc, st,
                         b->pts, b->kpts, b->kres, b0, b4, P, b->slots,
                         (const float4*)nullptr, (float*)nullptr, (float*)nullptr,
                         keep ? b->ma : MaskArgs{nullptr, nullptr, nullptr, nullptr},
                         D.ln_mask ? ctx->lnws[g] : (float*)nullptr);
      if (timing) DSR_CHECK(ctx, hipEventRecord(ev[je + 1], s));
      float* sred = b->sred + (size_t)o0 * SRED_STRIDE;
      hipLaunchKernelGGL(k_reduce_slots, dim3(ng * SLOT_BLOCKS), dim3(256), 0, s, desc, st, b->slots, sred, it,
                         b->counts + (size_t)o0 * COUNT_STRIDE, n);
      if (b->n_tied) {                           // one solve per tied object, then its views' poses
        hipLaunchKernelGGL(k_solve_views, dim3(gr.nt), dim3(SOLVE_THREADS), 0, s, (const int2*)b->tie + gr.t0, desc,
                           st, zbuf, P, sred, b->tr_H ? b->tr_H + (size_t)o0 * TRACE_H_STRIDE : nullptr,
                           b->tr_v ? b->tr_v + (size_t)o0 * TRACE_V_STRIDE : nullptr,
                           b->tr_i ? b->tr_i + (size_t)o0 * TRACE_I_STRIDE : nullptr, n, b->fail_view + gr.t0);
        if (b->tie_multi)
          hipLaunchKernelGGL(k_views_pose, dim3(gr.nt), dim3(64), 0, s, (const int2*)b->tie + gr.t0, st,
                             (const float*)b->cview + (size_t)o0 * 16);
        continue;
      }
      hipLaunchKernelGGL(k_solve, dim3(ng), dim3(SOLVE_THREADS), 0, s, ng, desc, st, zbuf, P, sred,
                         b->tr_H ? b->tr_H + (size_t)o0 * TRACE_H_STRIDE : nullptr,
                         b->tr_v ? b->tr_v + (size_t)o0 * TRACE_V_STRIDE : nullptr,
                         b->tr_i ? b->tr_i + (size_t)o0 * TRACE_I_STRIDE : nullptr, n);
    }
  }
  for (int g = 1; g < G; ++g) {
    DSR_CHECK(ctx, hipEventRecord(b->join_ev[g], ctx->gstream[g]));
    DSR_CHECK(ctx, hipStreamWaitEvent(s0, b->join_ev[g], 0));
  }
  hipLaunchKernelGGL(k_finalize, dim3(cb), dim3(64), 0, s0, n, b->st, b->zbuf, b->out);
  DSR_CHECK(ctx, hipGetLastError());
  if (timing) DSR_CHECK(ctx, hipEventRecord(b->ev[1], s0));
  return 0;
}

static int batch_enqueue(dsr_batch* b, bool timing = true) {
  dsr_ctx* ctx = b->ctx;
  const int n = b->n_obj;
  if (timing) DSR_CHECK(ctx, hipEventRecord(b->ev[0], ctx->stream));
  hipLaunchKernelGGL(k_init_state, dim3(n), dim3(64), 0, ctx->stream, n, b->t_in, b->is_oc, b->z_in, b->st,
                     b->zbuf, b->iters, win_table(b->passes));
  DSR_CHECK(ctx, hipMemsetAsync(b->diag, 0, sizeof(int) * STD_INTS, ctx->stream));
  if (b->n_tied) DSR_CHECK(ctx, hipMemsetAsync(b->fail_view, 0xff, sizeof(int) * b->n_tied, ctx->stream));
  if (b->tie_multi)               // the views' start poses from their leaders' (before the groups fork)
    for (const auto& gr : b->groups)
      hipLaunchKernelGGL(k_views_pose, dim3(gr.nt), dim3(64), 0, ctx->stream, (const int2*)b->tie + gr.t0,
                         b->st + gr.o0, (const float*)b->cview + (size_t)gr.o0 * 16);
  b->spare_run = false;
  return batch_enqueue_iters(b, timing, 0, b->iters);
}

// The spare iteration (lite + audit): only objects whose iteration an audit discarded
// (k_solve) are still running after the regular iterations.  It is enqueued on demand once
// the regular iterations have finished (batch_finish, dsr_batch_query), so a run without
// violations launches nothing extra; graphs capture the regular iterations only.
// Returns 1 if the spare iteration was enqueued now, 0 if there is nothing to redo.
static int batch_redo(dsr_batch* b) {
  dsr_ctx* ctx = b->ctx;
  if (b->loop_iters <= b->iters || b->spare_run) return 0;
  std::vector<ObjState> hs(b->n_obj);
  DSR_CHECK(ctx, hipMemcpy(hs.data(), b->st, sizeof(ObjState) * hs.size(), hipMemcpyDeviceToHost));
  bool any = false;
  for (const ObjState& o : hs) any = any || (o.status == ST_RUNNING && o.lite_redo);
  if (!any) return 0;
  b->spare_run = true;
  const int rc = batch_enqueue_iters(b, b->timed, b->iters, b->loop_iters);
  if (rc) return rc;
  DSR_CHECK(ctx, hipEventRecord(b->done_ev, ctx->stream));
  return 1;
}
static int batch_finish(dsr_batch* b) {
  dsr_ctx* ctx = b->ctx;
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  DSR_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const int rc = batch_redo(b);
  if (rc < 0) return rc;
  if (rc == 1) DSR_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

// dsr_batch_run: with DSR_GRAPH=1 the first run of a batch is enqueued eagerly and from
// the second on (a re-run batch: streaming keyframes, config 5) the whole launch sequence —
// ~6 + 3 x passes launches per iteration and object group; one group by default under
// DSR_GRAPH=1 (batch_create_impl) — is captured once into a hipGraph and replayed with one
// launch; dsr_batch_graph captures up front.  A
// replayed run records only its total time (kernel events stay out of the graph: HIP
// cannot time events recorded inside one), so dsr_batch_stats reports no kernel times.
static long graph_key() { return ((long)fwd_variant() * 100000 + jac_variant()) * 10 + split_ring(); }

static int batch_capture(dsr_batch* b) {
  dsr_ctx* ctx = b->ctx;
  if (b->graph) {
    hipGraphExecDestroy(b->graph);
    b->graph = nullptr;
  }
  hipGraph_t g = nullptr;
  DSR_CHECK(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  const int rc = batch_enqueue(b, false);      // kernel timing events stay out of the graph
  const hipError_t ec = hipStreamEndCapture(ctx->stream, &g);
  if (rc) {
    if (g) hipGraphDestroy(g);
    return rc;
  }
  DSR_CHECK(ctx, ec);
  const hipError_t ei = hipGraphInstantiate(&b->graph, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  DSR_CHECK(ctx, ei);
  b->graph_key = graph_key();
  ++b->captures;
  return 0;
}

static int batch_launch(dsr_batch* b) {
  dsr_ctx* ctx = b->ctx;
  if (b->capacity && b->n_active == 0) return fail(ctx, "capacity batch holds no objects (dsr_batch_refill)");
  // a DSR_BATCH_GRAPH capacity batch replays from its first run (its refills keep every kernel
  // argument); other batches under DSR_GRAPH=1 run eagerly once, then replay
  const bool first_eager = !b->cap_graph;
  if (!(graph_enabled() || b->cap_graph) || (b->runs++ == 0 && first_eager)) {
    const int rc = batch_enqueue(b);
    if (rc) return rc;
    b->ran = true;
    b->timed = true;
    return 0;
  }
  if (!b->graph || b->graph_key != graph_key()) {
    const int rc = batch_capture(b);
    if (rc) return rc;
  }
  DSR_CHECK(ctx, hipEventRecord(b->ev[0], ctx->stream));
  // poison the out-records first: a replay's k_finalize (inside the graph) rewrites every one,
  // so a download that ever saw these bytes would expose work ordered wrongly around the graph
  // launch (test_graph_replays_never_return_stale_records) instead of returning stale results
  DSR_CHECK(ctx, hipMemsetAsync(b->out, 0xff, sizeof(dsr_object_out) * b->n_obj, ctx->stream));
  DSR_CHECK(ctx, hipGraphLaunch(b->graph, ctx->stream));
  DSR_CHECK(ctx, hipEventRecord(b->ev[1], ctx->stream));
  ++b->replays;
  b->spare_run = false;          // a replay runs the regular iterations only (batch_finish)
  b->ran = true;
  b->timed = false;
  return 0;
}

int dsr_batch_graph(dsr_batch* b) {
  if (!b) return -2;
  std::lock_guard<std::recursive_mutex> run(b->ctx->run_mu);
  hipSetDevice(b->ctx->device);
  if (!graph_enabled() && !b->cap_graph) return 0;
  b->runs = std::max(b->runs, 1);
  return batch_capture(b);
}

int dsr_batch_run(dsr_batch* b) {
  if (!b) return -2;
  dsr_ctx* ctx = b->ctx;
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  const int rc = batch_launch(b);
  if (rc) return rc;
  DSR_CHECK(ctx, hipEventRecord(b->done_ev, ctx->stream));
  return 0;
}

int dsr_batch_query(dsr_batch* b) {
  if (!b) return -2;
  if (!b->ran) return fail(b->ctx, "batch has not run");
  std::lock_guard<std::recursive_mutex> run(b->ctx->run_mu);
  hipSetDevice(b->ctx->device);
  const hipError_t e = hipEventQuery(b->done_ev);
  if (e == hipSuccess) {
    // a pending audit redo is enqueued here and the batch reported as still in flight: the
    // caller's next query sees it finish (never blocks for a GN iteration)
    const int rc = batch_redo(b);
    return rc < 0 ? rc : (rc == 1 ? 0 : 1);
  }
  if (e == hipErrorNotReady) return 0;
  return fail(b->ctx, std::string("hipEventQuery: ") + hipGetErrorString(e));
}

int dsr_batch_sync(dsr_batch* b) {
  if (!b) return -2;
  hipSetDevice(b->ctx->device);
  return b->ran ? batch_finish(b) : 0;
}

int dsr_batch_download(dsr_batch* b, dsr_object_out* out) {
  if (!b || !out) return -2;
  hipSetDevice(b->ctx->device);
  if (b->ran) {
    const int rc = batch_finish(b);
    if (rc) return rc;
  }
  DSR_CHECK(b->ctx, hipMemcpyAsync(out, b->out, sizeof(dsr_object_out) * b->n_active, hipMemcpyDeviceToHost,
                                   b->ctx->stream));
  DSR_CHECK(b->ctx, hipStreamSynchronize(b->ctx->stream));
  return 0;
}

int dsr_batch_stats(dsr_batch* b, dsr_stats* st) {
  if (!b || !st) return -2;
  if (!b->ran) return fail(b->ctx, "batch has not run");
  hipSetDevice(b->ctx->device);
  {
    const int rc = batch_finish(b);
    if (rc) return rc;
  }
  *st = dsr_stats{};
  float ms = 0.f;
  const int np = (int)b->passes.size() - 1;
  const size_t epi = ev_per_iter(b);
  const int G = (int)b->groups.size();
  std::vector<ObjState> hs(b->n_obj);
  DSR_CHECK(b->ctx, hipMemcpy(hs.data(), b->st, sizeof(ObjState) * hs.size(), hipMemcpyDeviceToHost));
  // the spare iteration (audit redo) counts only when some object ran in it
  const int used_iters = b->spare_run ? b->loop_iters : b->iters;
  for (int it = 0; it < (b->timed ? used_iters : 0); ++it)
    for (int g = 0; g < G; ++g) {
      const hipEvent_t* ev = b->ev.data() + 2 + ((size_t)it * G + g) * epi;
      for (int pz = 0; pz < np; ++pz) {
        DSR_CHECK(b->ctx, hipEventElapsedTime(&ms, ev[2 * pz], ev[2 * pz + 1]));
        st->fwd_ms += ms;
      }
      const int je = 2 * (np + (b->lite ? 1 : 0));
      if (b->lite) {
        DSR_CHECK(b->ctx, hipEventElapsedTime(&ms, ev[2 * np], ev[2 * np + 1]));
        st->refine_ms += ms;
      }
      DSR_CHECK(b->ctx, hipEventElapsedTime(&ms, ev[je], ev[je + 1]));
      st->jac_ms += ms;
    }
  DSR_CHECK(b->ctx, hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
  st->total_ms = ms;
  st->fwd_launches = b->timed ? used_iters * np * G : 0;
  st->jac_launches = b->timed ? used_iters * G : 0;
  st->refine_launches = (b->timed && b->lite) ? used_iters * G : 0;
  st->lite = b->lite ? 1 : 0;
  st->test_hooks = b->hooks ? 1 : 0;
  st->lite_eligible = b->dec->info.lite_eligible;
  st->audit = (b->lite && b->lite_cfg.audit) ? 1 : 0;
  st->audit_shell = b->lite_cfg.shell;
  st->audit_log2 = b->lite_cfg.audit_log2;
  st->lite_margin0 = b->P.lite_margin0;
  st->lite_floor = b->P.lite_floor;
  st->lite_safety = b->P.lite_safety;
  st->graph_captures = b->captures;
  st->graph_replays = b->replays;
  st->n_groups = (int)b->groups.size();
  st->graph_mode = b->cap_graph ? 2 : (graph_enabled() ? 1 : 0);
  st->fwd_variant = b->ran_fwd;
  st->jac_variant = b->ran_jac;
  st->lite_variant = b->ran_lite;
  st->split_ring = b->ran_ring;
  st->prescan = b->prescan ? 1 : 0;
  {
    int nb = 0;
    DSR_CHECK(b->ctx, hipMemcpy(&nb, b->diag + STD_BROKEN, sizeof(int), hipMemcpyDeviceToHost));
    st->lite_broken_blocks = nb;
  }
  st->keep_masks = (b->lite && b->ma.msk && b->ran_fwd == 12) ? 1 : 0;
  st->surface_in_exact = (st->keep_masks && b->ma.pts && b->ran_jac == 12) ? 1 : 0;
  if (b->lite) {
    st->lite_min_margin = 1e30;
    for (const ObjState& o : hs) {
      st->lite_max_err = std::max(st->lite_max_err, (double)o.lite_err);
      if (o.iters_done > 0) st->lite_min_margin = std::min(st->lite_min_margin, (double)o.lite_margin);
      st->lite_audit_violations += o.lite_viol_total;
      st->lite_redo_objects += o.lite_redo ? 1 : 0;
    }
  }
  std::vector<int> c((size_t)COUNT_STRIDE * std::max(1, b->loop_iters) * b->n_obj);
  DSR_CHECK(b->ctx, hipMemcpy(c.data(), b->counts, sizeof(int) * c.size(), hipMemcpyDeviceToHost));
  for (int it = 0; it < used_iters; ++it)
    for (int o = 0; o < b->n_obj; ++o) {
      const int* e = c.data() + ((size_t)it * b->n_obj + o) * COUNT_STRIDE;
      st->fwd_points += e[0];
      st->jac_points += e[1];
      st->inball_points += e[2];
      st->refine_points += e[3];
      st->audit_points += e[4];
      st->jac_render_points += e[5];
      st->jac_surface_points += e[1] - e[5];
    }
  return 0;
}

#ifdef DSR_EXP_PROV
// diagnostic build only: the provenance arrays of the batch's last run (tools/prov_diff.py);
// null pointers: just the sizes R (rays) and C (samples)
int dsr_exp_prov(dsr_batch* b, int* alive, float* y, int* set, int* xcc, int* R, int* C, int* jf, unsigned* t,
                 unsigned* h, unsigned* ri, float* nrm, float* nrm2) {
  if (!b) return -2;
  hipSetDevice(b->ctx->device);
  if (b->ran) {
    const int rc = batch_finish(b);
    if (rc) return rc;
  }
  if (R) *R = b->prov_R;
  if (C) *C = b->prov_C;
  if (alive) DSR_CHECK(b->ctx, hipMemcpy(alive, b->prov_alive, sizeof(int) * (size_t)PROV_IT * 64 * b->prov_R, hipMemcpyDeviceToHost));
  if (y) DSR_CHECK(b->ctx, hipMemcpy(y, b->prov_y, sizeof(float) * (size_t)PROV_IT * b->prov_C, hipMemcpyDeviceToHost));
  if (nrm2) DSR_CHECK(b->ctx, hipMemcpy(nrm2, b->prov_nrm2, sizeof(float) * (size_t)PROV_IT * b->prov_R * 8, hipMemcpyDeviceToHost));
  if (nrm) DSR_CHECK(b->ctx, hipMemcpy(nrm, b->prov_nrm, sizeof(float) * (size_t)PROV_IT * b->prov_R * 12, hipMemcpyDeviceToHost));
  if (ri) DSR_CHECK(b->ctx, hipMemcpy(ri, b->prov_ri, sizeof(unsigned) * 2 * (size_t)PROV_IT * b->prov_R * 2, hipMemcpyDeviceToHost));
  if (h) DSR_CHECK(b->ctx, hipMemcpy(h, b->prov_h, sizeof(unsigned) * 2 * (size_t)PROV_IT * b->prov_R * 3, hipMemcpyDeviceToHost));
  if (jf) DSR_CHECK(b->ctx, hipMemcpy(jf, b->prov_j, sizeof(int) * (size_t)PROV_IT * 64 * b->prov_R, hipMemcpyDeviceToHost));
  if (t) DSR_CHECK(b->ctx, hipMemcpy(t, b->prov_t, sizeof(unsigned) * (size_t)PROV_IT * 65 * b->prov_R, hipMemcpyDeviceToHost));
  if (xcc) DSR_CHECK(b->ctx, hipMemcpy(xcc, b->prov_xcc, sizeof(int) * (size_t)PROV_IT * b->prov_R * 2, hipMemcpyDeviceToHost));
  if (set) DSR_CHECK(b->ctx, hipMemcpy(set, b->prov_set, sizeof(int) * (size_t)PROV_IT * b->prov_R, hipMemcpyDeviceToHost));
  return 0;
}
#endif
int dsr_batch_windows(dsr_batch* b, int* adaptive, int* n_bounds, int* bounds) {
  if (!b || !adaptive || !n_bounds) return -2;
  *adaptive = b->P.n_win > 0 ? 1 : 0;
  *n_bounds = (int)b->passes.size();
  if (!bounds) return 0;
  if (!b->ran) return fail(b->ctx, "batch has not run");
  hipSetDevice(b->ctx->device);
  {
    const int rc = batch_finish(b);
    if (rc) return rc;
  }
  std::vector<ObjState> hs(b->n_obj);
  DSR_CHECK(b->ctx, hipMemcpy(hs.data(), b->st, sizeof(ObjState) * hs.size(), hipMemcpyDeviceToHost));
  for (int o = 0; o < b->n_obj; ++o)
    for (int i = 0; i < *n_bounds; ++i)       // (a schedule too long for the table: the fixed one)
      bounds[(size_t)o * *n_bounds + i] = *n_bounds <= WIN_MAX ? hs[o].win[i] : b->passes[i];
  return 0;
}

int dsr_batch_lite_diag(dsr_batch* b, int* rec, int n) {
  if (!b || !rec || n < 0) return -2;
  if (!b->ran) return fail(b->ctx, "batch has not run");
  hipSetDevice(b->ctx->device);
  {
    const int rc = batch_finish(b);
    if (rc) return rc;
  }
  const int k = std::min(n, (int)STD_INTS);
  DSR_CHECK(b->ctx, hipMemcpy(rec, b->diag, sizeof(int) * k, hipMemcpyDeviceToHost));
  return 0;
}

// Multi-GPU from one process, replacing the per-detection loop of
// LocalMapping_util.cc:165-206: longest-processing-time-first partition of the objects over the
// devices (cost = n_rays * M + n_pts, the decoder work of one iteration, greedy to the least loaded
// device, ties to the lower device; the rule of reconstruct/parallel.py), one host thread per
// device runs its shard's batch, and ONE RCCL gather (ncclCommInitAll over the devices, ncclGather
// to device 0 over xGMI) brings every shard's fixed-size dsr_object_out records to device 0, whose
// single download is unpacked into input order.  Each shard's records sit in a slot of
// max-shard-size records (the gather's equal counts): object i lands at record
// dev[i] * maxn + slot[i] of the gathered buffer (dsr_gather_layout).  RCCL is loaded at run time;
// when it is missing or its communicator cannot be built (e.g. two contexts on one device), the
// records are gathered through host memory instead, and *path says which route ran.
int dsr_gather_layout(int n_obj, const dsr_object_in* in, int num_depth_samples, int n_dev, int* dev, int* slot,
                      int* maxn) {
  if (n_obj <= 0 || !in || n_dev <= 0 || !dev || !slot || !maxn) return -2;
  std::vector<int> order(n_obj);
  for (int i = 0; i < n_obj; ++i) order[i] = i;
  auto cost = [&](int i) { return (double)in[i].n_rays * num_depth_samples + in[i].n_pts; };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost(a) > cost(b); });
  std::vector<double> load(n_dev, 0.0);
  for (int i : order) {
    const int g = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    dev[i] = g;
    load[g] += cost(i);
  }
  std::vector<int> cnt(n_dev, 0);
  for (int i = 0; i < n_obj; ++i) slot[i] = cnt[dev[i]]++;   // input order within a shard
  *maxn = *std::max_element(cnt.begin(), cnt.end());
  return 0;
}

}  // extern "C" (the RCCL loader is C++: the block reopens after it)

namespace {
// RCCL entry points, resolved from librccl at first use (no link-time dependency: a host
// without RCCL still loads libdsr and gathers through host memory)
struct Rccl {
  decltype(&ncclCommInitAll) init_all = nullptr;
  decltype(&ncclGather) gather = nullptr;
  decltype(&ncclGroupStart) group_start = nullptr;
  decltype(&ncclGroupEnd) group_end = nullptr;
  decltype(&ncclGetErrorString) err = nullptr;
  bool ok = false;
};
const Rccl& rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    r.init_all = (decltype(r.init_all))dlsym(h, "ncclCommInitAll");
    r.gather = (decltype(r.gather))dlsym(h, "ncclGather");
    r.group_start = (decltype(r.group_start))dlsym(h, "ncclGroupStart");
    r.group_end = (decltype(r.group_end))dlsym(h, "ncclGroupEnd");
    r.err = (decltype(r.err))dlsym(h, "ncclGetErrorString");
    r.ok = r.init_all && r.gather && r.group_start && r.group_end && r.err;
  });
  return r;
}
// one communicator set per device list, built once and kept for the process (ncclCommInitAll
// costs far more than a gather); an empty entry records a list RCCL refused
std::mutex comm_mu;
std::map<std::vector<int>, std::vector<ncclComm_t>> comm_cache;
const std::vector<ncclComm_t>* comms_for(const std::vector<int>& devs, std::string& why) {
  const Rccl& R = rccl();
  if (!R.ok) {
    why = "librccl not loadable";
    return nullptr;
  }
  std::lock_guard<std::mutex> lk(comm_mu);
  auto it = comm_cache.find(devs);
  if (it == comm_cache.end()) {
    std::vector<ncclComm_t> c(devs.size(), nullptr);
    const ncclResult_t rc = R.init_all(c.data(), (int)devs.size(), devs.data());
    if (rc != ncclSuccess) {
      why = std::string("ncclCommInitAll: ") + R.err(rc);
      c.clear();
    }
    it = comm_cache.emplace(devs, c).first;
  }
  if (it->second.empty()) {
    if (why.empty()) why = "ncclCommInitAll refused this device list";
    return nullptr;
  }
  return &it->second;
}
}  // namespace

extern "C" {

int dsr_reconstruct_multi_ex(dsr_ctx* const* ctxs, const dsr_decoder* const* decs, int n_dev,
                             const dsr_optim_params* p, int n_obj, const dsr_object_in* in, dsr_object_out* out,
                             int* path) {
  if (!ctxs || !decs || n_dev <= 0 || !ctxs[0]) return -2;
  dsr_ctx* c0 = ctxs[0];
  if (!p || !out || (n_obj > 0 && !in)) return fail(c0, "null argument");
  if (n_obj <= 0) return fail(c0, "n_obj must be > 0");
  for (int g = 0; g < n_dev; ++g)
    if (!ctxs[g] || !decs[g]) return fail(c0, "null context or decoder");
  if (path) *path = DSR_GATHER_HOST;
  std::vector<int> dev(n_obj), slot(n_obj);
  int maxn = 0;
  dsr_gather_layout(n_obj, in, p->num_depth_samples, n_dev, dev.data(), slot.data(), &maxn);
  std::vector<std::vector<int>> shard(n_dev);
  for (int i = 0; i < n_obj; ++i) shard[dev[i]].push_back(i);
  // the communicators first (one per device, device 0 the root), before any work is queued
  std::vector<int> devs(n_dev);
  for (int g = 0; g < n_dev; ++g) devs[g] = ctxs[g]->device;
  std::string why;
  const std::vector<ncclComm_t>* comms = comms_for(devs, why);
  const size_t rec = sizeof(dsr_object_out);
  std::vector<dsr_batch*> batch(n_dev, nullptr);
  std::vector<void*> send(n_dev, nullptr);
  void* recv = nullptr;
  std::vector<int> rc(n_dev, 0);
  auto run = [&](int g) {
    dsr_ctx* ctx = ctxs[g];
    hipSetDevice(ctx->device);
    const std::vector<int>& sh = shard[g];
    if (comms) {                                 // the shard's slot of the gather (zero-padded)
      if (hipMalloc(&send[g], rec * (size_t)std::max(1, maxn)) != hipSuccess ||
          hipMemsetAsync(send[g], 0, rec * (size_t)std::max(1, maxn), ctx->stream) != hipSuccess) {
        rc[g] = fail(ctx, "hipMalloc failed (gather slot)");
        return;
      }
    }
    if (sh.empty()) return;
    std::vector<dsr_object_in> sin;
    for (int i : sh) sin.push_back(in[i]);
    if ((rc[g] = batch_create_impl(ctx, decs[g], p, (int)sh.size(), sin.data(), false, &batch[g])) != 0) return;
    if ((rc[g] = dsr_batch_run(batch[g])) != 0) return;
    if ((rc[g] = batch_finish(batch[g])) != 0) return;       // (its spare iteration included)
    if (comms) {
      if (hipMemcpyAsync(send[g], batch[g]->out, rec * sh.size(), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
        rc[g] = fail(ctx, "hipMemcpyAsync failed (gather slot)");
    } else {                                     // host gather: each shard downloads its own records
      std::vector<dsr_object_out> res(sh.size());
      if ((rc[g] = dsr_batch_download(batch[g], res.data())) != 0) return;
      for (size_t k = 0; k < sh.size(); ++k) out[sh[k]] = res[k];
    }
  };
  if (comms) {
    hipSetDevice(c0->device);
    if (hipMalloc(&recv, rec * (size_t)maxn * n_dev) != hipSuccess) return fail(c0, "hipMalloc failed (gather)");
  }
  {
    std::vector<std::thread> th;
    for (int g = 1; g < n_dev; ++g) th.emplace_back(run, g);
    run(0);
    for (auto& t : th) t.join();
  }
  int status = 0;
  for (int g = 0; g < n_dev && !status; ++g)
    if (rc[g]) status = fail(c0, "device shard " + std::to_string(g) + ": " + ctxs[g]->err);
  if (!status && comms) {
    // ONE gather of every shard's slot to device 0 (ncclUint8 counts: the records are opaque)
    const Rccl& R = rccl();
    ncclResult_t nr = R.group_start();
    for (int g = 0; g < n_dev && nr == ncclSuccess; ++g) {
      hipSetDevice(ctxs[g]->device);
      nr = R.gather(send[g], g == 0 ? recv : nullptr, rec * (size_t)maxn, ncclUint8, 0, (*comms)[g], ctxs[g]->stream);
    }
    const ncclResult_t ne = R.group_end();
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) {
      status = fail(c0, std::string("ncclGather: ") + R.err(nr));
    } else {
      std::vector<unsigned char> h(rec * (size_t)maxn * n_dev);
      hipSetDevice(c0->device);
      if (hipMemcpyAsync(h.data(), recv, h.size(), hipMemcpyDeviceToHost, c0->stream) != hipSuccess ||
          hipStreamSynchronize(c0->stream) != hipSuccess) {
        status = fail(c0, "gather download failed");
      } else {
        for (int i = 0; i < n_obj; ++i)
          std::memcpy(&out[i], h.data() + rec * ((size_t)dev[i] * maxn + slot[i]), rec);
        if (path) *path = DSR_GATHER_RCCL;
      }
    }
  }
  for (int g = 0; g < n_dev; ++g) {
    hipSetDevice(ctxs[g]->device);
    if (send[g]) {
      hipStreamSynchronize(ctxs[g]->stream);
      hipFree(send[g]);
    }
    if (batch[g]) dsr_batch_destroy(batch[g]);
  }
  if (recv) {
    hipSetDevice(c0->device);
    hipFree(recv);
  }
  return status;
}

int dsr_reconstruct_multi(dsr_ctx* const* ctxs, const dsr_decoder* const* decs, int n_dev,
                          const dsr_optim_params* p, int n_obj, const dsr_object_in* in, dsr_object_out* out) {
  return dsr_reconstruct_multi_ex(ctxs, decs, n_dev, p, n_obj, in, out, nullptr);
}

// The trace of a finished batch run into n_out caller records: record o is that of batch member
// member[o] (nullptr: member o).
static int trace_download(dsr_batch* b, int n_out, const int* member, const dsr_trace* trace) {
  dsr_ctx* ctx = b->ctx;
  const int it = b->iters, n_obj = b->n_obj, code_len = b->dec->code_len;
  std::vector<float> H((size_t)TRACE_H_STRIDE * std::max(1, it) * n_obj), V((size_t)TRACE_V_STRIDE * std::max(1, it) * n_obj);
  std::vector<int> I((size_t)TRACE_I_STRIDE * std::max(1, it) * n_obj);
  if (hipMemcpy(H.data(), b->tr_H, sizeof(float) * H.size(), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(V.data(), b->tr_v, sizeof(float) * V.size(), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(I.data(), b->tr_i, sizeof(int) * I.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(ctx, "trace download failed");
  for (int o = 0; o < n_out; ++o) {
    const dsr_trace& t = trace[o];
    for (int e = 0; e < it; ++e) {
      const size_t k = (size_t)e * n_obj + (member ? member[o] : o);
      if (t.H) std::memcpy(t.H + (size_t)e * NPAR * NPAR, H.data() + k * TRACE_H_STRIDE, sizeof(float) * NPAR * NPAR);
      const float* v = V.data() + k * TRACE_V_STRIDE;
      if (t.b) std::memcpy(t.b + (size_t)e * NPAR, v, sizeof(float) * NPAR);
      if (t.dx) std::memcpy(t.dx + (size_t)e * NPAR, v + NPAR, sizeof(float) * NPAR);
      if (t.loss) t.loss[e] = v[2 * NPAR];
      if (t.sdf_loss) t.sdf_loss[e] = v[2 * NPAR + 1];
      if (t.render_loss) t.render_loss[e] = v[2 * NPAR + 2];
      if (t.t_obj_cam) std::memcpy(t.t_obj_cam + (size_t)e * 16, v + 2 * NPAR + 3, sizeof(float) * 16);
      if (t.z) std::memcpy(t.z + (size_t)e * code_len, v + 2 * NPAR + 19, sizeof(float) * code_len);
      if (t.n_valid) t.n_valid[e] = I[k * TRACE_I_STRIDE];
      if (t.k) t.k[e] = I[k * TRACE_I_STRIDE + 1];
      if (t.n_decoded) t.n_decoded[e] = I[k * TRACE_I_STRIDE + 2];
      if (t.n_refined) t.n_refined[e] = I[k * TRACE_I_STRIDE + 3];
    }
  }
  return 0;
}

int dsr_reconstruct_batch(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, int n_obj,
                          const dsr_object_in* in, dsr_object_out* out, const dsr_trace* trace) {
  if (!out) return fail(ctx, "null output");
  dsr_batch* b = nullptr;
  int rc = batch_create_impl(ctx, dec, p, n_obj, in, trace != nullptr, &b);
  if (rc) return rc;
  rc = dsr_batch_run(b);
  if (!rc) rc = dsr_batch_download(b, out);
  if (!rc && trace) rc = trace_download(b, n_obj, nullptr, trace);
  dsr_batch_destroy(b);
  return rc;
}

int dsr_reconstruct_views(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, int n_obj,
                          const dsr_views_object_in* in, dsr_object_out* out, const dsr_trace* trace,
                          int* fail_view, dsr_stats* stats) {
  if (n_obj > 0 && !in) return fail(ctx, "null argument");
  if (!out) return fail(ctx, "null output");
  if (n_obj <= 0) return fail(ctx, "n_obj must be > 0");
  // every view one member of an ordinary batch, an object's views consecutive, view 0 first
  // (the views are validated here, before anything needs the device; batch_create_impl checks
  // the context, the decoder, the parameters and the members' buffers)
  std::vector<dsr_object_in> mem;
  std::vector<int> views(n_obj), leader(n_obj);
  std::vector<float> cview;
  for (int o = 0; o < n_obj; ++o) {
    const dsr_views_object_in& x = in[o];
    if (x.n_views < 1 || !x.views) return fail(ctx, "an object needs n_views >= 1 views");
    if ((long long)mem.size() + x.n_views > (long long)INT_MAX / 64) return fail(ctx, "too many views");
    views[o] = x.n_views;
    leader[o] = (int)mem.size();
    for (int v = 0; v < x.n_views; ++v) {
      const dsr_view_in& w = x.views[v];
      float c[16];
      if (!rigid_inverse(w.t_view_ref, c))
        return fail(ctx, "t_view_ref is not rigid (last row 0 0 0 1, R^T R = I within 1e-4, det R > 0)");
      if (v == 0)                                // the reference view: T_0 = T, never multiplied
        for (int i = 0; i < 16; ++i)
          if (std::fabs(w.t_view_ref[i] - (i % 5 == 0 ? 1.f : 0.f)) > 1e-6f)
            return fail(ctx, "view 0 is the reference view: its t_view_ref must be the identity");
      cview.insert(cview.end(), c, c + 16);
      dsr_object_in m{};
      std::copy(x.t_cam_obj, x.t_cam_obj + 16, m.t_cam_obj);     // (views >= 1: k_views_pose overwrites the pose)
      m.pts = w.pts; m.n_pts = w.n_pts;
      m.rays = w.rays; m.n_rays = w.n_rays;
      m.depth = w.depth; m.n_depth = w.n_depth;
      m.code = x.code;
      m.pose_is_obj_cam = x.pose_is_obj_cam;
      mem.push_back(m);
    }
  }
  const int n_mem = (int)mem.size();
  dsr_batch* b = nullptr;
  int rc = batch_create_impl(ctx, dec, p, n_mem, mem.data(), trace != nullptr, &b, false, &views, cview.data());
  if (rc) return rc;
  std::vector<dsr_object_out> mout(n_mem);
  rc = dsr_batch_run(b);
  if (!rc) rc = dsr_batch_download(b, mout.data());
  if (!rc) {
    for (int o = 0; o < n_obj; ++o) {            // the reference view's record, the counts summed
      out[o] = mout[leader[o]];
      for (int v = 1; v < views[o]; ++v) {
        out[o].n_valid_last += mout[leader[o] + v].n_valid_last;
        out[o].k_last += mout[leader[o] + v].k_last;
      }
    }
    if (fail_view) {                             // (tie[] order is object order)
      if (hipMemcpy(fail_view, b->fail_view, sizeof(int) * n_obj, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(ctx, "fail_view download failed");
    }
  }
  if (!rc && trace) rc = trace_download(b, n_obj, leader.data(), trace);
  if (!rc && stats) rc = dsr_batch_stats(b, stats);
  dsr_batch_destroy(b);
  return rc;
}

// ------------------------------------------------------------------------------------
// mesh extraction (MeshExtractor, optimizer.py:216-233; utils.py:119-140)
// ------------------------------------------------------------------------------------
// S slots of everything a mesh needs; a call runs its codes in passes of up to S.  S grows with
// the calls' code counts up to MESH_MAX_SLOTS and while one pass's buffers stay within
// MESH_BUDGET (the marching-cubes buffers hold the worst case of every slot: ~270 MB per slot at
// 128^3, so 6 slots there; 16 up to 96^3).
static constexpr int MESH_MAX_SLOTS = 16;
static constexpr size_t MESH_BUDGET = (size_t)2 << 30;
static constexpr float MESH_MARGIN = 0.01f;      // §3.4's first-iteration margin

struct MeshBatch {
  int S = 0, np = 0, ntl = 0, n_rb = 0;
  int last_ns = 0;             // slots of the last pass (dsr_mesher_peek)
  bool last_sign = false;
  DevArena mem;
  float4* pts = nullptr;       // the grid, once per slot (the kernels index it by ObjDesc.cand_off)
  float *lite = nullptr, *vol = nullptr, *codes = nullptr, *b0 = nullptr, *b4 = nullptr, *verts = nullptr;
  unsigned char *refine = nullptr, *tflag = nullptr;
  int *flag = nullptr, *vidx = nullptr, *ntri = nullptr, *toff = nullptr, *bsum = nullptr, *faces = nullptr;
  int *tmark = nullptr, *tpos = nullptr;
  Tile *ltiles = nullptr, *atiles = nullptr, *etiles = nullptr, *rtiles = nullptr;
  ObjDesc* desc = nullptr;
  ObjState* st = nullptr;
  // one record of ints read back per pass: vertex offsets (S+1), face offsets (S+1), counters
  // (MS_INTS), tile counts (4: lite, all, band, redo), per-slot error bits / violations / redo
  // flag (S each), the lite kernel's wait record (STD_INTS)
  int* rb = nullptr;
  int *offs_v = nullptr, *offs_f = nullptr, *stat = nullptr, *cnt = nullptr, *slot_err = nullptr,
      *slot_viol = nullptr, *slot_redo = nullptr, *diag = nullptr;
  hipEvent_t ev[4] = {};
  std::vector<float> hcodes, hv;
  std::vector<int> hrb, hf;
};

static void mesh_batch_free(MeshBatch* b) {
  if (!b) return;
  for (hipEvent_t e : b->ev)
    if (e) hipEventDestroy(e);
  delete b;
}

struct dsr_mesher {
  dsr_ctx* ctx = nullptr;
  const dsr_decoder* dec = nullptr;
  int d = 0, n = 0, nt = 0;
  DevArena mem;
  float4* pts = nullptr;       // grid points (x,y,z, bits(index)), tile-padded
  Tile* tiles = nullptr;
  int* ntiles = nullptr;
  ObjDesc* desc = nullptr;
  float *code = nullptr, *b0 = nullptr, *b4 = nullptr, *vol = nullptr;
  int *flag = nullptr, *vidx = nullptr, *ntri = nullptr, *toff = nullptr, *bsum = nullptr, *tot = nullptr;
  float* verts = nullptr;
  int* faces = nullptr;
  MeshBatch* mb = nullptr;     // dsr_mesher_run_batch's slots (allocated on its first call)
  dsr_mesher_stats st{};       // its last call
};

int dsr_mesher_destroy(dsr_mesher* m) {
  if (!m) return 0;
  hipSetDevice(m->ctx->device);
  mesh_batch_free(m->mb);
  delete m;
  return 0;
}

// The marching-cubes half of a mesher: the volume (tile-padded: the grid decode writes it) and
// the edge / cell / scan / output buffers for m->d.
static bool mesher_alloc_mc(dsr_mesher* m) {
  const int d = m->d, n = m->n, nc = (d - 1) * (d - 1) * (d - 1), ne = 3 * n;
  const int nb = (std::max(ne, nc) + MC_SCAN_BLOCK - 1) / MC_SCAN_BLOCK;
  DevArena& M = m->mem;
  return M.alloc(&m->vol, (size_t)m->nt * TILE) && M.alloc(&m->flag, ne) && M.alloc(&m->vidx, ne) &&
         M.alloc(&m->ntri, nc) && M.alloc(&m->toff, nc) && M.alloc(&m->bsum, nb) && M.alloc(&m->tot, 2) &&
         M.alloc(&m->verts, 3 * (size_t)ne) && M.alloc(&m->faces, 3 * (size_t)DSR_MC_MAX_TRI * nc);
}

int dsr_mesher_create(dsr_ctx* ctx, const dsr_decoder* dec, const float* grid_pts, int vol_dim,
                      dsr_mesher** out) {
  if (!ctx || !dec || !grid_pts || !out) return fail(ctx, "null argument");
  *out = nullptr;
  if (vol_dim < 2 || vol_dim > 512) return fail(ctx, "vol_dim must be in [2, 512]");
  if (int rc = decoder_ready(ctx, dec)) return rc;
  hipSetDevice(ctx->device);
  auto* m = new dsr_mesher();
  m->ctx = ctx;
  m->dec = dec;
  m->d = vol_dim;
  m->n = vol_dim * vol_dim * vol_dim;
  m->nt = (m->n + TILE - 1) / TILE;
  const int n = m->n, nt = m->nt;
  DevArena& M = m->mem;
  if (!M.alloc(&m->pts, (size_t)nt * TILE) || !M.alloc(&m->tiles, nt) || !M.alloc(&m->ntiles, 1) ||
      !M.alloc(&m->desc, 1) || !M.alloc(&m->code, CODE) || !M.alloc(&m->b0, HID) || !M.alloc(&m->b4, HID) ||
      !mesher_alloc_mc(m)) {
    dsr_mesher_destroy(m);
    return fail(ctx, "hipMalloc failed (mesher)");
  }
  std::vector<float4> hp((size_t)nt * TILE, make_float4(0.f, 0.f, 0.f, 0.f));
  for (int i = 0; i < n; ++i) {
    float fi;
    std::memcpy(&fi, &i, sizeof(float));
    hp[i] = make_float4(grid_pts[(size_t)i * 3], grid_pts[(size_t)i * 3 + 1], grid_pts[(size_t)i * 3 + 2], fi);
  }
  std::vector<Tile> ht(nt);
  for (int t = 0; t < nt; ++t) ht[t] = Tile{0, 0, t * TILE, std::min(TILE, n - t * TILE)};
  ObjDesc od{};
  od.n_pts = n;
  if (hipMemcpy(m->pts, hp.data(), sizeof(float4) * hp.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->tiles, ht.data(), sizeof(Tile) * nt, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->ntiles, &nt, sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(m->desc, &od, sizeof(ObjDesc), hipMemcpyHostToDevice) != hipSuccess) {
    dsr_mesher_destroy(m);
    return fail(ctx, "hipMemcpy failed (mesher)");
  }
  *out = m;
  return 0;
}

static void mc_scan(hipStream_t s, const int* in, int n, int* out, int* bsum, int* total) {
  const int nb = (n + MC_SCAN_BLOCK - 1) / MC_SCAN_BLOCK;
  hipLaunchKernelGGL(k_scan_blocks, dim3(nb), dim3(MC_SCAN_BLOCK), 0, s, in, n, bsum);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(MC_SCAN_BLOCK), 0, s, bsum, nb, total);
  hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(MC_SCAN_BLOCK), 0, s, in, n, (const int*)bsum, out);
}

// Marching cubes over m->vol (already on m's context stream) and the copy-out.
static int mc_run(dsr_mesher* m, float level, float* verts, int vcap, int* faces, int fcap, int* n_verts,
                  int* n_faces) {
  dsr_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int d = m->d, n = m->n, nc = (d - 1) * (d - 1) * (d - 1), ne = 3 * n;
  const int B = 256;
  hipLaunchKernelGGL(k_mc_edges, dim3((n + B - 1) / B), dim3(B), 0, s, (const float*)m->vol, d, level, m->flag);
  hipLaunchKernelGGL(k_mc_cells, dim3((nc + B - 1) / B), dim3(B), 0, s, (const float*)m->vol, d, level, m->ntri);
  mc_scan(s, m->flag, ne, m->vidx, m->bsum, m->tot);
  mc_scan(s, m->ntri, nc, m->toff, m->bsum, m->tot + 1);
  hipLaunchKernelGGL(k_mc_verts, dim3((ne + B - 1) / B), dim3(B), 0, s, (const float*)m->vol, d, level,
                     2.0 / (double)(d - 1), (const int*)m->flag, (const int*)m->vidx, m->verts);
  hipLaunchKernelGGL(k_mc_faces, dim3((nc + B - 1) / B), dim3(B), 0, s, (const float*)m->vol, d, level,
                     (const int*)m->vidx, (const int*)m->toff, m->faces);
  DSR_CHECK(ctx, hipGetLastError());
  int tot[2];
  DSR_CHECK(ctx, hipMemcpyAsync(tot, m->tot, sizeof(int) * 2, hipMemcpyDeviceToHost, s));
  DSR_CHECK(ctx, hipStreamSynchronize(s));
  *n_verts = tot[0];
  *n_faces = tot[1];
  if (tot[0] > vcap || tot[1] > fcap || (tot[0] > 0 && !verts) || (tot[1] > 0 && !faces)) {
    fail(ctx, "mesh larger than the given capacity");
    return -5;
  }
  if (tot[0] > 0) DSR_CHECK(ctx, hipMemcpy(verts, m->verts, sizeof(float) * 3 * tot[0], hipMemcpyDeviceToHost));
  if (tot[1] > 0) DSR_CHECK(ctx, hipMemcpy(faces, m->faces, sizeof(int) * 3 * tot[1], hipMemcpyDeviceToHost));
  return 0;
}

int dsr_mesher_run(dsr_mesher* m, const float* code, float level, float* verts, int vcap, int* faces,
                   int fcap, int* n_verts, int* n_faces) {
  if (!m || !code || !n_verts || !n_faces) return fail(m ? m->ctx : nullptr, "null argument");
  dsr_ctx* ctx = m->ctx;
  if (int rc = decoder_ready(ctx, m->dec)) return rc;
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  const DevDecoder& D = m->dec->D;
  float zc[CODE] = {};                               // a 32-D code runs padded with zeros
  std::memcpy(zc, code, sizeof(float) * m->dec->code_len);
  DSR_CHECK(ctx, hipMemcpyAsync(m->code, zc, sizeof(float) * CODE, hipMemcpyHostToDevice, s));
  DSR_CHECK(ctx, hipStreamSynchronize(s));          // (zc is on this stack frame)
  fold_codes(s, D, m->code, 1, m->b0, m->b4);
  launch_fwd(s, std::min(ctx->n_cu, m->nt), D, {m->tiles, m->ntiles, m->desc, m->pts, m->b0, m->b4, m->vol});
  return mc_run(m, level, verts, vcap, faces, fcap, n_verts, n_faces);
}

int dsr_mc_volume(dsr_ctx* ctx, const float* vol, int vol_dim, float level, float* verts, int vcap, int* faces,
                  int fcap, int* n_verts, int* n_faces) {
  if (!ctx || !vol || !n_verts || !n_faces) return fail(ctx, "null argument");
  if (vol_dim < 2 || vol_dim > 512) return fail(ctx, "vol_dim must be in [2, 512]");
  hipSetDevice(ctx->device);
  dsr_mesher m;
  m.ctx = ctx;
  m.d = vol_dim;
  m.n = vol_dim * vol_dim * vol_dim;
  m.nt = (m.n + TILE - 1) / TILE;
  struct Drain {      // the scratch lives for this call only: m's arena frees it once the stream is idle
    hipStream_t s;
    ~Drain() { hipStreamSynchronize(s); }
  } drain{ctx->stream};
  if (!mesher_alloc_mc(&m)) return fail(ctx, "hipMalloc failed (marching cubes)");
  DSR_CHECK(ctx, hipMemcpyAsync(m.vol, vol, sizeof(float) * (size_t)m.n, hipMemcpyHostToDevice, ctx->stream));
  return mc_run(&m, level, verts, vcap, faces, fcap, n_verts, n_faces);
}

// ------------------------------------------------------------------------------------
// batched mesh extraction (dsr_mesh.hpp)
// ------------------------------------------------------------------------------------
static size_t mesh_slot_bytes(const dsr_mesher* m) {
  const size_t n = m->n, nc = (size_t)(m->d - 1) * (m->d - 1) * (m->d - 1), np = (n + LTILE - 1) / LTILE * LTILE;
  return np * (sizeof(float4) + 2 * sizeof(float) + 1) + sizeof(int) * std::max(3 * n, np) + sizeof(int) * 3 * n +
         2 * sizeof(int) * nc + sizeof(float) * 9 * n + sizeof(int) * 3 * DSR_MC_MAX_TRI * nc +
         (size_t)m->nt * (3 * sizeof(Tile) + 2 * sizeof(int) + 1) + np / LTILE * sizeof(Tile);
}

// (re)allocate the batch half of a mesher for S slots; false: out of memory (nothing is kept)
static bool mesh_batch_alloc(dsr_mesher* m, int S) {
  mesh_batch_free(m->mb);
  m->mb = nullptr;
  auto* b = new MeshBatch();
  const int n = m->n, nt = m->nt, d = m->d, nc = (d - 1) * (d - 1) * (d - 1);
  const int np = (n + LTILE - 1) / LTILE * LTILE, ntl = np / LTILE;
  const size_t Sz = (size_t)S, fl = std::max((size_t)3 * n, (size_t)np);
  b->S = S;
  b->np = np;
  b->ntl = ntl;
  b->n_rb = 2 * (S + 1) + MS_INTS + 4 + 3 * S + STD_INTS;
  const size_t nb = (Sz * std::max(fl, (size_t)std::max(nc, nt)) + MC_SCAN_BLOCK - 1) / MC_SCAN_BLOCK;
  DevArena& M = b->mem;
  bool ok = M.alloc(&b->pts, Sz * np) && M.alloc(&b->lite, Sz * np) && M.alloc(&b->vol, Sz * np) &&
            M.alloc(&b->refine, Sz * np) && M.alloc(&b->codes, Sz * CODE) && M.alloc(&b->b0, Sz * HID) &&
            M.alloc(&b->b4, Sz * HID) &&
            M.alloc(&b->flag, Sz * fl) &&          // (the lite kernel's dead flags live here too)
            M.alloc(&b->vidx, Sz * 3 * n) && M.alloc(&b->ntri, Sz * nc) && M.alloc(&b->toff, Sz * nc) &&
            M.alloc(&b->bsum, nb) && M.alloc(&b->verts, 3 * Sz * 3 * n) &&
            M.alloc(&b->faces, 3 * Sz * DSR_MC_MAX_TRI * nc) && M.alloc(&b->tflag, Sz * nt) &&
            M.alloc(&b->tmark, Sz * nt) && M.alloc(&b->tpos, Sz * nt) && M.alloc(&b->ltiles, Sz * ntl) &&
            M.alloc(&b->atiles, Sz * nt) && M.alloc(&b->etiles, Sz * nt) && M.alloc(&b->rtiles, Sz * nt) &&
            M.alloc(&b->desc, Sz) && M.alloc(&b->st, Sz) && M.alloc(&b->rb, b->n_rb);
  for (hipEvent_t& e : b->ev)
    if (ok && hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); e = nullptr; ok = false; }
  if (ok) {
    b->offs_v = b->rb;
    b->offs_f = b->offs_v + S + 1;
    b->stat = b->offs_f + S + 1;
    b->cnt = b->stat + MS_INTS;
    b->slot_err = b->cnt + 4;
    b->slot_viol = b->slot_err + S;
    b->slot_redo = b->slot_viol + S;
    b->diag = b->slot_redo + S;
    std::vector<Tile> lt(Sz * ntl), at(Sz * nt);
    std::vector<ObjDesc> hd(S);
    for (int s = 0; s < S; ++s) {
      hd[s] = ObjDesc{};
      hd[s].n_pts = n;
      hd[s].ray_off = s * np;
      hd[s].n_rays = np;
      hd[s].cand_off = s * np;
      for (int t = 0; t < ntl; ++t) lt[(size_t)s * ntl + t] = Tile{s, 0, t * LTILE, std::min(LTILE, n - t * LTILE)};
      for (int t = 0; t < nt; ++t) at[(size_t)s * nt + t] = Tile{s, 0, t * TILE, std::min(TILE, n - t * TILE)};
    }
    ok = hipMemset(b->pts, 0, sizeof(float4) * Sz * np) == hipSuccess &&
         hipMemset(b->st, 0, sizeof(ObjState) * Sz) == hipSuccess &&
         hipMemcpy(b->ltiles, lt.data(), sizeof(Tile) * lt.size(), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(b->atiles, at.data(), sizeof(Tile) * at.size(), hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(b->desc, hd.data(), sizeof(ObjDesc) * Sz, hipMemcpyHostToDevice) == hipSuccess;
    for (int s = 0; ok && s < S; ++s)
      ok = hipMemcpy(b->pts + (size_t)s * np, m->pts, sizeof(float4) * n, hipMemcpyDeviceToDevice) == hipSuccess;
    if (!ok) (void)hipGetLastError();
  }
  if (!ok) {
    mesh_batch_free(b);
    return false;
  }
  b->hrb.resize(b->n_rb);
  m->mb = b;
  return true;
}

// may this decoder's lite values settle the sign of a grid?  (DSR_MESH_LITE=0: a plain runtime
// switch, read per call)
static bool mesh_sign_pass(const dsr_decoder* dec) {
  const char* e = getenv("DSR_MESH_LITE");
  if (e && atoi(e) == 0) return false;
  return dec->info.lite_eligible && !is_variant(dec->D);
}

// one pass: ns codes (zero-padded to 64 floats each in b->hcodes) through fold, sign pass, exact
// tiles and marching cubes; the read-back record is in b->hrb when it returns (stream idle)
static int mesh_pass(dsr_mesher* m, int ns, float level, bool sign, const ErtArgs& hooks) {
  dsr_ctx* ctx = m->ctx;
  MeshBatch* b = m->mb;
  hipStream_t s = ctx->stream;
  const DevDecoder& D = m->dec->D;
  const int d = m->d, n = m->n, nt = m->nt, np = b->np, nc = (d - 1) * (d - 1) * (d - 1), ne = 3 * n;
  const int B = 256;
  DSR_CHECK(ctx, hipMemcpyAsync(b->codes, b->hcodes.data(), sizeof(float) * CODE * ns, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_mesh_begin, dim3(1), dim3(256), 0, s, b->rb, b->n_rb, b->cnt, ns * b->ntl, ns * nt);
  DSR_CHECK(ctx, hipEventRecord(b->ev[0], s));
  fold_codes(s, D, b->codes, ns, b->b0, b->b4);
  const int egrid = std::min(ctx->n_cu, ns * nt);
  if (sign) {
    DSR_CHECK(ctx, hipMemsetAsync(b->refine, 0, (size_t)ns * np, s));
    ErtArgs E = hooks;                   // lag, perturb (test hook)
    E.dead = b->flag;                    // M = 1, level-free classes: "full" is y <= 0, written and unused
    E.M = 1;
    E.nth = 0.f;
    E.st = b->st;                        // zeroed: margin 0, so only NaN / the range guard flag `refine`
    E.refine = b->refine;
    E.audit = 0;
    E.diag = b->diag;
    launch_lite(s, std::min(ctx->n_cu, ns * b->ntl), D, {b->ltiles, b->cnt, b->desc, b->pts, b->b0, b->b4, b->lite, E});
    DSR_CHECK(ctx, hipEventRecord(b->ev[1], s));
    hipLaunchKernelGGL(k_mesh_mark, dim3((nt + 3) / 4, ns), dim3(256), 0, s, (const float*)b->lite,
                       (const unsigned char*)b->refine, d, n, np, nt, level, MESH_MARGIN, b->tflag, b->tmark, b->stat);
    mc_scan(s, b->tmark, ns * nt, b->tpos, b->bsum, b->cnt + 2);
    hipLaunchKernelGGL(k_mesh_compact, dim3((ns * nt + B - 1) / B), dim3(B), 0, s, (const int*)b->tmark,
                       (const int*)b->tpos, nt, n, ns * nt, b->etiles);
    launch_fwd(s, egrid, D, {b->etiles, b->cnt + 2, b->desc, b->pts, b->b0, b->b4, b->vol});
    hipLaunchKernelGGL(k_mesh_merge, dim3((n + 255) / 256, ns), dim3(256), 0, s, (const float*)b->lite,
                       (const unsigned char*)b->refine, (const unsigned char*)b->tflag, n, np, nt, level,
                       MESH_MARGIN, b->vol, b->slot_err, b->slot_viol);
    hipLaunchKernelGGL(k_mesh_redo, dim3(1), dim3(MC_SCAN_BLOCK), 0, s, (const int*)b->slot_err,
                       (const int*)b->slot_viol, ns, nt, n, MESH_MARGIN, (const unsigned char*)b->tflag, b->rtiles,
                       b->cnt + 3, b->slot_redo, b->stat);
    // the rejected slots' remaining tiles (an empty table when the guard holds: the blocks return)
    launch_fwd(s, egrid, D, {b->rtiles, b->cnt + 3, b->desc, b->pts, b->b0, b->b4, b->vol});
  } else {
    DSR_CHECK(ctx, hipEventRecord(b->ev[1], s));
    launch_fwd(s, egrid, D, {b->atiles, b->cnt + 1, b->desc, b->pts, b->b0, b->b4, b->vol});
  }
  DSR_CHECK(ctx, hipEventRecord(b->ev[2], s));
  hipLaunchKernelGGL(k_mcb_edges, dim3((n + B - 1) / B, ns), dim3(B), 0, s, (const float*)b->vol, d, np, level, b->flag);
  hipLaunchKernelGGL(k_mcb_cells, dim3((nc + B - 1) / B, ns), dim3(B), 0, s, (const float*)b->vol, d, np, level, b->ntri);
  mc_scan(s, b->flag, ns * ne, b->vidx, b->bsum, b->offs_v + ns);
  mc_scan(s, b->ntri, ns * nc, b->toff, b->bsum, b->offs_f + ns);
  hipLaunchKernelGGL(k_mcb_verts, dim3((ne + B - 1) / B, ns), dim3(B), 0, s, (const float*)b->vol, d, np, level,
                     2.0 / (double)(d - 1), (const int*)b->flag, (const int*)b->vidx, b->verts, b->offs_v);
  hipLaunchKernelGGL(k_mcb_faces, dim3((nc + B - 1) / B, ns), dim3(B), 0, s, (const float*)b->vol, d, np, level,
                     (const int*)b->vidx, (const int*)b->toff, b->faces, b->offs_f);
  DSR_CHECK(ctx, hipGetLastError());
  DSR_CHECK(ctx, hipEventRecord(b->ev[3], s));
  DSR_CHECK(ctx, hipMemcpyAsync(b->hrb.data(), b->rb, sizeof(int) * b->n_rb, hipMemcpyDeviceToHost, s));
  DSR_CHECK(ctx, hipStreamSynchronize(s));
  b->last_ns = ns;
  b->last_sign = sign;
  return 0;
}

int dsr_mesher_run_batch(dsr_mesher* m, int n_codes, const float* codes, float level, float* verts, int vcap,
                         int* faces, int fcap, int* vert_off, int* face_off) {
  if (!m || !vert_off || !face_off || (n_codes > 0 && !codes)) return fail(m ? m->ctx : nullptr, "null argument");
  if (n_codes < 0) return fail(m->ctx, "n_codes must not be negative");
  dsr_ctx* ctx = m->ctx;
  dsr_mesher_stats& st = m->st;
  st = dsr_mesher_stats{};
  st.margin = MESH_MARGIN;
  vert_off[0] = face_off[0] = 0;
  if (n_codes == 0) return 0;
  if (int rc = decoder_ready(ctx, m->dec)) return rc;
  hipSetDevice(ctx->device);
  const int cap = (int)std::max<size_t>(1, std::min<size_t>(MESH_MAX_SLOTS, MESH_BUDGET / mesh_slot_bytes(m)));
  int want = std::min(n_codes, cap);
  if (!m->mb || m->mb->S < want) {
    DSR_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    while (!mesh_batch_alloc(m, want)) {           // out of memory: fewer slots, more passes
      if (want == 1) return fail(ctx, "hipMalloc failed (mesher batch)");
      want = (want + 1) / 2;
    }
  }
  MeshBatch* b = m->mb;
  const int S = b->S, L = m->dec->code_len;
  const bool hooks = test_hooks();
  const bool sign = mesh_sign_pass(m->dec);
  const ErtArgs E = lite_settings(hooks);
  const bool multi = n_codes > S;
  st.n_codes = n_codes;
  st.slots = S;
  st.sign_pass = sign ? 1 : 0;
  st.test_hooks = hooks ? 1 : 0;
  b->hv.clear();
  b->hf.clear();
  long long tv = 0, tf = 0;                          // running totals
  bool fits = true;
  for (int c0 = 0; c0 < n_codes; c0 += S) {
    const int ns = std::min(S, n_codes - c0);
    b->hcodes.assign((size_t)ns * CODE, 0.f);        // a 32-D code runs padded with zeros
    for (int c = 0; c < ns; ++c)
      std::memcpy(b->hcodes.data() + (size_t)c * CODE, codes + (size_t)(c0 + c) * L, sizeof(float) * L);
    const int rc = mesh_pass(m, ns, level, sign, E);
    if (rc != 0) return rc;
    const int* r = b->hrb.data();
    const int *ov = r, *of = r + S + 1, *stat = of + S + 1, *cnt = stat + MS_INTS, *serr = cnt + 4,
              *sviol = serr + S, *diag = sviol + 2 * S;
    const int pv = ov[ns], pf = of[ns];
    if (tv + pv > INT_MAX || tf + pf > INT_MAX) return fail(ctx, "mesh batch larger than 2^31 vertices or faces");
    for (int c = 0; c <= ns; ++c) {
      vert_off[c0 + c] = (int)tv + (c < ns ? ov[c] : pv);
      face_off[c0 + c] = (int)tf + (c < ns ? of[c] : pf);
    }
    ++st.n_passes;
    st.all_tiles += ns * m->nt;
    if (sign) {
      st.lite_tiles += ns * b->ntl;
      st.exact_tiles += cnt[2];
      st.audit_tiles += stat[MS_AUDIT_TILES];
      st.redo_tiles += stat[MS_REDO_TILES];
      st.redone_codes += stat[MS_REDO_SLOTS];
      st.lite_broken_blocks += diag[STD_BROKEN];
      for (int c = 0; c < ns; ++c) {
        st.violations += sviol[c];
        float e;
        std::memcpy(&e, &serr[c], sizeof(float));
        st.max_lite_err = std::max(st.max_lite_err, (double)e);
      }
    } else {
      st.exact_tiles += ns * m->nt;
    }
    float ms[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < 3; ++k)
      if (hipEventElapsedTime(&ms[k], b->ev[k], b->ev[k + 1]) != hipSuccess) (void)hipGetLastError();
    st.lite_ms += ms[0];
    st.exact_ms += ms[1];
    st.mc_ms += ms[2];
    // copy-out: a one-pass call straight to the caller once it is known to fit; a call of several
    // passes through host staging, so that nothing is written when a later pass does not fit
    fits = fits && tv + pv <= vcap && tf + pf <= fcap && (tv + pv == 0 || verts) && (tf + pf == 0 || faces);
    if (fits) {
      float* dv = verts;
      int* df = faces;
      if (multi) {
        b->hv.resize((size_t)(tv + pv) * 3);
        b->hf.resize((size_t)(tf + pf) * 3);
        dv = b->hv.data();
        df = b->hf.data();
      }
      if (pv > 0) DSR_CHECK(ctx, hipMemcpy(dv + (size_t)tv * 3, b->verts, sizeof(float) * 3 * pv, hipMemcpyDeviceToHost));
      if (pf > 0) DSR_CHECK(ctx, hipMemcpy(df + (size_t)tf * 3, b->faces, sizeof(int) * 3 * pf, hipMemcpyDeviceToHost));
    }
    tv += pv;
    tf += pf;
  }
  if (!fits) {
    fail(ctx, "meshes larger than the given capacity");
    return -5;
  }
  if (multi) {
    if (tv > 0) std::memcpy(verts, b->hv.data(), sizeof(float) * 3 * (size_t)tv);
    if (tf > 0) std::memcpy(faces, b->hf.data(), sizeof(int) * 3 * (size_t)tf);
  }
  return 0;
}

int dsr_mesher_stats_get(const dsr_mesher* m, dsr_mesher_stats* st) {
  if (!m || !st) return -2;
  *st = m->st;
  return 0;
}

int dsr_mesher_peek(dsr_mesher* m, int slot, float* lite_vol, float* final_vol, unsigned char* tile_flags) {
  if (!m) return -2;
  dsr_ctx* ctx = m->ctx;
  MeshBatch* b = m->mb;
  if (!b || slot < 0 || slot >= b->last_ns) return fail(ctx, "no such slot in the last pass");
  if ((lite_vol || tile_flags) && !b->last_sign) return fail(ctx, "the last pass ran without the sign pass");
  hipSetDevice(ctx->device);
  DSR_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t o = (size_t)slot * b->np;
  if (lite_vol) DSR_CHECK(ctx, hipMemcpy(lite_vol, b->lite + o, sizeof(float) * m->n, hipMemcpyDeviceToHost));
  if (final_vol) DSR_CHECK(ctx, hipMemcpy(final_vol, b->vol + o, sizeof(float) * m->n, hipMemcpyDeviceToHost));
  if (tile_flags) DSR_CHECK(ctx, hipMemcpy(tile_flags, b->tflag + (size_t)slot * m->nt, m->nt, hipMemcpyDeviceToHost));
  return 0;
}

// ---- sphere-traced images (kernels: dsr_render.hpp) ---------------------------
constexpr int RENDER_PASS_OBJ = 64;   // objects per pass at most (bounds the tile padding)

struct dsr_renderer {
  dsr_ctx* ctx = nullptr;
  const dsr_decoder* dec = nullptr;
  dsr_camera cam{};
  int npix = 0, cap = 0;             // W*H; ray slots (2*W*H)
  int max_chunks = 0, max_tiles = 0; // of one pass
  DevArena mem;
  float *lam = nullptr, *lam0 = nullptr, *lam1 = nullptr, *dense = nullptr;
  int* state = nullptr;
  float4* cand = nullptr;            // cap + 64 * RENDER_PASS_OBJ (the normal pass pads tiles per object)
  int *ccnt = nullptr, *gpos = nullptr, *ntiles = nullptr;
  Tile* tiles = nullptr;
  unsigned long long* keys = nullptr;
  float *depth = nullptr, *normals = nullptr, *raw = nullptr;   // normals / raw: on the first normals call
  int* inst = nullptr;
  RenderStepStats* ss = nullptr;
  // per-call arrays, grown on demand
  int obj_cap = 0, chunk_cap = 0;
  RenderObj* objs = nullptr;
  ObjDesc* desc = nullptr;
  float *codes = nullptr, *b0 = nullptr, *b4 = nullptr;
  int *olive = nullptr, *otile = nullptr, *counters = nullptr;
  RayChunk* chunks = nullptr;
  hipEvent_t ev[4] = {};
  dsr_render_stats st{};
};

// One object's pose for the tracer: T_oc = inverse(t_cam_obj) in fp64, rounded once, the ball's
// centre and radius (s = det(R_co)^(1/3)).  false: last row not 0 0 0 1, or det <= 0.
struct RenderPose {
  float Toc[12];
  double c[3], rho;
};
static bool render_pose(const float* t, RenderPose* P) {
  if (t[12] != 0.f || t[13] != 0.f || t[14] != 0.f || t[15] != 1.f) return false;
  double m[9], t3[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) m[i * 3 + j] = t[i * 4 + j];
    t3[i] = t[i * 4 + 3];
  }
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  if (!(det > 0.0) || !std::isfinite(det)) return false;
  const double inv[9] = {c00 / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
                         c01 / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
                         c02 / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) P->Toc[i * 4 + j] = (float)inv[i * 3 + j];
    P->Toc[i * 4 + 3] = (float)(-(inv[i * 3] * t3[0] + inv[i * 3 + 1] * t3[1] + inv[i * 3 + 2] * t3[2]));
    P->c[i] = t3[i];
  }
  P->rho = std::cbrt(det);
  return true;
}

// The rectangle rule (include/dsr.h: dsr_render_layout): rect = u_min, v_min, u_max, v_max.
static int render_rect(const dsr_camera* cam, double near, const RenderPose& P, int* rect) {
  rect[0] = rect[1] = 0;
  rect[2] = rect[3] = -1;
  const double z0 = P.c[2] - P.rho, z1 = P.c[2] + P.rho;
  if (!(z0 >= near)) return DSR_RENDER_SKIP_NEAR;
  const double f[2] = {cam->fx, cam->fy}, pp[2] = {cam->cx, cam->cy};
  const int size[2] = {cam->width, cam->height};
  int lo[2], hi[2];
  for (int a = 0; a < 2; ++a) {
    const double x0 = P.c[a] - P.rho, x1 = P.c[a] + P.rho;
    const double q[4] = {x0 / z0, x0 / z1, x1 / z0, x1 / z1};
    const double mn = std::min(std::min(q[0], q[1]), std::min(q[2], q[3]));
    const double mx = std::max(std::max(q[0], q[1]), std::max(q[2], q[3]));
    const double l = std::floor(pp[a] + f[a] * mn), h = std::ceil(pp[a] + f[a] * mx);
    if (!(l <= size[a] - 1) || !(h >= 0)) return DSR_RENDER_OFFSCREEN;
    lo[a] = (int)std::max(l, 0.0);
    hi[a] = (int)std::min(h, (double)(size[a] - 1));
  }
  rect[0] = lo[0];
  rect[1] = lo[1];
  rect[2] = hi[0];
  rect[3] = hi[1];
  return DSR_RENDER_OK;
}

static const char* camera_error(const dsr_camera* cam) {
  if (cam->width <= 0 || cam->height <= 0) return "image size must be positive";
  if (!(cam->fx > 0.f) || !(cam->fy > 0.f)) return "focal lengths must be positive";
  if ((long long)cam->width * cam->height > (1 << 24)) return "image larger than 2^24 pixels";
  return nullptr;
}

int dsr_render_layout(const dsr_camera* cam, float near, int n_obj, const dsr_render_object* objs, int* rect,
                      int* status) {
  if (!cam || n_obj < 0 || (n_obj > 0 && (!objs || !rect || !status))) return -2;
  if (camera_error(cam)) return -2;
  const double nr = near > 0.f ? near : 0.01f;
  for (int i = 0; i < n_obj; ++i) {
    RenderPose P;
    if (!render_pose(objs[i].t_cam_obj, &P)) return -2;
    status[i] = render_rect(cam, nr, P, rect + 4 * i);
  }
  return 0;
}

int dsr_renderer_destroy(dsr_renderer* r) {
  if (!r) return 0;
  hipSetDevice(r->ctx->device);
  hipStreamSynchronize(r->ctx->stream);
  for (hipEvent_t e : r->ev)
    if (e) hipEventDestroy(e);
  delete r;
  return 0;
}

int dsr_renderer_create(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_camera* cam, dsr_renderer** out) {
  if (!ctx || !dec || !cam || !out) return fail(ctx, "null argument");
  *out = nullptr;
  if (const char* e = camera_error(cam)) return fail(ctx, e);
  if (int rc = decoder_ready(ctx, dec)) return rc;
  hipSetDevice(ctx->device);
  auto* r = new dsr_renderer();
  r->ctx = ctx;
  r->dec = dec;
  r->cam = *cam;
  r->npix = cam->width * cam->height;
  r->cap = 2 * r->npix;
  r->max_chunks = r->cap / RCHUNK + RENDER_PASS_OBJ;
  r->max_tiles = r->cap / TILE + RENDER_PASS_OBJ;
  const size_t cap = (size_t)r->cap;
  DevArena& M = r->mem;
  bool ok = M.alloc(&r->lam, cap) && M.alloc(&r->lam0, cap) && M.alloc(&r->lam1, cap) && M.alloc(&r->dense, cap) &&
            M.alloc(&r->state, cap) && M.alloc(&r->cand, cap + (size_t)TILE * RENDER_PASS_OBJ) &&
            M.alloc(&r->ccnt, r->max_chunks) && M.alloc(&r->gpos, r->max_chunks) && M.alloc(&r->ntiles, 1) &&
            M.alloc(&r->tiles, r->max_tiles) && M.alloc(&r->keys, r->npix) && M.alloc(&r->depth, r->npix) &&
            M.alloc(&r->inst, r->npix) && M.alloc(&r->ss, 1);
  for (hipEvent_t& e : r->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    dsr_renderer_destroy(r);
    return fail(ctx, "hipMalloc failed (renderer)");
  }
  *out = r;
  return 0;
}

int dsr_renderer_stats_get(const dsr_renderer* r, dsr_render_stats* st) {
  if (!r || !st) return -2;
  *st = r->st;
  return 0;
}

int dsr_renderer_render(dsr_renderer* r, const dsr_render_params* params, int n_obj, const dsr_render_object* in,
                        float* depth, int* instance, float* normals, dsr_render_object_out* per_obj) {
  if (!r) return -2;
  dsr_ctx* ctx = r->ctx;
  if (!params || !depth || !instance || (n_obj > 0 && !in)) return fail(ctx, "null argument");
  if (n_obj < 0) return fail(ctx, "n_obj must be >= 0");
  const float hit_eps = params->hit_eps == 0.f ? 1e-4f : params->hit_eps;
  const int max_steps = params->max_steps == 0 ? 48 : params->max_steps;
  const float damp = params->damp == 0.f ? 1.f : params->damp;
  const float near = params->near == 0.f ? 0.01f : params->near;
  if (!(hit_eps > 0.f)) return fail(ctx, "hit_eps must be > 0");
  if (max_steps < 1 || max_steps > 256) return fail(ctx, "max_steps must be in [1, 256]");
  if (!(near > 0.f)) return fail(ctx, "near must be > 0");
  if (!std::isfinite(damp)) return fail(ctx, "damp must be finite");
  const bool want_n = params->normals != 0;
  if (want_n && !normals) return fail(ctx, "null argument (normals requested)");
  for (int i = 0; i < n_obj; ++i)
    if (!in[i].code) return fail(ctx, "null argument (code)");
  if (int rc = decoder_ready(ctx, r->dec)) return rc;
  const dsr_decoder* dec = r->dec;
  const DevDecoder& D = dec->D;
  const RenderCam C{r->cam.fx, r->cam.fy, r->cam.cx, r->cam.cy, r->cam.width, r->cam.height};
  const int npix = r->npix;

  // ---- host layout: poses, rectangles, passes, chunks
  std::vector<RenderObj> ho(n_obj);
  std::vector<ObjDesc> hd(n_obj);
  std::vector<int> status(n_obj), rects((size_t)4 * n_obj);
  std::vector<float> hz((size_t)n_obj * CODE, 0.f);
  std::vector<RayChunk> hc;
  struct Pass { int obj0, n_obj, chunk0, n_chunk, n_tiles_max; };
  std::vector<Pass> passes;
  // objects per pass: RENDER_PASS_OBJ, or DSR_RENDER_PASS_OBJ (1..64) under DSR_TEST_HOOKS=1
  const int pass_obj = hook_int("DSR_RENDER_PASS_OBJ", RENDER_PASS_OBJ, 1, RENDER_PASS_OBJ);
  {
    Pass cur{0, 0, 0, 0, 0};
    int used = 0;
    for (int i = 0; i < n_obj; ++i) {
      RenderPose P;
      if (!render_pose(in[i].t_cam_obj, &P))
        return fail(ctx, "t_cam_obj must have the last row 0 0 0 1 and a positive determinant (object " + std::to_string(i) + ")");
      int* rc = &rects[(size_t)4 * i];
      status[i] = render_rect(&r->cam, near, P, rc);
      RenderObj& o = ho[i];
      std::memcpy(o.Toc, P.Toc, sizeof(o.Toc));
      o.u0 = rc[0];
      o.v0 = rc[1];
      o.w = rc[2] - rc[0] + 1;
      o.h = rc[3] - rc[1] + 1;
      const int area = o.w * o.h;                     // 0 for skipped / off-screen objects; <= W*H
      if (cur.n_obj > 0 && (used + area > r->cap || cur.n_obj >= pass_obj)) {
        passes.push_back(cur);
        cur = Pass{i, 0, (int)hc.size(), 0, 0};
        used = 0;
      }
      o.ray_off = used;
      o.chunk0 = (int)hc.size();
      o.nchunk = (area + RCHUNK - 1) / RCHUNK;
      o.pad = 0;
      for (int c = 0; c < o.nchunk; ++c) hc.push_back(RayChunk{i, c * RCHUNK});
      hd[i] = ObjDesc{};
      hd[i].cand_off = used;
      hd[i].ray_off = used;
      hd[i].n_rays = area;
      used += area;
      cur.n_obj += 1;
      cur.n_chunk += o.nchunk;
      cur.n_tiles_max += (area + TILE - 1) / TILE;
      std::memcpy(&hz[(size_t)i * CODE], in[i].code, sizeof(float) * dec->code_len);   // a 32-D code: zero-padded
    }
    if (cur.n_obj > 0) passes.push_back(cur);
  }
  const int n_chunk = (int)hc.size();

  hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  // the uploads below read the host vectors above asynchronously: no return, an error's
  // included, leaves this frame before the stream has drained
  struct Drain {
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{s};
  float* lnw = nullptr;          // LayerNorm decoders: the context stream's Jacobian workspace
  if (int rc = decoder_ready(ctx, dec, want_n, &lnw)) return rc;
  // ---- per-call device arrays
  if (n_obj > r->obj_cap) {
    for (void* p : {(void*)r->objs, (void*)r->desc, (void*)r->codes, (void*)r->b0, (void*)r->b4, (void*)r->olive,
                    (void*)r->otile, (void*)r->counters})
      r->mem.release(p);
    r->objs = nullptr; r->desc = nullptr; r->codes = r->b0 = r->b4 = nullptr; r->olive = r->otile = r->counters = nullptr;
    r->obj_cap = 0;
    const size_t n = (size_t)std::max(n_obj, 16);
    DevArena& M = r->mem;
    if (!M.alloc(&r->objs, n) || !M.alloc(&r->desc, n) || !M.alloc(&r->codes, CODE * n) || !M.alloc(&r->b0, HID * n) ||
        !M.alloc(&r->b4, HID * n) || !M.alloc(&r->olive, n) || !M.alloc(&r->otile, n) ||
        !M.alloc(&r->counters, RC_INTS * n))
      return fail(ctx, "hipMalloc failed (render objects)");
    r->obj_cap = (int)n;
  }
  if (n_chunk > r->chunk_cap) {
    r->mem.release(r->chunks);
    r->chunks = nullptr;
    r->chunk_cap = 0;
    const size_t n = (size_t)std::max(n_chunk, 64);
    if (!r->mem.alloc(&r->chunks, n)) return fail(ctx, "hipMalloc failed (render chunks)");
    r->chunk_cap = (int)n;
  }
  if (want_n && !r->raw) {
    const size_t np = (size_t)npix + (size_t)TILE * RENDER_PASS_OBJ;
    if (!r->mem.alloc(&r->normals, 3 * (size_t)npix) || !r->mem.alloc(&r->raw, (IN + 1) * np)) {
      r->raw = nullptr;
      return fail(ctx, "hipMalloc failed (render normals)");
    }
  }
  DSR_CHECK(ctx, hipMemsetAsync(r->keys, 0xff, sizeof(unsigned long long) * npix, s));
  DSR_CHECK(ctx, hipMemsetAsync(r->ss, 0, sizeof(RenderStepStats), s));
  if (n_obj > 0) {
    DSR_CHECK(ctx, hipMemcpyAsync(r->objs, ho.data(), sizeof(RenderObj) * n_obj, hipMemcpyHostToDevice, s));
    DSR_CHECK(ctx, hipMemcpyAsync(r->desc, hd.data(), sizeof(ObjDesc) * n_obj, hipMemcpyHostToDevice, s));
    DSR_CHECK(ctx, hipMemcpyAsync(r->codes, hz.data(), sizeof(float) * CODE * n_obj, hipMemcpyHostToDevice, s));
    DSR_CHECK(ctx, hipMemsetAsync(r->counters, 0, sizeof(int) * RC_INTS * n_obj, s));
    if (n_chunk > 0)
      DSR_CHECK(ctx, hipMemcpyAsync(r->chunks, hc.data(), sizeof(RayChunk) * n_chunk, hipMemcpyHostToDevice, s));
    fold_codes(s, D, r->codes, n_obj, r->b0, r->b4);
  }
  dsr_render_stats st{};
  st.n_obj = n_obj;
  // ---- the march, pass by pass: everything enqueued, one synchronisation per pass
  for (const Pass& p : passes) {
    if (p.n_chunk == 0) continue;                       // only objects without rays
    st.n_passes += 1;
    const RayChunk* ch = r->chunks + p.chunk0;
    const int grid = std::max(1, std::min(ctx->n_cu, p.n_tiles_max));
    DSR_CHECK(ctx, hipEventRecord(r->ev[0], s));
    hipLaunchKernelGGL(k_rt_setup, dim3(p.n_chunk), dim3(RCHUNK), 0, s, C, (const RenderObj*)r->objs, ch, r->lam,
                       r->lam0, r->lam1, r->state, r->ccnt);
    DSR_CHECK(ctx, hipEventRecord(r->ev[1], s));
    for (int k = 0; k < max_steps; ++k) {
      hipLaunchKernelGGL(k_rt_scan, dim3(1), dim3(RT_SCAN_THREADS), 0, s, p.n_chunk, p.chunk0, p.obj0, p.n_obj,
                         (const RenderObj*)r->objs, (const int*)r->ccnt, r->gpos, r->olive, r->otile, r->ntiles, k,
                         r->ss, r->counters);
      hipLaunchKernelGGL(k_rt_emit, dim3(p.n_chunk), dim3(RCHUNK), 0, s, C, (const RenderObj*)r->objs, ch, p.chunk0,
                         (const int*)r->gpos, (const int*)r->olive, (const int*)r->otile, (const int*)r->state,
                         (const float*)r->lam, r->cand, r->tiles, 0);
      launch_fwd(s, grid, D, {r->tiles, r->ntiles, r->desc, r->cand, r->b0, r->b4, r->dense});
      hipLaunchKernelGGL(k_rt_advance, dim3(p.n_chunk), dim3(RCHUNK), 0, s, C, (const RenderObj*)r->objs, ch,
                         (const float*)r->dense, r->lam, (const float*)r->lam0, (const float*)r->lam1, r->state,
                         r->keys, r->counters, r->ccnt, RenderMarch{hit_eps, damp, k == max_steps - 1});
    }
    DSR_CHECK(ctx, hipEventRecord(r->ev[2], s));
    DSR_CHECK(ctx, hipGetLastError());
    DSR_CHECK(ctx, hipStreamSynchronize(s));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r->ev[0], r->ev[1]) == hipSuccess) st.setup_ms += ms;
    if (hipEventElapsedTime(&ms, r->ev[1], r->ev[2]) == hipSuccess) st.march_ms += ms;
  }
  // ---- resolve, n_visible, normals
  DSR_CHECK(ctx, hipEventRecord(r->ev[0], s));
  hipLaunchKernelGGL(k_rt_resolve, dim3((npix + 255) / 256), dim3(256), 0, s, (const unsigned long long*)r->keys, npix,
                     r->depth, r->inst);
  if (n_chunk > 0)
    hipLaunchKernelGGL(k_rt_visible, dim3(n_chunk), dim3(RCHUNK), 0, s, C, (const RenderObj*)r->objs,
                       (const RayChunk*)r->chunks, (const int*)r->inst, r->counters);
  if (want_n) {
    DSR_CHECK(ctx, hipMemsetAsync(r->normals, 0, sizeof(float) * 3 * npix, s));
    JacQuery jq{r->tiles, r->ntiles, r->desc, r->b0, r->b4};
    jq.query_pts = r->cand;
    jq.raw_out = r->raw;
    jq.lnw = lnw;
    for (const Pass& p : passes) {
      if (p.n_chunk == 0) continue;
      const RayChunk* ch = r->chunks + p.chunk0;
      const int grid = std::max(1, std::min(ctx->n_cu, p.n_tiles_max));
      hipLaunchKernelGGL(k_rt_winners, dim3(p.n_chunk), dim3(RCHUNK), 0, s, C, (const RenderObj*)r->objs, ch,
                         (const unsigned long long*)r->keys, r->lam, r->state, r->ccnt);
      hipLaunchKernelGGL(k_rt_scan, dim3(1), dim3(RT_SCAN_THREADS), 0, s, p.n_chunk, p.chunk0, p.obj0, p.n_obj,
                         (const RenderObj*)r->objs, (const int*)r->ccnt, r->gpos, r->olive, r->otile, r->ntiles, -1,
                         r->ss, r->counters);
      hipLaunchKernelGGL(k_rt_emit, dim3(p.n_chunk), dim3(RCHUNK), 0, s, C, (const RenderObj*)r->objs, ch, p.chunk0,
                         (const int*)r->gpos, (const int*)r->olive, (const int*)r->otile, (const int*)r->state,
                         (const float*)r->lam, r->cand, r->tiles, 1);
      launch_jac(s, grid, D, jq);
      hipLaunchKernelGGL(k_rt_normals, dim3(grid), dim3(TILE), 0, s, C, (const RenderObj*)r->objs,
                         (const Tile*)r->tiles, (const int*)r->ntiles, (const float4*)r->cand, (const float*)r->raw,
                         r->normals);
    }
  }
  DSR_CHECK(ctx, hipEventRecord(r->ev[1], s));
  DSR_CHECK(ctx, hipGetLastError());
  DSR_CHECK(ctx, hipStreamSynchronize(s));
  // (blocking copies after the synchronise: an error return never leaves a copy in flight to
  // the caller's buffers or to this frame)
  DSR_CHECK(ctx, hipMemcpy(depth, r->depth, sizeof(float) * npix, hipMemcpyDeviceToHost));
  DSR_CHECK(ctx, hipMemcpy(instance, r->inst, sizeof(int) * npix, hipMemcpyDeviceToHost));
  if (want_n) DSR_CHECK(ctx, hipMemcpy(normals, r->normals, sizeof(float) * 3 * npix, hipMemcpyDeviceToHost));
  std::vector<int> hcnt((size_t)RC_INTS * std::max(n_obj, 1), 0);
  RenderStepStats hss{};
  if (n_obj > 0)
    DSR_CHECK(ctx, hipMemcpy(hcnt.data(), r->counters, sizeof(int) * RC_INTS * n_obj, hipMemcpyDeviceToHost));
  DSR_CHECK(ctx, hipMemcpy(&hss, r->ss, sizeof(hss), hipMemcpyDeviceToHost));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, r->ev[0], r->ev[1]) == hipSuccess) st.resolve_ms = ms;
  st.steps_run = hss.steps_run;
  st.decoded = hss.decoded;
  st.max_live_last = hss.max_live_last;
  r->st = st;
  if (per_obj)
    for (int i = 0; i < n_obj; ++i) {
      dsr_render_object_out& o = per_obj[i];
      o.status = status[i];
      std::memcpy(o.rect, &rects[(size_t)4 * i], sizeof(o.rect));
      o.n_rays = ho[i].w * ho[i].h;
      o.n_ball = hcnt[(size_t)i * RC_INTS + RC_BALL];
      o.n_hit = hcnt[(size_t)i * RC_INTS + RC_HIT];
      o.n_unconverged = hcnt[(size_t)i * RC_INTS + RC_UNCONV];
      o.n_visible = hcnt[(size_t)i * RC_INTS + RC_VISIBLE];
    }
  return 0;
}

// ---- scene SDF queries (kernels: dsr_scene.hpp) -------------------------------
constexpr int SCENE_PASS_OBJ = 64;                    // objects per pass at most (bounds the tile padding)
constexpr size_t SCENE_MIN_PAIRS = (size_t)1 << 22;   // pair slots of the pass buffers at least
constexpr int SCENE_MAX_PTS = 1 << 24;

struct dsr_scene {
  dsr_ctx* ctx = nullptr;
  const dsr_decoder* dec = nullptr;
  int max_obj = 0, max_pts = 0;
  size_t cap = 0;                    // pair slots: max(max_pts, SCENE_MIN_PAIRS)
  int max_chunks = 0, max_tiles = 0; // of one pass
  DevArena mem;
  // per object (max_obj)
  SceneObj* objs = nullptr;
  ObjDesc* desc = nullptr;
  float *codes = nullptr, *b0 = nullptr, *b4 = nullptr;
  int *ocount = nullptr, *otile = nullptr, *wcount = nullptr, *wtile = nullptr, *nwin = nullptr;
  SceneSums* sums = nullptr;
  // per point (max_pts)
  float* pts = nullptr;
  unsigned long long* keys = nullptr;
  float* dist = nullptr;
  int* obj = nullptr;
  // per pass
  float4* cand = nullptr;
  float* dense = nullptr;
  int *ccnt = nullptr, *gpos = nullptr, *ntiles = nullptr;
  Tile* tiles = nullptr;
  ScenePart* part = nullptr;
  // gradient: allocated at the first query that asks for it
  float *grad = nullptr, *raw = nullptr;
  float4* gcand = nullptr;           // max_pts + 64 * SCENE_PASS_OBJ (tiles padded per object)
  hipEvent_t ev[4] = {};
  std::vector<SceneObj> hobjs;       // the objects of dsr_scene_set_objects
  std::vector<ObjDesc> hdesc;
  int n_obj = -1;                    // -1: before dsr_scene_set_objects
  int q_obj = -1, q_pts = 0;         // the last query's objects and points (-1: none)
  int held0 = 0, held_k = 0;         // the objects whose candidates the pass buffers hold
  std::vector<int> q_in;             // the last query's n_in
  dsr_scene_stats st{};
  // association (dsr_scene_associate_*, §3.6d): allocated at the first call that needs them
  float* arows = nullptr;            // camera-frame rows, max_pts x 3
  dsr_batch::IngestBlock aframe;     // a frame call's block (frame_carve): it grows
  dsr_batch::IngestBlock ablock;     // counts, descriptors, rows, tables and records (assoc_layout): it grows
  hipEvent_t a_ev = nullptr;         // recorded after a call's last copy
};

// One object's pose for the query: T_ow = inverse(t_world_obj) in fp64 (adjugate / determinant, as
// render_pose), rounded once; s = det(R)^(1/3) rounded once.  false: a non-finite entry, a last
// row that is not 0 0 0 1, or det <= 0.
static bool scene_pose(const float* t, SceneObj* o) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(t[i])) return false;
  RenderPose P;
  if (!render_pose(t, &P)) return false;
  std::memcpy(o->T, P.Toc, sizeof(o->T));
  o->s = (float)P.rho;
  o->pad[0] = o->pad[1] = o->pad[2] = 0;
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(o->T[i])) return false;
  return std::isfinite(o->s) && o->s > 0.f;
}

// the pair rule on the host: the same fused operations as sc_point / sc_in_ball (dsr_scene.hpp)
static bool scene_pair_host(const SceneObj& o, const float* p, float* x) {
  for (int k = 0; k < 3; ++k)
    x[k] = std::fmaf(o.T[k * 4], p[0], std::fmaf(o.T[k * 4 + 1], p[1], std::fmaf(o.T[k * 4 + 2], p[2], o.T[k * 4 + 3])));
  const float r2 = std::fmaf(x[0], x[0], std::fmaf(x[1], x[1], x[2] * x[2]));
  return r2 < 1.0f;
}

int dsr_scene_bin_host(int n_obj, const dsr_scene_object* objs, int n_pts, const float* pts_world, int obj,
                       int cap, int* idx, float* x_obj, int* n_in, float* scale) {
  if (n_obj <= 0 || !objs || n_pts < 0 || (n_pts > 0 && !pts_world) || obj < 0 || obj >= n_obj || cap < 0) return -2;
  SceneObj o;
  for (int i = 0; i < n_obj; ++i)
    if (!scene_pose(objs[i].t_world_obj, &o)) return -2;
  scene_pose(objs[obj].t_world_obj, &o);
  if (scale) *scale = o.s;
  int n = 0;
  for (int p = 0; p < n_pts; ++p) {
    float x[3];
    if (scene_pair_host(o, pts_world + (size_t)p * 3, x)) n += 1;
  }
  if (n_in) *n_in = n;
  if (n > cap) return -5;
  n = 0;
  for (int p = 0; p < n_pts; ++p) {
    float x[3];
    if (!scene_pair_host(o, pts_world + (size_t)p * 3, x)) continue;
    if (idx) idx[n] = p;
    if (x_obj) std::memcpy(x_obj + (size_t)n * 3, x, sizeof(x));
    n += 1;
  }
  return 0;
}

int dsr_scene_destroy(dsr_scene* sc) {
  if (!sc) return 0;
  hipSetDevice(sc->ctx->device);
  hipStreamSynchronize(sc->ctx->stream);
  for (hipEvent_t e : sc->ev)
    if (e) hipEventDestroy(e);
  if (sc->a_ev) hipEventDestroy(sc->a_ev);
  for (dsr_batch::IngestBlock* g : {&sc->aframe, &sc->ablock}) {
    if (g->host) hipHostFree(g->host);
    if (g->dev) hipFree(g->dev);
  }
  delete sc;
  return 0;
}

int dsr_scene_create(dsr_ctx* ctx, const dsr_decoder* dec, int max_obj, int max_pts, dsr_scene** out) {
  if (!ctx || !dec || !out) return fail(ctx, "null argument");
  *out = nullptr;
  if (max_obj < 1) return fail(ctx, "max_obj must be >= 1");
  if (max_pts < 1 || max_pts > SCENE_MAX_PTS) return fail(ctx, "max_pts must be in [1, 2^24]");
  if (int rc = decoder_ready(ctx, dec)) return rc;
  hipSetDevice(ctx->device);
  auto* sc = new dsr_scene();
  sc->ctx = ctx;
  sc->dec = dec;
  sc->max_obj = max_obj;
  sc->max_pts = max_pts;
  sc->cap = std::max((size_t)max_pts, SCENE_MIN_PAIRS);
  sc->max_chunks = (int)(sc->cap / SCHUNK) + SCENE_PASS_OBJ;
  sc->max_tiles = (int)(sc->cap / TILE) + SCENE_PASS_OBJ;
  sc->hdesc.assign(max_obj, ObjDesc{});
  const size_t no = (size_t)max_obj, np = (size_t)max_pts, cap = sc->cap;
  DevArena& M = sc->mem;
  bool ok = M.alloc(&sc->objs, no) && M.alloc(&sc->desc, no) && M.alloc(&sc->codes, CODE * no) &&
            M.alloc(&sc->b0, HID * no) && M.alloc(&sc->b4, HID * no) && M.alloc(&sc->ocount, no) &&
            M.alloc(&sc->otile, no) && M.alloc(&sc->wcount, no) && M.alloc(&sc->wtile, no) && M.alloc(&sc->nwin, no) &&
            M.alloc(&sc->sums, no) && M.alloc(&sc->pts, 3 * np) && M.alloc(&sc->keys, np) && M.alloc(&sc->dist, np) &&
            M.alloc(&sc->obj, np) && M.alloc(&sc->cand, cap) && M.alloc(&sc->dense, cap) &&
            M.alloc(&sc->ccnt, sc->max_chunks) && M.alloc(&sc->gpos, sc->max_chunks) && M.alloc(&sc->ntiles, 1) &&
            M.alloc(&sc->tiles, sc->max_tiles) && M.alloc(&sc->part, sc->max_tiles);
  for (hipEvent_t& e : sc->ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    dsr_scene_destroy(sc);
    return fail(ctx, "hipMalloc failed (scene)");
  }
  *out = sc;
  return 0;
}

int dsr_scene_stats_get(const dsr_scene* sc, dsr_scene_stats* st) {
  if (!sc || !st) return -2;
  *st = sc->st;
  return 0;
}

int dsr_scene_set_objects(dsr_scene* sc, int n_obj, const dsr_scene_object* in) {
  if (!sc) return -2;
  dsr_ctx* ctx = sc->ctx;
  if (n_obj > 0 && !in) return fail(ctx, "null argument");
  if (n_obj < 0 || n_obj > sc->max_obj) return fail(ctx, "n_obj must be in [0, max_obj]");
  const dsr_decoder* dec = sc->dec;
  std::vector<SceneObj> ho(n_obj);
  std::vector<float> hz((size_t)n_obj * CODE, 0.f);
  for (int i = 0; i < n_obj; ++i) {
    if (!in[i].code) return fail(ctx, "null argument (code)");
    if (!scene_pose(in[i].t_world_obj, &ho[i]))
      return fail(ctx, "t_world_obj must be finite with the last row 0 0 0 1 and a positive determinant (object " +
                           std::to_string(i) + ")");
    for (int k = 0; k < dec->code_len; ++k)
      if (!std::isfinite(in[i].code[k])) return fail(ctx, "code must be finite (object " + std::to_string(i) + ")");
    std::memcpy(&hz[(size_t)i * CODE], in[i].code, sizeof(float) * dec->code_len);   // a 32-D code: zero-padded
  }
  if (int rc = decoder_ready(ctx, dec)) return rc;
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  sc->n_obj = -1;                    // (an error below leaves no half-uploaded map behind)
  sc->q_obj = -1;
  if (n_obj > 0) {
    DSR_CHECK(ctx, hipMemcpy(sc->objs, ho.data(), sizeof(SceneObj) * n_obj, hipMemcpyHostToDevice));
    DSR_CHECK(ctx, hipMemcpy(sc->codes, hz.data(), sizeof(float) * CODE * n_obj, hipMemcpyHostToDevice));
    fold_codes(s, dec->D, sc->codes, n_obj, sc->b0, sc->b4);
    DSR_CHECK(ctx, hipGetLastError());
    DSR_CHECK(ctx, hipStreamSynchronize(s));
  }
  sc->hobjs = std::move(ho);
  sc->n_obj = n_obj;
  return 0;
}

// The value pass of objects obj0 .. obj0 + k - 1 over the resident points, enqueued: bin, scan,
// emit, the exact decode and (composite) the min and the per-object sums.  The caller has set
// desc[obj].cand_off = (obj - obj0) * n_pts.  timing: events around the three stages.
static int scene_value_pass(dsr_scene* sc, int obj0, int k, int n_pts, bool composite, bool timing) {
  dsr_ctx* ctx = sc->ctx;
  hipStream_t s = ctx->stream;
  const DevDecoder& D = sc->dec->D;
  const int nc = (n_pts + SCHUNK - 1) / SCHUNK, n_chunk = k * nc;
  const int grid = std::max(1, std::min(ctx->n_cu, k * ((n_pts + TILE - 1) / TILE)));
  if (timing) DSR_CHECK(ctx, hipEventRecord(sc->ev[0], s));
  hipLaunchKernelGGL(k_sc_bin, dim3(n_chunk), dim3(SCHUNK), 0, s, obj0, nc, n_pts, (const SceneObj*)sc->objs,
                     (const float*)sc->pts, sc->ccnt);
  hipLaunchKernelGGL(k_sc_scan, dim3(1), dim3(RT_SCAN_THREADS), 0, s, n_chunk, nc, obj0, k, (const int*)sc->ccnt,
                     sc->gpos, sc->ocount, sc->otile, sc->ntiles);
  hipLaunchKernelGGL(k_sc_emit, dim3(n_chunk), dim3(SCHUNK), 0, s, obj0, nc, n_pts, (const SceneObj*)sc->objs,
                     (const float*)sc->pts, (const unsigned long long*)sc->keys, (const int*)sc->gpos,
                     (const int*)sc->ocount, (const int*)sc->otile, sc->cand, sc->tiles, 0);
  if (timing) DSR_CHECK(ctx, hipEventRecord(sc->ev[1], s));
  launch_fwd(s, grid, D, {sc->tiles, sc->ntiles, sc->desc, sc->cand, sc->b0, sc->b4, sc->dense});
  if (timing) DSR_CHECK(ctx, hipEventRecord(sc->ev[2], s));
  if (composite) {
    hipLaunchKernelGGL(k_sc_min, dim3(grid), dim3(TILE), 0, s, (const SceneObj*)sc->objs, (const ObjDesc*)sc->desc,
                       (const Tile*)sc->tiles, (const int*)sc->ntiles, (const float4*)sc->cand, (const float*)sc->dense,
                       sc->keys, sc->part);
    hipLaunchKernelGGL(k_sc_sums, dim3(k), dim3(64), 0, s, obj0, (const int*)sc->ocount, (const int*)sc->otile,
                       (const ScenePart*)sc->part, sc->sums);
  }
  if (timing) DSR_CHECK(ctx, hipEventRecord(sc->ev[3], s));
  DSR_CHECK(ctx, hipGetLastError());
  sc->held0 = obj0;
  sc->held_k = k;
  return 0;
}

int dsr_scene_query(dsr_scene* sc, int n_pts, const float* pts_world, float* dist, int* obj, float* grad,
                    dsr_scene_object_out* per_obj) {
  if (!sc) return -2;
  dsr_ctx* ctx = sc->ctx;
  if (n_pts < 0 || n_pts > sc->max_pts) return fail(ctx, "n_pts must be in [0, max_pts]");
  if (n_pts > 0 && (!pts_world || !dist || !obj)) return fail(ctx, "null argument");
  if (sc->n_obj < 0) return fail(ctx, "dsr_scene_query before dsr_scene_set_objects");
  if (int rc = decoder_ready(ctx, sc->dec)) return rc;
  const int n_obj = sc->n_obj;
  const DevDecoder& D = sc->dec->D;
  dsr_scene_stats st{};
  st.n_obj = n_obj;
  st.n_pts = n_pts;
  st.pairs = (long long)n_obj * n_pts;
  sc->q_obj = -1;
  sc->held_k = 0;
  sc->q_in.assign(n_obj, 0);
  if (per_obj)
    for (int i = 0; i < n_obj; ++i) per_obj[i] = dsr_scene_object_out{};
  if (n_obj == 0 || n_pts == 0) {      // nothing to decode: +inf, -1 and zeros
    for (int p = 0; p < n_pts; ++p) {
      dist[p] = INFINITY;
      obj[p] = -1;
      if (grad) grad[p * 3] = grad[p * 3 + 1] = grad[p * 3 + 2] = 0.f;
    }
    sc->st = st;
    sc->q_obj = n_obj;
    sc->q_pts = n_pts;
    return 0;
  }
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  float* lnw = nullptr;          // LayerNorm decoders: the context stream's Jacobian workspace
  if (int rc = decoder_ready(ctx, sc->dec, grad != nullptr, &lnw)) return rc;
  if (grad && !sc->raw) {
    const size_t np = (size_t)sc->max_pts + (size_t)TILE * SCENE_PASS_OBJ;
    if (!sc->mem.alloc(&sc->grad, 3 * (size_t)sc->max_pts) || !sc->mem.alloc(&sc->gcand, np) ||
        !sc->mem.alloc(&sc->raw, (IN + 1) * np)) {
      sc->raw = nullptr;
      return fail(ctx, "hipMalloc failed (scene gradient)");
    }
  }
  // ---- passes: objects in input order, the largest k <= 64 with k * n_pts pairs in the buffers
  // (SCENE_PASS_OBJ, or DSR_SCENE_PASS_OBJ (1..64) under DSR_TEST_HOOKS=1)
  const size_t pass_obj = hook_int("DSR_SCENE_PASS_OBJ", SCENE_PASS_OBJ, 1, SCENE_PASS_OBJ);
  const int k_pass = (int)std::min(pass_obj, sc->cap / (size_t)n_pts);
  for (int i = 0; i < n_obj; ++i) {
    sc->hdesc[i] = ObjDesc{};
    sc->hdesc[i].cand_off = (i % k_pass) * n_pts;
  }
  DSR_CHECK(ctx, hipMemcpy(sc->pts, pts_world, sizeof(float) * 3 * n_pts, hipMemcpyHostToDevice));
  DSR_CHECK(ctx, hipMemcpy(sc->desc, sc->hdesc.data(), sizeof(ObjDesc) * n_obj, hipMemcpyHostToDevice));
  DSR_CHECK(ctx, hipMemsetAsync(sc->keys, 0xff, sizeof(unsigned long long) * n_pts, s));
  DSR_CHECK(ctx, hipMemsetAsync(sc->nwin, 0, sizeof(int) * n_obj, s));
  for (int o0 = 0; o0 < n_obj; o0 += k_pass) {
    const int k = std::min(k_pass, n_obj - o0);
    st.n_passes += 1;
    if (int rc = scene_value_pass(sc, o0, k, n_pts, true, true)) return rc;
    DSR_CHECK(ctx, hipStreamSynchronize(s));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, sc->ev[0], sc->ev[1]) == hipSuccess) st.bin_ms += ms;
    if (hipEventElapsedTime(&ms, sc->ev[1], sc->ev[2]) == hipSuccess) st.decode_ms += ms;
    if (hipEventElapsedTime(&ms, sc->ev[2], sc->ev[3]) == hipSuccess) st.resolve_ms += ms;
  }
  // ---- resolve, n_win, the gradient at the winners
  const int nc = (n_pts + SCHUNK - 1) / SCHUNK;
  DSR_CHECK(ctx, hipEventRecord(sc->ev[0], s));
  hipLaunchKernelGGL(k_sc_resolve, dim3((n_pts + 255) / 256), dim3(256), 0, s, (const unsigned long long*)sc->keys, n_pts,
                     sc->dist, sc->obj);
  if (grad) DSR_CHECK(ctx, hipMemsetAsync(sc->grad, 0, sizeof(float) * 3 * n_pts, s));
  DSR_CHECK(ctx, hipEventRecord(sc->ev[1], s));
  JacQuery jq{sc->tiles, sc->ntiles, sc->desc, sc->b0, sc->b4};
  jq.query_pts = sc->gcand;
  jq.raw_out = sc->raw;
  jq.lnw = lnw;
  for (int o0 = 0; o0 < n_obj; o0 += k_pass) {
    const int k = std::min(k_pass, n_obj - o0);
    hipLaunchKernelGGL(k_sc_winners, dim3(k * nc), dim3(SCHUNK), 0, s, o0, nc, n_pts, (const unsigned long long*)sc->keys,
                       sc->ccnt, sc->nwin);
    if (!grad) continue;
    const int grid = std::max(1, std::min(ctx->n_cu, (n_pts + TILE - 1) / TILE + k));
    hipLaunchKernelGGL(k_sc_scan, dim3(1), dim3(RT_SCAN_THREADS), 0, s, k * nc, nc, o0, k, (const int*)sc->ccnt, sc->gpos,
                       sc->wcount, sc->wtile, sc->ntiles);
    hipLaunchKernelGGL(k_sc_emit, dim3(k * nc), dim3(SCHUNK), 0, s, o0, nc, n_pts, (const SceneObj*)sc->objs,
                       (const float*)sc->pts, (const unsigned long long*)sc->keys, (const int*)sc->gpos,
                       (const int*)sc->wcount, (const int*)sc->wtile, sc->gcand, sc->tiles, 1);
    launch_jac(s, grid, D, jq);
    hipLaunchKernelGGL(k_sc_grad, dim3(grid), dim3(TILE), 0, s, (const SceneObj*)sc->objs, (const Tile*)sc->tiles,
                       (const int*)sc->ntiles, (const float4*)sc->gcand, (const float*)sc->raw, sc->grad);
  }
  DSR_CHECK(ctx, hipEventRecord(sc->ev[2], s));
  DSR_CHECK(ctx, hipGetLastError());
  DSR_CHECK(ctx, hipStreamSynchronize(s));
  // (blocking copies after the synchronise: an error return never leaves a copy in flight)
  DSR_CHECK(ctx, hipMemcpy(dist, sc->dist, sizeof(float) * n_pts, hipMemcpyDeviceToHost));
  DSR_CHECK(ctx, hipMemcpy(obj, sc->obj, sizeof(int) * n_pts, hipMemcpyDeviceToHost));
  if (grad) DSR_CHECK(ctx, hipMemcpy(grad, sc->grad, sizeof(float) * 3 * n_pts, hipMemcpyDeviceToHost));
  std::vector<int> hwin(n_obj);
  std::vector<SceneSums> hs(n_obj);
  DSR_CHECK(ctx, hipMemcpy(sc->q_in.data(), sc->ocount, sizeof(int) * n_obj, hipMemcpyDeviceToHost));
  DSR_CHECK(ctx, hipMemcpy(hwin.data(), sc->nwin, sizeof(int) * n_obj, hipMemcpyDeviceToHost));
  DSR_CHECK(ctx, hipMemcpy(hs.data(), sc->sums, sizeof(SceneSums) * n_obj, hipMemcpyDeviceToHost));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, sc->ev[0], sc->ev[1]) == hipSuccess) st.resolve_ms += ms;
  if (hipEventElapsedTime(&ms, sc->ev[1], sc->ev[2]) == hipSuccess) (grad ? st.grad_ms : st.resolve_ms) += ms;
  for (int i = 0; i < n_obj; ++i) {
    st.decoded += sc->q_in[i];
    st.winners += hwin[i];
    if (per_obj) per_obj[i] = dsr_scene_object_out{sc->q_in[i], hwin[i], hs[i].n_neg, hs[i].n_nan, hs[i].sum, hs[i].sum_abs};
  }
  sc->st = st;
  sc->q_obj = n_obj;
  sc->q_pts = n_pts;
  return 0;
}

int dsr_scene_peek(dsr_scene* sc, int obj, int cap, int* idx, float* x_obj, float* sdf, int* n) {
  if (!sc) return -2;
  dsr_ctx* ctx = sc->ctx;
  if (!n || cap < 0) return fail(ctx, "null argument");
  if (sc->q_obj < 0 || obj < 0 || obj >= sc->q_obj) return fail(ctx, "dsr_scene_peek: object outside the last query");
  const int cnt = sc->q_in[obj], n_pts = sc->q_pts;
  *n = cnt;
  if (cnt > cap) return -5;
  if (cnt == 0) return 0;
  hipSetDevice(ctx->device);
  if (obj < sc->held0 || obj >= sc->held0 + sc->held_k) {
    // an earlier pass's object: its value pass again, alone (the same tiles, so the same values)
    sc->hdesc[obj].cand_off = 0;
    DSR_CHECK(ctx, hipMemcpy(sc->desc + obj, &sc->hdesc[obj], sizeof(ObjDesc), hipMemcpyHostToDevice));
    if (int rc = scene_value_pass(sc, obj, 1, n_pts, false, false)) return rc;
    DSR_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  const size_t off = (size_t)(obj - sc->held0) * n_pts;
  std::vector<float4> hc(cnt);
  std::vector<float> hd(n_pts);
  DSR_CHECK(ctx, hipMemcpy(hc.data(), sc->cand + off, sizeof(float4) * cnt, hipMemcpyDeviceToHost));
  DSR_CHECK(ctx, hipMemcpy(hd.data(), sc->dense + off, sizeof(float) * n_pts, hipMemcpyDeviceToHost));
  for (int j = 0; j < cnt; ++j) {
    int i;
    std::memcpy(&i, &hc[j].w, sizeof(int));
    if (idx) idx[j] = i;
    if (x_obj) {
      x_obj[j * 3] = hc[j].x;
      x_obj[j * 3 + 1] = hc[j].y;
      x_obj[j * 3 + 2] = hc[j].z;
    }
    if (sdf) sdf[j] = hd[i];
  }
  return 0;
}

// ---- data association (kernels and the shared rule: dsr_assoc.hpp) ----------
int dsr_assoc_params_default(dsr_assoc_params* p) {
  if (!p) return -2;
  p->inlier_tol = 0.05f;
  p->min_hits = 20;
  p->min_pct = 50;
  return 0;
}

// what an association reads of the frame parameters (as dsr_tracker_track_frame: no background
// grid, the mask's tight box) and its detections, one per label
static dsr_frame_params assoc_frame_params(const dsr_frame_params* P) {
  return dsr_frame_params{P->max_pts, 0, 1, 0, P->min_mask_area, P->near, P->far};
}
static std::vector<dsr_frame_det> assoc_frame_dets(int n_det, const int* labels) {
  std::vector<dsr_frame_det> dets(n_det > 0 ? n_det : 0);
  for (int j = 0; j < n_det; ++j) {
    dets[j] = dsr_frame_det{};
    dets[j].label = labels[j];
    dets[j].bbox[2] = dets[j].bbox[3] = -1;
  }
  return dets;
}
static bool assoc_rigid(const float* t) {
  float inv[16];
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(t[i])) return false;
  return rigid_inverse(t, inv);
}

int dsr_assoc_points_host(const dsr_camera* cam, const dsr_frame_params* frame_params, const float* t_world_cam,
                          const float* depth, const int* instance, int n_det, const int* labels,
                          float* pts_world, int* n_rows, dsr_frame_det_out* ingest) {
  if (!frame_params || !t_world_cam || !labels || !pts_world || !n_rows || n_det < 1) return -2;
  const dsr_frame_params Q = assoc_frame_params(frame_params);
  const std::vector<dsr_frame_det> dets = assoc_frame_dets(n_det, labels);
  if (frame_args_error(cam, &Q, depth, instance, n_det, dets.data())) return -2;
  if (!assoc_rigid(t_world_cam)) return -2;
  const size_t slots = (size_t)n_det * Q.max_pts;
  std::vector<float> rows(slots * 3, 0.f);
  std::vector<dsr_frame_det_out> recs(n_det);
  frame_inputs_host_impl(frame_cam(cam), Q, depth, instance, n_det, dets.data(), rows.data(), nullptr, nullptr, recs.data());
  const AssocXf X = assoc_xf(t_world_cam);
  for (int j = 0; j < n_det; ++j) {
    n_rows[j] = recs[j].n_pts;
    if (ingest) ingest[j] = recs[j];
    for (int k = 0; k < Q.max_pts; ++k) {
      const size_t p = (size_t)j * Q.max_pts + k;
      float* w = pts_world + p * 3;
      if (k < recs[j].n_pts) assoc_world(X, &rows[p * 3], w);
      else w[0] = w[1] = w[2] = __builtin_nanf("");
    }
  }
  return 0;
}

int dsr_assoc_pick_host(const dsr_assoc_params* assoc_params, int n_det, int n_obj, const int* table,
                        const int* n_rows, dsr_assoc_out* out) {
  if (assoc_params_error(assoc_params) || n_det < 1 || n_obj < 0 || (n_obj > 0 && !table) || !n_rows || !out) return -2;
  for (int j = 0; j < n_det; ++j)
    if (n_rows[j] < 0) return -2;
  const size_t plane = (size_t)n_det * n_obj;
  for (int j = 0; j < n_det; ++j) {
    const int* row = n_obj ? table + (size_t)j * n_obj : nullptr;
    assoc_pick_host_one(*assoc_params, n_obj, row, n_obj ? row + plane : nullptr, n_obj ? row + 2 * plane : nullptr,
                        n_rows[j], out + j);
  }
  return 0;
}

namespace {
struct AssocFrame {                  // a frame call's source: the images, through sc->aframe
  const dsr_camera* cam;
  dsr_frame_params Q;
  const float* depth;
  const int* inst;
  const std::vector<dsr_frame_det>* dets;
};
}  // namespace

// Everything of a call after its refusals.  F != null: the rows are the frame ingest's; else the
// caller's (rows, n_rows).  Every copy and kernel is enqueued on the context stream; the one wait
// of the host is at the end.  (The caller, assoc_run, holds the run lock and drains the stream if
// this returns an error.)
static int assoc_enqueue_wait(dsr_scene* sc, const dsr_assoc_params& A, const float* t_world_cam, int n_det,
                              int max_pts, const AssocFrame* F, const int* n_rows, const float* rows,
                              dsr_assoc_out* out, int* table) {
  dsr_ctx* ctx = sc->ctx;
  hipStream_t s = ctx->stream;
  const int n_obj = sc->n_obj, n_pts = n_det * max_pts;
  sc->q_obj = -1;
  sc->held_k = 0;
  if (!sc->a_ev) DSR_CHECK(ctx, hipEventCreateWithFlags(&sc->a_ev, hipEventDisableTiming));
  if (!sc->arows && !sc->mem.alloc(&sc->arows, 3 * (size_t)sc->max_pts)) {
    sc->arows = nullptr;
    return fail(ctx, "hipMalloc failed (scene association)");
  }
  // ---- staging: counts, descriptors and host rows into the pinned half, the frame into its block
  size_t row_floats = 0;
  if (!F)
    for (int j = n_det - 1; j >= 0 && !row_floats; --j)
      if (n_rows[j] > 0) row_floats = ((size_t)j * max_pts + n_rows[j]) * 3;      // up to the last counted row
  const AssocLayout L = assoc_layout(n_det, n_obj, row_floats);
  if (int rc = ingest_fit(ctx, sc->ablock, sc->a_ev, L.host_bytes, L.dev_bytes)) return rc;
  char* hb = static_cast<char*>(sc->ablock.host);
  char* db = static_cast<char*>(sc->ablock.dev);
  int* d_cnt = reinterpret_cast<int*>(db + L.d_cnt);
  int* d_table = reinterpret_cast<int*>(db + L.d_table);
  dsr_assoc_out* d_recs = reinterpret_cast<dsr_assoc_out*>(db + L.d_recs);
  // passes as dsr_scene_query's: objects in input order, the largest k <= 64 with k * n_pts pairs
  const size_t pass_obj = hook_int("DSR_SCENE_PASS_OBJ", SCENE_PASS_OBJ, 1, SCENE_PASS_OBJ);
  const int k_pass = (int)std::min(pass_obj, sc->cap / (size_t)n_pts);
  ObjDesc* hdesc = reinterpret_cast<ObjDesc*>(hb + L.desc);
  for (int i = 0; i < n_obj; ++i) {
    sc->hdesc[i] = ObjDesc{};
    sc->hdesc[i].cand_off = (i % k_pass) * n_pts;
    hdesc[i] = sc->hdesc[i];
  }
  int* hcnt = reinterpret_cast<int*>(hb + L.cnt);
  for (int j = 0; j < n_det; ++j) hcnt[j] = F ? 0 : n_rows[j];
  const dsr_frame_det_out* d_frecs = nullptr;
  FrameDev FD{};
  size_t fup = 0;
  if (F) {
    const int W = F->cam->width, H = F->cam->height;
    fup = frame_upload_bytes(W, H, n_det);
    if (int rc = ingest_fit(ctx, sc->aframe, sc->a_ev, fup, frame_dev_bytes(W, H, n_det))) return rc;
    frame_pack(sc->aframe.host, F->cam, F->depth, F->inst, n_det, F->dets->data());
    FD = frame_carve(sc->aframe.dev, W, H, n_det);
    d_frecs = FD.recs;
  } else {
    float* hrows = reinterpret_cast<float*>(hb + L.rows);
    for (int j = 0; j < n_det; ++j)
      if (n_rows[j] > 0)
        std::memcpy(hrows + (size_t)j * max_pts * 3, rows + (size_t)j * max_pts * 3, sizeof(float) * 3 * n_rows[j]);
  }
  // ---- uploads
  DSR_CHECK(ctx, hipMemcpyAsync(d_cnt, hcnt, sizeof(int) * n_det, hipMemcpyHostToDevice, s));
  if (n_obj > 0) DSR_CHECK(ctx, hipMemcpyAsync(sc->desc, hdesc, sizeof(ObjDesc) * n_obj, hipMemcpyHostToDevice, s));
  if (row_floats)
    DSR_CHECK(ctx, hipMemcpyAsync(sc->arows, hb + L.rows, sizeof(float) * row_floats, hipMemcpyHostToDevice, s));
  if (F) DSR_CHECK(ctx, hipMemcpyAsync(sc->aframe.dev, sc->aframe.host, fup, hipMemcpyHostToDevice, s));
  if (n_obj > 0) DSR_CHECK(ctx, hipMemsetAsync(d_table, 0, sizeof(int) * 3 * (size_t)n_det * n_obj, s));
  // ---- the rows (a frame call: the ingest's row passes and the points-only emit, at the fixed
  // stride max_pts), then the world points
  if (F) {
    const FrameCam FC = frame_cam(F->cam);
    const unsigned gy = (unsigned)((FC.H + FRAME_WAVES - 1) / FRAME_WAVES);
    hipLaunchKernelGGL(k_frame_rows, dim3(gy, n_det), dim3(FRAME_WG), 0, s, FC, F->Q, (const float*)FD.depth,
                       (const int*)FD.inst, (const FrameDet*)FD.dets, FD.rows);
    hipLaunchKernelGGL(k_frame_scan, dim3(n_det), dim3(FRAME_WG), 0, s, FC, F->Q, (const int*)FD.inst,
                       (const FrameDet*)FD.dets, (const int4*)FD.rows, FD.voff, FD.bgoff, FD.aux, FD.recs, (ObjDesc*)nullptr);
    hipLaunchKernelGGL(k_frame_emit<false>, dim3(gy, n_det), dim3(FRAME_WG), 0, s, FC, F->Q, (const float*)FD.depth,
                       (const int*)FD.inst, (const FrameDet*)FD.dets, (const int4*)FD.rows, (const int*)FD.voff,
                       (const int*)FD.bgoff, (const int*)FD.aux, (const dsr_frame_det_out*)FD.recs,
                       (const ObjDesc*)nullptr, sc->arows, (float*)nullptr, (float*)nullptr);
  }
  hipLaunchKernelGGL(k_assoc_world, dim3((n_pts + ASSOC_WG - 1) / ASSOC_WG), dim3(ASSOC_WG), 0, s, n_pts, max_pts,
                     assoc_xf(t_world_cam), (const float*)sc->arows, (const int*)d_cnt, d_frecs, sc->pts);
  // ---- the value passes, back to back: the tile count stays on the device
  dsr_scene_stats st{};
  st.n_obj = n_obj;
  st.n_pts = n_pts;
  st.pairs = (long long)n_obj * n_pts;
  const int grid = std::max(1, std::min(ctx->n_cu, k_pass * ((n_pts + TILE - 1) / TILE)));
  for (int o0 = 0; o0 < n_obj; o0 += k_pass) {
    const int k = std::min(k_pass, n_obj - o0);
    st.n_passes += 1;
    if (int rc = scene_value_pass(sc, o0, k, n_pts, false, false)) return rc;
    hipLaunchKernelGGL(k_assoc_vote, dim3(grid), dim3(TILE), 0, s, (const ObjDesc*)sc->desc, (const Tile*)sc->tiles,
                       (const int*)sc->ntiles, (const float4*)sc->cand, (const float*)sc->dense, max_pts, n_det, n_obj,
                       A.inlier_tol, d_table);
  }
  hipLaunchKernelGGL(k_assoc_pick, dim3(n_det), dim3(64), 0, s, A, n_det, n_obj, (const int*)d_table, (const int*)d_cnt,
                     d_frecs, d_recs);
  DSR_CHECK(ctx, hipGetLastError());
  // ---- the tables, the records and the objects' candidate counts come back; the call's one wait
  const size_t tb = sizeof(int) * 3 * (size_t)n_det * n_obj;
  if (n_obj > 0) DSR_CHECK(ctx, hipMemcpyAsync(hb + L.table, d_table, tb, hipMemcpyDeviceToHost, s));
  DSR_CHECK(ctx, hipMemcpyAsync(hb + L.recs, d_recs, sizeof(dsr_assoc_out) * n_det, hipMemcpyDeviceToHost, s));
  if (n_obj > 0) DSR_CHECK(ctx, hipMemcpyAsync(hb + L.desc, sc->ocount, sizeof(int) * n_obj, hipMemcpyDeviceToHost, s));
  DSR_CHECK(ctx, hipEventRecord(sc->a_ev, s));
  DSR_CHECK(ctx, hipStreamSynchronize(s));
  std::memcpy(out, hb + L.recs, sizeof(dsr_assoc_out) * n_det);
  if (table && n_obj > 0) std::memcpy(table, hb + L.table, tb);
  sc->q_in.assign(n_obj, 0);
  if (n_obj > 0) std::memcpy(sc->q_in.data(), hb + L.desc, sizeof(int) * n_obj);
  for (int i = 0; i < n_obj; ++i) st.decoded += sc->q_in[i];
  sc->st = st;
  sc->q_obj = n_obj;                 // dsr_scene_peek speaks of this call's points
  sc->q_pts = n_pts;
  return 0;
}

// A HIP error in the middle of a call must not leave a copy out of (or into) the pinned blocks in
// flight: the stream is drained before the error is returned, so the next call's staging is free,
// as after dsr_scene_query's blocking copies.
static int assoc_run(dsr_scene* sc, const dsr_assoc_params& A, const float* t_world_cam, int n_det, int max_pts,
                     const AssocFrame* F, const int* n_rows, const float* rows, dsr_assoc_out* out, int* table) {
  dsr_ctx* ctx = sc->ctx;
  if (int rc = decoder_ready(ctx, sc->dec)) return rc;
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  const int rc = assoc_enqueue_wait(sc, A, t_world_cam, n_det, max_pts, F, n_rows, rows, out, table);
  if (rc != 0) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
  }
  return rc;
}

// the refusals both forms share, after their own null checks
static const char* assoc_args_error(const dsr_scene* sc, const dsr_assoc_params* A, const float* t_world_cam, int n_det,
                                    int max_pts) {
  if (sc->n_obj < 0) return "dsr_scene_associate before dsr_scene_set_objects";
  if (n_det < 1) return "associate: n_det must be >= 1";
  if (max_pts < 1) return "associate: max_pts must be >= 1";
  if ((long long)n_det * max_pts > sc->max_pts) return "associate: n_det x max_pts exceeds the scene's max_pts";
  if (t_world_cam && !assoc_rigid(t_world_cam))
    return "associate: t_world_cam is not rigid (finite, last row 0 0 0 1, R^T R = I within 1e-4, det R > 0)";
  return assoc_params_error(A);
}

int dsr_scene_associate_frame(dsr_scene* sc, const dsr_camera* cam, const dsr_frame_params* frame_params,
                              const dsr_assoc_params* assoc_params, const float* t_world_cam,
                              const float* depth, const int* instance, int n_det, const int* labels,
                              dsr_assoc_out* out, int* table) {
  if (!sc) return -2;
  dsr_ctx* ctx = sc->ctx;
  if (!cam || !frame_params || !assoc_params || !t_world_cam || !depth || !instance || !labels || !out)
    return fail(ctx, "null argument");
  if (n_det < 1) return fail(ctx, "associate: n_det must be >= 1");
  AssocFrame F{cam, assoc_frame_params(frame_params), depth, instance, nullptr};
  const std::vector<dsr_frame_det> dets = assoc_frame_dets(n_det, labels);
  F.dets = &dets;
  if (const char* m = frame_args_error(cam, &F.Q, depth, instance, n_det, dets.data())) return fail(ctx, m);
  if (const char* m = assoc_args_error(sc, assoc_params, t_world_cam, n_det, F.Q.max_pts)) return fail(ctx, m);
  return assoc_run(sc, *assoc_params, t_world_cam, n_det, F.Q.max_pts, &F, nullptr, nullptr, out, table);
}

int dsr_scene_associate_points(dsr_scene* sc, const dsr_assoc_params* assoc_params, const float* t_world_cam,
                               int n_det, int max_pts, const int* n_rows, const float* rows,
                               dsr_assoc_out* out, int* table) {
  if (!sc) return -2;
  dsr_ctx* ctx = sc->ctx;
  if (!assoc_params || !n_rows || !rows || !out) return fail(ctx, "null argument");
  if (const char* m = assoc_args_error(sc, assoc_params, t_world_cam, n_det, max_pts)) return fail(ctx, m);
  for (int j = 0; j < n_det; ++j)
    if (n_rows[j] < 0 || n_rows[j] > max_pts) return fail(ctx, "associate: n_rows must be in [0, max_pts]");
  return assoc_run(sc, *assoc_params, t_world_cam, n_det, max_pts, nullptr, n_rows, rows, out, table);
}

// ------------------------------------------------------------------------------------
// raw decoder queries (dsr_sdf_eval)
// ------------------------------------------------------------------------------------
int dsr_sdf_eval(dsr_ctx* ctx, const dsr_decoder* dec, const float* code, const float* pts, int n,
                 float* sdf, float* jac) {
  if (!ctx || !dec || !code || (n > 0 && (!pts || !sdf))) return fail(ctx, "null argument");
  if (int rc = decoder_ready(ctx, dec)) return rc;
  if (n <= 0) return 0;
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  float* lnw = nullptr;          // LayerNorm decoders: the context stream's Jacobian workspace
  if (int rc = decoder_ready(ctx, dec, jac != nullptr, &lnw)) return rc;
  float zc[CODE] = {};                               // a 32-D code runs padded with zeros
  std::memcpy(zc, code, sizeof(float) * dec->code_len);
  const int nt = (n + TILE - 1) / TILE;
  std::vector<float4> hp((size_t)nt * TILE, make_float4(0.f, 0.f, 0.f, 0.f));
  for (int i = 0; i < n; ++i) {
    float fi;
    std::memcpy(&fi, &i, sizeof(float));
    hp[i] = make_float4(pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], fi);
  }
  std::vector<Tile> ht(nt);
  for (int t = 0; t < nt; ++t) ht[t] = Tile{0, jac ? 2 : 0, t * TILE, std::min(TILE, n - t * TILE)};
  ObjDesc d{};
  d.n_pts = n;
  float4* dp = nullptr;
  float *dz = nullptr, *db0 = nullptr, *db4 = nullptr, *dout = nullptr;
  Tile* dt = nullptr;
  int* dnt = nullptr;
  ObjDesc* dd = nullptr;
  DevArena mem;                                      // (freed on return: after the copy back)
  const size_t outw = jac ? (size_t)(IN + 1) : 1;
  if (!mem.alloc(&dp, hp.size()) || !mem.alloc(&dz, CODE) || !mem.alloc(&db0, HID) || !mem.alloc(&db4, HID) ||
      !mem.alloc(&dt, nt) || !mem.alloc(&dnt, 1) || !mem.alloc(&dout, outw * nt * TILE) || !mem.alloc(&dd, 1))
    return fail(ctx, "hipMalloc failed (sdf_eval)");
  bool ok = hipMemcpy(dp, hp.data(), sizeof(float4) * hp.size(), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dz, zc, sizeof(float) * CODE, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dt, ht.data(), sizeof(Tile) * nt, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dnt, &nt, sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dd, &d, sizeof(ObjDesc), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) return fail(ctx, "hipMemcpy failed (sdf_eval)");
  const DevDecoder& D = dec->D;
  fold_codes(s, D, dz, 1, db0, db4);
  const int grid = std::min(ctx->n_cu, nt);
  if (jac) {
    JacQuery q{dt, dnt, dd, db0, db4};
    q.query_pts = dp;
    q.raw_out = dout;
    q.lnw = lnw;
    launch_jac(s, grid, D, q);
  } else {
    launch_fwd(s, grid, D, {dt, dnt, dd, dp, db0, db4, dout});
  }
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
    return fail(ctx, "kernel failed (sdf_eval)");
  std::vector<float> h(outw * n);
  if (hipMemcpy(h.data(), dout, sizeof(float) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return fail(ctx, "hipMemcpy D2H failed (sdf_eval)");
  // jac rows: [code (code_len) | xyz (3)] (the kernels' 64-D layout holds code 0..63, xyz 64..66)
  const int L = dec->code_len, jw = L + 3;
  for (int i = 0; i < n; ++i) {
    sdf[i] = h[i * outw];
    if (jac) {
      for (int k = 0; k < L; ++k) jac[(size_t)i * jw + k] = h[i * outw + 1 + k];
      for (int k = 0; k < 3; ++k) jac[(size_t)i * jw + L + k] = h[i * outw + 1 + CODE + k];
    }
  }
  return 0;
}

// Optimizer.estimate_pose_cam_obj (optimizer.py:46-87) for n_obj independent objects in
// one device pass per GN iteration: one fwd+Jacobian launch over every object's tiles (the
// Jacobian kernel's tiles carry their object), one k_solve_pose workgroup per object.  The
// reference's iteration-4 inlier filter (:77-79, only effective past 5 iterations) is a
// host compaction of each object's points.
int dsr_pose_only_batch(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, int n_obj,
                        const dsr_pose_in* in, float* t_out) {
  if (!ctx || !dec || !p || !t_out || (n_obj > 0 && !in)) return fail(ctx, "null argument");
  if (n_obj <= 0) return fail(ctx, "n_obj must be > 0");
  if (p->code_len != dec->code_len) return fail(ctx, "optimizer code_len != decoder code_len");
  float* lnw = nullptr;          // LayerNorm decoders: the context stream's Jacobian workspace
  if (int rc = decoder_ready(ctx, dec, true, &lnw)) return rc;
  for (int o = 0; o < n_obj; ++o) {
    if (!in[o].code || (in[o].n_pts > 0 && !in[o].pts)) return fail(ctx, "null argument");
    if (in[o].n_pts < 0) return fail(ctx, "bad surface points");
  }
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->stream;
  std::vector<float> t_in((size_t)16 * n_obj), hz((size_t)CODE * n_obj);
  std::vector<std::vector<float>> hp(n_obj);
  size_t cap_pts = 0, cap_tiles = 0;
  for (int o = 0; o < n_obj; ++o) {
    const dsr_pose_in& x = in[o];
    for (int i = 0; i < 16; ++i) t_in[16 * o + i] = x.t_co_se3[i];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) t_in[16 * o + i * 4 + j] = t_in[16 * o + i * 4 + j] * x.scale;   // :56 (fp32)
    std::copy(x.code, x.code + dec->code_len, hz.begin() + (size_t)CODE * o);   // (rest 0)
    hp[o].assign(x.pts, x.pts + (size_t)x.n_pts * 3);
    cap_pts += x.n_pts;
    cap_tiles += (x.n_pts + TILE - 1) / TILE;
  }
  const int iters = p->pose_only_iterations;
  float *dpts = nullptr, *dz = nullptr, *db0 = nullptr, *db4 = nullptr, *dslots = nullptr, *dtin = nullptr,
        *dzb = nullptr, *dres = nullptr, *dout = nullptr;
  ObjState* dst = nullptr;
  ObjDesc* ddesc = nullptr;
  Tile* dt = nullptr;
  int *dnt = nullptr, *doc = nullptr;
  DevArena mem;                                      // (freed on return: after the copy back)
  const size_t n = (size_t)n_obj;
  if (!mem.alloc(&dpts, 3 * cap_pts) || !mem.alloc(&dst, n) || !mem.alloc(&dz, CODE * n) || !mem.alloc(&db0, HID * n) ||
      !mem.alloc(&db4, HID * n) || !mem.alloc(&dt, cap_tiles) || !mem.alloc(&dnt, 1) ||
      !mem.alloc(&dslots, SLOT_FLOATS * cap_tiles) || !mem.alloc(&ddesc, n) || !mem.alloc(&dtin, 16 * n) ||
      !mem.alloc(&doc, n) || !mem.alloc(&dzb, CODE * n) || !mem.alloc(&dres, cap_pts) || !mem.alloc(&dout, 16 * n))
    return fail(ctx, "hipMalloc failed (pose_only)");
  const std::vector<int> zeros(n, 0);
  bool ok = hipMemcpy(dz, hz.data(), sizeof(float) * CODE * n, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dtin, t_in.data(), sizeof(float) * 16 * n, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(doc, zeros.data(), sizeof(int) * n, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) return fail(ctx, "hipMemcpy failed (pose_only)");
  const DevDecoder& D = dec->D;
  GNParams P = make_params(p, false);
  P.raw_residual = 1;
  fold_codes(s, D, dz, n_obj, db0, db4);
  hipLaunchKernelGGL(k_init_state, dim3(n_obj), dim3(64), 0, s, n_obj, (const float*)dtin, (const int*)doc,
                     (const float*)dz, dst, dzb, 1, WinTable{});                       // :57 t_obj_cam = inv
  int n_tiles = 0;
  // points, descriptors and tile table of the current point sets (objects back to back)
  auto upload = [&]() {
    std::vector<ObjDesc> hd(n);
    std::vector<Tile> ht;
    std::vector<float> all;
    int poff = 0, soff = 0;
    for (int o = 0; o < n_obj; ++o) {
      const int np = (int)(hp[o].size() / 3);
      hd[o].pts_off = poff;
      hd[o].n_pts = np;
      hd[o].slot_sdf = soff;
      for (int t = 0; t * TILE < np; ++t) ht.push_back(Tile{o, 0, t * TILE, std::min(TILE, np - t * TILE)});
      all.insert(all.end(), hp[o].begin(), hp[o].end());
      poff += np;
      soff += (np + TILE - 1) / TILE;
    }
    n_tiles = (int)ht.size();
    return (all.empty() || hipMemcpy(dpts, all.data(), sizeof(float) * all.size(), hipMemcpyHostToDevice) == hipSuccess) &&
           hipMemcpy(ddesc, hd.data(), sizeof(ObjDesc) * n, hipMemcpyHostToDevice) == hipSuccess &&
           (ht.empty() || hipMemcpy(dt, ht.data(), sizeof(Tile) * ht.size(), hipMemcpyHostToDevice) == hipSuccess) &&
           hipMemcpy(dnt, &n_tiles, sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!upload()) return fail(ctx, "hipMemcpy failed (pose_only tiles)");
  std::vector<char> emptied(n, 0);
  for (int o = 0; o < n_obj; ++o)           // no points: J^T J / 0 -> a NaN pose (golden F10)
    if (in[o].n_pts == 0) emptied[o] = 1;
  JacQuery jq{dt, dnt, ddesc, db0, db4};
  jq.st = dst;
  jq.surf_pts = dpts;
  jq.P = P;
  jq.slots = dslots;
  jq.lnw = lnw;
  for (int e = 0; e < iters; ++e) {
    const bool filter = (e == 4) && (e + 1 < iters);   // :77-79 inlier filter (effective only past 5 iters)
    jq.res_out = filter ? dres : nullptr;
    if (n_tiles > 0) launch_jac(s, std::max(1, std::min(ctx->n_cu, n_tiles)), D, jq);
    hipLaunchKernelGGL(k_solve_pose, dim3(n_obj), dim3(256), 0, s, (const ObjDesc*)ddesc, dst, (const float*)dslots);
    if (filter) {
      size_t tot = 0;
      for (int o = 0; o < n_obj; ++o) tot += hp[o].size() / 3;
      std::vector<float> res(std::max<size_t>(1, tot));
      if (hipStreamSynchronize(s) != hipSuccess ||      // ctx->stream is non-blocking
          (tot && hipMemcpy(res.data(), dres, sizeof(float) * tot, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(ctx, "hipMemcpy failed (pose_only residuals)");
      size_t off = 0;
      for (int o = 0; o < n_obj; ++o) {
        const size_t np = hp[o].size() / 3;
        std::vector<float> kept;
        for (size_t i = 0; i < np; ++i)
          if (std::fabs(res[off + i]) <= 0.05f) kept.insert(kept.end(), hp[o].begin() + 3 * i, hp[o].begin() + 3 * i + 3);
        off += np;
        hp[o].swap(kept);
        if (hp[o].empty()) emptied[o] = 1;    // the reference goes on with an empty set: NaN pose
      }
      if (!upload()) return fail(ctx, "hipMemcpy failed (pose_only filter)");
    }
  }
  hipLaunchKernelGGL(k_inv_out, dim3((n_obj + 63) / 64), dim3(64), 0, s, n_obj, (const ObjState*)dst, dout);   // :84
  std::vector<float> T((size_t)16 * n);
  ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(s) == hipSuccess &&
       hipMemcpy(T.data(), dout, sizeof(float) * 16 * n, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) return fail(ctx, "pose_only failed");
  for (int o = 0; o < n_obj; ++o) {
    float* to = t_out + 16 * o;
    for (int i = 0; i < 16; ++i) to[i] = T[16 * o + i];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) to[i * 4 + j] = to[i * 4 + j] / in[o].scale;           // :85
    if (emptied[o])                     // J^T J / 0 in the reference: the pose turns NaN
      for (int i = 0; i < 16; ++i) to[i] = __builtin_nanf("");
  }
  return 0;
}

int dsr_pose_only(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, const float* t_co_se3,
                  float scale, const float* pts, int n_pts, const float* code, float* t_out) {
  if (!t_co_se3) return fail(ctx, "null argument");
  dsr_pose_in x;
  for (int i = 0; i < 16; ++i) x.t_co_se3[i] = t_co_se3[i];
  x.scale = scale;
  x.pts = pts;
  x.n_pts = n_pts;
  x.code = code;
  return dsr_pose_only_batch(ctx, dec, p, 1, &x, t_out);
}


// ------------------------------------------------------------------------------------
// tracker: dsr_pose_only_batch as a resident handle (dsr_tracker_*; the
// kernels and the host rule of the start pose in dsr_track.hpp)
// ------------------------------------------------------------------------------------
struct dsr_tracker {
  dsr_ctx* ctx = nullptr;
  const dsr_decoder* dec = nullptr;
  GNParams P{};
  int iters = 0, max_obj = 0, max_pts = 0, tpo = 0;
  float* lnw = nullptr;              // LayerNorm decoders: the context stream's Jacobian workspace
  DevArena mem;
  // device; head = t_in | z | cnt and tail = out | recs are one block each (one copy each way)
  char *head = nullptr, *tail = nullptr;
  float *t_in = nullptr, *z = nullptr, *zb = nullptr, *b0 = nullptr, *b4 = nullptr;
  int *cnt = nullptr, *is_oc = nullptr, *n_tiles = nullptr;
  float *pts = nullptr, *res = nullptr, *slots = nullptr, *out = nullptr;
  ObjDesc* desc = nullptr;
  ObjState* st = nullptr;
  Tile* tiles = nullptr;
  dsr_track_out* recs = nullptr;
  // pinned: head | pts | tail
  char* host = nullptr;
  size_t head_bytes = 0, pts_bytes = 0, tail_bytes = 0;
  dsr_batch::IngestBlock sweep;      // a sweep call's block (lidar_carve without an image): it grows
  dsr_batch::IngestBlock frame;      // a frame call's block (frame_carve): it grows
  hipEvent_t up_ev = nullptr;        // recorded after a call's uploads
  hipEvent_t done_ev = nullptr;      // recorded after a call's copy into the pinned tail
  int n_last = 0;                    // objects of the last call (0: none yet)
  std::vector<float> scale;          // their scales (optimizer.py:85 on the host)
};

// the parts of head and tail, on either side
static size_t track_head_z(int max_obj) { return frame_up256(sizeof(float) * 16 * (size_t)max_obj); }
static size_t track_head_cnt(int max_obj) { return track_head_z(max_obj) + frame_up256(sizeof(float) * CODE * (size_t)max_obj); }
static size_t track_tail_recs(int max_obj) { return frame_up256(sizeof(float) * 16 * (size_t)max_obj); }

int dsr_tracker_destroy(dsr_tracker* tr) {
  if (!tr) return 0;
  std::lock_guard<std::recursive_mutex> run(tr->ctx->run_mu);
  hipSetDevice(tr->ctx->device);
  hipStreamSynchronize(tr->ctx->stream);
  if (tr->up_ev) hipEventDestroy(tr->up_ev);
  if (tr->done_ev) hipEventDestroy(tr->done_ev);
  if (tr->host) hipHostFree(tr->host);
  if (tr->sweep.host) hipHostFree(tr->sweep.host);
  if (tr->sweep.dev) hipFree(tr->sweep.dev);
  if (tr->frame.host) hipHostFree(tr->frame.host);
  if (tr->frame.dev) hipFree(tr->frame.dev);
  delete tr;
  return 0;
}

int dsr_tracker_create(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, int max_obj, int max_pts,
                       dsr_tracker** out) {
  if (!ctx || !dec || !p || !out) return fail(ctx, "null argument");
  *out = nullptr;
  if (max_obj < 1) return fail(ctx, "tracker: max_obj must be >= 1");
  if (max_pts < 1 || max_pts > TRACK_MAX_PTS) return fail(ctx, "tracker: max_pts must be in [1, 2^20]");
  if ((long long)max_obj * max_pts > TRACK_MAX_ROWS) return fail(ctx, "tracker: max_obj x max_pts must be at most 2^22");
  if (p->code_len != dec->code_len) return fail(ctx, "optimizer code_len != decoder code_len");
  float* lnw = nullptr;
  if (int rc = decoder_ready(ctx, dec, true, &lnw)) return rc;
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  auto* tr = new dsr_tracker();
  tr->ctx = ctx;
  tr->dec = dec;
  tr->P = make_params(p, false);
  tr->P.raw_residual = 1;
  tr->iters = p->pose_only_iterations;
  tr->max_obj = max_obj;
  tr->max_pts = max_pts;
  tr->tpo = track_tiles_per_obj(max_pts);
  tr->lnw = lnw;
  const size_t no = (size_t)max_obj, rows = no * max_pts, nt = no * tr->tpo;
  tr->head_bytes = track_head_cnt(max_obj) + frame_up256(sizeof(int) * no);
  tr->pts_bytes = frame_up256(sizeof(float) * 3 * rows);
  tr->tail_bytes = track_tail_recs(max_obj) + frame_up256(sizeof(dsr_track_out) * no);
  DevArena& M = tr->mem;
  bool ok = M.alloc(&tr->head, tr->head_bytes) && M.alloc(&tr->tail, tr->tail_bytes) && M.alloc(&tr->pts, 3 * rows) &&
            M.alloc(&tr->res, rows) && M.alloc(&tr->desc, no) && M.alloc(&tr->st, no) && M.alloc(&tr->zb, CODE * no) &&
            M.alloc(&tr->b0, HID * no) && M.alloc(&tr->b4, HID * no) && M.alloc(&tr->is_oc, no) &&
            M.alloc(&tr->tiles, nt) && M.alloc(&tr->n_tiles, 1) && M.alloc(&tr->slots, SLOT_FLOATS * nt);
  ok = ok && hipHostMalloc((void**)&tr->host, tr->head_bytes + tr->pts_bytes + tr->tail_bytes, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&tr->up_ev, hipEventDisableTiming) == hipSuccess &&
       hipEventCreateWithFlags(&tr->done_ev, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipMemset(tr->is_oc, 0, sizeof(int) * no) == hipSuccess;      // t_in is camera<-object (:57)
  if (!ok) {
    (void)hipGetLastError();
    dsr_tracker_destroy(tr);
    return fail(ctx, "hipMalloc failed (tracker)");
  }
  std::memset(tr->host, 0, tr->head_bytes + tr->pts_bytes + tr->tail_bytes);
  tr->t_in = reinterpret_cast<float*>(tr->head);
  tr->z = reinterpret_cast<float*>(tr->head + track_head_z(max_obj));
  tr->cnt = reinterpret_cast<int*>(tr->head + track_head_cnt(max_obj));
  tr->out = reinterpret_cast<float*>(tr->tail);
  tr->recs = reinterpret_cast<dsr_track_out*>(tr->tail + track_tail_recs(max_obj));
  tr->scale.assign(no, 1.f);
  *out = tr;
  return 0;
}

static bool track_pose_ok(const float* t, float scale) {
  if (!(scale > 0.f) || std::isinf(scale)) return false;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(t[i])) return false;
  return true;
}

// object o's staged head rows: t_in = t_co_se3 with the fp32 scale on its rotation block
// (optimizer.py:56), the code padded with zeros, the count (0 for a sweep call: k_lidar_scan's)
static void track_stage(dsr_tracker* tr, int o, const float* t_co_se3, float scale, const float* code, int n_pts) {
  float* t = reinterpret_cast<float*>(tr->host) + (size_t)16 * o;
  for (int i = 0; i < 16; ++i) t[i] = t_co_se3[i];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) t[i * 4 + j] = t[i * 4 + j] * scale;
  float* z = reinterpret_cast<float*>(tr->host + track_head_z(tr->max_obj)) + (size_t)CODE * o;
  std::memset(z, 0, sizeof(float) * CODE);
  std::memcpy(z, code, sizeof(float) * tr->dec->code_len);
  reinterpret_cast<int*>(tr->host + track_head_cnt(tr->max_obj))[o] = n_pts;
  tr->scale[o] = scale;
}

namespace {
// where a call's points come from when not from host rows: a sweep (S, LP, tcv) through tr->sweep
// or a depth image (FC, FP) through tr->frame; `up` bytes of that block are uploaded
struct TrackIngest {
  const LidarShape* S = nullptr;
  const dsr_lidar_params* LP = nullptr;
  const float* tcv = nullptr;
  const FrameCam* FC = nullptr;
  const dsr_frame_params* FP = nullptr;
  size_t up = 0;
};
}  // namespace

// Everything of a call after its staging, on the context stream: the uploads (the head, then
// pts_floats of host rows or G.up bytes of the ingest block G names), the fill's kernels, the GN
// loop of dsr_pose_only_batch with the filter and the tile table on the device, and the copy into
// the pinned tail.  tile_bound: the call's tiles at most (sizes the Jacobian grid).
static int track_run(dsr_tracker* tr, int n, size_t pts_floats, int tile_bound, const TrackIngest& G) {
  dsr_ctx* ctx = tr->ctx;
  hipStream_t s = ctx->stream;
  const LidarShape* S = G.S;
  DSR_CHECK(ctx, hipMemcpyAsync(tr->head, tr->host, tr->head_bytes, hipMemcpyHostToDevice, s));
  if (pts_floats)
    DSR_CHECK(ctx, hipMemcpyAsync(tr->pts, tr->host + tr->head_bytes, sizeof(float) * pts_floats, hipMemcpyHostToDevice, s));
  LidarDev L{};
  FrameDev F{};
  if (S) {
    DSR_CHECK(ctx, hipMemcpyAsync(tr->sweep.dev, tr->sweep.host, G.up, hipMemcpyHostToDevice, s));
    L = lidar_carve(tr->sweep.dev, *S);
  }
  if (G.FC) {
    DSR_CHECK(ctx, hipMemcpyAsync(tr->frame.dev, tr->frame.host, G.up, hipMemcpyHostToDevice, s));
    F = frame_carve(tr->frame.dev, G.FC->W, G.FC->H, n);
  }
  DSR_CHECK(ctx, hipEventRecord(tr->up_ev, s));
  const int nc = S ? lidar_chunks(S->n_velo) : 0;
  const unsigned gc = (unsigned)((nc + FRAME_WAVES - 1) / FRAME_WAVES);
  const unsigned gy = G.FC ? (unsigned)((G.FC->H + FRAME_WAVES - 1) / FRAME_WAVES) : 0;
  if (S) {                                  // the crop passes of lidar_launch; no image pass runs
    if (nc > 0)
      hipLaunchKernelGGL(k_lidar_count, dim3(gc, n), dim3(FRAME_WG), 0, s, (const float*)L.velo, S->n_velo, S->stride,
                         (const LidarDet*)L.dets, nc, L.cnt);
    hipLaunchKernelGGL(k_lidar_scan, dim3(n), dim3(FRAME_WG), 0, s, *G.LP, (const LidarDet*)L.dets, nc, (const int*)L.cnt,
                       L.coff, L.hits, L.nproj, L.recs);
  }
  if (G.FC) {                               // the first two passes of frame_launch; max_bg = 0: no background
    hipLaunchKernelGGL(k_frame_rows, dim3(gy, n), dim3(FRAME_WG), 0, s, *G.FC, *G.FP, (const float*)F.depth,
                       (const int*)F.inst, (const FrameDet*)F.dets, F.rows);
    hipLaunchKernelGGL(k_frame_scan, dim3(n), dim3(FRAME_WG), 0, s, *G.FC, *G.FP, (const int*)F.inst,
                       (const FrameDet*)F.dets, (const int4*)F.rows, F.voff, F.bgoff, F.aux, F.recs, (ObjDesc*)nullptr);
  }
  hipLaunchKernelGGL(k_track_begin, dim3(1), dim3(TILE_SCAN_THREADS), 0, s, n, tr->max_pts, tr->tpo, (const int*)tr->cnt,
                     (const dsr_lidar_det_out*)(S ? L.recs : nullptr), (const dsr_frame_det_out*)(G.FC ? F.recs : nullptr),
                     tr->desc, tr->recs, tr->tiles, tr->n_tiles);
  if (S && nc > 0)
    hipLaunchKernelGGL(k_lidar_emit<false>, dim3(gc, n), dim3(FRAME_WG), 0, s, FrameCam{}, *G.LP, lidar_xf(G.tcv),
                       (const float*)L.velo, S->n_velo, S->stride, (const int*)nullptr, (const dsr_lidar_mask*)nullptr, 0,
                       (const LidarDet*)L.dets, nc, (const int*)L.cnt, (const int*)L.coff,
                       (const dsr_lidar_det_out*)L.recs, (int*)nullptr, (int*)nullptr, (const ObjDesc*)tr->desc, tr->pts,
                       (float*)nullptr, (float*)nullptr);
  if (G.FC)                                 // the points alone, without the background z-slice
    hipLaunchKernelGGL(k_frame_emit<false>, dim3(gy, n), dim3(FRAME_WG), 0, s, *G.FC, *G.FP, (const float*)F.depth,
                       (const int*)F.inst, (const FrameDet*)F.dets, (const int4*)F.rows, (const int*)F.voff,
                       (const int*)F.bgoff, (const int*)F.aux, (const dsr_frame_det_out*)F.recs,
                       (const ObjDesc*)tr->desc, tr->pts, (float*)nullptr, (float*)nullptr);
  const DevDecoder& D = tr->dec->D;
  fold_codes(s, D, tr->z, n, tr->b0, tr->b4);
  hipLaunchKernelGGL(k_init_state, dim3(n), dim3(64), 0, s, n, (const float*)tr->t_in, (const int*)tr->is_oc,
                     (const float*)tr->z, tr->st, tr->zb, 1, WinTable{});              // :57 t_obj_cam = inv
  JacQuery jq{tr->tiles, tr->n_tiles, tr->desc, tr->b0, tr->b4};
  jq.st = tr->st;
  jq.surf_pts = tr->pts;
  jq.P = tr->P;
  jq.slots = tr->slots;
  jq.lnw = tr->lnw;
  const int grid = std::max(1, std::min(ctx->n_cu, tile_bound));
  for (int e = 0; e < tr->iters; ++e) {
    const bool filter = (e == 4) && (e + 1 < tr->iters);   // :77-79 inlier filter (effective only past 5 iters)
    jq.res_out = filter ? tr->res : nullptr;
    if (tile_bound > 0) launch_jac(s, grid, D, jq);
    hipLaunchKernelGGL(k_solve_pose, dim3(n), dim3(256), 0, s, (const ObjDesc*)tr->desc, tr->st, (const float*)tr->slots);
    if (filter && tile_bound > 0) {
      hipLaunchKernelGGL(k_track_filter, dim3(n), dim3(FRAME_WG), 0, s, tr->desc, (const float*)tr->res, tr->pts, tr->recs);
      hipLaunchKernelGGL(k_track_tiles, dim3(1), dim3(TILE_SCAN_THREADS), 0, s, n, (const ObjDesc*)tr->desc, tr->tiles,
                         tr->n_tiles);
    }
  }
  hipLaunchKernelGGL(k_inv_out, dim3((n + 63) / 64), dim3(64), 0, s, n, (const ObjState*)tr->st, tr->out);   // :84
  DSR_CHECK(ctx, hipGetLastError());
  DSR_CHECK(ctx, hipMemcpyAsync(tr->host + tr->head_bytes + tr->pts_bytes, tr->tail, tr->tail_bytes,
                                hipMemcpyDeviceToHost, s));
  DSR_CHECK(ctx, hipEventRecord(tr->done_ev, s));
  tr->n_last = n;
  return 0;
}

int dsr_tracker_track(dsr_tracker* tr, int n_obj, const dsr_pose_in* in) {
  if (!tr) return -2;
  dsr_ctx* ctx = tr->ctx;
  if (!in) return fail(ctx, "null argument");
  if (n_obj < 1 || n_obj > tr->max_obj) return fail(ctx, "tracker: n_obj must be in [1, the tracker's max_obj]");
  long long tiles = 0;
  for (int o = 0; o < n_obj; ++o) {
    if (!in[o].code || (in[o].n_pts > 0 && !in[o].pts)) return fail(ctx, "null argument");
    if (in[o].n_pts < 0 || in[o].n_pts > tr->max_pts) return fail(ctx, "tracker: an object's points exceed the tracker's max_pts");
    if (!track_pose_ok(in[o].t_co_se3, in[o].scale)) return fail(ctx, "tracker: scale must be positive and finite, the pose finite");
    tiles += (in[o].n_pts + TILE - 1) / TILE;
  }
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  DSR_CHECK(ctx, hipEventSynchronize(tr->up_ev));    // the previous call's uploads have left the pinned block
  float* hp = reinterpret_cast<float*>(tr->host + tr->head_bytes);
  for (int o = 0; o < n_obj; ++o) {
    const dsr_pose_in& x = in[o];
    track_stage(tr, o, x.t_co_se3, x.scale, x.code, x.n_pts);
    if (x.n_pts) std::memcpy(hp + (size_t)o * tr->max_pts * 3, x.pts, sizeof(float) * 3 * x.n_pts);
  }
  // objects 0 .. n_obj - 1 at the fixed stride: up to the last object's last row
  const size_t up = ((size_t)(n_obj - 1) * tr->max_pts + in[n_obj - 1].n_pts) * 3;
  return track_run(tr, n_obj, tiles ? up : 0, (int)tiles, TrackIngest{});
}

// dsr_lidar_inputs_host's argument errors for what a tracker call reads: the fields that are not
// read are given valid values (a 1 x 1 camera and image, no masks, no background grid)
static const char* track_lidar_error(const dsr_lidar_params* P, bool crop, const float* tcv, const float* velo,
                                     int n_velo, int stride, int n_det, const dsr_lidar_det* dets) {
  if (!P) return "lidar: null camera or parameters";
  const dsr_camera cam{1, 1, 1.f, 1.f, 0.f, 0.f};
  const int inst = 0;
  const dsr_lidar_params Q{crop ? P->max_pts : 1, 0, 1, 0, 0, crop ? P->radius : 1.f, P->box_margin};
  return lidar_args_error(&cam, &Q, lidar_rigid(tcv), velo, n_velo, stride, &inst, 0, nullptr, n_det, dets);
}

int dsr_lidar_track_prep_host(const dsr_lidar_params* params, const float* t_cam_velo, int n_det,
                              const dsr_lidar_det* dets, float* t_co_se3, float* det_scale) {
  if (track_lidar_error(params, false, t_cam_velo, nullptr, 0, 3, n_det, dets)) return -2;
  if (n_det > 0 && (!t_co_se3 || !det_scale)) return -2;
  for (int d = 0; d < n_det; ++d) lidar_track_prep(*params, t_cam_velo, dets[d], t_co_se3 + (size_t)16 * d, det_scale + d);
  return 0;
}

int dsr_tracker_track_lidar(dsr_tracker* tr, const dsr_lidar_params* params, const float* t_cam_velo,
                            const float* velo, int n_velo, int stride, int n_det, const dsr_lidar_det* dets,
                            const dsr_track_det* prior) {
  if (!tr) return -2;
  dsr_ctx* ctx = tr->ctx;
  if (!params || !t_cam_velo || !dets || !prior) return fail(ctx, "null argument");
  if (n_det < 1 || n_det > tr->max_obj) return fail(ctx, "tracker: n_det must be in [1, the tracker's max_obj]");
  if (const char* m = track_lidar_error(params, true, t_cam_velo, velo, n_velo, stride, n_det, dets)) return fail(ctx, m);
  if (params->max_pts > tr->max_pts) return fail(ctx, "tracker: max_pts exceeds the tracker's max_pts");
  for (int o = 0; o < n_det; ++o) {
    if (!dets[o].code) return fail(ctx, "null argument");
    const float eye[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    if (!track_pose_ok(prior[o].pose_given ? prior[o].t_co_se3 : eye, prior[o].scale))
      return fail(ctx, "tracker: scale must be positive and finite, a given pose finite");
  }
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  // the sweep block is the ingest's without an image: sweep | masks (unused) | prepared detections
  // up, then the crop tables and records
  const LidarShape S{n_velo, stride, 0, 0, n_det};
  const size_t up = lidar_upload_bytes(S);
  if (int rc = ingest_fit(ctx, tr->sweep, tr->up_ev, up, lidar_dev_bytes(S))) return rc;
  const int no_image = 0;
  lidar_pack(tr->sweep.host, S, *params, t_cam_velo, velo, &no_image, 0, nullptr, dets);
  for (int o = 0; o < n_det; ++o) {
    float t[16], det_scale;
    lidar_track_prep(*params, t_cam_velo, dets[o], t, &det_scale);
    track_stage(tr, o, prior[o].pose_given ? prior[o].t_co_se3 : t, prior[o].scale, dets[o].code, 0);
  }
  const int tiles = n_det * track_tiles_per_obj(params->max_pts);
  TrackIngest G;
  G.S = &S; G.LP = params; G.tcv = t_cam_velo; G.up = up;
  return track_run(tr, n_det, 0, tiles, G);
}

// The same from a depth image and its instance labels: the ingest's row passes (k_frame_rows,
// k_frame_scan) and k_frame_emit<false> write detection i's surface points into
// the tracker's point block.  The fields that are not read are given valid values before
// dsr_frame_inputs_host's argument check (no background grid, the mask's tight box, no pose).
int dsr_tracker_track_frame(dsr_tracker* tr, const dsr_camera* cam, const dsr_frame_params* params,
                            const float* depth, const int* instance, int n_det, const dsr_frame_det* dets,
                            const dsr_track_det* prior) {
  if (!tr) return -2;
  dsr_ctx* ctx = tr->ctx;
  if (!cam || !params || !depth || !instance || !dets || !prior) return fail(ctx, "null argument");
  if (n_det < 1 || n_det > tr->max_obj) return fail(ctx, "tracker: n_det must be in [1, the tracker's max_obj]");
  const dsr_frame_params Q{params->max_pts, 0, 1, 0, params->min_mask_area, params->near, params->far};
  std::vector<dsr_frame_det> read(n_det);
  for (int o = 0; o < n_det; ++o) {
    read[o] = dsr_frame_det{};
    read[o].label = dets[o].label;
    read[o].bbox[2] = read[o].bbox[3] = -1;
    read[o].code = dets[o].code;
  }
  if (const char* m = frame_args_error(cam, &Q, depth, instance, n_det, read.data())) return fail(ctx, m);
  if (Q.max_pts > tr->max_pts) return fail(ctx, "tracker: max_pts exceeds the tracker's max_pts");
  for (int o = 0; o < n_det; ++o) {
    if (!read[o].code) return fail(ctx, "null argument");
    if (!prior[o].pose_given) return fail(ctx, "tracker: a frame call needs a start pose (pose_given)");
    if (!track_pose_ok(prior[o].t_co_se3, prior[o].scale))
      return fail(ctx, "tracker: scale must be positive and finite, the pose finite");
  }
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  const int W = cam->width, H = cam->height;
  const size_t up = frame_upload_bytes(W, H, n_det);
  if (int rc = ingest_fit(ctx, tr->frame, tr->up_ev, up, frame_dev_bytes(W, H, n_det))) return rc;
  frame_pack(tr->frame.host, cam, depth, instance, n_det, read.data());
  for (int o = 0; o < n_det; ++o) track_stage(tr, o, prior[o].t_co_se3, prior[o].scale, read[o].code, 0);
  const FrameCam FC = frame_cam(cam);
  TrackIngest G;
  G.FC = &FC; G.FP = &Q; G.up = up;
  return track_run(tr, n_det, 0, n_det * track_tiles_per_obj(Q.max_pts), G);
}

int dsr_tracker_query(dsr_tracker* tr) {
  if (!tr) return -2;
  if (!tr->n_last) return fail(tr->ctx, "tracker has not run");
  std::lock_guard<std::recursive_mutex> run(tr->ctx->run_mu);
  hipSetDevice(tr->ctx->device);
  const hipError_t e = hipEventQuery(tr->done_ev);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  return fail(tr->ctx, std::string("hipEventQuery: ") + hipGetErrorString(e));
}

int dsr_tracker_download(dsr_tracker* tr, float* t_out, dsr_track_out* rec) {
  if (!tr) return -2;
  dsr_ctx* ctx = tr->ctx;
  if (!t_out) return fail(ctx, "null argument");
  if (!tr->n_last) return fail(ctx, "tracker has not run");
  std::lock_guard<std::recursive_mutex> run(ctx->run_mu);
  hipSetDevice(ctx->device);
  DSR_CHECK(ctx, hipEventSynchronize(tr->done_ev));
  const char* tail = tr->host + tr->head_bytes + tr->pts_bytes;
  const float* T = reinterpret_cast<const float*>(tail);
  const dsr_track_out* R = reinterpret_cast<const dsr_track_out*>(tail + track_tail_recs(tr->max_obj));
  for (int o = 0; o < tr->n_last; ++o) {
    float* to = t_out + 16 * o;
    for (int i = 0; i < 16; ++i) to[i] = T[16 * o + i];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) to[i * 4 + j] = to[i * 4 + j] / tr->scale[o];          // :85
    if (R[o].status != DSR_TRACK_OK)    // J^T J / 0 in the reference: the pose turns NaN
      for (int i = 0; i < 16; ++i) to[i] = __builtin_nanf("");
    if (rec) rec[o] = R[o];
  }
  return 0;
}

}  // extern "C"
