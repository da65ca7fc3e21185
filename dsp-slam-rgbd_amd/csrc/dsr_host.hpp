// dsr_host.hpp — host-side scaffolding of the decoder-query entry points of dsr_api.hip: the owner of
// plain device blocks, the preamble of a query, the one form of a decoder query launch and the
// integer test hook.  Included by dsr_api.hip after its context, kernel selection and error helpers
// (it uses dsr_ctx, dsr_decoder, fail, ln_workspace and the kernel tables), in the same
// translation unit.
#pragma once

// Plain device blocks with one owner (the handles of the mesher, renderer and scene, and the
// scratch of a one-call query): every block is rounded up to a multiple of 256 B, a failed
// hipMalloc leaves no stale runtime error behind, and the destructor frees what is left.  The
// batch pool (batch_alloc) has its own rules and is not this.
struct DevArena {
  std::vector<void*> blocks;
  DevArena() = default;
  DevArena(const DevArena&) = delete;
  DevArena& operator=(const DevArena&) = delete;
  ~DevArena() {
    for (void* p : blocks) hipFree(p);
  }
  bool alloc(void** p, size_t bytes) {
    if (hipMalloc(p, (std::max<size_t>(bytes, 1) + 255) / 256 * 256) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    blocks.push_back(*p);
    return true;
  }
  template <class T>
  bool alloc(T** p, size_t count) {
    return alloc((void**)p, sizeof(T) * count);
  }
  void release(void* p) {
    if (!p) return;
    hipFree(p);
    blocks.erase(std::remove(blocks.begin(), blocks.end(), p), blocks.end());
  }
};

// The preamble of every entry point that queries the decoder: the decoder variants (use_tanh,
// xyz_in_all, LayerNorm) are refused under the fp32-MFMA A/B kernels, and with `lnw` a LayerNorm
// decoder whose query runs the Jacobian kernel gets the context stream's workspace.  A site that
// needs the workspace later than the refusal calls twice, the first time without `lnw`.
static int decoder_ready(dsr_ctx* ctx, const dsr_decoder* dec, bool needs_jac = false, float** lnw = nullptr) {
  if (!variant_kernels_ok(dec)) return fail(ctx, "use_tanh / xyz_in_all / LayerNorm decoders run on the split-fp16 kernels only");
  if (lnw && needs_jac && dec->D.ln_mask && !(*lnw = ln_workspace(ctx, 0)))
    return fail(ctx, "hipMalloc failed (LayerNorm workspace)");
  return 0;
}

// One decoder launch of a query outside the batch path.  The head every decoder kernel takes is
// given in order; a site names whatever else it passes, and the rest stays null.  The grid is the
// site's: they size it differently on purpose.
struct FwdQuery {
  const Tile* tiles;
  const int* n_tiles;
  const ObjDesc* desc;
  const float4* pts;
  const float *b0, *b4;
  float* out;
  ErtArgs ert{nullptr, 1, 0.f, nullptr, nullptr};      // no early termination, one sample per ray
  MaskArgs mask{nullptr, nullptr, nullptr, nullptr};   // no kept masks
  FwdKernel kernel = nullptr;                          // null: the query's exact kernel (query_fwd_variant)
};
static void launch_fwd(hipStream_t s, int grid, const DevDecoder& D, const FwdQuery& q) {
  hipLaunchKernelGGL(q.kernel ? q.kernel : fwd_kernel_for(D, query_fwd_variant()).kernel, dim3(grid), dim3(512), 0, s,
                     D, q.tiles, q.n_tiles, q.desc, q.pts, q.b0, q.b4, q.out, (unsigned*)nullptr, q.ert, q.mask);
}
// the lite pass over the same head; q.ert carries its settings
static void launch_lite(hipStream_t s, int grid, const DevDecoder& D, const FwdQuery& q) {
  hipLaunchKernelGGL(lite_schedule().kernel, dim3(grid), dim3(512), 0, s, D, q.tiles, q.n_tiles, q.desc, q.pts, q.b0,
                     q.b4, q.out, q.ert);
}
struct JacQuery {
  const Tile* tiles;
  const int* n_tiles;
  const ObjDesc* desc;
  const float *b0, *b4;
  const ObjState* st = nullptr;
  const float* surf_pts = nullptr;       // GN terms: surface points; render points and their residuals
  const float4* render_pts = nullptr;
  const float* render_res = nullptr;
  GNParams P{};
  float* slots = nullptr;
  const float4* query_pts = nullptr;     // raw queries: value and input Jacobian per point
  float* raw_out = nullptr;
  float* res_out = nullptr;              // per-point residuals (the pose-only inlier filter)
  MaskArgs mask{nullptr, nullptr, nullptr, nullptr};
  float* lnw = nullptr;                  // LayerNorm decoders: decoder_ready's workspace
};
static void launch_jac(hipStream_t s, int grid, const DevDecoder& D, const JacQuery& q) {
  hipLaunchKernelGGL(jac_kernel_for(D).kernel, dim3(grid), dim3(512), 0, s, D, q.tiles, q.n_tiles, q.desc, q.st,
                     q.surf_pts, q.render_pts, q.render_res, q.b0, q.b4, q.P, q.slots, q.query_pts, q.raw_out, q.res_out,
                     q.mask, q.lnw);
}

// an integer test hook (read under DSR_TEST_HOOKS=1 only): the default outside [lo, hi]
static int hook_int(const char* name, int dflt, int lo, int hi) {
  const char* e = hook_env(name);
  const int v = e ? atoi(e) : dflt;
  return v >= lo && v <= hi ? v : dflt;
}
