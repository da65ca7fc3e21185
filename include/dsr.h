/*
 * dsr.h — C ABI of libdsr, the MI355X-native DeepSDF shape-prior reconstruction
 * hot path (DSP-SLAM reconstruct/optimizer.py + loss.py + loss_utils.py +
 * deep_sdf/deep_sdf_decoder.py).
 *
 * The reference exposes this path only as Python (`reconstruct.optimizer.Optimizer`,
 * called from C++ ORB-SLAM2 through pybind11: src/LocalMapping_util.cc:181-182,
 * :394-395, :109-110, src/MapObject_util.cc:43).  The build keeps that Python API
 * (dsp-slam-rgbd_amd/reconstruct) and puts this library underneath it, loaded with
 * ctypes.  Every entry point below names the reference interface it replaces.
 *
 * Conventions
 *   - plain C types only; all matrices are row-major float32 (numpy C order);
 *   - every function returns int status: 0 = ok, <0 = error (message via
 *     dsr_last_error); numeric failure of an object is NOT an error — it is
 *     reported per object in dsr_object_out.is_good (reference convention,
 *     optimizer.py:132-152);
 *   - the caller owns all host buffers for the duration of a call; the library
 *     owns device memory; calls are synchronous unless stated otherwise;
 *   - a context is bound to one HIP device and is not thread-safe (the reference's
 *     callers are serialized on the GIL, include/System.h:57-71).
 */
#ifndef DSR_H
#define DSR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSR_ABI_VERSION 12
#define DSR_MAX_LAYERS 16
#define DSR_CODE_LEN 64

typedef struct dsr_ctx dsr_ctx;
typedef struct dsr_decoder dsr_decoder;
typedef struct dsr_batch dsr_batch;

/* Architecture of a DeepSDF decoder (replaces deep_sdf/deep_sdf_decoder.py:10-72 as
 * configured by specs.json through deep_sdf/workspace.py:202-223): dims [512]*8, latent
 * re-injection at lin4, ReLU, final self.th tanh, CodeLength 64 or 32, and the module's
 * use_tanh / xyz_in_all / LayerNorm switches (weight-norm or plain linear layers are folded by
 * the caller).  Anything else is rejected with an error (never silently approximated). */
typedef struct {
  int code_len;                   /* CodeLength (64) */
  int n_layers;                   /* number of lin{i} (9 for dims=[512]*8) */
  int out_dim[DSR_MAX_LAYERS];    /* rows of lin{i}.weight */
  int in_dim[DSR_MAX_LAYERS];     /* cols of lin{i}.weight */
  int latent_in;                  /* index of the layer that takes cat([x, input]) (4) */
  int use_tanh;                   /* NetworkSpecs.use_tanh: tanh after lin8, before the final tanh
                                     (deep_sdf_decoder.py:65-67, 93-94) — 0 or 1 */
  int xyz_in_all;                 /* NetworkSpecs.xyz_in_all (:46-47, 89-90): hidden layers but lin3 have
                                     509 outputs, every layer input but lin0's / lin4's is [h | xyz] — 0 or 1.
                                     Either variant runs the split-fp16 kernels and never the lite pass
                                     (dsr_decoder_info.lite_eligible 0) */
  int norm_mask;                  /* ABI 9: bit j = nn.LayerNorm(out_dim_j) between lin{j} and its ReLU
                                     (weight_norm=False with j in norm_layers, :58-63, 96-102; eps 1e-5).
                                     The weight buffer then continues, for each such j in order, with
                                     bn{j}.weight (gamma, out_dim_j) and bn{j}.bias (beta, out_dim_j).
                                     Split-fp16 kernels only, never the lite pass.  0 for DSP-SLAM's decoders */
} dsr_decoder_desc;

/* Optimizer hyper-parameters (reconstruct/optimizer.py:27-43; configs/config_*.json
 * "optimizer" block). */
typedef struct {
  float k1, k2, k3, k4;           /* render, sdf, code-reg, rotation-prior weights */
  float b1, b2;                   /* Huber thresholds render / sdf */
  float lr;                       /* joint_optim.learning_rate */
  float s_damp;                   /* joint_optim.scale_damping */
  int num_iterations;             /* joint_optim.num_iterations */
  int code_len;                   /* must equal the decoder's code_len */
  int num_depth_samples;          /* M (50), <= 64 */
  float cut_off;                  /* cut_off_threshold (0.01) */
  int pose_only_iterations;       /* pose_only_optim.num_iterations (5) */
} dsr_optim_params;

/* One object handed to Optimizer.reconstruct_object(t_cam_obj, pts, rays, depth,
 * code) — optimizer.py:90. */
typedef struct {
  float t_cam_obj[16];            /* initial object->camera Sim(3), row-major */
  const float* pts;               /* (n_pts,3) surface points, camera frame */
  int n_pts;
  const float* rays;              /* (n_rays,3) ray directions, fg rays first */
  int n_rays;
  const float* depth;             /* (n_depth,) observed depth of the fg rays */
  int n_depth;                    /* n_fg; n_rays - n_depth background rays */
  const float* code;              /* (code_len,) warm-start code or NULL (=zeros) */
  int pose_is_obj_cam;            /* 1: t_cam_obj[] already holds t_obj_cam (teacher forcing) */
} dsr_object_in;

enum {
  DSR_OK = 0,
  DSR_FAIL_SDF_NAN = 1,           /* optimizer.py:137-138 */
  DSR_FAIL_RENDER_FEW = 2,        /* loss.py:86-88 -> optimizer.py:144-145 */
  DSR_FAIL_RENDER_NAN = 3         /* optimizer.py:151-152 (includes K == 0) */
};

typedef struct {
  float t_cam_obj[16];            /* optimized object->camera (valid iff is_good) */
  float code[DSR_CODE_LEN];       /* optimized code (valid iff is_good) */
  float loss;                     /* k1*render + k2*sdf of the last iteration, pre-update */
  int is_good;
  int fail_reason;                /* DSR_FAIL_* */
  int iters_done;                 /* completed GN updates */
  int n_valid_last, k_last;       /* ray samples in the unit ball / render points, last iter */
} dsr_object_out;

/* Optional per-iteration trace for tests (teacher-forced parity).  Arrays are
 * [num_iterations] (H: [num_iterations][71*71]) for ONE object; the caller
 * allocates. */
typedef struct {
  float* H;                       /* damped normal matrix that is inverted (optimizer.py:188) */
  float* b;                       /* right-hand side */
  float* dx;                      /* inv(H) b */
  float* loss;                    /* k1*render+k2*sdf */
  float* sdf_loss;
  float* render_loss;
  int* n_valid;
  int* k;
  float* t_obj_cam;               /* [num_iterations][16] state the iteration started from */
  float* z;                       /* [num_iterations][code_len] */
  /* ABI 11 (may be NULL): the iteration's work counts — ray samples decoded by the render passes
     (early ray termination: every sample in front of a ray's first certainly-full one, plus
     those its pass window held behind it) and samples re-decoded exactly after the lite pass */
  int* n_decoded;
  int* n_refined;
} dsr_trace;

typedef struct {
  double fwd_ms;                  /* summed device time of the ray-sample decoder kernel */
  double jac_ms;                  /* summed device time of the fwd+Jacobian kernel */
  double total_ms;                /* wall (device events) of the last run */
  int64_t fwd_points;             /* ray samples decoded (early ray termination skips the
                                     samples behind a ray's first sdf <= -cut_off) */
  int64_t jac_points;             /* sum of (N + K) */
  int fwd_launches, jac_launches; /* fwd: one per render pass per iteration */
  int64_t inball_points;          /* sum over iterations/objects of N_valid (in-ball samples) */
  int lite;                       /* 1: fwd_* is the one-product lite pass (DSR_LITE) and
                                     refine_* the exact split-fp16 re-decode of its band */
  int refine_launches;
  double refine_ms;
  int64_t refine_points;
  double lite_max_err;            /* max |lite - exact| over the re-decoded samples (band and
                                     audited), all objects */
  double lite_min_margin;         /* smallest classification margin the last run used */
  int64_t jac_surface_points;     /* of jac_points: surface points N (forward + backward) */
  int64_t jac_render_points;      /* of jac_points: render points K (backward only when
                                     keep_masks, else forward + backward) */
  int keep_masks;                 /* 1: render points reuse the exact pass's ReLU masks */
  int lite_audit_violations;      /* audited out-of-band samples whose exact class (full /
                                     band / empty) differed from the lite pass's */
  int lite_redo_objects;          /* objects that discarded an iteration for a violation and
                                     finished with exact decoding */
  int surface_in_exact;           /* 1: the exact pass ran the surface points' forward too and
                                     the Jacobian kernel only backward chains (kept masks) */
  int64_t audit_points;           /* out-of-band samples re-decoded exactly as an audit */
  int lite_broken_blocks;         /* staggered lite-pass workgroups whose bounded event wait
                                     expired in the last run (their samples all went to the
                                     exact pass: results stay exact, the cost rises); 0 expected */
  int test_hooks;                 /* 1: the batch was created with DSR_TEST_HOOKS=1, so the test
                                     hooks (DSR_LITE_PERTURB / _BREAK) and the lite-guard settings
                                     below (DSR_LITE_AUDIT / _SHELL / _AUDIT_LOG2 / _MARGIN / _FLOOR /
                                     _SAFETY) were read from the environment */
  /* ---- the lite pass's guard as this batch ran it (ABI 8) ---- */
  int lite_eligible;              /* the decoder passed its load-time lite qualification
                                     (dsr_decoder_info); 0: every batch decodes exactly */
  int audit;                      /* 1: audited out-of-band samples (lite_flag) */
  float audit_shell;              /* certain audit of |y| < th + (1 + shell) * margin */
  int audit_log2;                 /* plus a hashed 2^-audit_log2 share of all other samples */
  float lite_margin0;             /* first-iteration margin */
  float lite_floor;               /* later margins: max(floor, safety x largest observed error) */
  float lite_safety;
  int graph_captures;             /* hipGraph captures / replays over the batch's life */
  int graph_replays;
  /* ---- the kernels and launch structure this batch ran (ABI 10) ---- */
  int n_groups;                   /* object groups on concurrent streams (DSR_STREAMS or the default) */
  int graph_mode;                 /* 0 eager, 1 DSR_GRAPH=1 (re-runs replay a graph), 2 a
                                     DSR_BATCH_GRAPH capacity batch */
  int fwd_variant;                /* exact-pass kernel (12: split-fp16, the shipped kernel) */
  int jac_variant;                /* Jacobian kernel (12: split-fp16) */
  int lite_variant;               /* lite-pass kernel (3544 shipped; 0 when the lite pass is off) */
  int split_ring;                 /* A-ring depth of the split kernels (2 shipped).  Only under
                                     DSR_TEST_HOOKS=1 can DSR_FWD_VARIANT / _JAC_VARIANT /
                                     _LITE_VARIANT / _SPLIT_RING move these from the shipped values.
                                     ABI 11: the four are the kernels the last run DISPATCHED
                                     (recorded as it was enqueued), not the environment's values */
  int prescan;                    /* ABI 11: 1 if the render passes ran over the ray chunks
                                     (k_sample_scan / k_sample_count + k_sample_emit; one-group
                                     batches), 0 for one workgroup per object (k_sample_pass) */
} dsr_stats;

/* ---- context ------------------------------------------------------------- */
int dsr_abi_version(void);
int dsr_ctx_create(int device, dsr_ctx** out);
int dsr_ctx_destroy(dsr_ctx* ctx);
const char* dsr_last_error(const dsr_ctx* ctx);
int dsr_device_count(int* n);

/* ---- decoder: replaces deep_sdf.workspace.config_decoder (workspace.py:202-223)
 * + reconstruct.utils.get_decoder (utils.py:93-94).  `weights` holds the folded
 * (weight-norm applied, W = g*v/||v||) layers back to back: for each layer i,
 * W_i (out_dim x in_dim, row-major) then b_i (out_dim). */
int dsr_decoder_load(dsr_ctx* ctx, const dsr_decoder_desc* desc, const float* weights,
                     size_t n_floats, dsr_decoder** out);
int dsr_decoder_free(dsr_ctx* ctx, dsr_decoder* dec);

/* Load-time qualification of the one-product fp16 classification pass (no reference
 * counterpart; it guards the build's replacement of decode_sdf, loss_utils.py:51-79, in the
 * render term's occupancy classification, loss.py:98-102 / loss_utils.py:40-48).
 * dsr_decoder_load decodes a fixed probe set — probe_points points uniform in the unit ball x
 * probe_codes latent codes (zero, then N(0, s^2) per component for s = 0.1, 0.3, 1.0) — with
 * the lite pass and with the exact split-fp16 pass and records, over every probe value, the
 * largest |lite - exact| / max(floor, ||exact| - th|) (th = 0.01, floor = 0.002): the lite
 * error as a fraction of the distance of the exact value to the nearest class boundary
 * (full | band | empty), and the largest |lite - exact| near the surface (|exact| < 0.1).  A
 * decoder whose ratio exceeds 0.5, or whose near-surface error exceeds half the floor (1e-3), is
 * lite-ineligible: every batch on it decodes every ray sample exactly (the DSR_LITE=0 path,
 * reported in dsr_stats). */
typedef struct {
  int code_len;
  int lite_eligible;
  double lite_probe_ratio;        /* max |lite - exact| / max(floor, ||exact| - th|) */
  double lite_probe_max_err;      /* max |lite - exact| over probe values with |exact| < 0.1 */
  double lite_probe_max_err_all;  /* max |lite - exact| over every probe value */
  int probe_points, probe_codes;
  double probe_ms;                /* host wall time of the qualification */
} dsr_decoder_info;
int dsr_decoder_info_get(const dsr_decoder* dec, dsr_decoder_info* info);

/* ---- joint shape + pose GN: replaces Optimizer.reconstruct_object
 * (optimizer.py:90-205) for n_obj independent objects in one device pass.
 * `trace` may be NULL; if not, it must point to n_obj dsr_trace records. */
int dsr_reconstruct_batch(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p,
                          int n_obj, const dsr_object_in* in, dsr_object_out* out,
                          const dsr_trace* trace);

/* ---- joint shape + pose GN over several views of one object: Optimizer.reconstruct_object
 * (optimizer.py:90-205) with the residuals of V >= 1 cameras pooled into ONE code and ONE pose
 * (no reference counterpart as a call: the mono caller re-runs the single-view fit every 5
 * keyframes with a warm start, LocalMapping_util.cc:284-295, :394; callers detect this entry
 * point by its symbol, the ABI number is unchanged).
 * View 0 is the reference view: t_cam_obj, the result pose and the upright prior (loss.py:169-192)
 * are in its camera frame and its t_view_ref must be the identity.  View v sees
 * x_view = t_view_ref . x_ref (rigid) and brings its own pts / rays / depth in ITS camera frame,
 * laid out as in dsr_object_in (pts may be empty).  Per iteration, with T = t_obj_ref and
 * C_v = inverse(t_view_ref_v) (fp64 on the host, rounded once): every view's depth range,
 * samples (optimizer.py:122-128), SDF and render residuals and Jacobians (loss.py:22-43,
 * :60-166) are taken under T_v = T . C_v (T_0 = T itself); the reference updates
 * t_obj_cam <- exp(dx) t_obj_cam (optimizer.py:192) and differentiates at object-frame points
 * (loss.py:38, :162), so all views' rows are derivatives with respect to the same 71 parameters
 * and J_sdf / r_sdf (N = sum N_v) and J_render / r_render (K = sum K_v) are their
 * concatenations; Huber weights, the means, the loss, the priors, the damping and the solve
 * (optimizer.py:157-194) are applied to the pooled sets unchanged, the rotation prior once, at T.
 * T <- exp_sim3(lr dx[:7]) T, z <- z + lr dx[7:], and every T_v is re-derived from the new T.
 * Numeric failures are the reference's, per object: a view with < 10 in-ball samples
 * (DSR_FAIL_RENDER_FEW, the lowest such view in fail_view), N == 0 over all views
 * (DSR_FAIL_SDF_NAN), K == 0 over all views (DSR_FAIL_RENDER_NAN; failures of the pooled terms
 * are reported as view 0's); one view without points or without render points is fine.
 * With n_views == 1 everywhere the results are bitwise those of dsr_reconstruct_batch.
 * out[i] is the reference view's record with n_valid_last / k_last summed over the views;
 * trace (NULL or n_obj records) holds the pooled H, b, dx and losses, the summed counts and the
 * reference view's t_obj_cam and z; fail_view (NULL or n_obj ints) the view that failed each
 * object, -1 if none; stats (NULL or one record) the statistics of the underlying batch, whose
 * members are the views.  Errors (not numeric failures): n_views < 1, a t_view_ref that is not
 * rigid (last row not 0 0 0 1, R^T R - I beyond 1e-4, a reflection), and every input
 * dsr_batch_create rejects. */
typedef struct {
  float t_view_ref[16];           /* rigid reference-camera -> this camera, row-major */
  const float* pts;               /* (n_pts,3) surface points, this view's camera frame */
  int n_pts;
  const float* rays;              /* (n_rays,3) ray directions, fg rays first */
  int n_rays;
  const float* depth;             /* (n_depth,) observed depth of the fg rays */
  int n_depth;
} dsr_view_in;

typedef struct {
  float t_cam_obj[16];            /* initial object->reference-camera Sim(3), row-major */
  const float* code;              /* (code_len,) warm-start code or NULL (=zeros) */
  int pose_is_obj_cam;            /* 1: t_cam_obj[] already holds t_obj_cam (teacher forcing) */
  int n_views;                    /* V >= 1 */
  const dsr_view_in* views;       /* views[0]: the reference view */
} dsr_views_object_in;

int dsr_reconstruct_views(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, int n_obj,
                          const dsr_views_object_in* in, dsr_object_out* out,
                          const dsr_trace* trace,   /* NULL or n_obj records */
                          int* fail_view,           /* NULL or n_obj: failing view, -1 if none */
                          dsr_stats* stats);        /* NULL or the underlying batch's stats */

/* Resident batches for benchmarking / streaming (inputs uploaded once; a run
 * re-initializes the optimizer state on device and executes all iterations on
 * the context stream). */
int dsr_batch_create(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p,
                     int n_obj, const dsr_object_in* in, dsr_batch** out);
int dsr_batch_run(dsr_batch* b);                  /* async on the context stream; with
                                                      DSR_GRAPH=1 re-runs replay a hipGraph */
int dsr_batch_graph(dsr_batch* b);                /* capture that graph now (DSR_GRAPH=1) */
int dsr_batch_sync(dsr_batch* b);
int dsr_batch_query(dsr_batch* b);                /* 1: the last run has finished, 0: still in
                                                      flight (host work can overlap it), <0 error */
int dsr_batch_download(dsr_batch* b, dsr_object_out* out);
int dsr_batch_stats(dsr_batch* b, dsr_stats* st);
/* Diagnostics of the staggered lite pass (no reference counterpart): copies up to n ints of
 * the last run's record — [0] broken workgroups, [1] 1 if the first expired event wait was
 * recorded, then its workgroup, wave, counter, target, observed value, tile iteration,
 * HW_ID, XCC_ID, and how many polls took how many 100 MHz ticks before it expired
 * (csrc/dsr_dev.hpp: STD_*; 16 ints). */
int dsr_batch_lite_diag(dsr_batch* b, int* rec, int n);
/* Render-pass windows of the early ray termination (no reference counterpart): *adaptive = 1 if
 * every object re-chooses its windows each iteration from where its rays terminated in the one
 * before (the default for lite-pass batches on their default multi-pass schedule; results do not
 * depend on the windows), 0 for the batch's fixed schedule; *n_bounds = passes + 1.  bounds, when
 * not NULL, receives [n_obj][*n_bounds] in-ball-rank boundaries (0 ... M) as the last run left
 * them (the batch must have run). */
int dsr_batch_windows(dsr_batch* b, int* adaptive, int* n_bounds, int* bounds);
int dsr_batch_destroy(dsr_batch* b);

/* Fixed-capacity batches for a keyframe stream (BASELINE config 5; the per-keyframe loop
 * LocalMapping_util.cc:256-445 / :165-206, overlapped with LocalMapping.cc:99-128): the batch
 * is laid out once for max_obj objects of at most max_pts surface points and max_rays rays,
 * and dsr_batch_refill uploads each keyframe's objects into those slots (host -> pinned
 * staging -> one stream-ordered copy per input buffer) and rewrites the per-slot counts in
 * device memory, so every kernel argument stays fixed.  With DSR_BATCH_GRAPH the whole GN run
 * is captured as ONE hipGraph at the first run and every later run — after any refill —
 * replays it (dsr_stats.graph_captures / graph_replays).  The batch starts empty; a run needs
 * a refill first; dsr_batch_download returns the current fill's n_obj records.  A refill
 * orders after the previous run's work on the context stream. */
#define DSR_BATCH_GRAPH 1
int dsr_batch_create_capacity(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, int max_obj,
                              int max_pts, int max_rays, int flags, dsr_batch** out);
int dsr_batch_refill(dsr_batch* b, int n_obj, const dsr_object_in* in);

/* ---- decoder queries: replaces decode_sdf / get_batch_sdf_jacobian
 * (loss_utils.py:51-113) as used by Optimizer.compute_sdf_loss_objectpoint_zhjd
 * (optimizer.py:207-213) and MeshExtractor.extract_mesh_from_code
 * (optimizer.py:224-233).  pts are decoder-frame xyz; jac (n x (code_len+3)) may
 * be NULL. */
int dsr_sdf_eval(dsr_ctx* ctx, const dsr_decoder* dec, const float* code, const float* pts,
                 int n, float* sdf, float* jac);

/* ---- mesh extraction: replaces MeshExtractor (optimizer.py:216-233) with
 * convert_sdf_voxels_to_mesh (utils.py:119-140).  `grid_pts` is the (vol_dim^3 x 3)
 * voxel grid of reconstruct.utils.create_voxel_grid (uploaded once, like the reference's
 * MeshExtractor.__init__); dsr_mesher_run decodes it with `code`, runs marching cubes
 * at `level` on device and copies out vertices (n_verts x 3, float) and faces
 * (n_faces x 3, int).  Worst-case capacities: 3*vol_dim^3 vertices and
 * 5*(vol_dim-1)^3 faces; on a smaller capacity the counts are still returned with
 * status -5 and nothing is copied. */
typedef struct dsr_mesher dsr_mesher;
int dsr_mesher_create(dsr_ctx* ctx, const dsr_decoder* dec, const float* grid_pts, int vol_dim,
                      dsr_mesher** out);
int dsr_mesher_run(dsr_mesher* m, const float* code, float level, float* verts, int vcap, int* faces,
                   int fcap, int* n_verts, int* n_faces);
int dsr_mesher_destroy(dsr_mesher* m);

/* ---- batched mesh extraction (ABI 12): the meshes of n_codes codes (n_codes x code_len floats)
 * from one call, bitwise those of n_codes dsr_mesher_run calls.  The codes run in passes of up to
 * 16 slots (fewer when a pass's device buffers would exceed 2 GiB), each pass on the context
 * stream with one host synchronisation: one lite (fp16) decode of all grids settles the
 * predicate v < level away from the surface, whole 64-point tiles of dsr_mesher_run's tiling are
 * decoded exactly where a lite value lies within the margin of the level or next to a sign
 * change, audited tiles guard the margin, and a slot the audit rejects is decoded exactly in
 * full.  Decoders that are not lite-eligible (dsr_decoder_info) and runs under
 * DSR_MESH_LITE=0 decode every tile exactly; batching and the single synchronisation remain.
 * Vertices and faces of all meshes come back concatenated: mesh i owns vertices
 * [vert_off[i], vert_off[i+1]) and faces [face_off[i], face_off[i+1]), face indices local to
 * their mesh.  vcap / fcap are total capacities; when one is too small the offsets are still
 * filled, the status is -5 and nothing is copied.  n_codes == 0 returns at once. */
int dsr_mesher_run_batch(dsr_mesher* m, int n_codes, const float* codes, float level, float* verts,
                         int vcap, int* faces, int fcap, int* vert_off, int* face_off);

/* the last dsr_mesher_run_batch call of a mesher */
typedef struct {
  int n_codes;
  int n_passes;
  int slots;                      /* codes per pass the mesher's buffers hold */
  int sign_pass;                  /* 1: the lite pass ran; 0: every tile decoded exactly (decoder not
                                     lite-eligible, or DSR_MESH_LITE=0) */
  float margin;                   /* m: band half-width around the level (0.01) */
  int lite_tiles;                 /* 128-point tiles of the lite pass */
  int all_tiles;                  /* 64-point tiles of all codes' grids */
  int exact_tiles;                /* of which decoded exactly by the band pass (needed + audit) */
  int audit_tiles;                /* ... decoded as audit only */
  int redo_tiles;                 /* tiles decoded by the redo of rejected codes */
  int violations;                 /* decoded voxels outside the band whose exact side of the level
                                     differs from the lite side */
  int redone_codes;               /* codes redone with every tile exact (a violation, or a lite
                                     error above margin / 4) */
  int lite_broken_blocks;         /* lite-pass workgroups whose event wait expired (dsr_stats) */
  int test_hooks;                 /* DSR_TEST_HOOKS=1 was set: DSR_LITE_PERTURB etc. were honoured */
  double max_lite_err;            /* max |lite - exact| over the decoded voxels */
  double lite_ms, exact_ms, mc_ms;   /* device events: fold + lite pass; mark, exact passes and
                                        merge; marching cubes (summed over the passes) */
} dsr_mesher_stats;
int dsr_mesher_stats_get(const dsr_mesher* m, dsr_mesher_stats* st);

/* diagnostic: slot `slot` of the last pass of the last dsr_mesher_run_batch call — its lite volume
 * and final (merged) volume (vol_dim^3 floats each) and the flags of its 64-point tiles
 * (ceil(vol_dim^3 / 64) bytes: 1 = needed, 2 = audit, 0 = left to the lite value).  Any output may
 * be NULL; the lite volume and the flags exist only when the sign pass ran (-2 otherwise). */
int dsr_mesher_peek(dsr_mesher* m, int slot, float* lite_vol, float* final_vol, unsigned char* tile_flags);

/* ---- marching cubes on a caller's volume: replaces convert_sdf_voxels_to_mesh
 * (utils.py:119-140) called on its own.  `vol` is the (vol_dim, vol_dim, vol_dim) SDF
 * volume in C order (vol[(i*vol_dim + j)*vol_dim + k] at voxel (i, j, k), the order
 * MeshExtractor's grid decode produces it in); vertices come back as voxel index x 2/(vol_dim-1)
 * - 1 (the reference's spacing and origin shift), faces as vertex indices.  Same kernels,
 * capacities and -5 status as dsr_mesher_run; device scratch lives for the call only. */
int dsr_mc_volume(dsr_ctx* ctx, const float* vol, int vol_dim, float level, float* verts, int vcap,
                  int* faces, int fcap, int* n_verts, int* n_faces);

/* ---- sphere-traced depth / instance / normal images of reconstructed objects: replaces
 * ObjectRenderer::SetupCamera / Render (src/ObjectRenderer.cc:82-125, the reference's mesh +
 * OpenGL rasteriser, include/Renderer.hpp) with a tracer over the decoder itself — no mesh, no
 * grid (DESIGN.md 3.6b states the algorithm exactly).  Callers detect these entry points by
 * symbol; the ABI number is unchanged.
 * Camera: pinhole, zero skew; pixel (u, v) (integers) has the ray ((u-cx)/fx, (v-cy)/fy, 1), so
 * the depth image holds z-depth, the convention of dsr_object_in.depth. */
typedef struct { int width, height; float fx, fy, cx, cy; } dsr_camera;
/* zeros = defaults: hit_eps 1e-4, max_steps 48, damp 1, near 0.01; normals != 0 renders normals */
typedef struct { float hit_eps; int max_steps; float damp; float near; int normals; } dsr_render_params;
typedef struct {
  float t_cam_obj[16];            /* object->camera Sim(3), row-major */
  const float* code;              /* (code_len,) */
} dsr_render_object;
enum {
  DSR_RENDER_OK = 0,
  DSR_RENDER_OFFSCREEN = 1,       /* the ball's rectangle misses the image: a valid object, zero rays */
  DSR_RENDER_SKIP_NEAR = 2        /* the ball reaches in front of the near plane: skipped, zero rays */
};
typedef struct {
  int status;                     /* DSR_RENDER_* */
  int rect[4];                    /* u_min, v_min, u_max, v_max (inclusive); 0, 0, -1, -1 without rays */
  int n_rays;                     /* pixels of the rectangle */
  int n_ball;                     /* rays that enter the unit ball */
  int n_hit;                      /* rays that found the surface */
  int n_unconverged;              /* rays still marching after max_steps (counted as misses) */
  int n_visible;                  /* the object's pixels in the final instance image */
} dsr_render_object_out;
typedef struct {
  int n_obj, n_passes;
  int steps_run;                  /* 1 + the last march step that had a live ray */
  long long decoded;              /* decoder evaluations of the march: sum over steps of the live rays */
  int max_live_last;              /* live rays that entered that last step */
  double setup_ms, march_ms, resolve_ms;   /* device events, summed over the passes; resolve
                                              includes the normal pass */
} dsr_render_stats;

typedef struct dsr_renderer dsr_renderer;
/* Replaces ObjectRenderer::SetupCamera (src/ObjectRenderer.cc:82-125): binds a camera and the ray
 * buffers for 2 x width x height rays to a decoder.  Errors: null arguments, non-positive image
 * size or focal length (checked before the device is touched). */
int dsr_renderer_create(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_camera* cam, dsr_renderer** out);
/* Replaces ObjectRenderer::Render (src/ObjectRenderer.cc:82-125) for n_obj objects at once:
 * depth (height x width float32, 0 where nothing was hit), instance (height x width int32, the
 * index of the nearest hit object, -1 where none; ties go to the lower index), normals (NULL or
 * height x width x 3, camera frame, unit, 0 where nothing was hit; filled only when
 * params->normals != 0), per_obj (NULL or n_obj records).  Objects are taken in input order into
 * passes whose rectangles fit the ray buffers; the whole march of a pass is enqueued without a
 * host round trip and synchronised once.  Every sample is decoded exactly (k_mlp_fwd16), and the
 * images are bitwise reproducible and independent of which other objects share the call.
 * Errors: null arguments, max_steps outside 1..256, hit_eps < 0 (0 = default), a t_cam_obj whose
 * last row is not 0 0 0 1 or whose determinant is <= 0.  n_obj == 0 returns an empty image. */
int dsr_renderer_render(dsr_renderer* r, const dsr_render_params* params, int n_obj,
                        const dsr_render_object* objs, float* depth, int* instance, float* normals,
                        dsr_render_object_out* per_obj);
/* the last dsr_renderer_render call (no counterpart in ObjectRenderer::Render, src/ObjectRenderer.cc:82-125) */
int dsr_renderer_stats_get(const dsr_renderer* r, dsr_render_stats* st);
int dsr_renderer_destroy(dsr_renderer* r);
/* Host only, no device: the rectangles (n_obj x 4, as dsr_render_object_out.rect) and statuses
 * (n_obj) dsr_renderer_render will use — the image bounds ObjectRenderer::SetupCamera / Render
 * (src/ObjectRenderer.cc:82-125) leave to OpenGL's clipping.  The ball of object i has centre
 * c = t_cam_obj[:3,3] and radius rho = det(R)^(1/3); c_z - rho < near skips it; otherwise
 * u_min = floor(cx + fx min), u_max = ceil(cx + fx max) over (c_x -+ rho) / (c_z -+ rho), the same
 * for v, clipped to the image.  near <= 0 means the default 0.01.  Returns < 0 for a bad argument
 * or pose (no message: there is no context). */
int dsr_render_layout(const dsr_camera* cam, float near, int n_obj, const dsr_render_object* objs,
                      int* rect, int* status);

/* ---- scene SDF queries: world points against every map object at once.  Replaces the per-object
 * loop of MapObject::compute_sdf_loss / compute_sdf_loss_of_all_inside_points
 * (src/MapObject_util.cc:9-69) over Optimizer.compute_sdf_loss_objectpoint_zhjd
 * (reconstruct/optimizer.py:207-213), and the per-vertex, per-object collision check of the RRT
 * planner (src/NbvGenerator.cpp:320-327, commented out in the reference) with one resident query
 * (DESIGN.md 3.6c states the algorithm exactly).  Callers detect these entry points by symbol; the
 * ABI number is unchanged.
 *
 * Object i: T_ow = inverse(t_world_obj) in fp64 (adjugate / determinant) rounded once to fp32 as
 * A (3x3) and t, s = det(R)^(1/3) rounded once.  Pair (p, i): x_k = fmaf(A_k0, p_x, fmaf(A_k1, p_y,
 * fmaf(A_k2, p_z, t_k))), r2 = fmaf(x_0, x_0, fmaf(x_1, x_1, x_2 * x_2)); the pair is a candidate
 * iff r2 < 1.0f (the in-ball rule of reconstruct/loss.py:82 on the squared norm); a point with a
 * non-finite coordinate is in no ball.  Object i's candidates, in point order, are decoded exactly
 * (k_mlp_fwd16) in 64-point tiles from the first, f; d = s * f. */
typedef struct {
  float t_world_obj[16];          /* object->world Sim(3), row-major (MapObject::Sim3Two, src/MapObject_util.cc:9-69) */
  const float* code;              /* (code_len,) (MapObject::vShapeCode, src/MapObject_util.cc:9-69) */
} dsr_scene_object;
typedef struct {
  int n_in;                       /* points inside this object's unit ball (candidates) */
  int n_win;                      /* points whose nearest object this is */
  int n_neg;                      /* candidates with f < 0 (inside the surface) */
  int n_nan;                      /* candidates whose decoded value is NaN (never win, not summed) */
  double sum_sdf;                 /* sum of f over the candidates: sum_sdf / n_in is
                                     compute_sdf_loss_objectpoint_zhjd (reconstruct/optimizer.py:207-213) on them */
  double sum_abs;                 /* sum of |f| */
} dsr_scene_object_out;
typedef struct {
  int n_obj, n_pts, n_passes;
  long long pairs;                /* n_obj x n_pts */
  long long decoded;              /* candidates (decoder evaluations of the value pass) */
  long long winners;              /* points in at least one ball */
  double bin_ms, decode_ms, resolve_ms, grad_ms;   /* device events, summed over the passes */
} dsr_scene_stats;

typedef struct dsr_scene dsr_scene;
/* The resident buffers of a map of at most max_obj objects queried with at most max_pts points
 * (the object list of src/MapObject_util.cc:9-69's callers).  Errors, before the device is
 * touched: null arguments, max_obj < 1, max_pts < 1 or > 2^24. */
int dsr_scene_create(dsr_ctx* ctx, const dsr_decoder* dec, int max_obj, int max_pts, dsr_scene** out);
/* The map's objects (MapObject::Sim3Two and vShapeCode, src/MapObject_util.cc:9-69): uploads the
 * inverse poses and folds every code on the device once; queries do not repeat it.  Errors,
 * returned before the device is touched: null arguments, n_obj outside 0..max_obj, a last row that
 * is not 0 0 0 1, a determinant <= 0, a non-finite pose entry or code. */
int dsr_scene_set_objects(dsr_scene* sc, int n_obj, const dsr_scene_object* objs);
/* compute_sdf_loss_objectpoint_zhjd (reconstruct/optimizer.py:207-213) of every object at n_pts
 * world points (n x 3), and the nearest object of every point — the collision check of
 * src/NbvGenerator.cpp:320-327: dist[p] = min_i s_i f_i(x) over the balls that hold p, obj[p] its
 * object (ties go to the lower index; +inf and -1 in no ball), grad (NULL or n x 3) the world-frame
 * gradient R g of dist (0 where nothing won), per_obj (NULL or n_obj records).  Bitwise
 * reproducible and independent of which other objects share the call.  Errors: null arguments,
 * n_pts outside 0..max_pts, a query before dsr_scene_set_objects. */
int dsr_scene_query(dsr_scene* sc, int n_pts, const float* pts_world, float* dist, int* obj, float* grad,
                    dsr_scene_object_out* per_obj);
/* Diagnostic: object `obj`'s candidates of the last query, in point order — their point indices,
 * object-frame coordinates and decoded f (the inside points of src/MapObject_util.cc:9-69).  Any
 * output may be NULL.  *n is the count; cap too small returns it with status -5 and copies nothing
 * (dsr_mesher_run's convention).  Error: an object outside the last query. */
int dsr_scene_peek(dsr_scene* sc, int obj, int cap, int* idx, float* x_obj, float* sdf, int* n);
/* the last dsr_scene_query call (no counterpart in src/MapObject_util.cc:9-69) */
int dsr_scene_stats_get(const dsr_scene* sc, dsr_scene_stats* st);
int dsr_scene_destroy(dsr_scene* sc);
/* Host only, no context, no device: the binning rule above for object `obj` of objs — its
 * candidates' point indices (idx, cap) and coordinates (x_obj, cap x 3) in point order, their
 * count *n_in and *scale = s (the inside test of src/MapObject_util.cc:9-69 made exact).  Any
 * output may be NULL; cap too small returns the count with status -5.  Returns -2 for a bad
 * argument or pose (no message: there is no context). */
int dsr_scene_bin_host(int n_obj, const dsr_scene_object* objs, int n_pts, const float* pts_world, int obj,
                       int cap, int* idx, float* x_obj, int* n_in, float* scale);

/* ---- frame ingest: one depth image + one instance-label image + a list of detections -> every
 * detection's surface points, rays and observed depths (the dsr_object_in arrays), on the host or
 * straight into the slots of a capacity batch on the device.  Replaces the per-detection numpy of
 * FrameWithLiDAR.get_detections + pixels_sampler (reconstruct/kitti_sequence.py:70-92, :139-146,
 * :200-210), Frame.pixels_sampler (reconstruct/mono_sequence.py:51-73) and get_rays
 * (reconstruct/loss_utils.py:23-37) for the RGB-D case: the images are what dsr_renderer_render
 * emits.  DESIGN.md 3.5b states the rule exactly; callers detect these entry points by symbol, the
 * ABI number is unchanged.  Out of scope: the occlusion masks of kitti_sequence.py:177-216 and
 * lens distortion (the camera is dsr_camera: pinhole, zero skew, no distortion).
 *
 * Per detection: mask pixels are those with instance == label, valid pixels the mask pixels with
 * z == z && z > near && z < far, both in row-major order.  sel(i, n, N) = (i (N-1)) / (n-1) in
 * 64-bit integers (0 for n = 1), applied only when N > n — np.linspace(0, N-1, n).astype(int32)
 * made exact (the integer rule is the specification; the float idiom differs from it where fp64
 * i * step lands just below an integer).  n_pts = n_fg = min(n_valid, max_pts); surface point and
 * foreground ray i come from valid pixel sel(i, max_pts, n_valid) = (u, v) of depth z: in fp32,
 * one correctly rounded operation each, rx = ((float)u - cx) / fx, ry = ((float)v - cy) / fy, ray
 * (rx, ry, 1), point (rx z, ry z, z), observed depth z — the pixel convention of dsr_camera, not
 * bitwise get_rays' fp64 inverse-K product.  Background rays (pixels_sampler): the box (l, t, r, b),
 * inclusive, is bbox clamped to the image when bbox[2] >= bbox[0], else the tight box of the mask;
 * it grows by `expand` (l = l > e ? l - e : 0, r = r < W-1-e ? r + e : W-1, the same for t, b); the
 * grid has gh = (b-t+1) / downsample rows t + sel(j, gh, b-t+1) and gw = (r-l+1) / downsample
 * columns l + sel(k, gw, r-l+1); its pixels in (j, k) order with instance != label are the N_bg
 * candidates, of which min(N_bg, max_bg) are kept by sel(i, max_bg, N_bg).  Rays are laid out
 * foreground first; background rays have observed depth 0 (as dsr_batch_refill).  Two detections
 * may carry the same label (the flipped hypothesis of LocalMapping_util.cc:400-410): they get the
 * same pixels.  A detection that is not DSR_FRAME_OK yields an empty object (no points, no rays:
 * the reference's numeric failure). */
typedef struct {
  int max_pts;                    /* surface points = foreground rays kept per detection (250) */
  int max_bg;                     /* background rays kept per detection (200) */
  int downsample;                 /* background grid stride (4) */
  int expand;                     /* box growth in pixels (5) */
  int min_mask_area;              /* masks of at most this many pixels are skipped (1000) */
  float near, far;                /* valid depth is near < z < far (0.01, +inf) */
} dsr_frame_params;
typedef struct {
  int label;                      /* the detection's value in the instance image */
  int bbox[4];                    /* l, t, r, b inclusive; bbox[2] < bbox[0]: the mask's tight box */
  float t_cam_obj[16];            /* as dsr_object_in */
  const float* code;              /* as dsr_object_in: (code_len,) or NULL */
  int pose_is_obj_cam;            /* as dsr_object_in */
} dsr_frame_det;
enum {
  DSR_FRAME_OK = 0,
  DSR_FRAME_NO_MASK = 1,          /* no pixel carries the label */
  DSR_FRAME_SMALL_MASK = 2,       /* n_mask <= min_mask_area (kitti_sequence.py:200) */
  DSR_FRAME_NO_DEPTH = 3          /* n_valid == 0 */
};
typedef struct {
  int status;                     /* DSR_FRAME_* */
  int n_mask, n_valid;
  int n_pts, n_bg;                /* rows written: n_pts points / depths, n_pts + n_bg rays (0 unless OK) */
  int box[4];                     /* the expanded box; 0, 0, -1, -1 when there is none (no mask and
                                     no given box, or a given box that misses the image) */
  int grid_h, grid_w;             /* gh, gw of that box (0 without one) */
} dsr_frame_det_out;

/* Host only: max_pts 250, max_bg 200, downsample 4, expand 5, min_mask_area 1000, near 0.01,
 * far +inf (the reference's sampler settings, kitti_sequence.py:70-92 / mono_sequence.py:51-73).
 * The other calls take every value literally: there is no "0 means default". */
int dsr_frame_params_default(dsr_frame_params* p);
/* The rule in plain C++ on the host — no context, no device (replaces get_detections /
 * pixels_sampler / get_rays, kitti_sequence.py:70-92, mono_sequence.py:51-73, loss_utils.py:23-37).
 * depth, instance: height x width.  Fixed strides per detection: pts max_pts x 3, rays
 * (max_pts + max_bg) x 3, dobs max_pts; rows beyond a detection's counts are left untouched; out:
 * n_det records.  Returns < 0 (no message: there is no context) for null images, a non-positive
 * image size or focal length, max_pts < 1, max_bg < 0, downsample < 1, expand < 0, n_det < 0. */
int dsr_frame_inputs_host(const dsr_camera* cam, const dsr_frame_params* params, const float* depth,
                          const int* instance, int n_det, const dsr_frame_det* dets, float* pts, float* rays,
                          float* dobs, dsr_frame_det_out* out);
/* The same arrays and records produced by the device kernels (k_frame_*, csrc/dsr_frame.hpp) and
 * copied back: bitwise those of dsr_frame_inputs_host (pixels_sampler / get_rays as above). */
int dsr_frame_inputs(dsr_ctx* ctx, const dsr_camera* cam, const dsr_frame_params* params, const float* depth,
                     const int* instance, int n_det, const dsr_frame_det* dets, float* pts, float* rays,
                     float* dobs, dsr_frame_det_out* out);
/* dsr_batch_refill from a frame (get_detections, kitti_sequence.py:139-146, without the host
 * arrays): the images go through pinned staging onto the context stream, ordered after the
 * previous run; the kernels write slot i's pts / rays / dobs rows and its counts in device memory
 * for detection i; poses, codes and pose_is_obj_cam are taken as dsr_batch_refill takes them;
 * slots >= n_det are empty.  No kernel argument of the run changes, so a DSR_BATCH_GRAPH graph
 * stays valid.  Errors, returned before the device is touched: a batch that is not a capacity
 * batch, n_det above its slot count, max_pts above its max_pts, max_pts + max_bg above its
 * max_rays, and the argument errors of dsr_frame_inputs_host.  The image buffers grow with the
 * image size, belong to the batch and are freed with it. */
int dsr_batch_refill_frame(dsr_batch* b, const dsr_camera* cam, const dsr_frame_params* params,
                           const float* depth, const int* instance, int n_det, const dsr_frame_det* dets);
/* Waits for the last dsr_batch_refill_frame and copies its n_det records (the ingest outcome
 * get_detections reports by dropping detections, kitti_sequence.py:200-210); an error when the
 * batch's last fill was not a frame. */
int dsr_batch_frame_info(dsr_batch* b, dsr_frame_det_out* out);

/* ---- frame ingest with cuboid start poses and outlier removal (DESIGN.md 3.5c states the rule
 * exactly; callers detect these entry points by symbol, the ABI number is unchanged).  On the
 * reference's mono / RGB-D path no 3-D detector supplies t_cam_obj; the start pose comes from the
 * object's own 3-D points: MapObject::RemoveOutliersSimple (src/MapObject.cc:249-283) drops points
 * farther than 1.0 from their mean, MapObject::ComputeCuboidPCA_onlyformono (src/MapObject.cc:330-443)
 * builds a PCA cuboid with 5 % / 95 % extents, flags the points outside 1.2 x the box and sets the
 * pose to 0.40 l R | centre, and LocalMapping_util.cc:284-410 leaves the flagged points out of
 * surface_points_cam and the rays, starts reconstruct_object from that pose and, for an object
 * not yet reconstructed, again from the flipped pose (flipped_Two, :402-404).  Here that runs per
 * detection on the rows the ingest above produced, in fp64 on the fp32 rows, every operation
 * rounded individually, sums in one fixed shape (256 strided partials added in index order), so
 * host, device and the numpy restatement agree bitwise.  Out of scope: RemoveOutliersModel
 * (src/MapObject.cc:285-328), occlusion masks, per-class scale factors. */
typedef struct {
  float outlier_radius;           /* pass 1: points farther than this from their mean are dropped
                                     (1.0, MapObject.cc:278); +inf switches the pass off */
  int lo_pct, hi_pct;             /* extents: order statistics at ranks (n lo_pct)/100 and
                                     (n hi_pct)/100, integer division (5, 95; MapObject.cc:387-388) */
  float box_margin;               /* pass 2: points outside box_margin x the box are dropped
                                     (1.2, MapObject.cc:410); +inf switches the pass off */
  float scale_factor;             /* pose scale = scale_factor x l (0.40, MapObject.cc:437) */
  int min_points;                 /* fewer points at any stage: no start pose (50,
                                     LocalMapping_util.cc:333) */
  float up[3];                    /* the camera-frame direction column 1 of R must not oppose
                                     ((0, -1, 0), MapObject.cc:380) */
} dsr_frame_pose_params;
enum {                            /* where a detection's start pose comes from */
  DSR_FRAME_POSE_GIVEN = 0,       /* its t_cam_obj: exactly a detection of dsr_batch_refill_frame */
  DSR_FRAME_POSE_CUBOID = 1,      /* the PCA cuboid of its points (MapObject.cc:330-443) */
  DSR_FRAME_POSE_CUBOID_FLIPPED = 2 /* that pose with columns 0 and 2 negated (LocalMapping_util.cc:402-404) */
};
enum {
  DSR_FRAME_POSE_OK = 0,
  DSR_FRAME_POSE_NOT_ASKED = 1,   /* mode DSR_FRAME_POSE_GIVEN */
  DSR_FRAME_POSE_NO_INPUT = 2,    /* the ingest status is not DSR_FRAME_OK */
  DSR_FRAME_POSE_FEW_POINTS = 3,  /* n_in, n_near or n_kept below min_points */
  DSR_FRAME_POSE_DEGENERATE = 4   /* l == 0 or a non-finite value */
};
typedef struct {
  int status;                     /* DSR_FRAME_POSE_* */
  int n_in;                       /* the ingest's n_pts */
  int n_near;                     /* after pass 1 (0 unless asked and the ingest is OK) */
  int n_kept;                     /* after pass 2 (0 before that stage is reached) */
  double dims[3];                 /* w, h, l (0 before that stage is reached) */
  double eig[3];                  /* eigenvalues of the scatter matrix, ascending (0 before ...) */
  float t_cam_obj[16];            /* the start pose handed to the run: the cuboid's (OK), the
                                     detection's own (NOT_ASKED), else the identity */
} dsr_frame_pose_out;

/* Host only: outlier_radius 1.0, lo_pct 5, hi_pct 95, box_margin 1.2, scale_factor 0.40,
 * min_points 50, up (0, -1, 0): the reference's constants (MapObject.cc:278, :380, :387-388, :410,
 * :437; LocalMapping_util.cc:333).  The other calls take every value literally. */
int dsr_frame_pose_params_default(dsr_frame_pose_params* p);
/* dsr_frame_inputs_host, then the rule of DESIGN.md 3.5c per detection (RemoveOutliersSimple +
 * ComputeCuboidPCA_onlyformono + the point / ray filtering of LocalMapping_util.cc:284-410) in
 * plain C++ — no context, no device.  modes: n_det DSR_FRAME_POSE_* values; the t_cam_obj of a
 * cuboid detection is ignored.  Strides as dsr_frame_inputs_host; for an OK cuboid detection the
 * first n_kept rows of pts / dobs / rays hold the kept points in order and the n_bg background
 * rays follow at ray row n_kept; rows beyond the counted ones are unspecified.  out keeps
 * describing the ingest; pose_out: n_det records.  Returns < 0 for the argument errors of
 * dsr_frame_inputs_host, a null array, an unknown mode, min_points < 1, !(0 <= lo_pct < hi_pct <
 * 100), a non-positive or NaN radius, margin or scale factor (+inf is allowed for radius and
 * margin), a non-finite or zero up. */
int dsr_frame_poses_host(const dsr_camera* cam, const dsr_frame_params* params,
                         const dsr_frame_pose_params* pose_params, const float* depth, const int* instance,
                         int n_det, const dsr_frame_det* dets, const int* modes, float* pts, float* rays,
                         float* dobs, dsr_frame_det_out* out, dsr_frame_pose_out* pose_out);
/* The same arrays and records produced by the device kernels (k_frame_* + k_frame_pose +
 * k_frame_compact, csrc/dsr_frame.hpp) and copied back: bitwise those of dsr_frame_poses_host on
 * every counted row (MapObject.cc:249-283, :330-443 as above). */
int dsr_frame_poses(dsr_ctx* ctx, const dsr_camera* cam, const dsr_frame_params* params,
                    const dsr_frame_pose_params* pose_params, const float* depth, const int* instance,
                    int n_det, const dsr_frame_det* dets, const int* modes, float* pts, float* rays,
                    float* dobs, dsr_frame_det_out* out, dsr_frame_pose_out* pose_out);
/* dsr_batch_refill_frame plus the two kernels (the mono / RGB-D call site,
 * LocalMapping_util.cc:284-410, without host arrays): slot i's rows are compacted in device
 * memory, its counts become n_kept / n_kept + n_bg, and the t_in row of a cuboid detection is
 * written by the device after the staged upload on the same stream (pose_is_obj_cam is ignored
 * for it).  A detection without a start pose (NO_INPUT, FEW_POINTS, DEGENERATE) is an empty
 * object.  No argument of the run changes, so a DSR_BATCH_GRAPH batch keeps replaying one graph.
 * Errors, returned before the device is touched: those of dsr_batch_refill_frame, the parameter
 * errors of dsr_frame_poses_host and an unknown mode. */
int dsr_batch_refill_frame_poses(dsr_batch* b, const dsr_camera* cam, const dsr_frame_params* params,
                                 const dsr_frame_pose_params* pose_params, const float* depth,
                                 const int* instance, int n_det, const dsr_frame_det* dets, const int* modes);
/* Waits for the last dsr_batch_refill_frame_poses and copies its n_det pose records (what
 * LocalMapping_util.cc:333 reports by skipping the object); an error when the batch's last fill
 * was not of this kind.  dsr_batch_frame_info still returns the ingest records. */
int dsr_batch_frame_pose_info(dsr_batch* b, dsr_frame_pose_out* out);

/* ---- LiDAR keyframe ingest: one Velodyne sweep + the 3-D detector's boxes + one instance-label
 * image and its mask list -> every detection's surface points, rays, observed depths and start
 * pose, on the host or straight into the slots of a capacity batch on the device.  Replaces the
 * per-detection numpy of FrameWithLiDAR.get_detections (reconstruct/kitti_sequence.py:99-216: the
 * 3 m cube and widened-box crop :118-138, the sub-sampling :139-143, the camera points and pose
 * :144-146, the projection and mask association :183-198, the background rays :200-210 with
 * pixels_sampler :70-92 and get_rays, reconstruct/loss_utils.py:23-37), whose result the C++ side
 * takes in Tracking::GetObjectDetectionsLiDAR (src/Tracking_util.cc:31-58).  DESIGN.md 3.5d states
 * the rule exactly; callers detect these entry points by symbol, the ABI number is unchanged.
 *
 * Per detection (fp64 on the fp32 inputs, every stored value rounded to fp32 once): c = cos theta,
 * s = sin theta, R = [[c,0,-s],[-s,0,-c],[0,1,0]], o = (x, y, z + h/2), A = R^T, t = -R^T o,
 * lo = trans - radius, hi = trans + radius, e = (m w/2, h/2, m l/2) with m = box_margin, and
 * t_cam_obj = t_cam_velo [m l/2 R | o] (kitti_sequence.py:145-146 scales by the widened l).  A
 * sweep point p is near when lo_k < p_k < hi_k for all k and in when also -e_k < x_k < e_k with
 * x_k = fmaf(A_k0, p_x, fmaf(A_k1, p_y, fmaf(A_k2, p_z, t_k))) in fp32 (strict inequalities; a NaN
 * coordinate is in nothing).  The in-points in sweep order are the n_crop candidates; n_pts =
 * min(n_crop, max_pts) rows are kept, row i from candidate sel(i, n_pts, n_crop) (the integer sel of
 * the frame ingest above).  A row's surface point is q = t_cam_velo p (the same nested fmaf), its
 * observed depth q_z, its foreground ray (q_x / q_z, q_y / q_z, 1).  Rows with q_z > 0 whose pixel
 * (fmaf(fx, r_x, cx), fmaf(fy, r_y, cy)) lies strictly inside (0, W) x (0, H) are the n_proj
 * projected rows; each counts one hit for the first mask-list entry whose label the instance image
 * carries at the truncated pixel.  The first entry with the most hits is matched when 2 hits >
 * n_proj.  Background rays come from the matched mask exactly as the frame ingest draws them from a
 * detection's label and box, and follow the foreground rays with observed depth 0.  Points, rays,
 * depths and t_cam_obj are written for every detection (the reference returns surface_points and
 * T_cam_obj for unmatched instances too; estimate_pose_cam_obj consumes them,
 * LocalMapping_util.cc:103-110); background rays only when the status is DSR_LIDAR_OK, and in a
 * batch slot a detection that is not OK is an empty object (the reference's rays = None,
 * LocalMapping_util.cc:173).  Out of scope: the occlusion masks of kitti_sequence.py:177-216
 * (computed, never read) and the depth-order sort :112-113 that only feeds them, overlapping masks
 * (a label image holds one label per pixel), the detectors themselves, and get_colored_pts. */
#define DSR_LIDAR_MAX_MASKS 256
typedef struct {
  int max_pts;                    /* surface points = foreground rays kept per detection (250, num_lidar_max) */
  int max_bg;                     /* background rays kept per detection (200) */
  int downsample;                 /* background grid stride (4) */
  int expand;                     /* box growth in pixels (5) */
  int min_mask_area;              /* masks of at most this many pixels are skipped (1000) */
  float radius;                   /* half edge of the cube around trans (3.0, kitti_sequence.py:125) */
  float box_margin;               /* widening of w and l (1.1, kitti_sequence.py:133-134) */
} dsr_lidar_params;
typedef struct {
  int label;                      /* the mask's value in the instance image */
  int bbox[4];                    /* l, t, r, b inclusive; bbox[2] < bbox[0]: the mask's tight box */
} dsr_lidar_mask;
typedef struct {
  float trans[3];                 /* box centre x, y and bottom z, velodyne frame (a PointPillars row) */
  float size[3];                  /* w, l, h */
  float theta;                    /* heading */
  const float* code;              /* as dsr_object_in: (code_len,) or NULL */
} dsr_lidar_det;
enum {
  DSR_LIDAR_OK = 0,
  DSR_LIDAR_BEHIND = 1,           /* t_cam_obj[2][3] <= 0 (is_front, kitti_sequence.py:154, :181) */
  DSR_LIDAR_NO_POINTS = 2,        /* n_crop == 0 */
  DSR_LIDAR_NO_MATCH = 3,         /* no mask holds more than half of the projected rows (:195) */
  DSR_LIDAR_SMALL_MASK = 4        /* n_mask_px <= min_mask_area (:200) */
};
typedef struct {
  int status;                     /* DSR_LIDAR_*: the first condition that applies, in the enum's order */
  int n_near, n_crop;             /* sweep points in the cube / also in the widened box */
  int n_pts;                      /* rows written: points, depths and foreground rays (every status) */
  int n_proj;                     /* rows projected into the image */
  int mask;                       /* index of the matched mask-list entry, or -1 */
  int n_hits;                     /* hits of the first entry with the most (0 without masks) */
  int n_mask_px;                  /* pixels carrying the matched label (0 unmatched) */
  int n_bg;                       /* background rays written (0 unless OK) */
  int box[4];                     /* the matched mask's expanded box; 0, 0, -1, -1 when there is none */
  int grid_h, grid_w;
  float t_cam_obj[16];
} dsr_lidar_det_out;

/* Host only: max_pts 250, max_bg 200, downsample 4, expand 5, min_mask_area 1000, radius 3.0,
 * box_margin 1.1 (kitti_sequence.py:70-92, :125, :133-134, :141, :203).  Every other call takes the
 * values literally. */
int dsr_lidar_params_default(dsr_lidar_params* p);
/* The rule in plain C++ on the host — no context, no device (replaces get_detections,
 * kitti_sequence.py:99-216).  velo: n_velo rows of stride >= 3 floats, x y z first (KITTI's .bin is
 * stride 4); t_cam_velo: 4 x 4 row-major, rigid; instance: height x width; masks: n_masks entries
 * (a label listed twice is only ever matched by its first entry).  Fixed strides per detection as
 * dsr_frame_inputs_host: pts max_pts x 3, rays (max_pts + max_bg) x 3, dobs max_pts; rows beyond a
 * detection's counts are left untouched; out: n_det records in the caller's order.  Returns < 0
 * (no message: there is no context) for the argument errors of dsr_frame_inputs_host that apply, a
 * t_cam_velo that is not rigid, stride < 3, n_velo < 0 or > 2^24, n_masks outside 0 ..
 * DSR_LIDAR_MAX_MASKS, a non-finite detection field, a size component <= 0, and a radius or
 * box_margin that is not positive and finite. */
int dsr_lidar_inputs_host(const dsr_camera* cam, const dsr_lidar_params* params, const float* t_cam_velo,
                          const float* velo, int n_velo, int stride, const int* instance, int n_masks,
                          const dsr_lidar_mask* masks, int n_det, const dsr_lidar_det* dets, float* pts,
                          float* rays, float* dobs, dsr_lidar_det_out* out);
/* The same arrays and records produced by the device kernels (k_lidar_*, csrc/dsr_lidar.hpp) and
 * copied back: bitwise those of dsr_lidar_inputs_host (get_detections as above). */
int dsr_lidar_inputs(dsr_ctx* ctx, const dsr_camera* cam, const dsr_lidar_params* params,
                     const float* t_cam_velo, const float* velo, int n_velo, int stride, const int* instance,
                     int n_masks, const dsr_lidar_mask* masks, int n_det, const dsr_lidar_det* dets, float* pts,
                     float* rays, float* dobs, dsr_lidar_det_out* out);
/* dsr_batch_refill from a sweep (the KITTI call site: get_detections, kitti_sequence.py:99-216,
 * then CreateNewMapObjects_foronlyStereo, src/LocalMapping_util.cc:156-208, without the host
 * arrays): the sweep, the image, the mask list and the prepared detections go through pinned
 * staging onto the context stream, ordered after the previous run; the kernels write slot i's pts /
 * rays / dobs rows and its counts in device memory for detection i, whose pose row is the rule's
 * t_cam_obj; slots >= n_det and detections that are not DSR_LIDAR_OK are empty objects.  No
 * argument of the run changes, so a DSR_BATCH_GRAPH batch keeps replaying its one graph.  Errors,
 * returned before the device is touched: those of dsr_lidar_inputs_host, a batch that is not a
 * capacity batch, n_det above its slot count, max_pts above its max_pts, max_pts + max_bg above
 * its max_rays.  The buffers grow with the sweep and the image, belong to the batch and are freed
 * with it. */
int dsr_batch_refill_lidar(dsr_batch* b, const dsr_camera* cam, const dsr_lidar_params* params,
                           const float* t_cam_velo, const float* velo, int n_velo, int stride,
                           const int* instance, int n_masks, const dsr_lidar_mask* masks, int n_det,
                           const dsr_lidar_det* dets);
/* Waits for the last dsr_batch_refill_lidar and copies its n_det records (what get_detections
 * reports through num_surface_points, mask and rays = None, kitti_sequence.py:148-157, :195-210);
 * an error when the batch's last fill was not a sweep. */
int dsr_batch_lidar_info(dsr_batch* b, dsr_lidar_det_out* out);

/* ---- multi-GPU from one process: replaces the per-detection loop
 * LocalMapping_util.cc:165-206 spread over devices.  ctx[g] / dec[g] are one context and
 * its decoder per device; objects are LPT-partitioned (cost n_rays*M + n_pts), each
 * device's shard runs on its own host thread, and ONE RCCL gather (ncclCommInitAll over the
 * devices, ncclGather of the fixed-size dsr_object_out records to ctx[0]'s device, ABI 11)
 * returns them; out[] is filled in input order (results bitwise equal to a one-device batch).
 * RCCL is loaded at run time; without it, or when it refuses the device list (two contexts
 * on one device), the records are gathered through host memory: *path (may be NULL) reports
 * DSR_GATHER_RCCL or DSR_GATHER_HOST.  One process per GPU is reconstruct/parallel.py. */
#define DSR_GATHER_HOST 0
#define DSR_GATHER_RCCL 1
int dsr_reconstruct_multi_ex(dsr_ctx* const* ctx, const dsr_decoder* const* dec, int n_dev,
                             const dsr_optim_params* p, int n_obj, const dsr_object_in* in,
                             dsr_object_out* out, int* path);
int dsr_reconstruct_multi(dsr_ctx* const* ctx, const dsr_decoder* const* dec, int n_dev,
                          const dsr_optim_params* p, int n_obj, const dsr_object_in* in,
                          dsr_object_out* out);   /* = _ex with path NULL */
/* Host-only (no device needed): the multi-device layout — dev[i] the device of object i (LPT),
 * slot[i] its record within that device's shard, *maxn the largest shard (every device's gather
 * slot holds maxn records; object i is record dev[i] * maxn + slot[i] of the gathered buffer). */
int dsr_gather_layout(int n_obj, const dsr_object_in* in, int num_depth_samples, int n_dev, int* dev,
                      int* slot, int* maxn);

/* ---- pose-only SE(3) GN: replaces Optimizer.estimate_pose_cam_obj
 * (optimizer.py:46-87).  t_co_se3: 4x4 SE(3) camera<-object, scale: object scale,
 * result written to t_out (4x4). */
int dsr_pose_only(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p,
                  const float* t_co_se3, float scale, const float* pts, int n_pts,
                  const float* code, float* t_out);

/* Batched form for the stereo path's per-keyframe loop over associated objects
 * (LocalMapping_util.cc:103-110 calls estimate_pose_cam_obj once per object): every
 * object's pose-only GN in one device pass per iteration.  t_out: n_obj x 16. */
typedef struct {
  float t_co_se3[16];             /* SE(3) camera<-object */
  float scale;
  const float* pts;               /* (n_pts,3) camera frame */
  int n_pts;
  const float* code;              /* (code_len,) */
} dsr_pose_in;
int dsr_pose_only_batch(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p,
                        int n_obj, const dsr_pose_in* in, float* t_out);

/* ---- resident object tracker: dsr_pose_only_batch as a handle.  Replaces the
 * loop of LocalMapping::GetNewObservations_onyforStereo (src/LocalMapping_util.cc:84-154), which
 * calls Optimizer.estimate_pose_cam_obj (reconstruct/optimizer.py:46-87) once per detection that
 * is associated with a map object, passing the detection's SE(3) pose, the map object's scale and
 * code and the detection's LiDAR surface points.  The handle owns every device block and the
 * pinned staging of a run from its creation; a call stages its inputs, enqueues everything on the
 * context stream — descriptors, tile table and the iteration-4 inlier filter (optimizer.py:77-79)
 * are device kernels, csrc/dsr_track.hpp — and returns; nothing between the staged upload and
 * the final copy into the pinned block waits on the host.  The points of a call are host rows
 * (dsr_tracker_track), or they are written on the device by an ingest's kernels from a Velodyne
 * sweep (dsr_tracker_track_lidar) or from a depth image and its instance labels
 * (dsr_tracker_track_frame).  The poses are bitwise those of dsr_pose_only_batch on the same rows.
 * Callers detect these entry points by symbol; the ABI number is unchanged. */
typedef struct dsr_tracker dsr_tracker;
enum {
  DSR_TRACK_OK = 0,
  DSR_TRACK_NO_POINTS = 1,        /* n_pts == 0: the reference's J^T J / 0, a NaN pose */
  DSR_TRACK_NO_INLIERS = 2        /* the filter kept nothing (optimizer.py:77-79): a NaN pose */
};
typedef struct {
  int status;                     /* DSR_TRACK_* */
  int n_pts;                      /* points the GN started with */
  int n_inliers;                  /* points the filter kept; n_pts when it does not run (optimizer.py:77) */
  int n_near, n_crop;             /* the ingest's counts.  A sweep call: n_near, n_crop of dsr_lidar_det_out;
                                     a frame call: n_mask, n_valid of dsr_frame_det_out; host rows: 0 */
} dsr_track_out;
typedef struct {
  float scale;                    /* the map object's scale (pMO->scale, LocalMapping_util.cc:110) */
  int pose_given;                 /* != 0: t_co_se3 is the start pose (e.g. Tcw Two of :106); a frame call needs it */
  float t_co_se3[16];             /* SE(3) camera<-object; read only with pose_given */
} dsr_track_det;
/* A tracker of at most max_obj objects x max_pts points per call, for the decoder and the
 * pose-only settings of p (pose_only_iterations, code_len; optimizer.py:46-87).  Nothing but two
 * ingest blocks is allocated after this call: the sweep block of dsr_tracker_track_lidar, which
 * grows with the largest sweep seen, and the image block of dsr_tracker_track_frame, which grows
 * with the largest image seen.  Errors: a null argument, max_obj < 1, max_pts outside 1 .. 2^20, max_obj x
 * max_pts above 2^22, a code_len mismatch. */
int dsr_tracker_create(dsr_ctx* ctx, const dsr_decoder* dec, const dsr_optim_params* p, int max_obj,
                       int max_pts, dsr_tracker** out);
/* Waits for the context stream, then frees the handle's blocks. */
int dsr_tracker_destroy(dsr_tracker* tr);
/* estimate_pose_cam_obj (optimizer.py:46-87) for n_obj objects given as host rows — the loop of
 * LocalMapping_util.cc:103-110 as one call — enqueued on the context stream; a call made while
 * the previous one is in flight is ordered after it.  Errors, returned before the device is
 * touched (the handle stays usable): a null argument, n_obj outside 1 .. max_obj, an object with
 * n_pts < 0 or > max_pts, a scale that is not positive and finite, a non-finite pose. */
int dsr_tracker_track(dsr_tracker* tr, int n_obj, const dsr_pose_in* in);
/* The same from a sweep: detection i's points are the rows DESIGN.md 3.5d gives it (the cube and
 * widened-box crop, the integer sel, q = t_cam_velo p; kitti_sequence.py:118-146), written by the
 * ingest's crop kernels into the tracker's point block; association, masks, background rays and
 * the camera play no part (the reference tracks a detection whether or not a mask matched,
 * LocalMapping_util.cc:103-110).  Of params only max_pts (<= the tracker's), radius and
 * box_margin are read; dets[i].code is the map object's code; prior[i] carries its scale and
 * optionally a start pose — without one the start pose is dsr_lidar_track_prep_host's
 * (det->SE3Tco, src/ObjectDetection.cc:29-37).  Errors, returned before the device is touched: a
 * null argument, n_det outside 1 .. max_obj, those of dsr_lidar_inputs_host for the fields that
 * are read, a scale that is not positive and finite, a non-finite given pose. */
int dsr_tracker_track_lidar(dsr_tracker* tr, const dsr_lidar_params* params, const float* t_cam_velo,
                            const float* velo, int n_velo, int stride, int n_det, const dsr_lidar_det* dets,
                            const dsr_track_det* prior);
/* The same from a depth image and an instance-label image (the RGB-D path, which has no sweep):
 * detection i's points are exactly the surface-point rows DESIGN.md 3.5b gives it — the pixels
 * with instance == label and near < z < far in row-major order, n_pts = min(n_valid, max_pts), row
 * k from valid pixel sel(k, max_pts, n_valid) as (rx z, ry z, z) — written by the ingest's kernels
 * into the tracker's point block.  No ray, observed depth, background grid or box is written and
 * no background pass runs.  Of params only max_pts (<= the tracker's), min_mask_area, near and far
 * are read; of dets[i] only label and code, the map object's code (not NULL).  prior[i] carries
 * the map object's scale and the start pose: pose_given must be non-zero (there is no 3-D
 * detector on this path; the caller passes Tcw Two, LocalMapping_util.cc:106).  A detection whose
 * ingest status is not DSR_FRAME_OK (no mask, a mask of at most min_mask_area pixels, no valid
 * depth) has n_pts = 0: DSR_TRACK_NO_POINTS and a NaN pose.  Two detections may carry the same
 * label.  The record's n_near, n_crop hold the ingest's n_mask, n_valid.  Ordering as
 * dsr_tracker_track_lidar: the images and the detections go through a pinned block of the handle
 * in one upload on the context stream.  Errors, returned before the device is touched (the handle
 * stays usable): a null argument, n_det outside 1 .. max_obj, max_pts above the tracker's, those
 * of dsr_frame_inputs_host for the fields that are read (image size, focal lengths, max_pts < 1),
 * a null code, pose_given == 0, a scale that is not positive and finite, a non-finite pose. */
int dsr_tracker_track_frame(dsr_tracker* tr, const dsr_camera* cam, const dsr_frame_params* params,
                            const float* depth, const int* instance, int n_det,
                            const dsr_frame_det* dets, const dsr_track_det* prior);
/* 1: the last call has finished, 0: still in flight (as dsr_batch_query), < 0: an error. */
int dsr_tracker_query(dsr_tracker* tr);
/* Waits for the last call and writes its poses (t_out: n x 16, the rotation block divided by the
 * scale, optimizer.py:84-85; NaN for an object that is not DSR_TRACK_OK) and, unless rec is NULL,
 * its n records. */
int dsr_tracker_download(dsr_tracker* tr, float* t_out, dsr_track_out* rec);
/* Host only — no context, no device: the start pose of a sweep call without a given one, the
 * decomposition of the ingest's t_cam_obj that ObjectDetection computes with a determinant and a
 * cube root (src/ObjectDetection.cc:29-37).  With dsr_lidar_inputs_host's quantities and
 * arithmetic (fp64 on the fp32 inputs, every operation rounded on its own, every stored value
 * rounded to fp32 once): t_co_se3[i] (n_det x 16) = t_cam_velo [R | o], each entry the
 * left-to-right sum DESIGN.md 3.5d gives for t_cam_obj with sigma left out, last row 0 0 0 1;
 * det_scale[i] = (float)sigma, sigma = m l / 2.  Of params only box_margin is read.  Returns < 0
 * for a null argument, n_det < 0 and dsr_lidar_inputs_host's errors for box_margin, t_cam_velo
 * and the detections. */
int dsr_lidar_track_prep_host(const dsr_lidar_params* params, const float* t_cam_velo, int n_det,
                              const dsr_lidar_det* dets, float* t_co_se3, float* det_scale);

/* ---- data association: which of a frame's detections are map objects already seen (DESIGN.md
 * 3.6d states the rule exactly).  Replaces Tracking::AssociateObjectsByProjection_onlyformono
 * (src/Tracking_util.cc:210-288), which votes per detection over the object ids of the ORB map
 * points under its mask; ORB-SLAM's map is outside this library, so the evidence here is the depth
 * under the mask and the map's decoders: a detection belongs to the map object whose surface its
 * back-projected points lie on.  Callers detect these entry points by symbol; the ABI number is
 * unchanged.
 *
 * Detection j has n_pts_j camera-frame rows q (from a frame: exactly the surface-point rows
 * DESIGN.md 3.5b gives its label, the points-only ingest of dsr_tracker_track_frame; from host
 * rows: the caller's).  World point w_k = fmaf(B_k0, q_x, fmaf(B_k1, q_y, fmaf(B_k2, q_z, b_k)))
 * with B | b rows 0..2 of t_world_cam, which must be rigid (last row 0 0 0 1, R^T R = I within
 * 1e-4, det R > 0).  Row k of detection j is scene point p = j max_pts + k; slots k >= n_pts_j
 * hold NaN (in no ball); the detection of a point is p / max_pts.  Candidates and decoded values
 * f are exactly dsr_scene_query's on those points.  Three int32 tables [n_det][n_obj]: n_in, the
 * detection's candidates of the object; n_hit, those with fabsf(f) <= inlier_tol (object units,
 * fp32; a NaN f counts in n_in only); n_neg, those with f < -inlier_tol (the measured surface lies
 * inside the model: evidence against the match).  Every detection decides on its own: the best
 * object is the first with the largest n_hit, the runner-up the first of the others with the
 * largest n_hit; the detection is DSR_ASSOC_MATCHED iff n_hit >= min_hits and 100 n_hit > min_pct
 * n_pts_j (integers), else DSR_ASSOC_NEW; n_pts_j == 0 is DSR_ASSOC_NO_POINTS. */
typedef struct {
  float inlier_tol;               /* |f| at most this is a hit (0.05: reconstruct/optimizer.py:78) */
  int min_hits;                   /* hits a match needs at least (20: src/Tracking_util.cc:199) */
  int min_pct;                    /* ... and more than this percentage of the detection's rows (50) */
} dsr_assoc_params;
enum {
  DSR_ASSOC_MATCHED = 0,          /* obj is the map object (the mpMapObjects hit of src/Tracking_util.cc:210-288) */
  DSR_ASSOC_NEW = 1,              /* no object passed: a new object (src/Tracking_util.cc:210-288, the isNew branch) */
  DSR_ASSOC_NO_POINTS = 2         /* n_pts == 0; a frame detection whose ingest status is not DSR_FRAME_OK */
};
typedef struct {
  int status;                     /* DSR_ASSOC_* */
  int n_pts;                      /* the detection's rows */
  int obj;                        /* the matched object; -1 unless DSR_ASSOC_MATCHED */
  int n_hit, n_in, n_neg;         /* the best object's counts, accepted or not (0 on an empty map) */
  int second, second_hit;         /* the runner-up and its n_hit (-1, 0 with fewer than two objects) */
  int ingest_status;              /* a frame call: DSR_FRAME_* of the detection; host rows: 0 */
  int n_mask, n_valid;            /* a frame call: those of dsr_frame_det_out; host rows: 0 */
} dsr_assoc_out;
/* Host only: inlier_tol 0.05, min_hits 20, min_pct 50 (the thresholds of
 * src/Tracking_util.cc:210-288's callers, see the fields).  Every other call takes the values
 * literally. */
int dsr_assoc_params_default(dsr_assoc_params* p);
/* The association of src/Tracking_util.cc:210-288 for the n_det detections of a depth image and
 * its instance labels against the map of dsr_scene_set_objects, in one call on the device: the
 * images and labels go through a pinned block of the scene (it grows with the largest image seen)
 * in one upload, the frame ingest's kernels write the rows, k_assoc_world the world points, the
 * scene's value passes decode the candidates, k_assoc_vote / k_assoc_pick (csrc/dsr_assoc.hpp)
 * write the tables and the records; the host waits once, at the end.  Of frame_params only
 * max_pts, min_mask_area, near and far are read.  out: n_det records; table: NULL or 3 n_det n_obj
 * ints in the order n_in, n_hit, n_neg.  Afterwards dsr_scene_peek and dsr_scene_stats_get speak
 * of this call's n_det max_pts points.  Errors, returned before the device is touched (the handle
 * stays usable): null arguments, a call before dsr_scene_set_objects, n_det < 1, n_det max_pts
 * above the scene's max_pts, a non-rigid or non-finite t_world_cam, the argument errors of
 * dsr_frame_inputs_host for the fields that are read, inlier_tol not positive and finite,
 * min_hits < 1, min_pct outside 0..99.  A map of zero objects is no error: every detection is
 * DSR_ASSOC_NEW or DSR_ASSOC_NO_POINTS and the tables are empty.  Threads: a dsr_scene handle is
 * single-threaded — its calls (set_objects, query, peek, associate_*) share the handle's point,
 * pass and staging buffers and must not overlap; the associate calls additionally hold the
 * context's run lock, as the tracker's calls do, so they are ordered against other handles' runs
 * on the context stream.  A HIP error in the middle of a call drains the stream before it is
 * returned: no copy out of the pinned blocks is left in flight. */
int dsr_scene_associate_frame(dsr_scene* sc, const dsr_camera* cam, const dsr_frame_params* frame_params,
                              const dsr_assoc_params* assoc_params, const float* t_world_cam,
                              const float* depth, const int* instance, int n_det, const int* labels,
                              dsr_assoc_out* out, int* table);
/* The same (src/Tracking_util.cc:210-288) for rows the caller holds, e.g. the LiDAR path's from
 * dsr_lidar_inputs: rows is n_det x max_pts x 3 camera-frame floats of which n_rows[j] rows count
 * for detection j; t_world_cam NULL: the rows are world points already and are taken as they are.
 * Errors as above, and n_rows[j] outside 0..max_pts. */
int dsr_scene_associate_points(dsr_scene* sc, const dsr_assoc_params* assoc_params, const float* t_world_cam,
                               int n_det, int max_pts, const int* n_rows, const float* rows,
                               dsr_assoc_out* out, int* table);
/* Host only, no context, no device: the points dsr_scene_associate_frame queries (the evidence
 * that stands in for the map points of src/Tracking_util.cc:210-288) — the frame's rows
 * transformed into pts_world (n_det x max_pts x 3, NaN beyond a detection's count), the counts
 * n_rows (n_det) and, unless NULL, the ingest records (those of dsr_frame_inputs_host at max_bg 0,
 * downsample 1, expand 0 and the mask's tight box).  Returns -2 for a bad argument. */
int dsr_assoc_points_host(const dsr_camera* cam, const dsr_frame_params* frame_params, const float* t_world_cam,
                          const float* depth, const int* instance, int n_det, const int* labels,
                          float* pts_world, int* n_rows, dsr_frame_det_out* ingest);
/* Host only: the decision of src/Tracking_util.cc:210-288's vote from the tables (3 n_det n_obj
 * ints: n_in, n_hit, n_neg; NULL allowed when n_obj == 0) and the detections' row counts.  The
 * ingest fields of the records are 0.  Returns -2 for a bad argument. */
int dsr_assoc_pick_host(const dsr_assoc_params* assoc_params, int n_det, int n_obj, const int* table,
                        const int* n_rows, dsr_assoc_out* out);

#ifdef __cplusplus
}
#endif
#endif /* DSR_H */
