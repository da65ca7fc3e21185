/*
 * dsr_c_stress.c — every entry point of the C ABI (include/dsr.h) from C, for the host-side
 * sanitizer build (Makefile: dsr_c_stress_asan = this file + libdsr_asan.so, host code under
 * AddressSanitizer + UndefinedBehaviorSanitizer; device code is the normal gfx950 build).
 *
 *   dsr_c_stress               no-device paths: ABI version, argument validation and error
 *                              reporting of every entry point that checks its arguments before
 *                              touching the device, the host rules (dsr_scene_bin_host,
 *                              dsr_assoc_pick_host, dsr_assoc_points_host,
 *                              dsr_lidar_inputs_host, dsr_lidar_track_prep_host) on hand-computed
 *                              inputs, context creation
 *                              (-3 without a device)
 *   dsr_c_stress <dir>         the same inputs as dsr_c_smoke (weights.f32, params.f32,
 *                              objects.bin), then every device entry point with cross-checks:
 *                              one-shot batch twice (bitwise), resident batch create / run /
 *                              query / download / stats / lite diag / destroy, pooled re-create,
 *                              graph capture + replays (DSR_GRAPH=1), multi-context
 *                              reconstruct_multi, sdf_eval with and without the Jacobian,
 *                              pose-only single and batched (including an empty object), the
 *                              mesher (and dsr_mc_volume on its decoded grid) with ample and
 *                              with too small capacities, the batch call (dsr_mesher_run_batch:
 *                              ample and too small totals, n = 0) against it, scene queries
 *                              (dsr_scene_*) against sdf_eval and their records, data association
 *                              (dsr_scene_associate_* against a recount over dsr_scene_peek and
 *                              the frame form against the points form), the LiDAR
 *                              ingest (dsr_lidar_inputs against a hand-computed sweep and the
 *                              host rule, dsr_batch_refill_lidar against dsr_batch_refill), the
 *                              resident tracker (dsr_tracker_* from the same sweep, from host
 *                              rows and from a depth image against dsr_pose_only_batch), forced audit
 *                              violations and their spare-iteration redo (test hooks), and the
 *                              error paths of a live context.  Exit status 0 = every check held.
 */
#define _POSIX_C_SOURCE 200112L   /* setenv / unsetenv */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "dsr.h"

static int n_checks = 0;
#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    ++n_checks;                                                              \
    if (!(cond)) {                                                           \
      fprintf(stderr, "check failed (%s:%d): %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                                          \
      fprintf(stderr, "\n");                                                 \
      exit(20);                                                              \
    }                                                                        \
  } while (0)

static void* slurp(const char* dir, const char* name, size_t* bytes) {
  char path[4096];
  snprintf(path, sizeof path, "%s/%s", dir, name);
  FILE* f = fopen(path, "rb");
  if (!f) return NULL;
  fseek(f, 0, SEEK_END);
  *bytes = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  void* p = malloc(*bytes ? *bytes : 1);
  if (p && fread(p, 1, *bytes, f) != *bytes) { free(p); p = NULL; }
  fclose(f);
  return p;
}

/* DSR_STRESS_SKIP="graph,multi,...": leave sections out (to attribute a sanitizer report) */
static int run_section(const char* name) {
  const char* skip = getenv("DSR_STRESS_SKIP");
  return !(skip && strstr(skip, name));
}

static const dsr_decoder_desc DESC = {64, 9, {512, 512, 512, 445, 512, 512, 512, 512, 1},
                                      {67, 512, 512, 512, 512, 512, 512, 512, 512}, 4, 0, 0};

static int same_out(const dsr_object_out* a, const dsr_object_out* b, int n) {
  return memcmp(a, b, sizeof(dsr_object_out) * (size_t)n) == 0;
}

/* A ten-point sweep around one box whose outcome is computed by hand.  theta = 0
 * and t_cam_velo an axis permutation keep every value exact: box axes x_0 = p_x - 8, x_1 = p_z,
 * x_2 = -p_y with half extents (1.1, 1, 2.2), the cube (5, 11) x (-3, 3) x (-4, 2), camera point
 * q = (-p_y, -p_z, p_x), pixel (16 + 16 q_x / q_z, 12 + 16 q_y / q_z). */
typedef struct {
  dsr_camera cam;
  dsr_lidar_params par;
  float tcv[16];
  float velo[10][4];
  int inst[24 * 32];
  dsr_lidar_mask masks[2];
  dsr_lidar_det det;
} lidar_scene;

static void lidar_scene_make(lidar_scene* s) {
  const dsr_camera cam = {32, 24, 16.f, 16.f, 16.f, 12.f};
  const float tcv[16] = {0, -1, 0, 0, 0, 0, -1, 0, 1, 0, 0, 0, 0, 0, 0, 1};
  const float velo[10][4] = {{8.f, 0.f, 0.f, 0.1f},       /* in: candidate 0 -> row 0, pixel (16, 12) */
                             {8.f, 1.f, 0.5f, 0.2f},      /* in: candidate 1, not picked */
                             {8.f, -2.f, -0.5f, 0.3f},    /* in: candidate 2 -> row 1, pixel (20, 13) */
                             {8.f, 2.5f, 0.f, 0.4f},      /* near; x_2 = -2.5 is outside */
                             {9.f, 0.f, 0.5f, 0.5f},      /* in: candidate 3, not picked */
                             {9.5f, 0.f, 0.f, 0.6f},      /* near; x_0 = 1.5 is outside */
                             {8.f, 0.f, 1.f, 0.7f},       /* near; x_1 == e_1 is outside (strict) */
                             {20.f, 0.f, 0.f, 0.8f},      /* not near */
                             {8.f, 3.f, 0.f, 0.9f},       /* p_y == hi_y: not near (strict) */
                             {7.5f, -1.f, -0.25f, 1.f}};  /* in: candidate 4 -> row 2, pixel (18, 12) */
  s->cam = cam;
  dsr_lidar_params_default(&s->par);
  s->par.max_pts = 3;
  s->par.min_mask_area = 100;
  memcpy(s->tcv, tcv, sizeof tcv);
  memcpy(s->velo, velo, sizeof velo);
  for (int v = 0; v < 24; ++v)
    for (int u = 0; u < 32; ++u) s->inst[v * 32 + u] = (u >= 10 && u <= 24 && v >= 8 && v <= 16) ? 7 : -1;   /* 135 pixels */
  const dsr_lidar_mask masks[2] = {{9, {0, 0, -1, -1}}, {7, {0, 0, -1, -1}}};
  memcpy(s->masks, masks, sizeof masks);
  const dsr_lidar_det det = {{8.f, 0.f, -1.f}, {2.f, 4.f, 2.f}, 0.f, NULL};
  s->det = det;
}

/* the hand-computed outcome: 8 near, 5 in, rows from candidates sel(i, 3, 5) = 0, 2, 4, all three
 * projected onto label 7 (entry 1); its tight box (10, 8, 24, 16) grows to (5, 3, 29, 21), the 4 x 6
 * grid has rows 3, 9, 15, 21 and columns 5, 9, 14, 19, 24, 29, of which 6 + 3 + 3 + 6 miss the mask */
static void lidar_scene_check(const float* pts, const float* rays, const float* dobs, const dsr_lidar_det_out* o) {
  CHECK(o->status == DSR_LIDAR_OK && o->n_near == 8 && o->n_crop == 5 && o->n_pts == 3, "lidar counts %d %d %d %d",
        o->status, o->n_near, o->n_crop, o->n_pts);
  CHECK(o->n_proj == 3 && o->mask == 1 && o->n_hits == 3 && o->n_mask_px == 135 && o->n_bg == 18,
        "lidar association %d %d %d %d %d", o->n_proj, o->mask, o->n_hits, o->n_mask_px, o->n_bg);
  CHECK(o->box[0] == 5 && o->box[1] == 3 && o->box[2] == 29 && o->box[3] == 21 && o->grid_h == 4 && o->grid_w == 6,
        "lidar box %d %d %d %d grid %d x %d", o->box[0], o->box[1], o->box[2], o->box[3], o->grid_h, o->grid_w);
  const float want[9] = {0.f, 0.f, 8.f, 2.f, 0.5f, 8.f, 1.f, 0.25f, 7.5f};
  for (int i = 0; i < 9; ++i) CHECK(pts[i] == want[i], "lidar point value %d: %g", i, pts[i]);
  CHECK(dobs[0] == 8.f && dobs[1] == 8.f && dobs[2] == 7.5f, "lidar depths");
  CHECK(rays[0] == 0.f && rays[2] == 1.f && rays[3] == 0.25f && rays[4] == 0.0625f && rays[6] == 1.f / 7.5f,
        "lidar foreground rays %g %g", rays[3], rays[6]);
  CHECK(rays[9] == -0.6875f && rays[10] == -0.5625f && rays[11] == 1.f, "lidar first background ray %g %g", rays[9],
        rays[10]);
  CHECK(rays[3 * 20] == (29.f - 16.f) / 16.f && rays[3 * 20 + 1] == (21.f - 12.f) / 16.f, "lidar last background ray");
  const float sg = 1.1f * 2.f;                      /* box_margin l / 2, exact */
  CHECK(o->t_cam_obj[2] == sg && o->t_cam_obj[5] == -sg && o->t_cam_obj[8] == sg && o->t_cam_obj[11] == 8.f &&
            o->t_cam_obj[0] == 0.f && o->t_cam_obj[3] == 0.f && o->t_cam_obj[7] == 0.f && o->t_cam_obj[15] == 1.f,
        "lidar t_cam_obj %g %g %g %g", o->t_cam_obj[2], o->t_cam_obj[5], o->t_cam_obj[8], o->t_cam_obj[11]);
}

/* the LiDAR ingest without a device: its argument errors and the host rule on the scene above */
static void lidar_no_device_paths(void) {
  lidar_scene s;
  lidar_scene_make(&s);
  float pts[9], rays[3 * 203], dobs[3];
  dsr_lidar_det_out o;
#define LIDAR_HOST(cam_, par_, tcv_, velo_, n_, stride_, inst_, nm_, masks_, nd_, det_) \
  dsr_lidar_inputs_host(cam_, par_, tcv_, velo_, n_, stride_, inst_, nm_, masks_, nd_, det_, pts, rays, dobs, &o)
  for (int i = 0; i < 3 * 203; ++i) rays[i] = -7.f;
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 1, &s.det) == 0, "lidar_inputs_host failed");
  lidar_scene_check(pts, rays, dobs, &o);
  CHECK(rays[3 * 21] == -7.f, "lidar_inputs_host wrote beyond its rows");
  CHECK(dsr_lidar_params_default(NULL) < 0, "lidar_params_default(NULL) accepted");
  CHECK(s.par.max_bg == 200 && s.par.downsample == 4 && s.par.expand == 5 && s.par.radius == 3.f && s.par.box_margin == 1.1f,
        "lidar defaults");
  CHECK(LIDAR_HOST(NULL, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 1, &s.det) < 0, "lidar: NULL camera accepted");
  CHECK(LIDAR_HOST(&s.cam, NULL, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 1, &s.det) < 0, "lidar: NULL params accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, NULL, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 1, &s.det) < 0, "lidar: NULL t_cam_velo accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, NULL, 10, 4, s.inst, 2, s.masks, 1, &s.det) < 0, "lidar: NULL sweep accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, NULL, 2, s.masks, 1, &s.det) < 0, "lidar: NULL image accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, NULL, 1, &s.det) < 0, "lidar: NULL masks accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 1, NULL) < 0, "lidar: NULL detections accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 2, s.inst, 2, s.masks, 1, &s.det) < 0, "lidar: stride 2 accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], -1, 4, s.inst, 2, s.masks, 1, &s.det) < 0, "lidar: n_velo -1 accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], (1 << 24) + 1, 4, s.inst, 2, s.masks, 1, &s.det) < 0,
        "lidar: n_velo 2^24 + 1 accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, -1, s.masks, 1, &s.det) < 0, "lidar: n_masks -1 accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, DSR_LIDAR_MAX_MASKS + 1, s.masks, 1, &s.det) < 0,
        "lidar: n_masks 257 accepted");
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, -1, &s.det) < 0, "lidar: n_det -1 accepted");
  {
    lidar_scene b = s;
    b.tcv[1] = -1.1f;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: scaled t_cam_velo accepted");
    b = s;
    b.tcv[1] = 1.f;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: reflection accepted");
    b = s;
    b.tcv[15] = 2.f;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: last row accepted");
    b = s;
    b.det.theta = NAN;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: NaN theta accepted");
    b = s;
    b.det.trans[1] = INFINITY;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: inf trans accepted");
    b = s;
    b.det.size[2] = 0.f;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: size 0 accepted");
    b = s;
    b.par.radius = 0.f;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: radius 0 accepted");
    b = s;
    b.par.box_margin = INFINITY;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: inf box_margin accepted");
    b = s;
    b.par.max_pts = 0;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: max_pts 0 accepted");
    b = s;
    b.cam.fx = 0.f;
    CHECK(LIDAR_HOST(&b.cam, &b.par, b.tcv, &b.velo[0][0], 10, 4, b.inst, 2, b.masks, 1, &b.det) < 0, "lidar: fx 0 accepted");
  }
  /* an empty sweep and an empty mask list are fine: NO_POINTS; the pose is still recorded */
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, NULL, 0, 4, s.inst, 0, NULL, 1, &s.det) == 0, "lidar: empty sweep refused");
  CHECK(o.status == DSR_LIDAR_NO_POINTS && o.n_pts == 0 && o.mask == -1 && o.t_cam_obj[11] == 8.f, "lidar: empty sweep record");
  /* the whole sweep against an empty mask list: NO_MATCH, rows written all the same */
  pts[8] = -7.f;
  CHECK(LIDAR_HOST(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 0, NULL, 1, &s.det) == 0, "lidar: no masks refused");
  CHECK(o.status == DSR_LIDAR_NO_MATCH && o.n_pts == 3 && o.n_proj == 3 && o.n_hits == 0 && o.n_bg == 0 && pts[8] == 7.5f,
        "lidar: no-mask record");
#undef LIDAR_HOST
  CHECK(dsr_lidar_inputs(NULL, &s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 1, &s.det, pts, rays, dobs, &o) < 0,
        "lidar_inputs(NULL ctx) accepted");
  CHECK(dsr_batch_refill_lidar(NULL, &s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 1, &s.det) < 0,
        "refill_lidar(NULL) accepted");
  CHECK(dsr_batch_lidar_info(NULL, &o) < 0, "lidar_info(NULL) accepted");
  /* the tracker's start pose on the same detection: t_cam_velo [R | o] = the t_cam_obj above without
     its scale, and the scale beside it; then the tracker's calls without a handle */
  float tse3[16], dscale = 0.f;
  CHECK(dsr_lidar_track_prep_host(&s.par, s.tcv, 1, &s.det, tse3, &dscale) == 0, "lidar_track_prep_host failed");
  CHECK(tse3[2] == 1.f && tse3[5] == -1.f && tse3[8] == 1.f && tse3[11] == 8.f && tse3[0] == 0.f && tse3[3] == 0.f &&
            tse3[7] == 0.f && tse3[12] == 0.f && tse3[15] == 1.f && dscale == 1.1f * 2.f,
        "track prep %g %g %g %g scale %g", tse3[2], tse3[5], tse3[8], tse3[11], dscale);
  CHECK(dsr_lidar_track_prep_host(NULL, s.tcv, 1, &s.det, tse3, &dscale) < 0, "track prep: NULL params accepted");
  CHECK(dsr_lidar_track_prep_host(&s.par, NULL, 1, &s.det, tse3, &dscale) < 0, "track prep: NULL t_cam_velo accepted");
  CHECK(dsr_lidar_track_prep_host(&s.par, s.tcv, 1, NULL, tse3, &dscale) < 0, "track prep: NULL detections accepted");
  CHECK(dsr_lidar_track_prep_host(&s.par, s.tcv, 1, &s.det, NULL, &dscale) < 0, "track prep: NULL pose array accepted");
  CHECK(dsr_lidar_track_prep_host(&s.par, s.tcv, 1, &s.det, tse3, NULL) < 0, "track prep: NULL scale array accepted");
  CHECK(dsr_lidar_track_prep_host(&s.par, s.tcv, -1, &s.det, tse3, &dscale) < 0, "track prep: n_det -1 accepted");
  CHECK(dsr_lidar_track_prep_host(&s.par, s.tcv, 0, NULL, NULL, NULL) == 0, "track prep: no detections refused");
  {
    dsr_tracker* tr = NULL;
    dsr_track_out trec;
    dsr_track_det pri = {1.f, 0, {0}};
    CHECK(dsr_tracker_create(NULL, NULL, NULL, 1, 1, &tr) < 0 && tr == NULL, "tracker_create(NULL ctx) accepted");
    CHECK(dsr_tracker_track(NULL, 1, NULL) < 0, "tracker_track(NULL) accepted");
    CHECK(dsr_tracker_track_lidar(NULL, &s.par, s.tcv, &s.velo[0][0], 10, 4, 1, &s.det, &pri) < 0, "tracker_track_lidar(NULL) accepted");
    CHECK(dsr_tracker_track_frame(NULL, &s.cam, NULL, NULL, s.inst, 1, NULL, &pri) < 0, "tracker_track_frame(NULL) accepted");
    CHECK(dsr_tracker_query(NULL) < 0 && dsr_tracker_download(NULL, tse3, &trec) < 0, "tracker query / download(NULL) accepted");
    CHECK(dsr_tracker_destroy(NULL) == 0, "tracker_destroy(NULL)");
  }
}

/* argument validation that needs no device (the CPU-container case) */
static void no_device_paths(void) {
  CHECK(dsr_abi_version() == DSR_ABI_VERSION, "ABI %d", dsr_abi_version());
  int n = -1;
  const int rc = dsr_device_count(&n);
  CHECK(rc == 0 || rc < 0, "device_count %d", rc);
  CHECK(dsr_device_count(NULL) < 0, "device_count(NULL) accepted");
  CHECK(dsr_ctx_create(0, NULL) < 0, "ctx_create(NULL) accepted");
  CHECK(dsr_last_error(NULL) != NULL, "last_error(NULL) is NULL");
  CHECK(dsr_ctx_destroy(NULL) == 0, "ctx_destroy(NULL)");
  CHECK(dsr_batch_destroy(NULL) == 0, "batch_destroy(NULL)");
  CHECK(dsr_batch_run(NULL) < 0 && dsr_batch_sync(NULL) < 0 && dsr_batch_query(NULL) < 0,
        "batch calls on NULL accepted");
  CHECK(dsr_batch_download(NULL, NULL) < 0 && dsr_batch_stats(NULL, NULL) < 0, "batch NULL accepted");
  CHECK(dsr_mesher_destroy(NULL) == 0, "mesher_destroy(NULL)");
  {
    int vo[2], fo[2];
    CHECK(dsr_mesher_run_batch(NULL, 1, NULL, 0.f, NULL, 0, NULL, 0, vo, fo) < 0, "mesher_run_batch(NULL) accepted");
    CHECK(dsr_mesher_run_batch(NULL, -1, NULL, 0.f, NULL, 0, NULL, 0, vo, fo) < 0, "mesher_run_batch(n = -1) accepted");
    CHECK(dsr_mesher_stats_get(NULL, NULL) < 0 && dsr_mesher_peek(NULL, 0, NULL, NULL, NULL) < 0, "mesher NULL accepted");
  }
  CHECK(dsr_batch_refill(NULL, 0, NULL) < 0, "refill(NULL) accepted");
  CHECK(dsr_batch_create_capacity(NULL, NULL, NULL, 1, 1, 1, 0, NULL) < 0, "create_capacity(NULL) accepted");
  CHECK(dsr_decoder_info_get(NULL, NULL) < 0, "decoder_info_get(NULL) accepted");
  {
    float v[8] = {0};
    int nv = 0, nf = 0;
    CHECK(dsr_mc_volume(NULL, v, 2, 0.f, NULL, 0, NULL, 0, &nv, &nf) < 0, "mc_volume(NULL ctx) accepted");
  }
  {
    /* dsr_reconstruct_views validates the views before it needs the device: no views, a scaled,
       a sheared-last-row and a reflected t_view_ref, a reference view that is not the identity —
       and, with every view valid, the missing context */
    static const float pt[3] = {0.f, 0.f, 3.f};
    static const float dep[1] = {3.f};
    dsr_view_in vw[3];
    memset(vw, 0, sizeof(vw));
    for (int v = 0; v < 3; ++v) {
      for (int i = 0; i < 4; ++i) vw[v].t_view_ref[i * 5] = 1.f;
      vw[v].pts = pt; vw[v].n_pts = 1;
      vw[v].rays = pt; vw[v].n_rays = 1;
      vw[v].depth = dep; vw[v].n_depth = 1;
    }
    vw[1].t_view_ref[3] = 0.5f;                       /* a translation: still rigid */
    vw[2].t_view_ref[0] = 0.f; vw[2].t_view_ref[2] = 1.f;      /* a quarter turn about y */
    vw[2].t_view_ref[8] = -1.f; vw[2].t_view_ref[10] = 0.f;
    dsr_views_object_in vin;
    memset(&vin, 0, sizeof(vin));
    for (int i = 0; i < 4; ++i) vin.t_cam_obj[i * 5] = 1.f;
    vin.n_views = 3;
    vin.views = vw;
    dsr_object_out vout;
    int fv = 7;
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 1, NULL, &vout, NULL, &fv, NULL) < 0, "views: NULL in accepted");
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 1, &vin, NULL, NULL, &fv, NULL) < 0, "views: NULL out accepted");
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 0, &vin, &vout, NULL, &fv, NULL) < 0, "views: n_obj 0 accepted");
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 1, &vin, &vout, NULL, &fv, NULL) < 0, "views: NULL ctx accepted");
    vin.n_views = 0;
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 1, &vin, &vout, NULL, &fv, NULL) < 0, "views: n_views 0 accepted");
    vin.n_views = 3;
    vin.views = NULL;
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 1, &vin, &vout, NULL, &fv, NULL) < 0, "views: NULL views accepted");
    vin.views = vw;
    for (int i = 0; i < 3; ++i) vw[1].t_view_ref[i * 5] = 1.1f;
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 1, &vin, &vout, NULL, &fv, NULL) < 0, "views: scale 1.1 accepted");
    for (int i = 0; i < 3; ++i) vw[1].t_view_ref[i * 5] = 1.f;
    vw[1].t_view_ref[12] = 0.25f;
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 1, &vin, &vout, NULL, &fv, NULL) < 0, "views: last row accepted");
    vw[1].t_view_ref[12] = 0.f;
    vw[1].t_view_ref[0] = -1.f;
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 1, &vin, &vout, NULL, &fv, NULL) < 0, "views: reflection accepted");
    vw[1].t_view_ref[0] = 1.f;
    vw[0].t_view_ref[3] = 0.5f;
    CHECK(dsr_reconstruct_views(NULL, NULL, NULL, 1, &vin, &vout, NULL, &fv, NULL) < 0, "views: moved view 0 accepted");
    CHECK(fv == 7, "views: fail_view written by a rejected call");
  }
  {
    /* the renderer: null arguments, and the host-only rectangle rule (dsr_render_layout) — a
       centred object, one off-screen, one in front of the near plane, then a bad camera, a bad
       last row and a reflected pose */
    dsr_camera cam = {48, 36, 120.f, 120.f, 23.5f, 17.5f};
    dsr_renderer* rr = (dsr_renderer*)&cam;           /* must come back NULL-free: never written */
    CHECK(dsr_renderer_create(NULL, NULL, &cam, &rr) < 0, "renderer_create(NULL ctx) accepted");
    CHECK(dsr_renderer_create(NULL, NULL, NULL, NULL) < 0, "renderer_create(NULL) accepted");
    CHECK(dsr_renderer_destroy(NULL) == 0, "renderer_destroy(NULL)");
    CHECK(dsr_renderer_stats_get(NULL, NULL) < 0, "renderer_stats_get(NULL) accepted");
    CHECK(dsr_renderer_render(NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL) < 0, "renderer_render(NULL) accepted");
    dsr_render_object ro[3];
    memset(ro, 0, sizeof(ro));
    for (int k = 0; k < 3; ++k)
      for (int i = 0; i < 4; ++i) ro[k].t_cam_obj[i * 5] = 1.f;
    ro[0].t_cam_obj[11] = 15.f;
    ro[1].t_cam_obj[3] = 30.f; ro[1].t_cam_obj[11] = 15.f;
    ro[2].t_cam_obj[11] = 1.005f;
    int rect[12], status[3];
    CHECK(dsr_render_layout(&cam, 0.01f, 3, ro, rect, status) == 0, "render_layout failed");
    CHECK(status[0] == DSR_RENDER_OK && status[1] == DSR_RENDER_OFFSCREEN && status[2] == DSR_RENDER_SKIP_NEAR,
          "render_layout statuses %d %d %d", status[0], status[1], status[2]);
    /* (0 -+ 1) / (15 -+ 1) * 120 = -+8.57 about 23.5 / 17.5 */
    CHECK(rect[0] == 14 && rect[1] == 8 && rect[2] == 33 && rect[3] == 27, "render_layout rect %d %d %d %d", rect[0],
          rect[1], rect[2], rect[3]);
    CHECK(rect[4] == 0 && rect[6] == -1 && rect[8] == 0 && rect[11] == -1, "render_layout empty rects");
    CHECK(dsr_render_layout(&cam, 0.01f, 0, NULL, NULL, NULL) == 0, "render_layout(n_obj 0)");
    CHECK(dsr_render_layout(NULL, 0.01f, 0, NULL, NULL, NULL) < 0, "render_layout(NULL camera) accepted");
    CHECK(dsr_render_layout(&cam, 0.01f, 1, ro, NULL, status) < 0, "render_layout(NULL rect) accepted");
    cam.fx = 0.f;
    CHECK(dsr_render_layout(&cam, 0.01f, 1, ro, rect, status) < 0, "render_layout(fx 0) accepted");
    cam.fx = 120.f;
    cam.height = 0;
    CHECK(dsr_render_layout(&cam, 0.01f, 1, ro, rect, status) < 0, "render_layout(height 0) accepted");
    cam.height = 36;
    ro[0].t_cam_obj[15] = 2.f;
    CHECK(dsr_render_layout(&cam, 0.01f, 1, ro, rect, status) < 0, "render_layout(last row) accepted");
    ro[0].t_cam_obj[15] = 1.f;
    ro[0].t_cam_obj[0] = -1.f;
    CHECK(dsr_render_layout(&cam, 0.01f, 1, ro, rect, status) < 0, "render_layout(reflection) accepted");
  }
  {
    /* the scene query: null arguments, and the host-only binning rule (dsr_scene_bin_host) — a
       scale-2 object at the origin and a unit one at x = 3, seven points, then a capacity too
       small, a bad object index, a bad last row, a reflected and a non-finite pose */
    dsr_scene* sc = NULL;
    CHECK(dsr_scene_create(NULL, NULL, 4, 64, &sc) < 0 && sc == NULL, "scene_create(NULL ctx) accepted");
    CHECK(dsr_scene_create(NULL, NULL, 4, 64, NULL) < 0, "scene_create(NULL) accepted");
    CHECK(dsr_scene_destroy(NULL) == 0, "scene_destroy(NULL)");
    CHECK(dsr_scene_set_objects(NULL, 0, NULL) < 0, "scene_set_objects(NULL) accepted");
    CHECK(dsr_scene_query(NULL, 0, NULL, NULL, NULL, NULL, NULL) < 0, "scene_query(NULL) accepted");
    CHECK(dsr_scene_peek(NULL, 0, 0, NULL, NULL, NULL, NULL) < 0, "scene_peek(NULL) accepted");
    CHECK(dsr_scene_stats_get(NULL, NULL) < 0, "scene_stats_get(NULL) accepted");
    dsr_scene_object so[2];
    memset(so, 0, sizeof(so));
    for (int i = 0; i < 3; ++i) so[0].t_world_obj[i * 5] = 2.f;
    for (int i = 0; i < 3; ++i) so[1].t_world_obj[i * 5] = 1.f;
    so[0].t_world_obj[15] = so[1].t_world_obj[15] = 1.f;
    so[1].t_world_obj[3] = 3.f;
    const float inf = INFINITY;
    const float pw[7 * 3] = {0.f, 0.f, 0.f,   1.5f, 0.f, 0.f,   2.5f, 0.f, 0.f,   3.5f, 0.5f, 0.f,
                             0.f, -1.9f, 0.f, inf, 0.f, 0.f,    0.f, NAN, 0.f};
    int idx[7], n_in = -1;
    float xo[7 * 3], scale = 0.f;
    CHECK(dsr_scene_bin_host(2, so, 7, pw, 0, 7, idx, xo, &n_in, &scale) == 0, "scene_bin_host failed");
    CHECK(n_in == 3 && idx[0] == 0 && idx[1] == 1 && idx[2] == 4 && scale == 2.f, "scene_bin_host object 0: %d", n_in);
    CHECK(xo[3] == 0.75f && xo[4] == 0.f && xo[7] == -0.95f, "scene_bin_host coordinates %g %g", xo[3], xo[7]);
    CHECK(dsr_scene_bin_host(2, so, 7, pw, 1, 7, idx, xo, &n_in, &scale) == 0, "scene_bin_host failed (1)");
    CHECK(n_in == 2 && idx[0] == 2 && idx[1] == 3 && scale == 1.f && xo[0] == -0.5f, "scene_bin_host object 1: %d", n_in);
    idx[0] = -9;
    CHECK(dsr_scene_bin_host(2, so, 7, pw, 0, 2, idx, xo, &n_in, NULL) == -5 && n_in == 3 && idx[0] == -9,
          "scene_bin_host(cap 2): count without copying");
    CHECK(dsr_scene_bin_host(2, so, 7, pw, 0, 0, NULL, NULL, &n_in, NULL) == -5 && n_in == 3, "scene_bin_host(count only)");
    CHECK(dsr_scene_bin_host(2, so, 0, NULL, 0, 0, NULL, NULL, &n_in, NULL) == 0 && n_in == 0, "scene_bin_host(n_pts 0)");
    CHECK(dsr_scene_bin_host(2, so, 7, pw, 2, 7, idx, xo, &n_in, &scale) < 0, "scene_bin_host(obj 2) accepted");
    CHECK(dsr_scene_bin_host(0, so, 7, pw, 0, 7, idx, xo, &n_in, &scale) < 0, "scene_bin_host(n_obj 0) accepted");
    CHECK(dsr_scene_bin_host(2, so, 7, NULL, 0, 7, idx, xo, &n_in, &scale) < 0, "scene_bin_host(NULL points) accepted");
    so[1].t_world_obj[15] = 2.f;
    CHECK(dsr_scene_bin_host(2, so, 7, pw, 0, 7, idx, xo, &n_in, &scale) < 0, "scene_bin_host(last row) accepted");
    so[1].t_world_obj[15] = 1.f;
    so[1].t_world_obj[0] = -1.f;
    CHECK(dsr_scene_bin_host(2, so, 7, pw, 0, 7, idx, xo, &n_in, &scale) < 0, "scene_bin_host(reflection) accepted");
    so[1].t_world_obj[0] = inf;
    CHECK(dsr_scene_bin_host(2, so, 7, pw, 0, 7, idx, xo, &n_in, &scale) < 0, "scene_bin_host(inf pose) accepted");
  }
  {
    /* data association: null arguments, the defaults, the host pick on a hand-made table (a tie,
       min_pct at equality, no points) and the host points of a 4 x 3 image under a translation */
    dsr_assoc_params ap;
    CHECK(dsr_assoc_params_default(NULL) < 0, "assoc_params_default(NULL) accepted");
    CHECK(dsr_assoc_params_default(&ap) == 0 && ap.inlier_tol == 0.05f && ap.min_hits == 20 && ap.min_pct == 50,
          "assoc defaults");
    dsr_assoc_out ao[3];
    int nr[3] = {40, 60, 0};
    const float eye[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    CHECK(dsr_scene_associate_points(NULL, &ap, eye, 3, 4, nr, eye, ao, NULL) < 0, "associate_points(NULL) accepted");
    CHECK(dsr_scene_associate_frame(NULL, NULL, NULL, &ap, eye, NULL, NULL, 1, nr, ao, NULL) < 0,
          "associate_frame(NULL) accepted");
    /*                     n_in               n_hit              n_neg */
    const int tab[27] = {30, 30, 5,  50, 9, 9,  0, 0, 0,     25, 25, 0,  30, 7, 7,  0, 0, 0,     1, 2, 3,  4, 5, 6,  0, 0, 0};
    CHECK(dsr_assoc_pick_host(&ap, 3, 3, tab, nr, ao) == 0, "assoc_pick_host failed");
    CHECK(ao[0].status == DSR_ASSOC_MATCHED && ao[0].obj == 0 && ao[0].second == 1 && ao[0].second_hit == 25 &&
          ao[0].n_in == 30 && ao[0].n_neg == 1, "pick: a tie goes to the lower index (%d %d)", ao[0].obj, ao[0].second);
    CHECK(ao[1].status == DSR_ASSOC_NEW && ao[1].obj == -1 && ao[1].n_hit == 30 && ao[1].second == 1 && ao[1].second_hit == 7,
          "pick: 100 * 30 == 50 * 60 is not a majority (%d)", ao[1].status);
    CHECK(ao[2].status == DSR_ASSOC_NO_POINTS && ao[2].obj == -1 && ao[2].n_pts == 0, "pick: no points (%d)", ao[2].status);
    CHECK(dsr_assoc_pick_host(&ap, 3, 0, NULL, nr, ao) == 0 && ao[0].status == DSR_ASSOC_NEW && ao[0].second == -1,
          "pick: an empty map");
    CHECK(dsr_assoc_pick_host(NULL, 3, 3, tab, nr, ao) < 0 && dsr_assoc_pick_host(&ap, 0, 3, tab, nr, ao) < 0 &&
          dsr_assoc_pick_host(&ap, 3, 3, NULL, nr, ao) < 0 && dsr_assoc_pick_host(&ap, 3, 3, tab, NULL, ao) < 0 &&
          dsr_assoc_pick_host(&ap, 3, 3, tab, nr, NULL) < 0, "assoc_pick_host(bad argument) accepted");
    dsr_assoc_params bad = ap;
    bad.inlier_tol = 0.f;
    CHECK(dsr_assoc_pick_host(&bad, 3, 3, tab, nr, ao) < 0, "inlier_tol 0 accepted");
    bad = ap; bad.min_hits = 0;
    CHECK(dsr_assoc_pick_host(&bad, 3, 3, tab, nr, ao) < 0, "min_hits 0 accepted");
    bad = ap; bad.min_pct = 100;
    CHECK(dsr_assoc_pick_host(&bad, 3, 3, tab, nr, ao) < 0, "min_pct 100 accepted");
    dsr_camera cam = {4, 3, 2.f, 2.f, 1.f, 1.f};
    dsr_frame_params fp;
    dsr_frame_params_default(&fp);
    fp.max_pts = 3; fp.min_mask_area = 1;
    const float depth[12] = {2.f, 2.f, 0.f, 2.f,   4.f, 2.f, 2.f, 2.f,   2.f, 2.f, 2.f, 8.f};
    const int inst[12] = {5, 5, 5, 0,   5, 0, 0, 0,   0, 0, 0, 5};
    const int labels[2] = {5, 9};
    float tw[16];
    memcpy(tw, eye, sizeof tw);
    tw[3] = 10.f; tw[7] = 20.f; tw[11] = 30.f;
    float pw[2 * 3 * 3];
    int rows[2] = {-1, -1};
    dsr_frame_det_out fo[2];
    CHECK(dsr_assoc_points_host(&cam, &fp, tw, depth, inst, 2, labels, pw, rows, fo) == 0, "assoc_points_host failed");
    /* valid pixels of label 5: (0,0) (1,0) (0,1) (3,2), three of four kept by sel: 0, 1, 3 */
    CHECK(rows[0] == 3 && rows[1] == 0 && fo[0].n_mask == 5 && fo[0].n_valid == 4 && fo[1].status == DSR_FRAME_NO_MASK,
          "assoc_points_host counts %d %d", rows[0], rows[1]);
    CHECK(pw[0] == 9.f && pw[1] == 19.f && pw[2] == 32.f && pw[3] == 10.f && pw[6] == 18.f && pw[7] == 24.f && pw[8] == 38.f,
          "assoc_points_host rows %g %g %g", pw[0], pw[6], pw[8]);
    for (int k = 9; k < 18; ++k) CHECK(pw[k] != pw[k], "assoc_points_host: NaN fill %d", k);
    CHECK(dsr_assoc_points_host(&cam, &fp, NULL, depth, inst, 2, labels, pw, rows, fo) < 0 &&
          dsr_assoc_points_host(&cam, &fp, tw, depth, inst, 0, labels, pw, rows, fo) < 0 &&
          dsr_assoc_points_host(NULL, &fp, tw, depth, inst, 2, labels, pw, rows, fo) < 0, "assoc_points_host(bad argument) accepted");
    tw[0] = -1.f;
    CHECK(dsr_assoc_points_host(&cam, &fp, tw, depth, inst, 2, labels, pw, rows, fo) < 0, "a reflected t_world_cam accepted");
  }
  lidar_no_device_paths();
  dsr_ctx* c = NULL;
  const int rc2 = dsr_ctx_create(-7, &c);
  CHECK(rc2 < 0 && c == NULL, "ctx_create(-7) = %d", rc2);
}

/* error paths of a live context: every one returns < 0 with a message, none crashes */
static void live_error_paths(dsr_ctx* ctx, const dsr_decoder* dec, const float* w, size_t nw,
                             const dsr_optim_params* p, const dsr_object_in* in) {
  dsr_decoder* d2 = NULL;
  dsr_decoder_desc bad = DESC;
  bad.use_tanh = 2;
  CHECK(dsr_decoder_load(ctx, &bad, w, nw, &d2) < 0 && d2 == NULL, "use_tanh 2 accepted");
  CHECK(strlen(dsr_last_error(ctx)) > 0, "no message");
  bad = DESC;
  bad.norm_mask = 0x100;                       /* a LayerNorm after lin8: not a DeepSDF layer */
  CHECK(dsr_decoder_load(ctx, &bad, w, nw, &d2) < 0 && d2 == NULL, "norm_mask 0x100 accepted");
  bad.norm_mask = 1;                           /* lin0's LayerNorm needs 2 x 512 more floats */
  CHECK(dsr_decoder_load(ctx, &bad, w, nw, &d2) < 0 && d2 == NULL, "short LayerNorm weights accepted");
  bad = DESC;
  bad.use_tanh = 1;                            /* a decoder variant: loads, never lite-eligible */
  CHECK(dsr_decoder_load(ctx, &bad, w, nw, &d2) == 0 && d2 != NULL, "use_tanh refused: %s", dsr_last_error(ctx));
  {
    dsr_decoder_info inf;
    CHECK(dsr_decoder_info_get(d2, &inf) == 0 && inf.lite_eligible == 0 && inf.code_len == 64, "use_tanh info");
  }
  CHECK(dsr_decoder_free(ctx, d2) == 0, "free");
  d2 = NULL;
  bad = DESC;
  bad.latent_in = 3;
  CHECK(dsr_decoder_load(ctx, &bad, w, nw, &d2) < 0, "latent_in 3 accepted");
  CHECK(dsr_decoder_load(ctx, &DESC, w, nw - 1, &d2) < 0, "short weights accepted");
  CHECK(dsr_decoder_load(ctx, &DESC, NULL, nw, &d2) < 0, "NULL weights accepted");
  dsr_optim_params q = *p;
  dsr_object_out out[1];
  q.code_len = 32;
  CHECK(dsr_reconstruct_batch(ctx, dec, &q, 1, in, out, NULL) < 0, "code_len mismatch accepted");
  q = *p;
  q.num_depth_samples = 65;
  CHECK(dsr_reconstruct_batch(ctx, dec, &q, 1, in, out, NULL) < 0, "M 65 accepted");
  q = *p;
  q.num_iterations = -1;
  CHECK(dsr_reconstruct_batch(ctx, dec, &q, 1, in, out, NULL) < 0, "iters -1 accepted");
  CHECK(dsr_reconstruct_batch(ctx, dec, p, 0, in, out, NULL) < 0, "n_obj 0 accepted");
  CHECK(dsr_reconstruct_batch(ctx, dec, p, 1, NULL, out, NULL) < 0, "NULL in accepted");
  dsr_batch* b = NULL;
  CHECK(dsr_batch_create(ctx, dec, p, 0, in, &b) < 0 && b == NULL, "empty batch accepted");
  /* more ray samples than 32-bit device offsets hold: refused before any input is read (the
     ray pointer below covers only the real object's rays) */
  dsr_object_in big = in[0];
  big.n_rays = 50000000;
  big.n_depth = 0;
  CHECK(dsr_batch_create(ctx, dec, p, 1, &big, &b) < 0 && b == NULL, "2.5e9-sample batch accepted");
  CHECK(strstr(dsr_last_error(ctx), "too large") != NULL, "%s", dsr_last_error(ctx));
  CHECK(dsr_sdf_eval(ctx, dec, NULL, NULL, 4, NULL, NULL) < 0, "sdf_eval NULLs accepted");
  dsr_mesher* m = NULL;
  CHECK(dsr_mesher_create(ctx, dec, NULL, 8, &m) < 0 && m == NULL, "mesher without grid accepted");
  /* the renderer: refused cameras and parameters, then a 32 x 24 image of two objects (the zero
     code) twice — the same bytes, consistent counts — and an empty call */
  {
    dsr_camera cam = {32, 24, 0.f, 80.f, 15.5f, 11.5f};
    dsr_renderer* r = NULL;
    CHECK(dsr_renderer_create(ctx, dec, &cam, &r) < 0 && r == NULL, "fx 0 accepted");
    CHECK(strlen(dsr_last_error(ctx)) > 0, "no message");
    cam.fx = 80.f;
    cam.width = -4;
    CHECK(dsr_renderer_create(ctx, dec, &cam, &r) < 0 && r == NULL, "width -4 accepted");
    cam.width = 32;
    CHECK(dsr_renderer_create(ctx, dec, &cam, &r) == 0 && r != NULL, "renderer_create: %s", dsr_last_error(ctx));
    static const float zero_code[DSR_CODE_LEN] = {0};
    dsr_render_object ro[2];
    memset(ro, 0, sizeof(ro));
    for (int k = 0; k < 2; ++k) {
      for (int i = 0; i < 3; ++i) ro[k].t_cam_obj[i * 5] = 2.f;      /* scale 2 */
      ro[k].t_cam_obj[15] = 1.f;
      ro[k].t_cam_obj[3] = k ? 1.5f : -1.5f;
      ro[k].t_cam_obj[11] = 10.f + 2.f * k;
      ro[k].code = zero_code;
    }
    dsr_render_params rp;
    memset(&rp, 0, sizeof(rp));                                    /* zeros = defaults */
    float depth[2][32 * 24], nrm[32 * 24 * 3];
    int inst[2][32 * 24];
    dsr_render_object_out po[2];
    rp.max_steps = 257;
    CHECK(dsr_renderer_render(r, &rp, 2, ro, depth[0], inst[0], NULL, po) < 0, "max_steps 257 accepted");
    rp.max_steps = 0;
    rp.hit_eps = -1.f;
    CHECK(dsr_renderer_render(r, &rp, 2, ro, depth[0], inst[0], NULL, po) < 0, "hit_eps -1 accepted");
    rp.hit_eps = 0.f;
    CHECK(dsr_renderer_render(r, &rp, 2, ro, NULL, inst[0], NULL, po) < 0, "NULL depth accepted");
    rp.normals = 1;
    CHECK(dsr_renderer_render(r, &rp, 2, ro, depth[0], inst[0], NULL, po) < 0, "normals without a buffer accepted");
    ro[1].t_cam_obj[15] = 0.f;
    CHECK(dsr_renderer_render(r, &rp, 2, ro, depth[0], inst[0], nrm, po) < 0, "bad last row accepted");
    ro[1].t_cam_obj[15] = 1.f;
    ro[1].code = NULL;
    CHECK(dsr_renderer_render(r, &rp, 2, ro, depth[0], inst[0], nrm, po) < 0, "NULL code accepted");
    ro[1].code = zero_code;
    for (int k = 0; k < 2; ++k)
      CHECK(dsr_renderer_render(r, &rp, 2, ro, depth[k], inst[k], nrm, po) == 0, "render: %s", dsr_last_error(ctx));
    CHECK(memcmp(depth[0], depth[1], sizeof(depth[0])) == 0 && memcmp(inst[0], inst[1], sizeof(inst[0])) == 0,
          "render not reproducible");
    int vis[2] = {0, 0}, none = 0;
    for (int i = 0; i < 32 * 24; ++i) {
      CHECK(inst[0][i] >= -1 && inst[0][i] < 2 && (inst[0][i] < 0) == (depth[0][i] == 0.f), "pixel %d", i);
      if (inst[0][i] >= 0) ++vis[inst[0][i]]; else ++none;
    }
    for (int k = 0; k < 2; ++k) {
      CHECK(po[k].status == DSR_RENDER_OK && po[k].n_visible == vis[k] && po[k].n_hit >= vis[k] && vis[k] > 0,
            "object %d: status %d visible %d / %d hit %d", k, po[k].status, po[k].n_visible, vis[k], po[k].n_hit);
      CHECK(po[k].n_rays >= po[k].n_ball && po[k].n_ball >= po[k].n_hit + po[k].n_unconverged, "object %d counts", k);
    }
    dsr_render_stats rs;
    CHECK(dsr_renderer_stats_get(r, &rs) == 0 && rs.n_obj == 2 && rs.n_passes == 1 && rs.steps_run >= 1 &&
              rs.steps_run <= 48 && rs.decoded >= po[0].n_ball + po[1].n_ball,
          "render stats");
    CHECK(dsr_renderer_render(r, &rp, 0, NULL, depth[1], inst[1], nrm, NULL) == 0, "empty render: %s", dsr_last_error(ctx));
    for (int i = 0; i < 32 * 24; ++i) CHECK(depth[1][i] == 0.f && inst[1][i] == -1, "empty render pixel %d", i);
    CHECK(none > 0, "no empty pixel");
    CHECK(dsr_renderer_destroy(r) == 0, "renderer_destroy");
  }
}

int main(int argc, char** argv) {
  setvbuf(stdout, NULL, _IOLBF, 0);   /* a sanitizer's exit-time report must not swallow it */
  no_device_paths();
  dsr_ctx* ctx = NULL;
  const int rc = dsr_ctx_create(0, &ctx);
  printf("dsr_ctx_create %d\n", rc);
  if (argc < 2) {
    if (ctx) dsr_ctx_destroy(ctx);
    CHECK(rc == 0 || rc == -3, "ctx_create %d", rc);
    printf("stress ok (no-device paths): %d checks\n", n_checks);
    return 0;
  }
  CHECK(rc == 0, "ctx_create %d: %s", rc, dsr_last_error(ctx));
  size_t wb = 0, pb = 0, ob = 0;
  float* w = (float*)slurp(argv[1], "weights.f32", &wb);
  float* pf = (float*)slurp(argv[1], "params.f32", &pb);
  char* objs = (char*)slurp(argv[1], "objects.bin", &ob);
  CHECK(w && pf && objs && pb >= 13 * sizeof(float), "missing inputs in %s", argv[1]);
  const size_t nw = wb / sizeof(float);
  dsr_decoder* dec = NULL;
  CHECK(dsr_decoder_load(ctx, &DESC, w, nw, &dec) == 0, "decoder_load: %s", dsr_last_error(ctx));
  const dsr_optim_params p = {pf[0], pf[1], pf[2], pf[3], pf[4], pf[5], pf[6], pf[7], (int)pf[8], (int)pf[9],
                              (int)pf[10], pf[11], (int)pf[12]};
  int n_obj = 0;
  memcpy(&n_obj, objs, sizeof(int));
  CHECK(n_obj > 0 && n_obj < 4096, "n_obj %d", n_obj);
  dsr_object_in* in = (dsr_object_in*)calloc((size_t)n_obj, sizeof(dsr_object_in));
  size_t off = sizeof(int);
  for (int o = 0; o < n_obj; ++o) {
    int hdr[3];
    memcpy(hdr, objs + off, sizeof hdr);
    off += sizeof hdr;
    memcpy(in[o].t_cam_obj, objs + off, 16 * sizeof(float));
    off += 16 * sizeof(float);
    in[o].pts = (const float*)(objs + off), in[o].n_pts = hdr[0];
    off += (size_t)3 * hdr[0] * sizeof(float);
    in[o].rays = (const float*)(objs + off), in[o].n_rays = hdr[1];
    off += (size_t)3 * hdr[1] * sizeof(float);
    in[o].depth = (const float*)(objs + off), in[o].n_depth = hdr[2];
    off += (size_t)hdr[2] * sizeof(float);
  }
  CHECK(off == ob, "objects.bin size mismatch");
  /* DSR_STRESS_MINIMAL=1: context + decoder + inputs only (what the runtime itself keeps) */
  const char* minimal = getenv("DSR_STRESS_MINIMAL");
  if (minimal && minimal[0] == '1') {
    CHECK(dsr_decoder_free(ctx, dec) == 0, "decoder_free");
    CHECK(dsr_ctx_destroy(ctx) == 0, "ctx_destroy");
    free(w); free(pf); free(objs); free(in);
    printf("stress ok (minimal): %d checks\n", n_checks);
    return 0;
  }
  const size_t osz = sizeof(dsr_object_out) * (size_t)n_obj;
  dsr_object_out* ref = (dsr_object_out*)calloc((size_t)n_obj, sizeof(dsr_object_out));
  dsr_object_out* out = (dsr_object_out*)calloc((size_t)n_obj, sizeof(dsr_object_out));

  /* one-shot batch, twice: deterministic */
  CHECK(dsr_reconstruct_batch(ctx, dec, &p, n_obj, in, ref, NULL) == 0, "%s", dsr_last_error(ctx));
  CHECK(dsr_reconstruct_batch(ctx, dec, &p, n_obj, in, out, NULL) == 0, "%s", dsr_last_error(ctx));
  CHECK(same_out(ref, out, n_obj), "one-shot batch not deterministic");
  int good = 0;
  for (int o = 0; o < n_obj; ++o) good += ref[o].is_good;
  CHECK(good > 0, "no object converged");

  /* per-object traces of the first object (caller-allocated arrays) */
  if (run_section("trace")) {
    const int it = p.num_iterations > 0 ? p.num_iterations : 1;
    dsr_trace* tr = (dsr_trace*)calloc((size_t)n_obj, sizeof(dsr_trace));
    float* H = (float*)calloc((size_t)it * 71 * 71, sizeof(float));
    float* b = (float*)calloc((size_t)it * 71, sizeof(float));
    float* dx = (float*)calloc((size_t)it * 71, sizeof(float));
    float* f3 = (float*)calloc((size_t)it * 3, sizeof(float));
    int* i2 = (int*)calloc((size_t)it * 2, sizeof(int));
    float* t = (float*)calloc((size_t)it * 16, sizeof(float));
    float* z = (float*)calloc((size_t)it * 64, sizeof(float));
    tr[0] = (dsr_trace){H, b, dx, f3, f3 + it, f3 + 2 * it, i2, i2 + it, t, z};
    CHECK(dsr_reconstruct_batch(ctx, dec, &p, n_obj, in, out, tr) == 0, "%s", dsr_last_error(ctx));
    CHECK(same_out(ref, out, n_obj), "traced batch differs");
    if (ref[0].iters_done > 0) CHECK(i2[0] > 0 && isfinite(H[0]), "empty trace");
    free(tr); free(H); free(b); free(dx); free(f3); free(i2); free(t); free(z);
  }

  /* resident batch: run / query / download / stats / diag, re-run, pooled re-create */
  for (int round = 0; round < 2 && run_section("resident"); ++round) {
    dsr_batch* bt = NULL;
    CHECK(dsr_batch_create(ctx, dec, &p, n_obj, in, &bt) == 0, "%s", dsr_last_error(ctx));
    for (int r = 0; r < 3; ++r) {
      memset(out, 0, osz);
      CHECK(dsr_batch_run(bt) == 0, "%s", dsr_last_error(ctx));
      int q, polls = 0;
      while ((q = dsr_batch_query(bt)) == 0) ++polls;
      CHECK(q == 1, "query %d", q);
      CHECK(dsr_batch_download(bt, out) == 0, "%s", dsr_last_error(ctx));
      CHECK(same_out(ref, out, n_obj), "resident run %d.%d differs (%d polls)", round, r, polls);
      dsr_stats st;
      CHECK(dsr_batch_stats(bt, &st) == 0, "%s", dsr_last_error(ctx));
      CHECK(st.fwd_points > 0 && st.lite_broken_blocks == 0 && st.test_hooks == 0, "stats");
      int rec[32];
      CHECK(dsr_batch_lite_diag(bt, rec, 32) >= 0, "%s", dsr_last_error(ctx));
      CHECK(rec[0] == 0, "broken blocks %d", rec[0]);
    }
    CHECK(dsr_batch_sync(bt) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_batch_destroy(bt) == 0, "destroy");
  }

  /* audit violations forced through the test hooks (read at batch creation): every run
     discards iterations and redoes them in the spare iteration, enqueued by dsr_batch_query
     (first run) or by the download (second run) */
  if (run_section("redo")) {
    setenv("DSR_TEST_HOOKS", "1", 1);
    setenv("DSR_LITE_PERTURB", "0.015", 1);
    dsr_batch* bt = NULL;
    CHECK(dsr_batch_create(ctx, dec, &p, n_obj, in, &bt) == 0, "%s", dsr_last_error(ctx));
    unsetenv("DSR_TEST_HOOKS");
    unsetenv("DSR_LITE_PERTURB");
    for (int r = 0; r < 2; ++r) {
      memset(out, 0, osz);
      CHECK(dsr_batch_run(bt) == 0, "%s", dsr_last_error(ctx));
      int q = 0;
      if (r == 0)
        while ((q = dsr_batch_query(bt)) == 0) {}
      CHECK(q >= 0, "query %d", q);
      CHECK(dsr_batch_download(bt, out) == 0, "%s", dsr_last_error(ctx));
      dsr_stats st;
      CHECK(dsr_batch_stats(bt, &st) == 0, "%s", dsr_last_error(ctx));
      CHECK(st.test_hooks == 1 && st.lite_redo_objects > 0, "hooks %d redo %d", st.test_hooks, st.lite_redo_objects);
      for (int o = 0; o < n_obj; ++o)
        CHECK(!out[o].is_good || out[o].iters_done == p.num_iterations, "object %d: %d iterations", o,
              out[o].iters_done);
    }
    CHECK(dsr_batch_destroy(bt) == 0, "destroy");
  }

  /* fixed-capacity batch (keyframe stream): refilled fills, eager and as one replayed graph;
     the same objects in reverse slot order come back reversed, bitwise */
  if (run_section("capacity")) {
    dsr_decoder_info di;
    CHECK(dsr_decoder_info_get(dec, &di) == 0 && di.lite_eligible == 1 && di.probe_points == 65536,
          "decoder info: eligible %d ratio %g", di.lite_eligible, di.lite_probe_ratio);
    int mp = 0, mr = 0;
    for (int o = 0; o < n_obj; ++o) {
      mp = in[o].n_pts > mp ? in[o].n_pts : mp;
      mr = in[o].n_rays > mr ? in[o].n_rays : mr;
    }
    dsr_object_in* rev = (dsr_object_in*)calloc((size_t)n_obj, sizeof(dsr_object_in));
    for (int o = 0; o < n_obj; ++o) rev[o] = in[n_obj - 1 - o];
    /* (the graph-captured variant counts as part of the "graph" section: HIP keeps memory after
       a capture, which the differential leak test leaves out) */
    const int max_flags = run_section("graph") ? DSR_BATCH_GRAPH : 0;
    for (int flags = 0; flags <= max_flags; ++flags) {
      dsr_batch* bt = NULL;
      CHECK(dsr_batch_create_capacity(ctx, dec, &p, n_obj, mp, mr, flags, &bt) == 0, "%s", dsr_last_error(ctx));
      CHECK(dsr_batch_run(bt) < 0, "run of an empty capacity batch accepted");
      CHECK(dsr_batch_refill(bt, n_obj + 1, in) < 0, "refill beyond the object capacity accepted");
      for (int r = 0; r < 4; ++r) {
        const int back = r & 1;
        CHECK(dsr_batch_refill(bt, n_obj, back ? rev : in) == 0, "%s", dsr_last_error(ctx));
        memset(out, 0, osz);
        CHECK(dsr_batch_run(bt) == 0, "%s", dsr_last_error(ctx));
        CHECK(dsr_batch_download(bt, out) == 0, "%s", dsr_last_error(ctx));
        for (int o = 0; o < n_obj; ++o)
          CHECK(same_out(&ref[o], &out[back ? n_obj - 1 - o : o], 1), "capacity fill %d (flags %d) object %d", r,
                flags, o);
      }
      dsr_stats st;
      CHECK(dsr_batch_stats(bt, &st) == 0, "%s", dsr_last_error(ctx));
      CHECK(st.graph_captures == (flags ? 1 : 0) && st.graph_replays == (flags ? 4 : 0), "captures %d replays %d",
            st.graph_captures, st.graph_replays);
      CHECK(dsr_batch_destroy(bt) == 0, "destroy");
    }
    dsr_batch* bt = NULL;
    CHECK(dsr_batch_create(ctx, dec, &p, n_obj, in, &bt) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_batch_refill(bt, n_obj, in) < 0, "refill of an ordinary batch accepted");
    CHECK(dsr_batch_destroy(bt) == 0, "destroy");
    free(rev);
  }

  /* LiDAR ingest: the device kernels against the hand-computed scene, and a capacity batch
     refilled from the sweep against the same batch refilled from the host rule's arrays */
  if (run_section("lidar")) {
    lidar_scene s;
    lidar_scene_make(&s);
    float hp[2][9], hr[2][3 * 203], hz[2][3], dp[2][9], dr[2][3 * 203], dz[2][3];
    dsr_lidar_det_out ho[2], dv[2];
    dsr_lidar_det dets[3] = {s.det, s.det, s.det};  /* (the third only for the call with n_det 3 below) */
    dets[1].trans[0] = -8.f;                        /* behind the camera: an empty object */
    memset(hp, 0, sizeof hp), memset(hr, 0, sizeof hr), memset(hz, 0, sizeof hz);
    memset(dp, 0, sizeof dp), memset(dr, 0, sizeof dr), memset(dz, 0, sizeof dz);
    CHECK(dsr_lidar_inputs_host(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 2, dets, &hp[0][0],
                                &hr[0][0], &hz[0][0], ho) == 0, "lidar_inputs_host failed");
    CHECK(dsr_lidar_inputs(ctx, &s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 2, dets, &dp[0][0],
                           &dr[0][0], &dz[0][0], dv) == 0, "%s", dsr_last_error(ctx));
    lidar_scene_check(dp[0], dr[0], dz[0], &dv[0]);
    CHECK(dv[1].status == DSR_LIDAR_BEHIND && dv[1].n_crop == 0 && dv[1].n_bg == 0, "lidar: behind %d", dv[1].status);
    CHECK(memcmp(ho, dv, sizeof ho) == 0 && memcmp(hp[0], dp[0], sizeof hp[0]) == 0 && memcmp(hr, dr, sizeof hr) == 0 &&
              memcmp(hz[0], dz[0], sizeof hz[0]) == 0, "lidar: device differs from host");
    CHECK(dsr_lidar_inputs(ctx, &s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 2, s.inst, 2, s.masks, 2, dets, &dp[0][0],
                           &dr[0][0], &dz[0][0], dv) < 0 && strlen(dsr_last_error(ctx)) > 0, "lidar: stride 2 accepted");
    dsr_batch* bt = NULL;
    dsr_object_out lo[2], fo[2];
    CHECK(dsr_batch_create_capacity(ctx, dec, &p, 2, 8, 256, 0, &bt) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_batch_lidar_info(bt, dv) < 0, "lidar_info before a sweep refill accepted");
    s.par.max_pts = 9;
    CHECK(dsr_batch_refill_lidar(bt, &s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 2, dets) < 0,
          "refill_lidar beyond max_pts accepted");
    s.par.max_pts = 3;
    CHECK(dsr_batch_refill_lidar(bt, &s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 3, dets) < 0,
          "refill_lidar beyond the object capacity accepted");
    CHECK(dsr_batch_refill_lidar(bt, &s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 2, dets) == 0, "%s",
          dsr_last_error(ctx));
    CHECK(dsr_batch_run(bt) == 0 && dsr_batch_download(bt, lo) == 0, "%s", dsr_last_error(ctx));
    memset(dv, 0, sizeof dv);
    CHECK(dsr_batch_lidar_info(bt, dv) == 0 && memcmp(ho, dv, sizeof ho) == 0, "lidar: batch records differ");
    dsr_object_in fin[2];
    memset(fin, 0, sizeof fin);
    for (int d = 0; d < 2; ++d) {
      const int ok = ho[d].status == DSR_LIDAR_OK;
      memcpy(fin[d].t_cam_obj, ho[d].t_cam_obj, sizeof fin[d].t_cam_obj);
      fin[d].pts = hp[d], fin[d].n_pts = ok ? ho[d].n_pts : 0;
      fin[d].rays = hr[d], fin[d].n_rays = ok ? ho[d].n_pts + ho[d].n_bg : 0;
      fin[d].depth = hz[d], fin[d].n_depth = ok ? ho[d].n_pts : 0;
    }
    CHECK(dsr_batch_refill(bt, 2, fin) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_batch_lidar_info(bt, dv) < 0, "lidar_info after a plain refill accepted");
    CHECK(dsr_batch_run(bt) == 0 && dsr_batch_download(bt, fo) == 0, "%s", dsr_last_error(ctx));
    CHECK(same_out(lo, fo, 2), "lidar: sweep refill differs from the host arrays' refill");
    CHECK(!lo[1].is_good, "lidar: an empty object converged");
    CHECK(dsr_batch_destroy(bt) == 0, "destroy");
  }

  /* resident tracker: a sweep call and a host-row call against dsr_pose_only_batch on the host
     rule's rows, 6 pose-only iterations (the iteration-4 filter runs) */
  if (run_section("track")) {
    lidar_scene s;
    lidar_scene_make(&s);
    s.par.max_pts = 5;
    s.par.max_bg = 0;
    float code[64] = {0.f};
    dsr_lidar_det dets[2] = {s.det, s.det};
    dets[0].code = dets[1].code = code;
    dets[1].trans[0] = -8.f;                        /* its box holds no sweep point */
    float hp[2][15], hr[2][15], hz[2][5], tse3[2][16], dscale[2], want[2][16], got[2][16];
    dsr_lidar_det_out ho[2];
    dsr_track_out recs[2];
    memset(hp, 0, sizeof hp), memset(hr, 0, sizeof hr), memset(hz, 0, sizeof hz);
    CHECK(dsr_lidar_inputs_host(&s.cam, &s.par, s.tcv, &s.velo[0][0], 10, 4, s.inst, 2, s.masks, 2, dets, &hp[0][0],
                                &hr[0][0], &hz[0][0], ho) == 0, "lidar_inputs_host failed");
    CHECK(dsr_lidar_track_prep_host(&s.par, s.tcv, 2, dets, &tse3[0][0], dscale) == 0, "lidar_track_prep_host failed");
    dsr_optim_params q = p;
    q.pose_only_iterations = 6;
    dsr_pose_in pin[3];
    dsr_track_det pri[2];
    memset(pri, 0, sizeof pri);
    for (int d = 0; d < 2; ++d) {
      memcpy(pin[d].t_co_se3, tse3[d], sizeof tse3[d]);
      pin[d].scale = pri[d].scale = dscale[d];
      pin[d].pts = hp[d], pin[d].n_pts = ho[d].n_pts, pin[d].code = code;
    }
    pin[2] = pin[0];
    CHECK(dsr_pose_only_batch(ctx, dec, &q, 2, pin, &want[0][0]) == 0, "%s", dsr_last_error(ctx));
    dsr_tracker* tr = NULL;
    CHECK(dsr_tracker_create(ctx, dec, &q, 2, 8, &tr) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_tracker_query(tr) < 0 && dsr_tracker_download(tr, &got[0][0], recs) < 0, "tracker: results before a call");
    CHECK(dsr_tracker_track_lidar(tr, &s.par, s.tcv, &s.velo[0][0], 10, 4, 2, dets, pri) == 0, "%s", dsr_last_error(ctx));
    int fin = 0;
    while ((fin = dsr_tracker_query(tr)) == 0) {}
    CHECK(fin == 1, "tracker_query %d: %s", fin, dsr_last_error(ctx));
    CHECK(dsr_tracker_download(tr, &got[0][0], recs) == 0, "%s", dsr_last_error(ctx));
    CHECK(memcmp(want, got, sizeof want) == 0, "tracker: sweep call differs from pose_only_batch");
    CHECK(recs[0].n_near == 8 && recs[0].n_crop == 5 && recs[0].n_pts == 5 && recs[0].n_inliers <= 5 &&
              recs[1].status == DSR_TRACK_NO_POINTS && recs[1].n_crop == 0 && got[1][0] != got[1][0],
          "tracker records %d %d %d %d", recs[0].n_near, recs[0].n_crop, recs[0].n_pts, recs[1].status);
    memset(got, 0, sizeof got);
    CHECK(dsr_tracker_track(tr, 2, pin) == 0 && dsr_tracker_download(tr, &got[0][0], NULL) == 0, "%s", dsr_last_error(ctx));
    CHECK(memcmp(want, got, sizeof want) == 0, "tracker: host rows differ from pose_only_batch");
    CHECK(dsr_tracker_track(tr, 3, pin) < 0 && dsr_tracker_track(tr, 0, pin) < 0, "tracker: n_obj outside 1 .. max_obj accepted");
    s.par.max_pts = 9;
    CHECK(dsr_tracker_track_lidar(tr, &s.par, s.tcv, &s.velo[0][0], 10, 4, 2, dets, pri) < 0, "tracker: max_pts 9 > 8 accepted");
    s.par.max_pts = 5;
    pri[1].scale = 0.f;
    CHECK(dsr_tracker_track_lidar(tr, &s.par, s.tcv, &s.velo[0][0], 10, 4, 2, dets, pri) < 0 &&
              strlen(dsr_last_error(ctx)) > 0, "tracker: scale 0 accepted");
    CHECK(dsr_tracker_track(tr, 1, pin) == 0 && dsr_tracker_download(tr, &got[0][0], NULL) == 0, "%s", dsr_last_error(ctx));
    CHECK(memcmp(want[0], got[0], sizeof want[0]) == 0, "tracker: wrong bits after refused calls");
    /* the same handle from a depth image: the 135 pixels of label 7 at z = 8 + u / 100, sub-sampled
       to 8 rows, and an absent label, against dsr_pose_only_batch on the host rule's rows */
    {
      static float depth[24 * 32];
      for (int v = 0; v < 24; ++v)
        for (int u = 0; u < 32; ++u) depth[v * 32 + u] = 8.f + 0.01f * (float)u;
      dsr_frame_params fp;
      CHECK(dsr_frame_params_default(&fp) == 0, "frame_params_default");
      fp.max_pts = 8, fp.max_bg = 0, fp.min_mask_area = 100;
      dsr_frame_det fd[2];
      memset(fd, 0, sizeof fd);
      fd[0].label = 7, fd[1].label = 9;
      fd[0].bbox[2] = fd[1].bbox[2] = -1;
      fd[0].code = fd[1].code = code;
      float fpts[2][24], frays[2][24], fz[2][8];
      dsr_frame_det_out fo[2];
      memset(fpts, 0, sizeof fpts);
      CHECK(dsr_frame_inputs_host(&s.cam, &fp, depth, s.inst, 2, fd, &fpts[0][0], &frays[0][0], &fz[0][0], fo) == 0,
            "frame_inputs_host failed");
      for (int d = 0; d < 2; ++d) {
        memcpy(pin[d].t_co_se3, tse3[0], sizeof tse3[0]);
        memcpy(pri[d].t_co_se3, tse3[0], sizeof tse3[0]);
        pin[d].scale = pri[d].scale = dscale[0];
        pri[d].pose_given = 1;
        pin[d].pts = fpts[d], pin[d].n_pts = fo[d].n_pts;
      }
      CHECK(dsr_pose_only_batch(ctx, dec, &q, 2, pin, &want[0][0]) == 0, "%s", dsr_last_error(ctx));
      memset(got, 0, sizeof got);
      CHECK(dsr_tracker_track_frame(tr, &s.cam, &fp, depth, s.inst, 2, fd, pri) == 0, "%s", dsr_last_error(ctx));
      CHECK(dsr_tracker_download(tr, &got[0][0], recs) == 0, "%s", dsr_last_error(ctx));
      CHECK(memcmp(want, got, sizeof want) == 0, "tracker: frame call differs from pose_only_batch");
      CHECK(recs[0].n_near == 135 && recs[0].n_crop == 135 && recs[0].n_pts == 8 && recs[0].n_inliers <= 8 &&
                recs[1].status == DSR_TRACK_NO_POINTS && recs[1].n_near == 0 && got[1][0] != got[1][0],
            "tracker frame records %d %d %d %d", recs[0].n_near, recs[0].n_crop, recs[0].n_pts, recs[1].status);
      pri[1].pose_given = 0;
      CHECK(dsr_tracker_track_frame(tr, &s.cam, &fp, depth, s.inst, 2, fd, pri) < 0 && strlen(dsr_last_error(ctx)) > 0,
            "tracker: a frame call without a start pose accepted");
      pri[1].pose_given = 1;
      fp.max_pts = 9;
      CHECK(dsr_tracker_track_frame(tr, &s.cam, &fp, depth, s.inst, 2, fd, pri) < 0, "tracker: frame max_pts 9 > 8 accepted");
      fd[1].code = NULL;
      fp.max_pts = 8;
      CHECK(dsr_tracker_track_frame(tr, &s.cam, &fp, depth, s.inst, 2, fd, pri) < 0, "tracker: a frame call with a NULL code accepted");
      CHECK(dsr_tracker_track_frame(tr, &s.cam, &fp, depth, s.inst, 1, fd, pri) == 0 &&
                dsr_tracker_download(tr, &got[0][0], NULL) == 0, "%s", dsr_last_error(ctx));
      CHECK(memcmp(want[0], got[0], sizeof want[0]) == 0, "tracker: wrong bits after refused frame calls");
    }
    CHECK(dsr_tracker_destroy(tr) == 0, "tracker_destroy");
  }

  /* graph capture and replays */
  setenv("DSR_GRAPH", "1", 1);
  if (run_section("graph")) {
    dsr_batch* bt = NULL;
    CHECK(dsr_batch_create(ctx, dec, &p, n_obj, in, &bt) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_batch_graph(bt) == 0, "%s", dsr_last_error(ctx));
    for (int r = 0; r < 4; ++r) {
      memset(out, 0, osz);
      CHECK(dsr_batch_run(bt) == 0, "%s", dsr_last_error(ctx));
      CHECK(dsr_batch_download(bt, out) == 0, "%s", dsr_last_error(ctx));
      CHECK(same_out(ref, out, n_obj), "graph replay %d differs", r);
    }
    CHECK(dsr_batch_destroy(bt) == 0, "destroy");
  }
  unsetenv("DSR_GRAPH");

  /* two contexts on this device through the multi-device entry point */
  if (run_section("multi")) {
    dsr_ctx* c2 = NULL;
    dsr_decoder* d2 = NULL;
    CHECK(dsr_ctx_create(0, &c2) == 0, "second context");
    CHECK(dsr_decoder_load(c2, &DESC, w, nw, &d2) == 0, "%s", dsr_last_error(c2));
    dsr_ctx* cs[2] = {ctx, c2};
    const dsr_decoder* ds[2] = {dec, d2};
    memset(out, 0, osz);
    CHECK(dsr_reconstruct_multi(cs, ds, 2, &p, n_obj, in, out) == 0, "%s", dsr_last_error(ctx));
    CHECK(same_out(ref, out, n_obj), "reconstruct_multi differs");
    CHECK(dsr_decoder_free(c2, d2) == 0, "decoder_free");
    CHECK(dsr_ctx_destroy(c2) == 0, "ctx_destroy");
  }

  /* decoder queries: sdf with and without the Jacobian, at the first object's code */
  if (run_section("query")) {
    const int n = 1000;
    float* x = (float*)malloc(sizeof(float) * 3 * n);
    float* s0 = (float*)malloc(sizeof(float) * n);
    float* s1 = (float*)malloc(sizeof(float) * n);
    float* J = (float*)malloc(sizeof(float) * (size_t)n * 67);
    unsigned r = 12345u;
    for (int i = 0; i < 3 * n; ++i) {
      r = r * 1664525u + 1013904223u;
      x[i] = ((float)(r >> 8) / 16777216.f) * 1.8f - 0.9f;
    }
    CHECK(dsr_sdf_eval(ctx, dec, ref[0].code, x, n, s0, NULL) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_sdf_eval(ctx, dec, ref[0].code, x, n, s1, J) == 0, "%s", dsr_last_error(ctx));
    for (int i = 0; i < n; ++i) CHECK(isfinite(s0[i]) && fabsf(s0[i] - s1[i]) <= 2e-6f, "sdf %d", i);
    for (int i = 0; i < n * 67; ++i) CHECK(isfinite(J[i]), "jac %d", i);
    CHECK(dsr_sdf_eval(ctx, dec, NULL, x, n, s0, NULL) < 0, "NULL code accepted");
    CHECK(dsr_sdf_eval(ctx, dec, ref[0].code, x, 0, NULL, NULL) == 0, "n = 0: %s", dsr_last_error(ctx));

    /* pose-only: single vs batch; an empty object gives NaN in its slot only */
    float T1[16], Tb[3 * 16];
    const float* z = ref[0].code;
    float Tse3[16];
    memcpy(Tse3, in[0].t_cam_obj, sizeof Tse3);
    float sc = cbrtf(Tse3[0] * (Tse3[5] * Tse3[10] - Tse3[6] * Tse3[9]) - Tse3[1] * (Tse3[4] * Tse3[10] - Tse3[6] * Tse3[8]) +
                     Tse3[2] * (Tse3[4] * Tse3[9] - Tse3[5] * Tse3[8]));
    for (int rr = 0; rr < 3; ++rr)
      for (int cc = 0; cc < 3; ++cc) Tse3[4 * rr + cc] /= sc;
    CHECK(dsr_pose_only(ctx, dec, &p, Tse3, sc, in[0].pts, in[0].n_pts, z, T1) == 0, "%s", dsr_last_error(ctx));
    dsr_pose_in pin[3];
    for (int k = 0; k < 3; ++k) {
      memcpy(pin[k].t_co_se3, Tse3, sizeof Tse3);
      pin[k].scale = sc;
      pin[k].pts = in[0].pts;
      pin[k].n_pts = k == 1 ? 0 : in[0].n_pts;
      pin[k].code = z;
    }
    CHECK(dsr_pose_only_batch(ctx, dec, &p, 3, pin, Tb) == 0, "%s", dsr_last_error(ctx));
    CHECK(memcmp(T1, Tb, sizeof T1) == 0 && memcmp(T1, Tb + 32, sizeof T1) == 0, "pose batch != single");
    CHECK(isnan(Tb[16]), "empty object not NaN");
    free(x); free(s0); free(s1); free(J);
  }

  /* scene queries: an identity-pose object is dsr_sdf_eval bitwise; a second, scale-2 object
     shifted by 1.5 shares the call; too many points / objects, a query before set_objects, a peek
     with too small a capacity and one outside the query are refused */
  if (run_section("scene")) {
    const int n = 500;
    float* x = (float*)malloc(sizeof(float) * 3 * n);
    float* s0 = (float*)malloc(sizeof(float) * n);
    float* dist = (float*)malloc(sizeof(float) * n);
    float* g = (float*)malloc(sizeof(float) * 3 * n);
    float* pf = (float*)malloc(sizeof(float) * n);
    float* px = (float*)malloc(sizeof(float) * 3 * n);
    int* who = (int*)malloc(sizeof(int) * n);
    int* pidx = (int*)malloc(sizeof(int) * n);
    unsigned r = 777u;
    for (int i = 0; i < n; ++i) {                     /* in the ball of radius 0.9 */
      float q[3], nn;
      do {
        for (int k = 0; k < 3; ++k) {
          r = r * 1664525u + 1013904223u;
          q[k] = ((float)(r >> 8) / 16777216.f) * 1.8f - 0.9f;
        }
        nn = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
      } while (nn >= 0.81f);
      memcpy(x + 3 * i, q, sizeof q);
    }
    dsr_scene* sc = NULL;
    CHECK(dsr_scene_create(ctx, dec, 0, n, &sc) < 0 && sc == NULL, "scene max_obj 0 accepted");
    CHECK(dsr_scene_create(ctx, dec, 2, n, &sc) == 0 && sc != NULL, "%s", dsr_last_error(ctx));
    CHECK(dsr_scene_query(sc, n, x, dist, who, NULL, NULL) < 0, "query before set_objects accepted");
    dsr_scene_object so[3];
    memset(so, 0, sizeof(so));
    for (int k = 0; k < 3; ++k) {
      for (int i = 0; i < 4; ++i) so[k].t_world_obj[i * 5] = 1.f;
      so[k].code = ref[0].code;
    }
    for (int i = 0; i < 3; ++i) so[1].t_world_obj[i * 5] = 2.f;
    so[1].t_world_obj[3] = 1.5f;
    CHECK(dsr_scene_set_objects(sc, 3, so) < 0, "n_obj > max_obj accepted");
    CHECK(dsr_scene_set_objects(sc, 1, so) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_scene_query(sc, n + 1, x, dist, who, NULL, NULL) < 0, "n_pts > max_pts accepted");
    dsr_scene_object_out rec[2];
    CHECK(dsr_scene_query(sc, n, x, dist, who, NULL, rec) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_sdf_eval(ctx, dec, ref[0].code, x, n, s0, NULL) == 0, "%s", dsr_last_error(ctx));
    CHECK(memcmp(dist, s0, sizeof(float) * n) == 0, "identity-pose scene query != sdf_eval");
    CHECK(rec[0].n_in == n && rec[0].n_win == n && rec[0].n_nan == 0, "scene record %d %d", rec[0].n_in, rec[0].n_win);
    for (int i = 0; i < n; ++i) CHECK(who[i] == 0, "obj %d", i);
    CHECK(dsr_scene_set_objects(sc, 2, so) == 0, "%s", dsr_last_error(ctx));
    CHECK(dsr_scene_query(sc, n, x, dist, who, g, rec) == 0, "%s", dsr_last_error(ctx));
    CHECK(rec[0].n_in == n && rec[1].n_in > 0 && rec[1].n_in < n && rec[0].n_win + rec[1].n_win == n, "two-object records");
    for (int i = 0; i < n; ++i) {
      CHECK(who[i] == 0 || who[i] == 1, "obj %d", i);
      CHECK(who[i] == 1 ? dist[i] < s0[i] : dist[i] == s0[i], "dist %d", i);
      CHECK(isfinite(g[3 * i]) && isfinite(g[3 * i + 1]) && isfinite(g[3 * i + 2]), "grad %d", i);
    }
    int cnt = -1;
    CHECK(dsr_scene_peek(sc, 1, 0, NULL, NULL, NULL, &cnt) == -5 && cnt == rec[1].n_in, "peek count %d", cnt);
    CHECK(dsr_scene_peek(sc, 1, n, pidx, px, pf, &cnt) == 0 && cnt == rec[1].n_in, "%s", dsr_last_error(ctx));
    double sum = 0.0;
    for (int j = 0; j < cnt; ++j) {
      CHECK(pidx[j] >= 0 && pidx[j] < n && (j == 0 || pidx[j] > pidx[j - 1]), "peek order %d", j);
      CHECK(px[3 * j] == 0.5f * x[3 * pidx[j]] - 0.75f, "peek x %d", j);
      sum += pf[j];
    }
    CHECK(fabs(sum - rec[1].sum_sdf) <= 1e-9 * cnt, "sum_sdf %g %g", sum, rec[1].sum_sdf);
    CHECK(dsr_scene_peek(sc, 2, n, pidx, px, pf, &cnt) < 0, "peek outside the query accepted");
    dsr_scene_stats sst;
    CHECK(dsr_scene_stats_get(sc, &sst) == 0 && sst.n_obj == 2 && sst.n_pts == n && sst.n_passes == 1 &&
          sst.pairs == 2 * n && sst.decoded == rec[0].n_in + rec[1].n_in && sst.winners == n, "scene stats");
    CHECK(dsr_scene_query(sc, 0, NULL, NULL, NULL, NULL, rec) == 0 && rec[0].n_in == 0, "n_pts 0: %s", dsr_last_error(ctx));
    /* data association on the same two objects: the points as two detections of world rows (250
       and 100 of a stride of 250), the tables recounted from dsr_scene_peek; then a 16 x 12 frame
       against the points form on dsr_frame_inputs_host's rows; the refusals leave the handle usable */
    {
      dsr_assoc_params ap;
      dsr_assoc_params_default(&ap);
      dsr_assoc_out ao[2], bo[2];
      int nr[2] = {250, 100}, tab[12], tab2[12];
      CHECK(dsr_scene_associate_points(sc, &ap, NULL, 2, 250, nr, x, ao, tab) == 0, "%s", dsr_last_error(ctx));
      CHECK(tab[0] == 250 && tab[2] == 100 && ao[0].n_pts == 250 && ao[1].n_pts == 100, "assoc n_in %d %d", tab[0], tab[2]);
      int want[12];
      memset(want, 0, sizeof want);
      for (int o = 0; o < 2; ++o) {
        CHECK(dsr_scene_peek(sc, o, n, pidx, px, pf, &cnt) == 0, "%s", dsr_last_error(ctx));
        for (int j = 0; j < cnt; ++j) {
          const int d = pidx[j] / 250;
          CHECK(d == 0 || (d == 1 && pidx[j] < 350), "assoc: a NaN slot is a candidate (%d)", pidx[j]);
          want[d * 2 + o] += 1;
          want[4 + d * 2 + o] += fabsf(pf[j]) <= ap.inlier_tol;
          want[8 + d * 2 + o] += pf[j] < -ap.inlier_tol;
        }
      }
      CHECK(memcmp(tab, want, sizeof tab) == 0, "assoc tables != the recount over peek");
      CHECK(dsr_assoc_pick_host(&ap, 2, 2, tab, nr, bo) == 0 && memcmp(ao, bo, sizeof ao) == 0, "assoc records != pick_host");
      CHECK(dsr_scene_stats_get(sc, &sst) == 0 && sst.n_pts == 500 && sst.n_passes == 1 &&
            sst.decoded == tab[0] + tab[1] + tab[2] + tab[3], "assoc stats");
      nr[1] = 251;
      CHECK(dsr_scene_associate_points(sc, &ap, NULL, 2, 250, nr, x, ao, tab2) < 0, "n_rows > max_pts accepted");
      nr[1] = 100;
      CHECK(dsr_scene_associate_points(sc, &ap, NULL, 3, 250, nr, x, ao, tab2) < 0, "n_det x max_pts > max_pts accepted");
      CHECK(dsr_scene_associate_points(sc, &ap, NULL, 0, 250, nr, x, ao, tab2) < 0, "n_det 0 accepted");
      CHECK(dsr_scene_associate_points(sc, NULL, NULL, 2, 250, nr, x, ao, tab2) < 0, "null parameters accepted");
      float twc[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
      twc[5] = 1.01f;
      CHECK(dsr_scene_associate_points(sc, &ap, twc, 2, 250, nr, x, ao, tab2) < 0, "a stretched t_world_cam accepted");
      twc[5] = 1.f;
      dsr_assoc_params bad = ap;
      bad.min_pct = 100;
      CHECK(dsr_scene_associate_points(sc, &bad, twc, 2, 250, nr, x, ao, tab2) < 0, "min_pct 100 accepted");
      CHECK(dsr_scene_associate_points(sc, &ap, twc, 2, 250, nr, x, ao, tab2) == 0 && memcmp(tab, tab2, sizeof tab) == 0,
            "assoc after the refusals (identity t_world_cam): %s", dsr_last_error(ctx));
      /* the frame: label 3 fills columns 2..13 of rows 1..10 at depth 0.5 with a hole; label 4 is absent */
      dsr_camera fcam = {16, 12, 16.f, 16.f, 7.5f, 5.5f};
      dsr_frame_params fp;
      dsr_frame_params_default(&fp);
      fp.max_pts = 100; fp.min_mask_area = 10;
      float fdepth[16 * 12];
      int finst[16 * 12];
      for (int v = 0; v < 12; ++v)
        for (int u = 0; u < 16; ++u) {
          const int in = v >= 1 && v <= 10 && u >= 2 && u <= 13;
          finst[v * 16 + u] = in ? 3 : -1;
          fdepth[v * 16 + u] = in && !(u == 7 && v == 5) ? 0.5f + 0.01f * (float)u : 0.f;
        }
      const int labels[2] = {3, 4};
      int ftab[12], ptab[12];                          /* 3 tables x 2 detections x 2 objects */
      CHECK(dsr_scene_associate_frame(sc, &fcam, &fp, &ap, twc, fdepth, finst, 2, labels, ao, ftab) == 0, "%s",
            dsr_last_error(ctx));
      CHECK(ao[0].n_pts == 100 && ao[0].n_mask == 120 && ao[0].n_valid == 119 && ao[0].ingest_status == DSR_FRAME_OK &&
            ao[1].status == DSR_ASSOC_NO_POINTS && ao[1].ingest_status == DSR_FRAME_NO_MASK, "assoc frame records %d %d",
            ao[0].n_pts, ao[1].status);
      CHECK(ftab[0] == 100, "assoc frame: every row lies in the unit object's ball (%d)", ftab[0]);
      dsr_frame_det fd[2];
      memset(fd, 0, sizeof fd);
      fd[0].label = 3; fd[1].label = 4;
      fd[0].bbox[2] = fd[0].bbox[3] = fd[1].bbox[2] = fd[1].bbox[3] = -1;
      float* hp = (float*)calloc(2 * 100 * 3, sizeof(float));
      float* hr = (float*)calloc(2 * 300 * 3, sizeof(float));
      float* hz = (float*)calloc(2 * 100, sizeof(float));
      dsr_frame_det_out fo[2];
      CHECK(dsr_frame_inputs_host(&fcam, &fp, fdepth, finst, 2, fd, hp, hr, hz, fo) == 0, "frame_inputs_host failed");
      int fr[2] = {fo[0].n_pts, fo[1].n_pts};
      CHECK(dsr_scene_associate_points(sc, &ap, twc, 2, 100, fr, hp, bo, ptab) == 0, "%s", dsr_last_error(ctx));
      CHECK(memcmp(ftab, ptab, sizeof ftab) == 0, "assoc frame tables != the points form on the host rows");
      CHECK(ao[0].status == bo[0].status && ao[0].obj == bo[0].obj && ao[0].n_hit == bo[0].n_hit && ao[1].status == bo[1].status,
            "assoc frame records != the points form");
      CHECK(dsr_scene_associate_frame(sc, &fcam, &fp, &ap, NULL, fdepth, finst, 2, labels, ao, ftab) < 0, "null t_world_cam accepted");
      fp.max_pts = 251;
      CHECK(dsr_scene_associate_frame(sc, &fcam, &fp, &ap, twc, fdepth, finst, 2, labels, ao, ftab) < 0, "2 x 251 rows accepted");
      free(hp); free(hr); free(hz);
    }
    CHECK(dsr_scene_destroy(sc) == 0, "scene_destroy");
    free(x); free(s0); free(dist); free(g); free(pf); free(px); free(who); free(pidx);
  }

  /* mesher: a d^3 grid over [-1, 1]^3, ample capacities, then too small ones (-5, counts) */
  if (run_section("mesher")) {
    const int d = 24;
    const size_t nv = (size_t)d * d * d;
    float* grid = (float*)malloc(sizeof(float) * 3 * nv);
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < d; ++j)
        for (int k = 0; k < d; ++k) {
          float* g = grid + 3 * (((size_t)i * d + j) * d + k);
          g[0] = -1.f + 2.f * i / (d - 1), g[1] = -1.f + 2.f * j / (d - 1), g[2] = -1.f + 2.f * k / (d - 1);
        }
    dsr_mesher* m = NULL;
    CHECK(dsr_mesher_create(ctx, dec, grid, d, &m) == 0, "%s", dsr_last_error(ctx));
    const int vcap = 3 * d * d * d, fcap = 5 * (d - 1) * (d - 1) * (d - 1);
    float* V = (float*)malloc(sizeof(float) * 3 * (size_t)vcap);
    int* F = (int*)malloc(sizeof(int) * 3 * (size_t)fcap);
    int nvert = -1, nface = -1, nv2 = -1, nf2 = -1;
    CHECK(dsr_mesher_run(m, ref[0].code, 0.f, V, vcap, F, fcap, &nvert, &nface) == 0, "%s", dsr_last_error(ctx));
    CHECK(nvert > 0 && nface > 0, "empty mesh");
    for (int f = 0; f < 3 * nface; ++f) CHECK(F[f] >= 0 && F[f] < nvert, "face index %d", F[f]);
    CHECK(dsr_mesher_run(m, ref[0].code, 0.f, V, 1, F, 1, &nv2, &nf2) == -5, "small capacity accepted");
    CHECK(nv2 == nvert && nf2 == nface, "counts on -5");
    /* the batch call: three codes (the first and last equal), ample and too-small totals, n = 0 */
    {
      float codes[3 * DSR_CODE_LEN];
      memset(codes, 0, sizeof codes);
      memcpy(codes, ref[0].code, sizeof(float) * DSR_CODE_LEN);
      memcpy(codes + 2 * DSR_CODE_LEN, ref[0].code, sizeof(float) * DSR_CODE_LEN);
      float* VB = (float*)malloc(sizeof(float) * 3 * 3 * (size_t)vcap);
      int* FB = (int*)malloc(sizeof(int) * 3 * 3 * (size_t)fcap);
      int vo[4] = {-1, -1, -1, -1}, fo[4] = {-1, -1, -1, -1}, vo2[4], fo2[4];
      CHECK(dsr_mesher_run_batch(m, 3, codes, 0.f, VB, 3 * vcap, FB, 3 * fcap, vo, fo) == 0, "%s", dsr_last_error(ctx));
      CHECK(vo[0] == 0 && fo[0] == 0 && vo[1] == nvert && fo[1] == nface, "batch offsets %d %d", vo[1], fo[1]);
      CHECK(vo[3] - vo[2] == nvert && fo[3] - fo[2] == nface, "batch counts of the last mesh");
      CHECK(memcmp(VB, V, sizeof(float) * 3 * (size_t)nvert) == 0 && memcmp(FB, F, sizeof(int) * 3 * (size_t)nface) == 0,
            "batch mesh 0 differs from the mesher's");
      CHECK(memcmp(VB + 3 * (size_t)vo[2], V, sizeof(float) * 3 * (size_t)nvert) == 0 &&
            memcmp(FB + 3 * (size_t)fo[2], F, sizeof(int) * 3 * (size_t)nface) == 0, "batch mesh 2 differs");
      dsr_mesher_stats ms;
      CHECK(dsr_mesher_stats_get(m, &ms) == 0 && ms.n_codes == 3 && ms.n_passes == 1 && ms.violations == 0 &&
            ms.redone_codes == 0 && ms.lite_broken_blocks == 0 && ms.exact_tiles <= ms.all_tiles, "mesher stats");
      VB[0] = 12345.f;
      FB[0] = -7;
      CHECK(dsr_mesher_run_batch(m, 3, codes, 0.f, VB, vo[3] - 1, FB, 3 * fcap, vo2, fo2) == -5, "one vertex short accepted");
      CHECK(memcmp(vo, vo2, sizeof vo) == 0 && memcmp(fo, fo2, sizeof fo) == 0, "offsets on -5");
      CHECK(VB[0] == 12345.f && FB[0] == -7, "output written on -5");
      CHECK(dsr_mesher_run_batch(m, 3, codes, 0.f, VB, 3 * vcap, FB, fo[3] - 1, vo2, fo2) == -5, "one face short accepted");
      vo2[0] = fo2[0] = -1;
      CHECK(dsr_mesher_run_batch(m, 0, NULL, 0.f, NULL, 0, NULL, 0, vo2, fo2) == 0 && vo2[0] == 0 && fo2[0] == 0, "n = 0");
      CHECK(dsr_mesher_run_batch(m, -1, codes, 0.f, VB, 1, FB, 1, vo2, fo2) < 0, "n = -1 accepted");
      CHECK(dsr_mesher_run_batch(m, 3, NULL, 0.f, VB, 1, FB, 1, vo2, fo2) < 0, "NULL codes accepted");
      CHECK(dsr_mesher_peek(m, 3, NULL, NULL, NULL) < 0, "peek beyond the last pass accepted");
      free(VB);
      free(FB);
    }
    CHECK(dsr_mesher_destroy(m) == 0, "mesher_destroy");
    /* the same grid decoded by dsr_sdf_eval, meshed by dsr_mc_volume: the mesher's mesh */
    float* vol = (float*)malloc(sizeof(float) * nv);
    float* V2 = (float*)malloc(sizeof(float) * 3 * (size_t)vcap);
    int* F2 = (int*)malloc(sizeof(int) * 3 * (size_t)fcap);
    CHECK(dsr_sdf_eval(ctx, dec, ref[0].code, grid, (int)nv, vol, NULL) == 0, "%s", dsr_last_error(ctx));
    nv2 = nf2 = -1;
    CHECK(dsr_mc_volume(ctx, vol, d, 0.f, V2, vcap, F2, fcap, &nv2, &nf2) == 0, "%s", dsr_last_error(ctx));
    CHECK(nv2 == nvert && nf2 == nface, "mc_volume counts %d/%d vs %d/%d", nv2, nf2, nvert, nface);
    CHECK(memcmp(V, V2, sizeof(float) * 3 * (size_t)nvert) == 0 && memcmp(F, F2, sizeof(int) * 3 * (size_t)nface) == 0,
          "mc_volume mesh differs from the mesher's");
    CHECK(dsr_mc_volume(ctx, vol, d, 0.f, V2, 1, F2, 1, &nv2, &nf2) == -5 && nv2 == nvert, "mc_volume small capacity");
    CHECK(dsr_mc_volume(ctx, NULL, d, 0.f, V2, vcap, F2, fcap, &nv2, &nf2) < 0, "mc_volume without volume");
    CHECK(dsr_mc_volume(ctx, vol, 1, 0.f, V2, vcap, F2, fcap, &nv2, &nf2) < 0, "mc_volume vol_dim 1 accepted");
    free(vol); free(V2); free(F2);
    free(grid); free(V); free(F);
  }

  if (run_section("errors")) live_error_paths(ctx, dec, w, nw, &p, in);
  /* the context still works after its errors */
  memset(out, 0, osz);
  CHECK(dsr_reconstruct_batch(ctx, dec, &p, n_obj, in, out, NULL) == 0, "%s", dsr_last_error(ctx));
  CHECK(same_out(ref, out, n_obj), "batch after error paths differs");

  CHECK(dsr_decoder_free(ctx, dec) == 0, "decoder_free");
  CHECK(dsr_ctx_destroy(ctx) == 0, "ctx_destroy");
  free(w); free(pf); free(objs); free(in); free(ref); free(out);
  printf("stress ok: %d checks, %d objects (%d good)\n", n_checks, n_obj, good);
  /* DSR_STRESS_QUICK_EXIT=1: skip the HIP runtime's static destructors (with host ASan, the
     sanitizer's device-allocator hook trips over the runtime freeing memory after its own
     teardown — at process exit, after every libdsr object here was destroyed) */
  const char* qe = getenv("DSR_STRESS_QUICK_EXIT");
  if (qe && qe[0] == '1') {
    fflush(stdout);
    _exit(0);
  }
  return 0;
}
